"""GPU tests of the attention backward with prefix rows / history states (modcr_qkv_attn_prefix_bwd: the cores of
csrc/attn_bias_bwd.hip behind modcr_hip.qkv_attn_bwd(hist=), hip_layers.layer_forward_train(hist=) / layer_backward,
hip_autograd.BertLayerPrefixFn and trainable_encoders.encoder_layers(encoder_history_states=)), P + S <= 256, bf16 and fp32.

Checker: torch autograd in float64 on the CPU of
    s_ij = q_i.k_j / 8 + bias,  P = softmax_j(s),  P' = P o m / (1 - p),  P'' = hm P',  ctx = P''.V,  keys j over [hist ; x]
-- oracle.self_attention(history_state=) in eval mode, and with dropout the test_hip_attn_bwd.attention formula extended by the
prefix keys (attention_prefix below, which equals the oracle at p = 0 to 1e-12) with the keep mask m of
helpers.attn_drop_keep_torch(keys=L).  The bias enters as a dense float64 [N,A,S,L] leaf, so its gradient is the dense dS the
kernel writes to d_bias.

Bounds (the repository's, from test_hip_attn_bias_bwd): max|got - ref| <= tol x max(1, max|ref|), tol = 2e-2 in bf16 and 1e-3 in
fp32, for ctx, dx, d_hist, dWqkv, dbqkv and d_bias; relative L2 < 2e-2 for dx, d_hist and dWqkv in bf16.  The key-bias slice of
dbqkv is analytically zero and is held as that file holds it.  On the CPU the same formula with q | k | v, P'' and dS rounded to
bf16 and the dq | dk | dv rows leaving in bf16 (tools/attn_prefix_bwd_tolerance.py -> profiles/attn_prefix_bwd_tolerance_report.txt;
the six shapes below, the three bias forms, head mask (1, 0.5), p = 0.2) uses at most 9.4e-3 of scale (47 % of the 2e-2: ctx at
(2, 170, 22) under the [1,A,S,L] bias; the gradients at most 9.2e-3, 46 %: dx at (2, 8, 120)) and 7.5e-3 relative L2 (37 %; dx at
(2, 8, 120)), the key-bias slice 9 % of its bound: less than half of every bound on every input, so inputs and bounds stand.  Layer
level: the bounds of
test_hip_kernels.test_layer_backward_golden as test_hip_attn_bias_bwd quotes them (y 2e-2 / 1e-3; gradients 2.5e-2 in bf16, 1e-3 in
fp32; the analytically zero key-bias gradient 6e-2 of the query-bias scale in bf16).  Two layers (encoder level) in bf16: twice the
one-layer bounds, for the reason given there -- the gradient stream is rounded to bf16 once more per layer; fp32 stays at 1e-3."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import helpers as H
from oracle import modcr_oracle as O
from test_hip_attn_bias import NEG_INF, layer_sd, soft_bias
from test_hip_attn_bias_bwd import G_TOL, MODE_DT, TOL, Y_TOL, Z_TOL, build_body, check_param_grads, head_scale
from test_hip_attn_bwd import check
from test_hip_attn_fullsize import bf16r

pytestmark = pytest.mark.gpu

DT = [torch.bfloat16, torch.float32]
# (n, s, p, h, a): one partial tile, P % 4 != 0 (unaligned bias rows, a dropout group that straddles the prefix boundary); ModCR's
# prefix length; more prefix keys than queries; L = 192, the MFMA core's edge; L = 193, the first bf16 shape on the exact core;
# L = 256, the limit
SHAPES = [(2, 37, 5, 128, 2), (3, 101, 10, 128, 2), (2, 8, 120, 128, 2), (2, 170, 22, 128, 2), (2, 171, 22, 256, 4), (1, 246, 10, 128, 2)]
FORMS = ["[N,A,S,L]", "[N,1,1,L]", "[1,A,S,L]"]
DROP = (0.2, 77, 5 << 32)


@pytest.fixture(scope="module")
def mh():
    import __graft_entry__ as g  # noqa: F401
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import modcr_hip
    modcr_hip.lib()
    return modcr_hip


def mdt(mh, dtype):
    return mh.BF16 if dtype == torch.bfloat16 else mh.F32


@functools.lru_cache(maxsize=None)
def case(n, s, p, h, a):
    """bf16-rounded weights (helpers._lin), inputs, prefix rows and dctx of one shape, shared by every test on it (read-only)"""
    rs = np.random.RandomState(5000 + 13 * n + s + 7 * p + h)
    sd = {}
    for nm in ("query", "key", "value"):
        H._lin(rs, sd, nm, h, h)
    sd = H.to_torch(sd)
    w = bf16r(torch.cat([sd["query.weight"], sd["key.weight"], sd["value.weight"]], 0))
    b = torch.cat([sd["query.bias"], sd["key.bias"], sd["value.bias"]], 0)
    x = bf16r(torch.from_numpy(rs.standard_normal((n, s, h)).astype(np.float32)))
    hist = bf16r(torch.from_numpy(rs.standard_normal((n, p, h)).astype(np.float32)))
    dctx = bf16r(torch.from_numpy(rs.standard_normal((n, s, h)).astype(np.float32)))
    return w, b, x, hist, dctx


def bias_of(form, n, s, p, a, seed):
    """the soft_bias mix (random values, -10000 and -inf, key 0 finite) in one of the three forms, as its OWN shape"""
    l = p + s
    shape = {"[N,A,S,L]": (n, a, s, l), "[N,1,1,L]": (n, 1, 1, l), "[1,A,S,L]": (1, a, s, l)}[form]
    return soft_bias(np.random.RandomState(seed), shape)


def attention_prefix(x, hist, w, b, a, add, keep=None, p=0.0):
    """test_hip_attn_bwd.attention extended by prefix keys: K and V over [hist ; x] (modeling_bert.py:36-44), queries from x"""
    n, s, h = x.shape
    F = torch.nn.functional
    xs = torch.cat([hist, x], 1)
    q, k, v = F.linear(x, w[:h], b[:h]), F.linear(xs, w[h:2 * h], b[h:2 * h]), F.linear(xs, w[2 * h:], b[2 * h:])
    sp = lambda t: t.view(n, t.shape[1], a, 64).transpose(1, 2)
    probs = torch.softmax(sp(q) @ sp(k).transpose(-1, -2) / 8.0 + add, -1)
    if keep is not None:
        probs = probs * keep / (1.0 - p)
    return (probs @ sp(v)).transpose(1, 2).reshape(n, s, h)


def oracle_attention(x, hist, w, b, a, add):
    h = x.shape[2]
    sd = {}
    for i, nm in enumerate(("query", "key", "value")):
        sd[nm + ".weight"], sd[nm + ".bias"] = w[i * h:(i + 1) * h], b[i * h:(i + 1) * h]
    return O.self_attention(x, add, sd, "", a, history_state=hist)[0]


def reference(c, a, bias, hm=None, drop=None, dctx=None, hist=None):
    """float64 autograd on the CPU: (ctx, dx, d_hist, dWqkv, dbqkv, dense dS [N,A,S,L]); oracle.self_attention(history_state=) in
    eval mode, attention_prefix with the host keep mask under dropout"""
    w, b, x, hist0, dctx0 = c
    dctx = dctx0 if dctx is None else dctx
    hist = hist0 if hist is None else hist
    n, s, h = x.shape
    l = hist.shape[1] + s
    xr, hr, wr, br = (t.double().clone().requires_grad_(True) for t in (x, hist, w, b))
    dense = torch.zeros(n, a, s, l, dtype=torch.float64)
    if bias is not None:
        dense = dense + bias.double()
    dense.requires_grad_(True)
    if drop is None:
        ctx = oracle_attention(xr, hr, wr, br, a, dense)
    else:
        p, seed, off = drop
        keep = H.attn_drop_keep_torch(range(n), a, s, p, seed, off, "cpu", keys=l).double()
        ctx = attention_prefix(xr, hr, wr, br, a, dense, keep=keep, p=p)
    if hm is not None:
        ctx = head_scale(ctx, hm, a)
    (ctx * dctx.double()).sum().backward()
    for g in (xr.grad, hr.grad, wr.grad, br.grad, dense.grad):
        assert torch.isfinite(g).all(), "the float64 reference itself is not finite"
    return ctx.detach(), xr.grad, hr.grad, wr.grad, br.grad, dense.grad


@functools.lru_cache(maxsize=None)
def soft_reference(shape, form):
    """the reference of the soft-bias case (head mask (1, 0.5), p = 0.2) of one shape and bias form, shared by both dtypes"""
    n, s, p, h, a = shape
    return reference(case(*shape), a, bias_of(form, n, s, p, a, s + p), torch.linspace(1.0, 0.5, a), DROP)


def run_hip(mh, dtype, c, a, bias=None, hm=None, drop=None, want_d_bias=True, dctx=None, forward=True, key_mask=None):
    """qkv_attn + qkv_attn_bwd(hist=) on the GPU; a bias that already lives there is handed over as it is (views keep their strides)"""
    w, b, x, hist, dctx0 = c
    dctx = dctx0 if dctx is None else dctx
    n, s, h = x.shape
    l = hist.shape[1] + s
    xd, hd, wd, bd = x.to(dtype).cuda(), hist.to(dtype).cuda(), w.to(dtype).cuda(), b.cuda()
    bias_d = None if bias is None else bias.cuda()
    hm_d = None if hm is None else hm.cuda()
    km_d = None if key_mask is None else key_mask.cuda()
    ctx = None
    if forward:
        fb = bias_d if key_mask is None else mh.fold_key_mask(km_d)
        ctx, _ = mh.qkv_attn(xd, wd, bd, hist=hd, num_heads=a, attn_dropout=drop, attn_bias=fb, head_mask=hm_d)
    dw, db = torch.full((3 * h, h), float("nan"), device="cuda"), torch.full((3 * h,), float("nan"), device="cuda")
    d_bias = torch.full((n, a, s, l), float("nan"), device="cuda") if want_d_bias and (bias is not None or key_mask is not None) else None
    dx, d_hist = mh.qkv_attn_bwd(dctx.to(dtype).cuda(), xd, wd, bd, dw, db, num_heads=a, attn_dropout=drop, attn_bias=bias_d,
                                 key_mask=km_d, head_mask=hm_d, d_bias=d_bias, hist=hd)
    torch.cuda.synchronize()
    return ctx, dx, d_hist, dw, db, d_bias


def check_all(dtype, got, ref, what, n, s, h):
    """ctx, dx, d_hist, dWqkv, dbqkv, d_bias against the reference at the file's bounds"""
    tol = TOL[dtype]
    ctx, dx, dh, dw, db, d_bias = got
    ctx_r, dx_r, dh_r, dw_r, db_r, ds_r = ref
    if ctx is not None:
        check(ctx, ctx_r, tol, what + " ctx")
    e_dx = check(dx, dx_r, tol, what + " dx")
    e_dh = check(dh, dh_r, tol, what + " d_hist")
    e_dw = check(dw, dw_r, tol, what + " dwqkv")
    kb = slice(h, 2 * h)            # the key-bias gradient is analytically zero: rounding noise of a sum over the rows on both sides
    dbm, dbr = db.detach().float().cpu().clone(), db_r.float().clone()
    dbm[kb] = 0
    dbr[kb] = 0
    check(dbm, dbr, tol, what + " dbqkv")
    assert torch.isfinite(db).all()
    kb_bound = tol * max(1.0, float(db_r.abs().max())) * (n * s) ** 0.5 * 0.25
    H.report_use(what + " key-bias slice", float(db[kb].abs().max()), kb_bound, kind="max|.|")
    assert float(db[kb].abs().max()) <= kb_bound, what + " key-bias slice"
    if d_bias is not None:
        check(d_bias, ds_r, tol, what + " d_bias")
    if dtype == torch.bfloat16:
        for nm, e in (("dx", e_dx), ("d_hist", e_dh), ("dw", e_dw)):
            H.report_use(what + " %s rel L2" % nm, e[1], 2e-2, kind="relative L2")
        assert e_dx[1] < 2e-2 and e_dh[1] < 2e-2 and e_dw[1] < 2e-2, (what, e_dx, e_dh, e_dw)


def want_core(dtype, l):
    return "mfma" if dtype == torch.bfloat16 and l <= 192 else "exact"


# ---- 1. a soft bias in three forms, head mask, dropout: every shape ----------------------------------------------------------------

@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("shape", SHAPES)
def test_soft_bias_head_mask_dropout(mh, dtype, form, shape):
    """all six quantities against float64; ctx comes from the forward with the same (p, seed, offset), so a backward that draws another
    mask than the forward cannot pass.  The broadcast forms are handed over as expand()ed views (stride 0), never expanded."""
    n, s, p, h, a = shape
    l = p + s
    assert mh.qkv_attn_prefix_bwd_route(n, s, p, h, a, mdt(mh, dtype)) == want_core(dtype, l)
    bias = bias_of(form, n, s, p, a, s + p).cuda()
    view = bias.expand(n, a, s, l)
    assert view.data_ptr() == bias.data_ptr() and all(view.stride(d) == 0 for d in range(3) if bias.shape[d] == 1 and view.shape[d] > 1)
    got = run_hip(mh, dtype, case(*shape), a, bias=view, hm=torch.linspace(1.0, 0.5, a), drop=DROP)
    check_all(dtype, got, soft_reference(shape, form), "%s L=%d" % (form, l), n, s, h)


# ---- 2. a binary key mask over [hist ; x] -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DT)
def test_key_mask_is_folded_on_the_host(mh, dtype):
    """qkv_attn_bwd(hist=, key_mask=[N, L]) equals the explicit 0 / -10000 [N,1,1,L] bias call bit for bit, and the reference"""
    shape = SHAPES[1]
    n, s, p, h, a = shape
    l = p + s
    c = case(*shape)
    km = torch.ones(n, l)
    km[1, 80:] = 0
    km[2, 3:7] = 0                  # prefix keys masked too
    km[2, 40:] = 0
    add = O.extend_mask(km).float()
    assert tuple(add.shape) == (n, 1, 1, l)
    r_mask = run_hip(mh, dtype, c, a, key_mask=km)
    r_bias = run_hip(mh, dtype, c, a, bias=add)
    for t1, t2, nm in zip(r_mask, r_bias, ("ctx", "dx", "d_hist", "dw", "db", "d_bias")):
        assert torch.equal(t1, t2), nm
    check_all(dtype, r_mask, reference(c, a, add), "key mask", n, s, h)


# ---- 3. every output element is written; accumulate; the prefix rows' contribution --------------------------------------------------

def raw_call(mh, dtype, c, a, bias, outs, accumulate=False, n_s_p=None, hist_null=False):
    """the C entry itself on caller-owned outputs (dx, d_hist, dwqkv, dbqkv, d_bias): returns its code"""
    w, b, x, hist, dctx = c
    n, s, h = x.shape
    p = hist.shape[1]
    if n_s_p is not None:
        n, s, p = n_s_p
    dt = mdt(mh, dtype)
    t = [v.to(dtype).cuda() for v in (dctx, x, hist, w)]
    bd, bias_d = b.cuda(), bias.cuda().contiguous()
    dx, dh, dw, db, d_bias = outs
    need = max(mh.lib().modcr_qkv_attn_prefix_bwd_workspace(n, s, max(p, 1), h, dt), 1 << 20)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    sn, sa, sq = [0 if bias_d.shape[d] == 1 else bias_d.stride(d) for d in range(3)]
    ptr = lambda v: ctypes.c_void_p(v.data_ptr())
    rc = mh.lib().modcr_qkv_attn_prefix_bwd(ptr(t[0]), ptr(t[1]), None if hist_null else ptr(t[2]), ptr(t[3]), ptr(bd), ptr(bias_d), sn, sa, sq,
                                            None, 0, None, ptr(dx), ptr(dh), ptr(dw), ptr(db), 1 if accumulate else 0, ptr(d_bias),
                                            n, s, p, h, a, 0.0, 0, 0, ptr(ws), need, dt, None)
    torch.cuda.synchronize()
    return rc


def prefix_value_bias_part(c, a, bias):
    """the prefix rows' share of the value-bias gradient in float64 (eval mode): sum_n sum_i (sum_{j < P} P_ij) dctx_i per head"""
    w, b, x, hist, dctx = (t.double() for t in c)
    n, s, h = x.shape
    p = hist.shape[1]
    sd = {}
    for i, nm in enumerate(("query", "key", "value")):
        sd[nm + ".weight"], sd[nm + ".bias"] = w[i * h:(i + 1) * h], b[i * h:(i + 1) * h]
    probs = O.self_attention(x, bias.double(), sd, "", a, history_state=hist)[1]
    return torch.einsum("nas,nsad->ad", probs[..., :p].sum(-1), dctx.view(n, s, a, 64)).reshape(h)


def nan_outs(dtype, n, s, p, h, a):
    f = lambda *shape, **kw: torch.full(shape, float("nan"), device="cuda", **kw)
    return [f(n, s, h, dtype=dtype), f(n, p, h, dtype=dtype), f(3 * h, h), f(3 * h), f(n, a, s, p + s)]


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[2], SHAPES[4]])
def test_outputs_fully_written_accumulate_and_prefix_contribution(mh, dtype, shape):
    n, s, p, h, a = shape
    c = case(*shape)
    tol = TOL[dtype]
    bias = bias_of("[N,A,S,L]", n, s, p, a, 3)
    ref = reference(c, a, bias)
    outs = nan_outs(dtype, n, s, p, h, a)
    assert raw_call(mh, dtype, c, a, bias, outs) == 0, mh.lib().modcr_last_error()
    for t, nm in zip(outs, ("dx", "d_hist", "dw", "db", "d_bias")):
        assert torch.isfinite(t.float()).all(), nm + ": an element was not written"
    check_all(dtype, [None] + outs, ref, "NaN prefill", n, s, h)
    # accumulate: prefill + gradient
    rs = np.random.RandomState(8)
    pre_w = torch.from_numpy(rs.standard_normal((3 * h, h)).astype(np.float32))
    pre_b = torch.from_numpy(rs.standard_normal((3 * h,)).astype(np.float32))
    acc = nan_outs(dtype, n, s, p, h, a)
    acc[2], acc[3] = pre_w.cuda(), pre_b.cuda()
    assert raw_call(mh, dtype, c, a, bias, acc, accumulate=True) == 0, mh.lib().modcr_last_error()
    scale_w, scale_b = max(1.0, float(ref[3].abs().max())), max(1.0, float(ref[4].abs().max()))
    e_w = float((acc[2].cpu().double() - pre_w.double() - ref[3]).abs().max())
    e_b = (acc[3].cpu().double() - pre_b.double() - ref[4])
    e_b[h:2 * h] = 0                # (the key-bias slice: held in check_all above)
    H.report_use("accumulate dwqkv", e_w / scale_w, tol)
    H.report_use("accumulate dbqkv", float(e_b.abs().max()) / scale_b, tol)
    assert e_w <= tol * scale_w and float(e_b.abs().max()) <= tol * scale_b
    # the prefix rows reach the key / value slices: against a reference whose hist rows are zeroed the same outputs MISS the bound
    ref0 = reference(c, a, bias, hist=torch.zeros_like(c[3]))
    for sl, nm in ((slice(h, 2 * h), "key"), (slice(2 * h, 3 * h), "value")):
        miss = float((outs[2][sl].cpu().double() - ref0[3][sl]).abs().max())
        assert miss > tol * max(1.0, float(ref0[3][sl].abs().max())), "the test would not notice a missing prefix contribution to dW " + nm
    # ... and the value-bias slice: zeroed hist rows still carry their probabilities, so the prefix rows' share is taken from the
    # float64 probabilities instead; outputs that lacked it would miss the reference by it
    part = float(prefix_value_bias_part(c, a, bias).abs().max())
    assert part > tol * scale_b, "the test would not notice a missing prefix contribution to the value bias"


# ---- 4. -inf entries and a pruned head ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[4]])
def test_minus_infinity_and_a_pruned_head(mh, dtype, shape):
    n, s, p, h, a = shape
    c = case(*shape)
    dctx = c[4]
    bias = bias_of("[N,A,S,L]", n, s, p, a, 5)
    bias[1, :, :, 3] = NEG_INF      # a prefix key hidden from every query of sequence 1
    bias[0, 1, 5, :] = NEG_INF      # a query row with every key at -inf
    hm = torch.zeros(a)
    hm[1:] = 1.0                    # head 0 pruned
    got = run_hip(mh, dtype, c, a, bias=bias, hm=hm)
    for t in got:
        assert torch.isfinite(t.float()).all()
    d_hist, d_bias = got[2], got[5]
    assert (d_hist[1, 3] == 0).all(), "a prefix key no query sees has a zero d_hist row"
    assert (d_bias[:, 0] == 0).all(), "the pruned head's d_bias is exactly 0"
    assert (d_bias[0, 1, 5] == 0).all()
    assert (d_bias.cpu()[torch.isinf(bias)] == 0).all(), "a -inf entry has a zero in d_bias"
    # reference: a finite stand-in for the all -inf row with dctx zeroed on its (row, head) columns -- it contributes nothing
    fin, dz = bias.clone(), dctx.clone()
    fin[0, 1, 5, :] = 0
    dz[0, 5, 64:128] = 0
    ref = list(reference(c, a, fin, hm, dctx=dz))
    ref[0][0, 5, 64:128] = 0
    ref[5][0, 1, 5] = 0
    assert float(ref[2][1, 3].abs().max()) == 0.0
    check_all(dtype, got, ref, "-inf + pruned head", n, s, h)


# ---- 5. reproducibility ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,shape", [(torch.bfloat16, SHAPES[0]), (torch.bfloat16, SHAPES[3]), (torch.bfloat16, SHAPES[5]),
                                         (torch.float32, SHAPES[1])])
def test_two_launches_are_bit_identical(mh, dtype, shape):
    n, s, p, h, a = shape
    c = case(*shape)
    bias = bias_of("[N,A,S,L]", n, s, p, a, 2)
    hm = torch.linspace(0.25, 1.0, a)
    r1 = run_hip(mh, dtype, c, a, bias=bias, hm=hm, drop=(0.2, 9, 1 << 20), forward=False)
    r2 = run_hip(mh, dtype, c, a, bias=bias, hm=hm, drop=(0.2, 9, 1 << 20), forward=False)
    for t1, t2, nm in zip(r1[1:], r2[1:], ("dx", "d_hist", "dw", "db", "d_bias")):
        assert torch.equal(t1, t2), nm


# ---- 6. against the code that existed before, independent of the checker -----------------------------------------------------------

@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[2], SHAPES[4]])
def test_agrees_with_the_square_backward_over_concatenated_rows(mh, shape):
    """fp32, p = 0: qkv_attn_bwd(attn_bias=) over [hist ; x] with zero dctx rows for the prefix and P finite padding rows in the
    bias computes the same dx, d_hist (the prefix rows' dx: their dq is zero), dWqkv, dbqkv and, on the query rows, d_bias"""
    dtype = torch.float32
    n, s, p, h, a = shape
    l = p + s
    w, b, x, hist, dctx = c = case(*shape)
    bias = bias_of("[N,A,S,L]", n, s, p, a, 11)
    got = run_hip(mh, dtype, c, a, bias=bias, forward=False)
    xc = torch.cat([hist, x], 1).cuda()
    dc = torch.cat([torch.zeros(n, p, h), dctx], 1).cuda()
    bc = torch.cat([torch.zeros(n, a, p, l), bias], 2).cuda()
    dw, db = torch.full((3 * h, h), float("nan"), device="cuda"), torch.full((3 * h,), float("nan"), device="cuda")
    dbc = torch.full((n, a, l, l), float("nan"), device="cuda")
    dxc = mh.qkv_attn_bwd(dc, xc, w.cuda(), b.cuda(), dw, db, num_heads=a, attn_bias=bc, d_bias=dbc)
    torch.cuda.synchronize()
    tol = 1e-3
    check(got[1], dxc[:, p:], tol, "dx vs square")
    check(got[2], dxc[:, :p], tol, "d_hist vs square")
    check(got[3], dw, tol, "dwqkv vs square")
    check(got[4], db, tol, "dbqkv vs square")
    check(got[5], dbc[:, :, p:], tol, "d_bias vs square")
    assert float(dbc[:, :, :p].abs().max()) == 0.0


# ---- 7. refusals: nothing is launched -----------------------------------------------------------------------------------------------

def test_refusals(mh):
    dtype, h, a = torch.bfloat16, 128, 2
    rs = np.random.RandomState(4)
    z = lambda *shape: torch.from_numpy(rs.standard_normal(shape).astype(np.float32))
    w, b = z(3 * h, h), z(3 * h)
    with pytest.raises(ValueError, match="256"):
        run_hip(mh, dtype, (w, b, z(1, 247, h), z(1, 10, h), z(1, 247, h)), a, bias=torch.zeros(1, 1, 1, 257), forward=False)
    # ... and from C: MODCR_ERR_UNSUPPORTED, the outputs keep their NaN prefill
    c257 = (w, b, z(1, 247, h), z(1, 10, h), z(1, 247, h))
    outs = nan_outs(dtype, 1, 247, 10, h, a)
    assert raw_call(mh, dtype, c257, a, torch.zeros(1, 1, 1, 257), outs) == -3
    assert b"256" in mh.lib().modcr_last_error()
    assert all(torch.isnan(t.float()).all() for t in outs)
    # P = 0 / no hist through the C entry: MODCR_ERR_INVALID naming the entry without prefix rows
    c = (w, b, z(1, 100, h), z(1, 10, h), z(1, 100, h))
    for kw in (dict(n_s_p=(1, 100, 0)), dict(hist_null=True)):
        outs = nan_outs(dtype, 1, 100, 10, h, a)
        assert raw_call(mh, dtype, c, a, torch.zeros(1, 1, 1, 110), outs, **kw) == -1
        assert b"modcr_qkv_attn_bias_bwd" in mh.lib().modcr_last_error()
        assert all(torch.isnan(t.float()).all() for t in outs)

    x, hist = c[2].to(dtype).cuda(), c[3].to(dtype).cuda()
    dw, db = torch.full((3 * h, h), float("nan"), device="cuda"), torch.full((3 * h,), float("nan"), device="cuda")
    bias = torch.zeros(1, 1, 1, 110).cuda()

    def bwd(**kw):
        return mh.qkv_attn_bwd(x, x, w.to(dtype).cuda(), b.cuda(), dw, db, num_heads=a, hist=hist, **kw)
    with pytest.raises(ValueError, match="lse"):
        bwd(attn_bias=bias, ctx=x, lse=torch.empty(1, a, 100, device="cuda"))
    with pytest.raises(ValueError, match="d_align"):
        bwd(attn_bias=bias, d_align=torch.zeros(1, 40, 60).cuda(), align_t=40)
    with pytest.raises(ValueError, match="chunk_id"):
        bwd(attn_bias=bias, chunk_id=torch.zeros(1, 40, dtype=torch.int32).cuda())
    with pytest.raises(ValueError, match="d_bias"):
        bwd(attn_bias=bias, d_bias=torch.empty(1, a, 100, 100, device="cuda"))
    torch.cuda.synchronize()
    assert torch.isnan(dw).all() and torch.isnan(db).all()


# ---- 8. layer level: hip_layers.layer_forward_train(hist=) + layer_backward --------------------------------------------------------

def layer64p(x, hist, add, sd, prefix, a, hm, keeps=None, p=0.0, akeep=None):
    """oracle.bert_layer(history_state=) with the head scale between its attention and its output blocks and, in training mode, the
    host keep masks of the attention dropout (akeep) and of the two hidden dropouts (keeps): float64, differentiable"""
    F = torch.nn.functional
    n, s, h = x.shape
    pa = prefix + "attention.self."
    if akeep is None:
        ctx, _ = O.self_attention(x, add, sd, pa, a, history_state=hist)
    else:
        w = torch.cat([sd[pa + nm + ".weight"] for nm in ("query", "key", "value")], 0)
        b = torch.cat([sd[pa + nm + ".bias"] for nm in ("query", "key", "value")], 0)
        ctx = attention_prefix(x, hist, w, b, a, add, keep=akeep, p=p)
    if hm is not None:
        ctx = head_scale(ctx, hm, a)
    t = F.linear(ctx, sd[prefix + "attention.output.dense.weight"], sd[prefix + "attention.output.dense.bias"])
    if keeps is not None:
        t = t * keeps[0] / (1.0 - p)
    att = F.layer_norm(t + x, (h,), sd[prefix + "attention.output.LayerNorm.weight"], sd[prefix + "attention.output.LayerNorm.bias"], 1e-12)
    inter = F.gelu(F.linear(att, sd[prefix + "intermediate.dense.weight"], sd[prefix + "intermediate.dense.bias"]))
    t = F.linear(inter, sd[prefix + "output.dense.weight"], sd[prefix + "output.dense.bias"])
    if keeps is not None:
        t = t * keeps[1] / (1.0 - p)
    return F.layer_norm(t + att, (h,), sd[prefix + "output.LayerNorm.weight"], sd[prefix + "output.LayerNorm.bias"], 1e-12)


@pytest.mark.parametrize("mode", ["bf16", "fp32"])
@pytest.mark.parametrize("train", [False, True])
@pytest.mark.parametrize("n,s,p", [(2, 101, 10), (2, 171, 22)])
def test_layer_forward_train_and_backward(mh, mode, train, n, s, p):
    """y, dx, the history-state gradient, the 16 parameter gradients and the dense bias gradient of one layer against float64 autograd
    of oracle.bert_layer(history_state=); with p = attn_p = 0.1 the reference applies the host keep masks of all three dropouts"""
    from modeling import hip_autograd as ag
    from modeling import hip_layers
    dtype, dev = MODE_DT[mode], torch.device("cuda")
    h, a = 128, 2
    l = p + s
    pd = 0.1 if train else 0.0
    rs = np.random.RandomState(95 + s)
    sdt, sd64 = layer_sd(rs, h, mode)
    rnd = lambda *shape: torch.from_numpy(rs.standard_normal(shape).astype(np.float32)).to(dtype).float()
    x, hist, dy = rnd(n, s, h), rnd(n, p, h), rnd(n, s, h)
    add = soft_bias(rs, (n, 1, s, l))
    hm = torch.tensor([0.5, 1.0])
    names = list(ag.BertLayerFn.NAMES)
    # the counters layer_forward_train takes from DROPOUT seed 5: the attention's n A s (p + s), then the two hidden masks' M H each
    keeps = akeep = None
    if train:
        na, m = n * a * s * l, n * s * h
        akeep = H.attn_drop_keep_torch(range(n), a, s, pd, 5, 0, "cpu", keys=l).double()
        off1 = (na + 3) & ~3
        off2 = (off1 + m + 3) & ~3
        keeps = [torch.from_numpy(H.hidden_drop_keep(5, off, m, np.float32(pd)).reshape(n, s, h)).double() for off in (off1, off2)]
    ref_p = {k: sd64[k].clone().requires_grad_(True) for k in names}
    xr, hr, addr = x.double().requires_grad_(True), hist.double().requires_grad_(True), add.double().requires_grad_(True)
    y_ref = layer64p(xr, hr, addr, ref_p, "", a, hm, keeps, pd, akeep)
    if not train:
        y_o, _ = O.bert_layer(x.double(), add.double(), sd64, "", a, 1e-12, history_state=hist.double())
        y_plain = layer64p(x.double(), hist.double(), add.double(), sd64, "", a, None)
        assert float((y_plain - y_o).abs().max()) < 1e-9
    (y_ref * dy.double()).sum().backward()
    ref_g = {k: v.grad for k, v in ref_p.items()}

    packed = hip_layers.pack_layer({k: sdt[k].to(dev) for k in names}, "", dev, dtype)
    mh.DROPOUT.manual_seed(5)
    y, saved = hip_layers.layer_forward_train(packed, x.to(dtype).to(dev), a, 1e-12, p=pd, attn_p=pd, attn_bias=add.to(dev),
                                              head_mask=hm.to(dev), hist=hist.to(dtype).to(dev))
    assert saved["hist"] is not None and saved["lse"] is None and saved["dump"] is None
    if train:
        assert saved["adrop"] == (pd, 5, 0) and saved["drop1"][2] == off1 and saved["drop2"][2] == off2
    dx, g = hip_layers.layer_backward(packed, saved, dy.to(dtype).to(dev), mfma=mode == "bf16", want_d_bias=True)
    torch.cuda.synchronize()
    what = "layer S=%d P=%d" % (s, p)
    check(y, y_ref, Y_TOL[mode], what + " y")
    check(dx, xr.grad, G_TOL[mode], what + " dx")
    assert g["history_state"].dtype == dtype and tuple(g["history_state"].shape) == (n, p, h)
    check(g["history_state"], hr.grad, G_TOL[mode], what + " history_state")
    assert tuple(g["attn_bias"].shape) == (n, a, s, l)
    check(g["attn_bias"].sum(1, keepdim=True), addr.grad, G_TOL[mode], what + " d attn_bias")
    check_param_grads(mode, g, ref_g, what)


# ---- 9. encoder level: trainable_encoders.encoder_layers(encoder_history_states=) --------------------------------------------------

def encoder64(x, hists, add, sd, a, nl):
    out = x
    for i in range(nl):
        out = layer64p(out, hists[i], add, sd, "layer.%d." % i, a, None)
    return out


def encoder_inputs(mode, n, s, p, h, nl, seed):
    dtype = MODE_DT[mode]
    rs = np.random.RandomState(seed)
    body, sd64 = build_body(mode, nl, rs, h)
    rnd = lambda *shape: torch.from_numpy(rs.standard_normal(shape).astype(np.float32)).to(dtype).float()
    x, dy = rnd(n, s, h), rnd(n, s, h)
    hists = [rnd(n, p, h) for _ in range(nl)]
    add = soft_bias(rs, (n, 1, 1, p + s))
    return body, sd64, x, dy, hists, add


@pytest.mark.parametrize("mode", ["bf16", "fp32"])
def test_encoder_layers_with_history_states(mh, mode):
    """two layers through torch.autograd: the gradients of both history states, of hidden and of the [N,1,1,L] attention mask and the
    32 parameter gradients against float64; then with frozen parameters gradients arrive at the history states only"""
    from modeling import hip_autograd as ag
    from modeling import trainable_encoders as te
    dtype = MODE_DT[mode]
    n, s, p, h, a, nl = 3, 101, 10, 128, 2, 2
    body, sd64, x, dy, hists, add = encoder_inputs(mode, n, s, p, h, nl, 96)
    ref_p = {k: v.clone().requires_grad_(True) for k, v in sd64.items()}
    xr, addr = x.double().requires_grad_(True), add.double().requires_grad_(True)
    hr = [t.double().requires_grad_(True) for t in hists]
    ref = encoder64(xr, hr, addr, ref_p, a, nl)
    (ref * dy.double()).sum().backward()
    depth = 2 if mode == "bf16" else 1
    ag.set_grad_sink(None)
    ag.set_exact(mode == "fp32")
    try:
        xg = x.to(dtype).cuda().requires_grad_(True)
        hg = [t.to(dtype).cuda().requires_grad_(True) for t in hists]
        bg = add.cuda().requires_grad_(True)
        out = te.encoder_layers(body, xg, bg, encoder_history_states=hg)
        assert out.grad_fn is not None
        (out.float() * dy.cuda()).sum().backward()
        torch.cuda.synchronize()
        check(out, ref, depth * Y_TOL[mode], "2-layer encoder output")
        check(xg.grad, xr.grad, depth * G_TOL[mode], "encoder hidden.grad")
        assert tuple(bg.grad.shape) == (n, 1, 1, p + s)
        check(bg.grad, addr.grad, depth * G_TOL[mode], "encoder attention_mask.grad")
        for i in range(nl):
            assert hg[i].grad.dtype == dtype
            # (h1 sits one layer from the loss, h0 two)
            check(hg[i].grad, hr[i].grad, (depth if i == 0 else 1) * G_TOL[mode], "encoder h%d.grad" % i)
        got = {k: v.grad for k, v in body.encoder.named_parameters()}
        for i in range(nl):
            pre = "layer.%d." % i
            qscale = max(1.0, float(ref_p[pre + "attention.self.query.bias"].grad.abs().max()))
            for k in ag.BertLayerFn.NAMES:
                g, r = got[pre + k].double().cpu(), ref_p[pre + k].grad
                if k == "attention.self.key.bias":
                    assert float((g - r).abs().max()) <= depth * Z_TOL[mode] * qscale, (pre + k, float((g - r).abs().max()))
                    continue
                check(g, r, depth * G_TOL[mode], "encoder grad " + pre + k)
        # prefix tuning: frozen parameters, trainable history states
        body.zero_grad(set_to_none=True)
        for prm in body.parameters():
            prm.requires_grad_(False)
        hg2 = [t.to(dtype).cuda().requires_grad_(True) for t in hists]
        out2 = te.encoder_layers(body, x.to(dtype).cuda(), add.cuda(), encoder_history_states=hg2)
        (out2.float() * dy.cuda()).sum().backward()
        torch.cuda.synchronize()
        assert torch.equal(out2, out)
        for i in range(nl):
            assert torch.equal(hg2[i].grad, hg[i].grad), "h%d.grad with frozen parameters" % i
        assert all(prm.grad is None for prm in body.parameters())
    finally:
        ag.set_exact(False)


def test_prefix_tuning_follows_the_oracle_s_trajectory(mh):
    """three SGD steps on fp32 history states of a frozen two-layer encoder under a fixed target, fp32 parity mode: the loss after
    each step equals the float64 trajectory at 1e-3 of scale"""
    from modeling import hip_autograd as ag
    from modeling import trainable_encoders as te
    mode = "fp32"
    n, s, p, h, a, nl = 2, 37, 5, 128, 2, 2
    body, sd64, x, target, hists, add = encoder_inputs(mode, n, s, p, h, nl, 97)
    lr, steps = 0.3, 3
    # float64 trajectory
    hr = [t.double().clone().requires_grad_(True) for t in hists]
    ref_losses = []
    for _ in range(steps + 1):
        loss = ((encoder64(x.double(), hr, add.double(), sd64, a, nl) - target.double()) ** 2).mean()
        ref_losses.append(float(loss.detach()))
        grads = torch.autograd.grad(loss, hr)
        with torch.no_grad():
            for t, g in zip(hr, grads):
                t -= lr * n * s * h * g           # (the mean's 1 / (N S H) undone: steps large enough to move the loss)
    assert ref_losses[-1] < ref_losses[0] * 0.98, ref_losses
    for prm in body.parameters():
        prm.requires_grad_(False)
    hg = [torch.nn.Parameter(t.cuda()) for t in hists]
    opt = torch.optim.SGD(hg, lr=lr * n * s * h)
    ag.set_grad_sink(None)
    ag.set_exact(True)
    try:
        losses = []
        for _ in range(steps + 1):
            opt.zero_grad(set_to_none=True)
            out = te.encoder_layers(body, x.cuda(), add.cuda(), encoder_history_states=hg)
            loss = ((out - target.cuda()) ** 2).mean()
            losses.append(float(loss.detach()))
            loss.backward()
            opt.step()
    finally:
        ag.set_exact(False)
    assert all(prm.grad is None for prm in body.parameters())
    scale = max(1.0, max(ref_losses))
    for i, (g, r) in enumerate(zip(losses, ref_losses)):
        H.report_use("loss after %d steps" % i, abs(g - r) / scale, 1e-3)
        assert abs(g - r) <= 1e-3 * scale, (i, losses, ref_losses)


def test_encoder_layers_refuse_257_keys_under_grad_mode(mh):
    from modeling import hip_autograd as ag
    from modeling import trainable_encoders as te
    mode, dtype = "bf16", torch.bfloat16
    n, s, p, h, nl = 1, 247, 10, 128, 1
    body, _, x, _, hists, add = encoder_inputs(mode, n, s, p, h, nl, 98)
    ag.set_grad_sink(None)
    hg = [t.to(dtype).cuda().requires_grad_(True) for t in hists]
    with pytest.raises(NotImplementedError, match="256"):
        te.encoder_layers(body, x.to(dtype).cuda(), add.cuda(), encoder_history_states=hg)
    with torch.no_grad():                                   # ... while the forward alone serves it
        y = te.encoder_layers(body, x.to(dtype).cuda(), add.cuda(), encoder_history_states=hg)
    torch.cuda.synchronize()
    assert torch.isfinite(y.float()).all()
