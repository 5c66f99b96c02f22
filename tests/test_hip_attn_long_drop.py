"""GPU tests of the opt-in attention-probability dropout from 257 to 512 keys (modcr_qkv_attn_long_drop_fwd / _bwd: MODE 2 of the
streaming forward core and the DROP instantiations of the streaming backward cores under the wide counter layout of
csrc/attn_common.h, behind modcr_hip.qkv_attn(wide_dropout=) / qkv_attn_long_bwd(wide_dropout=), hip_layers.layer_forward_train(
long_dropout=), hip_autograd.set_long_backward(True, dropout=True) and the module route), bf16 and fp32.

The mask: attn_wide_drop.keep, the host restatement of the layout with the stride as a parameter, compared bit for bit through a
forward with zero weights and a zero bias (uniform, strictly positive probabilities) and post-dropout probabilities.

Values: float64 autograd over the bf16-rounded inputs of test_hip_attn_long_bwd's cases with that mask applied (P o m / (1 - p)), the
head mask as an [N, A] leaf.  Bounds, the repository's (test_hip_attn_long_bwd.check_all): max|got - ref| <= tol x max(1, max|ref|), tol
= 2e-2 in bf16 and 1e-3 in fp32, for ctx, dx, d_hist, dWqkv, dbqkv, d_bias and d_head_mask; relative L2 < 2e-2 for dx, d_hist, dWqkv in
bf16.  Layer level: y 2e-2 / 1e-3, gradients 2.5e-2 / 1e-3.  tools/attn_long_bwd_tolerance.py --drop restates the bf16 arithmetic
with its roundings and this mask on the CPU (profiles/attn_long_drop_tolerance_report.txt: predicted use of every bound per case).

Shapes (n, s, p, h, a): one key in the fifth tile; 300; the limit; queries below 256 with keys above (70 prefix rows); prefix rows
alone past 256; four heads with chunk-mean queries at 320.  Two heads everywhere else, N = 2 wherever it fits, so the head and the
sequence stride of the counter are exercised."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import attn_wide_drop as W
import helpers as H
import test_hip_attn_bias_bwd as B
import test_hip_attn_head_mask_bwd as HM
import test_hip_attn_long_bwd as LB
import test_hip_attn_prefix_bwd as PF
from oracle import modcr_oracle as O
from test_hip_attn_bias import NEG_INF, soft_bias
from test_hip_attn_bias_bwd import G_TOL, MODE_DT, TOL, Y_TOL, check_param_grads
from test_hip_attn_bwd import attention, check
from test_hip_attn_long import seq_batch

pytestmark = pytest.mark.gpu

DT = [torch.bfloat16, torch.float32]
SHAPES = [(2, 257, 0, 128, 2), (2, 300, 0, 128, 2), (1, 512, 0, 128, 2), (2, 250, 70, 128, 2), (1, 200, 312, 128, 2)]
CHUNK_SHAPE = (2, 320, 0, 256, 4)
FORMS = ["key mask", "dense", "head mask"]
DROP = (0.1, 77, 5 << 32)
NAMES7 = LB.NAMES7


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


def operands(form, shape):
    """(additive bias or None, head mask [N, A]) of one bias form: a folded key mask with padded keys (prefix keys among them), a
    dense [N, A, S, L] soft bias with single -inf and -10000 entries (key 0 finite), the head mask alone"""
    n, s, p, h, a = shape
    l = p + s
    if form == "key mask":
        km = torch.ones(n, l)
        km[0, l - 37:] = 0
        km[-1, l - 5:] = 0
        if p:
            km[0, 1:3] = 0
        return O.extend_mask(km).float(), LB.head_mask(n, a)
    if form == "dense":
        return PF.bias_of("[N,A,S,L]", n, s, p, a, s + p), LB.head_mask(n, a)
    return None, HM.mask_0_1(n, a, s + p)


def reference(shape, bias, hm, drop, cid=None, dctx=None, c=None):
    """float64 autograd with the host keep mask of the call's layout and hm [N, A] as a leaf:
    (ctx, dx, d_hist or None, dWqkv, dbqkv, dS [N, A, S, L], d_hm)"""
    n, s, p, h, a = shape
    c = LB.case(shape) if c is None else c
    w, b, x = c[0], c[1], c[2]
    hist = c[3] if p else torch.zeros(n, 0, h)
    dctx = c[-1] if dctx is None else dctx
    l = p + s
    pd = drop[0]
    keep = W.keep_of_call(n, a, s, p, drop).double()
    xr, hr, wr, br = (t.double().clone().requires_grad_(True) for t in (x, hist, w, b))
    dense = torch.zeros(n, a, s, l, dtype=torch.float64)
    if bias is not None:
        dense = dense + bias.double()
    dense.requires_grad_(True)
    leaf = hm.double().clone().requires_grad_(True)
    if p:
        assert cid is None
        ctx = PF.attention_prefix(xr, hr, wr, br, a, dense, keep=keep, p=pd)
    else:
        ctx, _ = attention(xr, wr, br, a, dense, cid=None if cid is None else cid.long(), keep=keep, p=pd)
    ctx = B.head_scale(ctx, leaf, a)
    (ctx * dctx.double()).sum().backward()
    for g in (xr.grad, wr.grad, br.grad, dense.grad, leaf.grad):
        assert torch.isfinite(g).all(), "the float64 reference itself is not finite"
    return [ctx.detach(), xr.grad, hr.grad if p else None, wr.grad, br.grad, dense.grad, leaf.grad]


@functools.lru_cache(maxsize=None)
def form_reference(shape, form):
    """shared by both dtypes and by tools/attn_long_bwd_tolerance.py --drop, read-only"""
    bias, hm = operands(form, shape)
    return reference(shape, bias, hm, DROP)


def run_drop(mh, dtype, shape, bias=None, hm=None, key_mask=None, cid=None, drop=DROP, want_d_bias=True, want_d_hm=True, forward=True,
             wide=True, entry=None, c=None, want_probs=False):
    """qkv_attn(wide_dropout=) + qkv_attn_long_bwd(wide_dropout=) (or `entry`) on NaN-prefilled outputs ->
    (ctx or None, dx, d_hist or None, dw, db, d_bias or None, d_hm or None[, probs])"""
    n, s, p, h, a = shape
    c = LB.case(shape) if c is None else c
    w, b, x = c[0], c[1], c[2]
    hist, dctx = (c[3], c[4]) if p else (None, c[-1])
    xd, wd, bd = x.to(dtype).cuda(), w.to(dtype).cuda(), b.cuda()
    hd = None if hist is None else hist.to(dtype).cuda()
    bias_d = None if bias is None else bias.cuda()
    hm_d = None if hm is None else hm.cuda()
    km_d = None if key_mask is None else key_mask.cuda()
    cid_d = None if cid is None else cid.cuda()
    wkw = dict(wide_dropout=True) if wide else {}
    ctx = probs = None
    if forward:
        fb = bias_d if key_mask is None else mh.fold_key_mask(km_d)
        ctx, probs = mh.qkv_attn(xd, wd, bd, hist=hd, chunk_id=cid_d, num_heads=a, attn_dropout=drop, attn_bias=fb, head_mask=hm_d,
                                 want_probs=want_probs, side_post_dropout=want_probs, **wkw)
    nan = lambda *sh: torch.full(sh, float("nan"), device="cuda")
    dw, db = nan(3 * h, h), nan(3 * h)
    d_bias = nan(n, a, s, p + s) if want_d_bias and (bias is not None or key_mask is not None) else None
    d_hm = nan(n, a) if want_d_hm else None
    kw = dict(d_head_mask=d_hm) if want_d_hm else {}
    if entry is None:
        entry = mh.qkv_attn_long_bwd
        kw.update(wkw)
        if key_mask is not None:
            kw["key_mask"] = km_d
    out = entry(dctx.to(dtype).cuda(), xd, wd, bd, dw, db, chunk_id=cid_d, num_heads=a, attn_dropout=drop, attn_bias=bias_d,
                head_mask=hm_d, d_bias=d_bias, hist=hd, **kw)
    torch.cuda.synchronize()
    dx, d_hist = out if p else (out, None)
    r = (ctx, dx, d_hist, dw, db, d_bias, d_hm)
    return r + (probs,) if want_probs else r


# ---- 1. the mask, bit for bit ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("shape", SHAPES)
def test_mask_bit_for_bit(mh, dtype, p, shape):
    """zero weights and a zero bias: every probability is 1 / L > 0, so the post-dropout probabilities are non-zero exactly where the
    forward kept -- the host mask of the wide layout, every sequence, head, query and key"""
    n, s, pl, h, a = shape
    l = pl + s
    drop = (p, 1234, 3 << 32)
    z = lambda *sh: torch.zeros(sh, dtype=dtype, device="cuda")
    ctx, probs = mh.qkv_attn(z(n, s, h), z(3 * h, h), torch.zeros(3 * h, device="cuda"), hist=z(n, pl, h) if pl else None, num_heads=a,
                             attn_dropout=drop, attn_bias=torch.zeros(1, 1, 1, l, device="cuda"), want_probs=True, side_post_dropout=True,
                             wide_dropout=True)
    torch.cuda.synchronize()
    keep = W.keep_of_call(n, a, s, pl, drop).bool()
    assert W.stride_of(l) == 512 and tuple(probs.shape) == tuple(keep.shape) == (n, a, s, l)
    got = probs.cpu() != 0
    assert torch.equal(got, keep), "%d of %d decisions differ" % (int((got != keep).sum()), keep.numel())
    kept = probs.cpu()[keep]
    assert float((kept - 1.0 / (l * (1.0 - p))).abs().max()) <= 1e-6
    assert abs(float(keep.float().mean()) - (1.0 - p)) < 0.01
    assert (ctx == 0).all()


# ---- 2. values against float64 --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("shape", SHAPES)
def test_cores_against_float64(mh, dtype, form, shape):
    n, s, p, h, a = shape
    assert mh.qkv_attn_long_bwd_route(n, s, p, h, a, mdt(mh, dtype)) == LB.want_route(dtype)
    bias, hm = operands(form, shape)
    got = run_drop(mh, dtype, shape, bias=bias, hm=hm)
    LB.check_all(dtype, list(got), form_reference(shape, form), "%s L=%d p=%g" % (form, p + s, DROP[0]), shape)


@pytest.mark.parametrize("dtype", DT)
def test_chunk_mean_queries_four_heads(mh, dtype):
    """a seq_enc-shaped call (T = 40 chunk-mean text queries, R = 280 regions, 320 keys, H = 256, A = 4) under a soft bias"""
    n, s, p, h, a = shape = CHUNK_SHAPE
    rs = np.random.RandomState(61)
    im, cm, gi, cid = seq_batch(rs, n, 40, s - 40)
    add = torch.from_numpy(rs.standard_normal((n, 1, s, s)).astype(np.float32))
    hm = HM.mask_0_1(n, a, 62)
    got = run_drop(mh, dtype, shape, bias=add, hm=hm, cid=cid)
    LB.check_all(dtype, list(got), reference(shape, add, hm, DROP, cid=cid), "chunk mean, 320 keys", shape)


def flat_case(shape):
    """the shape's case with the query projection scaled so that the scores' standard deviation is 0.4 (flat rows: every probability
    of a row within a small factor of 1 / L), weights bf16-rounded again"""
    n, s, p, h, a = shape
    w, b, x, dctx = LB.case(shape)
    q = torch.nn.functional.linear(x, w[:h], b[:h]).view(n, s, a, 64).transpose(1, 2)
    k = torch.nn.functional.linear(x, w[h:2 * h], b[h:2 * h]).view(n, s, a, 64).transpose(1, 2)
    f = 0.4 / float((q @ k.transpose(-1, -2) / 8.0).std())
    w2, b2 = w.clone(), b.clone()
    w2[:h] = (w[:h] * f).to(torch.bfloat16).float()
    b2[:h] = b[:h] * f
    q2 = torch.nn.functional.linear(x, w2[:h], b2[:h]).view(n, s, a, 64).transpose(1, 2)
    std = float((q2 @ k.transpose(-1, -2) / 8.0).std())
    return (w2, b2, x, dctx), std


@pytest.mark.parametrize("dtype", DT)
def test_flat_scores_d_bias_element_wise(mh, dtype):
    """flat scores (std <= 0.5) under a zero bias: the probabilities of a row lie within a small factor of 1 / L, so every d_bias
    element P_ij (m_ij dP_ij / (1 - p) - D_i) has the size of its row neighbours and ONE wrong keep decision of the query kernel
    moves one element by about its own size.  Two element-wise bounds, neither with the floor of 1 the file's bound has (max|d_bias|
    is 0.56 here and a typical element 0.02: the floored bound, 2e-2 absolute, would hide a flipped decision):
      * tol x max|d_bias| over the whole tensor;
      * tol x max_j |d_bias_ij| per query row (n, head, i) -- the rounding errors of the bf16 route (q | k | v rows, P~ and dS as bf16
        operands, each 2^-9 relative) scale with the row's own |dctx_i| and probabilities, which is what the row maximum measures;
        the CPU restatement of those roundings uses 40 % of it (profiles/attn_long_drop_tolerance_report.txt).
    A flipped decision moves its element by 0.13 row maxima in the median: the last assertion holds that it stands clear of the bound."""
    shape = SHAPES[1]
    n, s, p, h, a = shape
    c, std = flat_case(shape)
    assert std <= 0.5
    bias, hm = torch.zeros(n, a, s, s), torch.ones(n, a)
    ref = reference(shape, bias, hm, DROP, c=c)
    got = run_drop(mh, dtype, shape, bias=bias, hm=hm, c=c)
    LB.check_all(dtype, list(got), ref, "flat scores", shape)
    err = (got[5].cpu().double() - ref[5]).abs()
    top = float(ref[5].abs().max())
    rowmax = ref[5].abs().amax(-1, keepdim=True)
    assert top < 1.0 and float(rowmax.min()) > 0, "below 1 the un-floored bounds are the stricter ones"
    H.report_use("flat scores d_bias element-wise / max|d_bias|", float(err.max()) / top, TOL[dtype])
    H.report_use("flat scores d_bias element-wise / row max", float((err / rowmax).max()), TOL[dtype])
    assert float(err.max()) <= TOL[dtype] * top, (float(err.max()), top)
    assert float((err / rowmax).max()) <= TOL[dtype], float((err / rowmax).max())
    # what the row bound separates: the elements whose decision differs under another seed move by far more than it
    other = (DROP[0], DROP[1] + 1, DROP[2])
    differs = W.keep_of_call(n, a, s, p, DROP) != W.keep_of_call(n, a, s, p, other)
    moved = ((reference(shape, bias, hm, other, c=c)[5] - ref[5]).abs() / rowmax)[differs]
    assert float(moved.median()) > 4 * TOL[dtype], "a flipped decision stands clear of the bound"


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[3]])
def test_minus_infinity_row_and_a_head_at_zero(mh, dtype, shape):
    """a query row whose every key is -inf contributes exactly nothing; with a head at 0 its dQ, dK, dV (the head's 64 columns of
    every weight gradient) and d_bias are exactly 0 while d_head_mask keeps its value"""
    n, s, p, h, a = shape
    c = LB.case(shape)
    dctx = c[-1]
    bias = PF.bias_of("[N,A,S,L]", n, s, p, a, 5)
    hidden = 3 if p else 70
    bias[1, :, :, hidden] = NEG_INF
    bias[0, 1, 5, :] = NEG_INF
    bias[1, 1, s - 1, :] = NEG_INF
    hm = torch.ones(n, a)
    hm[:, 0] = 0.0
    got = run_drop(mh, dtype, shape, bias=bias, hm=hm)
    for t in got:
        assert t is None or torch.isfinite(t.float()).all()
    ctx, dx, d_hist, dw, db, d_bias, d_hm = got
    if p:
        assert (d_hist[1, hidden] == 0).all()
    assert (d_bias[:, 0] == 0).all(), "d_bias of the head at 0 is exactly 0"
    assert (d_bias[0, 1, 5] == 0).all() and (d_bias[1, 1, s - 1] == 0).all()
    assert (d_bias.cpu()[torch.isinf(bias)] == 0).all()
    assert (ctx[:, :, :64] == 0).all() and (ctx[0, 5, 64:] == 0).all()
    for part in range(3):
        assert (dw[part * h:part * h + 64] == 0).all() and (db[part * h:part * h + 64] == 0).all()
    fin, dz = bias.clone(), dctx.clone()
    fin[0, 1, 5, :] = 0
    fin[1, 1, s - 1, :] = 0
    dz[0, 5, 64:128] = 0
    dz[1, s - 1, 64:128] = 0
    ref = reference(shape, fin, hm, DROP, dctx=dz)
    ref[0][0, 5, 64:128] = 0
    ref[0][1, s - 1, 64:128] = 0
    ref[5][0, 1, 5] = 0
    ref[5][1, 1, s - 1] = 0
    assert float(ref[6][:, 0].abs().max()) > 0.5, "the head at 0 has a gradient of its own"
    LB.check_all(dtype, list(got), ref, "-inf + head at 0", shape)


# ---- 3. identities --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("shape", [(2, 170, 22, 128, 2), (1, 246, 10, 128, 2)])
def test_up_to_256_keys_they_are_the_older_entries(mh, dtype, shape):
    n, s, p, h, a = shape
    bias = PF.bias_of("[N,A,S,L]", n, s, p, a, s + p)
    hm = LB.head_mask(n, a)
    drop = (0.2, 77, 5 << 32)
    new = run_drop(mh, dtype, shape, bias=bias, hm=hm, drop=drop, want_probs=True)
    old = run_drop(mh, dtype, shape, bias=bias, hm=hm, drop=drop, want_probs=True, wide=False, entry=mh.qkv_attn_bwd)
    assert all(torch.isfinite(t.float()).all() for t in new)
    assert float((new[7] == 0).float().mean()) > 0.1, "the dropout is on"
    LB.same(new, old, names=NAMES7 + ("probs",), first=0)


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("drop", [None, (0.0, 77, 5)])
def test_without_dropout_they_are_the_older_entries(mh, dtype, drop):
    n, s, p, h, a = shape = (2, 260, 10, 128, 2)
    bias = PF.bias_of("[N,A,S,L]", n, s, p, a, 2)
    hm = LB.head_mask(n, a)
    new = run_drop(mh, dtype, shape, bias=bias, hm=hm, drop=drop, want_probs=True)
    old = run_drop(mh, dtype, shape, bias=bias, hm=hm, drop=drop, want_probs=True, wide=False)
    LB.same(new, old, names=NAMES7 + ("probs",), first=0)


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("shape", [SHAPES[3], SHAPES[0]])
def test_two_calls_are_bit_identical(mh, dtype, shape):
    n, s, p, h, a = shape
    bias = PF.bias_of("[N,A,S,L]", n, s, p, a, 2)
    hm = torch.linspace(0.25, 1.0, a)
    r1 = run_drop(mh, dtype, shape, bias=bias, hm=hm, want_probs=True)
    r2 = run_drop(mh, dtype, shape, bias=bias, hm=hm, want_probs=True)
    assert all(t is None or torch.isfinite(t.float()).all() for t in r1)
    LB.same(r1, r2, names=NAMES7 + ("probs",), first=0)
    r3 = run_drop(mh, dtype, shape, bias=bias, hm=hm, forward=False, want_d_bias=False, want_d_hm=False)
    assert r3[5] is None and r3[6] is None
    LB.same(r1[:5], r3[:5], names=NAMES7[1:5])
    # another (seed, offset) is another mask
    r4 = run_drop(mh, dtype, shape, bias=bias, hm=hm, drop=(DROP[0], DROP[1], DROP[2] + 4), forward=False)
    assert not torch.equal(r4[1], r1[1])


def raw_call(mh, dtype, shape, bias, outs, accumulate=False, attn_p=DROP[0]):
    """modcr_qkv_attn_long_drop_bwd itself on caller-owned outputs (dx, d_hist, dwqkv, dbqkv, d_bias, d_hm): returns its code"""
    n, s, p, h, a = shape
    c = LB.case(shape)
    dt = mdt(mh, dtype)
    dctx = c[-1].to(dtype).cuda()
    x, w = c[2].to(dtype).cuda(), c[0].to(dtype).cuda()
    hist = c[3].to(dtype).cuda() if p else None
    bd, bias_d = c[1].cuda(), bias.cuda().contiguous()
    dx, dh, dw, db, d_bias, d_hm = outs
    need = mh.lib().modcr_qkv_attn_long_drop_bwd_workspace(n, s, p, h, dt)
    ws = torch.empty(max(need, 256), dtype=torch.uint8, device="cuda")
    sn, sa, sq = [0 if bias_d.shape[d] == 1 else bias_d.stride(d) for d in range(3)]
    ptr = lambda v: None if v is None else ctypes.c_void_p(v.data_ptr())
    rc = mh.lib().modcr_qkv_attn_long_drop_bwd(ptr(dctx), ptr(x), ptr(hist), ptr(w), ptr(bd), ptr(bias_d), sn, sa, sq, None, 0, None, 0, None,
                                               ptr(dx), ptr(dh), ptr(dw), ptr(db), 1 if accumulate else 0, ptr(d_bias), ptr(d_hm), n, s, p, h,
                                               a, attn_p, DROP[1], DROP[2], ptr(ws), need, dt, None)
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("shape", [SHAPES[3], SHAPES[0]])
def test_outputs_fully_written_guards_and_accumulate(mh, dtype, shape):
    n, s, p, h, a = shape
    l = p + s
    tol = TOL[dtype]
    bias = PF.bias_of("[N,A,S,L]", n, s, p, a, 3)
    ref = reference(shape, bias, torch.ones(n, a), DROP)
    sizes = (n * s * h, n * p * h, 3 * h * h, 3 * h, n * a * s * l, n * a)
    mk = lambda: [LB.guarded(sizes[0], dtype), LB.guarded(sizes[1], dtype) if p else None] + [LB.guarded(z) for z in sizes[2:]]
    outs = mk()
    assert raw_call(mh, dtype, shape, bias, outs) == 0, mh.lib().modcr_last_error()
    for t, z, nm in zip(outs, sizes, NAMES7[1:]):
        if t is None:
            continue
        assert torch.isfinite(t[:z].float()).all(), nm + ": an element was not written"
        assert (t[z:] == 7.0).all(), nm + ": written behind its end"
    shaped = [None, outs[0][:sizes[0]].view(n, s, h), outs[1][:sizes[1]].view(n, p, h) if p else None, outs[2][:sizes[2]].view(3 * h, h),
              outs[3][:sizes[3]], outs[4][:sizes[4]].view(n, a, s, l), outs[5][:sizes[5]].view(n, a)]
    LB.check_all(dtype, shaped, ref, "NaN prefill", shape)
    rs = np.random.RandomState(8)
    pre_w = torch.from_numpy(rs.standard_normal((3 * h, h)).astype(np.float32))
    pre_b = torch.from_numpy(rs.standard_normal((3 * h,)).astype(np.float32))
    acc = mk()
    acc[2][:sizes[2]] = pre_w.reshape(-1).cuda()
    acc[3][:sizes[3]] = pre_b.cuda()
    assert raw_call(mh, dtype, shape, bias, acc, accumulate=True) == 0, mh.lib().modcr_last_error()
    scale_w, scale_b = max(1.0, float(ref[3].abs().max())), max(1.0, float(ref[4].abs().max()))
    e_w = float((acc[2][:sizes[2]].view(3 * h, h).cpu().double() - pre_w.double() - ref[3]).abs().max())
    e_b = acc[3][:sizes[3]].cpu().double() - pre_b.double() - ref[4]
    e_b[h:2 * h] = 0                # (the key-bias slice: held in check_all above)
    assert e_w <= tol * scale_w and float(e_b.abs().max()) <= tol * scale_b
    assert torch.equal(acc[0], outs[0]) and torch.equal(acc[4], outs[4]) and torch.equal(acc[5], outs[5])
    # a refused call writes nothing
    ref_outs = mk()
    assert raw_call(mh, dtype, shape, bias, ref_outs, attn_p=1.5) == -1 and b"dropout" in mh.lib().modcr_last_error()
    assert all(t is None or torch.isnan(t[:z].float()).all() for t, z in zip(ref_outs, sizes))


# ---- 4. layer level -------------------------------------------------------------------------------------------------------------------

def run_layer_fn(mh, mode, fn_name, x, dy, hist, mask, hm, sdt, mask_grad, hm_grad, attn_p):
    """test_hip_attn_long_bwd.run_layer_fn with attention dropout attn_p (hidden dropout 0), DROPOUT seeded with 5"""
    from modeling import hip_autograd as ag
    from modeling import hip_layers
    dtype, dev = MODE_DT[mode], torch.device("cuda")
    a = 2
    names = list(ag.BertLayerFn.NAMES)
    params = [torch.nn.Parameter(sdt[k].to(dev)) for k in names]
    packed = hip_layers.pack_layer(dict(zip(names, params)), "", dev, dtype)
    xg = x.to(dtype).to(dev).requires_grad_(True)
    hg = hist.to(dtype).to(dev).requires_grad_(True) if hist is not None else None
    mg = mask.to(dev).requires_grad_(mask_grad)
    gg = hm.to(dev).requires_grad_(hm_grad) if hm is not None else None
    fn = getattr(ag, fn_name)
    mh.DROPOUT.manual_seed(5)
    if fn_name == "BertLayerFn":
        y = fn.apply(xg, mg, None, None, a, 1e-12, 0.0, attn_p, packed, *params)
    elif fn_name == "BertLayerBiasFn":
        y = fn.apply(xg, mg, gg, None, a, 1e-12, 0.0, attn_p, packed, *params)
    else:
        y = fn.apply(xg, hg, mg, gg, None, a, 1e-12, 0.0, attn_p, packed, *params)
    (y.float() * dy.to(dev)).sum().backward()
    torch.cuda.synchronize()
    return y, xg.grad, None if hg is None else hg.grad, mg.grad, None if gg is None else gg.grad, {k: prm.grad for k, prm in zip(names, params)}


LAYER_CASES = [("BertLayerFn", 2, 300, 0), ("BertLayerBiasFn", 2, 300, 0), ("BertLayerPrefixFn", 2, 260, 10), ("BertLayerGateFn", 2, 260, 10)]


@pytest.mark.parametrize("mode", ["bf16", "fp32"])
@pytest.mark.parametrize("fn_name,n,s,p", LAYER_CASES)
def test_layer_functions_with_the_dropout_switch_on(mh, mode, fn_name, n, s, p):
    """y and the gradients of x, hist, attn_bias, head_mask and the 16 parameters at attn_p = 0.1 against the oracle layer under float64
    autograd with the host mask of the counters the layer consumed: DROPOUT seed 5, offset 0, n A s (P + S) of them, wide layout.
    With set_long_backward(True) alone the same call still raises."""
    from modeling import hip_autograd as ag
    a, l, h, pd = 2, p + s, 128, 0.1
    rs, sdt, sd64, x, dy, hist = LB.layer_case(mode, n, s, p, 500 + s + p)
    names = list(ag.BertLayerFn.NAMES)
    binary = fn_name == "BertLayerFn"
    if binary:
        mask = torch.ones(n, l)
        mask[0, 250:] = 0
        mask[1, 290:] = 0
        add = O.extend_mask(mask).float()
    else:
        mask = add = soft_bias(rs, (n, 1, s, l))
    hm = None if binary else (HM.mask_0_1(n, a, s) if fn_name == "BertLayerGateFn" else torch.tensor([0.5, 1.0]))
    hm_grad = fn_name == "BertLayerGateFn"
    akeep = W.keep(range(n), a, s, pd, 5, 0, 512, keys=l).double()
    ref_p = {k: sd64[k].clone().requires_grad_(True) for k in names}
    xr, addr = x.double().requires_grad_(True), add.double().requires_grad_(True)
    hr = hist.double().requires_grad_(True) if p else torch.zeros(n, 0, h, dtype=torch.float64)
    hl = hm.double().requires_grad_(True) if hm_grad else hm
    y_ref = PF.layer64p(xr, hr, addr, ref_p, "", a, hl, None, pd, akeep)
    (y_ref * dy.double()).sum().backward()
    ref_g = {k: v.grad for k, v in ref_p.items()}
    ag.set_grad_sink(None)
    ag.set_exact(mode == "fp32")
    try:
        ag.set_long_backward(True)
        with pytest.raises(NotImplementedError, match="256"):
            run_layer_fn(mh, mode, fn_name, x, dy, hist, mask, hm, sdt, not binary, hm_grad, pd)
        ag.set_long_backward(True, dropout=True)
        y, dx, dh, dmask, dhm, grads = run_layer_fn(mh, mode, fn_name, x, dy, hist, mask, hm, sdt, not binary, hm_grad, pd)
        assert mh.DROPOUT.offset == n * a * s * l, "the layer took the attention's counters as below 256 keys, and no others"
    finally:
        ag.set_long_backward(False)
        ag.set_exact(False)
    what = "%s S=%d P=%d p=0.1" % (fn_name, s, p)
    check(y, y_ref, Y_TOL[mode], what + " y")
    check(dx, xr.grad, G_TOL[mode], what + " dx")
    if p:
        assert dh.dtype == MODE_DT[mode]
        check(dh, hr.grad, G_TOL[mode], what + " d_hist")
    if not binary:
        assert tuple(dmask.shape) == tuple(add.shape)
        check(dmask, addr.grad, G_TOL[mode], what + " d attn_bias")
    if hm_grad:
        assert tuple(dhm.shape) == (n, a) and dhm.dtype == torch.float32
        check(dhm, hl.grad, G_TOL[mode], what + " d head_mask")
    check_param_grads(mode, grads, ref_g, what)


def test_module_route_applies_the_dropout_with_the_switch_on(mh):
    """CaptionBertSelfAttention.hip_forward in training mode at 300 keys: today's error without the switch; with it the binary key
    mask is folded into the bias route and the probabilities it returns are the post-dropout ones under the wide mask"""
    from modeling import hip_autograd as ag
    from modeling.modeling_bert import CaptionBertSelfAttention
    from modeling.bert_primitives import BertConfig
    n, s, h, a = 2, 300, 128, 2
    cfg = BertConfig(hidden_size=h, num_attention_heads=a, attention_probs_dropout_prob=0.1, output_attentions=True, modcr_dtype="bf16")
    torch.manual_seed(3)
    mod = CaptionBertSelfAttention(cfg).cuda().train()
    x = torch.randn(n, s, h, device="cuda").to(torch.bfloat16)
    km = torch.ones(n, s, device="cuda")
    km[1, 280:] = 0
    with pytest.raises(NotImplementedError, match="exceeds the 256 keys the attention kernels take"):
        mod.hip_forward(x, key_mask=km, want_probs=True)
    try:
        ag.set_long_backward(True, dropout=True)
        mh.DROPOUT.manual_seed(9)
        ctx, probs = mod.hip_forward(x, key_mask=km, want_probs=True)
        torch.cuda.synchronize()
        with pytest.raises(NotImplementedError, match="256"):
            mod.hip_forward(x, mask_bits=torch.zeros(n, s, 10, dtype=torch.int32, device="cuda"))
    finally:
        ag.set_long_backward(False)
    keep = W.keep(range(n), a, s, 0.1, 9, 0, 512, keys=s).bool()
    live = km.cpu().bool()[:, None, None, :].expand(n, a, s, s)
    assert torch.equal((probs.cpu() != 0) & live, keep & live)
    assert torch.isfinite(ctx.float()).all()
    mod.eval()
    ctx_e, probs_e = mod.hip_forward(x, key_mask=km, want_probs=True)          # eval mode: no dropout, the binary route as before
    assert float((probs_e.sum(-1) - 1).abs().max()) < 1e-3


def test_roberta_prefix_body_trains_above_256_keys_with_dropout(mh):
    """RobertaPrefixModel in TRAINING mode at 260 tokens + 10 prompt rows = 270 keys, attention dropout 0.1 (hidden dropout 0): refused
    with the backward switch alone, runs with the dropout switch; every layer takes its n A s s counters, the result is a function of
    the DROPOUT seed, differs from the eval-mode forward, and every gradient is finite and non-zero"""
    from modeling import hip_autograd as ag
    from modeling.roberta_prefix import RobertaPrefixModel
    torch.manual_seed(12)
    cfg = dict(vocab_size=120, hidden_size=128, num_hidden_layers=3, num_attention_heads=2, intermediate_size=512,
               max_position_embeddings=514, type_vocab_size=2, layer_norm_eps=1e-5, pad_token_id=1)
    model = RobertaPrefixModel(**cfg, initializer_range=0.05, attention_probs_dropout_prob=0.1, hidden_dropout_prob=0.0).cuda().train()
    n, t, p = 2, 260, 10
    ids = torch.randint(3, 120, (n, t))
    ids[:, 0] = 0
    ids[1, 200:] = 1
    am = (ids != 1).float()
    prompt = torch.randn(n, p, 128) * 0.5
    kw = dict(input_ids=ids.cuda(), token_type_ids=torch.zeros(n, t, dtype=torch.int64).cuda(), attention_mask=am.cuda(), input_mask=torch.ones(n, p).cuda())
    ag.set_grad_sink(None)

    def step(seed):
        mh.DROPOUT.manual_seed(seed)
        pg = prompt.cuda().requires_grad_(True)
        model.zero_grad()
        seq, pool = model(prompt_embeddings=pg, **kw)
        (pool.float().sum() + seq.float().sum()).backward()
        torch.cuda.synchronize()
        return pool.detach().float(), pg.grad.detach().float()
    try:
        ag.set_long_backward(True)
        with pytest.raises(NotImplementedError, match="attention_probs_dropout_prob = 0"):
            step(4)
        ag.set_long_backward(True, dropout=True)
        pool1, g1 = step(4)
        assert mh.DROPOUT.offset == 3 * n * 2 * (t + p) * (t + p)
        grads = {k: prm.grad.clone() for k, prm in model.named_parameters() if prm.grad is not None}
        pool2, g2 = step(4)
        pool3, g3 = step(5)
        model.eval()
        with torch.no_grad():
            _, pool_e = model(prompt_embeddings=prompt.cuda(), **kw)
    finally:
        ag.set_long_backward(False)
    assert torch.equal(pool1, pool2) and torch.equal(g1, g2), "the same seed gives the same masks"
    assert not torch.equal(pool1, pool3) and not torch.equal(pool1, pool_e.float())
    assert torch.isfinite(g1).all() and float(g1.abs().max()) > 0
    assert len(grads) >= 3 * 16
    for k, g in grads.items():
        assert torch.isfinite(g).all(), k
        assert float(g.abs().max()) > 0 or k.endswith("key.bias") or "position" in k or "token_type" in k, k
