"""GPU tests of the attention backward under an additive float mask / bias and a head mask (modcr_qkv_attn_bias_bwd: the cores of
csrc/attn_bias_bwd.hip behind modcr_hip.qkv_attn_bwd(attn_bias=, head_mask=, d_bias=), hip_layers.layer_backward,
hip_autograd.BertLayerBiasFn and trainable_encoders.encoder_layers), S <= 256, bf16 and fp32.

Checker: torch autograd in float64 on the CPU of
    s = q.k^T / 8 + bias,  P = softmax(s),  P' = P o m / (1 - p),  P'' = hm P',  ctx = P''.V
(test_hip_attn_bwd.attention for the formula, the head mask as a scale of the context columns, helpers.attn_drop_keep_torch for
the keep mask m).  The bias enters as a dense float64 [N,A,S,S] leaf, so its gradient is the dense dS the kernel writes to d_bias.

Bounds (the repository's): max|got - ref| <= tol x max(1, max|ref|), tol = 2e-2 in bf16 and 1e-3 in fp32, for ctx, dx, dWqkv,
dbqkv and d_bias; relative L2 < 2e-2 for dx and dWqkv in bf16.  The key-bias slice of dbqkv is analytically zero and is held as in
test_hip_attn_bwd.test_attn_bwd5_vs_oracle.  On the CPU the same formula with q | k | v and P rounded to bf16 stays within 7.3e-3 of
scale and 4.1e-3 relative L2 of float64 on all five quantities (bias mix below, head mask (1, 0.5), p = 0.2, four shapes), fp32
within 1e-6: the bounds leave room.  Layer level: the bounds of test_hip_kernels.test_layer_backward_golden (y 2e-2 / 1e-3;
gradients 2.5e-2 in bf16, 1e-3 in fp32; the analytically zero key-bias gradient 6e-2 of the query-bias scale in bf16).  Two
layers (encoder level) in bf16: twice the one-layer bounds, as test_hip_attn_bias takes 2 x 2e-2 for a bf16 layer's output --
the gradient stream is rounded to bf16 once more per layer; fp32 stays at 1e-3."""
import functools

import numpy as np
import pytest
import torch

import helpers as H
from oracle import modcr_oracle as O
from test_hip_attn_bias import NEG_INF, layer_sd, oracle_layer, soft_bias
from test_hip_attn_bwd import attention, check
from test_hip_attn_fullsize import bf16r
from test_hip_attn_long import seq_batch, small_config

pytestmark = pytest.mark.gpu

TOL = {torch.bfloat16: 2e-2, torch.float32: 1e-3}
DT = [torch.bfloat16, torch.float32]
# (n, s, h, a): one partial tile; S % 4 != 0 (unaligned bias rows); 180; the MFMA core's edge; the first shape on the exact core; the limit
SHAPES = [(2, 37, 128, 2), (3, 101, 128, 2), (2, 180, 128, 2), (2, 192, 128, 2), (2, 193, 256, 4), (1, 256, 128, 2)]


@pytest.fixture(scope="module")
def mh():
    import __graft_entry__ as g  # noqa: F401
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import modcr_hip
    modcr_hip.lib()
    return modcr_hip


@functools.lru_cache(maxsize=None)
def case(n, s, h, a):
    """bf16-rounded weights (helpers._lin), inputs and dctx of one shape, shared by every test on it (read-only)"""
    rs = np.random.RandomState(4000 + 13 * n + s + h)
    sd = {}
    for nm in ("query", "key", "value"):
        H._lin(rs, sd, nm, h, h)
    sd = H.to_torch(sd)
    w = bf16r(torch.cat([sd["query.weight"], sd["key.weight"], sd["value.weight"]], 0))
    b = torch.cat([sd["query.bias"], sd["key.bias"], sd["value.bias"]], 0)
    x = bf16r(torch.from_numpy(rs.standard_normal((n, s, h)).astype(np.float32)))
    dctx = bf16r(torch.from_numpy(rs.standard_normal((n, s, h)).astype(np.float32)))
    return w, b, x, dctx


def head_scale(ctx, hm, a):
    n, s, h = ctx.shape
    return (ctx.view(n, s, a, 64) * hm.to(ctx.dtype).reshape(-1, a)[:, None, :, None]).reshape(n, s, h)


def reference(c, a, bias, hm=None, cid=None, drop=None, dctx=None):
    """float64 autograd on the CPU: (ctx, dx, dWqkv, dbqkv, dense dS [N,A,S,S])"""
    w, b, x, dctx0 = c
    dctx = dctx0 if dctx is None else dctx
    n, s, h = x.shape
    xr, wr, br = (t.double().clone().requires_grad_(True) for t in (x, w, b))
    dense = torch.zeros(n, a, s, s, dtype=torch.float64)
    if bias is not None:
        dense = dense + bias.double()
    dense.requires_grad_(True)
    keep, p = None, 0.0
    if drop is not None:
        p, seed, off = drop
        keep = H.attn_drop_keep_torch(range(n), a, s, p, seed, off, "cpu", keys=s).double()
    ctx, _ = attention(xr, wr, br, a, dense, cid=None if cid is None else cid.long(), keep=keep, p=p)
    if hm is not None:
        ctx = head_scale(ctx, hm, a)
    (ctx * dctx.double()).sum().backward()
    for g in (xr.grad, wr.grad, br.grad, dense.grad):
        assert torch.isfinite(g).all(), "the float64 reference itself is not finite"
    return ctx.detach(), xr.grad, wr.grad, br.grad, dense.grad


def run_hip(mh, dtype, c, a, bias=None, hm=None, cid=None, drop=None, want_d_bias=True, dctx=None, forward=True):
    """qkv_attn + qkv_attn_bwd on the GPU; a bias that already lives there is handed over as it is (views keep their strides)"""
    w, b, x, dctx0 = c
    dctx = dctx0 if dctx is None else dctx
    n, s, h = x.shape
    xd, wd, bd = x.to(dtype).cuda(), w.to(dtype).cuda(), b.cuda()
    bias_d = None if bias is None else bias.cuda()
    hm_d = None if hm is None else hm.cuda()
    cid_d = None if cid is None else cid.cuda()
    ctx = None
    if forward:
        ctx, _ = mh.qkv_attn(xd, wd, bd, chunk_id=cid_d, num_heads=a, attn_dropout=drop, attn_bias=bias_d, head_mask=hm_d)
    dw, db = torch.full((3 * h, h), float("nan"), device="cuda"), torch.full((3 * h,), float("nan"), device="cuda")
    d_bias = torch.full((n, a, s, s), float("nan"), device="cuda") if want_d_bias and bias is not None else None
    dx = mh.qkv_attn_bwd(dctx.to(dtype).cuda(), xd, wd, bd, dw, db, chunk_id=cid_d, num_heads=a, attn_dropout=drop,
                         attn_bias=bias_d, head_mask=hm_d, d_bias=d_bias)
    torch.cuda.synchronize()
    return ctx, dx, dw, db, d_bias


def check_all(dtype, got, ref, what, n, s, h):
    """ctx, dx, dWqkv, dbqkv, d_bias against the reference at the file's bounds"""
    tol = TOL[dtype]
    ctx, dx, dw, db, d_bias = got
    ctx_r, dx_r, dw_r, db_r, ds_r = ref
    if ctx is not None:
        check(ctx, ctx_r, tol, what + " ctx")
    e_dx = check(dx, dx_r, tol, what + " dx")
    e_dw = check(dw, dw_r, tol, what + " dwqkv")
    kb = slice(h, 2 * h)            # the key-bias gradient is analytically zero: rounding noise of a sum over N S rows on both sides
    dbm, dbr = db.detach().float().cpu().clone(), db_r.float().clone()
    dbm[kb] = 0
    dbr[kb] = 0
    check(dbm, dbr, tol, what + " dbqkv")
    assert torch.isfinite(db).all()
    assert float(db[kb].abs().max()) <= tol * max(1.0, float(db_r.abs().max())) * (n * s) ** 0.5 * 0.25, what + " key-bias slice"
    if d_bias is not None:
        check(d_bias, ds_r, tol, what + " d_bias")
    if dtype == torch.bfloat16:
        H.report_use(what + " dx rel L2", e_dx[1], 2e-2, kind="relative L2")
        H.report_use(what + " dw rel L2", e_dw[1], 2e-2, kind="relative L2")
        assert e_dx[1] < 2e-2 and e_dw[1] < 2e-2, (what, e_dx, e_dw)


def want_core(dtype, s):
    return "mfma" if dtype == torch.bfloat16 and s <= 192 else "exact"


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("n,s,h,a", SHAPES)
def test_shapes_and_cores(mh, dtype, n, s, h, a):
    """a soft [N,1,S,S] bias (10 % -10000, 10 % -inf) with a head mask at every shape class; the core each shape takes"""
    assert mh.qkv_attn_bias_bwd_route(n, s, h, a, mh.BF16 if dtype == torch.bfloat16 else mh.F32) == want_core(dtype, s)
    c = case(n, s, h, a)
    rs = np.random.RandomState(s)
    bias = soft_bias(rs, (n, 1, s, s))
    hm = torch.linspace(1.0, 0.5, a)
    check_all(dtype, run_hip(mh, dtype, c, a, bias=bias, hm=hm), reference(c, a, bias, hm), "S=%d" % s, n, s, h)


@pytest.mark.parametrize("dtype", DT)
def test_bias_forms(mh, dtype):
    """every broadcast form and two strided views; d_bias is the reference's DENSE dS for each of them"""
    n, s, h, a = 3, 101, 128, 2
    c = case(n, s, h, a)
    rs = np.random.RandomState(17)
    forms = {"[N,A,S,S]": (n, a, s, s), "[N,1,S,S]": (n, 1, s, s), "[1,A,S,S]": (1, a, s, s), "[N,1,1,S]": (n, 1, 1, s), "[S,S]": (s, s)}
    for name, shape in forms.items():
        bias = soft_bias(rs, shape)
        check_all(dtype, run_hip(mh, dtype, c, a, bias=bias), reference(c, a, bias), name, n, s, h)
    # an expand()ed view: rows of a wider tensor (row stride S + 3), broadcast over the heads by stride 0
    wide = soft_bias(rs, (n, 1, s, s + 3))
    view = wide.cuda()[..., :s].expand(n, a, s, s)
    assert not view.is_contiguous() and view.stride(1) == 0 and view.stride(2) == s + 3
    check_all(dtype, run_hip(mh, dtype, c, a, bias=view), reference(c, a, wide[..., :s]), "expand()ed view", n, s, h)
    # a sliced view with a non-contiguous query stride: every second row of a [N,A,2S,S] tensor
    tall = soft_bias(rs, (n, a, 2 * s, s))
    view = tall.cuda()[:, :, ::2]
    assert view.stride(2) == 2 * s and view.stride(3) == 1
    check_all(dtype, run_hip(mh, dtype, c, a, bias=view), reference(c, a, tall[:, :, ::2]), "sliced view", n, s, h)


@pytest.mark.parametrize("dtype", DT)
def test_head_mask(mh, dtype):
    n, s, h, a = 3, 101, 128, 2
    c = case(n, s, h, a)
    rs = np.random.RandomState(23)
    bias = soft_bias(rs, (n, 1, s, s))
    hm0 = torch.tensor([0.0, 0.5])
    got = run_hip(mh, dtype, c, a, bias=bias, hm=hm0)
    check_all(dtype, got, reference(c, a, bias, hm0), "head mask [A] with a 0", n, s, h)
    # the masked head's dq | dk | dv columns are exactly 0: so are the rows of dWqkv and the entries of dbqkv they feed, and its dS
    dw, db, d_bias = got[2], got[3], got[4]
    for part in range(3):
        assert (dw[part * h:part * h + 64] == 0).all() and (db[part * h:part * h + 64] == 0).all()
    assert (d_bias[:, 0] == 0).all() and (got[0][:, :, :64] == 0).all()
    hm_na = torch.from_numpy(rs.uniform(size=(n, a)).astype(np.float32))
    check_all(dtype, run_hip(mh, dtype, c, a, bias=bias, hm=hm_na), reference(c, a, bias, hm_na), "head mask [N,A]", n, s, h)
    check_all(dtype, run_hip(mh, dtype, c, a, hm=hm_na), reference(c, a, None, hm_na), "head mask alone", n, s, h)


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("n,s,h,a", [(3, 101, 128, 2), (2, 180, 128, 2), (2, 230, 128, 2)])
def test_attention_dropout(mh, dtype, n, s, h, a):
    c = case(n, s, h, a)
    rs = np.random.RandomState(s + 1)
    bias = soft_bias(rs, (n, 1, s, s))
    hm = torch.tensor([1.0, 0.5])
    drop = (0.2, 77 + s, 5 << 32)
    assert mh.qkv_attn_bias_bwd_route(n, s, h, a, mh.BF16 if dtype == torch.bfloat16 else mh.F32) == want_core(dtype, s)
    check_all(dtype, run_hip(mh, dtype, c, a, bias=bias, hm=hm, drop=drop), reference(c, a, bias, hm, drop=drop), "p=0.2 S=%d" % s, n, s, h)


@pytest.mark.parametrize("dtype", DT)
def test_chunk_mean_queries(mh, dtype):
    """a seq_enc-shaped call (T = 60, R = 41): the phase-3 additive mask with a soft term on top, chunk-mean queries"""
    n, t, r, h, a = 3, 60, 41, 128, 2
    s = t + r
    c = case(n, s, h, a)
    rs = np.random.RandomState(60)
    im, cm, gi, cid = seq_batch(rs, n, t, r)
    add = O.seq_phase_mask(im.double(), cm.double(), t, r, 3).float() + torch.from_numpy(rs.standard_normal((n, 1, s, s)).astype(np.float32))
    check_all(dtype, run_hip(mh, dtype, c, a, bias=add, cid=cid), reference(c, a, add, cid=cid), "phase 3", n, s, h)


def test_consistent_with_the_binary_backward(mh):
    """a 0 / -10000 [N,1,1,S] bias and qkv_attn_bwd(key_mask=) without lse: the same class of core on the same arithmetic"""
    dtype = torch.bfloat16
    n, s, h, a = 3, 101, 128, 2
    c = case(n, s, h, a)
    w, b, x, dctx = c
    km = torch.ones(n, s)
    km[1, 70:] = 0
    km[2, 33:] = 0
    add = O.extend_mask(km).float()
    assert tuple(add.shape) == (n, 1, 1, s)
    ref = reference(c, a, add)
    got = run_hip(mh, dtype, c, a, bias=add)
    check_all(dtype, got, ref, "0 / -10000 bias", n, s, h)
    dw, db = torch.empty(3 * h, h, device="cuda"), torch.empty(3 * h, device="cuda")
    dx = mh.qkv_attn_bwd(dctx.to(dtype).cuda(), x.to(dtype).cuda(), w.to(dtype).cuda(), b.cuda(), dw, db, key_mask=km.cuda(), num_heads=a)
    check_all(dtype, (None, dx, dw, db, None), ref, "binary backward", n, s, h)
    check(got[1], dx.float(), TOL[dtype], "dx, bias route vs binary route")
    check(got[2], dw, TOL[dtype], "dwqkv, bias route vs binary route")
    kb = slice(h, 2 * h)
    d1, d2 = got[3].clone(), db.clone()
    d1[kb] = 0
    d2[kb] = 0
    check(d1, d2, TOL[dtype], "dbqkv, bias route vs binary route")


@pytest.mark.parametrize("dtype", DT)
def test_rows_of_minus_infinity_everywhere(mh, dtype):
    n, s, h, a = 3, 101, 128, 2
    c = case(n, s, h, a)
    dctx = c[3]
    bias = soft_bias(np.random.RandomState(5), (n, a, s, s))
    bias[1, 0, 5, :] = NEG_INF
    bias[2, :, 70, :] = NEG_INF
    got = run_hip(mh, dtype, c, a, bias=bias)
    for t in got:
        assert torch.isfinite(t.float()).all()
    d_bias = got[4]
    assert (d_bias[1, 0, 5] == 0).all() and (d_bias[2, :, 70] == 0).all()
    assert (d_bias.cpu()[torch.isinf(bias)] == 0).all(), "a -inf entry has a zero in d_bias"
    # reference: a finite stand-in for the two rows with dctx zeroed on their (row, head) columns -- they contribute nothing
    fin, dz = bias.clone(), dctx.clone()
    fin[1, 0, 5, :] = 0
    fin[2, :, 70, :] = 0
    dz[1, 5, :64] = 0
    dz[2, 70] = 0
    ref = list(reference(c, a, fin, dctx=dz))
    ref[0][1, 5, :64] = 0
    ref[0][2, 70] = 0
    check_all(dtype, got, ref, "all -inf rows", n, s, h)


@pytest.mark.parametrize("dtype,s", [(torch.bfloat16, 180), (torch.bfloat16, 230), (torch.float32, 101)])
def test_two_launches_are_bit_identical(mh, dtype, s):
    n, h, a = 2 if s > 101 else 3, 128, 2
    c = case(n, s, h, a)
    bias = soft_bias(np.random.RandomState(2), (n, a, s, s))
    hm = torch.tensor([0.25, 1.0])
    drop = (0.2, 9, 1 << 20)
    r1 = run_hip(mh, dtype, c, a, bias=bias, hm=hm, drop=drop, forward=False)
    r2 = run_hip(mh, dtype, c, a, bias=bias, hm=hm, drop=drop, forward=False)
    for t1, t2, nm in zip(r1[1:], r2[1:], ("dx", "dw", "db", "d_bias")):
        assert torch.equal(t1, t2), nm


def test_refusals(mh):
    dtype, h, a = torch.bfloat16, 128, 2
    rs = np.random.RandomState(4)
    z = lambda *shape: torch.from_numpy(rs.standard_normal(shape).astype(np.float32))
    w, b = z(3 * h, h), z(3 * h)
    with pytest.raises(ValueError, match="256"):
        run_hip(mh, dtype, (w, b, z(1, 257, h), z(1, 257, h)), a, bias=torch.zeros(1, 1, 1, 257), forward=False)
    c = (w, b, z(1, 100, h), z(1, 100, h))

    def bwd(**kw):
        x = c[2].to(dtype).cuda()
        dw, db = torch.empty(3 * h, h, device="cuda"), torch.empty(3 * h, device="cuda")
        return mh.qkv_attn_bwd(x, x, w.to(dtype).cuda(), b.cuda(), dw, db, num_heads=a, **kw)
    bias = torch.zeros(1, 1, 1, 100).cuda()
    with pytest.raises(ValueError, match="key_mask"):
        bwd(attn_bias=bias, key_mask=torch.ones(1, 100).cuda())
    with pytest.raises(ValueError, match="lse"):
        bwd(attn_bias=bias, ctx=c[2].to(dtype).cuda(), lse=torch.empty(1, a, 100, device="cuda"))
    with pytest.raises(ValueError, match="d_align"):
        bwd(attn_bias=bias, d_align=torch.zeros(1, 40, 60).cuda(), align_t=40)
    with pytest.raises(ValueError, match="broadcast"):
        bwd(attn_bias=torch.zeros(2, 1, 1, 100).cuda())
    with pytest.raises(ValueError, match="head_mask"):
        bwd(head_mask=torch.ones(3).cuda())
    with pytest.raises(ValueError, match="d_bias"):
        bwd(attn_bias=bias, d_bias=torch.empty(1, a, 100, 99, device="cuda"))


# ---- layer level: hip_autograd.BertLayerBiasFn ---------------------------------------------------------------------------------------

MODE_DT = {"bf16": torch.bfloat16, "fp32": torch.float32}
Y_TOL = {"bf16": 2e-2, "fp32": 1e-3}
G_TOL = {"bf16": 2.5e-2, "fp32": 1e-3}          # test_layer_backward_golden: bf16 gradients through one layer
Z_TOL = {"bf16": 6e-2, "fp32": 1e-3}            # ... and the analytically zero key-bias gradient, of the query-bias gradient's scale


def layer64(x, add, sd, prefix, a, hm, keeps=None, p=0.0):
    """oracle_layer (test_hip_attn_bias) with the hidden dropout masks of training mode: float64, differentiable"""
    F = torch.nn.functional
    n, s, h = x.shape
    ctx, _ = O.self_attention(x, add, sd, prefix + "attention.self.", a)
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


def check_param_grads(mode, got, ref, what):
    """got / ref: {HF parameter name (without prefix): gradient}"""
    qscale = max(1.0, float(ref["attention.self.query.bias"].abs().max()))
    for k, r in ref.items():
        g = got[k].detach().double().cpu()
        assert torch.isfinite(g).all(), k
        if k == "attention.self.key.bias":
            assert float((g - r).abs().max()) <= Z_TOL[mode] * qscale, (what, k, float((g - r).abs().max()), qscale)
            continue
        check(g, r, G_TOL[mode], "%s grad %s" % (what, k))


@pytest.mark.parametrize("mode", ["bf16", "fp32"])
@pytest.mark.parametrize("train", [False, True])
def test_layer_under_autograd(mh, mode, train):
    """BertLayerBiasFn with an [N,1,S,S] bias that requires grad and a head mask: y, dx, the 16 parameter gradients and the bias
    gradient (the dense dS summed over the heads) against float64 autograd; the same gradients through the gradient sink
    (FlatGrads, written in place) and with in_place = False"""
    from modeling import hip_autograd as ag
    from modeling import hip_layers
    from modeling import train_utils as tu
    dtype, dev = MODE_DT[mode], torch.device("cuda")
    n, s, h, a = 3, 101, 128, 2
    p = 0.1 if train else 0.0
    rs = np.random.RandomState(91)
    sdt, sd64 = layer_sd(rs, h, mode)
    x = torch.from_numpy(rs.standard_normal((n, s, h)).astype(np.float32)).to(dtype).float()
    dy = torch.from_numpy(rs.standard_normal((n, s, h)).astype(np.float32)).to(dtype).float()
    add = soft_bias(rs, (n, 1, s, s))
    hm = torch.tensor([0.5, 1.0])
    names = list(ag.BertLayerFn.NAMES)
    # float64 reference; in training mode the two hidden-dropout masks are those of DROPOUT seed 5: counters [0, M H) and [M H, 2 M H)
    keeps = None
    if train:
        m = n * s * h
        keeps = [torch.from_numpy(H.hidden_drop_keep(5, off, m, np.float32(p)).reshape(n, s, h)).double() for off in (0, m)]
    ref_p = {k: sd64[k].clone().requires_grad_(True) for k in names}
    xr, addr = x.double().requires_grad_(True), add.double().requires_grad_(True)
    y_ref = layer64(xr, addr, ref_p, "", a, hm, keeps, p)
    if not train:
        assert float((y_ref.detach() - oracle_layer(x.double(), add.double(), sd64, "", a, hm)[0]).abs().max()) < 1e-9
    (y_ref * dy.double()).sum().backward()
    ref_g = {k: v.grad for k, v in ref_p.items()}

    params = [torch.nn.Parameter(sdt[k].to(dev)) for k in names]
    packed = hip_layers.pack_layer(dict(zip(names, params)), "", dev, dtype)
    ag.set_grad_sink(None)
    ag.set_exact(mode == "fp32")
    try:
        def run():
            mh.DROPOUT.manual_seed(5)
            xg = x.to(dtype).to(dev).requires_grad_(True)
            bg = add.to(dev).requires_grad_(True)
            y = ag.BertLayerBiasFn.apply(xg, bg, hm.to(dev), None, a, 1e-12, p, 0.0, packed, *params)
            (y.float() * dy.to(dev)).sum().backward()
            torch.cuda.synchronize()
            return y, xg.grad, bg.grad
        y, dx, dbias = run()
        assert y.grad_fn is not None
        check(y, y_ref, Y_TOL[mode], "layer y")
        check(dx, xr.grad, G_TOL[mode], "layer dx")
        assert tuple(dbias.shape) == tuple(add.shape)
        check(dbias, addr.grad, G_TOL[mode], "layer d attn_bias")
        plain = {k: prm.grad.clone() for k, prm in zip(names, params)}
        check_param_grads(mode, plain, ref_g, "layer")
        for prm in params:
            prm.grad = None
        # the gradient sink: the kernels write into the flat buffer (in_place) or autograd accumulates into its views
        flat = tu.FlatGrads(params, dev, names=["encoder.layer.0." + k for k in names])
        for in_place in (True, False):
            flat.in_place = in_place
            flat.zero()
            flat.begin(1, force=False)
            _, dx2, dbias2 = run()
            flat.finish(1)
            assert torch.equal(dx2, dx) and torch.equal(dbias2, dbias)          # (no parameter gradient feeds them)
            for k, prm in zip(names, params):
                scale = max(1.0, float(plain[k].abs().max()))
                assert float((prm.grad - plain[k]).abs().max()) <= 1e-5 * scale, (in_place, k)
        # a head mask that wants a gradient, and a trainable layer beyond the backward's 256 keys: refused before any launch
        with pytest.raises(NotImplementedError, match="head_mask"):
            ag.BertLayerBiasFn.apply(x.to(dtype).to(dev), add.to(dev), hm.to(dev).requires_grad_(True), None, a, 1e-12, 0.0, 0.0, packed, *params)
        x300 = torch.zeros(1, 300, h, dtype=dtype, device=dev)
        with pytest.raises(NotImplementedError, match="256"):
            ag.BertLayerBiasFn.apply(x300, torch.zeros(1, 1, 1, 300, device=dev), None, None, a, 1e-12, 0.0, 0.0, packed, *params)
        with torch.no_grad():                               # ... while the forward alone serves it
            y300 = ag.BertLayerBiasFn.apply(x300, torch.zeros(1, 1, 1, 300, device=dev), None, None, a, 1e-12, 0.0, 0.0, packed, *params)
        assert torch.isfinite(y300.float()).all()
    finally:
        ag.set_grad_sink(None)
        ag.set_exact(False)


# ---- encoder level: trainable_encoders.encoder_layers -------------------------------------------------------------------------------

class Body(torch.nn.Module):
    """what encoder_layers looks at: .config, .encoder.layer, .training"""

    def __init__(self, cfg):
        from modeling.modeling_transfomres import CaptionBertEncoder
        super(Body, self).__init__()
        self.config = cfg
        self.encoder = CaptionBertEncoder(cfg)


def build_body(mode, nl, rs, h):
    sdt, sd64 = {}, {}
    for i in range(nl):
        t_, d_ = layer_sd(rs, h, mode, "layer.%d." % i)
        sdt.update(t_)
        sd64.update(d_)
    body = Body(small_config(mode, num_hidden_layers=nl))
    missing, unexpected = body.encoder.load_state_dict(sdt, strict=False)
    assert not unexpected, unexpected
    return body.cuda().eval(), sd64


@pytest.mark.parametrize("mode", ["bf16", "fp32"])
def test_encoder_layers_soft_mask_and_head_masks(mh, mode):
    from modeling import hip_autograd as ag
    from modeling import trainable_encoders as te
    dtype = MODE_DT[mode]
    n, s, h, a, nl = 3, 101, 128, 2, 2
    rs = np.random.RandomState(93)
    body, sd64 = build_body(mode, nl, rs, h)
    x = torch.from_numpy(rs.standard_normal((n, s, h)).astype(np.float32)).to(dtype).float()
    dy = torch.from_numpy(rs.standard_normal((n, s, h)).astype(np.float32)).to(dtype).float()
    add = soft_bias(rs, (n, 1, 1, s))
    hm = torch.tensor([[1.0, 0.5], [0.25, 1.0]])
    ref_p = {k: v.clone().requires_grad_(True) for k, v in sd64.items()}
    ref = x.double()
    for i in range(nl):
        ref = layer64(ref, add.double(), ref_p, "layer.%d." % i, a, hm[i])
    (ref * dy.double()).sum().backward()
    ag.set_grad_sink(None)
    ag.set_exact(mode == "fp32")
    try:
        out = te.encoder_layers(body, x.to(dtype).cuda(), add.cuda(), head_mask=hm.cuda())
        assert out.grad_fn is not None
        (out.float() * dy.cuda()).sum().backward()
        torch.cuda.synchronize()
    finally:
        ag.set_exact(False)
    depth = 2 if mode == "bf16" else 1
    check(out, ref, depth * Y_TOL[mode], "2-layer encoder output")
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


@pytest.mark.parametrize("mode", ["bf16", "fp32"])
def test_encoder_layers_binary_mask_keeps_its_route(mh, mode, monkeypatch):
    """a 0 / -10000 [N,1,1,S] mask without head mask: every layer goes through _run_layer(key_mask=) with the 0/1 mask, never
    through the bias form, and output, dx and the weight-matrix gradients are those of the _run_layer(key_mask=) loop bit for
    bit.  (The LayerNorm-parameter and FFN-bias gradients are accumulated by float atomics in kernels older than this route
    (csrc/rowops.hip, the GELU-gradient epilogue of csrc/gemm.hip): two runs of the SAME loop differ in their last bits, so the
    1-D gradients are held to 1e-5 of their scale, the bound the gradient-sink tests use for the same reason.)"""
    from modeling import hip_autograd as ag
    from modeling import trainable_encoders as te
    dtype = MODE_DT[mode]
    n, s, h, nl = 3, 101, 128, 2
    rs = np.random.RandomState(94)
    body, _ = build_body(mode, nl, rs, h)
    x = torch.from_numpy(rs.standard_normal((n, s, h)).astype(np.float32)).to(dtype).cuda()
    dy = torch.from_numpy(rs.standard_normal((n, s, h)).astype(np.float32)).cuda()
    km = torch.ones(n, s)
    km[1, 70:] = 0
    add = O.extend_mask(km).float().cuda()
    calls = []
    run_layer = te._run_layer
    monkeypatch.setattr(te, "_run_layer", lambda *a_, **kw: (calls.append(kw), run_layer(*a_, **kw))[1])
    monkeypatch.setattr(te, "_run_layer_bias", lambda *a_, **kw: pytest.fail("a binary mask took the bias form"))
    ag.set_grad_sink(None)
    ag.set_exact(mode == "fp32")
    try:
        res = []
        for form in ("encoder_layers", "loop"):
            body.zero_grad(set_to_none=True)
            xg = x.clone().requires_grad_(True)
            if form == "loop":
                out = xg
                for i, layer in enumerate(body.encoder.layer):
                    out = run_layer(body, i, layer, out, key_mask=km.cuda())
            else:
                out = te.encoder_layers(body, xg, add)
                assert len(calls) == nl and all(set(kw) == {"key_mask"} and torch.equal(kw["key_mask"].cpu(), km) for kw in calls)
            (out.float() * dy).sum().backward()
            torch.cuda.synchronize()
            res.append((out.detach(), xg.grad, [p_.grad.clone() for p_ in body.encoder.parameters()]))
    finally:
        ag.set_exact(False)
    (o1, d1, g1), (o2, d2, g2) = res
    assert torch.equal(o1, o2) and torch.equal(d1, d2)
    assert len(g1) == 16 * nl
    for u, v in zip(g1, g2):
        if u.dim() == 2:
            assert torch.equal(u, v)
        else:
            assert float((u - v).abs().max()) <= 1e-5 * max(1.0, float(v.abs().max()))
