"""GPU tests of the gradient of head_mask in the attention backward (modcr_qkv_attn_gate_bwd: the DHM instantiations of the cores of
csrc/attn_bias_bwd.hip behind modcr_hip.qkv_attn_bwd(d_head_mask=), hip_layers.layer_backward(want_d_head_mask=),
hip_autograd.BertLayerGateFn, trainable_encoders.encoder_layers and head_importance), P + S <= 256, bf16 and fp32.

Checker: the float64 CPU autograd references of test_hip_attn_bias_bwd (no prefix rows) and test_hip_attn_prefix_bwd (prefix rows)
with the head mask handed over as a float64 LEAF [N, A]: its .grad is
    d_hm[n, a] = sum_i dctx_i . (P'.V)_i,     P' = P o m / (1 - p),     ctx = hm P'.V
which does not depend on hm itself -- at hm = 0 every other gradient of the head is exactly 0 and this one is not.

Bounds (the repository's): max|got - ref| <= tol x max(1, max|ref|), tol = 2e-2 in bf16 and 1e-3 in fp32, for d_head_mask as for
every other quantity.  On the CPU the float64 formula with q | k | v, the scaled q and P' rounded to bf16 deviates from float64 by at
most 7.1e-3 of scale on this file's inputs (35 % of 2e-2, the head-at-zero case at (3, 101); 0.9e-3 to 5.2e-3 on the seven shapes;
max|ref| 56 to 193; the zeroed heads' reference gradients 0.95 to 193 in magnitude: tools/head_mask_grad_bounds.py ->
profiles/attn_head_mask_bwd_tolerance_report.txt).  Layer and encoder level: G_TOL of test_hip_attn_bias_bwd (2.5e-2 / 1e-3), two
layers in bf16 twice that, as the existing encoder tests take."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import helpers as H
import test_hip_attn_bias_bwd as B
import test_hip_attn_prefix_bwd as PF
from oracle import modcr_oracle as O
from test_hip_attn_bias import NEG_INF, layer_sd, soft_bias
from test_hip_attn_bias_bwd import G_TOL, MODE_DT, TOL, Y_TOL, build_body, check_param_grads, layer64
from test_hip_attn_bwd import check
from test_hip_attn_long import seq_batch

pytestmark = pytest.mark.gpu

DT = [torch.bfloat16, torch.float32]
# (n, s, p, h, a).  Without prefix rows: a partial tile; S % 4 != 0; the MFMA core's edge; the first bf16 shape on the exact core; the limit.
# With prefix rows: a few prefix keys; L = 193, the exact core.
SHAPES = [(3, 37, 0, 128, 2), (3, 101, 0, 128, 2), (2, 192, 0, 128, 2), (2, 193, 0, 256, 4), (1, 256, 0, 128, 2),
          (2, 120, 8, 128, 2), (2, 150, 43, 128, 2)]
DROPS = {"p=0": None, "p=0.2": (0.2, 77, 5 << 32)}


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


def case(shape):
    n, s, p, h, a = shape
    return PF.case(n, s, p, h, a) if p else B.case(n, s, h, a)


def mask_0_1(n, a, seed):
    """a head mask [N, A] that holds a 0 (first sequence, first head) and a 1 (last sequence, last head), uniform values elsewhere"""
    hm = torch.from_numpy(np.random.RandomState(seed).uniform(0.1, 0.9, size=(n, a)).astype(np.float32))
    hm[0, 0], hm[-1, -1] = 0.0, 1.0
    return hm


def reference(shape, bias, hm, drop=None, cid=None):
    """the two files' float64 references with hm [N, A] as a leaf: their tuple as it is + d_hm [N, A]; without
    prefix rows a None stands at d_hist's place, so both read (ctx, dx, d_hist, dWqkv, dbqkv, dS, d_hm)"""
    n, s, p, h, a = shape
    leaf = hm.double().clone().requires_grad_(True)
    if p:
        assert cid is None
        r = list(PF.reference(case(shape), a, bias, leaf, drop))
    else:
        r = list(B.reference(case(shape), a, bias, leaf, cid=cid, drop=drop))
        r.insert(2, None)
    assert tuple(leaf.grad.shape) == (n, a) and torch.isfinite(leaf.grad).all()
    return r + [leaf.grad]


@functools.lru_cache(maxsize=None)
def soft_case(shape, drop_key):
    """bias [N,1,S,L] (10 % -10000, 10 % -inf), head mask with a 0 and a 1, and their reference: shared by both dtypes, read-only"""
    n, s, p, h, a = shape
    bias = soft_bias(np.random.RandomState(s + p), (n, 1, s, p + s))
    hm = mask_0_1(n, a, s)
    return bias, hm, reference(shape, bias, hm, DROPS[drop_key])


def run_hip(mh, dtype, shape, bias=None, hm=None, drop=None, cid=None, want_d_hm=True, forward=False):
    """qkv_attn_bwd(d_head_mask=) on NaN-prefilled outputs -> (ctx or None, dx, d_hist or None, dw, db, d_bias or None, d_hm or None);
    a head mask that already lives on the GPU is handed over as it is"""
    n, s, p, h, a = shape
    c = case(shape)
    w, b, x = c[0], c[1], c[2]
    hist, dctx = (c[3], c[4]) if p else (None, c[3])
    xd, wd, bd = x.to(dtype).cuda(), w.to(dtype).cuda(), b.cuda()
    hd = None if hist is None else hist.to(dtype).cuda()
    bias_d = None if bias is None else bias.cuda()
    hm_d = None if hm is None else hm.cuda()
    cid_d = None if cid is None else cid.cuda()
    ctx = None
    if forward:
        ctx, _ = mh.qkv_attn(xd, wd, bd, hist=hd, chunk_id=cid_d, num_heads=a, attn_dropout=drop, attn_bias=bias_d, head_mask=hm_d)
    nan = lambda *sh: torch.full(sh, float("nan"), device="cuda")
    dw, db = nan(3 * h, h), nan(3 * h)
    d_bias = nan(n, a, s, p + s) if bias is not None else None
    d_hm = nan(n, a) if want_d_hm else None
    kw = dict(d_head_mask=d_hm) if want_d_hm else {}
    out = mh.qkv_attn_bwd(dctx.to(dtype).cuda(), xd, wd, bd, dw, db, chunk_id=cid_d, num_heads=a, attn_dropout=drop, attn_bias=bias_d,
                          head_mask=hm_d, d_bias=d_bias, hist=hd, **kw)
    torch.cuda.synchronize()
    dx, d_hist = out if p else (out, None)
    return ctx, dx, d_hist, dw, db, d_bias, d_hm


def check_all(dtype, got, ref, what, shape):
    """d_head_mask and every other quantity against the reference at the file's bound"""
    n, s, p, h, a = shape
    tol = TOL[dtype]
    assert got[6].dtype == torch.float32 and tuple(got[6].shape) == (n, a)
    check(got[6], ref[6], tol, what + " d_head_mask")
    if p:
        PF.check_all(dtype, got[:6], ref[:6], what, n, s, h)
    else:
        B.check_all(dtype, got[:2] + got[3:6], ref[:2] + ref[3:6], what, n, s, h)


def want_core(dtype, shape):
    return "mfma" if dtype == torch.bfloat16 and shape[1] + shape[2] <= 192 else "exact"


# ---- 1. entry level: every shape class, both cores, with and without prefix rows and dropout -------------------------------------

@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("drop", list(DROPS))
@pytest.mark.parametrize("shape", SHAPES)
def test_shapes_and_cores(mh, dtype, drop, shape):
    n, s, p, h, a = shape
    assert mh.qkv_attn_gate_bwd_route(n, s, p, h, a, mdt(mh, dtype)) == want_core(dtype, shape)
    bias, hm, ref = soft_case(shape, drop)
    assert float(hm.min()) == 0.0 and float(hm.max()) == 1.0
    got = run_hip(mh, dtype, shape, bias=bias, hm=hm, drop=DROPS[drop], forward=True)
    check_all(dtype, list(got), ref, "S=%d P=%d %s" % (s, p, drop), shape)


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[3], SHAPES[5], SHAPES[6]])
def test_a_head_at_zero_keeps_its_gradient(mh, dtype, shape):
    """hm = 0 on head 0 of every sequence: its d_head_mask is the reference's, which is far from 0, while the dq | dk | dv-fed rows of
    dWqkv and dbqkv and its d_bias are exactly 0 as before.  (A gradient formed as delta / hm, or from the hm-scaled delta, fails
    here: it is NaN or 0.)  Then hm = 0 on EVERY head: the reference's d_head_mask is the same tensor (it does not depend on hm) and
    has to be met with nothing but zeros in every other output."""
    n, s, p, h, a = shape
    rs = np.random.RandomState(23 + s)
    bias = soft_bias(rs, (n, 1, s, p + s))
    hm = torch.from_numpy(rs.uniform(0.25, 1.0, size=(n, a)).astype(np.float32))
    hm[:, 0] = 0.0
    ref = reference(shape, bias, hm)
    zero_ref = ref[6][:, 0]
    assert float(zero_ref.abs().max()) > 0.5, zero_ref
    got = run_hip(mh, dtype, shape, bias=bias, hm=hm, forward=True)
    check_all(dtype, list(got), ref, "head 0 at 0", shape)
    scale = max(1.0, float(ref[6].abs().max()))
    err0 = float((got[6][:, 0].cpu().double() - zero_ref).abs().max())
    H.report_use("head 0 at 0: its own d_head_mask", err0 / scale, TOL[dtype])
    assert err0 <= TOL[dtype] * scale
    ctx, dw, db, d_bias = got[0], got[3], got[4], got[5]
    for part in range(3):
        assert (dw[part * h:part * h + 64] == 0).all() and (db[part * h:part * h + 64] == 0).all()
    assert (d_bias[:, 0] == 0).all() and (ctx[:, :, :64] == 0).all()
    allz = run_hip(mh, dtype, shape, bias=bias, hm=torch.zeros(n, a))
    check(allz[6], ref[6], TOL[dtype], "every head at 0: d_head_mask")
    for t, nm in zip((allz[1], allz[2], allz[3], allz[4], allz[5]), ("dx", "d_hist", "dw", "db", "d_bias")):
        assert t is None or (t == 0).all(), nm


@pytest.mark.parametrize("dtype", DT)
def test_forms(mh, dtype):
    n, s, p, h, a = shape = SHAPES[1]
    rs = np.random.RandomState(31)
    bias = soft_bias(rs, (n, 1, s, s))
    # head_mask [A] (sequence stride 0): d_head_mask stays [N, A], the reference takes the mask expanded
    hm_a = torch.tensor([0.0, 1.0])
    got = run_hip(mh, dtype, shape, bias=bias, hm=hm_a, forward=True)
    check_all(dtype, list(got), reference(shape, bias, hm_a.expand(n, a)), "head mask [A]", shape)
    hm_na = mask_0_1(n, a, 5)
    ref_na = reference(shape, bias, hm_na)
    check_all(dtype, list(run_hip(mh, dtype, shape, bias=bias, hm=hm_na, forward=True)), ref_na, "head mask [N,A]", shape)
    check_all(dtype, list(run_hip(mh, dtype, shape, bias=bias, hm=hm_na.reshape(n, a, 1, 1), forward=True)), ref_na, "head mask [N,A,1,1]", shape)
    # head_mask = None with d_head_mask: the run with a mask of ones, bit for bit -- with and without a bias (bias alone)
    ones = torch.ones(n, a)
    for bs, nm in ((bias, "bias alone"), (None, "neither bias nor head mask")):
        none, one = run_hip(mh, dtype, shape, bias=bs), run_hip(mh, dtype, shape, bias=bs, hm=ones)
        for t1, t2 in zip(none[1:], one[1:]):
            assert (t1 is None and t2 is None) or torch.equal(t1, t2), nm
        check_all(dtype, list(none), reference(shape, bs, ones), nm, shape)
    # head mask alone
    check_all(dtype, list(run_hip(mh, dtype, shape, hm=hm_na, forward=True)), reference(shape, None, hm_na), "head mask alone", shape)


@pytest.mark.parametrize("dtype", DT)
def test_chunk_mean_queries(mh, dtype):
    """a seq_enc-shaped call (T = 60, R = 41) without prefix rows: the phase-3 additive mask with a soft term on top"""
    n, t, r, h, a = 3, 60, 41, 128, 2
    s = t + r
    shape = (n, s, 0, h, a)
    rs = np.random.RandomState(60)
    im, cm, gi, cid = seq_batch(rs, n, t, r)
    add = O.seq_phase_mask(im.double(), cm.double(), t, r, 3).float() + torch.from_numpy(rs.standard_normal((n, 1, s, s)).astype(np.float32))
    hm = mask_0_1(n, a, 61)
    check_all(dtype, list(run_hip(mh, dtype, shape, bias=add, hm=hm, cid=cid, forward=True)), reference(shape, add, hm, cid=cid), "phase 3", shape)


@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[5]])
def test_identity_with_the_forward_s_context(mh, shape):
    """fp32, p = 0, a mask of ones: d_head_mask[n, a] = sum_i dctx[n, i, 64a:64a+64] . ctx[n, i, 64a:64a+64] of the forward's OWN ctx --
    no reference, no recomputation on the host"""
    n, s, p, h, a = shape
    bias = soft_bias(np.random.RandomState(41), (n, 1, s, p + s))
    got = run_hip(mh, torch.float32, shape, bias=bias, hm=torch.ones(n, a), forward=True)
    dctx = case(shape)[-1].double()
    want = (got[0].cpu().double() * dctx).view(n, s, a, 64).sum((1, 3))
    check(got[6], want, 1e-3, "d_head_mask = sum dctx . ctx")


@pytest.mark.parametrize("dtype,shape", [(torch.bfloat16, SHAPES[1]), (torch.bfloat16, SHAPES[3]), (torch.float32, SHAPES[1]),
                                         (torch.bfloat16, SHAPES[5]), (torch.bfloat16, SHAPES[6]), (torch.float32, SHAPES[5])])
def test_nothing_else_moves(mh, dtype, shape):
    """dx, d_hist, dWqkv, dbqkv and d_bias of a call with d_head_mask are those of the same call without it, bit for bit: both
    cores, with and without prefix rows, under dropout"""
    bias, hm, _ = soft_case(shape, "p=0.2")
    drop = DROPS["p=0.2"]
    with_, without = run_hip(mh, dtype, shape, bias=bias, hm=hm, drop=drop), run_hip(mh, dtype, shape, bias=bias, hm=hm, drop=drop, want_d_hm=False)
    assert without[6] is None and torch.isfinite(with_[6]).all()
    for t1, t2, nm in zip(with_[1:6], without[1:6], ("dx", "d_hist", "dw", "db", "d_bias")):
        assert (t1 is None and t2 is None) or torch.equal(t1, t2), nm


@pytest.mark.parametrize("dtype,s", [(torch.bfloat16, 180), (torch.bfloat16, 230), (torch.float32, 101)])
def test_two_launches_are_bit_identical(mh, dtype, s):
    """every element of the NaN-prefilled d_head_mask is written, and two launches agree in every bit (one lane per element, a fixed
    summation order, no atomics)"""
    n, h, a = 2 if s > 101 else 3, 128, 2
    shape = (n, s, 0, h, a)
    bias = soft_bias(np.random.RandomState(2), (n, a, s, s))
    hm = torch.tensor([0.0, 1.0])
    drop = (0.2, 9, 1 << 20)
    r1 = run_hip(mh, dtype, shape, bias=bias, hm=hm, drop=drop)
    r2 = run_hip(mh, dtype, shape, bias=bias, hm=hm, drop=drop)
    assert torch.isfinite(r1[6]).all() and float(r1[6].abs().min()) > 0
    for t1, t2, nm in zip(r1[1:], r2[1:], ("dx", "d_hist", "dw", "db", "d_bias", "d_head_mask")):
        assert (t1 is None and t2 is None) or torch.equal(t1, t2), nm


@pytest.mark.parametrize("dtype", DT)
def test_rows_of_minus_infinity_add_nothing(mh, dtype):
    """a query row whose every key is -inf contributes 0: the reference runs on a finite stand-in with dctx zeroed on those rows"""
    n, s, p, h, a = shape = SHAPES[1]
    c = case(shape)
    bias = soft_bias(np.random.RandomState(5), (n, a, s, s))
    bias[1, 0, 5, :] = NEG_INF
    bias[2, :, 70, :] = NEG_INF
    got = run_hip(mh, dtype, shape, bias=bias, hm=mask_0_1(n, a, 7))
    assert all(t is None or torch.isfinite(t.float()).all() for t in got)
    fin, dz = bias.clone(), c[3].clone()
    fin[1, 0, 5, :] = 0
    fin[2, :, 70, :] = 0
    dz[1, 5, :64] = 0
    dz[2, 70] = 0
    leaf = mask_0_1(n, a, 7).double().requires_grad_(True)
    B.reference(c, a, fin, leaf, dctx=dz)
    check(got[6], leaf.grad, TOL[dtype], "all -inf rows d_head_mask")


def test_refusals(mh):
    """before any launch: the outputs keep their NaN prefill"""
    dtype, h, a = torch.bfloat16, 128, 2
    dt = mdt(mh, dtype)
    lib = mh.lib()
    f = lambda *sh, **kw: torch.full(sh, float("nan"), device="cuda", **kw)
    ptr = lambda v: None if v is None else ctypes.c_void_p(v.data_ptr())

    def raw(n, s, p, cid=None, hist_given=None):
        hist_given = p > 0 if hist_given is None else hist_given
        x, dctx, hist = (torch.zeros(n, r, h, dtype=dtype, device="cuda") for r in (s, s, max(p, 1)))
        w, b = torch.zeros(3 * h, h, dtype=dtype, device="cuda"), torch.zeros(3 * h, device="cuda")
        bias = torch.zeros(n, 1, 1, p + s, device="cuda")
        outs = [f(n, s, h, dtype=dtype), f(n, max(p, 1), h, dtype=dtype), f(3 * h, h), f(3 * h), f(n, a, s, p + s), f(n, a)]
        ws = torch.empty(1 << 24, dtype=torch.uint8, device="cuda")
        rc = lib.modcr_qkv_attn_gate_bwd(ptr(dctx), ptr(x), ptr(hist) if hist_given else None, ptr(w), ptr(b), ptr(bias), p + s, 0, 0, None, 0,
                                         ptr(cid), 0 if cid is None else cid.shape[1], None, ptr(outs[0]), ptr(outs[1]) if hist_given else None,
                                         ptr(outs[2]), ptr(outs[3]), 0, ptr(outs[4]), ptr(outs[5]), n, s, p, h, a, 0.0, 0, 0, ptr(ws),
                                         ws.numel(), dt, None)
        msg = lib.modcr_last_error()
        torch.cuda.synchronize()
        assert all(torch.isnan(t.float()).all() for t in outs), "a refused call wrote an output"
        return rc, msg
    for s, p in ((257, 0), (247, 10), (1, 256)):
        rc, msg = raw(1, s, p)
        assert rc == -3 and b"256" in msg and b"qkv_attn_gate_bwd" in msg, (s, p, rc, msg)
    cid = torch.zeros(1, 4, dtype=torch.int32, device="cuda")
    rc, msg = raw(1, 100, 10, cid=cid)
    assert rc == -1 and b"chunk-mean" in msg, msg
    rc, msg = raw(1, 100, 10, hist_given=False)
    assert rc == -1 and b"prefix rows" in msg, msg
    rc, msg = raw(1, 100, 0, hist_given=True)
    assert rc == -1 and b"prefix rows" in msg, msg

    # the Python wrapper
    n, s = 2, 100
    x = torch.zeros(n, s, h, dtype=dtype, device="cuda")
    w, b = torch.zeros(3 * h, h, dtype=dtype, device="cuda"), torch.zeros(3 * h, device="cuda")
    dw, db = f(3 * h, h), f(3 * h)
    hm = torch.ones(a, device="cuda")
    bwd = lambda **kw: mh.qkv_attn_bwd(x, x, w, b, dw, db, num_heads=a, head_mask=hm, **kw)
    for bad in (f(a), f(n, a + 1), f(n, a, 1, 1), f(n, a, dtype=torch.float64), f(n, a, dtype=torch.bfloat16), f(a, n).t(), f(n, 2 * a)[:, ::2],
                torch.full((n, a), float("nan"))):
        with pytest.raises(ValueError, match="d_head_mask"):
            bwd(d_head_mask=bad)
        assert torch.isnan(bad.float()).all()
    with pytest.raises(ValueError, match="chunk_id"):
        bwd(d_head_mask=f(n, a), hist=torch.zeros(n, 10, h, dtype=dtype, device="cuda"), chunk_id=torch.zeros(n, 4, dtype=torch.int32, device="cuda"))
    x257 = torch.zeros(1, 257, h, dtype=dtype, device="cuda")
    with pytest.raises(ValueError, match="256"):
        mh.qkv_attn_bwd(x257, x257, w, b, dw, db, num_heads=a, head_mask=hm, d_head_mask=f(1, a))
    torch.cuda.synchronize()
    assert torch.isnan(dw).all() and torch.isnan(db).all()


# ---- 2. layer level: hip_autograd.BertLayerGateFn ----------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["bf16", "fp32"])
@pytest.mark.parametrize("n,s,p", [(2, 101, 0), (2, 90, 12)])
def test_gate_layer_under_autograd(mh, mode, n, s, p):
    """x, hist, the [N,1,S,L] bias, the [N, A] head mask (holding a 0 and a 1) and the 16 parameters against float64 autograd of
    layer64 / layer64p with hm a leaf; the head mask in the forms [A] and [1,A,1,1] receives the gradient summed over N, in its own
    shape; through the gradient sink the same gradients arrive"""
    from modeling import hip_autograd as ag
    from modeling import hip_layers
    from modeling import train_utils as tu
    dtype, dev = MODE_DT[mode], torch.device("cuda")
    h, a = 128, 2
    rs = np.random.RandomState(191 + s)
    sdt, sd64 = layer_sd(rs, h, mode)
    rnd = lambda *shape: torch.from_numpy(rs.standard_normal(shape).astype(np.float32)).to(dtype).float()
    x, dy = rnd(n, s, h), rnd(n, s, h)
    hist = rnd(n, p, h) if p else None
    add = soft_bias(rs, (n, 1, s, p + s))
    hm = mask_0_1(n, a, s)
    names = list(ag.BertLayerFn.NAMES)

    def ref_run(hm_leaf):
        ref_p = {k: sd64[k].clone().requires_grad_(True) for k in names}
        xr, addr = x.double().requires_grad_(True), add.double().requires_grad_(True)
        hr = hist.double().requires_grad_(True) if p else None
        y = PF.layer64p(xr, hr, addr, ref_p, "", a, hm_leaf) if p else layer64(xr, addr, ref_p, "", a, hm_leaf)
        (y * dy.double()).sum().backward()
        return y.detach(), xr.grad, None if hr is None else hr.grad, addr.grad, hm_leaf.grad, {k: v.grad for k, v in ref_p.items()}
    y_ref, dx_ref, dh_ref, dadd_ref, dhm_ref, ref_g = ref_run(hm.double().requires_grad_(True))
    assert float(dhm_ref[0, 0].abs()) > 1e-3            # (the head at 0 has a gradient of its own)

    params = [torch.nn.Parameter(sdt[k].to(dev)) for k in names]
    packed = hip_layers.pack_layer(dict(zip(names, params)), "", dev, dtype)
    ag.set_grad_sink(None)
    ag.set_exact(mode == "fp32")
    try:
        def run(mask):
            xg = x.to(dtype).to(dev).requires_grad_(True)
            hg = hist.to(dtype).to(dev).requires_grad_(True) if p else None
            bg = add.to(dev).requires_grad_(True)
            mg = mask.to(dev).requires_grad_(True)
            y = ag.BertLayerGateFn.apply(xg, hg, bg, mg, None, a, 1e-12, 0.0, 0.0, packed, *params)
            (y.float() * dy.to(dev)).sum().backward()
            torch.cuda.synchronize()
            return y, xg.grad, None if hg is None else hg.grad, bg.grad, mg.grad
        y, dx, dh, dadd, dhm = run(hm)
        what = "gate layer S=%d P=%d" % (s, p)
        check(y, y_ref, Y_TOL[mode], what + " y")
        check(dx, dx_ref, G_TOL[mode], what + " dx")
        if p:
            assert dh.dtype == dtype
            check(dh, dh_ref, G_TOL[mode], what + " d_hist")
        assert tuple(dadd.shape) == tuple(add.shape)
        check(dadd, dadd_ref, G_TOL[mode], what + " d attn_bias")
        assert tuple(dhm.shape) == (n, a) and dhm.dtype == torch.float32
        check(dhm, dhm_ref, G_TOL[mode], what + " d head_mask")
        plain = {k: prm.grad.clone() for k, prm in zip(names, params)}
        check_param_grads(mode, plain, ref_g, what)
        # a mask broadcast over N: the gradient is summed over N and has the mask's shape
        for form in ((a,), (1, a, 1, 1)):
            m1 = torch.tensor([0.0, 1.0])
            r1 = ref_run(m1.double().expand(n, a).clone().requires_grad_(True))
            g1 = run(m1.reshape(form))[4]
            assert tuple(g1.shape) == form
            check(g1.reshape(a), r1[4].sum(0), G_TOL[mode], what + " d head_mask %s" % (form,))
        for prm in params:
            prm.grad = None
        # the gradient sink
        flat = tu.FlatGrads(params, dev, names=["encoder.layer.0." + k for k in names])
        flat.in_place = True
        flat.zero()
        flat.begin(1, force=False)
        _, dx2, _, dadd2, dhm2 = run(hm)
        flat.finish(1)
        assert torch.equal(dx2, dx) and torch.equal(dadd2, dadd) and torch.equal(dhm2, dhm)
        for k, prm in zip(names, params):
            assert float((prm.grad - plain[k]).abs().max()) <= 1e-5 * max(1.0, float(plain[k].abs().max())), k
        # a constant head mask in the gate function: no gradient slot is filled, the others are what they were
        xg = x.to(dtype).to(dev).requires_grad_(True)
        hg = hist.to(dtype).to(dev) if p else None
        y3 = ag.BertLayerGateFn.apply(xg, hg, add.to(dev), hm.to(dev), None, a, 1e-12, 0.0, 0.0, packed, *params)
        (y3.float() * dy.to(dev)).sum().backward()
        assert torch.equal(y3, y) and torch.equal(xg.grad, dx)
    finally:
        ag.set_grad_sink(None)
        ag.set_exact(False)


# ---- 3. encoder level: trainable_encoders.encoder_layers, head_importance -----------------------------------------------------------

@pytest.mark.parametrize("mode", ["bf16", "fp32"])
def test_encoder_layers_head_mask_gradient_and_head_importance(mh, mode):
    from modeling import hip_autograd as ag
    from modeling import trainable_encoders as te
    dtype = MODE_DT[mode]
    n, s, h, a, nl = 3, 101, 128, 2, 2
    rs = np.random.RandomState(193)
    body, sd64 = build_body(mode, nl, rs, h)
    x = torch.from_numpy(rs.standard_normal((n, s, h)).astype(np.float32)).to(dtype).float()
    dy = torch.from_numpy(rs.standard_normal((n, s, h)).astype(np.float32)).to(dtype).float()
    add = soft_bias(rs, (n, 1, 1, s))
    hm = torch.tensor([[1.0, 0.0], [0.25, 1.0]])

    def ref_run(mask):
        leaf = mask.double().clone().requires_grad_(True)
        ref = x.double()
        for i in range(nl):
            ref = layer64(ref, add.double(), sd64, "layer.%d." % i, a, leaf[i])
        (ref * dy.double()).sum().backward()
        return ref.detach(), leaf.grad
    depth = 2 if mode == "bf16" else 1
    loss_fn = lambda out: (out.float() * dy.cuda()).sum()
    ag.set_grad_sink(None)
    ag.set_exact(mode == "fp32")
    try:
        def run(mask):
            body.zero_grad(set_to_none=True)
            mg = mask.cuda().requires_grad_(True)
            out = te.encoder_layers(body, x.to(dtype).cuda(), add.cuda(), head_mask=mg)
            loss_fn(out).backward()
            torch.cuda.synchronize()
            return out, mg.grad
        out, g = run(hm)
        out_ref, g_ref = ref_run(hm)
        assert tuple(g.shape) == (nl, a) and g.dtype == torch.float32
        check(out, out_ref, depth * Y_TOL[mode], "2-layer encoder output")
        check(g, g_ref, depth * G_TOL[mode], "encoder head_mask.grad")
        assert all(prm.grad is not None for prm in body.encoder.parameters())
        # head importance: |grad| at a mask of ones, the parameters frozen inside the call only
        _, g1 = run(torch.ones(nl, a))
        check(g1, ref_run(torch.ones(nl, a))[1], depth * G_TOL[mode], "encoder head_mask.grad at ones")
        body.zero_grad(set_to_none=True)
        prms = list(body.parameters())
        prms[3].requires_grad_(False)
        flags = [prm.requires_grad for prm in prms]
        imp = te.head_importance(body, x.to(dtype).cuda(), add.cuda(), loss_fn)
        torch.cuda.synchronize()
        assert tuple(imp.shape) == (nl, a) and imp.dtype == torch.float32 and not imp.requires_grad
        assert torch.equal(imp, g1.abs())
        assert [prm.requires_grad for prm in prms] == flags and all(prm.grad is None for prm in prms)
        # ... and it is restored when the loss raises
        with pytest.raises(ZeroDivisionError):
            te.head_importance(body, x.to(dtype).cuda(), add.cuda(), lambda out: 1 // 0)
        assert [prm.requires_grad for prm in prms] == flags
        prms[3].requires_grad_(True)
        # with history states the scores are those of autograd through the same layers
        hists = [torch.from_numpy(rs.standard_normal((n, 10, h)).astype(np.float32)).to(dtype).cuda() for _ in range(nl)]
        addp = soft_bias(rs, (n, 1, 1, 10 + s)).cuda()
        imp_p = te.head_importance(body, x.to(dtype).cuda(), addp, loss_fn, encoder_history_states=hists)
        mg = torch.ones(nl, a, device="cuda", requires_grad=True)
        loss_fn(te.encoder_layers(body, x.to(dtype).cuda(), addp, head_mask=mg, encoder_history_states=hists)).backward()
        assert torch.equal(imp_p, mg.grad.abs()) and float(imp_p.min()) > 0
    finally:
        ag.set_exact(False)


def test_encoder_layers_only_a_mask_that_requires_grad_takes_the_gate_route(mh, monkeypatch):
    """per layer: head_mask[i] requires grad -> BertLayerGateFn; a constant head mask, no head mask, a history state with a constant
    mask, and every layer under torch.no_grad() run as before (counted calls)"""
    from modeling import hip_autograd as ag
    from modeling import trainable_encoders as te
    mode, dtype = "bf16", torch.bfloat16
    n, s, h, a, nl = 2, 37, 128, 2, 2
    rs = np.random.RandomState(194)
    body, _ = build_body(mode, nl, rs, h)
    x = torch.from_numpy(rs.standard_normal((n, s, h)).astype(np.float32)).to(dtype).cuda()
    add = soft_bias(rs, (n, 1, 1, s)).cuda()
    calls = []
    for name in ("_run_layer", "_run_layer_bias", "_run_layer_prefix", "_run_layer_gate"):
        orig = getattr(te, name)
        monkeypatch.setattr(te, name, (lambda nm, fn: lambda *a_, **kw: (calls.append(nm), fn(*a_, **kw))[1])(name, orig))
    ag.set_grad_sink(None)

    def routes(**kw):
        del calls[:]
        out = te.encoder_layers(body, x, add, **kw)
        return out, list(calls)
    grad_hm, const_hm = torch.tensor([0.5, 1.0], device="cuda", requires_grad=True), torch.tensor([0.5, 1.0], device="cuda")
    out_g, r = routes(head_mask=[grad_hm, const_hm])
    assert r == ["_run_layer_gate", "_run_layer_bias"]
    out_c, r = routes(head_mask=[const_hm, const_hm])
    assert r == ["_run_layer_bias", "_run_layer_bias"]
    assert torch.equal(out_g, out_c)                      # (the forward is the same arithmetic)
    assert routes(head_mask=[None, grad_hm])[1][1] == "_run_layer_gate"
    assert "_run_layer_gate" not in routes()[1] and "_run_layer_gate" not in routes(head_mask=[None, None])[1]
    with torch.no_grad():
        assert routes(head_mask=[grad_hm, grad_hm])[1] == ["_run_layer_bias", "_run_layer_bias"]
    hist = torch.zeros(n, 5, h, dtype=dtype, device="cuda")
    addp = soft_bias(rs, (n, 1, 1, 5 + s)).cuda()
    del calls[:]
    te.encoder_layers(body, x, addp, head_mask=[const_hm, grad_hm], encoder_history_states=[hist, hist])
    assert calls == ["_run_layer_prefix", "_run_layer_gate"]
    # the older layer functions keep their refusal
    with pytest.raises(NotImplementedError, match="head_mask"):
        te._run_layer_bias(body, 0, body.encoder.layer[0], x, add, grad_hm)
