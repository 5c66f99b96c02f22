"""GPU tests of the opt-in dense mask bits and align-map gradient from 257 to 512 keys (modcr_qkv_attn_long_align_fwd / _bwd: the BITS
instantiations of the streaming forward core and the MASK / DALIGN instantiations of the streaming backward cores, behind
modcr_hip.qkv_attn(dense_bits=) / qkv_attn_long_bwd(dense_bits=, d_align=, align_t=, side_post_dropout=),
hip_layers.layer_forward_train(long_align=), hip_autograd.set_long_backward(True, align=True) and seq_encoder), bf16 and fp32.

Reference: float64 autograd over the inputs rounded to the storage dtype, the bits as a 0 / -10000 additive mask (oracle.seq_phase_mask,
held equal to modcr_build_phase_mask's bits), the host keep mask of tests/attn_wide_drop.py, the align map as a differentiable output
with a seeded N(0, 1) d_align.  Bounds, the repository's (test_hip_attn_long_bwd.check_all): max|got - ref| <= tol x max(1, max|ref|),
tol = 2e-2 in bf16 and 1e-3 in fp32, for ctx, align_map, dx, dWqkv, dbqkv, d_bias, d_head_mask; relative L2 < 2e-2 for dx and dWqkv in
bf16.  Layer level: y 2e-2 / 1e-3, gradients 2.5e-2 / 1e-3.  tools/attn_long_bwd_tolerance.py --align restates the bf16 arithmetic
on the CPU (profiles/attn_long_align_tolerance_report.txt).

Shapes (N, S, T): one key in the fifth tile; T and R off every 16 / 64 boundary; the limit; R = 1 (the scalar d_align loads); four
heads with chunk-mean queries, the text block inside one tile and the region keys over four."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import attn_wide_drop as W
import helpers as H
import test_hip_attn_bias_bwd as B
import test_hip_attn_long_bwd as LB
import test_hip_attn_prefix_bwd as PF
from oracle import modcr_oracle as O
from test_hip_attn_bias_bwd import G_TOL, MODE_DT, TOL, Y_TOL, check_param_grads
from test_hip_attn_bwd import check, chunk_mean_device
from test_hip_attn_long import seq_batch

pytestmark = pytest.mark.gpu

DT = [torch.bfloat16, torch.float32]
SHAPES = [(2, 257, 200, 128, 2), (2, 300, 229, 128, 2), (1, 512, 450, 128, 2), (1, 258, 257, 128, 2)]
CHUNK_SHAPE = (2, 320, 64, 256, 4)
DROP = (0.1, 77, 5 << 32)
NEG = -10000.0


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
def batch(shape):
    """ragged chunk masks with padded text and padded region slots in EVERY sequence (seq_batch's first sequence is full: dropped),
    chunk ids, and the case's rows (w, b, x, dctx) with a seeded N(0, 1) d_align (unit variance everywhere)"""
    n, s, t, h, a = shape
    rs = np.random.RandomState(1000 + s + t)
    im, cm, _, cid = seq_batch(rs, n + 1, t, s - t)
    g = torch.from_numpy(rs.standard_normal((n, t, s - t)).astype(np.float32))
    c = LB.case((n, s, 0, h, a))
    if s - t == 1:
        # R = 1: d_head_mask = sum_i dctx_i . (P.V)_i is a sum of 258 terms of either sign (|sum| ~ 10 of terms ~ 1), and with the
        # case's +-10 scores the bf16 q | k rows move every probability by percents: the number formats alone predict 1.05-1.16 of
        # that bound (profiles/attn_long_align_tolerance_report.txt, first pass; scaling dctx does not help, the sum scales with it).
        # The bound stays; this case takes test_hip_attn_long_drop.flat_case's rows instead: the query projection scaled so that
        # the scores' standard deviation is 0.4
        import test_hip_attn_long_drop as D
        c = D.flat_case((n, s, 0, h, a))[0]
    return im[1:].contiguous(), cm[1:].contiguous(), cid[1:].contiguous(), c, g


@functools.lru_cache(maxsize=None)
def phase_add(shape, phase):
    """the additive 0 / -10000 mask [N, 1, S, S] of a phase, with one query row hidden everywhere (a text row; in phase 3 a region row too)"""
    n, s, t, h, a = shape
    im, cm = batch(shape)[:2]
    add = O.seq_phase_mask(im.double(), cm.double(), t, s - t, phase).float()
    add[0, 0, 5, :] = NEG
    if phase == 3:
        add[n - 1, 0, s - 1, :] = NEG
    return add


def bits_of(mh, shape, phase):
    """modcr_build_phase_mask's bits with the same rows cleared; held equal to phase_add bit for bit"""
    n, s, t, h, a = shape
    im, cm = batch(shape)[:2]
    bits = mh.build_phase_mask(im.cuda(), cm.cuda(), phase)
    bits[0, 5, :] = 0
    if phase == 3:
        bits[n - 1, s - 1, :] = 0
    bn = bits.cpu().numpy().view(np.uint32)
    j = np.arange(s)
    see = torch.from_numpy(((bn[:, :, j // 32] >> (j % 32).astype(np.uint32)) & 1).astype(bool))
    assert torch.equal(see, phase_add(shape, phase)[:, 0] == 0), "phase %d mask bits" % phase
    assert not see[0, 5].any(), "a query row hidden everywhere"
    return bits


def reference(shape, add, hm, drop=None, cid=None, post=False, with_align=True):
    """float64 autograd -> (ctx, dx, None, dWqkv, dbqkv, dS [N, A, S, S], d_hm, align_map); add: the whole additive term (bits as
    0 / -10000 plus any bias), hm [N, A]"""
    n, s, t, h, a = shape
    w, b, x, dctx = batch(shape)[3]
    g = batch(shape)[4]
    xr, wr, br = (v.double().clone().requires_grad_(True) for v in (x, w, b))
    dense = (torch.zeros(n, a, s, s, dtype=torch.float64) + add.double()).requires_grad_(True)
    leaf = hm.double().clone().requires_grad_(True)
    qkv = torch.nn.functional.linear(xr, wr, br)
    q, k, v = qkv[..., :h], qkv[..., h:2 * h], qkv[..., 2 * h:]
    if cid is not None:
        q = chunk_mean_device(q, cid.long())
    sp = lambda z: z.view(n, s, a, 64).transpose(1, 2)
    probs = torch.softmax(sp(q) @ sp(k).transpose(-1, -2) / 8.0 + dense, -1)
    pt = probs
    if drop is not None:
        pt = probs * W.keep_of_call(n, a, s, 0, drop).double() / (1.0 - drop[0])
    hm4 = leaf[:, :, None, None]
    ctx = (hm4 * (pt @ sp(v))).transpose(1, 2).reshape(n, s, h)
    side = pt if (post and drop is not None) else probs
    amap = (hm4 * side)[:, :, :t, t:].sum(1)
    loss = (ctx * dctx.double()).sum()
    if with_align:
        loss = loss + (amap * g.double()).sum()
    loss.backward()
    out = [ctx.detach(), xr.grad, None, wr.grad, br.grad, dense.grad, leaf.grad, amap.detach()]
    for z in out:
        assert z is None or torch.isfinite(z).all(), "the float64 reference itself is not finite"
    return out


def run(mh, dtype, shape, bits=None, bias=None, hm=None, drop=None, cid=None, post=False, with_align=True, want_d_bias=True, amap=True):
    """qkv_attn(dense_bits=, align_map=) + qkv_attn_long_bwd(dense_bits=, d_align=) on NaN-prefilled outputs ->
    [ctx, dx, None, dw, db, d_bias or None, d_hm, align_map or None]"""
    n, s, t, h, a = shape
    w, b, x, dctx = batch(shape)[3]
    g = batch(shape)[4]
    xd, wd, bd = x.to(dtype).cuda(), w.to(dtype).cuda(), b.cuda()
    bias_d = None if bias is None else bias.cuda()
    hm_d = None if hm is None else hm.cuda()
    cid_d = None if cid is None else cid.cuda()
    am = torch.zeros(n, t, s - t, device="cuda") if amap else None
    ctx, _ = mh.qkv_attn(xd, wd, bd, chunk_id=cid_d, num_heads=a, attn_dropout=drop, attn_bias=bias_d, head_mask=hm_d, dense_bits=bits,
                         align_map=am, align_t=t if amap else 0, side_post_dropout=post, wide_dropout=drop is not None)
    nan = lambda *sh: torch.full(sh, float("nan"), device="cuda")
    dw, db, d_hm = nan(3 * h, h), nan(3 * h), nan(n, a)
    d_bias = nan(n, a, s, s) if want_d_bias and bias is not None else None
    kw = dict(d_align=g.cuda(), align_t=t, side_post_dropout=post) if with_align else {}
    dx = mh.qkv_attn_long_bwd(dctx.to(dtype).cuda(), xd, wd, bd, dw, db, chunk_id=cid_d, num_heads=a, attn_dropout=drop, attn_bias=bias_d,
                              head_mask=hm_d, d_bias=d_bias, d_head_mask=d_hm, dense_bits=bits, wide_dropout=drop is not None, **kw)
    torch.cuda.synchronize()
    return [ctx, dx, None, dw, db, d_bias, d_hm, am]


def check_case(dtype, got, ref, what, shape, d_bias=True):
    n, s, t, h, a = shape
    if not d_bias:
        got, ref = list(got), list(ref)
        got[5] = ref[5] = None
    LB.check_all(dtype, got[:7], ref[:7], what, (n, s, 0, h, a))
    if got[7] is not None:
        check(got[7], ref[7], TOL[dtype], what + " align_map")


def soft(shape):
    """a dense [N, A, S, S] soft bias with single -inf and -10000 entries (key 0 finite)"""
    n, s, t, h, a = shape
    return PF.bias_of("[N,A,S,L]", n, s, 0, a, s)


# ---- 1. / 2. forward and backward values against float64 -----------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("phase", [1, 3])
@pytest.mark.parametrize("shape", SHAPES)
def test_bits_only(mh, dtype, phase, shape):
    """bits alone select the route: ctx and the (un-differentiated) align map at p = 0, the backward without d_align"""
    n, s, t, h, a = shape
    assert mh.qkv_attn_long_align_bwd_route(n, s, 0, h, a, mdt(mh, dtype)) == LB.want_route(dtype)
    hm = LB.head_mask(n, a)
    got = run(mh, dtype, shape, bits=bits_of(mh, shape, phase), hm=hm, with_align=False)
    check_case(dtype, got, reference(shape, phase_add(shape, phase), hm, with_align=False), "bits phase %d S=%d" % (phase, s), shape, d_bias=False)


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("shape", SHAPES)
def test_d_align_only_on_the_bias_route(mh, dtype, shape):
    """no bits: a soft [N, A, S, S] bias with single -inf entries, the align map and its gradient, d_bias"""
    n, s, t, h, a = shape
    hm, bias = LB.head_mask(n, a), soft(shape)
    got = run(mh, dtype, shape, bias=bias, hm=hm)
    check_case(dtype, got, reference(shape, bias, hm), "d_align only S=%d" % s, shape)


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("post", [False, True], ids=["undropped", "post_dropout"])
@pytest.mark.parametrize("shape", SHAPES)
def test_bits_d_align_dropout(mh, dtype, post, shape):
    """phase-3 bits + d_align at p = 0.1 under the wide counter layout: the map and its gradient un-dropped or post-dropout"""
    n, s, t, h, a = shape
    hm = LB.head_mask(n, a)
    got = run(mh, dtype, shape, bits=bits_of(mh, shape, 3), hm=hm, drop=DROP, post=post)
    ref = reference(shape, phase_add(shape, 3), hm, drop=DROP, post=post)
    check_case(dtype, got, ref, "bits + d_align p=0.1 %s S=%d" % ("post" if post else "undropped", s), shape, d_bias=False)


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("shape", SHAPES[:2])
def test_bits_d_align_without_dropout(mh, dtype, shape):
    n, s, t, h, a = shape
    hm = LB.head_mask(n, a)
    got = run(mh, dtype, shape, bits=bits_of(mh, shape, 1), hm=hm)
    check_case(dtype, got, reference(shape, phase_add(shape, 1), hm), "bits + d_align p=0 S=%d" % s, shape, d_bias=False)


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("drop", [None, DROP], ids=["p0", "p0.1"])
def test_bits_d_align_chunk_mean_four_heads(mh, dtype, drop):
    """the seq_enc phase-3 call: bits + chunk-mean queries + align map and gradient at H = 256, A = 4, T = 64, R = 256"""
    shape = CHUNK_SHAPE
    n, s, t, h, a = shape
    cid = batch(shape)[2]
    hm = LB.head_mask(n, a)
    got = run(mh, dtype, shape, bits=bits_of(mh, shape, 3), hm=hm, cid=cid, drop=drop, post=drop is not None)
    ref = reference(shape, phase_add(shape, 3), hm, cid=cid, drop=drop, post=drop is not None)
    check_case(dtype, got, ref, "chunk mean, bits + d_align", shape, d_bias=False)


@pytest.mark.parametrize("dtype", DT)
def test_bits_plus_soft_bias(mh, dtype):
    """bits and a soft bias with single -inf entries add; d_bias is the gradient of the bias"""
    shape = SHAPES[1]
    n, s, t, h, a = shape
    hm, bias = LB.head_mask(n, a), soft(shape)
    got = run(mh, dtype, shape, bits=bits_of(mh, shape, 1), bias=bias, hm=hm, drop=DROP, post=True)
    ref = reference(shape, phase_add(shape, 1) + bias, hm, drop=DROP, post=True)
    check_case(dtype, got, ref, "bits + soft bias", shape)


# ---- 3. a head at 0 ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DT)
def test_a_head_at_zero(mh, dtype):
    shape = SHAPES[1]
    n, s, t, h, a = shape
    hm = torch.tensor([[1.0, 0.0], [0.0, 0.7]])
    bias = torch.zeros(n, a, s, s)
    got = run(mh, dtype, shape, bits=bits_of(mh, shape, 3), bias=bias, hm=hm, drop=DROP, post=True)
    ref = reference(shape, phase_add(shape, 3), hm, drop=DROP, post=True)
    check_case(dtype, got, ref, "head at 0", shape)
    assert torch.isfinite(got[6]).all() and float(got[6][0, 1].abs()) > 0 and float(got[6][1, 0].abs()) > 0      # d_head_mask keeps its value
    for nn_, dead in ((0, 1), (1, 0)):
        assert (got[5][nn_, dead] == 0).all(), "d_bias of the head at 0 is exactly 0"
    # one sequence alone: the dead head's dQ | dK | dV rows are exactly 0, so its 64 columns of every weight gradient are
    im, cm, cid, c, g = batch(shape)
    w, b, x, dctx = c
    bits1 = bits_of(mh, shape, 3)[:1].contiguous()
    xd, wd, bd = x[:1].to(dtype).cuda(), w.to(dtype).cuda(), b.cuda()
    dw1, db1 = torch.full((3 * h, h), float("nan"), device="cuda"), torch.full((3 * h,), float("nan"), device="cuda")
    d_hm1 = torch.full((1, a), float("nan"), device="cuda")
    mh.qkv_attn_long_bwd(dctx[:1].to(dtype).cuda(), xd, wd, bd, dw1, db1, num_heads=a, attn_dropout=DROP, head_mask=hm[:1].cuda(),
                         d_head_mask=d_hm1, dense_bits=bits1, d_align=g[:1].contiguous().cuda(), align_t=t, side_post_dropout=True)
    torch.cuda.synchronize()
    assert (dw1.view(3, a, 64, h)[:, 1] == 0).all() and (db1.view(3, a, 64)[:, 1] == 0).all(), "the head at 0: dQ, dK, dV exactly 0"
    assert (dw1.view(3, a, 64, h)[:, 0] != 0).any() and float(d_hm1[0, 1].abs()) > 0


# ---- 4. fold equivalence ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("drop", [None, DROP], ids=["p0", "p0.1"])
def test_bits_equal_the_folded_bias(mh, dtype, drop, capsys):
    """the bits call and the call with the bits folded into a 0 / -10000 [N,1,S,S] bias: both inside the bounds; bit equality is
    printed (the kernels join 0 / -10000 to the bias before the multiplication by log2e, which is the folded call's arithmetic)"""
    shape = SHAPES[1]
    n, s, t, h, a = shape
    hm = LB.head_mask(n, a)
    add = phase_add(shape, 3)
    ref = reference(shape, add, hm, drop=drop, post=True)
    g_bits = run(mh, dtype, shape, bits=bits_of(mh, shape, 3), hm=hm, drop=drop, post=True)
    g_fold = run(mh, dtype, shape, bias=add, hm=hm, drop=drop, post=True, want_d_bias=False)
    check_case(dtype, g_bits, ref, "bits", shape, d_bias=False)
    check_case(dtype, g_fold, ref, "folded", shape, d_bias=False)
    names = ("ctx", "dx", None, "dw", "db", None, "d_head_mask", "align_map")
    eq = {nm: bool(torch.equal(u, v)) for nm, u, v in zip(names, g_bits, g_fold) if nm}
    with capsys.disabled():
        print("\nfold equivalence %s %s: bit-equal %s" % (str(dtype)[6:], "p=0.1" if drop else "p=0", eq))
    for nm in ("ctx", "dx", "dw", "db", "d_head_mask"):        # (the align map is summed over the heads by float atomics in both calls)
        assert eq[nm], nm


# ---- 5. write coverage, repeatability ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[3]])
def test_outputs_fully_written_and_two_calls_bit_identical(mh, dtype, shape):
    n, s, t, h, a = shape
    hm, bias = LB.head_mask(n, a), torch.zeros(n, 1, s, s)
    r1 = run(mh, dtype, shape, bits=bits_of(mh, shape, 3), bias=bias, hm=hm, drop=DROP, post=True)
    r2 = run(mh, dtype, shape, bits=bits_of(mh, shape, 3), bias=bias, hm=hm, drop=DROP, post=True)
    for nm, u, v in zip(LB.NAMES7, r1[:7], r2[:7]):
        if u is not None:
            assert torch.isfinite(u).all(), nm + ": an element was not written"
            assert torch.equal(u, v), nm


# ---- 6. without bits and d_align the entries are the drop entries -------------------------------------------------------------------------

def raw_fwd(mh, entry, dtype, shape, bias, hm, drop, extra):
    n, s, t, h, a = shape
    w, b, x, _ = batch(shape)[3]
    xd, wd, bd = x.to(dtype).cuda(), w.to(dtype).cuda(), b.cuda()
    ctx = torch.full((n, s, h), float("nan"), dtype=dtype, device="cuda")
    need = mh.lib().modcr_qkv_attn_bias_workspace(n, s, 0, h, mdt(mh, dtype))
    ws = torch.empty(need // 4 + 1, device="cuda")
    P = mh._ptr
    rc = getattr(mh.lib(), entry)(P(xd), None, P(wd), P(bd), P(bias), 0, 0, 0, P(hm), a, None, 0, P(ctx), None, None, 0, n, s, 0, h, a,
                                  float(drop[0]), drop[1], drop[2], 0, P(ws), need, mdt(mh, dtype), mh._stream(), *extra)
    torch.cuda.synchronize()
    return rc, ctx


def raw_bwd(mh, entry, dtype, shape, bias, hm, drop, extra):
    n, s, t, h, a = shape
    w, b, x, dctx = batch(shape)[3]
    xd, wd, bd, dd = x.to(dtype).cuda(), w.to(dtype).cuda(), b.cuda(), dctx.to(dtype).cuda()
    nan = lambda *sh: torch.full(sh, float("nan"), device="cuda")
    dx = torch.full((n, s, h), float("nan"), dtype=dtype, device="cuda")
    dw, db, d_hm = nan(3 * h, h), nan(3 * h), nan(n, a)
    need = mh.lib().modcr_qkv_attn_long_align_bwd_workspace(n, s, 0, h, mdt(mh, dtype))
    assert need == mh.lib().modcr_qkv_attn_long_drop_bwd_workspace(n, s, 0, h, mdt(mh, dtype))
    ws = torch.empty(need // 4 + 1, device="cuda")
    P = mh._ptr
    rc = getattr(mh.lib(), entry)(P(dd), P(xd), None, P(wd), P(bd), P(bias), 0, 0, 0, P(hm), a, None, 0, None, P(dx), None, P(dw), P(db), 0,
                                  None, P(d_hm), n, s, 0, h, a, float(drop[0]), drop[1], drop[2], P(ws), need, mdt(mh, dtype), mh._stream(),
                                  *extra)
    torch.cuda.synchronize()
    return rc, dx, dw, db, d_hm


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("s", [200, 300])
def test_without_bits_and_d_align_it_is_the_drop_entry(mh, dtype, s):
    shape = (2, s, 100, 128, 2)
    n, _, t, h, a = shape
    bias = torch.zeros(1, 1, 1, s, device="cuda")
    hm = LB.head_mask(n, a).cuda()
    f0 = raw_fwd(mh, "modcr_qkv_attn_long_drop_fwd", dtype, shape, bias, hm, DROP, ())
    f1 = raw_fwd(mh, "modcr_qkv_attn_long_align_fwd", dtype, shape, bias, hm, DROP, (None,))
    assert f0[0] == f1[0] == 0 and torch.isfinite(f0[1]).all() and torch.equal(f0[1], f1[1])
    b0 = raw_bwd(mh, "modcr_qkv_attn_long_drop_bwd", dtype, shape, bias, hm, DROP, ())
    b1 = raw_bwd(mh, "modcr_qkv_attn_long_align_bwd", dtype, shape, bias, hm, DROP, (None, None, 0, 0))
    assert b0[0] == b1[0] == 0
    for u, v in zip(b0[1:], b1[1:]):
        assert torch.isfinite(u).all() and torch.equal(u, v)


# ---- 7. refusals, outputs untouched -------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_outputs_untouched(mh):
    dtype = torch.bfloat16
    small, big = (1, 200, 100, 128, 2), (1, 300, 100, 128, 2)
    hm = torch.ones(1, 2, device="cuda")
    bits = lambda s: torch.full((1, s, (s + 31) // 32), -1, dtype=torch.int32, device="cuda")
    g = lambda t, r: torch.zeros(1, t, r, device="cuda")

    def refused(shape, extra_f, extra_b, code, *words):
        if extra_f is not None:
            rc, ctx = raw_fwd(mh, "modcr_qkv_attn_long_align_fwd", dtype, shape, None, hm, (0.0, 0, 0), extra_f)
            msg = mh.lib().modcr_last_error().decode()
            assert rc == code and all(w_ in msg for w_ in words), (rc, msg)
            assert torch.isnan(ctx.float()).all()
        rc, dx, dw, db, d_hm = raw_bwd(mh, "modcr_qkv_attn_long_align_bwd", dtype, shape, None, hm, (0.0, 0, 0), extra_b)
        msg = mh.lib().modcr_last_error().decode()
        assert rc == code and all(w_ in msg for w_ in words), (rc, msg)
        assert all(torch.isnan(z.float()).all() for z in (dx, dw, db, d_hm))

    P = mh._ptr
    b2, b3 = bits(200), bits(300)
    refused(small, (P(b2),), (P(b2), None, 0, 0), -3, "256", "modcr_qkv_attn")
    refused(small, None, (None, P(g(100, 100)), 100, 0), -3, "256", "modcr_qkv_attn_bwd")
    refused(big, None, (None, P(g(100, 200)), 0, 0), -1, "align_t=0")
    refused(big, None, (None, P(g(100, 200)), 300, 0), -1, "align_t=300")
    refused(big, (ctypes.c_void_p(P(b3).value + 2),), (ctypes.c_void_p(P(b3).value + 2), None, 0, 0), -1, "4-byte")
    refused(big, None, (P(b3), None, 0, 2), -1, "flags")
    with pytest.raises(ValueError, match="attn_bias / head_mask replace key_mask / mask_bits"):
        mh.qkv_attn(torch.zeros(1, 300, 128, device="cuda"), torch.zeros(384, 128, device="cuda"), torch.zeros(384, device="cuda"),
                    mask_bits=b3, attn_bias=torch.zeros(1, 1, 1, 300, device="cuda"), num_heads=2)


# ---- 8. layer level -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["bf16", "fp32"])
@pytest.mark.parametrize("combo", ["bits", "d_align", "bits+d_align", "bits+d_align+chunk"])
def test_layer_forward_train_long_align(mh, mode, combo):
    """hip_layers.layer_forward_train(long_align=True) / layer_backward(d_align=) against the oracle layer under float64 autograd;
    with long_align off the same call raises its NotImplementedError, word for word"""
    from modeling import hip_autograd as ag
    from modeling import hip_layers
    dtype, dev = MODE_DT[mode], torch.device("cuda")
    shape = (2, 300, 229, 128, 2)
    n, s, t, h, a = shape
    im, cm, cid, _, g = batch(shape)
    names = list(ag.BertLayerFn.NAMES)
    rs, sdt, sd64, x, dy, _ = LB.layer_case(mode, n, s, 0, 900 + len(combo))
    use_bits, use_align, use_chunk = "bits" in combo, "d_align" in combo, "chunk" in combo
    phase = 3 if use_chunk else 1
    add = phase_add(shape, phase).double() if use_bits else O.extend_mask(im).double()
    gi = None
    if use_chunk:
        gi = [cid[i][cid[i] >= 0].long() for i in range(n)]
    ref_p = {k: sd64[k].clone().requires_grad_(True) for k in names}
    xr = x.double().requires_grad_(True)
    y_ref, probs = O.bert_layer(xr, add, ref_p, "", a, 1e-12, gather_index=gi)
    amap_ref = probs.sum(1)[:, :t, t:]
    loss = (y_ref * dy.double()).sum()
    if use_align:
        loss = loss + (amap_ref * g.double()).sum()
    loss.backward()
    packed = hip_layers.pack_layer({k: sdt[k].to(dev) for k in names}, "", dev, dtype)
    xd, dyd = x.to(dtype).to(dev), dy.to(dtype).to(dev)
    kw = dict(chunk_id=cid.to(dev) if use_chunk else None)
    if use_bits:
        kw["mask_bits"] = bits_of(mh, shape, phase)
    else:
        kw["key_mask"] = im.to(dev)
    amap = torch.zeros(n, t, s - t, device=dev) if use_align else None
    if use_align:
        kw.update(align_map=amap, align_t=t)
    with pytest.raises(NotImplementedError) as e:
        hip_layers.layer_forward_train(packed, xd, a, 1e-12, long_backward=True, **kw)
    assert str(e.value) == "layer_forward_train: no mask_bits and no align map above 256 keys (long_backward)"
    if amap is not None:
        amap.zero_()
    y, saved = hip_layers.layer_forward_train(packed, xd, a, 1e-12, long_backward=True, long_align=True, **kw)
    assert saved["long_align"] and saved["mask_bits"] is None and saved["lse"] is None
    dx, grads = hip_layers.layer_backward(packed, saved, dyd, mfma=mode == "bf16", d_align=g.to(dev) if use_align else None)
    torch.cuda.synchronize()
    what = "long_align layer " + combo
    check(y, y_ref, Y_TOL[mode], what + " y")
    if use_align:
        check(amap, amap_ref, Y_TOL[mode], what + " align map")
    check(dx, xr.grad, G_TOL[mode], what + " dx")
    check_param_grads(mode, grads, {k: v.grad for k, v in ref_p.items()}, what)


# ---- 9. model level: seq_encoder at 270 keys, trained -----------------------------------------------------------------------------------

def seq_model_case(mode, attn_p):
    """a 12-layer H = 128, two-head SeqBertImgModel twin in training mode and a synthetic batch with T = 40 text rows and R = 230 regions"""
    import test_hip_models as M
    from modeling.modeling_vcr_chunkalign_v10 import SeqBertImgModel
    from Data import synthetic
    cfgd = H.cfg_dict(hidden=128, heads=2, layers=12, vocab=3000, max_pos=64, img_dim=70)
    sd_s = H.bert_img_weights(np.random.RandomState(270), cfgd, seq=True)
    sm = M.load(SeqBertImgModel(M.small_config(mode, vocab_size=3000, attention_probs_dropout_prob=attn_p)), sd_s)
    sm.trainable = True
    sm.train()
    b = synthetic.make_batch(1, T=40, R=230, seed=5, vocab_size=3000, img_dim=70, min_text=8, min_regions=4, roberta_len=8)
    return cfgd, sd_s, sm, b


def seq_model_forward(sm, b):
    d = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in b.items()}
    t = b["input_ids"].shape[1]
    so, ch = sm(d["input_ids"], img_feats=d["img_feat"], img_mask=d["input_mask"][:, t:], input_mask=d["input_mask"],
                attention_mask=d["chunk_attention_mask"], token_type_ids=d["token_type_ids"], offsets=None,
                gather_index=[g_.cuda() for g_ in b["gather_index"]])
    return so, ch


@pytest.mark.parametrize("mode", ["bf16", "fp32"])
def test_seq_encoder_trains_at_270_keys(mh, mode):
    """trainable_encoders.seq_encoder (through SeqBertImgModel.forward, trainable) at S = 270 under set_long_backward(True, align=True):
    parameter gradients of a random linear functional of (sequence output, pooled, chunk_hidden, align map) against the oracle's
    autograd; the parameter subset and the bounds of test_hip_models.test_seq_enc_residual_flags_gradients_vs_oracle"""
    import test_hip_models as M
    from modeling import hip_autograd as ag
    cfgd, sd_s, sm, b = seq_model_case(mode, 0.0)
    t, r = 40, 230
    valid = b["input_mask"].float()[..., None]
    ref_sd = {k: torch.from_numpy(v).clone().requires_grad_(v.dtype.kind == "f") for k, v in sd_s.items()}
    (rseq, rpool, atts), rch = O.seq_bert_img_model(ref_sd, "", cfgd, b["input_ids"], b["token_type_ids"], b["chunk_attention_mask"],
                                                    b["input_mask"], b["img_feat"], list(b["gather_index"]))
    ramap = sum(atts[i].sum(1)[:, :t, t:] for i in (9, 10, 11))
    torch.manual_seed(5)
    w_seq, w_pool, w_ch = torch.randn_like(rseq) * 0.1 * valid, torch.randn_like(rpool), torch.randn_like(rch) * 0.1 * valid
    w_am = torch.randn_like(ramap) * valid[:, :t] * valid[:, t:, 0][:, None, :]
    ((rseq * w_seq).sum() + (rpool * w_pool).sum() + (rch * w_ch).sum() + (ramap * w_am).sum()).backward()
    assert all(torch.isfinite(v.grad).all() for v in ref_sd.values() if v.grad is not None), "the reference itself is not finite"
    ag.set_grad_sink(None)
    ag.set_exact(mode == "fp32")
    try:
        ag.set_long_backward(True)
        with pytest.raises(NotImplementedError, match="takes no mask_bits"):
            seq_model_forward(sm, b)
        ag.set_long_backward(True, align=True)
        so, ch = seq_model_forward(sm, b)
        assert so[0].requires_grad and tuple(so.align_map.shape) == (4, t, r)
        M.check(so.align_map, ramap, M.TOL[mode] * M.DEEP[mode], "seq_enc 270 keys align map")      # (the suite's 12-layer bound)
        ((so[0].float() * w_seq.cuda()).sum() + (so[1] * w_pool.cuda()).sum() + (ch.float() * w_ch.cuda()).sum() +
         (so.align_map * w_am.cuda()).sum()).backward()
        torch.cuda.synchronize()
    finally:
        ag.set_long_backward(False)
        ag.set_exact(False)
    got = dict(sm.named_parameters())
    gtol = 2e-3 if mode == "fp32" else 0.1
    for k in ("pooler.dense.weight", "encoder.layer.11.output.dense.weight", "encoder.layer.10.attention.self.value.weight",
              "encoder.layer.9.intermediate.dense.weight", "encoder.layer.8.output.dense.weight", "encoder.layer.5.attention.self.query.weight",
              "encoder.layer.3.attention.output.dense.weight", "encoder.layer.0.attention.self.value.weight", "img_embedding.weight",
              "embeddings.word_embeddings.weight"):
        M.check_grad(got[k].grad, ref_sd[k].grad, gtol, "seq_enc 270 keys grad " + k)


def test_seq_encoder_at_270_keys_with_attention_dropout(mh):
    """attention_probs_dropout_prob = 0.1: refused with `align` off (dropout alone does not lift the mask_bits refusal), finite
    gradients everywhere with set_long_backward(True, dropout=True, align=True)"""
    from modeling import hip_autograd as ag
    cfgd, sd_s, sm, b = seq_model_case("bf16", 0.1)
    ag.set_grad_sink(None)
    try:
        ag.set_long_backward(True, dropout=True)
        with pytest.raises(NotImplementedError, match="takes no mask_bits"):
            seq_model_forward(sm, b)
        ag.set_long_backward(True, dropout=True, align=True)
        mh.DROPOUT.manual_seed(11)
        so, ch = seq_model_forward(sm, b)
        (so[0].float().sum() + so[1].sum() + ch.float().sum() + so.align_map.sum()).backward()
        torch.cuda.synchronize()
    finally:
        ag.set_long_backward(False)
    assert torch.isfinite(so.align_map).all()
    grads = {k: p.grad for k, p in sm.named_parameters() if k.startswith("encoder.layer.")}
    assert grads and all(g is not None and torch.isfinite(g).all() for g in grads.values())
    assert float(grads["encoder.layer.9.attention.self.query.weight"].abs().max()) > 0
