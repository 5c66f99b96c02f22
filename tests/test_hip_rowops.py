"""The row passes of csrc/rowops.hip and the hidden-dropout mask of csrc/common.h, route by route, against float64 and a host mask.

What a case lands on is computed here from its shape by the dispatcher's rule (ln_bwd_route, vec_route) and stated in its id; the
case tables are module-level, and tests/test_host_logic.py asserts without a GPU that they cover every kernel, rows-per-wave class
and dtype route, so a table edited later cannot silently lose one.

Every comparison is against float64 formed from the SAME stored inputs (bf16 / fp16 operands are rounded first).  The bound of a
compared quantity is measured against a plain fp32 evaluation of the same operation (torch on the CPU), not against the kernels:

    |got - ref| <= min(k * max(yardstick, eps32 * scale), ceiling * scale) + half an output ulp at |ref|      (element-wise)

yardstick = max |plain fp32 - float64| of that quantity, scale = max(1, max |ref|), eps32 = 2^-23; the half ulp only for bf16 / fp16
outputs; `ceiling` is what the older tests hold the same quantity to.  k is one constant per quantity family (below).  Mask
comparisons (against helpers.hidden_drop_keep), guard rows and refusals are exact.

Every output sits between two guard rows filled with a sentinel that must come back untouched; a refused call must not write at all."""
import itertools

import numpy as np
import pytest
import torch

import helpers as H

pytestmark = pytest.mark.gpu

# k per quantity family: at most 2x the worst (err - half ulp) / max(yardstick, eps32 * scale) of profiles/rowops_tolerance_report.txt
K_LN_FWD = 2.8      # 1.42: test_layernorm_fwd_routes[bf16_resf32_f32-4], M=4099
K_LN_DX = 3.9       # 1.96: test_layernorm_dropout_bwd_routes[vec1_dyf32_pref32_rpw2_M8197], d_pre against the rows kernel
K_DG_SMALL = 17.0   # 8.51: test_layernorm_bwd_routes[generic_rpw1_M4097_H1028], dgamma (M < 8192)
K_DG_LARGE = 16.7   # 8.36: test_layernorm_bwd_routes[generic_rpw11_M46080_H1028], dgamma (M >= 8192: up to 4400 block sums added in scheduling order)
K_MC_CE = 1.5       # 0.752: test_mc_ce_soft_labels[37-4], loss
K_ACT_BWD = 1.6     # 0.816: test_act_bwd_on_a_grid[gelu]
# ceilings: the bounds of tests/test_hip_kernels.py for the same quantities, as a multiple of scale
CEIL_LN_F32, CEIL_LN_BF16, CEIL_LN_BWD, CEIL_MC_CE, CEIL_ACT_BWD = 1e-5, 1e-2, 1e-4, 1e-5, 1e-5

EPS32 = 2.0 ** -23
SENTINEL = 1234.5   # exact in bf16, fp16 and fp32
LN_EPS = 1e-12
TD = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
MANT = {torch.float32: 23, torch.bfloat16: 7, torch.float16: 10}

# ---- case tables (read by tests/test_host_logic.py::test_rowops_case_tables_cover_every_route) -------------------------------
LN_FWD_H = (4, 128, 132, 260, 768, 1020, 1024)
LN_FWD_M = (1, 5, 37, 4099)
# (x, residual, out): the 8 combinations of the dispatcher's switch + the two fp16 -> bf16 forms
LN_FWD_ROUTES = [(i, r, o) for i in ("bf16", "f32") for r in ("bf16", "f32") for o in ("bf16", "f32")] + [("f16", None, "bf16"), ("f16", "bf16", "bf16")]

FUSED_H = (256, 772, 1024)
FUSED_M = (3, 300)
FUSED_ROUTES = [("f32", r, o) for r in (None, "bf16", "f32") for o in ("bf16", "f32")] + [("f16", None, "bf16"), ("f16", "bf16", "bf16")]

LN_BWD_H = {"rows4": (64, 200, 256), "rows12": (260, 512, 768), "rows16": (772, 1024), "generic": (1028, 2052)}
LN_BWD_SMALL_M = (1, 3, 150, 4097)              # rpw 1; 1, 3 and 4097 leave trailing waves of a block without a row
LN_BWD_LARGE_M = (8197, 27136, 46080, 70001)    # rpw 2 (ragged), 6 (27136 % 24 != 0), 11, 16 (capped, ragged)


def rows_per_wave(m):
    """modcr_layernorm_bwd / modcr_layernorm_dropout_bwd: rpw = clamp(M / 4096, 1, 16)"""
    return min(max(m // 4096, 1), 16)


def rpw_class(rpw):
    return "1" if rpw == 1 else ("16" if rpw == 16 else "2-15")


def ln_bwd_route(m, h):
    """(kernel, rows per wave) of modcr_layernorm_bwd.  The generic kernel (H > 1024) has no row loop (one wave per row, M / 4
    blocks): its rpw is only the M class of the case."""
    kernel = "rows4" if h <= 256 else "rows12" if h <= 768 else "rows16" if h <= 1024 else "generic"
    return kernel, rows_per_wave(m)


LN_BWD_CASES = [(m, h) for m in LN_BWD_SMALL_M for hs in LN_BWD_H.values() for h in hs] + \
               [(m, hs[0]) for m in LN_BWD_LARGE_M for hs in LN_BWD_H.values()]


def ln_bwd_id(c):
    return "%s_rpw%d_M%d_H%d" % (ln_bwd_route(*c) + c)


VEC_H = (256, 512, 768, 1024)
VEC_DT = [(dy, pre) for dy in ("f32", "bf16") for pre in ("f32", "f16")]
# small M: every instantiation; large M (rpw 2 ragged, rpw 11): every NV, the dtype pairs in rotation
VEC_CASES = [(m, h, dy, pre) for m in (5, 300) for h in VEC_H for dy, pre in VEC_DT] + \
            [(m, h) + VEC_DT[(i + j) % 4] for j, m in enumerate((8197, 46080)) for i, h in enumerate(VEC_H)]


def vec_route(m, h, dy, pre):
    """(NV, dY type, pre type, rows per wave) of layernorm_bwd_vec_kernel"""
    return h // 256, dy, pre, rows_per_wave(m)


def vec_id(c):
    return "vec%d_dy%s_pre%s_rpw%d_M%d" % (vec_route(*c) + (c[0],))


# ---- plumbing -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mh():
    import __graft_entry__ as g
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import modcr_hip
    modcr_hip.lib()         # must already be built in-tree; fails loudly otherwise
    return modcr_hip


def rand(shape, seed, dtype=torch.float32, mul=1.0, add=0.0):
    """deterministic normal values on the device, stored as `dtype`"""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return (torch.randn(shape, generator=g, device="cuda") * mul + add).to(dtype)


class Guard(object):
    """an output [rows, cols] between two guard rows of the sentinel"""

    def __init__(self, rows, cols, dtype, fill=None):
        self.buf = torch.full((rows + 2, cols), SENTINEL, dtype=dtype, device="cuda")
        self.v = self.buf[1:rows + 1]
        if fill is not None:
            self.v.copy_(fill)

    def intact(self):
        torch.cuda.synchronize()
        return bool((self.buf[0] == SENTINEL).all()) and bool((self.buf[-1] == SENTINEL).all())

    def untouched(self):
        torch.cuda.synchronize()
        return bool((self.buf == SENTINEL).all())


def ulp(ref, dtype):
    """spacing of `dtype` at |ref| (float64 tensor; the normal range is all these tests produce, 2^-24 floors the fp16 one)"""
    _, e = torch.frexp(ref.abs().clamp_min(2.0 ** -60))
    u = ((e.to(torch.int64) - 1 - MANT[dtype] + 1023) << 52).view(torch.float64)        # 2^(e - 1 - mantissa bits), built from its bits: exact
    return u.clamp_min(2.0 ** -24) if dtype == torch.float16 else u


FAMILY_K = {"ln fwd": lambda: K_LN_FWD, "ln dX": lambda: K_LN_DX, "dgamma/dbeta M<8192": lambda: K_DG_SMALL,
            "dgamma/dbeta M>=8192": lambda: K_DG_LARGE, "mc_ce": lambda: K_MC_CE, "act_bwd": lambda: K_ACT_BWD}


class Worst(object):
    """worst use of k and of the ceiling per quantity family over the checks of one test: one report line each (helpers.report_use)"""

    def __init__(self):
        self.k, self.ceil = {}, {}

    def add(self, fam, what, used, k, ceil_used, ceil):
        if fam not in self.k or used > self.k[fam][1]:
            self.k[fam] = (what, used, k)
        ckey = "%s <= %.0e" % (fam, ceil)
        if ckey not in self.ceil or ceil_used > self.ceil[ckey][1]:
            self.ceil[ckey] = (what, ceil_used, ceil)

    def flush(self):
        for fam, (what, used, k) in sorted(self.k.items()):
            H.report_use("%s: %s" % (fam, what), used, k, kind="(|err|-ulp/2)/yardstick")
        for fam, (what, used, ceil) in sorted(self.ceil.items()):
            H.report_use("%s: %s" % (fam, what), used, ceil, kind="(|err|-ulp/2)/scale    ")


@pytest.fixture
def tol():
    w = Worst()
    yield w
    w.flush()


def check(tol, fam, what, got, ref, plain, ceil, truth=None):
    """the bound of the module docstring; got: device tensor of the output dtype, ref: float64, plain: the fp32 evaluation of
    `truth` (default: of ref -- `truth` is the float64 result when ref is another kernel's output)"""
    ref = ref.cuda()
    k = FAMILY_K[fam]()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), what + ": non-finite output"
    err = (got.double() - ref).abs()
    scale = max(1.0, ref.abs().max().item())
    yard = (plain.cuda().double() - (ref if truth is None else truth.cuda())).abs().max().item()
    base = max(yard, EPS32 * scale)
    hu = 0.5 * ulp(ref, got.dtype) if got.dtype != torch.float32 else torch.zeros_like(ref)
    over = (err - hu).clamp_min(0).max().item()
    tol.add(fam, what, over / base, k, over / scale, ceil)
    bad = err > min(k * base, ceil * scale) + hu
    assert not bool(bad.any()), "%s %s: %d elements over the bound, worst |err| %.4g (yardstick %.3g, scale %.3g, k %.3g)" % (
        fam, what, int(bad.sum()), err.max().item(), yard, scale, k)


def host_keep(seed, off, shape, p):
    """hidden_drop_keep over the flat indices of a contiguous tensor of `shape`, on the device"""
    n = int(np.prod(shape))
    return torch.from_numpy(H.hidden_drop_keep(seed, off, n, p).reshape(shape)).cuda()


def scale32(p):
    """1.0f / (1.0f - p) as the entries form it on the host"""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


def ln64(v, g, b):
    return torch.nn.functional.layer_norm(v, (v.shape[-1],), g.double(), b.double(), LN_EPS)


def ln32_cpu(v, g, b):
    return torch.nn.functional.layer_norm(v.cpu(), (v.shape[-1],), g.cpu(), b.cpu(), LN_EPS)


def gamma_beta(h, seed):
    return rand((h,), seed, mul=0.1, add=1.0), rand((h,), seed + 1, mul=0.1)


def dt_code(mh, name):
    return 0 if name is None else mh.dt_of(torch.empty(0, dtype=TD[name]))


SEEDS = (1234, 2 ** 63 + 5)                     # zero and non-zero high word
OFFSETS = (0, 77, 2 ** 33, 2 ** 34 - 6)         # aligned, unaligned, high group word, groups crossing 2^32 inside the call


# ---- mask identity (exact) --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 7, 4099, 5000003])          # 5,000,003 > 16384 * 256: more than one grid-stride pass
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_dropout_mask_is_the_host_restatement(mh, dtype, n):
    td = TD[dtype]
    ones = torch.ones(n, dtype=td, device="cuda")
    x = rand((n,), n, td, add=3.0)
    combos = list(itertools.product(SEEDS, OFFSETS, (0.1, 0.3)))
    if n > 10000:
        combos = [(1234, 77, 0.3), (2 ** 63 + 5, 2 ** 34 - 6, 0.1), (4242, 2 ** 33, 0.1)]
    for seed, off, p in combos:
        keep = host_keep(seed, off, (n,), p)
        g = Guard(1, n, td)
        mh.dropout(ones, p, seed, off, out=g.v[0])
        assert g.intact()
        assert torch.equal(g.v[0] != 0, keep), (seed, off, p)
        y = mh.dropout(x, p, seed, off)
        assert torch.equal(y != 0, keep), (seed, off, p)
        # kept values: x / (1 - p) (p as the fp32 number the entry receives) within 1 ulp of fp32; bf16: rounded once more
        # (x times the fp32 reciprocal: <= 1.4 ulp from the quotient, so at most one fp32 step from its rounding)
        want = (x.double() / (1.0 - float(np.float32(p))) * keep).float().double()
        err = (y.double() - want).abs()
        bound = ulp(want, torch.float32) + (0.5 * ulp(want, td) if td != torch.float32 else 0.0)
        assert bool((err <= bound).all()), (seed, off, p, err.max().item())
    for seed, off in ((1234, 77), (2 ** 63 + 5, 2 ** 33)):      # p = 0: everything kept, bit for bit
        g = Guard(1, n, td)
        mh.dropout(x, 0.0, seed, off, out=g.v[0])
        assert g.intact() and torch.equal(g.v[0], x)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_rows_scatter_dropout_takes_its_counters_from_the_destination(mh, dtype):
    td = TD[dtype]
    n, s, r, row0, h = 3, 9, 4, 5, 132
    src = torch.ones(n * r, h, dtype=td, device="cuda")
    for seed, off, p in ((1234, 77, 0.3), (2 ** 63 + 5, 2 ** 33, 0.1), (1234, 2 ** 34 - 6, 0.3), (7, 4000, 0.0)):
        g = Guard(n * s, h, td)
        dst = g.v.view(n, s, h)
        mh.rows_scatter_dropout(src, dst, row0, (p, seed, off))
        keep = host_keep(seed, off, (n, s, h), p)[:, row0:row0 + r]
        assert g.intact()
        assert torch.equal(dst[:, row0:row0 + r] != 0, keep), (seed, off, p)
        assert bool((dst[:, :row0] == SENTINEL).all()) and bool((dst[:, row0 + r:] == SENTINEL).all())
        kept = dst[:, row0:row0 + r][keep].double()
        assert bool(((kept - scale32(p)).abs() <= ulp(kept, td)).all())


# ---- modcr_layernorm_fwd -----------------------------------------------------------------------------------------------------
def run_ln_fwd(mh, x, res, g, b, out, m, h, rpg=0, gstride=0):
    return mh.lib().modcr_layernorm_fwd(mh._ptr(x), mh.dt_of(x), mh._ptr(res), mh.dt_of(res) if res is not None else 0, mh._ptr(g), mh._ptr(b),
                                        LN_EPS, mh._ptr(out), mh.dt_of(out), m, h, rpg, gstride, mh._stream())


@pytest.mark.parametrize("h", LN_FWD_H)
@pytest.mark.parametrize("route", LN_FWD_ROUTES, ids=lambda r: "%s_res%s_%s" % r)
def test_layernorm_fwd_routes(mh, tol, route, h):
    ti, tr, to = route
    g, b = gamma_beta(h, h)
    for m in LN_FWD_M:
        x = rand((m, h), m * 7 + h, TD[ti], mul=3.0, add=1.0)
        r = rand((m, h), m * 11 + h, TD[tr]) if tr else None
        forms = [r] + ([None] if (r is not None and tr == ti) else [])      # no residual: the kernel of (x, x's type, out)
        for res in forms:
            v = x.double() + (res.double() if res is not None else 0.0)
            v32 = x.float() + res.float() if res is not None else x.float()
            out = Guard(m, h, TD[to])
            assert run_ln_fwd(mh, x, res, g, b, out.v, m, h) == 0, mh.lib().modcr_last_error()
            assert out.intact()
            check(tol, "ln fwd", "M=%d%s" % (m, "" if res is not None else " no residual"), out.v, ln64(v, g, b), ln32_cpu(v32, g, b),
                  CEIL_LN_F32 if to == "f32" else CEIL_LN_BF16)


@pytest.mark.parametrize("to", ["f32", "bf16"])
def test_layernorm_fwd_grouped_rows_and_refusals(mh, tol, to):
    h, groups, rpg, gstride, row0 = 260, 8, 3, 8, 5
    m = groups * rpg
    g, b = gamma_beta(h, 3)
    x = rand((m, h), 21, mul=3.0, add=1.0)
    out = Guard(groups * gstride, h, TD[to])
    assert run_ln_fwd(mh, x, None, g, b, out.v[row0:], m, h, rpg, gstride) == 0        # rows of group i behind 5 rows of an 8-row sequence
    assert out.intact()
    seq = out.v.view(groups, gstride, h)
    assert bool((seq[:, :row0] == SENTINEL).all())
    check(tol, "ln fwd", "grouped rows", seq[:, row0:].reshape(m, h), ln64(x.double(), g, b), ln32_cpu(x, g, b),
          CEIL_LN_F32 if to == "f32" else CEIL_LN_BF16)
    for bad_h in (1028, 130):                                                        # > 1024; not a multiple of 4
        xb = rand((5, bad_h), 1)
        gb, bb = gamma_beta(bad_h, 2)
        o = Guard(5, bad_h, TD[to])
        assert run_ln_fwd(mh, xb, None, gb, bb, o.v, 5, bad_h) != 0
        assert b"layernorm_fwd" in mh.lib().modcr_last_error()
        assert o.untouched()


# ---- modcr_dropout_residual_ln_fwd ---------------------------------------------------------------------------------------------
def run_fused(mh, x, res, g, b, out, pre, m, h, p, seed, off):
    return mh.lib().modcr_dropout_residual_ln_fwd(mh._ptr(x), mh.dt_of(x), mh._ptr(res), mh.dt_of(res) if res is not None else 0, mh._ptr(g),
                                                  mh._ptr(b), LN_EPS, mh._ptr(out), mh.dt_of(out), mh._ptr(pre),
                                                  mh.dt_of(pre) if pre is not None else mh.F32, m, h, float(p), seed, off, mh._stream())


@pytest.mark.parametrize("h", FUSED_H)
@pytest.mark.parametrize("route", FUSED_ROUTES, ids=lambda r: "%s_res%s_%s" % r)
def test_dropout_residual_ln_fwd_routes(mh, tol, route, h):
    """x and the residual agree in sign element by element (the row as a whole has both signs): the sum dropout(x) + residual then
    never cancels, and two fp32 roundings (product, sum) stay within 1 ulp of the rounded float64 sum -- the bound asked of pre_out."""
    tx, tr, to = route
    g, b = gamma_beta(h, h + 5)
    ones, zeros = torch.ones(h, device="cuda"), torch.zeros(h, device="cuda")
    for (m, seed, off), p, tp in itertools.product(((3, 1234, 77), (300, 2 ** 63 + 5, 2 ** 33 + 4)), (0.0, 0.3), (None, "f32", "f16")):
        sgn = torch.sign(rand((m, h), m + h, add=0.1))
        x = (sgn * (0.5 + rand((m, h), m * 3 + h).abs())).to(TD[tx])
        res = (sgn * rand((m, h), m * 5 + h).abs()).to(TD[tr]) if tr else None
        keep = host_keep(seed, off, (m, h), p)
        sc = scale32(p)
        r64 = res.double() if res is not None else torch.zeros(m, h, dtype=torch.float64, device="cuda")
        pre64 = x.double() * keep * sc + r64
        pre32 = x.float() * keep * sc + r64.float()
        what = "M=%d p=%g pre_out=%s" % (m, p, tp)
        for gg, bb in ((g, b), (ones, zeros)):
            out = Guard(m, h, TD[to])
            pre = Guard(m, h, TD[tp]) if tp else None
            assert run_fused(mh, x, res, gg, bb, out.v, pre.v if pre else None, m, h, p, seed, off) == 0, mh.lib().modcr_last_error()
            assert out.intact() and (pre is None or pre.intact())
            check(tol, "ln fwd", what, out.v, ln64(pre64, gg, bb), ln32_cpu(pre32, gg, bb), CEIL_LN_F32 if to == "f32" else CEIL_LN_BF16)
            if tp is None:
                break                       # gamma = 1, beta = 0 only matters with the pre-LayerNorm rows beside it
            got = pre.v.double()
            if tp == "f32":
                want = pre64.float().double()
                assert bool(((got - want).abs() <= ulp(want, torch.float32)).all()), what
                assert torch.equal((pre.v - r64.float()) == 0, ~keep), what         # dropped: 0 + residual, exactly
            else:
                assert bool(((got - pre64).abs() <= 0.5 * ulp(pre64, torch.float16) + ulp(pre64, torch.float32)).all()), what
                if res is None:
                    assert torch.equal(pre.v == 0, ~keep), what


def test_dropout_residual_ln_wrapper_passes_pre_out(mh):
    m, h = 37, 772
    g, b = gamma_beta(h, 1)
    x, res = rand((m, h), 2), rand((m, h), 3, torch.bfloat16)
    for tp in (torch.float32, torch.float16):
        pre_w = torch.empty(m, h, dtype=tp, device="cuda")
        out_w = mh.dropout_residual_ln(x, res, g, b, LN_EPS, 0.3, 99, 1001, mh.F32, pre_out=pre_w)
        out, pre = Guard(m, h, torch.float32), Guard(m, h, tp)
        assert run_fused(mh, x, res, g, b, out.v, pre.v, m, h, 0.3, 99, 1001) == 0
        assert torch.equal(out_w, out.v) and torch.equal(pre_w, pre.v)
    with pytest.raises(ValueError):
        mh.dropout_residual_ln(x, res, g, b, LN_EPS, 0.3, 99, 1001, mh.F32, pre_out=torch.empty(m, h, dtype=torch.bfloat16, device="cuda"))


# ---- modcr_layernorm_bwd -------------------------------------------------------------------------------------------------------
def ln_bwd_refs(v, gamma, dy):
    """(dX, dgamma, dbeta) by autograd of layer_norm(v) . dY, in the dtype and on the device of `v`"""
    v = v.detach().requires_grad_(True)
    g = gamma.detach().to(v.dtype).to(v.device).requires_grad_(True)
    b = torch.zeros_like(g).requires_grad_(True)
    (torch.nn.functional.layer_norm(v, (v.shape[-1],), g, b, LN_EPS) * dy.to(v.dtype).to(v.device)).sum().backward()
    return v.grad, g.grad, b.grad


def fill_pattern(h):
    return 0.25 * (torch.arange(h, device="cuda") % 5).float() - 0.5


def grad_acc(mode, h):
    """dgamma / dbeta accumulators: None (NULL), zeroed or pre-filled (the contract: accumulated into)"""
    if mode == "null":
        return None
    return Guard(1, h, torch.float32, fill=(fill_pattern(h) if mode == "fill" else torch.zeros(h, device="cuda")))


@pytest.mark.parametrize("case", LN_BWD_CASES, ids=ln_bwd_id)
def test_layernorm_bwd_routes(mh, tol, case):
    m, h = case
    kernel = ln_bwd_route(m, h)[0]
    gamma = gamma_beta(h, h)[0]
    pre, res, dy = rand((m, h), m + h, mul=2.0, add=0.5), rand((m, h), m + h + 1), rand((m, h), m + h + 2)
    if m in LN_BWD_SMALL_M:
        combos = list(itertools.product((True, False), ("null", "zero", "fill")))
    else:       # one residual form per large case (both over the table), NULL accumulators on the rpw-2 cases
        with_res = (LN_BWD_LARGE_M.index(m) + list(LN_BWD_H).index(kernel)) % 2 == 0
        combos = [(with_res, "fill"), (with_res, "null" if m == 8197 else "zero")]
    fam_dg = "dgamma/dbeta M<8192" if m < 8192 else "dgamma/dbeta M>=8192"
    refs = {}
    for with_res, mode in combos:
        if with_res not in refs:
            v64 = pre.double() + res.double() if with_res else pre.double()
            v32 = pre.cpu() + res.cpu() if with_res else pre.cpu()
            refs[with_res] = (ln_bwd_refs(v64, gamma, dy), ln_bwd_refs(v32, gamma.cpu(), dy.cpu()))
        (dx64, dg64, db64), (dx32, dg32, db32) = refs[with_res]
        dx, dg, db = Guard(m, h, torch.float32), grad_acc(mode, h), grad_acc(mode, h)
        rc = mh.lib().modcr_layernorm_bwd(mh._ptr(dy), mh._ptr(pre), mh._ptr(res if with_res else None), mh._ptr(gamma), LN_EPS, mh._ptr(dx.v),
                                          mh._ptr(dg.v[0]) if dg else None, mh._ptr(db.v[0]) if db else None, m, h, mh._stream())
        assert rc == 0, mh.lib().modcr_last_error()
        assert dx.intact() and (dg is None or (dg.intact() and db.intact()))
        what = "%s%s" % ("+res " if with_res else "", mode)
        check(tol, "ln dX", what, dx.v, dx64, dx32, CEIL_LN_BWD)
        if dg:
            start = fill_pattern(h) if mode == "fill" else torch.zeros(h, device="cuda")
            check(tol, fam_dg, what + " dgamma", dg.v[0], start.double() + dg64, start.cpu() + dg32, CEIL_LN_BWD)
            check(tol, fam_dg, what + " dbeta", db.v[0], start.double() + db64, start.cpu() + db32, CEIL_LN_BWD)


# ---- modcr_layernorm_dropout_bwd -----------------------------------------------------------------------------------------------
def run_vec(mh, dy, pre, gamma, d_pre, d_sub, dg, db, m, h, p, seed, off):
    return mh.lib().modcr_layernorm_dropout_bwd(mh._ptr(dy), mh.dt_of(dy), mh._ptr(pre), mh.dt_of(pre), mh._ptr(gamma), LN_EPS, mh._ptr(d_pre),
                                                mh._ptr(d_sub), mh._ptr(dg), mh._ptr(db), m, h, float(p), seed, off, mh._stream())


def sample_rows(m):
    """row blocks whose host mask is formed: every row at small M; 16 blocks of 8 rows (first and last included) beyond that"""
    if m <= 512:
        return [(0, m)]
    return [(int(r0), 8) for r0 in np.linspace(0, m - 8, 16).astype(np.int64)]


@pytest.mark.parametrize("case", VEC_CASES, ids=vec_id)
def test_layernorm_dropout_bwd_routes(mh, tol, case):
    m, h, tdy, tpre = case
    gamma = gamma_beta(h, h + 9)[0]
    pre, dy = rand((m, h), m + h, TD[tpre], mul=2.0, add=0.5), rand((m, h), m + h + 2, TD[tdy])
    (dx64, dg64, db64), (dx32, dg32, db32) = ln_bwd_refs(pre.double(), gamma, dy.double()), ln_bwd_refs(pre.float().cpu(), gamma.cpu(), dy.float().cpu())
    fam_dg = "dgamma/dbeta M<8192" if m < 8192 else "dgamma/dbeta M>=8192"
    # the other backward family on the fp32-converted operands: same H, same M, same bound
    dg_r, db_r = torch.zeros(h, device="cuda"), torch.zeros(h, device="cuda")
    dx_rows = mh.layernorm_bwd(dy.float(), pre.float(), gamma, LN_EPS, dg_r, db_r)
    small = m <= 512
    settings = list(itertools.product((0.0, 0.1), (4 * 1000, 2 ** 33 + 1))) if small else [(0.1, 2 ** 33 + 4), (0.1, 4001)]
    for p, off in settings:
        seed = SEEDS[off & 1]
        sc = scale32(p)
        both_sub = None
        for want_pre, want_sub in ((True, True), (True, False), (False, True)):
            d_pre = Guard(m, h, torch.float32) if want_pre else None
            d_sub = Guard(m, h, torch.bfloat16) if want_sub else None
            dg, db = Guard(1, h, torch.float32, fill=fill_pattern(h)), Guard(1, h, torch.float32, fill=torch.zeros(h, device="cuda"))
            rc = run_vec(mh, dy, pre, gamma, d_pre.v if d_pre else None, d_sub.v if d_sub else None, dg.v[0], db.v[0], m, h, p, seed, off)
            assert rc == 0, mh.lib().modcr_last_error()
            assert all(t is None or t.intact() for t in (d_pre, d_sub, dg, db))
            tag = "p=%g off%%4=%d %s%s" % (p, off % 4, "d_pre" if want_pre else "", "+d_sub" if want_sub else "")
            check(tol, fam_dg, tag + " dgamma", dg.v[0], fill_pattern(h).double() + dg64, fill_pattern(h).cpu() + dg32, CEIL_LN_BWD)
            check(tol, fam_dg, tag + " dbeta", db.v[0], db64, db32, CEIL_LN_BWD)
            if want_pre:
                check(tol, "ln dX", tag, d_pre.v, dx64, dx32, CEIL_LN_BWD)
                check(tol, "ln dX", tag + " vs rows kernel", d_pre.v, dx_rows.double(), dx32, CEIL_LN_BWD, truth=dx64)
            if want_pre and want_sub:
                both_sub = d_sub.v.clone()
                v = d_pre.v.double() * sc                   # elsewhere: bf16(d_pre / (1 - p)) within half a bf16 ulp (+ the product's fp32 rounding)
                for r0, nr in sample_rows(m):
                    keep = host_keep(seed, off + r0 * h, (nr, h), p)
                    blk, vb = d_sub.v[r0:r0 + nr], v[r0:r0 + nr]
                    assert torch.equal(blk != 0, keep & (vb.abs() > 1e-30)), tag + ": mask, rows %d.." % r0
                    err = (blk.double() - vb * keep).abs()
                    assert bool((err <= 0.5 * ulp(vb, torch.bfloat16) + 0.5 * ulp(vb, torch.float32)).all()), tag + ": kept values, rows %d.." % r0
                if p == 0.0:
                    assert torch.equal(d_sub.v, d_pre.v.to(torch.bfloat16)), tag + ": p = 0 is a plain bf16 copy"
                elif not small:
                    frac = (d_sub.v != 0).float().mean().item()
                    assert abs(frac - (1 - p)) < 4e-3, (tag, frac)
            elif want_sub:
                assert torch.equal(d_sub.v, both_sub), tag + ": d_sub alone differs from d_sub beside d_pre"


def test_layernorm_dropout_bwd_refusals_and_wrapper(mh):
    m = 6
    for h, p, tpre, why in ((384, 0.1, "f32", b"H=384"), (256, 1.0, "f32", b"p=1"), (256, 0.1, "bf16", b"pre-LayerNorm rows")):
        gamma = gamma_beta(h, 1)[0]
        pre, dy = rand((m, h), 2, TD[tpre]), rand((m, h), 3)
        d_pre, d_sub = Guard(m, h, torch.float32), Guard(m, h, torch.bfloat16)
        dg, db = Guard(1, h, torch.float32), Guard(1, h, torch.float32)
        assert run_vec(mh, dy, pre, gamma, d_pre.v, d_sub.v, dg.v[0], db.v[0], m, h, p, 5, 8) != 0
        assert why in mh.lib().modcr_last_error(), mh.lib().modcr_last_error()
        assert all(t.untouched() for t in (d_pre, d_sub, dg, db))
        with pytest.raises(mh.ModcrHipError):
            mh.layernorm_dropout_bwd(dy, pre, gamma, LN_EPS, None, None, dropout=(p, 5, 8))
    h, m = 512, 37
    gamma = gamma_beta(h, 1)[0]
    pre, dy = rand((m, h), 2, torch.float16), rand((m, h), 3, torch.bfloat16)
    d_pre, d_sub, dg, db = Guard(m, h, torch.float32), Guard(m, h, torch.bfloat16), torch.zeros(h, device="cuda"), torch.zeros(h, device="cuda")
    assert run_vec(mh, dy, pre, gamma, d_pre.v, d_sub.v, dg, db, m, h, 0.1, 5, 8) == 0
    dg_w, db_w = torch.zeros(h, device="cuda"), torch.zeros(h, device="cuda")
    a, b = mh.layernorm_dropout_bwd(dy, pre, gamma, LN_EPS, dg_w, db_w, dropout=(0.1, 5, 8))
    assert a.dtype == torch.float32 and b.dtype == torch.bfloat16
    assert torch.equal(a, d_pre.v) and torch.equal(b, d_sub.v)
    assert torch.allclose(dg_w, dg, rtol=1e-5, atol=1e-5) and torch.allclose(db_w, db, rtol=1e-5, atol=1e-5)      # (atomics: the order of the block sums is free)
    a, b = mh.layernorm_dropout_bwd(dy, pre, gamma, LN_EPS, None, None, want_d_sub=False)
    assert b is None and torch.equal(a, d_pre.v)
    a, b = mh.layernorm_dropout_bwd(dy, pre, gamma, LN_EPS, None, None, want_d_pre=False)
    assert a is None and torch.equal(b, d_pre.v.to(torch.bfloat16))


# ---- small entries ---------------------------------------------------------------------------------------------------------
def mc_ce_refs(z, y, gs):
    """loss = mean_b(-sum_c label * log_softmax(logits)), dlogits = gs * (softmax * sum_c(label) - label) / B (include/modcr_hip.h)"""
    ls = torch.log_softmax(z, dim=1)
    return -(y * ls).sum(1).mean(), (torch.exp(ls) * y.sum(1, keepdim=True) - y) * (gs / z.shape[0])


@pytest.mark.parametrize("b,c", [(1, 4), (37, 4), (256, 4), (257, 4), (1000, 4), (37, 7)])      # > 256 examples: the b += 256 loop iterates
def test_mc_ce_soft_labels(mh, tol, b, c):
    z = rand((b, c), b + c, mul=3.0)
    y = rand((b, c), b + c + 1).abs() + 0.05
    sums = torch.tensor([0.5, 1.0, 2.0], device="cuda")[torch.arange(b, device="cuda") % 3]
    y = (y / y.sum(1, keepdim=True) * sums[:, None]).contiguous()
    gs = torch.tensor([0.25], device="cuda")
    for want_loss, want_grad, scale in ((True, False, None), (False, True, None), (True, True, gs)):
        loss, dl = (Guard(1, 1, torch.float32) if want_loss else None), (Guard(b, c, torch.float32) if want_grad else None)
        rc = mh.lib().modcr_mc_ce_fwd_bwd(mh._ptr(z), mh._ptr(y), mh._ptr(loss.v) if loss else None, mh._ptr(dl.v) if dl else None,
                                          mh._ptr(scale), b, c, mh._stream())
        assert rc == 0, mh.lib().modcr_last_error()
        assert all(t is None or t.intact() for t in (loss, dl))
        s = 0.25 if scale is not None else 1.0
        l64, d64 = mc_ce_refs(z.double(), y.double(), s)
        l32, d32 = mc_ce_refs(z.cpu(), y.cpu(), s)
        what = "grad_scale " if scale is not None else ""
        if loss:
            check(tol, "mc_ce", what + "loss", loss.v.view(()), l64, l32, CEIL_MC_CE)
        if dl:
            check(tol, "mc_ce", what + "dlogits", dl.v, d64, d32, CEIL_MC_CE)


@pytest.mark.parametrize("n", [1, 1000, 3000001])               # 3,000,001 > 8192 * 256: more than one grid-stride pass
@pytest.mark.parametrize("tb,to", [("f32", "f32"), ("f32", "bf16"), ("bf16", "f32"), ("bf16", "bf16")])
def test_add_is_the_rounded_fp32_sum(mh, tb, to, n):
    a, b = rand((n,), n, mul=3.0), rand((n,), n + 1, TD[tb], mul=3.0)
    out = Guard(1, n, TD[to])
    rc = mh.lib().modcr_add(mh._ptr(a), mh._ptr(b), mh.dt_of(b), mh._ptr(out.v), mh.dt_of(out.v), n, mh._stream())
    assert rc == 0, mh.lib().modcr_last_error()
    assert out.intact()
    want = a + b.float()                            # IEEE: the exactly rounded fp32 sum (a bf16 number is an fp32 number)
    assert torch.equal(out.v[0], want.to(TD[to]))
    assert torch.equal(mh.add(a, b, mh.dt_of(out.v)), out.v[0])


@pytest.mark.parametrize("to", ["f32", "bf16"])
@pytest.mark.parametrize("h", [128, 260, 1024])
def test_embed_ln_explicit_positions(mh, tol, h, to):
    """explicit position_ids (out of order, with repeats, all in range), token_type_ids = NULL (type row 0), seq_stride > T"""
    n, t, stride, vocab, max_pos = 3, 10, 14, 50, 16
    rs = np.random.RandomState(h)
    ids = torch.from_numpy(rs.randint(0, vocab, size=(n, t))).cuda()
    pos_ids = torch.from_numpy(np.stack([rs.permutation(max_pos)[:t] for _ in range(n)])).cuda()
    pos_ids[:, 3] = pos_ids[:, 7]                   # a repeat in every sequence
    pos_ids[0, 0] = max_pos - 1
    word, pos, typ = rand((vocab, h), 1, mul=0.5), rand((max_pos, h), 2, mul=0.5), rand((2, h), 3, mul=0.5)
    g, b = gamma_beta(h, 4)
    v64 = (word.double()[ids] + typ.double()[0]) + pos.double()[pos_ids]
    v32 = (word.cpu()[ids.cpu()] + typ.cpu()[0]) + pos.cpu()[pos_ids.cpu()]
    ref, plain = ln64(v64, g, b), ln32_cpu(v32, g, b)
    ceil = CEIL_LN_F32 if to == "f32" else CEIL_LN_BF16
    for drop in (None, (0.3, 2 ** 63 + 5, 77), (0.1, 1234, 2 ** 33)):
        out = Guard(n * stride, h, TD[to])
        buf = out.v.view(n, stride, h)
        mh.embed_ln(ids, None, pos_ids, word, pos, typ, g, b, LN_EPS, buf, stride, dropout=drop)
        assert out.intact() and bool((buf[:, t:] == SENTINEL).all())
        what = "embed_ln %s" % ("p=%g" % drop[0] if drop else "no dropout")
        if drop is None:
            check(tol, "ln fwd", what, buf[:, :t], ref, plain, ceil)
        else:
            p, seed, off = drop
            keep = host_keep(seed, off, (n, stride, h), p)[:, :t]
            assert torch.equal(buf[:, :t] != 0, keep), what
            check(tol, "ln fwd", what, buf[:, :t], ref * keep * scale32(p), plain * keep.cpu() * scale32(p), ceil)


@pytest.mark.parametrize("act", ["gelu", "tanh"])
def test_act_bwd_on_a_grid(mh, tol, act):
    n = 300001
    x = torch.linspace(-12.0, 12.0, n, dtype=torch.float64, device="cuda").float()
    x[n // 2], x[n // 2 + 1] = 0.0, -0.0
    assert x[0] == -12 and x[-1] == 12 and x[n // 2] == 0
    d = rand((n,), 5)

    def grad(v):
        if act == "tanh":
            return 1.0 - torch.tanh(v) ** 2
        return 0.5 * (1.0 + torch.erf(v * 0.7071067811865476)) + v * torch.exp(-0.5 * v * v) * 0.3989422804014327

    out = Guard(1, n, torch.float32)
    rc = mh.lib().modcr_act_bwd(mh._ptr(d), mh._ptr(x), mh._ptr(out.v), n, mh.ACT_GELU if act == "gelu" else mh.ACT_TANH, mh._stream())
    assert rc == 0, mh.lib().modcr_last_error()
    assert out.intact()
    check(tol, "act_bwd", act, out.v[0], d.double() * grad(x.double()), d.cpu() * grad(x.cpu()), CEIL_ACT_BWD)
