"""Every route of the bf16 GEMM dispatcher (csrc/gemm.hip: route_bf16) against a float64 reference.

Shape-parametrized tests cannot see which kernel a shape reached: a heuristic change moves them off the kernel they were
written for without failing.  Each case here first asserts the route modcr_linear_route reports (kernel, epilogue, column
groups, reversed walk), then runs the product and compares EVERY element with a float64 product of the bf16 operands,
formed on the device in row blocks.

Bounds (element-wise): |out - ref| <= half an output ulp of |ref| + tol * scale, scale = max |ref| of the row block.  The
reference applies the activation the epilogues implement (GELU: Page's logistic form of the normal CDF, common.h gelu2, which
test_logistic_gelu_is_the_documented_approximation holds to the exact erf GELU), so tol only covers fp32 accumulation and the
fp32 epilogue arithmetic: a skipped K-tile, a wrong row or column or a stride mix-up is orders of magnitude above it.

Operands are strided (lda > K, ldw > K, ldc > N, ldr > N) with NaN in the A / W padding columns and the A rows past M, so a
kernel that reads them produces a non-finite output; the C padding columns and the C rows past M hold a sentinel that must
come back unchanged."""
import collections

import pytest
import torch

import helpers as H
import modcr_hip as mh

pytestmark = pytest.mark.gpu

DX_TOL = 8.7e-8     # test_ffn_up_dx_through_bwd_input (see Case.tol)
EXTRA_ROWS = 3      # rows allocated past M (A: NaN, C: sentinel)
SENTINEL = 1234.5   # exact in bf16, fp16 and fp32

OUT = {"bf16": (mh.BF16, torch.bfloat16), "f16": (mh.F16, torch.float16), "f32": (mh.F32, torch.float32)}
RES = {None: (0, None), "bf16": (mh.BF16, torch.bfloat16), "f32": (mh.F32, torch.float32)}
NONE, GELU, TANH = mh.ACT_NONE, mh.ACT_GELU, mh.ACT_TANH


def R(kernel, direct=0, spec=0, ngroup=0, rev=0):
    return mh.LinearRoute(kernel, direct, spec, ngroup, rev)


# pad = (lda - K, ldw - K, ldc - N, ldr - N)
# tol: the element-wise bound as a multiple of scale beyond half an output ulp, ~2x its observed use (README.md, Tolerances)
Case = collections.namedtuple("Case", "id m n k act res out pad route tol")
PAD = (8, 16, 8, 24)
DENSE = (0, 0, 0, 0)

CASES = [
    # ring kernels (linear_bf16_kernel<TileS | TileM | TileL>)
    Case("ring128_tanh_bf16res_f32", 300, 256, 128, TANH, "bf16", "f32", PAD, R("ring128"), 1.8e-7),
    Case("ring128_none_bf16res_f16", 777, 264, 192, NONE, "bf16", "f16", PAD, R("ring128"), 7.8e-8),
    Case("ring192_gelu_bf16", 7180, 1152, 256, GELU, None, "bf16", PAD, R("ring192"), 1.5e-7),
    Case("ring192_k64_f32res_f32", 20000, 1024, 192, NONE, "f32", "f32", PAD, R("ring192"), 3.7e-7),
    Case("ring256_gelu_bf16", 16300, 2048, 320, GELU, None, "bf16", PAD, R("ring256"), 1.7e-7),
    # persistent 256 x 256 (linear_bf16_p8_kernel): register / LDS / seamless-ring epilogues
    Case("p8_direct_gelu_f32", 5384, 1536, 256, GELU, None, "f32", PAD, R("p8", direct=1), 4.7e-7),
    Case("p8_direct_gelu_bf16", 5384, 1536, 256, GELU, None, "bf16", PAD, R("p8", direct=1), 9e-8),
    Case("p8_lds_bf16res_bf16", 5384, 1536, 256, NONE, "bf16", "bf16", PAD, R("p8"), 1.8e-7),
    Case("p8_lds_tanh_f32res_f32", 5384, 1536, 256, TANH, "f32", "f32", PAD, R("p8"), 2.4e-7),
    Case("p8_lds_bf16res_f16", 5384, 1536, 256, NONE, "bf16", "f16", PAD, R("p8"), 1.2e-7),
    Case("p8_spec_tanh_bf16", 5632, 1536, 256, TANH, None, "bf16", PAD, R("p8", direct=1, spec=1), 6.9e-7),
    Case("p8_spec_none_f16", 5632, 1536, 256, NONE, None, "f16", PAD, R("p8", direct=1, spec=1), 1.3e-7),
    Case("p8_ngroup_direct_bf16", 20100, 2048, 1024, NONE, None, "bf16", PAD, R("p8", direct=1, ngroup=4), 3e-7),
    Case("p8_ngroup_spec_gelu_bf16", 20224, 2048, 1024, GELU, None, "bf16", PAD, R("p8", direct=1, spec=1, ngroup=4), 3.9e-7),
    # persistent 192 x 384 (linear_bf16_t192_kernel)
    Case("t192_direct_gelu_f32", 12104, 1152, 256, GELU, None, "f32", PAD, R("t192", direct=1), 4.9e-7),
    Case("t192_direct_none_f16", 12104, 1152, 256, NONE, None, "f16", PAD, R("t192", direct=1), 2.2e-7),
    Case("t192_lds_f32res_f32", 12104, 1152, 256, NONE, "f32", "f32", PAD, R("t192"), 3.5e-7),
    Case("t192_lds_tanh_bf16res_bf16", 12104, 1152, 256, TANH, "bf16", "bf16", PAD, R("t192"), 8.6e-8),
    # reversed walk (M K 2 > 256 MB), ragged last tile row except where the seamless ring needs M % 256 == 0
    Case("rev_p8_spec_bf16", 140032, 1024, 1024, NONE, None, "bf16", PAD, R("p8", direct=1, spec=1, rev=1), 3.6e-7),
    Case("rev_p8_lds_f32res_f32", 140000, 1024, 1024, NONE, "f32", "f32", PAD, R("p8", rev=1), 8.7e-7),
    Case("rev_p8_ngroup_direct_gelu_bf16", 139960, 2048, 1024, GELU, None, "bf16", PAD, R("p8", direct=1, ngroup=4, rev=1), 5.5e-7),
    Case("rev_t192_direct_f16", 44000, 768, 3072, NONE, None, "f16", PAD, R("t192", direct=1, rev=1), 8.6e-7),
    Case("rev_t192_lds_bf16res_bf16", 44000, 768, 3072, NONE, "bf16", "bf16", PAD, R("t192", rev=1), 5.8e-7),
    # ldc % 8 != 0: the persistent kernels refuse it (16-byte row stores); the ring kernels take it, vectorized (ldc % 4 == 0)
    # or element by element
    Case("ldc4_fallback_bf16", 5384, 1536, 256, GELU, None, "bf16", (8, 16, 4, 24), R("ring256"), 9e-8),
    Case("ldc1_fallback_f32res_f32", 5384, 1536, 256, NONE, "f32", "f32", (8, 16, 1, 24), R("ring256"), 3.4e-7),
    # the headline's own launches at their real sizes (dense operands, as the model lays them out)
    Case("ffn_up_92160", 92160, 3072, 768, GELU, None, "bf16", DENSE, R("p8", direct=1, spec=1, ngroup=6), 5.1e-7),
    Case("ffn_up_143872", 143872, 3072, 768, GELU, None, "bf16", DENSE, R("p8", direct=1, spec=1, ngroup=6), 4.1e-7),
    Case("ffn_down_92160", 92160, 768, 3072, NONE, None, "f16", DENSE, R("t192", direct=1, rev=1), 1e-6),
    Case("ffn_down_143872", 143872, 768, 3072, NONE, None, "f16", DENSE, R("p8", direct=1, spec=1, rev=1), 1.1e-6),
    Case("proj_92160", 92160, 768, 768, NONE, None, "f16", DENSE, R("t192", direct=1), 5e-7),
]


def gelu_logistic(x):
    """the GELU the bf16 epilogues compute (common.h gelu2): x / (1 + exp(-(1.59576912 x + 0.07135481 x^3)))"""
    return x / (1.0 + torch.exp(-(1.59576912161 * x + 0.07135481283 * x ** 3)))


ACT_REF = {NONE: lambda v: v, GELU: gelu_logistic, TANH: torch.tanh}


class Operands(object):
    """A [M+3, lda], W [N, ldw], bias [N], residual [M, ldr], C [M+3, ldc] on the device; NaN / sentinel padding."""

    def __init__(self, c, seed=0, lda=None):
        dev = torch.device("cuda")
        g = torch.Generator(device=dev)
        g.manual_seed(seed * 7919 + c.m * 31 + c.n * 7 + c.k)
        pa, pw, pc, pr = c.pad
        self.c = c
        self.lda, self.ldw, self.ldc, self.ldr = (lda or c.k + pa), c.k + pw, c.n + pc, c.n + pr
        self.A = torch.full((c.m + EXTRA_ROWS, self.lda), float("nan"), dtype=torch.bfloat16, device=dev)
        self.A[:c.m, :c.k] = torch.randn((c.m, c.k), generator=g, device=dev).to(torch.bfloat16)
        self.W = torch.full((c.n, self.ldw), float("nan"), dtype=torch.bfloat16, device=dev)
        self.W[:, :c.k] = (torch.randn((c.n, c.k), generator=g, device=dev) / c.k ** 0.5).to(torch.bfloat16)
        self.bias = 0.5 * torch.randn((c.n,), generator=g, device=dev)
        self.res_dt, rt = RES[c.res]
        self.res = None
        if rt is not None:
            self.res = torch.full((c.m, self.ldr), float("nan"), dtype=rt, device=dev)
            self.res[:, :c.n] = torch.randn((c.m, c.n), generator=g, device=dev).to(rt)
        self.out_dt, self.ot = OUT[c.out]
        self.C = torch.full((c.m + EXTRA_ROWS, self.ldc), SENTINEL, dtype=self.ot, device=dev)

    def views(self):
        c = self.c
        return (self.A[:c.m, :c.k], self.W[:, :c.k], None if self.res is None else self.res[:, :c.n], self.C[:c.m, :c.n])

    def route(self):
        a, w, r, out = self.views()
        return mh.linear_route(a, w, bias=self.bias, residual=r, out_dtype=self.out_dt, act=self.c.act, out=out)

    def run(self):
        c = self.c
        rc = mh.lib().modcr_linear_fwd(self.A.data_ptr(), self.lda, self.W.data_ptr(), self.ldw, self.bias.data_ptr(),
                                       None if self.res is None else self.res.data_ptr(), self.ldr, self.res_dt,
                                       self.C.data_ptr(), self.ldc, c.m, c.n, c.k, c.act, mh.BF16, self.out_dt, mh._stream())
        mh._check(rc, "modcr_linear_fwd")
        torch.cuda.synchronize()
        return self.C[:c.m, :c.n]

    def free(self):
        self.A = self.W = self.bias = self.res = self.C = None


def half_ulp(ref, ot):
    """half an ulp of |ref| in the output type (fp32: none -- tol is the whole bound)"""
    if ot == torch.float32:
        return torch.zeros_like(ref)
    _, e = torch.frexp(ref)                     # |ref| = f 2^e, f in [0.5, 1): ulp = 2^(e - 1 - mantissa bits)
    bits = 7 if ot == torch.bfloat16 else 10
    return torch.ldexp(torch.ones_like(ref), (e - 2 - bits).clamp(min=-25))


def check_reference(ops, what, out=None):
    """element-wise bound against the float64 product of the bf16 operands, row block by row block: |out - ref| <= half an
    output ulp of |ref| + ops.c.tol * scale.  Also: the output is finite, and the C padding holds the sentinel."""
    c = ops.c
    out = ops.views()[3] if out is None else out
    wd = ops.W[:, :c.k].double()
    bd = ops.bias.double()
    coef = c.tol
    used = 0.0
    rows = max(256, (1 << 24) // max(c.k, c.n))
    for r0 in range(0, c.m, rows):
        r1 = min(c.m, r0 + rows)
        ref = ACT_REF[c.act](ops.A[r0:r1, :c.k].double() @ wd.t() + bd)
        if ops.res is not None:
            ref += ops.res[r0:r1, :c.n].double()
        o = out[r0:r1].double()
        assert torch.isfinite(o).all(), "%s: non-finite output in rows %d..%d" % (what, r0, r1)
        err = (o - ref).abs() - half_ulp(ref, ops.ot)
        scale = max(ref.abs().max().item(), 1e-30)
        used = max(used, err.max().item() / scale)
        if used > coef:
            i = int(torch.argmax(err).item())
            row, col = r0 + i // c.n, i % c.n
            raise AssertionError("%s: |out - ref| at (%d, %d) = %g (ref %g): %.3g x scale beyond half an ulp, bound %g"
                                 % (what, row, col, abs(o.flatten()[i] - ref.flatten()[i]).item(), ref.flatten()[i].item(),
                                    used, coef))
    H.report_use(what, used, coef, kind="(|err|-ulp/2)/scale")
    return used


def check_canaries(ops, what):
    c = ops.c
    bits = {torch.bfloat16: torch.int16, torch.float16: torch.int16, torch.float32: torch.int32}[ops.ot]
    want = torch.tensor([SENTINEL], dtype=ops.ot).view(bits).item()
    past = ops.C[c.m:].view(bits)
    assert (past == want).all(), "%s: C rows past M were written" % what
    if ops.ldc > c.n:
        assert (ops.C[:c.m, c.n:].view(bits) == want).all(), "%s: C padding columns were written" % what


def bits_of(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


@pytest.mark.parametrize("c", CASES, ids=[c.id for c in CASES])
def test_route_table(mh_gpu, c):
    ops = Operands(c)
    try:
        got = ops.route()
        assert got == c.route, "%s: dispatcher route %s, the table expects %s" % (c.id, got, c.route)
        ops.run()
        check_reference(ops, c.id)
        check_canaries(ops, c.id)
    finally:
        ops.free()


def test_ffn_up_dx_through_bwd_input(mh_gpu):
    """dX of FFN-up at the headline size: modcr_ffn_up_du_bwd -> dX = du . W1 + dx_residual (fp32, added in the epilogue),
    bf16 out.  The route is queried with the arguments the inner modcr_linear_fwd call receives (A = du, W = W1^T [H, I] in
    the workspace, the fp32 residual, C = dx)."""
    m, h, i = 92160, 768, 3072
    dev = torch.device("cuda")
    g = torch.Generator(device=dev)
    g.manual_seed(11)
    du = (0.1 * torch.randn((m, i), generator=g, device=dev)).to(torch.bfloat16)
    x = torch.randn((m, h), generator=g, device=dev).to(torch.bfloat16)
    w1 = (torch.randn((i, h), generator=g, device=dev) / i ** 0.5).to(torch.bfloat16)
    res = torch.randn((m, h), generator=g, device=dev)
    assert mh.ffn_keep_supported(x, w1)
    wt = torch.empty((h, i), dtype=torch.bfloat16, device=dev)
    got = mh.linear_route(du, wt, residual=res, out_dtype=mh.BF16, out=torch.empty_like(x))
    assert got == R("t192", rev=1), got
    dx, _, _ = mh.ffn_up_du_bwd(du, x, w1, dx_residual=res)
    torch.cuda.synchronize()
    wd = w1.double()
    used = 0.0
    for r0 in range(0, m, 8192):
        ref = du[r0:r0 + 8192].double() @ wd + res[r0:r0 + 8192].double()
        o = dx[r0:r0 + 8192].double()
        assert torch.isfinite(o).all()
        err = (o - ref).abs() - half_ulp(ref, torch.bfloat16)
        used = max(used, err.max().item() / ref.abs().max().item())
    H.report_use("ffn_up dX (t192 rev, fp32 residual)", used, DX_TOL, kind="(|err|-ulp/2)/scale")
    assert used <= DX_TOL, used


def test_logistic_gelu_is_the_documented_approximation():
    """the reference's GELU is within the documented 5e-4 of the exact erf GELU (common.h gelu2)"""
    x = torch.linspace(-12, 12, 200001, dtype=torch.float64)
    exact = 0.5 * x * (1 + torch.erf(x / 2 ** 0.5))
    err = (gelu_logistic(x) - exact).abs().max().item()
    H.report_use("logistic GELU vs erf GELU", err, 5e-4, kind="max|err|")
    assert err <= 5e-4


# ---- forced routes (tuning library: the MODCR_GEMM_* knobs) --------------------------------------------------------------
FORCE = {
    "spec": Case("force_spec", 5632, 1536, 256, GELU, None, "bf16", PAD, R("p8", direct=1, spec=1), 1.5e-7),
    "p8_lds": Case("force_p8_lds", 5384, 1536, 256, NONE, "f32", "f32", PAD, R("p8"), 3.9e-7),
    "p8_direct": Case("force_p8_direct", 5384, 1536, 256, TANH, None, "bf16", PAD, R("p8", direct=1), 6.4e-7),
    "t192_direct": Case("force_t192_direct", 12104, 1152, 256, NONE, None, "f16", PAD, R("t192", direct=1), 2.2e-7),
    "t192_lds": Case("force_t192_lds", 12104, 1152, 256, GELU, "bf16", "bf16", PAD, R("t192"), 1.4e-7),
    "ngroup": Case("force_ngroup", 20100, 2048, 1024, GELU, None, "bf16", PAD, R("p8", direct=1, ngroup=4), 3.7e-7),
}


def forced(ops, monkeypatch, env, want):
    """run `ops` with the knobs `env`; the route must be `want`; returns a copy of the output"""
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    try:
        got = ops.route()
        assert got == want, "%s under %s: route %s, expected %s" % (ops.c.id, env, got, want)
        ops.C.fill_(SENTINEL)
        out = ops.run().clone()
        check_canaries(ops, "%s %s" % (ops.c.id, env))
        return out
    finally:
        for k in env:
            monkeypatch.delenv(k)


@pytest.mark.parametrize("name", ["spec", "p8_lds", "t192_direct", "t192_lds"])
def test_reversed_walk_is_bit_identical(tuning_lib, monkeypatch, name):
    """MODCR_GEMM_REV = 0 vs 1: the walk order changes, the per-tile arithmetic does not (gemm.hip rev_walk_for), so the outputs
    are bit-identical.  Ragged M on every route but the seamless ring, which needs M % 256 == 0."""
    c = FORCE[name]
    ops = Operands(c, seed=1)
    fwd = forced(ops, monkeypatch, {"MODCR_GEMM_REV": 0}, c.route)
    rev = forced(ops, monkeypatch, {"MODCR_GEMM_REV": 1}, c.route._replace(rev_walk=1))
    assert torch.equal(bits_of(fwd), bits_of(rev)), "%s: reversed walk differs from the forward walk" % c.id
    check_reference(ops, c.id + " rev", out=rev)
    ops.free()


def test_column_groups_are_bit_identical(tuning_lib, monkeypatch):
    """MODCR_GEMM_NGROUP = 0 (row-major walk) vs the default column groups: bit-identical, ragged M, and with the reversed walk"""
    c = FORCE["ngroup"]
    ops = Operands(c, seed=2)
    grouped = forced(ops, monkeypatch, {}, c.route)
    plain = forced(ops, monkeypatch, {"MODCR_GEMM_NGROUP": 0}, c.route._replace(ngroup=0))
    assert torch.equal(bits_of(grouped), bits_of(plain)), "column-grouped walk differs from the row-major walk"
    both = forced(ops, monkeypatch, {"MODCR_GEMM_REV": 1}, c.route._replace(rev_walk=1))
    assert torch.equal(bits_of(grouped), bits_of(both)), "reversed column-grouped walk differs"
    check_reference(ops, c.id, out=grouped)
    ops.free()


def test_forced_epilogues(tuning_lib, monkeypatch):
    """MODCR_GEMM_SPEC = 0 / 1 and MODCR_GEMM_DIRECT = 0 / 1 / 2, each held to the float64 reference.  Bit-equality where the K
    accumulation is the same: the seamless ring (SPEC) and the register epilogue (DIRECT = 1) issue the same operand-swapped MFMA
    sequence (gemm.hip, the K loop: `if constexpr (DIRECT)`), so SPEC = 0 vs 1 must agree bit for bit.  The LDS epilogue
    (DIRECT = 0) accumulates the transposed product, whose per-element summation order the hardware does not promise to keep:
    held to the reference only."""
    c = FORCE["spec"]
    ops = Operands(c, seed=3)
    spec = forced(ops, monkeypatch, {"MODCR_GEMM_SPEC": 1}, c.route)
    check_reference(ops, "spec=1", out=spec)
    nospec = forced(ops, monkeypatch, {"MODCR_GEMM_SPEC": 0}, R("p8", direct=1))
    check_reference(ops, "spec=0", out=nospec)
    assert torch.equal(bits_of(spec), bits_of(nospec)), "seamless ring differs from the register epilogue"
    lds = forced(ops, monkeypatch, {"MODCR_GEMM_DIRECT": 0}, R("p8"))
    check_reference(ops, "spec shape, direct=0", out=lds)
    ops.free()
    for name, with_res in (("p8_lds", True), ("t192_lds", True), ("p8_direct", False), ("t192_direct", False)):
        c = FORCE[name]
        ops = Operands(c, seed=4)
        for direct in (0, 1, 2):
            d = 1 if direct == 2 or (direct == 1 and not with_res) else 0
            out = forced(ops, monkeypatch, {"MODCR_GEMM_DIRECT": direct}, c.route._replace(direct=d))
            check_reference(ops, "%s direct=%d" % (name, direct), out=out)
        ops.free()


# ---- 32-bit offset guards: t192_ok (M lda < 2^30), p8_ok (M lda < 2^31) ---------------------------------------------------
GUARDS = [
    # (id, case, lda, route): K = 256 real columns of a row of lda elements, the rest NaN
    ("t192_below", Case("t192_below", 40000, 384, 256, NONE, None, "bf16", DENSE, None, 1.1e-7), 26840, R("t192", direct=1)),
    ("t192_above", Case("t192_above", 40000, 384, 256, NONE, None, "bf16", DENSE, None, 1.1e-7), 26848, R("ring128")),
    ("p8_below", Case("p8_below", 40000, 256, 256, NONE, None, "f32", DENSE, None, 4.5e-7), 53680, R("p8", direct=1)),
    ("p8_above", Case("p8_above", 40000, 256, 256, NONE, None, "f32", DENSE, None, 4.5e-7), 53688, R("ring256")),
]


@pytest.mark.parametrize("gid,c,lda,route", GUARDS, ids=[g[0] for g in GUARDS])
def test_offset_guards(mh_gpu, gid, c, lda, route):
    """a huge lda (2-4 GB of A, nearly all NaN padding) on either side of the 32-bit offset limit of each persistent kernel:
    the route is the one the guard selects, and the last tile rows -- the largest byte offsets -- are correct"""
    ops = Operands(c, lda=lda)
    try:
        got = ops.route()
        assert got == route, "%s: route %s, expected %s (M lda = %d)" % (gid, got, route, c.m * lda)
        ops.run()
        check_reference(ops, gid)
        check_canaries(ops, gid)
    finally:
        ops.free()
        torch.cuda.empty_cache()


@pytest.fixture
def mh_gpu():
    assert torch.cuda.is_available()
    return mh
