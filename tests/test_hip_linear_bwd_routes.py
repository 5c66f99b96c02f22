"""Every route of the linear backward (csrc/gemm.hip: route_bwd_weight, route_bwd_input) against a float64 reference.

The shape-parametrized dW / dX tests of test_hip_kernels.py cannot see which form a shape reached: a change to a predicate moves
them off the form they were written for without failing.  Each case here first asserts the route that
modcr_linear_bwd_weight_route / modcr_linear_bwd_input_route report (form, split plan, product launcher, direct output, reduction,
the way db is formed), then runs the entry through lib() and compares EVERY element of dW, db and dX with a float64 product of
the operands as the kernels see them: rounded to bf16 wherever the form rounds them (every form but the exact fp32 one).

Bound (element-wise): |out - ref| <= half an output ulp of |ref| (bf16 dX; none for fp32) + tol * scale, scale = max |ref|.  tol
is per case, about twice the use recorded in profiles/linear_bwd_routes_tolerance_report.txt (README.md, Tolerances); it covers
fp32 accumulation over M tokens in the order the split plan gives and nothing else.  That is still a test: operands are N(0, 1)
(dY scaled by 0.1), so one dropped or doubled 64-token K-tile moves an element by ~0.1 * sqrt(64) / (0.1 * sqrt(M) * 4) of scale,
1e-1 to 1e-2 at these sizes, against tol ~ 1e-7 to 1e-6; a wrong row, column or stride is larger still.

Operands are strided (lddy = N + 8, ldx = K + 16, ldw = K + 16, lddx = K + 8) with NaN in the padding columns and in three rows
past M, so a kernel that reads them produces a non-finite output.  dW and db start from a sentinel for plain calls (it must be
gone) and from known values for accumulating ones; a row of dW past N, an element of db past N and the padding of dX must come
back unchanged."""
import collections

import pytest
import torch

import helpers as H
import modcr_hip as mh

pytestmark = pytest.mark.gpu

EXTRA_ROWS = 3
SENTINEL = 1234.5
BF, F32 = mh.BF16, mh.F32
TT = {BF: torch.bfloat16, F32: torch.float32}


def W(form, splits=0, kps=0, product="splitk", direct=0, reduction="plain", db="fused_reduce"):
    return mh.BwdWeightRoute(form, splits, kps, product, direct, reduction, db)


F32_ROUTE = W("f32", product="f32", direct=1, reduction="none", db="colsum")

# ws: "full" = modcr_linear_bwd_weight_workspace bytes, "short" = one byte less (the silent fall-back), None = no workspace
# pad = (lddy - N, ldx - K)
WCase = collections.namedtuple("WCase", "id m n k dy x db acc ws pad route tol")
PAD = (8, 16)
W_CASES = [
    # HALF_TN (K >= N): dY transposed, X token-major
    WCase("half_tn_direct", 256, 256, 256, BF, BF, True, False, "full", PAD, W("half_tn", 1, 4, direct=1, reduction="none", db="fused_fold"), 3.6e-7),
    WCase("half_tn_accumulate", 256, 256, 256, BF, BF, True, True, "full", PAD, W("half_tn", 1, 4), 3.5e-7),
    WCase("half_tn_reread_last_tile", 320, 256, 256, BF, BF, True, False, "full", PAD, W("half_tn", 2, 4), 4.6e-7),      # Mp 512 > M
    WCase("half_tn_transpose256", 4096, 256, 256, BF, BF, True, False, "full", PAD, W("half_tn", 16, 4), 3.4e-7),
    WCase("half_tn_ragged_tail", 4160, 256, 512, BF, BF, True, True, "full", PAD, W("half_tn", 17, 4), 3.7e-7),           # Mp 4352
    WCase("half_tn_f32dy_rowsum", 256, 256, 256, F32, BF, True, False, "full", (4, 16), W("half_tn", 1, 4, direct=1, reduction="none", db="rowsum"), 3.6e-7),
    WCase("half_tn_no_db", 320, 256, 256, BF, BF, False, False, "full", PAD, W("half_tn", 2, 4, db="none"), 4.6e-7),
    # SWAPPED (N > K): dW^T = X^T . dY, the plan of (M, K, N)
    WCase("swapped_1", 256, 512, 256, BF, BF, True, False, "full", PAD, W("swapped", 1, 4, reduction="transposed", db="block_fold"), 3.9e-7),
    WCase("swapped_16_accumulate", 4096, 512, 256, BF, BF, True, True, "full", PAD, W("swapped", 16, 4, reduction="transposed", db="block_fold"), 3.6e-7),
    # NT: both transposed
    WCase("nt_f32x_splitk", 256, 256, 256, BF, F32, True, False, "full", PAD, W("nt", 1, 4, direct=1, reduction="none", db="fused_fold"), 3.6e-7),
    WCase("nt_dispatch", 320, 192, 320, BF, BF, True, False, "full", PAD, W("nt", 2, 4, product="dispatch"), 4.1e-7),
    WCase("nt_m200", 200, 256, 256, BF, BF, True, True, "full", PAD, W("nt", 1, 4), 3.6e-7),
    # a workspace one byte short of the query, or none: the exact fp32 form, no error
    WCase("short_half_tn", 256, 256, 256, BF, BF, True, False, "short", PAD, F32_ROUTE, 5.7e-7),
    WCase("short_swapped", 256, 512, 256, BF, BF, True, True, "short", PAD, F32_ROUTE, 4.7e-7),
    WCase("short_nt", 320, 192, 320, F32, F32, False, False, "short", PAD, F32_ROUTE._replace(db="none"), 1.2e-6),
    WCase("no_workspace", 256, 256, 256, F32, BF, True, False, None, PAD, F32_ROUTE, 1.3e-6),
]
# the tuning library's opt-in form (MODCR_GEMM_TN=1): no transposes, db by float atomics
TN_CASE = WCase("tn_forced", 512, 256, 256, BF, BF, True, False, "full", PAD, W("tn", 2, 4, db="atomic"), 3.1e-7)

# dX: res = an fp32 residual added in the epilogue (the composites' path); out = dX dtype
XCase = collections.namedtuple("XCase", "id m n k dy w out res ws route tol")
X_CASES = [
    XCase("splitk", 256, 1024, 256, BF, BF, F32, False, "full", mh.BwdInputRoute("splitk", 0, None), 2.5e-7),
    XCase("fwd_residual", 256, 1024, 256, BF, BF, BF, True, "full", mh.BwdInputRoute("fwd", 0, mh.LinearRoute("ring128", 0, 0, 0, 0)), 7.4e-9),
    XCase("fwd_cast_pad", 300, 100, 200, F32, BF, F32, False, "full", mh.BwdInputRoute("fwd", 1, mh.LinearRoute("ring128", 0, 0, 0, 0)), 3.3e-7),
    XCase("f32_small_n", 300, 48, 200, BF, BF, F32, False, "full", mh.BwdInputRoute("f32", 0, None), 2.2e-7),
    XCase("f32_no_workspace", 256, 1024, 256, BF, F32, F32, False, None, mh.BwdInputRoute("f32", 0, None), 2.4e-6),
]
X_REFUSED = (300, 100, 200)       # bf16 dY, N % 64 != 0, with a workspace
X_REFUSED_MESSAGE = "linear_bwd_input: bf16 dY needs N % 64 == 0"


def workspace_bytes(query, c):
    need = query(c.m, c.n, c.k)
    return {"full": need, "short": need - 1, None: 0}[c.ws]


def weight_route(c, **ptrs):
    return mh.linear_bwd_weight_route(c.m, c.n, c.k, dy_dtype=c.dy, dtype=c.x, db=c.db, accumulate=c.acc, lddy=c.n + c.pad[0], ldx=c.k + c.pad[1],
                                      workspace_bytes=workspace_bytes(mh.lib().modcr_linear_bwd_weight_workspace, c), **ptrs)


def input_route(c, **ptrs):
    return mh.linear_bwd_input_route(c.m, c.n, c.k, dy_dtype=c.dy, dtype=c.w, out_dtype=c.out, residual=ptrs.pop("residual", c.res),
                                     lddy=c.n + 8, ldw=c.k + 16, lddx=c.k + 8, ldr=c.k,
                                     workspace_bytes=workspace_bytes(mh.lib().modcr_linear_bwd_input_workspace, c), **ptrs)


def padded(rows, cols, ld, dt, g, scale=1.0, extra=EXTRA_ROWS):
    """[rows + extra, ld] of NaN with N(0, scale) in [:rows, :cols]"""
    t = torch.full((rows + extra, ld), float("nan"), dtype=TT[dt], device="cuda")
    t[:rows, :cols] = (scale * torch.randn((rows, cols), generator=g, device="cuda")).to(TT[dt])
    return t


def as_seen(t, rounds):
    """the operand in float64, rounded to bf16 first where the form rounds it"""
    return (t.to(torch.bfloat16) if rounds else t).double()


def used_of(out, ref, what, ot=torch.float32):
    """(|out - ref| - half an output ulp of |ref|) / max |ref|, the largest over all elements"""
    o = out.double()
    assert torch.isfinite(o).all(), "%s: non-finite output" % what
    half = torch.zeros_like(ref)
    if ot == torch.bfloat16:
        _, e = torch.frexp(ref)
        half = torch.ldexp(torch.ones_like(ref), (e - 9).clamp(min=-25))
    return (((o - ref).abs() - half).max() / ref.abs().max().clamp(min=1e-30)).item()


def held(what, used, tol):
    H.report_use(what, used, tol, kind="(|err|-ulp/2)/scale")
    assert used <= tol, "%s: %.3g x scale beyond half an ulp, bound %g" % (what, used, tol)


def run_weight(c, seed=0):
    """runs modcr_linear_bwd_weight for the case; returns (route, use of dW, use of db or None, dW, db)"""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed * 7919 + c.m * 31 + c.n * 7 + c.k)
    lddy, ldx = c.n + c.pad[0], c.k + c.pad[1]
    dy = padded(c.m, c.n, lddy, c.dy, g, 0.1)
    x = padded(c.m, c.k, ldx, c.x, g)
    dw = torch.full((c.n + 1, c.k), SENTINEL, dtype=torch.float32, device="cuda")
    db = torch.full((c.n + 1,), SENTINEL, dtype=torch.float32, device="cuda")
    if c.acc:
        dw[:c.n] = torch.randn((c.n, c.k), generator=g, device="cuda")
        db[:c.n] = torch.randn((c.n,), generator=g, device="cuda")
    dw0, db0 = dw[:c.n].double().clone(), db[:c.n].double().clone()
    nb = workspace_bytes(mh.lib().modcr_linear_bwd_weight_workspace, c)
    ws = torch.empty((max(nb, 1),), dtype=torch.uint8, device="cuda") if c.ws else None
    route = weight_route(c, dy=dy, x=x, dw=dw, workspace=ws)
    rc = mh.lib().modcr_linear_bwd_weight(dy.data_ptr(), lddy, c.dy, x.data_ptr(), ldx, dw.data_ptr(), db.data_ptr() if c.db else None,
                                          c.m, c.n, c.k, int(c.acc), c.x, ws.data_ptr() if c.ws else None, nb, mh._stream())
    mh._check(rc, "modcr_linear_bwd_weight")
    torch.cuda.synchronize()
    rounds = route.form != "f32"
    dyd, xd = as_seen(dy[:c.m, :c.n], rounds), as_seen(x[:c.m, :c.k], rounds)
    ref_w = dyd.t() @ xd + (dw0 if c.acc else 0.0)
    ref_b = dyd.sum(0) + (db0 if c.acc else 0.0)
    use_w = used_of(dw[:c.n], ref_w, c.id + " dW")
    assert (dw[c.n:] == SENTINEL).all(), "%s: the dW row past N was written" % c.id
    use_b = used_of(db[:c.n], ref_b, c.id + " db") if c.db else None
    assert (db[c.n:] == SENTINEL).all() and (c.db or (db == SENTINEL).all()), "%s: db written where it must not be" % c.id
    return route, use_w, use_b, dw[:c.n], db[:c.n]


@pytest.mark.parametrize("c", W_CASES, ids=[c.id for c in W_CASES])
def test_weight_route_table(c):
    route, use_w, use_b, _, _ = run_weight(c)
    assert route == c.route, "%s: route %s, the table expects %s" % (c.id, route, c.route)
    held(c.id + " dW", use_w, c.tol)
    if c.db:
        held(c.id + " db", use_b, c.tol)


def test_weight_forced_tn(tuning_lib, monkeypatch):
    """the tuning library's TN form (MODCR_GEMM_TN=1), and HALF_TN off (MODCR_GEMM_HALF_TN=0): the same shape through NT"""
    c = TN_CASE
    monkeypatch.setenv("MODCR_GEMM_TN", "1")
    route, use_w, use_b, _, _ = run_weight(c)
    monkeypatch.delenv("MODCR_GEMM_TN")
    assert route == c.route, route
    held("tn dW", use_w, c.tol)
    held("tn db (atomics)", use_b, c.tol)
    monkeypatch.setenv("MODCR_GEMM_HALF_TN", "0")
    route, use_w, use_b, _, _ = run_weight(c)
    monkeypatch.delenv("MODCR_GEMM_HALF_TN")
    assert route == W("nt", 2, 4), route
    held("half_tn off: nt dW", use_w, c.tol)
    held("half_tn off: nt db", use_b, c.tol)


def run_input(c, seed=0):
    """runs the dX entry for the case (with a residual: modcr_ffn_up_du_bwd, dense operands); returns (route, use, dX)"""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed * 7919 + c.m * 31 + c.n * 7 + c.k + 1)
    if c.res:
        du = (0.1 * torch.randn((c.m, c.n), generator=g, device="cuda")).to(torch.bfloat16)
        x = torch.randn((c.m, c.k), generator=g, device="cuda").to(torch.bfloat16)
        w1 = (torch.randn((c.n, c.k), generator=g, device="cuda") / c.n ** 0.5).to(torch.bfloat16)
        res = torch.randn((c.m, c.k), generator=g, device="cuda")
        assert mh.ffn_keep_supported(x, w1)
        route = mh.linear_bwd_input_route(c.m, c.n, c.k, out_dtype=c.out, residual=res, dy=du, w=w1,
                                          workspace_bytes=mh.lib().modcr_ffn_up_du_bwd_workspace(c.m, c.k, c.n))
        dx, _, _ = mh.ffn_up_du_bwd(du, x, w1, dx_residual=res)
        torch.cuda.synchronize()
        ref = du.double() @ w1.double() + res.double()
        return route, used_of(dx, ref, c.id, torch.bfloat16), dx
    lddy, ldw, lddx = c.n + 8, c.k + 16, c.k + 8
    dy = padded(c.m, c.n, lddy, c.dy, g, 0.1)
    w = padded(c.n, c.k, ldw, c.w, g, 1.0 / c.n ** 0.5, extra=0)
    dx = torch.full((c.m + EXTRA_ROWS, lddx), SENTINEL, dtype=TT[c.out], device="cuda")
    nb = workspace_bytes(mh.lib().modcr_linear_bwd_input_workspace, c)
    ws = torch.empty((max(nb, 1),), dtype=torch.uint8, device="cuda") if c.ws else None
    route = input_route(c, dy=dy, w=w, dx=dx, workspace=ws)
    rc = mh.lib().modcr_linear_bwd_input(dy.data_ptr(), lddy, c.dy, w.data_ptr(), ldw, dx.data_ptr(), lddx, c.m, c.n, c.k, c.w, c.out,
                                         ws.data_ptr() if c.ws else None, nb, mh._stream())
    mh._check(rc, "modcr_linear_bwd_input")
    torch.cuda.synchronize()
    rounds = route.form != "f32"
    ref = as_seen(dy[:c.m, :c.n], rounds) @ as_seen(w[:, :c.k], rounds)
    use = used_of(dx[:c.m, :c.k], ref, c.id, TT[c.out])
    assert (dx[c.m:] == SENTINEL).all() and (dx[:c.m, c.k:] == SENTINEL).all(), "%s: dX rows past M or padding columns were written" % c.id
    return route, use, dx[:c.m, :c.k]


@pytest.mark.parametrize("c", X_CASES, ids=[c.id for c in X_CASES])
def test_input_route_table(c):
    route, use, _ = run_input(c)
    assert route == c.route, "%s: route %s, the table expects %s" % (c.id, route, c.route)
    held(c.id + " dX", use, c.tol)


def test_input_refusal_comes_before_any_launch():
    """bf16 dY with N % 64 != 0 and a workspace: refused with the documented code and message, dX untouched"""
    m, n, k = X_REFUSED
    dy = torch.zeros((m, n + 4), dtype=torch.bfloat16, device="cuda")
    w = torch.zeros((n, k), dtype=torch.bfloat16, device="cuda")
    dx = torch.full((m, k), SENTINEL, dtype=torch.float32, device="cuda")
    nb = mh.lib().modcr_linear_bwd_input_workspace(m, n, k)
    ws = torch.empty((nb,), dtype=torch.uint8, device="cuda")
    rc = mh.lib().modcr_linear_bwd_input(dy.data_ptr(), n + 4, BF, w.data_ptr(), k, dx.data_ptr(), k, m, n, k, BF, F32, ws.data_ptr(), nb, mh._stream())
    assert rc == -1 and mh.lib().modcr_last_error().decode() == X_REFUSED_MESSAGE
    with pytest.raises(mh.ModcrHipError, match="bf16 dY needs N % 64 == 0"):
        mh.linear_bwd_input_route(m, n, k, lddy=n + 4)
    torch.cuda.synchronize()
    assert (dx == SENTINEL).all()
