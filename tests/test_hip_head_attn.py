"""The attention kernels of the trainable heads, route by route, against float64 and the host dropout mask:
modcr_align_attn_fwd / _bwd (csrc/rowops.hip) and modcr_cls_xattn_fwd / _bwd (csrc/clsattn.hip).

The four C entries are called through modcr_hip.lib() by thin wrappers of this file that own every buffer, so row strides, guard
rows, aliased k / v and refusals are reachable.  What a case lands on is computed here from its shape by a restatement of the host
rule (align_route: csrc/rowops.hip align_attn_lds; cls_route: the instantiation switch and LDS formula of csrc/clsattn.hip) and
stated in its id; the case tables are module-level and tests/test_host_logic.py asserts without a GPU that they keep every class.
The cases at the largest accepted L, with the refusal one key above, tie the restatements to the C code.

Every comparison is element-wise, of every element, against float64 formed from the SAME stored inputs (bf16 operands are rounded
first), with the dropout mask of helpers.hidden_drop_keep(seed, offset, N * heads * L, p) (counter offset + (n * heads + h) * L + j)
and keep_scale = the fp32 value of 1 / (1 - p).  The bound is that of tests/test_hip_rowops.py:

    |got - ref| <= min(k * max(yardstick, eps32 * scale), ceiling * scale) + half an output ulp at |ref|

yardstick = max |plain fp32 torch CPU evaluation - float64| of that quantity on that case, scale = max(1, max |ref|); the half ulp
for bf16 outputs only; `ceiling` is what tests/test_hip_kernels.py holds the same quantity to.  k is one constant per quantity
family (below).  Every case runs on two score distributions: the peaked one of the older tests and a flat one (max p of the order of
1 / L) in which every key carries weight.

A backward is judged alone: it is fed the reference probabilities rounded to fp32 (cls: also the reference ctx and ssum); one
chained forward -> backward case per family and dtype uses the kernel's own outputs.  Mask agreement is exact: the dv piece of a
dropped (key, head) is exactly zero, that of a kept one with p > 0 is not.

Padding columns of strided operands and the rows before and after every operand (k, v and the x blocks; also q, dout, key_bias, the
fed probabilities, qt, dctx, dssum and the fed ctx / ssum) hold NaN (a kernel that read them would turn non-finite); every output sits between guard rows, strided dk / dv have padding columns, and both hold a sentinel that must come
back bit-identical.  A refused call must write nothing.

Current contract, not changed here: the forward entries accept key counts that the backward entries then refuse (two [L][heads]
tables instead of one in LDS) -- cls_xattn at E = 768: 2176 < L <= 4352; align_attn at E = 768 with 8 heads: 2208 < L <= 4416."""
import ctypes
import os
from collections import namedtuple

import numpy as np
import pytest
import torch

import helpers as H
from test_hip_rowops import EPS32, SENTINEL, Guard, mh, rand, scale32, ulp  # noqa: F401  (mh is a fixture)

pytestmark = pytest.mark.gpu

# k per quantity family: at most 2x the worst (err - half ulp) / max(yardstick, eps32 * scale) of profiles/head_attn_tolerance_report.txt
K_ALIGN_OUT = 6.5       # 3.27: test_align_attn_routes[E1024h1_L3_N3_f32_..._ld1024_1032-peaked]
K_ALIGN_PROBS = 8.1     # 4.06: test_align_attn_routes[E1024h1_L283_N2_f32_..._f283x1_b283x1_ld1024_1032_p0.5_offcross-peaked]
K_ALIGN_DQ = 7.2        # 3.60: test_align_attn_routes[E768h1_L57_N3_bf16_..._ld776_776_bias-ragged_kisv_scale1-peaked]
K_ALIGN_DK = 6.1        # 3.07: test_align_attn_routes[E768h1_L57_N3_f32_..._ld776_768_p0.1_off0_bias-ragged_kisv_scale1-peaked]
K_ALIGN_DV = 1.6        # 0.82: test_align_attn_routes[E768h3_L3_N3_f32_..._ld768_768_p0.1_offmod3-flat]
K_CLS_PROBS = 3.5       # 1.76: test_cls_xattn_routes[E1020_G4U2F_rows1048-1000_L2048_N1_..._p0.1_offcross-peaked]
K_CLS_SSUM = 4.0        # 2.00: test_cls_xattn_routes[E516_G3U4F_rows3-13_L16_N3_ld520_...-peaked] (yardstick below eps32 * scale: two fp32 steps)
K_CLS_CTX = 6.0         # 3.03: test_cls_xattn_routes[E1020_G4U2F_rows1048-1000_L2048_N1_..._p0.1_offcross-peaked]
K_CLS_DQT = 5.8         # 2.94: test_cls_xattn_routes[E128_G1U4F_rows1432-1000_L2432_N1_..._p0.1_offcross-flat]
FAMILY_K = {"align out": K_ALIGN_OUT, "align probs": K_ALIGN_PROBS, "align dq": K_ALIGN_DQ, "align dk": K_ALIGN_DK, "align dv": K_ALIGN_DV,
            "cls probs": K_CLS_PROBS, "cls ssum": K_CLS_SSUM, "cls ctx": K_CLS_CTX, "cls dqt": K_CLS_DQT}
# ceilings: the bounds of tests/test_hip_kernels.py for the same quantities, as a multiple of scale
CEIL = {"align out": 1e-4, "align probs": 1e-4, "align dq": 1e-4, "align dk": {"f32": 1e-3, "bf16": 2e-2},
        "align dv": {"f32": 1e-3, "bf16": 2e-2}, "cls probs": 1e-5, "cls ssum": 1e-5, "cls ctx": 1e-4, "cls dqt": 2e-4}

TD = {"f32": torch.float32, "bf16": torch.bfloat16}
NAN = float("nan")
DISTS = ("peaked", "flat")
SEED = 2 ** 63 + 99                                      # non-zero high word


# ---- host rules, restated -------------------------------------------------------------------------------------------------------
def align_route(l, e, heads, tables):
    """csrc/rowops.hip align_attn_lds + the 160 KB check of the entries: (LB, key blocks, LDS bytes) or None (refused: "too long").
    tables = 1 (forward: scores) or 2 (backward: dp and probabilities)"""
    c = e // 8
    ks = 256 // c
    budget, tab, out = 144 * 1024, tables * l * heads * 4, ks * e * 4
    if tab + out > budget:
        return None
    lb = (budget - tab) // (c * 4)
    lb = l if lb >= l else lb // (4 * ks) * (4 * ks)
    if lb < 4 * ks and lb < l:
        return None
    shm = max(lb * c * 4, out) + tab
    return (lb, -(-l // lb), shm) if shm <= 160 * 1024 else None


def align_geom(e, heads):
    """(C chunks per row, KS key slots, chunks per head, idle threads)"""
    c = e // 8
    return c, 256 // c, c // heads, 256 - (256 // c) * c


def align_last_unblocked(e, heads, tables):
    """the largest L whose keys are one block (LB == L)"""
    l = 1
    while align_route(l + 1, e, heads, tables) is not None and align_route(l + 1, e, heads, tables)[1] == 1:
        l += 1
    return l


def align_max_l(e, heads, tables):
    """the largest accepted L"""
    l = 144 * 1024 // (tables * heads * 4) + 1
    while align_route(l, e, heads, tables) is None:
        l -= 1
    return l


def cls_route(e, l):
    """csrc/clsattn.hip: ((G, U, FULL), forward LDS bytes or None, backward LDS bytes or None); None = refused ("too long")"""
    g = (e + 255) // 256
    inst = (3, 4, True) if e == 768 else (4, 2, True) if e == 1024 else (g, 2 if g == 4 else 4, False)
    tab, red = (l * 8 + 3) & ~3, 8 * 256 * g
    f, b = (tab + red) * 4, (2 * tab + red) * 4
    return inst, (f if f <= 160 * 1024 else None), (b if b <= 160 * 1024 else None)


def cls_max_l(e, tables):
    g = (e + 255) // 256
    return (160 * 1024 // 4 - 8 * 256 * g) // (8 * tables)


def drop_offset(kind, heads, l):
    """"0"; "mod3": offset % 4 == 3; "cross": offset + (n * heads + h) * L + j passes 2^32 in the middle of sequence 0"""
    return {"0": 0, "mod3": 4003, "cross": 2 ** 32 - max(1, heads * l // 2)}[kind]


# ---- case tables (read by tests/test_host_logic.py::test_head_attn_case_tables_cover_every_class) -----------------------------------
AlignCase = namedtuple("AlignCase", "e heads l n dt kpad dpad bias p off alias scale1 noprobs")


def acase(e, heads, l, n=2, dt="bf16", kpad=0, dpad=0, bias=None, p=0.0, off="0", alias=False, scale1=False, noprobs=False):
    return AlignCase(e, heads, l, n, dt, kpad, dpad, bias, p, off, alias, scale1, noprobs)


ALIGN_EH = ((8, 1), (64, 8), (128, 2), (520, 5), (768, 8), (768, 3), (1024, 8), (1024, 1), (2048, 8), (2048, 1))
ALIGN_P = (0.0, 0.1, 0.5)
ALIGN_OFF = ("0", "mod3", "cross")
BIAS_KINDS = (None, "ragged", "allmasked", "inf")


def _align_cases():
    cases, i = [], 0

    def add(e, heads, l, **kw):
        # operand and gradient strides (E, E + 8) independently, the dtype and the dropout setting rotate over the table
        nonlocal i
        kw.setdefault("dt", ("bf16", "f32")[i % 2])
        kw.setdefault("kpad", 8 * ((i // 2) % 2))
        kw.setdefault("dpad", 8 * ((i // 3) % 2))
        if "p" not in kw:
            kw["p"], kw["off"] = ALIGN_P[i % 3], ALIGN_OFF[(i // 3) % 3]
        cases.append(acase(e, heads, l, **kw))
        i += 1

    for e, heads in ALIGN_EH:
        ks = align_geom(e, heads)[1]
        for l in sorted({1, 2, 3, 4 * ks, 4 * ks + 1} | ({ks - 1} if ks > 1 else set())):       # fewer keys than slots ... one full pass + 1
            add(e, heads, l, n=3)
        for tables in (1, 2):
            l0 = align_last_unblocked(e, heads, tables)
            lb = align_route(l0 + 1, e, heads, tables)[0]
            add(e, heads, l0)                            # L == LB: one block at the edge of the budget
            add(e, heads, l0 + 1)                        # two blocks, a ragged tail
            lmax = align_max_l(e, heads, tables)
            add(e, heads, min(2 * lb + lb // 2 + 3, lmax - 5))       # three or more blocks, a ragged tail
            add(e, heads, lmax, n=1)
            add(e, heads, lmax + 1, n=1)                 # refused
        lo, hi = align_last_unblocked(e, heads, 2) + 1, align_last_unblocked(e, heads, 1)
        add(e, heads, (lo + hi) // 2)                    # only the backward walks the keys in blocks
    for dt in ("bf16", "f32"):
        for bias in BIAS_KINDS[1:]:
            add(768, 8, 57, n=3, dt=dt, bias=bias)
        add(128, 2, 9, n=3, dt=dt, bias="inf", p=0.5, off="mod3")
        for p in (0.0, 0.1):                             # the ClsLayer2 call: one unscaled head, k is v, the word mask as key_bias
            add(768, 1, 57, n=3, dt=dt, bias="ragged", alias=True, scale1=True, p=p, off="0")
        for p in ALIGN_P[1:]:
            for off in ALIGN_OFF:
                add(768, 8, 237, n=3, dt=dt, p=p, off=off)
        add(520, 5, 40, n=5, dt=dt, p=0.1, off="cross")
        add(768, 8, 57, n=2, dt=dt, noprobs=True, p=0.0)
        for kpad in (0, 8):
            for dpad in (0, 8):
                add(1024, 8, 33, n=2, dt=dt, kpad=kpad, dpad=dpad, p=0.1, off="mod3")
    return list(dict.fromkeys(cases))


ALIGN_CASES = _align_cases()


def align_id(c):
    cc, ks, cph, _ = align_geom(c.e, c.heads)
    f, b = align_route(c.l, c.e, c.heads, 1), align_route(c.l, c.e, c.heads, 2)
    s = "E%dh%d_L%d_N%d_%s_C%d_KS%d_cph%d_f%s_b%s_ld%d_%d" % (
        c.e, c.heads, c.l, c.n, c.dt, cc, ks, cph, "%dx%d" % f[:2] if f else "refused", "%dx%d" % b[:2] if b else "refused",
        c.e + c.kpad, c.e + c.dpad)
    s += "_p%g_off%s" % (c.p, c.off) if c.p else ""
    return s + ("_bias-%s" % c.bias if c.bias else "") + ("_kisv_scale1" if c.alias else "") + ("_noprobs" if c.noprobs else "")


ClsCase = namedtuple("ClsCase", "e rows n ldpad p off stride0")
CLS_E = (4, 128, 256, 260, 512, 516, 764, 768, 772, 1020, 1024)
CLS_MAX_E = (128, 768, 1020)


def _cls_cases():
    cases, i = [], 0
    for e in CLS_E:
        u4 = 4 * cls_route(e, 1)[0][1]
        # L = 1, 2, 3, 4U - 1, 4U, 4U + 1 and 300 in one, two and three blocks, blocks of one row among them
        for rows in ((1,), (2,), (1, 2), (u4 - 1,), (3, u4 - 3), (u4 - 2, 1, 2), (79, 120, 101)):
            cases.append(ClsCase(e, rows, 3, 4 * (i % 2), ALIGN_P[i % 3], ALIGN_OFF[(i // 3) % 3], (i % len(rows)) if i % 4 == 1 else None))
            i += 1
    for e in CLS_MAX_E:
        for tables in (1, 2):
            lmax = cls_max_l(e, tables)
            cases.append(ClsCase(e, (lmax - 1000, 1000), 1, 0, 0.1, "cross", None))
            cases.append(ClsCase(e, (lmax - 1000, 1, 1000), 1, 4, 0.0, "0", None))       # one key too many
    return cases


CLS_CASES = _cls_cases()


def cls_id(c):
    l = sum(c.rows)
    inst, f, b = cls_route(c.e, l)
    s = "E%d_G%dU%d%s_rows%s_L%d_N%d_ld%d_lds%s_%s" % (c.e, inst[0], inst[1], "T" if inst[2] else "F", "-".join(map(str, c.rows)), l, c.n,
                                                       c.e + c.ldpad, f if f else "refused", b if b else "refused")
    s += "_p%g_off%s" % (c.p, c.off) if c.p else ""
    return s + ("_seqstride0@%d" % c.stride0 if c.stride0 is not None else "")


# ---- plumbing -------------------------------------------------------------------------------------------------------------------
class Uses(object):
    """per quantity family over the checks of one test: the worst use of k, the largest yardstick and the worst use of the ceiling.
    MODCR_TEST_REPORT=1 (pytest -s): one `[tol-k]` line per test, condensed by tools/tol_summary.py"""

    def __init__(self):
        self.fam = {}

    def add(self, fam, used, yard, ceil_used):
        u, y, c = self.fam.get(fam, (0.0, 0.0, 0.0))
        self.fam[fam] = (max(u, used), max(y, yard), max(c, ceil_used))

    def flush(self):
        if os.environ.get("MODCR_TEST_REPORT") and self.fam:
            test = os.environ.get("PYTEST_CURRENT_TEST", "").split(" ")[0].split("::", 1)[-1]
            print("  [tol-k] %s | %s" % (test, " | ".join("%s: k-use %.3f yardstick/scale %.2e ceiling-use %.4f" % ((f,) + v)
                                                         for f, v in sorted(self.fam.items()))))


@pytest.fixture
def tol():
    w = Uses()
    yield w
    w.flush()


def check(tol, fam, what, got, ref, plain, dt="f32", extra=None):
    """the bound of the module docstring; got: device tensor of the output dtype, ref: float64, plain: the fp32 evaluation;
    extra: a further element-wise allowance for roundings that are not the kernel's (float64 tensor)"""
    ref = ref.cuda()
    k, ceil = FAMILY_K[fam], CEIL[fam]
    ceil = ceil[dt] if isinstance(ceil, dict) else ceil
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), "%s %s: non-finite output" % (fam, what)
    err = (got.double() - ref).abs()
    scale = max(1.0, ref.abs().max().item())
    yard = (plain.cuda().double() - ref).abs().max().item()
    base = max(yard, EPS32 * scale)
    hu = 0.5 * ulp(ref, got.dtype) if got.dtype != torch.float32 else torch.zeros_like(ref)
    if extra is not None:
        hu = hu + extra.cuda()
    over = (err - hu).clamp_min(0).max().item()
    tol.add(fam, over / base, yard / scale, over / (ceil * scale))
    bad = err > min(k * base, ceil * scale) + hu
    assert not bool(bad.any()), "%s %s: %d elements over the bound, worst |err| %.4g (yardstick %.3g, scale %.3g, k %.3g)" % (
        fam, what, int(bad.sum()), err.max().item(), yard, scale, k)


class Rows(object):
    """[n, l, e] rows of stride ld (elements) between one guard row before and one after; guard rows and the padding columns
    ld - e hold `fill` (NaN for operands, the sentinel for outputs)"""

    def __init__(self, n, l, e, ld, dtype, fill, data=None):
        self.buf = torch.full((n * l + 2, ld), fill, dtype=dtype, device="cuda")
        self.v = self.buf[1:-1].view(n, l, ld)[:, :, :e]
        self.e, self.ld = e, ld
        if data is not None:
            self.v.copy_(data)

    def frame_intact(self):
        torch.cuda.synchronize()
        return bool((self.buf[0] == SENTINEL).all()) and bool((self.buf[-1] == SENTINEL).all()) and bool((self.buf[1:-1, self.e:] == SENTINEL).all())

    def untouched(self):
        torch.cuda.synchronize()
        return bool((self.buf == SENTINEL).all())


def framed(t):
    """a copy of a dense operand between a NaN row before and one after: a kernel that read past it by a row or a sequence would
    turn non-finite"""
    flat = t.reshape(-1, t.shape[-1])
    buf = torch.full((flat.shape[0] + 2, flat.shape[1]), NAN, dtype=t.dtype, device="cuda")
    buf[1:-1] = flat
    return buf[1:-1].view(t.shape)


def keep_weights(p, off, n, heads, l):
    """(keep [n, heads, l] bool, keep * keep_scale float64 with keep_scale the fp32 number of the entries), on the CPU"""
    keep = torch.from_numpy(H.hidden_drop_keep(SEED, off, n * heads * l, p).reshape(n, heads, l)) if p else torch.ones(n, heads, l, dtype=torch.bool)
    return keep, keep.double() * (scale32(p) if p else 1.0)


def last_error(mh):
    return mh.lib().modcr_last_error().decode()


# ---- align_attn ---------------------------------------------------------------------------------------------------------------
def align_fwd(mh, q, k, v, out, probs, c, scale, p, off, bias, ldkv=None, kptr=None):
    n, l, e = k.v.shape
    return mh.lib().modcr_align_attn_fwd(mh._ptr(q), kptr or mh._ptr(k.v), mh._ptr(v.v), k.ld if ldkv is None else ldkv, mh._ptr(out),
                                         mh._ptr(probs), n, l, e, c.heads, float(scale), float(p), SEED, off, mh._ptr(bias),
                                         mh.dt_of(k.v), mh._stream())


def align_bwd(mh, dout, q, k, v, probs, dq, dk, dv, c, scale, p, off, lddkv=None, dkptr=None):
    n, l, e = k.v.shape
    return mh.lib().modcr_align_attn_bwd(mh._ptr(dout), mh._ptr(q), mh._ptr(k.v), mh._ptr(v.v), k.ld, mh._ptr(probs), mh._ptr(dq),
                                         dkptr or mh._ptr(dk.v), mh._ptr(dv.v), dk.ld if lddkv is None else lddkv, n, l, e, c.heads,
                                         float(scale), float(p), SEED, off, mh.dt_of(k.v), mh._stream())


def align_math(q, k, v, bias, scale, keepw, dout, heads, dt, probs=None):
    """the operation in `dt` (float64: the reference; float32: the yardstick) from the stored inputs; the backward from `probs`
    (the fp32 numbers the kernel is fed) when given.  keepw = keep * keep_scale"""
    n, l, e = k.shape
    d = e // heads
    q, k, v, keepw = q.to(dt), k.to(dt), v.to(dt), keepw.to(dt)
    qs = (q * scale).view(n, heads, d)
    kh, vh = k.view(n, l, heads, d), v.view(n, l, heads, d)
    s = torch.einsum("nhd,nlhd->nhl", qs, kh)
    if bias is not None:
        s = s + bias.to(dt)[:, None, :]
    p = torch.softmax(s, -1)
    r = {"out": torch.einsum("nhl,nlhd->nhd", p * keepw, vh).reshape(n, e), "probs": p}
    if dout is not None:
        pf = p if probs is None else probs.to(dt)
        doh = dout.to(dt).view(n, heads, d)
        r["dv"] = torch.einsum("nhl,nhd->nlhd", pf * keepw, doh).reshape(n, l, e)
        dp = torch.einsum("nhd,nlhd->nhl", doh, vh) * keepw
        ds = pf * (dp - (pf * dp).sum(-1, keepdim=True))
        r["dq"] = scale * torch.einsum("nhl,nlhd->nhd", ds, kh).reshape(n, e)
        r["dk"] = torch.einsum("nhl,nhd->nlhd", ds, qs).reshape(n, l, e)
    return r


def align_bias(kind, n, l):
    """additive key mask [n, l] fp32 on the CPU: ragged 0 / -10000 (sequence i keeps its first 1 + (7 i + 3) % l keys); "allmasked":
    sequence 0 all -10000 (the softmax of the scores alone); "inf": -inf on every third key (never key 0)"""
    if kind is None:
        return None
    b = torch.zeros(n, l)
    for i in range(n):
        b[i, 1 + (7 * i + 3) % l:] = -10000.0
    if kind == "allmasked":
        b[0] = -10000.0
    if kind == "inf":
        b = torch.zeros(n, l)
        b[:, 2::3] = float("-inf")
    return b


def align_setup(c, dist):
    d = c.e // c.heads
    scale = 1.0 if c.scale1 else float(np.float32(d ** -0.5))
    seed = c.e * 131 + c.l * 7 + c.heads + (1000003 if dist == "flat" else 0)
    amp = (3.0 if dist == "peaked" else 0.05) / (scale * d ** 0.5)             # scores of standard deviation 3 / 0.05
    td = TD[c.dt]
    q = framed(rand((c.n, c.e), seed, mul=amp))
    k = Rows(c.n, c.l, c.e, c.e + c.kpad, td, NAN, rand((c.n, c.l, c.e), seed + 1))
    v = k if c.alias else Rows(c.n, c.l, c.e, c.e + c.kpad, td, NAN, rand((c.n, c.l, c.e), seed + 2))
    dout = framed(rand((c.n, c.e), seed + 3))
    bias = align_bias(c.bias, c.n, c.l)
    off = drop_offset(c.off, c.heads, c.l)
    keep, keepw = keep_weights(c.p, off, c.n, c.heads, c.l)
    return scale, q, k, v, dout, bias, off, keep, keepw


def run_align(mh, tol, c, dist, chained=False):
    scale, q, k, v, dout, bias, off, keep, keepw = align_setup(c, dist)
    n, l, e, heads, td = c.n, c.l, c.e, c.heads, TD[c.dt]
    bias_d = framed(bias.cuda()) if bias is not None else None
    f_ok, b_ok = align_route(l, e, heads, 1) is not None, align_route(l, e, heads, 2) is not None
    out, probs = Guard(n, e, torch.float32), Guard(n * heads, l, torch.float32)
    rc = align_fwd(mh, q, k, v, out.v, None if c.noprobs else probs.v, c, scale, c.p, off, bias_d)
    if not f_ok:
        assert rc != 0 and "too long" in last_error(mh), (rc, last_error(mh))
        assert out.untouched() and probs.untouched()
    else:
        assert rc == 0, last_error(mh)
    if not b_ok:                                        # the backward has two tables in LDS: refused from a smaller L on (docstring)
        dq, dk, dv = Guard(n, e, torch.float32), Rows(n, l, e, e + c.dpad, td, SENTINEL), Rows(n, l, e, e + c.dpad, td, SENTINEL)
        pr = framed(torch.full((n * heads, l), 1.0 / l, device="cuda"))
        rc = align_bwd(mh, dout, q, k, v, pr, dq.v, dk, dv, c, scale, c.p, off)
        assert rc != 0 and "too long" in last_error(mh), (rc, last_error(mh))
        assert dq.untouched() and dk.untouched() and dv.untouched()
    if not f_ok:
        return
    qc, kc, vc, dc = q.cpu(), k.v.cpu(), v.v.cpu(), dout.cpu()
    ref = align_math(qc, kc, vc, bias, scale, keepw, dc if b_ok else None, heads, torch.float64)
    fed = ref["probs"].float()
    what = "%s %s" % (dist, "chained" if chained else "")
    assert out.intact() and (probs.untouched() if c.noprobs else probs.intact())
    if chained:
        fed = probs.v.view(n, heads, l).cpu().clone()
        ref = align_math(qc, kc, vc, bias, scale, keepw, dc, heads, torch.float64, probs=fed)
    plain = align_math(qc, kc, vc, bias, scale, keepw, dc if b_ok else None, heads, torch.float32, probs=fed)
    check(tol, "align out", what, out.v, ref["out"], plain["out"])
    if not c.noprobs:
        got_p = probs.v.view(n, heads, l)
        check(tol, "align probs", what, got_p, ref["probs"], plain["probs"])
        if c.bias == "inf":
            assert bool((got_p[:, :, 2::3] == 0).all()), "p must be exactly 0 under a -inf key bias"
    if not b_ok:
        return
    dq, dk, dv = Guard(n, e, torch.float32), Rows(n, l, e, e + c.dpad, td, SENTINEL), Rows(n, l, e, e + c.dpad, td, SENTINEL)
    rc = align_bwd(mh, dout, q, k, v, framed(fed.cuda().view(n * heads, l)), dq.v, dk, dv, c, scale, c.p, off)
    assert rc == 0, last_error(mh)
    assert dq.intact() and dk.frame_intact() and dv.frame_intact()
    check(tol, "align dq", what, dq.v, ref["dq"], plain["dq"])
    check(tol, "align dk", what, dk.v, ref["dk"], plain["dk"], c.dt)
    check(tol, "align dv", what, dv.v, ref["dv"], plain["dv"], c.dt)
    # mask agreement, exact: the dv piece of (key, head) is p' dout_h
    piece = (dv.v.reshape(n, l, heads, e // heads) != 0).any(-1).transpose(1, 2).cpu()       # [n, heads, l]
    live = keep & (fed > 0)
    assert torch.equal(piece, live), "%d (key, head) pieces of dv disagree with the host mask" % int((piece != live).sum())
    if c.bias == "inf":
        assert bool((dk.v[:, 2::3] == 0).all()) and bool((dv.v[:, 2::3] == 0).all()), "-inf keys must get exactly zero dk / dv rows"


@pytest.mark.parametrize("dist", DISTS)
@pytest.mark.parametrize("c", ALIGN_CASES, ids=align_id)
def test_align_attn_routes(mh, tol, c, dist):
    run_align(mh, tol, c, dist)


@pytest.mark.parametrize("dist", DISTS)
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_align_attn_chained_forward_backward(mh, tol, dt, dist):
    """the backward on the forward's own probabilities (blocked backward, unblocked forward, dropout, a ragged key bias)"""
    run_align(mh, tol, acase(768, 8, 341, n=3, dt=dt, kpad=8, bias="ragged", p=0.1, off="mod3"), dist, chained=True)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_align_attn_refuses_misaligned_rows(mh, dt):
    """a row stride or a pointer that is no multiple of 16 bytes: refused, nothing written"""
    c = acase(768, 8, 9, n=2, dt=dt)
    scale, q, k, v, dout, _, off, _, _ = align_setup(c, "peaked")
    n, l, e, td = c.n, c.l, c.e, TD[dt]
    step = 16 // k.v.element_size()
    out, probs = Guard(n, e, torch.float32), Guard(n * c.heads, l, torch.float32)
    big = Rows(n, l, e, e + step, td, NAN, k.v)                       # room for the one-element shift and the odd stride
    shifted = ctypes.c_void_p(big.v.data_ptr() + big.v.element_size())
    for kw in (dict(ldkv=big.ld - 1), dict(kptr=shifted)):
        assert align_fwd(mh, q, big, big, out.v, probs.v, c, scale, 0.0, off, None, **kw) != 0
        assert "16-byte aligned" in last_error(mh)
        assert out.untouched() and probs.untouched()
    pr = torch.full((n * c.heads, l), 1.0 / l, device="cuda")
    dq, dk, dv = Guard(n, e, torch.float32), Rows(n, l, e, e + step, td, SENTINEL), Rows(n, l, e, e + step, td, SENTINEL)
    for kw in (dict(lddkv=dk.ld - 1), dict(dkptr=ctypes.c_void_p(dk.v.data_ptr() + dk.v.element_size()))):
        assert align_bwd(mh, dout, q, k, v, pr, dq.v, dk, dv, c, scale, 0.0, off, **kw) != 0
        assert "16-byte aligned" in last_error(mh)
        assert dq.untouched() and dk.untouched() and dv.untouched()


# ---- cls_xattn ------------------------------------------------------------------------------------------------------------------
class XBlocks(object):
    """1-3 bf16 row blocks [n, rows_i, e] of one row stride ld, each in a buffer of its own with a NaN guard row before it, i + 1 NaN
    guard rows after it (so the sequence strides differ) and NaN padding columns; block `stride0` is stored once and shared by
    every sequence (seq_stride 0)"""

    def __init__(self, c, seed):
        ld = c.e + c.ldpad
        self.bufs, self.views, ptrs, strides = [], [], [], []
        for i, r in enumerate(c.rows):
            ns = 1 if c.stride0 == i else c.n
            buf = torch.full((ns, r + 2 + i, ld), NAN, dtype=torch.bfloat16, device="cuda")
            buf[:, 1:1 + r, :c.e] = rand((ns, r, c.e), seed + i)
            self.bufs.append(buf)
            self.views.append(buf[:, 1:1 + r, :c.e].expand(c.n, r, c.e))
            ptrs.append(buf[:, 1:].data_ptr())
            strides.append(0 if c.stride0 == i else buf.stride(0))
        k = len(c.rows)
        self.k, self.ld = k, ld
        self.ptrs, self.strides = (ctypes.c_void_p * k)(*ptrs), (ctypes.c_int64 * k)(*strides)
        self.rows = (ctypes.c_int32 * k)(*c.rows)
        self.x = torch.cat(self.views, 1)                # [n, L, e] bf16


def cls_fwd(mh, qt, xb, ctx, ssum, probs, n, e, p, off, heads=8, ptrs=None):
    return mh.lib().modcr_cls_xattn_fwd(mh._ptr(qt), ptrs or xb.ptrs, xb.strides, xb.rows, xb.k, xb.ld, mh._ptr(ctx), mh._ptr(ssum),
                                        mh._ptr(probs), n, e, heads, float(p), SEED, off, mh._stream())


def cls_bwd(mh, dctx, dssum, ctx, ssum, probs, xb, dqt, n, e, p, off, heads=8, ptrs=None):
    return mh.lib().modcr_cls_xattn_bwd(mh._ptr(dctx), mh._ptr(dssum), mh._ptr(ctx), mh._ptr(ssum), mh._ptr(probs), ptrs or xb.ptrs,
                                        xb.strides, xb.rows, xb.k, xb.ld, mh._ptr(dqt), n, e, heads, float(p), SEED, off, mh._stream())


def cls_math(qt, x, keepw, dctx, dssum, dt, fed=None):
    """csrc/clsattn.hip's formulas in `dt`; the backward from `fed` = (ctx, ssum, probs) as the kernel is fed them (fp32)"""
    qt, x, keepw = qt.to(dt), x.to(dt), keepw.to(dt)
    p = torch.softmax(torch.einsum("nhe,nje->nhj", qt, x), -1)
    pm = p * keepw
    r = {"probs": p, "ctx": torch.einsum("nhj,nje->nhe", pm, x), "ssum": pm.sum(-1)}
    if dctx is not None:
        ctx, ssum, pf = (t.to(dt) for t in fed) if fed is not None else (r["ctx"], r["ssum"], p)
        dctx, dssum = dctx.to(dt), dssum.to(dt)
        dp = torch.einsum("nhe,nje->nhj", dctx, x) + dssum[:, :, None]
        delta = (dctx * ctx).sum(-1) + dssum * ssum
        r["dqt"] = torch.einsum("nhj,nje->nhe", pf * keepw * dp - pf * delta[:, :, None], x)
    return r


def run_cls(mh, tol, c, dist, chained=False):
    n, e, l = c.n, c.e, sum(c.rows)
    seed = e * 17 + l * 5 + (1000003 if dist == "flat" else 0)
    _, f_ok, b_ok = cls_route(e, l)
    xb = XBlocks(c, seed)
    qt = framed(rand((n, 8, e), seed + 10, mul=(2.0 if dist == "peaked" else 0.05) / e ** 0.5))
    dctx, dssum = framed(rand((n, 8, e), seed + 11)), framed(rand((n, 8), seed + 12))
    off = drop_offset(c.off, 8, l)
    _, keepw = keep_weights(c.p, off, n, 8, l)
    ctx, ssum, probs = Guard(n * 8, e, torch.float32), Guard(1, n * 8, torch.float32), Guard(n * 8, l, torch.float32)
    rc = cls_fwd(mh, qt, xb, ctx.v, ssum.v, probs.v, n, e, c.p, off)
    if not f_ok:
        assert rc != 0 and "too long" in last_error(mh), (rc, last_error(mh))
        assert ctx.untouched() and ssum.untouched() and probs.untouched()
    else:
        assert rc == 0, last_error(mh)
    if not b_ok:                                        # two [L][8] tables in LDS: refused from a smaller L on (docstring)
        dqt = Guard(n * 8, e, torch.float32)
        z = torch.zeros(n * 8 * max(l, e), device="cuda")
        rc = cls_bwd(mh, dctx, dssum, z, z, z, xb, dqt.v, n, e, c.p, off)
        assert rc != 0 and "too long" in last_error(mh), (rc, last_error(mh))
        assert dqt.untouched()
    if not f_ok:
        return
    qc, xc, dcc, dsc = qt.cpu(), xb.x.cpu(), dctx.cpu(), dssum.cpu()
    ref = cls_math(qc, xc, keepw, dcc if b_ok else None, dsc, torch.float64)
    fed = tuple(ref[key].float() for key in ("ctx", "ssum", "probs"))
    what = "%s %s" % (dist, "chained" if chained else "")
    assert ctx.intact() and ssum.intact() and probs.intact()
    if chained:
        fed = (ctx.v.view(n, 8, e).cpu().clone(), ssum.v.view(n, 8).cpu().clone(), probs.v.view(n, 8, l).cpu().clone())
        ref = cls_math(qc, xc, keepw, dcc, dsc, torch.float64, fed=fed)
    plain = cls_math(qc, xc, keepw, dcc if b_ok else None, dsc, torch.float32, fed=fed)
    check(tol, "cls probs", what, probs.v.view(n, 8, l), ref["probs"], plain["probs"])
    check(tol, "cls ssum", what, ssum.v.view(n, 8), ref["ssum"], plain["ssum"])
    check(tol, "cls ctx", what, ctx.v.view(n, 8, e), ref["ctx"], plain["ctx"])
    if not b_ok:
        return
    dqt = Guard(n * 8, e, torch.float32)
    rc = cls_bwd(mh, dctx, dssum, framed(fed[0].cuda()), framed(fed[1].cuda()), framed(fed[2].cuda()), xb, dqt.v, n, e, c.p, off)
    assert rc == 0, last_error(mh)
    assert dqt.intact()
    check(tol, "cls dqt", what, dqt.v.view(n, 8, e), ref["dqt"], plain["dqt"])


@pytest.mark.parametrize("dist", DISTS)
@pytest.mark.parametrize("c", CLS_CASES, ids=cls_id)
def test_cls_xattn_routes(mh, tol, c, dist):
    """Current contract: the forward accepts key counts (E = 768: 2176 < L <= 4352) that the backward then refuses."""
    run_cls(mh, tol, c, dist)


@pytest.mark.parametrize("dist", DISTS)
def test_cls_xattn_chained_forward_backward(mh, tol, dist):
    run_cls(mh, tol, ClsCase(768, (79, 1, 120), 3, 4, 0.1, "mod3", 1), dist, chained=True)


def test_cls_xattn_refusals_write_nothing(mh):
    """heads != 8, E > 1024, E % 4 != 0, a row block that is only 4-byte aligned"""
    for e, heads, shift, msg in ((768, 4, 0, "8 heads"), (1028, 8, 0, "E <= 1024"), (130, 8, 0, "E % 4 == 0"), (768, 8, 2, "8-byte aligned")):
        c = ClsCase(e, (5, 3), 2, 4, 0.0, "0", None)
        n, l = c.n, 8
        xb = XBlocks(c, 5)
        ptrs = (ctypes.c_void_p * 2)(xb.bufs[0][:, 1:].data_ptr(), xb.bufs[1][:, 1:].data_ptr() + 2 * shift)
        qt, dctx, dssum = rand((n, heads, e), 1), rand((n, heads, e), 2), rand((n, heads), 3)
        ctx, ssum, probs = Guard(n * heads, e, torch.float32), Guard(1, n * heads, torch.float32), Guard(n * heads, l, torch.float32)
        assert cls_fwd(mh, qt, xb, ctx.v, ssum.v, probs.v, n, e, 0.0, 0, heads=heads, ptrs=ptrs) != 0
        assert msg in last_error(mh), last_error(mh)
        assert ctx.untouched() and ssum.untouched() and probs.untouched()
        dqt = Guard(n * heads, e, torch.float32)
        z = torch.zeros(n * heads * e, device="cuda")
        assert cls_bwd(mh, dctx, dssum, z, z, z, xb, dqt.v, n, e, 0.0, 0, heads=heads, ptrs=ptrs) != 0
        assert msg in last_error(mh), last_error(mh)
        assert dqt.untouched()


# ---- the autograd wrappers --------------------------------------------------------------------------------------------------------
def take_offset(mh):
    """the (seed, offset) the next DROPOUT.take will hand out"""
    return mh.DROPOUT.seed, (mh.DROPOUT.offset + 3) & ~3


@pytest.mark.parametrize("dt,p", [("f32", 0.0), ("f32", 0.1), ("bf16", 0.1)])
def test_align_attn_fn_aliased_k_v(mh, tol, dt, p):
    """AlignAttnFn as ClsLayer2 calls it: k is v, so autograd adds dk and dv; no gradient for key_bias, heads, scale, p.  The bf16 sum
    of two bf16 gradients is rounded three times (dk, dv, their sum): half an ulp at |dk| and at |dv| is allowed on top of the half
    ulp at the sum, which no implementation that forms dk and dv in bf16 can do without."""
    from modeling import hip_autograd as ag
    n, l, e = 3, 57, 768
    td = TD[dt]
    mh.DROPOUT.manual_seed(4242)
    mh.DROPOUT.take(4099)                                # a running offset, as in a step
    seed, off = take_offset(mh)
    q = rand((n, e), 31, mul=3.0 / e ** 0.5).requires_grad_(True)
    k = rand((n, l, e), 32, td).requires_grad_(True)
    bias = align_bias("ragged", n, l).cuda().requires_grad_(True)
    dout = rand((n, e), 33)
    out = ag.AlignAttnFn.apply(q, k, k, 1, 1.0, p, bias)
    out.backward(dout)
    assert bias.grad is None
    keep = torch.from_numpy(H.hidden_drop_keep(seed, off, n * l, p).reshape(n, 1, l)) if p else torch.ones(n, 1, l, dtype=torch.bool)
    keepw = keep.double() * (scale32(p) if p else 1.0)
    kc = k.detach().cpu()
    ref = align_math(q.detach().cpu(), kc, kc, bias.detach().cpu(), 1.0, keepw, dout.cpu(), 1, torch.float64)
    plain = align_math(q.detach().cpu(), kc, kc, bias.detach().cpu(), 1.0, keepw, dout.cpu(), 1, torch.float32)
    check(tol, "align out", "AlignAttnFn", out.detach(), ref["out"], plain["out"])
    check(tol, "align dq", "AlignAttnFn", q.grad, ref["dq"], plain["dq"])
    inner = 0.5 * (ulp(ref["dk"], td) + ulp(ref["dv"], td)) if dt == "bf16" else None
    check(tol, "align dk", "AlignAttnFn dk + dv", k.grad, ref["dk"] + ref["dv"], plain["dk"] + plain["dv"], dt, extra=inner)


@pytest.mark.parametrize("p", [0.0, 0.1])
def test_cls_xattn_fn(mh, tol, p):
    """ClsXAttnFn: d qt against float64, the gradient of k_bias exactly zero"""
    from modeling import hip_autograd as ag
    c = ClsCase(768, (79, 50), 3, 0, p, "0", None)
    n, e, l = c.n, c.e, sum(c.rows)
    mh.DROPOUT.manual_seed(777)
    mh.DROPOUT.take(1021)
    seed, off = take_offset(mh)
    xb = XBlocks(c, 41)
    qt = rand((n, 8, e), 42, mul=2.0 / e ** 0.5).requires_grad_(True)
    k_bias = rand((e,), 43).requires_grad_(True)
    dctx, dssum = rand((n, 8, e), 44), rand((n, 8), 45)
    ctx, ssum = ag.ClsXAttnFn.apply(qt, k_bias, 8, p, *xb.views)
    torch.autograd.backward([ctx, ssum], [dctx, dssum])
    assert k_bias.grad is not None and bool((k_bias.grad == 0).all())
    keep = torch.from_numpy(H.hidden_drop_keep(seed, off, n * 8 * l, p).reshape(n, 8, l)) if p else torch.ones(n, 8, l, dtype=torch.bool)
    keepw = keep.double() * (scale32(p) if p else 1.0)
    fed = None                                           # the wrapper feeds the backward the forward's own outputs
    ref = cls_math(qt.detach().cpu(), xb.x.cpu(), keepw, dctx.cpu(), dssum.cpu(), torch.float64, fed=fed)
    plain = cls_math(qt.detach().cpu(), xb.x.cpu(), keepw, dctx.cpu(), dssum.cpu(), torch.float32, fed=fed)
    check(tol, "cls ctx", "ClsXAttnFn", ctx.detach(), ref["ctx"], plain["ctx"])
    check(tol, "cls ssum", "ClsXAttnFn", ssum.detach(), ref["ssum"], plain["ssum"])
    check(tol, "cls dqt", "ClsXAttnFn", qt.grad, ref["dqt"], plain["dqt"])
