"""CPU-side checks of the attention forward's host half (csrc/attn.hip: attn_fwd_setup, attn_fwd_route): the route
modcr_qkv_attn_route reports against a hand-written table, modcr_hip.side_outputs_on_tiles against the expression it replaced,
the refusals of every public forward entry (validation returns before any launch, so no GPU is needed), and the symbols.

The "rule" column of the table cites the dispatcher this one replaced -- csrc/attn.hip at commit f4e36b1, by line -- or the
document that states the rule."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    import modcr_hip
    return modcr_hip


def tile(nw, hpw, occ, bka, nslot):
    return ("tile", (nw, hpw, occ, bka, nslot), 0)


def tile4(mode, lp, nh, concat=0):
    return ("tile4", (mode, lp, nh, 0, 0), concat)


def core(family, mode=0):
    return (family, (mode, 0, 0, 0, 0), 0)


POST = 1        # MODCR_ATTN_SIDE_POST_DROPOUT
H4, H3, H2 = dict(h=256, a=4), dict(h=192, a=3), dict(h=128, a=2)
# (arguments of modcr_hip.qkv_attn_route beyond n = 2 and p = 0, expected route or (rc, message fragment), rule)
ROUTES = [
    # ---- key counts: both sides of 64 | 65, 128 | 129, 192 | 193, 256 | 257, 512 | 513
    (dict(s=64, **H4), tile(2, 2, 2, 64, 2), "f4e36b1:2435 L <= 64: the older kernel, a head pair per workgroup"),
    (dict(s=65, **H4), tile4(1, 128, 2), "f4e36b1:2436-2442 64 < L <= 128: the 128-token tile, key mask = MODE 1"),
    (dict(s=128, dense=True, **H4), tile4(2, 128, 2), "f4e36b1:2442 dense mask = MODE 2"),
    (dict(s=129, **H4), tile4(1, 192, 2), "f4e36b1:2456-2459 128 < L <= 192: the 192-token tile"),
    (dict(s=192, dense=True, **H4), tile4(2, 192, 2), "f4e36b1:2459"),
    (dict(s=193, **H4), tile4(1, 256, 1), "f4e36b1:2478-2480 192 < L <= 256: the 256-token tile, one head per workgroup"),
    (dict(s=256, dense=True, **H4), tile4(2, 256, 1), "f4e36b1:2480"),
    (dict(s=257, **H4), core("long_bf16"), "f4e36b1:2368 P + S > 256: the streaming core (INTEGRATION.md, 256 < P+S <= 512)"),
    (dict(s=512, **H4), core("long_bf16"), "f4e36b1:2271 the 512-key limit is inclusive"),
    (dict(s=513, **H4), (-3, "512-key limit"), "f4e36b1:2271-2274"),
    # ---- head count odd (H = 192, A = 3) and H below 256 (H = 128, A = 2): the older kernel at every tile
    (dict(s=64, **H3), tile(2, 1, 2, 64, 2), "f4e36b1:2435 odd head count: one head per workgroup"),
    (dict(s=65, **H3), tile(4, 1, 2, 64, 2), "f4e36b1:2436 needs A even; 2452"),
    (dict(s=100, **H2), tile(4, 2, 2, 64, 2), "f4e36b1:2436 needs H >= 256; 2452 head pair"),
    (dict(s=150, **H3), tile(6, 1, 2, 64, 2), "f4e36b1:2456 needs a head pair; 2468"),
    (dict(s=150, **H2), tile(6, 2, 3, 32, 4), "f4e36b1:2456 needs H >= 256; 2473"),
    (dict(s=193, **H3), tile(8, 1, 2, 64, 2), "f4e36b1:2478 needs H % 128 == 0; 2490"),
    (dict(s=230, **H2), tile(8, 1, 2, 64, 2), "f4e36b1:2478 needs H >= 256; 2490"),
    # ---- side outputs and row statistics
    (dict(s=100, probs=True, **H4), tile4(0, 128, 2), "f4e36b1:2441 a probabilities output: the generic variant, MODE 0"),
    (dict(s=100, align_t=40, **H4), tile4(0, 128, 2), "f4e36b1:2441 an align map alone: MODE 0"),
    (dict(s=100, chunk_t=40, align_t=40, dense=True, **H4), tile4(3, 128, 2), "f4e36b1:2440 the phase-3 call on the 128-token tile: MODE 3"),
    (dict(s=100, chunk_t=40, align_t=40, dense=True, probs=True, **H4), tile4(0, 128, 2), "f4e36b1:2440-2441 MODE 3 needs probs = NULL"),
    (dict(s=150, chunk_t=40, **H4), tile4(0, 192, 2), "f4e36b1:2458 chunk-mean queries alone: MODE 0"),
    (dict(s=150, chunk_t=40, align_t=40, dense=True, **H4), tile4(3, 192, 2), "f4e36b1:2457 the phase-3 call: MODE 3"),
    (dict(s=150, chunk_t=40, align_t=40, dense=True, probs=True, **H4), tile4(0, 192, 2), "f4e36b1:2457 MODE 3 needs probs = NULL"),
    (dict(s=230, probs=True, **H4), tile4(0, 256, 1), "f4e36b1:2487-2488 the generic variant of the 256-token tile"),
    (dict(s=230, chunk_t=40, **H4), tile4(0, 256, 1), "f4e36b1:2487-2488"),
    (dict(s=100, lse=True, **H4), tile4(1, 128, 2), "f4e36b1:2226 row statistics: written by the tile kernels"),
    (dict(s=150, lse=True, dump=True, **H4), tile4(1, 192, 2), "f4e36b1:2372 the dump comes with lse, 64 < S <= 192 (DUMPV: launcher)"),
    (dict(s=64, lse=True, **H4), (-3, "no row statistics"), "f4e36b1:2434 MODCR_NO_LSE_HERE at L <= 64"),
    (dict(s=100, lse=True, **H3), (-3, "no row statistics"), "f4e36b1:2446 MODCR_NO_LSE_HERE on the older kernel"),
    (dict(s=300, lse=True, **H4), (-3, "not produced above 256 keys"), "f4e36b1:2279-2282"),
    (dict(s=230, lse=True, dump=True, **H4), (-1, "64 < S <= 192"), "f4e36b1:2372-2373"),
    # ---- the MODE-3 align tile of the 256-token tile: align_t (S - align_t) 4 <= 64 A4T<256,1>::VT_STRIDE = 64 x 520 bytes
    (dict(s=230, chunk_t=44, align_t=44, dense=True, **H4), tile4(3, 256, 1), "f4e36b1:2481-2483 44 x 186 x 4 = 32736 <= 33280"),
    (dict(s=230, chunk_t=45, align_t=45, dense=True, **H4), tile4(0, 256, 1), "f4e36b1:2481-2488 45 x 185 x 4 = 33300 > 33280"),
    # ---- prefix rows: the tile kernels over a concatenated copy in the workspace, when it is there
    (dict(s=92, p=8, **H4), tile4(1, 128, 2, 1), "f4e36b1:2419-2429 prefix_tiles (the binding's workspace suffices)"),
    (dict(s=92, p=8, workspace_bytes=0, **H4), tile(4, 2, 2, 64, 2), "f4e36b1:2420 no workspace: the older kernel"),
    (dict(s=92, p=8, workspace_aligned=False, **H4), tile(4, 2, 2, 64, 2), "f4e36b1:2420 modcr_aligned16(workspace)"),
    (dict(s=92, p=8, probs=True, **H4), tile(4, 2, 2, 64, 2), "f4e36b1:2419 prefix_tiles needs no side outputs"),
    (dict(s=56, p=8, **H4), tile(2, 2, 2, 64, 2), "f4e36b1:2419 prefix_tiles needs L > 64"),
    (dict(s=172, p=8, dense=True, **H4), tile4(2, 192, 2, 1), "f4e36b1:2456 (P == 0 || prefix_tiles)"),
    (dict(s=222, p=8, **H4), tile4(1, 256, 1, 1), "f4e36b1:2478-2480"),
    (dict(s=222, p=8, chunk_t=40, **H4), tile(8, 1, 2, 64, 2), "f4e36b1:2487 the generic variant needs P == 0; 2490"),
    (dict(s=222, p=8, **H3), tile(8, 1, 2, 64, 2), "f4e36b1:2419 prefix_tiles needs H % 128 == 0"),
    (dict(s=292, p=8, **H4), core("long_bf16"), "f4e36b1:2368 P + S > 256"),
    # ---- attention-probability dropout and MODCR_ATTN_SIDE_POST_DROPOUT
    (dict(s=100, attn_p=0.1, **H4), tile4(1, 128, 2), "f4e36b1:2440-2442 the route does not depend on p (DROP: launcher)"),
    (dict(s=100, attn_p=0.1, probs=True, **H4), (-3, "needs MODCR_ATTN_SIDE_POST_DROPOUT"), "f4e36b1:2397-2400"),
    (dict(s=100, attn_p=0.1, probs=True, flags=POST, **H4), tile4(0, 128, 2), "f4e36b1:2441"),
    (dict(s=64, attn_p=0.1, probs=True, flags=POST, **H4), (-3, "post-dropout side outputs"), "f4e36b1:2433-2434"),
    (dict(s=100, attn_p=0.1, align_t=40, flags=POST, **H3), (-3, "post-dropout side outputs"), "f4e36b1:2433, 2446"),
    (dict(s=100, attn_p=0.1, align_t=40, **H3), tile(4, 1, 2, 64, 2), "f4e36b1:2433 without the flag the map is un-dropped: served"),
    (dict(s=64, probs=True, flags=POST, **H4), tile(2, 2, 2, 64, 2), "f4e36b1:2393 the flag is irrelevant at p = 0"),
    (dict(s=300, attn_p=0.1, **H4), (-3, "not implemented above 256 keys"), "f4e36b1:2275-2278"),
    # ---- fp32
    (dict(s=100, dtype=1, **H4), core("f32"), "f4e36b1:2492-2536 the exact core at P + S <= 256"),
    (dict(s=92, p=8, dtype=1, probs=True, attn_p=0.1, flags=POST, **H3), core("f32"), "f4e36b1:2494 any shape, prefix rows, post-dropout"),
    (dict(s=300, dtype=1, **H4), core("long_f32"), "f4e36b1:2368; attn_long.hip:488"),
    (dict(s=100, dtype=1, lse=True, **H4), (-1, "bf16 path only"), "f4e36b1:2492"),
    (dict(s=100, dtype=1, probs=True, attn_p=0.1, **H4), (-1, "needs MODCR_ATTN_SIDE_POST_DROPOUT"), "f4e36b1:2494-2495"),
    (dict(s=100, dtype=1, workspace_bytes=64, **H4), (-1, "workspace"), "f4e36b1:2496-2498"),
    (dict(s=300, workspace_bytes=64, **H4), (-1, "workspace"), "f4e36b1:2291-2293"),
    # ---- modcr_qkv_attn_bias_fwd: the streaming core at every key count, mode 1, or 2 with dropout
    (dict(s=100, bias=True, **H4), core("long_bf16", 1), "f4e36b1:2346-2356; attn_long.hip:476"),
    (dict(s=100, bias=True, attn_p=0.1, **H3), core("long_bf16", 2), "attn_long.hip:476 drop_thr16 != 0"),
    (dict(s=292, p=8, bias=True, probs=True, **H4), core("long_bf16", 1), "f4e36b1:2323 up to 512 keys"),
    (dict(s=100, bias=True, dtype=1, attn_p=0.1, **H2), core("long_f32", 2), "attn_long.hip:490"),
    (dict(s=300, bias=True, attn_p=0.1, **H4), (-3, "not implemented above 256 keys"), "f4e36b1:2329-2332"),
    (dict(s=100, bias=True, workspace_bytes=64, **H4), (-1, "workspace"), "f4e36b1:2339-2341"),
]


class Case:
    """GPU side (tests/test_hip_kernels.py, tools/attn_route_trace.py): the tensors of one row of ROUTES at N = 2, and the call"""

    def __init__(self, mh, kw, seed):
        import torch
        self.kw = kw = dict(kw)
        g = torch.Generator(device="cpu").manual_seed(seed)
        n, s, p, h, a = 2, kw["s"], kw.get("p", 0), kw["h"], kw["a"]
        l = p + s
        self.dims = (n, s, p, h, a)
        self.dt = kw.get("dtype", mh.BF16)
        td = mh.torch_dtype(self.dt)

        def rnd(*shape, scale=1.0):
            return (torch.randn(*shape, generator=g) * scale).cuda()
        self.x = rnd(n, s, h).to(td)
        self.hist = rnd(n, p, h).to(td) if p else None
        self.w = rnd(3 * h, h, scale=0.05).to(td)
        self.b = rnd(3 * h, scale=0.1)
        km = torch.ones(n, l)
        km[1, l - 5:] = 0
        self.km = km.cuda()
        self.bits = None
        if kw.get("dense"):
            dense = (torch.rand(n, s, l, generator=g) < 0.7).float()
            dense[:, torch.arange(s), p + torch.arange(s)] = 1
            self.bits = mh.pack_mask_bits(dense.cuda())
        self.bias = (rnd(n, 1, 1, l) - 10000.0 * (1 - self.km.view(n, 1, 1, l))) if kw.get("bias") else None
        ct = kw.get("chunk_t", 0)
        self.chunk = None
        if ct:
            cid = (torch.arange(ct) // 3).to(torch.int32).repeat(n, 1)
            cid[:, 0] = -1
            self.chunk = cid.cuda()
        self.ws_bytes = kw.get("workspace_bytes")
        if self.ws_bytes is None:
            self.ws_bytes = (mh.lib().modcr_qkv_attn_bias_workspace if kw.get("bias") else mh.lib().modcr_qkv_attn_workspace)(n, s, p, h, self.dt)
        self.ws = torch.zeros(max(self.ws_bytes, 0) + 32, dtype=torch.uint8, device="cuda") if self.ws_bytes else None

    def outputs(self):
        import torch
        n, s, p, h, a = self.dims
        kw, at = self.kw, self.kw.get("align_t", 0)
        return {"ctx": torch.zeros_like(self.x),
                "probs": torch.zeros(n, a, s, p + s, device="cuda") if kw.get("probs") else None,
                "align_map": torch.zeros(n, at, s - at, device="cuda") if at else None,
                "lse": torch.zeros(n, a, s, device="cuda") if kw.get("lse") else None,
                "dump": torch.zeros(max(self.dump_bytes, 2) // 2, dtype=torch.bfloat16, device="cuda") if kw.get("dump") else None}

    def call(self, lib, mh):
        """(rc, message, outputs) of modcr_qkv_attn_opt_fwd / modcr_qkv_attn_bias_fwd in `lib`"""
        import torch
        n, s, p, h, a = self.dims
        kw = self.kw
        self.dump_bytes = mh.lib().modcr_qkv_attn_dump_bytes(n, s, a)
        o = self.outputs()
        ptr = mh._ptr
        ws = None
        if self.ws is not None:
            base = (self.ws.data_ptr() + 15) & ~15
            ws = ctypes.c_void_p(base if kw.get("workspace_aligned", True) else base + 4)
        drop = (float(kw.get("attn_p", 0.0)), 1234, 77, kw.get("flags", 0))
        tail = (ptr(self.chunk), kw.get("chunk_t", 0), ptr(o["ctx"]), ptr(o["probs"]), ptr(o["align_map"]), kw.get("align_t", 0))
        if kw.get("bias"):
            fn = lib.modcr_qkv_attn_bias_fwd
            fn.restype, fn.argtypes = mh.SIGNATURES["modcr_qkv_attn_bias_fwd"]
            rc = fn(ptr(self.x), ptr(self.hist), ptr(self.w), ptr(self.b), ptr(self.bias), p + s, 0, 0, None, 0, *tail, n, s, p, h, a, *drop,
                    ws, self.ws_bytes, self.dt, mh._stream())
        else:
            fn = lib.modcr_qkv_attn_opt_fwd
            fn.restype, fn.argtypes = mh.SIGNATURES["modcr_qkv_attn_opt_fwd"]
            rc = fn(ptr(self.x), ptr(self.hist), ptr(self.w), ptr(self.b), None if self.bits is not None else ptr(self.km), ptr(self.bits),
                    *tail, ptr(o["lse"]), ptr(o["dump"]), n, s, p, h, a, *drop, ws, self.ws_bytes, self.dt, mh._stream())
        torch.cuda.synchronize()
        lib.modcr_last_error.restype = ctypes.c_char_p
        return rc, lib.modcr_last_error().decode() if rc else "", o


def route_of_call(mh, kw):
    return mh.qkv_attn_route(2, kw["s"], kw.get("p", 0), kw["h"], kw["a"], **{k: v for k, v in kw.items() if k not in ("s", "p", "h", "a")})


def route_of(mh, kw):
    r = route_of_call(mh, kw)
    return (r.family, r.inst, r.concat) if r.rc == 0 else (r.rc, r.message)


@pytest.mark.parametrize("lib_name", ["product", "tuning"])
def test_route_table(built, lib_name, monkeypatch):
    """every row in both libraries (no knob set: the tuning build takes the defaults)"""
    for name in ("MODCR_ATTN_HPW1", "MODCR_ATTN_RING32", "MODCR_ATTN_RING64", "MODCR_ATTN_NO_V4", "MODCR_ATTN_NO_V4S", "MODCR_ATTN_NO_V4L",
                 "MODCR_ATTN_NO_PREFIX_TILES"):
        monkeypatch.delenv(name, raising=False)
    built.use_tuning_library(lib_name == "tuning")
    try:
        for kw, want, rule in ROUTES:
            got = route_of(built, kw)
            if isinstance(want[0], int):
                prefix = "qkv_attn_bias_fwd" if kw.get("bias") else "qkv_attn_fwd"
                assert got[0] == want[0] and want[1] in got[1] and got[1].startswith(prefix), (kw, got, rule)
            else:
                assert got == want, (kw, got, rule)
    finally:
        built.use_tuning_library(False)


def test_tuning_knobs_are_read_by_the_route(built, monkeypatch):
    """the tuning library reports what it will launch under its knobs (f4e36b1:2412-2490); the product library ignores them"""
    cases = [
        ("MODCR_ATTN_HPW1", "1", dict(s=100, **H4), tile(4, 1, 2, 64, 2)),
        ("MODCR_ATTN_HPW1", "2", dict(s=150, **H4), tile(6, 1, 3, 32, 3)),
        ("MODCR_ATTN_HPW1", "3", dict(s=150, **H4), tile(6, 1, 3, 32, 2)),
        ("MODCR_ATTN_RING32", "1", dict(s=100, **H2), tile(4, 2, 2, 32, 4)),
        ("MODCR_ATTN_RING32", "2", dict(s=100, **H2), tile(4, 2, 2, 32, 3)),
        ("MODCR_ATTN_RING64", "1", dict(s=150, **H2), tile(6, 2, 3, 64, 2)),
        ("MODCR_ATTN_NO_V4", "1", dict(s=150, **H4), tile(6, 2, 3, 32, 4)),
        ("MODCR_ATTN_NO_V4S", "1", dict(s=100, **H4), tile(4, 2, 2, 64, 2)),
        ("MODCR_ATTN_NO_V4L", "1", dict(s=230, **H4), tile(8, 1, 2, 64, 2)),
        ("MODCR_ATTN_NO_V4L", "1", dict(s=222, p=8, **H4), tile(8, 1, 2, 64, 2)),       # and no concatenated copy for it
        ("MODCR_ATTN_NO_PREFIX_TILES", "1", dict(s=92, p=8, **H4), tile(4, 2, 2, 64, 2)),
    ]
    for name, value, kw, want in cases:
        monkeypatch.setenv(name, value)
        product = route_of(built, kw)
        built.use_tuning_library(True)
        try:
            got = route_of(built, kw)
        finally:
            built.use_tuning_library(False)
            monkeypatch.delenv(name)
        assert got == want, (name, value, kw, got)
        assert product == route_of(built, kw) != want, (name, kw, product)


def test_side_outputs_on_tiles_is_the_expression_it_replaced(built):
    for s in range(1, 257):
        for p in (0, 8):
            for h, a in ((128, 2), (192, 3), (256, 4), (384, 6), (1024, 16)):
                want = p == 0 and 64 < s <= 256 and h % 128 == 0 and 256 <= h <= 8192 and (a % 2 == 0 or s > 192)
                assert built.side_outputs_on_tiles(s, p, h, a) == want, (s, p, h, a)


# ---- refusals through the public entries -------------------------------------------------------------------------------------------
ENTRIES = ("modcr_qkv_attn_fwd", "modcr_qkv_attn_dropout_fwd", "modcr_qkv_attn_lse_fwd", "modcr_qkv_attn_opt_fwd", "modcr_qkv_attn_bias_fwd")


def call(lib, entry, ptr, n=1, s=100, p=0, h=256, a=4, dtype=0, attn_p=0.0, flags=0, x=True, hist=None, key_mask=True, dense=False,
         chunk=False, chunk_t=0, probs=False, align=False, align_t=0, lse=False, dump=False, ws=True, ws_bytes=1 << 40, sn=0, bias_ptr=None):
    """`entry` with `ptr` in every pointer argument the case sets, or None when the entry has no argument the case needs.  Every
    case fails validation, so nothing is read or launched."""
    q = ctypes.c_void_p(ptr)

    def given(on):
        return q if on else None
    short = entry[len("modcr_qkv_attn_"):-len("_fwd")] or "plain"
    if (attn_p and short == "plain") or ((lse or dump) and short not in ("lse", "opt")) or (flags and short not in ("opt", "bias")):
        return None
    if short == "bias" and (dense or not key_mask or lse or dump):
        return None
    if short != "bias" and (sn or bias_ptr is not None):
        return None
    head = [given(x), given(p > 0 if hist is None else hist), q, q]
    tail = [given(chunk), chunk_t, q, given(probs), given(align), align_t]
    shape = [n, s, p, h, a]
    end = [given(ws), ws_bytes, dtype, None]
    drop = [attn_p, 1, 2]
    fn = getattr(lib, entry)
    if short == "bias":
        return fn(*head, q if bias_ptr is None else ctypes.c_void_p(bias_ptr), sn, 0, 0, None, 0, *tail, *shape, *drop, flags, *end)
    head += [given(key_mask), given(dense)]
    if short == "plain":
        return fn(*head, *tail, *shape, *end)
    if short == "dropout":
        return fn(*head, *tail, *shape, *drop, *end)
    if short == "lse":
        return fn(*head, *tail, given(lse), given(dump), *shape, *drop, *end)
    return fn(*head, *tail, given(lse), given(dump), *shape, *drop, flags, *end)


# (arguments, return code, message fragment): one violated condition each.  Where the three validators of f4e36b1 (lines 2367-2381
# and 2492-2498, 2270-2296, 2317-2345) worded a condition differently, the fragment is what they share.
REFUSALS = [
    (dict(x=False), -1, "null pointer"),
    (dict(flags=2), -1, "unknown flags 0x2"),
    (dict(dtype=2), -1, "unknown dtype 2"),
    (dict(n=0), -1, "bad shape"),
    (dict(s=0), -1, "bad shape"),
    (dict(p=-1, hist=True), -1, "bad shape"),
    (dict(a=0, h=0), -1, "bad shape"),
    (dict(h=250), -1, "head size must be 64"),
    (dict(s=513), -3, "exceeds the 512-key limit"),
    (dict(s=505, p=8), -3, "exceeds the 512-key limit"),
    (dict(attn_p=1.0), -1, "out of [0, 1)"),
    (dict(attn_p=-0.5), -1, "out of [0, 1)"),
    (dict(s=257, attn_p=0.1), -3, "not implemented above 256 keys"),
    (dict(p=8, hist=False), -1, "P=8 but hist is null"),
    (dict(s=300, p=8, hist=False), -1, "P=8 but hist is null"),
    (dict(key_mask=False), -1, "need key_mask or dense_mask_bits"),
    (dict(s=300, key_mask=False), -1, "need key_mask or dense_mask_bits"),
    (dict(chunk=True, chunk_t=0), -1, "chunk_t=0 out of range"),
    (dict(chunk=True, chunk_t=101), -1, "chunk_t=101 out of range"),
    (dict(s=300, chunk=True, chunk_t=301), -1, "chunk_t=301 out of range"),
    (dict(align=True, align_t=0), -1, "align_t=0 out of range"),
    (dict(align=True, align_t=100), -1, "align_t=100 out of range"),
    (dict(s=300, align=True, align_t=300), -1, "align_t=300 out of range"),
    (dict(s=300, n=65536), -1, "too large"),
    (dict(s=300, ws_bytes=64), -1, "workspace"),
    (dict(s=300, ws=False), -1, "workspace"),
    (dict(dtype=1, ws_bytes=64), -1, "workspace"),
    (dict(dtype=1, ws=False), -1, "workspace"),
    (dict(dump=True, lse=False), -1, "the q|k|v dump comes with lse"),
    (dict(dump=True, lse=True, s=64), -1, "the q|k|v dump comes with lse"),
    (dict(dump=True, lse=True, s=193), -1, "the q|k|v dump comes with lse"),
    (dict(dump=True, lse=True, s=92, p=8), -1, "the q|k|v dump comes with lse"),
    (dict(lse=True, s=64), -3, "no row statistics (lse) on this route"),
    (dict(lse=True, h=192, a=3), -3, "no row statistics (lse) on this route"),
    (dict(lse=True, s=300), -3, "not produced above 256 keys"),
    (dict(lse=True, dtype=1), -1, "written on the bf16 path only"),
    (dict(probs=True, attn_p=0.1), -3, "needs MODCR_ATTN_SIDE_POST_DROPOUT"),
    (dict(probs=True, attn_p=0.1, dtype=1), -1, "needs MODCR_ATTN_SIDE_POST_DROPOUT"),
    (dict(probs=True, attn_p=0.1, flags=1, s=64), -3, "post-dropout side outputs on the tile kernels only"),
    (dict(align=True, align_t=40, attn_p=0.1, flags=1, h=192, a=3), -3, "post-dropout side outputs on the tile kernels only"),
    (dict(sn=-4), -1, "negative stride"),
]
# conditions one family of entries does not have: the bias entry takes any shape under dropout with any side output, serves no
# lse, and needs its workspace at every key count; the binary-mask entries need none on the bf16 tile kernels
BIAS_ACCEPTS = ("needs MODCR_ATTN_SIDE_POST_DROPOUT", "post-dropout side outputs")


def test_single_violation_refusals_through_every_entry(built):
    lib = built.lib()
    buf = ctypes.create_string_buffer(64)
    ptr = (ctypes.addressof(buf) + 15) & ~15
    seen = set()
    for kw, rc_want, text in REFUSALS:
        for entry in ENTRIES:
            bias = entry.endswith("bias_fwd")
            if bias and any(t in text for t in BIAS_ACCEPTS):
                continue
            rc = call(lib, entry, ptr, **kw)
            if rc is None:
                continue
            msg = lib.modcr_last_error().decode()
            assert rc == rc_want and text in msg, (entry, kw, rc, msg)
            assert msg.startswith("qkv_attn_bias_fwd" if bias else "qkv_attn_fwd:") or msg.startswith("qkv_attn_fwd("), (entry, msg)
            seen.add((entry, text))
    # every entry was refused for every condition it has arguments for
    for entry in ENTRIES[:4]:
        assert (entry, "null pointer") in seen and (entry, "workspace") in seen and (entry, "too large") in seen
    assert len({t for e, t in seen if e == "modcr_qkv_attn_opt_fwd"}) == len({t for _, _, t in REFUSALS}) - 1      # (all but the bias stride)
    # bf16 alignment of x / wqkv / ctx / hist, and the bias entry's own 4-byte check
    for entry in ENTRIES:
        rc = call(lib, entry, ptr + 4)
        assert rc == -1 and "(bf16): 16-byte alignment" in lib.modcr_last_error().decode(), entry
        assert call(lib, entry, ptr + 4, dtype=1, ws_bytes=64) == -1 and "workspace" in lib.modcr_last_error().decode(), entry
    assert call(lib, ENTRIES[4], ptr, bias_ptr=ptr + 2) == -1 and "not 4-byte aligned" in lib.modcr_last_error().decode()
    assert call(lib, ENTRIES[4], ptr, ws_bytes=64) == -1 and "workspace" in lib.modcr_last_error().decode()


def test_route_symbol_and_signatures(built):
    assert "modcr_qkv_attn_route" in built.SIGNATURES and len(built.SIGNATURES["modcr_qkv_attn_route"][1]) == 14
    for path in (built.LIB_PATH, built.TUNING_LIB_PATH):
        assert hasattr(ctypes.CDLL(path), "modcr_qkv_attn_route"), path
    want = {"modcr_qkv_attn_fwd": 21, "modcr_qkv_attn_dropout_fwd": 24, "modcr_qkv_attn_lse_fwd": 26, "modcr_qkv_attn_opt_fwd": 27,
            "modcr_qkv_attn_bwd": 20, "modcr_qkv_attn_dropout_bwd": 26, "modcr_qkv_attn_lse_bwd": 29, "modcr_qkv_attn_opt_bwd": 30}
    for name, nargs in want.items():
        assert len(built.SIGNATURES[name][1]) == nargs, name
        for path in (built.LIB_PATH, built.TUNING_LIB_PATH):
            assert hasattr(ctypes.CDLL(path), name), (path, name)
    info = (ctypes.c_int32 * 7)()
    assert built.lib().modcr_qkv_attn_route(0, 0, 0, 2, 100, 0, 256, 4, 0.0, 0, 0, 1, 0, None) == -1      # null info
    assert built.lib().modcr_qkv_attn_route(1 | 32, 0, 0, 2, 100, 0, 256, 4, 0.0, 0, 1 << 30, 1, 0, info) == -1   # the bias entry has no lse
