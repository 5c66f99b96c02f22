"""Host answers of the attention entries of two builds of libmodcr_hip.so, side by side (CPU, no GPU needed): every _workspace and
_route value and every REFUSED call (return code and message) of the entries both builds export must be equal.  Used when a change
adds entries or fields to the shared host bodies (csrc/attn.hip: attn_fwd; csrc/attn_bwd_host.hip: attn_bwd) and must leave the
existing entries as they were.  Refused calls are made with never-read pointers; a call that would pass validation is not made.

    python tools/attn_host_equivalence.py --parent /path/to/parent/libmodcr_hip.so [--out profiles/...txt]
"""
import argparse
import ctypes
import itertools
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p_ in (ROOT, os.path.join(ROOT, "multimodal-context-reasoning_amd")):
    if p_ not in sys.path:
        sys.path.insert(0, p_)

import modcr_hip as mh  # noqa: E402

BWD_BIAS = ("gate", "long", "prefix", "bias")


def load(path):
    lib = ctypes.CDLL(path)
    for name, (res, args) in mh.SIGNATURES.items():
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
    lib.modcr_last_error.restype = ctypes.c_char_p
    return lib


def shapes():
    for l in list(range(1, 521, 9)) + [191, 192, 193, 255, 256, 257, 258, 511, 512, 513, 520]:
        yield l, 0
        if l > 10:
            yield l - 10, 10
        if l > 64:
            yield 64, l - 64
    for s, p in ((0, 300), (300, -1), (2 ** 31 - 1, 2)):
        yield s, p


def sweep_values(a, b):
    n_eq = 0
    for dt, n, (h, heads), (s, p) in itertools.product((0, 1, 7), (0, 1, 3, 128), ((64, 1), (128, 2), (768, 12), (100, 2)), list(shapes())):
        calls = [("modcr_qkv_attn_workspace", (n, s, p, h, dt)), ("modcr_qkv_attn_bias_workspace", (n, s, p, h, dt)),
                 ("modcr_qkv_attn_bwd_workspace", (n, s, h, dt)), ("modcr_qkv_attn_bias_bwd_workspace", (n, s, h, dt)),
                 ("modcr_qkv_attn_bias_bwd_route", (n, s, h, heads, dt))]
        for e in ("prefix", "gate", "long"):
            calls.append(("modcr_qkv_attn_%s_bwd_workspace" % e, (n, s, p, h, dt)))
            calls.append(("modcr_qkv_attn_%s_bwd_route" % e, (n, s, p, h, heads, dt)))
        for name, args in calls:
            va, vb = getattr(a, name)(*args), getattr(b, name)(*args)
            assert va == vb, (name, args, va, vb)
            n_eq += 1
    # modcr_qkv_attn_route: families, instantiations and refusals of the forward for the same scalars
    info_a, info_b = (ctypes.c_int32 * 7)(), (ctypes.c_int32 * 7)()
    for present, (s, p), (h, heads), attn_p, flags, ws, dt in itertools.product(
            (0, 1, 2, 8, 1 | 8, 16 | 4, 32, 64 | 32, 128), ((8, 0), (100, 0), (180, 10), (230, 0), (256, 0), (257, 0), (300, 0), (250, 70), (512, 0), (513, 0)),
            ((128, 2), (768, 12)), (0.0, 0.1), (0, 1, 2), (0, 1 << 40), (0, 1)):
        args = (present, 4 if present & 4 else 0, 3 if present & 16 else 0, 2, s, p, h, heads, attn_p, flags, ws, 1, dt)
        ra, rb = a.modcr_qkv_attn_route(*args, info_a), b.modcr_qkv_attn_route(*args, info_b)
        assert ra == rb and (ra != 0 or list(info_a) == list(info_b)), (args, ra, rb)
        assert ra == 0 or a.modcr_last_error() == b.modcr_last_error(), (args, a.modcr_last_error(), b.modcr_last_error())
        n_eq += 1
    return n_eq


def refused_calls(a, b):
    """every pre-existing entry with one or two faults: return code and message of both builds"""
    buf = ctypes.create_string_buffer(64)
    good = (ctypes.addressof(buf) + 15) & ~15
    n_cmp, distinct = 0, set()
    base = dict(n=1, s=300, p=0, h=128, a=2, attn_p=0.0, dt=0, ws=1 << 40, flags=0, ptr=good, bias=True, chunk_t=0, align_t=0)
    faults = [dict(), dict(s=513), dict(s=503, p=10), dict(attn_p=0.1), dict(attn_p=0.1, p=10, s=290), dict(attn_p=1.5), dict(attn_p=1.5, s=100),
              dict(ptr=0), dict(h=100), dict(a=0), dict(n=0), dict(n=70000), dict(ws=16), dict(ws=16, s=8), dict(dt=7), dict(flags=2),
              dict(flags=2, s=100), dict(bias=False), dict(p=-1), dict(s=0), dict(s=256, ws=16), dict(s=257, ws=16), dict(s=192, ws=16), dict(dt=1, ws=16),
              dict(attn_p=0.1, dt=1), dict(chunk_t=400), dict(align_t=400), dict(n=65535, h=4096, a=64, ws=16), dict(n=65535, h=4096, a=64, attn_p=0.1),
              dict(s=100, ptr=good + 4, ws=16), dict(s=100, attn_p=0.1, ws=16)]

    def bwd_bias_family(lib, e, k):
        q = ctypes.c_void_p(k["ptr"]) if k["ptr"] else None
        hq = q if k["p"] > 0 else None
        bq = q if k["bias"] else None
        cq = q if k["chunk_t"] else None
        tail = (k["attn_p"], 1, 2, q, k["ws"], k["dt"], None)
        if e == "bias":
            return lib.modcr_qkv_attn_bias_bwd(q, q, q, q, bq, 0, 0, 0, None, 0, cq, k["chunk_t"], None, q, q, q, 0, None, k["n"], k["s"], k["h"], k["a"], *tail)
        if e == "prefix":
            return lib.modcr_qkv_attn_prefix_bwd(q, q, hq, q, q, bq, 0, 0, 0, None, 0, None, q, hq, q, q, 0, None, k["n"], k["s"], k["p"], k["h"], k["a"], *tail)
        return getattr(lib, "modcr_qkv_attn_%s_bwd" % e)(q, q, hq, q, q, bq, 0, 0, 0, None, 0, cq, k["chunk_t"], None, q, hq, q, q, 0, None, None, k["n"], k["s"],
                                                         k["p"], k["h"], k["a"], *tail)

    def bwd_mask_family(lib, k):
        q = ctypes.c_void_p(k["ptr"]) if k["ptr"] else None
        mq = q if k["bias"] else None
        return lib.modcr_qkv_attn_opt_bwd(q, q, q, q, mq, None, q if k["chunk_t"] else None, k["chunk_t"], None, q, q, q, 0, k["n"], k["s"], k["h"], k["a"],
                                          k["attn_p"], 1, 2, q if k["align_t"] else None, k["align_t"], None, None, None, k["flags"], q, k["ws"], k["dt"], None)

    def fwd_opt(lib, k):
        q = ctypes.c_void_p(k["ptr"]) if k["ptr"] else None
        return lib.modcr_qkv_attn_opt_fwd(q, q if k["p"] > 0 else None, q, q, q if k["bias"] else None, None, q if k["chunk_t"] else None, k["chunk_t"], q, None,
                                          q if k["align_t"] else None, k["align_t"], None, None, k["n"], k["s"], k["p"], k["h"], k["a"], k["attn_p"], 1, 2,
                                          k["flags"], q, k["ws"], k["dt"], None)

    def fwd_bias(lib, k):
        q = ctypes.c_void_p(k["ptr"]) if k["ptr"] else None
        return lib.modcr_qkv_attn_bias_fwd(q, q if k["p"] > 0 else None, q, q, q if k["bias"] else None, 0, 0, 0, None, 0, q if k["chunk_t"] else None,
                                           k["chunk_t"], q, None, q if k["align_t"] else None, k["align_t"], k["n"], k["s"], k["p"], k["h"], k["a"],
                                           k["attn_p"], 1, 2, k["flags"], q, k["ws"], k["dt"], None)

    entries = [("bwd_" + e, lambda lib, k, e=e: bwd_bias_family(lib, e, k)) for e in BWD_BIAS]
    entries += [("opt_bwd", bwd_mask_family), ("opt_fwd", fwd_opt), ("bias_fwd", fwd_bias)]
    combos = [f for f in faults] + [dict(f, **g) for f, g in itertools.combinations(faults[1:], 2)]
    for k_over in combos:
        k = dict(base, **k_over)
        # only calls that certainly fail validation are made: a fault must be present
        if not k_over:
            continue
        for name, fn in entries:
            ra = fn(a, k)
            ma = a.modcr_last_error() if ra != 0 else b""
            if ra == 0:
                raise SystemExit("a call passed validation: %s %r" % (name, k_over))
            rb = fn(b, k)
            mb = b.modcr_last_error()
            assert ra == rb and ma == mb, (name, k_over, ra, rb, ma, mb)
            n_cmp += 1
            distinct.add((name, ma))
    return n_cmp, len(distinct)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    a, b = load(args.parent), load(mh.LIB_PATH)
    n_val = sweep_values(a, b)
    n_cmp, n_distinct = refused_calls(a, b)
    text = ("host equivalence of the attention entries, parent build against this build (ctypes, no GPU):\n"
            "  workspace / route values: %d equal (the forward's two workspace queries and modcr_qkv_attn_route, the backward's five workspace and four\n"
            "    route queries; dtype x N x (H, A) x (S, P) around 192 / 256 / 512 / 513 and malformed shapes)\n"
            "  refused calls: %d compared (return code and message equal), %d distinct (entry, message) pairs (modcr_qkv_attn_opt_fwd, _bias_fwd,\n"
            "    _opt_bwd, _bias_bwd, _prefix_bwd, _gate_bwd, _long_bwd; one fault and every pair of faults, so the ORDER of the checks is compared too)\n"
            % (n_val, n_cmp, n_distinct))
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
