"""Host answers of the GEMM entries of two builds of libmodcr_hip.so, side by side (CPU, no GPU needed): every _workspace value,
modcr_ffn_keep_supported, modcr_linear_route and every REFUSED call (return code and message) must be equal.  Used when a change
touches the host code of csrc/gemm.hip (linear_args, route_bwd_weight, route_bwd_input, the plans) and must leave what the entries
answer as it was.  Refused calls are made with never-read pointers; a call that would pass validation is not made.

    python tools/linear_bwd_host_equivalence.py --parent /path/to/parent/libmodcr_hip.so [--out profiles/...txt]
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

MS = list(range(1, 521, 7)) + [1024, 4096, 46080, 92160, 143872]
NK = [1, 48, 64, 100, 192, 256, 320, 512, 768, 1024, 2304, 3072]
WORKSPACES = ("modcr_linear_bwd_weight_workspace", "modcr_linear_bwd_input_workspace", "modcr_linear_splitk_workspace",
              "modcr_linear_residual_ln_bwd_workspace", "modcr_ffn_up_du_bwd_workspace", "modcr_ffn_up_gelu_bwd_workspace",
              "modcr_ffn_down_gelu_bwd_workspace")


def load(path):
    lib = ctypes.CDLL(path)
    for name, (res, args) in mh.SIGNATURES.items():
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
    return lib


def sweep_values(a, b):
    n_eq = 0
    ia, ib = (ctypes.c_int32 * 4)(), (ctypes.c_int32 * 4)()
    for m, n, k in itertools.product(MS, NK, NK):
        for name in WORKSPACES:
            va, vb = getattr(a, name)(m, n, k), getattr(b, name)(m, n, k)
            assert va == vb, (name, m, n, k, va, vb)
            n_eq += 1
        for dt in (mh.BF16, mh.F32):
            va, vb = a.modcr_ffn_keep_supported(m, n, k, dt), b.modcr_ffn_keep_supported(m, n, k, dt)
            assert va == vb, ("modcr_ffn_keep_supported", m, n, k, dt)
            n_eq += 1
        # modcr_linear_route: dense and padded strides, with and without a residual, the three output types
        for (pad, res, od, act) in ((0, None, mh.BF16, mh.ACT_GELU), (8, 256, mh.F32, mh.ACT_NONE), (0, 256, mh.F16, mh.ACT_NONE), (4, None, mh.F32, mh.ACT_TANH)):
            args = (256, k + pad, 256, k + pad, 256, res, n + pad, mh.F32, 256, n + pad, m, n, k, act, mh.BF16, od)
            ra, rb = a.modcr_linear_route(*args, ia), b.modcr_linear_route(*args, ib)
            assert ra == rb and (ra != 0 or list(ia) == list(ib)), ("modcr_linear_route", args, ra, rb, list(ia), list(ib))
            assert ra == 0 or a.modcr_last_error() == b.modcr_last_error(), args
            n_eq += 1
    return n_eq


def refused_calls(a, b):
    """the compute entries with a fault that validation catches before any launch: return code and message of both builds"""
    buf = ctypes.create_string_buffer(64)
    q = (ctypes.addressof(buf) + 15) & ~15
    odd = q + 4
    big = 1 << 50
    calls = []

    def add(name, *args):
        calls.append((name, args))

    for dy, x, dw, m, n, k in ((None, q, q, 256, 256, 256), (q, None, q, 256, 256, 256), (q, q, None, 256, 256, 256), (q, q, q, 0, 256, 256),
                               (q, q, q, 256, -1, 256), (q, q, q, 256, 256, 0)):
        add("modcr_linear_bwd_weight", dy, n, 0, x, k, dw, q, m, n, k, 0, 0, q, big, None)
        add("modcr_linear_bwd_input", dy, n, 0, x, k, dw, k, m, n, k, 0, 0, q, big, None)
    for a_, w_, c_, ws_, lda, m, n, k, wsb in ((None, q, q, q, 1024, 256, 256, 1024, big), (q, q, q, None, 1024, 256, 256, 1024, big),
                                              (q, q, q, q, 1024, 256, 256, 512, big), (q, q, q, q, 1024, 128, 256, 1024, big),
                                              (q, q, q, q, 1024, 256, 256, 1024, 16), (q, q, q, q, 1028, 256, 256, 1024, big),
                                              (odd, q, q, q, 1024, 256, 256, 1024, big), (q, q, q, odd, 1024, 256, 256, 1024, big)):
        add("modcr_linear_splitk_fwd", a_, lda, w_, k, None, c_, n, m, n, k, 0, 1, ws_, wsb, None)
    for a_, m, n, k, lda, ldc in ((None, 256, 256, 256, 256, 256), (q, 0, 256, 256, 256, 256), (q, 256, 256, 256, 128, 256), (q, 256, 256, 256, 256, 128),
                                  (q, 256, 256, 200, 200, 256), (odd, 256, 256, 256, 256, 256)):
        add("modcr_linear_fwd", a_, lda, q, lda, None, None, 0, 0, q, ldc, m, n, k, 0, 0, 0, None)
    add("modcr_linear_fwd", q, 256, q, 256, None, None, 0, 0, q, 256, 256, 256, 256, 7, 0, 0, None)
    add("modcr_linear_fwd", q, 256, q, 256, None, None, 0, 0, q, 256, 256, 256, 256, 1, 0, 2, None)
    for dy, lda, m, n, k, wsb in ((None, 256, 512, 256, 256, big), (q, 264, 512, 256, 256, big), (q, 256, 512, 256, 256, 16), (q, 1024, 512, 768, 1024, 1 << 20)):
        add("modcr_linear_residual_ln_dropout_bwd", dy, 0, q, 0, q, lda, q, q, 1e-5, q, q, q, q, q, q, m, n, k, 0.0, 0, 0, q, wsb, 0, None)
    add("modcr_linear_residual_ln_dropout_bwd", q, 0, q, 0, q, 256, q, q, 1e-5, q, q, q, q, q, q, 512, 320, 256, 0.1, 0, 0, q, big, 0, None)
    for dy, m, h, i, dt, wsb in ((None, 512, 256, 1024, 0, big), (q, 100, 256, 1024, 0, big), (q, 512, 320, 1024, 0, big), (q, 512, 256, 1024, 1, big),
                                 (q, 512, 256, 1024, 0, 16), (q, 512, 256, 1024, 0, 0)):
        add("modcr_ffn_down_residual_ln_gelu_bwd", dy, 0, q, 0, q, q, q, 1e-5, q, q, q, q, q, q, q, q, m, h, i, 0.0, 0, 0, q, wsb, dt, None)
        add("modcr_ffn_up_du_bwd", dy, q, q, None, q, q, q, m, h, i, q, wsb, dt, None)
        if wsb == big:              # (no workspace argument: the last two would pass validation)
            add("modcr_ffn_up_gelu_keep_fwd", dy, q, q, q, q, m, h, i, dt, None)
    add("modcr_ffn_up_gelu_keep_fwd", odd, q, q, q, q, 512, 256, 1024, 0, None)
    add("modcr_ffn_up_gelu_keep_fwd", q, q, q, q, odd, 512, 256, 1024, 0, None)
    for dy, wsb, ws_ in ((None, big, q), (q, 16, q), (q, big, None)):
        add("modcr_ffn_up_gelu_bwd", dy, 0, q, q, q, None, q, q, q, 512, 256, 1024, ws_, wsb, 0, None)
    n_cmp, distinct = 0, set()
    for name, args in calls:
        ra = getattr(a, name)(*args)
        if ra == 0:
            raise SystemExit("a call passed validation: %s %r" % (name, args))
        ma = a.modcr_last_error()
        rb = getattr(b, name)(*args)
        mb = b.modcr_last_error()
        assert ra == rb and ma == mb, (name, args, ra, rb, ma, mb)
        n_cmp += 1
        distinct.add((name, ma))
    return n_cmp, len(distinct)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True)
    ap.add_argument("--branch", default=mh.LIB_PATH)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    a, b = load(args.parent), load(args.branch)
    n_val = sweep_values(a, b)
    n_cmp, n_distinct = refused_calls(a, b)
    text = ("host equivalence of the GEMM entries, parent build against this build (ctypes, no GPU):\n"
            "  values: %d equal (the seven *_workspace queries, modcr_ffn_keep_supported for bf16 / fp32, modcr_linear_route with four\n"
            "    stride / residual / output / activation settings; M in {1..520 step 7, 1024, 4096, 46080, 92160, 143872} x N, K in\n"
            "    {1, 48, 64, 100, 192, 256, 320, 512, 768, 1024, 2304, 3072})\n"
            "  refused calls: %d compared (return code and message equal), %d distinct (entry, message) pairs (modcr_linear_fwd, _splitk_fwd,\n"
            "    _bwd_weight, _bwd_input, _residual_ln_dropout_bwd, modcr_ffn_down_residual_ln_gelu_bwd, _up_du_bwd, _up_gelu_bwd, _up_gelu_keep_fwd)\n"
            % (n_val, n_cmp, n_distinct))
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "a") as f:
            f.write(text)


if __name__ == "__main__":
    main()
