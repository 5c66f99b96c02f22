"""Times what the attention-probability dropout costs the streaming attention cores above 256 keys (the wide counter layout:
modcr_qkv_attn_long_drop_fwd / _bwd), bf16, N = 64, H = 768, at L = 320 and 512, p = 0.1 against p = 0; one process, device events.

Forward: the core kernel alone (modcr_time_next_attn: events stamped by the kernel's own launch), MODE 2 of attn_long_bf16_kernel
against MODE 1.  Backward: the whole call through qkv_attn_long_bwd with p = 0.1 and with p = 0; the GEMM steps around the core are
the same launches in both, so the DIFFERENCE of the two calls is the difference of the cores, and the core's own time is the call
less its GEMM steps timed alone (tools/bench_attn_long_bwd.py's estimate).  The p = 0 legs run the kernels of the parent commit (the
instruction streams of the instantiations without DROP are unchanged).  The variants run interleaved, --repeats rounds of --iters
calls after a warm-up; the median of every round is kept.  No ratio is a pass / fail bound: the file records what was measured.

    python tools/bench_attn_long_drop.py [--iters 10] [--warmup 3] [--repeats 3] [--out profiles/attn_long_drop_bench.txt]
One JSON line per shape, written to --out as well."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "multimodal-context-reasoning_amd"), os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

import bench  # noqa: E402  (hip_runtime: the HIP runtime torch already loaded)
import modcr_hip as mh  # noqa: E402
from bench_attn_long import core_ms, median_ms  # noqa: E402

SHAPES = [(64, 320, 0, 768, 12), (64, 512, 0, 768, 12)]         # (N, S, P, H, A)
P_DROP = 0.1


def bench_shape(n, s, p, h, a, args, hip):
    dev = torch.device("cuda")
    l = p + s
    bf = torch.bfloat16
    x = (torch.randn(n, s, h, device=dev) * 0.5).to(bf)
    dctx = (torch.randn(n, s, h, device=dev) * 0.5).to(bf)
    w = (torch.randn(3 * h, h, device=dev) / h ** 0.5).to(bf)
    b = torch.randn(3 * h, device=dev) * 0.1
    dw, db = torch.empty(3 * h, h, device=dev), torch.empty(3 * h, device=dev)
    km = torch.ones(n, l, device=dev)
    km[1::2, l - l // 5:] = 0                                   # every other sequence padded by a fifth
    add = mh.fold_key_mask(km)
    drop = (P_DROP, 11, 5 << 32)
    ctx = torch.empty_like(x)
    ws = torch.empty(((mh.lib().modcr_qkv_attn_bias_workspace(n, s, p, h, mh.BF16) + 3) // 4,), dtype=torch.float32, device=dev)

    def fwd(d):
        return lambda: mh.qkv_attn(x, w, b, num_heads=a, attn_bias=add, attn_dropout=d, wide_dropout=True, out=ctx, workspace=ws)

    def bwd(d):
        return lambda: mh.qkv_attn_long_bwd(dctx, x, w, b, dw, db, num_heads=a, attn_bias=add, attn_dropout=d, wide_dropout=True)

    qkv = torch.empty(n * s, 3 * h, device=dev, dtype=bf)
    dqkv = (torch.randn(n * s, 3 * h, device=dev) * 0.1).to(bf)
    x2 = x.view(n * s, h)

    def gemms():
        mh.linear(x2, w, b, out_dtype=mh.BF16, out=qkv)
        mh.linear_bwd_input(dqkv, w, out_dtype=mh.BF16)
        mh.linear_bwd_weight(dqkv, x2, dw, db)

    t = {k: [] for k in ("fwd_core_p0", "fwd_core_drop", "bwd_call_p0", "bwd_call_drop", "bwd_gemms")}
    for _ in range(args.repeats):
        t["fwd_core_p0"].append(round(core_ms(fwd(None), args.iters, args.warmup, hip), 4))
        t["fwd_core_drop"].append(round(core_ms(fwd(drop), args.iters, args.warmup, hip), 4))
        t["bwd_call_p0"].append(round(median_ms(bwd(None), args.iters, args.warmup), 4))
        t["bwd_call_drop"].append(round(median_ms(bwd(drop), args.iters, args.warmup), 4))
        t["bwd_gemms"].append(round(median_ms(gemms, args.iters, args.warmup), 4))
    med = {k: statistics.median(v) for k, v in t.items()}
    core0, core1 = med["bwd_call_p0"] - med["bwd_gemms"], med["bwd_call_drop"] - med["bwd_gemms"]
    out = {"N": n, "S": s, "P": p, "H": h, "A": a, "dtype": "bf16", "p": P_DROP}
    out.update({k + "_ms": v for k, v in t.items()})
    out.update({"fwd_core_drop_over_p0": round(med["fwd_core_drop"] / med["fwd_core_p0"], 3),
                "bwd_core_by_difference_p0_ms": round(core0, 4), "bwd_core_by_difference_drop_ms": round(core1, 4),
                "bwd_core_drop_over_p0": round(core1 / core0, 3), "bwd_call_drop_over_p0": round(med["bwd_call_drop"] / med["bwd_call_p0"], 3)})
    return json.dumps(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attn_long_drop_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_attn_long_drop: needs a GPU")
    torch.manual_seed(0)
    hip = bench.hip_runtime()
    lines = [json.dumps({"device": torch.cuda.get_device_name(0), "iters": args.iters, "warmup": args.warmup, "repeats": args.repeats,
                         "timed": "device events, median per round; forward: the core kernel's own launch; backward: whole call, core = call - its "
                                  "GEMM steps timed alone"})]
    for shape in SHAPES:
        lines.append(bench_shape(*shape, args, hip))
        print(lines[-1], flush=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
