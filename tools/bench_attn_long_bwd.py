"""Times the attention backward from 257 to 512 keys (modcr_qkv_attn_long_bwd: the streaming cores of csrc/attn_long_bwd.hip), one
process, device events.

Per shape (bf16): the whole call (recomputed projections + core + dX / dW GEMMs), its GEMM steps alone at the same sizes (the q|k|v
projection, dX = dqkv.W, dW = dqkv^T.X; with prefix rows their K | V set too), the core by difference, and as the yardstick of
tools/bench_attn_long.py the forward + backward of torch.nn.functional.scaled_dot_product_attention under autograd on the same
device with the same q / k / v sizes and additive key mask.  For scale: the parent's whole-row exact core at L = 256 through
qkv_attn_bwd, the same way; its host body keeps fp32 rows between the GEMMs and the core, so the GEMM steps are timed with fp32 rows
there and with bf16 rows on the streaming route.  "Core by difference" is an estimate: the call's chunk-free host body has nothing
else in it, but launches timed alone do not overlap as they do inside the call.  The variants run interleaved, --repeats rounds of --iters calls after a warm-up; the median of every
round is kept.  The core's rate counts 10 S (P + S) H flops per sequence (five products) against the 2.5 PF dense bf16 peak.  No
ratio is a pass / fail bound: the file records what was measured.

    python tools/bench_attn_long_bwd.py [--iters 10] [--warmup 3] [--repeats 3] [--out profiles/attn_long_bwd_bench.txt]
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

import modcr_hip as mh  # noqa: E402
from bench_attn_long import median_ms  # noqa: E402

PEAK = 2.5e15
# (N, S, P, H, A): L = 320 and 512 at the Oscar-base width, the RoBERTa-large body with its prompt rows, and the parent's limit
SHAPES = [(64, 320, 0, 768, 12), (64, 512, 0, 768, 12), (64, 300, 10, 1024, 16), (64, 256, 0, 768, 12)]


def bench_shape(n, s, p, h, a, args):
    dev = torch.device("cuda")
    l = p + s
    bf = torch.bfloat16
    x = (torch.randn(n, s, h, device=dev) * 0.5).to(bf)
    hist = (torch.randn(n, p, h, device=dev) * 0.5).to(bf) if p else None
    dctx = (torch.randn(n, s, h, device=dev) * 0.5).to(bf)
    w = (torch.randn(3 * h, h, device=dev) / h ** 0.5).to(bf)
    b = torch.randn(3 * h, device=dev) * 0.1
    dw, db = torch.empty(3 * h, h, device=dev), torch.empty(3 * h, device=dev)
    km = torch.ones(n, l, device=dev)
    km[1::2, l - l // 5:] = 0                                   # every other sequence padded by a fifth
    add = mh.fold_key_mask(km)
    entry = mh.qkv_attn_long_bwd if l > mh.ATTN_BWD_MAX_KEYS else mh.qkv_attn_bwd

    def call():
        return entry(dctx, x, w, b, dw, db, num_heads=a, attn_bias=add, hist=hist)

    route = mh.qkv_attn_long_bwd_route(n, s, p, h, a, mh.BF16)
    rows = (torch.float32, mh.F32) if route == "exact" else (bf, mh.BF16)      # what the host body keeps between GEMMs and core
    qkv = torch.empty(n * s, 3 * h, device=dev, dtype=rows[0])
    dqkv = (torch.randn(n * s, 3 * h, device=dev) * 0.1).to(rows[0])
    dkvh = dqkv[:n * p, :2 * h].contiguous() if p else None
    x2 = x.view(n * s, h)

    def gemms():
        mh.linear(x2, w, b, out_dtype=rows[1], out=qkv)
        mh.linear_bwd_input(dqkv, w, out_dtype=mh.BF16)
        mh.linear_bwd_weight(dqkv, x2, dw, db)
        if p:
            h2 = hist.view(n * p, h)
            mh.linear(h2, w[h:], b[h:], out_dtype=rows[1])
            mh.linear_bwd_input(dkvh, w[h:], out_dtype=mh.BF16)

    q, k, v = ((torch.randn(n, a, t, 64, device=dev) * 0.5).to(bf).requires_grad_(True) for t in (s, l, l))
    mask = add.to(bf)
    go = (torch.randn(n, a, s, 64, device=dev) * 0.5).to(bf)

    def sdpa():
        o = torch.nn.functional.scaled_dot_product_attention(q, k, v, attn_mask=mask)
        o.backward(go)
        q.grad = k.grad = v.grad = None

    variants = [("call", call), ("gemms", gemms), ("sdpa_fwd_bwd", sdpa)]
    times = {name: [] for name, _ in variants}
    for _ in range(args.repeats):
        for name, fn in variants:
            times[name].append(round(median_ms(fn, args.iters, args.warmup), 4))
    med = {k_: statistics.median(v_) for k_, v_ in times.items()}
    core = med["call"] - med["gemms"]
    flops = 10.0 * s * l * h * n
    return json.dumps({"N": n, "S": s, "P": p, "H": h, "A": a, "dtype": "bf16", "core": route, "call_ms": times["call"], "gemm_steps_ms": times["gemms"],
                       "core_by_difference_ms": round(core, 4), "core_peak_fraction": round(flops / (core * 1e-3) / PEAK, 4),
                       "sdpa_fwd_bwd_ms": times["sdpa_fwd_bwd"], "core_vs_sdpa_fwd_bwd": round(core / med["sdpa_fwd_bwd"], 3)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attn_long_bwd_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_attn_long_bwd: needs a GPU")
    torch.manual_seed(0)
    lines = [json.dumps({"device": torch.cuda.get_device_name(0), "iters": args.iters, "warmup": args.warmup, "repeats": args.repeats,
                         "timed": "device events, median per round; core = whole call - its GEMM steps timed alone"})]
    for shape in SHAPES:
        lines.append(bench_shape(*shape, args))
        print(lines[-1], flush=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
