"""Times the dense mask bits and the align map's gradient on the streaming attention cores above 256 keys
(modcr_qkv_attn_long_align_fwd / _bwd), bf16, N = 64, H = 768, at S = 320 and 512 (T = 64 text rows); one process, device events.

  bits against the parent capability: the same phase-3 mask folded into an fp32 [N,1,S,S] 0 / -10000 bias (1 MB per sequence at
      S = 512 against 32 KB of bits).  Forward: the core kernel alone (modcr_time_next_attn); backward: the whole call through
      qkv_attn_long_bwd -- the GEMM steps around the core are the same launches in both legs.
  d_align against without: the backward call with bits and d_align (DALIGN instantiations, the sweep-1 accumulator) against the call
      with bits alone.
The legs run alternating, --repeats rounds of --iters calls after a warm-up; the median of every round is kept, and the spread (max - min
over the rounds) is written beside the median of the rounds.  No ratio is a pass / fail bound: the file records what was measured.

    python tools/bench_attn_long_align.py [--iters 10] [--warmup 3] [--repeats 3] [--out profiles/attn_long_align_bench.txt]
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

SHAPES = [(64, 320, 64, 768, 12), (64, 512, 64, 768, 12)]       # (N, S, T, H, A)


def bench_shape(n, s, t, h, a, args, hip):
    dev = torch.device("cuda")
    bf = torch.bfloat16
    x = (torch.randn(n, s, h, device=dev) * 0.5).to(bf)
    dctx = (torch.randn(n, s, h, device=dev) * 0.5).to(bf)
    w = (torch.randn(3 * h, h, device=dev) / h ** 0.5).to(bf)
    b = torch.randn(3 * h, device=dev) * 0.1
    dw, db = torch.empty(3 * h, h, device=dev), torch.empty(3 * h, device=dev)
    im = torch.ones(n, s, device=dev)
    im[1::2, s - s // 5:] = 0                                   # every other sequence: a fifth of the region slots padded
    im[1::2, t - t // 4:t] = 0                                  # ... and a quarter of the text
    cm = torch.ones(n, t, t, device=dev) * im[:, :t, None] * im[:, None, :t]
    bits = mh.build_phase_mask(im, cm, 3)
    j = torch.arange(s, device=dev)
    see = (bits[:, :, j // 32] >> (j % 32)) & 1
    fold = ((1 - see.float()) * -10000.0).view(n, 1, s, s).contiguous()
    g = torch.randn(n, t, s - t, device=dev)
    ctx = torch.empty_like(x)
    ws = torch.empty(((mh.lib().modcr_qkv_attn_bias_workspace(n, s, 0, h, mh.BF16) + 3) // 4,), dtype=torch.float32, device=dev)
    legs = {
        "fwd_core_bits": lambda: mh.qkv_attn(x, w, b, num_heads=a, dense_bits=bits, out=ctx, workspace=ws),
        "fwd_core_folded": lambda: mh.qkv_attn(x, w, b, num_heads=a, attn_bias=fold, out=ctx, workspace=ws),
        "bwd_call_bits": lambda: mh.qkv_attn_long_bwd(dctx, x, w, b, dw, db, num_heads=a, dense_bits=bits),
        "bwd_call_folded": lambda: mh.qkv_attn_long_bwd(dctx, x, w, b, dw, db, num_heads=a, attn_bias=fold),
        "bwd_call_bits_d_align": lambda: mh.qkv_attn_long_bwd(dctx, x, w, b, dw, db, num_heads=a, dense_bits=bits, d_align=g, align_t=t),
    }
    rounds = {k: [] for k in legs}
    for _ in range(args.repeats):
        for k, fn in legs.items():
            ms = core_ms(fn, args.iters, args.warmup, hip) if k.startswith("fwd_core") else median_ms(fn, args.iters, args.warmup)
            rounds[k].append(round(ms, 4))
    med = {k: statistics.median(v) for k, v in rounds.items()}
    out = {"N": n, "S": s, "T": t, "H": h, "A": a, "dtype": "bf16", "mask_bytes_per_sequence": {"bits": s * ((s + 31) // 32) * 4, "folded": s * s * 4}}
    for k, v in rounds.items():
        out[k + "_ms"] = {"rounds": v, "median": med[k], "spread": round(max(v) - min(v), 4)}
    out.update({"fwd_core_bits_over_folded": round(med["fwd_core_bits"] / med["fwd_core_folded"], 3),
                "bwd_call_bits_over_folded": round(med["bwd_call_bits"] / med["bwd_call_folded"], 3),
                "bwd_call_d_align_over_bits_alone": round(med["bwd_call_bits_d_align"] / med["bwd_call_bits"], 3)})
    return json.dumps(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attn_long_align_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_attn_long_align: needs a GPU")
    torch.manual_seed(0)
    hip = bench.hip_runtime()
    lines = [json.dumps({"device": torch.cuda.get_device_name(0), "iters": args.iters, "warmup": args.warmup, "repeats": args.repeats,
                         "timed": "device events, median per round, legs alternating; forward: the core kernel's own launch; backward: the whole call"})]
    for shape in SHAPES:
        lines.append(bench_shape(*shape, args, hip))
        print(lines[-1], flush=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
