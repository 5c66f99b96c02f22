"""Times the attention backward under an additive bias (modcr_qkv_attn_bias_bwd: csrc/attn_bias_bwd.hip) next to the binary
backward of the same class of core -- mh.qkv_attn_bwd(key_mask=) without lse / dump: attn_bwd_mfma_kernel, which also recomputes
the row statistics -- in one process, back to back, at N = 512, S = 180, H = 768, A = 12, bf16.

Every variant is the WHOLE call (q | k | v recomputed by the projection GEMM, the core, the dX and dW GEMMs), timed with device
events around it; the GEMMs are the same launches in every variant, so a difference is the core's.  Variants:
    binary            key_mask [N,S] 0/1 (every other sequence padded by a fifth)
    bias [N,1,1,S]    the same mask as a 0 / -10000 broadcast bias
    bias [N,A,S,S]    the same mask expanded to a dense bias: N A S S 4 bytes (0.8 GB) more to read
    each bias form with and without d_bias (N A S S 4 bytes to write)
The variants run interleaved, --repeats rounds of --iters calls after a warm-up; the median of every round is kept, so the
round-to-round spread is visible next to the ratios (each bias variant's median of medians over the binary call's).

    python tools/bench_attn_bias_bwd.py [--iters 20] [--warmup 5] [--repeats 3] [--out profiles/attn_bias_bwd_bench.txt]
One JSON line per variant, written to --out as well."""
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

N, S, H, A = 512, 180, 768, 12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attn_bias_bwd_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_attn_bias_bwd: needs a GPU")
    torch.manual_seed(0)
    dev = torch.device("cuda")
    x = (torch.randn(N, S, H, device=dev) * 0.5).to(torch.bfloat16)
    dctx = (torch.randn(N, S, H, device=dev) * 0.5).to(torch.bfloat16)
    w = (torch.randn(3 * H, H, device=dev) / H ** 0.5).to(torch.bfloat16)
    b = torch.randn(3 * H, device=dev) * 0.1
    dw, db = torch.empty(3 * H, H, device=dev), torch.empty(3 * H, device=dev)
    km = torch.ones(N, S, device=dev)
    km[1::2, S - S // 5:] = 0
    add = ((1.0 - km) * -10000.0)[:, None, None, :].contiguous()
    dense = add.expand(N, A, S, S).contiguous()
    d_bias = torch.empty(N, A, S, S, device=dev)
    assert mh.qkv_attn_bias_bwd_route(N, S, H, A, mh.BF16) == "mfma"
    variants = [("binary (key_mask)", dict(key_mask=km)),
                ("bias [N,1,1,S]", dict(attn_bias=add)), ("bias [N,1,1,S] + d_bias", dict(attn_bias=add, d_bias=d_bias)),
                ("bias [N,A,S,S]", dict(attn_bias=dense)), ("bias [N,A,S,S] + d_bias", dict(attn_bias=dense, d_bias=d_bias))]
    # the variants compute the same thing: hold them together before timing them
    ref = mh.qkv_attn_bwd(dctx, x, w, b, dw, db, num_heads=A, key_mask=km).float()
    for name, kw in variants[1:]:
        got = mh.qkv_attn_bwd(dctx, x, w, b, dw, db, num_heads=A, **kw).float()
        err = float((got - ref).abs().max()) / max(1.0, float(ref.abs().max()))
        assert err <= 2e-2, (name, err)
    times = {name: [] for name, _ in variants}
    for _ in range(args.repeats):
        for name, kw in variants:
            times[name].append(round(median_ms(lambda: mh.qkv_attn_bwd(dctx, x, w, b, dw, db, num_heads=A, **kw), args.iters, args.warmup), 4))
    base = statistics.median(times[variants[0][0]])
    lines = [json.dumps({"device": torch.cuda.get_device_name(0), "N": N, "S": S, "H": H, "A": A, "dtype": "bf16", "iters": args.iters,
                         "warmup": args.warmup, "repeats": args.repeats, "timed": "whole call, device events, median per round"})]
    for name, _ in variants:
        lines.append(json.dumps({"variant": name, "call_ms": times[name], "vs_binary": round(statistics.median(times[name]) / base, 4)}))
    print("\n".join(lines), flush=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
