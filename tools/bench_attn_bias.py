"""Times the additive-bias attention forward (modcr_qkv_attn_bias_fwd: the bias variant of the streaming core in csrc/attn_long.hip)
next to the binary-mask routes of the same shapes, one process, bf16, kernel-exact HIP events (modcr_time_next_attn: stamped by the
attention kernel's own launch).

Per S: the core with a key-broadcast bias [N,1,1,L] and with a per-query bias [N,1,S,L] (the 0 / -10000 padding mask of the binary
run, so all three compute the same thing), and the binary route of the parent: the fused tile kernel at S <= 256 (projection
included: it is one launch), the attn_long core above.  The general route's projection runs in separate launches; `total_ms` (events
around the whole call) shows what a caller pays.  Warm-up, then --repeats x --iters launches: the median of every repeat is printed,
so the run-to-run spread is visible.

    python tools/bench_attn_bias.py [--iters 30] [--warmup 10] [--repeats 3]
One JSON line per (S, variant)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "multimodal-context-reasoning_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

import bench  # noqa: E402  (hip_runtime: the HIP runtime torch already loaded)
import modcr_hip as mh  # noqa: E402
from bench_attn_long import core_ms, median_ms  # noqa: E402

N, H, A = 64, 768, 12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    torch.manual_seed(0)
    dev = torch.device("cuda")
    hip = bench.hip_runtime()
    print(json.dumps({"device": torch.cuda.get_device_name(0), "iters": args.iters, "warmup": args.warmup, "repeats": args.repeats}), flush=True)
    for s in (180, 300):
        x = (torch.randn(N, s, H, device=dev) * 0.5).to(torch.bfloat16)
        w = (torch.randn(3 * H, H, device=dev) / H ** 0.5).to(torch.bfloat16)
        b = torch.randn(3 * H, device=dev) * 0.1
        km = torch.ones(N, s, device=dev)
        km[1::2, s - s // 5:] = 0                               # every other sequence padded by a fifth
        add = ((1.0 - km) * -10000.0)[:, None, None, :]
        add_q = add.expand(N, 1, s, s).contiguous()             # the same mask with a row per query: N S L 4 bytes more to read
        need = max(mh.lib().modcr_qkv_attn_bias_workspace(N, s, 0, H, mh.BF16), mh.lib().modcr_qkv_attn_workspace(N, s, 0, H, mh.BF16))
        ws = torch.empty(need // 4, device=dev)
        ctx = torch.empty_like(x)
        variants = [("binary route (%s)" % ("fused tile kernel" if s <= 256 else "attn_long core"), dict(key_mask=km)),
                    ("bias [N,1,1,L]", dict(attn_bias=add)), ("bias [N,1,S,L]", dict(attn_bias=add_q))]
        for name, kw in variants:
            def call():
                mh.qkv_attn(x, w, b, num_heads=A, workspace=ws, out=ctx, **kw)
            kernel = [round(core_ms(call, args.iters, args.warmup, hip), 4) for _ in range(args.repeats)]
            total = [round(median_ms(call, args.iters, args.warmup), 4) for _ in range(args.repeats)]
            print(json.dumps({"N": N, "S": s, "H": H, "A": A, "variant": name, "attention_kernel_ms": kernel, "total_ms": total}), flush=True)


if __name__ == "__main__":
    main()
