"""Times the attention backward with prefix rows (modcr_qkv_attn_prefix_bwd: csrc/attn_bias_bwd.hip) next to the only thing
the library offered for the same gradients before it: modcr_qkv_attn_bias_bwd over the concatenated [hist ; x] rows, with zero
dctx rows for the prefix (their queries then add nothing) and the bias over L = P + S query rows, dx[:, :P] being d_hist.

Shapes (bf16): N = 512, S = 180, P = 10, H = 768, A = 12 (L = 190: the MFMA cores) and N = 128, S = 220, P = 10, H = 1024, A = 16
(L = 230: the exact cores).  The bias is a 0 / -10000 [N,1,1,L] padding mask (every other sequence padded by a fifth), broadcast
over the queries, so the emulation needs no padded bias rows.  Every variant is the WHOLE call, timed with device events:
    prefix                   qkv_attn_bwd(hist=): S query rows, K | V GEMMs only for the P prefix rows, no copies
    emulation                torch.cat of [hist ; x] and [0 ; dctx], qkv_attn_bwd(attn_bias=) over L rows, the split of dx
    emulation, no copies     the same call on rows concatenated beforehand (what the copies cost is the difference)
The variants run interleaved, --repeats rounds of --iters calls after a warm-up; the median of every round is kept.

    python tools/bench_attn_prefix_bwd.py [--iters 20] [--warmup 5] [--repeats 3] [--out profiles/attn_prefix_bwd_bench.txt]
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

SHAPES = [(512, 180, 10, 768, 12), (128, 220, 10, 1024, 16)]


def bench_shape(n, s, p, h, a, args):
    dev = torch.device("cuda")
    l = p + s
    x = (torch.randn(n, s, h, device=dev) * 0.5).to(torch.bfloat16)
    hist = (torch.randn(n, p, h, device=dev) * 0.5).to(torch.bfloat16)
    dctx = (torch.randn(n, s, h, device=dev) * 0.5).to(torch.bfloat16)
    w = (torch.randn(3 * h, h, device=dev) / h ** 0.5).to(torch.bfloat16)
    b = torch.randn(3 * h, device=dev) * 0.1
    dw, db = torch.empty(3 * h, h, device=dev), torch.empty(3 * h, device=dev)
    km = torch.ones(n, l, device=dev)
    km[1::2, l - l // 5:] = 0
    add = mh.fold_key_mask(km)
    zeros = torch.zeros(n, p, h, device=dev, dtype=torch.bfloat16)
    xc, dc = torch.cat([hist, x], 1), torch.cat([zeros, dctx], 1)

    def prefix():
        return mh.qkv_attn_bwd(dctx, x, w, b, dw, db, num_heads=a, attn_bias=add, hist=hist)

    def emulation():
        dxc = mh.qkv_attn_bwd(torch.cat([zeros, dctx], 1), torch.cat([hist, x], 1), w, b, dw, db, num_heads=a, attn_bias=add)
        return dxc[:, p:].contiguous(), dxc[:, :p].contiguous()

    def emulation_no_copies():
        dxc = mh.qkv_attn_bwd(dc, xc, w, b, dw, db, num_heads=a, attn_bias=add)
        return dxc[:, p:], dxc[:, :p]
    variants = [("prefix", prefix), ("emulation", emulation), ("emulation, no copies", emulation_no_copies)]
    # the variants compute the same thing: hold them together before timing them
    dx, dh = prefix()
    dw_ref = dw.clone()
    ex, eh = emulation()
    for nm, g, r in (("dx", dx, ex), ("d_hist", dh, eh), ("dwqkv", dw_ref, dw)):
        err = float((g.float() - r.float()).abs().max()) / max(1.0, float(r.float().abs().max()))
        assert err <= 2e-2, (nm, err)
    times = {name: [] for name, _ in variants}
    for _ in range(args.repeats):
        for name, fn in variants:
            times[name].append(round(median_ms(fn, args.iters, args.warmup), 4))
    base = statistics.median(times["emulation"])
    lines = [json.dumps({"N": n, "S": s, "P": p, "H": h, "A": a, "dtype": "bf16", "core": mh.qkv_attn_prefix_bwd_route(n, s, p, h, a, mh.BF16),
                         "emulation_core": mh.qkv_attn_bias_bwd_route(n, l, h, a, mh.BF16)})]
    for name, _ in variants:
        lines.append(json.dumps({"variant": name, "call_ms": times[name], "vs_emulation": round(statistics.median(times[name]) / base, 4)}))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attn_prefix_bwd_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_attn_prefix_bwd: needs a GPU")
    torch.manual_seed(0)
    lines = [json.dumps({"device": torch.cuda.get_device_name(0), "iters": args.iters, "warmup": args.warmup, "repeats": args.repeats,
                         "timed": "whole call, device events, median per round"})]
    for shape in SHAPES:
        lines += bench_shape(*shape, args)
    print("\n".join(lines), flush=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
