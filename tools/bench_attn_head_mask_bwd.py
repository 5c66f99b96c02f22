"""What the head-mask gradient costs: the attention backward under a bias and a head mask with and without d_head_mask, in one
process on one build (modcr_qkv_attn_gate_bwd's DHM instantiations of csrc/attn_bias_bwd.hip against the existing instantiations
behind modcr_qkv_attn_bias_bwd).

Shapes (bf16): N = 512, S = 180, H = 768, A = 12 (the MFMA core) and N = 128, S = 230, H = 1024, A = 16 (the exact core); a
0 / -10000 [N,1,1,S] padding mask (every other sequence padded by a fifth), a head mask [A], attention dropout p = 0.1.  The two
calls differ in the core alone (same projections, same GEMMs), so the difference of the whole-call times is the core's; every
variant is the WHOLE call, timed with device events.  The variants run interleaved, --repeats rounds of --iters calls after a
warm-up, the median of every round is kept; the variant without d_head_mask runs TWICE per round ("without", "without again"), and
the distance between those two is the noise a difference has to exceed.  Before timing, dx / dWqkv / dbqkv of the two calls are
compared bit for bit.

    python tools/bench_attn_head_mask_bwd.py [--iters 20] [--warmup 5] [--repeats 5] [--out profiles/attn_head_mask_bwd_bench.txt]
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

SHAPES = [(512, 180, 768, 12), (128, 230, 1024, 16)]


def bench_shape(n, s, h, a, args):
    dev = torch.device("cuda")
    x = (torch.randn(n, s, h, device=dev) * 0.5).to(torch.bfloat16)
    dctx = (torch.randn(n, s, h, device=dev) * 0.5).to(torch.bfloat16)
    w = (torch.randn(3 * h, h, device=dev) / h ** 0.5).to(torch.bfloat16)
    b = torch.randn(3 * h, device=dev) * 0.1
    dw, db = torch.empty(3 * h, h, device=dev), torch.empty(3 * h, device=dev)
    km = torch.ones(n, s, device=dev)
    km[1::2, s - s // 5:] = 0
    add = mh.fold_key_mask(km)
    hm = torch.linspace(1.0, 0.5, a, device=dev)
    d_hm = torch.empty(n, a, device=dev)
    drop = (0.1, 11, 0)

    def without():
        return mh.qkv_attn_bwd(dctx, x, w, b, dw, db, num_heads=a, attn_dropout=drop, attn_bias=add, head_mask=hm)

    def with_():
        return mh.qkv_attn_bwd(dctx, x, w, b, dw, db, num_heads=a, attn_dropout=drop, attn_bias=add, head_mask=hm, d_head_mask=d_hm)
    # the two calls compute the same dx / dWqkv / dbqkv, bit for bit
    dx0 = without()
    dw0, db0 = dw.clone(), db.clone()
    dx1 = with_()
    torch.cuda.synchronize()
    assert torch.equal(dx0, dx1) and torch.equal(dw0, dw) and torch.equal(db0, db) and bool(torch.isfinite(d_hm).all())
    variants = [("without", without), ("with d_head_mask", with_), ("without again", without)]
    times = {name: [] for name, _ in variants}
    for _ in range(args.repeats):
        for name, fn in variants:
            times[name].append(round(median_ms(fn, args.iters, args.warmup), 4))
    med = {name: statistics.median(ts) for name, ts in times.items()}
    base = med["without"]
    lines = [json.dumps({"N": n, "S": s, "H": h, "A": a, "dtype": "bf16", "core": mh.qkv_attn_gate_bwd_route(n, s, 0, h, a, mh.BF16)})]
    for name, _ in variants:
        lines.append(json.dumps({"variant": name, "call_ms": times[name], "median_ms": round(med[name], 4),
                                 "minus_without_us": round(1e3 * (med[name] - base), 1), "vs_without": round(med[name] / base, 4)}))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attn_head_mask_bwd_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_attn_head_mask_bwd: needs a GPU")
    torch.manual_seed(0)
    lines = [json.dumps({"device": torch.cuda.get_device_name(0), "iters": args.iters, "warmup": args.warmup, "repeats": args.repeats,
                         "timed": "whole call, device events, median per round; 'without again' = the noise floor"})]
    for shape in SHAPES:
        lines += bench_shape(*shape, args)
    print("\n".join(lines), flush=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
