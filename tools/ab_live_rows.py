#!/usr/bin/env python
"""The headline training step (bench.py's model, batches and optimizer: 128 examples, T = 80, R = 100, hidden dropout 0.3, attention
dropout 0.1) with modeling_transfomres.LIVE_ROWS off / on in ONE process, interleaved rounds: ms per step of each run, and whether
the two routes' losses agree bit for bit.  Every run starts from the same weights, optimizer state and dropout seed (a snapshot
taken before the first run is restored), so equal routes give equal loss sequences and the tool compares them step by step.
    python tools/ab_live_rows.py [--rounds 3] [--steps 20] [--warmup 3] [--batch 128] [--min-regions 20]
--min-regions 100: every region slot is filled, nothing is dead, M' = M -- the switch must then cost nothing."""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multimodal-context-reasoning_amd"))
import modcr_hip as mh  # noqa: E402
from Data import synthetic  # noqa: E402
from modeling import modeling_transfomres as mt  # noqa: E402
from modeling import train_utils as tu  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--batch", type=int, default=128)
ap.add_argument("--min-regions", type=int, default=20)
args = ap.parse_args()

dev = torch.device("cuda")
model = tu.build_model(dev, seed=0, hidden_dropout_prob=0.3, attention_probs_dropout_prob=0.1)
model.train()
names = tu.trainable_parameters(model)
pdict = dict(model.named_parameters())
for k, p in pdict.items():
    p.requires_grad_(k in names)
flat = tu.FlatGrads([pdict[k] for k in names], dev, names=names)
opt = tu.FlatAdamW(flat, names, t_total=100000)
batches = [tu.batch_to_device(synthetic.make_batch(args.batch, T=80, R=100, seed=1234 + i, min_regions=args.min_regions), dev) for i in range(4)]
live = batches[0]["live_rows"]
print("batch 0: %d of %d rows dead (pair %d -> %d launch rows, seq_enc %d -> %d)" % (
    live.dead_rows + live.full.capacity - live.full.m_live, live.pair.capacity + live.full.capacity, live.pair.capacity, live.pair.m_launch,
    live.full.capacity, live.full.m_launch), flush=True)


start = (opt.flat_p.clone(), opt.state_dict())      # every run starts here


def run(on):
    """(ms per step, the losses of all steps as one device tensor)"""
    mt.LIVE_ROWS = bool(on)
    opt.flat_p.copy_(start[0])
    opt.load_state_dict(start[1])
    for p in flat.params:
        torch.autograd.graph.increment_version(p)
    mh.DROPOUT.manual_seed(1000)
    losses = []
    for i in range(args.warmup):
        losses.append(tu.train_step(model, batches[i % 4], opt, None, flat, 1)[0].detach().reshape(()))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(args.steps):
        losses.append(tu.train_step(model, batches[i % 4], opt, None, flat, 1)[0].detach().reshape(()))
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / args.steps * 1e3, torch.stack(losses).float().cpu()


res = {0: [], 1: []}
first = None
same = True
for r in range(args.rounds):
    for on in (0, 1):
        ms, losses = run(on)
        res[on].append(ms)
        first = losses if first is None else first
        same = same and torch.equal(losses, first)
        print("round %d  LIVE_ROWS=%d: %.3f ms/step  (last loss %.9g, %d losses %s the first run's)" % (
            r, on, ms, float(losses[-1]), losses.numel(), "equal" if torch.equal(losses, first) else "DIFFER from"), flush=True)
print("loss sequences of all runs bit-identical: %s" % same)
for on in (0, 1):
    print("LIVE_ROWS=%d: %s  spread %.3f ms" % (on, " / ".join("%.3f" % v for v in res[on]), max(res[on]) - min(res[on])))
print("every on-run below every off-run: %s;  off - on (medians) = %.3f ms" % (
    max(res[1]) < min(res[0]), sorted(res[0])[len(res[0]) // 2] - sorted(res[1])[len(res[1]) // 2]))
