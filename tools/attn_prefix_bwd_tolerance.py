"""How much of the bf16 bounds of tests/test_hip_attn_prefix_bwd.py the number formats alone use (CPU, no GPU needed).

The attention backward with prefix rows is restated in float64 with every quantity the bf16 route holds in bf16 rounded to bf16
where the MFMA core of csrc/attn_bias_bwd.hip rounds it: the recomputed q | k | v rows, the scaled queries, the probabilities
P'' and the dS tile that enter the dV / dK / dQ products, the dq | dk | dv rows, and dx / d_hist as they leave their GEMMs (above
192 keys the exact core keeps fp32 rows: only dx and d_hist are rounded).  Inputs are those of the tests' soft-bias case: the six
shapes, the three bias forms, head mask (1, 0.5), p = 0.2.  Each line is the share of a bound this restatement uses against the
float64 reference; if one exceeded half a bound, the INPUT would have to change, not the bound.

    python tools/attn_prefix_bwd_tolerance.py [--out profiles/attn_prefix_bwd_tolerance_report.txt]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p_ in (ROOT, os.path.join(ROOT, "multimodal-context-reasoning_amd"), os.path.join(ROOT, "tests")):
    if p_ not in sys.path:
        sys.path.insert(0, p_)

import helpers as H  # noqa: E402
import test_hip_attn_prefix_bwd as T  # noqa: E402

LOG2E = 1.44269504088896340736


def r16(t):
    return t.float().to(torch.bfloat16).double()


def rounded_restatement(c, a, bias, hm, drop):
    """(ctx, dx, d_hist, dWqkv, dbqkv, dS) of the bf16 route's arithmetic in float64 with its roundings"""
    w, b, x, hist, dctx = (t.double() for t in c)
    n, s, h = x.shape
    p = hist.shape[1]
    l = p + s
    mfma = l <= 192
    rr = r16 if mfma else (lambda t: t)
    F = torch.nn.functional
    qkv = rr(F.linear(x, w, b))                                             # own rows q | k | v
    kvh = rr(F.linear(hist, w[h:], b[h:]))                                  # prefix rows k | v
    sp = lambda t: t.reshape(n, t.shape[1], a, 64).transpose(1, 2)
    q = sp(rr(qkv[..., :h] * (0.125 * LOG2E))) if mfma else sp(qkv[..., :h]) * (0.125 * LOG2E)
    k = sp(torch.cat([kvh[..., :h], qkv[..., h:2 * h]], 1))
    v = sp(torch.cat([kvh[..., h:], qkv[..., 2 * h:]], 1))
    do = sp(dctx)
    sc = q @ k.transpose(-1, -2) / LOG2E + bias.double()
    P = torch.softmax(sc, -1)
    pd, seed, off = drop
    mk = H.attn_drop_keep_torch(range(n), a, s, pd, seed, off, "cpu", keys=l).double() / (1.0 - pd)
    hmv = hm.double().reshape(1, a, 1, 1)
    back = lambda t: t.transpose(1, 2).reshape(n, t.shape[2], h)
    ctx = r16(back(rr(P * mk) @ v * hmv))
    dp = (do @ v.transpose(-1, -2)) * mk
    dl = (P * dp).sum(-1, keepdim=True)
    ds = P * (dp - dl)
    dq = rr(back(rr(ds) @ k * hmv * 0.125))
    dk = rr(back(rr(ds).transpose(-1, -2) @ (q / LOG2E) * hmv))
    dv = rr(back(rr(P * mk).transpose(-1, -2) @ do * hmv))
    dqkv = torch.cat([dq, dk[:, p:], dv[:, p:]], -1)                         # [N, S, 3H]
    dkvh = torch.cat([dk[:, :p], dv[:, :p]], -1)                             # [N, P, 2H]
    dx = r16(dqkv @ w)
    dh = r16(dkvh @ w[h:])
    dw = dqkv.reshape(-1, 3 * h).t() @ x.reshape(-1, h)
    dw[h:] += dkvh.reshape(-1, 2 * h).t() @ hist.reshape(-1, h)
    db = dqkv.reshape(-1, 3 * h).sum(0)
    db[h:] += dkvh.reshape(-1, 2 * h).sum(0)
    return ctx, dx, dh, dw, db, ds * hmv


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attn_prefix_bwd_tolerance_report.txt"))
    args = ap.parse_args()
    lines = ["bf16-rounded restatement of the attention backward with prefix rows against float64 (CPU): share of each bound of",
             "tests/test_hip_attn_prefix_bwd.py used by the number formats alone.  Soft-bias case: head mask (1, 0.5), p = 0.2.",
             "max|err| / max(1, max|ref|) against 2e-2; relative L2 against 2e-2; key-bias slice against 2e-2 x scale x sqrt(N S) / 4.", ""]
    worst = {}
    names = ("ctx", "dx", "d_hist", "dwqkv", "dbqkv", "d_bias")
    for shape in T.SHAPES:
        n, s, p, h, a = shape
        for form in T.FORMS:
            bias = T.bias_of(form, n, s, p, a, s + p)
            hm = torch.linspace(1.0, 0.5, a)
            ref = T.soft_reference(shape, form)
            got = rounded_restatement(T.case(*shape), a, bias, hm, T.DROP)
            row = []
            for nm, g, r in zip(names, got, ref):
                g, r = g.clone(), r.clone()
                if nm == "dbqkv":
                    g[h:2 * h] = 0
                    r[h:2 * h] = 0
                use = float((g - r).abs().max()) / max(1.0, float(r.abs().max())) / 2e-2
                row.append("%s %4.1f %%" % (nm, 100 * use))
                worst[nm] = max(worst.get(nm, (0.0, None)), (use, (shape, form)))
                if nm in ("dx", "d_hist", "dwqkv"):
                    rel = float((g - r).norm() / r.norm()) / 2e-2
                    row.append("%s L2 %4.1f %%" % (nm, 100 * rel))
                    worst[nm + " rel L2"] = max(worst.get(nm + " rel L2", (0.0, None)), (rel, (shape, form)))
            kb = float(got[4][h:2 * h].abs().max()) / (2e-2 * max(1.0, float(ref[4].abs().max())) * (n * s) ** 0.5 * 0.25)
            row.append("key-bias %4.1f %%" % (100 * kb))
            worst["key-bias slice"] = max(worst.get("key-bias slice", (0.0, None)), (kb, (shape, form)))
            lines.append("%-24s %-10s %s" % (shape, form, "  ".join(row)))
    lines.append("")
    lines.append("worst use of each bound:")
    for nm, (use, where) in worst.items():
        err = use * 2e-2
        lines.append("  %-16s %5.1f %%  (%.2e against 2e-2%s)  at %s %s" % (nm, 100 * use, err, "" if nm != "key-bias slice" else " x its scale", where[0], where[1]))
    top = max(u for u, _ in worst.values())
    lines.append("")
    lines.append("largest share: %.1f %% -- %s" % (100 * top, "below half of every bound: inputs and bounds stand" if top < 0.5 else "ABOVE HALF A BOUND: change the input"))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
