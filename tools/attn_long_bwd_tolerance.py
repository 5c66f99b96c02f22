"""How much of the bf16 bounds of tests/test_hip_attn_long_bwd.py the number formats alone use (CPU, no GPU needed).

The attention backward from 257 to 512 keys is restated in float64 with every quantity the bf16 route holds in bf16 rounded to bf16
where the streaming MFMA core of csrc/attn_long_bwd.hip (and, for ctx, the streaming forward of csrc/attn_long.hip) rounds it: the
recomputed q | k | v rows, the probabilities that enter the context and dV products, the dS tile that enters the dQ and dK products,
the dq | dk | dv rows, and ctx, dx, d_hist as they leave.  Above 256 keys the q rows are NOT scaled and rounded a second time (the
accumulator takes log2e / 8), so that rounding of the cores below 257 keys is absent here.  The row statistics (max, 1 / sum, D) and
d_head_mask stay fp32 on the device and are not rounded.  Inputs are those of the tests' soft-bias case: the seven shapes, the three
bias forms, head mask (1, 0.5), no dropout.  Each line is the share of a bound this restatement uses against the float64 reference;
if one exceeded half a bound, the INPUT would have to change, not the bound.

    python tools/attn_long_bwd_tolerance.py [--out profiles/attn_long_bwd_tolerance_report.txt]

--drop: the same restatement with the attention-probability dropout of the wide counter layout (modcr_qkv_attn_long_drop_fwd / _bwd),
on the cases of tests/test_hip_attn_long_drop.py: the keep mask m of tests/attn_wide_drop.py clears the bf16 probabilities that enter
the context and D, 1 / (1 - p) multiplies in fp32, dP takes m / (1 - p), the dV operand is bf16(P / (1 - p)) o m.

    python tools/attn_long_bwd_tolerance.py --drop [--out profiles/attn_long_drop_tolerance_report.txt]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p_ in (ROOT, os.path.join(ROOT, "multimodal-context-reasoning_amd"), os.path.join(ROOT, "tests")):
    if p_ not in sys.path:
        sys.path.insert(0, p_)

import test_hip_attn_long_bwd as T  # noqa: E402
import test_hip_attn_prefix_bwd as PF  # noqa: E402


def r16(t):
    return t.float().to(torch.bfloat16).double()


def rounded_restatement(shape, bias, hm, keep=None, pd=0.0, c=None, e=None, post=False):
    """(ctx, dx, d_hist or None, dWqkv, dbqkv, dS, d_hm) of the bf16 route's arithmetic in float64 with its roundings; keep [N, A, S, L]
    (0 / 1) and pd: the attention-probability dropout of the DROP instantiations; c: another case than the shape's;
    e [N, 1, S, L] (zero outside text rows x region keys) and post: the align map's gradient of the DALIGN instantiations -- it joins dP
    in fp32 (under keep / (1 - p) with post) and D through the fp32 exponentials of sweep 1, neither of them a bf16 operand"""
    n, s, p, h, a = shape
    c = T.case(shape) if c is None else c
    w, b, x = (t.double() for t in c[:3])
    hist = c[3].double() if p else torch.zeros(n, 0, h, dtype=torch.float64)
    dctx = c[-1].double()
    F = torch.nn.functional
    qkv = r16(F.linear(x, w, b))                                            # own rows q | k | v
    kvh = r16(F.linear(hist, w[h:], b[h:]))                                 # prefix rows k | v
    sp = lambda t: t.reshape(n, t.shape[1], a, 64).transpose(1, 2)
    q = sp(qkv[..., :h])
    k = sp(torch.cat([kvh[..., :h], qkv[..., h:2 * h]], 1))
    v = sp(torch.cat([kvh[..., h:], qkv[..., 2 * h:]], 1))
    do = sp(dctx)
    P = torch.softmax(q @ k.transpose(-1, -2) / 8.0 + (0.0 if bias is None else bias.double()), -1)
    hmv = hm.double().reshape(n, a, 1, 1)
    back = lambda t: t.transpose(1, 2).reshape(n, t.shape[2], h)
    if keep is None:
        ctx = r16(back(r16(P) @ v * hmv))
        dp = do @ v.transpose(-1, -2)
        dl = (r16(P) @ v * do).sum(-1, keepdim=True)                        # D = dctx . (P.V), P as the context product takes it
        Pv = r16(P)                                                         # the dV operand
    else:
        inv = 1.0 / (1.0 - pd)
        ctx = r16(back((r16(P) * keep) @ v * hmv * inv))                    # dropped bf16 weights cleared, 1 / (1 - p) in fp32
        dp = do @ v.transpose(-1, -2) * keep * inv
        dl = ((r16(P) * keep) @ v * do).sum(-1, keepdim=True) * inv
        Pv = r16(P * inv) * keep
    if e is not None:
        ek = e.double() * (keep / (1.0 - pd) if (post and keep is not None) else 1.0)
        dp = dp + ek
        dl = dl + (P * ek).sum(-1, keepdim=True)
    ds = P * (dp - dl)
    dq = r16(back(r16(ds) @ k * hmv * 0.125))
    dk = r16(back(r16(ds).transpose(-1, -2) @ q * hmv * 0.125))
    dv = r16(back(Pv.transpose(-1, -2) @ do * hmv))
    dqkv = torch.cat([dq, dk[:, p:], dv[:, p:]], -1)                         # [N, S, 3H]
    dkvh = torch.cat([dk[:, :p], dv[:, :p]], -1)                             # [N, P, 2H]
    dx = r16(dqkv @ w)
    dh = r16(dkvh @ w[h:]) if p else None
    dw = dqkv.reshape(-1, 3 * h).t() @ x.reshape(-1, h)
    dw[h:] += dkvh.reshape(-1, 2 * h).t() @ hist.reshape(-1, h)
    db = dqkv.reshape(-1, 3 * h).sum(0)
    db[h:] += dkvh.reshape(-1, 2 * h).sum(0)
    return ctx, dx, dh, dw, db, ds * hmv, dl.sum((-1, -2))


def uses(names, got, ref, shape, tol=2e-2):
    """[(quantity, share of its bound)] of one case, as test_hip_attn_long_bwd.check_all holds them"""
    n, s, p, h, a = shape
    out = []
    for nm, g, r in zip(names, got, ref):
        if r is None:
            continue
        g, r = g.clone(), r.clone()
        if nm == "dbqkv":
            g[h:2 * h] = 0
            r[h:2 * h] = 0
        out.append((nm, float((g - r).abs().max()) / max(1.0, float(r.abs().max())) / tol))
        if nm in ("dx", "d_hist", "dwqkv"):
            out.append((nm + " rel L2", float((g - r).norm() / r.norm()) / 2e-2))
    out.append(("key-bias slice", float(got[4][h:2 * h].abs().max()) / (tol * max(1.0, float(ref[4].abs().max())) * (n * s) ** 0.5 * 0.25)))
    return out


def main_drop(out):
    import attn_wide_drop as W
    import test_hip_attn_long_drop as D
    names = ("ctx", "dx", "d_hist", "dwqkv", "dbqkv", "d_bias", "d_head_mask")
    lines = ["bf16-rounded restatement of the attention backward from 257 to 512 keys UNDER ATTENTION DROPOUT (wide counter layout, p = %g)" % D.DROP[0],
             "against float64 with the same mask (CPU): PREDICTED share of each bound of tests/test_hip_attn_long_drop.py used by the number",
             "formats alone.  max|err| / max(1, max|ref|) against 2e-2; relative L2 against 2e-2; key-bias slice against 2e-2 x scale x",
             "sqrt(N S) / 4; the flat-score case also d_bias element-wise against 2e-2 x max|d_bias| and against 2e-2 x its row's max|d_bias| (no floor of 1).  The chunk-mean case",
             "(2, 320, 0, 256, 4) is not restated: the chunk mean adds no rounding site that the dropout touches.", ""]
    worst = {}
    cases = [(shape, form, None) for shape in D.SHAPES for form in D.FORMS] + [(D.SHAPES[1], "flat scores", D.flat_case(D.SHAPES[1])[0])]
    for shape, form, c in cases:
        n, s, p, h, a = shape
        if c is None:
            bias, hm = D.operands(form, shape)
            ref = D.form_reference(shape, form)
        else:
            bias, hm = torch.zeros(n, a, s, s), torch.ones(n, a)
            ref = D.reference(shape, bias, hm, D.DROP, c=c)
        keep = W.keep_of_call(n, a, s, p, D.DROP).double()
        got = rounded_restatement(shape, bias, hm.expand(n, a), keep, D.DROP[0], c=c)
        row = uses(names, got, ref, shape)
        if c is not None:
            row.append(("d_bias element-wise", float((got[5] - ref[5]).abs().max()) / float(ref[5].abs().max()) / 2e-2))
            row.append(("d_bias / row max", float(((got[5] - ref[5]).abs() / ref[5].abs().amax(-1, keepdim=True)).max()) / 2e-2))
        for nm, use in row:
            worst[nm] = max(worst.get(nm, (0.0, None)), (use, (shape, form)))
        lines.append("%-24s %-11s %s" % (shape, form, "  ".join("%s %4.1f %%" % (nm, 100 * u) for nm, u in row)))
    lines += ["", "worst predicted use of each bound:"]
    for nm, (use, where) in worst.items():
        lines.append("  %-20s %5.1f %%  at %s %s" % (nm, 100 * use, where[0], where[1]))
    top = max(u for u, _ in worst.values())
    lines += ["", "largest predicted share: %.1f %% -- %s" % (100 * top, "below half of every bound: inputs, p and bounds stand" if top < 0.5 else
                                                              "ABOVE HALF A BOUND: reduce that case's p or weight scale")]
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    with open(out, "w") as f:
        f.write(text)


def main_align(out):
    import attn_wide_drop as W
    import test_hip_attn_long_align as A
    names = ("ctx", "dx", "d_hist", "dwqkv", "dbqkv", "d_bias", "d_head_mask")
    lines = ["bf16-rounded restatement of the attention backward from 257 to 512 keys WITH DENSE MASK BITS AND THE ALIGN MAP'S GRADIENT",
             "(modcr_qkv_attn_long_align_bwd; bits as a 0 / -10000 additive mask, d_align ~ N(0, 1), dropout p = %g under the wide counter layout)" % A.DROP[0],
             "against float64 (CPU): PREDICTED share of each bound of tests/test_hip_attn_long_align.py used by the number formats alone.",
             "max|err| / max(1, max|ref|) against 2e-2; relative L2 against 2e-2; key-bias slice against 2e-2 x scale x sqrt(N S) / 4.  Shapes are",
             "(N, S, T, H, A).  The chunk-mean case (2, 320, 64, 256, 4) is not restated: the chunk mean adds no rounding site that the bits or the",
             "align map's gradient touch.  d_align has unit variance in every case.  One case is rescaled, the bound is not: at (1, 258, 257) the first",
             "pass predicted 104.9 - 115.6 % of the d_head_mask bound (a sum of 258 terms of either sign under +-10 scores whose bf16 q | k rows move",
             "every probability by percents), so that case takes flat-score rows (the query projection scaled to a score deviation of 0.4:",
             "tests/test_hip_attn_long_align.py, batch()); the figures below are with those rows.", ""]
    worst = {}
    cases = []
    for shape in A.SHAPES:
        cases += [(shape, "bits phase 1", 1, False, None, False, False), (shape, "bits phase 3", 3, False, None, False, False),
                  (shape, "d_align, soft bias", 0, True, None, False, True),
                  (shape, "bits + d_align p=0.1", 3, False, A.DROP, False, True), (shape, "bits + d_align p=0.1 post", 3, False, A.DROP, True, True)]
    for shape, what, phase, soft, drop, post, align in cases:
        n, s, t, h, a = shape
        hm = T.head_mask(n, a)
        add = A.soft(shape) if soft else A.phase_add(shape, phase)
        ref = A.reference(shape, add, hm, drop=drop, post=post, with_align=align)
        if not soft:
            ref[5] = None
        e = None
        if align:
            e = torch.zeros(n, 1, s, s, dtype=torch.float64)
            e[:, 0, :t, t:] = A.batch(shape)[4].double()
        keep = W.keep_of_call(n, a, s, 0, drop).double() if drop else None
        got = rounded_restatement((n, s, 0, h, a), add, hm, keep, drop[0] if drop else 0.0, c=A.batch(shape)[3], e=e, post=post)
        row = uses(names, got, ref[:7], (n, s, 0, h, a))
        for nm, use in row:
            worst[nm] = max(worst.get(nm, (0.0, None)), (use, (shape, what)))
        lines.append("%-24s %-26s %s" % (shape, what, "  ".join("%s %4.1f %%" % (nm, 100 * u) for nm, u in row)))
    lines += ["", "worst predicted use of each bound:"]
    for nm, (use, where) in worst.items():
        lines.append("  %-20s %5.1f %%  at %s %s" % (nm, 100 * use, where[0], where[1]))
    top = max(u for u, _ in worst.values())
    lines += ["", "largest predicted share: %.1f %% -- %s" % (100 * top, "below every bound: inputs and bounds stand" if top < 1.0 else
                                                              "ABOVE A BOUND: rescale that case's inputs")]
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    with open(out, "w") as f:
        f.write(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--drop", action="store_true", help="the dropout cases of tests/test_hip_attn_long_drop.py")
    ap.add_argument("--align", action="store_true", help="the mask-bits / align-map-gradient cases of tests/test_hip_attn_long_align.py")
    args = ap.parse_args()
    if args.drop:
        return main_drop(args.out or os.path.join(ROOT, "profiles", "attn_long_drop_tolerance_report.txt"))
    if args.align:
        return main_align(args.out or os.path.join(ROOT, "profiles", "attn_long_align_tolerance_report.txt"))
    args.out = args.out or os.path.join(ROOT, "profiles", "attn_long_bwd_tolerance_report.txt")
    lines = ["bf16-rounded restatement of the attention backward from 257 to 512 keys against float64 (CPU): share of each bound of",
             "tests/test_hip_attn_long_bwd.py used by the number formats alone.  Soft-bias case: head mask (1, 0.5), no dropout.",
             "max|err| / max(1, max|ref|) against 2e-2; relative L2 against 2e-2; key-bias slice against 2e-2 x scale x sqrt(N S) / 4.", ""]
    worst = {}
    names = ("ctx", "dx", "d_hist", "dwqkv", "dbqkv", "d_bias", "d_head_mask")
    for shape in T.SHAPES:
        n, s, p, h, a = shape
        for form in T.FORMS:
            bias = PF.bias_of(form, n, s, p, a, s + p)
            ref = T.soft_reference(shape, form)
            got = rounded_restatement(shape, bias, T.head_mask(n, a))
            row = []
            for nm, g, r in zip(names, got, ref):
                if r is None:
                    continue
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
