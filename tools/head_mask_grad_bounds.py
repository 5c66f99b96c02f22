"""How much of the bf16 bound of tests/test_hip_attn_head_mask_bwd.py the number formats alone use for d_head_mask (CPU, no GPU).

The head-mask gradient d_hm[n, a] = sum_i sum_j P'_ij (dctx_i . v_j), P' = P o m / (1 - p), is restated in float64 with the
recomputed q | k | v rows, the scaled queries and P' rounded to bf16 (more than the MFMA core of csrc/attn_bias_bwd.hip rounds: it
keeps P in fp32 for this sum) and compared with the float64 autograd reference of the tests, the head mask a leaf.  Inputs are the
tests' own: the seven shapes of test_shapes_and_cores with their soft bias and head mask, without and with dropout p = 0.2, and the
head-at-zero cases.  Each line: max|ref|, the restatement's max|err| / max(1, max|ref|), its share of the 2e-2 bound; for the
head-at-zero cases also the zeroed heads' reference values (the test asserts max|.| > 0.5).

    python tools/head_mask_grad_bounds.py [--out profiles/attn_head_mask_bwd_tolerance_report.txt]
The GPU run's report_use lines are appended to that file by hand (MODCR_TEST_REPORT=1 pytest -s tests/test_hip_attn_head_mask_bwd.py).
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p_ in (ROOT, os.path.join(ROOT, "multimodal-context-reasoning_amd"), os.path.join(ROOT, "tests")):
    if p_ not in sys.path:
        sys.path.insert(0, p_)

import helpers as H  # noqa: E402
import test_hip_attn_head_mask_bwd as T  # noqa: E402
from test_hip_attn_bias import soft_bias  # noqa: E402

LOG2E = 1.44269504088896340736


def r16(t):
    return t.float().to(torch.bfloat16).double()


def rounded_d_hm(shape, bias, drop):
    """d_hm [N, A] of the bf16 route's arithmetic in float64 with its roundings (and P' rounded on top)"""
    n, s, p, h, a = shape
    c = [t.double() for t in T.case(shape)]
    w, b, x, dctx = c[0], c[1], c[2], c[-1]
    F = torch.nn.functional
    rows = torch.cat([c[3], x], 1) if p else x
    q = r16(r16(F.linear(x, w[:h], b[:h])) * (0.125 * LOG2E))
    k, v = r16(F.linear(rows, w[h:2 * h], b[h:2 * h])), r16(F.linear(rows, w[2 * h:], b[2 * h:]))
    sp = lambda t: t.reshape(n, t.shape[1], a, 64).transpose(1, 2)
    P = torch.softmax(sp(q) @ sp(k).transpose(-1, -2) / LOG2E + bias.double(), -1)
    if drop is not None:
        pd, seed, off = drop
        P = P * H.attn_drop_keep_torch(range(n), a, s, pd, seed, off, "cpu", keys=p + s).double() / (1.0 - pd)
    return (r16(P) * (sp(dctx) @ sp(v).transpose(-1, -2))).sum((2, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attn_head_mask_bwd_tolerance_report.txt"))
    args = ap.parse_args()
    lines = ["bf16-rounded restatement of d_head_mask against float64 (CPU): share of the 2e-2 bound of",
             "tests/test_hip_attn_head_mask_bwd.py used by the number formats alone (q | k | v, the scaled q and P' rounded to bf16).", ""]
    worst = (0.0, None)
    for shape in T.SHAPES:
        for dk in T.DROPS:
            bias, hm, ref = T.soft_case(shape, dk)
            got = rounded_d_hm(shape, bias, T.DROPS[dk])
            scale = max(1.0, float(ref[6].abs().max()))
            use = float((got - ref[6]).abs().max()) / scale
            worst = max(worst, (use, (shape, dk)))
            lines.append("%-24s %-6s max|ref| %6.1f   err / scale %.2e   %4.1f %% of 2e-2" % (shape, dk, float(ref[6].abs().max()), use, 100 * use / 2e-2))
    lines += ["", "a head at 0 (test_a_head_at_zero_keeps_its_gradient): the zeroed heads' reference gradients"]
    for shape in (T.SHAPES[1], T.SHAPES[3], T.SHAPES[5], T.SHAPES[6]):
        n, s, p, h, a = shape
        rs = np.random.RandomState(23 + s)
        bias = soft_bias(rs, (n, 1, s, p + s))
        hm = torch.from_numpy(rs.uniform(0.25, 1.0, size=(n, a)).astype(np.float32))
        hm[:, 0] = 0.0
        ref = T.reference(shape, bias, hm)[6]
        got = rounded_d_hm(shape, bias, None)
        use = float((got - ref).abs().max()) / max(1.0, float(ref.abs().max()))
        worst = max(worst, (use, (shape, "head 0 at 0")))
        lines.append("%-24s max|ref| %6.1f   err / scale %.2e   %4.1f %% of 2e-2   head 0: %s" %
                     (shape, float(ref.abs().max()), use, 100 * use / 2e-2, ", ".join("%.2f" % v for v in ref[:, 0].tolist())))
    lines += ["", "largest share: %.1f %% of the bound (%.2e against 2e-2) at %s %s" % (100 * worst[0] / 2e-2, worst[0], worst[1][0], worst[1][1])]
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
