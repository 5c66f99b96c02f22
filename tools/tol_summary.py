#!/usr/bin/env python
"""Condense `MODCR_TEST_REPORT=1 python -m pytest tests -q -m gpu -s` (one `[tol]` line per tolerance check, tests/helpers.py) into
profiles/rNN_tolerance_report*.txt: per test function and bound the worst observed use, then every check.
`[tol-k]` lines (tests/test_hip_head_attn.py: one per test, every quantity family's use of its k, fp32 yardstick and use of its
ceiling) are condensed per test function and family, then listed.
usage: tol_summary.py <pytest output> <report file> [title]"""
import re
import sys
from collections import OrderedDict


def main(src, dst, title):
    lines = [l.rstrip("\n") for l in open(src, errors="replace")]
    tol = [l for l in lines if "[tol]" in l]
    tail = [l for l in lines if re.search(r"\d+ passed", l)]
    pat = re.compile(r"\[tol\]\s+(\S+)\s+(.*?)\s+(max\|err\|/scale|relative L2)\s+([0-9.e+-]+)\s+bound\s+([0-9.e+-]+)\s+used\s+(\d+)\s*%")
    groups = OrderedDict()
    for l in tol:
        m = pat.search(l)
        if not m:
            continue
        test, what, kind, err, bound, _ = m.groups()
        fn = test.split("[")[0]
        key = (fn, float(bound), kind)
        g = groups.setdefault(key, [0.0, "", 0])
        g[2] += 1
        if float(err) >= g[0]:
            g[0], g[1] = float(err), what.strip()
    with open(dst, "w") as fh:
        fh.write(title + "\n")
        if not tol:             # a file of [tol-k] lines only (tests/test_hip_head_attn.py)
            fh.write("command: MODCR_TEST_REPORT=1 python -m pytest <the file> -q -m gpu -s   (%s; one [tol-k] line per test)\n"
                     "convention: element-wise |got - ref| <= min(k * max(yardstick, eps32 * scale), ceiling * scale) + half an output ulp "
                     "(the test file's docstring)\n" % (tail[-1].strip(" =") if tail else "?"))
            wall = re.search(r"in ([0-9.]+s)", tail[-1]) if tail else None
            fh.write("wall time of the file: %s\n" % (wall.group(1) if wall else "?"))
        else:
            fh.write("command: MODCR_TEST_REPORT=1 python -m pytest tests -q -m gpu -s   (%s; one [tol] line per check, %d checks)\n"
                     % (tail[-1].strip(" =") if tail else "?", len(tol)))
            fh.write("convention: every max|err| check is  max|got - ref| <= bound * max(1, max|ref|);  gradient checks marked 'relative L2' are "
                     "|got - ref|_2 / |ref|_2 <= bound.\nContract bounds (north_star): 1e-3 fp32, 2e-2 bf16.  Bounds above 2e-2 are deep-stack / "
                     "gradient bounds, each <= ~2x its worst observed use.\n\n== per test function and bound: worst use ==\n")
            for (fn, bound, kind), (err, what, n) in sorted(groups.items(), key=lambda kv: -kv[1][0] / kv[0][1]):
                fh.write("  %3.0f%%  %-62s bound %.1e %-14s worst %.2e (%s) checks=%d\n" % (100.0 * err / bound, fn, bound, kind, err, what, n))
        kpat = re.compile(r"(.*?): k-use ([0-9.e+-]+) yardstick/scale ([0-9.e+-]+) ceiling-use ([0-9.e+-]+)")
        klines = [l[l.index("[tol-k]") + 7:].strip() for l in lines if "[tol-k]" in l]
        fams = OrderedDict()
        for l in klines:
            parts = l.split(" | ")
            for seg in parts[1:]:
                m = kpat.match(seg)
                g = fams.setdefault((parts[0].split("[")[0], m.group(1)), [0.0, "", 0.0, 0.0, 0])
                use, yard, ceil = (float(m.group(i)) for i in (2, 3, 4))
                if use >= g[0]:
                    g[0], g[1] = use, parts[0]
                g[2], g[3], g[4] = max(g[2], yard), max(g[3], ceil), g[4] + 1
        if fams:
            fh.write("\n== per test function and quantity family: worst use of k = (|err| - ulp/2) / max(yardstick, eps32 * scale), largest fp32 "
                     "yardstick / scale, worst (|err| - ulp/2) / (ceiling * scale) ==\n")
            for (fn, fam), (use, tid, yard, ceil, n) in sorted(fams.items(), key=lambda kv: -kv[1][0]):
                fh.write("  k-use %6.3f  yardstick/scale %.2e  ceiling-use %.4f  %-12s checks=%-4d %s\n" % (use, yard, ceil, fam, n, tid))
            fh.write("\n== every test (family: k-use yardstick/scale ceiling-use) ==\n")
            for l in klines:
                fh.write("  " + l.replace("k-use ", "").replace("yardstick/scale ", "").replace("ceiling-use ", "") + "\n")
        if tol:
            fh.write("\n== every check ==\n")
        for l in tol:
            fh.write(l[l.index("[tol]") - 2:] + "\n" if l.index("[tol]") >= 2 else l + "\n")


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else "Tolerance use of the GPU parity suite")
