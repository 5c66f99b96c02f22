"""Run every row of tests/test_attn_route_host.py's route table (N = 2) through the parent commit's product library and through
this tree's on the same seeded inputs; compare the return code, the message and every output; record the route
modcr_qkv_attn_route reported.  `--check` then matches the records against a rocprofv3 kernel trace of the run: the attention and
concat kernels come in equal parent / new pairs, and each pair is the launch the recorded route implies.

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o trace -- python tools/attn_route_trace.py --parent-lib PATH OUT/routes.json
    python tools/attn_route_trace.py --check OUT/routes.json OUT/.../trace_kernel_trace.csv

ctx, probs, lse and the q|k|v dump must agree bit for bit; align_map, a float atomic sum of one term per head, to within
2 (A - 1) 2^-24 relative (the bound on any two summation orders of A terms).
"""
import csv
import ctypes
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "multimodal-context-reasoning_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

KERNELS = "qkv_attn_bf16_kernel|qkv_attn4_kernel|attn_long_bf16_kernel|attn_long_f32_kernel|attn_f32_kernel|concat_prefix_kernel"


def record(parent_path, path):
    import torch
    import modcr_hip as mh
    import test_attn_route_host as T
    assert os.path.abspath(parent_path) != os.path.abspath(mh.LIB_PATH)
    parent, new = ctypes.CDLL(parent_path), mh.lib()
    assert not hasattr(parent, "modcr_qkv_attn_route"), "--parent-lib is not the parent commit's library"
    rows, bad = [], 0
    for i, (kw, want, rule) in enumerate(T.ROUTES):
        r = T.route_of_call(mh, kw)
        c = T.Case(mh, kw, 100 + i)
        rc0, msg0, out0 = c.call(parent, mh)
        rc1, msg1, out1 = c.call(new, mh)
        problems = []
        if (rc0, msg0) != (rc1, msg1):
            problems.append("parent (%d, %r) != new (%d, %r)" % (rc0, msg0, rc1, msg1))
        if (rc1, msg1) != (r.rc, r.message):
            problems.append("the query said (%d, %r), the call (%d, %r)" % (r.rc, r.message, rc1, msg1))
        if rc1 == 0:
            a = kw["a"]
            for name in ("ctx", "probs", "lse", "dump"):
                if out1[name] is not None and not torch.equal(out0[name].view(torch.uint8), out1[name].view(torch.uint8)):
                    problems.append("%s differs" % name)
            assert bool(torch.isfinite(out1["ctx"].float()).all()) and float(out1["ctx"].float().abs().max()) > 0
            if out1["align_map"] is not None:
                m0, m1 = out0["align_map"].double(), out1["align_map"].double()
                tol = 2 * (a - 1) * 2.0 ** -24
                if not bool(((m0 - m1).abs() <= tol * torch.maximum(m0.abs(), m1.abs())).all()):
                    problems.append("align_map differs by more than %.3g relative" % tol)
        bad += bool(problems)
        rows.append({"kw": kw, "rc": r.rc, "family": r.family, "inst": r.inst, "concat": r.concat, "problems": problems})
        print("%-4s %-90s %s %s" % ("BAD" if problems else "ok", kw, (r.family, r.inst, r.concat) if r.rc == 0 else (r.rc, r.message), problems or ""))
        del c, out0, out1
        torch.cuda.empty_cache()
    # the coverage condition: every distinct answer of the CPU table was launched (the table is run whole), the refused calls too
    answers = {(row["family"], tuple(row["inst"] or ()), row["concat"]) for row in rows if row["rc"] == 0}
    table = {w for _, w, _ in T.ROUTES if not isinstance(w[0], int)}
    assert answers == table, answers ^ table
    assert sum(row["rc"] != 0 for row in rows) == sum(isinstance(w[0], int) for _, w, _ in T.ROUTES)
    with open(path, "w") as f:
        json.dump(rows, f, indent=1)
    print("%d cases, %d distinct routes, %d refused, %d with problems" % (len(rows), len(answers), sum(row["rc"] != 0 for row in rows), bad))
    return bad == 0


def expected(row):
    """the attention (and concat) launches a record's route implies: [(kernel base name, template integers)]"""
    kw, inst = row["kw"], row["inst"]
    drop = kw.get("attn_p", 0.0) > 0
    if row["family"] == "tile":
        k = ("qkv_attn_bf16_kernel", list(inst))
    elif row["family"] == "tile4":
        mode, lp, nh = inst[:3]
        k = ("qkv_attn4_kernel", [mode, lp, int(drop and mode != 0), nh, int(bool(kw.get("dump")) and nh == 2 and mode != 0 and lp != 256)])
    elif row["family"] == "long_bf16":
        k = ("attn_long_bf16_kernel", [int(bool(kw.get("probs") or kw.get("align_t"))), inst[0]])
    elif row["family"] == "long_f32":
        k = ("attn_long_f32_kernel", [int(inst[0] != 0)])
    else:
        k = ("attn_f32_kernel", [])
    return ([("concat_prefix_kernel", [])] if row["concat"] else []) + [k]


def check(routes, trace):
    rows = [r for r in json.load(open(routes)) if r["rc"] == 0]
    launches = []
    with open(trace) as f:
        for k in csv.DictReader(f):
            m = re.search(r"(%s)(?:<(.*?)>)?\(" % KERNELS, k["Kernel_Name"]) or re.search(r"(%s)(?:<(.*?)>)?$" % KERNELS, k["Kernel_Name"])
            if m:
                args = (m.group(2) or "").replace("true", "1").replace("false", "0")
                launches.append((int(k["Start_Timestamp"]), m.group(1), [int(v) for v in re.findall(r"(?<![\w.])-?\d+(?![\w.])", args)]))
    launches = [(name, ints) for _, name, ints in sorted(launches)]
    bad, at = 0, 0
    for row in rows:
        want = expected(row)
        got_parent, got_new = launches[at:at + len(want)], launches[at + len(want):at + 2 * len(want)]
        at += 2 * len(want)
        ok = got_parent == got_new == want
        bad += not ok
        print("%-4s %-90s %s" % ("ok" if ok else "BAD", row["kw"], want if ok else "want %s parent %s new %s" % (want, got_parent, got_new)))
    if at != len(launches):
        print("BAD  %d attention / concat launches in the trace, the records imply %d" % (len(launches), at))
        bad += 1
    print("%d launching cases, %d mismatches" % (len(rows), bad))
    return bad == 0


if __name__ == "__main__":
    if sys.argv[1] == "--check":
        sys.exit(0 if check(sys.argv[2], sys.argv[3]) else 1)
    assert sys.argv[1] == "--parent-lib", __doc__
    sys.exit(0 if record(sys.argv[2], sys.argv[3]) else 1)
