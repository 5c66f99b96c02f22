"""Launch every case of tests/test_hip_gemm_routes.py's route table once and record the route modcr_linear_route reported;
`--check` then matches the records against a rocprofv3 kernel trace of the run (kernel name and template arguments).

    rocprofv3 --kernel-trace --stats -d OUT -o trace -- python tools/gemm_route_trace.py OUT/routes.json
    python tools/gemm_route_trace.py --check OUT/routes.json OUT/.../trace_kernel_trace.csv
"""
import csv
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "multimodal-context-reasoning_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

RES_CODE = {None: 0, "bf16": 1, "f32": 2}
OUT_CODE = {"bf16": 0, "f32": 1, "f16": 2}
TILES = {"ring128": (128, 128), "ring192": (192, 256), "ring256": (256, 256)}


def record(path):
    import torch
    import test_hip_gemm_routes as T
    rows = []
    for c in T.CASES:
        ops = T.Operands(c)
        r = ops.route()
        ops.run()
        torch.cuda.synchronize()
        ops.free()
        torch.cuda.empty_cache()
        rows.append({"id": c.id, "act": c.act, "res": RES_CODE[c.res], "out": OUT_CODE[c.out], "route": r._asdict()})
        print("%-34s %s" % (c.id, r))
    with open(path, "w") as f:
        json.dump(rows, f, indent=1)


def expected(row):
    """(kernel base name, template integers) of the launch a record's route implies"""
    r, a = row["route"], [row["act"], row["res"], row["out"]]
    if r["kernel"] in TILES:
        return "linear_bf16_kernel", list(TILES[r["kernel"]]) + a
    if r["kernel"] == "p8":
        return "linear_bf16_p8_kernel", a + [r["direct"], 0, r["spec"]]
    if r["kernel"] == "t192":
        return "linear_bf16_t192_kernel", a + [r["direct"]]
    raise ValueError(r)


def check(routes, trace):
    rows = json.load(open(routes))
    launches = []
    with open(trace) as f:
        for k in csv.DictReader(f):
            m = re.search(r"(linear_bf16(?:_p8|_t192)?_kernel)<(.*)>\(", k["Kernel_Name"])
            if m:
                ints = [int(v) for v in re.findall(r"(?<![\w.])-?\d+(?![\w.])", m.group(2))]
                if m.group(1) == "linear_bf16_kernel":
                    ints = ints[:2] + ints[-3:]          # Tile<BM, BN, ...>, ACT, RES, OUT
                launches.append((int(k["Start_Timestamp"]), m.group(1), ints))
    launches.sort()
    assert len(launches) == len(rows), "%d GEMM launches in the trace, %d cases" % (len(launches), len(rows))
    bad = 0
    for row, (_, name, ints) in zip(rows, launches):
        want = expected(row)
        ok = want == (name, ints)
        bad += not ok
        print("%-4s %-34s route %-60s kernel %s<%s>" % ("ok" if ok else "BAD", row["id"], row["route"], name, ", ".join(map(str, ints))))
    print("%d cases, %d mismatches" % (len(rows), bad))
    return bad == 0


if __name__ == "__main__":
    if sys.argv[1] == "--check":
        sys.exit(0 if check(sys.argv[2], sys.argv[3]) else 1)
    record(sys.argv[1])
