#!/usr/bin/env python3
"""Record which kernel every case of tests/gemm_dispatch_cases.py launches, with its grid, block and an output hash.

  1. on the GPU, one fresh process under a kernel trace (kernel trace only, no counters):
         rocprofv3 --kernel-trace --output-format csv -d OUT -- python tools/gemm_dispatch_probe.py --run OUT/run.json
     AC_LIBACAMD_PATH selects the library (the parent commit's build for the committed fixture).
  2. anywhere:
         python tools/gemm_dispatch_probe.py --merge OUT/run.json OUT/**/*_kernel_trace.csv -o tests/data/gemm_dispatch_parent.json
     Every case is one call of a public entry, i.e. one GEMM kernel launch or a refusal, so the i-th GEMM kernel of the trace (by
     start time) belongs to the i-th case that returned 0.
  3. --compare A.json B.json: kernel names, grids and blocks (and hashes) of two recordings, case by case.
"""
import argparse
import csv
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "adaptive-classifier_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

GEMM_KERNEL = re.compile(r"\bgemm_(smallm_nt|fewtiles_nt|pipe_nt|planes_nt|split_nt|tile_nt|direct)\b")


def run(out):
    os.environ.setdefault("AC_TEST_HOOKS", "1")
    import torch
    from adaptive_classifier import _native as nv
    from gemm_dispatch_cases import CASES, run_case
    dev = torch.device("cuda:0")
    rec = {"cus": nv.device_info()["cus"], "cases": []}
    for c in CASES:
        rc, sha = run_case(nv, dev, c)
        rec["cases"].append(dict(c, rc=rc, sha256=sha))
        print("%-36s rc %d %s" % (c["id"], rc, (sha or "")[:16]), flush=True)
    with open(out, "w") as f:
        json.dump(rec, f, indent=1)


def demangle(name):
    if name.startswith("_Z"):
        name = subprocess.run(["c++filt", name], capture_output=True, text=True, check=True).stdout.strip()
    return re.sub(r"^void |\(anonymous namespace\)::|\(.*$", "", name)          # "gemm_planes_nt<1, 2, true, false, 2>"


def merge(run_json, traces, out):
    rec = json.load(open(run_json))
    rows = [r for t in traces for r in csv.DictReader(open(t)) if GEMM_KERNEL.search(demangle(r["Kernel_Name"]))]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    ok = [c for c in rec["cases"] if c["rc"] == 0]
    assert len(rows) == len(ok), "%d GEMM kernels in the trace for %d cases that ran" % (len(rows), len(ok))
    for c, r in zip(ok, rows):
        block = [int(r["Workgroup_Size_X"]), int(r["Workgroup_Size_Y"]), int(r["Workgroup_Size_Z"])]
        c["kernel"] = demangle(r["Kernel_Name"])
        c["block"] = block                                                      # (the trace gives the grid in work-items)
        c["grid"] = [int(r["Grid_Size_X"]) // block[0], int(r["Grid_Size_Y"]) // block[1], int(r["Grid_Size_Z"]) // block[2]]
    with open(out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("%d cases, %d kernels -> %s" % (len(rec["cases"]), len(rows), out))


def compare(a, b):
    A, B = json.load(open(a)), json.load(open(b))
    bad = 0
    if A["cus"] != B["cus"]:
        print("CU counts differ: %d and %d" % (A["cus"], B["cus"]))
        bad += 1
    for x, y in zip(A["cases"], B["cases"]):
        for k in ("id", "rc", "kernel", "grid", "block", "sha256"):
            if x.get(k) != y.get(k):
                print("%s: %s %r != %r" % (x["id"], k, x.get(k), y.get(k)))
                bad += 1
    print("%d cases compared, %d differences" % (min(len(A["cases"]), len(B["cases"])), bad + abs(len(A["cases"]) - len(B["cases"]))))
    return 1 if bad or len(A["cases"]) != len(B["cases"]) else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--run")
    ap.add_argument("--merge", nargs="+")
    ap.add_argument("--compare", nargs=2)
    ap.add_argument("-o")
    a = ap.parse_args()
    if a.run:
        run(a.run)
    elif a.merge:
        merge(a.merge[0], a.merge[1:], a.o)
    elif a.compare:
        sys.exit(compare(*a.compare))
