#!/usr/bin/env python3
"""Matrix-pipe counters per kernel of the encoder forward (bench batch: 256 ragged texts = 5141 rows), for a before / after of
the dead-wave and dead-PV-step removal.

    rocprofv3 --pmc SQ_INSTS_VALU_MFMA_MOPS_BF16 SQ_INSTS_VALU_MFMA_MOPS_F32 SQ_VALU_MFMA_BUSY_CYCLES --output-format csv -d OUT -- \
        python tools/dead_rows_pmc.py --run              (counters only, no tracing in that run; AC_LIBACAMD_PATH = the library)
    python tools/dead_rows_pmc.py --agg OUT -o counters.json
    python tools/dead_rows_pmc.py --ratio parent.json new.json

The forward runs FORWARDS times after one warm-up; the aggregate is the per-launch mean of every counter per kernel name."""
import argparse
import csv
import glob
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORWARDS = 3


def run():
    sys.path[:0] = [ROOT, os.path.join(ROOT, "adaptive-classifier_amd")]
    import torch
    from adaptive_classifier.encoder import HipBertEncoder
    from transformers import BertConfig, BertModel
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    enc = HipBertEncoder(BertModel(BertConfig(), add_pooling_layer=False).eval(), device=dev)
    B, S = 256, 32
    g = torch.Generator().manual_seed(1234)
    ids = torch.randint(1000, 30000, (B, S), generator=g); ids[:, 0] = 101
    lens = torch.randint(8, S + 1, (B,), generator=g); lens[0] = S
    mask = (torch.arange(S)[None, :] < lens[:, None]).to(torch.int64)
    ids = (ids * mask).to(dev); mask = mask.to(dev); types = torch.zeros_like(ids)
    for _ in range(1 + FORWARDS):
        enc.encode_cls(ids, types, mask, verify=False)
    torch.cuda.synchronize()
    print("rows", enc.last_tokens)


def short(name):
    if name.startswith("_Z"):
        name = subprocess.run(["c++filt", name], capture_output=True, text=True, check=True).stdout.strip()
    return re.sub(r"^void |\(anonymous namespace\)::|\(.*$", "", name)


def agg(d, out):
    acc = {}
    for f in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            k = acc.setdefault(short(r["Kernel_Name"]), {}).setdefault(r["Counter_Name"], [0.0, 0])
            k[0] += float(r["Counter_Value"]); k[1] += 1
    res = {k: dict({c: v[0] / v[1] for c, v in cs.items()}, launches_counted=max(v[1] for v in cs.values())) for k, cs in sorted(acc.items())}
    json.dump(res, open(out, "w"), indent=1)
    print("%d kernels -> %s" % (len(res), out))


def ratio(a, b):
    A, B = json.load(open(a)), json.load(open(b))
    for k in A:
        for c in A[k]:
            if c != "launches_counted" and A[k][c] > 0 and k in B and ("mfma" in k or "gemm" in k or "attention" in k):
                print("%-52s %-30s %14.1f -> %14.1f  %+.2f %%" % (k[:52], c, A[k][c], B[k][c], 100 * (B[k][c] / A[k][c] - 1)))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--run", action="store_true")
    ap.add_argument("--agg")
    ap.add_argument("--ratio", nargs=2)
    ap.add_argument("-o")
    a = ap.parse_args()
    if a.run:
        run()
    elif a.agg:
        agg(a.agg, a.o)
    elif a.ratio:
        ratio(*a.ratio)
