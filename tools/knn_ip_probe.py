"""Probe: the inner-product sweep against the L2 sweep, same process, same store (not part of the product or the tests).

Store 10M x 768 fp32 (30.72 GB), 16 resident queries, k = 16: the sweep kernel alone through ac_knn_set_profile_events (HIP
events around the kernel on the call's stream), L2 and IP ALTERNATED launch by launch, medians of REPS launches each after
warm-up.  The yardstick is the L2 sweep measured in this same run; its run-to-run spread is the margin for "IP <= L2".

    python tools/knn_ip_probe.py [--rows N] [--reps R] [--out DIR]        writes DIR/knn_ip_sweep.json
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/knn_ip_probe.py --reps 5      (kernel durations, a run of its own)
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "adaptive-classifier_amd")]
import numpy as np
import torch
from adaptive_classifier import _native as nv
from adaptive_classifier import index as ix

HBM_PEAK_GBS = 8000.0

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=10_000_000)
ap.add_argument("--dim", type=int, default=768)
ap.add_argument("--nq", type=int, default=16)
ap.add_argument("--k", type=int, default=16)
ap.add_argument("--reps", type=int, default=24)
ap.add_argument("--out", default=None)
a = ap.parse_args()

nv.require_gpu()
dev = torch.device("cuda:0")
torch.cuda.set_device(dev)
N, D, nq, k = a.rows, a.dim, a.nq, a.k
P = ix.synth_unit_rows(N, D, 1, device=dev)
Q = ix.synth_unit_rows(nq, D, 2, device=dev)
ws = torch.empty(max(ix.knn_workspace_bytes(N, D, nq, k), 256), dtype=torch.uint8, device=dev)
stats = torch.zeros(4, dtype=torch.int32, device=dev)
out = (torch.empty((nq, k), dtype=torch.float32, device=dev), torch.empty((nq, k), dtype=torch.int64, device=dev))
fns = {"l2": ix.knn_l2_topk, "ip": ix.knn_ip_topk}
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record(); e1.record(); torch.cuda.synchronize()          # materialise the hipEvent handles
for _ in range(3):                                          # warm-up, both kernels
    for f in fns.values():
        f(P, N, D, Q, k, out=out, workspace=ws, stats=stats)
torch.cuda.synchronize()
times = {m: [] for m in fns}
info = {}
nv.lib().ac_knn_set_profile_events(e0.cuda_event, e1.cuda_event)
try:
    for _ in range(a.reps):
        for m, f in fns.items():                            # alternated: drift of the box hits both alike
            f(P, N, D, Q, k, out=out, workspace=ws, stats=stats)
            torch.cuda.synchronize()
            times[m].append(e0.elapsed_time(e1))
            info[m] = {"ring": int(stats[1].item()), "exact_fallback_queries": int(stats[0].item())}
finally:
    nv.lib().ac_knn_set_profile_events(None, None)
bytes_alg = N * D * 4
res = {"workload": "%d x %d fp32 store, %d resident queries, k = %d; sweep kernel alone (HIP events), L2 / IP alternated" % (N, D, nq, k),
       "device": torch.cuda.get_device_name(0), "launches_per_metric": a.reps, "algorithmic_bytes": bytes_alg}
for m, t in times.items():
    t = np.asarray(t)
    med = float(np.median(t))
    res[m] = dict(info[m], median_ms=med, min_ms=float(t.min()), max_ms=float(t.max()),
                  spread_pct=float((t.max() - t.min()) / med * 100.0), GBps=bytes_alg / med / 1e6,
                  frac_of_8TBps=bytes_alg / med / 1e6 / HBM_PEAK_GBS)
res["ip_over_l2_median"] = res["ip"]["median_ms"] / res["l2"]["median_ms"]
line = json.dumps(res)
print(line)
if a.out:
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "knn_ip_sweep.json"), "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
