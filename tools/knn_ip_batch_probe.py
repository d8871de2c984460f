"""Probe: inner-product search over a prepared store against its two neighbours, same process, same stores (not part of the
product or the tests).

Legs, ALTERNATED call by call so that drift of the box hits all alike; (b) and (c) swap places every repetition (a, b, c /
a, c, b), so that each follows the long fp32 leg -- and the clock it leaves behind on a power-limited part -- equally often:
    (a) ip_fp32      knn_ip_topk without a prepared store: the fp32 sweeps (what the search did before the prepared form)
    (b) ip_prepared  knn_ip_topk(prepared=...): ac_knn_ip_topk_batch
    (c) l2_prepared  knn_l2_topk(prepared=...): ac_knn_l2_topk_batch, the yardstick (same plan, same launches, one norm term more)
Whole-call times: device events around one call, read after a synchronise; every shape is warmed up first.  Acceptance:
(b) <= (c) x (1 + spread of (c) in this run); (a) / (b) is reported, not gated.

    python tools/knn_ip_batch_probe.py [--reps R] [--shapes 0,1,2,3] [--out DIR]      writes DIR/knn_ip_batch.json, DIR/table.md
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/knn_ip_batch_probe.py --reps 3        (kernel durations, a run of its own)
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

# (queries, rows, dim, k, repetitions at --reps 20: fewer for the big shapes)
SHAPES = [(256, 100_000, 768, 16, 1.0), (1024, 2_000_000, 1024, 32, 0.5), (4096, 10_000_000, 768, 32, 0.25), (16, 10_000_000, 768, 16, 0.5)]

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--shapes", default="0,1,2,3")
ap.add_argument("--out", default=None)
a = ap.parse_args()

nv.require_gpu()
dev = torch.device("cuda:0")
torch.cuda.set_device(dev)
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
results = []
for si in [int(x) for x in a.shapes.split(",")]:
    nq, N, D, k, frac = SHAPES[si]
    reps = max(3, int(round(a.reps * frac)))
    P = ix.synth_unit_rows(N, D, 1, device=dev)
    Q = ix.synth_unit_rows(nq, D, 2, device=dev)
    prep = ix.prepare_store(P, N, D)
    ws = torch.empty(max(ix.knn_workspace_bytes(N, D, nq, k), ix.knn_batch_workspace_bytes(N, D, nq, k), 256), dtype=torch.uint8, device=dev)
    stats = torch.zeros(4, dtype=torch.int32, device=dev)
    out = (torch.empty((nq, k), dtype=torch.float32, device=dev), torch.empty((nq, k), dtype=torch.int64, device=dev))
    legs = {"ip_fp32": lambda: ix.knn_ip_topk(P, N, D, Q, k, out=out, workspace=ws, stats=stats),
            "ip_prepared": lambda: ix.knn_ip_topk(P, N, D, Q, k, out=out, workspace=ws, stats=stats, prepared=prep),
            "l2_prepared": lambda: ix.knn_l2_topk(P, N, D, Q, k, out=out, workspace=ws, stats=stats, prepared=prep)}
    ids = {}
    for _ in range(2):                                       # warm-up of every leg at this shape
        for m, f in legs.items():
            f()
            torch.cuda.synchronize()
            ids[m] = out[1].clone()
    same_ids = bool(torch.equal(ids["ip_fp32"], ids["ip_prepared"]))
    times = {m: [] for m in legs}
    info = {}
    reps += reps & 1                                         # (even: both orders equally often)
    for rep in range(reps):
        for m in (("ip_fp32", "ip_prepared", "l2_prepared") if rep % 2 == 0 else ("ip_fp32", "l2_prepared", "ip_prepared")):
            f = legs[m]
            e0.record()
            f()
            e1.record()
            torch.cuda.synchronize()
            times[m].append(e0.elapsed_time(e1))
            info[m] = {"exact_fallback_queries": int(stats[0].item()), "form": int(stats[1].item())}
    r = {"queries": nq, "rows": N, "dim": D, "k": k, "calls_per_leg": reps, "ip_prepared_ids_equal_ip_fp32": same_ids}
    for m, t in times.items():
        t = np.asarray(t)
        med = float(np.median(t))
        r[m] = dict(info[m], median_ms=med, min_ms=float(t.min()), max_ms=float(t.max()), spread_pct=float((t.max() - t.min()) / med * 100.0))
    r["b_over_c"] = r["ip_prepared"]["median_ms"] / r["l2_prepared"]["median_ms"]
    r["a_over_b"] = r["ip_fp32"]["median_ms"] / r["ip_prepared"]["median_ms"]
    r["margin"] = 1.0 + r["l2_prepared"]["spread_pct"] / 100.0
    r["accepted"] = bool(r["b_over_c"] <= r["margin"])
    results.append(r)
    print(json.dumps(r), flush=True)
    del P, Q, prep, ws, legs
    torch.cuda.empty_cache()

res = {"workload": "whole-call device-event times, legs alternated call by call, synth_unit_rows stores (seed 1) and queries (seed 2)",
       "device": torch.cuda.get_device_name(0), "shapes": results}
if a.out:
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "knn_ip_batch.json"), "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
    names = {"ip_fp32": "(a) IP fp32 sweeps", "ip_prepared": "(b) IP prepared", "l2_prepared": "(c) L2 prepared"}
    with open(os.path.join(a.out, "table.md"), "w") as f:
        f.write("| queries x rows x dim, k | leg | median | min – max | spread | fallbacks | (b)/(c) | margin 1 + spread(c) | (a)/(b) |\n|---|---|---|---|---|---|---|---|---|\n")
        for r in results:
            for m in ("ip_fp32", "ip_prepared", "l2_prepared"):
                x = r[m]
                tail = "| %.4f | %.4f | %.2f |" % (r["b_over_c"], r["margin"], r["a_over_b"]) if m == "ip_prepared" else "| | | |"
                f.write("| %d x %d x %d, %d | %s | %.3f ms | %.3f – %.3f | %.2f %% | %d %s\n" % (
                    r["queries"], r["rows"], r["dim"], r["k"], names[m], x["median_ms"], x["min_ms"], x["max_ms"], x["spread_pct"],
                    x["exact_fallback_queries"], tail))
