"""Probe: the range count over the PREPARED store's fp16 plane (ac_knn_*_range_count_batch + the unchanged fill) against the fp32
route and the top-k search over the same plane (not part of the product or the tests).

Shapes (a fresh process each), both metrics:
  big     10M x 768, 16 queries, radii in the widest gap around rank 32 (~30 hits per query)
  many    1M x 768, 16 queries, radii admitting ~1 % of the rows (from a 20 000-row sample)
  wide    1M x 768, 256 queries, the gap radii again: four passes over the plane against eight over the fp32 rows
Legs, ALTERNATED call by call in one process, HIP events around whole calls, 3 warm-up rounds, 12 repeats, outputs pre-sized:
  (a) fp32   ac_knn_*_range_count + ac_knn_*_range_fill
  (b) plane  ac_knn_*_range_count_batch + the same fill
  (c) topk   ac_knn_*_topk_batch at k = 32 on the same store, for orientation
Recorded per leg: median / min / max, the count and fill medians, d_stats[0] (pairs decided exactly); for (b) the plane GB/s of the
count (plane bytes x passes / count median); per shape the cost of ac_knn_prepare_store, i.e. the break-even number of calls for
preparing a plane from inside a range search.  Gate per shape and metric: (b) below (a) by more than (a)'s own max / min spread.

    python tools/knn_range_batch_probe.py [--out DIR]            spawns the children, writes DIR/knn_range_batch.json
    python tools/knn_range_batch_probe.py --child big|many|wide  one shape in this process (prints one JSON line)
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "adaptive-classifier_amd")]

SHAPES = {"big": (10_000_000, 16), "many": (1_000_000, 16), "wide": (1_000_000, 256)}

ap = argparse.ArgumentParser()
ap.add_argument("--child", choices=sorted(SHAPES), default=None)
ap.add_argument("--rows", type=int, default=None)
ap.add_argument("--dim", type=int, default=768)
ap.add_argument("--reps", type=int, default=12)
ap.add_argument("--out", default=None)
a = ap.parse_args()


def parent():
    res = {}
    for name in ("big", "many", "wide"):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", name, "--dim", str(a.dim), "--reps", str(a.reps)]
        if a.rows:
            cmd += ["--rows", str(a.rows)]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=400)          # a fresh process per shape
        if p.returncode != 0:
            print(p.stdout[-2000:], p.stderr[-4000:], file=sys.stderr)
            raise SystemExit("child %s failed with status %d: nothing further is started" % (name, p.returncode))
        r = res[name] = json.loads(p.stdout.strip().splitlines()[-1])
        for m in ("l2", "ip"):
            f, b = r["fp32_" + m], r["plane_" + m]
            limit = f["median_ms"] * f["min_ms"] / f["max_ms"]
            r["gate_" + m] = {"fp32_median_ms": f["median_ms"], "plane_median_ms": b["median_ms"], "fp32_max_over_min": f["max_ms"] / f["min_ms"],
                              "limit_ms": limit, "met": bool(b["median_ms"] < limit), "plane_over_fp32": b["median_ms"] / f["median_ms"],
                              "prepare_break_even_calls": r["prepare_store_ms"] / max(f["median_ms"] - b["median_ms"], 1e-9)}
        print(name, json.dumps(r), flush=True)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "knn_range_batch.json"), "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


def child():
    import numpy as np
    import torch
    from adaptive_classifier import _native as nv
    from adaptive_classifier import index as ix
    nv.require_gpu()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    L = nv.lib()
    N, nq = SHAPES[a.child]
    N, D, k = a.rows or N, a.dim, 32
    P = ix.synth_unit_rows(N, D, 1, device=dev)
    Q = ix.synth_unit_rows(nq, D, 2, device=dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    prep_ms = []
    for _ in range(3):                                      # the cost a range search would pay to prepare the plane itself
        ev[0].record()
        prepared = ix.prepare_store(P, N, D)
        ev[1].record()
        torch.cuda.synchronize()
        prep_ms.append(ev[0].elapsed_time(ev[1]))
    planes, norms = prepared
    rad = {}
    for m in ("l2", "ip"):
        if a.child == "many":                               # the 1 % quantile of a 20 000-row sample
            if m == "l2":
                d = ((P[:20000, :D].double()[None] - Q.double()[:, None]) ** 2).sum(-1)
                rad[m] = torch.quantile(d, 0.01, dim=1).float().contiguous()
            else:
                d = (P[:20000, :D].double()[None] * Q.double()[:, None]).sum(-1)
                rad[m] = torch.quantile(d, 0.99, dim=1).float().contiguous()
        else:                                               # the fp32 midpoint of the widest gap between ranks 28 .. 36
            v, _ = (ix.knn_ip_topk if m == "ip" else ix.knn_l2_topk)(P, N, D, Q, 40, prepared=prepared)
            v = v.double()
            i = 28 + (v[:, 29:37] - v[:, 28:36]).abs().argmax(dim=1)
            rows = torch.arange(nq, device=dev)
            rad[m] = (0.5 * (v[rows, i] + v[rows, i + 1])).float().contiguous()
    ws_t = torch.empty(max(ix.knn_batch_workspace_bytes(N, D, nq, k), 256), dtype=torch.uint8, device=dev)
    ws_r = torch.empty(ix.knn_range_batch_workspace_bytes(N, D, nq), dtype=torch.uint8, device=dev)    # (its prefix serves the fp32 route)
    assert ws_r.numel() >= ix.knn_range_workspace_bytes(N, D, nq)
    stats = torch.zeros(4, dtype=torch.int32, device=dev)
    out = (torch.empty((nq, k), dtype=torch.float32, device=dev), torch.empty((nq, k), dtype=torch.int64, device=dev))
    lims = torch.empty(nq + 1, dtype=torch.int64, device=dev)
    st = nv.stream_ptr(dev)
    head = (nv.ptr(P), N, P.stride(0), D)
    qargs = (nv.ptr(Q), nq, Q.stride(0))
    bufs, info = {}, {}

    def count(m, plane):
        if plane:
            rc = getattr(L, "ac_knn_%s_range_count_batch" % m)(*head, nv.ptr(planes), nv.ptr(norms), *qargs, nv.ptr(rad[m]), nv.ptr(lims),
                                                                nv.ptr(ws_r), ws_r.numel(), nv.ptr(stats), st)
        else:
            rc = getattr(L, "ac_knn_%s_range_count" % m)(*head, *qargs, nv.ptr(rad[m]), nv.ptr(lims), nv.ptr(ws_r), ws_r.numel(), nv.ptr(stats), st)
        nv.check(rc, "count")

    def fill(m):
        oD, oI = bufs[m]
        nv.check(getattr(L, "ac_knn_%s_range_fill" % m)(*head, *qargs, 0, nv.ptr(lims), oD.numel(), nv.ptr(oD), None, nv.ptr(oI), nv.ptr(ws_r),
                                                         ws_r.numel(), nv.ptr(stats), st), "fill")

    for m in ("l2", "ip"):                                  # sizes the outputs once; the timed calls below never read the host
        for plane in (False, True):
            count(m, plane)
            total = int(lims[-1].item())
            if not plane:
                bufs[m] = (torch.empty(max(total, 1), dtype=torch.float32, device=dev), torch.empty(max(total, 1), dtype=torch.int64, device=dev))
                ref_lims = lims.clone()
            else:
                assert torch.equal(lims, ref_lims), "the two routes disagree"
            decided, ran = int(stats[0].item()), int(stats[2].item())
            fill(m)
            torch.cuda.synchronize()
            info[("plane_" if plane else "fp32_") + m] = {
                "hits_total": total, "hits_per_query_min": int(lims.diff().min().item()), "hits_per_query_max": int(lims.diff().max().item()),
                "pairs_decided_exactly": decided, "stats2": ran, "fill_overflow": int(stats[1].item())}
    legs = {}
    for m in ("l2", "ip"):
        f = ix.knn_ip_topk if m == "ip" else ix.knn_l2_topk
        legs["fp32_" + m] = [lambda m=m: count(m, False), lambda m=m: fill(m)]
        legs["plane_" + m] = [lambda m=m: count(m, True), lambda m=m: fill(m)]
        legs["topk_" + m] = [lambda f=f: f(P, N, D, Q, k, out=out, workspace=ws_t, stats=stats, prepared=prepared)]
    for _ in range(3):                                      # warm-up, every leg
        for steps in legs.values():
            for s in steps:
                s()
    torch.cuda.synchronize()
    times = {n: [] for n in legs}
    for _ in range(a.reps):
        for n, steps in legs.items():                       # alternated: drift of the box hits every leg alike
            ev[0].record()
            steps[0]()
            ev[1].record()
            if len(steps) > 1:
                steps[1]()
            ev[2].record()
            torch.cuda.synchronize()
            times[n].append((ev[0].elapsed_time(ev[2]), ev[0].elapsed_time(ev[1]), ev[1].elapsed_time(ev[2])))
    plane_bytes = ((N + 255) // 256 * 256) * ((D + 63) // 64 * 64) * 2
    res = {"workload": "%d x %d store, %d queries; HIP events around whole calls, legs alternated, 3 warm-ups, %d repeats" % (N, D, nq, a.reps),
           "device": torch.cuda.get_device_name(0), "store_bytes": N * D * 4, "plane_bytes": plane_bytes,
           "workspace_bytes": int(ws_r.numel()), "prepare_store_ms": float(np.median(prep_ms)), "prepare_store_all_ms": prep_ms}
    for n, t in times.items():
        t = np.asarray(t)
        res[n] = {"median_ms": float(np.median(t[:, 0])), "min_ms": float(t[:, 0].min()), "max_ms": float(t[:, 0].max())}
        if len(legs[n]) > 1:
            res[n].update(count_median_ms=float(np.median(t[:, 1])), fill_median_ms=float(np.median(t[:, 2])), **info[n])
        if n.startswith("plane_"):
            passes = (nq + 63) // 64
            res[n].update(plane_passes=passes, plane_GBps=plane_bytes * passes / float(np.median(t[:, 1])) / 1e6)
        if n.startswith("fp32_"):
            passes = (nq + 31) // 32
            res[n].update(store_passes=passes, store_GBps=N * D * 4 * passes / float(np.median(t[:, 1])) / 1e6)
    print(json.dumps(res))


if a.child:
    child()
else:
    parent()
