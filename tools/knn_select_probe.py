"""Probe: the filtered top-k search (ac_knn_*_topk_sel / _ids) against the unfiltered search on the same store (not part of the
product or the tests).

  gate      10M x 768 fp32 (30.72 GB), 16 queries, k = 32, both metrics: ac_knn_*_topk_sel with an ALL-ONES bitmap against
            ac_knn_*_topk_x, legs ALTERNATED in one process, HIP events around whole calls, 3 warm-up rounds, medians of the
            repeats.  AC_KNN_RING is read once per process, so both forms of the sweep (as shipped: knn_sweep_ring;
            AC_KNN_RING=0: knn_sweep<1>) run in a child process each.  Gate: the filtered median <= the unfiltered median of the
            same process times that leg's own max / min spread.
            Recorded next to it (no gate): a 50 % and a 1 % random selection, one block of 100 000 rows, and the id-list route
            at M = 1000 and 8192.
  many      256 queries x 1M x 768, a 50 % selection (the fp32 sweep once per 32-query tile) next to the unfiltered search over
            the prepared fp16 plane: what the missing plane form costs.

  batch     (--suite batch) the filtered search over the PREPARED store, 1M x 768, k = 32, both metrics, in one process per
            query count: 256 queries -- ac_knn_*_topk_batch against ac_knn_*_topk_batch_sel at all ones, 50 %, 1/8, 1/32, 1 % and
            one block of 100 000 rows, and ac_knn_*_topk_sel (fp32 rows) at 50 %; 16 queries -- the plane form against the
            filtered fp32 sweep at all ones and 50 %.  d_stats[0] (queries answered by the fp64 fallback) per leg.  Gates: all
            ones <= unfiltered x its own max / min; 50 % prepared < 50 % fp32; d_stats[0] == 0 at densities >= 1/32.

    python tools/knn_select_probe.py [--out DIR]                 spawns the children, writes DIR/knn_select.json
    python tools/knn_select_probe.py --suite batch [--out DIR]   the prepared-store legs, writes DIR/knn_select_batch.json
    python tools/knn_select_probe.py --child gate|many           one configuration in this process (prints one JSON line)
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/knn_select_probe.py --child gate --reps 3      (a run of its own)
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "adaptive-classifier_amd")]

ap = argparse.ArgumentParser()
ap.add_argument("--child", choices=["gate", "many", "batch"], default=None)
ap.add_argument("--suite", choices=["select", "batch"], default="select")
ap.add_argument("--rows", type=int, default=None)
ap.add_argument("--dim", type=int, default=768)
ap.add_argument("--nq", type=int, default=None)
ap.add_argument("--reps", type=int, default=12)
ap.add_argument("--out", default=None)
a = ap.parse_args()


def parent():
    res = {}
    for name, mode, env in (("gate_shipped", "gate", {}), ("gate_ring0", "gate", {"AC_KNN_RING": "0"}), ("many_queries", "many", {})):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", mode, "--dim", str(a.dim), "--reps", str(a.reps)]
        if a.rows:
            cmd += ["--rows", str(a.rows)]
        if a.nq:
            cmd += ["--nq", str(a.nq)]
        e = {k: v for k, v in os.environ.items() if k != "AC_KNN_RING"}
        e.update(env)
        p = subprocess.run(cmd, env=e, capture_output=True, text=True, timeout=400)      # a fresh process per configuration
        if p.returncode != 0:
            print(p.stdout[-2000:], p.stderr[-4000:], file=sys.stderr)
            raise SystemExit("child %s failed with status %d: nothing further is started" % (name, p.returncode))
        res[name] = json.loads(p.stdout.strip().splitlines()[-1])
        print(name, json.dumps(res[name]), flush=True)
    for leg in ("gate_shipped", "gate_ring0"):
        for m in ("l2", "ip"):
            t, s = res[leg]["topk_" + m], res[leg]["sel_ones_" + m]
            limit = t["median_ms"] * t["max_ms"] / t["min_ms"]
            res["gate_%s_%s" % (leg[5:], m)] = {"sel_ones_median_ms": s["median_ms"], "topk_median_ms": t["median_ms"],
                                               "topk_max_over_min": t["max_ms"] / t["min_ms"], "limit_ms": limit,
                                               "ratio": s["median_ms"] / t["median_ms"], "met": bool(s["median_ms"] <= limit)}
    print(json.dumps({k: v for k, v in res.items() if k.startswith("gate_") and "met" in v}))
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "knn_select.json"), "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


def _run_child(name, mode, env, extra=()):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", mode, "--dim", str(a.dim), "--reps", str(a.reps)] + list(extra)
    e = {k: v for k, v in os.environ.items() if k != "AC_KNN_RING"}
    e.update(env)
    p = subprocess.run(cmd, env=e, capture_output=True, text=True, timeout=400)          # a fresh process per configuration
    if p.returncode != 0:
        print(p.stdout[-2000:], p.stderr[-4000:], file=sys.stderr)
        raise SystemExit("child %s failed with status %d: nothing further is started" % (name, p.returncode))
    return json.loads(p.stdout.strip().splitlines()[-1])


def parent_batch():
    res = {}
    rows = ["--rows", str(a.rows)] if a.rows else []
    for name, nq in (("queries_256", 256), ("queries_16", 16)):
        res[name] = _run_child(name, "batch", {}, rows + ["--nq", str(nq)])
        print(name, json.dumps(res[name]), flush=True)
    gates = {}
    for name in ("queries_256", "queries_16"):
        r = res[name]
        for m in ("l2", "ip"):
            t, s = r["batch_" + m], r["batch_sel_ones_" + m]
            limit = t["median_ms"] * t["max_ms"] / t["min_ms"]
            gates["gate1_%s_%s" % (name, m)] = {"sel_ones_median_ms": s["median_ms"], "unfiltered_median_ms": t["median_ms"],
                                                "unfiltered_max_over_min": t["max_ms"] / t["min_ms"], "limit_ms": limit,
                                                "ratio": s["median_ms"] / t["median_ms"], "met": bool(s["median_ms"] <= limit)}
            h, f = r["batch_sel_half_" + m], r["fp32_sel_half_" + m]
            gates["gate2_%s_%s" % (name, m)] = {"prepared_half_median_ms": h["median_ms"], "fp32_half_median_ms": f["median_ms"],
                                                "fp32_over_prepared": f["median_ms"] / h["median_ms"], "met": bool(h["median_ms"] < f["median_ms"])}
    r = res["queries_256"]
    for m in ("l2", "ip"):
        fb = {s: r["batch_sel_%s_%s" % (s, m)]["fallback_queries"] for s in ("ones", "half", "eighth", "d32", "sparse", "block")}
        gates["gate3_" + m] = {"fallback_queries": fb, "met": all(fb[s] == 0 for s in ("ones", "half", "eighth", "d32"))}
    res["gates"] = gates
    print(json.dumps(gates))
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "knn_select_batch.json"), "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


def child_batch():
    import numpy as np
    import torch
    from adaptive_classifier import _native as nv
    from adaptive_classifier import index as ix
    nv.require_gpu()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    N, D, k, nq = a.rows or 1_000_000, a.dim, 32, a.nq or 256
    P = ix.synth_unit_rows(N, D, 1, device=dev)
    Q = ix.synth_unit_rows(nq, D, 2, device=dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(3)
    u = torch.rand(N, device=dev, generator=gen)
    block = torch.zeros(N, dtype=torch.bool, device=dev)
    block[N // 3: N // 3 + 100_000] = True
    sels = {"ones": ix.RowSelector.from_mask(torch.ones(N, dtype=torch.bool, device=dev)), "half": ix.RowSelector.from_mask(u < 0.5)}
    if nq > 64:
        sels.update(eighth=ix.RowSelector.from_mask(u < 0.125), d32=ix.RowSelector.from_mask(u < 1.0 / 32),
                    sparse=ix.RowSelector.from_mask(u < 0.01), block=ix.RowSelector.from_mask(block))
    del u, block
    prepared = ix.prepare_store(P, N, D)
    ws = torch.empty(max(ix.knn_workspace_bytes(N, D, nq, k), 256), dtype=torch.uint8, device=dev)
    wsb = torch.empty(ix.knn_batch_workspace_bytes(N, D, nq, k), dtype=torch.uint8, device=dev)
    stats = torch.zeros(4, dtype=torch.int32, device=dev)
    out = (torch.empty((nq, k), dtype=torch.float32, device=dev), torch.empty((nq, k), dtype=torch.int64, device=dev))
    legs = {}
    for m in ("l2", "ip"):
        f = ix.knn_ip_topk if m == "ip" else ix.knn_l2_topk
        legs["batch_" + m] = lambda f=f: f(P, N, D, Q, k, out=out, workspace=wsb, stats=stats, prepared=prepared)
        for s in sels:
            legs["batch_sel_%s_%s" % (s, m)] = lambda s=s, m=m: ix.knn_topk_sel(P, N, D, Q, k, sels[s], metric=m, out=out, workspace=wsb,
                                                                              stats=stats, prepared=prepared)
        for s in ("half",) if nq > 64 else ("ones", "half"):
            legs["fp32_sel_%s_%s" % (s, m)] = lambda s=s, m=m: ix.knn_topk_sel(P, N, D, Q, k, sels[s], metric=m, out=out, workspace=ws, stats=stats)
    info = {}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for _ in range(3):                                      # warm-up, every leg
        for n, f in legs.items():
            f()
            torch.cuda.synchronize()
            info[n] = {"fallback_queries": int(stats[0].item()), "stats1": int(stats[1].item())}
    times = {n: [] for n in legs}
    for _ in range(a.reps):
        for n, f in legs.items():                           # alternated: drift of the box hits every leg alike
            ev[0].record()
            f()
            ev[1].record()
            torch.cuda.synchronize()
            times[n].append(ev[0].elapsed_time(ev[1]))
            info[n]["fallback_queries"] = max(info[n]["fallback_queries"], int(stats[0].item()))
    res = {"workload": "%d x %d fp32 store + its fp16 plane, %d queries, k = %d; HIP events around whole calls, legs alternated, %d repeats"
                       % (N, D, nq, k, a.reps),
           "device": torch.cuda.get_device_name(0), "selected_rows": {s: v.count() for s, v in sels.items()}}
    for n, t in times.items():
        t = np.asarray(t)
        res[n] = dict(median_ms=float(np.median(t)), min_ms=float(t.min()), max_ms=float(t.max()), **info[n])
    print(json.dumps(res))


def child():
    import numpy as np
    import torch
    from adaptive_classifier import _native as nv
    from adaptive_classifier import index as ix
    nv.require_gpu()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    many = a.child == "many"
    N, D, k = a.rows or (1_000_000 if many else 10_000_000), a.dim, 32
    nq = a.nq or (256 if many else 16)
    P = ix.synth_unit_rows(N, D, 1, device=dev)
    Q = ix.synth_unit_rows(nq, D, 2, device=dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(3)
    u = torch.rand(N, device=dev, generator=gen)
    sels = {"half": ix.RowSelector.from_mask(u < 0.5)}
    if not many:
        block = torch.zeros(N, dtype=torch.bool, device=dev)
        block[N // 3: N // 3 + 100_000] = True
        sels.update(ones=ix.RowSelector.from_mask(torch.ones(N, dtype=torch.bool, device=dev)), sparse=ix.RowSelector.from_mask(u < 0.01),
                    block=ix.RowSelector.from_mask(block))
    del u
    ws = torch.empty(max(ix.knn_workspace_bytes(N, D, nq, k), 256), dtype=torch.uint8, device=dev)
    stats = torch.zeros(4, dtype=torch.int32, device=dev)
    out = (torch.empty((nq, k), dtype=torch.float32, device=dev), torch.empty((nq, k), dtype=torch.int64, device=dev))
    legs, info = {}, {}
    if many:
        prepared = ix.prepare_store(P, N, D)
        wsb = torch.empty(ix.knn_batch_workspace_bytes(N, D, nq, k), dtype=torch.uint8, device=dev)
        legs["topk_prepared_l2"] = lambda: ix.knn_l2_topk(P, N, D, Q, k, out=out, workspace=wsb, stats=stats, prepared=prepared)
        legs["topk_fp32_l2"] = lambda: ix.knn_l2_topk(P, N, D, Q, k, out=out, workspace=ws, stats=stats)
        legs["sel_half_l2"] = lambda: ix.knn_topk_sel(P, N, D, Q, k, sels["half"], metric="l2", out=out, workspace=ws, stats=stats)
    else:
        for m in ("l2", "ip"):
            f = ix.knn_ip_topk if m == "ip" else ix.knn_l2_topk
            legs["topk_" + m] = lambda f=f: f(P, N, D, Q, k, out=out, workspace=ws, stats=stats)
            for s in ("ones", "half", "sparse", "block"):
                legs["sel_%s_%s" % (s, m)] = lambda s=s, m=m: ix.knn_topk_sel(P, N, D, Q, k, sels[s], metric=m, out=out, workspace=ws, stats=stats)
        for M in (1000, 8192):
            ids = torch.sort(torch.randperm(N, device=dev, generator=gen)[:M])[0].contiguous()
            legs["ids_%d_l2" % M] = lambda ids=ids: ix.knn_topk_ids(P, N, D, Q, k, ids, metric="l2", out=out)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for _ in range(3):                                      # warm-up, every leg
        for n, f in legs.items():
            f()
            torch.cuda.synchronize()
            info[n] = {"fallback_queries": int(stats[0].item()), "ring": int(stats[1].item())} if not n.startswith("ids") else {}
    times = {n: [] for n in legs}
    for _ in range(a.reps):
        for n, f in legs.items():                           # alternated: drift of the box hits every leg alike
            ev[0].record()
            f()
            ev[1].record()
            torch.cuda.synchronize()
            times[n].append(ev[0].elapsed_time(ev[1]))
    res = {"workload": "%d x %d fp32 store, %d queries, k = %d; HIP events around whole calls, legs alternated, %d repeats" % (N, D, nq, k, a.reps),
           "device": torch.cuda.get_device_name(0), "AC_KNN_RING": os.environ.get("AC_KNN_RING", "unset"), "store_bytes": N * D * 4,
           "selected_rows": {s: v.count() for s, v in sels.items()}}
    for n, t in times.items():
        t = np.asarray(t)
        med = float(np.median(t))
        res[n] = dict(median_ms=med, min_ms=float(t.min()), max_ms=float(t.max()), store_GBps=N * D * 4 / med / 1e6, **info[n])
    print(json.dumps(res))


if a.child == "batch":
    child_batch()
elif a.child:
    child()
elif a.suite == "batch":
    parent_batch()
else:
    parent()
