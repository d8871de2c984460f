"""Probe: the range search (ac_knn_*_range_count + _fill) against the top-k search on the same store (not part of the product
or the tests).

  sweep-bound case   10M x 768 fp32 (30.72 GB), 16 queries, radii in the widest gap around rank 32 (taken from a top-k call):
                     range count + fill against ac_knn_*_topk at k = 32, both metrics, legs ALTERNATED in one process, HIP events
                     around whole calls, medians after warm-up.  AC_KNN_RING is read once per process, so the two forms of the
                     top-k sweep (AC_KNN_RING=0: knn_sweep<1>, the load path of the range sweep; as shipped: knn_sweep_ring) run
                     in a child process each.  Acceptance: range l2 median <= the AC_KNN_RING=0 top-k median times that leg's own
                     max / min spread.
  many-hit case      1M x 768, 16 queries, radii admitting ~1 % of the rows (from a 20 000-row sample): count and fill apart.
  selection case     what a selection costs the range sweep: the sweep-bound store and radii, four legs ALTERNATED in one process --
                     (a) the unfiltered count + fill, (b) count_sel with an all-ones selection + fill, (c) a random 1/32 selection,
                     (d) the id-list route at M = 8192 (count_ids + fill_ids).  Acceptance for (b): its median <= (a)'s median
                     times (a)'s own max / min spread.  (c) and (d) are recorded only.

    python tools/knn_range_probe.py [--out DIR]                 spawns the children, writes DIR/knn_range.json
    python tools/knn_range_probe.py --child sweep|many|sel      one configuration in this process (prints one JSON line)
    python tools/knn_range_probe.py --sel [--out DIR]           the FILTERED range search only: writes DIR/knn_range_sel.json
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/knn_range_probe.py --child sweep --reps 3     (a run of its own)
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "adaptive-classifier_amd")]

ap = argparse.ArgumentParser()
ap.add_argument("--child", choices=["sweep", "many", "sel"], default=None)
ap.add_argument("--sel", action="store_true", help="run the selection case only")
ap.add_argument("--rows", type=int, default=None)
ap.add_argument("--dim", type=int, default=768)
ap.add_argument("--nq", type=int, default=16)
ap.add_argument("--reps", type=int, default=12)
ap.add_argument("--out", default=None)
a = ap.parse_args()


def parent():
    res = {}
    for name, mode, env in (("sweep_ring0", "sweep", {"AC_KNN_RING": "0"}), ("sweep_shipped", "sweep", {}), ("many_hits", "many", {})):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", mode, "--dim", str(a.dim), "--nq", str(a.nq), "--reps", str(a.reps)]
        if a.rows:
            cmd += ["--rows", str(a.rows)]
        e = {k: v for k, v in os.environ.items() if k != "AC_KNN_RING"}
        e.update(env)
        p = subprocess.run(cmd, env=e, capture_output=True, text=True, timeout=400)      # a fresh process per configuration
        if p.returncode != 0:
            print(p.stdout[-2000:], p.stderr[-4000:], file=sys.stderr)
            raise SystemExit("child %s failed with status %d: nothing further is started" % (name, p.returncode))
        res[name] = json.loads(p.stdout.strip().splitlines()[-1])
        print(name, json.dumps(res[name]), flush=True)
    r0 = res["sweep_ring0"]
    for m in ("l2", "ip"):
        t, r = r0["topk_" + m], r0["range_" + m]
        limit = t["median_ms"] * t["max_ms"] / t["min_ms"]
        res["acceptance_" + m] = {"range_median_ms": r["median_ms"], "topk_ring0_median_ms": t["median_ms"],
                                  "topk_ring0_max_over_min": t["max_ms"] / t["min_ms"], "limit_ms": limit,
                                  "met": bool(r["median_ms"] <= limit),
                                  "range_over_topk_shipped": r["median_ms"] / res["sweep_shipped"]["topk_" + m]["median_ms"]}
    print(json.dumps({k: v for k, v in res.items() if k.startswith("acceptance")}))
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "knn_range.json"), "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


def run_child(name, mode, env):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", mode, "--dim", str(a.dim), "--nq", str(a.nq), "--reps", str(a.reps)]
    if a.rows:
        cmd += ["--rows", str(a.rows)]
    e = {k: v for k, v in os.environ.items() if k != "AC_KNN_RING"}
    e.update(env)
    p = subprocess.run(cmd, env=e, capture_output=True, text=True, timeout=400)      # a fresh process per configuration
    if p.returncode != 0:
        print(p.stdout[-2000:], p.stderr[-4000:], file=sys.stderr)
        raise SystemExit("child %s failed with status %d: nothing further is started" % (name, p.returncode))
    return json.loads(p.stdout.strip().splitlines()[-1])


def parent_sel():
    res = {"selection": run_child("selection", "sel", {})}
    r = res["selection"]
    for m in ("l2", "ip"):
        u, b = r["unfiltered_" + m], r["sel_ones_" + m]
        limit = u["median_ms"] * u["max_ms"] / u["min_ms"]
        res["acceptance_" + m] = {"sel_ones_median_ms": b["median_ms"], "unfiltered_median_ms": u["median_ms"],
                                  "unfiltered_max_over_min": u["max_ms"] / u["min_ms"], "limit_ms": limit,
                                  "met": bool(b["median_ms"] <= limit), "sel_ones_over_unfiltered": b["median_ms"] / u["median_ms"]}
    print(json.dumps(res))
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "knn_range_sel.json"), "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


def child_sel():
    import numpy as np
    import torch
    from adaptive_classifier import _native as nv
    from adaptive_classifier import index as ix
    nv.require_gpu()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    L = nv.lib()
    N, D, nq, M = a.rows or 10_000_000, a.dim, a.nq, min(8192, a.rows or 10_000_000)
    P = ix.synth_unit_rows(N, D, 1, device=dev)
    Q = ix.synth_unit_rows(nq, D, 2, device=dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(3)
    sels = {"ones": ix.RowSelector.from_mask(torch.ones(N, dtype=torch.bool, device=dev)).words,
            "d32": ix.RowSelector.from_mask(torch.rand(N, device=dev, generator=gen) < 1.0 / 32).words}
    ids = torch.randperm(N, device=dev, generator=gen)[:M].sort().values.contiguous()
    rad = {}
    for m in ("l2", "ip"):                                  # the fp32 midpoint of the widest gap between ranks 28 .. 36 (all rows)
        v, _ = (ix.knn_ip_topk if m == "ip" else ix.knn_l2_topk)(P, N, D, Q, 40)
        v = v.double()
        i = 28 + (v[:, 29:37] - v[:, 28:36]).abs().argmax(dim=1)
        rows = torch.arange(nq, device=dev)
        rad[m] = (0.5 * (v[rows, i] + v[rows, i + 1])).float().contiguous()
    ws_r = torch.empty(ix.knn_range_workspace_bytes(N, D, nq), dtype=torch.uint8, device=dev)
    ws_i = torch.empty(ix.knn_range_ids_workspace_bytes(M, nq), dtype=torch.uint8, device=dev)
    stats = torch.zeros(4, dtype=torch.int32, device=dev)
    lims = torch.empty(nq + 1, dtype=torch.int64, device=dev)
    st = nv.stream_ptr(dev)
    oD = torch.empty(nq * 64, dtype=torch.float32, device=dev)            # (ranks 28 .. 36: at most 37 hits per query)
    oI = torch.empty(nq * 64, dtype=torch.int64, device=dev)
    head = (nv.ptr(P), N, P.stride(0), D)
    qargs = (nv.ptr(Q), nq, Q.stride(0))

    def count(m, sel):
        if sel is None:
            rc = getattr(L, "ac_knn_%s_range_count" % m)(*head, *qargs, nv.ptr(rad[m]), nv.ptr(lims), nv.ptr(ws_r), ws_r.numel(), nv.ptr(stats), st)
        else:
            rc = getattr(L, "ac_knn_%s_range_count_sel" % m)(*head, *qargs, nv.ptr(rad[m]), nv.ptr(sels[sel]), 0, nv.ptr(lims), nv.ptr(ws_r),
                                                              ws_r.numel(), nv.ptr(stats), st)
        nv.check(rc, "count")

    def fill(m):
        nv.check(getattr(L, "ac_knn_%s_range_fill" % m)(*head, *qargs, 0, nv.ptr(lims), oD.numel(), nv.ptr(oD), None, nv.ptr(oI), nv.ptr(ws_r),
                                                         ws_r.numel(), nv.ptr(stats), st), "fill")

    def count_ids(m):
        nv.check(getattr(L, "ac_knn_%s_range_count_ids" % m)(*head, nv.ptr(ids), M, *qargs, nv.ptr(rad[m]), nv.ptr(lims), nv.ptr(ws_i),
                                                              ws_i.numel(), nv.ptr(stats), st), "count_ids")

    def fill_ids(m):
        nv.check(getattr(L, "ac_knn_%s_range_fill_ids" % m)(*head, nv.ptr(ids), M, *qargs, 0, nv.ptr(lims), oD.numel(), nv.ptr(oD), None,
                                                             nv.ptr(oI), nv.ptr(ws_i), ws_i.numel(), nv.ptr(stats), st), "fill_ids")

    legs, info = {}, {}
    for m in ("l2", "ip"):
        legs["unfiltered_" + m] = [lambda m=m: count(m, None), lambda m=m: fill(m)]
        legs["sel_ones_" + m] = [lambda m=m: count(m, "ones"), lambda m=m: fill(m)]
        legs["sel_d32_" + m] = [lambda m=m: count(m, "d32"), lambda m=m: fill(m)]
        legs["ids_8192_" + m] = [lambda m=m: count_ids(m), lambda m=m: fill_ids(m)]
    for n, steps in legs.items():                           # one run each for the figures the timed calls never read
        steps[0]()
        steps[1]()
        torch.cuda.synchronize()
        info[n] = {"hits_total": int(lims[-1].item()), "pairs_decided_exactly": int(stats[0].item()), "fill_overflow": int(stats[1].item())}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
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
            steps[1]()
            ev[2].record()
            torch.cuda.synchronize()
            times[n].append((ev[0].elapsed_time(ev[2]), ev[0].elapsed_time(ev[1]), ev[1].elapsed_time(ev[2])))
    res = {"workload": "%d x %d fp32 store, %d queries; HIP events around count + fill, legs alternated, 3 warm-ups, %d repeats" % (N, D, nq, a.reps),
           "device": torch.cuda.get_device_name(0), "store_bytes": N * D * 4, "bitmap_ws_bytes": int(ws_r.numel()),
           "ids_ws_bytes": int(ws_i.numel()), "M": M}
    for n, t in times.items():
        t = np.asarray(t)
        med = float(np.median(t[:, 0]))
        res[n] = dict(median_ms=med, min_ms=float(t[:, 0].min()), max_ms=float(t[:, 0].max()), count_median_ms=float(np.median(t[:, 1])),
                      fill_median_ms=float(np.median(t[:, 2])), **info[n])
    print(json.dumps(res))


def child():
    import numpy as np
    import torch
    from adaptive_classifier import _native as nv
    from adaptive_classifier import index as ix
    nv.require_gpu()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    L = nv.lib()
    many = a.child == "many"
    N, D, nq, k = a.rows or (1_000_000 if many else 10_000_000), a.dim, a.nq, 32
    P = ix.synth_unit_rows(N, D, 1, device=dev)
    Q = ix.synth_unit_rows(nq, D, 2, device=dev)
    metrics = ("l2",) if many else ("l2", "ip")
    rad, hits = {}, {}
    for m in metrics:
        if many:                                            # the 1 % quantile of a 20 000-row sample
            d = ((P[:20000, :D].double()[None] - Q.double()[:, None]) ** 2).sum(-1)
            rad[m] = torch.quantile(d, 0.01, dim=1).float().contiguous()
        else:                                               # the fp32 midpoint of the widest gap between ranks 28 .. 36
            v, _ = (ix.knn_ip_topk if m == "ip" else ix.knn_l2_topk)(P, N, D, Q, 40)
            v = v.double()
            gaps = (v[:, 29:37] - v[:, 28:36]).abs()
            i = 28 + gaps.argmax(dim=1)
            rows = torch.arange(nq, device=dev)
            rad[m] = (0.5 * (v[rows, i] + v[rows, i + 1])).float().contiguous()
    ws_t = torch.empty(max(ix.knn_workspace_bytes(N, D, nq, k), 256), dtype=torch.uint8, device=dev)
    ws_r = torch.empty(ix.knn_range_workspace_bytes(N, D, nq), dtype=torch.uint8, device=dev)
    stats = torch.zeros(4, dtype=torch.int32, device=dev)
    out = (torch.empty((nq, k), dtype=torch.float32, device=dev), torch.empty((nq, k), dtype=torch.int64, device=dev))
    lims = torch.empty(nq + 1, dtype=torch.int64, device=dev)
    st = nv.stream_ptr(dev)
    bufs, info = {}, {}

    def count(m):
        nv.check(getattr(L, "ac_knn_%s_range_count" % m)(nv.ptr(P), N, P.stride(0), D, nv.ptr(Q), nq, Q.stride(0), nv.ptr(rad[m]), nv.ptr(lims),
                                                          nv.ptr(ws_r), ws_r.numel(), nv.ptr(stats), st), "count")

    def fill(m):
        oD, oI = bufs[m]
        nv.check(getattr(L, "ac_knn_%s_range_fill" % m)(nv.ptr(P), N, P.stride(0), D, nv.ptr(Q), nq, Q.stride(0), 0, nv.ptr(lims), oD.numel(),
                                                         nv.ptr(oD), None, nv.ptr(oI), nv.ptr(ws_r), ws_r.numel(), nv.ptr(stats), st), "fill")

    for m in metrics:                                       # sizes the outputs once; the timed calls below never read the host
        count(m)
        total = int(lims[-1].item())
        bufs[m] = (torch.empty(max(total, 1), dtype=torch.float32, device=dev), torch.empty(max(total, 1), dtype=torch.int64, device=dev))
        fill(m)
        torch.cuda.synchronize()
        info[m] = {"hits_total": total, "hits_per_query_min": int(lims.diff().min().item()), "hits_per_query_max": int(lims.diff().max().item()),
                   "pairs_decided_exactly": int(stats[0].item()), "fill_overflow": int(stats[1].item())}
    legs = {}
    for m in metrics:
        if not many:
            f = ix.knn_ip_topk if m == "ip" else ix.knn_l2_topk
            legs["topk_" + m] = [lambda f=f: f(P, N, D, Q, k, out=out, workspace=ws_t, stats=stats)]
        legs["range_" + m] = [lambda m=m: count(m), lambda m=m: fill(m)]
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    for _ in range(3):                                      # warm-up, every leg
        for steps in legs.values():
            for s in steps:
                s()
    torch.cuda.synchronize()
    times = {n: [] for n in legs}
    parts = {n: [] for n in legs}
    ring = {}
    for _ in range(a.reps):
        for n, steps in legs.items():                       # alternated: drift of the box hits every leg alike
            ev[0].record()
            steps[0]()
            ev[1].record()
            if len(steps) > 1:
                steps[1]()
                ev[2].record()
            torch.cuda.synchronize()
            if len(steps) > 1:
                times[n].append(ev[0].elapsed_time(ev[2]))
                parts[n].append((ev[0].elapsed_time(ev[1]), ev[1].elapsed_time(ev[2])))
            else:
                times[n].append(ev[0].elapsed_time(ev[1]))
                ring[n] = int(stats[1].item())
    bytes_alg = N * D * 4
    res = {"workload": "%d x %d fp32 store, %d queries; HIP events around whole calls, legs alternated, %d repeats" % (N, D, nq, a.reps),
           "device": torch.cuda.get_device_name(0), "AC_KNN_RING": os.environ.get("AC_KNN_RING", "unset"), "store_bytes": bytes_alg,
           "bitmap_bytes": int(ws_r.numel())}
    for n, t in times.items():
        t = np.asarray(t)
        med = float(np.median(t))
        res[n] = {"median_ms": med, "min_ms": float(t.min()), "max_ms": float(t.max()), "store_GBps": bytes_alg / med / 1e6}
        if parts[n]:
            p = np.asarray(parts[n])
            res[n].update(count_median_ms=float(np.median(p[:, 0])), fill_median_ms=float(np.median(p[:, 1])), **info[n.split("_")[1]])
        else:
            res[n]["ring"] = ring[n]
    print(json.dumps(res))


if a.child == "sel":
    child_sel()
elif a.child:
    child()
elif a.sel:
    parent_sel()
else:
    parent()
