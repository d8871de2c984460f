"""What a mean-pooled forward costs: `encode_cls` at the configs[1] shape (bert-base, 256 ragged texts of <= 32 tokens, the batch
of tools/encode_ab.py) timed on three legs,
    parent   the parent commit's library (--parent PATH, loaded through AC_LIBACAMD_PATH), pooling="cls"
    cls      this tree, pooling="cls"
    mean     this tree, pooling="mean"
each leg in a fresh child process (a library is loaded once per process), the legs alternated round by round on the same box;
a child warms the shape up, then times WINDOWS windows of CALLS calls each with device events and reports the median window.
The driver prints one JSON line: per leg the per-round medians, their median and their spread, the ratios cls / parent and
mean / cls, and max |cls - parent| of the embeddings (the CLS route must not have changed by a bit).

    python tools/pooling_probe.py --parent tools/ab/libacamd_parent.so [--rounds 3] [--out FILE]
    python tools/pooling_probe.py --leg mean --calls 20 --windows 1       (one child alone, e.g. under rocprofv3 --kernel-trace --stats)
    python tools/pooling_probe.py --kernel-time STATS.csv                 (the pool kernel's row of a rocprofv3 kernel-stats file)
"""
import argparse
import csv
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, S = 256, 32


def child(leg, calls, windows):
    os.environ.setdefault("AC_TEST_HOOKS", "1")
    sys.path[:0] = [ROOT, os.path.join(ROOT, "adaptive-classifier_amd")]
    import torch
    from adaptive_classifier import _native as nv
    from adaptive_classifier.encoder import HipBertEncoder
    from transformers import BertConfig, BertModel
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    enc = HipBertEncoder(BertModel(BertConfig(), add_pooling_layer=False).eval(), device=dev)
    g = torch.Generator().manual_seed(1234)
    ids = torch.randint(1000, 30000, (B, S), generator=g)
    ids[:, 0] = 101
    lens = torch.randint(8, S + 1, (B,), generator=g)
    lens[0] = S
    mask = (torch.arange(S)[None, :] < lens[:, None]).to(torch.int64)
    ids = (ids * mask).to(dev)
    mask = mask.to(dev)
    types = torch.zeros_like(ids)
    kw = {"pooling": "mean"} if leg == "mean" else {}        # (the parent's encoder has no such keyword: "cls" legs pass none)
    for _ in range(5):
        out = enc.encode_cls(ids, types, mask, **kw)
    torch.cuda.synchronize()
    times = []
    for _ in range(windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            out = enc.encode_cls(ids, types, mask, **kw)
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) / calls)
    times.sort()
    host = out.float().cpu()
    assert bool(torch.isfinite(host).all())
    print(json.dumps({"leg": leg, "version": nv.lib().ac_version(), "ms": times[len(times) // 2], "ms_min": times[0], "ms_max": times[-1],
                      "tokens": enc.last_tokens, "sha256": hashlib.sha256(host.numpy().tobytes()).hexdigest(),
                      "flops": enc.flops(B, S, tokens=int(lens.sum()), sum_len_sq=float((lens * lens).sum()), **kw)}))


def kernel_time(path):
    rows = [r for r in csv.DictReader(open(path)) if "pool_mean_normalize_kernel" in r["Name"]]
    assert len(rows) == 1, [r["Name"] for r in rows]
    r = rows[0]
    print(json.dumps({"kernel": "pool_mean_normalize_kernel", "calls": int(r["Calls"]), "average_us": float(r["AverageNs"]) / 1e3,
                      "min_us": float(r["MinNs"]) / 1e3, "max_us": float(r["MaxNs"]) / 1e3, "share_of_kernel_time_percent": float(r["Percentage"])}))


def driver(parent, rounds, calls, windows, out):
    legs = (["parent"] if parent else []) + ["cls", "mean"]
    runs = {leg: [] for leg in legs}
    for _ in range(rounds):
        for leg in legs:
            env = dict(os.environ)
            env.pop("AC_LIBACAMD_PATH", None)
            if leg == "parent":
                env["AC_LIBACAMD_PATH"] = os.path.abspath(parent)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", leg, "--calls", str(calls), "--windows", str(windows)],
                               env=env, capture_output=True, text=True, timeout=600)
            if p.returncode != 0:                        # nothing more on the device after a failed leg
                sys.stderr.write(p.stdout + p.stderr)
                sys.exit(p.returncode or 1)
            runs[leg].append(json.loads(p.stdout.strip().splitlines()[-1]))
    med = lambda v: sorted(v)[len(v) // 2]
    res = {"shape": f"bert-base, {B} ragged texts <= {S} tokens", "rounds": rounds, "calls_per_window": calls, "windows": windows, "legs": {}}
    for leg in legs:
        ms = [r["ms"] for r in runs[leg]]
        assert len({r["sha256"] for r in runs[leg]}) == 1, leg                 # the same bits in every round
        res["legs"][leg] = {"version": runs[leg][0]["version"], "ms_rounds": ms, "ms": med(ms), "spread_percent": 100.0 * (max(ms) - min(ms)) / med(ms),
                            "tokens": runs[leg][0]["tokens"], "flops": runs[leg][0]["flops"], "sha256": runs[leg][0]["sha256"]}
    if parent:
        res["cls_over_parent"] = res["legs"]["cls"]["ms"] / res["legs"]["parent"]["ms"]
        res["cls_bits_equal_parent"] = res["legs"]["cls"]["sha256"] == res["legs"]["parent"]["sha256"]
    res["mean_over_cls"] = res["legs"]["mean"]["ms"] / res["legs"]["cls"]["ms"]
    line = json.dumps(res)
    print(line)
    if out:
        with open(out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="the parent commit's libacamd.so (built under the git-ignored tools/ab/)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--leg", default=None, choices=["parent", "cls", "mean"])
    ap.add_argument("--kernel-time", default=None)
    a = ap.parse_args()
    if a.kernel_time:
        kernel_time(a.kernel_time)
    elif a.leg:
        child(a.leg, a.calls, a.windows)
    else:
        driver(a.parent, a.rounds, a.calls, a.windows, a.out)
