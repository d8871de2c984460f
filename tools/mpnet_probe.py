"""What the relative position bias costs: an MPNet-base encoder (12 x 768, random weights) on 256 ragged texts of <= 32 tokens
(5141 token rows, the batch of tools/pooling_probe.py), ONE process, the same weights, three legs alternated window by window:

    bias             the table in place (AC_QKV_ATTN_FUSION=0: what a table forces anyway)     attention_mfma_kernel<false, 64, true>
    nobias_unfused   the table pointer nulled, AC_QKV_ATTN_FUSION=0                            attention_mfma_kernel<false, 64, false>
    nobias_fused     the table pointer nulled, attention in the QKV GEMM's epilogue            gemm_pipe_nt<... EPI_QKV_ATTN ...>

bias - nobias_unfused is the price of the bias itself; nobias_unfused - nobias_fused is the price of not having the bias inside
the fused epilogue.  A nulled table computes another function (BERT's attention); the times do not depend on the values.

    python tools/mpnet_probe.py [--rounds 7] [--calls 50] [--out FILE]         timing with device events, one JSON line
    python tools/mpnet_probe.py --trace 24                                     24 forwards per leg (bias, nobias_unfused) alternated,
                                                                               nothing timed: run it under rocprofv3 --kernel-trace
    python tools/mpnet_probe.py --kernels TRACE.csv [--out FILE]               the two attention kernels of such a trace: medians, spreads
"""
import argparse
import csv
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, S = 256, 32
LEGS = ("bias", "nobias_unfused", "nobias_fused")


def setup():
    sys.path[:0] = [ROOT, os.path.join(ROOT, "adaptive-classifier_amd")]
    import torch
    from adaptive_classifier.encoder import make_encoder
    from transformers import MPNetConfig, MPNetModel
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    enc = make_encoder(MPNetModel(MPNetConfig(), add_pooling_layer=False).eval(), device=dev)
    g = torch.Generator().manual_seed(1234)
    ids = torch.randint(1000, 30000, (B, S), generator=g)
    ids[:, 0] = 0
    lens = torch.randint(8, S + 1, (B,), generator=g)
    lens[0] = S
    mask = (torch.arange(S)[None, :] < lens[:, None]).to(torch.int64)
    ids = torch.where(mask.bool(), ids, torch.ones_like(ids)).to(dev)          # <pad> = 1
    table = enc.weights.attn_rel_bias

    def call(leg):
        os.environ["AC_QKV_ATTN_FUSION"] = "1" if leg == "nobias_fused" else "0"            # (read per call)
        enc.weights.attn_rel_bias = table if leg == "bias" else None
        try:
            return enc.encode_cls(ids, None, mask.to(dev), verify=False)
        finally:
            enc.weights.attn_rel_bias = table

    return torch, enc, call, int(lens.sum())


def timing(rounds, calls, out):
    torch, enc, call, tokens = setup()
    for leg in LEGS:
        for _ in range(5):
            r = call(leg)
        assert bool(torch.isfinite(r).all()), leg
    torch.cuda.synchronize()
    ms = {leg: [] for leg in LEGS}
    for _ in range(rounds):
        for leg in LEGS:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                call(leg)
            e1.record()
            torch.cuda.synchronize()
            ms[leg].append(e0.elapsed_time(e1) / calls)
    med = lambda v: sorted(v)[len(v) // 2]
    res = {"shape": f"mpnet-base 12 x 768, {B} ragged texts <= {S} tokens, {tokens} token rows", "rounds": rounds, "calls_per_window": calls,
           "legs": {leg: {"ms": med(v), "min": min(v), "max": max(v), "windows": [round(x, 4) for x in v]} for leg, v in ms.items()}}
    L = enc.ccfg.layers
    res["bias_us_per_token_layer"] = 1e3 * (res["legs"]["bias"]["ms"] - res["legs"]["nobias_unfused"]["ms"]) / (L - 1)
    res["unfused_us_per_token_layer"] = 1e3 * (res["legs"]["nobias_unfused"]["ms"] - res["legs"]["nobias_fused"]["ms"]) / (L - 1)
    line = json.dumps(res)
    print(line)
    if out:
        with open(out, "w") as f:
            f.write(line + "\n")


def trace(forwards):
    torch, _, call, _ = setup()
    for leg in LEGS[:2]:
        for _ in range(3):
            call(leg)
    torch.cuda.synchronize()
    for _ in range(forwards):
        for leg in LEGS[:2]:
            call(leg)
        torch.cuda.synchronize()


def kernels(path, out):
    dur = {"biased": [], "plain": []}
    for r in csv.DictReader(open(path)):
        name = r["Kernel_Name"]
        if "attention_mfma_kernel<false, 64" in name:
            dur["biased" if "attention_mfma_kernel<false, 64, true" in name else "plain"].append(
                (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    res = {}
    for k, v in dur.items():
        v.sort()
        n = len(v)
        res[k] = {"launches": n, "median_us": v[n // 2], "min_us": v[0], "p10_us": v[n // 10], "p90_us": v[(9 * n) // 10], "max_us": v[-1]}
    res["biased_over_plain"] = res["biased"]["median_us"] / res["plain"]["median_us"]
    line = json.dumps(res)
    print(line)
    if out:
        with open(out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--trace", type=int, default=0)
    ap.add_argument("--kernels", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.kernels:
        kernels(a.kernels, a.out)
    elif a.trace:
        trace(a.trace)
    else:
        timing(a.rounds, a.calls, a.out)
