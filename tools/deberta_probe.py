"""What the disentangled attention costs: a random-weight encoder of deberta-v3-base's architecture (12 x 768, 12 heads, 256 buckets,
512 positions, a 2000-word vocabulary) against a BERT-base of the same dimensions, ONE process, legs alternated window by window:

    deberta         position_scores_kernel + attention_mfma_kernel<false, 64, false, PosScores> in every token layer
    bert_unfused    the BERT block, AC_QKV_ATTN_FUSION=0: attention_mfma_kernel<false, 64, false>
    bert_fused      the BERT block, attention in the QKV GEMM's epilogue where it applies (longest sequence <= 64)

at two shapes: `bench` = 256 ragged texts of 8 .. 32 tokens (packed), `long` = 16 x 512 tokens (no padding).
deberta - bert_unfused is the price of the two position terms (scores + gather), bert_unfused - bert_fused that of the lost fusion.
The kernel trace splits the first: position_scores_kernel, the two attention kernels, and the QKV GEMM launched right before every
position_scores_kernel.

    python tools/deberta_probe.py [--rounds 5] [--calls 20] [--out FILE]          timing with device events, one JSON line
    python tools/deberta_probe.py --trace 8                                       8 forwards per leg and shape, nothing timed: run it
                                                                                  under rocprofv3 --kernel-trace
    python tools/deberta_probe.py --kernels TRACE.csv [--out FILE]                per-kernel medians of such a trace
"""
import argparse
import csv
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEGS = ("deberta", "bert_unfused", "bert_fused")
SHAPES = ("bench", "long")


def setup():
    sys.path[:0] = [ROOT, os.path.join(ROOT, "adaptive-classifier_amd")]
    import torch
    from adaptive_classifier.encoder import make_encoder
    from transformers import BertConfig, BertModel, DebertaV2Config, DebertaV2Model
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    dcfg = DebertaV2Config(vocab_size=2000, hidden_size=768, num_hidden_layers=12, num_attention_heads=12, intermediate_size=3072,
                           max_position_embeddings=512, type_vocab_size=0, relative_attention=True, position_buckets=256,
                           pos_att_type=["p2c", "c2p"], share_att_key=True, norm_rel_ebd="layer_norm", position_biased_input=False,
                           max_relative_positions=-1, hidden_act="gelu")
    deb = make_encoder(DebertaV2Model(dcfg).eval(), device=dev)
    bert = make_encoder(BertModel(BertConfig(vocab_size=2000, hidden_size=768, num_hidden_layers=12, num_attention_heads=12,
                                             intermediate_size=3072, max_position_embeddings=512), add_pooling_layer=False).eval(), device=dev)
    g = torch.Generator().manual_seed(1234)
    B, S = 256, 32
    ids = torch.randint(1000, 2000, (B, S), generator=g)
    ids[:, 0] = 101
    lens = torch.randint(8, S + 1, (B,), generator=g)
    lens[0] = S
    mask = (torch.arange(S)[None, :] < lens[:, None]).to(torch.int64)
    batches = {"bench": (torch.where(mask.bool(), ids, torch.zeros_like(ids)).to(dev), mask.to(dev), int(lens.sum())),
               "long": (torch.randint(1000, 2000, (16, 512), generator=g).to(dev), None, 16 * 512)}

    def call(leg, shape):
        os.environ["AC_QKV_ATTN_FUSION"] = "1" if leg == "bert_fused" else "0"             # (read per call)
        ids, mask, _ = batches[shape]
        return (deb if leg == "deberta" else bert).encode_cls(ids, None, mask, verify=False)

    return torch, deb, call, {k: v[2] for k, v in batches.items()}


def timing(rounds, calls, out):
    torch, deb, call, tokens = setup()
    res = {"model": "12 x 768, 12 heads, 256 buckets, 512 positions; BERT-base of the same dimensions", "rounds": rounds,
           "calls_per_window": calls, "shapes": {}}
    layers = deb.ccfg.layers
    for shape in SHAPES:
        for leg in LEGS:
            for _ in range(3):
                r = call(leg, shape)
            assert bool(torch.isfinite(r).all()), (leg, shape)
        torch.cuda.synchronize()
        ms = {leg: [] for leg in LEGS}
        for _ in range(rounds):
            for leg in LEGS:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(calls):
                    call(leg, shape)
                e1.record()
                torch.cuda.synchronize()
                ms[leg].append(e0.elapsed_time(e1) / calls)
        med = lambda v: sorted(v)[len(v) // 2]
        legs = {leg: {"ms": med(v), "min": min(v), "max": max(v), "windows": [round(x, 4) for x in v]} for leg, v in ms.items()}
        res["shapes"][shape] = {"token_rows": tokens[shape], "legs": legs,
                                "position_terms_us_per_token_layer": 1e3 * (legs["deberta"]["ms"] - legs["bert_unfused"]["ms"]) / (layers - 1),
                                "unfused_us_per_token_layer": 1e3 * (legs["bert_unfused"]["ms"] - legs["bert_fused"]["ms"]) / (layers - 1)}
    line = json.dumps(res)
    print(line)
    if out:
        with open(out, "w") as f:
            f.write(line + "\n")


def trace(forwards):
    torch, _, call, _ = setup()
    for shape in SHAPES:
        for leg in LEGS[:2]:
            for _ in range(2):
                call(leg, shape)
        torch.cuda.synchronize()
        for _ in range(forwards):
            for leg in LEGS[:2]:
                call(leg, shape)
            torch.cuda.synchronize()


def kernels(path, out):
    """medians per kernel and grid size (the two shapes launch different grids); the QKV GEMM = the launch before every
    position_scores_kernel"""
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    dur = {}

    def put(key, r):
        dur.setdefault(key, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)

    for i, r in enumerate(rows):
        name, grid = r["Kernel_Name"], r.get("Grid_Size", r.get("Grid_Size_X", "?"))
        if "position_scores_kernel" in name:
            put(f"position_scores_kernel grid {grid}", r)
            if i and "gemm" in rows[i - 1]["Kernel_Name"]:
                put(f"qkv gemm before position_scores grid {grid}", rows[i - 1])
        elif "attention_mfma_kernel<false, 64" in name:
            put(("attention_mfma PosScores" if "PosScores" in name else "attention_mfma plain") + f" grid {grid}", r)
        elif "attention_cls_kernel" in name:
            put(("attention_cls PosScores" if "PosScores" in name else "attention_cls plain") + f" grid {grid}", r)
    res = {}
    for k, v in sorted(dur.items()):
        v.sort()
        n = len(v)
        res[k] = {"launches": n, "median_us": v[n // 2], "min_us": v[0], "p10_us": v[n // 10], "p90_us": v[(9 * n) // 10], "max_us": v[-1]}
    line = json.dumps(res)
    print(line)
    if out:
        with open(out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
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
