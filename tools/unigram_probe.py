"""What tokenising a predict batch costs with a Unigram (SentencePiece-style) tokenizer, host route against device route: 256 texts
of <= 32 tokens (the BASELINE configs[1] batch shape), ONE process, the two legs alternated call by call:

    host     the wrapped tokenizer's call (max_length=32, truncation, padding, return_tensors="pt") + .to(device) of its tensors
             + a device synchronise: what a classifier does without a device tokenizer
    device   HipUnigramTokenizer.__call__ (one H2D of the packed bytes, ac_unigram_encode, one D2H of the lengths)

Each call is timed twice: wall clock around the call and its synchronise, and device events around it.  Two vocabularies: the
XLM-R style pipeline of tests/unigram_helpers.py over its trained pieces (a few hundred), and the same pieces plus random filler
pieces up to --pieces (default 250 000, XLM-R's size: a 16 MB piece table instead of one that fits any cache).  The ids of the
two legs are compared before anything is timed.

    python tools/unigram_probe.py [--calls 60] [--warmup 10] [--pieces 250000] [--out FILE]        one JSON line
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, M = 256, 32


def texts_of(n):
    import numpy as np
    from unigram_helpers import WORDS
    rng = np.random.default_rng(7)
    out = []
    for _ in range(n):
        ws = [str(rng.choice(WORDS)) for _ in range(int(rng.integers(4, 22)))]
        out.append(" ".join(ws) + str(rng.choice([".", "!", "?", ""])))
    return out


def tokenizer_of(pieces_wanted):
    """The xlmr pipeline of unigram_helpers; with pieces_wanted > 0 its vocabulary is padded with random lower-case filler
    pieces (with and without the metaspace, scores below every trained piece) up to that size."""
    import numpy as np
    import unigram_helpers as H
    pieces = list(H.trained_pieces("full"))
    if pieces_wanted > len(pieces):
        rng = np.random.default_rng(11)
        have = {p for p, _ in pieces}
        low = min(s for _, s in pieces)
        letters = np.array(list("abcdefghijklmnopqrstuvwxyz"))
        while len(pieces) < pieces_wanted:
            lens = rng.integers(3, 12, 65536)
            flat = rng.choice(letters, int(lens.sum()))
            at = 0
            for i, n in enumerate(lens):
                w = ("▁" if i & 1 else "") + "".join(flat[at:at + n])
                at += n
                if w not in have and len(pieces) < pieces_wanted:
                    have.add(w)
                    pieces.append((w, low - 1.0 - (i % 64) / 16.0))
    from transformers import XLMRobertaTokenizer
    return XLMRobertaTokenizer(vocab=H._xlmr_vocab(pieces), _spm_precompiled_charsmap=H.charsmap())


def main(calls, warmup, pieces, out):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "adaptive-classifier_amd"), os.path.join(ROOT, "tests")]
    import torch
    from adaptive_classifier.tokenizer import HipUnigramTokenizer
    dev = torch.device("cuda:0")
    texts = texts_of(B)
    res = {"box": torch.cuda.get_device_name(0), "texts": B, "max_length": M, "calls": calls, "warmup": warmup, "vocabularies": {}}
    for name, want in (("trained", 0), ("filled", pieces)):
        hf = tokenizer_of(want)
        t0 = time.perf_counter()
        dt = HipUnigramTokenizer(hf, device=dev)
        build_s = time.perf_counter() - t0

        def host():
            enc = hf(texts, max_length=M, truncation=True, padding=True, return_tensors="pt")
            return {k: v.to(dev) for k, v in enc.items()}

        def device():
            return dt(texts, max_length=M, truncation=True, padding=True, return_tensors="pt")

        a, b = host(), device()
        assert set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a), name
        assert dt.host_texts == 0
        legs = {"host": host, "device": device}
        for _ in range(warmup):
            for f in legs.values():
                f()
        torch.cuda.synchronize()
        wall, evt = {k: [] for k in legs}, {k: [] for k in legs}
        for _ in range(calls):
            for k, f in legs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                e0.record()
                f()
                e1.record()
                torch.cuda.synchronize()
                wall[k].append(1e3 * (time.perf_counter() - t0))
                evt[k].append(e0.elapsed_time(e1))
        med = lambda v: sorted(v)[len(v) // 2]                                                # noqa: E731
        res["vocabularies"][name] = {
            "pieces": len(hf), "table_slots": int(dt.vocab.slots), "tokens": int(a["attention_mask"].sum()), "padded_length": int(a["input_ids"].shape[1]),
            "wrapper_build_s": round(build_s, 3),
            **{k: {"wall_ms": round(med(wall[k]), 4), "wall_min": round(min(wall[k]), 4), "wall_p90": round(sorted(wall[k])[(9 * calls) // 10], 4),
                   "events_ms": round(med(evt[k]), 4)} for k in legs},
            "device_over_host_wall": round(med(wall["device"]) / med(wall["host"]), 4)}
    line = json.dumps(res)
    print(line)
    if out:
        with open(out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--pieces", type=int, default=250_000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    main(a.calls, a.warmup, a.pieces, a.out)
