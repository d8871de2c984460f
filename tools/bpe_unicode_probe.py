"""What tokenising a predict batch of mostly-English texts that carry typographic punctuation, accents and emoji costs with a
byte-level BPE tokenizer (RoBERTa style and ModernBERT style): 256 and 1024 texts at max_length 32, ONE process, three legs
alternated call by call on the same texts:

    wrapped  the wrapped tokenizer's call (max_length=32, truncation, padding, return_tensors="pt") + .to(device) of its tensors
             + a device synchronise: what a classifier does without a device tokenizer
    host     HipByteBPETokenizer(hf).__call__, the default routing: every text with a non-ASCII byte goes to the wrapped tokenizer
             and is spliced into the batch, the ASCII ones run through ac_bpe_encode
    device   HipByteBPETokenizer(hf, unicode=True).__call__: one H2D of the packed bytes, ac_bpe_utf8_encode, one D2H of the lengths

The texts are word salads of tests/bpe_helpers.py (English) in which about every fifth word is one of tests/bpe_unicode_helpers.py
(accented, Cyrillic, short CJK, typographic apostrophes and quotes, currency), most with a typographic tail (an ellipsis, a dash,
an emoji): about two texts in three hold a non-ASCII character.  The tokenizers are the pipelines of bpe_unicode_helpers over its
trained vocabulary.  Also reported: the table build (build_bpe_unicode_tables, uncached) and its host_only counts per pipeline.
Each call is timed twice: wall clock around the call and its synchronise, and device events around it.  The ids of the three
legs are compared before anything is timed.

    python tools/bpe_unicode_probe.py [--calls 40] [--warmup 8] [--out FILE]        one JSON line
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M = 32


def texts_of(n):
    import numpy as np
    import bpe_helpers as B
    import bpe_unicode_helpers as H
    rng = np.random.default_rng(7)
    tails = H.UNI_TAILS + ["", "", ".", "!", "?"]
    out = []
    for _ in range(n):
        ws = [str(rng.choice(H.UNI_WORDS if rng.random() < 0.2 else B.WORDS)) for _ in range(int(rng.integers(4, 22)))]
        out.append(" ".join(ws) + (str(rng.choice(tails)) if rng.random() < 0.5 else ""))
    return out


def main(calls, warmup, out):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "adaptive-classifier_amd"), os.path.join(ROOT, "tests")]
    import torch
    import bpe_unicode_helpers as H
    from adaptive_classifier import tokenizer as tkz
    dev = torch.device("cuda:0")
    res = {"box": torch.cuda.get_device_name(0), "max_length": M, "calls": calls, "warmup": warmup, "pipelines": {}}
    for kind in ("roberta", "modernbert"):
        hf = H.build_tokenizer(kind)
        tkz._BPE_UNICODE_CACHE.clear()
        tables = tkz.build_bpe_unicode_tables(hf)
        t0 = time.perf_counter()
        plain = tkz.HipByteBPETokenizer(hf, device=dev)
        t1 = time.perf_counter()
        uni = tkz.HipByteBPETokenizer(hf, device=dev, unicode=True)                # (the table comes from the cache: the guard runs)
        t2 = time.perf_counter()
        assert uni.unicode
        p = res["pipelines"][kind] = {
            "vocab": len(hf), "table_build_s": round(tables["seconds"], 3), "n_pages": tables["n_pages"],
            "table_bytes": int(sum(t.numel() * t.element_size() for t in uni._ut)), "host_only": len(tables["host_only"]),
            "host_only_reasons": tables["reasons"], "whitespace_code_points": len(tables["whitespace"]),
            "wrapper_build_s": round(t1 - t0, 3), "unicode_wrapper_build_s_table_cached": round(t2 - t1, 3), "batches": {}}
        for b in (256, 1024):
            texts = texts_of(b)

            def wrapped():
                enc = hf(texts, max_length=M, truncation=True, padding=True, return_tensors="pt")
                return {k: v.to(dev) for k, v in enc.items()}

            def host():
                return plain(texts, max_length=M, truncation=True, padding=True, return_tensors="pt")

            def device():
                return uni(texts, max_length=M, truncation=True, padding=True, return_tensors="pt")

            a = wrapped()
            before = (uni.device_texts, uni.host_texts, plain.host_texts)
            for other in (host(), device()):
                assert set(a) == set(other) and all(torch.equal(a[k], other[k]) for k in a), (kind, b)
            on_device, deferred, routed = uni.device_texts - before[0], uni.host_texts - before[1], plain.host_texts - before[2]
            legs = {"wrapped": wrapped, "host": host, "device": device}
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
            p["batches"][str(b)] = {
                "non_ascii_texts": sum(1 for t in texts if not t.isascii()), "tokens": int(a["attention_mask"].sum()),
                "padded_length": int(a["input_ids"].shape[1]), "text_bytes": sum(len(t.encode()) for t in texts),
                "unicode_route_device_texts": on_device, "unicode_route_host_texts": deferred, "default_route_host_texts": routed,
                **{k: {"wall_ms": round(med(wall[k]), 4), "wall_min": round(min(wall[k]), 4),
                       "wall_p90": round(sorted(wall[k])[(9 * calls) // 10], 4), "events_ms": round(med(evt[k]), 4)} for k in legs},
                "device_over_host_wall": round(med(wall["device"]) / med(wall["host"]), 4),
                "device_over_wrapped_wall": round(med(wall["device"]) / med(wall["wrapped"]), 4)}
    line = json.dumps(res)
    print(line)
    if out:
        with open(out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    main(a.calls, a.warmup, a.out)
