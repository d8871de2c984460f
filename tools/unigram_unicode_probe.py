"""What tokenising a predict batch of NON-ASCII texts costs with a Unigram (SentencePiece-style) tokenizer: 256 texts of <= 32
tokens (the BASELINE configs[1] batch shape), ONE process, three legs alternated call by call:

    wrapped  the wrapped tokenizer's call (max_length=32, truncation, padding, return_tensors="pt") + .to(device) of its tensors
             + a device synchronise: what a classifier does without a device tokenizer
    host     HipUnigramTokenizer(hf).__call__, the default routing: every non-ASCII text goes to the wrapped tokenizer and is
             spliced into the batch, the ASCII ones run through ac_unigram_encode
    device   HipUnigramTokenizer(hf, unicode=True).__call__: one H2D of the packed bytes, ac_unigram_encode_utf8, one D2H of the
             lengths

Two batches: every text non-ASCII, and every second text ASCII.  The texts are words of the multilingual lexicon of
tests/unigram_unicode_helpers.py (accented Latin, Greek, Cyrillic, kana, CJK, Hangul, full-width; CJK and kana partly without
spaces, so words of more than 64 bytes occur), the tokenizer its XLM-R style pipeline over the trained "full" vocabulary.  Each
call is timed twice: wall clock around the call and its synchronise, and device events around it.  The ids of the three legs are
compared before anything is timed.

    python tools/unigram_unicode_probe.py [--calls 60] [--warmup 10] [--out FILE]        one JSON line
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, M = 256, 32


def texts_of(n, ascii_every=0):
    import numpy as np
    import unigram_unicode_helpers as H
    from unigram_helpers import WORDS
    rng = np.random.default_rng(7)
    lex = H._lexicon()
    names = [k for k in H.TRAIN_POOLS if k != "ascii"]
    out = []
    for i in range(n):
        if ascii_every and i % ascii_every == 0:
            out.append(" ".join(str(rng.choice(WORDS)) for _ in range(int(rng.integers(4, 22)))))
            continue
        name = names[int(rng.integers(0, len(names)))]
        ws = [lex[name][int(j)] for j in rng.integers(0, 120, int(rng.integers(3, 12)))]
        out.append(("" if name in ("cjk", "kana") and rng.random() < 0.5 else " ").join(ws))
    return out


def main(calls, warmup, out):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "adaptive-classifier_amd"), os.path.join(ROOT, "tests")]
    import torch
    import unigram_unicode_helpers as H
    from adaptive_classifier.tokenizer import HipUnigramTokenizer
    dev = torch.device("cuda:0")
    hf = H.build_tokenizer("full", "xlmr")
    t0 = time.perf_counter()
    plain = HipUnigramTokenizer(hf, device=dev)
    t1 = time.perf_counter()
    uni = HipUnigramTokenizer(hf, device=dev, unicode=True)
    t2 = time.perf_counter()
    assert uni.unicode
    res = {"box": torch.cuda.get_device_name(0), "texts": B, "max_length": M, "calls": calls, "warmup": warmup, "pieces": len(hf),
           "wrapper_build_s": round(t1 - t0, 3), "unicode_wrapper_build_s": round(t2 - t1, 3),
           "unicode_table_bytes": int(sum(t.numel() * t.element_size() for t in uni._ut)),
           "piece_table_bytes": int(sum(t.numel() * t.element_size() for t in uni._t8)), "batches": {}}
    for name, every in (("all_non_ascii", 0), ("every_second_ascii", 2)):
        texts = texts_of(B, every)

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
            assert set(a) == set(other) and all(torch.equal(a[k], other[k]) for k in a), name
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
        res["batches"][name] = {
            "non_ascii_texts": sum(1 for t in texts if not t.isascii()), "tokens": int(a["attention_mask"].sum()),
            "padded_length": int(a["input_ids"].shape[1]), "text_bytes": sum(len(t.encode()) for t in texts),
            "texts_with_a_word_over_64_bytes": sum(1 for t in texts if H.longest_word_bytes(t) > 64),
            "unicode_route_device_texts": on_device, "unicode_route_host_texts": deferred, "default_route_host_texts": routed,
            **{k: {"wall_ms": round(med(wall[k]), 4), "wall_min": round(min(wall[k]), 4), "wall_p90": round(sorted(wall[k])[(9 * calls) // 10], 4),
                   "events_ms": round(med(evt[k]), 4)} for k in legs},
            "device_over_host_wall": round(med(wall["device"]) / med(wall["host"]), 4),
            "device_over_wrapped_wall": round(med(wall["device"]) / med(wall["wrapped"]), 4)}
    line = json.dumps(res)
    print(line)
    if out:
        with open(out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    main(a.calls, a.warmup, a.out)
