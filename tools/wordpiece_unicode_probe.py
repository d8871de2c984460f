"""What tokenising a predict batch of Unicode text costs with a WordPiece tokenizer, host route against device route: 256 texts of
<= 32 tokens (the BASELINE configs[1] batch shape), ONE process, the two legs alternated call by call:

    host     HipWordPieceTokenizer(hf) -- every non-ASCII text goes to the wrapped tokenizer and is spliced back in (today's
             default), the ASCII texts of the batch through ac_wordpiece_encode
    device   HipWordPieceTokenizer(hf, unicode=True) -- one H2D of the packed bytes, ac_wordpiece_encode_utf8, one D2H of the
             lengths

and, for scale, `plain`: the wrapped tokenizer's own call + .to(device) of its tensors (no device tokenizer at all).  Two
batches: `non_ascii` (every text holds non-ASCII characters: Latin with accents, Cyrillic, Greek, CJK, kana, Hangul) and `mixed`
(every second text plain ASCII).  Each call is timed twice: wall clock around the call and its synchronise, and device events
around it.  The vocabulary is the synthetic multilingual one of tests/wordpiece_helpers.py (accent-stripping, lower-casing
configuration).  The ids of the legs are compared before anything is timed; the table build time at construction is reported.

    python tools/wordpiece_unicode_probe.py [--calls 60] [--warmup 10] [--out FILE]        one JSON line
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, M = 256, 32


def texts_of(n, every_other_ascii):
    import numpy as np
    import wordpiece_helpers as H
    rng = np.random.default_rng(7)
    scripts = [cps for name, cps, _ in H.POOLS if name in ("latin", "greek", "cyrillic", "kana", "cjk", "hangul")]
    pieces = [t for t in H.vocab() if t not in H.SPECIALS and not t.startswith("##") and len(t) > 1 and not t.isascii()]
    out = []
    for i in range(n):
        if every_other_ascii and i % 2:
            out.append(" ".join(H.WORDS[int(j)] for j in rng.integers(0, len(H.WORDS), int(rng.integers(4, 16)))) + ".")
            continue
        cps = scripts[int(rng.integers(0, len(scripts)))]
        ws = []
        for _ in range(int(rng.integers(3, 9))):
            if rng.random() < 0.6:
                ws.append(pieces[int(rng.integers(0, len(pieces)))])
            else:
                ws.append("".join(chr(cps[int(j)]) for j in rng.integers(0, len(cps), int(rng.integers(1, 4)))))
        out.append(" ".join(ws) + ".")
    return out


def main(calls, warmup, out):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "adaptive-classifier_amd"), os.path.join(ROOT, "tests")]
    import torch
    import wordpiece_helpers as H
    from adaptive_classifier import tokenizer as tkz
    dev = torch.device("cuda:0")
    hf = H.build_tokenizer("uncased")
    t0 = time.perf_counter()
    host_tok = tkz.HipWordPieceTokenizer(hf, device=dev)
    ascii_build_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    dev_tok = tkz.HipWordPieceTokenizer(hf, device=dev, unicode=True)
    unicode_build_s = time.perf_counter() - t0
    assert dev_tok.unicode
    tables = tkz.build_wordpiece_unicode_tables(hf)
    t0 = time.perf_counter()
    tkz.HipWordPieceTokenizer(hf, device=dev, unicode=True)
    cached_build_s = time.perf_counter() - t0
    res = {"box": torch.cuda.get_device_name(0), "texts": B, "max_length": M, "calls": calls, "warmup": warmup, "pieces": len(H.vocab()),
           "table_sweep_s": round(tables["seconds"], 3), "table_pages": tables["n_pages"], "table_image_bytes": tables["image_bytes"],
           "table_bytes": int(tables["page_of"].nbytes + tables["entries"].nbytes + tables["image_bytes"]),
           "host_only_code_points": len(tables["host_only"]), "wrapper_build_s": round(ascii_build_s, 3),
           "wrapper_build_unicode_s": round(unicode_build_s, 3), "wrapper_build_unicode_cached_s": round(cached_build_s, 3), "batches": {}}
    for name, mixed in (("non_ascii", False), ("mixed", True)):
        texts = texts_of(B, mixed)

        def plain():
            enc = hf(texts, max_length=M, truncation=True, padding=True, return_tensors="pt")
            return {k: v.to(dev) for k, v in enc.items()}

        def host():
            return host_tok(texts, max_length=M, truncation=True, padding=True, return_tensors="pt")

        def device():
            return dev_tok(texts, max_length=M, truncation=True, padding=True, return_tensors="pt")

        a, b, c = plain(), host(), device()
        assert set(a) == set(b) == set(c) and all(torch.equal(a[k], b[k]) and torch.equal(a[k], c[k]) for k in a), name
        before = (dev_tok.device_texts, dev_tok.host_texts, host_tok.host_texts)
        legs = {"host": host, "device": device, "plain": plain}
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
        n = warmup + calls
        res["batches"][name] = {
            "non_ascii_texts": sum(1 for t in texts if not t.isascii()), "tokens": int(a["attention_mask"].sum()),
            "unk_share": round(float((a["input_ids"] == hf.unk_token_id).sum()) / float(a["attention_mask"].sum() - 2 * B), 3),
            "padded_length": int(a["input_ids"].shape[1]),
            "device_leg_host_texts_per_call": (dev_tok.host_texts - before[1]) / n,
            "host_leg_host_texts_per_call": (host_tok.host_texts - before[2]) / n,
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
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    main(a.calls, a.warmup, a.out)
