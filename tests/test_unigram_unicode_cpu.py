"""CPU side of Unigram on UTF-8 text: csrc/unigram_core.h through ac_unigram_encode_utf8_host (the routines the kernel runs, text by
text on the host) over the probed normalizer table (build_unigram_unicode_tables) and the all-piece table
(build_unigram_tables(utf8=True)) against the tokenizers library, in four pipelines over two multilingual vocabularies and a
hand-made vocabulary of exact ties; the concatenation law the table rests on; malformed input and the buffer edge through the C
entry; the tables and their probe guard; argument validation and the ABI; the kernel's listing; the header under host
sanitizers in a stand-alone program.  No GPU needed, no tolerance anywhere: ids, mask and lengths are compared for equality.

The vocabularies are trained in-process (unigram_unicode_helpers): nothing pretrained is available offline."""
import ctypes
import functools
import os
import re
import shutil
import subprocess
import time

import numpy as np
import pytest

import unigram_unicode_helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "adaptive-classifier_amd", "csrc")


@functools.lru_cache(maxsize=None)
def _random():
    return H.random_texts(3000, 3)


@pytest.fixture(scope="module", params=H.CONFIGS, ids=lambda c: "-".join(c))
def setup(request):
    which, pipeline = request.param
    hf = H.build_tokenizer(which, pipeline)
    return which, pipeline, hf, H.HostTables(hf)


@pytest.fixture(scope="module", params=H.PIPELINES)
def full_setup(request):
    """The pipelines over the full vocabulary: for what does not depend on the vocabulary (the decoder, the normalizer table)."""
    hf = H.build_tokenizer("full", request.param)
    return "full", request.param, hf, H.HostTables(hf)


def _assert_equal(texts, got, want):
    ids, mask, lens = got
    wi, wm, wl = want
    bad = np.nonzero((ids != wi).any(1) | (mask != wm).any(1) | (lens != wl))[0]
    assert len(bad) == 0, [(texts[i][:40], [hex(ord(c)) for c in texts[i][:10]], ids[i, :12].tolist(), wi[i, :12].tolist(), int(lens[i]),
                            int(wl[i])) for i in bad[:3]]


@pytest.mark.parametrize("pipeline", H.PIPELINES)
def test_the_generator_exercises_the_new_route(pipeline):
    """At least 60 % of 3000 generated texts are device texts and at least 20 % of those hold a word of more than 64 bytes:
    otherwise everything below could pass on the host route and the windowed schedule alone."""
    ht = H.HostTables(H.build_tokenizer("full", pipeline))
    texts = _random()
    eligible = [t for t in texts if ht.eligible(t)]
    long_words = [t for t in eligible if H.longest_word_bytes(t) > 64]
    print(pipeline, "eligible", len(eligible), "with a word over 64 bytes", len(long_words))
    assert len(texts) == 3000 and len(eligible) >= 0.6 * len(texts) and len(long_words) >= 0.2 * len(eligible)
    assert sum(1 for t in eligible if not t.isascii()) >= 0.5 * len(texts)


@pytest.mark.parametrize("pipeline", H.PIPELINES)
def test_concatenation_law(pipeline):
    """The law the table rests on, against the real table: for 50 000 random strings of 2-6 code points that are not host-only
    (half of them drawn below U+3100; images that hold whitespace left out, whitespace is the word splitter's business),
    normalize_str(s) is the concatenation of the table's images -- inside a carrier in every pipeline, and without one where
    the chain has no Strip."""
    hf = H.build_tokenizer("full", pipeline)
    tables = H.HostTables(hf).tables
    norm = hf.backend_tokenizer.normalizer.normalize_str
    flagged = np.zeros(0x110000, bool)
    flagged[tables["host_only"]] = True
    flagged[0xD800:0xE000] = True
    ok = np.flatnonzero(~flagged)
    low = ok[ok < 0x3100]
    rng = np.random.default_rng(29)
    image = functools.lru_cache(maxsize=None)(lambda cp: H.table_image(tables, cp))
    done = failures = 0
    while done < 50_000:
        src = low if rng.random() < 0.5 else ok
        cps = [int(src[int(i)]) for i in rng.integers(0, len(src), int(rng.integers(2, 7)))]
        imgs = [image(cp) for cp in cps]
        if any(re.search(r"\s", im) for im in imgs):
            continue
        done += 1
        s, want = "".join(map(chr, cps)), "".join(imgs)
        forms = [("a" + s + "b", "a" + want + "b")] + ([(s, want)] if pipeline.startswith("xlmr") else [])
        for text, expect in forms:
            if norm(text) != expect:
                failures += 1
                if failures <= 3:
                    print(pipeline, [hex(c) for c in cps], repr(norm(text)), repr(expect))
    assert failures == 0, failures


@pytest.mark.parametrize("max_length", [512, 16, 2])
def test_host_entry_equals_the_wrapped_tokenizer(setup, max_length):
    which, pipeline, hf, ht = setup
    texts = H.FIXED + _random()
    eligible = [t for t in texts if ht.eligible(t) and ht.fits(t)]
    assert len(eligible) >= 0.6 * len(texts)
    want = H.reference(hf, eligible, max_length)
    if max_length == 512:
        pieces = (want[1] == 1).sum() - 2 * len(eligible)
        unknown = (want[0] == ht.struct.unk_id).sum()
        print(which, pipeline, "pieces", int(pieces), "unknown", int(unknown))
        if which == "full":                                # not vacuous: well under half of the pieces are unknown
            assert unknown < 0.2 * pieces
        else:                                              # ... and the sparse vocabulary does meet unknowns
            assert 0.1 * pieces < unknown < 0.6 * pieces
    _assert_equal(eligible, H.encode_host(ht, eligible, max_length), want)
    # host-only code points, over 4096 bytes, a normalised text beyond the buffer: not done, the rows untouched
    rest = [t for t in texts if not any(sp in t for sp in ht.specials) and not (ht.eligible(t) and ht.fits(t))]
    assert len(rest) > 100
    ids, mask, lens = H.encode_host(ht, rest, max_length)
    assert (lens == -1).all() and (ids == -7).all() and (mask == -7).all()


def test_named_fixed_cases(setup):
    """The fixed cases do what their comments say, in the wrapped tokenizer (so that they test what they name) and in the host
    entry alike."""
    which, pipeline, hf, ht = setup
    v = ht.struct
    norm = hf.backend_tokenizer.normalizer.normalize_str

    def enc(text, M=512):
        ids, mask, lens = H.encode_host(ht, [text], M)
        wi, wm, wl = H.reference(hf, [text], M)
        assert lens[0] == wl[0] and np.array_equal(ids, wi) and np.array_equal(mask, wm), text
        return ids[0, :lens[0]].tolist()

    # a grapheme cluster / a combining sequence is not a table lookup: the text defers
    ids, mask, lens = H.encode_host(ht, ["\uff21\u0301", "e\u0301", "\uac00\u11a8", "ok"], 16)
    assert lens[:3].tolist() == [-1, -1, -1] and lens[3] > 2 and (ids[:3] == -7).all()
    if pipeline.startswith("xlmr"):                         # Precompiled drops the accent with the cluster: not a per-character map
        assert norm("\uff21\u0301") == "A" and norm("\r\n") == " "
        assert enc("\uff21\uff22\uff23") == enc("ABC")      # full-width forms are their ASCII images (NFKC)
        assert enc("a\u3000b") == enc("a b") != enc("ab")    # U+3000 separates words
        assert H.table_image(ht.tables, 0xFDFA) == norm("\ufdfa") and len(norm("\ufdfa").encode()) == 33
        assert H.table_image(ht.tables, 0x2581) == " "      # the charsmap turns a typed metaspace into a space
    else:                                                   # NFC keeps full-width forms; a typed metaspace is split off: host-only
        assert enc("\uff21\uff22\uff23") != enc("ABC") and H.table_image(ht.tables, 0x2581) is None
        assert H.table_image(ht.tables, 0x3000) is None     # Strip and \s{2,} make U+3000 depend on its place
        assert H.table_image(ht.tables, 0x212B) == ("\u00e5" if pipeline == "deberta_lower" else "\u00c5")    # a singleton: NFC's image
    if pipeline == "deberta_lower":
        assert H.table_image(ht.tables, 0x130) == "i\u0307" and len(enc("\u0130stanbul")) > 3      # a two-code-point case mapping
    # the 99-byte Japanese sentence is one word of 100 bytes: tokenised, not deferred; so is the ~1000-byte one
    assert H.longest_word_bytes(H.CJK_99) == 100 and len(enc(H.CJK_99)) > 3
    assert len(enc(H.LONG_CJK)) > 12
    if which == "full":
        assert v.unk_id not in enc(H.CJK_99)[1:-1]
    # exactly 4096 bytes is done, one more is not; 2048 words
    assert len(enc("\u00e9" * 2048, 24)) == (24 if which == "full" else 4) and len(enc("a " * 2048, 16)) == 16
    assert H.encode_host(ht, ["\u00e9" * 2048 + "a"], 8)[2][0] == -1
    # truncation inside a long word
    assert len(enc(H.LONG_CJK, 8)) == 8 and enc(H.LONG_CJK, 2) == [v.cls_id, v.sep_id] and enc("") == [v.cls_id, v.sep_id]


def test_exact_ties_and_unknowns_of_different_widths():
    """The hand-made vocabulary over multi-byte characters: every segmentation has the same total score, so the pieces show the
    tie rule (earliest start wins); a 3-byte unknown next to a 2-byte unknown is ONE unk_id, and the unknown at a start spans
    the character, not a byte."""
    hf = H.tie_tokenizer()
    ht = H.HostTables(hf)
    ids_of = {p: i for i, (p, _) in enumerate(H.TIE_VOCAB)}
    for text, pieces in H.TIE_ROWS:
        assert hf([text])["input_ids"][0] == [10] + [ids_of[p] for p in pieces] + [11], (text, hf.tokenize(text))
        ids, mask, lens = H.encode_host(ht, [text], 16)
        assert ids[0, :lens[0]].tolist() == [10] + [ids_of[p] for p in pieces] + [11], text
    texts = [t for t, _ in H.TIE_ROWS] + ["éa 文ß a中éa", " ".join(t for t, _ in H.TIE_ROWS), "文" * 70 + "éa"]
    for M in (32, 4):
        _assert_equal(texts, H.encode_host(ht, texts, M), H.reference(hf, texts, M))


@pytest.mark.parametrize("slack", [64, 0])
def test_malformed_utf8_defers(full_setup, slack):
    """Each malformed form as the last bytes of a text (a good text behind it) and as the last bytes of the whole blob: -1 for
    that row, its cells untouched, correct rows on both sides."""
    which, pipeline, hf, ht = full_setup
    good = ["café 中文", "plain ascii", "한국어 \U0001f600"]
    want = H.reference(hf, good, 16)
    for bad in H.MALFORMED:
        for prefix in (b"", b"ab ", "é中".encode()):
            rows = [good[0].encode(), prefix + bad, good[1].encode(), good[2].encode(), prefix + bad]
            ids, mask, lens = H.encode_host(ht, rows, 16, slack)
            assert lens[1] == -1 and lens[4] == -1, (bad, prefix, lens)
            assert (ids[[1, 4]] == -7).all() and (mask[[1, 4]] == -7).all()
            for r, g in ((0, 0), (2, 1), (3, 2)):
                assert lens[r] == want[2][g] and np.array_equal(ids[r], want[0][g]) and np.array_equal(mask[r], want[1][g]), (bad, r)
    # a sequence cut by the text boundary is malformed on both sides: the bytes of the next text are not borrowed
    ids, mask, lens = H.encode_host(ht, [b"a\xc3", b"\xa9b", b"ok"], 16, slack)
    assert lens.tolist()[:2] == [-1, -1] and lens[2] == 3


def test_buffer_edge():
    """Texts whose normalised UTF-8 with the leading 0x20 is one byte short of the buffer, fills it exactly, and exceeds it by
    one: only the last is not done.  Only a compatibility image can grow a text of <= 4096 bytes past the buffer (U+FDFA: 3 ->
    33 bytes under the NFKC charsmap); NFC never does."""
    hf = H.build_tokenizer("full", "xlmr")
    ht = H.HostTables(hf)
    norm = hf.backend_tokenizer.normalizer.normalize_str
    k = (H.BUF - 1) // 33
    texts = ["\ufdfa" * k + "a" * (H.BUF - 2 - 33 * k + r) for r in (0, 1, 2)]
    assert [1 + len(norm(t).encode()) for t in texts] == [H.BUF - 1, H.BUF, H.BUF + 1]
    assert [ht.fits(t) for t in texts] == [True, True, False]
    ids, mask, lens = H.encode_host(ht, texts, 512)
    assert lens[2] == -1 and (ids[2] == -7).all()
    _assert_equal(texts[:2], (ids[:2], mask[:2], lens[:2]), H.reference(hf, texts[:2], 512))
    other = H.HostTables(H.build_tokenizer("full", "deberta"))
    full = ["中" * 1365, "한" * 1365, H.OVERFLOW]
    _assert_equal(full, H.encode_host(other, full, 512), H.reference(other.hf, full, 512))


def test_tables(full_setup):
    which, pipeline, hf, ht = full_setup
    from adaptive_classifier import tokenizer as tkz
    t = ht.tables
    norm = hf.backend_tokenizer.normalizer.normalize_str
    flagged = set(t["host_only"])
    # images round-trip for every code point of the pools (inside the carrier: alone a Unicode space may be stripped)
    for cp in H.WH.pool_code_points():
        img = H.table_image(t, cp)
        assert (img is None and cp in flagged) or "a" + img + "b" == norm("a" + chr(cp) + "b"), hex(cp)
    assert {0x301, 0x1161, 0x11A8} <= flagged                                  # a combining mark, V and T jamo: NFC composes them
    # ZWJ, a variation selector, a Thai vowel sign: extenders of Precompiled's grapheme clusters, nothing to NFC
    assert ({0x200D, 0xFE0F, 0xE31} <= flagged) == pipeline.startswith("xlmr")
    assert not flagged & (set(range(0x20, 0x7F)) | {0x09, 0x0A, 0x0D, 0xE9, 0x4E2D, 0xAC00, 0x3042, 0x1F600, 0x20000})
    print(pipeline, "pages", t["n_pages"], "image bytes", t["image_bytes"], "host-only", len(flagged), t["reasons"], "%.1f s" % t["seconds"])
    # the page bound: at most 256 of the 4352 pages are distinct, the images fit 128 KiB, the longest fits the length field
    assert t["page_of"].shape == (0x1100,) and t["page_of"].dtype == np.uint16 and int(t["page_of"].max()) == t["n_pages"] - 1
    assert t["entries"].shape == (t["n_pages"], 256) and t["entries"].dtype == np.uint32
    assert t["n_pages"] <= 256 and t["image_bytes"] <= 128 * 1024 and len(t["images"]) >= t["image_bytes"]
    lens = (t["entries"] >> 2) & 63
    assert int(lens[(t["entries"] & 3) == 2].max()) == (33 if pipeline.startswith("xlmr") else int(lens.max())) <= 63
    # cached in-process by the serialised normalizer + pre-tokenizer
    assert tkz.build_unigram_unicode_tables(H.build_tokenizer("sparse", pipeline)) is t
    # the probe guard passes on the real tables ...
    spec = dict(ht.spec)
    got = tkz.unigram_unicode_tables(hf, spec)
    assert got is not None and got[0] is t
    probes = tkz._unigram_unicode_probes()
    assert len(probes) >= 40 and any(len(p.encode()) > 64 and " " not in p for p in probes)
    deferred = [p for p in probes if ht.host_only.search(p)]
    assert len(deferred) >= 4 and len(probes) - len(deferred) >= 36
    # ... no probe is compared truncated ...
    _, _, lens = H.encode_host(ht, [p for p in probes if not any(sp in p for sp in ht.specials)], tkz._PROBE_MAX_LENGTH)
    assert int(lens.max()) < tkz._PROBE_MAX_LENGTH
    # ... and a tampered table (one image changed; one flag dropped) trips it: the tokenizer keeps its ASCII-only routing
    for cp in (0xC9 if pipeline == "deberta_lower" else 0x212B, 0x301):
        bad = dict(t, entries=t["entries"].copy(), images=t["images"].copy())
        e = int(bad["entries"][int(bad["page_of"][cp >> 8]), cp & 255])
        if cp == 0x301:
            assert e & 3 == 3
            bad["entries"][int(bad["page_of"][cp >> 8]), cp & 255] = 0           # "itself": the combining acute would go through
            bad["host_only"] = [c for c in t["host_only"] if c != cp]
        else:
            assert e & 3 == 2
            bad["images"][e >> 8] ^= 1
        assert tkz._unigram_unicode_matches(hf, spec, (ht.arrays, ht.slots), t, probes)
        assert not tkz._unigram_unicode_matches(hf, spec, (ht.arrays, ht.slots), bad, probes), hex(cp)
        key, = [k for k, v in tkz._UNI_UNICODE_CACHE.items() if v is t]
        tkz._UNI_UNICODE_CACHE[key] = bad
        try:
            assert tkz.unigram_unicode_tables(hf, dict(ht.spec)) is None
        finally:
            tkz._UNI_UNICODE_CACHE[key] = t


def test_a_table_that_points_outside_reads_as_host_only():
    hf = H.build_tokenizer("full", "xlmr")
    ht = H.HostTables(hf)
    t = ht.tables
    text = ["Å ok", "plain"]
    assert H.encode_host(ht, text, 8)[2].min() > 2
    short = H.HostTables(hf, dict(t, image_bytes=1))                              # every image but a 1-byte one at offset 0 lies outside
    assert H.encode_host(short, text, 8)[2][0] == -1
    pages = t["page_of"].copy()
    pages[0x21] = t["n_pages"]                                                    # the page of U+212B: a page number past the table
    assert H.encode_host(H.HostTables(hf, dict(t, page_of=pages)), text, 8)[2].tolist()[0] == -1


def test_all_piece_table():
    """build_unigram_tables(spec, utf8=True): every piece as UTF-8 bytes under ac_unigram_hash, only unmatchable ones left out;
    the default call's result is what it was; a storable piece of more than 64 bytes keeps the Unicode route off."""
    from adaptive_classifier import _native as nv
    from adaptive_classifier import tokenizer as tkz
    hf = H.build_tokenizer("full", "xlmr")
    spec = tkz._unigram_spec(hf)
    default = spec.pop("tables")
    max_ascii = spec["max_piece"]
    (keys, entries, scores, blob), slots = tkz.build_unigram_tables(spec, utf8=True)
    again = tkz.build_unigram_tables(spec)
    assert spec["max_piece"] == max_ascii and all(np.array_equal(a, b) for a, b in zip(default[0], again[0])) and default[1] == again[1]
    stored = {}
    for s in np.flatnonzero(keys):
        raw = bytes(blob[entries[s, 2]:entries[s, 2] + entries[s, 1]])
        assert int(keys[s]) == nv.lib().ac_unigram_hash((ctypes.c_uint8 * len(raw)).from_buffer_copy(raw), len(raw))
        stored[raw.decode("utf-8")] = (int(entries[s, 0]), float(scores[s]))
    want = {}
    for i, (p, sc) in enumerate(spec["vocab"]):
        q = " " + p[1:] if p[:1] == "▁" else p
        if q and " " not in p and "▁" not in q and not any(ord(ch) < 0x20 or ord(ch) == 0x7F for ch in q):
            want[q] = (i, sc)
    assert stored == want and sum(1 for q in stored if not q.isascii()) > 2000
    assert spec["max_piece_utf8"] == max(len(q.encode()) for q in stored) <= H.REACH and slots >= 2 * len(stored)
    # unmatchable pieces stay out; a piece over the reach turns the route off
    odd = {"vocab": [("<unk>", 0.0), ("▁", -1.0), ("a b", -1.0), ("a▁b", -1.0), ("\x01", -1.0), ("é", -1.0), ("▁中", -2.0)]}
    (k2, e2, _, b2), _ = tkz.build_unigram_tables(odd, utf8=True)
    assert sorted(bytes(b2[e2[s, 2]:e2[s, 2] + e2[s, 1]]).decode() for s in np.flatnonzero(k2)) == [" ", " 中", "<unk>", "é"]
    assert odd["max_piece_utf8"] == 5
    long_spec = dict(spec, vocab=list(spec["vocab"]) + [("中" * 22, -20.0)])         # 66 bytes
    assert tkz.unigram_unicode_tables(hf, long_spec) is None and long_spec["max_piece_utf8"] == 66
    assert tkz.unigram_unicode_tables(hf, dict(spec)) is not None


def test_a_250k_piece_vocabulary_builds_in_seconds():
    from adaptive_classifier.tokenizer import build_unigram_tables
    rng = np.random.default_rng(3)
    letters = np.array(list("abcdefghijklmnopqrstuvwxyz"))
    words = {"".join(rng.choice(letters, int(n))) for n in rng.integers(1, 12, 300_000)}
    vocab = [("<unk>", 0.0)] + [(("▁" if i % 3 == 0 else "") + w, -float(i % 97) - 1.0) for i, w in enumerate(sorted(words))]
    vocab += [(("▁" if i % 2 else "") + "中%dé" % i, -12.0) for i in range(20_000)]
    assert len(vocab) >= 250_000
    spec = {"vocab": vocab}
    t0 = time.perf_counter()
    (keys, entries, scores, blob), slots = build_unigram_tables(spec, utf8=True)
    took = time.perf_counter() - t0
    print("250k pieces, utf8=True: %.2f s" % took)
    assert np.count_nonzero(keys) == len(vocab) and len(np.unique(entries[keys != 0, 0])) == len(vocab)
    assert took < 20.0, took                               # the bound only catches per-piece Python probing


def test_argument_validation_and_abi():
    from adaptive_classifier import _native as nv
    from adaptive_classifier import tokenizer as tkz
    L = nv.lib()
    assert L.ac_version() >= 15
    header = open(os.path.join(ROOT, "include", "acamd.h")).read()
    for name in ("ac_unigram_encode_utf8", "ac_unigram_encode_utf8_host", "ac_unigram_encode", "ac_unigram_encode_host", "ac_unigram_hash"):
        assert re.search(r"\b%s\s*\(" % name, header) and hasattr(L, name) and name in nv.exported_symbols(), name
    fields = re.search(r"typedef struct ac_unigram_unicode \{(.*?)\} ac_unigram_unicode;", header, re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    assert re.findall(r"(\w+)\s*[;,]", fields) == [f for f, _ in nv.ac_unigram_unicode._fields_]
    assert ctypes.sizeof(nv.ac_unigram_unicode) == 3 * ctypes.sizeof(ctypes.c_void_p) + 8
    ht = H.HostTables(H.build_tokenizer("full", "xlmr"))
    blob, offs = H.pack([b"ab", b"c"])
    ids, mask, lens = np.zeros((2, 8), np.int64), np.zeros((2, 8), np.int64), np.zeros(2, np.int32)
    p = lambda a: a.ctypes.data                                                          # noqa: E731

    def both(text, offsets, b, vocab, uni, M, i, m, n):
        v = ctypes.byref(vocab) if vocab is not None else None
        u = ctypes.byref(uni) if uni is not None else None
        return (L.ac_unigram_encode_utf8(text, offsets, b, v, u, M, i, m, n, None),
                L.ac_unigram_encode_utf8_host(text, offsets, b, v, u, M, i, m, n))

    EINVAL = -1
    V, U = ht.struct, ht.unicode
    assert both(p(blob), p(offs), 2, None, U, 8, p(ids), p(mask), p(lens)) == (EINVAL, EINVAL)
    assert both(p(blob), p(offs), 2, V, None, 8, p(ids), p(mask), p(lens)) == (EINVAL, EINVAL)
    assert both(p(blob), None, 2, V, U, 8, p(ids), p(mask), p(lens)) == (EINVAL, EINVAL)
    assert both(p(blob), p(offs), 2, V, U, 8, None, p(mask), p(lens)) == (EINVAL, EINVAL)
    assert both(p(blob), p(offs), 2, V, U, 8, p(ids), None, p(lens)) == (EINVAL, EINVAL)
    assert both(p(blob), p(offs), 2, V, U, 8, p(ids), p(mask), None) == (EINVAL, EINVAL)
    assert both(p(blob), p(offs), 2, V, U, 1, p(ids), p(mask), p(lens)) == (EINVAL, EINVAL)          # max_length < 2
    assert both(p(blob), p(offs), -1, V, U, 8, p(ids), p(mask), p(lens)) == (EINVAL, EINVAL)
    assert both(None, p(offs), 2, V, U, 8, p(ids), p(mask), p(lens)) == (EINVAL, EINVAL)             # text NULL with b > 0
    assert b"unigram utf8" in L.ac_last_error()
    ptrs = [a.ctypes.data for a in ht.arrays]
    odd = tkz.unigram_vocab_struct(ht.spec, ptrs, ht.slots - 1, utf8=True)                           # not a power of two
    assert both(p(blob), p(offs), 2, odd, U, 8, p(ids), p(mask), p(lens)) == (EINVAL, EINVAL)
    for hole in range(4):
        holes = tkz.unigram_vocab_struct(ht.spec, [None if i == hole else q for i, q in enumerate(ptrs)], ht.slots, utf8=True)
        assert both(p(blob), p(offs), 2, holes, U, 8, p(ids), p(mask), p(lens)) == (EINVAL, EINVAL)
    far = tkz.unigram_vocab_struct(dict(ht.spec, max_piece_utf8=65), ptrs, ht.slots, utf8=True)     # beyond the kernel's reach
    assert both(p(blob), p(offs), 2, far, U, 8, p(ids), p(mask), p(lens)) == (EINVAL, EINVAL)
    t = ht.tables
    for broken in (nv.ac_unigram_unicode(None, p(t["entries"]), p(t["images"]), t["n_pages"], t["image_bytes"]),
                   nv.ac_unigram_unicode(p(t["page_of"]), None, p(t["images"]), t["n_pages"], t["image_bytes"]),
                   nv.ac_unigram_unicode(p(t["page_of"]), p(t["entries"]), None, t["n_pages"], t["image_bytes"]),
                   nv.ac_unigram_unicode(p(t["page_of"]), p(t["entries"]), p(t["images"]), 0, t["image_bytes"])):
        assert both(p(blob), p(offs), 2, V, broken, 8, p(ids), p(mask), p(lens)) == (EINVAL, EINVAL)
    assert both(None, p(offs), 0, V, U, 8, p(ids), p(mask), p(lens)) == (0, 0)                       # b == 0: nothing to do
    assert L.ac_unigram_encode_utf8_host(p(blob), p(offs), 2, ctypes.byref(V), ctypes.byref(U), 8, p(ids), p(mask), p(lens)) == 0
    assert lens.min() >= 3


def test_utf8_kernel_has_no_scratch():
    """No private segment, at most 128 VGPRs (the bound the other tokenizer kernels are held to); the kernel's name does not
    contain the ASCII kernel's."""
    from test_kernel_resources_cpu import HIPCC, kernel_resources
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    res = kernel_resources("unigram_utf8.hip")
    new = {k: v for k, v in res.items() if "unigram_utf8_kernel" in k}
    assert len(new) == 1 and not any("unigram_kernel" in k for k in res), res
    (scratch, vgpr), = new.values()
    print("unigram_utf8_kernel: scratch", scratch, "VGPRs", vgpr)
    assert scratch == 0 and vgpr <= 128, (scratch, vgpr)


SANITIZER_MAIN = r"""
// stand-alone: csrc/unigram_core.h over dumped tables and texts (unigram_unicode_helpers.dump), one line per text: its ids, or -1
#include <cstdio>
#include <cstring>
#include <vector>
#include "unigram_core.h"
template <class T> static bool rd(FILE* f, std::vector<T>& v) { return v.empty() || fread(v.data(), sizeof(T), v.size(), f) == v.size(); }
int main(int argc, char** argv) {
    FILE* f = argc > 1 ? fopen(argv[1], "rb") : nullptr;
    if (!f) return 2;
    int32_t hd[16];
    double unk_score;
    if (fread(hd, 4, 16, f) != 16 || fread(&unk_score, 8, 1, f) != 1) return 2;
    const int slots = hd[0], blob_len = hd[1], b = hd[2], text_len = hd[3], M = hd[4], max_piece = hd[5], unk = hd[6];
    const int trailing = hd[10], ws_controls = hd[11], n_pages = hd[12], image_bytes = hd[13];
    // exact-size heap blocks: a read past any table, past a text's end, past the normalisation buffer or a work array is a report
    std::vector<uint64_t> keys(slots);
    std::vector<int32_t> entries(4 * (size_t)slots), offs(b + 1);
    std::vector<double> scores(slots);
    std::vector<uint16_t> page_of(unigram::kPages);
    std::vector<uint32_t> uentries(256 * (size_t)n_pages);
    std::vector<uint8_t> blob(blob_len), images(image_bytes), text(text_len);
    const bool ok = rd(f, keys) && rd(f, entries) && rd(f, scores) && rd(f, blob) && rd(f, page_of) && rd(f, uentries) && rd(f, images) &&
                    rd(f, offs) && rd(f, text);
    fclose(f);
    if (!ok) return 2;
    const unigram::Table t{keys.data(), entries.data(), scores.data(), blob.data(), (uint32_t)(slots - 1)};
    const unigram::Unicode u{page_of.data(), uentries.data(), images.data(), n_pages, image_bytes};
    bool aligned = true;
    for (int tx = 0; tx < b; ++tx) {
        const int n = offs[tx + 1] - offs[tx];
        std::vector<uint8_t> one(text.begin() + offs[tx], text.begin() + offs[tx + 1]);        // the text alone in its own block
        std::vector<uint8_t> buf(unigram::kUtf8BufBytes);
        std::vector<int64_t> out(M - 2);
        std::vector<double> best(unigram::kUtf8BufBytes + 1);
        std::vector<int32_t> w1(unigram::kUtf8BufBytes + 1), w2(unigram::kUtf8BufBytes + 1), w3(unigram::kUtf8BufBytes + 1);
        const int k = unigram::encode_text_utf8(u, t, max_piece, unk_score, unk, trailing, ws_controls, one.data(), n, buf.data(),
                                                unigram::kUtf8BufBytes, M - 2, out.data(), best.data(), w1.data(), w2.data(), w3.data(),
                                                &aligned);
        if (k < 0) { printf("-1\n"); continue; }
        printf("%d", hd[7]);
        for (int i = 0; i < k; ++i) printf(" %lld", (long long)out[i]);
        printf(" %d\n", hd[8]);
    }
    return aligned ? 0 : 3;
}
"""


def _host_compiler():
    for cand in ("/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++", shutil.which("amdclang++"), shutil.which("clang++")):
        if cand and os.path.exists(cand):
            return cand
    return None


@pytest.mark.skipif(_host_compiler() is None, reason="no clang++ found")
@pytest.mark.parametrize("which,pipeline", [("sparse", "xlmr_legacy"), ("full", "deberta_lower")])
def test_core_header_under_host_sanitizers(tmp_path, which, pipeline):
    """unigram_core.h as plain C++ in a stand-alone program built with -fsanitize=address,undefined: clean, the same ids /
    not-done rows as the library, and the wrapped tokenizer's ids for the device texts.  The tables, every text, the
    normalisation buffer and every work array sit in exact-size heap blocks; the malformed, the buffer-edge and the block-edge
    texts are in."""
    hf = H.build_tokenizer(which, pipeline)
    ht = H.HostTables(hf)
    texts = [t for t in H.FIXED + H.random_texts(400, 23) if not any(sp in t for sp in ht.specials)]
    raws = H.raw(texts) + [p + bad for bad in H.MALFORMED for p in (b"", b"ab ")] + H.raw(["\ufdfa" * 155 + "a" * r for r in (3, 4, 5)])
    M = 24
    data = str(tmp_path / "unigram_utf8.bin")
    H.dump(ht, raws, M, data)
    src, exe = tmp_path / "unigram_utf8_main.cpp", str(tmp_path / "unigram_utf8_main")
    src.write_text(SANITIZER_MAIN)
    subprocess.run([_host_compiler(), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover",
                    "-I", CSRC, str(src), "-o", exe], check=True, capture_output=True, text=True)
    run = subprocess.run([exe, data], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    ids, _, lens = H.encode_host(ht, raws, M)
    want = ["-1" if lens[i] < 0 else " ".join(str(x) for x in ids[i, :lens[i]]) for i in range(len(raws))]
    assert sum(1 for w in want if w == "-1") >= 2 * len(H.MALFORMED) + 1
    lines = run.stdout.strip("\n").split("\n")
    assert lines == want
    done = [i for i, t in enumerate(texts) if ht.eligible(t) and ht.fits(t)]
    assert len(done) > 300
    wi, wm, wl = H.reference(hf, [texts[i] for i in done], M)
    assert [lines[i] for i in done] == [" ".join(str(x) for x in wi[j, :wl[j]]) for j in range(len(done))]
