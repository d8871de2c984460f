"""CPU side of the Unigram device tokenizer: csrc/unigram_core.h through ac_unigram_encode_host (the routines the kernel runs,
text by text on the host) against the wrapped transformers tokenizers, the hand-made vocabulary of exact score ties, the piece
hash, tokenizer recognition (_unigram_spec and its probe guard), argument validation, the kernel's resource counts, and the
same header under host sanitizers in a stand-alone program.  No GPU needed.

The vocabularies are trained in-process (unigram_helpers): no pretrained vocabulary is available offline."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import unigram_helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "adaptive-classifier_amd", "csrc")
CONTROL_BYTE_TEXTS = [t for t in H.FIXED if any(ord(c) < 0x20 and c not in "\t\n\r" or ord(c) == 0x7f for c in t)]


@pytest.fixture(scope="module", params=H.CONFIGS, ids=["-".join(c) for c in H.CONFIGS])
def setup(request):
    which, pipeline = request.param
    hf = H.build_tokenizer(which, pipeline)
    hv = H.HostVocab(hf)
    assert hv.spec["ws_controls"]                          # the four pipelines treat \t \n \r as plain whitespace
    texts = [t for t in H.FIXED + H.random_texts(3000, 11) if H.eligible(t, hv.spec["specials"])]
    return request.param, hf, hv, texts


@pytest.mark.parametrize("max_length", [512, 24, 8, 2])
def test_host_encode_equals_the_wrapped_tokenizer(setup, max_length):
    """ids, mask and lengths identical to the wrapped tokenizer called as the classifier calls it, on every device-eligible
    text of the set: no tolerance.  The two words of more than 64 bytes are among them: only the kernel defers those."""
    _, hf, hv, texts = setup
    assert len(CONTROL_BYTE_TEXTS) == 2 and len(texts) >= 2300
    for t in H.FIXED:                                      # none of the fixed cases is lost to routing without a reason
        assert t in texts or t in CONTROL_BYTE_TEXTS, t
    assert "x" * 300 in texts and "q" * 4096 in texts
    want = hf(texts, max_length=max_length, truncation=True, padding=True, return_tensors="np")
    ids, mask, lens = H.encode_host(hv, texts, max_length)
    S = want["input_ids"].shape[1]
    bad = np.nonzero((ids[:, :S] != want["input_ids"]).any(1) | (mask[:, :S] != want["attention_mask"]).any(1))[0]
    assert len(bad) == 0, [(texts[i][:60], ids[i, :S].tolist()[:16], want["input_ids"][i].tolist()[:16]) for i in bad[:3]]
    assert (ids[:, S:] == hv.spec["pad_id"]).all() and (mask[:, S:] == 0).all()
    assert np.array_equal(lens, want["attention_mask"].sum(1)) and int(lens.max()) == S


def test_the_sparse_vocabulary_exercises_unknowns(setup):
    """Without an initial alphabet most texts hold an unknown character, so fusing is checked for real; with the full
    alphabet none does."""
    (which, _), hf, hv, texts = setup
    ids, _, _ = H.encode_host(hv, texts, 512)
    share = float((ids[:, 1:] == hv.spec["unk_id"]).any(1).mean())
    assert share > 0.5 if which == "sparse" else share == 0.0, share


def test_exact_ties_resolve_as_the_library_does():
    """The hand-made vocabulary: every segmentation of "ab", "abc" ... has the same total score, so the pieces show the tie
    rule (earliest start wins, a later proposal only when strictly greater) and the per-word fusing of unknowns."""
    hf = H.tie_tokenizer()
    hv = H.HostVocab(hf)
    texts = [t for t, _ in H.TIE_ROWS]
    ids, _, lens = H.encode_host(hv, texts, 16)
    want = hf(texts, max_length=16, truncation=True, padding=True, return_tensors="np")["input_ids"]
    for i, (text, pieces) in enumerate(H.TIE_ROWS):
        row = ids[i, :lens[i]].tolist()
        assert hf.convert_ids_to_tokens(row[1:-1]) == pieces, (text, row)
        assert row == want[i, :lens[i]].tolist() and (want[i, lens[i]:] == hv.spec["pad_id"]).all(), text
    # unknowns of different words do not fuse
    ids, _, lens = H.encode_host(hv, ["X Y"], 16)
    assert hf.convert_ids_to_tokens(ids[0, 1:lens[0] - 1].tolist()) == ["▁", "<unk>", "▁", "<unk>"]
    assert ids[0, :lens[0]].tolist() == hf("X Y")["input_ids"]


def test_hash_is_the_finished_polynomial():
    from adaptive_classifier import _native as nv
    from adaptive_classifier.tokenizer import _unigram_hash_rows
    M64 = 0xffffffffffffffff

    def restated(raw):
        p = 0
        for c in raw:
            p = (p * 0x9e3779b97f4a7c15 + c + 1) & M64
        p ^= p >> 29
        p = (p * 0xbf58476d1ce4e5b9) & M64
        p ^= p >> 32
        return p or 1

    def native(raw):
        return nv.lib().ac_unigram_hash((ctypes.c_uint8 * max(1, len(raw))).from_buffer_copy(raw or b"\0"), len(raw))

    cases = [b"", b"a", b" a", b"a ", b" the", b"ab", b"ba", bytes(range(0x20, 0x7f)), b"\x00", b"\x00\x00", bytes(range(256))]
    for raw in cases:
        assert native(raw) == restated(raw), raw
    assert len({native(r) for r in cases}) == len(cases)
    # the table builder's vectorised form, and the O(1) range form the kernel uses: prefix[t] - prefix[s] * B^(t - s)
    width = max(map(len, cases))
    mat = np.zeros((len(cases), width), np.uint8)
    for i, raw in enumerate(cases):
        mat[i, :len(raw)] = np.frombuffer(raw, np.uint8)
    assert _unigram_hash_rows(mat, np.array([len(r) for r in cases])).tolist() == [restated(r) for r in cases]
    word = b" tokenization"
    prefix = [0]
    for c in word:
        prefix.append((prefix[-1] * 0x9e3779b97f4a7c15 + c + 1) & M64)
    for s in range(len(word)):
        for t in range(s + 1, len(word) + 1):
            p = (prefix[t] - prefix[s] * pow(0x9e3779b97f4a7c15, t - s, 1 << 64)) & M64
            p ^= p >> 29
            p = (p * 0xbf58476d1ce4e5b9) & M64
            p ^= p >> 32
            assert (p or 1) == native(word[s:t])


def test_table_holds_exactly_the_matchable_pieces():
    """Pure-ASCII pieces with the metaspace in front as 0x20; everything that can match no eligible word is left out; every
    stored piece is found where linear probing looks for it."""
    from adaptive_classifier.tokenizer import build_unigram_tables
    vocab = [("<unk>", 0.0), ("▁", -1.0), ("▁the", -2.0), ("the", -2.5), ("café", -3.0), ("a▁b", -3.0), ("▁▁", -3.0),
             ("a b", -3.5), ("tab\t", -3.0), ("\x7f", -3.0), ("", -9.0), ("T", -4.0), ("▁é", -30.0)]
    spec = {"vocab": vocab}
    (keys, entries, scores, blob), slots = build_unigram_tables(spec)
    assert spec["max_piece"] == 5 and spec["unk_score"] == -40.0          # <unk> is 5 bytes; the minimum is over ALL pieces
    stored = {}
    for s in np.flatnonzero(keys):
        tid, n, off, zero = entries[s]
        stored[bytes(blob[off:off + n])] = (int(tid), float(scores[s]))
        assert zero == 0
    assert stored == {b"<unk>": (0, 0.0), b" ": (1, -1.0), b" the": (2, -2.0), b"the": (3, -2.5), b"T": (11, -4.0)}
    mask = slots - 1
    for s in np.flatnonzero(keys):
        h = int(keys[s])
        home = (h ^ (h >> 32)) & mask
        assert all(keys[(home + d) & mask] != 0 for d in range((int(s) - home) & mask)), s
    assert slots & mask == 0 and np.count_nonzero(keys) * 2 <= slots


def test_a_piece_longer_than_the_dense_width_is_stored_and_found():
    """Pieces of more than 64 bytes stay out of the dense hashing matrix (one of them must not cost pieces x length bytes) but
    are in the table under the same hash, and the host entry matches them inside a word of that length."""
    from adaptive_classifier import _native as nv
    from adaptive_classifier.tokenizer import build_unigram_tables, unigram_vocab_struct
    long_piece = "y" * 200
    spec = {"vocab": [("<unk>", 0.0), ("▁", -1.0), ("y", -5.0), (long_piece, -2.0), ("▁" + "z" * 65, -2.0)],
            "unk_id": 0, "cls_id": 7, "sep_id": 8, "pad_id": 9, "lowercase": False, "trailing_space_piece": False, "ws_controls": True}
    (keys, entries, scores, blob), slots = build_unigram_tables(spec)
    assert spec["max_piece"] == 200
    raw = long_piece.encode()
    h = nv.lib().ac_unigram_hash((ctypes.c_uint8 * len(raw)).from_buffer_copy(raw), len(raw))
    s, = np.flatnonzero(keys == np.uint64(h))
    assert entries[s].tolist()[:2] == [3, 200] and bytes(blob[entries[s, 2]:entries[s, 2] + 200]) == raw
    vocab = unigram_vocab_struct(spec, [a.ctypes.data for a in (keys, entries, scores, blob)], slots)
    text, offs = H.pack([long_piece, "z" * 65])
    ids, mask, lens = np.zeros((2, 8), np.int64), np.zeros((2, 8), np.int64), np.zeros(2, np.int32)
    assert nv.lib().ac_unigram_encode_host(text.ctypes.data, offs.ctypes.data, 2, ctypes.byref(vocab), 8, ids.ctypes.data,
                                           mask.ctypes.data, lens.ctypes.data) == 0
    assert ids[0, :lens[0]].tolist() == [7, 1, 3, 8] and ids[1, :lens[1]].tolist() == [7, 4, 8]


def test_a_250k_piece_vocabulary_builds_in_seconds():
    import time
    from adaptive_classifier.tokenizer import build_unigram_tables
    rng = np.random.default_rng(3)
    letters = np.array(list("abcdefghijklmnopqrstuvwxyz"))
    words = {"".join(rng.choice(letters, int(n))) for n in rng.integers(1, 12, 300_000)}
    vocab = [("<unk>", 0.0)] + [(("▁" if i % 3 == 0 else "") + w, -float(i % 97) - 1.0) for i, w in enumerate(sorted(words))]
    vocab += [("中%d" % i, -12.0) for i in range(20_000)]                  # non-ASCII pieces: skipped
    assert len(vocab) >= 250_000
    t0 = time.perf_counter()
    (keys, entries, scores, blob), slots = build_unigram_tables({"vocab": vocab})
    took = time.perf_counter() - t0
    n_ascii = len(vocab) - 20_000
    assert np.count_nonzero(keys) == n_ascii and len(np.unique(entries[keys != 0, 0])) == n_ascii
    assert took < 20.0, took                               # about a second here; the bound only catches per-piece Python probing


def test_unigram_spec_recognition():
    """Recognised by the serialised configuration plus the probe guard: the four pipelines are taken, everything else is
    left alone, and the two older recognisers do not take them."""
    from tokenizers import Regex, normalizers, pre_tokenizers
    from transformers import BertTokenizer
    from adaptive_classifier.tokenizer import _bpe_spec, _unigram_spec, _unigram_structure, _wordpiece_spec
    import bpe_helpers
    for which, pipeline in H.CONFIGS:
        hf = H.build_tokenizer(which, pipeline)
        spec = _unigram_spec(hf)
        assert spec is not None, (which, pipeline)
        assert spec["lowercase"] == (pipeline == "deberta_lower")
        assert spec["trailing_space_piece"] == (pipeline == "xlmr_legacy")
        assert spec["token_type_ids"] == pipeline.startswith("deberta")
        assert (spec["unk_id"], spec["cls_id"], spec["sep_id"], spec["pad_id"]) == ((3, 1, 2, 0) if pipeline.startswith("deberta")
                                                                                    else (3, 0, 2, 1))
        assert spec["ws_controls"] is True and hf.sep_token in spec["specials"]
        assert _wordpiece_spec(hf) is None and _bpe_spec(hf) is None

    vocab = H._xlmr_vocab(H.trained_pieces("sparse"))
    meta = lambda scheme="always": pre_tokenizers.Metaspace(replacement="▁", prepend_scheme=scheme)      # noqa: E731
    assert _unigram_spec(H.legacy_tokenizer(vocab)) is not None                            # the base the variants depart from
    assert _unigram_spec(H.legacy_tokenizer(vocab, pre_tokenizer=pre_tokenizers.Sequence(
        [pre_tokenizers.WhitespaceSplit(), meta()]), normalizer=None)) is not None
    assert _unigram_spec(H.legacy_tokenizer(vocab, byte_fallback=True)) is None
    assert _unigram_spec(H.legacy_tokenizer(vocab, unk_id=None)) is None
    assert _unigram_spec(H.legacy_tokenizer(vocab, pre_tokenizer=meta("first"))) is None
    assert _unigram_spec(H.legacy_tokenizer(vocab, pre_tokenizer=pre_tokenizers.Sequence(
        [pre_tokenizers.WhitespaceSplit(), pre_tokenizers.Punctuation(), meta()]))) is None
    assert _unigram_spec(H.legacy_tokenizer(vocab, padding_side="left")) is None
    assert _unigram_spec(H.legacy_tokenizer(vocab, pad_token=None)) is None
    assert _unigram_spec(H.legacy_tokenizer(vocab, normalizer=None)) is None               # nothing collapses runs of spaces
    assert _unigram_spec(H.legacy_tokenizer(vocab, normalizer=normalizers.Sequence(
        [normalizers.Replace("``", '"'), normalizers.Replace(Regex(" {2,}"), " ")]))) is None          # ALBERT's quote replacement
    assert _unigram_spec(H.legacy_tokenizer(vocab, normalizer=normalizers.Sequence(
        [normalizers.Replace("a", "b"), normalizers.Replace(Regex(" {2,}"), " ")]))) is None
    assert _unigram_spec(bpe_helpers.build_tokenizer("roberta")) is None
    bert_vocab = {t: i for i, t in enumerate(["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]", "a", "b", "##a"])}
    bert = BertTokenizer(vocab=bert_vocab, do_lower_case=True)
    assert _unigram_spec(bert) is None
    # ... and the two older recognisers are what they were
    assert _wordpiece_spec(bert) is not None and _bpe_spec(bpe_helpers.build_tokenizer("roberta")) is not None
    assert _unigram_structure(H.legacy_tokenizer(vocab)) is not None


class _Drifted:
    """A tokenizer whose serialised configuration reads like the recognised pipeline but which behaves differently: what
    another library version, or a Precompiled map that touches an ASCII character, may be.  `swap` exchanges two ids in the
    output; `char_map` replaces one character of every text before the wrapped tokenizer sees it."""

    def __init__(self, hf, swap=None, char_map=None):
        self._hf, self._swap, self._char_map = hf, swap, char_map

    def __getattr__(self, name):
        return getattr(self._hf, name)

    def __call__(self, texts, **kw):
        if self._char_map:
            texts = [t.replace(*self._char_map) for t in texts]
        out = self._hf(texts, **kw)
        if self._swap:
            ids = out["input_ids"]
            lo, hi = self._swap
            out["input_ids"] = np.where(ids == lo, hi, np.where(ids == hi, lo, ids))
        return out


def test_no_probe_is_compared_truncated():
    """The probe list names every printable ASCII character alone, inside a word, in front of a letter and behind one, and no
    probe comes near the guard's max_length on either side: nothing of it goes uncompared."""
    from adaptive_classifier.tokenizer import _PROBE_MAX_LENGTH, _unigram_probes
    plain, controls = _unigram_probes()
    words = {w for t in plain for w in t.split(" ")}
    for ch in H.PRINTABLE:
        assert {ch, "w" + ch + "w", ch + "a", "a" + ch} <= words, ch
    assert "" in plain and any(t and not t.strip(" ") for t in plain) and any("``" in t for t in plain) and any("''" in t for t in plain)
    assert all(any(c in t for t in controls) for c in "\t\n\r")
    for config in list(H.CONFIGS) + [("tie", None)]:
        hf = H.tie_tokenizer() if config[0] == "tie" else H.build_tokenizer(*config)
        hv = H.HostVocab(hf)
        probes = [t for t in plain + controls if not any(sp in t for sp in hv.spec["specials"])]
        assert len(probes) >= len(plain) + len(controls) - 2
        want = hf(probes, max_length=_PROBE_MAX_LENGTH, truncation=True, padding=True, return_tensors="np")["attention_mask"].sum(1)
        _, _, lens = H.encode_host(hv, probes, _PROBE_MAX_LENGTH)
        assert np.array_equal(lens, want) and int(lens.max()) <= _PROBE_MAX_LENGTH - 32, (config, int(lens.max()))


def test_the_probe_guard_fires():
    """Structure alone is never trusted: a pipeline that passes the structural check but behaves differently comes back
    None -- whichever printable ASCII character it treats differently; where only the \\t \\n \\r probes differ, the spec
    stays and ws_controls is off."""
    from tokenizers import Regex, normalizers
    from adaptive_classifier.tokenizer import _unigram_spec, _unigram_structure
    hf = H.build_tokenizer("full", "xlmr_legacy")
    assert _unigram_spec(hf) is not None
    dot = hf.convert_tokens_to_ids(".")
    drifted = _Drifted(hf, swap=(dot, dot + 1))
    assert _unigram_structure(drifted) is not None and _unigram_spec(drifted) is None
    structure = _unigram_structure(hf)
    for ch in H.PRINTABLE:                                 # as a Precompiled map that rewrites this one character would
        drifted = _Drifted(hf, char_map=(ch, "#" if ch != "#" else "$"))
        assert _unigram_spec(drifted, dict(structure)) is None, ch
    # Replace(" {2,}") alone leaves \t \n \r to the model (no Precompiled map in front): unknown bytes inside words there, word
    # separators here -- the plain probes match, the control probes do not
    vocab = H._xlmr_vocab(H.trained_pieces("full"))
    bare = H.legacy_tokenizer(vocab, normalizer=normalizers.Replace(Regex(" {2,}"), " "))
    spec = _unigram_spec(bare)
    assert spec is not None and spec["ws_controls"] is False and spec["trailing_space_piece"] is True


def test_argument_validation_without_gpu():
    from adaptive_classifier import _native as nv
    from adaptive_classifier.tokenizer import unigram_vocab_struct
    L = nv.lib()
    assert L.ac_version() >= 13
    hv = H.HostVocab(H.build_tokenizer("full", "xlmr"))
    blob, offs = H.pack(["ab", "c"])
    ids, mask, lens = np.zeros((2, 8), np.int64), np.zeros((2, 8), np.int64), np.zeros(2, np.int32)
    p = lambda a: a.ctypes.data                                                          # noqa: E731

    def both(text, offsets, b, vocab, M, i, m, n):
        v = ctypes.byref(vocab) if vocab is not None else None
        return (L.ac_unigram_encode(text, offsets, b, v, M, i, m, n, None), L.ac_unigram_encode_host(text, offsets, b, v, M, i, m, n))

    EINVAL = -1
    assert both(p(blob), p(offs), 2, None, 8, p(ids), p(mask), p(lens)) == (EINVAL, EINVAL)
    assert both(p(blob), None, 2, hv.struct, 8, p(ids), p(mask), p(lens)) == (EINVAL, EINVAL)
    assert both(p(blob), p(offs), 2, hv.struct, 8, None, p(mask), p(lens)) == (EINVAL, EINVAL)
    assert both(p(blob), p(offs), 2, hv.struct, 8, p(ids), None, p(lens)) == (EINVAL, EINVAL)
    assert both(p(blob), p(offs), 2, hv.struct, 8, p(ids), p(mask), None) == (EINVAL, EINVAL)
    assert both(p(blob), p(offs), 2, hv.struct, 1, p(ids), p(mask), p(lens)) == (EINVAL, EINVAL)      # max_length < 2
    assert both(None, p(offs), 2, hv.struct, 8, p(ids), p(mask), p(lens)) == (EINVAL, EINVAL)         # text NULL with b > 0
    assert b"unigram" in L.ac_last_error()
    ptrs = [a.ctypes.data for a in hv.arrays]
    odd = unigram_vocab_struct(hv.spec, ptrs, hv.slots - 1)                                           # not a power of two
    assert both(p(blob), p(offs), 2, odd, 8, p(ids), p(mask), p(lens)) == (EINVAL, EINVAL)
    assert b"unigram" in L.ac_last_error()
    for hole in range(4):
        holes = unigram_vocab_struct(hv.spec, [None if i == hole else q for i, q in enumerate(ptrs)], hv.slots)
        assert both(p(blob), p(offs), 2, holes, 8, p(ids), p(mask), p(lens)) == (EINVAL, EINVAL)
    assert both(None, p(offs), 0, hv.struct, 8, p(ids), p(mask), p(lens)) == (0, 0)                   # b == 0: nothing to do
    assert L.ac_unigram_encode_host(p(blob), p(offs), 2, ctypes.byref(hv.struct), 8, p(ids), p(mask), p(lens)) == 0
    assert lens.min() >= 2


def test_unigram_kernel_has_no_scratch():
    """The Viterbi state is three registers per lane, the walk goes through LDS: the device listing of unigram.hip must show
    no private segment and at most 128 VGPRs (read the way test_kernel_resources_cpu.py reads listings)."""
    from test_kernel_resources_cpu import HIPCC, kernel_resources
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    res = {k: v for k, v in kernel_resources("unigram.hip").items() if "unigram_kernel" in k}
    assert len(res) == 1, res
    (scratch, vgpr), = res.values()
    assert scratch == 0 and vgpr <= 128, (scratch, vgpr)      # 128 VGPRs: four waves per SIMD stay possible


SANITIZER_MAIN = r"""
// stand-alone: csrc/unigram_core.h over a dumped table and texts (unigram_helpers.dump), one line of ids per text
#include <cstdio>
#include <cstring>
#include <vector>
#include "unigram_core.h"
int main(int argc, char** argv) {
    FILE* f = argc > 1 ? fopen(argv[1], "rb") : nullptr;
    if (!f) return 2;
    int32_t hd[16];
    double unk_score;
    if (fread(hd, 4, 16, f) != 16 || fread(&unk_score, 8, 1, f) != 1) return 2;
    const int slots = hd[0], blob_len = hd[1], b = hd[2], text_len = hd[3], M = hd[4], max_piece = hd[5], unk = hd[6];
    const int lowercase = hd[10], trailing = hd[11], ws_controls = hd[12];
    // exact-size heap blocks: a read past any table or past a text's end is a report
    std::vector<uint64_t> keys(slots);
    std::vector<int32_t> entries(4 * (size_t)slots), offs(b + 1);
    std::vector<double> scores(slots);
    std::vector<uint8_t> blob(blob_len), text(text_len);
    bool ok = fread(keys.data(), 8, slots, f) == (size_t)slots && fread(entries.data(), 4, 4 * (size_t)slots, f) == 4 * (size_t)slots &&
              fread(scores.data(), 8, slots, f) == (size_t)slots && fread(blob.data(), 1, blob_len, f) == (size_t)blob_len &&
              fread(offs.data(), 4, b + 1, f) == (size_t)b + 1 && fread(text.data(), 1, text_len, f) == (size_t)text_len;
    fclose(f);
    if (!ok) return 2;
    const unigram::Table t{keys.data(), entries.data(), scores.data(), blob.data(), (uint32_t)(slots - 1)};
    for (int tx = 0; tx < b; ++tx) {
        const int n = offs[tx + 1] - offs[tx] + 1;
        std::vector<uint8_t> c(n);
        c[0] = 0x20;
        for (int i = 1; i < n; ++i) c[i] = unigram::norm_byte(text[offs[tx] + i - 1], lowercase, ws_controls);
        std::vector<int64_t> out(M - 2);
        std::vector<double> best(n + 1);
        std::vector<int32_t> w1(n + 1), w2(n + 1), w3(n + 1);
        const int k = unigram::encode_text(t, max_piece, unk_score, unk, trailing, c.data(), n, M - 2, out.data(), best.data(), w1.data(),
                                           w2.data(), w3.data());
        printf("%d", hd[7]);
        for (int i = 0; i < k; ++i) printf(" %lld", (long long)out[i]);
        printf(" %d\n", hd[8]);
    }
    return 0;
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
    """unigram_core.h as plain C++ in a stand-alone program built with -fsanitize=address,undefined: clean, and the same ids
    as the library.  The tables, every text and every work array sit in exact-size heap blocks, so a probe, a look-ahead or a
    Viterbi write past an end is reported."""
    hv = H.HostVocab(H.build_tokenizer(which, pipeline))
    texts = [t for t in H.FIXED + H.random_texts(400, 23) if H.eligible(t, hv.spec["specials"])]
    assert len(texts) > 300
    M = 24
    data = str(tmp_path / "unigram.bin")
    H.dump(hv, texts, M, data)
    src, exe = tmp_path / "unigram_main.cpp", str(tmp_path / "unigram_main")
    src.write_text(SANITIZER_MAIN)
    subprocess.run([_host_compiler(), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover",
                    "-I", CSRC, str(src), "-o", exe], check=True, capture_output=True, text=True)
    run = subprocess.run([exe, data], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    ids, _, lens = H.encode_host(hv, texts, M)
    want = [" ".join(str(x) for x in ids[i, :lens[i]]) for i in range(len(texts))]
    assert run.stdout.strip("\n").split("\n") == want
