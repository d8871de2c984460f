"""CPU side of WordPiece on UTF-8 text: csrc/wordpiece_core.h through ac_wordpiece_encode_utf8_host (the routines the kernel
runs, text by text on the host) over the probed normaliser / class tables (build_wordpiece_unicode_tables) against the
tokenizers library, in three normalizer configurations; malformed input and the buffer edge through the C entry; the tables
and their probe guard; argument validation and the ABI; the kernel's listing; the header under host sanitizers in a
stand-alone program.  No GPU needed, no tolerance anywhere: ids, mask and lengths are compared for equality.

The vocabulary is synthetic (wordpiece_helpers.vocab): nothing pretrained is available offline."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import wordpiece_helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "adaptive-classifier_amd", "csrc")
BUF = 8192                                                 # wpu::kBufBytes


@pytest.fixture(scope="module", params=H.CONFIGS)
def setup(request):
    hf = H.build_tokenizer(request.param)
    return request.param, hf, H.HostTables(hf), H.FIXED + H.random_texts(3000, 3)


def _assert_equal(ht, texts, got, want):
    ids, mask, lens = got
    wi, wm, wl = want
    bad = np.nonzero((ids != wi).any(1) | (mask != wm).any(1) | (lens != wl))[0]
    assert len(bad) == 0, [(texts[i][:40], [hex(ord(c)) for c in texts[i][:10]], ids[i, :12].tolist(), wi[i, :12].tolist(), int(lens[i]),
                            int(wl[i])) for i in bad[:3]]


@pytest.mark.parametrize("max_length", [512, 16, 2])
def test_host_entry_equals_the_wrapped_tokenizer(setup, max_length):
    kind, hf, ht, texts = setup
    eligible = [t for t in texts if ht.eligible(t)]
    assert len(eligible) >= 0.9 * len(texts) and len(texts) >= 3000
    for t in H.FIXED:                                      # none of the fixed cases is lost to routing without a named reason
        assert ht.eligible(t) or (t in H.HOST_ONLY_FIXED and H.HOST_ONLY_FIXED[t][0] == kind), (kind, t)
    want = H.reference(hf, eligible, max_length)
    if max_length == 512:                                  # not vacuous: well under half of the pieces are [UNK]
        pieces = (want[1] == 1).sum() - 2 * len(eligible)
        assert (want[0] == ht.struct.unk_id).sum() < 0.5 * pieces
    _assert_equal(ht, eligible, H.encode_host(ht, eligible, max_length), want)
    # the texts with a host-only code point come back as not done, their rows untouched
    rest = [t for t in texts if not ht.eligible(t)]
    if rest:
        ids, mask, lens = H.encode_host(ht, rest, max_length)
        assert (lens == -1).all() and (ids == -7).all() and (mask == -7).all()


def test_fixed_cases_tokenise_as_intended(setup):
    """The fixed cases do what their comments say, in the wrapped tokenizer (so that they test what they name) and in the
    host entry alike."""
    kind, hf, ht, _ = setup
    v = ht.vocab
    unk, cls, sep = v["[UNK]"], v["[CLS]"], v["[SEP]"]

    def enc(text, M=512):
        ids, mask, lens = H.encode_host(ht, [text], M)
        wi, wm, wl = H.reference(hf, [text], M)
        assert lens[0] == wl[0] and np.array_equal(ids, wi) and np.array_equal(mask, wm), text
        return ids[0, :lens[0]].tolist()

    # 100 characters of two bytes each are a word, 101 are [UNK]: the limit counts characters
    first, cont = (v["e"], v["##e"]) if kind == "uncased" else (v["é"], v["##é"])
    assert enc("é" * 100) == [cls, first] + [cont] * 99 + [sep]
    assert enc("é" * 101) == [cls, unk, sep]
    # a run of CJK characters: every character its own word; U+20000 padded with spaces as well
    assert len(enc("".join(chr(0x4E00 + i) for i in range(200)))) == 202
    assert len(enc("x\U00020000\U00020001y")) == 6
    # removed characters only, and the empty text
    assert enc("\u200d\u00ad\ufffd\x00") == [cls, sep] and enc("") == [cls, sep]
    assert enc("a\u200db\u00adc\ufffdd\x00e") == enc("abcde")
    # Unicode spaces separate words; punctuation stands alone
    assert len(enc("a\u3000b\u00a0c")) == 5
    assert len(enc("“a” — b… 、c。")) == 2 + 9
    # a Hangul syllable is three jamo under accent stripping, itself otherwise; U+1D163 has a 12-byte image under NFD
    norm = hf.backend_tokenizer.normalizer.normalize_str
    assert len(norm("한")) == (3 if kind == "uncased" else 1)
    assert len(norm("\U0001d163").encode()) == (12 if kind == "uncased" else 4)
    assert H.table_image(ht.tables, 0x1D163) == norm("\U0001d163")
    # case mappings: two code points for U+0130 without accent stripping; no compatibility decomposition of the fi ligature
    if kind != "cased":
        assert norm("İ") == ("i" if kind == "uncased" else "i\u0307") and norm("ß ſ ǅ Σ ς \u212a") == "ß ſ ǆ σ ς k"
    assert norm("ﬁ") == "ﬁ"
    for t in ("İ", "ß ſ ǅ Σ ς \u212a", "ﬁ", "한", "\U0001d163", "\U00020000", "ok \U0001f600 fine \U0001f1e9\U0001f1ea"):
        enc(t)
    # marks in both orders give the same pieces where accents are stripped
    if kind == "uncased":
        assert enc("a\u0323\u0301") == enc("a\u0301\u0323") == enc("a")
    # truncation inside a multi-piece word
    long_word = "e" * 40 + "é" * 30 + " tail"
    assert len(enc(long_word)) > 16 and len(enc(long_word, 16)) == 16 and enc(long_word, 2) == [cls, sep]


def test_ascii_parity():
    """On the ASCII text set of test_tokenizer_gpu.py the UTF-8 host entry gives the wrapped tokenizer's ids."""
    from transformers import BertTokenizer
    for lower, drop, M in [(True, (), 512), (True, ("z", "##q", "7", "'"), 64), (False, (), 24), (True, (), 8)]:
        vocab = H.ascii_vocab(drop)
        hf = BertTokenizer(vocab=vocab, do_lower_case=lower)
        ht = H.HostTables(hf)
        texts = [t for t in H.ascii_texts() if t.isascii() and ht.eligible(t)]
        assert len(texts) >= 75
        _assert_equal(ht, texts, H.encode_host(ht, texts, M), H.reference(hf, texts, M))


@pytest.mark.parametrize("slack", [64, 0])
def test_malformed_utf8_through_the_c_entry(setup, slack):
    """Each malformed form as the last bytes of a text (a good text behind it) and as the last bytes of the whole blob: -1 for
    that row, its cells untouched, correct rows on both sides."""
    kind, hf, ht, _ = setup
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
    # more than 4096 bytes: not done
    ids, mask, lens = H.encode_host(ht, ["a " * 2048, "a " * 2048 + "b"], 8, slack)
    assert lens.tolist() == [8, -1]


def test_buffer_edge():
    """Texts whose normalised UTF-8 is one byte short of the buffer, fills it exactly, and exceeds it by one: only the last is
    not done.  Only accent stripping can grow a text of <= 4096 bytes past the buffer (a Hangul syllable: 3 bytes -> 9); the
    largest growth without it is CJK spacing, 3 -> 5 bytes, 6827 bytes at most."""
    hf = H.build_tokenizer("uncased")
    ht = H.HostTables(hf)
    norm = hf.backend_tokenizer.normalizer.normalize_str
    texts = ["한 " * 819 + "a" * r for r in (1, 2, 3)]
    assert [len(norm(t).encode()) for t in texts] == [BUF - 1, BUF, BUF + 1] and all(len(t.encode()) <= 4096 for t in texts)
    ids, mask, lens = H.encode_host(ht, texts, 512)
    assert lens[2] == -1 and (ids[2] == -7).all()
    _assert_equal(ht, texts[:2], (ids[:2], mask[:2], lens[:2]), H.reference(hf, texts[:2], 512))
    for kind in ("cased", "uncased_keep_accents"):
        other = H.HostTables(H.build_tokenizer(kind))
        full = ["中" * 1365, "한" * 1365]
        _assert_equal(other, full, H.encode_host(other, full, 512), H.reference(other.hf, full, 512))


def test_tables(setup):
    kind, hf, ht, _ = setup
    from adaptive_classifier import tokenizer as tkz
    t = ht.tables
    norm = hf.backend_tokenizer.normalizer.normalize_str
    # images round-trip for every code point of the pools
    flagged = set(t["host_only"])
    for cp in H.pool_code_points():
        img = H.table_image(t, cp)
        assert (img is None and cp in flagged) or img == norm(chr(cp)), hex(cp)
    assert (kind == "uncased") == bool(flagged) == t["strips_accents"]
    assert 0x1D165 in flagged or kind != "uncased"
    # the page deduplication bound of DESIGN 2.4v: at most 256 of the 4352 pages are distinct, the images fit 128 KiB
    assert t["page_of"].shape == (0x1100,) and t["page_of"].dtype == np.uint16 and int(t["page_of"].max()) == t["n_pages"] - 1
    assert t["entries"].shape == (t["n_pages"], 256) and t["entries"].dtype == np.uint32
    assert t["n_pages"] <= 256 and t["image_bytes"] <= 128 * 1024 and len(t["images"]) >= t["image_bytes"]
    # cached in-process by the serialised normalizer + pre-tokenizer
    assert tkz.build_wordpiece_unicode_tables(H.build_tokenizer(kind)) is t
    # the probe guard passes on the real tables ...
    assert tkz.wordpiece_unicode_tables(hf, ht.specials, ht.struct) is t
    # ... and a tampered table (one image changed) trips it: the tokenizer keeps its ASCII-only routing
    bad = dict(t, entries=t["entries"].copy(), images=t["images"].copy())
    e = int(bad["entries"][int(bad["page_of"][0]), ord("\t")])
    assert e & 7 == 2                                      # the tab's image is a space in every configuration
    bad["images"][e >> 9] = ord("x")
    assert tkz._wordpiece_unicode_matches(hf, ht.specials, ht.struct, t, tkz._wordpiece_unicode_probes())
    assert not tkz._wordpiece_unicode_matches(hf, ht.specials, ht.struct, bad, tkz._wordpiece_unicode_probes())
    key = [k for k, v in tkz._WP_UNICODE_CACHE.items() if v is t]
    assert len(key) == 1
    tkz._WP_UNICODE_CACHE[key[0]] = bad
    try:
        assert tkz.wordpiece_unicode_tables(hf, ht.specials, ht.struct) is None
    finally:
        tkz._WP_UNICODE_CACHE[key[0]] = t


def test_wordpiece_spec_is_unchanged():
    from adaptive_classifier.tokenizer import _wordpiece_spec
    hf = H.build_tokenizer("uncased")
    spec = _wordpiece_spec(hf)
    assert isinstance(spec, tuple) and len(spec) == 3 and spec[0] == H.vocab() and spec[1] is True and set(spec[2]) == set(H.SPECIALS)
    assert _wordpiece_spec(H.build_tokenizer("cased"))[1] is False


def test_argument_validation_without_gpu():
    from adaptive_classifier import _native as nv
    from adaptive_classifier import tokenizer as tkz
    L = nv.lib()
    ht = H.HostTables(H.build_tokenizer("cased"))
    blob, offs = H.pack([b"ab", b"c"])
    ids, mask, lens = np.zeros((2, 8), np.int64), np.zeros((2, 8), np.int64), np.zeros(2, np.int32)
    p = lambda a: a.ctypes.data                                                          # noqa: E731

    def both(text, offsets, b, vocab, uni, M, i, m, n):
        v = ctypes.byref(vocab) if vocab is not None else None
        u = ctypes.byref(uni) if uni is not None else None
        return (L.ac_wordpiece_encode_utf8(text, offsets, b, v, u, M, i, m, n, None),
                L.ac_wordpiece_encode_utf8_host(text, offsets, b, v, u, M, i, m, n))

    EINVAL = -1
    V, U = ht.struct, ht.unicode
    assert both(p(blob), p(offs), 2, None, U, 8, p(ids), p(mask), p(lens)) == (EINVAL, EINVAL)
    assert both(p(blob), p(offs), 2, V, None, 8, p(ids), p(mask), p(lens)) == (EINVAL, EINVAL)       # NULL table
    assert both(p(blob), None, 2, V, U, 8, p(ids), p(mask), p(lens)) == (EINVAL, EINVAL)
    assert both(p(blob), p(offs), 2, V, U, 8, None, p(mask), p(lens)) == (EINVAL, EINVAL)
    assert both(p(blob), p(offs), 2, V, U, 8, p(ids), None, p(lens)) == (EINVAL, EINVAL)
    assert both(p(blob), p(offs), 2, V, U, 8, p(ids), p(mask), None) == (EINVAL, EINVAL)
    assert both(p(blob), p(offs), 2, V, U, 1, p(ids), p(mask), p(lens)) == (EINVAL, EINVAL)          # max_length < 2
    assert both(None, p(offs), 2, V, U, 8, p(ids), p(mask), p(lens)) == (EINVAL, EINVAL)             # text NULL with b > 0
    assert b"wordpiece utf8" in L.ac_last_error()
    odd = tkz.wordpiece_vocab_struct(ht.hf, ht.vocab, ht.lower, [a.ctypes.data for a in ht.arrays], ht.slots - 1, ht.max_piece)
    assert both(p(blob), p(offs), 2, odd, U, 8, p(ids), p(mask), p(lens)) == (EINVAL, EINVAL)        # not a power of two
    ptrs = [a.ctypes.data for a in ht.arrays]
    holes = tkz.wordpiece_vocab_struct(ht.hf, ht.vocab, ht.lower, [ptrs[0], None] + ptrs[2:], ht.slots, ht.max_piece)
    assert both(p(blob), p(offs), 2, holes, U, 8, p(ids), p(mask), p(lens)) == (EINVAL, EINVAL)
    t = ht.tables
    for broken in (nv.ac_wordpiece_unicode(None, p(t["entries"]), p(t["images"]), t["n_pages"], t["image_bytes"]),
                   nv.ac_wordpiece_unicode(p(t["page_of"]), None, p(t["images"]), t["n_pages"], t["image_bytes"]),
                   nv.ac_wordpiece_unicode(p(t["page_of"]), p(t["entries"]), None, t["n_pages"], t["image_bytes"]),
                   nv.ac_wordpiece_unicode(p(t["page_of"]), p(t["entries"]), p(t["images"]), 0, t["image_bytes"])):
        assert both(p(blob), p(offs), 2, V, broken, 8, p(ids), p(mask), p(lens)) == (EINVAL, EINVAL)
    assert both(None, p(offs), 0, V, U, 8, p(ids), p(mask), p(lens)) == (0, 0)                       # b == 0: nothing to do


def test_abi():
    """The new symbols are in the header, the library and the ctypes table; ac_version() is 14; the existing entry is still there."""
    from adaptive_classifier import _native as nv
    L = nv.lib()
    assert L.ac_version() >= 14
    header = open(os.path.join(ROOT, "include", "acamd.h")).read()
    for name in ("ac_wordpiece_encode_utf8", "ac_wordpiece_encode_utf8_host", "ac_wordpiece_encode", "ac_wordpiece_hash"):
        assert re.search(r"\b%s\s*\(" % name, header) and hasattr(L, name) and name in nv.exported_symbols(), name
    assert "typedef struct ac_wordpiece_unicode {" in header
    fields = re.search(r"typedef struct ac_wordpiece_unicode \{(.*?)\} ac_wordpiece_unicode;", header, re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    assert re.findall(r"(\w+)\s*[;,]", fields) == [f for f, _ in nv.ac_wordpiece_unicode._fields_]
    assert ctypes.sizeof(nv.ac_wordpiece_unicode) == 3 * ctypes.sizeof(ctypes.c_void_p) + 8


def test_utf8_kernel_has_no_scratch():
    """No private segment, at most 128 VGPRs (the bound the BPE and Unigram kernels are held to); the ASCII kernel is still there."""
    from test_kernel_resources_cpu import HIPCC, kernel_resources
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    res = kernel_resources("wordpiece.hip")
    new = {k: v for k, v in res.items() if "wordpiece_utf8_kernel" in k}
    old = {k: v for k, v in res.items() if "wordpiece_kernel" in k}
    assert len(new) == 1 and len(old) == 1, res
    (scratch, vgpr), = new.values()
    assert scratch == 0 and vgpr <= 128, (scratch, vgpr)
    assert list(old.values())[0][0] == 0


SANITIZER_MAIN = r"""
// stand-alone: csrc/wordpiece_core.h over dumped tables and texts (wordpiece_helpers.dump), one line per text: its ids, or -1
#include <cstdio>
#include <cstring>
#include <vector>
#include "wordpiece_core.h"
template <class T> static bool rd(FILE* f, std::vector<T>& v) { return v.empty() || fread(v.data(), sizeof(T), v.size(), f) == v.size(); }
int main(int argc, char** argv) {
    FILE* f = argc > 1 ? fopen(argv[1], "rb") : nullptr;
    if (!f) return 2;
    int32_t hd[12];
    if (fread(hd, 4, 12, f) != 12) return 2;
    const int slots = hd[0], blob_len = hd[1], n_pages = hd[7], image_bytes = hd[8], b = hd[9], text_len = hd[10], M = hd[11];
    // exact-size heap blocks: a read past any table, past a text's end or past the normalisation buffer is a report
    std::vector<uint64_t> keys(slots);
    std::vector<uint32_t> offs(slots), entries(256 * (size_t)n_pages);
    std::vector<int32_t> ids(slots), toffs(b + 1);
    std::vector<uint16_t> lens(slots), page_of(wpu::kPages);
    std::vector<uint8_t> blob(blob_len), images(image_bytes), text(text_len);
    const bool ok = rd(f, keys) && rd(f, offs) && rd(f, ids) && rd(f, lens) && rd(f, blob) && rd(f, page_of) && rd(f, entries) &&
                    rd(f, images) && rd(f, toffs) && rd(f, text);
    fclose(f);
    if (!ok) return 2;
    const wpu::Vocab v{keys.data(), offs.data(), ids.data(), lens.data(), blob.data(), (uint32_t)(slots - 1), hd[2], hd[3], hd[4], hd[5], hd[6]};
    const wpu::Unicode u{page_of.data(), entries.data(), images.data(), n_pages, image_bytes};
    for (int tx = 0; tx < b; ++tx) {
        const int n = toffs[tx + 1] - toffs[tx];
        std::vector<uint8_t> one(text.begin() + toffs[tx], text.begin() + toffs[tx + 1]);      // the text alone in its own block
        std::vector<uint8_t> buf(wpu::kBufBytes);
        std::vector<int64_t> out(M - 2);
        const int k = wpu::encode_text(u, v, one.data(), n, buf.data(), wpu::kBufBytes, M - 2, out.data());
        if (k < 0) { printf("-1\n"); continue; }
        printf("%d", hd[4]);
        for (int i = 0; i < k; ++i) printf(" %lld", (long long)out[i]);
        printf(" %d\n", hd[5]);
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
def test_core_header_under_host_sanitizers(tmp_path):
    """wordpiece_core.h as plain C++ in a stand-alone program built with -fsanitize=address,undefined: clean, and the same
    ids / not-done rows as the library.  The tables, every text and the normalisation buffer sit in exact-size heap blocks; the
    malformed and the buffer-edge texts are in."""
    hf = H.build_tokenizer("uncased")
    ht = H.HostTables(hf)
    texts = [t for t in H.FIXED + H.random_texts(400, 23) if len(t.encode()) <= 4096]
    raws = H.raw(texts) + [p + bad for bad in H.MALFORMED for p in (b"", b"ab ")] + H.raw(["한 " * 819 + "a" * r for r in (1, 2, 3)])
    M = 24
    data = str(tmp_path / "wp.bin")
    H.dump(ht, raws, M, data)
    src, exe = tmp_path / "wp_main.cpp", str(tmp_path / "wp_main")
    src.write_text(SANITIZER_MAIN)
    subprocess.run([_host_compiler(), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover",
                    "-I", CSRC, str(src), "-o", exe], check=True, capture_output=True, text=True)
    run = subprocess.run([exe, data], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    ids, _, lens = H.encode_host(ht, raws, M)
    want = ["-1" if lens[i] < 0 else " ".join(str(x) for x in ids[i, :lens[i]]) for i in range(len(raws))]
    assert lens[-1] == -1 and lens[-2] > 0 and sum(1 for w in want if w == "-1") >= 2 * len(H.MALFORMED) + 1
    assert run.stdout.strip("\n").split("\n") == want
