"""CPU side of byte-level BPE on UTF-8 text: csrc/bpe_core.h through ac_bpe_utf8_encode_host (the routines bpe_utf8_kernel runs,
text by text on the host) over the probed class table (build_bpe_unicode_tables) against the tokenizers library -- ids and mask bit
for bit, no tolerance --, the table itself, malformed UTF-8, the ABI and argument validation, the kernel's listing, and the same
header under host sanitizers in a stand-alone program.  No GPU needed.

The vocabularies are trained in-process (bpe_unicode_helpers): nothing pretrained is available offline."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import bpe_helpers as B
import bpe_unicode_helpers as H
from test_bpe_tokenizer_cpu import _host_compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "adaptive-classifier_amd", "csrc")
EINVAL = -1


@pytest.fixture(scope="module", params=H.CONFIGS)
def setup(request):
    hf = H.build_tokenizer(request.param)
    ht = H.HostTables(hf)
    return request.param, hf, ht


def _cls(c):
    """bpe::cls restated (test_core_header_under_host_sanitizers holds it against the header's own)"""
    if c == 0x20 or 0x09 <= c <= 0x0d:
        return 0
    if chr(c).isascii() and chr(c).isalpha():
        return 1
    if 0x30 <= c <= 0x39:
        return 2
    return 3


def _entry(t, cp):
    return int(t["entries"][t["page_of"][cp >> 8], cp & 0xff])


# ---- ABI ---------------------------------------------------------------------------------------------------------------------
def test_abi_names_version_and_struct():
    """The new symbols are in the header, the library and the ctypes table; ac_version() is 17; the wrapper takes `unicode=`;
    the ASCII entries are still there."""
    from adaptive_classifier import _native as nv
    from adaptive_classifier.tokenizer import HipByteBPETokenizer, maybe_device_tokenizer
    L = nv.lib()
    assert L.ac_version() >= 17
    header = open(os.path.join(ROOT, "include", "acamd.h")).read()
    for name in ("ac_bpe_utf8_encode", "ac_bpe_utf8_encode_host", "ac_bpe_encode", "ac_bpe_encode_host"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in nv.exported_symbols() and name in nv._SIGNATURES and hasattr(L, name), name
    fields = re.search(r"typedef struct ac_bpe_unicode \{(.*?)\} ac_bpe_unicode;", header, re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    assert re.findall(r"(\w+)\s*[;,]", fields) == [f for f, _ in nv.ac_bpe_unicode._fields_]
    assert ctypes.sizeof(nv.ac_bpe_unicode) == 2 * ctypes.sizeof(ctypes.c_void_p) + 8
    assert len(nv._SIGNATURES["ac_bpe_utf8_encode"][1]) == 10 and len(nv._SIGNATURES["ac_bpe_utf8_encode_host"][1]) == 9
    assert inspect.signature(HipByteBPETokenizer.__init__).parameters["unicode"].default is False
    assert inspect.signature(maybe_device_tokenizer).parameters["unicode"].default is False


def test_argument_validation_without_gpu():
    from adaptive_classifier import _native as nv
    from adaptive_classifier.tokenizer import bpe_vocab_struct
    L = nv.lib()
    ht = H.HostTables(H.build_tokenizer("roberta"))
    hv, t = ht.hv, ht.tables
    blob, offs = H.pack([b"ab", "é".encode()])
    ids, mask, lens = np.zeros((2, 8), np.int64), np.zeros((2, 8), np.int64), np.zeros(2, np.int32)
    p = lambda a: a.ctypes.data                                                          # noqa: E731

    def both(text, offsets, b, vocab, uni, M, i, m, n):
        v = ctypes.byref(vocab) if vocab is not None else None
        u = ctypes.byref(uni) if uni is not None else None
        return (L.ac_bpe_utf8_encode(text, offsets, b, v, u, M, i, m, n, None), L.ac_bpe_utf8_encode_host(text, offsets, b, v, u, M, i, m, n))

    ok = (ht.vocab, ht.unicode)
    assert both(p(blob), p(offs), 2, None, ht.unicode, 8, p(ids), p(mask), p(lens)) == (EINVAL, EINVAL)
    assert both(p(blob), p(offs), 2, ht.vocab, None, 8, p(ids), p(mask), p(lens)) == (EINVAL, EINVAL)
    assert both(p(blob), None, 2, *ok, 8, p(ids), p(mask), p(lens)) == (EINVAL, EINVAL)
    assert both(p(blob), p(offs), 2, *ok, 8, None, p(mask), p(lens)) == (EINVAL, EINVAL)
    assert both(p(blob), p(offs), 2, *ok, 8, p(ids), None, p(lens)) == (EINVAL, EINVAL)
    assert both(p(blob), p(offs), 2, *ok, 8, p(ids), p(mask), None) == (EINVAL, EINVAL)
    assert both(p(blob), p(offs), 2, *ok, 1, p(ids), p(mask), p(lens)) == (EINVAL, EINVAL)            # max_length < 2
    assert both(p(blob), p(offs), -1, *ok, 8, p(ids), p(mask), p(lens)) == (EINVAL, EINVAL)
    assert both(None, p(offs), 2, *ok, 8, p(ids), p(mask), p(lens)) == (EINVAL, EINVAL)               # text NULL with b > 0
    assert b"bpe utf8" in L.ac_last_error()
    odd = bpe_vocab_struct(hv.spec, [a.ctypes.data for a in hv.arrays], hv.slots - 1)              # not a power of two
    assert both(p(blob), p(offs), 2, odd, ht.unicode, 8, p(ids), p(mask), p(lens)) == (EINVAL, EINVAL)
    holes = bpe_vocab_struct(hv.spec, [hv.arrays[0].ctypes.data, None, hv.arrays[2].ctypes.data, hv.arrays[3].ctypes.data], hv.slots)
    assert both(p(blob), p(offs), 2, holes, ht.unicode, 8, p(ids), p(mask), p(lens)) == (EINVAL, EINVAL)
    for broken in (nv.ac_bpe_unicode(None, p(t["entries"]), t["n_pages"]), nv.ac_bpe_unicode(p(t["page_of"]), None, t["n_pages"]),
                   nv.ac_bpe_unicode(p(t["page_of"]), p(t["entries"]), 0), nv.ac_bpe_unicode(p(t["page_of"]), p(t["entries"]), 65536)):
        assert both(p(blob), p(offs), 2, ht.vocab, broken, 8, p(ids), p(mask), p(lens)) == (EINVAL, EINVAL)
    assert both(None, p(offs), 0, *ok, 8, p(ids), p(mask), p(lens)) == (0, 0)                         # b == 0: nothing to do
    assert L.ac_bpe_utf8_encode_host(p(blob), p(offs), 2, ctypes.byref(ht.vocab), ctypes.byref(ht.unicode), 8, p(ids), p(mask), p(lens)) == 0
    assert lens.min() >= 3


# ---- the table ---------------------------------------------------------------------------------------------------------------
def test_table_classes_whitespace_and_host_only(setup):
    kind, hf, ht = setup
    t = ht.tables
    assert t["page_of"].shape == (0x1100,) and t["page_of"].dtype == np.uint16 and t["entries"].dtype == np.uint8
    assert t["entries"].shape == (t["n_pages"], 256) and int(t["page_of"].max()) < t["n_pages"]
    assert [_entry(t, c) & 3 for c in range(128)] == [_cls(c) for c in range(128)]                    # the ASCII rows are bpe::cls
    # whitespace: exactly what the pre-tokenizer shows (a whitespace character joins none of a letter, a digit, a punctuation mark)
    pre = hf.backend_tokenizer.pre_tokenizer.pre_tokenize_str
    ws = [cp for cp in t["whitespace"]]
    assert ws == sorted(cp for cp in range(0x110000) if not 0xD800 <= cp < 0xE000 and (_entry(t, cp) & 3) == 0)
    for cp in ws:
        assert all(len(pre(c + chr(cp))) == 2 for c in "a1!"), hex(cp)
    assert {0x85, 0xa0, 0x1680, 0x2028, 0x2029, 0x202f, 0x205f, 0x3000} | set(range(0x2000, 0x200b)) <= set(ws)
    assert 0x200b not in ws and 0x1c not in ws and 0x1f not in ws
    # spot classes, each asked of the pre-tokenizer alone as well
    rng = np.random.default_rng(3)
    for cp in [0xe9, 0xdf, 0x416, 0x4e2d, 0xd55c, 0x661, 0xb2, 0x2167, 0x20ac, 0x2026, 0x2019, 0x201c, 0x1f600, 0x301, 0x200b, 0x10ffff] + \
            rng.integers(0x80, 0x30000, 300).tolist():
        if 0xD800 <= cp < 0xE000:
            continue
        joins = [len(pre(c + chr(cp))) == 1 for c in "a1!"]
        assert (_entry(t, cp) & 3) == (1 if joins[0] else 2 if joins[1] else 3 if joins[2] else 0), hex(cp)
    for cp in (0xe9, 0x4e2d, 0x1f600, 0x2019):
        assert not _entry(t, cp) & 4, hex(cp)
    assert all(_entry(t, cp) & 4 for cp in (0xD800, 0xDFFF))                                            # surrogates
    if kind == "modernbert":                                                                            # NFC
        for cp in (0x301, 0x212b, 0x1161, 0x345):
            assert _entry(t, cp) & 4 and cp in t["host_only"], hex(cp)
        assert t["reasons"]["image"] > 1000 and t["reasons"]["composes"] > 0 and t["reasons"]["non-starter"] > 0
        norm = hf.backend_tokenizer.normalizer.normalize_str
        flagged = set(t["host_only"])
        assert all(norm(chr(cp)) == chr(cp) or cp in flagged for cp in list(range(0x3000)) + rng.integers(0, 0x30000, 2000).tolist()
                   if not 0xD800 <= cp < 0xE000)
    else:
        assert t["host_only"] == [] and t["reasons"] == {} and ht.flagged is None
    assert t["seconds"] > 0


def test_tables_are_cached_by_normalizer_and_pre_tokenizer():
    from adaptive_classifier import tokenizer as tkz
    a = tkz.build_bpe_unicode_tables(H.build_tokenizer("roberta"))
    assert tkz.build_bpe_unicode_tables(B.build_tokenizer("roberta")) is a        # another vocabulary, the same pipeline
    assert tkz.build_bpe_unicode_tables(H.build_tokenizer("modernbert")) is not a
    assert tkz.build_bpe_unicode_tables(H.build_tokenizer("modernbert")) is tkz.build_bpe_unicode_tables(B.build_tokenizer("modernbert"))


def test_probe_guard_accepts_the_tables_and_rejects_a_wrong_one(setup):
    from adaptive_classifier import tokenizer as tkz
    kind, hf, ht = setup
    probes = tkz._bpe_unicode_probes()
    assert tkz.bpe_unicode_tables(hf, ht.spec, ht.vocab) is ht.tables
    # é, e and the space as other: each cuts a pre-token whose bytes the merges of every trained vocabulary here join.  (A wrong
    # class shows in the ids only where a merge crosses the wrong boundary: the guard is a check of the model, not of each entry.)
    for cp, wrong in ((0xe9, 3), (0x65, 3), (0x20, 3)):
        bad = dict(ht.tables)
        bad["entries"] = ht.tables["entries"].copy()
        bad["entries"][bad["page_of"][cp >> 8], cp & 0xff] = wrong
        assert not tkz._bpe_unicode_matches(hf, ht.spec, ht.vocab, bad, probes), hex(cp)


# ---- the host entry against the wrapped tokenizer --------------------------------------------------------------------------------
def test_training_left_merges_inside_and_across_characters(setup):
    _, hf, _ = setup
    inside, across = H.multibyte_merges(hf)
    assert inside >= 20 and across >= 20, (inside, across)


@pytest.mark.parametrize("max_length", [512, 24, 8, 2])
def test_host_encode_equals_tokenizers(setup, max_length):
    """ids, mask and lengths identical to the wrapped tokenizer called as the classifier calls it, on every text of the set that
    is routed to the device; the texts with a host-only code point come back as -1, their rows unwritten."""
    kind, hf, ht = setup
    every = H.text_set(kind, 2000)
    texts = ht.device_route(every)
    held = [t for t in every if ht.flagged is not None and ht.flagged.search(t)]
    assert len(texts) > (700 if kind == "modernbert" else 1900)
    for t in H.FIXED:                                      # none of the fixed cases is lost to routing without a reason
        assert t in texts or (kind == "modernbert" and "  " in t), t
    assert (len(held) >= len(H.NFC_SENSITIVE)) == (kind == "modernbert") and all(t in held for t in H.NFC_SENSITIVE if kind == "modernbert")
    want = hf(texts, max_length=max_length, truncation=True, padding=True, return_tensors="np")
    ids, mask, lens = H.encode_host(ht, texts, max_length)
    S = want["input_ids"].shape[1]
    bad = np.nonzero((ids[:, :S] != want["input_ids"]).any(1) | (mask[:, :S] != want["attention_mask"]).any(1))[0]
    assert len(bad) == 0, [(texts[i][:60], ids[i, :S].tolist()[:16], want["input_ids"][i].tolist()[:16]) for i in bad[:3]]
    assert (ids[:, S:] == ht.spec["pad_id"]).all() and (mask[:, S:] == 0).all()
    assert np.array_equal(lens, want["attention_mask"].sum(1)) and int(lens.max()) == S
    if held:
        ids, mask, lens = H.encode_host(ht, held, max_length)
        assert (lens == -1).all() and (ids == -7).all() and (mask == -7).all()


def test_ascii_texts_equal_the_ascii_host_entry(setup):
    kind, hf, ht = setup
    texts = [t for t in B.text_set(kind, 600) if t.isascii() and len(t) <= 4096]
    for M in (64, 8):
        a = B.encode_host(ht.hv, texts, M)
        u = H.encode_host(ht, texts, M)
        assert all(np.array_equal(x, y) for x, y in zip(a, u))


def test_long_pretokens_are_done_on_the_host_entry(setup):
    """any pre-token length: a 30-character CJK run (90 bytes), 300 accented letters, a 4096-byte text ending in a 3-byte character"""
    kind, hf, ht = setup
    texts = ["中文产品很好" * 5, "é" * 300 + " x", "q" * 4093 + "中", "é" * 2048]
    want = hf(texts, max_length=512, truncation=True, padding=True, return_tensors="np")
    ids, mask, lens = H.encode_host(ht, texts, 512)
    S = want["input_ids"].shape[1]
    assert np.array_equal(ids[:, :S], want["input_ids"]) and np.array_equal(mask[:, :S], want["attention_mask"])
    ids, mask, lens = H.encode_host(ht, ["q" * 4094 + "中", "ok"], 16)                             # 4097 bytes: not done
    assert lens[0] == -1 and (ids[0] == -7).all() and lens[1] > 0


MALFORMED = {"overlong 2": b"a\xc0\xafb", "overlong 3": b"\xe0\x80\xaf", "overlong 4": b"\xf0\x80\x80\xaf", "c1 lead": b"\xc1\xbf",
             "surrogate": b"x\xed\xa0\x80", "low surrogate": b"\xed\xbf\xbf", "above U+10FFFF": b"\xf4\x90\x80\x80", "f5 lead": b"\xf5\x80\x80\x80",
             "stray 0x80": b"a\x80b", "stray at start": b"\x80", "stray after a character": b"\xc3\xa9\xa9",
             "cut in 2": b"caf\xc3", "cut in 3": b"x\xe4\xb8", "cut in 4": b"x \xf0\x9f\x98", "lead then ascii": b"\xe4\xb8a",
             "0xff": b"a\xffb"}


def test_malformed_utf8_is_not_done(setup):
    """never guessed: lens -1, the row unwritten, the neighbours unaffected"""
    kind, hf, ht = setup
    good = ["café", "中 x", "\U0001f600"]
    raws = []
    for m in MALFORMED.values():
        raws += [good[len(raws) % 3].encode(), m]
    raws.append(good[0].encode())
    ids, mask, lens = H.encode_host(ht, raws, 16)
    want = hf(good, max_length=16, truncation=True, padding="max_length", return_tensors="np")
    for i, r in enumerate(raws):
        if i % 2:
            assert lens[i] == -1 and (ids[i] == -7).all() and (mask[i] == -7).all(), list(MALFORMED)[i // 2]
        else:
            g = good.index(r.decode())
            assert np.array_equal(ids[i], want["input_ids"][g]) and np.array_equal(mask[i], want["attention_mask"][g]), r


# ---- the kernel's listing ----------------------------------------------------------------------------------------------------------
def test_bpe_utf8_kernel_has_no_scratch_and_at_most_128_vgprs():
    from test_kernel_resources_cpu import HIPCC, kernel_resources
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    res = {k: v for k, v in kernel_resources("bpe_utf8.hip").items() if "bpe_utf8_kernel" in k}
    assert len(res) == 1, res
    (scratch, vgpr), = res.values()
    print("bpe_utf8_kernel: scratch", scratch, "VGPRs", vgpr)
    assert scratch == 0 and vgpr <= 128, (scratch, vgpr)


# ---- the core header under host sanitizers -------------------------------------------------------------------------------------------
SANITIZER_MAIN = r"""
// stand-alone: csrc/bpe_core.h over dumped tables and texts (bpe_unicode_helpers.dump).  First line: bpe::cls of the bytes 0 .. 127;
// then one line per text: its ids, or -1
#include <cstdio>
#include <cstring>
#include <vector>
#include "bpe_core.h"
int main(int argc, char** argv) {
    FILE* f = argc > 1 ? fopen(argv[1], "rb") : nullptr;
    if (!f) return 2;
    int32_t hd[12];
    if (fread(hd, 4, 12, f) != 12) return 2;
    const int slots = hd[0], blob_len = hd[1], b = hd[2], text_len = hd[3], M = hd[4], prefix = hd[8], n_pages = hd[9];
    // exact-size heap blocks: a read past any table or past a text's end is a report
    std::vector<uint64_t> keys(slots);
    std::vector<int32_t> entries(4 * (size_t)slots), byte_id(256), offs(b + 1);
    std::vector<uint16_t> page_of(0x1100);
    std::vector<uint8_t> blob(blob_len), uent(256 * (size_t)n_pages), text(text_len);
    bool ok = fread(keys.data(), 8, slots, f) == (size_t)slots && fread(entries.data(), 4, 4 * (size_t)slots, f) == 4 * (size_t)slots &&
              fread(blob.data(), 1, blob_len, f) == (size_t)blob_len && fread(byte_id.data(), 4, 256, f) == 256 &&
              fread(page_of.data(), 2, 0x1100, f) == 0x1100 && fread(uent.data(), 1, uent.size(), f) == uent.size() &&
              fread(offs.data(), 4, b + 1, f) == (size_t)b + 1 && fread(text.data(), 1, text_len, f) == (size_t)text_len;
    fclose(f);
    if (!ok) return 2;
    for (int c = 0; c < 128; ++c) printf("%d", bpe::cls((uint8_t)c));
    printf("\n");
    const bpe::Table t{keys.data(), entries.data(), blob.data(), byte_id.data(), (uint32_t)(slots - 1)};
    const bpe::Unicode u{page_of.data(), uent.data(), n_pages};
    for (int tx = 0; tx < b; ++tx) {
        int n = offs[tx + 1] - offs[tx];
        const uint8_t* src = text.data() + offs[tx];
        const int shift = (prefix && n > 0 && src[0] != 0x20) ? 1 : 0;
        std::vector<uint8_t> c(n + shift), k(n + shift);
        if (shift) c[0] = 0x20;
        if (n) memcpy(c.data() + shift, src, n);
        n += shift;
        std::vector<int64_t> out(M - 2);
        std::vector<int32_t> w0(n), w1(n), w2(n), w3(n);
        const int got = bpe::encode_text_utf8(t, u, c.data(), n, M - 2, out.data(), k.data(), w0.data(), w1.data(), w2.data(), w3.data());
        if (got < 0) { printf("-1\n"); continue; }
        printf("%d", hd[5]);
        for (int i = 0; i < got; ++i) printf(" %lld", (long long)out[i]);
        printf(" %d\n", hd[6]);
    }
    return 0;
}
"""


@pytest.mark.skipif(_host_compiler() is None, reason="no clang++ found")
@pytest.mark.parametrize("kind", ["roberta_prefix", "modernbert"])
def test_core_header_under_host_sanitizers(kind, tmp_path):
    """bpe_core.h as plain C++ in a stand-alone program built with -fsanitize=address,undefined: clean, and the same ids as the
    library.  The tables, every text and its class array sit in exact-size heap blocks, so a decode past a truncated tail, the
    `p + width` read behind a text's last whitespace character or a look-back in front of its first byte is reported."""
    ht = H.HostTables(H.build_tokenizer(kind))
    texts = ht.device_route(H.text_set(kind, 300, seed=41))
    edges = ["tail\u00a0", "tail \u3000", "\u2028", "a\u0085", "x's", "x'r", "x'", "é'", "'", "é's", "'sé", "中"]
    raws = [t.encode("utf-8") for t in texts + edges] + list(MALFORMED.values()) + [b"tail \xc3", b"\xf0", b"\xe4", b" \xe2\x80"]
    M = 24
    data = str(tmp_path / "bpe_utf8.bin")
    H.dump(ht, raws, M, data)
    src, exe = tmp_path / "bpe_utf8_main.cpp", str(tmp_path / "bpe_utf8_main")
    src.write_text(SANITIZER_MAIN)
    subprocess.run([_host_compiler(), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover",
                    "-I", CSRC, str(src), "-o", exe], check=True, capture_output=True, text=True)
    run = subprocess.run([exe, data], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    lines = run.stdout.strip("\n").split("\n")
    assert lines[0] == "".join(str(_cls(c)) for c in range(128))
    ids, _, lens = H.encode_host(ht, raws, M)
    want = [" ".join(str(x) for x in ids[i, :lens[i]]) if lens[i] >= 0 else "-1" for i in range(len(raws))]
    assert lines[1:] == want
    assert want[-4:] == ["-1"] * 4 and "-1" not in want[:len(texts) + len(edges)]
