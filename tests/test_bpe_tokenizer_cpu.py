"""CPU side of the byte-level BPE device tokenizer: csrc/bpe_core.h through ac_bpe_encode_host (the routines the kernel
runs, text by text on the host) against the tokenizers library, the pair hash, tokenizer recognition (_bpe_spec), argument
validation, and the same header under a host sanitizer in a stand-alone program.  No GPU needed.

The vocabularies are trained in-process (bpe_helpers.build_tokenizer): no pretrained vocabulary is available offline."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import bpe_helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "adaptive-classifier_amd", "csrc")


def _device_route(hv, texts):
    """The texts the wrapper sends to the kernel: ASCII, at most 4096 bytes, free of special / added-token strings (in the
    ModernBERT-style configuration the added token of two spaces sends every text with a double space to the host)."""
    return [t for t in texts if t.isascii() and len(t) <= 4096 and not any(s in t for s in hv.spec["specials"])]


@pytest.fixture(scope="module", params=H.CONFIGS)
def setup(request):
    hf = H.build_tokenizer(request.param)
    hv = H.HostVocab(hf)
    return request.param, hf, hv, _device_route(hv, H.text_set(request.param, 3000))


@pytest.mark.parametrize("max_length", [512, 24, 8, 2])
def test_host_encode_equals_tokenizers(setup, max_length):
    """ids, mask and lengths identical to the wrapped tokenizer called as the classifier calls it, on every text of the set
    that is routed to the device: no tolerance."""
    kind, hf, hv, texts = setup
    assert len(texts) > (1000 if kind == "modernbert" else 2500)
    for t in H.FIXED:                                      # none of the fixed cases is lost to routing without a reason
        assert t in texts or (kind == "modernbert" and "  " in t), t
    want = hf(texts, max_length=max_length, truncation=True, padding=True, return_tensors="np")
    ids, mask, lens = H.encode_host(hv, texts, max_length)
    S = want["input_ids"].shape[1]
    bad = np.nonzero((ids[:, :S] != want["input_ids"]).any(1) | (mask[:, :S] != want["attention_mask"]).any(1))[0]
    assert len(bad) == 0, [(texts[i][:60], ids[i, :S].tolist()[:16], want["input_ids"][i].tolist()[:16]) for i in bad[:3]]
    assert (ids[:, S:] == hv.spec["pad_id"]).all() and (mask[:, S:] == 0).all()
    assert np.array_equal(lens, want["attention_mask"].sum(1)) and int(lens.max()) == S


def test_pair_hash_is_fnv1a_with_a_separator_step():
    from adaptive_classifier import _native as nv

    def fnv(left, right):
        h = 0xcbf29ce484222325
        for c in list(left) + [0x100] + list(right):
            h = ((h ^ c) * 0x100000001b3) & 0xffffffffffffffff
        return h or 1

    def native(left, right):
        return nv.lib().ac_bpe_pair_hash((ctypes.c_uint8 * max(1, len(left))).from_buffer_copy(left or b"\0"), len(left),
                                         (ctypes.c_uint8 * max(1, len(right))).from_buffer_copy(right or b"\0"), len(right))

    for left, right in [(b"a", b"bc"), (b"ab", b"c"), (b"\xc4\xa0", b"the"), (b"", b""), (b"x", b""), (bytes(range(256)), b"\xff\x00")]:
        assert native(left, right) == fnv(left, right), (left, right)
    assert native(b"a", b"bc") != native(b"ab", b"c")


def test_bpe_spec_recognition():
    """Recognised by the serialised configuration: the three configurations are taken, everything else is left alone."""
    from tokenizers import Tokenizer, models, pre_tokenizers, processors, trainers
    from transformers import BertTokenizer, PreTrainedTokenizerFast
    from adaptive_classifier.tokenizer import _bpe_spec, _wordpiece_spec
    for kind in H.CONFIGS:
        spec = _bpe_spec(H.build_tokenizer(kind))
        assert spec is not None and spec["add_prefix_space"] == (kind == "roberta_prefix")
        assert (spec["cls_id"], spec["sep_id"], spec["pad_id"]) == ((1, 2, 3) if kind == "modernbert" else (0, 2, 1))
        assert spec["token_type_ids"] == (kind == "roberta_prefix")
        assert ("  " in spec["specials"]) == (kind == "modernbert")
        assert _wordpiece_spec(H.build_tokenizer(kind)) is None

    specials = ["<s>", "<pad>", "</s>", "<unk>"]

    def variant(model=None, pre=None, post="roberta", pad="<pad>", **hf_kw):
        tk = Tokenizer(model or models.BPE())
        tk.pre_tokenizer = pre or pre_tokenizers.ByteLevel(add_prefix_space=False, use_regex=True)
        tk.train_from_iterator(["the cat sat on the mat", "it's the hat"] * 5,
                               trainers.BpeTrainer(vocab_size=300, initial_alphabet=pre_tokenizers.ByteLevel.alphabet(),
                                                   special_tokens=specials, show_progress=False))
        tk.post_processor = (processors.RobertaProcessing(sep=("</s>", 2), cls=("<s>", 0)) if post == "roberta"
                             else processors.ByteLevel(trim_offsets=False))
        return PreTrainedTokenizerFast(tokenizer_object=tk, pad_token=pad, unk_token="<unk>", **hf_kw)

    assert _bpe_spec(variant()) is not None                                              # the base the variants depart from
    vocab = {t: i for i, t in enumerate(["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]", "a", "b", "##a"])}
    bert = BertTokenizer(vocab=vocab, do_lower_case=True)
    assert _bpe_spec(bert) is None                                                       # a WordPiece tokenizer
    assert _bpe_spec(variant(model=models.BPE(ignore_merges=True))) is None
    assert _bpe_spec(variant(model=models.BPE(dropout=0.1))) is None
    assert _bpe_spec(variant(pre=pre_tokenizers.ByteLevel(add_prefix_space=False, use_regex=False))) is None
    assert _bpe_spec(variant(pre=pre_tokenizers.Sequence([pre_tokenizers.ByteLevel(add_prefix_space=False, use_regex=True)]))) is None
    assert _bpe_spec(variant(padding_side="left")) is None
    assert _bpe_spec(variant(pad=None)) is None
    assert _bpe_spec(variant(post="gpt2")) is None                                       # no specials around the sequence
    # ... and the WordPiece recognition is what it was
    wp = _wordpiece_spec(bert)
    assert wp is not None and wp[0] == vocab and wp[1] is True
    assert set(wp[2]) == {"[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"}
    assert _wordpiece_spec(BertTokenizer(vocab=vocab, do_lower_case=False))[1] is False


def test_argument_validation_without_gpu():
    from adaptive_classifier import _native as nv
    L = nv.lib()
    assert L.ac_version() >= 10
    hv = H.HostVocab(H.build_tokenizer("roberta"))
    blob, offs = H.pack(["ab", "c"])
    ids, mask, lens = np.zeros((2, 8), np.int64), np.zeros((2, 8), np.int64), np.zeros(2, np.int32)
    p = lambda a: a.ctypes.data                                                          # noqa: E731

    def both(text, offsets, b, vocab, M, i, m, n):
        v = ctypes.byref(vocab) if vocab is not None else None
        return (L.ac_bpe_encode(text, offsets, b, v, M, i, m, n, None), L.ac_bpe_encode_host(text, offsets, b, v, M, i, m, n))

    EINVAL = -1
    assert both(p(blob), p(offs), 2, None, 8, p(ids), p(mask), p(lens)) == (EINVAL, EINVAL)
    assert both(p(blob), None, 2, hv.struct, 8, p(ids), p(mask), p(lens)) == (EINVAL, EINVAL)
    assert both(p(blob), p(offs), 2, hv.struct, 8, None, p(mask), p(lens)) == (EINVAL, EINVAL)
    assert both(p(blob), p(offs), 2, hv.struct, 8, p(ids), None, p(lens)) == (EINVAL, EINVAL)
    assert both(p(blob), p(offs), 2, hv.struct, 8, p(ids), p(mask), None) == (EINVAL, EINVAL)
    assert both(p(blob), p(offs), 2, hv.struct, 1, p(ids), p(mask), p(lens)) == (EINVAL, EINVAL)      # max_length < 2
    assert both(None, p(offs), 2, hv.struct, 8, p(ids), p(mask), p(lens)) == (EINVAL, EINVAL)         # text NULL with b > 0
    assert b"bpe" in L.ac_last_error()
    from adaptive_classifier.tokenizer import bpe_vocab_struct
    odd = bpe_vocab_struct(hv.spec, [a.ctypes.data for a in hv.arrays], hv.slots - 1)              # not a power of two
    assert both(p(blob), p(offs), 2, odd, 8, p(ids), p(mask), p(lens)) == (EINVAL, EINVAL)
    holes = bpe_vocab_struct(hv.spec, [hv.arrays[0].ctypes.data, None, hv.arrays[2].ctypes.data, hv.arrays[3].ctypes.data], hv.slots)
    assert both(p(blob), p(offs), 2, holes, 8, p(ids), p(mask), p(lens)) == (EINVAL, EINVAL)
    assert both(None, p(offs), 0, hv.struct, 8, p(ids), p(mask), p(lens)) == (0, 0)                   # b == 0: nothing to do


def test_bpe_kernel_has_no_scratch():
    """The symbol state is a wave-uniform mask plus registers: the device listing of bpe.hip must show no private segment
    (read the way test_kernel_resources_cpu.py reads listings)."""
    from test_kernel_resources_cpu import HIPCC, kernel_resources
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    res = {k: v for k, v in kernel_resources("bpe.hip").items() if "bpe_kernel" in k}
    assert len(res) == 1, res
    (scratch, vgpr), = res.values()
    assert scratch == 0 and vgpr <= 128, (scratch, vgpr)      # 128 VGPRs: four waves per SIMD stay possible


SANITIZER_MAIN = r"""
// stand-alone: csrc/bpe_core.h over a dumped table and texts (bpe_helpers.dump), one line of ids per text
#include <cstdio>
#include <cstring>
#include <vector>
#include "bpe_core.h"
int main(int argc, char** argv) {
    FILE* f = argc > 1 ? fopen(argv[1], "rb") : nullptr;
    if (!f) return 2;
    int32_t hd[10];
    if (fread(hd, 4, 10, f) != 10) return 2;
    const int slots = hd[0], blob_len = hd[1], b = hd[2], text_len = hd[3], M = hd[4], prefix = hd[8];
    // exact-size heap blocks: a read past any table or past a text's end is a report
    std::vector<uint64_t> keys(slots);
    std::vector<int32_t> entries(4 * (size_t)slots), byte_id(256), offs(b + 1);
    std::vector<uint8_t> blob(blob_len), text(text_len);
    bool ok = fread(keys.data(), 8, slots, f) == (size_t)slots && fread(entries.data(), 4, 4 * (size_t)slots, f) == 4 * (size_t)slots &&
              fread(blob.data(), 1, blob_len, f) == (size_t)blob_len && fread(byte_id.data(), 4, 256, f) == 256 &&
              fread(offs.data(), 4, b + 1, f) == (size_t)b + 1 && fread(text.data(), 1, text_len, f) == (size_t)text_len;
    fclose(f);
    if (!ok) return 2;
    const bpe::Table t{keys.data(), entries.data(), blob.data(), byte_id.data(), (uint32_t)(slots - 1)};
    for (int tx = 0; tx < b; ++tx) {
        int n = offs[tx + 1] - offs[tx];
        const uint8_t* src = text.data() + offs[tx];
        const int shift = (prefix && n > 0 && src[0] != 0x20) ? 1 : 0;
        std::vector<uint8_t> c(n + shift);
        if (shift) c[0] = 0x20;
        if (n) memcpy(c.data() + shift, src, n);
        n += shift;
        std::vector<int64_t> out(M - 2);
        std::vector<int32_t> w0(n), w1(n), w2(n), w3(n);
        const int k = bpe::encode_text(t, c.data(), n, M - 2, out.data(), w0.data(), w1.data(), w2.data(), w3.data());
        printf("%d", hd[5]);
        for (int i = 0; i < k; ++i) printf(" %lld", (long long)out[i]);
        printf(" %d\n", hd[6]);
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
    """bpe_core.h as plain C++ in a stand-alone program built with -fsanitize=address,undefined: clean, and the same ids as
    the library.  The tables and every text sit in exact-size heap blocks, so a probe or a look-ahead past an end is reported."""
    kind = "roberta_prefix"
    hv = H.HostVocab(H.build_tokenizer(kind))
    texts = _device_route(hv, H.text_set(kind, 400, seed=23))
    M = 24
    data = str(tmp_path / "bpe.bin")
    H.dump(hv, texts, M, data)
    src, exe = tmp_path / "bpe_main.cpp", str(tmp_path / "bpe_main")
    src.write_text(SANITIZER_MAIN)
    subprocess.run([_host_compiler(), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover",
                    "-I", CSRC, str(src), "-o", exe], check=True, capture_output=True, text=True)
    run = subprocess.run([exe, data], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    ids, _, lens = H.encode_host(hv, texts, M)
    want = [" ".join(str(x) for x in ids[i, :lens[i]]) for i in range(len(texts))]
    assert run.stdout.strip("\n").split("\n") == want
