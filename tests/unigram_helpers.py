"""Shared by test_unigram_tokenizer_cpu.py and test_unigram_tokenizer_gpu.py: SentencePiece-style Unigram tokenizers built
in-process (no pretrained vocabulary is available offline) in the four pipelines the device path covers, over two trained
vocabularies and one hand-made vocabulary of exact score ties; the text set is bpe_helpers'."""
import ctypes
import functools
import io

import numpy as np

from bpe_helpers import FIXED, WORDS, _corpus, pack, random_texts  # noqa: F401  (re-exported for the two test files)

PIPELINES = ("deberta", "deberta_lower", "xlmr", "xlmr_legacy")
VOCABS = ("full", "sparse")          # full: all printable ASCII in the alphabet (no unknowns); sparse: no initial alphabet
CONFIGS = tuple((v, p) for v in VOCABS for p in PIPELINES)

PRINTABLE = [chr(c) for c in range(0x21, 0x7f)]

TIE_VOCAB = [("<unk>", 0.0), ("▁", -1.0), ("a", -1.0), ("b", -1.0), ("ab", -2.0), ("▁a", -2.0), ("▁ab", -3.0),
             ("c", -1.0), ("bc", -2.0), ("abc", -3.0)]
TIE_ROWS = [("ab", ["▁ab"]), ("abc", ["▁", "abc"]), ("abcab", ["▁", "abc", "ab"]),
            ("aXYb", ["▁a", "<unk>", "b"]), ("XY", ["▁", "<unk>"]), ("aXbYc", ["▁a", "<unk>", "b", "<unk>", "c"])]


@functools.lru_cache(maxsize=None)
def trained_pieces(which):
    """[(piece, score)] of a Unigram model trained on bpe_helpers._corpus() behind Metaspace(always)."""
    from tokenizers import Tokenizer, models, pre_tokenizers, trainers
    assert which in VOCABS
    tk = Tokenizer(models.Unigram())
    tk.pre_tokenizer = pre_tokenizers.Metaspace(replacement="▁", prepend_scheme="always")
    kw = {"initial_alphabet": PRINTABLE} if which == "full" else {}
    tk.train_from_iterator(_corpus(), trainers.UnigramTrainer(vocab_size=500, special_tokens=[], unk_token=None,
                                                              show_progress=False, **kw))
    import json
    return tuple((p, float(s)) for p, s in json.loads(tk.to_str())["model"]["vocab"])


@functools.lru_cache(maxsize=None)
def charsmap():
    """The precompiled_charsmap (NFKC-based) of a sentencepiece model trained in-process: what XLM-R's normalizer holds."""
    import sentencepiece as spm
    from sentencepiece import sentencepiece_model_pb2 as pb
    out = io.BytesIO()
    spm.SentencePieceTrainer.train(sentence_iterator=iter(_corpus()), model_writer=out, vocab_size=300, minloglevel=2)
    m = pb.ModelProto()
    m.ParseFromString(out.getvalue())
    return bytes(m.normalizer_spec.precompiled_charsmap)


def _deberta_vocab(pieces):
    # DebertaV2Tokenizer's own layout: [PAD] [CLS] [SEP] [UNK] in front, [MASK] behind (it adds what is missing)
    return [("[PAD]", 0.0), ("[CLS]", 0.0), ("[SEP]", 0.0), ("[UNK]", 0.0)] + list(pieces)


def _xlmr_vocab(pieces):
    return [("<s>", 0.0), ("<pad>", 0.0), ("</s>", 0.0), ("<unk>", 0.0)] + list(pieces)


@functools.lru_cache(maxsize=None)
def build_tokenizer(which, pipeline):
    """The wrapped tokenizer of one configuration.
    deberta / deberta_lower: transformers.DebertaV2Tokenizer(vocab=..., unk_id=3[, do_lower_case=True]);
    xlmr: transformers.XLMRobertaTokenizer(vocab=..., _spm_precompiled_charsmap=charsmap());
    xlmr_legacy: the serialised form of older XLM-R tokenizer.json files, built with `tokenizers` directly --
        Sequence[Precompiled, Replace(" {2,}", " ")] + Metaspace(always) without WhitespaceSplit + "<s> $A </s>" --
        wrapped in PreTrainedTokenizerFast."""
    assert pipeline in PIPELINES
    pieces = trained_pieces(which)
    if pipeline in ("deberta", "deberta_lower"):
        from transformers import DebertaV2Tokenizer
        return DebertaV2Tokenizer(vocab=_deberta_vocab(pieces), unk_id=3, do_lower_case=(pipeline == "deberta_lower"))
    if pipeline == "xlmr":
        from transformers import XLMRobertaTokenizer
        return XLMRobertaTokenizer(vocab=_xlmr_vocab(pieces), _spm_precompiled_charsmap=charsmap())
    return legacy_tokenizer(_xlmr_vocab(pieces))


def legacy_tokenizer(vocab, unk_id=3, normalizer="default", pre_tokenizer=None, byte_fallback=False, **hf_kw):
    """PreTrainedTokenizerFast over a hand-assembled Unigram pipeline (the xlmr_legacy form by default); the recognition test
    departs from it one setting at a time."""
    from tokenizers import Regex, Tokenizer, decoders, models, normalizers, pre_tokenizers, processors
    from transformers import PreTrainedTokenizerFast
    tk = Tokenizer(models.Unigram(list(vocab), unk_id=unk_id, byte_fallback=byte_fallback))
    if normalizer == "default":
        normalizer = normalizers.Sequence([normalizers.Precompiled(charsmap()), normalizers.Replace(Regex(" {2,}"), " ")])
    if normalizer is not None:
        tk.normalizer = normalizer
    tk.pre_tokenizer = pre_tokenizer or pre_tokenizers.Metaspace(replacement="▁", prepend_scheme="always")
    tk.decoder = decoders.Metaspace(replacement="▁", prepend_scheme="always")
    tk.post_processor = processors.TemplateProcessing(single="<s> $A </s>", special_tokens=[("<s>", 0), ("</s>", 2)])
    kw = dict(bos_token="<s>", eos_token="</s>", cls_token="<s>", sep_token="</s>", pad_token="<pad>", unk_token="<unk>",
              model_input_names=["input_ids", "attention_mask"])
    kw.update(hf_kw)
    return PreTrainedTokenizerFast(tokenizer_object=tk, **kw)


@functools.lru_cache(maxsize=None)
def tie_tokenizer():
    """The hand-made vocabulary of exact score ties behind WhitespaceSplit + Metaspace(always), no normalizer (Metaspace alone
    without a normalizer turns every space of a run into a piece and is not a recognised pipeline); <s> / </s> / <pad> are
    added tokens behind the ten pieces (ids 10, 11, 12)."""
    from tokenizers import Tokenizer, models, pre_tokenizers, processors
    from transformers import PreTrainedTokenizerFast
    tk = Tokenizer(models.Unigram(list(TIE_VOCAB), unk_id=0, byte_fallback=False))
    tk.pre_tokenizer = pre_tokenizers.Sequence([pre_tokenizers.WhitespaceSplit(),
                                                pre_tokenizers.Metaspace(replacement="▁", prepend_scheme="always")])
    tk.add_special_tokens(["<s>", "</s>", "<pad>"])
    tk.post_processor = processors.TemplateProcessing(single="<s> $A </s>", special_tokens=[("<s>", 10), ("</s>", 11)])
    return PreTrainedTokenizerFast(tokenizer_object=tk, bos_token="<s>", eos_token="</s>", cls_token="<s>", sep_token="</s>",
                                   pad_token="<pad>", unk_token="<unk>", model_input_names=["input_ids", "attention_mask"])


ELIGIBLE = frozenset(range(0x20, 0x7f)) | {0x09, 0x0a, 0x0d}


def eligible(text, specials=()):
    """The device route's rule: bytes 0x20-0x7E plus \\t \\n \\r, at most 4096 bytes, no literal special-token string."""
    return (text.isascii() and len(text) <= 4096 and all(ord(c) in ELIGIBLE for c in text)
            and not any(s in text for s in specials))


def host_route_texts(hf):
    """Texts the wrapper must hand to the wrapped tokenizer: non-ASCII, an emoji, a literal special token, over 4096 bytes."""
    return ["café naïve résumé", "emoji \U0001f600 here", "has a %s literal inside" % hf.sep_token, "long " * 900]


def longest_word(text):
    """Bytes of the longest whitespace-separated word plus 1 (its ▁); 0 for a text without a word."""
    return max((len(w) + 1 for w in text.split()), default=0)


class HostVocab:
    """ac_unigram_vocab over host (numpy) arrays, built by the wrapper's own table builder."""

    def __init__(self, hf):
        from adaptive_classifier import tokenizer as tkz
        self.spec = tkz._unigram_spec(hf)
        assert self.spec is not None
        self.arrays, self.slots = tkz.build_unigram_tables(self.spec)
        self.struct = tkz.unigram_vocab_struct(self.spec, [a.ctypes.data for a in self.arrays], self.slots)


def dump(hv, texts, max_length, path):
    """Table + texts as one little-endian binary file, for a stand-alone C++ program over csrc/unigram_core.h:
    int32 [16] slots, blob bytes, b, text bytes, max_length, max_piece, unk, cls, sep, pad, lowercase, trailing_space_piece,
    ws_controls, 0, 0, 0 | float64 unk_score | keys | entries | scores | blob | offsets [b + 1] | text"""
    keys, entries, scores, blob = hv.arrays
    text, offs = pack(texts)
    text = text[:offs[-1]]                                 # exactly the texts' bytes: no slack behind the last one
    v = hv.struct
    head = np.array([hv.slots, len(blob), len(texts), len(text), max_length, v.max_piece, v.unk_id, v.cls_id, v.sep_id, v.pad_id,
                     v.lowercase, v.trailing_space_piece, v.ws_controls, 0, 0, 0], np.int32)
    with open(path, "wb") as f:
        for a in (head, np.array([v.unk_score], np.float64), keys, entries, scores, blob, offs, text):
            f.write(np.ascontiguousarray(a).tobytes())


def encode_host(hv, texts, max_length):
    """ac_unigram_encode_host -> (ids int64 [b, max_length], mask, lens)"""
    from adaptive_classifier import _native as nv
    blob, offs = pack(texts)
    b = len(texts)
    ids = np.full((b, max_length), -7, np.int64)
    mask = np.full((b, max_length), -7, np.int64)
    lens = np.full(b, -7, np.int32)
    rc = nv.lib().ac_unigram_encode_host(blob.ctypes.data, offs.ctypes.data, b, ctypes.byref(hv.struct), max_length, ids.ctypes.data,
                                         mask.ctypes.data, lens.ctypes.data)
    assert rc == 0, nv.lib().ac_last_error()
    return ids, mask, lens
