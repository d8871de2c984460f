"""Shared by test_unigram_unicode_cpu.py and test_unigram_unicode_gpu.py: SentencePiece-style Unigram tokenizers in the four
pipelines of unigram_helpers over MULTILINGUAL vocabularies trained in-process (nothing pretrained is available offline), a
hand-made vocabulary of exact score ties with multi-byte characters, the text sets (fixed cases, block-edge words, a random
generator) and the host-table wrapper."""
import ctypes
import functools
import json

import numpy as np

import unigram_helpers as UH
import wordpiece_helpers as WH
from wordpiece_helpers import MALFORMED, pack, raw, reference  # noqa: F401  (re-exported for the two test files)

PIPELINES = UH.PIPELINES
VOCABS = ("full", "sparse")          # full: every pool character in the alphabet (few unknowns); sparse: no initial alphabet
CONFIGS = tuple((v, p) for v in VOCABS for p in PIPELINES)
BUF = 5120                           # unigram::kUtf8BufBytes
REACH = 64                           # unigram::kReach

POOL = {name: cps for name, cps, _ in WH.POOLS}
# pools without joining code points (no combining marks, vowel signs, jamo, ZWJ): texts over them are device texts
PLAIN_POOLS = ("ascii", "latin", "greek", "cyrillic", "kana", "cjk", "hangul", "punct", "fullwidth", "astral_cjk", "single", "emoji")
TRAIN_POOLS = ("ascii", "latin", "greek", "cyrillic", "kana", "cjk", "hangul", "fullwidth")

CJK_99 = "東京都に住んでいます。今日は天気がいいですね、散歩に行きましょう。"
assert len(CJK_99.encode()) == 99


def _lexicon():
    """Per training pool 120 'words' of 1-5 characters: what the corpus repeats, so that multi-character pieces emerge."""
    rng = np.random.default_rng(17)
    return {name: ["".join(chr(POOL[name][int(i)]) for i in rng.integers(0, len(POOL[name]), int(rng.integers(1, 6))))
                   for _ in range(120)] for name in TRAIN_POOLS}


@functools.lru_cache(maxsize=None)
def _corpus(words_per_pool=120):
    rng = np.random.default_rng(19)
    lex = _lexicon()
    out = list(UH._corpus())
    for _ in range(1500):
        name = TRAIN_POOLS[int(rng.integers(0, len(TRAIN_POOLS)))]
        words = [lex[name][int(i)] for i in rng.integers(0, words_per_pool, int(rng.integers(2, 10)))]
        out.append(("" if name in ("cjk", "kana") and rng.random() < 0.5 else " ").join(words))
    out.append(CJK_99)
    return out


@functools.lru_cache(maxsize=None)
def trained_pieces(which):
    """[(piece, score)] of a Unigram model trained on the multilingual corpus behind Metaspace(always)."""
    from tokenizers import Tokenizer, models, pre_tokenizers, trainers
    assert which in VOCABS
    tk = Tokenizer(models.Unigram())
    tk.pre_tokenizer = pre_tokenizers.Metaspace(replacement="▁", prepend_scheme="always")
    if which == "full":
        alphabet = UH.PRINTABLE + sorted({chr(cp) for name in TRAIN_POOLS for cp in POOL[name]} | set(CJK_99))
        kw = dict(vocab_size=4000, initial_alphabet=alphabet)
    else:                                                  # a quarter of each pool's words: most characters are unknown
        kw = dict(vocab_size=1000)
    tk.train_from_iterator(_corpus(120 if which == "full" else 30), trainers.UnigramTrainer(special_tokens=[], unk_token=None, show_progress=False, **kw))
    return tuple((p, float(s)) for p, s in json.loads(tk.to_str())["model"]["vocab"])


@functools.lru_cache(maxsize=None)
def build_tokenizer(which, pipeline):
    """unigram_helpers.build_tokenizer over the multilingual vocabulary."""
    assert pipeline in PIPELINES
    pieces = trained_pieces(which)
    if pipeline in ("deberta", "deberta_lower"):
        from transformers import DebertaV2Tokenizer
        return DebertaV2Tokenizer(vocab=UH._deberta_vocab(pieces), unk_id=3, do_lower_case=(pipeline == "deberta_lower"))
    if pipeline == "xlmr":
        from transformers import XLMRobertaTokenizer
        return XLMRobertaTokenizer(vocab=UH._xlmr_vocab(pieces), _spm_precompiled_charsmap=UH.charsmap())
    return UH.legacy_tokenizer(UH._xlmr_vocab(pieces))


# exact score ties over multi-byte characters: é (2 bytes), 中 (3 bytes); ß (2 bytes) and 文 (3 bytes) are in no piece
TIE_VOCAB = [("<unk>", 0.0), ("▁", -1.0), ("é", -1.0), ("a", -1.0), ("éa", -2.0), ("▁é", -2.0), ("▁éa", -3.0),
             ("中", -1.0), ("a中", -2.0), ("éa中", -3.0)]
TIE_ROWS = [("éa", ["▁éa"]), ("éa中", ["▁", "éa中"]), ("éa中éa", ["▁", "éa中", "éa"]),
            ("é文ßa", ["▁é", "<unk>", "a"]), ("文ß", ["▁", "<unk>"]), ("é文aß中", ["▁é", "<unk>", "a", "<unk>", "中"])]


@functools.lru_cache(maxsize=None)
def tie_tokenizer():
    """unigram_helpers.tie_tokenizer's pipeline (WhitespaceSplit + Metaspace(always), no normalizer) over TIE_VOCAB."""
    from tokenizers import Tokenizer, models, pre_tokenizers, processors
    from transformers import PreTrainedTokenizerFast
    tk = Tokenizer(models.Unigram(list(TIE_VOCAB), unk_id=0, byte_fallback=False))
    tk.pre_tokenizer = pre_tokenizers.Sequence([pre_tokenizers.WhitespaceSplit(),
                                                pre_tokenizers.Metaspace(replacement="▁", prepend_scheme="always")])
    tk.add_special_tokens(["<s>", "</s>", "<pad>"])
    tk.post_processor = processors.TemplateProcessing(single="<s> $A </s>", special_tokens=[("<s>", 10), ("</s>", 11)])
    return PreTrainedTokenizerFast(tokenizer_object=tk, bos_token="<s>", eos_token="</s>", cls_token="<s>", sep_token="</s>",
                                   pad_token="<pad>", unk_token="<unk>", model_input_names=["input_ids", "attention_mask"])


def _chars(n_bytes, shift=0, width2="éüñ", width3="中日本한가"):
    """A word of exactly n_bytes bytes: `shift` 2-byte characters, then 3-byte ones (with the metaspace in front the 64-byte block
    edges fall behind, one byte into and two bytes into a character for shift 0, 1, 2), 2-byte and 1-byte ones to fill."""
    out, left, i = [width2[j % len(width2)] for j in range(shift)], n_bytes - 2 * shift, 0
    while left:
        take = 3 if left >= 3 and left != 4 else 2 if left >= 2 else 1
        out.append(width3[i % len(width3)] if take == 3 else width2[i % len(width2)] if take == 2 else "x")
        left -= take
        i += 1
    word = "".join(out)
    assert len(word.encode()) == n_bytes
    return word


def straddling_word(pieces):
    """A word of REACH + 1 bytes with its metaspace in which the longest multi-byte piece of `pieces` (no metaspace in it) lies
    across the edge between the first and the second block of 64 ends, and that piece's byte length."""
    cands = [p for p, _ in pieces if "▁" not in p and not p.isascii() and len(p) > 1]
    piece = max(cands, key=lambda p: len(p.encode()))
    k = len(piece.encode())
    head = _chars(63 - k // 2)                              # the metaspace is byte 0: the piece starts at byte 64 - k // 2
    word = head + piece
    word += _chars(REACH - len(word.encode())) if len(word.encode()) < REACH else ""
    return word, k


EDGE_WORDS = [_chars(n, s) for n in (62, 63, 64, 65, 66, 127, 128, 129, 191, 192, 193, 300) for s in (0, 1, 2)]   # + 1: the metaspace
LONG_CJK = (CJK_99 * 11)[:340]                              # ~1000 bytes without a space
assert 1000 <= len(LONG_CJK.encode()) <= 1024
OVERFLOW = "\ufdfa" * 1300                                  # 3 bytes -> an 18-code-point image: beyond the buffer in NFKC pipelines

FIXED = list(WH.FIXED) + [
    CJK_99, LONG_CJK, "a " * 2048, "\u00e9" * 2048, "\u4e2d" * 1365 + "a", OVERFLOW,
    "\uff21\u0301", "\uff21\uff22\uff23", "ABC", "a\u3000b", "\u6587\u00df", "x\u6587\u00dfy", "caf\u00e9 na\u00efve", "trailing\u3000",
    " leading", "\u041f\u0440\u0438\u0432\u0435\u0442, \u041c\u0418\u0420! \u0401\u043b\u043a\u0430 \u0438 " + "\u0451\u043b\u043a\u0430" * 20,
    "\ud55c\uad6d\uc5b4\ud14d\uc2a4\ud2b8" * 12, "\uff57\uff49\uff44\uff54\uff48" * 15, " ".join(EDGE_WORDS[:6]),
] + EDGE_WORDS + ["lead " + w + " tail" for w in EDGE_WORDS[6:18]]


def random_texts(n, seed):
    """Each text draws from 1-3 pools: 85 % of the texts from the pools without joining code points only, 15 % from all of
    wordpiece_helpers.POOLS.  Words of 1-8 characters; about 8 % of the words are 30-120 characters long (over 64 bytes in most
    scripts).  Separated by spaces / tabs / newlines / U+3000 / punctuation / nothing."""
    rng = np.random.default_rng(seed)
    plain = [POOL[k] for k in PLAIN_POOLS]
    every = [cps for _, cps, _ in WH.POOLS]
    seps = [" ", " ", " ", " ", "  ", "\t", "\n", ", ", "\u3000", ""]      # U+3000 only in the texts over all pools
    out = []
    for _ in range(n):
        src = plain if rng.random() < 0.85 else every
        pools = [src[int(i)] for i in rng.integers(0, len(src), int(rng.integers(1, 4)))]
        ws = []
        for _ in range(int(rng.integers(1, 12))):
            cps = pools[int(rng.integers(0, len(pools)))]
            k = int(rng.integers(30, 121)) if rng.random() < 0.08 else int(rng.integers(1, 9))
            ws.append("".join(chr(cps[int(i)]) for i in rng.integers(0, len(cps), k)))
        use = seps if src is every else seps[:8] + seps[9:]
        out.append("".join(w + use[int(i)] for w, i in zip(ws, rng.integers(0, len(use), len(ws)))))
    return out


def longest_word_bytes(text):
    """Bytes of the longest whitespace-separated word plus 1 (its metaspace)."""
    return max((len(w.encode()) + 1 for w in text.split()), default=0)


class HostTables:
    """ac_unigram_vocab (every piece, UTF-8) and ac_unigram_unicode over host (numpy) arrays, built by the wrapper's own builders."""

    def __init__(self, hf, unicode_tables=None):
        from adaptive_classifier import tokenizer as tkz
        self.hf = hf
        self.spec = tkz._unigram_spec(hf)
        assert self.spec is not None
        self.spec.pop("tables")
        self.arrays, self.slots = tkz.build_unigram_tables(self.spec, utf8=True)
        self.struct = tkz.unigram_vocab_struct(self.spec, [a.ctypes.data for a in self.arrays], self.slots, utf8=True)
        self.tables = unicode_tables if unicode_tables is not None else tkz.build_unigram_unicode_tables(hf)
        self.unicode = tkz.unigram_unicode_struct(self.tables)
        self.host_only = tkz._host_only_regex(self.tables)
        self.specials = self.spec["specials"]

    def eligible(self, text):
        """The wrapper's rule for a non-ASCII text: at most 4096 bytes, no literal special token, no host-only code point."""
        return len(text.encode("utf-8")) <= 4096 and not any(sp in text for sp in self.specials) \
            and not (self.host_only is not None and self.host_only.search(text))

    def fits(self, text):
        """Does the normalised text, with its leading 0x20, fit the buffer?  (By the table's own images.)"""
        return 1 + sum(len(table_image(self.tables, ord(ch)).encode()) for ch in text) <= BUF


def table_image(tables, cp):
    """What the table says the normalizer chain makes of chr(cp): a string, or None for host-only."""
    e = int(tables["entries"][int(tables["page_of"][cp >> 8]), cp & 255])
    kind = e & 3
    if kind == 0:
        return chr(cp)
    if kind == 1:
        return ""
    if kind == 2:
        off, n = e >> 8, (e >> 2) & 63
        return bytes(tables["images"][off:off + n]).decode("utf-8")
    return None


def encode_host(ht, texts, max_length, slack=64):
    """ac_unigram_encode_utf8_host over str or bytes texts -> (ids int64 [b, max_length], mask, lens); untouched cells hold -7"""
    from adaptive_classifier import _native as nv
    blob, offs = pack(raw(texts), slack)
    b = len(texts)
    ids = np.full((b, max_length), -7, np.int64)
    mask = np.full((b, max_length), -7, np.int64)
    lens = np.full(b, -7, np.int32)
    rc = nv.lib().ac_unigram_encode_utf8_host(blob.ctypes.data, offs.ctypes.data, b, ctypes.byref(ht.struct), ctypes.byref(ht.unicode),
                                              max_length, ids.ctypes.data, mask.ctypes.data, lens.ctypes.data)
    assert rc == 0, nv.lib().ac_last_error()
    return ids, mask, lens


def dump(ht, raws, max_length, path):
    """Tables + texts as one little-endian binary file for a stand-alone C++ program over csrc/unigram_core.h:
    int32 [16] slots, blob bytes, b, text bytes, max_length, max_piece, unk, cls, sep, pad, trailing_space_piece, ws_controls,
    n_pages, image_bytes, 0, 0 | float64 unk_score | keys | entries | scores | blob | page_of | unicode entries |
    images[:image_bytes] | offsets [b + 1] | text (exactly its bytes)"""
    keys, entries, scores, blob = ht.arrays
    t = ht.tables
    text, offs = pack(raws, 0)
    text = text[:offs[-1]]
    v = ht.struct
    head = np.array([ht.slots, len(blob), len(raws), len(text), max_length, v.max_piece, v.unk_id, v.cls_id, v.sep_id, v.pad_id,
                     v.trailing_space_piece, v.ws_controls, t["n_pages"], t["image_bytes"], 0, 0], np.int32)
    with open(path, "wb") as f:
        for a in (head, np.array([v.unk_score], np.float64), keys, entries, scores, blob, t["page_of"], t["entries"],
                  t["images"][:t["image_bytes"]], offs, text):
            f.write(np.ascontiguousarray(a).tobytes())
