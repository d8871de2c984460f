"""Shared by test_bpe_unicode_cpu.py, test_bpe_unicode_gpu.py and test_stream_tokenizer_bpe_utf8_gpu.py: byte-level BPE tokenizers
trained in-process (no pretrained vocabulary is available offline) in the three configurations of bpe_helpers.py, over a corpus
that also holds accented words, typographic punctuation, Cyrillic, a few CJK characters and emoji -- so that merges inside and
across multi-byte characters exist -- and the text sets."""
import ctypes
import functools

import numpy as np

import bpe_helpers as B

CONFIGS = B.CONFIGS

UNI_WORDS = ("café naïve résumé façade jalapeño über straße crème brûlée déjà vu piñata "
             "привет мир спасибо хорошо плохо товар "
             "中文 产品 很好 不好 日本語 文本 한국어 "
             "it’s don’t we’ll “great” “bad” café's naïve's "
             "€5 £10 12² Ⅷ ١٢٣").split()
UNI_TAILS = [".", "!", "…", " — ok", " \U0001f600", " \U0001f44d\U0001f44d", "–", " « sic »", "", "?", " \U0001f600\U0001f600!"]
# the alphabet of the random strings: ASCII, contractions, letters / numbers / punctuation / whitespace of several scripts, emoji
ALPHABET = list("ab sx1!'") + ["'s", "'ll", "'re", "  ", "\t", "\n", "é", "ß", "Ж", "中", "한", "١", "²", "Ⅷ", "€",
                               "…", "’", "“", "\U0001f600", "\u200b", "\u00a0", "\u3000", "\u2028", "\u0085", "és", "中文"]


def _corpus():
    rng = np.random.default_rng(7)
    out = list(B._corpus())
    for _ in range(400):
        ws = [str(rng.choice(UNI_WORDS if rng.random() < 0.5 else B.WORDS)) for _ in range(int(rng.integers(3, 12)))]
        out.append(" ".join(ws) + str(rng.choice(UNI_TAILS)))
    return out


@functools.lru_cache(maxsize=None)
def build_tokenizer(kind):
    """bpe_helpers.build_tokenizer over the wider corpus, vocab_size 1100: the same three configurations (roberta, roberta_prefix:
    RobertaProcessing, no normalizer; modernbert: NFC, TemplateProcessing, an added non-special token of two spaces)."""
    from tokenizers import Tokenizer, models, normalizers, pre_tokenizers, processors, trainers, decoders
    from transformers import PreTrainedTokenizerFast
    assert kind in CONFIGS
    roberta = kind != "modernbert"
    specials = ["<s>", "<pad>", "</s>", "<unk>", "<mask>"] if roberta else ["[UNK]", "[CLS]", "[SEP]", "[PAD]", "[MASK]"]
    tk = Tokenizer(models.BPE())
    tk.pre_tokenizer = pre_tokenizers.ByteLevel(add_prefix_space=(kind == "roberta_prefix"), use_regex=True)
    tk.decoder = decoders.ByteLevel()
    if not roberta:
        tk.normalizer = normalizers.NFC()
    trainer = trainers.BpeTrainer(vocab_size=1100, initial_alphabet=pre_tokenizers.ByteLevel.alphabet(), special_tokens=specials,
                                  show_progress=False)
    tk.train_from_iterator(_corpus(), trainer)
    if roberta:
        tk.post_processor = processors.RobertaProcessing(sep=("</s>", 2), cls=("<s>", 0))
        hf = PreTrainedTokenizerFast(tokenizer_object=tk, bos_token="<s>", eos_token="</s>", cls_token="<s>", sep_token="</s>",
                                     pad_token="<pad>", unk_token="<unk>", mask_token="<mask>",
                                     model_input_names=["input_ids", "attention_mask"] if kind == "roberta" else
                                     ["input_ids", "token_type_ids", "attention_mask"])
        assert hf.pad_token_id == 1
    else:
        tk.post_processor = processors.TemplateProcessing(single="[CLS] $A [SEP]", special_tokens=[("[CLS]", 1), ("[SEP]", 2)])
        hf = PreTrainedTokenizerFast(tokenizer_object=tk, cls_token="[CLS]", sep_token="[SEP]", pad_token="[PAD]",
                                     unk_token="[UNK]", mask_token="[MASK]")
        hf.add_tokens(["  "])
    return hf


def multibyte_merges(hf):
    """(merges whose joined symbol lies inside one multi-byte character, merges whose joined symbol spans more than one character
    and holds a non-ASCII byte) of the trained vocabulary, in raw bytes"""
    from adaptive_classifier import tokenizer as tkz
    u2b = {u: b for b, u in tkz._byte_to_unicode().items()}
    inside = across = 0
    for left, right in tkz._bpe_spec(hf)["merges"]:
        raw = bytes(u2b[ch] for ch in left + right)
        if raw.isascii():
            continue
        leads = sum(1 for x in raw if (x & 0xC0) != 0x80)
        if leads <= 1:
            inside += 1
        else:
            across += 1
    return inside, across


FIXED = ["", "é", "中", "\U0001f600", "a", " ", "\u00a0", "\u3000",
         "it’s “quoted” — dash… en–dash", "café naïve résumé", "emoji \U0001f600 here \U0001f44d\U0001f3fd!",
         "é's", "'sé", "中's", "x’s", "x'ré", "x'reé", "é'llé é'S", "1'sé ١'s",
         "12²", "١٢٣4", "Ⅷ", "x²y 3é ½",
         "a\u00a0\u00a0b", "a \u00a0b", "a\u00a0 b", "a\u3000\u2028\u0085 b", "a\u3000\u2028\u0085b", "tail\u00a0\u3000", "tail \u2028", "\u2028\u0085", "\u00a0 \u3000", "\u0085lead",
         "\u00a0's", " \u00a0 's", "\u3000é", " \u3000 é",
         "Привет, мир! хорошо", "中文 mixed 文本 日本語", "한국어 text",
         "zero\u200bwidth soft\u00adhyphen \ufeffbom", "\U00020000\U0002a6d6 x\U00020000y", "€100 £5 ™ « x » ¿Qué?",
         "Hello, World!  This is GREAT...", "we'll see; they’ve gone, I’m sure"]

# what NFC changes or may combine (ModernBERT style: host-only there; RoBERTa style has no normalizer and takes them as they are)
NFC_SENSITIVE = ["e\u0301 combining", "A\u0301\u0323", "\u212b ngstrom", "\u1100\u1161 jamo", "가\u11a8", "\u0345 alone"]


def random_texts(n, seed):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        if i % 3 == 0:
            ws = [str(rng.choice(UNI_WORDS if rng.random() < 0.5 else B.WORDS)) for _ in range(int(rng.integers(1, 20)))]
            seps = [" ", " ", " ", "  ", "\u00a0", "\n", " \u3000", "\u2028 ", ""]
            out.append("".join(w + str(rng.choice(seps)) for w in ws) + str(rng.choice(UNI_TAILS)))
        else:
            out.append("".join(str(rng.choice(ALPHABET)) for _ in range(int(rng.integers(1, 40)))))
    return out


def text_set(kind, n_random, seed=31):
    return FIXED + NFC_SENSITIVE + random_texts(n_random, seed)


class HostTables:
    """ac_bpe_vocab and ac_bpe_unicode over host (numpy) arrays, built by the wrapper's own builders."""

    def __init__(self, hf):
        from adaptive_classifier import tokenizer as tkz
        self.hv = B.HostVocab(hf)
        self.spec, self.vocab = self.hv.spec, self.hv.struct
        self.tables = tkz.build_bpe_unicode_tables(hf)
        self.unicode = tkz.bpe_unicode_struct(self.tables)
        self.flagged = tkz._host_only_regex(self.tables)

    def device_route(self, texts):
        """the texts the wrapper sends to the kernel with unicode=True"""
        return [t for t in texts if len(t.encode("utf-8")) <= 4096 and not any(s in t for s in self.spec["specials"])
                and not (self.flagged is not None and self.flagged.search(t))]


def pack(raws):
    """(blob uint8 with 64 bytes of slack, offsets int32 [b + 1]) of byte strings"""
    offs = np.zeros(len(raws) + 1, np.int32)
    offs[1:] = np.cumsum([len(r) for r in raws])
    blob = np.frombuffer(b"".join(raws) + b"\0" * 64, np.uint8).copy()
    return blob, offs


def encode_host(ht, texts, max_length, fill=-7):
    """ac_bpe_utf8_encode_host over str or bytes texts -> (ids int64 [b, max_length], mask, lens), outputs pre-filled with `fill`"""
    from adaptive_classifier import _native as nv
    raws = [t if isinstance(t, bytes) else t.encode("utf-8") for t in texts]
    blob, offs = pack(raws)
    b = len(raws)
    ids = np.full((b, max_length), fill, np.int64)
    mask = np.full((b, max_length), fill, np.int64)
    lens = np.full(b, fill, np.int32)
    rc = nv.lib().ac_bpe_utf8_encode_host(blob.ctypes.data, offs.ctypes.data, b, ctypes.byref(ht.vocab), ctypes.byref(ht.unicode),
                                          max_length, ids.ctypes.data, mask.ctypes.data, lens.ctypes.data)
    assert rc == 0, nv.lib().ac_last_error()
    return ids, mask, lens


def dump(ht, raws, max_length, path):
    """Tables + texts as one little-endian binary file, for a stand-alone C++ program over csrc/bpe_core.h:
    int32 [12] slots, blob bytes, b, text bytes, max_length, cls, sep, pad, add_prefix_space, n_pages, 0, 0 | keys | entries | blob |
    byte_id | page_of | unicode entries | offsets [b + 1] | text"""
    keys, entries, blob, byte_id = ht.hv.arrays
    text, offs = pack(raws)
    text = text[:offs[-1]]                                 # exactly the texts' bytes: no slack behind the last one
    s, t = ht.spec, ht.tables
    head = np.array([ht.hv.slots, len(blob), len(raws), len(text), max_length, s["cls_id"], s["sep_id"], s["pad_id"],
                     1 if s["add_prefix_space"] else 0, t["n_pages"], 0, 0], np.int32)
    with open(path, "wb") as f:
        for a in (head, keys, entries, blob, byte_id, t["page_of"], t["entries"], offs, text):
            f.write(np.ascontiguousarray(a).tobytes())
