"""Shared by test_wordpiece_unicode_cpu.py and test_wordpiece_unicode_gpu.py: synthetic multilingual WordPiece vocabularies
(nothing pretrained is available offline), the three normalizer configurations, the text sets and the host-table wrapper."""
import ctypes
import functools

import numpy as np

CONFIGS = ("uncased", "cased", "uncased_keep_accents")
_KW = {"uncased": dict(do_lower_case=True), "cased": dict(do_lower_case=False),
       "uncased_keep_accents": dict(do_lower_case=True, strip_accents=False)}
SPECIALS = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"]

# script pools: (name, code points, makes multi-character pieces)
POOLS = [
    ("ascii", list(range(0x41, 0x5B)) + list(range(0x61, 0x7B)) + list(range(0x30, 0x3A)), True),
    ("latin", list(range(0xC0, 0x250)), True),
    ("marks", list(range(0x300, 0x370)), False),
    ("greek", list(range(0x386, 0x3CF)), True),
    ("cyrillic", list(range(0x400, 0x482)), True),
    ("hebrew", list(range(0x5B0, 0x5C8)) + list(range(0x5D0, 0x5EB)), True),
    ("arabic", list(range(0x620, 0x653)), True),
    ("devanagari", list(range(0x900, 0x980)), True),
    ("thai", list(range(0xE01, 0xE3B)) + list(range(0xE40, 0xE5C)), True),
    ("kana", list(range(0x3041, 0x3097)) + list(range(0x30A1, 0x30FB)), True),
    ("cjk", list(range(0x4E00, 0x4E00 + 400)) + list(range(0x9F00, 0x9F60)), False),
    ("hangul", list(range(0xAC00, 0xAC00 + 300)) + list(range(0xD700, 0xD7A4)), True),
    ("punct", list(range(0x2010, 0x2028)) + list(range(0x2030, 0x205F)) + list(range(0x3001, 0x3004)) + list(range(0x21, 0x30)), False),
    ("fullwidth", list(range(0xFF01, 0xFF5F)), True),
    ("control", list(range(0x00, 0x20)) + list(range(0x7F, 0xA1)) + [0xAD, 0x200B, 0x200C, 0x200D, 0x200E, 0x2028, 0x2029, 0x202F, 0x2060,
                                                                      0x3000, 0xFEFF, 0xFFFD], False),
    ("emoji", list(range(0x1F600, 0x1F650)) + [0x1F1E9, 0x1F1EA, 0x1D11E, 0x1D15E, 0x1D163, 0x1D165], False),
    ("astral_cjk", list(range(0x20000, 0x20040)) + [0x2A6D6, 0x2F800], False),
    ("single", [ord(c) for c in "İıſßΣςǅǄǆﬁﬂ"] + [0x212A, 0x212B, 0x2126, 0xB5, 0x1E9E, 0x130, 0x149, 0x1F0, 0x390], True),
]


def pool_code_points():
    return sorted({cp for _, cps, _ in POOLS for cp in cps})


@functools.lru_cache(maxsize=None)
def vocab():
    """One vocabulary for the three configurations: the normalised single characters of the pools (under every configuration) as
    whole-word pieces for ~85 % and as ## pieces for ~70 % of them, 600 random 2-5 character pieces per script (each also as ##),
    the five specials.  e / é and their ## forms are always in: the 100-character test needs them to match."""
    from transformers import BertTokenizer
    rng = np.random.default_rng(7)
    stub = {t: i for i, t in enumerate(SPECIALS)}
    norms = [BertTokenizer(vocab=stub, **_KW[k]).backend_tokenizer.normalizer.normalize_str for k in CONFIGS]
    toks, seen = list(SPECIALS), set(SPECIALS)

    def add(p):
        if p not in seen:
            seen.add(p)
            toks.append(p)

    for p in ("e", "##e", "é", "##é"):
        add(p)
    for name, cps, multi in POOLS:
        chars = sorted({d for cp in cps for nm in norms for d in nm(chr(cp)) if not d.isspace()})
        for d in chars:
            if rng.random() < 0.85:
                add(d)
            if rng.random() < 0.70:
                add("##" + d)
        if multi and chars:
            for _ in range(600):
                s = "".join(rng.choice(chars, int(rng.integers(2, 6))))
                add(s)
                add("##" + s)
    return {t: i for i, t in enumerate(toks)}


@functools.lru_cache(maxsize=None)
def build_tokenizer(kind):
    from transformers import BertTokenizer
    return BertTokenizer(vocab=vocab(), **_KW[kind])


def _pieces_by_pool():
    v = [t for t in vocab() if t not in SPECIALS and not t.startswith("##") and len(t) > 1]
    return v


FIXED = [
    "", " ", "a", "Hello, World!  This is GREAT...", "a\tb\nc\rd",
    "é" * 100, "é" * 101, "x " + "é" * 100 + " y " + "é" * 101 + " z",           # the 100-character limit counts characters
    "İ", "İstanbul ısı", "ß ſ ǅ Σ ς \u212a", "ΣΊΣΥΦΟΣ ς",                              # case mappings
    "ﬁ", "ﬁn ﬂow",                                                                     # no compatibility decomposition
    "한", "한국어 텍스트", "\U0001d163", "a\U0001d163b",                                   # NFD expansions (3 jamo; a 12-byte image)
    "".join(chr(0x4E00 + i) for i in range(200)), "\U00020000", "x\U00020000\U00020001y",    # CJK: every character its own word
    "a\u3000b\u00a0c",                                                                  # Unicode spaces
    "a\u200db\u00adc\ufffdd\x00e", "\u200d\u00ad\ufffd\x00",                            # removed characters
    "“a” — b… 、c。", "ＡＢＣ，ｄ！（ｅ）",                                                   # punctuation, full-width forms
    "a\u0323\u0301 a\u0301\u0323 e\u0327\u0301 e\u0301\u0327 o\u0308\u0304\u0301",    # marks in canonical and non-canonical order
    "ok \U0001f600 fine \U0001f1e9\U0001f1ea",                                         # astral emoji
    "e" * 40 + "é" * 30 + " tail",                                                      # truncation inside a multi-piece word
    "café naïve résumé CAFÉ", "Привет, МИР! Ёлка", "中文 mixed with english", "ひらがな カタカナ",
]
# fixed cases that are NOT eligible for the device, by configuration, each with its reason
HOST_ONLY_FIXED = {
    "a\U0001d165b": ("uncased", "U+1D165 survives accent stripping and has combining class 216: NFD may move it"),
}
FIXED += list(HOST_ONLY_FIXED)


def random_texts(n, seed):
    """Words of 1-3 vocabulary pieces or of 1-8 raw pool characters (marks sprinkled in, in random order), from 1-3 pools per
    text, separated by spaces / tabs / punctuation / nothing."""
    rng = np.random.default_rng(seed)
    pieces = _pieces_by_pool()
    marks = POOLS[2][1]
    out = []
    for _ in range(n):
        pools = [POOLS[int(i)] for i in rng.integers(0, len(POOLS), int(rng.integers(1, 4)))]
        ws = []
        for _ in range(int(rng.integers(1, 14))):
            r = rng.random()
            if r < 0.45:
                w = "".join(pieces[int(i)] for i in rng.integers(0, len(pieces), int(rng.integers(1, 4))))
                if rng.random() < 0.3:
                    w = w.upper()
            else:
                cps = pools[int(rng.integers(0, len(pools)))][1]
                w = "".join(chr(cps[int(i)]) for i in rng.integers(0, len(cps), int(rng.integers(1, 9))))
                if rng.random() < 0.3:
                    k = int(rng.integers(0, len(w) + 1))
                    w = w[:k] + "".join(chr(int(c)) for c in rng.choice(marks, int(rng.integers(1, 4)))) + w[k:]
            ws.append(w)
        seps = [" ", " ", " ", "  ", "\t", "\n", ", ", "\u3000", "—", ""]
        out.append("".join(w + seps[int(i)] for w, i in zip(ws, rng.integers(0, len(seps), len(ws)))))
    return out


# the ASCII text set of tests/test_tokenizer_gpu.py (its generator, copied)
WORDS = ("the of and to in is that for it as was with be by on not he this are or his from at which but have an had they "
         "you were their one all we can her has there been if more when will would who so no out up into do any what them "
         "great product works well love much best purchase ever made terrible waste money awful buy broke after day fine "
         "nothing special average okay neither good bad password reset login help support please account payment refund "
         "shipping order tracking number classifier adaptive prototype memory neural network embedding transformer attention "
         "playing played plays player unbelievable internationalization tokenization tokenizer wordpiece").split()


def ascii_vocab(drop=()):
    toks = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"]
    chars = [chr(c) for c in range(33, 127)]
    toks += [c for c in chars if c not in drop and not ("A" <= c <= "Z")]
    toks += ["##" + c for c in chars if ("##" + c) not in drop and (c.isalnum() and not c.isupper())]
    seen = set(toks)
    rng = np.random.default_rng(0)
    for w in WORDS:
        for piece in (w, w[: max(2, len(w) // 2)], "##" + w[len(w) // 2:], "##" + w[-3:], "##ing", "##ed", "##s", "##ly", "##tion"):
            if piece not in seen and len(piece.replace("##", "")) > 0:
                seen.add(piece); toks.append(piece)
    for _ in range(300):
        n = int(rng.integers(2, 7))
        s = "".join(rng.choice(list("abcdefghijklmnopqrstuvwxyz0123456789"), n))
        for piece in (s, "##" + s):
            if piece not in seen:
                seen.add(piece); toks.append(piece)
    return {t: i for i, t in enumerate(toks)}


def ascii_texts():
    rng = np.random.default_rng(1)
    out = ["", "   ", "hello", "Hello, World!  This is GREAT...", "a\tb\nc\rd", "ctrl\x01inside\x7fword \x00 nul",
           "x" * 100 + " " + "y" * 101 + " z", "don't stop-believing (really)!?", "price: $12.50 + 3% = #wow @home",
           "unbelievable internationalization tokenization", "UPPER lower MiXeD 123abc abc123", "q" * 300,
           "trailing space ", " leading", "multiple    spaces\t\ttabs", "[brackets] {braces} <angles> |pipes|",
           "café naïve résumé", "中文 mixed with english", "emoji \U0001f600 here",
           "has a [SEP] literal and a [MASK] too", "long " * 1200]
    for _ in range(60):
        n = int(rng.integers(1, 40))
        ws = []
        for _ in range(n):
            w = str(rng.choice(WORDS))
            r = rng.random()
            if r < 0.15: w = w.upper()
            elif r < 0.3: w = w.capitalize()
            elif r < 0.4: w = w + str(int(rng.integers(0, 1000)))
            elif r < 0.5: w = w + str(rng.choice(list(",.;:!?'\"-()")))
            elif r < 0.55: w = "".join(rng.choice(list("abcdefghijklmnopqrstuvwxyz"), int(rng.integers(1, 15))))
            ws.append(w)
        out.append(str(rng.choice([" ", "  ", "\t", "\n"])).join(ws))
    return out


# malformed UTF-8, one of each form the entries must report as not done
MALFORMED = [b"\xc3", b"\xe4\xb8", b"\xf0\x9f\x98",                                     # truncated 2-, 3-, 4-byte sequences
             b"\x80", b"\xbf", b"\xc3\xa9\xa9",                                         # lone continuation bytes
             b"\xc0\xaf", b"\xc1\xbf", b"\xe0\x80\xaf", b"\xe0\x9f\xbf", b"\xf0\x80\x80\xaf", b"\xf0\x8f\xbf\xbf",   # overlong forms
             b"\xed\xa0\x80", b"\xed\xbf\xbf",                                          # encoded surrogates
             b"\xf4\x90\x80\x80", b"\xf5\x80\x80\x80", b"\xf8\x88\x80\x80\x80", b"\xff", b"\xfe"]          # above U+10FFFF / no lead byte


class HostTables:
    """ac_wordpiece_vocab and ac_wordpiece_unicode over host (numpy) arrays, built by the wrapper's own builders."""

    def __init__(self, hf, unicode_tables=None):
        from adaptive_classifier import tokenizer as tkz
        spec = tkz._wordpiece_spec(hf)
        assert spec is not None
        self.hf = hf
        self.vocab, self.lower, self.specials = spec
        self.arrays, self.slots, self.max_piece = tkz.build_wordpiece_tables(self.vocab)
        self.struct = tkz.wordpiece_vocab_struct(hf, self.vocab, self.lower, [a.ctypes.data for a in self.arrays], self.slots, self.max_piece)
        self.tables = unicode_tables if unicode_tables is not None else tkz.build_wordpiece_unicode_tables(hf)
        self.unicode = tkz.wordpiece_unicode_struct(self.tables)
        self.host_only = tkz._host_only_regex(self.tables)
        self.pad_id = self.vocab[hf.pad_token]

    def eligible(self, text):
        """The wrapper's rule: at most 4096 bytes, no literal special token, no host-only code point."""
        return len(text.encode("utf-8")) <= 4096 and not any(sp in text for sp in self.specials) \
            and not (self.host_only is not None and self.host_only.search(text))


def pack(raws, slack=64):
    """(blob uint8 with `slack` bytes behind the last text, offsets int32 [b + 1]) of byte strings"""
    offs = np.zeros(len(raws) + 1, np.int32)
    offs[1:] = np.cumsum([len(r) for r in raws])
    blob = np.frombuffer(b"".join(raws) + b"\0" * slack, np.uint8).copy()
    if len(blob) == 0:
        blob = np.zeros(1, np.uint8)
    return blob, offs


def raw(texts):
    return [t.encode("utf-8") if isinstance(t, str) else t for t in texts]


def encode_host(ht, texts, max_length, slack=64):
    """ac_wordpiece_encode_utf8_host over str or bytes texts -> (ids int64 [b, max_length], mask, lens); untouched cells hold -7"""
    from adaptive_classifier import _native as nv
    blob, offs = pack(raw(texts), slack)
    b = len(texts)
    ids = np.full((b, max_length), -7, np.int64)
    mask = np.full((b, max_length), -7, np.int64)
    lens = np.full(b, -7, np.int32)
    rc = nv.lib().ac_wordpiece_encode_utf8_host(blob.ctypes.data, offs.ctypes.data, b, ctypes.byref(ht.struct), ctypes.byref(ht.unicode),
                                                max_length, ids.ctypes.data, mask.ctypes.data, lens.ctypes.data)
    assert rc == 0, nv.lib().ac_last_error()
    return ids, mask, lens


def reference(hf, texts, max_length):
    """The wrapped tokenizer called as the classifier calls it, padded to max_length: (ids, mask, lens)"""
    if not texts:
        return np.zeros((0, max_length), np.int64), np.zeros((0, max_length), np.int64), np.zeros(0, np.int64)
    enc = hf(texts, max_length=max_length, truncation=True, padding="max_length", return_tensors="np")
    return enc["input_ids"], enc["attention_mask"], enc["attention_mask"].sum(1)


def table_image(tables, cp):
    """What the table says the normaliser makes of chr(cp): a string, or None for host-only."""
    e = int(tables["entries"][int(tables["page_of"][cp >> 8]), cp & 255])
    kind = e & 7
    if kind == 0:
        return chr(cp)
    if kind == 1:
        return ""
    if kind == 2:
        off, n = e >> 9, (e >> 5) & 15
        return bytes(tables["images"][off:off + n]).decode("utf-8")
    if kind == 4:
        return " " + chr(cp) + " "
    return None


def dump(ht, raws, max_length, path):
    """Tables + texts as one little-endian binary file for a stand-alone C++ program over csrc/wordpiece_core.h:
    int32 [12] slots, vocab blob bytes, max_piece, unk, cls, sep, pad, n_pages, image_bytes, b, text bytes, max_length |
    keys | offs | ids | lens | blob | page_of | entries | images[:image_bytes] | offsets [b + 1] | text (exactly its bytes)"""
    keys, offs, ids, lens, blob = ht.arrays
    t = ht.tables
    text, toffs = pack(raws, 0)
    text = text[:toffs[-1]]
    v = ht.struct
    head = np.array([ht.slots, len(blob), ht.max_piece, v.unk_id, v.cls_id, v.sep_id, v.pad_id, t["n_pages"], t["image_bytes"],
                     len(raws), len(text), max_length], np.int32)
    with open(path, "wb") as f:
        for a in (head, keys, offs, ids, lens, blob, t["page_of"], t["entries"], t["images"][:t["image_bytes"]], toffs, text):
            f.write(np.ascontiguousarray(a).tobytes())
