"""Device tokenizers: the tokenizer call of the hot path on MI355X.

Replace `self.tokenizer(texts, max_length=..., truncation=True, padding=True, return_tensors="pt")`
(/root/reference/src/adaptive_classifier/classifier.py:1259-1265) for the three tokenizer families the encoders cover:

* `HipWordPieceTokenizer` -- BERT-family WordPiece vocabularies (transformers BertTokenizer / DistilBertTokenizer ...:
  tokenizers BertNormalizer + BertPreTokenizer + WordPiece), ids from `ac_wordpiece_encode` (ASCII texts) and, with
  `unicode=True`, from `ac_wordpiece_encode_utf8` (UTF-8 texts: below);
* `HipByteBPETokenizer` -- GPT-2 byte-level BPE (RoBERTa-style and ModernBERT-style tokenizers: tokenizers
  ByteLevel(use_regex=True) + BPE behind RobertaProcessing or a `<cls> $A <sep>` template), ids from `ac_bpe_encode` (ASCII
  texts) and, with `unicode=True`, from `ac_bpe_utf8_encode` (UTF-8 texts: below).
  The vocabulary strings and merge sides are turned back into raw bytes (ByteLevel's byte <-> unicode map inverted), so the
  kernel works on the text's own bytes; `ac_bpe_encode_host` runs the same algorithm on the CPU;
* `HipUnigramTokenizer` -- SentencePiece-style Unigram (DeBERTa-v2/v3 and XLM-R style tokenizers: tokenizers
  Metaspace(prepend_scheme="always") + Unigram behind a `<cls> $A <sep>` template), ids from `ac_unigram_encode`: per
  whitespace-separated word a Viterbi search in fp64 over the pure-ASCII pieces of the vocabulary, the metaspace stored as
  0x20; `ac_unigram_encode_host` runs the same algorithm on the CPU, and recognition ends with a probe list on which it
  must reproduce the wrapped tokenizer (`_unigram_spec`).

Either way the ids are produced on the device and handed to the encoder without a host round trip: host work per batch is
one concatenation of the texts' bytes, one small H2D and one small D2H (the padded length, which the encoder launch needs).
A tokenizer is recognised by its serialised configuration (`_wordpiece_spec`, `_bpe_spec`, `_unigram_spec`), never by a model
name.

Exactness: identical ids / mask to the wrapped transformers tokenizer.  The kernels cover ASCII texts of up to 4096
bytes; texts with non-ASCII bytes (accent stripping / CJK spacing / Unicode categories / NFC live in the host library),
longer texts, texts containing a literal special- or added-token string ("[SEP]", "<s>", ModernBERT's runs of spaces ...)
and texts the BPE / Unigram kernels report as not done (a pre-token / word of more than 64 bytes) are tokenised by the wrapped
tokenizer itself and spliced into the batch -- the reference's own tokenizer, not a re-implementation.  The Unigram wrapper is
narrower still: bytes 0x20-0x7E and \\t \\n \\r only (the other control bytes go through the host's normalizer).

WordPiece on Unicode text (opt-in: `HipWordPieceTokenizer(hf, unicode=True)`, `maybe_device_tokenizer(hf, device, unicode=True)`,
`AdaptiveClassifier(config={"device_tokenizer_unicode": True})`).  BertNormalizer and BertPreTokenizer act code point by code
point, so `build_wordpiece_unicode_tables` turns them into a paged table by probing the wrapped pipeline itself (no Unicode data of
our own) and `ac_wordpiece_encode_utf8` runs decode, table lookup, segmentation and greedy matching on character boundaries on the
device (csrc/wordpiece_core.h; `ac_wordpiece_encode_utf8_host` is the same code on the CPU, and a probe list must reproduce the
wrapped tokenizer on it or the ASCII-only routing stays).  A pure-ASCII batch still takes the ASCII entry.  What still goes to the
wrapped tokenizer: texts with a host-only code point (a surviving combining mark that NFD may reorder; only with accent
stripping), over 4096 bytes or with a literal special token -- decided per text by one compiled regular expression -- and what the
kernel reports as not done (normalised text over 8192 bytes; malformed UTF-8 cannot come out of a str).  It is opt-in because the
default routing of non-ASCII texts is pinned by existing tests.

Unigram on Unicode text (the same opt-in switch: `HipUnigramTokenizer(hf, unicode=True)`).  The whole normalizer chain (Precompiled /
NFC / NFKC / Nmt / Lowercase / Replace / Strip) becomes a paged table by probing the wrapped pipeline (`build_unigram_unicode_tables`:
images inside a carrier; host-only where the chain does not act on the code point alone -- grapheme clusters of Precompiled,
composition under NFC, Strip and runs of Unicode spaces), `build_unigram_tables(spec, utf8=True)` stores every piece as UTF-8 bytes,
and `ac_unigram_encode_utf8` runs decode, table lookup, word splitting and the character-aware Viterbi on the device, long words
in blocks of 64 piece ends (csrc/unigram_core.h, csrc/unigram_utf8.hip; `ac_unigram_encode_utf8_host` is the same code on the CPU,
and a probe list must reproduce the wrapped tokenizer on it or the ASCII-only routing stays).  What still goes to the wrapped
tokenizer: texts with a host-only code point, over 4096 bytes or with a literal special token, and what the kernel reports as
not done (normalised text over 5120 bytes).

Byte-level BPE on Unicode text (the same opt-in switch: `HipByteBPETokenizer(hf, unicode=True)`).  The merges already work on raw
bytes; the only Unicode knowledge of the pipeline is the class of each code point in the pre-tokeniser pattern (whitespace, letter,
number, other), which `build_bpe_unicode_tables` probes from the wrapped pre-tokenizer into a paged one-byte table.
`ac_bpe_utf8_encode` decodes strictly, classifies every character and runs the pattern on characters, then the merge rounds of the
ASCII kernel on the same bytes (csrc/bpe_core.h, csrc/bpe_utf8.hip; `ac_bpe_utf8_encode_host` is the same code on the CPU, and a
probe list must reproduce the wrapped tokenizer on it or the ASCII-only routing stays).  The device does no normalisation: with an
NFC normalizer (ModernBERT style) every code point NFC changes or may combine with a neighbour is host-only, so a device text is
its own NFC.  What still goes to the wrapped tokenizer: texts with a host-only code point, over 4096 bytes or with a literal special
token, and what the kernel reports as not done (a pre-token of more than 64 bytes: an unsegmented CJK or Thai run of more than
about 21 characters).
"""
import ctypes
import json
import re

import numpy as np
import torch

from . import _native as nv

MAX_DEVICE_BYTES = 4096


def _backend_config(tok):
    """The serialised tokenizers pipeline behind a transformers fast tokenizer, or None."""
    be = getattr(tok, "backend_tokenizer", None) or getattr(tok, "_tokenizer", None)
    if be is None:
        return None
    try:
        return json.loads(be.to_str())
    except Exception:
        return None


def _literal_tokens(tok, cfg, need):
    """Strings the host tokenizer cuts out of a text before its model runs: special and added tokens."""
    return sorted((set(str(t) for t in getattr(tok, "all_special_tokens", need)) |
                   set(a["content"] for a in cfg.get("added_tokens") or [])) - {""})


def _wordpiece_spec(tok):
    """(vocab dict, lower_case, specials) if `tok` is a BERT-style WordPiece tokenizer this module reproduces, else None."""
    cfg = _backend_config(tok)
    if cfg is None:
        return None
    model, norm, pre = cfg.get("model") or {}, cfg.get("normalizer") or {}, cfg.get("pre_tokenizer") or {}
    if model.get("type") != "WordPiece" or norm.get("type") != "BertNormalizer" or pre.get("type") != "BertPreTokenizer":
        return None
    if model.get("continuing_subword_prefix", "##") != "##" or int(model.get("max_input_chars_per_word", 100)) != 100:
        return None
    if not norm.get("clean_text", True):
        return None
    post = cfg.get("post_processor") or {}
    if post.get("type") not in ("TemplateProcessing", "BertProcessing"):
        return None
    vocab = model.get("vocab") or {}
    need = [tok.unk_token, tok.cls_token, tok.sep_token, tok.pad_token]
    if any(t is None or t not in vocab for t in need) or model.get("unk_token") != tok.unk_token:
        return None
    return vocab, bool(norm.get("lowercase", True)), _literal_tokens(tok, cfg, need)


def build_wordpiece_tables(vocab):
    """The arrays behind ac_wordpiece_vocab for a WordPiece vocabulary dict, on the host (numpy): (keys uint64 [slots], offs
    uint32 [slots], ids int32 [slots], lens uint16 [slots], blob uint8), slots, max_piece.  Needs no GPU: the slots are filled
    with ac_wordpiece_hash, the function the kernels probe with."""
    L = nv.lib()
    pieces = []
    for tokstr, tid in vocab.items():
        cont = tokstr.startswith("##") and len(tokstr) > 2
        raw = (tokstr[2:] if cont else tokstr).encode("utf-8")
        if len(raw) == 0 or len(raw) > 65535:
            continue
        pieces.append((raw, int(tid), cont))
    slots = 1
    while slots < 2 * len(pieces) + 16:
        slots <<= 1
    keys = np.zeros(slots, np.uint64)
    offs = np.zeros(slots, np.uint32)
    ids = np.zeros(slots, np.int32)
    lens = np.zeros(slots, np.uint16)
    blob = bytearray()
    mask = slots - 1
    max_piece = 1
    for raw, tid, cont in pieces:
        buf = (ctypes.c_uint8 * len(raw)).from_buffer_copy(raw)
        h = int(L.ac_wordpiece_hash(buf, len(raw), 1 if cont else 0))
        s = (h ^ (h >> 32)) & mask
        while keys[s] != 0:
            s = (s + 1) & mask
        keys[s], offs[s], ids[s], lens[s] = h, len(blob), tid | ((1 << 30) if cont else 0), len(raw)
        blob += raw
        max_piece = max(max_piece, len(raw))
    blob += b"\0" * 16
    return (keys, offs, ids, lens, np.frombuffer(bytes(blob), np.uint8).copy()), slots, max_piece


def wordpiece_vocab_struct(hf, vocab, lower, pointers, slots, max_piece):
    """ac_wordpiece_vocab over the five arrays' addresses (device or host), in build_wordpiece_tables order."""
    return nv.ac_wordpiece_vocab(*pointers, slots, max_piece, vocab[hf.unk_token], vocab[hf.cls_token], vocab[hf.sep_token],
                                 vocab[hf.pad_token], 1 if lower else 0)


# ---- BertNormalizer + BertPreTokenizer as a probed table (csrc/wordpiece_core.h) ----------------------------------------------
WP_BUFFER_BYTES = 8192                                            # wpu::kBufBytes: normalised UTF-8 of one text
_WP_PAGES = 0x1100
_WP_IDENTITY, _WP_REMOVED, _WP_IMAGE, _WP_HOST_ONLY, _WP_PADDED = range(5)
_WP_SPACE, _WP_PUNCT, _WP_WORD = 1, 2, 3
_WP_UNICODE_CACHE = {}


def _ranges(cps):
    """Sorted code points -> [(first, last)] of the runs."""
    out = []
    for cp in cps:
        if out and cp == out[-1][1] + 1:
            out[-1][1] = cp
        else:
            out.append([cp, cp])
    return [(a, b) for a, b in out]


def build_wordpiece_unicode_tables(hf_tokenizer):
    """BertNormalizer + BertPreTokenizer of `hf_tokenizer` as the table behind ac_wordpiece_unicode, on the host (numpy); needs
    no GPU.  A dict: page_of uint16 [0x1100], entries uint32 [n_pages, 256], images uint8, n_pages, image_bytes, host_only (the
    flagged code points, sorted), strips_accents, seconds (of the build).

    No Unicode data of our own: a Python `unicodedata` of another Unicode version would silently disagree with the Rust tables.
    The wrapped pipeline itself is probed -- image(cp) = normalizer.normalize_str(chr(cp)) for every code point but the
    surrogates, class(d) = what pre_tokenizer.pre_tokenize_str("a" + d + "b") does to every d that occurs in an image.  The one
    context dependence: with accent stripping the normaliser runs NFD, which sorts combining marks by combining class.  The Mn
    marks vanish afterwards, so only a SURVIVING non-starter can end up somewhere else than its image says; whether a survivor
    is one is probed with the library's own NFD (does it change places with a mark of class 240 in front / of class 1 behind).
    A code point whose image opens with such a survivor is host-only: in a text without one every surviving non-starter
    follows a starter of its own image, where NFD already put it in order.

    The result is cached in-process by the serialised normalizer + pre-tokenizer (the sweep takes over a second)."""
    import time
    from tokenizers import normalizers
    cfg = _backend_config(hf_tokenizer) or {}
    key = json.dumps([cfg.get("normalizer"), cfg.get("pre_tokenizer")], sort_keys=True)
    if key in _WP_UNICODE_CACHE:
        return _WP_UNICODE_CACHE[key]
    t0 = time.perf_counter()
    be = hf_tokenizer.backend_tokenizer
    norm, pre = be.normalizer.normalize_str, be.pre_tokenizer.pre_tokenize_str
    strips = "\u0301" not in norm("e\u0301")
    cps = list(range(0xD800)) + list(range(0xE000, 0x110000))
    chars = list(map(chr, cps))
    imgs = list(map(norm, chars))
    kind = np.zeros(0x110000, np.uint32)
    kind[0xD800:0xE000] = _WP_HOST_ONLY                          # (no UTF-8 text holds one: the decoder rejects them)
    same, gone, other = [], [], {}                               # itself | removed | cp -> image
    for cp, ch, img in zip(cps, chars, imgs):
        if img == ch:
            same.append(cp)
        elif not img:
            gone.append(cp)
        else:
            other[cp] = img
    kind[gone] = _WP_REMOVED
    is_out = np.zeros(0x110000, bool)                            # the code points that occur in normalised text
    is_out[same] = True
    where = {}                                                   # image string -> offset | length << 23
    blob = bytearray()
    for cp, img in other.items():
        if img == " " + chr(cp) + " ":
            kind[cp] = _WP_PADDED
            is_out[cp] = True
            continue
        raw = img.encode("utf-8")
        if len(raw) > 15 or len(blob) + len(raw) >= 1 << 23:     # what an entry cannot hold (nothing known comes near: <= 12 bytes)
            kind[cp] = _WP_HOST_ONLY
            continue
        if img not in where:
            where[img] = len(blob) | (len(raw) << 23)
            blob += raw
            is_out[[ord(d) for d in img]] = True
        w = where[img]
        kind[cp] = _WP_IMAGE | ((w >> 23) << 5) | ((w & ((1 << 23) - 1)) << 9)
    is_out[0x20] = True
    # Classes of the output code points, and (accent stripping) which of them are non-starters.  Both properties are per code
    # point, so a page of 256 is first asked as one string -- "a" + page + "b" stays one piece iff every code point of it is a
    # word character; marks of class 240 / 1 around every code point stay where they are iff every one is a starter -- and
    # only a page that fails is asked code point by code point (most pages are CJK, Hangul, unassigned: they pass).
    cls = np.zeros(0x110000, np.uint8)
    odd = set()                                                  # outputs without a clean class, or non-starters
    nfd = normalizers.NFD().normalize_str
    hi, lo = "\u0345", "\u0334"                                  # combining classes 240 and 1
    for page in range(_WP_PAGES):
        at = np.flatnonzero(is_out[page * 256:(page + 1) * 256]) + page * 256
        if not len(at):
            continue
        ds = list(map(chr, at.tolist()))
        run = "".join(ds)
        if [p for p, _ in pre("a" + run + "b")] == ["a" + run + "b"]:
            cls[at] = _WP_WORD
        else:
            for d in ds:
                got = [p for p, _ in pre("a" + d + "b")]
                cls[ord(d)] = _WP_SPACE if got == ["a", "b"] else _WP_PUNCT if got == ["a", d, "b"] else \
                    _WP_WORD if got == ["a" + d + "b"] else 0
                if cls[ord(d)] == 0:
                    odd.add(d)
        if strips:
            marked = "".join(hi + d + lo for d in ds)
            if nfd(marked) != marked:
                odd |= {d for d in ds if nfd(hi + d) != hi + nfd(d) or nfd(d + lo) != nfd(d) + lo}
    kind |= cls.astype(np.uint32) << 3
    # host-only: a code point that is such an output itself, or whose image opens with one / holds one without a class
    for d in odd:
        if (kind[ord(d)] & 7) == _WP_IDENTITY:
            kind[ord(d)] |= _WP_HOST_ONLY
    if odd:
        for cp, img in other.items():
            first = img[1] if (kind[cp] & 7) == _WP_PADDED else img[0]
            if first in odd or any(cls[ord(d)] == 0 for d in img):
                kind[cp] = (kind[cp] & np.uint32(0x18)) | _WP_HOST_ONLY
    pages, page_of = np.unique(kind.reshape(_WP_PAGES, 256), axis=0, return_inverse=True)
    images = np.frombuffer(bytes(blob) + b"\0" * 16, np.uint8).copy()
    host_only = np.flatnonzero((kind & 7) == _WP_HOST_ONLY)
    host_only = [int(c) for c in host_only if not 0xD800 <= c < 0xE000]
    tables = {"page_of": page_of.reshape(-1).astype(np.uint16), "entries": np.ascontiguousarray(pages, np.uint32), "images": images,
              "n_pages": int(len(pages)), "image_bytes": int(len(blob)), "host_only": host_only, "strips_accents": bool(strips),
              "seconds": time.perf_counter() - t0}
    _WP_UNICODE_CACHE[key] = tables
    return tables


def wordpiece_unicode_struct(tables, pointers=None):
    """ac_wordpiece_unicode over the three arrays' addresses (device), or over the host arrays themselves."""
    if pointers is None:
        pointers = [tables[k].ctypes.data for k in ("page_of", "entries", "images")]
    return nv.ac_wordpiece_unicode(*pointers, tables["n_pages"], tables["image_bytes"])


def _host_only_regex(tables):
    """One compiled character class of the host-only code points (None if there is none): eligibility in one C-speed pass."""
    import re
    if not tables["host_only"]:
        return None
    return re.compile("[" + "".join(re.escape(chr(a)) if a == b else re.escape(chr(a)) + "-" + re.escape(chr(b))
                                    for a, b in _ranges(tables["host_only"])) + "]")


def _wordpiece_unicode_probes():
    """The fixed probe list of the guard: multi-character strings over what the table encodes -- decompositions, case mappings
    of one and two code points, CJK spacing, Unicode spaces and punctuation, removed characters, marks in both orders, astral
    code points, scripts without case -- each also inside a longer text."""
    base = ["", "a", "Hello, World!", "a\tb\nc\rd", "ctrl\x01in\x7fword \x00 nul",
            "café naïve résumé", "CAFÉ NAÏVE RÉSUMÉ", "Ångström Œuvre Ærø Ðið Þú ǅemal", "İstanbul ısı ſtraße Maß",
            "ΣΊΣΥΦΟΣ σίσυφος ς", "\u212a \u212b \u2126 \u00b5", "ﬁn ﬂow ǆ", "한국어 텍스트 각", "\U0001d163 \U0001d15e",
            "中文 mixed 文本 with 日本語のテキスト", "\U00020000\U0002a6d6 x\U00020000y", "a\u3000b\u00a0c\u2003d\u2028e\u0085f",
            "zero\u200dwidth soft\u00adhyphen re\ufffdplaced \ufeffbom", "\u200d\u00ad\ufffd",
            "“quoted” — dash… 、。「」 ！？（）", "full ｗｉｄｔｈ ＡＢＣ １２３",
            "e\u0327\u0301 e\u0301\u0327 a\u0323\u0302 a\u0302\u0323",              # marks in canonical and in reversed order
            "ệ Ệ ǖ Ǖ ṩ", "emoji \U0001f600 \U0001f1e9\U0001f1ea here", "Привет, МИР! Ёлка й",
            "שָׁלוֹם עולם", "مَرْحَبًا بالعالم",
            "हिन्दी भाषा क़", "ภาษาไทย สวัสดี",
            "ひらがな カタカナ ｶﾞ が", "¿Qué? ¡Sí! §1 ©2 ª º «x» ±½ µ ¶ · × ÷", "x" * 30 + "é" * 80,
            "€100 £5 ¥7 ₹9 №3 ™ ℃ Ⅳ ⅷ ① ㈱"]
    return base + [" ".join(base[i:i + 3]) for i in range(5, len(base) - 2, 3)]


def _wordpiece_unicode_matches(hf, specials, vocab_struct, tables, probes):
    """Does ac_wordpiece_encode_utf8_host (host tables) give the wrapped tokenizer's ids, mask and lengths on these probes, and
    report as not done exactly those that hold a host-only code point?"""
    M = _PROBE_MAX_LENGTH
    probes = [t for t in probes if not any(sp in t for sp in specials)]
    flagged = _host_only_regex(tables)
    raws = [t.encode("utf-8") for t in probes]
    offs = np.zeros(len(raws) + 1, np.int32)
    offs[1:] = np.cumsum([len(r) for r in raws])
    blob = np.frombuffer(b"".join(raws) + b"\0" * 64, np.uint8).copy()
    ids = np.zeros((len(raws), M), np.int64)
    mask = np.zeros((len(raws), M), np.int64)
    lens = np.zeros(len(raws), np.int32)
    uni = wordpiece_unicode_struct(tables)
    nv.check(nv.lib().ac_wordpiece_encode_utf8_host(blob.ctypes.data, offs.ctypes.data, len(raws), ctypes.byref(vocab_struct),
                                                    ctypes.byref(uni), M, ids.ctypes.data, mask.ctypes.data, lens.ctypes.data),
             "ac_wordpiece_encode_utf8_host")
    want = hf(probes, max_length=M, truncation=True, padding="max_length", return_tensors="np")
    for i, t in enumerate(probes):
        if flagged is not None and flagged.search(t):
            if lens[i] != -1:
                return False
        elif lens[i] < 0 or not np.array_equal(want["input_ids"][i], ids[i]) or not np.array_equal(want["attention_mask"][i], mask[i]):
            return False
    return True


def wordpiece_unicode_tables(hf, specials, vocab_struct):
    """build_wordpiece_unicode_tables(hf) behind its probe guard: the tables if the host entry over them (and the host
    vocabulary table behind `vocab_struct`) reproduces the wrapped tokenizer on the probe list, else None -- the tokenizer
    then keeps its ASCII-only routing."""
    try:
        tables = build_wordpiece_unicode_tables(hf)
        return tables if _wordpiece_unicode_matches(hf, specials, vocab_struct, tables, _wordpiece_unicode_probes()) else None
    except Exception:
        return None


def _byte_to_unicode():
    """ByteLevel's byte -> printable character map (GPT-2 bytes_to_unicode)."""
    keep = list(range(33, 127)) + list(range(161, 173)) + list(range(174, 256))
    out, extra = {}, 0
    for b in range(256):
        if b in keep:
            out[b] = chr(b)
        else:
            out[b] = chr(256 + extra)
            extra += 1
    return out


def _template_ends(post):
    """(first id, last id) of a post-processor that wraps a single sequence as <one special> $A <one special>, else None."""
    if post.get("type") == "RobertaProcessing":
        try:
            return int(post["cls"][1]), int(post["sep"][1])
        except Exception:
            return None
    if post.get("type") != "TemplateProcessing":
        return None
    single, table = post.get("single") or [], post.get("special_tokens") or {}
    if len(single) != 3 or (single[1].get("Sequence") or {}) != {"id": "A", "type_id": 0}:
        return None
    ends = []
    for piece in (single[0], single[2]):
        sp = piece.get("SpecialToken") or {}
        ids = (table.get(sp.get("id")) or {}).get("ids") or []
        if sp.get("type_id") != 0 or len(ids) != 1:
            return None
        ends.append(int(ids[0]))
    return tuple(ends)


def _bpe_spec(tok):
    """What HipByteBPETokenizer needs, as a dict, if `tok` is a GPT-2 byte-level BPE tokenizer this module reproduces
    (RoBERTa-style / ModernBERT-style), else None:
    vocab, merges [(left, right)] in rank order, add_prefix_space, cls_id, sep_id, pad_id, specials, token_type_ids."""
    cfg = _backend_config(tok)
    if cfg is None:
        return None
    model, norm, pre = cfg.get("model") or {}, cfg.get("normalizer"), cfg.get("pre_tokenizer") or {}
    if model.get("type") != "BPE" or model.get("dropout") or model.get("byte_fallback") or model.get("ignore_merges") \
            or model.get("continuing_subword_prefix") or model.get("end_of_word_suffix") or model.get("fuse_unk"):
        return None
    if norm is not None:                                     # NFC is the identity on ASCII; anything else is not reproduced
        if norm.get("type") == "Sequence" and len(norm.get("normalizers") or []) == 1:
            norm = norm["normalizers"][0]
        if norm.get("type") != "NFC":
            return None
    if pre.get("type") != "ByteLevel" or not pre.get("use_regex", True):
        return None
    ends = _template_ends(cfg.get("post_processor") or {})
    if ends is None:
        return None
    if getattr(tok, "padding_side", "right") != "right" or getattr(tok, "truncation_side", "right") != "right":
        return None
    vocab = model.get("vocab") or {}
    added = {a["content"]: int(a["id"]) for a in cfg.get("added_tokens") or []}
    pad = getattr(tok, "pad_token", None)
    if pad is None or (pad not in vocab and pad not in added):
        return None
    b2u = _byte_to_unicode()
    if any(ch not in vocab for ch in b2u.values()):
        return None
    merges = [tuple(m.split(" ")) if isinstance(m, str) else tuple(m) for m in model.get("merges") or []]
    if any(len(m) != 2 for m in merges):
        return None
    return {"vocab": vocab, "merges": merges, "add_prefix_space": bool(pre.get("add_prefix_space", True)),
            "cls_id": ends[0], "sep_id": ends[1], "pad_id": int(vocab[pad] if pad in vocab else added[pad]),
            "specials": _literal_tokens(tok, cfg, [pad]),
            "token_type_ids": "token_type_ids" in (getattr(tok, "model_input_names", None) or [])}


def build_bpe_tables(spec):
    """The arrays behind ac_bpe_vocab for a `_bpe_spec` result, on the host (numpy): keys uint64 [slots], entries int32
    [slots, 4] (rank, joined id, blob offset, left_len | total_len << 16), blob uint8, byte_id int32 [256].  Needs no GPU:
    the slots are filled with ac_bpe_pair_hash, the function the kernel probes with."""
    L = nv.lib()
    vocab = spec["vocab"]
    u2b = {u: b for b, u in _byte_to_unicode().items()}

    def raw(s):
        return bytes(u2b[ch] for ch in s)

    byte_id = np.zeros(256, np.int32)
    for u, b in u2b.items():
        byte_id[b] = vocab[u]
    pairs = {}                                               # (left bytes, right bytes) -> (rank, id); a repeated pair keeps its last rank
    for rank, (left, right) in enumerate(spec["merges"]):
        if left + right not in vocab or any(ch not in u2b for ch in left + right) or len(left + right) > 0xffff:
            raise nv.NativeError("byte-level BPE: merge %r %r does not name a vocabulary entry over the byte alphabet" % (left, right))
        pairs[(raw(left), raw(right))] = (rank, int(vocab[left + right]))
    slots = 2
    while slots < 2 * len(pairs) + 16:
        slots <<= 1
    keys = np.zeros(slots, np.uint64)
    entries = np.zeros((slots, 4), np.int32)
    blob = bytearray()
    mask = slots - 1
    for (lb, rb), (rank, tid) in pairs.items():
        h = int(L.ac_bpe_pair_hash((ctypes.c_uint8 * len(lb)).from_buffer_copy(lb), len(lb),
                                   (ctypes.c_uint8 * len(rb)).from_buffer_copy(rb), len(rb)))
        s = (h ^ (h >> 32)) & mask
        while keys[s] != 0:
            s = (s + 1) & mask
        keys[s] = h
        entries[s] = (rank, tid, len(blob), len(lb) | ((len(lb) + len(rb)) << 16))
        blob += lb + rb
    blob += b"\0" * 16
    return keys, entries, np.frombuffer(bytes(blob), np.uint8).copy(), byte_id, slots


def bpe_vocab_struct(spec, pointers, slots):
    """ac_bpe_vocab over the four arrays' addresses (device or host), in build_bpe_tables order."""
    return nv.ac_bpe_vocab(*pointers, slots, spec["cls_id"], spec["sep_id"], spec["pad_id"], 1 if spec["add_prefix_space"] else 0)


# ---- the classes of the GPT-2 pre-tokeniser pattern as a probed table (csrc/bpe_core.h) ---------------------------------------
_BPE_WS, _BPE_LETTER, _BPE_DIGIT, _BPE_OTHER, _BPE_HOST_ONLY = 0, 1, 2, 3, 4      # bpe::kWs ... bpe::kHostOnly
_BPE_UNICODE_CACHE = {}


def _joins_carrier(pre, carrier, chars):
    """For every character of `chars`: does the pre-tokenizer keep it in one piece with a `carrier` in front?  One call for the
    whole list: the probes stand back to back (carrier, character, carrier, character ...) and the piece offsets (in characters
    of the probe string) say where the pipeline cut.  Whether it cuts between a carrier and the character behind it depends on
    those two alone; that this is so for the whole list is checked on each end of it by asking those probes alone again."""
    cuts = {start for _, (start, _) in pre("".join(carrier + ch for ch in chars))}
    got = [2 * i + 1 not in cuts for i in range(len(chars))]
    for i in (0, len(chars) - 1):
        if (len(pre(carrier + chars[i])) == 1) != got[i]:
            return [len(pre(carrier + ch)) == 1 for ch in chars]
    return got


def build_bpe_unicode_tables(hf_tokenizer):
    """The pre-tokeniser classes of a byte-level BPE tokenizer as the table behind ac_bpe_unicode, on the host (numpy); needs no
    GPU.  A dict: page_of uint16 [0x1100], entries uint8 [n_pages, 256], n_pages, host_only (the flagged code points, sorted),
    reasons (counts per probe), whitespace (the code points of class \\s, sorted), seconds (of the build).  An entry: bits 0-1
    whitespace | letter | number | other, bit 2 host-only.

    No Unicode data of our own: a Python `unicodedata` of another Unicode version would silently disagree with the library's
    tables.  The only Unicode knowledge of the pipeline is the class of a code point d in the pattern, and the wrapped
    pre-tokenizer itself shows it: d is a letter iff pre_tokenize_str("a" + d) stays one piece, a number iff "1" + d does, other
    iff "!" + d does, and whitespace iff none does.  The probes of a page go in one call per carrier (`_joins_carrier`).
    With an NFC normalizer the device does no normalisation: a text either is its own NFC or goes to the host.  Host-only are
    * every code point whose normalize_str image differs from itself,
    * every code point in a non-first position of the library's NFD of some code point (it may compose with what stands in
      front), every non-starter (it changes places with U+0345 in front or U+0334 behind under the library's NFD) and every code
      point whose decomposition opens with one of those,
    * the surrogates (no UTF-8 text holds one: the decoder rejects them).
    In a text without any of them every code point is NFC-stable and no neighbours interact, so the text is its own NFC.
    The result is cached in-process by the serialised normalizer + pre-tokenizer (the sweep takes a few seconds)."""
    import time
    from tokenizers import normalizers
    cfg = _backend_config(hf_tokenizer) or {}
    key = json.dumps([cfg.get("normalizer"), cfg.get("pre_tokenizer")], sort_keys=True)
    if key in _BPE_UNICODE_CACHE:
        return _BPE_UNICODE_CACHE[key]
    t0 = time.perf_counter()
    be = hf_tokenizer.backend_tokenizer
    pre = be.pre_tokenizer.pre_tokenize_str
    kind = np.full(0x110000, _BPE_OTHER, np.uint8)
    for page in range(0x1100):
        cps = [cp for cp in range(page * 256, page * 256 + 256) if not 0xD800 <= cp < 0xE000]
        if not cps:
            continue
        chars = list(map(chr, cps))
        # most pages are of one class (CJK, Hangul: letters; unassigned, private use, symbols: other): the whole page behind one
        # carrier stays one piece iff every code point of it joins that carrier
        run = "".join(chars)
        if len(pre("a" + run)) == 1:
            kind[cps] = _BPE_LETTER
            continue
        if len(pre("!" + run)) == 1:
            continue
        letter, digit, other = (_joins_carrier(pre, carrier, chars) for carrier in "a1!")
        for cp, l, d, o in zip(cps, letter, digit, other):
            if l + d + o > 1:
                raise nv.NativeError("build_bpe_unicode_tables: U+%04X joins more than one class of the pre-tokenizer" % cp)
            kind[cp] = _BPE_LETTER if l else _BPE_DIGIT if d else _BPE_OTHER if o else _BPE_WS
    host = np.zeros(0x110000, bool)
    host[0xD800:0xE000] = True
    reasons = {}

    def flag(which, why):
        which = [c for c in which if not host[c]]
        host[which] = True
        reasons[why] = reasons.get(why, 0) + len(which)

    if be.normalizer is not None:
        norm = be.normalizer.normalize_str
        cps = list(range(0xD800)) + list(range(0xE000, 0x110000))
        chars = list(map(chr, cps))
        flag([cp for cp, ch in zip(cps, chars) if norm(ch) != ch], "image")
        # composition seconds and non-starters, by the library's own NFD (as build_unigram_unicode_tables finds them)
        nfd = normalizers.NFD().normalize_str
        decs = list(map(nfd, chars))
        seconds = {ord(d) for dec in decs if len(dec) > 1 for d in dec[1:]}
        hi, lo = "\u0345", "\u0334"                              # combining classes 240 and 1
        nonstart = set()
        for page in range(0x1100):
            ds = [ch for ch in map(chr, range(page * 256, page * 256 + 256)) if not 0xD800 <= ord(ch) < 0xE000]
            ds = [d for d in ds if nfd(d) == d]
            marked = "".join(hi + d + lo for d in ds)
            if nfd(marked) != marked:
                nonstart |= {ord(d) for d in ds if nfd(hi + d) != hi + d or nfd(d + lo) != d + lo}
        flag(sorted(seconds), "composes")
        flag(sorted(nonstart), "non-starter")
        flag([cp for cp, dec in zip(cps, decs) if dec and (ord(dec[0]) in nonstart or ord(dec[0]) in seconds)], "decomposes to one")
    whitespace = [int(c) for c in np.flatnonzero(kind == _BPE_WS) if not 0xD800 <= c < 0xE000]
    kind[host] |= _BPE_HOST_ONLY
    pages, page_of = np.unique(kind.reshape(0x1100, 256), axis=0, return_inverse=True)
    host_only = [int(c) for c in np.flatnonzero(host) if not 0xD800 <= c < 0xE000]
    tables = {"page_of": page_of.reshape(-1).astype(np.uint16), "entries": np.ascontiguousarray(pages, np.uint8),
              "n_pages": int(len(pages)), "host_only": host_only, "reasons": reasons, "whitespace": whitespace,
              "seconds": time.perf_counter() - t0}
    _BPE_UNICODE_CACHE[key] = tables
    return tables


def bpe_unicode_struct(tables, pointers=None):
    """ac_bpe_unicode over the two arrays' addresses (device), or over the host arrays themselves."""
    if pointers is None:
        pointers = [tables[k].ctypes.data for k in ("page_of", "entries")]
    return nv.ac_bpe_unicode(*pointers, tables["n_pages"])


def _bpe_unicode_probes():
    """The fixed probe list of the guard: typographic punctuation, accents, Cyrillic, Greek, CJK, kana, Hangul, emoji, Unicode
    whitespace of each kind (leading, trailing, doubled, next to 0x20), numbers of several scripts, contractions next to
    non-ASCII letters -- and strings that must defer where the table flags them (combining sequences, jamo)."""
    base = ["", "a", "Hello, World!", "it\u2019s \u201cquoted\u201d \u2014 dash\u2026 en\u2013dash", "caf\u00e9 na\u00efve r\u00e9sum\u00e9",
            "CAF\u00c9 NA\u00cfVE", "\u00e9's 's\u00e9 \u4e2d's x\u2019s x'r\u00e9 x're\u00e9 we\u2019ll we'll\u00e9",
            "\u00c5ngstr\u00f6m \u0152uvre Stra\u00dfe \u0130stanbul", "\u041f\u0440\u0438\u0432\u0435\u0442, \u041c\u0418\u0420! \u0401\u043b\u043a\u0430",
            "\u03a3\u038a\u03a3\u03a5\u03a6\u039f\u03a3 \u03c3\u03af\u03c3\u03c5\u03c6\u03bf\u03c2", "\u4e2d\u6587 mixed \u6587\u672c with \u65e5\u672c\u8a9e",
            "\u3072\u3089\u304c\u306a \u30ab\u30bf\u30ab\u30ca", "\ud55c\uad6d\uc5b4 \ud14d\uc2a4\ud2b8",
            "emoji \U0001f600 \U0001f1e9\U0001f1ea here \U0001f44d\U0001f3fd",
            "a\u3000b\u00a0c\u2003d\u2028e\u0085f\u1680g\u202fh\u205fi", "\u00a0lead", "trail\u3000", "a\u00a0\u00a0b", "a \u2003 b", "\u3000\u3000",
            "a\u00a0 b", "a \u00a0b", "\u2028", "a \u2029", "\u00a0's \u00a0\u00a0 's", "zero\u200bwidth soft\u00adhyphen \ufeffbom",
            "12\u00b2 \u0661\u0662\u06634 \u2167 \u2460 \u00bd x\u00b2y 3\u00e9", "\u20ac100 \u00a35 \u00a57 \u2122 \u2103 \u00a9 \u00ab x \u00bb \u00bfQu\u00e9?",
            "\U00020000\U0002a6d6 x\U00020000y", "\u0e20\u0e32\u0e29\u0e32 \u0939\u093f\u0928\u094d\u0926\u0940", "full \uff57\uff49\uff44\uff54\uff48 \uff11\uff12\uff13",
            "e\u0301 combining", "A\u0301\u0323", "\u212b \u2126", "\u1100\u1161 jamo", "\uac00\u11a8"]
    return base + [" ".join(base[i:i + 3]) for i in range(3, 30, 3)]


def _bpe_unicode_matches(hf, spec, vocab_struct, tables, probes):
    """Does ac_bpe_utf8_encode_host (host tables) give the wrapped tokenizer's ids, mask and lengths on these probes, and report
    as not done exactly those that hold a host-only code point?  A probe that fills max_length counts as a mismatch."""
    M = _PROBE_MAX_LENGTH
    probes = [t for t in probes if not any(sp in t for sp in spec["specials"])]
    flagged = _host_only_regex(tables)
    raws = [t.encode("utf-8") for t in probes]
    offs = np.zeros(len(raws) + 1, np.int32)
    offs[1:] = np.cumsum([len(r) for r in raws])
    blob = np.frombuffer(b"".join(raws) + b"\0" * 64, np.uint8).copy()
    ids = np.zeros((len(raws), M), np.int64)
    mask = np.zeros((len(raws), M), np.int64)
    lens = np.zeros(len(raws), np.int32)
    uni = bpe_unicode_struct(tables)
    nv.check(nv.lib().ac_bpe_utf8_encode_host(blob.ctypes.data, offs.ctypes.data, len(raws), ctypes.byref(vocab_struct), ctypes.byref(uni),
                                              M, ids.ctypes.data, mask.ctypes.data, lens.ctypes.data), "ac_bpe_utf8_encode_host")
    want = hf(probes, max_length=M, truncation=True, padding="max_length", return_tensors="np")
    for i, t in enumerate(probes):
        if flagged is not None and flagged.search(t):
            if lens[i] != -1:
                return False
        elif lens[i] < 0 or lens[i] >= M or not np.array_equal(want["input_ids"][i], ids[i]) \
                or not np.array_equal(want["attention_mask"][i], mask[i]):
            return False
    return True


def bpe_unicode_tables(hf, spec, vocab_struct):
    """build_bpe_unicode_tables(hf) behind its probe guard: the tables if the host entry over them (and the host merge table
    behind `vocab_struct`) reproduces the wrapped tokenizer on the probe list, else None -- the tokenizer then keeps its
    ASCII-only routing."""
    try:
        tables = build_bpe_unicode_tables(hf)
        return tables if _bpe_unicode_matches(hf, spec, vocab_struct, tables, _bpe_unicode_probes()) else None
    except Exception:
        return None


# ---- SentencePiece-style Unigram (DeBERTa-v2/v3, XLM-R) ---------------------------------------------------------------------
METASPACE = "▁"
_UNIGRAM_NORMALIZERS = {"Lowercase", "NFC", "NFKC", "Nmt", "Strip", "Precompiled", "Replace"}
_UNIGRAM_REPLACES = {" {2,}", "\\s{2,}|[\\n\\r\\t]"}            # runs of whitespace -> one space: what word splitting does anyway
_WORD_BYTES = bytes(range(0x20, 0x7f))
_POLY_BASE, _MIX_MUL = 0x9e3779b97f4a7c15, 0xbf58476d1ce4e5b9    # csrc/unigram_core.h
_DENSE_PIECE_BYTES = 64                                           # build_unigram_tables: pieces up to here are hashed as one matrix
_UNMATCHABLE = re.compile("[\x00-\x20\x7f" + METASPACE + "]")   # in a piece (behind its leading metaspace): it matches no word


def _unigram_structure(tok):
    """The structural half of _unigram_spec: the dict without `ws_controls`, from the serialised configuration alone."""
    cfg = _backend_config(tok)
    if cfg is None:
        return None
    model, norm, pre = cfg.get("model") or {}, cfg.get("normalizer"), cfg.get("pre_tokenizer") or {}
    if model.get("type") != "Unigram" or model.get("byte_fallback") or model.get("unk_id") is None:
        return None
    vocab = model.get("vocab") or []
    unk_id = int(model["unk_id"])
    if not 0 <= unk_id < len(vocab) or len(set(p for p, _ in vocab)) != len(vocab):
        return None
    lowercase = right_strip = collapses = False
    if norm is not None:
        for nm in (norm.get("normalizers") or []) if norm.get("type") == "Sequence" else [norm]:
            kind = nm.get("type")
            if kind not in _UNIGRAM_NORMALIZERS:
                return None
            if kind == "Replace" and ((nm.get("pattern") or {}).get("Regex") not in _UNIGRAM_REPLACES or nm.get("content") != " "):
                return None
            collapses |= kind == "Replace"
            lowercase |= kind == "Lowercase"
            right_strip |= kind == "Strip" and bool(nm.get("strip_right"))
    steps = pre.get("pretokenizers") or [] if pre.get("type") == "Sequence" else [pre]
    kinds = [st.get("type") for st in steps]
    if kinds not in (["Metaspace"], ["WhitespaceSplit", "Metaspace"]):
        return None
    if kinds == ["Metaspace"] and not collapses:            # every space of a run would become a piece of its own
        return None
    meta = steps[-1]
    if meta.get("replacement") != METASPACE or meta.get("prepend_scheme") != "always" or not meta.get("split", True):
        return None
    ends = _template_ends(cfg.get("post_processor") or {})
    if ends is None:
        return None
    if getattr(tok, "padding_side", "right") != "right" or getattr(tok, "truncation_side", "right") != "right":
        return None
    added = {a["content"]: int(a["id"]) for a in cfg.get("added_tokens") or []}
    pieces = {p: i for i, (p, _) in enumerate(vocab)}
    pad = getattr(tok, "pad_token", None)
    if pad is None or (pad not in pieces and pad not in added):
        return None
    return {"vocab": vocab, "unk_id": unk_id, "cls_id": ends[0], "sep_id": ends[1],
            "pad_id": int(added[pad] if pad in added else pieces[pad]), "lowercase": bool(lowercase),
            "trailing_space_piece": kinds == ["Metaspace"] and not right_strip, "specials": _literal_tokens(tok, cfg, [pad]),
            "token_type_ids": "token_type_ids" in (getattr(tok, "model_input_names", None) or [])}


_PROBE_MAX_LENGTH = 128       # no probe comes near it (at most 16 short words or 70 bytes each): nothing is compared truncated


def _unigram_probes():
    """The fixed probe list of the guard: (plain probes, probes with \t \n \r).  Every printable ASCII character stands alone
    as a word, inside a word (w?w), in front of a letter (?a) and behind one (a?), 16 words per probe, and in runs of 24
    characters without a space."""
    printable = [chr(c) for c in range(0x21, 0x7f)]
    plain = ["", " ", "  ", "   ", "a", " a", "a ", "  a", "a  ", " a ", "a b", "a  b", "a   b  c", "Hello World", "HELLO world",
             "MiXeD CaSe", "``quoted''", "`` a ''", "''", "``", "it's don't", "3.14 1,000 #1", "x" * 70, "the quick brown fox jumps",
             "a, b; c: d. e! f?", "(a) [b] {c} <d>", "e-mail under_score", "a/b\\c|d", "100% $5 &co @home ^up ~so *x +y =z",
             "  lead  and  trail  "]
    for lo in range(0, len(printable), 16):
        chunk = printable[lo:lo + 16]
        plain += [" ".join(chunk), " ".join("w" + ch + "w" for ch in chunk), " ".join(ch + "a" for ch in chunk),
                  " ".join("a" + ch for ch in chunk)]
    plain += ["".join(printable[lo:lo + 24]) for lo in range(0, len(printable), 24)]
    controls = ["\t", "\n", "\r", "a\tb", "a\nb", "a\rb", "\ta", "a\t", "\na", "a\n", "\ra", "a\r", "a\t\tb", "a\n\nb", "a \t b",
                "a\t \nb", " \n ", "\r\n", "a\r\nb", "tail\n\n", "\n\n lead", "a \n", "a\n "]
    return plain, controls


def _unigram_matches(tok, spec, tables, probes):
    """Does ac_unigram_encode_host (host tables) give the wrapped tokenizer's ids, mask and lengths on these probes?  A probe
    that fills max_length on either side counts as a mismatch: its tail would have gone uncompared."""
    M = _PROBE_MAX_LENGTH
    arrays, slots = tables
    vocab = unigram_vocab_struct(spec, [a.ctypes.data for a in arrays], slots)
    raws = [t.encode("ascii") for t in probes]
    offs = np.zeros(len(raws) + 1, np.int32)
    offs[1:] = np.cumsum([len(r) for r in raws])
    blob = np.frombuffer(b"".join(raws) + b"\0" * 64, np.uint8).copy()
    ids = np.zeros((len(raws), M), np.int64)
    mask = np.zeros((len(raws), M), np.int64)
    lens = np.zeros(len(raws), np.int32)
    nv.check(nv.lib().ac_unigram_encode_host(blob.ctypes.data, offs.ctypes.data, len(raws), ctypes.byref(vocab), M, ids.ctypes.data,
                                             mask.ctypes.data, lens.ctypes.data), "ac_unigram_encode_host")
    want = tok(probes, max_length=M, truncation=True, padding="max_length", return_tensors="np")
    if int(lens.max(initial=0)) >= M or int(want["attention_mask"].sum(1).max(initial=0)) >= M:
        return False
    return np.array_equal(want["input_ids"], ids) and np.array_equal(want["attention_mask"], mask)


def _unigram_spec(tok, structure=None):
    """What HipUnigramTokenizer needs, as a dict, if `tok` is a Metaspace(always) + Unigram tokenizer this module reproduces
    (DeBERTa-v2/v3 style, XLM-R style), else None: vocab [(piece, score)], unk_id, cls_id, sep_id, pad_id, lowercase,
    trailing_space_piece, ws_controls, specials, token_type_ids.
    The serialised form varies across library versions, so the structural reading is never trusted blind: the host entry
    (ac_unigram_encode_host over host tables; no GPU) must reproduce the wrapped tokenizer on a fixed list of short probes,
    none compared truncated -- every printable ASCII character alone and inside a word, whitespace of each kind leading / trailing / doubled / mixed, both
    cases, `` and '', the empty string.  ws_controls is set only if the \t \n \r probes match as well (otherwise texts with
    those bytes go to the host); any other mismatch gives None.
    `structure`: an `_unigram_structure(tok)` result the caller already has.  The host tables the probes ran on stay in
    spec["tables"] (build_unigram_tables' result: ws_controls changes the struct, not the arrays) for the wrapper to upload."""
    spec = structure if structure is not None else _unigram_structure(tok)
    if spec is None:
        return None
    try:
        plain, controls = _unigram_probes()
        keep = lambda ps: [t for t in ps if not any(sp in t for sp in spec["specials"])]      # noqa: E731
        spec["tables"] = build_unigram_tables(spec)
        spec["ws_controls"] = False
        if not _unigram_matches(tok, spec, spec["tables"], keep(plain)):
            return None
        spec["ws_controls"] = True
        spec["ws_controls"] = bool(_unigram_matches(tok, spec, spec["tables"], keep(controls)))
    except Exception:
        return None
    return spec


def _unigram_hash_rows(mat, lens):
    """ac_unigram_hash of every row of a [n, width] uint8 matrix (row i holds lens[i] bytes), vectorised."""
    h = np.zeros(len(lens), np.uint64)
    base = np.uint64(_POLY_BASE)
    for j in range(mat.shape[1]):
        live = lens > j
        h[live] = h[live] * base + mat[live, j].astype(np.uint64) + np.uint64(1)
    h ^= h >> np.uint64(29)
    h *= np.uint64(_MIX_MUL)
    h ^= h >> np.uint64(32)
    h[h == 0] = 1
    return h


def build_unigram_tables(spec, utf8=False):
    """((keys uint64 [slots], entries int32 [slots, 4] (id, length, blob offset, 0), scores float64 [slots], blob uint8), slots)
    behind ac_unigram_vocab for a `_unigram_spec` result, on the host (numpy); needs no GPU.  Only the pure-ASCII pieces go in,
    the metaspace in front as 0x20: a piece with a literal space, a control byte, a non-ASCII character or a metaspace further
    in can match no word.  Hashing and slot filling are array operations (a 250k-piece vocabulary takes well under a second);
    the hash restates ac_unigram_hash (tests compare the two).  Adds `max_piece` (longest stored piece) and `unk_score` (the
    minimum score of the WHOLE vocabulary - 10) to `spec`: unigram_vocab_struct reads them.

    utf8=True: the table ac_unigram_encode_utf8 reads -- the same struct, hash, open addressing and array operations over EVERY
    piece as its UTF-8 bytes (the metaspace in front as 0x20); only pieces that can match nothing stay out: a literal space, a
    control byte (a code point with one in its image is host-only), a metaspace further in.  The default call's result and its
    `max_piece` are untouched: the longest stored piece in BYTES goes to spec["max_piece_utf8"].  The UTF-8 kernel matches pieces of
    up to 64 bytes (its reach); a vocabulary with a longer storable piece keeps the Unicode route off (unigram_unicode_tables) and
    the ASCII routing stays.  SentencePiece's trainer caps a piece at 16 characters by default, i.e. at most 64 bytes."""
    vocab = spec["vocab"]
    texts, tids = [], []
    unmatchable = _UNMATCHABLE.search
    for i, (p, _) in enumerate(vocab):
        q = " " + p[1:] if p[:1] == METASPACE else p
        if utf8:
            if q and not unmatchable(q, 1 if q is not p else 0):
                texts.append(q)
                tids.append(i)
        elif q and " " not in p and q.isascii() and q.isprintable() and len(q) <= MAX_DEVICE_BYTES + 1:
            texts.append(q)
            tids.append(i)
    n = len(texts)
    flat = np.frombuffer("".join(texts).encode("utf-8"), np.uint8)
    if utf8 and len(flat) != sum(map(len, texts)):           # byte lengths: ASCII pieces as they are, the others one by one
        lens = np.fromiter((len(t) if t.isascii() else len(t.encode("utf-8")) for t in texts), np.int64, n)
    else:
        lens = np.fromiter(map(len, texts), np.int64, n)
    if utf8:
        spec["max_piece_utf8"] = int(lens.max(initial=1))
    else:
        spec["max_piece"] = max(map(len, texts), default=1)
    spec["unk_score"] = float(min(s for _, s in vocab)) - 10.0 if vocab else -10.0
    slots = 2
    while slots < 2 * n + 16:
        slots <<= 1
    offs = np.zeros(n, np.int64)
    offs[1:] = np.cumsum(lens)[:-1]
    # the dense [pieces, width] matrix holds the pieces of up to 64 bytes (all but a stray few; all a kernel window can match);
    # longer ones -- only the host entry can meet them, inside a word of that length -- are hashed one by one
    short = np.flatnonzero(lens <= _DENSE_PIECE_BYTES)
    rows = np.repeat(np.arange(len(short)), lens[short])
    at = np.repeat(offs[short], lens[short])
    within = np.arange(len(rows)) - np.repeat(np.cumsum(lens[short]) - lens[short], lens[short])
    mat = np.zeros((len(short), int(lens[short].max(initial=1))), np.uint8)
    mat[rows, within] = flat[at + within]
    h = np.zeros(n, np.uint64)
    h[short] = _unigram_hash_rows(mat, lens[short])
    for i in np.flatnonzero(lens > _DENSE_PIECE_BYTES):
        h[i] = _unigram_hash_rows(flat[offs[i]:offs[i] + lens[i]][None, :], lens[i:i + 1])[0]
    keys = np.zeros(slots, np.uint64)
    where = np.zeros(n, np.int64)
    mask = slots - 1
    slot = ((h ^ (h >> np.uint64(32))) & np.uint64(mask)).astype(np.int64)
    todo = np.arange(n)
    while len(todo):                                         # linear probing, a round per probe distance: a piece moves on only
        free = keys[slot[todo]] == 0                         # from a slot that is (or in this round becomes) taken
        cand = todo[free]
        _, first = np.unique(slot[cand], return_index=True)
        placed = cand[first]
        keys[slot[placed]] = h[placed]
        where[placed] = slot[placed]
        stay = np.ones(len(todo), bool)
        stay[np.flatnonzero(free)[first]] = False
        todo = todo[stay]
        slot[todo] = (slot[todo] + 1) & mask
    entries = np.zeros((slots, 4), np.int32)
    scores = np.zeros(slots, np.float64)
    entries[where, 0] = np.asarray(tids, np.int32)
    entries[where, 1] = lens
    entries[where, 2] = offs
    scores[where] = np.asarray([vocab[i][1] for i in tids], np.float64)
    blob = np.concatenate([flat, np.zeros(16, np.uint8)])
    return (keys, entries, scores, blob), slots


def unigram_vocab_struct(spec, pointers, slots, utf8=False):
    """ac_unigram_vocab over the four arrays' addresses (device or host), in build_unigram_tables order (utf8: of its utf8=True
    form, with that table's max_piece)."""
    which = "max_piece_utf8" if utf8 else "max_piece"
    if which not in spec:
        raise nv.NativeError("unigram_vocab_struct: build_unigram_tables(spec) comes first (it measures max_piece and unk_score)")
    return nv.ac_unigram_vocab(*pointers, slots, spec[which], spec["unk_score"], spec["unk_id"], spec["cls_id"], spec["sep_id"],
                               spec["pad_id"], 1 if spec["lowercase"] else 0, 1 if spec["trailing_space_piece"] else 0,
                               1 if spec.get("ws_controls") else 0)


# ---- the Unigram normalizer chain as a probed table (csrc/unigram_core.h) -------------------------------------------------------
UNIGRAM_BUFFER_BYTES = 5120                                       # unigram::kUtf8BufBytes: 0x20 + normalised UTF-8 of one text
UNIGRAM_REACH = 64                                                # unigram::kReach: longest piece the UTF-8 entries match
_UNI_IDENTITY, _UNI_REMOVED, _UNI_IMAGE, _UNI_HOST_ONLY = range(4)
_UNI_MAX_IMAGE = 63                                               # an entry's length field: 6 bits
_UNI_UNICODE_CACHE = {}


def build_unigram_unicode_tables(hf_tokenizer):
    """The whole normalizer chain of a Unigram tokenizer (Precompiled / NFC / NFKC / Nmt / Lowercase / Replace / Strip) as the
    table behind ac_unigram_unicode, on the host (numpy); needs no GPU.  A dict: page_of uint16 [0x1100], entries uint32
    [n_pages, 256], images uint8, n_pages, image_bytes, host_only (the flagged code points, sorted), reasons (counts per probe),
    seconds (of the build).  An entry: bits 0-1 itself | removed | image | host-only, bits 2-7 image bytes, bits 8-31 image offset.

    No Unicode data of our own: every fact is probed from the wrapped normalizer and pre-tokenizer, per code point d (surrogates
    excluded), and where a probe cannot show that the chain acts on d alone the answer is host-only:
    * image(d) = normalize_str("a" + d + "b") without its carrier -- alone in a string a Unicode space may be stripped;
    * the same image at the end ("a" + d), at the start and next to a multi-byte character that has an image (X + d + X + "b",
      d + "b"; X = U+00AA): Precompiled replaces a whole grapheme cluster of fewer than 6 bytes by the image of its shortest
      matching prefix, so a d that clusters with X (combining marks, vowel signs, ZWJ, variation selectors, jamo, prepended marks)
      shows here; Strip and `\\s{2,}` show at the ends and doubled ("a" + d + d + "b");
    * a d whose image is one space must behave as U+0020 does at the end, at the start, doubled and next to a U+0020 -- the
      ASCII probe guard has shown what that is, and the kernel treats every 0x20 of the buffer alike;
    * composition and reordering (NFC / NFKC / Precompiled in the chain): every code point in a non-first position of the
      library's NFD of some code point, and every non-starter (it changes places with U+0345 in front or U+0334 behind under the
      library's NFD; asked of fully decomposed code points, a decomposing one is judged by its first);
    * an image that OPENS with a flagged code point, holds a control character, holds a character the pre-tokenizer splits off
      other than U+0020 (a literal metaspace), or is longer than an entry can say (63 bytes).
    The result is cached in-process by the serialised normalizer + pre-tokenizer (the sweeps take a few seconds)."""
    import time
    from tokenizers import normalizers
    cfg = _backend_config(hf_tokenizer) or {}
    key = json.dumps([cfg.get("normalizer"), cfg.get("pre_tokenizer")], sort_keys=True)
    if key in _UNI_UNICODE_CACHE:
        return _UNI_UNICODE_CACHE[key]
    t0 = time.perf_counter()
    be = hf_tokenizer.backend_tokenizer
    norm = be.normalizer.normalize_str if be.normalizer is not None else (lambda s: s)
    pre = be.pre_tokenizer.pre_tokenize_str
    X = "ª"
    iX = norm(X)
    if norm("ab") != "ab" or norm("a" + X + "b") != "a" + iX + "b":
        raise nv.NativeError("build_unigram_unicode_tables: the normalizer does not keep the probe carrier")
    cps = list(range(0xD800)) + list(range(0xE000, 0x110000))
    chars = list(map(chr, cps))
    host = np.zeros(0x110000, bool)
    host[0xD800:0xE000] = True                                   # (no UTF-8 text holds one: the decoder rejects them)
    reasons = {}

    def flag(which, why):
        which = [c for c in which if not host[c]]
        host[which] = True
        reasons[why] = reasons.get(why, 0) + len(which)

    # the image inside a carrier
    mids = [norm("a" + ch + "b") for ch in chars]
    flag([cp for cp, r in zip(cps, mids) if len(r) < 2 or r[0] != "a" or r[-1] != "b"], "carrier")
    imgs = [r[1:-1] for r in mids]
    del mids
    spaces = {cp for cp, img in zip(cps, imgs) if img == " " and not host[cp]}
    # position, doubling, neighbours with an image (grapheme clusters)
    bad = [cp for cp, ch, img in zip(cps, chars, imgs) if cp not in spaces and norm(X + ch + X + "b") != iX + img + iX + "b"]
    flag(bad, "neighbour")
    bad = [cp for cp, ch, img in zip(cps, chars, imgs) if cp not in spaces and norm("a" + ch) != "a" + img]
    flag(bad, "end")
    bad = [cp for cp, ch, img in zip(cps, chars, imgs) if cp not in spaces and norm(ch + "b") != img + "b"]
    flag(bad, "start")
    bad = [cp for cp, ch, img in zip(cps, chars, imgs) if cp not in spaces and norm("a" + ch + ch + "b") != "a" + img + img + "b"]
    flag(bad, "doubled")
    # a code point that becomes one space is U+0020 to the chain, wherever it stands
    like = [norm(s.replace("_", " ")) for s in ("a_", "_b", "a__b", "a__b", "a__b", X + "_" + X + "b")]
    flag([cp for cp in sorted(spaces) if [norm(s.replace("_", chr(cp))) for s in ("a_", "_b", "a__b")] +
          [norm("a" + chr(cp) + " b"), norm("a " + chr(cp) + "b"), norm(X + chr(cp) + X + "b")] != like], "space")
    # composition seconds and non-starters, by the library's own NFD
    chain = json.dumps(cfg.get("normalizer") or {})
    if any(k in chain for k in ('"NFC"', '"NFKC"', '"NFD"', '"NFKD"', '"Precompiled"')):
        nfd = normalizers.NFD().normalize_str
        decs = list(map(nfd, chars))
        seconds = {ord(d) for dec in decs if len(dec) > 1 for d in dec[1:]}
        hi, lo = "\u0345", "\u0334"                              # combining classes 240 and 1
        nonstart = set()
        for page in range(0x1100):
            ds = [ch for ch in map(chr, range(page * 256, page * 256 + 256)) if not 0xD800 <= ord(ch) < 0xE000]
            ds = [d for d in ds if nfd(d) == d]
            marked = "".join(hi + d + lo for d in ds)
            if nfd(marked) != marked:
                nonstart |= {ord(d) for d in ds if nfd(hi + d) != hi + d or nfd(d + lo) != d + lo}
        flag(sorted(seconds), "composes")
        flag(sorted(nonstart), "non-starter")
        flag([cp for cp, dec in zip(cps, decs) if dec and (ord(dec[0]) in nonstart or ord(dec[0]) in seconds)], "decomposes to one")
        del decs
    # what the images hold
    outs = np.zeros(0x110000, bool)
    for cp, img in zip(cps, imgs):
        if not host[cp] and img:
            outs[[ord(d) for d in img] if len(img) > 1 else ord(img)] = True
    split_off = set()                                            # output characters the pre-tokenizer does not keep inside a word
    for page in range(0x1100):
        at = np.flatnonzero(outs[page * 256:(page + 1) * 256]) + page * 256
        if not len(at):
            continue
        ds = list(map(chr, at.tolist()))
        run = "".join(ds)
        if [p for p, _ in pre("a" + run + "b")] != [METASPACE + "a" + run + "b"]:
            split_off |= {d for d in ds if d != " " and [p for p, _ in pre("a" + d + "b")] != [METASPACE + "a" + d + "b"]}
    bad_img = []
    for cp, img in zip(cps, imgs):
        if host[cp] or not img:
            continue
        if host[ord(img[0])] and img[0] != chr(cp):
            bad_img.append(cp)
        elif any(d in split_off or d < " " or d == "\x7f" for d in img) or len(img.encode("utf-8")) > _UNI_MAX_IMAGE:
            bad_img.append(cp)
    flag(bad_img, "image")
    # entries and the image blob (identical images stored once)
    kind = np.zeros(0x110000, np.uint32)
    where, blob = {}, bytearray()
    for cp, ch, img in zip(cps, chars, imgs):
        if host[cp] or img == ch:
            continue
        if not img:
            kind[cp] = _UNI_REMOVED
            continue
        if img not in where:
            raw = img.encode("utf-8")
            if len(blob) + len(raw) >= 1 << 24:
                host[cp] = True
                continue
            where[img] = _UNI_IMAGE | (len(raw) << 2) | (len(blob) << 8)
            blob += raw
        kind[cp] = where[img]
    kind[host] = _UNI_HOST_ONLY
    pages, page_of = np.unique(kind.reshape(0x1100, 256), axis=0, return_inverse=True)
    host_only = [int(c) for c in np.flatnonzero(host) if not 0xD800 <= c < 0xE000]
    tables = {"page_of": page_of.reshape(-1).astype(np.uint16), "entries": np.ascontiguousarray(pages, np.uint32),
              "images": np.frombuffer(bytes(blob) + b"\0" * 16, np.uint8).copy(), "n_pages": int(len(pages)),
              "image_bytes": int(len(blob)), "host_only": host_only, "reasons": reasons, "seconds": time.perf_counter() - t0}
    _UNI_UNICODE_CACHE[key] = tables
    return tables


def unigram_unicode_struct(tables, pointers=None):
    """ac_unigram_unicode over the three arrays' addresses (device), or over the host arrays themselves."""
    if pointers is None:
        pointers = [tables[k].ctypes.data for k in ("page_of", "entries", "images")]
    return nv.ac_unigram_unicode(*pointers, tables["n_pages"], tables["image_bytes"])


_CJK_99 = "\u6771\u4eac\u90fd\u306b\u4f4f\u3093\u3067\u3044\u307e\u3059\u3002\u4eca\u65e5\u306f\u5929\u6c17\u304c\u3044\u3044\u3067\u3059\u306d\u3001\u6563\u6b69\u306b\u884c\u304d\u307e\u3057\u3087\u3046\u3002"       # a Japanese sentence without a space: one word of 99 bytes


def _unigram_unicode_probes():
    """The fixed probe list of the Unicode guard: multi-character strings over what the table encodes -- accented Latin, Cyrillic,
    Greek, CJK and kana without spaces and over 64 bytes, precomposed Hangul, full-width forms, Unicode spaces leading / trailing /
    doubled, ligatures, one- and two-code-point case mappings, astral code points -- and strings that must defer where the table
    flags them: combining sequences, CRLF, ZWJ emoji, a literal metaspace."""
    base = ["", "a", "Hello, World!", "caf\u00e9 na\u00efve r\u00e9sum\u00e9", "CAF\u00c9 NA\u00cfVE R\u00c9SUM\u00c9",
            "\u00c5ngstr\u00f6m \u0152uvre \u00c6r\u00f8 \u00d0i\u00f0 \u00de\u00fa \u01c5emal",
            "\u0130stanbul \u0131s\u0131 \u017ftra\u00dfe Ma\u00df", "\u03a3\u038a\u03a3\u03a5\u03a6\u039f\u03a3 \u03c3\u03af\u03c3\u03c5\u03c6\u03bf\u03c2 \u03c2",
            "\u212a \u212b \u2126 \u00b5", "\ufb01n \ufb02ow \u01c6 \ufb03", "\ud55c\uad6d\uc5b4 \ud14d\uc2a4\ud2b8 \uac01",
            "\u041f\u0440\u0438\u0432\u0435\u0442, \u041c\u0418\u0420! \u0401\u043b\u043a\u0430 \u0439", _CJK_99,
            "\u4e2d\u6587 mixed \u6587\u672c with \u65e5\u672c\u8a9e\u306e\u30c6\u30ad\u30b9\u30c8",
            "\u8fd9\u4e2a\u4ea7\u54c1\u5f88\u7cdf\u7cd5\u6d6a\u8d39\u94b1\u4e0d\u8981\u4e70" * 3,
            "\u3072\u3089\u304c\u306a \u30ab\u30bf\u30ab\u30ca \uff76\uff9e \u304c", "\U00020000\U0002a6d6 x\U00020000y",
            "emoji \U0001f600 \U0001f1e9\U0001f1ea here", "full \uff57\uff49\uff44\uff54\uff48 \uff21\uff22\uff23 \uff11\uff12\uff13",
            "a\u3000b\u00a0c\u2003d", "\u00a0lead", "trail\u3000", "a\u00a0\u00a0b", "a \u2003 b", "\u3000\u3000",
            "\u201cquoted\u201d \u2014 dash\u2026 \u3001\u3002\u300c\u300d \uff01\uff1f\uff08\uff09",
            "\u00bfQu\u00e9? \u00a1S\u00ed! \u00a71 \u00a92 \u00aa \u00ba \u00abx\u00bb \u00b1\u00bd \u00b5 \u00b6 \u00b7 \u00d7 \u00f7 \u00a8 \u00b4",
            "x" * 20 + "\u00e9" * 30, "\u20ac100 \u00a35 \u00a57 \u20b99 \u21163 \u2122 \u2103 \u2163 \u2177 \u2460 \u3231 \ufdfa",
            "zero\u200bwidth soft\u00adhyphen re\ufffdplaced \ufeffbom", "\u1ec7 \u1ec6 \u01d6 \u01d5 \u1e69",
            "Stra\u00dfe STRASSE \u1e9e", "\u0386\u0388\u0389 \u03ac\u03ad\u03ae", "\u0e20\u0e32\u0e29\u0e32", "\u0939\u093f\u0928\u094d\u0926\u0940",
            "e\u0301 combining", "A\u0301\u0323", "\uff21\u0301", "a\r\nb", "\U0001f468\u200d\U0001f469\u200d\U0001f467 zwj",
            "literal " + METASPACE + " metaspace", "a" + METASPACE + "b", "\uac00\u11a8 \u1100\u1161 jamo"]
    return base + [" ".join(base[i:i + 3]) for i in range(3, 30, 3)]


def _unigram_unicode_matches(hf, spec, pieces, tables, probes):
    """Does ac_unigram_encode_utf8_host (host tables) give the wrapped tokenizer's ids, mask and lengths on these probes, and
    report as not done exactly those that hold a host-only code point?  A probe that fills max_length counts as a mismatch."""
    M = _PROBE_MAX_LENGTH
    probes = [t for t in probes if not any(sp in t for sp in spec["specials"])]
    flagged = _host_only_regex(tables)
    arrays, slots = pieces
    vocab = unigram_vocab_struct(spec, [a.ctypes.data for a in arrays], slots, utf8=True)
    raws = [t.encode("utf-8") for t in probes]
    offs = np.zeros(len(raws) + 1, np.int32)
    offs[1:] = np.cumsum([len(r) for r in raws])
    blob = np.frombuffer(b"".join(raws) + b"\0" * 64, np.uint8).copy()
    ids = np.zeros((len(raws), M), np.int64)
    mask = np.zeros((len(raws), M), np.int64)
    lens = np.zeros(len(raws), np.int32)
    uni = unigram_unicode_struct(tables)
    nv.check(nv.lib().ac_unigram_encode_utf8_host(blob.ctypes.data, offs.ctypes.data, len(raws), ctypes.byref(vocab), ctypes.byref(uni),
                                                  M, ids.ctypes.data, mask.ctypes.data, lens.ctypes.data), "ac_unigram_encode_utf8_host")
    want = hf(probes, max_length=M, truncation=True, padding="max_length", return_tensors="np")
    for i, t in enumerate(probes):
        if flagged is not None and flagged.search(t):
            if lens[i] != -1:
                return False
        elif lens[i] < 0 or lens[i] >= M or not np.array_equal(want["input_ids"][i], ids[i]) \
                or not np.array_equal(want["attention_mask"][i], mask[i]):
            return False
    return True


def unigram_unicode_tables(hf, spec):
    """(build_unigram_unicode_tables(hf), build_unigram_tables(spec, utf8=True)) behind their probe guard, or None -- the
    tokenizer then keeps its ASCII-only routing: a storable piece of more than 64 bytes (the kernel's reach), or a probe on which
    the host entry over these tables does not reproduce the wrapped tokenizer."""
    try:
        pieces = build_unigram_tables(spec, utf8=True)
        if spec["max_piece_utf8"] > UNIGRAM_REACH:
            return None
        tables = build_unigram_unicode_tables(hf)
        return (tables, pieces) if _unigram_unicode_matches(hf, spec, pieces, tables, _unigram_unicode_probes()) else None
    except Exception:
        return None


# ---- what the wrappers share ---------------------------------------------------------------------------------------
def _pack_batch(blob, sizes, dev):
    """Offsets and text in ONE host-to-device copy: [int32 offs[b + 1] | pad to 16 | text bytes | 64 zero bytes]."""
    b = len(sizes)
    head = (4 * (b + 1) + 15) // 16 * 16
    buf = np.zeros(head + len(blob) + 64, np.uint8)
    buf[:4 * (b + 1)].view(np.int32)[1:] = np.cumsum(sizes, dtype=np.int64).astype(np.int32)
    buf[head:head + len(blob)] = np.frombuffer(blob, np.uint8)
    d_buf = torch.from_numpy(buf).to(dev)
    return d_buf[:4 * (b + 1)], d_buf[head:]


def _splice_host_rows(hf, texts, host_rows, M, ids, mask, lens):
    """The wrapped tokenizer itself for what the kernel does not cover, written over those rows of the batch."""
    dev = ids.device
    enc = hf([texts[i] for i in host_rows], max_length=M, truncation=True, padding="max_length", return_tensors="pt")
    rows = torch.tensor(host_rows, dtype=torch.int64, device=dev)
    ids[rows] = enc["input_ids"].to(dev)
    mask[rows] = enc["attention_mask"].to(dev)
    lens[rows] = enc["attention_mask"].sum(1).to(device=dev, dtype=torch.int32)


class _DeviceTokenizer:
    """Callable with the signature the classifier uses; returns device tensors.  A subclass sets `specials`, `_with_types`
    (return token_type_ids), `_defers` (its kernel may mark a text not done: lens -1) and launches its kernel in `_encode` (ascii_only: every device text of the
    batch is ASCII)."""
    _defers = False
    _with_types = True
    _eligible = None                                     # bytes a device text may hold (None: any ASCII byte)
    _utf8 = False                                        # device texts may hold non-ASCII bytes (the subclass overrides _device_ok)

    def __init__(self, hf_tokenizer, device=None):
        self.hf = hf_tokenizer
        self.device = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")
        self.device_texts = self.host_texts = 0          # routing statistics

    def _bytes_ok(self, raw):
        return raw.isascii() and (self._eligible is None or not raw.translate(None, self._eligible))

    def _device_ok(self, text, raw):
        return len(raw) <= MAX_DEVICE_BYTES and self._bytes_ok(raw) and not any(sp in text for sp in self.specials)

    def __call__(self, texts, max_length=512, truncation=True, padding=True, return_tensors="pt", **kw):
        if isinstance(texts, str):
            texts = [texts]
        if not truncation or not padding or return_tensors != "pt" or kw:
            raise nv.NativeError(f"{type(self).__name__} supports the classifier's call only: truncation=True, padding=True, "
                                 "return_tensors='pt'")
        b = len(texts)
        M = int(max_length)
        dev = self.device
        # common case first: one pass over the joined batch decides that every text is plain ASCII, short enough and free
        # of special-token strings (a match across a text boundary only costs the slow path)
        joined = "".join(texts)
        blob = joined.encode("ascii") if joined.isascii() else None
        if blob is not None and self._bytes_ok(blob) and not any(sp in joined for sp in self.specials) \
                and max(map(len, texts), default=0) <= MAX_DEVICE_BYTES:
            on_dev = [True] * b
            sizes = [len(t) for t in texts]
        else:
            raws = [t.encode("utf-8") for t in texts]
            on_dev = [self._device_ok(t, r) for t, r in zip(texts, raws)]
            sizes = [len(r) if ok else 0 for r, ok in zip(raws, on_dev)]
            blob = b"".join(r for r, ok in zip(raws, on_dev) if ok)
        ascii_only = not self._utf8 or joined.isascii()
        ids = torch.empty((b, M), dtype=torch.int64, device=dev)
        mask = torch.empty((b, M), dtype=torch.int64, device=dev)
        lens = torch.empty(b, dtype=torch.int32, device=dev)
        d_offs, d_text = _pack_batch(blob, sizes, dev)
        with torch.cuda.device(dev):
            self._encode(d_text, d_offs, b, M, ids, mask, lens, ascii_only)
        host_rows = [i for i, ok in enumerate(on_dev) if not ok]
        if host_rows:
            _splice_host_rows(self.hf, texts, host_rows, M, ids, mask, lens)
        # the one host sync: the encoder launch needs S (and, where the kernel may defer a text, whether it did: the minimum
        # of lens travels with the maximum)
        if not b:
            S = 0
        elif self._defers:
            lo, S = torch.stack(torch.aminmax(lens)).tolist()
            if lo < 0:                                   # rare: those texts go to the wrapped tokenizer after all
                later = (lens < 0).nonzero().flatten().tolist()
                _splice_host_rows(self.hf, texts, later, M, ids, mask, lens)
                host_rows = host_rows + later
                S = int(lens.max().item())
        else:
            S = int(lens.max().item())
        self.device_texts += b - len(host_rows)
        self.host_texts += len(host_rows)
        ids_s, mask_s = ids[:, :S].contiguous(), mask[:, :S].contiguous()
        if self._with_types:
            return {"input_ids": ids_s, "token_type_ids": torch.zeros_like(ids_s), "attention_mask": mask_s}
        return {"input_ids": ids_s, "attention_mask": mask_s}

    # pass-through of what callers may read from the wrapped tokenizer
    def __getattr__(self, name):
        return getattr(self.hf, name)


class HipWordPieceTokenizer(_DeviceTokenizer):
    """BERT WordPiece on the device: ASCII batches through ac_wordpiece_encode; with `unicode=True` a batch that holds
    non-ASCII text goes through ac_wordpiece_encode_utf8 (the probed normaliser / class table of
    build_wordpiece_unicode_tables), except the texts with a host-only code point.  Opt-in: without it every non-ASCII text
    takes the host route, as before.  `unicode` reads False afterwards if the probe guard rejected the tables."""

    def __init__(self, hf_tokenizer, device=None, unicode=False):
        nv.require_gpu()
        spec = _wordpiece_spec(hf_tokenizer)
        if spec is None:
            raise nv.NativeError("HipWordPieceTokenizer: not a BERT WordPiece tokenizer (BertNormalizer + BertPreTokenizer + WordPiece)")
        super().__init__(hf_tokenizer, device)
        vocab, self.lower, self.specials = spec
        host = self._build_table(vocab)
        self.unicode = False
        if unicode:
            self._enable_unicode(vocab, host)

    # ---- vocabulary -> device hash table ---------------------------------------------------------------
    def _build_table(self, vocab):
        arrays, slots, max_piece = build_wordpiece_tables(vocab)
        keys, offs, ids, lens, blob = arrays
        self._t = [torch.from_numpy(a).to(self.device) for a in (keys.view(np.int64), offs.view(np.int32), ids, lens.view(np.int16), blob)]
        self.vocab = wordpiece_vocab_struct(self.hf, vocab, self.lower, [t.data_ptr() for t in self._t], slots, max_piece)
        self.pad_id = vocab[self.hf.pad_token]
        return arrays, slots, max_piece

    # ---- normaliser / class table -> device (behind the probe guard, which runs on the host arrays) ----
    def _enable_unicode(self, vocab, host):
        arrays, slots, max_piece = host
        host_vocab = wordpiece_vocab_struct(self.hf, vocab, self.lower, [a.ctypes.data for a in arrays], slots, max_piece)
        tables = wordpiece_unicode_tables(self.hf, self.specials, host_vocab)
        if tables is None:
            return
        self._ut = [torch.from_numpy(a).to(self.device) for a in (tables["page_of"].view(np.int16), tables["entries"].view(np.int32),
                                                                   tables["images"])]
        self.unicode_tables = wordpiece_unicode_struct(tables, [t.data_ptr() for t in self._ut])
        self._host_only = _host_only_regex(tables)
        self.unicode = self._utf8 = self._defers = True

    def _device_ok(self, text, raw):
        if not self._utf8 or raw.isascii():
            return super()._device_ok(text, raw)
        return len(raw) <= MAX_DEVICE_BYTES and not (self._host_only is not None and self._host_only.search(text)) \
            and not any(sp in text for sp in self.specials)

    def _encode(self, d_text, d_offs, b, M, ids, mask, lens, ascii_only=True):
        if ascii_only:
            nv.check(nv.lib().ac_wordpiece_encode(nv.ptr(d_text), nv.ptr(d_offs), b, ctypes.byref(self.vocab), M, nv.ptr(ids),
                                                  nv.ptr(mask), nv.ptr(lens), nv.stream_ptr(self.device)), "ac_wordpiece_encode")
        else:
            nv.check(nv.lib().ac_wordpiece_encode_utf8(nv.ptr(d_text), nv.ptr(d_offs), b, ctypes.byref(self.vocab),
                                                       ctypes.byref(self.unicode_tables), M, nv.ptr(ids), nv.ptr(mask), nv.ptr(lens),
                                                       nv.stream_ptr(self.device)), "ac_wordpiece_encode_utf8")


class HipByteBPETokenizer(_DeviceTokenizer):
    """GPT-2 byte-level BPE on the device (ac_bpe_encode): RoBERTa-style and ModernBERT-style tokenizers.  Returns the keys
    the wrapped tokenizer returns (no token_type_ids where its model_input_names has none).

    With `unicode=True` a batch that holds non-ASCII text goes through ac_bpe_utf8_encode: the classes of the pre-tokeniser
    pattern as the probed table of build_bpe_unicode_tables, the merges on the text's own bytes as before.  A non-ASCII text is a
    device text if it has at most 4096 bytes, no literal special / added-token string and no host-only code point (one compiled
    character class; with an NFC normalizer: what NFC changes or may combine); a pre-token of more than 64 bytes comes back
    from the kernel as not done.  Opt-in: without it every non-ASCII text takes the host route, as before.  `unicode` reads False
    afterwards if the probe guard rejected the tables."""
    _defers = True

    def __init__(self, hf_tokenizer, device=None, unicode=False):
        nv.require_gpu()
        spec = _bpe_spec(hf_tokenizer)
        if spec is None:
            raise nv.NativeError("HipByteBPETokenizer: not a byte-level BPE tokenizer this build reproduces (ByteLevel(use_regex) + BPE "
                                 "behind RobertaProcessing or a <cls> $A <sep> template)")
        super().__init__(hf_tokenizer, device)
        self.specials, self._with_types, self.pad_id = spec["specials"], spec["token_type_ids"], spec["pad_id"]
        keys, entries, blob, byte_id, slots = build_bpe_tables(spec)
        self._t = [torch.from_numpy(a).to(self.device) for a in (keys.view(np.int64), entries, blob, byte_id)]
        self.vocab = bpe_vocab_struct(spec, [t.data_ptr() for t in self._t], slots)
        self.unicode = False
        if unicode:
            self._enable_unicode(spec, (keys, entries, blob, byte_id), slots)

    # ---- class table -> device (behind the probe guard, which runs on the host arrays) ----
    def _enable_unicode(self, spec, arrays, slots):
        host_vocab = bpe_vocab_struct(spec, [a.ctypes.data for a in arrays], slots)
        tables = bpe_unicode_tables(self.hf, spec, host_vocab)
        if tables is None:
            return
        self._ut = [torch.from_numpy(a).to(self.device) for a in (tables["page_of"].view(np.int16), tables["entries"])]
        self.unicode_tables = bpe_unicode_struct(tables, [t.data_ptr() for t in self._ut])
        self._host_only = _host_only_regex(tables)
        self.unicode = self._utf8 = True

    def _device_ok(self, text, raw):
        if not self._utf8 or raw.isascii():
            return super()._device_ok(text, raw)
        return len(raw) <= MAX_DEVICE_BYTES and not (self._host_only is not None and self._host_only.search(text)) \
            and not any(sp in text for sp in self.specials)

    def _encode(self, d_text, d_offs, b, M, ids, mask, lens, ascii_only=True):
        if ascii_only:
            nv.check(nv.lib().ac_bpe_encode(nv.ptr(d_text), nv.ptr(d_offs), b, ctypes.byref(self.vocab), M, nv.ptr(ids),
                                            nv.ptr(mask), nv.ptr(lens), nv.stream_ptr(self.device)), "ac_bpe_encode")
        else:
            nv.check(nv.lib().ac_bpe_utf8_encode(nv.ptr(d_text), nv.ptr(d_offs), b, ctypes.byref(self.vocab),
                                                 ctypes.byref(self.unicode_tables), M, nv.ptr(ids), nv.ptr(mask), nv.ptr(lens),
                                                 nv.stream_ptr(self.device)), "ac_bpe_utf8_encode")


class HipUnigramTokenizer(_DeviceTokenizer):
    """SentencePiece-style Unigram on the device (ac_unigram_encode): DeBERTa-v2/v3 style and XLM-R style tokenizers.  Device
    texts hold the bytes 0x20-0x7E and (where the wrapped tokenizer treats them as plain whitespace) \\t \\n \\r only; returns
    the keys the wrapped tokenizer returns.

    With `unicode=True` a batch that holds non-ASCII text goes through ac_unigram_encode_utf8: the whole normalizer chain as the
    probed table of build_unigram_unicode_tables, every piece of the vocabulary as UTF-8 bytes, words of any length (a Chinese
    or Japanese sentence is one word).  A non-ASCII text is a device text if it has at most 4096 bytes, no literal special /
    added-token string and no host-only code point (one compiled character class).  Opt-in: without it every non-ASCII text takes
    the host route, as before.  `unicode` reads False afterwards if the probe guard rejected the tables or the vocabulary holds a
    piece of more than 64 bytes."""
    _defers = True

    def __init__(self, hf_tokenizer, device=None, structure=None, unicode=False):
        nv.require_gpu()
        spec = _unigram_spec(hf_tokenizer, structure)      # structure: the caller's _unigram_structure(hf_tokenizer), if it has one
        if spec is None:
            raise nv.NativeError("HipUnigramTokenizer: not a Unigram tokenizer this build reproduces (Metaspace(always) + Unigram "
                                 "behind a <cls> $A <sep> template, and identical ids on the probe list)")
        super().__init__(hf_tokenizer, device)
        self.specials, self._with_types, self.pad_id = spec["specials"], spec["token_type_ids"], spec["pad_id"]
        self._eligible = _WORD_BYTES + (b"\t\n\r" if spec["ws_controls"] else b"")
        arrays, slots = spec.pop("tables")                  # the host tables the probe guard ran on
        self._t = [torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(self.device) for a in arrays]
        self.vocab = unigram_vocab_struct(spec, [t.data_ptr() for t in self._t], slots)
        self.unicode = False
        if unicode:
            self._enable_unicode(spec)

    # ---- normalizer table and the all-piece table -> device (behind the probe guard, which runs on the host arrays) ----
    def _enable_unicode(self, spec):
        got = unigram_unicode_tables(self.hf, spec)
        if got is None:
            return
        tables, (arrays, slots) = got
        self._ut = [torch.from_numpy(a).to(self.device) for a in (tables["page_of"].view(np.int16), tables["entries"].view(np.int32),
                                                                   tables["images"])]
        self._t8 = [torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(self.device) for a in arrays]
        self.unicode_tables = unigram_unicode_struct(tables, [t.data_ptr() for t in self._ut])
        self.vocab_utf8 = unigram_vocab_struct(spec, [t.data_ptr() for t in self._t8], slots, utf8=True)
        self._host_only = _host_only_regex(tables)
        self.unicode = self._utf8 = True

    def _device_ok(self, text, raw):
        if not self._utf8 or raw.isascii():
            return super()._device_ok(text, raw)
        return len(raw) <= MAX_DEVICE_BYTES and not (self._host_only is not None and self._host_only.search(text)) \
            and not any(sp in text for sp in self.specials)

    def _encode(self, d_text, d_offs, b, M, ids, mask, lens, ascii_only=True):
        if ascii_only:
            nv.check(nv.lib().ac_unigram_encode(nv.ptr(d_text), nv.ptr(d_offs), b, ctypes.byref(self.vocab), M, nv.ptr(ids),
                                                nv.ptr(mask), nv.ptr(lens), nv.stream_ptr(self.device)), "ac_unigram_encode")
        else:
            nv.check(nv.lib().ac_unigram_encode_utf8(nv.ptr(d_text), nv.ptr(d_offs), b, ctypes.byref(self.vocab_utf8),
                                                     ctypes.byref(self.unicode_tables), M, nv.ptr(ids), nv.ptr(mask), nv.ptr(lens),
                                                     nv.stream_ptr(self.device)), "ac_unigram_encode_utf8")


def maybe_device_tokenizer(hf_tokenizer, device, unicode=False):
    """HipWordPieceTokenizer around a BERT WordPiece tokenizer, HipByteBPETokenizer around a GPT-2 byte-level BPE tokenizer,
    HipUnigramTokenizer around a Metaspace + Unigram tokenizer, anything else unchanged.  unicode: non-ASCII texts on the device
    too (all three families have a kernel for them; each keeps its ASCII-only routing if its probe guard rejects the tables)."""
    if hf_tokenizer is None or isinstance(hf_tokenizer, _DeviceTokenizer):
        return hf_tokenizer
    try:
        if _wordpiece_spec(hf_tokenizer) is not None:
            return HipWordPieceTokenizer(hf_tokenizer, device, unicode=unicode)
        if _bpe_spec(hf_tokenizer) is not None:
            return HipByteBPETokenizer(hf_tokenizer, device, unicode=unicode)
        structure = _unigram_structure(hf_tokenizer)
        if structure is not None:                             # (the probe guard runs inside the constructor)
            return HipUnigramTokenizer(hf_tokenizer, device, structure, unicode=unicode)
        return hf_tokenizer
    except Exception:
        return hf_tokenizer
