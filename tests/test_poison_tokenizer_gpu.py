"""GPU suite: the four device tokenizer entries into poisoned ids / mask / lens (tests/poison.py).

Regions, read from csrc/wordpiece.hip, bpe.hip, unigram.hip and tokenizer.py::_DeviceTokenizer.__call__ before any poisoned run:
the entries have no workspace (their scratch is LDS, filled by the wave before it reads it); the outputs ids [b, M], mask [b, M]
and lens [b] come from torch.empty (tokenizer.py:729-731).  A text that is DONE has its whole row written -- pieces, [SEP], pad
ids up to M, the mask over all M columns -- and lens[tx] = its length; a text the kernel hands back (lens[tx] = -1) has its row
left unwritten and the wrapper writes that row from the wrapped tokenizer, as it does for the texts it routes to the host before
the launch (those travel as empty texts and get a [CLS] [SEP] row first).  lens is written for every text.  Nothing is the
caller's duty to clear, and no output word is an index or a count to any kernel.

Per entry one batch holds: a text of zero length, one of 1 byte, one that fills max_length exactly, one that is truncated, and one
the kernel hands back as not done (BPE: a pre-token beyond the 64-byte window; Unigram: such a word; WordPiece UTF-8: Hangul whose
NFD image overflows the 8 KiB buffer -- the uncased configuration; the ASCII WordPiece entry has no such verdict, it never defers,
so that batch has none).  A second batch of short texts only is padded to its longest text, below max_length.  Four states
(zero, zero again, ff, leftover: a larger batch at a larger max_length first); padding=True and padding="max_length" (the batch
with the exactly-filling text: both forms are [b, max_length]).  (a) the returned tensors are bit-identical in every state;
(b) they equal the wrapped tokenizer's in every position (the reference of the tokenizer suites), and the routing counts say that
the hand-back really happened.
"""
import time

import pytest
import torch

import bpe_helpers as BH
import poison
import unigram_helpers as UH
import wordpiece_helpers as WH

pytestmark = pytest.mark.gpu

_T0 = time.time()
M_LEN = 8
WORDS = WH.WORDS


@pytest.fixture(scope="module", autouse=True)
def _wall():
    yield
    print(f"\nMEASURED test_poison_tokenizer_gpu wall time {time.time() - _T0:.1f} s")


def _build(entry, dev):
    """(wrapped tokenizer, device tokenizer, the text the kernel hands back or None)"""
    from adaptive_classifier import tokenizer as T
    if entry == "wordpiece_ascii":
        from transformers import BertTokenizer
        hf = BertTokenizer(vocab=WH.ascii_vocab(), do_lower_case=True)
        return hf, T.HipWordPieceTokenizer(hf, device=dev), None
    if entry == "wordpiece_utf8":
        hf = WH.build_tokenizer("uncased")
        tok = T.HipWordPieceTokenizer(hf, device=dev, unicode=True)
        assert tok.unicode and tok._defers
        return hf, tok, "한" * 1300                       # 3900 bytes in, 11700 bytes of jamo out: more than the 8 KiB buffer
    if entry == "bpe":
        hf = BH.build_tokenizer("roberta")
        return hf, T.HipByteBPETokenizer(hf, device=dev), "x" * 80 + " tail"
    hf = UH.build_tokenizer("sparse", "deberta")
    return hf, T.HipUnigramTokenizer(hf, device=dev), "x" * 80 + " tail"


def _length(hf, text):
    return len(hf(text, truncation=False)["input_ids"])


def _texts_of_length(hf, words):
    """(a text of exactly M_LEN tokens with its specials, a text of more): words added one by one, those that overshoot left out"""
    text, exact = "", None
    for w in words:
        cand = (text + " " + w).strip()
        n = _length(hf, cand)
        if n <= M_LEN:
            text = cand
        if n == M_LEN:
            exact = cand
            break
    assert exact is not None, "no prefix of the word list fills max_length exactly"
    longer = exact + " " + " ".join(words[:6])
    assert _length(hf, longer) > M_LEN and _length(hf, exact) == M_LEN
    return exact, longer


def _equal_everywhere(got, want, batch):
    assert set(got.keys()) == set(want.keys())
    for key in want.keys():
        g, w = got[key].cpu(), want[key]
        assert got[key].is_cuda and g.shape == w.shape, (key, g.shape, w.shape)
        bad = (g != w).any(dim=1).nonzero().flatten().tolist()
        assert not bad, (key, [(batch[i][:40], g[i].tolist(), w[i].tolist()) for i in bad[:2]])


@pytest.mark.parametrize("entry", ["wordpiece_ascii", "wordpiece_utf8", "bpe", "unigram"])
def test_device_tokenizer_outputs(entry, cuda_dev, monkeypatch):
    hf, tok, handed_back = _build(entry, cuda_dev)
    words = [w for w in WORDS if w.isalpha()]
    if entry == "wordpiece_utf8":                            # non-ASCII words of this vocabulary: the UTF-8 entry is the one launched
        words = ["café", "naïve", "é", "中", "文", "e", "한"] + [w for w in WH.vocab() if w.isalpha() and not w.isascii()][:40]
    exact, longer = _texts_of_length(hf, words)
    full = ["", words[0][:1], exact, longer] + ([handed_back] if handed_back else [])
    short = ["", words[0][:1], " ".join(words[:2])]
    if entry == "wordpiece_utf8":
        assert not "".join(full).isascii() and not "".join(short).isascii()
    assert max(_length(hf, t) for t in short) < M_LEN
    bigger = (full + short) * 3                              # the leftover state's first call: more rows, max_length 24
    calls = [(full, True), (full, "max_length"), (short, True)]
    want = [hf(batch, max_length=M_LEN, truncation=True, padding=padding, return_tensors="pt") for batch, padding in calls]
    assert want[0]["input_ids"].shape == want[1]["input_ids"].shape == (len(full), M_LEN) and want[2]["input_ids"].shape[1] < M_LEN

    p = poison.poisoned_empty(monkeypatch, None)
    res = {}
    for state, byte in (("zero", 0x00), ("zero2", 0x00), ("ff", 0xFF), ("leftover", None)):
        p.byte = byte
        if state == "leftover":
            tok(bigger, max_length=24, truncation=True, padding=True, return_tensors="pt")
        before = (tok.device_texts, tok.host_texts)
        res[state] = [tok(batch, max_length=M_LEN, truncation=True, padding=padding, return_tensors="pt") for batch, padding in calls]
        torch.cuda.synchronize()
        on_dev, on_host = tok.device_texts - before[0], tok.host_texts - before[1]
        # the hand-back happened (two calls hold that text) and nothing else left the device
        assert (on_dev, on_host) == (2 * len(full) + len(short) - (2 if handed_back else 0), 2 if handed_back else 0), (state, on_dev, on_host)
        for got, w, (batch, _) in zip(res[state], want, calls):
            _equal_everywhere(got, w, batch)
    p.byte = None
    assert p.filled >= 3 * 3 * 3                             # ids, mask, lens of three calls in three filled states
    res = {s: [{k: v.cpu() for k, v in r.items()} for r in rs] for s, rs in res.items()}
    assert poison.same_bits(res["zero"], res["zero2"]), "two zero-state runs differ: " + poison.first_difference(res["zero"], res["zero2"])
    for state in ("ff", "leftover"):
        assert poison.same_bits(res["zero"], res[state]), f"the {state} state changed the result: " + poison.first_difference(res["zero"], res[state])
