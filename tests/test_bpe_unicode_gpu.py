"""Byte-level BPE on UTF-8 text on the device: bpe_utf8_kernel (ac_bpe_utf8_encode) against the host entry over the same tables
(which test_bpe_unicode_cpu.py holds against the tokenizers library) and against the wrapped tokenizer itself -- bit for bit, no
tolerance -- on the smallest shapes that can go wrong: characters of every width alone, pre-tokens of exactly 64 and of 65 bytes,
characters straddling a window's last byte, a full 4096-byte text, Unicode whitespace, contractions, numbers, truncation; outputs
start poisoned.  Then HipByteBPETokenizer(unicode=True): equality, exact routing counts, the ASCII entry for ASCII batches, the
default routing unchanged, and a classifier with config["device_tokenizer_unicode"]."""
import ctypes

import numpy as np
import pytest
import torch

import bpe_helpers as B
import bpe_unicode_helpers as H
import poison

pytestmark = pytest.mark.gpu

KERNEL_WINDOW = 64
ASTRAL_LETTER = "\U00020000"                              # a 4-byte letter (CJK extension B)


def _pretoken_of(n_bytes, last):
    """a text whose second pre-token (a space, ASCII letters, `last`) has exactly n_bytes bytes"""
    return "x " + "a" * (n_bytes - 1 - len(last.encode("utf-8"))) + last


def _straddlers():
    """short pre-tokens, a multi-byte character whose bytes lie on both sides of byte 63 / 64 of the first window, for every
    alignment (with and without the prefix-space shift): inside a word, and as a pre-token start of its own (the emoji)"""
    out = []
    for pad in range(57, 66):
        for ch in ("é", "中", ASTRAL_LETTER, "\U0001f600", "\u3000"):
            out.append(("abc de " * 12)[:pad] + "xy" + ch + "q and the rest of it")
    return out


EDGES = (["", "é", "中", "\U0001f600", ASTRAL_LETTER, "a"] +
         [_pretoken_of(64, ch) for ch in ("é", "中", ASTRAL_LETTER)] +
         [_pretoken_of(64, ch) + " tail" for ch in ("é", "中", ASTRAL_LETTER)] +
         ["ab " * 1364 + "q中", " ab" * 1364 + "q中"] +                                       # 4096 bytes, with and without the shift
         ["\u00a0\u00a0x", "a\u3000\u3000 b", "a \u2028\u0085b", "a\u00a0 \u3000 é", "tail\u00a0\u3000", "tail \u2028", "tail\u0085",
          "\u00a0", "\u3000\u2028", " \u0085 ", "\u2028\u0085\u00a0\u3000", "\u00a0's", "a\u3000's"] +
         ["é's", "'sé", "中's", "x’s", "x'ré", "é'll", "x'llé", "é'S"] +
         ["12²", "١٢٣4", "Ⅷ", "3é ½ x²"] +
         ["it’s “quoted” — dash… en–dash", "Привет, мир! хорошо", "中文 mixed 文本", "emoji \U0001f600\U0001f600 here \U0001f44d\U0001f3fd!",
          "great product works well", "AWFUL... don't buy", "café naïve résumé " * 6])
TOO_LONG = [_pretoken_of(65, ch) for ch in ("é", "中", ASTRAL_LETTER)] + ["中文产品很好" * 5]       # a pre-token of 65 bytes; of 90


class _Device:
    """the host tables of a configuration and their device copies"""

    def __init__(self, kind, dev):
        from adaptive_classifier import tokenizer as tkz
        self.kind, self.dev = kind, dev
        self.hf = H.build_tokenizer(kind)
        self.ht = H.HostTables(self.hf)
        hv, t = self.ht.hv, self.ht.tables
        self.keep = [torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(dev) for a in hv.arrays]
        self.keep_u = [torch.from_numpy(a).to(dev) for a in (t["page_of"].view(np.int16), t["entries"])]
        self.vocab = tkz.bpe_vocab_struct(hv.spec, [x.data_ptr() for x in self.keep], hv.slots)
        self.unicode = tkz.bpe_unicode_struct(t, [x.data_ptr() for x in self.keep_u])

    def encode(self, raws, M, byte):
        """ac_bpe_utf8_encode over byte strings, outputs byte-filled first -> (ids, mask, lens) as numpy"""
        from adaptive_classifier import _native as nv
        b = len(raws)
        rows = max(b, 1)                                   # (b = 0: the entry still wants non-NULL outputs, and must leave them alone)
        blob, offs = H.pack(raws)
        d_blob, d_offs = torch.from_numpy(blob).to(self.dev), torch.from_numpy(offs).to(self.dev)
        ids = poison.fill(torch.empty((rows, M), dtype=torch.int64, device=self.dev), byte)
        mask = poison.fill(torch.empty((rows, M), dtype=torch.int64, device=self.dev), byte)
        lens = poison.fill(torch.empty(rows, dtype=torch.int32, device=self.dev), byte)
        with torch.cuda.device(self.dev):
            nv.check(nv.lib().ac_bpe_utf8_encode(nv.ptr(d_blob), nv.ptr(d_offs), b, ctypes.byref(self.vocab), ctypes.byref(self.unicode), M,
                                                 nv.ptr(ids), nv.ptr(mask), nv.ptr(lens), nv.stream_ptr(self.dev)), "ac_bpe_utf8_encode")
        torch.cuda.synchronize()
        return ids.cpu().numpy(), mask.cpu().numpy(), lens.cpu().numpy()


@pytest.fixture(scope="module", params=H.CONFIGS)
def device(request, cuda_dev):
    return _Device(request.param, cuda_dev)


def _poison_word(byte, dtype):
    return np.frombuffer(bytes([byte]) * 8, dtype)[0]


@pytest.mark.parametrize("byte", [poison.FF, poison.ZERO])
@pytest.mark.parametrize("max_length", [96, 8, 2])
def test_kernel_equals_host_entry_and_wrapped_tokenizer_on_the_edges(device, max_length, byte):
    d = device
    texts = d.ht.device_route(EDGES + _straddlers())
    assert len(texts) >= len(EDGES) + 40 and all(t in texts for t in EDGES)
    for t in EDGES[6:12]:                                  # exactly the window, by the library's own pre-tokenizer
        assert B.longest_pretoken(d.hf, t) == KERNEL_WINDOW, t
    assert [len(t.encode()) for t in EDGES[12:14]] == [4096, 4096]
    raws = [t.encode("utf-8") for t in texts]
    ids, mask, lens = d.encode(raws, max_length, byte)
    h_ids, h_mask, h_lens = H.encode_host(d.ht, raws, max_length)
    assert (lens >= 2).all(), [texts[i][:40] for i in np.nonzero(lens < 2)[0]]
    assert np.array_equal(lens, h_lens) and np.array_equal(ids, h_ids) and np.array_equal(mask, h_mask)      # every position written
    want = d.hf(texts, max_length=max_length, truncation=True, padding="max_length", return_tensors="np")
    bad = np.nonzero((ids != want["input_ids"]).any(1) | (mask != want["attention_mask"]).any(1))[0]
    assert len(bad) == 0, [(texts[i][:60], ids[i].tolist()[:16], want["input_ids"][i].tolist()[:16]) for i in bad[:3]]


@pytest.mark.parametrize("byte", [poison.FF, poison.ZERO])
def test_handed_back_rows_stay_untouched(device, byte):
    """a pre-token of 65 bytes, malformed UTF-8, a host-only code point, 4097 bytes: lens -1 and the rows still poison; the rows
    between them are done"""
    d = device
    for t in TOO_LONG[:3]:
        assert B.longest_pretoken(d.hf, t) == KERNEL_WINDOW + 1, t
    back = [t.encode("utf-8") for t in TOO_LONG] + [b"a\xc0\xafb", b"x\xed\xa0\x80", b"a\x80b", b"caf\xc3", b"\xf4\x90\x80\x80",
                                                     b"ab " * 1365 + b"\xc3\xa9"]
    if d.kind == "modernbert":
        back += [t.encode("utf-8") for t in H.NFC_SENSITIVE]
    good = ["café", "中 x", "\U0001f600", "plain"]
    raws = []
    for i, r in enumerate(back):
        raws += [r, good[i % 4].encode("utf-8")]
    M = 16
    ids, mask, lens = d.encode(raws, M, byte)
    want = d.hf(good, max_length=M, truncation=True, padding="max_length", return_tensors="np")
    p64 = _poison_word(byte, np.int64)
    for i in range(len(raws)):
        if i % 2 == 0:
            assert lens[i] == -1 and (ids[i] == p64).all() and (mask[i] == p64).all(), raws[i][:40]
        else:
            g = (i // 2) % 4
            assert lens[i] == want["attention_mask"][g].sum()
            assert np.array_equal(ids[i], want["input_ids"][g]) and np.array_equal(mask[i], want["attention_mask"][g]), raws[i]
    h_ids, h_mask, h_lens = H.encode_host(d.ht, raws, M)
    n_long = 2 * len(TOO_LONG)
    assert np.array_equal(h_lens[n_long:], lens[n_long:]) and (h_lens[:n_long] > 0).all()      # the host entry does long pre-tokens


@pytest.mark.parametrize("b", [0, 1, 4, 5, 130])
def test_batch_shapes_mixing_ascii_and_non_ascii(device, b):
    """nothing to do, a lone wave, a full workgroup, a partial last workgroup, many workgroups"""
    d = device
    pool = d.ht.device_route(H.text_set(d.kind, 150) + [t for t in B.text_set(d.kind, 60) if t.isascii()])
    texts = [pool[(7 * i + b) % len(pool)] for i in range(b)]
    assert b < 5 or (any(t.isascii() for t in texts) and any(not t.isascii() for t in texts))
    raws = [t.encode("utf-8") for t in texts]
    ids, mask, lens = d.encode(raws, 24, poison.FF)
    if b == 0:
        assert (ids == -1).all() and (mask == -1).all() and (lens == -1).all()
        return
    h_ids, h_mask, h_lens = H.encode_host(d.ht, raws, 24, fill=-1)
    done = lens >= 0
    for i in np.nonzero(~done)[0]:
        assert lens[i] == -1 and B.longest_pretoken(d.hf, texts[i]) > KERNEL_WINDOW and (ids[i] == -1).all(), texts[i][:80]
    assert np.array_equal(lens[done], h_lens[done]) and np.array_equal(ids[done], h_ids[done]) and np.array_equal(mask[done], h_mask[done])


# ---- the wrapper -------------------------------------------------------------------------------------------------------------------
DEVICE_TEXTS = ["it’s “quoted” — dash… en–dash", "café naïve résumé", "emoji \U0001f600 here \U0001f44d", "Привет, мир! хорошо",
                "中文 mixed 文本 with 日本語", "€5 for the piñata – déjà vu", "we’ll see… they’ve gone", "great product works well",
                "12² and ١٢٣ and Ⅷ", "tail\u00a0", "über straße crème brûlée", "한국어 text \U0001f600\U0001f600!"]


def _host_cases(kind):
    special = "</s>" if kind != "modernbert" else "[SEP]"
    cases = ["has a %s literal and an é inside" % special, "é long " * 700, ("这个产品很糟糕浪费钱不要买" * 3)[:30]]
    assert len(cases[1].encode()) > 4096 and len(cases[2]) == 30
    return cases + (["e\u0301 combining mark"] if kind == "modernbert" else [])


@pytest.fixture(scope="module")
def wrapped(device):
    from adaptive_classifier.tokenizer import HipByteBPETokenizer
    tok = HipByteBPETokenizer(device.hf, device=device.dev, unicode=True)
    assert tok.unicode
    return tok


def _same(hf, tok, batch, M):
    want = hf(batch, max_length=M, truncation=True, padding=True, return_tensors="pt")
    got = tok(batch, max_length=M, truncation=True, padding=True, return_tensors="pt")
    assert set(got.keys()) == set(want.keys())
    for key in want.keys():
        g, w = got[key].cpu(), want[key]
        assert g.shape == w.shape, (key, g.shape, w.shape)
        bad = (g != w).any(dim=1).nonzero().flatten().tolist()
        assert not bad, (key, [(batch[i], g[i].tolist(), w[i].tolist()) for i in bad[:2]])
    assert got["input_ids"].is_cuda


@pytest.mark.parametrize("max_length", [512, 24, 8])
def test_wrapper_equals_transformers_on_the_full_list(device, wrapped, max_length, monkeypatch):
    poison.poisoned_empty(monkeypatch, poison.FF)
    texts = H.text_set(device.kind, 150) + EDGES + TOO_LONG + _host_cases(device.kind) + B.host_route_texts(device.kind)
    for lo in range(0, len(texts), 23):
        _same(device.hf, wrapped, texts[lo:lo + 23], max_length)


def test_routing_counts_are_exact(device, wrapped):
    """every text of DEVICE_TEXTS is tokenised on the device, and exactly the designed cases go to the wrapped tokenizer: a literal
    special token, a text over 4096 bytes, a 30-character CJK run (handed back by the kernel) and, under NFC, a combining mark"""
    assert all(len(w) <= 20 for t in DEVICE_TEXTS for w in t.split()) and not any("  " in t for t in DEVICE_TEXTS)
    before = (wrapped.device_texts, wrapped.host_texts)
    _same(device.hf, wrapped, DEVICE_TEXTS, 64)
    assert (wrapped.device_texts - before[0], wrapped.host_texts - before[1]) == (len(DEVICE_TEXTS), 0)
    cases = _host_cases(device.kind)
    batch = DEVICE_TEXTS[:5] + cases + DEVICE_TEXTS[5:]
    before = (wrapped.device_texts, wrapped.host_texts)
    _same(device.hf, wrapped, batch, 64)
    assert (wrapped.device_texts - before[0], wrapped.host_texts - before[1]) == (len(DEVICE_TEXTS), len(cases))
    if device.kind != "modernbert":                        # without a normalizer a combining mark is a character like any other
        before = (wrapped.device_texts, wrapped.host_texts)
        _same(device.hf, wrapped, ["e\u0301 combining mark"], 64)
        assert (wrapped.device_texts - before[0], wrapped.host_texts - before[1]) == (1, 0)


class _CallSpy:
    def __init__(self, monkeypatch, names):
        from adaptive_classifier import _native as nv
        self.calls = []
        L = nv.lib()
        for name in names:
            monkeypatch.setattr(L, name, self._wrap(name, getattr(L, name)))

    def _wrap(self, name, fn):
        def call(*args):
            self.calls.append(name)
            return fn(*args)
        return call


def test_an_all_ascii_batch_takes_the_ascii_entry_only(device, wrapped, monkeypatch):
    spy = _CallSpy(monkeypatch, ["ac_bpe_encode", "ac_bpe_utf8_encode"])
    _same(device.hf, wrapped, ["great product works well", "AWFUL... don't buy", ""], 32)
    assert spy.calls == ["ac_bpe_encode"]
    _same(device.hf, wrapped, ["great product works well", "café", ""], 32)
    assert spy.calls == ["ac_bpe_encode", "ac_bpe_utf8_encode"]


def test_without_the_switch_the_routing_is_what_it_was(device, monkeypatch):
    from adaptive_classifier.tokenizer import HipByteBPETokenizer
    tok = HipByteBPETokenizer(device.hf, device=device.dev)
    assert tok.unicode is False and tok._utf8 is False
    spy = _CallSpy(monkeypatch, ["ac_bpe_encode", "ac_bpe_utf8_encode"])
    batch = DEVICE_TEXTS + ["plain ascii text"]
    _same(device.hf, tok, batch, 64)
    n_ascii = sum(t.isascii() for t in batch)
    assert (tok.device_texts, tok.host_texts) == (n_ascii, len(batch) - n_ascii) and set(spy.calls) == {"ac_bpe_encode"}


def test_classifier_with_device_tokenizer_unicode(cuda_dev):
    """config["device_tokenizer_unicode"] reaches the byte-level BPE family: such a classifier tokenises non-ASCII texts on the
    device and predicts what the same classifier with the host tokenizer predicts (identical ids: only the launch paths differ)."""
    from adaptive_classifier import AdaptiveClassifier
    from adaptive_classifier.encoder import make_encoder
    from adaptive_classifier.tokenizer import HipByteBPETokenizer
    from oracle import bert_oracle
    hf = H.build_tokenizer("roberta")
    model = bert_oracle.make_roberta(128, 2, 2, 512, vocab=len(hf) + 8, max_pos=66, seed=4)
    enc = make_encoder(model, device=cuda_dev)
    a = AdaptiveClassifier("synthetic", device="cuda:0", config={"device_tokenizer_unicode": True}, encoder=enc, tokenizer=hf)
    b = AdaptiveClassifier("synthetic", device="cuda:0", config={"device_tokenizer": False}, encoder=enc, tokenizer=hf)
    assert isinstance(a.tokenizer, HipByteBPETokenizer) and a.tokenizer.unicode and b.tokenizer is hf
    texts = ["great product — works well \U0001f600", "love it… so much", "terrible waste of money – “awful”", "don’t buy, it’s bad",
             "it is fine, nothing special, café average", "average product, okay… привет"]
    labels = ["pos", "pos", "neg", "neg", "neu", "neu"]
    for c in (a, b):
        c.add_examples(texts, labels)
    for t in ["really “great” product \U0001f600!", "AWFUL… don’t buy", "okay I guess – café"]:
        pa, pb = a.predict(t, k=3), b.predict(t, k=3)
        assert [l for l, _ in pa] == [l for l, _ in pb]
        assert np.allclose([s for _, s in pa], [s for _, s in pb], atol=1e-6)
    oa, ob = a.predict_batch(texts, k=2), b.predict_batch(texts, k=2)
    assert [[l for l, _ in p] for p in oa] == [[l for l, _ in p] for p in ob]
    assert np.allclose([[s for _, s in p] for p in oa], [[s for _, s in p] for p in ob], atol=1e-6)
    assert a.tokenizer.device_texts > 0 and a.tokenizer.host_texts == 0
