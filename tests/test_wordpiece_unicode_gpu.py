"""WordPiece on UTF-8 text on the device: wordpiece_utf8_kernel (ac_wordpiece_encode_utf8) against the host entry over the same
tables (which test_wordpiece_unicode_cpu.py holds against the tokenizers library), the lane-chunk edges of its first two
passes, HipWordPieceTokenizer(unicode=True) against the wrapped tokenizer with its routing counts, and the classifier option.
No tolerance: ids, mask and lengths are compared for equality."""
import ctypes

import numpy as np
import pytest
import torch

import wordpiece_helpers as H

pytestmark = pytest.mark.gpu


def encode_device(ht, dt, raws, max_length, dev):
    """ac_wordpiece_encode_utf8 over byte strings -> (ids, mask, lens) as numpy; untouched cells hold -7"""
    from adaptive_classifier import _native as nv
    blob, offs = H.pack(raws, 0)                           # no slack behind the last text
    b = len(raws)
    d_blob, d_offs = torch.from_numpy(blob).to(dev), torch.from_numpy(offs).to(dev)
    ids = torch.full((b, max_length), -7, dtype=torch.int64, device=dev)
    mask = torch.full((b, max_length), -7, dtype=torch.int64, device=dev)
    lens = torch.full((b,), -7, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        nv.check(nv.lib().ac_wordpiece_encode_utf8(nv.ptr(d_blob), nv.ptr(d_offs), b, ctypes.byref(dt[0]), ctypes.byref(dt[1]), max_length,
                                                   nv.ptr(ids), nv.ptr(mask), nv.ptr(lens), nv.stream_ptr(dev)), "ac_wordpiece_encode_utf8")
    return ids.cpu().numpy(), mask.cpu().numpy(), lens.cpu().numpy()


def device_tables(ht, dev):
    """(ac_wordpiece_vocab, ac_wordpiece_unicode, keep-alive) over device copies of the host tables"""
    from adaptive_classifier import tokenizer as tkz
    keys, offs, ids, lens, blob = ht.arrays
    tv = [torch.from_numpy(a).to(dev) for a in (keys.view(np.int64), offs.view(np.int32), ids, lens.view(np.int16), blob)]
    t = ht.tables
    tu = [torch.from_numpy(a).to(dev) for a in (t["page_of"].view(np.int16), t["entries"].view(np.int32), t["images"])]
    return (tkz.wordpiece_vocab_struct(ht.hf, ht.vocab, ht.lower, [x.data_ptr() for x in tv], ht.slots, ht.max_piece),
            tkz.wordpiece_unicode_struct(t, [x.data_ptr() for x in tu]), tv + tu)


@pytest.fixture(scope="module", params=H.CONFIGS)
def setup(request, cuda_dev):
    hf = H.build_tokenizer(request.param)
    ht = H.HostTables(hf)
    return request.param, hf, ht, device_tables(ht, cuda_dev)


def _same(got, want, what):
    for g, w, name in zip(got, want, ("ids", "mask", "lens")):
        bad = np.nonzero((g != w).reshape(len(g), -1).any(1))[0]
        assert len(bad) == 0, (what, name, bad[:5].tolist(), g[bad[:2]].tolist()[:2], w[bad[:2]].tolist()[:2])


def test_kernel_equals_host_entry(setup, cuda_dev):
    """About 300 texts -- the fixed cases, random ones, texts with a host-only code point, every malformed form, the buffer
    edge, an over-long one -- in batches of 67, 5 (a partly filled workgroup) and 1: the same ids, mask and lengths as the host
    entry, -1 rows and their untouched cells included."""
    kind, hf, ht, dt = setup
    raws = H.raw(H.FIXED + H.random_texts(220, 5)) + [p + bad for bad in H.MALFORMED for p in (b"", "ab é".encode())] \
        + H.raw(["한 " * 819 + "a" * r for r in (1, 2, 3)]) + [b"a " * 2048, b"a " * 2048 + b"b", b"a\xc3", b"\xa9b"]
    assert 280 <= len(raws) <= 320
    seen_not_done = 0
    for M in (512, 16, 2):
        want = H.encode_host(ht, raws, M)
        seen_not_done = int((want[2] < 0).sum())
        for b, starts in ((67, range(0, len(raws), 67)), (5, (0, 5, 233, len(raws) - 5)), (1, (0, 6, 7, 240, len(raws) - 1))):
            for lo in starts:
                got = encode_device(ht, dt, raws[lo:lo + b], M, cuda_dev)
                _same(got, [w[lo:lo + b] for w in want], (kind, M, b, lo))
    assert seen_not_done >= 2 * len(H.MALFORMED) + 3       # the malformed rows, the over-long one, the cut pair
    if kind == "uncased":
        assert seen_not_done >= 2 * len(H.MALFORMED) + 5   # ... the buffer overflow and the host-only fixed case


def test_lane_chunk_edges(setup, cuda_dev):
    """A 2-, 3- and 4-byte character that starts at byte 61, 62 and 63 of a 64-byte chunk (the lead lane reads its continuation
    bytes from the next chunk's bytes), an image of three code points whose output straddles a chunk of the normalised buffer,
    and a word that straddles one: the kernel, the host entry and the wrapped tokenizer agree."""
    kind, hf, ht, dt = setup
    filler = "ab cd, " * 40
    texts = []
    for chunk in (0, 64, 192):
        for at in (61, 62, 63):
            for ch in ("é", "中", "한", "\U0001f600", "\U0001d163", "İ"):
                texts.append(filler[:chunk + at] + ch + "x é中 tail")                  # the character inside / in front of a word
                assert texts[-1].encode()[chunk + at:].startswith(ch.encode()) and (chunk + at) % 64 == at
                texts.append(filler[:chunk + at - 1] + " " + ch * 3 + " end")
            texts.append(filler[:chunk + at - 5] + " internationalisé" + "é" * 20 + " end")       # a word across the edge
    texts.append("한" * 30 + " " + "한국어" * 11)                                           # 9-byte images across output chunks
    assert all(ht.eligible(t) for t in texts)
    for M in (512, 24):
        want = H.reference(hf, texts, M)
        host = H.encode_host(ht, texts, M)
        _same(host, want, (kind, M, "host entry vs tokenizers"))
        _same(encode_device(ht, dt, H.raw(texts), M, cuda_dev), host, (kind, M, "kernel vs host entry"))


def test_device_tokenizer_unicode_equals_transformers(setup, cuda_dev):
    """HipWordPieceTokenizer(hf, unicode=True) on mixed batches: every returned key equal to the wrapped tokenizer's and on the
    device; device_texts / host_texts count exactly the eligible / ineligible texts.  (Fails on a build without the `unicode`
    argument.)"""
    from adaptive_classifier.tokenizer import HipWordPieceTokenizer
    kind, hf, ht, _ = setup
    tok = HipWordPieceTokenizer(hf, device=cuda_dev, unicode=True)
    assert tok.unicode and tok._defers
    ineligible = ["has a [SEP] literal, café", "long é " * 1200, "a\U0001d165b" if kind == "uncased" else "second [MASK] 中文"]
    pool = H.FIXED[:len(H.FIXED) - len(H.HOST_ONLY_FIXED)] + H.random_texts(60, 9) + H.ascii_texts()[:12]
    pool = [t for t in pool if ht.eligible(t)]
    batches = [pool[lo:lo + 23] + [ineligible[i % 3], ineligible[(i + 1) % 3]] for i, lo in enumerate(range(0, len(pool), 23))]
    batches.append(["plain ascii only", "second ASCII text, with punctuation!"])             # the ASCII fast path, existing entry
    want_dev = want_host = 0
    for batch in batches:
        for M in (64, 8):
            want = hf(batch, max_length=M, truncation=True, padding=True, return_tensors="pt")
            got = tok(batch, max_length=M, truncation=True, padding=True, return_tensors="pt")
            assert set(got) == {"input_ids", "token_type_ids", "attention_mask"}
            for key in got:
                g, w = got[key].cpu(), want[key]
                assert got[key].is_cuda and g.shape == w.shape, (key, g.shape, w.shape)
                bad = (g != w).any(dim=1).nonzero().flatten().tolist()
                assert not bad, (key, [(batch[i][:40], g[i].tolist()[:12], w[i].tolist()[:12]) for i in bad[:2]])
            want_host += sum(1 for t in batch if not ht.eligible(t))
            want_dev += sum(1 for t in batch if ht.eligible(t))
    assert (tok.device_texts, tok.host_texts) == (want_dev, want_host) and want_host >= 2 * (len(batches) - 1)
    assert sum(1 for b in batches for t in b if ht.eligible(t) and not t.isascii()) > 40     # the non-ASCII texts ran on the device
    # without the option the same tokenizer keeps the host route for every non-ASCII text
    plain = HipWordPieceTokenizer(hf, device=cuda_dev)
    plain(["café", "中文", "ascii"], max_length=8)
    assert not plain.unicode and (plain.device_texts, plain.host_texts) == (1, 2)


def test_rejected_tables_fall_back_to_ascii_routing(cuda_dev):
    """Tables that fail the probe guard (one image changed) are not used: the tokenizer keeps the ASCII-only routing."""
    from adaptive_classifier import tokenizer as tkz
    hf = H.build_tokenizer("cased")
    t = tkz.build_wordpiece_unicode_tables(hf)
    bad = dict(t, images=t["images"].copy())
    bad["images"][int(t["entries"][int(t["page_of"][0]), ord("\t")]) >> 9] = ord("x")
    key, = [k for k, v in tkz._WP_UNICODE_CACHE.items() if v is t]
    tkz._WP_UNICODE_CACHE[key] = bad
    try:
        tok = tkz.HipWordPieceTokenizer(hf, device=cuda_dev, unicode=True)
    finally:
        tkz._WP_UNICODE_CACHE[key] = t
    assert not tok.unicode and not tok._defers
    batch = ["café", "plain"]
    got = tok(batch, max_length=8)
    want = hf(batch, max_length=8, truncation=True, padding=True, return_tensors="pt")
    assert torch.equal(got["input_ids"].cpu(), want["input_ids"]) and (tok.device_texts, tok.host_texts) == (1, 1)


def test_classifier_option(cuda_dev):
    """config={"device_tokenizer_unicode": True}: accented, CJK and Cyrillic texts are tokenised on the device and predicted as
    the same classifier with the host tokenizer predicts them; a default classifier still routes an accented text to the host."""
    from adaptive_classifier import AdaptiveClassifier
    from adaptive_classifier.encoder import HipBertEncoder
    from adaptive_classifier.tokenizer import HipWordPieceTokenizer
    from helpers import small_bert
    hf = H.build_tokenizer("uncased")
    enc = HipBertEncoder(small_bert(vocab=len(H.vocab()) + 8), device=cuda_dev)
    a = AdaptiveClassifier("synthetic", device="cuda:0", config={"device_tokenizer_unicode": True}, encoder=enc, tokenizer=hf)
    b = AdaptiveClassifier("synthetic", device="cuda:0", config={"device_tokenizer": False}, encoder=enc, tokenizer=hf)
    c = AdaptiveClassifier("synthetic", device="cuda:0", encoder=enc, tokenizer=hf)
    assert isinstance(a.tokenizer, HipWordPieceTokenizer) and a.tokenizer.unicode and b.tokenizer is hf
    assert isinstance(c.tokenizer, HipWordPieceTokenizer) and not c.tokenizer.unicode
    texts = ["très bon produit, génial", "j'adore ça énormément", "这个产品很糟糕", "浪费钱不要买",
             "Обычный товар, ничего особенного", "средне, нормально"]
    labels = ["pos", "pos", "neg", "neg", "neu", "neu"]
    for clf in (a, b, c):
        clf.add_examples(texts, labels)
    for t in ["vraiment génial ce produit!", "很糟糕 不要买", "НОРМАЛЬНО, ничего"]:
        pa, pb = a.predict(t, k=3), b.predict(t, k=3)
        assert [l for l, _ in pa] == [l for l, _ in pb]
        assert np.allclose([s for _, s in pa], [s for _, s in pb], atol=1e-6)
    oa, ob = a.predict_batch(texts, k=2), b.predict_batch(texts, k=2)
    assert [[l for l, _ in p] for p in oa] == [[l for l, _ in p] for p in ob]
    assert a.tokenizer.host_texts == 0 and a.tokenizer.device_texts > 0
    before = c.tokenizer.host_texts
    c.predict("très génial", k=3)
    assert c.tokenizer.host_texts == before + 1
