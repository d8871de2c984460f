"""Unigram on UTF-8 text on the device: unigram_utf8_kernel (ac_unigram_encode_utf8) against the host entry over the same tables
(which test_unigram_unicode_cpu.py holds against the tokenizers library) -- batch shapes, deferred rows, the edges of its
64-end blocks, the vocabulary of exact ties -- and HipUnigramTokenizer(unicode=True) against the wrapped tokenizer with its
routing counts.  No tolerance: ids, mask and lengths are compared for equality."""
import ctypes

import numpy as np
import pytest
import torch

import unigram_unicode_helpers as H

pytestmark = pytest.mark.gpu

GPU_CONFIGS = [("full", "xlmr"), ("sparse", "deberta_lower"), ("sparse", "xlmr_legacy")]


def encode_device(dt, raws, max_length, dev):
    """ac_unigram_encode_utf8 over byte strings -> (ids, mask, lens) as numpy; untouched cells hold -7"""
    from adaptive_classifier import _native as nv
    blob, offs = H.pack(raws, 0)                           # no slack behind the last text
    b = len(raws)
    d_blob, d_offs = torch.from_numpy(blob).to(dev), torch.from_numpy(offs).to(dev)
    ids = torch.full((b, max_length), -7, dtype=torch.int64, device=dev)
    mask = torch.full((b, max_length), -7, dtype=torch.int64, device=dev)
    lens = torch.full((b,), -7, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        nv.check(nv.lib().ac_unigram_encode_utf8(nv.ptr(d_blob), nv.ptr(d_offs), b, ctypes.byref(dt[0]), ctypes.byref(dt[1]), max_length,
                                                 nv.ptr(ids), nv.ptr(mask), nv.ptr(lens), nv.stream_ptr(dev)), "ac_unigram_encode_utf8")
    return ids.cpu().numpy(), mask.cpu().numpy(), lens.cpu().numpy()


def device_tables(ht, dev):
    """(ac_unigram_vocab, ac_unigram_unicode, keep-alive) over device copies of the host tables"""
    from adaptive_classifier import tokenizer as tkz
    tv = [torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(dev) for a in ht.arrays]
    t = ht.tables
    tu = [torch.from_numpy(a).to(dev) for a in (t["page_of"].view(np.int16), t["entries"].view(np.int32), t["images"])]
    return (tkz.unigram_vocab_struct(ht.spec, [x.data_ptr() for x in tv], ht.slots, utf8=True),
            tkz.unigram_unicode_struct(t, [x.data_ptr() for x in tu]), tv + tu)


@pytest.fixture(scope="module", params=GPU_CONFIGS, ids=["-".join(c) for c in GPU_CONFIGS])
def setup(request, cuda_dev):
    hf = H.build_tokenizer(*request.param)
    ht = H.HostTables(hf)
    return request.param, hf, ht, device_tables(ht, cuda_dev)


def _same(got, want, what):
    for g, w, name in zip(got, want, ("ids", "mask", "lens")):
        bad = np.nonzero((g != w).reshape(len(g), -1).any(1))[0]
        assert len(bad) == 0, (what, name, bad[:5].tolist(), g[bad[:2]].tolist()[:2], w[bad[:2]].tolist()[:2])


def _raws(ht):
    texts = [t for t in H.FIXED + H.random_texts(160, 5) if not any(sp in t for sp in ht.specials)]
    return H.raw(texts) + [p + bad for bad in H.MALFORMED for p in (b"", "ab \u00e9".encode())] \
        + H.raw(["\ufdfa" * 155 + "a" * r for r in (3, 4, 5)]) + [b"a " * 2048 + b"b", b"a\xc3", b"\xa9b"]


@pytest.mark.parametrize("max_length", [2, 8])
def test_kernel_equals_host_entry(setup, cuda_dev, max_length):
    """About 330 texts -- the fixed cases with the block-edge words, random ones (a third with a word over 64 bytes), texts with
    a host-only code point, every malformed form, the buffer edge, an over-long one -- in batches of 130 (many workgroups), 5 (a
    partly filled last workgroup), 4 (one full workgroup) and 1 (a lone wave): the same ids, mask and lengths as the host entry,
    the same rows deferred and their cells untouched."""
    config, hf, ht, dt = setup
    raws = _raws(ht)
    assert 300 <= len(raws) <= 380
    want = H.encode_host(ht, raws, max_length)
    deferred = want[2] < 0
    assert int(deferred.sum()) >= 2 * len(H.MALFORMED) + 3 and (want[0][deferred] == -7).all() and (want[1][deferred] == -7).all()
    n_long = sum(1 for r, d in zip(raws, deferred) if not d and max((len(w) for w in r.split()), default=0) >= 64)
    assert n_long >= 60                                     # the block schedule runs, not only the windows
    for b, starts in ((130, range(0, len(raws), 130)), (5, (0, 45, 131, len(raws) - 5)), (4, (0, 60, len(raws) - 4)),
                      (1, (0, 41, 42, 43, 200, len(raws) - 1))):
        for lo in starts:
            got = encode_device(dt, raws[lo:lo + b], max_length, cuda_dev)
            _same(got, [w[lo:lo + b] for w in want], (config, max_length, b, lo))


def test_kernel_equals_host_entry_untruncated(setup, cuda_dev):
    """The same texts at max_length 512: every piece of every word is compared, long words included."""
    config, hf, ht, dt = setup
    raws = _raws(ht)
    want = H.encode_host(ht, raws, 512)
    for lo in range(0, len(raws), 67):
        _same(encode_device(dt, raws[lo:lo + 67], 512, cuda_dev), [w[lo:lo + 67] for w in want], (config, lo))


def test_block_edges(setup, cuda_dev):
    """Words of 63 ... 301 bytes (metaspace included) of 2- and 3-byte characters, so that the edge between two blocks of 64
    ends falls behind, one byte into and two bytes into a character; the vocabulary's longest multi-byte piece across the edge;
    a 2-, 3- and 4-byte character that starts at byte 61, 62 and 63 of a 64-byte chunk of the text (pass 1); ~100 and ~1000
    bytes without a space; each alone, between other words and at max_length 24: the kernel, the host entry and the wrapped
    tokenizer agree."""
    config, hf, ht, dt = setup
    word, k = H.straddling_word(ht.spec["vocab"])
    assert len(word.encode()) + 1 >= H.REACH + 1 and k >= 6
    texts = list(H.EDGE_WORDS) + ["lead " + w + " tail" for w in H.EDGE_WORDS] + [word, "x " + word + " y", word + word]
    texts += [H.CJK_99, H.LONG_CJK, H.CJK_99 + " " + H.LONG_CJK, "\u00e9" * 2048, "\u4e2d" * 1365 + "a", "a " * 2048]
    filler = "ab cd, " * 40
    for chunk in (0, 64, 192):
        for at in (61, 62, 63):
            for ch in ("\u00e9", "\u4e2d", "\ud55c", "\U0001f600", "\U00020000", "\u0130"):
                texts.append(filler[:chunk + at] + ch + "x \u00e9\u4e2d tail")
                texts.append(filler[:chunk + at - 1] + " " + ch * 30 + " end")
    texts = [t for t in texts if ht.eligible(t) and ht.fits(t)]
    assert len(texts) >= 120
    for M in (512, 24):
        want = H.reference(hf, texts, M)
        host = H.encode_host(ht, texts, M)
        _same(host, want, (config, M, "host entry vs tokenizers"))
        _same(encode_device(dt, H.raw(texts), M, cuda_dev), host, (config, M, "kernel vs host entry"))


def test_exact_ties_on_the_device(cuda_dev):
    """The vocabulary of exact ties over multi-byte characters: the kernel resolves them as the library does, fuses a 3-byte and
    a 2-byte unknown into one unk_id, also across a block edge."""
    hf = H.tie_tokenizer()
    ht = H.HostTables(hf)
    dt = device_tables(ht, cuda_dev)
    texts = [t for t, _ in H.TIE_ROWS] + ["éa 文ß a中éa", " ".join(t for t, _ in H.TIE_ROWS),
                                          "文" * 70 + "éa", "éa" * 40 + "文ß" * 30 + "a中"]
    for M in (64, 4):
        want = H.reference(hf, texts, M)
        _same(H.encode_host(ht, texts, M), want, (M, "host entry vs tokenizers"))
        _same(encode_device(dt, H.raw(texts), M, cuda_dev), want, (M, "kernel vs tokenizers"))


def test_device_tokenizer_unicode_equals_transformers(setup, cuda_dev):
    """HipUnigramTokenizer(hf, unicode=True) on mixed batches: every returned key equal to the wrapped tokenizer's and on the
    device; device_texts / host_texts count the eligible / ineligible texts (a text whose normalised form outgrows the buffer is
    deferred by the kernel and counts as a host text).  (Fails on a build without the `unicode` argument.)"""
    from adaptive_classifier.tokenizer import HipUnigramTokenizer
    config, hf, ht, _ = setup
    tok = HipUnigramTokenizer(hf, device=cuda_dev, unicode=True)
    assert tok.unicode and tok._utf8 and tok._defers
    ineligible = ["has a %s literal, caf\u00e9" % hf.sep_token, "long \u00e9 " * 1200, "combining e\u0301 mark"]
    import unigram_helpers as UH
    pool = [t for t in H.FIXED + H.random_texts(80, 9) if ht.eligible(t) and ht.fits(t) and (not t.isascii() or UH.eligible(t, ht.specials))]
    batches = [pool[lo:lo + 23] + [ineligible[i % 3], ineligible[(i + 1) % 3]] for i, lo in enumerate(range(0, len(pool), 23))]
    batches.append(["plain ascii only", "second ASCII text, with punctuation!"])             # the ASCII fast path, existing entry
    want_dev = want_host = 0
    for batch in batches:
        for M in (64, 8):
            want = hf(batch, max_length=M, truncation=True, padding=True, return_tensors="pt")
            got = tok(batch, max_length=M, truncation=True, padding=True, return_tensors="pt")
            assert set(got) == set(want)
            for key in got:
                g, w = got[key].cpu(), want[key]
                assert got[key].is_cuda and g.shape == w.shape, (key, g.shape, w.shape)
                bad = (g != w).any(dim=1).nonzero().flatten().tolist()
                assert not bad, (key, [(batch[i][:40], g[i].tolist()[:12], w[i].tolist()[:12]) for i in bad[:2]])
            want_host += sum(1 for t in batch if t in ineligible)
            want_dev += sum(1 for t in batch if t not in ineligible)
    assert (tok.device_texts, tok.host_texts) == (want_dev, want_host) and want_host >= 2 * (len(batches) - 1)
    assert sum(1 for b in batches for t in b if t not in ineligible and not t.isascii()) > 60   # the non-ASCII texts ran on the device
    assert sum(1 for b in batches for t in b if t not in ineligible and H.longest_word_bytes(t) > 64) > 15
    # without the option the same tokenizer keeps the host route for every non-ASCII text
    plain = HipUnigramTokenizer(hf, device=cuda_dev)
    plain(["caf\u00e9", "\u4e2d\u6587", "ascii"], max_length=8)
    assert not plain.unicode and (plain.device_texts, plain.host_texts) == (1, 2)


def test_rejected_tables_and_long_pieces_keep_ascii_routing(cuda_dev):
    """Tables that fail the probe guard (one image changed) are not used, and a vocabulary with a piece beyond the kernel's reach
    keeps the route off: `unicode` reads False and non-ASCII texts take the host route."""
    from adaptive_classifier import tokenizer as tkz
    hf = H.build_tokenizer("full", "xlmr")
    t = tkz.build_unigram_unicode_tables(hf)
    bad = dict(t, images=t["images"].copy())
    bad["images"][int(t["entries"][int(t["page_of"][0x21]), 0x2B]) >> 8] ^= 1             # the image of U+212B
    key, = [k for k, v in tkz._UNI_UNICODE_CACHE.items() if v is t]
    tkz._UNI_UNICODE_CACHE[key] = bad
    try:
        tok = tkz.HipUnigramTokenizer(hf, device=cuda_dev, unicode=True)
    finally:
        tkz._UNI_UNICODE_CACHE[key] = t
    assert not tok.unicode and not tok._utf8
    batch = ["caf\u00e9", "plain"]
    got = tok(batch, max_length=8)
    want = hf(batch, max_length=8, truncation=True, padding=True, return_tensors="pt")
    assert torch.equal(got["input_ids"].cpu(), want["input_ids"]) and (tok.device_texts, tok.host_texts) == (1, 1)
    import unigram_helpers as UH
    far = UH.legacy_tokenizer(UH._xlmr_vocab(H.trained_pieces("sparse")) + [("中" * 22, -20.0)])      # a piece of 66 bytes
    tok = tkz.HipUnigramTokenizer(far, device=cuda_dev, unicode=True)
    assert not tok.unicode
    tok(batch, max_length=8)
    assert (tok.device_texts, tok.host_texts) == (1, 1)
    # maybe_device_tokenizer passes the flag on
    assert tkz.maybe_device_tokenizer(hf, cuda_dev, unicode=True).unicode and not tkz.maybe_device_tokenizer(hf, cuda_dev).unicode
