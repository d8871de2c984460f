"""On-device Unigram tokenisation (ac_unigram_encode behind HipUnigramTokenizer) against the wrapped transformers tokenizer:
identical keys, shapes, input_ids, attention_mask (and token_type_ids) for the classifier's call in the pipelines of
unigram_helpers; the kernel against ac_unigram_encode_host on the same buffers, at the window's edges and on the vocabulary of
exact ties; and DeBERTa / XLM-R classifiers that tokenise on the device against the same classifiers with the host tokenizer."""
import ctypes

import numpy as np
import pytest
import torch

import unigram_helpers as H

pytestmark = pytest.mark.gpu

KERNEL_WINDOW = 64          # bytes of the longest word (metaspace included) the kernel takes; longer ones come back as not done
WRAPPER_CONFIGS = [("sparse", p) for p in H.PIPELINES] + [("full", "deberta")]


def text_set(hf, n_random=150):
    return H.FIXED + H.host_route_texts(hf) + H.random_texts(n_random, 11)


@pytest.fixture(scope="module", params=WRAPPER_CONFIGS, ids=["-".join(c) for c in WRAPPER_CONFIGS])
def setup(request, cuda_dev):
    from adaptive_classifier.tokenizer import HipUnigramTokenizer
    hf = H.build_tokenizer(*request.param)
    return request.param, hf, HipUnigramTokenizer(hf, device=cuda_dev), text_set(hf)


def _tokens_before(text, word_bytes):
    """A lower bound of the pieces in front of the first word of more than word_bytes bytes: one per earlier word."""
    n = 0
    for w in text.split():
        if len(w) + 1 > word_bytes:
            return n
        n += 1
    return None


@pytest.mark.parametrize("max_length", [512, 64, 24, 8])
def test_device_unigram_equals_transformers(setup, max_length):
    (which, pipeline), hf, dev_tok, texts = setup
    before = (dev_tok.device_texts, dev_tok.host_texts)
    for lo in range(0, len(texts), 17):                     # several batches: different padded lengths
        batch = texts[lo:lo + 17]
        want = hf(batch, max_length=max_length, truncation=True, padding=True, return_tensors="pt")
        got = dev_tok(batch, max_length=max_length, truncation=True, padding=True, return_tensors="pt")
        assert set(got.keys()) == set(want.keys())
        assert ("token_type_ids" in got) == pipeline.startswith("deberta")
        for key in want.keys():
            g, w = got[key].cpu(), want[key]
            assert g.shape == w.shape, (key, g.shape, w.shape)
            bad = (g != w).any(dim=1).nonzero().flatten().tolist()
            assert not bad, (key, [(batch[i], g[i].tolist(), w[i].tolist()) for i in bad[:2]])
        assert got["input_ids"].is_cuda
    on_device, on_host = dev_tok.device_texts - before[0], dev_tok.host_texts - before[1]
    assert len(texts) == 181 and on_device + on_host == len(texts)
    routed = [t for t in texts if not H.eligible(t, dev_tok.specials)]      # control bytes, non-ASCII, literal special, over length
    assert set(H.host_route_texts(hf)) <= set(routed) and len(texts) - len(routed) >= 130
    # ... and nothing else goes to the host, but texts the kernel may hand back: a word beyond its window, unless truncation
    # ends the text before the kernel reaches it
    long_words = [t for t in texts if t not in routed and H.longest_word(t) > KERNEL_WINDOW]
    assert sorted(long_words) == sorted(["x" * 300, "q" * 4096])
    must_defer = [t for t in long_words if _tokens_before(t, KERNEL_WINDOW) < max_length - 2]
    assert len(routed) + len(must_defer) <= on_host <= len(routed) + len(long_words)
    assert on_device >= 130
    print(f"[unigram] {which}/{pipeline} M={max_length}: device {on_device}, host {on_host} ({len(routed)} routed, "
          f"{on_host - len(routed)} deferred)")


def _run_kernel(hv, texts, max_length, dev):
    from adaptive_classifier import _native as nv
    from adaptive_classifier.tokenizer import unigram_vocab_struct
    b = len(texts)
    blob, offs = H.pack(texts)
    d_arrays = [torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(dev) for a in hv.arrays]
    vocab = unigram_vocab_struct(hv.spec, [t.data_ptr() for t in d_arrays], hv.slots)
    d_blob, d_offs = torch.from_numpy(blob).to(dev), torch.from_numpy(offs).to(dev)
    ids = torch.full((b, max_length), -7, dtype=torch.int64, device=dev)
    mask = torch.full((b, max_length), -7, dtype=torch.int64, device=dev)
    lens = torch.full((b,), -7, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        nv.check(nv.lib().ac_unigram_encode(nv.ptr(d_blob), nv.ptr(d_offs), b, ctypes.byref(vocab), max_length, nv.ptr(ids),
                                            nv.ptr(mask), nv.ptr(lens), nv.stream_ptr(dev)), "ac_unigram_encode")
    torch.cuda.synchronize()
    return ids.cpu().numpy(), mask.cpu().numpy(), lens.cpu().numpy()


def _assert_kernel_equals_host(hv, texts, max_length, dev, may_defer=True):
    want_ids, want_mask, want_lens = H.encode_host(hv, texts, max_length)
    ids, mask, lens = _run_kernel(hv, texts, max_length, dev)
    done = lens >= 0
    for i in np.nonzero(~done)[0]:
        assert may_defer and lens[i] == -1 and H.longest_word(texts[i]) > KERNEL_WINDOW, texts[i][:80]
        assert (mask[i] == -7).all() and ids[i, 0] == -7                  # never finished: no specials, no padding, no mask
    bad = [i for i in np.nonzero(done)[0] if lens[i] != want_lens[i] or not np.array_equal(ids[i], want_ids[i])
           or not np.array_equal(mask[i], want_mask[i])]
    assert not bad, [(texts[i][:70], ids[i][:12].tolist(), want_ids[i][:12].tolist()) for i in bad[:3]]
    return done


@pytest.mark.parametrize("b", [1, 4, 5, 130])
@pytest.mark.parametrize("max_length", [2, 8])
def test_kernel_equals_host_encode(b, max_length, cuda_dev):
    """ac_unigram_encode against ac_unigram_encode_host on the same buffers: a lone wave, a full workgroup, a partial last
    workgroup, many workgroups.  A text the kernel reports as not done must hold a word longer than its window."""
    hf = H.build_tokenizer("sparse", "xlmr_legacy")
    hv = H.HostVocab(hf)
    pool = [t for t in text_set(hf) if H.eligible(t)]
    texts = [pool[(7 * i + b) % len(pool)] for i in range(b)]
    _assert_kernel_equals_host(hv, texts, max_length, cuda_dev)


@pytest.mark.parametrize("which,pipeline", [("full", "deberta"), ("sparse", "xlmr_legacy"), ("sparse", "deberta_lower")])
def test_window_edges(which, pipeline, cuda_dev):
    """Hand-built texts around the 64-byte window: words of exactly 63, 64 and 65 bytes with their metaspace, words that end
    exactly on a window boundary, 4096 bytes of one-character words, whitespace only, a trailing space behind a full window."""
    hv = H.HostVocab(H.build_tokenizer(which, pipeline))
    w = lambda n: ("tokenization" * 6)[:n]                                               # noqa: E731
    fit = ["the " * 15 + "abc", "the " * 16, "the " * 15 + "abcd", "ab " * 21 + w(62), w(31) + " " + w(31) + " " + w(63) + " ok",
           "a " * 2048, "Zz " * 1365, " " * 64, " " * 63 + "a", " " * 64 + "a", " ", "", "\n\t\r ", w(63) + " ", w(62) + "  x",
           w(20) + " " * 50 + w(20), "it's " + w(58) + " " + w(5), "a" * 63 + " " + "b" * 63 + " " + "c" * 63]
    done = _assert_kernel_equals_host(hv, fit, 512, cuda_dev, may_defer=False)
    assert done.all()
    # a word of 62 / 63 bytes is 63 / 64 with its metaspace and fits; 64 bytes make 65 and the text is not done -- wherever
    # the word stands, unless truncation ends the text in front of it
    edge = [w(62), w(63), w(64), "ok " + w(64), w(64) + " ok", "a b c " + w(300) + " d", " " + w(63), " " + w(64)]
    done = _assert_kernel_equals_host(hv, edge, 512, cuda_dev)
    assert done.tolist() == [True, True, False, False, False, False, True, False]
    done = _assert_kernel_equals_host(hv, edge, 4, cuda_dev)                              # room for two pieces
    assert done[0] and done[1] and not done[2] and not done[4] and not done[7]


def test_exact_ties_on_the_device(cuda_dev):
    """The fp64 adds happen in start-ascending order with the strict-greater rule: the hand-made vocabulary's six rows."""
    hf = H.tie_tokenizer()
    hv = H.HostVocab(hf)
    texts = [t for t, _ in H.TIE_ROWS] + ["X Y", " ".join(t for t, _ in H.TIE_ROWS)]
    ids, _, lens = _run_kernel(hv, texts, 32, cuda_dev)
    for i, (text, pieces) in enumerate(H.TIE_ROWS):
        assert hf.convert_ids_to_tokens(ids[i, 1:lens[i] - 1].tolist()) == pieces, text
    want = hf(texts, max_length=32, truncation=True, padding="max_length", return_tensors="np")["input_ids"]
    assert np.array_equal(ids, want)
    _assert_kernel_equals_host(hv, texts, 32, cuda_dev, may_defer=False)


QUERIES = ["really great product!", "AWFUL... don't buy", "okay I guess"]
TEXTS = ["great product works well", "love it so much", "terrible waste of money", "awful do not buy",
         "it is fine nothing special", "average product okay"]
LABELS = ["pos", "pos", "neg", "neg", "neu", "neu"]


def _model(family, vocab):
    if family == "deberta":
        import encoder_deberta_ref as D
        import encoder_ref as R
        return D.build_model(D.deberta_config(128, R.L, 2, 512, 64, vocab=vocab), "peaked", seed=0)
    from oracle import bert_oracle
    return bert_oracle.make_roberta(128, 2, 2, 512, vocab=vocab, max_pos=66, seed=4, model_type="xlm-roberta")


@pytest.mark.parametrize("family,pipeline", [("deberta", "deberta"), ("xlm-roberta", "xlmr")])
def test_classifier_uses_the_device_unigram_tokenizer(family, pipeline, cuda_dev):
    """A classifier built with a DeBERTa / XLM-R style tokenizer tokenises on the device and predicts what the same classifier
    with the host tokenizer predicts (identical ids: only the launch paths differ)."""
    from adaptive_classifier import AdaptiveClassifier
    from adaptive_classifier.encoder import make_encoder
    from adaptive_classifier.tokenizer import HipUnigramTokenizer
    hf = H.build_tokenizer("full", pipeline)
    enc = make_encoder(_model(family, len(hf) + 8), device=cuda_dev)
    a = AdaptiveClassifier("synthetic", device="cuda:0", encoder=enc, tokenizer=hf)
    b = AdaptiveClassifier("synthetic", device="cuda:0", config={"device_tokenizer": False}, encoder=enc, tokenizer=hf)
    assert isinstance(a.tokenizer, HipUnigramTokenizer) and b.tokenizer is hf
    for c in (a, b):
        c.add_examples(TEXTS, LABELS)
    for t in QUERIES:
        pa, pb = a.predict(t, k=3), b.predict(t, k=3)
        assert [l for l, _ in pa] == [l for l, _ in pb]
        assert np.allclose([s for _, s in pa], [s for _, s in pb], atol=1e-6)
    oa, ob = a.predict_batch(TEXTS, k=2), b.predict_batch(TEXTS, k=2)
    assert [[l for l, _ in p] for p in oa] == [[l for l, _ in p] for p in ob]
    assert np.allclose([[s for _, s in p] for p in oa], [[s for _, s in p] for p in ob], atol=1e-6)
    assert a.tokenizer.device_texts > 0 and a.tokenizer.host_texts == 0
