"""On-device byte-level BPE (ac_bpe_encode behind HipByteBPETokenizer) against the wrapped transformers tokenizer: identical
keys, shapes, input_ids and attention_mask for the classifier's call, in the three configurations of bpe_helpers; the
kernel against ac_bpe_encode_host on the same buffers; and a classifier that tokenises on the device against the same
classifier with the host tokenizer."""
import ctypes

import numpy as np
import pytest
import torch

import bpe_helpers as H

pytestmark = pytest.mark.gpu

KERNEL_WINDOW = 64          # bytes of the longest pre-token the kernel takes; longer ones come back as not done (lens -1)


@pytest.fixture(scope="module", params=H.CONFIGS)
def setup(request, cuda_dev):
    from adaptive_classifier.tokenizer import HipByteBPETokenizer
    hf = H.build_tokenizer(request.param)
    return request.param, hf, HipByteBPETokenizer(hf, device=cuda_dev), H.text_set(request.param, 150)


@pytest.mark.parametrize("max_length", [512, 64, 24, 8])
def test_device_bpe_equals_transformers(setup, max_length):
    kind, hf, dev_tok, texts = setup
    before = (dev_tok.device_texts, dev_tok.host_texts)
    for lo in range(0, len(texts), 17):                     # several batches: different padded lengths
        batch = texts[lo:lo + 17]
        want = hf(batch, max_length=max_length, truncation=True, padding=True, return_tensors="pt")
        got = dev_tok(batch, max_length=max_length, truncation=True, padding=True, return_tensors="pt")
        assert set(got.keys()) == set(want.keys())
        for key in want.keys():
            g, w = got[key].cpu(), want[key]
            assert g.shape == w.shape, (key, g.shape, w.shape)
            bad = (g != w).any(dim=1).nonzero().flatten().tolist()
            assert not bad, (key, [(batch[i], g[i].tolist(), w[i].tolist()) for i in bad[:2]])
        assert got["input_ids"].is_cuda
    on_device, on_host = dev_tok.device_texts - before[0], dev_tok.host_texts - before[1]
    assert on_device + on_host == len(texts) and on_device > 0
    routed = H.host_route_texts(kind)
    if kind == "modernbert":                                # the added token of two spaces: those texts take the host route
        routed = routed + [t for t in texts if "  " in t and t not in routed]
    assert on_host >= len(routed)
    # ... and nothing else does, but texts the kernel may hand back: a pre-token beyond its window (unless truncation ends
    # the text before it)
    deferred = sum(H.longest_pretoken(hf, t) > KERNEL_WINDOW for t in texts if t not in routed)
    assert deferred == 2 and on_host <= len(routed) + deferred


@pytest.mark.parametrize("b", [1, 4, 5, 130])
@pytest.mark.parametrize("max_length", [2, 8])
def test_kernel_equals_host_encode(b, max_length, cuda_dev):
    """ac_bpe_encode against ac_bpe_encode_host on the same buffers: a lone wave, a full workgroup, a partial last workgroup,
    many workgroups.  A text the kernel reports as not done must hold a pre-token longer than its window."""
    from adaptive_classifier import _native as nv
    from adaptive_classifier.tokenizer import bpe_vocab_struct
    kind = "roberta_prefix"
    hf = H.build_tokenizer(kind)
    hv = H.HostVocab(hf)
    pool = [t for t in H.text_set(kind, 150) if t.isascii() and len(t) <= 4096]
    texts = [pool[(7 * i + b) % len(pool)] for i in range(b)]
    want_ids, want_mask, want_lens = H.encode_host(hv, texts, max_length)
    blob, offs = H.pack(texts)
    d_arrays = [torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(cuda_dev) for a in hv.arrays]
    vocab = bpe_vocab_struct(hv.spec, [t.data_ptr() for t in d_arrays], hv.slots)
    d_blob, d_offs = torch.from_numpy(blob).to(cuda_dev), torch.from_numpy(offs).to(cuda_dev)
    ids = torch.full((b, max_length), -7, dtype=torch.int64, device=cuda_dev)
    mask = torch.full((b, max_length), -7, dtype=torch.int64, device=cuda_dev)
    lens = torch.full((b,), -7, dtype=torch.int32, device=cuda_dev)
    with torch.cuda.device(cuda_dev):
        nv.check(nv.lib().ac_bpe_encode(nv.ptr(d_blob), nv.ptr(d_offs), b, ctypes.byref(vocab), max_length, nv.ptr(ids), nv.ptr(mask),
                                        nv.ptr(lens), nv.stream_ptr(cuda_dev)), "ac_bpe_encode")
    torch.cuda.synchronize()
    ids, mask, lens = ids.cpu().numpy(), mask.cpu().numpy(), lens.cpu().numpy()
    done = lens >= 0
    for i in np.nonzero(~done)[0]:
        assert lens[i] == -1 and H.longest_pretoken(hf, texts[i]) > KERNEL_WINDOW, texts[i][:80]
    assert np.array_equal(lens[done], want_lens[done])
    assert np.array_equal(ids[done], want_ids[done]) and np.array_equal(mask[done], want_mask[done])


def test_classifier_uses_the_device_bpe_tokenizer(cuda_dev):
    """A classifier built with a RoBERTa-style tokenizer tokenises on the device and predicts what the same classifier with
    the host tokenizer predicts (identical ids: only the launch paths differ)."""
    from adaptive_classifier import AdaptiveClassifier
    from adaptive_classifier.encoder import make_encoder
    from adaptive_classifier.tokenizer import HipByteBPETokenizer
    from oracle import bert_oracle
    hf = H.build_tokenizer("roberta")
    model = bert_oracle.make_roberta(128, 2, 2, 512, vocab=len(hf) + 8, max_pos=66, seed=4)
    enc = make_encoder(model, device=cuda_dev)
    a = AdaptiveClassifier("synthetic", device="cuda:0", encoder=enc, tokenizer=hf)
    b = AdaptiveClassifier("synthetic", device="cuda:0", config={"device_tokenizer": False}, encoder=enc, tokenizer=hf)
    assert isinstance(a.tokenizer, HipByteBPETokenizer) and b.tokenizer is hf
    texts = ["great product works well", "love it so much", "terrible waste of money", "awful do not buy",
             "it is fine nothing special", "average product okay"]
    labels = ["pos", "pos", "neg", "neg", "neu", "neu"]
    for c in (a, b):
        c.add_examples(texts, labels)
    for t in ["really great product!", "AWFUL... don't buy", "okay I guess"]:
        pa, pb = a.predict(t, k=3), b.predict(t, k=3)
        assert [l for l, _ in pa] == [l for l, _ in pb]
        assert np.allclose([s for _, s in pa], [s for _, s in pb], atol=1e-6)
    oa, ob = a.predict_batch(texts, k=2), b.predict_batch(texts, k=2)
    assert [[l for l, _ in p] for p in oa] == [[l for l, _ in p] for p in ob]
    assert np.allclose([[s for _, s in p] for p in oa], [[s for _, s in p] for p in ob], atol=1e-6)
    assert a.tokenizer.device_texts > 0 and a.tokenizer.host_texts == 0
