"""GPU suite: a DeBERTa-v2/v3 encoder behind AdaptiveClassifier -- tokenizer -> _embed_device -> add_examples / predict / save /
load under both poolings, through the encoder= / tokenizer= injection of tests/test_classifier_pool_gpu.py.  The model is the tiny
random DeBERTa of tests/encoder_deberta_ref.py (no position table, no type table: the token_type_ids the HashTokenizer emits are
ignored); its pad id is the HashTokenizer's (0)."""
import numpy as np
import pytest
import torch

import encoder_ref as R
import encoder_deberta_ref as D
import encoder_pool_ref as P
from helpers import HashTokenizer

pytestmark = pytest.mark.gpu

TEXTS = ["great product works well", "love it so much", "best purchase ever made",
         "terrible waste of money", "awful do not buy", "broke after one day",
         "it is fine nothing special", "average product okay", "neither good nor bad"]
LABELS = ["positive"] * 3 + ["negative"] * 3 + ["neutral"] * 3
QUERIES = ["really great product", "awful thing", "fine I guess", "x"]
LONG = [" ".join(f"word{i}" for i in range(n)) for n in (40, 3, 31, 17, 36, 25, 38)]     # 204 rows packed: planes, two key tiles
BOUND = R.KERNEL_FACTOR * D.FP32_DEV_DEBERTA["peaked"]


@pytest.fixture(scope="module")
def model():
    return D.build_model(D.deberta_config(128, R.L, 2, 512, 64), "peaked", seed=0)


@pytest.fixture(scope="module")
def enc(model, cuda_dev):
    from adaptive_classifier.encoder import make_encoder
    e = make_encoder(model, device=cuda_dev)
    assert e.weights.attn_disentangled and e._dis.rel_span == 64 and e._dis.scale_factor == 3 and not e._has_types
    return e


@pytest.fixture(scope="module")
def clfs(enc):
    from adaptive_classifier import AdaptiveClassifier
    out = {}
    for pooling in ("cls", "mean"):
        c = AdaptiveClassifier("synthetic-deberta-tiny", device="cuda:0", config={"pooling": pooling}, encoder=enc, tokenizer=HashTokenizer())
        c.add_examples(TEXTS, LABELS)
        out[pooling] = c
    return out


def _fp64(model, texts, pooling):
    tok = HashTokenizer()(texts)
    ids, mask = tok["input_ids"], tok["attention_mask"]
    hs = []
    cls = D.deberta_forward(model, ids, None, mask, hidden_out=hs)
    return cls if pooling == "cls" else P.masked_mean_normalize(hs[-1], mask.bool())


@pytest.mark.parametrize("pooling", ["cls", "mean"])
def test_embed_device_is_the_fp64_embedding(clfs, enc, model, pooling):
    clf = clfs[pooling]
    for texts in (TEXTS, QUERIES, ["x"], LONG):     # 9 ragged texts (packed), 4 and 1 (<= 32 rows: layer by layer), 204 rows on planes
        got = clf._embed_device(texts).double().cpu()
        d = float((got - _fp64(model, texts, pooling)).abs().max())
        print(f"[classifier deberta] {pooling}: {len(texts)} texts: deviation {d:.1e} (bound {BOUND:.1e})")
        assert d <= BOUND, (pooling, len(texts), d)
        assert enc.last_one_launch is False
    other = "mean" if pooling == "cls" else "cls"
    assert float((clf._embed_device(TEXTS).double().cpu() - _fp64(model, TEXTS, other)).abs().max()) > 1e-2
    stored = torch.stack([e.embedding.cpu() for e in clf.memory.examples["positive"]]).double()
    assert float((stored - _fp64(model, TEXTS[:3], pooling)).abs().max()) <= BOUND


@pytest.mark.parametrize("pooling", ["cls", "mean"])
def test_add_examples_predict_and_predict_batch_run(clfs, pooling):
    clf = clfs[pooling]
    preds = clf.predict("really great product", k=3)
    assert len(preds) == 3 and abs(sum(s for _, s in preds) - 1.0) < 1e-6
    assert preds == sorted(preds, key=lambda x: -x[1])
    out = clf.predict_batch(QUERIES, k=2, batch_size=3)
    assert len(out) == 4 and all(1 <= len(p) <= 2 for p in out)
    assert all(isinstance(l, str) and isinstance(s, float) and np.isfinite(s) for p in out for l, s in p)
    assert clf.training_history == {"positive": 3, "negative": 3, "neutral": 3}


@pytest.mark.parametrize("pooling", ["cls", "mean"])
def test_save_load_round_trips(clfs, enc, tmp_path, pooling):
    from adaptive_classifier import AdaptiveClassifier
    clf = clfs[pooling]
    clf.save(str(tmp_path / pooling))
    c2 = AdaptiveClassifier.load(str(tmp_path / pooling), device="cuda:0", encoder=enc, tokenizer=HashTokenizer())
    assert c2._pooling == pooling
    assert torch.equal(c2._embed_device(QUERIES), clf._embed_device(QUERIES))
    for a, b in zip(clf.predict_batch(QUERIES, k=3), c2.predict_batch(QUERIES, k=3)):
        assert [l for l, _ in a] == [l for l, _ in b]
        assert np.allclose([s for _, s in a], [s for _, s in b], atol=1e-6)
