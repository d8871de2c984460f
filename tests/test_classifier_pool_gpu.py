"""GPU suite: config["pooling"] of AdaptiveClassifier / MultiLabelAdaptiveClassifier -- the mean-pooled embedding through the
classifier's own paths (tokenizer -> _embed_device -> add_examples / predict), persistence of the choice, and the refusal of an
encoder that cannot pool.  A tiny random BERT through the encoder= / tokenizer= injection of tests/test_classifier_gpu.py."""
import json

import numpy as np
import pytest
import torch

import encoder_ref as R
import encoder_pool_ref as P
from helpers import HashTokenizer

pytestmark = pytest.mark.gpu

TEXTS = ["great product works well", "love it so much", "best purchase ever made",
         "terrible waste of money", "awful do not buy", "broke after one day",
         "it is fine nothing special", "average product okay", "neither good nor bad"]
LABELS = ["positive"] * 3 + ["negative"] * 3 + ["neutral"] * 3
QUERIES = ["really great product", "awful thing", "fine I guess", "x"]
SPEC = R.ModelSpec("bert", 128, R.L, 2, 512, "peaked", max_pos=64, seed=0)   # the architecture and regime of the grid's bert / peaked group (its bound)


@pytest.fixture(scope="module")
def enc(cuda_dev):
    from adaptive_classifier.encoder import HipBertEncoder
    return HipBertEncoder(R.make_model(SPEC), device=cuda_dev)


@pytest.fixture(scope="module")
def clf(enc):
    from adaptive_classifier import AdaptiveClassifier
    c = AdaptiveClassifier("synthetic-bert-tiny", device="cuda:0", config={"pooling": "mean"}, encoder=enc, tokenizer=HashTokenizer())
    c.add_examples(TEXTS, LABELS)
    return c


def _fp64_pooled(texts, mean=True):
    """the fp64 forward of tests/encoder_ref.py on the tokenizer's own output, pooled by tests/encoder_pool_ref.py"""
    tok = HashTokenizer()(texts)
    ids, types, mask = tok["input_ids"], tok["token_type_ids"], tok["attention_mask"]
    model = R.make_model(SPEC)
    hs = []
    cls = R.bert_forward(model.state_dict(), model.config, ids, types, mask, hidden_out=hs)
    return P.masked_mean_normalize(hs[-1], mask.bool()) if mean else cls


def test_embed_device_is_the_mean_pooled_embedding(clf, enc):
    bound = R.KERNEL_FACTOR * P.FP32_DEV_POOL[("bert", "peaked")]
    for texts in (TEXTS, QUERIES, ["x"]):          # 9 ragged texts (packed), 4 (<= 32 rows: layer by layer), a single short one
        got = clf._embed_device(texts).double().cpu()
        want = _fp64_pooled(texts)
        d = float((got - want).abs().max())
        print(f"[classifier pool] {len(texts)} texts: deviation {d:.1e} (bound {bound:.1e}); from the CLS rows "
              f"{float((got - _fp64_pooled(texts, mean=False)).abs().max()):.1e}")
        assert d <= bound, (len(texts), d)
        assert enc.last_one_launch is False
    assert float((clf._embed_device(TEXTS).double().cpu() - _fp64_pooled(TEXTS, mean=False)).abs().max()) > 1e-2
    # the stored examples carry the same rows (add_examples went through the same path)
    stored = torch.stack([e.embedding.cpu() for e in clf.memory.examples["positive"]]).double()
    assert float((stored - _fp64_pooled(TEXTS[:3])).abs().max()) <= bound


def test_add_examples_predict_and_predict_batch_run(clf):
    preds = clf.predict("really great product", k=3)
    assert len(preds) == 3 and abs(sum(s for _, s in preds) - 1.0) < 1e-6
    assert preds == sorted(preds, key=lambda x: -x[1])
    out = clf.predict_batch(QUERIES, k=2, batch_size=3)
    assert len(out) == 4 and all(1 <= len(p) <= 2 for p in out)
    assert all(isinstance(l, str) and isinstance(s, float) and np.isfinite(s) for p in out for l, s in p)
    assert clf.memory.index.ntotal == 3 and clf.training_history == {"positive": 3, "negative": 3, "neutral": 3}


def test_save_load_keeps_the_pooling(clf, enc, tmp_path):
    from adaptive_classifier import AdaptiveClassifier
    clf.save(str(tmp_path / "mean"))
    cfg = json.loads((tmp_path / "mean" / "config.json").read_text())
    assert cfg["config"]["pooling"] == "mean"
    for loader in (AdaptiveClassifier.load, AdaptiveClassifier.from_pretrained):
        c2 = loader(str(tmp_path / "mean"), device="cuda:0", encoder=enc, tokenizer=HashTokenizer())
        assert c2._pooling == "mean"
        assert torch.equal(c2._embed_device(QUERIES), clf._embed_device(QUERIES))
        for a, b in zip(clf.predict_batch(QUERIES, k=3), c2.predict_batch(QUERIES, k=3)):
            assert [l for l, _ in a] == [l for l, _ in b]
            assert np.allclose([s for _, s in a], [s for _, s in b], atol=1e-6)
        a, b = clf.predict(QUERIES[0], k=3), c2.predict(QUERIES[0], k=3)
        assert [l for l, _ in a] == [l for l, _ in b] and np.allclose([s for _, s in a], [s for _, s in b], atol=1e-6)


def test_default_directories_keep_their_bytes(enc, tmp_path):
    """a default classifier writes no "pooling" key: config.json is what it was before the option existed"""
    from adaptive_classifier import AdaptiveClassifier
    from adaptive_classifier.models import ModelConfig
    for i, config in enumerate((None, {"pooling": "cls"})):
        c = AdaptiveClassifier("synthetic-bert-tiny", device="cuda:0", config=config, encoder=enc, tokenizer=HashTokenizer())
        c.add_examples(TEXTS, LABELS)
        c.save(str(tmp_path / str(i)))
        cfg = json.loads((tmp_path / str(i) / "config.json").read_text())
        assert "pooling" not in cfg["config"] and "pooling" not in cfg
        assert cfg["config"] == ModelConfig().to_dict()
        c2 = AdaptiveClassifier.load(str(tmp_path / str(i)), device="cuda:0", encoder=enc, tokenizer=HashTokenizer())
        assert c2._pooling == "cls"
        want = _fp64_pooled(QUERIES, mean=False)
        assert float((c2._embed_device(QUERIES).double().cpu() - want).abs().max()) <= R.KERNEL_FACTOR * R.FP32_DEV[("bert", "peaked")]
    assert (tmp_path / "0" / "config.json").read_bytes() == (tmp_path / "1" / "config.json").read_bytes()


class _ClsOnlyEncoder:
    """a user-supplied encoder from before the option: encode_cls takes no `pooling`"""

    def __init__(self, inner):
        self.inner, self.config, self.calls = inner, inner.config, 0

    def eval(self):
        return self

    def encode_cls(self, input_ids, token_type_ids=None, attention_mask=None, verify=True):
        self.calls += 1
        return self.inner.encode_cls(input_ids, token_type_ids, attention_mask, verify=verify)


def test_an_encoder_without_the_keyword_refuses_mean(enc):
    from adaptive_classifier import AdaptiveClassifier, MultiLabelAdaptiveClassifier
    old = _ClsOnlyEncoder(enc)
    for cls in (AdaptiveClassifier, MultiLabelAdaptiveClassifier):
        with pytest.raises(ValueError, match="pooling"):
            cls("synthetic", device="cuda:0", config={"pooling": "mean"}, encoder=old, tokenizer=HashTokenizer())
    assert old.calls == 0                                                   # refused before anything was encoded
    c = AdaptiveClassifier("synthetic", device="cuda:0", encoder=old, tokenizer=HashTokenizer())     # "cls" still works with it
    assert c._embed_device(QUERIES).shape == (4, 128) and old.calls == 1
    # ... and never silently CLS: an encoder swapped in after construction is refused at the call
    m = AdaptiveClassifier("synthetic", device="cuda:0", config={"pooling": "mean"}, encoder=enc, tokenizer=HashTokenizer())
    m.model = old
    with pytest.raises(ValueError, match="pooling"):
        m._embed_device(QUERIES)
    assert old.calls == 1


def test_multilabel_accepts_the_key(enc, tmp_path):
    from adaptive_classifier import MultiLabelAdaptiveClassifier
    m = MultiLabelAdaptiveClassifier("synthetic", device="cuda:0", config={"pooling": "mean"}, encoder=enc, tokenizer=HashTokenizer())
    assert m._pooling == "mean"
    got = m._embed_device(QUERIES).double().cpu()
    assert float((got - _fp64_pooled(QUERIES)).abs().max()) <= R.KERNEL_FACTOR * P.FP32_DEV_POOL[("bert", "peaked")]
    with pytest.raises(ValueError, match="pooling"):
        MultiLabelAdaptiveClassifier("synthetic", device="cuda:0", config={"pooling": "max"}, encoder=enc, tokenizer=HashTokenizer())
