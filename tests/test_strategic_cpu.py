"""CPU suite: strategic mode's host logic -- activation rules (classifier.py:1573-1600), the candidate table of the best-response
search against the reference's own (tests/golden/strategic_bert_mini.json, written by gen_strategic.py) and the cost
functions' compute_cost formulas."""
import json
import logging
import os

import pytest
import torch

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def _bare(config):
    """An AdaptiveClassifier with only what activation touches (constructing one needs a GPU)."""
    from adaptive_classifier import AdaptiveClassifier, ModelConfig
    clf = AdaptiveClassifier.__new__(AdaptiveClassifier)
    clf.config = ModelConfig(config)
    clf.strategic_cost_function = clf.strategic_optimizer = clf.strategic_evaluator = None
    clf._initialize_strategic_components()
    return clf


@pytest.mark.parametrize("coefs", [None, {}, []])
def test_no_coefficients_leave_strategic_mode_off_with_a_warning(coefs, caplog):
    with caplog.at_level(logging.WARNING):
        clf = _bare({"enable_strategic_mode": True, "cost_coefficients": coefs})
    assert clf.strategic_mode is False and clf.config.enable_strategic_mode is True
    assert "no cost coefficients" in caplog.text


def test_dict_coefficients_switch_the_mode_off():
    clf = _bare({"enable_strategic_mode": True, "cost_coefficients": {"a": 1.0}})
    assert clf.strategic_mode is False and clf.config.enable_strategic_mode is False


@pytest.mark.parametrize("kind,cls", [("separable", "SeparableCostFunction"), ("linear", "LinearCostFunction")])
def test_list_coefficients_turn_the_mode_on(kind, cls):
    clf = _bare({"enable_strategic_mode": True, "cost_coefficients": [0.1] * 8, "cost_function_type": kind})
    assert clf.strategic_mode is True
    assert type(clf.strategic_cost_function).__name__ == cls
    assert clf.strategic_optimizer is not None and clf.strategic_evaluator is not None


def test_unknown_cost_type_switches_the_mode_off():
    clf = _bare({"enable_strategic_mode": True, "cost_coefficients": [0.1] * 8, "cost_function_type": "quadratic"})
    assert clf.strategic_mode is False and clf.config.enable_strategic_mode is False


def test_mode_off_without_enable():
    assert _bare({"cost_coefficients": [0.1] * 8}).strategic_mode is False


def test_candidate_table_equals_the_references():
    from adaptive_classifier.strategic import candidate_table
    ex = json.load(open(os.path.join(GOLD, "strategic_bert_mini.json")))
    feat, delta = candidate_table(len(ex["coefficients"]))
    assert feat.tolist() == [f for f, _ in ex["table"]]
    assert delta.tolist() == [d for _, d in ex["table"]]
    assert len(feat) == 50 and feat[0] == -1 and set(feat.tolist()[1:]) == {0, 1, 2, 3, 4}


def test_candidate_table_refuses_the_random_fill():
    from adaptive_classifier import _native as nv
    from adaptive_classifier.strategic import candidate_table
    with pytest.raises(nv.NativeError):
        candidate_table(4)


def test_host_candidates_are_the_table():
    from adaptive_classifier.strategic import SeparableCostFunction
    x = torch.randn(16)
    cands = SeparableCostFunction([1.0] * 16, [1.0] * 16)._generate_candidates(x)
    assert torch.equal(cands[0], x) and len(cands) == 50
    assert torch.equal(cands[1], torch.cat([x[:1] - 2.0, x[1:]]))


def test_compute_cost_formulas():
    from adaptive_classifier.strategic import CostFunctionFactory, LinearCostFunction, SeparableCostFunction
    g = torch.Generator().manual_seed(0)
    x, y = torch.randn(32, generator=g), torch.randn(32, generator=g)
    c = torch.randn(32, generator=g)
    sep = CostFunctionFactory.create_cost_function("separable", c.tolist())
    lin = CostFunctionFactory.create_cost_function("linear", c.tolist())
    assert isinstance(sep, SeparableCostFunction) and isinstance(lin, LinearCostFunction)
    cc = torch.tensor(c.tolist())
    assert torch.equal(sep.compute_cost(x, y), torch.relu(torch.dot(cc, y) - torch.dot(cc, x)))
    assert torch.equal(lin.compute_cost(x, y), torch.relu(torch.dot(cc, y - x)))
    assert lin.compute_cost(x, x).item() == 0.0
    c2 = SeparableCostFunction(c.tolist(), (2 * c).tolist())
    assert torch.equal(c2.compute_cost(x, y), torch.relu(torch.dot(2 * cc, y) - torch.dot(cc, x)))
    with pytest.raises(ValueError):
        CostFunctionFactory.create_cost_function("other", c.tolist())
    with pytest.raises(ValueError):
        SeparableCostFunction({"a": 1.0}, {"a": 1.0})
    named = LinearCostFunction({"a": 2.0}, feature_names=["a", "b"])
    assert named.alpha.tolist() == [2.0, 0.0]


def test_multilabel_keeps_refusing_strategic_mode():
    from adaptive_classifier import MultiLabelAdaptiveClassifier
    assert MultiLabelAdaptiveClassifier._STRATEGIC_SUPPORTED is False
    assert "Strategic mode is not built" in MultiLabelAdaptiveClassifier.__doc__
