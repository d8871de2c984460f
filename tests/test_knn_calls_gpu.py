"""The native calls of the kNN Python layer equal the recorded ones (tests/data/knn_calls_parent.json, written by
tools/knn_call_probe.py at the parent of the commit that introduced the route planner and the two call builders): per case of
tests/knn_call_cases.py the same entries in the same order -- the workspace planners included, so the number of host calls per
search is part of the fixture -- with the same integers and the same pointers (by the tensor they point into)."""
import json
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import knn_call_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "knn_calls_parent.json")


@pytest.fixture(scope="module")
def recorded():
    return json.load(open(FIXTURE))


@pytest.fixture(scope="module")
def replay():
    from adaptive_classifier import _native as nv
    from adaptive_classifier import index as ix
    with cases.Recorder(nv) as rec:
        env = cases.Env(ix, torch.device("cuda:0"), rec)

        def run(name):
            env.obj = None
            return rec.record(dict(cases.CASES)[name], env)
        yield run


def test_fixture_holds_every_case(recorded):
    assert sorted(recorded) == sorted(cases.NAMES)
    entries = {c.split(" ")[0] for r in recorded.values() for c in r["calls"]}
    for m in ("l2", "ip"):                                     # every search entry is reached
        for e in ("topk_x", "topk_batch", "topk_sel", "topk_batch_sel", "topk_ids", "range_count", "range_count_sel", "range_count_batch",
                  "range_count_batch_sel", "range_count_ids", "range_fill", "range_fill_ids"):
            assert f"knn_{m}_{e}" in entries
    for name in ("range_l2_300_chunked", "range_ip_65536_prepared_sel_chunks_exact"):
        assert sum("_range_count" in c.split(" ")[0] for c in recorded[name]["calls"]) >= 3


@pytest.mark.parametrize("name", cases.NAMES)
def test_native_calls_equal_the_recorded_ones(name, recorded, replay):
    got, want = replay(name), recorded[name]
    assert got["raised"] == want["raised"]
    assert [c.split(" ")[0] for c in got["calls"]] == [c.split(" ")[0] for c in want["calls"]]
    for g, w in zip(got["calls"], want["calls"]):
        assert g == w
