"""The routing of the kNN Python layer equals the recorded one (tests/data/knn_route_parent.json, written by tools/knn_route_probe.py
at the parent of the commit that introduced `plan_topk` / `plan_range`): every scripted sequence of tests/knn_route_cases.py reaches
the same function with the same `prepared`, prepares as often and for the same capacity, asks the same workspace planner, passes the
same sel_bit0 / row_offset and leaves the same search count.  And the planner, called directly with the facts of each step, returns
the kind and the prepare flag the record shows."""
import json
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import knn_route_cases as cases  # noqa: E402

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "knn_route_parent.json")


@pytest.fixture(scope="module")
def recorded():
    return json.load(open(FIXTURE))


def test_sequences_replay_to_the_recorded_routing(recorded):
    from adaptive_classifier import index as ix
    got = cases.run_all(ix)
    assert list(got) == cases.NAMES and sorted(recorded) == sorted(cases.NAMES)
    for name in cases.NAMES:
        assert got[name] == recorded[name], name


def test_recorded_routing_sits_on_both_sides_of_every_rule(recorded):
    """the fixture is not vacuous: per target every kind and both prepare verdicts occur"""
    for target in cases.INDEXES + cases.SHARDED:
        steps = [cases.decode(s) for name in cases.NAMES if name.startswith(target + "-") for s in recorded[name]]
        topk = {(s["kind"], s["prepare"]) for s in steps if s["fn"] in ("l2", "ip", "sel", "ids", "l2x", "ipx")}
        assert {("plane", "1"), ("plane", "0"), ("rows", "0")} <= topk
        assert ("ids" in {s["kind"] for s in steps}) == (target in cases.INDEXES)         # a row shard has no id-list route
        assert {"plane", "rows"} <= {s["kind"] for s in steps if s["fn"] == "range"}


def test_thresholds_are_read_from_the_module_when_a_route_is_planned(monkeypatch):
    """the GPU suites lower `index.BATCH_MIN_PAIRS` / `index.PLANE_MIN_ROWS` to reach the plane route with small stores: every
    caller of the planner follows the module's value of the moment"""
    from adaptive_classifier import index as ix
    assert ix.plan_topk(70000, 80, 5) == ix.Route("rows", False)
    assert ix.plan_topk(70000, 4, 5, searches=1, policy=ix.PREPARE_SECOND_SEARCH) == ix.Route("rows", False)
    assert ix.plan_range(70000, True, True) == "rows"
    monkeypatch.setattr(ix, "BATCH_MIN_PAIRS", 1.0)
    monkeypatch.setattr(ix, "PLANE_MIN_ROWS", 65536)
    assert ix.plan_topk(70000, 80, 5) == ix.Route("plane", True)
    assert ix.plan_topk(70000, 4, 5, searches=1, policy=ix.PREPARE_SECOND_SEARCH) == ix.Route("plane", True)
    assert ix.plan_range(70000, True, True) == "plane"
    with cases.Harness(ix).patches():
        idx = ix.HipFlatL2Index(8, device="cpu")
        idx._n, idx._store = 70000, torch.zeros((1, 8)).expand(70000, 8)
        idx.search_device(torch.zeros((80, 8)), 5)
        assert idx._prepared is not None


def _facts(target, spec, total, counted, ix):
    if spec is None:
        return None
    ids = int(spec[3:]) if isinstance(spec, str) and spec.startswith("ids") and target in cases.INDEXES else None
    if spec == "unknown":
        count = (total + 1) // 2 if counted else None                                      # (every second row, once count() ran)
    else:
        count = int(spec[3:]) if isinstance(spec, str) else spec[1]
    return ix.Selection(ids, count, total)


def test_planner_returns_what_every_recorded_step_shows(recorded):
    from adaptive_classifier import index as ix
    for fn in (ix.plan_topk, ix.plan_range, ix.batch_applies, ix.sel_batch_applies):       # pure host code: no tensor, no library
        assert not {"torch", "nv", "np", "ctypes"} & set(fn.__code__.co_names)
    checked = 0
    for name, target, n0, D, steps in cases.SEQUENCES:
        n = n0
        total, counted, lines = cases.total_rows(target, n), False, iter(recorded[name])
        for step in steps:
            if step[0] == "fresh":
                n = step[3] if len(step) > 3 else n0
                total, counted = cases.total_rows(target, n), False
                continue
            rec = cases.decode(next(lines))
            have_plane, searches = rec["plane_before"] == "1", int(rec["searches_before"].replace("-", "0"))
            if step[0] == "count":
                counted = True
            elif step[0] == "search":
                _, nq, k, spec = step
                policy = (ix.PREPARE_ALWAYS if target in cases.SHARDED and spec is None else
                          ix.PREPARE_SECOND_SEARCH if target == "l2" and spec is None else ix.PREPARE_NEVER_SMALL)
                route = ix.plan_topk(n, nq, k, _facts(target, spec, total, counted, ix), have_plane, searches, policy)
                assert (route.kind, str(int(route.prepare))) == (rec["kind"], rec["prepare"]), (name, step)
                checked += 1
            elif step[0] == "range":
                _, nq, spec = step
                got = ix.plan_range(n, have_plane, ix.range_batch_applies(n, D, nq), _facts(target, spec, total, counted, ix))
                assert got == rec["kind"], (name, step)
                checked += 1
    assert checked > 500
