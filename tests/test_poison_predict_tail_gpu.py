"""GPU suite: the tail of a predict batch over poisoned staging buffers and outputs (tests/poison.py).

Regions, read from csrc/blend.hip and classifier.py before any poisoned run:

  classifier._post_stage   persistent torch.empty (>= 64 KB, never cleared).  predict_post_kernel writes n[q] for every query and
                           the class / score slots r < n[q] only (blend.hip: the store loop `for (r = lane; r < n; ...)`); the
                           alignment gap before the score block and the round-up to 16 bytes are never written.  The kernel reads
                           the stage back only to copy it, whole, to the host buffer (buffer loads bounded by the descriptor):
                           stale bytes travel but are never an index, a count or a wait target.
  classifier._post_buf     host-mapped, written by that copy alone; completion is a flag of the library's own (post_slot: a
                           hipMemset counter and a host flag it zeroes itself), not a word of these buffers.
  _blend_device's `out`    torch.empty per call; blend_topk_kernel writes n[q] and the slots r < n[q].
  ac_proto_scores / ac_rows_to_class / ac_softmax_rows outputs (torch.empty_like): every element written.
  No region is the caller's duty to clear.

So the only reader of unwritten slots is the host: _unpack's NaN test used to look at all b * kk score slots (and, in the numpy
form, at the round-up double behind them).  Fixed there (slots j < n[q] only); the kernels' stores are unchanged.

Every case runs under AC_PREDICT_POST = 1 (host-waited), 2 (device stage + D2H) and 0 (separate kernels) through
AdaptiveClassifier._finish_from_embeddings -> _post_launch / _finish -> _unpack on a classifier whose search and head are
stand-ins handing over the case's tensors, in four states: zero, zero again, ff, leftover (the 257-query case of the family first
on the same object).  (a) the lists and _last_nan are bit-identical in all four; (b) the lists equal predict_tail_ref.blend_topk
over the device preludes' fp32 results (same class order, scores to BLEND_ATOL = 1e-12, the bar of test_predict_tail_gpu.py),
and the preludes are within PRELUDE_ATOL = 1e-6 of fp64.
"""
import time
import types

import numpy as np
import pytest
import torch

import poison
import predict_tail_ref as R
from test_predict_tail_gpu import POST_SHAPES, _post_inputs

pytestmark = pytest.mark.gpu

_T0 = time.time()


@pytest.fixture(scope="module", autouse=True)
def _wall():
    yield
    print(f"\nMEASURED test_poison_predict_tail_gpu wall time {time.time() - _T0:.1f} s")


def _clf(case, dev):
    """An AdaptiveClassifier whose search and head hand over the case's tensors: everything behind them is the product's code."""
    from adaptive_classifier import AdaptiveClassifier, index as ix, ops, _native as nv
    D, I, rc, nrows, lut, nlut, Z, C = (case[x] for x in ("D", "I", "rc", "nrows", "lut", "nlut", "Z", "C"))
    c = AdaptiveClassifier.__new__(AdaptiveClassifier)
    c.id_to_label = {i: "label-%d" % i for i in range(C)}
    c.label_to_id = {v: i for i, v in c.id_to_label.items()}
    c.device = dev
    c.config = types.SimpleNamespace(prototype_update_frequency=1 << 30)
    c.memory = types.SimpleNamespace(index=types.SimpleNamespace(ntotal=1 if D is not None else 0), updates_since_rebuild=0,
                                     search_raw=lambda emb, kp: (D, I), class_map=lambda l2i, d: (rc, nrows, lut, nlut))
    c.adaptive_head = types.SimpleNamespace(eval=lambda: None) if Z is not None else None
    c._head_outputs = lambda emb: Z

    def device_stage(emb, kp):                     # AC_PREDICT_POST=0: the separate kernels, their outputs from torch.empty_like
        S = Cid = P = None
        if D is not None:
            S = ix.proto_scores(D, I)
            Cid = torch.empty_like(I)
            nv.check(nv.lib().ac_rows_to_class(nv.ptr(I), I.numel(), nv.ptr(rc), nrows, nv.ptr(lut), nlut, nv.ptr(Cid),
                                               nv.stream_ptr(dev)), "ac_rows_to_class")
        if Z is not None:
            P = ops.softmax_rows(Z)
        return S, Cid, P
    c._device_stage = device_stage
    return c


def _run(c, case, mode, monkeypatch):
    monkeypatch.setenv("AC_PREDICT_POST", mode)
    emb = torch.zeros(case["b"], 1, device=c.device)
    res = c._finish_from_embeddings(emb, case["k"], regular=case["regular"], check=False, k_proto=case["kp"], weights=case["wts"])
    return res, c._last_nan


def _need(b, kk):
    off_val = (4 * b + 4 * b * kk + 7) // 8 * 8
    return (off_val + 8 * b * kk + 15) // 16 * 16


def _reference(case):
    """blend_topk over the device preludes' fp32 results (computed once, unpoisoned), as labels; the preludes against fp64."""
    from adaptive_classifier import index as ix, ops
    D, I, Z, C = case["D"], case["I"], case["Z"], case["C"]
    S = Cid = P = None
    if D is not None:
        S = ix.proto_scores(D, I).cpu().numpy()
        ok = np.isfinite(D.cpu().numpy()).all(axis=1)                 # (a query with a NaN distance has no reference)
        assert np.abs(S - R.proto_scores(D.cpu().numpy(), I.cpu().numpy()))[ok].max(initial=0) <= R.PRELUDE_ATOL
        Cid = R.rows_to_class(I.cpu().numpy(), None if case["rc"] is None else case["rc"].cpu().numpy(), case["nrows"],
                              None if case["lut"] is None else case["lut"].cpu().numpy(), case["nlut"])
    if Z is not None:
        P = ops.softmax_rows(Z).cpu().numpy()
        assert np.abs(P - R.softmax_rows(Z.cpu().numpy())).max() <= R.PRELUDE_ATOL
    w = case["wts"].cpu().numpy()
    kk = max(1, min(case["k"], C))
    ncls = C if case["regular"] else min(case["k"], C)
    return R.blend_topk(S, Cid, P, w[0], w[1], ncls, min(kk, case["k"]))


def _check_lists(got, want, skip=()):
    assert len(got) == len(want)
    for q, (g, w) in enumerate(zip(got, want)):
        if q in skip:
            continue
        assert [l for l, _ in g] == ["label-%d" % c for c, _ in w], (q, g, w)
        assert all(abs(a[1] - b[1]) <= R.BLEND_ATOL for a, b in zip(g, w)), (q, g, w)


def _big_case(dev):
    b, C, kp, k = 257, 37, 16, 5
    D, I, rc, nrows, lut, nlut, Z, wts = _post_inputs(C, kp, b, np.random.default_rng(1), dev)
    return dict(b=b, C=C, kp=kp, k=k, D=D, I=I, rc=rc, nrows=nrows, lut=lut, nlut=nlut, Z=Z, wts=wts, regular=True)


def _four_states(case, mode, monkeypatch, dev, nan_queries=()):
    p = poison.poisoned_empty(monkeypatch, None)
    want = _reference(case)
    kk = max(1, min(case["k"], case["C"]))
    need = _need(case["b"], kk)
    res = {}
    for state, byte in (("zero", 0x00), ("zero2", 0x00), ("ff", 0xFF), ("leftover", 0x00)):
        p.byte = byte
        c = _clf(case, dev)
        if state == "leftover":
            big = _big_case(dev)
            cb = _clf(big, dev)
            _run(cb, big, mode, monkeypatch)
            for name in ("_post_stage", "_post_buf"):                 # the case under test on the same buffers
                if getattr(cb, name, None) is not None:
                    setattr(c, name, getattr(cb, name))
                    setattr(cb, name, None)
            assert mode == "0" or c._post_stage.numel() >= need
        elif mode == "1":
            poison.fill(c._post_buffer(need)[1], byte)                 # the host-mapped buffer: the caller's to fill
        res[state] = _run(c, case, mode, monkeypatch)
        if mode != "0":
            assert c._post_stage.numel() >= need
    assert p.filled > 0
    p.byte = None
    assert poison.same_bits(res["zero"], res["zero2"]), "two zero-state runs differ: " + poison.first_difference(res["zero"], res["zero2"])
    for state in ("ff", "leftover"):
        assert poison.same_bits(res["zero"], res[state]), f"the {state} state changed the result: " + poison.first_difference(res["zero"], res[state])
    for state, (lists, last_nan) in res.items():
        _check_lists(lists, want, skip=nan_queries)
        assert last_nan is bool(nan_queries), (state, last_nan)
        assert poison.all_finite([r for q, r in enumerate(lists) if q not in nan_queries])
    return res["ff"][0]


def _table_case(b, C, kp, k, hits, head, regular, dev):
    D, I, rc, nrows, lut, nlut, Z, wts = _post_inputs(C, kp, b, np.random.default_rng(b * 100003 + C * 7 + kp), dev)
    return dict(b=b, C=C, kp=kp, k=k, D=D if hits else None, I=I if hits else None, rc=rc, nrows=nrows, lut=lut, nlut=nlut,
                Z=Z if head else None, wts=wts, regular=regular)


@pytest.mark.parametrize("mode", ["1", "2", "0"])
@pytest.mark.parametrize("b,C,kp,k", POST_SHAPES)
def test_predict_tail_cases_over_poisoned_buffers(b, C, kp, k, mode, cuda_dev, monkeypatch):
    """The shapes of test_predict_tail_gpu.py (its inputs: ids of -1 and past the store, a query without hits, a tied head row):
    hits + head, hits only (queries with fewer than k classes), head only; predict's and predict_batch's head widths."""
    for hits, head, regular in ((True, True, True), (True, True, False), (True, False, False), (False, True, False)):
        _four_states(_table_case(b, C, kp, k, hits, head, regular, cuda_dev), mode, monkeypatch, cuda_dev)


def _short_case(kind, dev):
    """Queries that leave slots of their row unwritten.  No row map and no LUT: a hit's row id is its class (an index that lags
    behind id_to_label has ids of classes only), C = 6 classes, four hits per query."""
    C, kp = 6, 4
    t = lambda a, dt: torch.tensor(a, dtype=dt, device=dev)
    D = t([[0.1, 0.2, 0.3, 0.4]] * 5, torch.float32)
    Z = None
    if kind == "few_classes":          # no head; 4, 2, 1, 3 and 4 classes among the hits: full and short queries in one batch
        I, k = t([[0, 1, 2, 3], [4, 4, 5, 5], [2, 2, 2, 2], [0, 1, 1, 3], [5, 4, 3, 2]], torch.int64), 4
    elif kind == "padded":             # hits padded with id -1, one query all padding (n = 0), one full
        I, k = t([[0, 1, -1, -1], [-1, -1, -1, -1], [3, -1, -1, -1], [0, 1, 2, 3], [2, 2, -1, -1]], torch.int64), 4
        D = torch.where(I < 0, torch.full_like(D, R.FLT_MAX), D)
    elif kind == "k_gt_C":             # k = 9 > C = 6: kk = 6 slots, at most four classes hit
        I, k = t([[0, 1, 2, 3], [4, 4, 5, 5], [-1, -1, -1, -1], [0, 0, 0, 1], [5, 4, 3, 2]], torch.int64), 9
    elif kind == "k_gt_C_head":        # ... and with a head: every query fills its C slots
        I, k = t([[0, 1, 2, 3], [4, 4, 5, 5], [-1, -1, -1, -1], [0, 0, 0, 1], [5, 4, 3, 2]], torch.int64), 9
        Z = torch.from_numpy(np.random.default_rng(4).standard_normal((5, C)).astype(np.float32)).to(dev)
    elif kind == "short_head":         # predict_batch's head width min(k, C) = 3 with k = 3 ... full rows beside a no-hit query
        I, k = t([[0, 1, 2, 3], [4, 4, 5, 5], [-1, -1, -1, -1], [0, 0, 0, 1], [5, 4, 3, 2]], torch.int64), 3
        Z = torch.from_numpy(np.random.default_rng(5).standard_normal((5, C)).astype(np.float32)).to(dev)
    wts = torch.tensor([[0.7] * C, [0.3] * C], dtype=torch.float64, device=dev)
    return dict(b=5, C=C, kp=kp, k=k, D=D, I=I, rc=None, nrows=C, lut=None, nlut=0, Z=Z, wts=wts, regular=False)


@pytest.mark.parametrize("mode", ["1", "2", "0"])
@pytest.mark.parametrize("kind", ["few_classes", "padded", "k_gt_C", "k_gt_C_head", "short_head"])
def test_queries_that_leave_slots_unwritten(kind, mode, cuda_dev, monkeypatch):
    case = _short_case(kind, cuda_dev)
    got = _four_states(case, mode, monkeypatch, cuda_dev)
    kk = max(1, min(case["k"], case["C"]))
    if case["Z"] is None:
        assert any(len(r) < kk for r in got) and (kind == "k_gt_C" or any(len(r) == kk for r in got))   # short and full rows


@pytest.mark.parametrize("mode", ["1", "2", "0"])
def test_a_genuine_nan_in_a_used_slot_is_still_seen(mode, cuda_dev, monkeypatch):
    """Query 1's first distance is NaN: its hit scores are NaN in slots the kernel wrote.  _last_nan must be True in every state
    (the fix must not blind the check), and the other queries' lists are the reference's."""
    case = _short_case("few_classes", cuda_dev)
    case["D"] = case["D"].clone()
    case["D"][1, 0] = float("nan")
    got = _four_states(case, mode, monkeypatch, cuda_dev, nan_queries=(1,))
    assert len(got[1]) >= 1 and all(s != s for _, s in got[1])


def test_the_stale_slots_are_really_there(cuda_dev, monkeypatch):
    """The scenario itself, on the device: after a batch with short queries the never-written score slots of the ff-filled
    staging buffer still read as NaN doubles -- what the host tail used to take for NaN scores -- while every used slot is finite
    and _last_nan stays False."""
    case = _short_case("few_classes", cuda_dev)
    poison.poisoned_empty(monkeypatch, 0xFF)
    c = _clf(case, cuda_dev)
    lists, last_nan = _run(c, case, "2", monkeypatch)
    b, kk = case["b"], 4
    off_val = (4 * b + 4 * b * kk + 7) // 8 * 8
    val = c._post_stage[off_val:off_val + 8 * b * kk].cpu().numpy().view(np.float64).reshape(b, kk)
    n = np.array([len(r) for r in lists])
    used = np.arange(kk)[None, :] < n[:, None]
    assert n.tolist() == [4, 2, 1, 3, 4] and np.isnan(val[~used]).all() and np.isfinite(val[used]).all() and last_nan is False
