"""CPU suite: tests/predict_tail_ref.py (the fp64 statement of the predict tail that tests/test_predict_tail_gpu.py holds
the kernels to) is anchored on what the reference project itself returned (tests/golden/*), on torch's fp64 operators,
and on hand-worked tie cases; and the comparison it offers is shown to fail on the mistakes it is there to catch."""
import json
import os

import numpy as np
import pytest
import torch

import predict_tail_ref as R
from oracle import head_oracle, knn_oracle, synth

G = os.path.join(os.path.dirname(__file__), "golden")


def _memory_blend_inputs():
    """The store, queries and head of tests/golden/gen_golden.py::gen_memory_and_blend, regenerated (as test_host_logic does)."""
    C, per, D = 4, 25, 768
    X, cent = synth.synth_unit_rows(C * per, D, 10), synth.synth_unit_rows(C, D, 11)
    protos = np.zeros((C, D), np.float64)
    for i in range(C * per):
        v = X[i] * 0.5 + cent[i % C]
        protos[i % C] += (v / np.linalg.norm(v)).astype(np.float32)
    protos = (protos / per).astype(np.float32)
    Q = synth.synth_unit_rows(8, D, 77)
    Q = np.stack([(q * 0.5 + cent[i % 4]) / np.linalg.norm(q * 0.5 + cent[i % 4]) for i, q in enumerate(Q)]).astype(np.float32)
    with torch.no_grad():
        P = torch.softmax(head_oracle.make_head(768, 4).eval()(torch.from_numpy(Q)), 1).numpy()
    return protos, Q, P


def test_proto_scores_and_blend_reproduce_the_reference_outputs():
    """memory_blend.json: get_nearest_prototypes' scores, _predict_regular (weights by training history, every class of the
    head votes) and predict_batch (0.7 / 0.3, the head's top min(k, C))."""
    g = json.load(open(os.path.join(G, "memory_blend.json")))
    protos, Q, P = _memory_blend_inputs()
    labels = [f"c{i}" for i in range(4)]
    for key, k in (("nearest", 4), ("nearest_k2", 2)):
        Dd, I = knn_oracle.knn_l2_topk(protos, Q, k)
        S = R.proto_scores(Dd, I)
        for q, want in enumerate(g[key]):
            assert [labels[i] for i in I[q]] == [l for l, _ in want]
            assert np.abs(S[q] - [s for _, s in want]).max() <= R.PRELUDE_ATOL
    hist = {"c0": 25, "c1": 5, "c2": 25, "c3": 9}
    wp = np.array([0.3 if hist[l] < 10 else 0.7 for l in labels])
    wh = np.array([0.7 if hist[l] < 10 else 0.3 for l in labels])

    def same(got, want):
        assert [labels[c] for c, _ in got] == [l for l, _ in want]
        assert np.allclose([s for _, s in got], [s for _, s in want], rtol=0, atol=1e-6)

    for key, want in g["predict"].items():
        Dd, I = knn_oracle.knn_l2_topk(protos, Q, 4)
        S = R.proto_scores(Dd, I).astype(np.float32)
        for a, w in zip(R.blend_topk(S, R.rows_to_class(I, None, 4), P, wp, wh, 4, int(key[1:])), want):
            same(a, w)
    for key, want in g["predict_batch"].items():
        k = int(key[1:])
        Dd, I = knn_oracle.knn_l2_topk(protos, Q, k)
        S = R.proto_scores(Dd, I).astype(np.float32)
        got = R.blend_topk(S, R.rows_to_class(I, None, 4), P, np.full(4, 0.7), np.full(4, 0.3), min(k, 4), k)
        for a, w in zip(got, want):
            same(a, w)


def test_proto_scores_on_the_router_fixture_and_the_knn_cases():
    """router_fixture.npz holds the reference memory's scores for its own shipped classifier; knn_cases.json holds real
    search results (tied distances of duplicate rows, padding-free) but no scores: there torch's fp64 softmax is the anchor."""
    f = np.load(os.path.join(G, "router_fixture.npz"))
    D = np.take_along_axis(f["dist"], f["order"], 1).astype(np.float32)
    assert np.abs(R.proto_scores(D, f["order"]) - f["scores"]).max() <= R.PRELUDE_ATOL
    cases = json.load(open(os.path.join(G, "knn_cases.json")))
    for name, c in cases.items():
        D, I = np.asarray(c["D_out"], np.float32), np.asarray(c["I"], np.int64)
        S = R.proto_scores(D, I)
        want = torch.softmax(torch.exp(-torch.from_numpy(D).double()), 1).numpy()
        assert np.abs(S - want).max() <= 1e-15, name
        assert np.abs(S.sum(1) - 1).max() <= 1e-14
    D = np.asarray(cases["dups"]["D_out"], np.float32)
    S = R.proto_scores(D, np.asarray(cases["dups"]["I"]))
    assert D[0, 0] == D[0, 1] == D[0, 2] and S[0, 0] == S[0, 1] == S[0, 2]          # equal distances, equal scores


def test_preludes_equal_torch_fp64_and_the_edge_rows():
    rng = np.random.default_rng(0)
    Z = rng.standard_normal((5, 65)) * 3
    Z[1] = rng.choice([-80.0, 80.0], 65)
    Z[2, 7] += 1e4
    Z[3] = 0.5
    zt = torch.from_numpy(Z)
    assert np.abs(R.softmax_rows(Z) - torch.softmax(zt, 1).numpy()).max() <= 1e-15
    assert np.abs(R.sigmoid(Z) - torch.sigmoid(zt).numpy()).max() <= 1e-15
    assert R.softmax_rows(Z)[2, 7] == 1.0 and (R.softmax_rows(Z)[3] == 1 / 65).all()
    assert R.sigmoid(np.array([-1e4, 0.0, 1e4])).tolist() == [0.0, 0.5, 1.0]
    X = rng.standard_normal((4, 63))
    X[1] = 0
    X[2] *= 1e-20 / np.linalg.norm(X[2])
    X[3] *= 1e15 / np.linalg.norm(X[3])
    want = torch.nn.functional.normalize(torch.from_numpy(X), p=2, dim=1, eps=1e-12).numpy()
    got = R.l2_normalize_rows(X)
    assert np.abs(got - want).max() <= 1e-15 and (got[1] == 0).all()
    assert abs(np.linalg.norm(got[2]) - 1e-8) < 1e-20 and abs(np.linalg.norm(got[3]) - 1) < 1e-12
    # proto_scores: padding, underflow of exp(-d), one valid hit, FLT_MAX in the padding
    D = np.array([[0, 0, 0, 0], [250, 300, R.FLT_MAX, 200], [R.FLT_MAX] * 4, [1, R.FLT_MAX, R.FLT_MAX, R.FLT_MAX]], np.float32)
    I = np.array([[3, 2, 1, 0], [5, 6, -1, 7], [-1, -1, -1, -1], [9, -1, -1, -1]])
    S = R.proto_scores(D, I)
    assert S[0].tolist() == [0.25] * 4 and np.allclose(S[1], [1 / 3, 1 / 3, 0, 1 / 3], rtol=0, atol=1e-15)
    assert S[2].tolist() == [0] * 4 and S[3].tolist() == [1, 0, 0, 0]


def test_rows_to_class_maps_and_bounds():
    I = np.array([-1, 0, 4, 5, 10 ** 12, -(2 ** 40), 2])
    assert R.rows_to_class(I, None, 5).tolist() == [-1, 0, 4, -1, -1, -1, 2]
    rc = np.array([3, 3, 0, 7, -2], np.int32)
    assert R.rows_to_class(I, rc, 5).tolist() == [-1, 3, -2, -1, -1, -1, 0]
    lut = np.array([10, -1, 12, 13], np.int64)
    assert R.rows_to_class(I, rc, 5, lut, 4).tolist() == [-1, 13, -1, -1, -1, -1, 10]
    assert R.rows_to_class(I, None, 5, lut, 4).tolist() == [-1, 10, -1, -1, -1, -1, 12]
    assert R.rows_to_class(I.reshape(1, 7), None, 5).shape == (1, 7)


def test_blend_tie_rules_by_hand():
    """Exactly representable values, weights 1: hits first in hit order, then head classes in rank order."""
    one = np.ones(6)
    S = np.array([[0.5, 0.25, 0.25, 0.5]], np.float32)
    Cid = np.array([[4, 1, 4, -1]], np.int64)                 # class 4: 0.5 + 0.25; class 1: 0.25; one padded hit
    P = np.array([[0.25, 0.0, 0.75, 0.25, 0.0, 0.125]], np.float32)
    # head order: 2 (0.75), 0 (0.25), 3 (0.25), 5 (0.125), 1 (0), 4 (0); the top four vote
    got = R.blend_topk(S, Cid, P, one, one, 4, 6)[0]
    # combined: 4 -> 0.75 (hit, rank 0), 1 -> 0.25 (hit, rank 1), 2 -> 0.75, 0 -> 0.25, 3 -> 0.25, 5 -> 0.125; total 2.375
    assert [c for c, _ in got] == [4, 2, 1, 0, 3, 5]
    assert [s for _, s in got] == [v / 2.375 for v in (0.75, 0.75, 0.25, 0.25, 0.25, 0.125)]
    assert R.blend_topk(S, Cid, P, one, one, 4, 2)[0] == got[:2]
    assert [c for c, _ in R.blend_topk(None, None, P, one, one, 9, 9)[0]] == [2, 0, 3, 5, 1, 4]
    assert R.blend_topk(None, None, P, one, one, 0, 3) == [[]]
    assert R.blend_topk(S, Cid, None, one, one, 4, 3)[0] == [(4, 0.75), (1, 0.25)]
    zero = np.zeros(6)                                          # total 0: scores stay as they are (0), insertion order
    assert R.blend_topk(S, Cid, P, zero, zero, 2, 6)[0] == [(4, 0.0), (1, 0.0), (2, 0.0), (0, 0.0)]
    assert R.blend_topk(np.zeros((1, 2), np.float32), np.array([[-1, 99]]), None, one, one, 0, 3) == [[]]


def _device_like(want, k, sentinel_cls=-7, sentinel_val=-7.0):
    n = np.array([len(w) for w in want], np.int32)
    cls = np.full((len(want), k), sentinel_cls, np.int32)
    val = np.full((len(want), k), sentinel_val, np.float64)
    for q, w in enumerate(want):
        for r, (c, s) in enumerate(w):
            cls[q, r], val[q, r] = c, s
    return n, cls, val


def test_the_blend_comparison_fails_on_planted_mistakes():
    C, kp, k, b = 70, 5, 73, 3
    rng = np.random.default_rng(3)
    S = rng.choice([0.25, 0.5], (b, kp)).astype(np.float32)
    Cid = np.stack([rng.permutation(C)[:kp] for _ in range(b)]).astype(np.int64)
    Cid[0, :2] = [66, 2]
    S[0, :2] = 0.5                                              # query 0: classes 66 and 2 tie, 66 first (hit order)
    P = np.full((b, C), 0.0, np.float32)                        # head-only classes all at 0: one long tie in class order
    one = np.ones(C)
    want = R.blend_topk(S, Cid, P, one, one, C, k)
    assert all(len(w) == C for w in want) and [c for c, _ in want[0][:2]] == [66, 2] and want[0][0][1] == want[0][1][1]
    n, cls, val = _device_like(want, k)
    assert R.check_blend(want, n, cls, val, -7, -7.0) == 0.0   # the faithful result passes
    # two tied entries swapped (what a rank rule that breaks ties by class id would give)
    r = next(i for i in range(C - 1) if want[0][i][1] == want[0][i + 1][1])
    c2 = cls.copy()
    c2[0, [r, r + 1]] = c2[0, [r + 1, r]]
    with pytest.raises(AssertionError, match="class order"):
        R.check_blend(want, n, c2, val, -7, -7.0)
    # a class past index 64 dropped (what a lane loop that stops at 64 would give)
    r = next(i for i, (c, _) in enumerate(want[1]) if c >= 64)
    n3, c3, v3 = n.copy(), cls.copy(), val.copy()
    c3[1, r:C - 1], v3[1, r:C - 1] = cls[1, r + 1:C], val[1, r + 1:C]
    c3[1, C - 1], v3[1, C - 1], n3[1] = -7, -7.0, C - 1
    with pytest.raises(AssertionError, match="out_n"):
        R.check_blend(want, n3, c3, v3, -7, -7.0)
    # a score off by 2e-12
    v4 = val.copy()
    v4[2, 0] += 2e-12
    with pytest.raises(AssertionError, match="diff"):
        R.check_blend(want, n, cls, v4, -7, -7.0)
    v5 = val.copy()
    v5[2, 0] += 5e-13                                           # (inside the bar: passes)
    assert 0 < R.check_blend(want, n, cls, v5, -7, -7.0) <= R.BLEND_ATOL
    # a slot past out_n written
    c6 = cls.copy()
    c6[0, C] = 0
    with pytest.raises(AssertionError, match="past out_n"):
        R.check_blend(want, n, c6, val, -7, -7.0)
