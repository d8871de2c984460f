"""Shared by tests/test_predict_tail_ref_cpu.py and tests/test_predict_tail_gpu.py: the tail of predict() / predict_batch()
-- what turns kNN hits and head outputs into the returned (label, score) lists -- stated once in plain numpy fp64 and
Python floats, from the reference project's formulas (the lines the kernels' comments cite).  Nothing here imports the
product package.

  proto_scores       memory.py:117 (exp(-d)) and :129-130 (softmax over the valid hits)        ac_proto_scores
  rows_to_class      memory.py:123 (index_to_label) generalised to an int32 row map + class LUT ac_rows_to_class
  softmax_rows       classifier.py:435 / :1345 (F.softmax)                                      ac_softmax_rows
  sigmoid            multilabel.py:43 (torch.sigmoid)                                           ac_sigmoid
  l2_normalize_rows  classifier.py:1450 (F.normalize, p = 2, eps = 1e-12)                       ac_l2_normalize_rows
  blend_topk         classifier.py:447-480 and :1359-1384 (dict in insertion order, sorted())   ac_blend_topk

Bars.  The prelude kernels are fp32 exp / divide arithmetic over values in [0, 1] (or unit rows): 1e-6 absolute, the
project's bar for that arithmetic elsewhere.  The blend is fp64 on both sides over the same fp32 inputs, the same sums
in the same order: identical class order (ties included), scores to 1e-12.

Worst measured |device - fp64| per kernel over the grid of tests/test_predict_tail_gpu.py (MI355X):

    kernel                  worst abs error    bar
    ac_softmax_rows         5.9e-08            1e-6
    ac_sigmoid              8.3e-08            1e-6
    ac_proto_scores         4.1e-09            1e-6
    ac_l2_normalize_rows    2.2e-08            1e-6
    ac_blend_topk (scores)  7.7e-15            1e-12
"""
import numpy as np

PRELUDE_ATOL = 1e-6
BLEND_ATOL = 1e-12
FLT_MAX = float(np.finfo(np.float32).max)


def proto_scores(D, I):
    """[nq, k] fp64: softmax over the valid hits (id >= 0) of exp(-d); 0 where id < 0; a row without a valid hit is all zeros."""
    D = np.asarray(D, dtype=np.float64)
    I = np.asarray(I)
    out = np.zeros(D.shape, dtype=np.float64)
    for q in range(D.shape[0]):
        v = I[q] >= 0
        if not v.any():
            continue
        s = np.exp(-D[q][v])                       # memory.py:117
        e = np.exp(s - s.max())                    # memory.py:129-130
        out[q][v] = e / e.sum()
    return out


def rows_to_class(I, row_class=None, nrows=0, lut=None, nlut=0):
    """int64 like I: hit row id -> class id.  id outside [0, nrows) gives -1; row_class (int32 [nrows]) maps a row to a label
    index (None: the row id is the label index); lut (int64 [nlut]) maps a label index to a class id, -1 for an index outside
    [0, nlut) (None: the label index is the class id)."""
    I = np.asarray(I, dtype=np.int64)
    out = np.full(I.shape, -1, dtype=np.int64)
    flat_in, flat_out = I.reshape(-1), out.reshape(-1)
    for t in range(flat_in.size):
        i = int(flat_in[t])
        if not 0 <= i < nrows:
            continue
        c = int(row_class[i]) if row_class is not None else i
        if lut is not None:
            c = int(lut[c]) if 0 <= c < nlut else -1
        flat_out[t] = c
    return out


def softmax_rows(Z):
    Z = np.asarray(Z, dtype=np.float64)
    e = np.exp(Z - Z.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def sigmoid(X):
    X = np.asarray(X, dtype=np.float64)
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-X))


def l2_normalize_rows(X, eps=1e-12):
    X = np.asarray(X, dtype=np.float64)
    n = np.sqrt((X * X).sum(axis=1, keepdims=True))
    return X / np.maximum(n, eps)


def blend_topk(S, Cid, P, wp, wh, ncls_head, k):
    """Per query a list of at most k (class id, score) pairs.  S / Cid [b, kp] hit scores and hit classes (class outside
    [0, C) = no class; both None: no hits), P [b, C] head probabilities (None: no head), wp / wh [C] weights.
    classifier.py:447-480: a dict filled with the hits in hit order (several hits of one class add up before the weight),
    then with the head's top `ncls_head` classes in torch.topk's order (descending, equal values by ascending class id);
    sorted() by descending score -- stable, so ties stay in insertion order; normalised by the total when it is positive."""
    b = (S if S is not None else P).shape[0]
    C = len(wp)
    out = []
    for q in range(b):
        hit_sum = {}
        if S is not None:
            for s, c in zip(S[q].tolist(), np.asarray(Cid[q]).tolist()):
                if 0 <= c < C:
                    hit_sum[c] = hit_sum.get(c, 0.0) + float(s)
        combined = {c: s * float(wp[c]) for c, s in hit_sum.items()}
        if P is not None and ncls_head > 0:
            p = [float(x) for x in P[q].tolist()]
            order = sorted(range(C), key=lambda c: -p[c])[:ncls_head]            # stable: equal values by ascending id
            for c in order:
                combined[c] = combined.get(c, 0.0) + p[c] * float(wh[c])
        preds = sorted(combined.items(), key=lambda x: x[1], reverse=True)
        total = sum(s for _, s in preds)
        if total > 0:
            preds = [(c, s / total) for c, s in preds]
        out.append(preds[:k])
    return out


def check_blend(want, n, cls, val, sentinel_cls=None, sentinel_val=None):
    """The comparison the GPU test makes, as a function so that the CPU suite can show it fails on a wrong result.
    want: blend_topk's lists; n [b], cls [b, k], val [b, k]: the device's out_n / out_class / out_score.  Raises AssertionError."""
    n, cls, val = np.asarray(n), np.asarray(cls), np.asarray(val)
    assert len(want) == n.shape[0] == cls.shape[0] == val.shape[0]
    worst = 0.0
    for q, w in enumerate(want):
        assert int(n[q]) == len(w), f"query {q}: out_n {int(n[q])}, reference has {len(w)} entries"
        got_c = cls[q, :len(w)].tolist()
        assert got_c == [c for c, _ in w], f"query {q}: class order {got_c} != {[c for c, _ in w]}"
        if w:
            err = np.abs(val[q, :len(w)] - np.array([s for _, s in w], dtype=np.float64))
            r = int(err.argmax())
            worst = max(worst, float(err[r]))
            assert err[r] <= BLEND_ATOL, f"query {q} rank {r} class {w[r][0]}: {float(val[q, r])!r} vs {w[r][1]!r} (|diff| {err[r]:.3e})"
        if sentinel_cls is not None:
            assert (cls[q, len(w):] == sentinel_cls).all(), f"query {q}: class slots past out_n were written"
        if sentinel_val is not None:
            assert (val[q, len(w):] == sentinel_val).all(), f"query {q}: score slots past out_n were written"
    return worst
