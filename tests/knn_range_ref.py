"""TEST INFRASTRUCTURE -- the oracle of the range search (ac_knn_l2_range_* / ac_knn_ip_range_*, faiss range_search).

    l2: x(q, n) = sum_c (float64(P[n,c]) - float64(Q[q,c]))^2      hit iff float32(x) <  r_q
    ip: x(q, n) = sum_c  float64(P[n,c]) * float64(Q[q,c])         hit iff float32(x) >  r_q
    the sum runs over c = 0, 1, ..., D-1 in that fixed order for every row, so identical rows get identical values; both
    comparisons are strict and made on the fp32 rounding; the hits of a query are listed by ascending row id.
    Returns lims int64 [nq + 1], D float32, I int64 (row id + row_offset) -- faiss's (lims, D, I).

The library sums in another order, so a value within a few fp64 ulps of the midpoint between two fp32 numbers next to r could
round to the other side.  The two helpers keep tests free of such undecidable cases WITHOUT leaving any query out: `gap_radius`
picks a radius in the middle of a wide gap between two ranks, `margin_ulps` measures how far the nearest value stays from it (the
tests assert that margin before they compare ids).
"""
import numpy as np


def unit_rows(n, D, seed):
    """unit-norm Gaussian rows (fp32)"""
    x = np.random.default_rng(seed).standard_normal((n, D))
    return np.ascontiguousarray(x / np.linalg.norm(x, axis=1, keepdims=True), dtype=np.float32)


def fixed_order_values(P, Q, metric):
    """[nq, N] fp64 values, summed over the columns in index order"""
    P64 = np.asarray(P, dtype=np.float32).astype(np.float64)
    Q64 = np.asarray(Q, dtype=np.float32).astype(np.float64)
    acc = np.zeros((Q64.shape[0], P64.shape[0]), dtype=np.float64)
    for c in range(Q64.shape[1]):
        if metric == "ip":
            acc += P64[None, :, c] * Q64[:, c:c + 1]
        else:
            e = P64[None, :, c] - Q64[:, c:c + 1]
            acc += e * e
    return acc


def is_hit(values32, radius, metric):
    with np.errstate(invalid="ignore"):
        return values32 > np.float32(radius) if metric == "ip" else values32 < np.float32(radius)


def range_search(P, Q, radius, metric="l2", row_offset=0, return_exact=False, values=None):
    """(lims, D, I) [+ the exact fp64 values]; radius: a scalar or one per query; values: fixed_order_values(P, Q, metric) if
    the caller has them already"""
    Q = np.asarray(Q, dtype=np.float32)
    nq = Q.shape[0]
    rad = np.broadcast_to(np.asarray(radius, dtype=np.float32), (nq,))
    x = fixed_order_values(P, Q, metric) if values is None else values
    lims = np.zeros(nq + 1, dtype=np.int64)
    Ds, Is, Es = [], [], []
    for q in range(nq):
        ids = np.nonzero(is_hit(x[q].astype(np.float32), rad[q], metric))[0].astype(np.int64)      # ascending row id
        lims[q + 1] = lims[q] + ids.size
        Ds.append(x[q, ids].astype(np.float32)); Es.append(x[q, ids]); Is.append(ids + row_offset)
    D = np.concatenate(Ds) if Ds else np.empty(0, np.float32)
    I = np.concatenate(Is) if Is else np.empty(0, np.int64)
    E = np.concatenate(Es) if Es else np.empty(0, np.float64)
    return (lims, D.astype(np.float32), I.astype(np.int64), E) if return_exact else (lims, D.astype(np.float32), I.astype(np.int64))


def gap_radius(sorted_values, lo, hi):
    """sorted_values: one query's fp32 values in rank order (best first: ascending for l2, descending for ip).  The fp32
    midpoint of the widest gap between two consecutive ranks i, i + 1 with lo <= i < hi: a radius that admits i + 1 rows."""
    v = np.asarray(sorted_values, dtype=np.float32).astype(np.float64)
    gaps = np.abs(np.diff(v[lo:hi + 1]))
    i = lo + int(np.argmax(gaps))
    return np.float32(0.5 * (v[i] + v[i + 1]))


def gap_radii(values, metric, lo, hi):
    """[nq] gap_radius of every query of an [nq, N] value matrix"""
    v32 = np.asarray(values).astype(np.float32)
    s = np.sort(v32, axis=1)
    if metric == "ip":
        s = s[:, ::-1]
    return np.array([gap_radius(s[q], lo, hi) for q in range(s.shape[0])], dtype=np.float32)


def margin_ulps(values, radius):
    """distance, in ulps of the radius, of the nearest fp32 value to it (values: one query's, any order)"""
    v = np.asarray(values).astype(np.float32).astype(np.float64)
    r = np.float32(radius)
    return float(np.min(np.abs(v - np.float64(r))) / np.float64(np.spacing(np.abs(r))))
