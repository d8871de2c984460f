"""TEST INFRASTRUCTURE -- the oracle of the filtered top-k search (ac_knn_*_topk_sel / ac_knn_*_topk_ids).

    values as knn_range_ref.fixed_order_values (fp64, columns summed in index order, so identical rows get identical values);
    unselected rows removed; the rest ordered by (value ascending, id) for l2, (value descending, id) for ip; the first k kept,
    each rounded once to fp32; fewer than k selected rows padded with (FLT_MAX, -1) / (-FLT_MAX, -1) (fp64: +inf / -inf).

The library sums in another order than the oracle, so two rows whose exact values differ by a few fp64 ulps could swap.
`min_rel_gap` measures how far the ranks that decide a result lie apart; the tests assert it (>= 2^-40, a million times the
fp64 summation error of these shapes) before they compare ids -- no query is left out.

The shapes, selections and inputs of the oracle-equality cases live here, so that the CPU test (gaps) and the GPU test
(results) speak about the same arrays; they are computed once per process and never modified."""
import functools

import numpy as np

import knn_range_ref as rref

FLT_MAX = np.finfo(np.float32).max
MIN_GAP = 2.0 ** -40

# (N, D, nq, k): the route each pins is noted in tests/test_knn_select_gpu.py
CASES = [
    (5000, 768, 7, 16),
    (3000, 1024, 16, 8),
    (5000, 768, 33, 16),
    (1153, 100, 9, 10),
    (70000, 64, 5, 32),
    (300, 4096, 3, 20),
    (65537, 32, 1, 16),
    (999, 770, 7, 8),
]
SELECTIONS = ["half", "sparse", "block"]


def selection(name, N, k):
    """bool [N]: half = rng(3) < 0.5; sparse = rng(4) < 0.01; block = one contiguous run [N//3 + 5, N//3 + 5 + max(3k, N//50))"""
    if name == "half":
        return np.random.default_rng(3).random(N) < 0.5
    if name == "sparse":
        return np.random.default_rng(4).random(N) < 0.01
    assert name == "block"
    m = np.zeros(N, dtype=bool)
    lo = N // 3 + 5
    m[lo: lo + max(3 * k, N // 50)] = True
    return m


@functools.lru_cache(maxsize=None)
def case(N, D, nq, metric):
    """(P, Q, exact values [nq, N]) of one shape: unit Gaussian rows, seeds 1 (rows) and 2 (queries); read-only"""
    P, Q = rref.unit_rows(N, D, 1), rref.unit_rows(nq, D, 2)
    x = rref.fixed_order_values(P, Q, metric)
    for a in (P, Q, x):
        a.setflags(write=False)
    return P, Q, x


def pack(mask, bit0=0, total_bits=None, fill=True):
    """bool [n] -> uint64 words with the mask at bits [bit0, bit0 + n) of a bitmap of total_bits (default: just enough) whose
    other bits are `fill`; numpy little-endian bit order = the library's layout"""
    mask = np.asarray(mask, dtype=bool).reshape(-1)
    total = bit0 + mask.size if total_bits is None else total_bits
    bits = np.full(((max(total, 1) + 63) // 64) * 64, bool(fill))
    bits[bit0: bit0 + mask.size] = mask
    if total_bits is None and bit0 == 0:
        bits[mask.size:] = False
    return np.packbits(bits, bitorder="little").view("<u8").copy()


def filtered_topk(P, Q, k, mask, metric, row_offset=0, values=None):
    """(D fp32 [nq, k], I int64 [nq, k], E fp64 [nq, k]) of the k best SELECTED rows per query"""
    x = rref.fixed_order_values(P, Q, metric) if values is None else values
    mask = np.asarray(mask, dtype=bool).reshape(-1)
    ids = np.nonzero(mask)[0].astype(np.int64)
    nq = x.shape[0]
    pad = -np.inf if metric == "ip" else np.inf
    E = np.full((nq, k), pad, dtype=np.float64)
    I = np.full((nq, k), -1, dtype=np.int64)
    for q in range(nq):
        v = x[q, ids]
        order = np.lexsort((ids, -v if metric == "ip" else v))[:k]       # by (value, id): lexsort's LAST key is the primary one
        E[q, : order.size] = v[order]
        I[q, : order.size] = ids[order] + row_offset
    D = np.where(I >= 0, E, -FLT_MAX if metric == "ip" else FLT_MAX).astype(np.float32)
    return D, I, E


def min_rel_gap(values, mask, k, metric="l2"):
    """the smallest relative gap |a - b| / max(|a|, |b|) between consecutive DISTINCT exact values among the best k + 1 selected
    rows of any query (inf when no query has two distinct values there)"""
    mask = np.asarray(mask, dtype=bool).reshape(-1)
    v = np.asarray(values)[:, mask]
    v = np.sort(-v if metric == "ip" else v, axis=1)[:, : k + 1]
    best = np.inf
    for row in v:
        d = np.unique(row)
        if d.size > 1:
            a, b = d[:-1], d[1:]
            best = min(best, float(np.min(np.abs(b - a) / np.maximum(np.maximum(np.abs(a), np.abs(b)), np.finfo(np.float64).tiny))))
    return best
