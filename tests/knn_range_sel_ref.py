"""TEST INFRASTRUCTURE -- the oracle of the FILTERED range search (ac_knn_*_range_count_sel / _ids, range_search(sel=)).

The oracle is tests/knn_range_ref.py's `range_search` on the SUB-MATRIX of the selected rows, with the ids mapped back to the rows
of the full store: a row is a hit iff it is selected and the unfiltered predicate holds; the hits of a query ascend by row id
(the selected rows keep their order).  Radii are `gap_radii` over the SELECTED rows' values (ranks 20..60), and every test first
asserts `margin` >= 64 ulps over those values, so no query is ever left out (the library sums in another order than the oracle).
Shared by tests/test_knn_range_sel_gpu.py and tests/test_knn_range_sel_cpu.py; everything `case` returns is read-only."""
import functools

import numpy as np

import knn_range_ref as ref


def filtered_range_search(P, Q, radius, mask, metric="l2", row_offset=0, return_exact=False, values=None):
    """(lims, D, I[, exact]) among the rows with mask[row] set; values: fixed_order_values(P, Q, metric) over ALL rows, if the
    caller has them (the sub-matrix's values are its columns: the sum runs over the columns of a row, never across rows)"""
    mask = np.asarray(mask, dtype=bool).reshape(-1)
    ids = np.nonzero(mask)[0].astype(np.int64)
    sub = None if values is None else np.ascontiguousarray(values[:, ids])
    out = ref.range_search(np.asarray(P)[ids], Q, radius, metric, row_offset=0, return_exact=return_exact, values=sub)
    return (out[0], out[1], ids[out[2]] + row_offset) + tuple(out[3:])


def pack(mask, bit0=0, tail_ones=True):
    """bool [n] -> uint64 words, exactly ceil((bit0 + n) / 64) of them (>= 1): row r is bit (bit0 + r).  Every bit that belongs to
    no row -- the bit0 bits in front and the tail of the last word -- is set to 1 (tail_ones): none of them may show up as a hit."""
    mask = np.asarray(mask, dtype=bool).reshape(-1)
    nbits = max((bit0 + mask.size + 63) // 64, 1) * 64
    bits = np.full(nbits, bool(tail_ones))
    bits[bit0: bit0 + mask.size] = mask
    return np.packbits(bits, bitorder="little").view("<u8").astype(np.uint64)


def margin(x, mask, rad):
    """the smallest distance, in ulps of the radius, of a SELECTED row's value to its query's radius"""
    radv = np.broadcast_to(np.asarray(rad, np.float32), (x.shape[0],))
    xs = x[:, np.asarray(mask, dtype=bool)]
    return min([ref.margin_ulps(xs[q], radv[q]) for q in range(x.shape[0]) if np.isfinite(radv[q]) and xs.shape[1]], default=np.inf)


# (N, D, nq) of the oracle test; the last one runs with ONLY ITS LAST ROW selected and an infinite radius
CASES = [(5000, 768, 33), (1153, 100, 17), (70000, 64, 5), (300, 4096, 3), (999, 770, 7)]
LAST_ROW_CASE = (65537, 32, 1)
IDS_ONLY_CASE = (20000, 4096, 2)         # a store the bitmap route refuses (D beyond the sweep, N > 8192): id-list route only


@functools.lru_cache(maxsize=None)
def case(N, D, nq, metric, density=0.5):
    """rows, queries, a random mask of the given density, the exact values of ALL rows and per-query gap radii (ranks 20..60 of
    the SELECTED rows' values): computed once, shared, never modified"""
    P, Q = ref.unit_rows(N, D, 1), ref.unit_rows(nq, D, 2)
    mask = np.random.default_rng(1000 + N).random(N) < density
    x = ref.fixed_order_values(P, Q, metric)
    rad = ref.gap_radii(x[:, mask], metric, 20, 60)
    for a in (P, Q, mask, x, rad):
        a.setflags(write=False)
    return P, Q, mask, x, rad
