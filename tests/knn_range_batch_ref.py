"""TEST INFRASTRUCTURE -- shapes, inputs and the a-priori bound of the range search over the prepared fp16-plane store
(ac_knn_*_range_count_batch[_sel]).  The oracle is tests/knn_range_ref.py; inputs are unit rows with seeds 1 / 2 and gap radii of
ranks 20..60, as in tests/test_knn_range_gpu.py.  Shared by tests/test_knn_range_batch_gpu.py and tests/test_knn_range_batch_cpu.py;
everything `case` returns is read-only."""
import functools

import numpy as np

import knn_range_ref as ref

# (N, D, nq): Kp = D with several tiles per workgroup | D < 64 padded to Kp = 64, one row in the last 256-row tile | the 64-query
# tile, D % 64 != 0 | two query tiles, the second ragged | the production D | D % 4 != 0
CASES = [(70000, 64, 5), (65537, 32, 1), (65600, 100, 33), (66000, 72, 70), (65793, 768, 3), (65536, 70, 7)]


@functools.lru_cache(maxsize=None)
def case(N, D, nq, metric):
    """rows, queries, exact values and per-query gap radii (ranks 20..60) of one shape: computed once, shared, never modified"""
    P, Q = ref.unit_rows(N, D, 1), ref.unit_rows(nq, D, 2)
    x = ref.fixed_order_values(P, Q, metric)
    rad = ref.gap_radii(x, metric, 20, 60)
    for a in (P, Q, x, rad):
        a.setflags(write=False)
    return P, Q, x, rad


def batch_gamma(D):
    """include/acamd.h at ac_knn_l2_topk_batch: |v - s| <= gamma (|p|max + |q|)^2 for the one-product fp16 sweep value"""
    Kp = (D + 63) // 64 * 64
    return 1.01 * (2.0 ** -11 + (Kp + 18 + np.sqrt(Kp)) * 2.0 ** -24)


def bound(P, Q):
    """[nq] E_q = 1.02 gamma (|p|max + |q|)^2, |p|max from the fp32-rounded maximum |p|^2 the prepared store keeps"""
    P64, Q64 = np.asarray(P, np.float32).astype(np.float64), np.asarray(Q, np.float32).astype(np.float64)
    pmax = np.sqrt(np.float64(np.float32((P64 * P64).sum(axis=1).max())))
    qn = np.sqrt((Q64 * Q64).sum(axis=1))
    return 1.02 * batch_gamma(P64.shape[1]) * (pmax + qn) ** 2


def undecided_cap(x, rad, E, metric, mask=None):
    """pairs the plane MAY leave to the exact decision: the oracle value within 2.1 E_q (l2: E on each side of the threshold pair
    plus the sweep value's own E) or 1.05 E_q (ip: the same in product space, where the value is -v / 2) of the radius"""
    radv = np.broadcast_to(np.asarray(rad, np.float32), (x.shape[0],)).astype(np.float64)
    near = np.abs(x - radv[:, None]) <= ((2.1 if metric == "l2" else 1.05) * np.asarray(E))[:, None]
    near &= np.isfinite(radv)[:, None]
    if mask is not None:
        near &= np.asarray(mask, bool)[None, :]
    return int(near.sum())


def min_margin(x, rad):
    """the smallest distance, in ulps of the radius, of a value to its query's (finite) radius"""
    radv = np.broadcast_to(np.asarray(rad, np.float32), (x.shape[0],))
    return min([ref.margin_ulps(x[q], radv[q]) for q in range(x.shape[0]) if np.isfinite(radv[q]) and x.shape[1]], default=np.inf)
