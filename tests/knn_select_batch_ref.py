"""TEST INFRASTRUCTURE -- shapes, selections and inputs of the filtered search over the PREPARED store
(ac_knn_*_topk_batch_sel), shared by tests/test_knn_select_batch_cpu.py (gaps) and tests/test_knn_select_batch_gpu.py (results).
The oracle is knn_select_ref.filtered_topk; inputs are computed once per process and never modified.

Every shape has N >= 65536, the floor of the prepared-store route; each is the smallest that reaches its code path."""
import functools

import numpy as np

import knn_range_ref as rref
import knn_select_ref as ref

# (N, D, nq, k, qstep): the oracle runs on queries [::qstep] (every query is compared bit for bit with the fp32 filtered route)
ORACLE_CASES = [
    (70000, 64, 5, 32, 1),       # ref.CASES[4]: plane sweep, 32-query tile
    (65537, 32, 1, 16, 1),       # ref.CASES[6]: plane sweep, one row in the last tile and in the last word
    (66000, 96, 40, 10, 1),      # plane sweep, 64-query tile
    (70001, 100, 65, 8, 1),      # GEMM form, D % 16 != 0, ragged tiles; two-phase thresholds or sample stages (AC_KNN_TWO_PHASE)
    (65536, 32, 260, 100, 1),    # two query tiles (the second ragged): sample stages; the largest k
    (600000, 32, 65, 8, 9),      # a big store: two-phase thresholds, or (AC_KNN_TWO_PHASE=0) two sample stages at a large stride
]
ORACLE_IDS = ["plane32", "plane32-last-word", "plane64", "gemm-ragged", "two-query-tiles-k100", "big-store"]
INDEX_CASE = (80000, 32, 256, 8, 16)
SELECTIONS = ["half", "sparse", "block", "tiny", "empty"]


def selection(name, N, k):
    """knn_select_ref.selection plus tiny = rows 3, N // 2, N - 1 and empty"""
    if name == "tiny":
        m = np.zeros(N, dtype=bool)
        m[[3, N // 2, N - 1]] = True
        return m
    if name == "empty":
        return np.zeros(N, dtype=bool)
    return ref.selection(name, N, k)


@functools.lru_cache(maxsize=None)
def case(N, D, nq, metric, qstep=1):
    """(P, Q [nq], exact values of queries [::qstep]): unit Gaussian rows, seeds 1 (rows) and 2 (queries); read-only"""
    if qstep == 1:
        return ref.case(N, D, nq, metric)
    P, Q = rref.unit_rows(N, D, 1), rref.unit_rows(nq, D, 2)
    x = rref.fixed_order_values(P, Q[::qstep], metric)
    for a in (P, Q, x):
        a.setflags(write=False)
    return P, Q, x


CLUSTER = (70000, 128, 80, 8)       # one tight cluster: every sweep value lies within the fp16 bound of every other


@functools.lru_cache(maxsize=None)
def cluster_case(metric):
    """(P, Q, exact values): rows and queries = one unit centre + 1e-4 * Gaussian noise -- no certificate can hold, every query is
    answered by the fp64 fallback over the selected rows"""
    N, D, nq, _ = CLUSTER
    c = rref.unit_rows(1, D, 7)[0].astype(np.float64)
    P = (c + 1e-4 * np.random.default_rng(8).standard_normal((N, D))).astype(np.float32)
    Q = (c + 1e-4 * np.random.default_rng(9).standard_normal((nq, D))).astype(np.float32)
    x = rref.fixed_order_values(P, Q, metric)
    for a in (P, Q, x):
        a.setflags(write=False)
    return P, Q, x
