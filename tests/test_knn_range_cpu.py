"""CPU suite of the range search: the oracle's own properties, the workspace planner's accept / reject rule, the ABI version,
the loud failure without a GPU and the host-side chunk arithmetic of knn_range_search.  No GPU needed."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import knn_range_ref as ref  # noqa: E402


def _int_rows(n, D, seed):
    return np.random.default_rng(seed).integers(-3, 4, (n, D)).astype(np.float32)


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_oracle_on_integer_rows_is_exact_and_strict(metric):
    P, Q = _int_rows(300, 24, 1), _int_rows(3, 24, 2)
    x = ref.fixed_order_values(P, Q, metric)
    exact = ((P[None].astype(np.int64) - Q[:, None].astype(np.int64)) ** 2).sum(-1) if metric == "l2" else \
        (P[None].astype(np.int64) * Q[:, None].astype(np.int64)).sum(-1)
    assert np.array_equal(x, exact.astype(np.float64))                  # integer arithmetic: every sum is exact
    for q in range(3):
        vals, counts = np.unique(exact[q], return_counts=True)
        v = vals[counts > 1][len(vals[counts > 1]) // 2]               # a value several rows share
        held = np.nonzero(exact[q] == v)[0]
        lims, D, I = ref.range_search(P, Q[q:q + 1], np.float32(v), metric)
        assert not np.isin(held, I).any()                               # strict: none of the rows AT the radius
        better = exact[q] < v if metric == "l2" else exact[q] > v
        assert np.array_equal(I, np.nonzero(better)[0]) and lims.tolist() == [0, int(better.sum())]
        step = np.nextafter(np.float32(v), np.float32(np.inf if metric == "l2" else -np.inf))
        _, _, I2 = ref.range_search(P, Q[q:q + 1], step, metric)
        assert np.isin(held, I2).all() and I2.size == better.sum() + held.size      # one fp32 step further: all of them
        assert np.all(np.diff(I2) > 0)                                  # ascending row ids


def test_oracle_edge_radii_and_helpers():
    P, Q = _int_rows(50, 8, 3), _int_rows(4, 8, 4)
    for r in (0.0, -1.0, np.nan):
        assert ref.range_search(P, Q, r, "l2")[0].tolist() == [0] * 5
    lims, D, I = ref.range_search(P, Q, np.inf, "l2", row_offset=10 ** 10)
    assert lims.tolist() == [0, 50, 100, 150, 200] and np.array_equal(I[:50], np.arange(50) + 10 ** 10)
    assert ref.range_search(P, Q, -np.inf, "ip")[0][-1] == 200 and ref.range_search(P, Q, np.inf, "ip")[0][-1] == 0
    assert ref.range_search(P, Q, np.nan, "ip")[0][-1] == 0
    lims, _, _ = ref.range_search(P, Q, np.array([np.inf, 0, np.inf, 0], np.float32), "l2")       # one radius per query
    assert lims.tolist() == [0, 50, 50, 100, 100]
    assert ref.range_search(P[:0], Q, 1.0)[0].tolist() == [0] * 5 and ref.range_search(P, Q[:0], 1.0)[0].tolist() == [0]
    s = np.array([1, 2, 3, 10, 11, 30], np.float32)
    assert ref.gap_radius(s, 0, 4) == np.float32(6.5) and ref.gap_radius(s, 0, 5) == np.float32(20.5)
    assert ref.gap_radius(s[::-1], 0, 2) == np.float32(20.5)            # descending input (ip)
    assert ref.margin_ulps(s, np.float32(6.5)) == 3.5 / np.spacing(np.float32(6.5))


@pytest.mark.parametrize("N,D,nq", [(5000, 768, 33), (1153, 100, 17), (70000, 64, 5)])
def test_gap_radii_leave_a_wide_margin_on_the_gpu_test_shapes(N, D, nq):
    """what tests/test_knn_range_gpu.py relies on (it asserts margin_ulps >= 64 before it compares ids): on its shapes the gap
    radii of ranks 20..60 admit 21..60 rows and keep every value thousands of ulps away (smallest: 6582 ulps at 5000 x 768 l2)"""
    P, Q = ref.unit_rows(N, D, 1), ref.unit_rows(nq, D, 2)
    for metric in ("l2", "ip"):
        x = ref.fixed_order_values(P, Q, metric)
        rad = ref.gap_radii(x, metric, 20, 60)
        lims = ref.range_search(P, Q, rad, metric, values=x)[0]
        hits = np.diff(lims)
        assert hits.min() >= 21 and hits.max() <= 60, hits
        assert min(ref.margin_ulps(x[q], rad[q]) for q in range(nq)) >= 64


def test_range_workspace_follows_the_topk_planner():
    from adaptive_classifier import _native as nv
    L = nv.lib()
    assert L.ac_version() >= 4
    b, t = ctypes.c_size_t(0), ctypes.c_size_t(0)
    for N, D, nq in [(100, 4096, 3), (100000, 4096, 3), (10_000_000, 768, 16), (8192, 4096, 1), (8193, 4096, 1), (0, 16, 4),
                     (5000, 768, 33), (1000, 2560, 2), (100000, 2600, 2)]:
        assert L.ac_knn_range_workspace(N, D, nq, ctypes.byref(b)) == L.ac_knn_l2_topk_workspace(N, D, nq, 1, ctypes.byref(t)), (N, D, nq)
    assert L.ac_knn_range_workspace(100, 4096, 3, ctypes.byref(b)) == 0
    assert L.ac_knn_range_workspace(100000, 4096, 3, ctypes.byref(b)) == -2
    assert b"D=4096" in L.ac_last_error()
    assert L.ac_knn_range_workspace(10_000_000, 768, 16, ctypes.byref(b)) == 0
    assert b.value >= 16 * ((10_000_000 + 63) // 64) * 8               # at least the membership bitmap
    assert L.ac_knn_range_workspace(100, 8, 3, None) == -1


def test_range_search_fails_loudly_without_gpu():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from adaptive_classifier import _native as nv
    from adaptive_classifier.index import HipFlatIPIndex, HipFlatL2Index
    for cls in (HipFlatL2Index, HipFlatIPIndex):
        idx = cls(8)
        idx.add(torch.zeros(3, 8))
        with pytest.raises(nv.NativeError):
            idx.range_search(np.zeros((1, 8), np.float32), 1.0)        # no CPU search path exists


def test_chunk_results_are_stitched_with_lims_offsets():
    from adaptive_classifier.index import range_query_chunk, stitch_range_chunks
    t = lambda a, dt: torch.tensor(a, dtype=dt)
    parts = [(t([0, 2, 2], torch.int64), t([.1, .2], torch.float32), t([5, 9], torch.int64)),
             (t([0, 0], torch.int64), t([], torch.float32), t([], torch.int64)),                    # a chunk without hits
             (t([0, 1, 4], torch.int64), t([.3, .4, .5, .6], torch.float32), t([1, 0, 2, 7], torch.int64))]
    lims, D, I = stitch_range_chunks(parts)
    assert lims.tolist() == [0, 2, 2, 2, 3, 6] and lims.dtype == torch.int64
    assert I.tolist() == [5, 9, 1, 0, 2, 7] and torch.equal(D, t([.1, .2, .3, .4, .5, .6], torch.float32))
    one = stitch_range_chunks(parts[:1])
    assert one[0].tolist() == [0, 2, 2]
    lims0, D0, I0 = stitch_range_chunks([])
    assert lims0.tolist() == [0] and D0.numel() == 0 and I0.dtype == torch.int64
    # queries per call: the largest count whose workspace fits, never below one
    from adaptive_classifier.index import knn_range_workspace_bytes as wsb
    for N, D, nq, cap in [(70000, 64, 40, 100_000), (70000, 64, 40, 1 << 28), (70000, 64, 40, 1), (1000, 4096, 9, 2000)]:
        c = range_query_chunk(N, D, nq, cap)
        assert 1 <= c <= nq and (c == 1 or wsb(N, D, c) <= cap)
    assert range_query_chunk(70000, 64, 40, 1 << 28) == 40 and range_query_chunk(70000, 64, 40, 1) == 1
    assert 40 / range_query_chunk(70000, 64, 40, 100_000) >= 3         # the GPU chunking test's setting: >= 3 chunks
