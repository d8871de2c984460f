"""CPU suite of the filtered search: the oracle and its gap helper, the bit layout of RowSelector, the ABI additions (version,
argument checks that return before any device work, the shared workspace plan) and the host-side behaviour without a GPU."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import knn_select_ref as ref  # noqa: E402


# ---- oracle ----------------------------------------------------------------------------------------------------------------------
def test_oracle_orders_filters_and_pads():
    P = np.array([[0.0], [1.0], [1.0], [3.0], [-2.0]], dtype=np.float32)
    Q = np.array([[1.0]], dtype=np.float32)
    mask = np.array([True, False, True, True, True])
    D, I, E = ref.filtered_topk(P, Q, 3, mask, "l2")
    assert I.tolist() == [[2, 0, 3]] and D.tolist() == [[0.0, 1.0, 4.0]]            # row 1 (distance 0) is unselected
    D, I, E = ref.filtered_topk(P, Q, 6, mask, "ip", row_offset=10)
    assert I.tolist() == [[13, 12, 10, 14, -1, -1]]
    assert D[0, :4].tolist() == [3.0, 1.0, 0.0, -2.0] and np.all(D[0, 4:] == -ref.FLT_MAX) and np.all(np.isneginf(E[0, 4:]))
    P2 = np.zeros((4, 2), dtype=np.float32)                                          # ties: the lower id first
    assert ref.filtered_topk(P2, np.zeros((1, 2), np.float32), 2, [False, True, True, True], "l2")[1].tolist() == [[1, 2]]
    assert ref.filtered_topk(P2, np.zeros((1, 2), np.float32), 2, [False] * 4, "l2")[1].tolist() == [[-1, -1]]
    assert np.all(ref.filtered_topk(P2, np.zeros((1, 2), np.float32), 2, [False] * 4, "l2")[0] == ref.FLT_MAX)


def test_gap_helper():
    x = np.array([[1.0, 1.0, 2.0, 2.5, 9.0]])
    assert ref.min_rel_gap(x, [True] * 5, 2) == pytest.approx(0.5)                  # best 3: 1, 1, 2 -> distinct 1, 2
    assert ref.min_rel_gap(x, [True, True, False, True, True], 2) == pytest.approx(0.6)
    assert ref.min_rel_gap(x, [True, True, False, False, False], 4) == np.inf
    assert ref.min_rel_gap(-x, [True] * 5, 2, "ip") == pytest.approx(0.5)


@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("N,D,nq,k", ref.CASES)
def test_cases_have_order_independent_results(N, D, nq, k, metric):
    """every shape x metric x selection of the GPU oracle test: the ranks that decide the result lie >= 2^-40 apart (relative),
    so the ids do not depend on the order in which an exact value is summed -- no query needs to be left out"""
    _, _, x = ref.case(N, D, nq, metric)
    for name in ref.SELECTIONS:
        gap = ref.min_rel_gap(x, ref.selection(name, N, k), k, metric)
        print(N, D, nq, k, metric, name, "min relative gap %.3g" % gap)
        assert gap >= ref.MIN_GAP


# ---- bit layout ------------------------------------------------------------------------------------------------------------------
def _words(sel):
    return sel.words.cpu().numpy().view(np.uint64)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000, 4097])
def test_row_selector_bit_layout(n):
    from adaptive_classifier.index import RowSelector
    mask = np.random.default_rng(n).random(n) < 0.4
    want = np.zeros((n + 63) // 64 * 8, dtype=np.uint8)
    raw = np.packbits(mask, bitorder="little")
    want[: raw.size] = raw
    want = want.view("<u8")
    for sel in (RowSelector.from_mask(mask, device="cpu"), RowSelector.from_mask(torch.from_numpy(mask), device="cpu")):
        assert sel.n == n and sel.words.dtype == torch.int64 and sel.ids is None
        assert np.array_equal(_words(sel), want)
        assert (int(_words(sel)[-1]) >> ((n - 1) % 64 + 1)) == 0 or n % 64 == 0       # tail bits are zero
        assert sel.count() == int(mask.sum())
    ids = np.nonzero(mask)[0]
    shuffled = np.concatenate([ids[::-1], ids[:3], [-4, n, n + 70]])                   # unsorted, duplicates, out of range
    sel = RowSelector.from_ids(shuffled, n, device="cpu")
    assert np.array_equal(_words(sel), want) and np.array_equal(sel.ids.numpy(), ids) and sel.ids.dtype == torch.int64
    lo, hi = n // 4, n // 4 + max(n // 2, 1)
    rmask = np.zeros(n, dtype=bool); rmask[lo:hi] = True
    assert np.array_equal(_words(RowSelector.from_range(lo, hi, n, device="cpu")), ref.pack(rmask))
    assert np.array_equal(_words(RowSelector.from_range(-5, n + 9, n, device="cpu")), ref.pack(np.ones(n, dtype=bool)))
    assert np.array_equal(ref.pack(mask), want)                                         # the test helper speaks the same layout


def test_row_selector_from_classes_host():
    from adaptive_classifier.index import RowSelector
    rc = np.array([0, 1, 2, -1, 5, 4, 1, 3], dtype=np.int32)
    sel = RowSelector.from_classes(rc, [1, 4, 9], 5, device="cpu")                      # class 5 = n_classes and -1: unselected
    assert np.array_equal(_words(sel), ref.pack(np.array([0, 1, 0, 0, 0, 1, 1, 0], dtype=bool))) and sel.n == 8
    assert RowSelector.from_classes(torch.from_numpy(rc), [], 5, device="cpu").count() == 0


# ---- ABI -------------------------------------------------------------------------------------------------------------------------
def _sel_args(L, N, D, nq, k, d_sel, bit0, ws_bytes):
    buf = (ctypes.c_uint64 * 64)()
    a = ctypes.addressof(buf)
    p = ctypes.c_void_p
    return [p(a), N, D, D, p(a), nq, D, k, 0, d_sel, bit0, p(a), None, p(a), p(a), ws_bytes, None, None], buf


def test_abi_version_and_argument_checks():
    from adaptive_classifier import _native as nv
    L = nv.lib()
    assert L.ac_version() >= 5
    need = ctypes.c_size_t(0)
    N, D, nq, k = 5000, 768, 7, 16
    assert L.ac_knn_l2_topk_workspace(N, D, nq, k, ctypes.byref(need)) == 0
    buf = (ctypes.c_uint64 * 64)()
    a = ctypes.addressof(buf)
    for name in ("ac_knn_l2_topk_sel", "ac_knn_ip_topk_sel"):
        fn = getattr(L, name)
        args, keep = _sel_args(L, N, D, nq, k, None, 0, need.value)
        assert fn(*args) == -1 and b"d_sel" in L.ac_last_error()                        # NULL d_sel with N > 0
        args, keep = _sel_args(L, N, D, nq, k, ctypes.c_void_p(a + 4), 0, need.value)
        assert fn(*args) == -1 and b"d_sel" in L.ac_last_error() and b"aligned" in L.ac_last_error()
        args, keep = _sel_args(L, N, D, nq, k, ctypes.c_void_p(a), -1, need.value)
        assert fn(*args) == -1 and b"sel_bit0" in L.ac_last_error()
        # the plan -- hence the workspace -- is ac_knn_l2_topk_workspace's: one byte less is refused with that very figure ...
        args, keep = _sel_args(L, N, D, nq, k, ctypes.c_void_p(a), 0, need.value - 1)
        assert fn(*args) == -3 and (b"required %d" % need.value) in L.ac_last_error()
        # ... and a call with no query accepts it and does nothing
        args, keep = _sel_args(L, N, D, 0, k, ctypes.c_void_p(a), 0, need.value)
        assert fn(*args) == 0
    p = ctypes.c_void_p
    for name in ("ac_knn_l2_topk_ids", "ac_knn_ip_topk_ids"):
        fn = getattr(L, name)
        assert fn(p(a), N, D, D, p(a), 8193, p(a), nq, D, k, 0, p(a), None, p(a), None) == -1 and b"M=8193" in L.ac_last_error()
        assert fn(p(a), N, D, D, p(a), -1, p(a), nq, D, k, 0, p(a), None, p(a), None) == -1 and b"M=-1" in L.ac_last_error()
        assert fn(p(a), N, D, D, None, 5, p(a), nq, D, k, 0, p(a), None, p(a), None) == -1 and b"d_ids" in L.ac_last_error()
        assert fn(p(a), N, D, D, p(a), 8192, p(a), 0, D, k, 0, p(a), None, p(a), None) == 0     # no query: nothing to do
    assert L.ac_knn_sel_pack(None, 5, p(a), None) == -1 and b"d_mask" in L.ac_last_error()
    assert L.ac_knn_sel_pack(p(a), 5, p(a + 4), None) == -1 and b"d_sel" in L.ac_last_error()
    assert L.ac_knn_sel_pack(p(a), 0, None, None) == 0
    assert L.ac_knn_sel_classes(p(a), 5, p(a), -1, p(a), None) == -1 and b"n_classes" in L.ac_last_error()
    assert L.ac_knn_sel_classes(None, 0, None, 0, None, None) == 0


# ---- host behaviour without a GPU ------------------------------------------------------------------------------------------------
def test_filtered_search_fails_loudly_without_gpu_and_unfiltered_bookkeeping_is_untouched():
    from adaptive_classifier import _native as nv
    from adaptive_classifier.index import HipFlatIPIndex, HipFlatL2Index, RowSelector
    for cls in (HipFlatL2Index, HipFlatIPIndex):
        idx = cls(8)
        idx.add(torch.zeros(3, 8))
        idx.add(torch.ones(2, 8))
        assert idx.ntotal == 5 and idx._prepared is None and idx._searches_since_change == 0      # sel=None: host bookkeeping as ever
        if torch.cuda.is_available():
            continue
        for sel in (np.array([True, False, True, True, False]), [0, 2], RowSelector.from_ids([1], 5, device="cpu")):
            with pytest.raises(nv.NativeError):
                idx.search(np.zeros((1, 8), np.float32), 1, sel=sel)
        with pytest.raises(nv.NativeError):
            idx.search(np.zeros((1, 8), np.float32), 1)
        assert idx.ntotal == 5


def test_sharded_fixed_batch_path_refuses_a_selector():
    from adaptive_classifier.index import RowSelector
    from adaptive_classifier.sharded import ShardedSearch
    rows = torch.zeros(10, 8)
    calls = []
    ss = ShardedSearch(rows, 10, 8, 0, block_rows=4, local_search=lambda *a: calls.append(a), merge=lambda *a: a)
    with pytest.raises(ValueError):
        ss.search_block(torch.zeros(2, 8), 3, sel=RowSelector.from_range(0, 5, 10, device="cpu"))
    assert not calls
