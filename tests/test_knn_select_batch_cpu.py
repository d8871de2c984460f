"""CPU suite of the filtered search over the prepared store (ac_knn_*_topk_batch_sel): the ABI additions, the argument checks that
return before any device work, the host-side routing policy (which selector takes the prepared store) with the low-level calls
replaced by recorders, and the gaps that let tests/test_knn_select_batch_gpu.py compare ids with the oracle for every query."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import knn_select_batch_ref as bref  # noqa: E402
import knn_select_ref as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("ac_knn_l2_topk_batch_sel", "ac_knn_ip_topk_batch_sel")


# ---- ABI -------------------------------------------------------------------------------------------------------------------------
def test_symbols_in_header_library_and_ctypes_table():
    from adaptive_classifier import _native as nv
    L = nv.lib()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "acamd.h")).read(), flags=re.S)
    exports = subprocess.run(["nm", "-D", "--defined-only", L._name], capture_output=True, text=True, check=True).stdout
    for name in ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), f"{name} is not declared in acamd.h"
        assert re.search(r"\sT\s+%s$" % name, exports, flags=re.M), f"{name} is not exported by libacamd.so"
        assert name in nv.exported_symbols() and hasattr(L, name)
    assert L.ac_version() >= 6


def _args(N, D, nq, k, d_sel, bit0, ws_bytes, a):
    p = ctypes.c_void_p
    #       d_P   N  ldP D  planes norms d_Q  nq  ldQ k  row_offset sel    bit0  outD  outD64 outI  ws    ws_bytes  stats stream
    return [p(a), N, D, D, p(a), p(a), p(a), nq, D, k, 0, d_sel, bit0, p(a), None, p(a), p(a), ws_bytes, None, None]


def test_argument_checks_return_before_any_device_work():
    from adaptive_classifier import _native as nv
    L = nv.lib()
    buf = (ctypes.c_uint64 * 64)()
    a = ctypes.addressof(buf)
    p = ctypes.c_void_p
    N, D, nq, k = 70000, 64, 5, 32
    need, plain = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert L.ac_knn_l2_topk_batch_workspace(N, D, nq, k, ctypes.byref(need)) == 0 and need.value > 0
    for name in ENTRIES:
        fn = getattr(L, name)
        assert fn(*_args(N, D, nq, k, None, 0, need.value, a)) == -1 and b"d_sel" in L.ac_last_error()                 # NULL d_sel
        assert fn(*_args(N, D, nq, k, p(a + 4), 0, need.value, a)) == -1 and b"aligned" in L.ac_last_error()           # misaligned
        assert fn(*_args(N, D, nq, k, p(a), -1, need.value, a)) == -1 and b"sel_bit0" in L.ac_last_error()
        assert fn(*_args(65535, D, nq, k, p(a), 0, need.value, a)) == -2 and b"N=65535" in L.ac_last_error()           # the batch limits
        assert fn(*_args(N, D, nq, 101, p(a), 0, need.value, a)) == -2 and b"k=101" in L.ac_last_error()
        # the workspace is the unfiltered batch search's: one byte less than its planner's figure is refused with that figure
        for shape in ((N, D, nq, k), (N, D, 300, k)):
            assert L.ac_knn_l2_topk_batch_workspace(*shape, ctypes.byref(plain)) == 0
            assert fn(*_args(*shape, p(a), 0, plain.value - 1, a)) == -3 and (b"required %d" % plain.value) in L.ac_last_error()


def test_filtered_batch_search_fails_loudly_without_gpu():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from adaptive_classifier import _native as nv
    from adaptive_classifier import index as ix
    sel = ix.RowSelector.from_mask(np.ones(70000, dtype=bool), device="cpu")
    P, Q = torch.zeros((70000, 8)), torch.zeros((2, 8))
    with pytest.raises(nv.NativeError):
        ix.knn_topk_sel(P, 70000, 8, Q, 4, sel, prepared=(torch.zeros(8, dtype=torch.int16), torch.zeros(8)))
    with pytest.raises(nv.NativeError):
        ix.prepare_store(P, 70000, 8)


# ---- the selector's known count --------------------------------------------------------------------------------------------------
def test_row_selector_known_count():
    from adaptive_classifier.index import RowSelector
    n = 1000
    mask = np.random.default_rng(1).random(n) < 0.3
    ids = np.nonzero(mask)[0]
    rc = np.arange(n, dtype=np.int32) % 5
    assert RowSelector.from_mask(mask, device="cpu").known_count == int(mask.sum())
    assert RowSelector.from_mask(torch.from_numpy(mask), device="cpu").known_count == int(mask.sum())
    assert RowSelector.from_ids(np.concatenate([ids[::-1], ids[:7], [-1, n]]), n, device="cpu").known_count == ids.size
    assert RowSelector.from_range(-3, 40, n, device="cpu").known_count == 40
    assert RowSelector.from_range(990, 2000, n, device="cpu").known_count == 10
    assert RowSelector.from_classes(rc, [1, 3, 9], 5, device="cpu").known_count == 400
    unknown = RowSelector(RowSelector.from_mask(mask, device="cpu").words, n)           # (what a device builder returns)
    assert unknown.known_count is None and unknown.to("cpu").known_count is None
    assert unknown.count() == int(mask.sum()) and unknown.known_count == int(mask.sum())
    unknown.words = None                                                                 # count() cached: the bitmap is not read again
    assert unknown.count() == int(mask.sum())
    known = RowSelector.from_mask(mask, device="cpu")
    moved = known.to("cpu")
    assert moved is not known and moved.known_count == known.known_count and moved.n == n


# ---- routing policy --------------------------------------------------------------------------------------------------------------
class _Recorder:
    def __init__(self, monkeypatch):
        from adaptive_classifier import index as ix
        self.calls, self.prepared = [], 0
        monkeypatch.setattr(ix, "knn_topk_sel", lambda *a, **kw: self.calls.append(("sel", kw.get("prepared"), kw)) or ("D", "I"))
        monkeypatch.setattr(ix, "knn_topk_ids", lambda *a, **kw: self.calls.append(("ids", None, kw)) or ("D", "I"))
        monkeypatch.setattr(ix, "knn_workspace_bytes", lambda *a: 256)
        monkeypatch.setattr(ix, "knn_batch_workspace_bytes", lambda *a: 512)
        monkeypatch.setattr(ix, "prepare_store", self._prepare)

    def _prepare(self, *a, **kw):
        self.prepared += 1
        return ("planes", "norms")

    def last(self):
        return self.calls[-1][:2]


def _host_index(monkeypatch, n):
    from adaptive_classifier import index as ix
    idx = ix.HipFlatL2Index(8, device="cpu")
    idx._n, idx._store = n, torch.zeros((4, 8))
    monkeypatch.setattr(idx, "_materialize", lambda: None)
    return idx


def test_index_routing_policy(monkeypatch):
    from adaptive_classifier import index as ix
    n = 400000                                                # >= PLANE_MIN_ROWS, and 64 queries make BATCH_MIN_PAIRS
    rec = _Recorder(monkeypatch)
    idx = _host_index(monkeypatch, n)
    q64, q8 = torch.zeros((64, 8)), torch.zeros((8, 8))
    half = np.random.default_rng(2).random(n) < 0.5
    dense = ix.RowSelector.from_mask(half, device="cpu")
    # unknown count: the fp32 route, nothing prepared -- what every caller got before
    unknown = ix.RowSelector(dense.words, n)
    idx.search_device(q64, 8, unknown)
    assert rec.last() == ("sel", None) and rec.prepared == 0 and idx._prepared is None
    # a known dense count with few queries and no plane: still the fp32 route, nothing prepared
    idx.search_device(q8, 8, dense)
    assert rec.last() == ("sel", None) and rec.prepared == 0
    # a known dense count, >= BATCH_MIN_QUERIES queries: prepared at once, the prepared route with the batch workspace
    idx.search_device(q64, 8, dense)
    assert rec.last() == ("sel", ("planes", "norms")) and rec.prepared == 1 and idx._ws.numel() >= 512
    # ... and now that a plane exists, the small batch uses it
    idx.search_device(q8, 8, dense)
    assert rec.last() == ("sel", ("planes", "norms")) and rec.prepared == 1
    # the unknown selector still keeps the fp32 route -- until count() is called
    idx.search_device(q64, 8, unknown)
    assert rec.last() == ("sel", None)
    assert unknown.count() == int(half.sum())
    idx.search_device(q64, 8, unknown)
    assert rec.last() == ("sel", ("planes", "norms"))
    # known and sparse (count * 32 < n): the fp32 route; exactly 1 / 32: the prepared route
    m = np.zeros(n, dtype=bool); m[: n // 32 - 1] = True
    idx.search_device(q64, 8, ix.RowSelector.from_mask(m, device="cpu"))
    assert rec.last() == ("sel", None)
    m[: (n + 31) // 32] = True
    idx.search_device(q64, 8, ix.RowSelector.from_mask(m, device="cpu"))
    assert rec.last() == ("sel", ("planes", "norms"))
    # more than KNN_IDS_MAX host ids but sparse: the bitmap over the fp32 rows; <= KNN_IDS_MAX host ids: the id-list route
    idx.search_device(q64, 8, ix.RowSelector.from_ids(np.arange(0, 9000 * 3, 3), n, device="cpu"))
    assert rec.last() == ("sel", None)
    idx.search_device(q64, 8, ix.RowSelector.from_ids(np.arange(ix.KNN_IDS_MAX), n, device="cpu"))
    assert rec.last() == ("ids", None)
    # outside the prepared-store limits nothing changes route: k > 100, a store below 65536 rows
    idx.search_device(q64, 101, dense)
    assert rec.last() == ("sel", None)
    small = _host_index(monkeypatch, 60000)
    small.search_device(q64, 8, ix.RowSelector.from_mask(np.ones(60000, dtype=bool), device="cpu"))
    assert rec.last() == ("sel", None) and small._prepared is None and rec.prepared == 1


def test_sharded_routing_policy(monkeypatch):
    from adaptive_classifier import index as ix
    from adaptive_classifier.sharded import ShardedSearch
    rec = _Recorder(monkeypatch)
    n_local, total, off = 150000, 300000, 150000
    ss = ShardedSearch(torch.zeros((4, 8)), n_local, 8, off, local_search=lambda *a: None, merge=lambda *a: a)
    q = torch.zeros((300, 8))
    half = np.random.default_rng(2).random(total) < 0.5
    dense = ix.RowSelector.from_mask(half, device="cpu")
    ss._local(q, 8, ix.RowSelector(dense.words, total))                                   # unknown count
    assert rec.last() == ("sel", None) and ss._prepared is None
    ss._local(q, 8, dense)                                                                # the GLOBAL count over the GLOBAL rows
    kind, prepared, kw = rec.calls[-1]
    assert (kind, prepared) == ("sel", ("planes", "norms")) and kw["sel_bit0"] == off and kw["row_offset"] == off and rec.prepared == 1
    # dense inside this shard only, sparse globally: the fp32 route
    m = np.zeros(total, dtype=bool); m[off: off + total // 32 - 1] = True
    ss._local(q, 8, ix.RowSelector.from_mask(m, device="cpu"))
    assert rec.last() == ("sel", None)


# ---- gaps ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("N,D,nq,k,qstep", bref.ORACLE_CASES + [bref.INDEX_CASE], ids=bref.ORACLE_IDS + ["index"])
def test_cases_have_order_independent_results(N, D, nq, k, qstep, metric):
    """every (shape, metric, selection) whose ids the GPU file compares with the oracle: the deciding ranks lie >= 2^-40 apart"""
    _, _, x = bref.case(N, D, nq, metric, qstep)
    for name in bref.SELECTIONS:
        gap = ref.min_rel_gap(x, bref.selection(name, N, k), k, metric)
        print(N, D, nq, k, metric, name, "min relative gap %.3g" % gap)
        assert gap >= ref.MIN_GAP


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_cluster_case_has_order_independent_results(metric):
    N, _, _, k = bref.CLUSTER
    _, _, x = bref.cluster_case(metric)
    gap = ref.min_rel_gap(x, bref.selection("half", N, k), k, metric)
    print("cluster", metric, "min relative gap %.3g" % gap)
    assert gap >= ref.MIN_GAP
