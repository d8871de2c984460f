"""Filtered top-k search over the PREPARED store on the GPU (ac_knn_*_topk_batch_sel through the C ABI, then the flat indexes,
PrototypeMemory and ShardedSearch).

Two bars for every case: ids EQUAL to the fp64 oracle tests/knn_select_ref.py (tests/test_knn_select_batch_cpu.py asserts that the
deciding ranks lie >= 2^-40 apart, so no query is left out; big cases run the oracle on a strided subset of the queries), and
D, I and exact_out BIT-EQUAL to ac_knn_*_topk_sel -- the filtered search over the fp32 rows, itself oracle-tested -- for all of
them.  d_stats[0] (queries answered by the fp64 fallback) is bounded: thresholds that counted unselected rows, or a missing
certificate rule, would send whole batches there."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import knn_range_ref as rref  # noqa: E402
import knn_select_batch_ref as bref  # noqa: E402
import knn_select_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
METRICS = ["l2", "ip"]


def _ulp_close(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    with np.errstate(over="ignore"):
        return a.shape == b.shape and np.all(np.abs(a - b) <= np.spacing(np.maximum(np.abs(a), np.abs(b)).astype(np.float32)))


def _store(P, dev):
    ld = (P.shape[1] + 3) // 4 * 4
    store = torch.zeros((P.shape[0], ld), dtype=torch.float32, device=dev)
    store[:, : P.shape[1]] = torch.tensor(P, device=dev)
    return store


def _words(mask_or_words, dev):
    w = mask_or_words if mask_or_words.dtype == np.uint64 else ref.pack(mask_or_words)
    return torch.from_numpy(w.view(np.int64).copy()).to(dev)


def _call(entry, store, N, D, Qd, k, dev, prepared=None, sel=None, sel_bit0=0, row_offset=0, ws=None):
    """one search through the C ABI: entry = 'l2_topk_batch_sel' | 'ip_topk_sel' | 'l2_topk_batch' ... -> (D, I, exact), stats"""
    from adaptive_classifier import _native as nv
    L = nv.lib()
    nq = Qd.shape[0]
    need = ctypes.c_size_t(0)
    planner = L.ac_knn_l2_topk_batch_workspace if "batch" in entry else L.ac_knn_l2_topk_workspace
    assert planner(N, D, nq, k, ctypes.byref(need)) == 0
    if ws is None:
        ws = torch.empty(max(need.value, 256), dtype=torch.uint8, device=dev)
    assert ws.numel() >= need.value
    outD = torch.empty((nq, k), dtype=torch.float32, device=dev)
    outE = torch.empty((nq, k), dtype=torch.float64, device=dev)
    outI = torch.empty((nq, k), dtype=torch.int64, device=dev)
    stats = torch.full((4,), -7, dtype=torch.int32, device=dev)
    head = [nv.ptr(store), N, store.stride(0), D]
    if "batch" in entry:
        head += [nv.ptr(prepared[0]), nv.ptr(prepared[1])]
    head += [nv.ptr(Qd), nq, Qd.stride(0), k, row_offset]
    mid = [nv.ptr(sel), sel_bit0] if entry.endswith("_sel") else []
    tail = [nv.ptr(outD), nv.ptr(outE), nv.ptr(outI), nv.ptr(ws), ws.numel(), nv.ptr(stats), nv.stream_ptr(dev)]
    with torch.cuda.device(dev):
        nv.check(getattr(L, "ac_knn_" + entry)(*(head + mid + tail)), entry)
    torch.cuda.synchronize()
    return (outD, outI, outE), stats.tolist()


def _assert_oracle(got, want, metric):
    (D, I, E), (oD, oI, oE) = [tuple(t.cpu().numpy() if torch.is_tensor(t) else t for t in g) for g in (got, want)]
    assert np.array_equal(I, oI), f"id mismatch in {(I != oI).any(axis=1).sum()} of {I.shape[0]} queries"
    assert _ulp_close(D, oD)
    real = I >= 0
    assert np.array_equal(E[real].astype(np.float32), D[real])               # D is the fp64 output rounded once
    assert np.all(np.isinf(E[~real])) and np.all(np.sign(E[~real]) == (-1 if metric == "ip" else 1))      # padding values are exact
    assert np.all(D[~real] == (-ref.FLT_MAX if metric == "ip" else ref.FLT_MAX))


def _assert_same_bits(a, b, what=""):
    for t, u, name in zip(a, b, ("D", "I", "exact_out")):
        assert torch.equal(t, u), f"{name} differs {what}"


@functools.lru_cache(maxsize=None)
def _dev_store(key, dev):
    """(rows, queries, prepared store) on the device for a shape of knn_select_batch_ref, or the cluster case"""
    from adaptive_classifier import index as ix
    if key == "cluster":
        P, Q, _ = bref.cluster_case("l2")
    else:
        N, D, nq, qstep = key
        P, Q, _ = bref.case(N, D, nq, "l2", qstep)
    store = _store(P, dev)
    return store, torch.tensor(Q, device=dev), ix.prepare_store(store, P.shape[0], P.shape[1])


# ---- 1. oracle equality, bit equality with the fp32 filtered route, fallback counts ------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("ci,two_phase", [(0, None), (1, None), (2, None), (3, "1"), (3, "0"), (4, None), (5, None), (5, "0")],
                         ids=["plane32", "plane32-last-word", "plane64", "gemm-ragged-two-phase", "gemm-ragged-sample-stages",
                              "two-query-tiles-k100", "big-store", "big-store-two-sample-stages"])
def test_filtered_batch_matches_oracle_and_fp32_route(ci, two_phase, metric, cuda_dev, monkeypatch):
    N, D, nq, k, qstep = bref.ORACLE_CASES[ci]
    if two_phase is not None:
        monkeypatch.setenv("AC_KNN_TWO_PHASE", two_phase)                   # (read per call)
    P, Q, x = bref.case(N, D, nq, metric, qstep)
    store, Qd, prepared = _dev_store((N, D, nq, qstep), cuda_dev)
    for name in bref.SELECTIONS:
        mask = bref.selection(name, N, k)
        words = _words(mask, cuda_dev)
        got, st = _call(metric + "_topk_batch_sel", store, N, D, Qd, k, cuda_dev, prepared=prepared, sel=words)
        fp32, _ = _call(metric + "_topk_sel", store, N, D, Qd, k, cuda_dev, sel=words)
        print(N, D, nq, k, metric, name, "selected", int(mask.sum()), "stats", st)
        _assert_same_bits(got, fp32, f"from ac_knn_{metric}_topk_sel ({name})")
        _assert_oracle(tuple(t[::qstep] for t in got), ref.filtered_topk(P, Q[::qstep], k, mask, metric, values=x), metric)
        assert (got[1].cpu().numpy() >= 0).sum(axis=1).tolist() == [min(int(mask.sum()), k)] * nq
        if nq <= 64:
            assert st[1] == 2, "the plane sweep did not run"
        if name in ("tiny", "empty"):
            assert st[0] == 0, f"{name}: {st[0]} queries took the exact fallback (the short-selection certificate rule)"
        else:
            assert 0 <= st[0] <= 2, f"{name}: {st[0]} of {nq} queries took the exact fallback"


# ---- 2. an all-ones selection returns the bits -- and the stats -- of the unfiltered prepared-store search -------------------------
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("ci,two_phase", [(0, None), (3, "1"), (3, "0")], ids=["plane", "gemm-two-phase", "gemm-sample-stages"])
def test_all_ones_equals_unfiltered_batch(ci, two_phase, metric, cuda_dev, monkeypatch):
    N, D, nq, k, qstep = bref.ORACLE_CASES[ci]
    if two_phase is not None:
        monkeypatch.setenv("AC_KNN_TWO_PHASE", two_phase)
    store, Qd, prepared = _dev_store((N, D, nq, qstep), cuda_dev)
    a, sa = _call(metric + "_topk_batch", store, N, D, Qd, k, cuda_dev, prepared=prepared)
    b, sb = _call(metric + "_topk_batch_sel", store, N, D, Qd, k, cuda_dev, prepared=prepared, sel=_words(np.ones(N, dtype=bool), cuda_dev))
    _assert_same_bits(a, b, "from the unfiltered search")
    assert sa == sb


# ---- 3. sel_bit0 and row_offset ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("ci,two_phase", [(0, None), (3, "1"), (3, "0")], ids=["plane", "gemm-two-phase", "gemm-sample-stages"])
def test_sel_bit0_and_row_offset(ci, two_phase, metric, cuda_dev, monkeypatch):
    """the half mask at bit 70001 of a bitmap whose other bits are ones: a sweep that dropped sel_bit0, or a sample stage that
    tested the bit of the logical instead of the store row, reads other rows' bits"""
    N, D, nq, k, qstep = bref.ORACLE_CASES[ci]
    if two_phase is not None:
        monkeypatch.setenv("AC_KNN_TWO_PHASE", two_phase)
    store, Qd, prepared = _dev_store((N, D, nq, qstep), cuda_dev)
    mask = bref.selection("half", N, k)
    base, sb = _call(metric + "_topk_batch_sel", store, N, D, Qd, k, cuda_dev, prepared=prepared, sel=_words(mask, cuda_dev))
    bit0 = 70001
    big = ref.pack(mask, bit0=bit0, total_bits=bit0 + N + 200, fill=True)
    got, sg = _call(metric + "_topk_batch_sel", store, N, D, Qd, k, cuda_dev, prepared=prepared, sel=_words(big, cuda_dev),
                    sel_bit0=bit0, row_offset=7)
    assert torch.equal(got[1], torch.where(base[1] >= 0, base[1] + 7, base[1]))
    assert torch.equal(got[0], base[0]) and torch.equal(got[2], base[2])
    assert 0 <= sg[0] <= 2 and 0 <= sb[0] <= 2
    # the upper half of the store: the sample's STORE rows are spread over the whole store and half of them are selected, while its
    # LOGICAL row numbers all lie in the unselected lower half -- a stage that tested those would see no selected row, keep no
    # threshold and overflow every candidate buffer in the main sweep
    upper = np.arange(N) >= N // 2
    fp32, _ = _call(metric + "_topk_sel", store, N, D, Qd, k, cuda_dev, sel=_words(upper, cuda_dev))
    got, sg = _call(metric + "_topk_batch_sel", store, N, D, Qd, k, cuda_dev, prepared=prepared,
                    sel=_words(ref.pack(upper, bit0=bit0, total_bits=bit0 + N + 200, fill=True), cuda_dev), sel_bit0=bit0)
    _assert_same_bits(got, fp32, "from the fp32 route (upper half)")
    assert 0 <= sg[0] <= 2, f"upper half: {sg[0]} of {nq} queries took the exact fallback"


# ---- 4. queries no certificate can hold for are answered by the FILTERED fallback ---------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
def test_uncertified_queries_take_the_filtered_fallback(metric, cuda_dev):
    N, D, nq, k = bref.CLUSTER
    P, Q, x = bref.cluster_case(metric)
    store, Qd, prepared = _dev_store("cluster", cuda_dev)
    mask = bref.selection("half", N, k)
    words = _words(mask, cuda_dev)
    want = ref.filtered_topk(P, Q, k, mask, metric, values=x)
    got, st = _call(metric + "_topk_batch_sel", store, N, D, Qd, k, cuda_dev, prepared=prepared, sel=words)      # GEMM form, candidate buffer
    _assert_oracle(got, want, metric)
    assert st[0] == nq                                                       # more flagged queries than fallback slots: both forms run
    got, st = _call(metric + "_topk_batch_sel", store, N, D, Qd[:20], k, cuda_dev, prepared=prepared, sel=words)  # plane form
    _assert_oracle(got, tuple(t[:20] for t in want), metric)
    assert st[1] == 2


# ---- 5. a filtered call between two unfiltered ones: one store, one workspace --------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("ci", [0, 3], ids=["plane", "gemm"])
def test_filtered_call_between_two_unfiltered_ones(ci, metric, cuda_dev):
    from adaptive_classifier import index as ix
    N, D, nq, k, qstep = bref.ORACLE_CASES[ci]
    store, Qd, prepared = _dev_store((N, D, nq, qstep), cuda_dev)
    planes0, norms0 = prepared[0].clone(), prepared[1].clone()
    ws = torch.empty(ix.knn_batch_workspace_bytes(N, D, nq, k), dtype=torch.uint8, device=cuda_dev)
    a, sa = _call(metric + "_topk_batch", store, N, D, Qd, k, cuda_dev, prepared=prepared, ws=ws)
    _call(metric + "_topk_batch_sel", store, N, D, Qd, k, cuda_dev, prepared=prepared, ws=ws, sel=_words(bref.selection("sparse", N, k), cuda_dev))
    b, sb = _call(metric + "_topk_batch", store, N, D, Qd, k, cuda_dev, prepared=prepared, ws=ws)
    _assert_same_bits(a, b, "after a filtered call")
    assert sa == sb
    assert torch.equal(prepared[0], planes0) and torch.equal(prepared[1], norms0)        # the prepared store is not changed


# ---- 6. index and memory -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
def test_index_routes_dense_known_selections_to_the_prepared_store(metric, cuda_dev, monkeypatch):
    from adaptive_classifier import index as ix
    N, D, nq, k, qstep = bref.INDEX_CASE
    P, Q, x = bref.case(N, D, nq, metric, qstep)
    store, Qd, _ = _dev_store((N, D, nq, qstep), cuda_dev)
    entries = []
    real = ix.knn_topk_sel
    monkeypatch.setattr(ix, "knn_topk_sel", lambda *a, **kw: entries.append(kw.get("prepared") is not None) or real(*a, **kw))
    idx = (ix.HipFlatIPIndex if metric == "ip" else ix.HipFlatL2Index)(D, device=cuda_dev)
    idx.add_device_rows(store)
    mask = bref.selection("half", N, k)
    fp32, _ = _call(metric + "_topk_sel", store, N, D, Qd, k, cuda_dev, sel=_words(mask, cuda_dev))
    # a device-mask selector has no known count: the fp32 route, and the plane stays as it was
    dsel = ix.RowSelector.from_mask(torch.from_numpy(mask).to(cuda_dev))
    assert dsel.known_count is None
    Dg, Ig = idx.search_device(Qd, k, dsel)
    assert entries == [False] and idx._prepared is None and torch.equal(Ig, fp32[1]) and torch.equal(Dg, fp32[0])
    # a known-sparse selector stays on the fp32 route too
    sparse = np.zeros(N, dtype=bool); sparse[:: 40] = True
    idx.search_device(Qd, k, ix.RowSelector.from_mask(sparse, device=cuda_dev))
    assert entries == [False, False] and idx._prepared is None
    # a host-mask selector knows its count: the plane is prepared and the prepared route taken
    Dg, Ig = idx.search_device(Qd, k, mask)
    assert entries[-1] is True and idx._prepared is not None
    assert torch.equal(Ig, fp32[1]) and torch.equal(Dg, fp32[0])
    want = ref.filtered_topk(P, Q[::qstep], k, mask, metric, values=x)
    assert np.array_equal(Ig[::qstep].cpu().numpy(), want[1]) and _ulp_close(Dg[::qstep].cpu().numpy(), want[0])
    assert idx.exact_fallbacks <= 2
    # ... and so does the device-mask selector once its count has been read
    assert dsel.count() == int(mask.sum())
    Dg, Ig = idx.search_device(Qd, k, dsel)
    assert entries[-1] is True and torch.equal(Ig, fp32[1]) and torch.equal(Dg, fp32[0])


def test_memory_among_on_a_big_load_rows_store(cuda_dev, monkeypatch):
    from adaptive_classifier import index as ix
    from adaptive_classifier.memory import PrototypeMemory
    N, D, nq, k, qstep = bref.INDEX_CASE
    P, Q, _ = bref.case(N, D, nq, "l2", qstep)
    store, Qd, _ = _dev_store((N, D, nq, qstep), cuda_dev)
    labels = np.random.default_rng(6).integers(0, 4, N).astype(np.int32)
    mem = PrototypeMemory(D, device=str(cuda_dev))
    mem.load_rows(store, torch.from_numpy(labels), [f"L{i}" for i in range(4)])
    entries = []
    real = ix.knn_topk_sel
    monkeypatch.setattr(ix, "knn_topk_sel", lambda *a, **kw: entries.append(kw.get("prepared") is not None) or real(*a, **kw))
    Dg, Ig = mem.search_raw(Qd, k, among=["L1", "L3", "unknown"])
    assert entries == [True]                                                 # _among_selector counted the rows: the prepared route
    mask = np.isin(labels, [1, 3])
    fp32, _ = _call("l2_topk_sel", store, N, D, Qd, k, cuda_dev, sel=_words(mask, cuda_dev))
    assert torch.equal(Ig, fp32[1]) and torch.equal(Dg, fp32[0])
    assert np.isin(labels[Ig.cpu().numpy()], [1, 3]).all()


# ---- 7. logical shards: slices of one global bitmap over prepared shards --------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
def test_prepared_shards_of_one_bitmap_equal_the_unsharded_search(metric, cuda_dev):
    from adaptive_classifier import index as ix
    from adaptive_classifier.sharded import ShardedSearch
    n_shard, D, nq, k = 70001, 32, 300, 8
    N = 2 * n_shard
    store = _store(rref.unit_rows(N, D, 1), cuda_dev)
    Qd = torch.tensor(rref.unit_rows(nq, D, 2), device=cuda_dev)
    mask = np.random.default_rng(3).random(N) < 0.5
    sel = ix.RowSelector.from_mask(mask, device=cuda_dev)
    whole, _ = _call(metric + "_topk_sel", store, N, D, Qd, k, cuda_dev, sel=sel.words)
    Es, Is = [], []
    for lo in (0, n_shard):
        ss = ShardedSearch(store[lo:], n_shard, D, lo, metric=metric)
        E, I = ss._local(Qd, k, sel)
        assert ss._prepared is not None                                      # the shard's plane, with sel_bit0 = row_offset
        Es.append(E); Is.append(I)
    mD, mI = (ix.topk_merge_ip if metric == "ip" else ix.topk_merge)(torch.stack(Es), torch.stack(Is))
    assert torch.equal(mI, whole[1]) and torch.equal(mD, whole[0])
