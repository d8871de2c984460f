"""Filtered top-k search on the GPU (ac_knn_*_topk_sel / ac_knn_*_topk_ids / ac_knn_sel_* through the C ABI, then the flat
indexes, PrototypeMemory and ShardedSearch) against the fp64 oracle tests/knn_select_ref.py.

Bar: ids EQUAL to the oracle's for every query (tests/test_knn_select_cpu.py asserts that the deciding ranks of every case lie
>= 2^-40 apart, so no query is left out), values within 1 fp32 ulp, exact_out rounded once == the fp32 output."""
import ctypes
import functools
import os
import socket
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import knn_range_ref as rref  # noqa: E402
import knn_select_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu


def _ulp_close(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    with np.errstate(over="ignore"):                                # (the spacing of the FLT_MAX padding overflows to inf)
        return a.shape == b.shape and np.all(np.abs(a - b) <= np.spacing(np.maximum(np.abs(a), np.abs(b)).astype(np.float32)))


def _store(P, dev):
    ld = (P.shape[1] + 3) // 4 * 4
    store = torch.zeros((max(P.shape[0], 1), ld), dtype=torch.float32, device=dev)
    if P.shape[0]:
        store[: P.shape[0], : P.shape[1]] = torch.tensor(P, device=dev)        # (a copy: the shared inputs are read-only)
    return store


def _words(mask_or_words, dev):
    w = mask_or_words if mask_or_words.dtype == np.uint64 else ref.pack(mask_or_words)
    return torch.from_numpy(w.view(np.int64).copy()).to(dev)


def _call(entry, store, N, D, Qd, k, dev, sel=None, sel_bit0=0, row_offset=0):
    """one search through the C ABI: entry = 'l2_topk_x' | 'ip_topk_sel' | ...  -> (D, I, exact) device tensors, stats list"""
    from adaptive_classifier import _native as nv
    L = nv.lib()
    nq = Qd.shape[0]
    need = ctypes.c_size_t(0)
    assert L.ac_knn_l2_topk_workspace(N, D, nq, k, ctypes.byref(need)) == 0
    ws = torch.empty(max(need.value, 256), dtype=torch.uint8, device=dev)
    outD = torch.empty((nq, k), dtype=torch.float32, device=dev)
    outE = torch.empty((nq, k), dtype=torch.float64, device=dev)
    outI = torch.empty((nq, k), dtype=torch.int64, device=dev)
    stats = torch.full((4,), -7, dtype=torch.int32, device=dev)
    head = [nv.ptr(store), N, store.stride(0), D, nv.ptr(Qd), nq, Qd.stride(0), k, row_offset]
    mid = [nv.ptr(sel), sel_bit0] if entry.endswith("_sel") else []
    tail = [nv.ptr(outD), nv.ptr(outE), nv.ptr(outI), nv.ptr(ws), need.value, nv.ptr(stats), nv.stream_ptr(dev)]
    with torch.cuda.device(dev):
        nv.check(getattr(L, "ac_knn_" + entry)(*(head + mid + tail)), entry)
    torch.cuda.synchronize()
    return (outD, outI, outE), stats.tolist()


def _assert_oracle(got, want, metric):
    (D, I, E), (oD, oI, oE) = [tuple(t.cpu().numpy() if torch.is_tensor(t) else t for t in g) for g in (got, want)]
    assert np.array_equal(I, oI), f"id mismatch in {(I != oI).any(axis=1).sum()} of {I.shape[0]} queries"
    assert _ulp_close(D, oD)
    real = I >= 0
    if E is not None:
        assert np.array_equal(E[real].astype(np.float32), D[real])           # D is the fp64 output rounded once
        assert np.all(np.isinf(E[~real])) and np.all(np.sign(E[~real]) == (-1 if metric == "ip" else 1))
    assert np.all(D[~real] == (-ref.FLT_MAX if metric == "ip" else ref.FLT_MAX))


@functools.lru_cache(maxsize=None)
def _dev_case(N, D, nq, dev):
    P, Q, _ = ref.case(N, D, nq, "l2")
    return _store(P, dev), torch.tensor(Q, device=dev)


# ---- 1. oracle equality --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("N,D,nq,k", ref.CASES, ids=[
    "ring24-N%128",          # knn_sweep_ring<4,24>; N % 128 != 0
    "ring32",                # knn_sweep_ring<4,32>
    "sweep2-ragged",         # knn_sweep<2>, ragged third tile
    "sweep1-tailgroup",      # knn_sweep<1>, tail k-group
    "tiles-per-block",       # several tiles per block
    "small-exact",           # knn_small_exact with a selection
    "last-word",             # one row in the last tile and the last word
    "D%4",                   # D % 4 != 0
])
def test_filtered_matches_oracle(N, D, nq, k, metric, cuda_dev):
    P, Q, x = ref.case(N, D, nq, metric)
    store, Qd = _dev_case(N, D, nq, cuda_dev)
    for name in ref.SELECTIONS:
        mask = ref.selection(name, N, k)
        got, st = _call(metric + "_topk_sel", store, N, D, Qd, k, cuda_dev, sel=_words(mask, cuda_dev))
        print(N, D, nq, k, metric, name, "selected", int(mask.sum()), "stats", st)
        _assert_oracle(got, ref.filtered_topk(P, Q, k, mask, metric, values=x), metric)
        assert st[0] >= 0 and st[2] == 0 and st[3] == 0


# ---- 2. an all-ones selection returns the bits of the unfiltered search ------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("N,D,nq,k", [ref.CASES[0], ref.CASES[3], ref.CASES[2], ref.CASES[5]], ids=["ring", "sweep1", "sweep2", "small"])
def test_all_ones_equals_unfiltered(N, D, nq, k, metric, cuda_dev):
    store, Qd = _dev_case(N, D, nq, cuda_dev)
    a, sa = _call(metric + "_topk_x", store, N, D, Qd, k, cuda_dev)
    b, sb = _call(metric + "_topk_sel", store, N, D, Qd, k, cuda_dev, sel=_words(np.ones(N, dtype=bool), cuda_dev))
    for t, u in zip(a, b):
        assert torch.equal(t, u)
    assert sa == sb


# ---- 3. sel_bit0 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("N,D,nq,k", [ref.CASES[0], ref.CASES[3], ref.CASES[2], ref.CASES[5]], ids=["ring", "sweep1", "sweep2", "small"])
def test_sel_bit0_embeds_the_selection(N, D, nq, k, metric, cuda_dev):
    store, Qd = _dev_case(N, D, nq, cuda_dev)
    mask = ref.selection("half", N, k)
    base, _ = _call(metric + "_topk_sel", store, N, D, Qd, k, cuda_dev, sel=_words(mask, cuda_dev))
    for bit0 in (1, 15, 37, 63, 64, 1000):
        big = ref.pack(mask, bit0=bit0, total_bits=bit0 + N + 200, fill=True)          # every surrounding bit is set
        got, _ = _call(metric + "_topk_sel", store, N, D, Qd, k, cuda_dev, sel=_words(big, cuda_dev), sel_bit0=bit0)
        for t, u in zip(base, got):
            assert torch.equal(t, u), f"sel_bit0={bit0}"


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_sharded_slices_of_one_bitmap_equal_the_unsharded_search(metric, cuda_dev):
    from adaptive_classifier import index as ix
    N, D, nq, k = ref.CASES[0]
    store, Qd = _dev_case(N, D, nq, cuda_dev)
    mask = ref.selection("half", N, k)
    words = _words(mask, cuda_dev)
    whole, _ = _call(metric + "_topk_sel", store, N, D, Qd, k, cuda_dev, sel=words)
    bounds = [0, 1700, 3333, 5000]                                  # not multiples of 16 or 64
    Es, Is = [], []
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        (_, I, E), _ = _call(metric + "_topk_sel", store[lo:], hi - lo, D, Qd, k, cuda_dev, sel=words, sel_bit0=lo, row_offset=lo)
        Es.append(E); Is.append(I)
    merge = ix.topk_merge_ip if metric == "ip" else ix.topk_merge
    mD, mI = merge(torch.stack(Es), torch.stack(Is))
    assert torch.equal(mI, whole[1]) and torch.equal(mD, whole[0])


# ---- 4. short and empty selections: certified, not sent to the fallback ---------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_short_selections_pad_and_stay_certified(metric, cuda_dev):
    N, D, nq, k = ref.CASES[0]
    P, Q, x = ref.case(N, D, nq, metric)
    store, Qd = _dev_case(N, D, nq, cuda_dev)
    rows = np.random.default_rng(5).permutation(N)
    for m in (0, 1, k - 1, k, k + 1):
        mask = np.zeros(N, dtype=bool)
        mask[rows[:m]] = True
        got, st = _call(metric + "_topk_sel", store, N, D, Qd, k, cuda_dev, sel=_words(mask, cuda_dev))
        want = ref.filtered_topk(P, Q, k, mask, metric, values=x)
        _assert_oracle(got, want, metric)
        assert (got[1].cpu().numpy() >= 0).sum(axis=1).tolist() == [min(m, k)] * nq
        assert st[0] == 0, f"{m} selected rows: {st[0]} queries took the exact fallback"


# ---- 5. unselected rows never leak ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_unselected_rows_never_leak(metric, cuda_dev):
    N, D, nq, k = 2000, 256, 10, 8
    P = rref.unit_rows(N, D, 1).copy()
    Q = rref.unit_rows(nq, D, 2)
    P[0:10] = Q                                                     # distance 0 / the largest possible product of unit rows
    P[1000:1010] = Q
    store, Qd = _store(P, cuda_dev), torch.tensor(Q, device=cuda_dev)
    x = rref.fixed_order_values(P, Q, metric)
    mask = np.ones(N, dtype=bool); mask[0:10] = False
    got, _ = _call(metric + "_topk_sel", store, N, D, Qd, k, cuda_dev, sel=_words(mask, cuda_dev))
    _assert_oracle(got, ref.filtered_topk(P, Q, k, mask, metric, values=x), metric)
    assert got[1][:, 0].tolist() == list(range(1000, 1010))
    mask[1000:1010] = False
    got, _ = _call(metric + "_topk_sel", store, N, D, Qd, k, cuda_dev, sel=_words(mask, cuda_dev))
    _assert_oracle(got, ref.filtered_topk(P, Q, k, mask, metric, values=x), metric)
    I = got[1].cpu().numpy()
    assert not np.isin(I, np.r_[0:10, 1000:1010]).any() and (I >= 0).all()


# ---- 6. ties and the fallback -----------------------------------------------------------------------------------------------------
def _copies(nbase, ncopies, D, seed, dropped):
    base = rref.unit_rows(nbase, D, seed)
    P = np.concatenate([base] * ncopies, axis=0)                    # row c * nbase + b = copy c of base row b
    mask = np.repeat(~np.isin(np.arange(ncopies), dropped), nbase)
    return base, P, mask


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_ties_beyond_the_candidate_list_take_the_filtered_fallback(metric, cuda_dev):
    """30 of 40 copies selected: the selected tie group (30) exceeds k' = 24, so every query is flagged and the fallback --
    which must skip the dropped copies -- decides; the ids are the 16 lowest SELECTED copies"""
    base, P, mask = _copies(50, 40, 768, 5, [0, 3, 7, 11, 14, 19, 22, 27, 31, 38])
    Q, k = base[:6].copy(), 16
    got, st = _call(metric + "_topk_sel", _store(P, cuda_dev), P.shape[0], 768, torch.tensor(Q, device=cuda_dev), k, cuda_dev,
                    sel=_words(mask, cuda_dev))
    _assert_oracle(got, ref.filtered_topk(P, Q, k, mask, metric), metric)
    sel_copies = [c for c in range(40) if mask[c * 50]][:k]
    assert got[1].cpu().numpy().tolist() == [[c * 50 + q for c in sel_copies] for q in range(6)]
    assert st[0] == 6


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_ties_within_the_candidate_list_are_reranked(metric, cuda_dev):
    """20 of 40 copies selected: the whole tie group (20 <= k' = 24) is re-ranked, nothing is flagged"""
    base, P, mask = _copies(50, 40, 768, 5, list(range(1, 40, 2)))
    Q, k = base[:6].copy(), 16
    got, st = _call(metric + "_topk_sel", _store(P, cuda_dev), P.shape[0], 768, torch.tensor(Q, device=cuda_dev), k, cuda_dev,
                    sel=_words(mask, cuda_dev))
    _assert_oracle(got, ref.filtered_topk(P, Q, k, mask, metric), metric)
    assert got[1].cpu().numpy().tolist() == [[c * 50 + q for c in range(0, 32, 2)] for q in range(6)]
    assert st[0] == 0


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_many_filtered_fallbacks_slots_and_direct(metric, cuda_dev):
    """100 flagged queries, more than the 64 fallback slots: the slab-parallel and the direct form both honour the selection"""
    base, P, mask = _copies(100, 30, 256, 11, [1, 8, 15, 22])      # 26 of 30 copies selected: > k' = 24
    Q, k = base.copy(), 16
    got, st = _call(metric + "_topk_sel", _store(P, cuda_dev), P.shape[0], 256, torch.tensor(Q, device=cuda_dev), k, cuda_dev,
                    sel=_words(mask, cuda_dev))
    _assert_oracle(got, ref.filtered_topk(P, Q, k, mask, metric), metric)
    assert st[0] == 100


# ---- 7. id-list route -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ids_case(metric):
    P, Q = rref.unit_rows(20000, 128, 1), rref.unit_rows(5, 128, 2)
    x = rref.fixed_order_values(P, Q, metric)
    for a in (P, Q, x):
        a.setflags(write=False)
    return P, Q, x


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_id_list_route(metric, cuda_dev):
    from adaptive_classifier import index as ix
    N, D = 20000, 128
    P, Q, x = _ids_case(metric)
    store, Qd = _store(P, cuda_dev), torch.tensor(Q, device=cuda_dev)
    for M, k in ((1, 8), (17, 8), (17, 40), (4096, 8), (8192, 8)):
        ids = np.sort(np.random.default_rng(M).choice(N, M, replace=False)).astype(np.int64)
        mask = np.zeros(N, dtype=bool); mask[ids] = True
        assert ref.min_rel_gap(x, mask, k, metric) >= ref.MIN_GAP
        want = ref.filtered_topk(P, Q, k, mask, metric, values=x)
        E = torch.empty((5, k), dtype=torch.float64, device=cuda_dev)
        Di, Ii = ix.knn_topk_ids(store, N, D, Qd, k, torch.from_numpy(ids).to(cuda_dev), metric=metric, exact_out=E)
        _assert_oracle((Di, Ii, E), want, metric)
        Ds, Is = ix.knn_topk_sel(store, N, D, Qd, k, ix.RowSelector.from_mask(mask, device=cuda_dev), metric=metric)
        assert torch.equal(Ii, Is) and _ulp_close(Di.cpu().numpy(), Ds.cpu().numpy())
        # unsorted, with duplicates and out-of-range ids, through RowSelector.from_ids
        messy = np.concatenate([ids[::-1], ids[:5], [-3, N, N + 99]])
        Dm, Im = ix.knn_topk_ids(store, N, D, Qd, k, ix.RowSelector.from_ids(messy, N, device=cuda_dev), metric=metric)
        assert torch.equal(Im, Ii) and torch.equal(Dm, Di)
    # an id outside [0, N) handed to the entry point itself is skipped on the device
    ids = np.array([-5, 3, 700, 19999, 20000, 1 << 40], dtype=np.int64)
    mask = np.zeros(N, dtype=bool); mask[[3, 700, 19999]] = True
    Di, Ii = ix.knn_topk_ids(store, N, D, Qd, 4, torch.from_numpy(ids).to(cuda_dev), metric=metric, row_offset=7)
    _assert_oracle((Di, Ii, None), ref.filtered_topk(P, Q, 4, mask, metric, row_offset=7, values=x), metric)
    # an empty list: all padding
    Di, Ii = ix.knn_topk_ids(store, N, D, Qd, 3, torch.empty(0, dtype=torch.int64, device=cuda_dev), metric=metric)
    assert (Ii == -1).all() and (Di == (-ref.FLT_MAX if metric == "ip" else ref.FLT_MAX)).all()


# ---- 8. builders ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097, 70001])
def test_selection_builders_equal_numpy_packing(n, cuda_dev):
    from adaptive_classifier import _native as nv
    L = nv.lib()
    rng = np.random.default_rng(n)
    mask = rng.random(n) < 0.5
    rc = rng.integers(0, 5, n).astype(np.int32)
    rc[rc == 3] = 2                                                 # 5 classes, class 3 absent
    rc[rng.integers(0, n)] = -1                                     # out-of-range classes: unselected
    rc[rng.integers(0, n)] = 5
    on = np.array([1, 0, 1, 1, 1], dtype=np.uint8)
    cmask = np.zeros(n, dtype=bool)
    ok = (rc >= 0) & (rc < 5)
    cmask[ok] = on[rc[ok]] != 0
    nw = (n + 63) // 64
    d_mask, d_rc, d_on = (torch.from_numpy(t).to(cuda_dev) for t in (mask.astype(np.uint8), rc, on))       # (alive across the calls)
    for want, call in (
        (ref.pack(mask), lambda out: L.ac_knn_sel_pack(nv.ptr(d_mask), n, nv.ptr(out), nv.stream_ptr(cuda_dev))),
        (ref.pack(cmask), lambda out: L.ac_knn_sel_classes(nv.ptr(d_rc), n, nv.ptr(d_on), 5, nv.ptr(out), nv.stream_ptr(cuda_dev))),
    ):
        out = torch.full((nw + 2,), -1, dtype=torch.int64, device=cuda_dev)        # 0xFF bytes everywhere
        with torch.cuda.device(cuda_dev):
            assert call(out) == 0
        torch.cuda.synchronize()
        got = out.cpu().numpy().view(np.uint64)
        assert np.array_equal(got[:nw], want)                                       # tail bits of the last word came back 0
        assert (got[nw:] == np.uint64(0xFFFFFFFFFFFFFFFF)).all()                    # nothing past ceil(n / 64) words is touched
    from adaptive_classifier.index import RowSelector
    assert np.array_equal(RowSelector.from_mask(torch.from_numpy(mask).to(cuda_dev)).words.cpu().numpy().view(np.uint64), ref.pack(mask))
    assert np.array_equal(RowSelector.from_classes(torch.from_numpy(rc).to(cuda_dev), [0, 2, 3, 4], 5).words.cpu().numpy().view(np.uint64),
                          ref.pack(cmask))
    ids = np.nonzero(mask)[0]
    assert np.array_equal(RowSelector.from_ids(torch.from_numpy(np.concatenate([ids[::-1], [-1, n + 3]])).to(cuda_dev), n)
                          .words.cpu().numpy().view(np.uint64), ref.pack(mask))


# ---- 9. index, memory, sharded ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_index_search_with_selectors(metric, cuda_dev):
    from adaptive_classifier.index import HipFlatIPIndex, HipFlatL2Index, RowSelector
    N, D, nq, k = ref.CASES[3]
    P, Q, x = ref.case(N, D, nq, metric)
    idx = (HipFlatIPIndex if metric == "ip" else HipFlatL2Index)(D, device=cuda_dev)
    idx.add(P)
    mask = ref.selection("half", N, k)
    want = ref.filtered_topk(P, Q, k, mask, metric, values=x)
    ids = np.nonzero(mask)[0]
    for sel in (mask, torch.from_numpy(mask).to(cuda_dev), ids[::-1].copy(), RowSelector.from_mask(mask, device=cuda_dev),
                RowSelector.from_ids(ids, N), RowSelector.from_range(0, N, N)):
        Dg, Ig = idx.search(Q, k, sel=sel)
        assert Dg.dtype == np.float32 and Ig.dtype == np.int64
        _assert_oracle((Dg, Ig, None), want if not (isinstance(sel, RowSelector) and sel.ids is None and sel.count() == N)
                       else ref.filtered_topk(P, Q, k, np.ones(N, dtype=bool), metric, values=x), metric)
    assert idx._prepared is None                                     # a filtered search neither uses nor prepares the fp16 plane
    with pytest.raises(ValueError):
        idx.search(Q, k, sel=RowSelector.from_range(0, 5, N - 1))
    # after remove_ids + add, a selector for the new ntotal
    gone = np.array([0, 5, 700, 1152])
    idx.remove_ids(gone)
    extra = rref.unit_rows(40, D, 9)
    idx.add(extra)
    P2 = np.concatenate([np.delete(P, gone, axis=0), extra])
    assert idx.ntotal == P2.shape[0]
    mask2 = np.random.default_rng(8).random(P2.shape[0]) < 0.3
    assert ref.min_rel_gap(rref.fixed_order_values(P2, Q, metric), mask2, k, metric) >= ref.MIN_GAP
    Dg, Ig = idx.search(Q, k, sel=mask2)
    _assert_oracle((Dg, Ig, None), ref.filtered_topk(P2, Q, k, mask2, metric), metric)


def test_memory_among(cuda_dev):
    from adaptive_classifier.memory import PrototypeMemory
    from adaptive_classifier.models import Example
    D = 64
    protos = rref.unit_rows(12, D, 3)
    mem = PrototypeMemory(D, device=str(cuda_dev))
    for c in range(12):
        mem.add_example(Example(text=f"t{c}", label=f"c{c:02d}", embedding=torch.tensor(protos[c])), f"c{c:02d}")
    mem._rebuild_index()                                            # (the index follows the prototypes at the next scheduled rebuild; do it now)
    q = torch.tensor(rref.unit_rows(1, D, 4)[0])
    chosen = ["c03", "c07", "c10", "nope"]                          # an unknown label is ignored
    res = mem.get_nearest_prototypes(q, k=5, among=chosen)
    assert len(res) == 3 and {l for l, _ in res} == {"c03", "c07", "c10"}
    assert abs(sum(s for _, s in res) - 1.0) <= 1e-5
    d = ((protos[[3, 7, 10]] - q.numpy()) ** 2).sum(1)
    assert [l for l, _ in res] == [["c03", "c07", "c10"][i] for i in np.argsort(d)]
    assert mem.get_nearest_prototypes(q, k=5, among=[]) == [] and mem.get_nearest_prototypes(q, k=5, among=["nope"]) == []
    assert len(mem.get_nearest_prototypes(q, k=5)) == 5              # the unfiltered call is what it was
    S, I, Dd = mem.search_batch(q.reshape(1, -1).to(cuda_dev), 5, among=chosen)
    assert I[0].tolist()[3:] == [-1, -1] and sorted(I[0].tolist()[:3]) == [3, 7, 10] and abs(float(S.sum()) - 1.0) <= 1e-5
    # a load_rows() store: 3000 rows, 6 classes
    N, nq, k = 3000, 4, 9
    P, Q = rref.unit_rows(N, D, 1), rref.unit_rows(nq, D, 2)
    labels = (np.random.default_rng(6).integers(0, 6, N)).astype(np.int32)
    names = [f"L{i}" for i in range(6)]
    mem2 = PrototypeMemory(D, device=str(cuda_dev))
    mem2.load_rows(_store(P, cuda_dev), torch.from_numpy(labels), names)
    Dg, Ig = mem2.search_raw(torch.tensor(Q, device=cuda_dev), k, among=["L1", "L4", "unknown"])
    mask = np.isin(labels, [1, 4])
    assert ref.min_rel_gap(rref.fixed_order_values(P, Q, "l2"), mask, k) >= ref.MIN_GAP
    _assert_oracle((Dg, Ig, None), ref.filtered_topk(P, Q, k, mask, "l2"), "l2")
    assert np.isin(labels[Ig.cpu().numpy()], [1, 4]).all()
    assert mem2._among_selector(["L1", "L4", "unknown"])[0] is mem2._among_selector(["L4", "L1", "unknown"])[0]      # cached per label set
    Dg, Ig = mem2.search_raw(torch.tensor(Q, device=cuda_dev), k, among=[])
    assert (Ig == -1).all() and (Dg == ref.FLT_MAX).all()
    assert {l for l, _ in mem2.get_nearest_prototypes(torch.tensor(Q[0]), k=4, among=["L2"])} == {"L2"}


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _sharded_worker(rank, port, ret):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [root, os.path.join(root, "adaptive-classifier_amd"), os.path.join(root, "tests")]
    import torch.distributed as dist
    from adaptive_classifier.index import HipFlatL2Index, RowSelector
    from adaptive_classifier.sharded import ShardedSearch
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    N, D, nq, k = 1153, 100, 9, 10
    P, Q = rref.unit_rows(N, D, 1), rref.unit_rows(nq, D, 2)
    idx = HipFlatL2Index(D, device=dev)
    idx.add(P)
    sel = RowSelector.from_mask(ref.selection("half", N, k), device=dev)
    Qd = torch.tensor(Q, device=dev)
    uD, uI = idx.search_device(Qd, k, sel)
    ss = ShardedSearch(idx._store, N, D, 0, force_collectives=True)
    gD, gI = ss.search(Qd, k, sel=sel)
    bD, bI = ss.search_block(Qd, k, sel=sel)
    ret["ok"] = bool(ss._collective and torch.equal(gI, uI) and torch.equal(gD, uD) and torch.equal(bI, uI) and torch.equal(bD, uD))
    dist.barrier()
    dist.destroy_process_group()


def test_sharded_search_with_selector_world1(cuda_dev):
    """ShardedSearch(force_collectives=True) on a one-rank group with sel= (the collectives execute): equals the index result"""
    import torch.multiprocessing as mp
    mgr = mp.Manager()
    ret = mgr.dict()
    mp.spawn(_sharded_worker, args=(_free_port(), ret), nprocs=1, join=True)
    assert ret.get("ok") is True
