"""FILTERED range search on the GPU: ac_knn_*_range_count_sel (+ the unfiltered fill) and ac_knn_*_range_count_ids / _fill_ids
through knn_range_search(sel=) / knn_range_ids, the flat indexes, PrototypeMemory.prototypes_within(among=) and logical row
shards, against the fp64 oracle of tests/knn_range_sel_ref.py (knn_range_ref.range_search on the sub-matrix of the selected rows,
ids mapped back).

Bar: lims and ids EQUAL to the oracle's for every query, D within 1 ulp, every D satisfies the predicate, ids ascend.  No query
is left out: each test first asserts that no SELECTED row's value lies within 64 ulps of its radius (only such a value could be
decided differently by another summation order)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import knn_range_ref as ref  # noqa: E402
import knn_range_sel_ref as sref  # noqa: E402

pytestmark = pytest.mark.gpu


def _ulp_close(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and np.all(np.abs(a - b) <= np.spacing(np.maximum(np.abs(a), np.abs(b)).astype(np.float32)))


def _store(P, dev):
    ld = (P.shape[1] + 3) // 4 * 4
    store = torch.zeros((max(P.shape[0], 1), ld), dtype=torch.float32, device=dev)
    if P.shape[0]:
        store[: P.shape[0], : P.shape[1]] = torch.tensor(P, device=dev)        # (a copy: the shared inputs are read-only)
    return store


def _words(mask, dev, bit0=0):
    """the selection as the device words tensor: exactly ceil((bit0 + n) / 64) words, every bit that is no row set to 1"""
    return torch.from_numpy(sref.pack(mask, bit0).view(np.int64).copy()).to(dev)


def _rad(rad, dev):
    return torch.from_numpy(np.asarray(rad, np.float32)).to(dev) if np.ndim(rad) else float(rad)


def _gpu(P, Q, rad, metric, dev, mask=None, bit0=0, store=None, n=None, **kw):
    """knn_range_search(sel=) -> numpy (lims, D, I[, exact]) and d_stats as a list; mask=None: the unfiltered call"""
    from adaptive_classifier import index as ix
    store = _store(P, dev) if store is None else store
    stats = torch.zeros(4, dtype=torch.int32, device=dev)
    sel = {} if mask is None else {"sel": _words(mask, dev, bit0), "sel_bit0": bit0}
    out = ix.knn_range_search(store, P.shape[0] if n is None else n, P.shape[1], torch.tensor(Q, device=dev), _rad(rad, dev), metric=metric,
                              stats=stats, **sel, **kw)
    torch.cuda.synchronize()
    return tuple(o.cpu().numpy() for o in out), stats.tolist()


def _gpu_ids(P, Q, rad, metric, dev, ids, store=None, **kw):
    """knn_range_ids -> numpy (lims, D, I[, exact]) and d_stats as a list"""
    from adaptive_classifier import index as ix
    store = _store(P, dev) if store is None else store
    stats = torch.zeros(4, dtype=torch.int32, device=dev)
    d_ids = torch.from_numpy(np.asarray(ids, np.int64)).to(dev)
    out = ix.knn_range_ids(store, P.shape[0], P.shape[1], torch.tensor(Q, device=dev), _rad(rad, dev), d_ids, metric=metric, stats=stats, **kw)
    torch.cuda.synchronize()
    return tuple(o.cpu().numpy() for o in out), stats.tolist()


def _assert_equals_oracle(got, P, Q, rad, mask, metric, x=None, row_offset=0, need_margin=True):
    lims, D, I = got[:3]
    x = ref.fixed_order_values(P, Q, metric) if x is None else x
    radv = np.broadcast_to(np.asarray(rad, np.float32), (Q.shape[0],))
    margin = sref.margin(x, mask, rad)
    print("min margin over the selected rows %.1f ulps" % margin)
    assert margin >= 64 or not need_margin, "a selected value sits too close to its radius for a summation-order independent verdict"
    olims, oD, oI = sref.filtered_range_search(P, Q, rad, mask, metric, row_offset=row_offset, values=x)
    assert lims.dtype == np.int64 and I.dtype == np.int64 and D.dtype == np.float32
    assert np.array_equal(lims, olims), (lims, olims)
    assert np.array_equal(I, oI), f"id mismatch: {(I != oI).sum()} of {I.size}"
    assert _ulp_close(D, oD)
    assert np.asarray(mask, bool)[I - row_offset].all()                       # no unselected row, no bit that belongs to no row
    for q in range(Q.shape[0]):                                               # every returned D satisfies the predicate; ids ascend
        seg = slice(lims[q], lims[q + 1])
        assert ref.is_hit(D[seg], radv[q], metric).all() and np.all(np.diff(I[seg]) > 0)


def _bit_equal(a, b):
    return len(a) == len(b) and all(u.dtype == v.dtype and np.array_equal(u, v) for u, v in zip(a, b))


# ---- 1. oracle equality: random 50 % masks, sel_bit0 = 0 and a bitmap shifted by 37 bits ----------------------------------------
@pytest.mark.parametrize("bit0", [0, 37])
@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("N,D,nq", sref.CASES)
def test_filtered_range_matches_oracle(N, D, nq, metric, bit0, cuda_dev):
    """(5000, 768, 33): with sel_bit0 = 37 a tile's 16 bits straddle two words at row_base 16; N % 64 != 0: the guarded second
    word -- the bitmap holds exactly ceil((sel_bit0 + N) / 64) words and every tail bit past the last row is 1.  (70000, 64, 5):
    several tiles per block.  (300, 4096, 3): the small-store kernel.  (1153, 100, 17), (999, 770, 7): ragged D."""
    P, Q, mask, x, rad = sref.case(N, D, nq, metric)
    got, st = _gpu(P, Q, rad, metric, cuda_dev, mask, bit0, exact_out=True)
    _assert_equals_oracle(got, P, Q, rad, mask, metric, x)
    assert 21 <= np.diff(got[0]).min() and np.diff(got[0]).max() <= 60
    assert np.array_equal(got[3].astype(np.float32), got[1])                  # D is the fp64 output rounded once
    if D == 4096:
        assert st[0] == int(mask.sum()) * nq                                  # the small-store kernel decides every SELECTED pair
    else:
        assert st[0] <= int(mask.sum()) * nq


@pytest.mark.parametrize("bit0", [0, 37])
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_only_the_last_row_selected(metric, bit0, cuda_dev):
    N, D, nq = sref.LAST_ROW_CASE                                             # N = 2^16 + 1: one row in the last tile / word / strip
    P, Q = ref.unit_rows(N, D, 1), ref.unit_rows(nq, D, 2)
    mask = np.zeros(N, bool); mask[-1] = True
    rad = np.inf if metric == "l2" else -np.inf
    got, st = _gpu(P, Q, rad, metric, cuda_dev, mask, bit0, exact_out=True)
    x = ref.fixed_order_values(P[-1:], Q, metric)
    assert got[0].tolist() == [0, 1] and got[2].tolist() == [N - 1]
    assert _ulp_close(got[1], x[0].astype(np.float32)) and np.array_equal(got[3].astype(np.float32), got[1])
    assert st[0] <= 1                                                         # at most the one selected pair was decided exactly


# ---- 2. all-ones = the unfiltered call bit for bit; the empty selection ---------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("N,D,nq", [(5000, 768, 33), (300, 4096, 3), (70000, 64, 5)])
def test_all_ones_equals_unfiltered_and_empty_selects_nothing(N, D, nq, metric, cuda_dev):
    P, Q, _, x, _ = sref.case(N, D, nq, metric)
    rad = ref.gap_radii(x, metric, 20, 60)
    store = _store(P, cuda_dev)
    plain, st0 = _gpu(P, Q, rad, metric, cuda_dev, store=store, exact_out=True)
    for bit0 in (0, 37):
        ones, st1 = _gpu(P, Q, rad, metric, cuda_dev, np.ones(N, bool), bit0, store=store, exact_out=True)
        assert _bit_equal(ones, plain) and st1[0] == st0[0]                   # lims, D, I, D64 and stats[0]
        none, st2 = _gpu(P, Q, rad, metric, cuda_dev, np.zeros(N, bool), bit0, store=store, exact_out=True)
        assert none[0].tolist() == [0] * (nq + 1) and none[1].size == 0 and none[2].size == 0 and none[3].size == 0 and st2[0] == 0
    assert plain[0][-1] > 0 and (st0[0] == N * nq if D == 4096 else True)


# ---- 3. the ambiguous band ------------------------------------------------------------------------------------------------------
def _band(metric):
    """tests/test_knn_range_gpu.py's construction: 2048 rows whose exact values straddle the radius in steps far below the
    sweep's error bound -- q + s_i u_i, u_i unit, s_i^2 = 1 + (i - 1024) 2^-22; l2: radius 1.0; ip: the (upper) median exact
    product rounded to fp32, the value of an actual row (out, by strictness) inside the ambiguous band"""
    rng = np.random.default_rng(7)
    D = 128
    q = rng.standard_normal(D); q /= np.linalg.norm(q)
    u = rng.standard_normal((2048, D)); u /= np.linalg.norm(u, axis=1, keepdims=True)
    s2 = 1.0 + (np.arange(2048) - 1024) * 2.0 ** -22
    P = (q[None] + np.sqrt(s2)[:, None] * u).astype(np.float32)
    Q = q[None].astype(np.float32)
    x = ref.fixed_order_values(P, Q, metric)
    rad = np.float32(1.0) if metric == "l2" else np.float32(np.sort(x[0])[1024])
    return P, Q, x, rad


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_ambiguous_band_decides_selected_pairs_only(metric, cuda_dev):
    P, Q, x, rad = _band(metric)
    # no fp64 value within 2^-40 of a point where the fp32 rounding changes sides of the radius: the verdict of every row is the
    # same for any summation order; no row is left out (this midpoint condition replaces the margin)
    r64 = np.float64(rad)
    mids = [0.5 * (r64 + np.float64(np.nextafter(rad, np.float32(-np.inf)))), 0.5 * (r64 + np.float64(np.nextafter(rad, np.float32(np.inf))))]
    near = min(np.abs(x[0] - m).min() for m in mids)
    print("nearest exact value to a deciding midpoint: %.3e" % near)
    assert near > 2.0 ** -40
    even = np.arange(2048) % 2 == 0
    store = _store(P, cuda_dev)
    plain, st = _gpu(P, Q, rad, metric, cuda_dev, store=store)
    decided, hits = {}, []
    for name, mask in (("even", even), ("odd", ~even)):
        got, s = _gpu(P, Q, rad, metric, cuda_dev, mask, store=store)
        _assert_equals_oracle(got, P, Q, rad, mask, metric, x, need_margin=False)
        assert s[0] > 0                                                       # the exact decision ran, on selected pairs
        decided[name] = s[0]
        hits.append(got[2])
    print("pairs decided exactly: even %d + odd %d, unfiltered %d" % (decided["even"], decided["odd"], st[0]))
    # the ambiguous set does not depend on the selection; each half decides exactly its own part of it
    assert decided["even"] + decided["odd"] == st[0]
    assert np.array_equal(np.sort(np.concatenate(hits)), plain[2])


# ---- 4. the id-list route -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("N,D,nq", [(5000, 768, 33), (300, 4096, 3), (70000, 64, 5)])
def test_id_list_equals_the_bitmap_route_bit_for_bit(N, D, nq, metric, cuda_dev):
    """the two routes sum a pair's exact value in the same order (a wave per pair on a big store, a lane per pair on a small
    one): same lims, I, D and D64.  (70000, 64, 5): M = 8192, the longest list; ids outside [0, N) are mixed in and skipped."""
    P, Q, mask, x, rad = sref.case(N, D, nq, metric)
    ids = np.nonzero(mask)[0][:8192 - 3] if N == 70000 else np.nonzero(mask)[0]
    listed = np.zeros(N, bool); listed[ids] = True
    mixed = np.concatenate([[-7], ids, [N, N + 1000]]).astype(np.int64)       # sorted, unique, three of them outside the store
    assert N != 70000 or mixed.size == 8192
    store = _store(P, cuda_dev)
    a, sa = _gpu_ids(P, Q, rad, metric, cuda_dev, mixed, store=store, exact_out=True)
    b, _ = _gpu(P, Q, rad, metric, cuda_dev, listed, store=store, exact_out=True)
    _assert_equals_oracle(a, P, Q, rad, listed, metric, x)
    assert _bit_equal(a, b)
    assert sa[0] == ids.size * nq                                             # the valid listed pairs, all decided exactly
    off, _ = _gpu_ids(P, Q, rad, metric, cuda_dev, mixed, store=store, row_offset=10 ** 10)
    assert np.array_equal(off[2], a[2] + 10 ** 10) and np.array_equal(off[1], a[1])


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_id_list_on_a_store_the_bitmap_route_refuses(metric, cuda_dev):
    from adaptive_classifier import _native as nv
    from adaptive_classifier import index as ix
    N, D, nq = sref.IDS_ONLY_CASE
    with pytest.raises(nv.NativeError):
        ix.knn_range_workspace_bytes(N, D, nq)                                # D beyond the sweep, N beyond the small-store path
    P, Q, mask, x, rad = sref.case(N, D, nq, metric, 0.15)
    ids = np.nonzero(mask)[0]
    assert 1 < ids.size <= 8192
    got, st = _gpu_ids(P, Q, rad, metric, cuda_dev, ids, exact_out=True)
    _assert_equals_oracle(got, P, Q, rad, mask, metric, x)
    assert st[0] == ids.size * nq and np.array_equal(got[3].astype(np.float32), got[1])


def test_id_list_edges_and_capacity(cuda_dev):
    from adaptive_classifier import _native as nv
    N, D, nq = 5000, 768, 33
    P, Q, mask, x, rad = sref.case(N, D, nq, "l2")
    store = _store(P, cuda_dev)
    (lims, Dv, I), st = _gpu_ids(P, Q, rad, "l2", cuda_dev, [], store=store)                  # M = 0
    assert lims.tolist() == [0] * (nq + 1) and Dv.size == 0 and I.size == 0 and st[0] == 0
    (lims, Dv, I), st = _gpu_ids(P, Q, rad, "l2", cuda_dev, [-3, N], store=store)             # nothing inside the store
    assert lims.tolist() == [0] * (nq + 1) and I.size == 0 and st[0] == 0
    one = int(sref.filtered_range_search(P, Q, rad, mask, "l2", values=x)[2][0])             # M = 1: a hit of query 0
    only = np.zeros(N, bool); only[one] = True
    got, st = _gpu_ids(P, Q, rad, "l2", cuda_dev, [one], store=store)
    _assert_equals_oracle(got, P, Q, rad, only, "l2", x)
    assert got[0][1] == 1 and got[2][0] == one and st[0] == nq
    (lims, Dv, I), _ = _gpu_ids(P, Q[:0], rad[:0], "l2", cuda_dev, [one], store=store)        # nq = 0
    assert lims.tolist() == [0] and Dv.size == 0 and I.size == 0
    # M = 8193 is refused; a fill whose capacity is one short writes nothing and raises the flag
    L = nv.lib()
    ids = np.nonzero(mask)[0]
    d_ids = torch.from_numpy(np.concatenate([ids, np.arange(N, N + 8193 - ids.size)]).astype(np.int64)).to(cuda_dev)
    b = ctypes.c_size_t(0)
    nv.check(L.ac_knn_range_ids_workspace(8192, nq, ctypes.byref(b)), "ws")
    ws = torch.empty(b.value, dtype=torch.uint8, device=cuda_dev)
    Qd = torch.from_numpy(Q).to(cuda_dev)
    rd = torch.from_numpy(rad).to(cuda_dev)
    lims_d = torch.empty(nq + 1, dtype=torch.int64, device=cuda_dev)
    stats = torch.zeros(4, dtype=torch.int32, device=cuda_dev)
    head = lambda M: (nv.ptr(store), N, store.stride(0), D, nv.ptr(d_ids), M, nv.ptr(Qd), nq, Qd.stride(0))
    tail = (nv.ptr(ws), ws.numel(), nv.ptr(stats), nv.stream_ptr(cuda_dev))
    with torch.cuda.device(cuda_dev):
        assert L.ac_knn_l2_range_count_ids(*head(8193), nv.ptr(rd), nv.ptr(lims_d), *tail) == -1 and b"M=8193" in L.ac_last_error()
        nv.check(L.ac_knn_l2_range_count_ids(*head(8192), nv.ptr(rd), nv.ptr(lims_d), *tail), "count")
        total = int(lims_d[-1].item())
        assert total == sref.filtered_range_search(P, Q, rad, mask, "l2", values=x)[0][-1] and total > 100
        for cap in (total - 1, total):
            outD = torch.full((total + 8,), -7.0, dtype=torch.float32, device=cuda_dev)
            outI = torch.full((total + 8,), -7, dtype=torch.int64, device=cuda_dev)
            nv.check(L.ac_knn_l2_range_fill_ids(*head(8192), 0, nv.ptr(lims_d), cap, nv.ptr(outD), None, nv.ptr(outI), *tail), "fill")
            torch.cuda.synchronize()
            if cap < total:
                assert stats[1].item() == 1 and bool((outI == -7).all()) and bool((outD == -7.0).all())
            else:
                assert stats[1].item() == 0 and bool((outI[:total] >= 0).all()) and bool((outI[total:] == -7).all())
        assert L.ac_knn_l2_range_count_ids(*head(8192), nv.ptr(rd), nv.ptr(lims_d), nv.ptr(ws), 16, nv.ptr(stats),
                                           nv.stream_ptr(cuda_dev)) == -3                      # a workspace that is too small


# ---- 5. the flat indexes --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_flat_index_filtered_range_search_follows_row_changes(metric, cuda_dev):
    from adaptive_classifier.index import HipFlatIPIndex, HipFlatL2Index, RowSelector
    D = 40
    rows = ref.unit_rows(600, D, 21)
    Q = ref.unit_rows(5, D, 22)
    idx = (HipFlatIPIndex if metric == "ip" else HipFlatL2Index)(D, device=cuda_dev)

    def check(P):
        n = P.shape[0]
        mask = np.random.default_rng(n).random(n) < 0.5
        x = ref.fixed_order_values(P, Q, metric)
        rad = ref.gap_radii(x[:, mask], metric, 10, 40)
        assert sref.margin(x, mask, rad) >= 64
        olims, oD, oI = sref.filtered_range_search(P, Q, rad, mask, metric, values=x)
        r = torch.from_numpy(rad)
        for sel in (mask, torch.from_numpy(mask).to(cuda_dev), np.nonzero(mask)[0][::-1].copy(),       # bool masks, ids (any order),
                    RowSelector.from_mask(mask, device=cuda_dev), RowSelector.from_ids(np.nonzero(mask)[0], n, device=cuda_dev)):
            lims, Dv, I = idx.range_search(Q, r, sel=sel)
            assert lims.dtype == np.int64 and Dv.dtype == np.float32 and I.dtype == np.int64
            assert np.array_equal(lims, olims) and np.array_equal(I, oI) and _ulp_close(Dv, oD)
        assert idx._prepared is None                                    # no fp16 plane was built for it
        for bad in (np.zeros(n + 1, bool), RowSelector.from_mask(np.zeros(n - 1, bool), device=cuda_dev)):
            with pytest.raises(ValueError):
                idx.range_search(Q, r, sel=bad)                         # a selector of the wrong length

    idx.add(rows[:400])                                                 # queued on the host: range_search materialises first
    assert idx._npending == 400
    check(rows[:400])
    idx.add(torch.from_numpy(rows[400:500]).to(cuda_dev))
    check(rows[:500])
    cur = rows[:500].copy()
    cur[[3, 77, 499]] = rows[500:503]
    idx.update_rows([3, 77, 499], rows[500:503])
    check(cur)
    idx.remove_ids(np.array([0, 5, 77, 300]))
    cur = np.delete(cur, [0, 5, 77, 300], axis=0)
    check(cur)


# ---- 6. PrototypeMemory.prototypes_within(among=) -------------------------------------------------------------------------------
def test_prototypes_within_among(cuda_dev, monkeypatch):
    from adaptive_classifier import index as ix
    from adaptive_classifier.memory import PrototypeMemory
    from adaptive_classifier.models import Example
    routes = []
    ids_fn, bitmap_fn = ix.knn_range_ids, ix.knn_range_search
    monkeypatch.setattr(ix, "knn_range_ids", lambda *a, **k: routes.append("ids") or ids_fn(*a, **k))
    monkeypatch.setattr(ix, "knn_range_search", lambda *a, **k: routes.append("bitmap" if k.get("sel") is not None else "plain") or bitmap_fn(*a, **k))
    D = 32
    rng = np.random.default_rng(5)
    centres = ref.unit_rows(6, D, 31)
    mem = PrototypeMemory(D, device=cuda_dev)
    labels = ["a", "b", "c", "d", "e", "f"]
    for i, l in enumerate(labels):
        for _ in range(2):
            mem.add_example(Example("t", l, torch.from_numpy((centres[i] + 0.01 * rng.standard_normal(D)).astype(np.float32))), l)
    mem._rebuild_index()
    q = torch.from_numpy(centres[1].astype(np.float32))
    full = mem.prototypes_within(q, 1e9)
    assert len(full) == 6 and routes == ["plain"]
    for among in (["b", "e", "a"], ["f"], ["c", "nope"], {"a", "b", "c", "d", "e", "f"}):
        got = mem.prototypes_within(q, 1e9, among=among)
        assert got == [g for g in full if g[0] in among]                # the unfiltered result filtered by label: order, values
    assert routes[1:] == ["ids"] * 4                                    # one prototype per class: the id-list route
    near = mem.prototypes_within(q, 1.0)
    assert [g[0] for g in near] == ["b"]
    assert mem.prototypes_within(q, 1.0, among=["b", "c"]) == near and mem.prototypes_within(q, 1.0, among=["c", "d"]) == []
    assert mem.prototypes_within(q, 1e9, among=[]) == [] and mem.prototypes_within(q, 1e9, among=["nope"]) == []
    # a load_rows() store: the class bitmap
    del routes[:]
    rows = ref.unit_rows(500, D, 33)
    rows[400] = rows[7]
    row_labels = torch.from_numpy((np.arange(500) % 3).astype(np.int32))
    mem2 = PrototypeMemory(D, device=cuda_dev)
    mem2.load_rows(_store(rows, cuda_dev), row_labels, ["x", "y", "z"])
    qv = ref.unit_rows(1, D, 34)
    x = ref.fixed_order_values(rows, qv, "l2")
    rad = float(max(ref.gap_radii(x, "l2", 30, 60)[0], np.nextafter(np.float32(x[0, 7]), np.float32(np.inf))))
    assert ref.margin_ulps(np.delete(x[0], [7, 400]), rad) >= 64
    full = mem2.prototypes_within(torch.from_numpy(qv[0]), rad)
    assert len(full) >= 30 and {g[0] for g in full} == {"x", "y", "z"}
    for among in (["x"], ["y", "z"], ["z", "nope"], ["x", "y", "z"]):
        assert mem2.prototypes_within(torch.from_numpy(qv[0]), rad, among=among) == [g for g in full if g[0] in among]
    assert routes == ["plain"] + ["bitmap"] * 4
    assert mem2.prototypes_within(torch.from_numpy(qv[0]), rad, among=[]) == [] and mem2.prototypes_within(torch.from_numpy(qv[0]), rad, among=["nope"]) == []
    assert routes == ["plain"] + ["bitmap"] * 4                         # an empty selection searches nothing


# ---- 7. logical row shards on one GPU -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("N,D,nq", [(5000, 768, 33), (300, 4096, 3)])
def test_row_shards_concatenate_to_the_unsharded_result(N, D, nq, metric, cuda_dev):
    """2 / 4 / 8 contiguous shards, each searched with row_offset (and sel_bit0 = row_offset on the GLOBAL bitmap), concatenated
    per query in shard order = the unsharded call, bit for bit.  Every shard is on the same side of the small-store boundary as
    the full store (D = 768: the sweep at any N; D = 4096: N <= 8192 everywhere), so every value is summed in the same order."""
    from adaptive_classifier import index as ix
    from adaptive_classifier.sharded import shard_bounds
    P, Q, mask, x, rad = sref.case(N, D, nq, metric)
    store = _store(P, cuda_dev)
    Qd = torch.tensor(Q, device=cuda_dev)
    rd = _rad(rad, cuda_dev)
    words = _words(mask, cuda_dev)
    for sel in (None, words):
        whole = ix.knn_range_search(store, N, D, Qd, rd, metric=metric, exact_out=True, sel=sel)
        whole = [t.cpu().numpy() for t in whole]
        if sel is not None:
            _assert_equals_oracle(whole, P, Q, rad, mask, metric, x)
        for world in (2, 4, 8):
            parts = []
            for g in range(world):
                lo, hi = shard_bounds(N, world, g)
                parts.append([t.cpu().numpy() for t in ix.knn_range_search(store[lo:hi], hi - lo, D, Qd, rd, metric=metric, row_offset=lo,
                                                                         exact_out=True, sel=sel, sel_bit0=lo)])
            lims = np.concatenate([[0], np.cumsum(sum(np.diff(p[0]) for p in parts))])
            cat = lambda k: np.concatenate([p[k][p[0][q]: p[0][q + 1]] for q in range(nq) for p in parts])
            assert np.array_equal(lims, whole[0]) and all(np.array_equal(cat(k), whole[k]) for k in (1, 2, 3)), (world, sel is not None)
