"""Range search on the GPU (ac_knn_l2_range_* / ac_knn_ip_range_* through the C ABI, knn_range_search, the flat indexes,
PrototypeMemory.prototypes_within) against the fp64 oracle tests/knn_range_ref.py.

Bar: lims and ids EQUAL to the oracle's for every query -- no query is left out; the tests first assert that no value lies within
64 ulps of its radius (the oracle sums in another order than the library, so only such a value could be decided differently) --
and D within 1 ulp (equal where the arithmetic is exact)."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import knn_range_ref as ref  # noqa: E402

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


def _gpu(P, Q, rad, metric, dev, store=None, **kw):
    """knn_range_search -> numpy (lims, D, I[, exact]) and d_stats as a list"""
    from adaptive_classifier import index as ix
    store = _store(P, dev) if store is None else store
    stats = torch.zeros(4, dtype=torch.int32, device=dev)
    r = torch.from_numpy(np.asarray(rad, np.float32)).to(dev) if np.ndim(rad) else float(rad)
    out = ix.knn_range_search(store, P.shape[0], P.shape[1], torch.tensor(Q, device=dev), r, metric=metric, stats=stats, **kw)
    torch.cuda.synchronize()
    return tuple(o.cpu().numpy() for o in out), stats.tolist()


@functools.lru_cache(maxsize=None)
def _case(N, D, nq, metric):
    """rows, queries, exact values and per-query gap radii (ranks 20..60) of one shape: computed once, shared, never modified"""
    P, Q = ref.unit_rows(N, D, 1), ref.unit_rows(nq, D, 2)
    x = ref.fixed_order_values(P, Q, metric)
    rad = ref.gap_radii(x, metric, 20, 60)
    for a in (P, Q, x, rad):
        a.setflags(write=False)
    return P, Q, x, rad


def _assert_equals_oracle(got, P, Q, rad, metric, x=None, row_offset=0, need_margin=True):
    lims, D, I = got[:3]
    x = ref.fixed_order_values(P, Q, metric) if x is None else x
    radv = np.broadcast_to(np.asarray(rad, np.float32), (Q.shape[0],))
    finite = [q for q in range(Q.shape[0]) if np.isfinite(radv[q]) and x.shape[1]]
    margin = min([ref.margin_ulps(x[q], radv[q]) for q in finite], default=np.inf)
    print("min margin %.1f ulps" % margin)
    assert margin >= 64 or not need_margin, "a value sits too close to its radius for a summation-order independent verdict"
    olims, oD, oI = ref.range_search(P, Q, rad, metric, row_offset=row_offset, values=x)
    assert lims.dtype == np.int64 and I.dtype == np.int64 and D.dtype == np.float32
    assert np.array_equal(lims, olims), (lims, olims)
    assert np.array_equal(I, oI), f"id mismatch: {(I != oI).sum()} of {I.size}"
    assert _ulp_close(D, oD)
    for q in range(Q.shape[0]):                              # every returned D satisfies the predicate; ids ascend
        seg = slice(lims[q], lims[q + 1])
        assert ref.is_hit(D[seg], radv[q], metric).all() and np.all(np.diff(I[seg]) > 0)


# ---- 1. oracle equality --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("N,D,nq", [
    (5000, 768, 33),         # two 32-query tiles + a ragged third; N % 128 != 0
    (1153, 100, 17),         # D % 16 != 0 (tail group), 17 queries: across the 16 / 32 tile edge
    (70000, 64, 5),          # more tiles than blocks: several tiles per block, 18 strips per query
    (300, 4096, 3),          # D too wide for the LDS query tile: the small-store kernel
    (65537, 32, 1),          # N = 2^16 + 1: one row in the last tile / word / strip
    (999, 770, 7),           # D % 4 != 0 (zero padded leading dimension)
])
def test_range_matches_oracle(N, D, nq, metric, cuda_dev):
    P, Q, x, rad = _case(N, D, nq, metric)
    got, st = _gpu(P, Q, rad, metric, cuda_dev, exact_out=True)
    _assert_equals_oracle(got, P, Q, rad, metric, x)
    assert 21 <= np.diff(got[0]).min() and np.diff(got[0]).max() <= 60
    assert np.array_equal(got[3].astype(np.float32), got[1])            # D is the fp64 output rounded once
    if D == 4096:
        assert st[0] == N * nq                                          # the small-store kernel decides every pair exactly


# ---- 2. the ambiguous band -----------------------------------------------------------------------------------------------------
def _band(metric):
    """2048 rows whose exact values straddle the radius in steps far below the sweep's error bound: q + s_i u_i, u_i unit,
    s_i^2 = 1 + (i - 1024) 2^-22 -- squared distances ~ s_i^2 around radius 1.0 (l2).  ip: the radius is the (upper) median exact
    product rounded to fp32 -- the value of an actual row, which therefore sits AT the radius (out, by strictness) and inside the
    ambiguous band however narrow the bound is (the products 1 + s_i q.u_i spread over 0.7 .. 1.3, so a radius BETWEEN two rows is
    farther from both than the bound E / 2 ~ 2.6e-5 at D = 128)"""
    rng = np.random.default_rng(7)
    D = 128
    q = rng.standard_normal(D); q /= np.linalg.norm(q)
    u = rng.standard_normal((2048, D)); u /= np.linalg.norm(u, axis=1, keepdims=True)
    s2 = 1.0 + (np.arange(2048) - 1024) * 2.0 ** -22
    P = (q[None] + np.sqrt(s2)[:, None] * u).astype(np.float32)
    Q = q[None].astype(np.float32)
    x = ref.fixed_order_values(P, Q, metric)
    if metric == "l2":
        rad = np.float32(1.0)
    else:
        rad = np.float32(np.sort(x[0])[1024])
    return P, Q, x, rad


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_ambiguous_band_is_decided_exactly(metric, cuda_dev):
    P, Q, x, rad = _band(metric)
    # no fp64 value within 2^-40 of a point where the fp32 rounding changes sides of the radius (the midpoints between the radius
    # and its two fp32 neighbours): the verdict of every row is the same for any summation order; no row is left out
    r64 = np.float64(rad)
    mids = [0.5 * (r64 + np.float64(np.nextafter(rad, np.float32(-np.inf)))), 0.5 * (r64 + np.float64(np.nextafter(rad, np.float32(np.inf))))]
    near = min(np.abs(x[0] - m).min() for m in mids)
    print("nearest exact value to a deciding midpoint: %.3e" % near)
    assert near > 2.0 ** -40
    n_at = int((x[0].astype(np.float32) == rad).sum())
    olims = ref.range_search(P, Q, rad, metric, values=x)[0]
    print("oracle hits %d of 2048, rows rounding to the radius itself: %d" % (olims[1], n_at))
    assert n_at == 1 and olims[1] == (1024 if metric == "l2" else 1023)     # one row rounds to the radius itself: out, by strictness
    got, st = _gpu(P, Q, rad, metric, cuda_dev)
    _assert_equals_oracle(got, P, Q, rad, metric, x, need_margin=False)      # (the midpoint condition above replaces the margin)
    assert st[0] > 0                                                    # the exact decision ran in the count phase
    print("pairs decided exactly: %d" % st[0])


# ---- 3. exact ties and strictness ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_ties_at_the_radius_are_all_out_and_one_step_further_all_in(metric, cuda_dev):
    rng = np.random.default_rng(11)
    P = rng.integers(-3, 4, (300, 24)).astype(np.float32)
    P[200:220] = P[17]                                                  # duplicates: all in or all out
    Q = rng.integers(-3, 4, (4, 24)).astype(np.float32)
    x = ref.fixed_order_values(P, Q, metric)                            # integers: exact in every arithmetic involved
    store = _store(P, cuda_dev)
    for q in range(4):
        v = np.float32(x[q, 17])                                        # held by rows 17, 200..219 (and maybe more)
        held = np.nonzero(x[q] == v)[0]
        assert held.size >= 21
        (lims, D, I), _ = _gpu(P, Q[q:q + 1], v, metric, cuda_dev, store=store)
        assert not np.isin(held, I).any()
        step = np.nextafter(v, np.float32(np.inf if metric == "l2" else -np.inf))
        if metric == "l2" and v == 0:
            continue
        (lims2, D2, I2), _ = _gpu(P, Q[q:q + 1], step, metric, cuda_dev, store=store)
        assert np.isin(held, I2).all() and I2.size == I.size + held.size
        for rad, got in ((v, (lims, D, I)), (step, (lims2, D2, I2))):
            olims, oD, oI = ref.range_search(P, Q[q:q + 1], rad, metric, values=x[q:q + 1])
            assert np.array_equal(got[0], olims) and np.array_equal(got[2], oI) and np.array_equal(got[1], oD)       # D equal: exact


# ---- 4. edge cases -------------------------------------------------------------------------------------------------------------
def test_edge_radii_empty_inputs_offsets_and_capacity(cuda_dev):
    from adaptive_classifier import _native as nv
    from adaptive_classifier import index as ix
    P, Q = ref.unit_rows(1000, 48, 3), ref.unit_rows(6, 48, 4)
    store = _store(P, cuda_dev)
    x = ref.fixed_order_values(P, Q, "l2")
    for r in (0.0, -1.0, np.nan):
        (lims, D, I), _ = _gpu(P, Q, r, "l2", cuda_dev, store=store)
        assert lims.tolist() == [0] * 7 and D.size == 0 and I.size == 0
    (lims, D, I), _ = _gpu(P, Q, np.inf, "l2", cuda_dev, store=store, row_offset=10 ** 10)
    assert lims.tolist() == [1000 * i for i in range(7)]
    assert np.array_equal(I, np.tile(np.arange(1000, dtype=np.int64) + 10 ** 10, 6))               # every row, in id order
    assert _ulp_close(D, x.astype(np.float32).reshape(-1))
    xi = ref.fixed_order_values(P, Q, "ip")
    (lims, D, I), _ = _gpu(P, Q, -np.inf, "ip", cuda_dev, store=store)
    assert lims[-1] == 6000 and _ulp_close(D, xi.astype(np.float32).reshape(-1))
    for r in (np.inf, np.nan):
        assert _gpu(P, Q, r, "ip", cuda_dev, store=store)[0][0].tolist() == [0] * 7
    # per-query radii: queries without hits between queries with many
    rad = np.array([np.inf, 0.0, 2.0, np.nan, -3.0, 1.9], np.float32)
    got, _ = _gpu(P, Q, rad, "l2", cuda_dev, store=store)
    _assert_equals_oracle(got, P, Q, rad, "l2", x)
    assert np.diff(got[0])[[1, 3, 4]].tolist() == [0, 0, 0] and np.diff(got[0])[0] == 1000 and np.diff(got[0])[2] > 100
    # N = 0 and nq = 0
    (lims, D, I), _ = _gpu(P[:0], Q, 1.0, "l2", cuda_dev)
    assert lims.tolist() == [0] * 7 and D.size == 0
    (lims, D, I), _ = _gpu(P, Q[:0], 1.0, "l2", cuda_dev, store=store)
    assert lims.tolist() == [0] and D.size == 0 and I.size == 0
    # capacity too small: nothing is written past it (here: nothing at all), the flag is raised
    L = nv.lib()
    b = ctypes.c_size_t(0)
    nv.check(L.ac_knn_range_workspace(1000, 48, 6, ctypes.byref(b)), "ws")
    ws = torch.empty(b.value, dtype=torch.uint8, device=cuda_dev)
    Qd = torch.from_numpy(Q).to(cuda_dev)
    rd = torch.from_numpy(np.full(6, 2.0, np.float32)).to(cuda_dev)
    lims_d = torch.empty(7, dtype=torch.int64, device=cuda_dev)
    stats = torch.zeros(4, dtype=torch.int32, device=cuda_dev)
    with torch.cuda.device(cuda_dev):
        nv.check(L.ac_knn_l2_range_count(nv.ptr(store), 1000, store.stride(0), 48, nv.ptr(Qd), 6, Qd.stride(0), nv.ptr(rd), nv.ptr(lims_d),
                                         nv.ptr(ws), ws.numel(), nv.ptr(stats), nv.stream_ptr(cuda_dev)), "count")
        total = int(lims_d[-1].item())
        assert total > 100
        for cap in (total - 1, total):
            outD = torch.full((total + 8,), -7.0, dtype=torch.float32, device=cuda_dev)
            outI = torch.full((total + 8,), -7, dtype=torch.int64, device=cuda_dev)
            nv.check(L.ac_knn_l2_range_fill(nv.ptr(store), 1000, store.stride(0), 48, nv.ptr(Qd), 6, Qd.stride(0), 0, nv.ptr(lims_d), cap,
                                            nv.ptr(outD), None, nv.ptr(outI), nv.ptr(ws), ws.numel(), nv.ptr(stats), nv.stream_ptr(cuda_dev)), "fill")
            torch.cuda.synchronize()
            if cap < total:
                assert stats[1].item() == 1 and bool((outI == -7).all()) and bool((outD == -7.0).all())
            else:
                assert stats[1].item() == 0 and bool((outI[:total] >= 0).all()) and bool((outI[total:] == -7).all())
        # a workspace that is too small is refused, as for the top-k search
        assert L.ac_knn_l2_range_count(nv.ptr(store), 1000, store.stride(0), 48, nv.ptr(Qd), 6, Qd.stride(0), nv.ptr(rd), nv.ptr(lims_d),
                                       nv.ptr(ws), 16, nv.ptr(stats), nv.stream_ptr(cuda_dev)) == -3
    assert ix.knn_range_workspace_bytes(1000, 48, 6) == b.value
    # one planner rule for both searches (a 16-query tile + the k = 1 lists against the LDS limit): D = 2304 is the last dimension
    # the sweep takes (ng = 18: 155 872 B), D = 2308 the first it does not (ng = 19: 164 064 B > 163 840), and then only a store of
    # <= 8192 rows is searched.  Host-only calls.
    t = ctypes.c_size_t(0)
    for N, D, want in ((8193, 2304, 0), (8192, 2308, 0), (8193, 2308, -2)):
        assert L.ac_knn_range_workspace(N, D, 6, ctypes.byref(b)) == want, (N, D)
        assert L.ac_knn_l2_topk_workspace(N, D, 6, 1, ctypes.byref(t)) == want, (N, D)


# ---- 5. consistency with search ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_range_equals_thresholded_full_search(metric, cuda_dev):
    from adaptive_classifier import index as ix
    N, D, nq = 2000, 96, 8
    P, Q, x, rad = _case(N, D, nq, metric)
    store = _store(P, cuda_dev)
    search = ix.knn_ip_topk if metric == "ip" else ix.knn_l2_topk
    sD, sI = search(store, N, D, torch.tensor(Q, device=cuda_dev), N)
    sD, sI = sD.cpu().numpy(), sI.cpu().numpy()
    (lims, rD, rI), _ = _gpu(P, Q, rad, metric, cuda_dev, store=store)
    for q in range(nq):
        keep = ref.is_hit(sD[q], rad[q], metric)
        order = np.argsort(sI[q][keep])                                 # the search lists by value, the range result by id
        seg = slice(lims[q], lims[q + 1])
        assert np.array_equal(rI[seg], sI[q][keep][order])
        assert np.array_equal(rD[seg], sD[q][keep][order])


# ---- 6. chunking ---------------------------------------------------------------------------------------------------------------
def test_result_does_not_depend_on_calls_or_chunking(cuda_dev):
    from adaptive_classifier import index as ix
    N, D, nq = 70000, 64, 40
    P, Q = ref.unit_rows(N, D, 1), ref.unit_rows(nq, D, 5)
    store = _store(P, cuda_dev)
    Qd = torch.from_numpy(Q).to(cuda_dev)
    sD, _ = ix.knn_l2_topk(store, N, D, Qd, 41)
    s = sD.cpu().numpy()
    rad = np.array([ref.gap_radius(s[q], 20, 40) for q in range(nq)], np.float32)
    a, _ = _gpu(P, Q, rad, "l2", cuda_dev, store=store)
    b, _ = _gpu(P, Q, rad, "l2", cuda_dev, store=store)
    assert all(np.array_equal(u, v) for u, v in zip(a, b))              # two calls: bit-equal
    assert 21 <= np.diff(a[0]).min() and np.diff(a[0]).max() <= 40
    assert ix.range_query_chunk(N, D, nq, 100_000) * 3 <= nq
    c, _ = _gpu(P, Q, rad, "l2", cuda_dev, store=store, max_ws_bytes=100_000)                       # >= 3 chunks
    assert all(np.array_equal(u, v) for u, v in zip(a, c))
    parts = [_gpu(P, Q[q:q + 1], rad[q:q + 1], "l2", cuda_dev, store=store)[0] for q in range(nq)]  # one query at a time
    assert np.array_equal(np.concatenate([p[2] for p in parts]), a[2])
    assert np.array_equal(np.concatenate([p[1] for p in parts]), a[1])
    assert np.array_equal(np.cumsum([0] + [p[0][1] for p in parts]), a[0])


# ---- 7. index and memory level -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_flat_index_range_search_follows_row_changes(metric, cuda_dev):
    from adaptive_classifier.index import HipFlatIPIndex, HipFlatL2Index
    D = 40
    rows = ref.unit_rows(600, D, 21)
    Q = ref.unit_rows(5, D, 22)
    idx = (HipFlatIPIndex if metric == "ip" else HipFlatL2Index)(D, device=cuda_dev)

    def check(P):
        x = ref.fixed_order_values(P, Q, metric)
        rad = ref.gap_radii(x, metric, 10, 40)
        for r in (rad, float(rad[0])):                                  # per-query radii (tensor) and one float
            assert min(ref.margin_ulps(x[q], np.broadcast_to(r, (5,))[q]) for q in range(5)) >= 64
            lims, Dv, I = idx.range_search(Q, torch.from_numpy(r) if np.ndim(r) else r)
            olims, oD, oI = ref.range_search(P, Q, r, metric, values=x)
            assert lims.dtype == np.int64 and Dv.dtype == np.float32 and I.dtype == np.int64
            assert np.array_equal(lims, olims) and np.array_equal(I, oI) and _ulp_close(Dv, oD)
        assert idx._prepared is None                                    # no fp16 plane was built for it

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
    idx.add(rows[503:520])                                              # queued rows on top of resident ones
    check(np.concatenate([cur, rows[503:520]]))


def test_prototypes_within(cuda_dev):
    from adaptive_classifier.memory import PrototypeMemory
    from adaptive_classifier.models import Example
    D = 32
    rng = np.random.default_rng(5)
    centres = ref.unit_rows(4, D, 31) * 3
    mem = PrototypeMemory(D, device=cuda_dev)
    labels = ["a", "b", "c", "d"]
    for i, l in enumerate(labels):
        for _ in range(3):
            e = torch.from_numpy((centres[i] + 0.01 * rng.standard_normal(D)).astype(np.float32))
            mem.add_example(Example("t", l, e), l)
    mem._rebuild_index()
    e = torch.from_numpy((centres[1] + 0.01 * rng.standard_normal(D)).astype(np.float32))
    mem.add_example(Example("t", "b", e), "b")                          # prototype "b" is dirty now: flushed by the query
    assert "b" in mem._dirty
    protos = np.stack([mem.prototypes[l].float().numpy() for l in sorted(labels)])
    q = torch.from_numpy(centres[1].astype(np.float32))
    d = ref.fixed_order_values(protos, q[None].numpy(), "l2")[0]
    assert mem.prototypes_within(q, 1e-6) == []
    got = mem.prototypes_within(q, 1.0)
    assert [g[0] for g in got] == ["b"] and abs(got[0][1] - d[1]) <= 1e-6 * d[1] + 1e-12
    got = mem.prototypes_within(q, 1e9)
    assert [g[0] for g in got] == [sorted(labels)[i] for i in np.lexsort((np.arange(4), d.astype(np.float32)))]
    assert _ulp_close([g[1] for g in got], np.sort(d.astype(np.float32)))
    # a load_rows() store: labels through the row -> class map; ties (duplicate rows) to the lower row
    rows = ref.unit_rows(500, D, 33)
    rows[400] = rows[7]
    row_labels = torch.from_numpy((np.arange(500) % 3).astype(np.int32))
    mem2 = PrototypeMemory(D, device=cuda_dev)
    mem2.load_rows(_store(rows, cuda_dev), row_labels, ["x", "y", "z"])
    qv = ref.unit_rows(1, D, 34)
    x = ref.fixed_order_values(rows, qv, "l2")
    rad = ref.gap_radii(x, "l2", 10, 30)[0]
    rad = max(rad, np.nextafter(np.float32(x[0, 7]), np.float32(np.inf)))                           # the duplicates are inside
    got = mem2.prototypes_within(torch.from_numpy(qv[0]), float(rad))
    _, oD, oI = ref.range_search(rows, qv, rad, "l2", values=x)
    order = np.lexsort((oI, oD))
    assert [g[0] for g in got] == [["x", "y", "z"][i % 3] for i in oI[order]]
    assert _ulp_close([g[1] for g in got], oD[order])
    at = list(oI[order]).index(7)
    assert oI[order][at + 1] == 400 and got[at][1] == got[at + 1][1]
