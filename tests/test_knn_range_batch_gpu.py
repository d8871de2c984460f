"""Range search over the PREPARED fp16-plane store on the GPU (ac_knn_*_range_count_batch[_sel] + the unchanged fill, through
knn_range_search(prepared=), the flat indexes and PrototypeMemory.prototypes_within) against the fp64 oracle
tests/knn_range_ref.py and against the fp32 route.

Bar: lims and ids EQUAL to the oracle's for every query (after asserting that no value lies within 64 ulps of its radius), D
within 1 ulp; and lims / I / D / D64 EQUAL, bit for bit, to knn_range_search without `prepared` at ANY radius -- both routes decide
every pair that is not certain by the same exact value.  d_stats[2] == 2 says that the plane sweep ran; d_stats[0] (pairs decided
exactly) is capped by the pairs the a-priori bound E_q cannot decide, so a kernel that calls everything ambiguous does not pass."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import knn_range_batch_ref as bref  # noqa: E402
import knn_range_ref as ref  # noqa: E402
import knn_range_sel_ref as sref  # noqa: E402

pytestmark = pytest.mark.gpu


def _ulp_close(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and np.all(np.abs(a - b) <= np.spacing(np.maximum(np.abs(a), np.abs(b)).astype(np.float32)))


def _bit_equal(a, b):
    return len(a) == len(b) and all(u.dtype == v.dtype and np.array_equal(u, v) for u, v in zip(a, b))


def _prepared_store(P, dev):
    """(store, (planes, norms)) of the rows P"""
    from adaptive_classifier import index as ix
    ld = (P.shape[1] + 3) // 4 * 4
    store = torch.zeros((P.shape[0], ld), dtype=torch.float32, device=dev)
    store[:, : P.shape[1]] = torch.tensor(P, device=dev)                       # (a copy: the shared inputs are read-only)
    return store, ix.prepare_store(store, P.shape[0], P.shape[1])


@functools.lru_cache(maxsize=None)
def _case_store(N, D, dev):
    """the device store of a shared shape (the rows do not depend on the metric or on nq): built once"""
    return _prepared_store(ref.unit_rows(N, D, 1), dev)


def _words(mask, dev, bit0=0):
    return torch.from_numpy(sref.pack(mask, bit0).view(np.int64).copy()).to(dev)


def _gpu(sp, n, D, Q, rad, metric, dev, plane=True, mask=None, bit0=0, **kw):
    """knn_range_search over sp = (store, prepared) -> numpy (lims, D, I[, exact]) and d_stats as a list; plane=False: the fp32 route"""
    from adaptive_classifier import index as ix
    store, prepared = sp
    stats = torch.zeros(4, dtype=torch.int32, device=dev)
    r = torch.tensor(np.asarray(rad, np.float32), device=dev) if np.ndim(rad) else float(rad)
    sel = {} if mask is None else {"sel": _words(mask, dev, bit0), "sel_bit0": bit0}
    out = ix.knn_range_search(store, n, D, torch.tensor(Q, device=dev), r, metric=metric, stats=stats,
                              prepared=prepared if plane else None, **sel, **kw)
    torch.cuda.synchronize()
    return tuple(o.cpu().numpy() for o in out), stats.tolist()


def _assert_equals_oracle(got, P, Q, rad, metric, x, row_offset=0, need_margin=True, mask=None):
    lims, D, I = got[:3]
    radv = np.broadcast_to(np.asarray(rad, np.float32), (Q.shape[0],))
    if need_margin:
        margin = bref.min_margin(x, radv)
        print("min margin %.1f ulps" % margin)
        assert margin >= 64, "a value sits too close to its radius for a summation-order independent verdict"
    olims, oD, oI = sref.filtered_range_search(P, Q, rad, np.ones(P.shape[0], bool) if mask is None else mask, metric,
                                               row_offset=row_offset, values=x)
    assert lims.dtype == np.int64 and I.dtype == np.int64 and D.dtype == np.float32
    assert np.array_equal(lims, olims), (lims, olims)
    assert np.array_equal(I, oI), f"id mismatch: {(I != oI).sum()} of {I.size}"
    assert _ulp_close(D, oD)
    for q in range(Q.shape[0]):                              # every returned D satisfies the predicate; ids ascend
        seg = slice(lims[q], lims[q + 1])
        assert ref.is_hit(D[seg], radv[q], metric).all() and np.all(np.diff(I[seg]) > 0)


# ---- 1. oracle equality --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("N,D,nq", bref.CASES)
def test_plane_range_matches_oracle(N, D, nq, metric, cuda_dev):
    P, Q, x, rad = bref.case(N, D, nq, metric)
    got, st = _gpu(_case_store(N, D, cuda_dev), N, D, Q, rad, metric, cuda_dev, exact_out=True)
    _assert_equals_oracle(got, P, Q, rad, metric, x)
    assert 21 <= np.diff(got[0]).min() and np.diff(got[0]).max() <= 59
    assert np.array_equal(got[3].astype(np.float32), got[1])            # D is the fp64 output rounded once
    cap = bref.undecided_cap(x, rad, bref.bound(P, Q), metric)
    print("stats", st, "cap on the pairs decided exactly: %d of %d" % (cap, N * nq))
    assert st[2] == 2 and st[1] == 0 and st[3] == 0                     # the plane sweep ran
    assert 0 <= st[0] <= cap                                            # ... and decided what the bound lets it decide


# ---- 2. bit equality with the fp32 route at radii that sit ON values -----------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("N,D,nq", bref.CASES)
def test_plane_range_equals_fp32_route_at_radii_on_values(N, D, nq, metric, cuda_dev):
    P, Q, x, _ = bref.case(N, D, nq, metric)
    sp = _case_store(N, D, cuda_dev)
    s = np.sort(x.astype(np.float32), axis=1)
    if metric == "ip":
        s = s[:, ::-1]
    for rank in (10, 30, 50):
        rad = np.ascontiguousarray(s[:, rank])                          # the fp32 value of a row: ties AT the radius exist
        a, sa = _gpu(sp, N, D, Q, rad, metric, cuda_dev, exact_out=True)
        b, sb = _gpu(sp, N, D, Q, rad, metric, cuda_dev, plane=False, exact_out=True)
        assert sa[2] == 2 and sb[2] == 0
        assert _bit_equal(a, b), (rank, a[0], b[0])
        assert np.diff(a[0]).max() <= rank + 1                          # strict: the row at the radius is out (near-ties may join it)
        assert sa[0] >= nq                                              # the row AT the radius can never be certain


# ---- 3. the ambiguous band -----------------------------------------------------------------------------------------------------
def _band(metric):
    """tests/test_knn_range_gpu.py _band: 2048 rows q + s_i u_i, s_i^2 = 1 + (i - 1024) 2^-22, whose exact values straddle the
    radius in steps far below the fp16 error -- embedded at every 32nd row of a 66 000-row store (one band row per 32-row wave
    tile) whose other rows are far from the radius: 10 x unit rows for l2 (squared distances ~ 101 against the radius 1), rows
    ~ -60 q for ip (products ~ -60 against a radius ~ 1; their norm also widens E_q / 2 to ~ 0.95, well beyond the spread +- 0.31
    of the band's products: in either metric every band value lies deep inside the zone the two thresholds leave undecided)"""
    rng = np.random.default_rng(7)
    D, N = 128, 66000
    q = rng.standard_normal(D); q /= np.linalg.norm(q)
    u = rng.standard_normal((2048, D)); u /= np.linalg.norm(u, axis=1, keepdims=True)
    s2 = 1.0 + (np.arange(2048) - 1024) * 2.0 ** -22
    band = (q[None] + np.sqrt(s2)[:, None] * u).astype(np.float32)
    far = ref.unit_rows(N, D, 9).astype(np.float64)
    P = (10.0 * far if metric == "l2" else -60.0 * q[None] + far).astype(np.float32)
    at = np.arange(2048) * 32
    P[at] = band
    Q = q[None].astype(np.float32)
    x = ref.fixed_order_values(P, Q, metric)
    rad = np.float32(1.0) if metric == "l2" else np.float32(np.sort(x[0, at])[1024])
    return P, Q, x, rad, at


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_ambiguous_band_is_decided_exactly(metric, cuda_dev):
    P, Q, x, rad, at = _band(metric)
    N, D = P.shape
    # no fp64 value of ANY row within 2^-40 of a point where the fp32 rounding changes sides of the radius
    r64 = np.float64(rad)
    mids = [0.5 * (r64 + np.float64(np.nextafter(rad, np.float32(-np.inf)))), 0.5 * (r64 + np.float64(np.nextafter(rad, np.float32(np.inf))))]
    near = min(np.abs(x[0] - m).min() for m in mids)
    print("nearest exact value to a deciding midpoint: %.3e" % near)
    assert near > 2.0 ** -40
    others = np.delete(x[0], at)
    E = bref.bound(P, Q)[0]
    assert np.abs(others - r64).min() > 4 * E                           # the other rows are far from the radius
    # the band sits within 0.8 of the zone's half width (E_q in l2 value space, E_q / 2 in product space): undecided unless the
    # sweep value were off by more than 0.2 E_q, hundreds of times the fp16 error of these rows
    assert np.abs(x[0, at] - r64).max() < (0.5 if metric == "ip" else 1.0) * E / 1.02 * 0.8
    got, st = _gpu(_prepared_store(P, cuda_dev), N, D, Q, rad, metric, cuda_dev)
    _assert_equals_oracle(got, P, Q, rad, metric, x, need_margin=False)  # (the midpoint condition above replaces the margin)
    assert 1000 <= got[0][1] <= 1048 and np.isin(got[2], at).all()
    print("pairs decided exactly: %d" % st[0])
    assert st[2] == 2 and st[0] >= 2048


# ---- 4. exact ties and strictness ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_ties_at_the_radius_are_all_out_and_one_step_further_all_in(metric, cuda_dev):
    rng = np.random.default_rng(11)
    N, D = 65600, 24
    P = rng.integers(-3, 4, (N, D)).astype(np.float32)                  # small integers: exact in the fp16 plane and everywhere else
    P[40000:40020] = P[17]                                              # duplicates: all in or all out
    Q = rng.integers(-3, 4, (4, D)).astype(np.float32)
    x = ref.fixed_order_values(P, Q, metric)
    sp = _prepared_store(P, cuda_dev)
    for q in range(4):
        v = np.float32(x[q, 17])                                        # held by rows 17, 40000..40019 (and more)
        held = np.nonzero(x[q] == v)[0]
        assert held.size >= 21
        if metric == "l2" and v == 0:
            continue
        step = np.nextafter(v, np.float32(np.inf if metric == "l2" else -np.inf))
        (lims, Dv, I), st = _gpu(sp, N, D, Q[q:q + 1], v, metric, cuda_dev)
        (lims2, D2, I2), st2 = _gpu(sp, N, D, Q[q:q + 1], step, metric, cuda_dev)
        assert st[2] == 2 and st2[2] == 2
        assert not np.isin(held, I).any()
        assert np.isin(held, I2).all() and I2.size == I.size + held.size
        for rad, got in ((v, (lims, Dv, I)), (step, (lims2, D2, I2))):
            olims, oD, oI = ref.range_search(P, Q[q:q + 1], rad, metric, values=x[q:q + 1])
            assert np.array_equal(got[0], olims) and np.array_equal(got[2], oI) and np.array_equal(got[1], oD)       # D equal: exact


# ---- 5. ip, every product negative, ragged last tile ---------------------------------------------------------------------------
def test_ip_all_products_negative_ragged_last_tile(cuda_dev):
    """every real value v = -2 p.q is POSITIVE: a zero plane row behind N, or the clamped reload of the last tile, would beat
    them all.  N = 2^16 + 1: one real row in the last 256-row tile, 31 padding rows in its first wave tile, 7 waves of padding."""
    N, D = 65537, 64
    P = np.abs(ref.unit_rows(N, D, 13))
    Q = np.ascontiguousarray(-P[[5, 40000, N - 1]])
    x = ref.fixed_order_values(P, Q, "ip")
    assert (x < 0).all()
    sp = _prepared_store(P, cuda_dev)
    (lims, Dv, I), st = _gpu(sp, N, D, Q, -np.inf, "ip", cuda_dev)
    assert st[2] == 2
    assert lims.tolist() == [0, N, 2 * N, 3 * N]                        # every row once, no bit behind N
    assert np.array_equal(I, np.tile(np.arange(N, dtype=np.int64), 3)) and _ulp_close(Dv, x.astype(np.float32).reshape(-1))
    rad = ref.gap_radii(x, "ip", 20, 60)
    got, st = _gpu(sp, N, D, Q, rad, "ip", cuda_dev)
    _assert_equals_oracle(got, P, Q, rad, "ip", x)
    assert st[2] == 2 and got[2].max() < N


# ---- 6. edge radii, offsets, capacity ------------------------------------------------------------------------------------------
def test_edge_radii_offsets_and_capacity(cuda_dev):
    from adaptive_classifier import _native as nv
    from adaptive_classifier import index as ix
    N, D, nq = 65600, 48, 6
    P, Q = ref.unit_rows(N, D, 3), ref.unit_rows(nq, D, 4)
    sp = _prepared_store(P, cuda_dev)
    store, (planes, norms) = sp
    x = ref.fixed_order_values(P, Q, "l2")
    for r in (0.0, -1.0, np.nan):
        (lims, Dv, I), st = _gpu(sp, N, D, Q, r, "l2", cuda_dev)
        assert lims.tolist() == [0] * 7 and Dv.size == 0 and I.size == 0 and st == [0, 0, 2, 0]      # switched off: nothing decided
    (lims, Dv, I), st = _gpu(sp, N, D, Q, np.inf, "l2", cuda_dev, row_offset=10 ** 10)
    assert lims.tolist() == [N * i for i in range(7)] and st[2] == 2
    assert np.array_equal(I, np.tile(np.arange(N, dtype=np.int64) + 10 ** 10, 6))                   # every row, in id order
    assert _ulp_close(Dv, x.astype(np.float32).reshape(-1))
    xi = ref.fixed_order_values(P, Q, "ip")
    (lims, Dv, I), st = _gpu(sp, N, D, Q, -np.inf, "ip", cuda_dev)
    assert lims[-1] == 6 * N and _ulp_close(Dv, xi.astype(np.float32).reshape(-1)) and st[2] == 2
    for r in (np.inf, np.nan):
        got, st = _gpu(sp, N, D, Q, r, "ip", cuda_dev)
        assert got[0].tolist() == [0] * 7 and st == [0, 0, 2, 0]
    # per-query radii: dead queries between live ones
    base = ref.gap_radii(x, "l2", 100, 400)
    rad = np.array([np.inf, 0.0, base[2], np.nan, -3.0, base[5]], np.float32)
    got, st = _gpu(sp, N, D, Q, rad, "l2", cuda_dev)
    _assert_equals_oracle(got, P, Q, rad, "l2", x)
    assert np.diff(got[0])[[1, 3, 4]].tolist() == [0, 0, 0] and np.diff(got[0])[0] == N and np.diff(got[0])[2] > 100
    assert _bit_equal(got, _gpu(sp, N, D, Q, rad, "l2", cuda_dev, plane=False)[0])
    base = ref.gap_radii(xi, "ip", 100, 400)
    rad = np.array([-np.inf, np.inf, base[2], np.nan, base[4], base[5]], np.float32)
    got, st = _gpu(sp, N, D, Q, rad, "ip", cuda_dev)
    _assert_equals_oracle(got, P, Q, rad, "ip", xi)
    assert np.diff(got[0])[[1, 3]].tolist() == [0, 0] and np.diff(got[0])[0] == N
    # nq = 0: nothing is written
    (lims, Dv, I), _ = _gpu(sp, N, D, Q[:0], 1.0, "l2", cuda_dev)
    assert lims.tolist() == [0] and Dv.size == 0 and I.size == 0
    # capacity too small: the unchanged fill writes nothing and raises its flag; [2] stays as the count left it
    L = nv.lib()
    ws = torch.empty(ix.knn_range_batch_workspace_bytes(N, D, nq), dtype=torch.uint8, device=cuda_dev)
    Qd = torch.from_numpy(Q).to(cuda_dev)
    rd = torch.from_numpy(np.full(nq, 1.5, np.float32)).to(cuda_dev)
    lims_d = torch.empty(nq + 1, dtype=torch.int64, device=cuda_dev)
    stats = torch.zeros(4, dtype=torch.int32, device=cuda_dev)
    with torch.cuda.device(cuda_dev):
        nv.check(L.ac_knn_l2_range_count_batch(nv.ptr(store), N, store.stride(0), D, nv.ptr(planes), nv.ptr(norms), nv.ptr(Qd), nq,
                                               Qd.stride(0), nv.ptr(rd), nv.ptr(lims_d), nv.ptr(ws), ws.numel(), nv.ptr(stats),
                                               nv.stream_ptr(cuda_dev)), "count")
        total = int(lims_d[-1].item())
        assert total > 100 and stats[2].item() == 2
        for cap in (total - 1, total):
            outD = torch.full((total + 8,), -7.0, dtype=torch.float32, device=cuda_dev)
            outI = torch.full((total + 8,), -7, dtype=torch.int64, device=cuda_dev)
            nv.check(L.ac_knn_l2_range_fill(nv.ptr(store), N, store.stride(0), D, nv.ptr(Qd), nq, Qd.stride(0), 0, nv.ptr(lims_d), cap,
                                            nv.ptr(outD), None, nv.ptr(outI), nv.ptr(ws), ws.numel(), nv.ptr(stats), nv.stream_ptr(cuda_dev)), "fill")
            torch.cuda.synchronize()
            assert stats[2].item() == 2
            if cap < total:
                assert stats[1].item() == 1 and bool((outI == -7).all()) and bool((outD == -7.0).all())
            else:
                assert stats[1].item() == 0 and bool((outI[:total] >= 0).all()) and bool((outI[total:] == -7).all())
        # a workspace that only fits the fp32 route is refused, with the size
        small = ix.knn_range_workspace_bytes(N, D, nq)
        assert L.ac_knn_l2_range_count_batch(nv.ptr(store), N, store.stride(0), D, nv.ptr(planes), nv.ptr(norms), nv.ptr(Qd), nq,
                                             Qd.stride(0), nv.ptr(rd), nv.ptr(lims_d), nv.ptr(ws), small, nv.ptr(stats),
                                             nv.stream_ptr(cuda_dev)) == -3
        assert (b"required %d" % ws.numel()) in L.ac_last_error()


# ---- 7. filtered ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_filtered_plane_range_equals_the_fp32_route(metric, cuda_dev):
    N, D, nq = 66000, 72, 70
    P, Q, x, _ = bref.case(N, D, nq, metric)
    sp = _case_store(N, D, cuda_dev)
    E = bref.bound(P, Q)
    rng = np.random.default_rng(77)
    s = np.sort(x.astype(np.float32), axis=1)
    rad = np.ascontiguousarray(s[:, ::-1][:, 30] if metric == "ip" else s[:, 30])      # on a value: that pair is never certain
    plain, st_plain = _gpu(sp, N, D, Q, rad, metric, cuda_dev, exact_out=True)
    for density, bit0 in ((0.5, 0), (1.0 / 64, 0), (0.5, 37)):
        mask = rng.random(N) < density
        a, sa = _gpu(sp, N, D, Q, rad, metric, cuda_dev, mask=mask, bit0=bit0, exact_out=True)
        b, sb = _gpu(sp, N, D, Q, rad, metric, cuda_dev, plane=False, mask=mask, bit0=bit0, exact_out=True)
        assert sa[2] == 2 and sb[2] == 0 and _bit_equal(a, b), (density, bit0)
        assert mask[a[2]].all()
        cap = bref.undecided_cap(x, rad, E, metric, mask)
        print("density %.3f bit0 %d: decided exactly %d (unfiltered %d), cap over the selected pairs %d" % (density, bit0, sa[0], st_plain[0], cap))
        assert sa[0] <= cap and sa[0] <= st_plain[0]                    # selected pairs only
    # the rows AT a radius, and nothing else within the band, deselected: no selected pair is left to decide
    near = (np.abs(x - rad.astype(np.float64)[:, None]) <= (2.1 if metric == "l2" else 1.05) * E[:, None]).any(axis=0)
    a, sa = _gpu(sp, N, D, Q, rad, metric, cuda_dev, mask=~near, exact_out=True)
    assert sa[0] == 0 and sa[2] == 2 and st_plain[0] >= nq
    assert _bit_equal(a, _gpu(sp, N, D, Q, rad, metric, cuda_dev, plane=False, mask=~near, exact_out=True)[0])
    # an all-ones selection is the unfiltered plane call, d_stats included
    ones, st_ones = _gpu(sp, N, D, Q, rad, metric, cuda_dev, mask=np.ones(N, bool), exact_out=True)
    assert _bit_equal(ones, plain) and st_ones == st_plain


@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_row_shard_reads_its_slice_of_a_global_bitmap(metric, cuda_dev):
    """a shard of rows [lo, lo + n) of a larger store passes the GLOBAL bitmap with sel_bit0 = row_offset = lo"""
    from adaptive_classifier import index as ix
    N, D, nq = 70000, 64, 5
    P, Q, x, rad = bref.case(N, D, nq, metric)
    lo, n = 2087, 65600                                                 # (lo % 64 = 39: a wave tile's 32 bits straddle two words)
    gmask = np.random.default_rng(3).random(N) < 0.5
    store = _case_store(N, D, cuda_dev)[0]
    shard = store[lo: lo + n]
    prepared = ix.prepare_store(shard, n, D)
    words = _words(gmask, cuda_dev)
    Qd, rd = torch.tensor(Q, device=cuda_dev), torch.tensor(rad, device=cuda_dev)
    outs = []
    for prep in (prepared, None):
        stats = torch.zeros(4, dtype=torch.int32, device=cuda_dev)
        o = ix.knn_range_search(shard, n, D, Qd, rd, metric=metric, row_offset=lo, exact_out=True, sel=words, sel_bit0=lo, stats=stats,
                                prepared=prep)
        outs.append(tuple(t.cpu().numpy() for t in o))
        assert stats[2].item() == (2 if prep is not None else 0)
    assert _bit_equal(outs[0], outs[1])
    olims, oD, oI = sref.filtered_range_search(P[lo: lo + n], Q, rad, gmask[lo: lo + n], metric, row_offset=lo, values=x[:, lo: lo + n])
    assert np.array_equal(outs[0][0], olims) and np.array_equal(outs[0][2], oI) and _ulp_close(outs[0][1], oD)


# ---- 8. chunking ---------------------------------------------------------------------------------------------------------------
def test_result_does_not_depend_on_chunking(cuda_dev):
    from adaptive_classifier import index as ix
    N, D, nq = 66000, 72, 70
    P, Q, x, rad = bref.case(N, D, nq, "l2")
    sp = _case_store(N, D, cuda_dev)
    a, sa = _gpu(sp, N, D, Q, rad, "l2", cuda_dev, exact_out=True)
    budget = ix.knn_range_batch_workspace_bytes(N, D, 20)
    assert ix.range_query_chunk(N, D, nq, budget, ix.knn_range_batch_workspace_bytes) * 3 <= nq
    c, sc = _gpu(sp, N, D, Q, rad, "l2", cuda_dev, exact_out=True, max_ws_bytes=budget)               # >= 3 chunks
    assert sa[2] == 2 and sc[2] == 2 and _bit_equal(a, c)
    _assert_equals_oracle(c, P, Q, rad, "l2", x)


# ---- 9. index and memory level -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "ip"])
def test_flat_index_uses_a_plane_that_exists_and_never_prepares_one(metric, cuda_dev):
    from adaptive_classifier import index as ix
    N, D = (1 << 18) + 5, 32
    rows = ref.unit_rows(N + 300, D, 21)
    Q = ref.unit_rows(5, D, 22)
    rad = 1.0 if metric == "l2" else 0.6
    idx = (ix.HipFlatIPIndex if metric == "ip" else ix.HipFlatL2Index)(D, device=cuda_dev)
    idx.add(torch.from_numpy(rows[:N]).to(cuda_dev))

    def fresh(n):
        """the fp32 route over the index's current rows"""
        return tuple(t.cpu().numpy() for t in ix.knn_range_search(idx._store, n, D, torch.tensor(Q, device=cuda_dev), rad, metric=metric))

    a = idx.range_search(Q, rad)
    assert idx._prepared is None and idx.range_stats[2] == 0            # no plane: the fp32 route, and none was built
    assert 5 <= np.diff(a[0]).min() and _bit_equal(a, fresh(N))
    idx._prepared = ix.prepare_store(idx._store, idx._n, D, capacity=idx._store.shape[0])
    b = idx.range_search(Q, rad)
    assert idx.range_stats[2] == 2 and _bit_equal(a, b)                 # the same bits over the plane
    idx.add(torch.from_numpy(rows[N: N + 300]).to(cuda_dev))           # the plane follows incrementally
    assert idx._prepared is not None
    c = idx.range_search(Q, rad)
    assert idx.range_stats[2] == 2 and _bit_equal(c, fresh(N + 300)) and c[0][-1] >= b[0][-1]
    hit = int(c[2][0])
    idx.update_rows([hit, 7, N + 299], rows[[3, 4, 5]] * np.float32(0.5))
    assert idx._prepared is not None
    d = idx.range_search(Q, rad)
    assert idx.range_stats[2] == 2 and _bit_equal(d, fresh(N + 300)) and not _bit_equal(c, d)
    idx.remove_ids(np.array([0, 5, hit]))
    assert idx._prepared is None                                        # compaction drops the plane
    e = idx.range_search(Q, rad)
    assert idx._prepared is None and idx.range_stats[2] == 0 and _bit_equal(e, fresh(N + 297))


def test_prototypes_within_inherits_the_plane_route(cuda_dev):
    from adaptive_classifier import index as ix
    from adaptive_classifier.memory import PrototypeMemory
    N, D = (1 << 18) + 5, 32
    rows = ref.unit_rows(N, D, 21)
    ld = (D + 3) // 4 * 4
    store = torch.zeros((N, ld), dtype=torch.float32, device=cuda_dev)
    store[:, :D] = torch.from_numpy(rows).to(cuda_dev)
    mem = PrototypeMemory(D, device=cuda_dev)
    mem.load_rows(store, torch.from_numpy((np.arange(N) % 3).astype(np.int32)), ["x", "y", "z"])
    q = torch.from_numpy(ref.unit_rows(1, D, 22)[0])
    a = mem.prototypes_within(q, 1.0)
    assert mem.index._prepared is None and mem.index.range_stats[2] == 0 and len(a) >= 5
    mem.index._prepared = ix.prepare_store(mem.index._store, mem.index._n, D)
    b = mem.prototypes_within(q, 1.0)
    assert mem.index.range_stats[2] == 2 and a == b
