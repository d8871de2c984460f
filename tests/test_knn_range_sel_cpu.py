"""CPU suite of the FILTERED range search: the ABI additions (header <-> ctypes table, the id-list workspace, the argument checks
that return before any device work), the margins the GPU tests rely on, the host routing of range_search(sel=) with the device
calls replaced, and ShardedSearch.range_search over gloo with the oracle as the local search."""
import ctypes
import os
import re
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import knn_range_ref as ref  # noqa: E402
import knn_range_sel_ref as sref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["ac_knn_l2_range_count_sel", "ac_knn_ip_range_count_sel", "ac_knn_range_ids_workspace", "ac_knn_l2_range_count_ids",
       "ac_knn_l2_range_fill_ids", "ac_knn_ip_range_count_ids", "ac_knn_ip_range_fill_ids"]


# ---- oracle ----------------------------------------------------------------------------------------------------------------------
def test_filtered_oracle_maps_ids_back_and_pack_sets_the_tail():
    P = np.array([[0.0], [1.0], [1.0], [3.0], [-2.0]], dtype=np.float32)
    Q = np.array([[1.0]], dtype=np.float32)
    mask = np.array([True, False, True, True, True])
    lims, D, I, E = sref.filtered_range_search(P, Q, 4.5, mask, "l2", row_offset=10, return_exact=True)
    assert lims.tolist() == [0, 3] and I.tolist() == [10, 12, 13] and D.tolist() == [1.0, 0.0, 4.0] and E.tolist() == [1.0, 0.0, 4.0]
    assert sref.filtered_range_search(P, Q, 0.5, mask, "ip")[2].tolist() == [2, 3]
    assert sref.filtered_range_search(P, Q, 9.0, np.zeros(5, bool), "l2")[0].tolist() == [0, 0]
    w = sref.pack(mask, 0)
    assert w.dtype == np.uint64 and w.size == 1 and int(w[0]) == (2 ** 64 - 1) & ~0b00010
    w = sref.pack(np.zeros(70, bool), 37)                                      # rows = bits 37 .. 106: exactly 2 words
    assert w.size == 2 and int(w[0]) == (1 << 37) - 1 and int(w[1]) == (2 ** 64 - 1) & ~((1 << 43) - 1)
    assert sref.pack(np.zeros(0, bool), 0, tail_ones=False).tolist() == [0]


@pytest.mark.parametrize("N,D,nq", sref.CASES + [sref.IDS_ONLY_CASE])
def test_gap_radii_over_the_selected_rows_leave_a_wide_margin(N, D, nq):
    """what tests/test_knn_range_sel_gpu.py relies on (it asserts the margin before it compares ids): on its shapes, masks and
    seeds the gap radii of ranks 20..60 OF THE SELECTED ROWS admit 21..60 of them and keep every selected value >= 64 ulps away"""
    for metric in ("l2", "ip"):
        P, Q, mask, x, rad = sref.case(N, D, nq, metric, 0.15 if (N, D, nq) == sref.IDS_ONLY_CASE else 0.5)
        hits = np.diff(sref.filtered_range_search(P, Q, rad, mask, metric, values=x)[0])
        m = sref.margin(x, mask, rad)
        print(N, D, nq, metric, "selected %d, hits %d..%d, margin %.0f ulps" % (mask.sum(), hits.min(), hits.max(), m))
        assert hits.min() >= 21 and hits.max() <= 60 and m >= 64


# ---- ABI -------------------------------------------------------------------------------------------------------------------------
def test_header_and_ctypes_table_declare_the_new_symbols():
    from adaptive_classifier import _native as nv
    L = nv.lib()
    assert L.ac_version() >= 7
    src = open(os.path.join(ROOT, "include", "acamd.h")).read()
    assert "Not covered: filtered range search" not in src
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in NEW:
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, code)
        assert m, f"{name} is not declared in acamd.h"
        assert name in nv.exported_symbols() and hasattr(L, name)
        assert len(getattr(L, name).argtypes) == len(m.group(1).split(",")), name      # one ctypes entry per declared argument
    # (d_sel, sel_bit0) follow d_radius; (d_ids, M) follow D -- as in ac_knn_*_topk_sel / _ids
    assert re.search(r"ac_knn_l2_range_count_sel\([^)]*d_radius,\s*const uint64_t\*\s*d_sel,\s*int64_t sel_bit0,\s*int64_t\*\s*d_lims", code)
    assert re.search(r"ac_knn_ip_range_fill_ids\([^)]*int D,\s*const int64_t\*\s*d_ids,\s*int64_t M,\s*const float\*\s*d_Q", code)


def test_ids_workspace_does_not_depend_on_the_store():
    from adaptive_classifier import _native as nv
    from adaptive_classifier.index import knn_range_ids_workspace_bytes
    L = nv.lib()
    b = ctypes.c_size_t(0)
    up = lambda n: (n + 255) // 256 * 256
    for M in (0, 1, 64, 65, 4097, 8192):
        for nq in (0, 1, 16, 33, 1000):
            n = max(nq, 1) * max((M + 63) // 64, 1)                            # words: nq x ceil(M / 64), at least one
            assert L.ac_knn_range_ids_workspace(M, nq, ctypes.byref(b)) == 0
            assert b.value == up(8 * n) + up(4 * n) + up(8 * n), (M, nq)       # bitmap, strip counts, strip offsets
            assert knn_range_ids_workspace_bytes(M, nq) == b.value
    assert L.ac_knn_range_ids_workspace(8193, 4, ctypes.byref(b)) == -1 and b"M=8193" in L.ac_last_error()
    assert L.ac_knn_range_ids_workspace(-1, 4, ctypes.byref(b)) == -1
    assert L.ac_knn_range_ids_workspace(5, 4, None) == -1


def test_argument_checks_return_before_any_device_work():
    from adaptive_classifier import _native as nv
    L = nv.lib()
    buf = (ctypes.c_uint64 * 64)()
    a = ctypes.addressof(buf)
    p = ctypes.c_void_p
    N, D, nq = 5000, 768, 7
    need = ctypes.c_size_t(0)
    assert L.ac_knn_range_workspace(N, D, nq, ctypes.byref(need)) == 0
    for name in ("ac_knn_l2_range_count_sel", "ac_knn_ip_range_count_sel"):
        fn = getattr(L, name)
        call = lambda n_rows, d_sel, bit0, ws=need.value, q=nq: fn(p(a), n_rows, D, D, p(a), q, D, p(a), d_sel, bit0, p(a), p(a), ws, None, None)
        assert call(N, None, 0) == -1 and b"d_sel" in L.ac_last_error()                         # NULL d_sel with N > 0
        assert call(N, p(a + 4), 0) == -1 and b"d_sel" in L.ac_last_error() and b"aligned" in L.ac_last_error()
        assert call(N, p(a), -1) == -1 and b"sel_bit0" in L.ac_last_error()
        assert call(N, p(a), 0, ws=need.value - 1) == -3 and (b"required %d" % need.value) in L.ac_last_error()    # the unfiltered plan
        assert call(N, p(a), 0, q=0) == 0                                                       # no query: nothing to do
    ids_ws = ctypes.c_size_t(0)
    assert L.ac_knn_range_ids_workspace(8192, nq, ctypes.byref(ids_ws)) == 0
    for metric in ("l2", "ip"):
        cnt = getattr(L, f"ac_knn_{metric}_range_count_ids")
        fill = getattr(L, f"ac_knn_{metric}_range_fill_ids")
        count = lambda d_ids, M, q=nq: cnt(p(a), N, D, D, d_ids, M, p(a), q, D, p(a), p(a), p(a), ids_ws.value, None, None)
        fillc = lambda d_ids, M, q=nq: fill(p(a), N, D, D, d_ids, M, p(a), q, D, 0, p(a), 0, p(a), None, p(a), p(a), ids_ws.value, None, None)
        for call in (count, fillc):
            assert call(p(a), 8193) == -1 and b"M=8193" in L.ac_last_error()
            assert call(p(a), -1) == -1 and b"M=-1" in L.ac_last_error()
            assert call(None, 5) == -1 and b"d_ids" in L.ac_last_error()
            assert call(p(a), 8192, q=0) == 0


# ---- host routing ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls_name", ["HipFlatL2Index", "HipFlatIPIndex"])
def test_range_search_routes_by_what_the_host_knows(cls_name, monkeypatch):
    """<= KNN_IDS_MAX host ids -> the id-list route; a bitmap without host ids (what a device mask becomes) or more ids -> the
    bitmap route on the fp32 rows; no selector -> the unfiltered call.  The bitmap is never read back to choose."""
    from adaptive_classifier import index as ix
    idx = getattr(ix, cls_name)(8, device="cpu")
    n = 9000
    idx._store, idx._n = torch.zeros((n, 8)), n
    monkeypatch.setattr(ix._HipFlatIndex, "_materialize", lambda self: None)
    monkeypatch.setattr(ix.RowSelector, "count", lambda self: pytest.fail("the bitmap was read back"))
    calls = []
    empty = (torch.zeros(2, dtype=torch.int64), torch.zeros(0), torch.zeros(0, dtype=torch.int64))
    monkeypatch.setattr(ix, "knn_range_ids", lambda P, N, D, Q, r, ids, **kw: calls.append(("ids", N, ids, kw)) or empty)
    monkeypatch.setattr(ix, "knn_range_search", lambda P, N, D, Q, r, **kw: calls.append(("bitmap", N, kw.get("sel"), kw)) or empty)
    q = np.zeros((1, 8), np.float32)
    idx.range_search(q, 1.0, sel=[5, 3, 3, 8999, 9000, -1])                    # host ids: sorted, unique, clipped
    assert calls[-1][0] == "ids" and calls[-1][2].tolist() == [3, 5, 8999] and calls[-1][3]["metric"] == idx.metric
    idx.range_search(q, 1.0, sel=np.arange(8192))
    assert calls[-1][0] == "ids" and calls[-1][2].numel() == 8192
    idx.range_search(q, 1.0, sel=np.arange(8193))                              # one id too many for the list
    assert calls[-1][0] == "bitmap" and isinstance(calls[-1][2], ix.RowSelector) and calls[-1][2].n == n
    dev_like = ix.RowSelector(torch.zeros((n + 63) // 64, dtype=torch.int64), n)   # no host ids, no known count
    idx.range_search(q, 1.0, sel=dev_like)
    assert calls[-1][0] == "bitmap" and calls[-1][2] is dev_like and dev_like.known_count is None
    mask = np.zeros(n, bool); mask[::3] = True
    idx.range_search(q, 1.0, sel=mask)                                         # a mask carries no id list, however sparse
    assert calls[-1][0] == "bitmap" and calls[-1][2].ids is None
    idx.range_search(q, 1.0)
    assert calls[-1][0] == "bitmap" and calls[-1][2] is None
    with pytest.raises(ValueError):
        idx.range_search(q, 1.0, sel=np.zeros(n - 1, bool))                    # a selector of the wrong length
    with pytest.raises(ValueError):
        idx.range_search(q, 1.0, sel=ix.RowSelector(torch.zeros(8, dtype=torch.int64), 100))
    assert len(calls) == 6


def test_sharded_fixed_batch_path_has_no_range_search():
    from adaptive_classifier.sharded import ShardedSearch
    ss = ShardedSearch(torch.zeros(10, 8), 10, 8, 0, block_rows=4, local_search=lambda *a: a, merge=lambda *a: a,
                       local_range=lambda *a: pytest.fail("searched"))
    with pytest.raises(ValueError):
        ss.range_search(torch.zeros(2, 8), 1.0)


def test_one_rank_group_returns_the_local_result():
    from adaptive_classifier.sharded import ShardedSearch
    out = (torch.tensor([0, 1]), torch.tensor([0.5]), torch.tensor([7]), torch.tensor([0.5], dtype=torch.float64))
    seen = []
    ss = ShardedSearch(torch.zeros(10, 8), 10, 8, 3, local_search=lambda *a: a, merge=lambda *a: a,
                       local_range=lambda *a: seen.append(a) or out)
    lims, D, I = ss.range_search(torch.zeros(1, 8), 1.0, sel="S")
    assert lims is out[0] and D is out[1] and I is out[2]
    assert seen[0][1:3] == (10, 8) and seen[0][5:] == (3, "S", 3)              # row_offset = sel_bit0 = the shard's first row


# ---- ShardedSearch.range_search over gloo ----------------------------------------------------------------------------------------
D_SH = 12
# (shard sizes per rank, the rank whose rows are put where no query can hit them): uneven shards with an empty one; N = 3 at world 4
LAYOUTS = {2: [([9, 4], None), ([13, 0], None)], 4: [([7, 3, 0, 5], 1), ([1, 1, 1, 0], None)]}


def _store(sizes, far, metric):
    N = sum(sizes)
    P = ref.unit_rows(N, D_SH, 41).copy()
    Q = ref.unit_rows(4, D_SH, 42).copy()
    Q[3] = 50.0                                                                # query 3 gets a radius nothing satisfies
    if far is not None:                                                        # a non-empty shard without a hit
        lo = sum(sizes[:far])
        P[lo: lo + sizes[far]] *= 30.0 if metric == "l2" else 0.0
    x = ref.fixed_order_values(P, Q, metric)
    rad = (ref.gap_radii(x, metric, 2, 5) if N > 8 else np.full(4, 1.2 if metric == "l2" else 0.1, np.float32)).copy()
    rad[3] = 1.0 if metric == "l2" else 1e6
    gmask = np.random.default_rng(5).random(N) < 0.6
    return P, Q, x, rad, gmask


def _worker(rank, world, port, ret):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [root, os.path.join(root, "adaptive-classifier_amd"), os.path.join(root, "tests")]
    from adaptive_classifier.sharded import ShardedSearch
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    out = []
    for sizes, far in LAYOUTS[world]:
        lo = sum(sizes[:rank])
        for metric in ("l2", "ip"):
            P, Q, _, rad, gmask = _store(sizes, far, metric)

            def local_range(Pl, n, Dd, Qq, radius, off, sel, bit0, metric=metric, lo=lo, sizes=sizes):
                r = radius.numpy() if torch.is_tensor(radius) else radius
                assert off == lo and bit0 == lo and n == sizes[rank]
                if sel is None:
                    o = ref.range_search(Pl.numpy()[:n], Qq.numpy(), r, metric, row_offset=off, return_exact=True)
                else:                                                         # the replicated GLOBAL mask, read at sel_bit0
                    o = sref.filtered_range_search(Pl.numpy()[:n], Qq.numpy(), r, sel[bit0: bit0 + n], metric, row_offset=off,
                                                   return_exact=True)
                return tuple(torch.from_numpy(np.ascontiguousarray(t)) for t in o)

            ss = ShardedSearch(torch.from_numpy(P[lo: lo + sizes[rank]]), sizes[rank], D_SH, lo, metric=metric,
                               local_search=lambda *a: a, merge=lambda *a: a, local_range=local_range)
            for sel in (None, gmask):
                for r in (torch.from_numpy(rad), float(rad[0])):
                    out.append(tuple(t.numpy() for t in ss.range_search(torch.from_numpy(Q), r, sel=sel)))
    ret[rank] = out
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 4])
def test_sharded_range_search_equals_the_oracle_on_the_whole_store(world):
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ret = mp.Manager().dict()
    mp.spawn(_worker, args=(world, port, ret), nprocs=world, join=True)
    at = 0
    for sizes, far in LAYOUTS[world]:
        N, bounds = sum(sizes), np.cumsum([0] + sizes)
        for metric in ("l2", "ip"):
            P, Q, x, rad, gmask = _store(sizes, far, metric)
            for sel in (None, gmask):
                for r in (rad, float(rad[0])):
                    olims, oD, oI = sref.filtered_range_search(P, Q, r, np.ones(N, bool) if sel is None else sel, metric, values=x)
                    per_rank = [int(((oI >= bounds[g]) & (oI < bounds[g + 1])).sum()) for g in range(world)]
                    if N > 8 and sel is None and np.ndim(r):                   # the cases are what they claim to be:
                        hits = np.diff(olims)
                        assert hits[3] == 0 and hits[:3].min() >= 3            # a query without a hit anywhere; the others have some
                        assert sum(1 for c in per_rank if c) >= (2 if min(sizes[0], sizes[1]) else 1)       # hits from several ranks
                        assert far is None or (sizes[far] > 0 and per_rank[far] == 0)                      # a non-empty rank with none
                    for rank in range(world):
                        lims, Dv, I = ret[rank][at]
                        assert lims.dtype == np.int64 and I.dtype == np.int64 and Dv.dtype == np.float32
                        assert np.array_equal(lims, olims), (sizes, metric, rank, lims, olims)
                        assert np.array_equal(I, oI) and np.array_equal(Dv, oD)      # the oracle's arithmetic on both sides: equal bits
                    at += 1
