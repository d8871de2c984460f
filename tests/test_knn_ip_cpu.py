"""CPU suite of the inner-product search (ac_knn_ip_topk / HipFlatIPIndex / ShardedSearch(metric="ip")): the host-only parts
of the C ABI, the index's host bookkeeping, the sharded orchestration over gloo with the oracle injected, and the oracle
(tests/knn_ip_ref.py) itself on hand-made cases."""
import ctypes
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import knn_ip_ref  # noqa: E402

FLT_MAX = np.finfo(np.float32).max


# ------------------------------------------------------------------------------------------------ C ABI, host side
def test_ip_workspace_planner_and_validation_without_gpu():
    from adaptive_classifier import _native as nv
    L = nv.lib()
    b, b2 = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert L.ac_knn_ip_topk_workspace(10_000_000, 768, 4096, 32, ctypes.byref(b)) == 0 and b.value > 0
    assert L.ac_knn_l2_topk_workspace(10_000_000, 768, 4096, 32, ctypes.byref(b2)) == 0 and b2.value == b.value   # one plan
    assert L.ac_knn_ip_topk_workspace(100, 768, 8, 4, ctypes.byref(b)) == 0
    assert L.ac_knn_ip_topk_workspace(100, 768, 8, 1000, ctypes.byref(b)) == 0           # small store: exact path, any k
    assert L.ac_knn_ip_topk_workspace(100, 4096, 8, 8, ctypes.byref(b)) == 0              # ... and any D
    assert L.ac_knn_ip_topk_workspace(100000, 768, 8, 1000, ctypes.byref(b)) == -2        # big store + k beyond the sweep
    assert b"k=1000" in L.ac_last_error()
    assert L.ac_knn_ip_topk_workspace(100000, 4096, 8, 8, ctypes.byref(b)) == -2          # big store + D too wide for LDS
    assert L.ac_knn_ip_topk_workspace(100, 768, 8, 0, ctypes.byref(b)) == -1              # k < 1
    assert L.ac_knn_ip_topk_workspace(100, 768, 8, 4, None) == -1                         # NULL result pointer


def test_abi_version_grew_with_the_ip_entry_points():
    from adaptive_classifier import _native as nv
    L = nv.lib()
    assert L.ac_version() >= 2
    for name in ("ac_knn_ip_topk_workspace", "ac_knn_ip_topk", "ac_knn_ip_topk_x", "ac_topk_merge_ip_f64"):
        assert hasattr(L, name) and name in nv.exported_symbols()


# ------------------------------------------------------------------------------------------------ index, host side
def test_ip_index_host_bookkeeping_and_loud_search():
    from adaptive_classifier import _native as nv
    from adaptive_classifier.index import HipFlatIPIndex, HipFlatL2Index
    idx = HipFlatIPIndex(8)
    assert idx.metric == "ip" and HipFlatL2Index(8).metric == "l2" and idx.ntotal == 0
    idx.add(torch.arange(24, dtype=torch.float32).reshape(3, 8))
    idx.add(np.ones((2, 8), np.float32))
    assert idx.ntotal == 5                                    # queued on the host: no GPU needed
    assert idx._prepared is None
    idx.reset()
    assert idx.ntotal == 0
    idx.add(torch.zeros(4, 8))
    assert idx.ntotal == 4
    if torch.cuda.is_available():
        d, i = idx.search(np.ones((1, 8), np.float32), 2)
        assert i.tolist() == [[0, 1]] and d.tolist() == [[0.0, 0.0]]
        assert idx.remove_ids(np.array([1, 1, 9])) == 1 and idx.ntotal == 3
    else:
        with pytest.raises(nv.NativeError):
            idx.search(np.ones((1, 8), np.float32), 2)        # no CPU search path exists
        with pytest.raises(nv.NativeError):
            idx.remove_ids(np.array([1]))                     # compaction happens on the device
        assert idx.remove_ids(np.array([17, -2])) == 0 and idx.ntotal == 4     # out-of-range ids: nothing to do, no device needed


def test_sharded_search_rejects_unknown_metric():
    from adaptive_classifier.sharded import ShardedSearch
    with pytest.raises(ValueError):
        ShardedSearch(torch.zeros((0, 8)), 0, 8, 0, metric="bogus")
    inj = dict(local_search=lambda *a: None, merge=lambda *a: None)
    assert ShardedSearch(torch.zeros((0, 8)), 0, 8, 0, metric="ip", **inj).metric == "ip"
    assert ShardedSearch(torch.zeros((0, 8)), 0, 8, 0, **inj).metric == "l2"


# ------------------------------------------------------------------------------------------------ sharded orchestration (gloo)
def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _rows(n, D, seed, lo=0):
    """unnormalised rows with negative products; row i depends on (seed, lo + i) only, so shards regenerate their slice"""
    out = np.empty((n, D), np.float32)
    for i in range(n):
        out[i] = np.random.default_rng([seed, lo + i]).standard_normal(D).astype(np.float32) * (1.0 + ((lo + i) % 5))
    return out


def _worker(rank, world, port, N, D, sizes, k, ret):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [root, os.path.join(root, "adaptive-classifier_amd"), os.path.join(root, "tests")]
    import knn_ip_ref as ref
    from adaptive_classifier.sharded import ShardedSearch, shard_bounds
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    lo, hi = shard_bounds(N, world, rank)
    rows = torch.from_numpy(_rows(hi - lo, D, 1, lo))
    q0 = sum(sizes[:rank])
    q_local = torch.from_numpy(_rows(sizes[rank], D, 2, q0))

    def local_search(P, n, Dd, Q, kk, off):
        d, i = ref.knn_ip_topk(P.numpy()[:n], Q.numpy(), kk, row_offset=off, return_exact=True)      # fp64 on the wire
        return torch.from_numpy(d), torch.from_numpy(i)

    def merge(Ds, Is):
        d, i = ref.topk_merge_ip(Ds.numpy(), Is.numpy(), Ds.shape[2])
        return torch.from_numpy(d), torch.from_numpy(i)

    ss = ShardedSearch(rows, hi - lo, D, lo, local_search=local_search, merge=merge, metric="ip")
    Q = ss.gather_queries(q_local)
    Dg, Ig = ss.search(Q, k)
    Db, Ib = ss.search_block(q_local, k)
    Db2, Ib2 = ss.search_block(q_local, k, block_sizes=sizes)
    ret[rank] = (Q.numpy(), Dg.numpy(), Ig.numpy(), Db.numpy(), Ib.numpy(), Db2.numpy(), Ib2.numpy())
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world,N,k,sizes", [
    (2, 1001, 8, [3, 3]),
    (2, 37, 16, [2, 5]),                        # uneven query blocks; k close to the shard size
    (4, 1003, 8, [3, 1, 0, 2]),                 # uneven row shards (251, 251, 251, 250), an empty query block
    (4, 3, 4, [1, 1, 1, 1]),                    # an EMPTY row shard (3 rows over 4 ranks) and k > N: padding through the merge
])
def test_sharded_ip_search_equals_unsharded_oracle(world, N, k, sizes):
    D = 48
    mgr = mp.Manager()
    ret = mgr.dict()
    mp.spawn(_worker, args=(world, _free_port(), N, D, sizes, k, ret), nprocs=world, join=True)
    P, Q = _rows(N, D, 1), _rows(sum(sizes), D, 2)
    oD, oI = knn_ip_ref.knn_ip_topk(P, Q, k)
    for r in range(world):
        Qr, Dg, Ig, Db, Ib, Db2, Ib2 = ret[r]
        lo = sum(sizes[:r])
        assert np.array_equal(Qr, Q)
        assert np.array_equal(Ig, oI) and np.array_equal(Dg, oD)
        assert Ib.shape == (sizes[r], k)
        assert np.array_equal(Ib, oI[lo:lo + sizes[r]]) and np.array_equal(Db, oD[lo:lo + sizes[r]])
        assert np.array_equal(Ib2, Ib) and np.array_equal(Db2, Db)


# ------------------------------------------------------------------------------------------------ the oracle itself
def test_oracle_hand_made_cases():
    P = np.array([[1, 0], [0, 1], [-1, 0], [2, 2], [1, 0], [0, -3]], np.float32)
    Q = np.array([[1, 0], [-1, -1]], np.float32)
    D, I = knn_ip_ref.knn_ip_topk(P, Q, 4)
    #   q0 = (1, 0):   products 1, 0, -1, 2, 1, 0  -> 3 (2), then the duplicates 0 and 4 (1, lower id first), then 1 (0; id 1 < id 5)
    assert I[0].tolist() == [3, 0, 4, 1] and D[0].tolist() == [2.0, 1.0, 1.0, 0.0]
    #   q1 = (-1,-1):  products -1, -1, 1, -4, -1, 3 -> 5 (3), 2 (1), then the tie at -1: ids 0, 1 (4 is cut)
    assert I[1].tolist() == [5, 2, 0, 1] and D[1].tolist() == [3.0, 1.0, -1.0, -1.0]
    # k > N: (-FLT_MAX, -1) padding, -inf in the exact output; row_offset shifts real ids only
    D, I = knn_ip_ref.knn_ip_topk(P[:2], Q[:1], 4, row_offset=100)
    assert I[0].tolist() == [100, 101, -1, -1] and D[0].tolist() == [1.0, 0.0, -FLT_MAX, -FLT_MAX]
    E, I = knn_ip_ref.knn_ip_topk(P[:2], Q[:1], 3, return_exact=True)
    assert E.dtype == np.float64 and E[0].tolist() == [1.0, 0.0, -np.inf]
    D, I = knn_ip_ref.knn_ip_topk(np.zeros((0, 2), np.float32), Q, 2)
    assert (I == -1).all() and (D == -FLT_MAX).all()


def test_oracle_fixed_order_and_shortlist_agree():
    rng = np.random.default_rng(0)
    P = (rng.standard_normal((3000, 40)) * 3).astype(np.float32)
    P[1500:] = P[:1500]                                         # every row twice: identical rows must give identical values
    Q = rng.standard_normal((5, 40)).astype(np.float32)
    v = knn_ip_ref.fixed_order_ip(P.astype(np.float64), Q.astype(np.float64))
    assert np.array_equal(v[:, :1500], v[:, 1500:])
    ref = np.array([[sum(float(a) * float(b) for a, b in zip(P[n], Q[q])) for n in range(3)] for q in range(5)])
    assert np.array_equal(v[:, :3], ref)                        # literally the left-to-right sum of the exact products
    D, I = knn_ip_ref.knn_ip_topk(P, Q, 6)
    assert all(I[q, 2 * j + 1] == I[q, 2 * j] + 1500 for q in range(5) for j in range(3))      # duplicates: lower id first
    Ds, Is, gap, bound = knn_ip_ref.knn_ip_topk_shortlisted(P, Q, 6)
    assert np.all(gap > bound)
    assert np.array_equal(Is, I) and np.array_equal(Ds, D)


def test_oracle_merge_descending_with_padding_and_ties():
    Din = np.array([[[5.0, 1.0, -np.inf]], [[5.0, -2.0, -7.0]]])
    Iin = np.array([[[9, 4, -1]], [[3, 8, 2]]])
    D, I = knn_ip_ref.topk_merge_ip(Din, Iin, 3)
    assert I.tolist() == [[3, 9, 4]] and D.tolist() == [[5.0, 5.0, 1.0]]
    D, I = knn_ip_ref.topk_merge_ip(Din[:1], Iin[:1], 3)
    assert I.tolist() == [[9, 4, -1]] and D[0, 2] == -FLT_MAX
