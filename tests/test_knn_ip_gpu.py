"""Parity of the inner-product search (ac_knn_ip_topk through the C ABI, HipFlatIPIndex, the sharded merge) against the
fp64 oracle tests/knn_ip_ref.py.

Bar: identical top-k ids for EVERY query; values are the exact inner product rounded to fp32 (tolerance: 1 ulp, because the
fp64 summation order differs from the oracle's -- the L2 tests' own bar, test_knn_gpu.py).
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import knn_ip_ref  # noqa: E402

pytestmark = pytest.mark.gpu

FLT_MAX = np.finfo(np.float32).max
SHORTLIST_FROM = 1_000_000          # rows x queries from which the oracle shortlists with BLAS (and the test asserts the margin)


def _ulp_close(a, b):
    a = np.asarray(a, np.float32)
    b = np.asarray(b, np.float32)
    with np.errstate(over="ignore"):                      # (padding: the spacing of FLT_MAX is inf; equal padding passes)
        return np.all(np.abs(a - b) <= np.spacing(np.maximum(np.abs(a), np.abs(b)).astype(np.float32)))


def _oracle(P, Q, k, row_offset=0):
    if P.shape[0] * Q.shape[0] >= SHORTLIST_FROM and P.shape[0] > k + 64:
        oD, oI, gap, bound = knn_ip_ref.knn_ip_topk_shortlisted(P, Q, k, row_offset)
        print("shortlist margin: min gap %.3e, max bound %.3e" % (gap.min(), bound.max()))
        assert np.all(gap > bound), "the oracle's shortlist cut-off is too close to the k-th value"
        return oD, oI
    return knn_ip_ref.knn_ip_topk(P, Q, k, row_offset)


def _store(P, cuda_dev, ld=None):
    ld = ld or (P.shape[1] + 3) // 4 * 4
    store = torch.zeros((max(P.shape[0], 1), ld), dtype=torch.float32, device=cuda_dev)
    if P.shape[0]:
        store[: P.shape[0], : P.shape[1]] = torch.from_numpy(P).to(cuda_dev)
    return store


def _check(P, Q, k, cuda_dev, row_offset=0, ld=None):
    """search through the C ABI, compare EVERY query with the oracle; returns d_stats as a list"""
    from adaptive_classifier import index as ix
    store = _store(P, cuda_dev, ld)
    Qd = torch.from_numpy(Q).to(cuda_dev)
    stats = torch.zeros(4, dtype=torch.int32, device=cuda_dev)
    ex = torch.empty((Q.shape[0], k), dtype=torch.float64, device=cuda_dev)
    D, I = ix.knn_ip_topk(store, P.shape[0], P.shape[1], Qd, k, row_offset=row_offset, stats=stats, exact_out=ex)
    torch.cuda.synchronize()
    oD, oI = _oracle(P, Q, k, row_offset)
    I, D, ex = I.cpu().numpy(), D.cpu().numpy(), ex.cpu().numpy()
    assert np.array_equal(I, oI), f"id mismatch: {(I != oI).sum()} of {I.size}"
    assert _ulp_close(D, oD)
    assert np.array_equal(D[I < 0], oD[oI < 0]) and np.all(ex[I < 0] == -np.inf)      # padding: (-FLT_MAX, -1), -inf in fp64
    assert np.array_equal(ex[I >= 0].astype(np.float32), D[I >= 0])                    # d_outD is d_outD64 rounded once
    assert np.all(ex[:, :-1] >= ex[:, 1:])                                            # descending
    return stats.tolist()


@pytest.mark.parametrize("N,D,nq,k", [
    (4, 768, 1, 4),
    (100, 768, 8, 5),
    (77, 768, 3, 77),        # k = N: the whole (descending) order incl. the negative products
    (1000, 128, 16, 16),     # nq <= 16, D % 32 == 0: the LDS-ring sweep (asserted below)
    (5000, 768, 33, 16),     # 2 query tiles, ragged -> knn_sweep<2>
    (4097, 1024, 17, 32),    # TQ = 16 variant by LDS budget
    (3000, 384, 64, 1),
    (2500, 100, 5, 10),      # D % 8 != 0 (tail group)
    (999, 770, 7, 9),        # D % 4 != 0 (zero padded ld)
    (20000, 768, 256, 16),
    (300, 64, 40, 200),      # large k -> cap 512
    (300, 64, 40, 300),      # k > 248: small-store exact path
    (1000, 768, 5, 1000),    # k = N, full ordering of 1000 rows
    (500, 4096, 3, 10),      # D too wide for the LDS query tile: small-store exact path
    (10, 768, 2, 300),       # small-store path with k > N (padding)
])
def test_knn_ip_matches_oracle(N, D, nq, k, cuda_dev):
    from oracle import synth
    P = synth.synth_unit_rows(N, D, seed=1)
    Q = synth.synth_unit_rows(nq, D, seed=2)
    st = _check(P, Q, k, cuda_dev)
    if (N, D, nq, k) == (1000, 128, 16, 16):
        assert st[1] == 1                                   # the rows went through knn_sweep_ring
    if (N, D, nq, k) == (5000, 768, 33, 16):
        assert st[1] == 0


@pytest.mark.parametrize("N,D,nq,k", [(70_001, 768, 1, 16), (30_000, 544, 3, 5), (20_000, 1024, 4, 8)])
def test_knn_ip_ring_sweep_matches_oracle(N, D, nq, k, cuda_dev):
    """the three fragment placements of knn_sweep_ring (registers only / one chunk in LDS / the 32-chunk form), ragged last tile"""
    from oracle import synth
    st = _check(synth.synth_unit_rows(N, D, seed=5), synth.synth_unit_rows(nq, D, seed=6), k, cuda_dev)
    assert st[1] == 1 and st[0] == 0


def test_knn_ip_padded_ld(cuda_dev):
    from oracle import synth
    _check(synth.synth_unit_rows(3000, 100, seed=3), synth.synth_unit_rows(9, 100, seed=4), 7, cuda_dev, ld=128)


def test_knn_ip_row_offset_and_unnormalised(cuda_dev):
    rng = np.random.default_rng(0)
    P = (rng.standard_normal((3000, 768)) * 3).astype(np.float32)
    Q = (rng.standard_normal((9, 768)) * 0.5).astype(np.float32)
    _check(P, Q, 8, cuda_dev, row_offset=10_000_000_000)


def test_knn_ip_mixed_norms_differs_from_l2(cuda_dev):
    """Row norms over four decades: the inner product prefers long rows, L2 short ones -- the two rankings differ, so this
    test cannot pass on an L2 result."""
    from adaptive_classifier import index as ix
    from oracle import synth
    rng = np.random.default_rng(1)
    N, D, k = 6000, 256, 12
    P = (synth.synth_unit_rows(N, D, seed=3) * (10.0 ** rng.uniform(-2, 2, size=(N, 1)))).astype(np.float32)
    Q = synth.synth_unit_rows(10, D, seed=4)
    _check(P, Q, k, cuda_dev)
    store, Qd = _store(P, cuda_dev), torch.from_numpy(Q).to(cuda_dev)
    _, I_ip = ix.knn_ip_topk(store, N, D, Qd, k)
    _, I_l2 = ix.knn_l2_topk(store, N, D, Qd, k)
    assert all(set(a) != set(b) for a, b in zip(I_ip.cpu().tolist(), I_l2.cpu().tolist()))


def test_knn_ip_duplicates_and_ties(cuda_dev):
    """Exact duplicates straddling the k boundary (every row 40 times): lowest ids first; the certificate cannot separate
    exact ties, so every such query takes the exact fallback."""
    from oracle import synth
    base = synth.synth_unit_rows(50, 768, seed=5)
    P = np.concatenate([base] * 40, axis=0)
    Q = base[:6].copy()
    st = _check(P, Q, 16, cuda_dev)
    assert st[0] == 6


def test_knn_ip_many_fallbacks_slots_and_direct(cuda_dev):
    """more flagged queries (100) than fallback slots (64): the slab-parallel and the single-block fallback both rank by IP"""
    from oracle import synth
    base = synth.synth_unit_rows(100, 256, seed=11)
    P = np.concatenate([base] * 30, axis=0)
    st = _check(P, base[:100].copy(), 16, cuda_dev)
    assert st[0] == 100


def test_knn_ip_empty_index(cuda_dev):
    from adaptive_classifier import index as ix
    Q = torch.ones((2, 768), dtype=torch.float32, device=cuda_dev)
    st = _check(np.zeros((0, 768), np.float32), np.ones((2, 768), np.float32), 4, cuda_dev)
    assert st[0] == 0
    D, I = ix.knn_ip_topk(torch.zeros((1, 768), device=cuda_dev), 0, 768, Q, 4)
    assert (I == -1).all() and (D == -FLT_MAX).all()


def test_knn_ip_adversarial_order(cuda_dev):
    """rows sorted so that every later tile beats all earlier ones: every row is pushed, lists overflow and are pruned every tile"""
    from oracle import synth
    P = synth.synth_unit_rows(6000, 768, seed=7)
    q = synth.synth_unit_rows(1, 768, seed=8)
    P = P[np.argsort((P.astype(np.float64) @ q[0].astype(np.float64)))]           # best rows last
    Q = np.repeat(q, 20, axis=0) + synth.synth_unit_rows(20, 768, seed=9) * 1e-3
    _check(P, Q.astype(np.float32), 32, cuda_dev)


def test_knn_ip_baseline_config1_all_queries(cuda_dev):
    """BASELINE configs[1]: 100 000 x 768, 256 queries, k = 16 -- all 256 queries against the oracle."""
    from adaptive_classifier import index as ix
    N, D, nq, k = 100_000, 768, 256, 16
    P = ix.synth_unit_rows(N, D, 1, device=cuda_dev)
    Q = ix.synth_unit_rows(nq, D, 2, device=cuda_dev)
    stats = torch.zeros(4, dtype=torch.int32, device=cuda_dev)
    Dd, Id = ix.knn_ip_topk(P, N, D, Q, k, stats=stats)
    oD, oI = _oracle(P.cpu().numpy(), Q.cpu().numpy(), k)
    assert oI.shape == (nq, k) and np.array_equal(Id.cpu().numpy(), oI)
    assert _ulp_close(Dd.cpu().numpy(), oD)
    print("exact fallbacks at configs[1]:", int(stats[0].item()))


def test_ip_index_protocol_against_oracle(cuda_dev):
    from adaptive_classifier import index as ix
    from adaptive_classifier.index import HipFlatIPIndex
    from oracle import synth
    D = 96
    X = (synth.synth_unit_rows(400, D, 21) * np.linspace(0.5, 4.0, 400, dtype=np.float32)[:, None]).astype(np.float32)
    Q = synth.synth_unit_rows(7, D, 22)
    idx = HipFlatIPIndex(D, device=cuda_dev)
    ref = np.zeros((0, D), np.float32)
    for blk in (X[:100], X[100:250]):
        idx.add(blk)
        ref = np.concatenate([ref, blk])
    d, i = idx.search(Q, 12)
    oD, oI = knn_ip_ref.knn_ip_topk(ref, Q, 12)
    assert np.array_equal(i, oI) and _ulp_close(d, oD) and idx.exact_fallbacks == 0
    ids = np.array([0, 17, 17, 248, 400, -3, 100])                       # duplicates / out of range ignored, rows compact
    assert idx.remove_ids(ids) == 4 and idx.ntotal == 246
    ref = np.delete(ref, [0, 17, 100, 248], axis=0)
    idx.update_rows(torch.tensor([3, 200]), X[300:302])                  # in place: ids keep their meaning
    ref[[3, 200]] = X[300:302]
    idx.add(torch.from_numpy(X[250:300]).to(cuda_dev))                   # device rows appended after the compaction
    ref = np.concatenate([ref, X[250:300]])
    assert idx.ntotal == ref.shape[0] == 296 and idx._prepared is None
    d, i = idx.search(Q, 12)
    oD, oI = knn_ip_ref.knn_ip_topk(ref, Q, 12)
    assert np.array_equal(i, oI) and _ulp_close(d, oD)
    dd, ii = idx.search_device(torch.from_numpy(Q), 12)
    assert np.array_equal(ii.cpu().numpy(), oI)
    assert np.array_equal(idx._store[: idx.ntotal, :D].cpu().numpy(), ref)
    idx.reset()
    d, i = idx.search(Q[:1], 3)
    assert i.tolist() == [[-1, -1, -1]] and d.tolist() == [[-FLT_MAX] * 3]
    big = HipFlatIPIndex(768)
    big.add_device_rows(ix.synth_unit_rows(300_000, 768, 1, device=cuda_dev))
    for _ in range(2):                                                   # an L2 index would prepare its plane at the second search
        big.search_device(torch.from_numpy(synth.synth_unit_rows(4, 768, 2)), 8)
    assert big._prepared is None and big.ntotal == 300_000


@pytest.mark.parametrize("G", [2, 4, 8])
def test_ip_logical_shards_equal_unsharded_1M(G, cuda_dev):
    from adaptive_classifier import index as ix
    from adaptive_classifier.sharded import ShardedSearch, shard_bounds
    N, D, nq, k = 1_000_000, 768, 96, 32
    P = ix.synth_unit_rows(N, D, 1, device=cuda_dev)
    Q = ix.synth_unit_rows(nq, D, 2, device=cuda_dev)
    uD, uI = ix.knn_ip_topk(P, N, D, Q, k)
    parts = []
    for g in range(G):
        lo, hi = shard_bounds(N, G, g)
        ss = ShardedSearch(P[lo:hi], hi - lo, D, lo, metric="ip")       # world 1: the wired local search of the metric
        parts.append(ss._search(ss.rows, ss.n_local, D, Q, k, lo))
        if g == 0:
            assert ss._merge is ix.topk_merge_ip
            sD, sI = ss.search(Q[:8], k)
            eD, eI = ix.knn_ip_topk(P[lo:hi], hi - lo, D, Q[:8], k, row_offset=lo)
            assert torch.equal(sI, eI) and torch.equal(sD, eD)
    mD, mI = ix.topk_merge_ip(torch.stack([p[0] for p in parts]), torch.stack([p[1] for p in parts]))
    assert torch.equal(mI, uI) and torch.equal(mD, uD)


def test_ip_shard_merge_against_oracle(cuda_dev):
    from adaptive_classifier import index as ix
    rng = np.random.default_rng(3)
    S, nq, k = 8, 13, 32
    Din = -np.sort(-rng.standard_normal((S, nq, k)), axis=2)               # descending, negative values included
    Iin = rng.permutation(S * nq * k).reshape(S, nq, k).astype(np.int64)
    Din[2, :, 20:] = -np.inf
    Iin[2, :, 20:] = -1
    Din[3, 0, 0] = Din[4, 0, 0]                                            # a tie across shards
    D, I = ix.topk_merge_ip(torch.from_numpy(Din).to(cuda_dev), torch.from_numpy(Iin).to(cuda_dev))
    oD, oI = knn_ip_ref.topk_merge_ip(Din, Iin, k)
    assert np.array_equal(I.cpu().numpy(), oI) and np.array_equal(D.cpu().numpy(), oD)
    D, I = ix.topk_merge_ip(torch.from_numpy(Din[2:3, :, 10:]).to(cuda_dev), torch.from_numpy(Iin[2:3, :, 10:]).to(cuda_dev))
    assert (I[:, 10:] == -1).all() and (D[:, 10:] == -FLT_MAX).all()      # fewer real entries than k: (-FLT_MAX, -1)


@pytest.mark.parametrize("N,D,nq,k", [(50_000, 768, 16, 16), (20_000, 770, 33, 8), (300, 64, 4, 300)])
def test_l2_search_unchanged_around_an_ip_search_on_one_workspace(N, D, nq, k, cuda_dev):
    from adaptive_classifier import index as ix
    P = ix.synth_unit_rows(N, D, 1, device=cuda_dev)
    Q = ix.synth_unit_rows(nq, D, 2, device=cuda_dev)
    ws = torch.empty(max(ix.knn_workspace_bytes(N, D, nq, k), 256), dtype=torch.uint8, device=cuda_dev)
    st = torch.zeros(4, dtype=torch.int32, device=cuda_dev)
    e0 = torch.empty((nq, k), dtype=torch.float64, device=cuda_dev)
    e1 = torch.empty_like(e0)
    D0, I0 = ix.knn_l2_topk(P, N, D, Q, k, workspace=ws, stats=st, exact_out=e0)
    s0 = st.clone()
    Dp, Ip = ix.knn_ip_topk(P, N, D, Q, k, workspace=ws, stats=st)
    D1, I1 = ix.knn_l2_topk(P, N, D, Q, k, workspace=ws, stats=st, exact_out=e1)
    torch.cuda.synchronize()
    assert torch.equal(I0, I1) and torch.equal(D0.view(torch.int32), D1.view(torch.int32))
    assert torch.equal(e0.view(torch.int64), e1.view(torch.int64)) and torch.equal(s0, st)
    assert bool((Dp[Ip >= 0] <= 1.0001).all()) and not torch.equal(Dp, D0)      # (the call in between did rank by inner product)
