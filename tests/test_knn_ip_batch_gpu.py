"""Inner-product search over a PREPARED store -- ac_knn_prepare_store + ac_knn_ip_topk_batch: the GEMM-form fp16 proposal sweep
(knn_batch_sweep<.., IP>, >= 64 queries) and the bandwidth-bound fp16-plane sweep (knn_plane_sweep<.., IP>, 1 .. 63 queries) --
against the fp64 oracle tests/knn_ip_ref.py and, bit for bit (ids, fp32 values, fp64 values), against the fp32-sweep route
(`knn_ip_topk` without `prepared`).  The proposal arithmetic differs (one fp16 product, no |p|^2 term), the answer may not.

Fallback cap: a test in which every query reaches the exact fallback hides a broken sweep, so on the uniform stores at most 2
queries per case may fall back (the L2 tests' own cap); the stress stores say where they assert a cap.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import knn_ip_ref  # noqa: E402
from helpers import near_tie_store  # noqa: E402

pytestmark = pytest.mark.gpu

SHORTLIST_FROM = 1_000_000          # rows x queries from which the oracle shortlists with BLAS (and the test asserts the margin)


def _ulp_close(a, b):
    a = np.asarray(a, np.float32)
    b = np.asarray(b, np.float32)
    with np.errstate(over="ignore"):
        return np.all(np.abs(a - b) <= np.spacing(np.maximum(np.abs(a), np.abs(b)).astype(np.float32)))


def _oracle(P, Q, k, row_offset=0, shortlist=None):
    if shortlist is None:
        shortlist = P.shape[0] * Q.shape[0] >= SHORTLIST_FROM and P.shape[0] > k + 64
    if not shortlist:
        return knn_ip_ref.knn_ip_topk(P, Q, k, row_offset)
    oD, oI = [], []
    for s in range(0, Q.shape[0], 128):                   # (query chunks: the BLAS product is [chunk, N] fp64)
        d, i, gap, bound = knn_ip_ref.knn_ip_topk_shortlisted(P, Q[s:s + 128], k, row_offset)
        assert np.all(gap > bound), "the oracle's shortlist cut-off is too close to the k-th value"
        oD.append(d); oI.append(i)
    return np.concatenate(oD), np.concatenate(oI)


def _store(Ph, dev):
    N, D = Ph.shape
    P = torch.zeros((N, (D + 3) // 4 * 4), dtype=torch.float32, device=dev)
    P[:, :D] = torch.from_numpy(Ph).to(dev)
    return P


def _bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int64 if a.element_size() == 8 else torch.int32),
                       b.contiguous().view(torch.int64 if b.element_size() == 8 else torch.int32))


def _search_both(P, N, D, Q, k, row_offset=0, prep=None, ws=None):
    """prepared route and fp32-sweep route on device tensors; asserts their bit equality.  -> (D, I, exact64, stats list)"""
    from adaptive_classifier import index as ix
    dev = Q.device
    prep = prep if prep is not None else ix.prepare_store(P, N, D)
    assert ix.batch_applies(N, Q.shape[0], k)
    st = torch.zeros(4, dtype=torch.int32, device=dev)
    ex = torch.empty((Q.shape[0], k), dtype=torch.float64, device=dev)
    ex0 = torch.empty_like(ex)
    Db, Ib = ix.knn_ip_topk(P, N, D, Q, k, row_offset=row_offset, stats=st, exact_out=ex, prepared=prep, workspace=ws)
    Ds, Is = ix.knn_ip_topk(P, N, D, Q, k, row_offset=row_offset, exact_out=ex0)          # the fp32 sweeps: the parent's route
    torch.cuda.synchronize()
    assert torch.equal(Ib, Is), "ids differ from the fp32-sweep route: %d" % int((Ib != Is).sum())
    assert _bits_equal(Db, Ds) and _bits_equal(ex, ex0)
    assert torch.equal(ex.float(), Db)                                                     # fp32 = fp64 rounded once
    return Db, Ib, ex, st.tolist()


def _run(Ph, Qh, k, dev, row_offset=0, oracle=True, shortlist=None):
    """-> (values, ids, fallback queries, form): form 2 = the fp16-plane sweep ran"""
    N, D = Ph.shape
    Db, Ib, ex, st = _search_both(_store(Ph, dev), N, D, torch.from_numpy(Qh).to(dev), k, row_offset)
    d, i = Db.cpu().numpy(), Ib.cpu().numpy()
    assert np.all((i == -1) | ((i >= row_offset) & (i < N + row_offset))), "an id outside the store"
    print("N=%d D=%d nq=%d k=%d: exact-fallback queries %d, form %d" % (N, D, Qh.shape[0], k, st[0], st[1]))
    if oracle:
        oD, oI = _oracle(Ph, Qh, k, row_offset, shortlist)
        assert np.array_equal(i, oI), f"{(i != oI).sum()} id mismatches against the oracle"
        assert _ulp_close(d, oD)
        e = ex.cpu().numpy()
        assert np.all(e[:, :-1] >= e[:, 1:])                                               # descending
    return d, i, st[0], st[1]


# ---------------------------------------------------------------------------------------------- GEMM form (>= 64 queries)
@pytest.mark.parametrize("N,D,nq,k", [
    (200_000, 768, 256, 16),
    (70_001, 100, 65, 8),          # D % 16 != 0 (zero-padded k-slots), ragged row / query tiles
    (131_072, 1024, 128, 32),      # exact tile multiples
    (65_536, 770, 64, 100),        # D % 4 != 0, the largest k of the batched path, the smallest store
])
def test_ip_batched_path_matches_oracle(N, D, nq, k, cuda_dev):
    from oracle import synth
    Ph = synth.synth_unit_rows(N, D, 1)
    Qh = synth.synth_unit_rows(nq, D, 2)
    d, i, nfb, form = _run(Ph, Qh, k, cuda_dev, row_offset=7)
    assert form != 2 or nq <= 64                 # (64 queries still fit the plane sweep, in two 32-column passes)
    assert nfb <= 2, "exact-fallback queries: %d" % nfb


# ---------------------------------------------------------------------------------------------- plane form (1 .. 63 queries)
@pytest.mark.parametrize("N,D,nq,k", [
    (70_001, 768, 1, 16), (70_001, 768, 16, 32), (131_072, 768, 32, 32), (100_003, 768, 33, 32), (90_000, 768, 48, 32),
    (65_536, 768, 63, 8), (70_001, 1024, 40, 32), (70_001, 100, 17, 8), (80_000, 64, 63, 100), (66_000, 770, 5, 1),
])
def test_ip_plane_sweep_matches_oracle(N, D, nq, k, cuda_dev):
    from oracle import synth
    Ph = synth.synth_unit_rows(N, D, 1)
    Qh = synth.synth_unit_rows(nq, D, 2)
    d, i, nfb, form = _run(Ph, Qh, k, cuda_dev, row_offset=11)
    assert form == 2, "the fp16-plane sweep did not run"
    assert nfb <= 2, "exact-fallback queries: %d" % nfb


# ---------------------------------------------------------------------------------------------- stress stores
@pytest.mark.parametrize("nq", [70, 20])
def test_ip_unnormalised_rows(nq, cuda_dev):
    """Rows and queries far from unit norm (the error bound scales with (|p|max + |q|)^2).  Cap 2: a CPU emulation of the
    fp16 proposal + certificate gave 0 failures on this store."""
    rng = np.random.default_rng(5)
    Ph = (rng.standard_normal((80_000, 256)) * 3 + 0.5).astype(np.float32)
    Qh = (rng.standard_normal((nq, 256)) * 0.3).astype(np.float32)
    d, i, nfb, form = _run(Ph, Qh, 10, cuda_dev)
    assert (form == 2) == (nq < 64) and nfb <= 2, (form, nfb)


@pytest.mark.parametrize("nq", [70, 20])
def test_ip_mixed_norms_differs_from_l2(nq, cuda_dev):
    """Unit rows x linspace(0.5, 4): the inner product prefers long rows, L2 short ones -- an L2 answer cannot pass."""
    from adaptive_classifier import index as ix
    from oracle import synth
    N, D, k = 80_000, 256, 10
    Ph = (synth.synth_unit_rows(N, D, 3) * np.linspace(0.5, 4.0, N, dtype=np.float32)[:, None]).astype(np.float32)
    Qh = synth.synth_unit_rows(nq, D, 4)
    d, i, nfb, form = _run(Ph, Qh, k, cuda_dev)
    assert (form == 2) == (nq < 64) and nfb <= 2, (form, nfb)
    P, Q = _store(Ph, cuda_dev), torch.from_numpy(Qh).to(cuda_dev)
    _, I_l2 = ix.knn_l2_topk(P, N, D, Q, k, prepared=ix.prepare_store(P, N, D))
    assert all(set(a) != set(b) for a, b in zip(i.tolist(), I_l2.cpu().tolist()))


def _all_negative(N, D, nq, seed):
    """rows in the positive orthant, queries = their negated mean plus noise: EVERY product is negative, so a padding row's
    v = 0 would be the best value of the whole sweep"""
    rng = np.random.default_rng(seed)
    Ph = (np.abs(rng.standard_normal((N, D))) + 0.1).astype(np.float32)
    Qh = (-Ph.mean(0)[None, :] + rng.standard_normal((nq, D)) * 0.05).astype(np.float32)
    assert (Qh < 0).all()
    return Ph, Qh


@pytest.mark.parametrize("two_phase", ["1", "0"])
@pytest.mark.parametrize("N", [70_001, 65_536 + 8])
def test_ip_all_products_negative_ragged_last_tile(N, two_phase, cuda_dev, monkeypatch):
    """Padding rows must never qualify and never be published as a two-phase minimum: the last 256-row tile is ragged, all real
    values v = -2 p.q are POSITIVE and a zero (or clamped-copy) padding row would beat them all.  A leak shows up as ids >= N
    or as mass fallbacks."""
    monkeypatch.setenv("AC_KNN_TWO_PHASE", two_phase)
    for nq in (80, 20) if two_phase == "1" else (80,):               # (the plane sweep does not read the switch)
        Ph, Qh = _all_negative(N, 64, nq, 17)
        d, i, nfb, form = _run(Ph, Qh, 10, cuda_dev)
        assert (d < 0).all() and (i >= 0).all() and (i < N).all()
        assert (form == 2) == (nq < 64)
        assert nfb <= 2, "exact-fallback queries: %d (padding rows in the minima?)" % nfb


@pytest.mark.parametrize("nq", [70, 40])
def test_ip_near_ties_and_duplicates(nq, cuda_dev):
    """A store full of fp32-unresolvable near-ties plus exact duplicates: whatever the fp16 proposal orders, the result is
    the exact-definition top-k, ties to the lower id."""
    from oracle import synth
    D, k = 128, 16
    Ph, centres = near_tie_store(66_000, D, 7)
    Ph[50_000:50_300] = Ph[100:400]                                    # exact duplicates of earlier rows
    nc = nq - 24
    Qh = np.concatenate([(centres[:nc] + synth.synth_unit_rows(nc, D, 8) * 1e-3), Ph[100:124]]).astype(np.float32)
    d, i, nfb, form = _run(Ph, Qh, k, cuda_dev, shortlist=False)
    assert (form == 2) == (nq < 64)
    dup = i[nc:]                                                       # queries that ARE duplicated rows: both copies tie exactly
    for q in range(24):
        row = dup[q].tolist()
        if 100 + q in row and 50_000 + q in row:
            assert row.index(100 + q) < row.index(50_000 + q)          # ... and the lower id comes first
    print("near-tie store: exact-fallback queries =", nfb)


@pytest.mark.parametrize("nq", [80, 40])
def test_ip_one_tight_cluster_goes_to_exact_fallback(nq, cuda_dev):
    """One tight cluster: every row passes every threshold, the lists overflow (or the certificate cannot separate the rows),
    and all queries must come back exact through the fp64 fallback."""
    from oracle import synth
    D, k, N = 128, 8, 70_000
    c = synth.synth_unit_rows(1, D, 3)
    rng = np.random.default_rng(1)
    Ph = (c + rng.standard_normal((N, D)).astype(np.float32) * 1e-4).astype(np.float32)
    Qh = (c + rng.standard_normal((nq, D)).astype(np.float32) * 1e-4).astype(np.float32)
    d, i, nfb, form = _run(Ph, Qh, k, cuda_dev, shortlist=False)
    assert nfb == nq


@pytest.mark.parametrize("two_phase", ["1", "0"])
def test_ip_largest_k_256_queries_ragged_tile(two_phase, cuda_dev, monkeypatch):
    """k = 100 (k' = 124 of 256 two-phase minima), 256 queries, unnormalised rows, a ragged last row tile; both threshold forms"""
    monkeypatch.setenv("AC_KNN_TWO_PHASE", two_phase)
    rng = np.random.default_rng(1)
    P3 = (rng.standard_normal((66_001, 96)) * 3 + 0.5).astype(np.float32)
    Q3 = (rng.standard_normal((256, 96)) * 0.3).astype(np.float32)
    _run(P3, Q3, 100, cuda_dev)


@pytest.mark.parametrize("nq", [65, 9])
def test_ip_zero_query_row(nq, cuda_dev):
    """A zero query: every product is 0, an exact tie over the whole store -> ids 0 .. k-1, values 0"""
    from oracle import synth
    N, D, k = 66_000, 64, 6
    Ph = synth.synth_unit_rows(N, D, 5)
    Qh = synth.synth_unit_rows(nq, D, 6)
    Qh[3] = 0.0
    d, i, nfb, form = _run(Ph, Qh, k, cuda_dev, shortlist=False)
    assert i[3].tolist() == list(range(k)) and (d[3] == 0).all()
    assert 1 <= nfb <= 3                                                # (the tie itself cannot be certified: 1, plus the cap of 2)


@pytest.mark.parametrize("two_phase", ["1", "0"])
def test_ip_thresholds_from_the_sweep_itself_or_from_sample_stages(two_phase, cuda_dev, monkeypatch):
    from oracle import synth
    monkeypatch.setenv("AC_KNN_TWO_PHASE", two_phase)
    N, D, nq, k = 90_000, 256, 100, 16
    d, i, nfb, form = _run(synth.synth_unit_rows(N, D, 1), synth.synth_unit_rows(nq, D, 2), k, cuda_dev)
    assert form != 2 and nfb <= 2


# the AC_KNN_THR_EXACT=1 leg: the switch is read once per process, so it runs in a fresh child (one GPU process at a time:
# this process only waits meanwhile)
def _thr_exact_child():
    from oracle import synth
    dev = torch.device("cuda:0")
    out = []
    # sample stages instead of the two-phase thresholds (AC_KNN_TWO_PHASE=0 in the child's environment), one and two stages
    Ph, Qh = synth.synth_unit_rows(70_001, 100, 1), synth.synth_unit_rows(65, 100, 2)
    out.append(_run(Ph, Qh, 8, dev, row_offset=7)[2])
    Ph, Qh = _all_negative(70_001, 64, 80, 17)                        # tau_key > 0: thr = 2 tau + E on positive sweep values
    out.append(_run(Ph, Qh, 10, dev)[2])
    rng = np.random.default_rng(5)
    Ph = (rng.standard_normal((80_000, 256)) * 3 + 0.5).astype(np.float32)
    Qh = (rng.standard_normal((70, 256)) * 0.3).astype(np.float32)
    out.append(_run(Ph, Qh, 10, dev)[2])
    from adaptive_classifier import index as ix
    N, D, nq, k = 1_000_000, 64, 300, 32                             # two threshold stages
    P, Q = ix.synth_unit_rows(N, D, 1, device=dev), ix.synth_unit_rows(nq, D, 2, device=dev)
    Db, Ib, ex, st = _search_both(P, N, D, Q, k)
    oD, oI = _oracle(P.cpu().numpy(), Q.cpu().numpy(), k)
    assert np.array_equal(Ib.cpu().numpy(), oI) and _ulp_close(Db.cpu().numpy(), oD)
    out.append(st[0])
    print("THR_EXACT_FALLBACKS", out)
    assert max(out) <= 2, out


def test_ip_exact_threshold_form_in_a_fresh_process(cuda_dev):
    """AC_KNN_THR_EXACT=1: the threshold stages re-rank their sample and take thr = 2 tau_key + E (rounded up), tau_key the
    k'-th smallest exact key -(p.q) of the sample."""
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    env = dict(os.environ, AC_KNN_THR_EXACT="1", AC_KNN_TWO_PHASE="0",
               PYTHONPATH=os.pathsep.join([here, root, os.path.join(root, "adaptive-classifier_amd")]))
    torch.cuda.synchronize()
    r = subprocess.run([sys.executable, "-c", "import test_knn_ip_batch_gpu as t; t._thr_exact_child()"], env=env, cwd=here,
                       capture_output=True, text=True, timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stderr[-3000:]
    assert "THR_EXACT_FALLBACKS" in r.stdout


def test_ip_two_threshold_stages_1M(cuda_dev):
    """1M rows, 768 queries: two threshold stages of similar size; <= 1 fallback, as for L2"""
    from adaptive_classifier import index as ix
    N, D, nq, k = 1_000_000, 64, 768, 32
    P = ix.synth_unit_rows(N, D, 1, device=cuda_dev)
    Q = ix.synth_unit_rows(nq, D, 2, device=cuda_dev)
    Db, Ib, ex, st = _search_both(P, N, D, Q, k)
    assert st[0] <= 1, "exact-fallback queries: %d" % st[0]
    oD, oI = _oracle(P.cpu().numpy(), Q.cpu().numpy(), k)
    assert np.array_equal(Ib.cpu().numpy(), oI) and _ulp_close(Db.cpu().numpy(), oD)


# ---------------------------------------------------------------------------------------------- metric interplay
@pytest.mark.parametrize("N,D,nq,k", [(70_001, 100, 65, 8), (70_001, 100, 17, 8)])
def test_l2_batch_unchanged_around_an_ip_batch_on_one_store_and_workspace(N, D, nq, k, cuda_dev):
    from adaptive_classifier import index as ix
    P = ix.synth_unit_rows(N, D, 1, device=cuda_dev)
    Q = ix.synth_unit_rows(nq, D, 2, device=cuda_dev)
    prep = ix.prepare_store(P, N, D)
    planes0, norms0 = prep[0].clone(), prep[1].clone()
    ws = torch.empty(ix.knn_batch_workspace_bytes(N, D, nq, k), dtype=torch.uint8, device=cuda_dev)
    st = torch.zeros(4, dtype=torch.int32, device=cuda_dev)
    e0 = torch.empty((nq, k), dtype=torch.float64, device=cuda_dev)
    e1, eu = torch.empty_like(e0), torch.empty_like(e0)
    D0, I0 = ix.knn_l2_topk(P, N, D, Q, k, workspace=ws, stats=st, exact_out=e0, prepared=prep)
    s0 = st.clone()
    Dp, Ip, _, _ = _search_both(P, N, D, Q, k, prep=prep, ws=ws)
    D1, I1 = ix.knn_l2_topk(P, N, D, Q, k, workspace=ws, stats=st, exact_out=e1, prepared=prep)
    Du, Iu = ix.knn_l2_topk(P, N, D, Q, k, exact_out=eu)                     # the unprepared L2 route
    torch.cuda.synchronize()
    assert torch.equal(I0, I1) and _bits_equal(D0, D1) and _bits_equal(e0, e1) and torch.equal(s0, st)
    assert torch.equal(I0, Iu) and _bits_equal(D0, Du) and _bits_equal(e0, eu)
    assert torch.equal(prep[0], planes0) and _bits_equal(prep[1], norms0)    # the store is read-only for both metrics
    assert not torch.equal(Dp, D0)


# ---------------------------------------------------------------------------------------------- index, sharded
def test_ip_index_prepares_on_a_many_query_search_and_follows_changes(cuda_dev, request):
    from adaptive_classifier import index as ixm
    from adaptive_classifier.index import HipFlatIPIndex
    from oracle import synth
    D = 64
    X = synth.synth_unit_rows(70_000, D, 11)
    Q = synth.synth_unit_rows(80, D, 12)
    idx = HipFlatIPIndex(D, device=cuda_dev)
    idx.add(X)
    old = ixm.BATCH_MIN_PAIRS
    ixm.BATCH_MIN_PAIRS = 1.0                                          # (the auto heuristic would keep this small case on the sweep)
    request.addfinalizer(lambda: setattr(ixm, "BATCH_MIN_PAIRS", old))

    def check(Xh, Qh, d, i):
        oD, oI = knn_ip_ref.knn_ip_topk(Xh, Qh, 5)
        assert np.array_equal(i, oI) and _ulp_close(d, oD)
    d, i = idx.search(Q, 5)
    assert idx._prepared is not None                                   # an 80-query search prepares the plane
    check(X, Q, d, i)
    idx.update_rows([3], Q[:1] * 1.5)                                  # row 3 := 1.5 x query 0: its best match by inner product (same store scale)
    assert idx._prepared is not None                                   # the plane follows the row
    d, i = idx.search(Q, 5)
    X2 = X.copy(); X2[3] = Q[0] * 1.5
    assert i[0, 0] == 3
    check(X2, Q, d, i)
    A = synth.synth_unit_rows(300, D, 13)                              # an append across a tile boundary
    A[5] = Q[2] * 1.75
    idx.add(torch.from_numpy(A).to(cuda_dev))
    X3 = np.concatenate([X2, A])
    assert idx._prepared is not None
    d, i = idx.search(Q, 5)
    assert i[2, 0] == 70_005
    check(X3, Q, d, i)
    d1, i1 = idx.search(Q[:8], 5)                                      # few queries: same answer
    assert np.array_equal(i1, i[:8]) and np.array_equal(d1, d[:8])
    idx.remove_ids(np.array([10]))
    assert idx._prepared is None                                       # a compaction drops the plane
    X4 = np.delete(X3, [10], axis=0)
    d, i = idx.search(Q[:8], 5)
    assert idx._prepared is None                                       # ... and few-query searches never prepare it again
    check(X4, Q[:8], d, i)


def test_ip_index_never_prepares_from_small_searches_but_uses_an_existing_plane(cuda_dev, request):
    from adaptive_classifier import index as ixm
    from adaptive_classifier.index import HipFlatIPIndex
    from oracle import synth
    D = 64
    X = synth.synth_unit_rows(70_000, D, 21)
    Q = synth.synth_unit_rows(80, D, 22)
    old = (ixm.PLANE_MIN_ROWS, ixm.BATCH_MIN_PAIRS)
    ixm.PLANE_MIN_ROWS, ixm.BATCH_MIN_PAIRS = 65_536, 1.0
    request.addfinalizer(lambda: (setattr(ixm, "PLANE_MIN_ROWS", old[0]), setattr(ixm, "BATCH_MIN_PAIRS", old[1])))
    idx = HipFlatIPIndex(D, device=cuda_dev)
    idx.add(X)
    oD, oI = knn_ip_ref.knn_ip_topk(X, Q, 5)
    for _ in range(3):                                                 # an L2 index would prepare at the second search
        d, i = idx.search(Q[:9], 5)
        assert idx._prepared is None and int(idx._stats[1].item()) != 2
        assert np.array_equal(i, oI[:9]) and _ulp_close(d, oD[:9])
    d, i = idx.search(Q, 5)
    assert idx._prepared is not None
    assert np.array_equal(i, oI) and _ulp_close(d, oD)
    d9, i9 = idx.search(Q[:9], 5)                                      # the plane exists: small batches sweep it
    assert int(idx._stats[1].item()) == 2
    assert np.array_equal(i9, i[:9]) and np.array_equal(d9, d[:9])
    idx.reset()
    assert idx._prepared is None


@pytest.mark.parametrize("G", [2, 8])
def test_ip_logical_shards_prepared_equal_unsharded_1M(G, cuda_dev):
    from adaptive_classifier import index as ix
    from adaptive_classifier.sharded import ShardedSearch, shard_bounds
    N, D, nq, k = 1_000_000, 768, 96, 32
    P = ix.synth_unit_rows(N, D, 1, device=cuda_dev)
    Q = ix.synth_unit_rows(nq, D, 2, device=cuda_dev)
    uD, uI = ix.knn_ip_topk(P, N, D, Q, k)                              # unsharded, the fp32 sweeps
    parts = []
    for g in range(G):
        lo, hi = shard_bounds(N, G, g)
        ss = ShardedSearch(P[lo:hi], hi - lo, D, lo, metric="ip")
        parts.append(ss._search(ss.rows, ss.n_local, D, Q, k, lo))
        assert (ss._prepared is not None) == ix.batch_applies(hi - lo, nq, k, auto=True)
        del ss
    assert ix.batch_applies(N // 2, nq, k, auto=True) and not ix.batch_applies(N // 8, nq, k, auto=True)   # both routes are covered
    mD, mI = ix.topk_merge_ip(torch.stack([p[0] for p in parts]), torch.stack([p[1] for p in parts]))
    assert torch.equal(mI, uI) and _bits_equal(mD, uD)
