"""GPU suite: every kNN entry on a non-default stream, with its inputs arriving late (tests/stream_lag.py).

Every case of tests/knn_call_cases.py (the functional wrappers for both metrics as listed there, the index and world-1 sharded
sequences, stores, merges) and the odd-sized range cases of tests/test_poison_knn_gpu.py runs three times: plainly on the default
stream; A. on a side stream that is still asleep, the queries, the radii and (stores) the appended rows holding another seed's
valid values until an in-stream copy_ behind the sleep brings the true ones; B. on an idle side stream while the default
stream sleeps.  (a) A and B are bit-identical to the plain run -- returned tensors plus the caller's out / exact_out / stats;
(b) as in test_poison_knn_gpu.py: ids and lims equal the fp64 oracle of the family, values within 1 ulp; (c) every native call of
A returned while the side stream was still asleep (the guard against an empty test); the kNN entries have no host wait:

HOST_WAITS, read from csrc/knn_l2.hip, knn_batch.hip, knn_exact.hip, knn_range.hip, knn_select.hip, memory_ops.hip, synth.hip:
  (none)  knn_l2.hip:1477-1482 synchronises and copies back only under the AC_KNN_DEBUG print; common.hip:74,86 (the active-CU
          probe) only where a CU mask is in the environment.  The range WRAPPERS (index.py) read `lims` on the host between the
          count and the fill entry: the entries themselves do not wait, and the spy lags the stream again before the fill.
"""
import time
import types

import numpy as np
import pytest
import torch

import knn_call_cases as cases
import poison
import stream_lag as sl
import test_poison_knn_gpu as pk
from knn_call_cases import D, K, N_BATCH, N_PLANE, N_SMALL

pytestmark = pytest.mark.gpu

_T0 = time.time()
HOST_WAITS = {}                          # entry -> "file:line  what waits" (see the module docstring: no kNN entry waits)
FAMILY = ("ac_knn_", "ac_topk_merge")
NOT_STREAMED = {"ac_knn_set_profile_events"}          # (takes two events, no stream)
SEEN = {}                                # entry -> True once a scenario-A call of it returned under the sleeping stream


# ---- the cases: name -> (metric, run(env) -> nested device result, check(world, host result)) ---------------------------------
def _wrapper_case(name, m, fn, s, uses_ex, uses_stats):
    def run(e):
        out = fn(e)
        return [out, e.ex[: s["nq"]] if uses_ex else None, e.stats if uses_stats else None]

    def check(w, got):
        pk.check(w, m, s, got[0], got[1])
        if "prepared" in name and "falls_back" not in name and name.startswith("range") and uses_stats:
            assert got[2][2] == 2, "the count did not read the plane"
    return run, check


def _sequence_case(name):
    m, specs = pk.SEQUENCES[name]
    fn = dict(cases.CASES)[name]

    def check(w, got):
        ss = specs()
        assert len(got) == len(ss)
        for s, g in zip(ss, got):
            pk.check(w, m, s, g)
    return fn, check


def _store_case():
    fn = dict(cases.CASES)["store_functions"]

    def run(e):
        ix = e.ix
        prepared, ok, small = fn(e)
        assert ok is True
        out = []
        for m in ("l2", "ip"):
            topk = ix.knn_ip_topk if m == "ip" else ix.knn_l2_topk
            out.append(topk(e.P, N_BATCH + 10, D, e.Q, K, prepared=prepared))
            out.append(topk(e.P, N_BATCH + 10, D, e.Q3, K, prepared=prepared))
            out.append(ix.knn_range_search(e.P, N_BATCH + 10, D, e.Q3, e.radius(m), metric=m, prepared=prepared))
        return out

    def check(w, got):
        for i, m in enumerate(("l2", "ip")):
            pk.check(w, m, pk.spec("topk", N=N_BATCH + 10, nq=70), got[3 * i])
            pk.check(w, m, pk.spec("topk", N=N_BATCH + 10), got[3 * i + 1])
            pk.check(w, m, pk.spec("range", N=N_BATCH + 10), got[3 * i + 2])
    return run, check


def _merge_case():
    fn = dict(cases.CASES)["merges"]

    def check(w, got):
        import knn_ip_ref
        d = np.arange(2 * 3 * K, dtype=np.float64).reshape(2, 3, K)
        i = np.arange(2 * 3 * K, dtype=np.int64).reshape(2, 3, K)
        for (gD, gI), src in ((got[0], d), (got[1], d.astype(np.float32))):
            oD, oI = knn_ip_ref.topk_merge_ip(-src.astype(np.float64), i, K)
            assert np.array_equal(gI, oI) and np.array_equal(gD, -oD)
        oD, oI = knn_ip_ref.topk_merge_ip(d[..., ::-1], i, K)
        assert np.array_equal(got[2][1], oI) and np.array_equal(got[2][0], oD)
    return fn, check


def _sharded_handles_case(m):
    """The GPU counterpart of test_sharded_gloo.py's slot test: two prefetched handles outstanding, a handle-less search_block
    between them; each search returns the neighbours of ITS OWN block."""
    def run(e):
        from adaptive_classifier.sharded import ShardedSearch
        ss = ShardedSearch(e.P, N_BATCH, D, 64, metric=m, block_rows=32)
        h1, h2 = ss.prefetch_queries(e.Q[:32]), ss.prefetch_queries(e.Q[32:64])
        with pytest.raises(RuntimeError):
            ss.prefetch_queries(e.Q[64:])
        r3 = ss.search_block(e.Q[64:], K)
        r1 = ss.search_block(None, K, gathered=h1)
        r2 = ss.search_block(None, K, gathered=h2)
        with pytest.raises(RuntimeError):
            ss.search_block(None, K, gathered=h1)
        return [r1, r2, r3]

    def check(w, got):
        assert [g[1].shape[0] for g in got] == [32, 32, 6]
        whole = (np.concatenate([g[0] for g in got]), np.concatenate([g[1] for g in got]))
        pk.check(w, m, pk.spec("topk", N=N_BATCH, nq=70, off=64), whole)
    return run, check


def _legacy_entry_case(m):
    """ac_knn_l2_topk / ac_knn_ip_topk, the entries without the exact output, which the Python layer no longer calls: the smallest
    direct call, into the caller's buffers"""
    def run(e):
        from adaptive_classifier import _native as nv
        fn = getattr(nv.lib(), f"ac_knn_{m}_topk")
        nv.check(fn(nv.ptr(e.P), N_SMALL, e.P.stride(0), D, nv.ptr(e.Q), 70, e.Q.stride(0), K, 5, nv.ptr(e.out[0]), nv.ptr(e.out[1]),
                    nv.ptr(e.ws), e.ws.numel(), nv.ptr(e.stats), nv.stream_ptr(e.dev)), f"ac_knn_{m}_topk")
        return [e.out[0], e.out[1], e.stats]

    def check(w, got):
        pk.check(w, m, pk.spec("topk", nq=70, off=5), (got[0], got[1]))
    return run, check


def _index_life_case(m):
    """A whole HipFlatL2Index / HipFlatIPIndex life from a fresh object: add, search twice (the L2 index prepares its plane at the
    second), add, remove_ids, range search.  Late inputs are not needed -- the object makes its own buffers; each result must
    be bit-identical to the same life of a fresh object on the default stream (and the first two equal the oracle)."""
    def run(e):
        idx = e.index(m, N_PLANE)
        res = [idx.search_device(e.Q3, K), idx.search_device(e.Q3, K)]
        idx.add(e.P[:5, :D])
        res.append(idx.search_device(e.Q3, K))
        idx.remove_ids([0, 17])
        res.append(idx.search_device(e.Q3, K))
        res.append(idx.range_search_device(e.Q3, e.radius(m)))
        return res

    def check(w, got):
        assert len(got) == 5
        for g in got[:2]:
            pk.check(w, m, pk.spec("topk", N=N_PLANE), g)
    return run, check


N_SELPACK = 333                           # not a multiple of 64: the last bitmap word is partial
MASK_HOST = np.arange(N_SELPACK) % 3 != 0
ROW_CLASS_HOST = (np.arange(N_SELPACK) % 3).astype(np.int32)          # classes 1 and 2 on <=> MASK_HOST


def _device_selector_case():
    """RowSelector.from_mask / from_classes of DEVICE inputs (ac_knn_sel_pack, ac_knn_sel_classes): the bitmaps equal the host
    packing of the same mask, and a filtered search through each returns the oracle's neighbours"""
    def run(e):
        ix = e.ix
        a = ix.RowSelector.from_mask(e.mask_dev)
        b = ix.RowSelector.from_classes(e.row_class_dev, [1, 2, 7], 3)
        return [a.words, b.words] + [ix.knn_topk_sel(e.P, N_SELPACK, D, e.Q3, K, s, metric="l2") for s in (a, b)]

    def check(w, got):
        want = w.ix.RowSelector.from_mask(MASK_HOST).words.cpu().numpy()
        assert np.array_equal(got[0], want) and np.array_equal(got[1], want)
        for g in got[2:]:
            pk.check(w, "l2", pk.spec("topk", N=N_SELPACK, mask=("mod3",)), g)
    return run, check


CASES = {}
for _c in pk.WRAPPER_CASES:
    CASES[_c[0]] = _wrapper_case(*_c)
for _n in pk.SEQUENCES:
    CASES[_n] = _sequence_case(_n)
CASES["store_functions"] = _store_case()
CASES["merges"] = _merge_case()
for _m in ("l2", "ip"):
    CASES[f"sharded_{_m}_two_handles_and_a_handle_less_search"] = _sharded_handles_case(_m)
    CASES[f"legacy_entry_{_m}_300_q70"] = _legacy_entry_case(_m)
    CASES[f"index_life_{_m}"] = _index_life_case(_m)
CASES["selectors_from_device_mask_and_classes"] = _device_selector_case()
assert all(n in CASES for n in cases.NAMES), "a case of knn_call_cases.py has no stream test"


@pytest.fixture(scope="module")
def world(cuda_dev):
    global _T0
    _T0 = time.time()
    from adaptive_classifier import _native as nv
    from adaptive_classifier import index as ix
    import knn_range_ref as rref
    env = pk._Env(ix, cuda_dev, types.SimpleNamespace(named=None))
    env.prep_odd = ix.prepare_store(env.P, pk.N_ODD, D)
    P = env.P[:, :D].cpu().numpy()
    Q = env.Q[:, :D].cpu().numpy()
    x = {m: rref.fixed_order_values(P, Q, m) for m in ("l2", "ip")}
    w = types.SimpleNamespace(env=env, P=P, Q=Q, x=x, refs={}, ix=ix, dev=cuda_dev)
    # the late inputs and their stale stand-ins: the queries (Q3 / Q0 are views of Q), the radii, the rows update_store appends
    w.live = [env.Q, env.rad["l2"], env.rad["ip"], env.P[N_BATCH: N_BATCH + 10]]
    w.stale = [ix.synth_unit_rows(70, D, 10, device=cuda_dev), torch.full((70,), 0.3, device=cuda_dev),
               torch.full((70,), 0.8, device=cuda_dev), env.P[N_BATCH + 100: N_BATCH + 110].clone()]
    env.mask_dev = torch.from_numpy(MASK_HOST).to(cuda_dev)
    env.row_class_dev = torch.from_numpy(ROW_CLASS_HOST).to(cuda_dev)
    w.live += [env.mask_dev, env.row_class_dev]
    w.stale += [~env.mask_dev, (env.row_class_dev + 1) % 3]
    w.side = torch.cuda.Stream(device=cuda_dev)
    per_ms = sl.calibrate(cuda_dev)
    with sl.EntrySpy(nv) as spy:
        w.spy = spy
        # every case plainly on the default stream first: the reference bits and the host time that sizes the lag
        w.plain, w.host_ms = {}, {}
        for name, (run, _) in CASES.items():
            env.obj = None
            out, w.host_ms[name] = sl.plain(spy, lambda: run(env))
            w.plain[name] = sl.to_host(out)
        slowest = max(w.host_ms, key=w.host_ms.get)
        w.lag_ms = sl.choose_lag(w.host_ms[slowest])
        print(f"\nMEASURED test_stream_knn_gpu: {per_ms:.0f} sleep cycles per ms; slowest case {slowest} {w.host_ms[slowest]:.2f} ms of host time "
              f"between its first and last native call; lag {w.lag_ms:.0f} ms")
        yield w
    print(f"\nMEASURED test_stream_knn_gpu wall time {time.time() - _T0:.1f} s")


@pytest.mark.parametrize("name", list(CASES))
def test_side_stream_lags_and_inputs_arrive_late(name, world):
    w, (run, check) = world, CASES[name]
    w.env.obj = None
    out, readings = sl.side_late(w.spy, w.side, w.lag_ms, lambda: run(w.env), w.live, w.stale)
    got = sl.to_host(out)
    if readings or not any(t in name for t in ("no_queries", "no_rows", "empty_list")):      # (an empty search may return at once)
        sl.assert_enqueued(readings, HOST_WAITS, name)
    sl.note(__name__, readings, HOST_WAITS)
    for n, done in readings:
        if not done:
            SEEN[n] = True
    assert poison.same_bits(w.plain[name], got), "work ran ahead of the side stream: " + poison.first_difference(w.plain[name], got)
    check(w, got)


@pytest.mark.parametrize("name", list(CASES))
def test_default_stream_lags_call_on_an_idle_side_stream(name, world):
    w, (run, check) = world, CASES[name]
    w.env.obj = None
    got, readings = sl.default_lags(w.spy, w.side, w.lag_ms, lambda: run(w.env))
    assert not any(done for _, done in readings), f"{name}: the default stream's lag ran out before the case had been enqueued"
    assert poison.same_bits(w.plain[name], got), "work went to the default stream: " + poison.first_difference(w.plain[name], got)
    check(w, got)


def test_every_knn_entry_was_seen_returning_under_a_sleeping_stream(world):
    """The guard: every exported kNN symbol that takes a stream returned, in scenario A above, while its stream was still behind
    the sleep (or is listed in HOST_WAITS with the line that waits)."""
    from adaptive_classifier import _native as nv
    mine = {n for n in nv.exported_symbols() if n.startswith(FAMILY)} & sl.stream_entries()
    assert mine and not (mine & NOT_STREAMED)
    missing = sorted(n for n in mine if not SEEN.get(n) and n not in HOST_WAITS)
    assert not missing, f"never seen returning under a lagging stream: {missing}"


# For the record (one run on an MI355X, inside the whole suite): 2412851 sleep cycles per ms; slowest case index_l2_2p18, 4.60 ms of host
# time between its first and last native call; lag 46 ms; module wall time 13.0 s.
