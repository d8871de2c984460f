"""GPU suite: every kNN entry over poisoned workspaces, outputs, stats and message buffers (tests/poison.py).

Regions, read from the host launchers (csrc/knn_l2.hip, knn_batch.hip, knn_exact.hip, knn_range.hip) and index.py / sharded.py
before any poisoned run.  No region is the caller's duty to clear.

  top-k over fp32 rows (ac_knn_{l2,ip}_topk_x / _sel; one plan, one workspace, knn_l2.hip knn_topk):
      part_d / part_i / part_maxnorm   written by every sweep workgroup for every query slot of its tile (slots past a list's
                                       count as +inf / -1); N == 0: part_i memset to -1, part_maxnorm to 0, part_d left as it
                                       is -- the merge reads part_d[t] only where part_i[t] >= 0 (knn_exact.hip `real`)
      fallback counter, d_stats        cleared by the sweep's workgroup 0 (N > 0), by hipMemsetAsync for N == 0 / the small store
      flags, exact-stage lists         written by the merge before the fallback stages read them
      small store (N <= 8192 beyond the sweep's k / D): no workspace
  top-k over the prepared store (_topk_batch / _batch_sel): the same tail; query plane, factors and thresholds are written by
      knn_prepare_queries, whose launch also zeroes the candidate counters (each threshold-stage merge re-zeroes the ones it read);
      fewer than 64 queries: knn_plane_sweep writes part_d / part_i like the fp32 sweep and clears the fallback counter and d_stats
  ac_knn_*_topk_ids: no workspace
  range count (knn_range.hip range_count / range_count_batch / range_count_ids):
      bm_in, bm_amb      large stores: hipMemsetAsync of both, the sweep ORs non-zero pieces in; small stores and the id-list
                         route: every (query, word) stored whole by the wave that owns it (tail bits of the last word = lanes
                         past N / M, never hits)
      cnt, off, lims     cnt by resolve / small / ids_count for every (query, strip); off and lims by knn_range_scan
      plane route        query plane, factors, thresholds, live flags for all q_rows (padding rows included) by
                         knn_prepare_queries / knn_plane_range_thresholds
      fill               reads bm_in / off / lims of the count; writes positions < lims[nq] <= capacity only
      d_stats            hipMemsetAsync at the head of every count
  ac_knn_prepare_store / ac_knn_update_store: plane rows and norms of the rows named, the store maximum at norms[round_up(N,256)]
      (memset, then atomic max); rows past N of the last 256-row tile are masked by the sweeps
  ac_topk_merge*: outputs only
  ShardedSearch (world 1): qpad rows [m, block_rows) zeroed by prefetch_queries; candidate messages only with collectives

Every case of tests/knn_call_cases.py (the functional wrappers for BOTH metrics, the index and sharded sequences, stores,
merges) and the extra cases below runs in four states: zero, zero again, ff, leftover (the family's largest calls first, on the
same caller buffers / the same object, nothing refilled).  (a) the returned tensors -- plus the caller's exact_out and stats
where the case passes them -- are bit-identical; (b) ids / lims equal the fp64 oracle of the family's suite (c_oracle,
knn_ip_ref, knn_select_ref, knn_range_ref, knn_range_sel_ref), values within 1 ulp, the fp64 output rounds to the fp32 one.
"""
import time
import types

import numpy as np
import pytest
import torch

import knn_call_cases as cases
import knn_ip_ref
import knn_range_ref as rref
import knn_range_sel_ref as rsref
import knn_select_ref as sref
import poison
from knn_call_cases import D, K, N_BATCH, N_PLANE, N_SMALL

pytestmark = pytest.mark.gpu

_T0 = time.time()
N_ODD = N_BATCH + 37                     # a plane-route store whose last bitmap word is partial
G_MASK = np.arange(N_PLANE + 128) % 3 != 0       # Env.sel: the global selector
IDS5 = [3, 10, 11, 200, 299]


def _ulp_close(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        return bool(np.all(np.abs(a - b) <= np.spacing(np.maximum(np.abs(a), np.abs(b)).astype(np.float32))))


class _Env(cases.Env):
    """Env whose index() can first run the family's largest searches on the new index (the leftover state)."""
    warm = False

    def index(self, metric, n):
        idx = super().index(metric, n)
        if self.warm:
            idx.search_device(self.Q, K)
            idx.range_search_device(self.Q, self.rad[metric])
            idx._prepared, idx._searches_since_change = None, 0        # (the route of the sequence's first search stays its own)
        return idx


@pytest.fixture(scope="module")
def world(cuda_dev):
    from adaptive_classifier import index as ix
    env = _Env(ix, cuda_dev, types.SimpleNamespace(named=None))
    env.prep_odd = ix.prepare_store(env.P, N_ODD, D)
    P = env.P[:, :D].cpu().numpy()
    Q = env.Q[:, :D].cpu().numpy()
    x = {m: rref.fixed_order_values(P, Q, m) for m in ("l2", "ip")}
    w = types.SimpleNamespace(env=env, P=P, Q=Q, x=x, refs={}, ix=ix, dev=cuda_dev)
    yield w
    print(f"\nMEASURED test_poison_knn_gpu wall time {time.time() - _T0:.1f} s")


# ---- what a call must return ---------------------------------------------------------------------------------------------------
def spec(kind, N=N_SMALL, nq=3, off=0, mask=None, store="base"):
    """kind: topk | topk_exact | range | range_exact;  mask: None | ("g", bit0) the global selector from bit0 | ("ids",) |
    ("mod3",) arange(N) % 3 != 0;  store: base | grown (5 rows appended, 4 overwritten) | compacted (row 0 of that removed)"""
    return dict(kind=kind, N=N, nq=nq, off=off, mask=mask, store=store)


def _store_values(w, m, s):
    """(rows, exact values [nq, N]) of the store a spec searches"""
    x, P = w.x[m][: s["nq"]], w.P
    if s["store"] == "base":
        return P[: s["N"]], x[:, : s["N"]]
    x2, P2 = np.concatenate([x[:, :N_PLANE], x[:, :5]], axis=1), np.concatenate([P[:N_PLANE], P[:5]])
    x2[:, [1, 2, 3, 9]], P2[[1, 2, 3, 9]] = x[:, 10:14], P[10:14]
    return (P2, x2) if s["store"] == "grown" else (P2[1:], x2[:, 1:])


def _mask(s, N):
    if s["mask"] is None:
        return None
    if s["mask"][0] == "g":
        return G_MASK[s["mask"][1]: s["mask"][1] + N]
    if s["mask"][0] == "mod3":
        return np.arange(N) % 3 != 0
    m = np.zeros(N, dtype=bool)
    m[[i for i in IDS5 if i < N]] = True
    return m


def _shortlist(x, mask, k, ip):
    """a sub-mask that still holds every query's k best selected rows (all rows tied with the k-th included): the oracle's
    per-query sort then runs over a few rows instead of the whole store -- the same result by construction"""
    v = np.where(mask[None, :], -x if ip else x, np.inf)
    if mask.sum() <= 4 * k + 64:
        return mask
    kth = np.partition(v, k, axis=1)[:, k]
    return mask & (v <= kth[:, None]).any(axis=0)


def expected(w, m, s):
    key = (m,) + tuple(sorted((k, str(v)) for k, v in s.items()))
    if key in w.refs:
        return w.refs[key]
    P, x = _store_values(w, m, s)
    N, nq, mask = P.shape[0], s["nq"], _mask(s, P.shape[0])
    rad = cases.R_IP if m == "ip" else cases.R_L2
    if s["kind"].startswith("topk"):
        if mask is None and N and nq:
            if m == "l2":
                from oracle import c_oracle
                oD, oI = c_oracle.knn_l2_topk(P, w.Q[:nq], K, row_offset=s["off"])
            else:
                oD, oI = knn_ip_ref.knn_ip_topk(P, w.Q[:nq], K, row_offset=s["off"])
        else:
            full = np.ones(N, dtype=bool) if mask is None else mask
            oD, oI, _ = sref.filtered_topk(None, None, K, _shortlist(x, full, K, m == "ip"), m, row_offset=s["off"], values=x)
        out = (np.asarray(oD, np.float32), np.asarray(oI, np.int64))
    elif mask is None:
        out = rref.range_search(P, w.Q[:nq], rad, m, row_offset=s["off"], values=x)
    else:
        out = rsref.filtered_range_search(P, w.Q[:nq], rad, mask, m, row_offset=s["off"], values=x)
    w.refs[key] = out
    return out


def check(w, m, s, got, ex=None):
    """one call's result (host arrays) against the oracle; ex: the caller's exact_out where the case passed one"""
    want = expected(w, m, s)
    if s["kind"].startswith("topk"):
        gD, gI = got
        oD, oI = want
        assert gI.shape == (s["nq"], K) and np.array_equal(gI, oI), f"{s}: {(gI != oI).sum()} ids differ"
        if s["kind"] == "topk_exact":
            ex, gD = gD, gD.astype(np.float32)
            pad = np.float32(-sref.FLT_MAX if m == "ip" else sref.FLT_MAX)
            gD = np.where(gI >= 0, gD, pad)
        assert _ulp_close(gD, oD), s
        if ex is not None:
            assert np.array_equal(ex[: s["nq"]][gI >= 0].astype(np.float32), gD[gI >= 0]), s
            assert np.all(np.isinf(ex[: s["nq"]][gI < 0])), s
        assert np.all(np.isfinite(gD))
    else:
        lims, gD, gI = got[:3]
        olims, oD, oI = want[:3]
        assert np.array_equal(lims, olims), (s, lims, olims)
        assert np.array_equal(gI, oI), s
        assert _ulp_close(gD, oD) and np.all(np.isfinite(gD)), s
        if s["kind"] == "range_exact":
            assert np.array_equal(got[3].astype(np.float32), gD), s


# ---- the wrapper cases: name without the metric -> (what it must return, does it pass exact_out= / stats=) -----------------
G0, G64, IDS = ("g", 0), ("g", 64), ("ids",)
WRAPPER = {
    "topk_{m}_300_q3": (spec("topk"), 0, 0),
    "topk_{m}_300_q70_caller_buffers": (spec("topk", nq=70, off=5), 1, 1),
    "topk_{m}_65535_prepared_falls_back": (spec("topk", N=N_BATCH - 1), 0, 0),
    "topk_{m}_65536_prepared_q3": (spec("topk", N=N_BATCH), 0, 0),
    "topk_{m}_65536_prepared_q70_caller_buffers": (spec("topk", N=N_BATCH, nq=70, off=5), 1, 1),
    "topk_{m}_65536_no_plane_q70": (spec("topk", N=N_BATCH, nq=70), 0, 0),
    "topk_exact_{m}_300": (spec("topk_exact", off=7), 0, 0),
    "topk_exact_{m}_65536_prepared": (spec("topk_exact", N=N_BATCH, nq=70), 0, 1),
    "topk_{m}_no_queries": (spec("topk", nq=0), 0, 0),
    "topk_{m}_no_rows": (spec("topk", N=0), 0, 0),
    "sel_{m}_300_bit0": (spec("topk", mask=G0), 0, 0),
    "sel_{m}_300_bit64_words_exact": (spec("topk", nq=70, off=64, mask=G64), 1, 1),
    "sel_{m}_65536_prepared_q3": (spec("topk", N=N_BATCH, mask=G0), 0, 0),
    "sel_{m}_65536_prepared_q70_bit64": (spec("topk", N=N_BATCH, nq=70, off=64, mask=G64), 1, 1),
    "sel_{m}_65535_prepared_falls_back": (spec("topk", N=N_BATCH - 1, mask=G0), 0, 0),
    "sel_{m}_no_queries": (spec("topk", nq=0, mask=G0), 0, 0),
    "ids_{m}_300": (spec("topk", mask=IDS), 0, 0),
    "ids_{m}_65536_exact_caller_buffers": (spec("topk", N=N_BATCH, nq=70, off=9, mask=IDS), 1, 0),
    "ids_{m}_empty_list": (spec("topk", N=0), 0, 0),                       # (no listed row: every slot is padding)
    "range_{m}_300_scalar": (spec("range"), 0, 0),
    "range_{m}_300_per_query_exact_stats": (spec("range_exact", nq=70, off=5), 0, 1),
    "range_{m}_300_chunked": (spec("range", nq=70), 0, 0),
    "range_{m}_300_sel_bit64": (spec("range", off=64, mask=G64), 0, 0),
    "range_{m}_65536_prepared": (spec("range", N=N_BATCH), 0, 1),
    "range_{m}_65536_prepared_sel_chunks_exact": (spec("range_exact", N=N_BATCH, nq=70, mask=G0), 0, 0),
    "range_{m}_65535_prepared_falls_back": (spec("range", N=N_BATCH - 1), 0, 0),
    "range_{m}_no_queries": (spec("range_exact", nq=0), 0, 0),
    "range_{m}_no_rows": (spec("range", N=0), 0, 0),
    "range_ids_{m}_scalar": (spec("range", mask=IDS), 0, 0),
    "range_ids_{m}_per_query_exact_stats": (spec("range_exact", N=N_BATCH, nq=70, off=9, mask=IDS), 0, 1),
    "range_ids_{m}_no_queries": (spec("range", nq=0, mask=IDS), 0, 0),
}


def _extra(m):
    """(name, call, spec, passes stats): N not a multiple of 64 on the range routes the table above leaves at whole words (the
    small store has N = 300, the fp32 sweep N = 65535, the id list M = 5 already)"""
    rng = lambda e: e.ix.knn_range_search                                       # noqa: E731
    return [
        (f"range_{m}_65573_prepared_q70", lambda e: rng(e)(e.P, N_ODD, D, e.Q, e.rad[m], metric=m, prepared=e.prep_odd, stats=e.stats),
         spec("range", N=N_ODD, nq=70), 1),
        (f"range_{m}_65573_prepared_sel", lambda e: rng(e)(e.P, N_ODD, D, e.Q3, e.radius(m), metric=m, prepared=e.prep_odd, sel=e.sel,
                                                           exact_out=True, stats=e.stats),
         spec("range_exact", N=N_ODD, mask=G0), 1),
        (f"range_{m}_65535_sel_q70", lambda e: rng(e)(e.P, N_BATCH - 1, D, e.Q, e.radius(m), metric=m, sel=e.sel.words, sel_bit0=64,
                                                      row_offset=64),
         spec("range", N=N_BATCH - 1, nq=70, off=64, mask=G64), 0),
    ]


WRAPPER_CASES = []
for _m in ("l2", "ip"):
    _fns = dict(cases._wrappers(_m))
    assert sorted(_fns) == sorted(n.format(m=_m) for n in WRAPPER)
    WRAPPER_CASES += [(n.format(m=_m), _m, _fns[n.format(m=_m)], s, ex, st) for n, (s, ex, st) in WRAPPER.items()]
    WRAPPER_CASES += [(n, _m, fn, s, 0, st) for n, fn, s, st in _extra(_m)]


def _host(x):
    if isinstance(x, torch.Tensor):
        return x.detach().cpu().numpy().copy()
    if isinstance(x, (list, tuple)):
        return [_host(v) for v in x]
    return x


def _states(w, monkeypatch, run, big=(), caller_buffers=True):
    """run(env) -> host results, in the four states.  big: the calls the leftover state runs first."""
    e = w.env
    p = poison.poisoned_empty(monkeypatch, None)
    res = {}
    for state, byte in (("zero", 0x00), ("zero2", 0x00), ("ff", 0xFF), ("leftover", None)):
        p.byte = byte
        e.warm = state == "leftover"
        if state == "leftover":
            for fn in big:
                fn(e)
        elif caller_buffers:
            for t in (e.ws, e.out[0], e.out[1], e.ex, e.stats):
                poison.fill(t, byte)
        e.obj = None
        res[state] = run(e)
        torch.cuda.synchronize()
    e.warm, p.byte = False, None
    assert poison.same_bits(res["zero"], res["zero2"]), "two zero-state runs differ: " + poison.first_difference(res["zero"], res["zero2"])
    for state in ("ff", "leftover"):
        assert poison.same_bits(res["zero"], res[state]), f"the {state} state changed the result: " + poison.first_difference(res["zero"], res[state])
    return res["ff"], p


@pytest.mark.parametrize("name,m,fn,s,uses_ex,uses_stats", WRAPPER_CASES, ids=[c[0] for c in WRAPPER_CASES])
def test_functional_wrappers(name, m, fn, s, uses_ex, uses_stats, world, monkeypatch):
    all_fns = dict(cases._wrappers(m))
    big = (all_fns[f"topk_{m}_65536_prepared_q70_caller_buffers"], all_fns[f"range_{m}_65536_prepared_sel_chunks_exact"])

    def run(e):
        out = _host(fn(e))
        return [out, _host(e.ex[: s["nq"]]) if uses_ex else None, _host(e.stats) if uses_stats else None]
    (got, ex, stats), p = _states(world, monkeypatch, run, big)
    check(world, m, s, got, ex)
    if "prepared" in name and "falls_back" not in name and name.startswith("range") and uses_stats:
        assert stats[2] == 2, "the count did not read the plane"


# ---- index and sharded sequences ---------------------------------------------------------------------------------------------
def _index_small_specs():
    return [spec("topk"), spec("topk", nq=70), spec("topk", mask=IDS), spec("topk", mask=("mod3",)), spec("range"),
            spec("range", nq=70, mask=("mod3",)), spec("range", mask=IDS), spec("range", nq=70)]


def _index_batch_specs():
    return [spec("topk", N=N_BATCH), spec("topk", N=N_BATCH), spec("topk", N=N_BATCH, nq=70),
            spec("topk", N=N_BATCH, nq=70, mask=("mod3",)), spec("range", N=N_BATCH)]


def _index_plane_specs():
    n, dense = dict(N=N_PLANE), dict(N=N_PLANE, mask=("mod3",))
    return [spec("topk", **n), spec("topk", **n), spec("topk", **dense), spec("topk", **n), spec("topk", **dense), spec("topk", **dense),
            spec("topk", N=N_PLANE, mask=IDS), spec("range", **n), spec("range", **dense), spec("range", N=N_PLANE, mask=IDS),
            spec("topk", N=N_PLANE + 5, store="grown"), spec("topk", N=N_PLANE + 4, store="compacted"),
            spec("range", N=N_PLANE + 4, store="compacted")]


def _sharded_specs():
    n = dict(N=N_PLANE, off=64)
    return [spec("topk", **n), spec("topk", nq=70, **n), spec("topk", mask=G64, **n), spec("range", **n), spec("range", mask=G64, **n),
            spec("topk", off=64, mask=G64), spec("range", off=64, mask=G64)]


SEQUENCES = {"index_l2_300": ("l2", _index_small_specs), "index_l2_65536": ("l2", _index_batch_specs),
             "index_l2_2p18": ("l2", _index_plane_specs), "index_ip_2p18": ("ip", _index_plane_specs),
             "sharded_l2_world1": ("l2", _sharded_specs), "sharded_ip_world1": ("ip", _sharded_specs)}


@pytest.mark.parametrize("name", list(SEQUENCES))
def test_index_and_sharded_sequences(name, world, monkeypatch):
    m, specs = SEQUENCES[name]
    fn = dict(cases.CASES)[name]
    got, p = _states(world, monkeypatch, lambda e: _host(fn(e)), caller_buffers=False)
    specs = specs()
    assert len(got) == len(specs) and p.filled > 0
    for s, g in zip(specs, got):
        check(world, m, s, g)


@pytest.mark.parametrize("m", ["l2", "ip"])
@pytest.mark.parametrize("N", [N_SMALL, N_BATCH])
def test_sharded_fixed_batch_with_a_short_last_block(N, m, world, monkeypatch):
    """block_rows = 32, 70 queries: blocks of 32, 32 and 6 -- the last travels with 26 padding rows in the persistent query
    message, which held a full block just before (leftover within the call sequence itself, in every state)."""
    from adaptive_classifier.sharded import ShardedSearch

    def run(e):
        ss = ShardedSearch(e.P, N, D, 64, metric=m, block_rows=32)
        out = [_host(r) for r in ss.search_blocks([e.Q[:32], e.Q[32:64], e.Q[64:]], K)]
        out.append(_host(ss.search_block(e.Q3, K)))                    # a short block into the slot a full one used
        assert ss.stats["buffer_allocations"] == 2
        return out
    got, p = _states(world, monkeypatch, run, caller_buffers=False)
    assert [g[1].shape[0] for g in got] == [32, 32, 6, 3] and p.filled > 0
    whole = (np.concatenate([g[0] for g in got[:3]]), np.concatenate([g[1] for g in got[:3]]))
    check(world, m, spec("topk", N=N, nq=70, off=64), whole)
    check(world, m, spec("topk", N=N, nq=3, off=64), got[3])


# ---- stores and merges -----------------------------------------------------------------------------------------------------
def test_store_functions_under_poisoned_plane_and_norms(world, monkeypatch):
    """prepare_store with spare capacity, update_store over ten appended rows, prepare_store of a small store: the plane and norms
    buffers come from torch.empty.  Their contents past the rows are undefined, so the defined result is what the searches over
    them return: top-k and range over the updated store, both metrics, in every state."""
    ix = world.ix
    fn = dict(cases.CASES)["store_functions"]

    def run(e):
        prepared, ok, small = fn(e)
        assert ok is True
        out = []
        for m in ("l2", "ip"):
            topk = ix.knn_ip_topk if m == "ip" else ix.knn_l2_topk
            st = torch.zeros(4, dtype=torch.int32, device=e.dev)
            out.append(_host(topk(e.P, N_BATCH + 10, D, e.Q, K, prepared=prepared)))        # 70 queries: the GEMM-form sweep
            out.append(_host(topk(e.P, N_BATCH + 10, D, e.Q3, K, prepared=prepared, stats=st)))
            assert st.tolist()[1] == 2, "the search did not read the plane"              # (< 64 queries: knn_plane_sweep reports itself)
            out.append(_host(ix.knn_range_search(e.P, N_BATCH + 10, D, e.Q3, e.radius(m), metric=m, prepared=prepared, stats=st)))
            assert st.tolist()[2] == 2, "the count did not read the plane"
        pe, ne = ix.store_buffers_sizes(N_SMALL, D)
        assert small[0].numel() == pe and small[1].numel() == ne
        return out
    got, p = _states(world, monkeypatch, run, caller_buffers=False)
    assert p.filled > 0
    for i, m in enumerate(("l2", "ip")):
        check(world, m, spec("topk", N=N_BATCH + 10, nq=70), got[3 * i])
        check(world, m, spec("topk", N=N_BATCH + 10), got[3 * i + 1])
        check(world, m, spec("range", N=N_BATCH + 10), got[3 * i + 2])


def test_merges_into_poisoned_outputs(world, monkeypatch):
    fn = dict(cases.CASES)["merges"]
    got, p = _states(world, monkeypatch, lambda e: _host(fn(e)), caller_buffers=False)
    assert p.filled >= 6
    d = np.arange(2 * 3 * K, dtype=np.float64).reshape(2, 3, K)
    i = np.arange(2 * 3 * K, dtype=np.int64).reshape(2, 3, K)
    # ascending merges: the oracle of the descending one on negated values (knn_ip_ref.topk_merge_ip orders by (-v, id))
    for (gD, gI), src in ((got[0], d), (got[1], d.astype(np.float32))):
        oD, oI = knn_ip_ref.topk_merge_ip(-src.astype(np.float64), i, K)
        assert np.array_equal(gI, oI) and np.array_equal(gD, -oD)
    oD, oI = knn_ip_ref.topk_merge_ip(d[..., ::-1], i, K)
    assert np.array_equal(got[2][1], oI) and np.array_equal(got[2][0], oD)
