"""The fixed list of kNN calls whose NATIVE call sequence is recorded (tools/knn_call_probe.py, once, at the parent of the commit
that put the Python layer behind one route planner and two call builders) and replayed (tests/test_knn_calls_gpu.py).

A record is the ordered list of `ac_knn_*` / `ac_topk_merge*` calls a case makes, workspace planners included; per call one line:
the entry name (without `ac_`) and every argument: integers as they are, a pointer as `name+byte offset` of the caller-supplied
tensor it points into, `fresh` for a buffer the wrapper allocated, `NULL` for a null pointer, `out` for a host out-parameter.
The case functions RETURN what their calls returned, in call order (tests/test_poison_knn_gpu.py compares the results; the record
does not depend on it).  D = 8 and k = 4 throughout; 3 and 70 queries; stores of 300, 65535 / 65536 (the library's batch limit) and 2^18 rows (the index's plane rule)."""
import ctypes

import numpy as np
import torch

D, K = 8, 4
N_SMALL, N_BATCH, N_PLANE = 300, 65536, 1 << 18
R_L2, R_IP = 0.1, 0.95            # unit rows and queries: ip > 0.95 <=> squared distance < 0.1


class Recorder:
    """pass-through recorders on every `ac_knn_*` / `ac_topk_merge*` attribute of the loaded library"""

    def __init__(self, nv):
        self.L = nv.lib()
        self.calls, self.named = None, lambda: {}
        self._orig = {n: getattr(self.L, n) for n in nv.exported_symbols() if n.startswith(("ac_knn_", "ac_topk_merge"))}

    def __enter__(self):
        for name, fn in self._orig.items():
            setattr(self.L, name, self._wrap(name, fn))
        return self

    def __exit__(self, *exc):
        for name, fn in self._orig.items():
            setattr(self.L, name, fn)

    def _wrap(self, name, fn):
        def call(*args):
            if self.calls is not None:
                self.calls.append(" ".join([name[3:]] + [str(self._arg(t, a)) for t, a in zip(fn.argtypes, args)]))
            return fn(*args)
        return call

    def _arg(self, ctype, a):
        if ctype is ctypes.c_void_p:
            addr = a.value if isinstance(a, ctypes.c_void_p) else a
            if not addr:
                return "NULL"
            for name, t in self.named().items():
                if t is None:
                    continue
                base = t.untyped_storage().data_ptr()
                if base <= addr < base + max(t.untyped_storage().nbytes(), 1):
                    return f"{name}+{addr - base}"
            return "fresh"
        if not issubclass(ctype, ctypes._SimpleCData):
            return "out"
        return int(a)

    def record(self, fn, env):
        """the native calls of fn(env) and the exception type it ended with (None = returned)"""
        self.calls, raised = [], None
        try:
            fn(env)
            torch.cuda.synchronize()
        except Exception as e:                     # noqa: BLE001  (the outcome is part of the record)
            raised = type(e).__name__
        calls, self.calls = self.calls, None
        return {"calls": calls, "raised": raised}


class Env:
    """the tensors every case shares; `names` = the caller-supplied tensors of the running case"""

    def __init__(self, ix, dev, rec):
        self.ix, self.dev, self.rec = ix, dev, rec
        self.P = ix.synth_unit_rows(N_PLANE, D, 7, device=dev)
        self.Q = ix.synth_unit_rows(70, D, 9, device=dev)
        self.Q3, self.Q0 = self.Q[:3], self.Q[:0]
        self.prep = ix.prepare_store(self.P, N_BATCH, D)
        self.sel = ix.RowSelector.from_mask(np.arange(N_PLANE + 128) % 3 != 0, device=dev)      # dense, count known
        self.ids5 = torch.tensor([3, 10, 11, 200, 299], dtype=torch.int64, device=dev)
        self.ws = torch.empty(64 << 20, dtype=torch.uint8, device=dev)
        self.stats = torch.zeros(4, dtype=torch.int32, device=dev)
        self.out = (torch.empty((70, K), dtype=torch.float32, device=dev), torch.empty((70, K), dtype=torch.int64, device=dev))
        self.ex = torch.empty((70, K), dtype=torch.float64, device=dev)
        self.rad = {"l2": torch.full((70,), R_L2, device=dev), "ip": torch.full((70,), R_IP, device=dev)}
        # workspace limits under which 70 queries go in three chunks (30 + 30 + 10): 30 one-query workspaces hold 30 queries
        self.chunk_ws = 30 * ix.knn_range_workspace_bytes(N_SMALL, D, 1)
        self.chunk_ws_batch = 30 * ix.knn_range_batch_workspace_bytes(N_BATCH, D, 1)
        self.base = {"P": self.P, "Q": self.Q, "planes": self.prep[0], "norms": self.prep[1], "sel": self.sel.words, "ids": self.ids5,
                     "ws": self.ws, "stats": self.stats, "outD": self.out[0], "outI": self.out[1], "ex": self.ex,
                     "rad_l2": self.rad["l2"], "rad_ip": self.rad["ip"]}
        self.obj, self._sels = None, {}
        rec.named = self.names

    def sel_for(self, n):
        """a dense selector (count known) over exactly n rows, named `sel<n>` in the records"""
        if n not in self._sels:
            self._sels[n] = self.ix.RowSelector.from_mask(np.arange(n) % 3 != 0, device=self.dev)
            self.base[f"sel{n}"] = self._sels[n].words
        return self._sels[n]

    def names(self):
        d = dict(self.base)
        o = self.obj
        if o is not None:
            prepared = o._prepared or (None, None)
            d.update({"o.store": getattr(o, "_store", None), "o.ws": o._ws, "o.stats": getattr(o, "_stats", None),
                      "o.range_stats": getattr(o, "_range_stats", None), "o.planes": prepared[0], "o.norms": prepared[1]})
        return d

    def index(self, metric, n):
        ix = self.ix
        idx = (ix.HipFlatIPIndex if metric == "ip" else ix.HipFlatL2Index)(D, device=self.dev)
        idx.add_device_rows(self.P[:n].clone())
        self.obj = idx
        return idx

    def radius(self, metric):
        return R_IP if metric == "ip" else R_L2


def _topk(env, metric):
    return env.ix.knn_ip_topk if metric == "ip" else env.ix.knn_l2_topk


def _exact(env, metric):
    return env.ix.knn_ip_topk_exact if metric == "ip" else env.ix.knn_l2_topk_exact


CASES = []


def case(name):
    def deco(fn):
        CASES.append((name, fn))
        return fn
    return deco


def _wrappers(m):
    """(name, call) of the functional wrappers' cases for metric m"""
    topk, exact = (lambda e: _topk(e, m)), (lambda e: _exact(e, m))
    sel, ids = (lambda e: e.ix.knn_topk_sel), (lambda e: e.ix.knn_topk_ids)          # (looked up on the module at call time)
    rng, rids = (lambda e: e.ix.knn_range_search), (lambda e: e.ix.knn_range_ids)
    ours = lambda e: dict(workspace=e.ws, stats=e.stats, exact_out=e.ex)          # noqa: E731  (the caller's buffers)
    return [
        (f"topk_{m}_300_q3", lambda e: topk(e)(e.P, N_SMALL, D, e.Q3, K)),
        (f"topk_{m}_300_q70_caller_buffers", lambda e: topk(e)(e.P, N_SMALL, D, e.Q, K, row_offset=5, out=e.out, **ours(e))),
        (f"topk_{m}_65535_prepared_falls_back", lambda e: topk(e)(e.P, N_BATCH - 1, D, e.Q3, K, prepared=e.prep)),
        (f"topk_{m}_65536_prepared_q3", lambda e: topk(e)(e.P, N_BATCH, D, e.Q3, K, prepared=e.prep)),
        (f"topk_{m}_65536_prepared_q70_caller_buffers",
         lambda e: topk(e)(e.P, N_BATCH, D, e.Q, K, row_offset=5, out=e.out, prepared=e.prep, **ours(e))),
        (f"topk_{m}_65536_no_plane_q70", lambda e: topk(e)(e.P, N_BATCH, D, e.Q, K)),
        (f"topk_exact_{m}_300", lambda e: exact(e)(e.P, N_SMALL, D, e.Q3, K, row_offset=7)),
        (f"topk_exact_{m}_65536_prepared", lambda e: exact(e)(e.P, N_BATCH, D, e.Q, K, workspace=e.ws, stats=e.stats, prepared=e.prep)),
        (f"topk_{m}_no_queries", lambda e: topk(e)(e.P, N_SMALL, D, e.Q0, K)),
        (f"topk_{m}_no_rows", lambda e: topk(e)(e.P, 0, D, e.Q3, K)),
        (f"sel_{m}_300_bit0", lambda e: sel(e)(e.P, N_SMALL, D, e.Q3, K, e.sel, metric=m)),
        (f"sel_{m}_300_bit64_words_exact",
         lambda e: sel(e)(e.P, N_SMALL, D, e.Q, K, e.sel.words, metric=m, sel_bit0=64, row_offset=64, out=e.out, **ours(e))),
        (f"sel_{m}_65536_prepared_q3", lambda e: sel(e)(e.P, N_BATCH, D, e.Q3, K, e.sel, metric=m, prepared=e.prep)),
        (f"sel_{m}_65536_prepared_q70_bit64",
         lambda e: sel(e)(e.P, N_BATCH, D, e.Q, K, e.sel, metric=m, sel_bit0=64, row_offset=64, prepared=e.prep, **ours(e))),
        (f"sel_{m}_65535_prepared_falls_back", lambda e: sel(e)(e.P, N_BATCH - 1, D, e.Q3, K, e.sel, metric=m, prepared=e.prep)),
        (f"sel_{m}_no_queries", lambda e: sel(e)(e.P, N_SMALL, D, e.Q0, K, e.sel, metric=m)),
        (f"ids_{m}_300", lambda e: ids(e)(e.P, N_SMALL, D, e.Q3, K, e.ids5, metric=m)),
        (f"ids_{m}_65536_exact_caller_buffers",
         lambda e: ids(e)(e.P, N_BATCH, D, e.Q, K, e.ids5, metric=m, row_offset=9, out=e.out, exact_out=e.ex)),
        (f"ids_{m}_empty_list", lambda e: ids(e)(e.P, N_SMALL, D, e.Q3, K, e.ids5[:0], metric=m)),
        (f"range_{m}_300_scalar", lambda e: rng(e)(e.P, N_SMALL, D, e.Q3, e.radius(m), metric=m)),
        (f"range_{m}_300_per_query_exact_stats",
         lambda e: rng(e)(e.P, N_SMALL, D, e.Q, e.rad[m], metric=m, row_offset=5, exact_out=True, stats=e.stats)),
        (f"range_{m}_300_chunked", lambda e: rng(e)(e.P, N_SMALL, D, e.Q, e.radius(m), metric=m, max_ws_bytes=e.chunk_ws)),
        (f"range_{m}_300_sel_bit64", lambda e: rng(e)(e.P, N_SMALL, D, e.Q3, e.radius(m), metric=m, sel=e.sel, sel_bit0=64, row_offset=64)),
        (f"range_{m}_65536_prepared", lambda e: rng(e)(e.P, N_BATCH, D, e.Q3, e.radius(m), metric=m, prepared=e.prep, stats=e.stats)),
        (f"range_{m}_65536_prepared_sel_chunks_exact",
         lambda e: rng(e)(e.P, N_BATCH, D, e.Q, e.rad[m], metric=m, exact_out=True, sel=e.sel.words, prepared=e.prep,
                          max_ws_bytes=e.chunk_ws_batch)),
        (f"range_{m}_65535_prepared_falls_back", lambda e: rng(e)(e.P, N_BATCH - 1, D, e.Q3, e.radius(m), metric=m, prepared=e.prep)),
        (f"range_{m}_no_queries", lambda e: rng(e)(e.P, N_SMALL, D, e.Q0, e.radius(m), metric=m, exact_out=True)),
        (f"range_{m}_no_rows", lambda e: rng(e)(e.P, 0, D, e.Q3, e.radius(m), metric=m)),
        (f"range_ids_{m}_scalar", lambda e: rids(e)(e.P, N_SMALL, D, e.Q3, e.radius(m), e.ids5, metric=m)),
        (f"range_ids_{m}_per_query_exact_stats",
         lambda e: rids(e)(e.P, N_BATCH, D, e.Q, e.rad[m], e.ids5, metric=m, row_offset=9, exact_out=True, stats=e.stats)),
        (f"range_ids_{m}_no_queries", lambda e: rids(e)(e.P, N_SMALL, D, e.Q0, e.radius(m), e.ids5, metric=m)),
    ]


# The metric reaches the marshalling in two places only, the entry's name and the prepared-store workspace planner: every wrapper
# case runs for L2, for IP the two below; the index and sharded sequences further down reach every IP entry.
IP_WRAPPER_CASES = ("topk_ip_65536_prepared_q70_caller_buffers", "range_ip_65536_prepared_sel_chunks_exact")
CASES += _wrappers("l2") + [c for c in _wrappers("ip") if c[0] in IP_WRAPPER_CASES]


# ---- stores and merges ------------------------------------------------------------------------------------------------------------
@case("store_functions")
def _store_functions(e):
    ix = e.ix
    ix.store_buffers_sizes(N_BATCH, D)
    ix.store_buffers(N_BATCH, D, e.dev)
    prepared = ix.prepare_store(e.P, N_BATCH, D, capacity=N_BATCH + 1000)
    ok = ix.update_store(e.P, N_BATCH, N_BATCH + 10, D, prepared, N_BATCH, 10)
    return [prepared, ok, ix.prepare_store(e.P, N_SMALL, D)]


@case("merges")
def _merges(e):
    ix = e.ix
    d = torch.arange(2 * 3 * K, dtype=torch.float64, device=e.dev).reshape(2, 3, K)
    i = torch.arange(2 * 3 * K, dtype=torch.int64, device=e.dev).reshape(2, 3, K)
    return [ix.topk_merge(d, i), ix.topk_merge(d.to(torch.float32), i), ix.topk_merge_ip(d.flip(-1), i)]


# ---- the index methods ------------------------------------------------------------------------------------------------------------
def _index_small(e, metric):
    idx = e.index(metric, N_SMALL)
    return [
        idx.search_device(e.Q3, K),
        idx.search_device(e.Q, K),
        idx.search_device(e.Q3, K, sel=[3, 10, 11, 200, 299]),
        idx.search_device(e.Q3, K, sel=np.arange(N_SMALL) % 3 != 0),
        idx.range_search_device(e.Q3, e.radius(metric)),
        idx.range_search_device(e.Q, e.rad[metric], sel=np.arange(N_SMALL) % 3 != 0),
        idx.range_search_device(e.Q3, e.radius(metric), sel=[3, 10, 11, 200, 299]),
        idx.range_search_device(e.Q, e.radius(metric), max_ws_bytes=e.chunk_ws),
    ]


def _index_batch_limit(e, metric):
    idx = e.index(metric, N_BATCH)
    return [
        idx.search_device(e.Q3, K),
        idx.search_device(e.Q3, K),                  # below PLANE_MIN_ROWS: no plane from small searches
        idx.search_device(e.Q, K),                   # 70 x 65536 pairs: below BATCH_MIN_PAIRS
        idx.search_device(e.Q, K, sel=e.sel_for(N_BATCH)),
        idx.range_search_device(e.Q3, e.radius(metric)),
    ]


def _index_plane(e, metric):
    ix = e.ix
    idx = e.index(metric, N_PLANE)
    dense = e.sel_for(N_PLANE)
    res = [
        idx.search_device(e.Q3, K),
        idx.search_device(e.Q3, K),                  # the L2 index prepares here; the IP index never from small searches
        idx.search_device(e.Q3, K, sel=dense),
    ]
    if idx._prepared is None:
        idx.prepare_plane() if hasattr(idx, "prepare_plane") else _prepare_from_outside(ix, idx)
    res += [
        idx.search_device(e.Q3, K),
        idx.search_device(e.Q3, K, sel=dense),
        idx.search_device(e.Q3, K, sel=ix.RowSelector(dense.words, N_PLANE)),                # unknown count
        idx.search_device(e.Q3, K, sel=[3, 10, 11, 200, 299]),
        idx.range_search_device(e.Q3, e.radius(metric)),
        idx.range_search_device(e.Q3, e.rad[metric][:3], sel=dense),
        idx.range_search_device(e.Q3, e.radius(metric), sel=[3, 10, 11, 200, 299]),
    ]
    idx.add(e.P[:5, :D])                             # the plane follows the append
    idx.update_rows([1, 2, 3, 9], e.P[10:14, :D])
    res.append(idx.search_device(e.Q3, K))
    idx.remove_ids([0])                              # compaction drops the plane
    res.append(idx.search_device(e.Q3, K))
    res.append(idx.range_search_device(e.Q3, e.radius(metric)))
    return res


def _prepare_from_outside(ix, idx):
    """what `PrototypeMemory.load_rows(prepare=True)` did before the index had `prepare_plane()`"""
    if idx.ntotal >= ix.BATCH_MIN_ROWS:
        idx._prepared = ix.prepare_store(idx._store, idx.ntotal, idx.d)
        idx._searches_since_change = 1


def _sharded(e, metric):
    from adaptive_classifier.sharded import ShardedSearch
    off = 64
    ss = ShardedSearch(e.P, N_PLANE, D, off, metric=metric)
    e.obj = ss
    res = [
        ss.search(e.Q3, K),                          # the sharded search prepares wherever batch_applies(auto=True) holds
        ss.search(e.Q, K),
        ss.search(e.Q3, K, sel=e.sel),               # the global selector: N_PLANE + 128 rows, known dense
        ss.range_search(e.Q3, e.radius(metric)),
        ss.range_search(e.Q3, e.rad[metric][:3], sel=e.sel),
    ]
    small = ShardedSearch(e.P, N_SMALL, D, off, metric=metric)
    e.obj = small
    return res + [small.search(e.Q3, K, sel=e.sel), small.range_search(e.Q3, e.radius(metric), sel=e.sel)]


case("index_l2_300")(lambda e: _index_small(e, "l2"))
case("index_l2_65536")(lambda e: _index_batch_limit(e, "l2"))
for _m in ("l2", "ip"):
    case(f"index_{_m}_2p18")(lambda e, m=_m: _index_plane(e, m))
    case(f"sharded_{_m}_world1")(lambda e, m=_m: _sharded(e, m))

NAMES = [n for n, _ in CASES]


def run_all(nv, ix, dev, only=None):
    """{case name: record} of every case (or of the cases named in `only`)"""
    out = {}
    with Recorder(nv) as rec:
        env = Env(ix, dev, rec)
        for name, fn in CASES:
            if only is None or name in only:
                env.obj = None
                out[name] = rec.record(fn, env)
    return out
