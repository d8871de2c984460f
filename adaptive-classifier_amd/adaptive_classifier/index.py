"""HipFlatL2Index: the `faiss.IndexFlatL2` protocol used by memory.py, on MI355X HBM.

Protocol kept (reference call sites in /root/reference/src/adaptive_classifier/memory.py):
  IndexFlatL2(d) :34,164,182,242 | .add(x[n,d]) :159,172,190 | .search(x[nq,d], k) :114 |
  .remove_ids(ids) :158 (compacting) | .ntotal :106,113

Rows live in one resident, row-major fp32 device matrix with a 16-byte aligned, zero padded
leading dimension (growth by doubling, so `add` is amortised O(1) like faiss's vector).
search() is exact squared L2, ascending, ties to the lower id; HipFlatIPIndex is the same store searched by inner product
(faiss.IndexFlatIP: descending, ties to the lower id); the reference itself never builds one.  search(x, k, sel=...) is the FILTERED
search (faiss SearchParameters(sel=IDSelector...)): the k best among the rows a `RowSelector` names; range_search() is faiss
range_search (every row within a radius), filtered by `sel=` likewise.  Both metrics share one prepared store (one fp16 plane +
norms, `prepare_store`).  Every search is one of three routes, chosen by `plan_topk` / `plan_range` (below) from what the host
knows -- no bitmap is ever read back to choose:

  route  | taken by                                            | top-k entry (`ac_knn_{l2,ip}_`)  | range entries (count; fill)
  -------+-----------------------------------------------------+----------------------------------+------------------------------------
  ids    | a selector carrying <= KNN_IDS_MAX host ids         | topk_ids                         | range_count_ids; range_fill_ids
  plane  | `batch_applies(auto=True)` (a selection: KNOWN to   | topk_batch, topk_batch_sel       | range_count_batch[_sel]; range_fill
         | hold >= 1 / SEL_BATCH_MAX_SPARSITY of the rows)     |                                  |   (a plane that exists, from
         | and a plane exists or may be prepared now           |                                  |   PLANE_MIN_ROWS rows on)
  rows   | everything else, an unknown count included          | topk_x, topk_sel                 | range_count[_sel]; range_fill

Who prepares a plane that does not exist (from BATCH_MIN_QUERIES queries on: every top-k search that takes the plane route):
  HipFlatL2Index.search, unfiltered       | small batches too, once the rows have served one search since they last changed
  HipFlatIPIndex.search; any search(sel=) | never from small batches: they only use a plane that exists
  ShardedSearch, unfiltered               | always (sized for the shard's rows; the indexes size it for the store's capacity)
  any range search; the functional API    | never (`knn_*_topk(prepared=)` / `knn_range_search(prepared=)` use the CALLER's plane
                                          | wherever the library takes it, and fall back to the fp32 entry elsewhere)
"""
import ctypes

import numpy as np
import torch

from collections import namedtuple

from . import _native as nv

# ---- the route planner: pure host code (integers in, a decision out; no tensor, no native call) -----------------------------------
# Every caller -- the flat indexes, the row-sharded search, the functional wrappers -- states the facts and keeps only what is its
# own: who owns the plane, the workspace, the stats tensor, the row offset.  The constants are read when a route is planned.
#
# Where the prepared-store paths apply (library limits: N >= 65536, k <= 100) and pay.
#   >= 64 queries: the GEMM-form proposal sweep (knn_batch_sweep); its fixed cost (sample stages, thresholds, query plane, a deeper
#      merge: ~0.3 ms) beats the fp32 sweep from ~20 M query-row pairs on (measured, round 3, fp32 sweep vs batched: 256 x 100k 0.56
#      vs 0.39 ms inside the predict step; 1024 x 2M x 1024 56 vs 6.5 ms; 4096 x 10M 552 vs 78 ms)
#   1 .. 63 queries (round 4): ONE bandwidth-bound pass over the fp16 plane with the query tile resident (knn_plane_sweep): half
#      the bytes of the fp32 sweep; pays once the sweep, not the launch chain, is what a search costs (PLANE_MIN_ROWS)
BATCH_MIN_QUERIES, BATCH_MIN_ROWS, BATCH_MAX_K, BATCH_MIN_PAIRS = 64, 65536, 100, 2.0e7
PLANE_MIN_ROWS = 1 << 18
KNN_IDS_MAX = 8192       # rows the id-list route covers (include/acamd.h: ac_knn_*_topk_ids)
# The filtered search takes the prepared store only for a selection KNOWN to hold at least 1 / 32 of the rows: the thresholds of
# the prepared-store sweeps come from selected rows only -- stage A samples >= 128 k' rows, a two-phase round sees 256 tiles of 256
# rows -- and at density 1 / 32 both still see >= 4 k' selected rows, the planner's own margin.  Sparser, the thresholds may stay
# +inf; a store with more selected rows than the candidate buffer holds then overflows it and every query is redone in fp64 (exact,
# but slower than the fp32 route).  Measured at 256 x 1M x 768 (profiles/knn_select/README.md): no query takes the fallback at
# 1/32 -- nor at 1 %, where the 10 159 selected rows still fit the buffer; the fraction stays at the planner's margin.
SEL_BATCH_MAX_SPARSITY = 32

# When a top-k search that would take the plane, has fewer than BATCH_MIN_QUERIES queries and finds no plane may prepare one (two
# passes over the rows, 2 B per element; from BATCH_MIN_QUERIES queries on preparing pays within the call: every policy prepares):
PREPARE_SECOND_SEARCH = "second search"            # once the rows have served a search since they last changed (L2 index, unfiltered)
PREPARE_NEVER_SMALL = "never from small batches"   # small batches only use a plane that exists (IP index; every filtered search)
PREPARE_ALWAYS = "always"                          # wherever batch_applies(auto=True) holds (the unfiltered sharded search)

# What the host knows of a row selection: ids = the length of its host id list (None: it has none), count = its known number of
# selected rows (None: unknown -- it is never read back to choose a route), total = the rows it covers (None: the searched rows; a
# row shard passes the GLOBAL count over the GLOBAL rows).
Selection = namedtuple("Selection", "ids count total")
# kind: "ids" (the id-list entries), "plane" (the prepared-store entries) or "rows" (the fp32 rows); prepare: build the plane first
Route = namedtuple("Route", "kind prepare")


def batch_applies(N, nq, k, auto=False):
    """Library limits of ac_knn_l2_topk_batch / ac_knn_ip_topk_batch (any number of queries: below 64 they run the fp16-plane
    sweep); auto=True adds the size heuristic the index uses to pick a path."""
    ok = nq >= 1 and N >= BATCH_MIN_ROWS and k <= BATCH_MAX_K
    if not ok or not auto:
        return ok
    return float(N) * nq >= BATCH_MIN_PAIRS if nq >= BATCH_MIN_QUERIES else N >= PLANE_MIN_ROWS


def sel_batch_applies(N, nq, k, count, total=None):
    """the routing rule of the filtered search: the prepared-store route for a selection whose size is known on the host and
    dense enough (count * SEL_BATCH_MAX_SPARSITY >= total rows; total defaults to N -- a row shard passes the global figures)
    where `batch_applies(N, nq, k, auto=True)` holds"""
    total = N if total is None else total
    return count is not None and int(count) * SEL_BATCH_MAX_SPARSITY >= int(total) and batch_applies(N, nq, k, auto=True)


def _takes_id_list(sel):
    return sel is not None and sel.ids is not None and sel.ids <= KNN_IDS_MAX


def plan_topk(n, nq, k, sel=None, have_plane=False, searches=0, policy=PREPARE_NEVER_SMALL, auto=True):
    """Route of a top-k search of nq queries over n (local) rows.  sel: None or the `Selection` facts; have_plane: a prepared plane
    exists; searches: searches served since the rows last changed; policy: one of PREPARE_*.
    auto=False is the functional API (`knn_l2_topk(..., prepared=)` and its kin): the caller's plane wherever the library takes it
    (`batch_applies` without the size heuristic, at any density of the selection), and nothing is ever prepared."""
    if _takes_id_list(sel):
        return Route("ids", False)
    if not auto:
        return Route("plane" if have_plane and batch_applies(n, nq, k) else "rows", False)
    pays = batch_applies(n, nq, k, auto=True) if sel is None else sel_batch_applies(n, nq, k, sel.count, sel.total)
    if not pays:
        return Route("rows", False)
    if have_plane:
        return Route("plane", False)
    prepare = nq >= BATCH_MIN_QUERIES or policy == PREPARE_ALWAYS or (policy == PREPARE_SECOND_SEARCH and searches >= 1)
    return Route("plane" if prepare else "rows", prepare)


def plan_range(n, have_plane, batch_ok, sel=None, auto=True):
    """Route of a range search over n (local) rows: "ids", "plane" (the COUNT reads the plane) or "rows".  A range search never
    prepares.  batch_ok: whether `range_batch_applies` holds -- the library's verdict on (N, D, nq); a caller that only hands
    the plane on to `knn_range_search`, which asks the library, passes True.  auto=True adds the rule of the index and the sharded
    search: a plane is used from PLANE_MIN_ROWS rows on."""
    if _takes_id_list(sel):
        return "ids"
    return "plane" if have_plane and batch_ok and (not auto or n >= PLANE_MIN_ROWS) else "rows"


# ---- the native calls ----------------------------------------------------------------------------------------------------------------

def _planned_bytes(entry, *shape, outs=1):
    """a host-only planner of the library, entry(*shape, &bytes ...): the byte count(s) it reports"""
    b = [ctypes.c_size_t(0) for _ in range(outs)]
    nv.check(getattr(nv.lib(), entry)(*shape, *map(ctypes.byref, b)), entry)
    return b[0].value if outs == 1 else tuple(x.value for x in b)


def knn_workspace_bytes(N, D, nq, k):
    return _planned_bytes("ac_knn_l2_topk_workspace", N, D, nq, k)


def knn_batch_workspace_bytes(N, D, nq, k):
    return _planned_bytes("ac_knn_l2_topk_batch_workspace", N, D, nq, k)


def store_buffers_sizes(rows, D):
    """(plane elements, norm elements) a prepared store of `rows` rows occupies"""
    pb, nb = _planned_bytes("ac_knn_store_bytes", rows, D, outs=2)
    return pb // 2, nb // 4


def store_buffers(rows, D, device):
    """Empty (plane int16, norms fp32) buffers of a prepared store of up to `rows` rows (`ac_knn_store_bytes`)."""
    pe, ne = store_buffers_sizes(rows, D)
    return torch.empty(pe, dtype=torch.int16, device=device), torch.empty(ne, dtype=torch.float32, device=device)


def update_store(P, n_old, n_new, D, prepared, row0, nrows):
    """`ac_knn_update_store`: rows [row0, row0 + nrows) of P changed / were appended.  Returns True when the prepared store is
    ready again, False when the new rows moved the store's power-of-two scale (every plane entry is stale: prepare anew).
    Reads a 4-byte verdict back (one stream sync per update)."""
    planes, norms = prepared
    flag = torch.zeros(1, dtype=torch.int32, device=P.device)
    with torch.cuda.device(P.device):
        nv.check(nv.lib().ac_knn_update_store(nv.ptr(P), n_old, n_new, P.stride(0), D, nv.ptr(planes), nv.ptr(norms), row0, nrows,
                                              nv.ptr(flag), nv.stream_ptr(P.device)), "ac_knn_update_store")
    return int(flag.item()) == 0


def prepare_store(P, N, D, capacity=None):
    """(plane, norms) of the first N rows of the store P for the batched search (`ac_knn_prepare_store`): one fp16
    operand plane + |p|^2 per row.  Costs two passes over the rows and 2 B per element.  After rows change: `update_store`
    (appended / overwritten rows) or prepare anew.  capacity: size the buffers for that many rows (stores that grow)."""
    nv.require_gpu()
    planes, norms = store_buffers(max(N, capacity or 0), D, P.device)
    with torch.cuda.device(P.device):
        nv.check(nv.lib().ac_knn_prepare_store(nv.ptr(P), N, P.stride(0), D, nv.ptr(planes), nv.ptr(norms),
                                               nv.stream_ptr(P.device)), "ac_knn_prepare_store")
    return planes, norms


def _check_rows_queries(P, Q, metric):
    """what every kNN entry asks of its rows and queries (and fails loudly without a GPU)"""
    nv.require_gpu()
    assert metric in ("l2", "ip")
    assert P.dtype == torch.float32 and Q.dtype == torch.float32 and P.is_cuda and Q.is_cuda
    assert P.stride(1) == 1 and Q.stride(1) == 1


def _sel_args(sel, sel_bit0, N):
    """(d_sel, sel_bit0) of a RowSelector / its words tensor; ValueError unless it covers rows [sel_bit0, sel_bit0 + N)"""
    words = sel.words if isinstance(sel, RowSelector) else sel
    assert words.dtype == torch.int64 and words.is_cuda and words.is_contiguous()
    if int(sel_bit0) + N > words.numel() * 64:
        raise ValueError(f"selection of {words.numel() * 64} bits does not cover rows [{sel_bit0}, {int(sel_bit0) + N})")
    return nv.ptr(words), int(sel_bit0)


def _ids_args(ids):
    """(d_ids, M) of a `from_ids` RowSelector / a sorted, unique int64 cuda tensor"""
    ids = ids.ids if isinstance(ids, RowSelector) else ids
    assert ids is not None and ids.dtype == torch.int64 and ids.is_cuda and ids.is_contiguous()
    return nv.ptr(ids) if ids.numel() else None, ids.numel()


def _knn_topk(metric, kind, P, N, D, Q, k, row_offset, out, exact_out, workspace=None, stats=None, prepared=None, sel=None, sel_bit0=0,
              ids=None):
    """THE top-k call: ac_knn_{metric}_topk_{x, batch, sel, batch_sel, ids}, by the route `kind` and whether a bitmap is given.
    The argument list is  rows [store] [id list] queries k row_offset [bitmap]  outD outD64 outI  [workspace stats]  stream."""
    _check_rows_queries(P, Q, metric)
    nq, dev = Q.shape[0], Q.device
    head = (nv.ptr(P), N, P.stride(0), D)
    if kind == "plane":
        head += (nv.ptr(prepared[0]), nv.ptr(prepared[1]))
    elif kind == "ids":
        head += _ids_args(ids)
    head += (nv.ptr(Q), nq, Q.stride(0), k, row_offset)
    if sel is not None:
        head += _sel_args(sel, sel_bit0, N)
    if out is None:
        out = (torch.empty((nq, k), dtype=torch.float32, device=dev), torch.empty((nq, k), dtype=torch.int64, device=dev))
    outD, outI = out
    tail = (nv.ptr(outD), nv.ptr(exact_out), nv.ptr(outI))
    if kind == "ids":
        entry = f"ac_knn_{metric}_topk_ids"                  # reads the listed rows only: no workspace, no stats
    else:
        form = ("batch", "batch_sel") if kind == "plane" else ("x", "sel")
        entry = f"ac_knn_{metric}_topk_{form[sel is not None]}"
        # (the planners of the two metrics report the same bytes; which one is asked is kept as it was, call for call)
        need = _planned_bytes("ac_knn_l2_topk_workspace" if kind == "rows" else
                              f"ac_knn_{metric if sel is None else 'l2'}_topk_batch_workspace", N, D, nq, k)
        if workspace is None or workspace.numel() < need:
            workspace = torch.empty(max(need, 256), dtype=torch.uint8, device=dev)
        tail += (nv.ptr(workspace), workspace.numel(), nv.ptr(stats))
    with torch.cuda.device(dev):
        rc = getattr(nv.lib(), entry)(*head, *tail, nv.stream_ptr(dev))
    nv.check(rc, entry)
    return outD, outI


def knn_l2_topk(P, N, D, Q, k, row_offset=0, out=None, workspace=None, stats=None, exact_out=None, prepared=None):
    """Low-level device call.  P: [>=N, ldP] fp32 cuda tensor, Q: [nq, >=D] fp32 cuda tensor.

    Returns (dist fp32 [nq,k], ids int64 [nq,k]) on the same device.  Asynchronous.
    exact_out: optional float64 [nq,k] cuda tensor that receives the exact fp64 distances (shard merges).
    prepared: optional (planes, norms) from `prepare_store`: the search then proposes from the store's fp16 plane
              (`ac_knn_l2_topk_batch`: one bandwidth-bound pass for < 64 queries, the GEMM-form sweep on the matrix pipe from 64
              on) -- same exact result, half the bytes / several times the throughput.  Outside `batch_applies(N, nq, k)` the
              fp32 entry (`ac_knn_l2_topk_x`) is called as without it.
    """
    kind = plan_topk(N, Q.shape[0], k, have_plane=prepared is not None, auto=False).kind
    return _knn_topk("l2", kind, P, N, D, Q, k, row_offset, out, exact_out, workspace, stats, prepared)


def knn_ip_topk(P, N, D, Q, k, row_offset=0, out=None, workspace=None, stats=None, exact_out=None, prepared=None):
    """Exact inner-product top-k (`ac_knn_ip_topk_x`, faiss.IndexFlatIP.search): the k rows with the largest p.q per query,
    descending, ties to the lower id; rows need not be normalised.  Arguments and workspace as `knn_l2_topk`, `prepared`
    included: the SAME (planes, norms) of `prepare_store` serve both metrics (`ac_knn_ip_topk_batch`, same exact result).
    Returns (values fp32 [nq,k], ids int64 [nq,k]); k > N pads with (-FLT_MAX, -1)."""
    kind = plan_topk(N, Q.shape[0], k, have_plane=prepared is not None, auto=False).kind
    return _knn_topk("ip", kind, P, N, D, Q, k, row_offset, out, exact_out, workspace, stats, prepared)


def _topk_exact(search, P, N, D, Q, k, row_offset, workspace, stats, prepared):
    ex = torch.empty((Q.shape[0], k), dtype=torch.float64, device=Q.device)
    _, I = search(P, N, D, Q, k, row_offset=row_offset, workspace=workspace, stats=stats, exact_out=ex, prepared=prepared)
    return ex, I


def knn_l2_topk_exact(P, N, D, Q, k, row_offset=0, workspace=None, stats=None, prepared=None):
    """(exact fp64 dist [nq,k], ids [nq,k]): what a row shard contributes to a sharded search."""
    return _topk_exact(knn_l2_topk, P, N, D, Q, k, row_offset, workspace, stats, prepared)


def knn_ip_topk_exact(P, N, D, Q, k, row_offset=0, workspace=None, stats=None, prepared=None):
    """(exact fp64 inner products [nq,k] descending, ids [nq,k]): what a row shard contributes to a sharded IP search."""
    return _topk_exact(knn_ip_topk, P, N, D, Q, k, row_offset, workspace, stats, prepared)


def _sel_words(n):
    return max((int(n) + 63) // 64, 1)


def _pack_host(mask):
    """bool [n] -> int64 words [ceil(n / 64)] (>= 1 word), bit r % 64 of word r / 64, bit 0 the least significant: numpy's
    little-endian bit order IS the layout (faiss IDSelectorBitmap); the tail bits of the last word are zero"""
    mask = np.ascontiguousarray(mask, dtype=bool).reshape(-1)
    raw = np.packbits(mask, bitorder="little")
    buf = np.zeros(_sel_words(mask.size) * 8, dtype=np.uint8)
    buf[: raw.size] = raw
    return buf.view("<i8").astype(np.int64, copy=False)


class RowSelector:
    """Which rows of a flat store a FILTERED search may return (faiss IDSelectorBitmap / IDSelectorBatch / IDSelectorRange).

    words: int64 tensor, the packed bitmap (`ac_knn_*_topk_sel`'s d_sel: row r = bit r % 64 of word r / 64, bit 0 the least
    significant); n: the rows it covers; ids: the sorted, unique int64 row ids when it was built from a host id list (else None)
    -- a selector of <= KNN_IDS_MAX ids is searched through the id-list route; known_count: the number of selected rows when the
    host knows it -- for free when the selector is built from host data, else after `count()` -- or None (the index then keeps a
    bitmap search on the fp32 rows: it never reads a bitmap back to pick a route).  Host inputs are packed with
    numpy.packbits(bitorder="little") and uploaded (to `device`; without one and without a GPU they stay on the host); device
    inputs are packed by `ac_knn_sel_pack` / `ac_knn_sel_classes` without any host synchronisation."""

    def __init__(self, words, n, ids=None, count=None):
        self.words, self.n, self.ids = words, int(n), ids
        self.known_count = None if count is None else int(count)

    @staticmethod
    def _upload(t, device):
        if device is None and torch.cuda.is_available():
            device = f"cuda:{torch.cuda.current_device()}"
        return t if device is None else t.to(device)

    @classmethod
    def from_mask(cls, mask, device=None):
        """mask: bool tensor / array [n]; True = selected"""
        if isinstance(mask, torch.Tensor) and mask.is_cuda:
            m = mask.detach().reshape(-1).to(torch.uint8).contiguous()
            n = m.numel()
            words = torch.empty(_sel_words(n), dtype=torch.int64, device=m.device)
            if n == 0:
                words.zero_()
            with torch.cuda.device(m.device):
                nv.check(nv.lib().ac_knn_sel_pack(nv.ptr(m), n, nv.ptr(words), nv.stream_ptr(m.device)), "ac_knn_sel_pack")
            return cls(words, n)
        m = mask.detach().cpu().numpy() if isinstance(mask, torch.Tensor) else np.asarray(mask)
        m = m.reshape(-1).astype(bool)
        return cls(cls._upload(torch.from_numpy(_pack_host(m)), device), m.size, count=int(m.sum()))

    @classmethod
    def from_ids(cls, ids, n, device=None):
        """ids: row ids in any order, duplicates allowed; ids outside [0, n) are dropped.  A host list is sorted and
        de-duplicated and kept next to the bitmap (the id-list route); a device tensor becomes a bitmap only (sorting it would
        need a host read of the unique count)."""
        n = int(n)
        if isinstance(ids, torch.Tensor) and ids.is_cuda:
            i = ids.detach().reshape(-1).to(torch.int64)
            m = torch.zeros(n + 1, dtype=torch.uint8, device=i.device)
            m[torch.where((i >= 0) & (i < n), i, torch.full_like(i, n))] = 1      # out-of-range ids land in the spare slot
            return cls.from_mask(m[:n])
        i = ids.detach().cpu().numpy() if isinstance(ids, torch.Tensor) else np.asarray(ids)
        i = np.unique(i.reshape(-1).astype(np.int64))
        i = i[(i >= 0) & (i < n)]
        m = np.zeros(n, dtype=bool)
        m[i] = True
        return cls(cls._upload(torch.from_numpy(_pack_host(m)), device), n, cls._upload(torch.from_numpy(i), device), count=i.size)

    @classmethod
    def from_range(cls, lo, hi, n, device=None):
        """rows lo <= r < hi (faiss IDSelectorRange), clipped to [0, n)"""
        n = int(n)
        m = np.zeros(n, dtype=bool)
        m[max(int(lo), 0): max(min(int(hi), n), 0)] = True
        return cls(cls._upload(torch.from_numpy(_pack_host(m)), device), n, count=int(m.sum()))

    @classmethod
    def from_classes(cls, row_class, class_ids, n_classes, device=None):
        """rows whose class (int32 row -> class map [n]) is one of class_ids; a row class outside [0, n_classes) is unselected"""
        n_classes = int(n_classes)
        on = np.zeros(max(n_classes, 1), dtype=np.uint8)
        cid = np.asarray(list(class_ids), dtype=np.int64).reshape(-1)
        on[cid[(cid >= 0) & (cid < n_classes)]] = 1
        if isinstance(row_class, torch.Tensor) and row_class.is_cuda:
            rc = row_class.detach().reshape(-1).to(torch.int32).contiguous()
            n = rc.numel()
            words = torch.empty(_sel_words(n), dtype=torch.int64, device=rc.device)
            if n == 0:
                words.zero_()
            d_on = torch.from_numpy(on).to(rc.device, non_blocking=True)
            with torch.cuda.device(rc.device):
                nv.check(nv.lib().ac_knn_sel_classes(nv.ptr(rc), n, nv.ptr(d_on), n_classes, nv.ptr(words), nv.stream_ptr(rc.device)),
                         "ac_knn_sel_classes")
            return cls(words, n)
        rc = row_class.detach().cpu().numpy() if isinstance(row_class, torch.Tensor) else np.asarray(row_class)
        rc = rc.reshape(-1).astype(np.int64)
        ok = (rc >= 0) & (rc < n_classes)
        m = np.zeros(rc.size, dtype=bool)
        m[ok] = on[rc[ok]] != 0
        return cls(cls._upload(torch.from_numpy(_pack_host(m)), device), rc.size, count=int(m.sum()))

    def to(self, device):
        return RowSelector(self.words.to(device), self.n, None if self.ids is None else self.ids.to(device), count=self.known_count)

    def count(self):
        """selected rows: known_count where it is known, else read from the bitmap (one host synchronisation) and kept"""
        if self.known_count is None:
            self.known_count = (int(self.ids.numel()) if self.ids is not None else
                                int(np.unpackbits(self.words.cpu().numpy().view(np.uint8), bitorder="little")[: self.n].sum()))
        return self.known_count


def selection_facts(sel, id_list=True):
    """the planner's `Selection` of a RowSelector (None stays None), from what the host already holds -- `count()` is never
    called.  id_list=False: the caller has no id-list route (a row shard: the ids are global)."""
    if sel is None:
        return None
    ids = getattr(sel, "ids", None) if id_list else None
    return Selection(None if ids is None else ids.numel(), getattr(sel, "known_count", None), getattr(sel, "n", None))


def knn_topk_sel(P, N, D, Q, k, sel, metric="l2", sel_bit0=0, row_offset=0, out=None, workspace=None, stats=None, exact_out=None,
                 prepared=None):
    """FILTERED top-k (`ac_knn_l2_topk_sel` / `ac_knn_ip_topk_sel`): the k best rows of P[:N] AMONG the selected ones -- what
    `knn_l2_topk` / `knn_ip_topk` return on a store of only those rows, with the original row ids; fewer than k selected rows
    pad with (FLT_MAX, -1) / (-FLT_MAX, -1).  sel: a RowSelector or its int64 words tensor; local row r is bit sel_bit0 + r (a
    row shard passes sel_bit0 = its first row and the replicated global bitmap).  Other arguments, the workspace
    (`knn_workspace_bytes`) and stats as `knn_l2_topk`.  prepared: optional (planes, norms) from `prepare_store`: where
    `batch_applies(N, nq, k)` holds the search proposes from the store's fp16 plane (`ac_knn_*_topk_batch_sel`, workspace
    `knn_batch_workspace_bytes`) -- the same exact result at any density of the selection, but only worth it for a dense one
    (`sel_batch_applies`); else, and without it, the fp32 rows are searched.  Asynchronous."""
    kind = plan_topk(N, Q.shape[0], k, have_plane=prepared is not None, auto=False).kind
    return _knn_topk(metric, kind, P, N, D, Q, k, row_offset, out, exact_out, workspace, stats, prepared, sel, sel_bit0)


def knn_topk_ids(P, N, D, Q, k, ids, metric="l2", row_offset=0, out=None, exact_out=None):
    """FILTERED top-k over a short id list (`ac_knn_l2_topk_ids` / `ac_knn_ip_topk_ids`): ids = a RowSelector built by
    `from_ids`, or a SORTED, UNIQUE int64 cuda tensor of <= KNN_IDS_MAX row ids (ids outside [0, N) are skipped).  Reads the
    listed rows only; exact by construction, any k and D, no workspace.  Same result as `knn_topk_sel` with those rows."""
    return _knn_topk(metric, "ids", P, N, D, Q, k, row_offset, out, exact_out, ids=ids)


def knn_range_workspace_bytes(N, D, nq):
    return _planned_bytes("ac_knn_range_workspace", N, D, nq)


def knn_range_batch_workspace_bytes(N, D, nq):
    """workspace of `ac_knn_*_range_count_batch[_sel]` (its prefix is the fp32 route's, which the fill reads)"""
    return _planned_bytes("ac_knn_range_batch_workspace", N, D, nq)


def knn_range_ids_workspace_bytes(M, nq):
    return _planned_bytes("ac_knn_range_ids_workspace", M, nq)


def range_batch_applies(N, D, nq):
    """Library limits of the range count over a prepared store (N >= 65536, a D whose query tile fits): asked of the workspace
    planner, a host-only call."""
    if nq < 1:
        return False
    b = ctypes.c_size_t(0)
    return nv.lib().ac_knn_range_batch_workspace(N, D, nq, ctypes.byref(b)) == 0


def range_query_chunk(N, D, nq, max_ws_bytes, workspace_bytes=None):
    """Queries per call of a range search of nq queries: the largest count whose workspace (the membership bitmap grows as
    nq * N / 8) stays within max_ws_bytes; at least 1.  Raises for an (N, D) the library does not cover.
    workspace_bytes: the planner that sizes a call, (N, D, nq) -> bytes; None = `knn_range_workspace_bytes` (the fp32 route)."""
    ws_bytes = workspace_bytes or knn_range_workspace_bytes
    chunk = max(1, min(nq, max_ws_bytes // max(ws_bytes(N, D, 1), 1)))
    while chunk > 1 and ws_bytes(N, D, chunk) > max_ws_bytes:
        chunk = max(1, chunk // 2)
    return chunk


def stitch_range_chunks(parts, device=None):
    """[(lims [c_i + 1], D, I), ...] of consecutive query chunks -> one (lims [sum c_i + 1], D, I): every chunk's lims shifted by
    the hits before it.  Tensors on any one device; no host synchronisation."""
    if len(parts) == 1:
        return parts[0]
    if not parts:
        return (torch.zeros(1, dtype=torch.int64, device=device), torch.empty(0, dtype=torch.float32, device=device),
                torch.empty(0, dtype=torch.int64, device=device))
    lims, base = [parts[0][0][:1]], parts[0][0][:1]
    for l, _, _ in parts:
        lims.append(l[1:] + base)
        base = base + l[-1:]
    return (torch.cat(lims), torch.cat([d for _, d, _ in parts]), torch.cat([i for _, _, i in parts]))


def _knn_range(metric, form, P, N, D, Q, radius, row_offset, exact_out, stats, chunk, ws_need, count_mid=(), fill_mid=(), sel_args=()):
    """THE range search: per chunk of `chunk` queries  count -> the protocol's one host read -> allocate -> fill.
    count entry ac_knn_{metric}_range_count{form}:  rows *count_mid queries radii *sel_args lims workspace stats stream;
    fill entry ac_knn_{metric}_range_fill[_ids]:    rows *fill_mid queries row_offset lims total outD outD64 outI workspace stats stream."""
    nq, dev = Q.shape[0], Q.device
    if torch.is_tensor(radius):
        rad = radius.detach().to(device=dev, dtype=torch.float32).reshape(-1).contiguous()
        assert rad.numel() == nq, "one radius per query"
    else:
        rad = torch.full((nq,), float(radius), dtype=torch.float32, device=dev)
    if nq == 0:
        empty = stitch_range_chunks([], dev)
        return empty + (torch.empty(0, dtype=torch.float64, device=dev),) if exact_out else empty
    count_name, fill_name = f"ac_knn_{metric}_range_count{form}", f"ac_knn_{metric}_range_fill" + ("_ids" if form == "_ids" else "")
    count, fill = getattr(nv.lib(), count_name), getattr(nv.lib(), fill_name)
    ws = torch.empty(max(ws_need, 256), dtype=torch.uint8, device=dev)
    rows, tail = (nv.ptr(P), N, P.stride(0), D), (nv.ptr(ws), ws.numel(), nv.ptr(stats), nv.stream_ptr(dev))
    parts = []
    with torch.cuda.device(dev):
        for s in range(0, nq, chunk):
            q, r = Q[s:s + chunk], rad[s:s + chunk]
            queries = (nv.ptr(q), q.shape[0], q.stride(0))
            lims = torch.empty(q.shape[0] + 1, dtype=torch.int64, device=dev)
            nv.check(count(*rows, *count_mid, *queries, nv.ptr(r), *sel_args, nv.ptr(lims), *tail), count_name)
            total = int(lims[-1].item())                      # the protocol's one host read: sizes the outputs
            outD = torch.empty(total, dtype=torch.float32, device=dev)
            outI = torch.empty(total, dtype=torch.int64, device=dev)
            outE = torch.empty(total, dtype=torch.float64, device=dev) if exact_out else None
            nv.check(fill(*rows, *fill_mid, *queries, row_offset, nv.ptr(lims), total, nv.ptr(outD), nv.ptr(outE), nv.ptr(outI), *tail),
                     fill_name)
            parts.append((lims, outD, outI, outE))
    out = stitch_range_chunks([p[:3] for p in parts], dev)
    if not exact_out:
        return out
    return out + (parts[0][3] if len(parts) == 1 else torch.cat([p[3] for p in parts]),)


def knn_range_search(P, N, D, Q, radius, metric="l2", row_offset=0, exact_out=False, max_ws_bytes=256 << 20, stats=None, sel=None,
                     sel_bit0=0, prepared=None):
    """Exact range search (`ac_knn_l2_range_count` / `_fill`, or the `ip` pair): every row of P[:N] with float32(exact squared
    distance) < radius (metric "l2"), or float32(exact inner product) > radius ("ip"); faiss range_search semantics, strict.

    radius: a float or a [nq] tensor (one radius per query).  Returns (lims int64 [nq + 1], D fp32, I int64) device tensors: the
    hits of query q are D / I[lims[q]:lims[q + 1]], by ascending row id (+ row_offset); exact_out=True appends the exact fp64
    values.  Queries go in chunks whose workspace stays within max_ws_bytes; the result does not depend on the chunking.  One
    host read (the hit count) per chunk.  stats: optional int32 [4] cuda tensor, the d_stats of the LAST chunk's calls ([0] =
    pairs the count phase decided by exact arithmetic, [1] = 1 if the fill did not fit -- it always fits here).
    sel: the FILTERED range search (`ac_knn_*_range_count_sel`; the fill is the unfiltered one) -- a RowSelector or its int64
    words tensor; local row r can be a hit iff bit sel_bit0 + r is set (a row shard passes sel_bit0 = its first row and the
    replicated global bitmap).  Raises ValueError when the bitmap does not cover [sel_bit0, sel_bit0 + N).  An unselected pair
    is never decided exactly (stats[0] counts selected pairs only); an all-ones selection returns the unfiltered bits.
    prepared: optional (planes, norms) from `prepare_store`, current for P[:N].  Where `range_batch_applies`, the COUNT then reads
    the store's fp16 plane (`ac_knn_*_range_count_batch[_sel]`: half the bytes; stats[2] = 2 reports it) -- the same bits at any
    radius, since every pair the plane cannot decide is decided from the fp32 rows as before.  The fill and the host read per chunk
    are unchanged; chunks are sized by the batch workspace."""
    _check_rows_queries(P, Q, metric)
    nq = Q.shape[0]
    plane = plan_range(N, prepared is not None, prepared is not None and range_batch_applies(N, D, nq), auto=False) == "plane"
    ws_bytes = knn_range_batch_workspace_bytes if plane else knn_range_workspace_bytes
    sel_args = () if sel is None else _sel_args(sel, sel_bit0, N)
    chunk = range_query_chunk(N, D, nq, max_ws_bytes, ws_bytes) if nq else 1
    return _knn_range(metric, ("_batch" if plane else "") + ("_sel" if sel is not None else ""), P, N, D, Q, radius, row_offset, exact_out,
                      stats, chunk, ws_bytes(N, D, min(chunk, nq)), count_mid=(nv.ptr(prepared[0]), nv.ptr(prepared[1])) if plane else (),
                      sel_args=sel_args)


def knn_range_ids(P, N, D, Q, radius, ids, metric="l2", row_offset=0, exact_out=False, stats=None):
    """FILTERED range search over a short id list (`ac_knn_*_range_count_ids` / `_fill_ids`): the hits AMONG the listed rows.
    ids = a RowSelector built by `from_ids`, or a SORTED, UNIQUE int64 cuda tensor of <= KNN_IDS_MAX row ids (ids outside [0, N)
    are skipped).  Reads the listed rows only, any D and N; the workspace (a bitmap over list positions) does not depend on N, so
    the queries go in one call.  Returns what `knn_range_search(..., sel=)` returns for those rows -- bit for bit where that route
    covers the store.  One host read (the hit count).  stats[0] = the listed pairs inside the store (all decided exactly)."""
    _check_rows_queries(P, Q, metric)
    listed, nq = _ids_args(ids), Q.shape[0]
    return _knn_range(metric, "_ids", P, N, D, Q, radius, row_offset, exact_out, stats, max(nq, 1),
                      knn_range_ids_workspace_bytes(listed[1], nq) if nq else 0, count_mid=listed, fill_mid=listed)


class _HipFlatIndex:
    """The flat store both metrics share: resident rows, lazy upload, compaction, in-place updates.  `metric` ("l2" / "ip")
    picks the search entry points; both metrics search the same kind of prepared store (one fp16 plane + norms).

    When the plane is prepared (two passes over the rows, 2 B per element): a many-query search (>= BATCH_MIN_QUERIES queries
    and N * nq >= BATCH_MIN_PAIRS) prepares it at once -- it pays within the call.  The L2 index also prepares it for a small
    batch on >= PLANE_MIN_ROWS rows once the store has served one search since it was last rebuilt.  The IP index NEVER
    prepares from small searches: an index that only ever answers few-query searches keeps to the fp32 sweeps and holds no
    plane.  Once a plane exists -- for either metric -- small batches on >= PLANE_MIN_ROWS rows use the fp16-plane sweep; the
    plane follows `add` / `update_rows` incrementally and is dropped by `remove_ids` / `reset`.

    Host-side bookkeeping (add / ntotal / remove_ids) works without a GPU: added rows are queued on
    the host and uploaded in one copy when the device matrix is first needed.  search() has no CPU
    implementation -- without a GPU it raises."""

    metric = None

    def __init__(self, d, device=None):
        self.d = int(d)
        self._device_arg = device
        self.ld = (self.d + 3) // 4 * 4
        self._n = 0                  # rows resident in the device matrix
        self._store = None
        self._pending = []           # host row blocks not yet uploaded
        self._npending = 0
        self._ws = None
        self._stats = None
        self._prepared = None        # (planes, norms) of the resident rows for the batched search; dropped when rows change
        self._searches_since_change = 0
        self._range_stats = None     # d_stats of the last range_search_device() that took the bitmap route

    def _rows_changed(self):
        """the resident rows changed in a way the prepared plane cannot follow (compaction, adoption of another matrix, reset)"""
        self._prepared = None
        self._searches_since_change = 0

    def _rows_written(self, n_old, row0, nrows):
        """rows [row0, row0 + nrows) were overwritten / appended (n_old -> self._n rows): the prepared plane follows
        incrementally (`ac_knn_update_store`: those rows only) unless the new rows change the store's scale -- an index that is
        both searched and added to keeps its fp16 plane instead of paying two passes over all rows per change (round 3 dropped
        the plane on every change)."""
        if self._prepared is None:
            return
        planes, norms = self._prepared
        need_p, need_n = store_buffers_sizes(self._n, self.d)
        if planes.numel() < need_p or norms.numel() < need_n:            # grow: the first n_old rows' entries are a prefix
            cap = max(self._store.shape[0], self._n)
            planes2, norms2 = store_buffers(cap, self.d, self.device)
            old_p, old_n = store_buffers_sizes(n_old, self.d)
            planes2[:old_p] = planes[:old_p]
            norms2[:old_n] = norms[:old_n]
            self._prepared = (planes2, norms2)
        if not update_store(self._store, n_old, self._n, self.d, self._prepared, row0, nrows):
            self._prepared = None                                         # scale changed: prepared anew at the next search

    def prepare_plane(self):
        """Build the fp16 plane NOW (a store of >= BATCH_MIN_ROWS rows; `prepare_store`: two passes over the rows) instead of at
        the first many-query / second few-query search, and count one search as served: every search of a static store, the
        first included, then proposes from the plane."""
        if self.ntotal >= BATCH_MIN_ROWS:
            self._prepared = prepare_store(self._store, self.ntotal, self.d)
            self._searches_since_change = 1

    @property
    def device(self):
        if self._device_arg is not None:
            return torch.device(self._device_arg)
        nv.require_gpu()
        return torch.device(f"cuda:{torch.cuda.current_device()}")

    # -- faiss protocol ------------------------------------------------------------------
    @property
    def ntotal(self):
        return self._n + self._npending

    def _as_rows(self, x):
        if isinstance(x, torch.Tensor):
            t = x.detach().to(dtype=torch.float32)
        else:
            t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
        return t.reshape(-1, self.d)

    def _reserve(self, n):
        dev = self.device
        if self._store is not None and n <= self._store.shape[0]:
            return
        have = 0 if self._store is None else self._store.shape[0]
        cap = max(n, 2 * have, 64)
        new = torch.zeros((cap, self.ld), dtype=torch.float32, device=dev)
        if self._n:
            new[: self._n] = self._store[: self._n]
        self._store = new

    def _materialize(self):
        """Upload queued rows (one H2D copy)."""
        nv.require_gpu()
        if self._pending:
            rows = torch.cat(self._pending, 0) if len(self._pending) > 1 else self._pending[0]
            self._pending, self._npending = [], 0
            m = rows.shape[0]
            self._reserve(self._n + m)
            self._store[self._n: self._n + m, : self.d] = rows.to(self.device, non_blocking=True)
            self._n += m
            self._rows_written(self._n - m, self._n - m, m) if self._n > m else self._rows_changed()
        if self._store is None:
            self._reserve(1)
        if self._stats is None:
            self._stats = torch.zeros(4, dtype=torch.int32, device=self.device)

    def add(self, x):
        rows = self._as_rows(x)
        if rows.shape[0] == 0:
            return
        if rows.is_cuda:
            self._materialize()
            m = rows.shape[0]
            self._reserve(self._n + m)
            self._store[self._n: self._n + m, : self.d] = rows.to(self.device)
            self._n += m
            self._rows_written(self._n - m, self._n - m, m) if self._n > m else self._rows_changed()
        else:
            self._pending.append(rows.clone())
            self._npending += rows.shape[0]

    def add_device_rows(self, rows):
        """Adopt an existing [n, ld] device matrix without copying (large synthetic stores)."""
        assert rows.is_cuda and rows.dtype == torch.float32 and rows.stride(1) == 1
        assert rows.stride(0) % 4 == 0 and rows.stride(0) >= self.ld and rows.data_ptr() % 16 == 0
        self._device_arg = rows.device
        self._pending, self._npending = [], 0
        self._store = rows
        self._n = rows.shape[0]
        self._rows_changed()

    def remove_ids(self, ids):
        if isinstance(ids, torch.Tensor):
            ids = ids.detach().cpu().numpy()
        ids = np.unique(np.asarray(ids).reshape(-1).astype(np.int64))
        ids = ids[(ids >= 0) & (ids < self.ntotal)]
        if ids.size == 0:
            return 0
        self._materialize()
        keep = torch.ones(self._n, dtype=torch.bool, device=self.device)
        keep[torch.from_numpy(ids).to(self.device)] = False
        kept = self._store[: self._n][keep]             # IndexFlat compacts: later rows shift down
        self._store[: kept.shape[0]] = kept
        self._n = kept.shape[0]
        self._rows_changed()
        return int(ids.size)

    def reset(self):
        self._n = 0
        self._pending, self._npending = [], 0
        self._rows_changed()

    def update_rows(self, rows, values):
        """Overwrite existing rows in place (ids keep their meaning; no compaction)."""
        rows = torch.as_tensor(rows, dtype=torch.int64)
        if rows.numel() == 0:
            return
        if int(rows.max()) >= self.ntotal or int(rows.min()) < 0:
            raise IndexError("update_rows: row id out of range")
        self._materialize()
        vals = self._as_rows(values).to(self.device)
        # (the runs are computed BEFORE the store is touched: nothing below can fail between the write and the plane's update)
        runs = None
        if self._prepared is not None:
            ids = np.unique(rows.detach().cpu().numpy())
            runs = np.split(ids, np.nonzero(np.diff(ids) != 1)[0] + 1)       # contiguous runs of row ids
        self._store[rows.to(self.device), : self.d] = vals
        if runs is not None:
            if len(runs) > 16:
                self._rows_changed()                                      # many scattered rows: a fresh preparation is cheaper
            else:
                try:
                    for run in runs:
                        if self._prepared is None:
                            break
                        self._rows_written(self._n, int(run[0]), int(run.size))
                except Exception:
                    self._rows_changed()                                  # never leave a plane that no longer matches the rows
                    raise

    def _as_selector(self, sel):
        """a RowSelector for the resident rows from what search() accepts: a RowSelector, a bool mask [ntotal] or row ids"""
        if isinstance(sel, RowSelector):
            if sel.n != self._n:
                raise ValueError(f"selector covers {sel.n} rows, the index holds {self._n}")
            return sel if sel.words.device == self.device else sel.to(self.device)
        is_bool = sel.dtype == torch.bool if isinstance(sel, torch.Tensor) else np.asarray(sel).dtype == np.bool_
        if is_bool:
            if int(np.prod(tuple(sel.shape))) != self._n:
                raise ValueError(f"mask has {int(np.prod(tuple(sel.shape)))} entries, the index holds {self._n} rows")
            return RowSelector.from_mask(sel if isinstance(sel, torch.Tensor) and sel.is_cuda else (
                sel.cpu().numpy() if isinstance(sel, torch.Tensor) else sel), device=self.device)
        return RowSelector.from_ids(sel, self._n, device=self.device)

    def _as_queries(self, q):
        """[nq, d] fp32 rows on the index's device, unit inner stride, from a tensor on any device (a vector is one query)"""
        q = q.detach().to(device=self.device, dtype=torch.float32)
        if q.dim() == 1:
            q = q.unsqueeze(0)
        return q if q.stride(-1) == 1 else q.contiguous()

    def search_device(self, q, k, sel=None):
        """q: [nq, d] fp32 tensor (any device) -> (dist, ids) CUDA tensors; no host sync.  sel: a RowSelector, a bool mask
        [ntotal] or row ids -- the FILTERED search, the k best AMONG those rows.  The route is `plan_topk`'s (module docstring):
        unfiltered, the L2 index prepares a missing plane on its second small search; the IP index and every filtered search
        prepare only from BATCH_MIN_QUERIES queries on, fewer use a plane that exists."""
        self._materialize()
        q = self._as_queries(q)
        if sel is not None:
            sel = self._as_selector(sel)
        # (appends and in-place updates do not reset the count of searches: once prepared, the plane follows them incrementally)
        policy = PREPARE_SECOND_SEARCH if sel is None and self.metric == "l2" else PREPARE_NEVER_SMALL
        route = plan_topk(self._n, q.shape[0], k, selection_facts(sel), self._prepared is not None, self._searches_since_change, policy)
        if route.kind == "ids":
            return knn_topk_ids(self._store, self._n, self.d, q, k, sel.ids, metric=self.metric)
        if route.prepare:
            # (sized for the store's CAPACITY: the first append after the preparation then updates the plane in place
            #  instead of allocating capacity-sized buffers and copying the whole old plane beside them)
            self._prepared = prepare_store(self._store, self._n, self.d, capacity=self._store.shape[0])
        if sel is None:
            self._searches_since_change += 1
        plane = route.kind == "plane"
        need = (knn_batch_workspace_bytes if plane else knn_workspace_bytes)(self._n, self.d, q.shape[0], k)
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(max(need, 256), dtype=torch.uint8, device=self.device)
        ours = dict(workspace=self._ws, stats=self._stats, prepared=self._prepared if plane else None)
        if sel is not None:
            return knn_topk_sel(self._store, self._n, self.d, q, k, sel, metric=self.metric, **ours)
        return (knn_ip_topk if self.metric == "ip" else knn_l2_topk)(self._store, self._n, self.d, q, k, **ours)

    def search(self, x, k, sel=None):
        """faiss signature: numpy in, (float32 [nq,k], int64 [nq,k]) numpy out.  sel (faiss: params=SearchParameters(sel=...)):
        a RowSelector, a bool mask or row ids; fewer than k selected rows pad as faiss does."""
        q = self._as_rows(x)
        D, I = self.search_device(q, int(k)) if sel is None else self.search_device(q, int(k), sel)
        return D.cpu().numpy(), I.cpu().numpy()

    def range_search_device(self, q, radius, sel=None, max_ws_bytes=256 << 20):
        """q: [nq, d] fp32 tensor (any device), radius: float or [nq] tensor -> (lims, D, I) CUDA tensors (`knn_range_search`).
        A range search NEVER prepares the fp16 plane; when one already exists (a top-k search or `prepare_store` built it and it
        has followed the rows since) and the store has >= PLANE_MIN_ROWS rows, the count reads it (`prepared=`: half the bytes,
        the same bits) -- `range_stats[2] == 2` then.  Otherwise the fp32 rows are searched.
        sel: a RowSelector, a bool mask [ntotal] or row ids (whatever `search(sel=)` accepts) -- the hits AMONG those rows.  A
        selector that carries <= KNN_IDS_MAX host ids takes the id-list route (`knn_range_ids`) first, everything else the bitmap
        route; no bitmap is read back to choose."""
        self._materialize()
        q = self._as_queries(q)
        if sel is not None:
            sel = self._as_selector(sel)
        kind = plan_range(self._n, self._prepared is not None, True, selection_facts(sel))     # (knn_range_search asks the library)
        if kind == "ids":
            return knn_range_ids(self._store, self._n, self.d, q, radius, sel.ids, metric=self.metric)
        if self._range_stats is None and q.is_cuda:
            self._range_stats = torch.zeros(4, dtype=torch.int32, device=q.device)
        return knn_range_search(self._store, self._n, self.d, q, radius, metric=self.metric, max_ws_bytes=max_ws_bytes, sel=sel,
                                stats=self._range_stats, prepared=self._prepared if kind == "plane" else None)

    def range_search(self, x, radius, sel=None):
        """faiss signature: numpy in, (lims int64 [nq + 1], D float32, I int64) numpy out.  L2: squared distance < radius;
        IP: inner product > radius.  Hits of a query by ascending row id.  sel (faiss: params=SearchParameters(sel=...)): a
        RowSelector, a bool mask or row ids."""
        lims, D, I = self.range_search_device(self._as_rows(x), radius, sel=sel)
        return lims.cpu().numpy(), D.cpu().numpy(), I.cpu().numpy()

    @property
    def range_stats(self):
        """d_stats of the last bitmap-route range search as a list: [0] pairs decided exactly, [2] == 2 iff the count read the plane"""
        return [0, 0, 0, 0] if self._range_stats is None else self._range_stats.tolist()

    @property
    def exact_fallbacks(self):
        """Queries of the last search() that needed the exact fp64 fallback sweep."""
        return 0 if self._stats is None else int(self._stats[0].item())


class HipFlatL2Index(_HipFlatIndex):
    """Drop-in for faiss.IndexFlatL2 as used by PrototypeMemory: exact squared L2, ascending, ties to the lower id."""
    metric = "l2"


class HipFlatIPIndex(_HipFlatIndex):
    """Drop-in for faiss.IndexFlatIP: exact inner product, descending, ties to the lower id (`ac_knn_ip_topk`).  Rows need not
    be normalised; for L2-normalised rows this is the cosine search.  Same protocol and storage as HipFlatL2Index; its fp16
    plane is prepared by many-query searches only (`_HipFlatIndex`)."""
    metric = "ip"


def _topk_merge(entry, D_in, I_in):
    """the merge entries share one argument list: [shards, nq, k] lists in, (values fp32, ids) [nq, k] out"""
    nv.require_gpu()
    S, nq, k = D_in.shape
    D_in, I_in = D_in.contiguous(), I_in.contiguous()
    outD = torch.empty((nq, k), dtype=torch.float32, device=D_in.device)
    outI = torch.empty((nq, k), dtype=torch.int64, device=D_in.device)
    with torch.cuda.device(D_in.device):
        nv.check(getattr(nv.lib(), entry)(nv.ptr(D_in), nv.ptr(I_in), S, nq, k, nv.ptr(outD), nv.ptr(outI), nv.stream_ptr(D_in.device)),
                 entry)
    return outD, outI


def topk_merge_ip(D_in, I_in):
    """[shards, nq, k] per-shard DESCENDING float64 lists (`knn_ip_topk_exact`) -> global (values fp32, ids) [nq, k] by (value
    descending, id ascending) -- ac_topk_merge_ip_f64, the merge of a row-sharded inner-product search."""
    assert D_in.dtype == torch.float64
    return _topk_merge("ac_topk_merge_ip_f64", D_in, I_in)


def topk_merge(D_in, I_in):
    """[shards, nq, k] per-shard ascending lists -> global (dist fp32, ids) [nq, k].  float64 input (the shards' exact
    distances, `knn_l2_topk_exact`) is merged by (exact distance, id) -- ac_topk_merge_f64, what a sharded search needs to
    equal the unsharded one bit for bit; float32 input by (fp32 distance, id) -- ac_topk_merge."""
    assert D_in.dtype in (torch.float32, torch.float64)
    return _topk_merge("ac_topk_merge_f64" if D_in.dtype == torch.float64 else "ac_topk_merge", D_in, I_in)


def proto_scores(D, I):
    """memory.py:117,129-130 on device: softmax(exp(-d)) over each query's valid hits."""
    nv.require_gpu()
    D = D.contiguous()
    I = I.contiguous()
    out = torch.empty_like(D)
    with torch.cuda.device(D.device):
        nv.check(nv.lib().ac_proto_scores(nv.ptr(D), nv.ptr(I), D.shape[0], D.shape[1], nv.ptr(out),
                                          nv.stream_ptr(D.device)), "ac_proto_scores")
    return out


def synth_unit_rows(n, D, seed, row_offset=0, device=None, ld=None):
    """Deterministic unit-norm rows generated on the device (bit-identical to oracle/synth.py)."""
    nv.require_gpu()
    device = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")
    ld = ld or (D + 3) // 4 * 4
    out = torch.empty((n, ld), dtype=torch.float32, device=device)
    with torch.cuda.device(device):
        nv.check(nv.lib().ac_synth_unit_rows(nv.ptr(out), n, ld, D, seed, row_offset, nv.stream_ptr(device)),
                 "ac_synth_unit_rows")
    return out
