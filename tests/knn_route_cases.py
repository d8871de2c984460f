"""The scripted search sequences whose ROUTING is recorded (tools/knn_route_probe.py, once, at the parent of the commit that put the
routing behind `plan_topk` / `plan_range`) and replayed on CPU (tests/test_knn_route_cpu.py), with the module-level calls of
`adaptive_classifier.index` replaced by recorders -- no device work.

A sequence: (name, target, n, D, steps), begun on an object without a plane or prior searches.  target: "l2" / "ip" (the flat
indexes) or "sharded-l2" / "sharded-ip" (a `ShardedSearch` over the SECOND of two shards of n rows each: row offset n, selectors
cover the 2 n global rows).  Steps:
    ("search", nq, k, sel)   ("range", nq, sel)   ("reset",)   ("remove",)   ("add", m, follows)   ("count",)
    ("fresh", plane, prior[, n]): go on with a NEW object (of n rows) on which a plane exists / that has served `prior` searches;
                                  it leaves no record
sel: None, "ids8192", "ids8193", ("known", count) or "unknown" (a bitmap of every second row whose count the host does not know until
the ("count",) step reads it).

A record, per step, one line of twelve fields (`encode`): [reached function, `prepared` passed, prepare_store calls of the sequence
so far, its last `capacity`, the workspace planner asked, sel_bit0, row_offset, _searches_since_change after, kind, prepare, plane
before, searches before]."""
from contextlib import ExitStack
from unittest import mock

import numpy as np
import torch

ROWS = (1000, 65535, 65536, (1 << 18) - 1, 1 << 18, 312499, 312500, 400000)
QUERIES = (1, 63, 64, 128, 300)
INDEXES, SHARDED = ("l2", "ip"), ("sharded-l2", "sharded-ip")


def total_rows(target, n):
    return 2 * n if target in SHARDED else n


def _selections(target, n):
    t = total_rows(target, n)
    edge = (t + 31) // 32                                    # the smallest count with count * 32 >= total
    sels = ["ids8192", "ids8193", ("known", edge), ("known", edge - 1), ("known", t // 2), "unknown"]
    if target in SHARDED:
        sels.append(("known", (n + 31) // 32))              # dense by the LOCAL figure only: the global one decides
    return sels


# the query counts that can change the route at each row count (64 x 2^18 and 64 x 312499 pairs stay under BATCH_MIN_PAIRS)
GRID = {1000: (1, 300), 65535: (1, 300), 65536: (1, 300), (1 << 18) - 1: (1, 63, 64, 128), 1 << 18: (1, 63, 64, 128),
        312499: (63, 64), 312500: (63, 64), 400000: QUERIES}


def _sequences():
    out = []
    for target in INDEXES + SHARDED:
        states = ((False, 0), (False, 1), (True, 0)) if target in INDEXES else ((False, 0), (True, 0))
        for n in (ROWS if target != "sharded-ip" else ()):       # (the shard's metric only picks the function: its grid runs once)
            steps = []
            for state in states:                                  # unfiltered top-k: every step on a fresh object
                for nq in GRID[n]:
                    steps += [("fresh",) + state, ("search", nq, 8, None)]
            # selections: without / over a plane, just under / at BATCH_MIN_QUERIES; once at the row count of the plane rule
            for plane, nq in {1 << 18: ((True, 63),), 400000: ((False, 63), (False, 64), (True, 63), (True, 64))}.get(n, ()):
                for sel in _selections(target, n):
                    steps += [("fresh", plane, 1), ("search", nq, 8, sel)]
            out.append((f"{target}-n{n}", target, n, 8, steps))
        for plane in (False, True):
            out.append((f"{target}-k-plane{int(plane)}", target, 400000, 8,
                        [st for nq in (1, 64) for k in (100, 101) for sel in (None, ("known", 400000))
                         for st in (("fresh", plane, 1), ("search", nq, k, sel))]))
        # range: every row count over a plane at a D the plane route takes and one whose query tile it refuses; without a plane;
        # each selection kind over a plane
        for D in (64, 2308):
            out.append((f"{target}-range-d{D}", target, 1 << 18, D,
                        [st for n in ROWS for st in (("fresh", True, 0, n), ("range", 3, None))] + [("fresh", False, 0), ("range", 3, None)] +
                        [("fresh", True, 0)] + [("range", 3, sel) for sel in ("ids8192", "ids8193", ("known", 1 << 17), "unknown")]))
    for target in INDEXES:
        # the plane's life: built by the policy, used by small batches and range searches, dropped by reset / remove_ids, followed by add
        out.append((f"{target}-life", target, 400000, 64, [
            ("range", 3, None), ("search", 1, 8, None), ("search", 1, 8, ("known", 200000)), ("search", 1, 8, None), ("search", 1, 8, None),
            ("range", 3, None), ("search", 63, 8, ("known", 200000)), ("reset",), ("search", 1, 8, None), ("search", 64, 8, None),
            ("range", 3, "unknown"), ("remove",), ("range", 3, None), ("search", 63, 8, ("known", 200000)),
            ("search", 64, 8, "unknown"), ("count",), ("search", 64, 8, "unknown"), ("search", 1, 8, "unknown"), ("add", 5, True),
            ("search", 1, 8, None), ("add", 5, False), ("search", 1, 8, None), ("search", 1, 8, None), ("search", 64, 8, "ids8192"),
            ("search", 300, 101, None), ("search", 300, 100, None)]))
    for target in SHARDED:
        out.append((f"{target}-life", target, 400000, 64, [
            ("range", 3, None), ("search", 63, 8, ("known", 400000)), ("search", 64, 8, "unknown"), ("count",), ("search", 64, 8, "unknown"),
            ("search", 1, 8, ("known", 400000)), ("range", 3, "unknown"), ("search", 1, 8, None), ("range", 3, None),
            ("fresh", False, 0), ("search", 1, 8, None), ("search", 1, 8, ("known", 400000)), ("range", 3, ("known", 400000))]))
    return out


SEQUENCES = _sequences()
NAMES = [s[0] for s in SEQUENCES]
SEARCH_FNS = ("knn_l2_topk", "knn_ip_topk", "knn_topk_sel", "knn_topk_ids", "knn_l2_topk_exact", "knn_ip_topk_exact")
RANGE_FNS = ("knn_range_search", "knn_range_ids")
PLANE = (torch.zeros(4, dtype=torch.int16), torch.zeros(4))


class Harness:
    """the recorders over `adaptive_classifier.index` and the object under a sequence"""

    def __init__(self, ix):
        self.ix = ix
        self.real_range_batch_applies = ix.range_batch_applies
        self.reached, self.planners, self.prepares, self.capacity, self.updates = [], [], 0, None, []

    def patches(self):
        ix, stack = self.ix, ExitStack()
        for name in SEARCH_FNS:
            stack.enter_context(mock.patch.object(ix, name, self._search(name)))
        for name in RANGE_FNS:
            stack.enter_context(mock.patch.object(ix, name, self._range(name)))
        for name, val in (("knn_workspace_bytes", 256), ("knn_batch_workspace_bytes", 512)):
            stack.enter_context(mock.patch.object(ix, name, self._planner(name, val)))
        stack.enter_context(mock.patch.object(ix, "prepare_store", self._prepare))
        stack.enter_context(mock.patch.object(ix, "update_store", lambda *a: self.updates.pop(0)))
        stack.enter_context(mock.patch.object(ix, "store_buffers_sizes", lambda *a: (0, 0)))      # (the stand-in plane never grows)
        stack.enter_context(mock.patch.object(ix._HipFlatIndex, "_materialize", lambda self: None))
        return stack

    def _search(self, name):
        def f(P, N, D, Q, k, *a, **kw):
            self.reached.append((name, kw.get("prepared") is not None, kw.get("sel_bit0"), kw.get("row_offset"), None))
            return "D", "I"
        return f

    def _range(self, name):
        def f(P, N, D, Q, radius, *a, **kw):
            taken = kw.get("prepared") is not None and bool(self.real_range_batch_applies(N, D, Q.shape[0]))
            self.reached.append((name, kw.get("prepared") is not None, kw.get("sel_bit0"), kw.get("row_offset"), taken))
            return "lims", "D", "I", "E"
        return f

    def _planner(self, name, val):
        def f(*a):
            self.planners.append(name)
            return val
        return f

    def _prepare(self, P, N, D, capacity=None):
        self.prepares += 1
        self.capacity = capacity
        return PLANE

    # ---- the object under test ----------------------------------------------------------------------------------------------
    def make(self, target, n, D, plane, prior):
        ix = self.ix
        if target in INDEXES:
            obj = (ix.HipFlatIPIndex if target == "ip" else ix.HipFlatL2Index)(D, device="cpu")
            obj._n, obj._store = n, torch.zeros((1, obj.ld)).expand(n + 7, obj.ld)       # capacity n + 7: not the row count
            obj._searches_since_change = prior
        else:
            from adaptive_classifier.sharded import ShardedSearch
            obj = ShardedSearch(torch.zeros((1, D)).expand(n, D), n, D, n, metric=target[-2:])
        obj._prepared = PLANE if plane else None
        return obj

    def selector(self, spec, total, state):
        ix = self.ix
        if spec is None:
            return None
        if spec == "unknown":
            if "unknown" not in state:
                mask = np.arange(total) % 2 == 0
                state["unknown"] = ix.RowSelector(ix.RowSelector.from_mask(mask, device="cpu").words, total)
            return state["unknown"]
        words = torch.zeros((total + 63) // 64, dtype=torch.int64)
        if spec in ("ids8192", "ids8193"):
            m = int(spec[3:])
            return ix.RowSelector(words, total, torch.arange(m, dtype=torch.int64), count=m)
        return ix.RowSelector(words, total, count=spec[1])

    def run(self, seq):
        _, target, n, D, steps = seq
        obj, state, out = self.make(target, n, D, False, 0), {}, []
        self.prepares, self.capacity = 0, None
        total = total_rows(target, n)
        for step in steps:
            if step[0] == "fresh":
                n = step[3] if len(step) > 3 else seq[2]
                obj, state, total = self.make(target, n, D, step[1], step[2]), {}, total_rows(target, n)
                continue
            del self.reached[:], self.planners[:]
            before = (obj._prepared is not None, getattr(obj, "_searches_since_change", None))
            prepares = self.prepares
            if step[0] == "search":
                q, sel = torch.zeros((step[1], D)), self.selector(step[3], total, state)
                obj.search_device(q, step[2], sel) if target in INDEXES else obj._local(q, step[2], sel)
            elif step[0] == "range":
                q, sel = torch.zeros((step[1], D)), self.selector(step[2], total, state)
                obj.range_search_device(q, 1.0, sel=sel) if target in INDEXES else obj._local_range(q, 1.0, sel)
            elif step[0] == "count":
                state["unknown"].count()
            elif step[0] == "reset":
                obj.reset()
                obj._n = n                                                  # (the rows come back: an upload is device work)
            elif step[0] == "remove":
                keep = obj._store
                obj._store = torch.zeros((16, obj.ld))                      # remove_ids compacts in place: give it rows it can write
                obj._n = 16
                obj.remove_ids([3])
                obj._n, obj._store = n, keep
            elif step[0] == "add":                                          # what _materialize does after the upload of m rows
                self.updates.append(step[2])
                obj._n += step[1]
                obj._rows_written(obj._n - step[1], obj._n - step[1], step[1])
                obj._n = n
            fn, prepared, bit0, off, taken = self.reached[0] if self.reached else (None, False, None, None, None)
            assert len(self.reached) <= 1
            kind = None if fn is None else "ids" if fn.endswith("_ids") else "plane" if (prepared if taken is None else taken) else "rows"
            assert len(self.planners) <= 1
            out.append(encode([fn, prepared, self.prepares, self.capacity, self.planners[0] if self.planners else None, bit0, off,
                               getattr(obj, "_searches_since_change", None), kind, self.prepares > prepares, before[0], before[1]]))
        return out


FN_CODES = {"knn_l2_topk": "l2", "knn_ip_topk": "ip", "knn_topk_sel": "sel", "knn_topk_ids": "ids", "knn_l2_topk_exact": "l2x",
            "knn_ip_topk_exact": "ipx", "knn_range_search": "range", "knn_range_ids": "rids",
            "knn_workspace_bytes": "w", "knn_batch_workspace_bytes": "b"}
FIELDS = ("fn", "prepared", "prepares", "capacity", "planners", "sel_bit0", "row_offset", "searches", "kind", "prepare", "plane_before",
          "searches_before")


def encode(record):
    """the twelve fields of a step as one short line: None -> "-", a flag -> 0 / 1, a function by its FN_CODES entry"""
    return " ".join("-" if v is None else str(int(v)) if isinstance(v, bool) else FN_CODES.get(v, str(v)) for v in record)


def decode(line):
    """{field: text} of a recorded line"""
    return dict(zip(FIELDS, line.split(" ")))


def run_all(ix):
    h = Harness(ix)
    with h.patches():
        return {seq[0]: h.run(seq) for seq in SEQUENCES}
