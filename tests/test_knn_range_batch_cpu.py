"""CPU suite of the range search over the prepared fp16-plane store: the ABI additions (header <-> ctypes table, the workspace
planner and its limits, the argument checks that return before any device work), the host routing of range_search with the device
calls replaced, the margins tests/test_knn_range_batch_gpu.py relies on, and the kernel's resource descriptors.  No GPU needed."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import knn_range_batch_ref as bref  # noqa: E402
import knn_range_ref as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTS = ["ac_knn_l2_range_count_batch", "ac_knn_ip_range_count_batch", "ac_knn_l2_range_count_batch_sel",
          "ac_knn_ip_range_count_batch_sel"]
NEW = ["ac_knn_range_batch_workspace"] + COUNTS


# ---- ABI -------------------------------------------------------------------------------------------------------------------------
def test_header_and_ctypes_table_declare_the_new_symbols():
    from adaptive_classifier import _native as nv
    L = nv.lib()
    assert L.ac_version() >= 8
    src = open(os.path.join(ROOT, "include", "acamd.h")).read()
    assert "no prepared-store form" not in src.replace("\n * ", " ")
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in NEW:
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, code)
        assert m, f"{name} is not declared in acamd.h"
        assert name in nv.exported_symbols() and hasattr(L, name)
        assert len(getattr(L, name).argtypes) == len(m.group(1).split(",")), name      # one ctypes entry per declared argument
    # (d_planes, d_norms) follow D, as in ac_knn_*_topk_batch; (d_sel, sel_bit0) follow d_radius, as in ac_knn_*_range_count_sel
    head = r"\(const float\*\s*d_P,\s*int64_t N,\s*int64_t ldP,\s*int D,\s*const uint16_t\*\s*d_planes,\s*const float\*\s*d_norms,\s*const float\*\s*d_Q,\s*int nq,\s*int64_t ldQ,\s*"
    tail = r"int64_t\*\s*d_lims,\s*void\*\s*d_ws,\s*size_t ws_bytes,\s*int32_t\*\s*d_stats,\s*ac_stream_t stream\)"
    for metric in ("l2", "ip"):
        assert re.search(r"ac_knn_%s_range_count_batch" % metric + head + r"const float\*\s*d_radius,\s*" + tail, code)
        assert re.search(r"ac_knn_%s_range_count_batch_sel" % metric + head +
                         r"const float\*\s*d_radius,\s*const uint64_t\*\s*d_sel,\s*int64_t sel_bit0,\s*" + tail, code)
    p, i64, i32, sz = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_size_t
    plain = [p, i64, i64, i32, p, p, p, i32, i64, p, p, p, sz, p, p]
    assert L.ac_knn_l2_range_count_batch.argtypes == plain and L.ac_knn_ip_range_count_batch.argtypes == plain
    sel = plain[:10] + [p, i64] + plain[10:]
    assert L.ac_knn_l2_range_count_batch_sel.argtypes == sel and L.ac_knn_ip_range_count_batch_sel.argtypes == sel


def test_workspace_planner_limits_and_layout():
    from adaptive_classifier import _native as nv
    from adaptive_classifier import index as ix
    L = nv.lib()
    b, r = ctypes.c_size_t(0), ctypes.c_size_t(0)
    up = lambda n: (n + 255) // 256 * 256
    for N, D, nq in bref.CASES + [(1 << 20, 768, 256), (65536, 2304, 1)]:
        assert L.ac_knn_range_batch_workspace(N, D, nq, ctypes.byref(b)) == 0, (N, D, nq)
        assert L.ac_knn_range_workspace(N, D, nq, ctypes.byref(r)) == 0
        q_rows, Kp = up(nq), (D + 63) // 64 * 64
        # the fp32 route's layout first (the fill reads it), then the query plane, its factors, and four per-query arrays
        assert b.value == up(r.value) + q_rows * Kp * 2 + 5 * up(q_rows * 4) and b.value >= r.value, (N, D, nq)
        assert ix.knn_range_batch_workspace_bytes(N, D, nq) == b.value and ix.range_batch_applies(N, D, nq)
    assert L.ac_knn_range_batch_workspace(65535, 64, 4, ctypes.byref(b)) == -2 and b"N=65535" in L.ac_last_error()
    assert L.ac_knn_range_batch_workspace(5000, 64, 4, ctypes.byref(b)) == -2
    assert L.ac_knn_range_batch_workspace(300, 4096, 4, ctypes.byref(b)) == -2         # a small store the fp32 route takes
    assert L.ac_knn_range_batch_workspace(2 ** 31 - 512, 64, 4, ctypes.byref(b)) == -2
    assert L.ac_knn_range_batch_workspace(70000, 2308, 4, ctypes.byref(b)) == -2       # too wide for the range search's query tile
    assert L.ac_knn_range_workspace(70000, 2308, 4, ctypes.byref(r)) == -2
    assert L.ac_knn_range_batch_workspace(70000, 64, 4, None) == -1
    assert not ix.range_batch_applies(65535, 64, 4) and not ix.range_batch_applies(70000, 2308, 4) and not ix.range_batch_applies(70000, 64, 0)
    # chunking by the batch workspace: the optional planner argument; the existing signature and results stay
    assert ix.range_query_chunk(70000, 64, 40, 100_000) == ix.range_query_chunk(70000, 64, 40, 100_000, ix.knn_range_workspace_bytes)
    budget = ix.knn_range_batch_workspace_bytes(66000, 72, 20)
    c = ix.range_query_chunk(66000, 72, 70, budget, ix.knn_range_batch_workspace_bytes)
    assert 1 <= c and 3 * c <= 70 and ix.knn_range_batch_workspace_bytes(66000, 72, c) <= budget    # the GPU chunking test's setting


def test_argument_checks_return_before_any_device_work():
    from adaptive_classifier import _native as nv
    L = nv.lib()
    buf = (ctypes.c_uint64 * 64)()
    a = ctypes.addressof(buf)
    a += (-a) % 16                                                             # (a 16-byte aligned HOST address: no call may touch it)
    p = ctypes.c_void_p
    N, D, nq = 70000, 768, 7
    need = ctypes.c_size_t(0)
    assert L.ac_knn_range_batch_workspace(N, D, nq, ctypes.byref(need)) == 0
    for name in COUNTS:
        fn = getattr(L, name)
        sel = name.endswith("_sel")

        def call(P=p(a), planes=p(a), norms=p(a), ldP=D, ldQ=D, d_sel=p(a), bit0=0, ws=need.value, q=nq, n_rows=N, fn=fn, sel=sel):
            extra = (d_sel, bit0) if sel else ()
            return fn(P, n_rows, ldP, D, planes, norms, p(a), q, ldQ, p(a), *extra, p(a), p(a), ws, None, None)

        assert call(planes=None) == -1 and b"d_planes" in L.ac_last_error()
        assert call(norms=None) == -1 and b"d_norms" in L.ac_last_error()
        assert call(P=None) == -1 and b"d_P" in L.ac_last_error()
        assert call(planes=p(a + 8)) == -1 and b"aligned" in L.ac_last_error()
        assert call(P=p(a + 4)) == -1 and b"alignment" in L.ac_last_error()    # the rules of ac_knn_l2_topk_batch
        assert call(ldP=D + 2) == -1 and call(ldP=D - 4) == -1 and call(ldQ=D - 1) == -1
        assert call(ws=need.value - 1) == -3 and (b"required %d" % need.value) in L.ac_last_error()
        assert call(n_rows=65535) == -2 and call(n_rows=5000) == -2            # the caller then uses ac_knn_*_range_count
        assert call(q=0) == 0 and call(q=0, planes=None, P=None) == 0          # no query: nothing to do
        if sel:
            assert call(d_sel=None) == -1 and b"d_sel" in L.ac_last_error()
            assert call(d_sel=p(a + 4)) == -1 and b"d_sel" in L.ac_last_error() and b"aligned" in L.ac_last_error()
            assert call(bit0=-1) == -1 and b"sel_bit0" in L.ac_last_error()


# ---- host routing ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls_name", ["HipFlatL2Index", "HipFlatIPIndex"])
def test_index_passes_a_plane_that_exists_and_never_prepares(cls_name, monkeypatch):
    """`prepared` is passed iff a plane exists and the store has >= PLANE_MIN_ROWS rows; a range search never prepares; <=
    KNN_IDS_MAX host ids still take the id-list route."""
    from adaptive_classifier import index as ix
    idx = getattr(ix, cls_name)(8, device="cpu")
    monkeypatch.setattr(ix._HipFlatIndex, "_materialize", lambda self: None)
    monkeypatch.setattr(ix, "prepare_store", lambda *a, **k: pytest.fail("a range search prepared the plane"))
    calls = []
    empty = (torch.zeros(2, dtype=torch.int64), torch.zeros(0), torch.zeros(0, dtype=torch.int64))
    monkeypatch.setattr(ix, "knn_range_ids", lambda P, N, D, Q, r, ids, **kw: calls.append(("ids", N, kw)) or empty)
    monkeypatch.setattr(ix, "knn_range_search", lambda P, N, D, Q, r, **kw: calls.append(("bitmap", N, kw)) or empty)
    q = np.zeros((1, 8), np.float32)
    plane = (torch.zeros(4, dtype=torch.int16), torch.zeros(4))
    for n, have, want in ((ix.PLANE_MIN_ROWS, False, False), (ix.PLANE_MIN_ROWS, True, True), (ix.PLANE_MIN_ROWS - 1, True, False),
                          (70000, True, False), (ix.PLANE_MIN_ROWS + 5, True, True)):
        idx._store, idx._n = torch.zeros((1, 8)).expand(n, 8), n
        idx._prepared = plane if have else None
        for sel in (None, np.arange(n) % 3 == 0):                             # unfiltered, and a mask (the bitmap route)
            idx.range_search(q, 1.0, sel=sel)
            kind, N, kw = calls[-1]
            assert kind == "bitmap" and N == n and (kw.get("prepared") is plane) == want and (want or kw.get("prepared") is None)
            assert kw["metric"] == idx.metric and (kw.get("sel") is None) == (sel is None)
            assert (idx._prepared is plane) == have                            # neither built nor dropped
        idx.range_search(q, 1.0, sel=[5, 3, 3])                               # a short id list keeps priority, plane or not
        assert calls[-1][0] == "ids" and "prepared" not in calls[-1][2]


def test_sharded_local_range_follows_the_same_rule(monkeypatch):
    from adaptive_classifier import index as ix
    from adaptive_classifier.sharded import ShardedSearch
    seen = []
    out = (torch.tensor([0, 0]), torch.zeros(0), torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.float64))
    monkeypatch.setattr(ix, "knn_range_search", lambda P, n, D, Q, r, **kw: seen.append((n, kw)) or out)
    monkeypatch.setattr(ix, "prepare_store", lambda *a, **k: pytest.fail("a range search prepared the shard's plane"))
    plane = (torch.zeros(4, dtype=torch.int16), torch.zeros(4))
    for n, have, want in ((ix.PLANE_MIN_ROWS, False, False), (ix.PLANE_MIN_ROWS, True, True), (ix.PLANE_MIN_ROWS - 1, True, False)):
        ss = ShardedSearch(torch.zeros((1, 8)).expand(n, 8), n, 8, 3, local_search=lambda *a: a, merge=lambda *a: a)
        ss._prepared = plane if have else None
        ss.range_search(torch.zeros(1, 8), 1.0)
        n_seen, kw = seen[-1]
        assert n_seen == n and (kw.get("prepared") is plane) == want and kw["row_offset"] == 3 and kw["exact_out"] is True


# ---- the margins behind the GPU tests --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,D,nq", bref.CASES)
def test_gap_radii_leave_a_wide_margin_and_a_small_undecided_band(N, D, nq):
    """what tests/test_knn_range_batch_gpu.py relies on (it asserts the margin before it compares ids): on its shapes and seeds the
    gap radii of ranks 20..60 admit 21..59 rows, keep every value >= 64 ulps away, and the pairs the fp16 bound cannot decide --
    the cap on d_stats[0] -- are a vanishing share of all pairs"""
    for metric in ("l2", "ip"):
        P, Q, x, rad = bref.case(N, D, nq, metric)
        hits = np.diff(ref.range_search(P, Q, rad, metric, values=x)[0])
        m = bref.min_margin(x, rad)
        cap = bref.undecided_cap(x, rad, bref.bound(P, Q), metric)
        print(N, D, nq, metric, "hits %d..%d, margin %.0f ulps, undecided cap %d of %d pairs" % (hits.min(), hits.max(), m, cap, N * nq))
        assert hits.min() >= 21 and hits.max() <= 59 and m >= 64
        assert cap <= 0.00022 * N * nq


def test_bound_formula_matches_the_header():
    src = open(os.path.join(ROOT, "include", "acamd.h")).read()
    assert "gamma = 1.01 (2^-11 + (K + 18 + sqrt K) 2^-24)" in src
    assert abs(bref.batch_gamma(768) - 1.01 * (2.0 ** -11 + (768 + 18 + np.sqrt(768.0)) * 2.0 ** -24)) < 1e-18
    assert bref.batch_gamma(32) == bref.batch_gamma(64) and bref.batch_gamma(65) == bref.batch_gamma(128)      # K = round_up(D, 64)


# ---- resources -------------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not installed")
def test_plane_range_kernels_use_no_scratch():
    """all eight instantiations (TQ = 32 / 64, L2 / IP, plain / SEL): a private segment of 0 bytes in the kernel descriptor -- a
    spill reload inside the k-loop would drain the 16 loads the wave keeps in flight"""
    from test_kernel_resources_cpu import kernel_resources
    res = {k: v for k, v in kernel_resources("knn_range.hip").items() if "knn_plane_rangeI" in k}
    assert len(res) == 8, sorted(res)
    assert all(scratch == 0 for scratch, _ in res.values()), res
    assert all(vgpr <= 256 for _, vgpr in res.values()), res
