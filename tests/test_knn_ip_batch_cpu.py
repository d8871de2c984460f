"""CPU suite of the inner-product search over a prepared store (ac_knn_ip_topk_batch, `knn_ip_topk(..., prepared=)`, the
HipFlatIPIndex preparation policy): the host-only parts of the C ABI and the host bookkeeping, as far as they run without a
device.  The kernels themselves: tests/test_knn_ip_batch_gpu.py."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ac_knn_ip_topk_batch_workspace", "ac_knn_ip_topk_batch")


def test_ip_batch_symbols_in_header_exports_and_ctypes_table():
    from adaptive_classifier import _native as nv
    L = nv.lib()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "acamd.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(ac_[a-z0-9_]+)\s*\(", src))
    for name in NEW:
        assert name in declared, name + " not declared in acamd.h"
        assert hasattr(L, name), name + " not exported by libacamd.so"
        assert name in nv.exported_symbols(), name + " missing from the ctypes table"
    # same argument list as the L2 namesakes
    assert getattr(L, NEW[1]).argtypes == L.ac_knn_l2_topk_batch.argtypes
    assert getattr(L, NEW[0]).argtypes == L.ac_knn_l2_topk_batch_workspace.argtypes


def test_abi_version_is_3():
    from adaptive_classifier import _native as nv
    assert nv.lib().ac_version() >= 3


def test_ip_batch_workspace_planner_is_the_l2_batch_planner():
    from adaptive_classifier import _native as nv
    L = nv.lib()
    for N, D, nq, k in [(10_000_000, 768, 4096, 32), (100_000, 768, 16, 16)]:
        a, b = ctypes.c_size_t(0), ctypes.c_size_t(0)
        assert L.ac_knn_ip_topk_batch_workspace(N, D, nq, k, ctypes.byref(a)) == 0
        assert L.ac_knn_l2_topk_batch_workspace(N, D, nq, k, ctypes.byref(b)) == 0
        assert a.value == b.value > 0


def test_ip_batch_validation_without_gpu():
    from adaptive_classifier import _native as nv
    L = nv.lib()
    b = ctypes.c_size_t(0)
    assert L.ac_knn_ip_topk_batch_workspace(65_535, 768, 256, 16, ctypes.byref(b)) == -2      # AC_EUNSUPPORTED: N < 65536
    assert L.ac_knn_ip_topk_batch_workspace(100_000, 768, 256, 101, ctypes.byref(b)) == -2    # ... k > 100
    assert L.ac_knn_ip_topk_batch_workspace(100_000, 768, 256, 16, None) == -1                # AC_EINVAL: NULL bytes
    assert L.ac_knn_ip_topk_batch_workspace(65_536, 768, 256, 100, ctypes.byref(b)) == 0 and b.value > 0
    # the search entry point refuses the same shapes before it touches any pointer or the device
    args = lambda N, k: (None, N, 768, 768, None, None, None, 256, 768, k, 0, None, None, None, None, 0, None, None)
    assert L.ac_knn_ip_topk_batch(*args(65_535, 16)) == -2
    assert L.ac_knn_ip_topk_batch(*args(100_000, 101)) == -2
    assert L.ac_knn_ip_topk_batch(*args(100_000, 16)) == -1                                   # null pointers


def test_prepared_ip_search_fails_loudly_without_gpu():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from adaptive_classifier import _native as nv
    from adaptive_classifier import index as ix
    P = torch.zeros((70_000, 8))
    Q = torch.zeros((4, 8))
    prepared = (torch.zeros(8, dtype=torch.int16), torch.zeros(8))
    with pytest.raises(nv.NativeError):
        ix.knn_ip_topk(P, 70_000, 8, Q, 2, prepared=prepared)
    with pytest.raises(nv.NativeError):
        ix.knn_ip_topk_exact(P, 70_000, 8, Q, 2, prepared=prepared)


def test_ip_index_preparation_policy_host_side(monkeypatch):
    """The policy of `_HipFlatIndex.search_device` with the device calls replaced by recorders: an IP index prepares its plane
    only on a many-query search (>= BATCH_MIN_QUERIES queries and N * nq >= BATCH_MIN_PAIRS), never on the "second small
    search" rule the L2 index has; once a plane exists small batches on >= PLANE_MIN_ROWS rows use it; remove_ids / reset drop
    it."""
    from adaptive_classifier import index as ix
    calls = []

    def fake_prepare(P, N, D, capacity=None):
        calls.append(("prepare", N))
        return ("planes", "norms")

    def fake_search(name):
        def f(P, N, D, Q, k, workspace=None, stats=None, prepared=None, **kw):
            calls.append((name, Q.shape[0], prepared is not None))
            return None, None
        return f
    monkeypatch.setattr(ix, "prepare_store", fake_prepare)
    monkeypatch.setattr(ix, "knn_ip_topk", fake_search("ip"))
    monkeypatch.setattr(ix, "knn_l2_topk", fake_search("l2"))
    monkeypatch.setattr(ix, "knn_workspace_bytes", lambda *a: 0)
    monkeypatch.setattr(ix, "knn_batch_workspace_bytes", lambda *a: 0)

    def index(cls, n):
        idx = cls(8, device="cpu")
        idx._materialize = lambda: None                   # the rows are "resident": no upload
        idx._store, idx._n = torch.zeros((n, 8)), n
        idx._ws = torch.zeros(256, dtype=torch.uint8)
        return idx
    N = ix.PLANE_MIN_ROWS + 1000
    small, many = torch.zeros((4, 8)), torch.zeros((128, 8))
    assert float(N) * 128 >= ix.BATCH_MIN_PAIRS and 128 >= ix.BATCH_MIN_QUERIES

    ip = index(ix.HipFlatIPIndex, N)
    for _ in range(3):
        ip.search_device(small, 5)
    assert ip._prepared is None and calls == [("ip", 4, False)] * 3      # never from small searches
    ip.search_device(many, 5)
    assert ip._prepared is not None and calls[3:] == [("prepare", N), ("ip", 128, True)]
    ip.search_device(small, 5)
    assert calls[-1] == ("ip", 4, True)                                  # the plane exists: small batches use it
    ip._store = torch.zeros((N, 8)); ip._n = N
    ip.reset()
    assert ip._prepared is None

    del calls[:]
    l2 = index(ix.HipFlatL2Index, N)                                     # the L2 rule is unchanged: second small search prepares
    l2.search_device(small, 5)
    assert l2._prepared is None
    l2.search_device(small, 5)
    assert l2._prepared is not None and calls == [("l2", 4, False), ("prepare", N), ("l2", 4, True)]

    del calls[:]
    few = index(ix.HipFlatIPIndex, 100_000)                              # many queries but too few pairs: the fp32 sweep
    few.search_device(torch.zeros((64, 8)), 5)
    assert few._prepared is None and calls == [("ip", 64, False)]
    tiny = index(ix.HipFlatIPIndex, 1000)                                # below the library's limits
    tiny.search_device(many, 5)
    assert tiny._prepared is None and calls[-1] == ("ip", 128, False)
