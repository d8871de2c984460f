"""GPU suite: the kernels that turn kNN hits and head outputs into what predict() returns, called through the C ABI and held
to tests/predict_tail_ref.py (numpy fp64 / Python floats, anchored in tests/test_predict_tail_ref_cpu.py) at the sizes
where such kernels go wrong: one class, the two sides of the 64-lane stride, several strides, the largest supported size;
a lone wave, a full and a partial four-wave workgroup; saturating, underflowing, tied and padded rows.

  prelude kernels (ac_softmax_rows, ac_sigmoid, ac_proto_scores, ac_l2_normalize_rows)   1e-6 absolute against fp64
  ac_rows_to_class                                                                        exact
  ac_blend_topk          same class order (ties included), out_n equal, scores to 1e-12, nothing written past out_n
  ac_predict_post        byte for byte the chain of the four kernels above, so their results carry over to it
"""
import ctypes

import numpy as np
import pytest
import torch

import predict_tail_ref as R

pytestmark = pytest.mark.gpu

WORST = {}


def _note(kernel, err):
    if float(err) > WORST.get(kernel, -1.0):
        WORST[kernel] = float(err)
        print(f"MEASURED {kernel} worst |device - fp64| so far {WORST[kernel]:.3e}")


@pytest.fixture(scope="module")
def nat(cuda_dev):
    from adaptive_classifier import _native as nv
    return nv, nv.lib(), nv.stream_ptr(cuda_dev)


def _logit_rows(kind, B, C, rng):
    if kind == "unit":
        return rng.standard_normal((B, C)).astype(np.float32)
    if kind == "pm80":
        return rng.choice(np.array([-80.0, 80.0], np.float32), (B, C))
    if kind == "spike":                                                       # one logit 1e4 above the rest
        Z = rng.standard_normal((B, C)).astype(np.float32)
        Z[np.arange(B), rng.integers(0, C, B)] += np.float32(1e4)
        return Z
    return np.repeat(rng.standard_normal((B, 1)).astype(np.float32), C, axis=1)   # fully tied rows


@pytest.mark.parametrize("C", [1, 2, 63, 64, 65, 257, 2048])
def test_softmax_and_sigmoid_against_fp64(C, nat, cuda_dev):
    nv, lib, sp = nat
    rng = np.random.default_rng(100 + C)
    for B in (1, 3, 4, 5):
        for kind in ("unit", "pm80", "spike", "tied"):
            Z = _logit_rows(kind, B, C, rng)
            z = torch.from_numpy(Z).to(cuda_dev)
            out = torch.full((B + 1, C), -7.0, device=cuda_dev)               # (a sentinel row behind the last one)
            nv.check(lib.ac_softmax_rows(nv.ptr(z), B, C, nv.ptr(out), sp), "ac_softmax_rows")
            got = out.cpu().numpy()
            assert (got[B] == -7.0).all(), (B, kind)
            err = np.abs(got[:B].astype(np.float64) - R.softmax_rows(Z)).max()
            _note("ac_softmax_rows", err)
            assert err <= R.PRELUDE_ATOL, (B, kind, err)
            if kind == "tied":
                assert (got[:B] == got[:B, :1]).all()
            out = torch.full((B * C + 1,), -7.0, device=cuda_dev)
            nv.check(lib.ac_sigmoid(nv.ptr(z), B * C, nv.ptr(out), sp), "ac_sigmoid")
            got = out.cpu().numpy()
            assert got[B * C] == -7.0
            err = np.abs(got[:B * C].astype(np.float64) - R.sigmoid(Z).reshape(-1)).max()
            _note("ac_sigmoid", err)
            assert err <= R.PRELUDE_ATOL, (B, kind, err)


@pytest.mark.parametrize("k", [1, 63, 64, 65, 1024])
def test_proto_scores_against_fp64(k, nat, cuda_dev):
    nv, lib, sp = nat
    rng = np.random.default_rng(200 + k)
    flt_max = np.float32(R.FLT_MAX)
    pad = rng.random(k) < 0.3
    pad[rng.integers(0, k)] = False                                           # (at least one valid hit where padding is mixed in)
    rows = []                                                                 # (distances, ids)
    ids = lambda: rng.integers(0, 10 ** 6, k)
    rows.append((np.zeros(k, np.float32), ids()))                             # distances 0: uniform
    rows.append((np.sort(rng.random(k).astype(np.float32) * 2), ids()))       # around 1, all valid
    d = np.sort(rng.random(k).astype(np.float32) * 2)
    rows.append((np.where(pad, flt_max, d), np.where(pad, -1, ids())))        # around 1, padding carrying FLT_MAX
    d = (200 + rng.random(k) * 300).astype(np.float32)
    rows.append((np.where(pad, flt_max, d), np.where(pad, -1, ids())))        # exp(-d) = 0 in fp32: uniform over the valid hits
    rows.append((np.full(k, flt_max), np.full(k, -1)))                        # all padding
    one = rng.integers(0, k)
    rows.append((np.where(np.arange(k) == one, np.float32(0.7), flt_max), np.where(np.arange(k) == one, 5, -1)))   # one valid hit
    D = np.stack([r[0] for r in rows]).astype(np.float32)
    I = np.stack([r[1] for r in rows]).astype(np.int64)
    nq = len(rows)
    out = torch.full((nq + 1, k), -7.0, device=cuda_dev)
    D_d, I_d = torch.from_numpy(D).to(cuda_dev), torch.from_numpy(I).to(cuda_dev)
    nv.check(lib.ac_proto_scores(nv.ptr(D_d), nv.ptr(I_d), nq, k, nv.ptr(out), sp), "ac_proto_scores")
    got = out.cpu().numpy()
    assert (got[nq] == -7.0).all()
    got = got[:nq]
    err = np.abs(got.astype(np.float64) - R.proto_scores(D, I)).max()
    _note("ac_proto_scores", err)
    assert err <= R.PRELUDE_ATOL, err
    assert (got[I < 0] == 0).all() and (got[4] == 0).all() and got[5, one] == 1.0
    assert (got[0] == got[0, 0]).all() and abs(float(got[0, 0]) * k - 1) <= 1e-6 * k
    valid = ~pad
    assert (got[3][valid] == got[3][valid][0]).all() and abs(float(got[3][valid][0]) * valid.sum() - 1) <= 1e-6 * k


@pytest.mark.parametrize("D", [1, 63, 64, 65, 768, 4096])
def test_l2_normalize_rows_against_fp64_with_padded_rows(D, nat, cuda_dev):
    nv, lib, sp = nat
    rng = np.random.default_rng(300 + D)
    B = 5
    X = rng.standard_normal((B, D))
    X[1] = 0
    X[2] *= 1e-20 / np.linalg.norm(X[2])
    X[3] *= 1e15 / np.linalg.norm(X[3])
    X = X.astype(np.float32)
    want = R.l2_normalize_rows(X)
    for ldi, ldo in ((D, D), (D + 3, D + 5), (D + 64, D + 1)):
        for nb in (1, 3, 4, 5):
            src = torch.full((B, ldi), 123.0, device=cuda_dev)
            src[:, :D] = torch.from_numpy(X).to(cuda_dev)
            out = torch.full((B + 1, ldo), -7.0, device=cuda_dev)
            nv.check(lib.ac_l2_normalize_rows(nv.ptr(src), ldi, nb, D, nv.ptr(out), ldo, sp), "ac_l2_normalize_rows")
            got = out.cpu().numpy()
            assert (got[:, D:] == -7.0).all() and (got[nb:] == -7.0).all(), (ldi, ldo, nb)     # bytes between and behind the rows
            assert (src.cpu().numpy()[:, D:] == 123.0).all()
            err = np.abs(got[:nb, :D].astype(np.float64) - want[:nb]).max()
            _note("ac_l2_normalize_rows", err)
            assert err <= R.PRELUDE_ATOL, (ldi, ldo, nb, err)
            if nb > 1:
                assert (got[1, :D] == 0).all()


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_rows_to_class_is_exact(n, nat, cuda_dev):
    nv, lib, sp = nat
    rng = np.random.default_rng(400 + n)
    nrows, nlut = 1000, 40
    row_class = rng.integers(-1, nlut + 6, nrows).astype(np.int32)            # (-1 and values past the LUT included)
    row_class[[0, nrows - 1]] = [3, nlut - 1]
    lut = rng.integers(0, 30, nlut).astype(np.int64)
    lut[[1, 5, nlut - 1]] = -1
    special = np.array([-1, nrows - 1, nrows, 0, 2 ** 40, -(2 ** 40), 2 ** 31, 2 ** 32 + 5, nrows + 1, 1, 5], np.int64)
    rc_d, lut_d = torch.from_numpy(row_class).to(cuda_dev), torch.from_numpy(lut).to(cuda_dev)
    starts = range(len(special)) if n == 1 else (0,)                          # n = 1: every special id in turn
    for s in starts:
        I = rng.integers(-3, nrows + 3, n).astype(np.int64)
        m = min(n, len(special))
        I[:m] = np.roll(special, -s)[:m]
        I_d = torch.from_numpy(I).to(cuda_dev)
        for use_rc in (True, False):
            for use_lut in (True, False):
                # without a row map the row id itself goes through the LUT: the valid ids are then [0, nrows) all the same
                out = torch.full((n + 1,), -7, dtype=torch.int64, device=cuda_dev)
                nv.check(lib.ac_rows_to_class(nv.ptr(I_d), n, nv.ptr(rc_d) if use_rc else None, nrows, nv.ptr(lut_d) if use_lut else None,
                                              nlut if use_lut else 0, nv.ptr(out), sp), "ac_rows_to_class")
                got = out.cpu().numpy()
                want = R.rows_to_class(I, row_class if use_rc else None, nrows, lut if use_lut else None, nlut if use_lut else 0)
                assert got[n] == -7 and np.array_equal(got[:n], want), (s, use_rc, use_lut)


# ---- ac_blend_topk -------------------------------------------------------------------------------------------------------------
def _blend_inputs(C, kp, rng):
    """Five queries: random; all hits padded; all hits in one class; every head probability tied; a hit class (the LAST class)
    tying a head-only class (class 0) at the same combined score, from exactly representable values under weights 1."""
    b = 5
    S = rng.random((b, kp)).astype(np.float32)
    S[:, 1:] = np.minimum.accumulate(S, axis=1)[:, 1:]
    Cid = rng.integers(-1, C + 2, (b, kp)).astype(np.int64)                   # -1 and ids >= C: no class
    P = rng.random((b, C)).astype(np.float32)
    P /= P.sum(1, keepdims=True)
    Cid[1] = -1
    Cid[2] = C // 2
    P[3] = np.float32(1.0 / C)
    S[4], Cid[4], P[4] = 0.25, -1, 0.0
    S[4, 0], Cid[4, 0] = 0.5, C - 1
    P[4, 0] = 0.5
    if C > 2:
        P[4, 1] = 0.25                                                        # ... and a head class below the tie
    w = rng.choice([0.3, 0.7], size=(2, C))
    w[:, [0, C - 1]] = 1.0
    return S, Cid, P, w[0].copy(), w[1].copy()


def _run_blend(nat, dev, S, Cid, P, wp, wh, kp, C, ncls, k, b):
    nv, lib, sp = nat
    n = torch.full((b + 1,), -9, dtype=torch.int32, device=dev)
    cls = torch.full((b + 1, k), -7, dtype=torch.int32, device=dev)
    val = torch.full((b + 1, k), -7.0, dtype=torch.float64, device=dev)
    nv.check(lib.ac_blend_topk(nv.ptr(S), nv.ptr(Cid), kp if S is not None else 0, nv.ptr(P), C, nv.ptr(wp), nv.ptr(wh), ncls, k, b,
                               nv.ptr(n), nv.ptr(cls), nv.ptr(val), sp), "ac_blend_topk")
    n, cls, val = n.cpu().numpy(), cls.cpu().numpy(), val.cpu().numpy()
    assert n[b] == -9 and (cls[b] == -7).all() and (val[b] == -7.0).all()     # nothing behind the last query
    return n[:b], cls[:b], val[:b]


@pytest.mark.parametrize("C", [1, 2, 63, 64, 65, 128, 2047, 2048])
def test_blend_topk_equals_the_reference_formula(C, nat, cuda_dev):
    rng = np.random.default_rng(500 + C)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda_dev)
    for kp in (1, 63, 64, 65):
        S, Cid, P, wp, wh = _blend_inputs(C, kp, rng)
        Sd, Cd, Pd, wpd, whd = dev(S), dev(Cid), dev(P), dev(wp), dev(wh)
        for ncls in (0, 1, C, C + 5):
            for use_s, use_p in ((True, True), (True, False), (False, True)):
                full = R.blend_topk(S if use_s else None, Cid if use_s else None, P if use_p else None, wp, wh, ncls, C + 3)
                if use_s and use_p and ncls >= 1 and C > 1:                   # the planted tie: the hit class ahead of the head-only class
                    assert [c for c, _ in full[4][:2]] == [C - 1, 0] and full[4][0][1] == full[4][1][1]
                for k, b in sorted({(k, b) for k in (1, C, C + 3) for b in (1, 5)}):     # (the reference's lists for smaller k / b are prefixes)
                    n, cls, val = _run_blend(nat, cuda_dev, Sd if use_s else None, Cd if use_s else None, Pd if use_p else None, wpd, whd,
                                             kp, C, ncls, k, b)
                    try:
                        err = R.check_blend([w[:k] for w in full[:b]], n, cls, val, -7, -7.0)
                    except AssertionError as e:
                        raise AssertionError(f"C={C} kp={kp} ncls_head={ncls} hits={use_s} head={use_p} k={k} b={b}: {e}") from None
                    WORST["ac_blend_topk"] = max(WORST.get("ac_blend_topk", 0.0), err)
        # all-zero weights: the total is 0, scores stay unnormalised (0), order = insertion order
        zero = torch.zeros(C, dtype=torch.float64, device=cuda_dev)
        full = R.blend_topk(S, Cid, P, np.zeros(C), np.zeros(C), C, C + 3)
        assert all(s == 0.0 for w in full for _, s in w)
        n, cls, val = _run_blend(nat, cuda_dev, Sd, Cd, Pd, zero, zero, kp, C, C, C + 3, 5)
        R.check_blend(full, n, cls, val, -7, -7.0)
    print(f"MEASURED ac_blend_topk worst |device - reference| so far {WORST.get('ac_blend_topk', 0.0):.3e}")


# ---- ac_predict_post against the chain it replaces -------------------------------------------------------------------------------
class _HostBuf:
    def __init__(self, nv, lib, nbytes):
        self.nv, self.lib, self.p = nv, lib, ctypes.c_void_p()
        nv.check(lib.ac_host_alloc(nbytes, ctypes.byref(self.p)), "ac_host_alloc")
        self.view = np.frombuffer((ctypes.c_ubyte * nbytes).from_address(self.p.value), dtype=np.uint8)

    def free(self):
        self.view = None
        self.nv.check(self.lib.ac_host_free(self.p), "ac_host_free")


def _layout(b, k):
    off_cls = 4 * b
    off_val = (off_cls + 4 * b * k + 7) // 8 * 8
    return off_cls, off_val, off_val + 8 * b * k, (off_val + 8 * b * k + 15) // 16 * 16


def _chain(nat, dev, Dd, Id, rc, nrows, lt, nlut, Zd, head_softmax, wts, C, kp, ncls, k, b):
    """ac_proto_scores -> ac_rows_to_class -> ac_softmax_rows -> ac_blend_topk into a 0x5C-filled packed buffer."""
    nv, lib, sp = nat
    off_cls, off_val, _, need = _layout(b, k)
    S = Cid = P = None
    if Dd is not None:
        S = torch.empty_like(Dd)
        nv.check(lib.ac_proto_scores(nv.ptr(Dd), nv.ptr(Id), b, kp, nv.ptr(S), sp), "ac_proto_scores")
        Cid = torch.empty_like(Id)
        nv.check(lib.ac_rows_to_class(nv.ptr(Id), Id.numel(), nv.ptr(rc), nrows, nv.ptr(lt), nlut, nv.ptr(Cid), sp), "ac_rows_to_class")
    if Zd is not None:
        P = Zd
        if head_softmax:
            P = torch.empty_like(Zd)
            nv.check(lib.ac_softmax_rows(nv.ptr(Zd), b, C, nv.ptr(P), sp), "ac_softmax_rows")
    want = torch.full((need,), 0x5C, dtype=torch.uint8, device=dev)
    base = want.data_ptr()
    nv.check(lib.ac_blend_topk(nv.ptr(S), nv.ptr(Cid), kp if S is not None else 0, nv.ptr(P), C, nv.ptr(wts[0]), nv.ptr(wts[1]), ncls, k, b,
                               base, base + off_cls, base + off_val, sp), "ac_blend_topk")
    return want.cpu().numpy()


def _same_packed(got, want, b, k, tag):
    """Byte for byte where n[q] says data was written; the rest of `got` still holds the 0x5C both buffers were filled with."""
    off_cls, off_val, end, _ = _layout(b, k)
    n = want[:off_cls].view(np.int32)
    assert np.array_equal(got[:off_cls], want[:off_cls]), (tag, got[:off_cls].view(np.int32), n)
    gc, wc = (a[off_cls:off_cls + 4 * b * k].view(np.int32).reshape(b, k) for a in (got, want))
    gv, wv = (a[off_val:off_val + 8 * b * k].view(np.uint64).reshape(b, k) for a in (got, want))
    written = np.arange(k)[None, :] < n[:, None]
    assert np.array_equal(gc[written], wc[written]) and np.array_equal(gv[written], wv[written]), tag
    assert (gc[~written] == 0x5C5C5C5C).all() and (gv[~written] == 0x5C5C5C5C5C5C5C5C).all(), tag
    assert (got[off_cls + 4 * b * k:off_val] == 0x5C).all(), tag


def _post_inputs(C, kp, b, rng, dev):
    nrows, nlut = 5000, C + 3
    D = np.sort(rng.random((b, kp)).astype(np.float32) * 2, axis=1)
    I = rng.integers(-1, nrows + 40, (b, kp)).astype(np.int64)
    I[::3, : max(1, kp // 2)] = rng.integers(0, min(C, nrows), (len(I[::3]), max(1, kp // 2)))     # (ids that are classes with no map at all)
    if b > 2:
        I[2] = -1
    row_class = rng.integers(0, nlut, nrows).astype(np.int32)
    lut = np.concatenate([rng.permutation(C), [-1, -1, -1]]).astype(np.int64)[rng.permutation(nlut)]
    Z = (rng.standard_normal((b, C)) * 3).astype(np.float32)
    if b > 3:
        Z[3] = 0.5
    wts = torch.tensor(rng.choice([0.3, 0.7], size=(2, C)), dtype=torch.float64, device=dev)
    t = lambda a: torch.from_numpy(a).to(dev)
    return t(D), t(I), t(row_class), nrows, t(lut), nlut, t(Z), wts


def _post(nat, dev, Dd, Id, rc, nrows, lt, nlut, Zd, head_softmax, wts, C, kp, ncls, k, b, host):
    """One ac_predict_post call into 0x5C-filled buffers -> the packed bytes (host-mapped buffer when given, else the device's)."""
    nv, lib, sp = nat
    need = _layout(b, k)[3]
    got_d = torch.full((need,), 0x5C, dtype=torch.uint8, device=dev)
    if host is not None:
        host.view[:] = 0xAB
    nv.check(lib.ac_predict_post(nv.ptr(Dd), nv.ptr(Id), kp, nv.ptr(rc), nrows, nv.ptr(lt), nlut, nv.ptr(Zd), C,
                                 head_softmax, nv.ptr(wts[0]), nv.ptr(wts[1]), ncls, k, b, nv.ptr(got_d), need,
                                 host.p if host is not None else None, sp), "ac_predict_post")
    return host.view[:need].copy() if host is not None else got_d.cpu().numpy()      # (host buffer: no synchronisation by the caller)


POST_SHAPES = [  # b, C, kp, k
    (1, 37, 16, 3),        # b = 1, k = 3: the packed result is 5 eight-byte words (odd: the last 16-byte store is half past the end)
    (4, 37, 16, 5), (5, 37, 16, 5),
    (257, 37, 16, 5),      # 16448 bytes = 1028 sixteen-byte stores: three passes of the last workgroup's 512-store copy loop
    (5, 1, 1, 1), (5, 63, 63, 63), (5, 64, 64, 64), (5, 65, 65, 65), (5, 2048, 1024, 3)]


@pytest.mark.parametrize("b,C,kp,k", POST_SHAPES)
def test_predict_post_equals_the_chain_at_the_edges(b, C, kp, k, nat, cuda_dev):
    """Every combination of: row map / class LUT present or NULL, hits + head / hits only / head only, the head's outputs as
    logits (head_softmax = 1) or as probabilities (0), host-waited or asynchronous."""
    nv, lib, sp = nat
    rng = np.random.default_rng(b * 100003 + C * 7 + kp)
    Dd, Id, rc, nrows, lt, nlut, Zd, wts = _post_inputs(C, kp, b, rng, cuda_dev)
    Pd = torch.from_numpy(R.softmax_rows(Zd.cpu().numpy()).astype(np.float32)).to(cuda_dev)
    assert _layout(1, 3)[2] // 8 % 2 == 1 and (_layout(257, 5)[2] + 15) // 16 > 2 * 512
    host = _HostBuf(nv, lib, _layout(b, k)[3])
    try:
        for use_rc, use_lut in ((True, True), (False, True), (True, False), (False, False)):
            maps = (rc if use_rc else None, nrows, lt if use_lut else None, nlut if use_lut else 0)
            for hits, head in ((True, True), (True, False), (False, True)):
                if not hits and (use_rc, use_lut) != (True, True):
                    continue                                                 # (the maps play no part without hits)
                for head_softmax in ((1, 0) if head else (1,)):
                    for ncls in (C, min(k, C)):
                        H = None if not head else (Zd if head_softmax else Pd)
                        args = (Dd if hits else None, Id if hits else None, *maps, H, head_softmax, wts, C, kp, ncls, k, b)
                        want = _chain(nat, cuda_dev, *args)
                        for h in (host, None):
                            _same_packed(_post(nat, cuda_dev, *args, h), want, b, k, (use_rc, use_lut, hits, head, head_softmax, ncls, h is not None))
    finally:
        host.free()


def test_predict_post_seventy_host_waited_calls_reuse_a_completion_slot(nat, cuda_dev):
    """The host-waited form hands out 64 completion slots round-robin: 70 calls in a row on one stream use at least six of them
    a second time.  Every call has inputs of its own and its result is checked against the chain's."""
    nv, lib, sp = nat
    b, C, kp, k = 4, 37, 16, 5
    rng = np.random.default_rng(70)
    calls = [_post_inputs(C, kp, b, rng, cuda_dev) for _ in range(70)]
    wants = [_chain(nat, cuda_dev, Dd, Id, rc, nrows, lt, nlut, Zd, 1, wts, C, kp, C, k, b) for Dd, Id, rc, nrows, lt, nlut, Zd, wts in calls]
    assert len({w.tobytes() for w in wants}) == 70
    host = _HostBuf(nv, lib, _layout(b, k)[3])
    try:
        for i, (Dd, Id, rc, nrows, lt, nlut, Zd, wts) in enumerate(calls):
            _same_packed(_post(nat, cuda_dev, Dd, Id, rc, nrows, lt, nlut, Zd, 1, wts, C, kp, C, k, b, host), wants[i], b, k, i)
    finally:
        host.free()
