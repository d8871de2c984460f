"""GPU suite: the remaining stream-taking entries and two whole objects on a non-default stream (tests/stream_lag.py).

Entries no table case of the other stream modules reaches, each by its smallest direct call against a plain fp64 reference:
  ac_linear_f32        200 x 136 x 96, bias + residual; |got - fp64| <= 1e-4 (tests/test_head_gpu.py's bar for the fp32 GEMMs)
  ac_gemm_f32          C = 0.5 A^T B + 2 C, 33 x 20 x 50; the same bar
  ac_split_bf16x3      planes of the live activations: h + m + l == x to 2^-24 |x| (three 8-bit significands)
  ac_linear_bf16x3     both operands pre-split (M >= 192, K % 32 == 0: the ring-staged kernel); the fp32 bar
  ac_split_f16x2       h + l == x 2^s to max(2^-22 |x 2^s|, 2^-25) (tests/test_gemm_f16x2_gpu.py's statement of the format)
  ac_linear_f16x2      (3.5 x 2^-22 + (3 K / 16 + 4) 2^-24) |A| |W|^T + 1e-6, the bound tests/test_gemm_f16x2_gpu.py derives
  ac_synth_unit_rows   bit-identical to oracle/synth.py (no input to arrive late)
  ac_clock_stamp       two stamps on the stream: the 100 MHz counter does not run backwards on any XCD both saw; the values are
                       times, so this case has no bit comparison
Late input: the activation matrix A (stale: another seed); the weights are setup.

Whole objects, scenarios A and B at the outer level (a leading sleep, no late inputs -- the objects make their own), each result
bit-identical to the same life of a FRESH object on the default stream:
  classifier life   the golden bert-mini classifier (tests/golden/e2e_bert_mini): add_examples, predict, predict_batch, a new
                    class, predict again; once with the device tokenizer and once with the wrapped host tokenizer.

HOST_WAITS, read from csrc/gemm.hip, gemm_pipe.hip, synth.hip, common.hip: (none of these entries waits on the host).
"""
import json
import os
import time
import types

import numpy as np
import pytest
import torch

import poison
import stream_lag as sl

pytestmark = pytest.mark.gpu

_T0 = time.time()
HOST_WAITS = {}
M_, N_, K_ = 200, 136, 96
TOL = 1e-4


def _unplane(planes, n_planes, rows, K):
    """[p][K / 8][row][8] uint16 -> [p, rows, K] uint16"""
    return planes.view(np.uint16)[: n_planes * rows * K].reshape(n_planes, K // 8, rows, 8).transpose(0, 2, 1, 3).reshape(n_planes, rows, K)


def _gemm_cases(dev):
    from adaptive_classifier import _native as nv
    rng = np.random.default_rng(5)
    A = rng.standard_normal((M_, K_)).astype(np.float32)
    A2 = rng.standard_normal((M_, K_)).astype(np.float32)
    W = (rng.standard_normal((N_, K_)) / np.sqrt(K_)).astype(np.float32)
    b = rng.standard_normal(N_).astype(np.float32)
    R = rng.standard_normal((M_, N_)).astype(np.float32)
    Ad, As, Wd, bd, Rd = (torch.from_numpy(x).to(dev) for x in (A, A2, W, b, R))
    want = A.astype(np.float64) @ W.astype(np.float64).T + b
    S = np.abs(A).astype(np.float64) @ np.abs(W).astype(np.float64).T
    lib = nv.lib()
    Wp3 = torch.empty(3 * N_ * K_, dtype=torch.int16, device=dev)
    nv.check(lib.ac_split_bf16x3(nv.ptr(Wd), K_, N_, K_, nv.ptr(Wp3), nv.stream_ptr(dev)), "ac_split_bf16x3")
    Wp2 = torch.empty(2 * N_ * K_, dtype=torch.int16, device=dev)
    nv.check(lib.ac_split_f16x2(nv.ptr(Wd), K_, N_, K_, 10, nv.ptr(Wp2), nv.stream_ptr(dev)), "ac_split_f16x2")
    # ac_gemm_f32: A^T B with A [K2, M2], B [K2, N2]
    M2, N2, K2 = 33, 20, 50
    G = rng.standard_normal((K2, M2)).astype(np.float32)
    G2 = rng.standard_normal((K2, M2)).astype(np.float32)
    H = rng.standard_normal((K2, N2)).astype(np.float32)
    C0 = rng.standard_normal((M2, N2)).astype(np.float32)
    Gd, Gs, Hd, C0d = (torch.from_numpy(x).to(dev) for x in (G, G2, H, C0))
    want_g = 0.5 * (G.T.astype(np.float64) @ H.astype(np.float64)) + 2.0 * C0.astype(np.float64)

    def linear_f32():
        C = torch.empty((M_, N_), device=dev)
        nv.check(lib.ac_linear_f32(nv.ptr(Ad), K_, nv.ptr(Wd), K_, nv.ptr(bd), nv.ptr(Rd), N_, nv.ptr(C), N_, M_, N_, K_, 0,
                                   nv.stream_ptr(dev)), "ac_linear_f32")
        return [C]

    def gemm_f32():
        C = C0d.clone()
        nv.check(lib.ac_gemm_f32(1, 0, M2, N2, K2, 0.5, nv.ptr(Gd), M2, nv.ptr(Hd), N2, 2.0, nv.ptr(C), N2, nv.stream_ptr(dev)), "ac_gemm_f32")
        return [C]

    def bf16x3():
        Ap = torch.empty(3 * M_ * K_, dtype=torch.int16, device=dev)
        nv.check(lib.ac_split_bf16x3(nv.ptr(Ad), K_, M_, K_, nv.ptr(Ap), nv.stream_ptr(dev)), "ac_split_bf16x3")
        C = torch.empty((M_, N_), device=dev)
        nv.check(lib.ac_linear_bf16x3(nv.ptr(Ad), K_, nv.ptr(Ap), nv.ptr(Wd), K_, nv.ptr(Wp3), nv.ptr(bd), None, 0, nv.ptr(C), N_, None,
                                      M_, N_, K_, 0, nv.stream_ptr(dev)), "ac_linear_bf16x3")
        return [Ap, C]

    def f16x2():
        Ap = torch.empty(2 * M_ * K_, dtype=torch.int16, device=dev)
        nv.check(lib.ac_split_f16x2(nv.ptr(Ad), K_, M_, K_, 6, nv.ptr(Ap), nv.stream_ptr(dev)), "ac_split_f16x2")
        C = torch.empty((M_, N_), device=dev)
        nv.check(lib.ac_linear_f16x2(nv.ptr(Ap), nv.ptr(Wp2), nv.ptr(bd), None, 0, nv.ptr(C), N_, None, M_, N_, K_, 0, nv.stream_ptr(dev)),
                 "ac_linear_f16x2")
        return [Ap, C]

    def check_linear(got):
        assert np.abs(got[0] - (want + R)).max() <= TOL

    def check_gemm(got):
        assert np.abs(got[0] - want_g).max() <= TOL

    def check_bf16x3(got):
        pl = _unplane(got[0], 3, M_, K_)
        back = (pl.astype(np.uint32) << 16).view(np.float32).astype(np.float64).sum(0)
        assert np.all(np.abs(back - A) <= 2.0 ** -24 * np.abs(A))
        assert np.abs(got[1] - want).max() <= TOL

    def check_f16x2(got):
        hl = _unplane(got[0], 2, M_, K_).view(np.float16).astype(np.float64)
        xs = A.astype(np.float64) * 2.0 ** 6
        assert np.all(np.abs(xs - hl[0] - hl[1]) <= np.maximum(2.0 ** -22 * np.abs(xs), 2.0 ** -25))
        assert np.all(np.abs(got[1] - want) <= (3.5 * 2.0 ** -22 + (3 * K_ / 16 + 4) * 2.0 ** -24) * S + 1e-6)

    C_ = types.SimpleNamespace
    return {"linear_f32": C_(live=[Ad], stale=[As], run=linear_f32, check=check_linear, bits=True),
            "gemm_f32": C_(live=[Gd], stale=[Gs], run=gemm_f32, check=check_gemm, bits=True),
            "split_and_linear_bf16x3": C_(live=[Ad], stale=[As], run=bf16x3, check=check_bf16x3, bits=True),
            "split_and_linear_f16x2": C_(live=[Ad], stale=[As], run=f16x2, check=check_f16x2, bits=True)}


def _synth_case(dev):
    from adaptive_classifier import index as ix
    from oracle import synth

    def check(got):
        assert np.array_equal(got[0][:, :24], synth.synth_unit_rows(301, 24, 13, row_offset=7))
    return types.SimpleNamespace(live=[], stale=[], run=lambda: [ix.synth_unit_rows(301, 24, 13, device=dev, row_offset=7)], check=check, bits=True)


def _clock_case(dev):
    from adaptive_classifier import _native as nv

    def run():
        a, b = torch.empty(16, dtype=torch.int64, device=dev), torch.empty(16, dtype=torch.int64, device=dev)
        nv.check(nv.lib().ac_clock_stamp(nv.ptr(a), nv.stream_ptr(dev)), "ac_clock_stamp")
        nv.check(nv.lib().ac_clock_stamp(nv.ptr(b), nv.stream_ptr(dev)), "ac_clock_stamp")
        return [a, b]

    def check(got):
        a, b = (g.view(np.uint64).reshape(8, 2) for g in got)
        both = (a[:, 1] != 0) & (b[:, 1] != 0)
        assert a[:, 1].any() and b[:, 1].any(), "no XCD stamped"
        assert np.all(b[both, 1] >= a[both, 1]), "the second stamp is older than the first"
    return types.SimpleNamespace(live=[], stale=[], run=run, check=check, bits=False)


def _classifier_life(dev, device_tokenizer):
    """a fresh golden classifier per run: add_examples, predict, predict_batch, a new class, predict again"""
    from adaptive_classifier import AdaptiveClassifier, tokenizer as T
    from oracle import hub_standin
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    gdir = os.path.join(root, "tests", "golden", "e2e_bert_mini")
    texts = json.load(open(os.path.join(gdir, "expected.json")))["texts"]

    def run():
        torch.manual_seed(0)
        np.random.seed(0)
        hub_standin.install()
        try:
            with pytest.MonkeyPatch.context() as mp:
                if not device_tokenizer:
                    mp.setattr(T, "maybe_device_tokenizer", lambda tok, *a, **kw: tok)
                clf = AdaptiveClassifier.load(gdir, device=str(dev))
        finally:
            hub_standin.uninstall()
        assert isinstance(clf.tokenizer, T._DeviceTokenizer) == device_tokenizer
        labels = sorted(clf.label_to_id)
        clf.add_examples(texts[:6], [labels[i % len(labels)] for i in range(6)])
        out = [clf.predict(texts[6], k=3), clf.predict_batch(texts[:8], k=3)]
        clf.add_examples(texts[8:12], ["a brand new class"] * 4)
        out.append(clf.predict(texts[9], k=3))
        assert "a brand new class" in clf.label_to_id
        return [[[(l, float(s)) for l, s in r] for r in (o if isinstance(o[0], list) else [o])] for o in out]

    def check(got):
        assert poison.all_finite(got) and all(len(q) >= 1 for o in got for q in o)
    return types.SimpleNamespace(live=[], stale=[], run=run, check=check, bits=True)


@pytest.fixture(scope="module")
def world(cuda_dev):
    global _T0
    _T0 = time.time()
    from adaptive_classifier import _native as nv
    w = types.SimpleNamespace(dev=cuda_dev, side=torch.cuda.Stream(device=cuda_dev), plain={}, host_ms={})
    per_ms = sl.calibrate(cuda_dev)
    w.cases = dict(_gemm_cases(cuda_dev), synth_unit_rows=_synth_case(cuda_dev), clock_stamp=_clock_case(cuda_dev))
    w.cases["classifier_life_device_tokenizer"] = _classifier_life(cuda_dev, True)
    w.cases["classifier_life_host_tokenizer"] = _classifier_life(cuda_dev, False)
    torch.cuda.synchronize()
    with sl.EntrySpy(nv) as spy:
        w.spy = spy
        for name, c in w.cases.items():
            out, w.host_ms[name] = sl.plain(spy, c.run)
            w.plain[name] = sl.to_host(out)
        entries = {n: ms for n, ms in w.host_ms.items() if not n.startswith("classifier_life")}
        slowest = max(entries, key=entries.get)
        w.lag_ms = sl.choose_lag(entries[slowest])
        # a life waits on the host many times (training, predict's read-back): its span is not a non-waiting host time; the spy
        # lags the stream again after every such wait
        print(f"\nMEASURED test_stream_misc_gpu: {per_ms:.0f} sleep cycles per ms; slowest non-waiting case {slowest} {entries[slowest]:.2f} ms "
              f"of host time between its first and last native call; lag {w.lag_ms:.0f} ms; classifier lives "
              f"{w.host_ms['classifier_life_device_tokenizer']:.0f} / {w.host_ms['classifier_life_host_tokenizer']:.0f} ms")
        yield w
    print(f"\nMEASURED test_stream_misc_gpu wall time {time.time() - _T0:.1f} s")


CASE_NAMES = ["linear_f32", "gemm_f32", "split_and_linear_bf16x3", "split_and_linear_f16x2", "synth_unit_rows", "clock_stamp",
              "classifier_life_device_tokenizer", "classifier_life_host_tokenizer"]


@pytest.mark.parametrize("name", CASE_NAMES)
def test_side_stream_lags_and_inputs_arrive_late(name, world):
    w, c = world, world.cases[name]
    out, readings = sl.side_late(w.spy, w.side, w.lag_ms, c.run, c.live, c.stale)
    if not name.startswith("classifier_life"):                   # (a life's own host waits are the wrappers', all over it)
        sl.assert_enqueued(readings, HOST_WAITS, name)
    sl.note(__name__, readings, HOST_WAITS)
    got = sl.to_host(out)
    if c.bits:
        assert poison.same_bits(w.plain[name], got), "work ran ahead of the side stream: " + poison.first_difference(w.plain[name], got)
    c.check(got)


@pytest.mark.parametrize("name", CASE_NAMES)
def test_default_stream_lags_call_on_an_idle_side_stream(name, world):
    w, c = world, world.cases[name]
    got, readings = sl.default_lags(w.spy, w.side, w.lag_ms, c.run)
    if c.bits:
        assert poison.same_bits(w.plain[name], got), "work went to the default stream: " + poison.first_difference(w.plain[name], got)
    c.check(got)


# For the record (one run on an MI355X, inside the whole suite): 2412851 sleep cycles per ms; slowest non-waiting case clock_stamp, 0.02 ms
# of host time between its first and last native call; lag 20 ms (the floor); the classifier lives span 18 / 12 ms on the default stream;
# module wall time 2.2 s.
