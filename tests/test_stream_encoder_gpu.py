"""GPU suite: the encoder entries on a non-default stream, with ids, types and mask arriving late (tests/stream_lag.py).

Cases: the first case of every branch of encoder_ref.BRANCHES, and the MPNet, DeBERTa, mean-pooling and fp16x2 cases of
tests/test_poison_encoder_gpu.py; the packed two-call form (AC_BERT_UNPAD_ONE_CALL=0: ac_bert_pack + ac_bert_encode_cls_packed)
and a direct call of the plain ac_bert_encode_cls, which the Python layer does not use.  Each case IS its suite's test function
(branch assertions -- one_launch, launch-counter deltas, path, tokens -- and the fp64 bound R.device_bound(case)), run three
times over device-resident ids / types / mask: plainly on the default stream; A. on a sleeping side stream, the three tensors
holding other valid values (ids shifted by one position, types flipped, an all-ones or one-shorter mask) until an in-stream copy_
brings the true ones; B. on an idle side stream while the default stream sleeps.  The rows every encode_cls returned, cloned in
stream order (a caller's `out` with its padding columns included), are bit-identical in all three.  A stream change does not
change the branch: the suite function's own assertions hold in every scenario.

HOST_WAITS, read from csrc/bert.hip, bert_small.hip, gemm*.hip (every hipStreamSynchronize / hipMemcpy / host spin):
  ac_bert_encode_cls_unpad    bert.hip:1354-1365  spins 200 000 pauses on the prologue's host slot, then hipStreamSynchronize
  ac_bert_ln_fusion_status    bert.hip:1262-1263  hipMemcpyAsync of the verdict words + hipStreamSynchronize
  ac_bert_one_launch_status   bert_small.hip:550-551 (bert_small_aborted, called at bert.hip:1252)  4-byte D2H + hipStreamSynchronize
  (bert_small.hip:528-529 and gemm debug stamps synchronise only under their debug switches; encoder.py's own reads --
   info.tolist() of the two-call form, torch.isfinite(out) under fp16x2 -- are the wrapper's: the spy lags the stream again)
For ac_bert_encode_cls_unpad scenario A also holds the wait the library measured (ac_bert_unpad_last_wait_ns) to at least
0.9 x lag minus the host time between enqueueing the sleep and the call, and requires that the call returned only after the
sleeping stream had drained.  With the lag at its 20 ms floor that is a wait of ~17 ms: the spin of 200 000 pauses would have to
cost more than 85 ns a pause to last that long (x86 pause: 10 .. 45 ns), so the blocking branch behind it ran.  That the
hipStreamSynchronize itself was reached cannot be read from outside the library; the wait getter is what there is.
"""
import ctypes
import time
import types

import pytest
import torch

import encoder_deberta_ref as DB
import encoder_mpnet_ref as MP
import encoder_pool_ref as PL
import encoder_ref as R
import poison
import stream_lag as sl
import test_encoder_deberta_gpu as t_db
import test_encoder_mpnet_gpu as t_mp
import test_encoder_pool_gpu as t_pl
import test_encoder_reference_gpu as t_ref
import test_poison_encoder_gpu as pe

pytestmark = pytest.mark.gpu

_T0 = time.time()
HOST_WAITS = {
    "ac_bert_encode_cls_unpad": "bert.hip:1354-1365 spin on the host slot, then hipStreamSynchronize",
    "ac_bert_ln_fusion_status": "bert.hip:1262-1263 hipMemcpyAsync + hipStreamSynchronize",
    "ac_bert_one_launch_status": "bert_small.hip:550-551 hipMemcpyAsync + hipStreamSynchronize (via bert.hip:1252)",
}
FAMILY = ("ac_bert_", "ac_modernbert_")
SEEN, CALLED = {}, set()


def _two_call_form(case, dev, mp):
    mp.setenv("AC_BERT_UNPAD_ONE_CALL", "0")
    import dataclasses
    t_ref.test_encoder_matches_fp64_on_its_branch(dataclasses.replace(case, path=None), dev, mp)     # (no unpad call to report a path)


class _Hook:
    """encode_cls of both encoder classes, wrapped: the suite function's host ids / types / mask are replaced by the LIVE device
    tensors of the same batch (no copy, no read: the call is made while their stream sleeps), the returned rows cloned in stream
    order"""

    def __init__(self, monkeypatch):
        from adaptive_classifier.encoder import HipBertEncoder, HipModernBertEncoder
        self.live, self.rows = None, []
        for cls in (HipBertEncoder, HipModernBertEncoder):
            monkeypatch.setattr(cls, "encode_cls", self._wrap(cls.encode_cls))

    def _wrap(self, real):
        hook = self

        def encode_cls(enc, input_ids, token_type_ids=None, attention_mask=None, out=None, **kw):
            ids, tt, mk = hook.live
            assert tuple(input_ids.shape) == tuple(ids.shape)
            got = real(enc, ids, None if token_type_ids is None else tt, None if attention_mask is None else mk, out=out, **kw)
            hook.rows.append(got.detach().clone())
            return got
        return encode_cls


_HOOK = [None]


def _plain_entry(case, dev, mp):
    """ac_bert_encode_cls itself (= _opts with no options), on the encoder object of the case"""
    from adaptive_classifier import _native as nv
    enc = t_ref._encoder(case, dev)
    ids, tt, mk = _HOOK[0].live
    b, S = ids.shape
    out = torch.empty((b, case.model.hidden), dtype=torch.float32, device=dev)
    need = enc.workspace_bytes(b, S)
    if enc._ws is None or enc._ws.numel() < need:
        enc._ws = torch.empty(need, dtype=torch.uint8, device=dev)
        enc._ws[:256].zero_()
    nv.check(nv.lib().ac_bert_encode_cls(ctypes.byref(enc.ccfg), ctypes.byref(enc.weights), nv.ptr(ids), nv.ptr(tt), nv.ptr(mk), b, S,
                                         nv.ptr(out), out.stride(0), nv.ptr(enc._ws), enc._ws.numel(), nv.stream_ptr(dev)), "ac_bert_encode_cls")
    _ROWS.append(out.clone())
    got = out.cpu()
    assert R.deviation(case, got) <= R.device_bound(case), case.id


_ROWS = []                      # rows of the direct call (the hook below records those of encode_cls)
_FIRST = {}
for _c in R.CASES:
    _FIRST.setdefault(_c.branch, _c)
assert sorted(_FIRST) == R.BRANCHES

CASES = [(f"branch_{b}:{c.id}", t_ref.test_encoder_matches_fp64_on_its_branch, c) for b, c in sorted(_FIRST.items())]
CASES += [(f"mpnet:{c.id}", t_mp.test_mpnet_matches_fp64_on_its_route, c) for c in MP.MPNET_CASES]
CASES += [(f"deberta:{c.id}", t_db.test_deberta_matches_fp64_on_its_route, c) for c in DB.DEBERTA_CASES]
CASES += [(f"mean:{c.id}", t_pl.test_mean_pooling_matches_fp64_on_its_branch, c) for c in PL.POOL_CASES]
CASES += [(f"f16x2:{cid}", pe._f16x2_run, R.BY_ID[cid]) for cid in ("ln_768_T384", "ol_768_ragged")]
CASES += [("two_call_form:T192_all_fused", _two_call_form, R.BY_ID["T192_all_fused"]),
          ("plain_entry:T192_all_fused", _plain_entry, R.BY_ID["T192_all_fused"]),
          ("plain_entry:ol_T32_ragged_len1", _plain_entry, R.BY_ID["ol_T32_ragged_len1"])]
BY_NAME = {n: (fn, c) for n, fn, c in CASES}


def _stale(ids, tt, mk):
    """other valid inputs of the same shapes: every id is one of the batch's own, types stay in {0, 1}, the mask stays a prefix"""
    s_ids = ids.roll(1, dims=1)
    s_tt = None if tt is None else 1 - tt
    s_mk = None
    if mk is not None:
        s_mk = torch.ones_like(mk)
        if bool((mk == 1).all()) and mk.shape[1] > 1:
            s_mk[:, -1] = 0
    return s_ids, s_tt, s_mk


@pytest.fixture(scope="module")
def world(cuda_dev):
    global _T0
    _T0 = time.time()
    from adaptive_classifier import _native as nv
    w = types.SimpleNamespace(dev=cuda_dev, side=torch.cuda.Stream(device=cuda_dev), lib=nv.lib(), batches={}, plain={}, host_ms={})
    per_ms = sl.calibrate(cuda_dev)
    def batch(c):
        bs = pe._case_of(c).batch
        if bs not in w.batches:
            true = tuple(None if t is None else t.to(cuda_dev) for t in R.make_batch(bs))
            w.batches[bs] = (true, _stale(*true))
        return w.batches[bs]

    def run(name):
        """the case's suite function over the LIVE device tensors; returns the rows its encode calls returned, cloned in stream order"""
        fn, c = BY_NAME[name]
        true, _ = batch(c)
        hook.rows, hook.live = [], true
        _ROWS.clear()
        with pytest.MonkeyPatch.context() as mp:
            fn(c, cuda_dev, mp)
        rows = list(hook.rows) + list(_ROWS)
        assert rows, name
        return rows

    w.batch, w.run = batch, run
    with pytest.MonkeyPatch.context() as outer, sl.EntrySpy(nv) as spy:
        hook = _HOOK[0] = _Hook(outer)
        w.spy = spy
        for name, _, c in CASES:
            out, w.host_ms[name] = sl.plain(spy, lambda: run(name))
            w.plain[name] = sl.to_host(out)
        slowest = max(w.host_ms, key=w.host_ms.get)
        w.lag_ms = sl.choose_lag(w.host_ms[slowest])
        print(f"\nMEASURED test_stream_encoder_gpu: {per_ms:.0f} sleep cycles per ms; slowest case {slowest} {w.host_ms[slowest]:.2f} ms of host "
              f"time between its first and last native call; lag {w.lag_ms:.0f} ms")
        yield w
    for m in (t_ref, t_mp, t_db, t_pl):
        m._ENCODERS.clear()
    print(f"\nMEASURED test_stream_encoder_gpu wall time {time.time() - _T0:.1f} s")


def _live(pair):
    true, stale = pair
    return [t for t in true if t is not None], [s for s in stale if s is not None]


@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_side_stream_lags_and_inputs_arrive_late(name, world):
    w = world
    live, stale = _live(w.batch(BY_NAME[name][1]))
    out, readings = sl.side_late(w.spy, w.side, w.lag_ms, lambda: w.run(name), live, stale)
    sl.assert_enqueued(readings, HOST_WAITS, name)
    CALLED.update(n for n, _ in readings)
    sl.note(__name__, readings, HOST_WAITS)
    for n, done in readings:
        if not done:
            SEEN[n] = True
    unpad = [done for n, done in readings if n == "ac_bert_encode_cls_unpad"]
    if unpad:
        wait_ms = w.lib.ac_bert_unpad_last_wait_ns() * 1e-6
        since_ms = [ms for n, ms in w.spy.since_arm if n == "ac_bert_encode_cls_unpad"][-1]
        assert all(unpad), "ac_bert_encode_cls_unpad returned before the sleeping stream could have run its prologue"
        # the sleep was enqueued since_ms of host time before the call on an idle stream, so the prologue's report cannot arrive
        # earlier than lag - since_ms after the call began; 10 % off for the calibration of the sleep
        need_ms = 0.9 * w.lag_ms - since_ms
        print(f"MEASURED {name}: unpad wait {wait_ms:.2f} ms, sleep enqueued {since_ms:.2f} ms before the call, lag {w.lag_ms:.0f} ms")
        assert wait_ms >= need_ms, f"the wait for the prologue's report took {wait_ms:.2f} ms, less than {need_ms:.2f} ms"
        SEEN["fallback:ac_bert_encode_cls_unpad"] = True
    got = sl.to_host(out)
    assert poison.same_bits(w.plain[name], got), "work ran ahead of the side stream: " + poison.first_difference(w.plain[name], got)


@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_default_stream_lags_call_on_an_idle_side_stream(name, world):
    w = world
    got, readings = sl.default_lags(w.spy, w.side, w.lag_ms, lambda: w.run(name))
    assert poison.same_bits(w.plain[name], got), "work went to the default stream: " + poison.first_difference(w.plain[name], got)


def test_every_encoder_entry_was_seen_returning_under_a_sleeping_stream(world):
    """The guard: every exported encoder symbol that takes a stream returned, in scenario A above, while its stream was still
    behind the sleep, or waits on the host at the line HOST_WAITS cites; and the fallback behind the unpad spin ran."""
    from adaptive_classifier import _native as nv
    mine = {n for n in nv.exported_symbols() if n.startswith(FAMILY)} & sl.stream_entries()
    assert mine
    missing = sorted(n for n in mine if not SEEN.get(n) and n not in HOST_WAITS)
    assert not missing, f"never seen returning under a lagging stream: {missing}"
    assert SEEN.get("fallback:ac_bert_encode_cls_unpad")
    assert set(HOST_WAITS) <= CALLED & mine, "a listed host wait was never called"


# For the record (one run on an MI355X, inside the whole suite): 2412851 sleep cycles per ms; slowest case mean:ln_768_T384, 0.85 ms of
# host time between its first and last native call; lag 20 ms (the floor); unpad waits 19.8 .. 19.95 ms under it; module wall time 8.4 s.
