"""Execution order for the suites that check: every native entry puts ALL of its work on the stream it was given.

In the other suites the caller's stream is the default stream, so a launch, a hipMemsetAsync, a counter clear or a read-back
that an entry put on stream 0 by mistake runs exactly where it should.  Here a native call is made while its stream is provably
still busy with earlier work (a device-side sleep), so that anything mis-placed on another stream runs at the wrong time,
deterministically.  PyTorch's side streams do not synchronise with the null stream.

calibrate(dev)          units of delay per millisecond (cycles of torch.cuda._sleep; matmuls of a fixed chain where it is missing),
                        timed once per process with two timing events.
lagging(stream, ms)     context manager: enqueues the sleep on `stream` (a side stream or the default one) and records a MARKER
                        event behind it; yields the marker.  marker.query() is False while the stream is still behind the sleep.
EntrySpy(nv)            wraps every `ac_*` attribute of the loaded library (the way knn_call_cases.Recorder does); right after each
                        native call of an entry that takes a stream returns it stores (entry name, marker.query()); False =
                        the call returned while the lagging stream was still asleep: the entry was enqueued, not waited for.  A wrapper's own host read (the range
                        searches read `lims`) drains the stream between two native calls: the spy then re-arms the lag before the
                        next call, so every native call is made under a busy stream.  Restored on exit.
Scenarios               both compare bit for bit with the same case run plainly on the default stream:
  A  side_late(...)     the side stream sleeps; the case's live inputs hold STALE BUT VALID values; on the side stream: sleep, copy_
                        of the true inputs, the case, clones of what it returned, synchronize.  Work that ran on stream 0 saw
                        the stale inputs.
  B  default_lags(...)  the default stream sleeps; the case runs on the idle side stream with its true inputs in place and is read
                        after side.synchronize(); only then the device.  A clear that went to stream 0 runs after the kernels it
                        was meant to precede.
At no time do two streams both hold library work: one sleeps, one works.

The modules' scenario-A tests report to this module (note): SEEN = entries seen returning under a sleeping stream, CALLED = entries
called at all, HOST_WAITS = every module's table of entries whose source shows a host wait, RAN = the modules that reported.
tests/test_stream_zz_guard_gpu.py holds all exported stream-taking entries against them.
"""
import contextlib
import os
import re
import time

import torch

LAG_MIN_MS, LAG_MAX_MS = 20.0, 200.0          # >= 20 ms: longer than any bounded host spin of the library; <= 200 ms per lag

_CAL, _CHAIN = {}, {}
SEEN, CALLED, HOST_WAITS, RAN = set(), set(), {}, set()


def note(module, readings, host_waits):
    """a scenario-A test's readings, for the guard over every exported entry"""
    RAN.add(module)
    HOST_WAITS.update(host_waits)
    CALLED.update(n for n, _ in readings)
    SEEN.update(n for n, done in readings if not done)


def _chain(n):
    """the fallback delay: n dependent matmuls of a fixed size"""
    dev = torch.cuda.current_device()
    if dev not in _CHAIN:
        _CHAIN[dev] = torch.eye(512, device=f"cuda:{dev}")
    a = b = _CHAIN[dev]
    for _ in range(int(n)):
        a = torch.matmul(a, b)
    return a


def _delay(units):
    if hasattr(torch.cuda, "_sleep"):
        torch.cuda._sleep(int(units))
    else:
        _chain(units)


def calibrate(dev):
    """delay units per millisecond on `dev` (timed once; the current stream must be idle)"""
    key = str(dev)
    if key in _CAL:
        return _CAL[key]
    units = 200_000 if hasattr(torch.cuda, "_sleep") else 8
    _delay(units)                                   # (first launch: module load)
    torch.cuda.synchronize()
    while True:
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        _delay(units)
        t1.record()
        t1.synchronize()
        ms = t0.elapsed_time(t1)
        if ms >= 2.0 or units >= 1 << 40:
            break
        units *= 8
    _CAL[key] = units / ms
    return _CAL[key]


@contextlib.contextmanager
def lagging(stream, ms):
    """enqueue `ms` of sleep on `stream`, then a marker event; yields the marker"""
    per_ms = calibrate(stream.device)
    with torch.cuda.stream(stream):
        _delay(per_ms * ms)
        marker = torch.cuda.Event()
        marker.record(stream)
    yield marker


def stream_entries():
    """the exported `ac_*` symbols whose declaration in include/acamd.h takes an ac_stream_t"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = re.sub(r"/\*.*?\*/|//[^\n]*", "", open(os.path.join(root, "include", "acamd.h")).read(), flags=re.S)
    return {name for name, args in re.findall(r"\b(ac_\w+)\s*\(([^;{}()]*)\)\s*;", text) if "ac_stream_t" in args}


class EntrySpy:
    """pass-through on every `ac_*` attribute of the loaded library.  While `arm(stream, ms)` is in force, each native call is
    made behind a sleep on that stream and its reading (entry, marker.query() right after it returned) goes to `readings`."""

    def __init__(self, nv):
        self.L = nv.lib()
        self._orig = {n: getattr(self.L, n) for n in nv.exported_symbols() if n.startswith("ac_") and hasattr(self.L, n)}
        self.readings, self.times, self.rearmed, self.since_arm = [], [], 0, []
        self._lag, self._marker, self._armed_at = None, None, 0.0
        self._streamed = stream_entries()                   # readings are taken of the entries that take a stream

    def __enter__(self):
        for name, fn in self._orig.items():
            setattr(self.L, name, self._wrap(name, fn))
        return self

    def __exit__(self, *exc):
        for name, fn in self._orig.items():
            setattr(self.L, name, fn)

    def _wrap(self, name, fn):
        def call(*args):
            lagged = self._lag is not None and name in self._streamed
            if lagged and self._marker.query():                     # a host wait of the wrapper drained the stream: lag again
                self._sleep()
                self.rearmed += 1
            t0 = time.perf_counter()
            rc = fn(*args)
            self.times.append((t0, time.perf_counter()))
            if lagged:
                self.readings.append((name, self._marker.query()))
                self.since_arm.append((name, (t0 - self._armed_at) * 1e3))     # host ms between enqueueing the sleep and this call
            return rc
        return call

    def _sleep(self):
        self._armed_at = time.perf_counter()
        with lagging(*self._lag) as m:
            self._marker = m

    def reset(self):
        self.readings, self.times, self.rearmed, self.since_arm = [], [], 0, []

    @contextlib.contextmanager
    def arm(self, stream, ms):
        self.reset()
        self._lag = (stream, ms)
        self._sleep()
        try:
            yield self
        finally:
            self._lag, self._marker = None, None

    def span_ms(self):
        """host time from the first native call to the return of the last one, since reset()"""
        return (self.times[-1][1] - self.times[0][0]) * 1e3 if self.times else 0.0


def choose_lag(host_ms):
    """10 x the slowest case's host time (host jitter on a shared machine is large), within [LAG_MIN_MS, LAG_MAX_MS]"""
    return min(max(10.0 * host_ms, LAG_MIN_MS), LAG_MAX_MS)


def clone_tree(x):
    """in-stream clones of every tensor of a nested result"""
    if isinstance(x, torch.Tensor):
        return x.clone()
    if isinstance(x, (list, tuple)):
        return type(x)(clone_tree(v) for v in x)
    if isinstance(x, dict):
        return {k: clone_tree(v) for k, v in x.items()}
    return x


def plain(spy, run):
    """the case on the default stream, twice (the first run pays for lazy initialisation): (result, host ms of the second)"""
    run()
    torch.cuda.synchronize()
    spy.reset()
    out = clone_tree(run())
    torch.cuda.synchronize()
    return out, spy.span_ms()


def side_late(spy, side, ms, run, live=(), stale=()):
    """Scenario A.  live: the case's input tensors; stale: valid other values of the same shapes.  Returns (result, readings)."""
    true = [t.clone() for t in live]
    for t, s in zip(live, stale):
        assert t.shape == s.shape and t.dtype == s.dtype
        t.copy_(s)
    torch.cuda.synchronize()                         # setup made on the default stream is complete
    try:
        with spy.arm(side, ms), torch.cuda.stream(side):
            for t, v in zip(live, true):
                t.copy_(v, non_blocking=True)
            out = clone_tree(run())
            side.synchronize()
            readings = list(spy.readings)
    finally:
        torch.cuda.synchronize()
        for t, v in zip(live, true):
            t.copy_(v)
        torch.cuda.synchronize()
    return out, readings


def default_lags(spy, side, ms, run):
    """Scenario B.  Returns (result, readings); the result is read after side.synchronize(), before the device is synchronised."""
    torch.cuda.synchronize()
    try:
        with spy.arm(torch.cuda.default_stream(side.device), ms), torch.cuda.stream(side):
            out = clone_tree(run())
            side.synchronize()
            out = to_host(out)
            readings = list(spy.readings)
    finally:
        torch.cuda.synchronize()
    return out, readings


def to_host(x):
    if isinstance(x, torch.Tensor):
        return x.detach().cpu().numpy().copy()
    if isinstance(x, (list, tuple)):
        return [to_host(v) for v in x]
    if isinstance(x, dict):
        return {k: to_host(v) for k, v in x.items()}
    return x


def assert_enqueued(readings, host_waits, what):
    """every native call returned while its stream was still asleep, unless its entry waits on the host (HOST_WAITS)"""
    assert readings, f"{what}: no native call was made"
    woke = sorted({n for n, done in readings if done and n not in host_waits})
    assert not woke, f"{what}: returned only after the lagging stream had drained, yet not listed as a host wait: {woke}"
