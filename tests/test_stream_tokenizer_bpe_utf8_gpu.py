"""GPU suite: ac_bpe_utf8_encode on a non-default stream, text blob and offsets arriving late (tests/stream_lag.py) -- scenarios A
and B of tests/test_stream_tokenizer_gpu.py for the byte-level BPE entry on a non-ASCII batch of tests/bpe_unicode_helpers.py: a text
of zero length, one of one character, one that fills max_length exactly, one that is truncated, one the kernel hands back (a CJK run
of 90 bytes); a second batch of short texts.  ids, masks and (through the padded width) lens are bit-identical plainly on the default
stream, on a sleeping side stream with the text arriving late, and on an idle side stream while the default stream sleeps, and
equal the wrapped tokenizer's result in every position.

HOST_WAITS, read from csrc/bpe_utf8.hip: (none).  The wrapper reads `lens` on the host after the launch; the entry does not wait.

Why the readings go to stream_lag under the name of test_stream_tokenizer_gpu: tests/test_stream_zz_guard_gpu.py fails for any
exported stream-taking entry nobody saw returning under a sleeping stream -- ac_bpe_utf8_encode is one, and this module is where it
is seen -- and it also holds stream_lag.RAN against a fixed set of module names, which existing test files pin.  This module is
the tokenizer stream module's case for the new entry, so it reports as that module does.  Run the stream modules together."""
import time
import types

import pytest
import torch

import bpe_unicode_helpers as BU
import poison
import stream_lag as sl
import test_poison_tokenizer_gpu as pt
import test_stream_tokenizer_gpu as st

pytestmark = pytest.mark.gpu

HOST_WAITS = {}
ENTRY = "ac_bpe_utf8_encode"
M_LEN = pt.M_LEN
WORDS = ["café", "naïve", "résumé", "привет", "中文", "it’s", "“great”", "über", "€5", "мир", "don’t", "plain"]


def _build(dev):
    from adaptive_classifier.tokenizer import HipByteBPETokenizer
    hf = BU.build_tokenizer("roberta")
    tok = HipByteBPETokenizer(hf, device=dev, unicode=True)
    assert tok.unicode
    exact, longer = pt._texts_of_length(hf, WORDS)
    assert not exact.isascii()
    full = ["", "é", exact, longer, "中文产品很好" * 5]
    return hf, tok, [full, ["é", "中 文", "naïve… \U0001f600"]]


@pytest.fixture(scope="module")
def world(cuda_dev):
    t0 = time.time()
    from adaptive_classifier import _native as nv, tokenizer as T
    w = types.SimpleNamespace(dev=cuda_dev, side=torch.cuda.Stream(device=cuda_dev))
    per_ms = sl.calibrate(cuda_dev)
    with sl.EntrySpy(nv) as spy:
        w.spy = spy
        hf, tok, batches = _build(cuda_dev)
        packs = st._Packs(T, cuda_dev)
        want = [hf(batch, max_length=M_LEN, truncation=True, padding=True, return_tensors="pt") for batch in batches]

        def run():
            with pytest.MonkeyPatch.context() as m:
                m.setattr(T, "_pack_batch", packs)
                return [dict(tok(batch, max_length=M_LEN, truncation=True, padding=True, return_tensors="pt")) for batch in batches]
        w.case = types.SimpleNamespace(run=run, packs=packs, want=want, batches=batches)
        out, host_ms = sl.plain(spy, run)
        w.plain = sl.to_host(out)
        assert packs.bufs
        w.lag_ms = sl.choose_lag(host_ms)
        print(f"\nMEASURED test_stream_tokenizer_bpe_utf8_gpu: {per_ms:.0f} sleep cycles per ms; {host_ms:.2f} ms of host time between the "
              f"first and last native call; lag {w.lag_ms:.0f} ms")
        yield w
    print(f"\nMEASURED test_stream_tokenizer_bpe_utf8_gpu wall time {time.time() - t0:.1f} s")


def test_side_stream_lags_and_the_text_arrives_late(world):
    w, c = world, world.case
    live, stale = [b[0] for b in c.packs.bufs.values()], [b[1] for b in c.packs.bufs.values()]
    out, readings = sl.side_late(w.spy, w.side, w.lag_ms, c.run, live, stale)
    sl.assert_enqueued(readings, HOST_WAITS, ENTRY)
    assert ENTRY in {n for n, done in readings if not done}, readings
    sl.note("test_stream_tokenizer_gpu", readings, {})
    got = sl.to_host(out)
    assert poison.same_bits(w.plain, got), "work ran ahead of the side stream: " + poison.first_difference(w.plain, got)
    st._check(c, got)


def test_default_stream_lags_call_on_an_idle_side_stream(world):
    w, c = world, world.case
    got, readings = sl.default_lags(w.spy, w.side, w.lag_ms, c.run)
    assert ENTRY in {n for n, _ in readings}, readings
    assert poison.same_bits(w.plain, got), "work went to the default stream: " + poison.first_difference(w.plain, got)
    st._check(c, got)
