"""GPU suite: the device tokenizer entries on a non-default stream, text blob and offsets arriving late (tests/stream_lag.py).

Entries and batches of tests/test_poison_tokenizer_gpu.py -- WordPiece ASCII and UTF-8, byte-level BPE, Unigram ASCII -- plus the
Unigram UTF-8 entry on a non-ASCII batch of tests/unigram_unicode_helpers.py: a text of zero length, one of one byte, one that
fills max_length exactly, one that is truncated, one the kernel hands back; a second batch of short texts.  The wrapper packs
offsets and text into ONE device buffer (tokenizer.py::_pack_batch); here that buffer is a persistent LIVE tensor per batch.
Plainly on the default stream; A. on a sleeping side stream, the buffer holding the SAME texts in reverse order (valid offsets,
valid UTF-8, the same byte count) until an in-stream copy_ brings the true packing; B. on an idle side stream while the default
stream sleeps.  ids, masks and (through the padded width) lens are bit-identical in all three and equal the wrapped tokenizer's
result in every position (the `*_encode_host` reference of the tokenizer suites is proven equal to it there).

HOST_WAITS, read from csrc/wordpiece.hip, bpe.hip, unigram.hip, unigram_utf8.hip: (none).  The wrapper reads `lens` on the host
after the launch (tokenizer.py: torch.aminmax(lens).tolist()); the entries do not wait.
"""
import time
import types

import numpy as np
import pytest
import torch

import poison
import stream_lag as sl
import test_poison_tokenizer_gpu as pt
import unigram_unicode_helpers as UU
import wordpiece_helpers as WH

pytestmark = pytest.mark.gpu

_T0 = time.time()
HOST_WAITS = {}
FAMILY = ("ac_wordpiece_encode", "ac_bpe_encode", "ac_unigram_encode")
ENTRY_OF = {"wordpiece_ascii": "ac_wordpiece_encode", "wordpiece_utf8": "ac_wordpiece_encode_utf8", "bpe": "ac_bpe_encode",
            "unigram": "ac_unigram_encode", "unigram_utf8": "ac_unigram_encode_utf8"}
SEEN = {}
M_LEN = pt.M_LEN


def _build(entry, dev):
    """(wrapped tokenizer, device tokenizer, batches)"""
    if entry == "unigram_utf8":
        from adaptive_classifier.tokenizer import HipUnigramTokenizer
        hf = UU.build_tokenizer("full", "xlmr")
        tok = HipUnigramTokenizer(hf, device=dev, unicode=True)
        assert tok.unicode
        full = ["", "é", "café naïve 中文 ß", "文" * 70 + "éa", "éa" * 40 + "文ß" * 30 + "a中"]
        return hf, tok, [full, ["é", "中 文", "naïve"]]
    hf, tok, handed_back = pt._build(entry, dev)
    words = [w for w in pt.WORDS if w.isalpha()]
    if entry == "wordpiece_utf8":
        words = ["café", "naïve", "é", "中", "文", "e", "한"] + [w for w in WH.vocab() if w.isalpha() and not w.isascii()][:40]
    exact, longer = pt._texts_of_length(hf, words)
    full = ["", words[0][:1], exact, longer] + ([handed_back] if handed_back else [])
    return hf, tok, [full, ["", words[0][:1], " ".join(words[:2])]]


class _Packs:
    """tokenizer._pack_batch, with one persistent device buffer per (blob, sizes): `live` the true packing, `stale` the packing
    of the same texts in reverse order"""

    def __init__(self, T, dev):
        self.T, self.real, self.dev, self.bufs = T, T._pack_batch, dev, {}

    def __call__(self, blob, sizes, dev):
        key = (bytes(blob), tuple(int(s) for s in sizes))
        b = len(sizes)
        head = (4 * (b + 1) + 15) // 16 * 16
        if key not in self.bufs:
            gap = torch.zeros(head - 4 * (b + 1), dtype=torch.uint8, device=dev)
            o, t = self.real(blob, sizes, dev)
            live = torch.cat((o, gap, t))
            ends = np.cumsum([0] + list(key[1]))
            texts = [key[0][ends[i]:ends[i + 1]] for i in range(b)]
            so, st = self.real(b"".join(reversed(texts)), list(reversed(key[1])), dev)
            stale = torch.cat((so, gap, st))
            assert stale.shape == live.shape
            self.bufs[key] = (live, stale)
        live = self.bufs[key][0]
        return live[:4 * (b + 1)], live[head:]


@pytest.fixture(scope="module")
def world(cuda_dev):
    global _T0
    _T0 = time.time()
    from adaptive_classifier import _native as nv, tokenizer as T
    w = types.SimpleNamespace(dev=cuda_dev, side=torch.cuda.Stream(device=cuda_dev), cases={}, plain={}, host_ms={})
    per_ms = sl.calibrate(cuda_dev)
    with pytest.MonkeyPatch.context() as mp, sl.EntrySpy(nv) as spy:
        w.spy = spy
        for entry in ENTRY_OF:
            hf, tok, batches = _build(entry, cuda_dev)
            packs = _Packs(T, cuda_dev)
            want = [hf(batch, max_length=M_LEN, truncation=True, padding=True, return_tensors="pt") for batch in batches]

            def run(tok=tok, batches=batches, packs=packs):
                with pytest.MonkeyPatch.context() as m:
                    m.setattr(T, "_pack_batch", packs)
                    return [dict(tok(batch, max_length=M_LEN, truncation=True, padding=True, return_tensors="pt")) for batch in batches]
            c = w.cases[entry] = types.SimpleNamespace(run=run, packs=packs, want=want, batches=batches)
            out, w.host_ms[entry] = sl.plain(spy, run)
            w.plain[entry] = sl.to_host(out)
            assert packs.bufs, entry
        slowest = max(w.host_ms, key=w.host_ms.get)
        w.lag_ms = sl.choose_lag(w.host_ms[slowest])
        print(f"\nMEASURED test_stream_tokenizer_gpu: {per_ms:.0f} sleep cycles per ms; slowest case {slowest} {w.host_ms[slowest]:.2f} ms of "
              f"host time between its first and last native call; lag {w.lag_ms:.0f} ms")
        yield w
    print(f"\nMEASURED test_stream_tokenizer_gpu wall time {time.time() - _T0:.1f} s")


def _check(c, got):
    for g, want, batch in zip(got, c.want, c.batches):
        assert set(g) == set(want.keys())
        for key in want.keys():
            assert g[key].shape == tuple(want[key].shape) and np.array_equal(g[key], want[key].numpy()), (key, batch)


@pytest.mark.parametrize("entry", list(ENTRY_OF))
def test_side_stream_lags_and_the_text_arrives_late(entry, world):
    w, c = world, world.cases[entry]
    live, stale = [b[0] for b in c.packs.bufs.values()], [b[1] for b in c.packs.bufs.values()]
    out, readings = sl.side_late(w.spy, w.side, w.lag_ms, c.run, live, stale)
    sl.assert_enqueued(readings, HOST_WAITS, entry)
    assert ENTRY_OF[entry] in {n for n, _ in readings}, (entry, readings)
    sl.note(__name__, readings, HOST_WAITS)
    for n, done in readings:
        if not done:
            SEEN[n] = True
    got = sl.to_host(out)
    assert poison.same_bits(w.plain[entry], got), "work ran ahead of the side stream: " + poison.first_difference(w.plain[entry], got)
    _check(c, got)


@pytest.mark.parametrize("entry", list(ENTRY_OF))
def test_default_stream_lags_call_on_an_idle_side_stream(entry, world):
    w, c = world, world.cases[entry]
    got, readings = sl.default_lags(w.spy, w.side, w.lag_ms, c.run)
    assert poison.same_bits(w.plain[entry], got), "work went to the default stream: " + poison.first_difference(w.plain[entry], got)
    _check(c, got)


def test_every_tokenizer_entry_was_seen_returning_under_a_sleeping_stream(world):
    from adaptive_classifier import _native as nv
    mine = {n for n in nv.exported_symbols() if n.startswith(FAMILY)} & sl.stream_entries()
    assert mine == set(ENTRY_OF.values()), mine
    missing = sorted(n for n in mine if not SEEN.get(n))
    assert not missing, f"never seen returning under a lagging stream: {missing}"


# For the record (one run on an MI355X, inside the whole suite): 2412851 sleep cycles per ms; slowest case wordpiece_utf8, 0.90 ms of host
# time between its first and last native call; lag 20 ms (the floor); module wall time 4.9 s.
