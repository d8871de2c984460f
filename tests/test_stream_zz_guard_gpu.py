"""GPU suite, last of the stream modules (pytest runs the files of a directory in name order): every exported `ac_*` symbol whose
declaration takes a stream was either seen returning while its stream was still asleep, in a scenario-A test of one of the stream
modules, or is listed in a module's HOST_WAITS with the source line that waits.  No exclusion list: a new stream-taking export
fails here until a case reaches it.  The modules report to tests/stream_lag.py (note); run the stream modules together."""
import pytest

import stream_lag as sl

pytestmark = pytest.mark.gpu

MODULES = {"test_stream_encoder_gpu", "test_stream_head_gpu", "test_stream_knn_gpu", "test_stream_misc_gpu", "test_stream_tokenizer_gpu"}


def test_every_exported_stream_entry_is_seen_under_a_sleeping_stream_or_is_a_cited_host_wait(cuda_dev):
    from adaptive_classifier import _native as nv
    assert sl.RAN == MODULES, f"the guard reads what the stream modules recorded in this session; missing: {sorted(MODULES - sl.RAN)}"
    entries = set(nv.exported_symbols()) & sl.stream_entries()
    assert len(entries) >= 74                            # (what include/acamd.h declared when this was written)
    missing = sorted(n for n in entries if n not in sl.SEEN and n not in sl.HOST_WAITS)
    assert not missing, f"neither seen returning under a lagging stream nor a cited host wait: {missing}"
    uncited = sorted(n for n, where in sl.HOST_WAITS.items() if ".hip:" not in where)
    assert not uncited, f"HOST_WAITS entries without a file:line: {uncited}"
    never = sorted(set(sl.HOST_WAITS) - sl.CALLED)
    assert not never, f"listed as host waits but never called: {never}"
    # an entry that waits in one form only (ac_predict_post with h_out) must also have been seen NOT waiting in the other
    assert "ac_predict_post" in sl.SEEN
