"""GPU suite: AC_EXCHANGE_FENCES=1, the release / acquire form of the in-launch exchanges (csrc/gemm_pipe.hip: the LayerNorm panel
counters, the QKV-attention straddle exchange; the switch is a function-local static read once per process), against the
fence-free default.

The same list runs twice: in a fresh child process whose environment is the parent's plus AC_EXCHANGE_FENCES=1, and in this
process with the variable unset.  The list: every encoder_ref case whose table says ln_launches > 0 or attn_launches > 0, the MPNet
and DeBERTa cases that fuse, and one predict_tokens step of a small classifier.  Each encoder case is its suite's own test
function, so in BOTH processes the launch counters equal the case table, no exchange gave up, and the rows are within
R.device_bound(case) of fp64.  Then the rows (and the prediction's scores) of the two processes are compared bit for bit: the
fences change ordering, never arithmetic or summation order.

What this cannot show from outside the library: that the launches of the child really carried fences = 1.  The child asserts that
the variable is set, and gemm_pipe.hip's exchange_fences() reads exactly that name; were the switch renamed, two fence-free runs
would be compared and pass.  (A tests-only change: the library has no getter for the switch.)
"""
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

import encoder_deberta_ref as DB
import encoder_mpnet_ref as MP
import encoder_ref as R
import test_encoder_deberta_gpu as t_db
import test_encoder_mpnet_gpu as t_mp
import test_encoder_reference_gpu as t_ref
import test_poison_encoder_gpu as pe

pytestmark = pytest.mark.gpu


def _fuses(c):
    c = pe._case_of(c)
    return c.ln_launches > 0 or c.attn_launches > 0


LIST = [(f"bert:{c.id}", t_ref.test_encoder_matches_fp64_on_its_branch, c) for c in R.CASES if _fuses(c)]
LIST += [(f"mpnet:{c.id}", t_mp.test_mpnet_matches_fp64_on_its_route, c) for c in MP.MPNET_CASES if _fuses(c)]
LIST += [(f"deberta:{c.id}", t_db.test_deberta_matches_fp64_on_its_route, c) for c in DB.DEBERTA_CASES if _fuses(c)]


def _predict_step(dev):
    """one predict_tokens step of a small classifier (fused encoder forward -> kNN + head -> blend): scores as an array"""
    from adaptive_classifier import AdaptiveClassifier
    from adaptive_classifier.encoder import HipBertEncoder
    from oracle import bert_oracle
    model = bert_oracle.make_bert(256, 3, 4, 1024, vocab=2000, seed=3)
    clf = AdaptiveClassifier("synthetic", device=str(dev), encoder=HipBertEncoder(model, device=dev))
    rng = np.random.default_rng(0)
    emb = rng.standard_normal((400, 256)).astype(np.float32)
    emb /= np.linalg.norm(emb, axis=1, keepdims=True)
    clf.add_embeddings([f"t{i}" for i in range(400)], torch.from_numpy(emb), [f"c{i % 4}" for i in range(400)])
    ids, types, mask = bert_oracle.synthetic_batch(64, 32, vocab=2000, seed=5, ragged=True)
    res = clf.predict_tokens(ids, types, mask, k=3)
    labels = np.array([[int(l[1:]) for l, _ in p] for p in res], dtype=np.int64)
    return labels, np.array([[s for _, s in p] for p in res], dtype=np.float64)


def run_list(dev):
    """{name: rows / counters} of the whole list in THIS process (whatever its AC_EXCHANGE_FENCES says)"""
    from adaptive_classifier import _native as nv
    lib = nv.lib()
    out = {}
    with pytest.MonkeyPatch.context() as outer:
        hook = pe._Hook(outer)
        for name, fn, c in LIST:
            hook.rows = []
            n_ln, n_at = lib.ac_gemm_ln_fusion_launches(), lib.ac_gemm_qkv_attn_launches()
            with pytest.MonkeyPatch.context() as mp:
                fn(c, dev, mp)                  # asserts: counters of the table, no exchange gave up, R.device_bound(case) of fp64
            out[f"{name}/launches"] = np.array([lib.ac_gemm_ln_fusion_launches() - n_ln, lib.ac_gemm_qkv_attn_launches() - n_at])
            for i, r in enumerate(hook.rows):
                out[f"{name}/rows{i}"] = r.cpu().numpy()
    n_ln = lib.ac_gemm_ln_fusion_launches()
    out["predict/labels"], out["predict/scores"] = _predict_step(dev)
    out["predict/launches"] = np.array([lib.ac_gemm_ln_fusion_launches() - n_ln])
    return out


def _child(path):
    assert os.environ.get("AC_EXCHANGE_FENCES") == "1"
    np.savez(path, **run_list(torch.device("cuda:0")))
    torch.cuda.synchronize()
    print("FENCED_LIST_DONE")


def test_fenced_and_fence_free_exchanges_give_the_same_bits(cuda_dev, tmp_path, monkeypatch):
    monkeypatch.delenv("AC_EXCHANGE_FENCES", raising=False)
    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(here)
    path = str(tmp_path / "fenced.npz")
    script = ("import sys; sys.path[:0] = %r; import test_exchange_fences_gpu as t; t._child(%r)"
              % ([here, root, os.path.join(root, "adaptive-classifier_amd")], path))
    torch.cuda.synchronize()                    # the parent runs no GPU work of its own while the child does
    t0 = time.time()
    r = subprocess.run([sys.executable, "-c", script], env=dict(os.environ, AC_EXCHANGE_FENCES="1"), cwd=here, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]            # (nothing more is started after a child that failed)
    assert "FENCED_LIST_DONE" in r.stdout
    t1 = time.time()
    fenced = dict(np.load(path))
    free = run_list(cuda_dev)
    print(f"\nMEASURED test_exchange_fences_gpu: {len(LIST)} encoder cases + 1 predict step; child {t1 - t0:.1f} s, parent {time.time() - t1:.1f} s")
    assert sorted(fenced) == sorted(free)
    assert free["predict/launches"][0] > 0, "the predict step did not run a fused LayerNorm GEMM"
    differ = [k for k in sorted(free) if fenced[k].shape != free[k].shape or fenced[k].tobytes() != free[k].tobytes()]
    assert not differ, f"fenced and fence-free results differ in {differ[:8]} ({len(differ)} of {len(free)})"


# For the record (one run on an MI355X): 63 encoder cases + 1 predict step; the fenced child 9.8 s (process start and library load
# included), the fence-free parent 6.1 s; every array of the two bit-identical.
