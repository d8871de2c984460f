"""GPU suite: no native entry point may read workspace bytes it did not write (round 5).

A fresh process gets zeroed pages from the driver, so `torch.empty` workspaces look clean; in a long-lived process the caching
allocator hands back blocks full of old data.  Found by the reference's own tests/test_classifier.py::test_prediction running
against the product in one process with other tests: the persistent training epoch (head_epoch.hip) with a batch of 5 < 32 rows
multiplied never-written rows of its activation scratch by zero weights -- NaN x 0 -- and the head came out all NaN.
Every workspace is filled with 0xFF bytes (fp32 / fp64 NaN, int -1) before the call; the result must equal the zero-filled run
bit for bit."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _fill(t, byte):
    t.view(torch.uint8).fill_(byte)


def _head_epoch_launches():
    import ctypes
    from adaptive_classifier import _native as nv
    he, bs = ctypes.c_int64(0), ctypes.c_int64(0)
    nv.check(nv.lib().ac_persistent_launches(ctypes.byref(he), ctypes.byref(bs)), "ac_persistent_launches")
    return he.value


def _table_device():
    """The expected paths below are written for 256 active CUs and 160 KB of LDS per workgroup."""
    import ctypes
    from adaptive_classifier import _native as nv
    chip, act = ctypes.c_int(0), ctypes.c_int(0)
    nv.check(nv.lib().ac_device_cus(ctypes.byref(chip), ctypes.byref(act)), "ac_device_cus")
    return act.value == 256 and nv.device_info()["lds_per_block"] >= 160 * 1024


def _train_on_garbage(cuda_dev, D, hidden, C, n, B, stepwise, persistent, bce=False):
    """Two epochs from a zero-filled and from a 0xFF-filled workspace: the same bits; and the path that was meant ran
    (`persistent`: written by hand from head_epoch_persistent()'s rule, as in tests/head_epoch_ref.py)."""
    from adaptive_classifier import AdaptiveHead, MultiLabelAdaptiveHead
    from adaptive_classifier.training import LOSS_BCE_SIGMOID, LOSS_CE, HeadTrainer
    g = torch.Generator().manual_seed(1)
    X = torch.nn.functional.normalize(torch.randn(n, D, generator=g), dim=1).to(cuda_dev)
    y = (torch.arange(n) % C).to(cuda_dev)
    T = ((torch.arange(n)[:, None] * 3 + torch.arange(C)[None, :] * 5) % 7 < 2).float().to(cuda_dev) if bce else None
    res = []
    for byte in (0, 0xFF):
        if bce:
            torch.manual_seed(7)
            head = MultiLabelAdaptiveHead(D, C, list(hidden)).to(cuda_dev)
        else:
            head = AdaptiveHead(D, C, list(hidden)).to(cuda_dev)
        tr = HeadTrainer(head)
        _fill(tr._workspace(min(B, n)), byte)
        _fill(tr.grads, byte)                            # the gradient block is scratch to the step (written before it is read)
        tr.loss_accum.zero_()
        before = _head_epoch_launches()
        for ep in range(2):
            tr.fused_epoch(X, None if bce else y, None, min(B, n), 0.1, 1234 + ep, stepwise=stepwise,
                           loss_kind=LOSS_BCE_SIGMOID if bce else LOSS_CE, targets_all=T)
        torch.cuda.synchronize()
        if _table_device():
            assert _head_epoch_launches() - before == (2 if persistent and not stepwise else 0)
        res.append(torch.cat([head.flat_params().detach().clone(), tr.loss_accum.clone()]))
    assert torch.isfinite(res[1]).all()
    assert torch.equal(res[0], res[1])


@pytest.mark.parametrize("D,C,n,B", [(768, 3, 5, 5), (768, 4, 64, 32), (768, 3, 40, 32), (128, 3, 5, 5), (128, 2, 1, 1),
                                     (1024, 64, 70, 32), (768, 3, 33, 32)])
@pytest.mark.parametrize("stepwise", [False, True])
def test_head_training_ignores_workspace_garbage(cuda_dev, D, C, n, B, stepwise):
    # every shape here fits the persistent epoch kernel but (1024 / [1024, 512], C = 64): C > 16, H2 > 384
    _train_on_garbage(cuda_dev, D, (D, D // 2), C, n, B, stepwise, persistent=C <= 16)


@pytest.mark.parametrize("D,hidden,C,n,B,bce", [
    (1024, (1024, 256), 16, 70, 32, False),         # r1 = 4: head_epoch_kernel<16, 4, 2>
    (1024, (1024, 256), 3, 5, 5, False),            #         head_epoch_kernel<4, 4, 2>, 5 rows
    (640, (520, 260), 7, 45, 32, False),            # ragged ownership, short last batch
    (640, (520, 260), 7, 18, 5, False),             # ... and an epoch of 5-row batches (5, 5, 5, 3)
    (768, (768, 384), 3, 20, 5, False),             # batch = 5 for a whole epoch
    (768, (768, 384), 3, 6, 1, False),              # batch = 1 for a whole epoch
    (64, (32, 16), 2, 40, 32, False),               # most workgroups own nothing
    (768, (768, 384), 6, 40, 32, True),             # BCE on sigmoid outputs, float targets
    (128, (128, 64), 16, 7, 7, True),
])
@pytest.mark.parametrize("stepwise", [False, True])
def test_head_training_ignores_workspace_garbage_more_shapes(cuda_dev, D, hidden, C, n, B, bce, stepwise):
    _train_on_garbage(cuda_dev, D, hidden, C, n, B, stepwise, persistent=True, bce=bce)


def test_head_forward_ignores_workspace_garbage(cuda_dev):
    from adaptive_classifier import AdaptiveHead
    X = torch.nn.functional.normalize(torch.randn(300, 768, generator=torch.Generator().manual_seed(2)), dim=1).to(cuda_dev)
    res = []
    for byte in (0, 0xFF):
        head = AdaptiveHead(768, 5, [768, 384]).to(cuda_dev)
        outs = []
        for nb in (1, 5, 33, 300):
            _fill(head._workspace(nb), byte)
            outs.append(head.forward_native(X[:nb]).reshape(-1))
        res.append(torch.cat(outs))
    assert torch.isfinite(res[1]).all() and torch.equal(res[0], res[1])


@pytest.mark.parametrize("H,L,A,I", [(128, 3, 2, 512), (768, 2, 12, 3072)])
def test_encoder_ignores_workspace_garbage(cuda_dev, H, L, A, I):
    from adaptive_classifier.encoder import HipBertEncoder
    from oracle import bert_oracle
    enc = HipBertEncoder(bert_oracle.make_bert(H, L, A, I, vocab=2000, seed=3), device=cuda_dev)
    for (b, S, ragged) in ((1, 5, False), (2, 16, False), (4, 12, True), (24, 16, False), (24, 16, True), (40, 32, True)):
        ids, types, mask = bert_oracle.synthetic_batch(b, S, vocab=2000, seed=9, ragged=ragged)
        res = []
        for byte in (0, 0xFF):
            enc._ws = None
            enc.encode_cls(ids, types, mask)                # sizes the workspace
            _fill(enc._ws, byte)
            enc._ws[:256].zero_()                            # (the verdict words: cleared by the caller, include/acamd.h)
            res.append(enc.encode_cls(ids, types, mask, verify=False).clone())
        assert torch.isfinite(res[1]).all() and torch.equal(res[0], res[1]), (b, S, ragged)


@pytest.mark.parametrize("N,nq,k", [(1000, 1, 5), (1000, 7, 16), (100_000, 16, 16), (100_000, 256, 16), (300_000, 40, 32)])
def test_knn_ignores_workspace_garbage(cuda_dev, N, nq, k):
    from adaptive_classifier import index as ix
    P = ix.synth_unit_rows(N, 768, 1, device=cuda_dev)
    Q = ix.synth_unit_rows(nq, 768, 2, device=cuda_dev)
    for prepared in (False, True):
        if prepared and not ix.batch_applies(N, nq, k):
            continue
        res = []
        for byte in (0, 0xFF):
            prep = ix.prepare_store(P, N, 768) if prepared else None
            need = max(ix.knn_workspace_bytes(N, 768, nq, k), ix.knn_batch_workspace_bytes(N, 768, nq, k) if prepared else 0)
            ws = torch.empty(need, dtype=torch.uint8, device=cuda_dev)
            _fill(ws, byte)
            stats = torch.zeros(4, dtype=torch.int32, device=cuda_dev)
            D_, I_ = ix.knn_l2_topk(P, N, 768, Q, k, workspace=ws, stats=stats, prepared=prep)
            res.append((D_.clone(), I_.clone()))
        assert torch.equal(res[0][1], res[1][1]) and torch.equal(res[0][0], res[1][0]), prepared


def test_classifier_in_a_process_with_a_dirty_allocator(cuda_dev):
    """The scenario of the reference's tests/test_classifier.py::test_prediction: five texts, three classes, then predict --
    with torch's caching allocator full of NaN-patterned free blocks."""
    from adaptive_classifier import AdaptiveClassifier
    from adaptive_classifier.encoder import HipBertEncoder
    from helpers import HashTokenizer, small_bert
    keep = []
    for sz in (256, 4096, 65536, 1 << 20, 1 << 22, 1 << 24, 1 << 26):
        for _ in range(6):
            keep.append(torch.full((sz // 4,), float("nan"), device=cuda_dev))
    torch.cuda.synchronize()
    del keep
    clf = AdaptiveClassifier("synthetic", device="cuda:0", encoder=HipBertEncoder(small_bert(hidden=768, heads=12, inter=1024),
                                                                                  device=cuda_dev), tokenizer=HashTokenizer())
    clf.add_examples(["This is amazing", "Terrible experience", "Just okay", "Love it", "Hate it"],
                     ["positive", "negative", "neutral", "positive", "negative"])
    assert np.isfinite(clf.last_train_info["final_loss"]) and torch.isfinite(clf.adaptive_head.flat_params()).all()
    preds = clf.predict("This is fantastic")
    assert len(preds) == 3 and all(s == s for _, s in preds) and abs(sum(s for _, s in preds) - 1.0) < 1e-6
