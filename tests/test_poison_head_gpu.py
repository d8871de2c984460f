"""GPU suite: the head-side entries over poisoned workspaces, scratch and outputs (tests/poison.py).

Regions, read from csrc/strategic.hip, head.hip, common.hip, memory_ops.hip and their Python callers before any poisoned run.
None is the caller's duty to clear.

  ac_strategic_best_response   workspace (ac_strategic_workspace: candidate rows, two activation blocks, logits, utilities):
                               written stage by stage for the b x M candidate rows before the next stage reads them; outputs
                               choice / util / Y / util_all / logits (torch.empty in strategic.py:87-98, 318-326): every element
  ac_head_fwd_bwd_strategic    HeadTrainer._ws (ac_head_workspace(2B)): activations, masks and deltas of the 2B rows, written by the
                               forward before the backward reads them; trainer.grads written whole, trainer.loss, mis [B]
  ac_head_fwd_bwd_loss         the same workspace for B rows (the Fisher pass, eval mode)
  ac_fisher_accumulate         reads grads, adds into fisher_flat (torch.zeros by ewc.py: state, not scratch)
  ac_ewc_loss                  8 KB scratch (torch.empty, ewc.py:107): block partials, each written by its block before the last
                               block (common.hip's device counter, cleared by its own launch) sums them
  ac_head_train_step           HeadTrainer._ws, grads (scratch to the step), out3
  ac_memory_add_prune          alive [n], dist [n], dropped [n_new] (torch.empty, memory.py:279-281): alive and dropped whole,
                               dist for every row that was live at the last prune -- zeros when no prune happened; all LDS state
                               is initialised by the kernel

Each case runs in four states -- zero, zero again, ff, leftover (a larger call of the same object or allocator first) -- with
(a) bit-identical results and (b) the family suite's own assertions: strategic_ref's BR_CASES and LOSS_CASES through
test_strategic_reference_gpu's test functions with their two C-ABI helpers replaced by the PRODUCT's callers
(strategic.best_response_batch; HeadTrainer workspace + the call of StrategicOptimizer.strategic_loss), memory_prune_ref's cases
through test_memory_prune_gpu's functions with torch.empty outputs, EWC against oracle/head_oracle.py.
"""
import ctypes
import time

import numpy as np
import pytest
import torch

import memory_prune_ref as M
import poison
import strategic_ref as R
import test_memory_prune_gpu as t_mem
import test_strategic_reference_gpu as t_sr

pytestmark = pytest.mark.gpu

_T0 = time.time()
STATES = (("zero", 0x00), ("zero2", 0x00), ("ff", 0xFF), ("leftover", None))


@pytest.fixture(scope="module", autouse=True)
def _wall():
    yield
    _HEADS.clear()
    _ROWS.clear()
    print(f"\nMEASURED test_poison_head_gpu wall time {time.time() - _T0:.1f} s")


class _State:
    byte, leftover, results = None, False, None


def _same_in_all_states(res):
    assert poison.same_bits(res["zero"], res["zero2"]), "two zero-state runs differ: " + poison.first_difference(res["zero"], res["zero2"])
    for state in ("ff", "leftover"):
        assert poison.same_bits(res["zero"], res[state]), f"the {state} state changed the result: " + poison.first_difference(res["zero"], res[state])


def _four_states(monkeypatch, run):
    p = poison.poisoned_empty(monkeypatch, None)
    st, res = _State(), {}
    for state, byte in STATES:
        p.byte = st.byte = byte
        st.leftover = state == "leftover"
        st.results = []
        run(st)
        res[state] = st.results
        assert st.results
    p.byte = None
    assert p.filled > 0
    _same_in_all_states(res)
    return res["ff"]


# ---- strategic best response --------------------------------------------------------------------------------------------------
_HEADS = {}


def _head_of(flat, dims, dev):
    key = (flat.data_ptr(), dims)
    if key not in _HEADS:
        _HEADS[key] = (flat, t_sr._device_head(flat, dims, dev))       # (the flat block is kept: its address is the key)
    return _HEADS[key][1]


def _product_best_response(st, monkeypatch):
    """test_strategic_reference_gpu._best_response's contract, served by strategic.best_response_batch"""
    from adaptive_classifier import strategic as S

    def call(dims, flat, X, feat, delta, coef, cost_type, mode, masks=None, seed=0, ws_short=0, dev=None):
        assert masks is None and not ws_short
        D, H1, H2, C = dims
        head = None if flat is None else _head_of(flat, dims, dev)
        table = (torch.tensor(list(feat), dtype=torch.int32, device=dev), torch.as_tensor(delta, dtype=torch.float32).to(dev))
        monkeypatch.setattr(S, "_device_table", lambda dim, device: table)
        Xd = X.to(dev)

        def once(rows):
            return S.best_response_batch(rows, head, num_classes=C, coef=coef, cost_type=cost_type, mask_mode=mode, seed=seed,
                                         dropout_p=t_sr.P, want_logits=True, want_all=True)
        if st.leftover:
            once(torch.cat([Xd, Xd]))
        r = once(Xd)
        torch.cuda.synchronize()
        out = {k: (None if v is None else v.cpu()) for k, v in r.items()}
        st.results.append(dict(out))
        if out["logits"] is None:                                       # (no head: the entry gets a NULL pointer, nothing is written)
            out["logits"] = torch.full((X.shape[0], C), t_sr.SENTINEL)
        out.update(rc_ws=0, rc=0)
        return out
    return call


@pytest.mark.parametrize("case", R.BR_CASES, ids=lambda c: c.id)
def test_best_response_through_the_product_wrapper(case, cuda_dev, monkeypatch):
    def run(st):
        monkeypatch.setattr(t_sr, "_best_response", _product_best_response(st, monkeypatch))
        t_sr.test_b_best_response_matches_fp64(cuda_dev, case)
    got = _four_states(monkeypatch, run)
    assert len(got) == 4 and poison.all_finite([{k: v for k, v in r.items() if v is not None} for r in got])


# ---- strategic loss -----------------------------------------------------------------------------------------------------------
def _product_loss_call(st):
    """test_strategic_reference_gpu._loss_call's contract through a HeadTrainer: its kept workspace, gradient block and loss word,
    the misprediction flags from torch.empty -- the call StrategicOptimizer.strategic_loss makes"""
    from adaptive_classifier import _native as nv
    from adaptive_classifier.training import HeadTrainer

    def call(dims, flat, X2, y, lam, masks2=None, use_seed=0, seed=0, dev=None):
        tr = HeadTrainer(_head_of(flat, dims, dev))
        assert torch.equal(tr.flat.cpu(), flat)

        def once(X2, y, masks2):
            B = X2.shape[0] // 2
            Xd, yd = X2.to(dev).contiguous(), y.to(dev).contiguous()
            m1 = m2 = None
            if masks2 is not None:
                m1, m2 = t_sr._u8(masks2[0], dev), t_sr._u8(masks2[1], dev)
            mis = torch.empty(B, dtype=torch.int32, device=dev)
            ws = tr._workspace(2 * B)
            with torch.cuda.device(dev):
                nv.check(nv.lib().ac_head_fwd_bwd_strategic(
                    ctypes.byref(tr.dims), nv.ptr(tr.flat), nv.ptr(Xd), Xd.stride(0), nv.ptr(yd), nv.ptr(m1), nv.ptr(m2), t_sr.P, use_seed,
                    seed & R.MASK64, B, lam, nv.ptr(tr.loss), nv.ptr(tr.grads), nv.ptr(mis), nv.ptr(ws), ws.numel(), nv.stream_ptr(dev)),
                    "ac_head_fwd_bwd_strategic")
            torch.cuda.synchronize()
            return tr.loss.cpu().clone(), tr.grads.cpu().clone(), mis.cpu()
        B = X2.shape[0] // 2
        if st.leftover:                                                 # the same head over the rows twice: a workspace twice as large
            two = lambda t: None if t is None else np.concatenate([t[:B], t[:B], t[B:], t[B:]])      # noqa: E731
            once(torch.cat([X2[:B], X2[:B], X2[B:], X2[B:]]), torch.cat([y, y]),
                 None if masks2 is None else (two(np.asarray(masks2[0])), two(np.asarray(masks2[1]))))
        else:
            for t in (tr.grads, tr.loss):
                poison.fill(t, st.byte)
        out = once(X2, y, masks2)
        st.results.append(out)
        return out
    return call


@pytest.mark.parametrize("case", R.LOSS_CASES, ids=lambda c: c.id)
def test_strategic_loss_through_the_trainer_workspace(case, cuda_dev, monkeypatch):
    def run(st):
        monkeypatch.setattr(t_sr, "_loss_call", _product_loss_call(st))
        t_sr.test_c_strategic_loss_matches_fp64_autograd(cuda_dev, case)
    got = _four_states(monkeypatch, run)
    assert poison.all_finite(got)


# ---- EWC: Fisher pass, penalty, fused step -----------------------------------------------------------------------------------
TOL = 1e-4                                                              # tests/test_head_gpu.py's bar (BASELINE north_star)


@pytest.mark.parametrize("D,hidden,C", [(768, (768, 384), 4), (640, (520, 260), 7)], ids=["768x768x384_C4", "ragged_640x520x260_C7"])
def test_ewc_fisher_penalty_and_fused_step(D, hidden, C, cuda_dev, monkeypatch):
    """The scenario of test_head_gpu.py::test_ewc_fisher_penalty_and_fused_step (Fisher from given labels over batches of 32, 32
    and 6; params += 0.1; ewc_loss() and ewc_loss(batch_size=32); one fused step with the penalty) and the ragged head of
    tests/head_epoch_ref.py, against oracle/head_oracle.py."""
    from adaptive_classifier.ewc import EWC
    from adaptive_classifier.models import AdaptiveHead
    from adaptive_classifier.training import HeadTrainer
    from oracle import head_oracle
    from test_head_gpu import _data
    B, lam = 32, 5.0
    Xs, _ = _data(70, D, C, seed=3)
    batches = [Xs[:32], Xs[32:64], Xs[64:]]
    g = torch.Generator().manual_seed(11)
    sampled = [torch.randint(0, C, (b.shape[0],), generator=g) for b in batches]
    X, y = _data(B, D, C, seed=5)
    Xbig, ybig = _data(2 * B, D, C, seed=6)
    ref0 = head_oracle.make_head(D, C, list(hidden))
    f_ref = head_oracle.fisher_from_labels(ref0, batches, sampled)
    want = {}

    def run(st):
        ref = head_oracle.make_head(D, C, list(hidden)).train()
        opt = torch.optim.AdamW(ref.parameters(), lr=0.001, weight_decay=0.01, betas=(0.9, 0.999))
        head = AdaptiveHead(D, C, list(hidden)).to(cuda_dev)
        with torch.no_grad():
            head.flat_params().copy_(head_oracle.flat(ref).to(cuda_dev))
        tr = HeadTrainer(head)
        if st.leftover:
            tr.forward_backward_loss(Xbig.to(cuda_dev), y=ybig.to(cuda_dev), dropout_p=0.0)     # a workspace of 64 rows, used
        else:
            for t in (tr.grads, tr.loss, tr.out3):
                poison.fill(t, st.byte)
        ewc = EWC.__new__(EWC)
        ewc.model, ewc.device, ewc.ewc_lambda, ewc._native = head, str(cuda_dev), lam, True
        ewc.old_flat = head.flat_params().detach().clone()
        ewc.old_params = {n: p.data.clone() for n, p in head.named_parameters()}
        head.eval()
        ewc.fisher_info = ewc._compute_fisher_native([(b, None) for b in batches], sampled_labels=[s.to(cuda_dev) for s in sampled])
        fisher = ewc.fisher_flat.cpu().clone()
        rel = (fisher - f_ref).abs().max().item() / f_ref.abs().max().item()
        assert rel < 1e-4, rel
        old_ref = head_oracle.flat(ref).clone()
        with torch.no_grad():
            for p in ref.parameters():
                p += 0.1
            for p in head.parameters():
                p += 0.1
            got, got32 = ewc.ewc_loss().cpu().clone(), ewc.ewc_loss(batch_size=32).cpu().clone()
        if not want:
            want["pen"] = float(head_oracle.ewc_penalty(ref, f_ref, old_ref, lam))
            want["pen32"] = float(head_oracle.ewc_penalty(ref, f_ref, old_ref, lam / 32))
        assert got.item() > 0 and got32.item() > 0 and got.item() != got32.item()
        assert abs(got.item() - want["pen"]) < TOL * max(1.0, abs(want["pen"]))
        assert abs(got32.item() - want["pen32"]) < TOL * max(1.0, abs(want["pen32"]))
        head.train()
        ce, pen, gn = head_oracle.train_step(ref, opt, X, y, masks=None, fisher_flat=f_ref, old_flat=old_ref, lam_over_B=lam / B)
        out3 = tr.fused_step(X.to(cuda_dev), y.to(cuda_dev), None, 0.0, 0, fisher=ewc.fisher_flat, old_params=ewc.old_flat,
                             lambda_over_B=lam / B).cpu().clone()
        flat = tr.flat.cpu().clone()
        assert abs(out3[0].item() - ce) < TOL
        assert abs(out3[1].item() - pen) < TOL * max(1.0, abs(pen))
        assert abs(out3[2].item() - gn) < TOL * max(1.0, gn)
        assert (flat - head_oracle.flat(ref)).abs().max().item() < 5e-5
        st.results.append([fisher, got, got32, out3, flat])
    got = _four_states(monkeypatch, run)
    assert poison.all_finite(got)


# ---- prototype memory: add + prune ------------------------------------------------------------------------------------------
_SUITE_JOB = t_mem._Job


def _empty_jobs(st, dev):
    """test_memory_prune_gpu._Job with its three outputs taken from torch.empty like memory.py:279-281 (one element longer, that
    element set to the suite's sentinel so that its 'nothing past the end' check stays in force)"""
    class Job(_SUITE_JOB):
        def __init__(self, c, rows, dev_):
            super().__init__(c, rows, dev_)
            for name, fill in (("d_alive", t_mem.ALIVE_FILL), ("d_dist", t_mem.DIST_FILL), ("d_drop", t_mem.DROP_FILL)):
                old = getattr(self, name)
                new = torch.empty(old.shape, dtype=old.dtype, device=old.device)
                new[-1] = fill
                setattr(self, name, new)

        def check(self):
            out = super().check()
            dropped, alive, dist, total = self.outputs()
            keep = alive.astype(bool)
            st.results.append([dropped.copy(), alive.copy(), dist[keep].copy(), total.copy()])       # (dist of a dropped row: undefined)
            return out
    return Job


_ROWS = {}


def _rows_once(c):
    """memory_prune_ref.make_rows, computed once per case for the four states (the rows are only read)"""
    if c not in _ROWS:
        _ROWS.clear()
        _ROWS[c] = _MAKE_ROWS(c)
    return _ROWS[c]


_MAKE_ROWS = M.make_rows


def _memory_states(monkeypatch, cuda_dev, fn, *args):
    big = M.MULTI_JOB_CASES[1]
    if fn is not t_mem.test_five_jobs_of_different_sizes_in_one_launch:
        monkeypatch.setattr(M, "make_rows", _rows_once)

    def run(st):
        monkeypatch.setattr(t_mem, "_Job", _empty_jobs(st, cuda_dev))
        if st.leftover:
            job = t_mem._Job(big, M.make_rows(big), cuda_dev)
            assert t_mem._launch(cuda_dev, [job], big.D) == 0
            del job
            st.results = []
        fn(*args, cuda_dev)
    return _four_states(monkeypatch, run)


@pytest.mark.parametrize("case", M.CASES, ids=[c.name for c in M.CASES])
def test_memory_prune_one_job(case, cuda_dev, monkeypatch):
    _memory_states(monkeypatch, cuda_dev, t_mem.test_one_job_against_the_reference, case)


def test_memory_prune_five_jobs_in_one_launch(cuda_dev, monkeypatch):
    got = _memory_states(monkeypatch, cuda_dev, t_mem.test_five_jobs_of_different_sizes_in_one_launch)
    assert len(got) == 5


@pytest.mark.parametrize("case", M.DUP_CASES, ids=[c.name for c in M.DUP_CASES])
def test_memory_prune_duplicates(case, cuda_dev, monkeypatch):
    _memory_states(monkeypatch, cuda_dev, t_mem.test_exact_duplicate_rows_follow_the_tie_rule, case)


@pytest.mark.parametrize("byte", [0x00, 0xFF])
def test_train_mode_robustness_evaluation(byte, cuda_dev, monkeypatch):
    """StrategicEvaluator's train-mode forwards (strategic.py::_head_logits: logits, choice, util, Y and the workspace from
    torch.empty) inside the suite's robustness scenario, against its fp64 dictionary."""
    p = poison.poisoned_empty(monkeypatch, byte)
    t_sr.test_e_train_mode_robustness_equals_the_fp64_dictionary(cuda_dev)
    assert p.filled > 0


@pytest.mark.parametrize("byte", [0x00, 0xFF])
def test_prototype_memory_batched_prune_under_poisoned_allocations(byte, cuda_dev, monkeypatch):
    """The product's own caller (PrototypeMemory.add_examples_batch -> _run_prune_jobs, class matrices from torch.empty) must leave
    the state of the per-example host logic: tests/test_classifier_gpu.py's scenario, with every device allocation byte-filled."""
    from test_classifier_gpu import test_batched_device_prune_equals_per_example_host_logic as scenario
    p = poison.poisoned_empty(monkeypatch, byte)
    scenario(10, 64, 90, cuda_dev)
    scenario(50, 128, 400, cuda_dev)
    assert p.filled > 0
