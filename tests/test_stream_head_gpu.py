"""GPU suite: the head-side entries and the prediction tail on a non-default stream, inputs arriving late (tests/stream_lag.py).

  head forward        ac_head_forward (AdaptiveHead.logits) + the small row kernels ac_softmax_rows / ac_sigmoid /
                      ac_l2_normalize_rows, against fp64 torch (1e-4, tests/test_head_gpu.py's bar; 1e-6 for the row kernels)
  training            cases of tests/head_epoch_ref.py through test_head_epoch_reference_gpu._run_leg: fused_epoch (the persistent,
                      cooperative launch) and the fused_step loop, CE with and without EWC, ragged ownership, a head that only has
                      the launch-by-launch path (C = 17), BCE with padded targets; each against the fp64 trajectory at
                      head_epoch_ref.bounds_of(case), launch-counter deltas as the table says
  explicit masks      HeadTrainer.step (ac_head_fwd_bwd_ce + ac_ewc_adamw_step) and forward_backward_loss (ac_head_fwd_bwd_loss, BCE)
                      against oracle/head_oracle.py at 1e-4 / 5e-5 (tests/test_head_gpu.py's bars)
  EWC                 Fisher pass (ac_head_fwd_bwd_loss + ac_fisher_accumulate), ac_ewc_loss, one fused step with the penalty:
                      the scenario of test_poison_head_gpu.py against head_oracle
  prune               ac_memory_add_prune with one job and with five jobs in one launch (test_memory_prune_gpu's jobs, replayed against
                      memory_prune_ref); the candidate rows are late inputs
  strategic           ac_strategic_best_response and ac_head_fwd_bwd_strategic: the first and last case of strategic_ref's BR_CASES and
                      LOSS_CASES through test_strategic_reference_gpu's own functions (fp64 comparison included), X and labels late
  prediction tail     the edge table of test_predict_tail_gpu.py (POST_SHAPES) through the classifier's tail in its three modes:
                      ac_predict_post with h_out (host-waited), without (device stage + D2H), and the separate kernels
                      ac_proto_scores / ac_rows_to_class / ac_softmax_rows / ac_blend_topk; lists equal predict_tail_ref.blend_topk

Each case runs plainly on the default stream, then A. on a sleeping side stream with its device inputs (X, labels / targets,
order, prune candidates, distances / ids / logits) holding other valid values until an in-stream copy_ brings the true ones,
then B. on an idle side stream while the default stream sleeps; the results are bit-identical in all three.

HOST_WAITS, read from csrc/head.hip, head_epoch.hip, strategic.hip, blend.hip, memory_ops.hip, common.hip, gemm.hip:
  ac_predict_post   blend.hip:321-334  with h_out: spins (up to 40 000 000 pauses) on its host flag, then hipStreamSynchronize.
                    The spin outlasts any lag this suite may use (<= 200 ms), so the flag is seen by the spin: the blocking
                    branch behind it is NOT reached here.
  (head_epoch.hip:820-821 synchronises only under AC_HEAD_EPOCH_DEBUG; nothing else on the head side waits)
"""
import ctypes
import time
import types

import numpy as np
import pytest
import torch

import head_epoch_ref as HR
import memory_prune_ref as M
import poison
import predict_tail_ref as PR
import stream_lag as sl
import test_head_epoch_reference_gpu as t_he
import test_memory_prune_gpu as t_mem
import test_poison_predict_tail_gpu as pp
from test_predict_tail_gpu import POST_SHAPES, _post_inputs

pytestmark = pytest.mark.gpu

_T0 = time.time()
HOST_WAITS = {"ac_predict_post": "blend.hip:321-334 with h_out: spin on the host flag, then hipStreamSynchronize"}
FAMILY = ("ac_head_", "ac_ewc_", "ac_fisher_", "ac_memory_", "ac_strategic_", "ac_predict_post", "ac_blend_topk", "ac_proto_scores", "ac_rows_to_class",
          "ac_softmax_rows", "ac_sigmoid", "ac_l2_normalize_rows")
SEEN, CALLED = {}, set()
TOL = 1e-4
WAITING = ("train:", "best_response:", "strategic_loss:")
EPOCH_CASES = ("inst-kc16-r3-ewc", "ragged-640", "limit-c17", "bce-c6-ldt")


class Case:
    """live: the device inputs that arrive late; stale: other valid values; run() -> nested device result; check(host result)"""

    def __init__(self, live, stale, run, check):
        self.live, self.stale, self.run, self.check = live, stale, run, check


# ---- head forward and the row kernels -----------------------------------------------------------------------------------------
def _forward_case(dev):
    from adaptive_classifier import AdaptiveHead, ops
    D, C, hidden, B = 640, 7, [520, 260], 37
    head = AdaptiveHead(D, C, hidden).to(dev).eval()
    g = torch.Generator().manual_seed(21)
    X = torch.nn.functional.normalize(torch.randn(B, D, generator=g), dim=1).to(dev)
    Xs = torch.nn.functional.normalize(torch.randn(B, D, generator=g), dim=1).to(dev)
    ref = AdaptiveHead(D, C, hidden).double().eval()

    def run():
        Z = head.forward_native(X)
        return [Z, ops.softmax_rows(Z), ops.sigmoid(Z), ops.l2_normalize_rows(X * 3.0)]

    def check(got):
        with torch.no_grad():
            Zr = ref(X.cpu().double()).numpy()
        assert np.abs(got[0] - Zr).max() < TOL
        Z = got[0].astype(np.float64)
        assert np.abs(got[1] - torch.softmax(torch.from_numpy(Z), 1).numpy()).max() < 1e-6
        assert np.abs(got[2] - torch.sigmoid(torch.from_numpy(Z)).numpy()).max() < 1e-6
        assert np.abs(got[3] - X.cpu().double().numpy()).max() < 1e-6
    return Case([X], [Xs], run, check)


# ---- fused epoch / fused step ---------------------------------------------------------------------------------------------------
def _epoch_case(cid, dev):
    case = t_he._BY_ID[cid]
    flat0 = HR.make_head_module(case).flat_params().detach().clone()
    data = HR.make_data(case, flat0)
    ref, _ = HR.run_ref(case, data, flat0, torch.float64)
    want, bounds = HR.state_of(ref), HR.bounds_of(case)
    dd = t_he._device_data(case, data, dev)
    Xd, yd, Td, od = dd[:4]
    live = [t for t in (Xd, yd, Td, od) if t is not None]
    stale = [Xd.flip(0).clone()] + ([(yd + 1) % case.C] if yd is not None else []) + ([(1.0 - Td).clone()] if Td is not None else []) \
        + ([od.flip(0).clone()] if od is not None else [])
    selection = t_he._selection_device() is None

    def run():
        out = []
        for entry, per in zip(("epoch", "steps"), case.expected_launches):
            state, deltas, bits = t_he._run_leg(case, data, dd, flat0, dev, entry, False)
            dv = HR.deviation(state, want)                          # (state_of's host copies: compared where they are made)
            for q in HR.QUANTITIES:
                assert dv[q] <= bounds[q], (cid, entry, q, dv[q], bounds[q])
            if selection:
                assert deltas == [per] * case.epochs, (cid, entry, deltas)        # a stream change does not change the branch
            out.append(bits)
        return out

    def check(got):
        assert np.array_equal(got[0], got[1]), "the epoch call and the step loop differ"
    return Case(live, stale, run, check)


# ---- explicit-mask step, BCE loss -----------------------------------------------------------------------------------------------
def _step_case(dev):
    from adaptive_classifier import AdaptiveHead, MultiLabelAdaptiveHead
    from adaptive_classifier.training import HeadTrainer, LOSS_BCE_SIGMOID
    from oracle import head_oracle
    from test_head_gpu import _data
    D, C, hidden, B = 768, 4, [768, 384], 32
    X, y = _data(B, D, C, seed=5)
    Xs, ys = _data(B, D, C, seed=6)
    Xd, yd = X.to(dev), y.to(dev)
    g = torch.Generator().manual_seed(3)
    T = (torch.rand(B, C, generator=g) < 0.3).float()
    Td, Ts = T.to(dev), (1.0 - T).to(dev)
    ref0 = head_oracle.make_head(D, C, hidden)
    flat0 = head_oracle.flat(ref0).clone()
    ref = head_oracle.make_head(D, C, hidden).train()
    opt = torch.optim.AdamW(ref.parameters(), lr=0.001, weight_decay=0.01, betas=(0.9, 0.999))
    ce, _, gn = head_oracle.train_step(ref, opt, X, y, masks=None, p=0.0)
    want_flat = head_oracle.flat(ref).clone()
    torch.manual_seed(7)
    ml0 = MultiLabelAdaptiveHead(D, C, hidden)
    mlflat0 = ml0.flat_params().detach().clone()
    mlref = MultiLabelAdaptiveHead(D, C, hidden).double().eval()
    with torch.no_grad():
        for p_, q_ in zip(mlref.parameters(), ml0.parameters()):
            p_.copy_(q_.double())
    with torch.no_grad():
        want_bce = float(torch.nn.functional.binary_cross_entropy_with_logits(mlref.model(X.double()), T.double()))

    def run():
        head = AdaptiveHead(D, C, hidden).to(dev)
        with torch.no_grad():
            head.flat_params().copy_(flat0.to(dev))
        tr = HeadTrainer(head)
        loss, out = tr.step(Xd, yd, None, None, 0.0)
        ml = MultiLabelAdaptiveHead(D, C, hidden).to(dev)
        with torch.no_grad():
            ml.flat_params().copy_(mlflat0.to(dev))
        tm = HeadTrainer(ml)
        bce = tm.forward_backward_loss(Xd, targets=Td, loss_kind=LOSS_BCE_SIGMOID, dropout_p=0.0)
        return [loss.clone(), out.clone(), tr.flat.clone(), bce.clone(), tm.grads.clone()]

    def check(got):
        assert abs(float(got[0][0]) - ce) < TOL and abs(float(got[1][1]) - gn) < TOL * max(1.0, gn)
        assert np.abs(got[2] - want_flat.numpy()).max() < 5e-5
        assert np.isfinite(got[4]).all() and abs(float(got[3][0]) - want_bce) < TOL, (float(got[3][0]), want_bce)
    return Case([Xd, yd, Td], [Xs.to(dev), ys.to(dev), Ts], run, check)


# ---- EWC ------------------------------------------------------------------------------------------------------------------------
def _ewc_case(dev):
    from adaptive_classifier.ewc import EWC
    from adaptive_classifier.models import AdaptiveHead
    from adaptive_classifier.training import HeadTrainer
    from oracle import head_oracle
    from test_head_gpu import _data
    D, hidden, C, B, lam = 640, (520, 260), 7, 32, 5.0
    Xs, _ = _data(70, D, C, seed=3)
    Xs_d = Xs.to(dev)
    batches = [Xs_d[:32], Xs_d[32:64], Xs_d[64:]]
    g = torch.Generator().manual_seed(11)
    sampled = [torch.randint(0, C, (b.shape[0],), generator=g) for b in batches]
    lab = torch.cat(sampled).to(dev)
    labs = [lab[:32], lab[32:64], lab[64:]]
    X, y = _data(B, D, C, seed=5)
    Xd, yd = X.to(dev), y.to(dev)
    X2, y2 = _data(70, D, C, seed=8)
    ref = head_oracle.make_head(D, C, list(hidden)).train()
    flat0 = head_oracle.flat(ref).clone()
    f_ref = head_oracle.fisher_from_labels(head_oracle.make_head(D, C, list(hidden)), [b.cpu() for b in batches], sampled)
    opt = torch.optim.AdamW(ref.parameters(), lr=0.001, weight_decay=0.01, betas=(0.9, 0.999))
    old_ref = flat0.clone()
    with torch.no_grad():
        for p in ref.parameters():
            p += 0.1
    pen = float(head_oracle.ewc_penalty(ref, f_ref, old_ref, lam))
    ce, pen_s, gn = head_oracle.train_step(ref, opt, X, y, masks=None, fisher_flat=f_ref, old_flat=old_ref, lam_over_B=lam / B)
    want_flat = head_oracle.flat(ref).clone()

    def run():
        head = AdaptiveHead(D, C, list(hidden)).to(dev)
        with torch.no_grad():
            head.flat_params().copy_(flat0.to(dev))
        tr = HeadTrainer(head)
        ewc = EWC.__new__(EWC)
        ewc.model, ewc.device, ewc.ewc_lambda, ewc._native = head, str(dev), lam, True
        ewc.old_flat = head.flat_params().detach().clone()
        ewc.old_params = {n: p.data.clone() for n, p in head.named_parameters()}
        head.eval()
        ewc.fisher_info = ewc._compute_fisher_native([(b, None) for b in batches], sampled_labels=labs)
        with torch.no_grad():
            for p in head.parameters():
                p += 0.1
            got = ewc.ewc_loss().clone()
        head.train()
        out3 = tr.fused_step(Xd, yd, None, 0.0, 0, fisher=ewc.fisher_flat, old_params=ewc.old_flat, lambda_over_B=lam / B).clone()
        return [ewc.fisher_flat.clone(), got, out3, tr.flat.clone()]

    def check(got):
        assert np.abs(got[0] - f_ref.numpy()).max() / f_ref.abs().max().item() < 1e-4
        assert abs(float(got[1]) - pen) < TOL * max(1.0, abs(pen))
        assert abs(got[2][0] - ce) < TOL and abs(got[2][1] - pen_s) < TOL * max(1.0, abs(pen_s)) and abs(got[2][2] - gn) < TOL * max(1.0, gn)
        assert np.abs(got[3] - want_flat.numpy()).max() < 5e-5
    return Case([Xs_d, lab, Xd, yd], [X2.to(dev), (lab + 1) % C, Xs_d[:B].clone(), (yd + 1) % C], run, check)


# ---- prune ----------------------------------------------------------------------------------------------------------------------
def _prune_case(dev, cases_, D):
    """test_memory_prune_gpu's jobs, built once and kept: the candidate rows are persistent LIVE device tensors (stale: the same
    rows in reverse order), the job table is on the device already, the outputs are refilled in stream order -- so nothing
    between the sleep and the entry waits on the host.  Every job is replayed against memory_prune_ref like the suite does."""
    from adaptive_classifier import _native as nv
    jobs = [t_mem._Job(c, M.make_rows(c), dev) for c in cases_]
    arr = (nv.ac_prune_job * len(jobs))()
    for i, job in enumerate(jobs):
        job.fill(arr[i])
    d_jobs = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev)
    sums = [j.d_sum.clone() for j in jobs]
    stale = []
    for j in jobs:
        c, host = j.c, j.rows_host.copy()
        view = host[c.offset:c.offset + c.n * c.stride].reshape(c.n, c.stride)
        view[:, :c.D] = j.rows[::-1]
        stale.append(torch.from_numpy(host).to(dev))

    def run():
        for j, s0 in zip(jobs, sums):
            j.d_sum.copy_(s0)
            j.d_alive.fill_(t_mem.ALIVE_FILL)
            j.d_dist.fill_(t_mem.DIST_FILL)
            j.d_drop.fill_(t_mem.DROP_FILL)
        with torch.cuda.device(dev):
            rc = nv.lib().ac_memory_add_prune(ctypes.cast(arr, ctypes.c_void_p), nv.ptr(d_jobs), len(jobs), D, nv.stream_ptr(dev))
        assert rc == 0
        return [[j.d_drop, j.d_alive, j.d_dist, j.d_sum] for j in jobs]

    def check(got):
        for j, (dr, a, d, s_) in zip(jobs, got):
            assert s_[-1] == t_mem.DIST_FILL and a[-1] == t_mem.ALIVE_FILL and d[-1] == t_mem.DIST_FILL and dr[-1] == t_mem.DROP_FILL
            c = j.c
            assert M.replay(j.rows, c.n_old, c.n_new, c.cap, j.sum0, dr[:-1], a[:-1], d[:-1], s_[:-1]) == [], c.name
    return Case([j.d_rows for j in jobs], stale, run, check)


# ---- strategic: best response and strategic loss ------------------------------------------------------------------------------
import strategic_ref as SR                              # noqa: E402
import test_strategic_reference_gpu as t_sr              # noqa: E402


class _Pool:
    """persistent live device tensors of a case's native calls, in call order: the first (plain) run builds them with their true
    values and a stale stand-in each, later runs get the same tensors back"""

    def __init__(self):
        self.live, self.stale, self.i = [], [], 0

    def get(self, make_true, make_stale):
        if self.i == len(self.live):
            t = make_true()
            self.live.append(t)
            self.stale.append(make_stale(t))
        self.i += 1
        return self.live[self.i - 1]


def _strategic_case(kind, case, dev):
    """test_strategic_reference_gpu's own test function (its fp64 comparison included) with its C-ABI helper replaced by one
    whose X (and labels) are the pool's live tensors; the call's outputs are kept, cloned in stream order"""
    from adaptive_classifier import _native as nv
    pool, kept, consts = _Pool(), [], {}

    def const(key, make):
        if key not in consts:
            consts[key] = make()
        return consts[key]

    def best_response(dims, flat, X, feat, delta, coef, cost_type, mode, masks=None, seed=0, ws_short=0, dev=None):
        assert not ws_short
        D, H1, H2, C = dims
        b, Mc = X.shape[0], len(feat)
        nd = nv.ac_head_dims(D, H1, H2, C)

        def padded():
            big = torch.full((b, D + 3), float("nan"), device=dev)
            big[:, :D] = X.to(dev)
            return big
        Xbig = pool.get(padded, lambda t: t.flip(0).clone())
        k = pool.i
        fd = const(("f", k), lambda: torch.tensor(list(feat), dtype=torch.int32, device=dev))
        dd = const(("d", k), lambda: torch.as_tensor(delta, dtype=torch.float32).to(dev))
        cd = const(("c", k), lambda: coef.to(dev))
        fl = None if flat is None else const(("w", k), lambda: flat.to(dev))
        m1 = m2 = None
        if masks is not None:
            m1, m2 = const(("m", k), lambda: (t_sr._u8(masks[0], dev), t_sr._u8(masks[1], dev)))
        Ybig = torch.full((b, D + 5), t_sr.SENTINEL, device=dev)
        out = {"choice": torch.full((b,), -7, dtype=torch.int32, device=dev), "util": torch.full((b,), t_sr.SENTINEL, device=dev),
               "util_all": torch.full((b, Mc), t_sr.SENTINEL, device=dev), "logits": torch.full((b, C), t_sr.SENTINEL, device=dev)}
        need = ctypes.c_size_t(0)
        rc = nv.lib().ac_strategic_workspace(ctypes.byref(nd), b, Mc, ctypes.byref(need))
        ws = torch.empty(max(need.value, 256), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            rc2 = nv.lib().ac_strategic_best_response(
                ctypes.byref(nd), nv.ptr(fl), nv.ptr(Xbig), Xbig.stride(0), b, nv.ptr(fd), nv.ptr(dd), Mc, nv.ptr(cd), cost_type, mode,
                nv.ptr(m1), nv.ptr(m2), t_sr.P, seed & SR.MASK64, nv.ptr(out["choice"]), nv.ptr(out["util"]), nv.ptr(out["util_all"]),
                nv.ptr(Ybig), Ybig.stride(0), nv.ptr(out["logits"]), nv.ptr(ws), ws.numel(), nv.stream_ptr(dev))
        kept.append([Ybig.clone()] + [v.clone() for v in out.values()])
        res = {k_: v.cpu() for k_, v in out.items()}
        assert (Ybig[:, D:] == t_sr.SENTINEL).all()
        res.update(rc_ws=rc, rc=rc2, Y=Ybig[:, :D].cpu())
        return res

    def loss_call(dims, flat, X2, y, lam, masks2=None, use_seed=0, seed=0, dev=None):
        D, H1, H2, C = dims
        B = X2.shape[0] // 2
        nd = nv.ac_head_dims(D, H1, H2, C)
        Xd = pool.get(lambda: X2.to(dev).contiguous(), lambda t: t.flip(0).clone())
        yd = pool.get(lambda: y.to(dev).contiguous(), lambda t: (t + 1) % C)
        k = pool.i
        fl = const(("w", k), lambda: flat.to(dev))
        m1 = m2 = None
        if masks2 is not None:
            m1, m2 = const(("m", k), lambda: (t_sr._u8(masks2[0], dev), t_sr._u8(masks2[1], dev)))
        loss = torch.full((1,), t_sr.SENTINEL, device=dev)
        grads = torch.full_like(fl, t_sr.SENTINEL)
        mis = torch.full((B,), -7, dtype=torch.int32, device=dev)
        need = ctypes.c_size_t(0)
        nv.check(nv.lib().ac_head_workspace(ctypes.byref(nd), 2 * B, ctypes.byref(need)), "ac_head_workspace")
        ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            nv.check(nv.lib().ac_head_fwd_bwd_strategic(
                ctypes.byref(nd), nv.ptr(fl), nv.ptr(Xd), Xd.stride(0), nv.ptr(yd), nv.ptr(m1), nv.ptr(m2), t_sr.P, use_seed,
                seed & SR.MASK64, B, lam, nv.ptr(loss), nv.ptr(grads), nv.ptr(mis), nv.ptr(ws), ws.numel(), nv.stream_ptr(dev)),
                "ac_head_fwd_bwd_strategic")
        kept.append([loss.clone(), grads.clone(), mis.clone()])
        return loss.cpu(), grads.cpu(), mis.cpu()

    def run():
        pool.i = 0
        kept.clear()
        with pytest.MonkeyPatch.context() as mp:
            if kind == "best_response":
                mp.setattr(t_sr, "_best_response", best_response)
                t_sr.test_b_best_response_matches_fp64(dev, case)
            else:
                mp.setattr(t_sr, "_loss_call", loss_call)
                t_sr.test_c_strategic_loss_matches_fp64_autograd(dev, case)
        assert kept
        return list(kept)
    c = Case(pool.live, pool.stale, run, lambda got: None)          # (the lists fill during the first, plain run)
    return c


# ---- prediction tail --------------------------------------------------------------------------------------------------------------
def _tail_case(b, C, kp, k, mode, dev):
    case = pp._table_case(b, C, kp, k, True, True, True, dev)
    other = _post_inputs(C, kp, b, np.random.default_rng(977 + b), dev)
    want = pp._reference(case)
    live, stale = [case["D"], case["I"], case["Z"]], [other[0], other[1], other[6]]

    def run():
        with pytest.MonkeyPatch.context() as mp:
            c = pp._clf(case, dev)
            lists, last_nan = pp._run(c, case, mode, mp)
        assert last_nan is False
        return [[(l, float(s)) for l, s in r] for r in lists]

    return Case(live, stale, run, lambda got: pp._check_lists([[tuple(x) for x in r] for r in got], want))


BUILDERS = {"head_forward": _forward_case, "explicit_mask_step_and_bce": _step_case, "ewc_fisher_penalty_fused_step": _ewc_case,
            "prune_one_job": lambda dev: _prune_case(dev, M.CASES[:1], M.CASES[0].D),
            "prune_five_jobs": lambda dev: _prune_case(dev, M.MULTI_JOB_CASES, M.MULTI_JOB_D)}
for _k, _c in (("best_response", SR.BR_CASES[0]), ("best_response", SR.BR_CASES[-1]), ("strategic_loss", SR.LOSS_CASES[0]),
               ("strategic_loss", SR.LOSS_CASES[-1])):
    BUILDERS[f"{_k}:{getattr(_c, 'id', None) or 'B%d_C%d_seed%d' % (_c.B, _c.C, _c.seed)}"] = lambda dev, k=_k, c=_c: _strategic_case(k, c, dev)
for _cid in EPOCH_CASES:
    BUILDERS[f"train:{_cid}"] = lambda dev, cid=_cid: _epoch_case(cid, dev)
for _b, _C, _kp, _k in POST_SHAPES:
    for _mode, _what in (("1", "host_waited"), ("2", "device_stage"), ("0", "separate_kernels")):
        BUILDERS[f"tail_{_what}:b{_b}_C{_C}_kp{_kp}_k{_k}"] = lambda dev, a=(_b, _C, _kp, _k), m=_mode: _tail_case(*a, m, dev)


@pytest.fixture(scope="module")
def world(cuda_dev):
    global _T0
    _T0 = time.time()
    from adaptive_classifier import _native as nv
    w = types.SimpleNamespace(dev=cuda_dev, side=torch.cuda.Stream(device=cuda_dev), cases={}, plain={}, host_ms={})
    per_ms = sl.calibrate(cuda_dev)
    with sl.EntrySpy(nv) as spy:
        w.spy = spy
        for name, build in BUILDERS.items():
            c = w.cases[name] = build(cuda_dev)
            torch.cuda.synchronize()
            out, w.host_ms[name] = sl.plain(spy, c.run)
            w.plain[name] = sl.to_host(out)
        # the training and strategic cases synchronise between their native calls (the suites' own functions): their span is not
        # a non-waiting host time, and the spy lags the stream again after each such wait
        steady = {n: ms for n, ms in w.host_ms.items() if not n.startswith(WAITING)}
        slowest = max(steady, key=steady.get)
        w.lag_ms = sl.choose_lag(steady[slowest])
        print(f"\nMEASURED test_stream_head_gpu: {per_ms:.0f} sleep cycles per ms; slowest non-waiting case {slowest} {w.host_ms[slowest]:.2f} ms of host "
              f"time between its first and last native call; lag {w.lag_ms:.0f} ms")
        yield w
    print(f"\nMEASURED test_stream_head_gpu wall time {time.time() - _T0:.1f} s")


@pytest.mark.parametrize("name", list(BUILDERS))
def test_side_stream_lags_and_inputs_arrive_late(name, world):
    w, c = world, world.cases[name]
    out, readings = sl.side_late(w.spy, w.side, w.lag_ms, c.run, c.live, c.stale)
    sl.assert_enqueued(readings, HOST_WAITS, name)
    if name.startswith("tail_device_stage"):                 # without h_out ac_predict_post does not wait
        assert not any(done for n, done in readings if n == "ac_predict_post"), name
    CALLED.update(n for n, _ in readings)
    sl.note(__name__, readings, HOST_WAITS)
    for n, done in readings:
        if not done:
            SEEN[n] = True
    got = sl.to_host(out)
    assert poison.same_bits(w.plain[name], got), "work ran ahead of the side stream: " + poison.first_difference(w.plain[name], got)
    c.check(got)


@pytest.mark.parametrize("name", list(BUILDERS))
def test_default_stream_lags_call_on_an_idle_side_stream(name, world):
    w, c = world, world.cases[name]
    got, readings = sl.default_lags(w.spy, w.side, w.lag_ms, c.run)
    assert poison.same_bits(w.plain[name], got), "work went to the default stream: " + poison.first_difference(w.plain[name], got)
    c.check(got)


def test_every_head_side_entry_was_seen_returning_under_a_sleeping_stream(world):
    """The guard for this module's entries (the scenario-A tests above fill SEEN)."""
    from adaptive_classifier import _native as nv
    mine = {n for n in nv.exported_symbols() if n.startswith(FAMILY)} & sl.stream_entries()
    assert mine
    missing = sorted(n for n in mine if not SEEN.get(n) and n not in HOST_WAITS)
    assert not missing, f"never seen returning under a lagging stream: {missing}"
    assert SEEN.get("ac_predict_post"), "ac_predict_post without h_out must return without waiting"
    assert set(HOST_WAITS) <= CALLED, "a listed host wait was never called"


# For the record (one run on an MI355X, inside the whole suite): 2412851 sleep cycles per ms; slowest non-waiting case
# tail_host_waited:b5_C2048_kp1024_k3, 2.29 ms of host time between its first and last native call; lag 23 ms; module wall time 3.7 s
# (with the lag sized from the waiting strategic cases too -- 18.33 ms, lag 183 ms -- the module took 23 s).
