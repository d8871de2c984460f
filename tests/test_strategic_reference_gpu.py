"""GPU suite: strategic mode (`ac_strategic_best_response`, `ac_head_fwd_bwd_strategic`, adaptive_classifier/strategic.py) against the
fp64 reference of tests/strategic_ref.py, over the kernels' branches and with the default (seeded) dropout path included.
tests/test_strategic_ref_cpu.py proves the reference and the admissibility of every case; nothing here reads anything but
tests/strategic_ref.py's tables.

  A  seeded mode == explicit mode under the ported masks (the numpy port of ac::dropout_keep), bit for bit: the search's five
     outputs and the loss call's loss, gradient block and misprediction flags.  Both forms run the same kernels on the same kept
     units; anything short of identity is a counter or seed mistake.
  B  the search through the C ABI with the test's own tables, sharp heads, modes NONE and SEED, both cost types, X and Y padded
     (ldx = D + 3, ldy = D + 5; NaN / sentinel columns): utilities within BOUND of fp64 everywhere; the fp64 choice on every decided
     row (at least 95 % of a case, proven on the CPU), within 2 BOUND of the maximum elsewhere; the choice is the FIRST maximum
     of the device's own utilities; Y the fp32 candidate row exactly; util == util_all[choice]; logits of the chosen row within
     LOGITS_BAR; the argument checks.
  C  the strategic loss against fp64 autograd: explicit masks and use_seed, label patterns mixed / none / all, lambda = 0, exact
     ties, NaN rows.
  D  four steps of the default training path (StrategicOptimizer.strategic_loss(masks=None, seed) + optimizer_step) against the
     fp64 trajectory: choices and flags equal per step, loss / parameters / m / v / raw gradients within strategic_ref.traj_bounds.
  E  StrategicEvaluator.evaluate_robustness, head in train mode, replay=False: the dictionary equals the fp64 one.

Observed on an MI355X: see the table at the end of this file (for the record -- no bound comes from it).
"""
import ctypes
import math
import time

import numpy as np
import pytest
import torch

import strategic_ref as R

pytestmark = pytest.mark.gpu

AC_EINVAL, AC_EWORKSPACE = -1, -3
MASK_NONE, MASK_EXPLICIT, MASK_SEED = 0, 1, 2
COSTS = (0, 1)                          # AC_STRAT_COST_SEPARABLE, AC_STRAT_COST_LINEAR
SENTINEL = -777.0
P = R.DROPOUT_P

_SEEN = {}                              # quantity -> observed maximum (printed at the end of the module)


def _see(key, value):
    _SEEN[key] = max(_SEEN.get(key, 0.0), float(value))


@pytest.fixture(scope="module", autouse=True)
def _wall_time(cuda_dev):
    t0 = time.time()
    yield
    print(f"\n[strategic reference] module wall time {time.time() - t0:.1f} s")
    for k in sorted(_SEEN):
        print(f"[strategic reference] observed max  {k:28s} {_SEEN[k]:.1e}")


def _u8(m, dev):
    return torch.from_numpy(np.ascontiguousarray(m)).to(torch.uint8).to(dev).contiguous()


def _best_response(dims, flat, X, feat, delta, coef, cost_type, mode, masks=None, seed=0, ws_short=0, dev=None):
    """One `ac_strategic_best_response` call on padded X / Y; returns the rc and the outputs (nothing is checked but the padding)."""
    from adaptive_classifier import _native as nv
    D, H1, H2, C = dims
    b, M = X.shape[0], len(feat)
    nd = nv.ac_head_dims(D, H1, H2, C)
    Xbig = torch.full((b, D + 3), float("nan"), device=dev)
    Xbig[:, :D] = X.to(dev)
    Xkeep = Xbig.clone()
    Ybig = torch.full((b, D + 5), SENTINEL, device=dev)
    fd = torch.tensor(list(feat), dtype=torch.int32, device=dev)
    dd = torch.as_tensor(delta, dtype=torch.float32).to(dev)
    cd = coef.to(dev)
    out = {"choice": torch.full((b,), -7, dtype=torch.int32, device=dev), "util": torch.full((b,), SENTINEL, device=dev),
           "util_all": torch.full((b, M), SENTINEL, device=dev), "logits": torch.full((b, C), SENTINEL, device=dev)}
    fl = None if flat is None else flat.to(dev)
    m1 = m2 = None
    if masks is not None:
        m1, m2 = _u8(masks[0], dev), _u8(masks[1], dev)
    need = ctypes.c_size_t(0)
    rc = nv.lib().ac_strategic_workspace(ctypes.byref(nd), b, M, ctypes.byref(need))
    if rc != 0:
        need = ctypes.c_size_t(1 << 20)
    ws = torch.empty(max(need.value, 256), dtype=torch.uint8, device=dev)
    ws_bytes = need.value - ws_short if ws_short else ws.numel()
    with torch.cuda.device(dev):
        rc2 = nv.lib().ac_strategic_best_response(
            ctypes.byref(nd), nv.ptr(fl), nv.ptr(Xbig), Xbig.stride(0), b, nv.ptr(fd), nv.ptr(dd), M, nv.ptr(cd), cost_type, mode,
            nv.ptr(m1), nv.ptr(m2), P, seed & R.MASK64, nv.ptr(out["choice"]), nv.ptr(out["util"]), nv.ptr(out["util_all"]),
            nv.ptr(Ybig), Ybig.stride(0), nv.ptr(out["logits"]), nv.ptr(ws), ws_bytes, nv.stream_ptr(dev))
    torch.cuda.synchronize()
    assert torch.equal(Xbig[:, :D], Xkeep[:, :D]) and torch.isnan(Xbig[:, D:]).all()        # X is only read
    assert (Ybig[:, D:] == SENTINEL).all()                                                  # nothing written past D
    out = {k: v.cpu() for k, v in out.items()}
    out.update(rc_ws=rc, rc=rc2, Y=Ybig[:, :D].cpu())
    return out


def _loss_call(dims, flat, X2, y, lam, masks2=None, use_seed=0, seed=0, dev=None):
    """One `ac_head_fwd_bwd_strategic` call; returns (loss fp32 [1], gradient block, mispred int32 [B]) on the host."""
    from adaptive_classifier import _native as nv
    D, H1, H2, C = dims
    B = X2.shape[0] // 2
    nd = nv.ac_head_dims(D, H1, H2, C)
    fl, Xd, yd = flat.to(dev), X2.to(dev).contiguous(), y.to(dev).contiguous()
    m1 = m2 = None
    if masks2 is not None:
        m1, m2 = _u8(masks2[0], dev), _u8(masks2[1], dev)
    loss = torch.full((1,), SENTINEL, device=dev)
    grads = torch.full_like(fl, SENTINEL)
    mis = torch.full((B,), -7, dtype=torch.int32, device=dev)
    need = ctypes.c_size_t(0)
    nv.check(nv.lib().ac_head_workspace(ctypes.byref(nd), 2 * B, ctypes.byref(need)), "ac_head_workspace")
    ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        nv.check(nv.lib().ac_head_fwd_bwd_strategic(
            ctypes.byref(nd), nv.ptr(fl), nv.ptr(Xd), Xd.stride(0), nv.ptr(yd), nv.ptr(m1), nv.ptr(m2), P, use_seed, seed & R.MASK64,
            B, lam, nv.ptr(loss), nv.ptr(grads), nv.ptr(mis), nv.ptr(ws), ws.numel(), nv.stream_ptr(dev)), "ac_head_fwd_bwd_strategic")
    torch.cuda.synchronize()
    return loss.cpu(), grads.cpu(), mis.cpu()


def _device_head(flat, dims, dev):
    """An AdaptiveHead on the device whose flat block is `flat`."""
    from adaptive_classifier import AdaptiveHead
    D, H1, H2, C = dims
    head = AdaptiveHead(D, C, [H1, H2]).to(dev)
    with torch.no_grad():
        for p, t in zip([q for l in head.linears() for q in (l.weight, l.bias)], R.split(flat, dims)):
            p.copy_(t)
    assert torch.equal(head.flat_params().cpu(), flat)
    return head


# ---- A: seeded == explicit under the ported masks, bit for bit --------------------------------------------------------------------
A_SHAPES = [(R.S768, 4, 16, 50), (R.S70, 65, 3, 50), (R.SR4, 7, 33, 50), (R.S64, 5, 40, 1)]       # (dims, C, b, M)
A_SEEDS = (0xD1B54A32D192ED03, 0x00000001F0000000 + 12345)                                        # bits above 2^32 set


@pytest.mark.parametrize("hidden,C,b,M", A_SHAPES, ids=lambda v: str(v).replace(" ", ""))
def test_a_seeded_search_equals_explicit_masks_bit_for_bit(cuda_dev, hidden, C, b, M):
    dims = hidden + (C,)
    D, H1, H2 = hidden
    g = torch.Generator().manual_seed(b)
    X = torch.nn.functional.normalize(torch.randn(b, D, generator=g), dim=1)
    coef = torch.randn(D, generator=g) * 0.05
    flat = R.sharp_head(D, H1, H2, C, seed=D + C)
    feat, delta = R.std_table(D, M)
    for seed in A_SEEDS:
        got_s = _best_response(dims, flat, X, feat, delta, coef, 0, MASK_SEED, seed=seed, dev=cuda_dev)
        got_e = _best_response(dims, flat, X, feat, delta, coef, 0, MASK_EXPLICIT, masks=R.masks_of(seed, b, M, H1, H2, P), dev=cuda_dev)
        assert got_s["rc"] == 0 and got_e["rc"] == 0
        for k in ("choice", "util", "util_all", "Y", "logits"):
            assert torch.equal(got_s[k], got_e[k]), (k, hex(seed))
        none = _best_response(dims, flat, X, feat, delta, coef, 0, MASK_NONE, dev=cuda_dev)
        assert not torch.equal(none["util_all"], got_s["util_all"])                    # (the masks do something)


@pytest.mark.parametrize("hidden,C,B,M", A_SHAPES[:3], ids=lambda v: str(v).replace(" ", ""))
def test_a_seeded_loss_equals_explicit_masks_bit_for_bit(cuda_dev, hidden, C, B, M):
    dims = hidden + (C,)
    D, H1, H2 = hidden
    g = torch.Generator().manual_seed(B)
    X2 = torch.nn.functional.normalize(torch.randn(2 * B, D, generator=g), dim=1)
    y = torch.randint(0, C, (B,), generator=g)
    flat = R.sharp_head(D, H1, H2, C, seed=D + C)
    for seed in A_SEEDS:
        ls, gs, ms = _loss_call(dims, flat, X2, y, 0.7, use_seed=1, seed=seed, dev=cuda_dev)
        le, ge, me = _loss_call(dims, flat, X2, y, 0.7, masks2=R.layer_masks(seed, 2 * B, H1, H2, P), dev=cuda_dev)
        assert torch.equal(ls, le) and torch.equal(gs, ge) and torch.equal(ms, me), hex(seed)
        assert 0 < int(ms.sum()) and torch.isfinite(gs).all()
        l0, _, _ = _loss_call(dims, flat, X2, y, 0.7, dev=cuda_dev)
        assert not torch.equal(l0, ls)


# ---- B: the search against fp64 ---------------------------------------------------------------------------------------------------
_REF_B = {}


def _ref_b(case, seeded):
    key = (case.id, seeded)
    if key not in _REF_B:
        d = R.br_data(case)
        u, z, Y = R.utilities(d.flat, case.dims, d.X, d.feat, d.delta, d.coef, R.br_masks(case, seeded))
        _REF_B[key] = (d, u, z, Y, R.choose(u), R.decided_gap(u) > 2 * R.BOUND)
    return _REF_B[key]


@pytest.mark.parametrize("case", R.BR_CASES, ids=lambda c: c.id)
def test_b_best_response_matches_fp64(cuda_dev, case):
    rows = torch.arange(case.b)
    for seeded in (False, True):
        d, u64, z64, Yref, want, sure = _ref_b(case, seeded)
        for ct in COSTS:
            r = _best_response(case.dims, d.flat, d.X, d.feat, d.delta, d.coef, ct, MASK_SEED if seeded else MASK_NONE,
                               seed=case.drop_seed, dev=cuda_dev)
            assert r["rc_ws"] == 0 and r["rc"] == 0
            ch = r["choice"].long()
            du = (r["util_all"].double() - u64).abs().max().item()
            behind = (u64.max(1).values - u64[rows, ch]).max().item()
            dz = 0.0 if z64 is None else (r["logits"].double() - z64[rows, ch]).abs().max().item()
            print(f"\n[search vs fp64] {case.id:14s} {'seed' if seeded else 'none'} cost {ct}: utility {du:.1e}  decided rows "
                  f"{int(sure.sum())}/{case.b}  wrong among them {int((ch[sure] != want[sure]).sum())}  behind the maximum "
                  f"{behind:.1e}  logits {dz:.1e}", end="")
            _see("B utility", du)
            _see("B logits", dz)
            assert du <= R.BOUND
            assert torch.equal(ch[sure], want[sure])
            assert behind <= 2 * R.BOUND
            assert torch.equal(ch, torch.from_numpy(np.argmax(r["util_all"].numpy(), axis=1)))      # the FIRST maximum
            assert torch.equal(r["Y"], Yref[rows, ch])
            assert torch.equal(r["util"], r["util_all"][rows, ch])
            if z64 is None:
                assert (r["logits"] == SENTINEL).all()                                              # no head: nothing written
            else:
                assert dz <= R.LOGITS_BAR
            if case.id == "c1-all-ties":
                assert ch.tolist() == [0] * case.b and (r["util_all"][:, 0] == 1.0).all()
            if case.id == "no-head":
                assert ch.tolist() == [0] * case.b and (r["util"] == 0.25).all()
            if case.id == "special-table" and not seeded:            # equal moves: equal utilities exactly, the first one wins
                ua = r["util_all"]
                assert torch.equal(ua[:, 1], ua[:, 2]) and torch.equal(ua[:, 1], ua[:, 5]) and torch.equal(ua[:, 0], ua[:, 6])
                assert not set(ch.tolist()) & {2, 5, 6}


def test_b_argument_checks_launch_nothing(cuda_dev):
    D, H1, H2, C = dims = R.S64 + (7,)
    flat = R.sharp_head(D, H1, H2, C, seed=1)
    X = torch.nn.functional.normalize(torch.randn(4, D, generator=torch.Generator().manual_seed(0)), dim=1)
    coef = torch.full((D,), 0.05)

    def untouched(r):
        return (r["choice"] == -7).all() and (r["util"] == SENTINEL).all() and (r["Y"] == SENTINEL).all()

    f65, d65 = [-1] + [0] * 64, torch.zeros(65)
    r = _best_response(dims, flat, X, f65, d65, coef, 0, MASK_NONE, dev=cuda_dev)
    assert r["rc_ws"] == AC_EINVAL and r["rc"] == AC_EINVAL and untouched(r)
    r = _best_response(dims, flat, X, [], torch.zeros(0), coef, 0, MASK_NONE, dev=cuda_dev)
    assert r["rc_ws"] == AC_EINVAL and r["rc"] == AC_EINVAL and untouched(r)
    f50, d50 = R.std_table(D)
    r = _best_response((D, H1, H2, 2049), None, X, f50, d50, coef, 0, MASK_NONE, dev=cuda_dev)
    assert r["rc_ws"] == AC_EINVAL and r["rc"] == AC_EINVAL and untouched(r)
    r = _best_response(dims, flat, X, f50, d50, coef, 0, MASK_NONE, ws_short=1, dev=cuda_dev)
    assert r["rc_ws"] == 0 and r["rc"] == AC_EWORKSPACE and untouched(r)
    r = _best_response(dims, flat, X, f50, d50, coef, 0, MASK_NONE, dev=cuda_dev)
    assert r["rc"] == 0 and not untouched(r)


# ---- C: the strategic loss against fp64 autograd -------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.LOSS_CASES, ids=lambda c: c.id)
def test_c_strategic_loss_matches_fp64_autograd(cuda_dev, case):
    flat, X2, masks2 = R.loss_data(case)
    B, lam = case.B, R.LOSS_LAMBDA
    z64 = R.forward(R.split(flat.double(), case.dims), X2.double(), masks2, P)
    pred = z64[B:].argmax(1)
    runs = {}
    for pattern, n_wrong in zip(R.LOSS_PATTERNS, (B // 2, 0, B)):
        y = R.loss_labels(pred, case.C, pattern)
        for lam_ in ((lam, 0.0) if pattern != "all" else (lam,)):
            l64, g64, w64, _ = R.strategic_loss(flat, case.dims, X2, y, lam_, masks2)
            assert int(w64.sum()) == n_wrong
            for form in ("explicit", "seed"):
                if form == "explicit":
                    loss, grads, mis = _loss_call(case.dims, flat, X2, y, lam_, masks2=masks2, dev=cuda_dev)
                else:
                    loss, grads, mis = _loss_call(case.dims, flat, X2, y, lam_, use_seed=1, seed=case.drop_seed, dev=cuda_dev)
                dl, dg = abs(loss.item() - l64), (grads.double() - g64).abs().max().item()
                print(f"\n[loss vs fp64] {case.id:16s} {pattern:5s} lambda {lam_:.1f} {form:8s}: loss {dl:.1e}  gradient {dg:.1e}", end="")
                _see("C loss", dl)
                _see("C gradient", dg)
                assert mis.bool().tolist() == w64.tolist()
                assert dl <= R.LOSS_BAR and dg <= R.GRAD_BAR
                runs[(pattern, lam_, form)] = (loss, grads)
    for form in ("explicit", "seed"):       # nothing mispredicted: the strategic term and its gradient rows are exactly 0
        assert torch.equal(runs[("none", lam, form)][0], runs[("none", 0.0, form)][0])
        assert torch.equal(runs[("none", lam, form)][1], runs[("none", 0.0, form)][1])
        assert not torch.equal(runs[("mixed", lam, form)][1], runs[("mixed", 0.0, form)][1]) or B == 1


@pytest.mark.parametrize("B,C,b3", [(8, 7, 0.0), (9, 130, 0.5), (70, 65, -1.25)])
def test_c_exact_ties_take_the_first_class(cuda_dev, B, C, b3):
    """W3 = 0 and a constant b3: every logit is equal, the argmax is class 0 by the first-maximum rule, every row's CE is log C."""
    D, H1, H2 = R.S64
    dims = R.S64 + (C,)
    flat = R.sharp_head(D, H1, H2, C, seed=9)
    Pv = R.split(flat, dims)
    Pv[4].zero_()
    Pv[5].fill_(b3)
    X2 = torch.randn(2 * B, D, generator=torch.Generator().manual_seed(B))
    y = torch.arange(B) % C
    y[0] = C - 1
    n_wrong = int((y != 0).sum())
    for lam in (0.0, 0.7):
        loss, grads, mis = _loss_call(dims, flat, X2, y, lam, masks2=R.layer_masks(5 << 40, 2 * B, H1, H2, P), dev=cuda_dev)
        assert mis.bool().tolist() == (y != 0).tolist()
        want = math.log(C) * (1 + lam * n_wrong / B)
        assert abs(loss.item() - want) <= 1e-6 * max(1.0, want)
        if lam == 0.0 and b3 == 0.0:                                # B = 8: the mean of eight equal fp32 numbers is exact
            assert abs(loss.item() - float(np.float32(math.log(C)))) <= float(np.spacing(np.float32(math.log(C))))
        assert (grads[:flat.numel() - C - C * H2] == 0).all()       # W3 = 0: nothing reaches the hidden layers


def test_c_nan_rows_follow_torch_argmax(cuda_dev):
    case = R.LOSS_CASES[1]                                          # B = 9, C = 7
    flat, X2, masks2 = R.loss_data(case)
    B = case.B
    X2 = X2.clone()
    X2[B + 2] = float("nan")
    X2[B + 4] = float("nan")
    z64 = R.forward(R.split(flat.double(), case.dims), X2.double(), masks2, P)
    y = z64[B:].argmax(1)                                            # NaN rows: index 0
    assert y[2] == 0 and y[4] == 0
    y[2] = 3                                                         # row B + 2 mispredicted (counted: the loss is NaN), B + 4 not
    y[6] = (y[6] + 1) % case.C
    _, _, w64, _ = R.strategic_loss(flat, case.dims, X2, y, 0.7, masks2)
    loss, _, mis = _loss_call(case.dims, flat, X2, y, 0.7, masks2=masks2, dev=cuda_dev)
    assert mis.bool().tolist() == w64.tolist() and mis.tolist()[2] == 1 and mis.tolist()[4] == 0 and mis.tolist()[6] == 1
    assert torch.isnan(loss).all()


# ---- D: the default training path ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.TRAJ_CASES, ids=lambda c: c.id)
def test_d_default_training_path_follows_the_fp64_trajectory(cuda_dev, case):
    from adaptive_classifier.strategic import LinearCostFunction, SeparableCostFunction, StrategicOptimizer
    from adaptive_classifier.training import HeadTrainer
    flat0, X, y, coef = R.traj_data(case)
    ref = R.run_traj(case)
    head = _device_head(flat0, case.dims, cuda_dev)
    head.train()
    tr = HeadTrainer(head, lr=5e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, max_grad_norm=1.0)
    opt = StrategicOptimizer(SeparableCostFunction(coef, coef) if case.cost == "separable" else LinearCostFunction(coef))
    Xd, yd = X.to(cuda_dev), y.to(cuda_dev)
    losses = []
    for i in range(case.steps):
        rows = slice(i * case.batch, (i + 1) * case.batch)
        loss, ch, mis = opt.strategic_loss(tr, Xd[rows], yd[rows], case.lam, masks=None, seed=case.step_seed(i))
        losses.append(loss.item())
        assert ch.tolist() == ref.steps[i]["choice"], (case.id, i)
        assert mis.bool().tolist() == ref.steps[i]["mispred"], (case.id, i)
        tr.optimizer_step()
    torch.cuda.synchronize()
    dev = R.traj_deviation(losses, R.traj_state(tr), ref)
    bounds = R.traj_bounds(case)
    print(f"\n[trajectory vs fp64] {case.id:24s} " + "  ".join(f"{q} {dev[q]:.1e}" for q in R.TRAJ_QUANTITIES), end="")
    for q in R.TRAJ_QUANTITIES:
        _see("D " + q, dev[q])
        assert dev[q] <= bounds[q][0], (case.id, q, dev[q], bounds[q])


# ---- E: evaluate_robustness, train mode, replay=False ----------------------------------------------------------------------------------
def test_e_train_mode_robustness_equals_the_fp64_dictionary(cuda_dev):
    from adaptive_classifier.strategic import SeparableCostFunction, StrategicEvaluator
    case = R.EVAL_CASE
    flat, X, labels, coef = R.eval_data(case)
    torch.manual_seed(case.torch_seed)
    want, _ = R.robustness(flat, case.dims, X, labels, list(case.levels), case.eval_seed, R.std_table(case.hidden[0]), coef)
    head = _device_head(flat, case.dims, cuda_dev)
    head.train()
    torch.manual_seed(case.torch_seed)
    got = StrategicEvaluator(SeparableCostFunction(coef, coef)).evaluate_robustness(head, X, labels, list(case.levels), replay=False,
                                                                                    seed=case.eval_seed)
    assert head.training
    assert got == want, (got, want)


# Observed on an MI355X, maximum over the cases of a section -- for the record (every bar above was fixed before the first run):
#
#   section / quantity                        observed    bar       fp32 torch-CPU instance
#   B  utility vs fp64                        3.5e-7      2e-5      6.7e-7
#   B  logits of the chosen row               2.0e-6      1e-4      2.7e-6
#   B  decided rows with another choice       0           0         (3 of 257 rows undecided in w768-c300 / seed, none elsewhere)
#   C  loss of one call                       1.1e-6      1e-5      1.9e-6
#   C  gradient of one call                   3.3e-6      1e-5      1.6e-6
#   D  loss per step (relative to max(1, .))  1.5e-7      1e-4      1.8e-7
#   D  parameters after 4 steps               2.7e-6      5e-5      5.5e-6
#   D  m                                      2.7e-8      1e-6      1.1e-7
#   D  v                                      4.6e-9      1e-8      4.2e-10
#   D  raw gradients of the last step         1.3e-6      1e-5      8.7e-7
#   A, E and every choice / flag of D         identical
#
# D's v is the one quantity where the device sits further from fp64 than the fp32 instance does (70 / [36, 20], 4.6e-9): the
# optimizer kernel forms 1 - beta2 in fp32 (1 - 0.999f = 0.99999e-3 x (1 - 1.3e-5)), a relative 1.3e-5 on v, inside the bar.
# Every section passed as written; no kernel line was changed.  Each assertion was run once against a scratch build with the
# mistake it targets (never committed): layer 2 of the search without ^ 0xA5A5A5A5A5A5A5A5 -> A (search), B, D, E fail; the same in
# the loss forward -> A (loss), C, D; the layer-1 counter with r * H2 + h -> A (search), B, D, E; the softmax sum of
# cand_select_kernel over `c < 64` -> every B case but C = 64 (65 .. 2048 lose the classes past the first stride; below 64 the
# loop reads stale LDS, which the older suite notices too), D, E; `>=` in its scan -> B
# c1-all-ties, special-table, no-head; strategic_loss_kernel's row loop over r < B -> A (loss), every C case, D.
# Wall time: this module takes 4 s of the GPU suite.
