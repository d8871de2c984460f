"""CPU suite: tests/strategic_ref.py is proven here, and so is the admissibility of every case the GPU module
(tests/test_strategic_reference_gpu.py) runs -- on the fp64 reference alone, before any device is involved.

  * std_table restates the product's candidate table; utilities / choose equal a literal restatement of the reference's loop
    (one single-row forward per candidate of `_generate_candidates`, `compute_cost` of the cost classes in fp64, strict `>` scan);
  * masks_of lays the counter out as the kernels do (row q * M + m, unit h -> index (q M + m) H + h; layer 2 under seed ^ 0xA5A5..),
    against a scalar Python restatement of ac::dropout_keep;
  * strategic_loss equals its definition (F.cross_entropy(reduction="none") and a Python loop over the mispredicted rows);
  * admissibility: at most 5 % undecided rows per best-response case and mode, exact ties only where they are structural; every
    loss case decides its argmax by 1e-3 and its three label patterns mispredict B // 2, 0 and B rows; no trajectory or evaluator
    row is within 2 BOUND in utility or 1e-3 in a used argmax, no kept unit within KINK_MIN_UNITS of a ReLU kink;
  * the fp32 torch-CPU instance of every trajectory case makes the fp64 run's decisions and deviates by no more than the figures
    of strategic_ref.TRAJ_FP32_DEV; the fp32 utilities and logits sit 4 x inside BOUND and LOGITS_BAR (so those bars stay).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import head_epoch_ref as E
import strategic_ref as R


# ---- the reference against literal restatements ---------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [64, 70, 768])
@pytest.mark.parametrize("M", [1, 2, 3, 5, 50, 64])
def test_std_table_is_the_products_table(D, M):
    from adaptive_classifier.strategic import candidate_table
    feat, delta = candidate_table(D, M)
    f, d = R.std_table(D, M)
    assert f == feat.tolist() and torch.equal(d, delta)


def _scalar_keep(seed, idx, p):
    """ac::dropout_keep (csrc/common.h) on Python integers."""
    m = (1 << 64) - 1
    z = (seed + idx * 0x9E3779B97F4A7C15) & m
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
    z ^= z >> 31
    return bool(np.float32(z >> 40) * np.float32(1.0 / 16777216.0) >= np.float32(p))


def test_masks_of_lays_the_counter_out_as_the_kernels_do():
    seed, rows, M, H1, H2, p = 0xD1B54A32D192ED03, 3, 5, 36, 20, 0.1
    m1, m2 = R.masks_of(seed, rows, M, H1, H2, p)
    assert m1.shape == (rows, M, H1) and m2.shape == (rows, M, H2)
    for q in range(rows):
        for m in range(M):
            for h in range(H1):
                assert m1[q, m, h] == _scalar_keep(seed, (q * M + m) * H1 + h, p)
            for h in range(H2):
                assert m2[q, m, h] == _scalar_keep(seed ^ 0xA5A5A5A5A5A5A5A5, (q * M + m) * H2 + h, p)
    assert 0.8 < m1.mean() < 0.97
    a1, a2 = R.loss_masks_of(77, 4, H1, H2, p)
    assert a1.shape == (8, H1) and a1[5, 7] == _scalar_keep(77 ^ 0x5DEECE66D, 5 * H1 + 7, p)
    assert a2[6, 3] == _scalar_keep(77 ^ 0x5DEECE66D ^ 0xA5A5A5A5A5A5A5A5, 6 * H2 + 3, p)


def _literal_best_responses(flat, dims, X, candidates_of, cost_fn, masks, p):
    """The reference's loop: per row, per candidate one single-row forward, utility = max softmax - compute_cost, strict `>`."""
    P = R.split(flat.double(), dims)
    us, choices, rows = [], [], []
    for q in range(X.shape[0]):
        x = X[q]
        cands = candidates_of(x)
        best_u, best_m, u_row = float("-inf"), 0, []
        for m, cand in enumerate(cands):
            mk = None if masks is None else (torch.from_numpy(masks[0][q, m:m + 1]), torch.from_numpy(masks[1][q, m:m + 1]))
            z = R.forward(P, cand.double().unsqueeze(0), mk, p)
            f_c = torch.max(torch.softmax(z, dim=-1).squeeze())
            u = float(f_c - cost_fn.compute_cost(x.double(), cand.double()))
            u_row.append(u)
            if u > best_u:
                best_u, best_m = u, m
        us.append(u_row)
        choices.append(best_m)
        rows.append(torch.stack(cands))
    return torch.tensor(us, dtype=torch.float64), torch.tensor(choices), torch.stack(rows)


@pytest.mark.parametrize("table", ["std", "special"])
@pytest.mark.parametrize("cost", ["separable", "linear"])
@pytest.mark.parametrize("seeded", [False, True])
def test_utilities_and_choose_equal_the_literal_loop(table, cost, seeded):
    from adaptive_classifier.strategic import LinearCostFunction, SeparableCostFunction
    D, H1, H2, C, b, p = 16, 12, 8, 3, 4, 0.1
    dims = (D, H1, H2, C)
    g = torch.Generator().manual_seed(11)
    X = F.normalize(torch.randn(b, D, generator=g), dim=1)
    coef = torch.randn(D, generator=g) * 0.05
    flat = R.sharp_head(D, H1, H2, C, seed=5)
    cf = SeparableCostFunction(coef.double(), coef.double()) if cost == "separable" else LinearCostFunction(coef.double())
    if table == "std":
        feat, delta = R.std_table(D)
        candidates_of = lambda x: cf._generate_candidates(x)
    else:
        feat, delta = R.special_table(D)

        def candidates_of(x):
            out = []
            for f, d in zip(feat, delta):
                c = x.clone()
                if 0 <= f < D:
                    c[f] += d
                out.append(c)
            return out
    masks = R.masks_of(0xABCDEF0123456789, b, len(feat), H1, H2, p) if seeded else None
    u, z, Y = R.utilities(flat, dims, X, feat, delta, coef, masks, p)
    u_lit, ch_lit, Y_lit = _literal_best_responses(flat, dims, X, candidates_of, cf, masks, p)
    assert torch.equal(Y, Y_lit)                                   # the candidate rows are _generate_candidates', fp32
    # compute_cost on fp64 copies takes y_f - x_f exactly; the search (and `utilities`) rounds it to fp32 first: |dy| <= 2 + an
    # ulp, so the two costs differ by at most |c_f| * 2^-24 * |dy| <= max|c| * 2^-23 * 1.01; the forward itself agrees to 1e-12
    tol = coef.abs().max().item() * 2.0 ** -23 * 1.01 + 1e-12
    assert (u - u_lit).abs().max().item() <= tol
    assert R.top2_gap(u_lit).min().item() > 2 * tol or table == "special"
    assert torch.equal(R.choose(u), ch_lit)
    assert z.shape == (b, len(feat), C)
    if table == "special" and not seeded:                          # equal moves: equal utilities, exactly
        assert torch.equal(u[:, 1], u[:, 2]) and torch.equal(u[:, 1], u[:, 5]) and torch.equal(u[:, 0], u[:, 6])


def test_utilities_without_a_head_and_choose_takes_the_first_maximum():
    D = 8
    X = F.normalize(torch.randn(3, D, generator=torch.Generator().manual_seed(0)), dim=1)
    coef = torch.full((D,), 0.05)
    feat, delta = R.std_table(D, 20)
    u, z, Y = R.utilities(None, (D, 1, 1, 4), X, feat, delta, coef)
    assert z is None and (u <= 0.25).all() and R.choose(u).tolist() == [0, 0, 0]
    assert torch.equal(u[:, 1], torch.full((3,), 0.25, dtype=torch.float64))        # a move down costs nothing: an exact tie
    t = torch.tensor([[1.0, 3.0, 3.0, 2.0], [5.0, 5.0, 5.0, 5.0]], dtype=torch.float64)
    assert R.choose(t).tolist() == [1, 0]
    assert R.decided_gap(t).tolist() == [1.0, float("inf")] and R.top2_gap(t).tolist() == [0.0, 0.0]


@pytest.mark.parametrize("B,C", [(1, 2), (5, 3), (9, 70)])
@pytest.mark.parametrize("lam", [0.0, 0.7])
def test_strategic_loss_equals_its_definition(B, C, lam):
    D, H1, H2, p = 16, 12, 8, 0.1
    dims = (D, H1, H2, C)
    g = torch.Generator().manual_seed(B * 100 + C)
    X2 = torch.randn(2 * B, D, generator=g)
    y = torch.randint(0, C, (B,), generator=g)
    flat = R.sharp_head(D, H1, H2, C, seed=3)
    masks2 = R.layer_masks(0x123456789ABCDEF1, 2 * B, H1, H2, p)
    loss, grad, wrong, z = R.strategic_loss(flat, dims, X2, y, lam, masks2, p)
    # the definition
    leaf = flat.double().clone().requires_grad_(True)
    zz = R.forward(R.split(leaf, dims), X2.double(), masks2, p)
    reg = F.cross_entropy(zz[:B], y)
    ce = F.cross_entropy(zz[B:], y, reduction="none")
    strat, flags = torch.zeros((), dtype=torch.float64), []
    for i in range(B):
        flags.append(int(torch.argmax(zz[B + i])) != int(y[i]))
        if flags[-1]:
            strat = strat + ce[i]
    total = reg + lam * strat / B
    total.backward()
    assert wrong.tolist() == flags and torch.equal(z, zz.detach())
    assert abs(loss - float(total.detach())) <= 1e-12 and (grad - leaf.grad).abs().max().item() <= 1e-12


def test_strategic_loss_ties_and_nan_follow_torch_argmax():
    D, H1, H2, C, B = 16, 12, 8, 6, 4
    dims = (D, H1, H2, C)
    flat = R.sharp_head(D, H1, H2, C, seed=3)
    P = R.split(flat, dims)
    P[4].zero_()
    P[5].fill_(0.25)
    X2 = torch.randn(2 * B, D, generator=torch.Generator().manual_seed(1))
    y = torch.tensor([0, 3, 0, 5])
    loss, _, wrong, z = R.strategic_loss(flat, dims, X2, y, 0.5, None)
    assert (z == 0.25).all() and wrong.tolist() == [False, True, False, True]       # every logit equal: the argmax is class 0
    assert abs(loss - (1 + 0.5 * 2 / B) * torch.log(torch.tensor(float(C), dtype=torch.float64)).item()) <= 1e-12
    flat = R.sharp_head(D, H1, H2, C, seed=3)
    X2[B + 1] = float("nan")
    loss, _, wrong, z = R.strategic_loss(flat, dims, X2, y, 0.5, None)
    assert torch.isnan(z[B + 1]).all() and bool(wrong[1]) and loss != loss           # NaN is maximal, the first NaN index is 0


# ---- admissibility of every case --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.BR_CASES, ids=lambda c: c.id)
def test_best_response_cases_decide_95_percent_of_their_rows(case):
    d = R.br_data(case)
    for seeded in (False, True):
        masks = R.br_masks(case, seeded)
        u, z, _ = R.utilities(d.flat, case.dims, d.X, d.feat, d.delta, d.coef, masks)
        undecided = int((R.decided_gap(u) <= 2 * R.BOUND).sum())
        ties = int((R.top2_gap(u) == 0).sum())
        u32, z32, _ = R.utilities(d.flat, case.dims, d.X, d.feat, d.delta, d.coef, masks, dtype=torch.float32)
        du = (u32.double() - u).abs().max().item()
        dz = 0.0 if z is None else (z32.double() - z).abs().max().item()
        print(f"\n[admissible] {case.id:14s} {'seed' if seeded else 'none'}: undecided {undecided}/{case.b}  exact ties {ties}  "
              f"distinct choices {len(set(R.choose(u).tolist()))}  fp32 instance: utility {du:.1e} logits {dz:.1e}", end="")
        assert undecided <= (1 - R.SURE_SHARE_MIN) * case.b, (case.id, seeded, undecided)
        assert case.ties or ties == 0, (case.id, seeded, ties)
        assert R.four_times_inside(du, R.BOUND) and R.four_times_inside(dz, R.LOGITS_BAR), (case.id, du, dz)
    if case.id == "c1-all-ties":
        assert R.choose(u).tolist() == [0] * case.b and (u[:, 0] == 1.0).all()


@pytest.mark.parametrize("case", R.LOSS_CASES, ids=lambda c: c.id)
def test_loss_cases_decide_every_argmax(case):
    flat, X2, masks2 = R.loss_data(case)
    z = R.forward(R.split(flat.double(), case.dims), X2.double(), masks2, R.DROPOUT_P)
    assert R.top2_gap(z[case.B:]).min().item() >= R.LOGIT_GAP
    pred = z[case.B:].argmax(1)
    for pattern, n_wrong in zip(R.LOSS_PATTERNS, (case.B // 2, 0, case.B)):
        _, _, wrong, _ = R.strategic_loss(flat, case.dims, X2, R.loss_labels(pred, case.C, pattern), R.LOSS_LAMBDA, masks2)
        assert int(wrong.sum()) == n_wrong, (case.id, pattern)


_SEPARABLE = [c for c in R.TRAJ_CASES if c.cost == "separable"]


@pytest.mark.parametrize("case", _SEPARABLE, ids=lambda c: c.id)
def test_trajectory_cases_are_admissible_and_the_fp32_instance_stays_with_fp64(case):
    ref = R.run_traj(case, track_kinks=True)
    print(f"\n[admissible] {case.id}: min utility gap {ref.min_util_gap:.1e}  min logit gap {ref.min_logit_gap:.1e}  kink units "
          f"{ref.kink_units:.2f}  grad norms {[round(g, 2) for g in ref.grad_norms]}", end="")
    assert ref.t == case.steps
    assert ref.min_util_gap > 2 * R.BOUND and ref.min_logit_gap >= R.LOGIT_GAP and ref.kink_units >= E.KINK_MIN_UNITS
    assert min(ref.grad_norms) > 1.0                              # the clip is active at every step
    assert all(0 < sum(s["mispred"]) for s in ref.steps)           # the strategic term is live
    inst = R.run_traj(case, dtype=torch.float32)
    for a, b in zip(inst.steps, ref.steps):
        assert a["choice"] == b["choice"] and a["mispred"] == b["mispred"]
    dev = R.traj_deviation([s["loss"] for s in inst.steps], R.traj_state(inst), ref)
    bounds = R.traj_bounds(case)
    print(f"\n[fp32 instance vs fp64] {case.id}: " + "  ".join(f"{q} {dev[q]:.1e} (bar {bounds[q][0]:.1e}, {bounds[q][1]})"
                                                               for q in R.TRAJ_QUANTITIES), end="")
    for q in R.TRAJ_QUANTITIES:
        assert dev[q] <= R.TRAJ_FP32_DEV[(case.hidden, case.C, case.lam)][q], (case.id, q, dev[q])


def test_the_linear_trajectory_cases_share_the_separable_reference():
    for c in R.TRAJ_CASES:
        if c.cost == "linear":
            assert any(s.hidden == c.hidden and s.C == c.C and s.lam == c.lam and s.seed == c.seed for s in _SEPARABLE)
        assert c.step_seed(3) >> 32 and c.step_seed(3) < 1 << 63


def test_evaluator_case_is_admissible_and_draws_one_number_per_row_per_level():
    case = R.EVAL_CASE
    flat, X, labels, coef = R.eval_data(case)
    table = R.std_table(case.hidden[0])
    torch.manual_seed(case.torch_seed)
    res, info = R.robustness(flat, case.dims, X, labels, list(case.levels), case.eval_seed, table, coef)
    after = torch.rand(1).item()
    torch.manual_seed(case.torch_seed)
    for _ in range(case.n * len(case.levels)):
        torch.rand(1)
    assert torch.rand(1).item() == after
    print(f"\n[admissible] evaluator: {info}  {res}", end="")
    assert info["min_util_gap"] > 2 * R.BOUND and info["min_logit_gap"] >= R.LOGIT_GAP
    for level in case.levels:
        k = res[f"accuracy_gaming_{level}"] * case.n
        assert abs(k - round(k)) < 1e-5 and 0 < round(k) < case.n
    torch.manual_seed(case.torch_seed)
    res32, _ = R.robustness(flat, case.dims, X, labels, list(case.levels), case.eval_seed, table, coef, dtype=torch.float32)
    assert res32 == res
