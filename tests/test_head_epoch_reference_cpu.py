"""CPU suite: pins tests/head_epoch_ref.py -- the plain-torch epoch that tests/test_head_epoch_reference_gpu.py holds the HIP
head-training kernels against -- and produces the figures that module's bounds are built from.

1. The helper's epoch (order, short last batch, EWC weight lambda_B / rows, dropout seeds seed0 + i) equals a hand-unrolled loop
   of `oracle/head_oracle.py` `train_step` / `train_step_loss` calls, bit for bit.
2. For EVERY case of the grid the fp32 instance of the helper is compared with the fp64 one and the deviations per quantity are
   printed (`pytest -s`):
     regime "default" (eps = 1e-8, <= 4 steps): the fp32 instance itself sits inside the bars the device is held to
       (head_epoch_ref.DEFAULT_BOUNDS) -- a case where plain fp32 does not is ill-conditioned and may not be in the grid;
     regime "conditioned" (eps = 1e-4): every 40-step case stays within head_epoch_ref.FP32_DEV_40 (so those constants ARE the
       grid's worst 40-step figures), and every conditioned case of s steps stays within ADMISSION x FP32_DEV_40 both at s and
       at 2 s steps (the same epochs run twice): the reference is well-conditioned with room to spare, or the case fails here
       before it can mislead on the GPU;
     both regimes: the fp64 trajectory keeps head_epoch_ref.KINK_MIN_UNITS fp32 rounding units from every ReLU kink (below that
       the sign of a pre-activation, so a whole row's gradient through that unit, is not determined in fp32 at all).
"""
import numpy as np
import pytest
import torch

import head_epoch_ref as R
from oracle import head_oracle


def _flat0(case):
    return R.make_head_module(case).flat_params().detach().clone()


def test_dropout_port_keep_rate_and_determinism():
    a = R.dropout_keep_np(1, 512, 768, 0.1)
    assert abs(a.mean() - 0.9) < 0.005 and np.array_equal(a, R.dropout_keep_np(1, 512, 768, 0.1))
    assert not np.array_equal(a, R.dropout_keep_np(1 ^ R.SEED_XOR, 512, 768, 0.1))
    assert np.array_equal(a[:7], R.dropout_keep_np(1, 7, 768, 0.1))           # the counter is row * N + col


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_epoch_equals_hand_unrolled_oracle_steps(dtype):
    """order with a repeated row, batches of 8 + 8 + 7, EWC, dropout: two epochs of the helper == 6 head_oracle.train_step calls."""
    D, C, hidden, n, B, p = 64, 3, (32, 16), 23, 8, 0.1
    g = torch.Generator().manual_seed(5)
    X = torch.nn.functional.normalize(torch.randn(40, D, generator=g), dim=1)
    y = torch.randint(0, C, (40,), generator=g)
    order = torch.randperm(40, generator=g)[:n]
    order[5] = order[2]
    flat0 = head_oracle.flat(head_oracle.make_head(D, C, list(hidden))).clone()
    fisher = torch.rand(flat0.numel(), generator=g)
    old = flat0 + 0.01 * torch.randn(flat0.numel(), generator=g)
    ref = R.RefTrainer(D, C, hidden, flat0, dtype)
    for ep in range(2):
        assert ref.epoch(X, y, None, order, B, p, 900 + 10 * ep, fisher, old, 5.0, "ce") == 3
    # by hand
    seq = head_oracle.make_head(D, C, list(hidden)).to(dtype).train()
    opt = torch.optim.AdamW(seq.parameters(), lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
    Xd, Fd, Od = X.to(dtype), fisher.to(dtype), old.to(dtype)
    p32 = float(np.float32(p))
    total = torch.zeros((), dtype=dtype)
    last = None
    for seed, rows in ((900, order[0:8]), (901, order[8:16]), (902, order[16:23]), (910, order[0:8]), (911, order[8:16]), (912, order[16:23])):
        nb = len(rows)
        masks = [torch.from_numpy(R.dropout_keep_np(seed, nb, 32, p)), torch.from_numpy(R.dropout_keep_np(seed ^ 0xA5A5A5A5A5A5A5A5, nb, 16, p))]
        last = head_oracle.train_step(seq, opt, Xd[rows], y[rows], masks=masks, p=p32, fisher_flat=Fd, old_flat=Od, lam_over_B=5.0 / nb)
        total += torch.tensor(last[0], dtype=dtype) + torch.tensor(last[1], dtype=dtype)
    assert ref.t == 6
    assert torch.equal(ref.flat, head_oracle.flat(seq))
    st = opt.state_dict()["state"]
    assert torch.equal(ref.m, torch.cat([st[i]["exp_avg"].reshape(-1) for i in range(6)]))
    assert torch.equal(ref.v, torch.cat([st[i]["exp_avg_sq"].reshape(-1) for i in range(6)]))
    assert [float(v) for v in ref.out3] == list(last)
    assert abs(float(ref.loss_accum) - float(total)) <= 1e-6 * abs(float(total))     # (floats of the step losses summed vs tensors)
    assert ref.grads.shape == flat0.shape and float(ref.grads.norm()) > 0


@pytest.mark.parametrize("kind", ["bce", "ce_sigmoid"])
def test_sigmoid_loss_steps_equal_the_oracle(kind):
    D, C, hidden, n, B = 64, 5, (32, 16), 19, 8
    g = torch.Generator().manual_seed(6)
    X = torch.nn.functional.normalize(torch.randn(n, D, generator=g), dim=1).double()
    y = torch.randint(0, C, (n,), generator=g)
    T = (torch.rand(n, C, generator=g) < 0.3).double()
    seq = head_oracle.make_multilabel_head(D, C, list(hidden), seed=3).double().train()
    flat0 = head_oracle.flat(seq).clone()
    opt = torch.optim.AdamW(seq.parameters(), lr=1e-3, weight_decay=0.01)
    ref = R.RefTrainer(D, C, hidden, flat0, torch.float64)
    ref.epoch(X, None if kind == "bce" else y, T if kind == "bce" else None, None, B, 0.0, 0, loss=kind)
    for off in (0, 8, 16):
        loss, gn = head_oracle.train_step_loss(seq, opt, X[off:off + B], (T if kind == "bce" else y)[off:off + B], kind, masks=None)
    assert torch.equal(ref.flat, head_oracle.flat(seq))
    assert float(ref.out3[0]) == loss and float(ref.out3[2]) == gn and float(ref.out3[1]) == 0.0


def test_max_norm_zero_means_no_clip():
    D, C, hidden = 64, 3, (32, 16)
    g = torch.Generator().manual_seed(7)
    X = 6.0 * torch.nn.functional.normalize(torch.randn(8, D, generator=g), dim=1).double()
    y = torch.randint(0, C, (8,), generator=g)
    flat0 = head_oracle.flat(head_oracle.make_head(D, C, list(hidden))).clone()
    a = R.RefTrainer(D, C, hidden, flat0, max_norm=0.0)
    b = R.RefTrainer(D, C, hidden, flat0, max_norm=1e9)
    c = R.RefTrainer(D, C, hidden, flat0, max_norm=1.0)
    for t in (a, b, c):
        t.epoch(X, y, None, None, 8, 0.0, 0)
    assert a.grad_norms[0] > 1.0 and torch.equal(a.m, b.m) and torch.equal(a.flat, b.flat) and not torch.equal(a.m, c.m)


def _fmt(d):
    return "  ".join(f"{q} {d[q]:.1e}" for q in R.QUANTITIES)


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.id)
def test_fp32_instance_against_fp64(case):
    flat0 = _flat0(case)
    data = R.make_data(case, flat0)
    s = case.steps
    epochs = case.epochs * (2 if case.conditioned else 1)
    r64, s64 = R.run_ref(case, data, flat0, torch.float64, epochs, (s,))
    r32, s32 = R.run_ref(case, data, flat0, torch.float32, epochs, (s,))
    assert r64.t == r32.t == s * (2 if case.conditioned else 1)
    dev = R.deviation(s32[s], s64[s])
    print(f"\n[fp32 vs fp64] {case.id:24s} {s:3d} steps: {_fmt(dev)}")
    rk, _ = R.run_ref(case, data, flat0, torch.float64, track_kinks=True)          # (the case's own length)
    print(f"[fp64 kinks]   {case.id:24s} nearest {rk.kink_units:.3g} units at (step, layer, row, unit) = {rk.kink_at}")
    assert rk.kink_units >= R.KINK_MIN_UNITS, (case.id, rk.kink_units, rk.kink_at)
    gn = r64.grad_norms[:s]
    if case.clip == "active":
        assert min(gn) > 1.05 * case.max_norm, gn
    if case.clip == "inactive":
        assert max(gn) < 0.95 * case.max_norm, gn
    if not case.conditioned:
        for q in R.QUANTITIES:
            assert dev[q] <= R.DEFAULT_BOUNDS[q], (case.id, q, dev[q])
        return
    dev2 = R.deviation(R.state_of(r32), R.state_of(r64))
    print(f"[fp32 vs fp64] {case.id:24s} {2 * s:3d} steps: {_fmt(dev2)}")
    for q in R.QUANTITIES:
        if s == 40:
            assert dev[q] <= R.FP32_DEV_40[q], (case.id, q, dev[q])
        assert dev[q] <= R.ADMISSION * R.FP32_DEV_40[q], (case.id, "s", q, dev[q])
        assert dev2[q] <= R.ADMISSION * R.FP32_DEV_40[q], (case.id, "2s", q, dev2[q])


def test_the_grid_covers_what_it_claims():
    """Hand-derived selection against the rule restated: a typo in the table fails here, not as a puzzling launch count."""
    lds_budget = 160 * 1024
    for c in R.CASES:
        D, (H1, H2) = c.D, c.hidden
        r1, r2 = -(-H1 // 256), -(-H2 // 256)
        R1 = 3 if r1 <= 3 else 4
        lds = 4 * (3 * (R1 * D + 2 * H1 + R1 * H2 + 56) + 32 * (H2 + 4) + 16 * H2 + 6064) + 528
        shape_ok = (c.C <= 16 and r1 <= 4 and r2 <= 2 and D <= 1024 and H1 <= 1024 and H2 <= 384 and D % 4 == 0 and H1 % 4 == 0
                    and H2 % 4 == 0 and lds <= lds_budget and c.layout in ("dense", "ld+4"))
        assert c.persistent == (shape_ok and c.batch <= 32), c.id
    ids = {c.id for c in R.CASES}
    pers = [c for c in R.CASES if c.persistent]
    assert {(c.C <= 4, -(-c.hidden[0] // 256) <= 3) for c in pers} == {(True, True), (True, False), (False, True), (False, False)}
    for shape in (R.H768, R.HR4, R.HRAG, R.H128, R.H64):
        assert any(c.steps == 40 and c.conditioned and (c.D, c.hidden) == shape for c in R.CASES), shape
    assert any(c.conditioned and c.epochs == 3 and c.steps > 100 for c in R.CASES)
    assert {"limit-c16", "limit-c17", "limit-batch33", "limit-h2-388", "limit-d770", "x-ld+2", "x-ld+4", "x-off4", "n1", "batch1", "batch5"} <= ids
