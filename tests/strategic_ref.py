"""Shared by tests/test_strategic_ref_cpu.py and tests/test_strategic_reference_gpu.py (BOUND and the sure-row print also by
tests/test_strategic_gpu.py): strategic mode stated once in plain numpy / torch-CPU, in any float dtype (fp64 for the reference
proper, fp32 for the yardstick instance), and the case tables both modules walk.  No GPU, no native library.

  utilities        every candidate of a table (ANY table) as its own row through the head: fp32 candidate rows as the search
                   builds them, forward, softmax maximum minus relu(c_f dy)                    (csrc/strategic.hip)
  choose           the first maximum (the reference's strict `>` scan)
  masks_of         the seeded mode's masks: the numpy port of ac::dropout_keep (head_epoch_ref.dropout_keep_np) over rows * M
                   candidate rows, layer 2 under seed ^ 0xA5A5A5A5A5A5A5A5
  strategic_loss   CE_mean(rows < B) + lambda * sum over mispredicted rows B + i of their CE / B, by autograd
                                                                                               (strategic_loss_kernel, csrc/head.hip)
  StrategicRefTrainer   one training step = best responses under masks_of(seed) + the [x; y] forward under the 2B-row masks of
                   seed ^ 0x5DEECE66D + loss, clip at 1.0, AdamW with the arguments of `_strategic_training_step`
  robustness       StrategicEvaluator.evaluate_robustness with the head in train mode and replay=False

Admissibility (proven by tests/test_strategic_ref_cpu.py, on the fp64 reference alone -- conditions, not measurements):
  best-response cases   at most 5 % of a case's rows have a DECIDED gap <= 2 BOUND (`decided_gap`: the maximum minus the largest
                        utility that is not exactly the maximum; exact ties are decided by the first-maximum rule and occur only
                        where they are structural -- C = 1, no head, identity / duplicate table entries in eval mode);
  trajectory, evaluator no row at any step within 2 BOUND in utility, none within LOGIT_GAP in the top-2 logits of a row whose
                        argmax is used, no kept hidden unit within head_epoch_ref.KINK_MIN_UNITS of a ReLU kink;
  loss cases            top-2 logit gap of rows B .. 2B at least LOGIT_GAP.
Seeds 0 .. 5 were tried per case in that order and the first admissible one is in the table; the rejected ones are named there.
"""
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F

import head_epoch_ref as E
from head_epoch_ref import SEED_XOR, dropout_keep_np
from oracle import head_oracle

BOUND = 2e-5                  # |utility - fp64 utility|: the project's bar (fp32 GEMM sums at D = 768; csrc/strategic.hip)
LOGIT_GAP = 1e-3              # an argmax that is used must be decided by at least this much in fp64
SURE_SHARE_MIN = 0.95         # a best-response case decides at least this share of its rows
LOSS_SEED_XOR = 0x5DEECE66D   # StrategicOptimizer.strategic_loss: the [x; y] forward runs under seed ^ this
MASK64 = 0xFFFFFFFFFFFFFFFF
DROPOUT_P = 0.1


# ---- heads ------------------------------------------------------------------------------------------------------------------
def _shapes(dims):
    D, H1, H2, C = dims
    return [(H1, D), (H1,), (H2, H1), (H2,), (C, H2), (C,)]


def split(flat, dims):
    """The six parameter views W1, b1, W2, b2, W3, b3 of a flat block (layout of include/acamd.h)."""
    out, off = [], 0
    for s in _shapes(dims):
        n = int(np.prod(s))
        out.append(flat[off:off + n].view(s))
        off += n
    assert off == flat.numel()
    return out


def sharp_head(D, H1, H2, C, seed, s2=2.0, s3=32.0):
    """Flat fp32 parameter block: the `_head` initialisation of tests/test_strategic_gpu.py (every tensor uniform in
    +-1/sqrt(last dimension), drawn in parameter order from Generator(seed)) with W2 x s2 and W3 x s3.  The scaling makes the
    softmax decide: with s2 = s3 = 1 its maximum is about 1/C for every candidate and the utilities are near-tied."""
    g = torch.Generator().manual_seed(seed)
    parts = []
    for i, s in enumerate(_shapes((D, H1, H2, C))):
        t = (torch.rand(s, generator=g) - 0.5) * (2.0 / s[-1] ** 0.5)
        if i == 2:
            t = t * s2
        if i == 4:
            t = t * s3
        parts.append(t.reshape(-1))
    return torch.cat(parts).float().contiguous()


# ---- tables and masks ---------------------------------------------------------------------------------------------------------
def std_table(D, M=50):
    """(features, deltas fp32) of the product's table, restated: x itself, then (i, delta) for i = 0, 1, ... and the ten values
    of torch.linspace(-2, 2, 10) (none is 0), cut at M."""
    feats, vals = [-1], [0.0]
    for i in range(D):
        for d in torch.linspace(-2.0, 2.0, 10):
            if d != 0 and len(feats) < M:
                feats.append(i)
                vals.append(float(d))
    assert len(feats) == M
    return feats[:M], torch.tensor(vals[:M], dtype=torch.float32)


def special_table(D):
    """Eight entries: identity entries (feature -1, D, D + 7, their deltas must be ignored) among real moves, two entries moving
    the same feature, and entry 6 an exact duplicate of entry 0."""
    return [3, -1, D, 5, 5, D + 7, 3, 9], torch.tensor([0.5, 0.0, 1.0, -1.0, 0.75, -2.0, 0.5, 1.5], dtype=torch.float32)


def layer_masks(key, rows, H1, H2, p):
    """Keep masks (numpy bool [rows, H1], [rows, H2]) of one seeded forward over `rows` rows under the 64-bit key `key`."""
    key &= MASK64
    return dropout_keep_np(key, rows, H1, p), dropout_keep_np(key ^ SEED_XOR, rows, H2, p)


def masks_of(seed, rows, M, H1, H2, p):
    """The seeded search's masks: candidate m of query q is row q * M + m of both layers."""
    m1, m2 = layer_masks(seed, rows * M, H1, H2, p)
    return m1.reshape(rows, M, H1), m2.reshape(rows, M, H2)


def loss_masks_of(seed, B, H1, H2, p):
    """The masks of the [x; y] forward of `StrategicOptimizer.strategic_loss(..., seed=seed)` (2B rows)."""
    return layer_masks((seed & MASK64) ^ LOSS_SEED_XOR, 2 * B, H1, H2, p)


# ---- forward, utilities, choice -------------------------------------------------------------------------------------------------
def _p32(p):
    return float(np.float32(p))          # the device divides by 1 - (float)p


def _t(m, dtype):
    return (torch.from_numpy(m) if isinstance(m, np.ndarray) else m).to(dtype)


def forward(P, x, masks, p):
    """Logits of the rows x [..., D] under the parameter views P; masks = (m1 [..., H1], m2 [..., H2]) or None (eval mode)."""
    dt = x.dtype
    a = torch.relu(x @ P[0].T + P[1])
    if masks is not None:
        a = a * _t(masks[0], dt) / (1.0 - _p32(p))
    a = torch.relu(a @ P[2].T + P[3])
    if masks is not None:
        a = a * _t(masks[1], dt) / (1.0 - _p32(p))
    return a @ P[4].T + P[5]


def utilities(flat, dims, X, feat, delta, coef, masks=None, p=DROPOUT_P, dtype=torch.float64):
    """(u [b, M], logits [b, M, C] | None, Y fp32 [b, M, D]) of the rows X [b, D] (fp32) against the table (feat, delta): entry m
    moves coordinate feat[m] by delta[m] in fp32; feat[m] < 0 or >= D is the identity move with cost 0.
    cost = relu(c_f dy), dy = fl32(fl32(x_f + delta) - x_f); u = max softmax(head(y)) - cost, or 1/C - cost with flat = None.
    In eval mode (masks None) equal moves are ONE row of the forward, so that their utilities are equal exactly, as they are
    by construction on the device."""
    D, H1, H2, C = dims
    X = X.float()
    b, M = X.shape[0], len(feat)
    feat = [int(f) for f in feat]
    delta = torch.as_tensor(delta, dtype=torch.float32)
    Y = X.unsqueeze(1).repeat(1, M, 1)
    dy = torch.zeros(b, M, dtype=torch.float32)
    cf = torch.zeros(M, dtype=dtype)
    for m, f in enumerate(feat):
        if 0 <= f < D:
            Y[:, m, f] = X[:, f] + delta[m]
            dy[:, m] = Y[:, m, f] - X[:, f]
            cf[m] = coef[f].to(dtype)
    cost = torch.relu(cf[None, :] * dy.to(dtype))
    if flat is None:
        return 1.0 / C - cost, None, Y
    P = split(flat.to(dtype), dims)
    if masks is None:
        keys = [(f, float(delta[m])) if 0 <= f < D else (-1, 0.0) for m, f in enumerate(feat)]
        first = {}
        for m, k in enumerate(keys):
            first.setdefault(k, m)
        uniq = sorted(first.values())
        inv = [uniq.index(first[k]) for k in keys]
        z = forward(P, Y[:, uniq].to(dtype), None, p)[:, inv]
    else:
        z = forward(P, Y.to(dtype), masks, p)
    return torch.softmax(z, -1).max(-1).values - cost, z, Y


def choose(u):
    """First maximum of every row (numpy.argmax: the first occurrence)."""
    return torch.from_numpy(np.argmax(u.detach().numpy(), axis=1))


def top2_gap(u):
    """Per row: the difference of the two largest values (inf with one column)."""
    if u.shape[1] < 2:
        return torch.full((u.shape[0],), float("inf"), dtype=u.dtype)
    t = u.topk(2, dim=1).values
    return t[:, 0] - t[:, 1]


def decided_gap(u):
    """Per row: the maximum minus the largest value that is not exactly the maximum (inf if there is none)."""
    mx = u.max(1, keepdim=True).values
    rest = torch.where(u == mx, torch.full_like(u, -float("inf")), u).max(1).values
    return mx[:, 0] - rest


# ---- the strategic loss --------------------------------------------------------------------------------------------------------
def loss_of_logits(z, y, lam):
    """(loss, misprediction flags bool [B]) of the logits z [2B, C]: strategic_loss_kernel's docstring, torch.argmax for ties
    (first maximum, NaN maximal)."""
    B = z.shape[0] // 2
    reg = F.cross_entropy(z[:B], y)
    wrong = z[B:].argmax(1) != y
    strat = F.cross_entropy(z[B:], y, reduction="none")[wrong].sum() / B
    return reg + lam * strat, wrong


def strategic_loss(flat, dims, X2, y, lam, masks2, p=DROPOUT_P, dtype=torch.float64):
    """(loss float, flat gradient, misprediction flags bool [B], logits [2B, C]) of the rows X2 = [x; y] under the 2B-row masks
    masks2 (None: no dropout)."""
    leaf = flat.to(dtype).clone().requires_grad_(True)
    z = forward(split(leaf, dims), X2.to(dtype), masks2, p)
    loss, wrong = loss_of_logits(z, y, lam)
    loss.backward()
    return float(loss.detach()), leaf.grad.detach(), wrong, z.detach()


# ---- one training step, a trajectory ---------------------------------------------------------------------------------------------
class StrategicRefTrainer(E.RefTrainer):
    """head_epoch_ref.RefTrainer with the strategic step; AdamW as `_strategic_training_step` builds its HeadTrainer
    (lr = learning_rate / 2 = 5e-4, betas (0.9, 0.999), eps 1e-8, weight decay 0.01, clip at 1.0)."""

    def __init__(self, dims, flat0, dtype=torch.float64):
        D, H1, H2, C = dims
        super().__init__(D, C, (H1, H2), flat0, dtype, lr=5e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, max_norm=1.0)
        self.dims = tuple(dims)
        self.min_util_gap = float("inf")      # over every step so far
        self.min_logit_gap = float("inf")     # rows B .. 2B
        self.steps = []                       # per step: dict(loss, choice, mispred)

    def strategic_step(self, X, y, table, coef, lam, seed, p=DROPOUT_P):
        D, H1, H2, C = self.dims
        feat, delta = table
        B, M = X.shape[0], len(feat)
        u, _, Y = utilities(self.flat, self.dims, X, feat, delta, coef, masks_of(seed, B, M, H1, H2, p), p, self.dtype)
        ch = choose(u)
        X2 = torch.cat([X.float(), Y[torch.arange(B), ch]]).to(self.dtype)
        masks2 = [torch.from_numpy(m) for m in loss_masks_of(seed, B, H1, H2, p)]
        if self.track_kinks:
            self._kink_units(X2, masks2, _p32(p))
        self.opt.zero_grad()
        z = head_oracle.forward_masked(self.seq, X2, masks2, _p32(p))
        loss, wrong = loss_of_logits(z, y, lam)
        loss.backward()
        self.grads = torch.cat([q.grad.reshape(-1) for q in self.params]).clone()
        gn = torch.nn.utils.clip_grad_norm_(self.params, max_norm=self.max_norm)
        self.opt.step()
        self.t += 1
        self.grad_norms.append(float(gn))
        self.min_util_gap = min(self.min_util_gap, float(top2_gap(u.double()).min()))
        self.min_logit_gap = min(self.min_logit_gap, float(top2_gap(z[B:].detach().double()).min()))
        self.steps.append({"loss": float(loss.detach()), "choice": ch.tolist(), "mispred": wrong.tolist()})
        return self.steps[-1]


TRAJ_QUANTITIES = ("loss", "params", "m", "v", "grads")


def traj_state(tr):
    """params, m, v and the last step's raw gradients of a StrategicRefTrainer or a HeadTrainer, fp64 on the host."""
    f = lambda t: t.detach().double().cpu().reshape(-1).clone()
    return {"params": f(tr.flat), "m": f(tr.m), "v": f(tr.v), "grads": f(tr.grads)}


def traj_deviation(got_losses, got_state, ref):
    """Max abs deviation per quantity of TRAJ_QUANTITIES from the reference trainer `ref` (loss: over the steps, relative to
    max(1, |reference|) as head_epoch_ref.deviation has it)."""
    want = traj_state(ref)
    out = {"loss": max(abs(a - s["loss"]) / max(1.0, abs(s["loss"])) for a, s in zip(got_losses, ref.steps))}
    for q in TRAJ_QUANTITIES[1:]:
        out[q] = float((got_state[q] - want[q]).abs().max())
    return out


# ---- robustness ------------------------------------------------------------------------------------------------------------------
def robustness(flat, dims, X, labels, levels, seed, table, coef, p=DROPOUT_P, dtype=torch.float64):
    """StrategicEvaluator.evaluate_robustness(head in train mode, replay=False, seed=seed): per level, one torch.rand(1) per row
    on the global CPU generator; the rows below the level move to their best response under masks_of(seed * 1000003 + li); the
    accuracy is that of the argmax of the one-candidate (identity) forward of all rows under the masks of
    seed * 1000003 + li + 7919.  Returns (the result dictionary, dict(min_util_gap, min_logit_gap))."""
    D, H1, H2, C = dims
    feat, delta = table
    n = X.shape[0]
    results, info = {}, {"min_util_gap": float("inf"), "min_logit_gap": float("inf")}
    for li, level in enumerate(levels):
        chosen = [i for i in range(n) if torch.rand(1).item() < level]
        Xs = X.float().clone()
        if chosen:
            key = seed * 1000003 + li
            u, _, Y = utilities(flat, dims, Xs[chosen], feat, delta, coef, masks_of(key, len(chosen), len(feat), H1, H2, p), p, dtype)
            Xs[chosen] = Y[torch.arange(len(chosen)), choose(u)]
            info["min_util_gap"] = min(info["min_util_gap"], float(top2_gap(u.double()).min()))
        _, z, _ = utilities(flat, dims, Xs, [-1], [0.0], coef, masks_of(seed * 1000003 + li + 7919, n, 1, H1, H2, p), p, dtype)
        z = z[:, 0]
        info["min_logit_gap"] = min(info["min_logit_gap"], float(top2_gap(z.double()).min()))
        results[f"accuracy_gaming_{level}"] = (torch.argmax(z, dim=-1) == labels).float().mean().item()
    results["robustness_score"] = results["accuracy_gaming_0.0"] - results["accuracy_gaming_1.0"]
    results["relative_robustness"] = results["accuracy_gaming_1.0"] / results["accuracy_gaming_0.0"]
    return results, info


# ---------------------------------------------------------------------------------------------------------------------------------
# The cases.  Seeds: the first of 0 .. 5 that is admissible (see the module docstring); "rejected" names the others tried.
# ---------------------------------------------------------------------------------------------------------------------------------
S64, S70, S768, SR4 = (64, 64, 32), (70, 36, 20), (768, 768, 384), (1024, 1024, 256)


@dataclass(frozen=True)
class BRCase:
    """One best-response case: b unit rows against a sharp head, run in modes NONE and SEED and for both cost types."""
    id: str
    hidden: Tuple[int, int, int]        # (D, H1, H2)
    C: int
    b: int
    M: int = 50
    table: str = "std"                  # std (the product's rule, cut at M) | special (special_table)
    head: bool = True
    seed: int = 0
    ties: bool = False                  # exact ties at the maximum are structural here (else the CPU suite proves there are none)

    @property
    def dims(self):
        return self.hidden + (self.C,) if self.head else (self.hidden[0], 1, 1, self.C)

    @property
    def drop_seed(self):                # bits above 2^32 (and bit 63) set
        return (0xD1B54A32D192ED03 ^ (self.seed * 7919 + self.b * 104729 + self.C)) & MASK64


BR_CASES = [
    BRCase("c1-all-ties", S64, 1, 5, ties=True),                 # every utility 1 - cost: choice 0 for every row
    BRCase("c64", S64, 64, 17),                                  # the lane-stride edge of the softmax loop, from both sides
    BRCase("c65", S64, 65, 17),
    BRCase("d70-c130", S70, 130, 17),                            # D % 4 != 0, H2 < 64, three class strides
    BRCase("c2048", S64, 2048, 3),                               # kMaxC: the whole lg array
    BRCase("m1", S64, 7, 9, M=1),                                # idle waves
    BRCase("m2", S64, 7, 9, M=2),
    BRCase("m3", S64, 7, 9, M=3),
    BRCase("m5", S64, 7, 9, M=5),
    BRCase("m64", S64, 7, 9, M=64),                              # AC_STRAT_MAX_CANDIDATES
    BRCase("special-table", S64, 7, 9, M=8, table="special", ties=True),
    BRCase("w768-c7", S768, 7, 257),                             # the product width; b * M = 12 850 GEMM rows
    BRCase("w768-c300", S768, 300, 257),
    BRCase("r4-c16", SR4, 16, 17),                               # the r1 = 4 head of head_epoch_ref
    BRCase("no-head", S64, 4, 3, M=64, head=False, ties=True),   # utility 1/C - cost; M at the limit
]
assert len({c.id for c in BR_CASES}) == len(BR_CASES)


@dataclass
class BRData:
    flat: Optional[torch.Tensor]
    X: torch.Tensor
    coef: torch.Tensor
    feat: list
    delta: torch.Tensor


def br_data(case):
    D, H1, H2 = case.hidden
    g = torch.Generator().manual_seed(100 + case.seed)
    X = F.normalize(torch.randn(case.b, D, generator=g), dim=1)
    coef = torch.randn(D, generator=g) * 0.05
    feat, delta = special_table(D) if case.table == "special" else std_table(D, case.M)
    assert len(feat) == case.M
    flat = sharp_head(D, H1, H2, case.C, seed=D + case.C) if case.head else None
    return BRData(flat, X, coef, feat, delta)


def br_masks(case, mode_seeded):
    D, H1, H2, C = case.dims
    return masks_of(case.drop_seed, case.b, case.M, H1, H2, DROPOUT_P) if (mode_seeded and case.head) else None


@dataclass(frozen=True)
class LossCase:
    """One strategic-loss case: 2B rows [x; y] against a sharp head, three label patterns + lambda = 0."""
    hidden: Tuple[int, int, int]
    B: int
    C: int
    seed: int = 0

    @property
    def id(self):
        return f"d{self.hidden[0]}-b{self.B}-c{self.C}"

    @property
    def dims(self):
        return self.hidden + (self.C,)

    @property
    def drop_seed(self):                # the C ABI's dropout_seed of the [x; y] forward
        return (0xB5AD4ECEDA1CE2A9 ^ (self.seed * 7919 + self.B * 104729 + self.C)) & MASK64


LOSS_CASES = [LossCase(S64, 1, 2), LossCase(S64, 9, 7), LossCase(S64, 32, 4), LossCase(S64, 32, 65), LossCase(S64, 70, 130),
              LossCase(S64, 130, 5), LossCase(S64, 16, 2048), LossCase(S768, 16, 4), LossCase(S768, 32, 65)]
LOSS_LAMBDA = 0.7
LOSS_PATTERNS = ("mixed", "none", "all")


def loss_data(case):
    """(flat, X2 fp32 [2B, D], masks2): unit rows x, and y = x with one coordinate moved, as a best response is."""
    D, H1, H2 = case.hidden
    B = case.B
    g = torch.Generator().manual_seed(200 + case.seed)
    X = F.normalize(torch.randn(B, D, generator=g), dim=1)
    Yr = X.clone()
    Yr[torch.arange(B), torch.arange(B) % D] += torch.linspace(-2.0, 2.0, 10)[torch.arange(B) % 10]
    flat = sharp_head(D, H1, H2, case.C, seed=D + case.C + case.B)
    return flat, torch.cat([X, Yr]).contiguous(), layer_masks(case.drop_seed, 2 * B, H1, H2, DROPOUT_P)


def loss_labels(pred, C, pattern):
    """Labels from the reference's own argmax of rows B .. 2B: `none` = pred (nothing mispredicted), `all` = pred + 1 mod C,
    `mixed` = the first B // 2 rows mispredicted."""
    B = pred.numel()
    wrong = {"none": torch.zeros(B, dtype=torch.bool), "all": torch.ones(B, dtype=torch.bool),
             "mixed": torch.arange(B) < B // 2}[pattern]
    return torch.where(wrong, (pred + 1) % C, pred)


@dataclass(frozen=True)
class TrajCase:
    """Four steps of the default (seeded) strategic training on batches of 16."""
    id: str
    hidden: Tuple[int, int, int]
    C: int
    lam: float
    cost: str = "separable"             # separable | linear (the same arithmetic in the search; the product's two classes)
    seed: int = 0
    steps: int = 4
    batch: int = 16

    @property
    def dims(self):
        return self.hidden + (self.C,)

    def step_seed(self, i):             # 63-bit keys with bits above 2^32 set, as `_strategic_seed` gives
        return (0x7A3D5EED00000000 + 1000003 * i + self.seed) & 0x7FFFFFFFFFFFFFFF


TRAJ_CASES = [
    TrajCase("w768-c4-lam0.1", S768, 4, 0.1),
    TrajCase("w768-c4-lam1", S768, 4, 1.0),
    TrajCase("w768-c4-lam0.1-linear", S768, 4, 0.1, cost="linear"),
    TrajCase("w768-c4-lam1-linear", S768, 4, 1.0, cost="linear"),
    TrajCase("d70-c7-lam0.1", S70, 7, 0.1),
    TrajCase("d70-c7-lam1", S70, 7, 1.0),
]


def traj_data(case):
    """(flat0, X [steps * batch, D], y, coef)."""
    D, H1, H2 = case.hidden
    g = torch.Generator().manual_seed(300 + case.seed)
    n = case.steps * case.batch
    X = F.normalize(torch.randn(n, D, generator=g), dim=1)
    y = torch.randint(0, case.C, (n,), generator=g)
    coef = torch.randn(D, generator=g) * 0.05
    return sharp_head(D, H1, H2, case.C, seed=D + case.C), X, y, coef


_TRAJ = {}


def run_traj(case, dtype=torch.float64, track_kinks=False):
    """The case's trajectory in `dtype` (a StrategicRefTrainer); the linear and separable forms of a case share one run."""
    key = (case.hidden, case.C, case.lam, case.seed, dtype, track_kinks)
    if key not in _TRAJ:
        flat0, X, y, coef = traj_data(case)
        tr = StrategicRefTrainer(case.dims, flat0, dtype)
        tr.track_kinks = track_kinks
        table = std_table(case.hidden[0])
        for i in range(case.steps):
            rows = slice(i * case.batch, (i + 1) * case.batch)
            tr.strategic_step(X[rows], y[rows], table, coef, case.lam, case.step_seed(i))
        _TRAJ[key] = tr
    return _TRAJ[key]


@dataclass(frozen=True)
class EvalCase:
    hidden: Tuple[int, int, int] = S64
    C: int = 5
    n: int = 40
    levels: Tuple[float, ...] = (0.0, 0.5, 1.0)
    seed: int = 0
    torch_seed: int = 1234

    @property
    def dims(self):
        return self.hidden + (self.C,)

    @property
    def eval_seed(self):                # evaluate_robustness(seed=...): keys seed * 1000003 + li stay below 2^63
        return 0x3F00000000 + self.seed


EVAL_CASE = EvalCase()


def eval_data(case):
    """(flat, X, labels, coef): labels are the head's eval-mode fp64 argmax, every fourth one moved to the next class."""
    D, H1, H2 = case.hidden
    g = torch.Generator().manual_seed(400 + case.seed)
    X = F.normalize(torch.randn(case.n, D, generator=g), dim=1)
    coef = torch.randn(D, generator=g) * 0.05
    flat = sharp_head(D, H1, H2, case.C, seed=D + case.C)
    pred = forward(split(flat.double(), case.dims), X.double(), None, DROPOUT_P).argmax(1)
    labels = torch.where(torch.arange(case.n) % 4 == 3, (pred + 1) % case.C, pred)
    return flat, X, labels, coef


# ---- tolerances -------------------------------------------------------------------------------------------------------------------
# Utility: BOUND.  Loss and gradient of one call: 1e-5 (tests/test_strategic_gpu.py).  Logits of the chosen row: LOGITS_BAR.
# Trajectory: head_epoch_ref.DEFAULT_BOUNDS where the fp32 torch-CPU instance of the case (StrategicRefTrainer in fp32, the same
# batches, masks and optimizer) sits at least 4 x inside the entry; else 16 x the instance's deviation (head_epoch_ref's
# KERNEL_FACTOR: another summation order).  tests/test_strategic_ref_cpu.py measures the instance and asserts it stays below the
# figure written here (the measurement rounded up); `traj_bounds` applies the rule.  Nothing here comes from a GPU run.
LOSS_BAR = 1e-5
GRAD_BAR = 1e-5
LOGITS_BAR = 1e-4
TRAJ_DEFAULT = {"loss": E.DEFAULT_BOUNDS["loss_accum"], "params": E.DEFAULT_BOUNDS["params"], "m": E.DEFAULT_BOUNDS["m"],
                "v": E.DEFAULT_BOUNDS["v"], "grads": E.DEFAULT_BOUNDS["grads"]}
#
#   fp32 torch-CPU instance against fp64, 4 steps (measured / figure held here; 4 x the figure <= the DEFAULT_BOUNDS entry in
#   every cell, so every trajectory bar is the default one):
#     case                   loss              params            m                 v                  grads
#     768 / C 4, lam 0.1     7.2e-8 / 2e-7     5.5e-6 / 8e-6     6.4e-8 / 1e-7     3.1e-10 / 6e-10    4.0e-7 / 8e-7
#     768 / C 4, lam 1.0     1.2e-7 / 2e-7     3.1e-6 / 8e-6     1.1e-7 / 2e-7     4.2e-10 / 6e-10    7.9e-7 / 1.5e-6
#     70 / C 7, lam 0.1      1.1e-7 / 2e-7     1.1e-6 / 2e-6     1.3e-8 / 3e-8     6.0e-11 / 1e-10    3.4e-7 / 7e-7
#     70 / C 7, lam 1.0      1.8e-7 / 3e-7     1.6e-6 / 3e-6     1.2e-8 / 3e-8     5.0e-11 / 1e-10    8.7e-7 / 1.5e-6
#     DEFAULT_BOUNDS         1e-4              5e-5              1e-6              1e-8               1e-5
#   (the figures leave room for another BLAS blocking of the same fp32 sums).  The clip is active at every step (reference
#   gradient norms 5.8 .. 17.9), the regime DEFAULT_BOUNDS had not been measured in.
#   Seeds: seed 0 is admissible for every best-response, loss, trajectory and evaluator case; none was rejected.
#   Logits at C = 2048 with W3 x 32: the fp32 instance deviates from fp64 by 2.7e-6, 37 x inside LOGITS_BAR, which stays; its
#   utilities deviate by at most 6.7e-7 over the best-response cases, 30 x inside BOUND.
TRAJ_FP32_DEV = {
    (S768, 4, 0.1): {"loss": 2e-7, "params": 8e-6, "m": 1e-7, "v": 6e-10, "grads": 8e-7},
    (S768, 4, 1.0): {"loss": 2e-7, "params": 8e-6, "m": 2e-7, "v": 6e-10, "grads": 1.5e-6},
    (S70, 7, 0.1): {"loss": 2e-7, "params": 2e-6, "m": 3e-8, "v": 1e-10, "grads": 7e-7},
    (S70, 7, 1.0): {"loss": 3e-7, "params": 3e-6, "m": 3e-8, "v": 1e-10, "grads": 1.5e-6},
}


def four_times_inside(dev, bar):
    """The rule under which a project bar stays: the fp32 instance sits at least ADMISSION = 4 x inside it."""
    return E.ADMISSION * dev <= bar


def traj_bounds(case):
    """{quantity: (bar, rule)} of a trajectory case."""
    out = {}
    for q in TRAJ_QUANTITIES:
        dev, default = TRAJ_FP32_DEV[(case.hidden, case.C, case.lam)][q], TRAJ_DEFAULT[q]
        out[q] = (default, "default") if four_times_inside(dev, default) else (E.KERNEL_FACTOR * dev, "16 x fp32")
    return out
