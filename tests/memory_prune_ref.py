"""Shared by tests/test_memory_prune_ref_cpu.py and tests/test_memory_prune_gpu.py: `ac_memory_add_prune`'s documented
arithmetic for ONE job (include/acamd.h, csrc/memory_ops.hip) restated in numpy, and the cases both modules walk.
Nothing here imports the product package.

  for t in 0 .. n_new-1:  row n_old+t joins: sum += float64(row)                       (running fp64 sum, per element)
      count <= cap:       dropped[t] = -1
      else:               mean = float32(sum / count)                                   (rounded to fp32 once per step)
                          dist[i] = sqrt(sum_d float64(row[i,d] - mean[d])**2)           (fp32 differences, fp64 squares)
                          drop the arg-max over the live rows; on an exactly equal distance the LARGER row index
                          (csrc/memory_ops.hip: "ties: the later row, as a stable ascending sort would drop")
                          sum -= float64(dropped row)
  out: dropped [n_new], alive [n], dist [n] (survivors: distance at the last prune; 0 when nothing was pruned), sum [D]

`run()` makes its own decisions.  `replay()` follows the device's `dropped[]`, so that one legitimately ambiguous decision
cannot cascade, and checks every step:
  * the device's choice is within DIST_RTOL = 2e-12 relative of the reference's arg-max distance.  The two differ only in
    the order of the fp64 additions: over D <= 4096 terms that is at most D * 2^-53 < 5e-13 relative on the sum of squares,
    half of it after the square root (the device's sqrt adds an ulp);
  * when that distance is exactly equal to another live row's, the dropped row is the larger index.
It returns the steps where the device's choice is not the reference's own arg-max ("excused" steps).  On the random cases
below there must be none: their seeds are chosen so that the reference's top two distances differ by more than 1e-9
relative at every step (tests/test_memory_prune_ref_cpu.py checks it); the minimum over all of them is

    MIN_TOP_TWO_GAP = 1.7e-09 (case n2_D128: with cap = 1 the two live rows are equidistant from their mean but for its rounding
                               to fp32; the smallest gap of a case with cap > 1 is 2.3e-05, multi_n1025_cap1000)

On the duplicate-row cases an exact tie is only ever between byte-identical rows.
At the end: alive[] exact, dist[] of the survivors to 1e-12 relative, sum bit-equal (per element it is the same sequence of
fp64 additions and subtractions on both sides).
"""
from dataclasses import dataclass

import numpy as np

DIST_RTOL = 2e-12
SURVIVOR_RTOL = 1e-12
MIN_GAP_REQUIRED = 1e-9


@dataclass
class Result:
    dropped: np.ndarray          # int32 [n_new]
    alive: np.ndarray            # uint8 [n]
    dist: np.ndarray             # float64 [n]
    sum: np.ndarray              # float64 [D]
    gaps: list                   # per prune step: (d1 - d2) / d1 of the two largest live distances (1.0 with one live row)


def _distances(rows, mean32, idx, chunk=1024):
    out = np.empty(len(idx), dtype=np.float64)
    for s in range(0, len(idx), chunk):
        diff = (rows[idx[s:s + chunk]] - mean32).astype(np.float64)          # fp32 subtraction, then widened
        out[s:s + chunk] = np.sqrt(np.einsum("nd,nd->n", diff, diff))
    return out


def _walk(rows, n_old, n_new, cap, sum0, choose):
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    n = n_old + n_new
    assert rows.shape[0] == n and 0 <= n_old <= cap and n_new >= 1 and cap >= 1
    total = np.array(sum0, dtype=np.float64, copy=True)
    alive = np.zeros(n, dtype=bool)
    alive[:n_old] = True
    dist = np.zeros(n, dtype=np.float64)
    dropped = np.full(n_new, -1, dtype=np.int32)
    gaps = []
    count = n_old
    for t in range(n_new):
        r = n_old + t
        total += rows[r].astype(np.float64)
        alive[r] = True
        count += 1
        if count <= cap:
            choose(t, None, None, None)
            continue
        mean32 = (total / count).astype(np.float32)
        idx = np.nonzero(alive)[0]
        d = _distances(rows, mean32, idx)
        dist[idx] = d
        dmax = d.max()
        best = int(idx[d == dmax].max())                                     # exactly equal distance: the larger row index
        top2 = np.partition(d, -2)[-2:] if len(d) > 1 else None
        gaps.append(1.0 if top2 is None else (float((top2[1] - top2[0]) / top2[1]) if top2[1] > 0 else 0.0))
        j = choose(t, best, idx, d)
        dropped[t] = j
        alive[j] = False
        total -= rows[j].astype(np.float64)
        count -= 1
    return Result(dropped, alive.astype(np.uint8), dist, total, gaps)


def run(rows, n_old, n_new, cap, sum0):
    """The reference's own decisions."""
    return _walk(rows, n_old, n_new, cap, sum0, lambda t, best, idx, d: best)


def replay(rows, n_old, n_new, cap, sum0, dropped, alive, dist, total):
    """Follow the device's dropped[] and check it step by step, then alive[] / dist[] / sum.  Raises AssertionError;
    returns the excused steps [(t, device's row, reference's row)]."""
    dropped = np.asarray(dropped)
    n = n_old + n_new
    excused = []

    def choose(t, best, idx, d):
        j = int(dropped[t])
        if best is None:
            assert j == -1, f"step {t}: at or under the cap, yet dropped[{t}] = {j}"
            return None
        assert 0 <= j < n and j in idx, f"step {t}: dropped[{t}] = {j} is not a live row"
        dj, dmax = float(d[idx == j][0]), float(d.max())
        assert dmax - dj <= DIST_RTOL * dmax, (f"step {t}: row {j} dropped at distance {dj!r}, the farthest live row {best} is at {dmax!r} "
                                                f"(relative gap {(dmax - dj) / dmax:.3e})")
        ties = idx[d == dj]
        assert j == int(ties.max()), f"step {t}: rows {ties.tolist()} are at exactly the same distance, the LARGER index goes, yet {j} was dropped"
        if j != best:
            excused.append((t, j, best))
        return j

    ref = _walk(rows, n_old, n_new, cap, sum0, choose)
    alive = np.asarray(alive).astype(np.uint8)
    assert np.array_equal(alive, ref.alive), f"alive[] differs at rows {np.nonzero(alive != ref.alive)[0].tolist()}"
    keep = ref.alive.astype(bool)
    got, want = np.asarray(dist, dtype=np.float64)[keep], ref.dist[keep]
    bad = np.abs(got - want) > SURVIVOR_RTOL * want
    assert not bad.any(), f"dist[] of survivors {np.nonzero(keep)[0][bad].tolist()}: {got[bad].tolist()} vs {want[bad].tolist()}"
    total = np.ascontiguousarray(total, dtype=np.float64)
    same = total.view(np.uint64) == ref.sum.view(np.uint64)
    assert same.all(), f"sum differs in elements {np.nonzero(~same)[0].tolist()[:8]} (bit-equal expected)"
    return excused


# ---- the cases -------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    name: str
    D: int
    n_old: int
    n_new: int
    cap: int
    seed: int
    ld: int = 0                  # 0 = tight (D)
    offset: int = 0              # floats in front of row 0 (1: the base is not 16-byte aligned)
    dup: bool = False

    @property
    def n(self):
        return self.n_old + self.n_new

    @property
    def stride(self):
        return self.ld or self.D


def make_rows(c):
    """[n, D] fp32: unit rows around a centroid with noise 0.5 (D = 1: not normalised -- unit rows of one element are all +-1).
    dup: stored and incoming rows hold exact copies, two of them of the row that is farthest when they arrive."""
    rng = np.random.default_rng(c.seed)
    cent = rng.standard_normal(c.D)
    X = cent + 0.5 * rng.standard_normal((c.n, c.D))
    if c.D > 1:
        X /= np.linalg.norm(X, axis=1, keepdims=True)
    X = X.astype(np.float32)
    if c.dup:
        assert c.n_old >= 7 and c.n_new >= 8
        o = c.n_old
        far = -cent + 0.1 * rng.standard_normal(c.D)
        X[6] = (far / np.linalg.norm(far)).astype(np.float32)               # the stored outlier: farthest at the first prune
        X[5] = X[2]                                                          # a stored pair
        X[o] = X[6]                                                          # incoming copies of the farthest row ...
        X[o + 1] = X[6]
        X[o + 2] = X[2]                                                      # ... of a stored pair (now three of a kind) ...
        X[o + 4] = X[o + 3]                                                  # ... and of each other
        X[o + 7] = X[0]
    return X


def sum_of_old(rows, n_old):
    return rows[:n_old].astype(np.float64).sum(axis=0)


def _grid():
    cs = []
    for D in (1, 3, 5, 66, 64, 768, 4096):                                   # tight ld, aligned; 1 / 3 / 5 / 66: the scalar path
        cs.append(Case(f"D{D}", D, 20, 12, 20, 1000 + D))
    cs.append(Case("D64_ld68_vector", 64, 20, 12, 20, 1101, ld=68))
    cs.append(Case("D64_ld67_scalar", 64, 20, 12, 20, 1102, ld=67))
    cs.append(Case("D64_base_plus_one_float_scalar", 64, 20, 12, 20, 1103, offset=1))
    for n in (2, 15, 16, 17, 31, 32, 33, 1025):                              # the two-rows-per-wave loop on either side of 16 and 32 waves
        k = min(4, n - 1)
        cs.append(Case(f"n{n}_D128", 128, n - k, k, n - k, 1200 + n))
        cs.append(Case(f"n{n}_D66", 66, n - k, k, n - k, 1300 + n))
    cs.append(Case("n_old0_cap3", 128, 0, 9, 3, 1401))                       # the first three steps report -1
    # cap = 1: the two live rows of every step are equidistant from their mean but for its rounding to fp32, so the gaps are
    # ~1e-8 by construction; these two seeds are the first (searched from 2000 up) whose 40 steps all stay above 3e-9
    cs.append(Case("cap1", 128, 1, 40, 1, 2573))
    cs.append(Case("cap1_from_empty", 64, 0, 40, 1, 2096))
    cs.append(Case("crossing_the_cap", 128, 10, 20, 17, 1404))               # n_old < cap: seven steps without a prune first
    cs.append(Case("never_over_the_cap", 128, 5, 6, 11, 1405))
    cs.append(Case("n8192_D64", 64, 8189, 3, 8189, 1501))
    cs.append(Case("n8192_D4096", 4096, 8189, 3, 8189, 1502))
    return cs


CASES = _grid()
# one launch, five jobs of different sizes (LDS is sized for the largest and laid out per job)
MULTI_JOB_D = 128
MULTI_JOB_CASES = [Case(f"multi_n{n}_cap{cap}", MULTI_JOB_D, cap, n - cap, cap, 1600 + n)
                   for n, cap in ((3, 1), (1025, 1000), (33, 32), (17, 5), (8192, 8190))]
DUP_CASES = [Case("dups_D128_cap8", 128, 8, 10, 8, 1701, dup=True), Case("dups_D66_cap8_scalar", 66, 8, 10, 8, 1702, dup=True)]
# the three random cases the CPU suite runs through the product's per-example host logic
HOST_LOGIC_CASES = ("D64", "crossing_the_cap", "n33_D128")
