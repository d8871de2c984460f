"""CPU suite: tests/memory_prune_ref.py (the numpy statement of `ac_memory_add_prune` that tests/test_memory_prune_gpu.py holds
the kernel to) agrees with the product's own per-example host logic, its random cases are free of near-ties, its duplicate
cases tie only between identical rows, and its step-by-step checker rejects the mistakes it is there to catch."""
import numpy as np
import pytest
import torch

import memory_prune_ref as M


@pytest.fixture(scope="module")
def ran():
    """run() over every case, once."""
    out = {}
    for c in M.CASES + M.MULTI_JOB_CASES + M.DUP_CASES:
        rows = M.make_rows(c)
        out[c.name] = (c, rows, M.run(rows, c.n_old, c.n_new, c.cap, M.sum_of_old(rows, c.n_old)))
    return out


def test_random_cases_have_no_near_ties(ran):
    """The seeds of the random cases: top-two gap above 1e-9 relative at every prune step (the device may differ from the
    reference by 2e-12), so the device has to take the reference's own arg-max at every step.  Prints the minimum."""
    worst = (np.inf, None)
    for name, (c, rows, res) in ran.items():
        if c.dup:
            continue
        assert len(res.gaps) == max(0, c.n - max(c.cap, c.n_old)), name
        if res.gaps:
            worst = min(worst, (min(res.gaps), name))
            assert min(res.gaps) > M.MIN_GAP_REQUIRED, (name, min(res.gaps))
    print(f"MEASURED minimum top-two gap over the random prune cases: {worst[0]:.3e} ({worst[1]})")


def test_run_bookkeeping(ran):
    for name, (c, rows, res) in ran.items():
        over = res.dropped >= 0
        assert int(res.alive.sum()) == min(c.n, max(c.cap, c.n_old)) and int(over.sum()) == c.n - int(res.alive.sum()), name
        assert (res.dropped[: max(0, c.cap - c.n_old)] == -1).all() and over[max(0, c.cap - c.n_old):].all(), name
        assert len(set(res.dropped[over].tolist())) == int(over.sum()) and not res.alive[res.dropped[over]].any()
        keep = res.alive.astype(bool)
        assert np.allclose(res.sum, rows[keep].astype(np.float64).sum(0), rtol=0, atol=1e-9), name
        # its own result replays clean, with no excused step
        assert M.replay(rows, c.n_old, c.n_new, c.cap, M.sum_of_old(rows, c.n_old), res.dropped, res.alive, res.dist, res.sum) == []
    c, rows, res = ran["n_old0_cap3"]
    assert res.dropped[:3].tolist() == [-1, -1, -1] and (res.dropped[3:] >= 0).all()
    c, rows, res = ran["never_over_the_cap"]
    assert (res.dropped == -1).all() and res.alive.all() and (res.dist == 0).all()


def test_duplicate_cases_tie_only_between_identical_rows(ran):
    for c in M.DUP_CASES:
        _, rows, res = ran[c.name]
        o = c.n_old
        # step 0 and step 1: the incoming copy of the farthest stored row (6) ties with it and, being the later row, goes
        assert res.gaps[0] == 0.0 and res.gaps[1] == 0.0 and res.dropped[:2].tolist() == [o, o + 1]
        assert res.alive[6] == 0 and 6 in res.dropped.tolist()               # ... and the outlier itself goes once it ties with nobody
        # wherever the top two are exactly equal, the rows are byte-identical (replayed by hand: the tie set at every step)
        seen = []
        M._walk(rows, c.n_old, c.n_new, c.cap, M.sum_of_old(rows, c.n_old),
                lambda t, best, idx, d: (seen.append(idx[d == d.max()]) if best is not None else None, best)[1])
        for tie in seen:
            assert all(np.array_equal(rows[i], rows[tie[0]]) for i in tie)
        assert sum(len(t) > 1 for t in seen) >= 2
        assert all(g == 0.0 or g > M.MIN_GAP_REQUIRED for g in res.gaps), res.gaps      # and no near-tie besides


@pytest.mark.parametrize("name", M.HOST_LOGIC_CASES)
def test_run_agrees_with_the_per_example_host_logic(name, ran):
    """PrototypeMemory.add_example on CPU tensors (the statement of memory.py:41-83 / :196-217 that test_host_logic checks
    against the reference algorithm step by step) keeps the same rows, in the order run()'s survivor distances give."""
    from adaptive_classifier import Example, ModelConfig, PrototypeMemory
    c, rows, res = ran[name]
    # the host logic measures the distances in fp32: only cases whose gaps are far above fp32 resolution can be compared
    assert min(res.gaps) > 1e-5, min(res.gaps)
    m = PrototypeMemory(c.D, ModelConfig({"max_examples_per_class": c.cap, "prototype_update_frequency": 10 ** 9}))
    for i in range(c.n):
        m.add_example(Example(f"r{i}", "x", torch.from_numpy(rows[i].copy())), "x")
    kept = [int(e.text[1:]) for e in m.examples["x"]]
    assert sorted(kept) == np.nonzero(res.alive)[0].tolist()
    idx = np.nonzero(res.alive)[0]
    assert kept == idx[np.argsort(res.dist[idx], kind="stable")].tolist()    # ascending distance at the last prune
    assert np.allclose(m.prototypes["x"].numpy(), (res.sum / len(kept)).astype(np.float32), rtol=0, atol=1e-6)


def _device_like(c, rows):
    res = M.run(rows, c.n_old, c.n_new, c.cap, M.sum_of_old(rows, c.n_old))
    return res.dropped.copy(), res.alive.copy(), res.dist.copy(), res.sum.copy()


def _forced(c, rows, forced):
    """What a device that takes forced[t] at step t (and the reference's choice elsewhere) would report, with every other
    output consistent with that choice."""
    res = M._walk(rows, c.n_old, c.n_new, c.cap, M.sum_of_old(rows, c.n_old), lambda t, best, idx, d: forced.get(t, best) if best is not None else None)
    return res.dropped, res.alive, res.dist, res.sum


def test_replay_rejects_planted_mistakes(ran):
    c, rows, res = ran["crossing_the_cap"]
    s0 = M.sum_of_old(rows, c.n_old)
    good = _device_like(c, rows)
    assert M.replay(rows, c.n_old, c.n_new, c.cap, s0, *good) == []
    # (1) the second-farthest row dropped at the first prune, everything after it consistent with that choice
    t0 = c.cap - c.n_old
    seen = {}
    M._walk(rows, c.n_old, c.n_new, c.cap, s0, lambda t, best, idx, d: (seen.setdefault(t, idx[np.argsort(d)[-2]]) if best is not None else None, best)[1])
    second = int(seen[t0])
    with pytest.raises(AssertionError, match="farthest live row"):
        M.replay(rows, c.n_old, c.n_new, c.cap, s0, *_forced(c, rows, {t0: second}))
    # (2) a tie broken toward the smaller index
    d = M.DUP_CASES[0]
    drows = ran[d.name][1]
    with pytest.raises(AssertionError, match="LARGER index"):
        M.replay(drows, d.n_old, d.n_new, d.cap, M.sum_of_old(drows, d.n_old), *_forced(d, drows, {0: 6}))
    assert M.replay(drows, d.n_old, d.n_new, d.cap, M.sum_of_old(drows, d.n_old), *_device_like(d, drows)) == []
    # (3) sum off by one ulp in one element
    dropped, alive, dist, total = (a.copy() for a in good)
    total[c.D // 2] = np.nextafter(total[c.D // 2], np.inf)
    with pytest.raises(AssertionError, match="bit-equal"):
        M.replay(rows, c.n_old, c.n_new, c.cap, s0, dropped, alive, dist, total)
    # and the other outputs: a drop reported under the cap, alive[] / dist[] not matching the drops
    dropped, alive, dist, total = (a.copy() for a in good)
    dropped[0] = 3
    with pytest.raises(AssertionError, match="under the cap"):
        M.replay(rows, c.n_old, c.n_new, c.cap, s0, dropped, alive, dist, total)
    dropped, alive, dist, total = (a.copy() for a in good)
    alive[np.nonzero(alive)[0][0]] = 0
    with pytest.raises(AssertionError, match="alive"):
        M.replay(rows, c.n_old, c.n_new, c.cap, s0, dropped, alive, dist, total)
    dropped, alive, dist, total = (a.copy() for a in good)
    dist[np.nonzero(alive)[0][1]] *= 1 + 3e-12
    with pytest.raises(AssertionError, match="survivors"):
        M.replay(rows, c.n_old, c.n_new, c.cap, s0, dropped, alive, dist, total)
    # an exact tie between different rows (hand-made): the later one goes
    erows = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0.5, 0]], np.float32)
    r = M.run(erows, 2, 1, 2, M.sum_of_old(erows, 2))
    assert r.gaps == [0.0] and r.dropped.tolist() == [1]                      # rows 0 and 1 tie exactly: the later one goes
