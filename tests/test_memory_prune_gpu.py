"""GPU suite: `ac_memory_add_prune` called directly with hand-built `ac_prune_job` arrays (as memory.py::_run_prune_jobs builds
them) and its four outputs -- dropped[], alive[], dist[], the fp64 sum -- held step by step to tests/memory_prune_ref.py:
the scalar and the float4 row paths, row counts on either side of the 16 waves and of the two-rows-per-wave stride, cap = 1,
an empty class, the largest supported class and embedding, several jobs of different sizes in one launch, exact duplicate
rows (the documented tie rule), and the refusals."""
import ctypes

import numpy as np
import pytest
import torch

import memory_prune_ref as M

pytestmark = pytest.mark.gpu

ROW_FILL, ALIVE_FILL, DIST_FILL, DROP_FILL = 777.0, 0xEE, -7.0, -99


class _Job:
    """Device buffers of one job, every output pre-filled with a sentinel and one element longer than the kernel may write."""

    def __init__(self, c, rows, dev):
        self.c, self.rows = c, rows
        ld = c.stride
        host = np.full(c.offset + c.n * ld + 4, ROW_FILL, np.float32)
        host[c.offset:c.offset + c.n * ld].reshape(c.n, ld)[:, :c.D] = rows
        self.rows_host = host
        self.d_rows = torch.from_numpy(host).to(dev)
        assert self.d_rows.data_ptr() % 16 == 0
        self.sum0 = M.sum_of_old(rows, c.n_old)
        self.d_sum = torch.from_numpy(np.concatenate([self.sum0, [DIST_FILL]])).to(dev)
        self.d_alive = torch.full((c.n + 1,), ALIVE_FILL, dtype=torch.uint8, device=dev)
        self.d_dist = torch.full((c.n + 1,), DIST_FILL, dtype=torch.float64, device=dev)
        self.d_drop = torch.full((c.n_new + 1,), DROP_FILL, dtype=torch.int32, device=dev)

    def fill(self, j, n_old=None, n_new=None, cap=None):
        c = self.c
        j.rows = self.d_rows.data_ptr() + 4 * c.offset
        j.ld = c.stride
        j.n_old, j.n_new, j.cap, j.reserved = (c.n_old if n_old is None else n_old, c.n_new if n_new is None else n_new,
                                               c.cap if cap is None else cap, 0)
        j.sum, j.alive, j.dist, j.dropped = self.d_sum.data_ptr(), self.d_alive.data_ptr(), self.d_dist.data_ptr(), self.d_drop.data_ptr()

    def outputs(self):
        s, a, d, dr = self.d_sum.cpu().numpy(), self.d_alive.cpu().numpy(), self.d_dist.cpu().numpy(), self.d_drop.cpu().numpy()
        assert s[-1] == DIST_FILL and a[-1] == ALIVE_FILL and d[-1] == DIST_FILL and dr[-1] == DROP_FILL      # nothing past the ends
        assert np.array_equal(self.d_rows.cpu().numpy(), self.rows_host)                                      # the rows are read only
        return dr[:-1], a[:-1], d[:-1], s[:-1]

    def untouched(self):
        s, a, d, dr = self.d_sum.cpu().numpy(), self.d_alive.cpu().numpy(), self.d_dist.cpu().numpy(), self.d_drop.cpu().numpy()
        return (np.array_equal(s[:-1], self.sum0) and (a == ALIVE_FILL).all() and (d == DIST_FILL).all() and (dr == DROP_FILL).all())

    def check(self):
        c = self.c
        dropped, alive, dist, total = self.outputs()
        try:
            return M.replay(self.rows, c.n_old, c.n_new, c.cap, self.sum0, dropped, alive, dist, total)
        except AssertionError as e:
            raise AssertionError(f"{c.name}: {e}") from None


def _launch(cuda_dev, jobs, D, overrides=None):
    from adaptive_classifier import _native as nv
    arr = (nv.ac_prune_job * len(jobs))()
    for i, job in enumerate(jobs):
        job.fill(arr[i], **((overrides or {}).get(i, {})))
    d_jobs = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(cuda_dev)
    with torch.cuda.device(cuda_dev):
        rc = nv.lib().ac_memory_add_prune(ctypes.cast(arr, ctypes.c_void_p), nv.ptr(d_jobs), len(jobs), D, nv.stream_ptr(cuda_dev))
    torch.cuda.synchronize(cuda_dev)
    return rc


@pytest.mark.parametrize("case", M.CASES, ids=[c.name for c in M.CASES])
def test_one_job_against_the_reference(case, cuda_dev):
    """Random rows: the seeds leave no near-tie (tests/test_memory_prune_ref_cpu.py), so besides passing the step-by-step
    replay the device has to take the reference's own arg-max at every step."""
    job = _Job(case, M.make_rows(case), cuda_dev)
    assert _launch(cuda_dev, [job], case.D) == 0
    assert job.check() == []
    dropped = job.outputs()[0]
    under = max(0, case.cap - case.n_old)
    assert (dropped[:under] == -1).all() and (dropped[under:] >= 0).all()


def test_five_jobs_of_different_sizes_in_one_launch(cuda_dev):
    jobs = [_Job(c, M.make_rows(c), cuda_dev) for c in M.MULTI_JOB_CASES]
    assert [(c.n, c.cap) for c in M.MULTI_JOB_CASES] == [(3, 1), (1025, 1000), (33, 32), (17, 5), (8192, 8190)]
    assert _launch(cuda_dev, jobs, M.MULTI_JOB_D) == 0
    for job in jobs:                                                         # each job on its own
        assert job.check() == [], job.c.name


@pytest.mark.parametrize("case", M.DUP_CASES, ids=[c.name for c in M.DUP_CASES])
def test_exact_duplicate_rows_follow_the_tie_rule(case, cuda_dev):
    """Stored and incoming rows hold exact copies, two of them of the row that is farthest when they arrive: on an exactly
    equal distance the later row goes (the replay checks it at every step), and only identical rows may be excused."""
    rows = M.make_rows(case)
    job = _Job(case, rows, cuda_dev)
    assert _launch(cuda_dev, [job], case.D) == 0
    for t, j, best in job.check():
        assert np.array_equal(rows[j], rows[best]), (t, j, best)
    dropped = job.outputs()[0]
    assert dropped[:2].tolist() == [case.n_old, case.n_old + 1]              # the copies of the farthest stored row, not the row itself
    # (every gap of these cases is either exactly 0, between identical rows, or above 1e-9: tests/test_memory_prune_ref_cpu.py)
    assert np.array_equal(dropped, M.run(rows, case.n_old, case.n_new, case.cap, job.sum0).dropped)


def test_refusals_launch_nothing(cuda_dev):
    from adaptive_classifier import _native as nv
    EINVAL, EUNSUPPORTED = -1, -2
    c = M.Case("refusal", 64, 8, 4, 8, 1)
    job = _Job(c, M.make_rows(c), cuda_dev)
    assert _launch(cuda_dev, [job], 4097) == EUNSUPPORTED and job.untouched()
    assert _launch(cuda_dev, [job], 64, {0: dict(n_old=8190, n_new=3, cap=8190)}) == EUNSUPPORTED and job.untouched()      # n = 8193
    assert _launch(cuda_dev, [job], 64, {0: dict(n_old=8, cap=7)}) == EINVAL and job.untouched()                             # n_old > cap
    assert _launch(cuda_dev, [job], 64, {0: dict(n_new=0)}) == EINVAL and job.untouched()
    assert nv.lib().ac_last_error()
    assert _launch(cuda_dev, [job], 64) == 0                                 # and the same buffers serve a valid call afterwards
    job.check()
