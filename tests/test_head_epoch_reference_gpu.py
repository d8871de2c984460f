"""GPU suite: head training (`ac_head_train_epoch`, `ac_head_train_step`) against a plain fp64 epoch, over every dispatch branch.

For every case of tests/head_epoch_ref.py's grid FOUR device legs run from the head's own initial parameters --
{fused_epoch, fused_step in a loop} x {the plain call, the call with stepwise=True} -- and each leg is compared with ONE fp64
trajectory of the same batches, dropout masks (the numpy port of ac::dropout_keep) and optimizer: never with another leg.

  numerics    parameters, m, v, the last step's raw gradients, loss_accum and out3 of every leg against fp64.
              Regime "default" (eps = 1e-8, at most 4 steps): head_epoch_ref.DEFAULT_BOUNDS, the bars tests/test_head_gpu.py
              holds.  Regime "conditioned" (eps = 1e-4; the long40-*, long120-*, epochs3-* cases): 16 x the fp32 torch-CPU
              instance's own deviation from fp64 (head_epoch_ref.CONDITIONED_BOUNDS; the table there, the figures from
              tests/test_head_epoch_reference_cpu.py).
  selection   the `head_epoch` counter of ac_persistent_launches() around every call: +1 per persistent epoch or step, +0 on the
              step-by-step path, against the expectation written by hand in the case table.  Skipped -- this assertion only -- on a
              device that does not have 256 active CUs and 160 KB of LDS per workgroup (the table is derived for that device).
  identity    on either path, the epoch call and the step loop leave the same bits (parameters, m, v, loss_accum, out3).

Observed on an MI355X (max over the cases of a regime, worst leg of the path; for the record -- the bounds do not come from these):
see the table at the end of this file.
"""
import ctypes
import time

import pytest
import torch

import head_epoch_ref as R

pytestmark = pytest.mark.gpu

_BY_ID = {c.id: c for c in R.CASES}
LEGS = (("epoch", False), ("steps", False), ("epoch", True), ("steps", True))      # (entry point, stepwise)


def _launches():
    from adaptive_classifier import _native as nv
    he, bs = ctypes.c_int64(0), ctypes.c_int64(0)
    nv.check(nv.lib().ac_persistent_launches(ctypes.byref(he), ctypes.byref(bs)), "ac_persistent_launches")
    return he.value


def _selection_device():
    """None if the case table's selection column applies to this device, else why not."""
    from adaptive_classifier import _native as nv
    chip, act = ctypes.c_int(0), ctypes.c_int(0)
    nv.check(nv.lib().ac_device_cus(ctypes.byref(chip), ctypes.byref(act)), "ac_device_cus")
    lds = nv.device_info()["lds_per_block"]
    if act.value != 256 or lds < 160 * 1024:
        return f"selection not asserted: {act.value} active CUs / {lds} bytes of LDS per workgroup (the table is written for 256 / 163840)"
    return None


def _padded(t, pad, dev):
    """t as a column slice of a block `pad` columns wider, the extra columns NaN."""
    big = torch.full((t.shape[0], t.shape[1] + pad), float("nan"), device=dev)
    big[:, :t.shape[1]] = t.to(dev)
    return big[:, :t.shape[1]]


def _device_data(case, data, dev):
    X = data.X
    if case.layout == "dense":
        Xd = X.to(dev)
    elif case.layout in ("ld+2", "ld+4"):
        Xd = _padded(X, int(case.layout[3:]), dev)
    else:                                                  # 4 bytes past a 16-byte boundary, rows D floats apart
        assert case.layout == "off4"
        buf = torch.full((X.numel() + 4,), float("nan"), device=dev)
        assert buf.data_ptr() % 16 == 0
        Xd = buf[1:1 + X.numel()].view(X.shape)
        Xd.copy_(X)
        assert Xd.data_ptr() % 16 == 4
    assert Xd.stride(1) == 1
    yd = None if data.y is None else data.y.to(dev)
    Td = None
    if data.targets is not None:
        Td = _padded(data.targets, case.ldt_pad, dev) if case.ldt_pad else data.targets.to(dev)
    od = None if data.order is None else data.order.to(dev)
    fd = None if data.fisher is None else data.fisher.to(dev)
    oldd = None if data.old is None else data.old.to(dev)
    return Xd, yd, Td, od, fd, oldd


def _run_leg(case, data, dd, flat0, dev, entry, stepwise):
    from adaptive_classifier.training import HeadTrainer
    Xd, yd, Td, od, fd, oldd = dd
    head = R.make_head_module(case).to(dev)
    tr = HeadTrainer(head, lr=case.lr, eps=case.eps, weight_decay=case.wd, max_grad_norm=case.max_norm)
    assert torch.equal(tr.flat.cpu(), flat0)
    tr.loss_accum.zero_()
    kind = R.LOSS_KIND[case.loss]
    n, B = case.n, case.batch
    deltas = []
    for ep in range(case.epochs):
        seed0 = R.seed0_of(case, ep)
        before = _launches()
        if entry == "epoch":
            done = tr.fused_epoch(Xd, yd, od, B, case.p, seed0, fisher=fd, old_params=oldd, lambda_B=data.lambda_B, loss_kind=kind,
                                  targets_all=Td, stepwise=stepwise)
            assert done == -(-n // B)
        else:
            for i, off in enumerate(range(0, n, B)):
                nb = min(B, n - off)
                lam = (data.lambda_B / nb) if fd is not None else 0.0
                if od is not None:
                    tr.fused_step(Xd, yd, od[off:off + nb], case.p, seed0 + i, fisher=fd, old_params=oldd, lambda_over_B=lam,
                                  loss_kind=kind, targets_all=Td, stepwise=stepwise)
                else:
                    tr.fused_step(Xd[off:off + nb], None if yd is None else yd[off:off + nb], None, case.p, seed0 + i, fisher=fd,
                                  old_params=oldd, lambda_over_B=lam, loss_kind=kind,
                                  targets_all=None if Td is None else Td[off:off + nb], stepwise=stepwise)
        torch.cuda.synchronize()
        deltas.append(_launches() - before)
    assert tr.t == case.steps
    bits = torch.cat([tr.flat, tr.m, tr.v, tr.loss_accum, tr.out3]).clone()
    return R.state_of(tr), deltas, bits


_RESULTS = {}


def _run_case(case_id):
    """A case runs ONCE per session, whichever test asks first; a failure inside it is kept and raised again, not re-run."""
    if case_id not in _RESULTS:
        try:
            _RESULTS[case_id] = _run_case_once(case_id)
        except Exception as e:          # noqa: BLE001
            _RESULTS[case_id] = e
    if isinstance(_RESULTS[case_id], Exception):
        raise _RESULTS[case_id]
    return _RESULTS[case_id]


def _run_case_once(case_id):
    """All four legs of a case against one fp64 trajectory; returns only small things (deviations, launch deltas, identities)."""
    case = _BY_ID[case_id]
    dev = torch.device("cuda:0")
    flat0 = R.make_head_module(case).flat_params().detach().clone()
    data = R.make_data(case, flat0)
    ref, _ = R.run_ref(case, data, flat0, torch.float64)
    want = R.state_of(ref)
    assert ref.t == case.steps
    dd = _device_data(case, data, dev)
    res = {"dev": {}, "deltas": {}, "identical": {}}
    bits = {}
    for entry, stepwise in LEGS:
        got, deltas, bits[(entry, stepwise)] = _run_leg(case, data, dd, flat0, dev, entry, stepwise)
        res["dev"][(entry, stepwise)] = R.deviation(got, want)
        res["deltas"][(entry, stepwise)] = deltas
    for stepwise in (False, True):
        res["identical"][stepwise] = bool(torch.equal(bits[("epoch", stepwise)], bits[("steps", stepwise)]))
    return res


@pytest.fixture(scope="module", autouse=True)
def _wall_time(cuda_dev):
    t0 = time.time()
    yield
    print(f"\n[head epoch reference] module wall time {time.time() - t0:.1f} s")


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.id)
def test_every_leg_matches_the_fp64_epoch(case, cuda_dev):
    res = _run_case(case.id)
    bounds = R.bounds_of(case)
    for (entry, stepwise), dev in res["dev"].items():
        print(f"\n[device vs fp64] {case.id:24s} {'stepwise  ' if stepwise else 'plain     '}{entry:5s} "
              + "  ".join(f"{q} {dev[q]:.1e}" for q in R.QUANTITIES), end="")
    for (entry, stepwise), dev in res["dev"].items():
        for q in R.QUANTITIES:
            assert dev[q] <= bounds[q], (case.id, entry, "stepwise" if stepwise else "plain", q, dev[q], bounds[q])


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.id)
def test_the_expected_path_ran(case, cuda_dev):
    res = _run_case(case.id)
    why_not = _selection_device()
    if why_not:
        pytest.skip(why_not)
    per_epoch, per_loop = case.expected_launches
    assert res["deltas"][("epoch", False)] == [per_epoch] * case.epochs, (case.id, "fused_epoch", res["deltas"])
    assert res["deltas"][("steps", False)] == [per_loop] * case.epochs, (case.id, "fused_step loop", res["deltas"])
    assert res["deltas"][("epoch", True)] == [0] * case.epochs and res["deltas"][("steps", True)] == [0] * case.epochs, res["deltas"]


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.id)
def test_epoch_call_and_step_loop_leave_the_same_bits(case, cuda_dev):
    """`epoch == step loop`, bit for bit, on the persistent path (ragged shapes, batches below 32 rows and 120-step epochs
    included) as on the step-by-step one."""
    res = _run_case(case.id)
    assert res["identical"][False], (case.id, "plain")
    assert res["identical"][True], (case.id, "stepwise")


# Observed on an MI355X (256 CUs), maximum over the cases of the regime and over both entry points -- for the record:
#
#   regime / path               params    m         v         grads     loss_accum  out3        bound (params .. out3)
#   default      persistent     1.5e-5    6.4e-8    2.4e-9    4.8e-7    1.5e-7      2.7e-7      5e-5  1e-6  1e-8  1e-5  1e-4  1e-4
#   default      step-by-step   1.6e-5    6.5e-8    2.3e-9    8.7e-7    1.5e-7      2.7e-7
#   conditioned  persistent     9.8e-7    6.5e-8    1.1e-8    1.1e-7    2.3e-7      7.9e-7      8e-6  1.1e-6  4.8e-8  1.9e-6  3.2e-6  6.4e-5
#   conditioned  step-by-step   9.8e-7    6.6e-8    1.2e-8    1.1e-7    2.3e-7      7.9e-7
#   fp32 torch-CPU instance, 40-step cases (head_epoch_ref.FP32_DEV_40):
#                               4.6e-7    6.5e-8    2.6e-9    1.1e-7    1.7e-7      3.6e-6
#
# Both device paths sit at the fp32 instance's own distance from fp64 (the conditioned worst cases are the 120-step ones), a
# factor 8 and more inside the bounds: neither needs the factor 16.  All four instantiations head_epoch_kernel<4|16, 3|4, 2> run
# (R1 = 4 from 1024 / [1024, 256], which no head with the default hidden sizes [D, D // 2] reaches on 256 CUs).
# Wall time: this module adds 9 s to the GPU suite (359 s at the parent commit): 58 cases x 4 legs, one fp64 trajectory per case.
