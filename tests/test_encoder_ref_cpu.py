"""No GPU: proves the fp64 encoder reference of tests/encoder_ref.py and the case grid the device is judged on.

  1. the reference IS the model: for every case the fp64 forward lies within ADMISSION x FP32_DEV of transformers fp32 eager, and
     for the BERT families within 1e-12 of the transformers module cast to fp64 (ModernBertModel.double() returns NaN on some
     shapes and is not used);
  2. admission: both fp32 instances of the reference (torch's matmul; K-chunks of 16 summed in sequence) lie within
     ADMISSION x FP32_DEV, and the FP32_DEV constants are the groups' worst figures (printed as a table);
  3. sensitivity: every mutant of the forward (a plausible kernel mistake) is farther than 4 x the device bound from the reference
     in at least one case of EACH expected-branch group it can occur in -- a grid that is blind to a mistake on some branch fails
     here (fix the case, not the bound).  Printed for the record: the mutants that stay below the older 1e-4 bar in every case;
  4. the peaked regimes are peaked: mean max attention probability >= 0.5 (>= 0.3 from S = 256) on the fp64 probabilities.
"""
import copy

import pytest
import torch
import torch.nn.functional as F

import encoder_ref as R

OLD_BAR = 1e-4
VISIBLE = 4                     # a mutant counts as seen when it is this many device bounds away


def _unique_inputs():
    seen, out = set(), []
    for c in R.CASES:
        if (c.model, c.batch) not in seen:
            seen.add((c.model, c.batch))
            out.append(c)
    return out


INPUTS = _unique_inputs()


@pytest.fixture(scope="module")
def fp32_devs():
    """case id -> {instance: deviation from fp64}, one entry per distinct (model, batch)"""
    torch.set_num_threads(min(16, torch.get_num_threads()))
    out = {}
    for c in INPUTS:
        out[c.id] = {"torch": R.deviation(c, R.fp32_instance(c)), "chunk16": R.deviation(c, R.fp32_instance(c, chunked=True)),
                     "transformers": R.deviation(c, R.transformers_fp32(c))}
    return out


def test_case_table_is_consistent():
    for c in R.CASES:
        assert c.group in R.FP32_DEV, c.id
        assert R.device_bound(c) <= R.DEVICE_BOUND_CEILING
        assert bool(R.compared_rows(c.batch).any()), c.id
        ids, types, mask = R.make_batch(c.batch)
        if c.batch.lengths is not None and mask is not None:
            holes = len(c.batch.holes)
            assert int(mask.sum()) == sum(c.batch.lengths) - holes, c.id                 # every length as the table states it
        if c.path == "packed":
            assert c.tokens == sum(c.batch.lengths) < c.batch.b * c.batch.S, c.id
        assert torch.isfinite(R.reference(c)[R.compared_rows(c.batch)]).all(), c.id
        assert (R.reference(c)[R.compared_rows(c.batch)].norm(dim=1) - 1).abs().max() < 1e-14
    for branch in R.BRANCHES:
        assert any(c.sens for c in R.CASES if c.branch == branch), f"no sensitivity case on branch {branch}"


def test_reference_is_the_model_and_cases_are_admitted(fp32_devs):
    worst = {}
    for c in INPUTS:
        d = fp32_devs[c.id]
        for inst, v in d.items():
            w = worst.setdefault(c.group, {})
            if v > w.get(inst, (0.0, ""))[0]:
                w[inst] = (v, c.id)
    print("\n[encoder reference] worst fp32 deviation from fp64 per group (max-abs on the unit CLS vector)")
    print(f"  {'group':28s} {'torch fp32':>26s} {'K-chunks of 16':>26s} {'transformers fp32':>26s}   FP32_DEV  device bound")
    for group in sorted(worst):
        cells = "".join(f" {worst[group][i][0]:9.1e} {worst[group][i][1][:16]:16s}" for i in ("torch", "chunk16", "transformers"))
        print(f"  {str(group):28s}{cells}   {R.FP32_DEV[group]:.0e}     {R.KERNEL_FACTOR * R.FP32_DEV[group]:.1e}")
    for c in INPUTS:
        for inst, v in fp32_devs[c.id].items():
            assert v <= R.ADMISSION * R.FP32_DEV[c.group], (c.id, inst, v)           # the reference is the model; admission
            # ... and the constants ARE the worst figures (x 1.5: torch's blocked sums depend on the thread count and the CPU,
            # which moves a figure by tens of percent between machines)
            assert v <= 1.5 * R.FP32_DEV[c.group], (c.id, inst, v)
    for group, w in worst.items():
        top = max(v for v, _ in w.values())
        assert top > R.FP32_DEV[group] / 4, (group, top)                             # ... rounded up to one digit, not padded


@pytest.mark.parametrize("case", [c for c in INPUTS if c.model.family in R.BERT_FAMILIES and c.model.hidden <= 384],
                         ids=lambda c: c.id)
def test_reference_equals_the_fp64_module(case):
    """transformers' own module in fp64 as a second opinion (BERT families; the narrow models: same code at every width)"""
    model = copy.deepcopy(R.make_model(case.model)).double()
    ids, types, mask = R.make_batch(case.batch)
    kw = dict(input_ids=ids)
    if mask is not None:
        kw["attention_mask"] = mask
    if types is not None:
        kw["token_type_ids"] = types
    with torch.no_grad():
        want = F.normalize(model(**kw).last_hidden_state[:, 0, :], p=2, dim=1)
    rows = R.compared_rows(case.batch)
    assert want.dtype == torch.float64
    assert float((want - R.reference(case))[rows].abs().max()) < 1e-12


def test_every_mutant_is_visible_on_every_branch_it_can_occur_in():
    dist = {}                                   # (case id, mutant) -> distance
    for c in R.CASES:
        if c.sens:
            for name in R.MUTANTS:
                if R.applicable(name, c):
                    dist[(c.id, name)] = R.mutant_distance(c, name)
    blind = []
    for branch in R.BRANCHES:
        cases = [c for c in R.CASES if c.branch == branch and c.sens]
        for name in R.MUTANTS:
            ds = [(dist[(c.id, name)] / R.device_bound(c), c.id) for c in cases if (c.id, name) in dist]
            if ds and max(ds)[0] <= VISIBLE:
                blind.append((branch, name, max(ds)))
    print("\n[encoder reference] the least visible mutant per branch group (distance in device bounds, best case of the group)")
    for branch in R.BRANCHES:
        cases = [c for c in R.CASES if c.branch == branch and c.sens]
        best = {}
        for name in R.MUTANTS:
            ds = [dist[(c.id, name)] / R.device_bound(c) for c in cases if (c.id, name) in dist]
            if ds:
                best[name] = max(ds)
        name = min(best, key=best.get)
        print(f"  {branch:22s} {len(best):2d} mutants, least visible: {name:18s} {best[name]:10.1f} x the bound")
    under_old = sorted(name for name in R.MUTANTS
                       if any(k[1] == name for k in dist) and all(v < OLD_BAR for k, v in dist.items() if k[1] == name))
    print(f"[encoder reference] mutants below the 1e-4 bar in EVERY case of the grid (invisible to the older tests): {under_old}")
    some_under_old = sorted({name for (cid, name), v in dist.items() if v < OLD_BAR})
    print(f"[encoder reference] mutants below the 1e-4 bar in at least one case where they apply: {some_under_old}")
    assert not blind, sorted(blind)


def test_peaked_regimes_are_peaked():
    for c in INPUTS:
        if c.model.regime.startswith("peaked") and c.batch.S > 1:
            p = R.peak_stats(c)
            assert p >= (0.3 if c.batch.S >= 256 else 0.5), (c.id, p)
