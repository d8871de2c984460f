"""No GPU: proves the fp16x2 yardstick of tests/encoder_f16x2_ref.py, which tests/test_encoder_f16x2_gpu.py holds the device to.

Which layer of the evidence this is: tests/test_f16x2_model_cpu.py states one product, tests/test_gemm_f16x2_gpu.py checks one GEMM
per element; this module and its GPU sibling check the whole encoder in that arithmetic on every dispatch branch and family.

  0. the counter: ac_gemm_f16x2_launches is exported (ac_version() >= 16) and answers without a GPU;
  1. the cases: F16_CASES is derived from the four grids (every planes branch of the BERT families, their mean-pooled cases, every
     planes case of MPNet and DeBERTa, the fall-back edges), with the fp16x2 launch count each must show;
  2. the split: encoder_f16x2_ref.split is tests/test_f16x2_model_cpu.py's, bit for bit; site_of names every nn.Linear;
  3. the instances (table 1): the three fp32 instances and the fp16x2 instance against fp64 per input -- rms (the yardstick is
     their maximum) and the fp16x2 instance's max-abs;
  4. F16X2_DEV (table 2): the constants hold, are rounded up and not padded, and no group exceeds ADMISSION x its fp32 figure;
  5. range admission: every nn.Linear operand of every case lies a factor 4 inside the fp16 range at its scale (a condition);
  6. the mutants (table 3): on every `sens` case of the BERT grid (CLS and mean) every harmful mutant lies at least
     2 x RMS_FACTOR yardsticks from fp64 -- so the GPU criterion RMS_FACTOR x yardstick fails it with a factor 2 to spare -- while
     the harmless one passes; MPNet / DeBERTa: the `_all` mutants and one single-site pair.  The same distances in max-abs device
     bounds are printed beside them: the max-abs criterion alone passes many of them.
"""
import numpy as np
import pytest
import torch

import encoder_ref as R
import encoder_pool_ref as P
import encoder_mpnet_ref as M
import encoder_deberta_ref as D
import encoder_f16x2_ref as F
from test_f16x2_model_cpu import split as model_split

OTHER_GRID_MUTANTS = ("lo_a_lost_all", "lo_w_lost_all", "hh_only", "lo_a_lost[qkv,0]", "lo_w_lost[ao,0]", "ll_added")


@pytest.fixture(scope="module", autouse=True)
def _threads():
    # (the instances are chains of small matmuls: more threads than this only slow them down)
    before = torch.get_num_threads()
    torch.set_num_threads(min(8, before))
    yield
    torch.set_num_threads(before)


def test_cases_are_derived_from_the_four_grids():
    ids = set(F.BY_ID)
    # one of every route the issue names as uncovered
    assert {"sa_longest33-cls", "attn_longest65-cls", "sa_longest129-cls", "sa_dh32_longest33-cls", "pm_holes_planes-cls",
            "pm_empty_row_planes-cls", "attn_straddle_boundary-cls", "last_T_lt_4b-cls", "last_b200-cls", "chunks_fused_then_not-cls",
            "last_ldo_wide-cls", "T192_ln_off-cls", "roberta_packed-cls", "xlm-roberta_packed-cls", "distilbert_packed-cls",
            "electra_packed-cls", "T192_all_fused-mean", "mp_S33_packed-cls", "mp_S33_packed-mean", "mp_dh32_S33-cls",
            "mp_S33_masked-mean", "db_S40_planes-cls", "db_S40_planes-mean", "db_holes-cls", "db_noshare-cls"} <= ids
    assert {fc.id for fc in F.F16_CASES if fc.fallback} == {"T191_no_planes-cls", "T150_of_100x2-cls", "mb_S40_planes_packed-cls",
                                                            "mp_S20_no_planes-cls", "mp_S20_no_planes-mean", "db_ragged9-cls",
                                                            "db_ragged9-mean"}
    takes = lambda c: c.model.family in R.BERT_FAMILIES and c.arith is None and c.branch in F.F16_BRANCHES
    assert sum(fc.grid == "bert" and not fc.fallback for fc in F.F16_CASES) == sum(takes(c) for c in R.CASES) >= 35
    assert sum(fc.grid == "pool" for fc in F.F16_CASES) == sum(takes(c) for c in P.POOL_CASES) >= 15
    assert sum(fc.grid == "mpnet" and not fc.fallback for fc in F.F16_CASES) == sum(bool(mc.case.ln_launches) for mc in M.MPNET_CASES)
    assert sum(fc.grid == "deberta" and not fc.fallback for fc in F.F16_CASES) == sum(bool(mc.case.ln_launches) for mc in D.DEBERTA_CASES)
    assert {fc.case.branch for fc in F.RUN_CASES if fc.grid == "bert"} == F.F16_BRANCHES
    for fc in F.F16_CASES:
        c, src = fc.case, fc.src if isinstance(fc.src, R.Case) else fc.src.case
        assert c.arith == "f16x2" and src.arith is None
        for f in ("id", "model", "batch", "branch", "ln_fusion", "env", "layered", "unpad", "ldo_extra", "max_tokens", "one_launch",
                  "ln_launches", "attn_launches", "path", "tokens"):
            assert getattr(c, f) == getattr(src, f), (fc.id, f)
        tokens = c.batch.b * c.batch.S if c.tokens < 0 else c.tokens
        L = c.model.layers
        if fc.fallback:
            assert F.f16_launches(fc) == 0 and (tokens < 192 or c.model.family == "modernbert"), fc.id
        else:
            assert tokens >= 192 and c.model.family != "modernbert", fc.id
            assert F.f16_launches(fc) == (4 * L if fc.pooling == "mean" else 4 * (L - 1) + 1) > 0, fc.id
            assert F.device_bound(fc) <= R.DEVICE_BOUND_CEILING
    ch = F.BY_ID["chunks_fused_then_not-cls"].case
    assert ch.max_tokens >= 192 > ch.batch.b * ch.batch.S - ch.max_tokens            # one fp16x2 chunk, then one that falls back
    assert set(F.F16X2_DEV) == {fc.group for fc in F.RUN_CASES}


def test_split_is_the_models_and_every_linear_has_a_site():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(4000, generator=g) * 10.0 ** (torch.rand(4000, generator=g) * 10 - 8)
    x = x[x.abs() < 60.0]
    for log2 in (F.ACT_LOG2, F.W_LOG2):
        h, l = F.split(x, log2)
        _, hn, ln = model_split(x.numpy(), log2)
        assert np.array_equal(h.double().numpy(), hn) and np.array_equal(l.double().numpy(), ln), log2
        ht, lt = F.split(x, log2, truncate=True)
        xs = x.double() * 2.0 ** log2
        normal = xs.abs() >= 2.0 ** -14
        assert bool((ht.double().abs() <= xs.abs())[normal].all()) and bool((ht != h).any())                  # toward zero
        assert bool(((xs - ht.double() - lt.double()).abs() <= torch.clamp(2.0 ** -21 * xs.abs(), min=2.0 ** -25)).all())
    assert (F.ACT_LOG2, F.W_LOG2) == (6, 10)
    for names, layer in ((R.BERT_NAMES, "encoder.layer.1."), (R.DISTIL_NAMES, "transformer.layer.1.")):
        got = [F.site_of(layer + names[k]) for k in ("q", "k", "v", "ao", "ff1", "ff2")]
        assert got == [("qkv", 1)] * 3 + [("ao", 1), ("ff1", 1), ("ff2", 1)], got
    assert F.site_of("encoder.layer.0.attention.attn.o") == ("ao", 0) and F.site_of("encoder.layer.2.attention.attn.k") == ("qkv", 2)
    assert F.site_of("encoder.layer.0.attention.self.key_proj") == ("qkv", 0)
    assert len(F.SINGLES) == 16 and all(F.F16_MUTANTS[n][0] for n in F.SINGLES)


def test_the_launch_counter_is_exported_and_answers_without_a_gpu():
    from adaptive_classifier import _native as nv
    L = nv.lib()
    assert L.ac_version() >= 16
    n = L.ac_gemm_f16x2_launches()
    assert isinstance(n, int) and n >= 0 and L.ac_gemm_f16x2_launches() == n          # a query: no launch, no growth


@pytest.fixture(scope="module")
def figures():
    out = {}
    for fc in F.RUN_CASES:
        f16 = F.f16x2_instance(fc)
        out[fc.id] = dict({k: F.rms(fc, v) for k, v in F.fp32_instances(fc).items()}, f16x2=F.rms(fc, f16), yard=F.rms_yard(fc),
                          dev=F.deviation(fc, f16))
    return out


def test_instances_and_the_yardstick(figures):
    print("\n[encoder f16x2 reference] rms deviation from fp64 per case: three fp32 instances, the fp16x2 instance; their maximum "
          "is the yardstick")
    print(f"  {'case':34s} {'torch fp32':>10s} {'chunks 16':>10s} {'transf.':>10s} {'fp16x2':>10s} {'rms_yard':>10s}   fp16x2 max-abs   fp32 figure")
    for fc in F.RUN_CASES:
        v = figures[fc.id]
        print(f"  {fc.id:34s} {v['torch']:10.1e} {v['chunk16']:10.1e} {v['transformers']:10.1e} {v['f16x2']:10.1e} {v['yard']:10.1e}"
              f"   {v['dev']:10.1e}       {F.fp32_figure(fc):.0e}")
        assert v["yard"] == max(v["torch"], v["chunk16"], v["transformers"], v["f16x2"]) > 0, fc.id
        # a correct fp16x2 model is an fp32-grade model: its rms is no worse than twice the worst fp32 instance's
        assert v["f16x2"] <= 2 * max(v["torch"], v["chunk16"], v["transformers"]), (fc.id, v)
        # ... so the yardstick is not inflated by it, and a yardstick is nowhere near a lost low plane (table 3)
        assert v["yard"] <= 1.5 * max(F.fp32_figure(fc), F.F16X2_DEV[fc.group]), (fc.id, v)      # (an rms is below its max-abs)


def test_f16x2_dev_table_holds_and_is_admitted(figures):
    worst = {}
    for fc in F.RUN_CASES:
        if figures[fc.id]["dev"] > worst.get(fc.group, (0.0, ""))[0]:
            worst[fc.group] = (figures[fc.id]["dev"], fc.id)
    fig32 = {fc.group: F.fp32_figure(fc) for fc in F.RUN_CASES}
    assert all(F.fp32_figure(fc) == fig32[fc.group] for fc in F.RUN_CASES)               # one fp32 figure per group
    print("\n[encoder f16x2 reference] worst max-abs deviation of the fp16x2 instance from fp64 per group")
    print(f"  {'pooling':9s} {'family':12s} {'regime':12s} {'fp16x2 instance':>40s}   F16X2_DEV   fp32 figure   ADMISSION x")
    for g in sorted(worst):
        print(f"  {g[0]:9s} {g[1]:12s} {g[2]:12s} {worst[g][0]:10.1e} {worst[g][1]:29s}   {F.F16X2_DEV[g]:.0e}       {fig32[g]:.0e}"
              f"         {R.ADMISSION * fig32[g]:.1e}")
    for fc in F.RUN_CASES:
        dev = figures[fc.id]["dev"]
        assert dev <= 1.5 * F.F16X2_DEV[fc.group], (fc.id, dev)      # (x 1.5: torch's blocked sums depend on the thread count and the CPU)
        assert dev <= R.ADMISSION * F.fp32_figure(fc), (fc.id, dev)
    for g, (top, cid) in worst.items():
        assert top > F.F16X2_DEV[g] / 4, (g, top)                                      # rounded up to one digit, not padded
        assert F.F16X2_DEV[g] <= R.ADMISSION * fig32[g], g                             # a group beyond it would be a finding: none
        assert R.KERNEL_FACTOR * fig32[g] >= 4 * F.F16X2_DEV[g], g                     # the grid's device bound holds fp16x2 too


def test_every_operand_lies_a_factor_four_inside_the_fp16_range():
    top = {"a": (0.0, ""), "w": (0.0, "")}
    for fc in F.RUN_CASES:
        seen = F.operand_range(fc)
        assert seen["a"] < F.ACT_MAX / F.RANGE_MARGIN and seen["w"] < F.W_MAX / F.RANGE_MARGIN, (fc.id, seen)
        for k in top:
            if seen[k] > top[k][0]:
                top[k] = (seen[k], fc.id)
    print(f"\n[encoder f16x2 reference] largest nn.Linear operands over {len(F.RUN_CASES)} cases: |activation| {top['a'][0]:.1f} ({top['a'][1]}) "
          f"against {F.ACT_MAX} / {F.RANGE_MARGIN}, |weight| {top['w'][0]:.2f} ({top['w'][1]}) against {F.W_MAX} / {F.RANGE_MARGIN}")
    assert top["a"][0] > 1.0 and top["w"][0] > 0.05                                     # the hook saw the operands


def test_every_harmful_mutant_fails_the_rms_criterion_with_a_factor_two_to_spare():
    need = 2 * F.RMS_FACTOR
    done, rows = set(), []
    weakest = {}                                    # grid kind -> (ratio, case, mutant) over the harmful single-site mutants
    below_maxabs = total = 0
    for fc in F.RUN_CASES:
        if not fc.sens or F._input(fc) in done:
            continue
        done.add(F._input(fc))
        bert = fc.grid in ("bert", "pool")
        names = tuple(F.F16_MUTANTS) if bert else OTHER_GRID_MUTANTS + ("split_truncates",)
        ratio, bounds = {}, {}
        for n in names:
            got = F.f16x2_instance(fc, (n,))
            finite = bool(torch.isfinite(got[R.compared_rows(fc.case.batch)]).all())
            ratio[n] = F.rms(fc, got) / F.rms_yard(fc) if finite else float("inf")     # (NaN rows: the device test asserts finite)
            bounds[n] = F.deviation(fc, got) / F.device_bound(fc) if finite else float("inf")
        rows.append((fc, ratio, bounds))
        for n in names:
            harmful = F.F16_MUTANTS[n][0]
            if harmful:
                assert ratio[n] >= need, (fc.id, n, ratio[n])
            elif harmful is False:
                assert ratio[n] <= F.RMS_FACTOR, (fc.id, n, ratio[n])                  # a harmless change passes the criterion
            if n in F.SINGLES:
                total += 1
                below_maxabs += bounds[n] <= 1.0
                key = "bert" if bert else fc.grid
                if ratio[n] < weakest.get(key, (float("inf"),))[0]:
                    weakest[key] = (ratio[n], fc.id, n)
    print(f"\n[encoder f16x2 reference] mutants: rms distance from fp64 in yardsticks (the device criterion is {F.RMS_FACTOR}; harmful "
          f"mutants must reach {need}); in brackets the same distance in max-abs device bounds (that criterion is 1)")
    print(f"  {'case':32s} {'weakest single-site':>22s} {'strongest single':>22s} {'lo_a_lost_all':>14s} {'lo_w_lost_all':>14s} {'hh_only':>14s} "
          f"{'act_scale_2^10':>14s} {'split_trunc.':>12s} {'ll_added':>12s}")
    short = lambda n: n[3] + n[9:]                   # lo_a_lost[qkv,1] -> a[qkv,1]
    cell = lambda r, b, n: f"{r[n]:7.0f} [{b[n]:5.1f}]" if n in r else f"{'-':>15s}"
    for fc, r, b in rows:
        sing = [n for n in r if n in F.SINGLES]
        lo, hi = min(sing, key=lambda n: r[n]), max(sing, key=lambda n: r[n])
        print(f"  {fc.id:32s} {short(lo):>8s} {cell(r, b, lo)} {short(hi):>8s} {cell(r, b, hi)} {cell(r, b, 'lo_a_lost_all')} {cell(r, b, 'lo_w_lost_all')} "
              f"{cell(r, b, 'hh_only')} {cell(r, b, 'act_scale_2^10')} {r['split_truncates']:5.2f} [{b['split_truncates']:4.2f}] "
              f"{r['ll_added']:5.2f} [{b['ll_added']:4.2f}]")
    print(f"  single-site mutants that PASS the max-abs device bound: {below_maxabs} of {total} (case, mutant) pairs; the weakest single-site "
          "ratio per grid: " + ", ".join(f"{k} {v[0]:.0f} ({v[2]} on {v[1]})" for k, v in sorted(weakest.items())))
    assert {fc.grid for fc, _, _ in rows} == {"bert", "pool", "mpnet", "deberta"}
    assert sum(fc.grid in ("bert", "pool") for fc, _, _ in rows) >= 30
    # the ceiling of RMS_FACTOR: half the weakest harmful single-site ratio (of the BERT grid, and of every grid)
    assert F.RMS_FACTOR <= min(v[0] for v in weakest.values()) / 2, weakest
    # ... and why rms: the max-abs bound alone passes single-site mistakes
    assert below_maxabs > 0
