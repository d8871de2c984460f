"""No GPU: proves the pooled reference of tests/encoder_pool_ref.py and the host side of `pooling="mean"`.

  1. admission: the three fp32 instances of the pooled reference (torch's matmul; K-chunks of 16; transformers fp32 eager) lie
     within ADMISSION x FP32_DEV_POOL of fp64 on every case, and the constants are the groups' worst figures (printed as a table);
  2. sensitivity: every pooling mutant is at least VISIBLE device bounds from the reference on EVERY case it applies to;
  3. the ABI: ac_version() >= 9, `pool_opt` is the trailing int of both config structs in the header and in the ctypes mirror, the
     library reads it there (the host-only workspace planners refuse pool_opt = 9 and accept 0, 1, 2 with equal sizes);
  4. the names: constructor and encode_cls validation ("cls" | "mean", anything else ValueError) -- on the functions the GPU
     classes call, which need no device.
"""
import ctypes
import os
import re

import pytest
import torch

import encoder_ref as R
import encoder_pool_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VISIBLE = 4                     # as tests/test_encoder_ref_cpu.py: a mutant counts as seen when it is this many device bounds away


def _unique_inputs():
    seen, out = set(), []
    for c in P.POOL_CASES:
        if (c.model, c.batch) not in seen:
            seen.add((c.model, c.batch))
            out.append(c)
    return out


INPUTS = _unique_inputs()


@pytest.fixture(scope="module")
def fp32_devs():
    torch.set_num_threads(min(16, torch.get_num_threads()))
    return {c.id: {"torch": P.deviation(c, P.fp32_instance(c)), "chunk16": P.deviation(c, P.fp32_instance(c, chunked=True)),
                   "transformers": P.deviation(c, P.transformers_fp32(c))} for c in INPUTS}


def test_pool_case_table_is_consistent():
    assert len(P.POOL_CASES) == 37
    for c in P.POOL_CASES:
        base = R.BY_ID[c.id]
        L = c.model.layers
        assert c.group in P.FP32_DEV_POOL, c.id
        assert P.device_bound(c) <= R.DEVICE_BOUND_CEILING
        assert P.FP32_DEV_POOL[c.group] <= R.FP32_DEV[c.group], c.group          # the mean is no noisier than the CLS row
        assert not c.one_launch
        assert c.ln_launches == (2 * L if base.ln_launches == 2 * (L - 1) else 0), c.id
        assert c.attn_launches == (L if base.attn_launches == L - 1 else 0), c.id
        assert (c.path, c.tokens) == (base.path, base.tokens), c.id
        tokens = c.batch.b * c.batch.S if c.tokens < 0 else c.tokens
        assert tokens <= 410 or c.id in ("last_b200", "mb_b200"), c.id          # small (the straddle cases need their 410 rows)
        rows = R.compared_rows(c.batch)
        ref = P.pooled_reference(c)
        assert torch.isfinite(ref).all(), c.id
        assert (ref[rows].norm(dim=1) - 1).abs().max() < 1e-14
        assert bool((ref[~rows] == 0).all()), c.id                               # an all-masked row: exactly zero
    assert set(P.FP32_DEV_POOL) == {c.group for c in P.POOL_CASES}


def test_pooled_reference_is_admitted_and_the_table_holds(fp32_devs):
    worst = {}
    for c in INPUTS:
        for inst, v in fp32_devs[c.id].items():
            w = worst.setdefault(c.group, {})
            if v > w.get(inst, (0.0, ""))[0]:
                w[inst] = (v, c.id)
    print("\n[encoder pool reference] worst fp32 deviation from fp64 per group (max-abs on the unit mean-pooled vector)")
    print(f"  {'group':28s} {'torch fp32':>26s} {'K-chunks of 16':>26s} {'transformers fp32':>26s}   FP32_DEV_POOL  device bound")
    for group in sorted(worst):
        cells = "".join(f" {worst[group][i][0]:9.1e} {worst[group][i][1][:16]:16s}" for i in ("torch", "chunk16", "transformers"))
        print(f"  {str(group):28s}{cells}   {P.FP32_DEV_POOL[group]:.0e}     {R.KERNEL_FACTOR * P.FP32_DEV_POOL[group]:.1e}")
    for c in INPUTS:
        for inst, v in fp32_devs[c.id].items():
            assert v <= R.ADMISSION * P.FP32_DEV_POOL[c.group], (c.id, inst, v)
            # ... and the constants ARE the worst figures (x 1.5: torch's blocked sums depend on the thread count and the CPU)
            assert v <= 1.5 * P.FP32_DEV_POOL[c.group], (c.id, inst, v)
    for group, w in worst.items():
        top = max(v for v, _ in w.values())
        assert top > P.FP32_DEV_POOL[group] / 4, (group, top)                    # ... rounded up to one digit, not padded


def test_every_pooling_mutant_is_visible_on_every_case_it_applies_to():
    least = {}
    pairs = 0
    for c in INPUTS:
        for name in P.POOL_MUTANTS:
            if not P.applicable(name, c):
                continue
            pairs += 1
            d = P.mutant_distance(c, name) / P.device_bound(c)
            if d < least.get(name, (float("inf"), ""))[0]:
                least[name] = (d, c.id)
            assert d >= VISIBLE, (c.id, name, d)
    print(f"\n[encoder pool reference] {pairs} (case, mutant) pairs; the least visible case of every mutant, in device bounds")
    for name, (d, cid) in sorted(least.items()):
        print(f"  {name:24s} {d:10.0f} x the bound   {cid}")
    assert set(least) == set(P.POOL_MUTANTS)                                     # every mutant applies somewhere
    # where a mutant does not apply it really changes nothing worth a bound (the flat regimes' equal token norms; no padding)
    for c in INPUTS:
        for name in ("include_pad", "normalize_tokens_first"):
            if c.model.family in P.POOL_MUTANTS[name][0] and not P.applicable(name, c):
                assert P.mutant_distance(c, name) < P.device_bound(c), (c.id, name)


# ---- the ABI -------------------------------------------------------------------------------------------------------------
def _header_struct(name):
    src = open(os.path.join(ROOT, "include", "acamd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    body = re.search(r"typedef struct \{([^}]*)\}\s*" + name + r"\s*;", src).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            typ, names = decl.split(None, 1)
            fields += [(typ, n.strip()) for n in names.split(",")]
    return fields


@pytest.mark.parametrize("struct", ["ac_bert_config", "ac_modernbert_config"])
def test_header_and_ctypes_agree_on_pool_opt(struct):
    from adaptive_classifier import _native as nv
    header = _header_struct(struct)
    mirror = getattr(nv, struct)._fields_
    assert header[-1] == ("int", "pool_opt"), header[-1]
    assert [n for _, n in header] == [n for n, _ in mirror]
    assert all({"int": ctypes.c_int, "float": ctypes.c_float}[t] is ct for (t, _), (_, ct) in zip(header, mirror))
    assert getattr(nv, struct).pool_opt.offset == ctypes.sizeof(getattr(nv, struct)) - 4       # the trailing field
    src = open(os.path.join(ROOT, "include", "acamd.h")).read()
    for name, value in (("AC_POOL_DEFAULT", 0), ("AC_POOL_CLS", 1), ("AC_POOL_MEAN", 2)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), src), name
        assert getattr(nv, name) == value


def test_library_reads_pool_opt_and_the_workspace_does_not_depend_on_it():
    from adaptive_classifier import _native as nv
    L = nv.lib()
    assert L.ac_version() >= 9
    n = ctypes.c_size_t(0)
    for b, S in ((256, 32), (2, 12), (1, 1)):
        sizes = []
        for opt in (nv.AC_POOL_DEFAULT, nv.AC_POOL_CLS, nv.AC_POOL_MEAN):
            cfg = nv.ac_bert_config(768, 12, 12, 3072, 30522, 512, 2, 1e-12, 0, 0, 0, opt)
            assert L.ac_bert_workspace(ctypes.byref(cfg), b, S, ctypes.byref(n)) == 0
            sizes.append(n.value)
            mb = nv.ac_modernbert_config(768, 22, 12, 1152, 50368, 8192, 3, 64, 1e-5, 0, opt)
            assert L.ac_modernbert_workspace(ctypes.byref(mb), b, S, ctypes.byref(n)) == 0
            sizes.append(n.value)
        assert sizes[0::2] == [sizes[0]] * 3 and sizes[1::2] == [sizes[1]] * 3, sizes
    for opt in (9, -1, 3):
        bad = nv.ac_bert_config(768, 12, 12, 3072, 30522, 512, 2, 1e-12, 0, 0, 0, opt)
        assert L.ac_bert_workspace(ctypes.byref(bad), 4, 8, ctypes.byref(n)) == -1             # AC_EINVAL
        assert b"pool_opt" in L.ac_last_error()
        bad = nv.ac_modernbert_config(768, 22, 12, 1152, 50368, 8192, 3, 64, 1e-5, 0, opt)
        assert L.ac_modernbert_workspace(ctypes.byref(bad), 4, 8, ctypes.byref(n)) == -1
        assert b"pool_opt" in L.ac_last_error()
    # a zero-initialised struct means the default
    assert nv.ac_bert_config().pool_opt == 0 and nv.ac_modernbert_config().pool_opt == 0


# ---- the names -------------------------------------------------------------------------------------------------------------
def test_pooling_names_are_validated():
    from adaptive_classifier import _native as nv, encoder as E
    assert E.pooling_mode("cls") == nv.AC_POOL_CLS and E.pooling_mode("mean") == nv.AC_POOL_MEAN
    for bad in ("max", "CLS", "", None, 2):
        with pytest.raises(ValueError):
            E.pooling_mode(bad)
    for cls in (E.HipBertEncoder, E.HipModernBertEncoder):
        assert cls.encode is cls.encode_cls
        enc = cls.__new__(cls)                                   # (no device: only the per-call config is built)
        enc.arith, enc.ln_fusion, enc.pooling = None, None, "cls"
        enc.ccfg = (nv.ac_bert_config if cls is E.HipBertEncoder else nv.ac_modernbert_config)()
        assert enc._call_cfg().pool_opt == nv.AC_POOL_DEFAULT            # the struct a call without the option always passed
        assert enc._call_cfg(pooling="cls").pool_opt == nv.AC_POOL_DEFAULT
        assert enc._call_cfg(pooling="mean").pool_opt == nv.AC_POOL_MEAN
        enc.pooling = "mean"
        assert enc._call_cfg().pool_opt == nv.AC_POOL_MEAN and enc._call_cfg(pooling="cls").pool_opt == nv.AC_POOL_DEFAULT
        with pytest.raises(ValueError):
            enc._call_cfg(pooling="max")
    # constructors: the name is checked before anything touches the device
    for cls in (E.HipBertEncoder, E.HipModernBertEncoder):
        with pytest.raises(ValueError):
            cls(object(), pooling="max")


def test_flops_count_the_full_last_layer_under_mean():
    from adaptive_classifier import _native as nv, encoder as E
    enc = E.HipBertEncoder.__new__(E.HipBertEncoder)
    enc.pooling = "cls"
    enc.ccfg = nv.ac_bert_config(768, 12, 12, 3072, 30522, 512, 2, 1e-12)
    full = enc.flops(256, 32, executed=False)
    assert enc.flops(256, 32, executed=True, pooling="mean") == full > enc.flops(256, 32, executed=True)
    assert enc.flops(256, 32, executed=True, pooling="cls") == enc.flops(256, 32, executed=True)
    packed = enc.flops(256, 32, tokens=5000, sum_len_sq=110000.0, pooling="mean")
    per_tok = 2.0 * (4.0 * 768 * 768 + 2.0 * 768 * 3072)
    assert packed == (per_tok * 5000 + 4.0 * 12 * 110000.0 * 64) * 12 > enc.flops(256, 32, tokens=5000, sum_len_sq=110000.0)
