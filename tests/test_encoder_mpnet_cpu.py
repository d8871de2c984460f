"""No GPU: proves the MPNet reference of tests/encoder_mpnet_ref.py and the host side of the family.

  1. the restatement: the helper's fp32 forward equals transformers' MPNetModel (fp32, eager) to the regime's figure on every case;
  2. admission: the three fp32 instances lie within ADMISSION x FP32_DEV_MPNET of fp64 on every case, and the constants are the
     regimes' worst figures (printed as a table);
  3. sensitivity: every mutant, on at least one case it applies to, lies at least VISIBLE = 8 device bounds from the reference;
  4. the table: encoder.build_rel_bias equals the model's own compute_position_bias read along every diagonal;
  5. the ABI: ac_version() >= 11, `attn_rel_bias` / `rel_span` trail ac_bert_weights in the header and in the ctypes mirror, the
     workspace does not depend on the table, S > rel_span is AC_EINVAL naming rel_span at every encode entry;
  6. the constructor's device-free part: the parameter-name map resolves a real MPNetModel.state_dict(), relu is refused;
  7. the device listing: the BIAS instantiations hold no scratch and no flat access, and read 16 more dwords per key tile.
"""
import ctypes
import os
import re

import pytest
import torch

import encoder_ref as R
import encoder_mpnet_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VISIBLE = 8


@pytest.fixture(scope="module")
def fp32_devs():
    torch.set_num_threads(min(16, torch.get_num_threads()))
    out = {}
    for mc in M.MPNET_CASES:
        mine, theirs = M.fp32_instance(mc), M.transformers_fp32(mc)
        out[mc.id] = {"torch": M.deviation(mc, mine), "chunk16": M.deviation(mc, M.fp32_instance(mc, chunked=True)),
                      "transformers": M.deviation(mc, theirs), "mine - transformers": float((mine - theirs).abs().max())}
    return out


def test_case_table_is_consistent():
    ids = {mc.case.id for mc in M.MPNET_CASES}
    assert {"mp_S33_packed", "mp_S70_packed", "mp_S140_packed", "mp_dh32_S33", "mp_S33_masked", "mp_small_T32", "mp_768_planes",
            "mp_768_f32"} <= ids
    for mc in M.MPNET_CASES:
        c = mc.case
        assert not c.one_launch and c.attn_launches == 0, mc.id                   # what a bias table rules out
        assert M.device_bound(mc) <= R.DEVICE_BOUND_CEILING
        token_layers = c.model.layers if mc.pooling == "mean" else c.model.layers - 1
        assert c.ln_launches in (0, 2 * token_layers), mc.id
        tokens = c.batch.b * c.batch.S if c.tokens < 0 else c.tokens
        assert (c.ln_launches > 0) == (tokens >= 192 and c.arith is None), mc.id  # gemm_plan.h kTileMinM, bf16x3 planes
        assert tokens <= 300, mc.id
        span = M.make_model(c.model).config.max_position_embeddings - (M.PAD_ID + 1)
        assert c.batch.S <= span, mc.id
        ref = M.reference(mc)
        assert torch.isfinite(ref).all() and (ref.norm(dim=1) - 1).abs().max() < 1e-14, mc.id
    lens = {l for mc in M.MPNET_CASES for l in mc.case.batch.lengths}
    assert 1 in lens and {32, 64} & lens and {17, 18, 19, 20} <= lens and max(lens) >= 129
    assert set(M.FP32_DEV_MPNET) == {mc.regime for mc in M.MPNET_CASES}


def test_reference_is_transformers_and_admitted_and_the_table_holds(fp32_devs):
    worst = {}
    for mc in M.MPNET_CASES:
        for inst, v in fp32_devs[mc.id].items():
            w = worst.setdefault(mc.regime, {})
            if v > w.get(inst, (0.0, ""))[0]:
                w[inst] = (v, mc.id)
    insts = ("torch", "chunk16", "transformers")
    print("\n[encoder mpnet reference] worst fp32 deviation from fp64 per regime (max-abs on the unit vector, both poolings)")
    print(f"  {'regime':12s} {'torch fp32':>30s} {'K-chunks of 16':>30s} {'transformers fp32':>30s}   FP32_DEV_MPNET  device bound")
    for regime in sorted(worst):
        cells = "".join(f" {worst[regime][i][0]:9.1e} {worst[regime][i][1][:20]:20s}" for i in insts)
        print(f"  {regime:12s}{cells}   {M.FP32_DEV_MPNET[regime]:.0e}     {R.KERNEL_FACTOR * M.FP32_DEV_MPNET[regime]:.1e}")
    for mc in M.MPNET_CASES:
        fig = M.FP32_DEV_MPNET[mc.regime]
        # the restatement IS the installed transformers' forward: two fp32 evaluations of one function, each within the figure of
        # fp64, so within twice the figure of each other
        assert fp32_devs[mc.id]["mine - transformers"] <= 2 * fig, (mc.id, fp32_devs[mc.id])
        for inst in insts:
            v = fp32_devs[mc.id][inst]
            assert v <= R.ADMISSION * fig, (mc.id, inst, v)
            assert v <= 1.5 * fig, (mc.id, inst, v)          # (x 1.5: torch's blocked sums depend on the thread count and the CPU)
    for regime, w in worst.items():
        top = max(w[i][0] for i in insts)
        assert top > M.FP32_DEV_MPNET[regime] / 4, (regime, top)                  # ... rounded up to one digit, not padded


def test_every_mutant_is_visible_on_a_case_it_applies_to():
    best = {}
    for mc in M.MPNET_CASES:
        if not mc.case.sens:
            continue
        for name in M.MPNET_MUTANTS:
            if not M.applicable(name, mc):
                assert M.mutant_distance(mc, name) < M.device_bound(mc), (mc.id, name)      # ... and changes nothing where it does not
                continue
            d = M.mutant_distance(mc, name) / M.device_bound(mc)
            if d > best.get(name, (0.0, ""))[0]:
                best[name] = (d, mc.id)
    print("\n[encoder mpnet reference] the most visible case of every mutant, in device bounds")
    for name, (d, cid) in sorted(best.items()):
        print(f"  {name:22s} {d:10.0f} x the bound   {cid}")
    assert set(best) == set(M.MPNET_MUTANTS)
    for name, (d, cid) in best.items():
        assert d >= VISIBLE, (name, d, cid)
    # the bias mistakes are seen on the very case the GPU suite uploads wrong tables on, and by both poolings
    for pooling in ("cls", "mean"):
        mc = M.BY_ID["mp_S70_packed-" + pooling]
        for name in M.BIAS_MUTANTS:
            if M.applicable(name, mc):
                assert M.mutant_distance(mc, name) >= VISIBLE * M.device_bound(mc), (mc.id, name)
    assert M.applicable("bias_saturate_64", M.BY_ID["mp_S140_packed-cls"])


@pytest.mark.parametrize("span", [64, 514 - 2])
def test_bias_table_is_the_models_position_bias_along_every_diagonal(span):
    from adaptive_classifier import encoder as E
    heads = 12 if span > 64 else 2
    model = M.build_model(M.mpnet_config(64 * heads, 1, heads, 128, span + 2), "flat", seed=3)
    table = E.build_rel_bias(model)
    assert table.shape == (heads, 2 * span - 1) and table.dtype == torch.float32 and table.is_contiguous()
    with torch.no_grad():
        full = model.encoder.compute_position_bias(torch.zeros(1, span, 8))[0]             # [heads, span, span]: [h, i, j]
    i = torch.arange(span)[:, None]
    j = torch.arange(span)[None, :]
    assert torch.equal(table[:, (j - i) + span - 1], full)
    short = E.build_rel_bias(model, span=16)                                               # a shorter span: the middle of the table
    assert torch.equal(short, table[:, span - 16:span + 15])


# ---- the ABI -------------------------------------------------------------------------------------------------------------
def _header_struct(name):
    src = open(os.path.join(ROOT, "include", "acamd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    body = re.search(r"typedef struct \{([^}]*)\}\s*" + name + r"\s*;", src).group(1)
    return [re.sub(r"\s+", " ", d.strip()) for d in body.split(";") if d.strip()]


def test_header_and_ctypes_agree_on_the_bias_fields():
    from adaptive_classifier import _native as nv
    assert nv.lib().ac_version() >= 11
    decls = _header_struct("ac_bert_weights")
    assert decls[-2:] == ["const float* attn_rel_bias", "int rel_span"], decls[-2:]
    mirror = nv.ac_bert_weights._fields_
    assert [d.split()[-1].lstrip("*") for d in decls] == [n for n, _ in mirror]
    assert mirror[-2] == ("attn_rel_bias", ctypes.c_void_p) and mirror[-1] == ("rel_span", ctypes.c_int)
    assert all(t is ctypes.c_void_p for _, t in mirror[:-1])
    assert nv.ac_bert_weights.attn_rel_bias.offset == 8 * (len(mirror) - 2) and nv.ac_bert_weights.rel_span.offset == 8 * (len(mirror) - 1)
    zero = nv.ac_bert_weights()
    assert not zero.attn_rel_bias and zero.rel_span == 0                                   # a zero-initialised struct: no table


def test_longer_than_rel_span_is_refused_by_every_entry_and_the_workspace_ignores_the_table():
    from adaptive_classifier import _native as nv
    L = nv.lib()
    cfg = nv.ac_bert_config(128, 3, 2, 512, 2000, 64, 1, 1e-12)
    n = ctypes.c_size_t(0)
    assert L.ac_bert_workspace(ctypes.byref(cfg), 8, 33, ctypes.byref(n)) == 0              # (takes no weights: cannot depend on them)
    assert "ac_bert_weights" not in re.search(r"int ac_bert_workspace\(([^)]*)\)", open(os.path.join(ROOT, "include", "acamd.h")).read()).group(1)
    host = ctypes.create_string_buffer(4096)               # stands in for every pointer: the calls below are refused before any is read
    p = ctypes.cast(host, ctypes.c_void_p)
    w = nv.ac_bert_weights()
    w.attn_rel_bias, w.rel_span = p.value, 16
    used, total, path = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    calls = {
        "opts": lambda S: L.ac_bert_encode_cls_opts(ctypes.byref(cfg), ctypes.byref(w), p, None, None, 3, S, p, 128, p, 1 << 40, 0,
                                                    ctypes.byref(used), None),
        "plain": lambda S: L.ac_bert_encode_cls(ctypes.byref(cfg), ctypes.byref(w), p, None, None, 3, S, p, 128, p, 1 << 40, None),
        "unpad": lambda S: L.ac_bert_encode_cls_unpad(ctypes.byref(cfg), ctypes.byref(w), p, None, p, 3, S, p, 128, p, 1 << 40, 0,
                                                      ctypes.byref(total), ctypes.byref(path), None),
        "packed": lambda S: L.ac_bert_encode_cls_packed(ctypes.byref(cfg), ctypes.byref(w), p, None, 3, S, p, p, 3, 1, p, 128, p, 1 << 40,
                                                        None),
    }
    for name, call in calls.items():
        assert call(17) == -1, name                                                         # AC_EINVAL
        assert b"rel_span" in L.ac_last_error(), (name, L.ac_last_error())
    w.rel_span = 0                                                                          # a table without a span is refused too
    assert calls["opts"](1) == -1 and b"rel_span" in L.ac_last_error()


def test_biased_attention_kernels_hold_no_scratch_and_no_flat_access():
    """The device listing of csrc/bert.hip (hipcc cross-compiles without a GPU): the BIAS instantiations exist for head dims 64
    and 32, keep private_segment_fixed_size 0, address memory with global / LDS instructions only (a generic pointer to the table
    would show as flat_load), and read exactly 16 more dwords per key tile than their unbiased twins."""
    from test_kernel_resources_cpu import HIPCC, listing, kernel_resources
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    text, res = listing("bert.hip"), kernel_resources("bert.hip")

    def body(name):
        return re.search(r"^%s:[^\n]*\n(.*?)\.Lfunc_end" % re.escape(name), text, re.S | re.M).group(1)

    def one(pattern):
        names = [k for k in res if re.search(pattern, k)]
        assert len(names) == 1, (pattern, names)
        return names[0]

    for dht in (64, 32):
        biased = one(r"attention_mfma_kernelILb0ELi%dELb1EJPKfiE" % dht)
        plain = one(r"attention_mfma_kernelILb0ELi%dELb0EJEE" % dht)
        assert res[biased][0] == 0 and res[plain][0] == 0, (res[biased], res[plain])
        assert res[biased][1] <= 512
        assert not re.search(r"\b(flat|scratch)_\w+", body(biased)), biased
        loads = lambda n: len(re.findall(r"\bglobal_load_dword\b", body(n)))
        assert loads(biased) == loads(plain) + 16, (loads(biased), loads(plain))
        assert body(biased).count("v_mfma") == body(plain).count("v_mfma")
    for pattern in (r"attention_cls_kernelILb0ELi64ELi32ELb1E", r"attention_cls_kernelILb0ELi64ELi64ELb1E", r"attention_cls_kernelILb0ELi32ELi64ELb1E"):
        k = one(pattern)
        assert res[k][0] == 0 and not re.search(r"\b(flat|scratch)_\w+", body(k)), k
    # ModernBERT gets no table, and the boundary mode of the fused attention is not instantiated with one
    assert not [k for k in res if re.search(r"attention_(mfma|cls)_kernelILb1E\w*ELb1EJ", k)]


# ---- the constructor's device-free part ----------------------------------------------------------------------------------------
def test_parameter_names_resolve_a_real_state_dict():
    from adaptive_classifier import encoder as E
    from transformers import MPNetModel
    cfg = M.mpnet_config(128, 2, 2, 512, 66)
    model = MPNetModel(cfg)                                                                 # with the pooler: it is ignored
    mtype, names, pos_offset, act, (H, L, A, I), type_vocab, eps = E.HipBertEncoder.architecture(cfg)
    assert (mtype, pos_offset, act, (H, L, A, I), type_vocab) == ("mpnet", M.PAD_ID + 1, "gelu", (128, 2, 2, 512), 1)
    assert names is E.MPNET_NAMES and names["type"] is None and eps == float(cfg.layer_norm_eps)
    read = {names["word"], names["pos"], names["eln"] + ".weight", names["eln"] + ".bias", E.MPNET_REL_BIAS}
    for l in range(L):
        for part in ("q", "k", "v", "ao", "ff1", "ff2", "ln1", "ln2"):
            read |= {names["layer"].format(l) + names[part] + ".weight", names["layer"].format(l) + names[part] + ".bias"}
    sd = set(model.state_dict())
    assert read <= sd, read - sd
    left = {k for k in sd - read if not k.startswith("pooler.") and not k.endswith("position_ids")}
    assert left == set(), left                                                              # every weight of the encoder is read


def test_other_activations_and_families_are_refused():
    from adaptive_classifier import _native as nv, encoder as E
    with pytest.raises(nv.NativeError, match="relu"):
        E.HipBertEncoder.architecture(M.mpnet_config(128, 2, 2, 512, 66, hidden_act="relu"))
    from transformers import AlbertConfig
    with pytest.raises(nv.NativeError, match="MPNet.*albert"):
        E.HipBertEncoder.architecture(AlbertConfig())
    assert "MPNet" in E.make_encoder.__doc__
