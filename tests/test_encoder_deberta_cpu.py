"""No GPU: proves the DeBERTa reference of tests/encoder_deberta_ref.py and the host side of the family.

  1. the restatement: the helper's fp64 forward equals transformers' DebertaV2Model in fp64 on the compared rows -- to rounding once
     the root of 3 d is taken in fp32 the way transformers takes it, and within that root's residue with the exact one;
  2. admission: the three fp32 instances lie within ADMISSION x FP32_DEV_DEBERTA of fp64 on every case, and the constants are the
     regimes' worst figures (printed as a table);
  3. sensitivity: every mutant, on at least one case it applies to, lies at least ADMISSION device bounds from the reference;
  4. encoder.build_disentangled: one index per distance, odd and monotone, inside [1, rel_rows - 1], the model's own
     relative_pos + att_span, the tables the model's own projections, zero tables for a missing term;
  5. architecture(): the family is accepted, every unsupported key is refused by name, the name map reads every weight;
  6. the ABI: ac_version() >= 12, header and ctypes mirror agree, attn_disentangled sits directly before attn_rel_bias, a zeroed struct
     means none, every refusal is AC_EINVAL naming its field at the four encode entries before any pointer is read, the workspace
     is what it was;
  7. the device listing: the new instantiations hold no scratch and no flat access;
  8. a SentencePiece-Unigram fast tokenizer passes through maybe_device_tokenizer unchanged.
"""
import ctypes
import os
import re

import pytest
import torch

import encoder_ref as R
import encoder_deberta_ref as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# ac_bert_workspace(hidden 128, 3 layers, 2 heads, 512; b 8, S 33): csrc/bert.hip bert_ws is untouched, this is the parent commit's figure
WORKSPACE_8x33 = 2576128
SQRT32_RESIDUE = 1e-9            # transformers' fp32 root of 3 d inside a double model: measured 4e-10 at most on these cases


@pytest.fixture(scope="module")
def fp32_devs():
    torch.set_num_threads(min(16, torch.get_num_threads()))
    out = {}
    for mc in D.DEBERTA_CASES:
        mine, theirs = D.fp32_instance(mc), D.transformers_instance(mc)
        out[mc.id] = {"torch": D.deviation(mc, mine), "chunk16": D.deviation(mc, D.fp32_instance(mc, chunked=True)),
                      "transformers": D.deviation(mc, theirs), "mine - transformers": float((mine - theirs).abs().max())}
    return out


def test_case_table_is_consistent():
    ids = {mc.case.id for mc in D.DEBERTA_CASES}
    assert {"db_small_T32", "db_ragged9", "db_S40_planes", "db_S40_f32", "db_S70_flat", "db_padded_no_mask", "db_holes", "db_T_lt_4b",
            "db_noshare", "db_c2p_only", "db_p2c_only", "db_posbiased_types"} <= ids
    for mc in D.DEBERTA_CASES:
        c = mc.case
        assert not c.one_launch and c.attn_launches == 0, mc.id                   # what the position terms rule out
        assert D.device_bound(mc) <= R.DEVICE_BOUND_CEILING
        token_layers = c.model.layers if mc.pooling == "mean" else c.model.layers - 1
        assert c.ln_launches in (0, 2 * token_layers), mc.id
        tokens = c.batch.b * c.batch.S if c.tokens < 0 else c.tokens
        assert (c.ln_launches > 0) == (tokens >= 192 and c.arith is None), mc.id  # gemm_plan.h kTileMinM, bf16x3 planes
        assert tokens <= 300, mc.id
        cfg = D.make_model(c.model).config
        assert (c.model.hidden, c.model.layers, c.model.heads, c.model.inter, cfg.position_buckets) == (128, 3, 2, 512, 8)
        assert c.batch.S <= cfg.max_position_embeddings in (64, 128), mc.id
        ref = D.reference(mc)
        assert torch.isfinite(ref).all() and (ref.norm(dim=1) - 1).abs().max() < 1e-14, mc.id
    by = {mc.case.id: mc.case for mc in D.DEBERTA_CASES}
    assert by["db_small_T32"].batch.b * by["db_small_T32"].batch.S <= 32
    assert len(by["db_ragged9"].batch.lengths) == 9 and min(by["db_ragged9"].batch.lengths) == 5 and max(by["db_ragged9"].batch.lengths) == 24
    assert by["db_S40_planes"].tokens == 204 and max(by["db_S40_planes"].batch.lengths) == 40
    assert max(by["db_S70_flat"].batch.lengths) == 70
    assert by["db_T_lt_4b"].tokens < 4 * by["db_T_lt_4b"].batch.b and by["db_ragged9"].tokens >= 4 * by["db_ragged9"].batch.b
    assert {mc.pooling for mc in D.DEBERTA_CASES} == {"cls", "mean"} and {mc.case.arith for mc in D.DEBERTA_CASES} == {None, "f32"}
    assert set(D.FP32_DEV_DEBERTA) == {mc.regime for mc in D.DEBERTA_CASES}
    # a 40-token sequence walks the logarithmic buckets, to +-7
    rp = D.relative_index(D.make_model(by["db_S40_planes"].model), 40) - 8
    assert int(rp.min()) == -7 and int(rp.max()) == 7 and len(rp.unique()) == 15


def test_reference_is_transformers_in_fp64():
    worst = (0.0, 0.0)
    for mc in D.DEBERTA_CASES:
        rows = R.compared_rows(mc.case.batch)
        theirs = D.transformers_instance(mc, double=True)
        same_root = float((theirs - D._pooled(mc, sqrt32=True))[rows].abs().max())
        exact_root = float((theirs - D.reference(mc))[rows].abs().max())
        worst = (max(worst[0], same_root), max(worst[1], exact_root))
        assert same_root <= 1e-13, (mc.id, same_root)                # one function, evaluated twice in fp64
        assert exact_root <= SQRT32_RESIDUE, (mc.id, exact_root)
    print(f"\n[encoder deberta reference] transformers fp64 - reference: {worst[0]:.1e} with its fp32 root, {worst[1]:.1e} with the exact root")


def test_fp32_instances_are_admitted_and_the_table_holds(fp32_devs):
    worst = {}
    for mc in D.DEBERTA_CASES:
        for inst, v in fp32_devs[mc.id].items():
            w = worst.setdefault(mc.regime, {})
            if v > w.get(inst, (0.0, ""))[0]:
                w[inst] = (v, mc.id)
    insts = ("torch", "chunk16", "transformers")
    print("\n[encoder deberta reference] worst fp32 deviation from fp64 per regime (max-abs on the unit vector, both poolings)")
    print(f"  {'regime':8s} {'torch fp32':>30s} {'K-chunks of 16':>30s} {'transformers fp32':>30s}   FP32_DEV_DEBERTA  device bound")
    for regime in sorted(worst):
        cells = "".join(f" {worst[regime][i][0]:9.1e} {worst[regime][i][1][:20]:20s}" for i in insts)
        print(f"  {regime:8s}{cells}   {D.FP32_DEV_DEBERTA[regime]:.0e}     {R.KERNEL_FACTOR * D.FP32_DEV_DEBERTA[regime]:.1e}")
    for mc in D.DEBERTA_CASES:
        fig = D.FP32_DEV_DEBERTA[mc.regime]
        assert fp32_devs[mc.id]["mine - transformers"] <= 2 * fig, (mc.id, fp32_devs[mc.id])
        for inst in insts:
            v = fp32_devs[mc.id][inst]
            assert v <= R.ADMISSION * fig, (mc.id, inst, v)
            assert v <= 1.5 * fig, (mc.id, inst, v)          # (x 1.5: torch's blocked sums depend on the thread count and the CPU)
    for regime, w in worst.items():
        top = max(w[i][0] for i in insts)
        assert top > D.FP32_DEV_DEBERTA[regime] / 4, (regime, top)                # ... rounded up to one digit, not padded


def test_every_mutant_is_visible_on_a_case_it_applies_to():
    best = {}
    for mc in D.DEBERTA_CASES:
        if not mc.case.sens:
            continue
        for name in D.DEBERTA_MUTANTS:
            if not D.applicable(name, mc):
                assert D.mutant_distance(mc, name) < D.device_bound(mc), (mc.id, name)      # ... and changes nothing where it does not
                continue
            d = D.mutant_distance(mc, name) / D.device_bound(mc)
            if d > best.get(name, (0.0, ""))[0]:
                best[name] = (d, mc.id)
    print("\n[encoder deberta reference] the most visible case of every mutant, in device bounds")
    for name, (d, cid) in sorted(best.items()):
        print(f"  {name:22s} {d:10.0f} x the bound   {cid}")
    assert set(best) == set(D.DEBERTA_MUTANTS)
    for name, (d, cid) in best.items():
        assert d >= R.ADMISSION, (name, d, cid)
    # the mistakes the GPU suite makes on purpose are seen on the very case it makes them on, under both poolings
    for pooling in ("cls", "mean"):
        mc = D.BY_ID["db_S40_planes-" + pooling]
        for name in ("index_sign_flipped", "pos_heads_rolled", "drop_c2p", "drop_p2c"):
            assert D.mutant_distance(mc, name) >= 8 * D.device_bound(mc), (mc.id, name)


# ---- build_disentangled ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,span", [("deberta", 64), ("deberta:noshare", 40), ("deberta:c2p", 64), ("deberta:p2c", 64)])
def test_build_disentangled_is_the_models_own_table(family, span):
    from adaptive_classifier import encoder as E
    model = D.make_model(R.ModelSpec(family, 128, 3, 2, 512, "peaked", max_pos=64))
    pos_key, pos_query, rel_index, sf = E.build_disentangled(model, span)
    cfg = model.config
    att = model.encoder.layer[0].attention.self
    A, rows = int(att.pos_ebd_size), 2 * int(att.pos_ebd_size)
    terms = D._terms(cfg)
    assert sf == 1 + len(terms) and len(pos_key) == len(pos_query) == cfg.num_hidden_layers
    assert rel_index.dtype == torch.int32 and rel_index.shape == (2 * span - 1,) and rel_index.is_contiguous()
    # one index per distance (d = key - query), odd about att_span, monotone (falling in d = rising in i - j), inside [1, rows - 1]
    centred = rel_index.long() - A
    assert torch.equal(centred, -torch.flip(centred, dims=[0])) and int(centred[span - 1]) == 0
    assert bool((centred[1:] <= centred[:-1]).all())
    assert 1 <= int(rel_index.min()) and int(rel_index.max()) <= rows - 1
    # ... and the model's own relative_pos + att_span, for both terms: c2p reads clamp(rp + A), p2c clamp(-rp^T + A) transposed
    i = torch.arange(span)
    probe = torch.zeros(1, span, 1)
    rp = model.encoder.get_rel_pos(probe)[0]                                               # [span, span] = bucket(i - j)
    table = rel_index.long()[(i[None, :] - i[:, None]) + span - 1]                         # [i, j] -> d = j - i
    assert torch.equal(table, (rp + A).clamp(0, rows - 1))
    assert torch.equal(table, ((-rp + A).clamp(0, rows - 1)).t())                          # p2c's index at key row j, transposed
    # the tables: the layer's own projection of the model's own rel embeddings, in fp32 within rounding; zero for a missing term
    with torch.no_grad():
        rel = model.encoder.get_rel_embedding()[:rows]
        for l, layer in enumerate(model.encoder.layer):
            s = layer.attention.self
            for term, got, proj in (("c2p", pos_key[l], s.key_proj if s.share_att_key else getattr(s, "pos_key_proj", None)),
                                    ("p2c", pos_query[l], s.query_proj if s.share_att_key else getattr(s, "pos_query_proj", None))):
                assert got.shape == (rows, cfg.hidden_size) and got.dtype == torch.float32 and got.is_contiguous()
                if term not in terms:
                    assert not got.any(), (l, term)
                else:
                    want = proj(rel)
                    assert float((got - want).abs().max()) <= 1e-5 * float(want.abs().max()), (l, term)
    short = E.build_disentangled(model, 16)[2]
    assert torch.equal(short, rel_index[span - 16:span + 15])                              # a shorter span: the middle of the table


# ---- architecture() ------------------------------------------------------------------------------------------------------------
def test_architecture_accepts_the_family_and_reads_every_weight():
    from adaptive_classifier import encoder as E
    for family in D.VARIANTS:
        model = D.make_model(R.ModelSpec(family, 128, 3, 2, 512, "peaked", max_pos=64))
        cfg = model.config
        mtype, names, pos_offset, act, (H, L, A, I), type_vocab, eps = E.HipBertEncoder.architecture(cfg)
        assert (mtype, pos_offset, act, (H, L, A, I)) == ("deberta-v2", 0, "gelu", (128, 3, 2, 512))
        assert eps == float(cfg.layer_norm_eps) and type_vocab == max(1, cfg.type_vocab_size)
        assert (names["type"] is None) == (cfg.type_vocab_size == 0) and (names["pos"] is None) == (not cfg.position_biased_input)
        assert E.deberta_rel_span(cfg) == 64
        read = {names["word"], names["eln"] + ".weight", names["eln"] + ".bias", "encoder.rel_embeddings.weight",
                "encoder.LayerNorm.weight", "encoder.LayerNorm.bias"} | {names[k] for k in ("pos", "type") if names[k]}
        for l in range(L):
            parts = ["q", "k", "v", "ao", "ff1", "ff2", "ln1", "ln2"]
            for part in parts:
                read |= {names["layer"].format(l) + names[part] + ".weight", names["layer"].format(l) + names[part] + ".bias"}
            if not cfg.share_att_key:
                for proj in ("pos_key_proj", "pos_query_proj"):
                    read |= {f"encoder.layer.{l}.attention.self.{proj}.weight", f"encoder.layer.{l}.attention.self.{proj}.bias"}
        sd = set(model.state_dict())
        assert read <= sd, read - sd
        assert {k for k in sd - read if not k.endswith("position_ids")} == set()             # every weight of the encoder is read
    import copy
    cfg = copy.deepcopy(D.make_model(R.ModelSpec("deberta", 128, 3, 2, 512, "peaked", max_pos=64)).config)
    cfg.max_relative_positions = 48
    assert E.deberta_rel_span(cfg) == 48
    assert "DeBERTa" in E.make_encoder.__doc__


@pytest.mark.parametrize("change,key", [
    ({"embedding_size": 64}, "embedding_size"), ({"conv_kernel_size": 3}, "conv_kernel_size"), ({"relative_attention": False}, "relative_attention"),
    ({"pos_att_type": ["c2p", "p2p"]}, "pos_att_type.*p2p"), ({"num_attention_heads": 4}, "num_attention_heads"),
    ({"hidden_act": "gelu_new"}, "gelu_new")])
def test_architecture_refuses_each_unsupported_key_by_name(change, key):
    from adaptive_classifier import _native as nv, encoder as E
    with pytest.raises(nv.NativeError, match=key):
        E.HipBertEncoder.architecture(D.deberta_config(128, 3, 2, 512, 64, **change))


def test_deberta_v1_and_other_families_are_refused():
    from adaptive_classifier import _native as nv, encoder as E
    from transformers import AlbertConfig, DebertaConfig
    with pytest.raises(nv.NativeError, match="v1.*different block"):
        E.HipBertEncoder.architecture(DebertaConfig())
    with pytest.raises(nv.NativeError, match="DeBERTa-v2/v3.*albert"):
        E.HipBertEncoder.architecture(AlbertConfig())


# ---- the ABI -------------------------------------------------------------------------------------------------------------
def _header_struct(name):
    src = open(os.path.join(ROOT, "include", "acamd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    body = re.search(r"typedef struct \{([^}]*)\}\s*" + name + r"\s*;", src).group(1)
    return [re.sub(r"\s+", " ", d.strip()) for d in body.split(";") if d.strip()]


def test_header_and_ctypes_agree_on_the_new_struct_and_field():
    from adaptive_classifier import _native as nv
    assert nv.lib().ac_version() >= 12
    decls = _header_struct("ac_bert_weights")
    assert decls[-3:] == ["const ac_bert_disentangled* attn_disentangled", "const float* attn_rel_bias", "int rel_span"], decls[-3:]
    mirror = nv.ac_bert_weights._fields_
    assert [d.split()[-1].lstrip("*") for d in decls] == [n for n, _ in mirror]
    assert mirror[-3] == ("attn_disentangled", ctypes.c_void_p)
    assert nv.ac_bert_weights.attn_disentangled.offset == nv.ac_bert_weights.attn_rel_bias.offset - 8 == 8 * (len(mirror) - 3)
    zero = nv.ac_bert_weights()
    assert not zero.attn_disentangled                                                       # a zero-initialised struct: none
    d = _header_struct("ac_bert_disentangled")
    assert d == ["const float* const* pos_key", "const float* const* pos_query", "const int32_t* rel_index",
                 "int rel_rows, rel_span, scale_factor", "void* scratch", "size_t scratch_bytes"], d
    assert nv.ac_bert_disentangled._fields_ == [("pos_key", ctypes.c_void_p), ("pos_query", ctypes.c_void_p), ("rel_index", ctypes.c_void_p),
                                                ("rel_rows", ctypes.c_int), ("rel_span", ctypes.c_int), ("scale_factor", ctypes.c_int),
                                                ("scratch", ctypes.c_void_p), ("scratch_bytes", ctypes.c_size_t)]
    assert ctypes.sizeof(nv.ac_bert_disentangled) == 56 and nv.ac_bert_disentangled.scratch.offset == 40
    assert _header_struct("ac_bert_config")[-1] == "int pool_opt"                           # untouched


def test_every_refusal_names_its_field_at_every_entry_and_the_workspace_is_what_it_was():
    from adaptive_classifier import _native as nv
    L = nv.lib()
    cfg = nv.ac_bert_config(128, 3, 2, 512, 2000, 64, 1, 1e-7)
    n = ctypes.c_size_t(0)
    assert L.ac_bert_workspace(ctypes.byref(cfg), 8, 33, ctypes.byref(n)) == 0 and n.value == WORKSPACE_8x33
    assert "ac_bert_weights" not in re.search(r"int ac_bert_workspace\(([^)]*)\)", open(os.path.join(ROOT, "include", "acamd.h")).read()).group(1)
    host = ctypes.create_string_buffer(4096)               # stands in for every pointer: the calls below are refused before any is read
    p = ctypes.cast(host, ctypes.c_void_p)
    b, S_ok, S_long = 3, 16, 33
    need = ctypes.c_size_t(0)
    assert L.ac_bert_disentangled_scratch(ctypes.byref(cfg), 16, b, S_ok, ctypes.byref(need)) == 0
    assert need.value >= 2 * b * S_ok * 2 * (2 * S_ok - 1) * 4                             # both terms, every reachable distance
    assert L.ac_bert_disentangled_scratch(ctypes.byref(cfg), 16, 0, S_ok, ctypes.byref(n)) == 0 and n.value == 0

    def struct(**kw):
        d = nv.ac_bert_disentangled(p.value, p.value, p.value, 16, 32, 3, p.value, need.value)
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    used, total, path = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)

    def entries(cfg, w, S):
        return {
            "opts": lambda: L.ac_bert_encode_cls_opts(ctypes.byref(cfg), ctypes.byref(w), p, None, None, b, S, p, 128, p, 1 << 40, 0,
                                                      ctypes.byref(used), None),
            "plain": lambda: L.ac_bert_encode_cls(ctypes.byref(cfg), ctypes.byref(w), p, None, None, b, S, p, 128, p, 1 << 40, None),
            "unpad": lambda: L.ac_bert_encode_cls_unpad(ctypes.byref(cfg), ctypes.byref(w), p, None, p, b, S, p, 128, p, 1 << 40, 0,
                                                        ctypes.byref(total), ctypes.byref(path), None),
            "packed": lambda: L.ac_bert_encode_cls_packed(ctypes.byref(cfg), ctypes.byref(w), p, None, b, S, p, p, b, 1, p, 128, p, 1 << 40,
                                                          None),
        }

    cfg4 = nv.ac_bert_config(128, 3, 4, 512, 2000, 64, 1, 1e-7)                             # head dim 32
    refusals = [("S > rel_span", cfg, struct(), S_long, False, b"rel_span"),
                ("rel_span 0", cfg, struct(rel_span=0), S_ok, False, b"rel_span"),
                ("NULL pos_key", cfg, struct(pos_key=None), S_ok, False, b"pos_key"),
                ("NULL pos_query", cfg, struct(pos_query=None), S_ok, False, b"pos_query"),
                ("NULL rel_index", cfg, struct(rel_index=None), S_ok, False, b"rel_index"),
                ("rel_rows 0", cfg, struct(rel_rows=0), S_ok, False, b"rel_rows"),
                ("scale_factor 4", cfg, struct(scale_factor=4), S_ok, False, b"scale_factor"),
                ("short scratch", cfg, struct(scratch_bytes=need.value - 1), S_ok, False, b"scratch_bytes"),
                ("NULL scratch", cfg, struct(scratch=None), S_ok, False, b"scratch_bytes"),
                ("both tables", cfg, struct(), S_ok, True, b"attn_rel_bias"),
                ("head dim 32", cfg4, struct(), S_ok, False, b"head dim")]
    for what, c, d, S, bias, field in refusals:
        w = nv.ac_bert_weights()
        w.attn_disentangled = ctypes.addressof(d)
        if bias:
            w.attn_rel_bias, w.rel_span = p.value, 64
        for name, call in entries(c, w, S).items():
            assert call() == -1, (what, name)                                               # AC_EINVAL
            assert field in L.ac_last_error(), (what, name, L.ac_last_error())


def test_workspace_ignores_the_struct_and_the_sizing_scales():
    """ac_bert_workspace takes no weights, so it cannot see the struct; the scratch is sized by its own call, quadratic in S."""
    from adaptive_classifier import _native as nv
    L = nv.lib()
    cfg = nv.ac_bert_config(768, 12, 12, 3072, 2000, 512, 1, 1e-7)
    a, c = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert L.ac_bert_disentangled_scratch(ctypes.byref(cfg), 512, 256, 32, ctypes.byref(a)) == 0
    assert L.ac_bert_disentangled_scratch(ctypes.byref(cfg), 512, 16, 512, ctypes.byref(c)) == 0
    assert a.value == 2 * 256 * 32 * 12 * 64 * 4 and c.value == 2 * 16 * 512 * 12 * 1024 * 4
    assert L.ac_bert_disentangled_scratch(ctypes.byref(cfg), 0, 1, 8, ctypes.byref(a)) == -1 and b"rel_rows" in L.ac_last_error()
    cfg32 = nv.ac_bert_config(384, 6, 12, 1536, 2000, 512, 1, 1e-7)
    assert L.ac_bert_disentangled_scratch(ctypes.byref(cfg32), 512, 1, 8, ctypes.byref(a)) == -1 and b"head dim" in L.ac_last_error()




# ---- the device listing --------------------------------------------------------------------------------------------------------
def test_new_kernels_hold_no_scratch_and_no_flat_access():
    """The device listing of csrc/bert.hip (hipcc cross-compiles without a GPU): position_scores_kernel and the PosScores
    instantiations of the two attention kernels keep private_segment_fixed_size 0 and address memory with global / LDS instructions
    only; the tile kernel reads exactly 32 more dwords per key tile than its plain twin (16 c2p + 16 p2c) on the same MFMAs, and the
    position scores are 32 MFMAs (K = 64 in steps of 2)."""
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

    tile = one(r"attention_mfma_kernelILb0ELi64ELb0EJN6acattn9PosScoresEEE")
    plain = one(r"attention_mfma_kernelILb0ELi64ELb0EJEE")
    loads = lambda n: len(re.findall(r"\bglobal_load_dword\b", body(n)))
    assert loads(tile) == loads(plain) + 32, (loads(tile), loads(plain))
    assert body(tile).count("v_mfma") == body(plain).count("v_mfma")
    scores = one(r"position_scores_kernel")
    assert body(scores).count("v_mfma_f32_32x32x2") == 32
    for k in (tile, scores, one(r"attention_cls_kernelILb0ELi64ELi32ELb0EJN6acattn9PosScoresEEE"),
              one(r"attention_cls_kernelILb0ELi64ELi64ELb0EJN6acattn9PosScoresEEE")):
        assert res[k][0] == 0 and res[k][1] <= 512, (k, res[k])
        assert not re.search(r"\b(flat|scratch)_\w+", body(k)), k
    # nothing else takes the position scores: no RoPE, no head dim 32, no biased instantiation
    assert len([k for k in res if "PosScores" in k]) == 3


# ---- the tokenizer ---------------------------------------------------------------------------------------------------------------
def test_a_unigram_tokenizer_passes_through_unchanged():
    from tokenizers import Tokenizer, models, pre_tokenizers
    from transformers import PreTrainedTokenizerFast
    from adaptive_classifier.tokenizer import maybe_device_tokenizer
    vocab = [("[PAD]", 0.0), ("[CLS]", 0.0), ("[SEP]", 0.0), ("[UNK]", 0.0)] + [(chr(0x2581) + w, -float(i + 1)) for i, w in enumerate(
        ("great", "product", "awful", "fine"))] + [(ch, -20.0) for ch in "abcdefghijklmnopqrstuvwxyz" + chr(0x2581)]
    tok = Tokenizer(models.Unigram(vocab, unk_id=3))
    tok.pre_tokenizer = pre_tokenizers.Metaspace()
    fast = PreTrainedTokenizerFast(tokenizer_object=tok, pad_token="[PAD]", cls_token="[CLS]", sep_token="[SEP]", unk_token="[UNK]")
    assert maybe_device_tokenizer(fast, "cpu") is fast
    enc = fast(["great product", "fine"], padding=True, return_tensors="pt")
    assert enc["input_ids"].shape[0] == 2 and int(enc["attention_mask"].sum()) < enc["attention_mask"].numel()
