"""Shared by tests/test_encoder_f16x2_cpu.py and tests/test_encoder_f16x2_gpu.py: the opt-in fp16x2 arithmetic of the BERT-path
encoder (include/acamd.h AC_GEMM_F16X2) stated on top of the four reference modules -- tests/encoder_ref.py, encoder_pool_ref.py,
encoder_mpnet_ref.py, encoder_deberta_ref.py.  Their forwards, models, batches, case grids, fp64 references and device bounds are
imported, never edited; the one thing they grew for this file is the `lin_mm` hook of their forwards.

Which layer of the evidence this is: tests/test_f16x2_model_cpu.py states what ONE product promises a priori,
tests/test_gemm_f16x2_gpu.py holds ONE GEMM to it per element against fp64 (and the encoder to the 1e-4 contract on one batch);
this file and its two test modules hold the WHOLE ENCODER in that arithmetic to fp64 on every dispatch branch and family -- the
embedding, the fused and the stand-alone attention emitting planes, both LayerNorm forms, the K|V GEMM of the last layer, mean
pooling -- with a statistic that sees one lost low plane at one GEMM of one layer.

  the fp16x2 instance   the module's fp32 forward with `lin_mm` = the three-product form of tests/test_f16x2_model_cpu.py: every
               nn.Linear operand split into h = fp16(x 2^s), l = fp16(x 2^s - h) (s = 6 activations, 10 weights), products
               la.hw + ha.lw + ha.hw summed in fp32 with encoder_ref.mm_chunk16, scaled by 2^-16.  Applied to EVERY layer; the
               device keeps the CLS-only tail of the last layer (attention output, FFN on the b CLS rows) in bf16x3, which is
               more accurate, so the instance is the coarser of the two.  Attention scores / P.V, MPNet's bias and DeBERTa's
               position projections keep the fp32 `mm`: on the device they run on fp32 `qkv`.
  mutants      F16_MUTANTS: switches on that instance, each a plausible kernel mistake (a low plane lost at one GEMM, at all of
               them, a truncating split, a wrong scale) and one harmless change (the l.l product added).
  cases        F16_CASES: derived from the four grids, no second grid -- see _derive().  Every case keeps its env, ln_fusion,
               unpad, ldo_extra, max_tokens, path and counters; `arith` becomes "f16x2".
  yardstick    rms_yard(case) = the largest rms deviation from fp64, over the compared rows, of four CORRECT instances: the
               module's three fp32 instances and the fp16x2 instance.  The device is held to RMS_FACTOR x it, beside the grid's
               own max-abs device bound.  F16X2_DEV = the worst max-abs deviation of the fp16x2 instance per group, a table
               like FP32_DEV.  No bound comes from a device observation.
  counter      f16_launches(case) = what ac_gemm_f16x2_launches must grow by: 4 (L - 1) + 1 under CLS pooling (the + 1: the last
               layer's QKV GEMM, or its K|V GEMM when T >= 4 b), 4 L under mean pooling, 0 for a call that falls back to bf16x3.

Why rms and not max-abs (measured with these functions on the CPU, tests/test_encoder_f16x2_cpu.py prints the table): the low
plane of one operand lost at ONE GEMM of ONE layer moves the unit vector by 0.2 .. 23 max-abs device bounds -- 83 of the 646
(case, mutant) pairs pass that bound -- but by 11 yardsticks or more in rms; lost at every GEMM it moves the vector by 9.2e-5 on
T192_all_fused, less than the 1e-4 contract of tests/test_gemm_f16x2_gpu.py.
"""
import dataclasses
import functools
import re

import torch

import encoder_ref as R
import encoder_pool_ref as P
import encoder_mpnet_ref as M
import encoder_deberta_ref as D

ACT_LOG2, W_LOG2 = 6, 10          # csrc/common.h kF16ActLog2 / kF16WLog2; tests/test_f16x2_model_cpu.py
ACT_MAX, W_MAX = 1023.0, 63.9     # the fp16 range at those scales (include/acamd.h)
RANGE_MARGIN = 4                  # every F16 case keeps its operands this factor inside the range (a condition, not a measurement)

# The device's rms deviation from fp64 may be RMS_FACTOR x rms_yard(case).  3 is the factor
# test_encoder_under_f16x2_matches_transformers (tests/test_gemm_f16x2_gpu.py) applies to the same statistic.  Its ceiling is half
# the weakest harmful single-site mutant ratio of tests/test_encoder_f16x2_cpu.py (asserted there: every one >= 2 x RMS_FACTOR).
RMS_FACTOR = 3

SITES = ("qkv", "ao", "ff1", "ff2")
_SITE_LEAVES = (
    ("ao", ("attention.output.dense", "attention.out_lin", "attention.attn.o")),
    ("qkv", ("query", "key", "value", "q_lin", "k_lin", "v_lin", "attn.q", "attn.k", "attn.v", "query_proj", "key_proj", "value_proj")),
    ("ff1", ("intermediate.dense", "ffn.lin1")),
    ("ff2", ("output.dense", "ffn.lin2")),
)


def site_of(name):
    """parameter prefix of an nn.Linear of a BERT-block family -> (site, layer)"""
    layer = int(re.search(r"\.(\d+)\.", name).group(1))
    for site, leaves in _SITE_LEAVES:
        if any(name.endswith("." + leaf) for leaf in leaves):
            return site, layer
    raise KeyError(name)


# ------------------------------------------------------------------------------------------------------------------------
# mutants: name -> (harmful?, what the mistake is)
# ------------------------------------------------------------------------------------------------------------------------
SINGLE_LAYERS = (0, 1)
F16_MUTANTS = {}
for _op, _what in (("a", "activation"), ("w", "weight")):
    for _site in SITES:
        for _layer in SINGLE_LAYERS:
            F16_MUTANTS[f"lo_{_op}_lost[{_site},{_layer}]"] = (True, f"the low plane of the {_what} operand zeroed at layer {_layer}'s {_site} GEMM only")
F16_MUTANTS.update({
    "lo_a_lost_all":  (True, "the low plane of the activation operand zeroed at every GEMM"),
    "lo_w_lost_all":  (True, "the low plane of the weight operand zeroed at every GEMM"),
    "hh_only":        (True, "both low planes zeroed at every GEMM: the h.h product alone"),
    # the producers split at 2^10 while the GEMM epilogues still scale by 2^-(6 + 10): every product 16 x too large
    "act_scale_2^10": (True, "activations split at the weights' scale 2^10, the epilogue's 2^-16 unchanged"),
    # h by truncation, l = fp16(x - h) by rounding: the pair still holds x to 2^-21 (a bit less than the 2^-22 of the rounding
    # split), which an fp32 dot product of K >= 8 loses anyway -- a priori not a harmful mistake, so its distance is printed, not
    # asserted
    "split_truncates": (None, "h taken by truncation instead of round-to-nearest-even"),
    "ll_added":       (False, "the l.l product added as a fourth term: harmless (2^-22 of a product)"),
})
SINGLES = tuple(n for n in F16_MUTANTS if "[" in n)


def split(x, log2, truncate=False):
    """x (any float tensor) -> h, l as fp32 tensors: h = fp16(x 2^log2), l = fp16(x 2^log2 - h); tests/test_f16x2_model_cpu.py's
    `split` in torch (the CPU test holds the two equal bit for bit).  truncate: h rounded toward zero."""
    xs = x.float() * 2.0 ** log2
    h = xs.half()
    if truncate:
        cut = torch.bitwise_and(xs.contiguous().view(torch.int32), -8192).view(torch.float32)      # 13 low bits: 11 significant left
        h = torch.where(xs.abs() < 2.0 ** -14, h.float(), cut).half()                             # (fp16 subnormals: left rounded)
    l = (xs - h.float()).half()
    return h.float(), l.float()


def f16x2_lin_mm(mut=(), cls_tail_layer=None):
    """the `lin_mm` hook of the fp16x2 instance with the mistakes of `mut`.  cls_tail_layer: that layer's query projection,
    attention output and FFN run in plain fp32 -- what the device's CLS-only last layer does with a call of T >= 4 b (bf16x3 on the b
    CLS rows; only its K|V GEMM is an fp16x2 one).  For comparing a mistake MADE on the device with the same one made here."""
    mut = frozenset(mut)
    assert mut <= set(F16_MUTANTS), mut
    trunc = "split_truncates" in mut
    a_log2 = W_LOG2 if "act_scale_2^10" in mut else ACT_LOG2

    def lin_mm(t, w_t, name):
        site, layer = site_of(name)
        if layer == cls_tail_layer and (site != "qkv" or name.endswith(("query", "q_lin", "attn.q", "query_proj"))):
            return t @ w_t
        ha, la = split(t, a_log2, trunc)
        hw, lw = split(w_t, W_LOG2, trunc)
        if mut & {"lo_a_lost_all", "hh_only", f"lo_a_lost[{site},{layer}]"}:
            la = torch.zeros_like(la)
        if mut & {"lo_w_lost_all", "hh_only", f"lo_w_lost[{site},{layer}]"}:
            lw = torch.zeros_like(lw)
        acc = R.mm_chunk16(la, hw) + R.mm_chunk16(ha, lw) + R.mm_chunk16(ha, hw)
        if "ll_added" in mut:
            acc = acc + R.mm_chunk16(la, lw)
        return (acc * 2.0 ** -(ACT_LOG2 + W_LOG2)).to(t.dtype)
    return lin_mm


# ------------------------------------------------------------------------------------------------------------------------
# the cases
# ------------------------------------------------------------------------------------------------------------------------
F16_BRANCHES = {"attn_fused", "attn_fused_boundary", "attn_standalone", "ln_fused", "planes_unfused", "padded_mask_planes"}
# calls that must fall back to bf16x3 as a whole: fewer than 192 token rows, or a family without fp16 weight planes
FALLBACK_BERT = ("T191_no_planes", "T150_of_100x2")
FALLBACK_MPNET = ("mp_S20_no_planes",)
FALLBACK_DEBERTA = ("db_ragged9",)
FALLBACK_MODERNBERT = ("mb_S40_planes_packed",)            # HipModernBertEncoder.encode_cls: "f16x2" runs as bf16x3


@dataclasses.dataclass(frozen=True)
class F16Case:
    grid: str                       # "bert" | "pool" | "mpnet" | "deberta": the module whose reference, instances and bound apply
    case: R.Case                    # the grid's case with arith="f16x2"
    pooling: str                    # "cls" | "mean"
    src: object                     # the grid's own record (R.Case of CASES / POOL_CASES, MPCase, DBCase): the key of its caches
    fallback: bool = False          # the whole call runs as bf16x3: 0 fp16x2 launches, the bits of arith="bf16x3"

    @property
    def id(self):
        return f"{self.case.id}-{self.pooling}"

    @property
    def family(self):
        return self.case.model.family.split(":")[0]

    @property
    def group(self):
        """the key of F16X2_DEV: the bound's group in its own module"""
        if self.grid in ("bert", "pool"):
            return ("cls" if self.grid == "bert" else "mean", self.family, self.case.model.regime)
        return ("cls+mean", self.family, self.case.model.regime)

    @property
    def sens(self):
        return self.case.sens


def _f16(c):
    assert c.arith is None, c.id
    return dataclasses.replace(c, arith="f16x2")


def _derive():
    out = []
    takes = lambda c: c.model.family in R.BERT_FAMILIES and c.arith is None and c.branch in F16_BRANCHES
    out += [F16Case("bert", _f16(c), "cls", c) for c in R.CASES if takes(c)]
    out += [F16Case("pool", _f16(c), "mean", c) for c in P.POOL_CASES if takes(c)]
    # MPNet / DeBERTa: planes=True is what gives a case its LayerNorm-fused launches (their add())
    out += [F16Case("mpnet", _f16(mc.case), mc.pooling, mc) for mc in M.MPNET_CASES if mc.case.ln_launches and mc.case.arith is None]
    out += [F16Case("deberta", _f16(mc.case), mc.pooling, mc) for mc in D.DEBERTA_CASES if mc.case.ln_launches and mc.case.arith is None]
    out += [F16Case("bert", _f16(R.BY_ID[i]), "cls", R.BY_ID[i], fallback=True) for i in FALLBACK_BERT + FALLBACK_MODERNBERT]
    out += [F16Case("mpnet", _f16(mc.case), mc.pooling, mc, fallback=True) for mc in M.MPNET_CASES if mc.case.id in FALLBACK_MPNET]
    out += [F16Case("deberta", _f16(mc.case), mc.pooling, mc, fallback=True) for mc in D.DEBERTA_CASES if mc.case.id in FALLBACK_DEBERTA]
    return out


F16_CASES = _derive()
BY_ID = {fc.id: fc for fc in F16_CASES}
assert len(BY_ID) == len(F16_CASES)
RUN_CASES = [fc for fc in F16_CASES if not fc.fallback]          # the cases whose token-row GEMMs run in fp16x2


def f16_launches(fc):
    """what ac_gemm_f16x2_launches grows by over the case's call (every case runs ONE chunk in fp16x2: chunks_fused_then_not's
    second chunk has 160 rows and falls back)"""
    if fc.fallback:
        return 0
    L = fc.case.model.layers
    return 4 * L if fc.pooling == "mean" else 4 * (L - 1) + 1


# ------------------------------------------------------------------------------------------------------------------------
# evaluation (cached per input: many cases share a model and a batch and differ only in how the device is called)
# ------------------------------------------------------------------------------------------------------------------------
def reference(fc):
    """fp64 unit-norm vectors [b, H] of the case under its pooling (the grid's own, shared; do not modify)"""
    return {"bert": R.reference, "pool": P.pooled_reference, "mpnet": M.reference, "deberta": D.reference}[fc.grid](fc.src)


def device_bound(fc):
    """the grid's own max-abs device bound: the correct fp16x2 model sits inside the fp32 figure, no new factor"""
    return {"bert": R.device_bound, "pool": P.device_bound, "mpnet": M.device_bound, "deberta": D.device_bound}[fc.grid](fc.src)


def fp32_figure(fc):
    """the grid's measured fp32 figure of the case's group (FP32_DEV and its siblings)"""
    c = fc.case
    return {"bert": lambda: R.FP32_DEV[c.group], "pool": lambda: P.FP32_DEV_POOL[c.group],
            "mpnet": lambda: M.FP32_DEV_MPNET[c.model.regime], "deberta": lambda: D.FP32_DEV_DEBERTA[c.model.regime]}[fc.grid]()


def _input(fc):
    """what the CPU figures of a case depend on: many cases share it and differ only in how the device is called"""
    return (_kind(fc), fc.case.model, fc.case.batch, fc.pooling, fc.case.path == "packed")


_FP32, _YARD = {}, {}


def _fp32_instances(grid, src):
    if grid == "bert":
        return R.fp32_instance(src), R.fp32_instance(src, chunked=True), R.transformers_fp32(src)
    if grid == "pool":
        return P.fp32_instance(src), P.fp32_instance(src, chunked=True), P.transformers_fp32(src)
    if grid == "mpnet":
        return M.fp32_instance(src), M.fp32_instance(src, chunked=True), M.transformers_fp32(src)
    return D.fp32_instance(src), D.fp32_instance(src, chunked=True), D.transformers_instance(src)


def fp32_instances(fc):
    """the module's three fp32 instances: torch fp32, K-chunks of 16, transformers fp32"""
    if _input(fc) not in _FP32:
        _FP32[_input(fc)] = _fp32_instances(fc.grid, fc.src)
    return dict(zip(("torch", "chunk16", "transformers"), _FP32[_input(fc)]))


@functools.lru_cache(maxsize=None)
def _forward(kind, m, bs, pooling, packed, dtype, lin_mm_key, cls_tail=False):
    """kind "bert" | "mpnet" | "deberta"; lin_mm_key: a tuple of mutants (the fp16x2 instance with them), or "range" (the operand
    magnitudes of every nn.Linear, returned beside the vectors); cls_tail: f16x2_lin_mm's cls_tail_layer = the last layer"""
    seen = {"a": 0.0, "w": 0.0}

    def ranged(t, w_t, name):
        site_of(name)
        seen["a"], seen["w"] = max(seen["a"], float(t.abs().max())), max(seen["w"], float(w_t.abs().max()))
        return t @ w_t

    lin_mm = ranged if lin_mm_key == "range" else f16x2_lin_mm(lin_mm_key, m.layers - 1 if cls_tail else None)
    ids, types, mask = R.make_batch(bs)
    if kind == "bert":
        if pooling == "cls":
            out = R._run(m, bs, dtype=dtype, lin_mm=lin_mm)
        else:
            out = P.pool(m, bs, P._last_hidden(m, bs, dtype, R.mm_plain, lin_mm))
    else:
        hs = []
        if kind == "mpnet":
            out = M.mpnet_forward(M.make_model(m), ids, mask, dtype=dtype, hidden_out=hs, packed=packed, lin_mm=lin_mm)
        else:
            out = D.deberta_forward(D.make_model(m), ids, types, mask, dtype=dtype, hidden_out=hs, lin_mm=lin_mm)
        if pooling == "mean":
            adm = torch.ones((bs.b, bs.S), dtype=torch.bool) if mask is None else mask.bool()
            out = P.masked_mean_normalize(hs[-1], adm)
    return (out, dict(seen)) if lin_mm_key == "range" else out


def _kind(fc):
    return "bert" if fc.grid in ("bert", "pool") else fc.grid


def f16x2_instance(fc, mut=(), cls_tail=False):
    """the fp16x2 instance of the case (module docstring) with the mistakes of `mut`; cls_tail: the last layer's CLS tail in fp32
    as on the device (CLS pooling, T >= 4 b)"""
    c = fc.case
    tokens = c.batch.b * c.batch.S if c.tokens < 0 else c.tokens
    assert not cls_tail or (fc.pooling == "cls" and tokens >= 4 * c.batch.b), fc.id
    return _forward(_kind(fc), c.model, c.batch, fc.pooling, c.path == "packed", torch.float32, tuple(sorted(mut)), cls_tail)


def operand_range(fc):
    """{"a": largest |activation operand|, "w": largest |weight|} over every nn.Linear of the fp64 forward"""
    c = fc.case
    out, seen = _forward(_kind(fc), c.model, c.batch, fc.pooling, c.path == "packed", torch.float64, "range")
    assert float((out - reference(fc))[R.compared_rows(c.batch)].abs().max()) == 0.0, fc.id           # the hook changed nothing
    return seen


def deviation(fc, got):
    """max-abs difference of `got` [b, H] from the fp64 reference over the compared rows"""
    rows = R.compared_rows(fc.case.batch)
    return float((got.detach().double().cpu() - reference(fc))[rows].abs().max())


def rms(fc, got):
    """rms difference of `got` [b, H] from the fp64 reference over the compared rows"""
    rows = R.compared_rows(fc.case.batch)
    return float((got.detach().double().cpu() - reference(fc))[rows].pow(2).mean().sqrt())


def rms_yard(fc):
    """the largest rms deviation from fp64 of four correct instances: the three fp32 ones and the fp16x2 one (CPU only)"""
    if _input(fc) not in _YARD:
        _YARD[_input(fc)] = max([rms(fc, v) for v in fp32_instances(fc).values()] + [rms(fc, f16x2_instance(fc))])
    return _YARD[_input(fc)]


def mutant_ratio(fc, name):
    """rms distance of the mutant from fp64, in yardsticks"""
    return rms(fc, f16x2_instance(fc, (name,))) / rms_yard(fc)


# ------------------------------------------------------------------------------------------------------------------------
# bounds
# ------------------------------------------------------------------------------------------------------------------------
# F16X2_DEV[group]: worst max-abs deviation from fp64 of the fp16x2 instance over the group's RUN_CASES, measured on the CPU and
# rounded up to one digit.  tests/test_encoder_f16x2_cpu.py asserts every case stays within 1.5 x its group's figure, that no
# figure exceeds encoder_ref.ADMISSION x the group's fp32 figure (FP32_DEV and its siblings: then the grid's own device bound,
# 16 x that figure, still holds the fp16x2 device with a factor 4 to spare), and prints this table.  The worst cases at the time
# of writing (8 CPU threads); no group needed the ADMISSION factor -- every figure is at or below its group's fp32 figure:
#
#   pooling   family       regime        fp16x2 instance                       F16X2_DEV   fp32 figure of the group
#   cls       bert         flat          7.1e-08 sa_longest32-cls              8e-8        9e-8
#   cls       bert         peaked        1.3e-07 sa_dh32_longest33-cls         2e-7        3e-7
#   cls       bert         peaked_wide   1.7e-07 ln_1024_ragged_panel-cls      2e-7        3e-7
#   cls       distilbert   peaked        8.1e-08 distilbert_packed-cls         9e-8        2e-7
#   cls       electra      peaked        8.0e-08 electra_packed-cls            9e-8        2e-7
#   cls       roberta      flat          6.7e-08 roberta_packed-cls            7e-8        8e-8
#   cls       xlm-roberta  flat          6.7e-08 xlm-roberta_packed-cls        7e-8        8e-8
#   mean      bert         peaked        1.1e-07 attn_straddle_exchange-mean   2e-7        2e-7
#   mean      bert         peaked_wide   5.5e-08 ln_768_T384-mean              6e-8        9e-8
#   mean      distilbert   peaked        9.1e-08 distilbert_packed-mean        1e-7        1e-7
#   mean      electra      peaked        8.3e-08 electra_packed-mean           9e-8        2e-7
#   mean      roberta      flat          5.2e-08 roberta_packed-mean           6e-8        7e-8
#   cls+mean  mpnet        flat          5.3e-08 mp_S140_packed-cls            6e-8        8e-8
#   cls+mean  mpnet        peaked        1.8e-07 mp_T_lt_4b-cls                2e-7        2e-7
#   cls+mean  mpnet        peaked_wide   1.2e-07 mp_768_planes-cls             2e-7        2e-7
#   cls+mean  deberta      flat          5.4e-08 db_S70_flat-cls               6e-8        7e-8
#   cls+mean  deberta      peaked        1.2e-07 db_padded_no_mask-mean        2e-7        2e-7
#
# Operand range over all of them (operand_range): |activation| <= 25.1 (db_posbiased_types), |weight| <= 0.90 (db_noshare), against
# 1023 / 4 and 63.9 / 4.  Mutants, in yardsticks (rms): the weakest harmful single-site pair of the BERT grid is lo_a_lost[qkv,1] on
# sa_longest32-cls at 17 (flat regime: small operands), of all grids lo_a_lost[qkv,0] on mp_S140_packed-cls at 11; the same
# mistakes in max-abs device bounds: 0.2 .. 23, and 83 of the 646 (case, single-site mutant) pairs PASS that bound.  RMS_FACTOR <= 17 / 2.
F16X2_DEV = {
    ("cls", "bert", "flat"): 8e-8,
    ("cls", "bert", "peaked"): 2e-7,
    ("cls", "bert", "peaked_wide"): 2e-7,
    ("cls", "distilbert", "peaked"): 9e-8,
    ("cls", "electra", "peaked"): 9e-8,
    ("cls", "roberta", "flat"): 7e-8,
    ("cls", "xlm-roberta", "flat"): 7e-8,
    ("mean", "bert", "peaked"): 2e-7,
    ("mean", "bert", "peaked_wide"): 6e-8,
    ("mean", "distilbert", "peaked"): 1e-7,
    ("mean", "electra", "peaked"): 9e-8,
    ("mean", "roberta", "flat"): 6e-8,
    ("cls+mean", "mpnet", "flat"): 6e-8,
    ("cls+mean", "mpnet", "peaked"): 2e-7,
    ("cls+mean", "mpnet", "peaked_wide"): 2e-7,
    ("cls+mean", "deberta", "flat"): 6e-8,
    ("cls+mean", "deberta", "peaked"): 2e-7,
}
