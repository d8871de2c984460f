"""Shared by tests/test_encoder_pool_cpu.py, tests/test_encoder_pool_gpu.py and tests/test_classifier_pool_gpu.py: masked mean
pooling (`pooling="mean"`, AC_POOL_MEAN) stated on top of tests/encoder_ref.py -- that file's forwards, models, batches and case
grid are imported, never edited.

  reference    `pooled_reference(case)` = the family's fp64 forward with `hidden_out`; ModernBERT's final_norm applied to
               hidden_out[-1] per token (the norm first, then the mean); the mean over the ADMITTED tokens (mask != 0; every token
               without a mask) divided by max(count, 1); F.normalize.  Unit-norm vectors [b, H]; an all-masked row is zero and is
               not compared (encoder_ref.compared_rows).
  fp32 instances (the yardstick, as in encoder_ref.py): the same in fp32; the same with every matmul summed in K-chunks of 16;
               transformers fp32 eager `last_hidden_state` pooled the same way.
  mutants      POOL_MUTANTS: switches on the fp64 pooling, each a plausible mistake of the pooling kernel or of its dispatch.  The
               divisor itself cannot be seen after the normalisation and has no mutant (the kernel divides by the count anyway).
  bounds       FP32_DEV_POOL[(family, regime)] = the worst deviation of the three fp32 instances from fp64 over the group's
               POOL_CASES, measured on the CPU and rounded up to one digit (tests/test_encoder_pool_cpu.py asserts the constants
               hold and prints the table); the device is held to encoder_ref.KERNEL_FACTOR x the figure, never more than
               encoder_ref.DEVICE_BOUND_CEILING.  No bound comes from a device observation.
  cases        POOL_CASES = cases of encoder_ref.CASES re-run with pooling="mean".  The last layer is an ordinary token layer then:
               it takes the fused route of the layers before it, so the counters read 2 L / L where the CLS case records
               2 (L - 1) / (L - 1), and a call of <= 32 token rows runs layer by layer (one_launch False).  Path and token count are
               those of the CLS case.
"""
import dataclasses
import functools

import torch
import torch.nn.functional as F

import encoder_ref as R

# ------------------------------------------------------------------------------------------------------------------------
# mutants: name -> (families it applies to, what the mistake is)
# ------------------------------------------------------------------------------------------------------------------------
POOL_MUTANTS = {
    "cls":                    (R.ALL, "row 0 of every sequence instead of the mean (the default pooling taken by mistake)"),
    "include_pad":            (R.ALL, "the rows that are not admitted summed too (the mask ignored by the pooling)"),
    "drop_last_token":        (R.ALL, "the last admitted token of every sequence (of more than one) left out"),
    "drop_first_token":       (R.ALL, "the first admitted token of every sequence (of more than one) left out"),
    "normalize_tokens_first": (R.ALL, "every token row L2-normalised before the mean"),
    "no_final_norm":          (("modernbert",), "the mean of the residual stream without the final norm"),
    "norm_after_pool":        (("modernbert",), "the final norm of the mean instead of the mean of the final norms"),
}


# ------------------------------------------------------------------------------------------------------------------------
# the pooled forward
# ------------------------------------------------------------------------------------------------------------------------
def _last_hidden(m, bs, dtype=torch.float64, mm=R.mm_plain, lin_mm=None):
    """[b, S, H] after the last layer (ModernBERT: BEFORE the final norm), in `dtype` (lin_mm: encoder_ref._lin_mm)"""
    model = R.make_model(m)
    ids, types, mask = R.make_batch(bs)
    hs = []
    R.FORWARD[m.family](model.state_dict(), model.config, ids, types, mask, dtype=dtype, mm=mm, hidden_out=hs, lin_mm=lin_mm)
    return hs[-1]


def _final_norm(m, h):
    """ModernBERT's final norm per row, in h's dtype (the expressions of encoder_ref._layer_norm)"""
    model = R.make_model(m)
    sd = model.state_dict()
    g = sd["final_norm.weight"].to(h.dtype)
    b = sd["final_norm.bias"].to(h.dtype) if "final_norm.bias" in sd else None
    return R._layer_norm(h, g, b, float(model.config.norm_eps), ())


def _admitted(bs, mut=()):
    """bool [b, S]: the tokens the mean runs over"""
    _, _, mask = R.make_batch(bs)
    adm = torch.ones((bs.b, bs.S), dtype=torch.bool) if mask is None else mask.bool().clone()
    if "include_pad" in mut:
        adm[:] = True
    for name, pick in (("drop_last_token", -1), ("drop_first_token", 0)):
        if name in mut:
            for i in range(bs.b):
                real = adm[i].nonzero()
                if len(real) > 1:
                    adm[i, int(real[pick])] = False
    return adm


def masked_mean_normalize(h, adm):
    """h [b, S, H], adm bool [b, S] -> F.normalize(sum over the admitted tokens / max(count, 1))"""
    w = adm.to(h.dtype)[:, :, None]
    mean = (h * w).sum(1) / adm.sum(1).clamp(min=1).to(h.dtype)[:, None]
    return F.normalize(mean, p=2, dim=1, eps=1e-12)


def pool(m, bs, h, mut=()):
    """the pooling of last-layer rows h (ModernBERT: before the final norm) with the mistakes of `mut`"""
    mb = m.family == "modernbert"
    if mb and "no_final_norm" not in mut and "norm_after_pool" not in mut:
        h = _final_norm(m, h)
    if "cls" in mut:
        return F.normalize(h[:, 0, :], p=2, dim=1, eps=1e-12)
    if "normalize_tokens_first" in mut:
        h = F.normalize(h, p=2, dim=2, eps=1e-12)
    adm = _admitted(bs, mut)
    if mb and "norm_after_pool" in mut:
        w = adm.to(h.dtype)[:, :, None]
        mean = (h * w).sum(1) / adm.sum(1).clamp(min=1).to(h.dtype)[:, None]
        return F.normalize(_final_norm(m, mean), p=2, dim=1, eps=1e-12)
    return masked_mean_normalize(h, adm)


@functools.lru_cache(maxsize=None)
def _hidden64(m, bs):
    return _last_hidden(m, bs)


@functools.lru_cache(maxsize=None)
def _reference(m, bs):
    return pool(m, bs, _hidden64(m, bs))


def pooled_reference(case):
    """fp64 unit-norm mean-pooled vectors [b, H] of the case (computed once per input, shared; do not modify)"""
    return _reference(case.model, case.batch)


def fp32_instance(case, chunked=False):
    return pool(case.model, case.batch, _last_hidden(case.model, case.batch, torch.float32, R.mm_chunk16 if chunked else R.mm_plain))


@torch.no_grad()
def transformers_fp32(case):
    """transformers fp32 eager last_hidden_state (ModernBERT: its final norm included) pooled the same way"""
    model = R.make_model(case.model)
    ids, types, mask = R.make_batch(case.batch)
    kw = dict(input_ids=ids)
    if mask is not None:
        kw["attention_mask"] = mask
    if types is not None:
        kw["token_type_ids"] = types
    return masked_mean_normalize(model(**kw).last_hidden_state, _admitted(case.batch))


def applicable(name, case):
    """can this mistake change anything on this case's input?"""
    fams, _ = POOL_MUTANTS[name]
    m, bs = case.model, case.batch
    if m.family not in fams:
        return False
    rows = R.compared_rows(bs)
    adm = _admitted(bs)[rows]
    if name == "cls":
        return bool((adm.sum(1) > 1).any() | (~adm[:, 0]).any())
    if name == "include_pad":
        return bool((~adm).any())                        # a masked-out position in a compared row
    if name in ("drop_last_token", "drop_first_token"):
        return bool((adm.sum(1) > 1).any())
    if name == "normalize_tokens_first":
        return m.regime != "flat"                        # (transformers' init: unit LayerNorm gains, every token row has the norm
    return True                                          #  sqrt(H) -- the mistake changes nothing there; it measured 0)


@functools.lru_cache(maxsize=None)
def _mutant(m, bs, name):
    rows = R.compared_rows(bs)
    return float((pool(m, bs, _hidden64(m, bs), mut=(name,)) - _reference(m, bs))[rows].abs().max())


def mutant_distance(case, name):
    """max-abs distance of the mutant's unit vectors from the pooled reference over the compared rows"""
    return _mutant(case.model, case.batch, name)


def deviation(case, got):
    """max-abs difference of `got` [b, H] (any dtype / device) from the fp64 pooled reference over the compared rows"""
    rows = R.compared_rows(case.batch)
    return float((got.detach().double().cpu() - pooled_reference(case))[rows].abs().max())


# ------------------------------------------------------------------------------------------------------------------------
# the cases
# ------------------------------------------------------------------------------------------------------------------------
POOL_IDS = (
    # one launch declined / layered small; packed; every fusion; the exchange; stand-alone attention; padded with a mask
    "ol_T32_forced_layered", "ol_T33_packed", "T192_all_fused", "attn_straddle_exchange", "sa_longest129", "pm_left_padded", "pm_holes",
    "pm_empty_row", "ones_explicit", "sa_dh32_longest33", "ln_768_T384", "mb_S16_small", "mb_S40_planes_packed", "mb_lonely_query",
    "distilbert_packed", "roberta_packed", "electra_packed",
    # the plane threshold and the arithmetic
    "T191_no_planes", "T192_f32_arith", "T192_both_off",
    # the fused attention's edges
    "attn_straddle_boundary", "attn_ends_on_boundary", "attn_many_short", "attn_longest65",
    "pm_holes_planes", "pm_empty_row_planes",
    # what used to be the CLS tail: the output stride, T < 4 b, b >= 192
    "last_ldo_wide", "last_T_lt_4b", "last_b200",
    "mb_S40_planes_padded", "mb_ge2", "mb_b200",
    "chunks_fused_then_not",
    # <= 32 token rows: no one-launch form under mean pooling, layer by layer
    "distilbert_one_launch", "roberta_one_launch", "xlm-roberta_one_launch", "electra_one_launch",
)


def _pooled_case(c):
    L = c.model.layers
    assert c.ln_launches in (0, 2 * (L - 1)) and c.attn_launches in (0, L - 1), c.id
    return dataclasses.replace(c, one_launch=False, ln_launches=2 * L if c.ln_launches else 0,
                               attn_launches=L if c.attn_launches else 0, sens=True)


POOL_CASES = [_pooled_case(R.BY_ID[i]) for i in POOL_IDS]
POOL_BY_ID = {c.id: c for c in POOL_CASES}
assert len(POOL_BY_ID) == len(POOL_IDS)

# ------------------------------------------------------------------------------------------------------------------------
# bounds
# ------------------------------------------------------------------------------------------------------------------------
# FP32_DEV_POOL[(family, regime)]: worst max-abs deviation from fp64 of the three fp32 instances over the group's POOL_CASES,
# measured on the CPU and rounded up to one digit.  tests/test_encoder_pool_cpu.py asserts every case stays within
# encoder_ref.ADMISSION x its group's figure and prints this table; the worst cases at the time of writing (16 CPU threads):
#
#   group                      torch fp32                     K-chunks of 16                 transformers fp32              FP32_DEV_POOL  16 x    (CLS: FP32_DEV)
#   bert        peaked         1.1e-07 attn_straddle_exchange 9.3e-08 attn_many_short        1.1e-07 attn_straddle_exchange 2e-7      3.2e-6   3e-7
#   bert        peaked_wide    9.0e-08 ln_768_T384            5.3e-08 ln_768_T384            8.7e-08 ln_768_T384            9e-8      1.4e-6   3e-7
#   distilbert  peaked         9.1e-08 distilbert_packed      8.9e-08 distilbert_packed      8.9e-08 distilbert_packed      1e-7      1.6e-6   2e-7
#   electra     peaked         6.7e-08 electra_packed         9.2e-08 electra_packed         1.003e-07 electra_packed       2e-7      3.2e-6   2e-7
#   modernbert  scaled         9.4e-08 mb_b200                7.9e-08 mb_b200                9.4e-08 mb_b200                1e-7      1.6e-6   1e-7
#   roberta     flat           6.2e-08 roberta_packed         4.8e-08 roberta_packed         5.2e-08 roberta_packed         7e-8      1.1e-6   8e-8
#   xlm-roberta flat           2.7e-08 xlm-roberta_one_launch 2.9e-08 xlm-roberta_one_launch 3.5e-08 xlm-roberta_one_launch 4e-8      6.4e-7   8e-8
#
# (the mean over a sequence averages the rows' rounding errors: no group's figure is above its CLS figure.)  The least visible
# mutant at the time of writing: normalize_tokens_first on ol_T32_forced_layered, 4.2e-3 = 1300 bounds; every other applicable
# (case, mutant) pair is farther in bounds.
FP32_DEV_POOL = {
    ("bert", "peaked"): 2e-7,
    ("bert", "peaked_wide"): 9e-8,
    ("distilbert", "peaked"): 1e-7,
    ("electra", "peaked"): 2e-7,
    ("modernbert", "scaled"): 1e-7,
    ("roberta", "flat"): 7e-8,
    ("xlm-roberta", "flat"): 4e-8,
}


def device_bound(case):
    bound = R.KERNEL_FACTOR * FP32_DEV_POOL[case.group]
    assert bound <= R.DEVICE_BOUND_CEILING, (case.id, bound)
    return bound
