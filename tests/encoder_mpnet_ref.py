"""Shared by tests/test_encoder_mpnet_cpu.py, tests/test_encoder_mpnet_gpu.py and tests/test_classifier_mpnet_gpu.py: the MPNet
family (transformers `model_type == "mpnet"`) stated on top of tests/encoder_ref.py -- that file's LayerNorm / GELU / key-mask
pieces, batches, Case record and factors are imported, never edited.

  reference    `mpnet_forward`: the BERT block (post-norm, erf GELU, fused heads) with MPNet's parameter names, no token types,
               positions from padding_idx + 1 over the non-pad tokens, and ONE relative position bias for all layers,
                   softmax(q k^T / sqrt(dh) + bias[h, bucket(j - i)] + key mask),   i = query, j = key, counted inside the sequence,
               in any dtype, from the `state_dict`.  The buckets are the loaded model's own `encoder.relative_position_bucket` (it
               takes a logarithm in fp32 and truncates: restating it in fp64 can land in the neighbouring bucket).  Returns the
               unit-norm CLS rows; `hidden_out` receives the hidden states, from which `pooled(...)` takes the masked mean through
               encoder_pool_ref.masked_mean_normalize.
  fp32 instances (the yardstick, as in encoder_ref.py): the same in fp32; the same with every matmul in K-chunks of 16; transformers
               fp32 eager (attn_implementation="eager").
  models       MPNetModel(MPNetConfig(...), add_pooling_layer=False) under a fixed seed; then relative_attention_bias.weight is
               redrawn from N(0, 1) (at the init's std 0.02 a kernel that ignores the bias is only ~1.5e-4 from the reference), the
               FFN-up weights get encoder_ref.FFN_GAIN, and the "peaked" regimes scale q / k and plant LayerNorm outliers with the
               figures of encoder_ref.regime_kw.
  mutants      MPNET_MUTANTS: the bias mistakes below plus those of encoder_ref.MUTANTS that apply to this block.
  bounds       FP32_DEV_MPNET[regime] = the worst deviation of the three fp32 instances from fp64 over the regime's cases (both
               poolings), measured on the CPU and rounded up to one digit (tests/test_encoder_mpnet_cpu.py asserts the constants and
               prints the table); the device is held to encoder_ref.KERNEL_FACTOR x the figure, never more than
               encoder_ref.DEVICE_BOUND_CEILING.  No bound comes from a device observation.
  cases        MPNET_CASES: (encoder_ref.Case, pooling) pairs on the shapes at which the biased kernels can go wrong.
"""
import dataclasses
import functools
import math

import torch
import torch.nn.functional as F

import encoder_ref as R
import encoder_pool_ref as P

PAD_ID = 1                       # MPNet's ids: <s> = 0, <pad> = 1, </s> = 2 -- what encoder_ref.make_batch writes for family="roberta"
BATCH_FAMILY = "roberta"

# ------------------------------------------------------------------------------------------------------------------------
# mutants: name -> what the mistake is
# ------------------------------------------------------------------------------------------------------------------------
BIAS_MUTANTS = {
    "no_bias":             "the relative position bias left out",
    "bias_transposed":     "the table read at i - j in place of j - i",
    "bias_shift_one":      "the table read at j - i + 1",
    "bias_heads_rotated":  "head h takes the table row of head h - 1",
    "bias_also_scaled":    "the bias multiplied by 1 / sqrt(dh) like the scores",
    "bias_layer0_only":    "the bias added in layer 0 only",
    # positions taken from the token's ROW in the batch as the kernels see it (packed: the rows of the real tokens one sequence
    # after the other; padded: row b * S + j) in place of the position inside the sequence.  A plain row index would give the same
    # j - i and hide the mistake, so the form stated here is the one a tiled kernel makes: the row index inside its 32-row tile,
    # (row mod 32) for the query and for the key -- equal to j - i only while both rows lie in one 32-row tile of the batch.
    "bias_absolute_rows":  "distance taken between the batch rows mod 32 in place of the positions inside the sequence",
    "bias_saturate_64":    "distances clamped to [-64, 64] before the bucket (the buckets saturate at 128)",
}
BASE_MUTANTS = ("gelu_tanh", "ln_var_h-1", "scale_hidden", "drop_last_key", "admit_first_pad", "roberta_offset_1", "v_heads_rotated",
                "resid_after_ln")
MPNET_MUTANTS = dict(BIAS_MUTANTS, **{k: R.MUTANTS[k][1] for k in BASE_MUTANTS})


# ------------------------------------------------------------------------------------------------------------------------
# the forward
# ------------------------------------------------------------------------------------------------------------------------
def _row_starts(mask, b, S, packed):
    """first batch row of every sequence: packed (the real tokens of right-padded rows one after the other) or padded (i * S)"""
    if packed and mask is not None:
        lens = mask.sum(1)
        return torch.cumsum(lens, 0) - lens
    return torch.arange(b) * S


def position_bias(model, b, S, dtype, mut=(), mask=None, packed=True):
    """[b | 1, heads, S, S]: what is added to the scaled scores (before the key mask)"""
    i = torch.arange(S)[:, None]
    j = torch.arange(S)[None, :]
    rel = (j - i)[None]                                                     # [1, S, S]
    if "bias_transposed" in mut:
        rel = -rel
    if "bias_shift_one" in mut:
        rel = rel + 1
    if "bias_absolute_rows" in mut:
        r0 = _row_starts(mask, b, S, packed)[:, None, None]
        rel = (r0 + j[None]) % 32 - (r0 + i[None]) % 32                     # [b, S, S]
    if "bias_saturate_64" in mut:
        rel = rel.clamp(-64, 64)
    bucket = model.encoder.relative_position_bucket(rel, num_buckets=int(model.config.relative_attention_num_buckets))
    table = model.state_dict()["encoder.relative_attention_bias.weight"].to(dtype)          # [buckets, heads]
    bias = table[bucket].permute(0, 3, 1, 2)                                # [b | 1, heads, S, S]
    if "bias_heads_rotated" in mut:
        bias = torch.roll(bias, 1, dims=1)
    if "bias_also_scaled" in mut:
        bias = bias / math.sqrt(model.config.hidden_size // model.config.num_attention_heads)
    if "no_bias" in mut:
        bias = torch.zeros_like(bias)
    return bias


def _attention(q, k, v, bias, allow, scale, mm, probs_out):
    """encoder_ref._attention with the bias between the scaling and the key mask"""
    s = mm(q, k.transpose(-1, -2)) * scale
    if bias is not None:
        s = s + bias
    s = s + torch.zeros_like(s).masked_fill(~allow, float("-inf"))
    m = s.max(-1, keepdim=True).values
    m = torch.where(torch.isinf(m), torch.zeros_like(m), m)
    e = torch.exp(s - m)
    den = e.sum(-1, keepdim=True)
    p = e / torch.where(den > 0, den, torch.ones_like(den))
    if probs_out is not None:
        probs_out.append(p)
    ctx = mm(p, v)
    b, h, S, dh = ctx.shape
    return ctx.transpose(1, 2).reshape(b, S, h * dh)


@torch.no_grad()
def mpnet_forward(model, ids, mask, dtype=torch.float64, mm=R.mm_plain, mut=(), hidden_out=None, probs_out=None, packed=True,
                  lin_mm=None):
    """unit-norm CLS rows [b, H] of an MPNetModel on (ids, mask); `packed` only tells the bias_absolute_rows mutant which rows
    the device call would see.  lin_mm: encoder_ref._lin_mm (the nn.Linear layers only; scores, bias and P.V keep `mm`)."""
    sd, cfg = model.state_dict(), model.config
    lmm = R._lin_mm(mm, lin_mm)
    W = lambda k: sd[k].to(dtype)
    H, L, heads, eps = cfg.hidden_size, cfg.num_hidden_layers, cfg.num_attention_heads, float(cfg.layer_norm_eps)
    b, S = ids.shape
    pad = int(cfg.pad_token_id)
    real = (ids != pad).long()
    off = pad - 1 if "roberta_offset_1" in mut else pad
    pos = torch.cumsum(real, dim=1) * real + off * real + pad * (1 - real)
    x = W("embeddings.word_embeddings.weight")[ids] + W("embeddings.position_embeddings.weight")[pos]
    x = R._layer_norm(x, W("embeddings.LayerNorm.weight"), W("embeddings.LayerNorm.bias"), eps, mut)
    if hidden_out is not None:
        hidden_out.append(x)
    allow = R._key_mask(mask, b, S, mut)[:, None, None, :].expand(b, 1, S, S)
    dh = H // heads
    scale = 1.0 / math.sqrt(H if "scale_hidden" in mut else dh)
    bias = position_bias(model, b, S, dtype, mut, mask, packed)

    def lin(t, name):
        return lmm(t, W(name + ".weight").T, name) + W(name + ".bias")

    def ln(t, name):
        return R._layer_norm(t, W(name + ".weight"), W(name + ".bias"), eps, mut)

    for l in range(L):
        p = f"encoder.layer.{l}."
        q, k, v = (R._heads(lin(x, p + "attention.attn." + n), heads) for n in ("q", "k", "v"))
        if "v_heads_rotated" in mut:
            v = torch.roll(v, 1, dims=1)
        layer_bias = None if ("bias_layer0_only" in mut and l > 0) else bias
        ao = lin(_attention(q, k, v, layer_bias, allow, scale, mm, probs_out), p + "attention.attn.o")
        x1 = ln(ao, p + "attention.LayerNorm") + x if "resid_after_ln" in mut else ln(x + ao, p + "attention.LayerNorm")
        f = lin(R._gelu(lin(x1, p + "intermediate.dense"), mut), p + "output.dense")
        x = ln(f, p + "output.LayerNorm") + x1 if "resid_after_ln" in mut else ln(x1 + f, p + "output.LayerNorm")
        if hidden_out is not None:
            hidden_out.append(x)
    return F.normalize(x[:, 0, :], p=2, dim=1, eps=1e-12)


# ------------------------------------------------------------------------------------------------------------------------
# models
# ------------------------------------------------------------------------------------------------------------------------
def mpnet_config(hidden, layers, heads, inter, max_pos, vocab=R.VOCAB, pad_token_id=PAD_ID, **kw):
    from transformers import MPNetConfig
    cfg = MPNetConfig(vocab_size=vocab, hidden_size=hidden, num_hidden_layers=layers, num_attention_heads=heads, intermediate_size=inter,
                      max_position_embeddings=max_pos, pad_token_id=pad_token_id, hidden_dropout_prob=0.0,
                      attention_probs_dropout_prob=0.0, **kw)
    try:
        cfg._attn_implementation = "eager"
    except Exception:
        pass
    return cfg


@torch.no_grad()
def build_model(cfg, regime, seed=0):
    """a seeded MPNetModel made sensitive: bias table N(0, 1), FFN-up x FFN_GAIN, and for the peaked regimes q / k x qk_scale with
    fresh biases plus four LayerNorm outlier channels per norm (the figures of encoder_ref.regime_kw for the BERT families)"""
    from transformers import MPNetModel
    torch.manual_seed(seed)
    try:
        model = MPNetModel(cfg, add_pooling_layer=False, attn_implementation="eager").eval()
    except TypeError:
        model = MPNetModel(cfg, add_pooling_layer=False).eval()
    g = torch.Generator().manual_seed(seed + 41)
    rb = model.encoder.relative_attention_bias.weight
    rb.copy_(torch.randn(rb.shape, generator=g))
    kw = R.regime_kw("bert", regime, cfg.hidden_size)
    for name, p in model.named_parameters():
        if name.endswith("intermediate.dense.weight"):
            p.mul_(R.FFN_GAIN[cfg.hidden_size])
    if kw:
        for name, mod in model.named_modules():
            leaf = name.rsplit(".", 1)[-1]
            if leaf in ("q", "k") and isinstance(mod, torch.nn.Linear):
                mod.weight.mul_(kw["qk_scale"])
                mod.bias.copy_(torch.randn(mod.bias.shape, generator=g) * 0.02 * kw["qk_scale"])
            elif isinstance(mod, torch.nn.LayerNorm):
                idx = torch.randperm(mod.weight.numel(), generator=g)[:4]
                mod.weight[idx] *= kw["ln_outlier"]
                mod.bias[idx] += 0.5 * kw["ln_outlier"] * torch.randn(4, generator=g)
    return model


@functools.lru_cache(maxsize=None)
def make_model(m: R.ModelSpec):
    assert m.family == "mpnet"
    return build_model(mpnet_config(m.hidden, m.layers, m.heads, m.inter, m.max_pos), m.regime, m.seed)


# ------------------------------------------------------------------------------------------------------------------------
# the cases: (Case, pooling).  Dispatch as encoder_ref.py states it, with what a bias table changes (csrc/bert.hip):
#   attention fusion    never                                                       [ac_gemm_qkv_attn_launches stays: attn_launches 0]
#   one launch          never: <= 32 token rows run layer by layer                  [used_one_launch False]
#   planes, LayerNorm fusion, unpad entry, CLS tail: untouched -- ln_launches is what the same shape records for the other
#   BERT-block families, 2 per token layer (L - 1 of them under "cls", L under "mean") once T >= 192 on bf16x3
# ------------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class MPCase:
    case: R.Case
    pooling: str

    @property
    def id(self):
        return f"{self.case.id}-{self.pooling}"

    @property
    def regime(self):
        return self.case.model.regime


MPNET_CASES = []
L = 3


def add(id, hidden, layers, heads, inter, b, S, lengths, regime, poolings=("cls",), planes=False, max_pos=0, **kw):
    m = R.ModelSpec("mpnet", hidden, layers, heads, inter, regime, max_pos=max_pos or max(S + 2, 64))
    bs = R.BatchSpec(BATCH_FAMILY, b, S, None if lengths is None else tuple(lengths))
    if kw.get("path") == "packed":
        kw["tokens"] = sum(lengths)
    for pooling in poolings:
        token_layers = layers if pooling == "mean" else layers - 1
        c = R.Case(id, m, bs, "mpnet", one_launch=False, attn_launches=0, ln_launches=2 * token_layers if planes else 0, **kw)
        MPNET_CASES.append(MPCase(c, pooling))


BOTH = ("cls", "mean")
LEN33 = (33, 31, 30, 25, 32, 21, 20)                     # 192 rows: planes; one key past a tile
LEN70 = (70, 64, 32, 1, 33)                              # 200 rows: three query / key tiles, multiples of 32, a lone token
LEN140 = (140, 40, 66)                                   # 246 rows: |j - i| >= 128, the saturated buckets
LEN20 = (20, 19, 18, 17, 1, 20, 17, 19, 18, 20, 1, 20)   # 190 rows: the first logarithmic buckets; fp32 activations (< 192)
LEN768 = (40, 33, 21, 40, 12, 37, 26, 40, 31)            # 280 rows
add("mp_S33_packed", 128, L, 2, 512, 7, 33, LEN33, "peaked", BOTH, planes=True, path="packed",
    note="second key tile holds one key; CLS attention on 64-key tiles; T >= 4 b")
add("mp_S70_packed", 128, L, 2, 512, 5, 70, LEN70, "peaked", BOTH, planes=True, path="packed",
    note="three query tiles x three key tiles; lengths 64 and 32 end on a tile edge, one sequence of one token")
add("mp_S140_packed", 128, L, 2, 512, 3, 140, LEN140, "flat", ("cls",), planes=True, path="packed", note="distances up to 139")
add("mp_S20_no_planes", 128, L, 2, 512, 12, 20, LEN20, "peaked", BOTH, path="packed",
    note="190 rows: fp32 activations, the attention writes fp32 rows; CLS attention on 32-key tiles")
add("mp_dh32_S33", 128, L, 4, 512, 7, 33, LEN33, "peaked", BOTH, planes=True, path="packed", note="head dim 32")
add("mp_S33_masked", 128, L, 2, 512, 7, 33, LEN33, "peaked", BOTH, planes=True, unpad=False,
    note="unpad=False: 231 padded rows with the mask; padding queries and keys index the table too")
add("mp_T_lt_4b", 128, L, 2, 512, 100, 3, R.cyc((3, 2, 3, 1, 3), 100), "peaked", ("cls",), planes=True, path="packed",
    note="240 rows < 4 b: the last layer computes Q for every row; CLS attention on 32-key tiles")
add("mp_small_T32", 128, L, 2, 512, 4, 8, (8, 5, 1, 7), "peaked", BOTH, note="32 token rows: layer by layer, never the one launch")
add("mp_768_planes", 768, 2, 12, 3072, 9, 40, LEN768, "peaked_wide", BOTH, planes=True, path="packed", sens=False,
    note="H 768: fused LayerNorm epilogues, the attention writes operand planes")
add("mp_768_f32", 768, 2, 12, 3072, 9, 40, LEN768, "peaked_wide", ("cls",), path="packed", arith="f32", sens=False,
    note='arith="f32": no planes')

BY_ID = {c.id: c for c in MPNET_CASES}
assert len(BY_ID) == len(MPNET_CASES)


# ------------------------------------------------------------------------------------------------------------------------
# evaluation (cached per input)
# ------------------------------------------------------------------------------------------------------------------------
def _packed(case):
    return case.path == "packed"


@functools.lru_cache(maxsize=None)
def _hidden(m, bs, dtype, chunked, mut, packed):
    ids, _, mask = R.make_batch(bs)
    hs = []
    cls = mpnet_forward(make_model(m), ids, mask, dtype=dtype, mm=R.mm_chunk16 if chunked else R.mm_plain, mut=mut, hidden_out=hs,
                        packed=packed)
    return cls, hs[-1]


def _admitted(bs):
    _, _, mask = R.make_batch(bs)
    return torch.ones((bs.b, bs.S), dtype=torch.bool) if mask is None else mask.bool()


def _pooled(mc, dtype=torch.float64, chunked=False, mut=()):
    c = mc.case
    cls, h = _hidden(c.model, c.batch, dtype, chunked, tuple(mut), _packed(c))
    return cls if mc.pooling == "cls" else P.masked_mean_normalize(h, _admitted(c.batch))


def reference(mc):
    """fp64 unit-norm vectors [b, H] of the case under its pooling (computed once per input, shared; do not modify)"""
    return _pooled(mc)


def fp32_instance(mc, chunked=False):
    return _pooled(mc, torch.float32, chunked)


@torch.no_grad()
def transformers_fp32(mc):
    c = mc.case
    ids, _, mask = R.make_batch(c.batch)
    h = make_model(c.model)(input_ids=ids, attention_mask=mask).last_hidden_state
    return F.normalize(h[:, 0, :], p=2, dim=1) if mc.pooling == "cls" else P.masked_mean_normalize(h, _admitted(c.batch))


def deviation(mc, got):
    return float((got.detach().double().cpu() - reference(mc)).abs().max())


def applicable(name, mc):
    """can this mistake change anything on this case's input?"""
    c = mc.case
    _, _, mask = R.make_batch(c.batch)
    longest = int(mask.sum(1).max())
    if name == "admit_first_pad":
        return bool((mask == 0).any())
    if name in ("drop_last_key",) or name in BIAS_MUTANTS and name not in ("bias_saturate_64", "bias_absolute_rows", "bias_layer0_only"):
        return longest > 1
    if name == "bias_layer0_only":
        return longest > 1 and c.model.layers > 1
    if name == "bias_saturate_64":
        return longest > 91                              # the bucket of 64 holds the distances 64 .. 90
    if name == "bias_absolute_rows":
        r0 = _row_starts(mask, c.batch.b, c.batch.S, _packed(c))
        lens = mask.sum(1)
        return bool(((r0 % 32 + lens) > 32).any())       # a sequence that crosses a 32-row tile edge of the batch
    return True


def mutant_distance(mc, name):
    return float((_pooled(mc, mut=(name,)) - reference(mc)).abs().max())


# ------------------------------------------------------------------------------------------------------------------------
# bounds
# ------------------------------------------------------------------------------------------------------------------------
# FP32_DEV_MPNET[regime]: worst max-abs deviation from fp64 of the three fp32 instances over the regime's MPNET_CASES (both
# poolings), measured on the CPU and rounded up to one digit; tests/test_encoder_mpnet_cpu.py asserts every case stays within
# encoder_ref.ADMISSION x the figure and prints this table.  The worst cases at the time of writing (16 CPU threads):
#
#   regime        torch fp32                  K-chunks of 16                 transformers fp32           FP32_DEV_MPNET   16 x
#   flat          6.0e-08 mp_S140_packed-cls  4.7e-08 mp_S140_packed-cls     7.5e-08 mp_S140_packed-cls  8e-8             1.3e-6
#   peaked        1.8e-07 mp_T_lt_4b-cls      1.9e-07 mp_S20_no_planes-cls   1.7e-07 mp_S33_packed-cls   2e-7             3.2e-6
#   peaked_wide   1.8e-07 mp_768_planes-cls   7.3e-08 mp_768_planes-cls      1.5e-07 mp_768_planes-cls   2e-7             3.2e-6
#
# The least visible mutant is gelu_tanh (9 .. 15 bounds: three layers of width 128); the least visible BIAS mutant on the cases the
# CPU test names for it sits hundreds of bounds out.
FP32_DEV_MPNET = {
    "flat": 8e-8,
    "peaked": 2e-7,
    "peaked_wide": 2e-7,
}


def device_bound(mc):
    bound = R.KERNEL_FACTOR * FP32_DEV_MPNET[mc.regime]
    assert bound <= R.DEVICE_BOUND_CEILING, (mc.id, bound)
    return bound
