"""Shared by tests/test_encoder_deberta_cpu.py, tests/test_encoder_deberta_gpu.py and tests/test_classifier_deberta_gpu.py: the
DeBERTa-v2/v3 family (transformers `model_type == "deberta-v2"`) stated on top of tests/encoder_ref.py -- that file's LayerNorm /
GELU / key-mask pieces, batches, Case record and factors are imported, never edited.

  reference    `deberta_forward`: the BERT block (post-norm, erf GELU) under DeBERTa's parameter names with the disentangled score
                   s[i, j] = ( q_i . k_j  +  q_i . PK[idx(i - j)]  +  k_j . PQ[idx(i - j)] ) / sqrt(dh * scale_factor)
               PK / PQ = the layer's key / query projection (pos_key_proj / pos_query_proj without share_att_key), with bias, of the
               LayerNorm'd relative-position embeddings; idx(i - j) = bucket(i - j) + att_span read off the module's own
               build_relative_position (its logarithm is taken in fp32 and rounded up); ONE index table serves both terms.  The root
               is exact (transformers takes it in fp32 even in a double model: `sqrt32=True` restates that, for the comparison).
               The embeddings are LayerNorm(word [+ position] [+ type]) times the mask.  Any dtype, from the `state_dict`.  Returns
               the unit-norm CLS rows; `hidden_out` receives the hidden states for the masked mean of encoder_pool_ref.
  fp32 instances (the yardstick, as in encoder_ref.py): the same in fp32; the same with every matmul in K-chunks of 16; transformers
               DebertaV2Model in fp32.
  models       DebertaV2Model under a fixed seed, 128 wide, 2 heads of 64, position_buckets 8 (att_span 8: a 40-token sequence
               already walks the logarithmic buckets, to +-7).  rel_embeddings are redrawn from N(0, 1) and the encoder's
               LayerNorm over them gets gains U(0.5, 1.5) and biases N(0, 0.5) (at the init's values skipping it changes nothing),
               every q / k / position projection gets a bias N(0, 0.2) (the init's is zero), the FFN-up weights get
               encoder_ref.FFN_GAIN, and the "peaked" regime scales q / k and plants LayerNorm outliers with encoder_ref.regime_kw.
               Variants: share_att_key off, pos_att_type c2p / p2c alone, position_biased_input with a type table.
  mutants      DEBERTA_MUTANTS: the mistakes of the position terms below plus those of encoder_ref.MUTANTS that apply to this block.
  bounds       FP32_DEV_DEBERTA[regime] = the worst deviation of the three fp32 instances from fp64 over the regime's cases (both
               poolings), measured on the CPU and rounded up to one digit (tests/test_encoder_deberta_cpu.py asserts the constants
               and prints the table); the device is held to encoder_ref.KERNEL_FACTOR x the figure, never more than
               encoder_ref.DEVICE_BOUND_CEILING.  No bound comes from a device observation.
  cases        DEBERTA_CASES: (encoder_ref.Case, pooling) pairs on the shapes at which the new kernels can go wrong.
"""
import copy
import dataclasses
import functools
import math
import sys

import torch
import torch.nn.functional as F

import encoder_ref as R
import encoder_pool_ref as P

POS_MUTANTS = {
    "drop_c2p":              "the content-to-position term left out",
    "drop_p2c":              "the position-to-content term left out",
    "scale_sqrt_d":          "scores scaled by 1 / sqrt(dh) in place of 1 / sqrt(dh * scale_factor)",
    "index_sign_flipped":    "the tables read at idx(j - i) in place of idx(i - j)",
    "p2c_on_query_row":      "the position-to-content term taken from the query's row (k_i . PQ) in place of the key's (k_j . PQ)",
    "no_log_bucket":         "raw distances clamped to the table in place of the logarithmic buckets",
    "rel_ln_skipped":        "the LayerNorm over the relative-position embeddings skipped",
    "pos_proj_bias_dropped": "the bias of the position projections dropped",
    "pos_heads_rolled":      "head h takes the position projections of head h - 1",
}
BASE_MUTANTS = ("gelu_tanh", "ln_var_h-1", "scale_hidden", "drop_last_key", "admit_first_pad", "v_heads_rotated", "resid_after_ln")
DEBERTA_MUTANTS = dict(POS_MUTANTS, **{k: R.MUTANTS[k][1] for k in BASE_MUTANTS})

VARIANTS = {                                   # family string of the ModelSpec -> config switches
    "deberta":           {},
    "deberta:noshare":   {"share_att_key": False},
    "deberta:c2p":       {"pos_att_type": ["c2p"]},
    "deberta:p2c":       {"pos_att_type": ["p2c"]},
    "deberta:posbiased": {"position_biased_input": True, "type_vocab_size": 2},
}
POSITION_BUCKETS = 8


# ------------------------------------------------------------------------------------------------------------------------
# the forward
# ------------------------------------------------------------------------------------------------------------------------
def _terms(cfg):
    t = cfg.pos_att_type or []
    return tuple(t.split("|")) if isinstance(t, str) else tuple(t)


def _attention(s, v, allow, mm):
    """encoder_ref._attention from the finished scores"""
    s = s + torch.zeros_like(s).masked_fill(~allow, float("-inf"))
    m = s.max(-1, keepdim=True).values
    m = torch.where(torch.isinf(m), torch.zeros_like(m), m)
    e = torch.exp(s - m)
    den = e.sum(-1, keepdim=True)
    p = e / torch.where(den > 0, den, torch.ones_like(den))
    ctx = mm(p, v)
    b, h, S, dh = ctx.shape
    return ctx.transpose(1, 2).reshape(b, S, h * dh)


def relative_index(model, S, mut=()):
    """[S, S] long: the table row of (query i, key j)"""
    att = model.encoder.layer[0].attention.self
    att_span = int(att.pos_ebd_size)
    probe = torch.zeros(S, 1)
    if "no_log_bucket" in mut:
        i = torch.arange(S)
        rp = (i[:, None] - i[None, :]).clamp(-(att_span - 1), att_span - 1)
    else:
        rp = sys.modules[type(model).__module__].build_relative_position(probe, probe, bucket_size=int(att.position_buckets),
                                                                         max_position=int(att.max_relative_positions))[0]
    if "index_sign_flipped" in mut:
        rp = -rp
    return (rp + att_span).clamp(0, 2 * att_span - 1)


@torch.no_grad()
def deberta_forward(model, ids, types, mask, dtype=torch.float64, mm=R.mm_plain, mut=(), hidden_out=None, sqrt32=False, lin_mm=None):
    """unit-norm CLS rows [b, H] of a DebertaV2Model on (ids, types, mask).  lin_mm: encoder_ref._lin_mm, for the nn.Linear layers of
    the token rows only -- the projections of the relative-position embeddings keep `mm` (on the device they are made once, outside
    the token-row GEMMs), as do the three score products and P.V."""
    sd, cfg = model.state_dict(), model.config
    lmm = R._lin_mm(mm, lin_mm)
    W = lambda k: sd[k].to(dtype)
    H, L, heads, eps = cfg.hidden_size, cfg.num_hidden_layers, cfg.num_attention_heads, float(cfg.layer_norm_eps)
    b, S = ids.shape
    x = W("embeddings.word_embeddings.weight")[ids]
    if getattr(cfg, "position_biased_input", True):
        x = x + W("embeddings.position_embeddings.weight")[torch.arange(S)][None]
    if cfg.type_vocab_size > 0:
        x = x + W("embeddings.token_type_embeddings.weight")[torch.zeros_like(ids) if types is None else types]
    x = R._layer_norm(x, W("embeddings.LayerNorm.weight"), W("embeddings.LayerNorm.bias"), eps, mut)
    if mask is not None:
        x = x * mask.to(dtype)[:, :, None]
    if hidden_out is not None:
        hidden_out.append(x)
    allow = R._key_mask(mask, b, S, mut)[:, None, None, :].expand(b, 1, S, S)
    dh = H // heads
    terms = _terms(cfg)
    sf = 1 + sum(1 for t in ("c2p", "p2c") if t in terms)
    under = (H if "scale_hidden" in mut else dh) * (1 if "scale_sqrt_d" in mut else sf)
    scale = 1.0 / (float(torch.sqrt(torch.tensor(float(under), dtype=torch.float32))) if sqrt32 else math.sqrt(under))
    att_span = int(model.encoder.layer[0].attention.self.pos_ebd_size)
    rel = W("encoder.rel_embeddings.weight")[:2 * att_span]
    if "layer_norm" in model.encoder.norm_rel_ebd and "rel_ln_skipped" not in mut:
        rel = R._layer_norm(rel, W("encoder.LayerNorm.weight"), W("encoder.LayerNorm.bias"), eps, mut)
    idx = relative_index(model, S, mut)[None, None].expand(b, heads, S, S)
    share = bool(getattr(cfg, "share_att_key", False))

    def lin(t, name, bias=True, token_rows=True):
        y = lmm(t, W(name + ".weight").T, name) if token_rows else mm(t, W(name + ".weight").T)
        return y + W(name + ".bias") if bias else y

    def ln(t, name):
        return R._layer_norm(t, W(name + ".weight"), W(name + ".bias"), eps, mut)

    def pos_proj(name):
        t = lin(rel, name, bias="pos_proj_bias_dropped" not in mut, token_rows=False).view(2 * att_span, heads, dh).transpose(0, 1)      # [heads, 2 A, dh]
        return torch.roll(t, 1, dims=0) if "pos_heads_rolled" in mut else t

    for l in range(L):
        p = f"encoder.layer.{l}."
        a = p + "attention.self."
        q, k, v = (R._heads(lin(x, a + n), heads) for n in ("query_proj", "key_proj", "value_proj"))
        if "v_heads_rotated" in mut:
            v = torch.roll(v, 1, dims=1)
        s = mm(q, k.transpose(-1, -2))
        if "c2p" in terms and "drop_c2p" not in mut:
            full = mm(q, pos_proj(a + ("key_proj" if share else "pos_key_proj")).transpose(-1, -2)[None])               # [b, h, S(i), 2 A]
            s = s + torch.gather(full, -1, idx)
        if "p2c" in terms and "drop_p2c" not in mut:
            full = mm(k, pos_proj(a + ("query_proj" if share else "pos_query_proj")).transpose(-1, -2)[None])           # [b, h, S(j), 2 A]
            if "p2c_on_query_row" in mut:
                s = s + torch.gather(full, -1, idx)
            else:
                s = s + torch.gather(full, -1, idx.transpose(-1, -2)).transpose(-1, -2)       # [j, idx(i - j)] read at [i, j]
        ao = lin(_attention(s * scale, v, allow, mm), p + "attention.output.dense")
        x1 = ln(ao, p + "attention.output.LayerNorm") + x if "resid_after_ln" in mut else ln(x + ao, p + "attention.output.LayerNorm")
        f = lin(R._gelu(lin(x1, p + "intermediate.dense"), mut), p + "output.dense")
        x = ln(f, p + "output.LayerNorm") + x1 if "resid_after_ln" in mut else ln(x1 + f, p + "output.LayerNorm")
        if hidden_out is not None:
            hidden_out.append(x)
    return F.normalize(x[:, 0, :], p=2, dim=1, eps=1e-12)


# ------------------------------------------------------------------------------------------------------------------------
# models
# ------------------------------------------------------------------------------------------------------------------------
def deberta_config(hidden, layers, heads, inter, max_pos, vocab=R.VOCAB, position_buckets=POSITION_BUCKETS, **kw):
    from transformers import DebertaV2Config
    base = dict(vocab_size=vocab, hidden_size=hidden, num_hidden_layers=layers, num_attention_heads=heads, intermediate_size=inter,
                max_position_embeddings=max_pos, hidden_act="gelu", hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0,
                type_vocab_size=0, relative_attention=True, max_relative_positions=-1, pad_token_id=0, position_biased_input=False,
                pos_att_type=["p2c", "c2p"], position_buckets=position_buckets, share_att_key=True, norm_rel_ebd="layer_norm")
    base.update(kw)
    return DebertaV2Config(**base)


@torch.no_grad()
def build_model(cfg, regime, seed=0):
    from transformers import DebertaV2Model
    torch.manual_seed(seed)
    model = DebertaV2Model(cfg).eval()
    g = torch.Generator().manual_seed(seed + 41)
    rel = model.encoder.rel_embeddings.weight
    rel.copy_(torch.randn(rel.shape, generator=g))
    if hasattr(model.encoder, "LayerNorm"):
        model.encoder.LayerNorm.weight.copy_(0.5 + torch.rand(cfg.hidden_size, generator=g))
        model.encoder.LayerNorm.bias.copy_(0.5 * torch.randn(cfg.hidden_size, generator=g))
    kw = R.regime_kw("bert", regime, cfg.hidden_size)
    qk = kw.get("qk_scale", 1.0)
    for name, p in model.named_parameters():
        if name.endswith("intermediate.dense.weight"):
            p.mul_(R.FFN_GAIN[cfg.hidden_size])
    for name, mod in model.named_modules():
        leaf = name.rsplit(".", 1)[-1]
        if leaf in ("query_proj", "key_proj", "pos_key_proj", "pos_query_proj") and isinstance(mod, torch.nn.Linear):
            mod.weight.mul_(qk)
            mod.bias.copy_(torch.randn(mod.bias.shape, generator=g) * 0.2)
        elif kw and isinstance(mod, torch.nn.LayerNorm) and name != "encoder.LayerNorm":
            idx = torch.randperm(mod.weight.numel(), generator=g)[:4]
            mod.weight[idx] *= kw["ln_outlier"]
            mod.bias[idx] += 0.5 * kw["ln_outlier"] * torch.randn(4, generator=g)
    return model


@functools.lru_cache(maxsize=None)
def make_model(m: R.ModelSpec):
    return build_model(deberta_config(m.hidden, m.layers, m.heads, m.inter, m.max_pos, **VARIANTS[m.family]), m.regime, m.seed)


# ------------------------------------------------------------------------------------------------------------------------
# the cases: (Case, pooling).  Dispatch as encoder_ref.py states it, with what attn_disentangled changes (csrc/bert.hip):
#   attention fusion    never                                                       [attn_launches 0]
#   one launch          never: <= 32 token rows run layer by layer                  [used_one_launch False]
#   planes, LayerNorm fusion, unpad entry, CLS tail: untouched -- 2 LayerNorm-fused launches per token layer once T >= 192 on bf16x3
# ------------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class DBCase:
    case: R.Case
    pooling: str

    @property
    def id(self):
        return f"{self.case.id}-{self.pooling}"

    @property
    def regime(self):
        return self.case.model.regime


DEBERTA_CASES = []
L = 3


def add(id, b, S, lengths, regime="peaked", poolings=("cls",), planes=False, family="deberta", max_pos=0, mask="right", holes=(), **kw):
    m = R.ModelSpec(family, 128, L, 2, 512, regime, max_pos=max_pos or (64 if S <= 64 else 128))
    bs = R.BatchSpec("bert" if family == "deberta:posbiased" else "deberta", b, S, None if lengths is None else tuple(lengths), mask, tuple(holes))
    if kw.get("path") == "packed":
        kw["tokens"] = sum(lengths)
    for pooling in poolings:
        token_layers = L if pooling == "mean" else L - 1
        c = R.Case(id, m, bs, "deberta", one_launch=False, attn_launches=0, ln_launches=2 * token_layers if planes else 0, **kw)
        DEBERTA_CASES.append(DBCase(c, pooling))


BOTH = ("cls", "mean")
LEN9 = (24, 5, 17, 11, 24, 9, 20, 13, 16)                # 139 rows: fp32 activations, CLS attention on 32-key tiles
LEN40 = (40, 3, 31, 17, 36, 25, 38, 14)                  # 204 rows: planes, two key tiles, buckets to +-7
LEN70 = (70, 64, 32, 1, 33)                              # 200 rows: three query / key tiles, tile edges, a lone token
LEN24 = (24, 11, 17, 5, 24, 9, 24, 20, 13)               # 9 x 24 = 216 padded rows
add("db_small_T32", 4, 8, (8, 5, 1, 7), poolings=BOTH, note="32 token rows: layer by layer, never the one launch")
add("db_ragged9", 9, 24, LEN9, poolings=BOTH, path="packed", note="139 rows packed, fp32 activations; T >= 4 b")
add("db_S40_planes", 8, 40, LEN40, poolings=BOTH, planes=True, path="packed", note="204 rows on planes, longest 40: two key tiles")
add("db_S40_f32", 8, 40, LEN40, path="packed", arith="f32", sens=False, note='arith="f32": no planes')
add("db_S70_flat", 5, 70, LEN70, regime="flat", poolings=BOTH, planes=True, path="packed", note="three key tiles; max_position_embeddings 128")
add("db_padded_no_mask", 9, 24, None, poolings=BOTH, planes=True, mask="none", sens=False, note="216 padded rows, no mask")
add("db_holes", 9, 24, LEN24, poolings=BOTH, planes=True, mask="holes", holes=R.HOLES, path="padded_mask",
    note="a mask with holes: the [b, S] forward with the mask; distances are between row indices")
add("db_T_lt_4b", 100, 3, R.cyc((3, 2, 3, 1, 3), 100), planes=True, path="packed", sens=False,
    note="240 rows < 4 b: the last layer projects Q for every row, the c2p rows of the CLS queries are gathered")
add("db_noshare", 8, 40, LEN40, planes=True, path="packed", family="deberta:noshare", note="share_att_key off: pos_key_proj / pos_query_proj")
add("db_c2p_only", 8, 40, LEN40, planes=True, path="packed", family="deberta:c2p", note="scale_factor 2, a zero PQ")
add("db_p2c_only", 8, 40, LEN40, planes=True, path="packed", family="deberta:p2c", note="scale_factor 2, a zero PK")
add("db_posbiased_types", 8, 40, LEN40, planes=True, path="packed", family="deberta:posbiased", sens=False,
    note="position_biased_input with a type table: the embedding kernel's real tables")

BY_ID = {c.id: c for c in DEBERTA_CASES}
assert len(BY_ID) == len(DEBERTA_CASES)


# ------------------------------------------------------------------------------------------------------------------------
# evaluation (cached per input)
# ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _hidden(m, bs, dtype, chunked, mut, sqrt32=False):
    ids, types, mask = R.make_batch(bs)
    hs = []
    cls = deberta_forward(make_model(m), ids, types, mask, dtype=dtype, mm=R.mm_chunk16 if chunked else R.mm_plain, mut=mut, hidden_out=hs,
                          sqrt32=sqrt32)
    return cls, hs[-1]


def _admitted(bs):
    _, _, mask = R.make_batch(bs)
    return torch.ones((bs.b, bs.S), dtype=torch.bool) if mask is None else mask.bool()


def _pool(mc, cls, h):
    return cls if mc.pooling == "cls" else P.masked_mean_normalize(h, _admitted(mc.case.batch))


def _pooled(mc, dtype=torch.float64, chunked=False, mut=(), sqrt32=False):
    c = mc.case
    return _pool(mc, *_hidden(c.model, c.batch, dtype, chunked, tuple(mut), sqrt32))


def reference(mc):
    """fp64 unit-norm vectors [b, H] of the case under its pooling (computed once per input, shared; do not modify)"""
    return _pooled(mc)


def fp32_instance(mc, chunked=False):
    return _pooled(mc, torch.float32, chunked)


@functools.lru_cache(maxsize=None)
def _transformers_hidden(m, bs, double):
    ids, types, mask = R.make_batch(bs)
    model = make_model(m)
    if double:
        model = copy.deepcopy(model).double()
    kw = dict(input_ids=ids)
    if mask is not None:
        kw["attention_mask"] = mask
    if types is not None:
        kw["token_type_ids"] = types
    with torch.no_grad():
        return model(**kw).last_hidden_state


def transformers_instance(mc, double=False):
    h = _transformers_hidden(mc.case.model, mc.case.batch, double)
    return _pool(mc, F.normalize(h[:, 0, :], p=2, dim=1), h)


def deviation(mc, got):
    return float((got.detach().double().cpu() - reference(mc)).abs().max())


def applicable(name, mc):
    """can this mistake change anything on this case's input?"""
    c = mc.case
    _, _, mask = R.make_batch(c.batch)
    longest = c.batch.S if mask is None else int(mask.sum(1).max())
    terms = _terms(make_model(c.model).config)
    if name == "admit_first_pad":
        return mask is not None and bool((mask == 0).any())
    if name in ("drop_c2p",):
        return "c2p" in terms and longest > 1
    if name in ("drop_p2c", "p2c_on_query_row"):
        return "p2c" in terms and longest > 1
    if name == "no_log_bucket":
        return longest > POSITION_BUCKETS // 2 + 1              # bucket(d) = d up to |d| = mid
    if name in POS_MUTANTS or name == "drop_last_key":
        return longest > 1
    return True


def mutant_distance(mc, name):
    return float((_pooled(mc, mut=(name,)) - reference(mc)).abs().max())


# ------------------------------------------------------------------------------------------------------------------------
# bounds
# ------------------------------------------------------------------------------------------------------------------------
# FP32_DEV_DEBERTA[regime]: worst max-abs deviation from fp64 of the three fp32 instances over the regime's DEBERTA_CASES (both
# poolings), measured on the CPU and rounded up to one digit; tests/test_encoder_deberta_cpu.py asserts every case stays within
# encoder_ref.ADMISSION x the figure and prints this table.  The worst cases at the time of writing (16 CPU threads):
#
#   regime   torch fp32                 K-chunks of 16            transformers fp32         FP32_DEV_DEBERTA   16 x
#   flat     6.2e-08 db_S70_flat-cls    4.3e-08 db_S70_flat-cls   6.1e-08 db_S70_flat-cls   7e-8               1.1e-6
#   peaked   1.7e-07 db_holes-cls       1.5e-07 db_T_lt_4b-cls    1.5e-07 db_T_lt_4b-cls    2e-7               3.2e-6
#
# The reference is transformers' DebertaV2Model in fp64 to 4e-10 on every case -- the residue of its fp32 root of 3 d -- and to 4e-16
# once the root is taken its way (sqrt32).  The least visible mutant is gelu_tanh (32 bounds); the least visible mistake of the
# position terms, pos_proj_bias_dropped, sits 3000 bounds out.
FP32_DEV_DEBERTA = {
    "flat": 7e-8,
    "peaked": 2e-7,
}


def device_bound(mc):
    bound = R.KERNEL_FACTOR * FP32_DEV_DEBERTA[mc.regime]
    assert bound <= R.DEVICE_BOUND_CEILING, (mc.id, bound)
    return bound
