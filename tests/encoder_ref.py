"""Shared by tests/test_encoder_ref_cpu.py and tests/test_encoder_reference_gpu.py: the encoder forward stated once in plain
torch, in any dtype, straight from a `state_dict` and the model's config; the mutants of that forward; and the case grid both
modules walk.

  reference    `reference(case)` = the fp64 forward of the case's family on the case's batch: unit-norm CLS vectors [b, H]
  fp32 instances (the yardstick): the same functions in fp32; the same in fp32 with every matmul summed in K-chunks of 16 one
               after the other (a second CORRECT fp32 implementation with another summation order); transformers fp32 eager
  mutants      switches on the fp64 forward, each one a plausible kernel mistake (MUTANTS)
  bounds       FP32_DEV[(family, regime)] = the worst deviation of the three fp32 instances from fp64 over the group's cases,
               measured on the CPU (tests/test_encoder_ref_cpu.py asserts the constants hold and prints the table);
               a case is in the grid only if every instance stays within ADMISSION x the figure; the device is held to
               KERNEL_FACTOR x the figure (device_bound), never more than DEVICE_BOUND_CEILING.  No bound comes from a device
               observation.

Key masks are additive -inf and the softmax subtracts the row maximum; a query row without any admitted key gets zero
probabilities (only padding queries and all-masked sequences have such rows; an all-masked sequence is a legal INPUT, its own
output row is not compared: `compared_rows`).

ModernBERT's rotary tables are model constants: ModernBertRotaryEmbedding computes inv_freq, the angles and cos / sin in fp32
whatever the model's dtype, and the device builds the same fp32 tables -- the reference takes them as given, in every dtype.
"""
import functools
import math
from dataclasses import dataclass
from typing import Optional, Tuple

import torch
import torch.nn.functional as F

from oracle import bert_oracle

VOCAB = 2000

# ------------------------------------------------------------------------------------------------------------------------
# matmuls
# ------------------------------------------------------------------------------------------------------------------------

def mm_plain(a, b):
    return a @ b


def mm_chunk16(a, b):
    """a[..., K] @ b[..., K, N] with the K sum taken in chunks of 16, one chunk after the other"""
    K = a.shape[-1]
    acc = a[..., 0:16] @ b[..., 0:16, :]
    for k0 in range(16, K, 16):
        acc = acc + a[..., k0:k0 + 16] @ b[..., k0:k0 + 16, :]
    return acc


# ------------------------------------------------------------------------------------------------------------------------
# mutants: name -> (families it applies to, what the mistake is)
# ------------------------------------------------------------------------------------------------------------------------
BERT_FAMILIES = ("bert", "electra", "distilbert", "roberta", "xlm-roberta")
ALL = BERT_FAMILIES + ("modernbert",)
MUTANTS = {
    "gelu_tanh":        (ALL, "tanh-approximate GELU in place of the erf form"),
    "ln_eps_1e-5":      (("bert", "electra", "distilbert"), "LayerNorm eps 1e-5 in place of the config's 1e-12"),
    # (eps 0 against BERT's 1e-12 changes a variance of order one in its 12th digit: no mistake in any arithmetic at hand, so the
    #  switch applies where the config's eps is 1e-5)
    "ln_eps_0":         (("roberta", "xlm-roberta", "modernbert"), "LayerNorm eps 0 in place of the config's 1e-5"),
    "ln_var_h-1":       (ALL, "LayerNorm variance divided by H - 1"),
    "scale_hidden":     (ALL, "softmax scale 1/sqrt(hidden) in place of 1/sqrt(head dim)"),
    "admit_first_pad":  (ALL, "the first masked key of every sequence admitted"),
    "drop_last_key":    (ALL, "the last real key of every sequence (of more than one token) dropped"),
    "no_types":         (("bert", "electra"), "token types ignored (type 0 everywhere)"),
    "pos_shift":        (BERT_FAMILIES, "positions shifted by one"),
    "resid_after_ln":   (ALL, "residual taken after the LayerNorm instead of before: post-norm families LN(sublayer) + x in "
                              "place of LN(x + sublayer), ModernBERT norm(x) + sublayer(norm(x)) in place of x + ..."),
    "v_heads_rotated":  (ALL, "the heads' V slices rotated by one head"),
    "window_plus":      (("modernbert",), "local window half-width + 1"),
    "window_minus":     (("modernbert",), "local window half-width - 1"),
    "rope_theta_global": (("modernbert",), "RoPE theta of the global layers used in the local ones"),
    "rope_interleaved": (("modernbert",), "RoPE pairs interleaved (2i, 2i+1) instead of half-split (i, i + dh/2)"),
    "geglu_swapped":    (("modernbert",), "gate and input halves of GeGLU swapped"),
    "layer0_norm":      (("modernbert",), "layer 0's missing attention norm applied (unit gain)"),
    "roberta_offset_1": (("roberta", "xlm-roberta"), "position offset padding_idx in place of padding_idx + 1"),
}


# ------------------------------------------------------------------------------------------------------------------------
# the forward
# ------------------------------------------------------------------------------------------------------------------------

def _layer_norm(x, g, b, eps, mut):
    if "ln_eps_1e-5" in mut:
        eps = 1e-5
    if "ln_eps_0" in mut:
        eps = 0.0
    mean = x.mean(-1, keepdim=True)
    d = x - mean
    var = (d * d).sum(-1, keepdim=True) / (x.shape[-1] - 1 if "ln_var_h-1" in mut else x.shape[-1])
    y = d / torch.sqrt(var + eps) * g
    return y if b is None else y + b


def _gelu(x, mut):
    if "gelu_tanh" in mut:
        return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def _key_mask(mask, b, S, mut):
    """bool [b, S]: the keys a query may see"""
    keep = torch.ones((b, S), dtype=torch.bool) if mask is None else mask.bool().clone()
    if mask is not None and "admit_first_pad" in mut:
        for i in range(b):
            gone = (~mask[i].bool()).nonzero()
            if len(gone):
                keep[i, int(gone[0])] = True
    if "drop_last_key" in mut:
        src = torch.ones((b, S), dtype=torch.bool) if mask is None else mask.bool()
        for i in range(b):
            real = src[i].nonzero()
            if len(real) > 1:
                keep[i, int(real[-1])] = False
    return keep


def _attention(q, k, v, allow, scale, mm, probs_out):
    """q, k, v [b, h, S, dh]; allow bool [b, 1 | h, S, S] -> context [b, S, h * dh]"""
    s = mm(q, k.transpose(-1, -2)) * scale
    s = s + torch.zeros_like(s).masked_fill(~allow, float("-inf"))          # additive -inf key mask
    m = s.max(-1, keepdim=True).values
    m = torch.where(torch.isinf(m), torch.zeros_like(m), m)                # (a row without keys: exp(-inf - 0) = 0 everywhere)
    e = torch.exp(s - m)
    den = e.sum(-1, keepdim=True)
    p = e / torch.where(den > 0, den, torch.ones_like(den))
    if probs_out is not None:
        probs_out.append(p)
    ctx = mm(p, v)
    b, h, S, dh = ctx.shape
    return ctx.transpose(1, 2).reshape(b, S, h * dh)


def _heads(x, heads):
    b, S, H = x.shape
    return x.view(b, S, heads, H // heads).transpose(1, 2)


def _lin_mm(mm, lin_mm):
    """the matmul of the nn.Linear layers: `lin_mm(t, w_t, name)` where a caller hooks it (name = the layer's parameter prefix;
    tests/encoder_f16x2_ref.py states the fp16x2 arithmetic of the token-row GEMMs through it), else `mm` like every other matmul"""
    return (lambda t, w_t, name: mm(t, w_t)) if lin_mm is None else lin_mm


BERT_NAMES = {"word": "embeddings.word_embeddings.weight", "pos": "embeddings.position_embeddings.weight",
              "type": "embeddings.token_type_embeddings.weight", "eln": "embeddings.LayerNorm",
              "layer": "encoder.layer.{}.", "q": "attention.self.query", "k": "attention.self.key",
              "v": "attention.self.value", "ao": "attention.output.dense", "ln1": "attention.output.LayerNorm",
              "ff1": "intermediate.dense", "ff2": "output.dense", "ln2": "output.LayerNorm"}
DISTIL_NAMES = {"word": "embeddings.word_embeddings.weight", "pos": "embeddings.position_embeddings.weight", "type": None,
                "eln": "embeddings.LayerNorm", "layer": "transformer.layer.{}.", "q": "attention.q_lin", "k": "attention.k_lin",
                "v": "attention.v_lin", "ao": "attention.out_lin", "ln1": "sa_layer_norm", "ff1": "ffn.lin1", "ff2": "ffn.lin2",
                "ln2": "output_layer_norm"}


@torch.no_grad()
def post_norm_forward(sd, cfg, ids, types, mask, dtype=torch.float64, mm=mm_plain, mut=(), names=BERT_NAMES, positions=None,
                      hidden_out=None, probs_out=None, lin_mm=None):
    """The BERT block (post-norm, erf GELU, absolute positions) from a state_dict: BERT / ELECTRA (names=BERT_NAMES),
    DistilBERT (DISTIL_NAMES, no token types); `positions` [b, S] overrides arange(S) (RoBERTa).  hidden_out / probs_out: lists
    that receive the hidden states after the embeddings and after every layer / every layer's attention probabilities.
    lin_mm: see _lin_mm (the attention's score and P.V matmuls keep `mm`)."""
    W = lambda k: sd[k].to(dtype)
    lmm = _lin_mm(mm, lin_mm)
    if names is DISTIL_NAMES:
        H, L, heads, eps = cfg.dim, cfg.n_layers, cfg.n_heads, 1e-12
    else:
        H, L, heads, eps = cfg.hidden_size, cfg.num_hidden_layers, cfg.num_attention_heads, float(cfg.layer_norm_eps)
    b, S = ids.shape
    pos = torch.arange(S)[None, :].expand(b, S) if positions is None else positions
    if "pos_shift" in mut:
        pos = pos + 1
    x = W(names["word"])[ids] + W(names["pos"])[pos]
    if names["type"] is not None:
        tt = torch.zeros_like(ids) if (types is None or "no_types" in mut) else types
        x = x + W(names["type"])[tt]
    x = _layer_norm(x, W(names["eln"] + ".weight"), W(names["eln"] + ".bias"), eps, mut)
    if hidden_out is not None:
        hidden_out.append(x)
    allow = _key_mask(mask, b, S, mut)[:, None, None, :].expand(b, 1, S, S)
    dh = H // heads
    scale = 1.0 / math.sqrt(H if "scale_hidden" in mut else dh)

    def lin(t, name):
        return lmm(t, W(name + ".weight").T, name) + W(name + ".bias")

    def ln(t, name):
        return _layer_norm(t, W(name + ".weight"), W(name + ".bias"), eps, mut)

    for l in range(L):
        p = names["layer"].format(l)
        q, k, v = (_heads(lin(x, p + names[n]), heads) for n in ("q", "k", "v"))
        if "v_heads_rotated" in mut:
            v = torch.roll(v, 1, dims=1)
        ctx = _attention(q, k, v, allow, scale, mm, probs_out)
        ao = lin(ctx, p + names["ao"])
        x1 = ln(ao, p + names["ln1"]) + x if "resid_after_ln" in mut else ln(x + ao, p + names["ln1"])
        f = lin(_gelu(lin(x1, p + names["ff1"]), mut), p + names["ff2"])
        x = ln(f, p + names["ln2"]) + x1 if "resid_after_ln" in mut else ln(x1 + f, p + names["ln2"])
        if hidden_out is not None:
            hidden_out.append(x)
    return F.normalize(x[:, 0, :], p=2, dim=1, eps=1e-12)


def bert_forward(sd, cfg, ids, types, mask, **kw):
    return post_norm_forward(sd, cfg, ids, types, mask, names=BERT_NAMES, **kw)


electra_forward = bert_forward


def distilbert_forward(sd, cfg, ids, types, mask, **kw):
    return post_norm_forward(sd, cfg, ids, None, mask, names=DISTIL_NAMES, **kw)


def roberta_forward(sd, cfg, ids, types, mask, mut=(), **kw):
    """RoBERTa / XLM-R: positions count from padding_idx + 1 over the non-pad tokens (pad tokens sit at padding_idx)"""
    pad = int(cfg.pad_token_id)
    real = (ids != pad).long()
    off = pad - 1 if "roberta_offset_1" in mut else pad
    positions = torch.cumsum(real, dim=1) * real + off * real + pad * (1 - real)
    return post_norm_forward(sd, cfg, ids, None, mask, names=BERT_NAMES, positions=positions, mut=mut, **kw)


def _rope_tables(cfg, S, key, dtype):
    """cos / sin [S, dh] as ModernBertRotaryEmbedding builds them: fp32 throughout, then cast"""
    dh = cfg.hidden_size // cfg.num_attention_heads
    theta = float(cfg.rope_parameters[key]["rope_theta"])
    inv_freq = 1.0 / (theta ** (torch.arange(0, dh, 2, dtype=torch.int64).to(dtype=torch.float) / dh))
    freqs = (inv_freq[:, None].float() @ torch.arange(S, dtype=torch.float32)[None, :]).transpose(0, 1)
    emb = torch.cat((freqs, freqs), dim=-1)
    return emb.cos().to(dtype), emb.sin().to(dtype)


def _rope(x, cos, sin, interleaved):
    dh = x.shape[-1]
    if interleaved:                                       # pairs (2i, 2i+1) rotated by angle i
        c, s = cos[..., :dh // 2], sin[..., :dh // 2]
        a, bb = x[..., 0::2], x[..., 1::2]
        return torch.stack((a * c - bb * s, bb * c + a * s), dim=-1).reshape(x.shape)
    x1, x2 = x[..., :dh // 2], x[..., dh // 2:]
    return x * cos + torch.cat((-x2, x1), dim=-1) * sin


@torch.no_grad()
def modernbert_forward(sd, cfg, ids, types, mask, dtype=torch.float64, mm=mm_plain, mut=(), hidden_out=None, probs_out=None,
                       lin_mm=None):
    """ModernBERT: RoPE with the per-layer theta, global attention every n-th layer and the |q - k| <= local/2 window otherwise,
    pre-norm with no attention norm in layer 0, GeGLU with erf GELU, optional biases, the final norm."""
    W = lambda k: sd[k].to(dtype)
    O = lambda k: sd[k].to(dtype) if k in sd else None
    lmm = _lin_mm(mm, lin_mm)
    H, L, heads, eps = cfg.hidden_size, cfg.num_hidden_layers, cfg.num_attention_heads, float(cfg.norm_eps)
    b, S = ids.shape
    dh = H // heads
    scale = 1.0 / math.sqrt(H if "scale_hidden" in mut else dh)

    def lin(t, name):
        y = lmm(t, W(name + ".weight").T, name)
        bias = O(name + ".bias")
        return y if bias is None else y + bias

    def ln(t, name):
        return _layer_norm(t, W(name + ".weight"), O(name + ".bias"), eps, mut)

    x = ln(W("embeddings.tok_embeddings.weight")[ids], "embeddings.norm")
    if hidden_out is not None:
        hidden_out.append(x)
    keys = _key_mask(mask, b, S, mut)[:, None, None, :]
    half = int(cfg.sliding_window) + (1 if "window_plus" in mut else 0) - (1 if "window_minus" in mut else 0)
    idx = torch.arange(S)
    window = ((idx[:, None] - idx[None, :]).abs() <= half)[None, None]
    for l in range(L):
        kind = cfg.layer_types[l]
        if l == 0:
            a_in = _layer_norm(x, torch.ones(H, dtype=dtype), None, eps, mut) if "layer0_norm" in mut else x
        else:
            a_in = ln(x, f"layers.{l}.attn_norm")
        qkv = lin(a_in, f"layers.{l}.attn.Wqkv").view(b, S, 3, heads, dh)
        q, k, v = (qkv[:, :, i].transpose(1, 2) for i in range(3))
        table = "full_attention" if (kind == "full_attention" or "rope_theta_global" in mut) else "sliding_attention"
        cos, sin = _rope_tables(cfg, S, table, dtype)
        q, k = _rope(q, cos, sin, "rope_interleaved" in mut), _rope(k, cos, sin, "rope_interleaved" in mut)
        if "v_heads_rotated" in mut:
            v = torch.roll(v, 1, dims=1)
        allow = keys.expand(b, 1, S, S) if kind == "full_attention" else (keys & window).expand(b, 1, S, S)
        ao = lin(_attention(q, k, v, allow, scale, mm, probs_out), f"layers.{l}.attn.Wo")
        x = (a_in if "resid_after_ln" in mut else x) + ao
        n = ln(x, f"layers.{l}.mlp_norm")
        inp, gate = lin(n, f"layers.{l}.mlp.Wi").chunk(2, dim=-1)
        if "geglu_swapped" in mut:
            inp, gate = gate, inp
        x = (n if "resid_after_ln" in mut else x) + lin(_gelu(inp, mut) * gate, f"layers.{l}.mlp.Wo")
        if hidden_out is not None:
            hidden_out.append(x)
    x = ln(x, "final_norm")
    return F.normalize(x[:, 0, :], p=2, dim=1, eps=1e-12)


FORWARD = {"bert": bert_forward, "electra": electra_forward, "distilbert": distilbert_forward, "roberta": roberta_forward,
           "xlm-roberta": roberta_forward, "modernbert": modernbert_forward}


# ------------------------------------------------------------------------------------------------------------------------
# regimes, models, batches
# ------------------------------------------------------------------------------------------------------------------------
# flat    transformers' own init (softmax within a few percent of uniform)
# peaked  query / key projections scaled (x8 below width 256, x5 from there: the figures of tests/test_encoder_gpu.py) and four
#         LayerNorm outlier channels of gain x LN_OUTLIER.  tests/test_encoder_gpu.py uses gain x12, under which a correct fp32
#         forward of the three-layer width-768 model is 2.3e-6 from fp64 -- 16 x that would pass the 1e-5 ceiling, so this grid
#         uses the softer gain below (the mean max attention probability stays above the thresholds: asserted on the CPU).
#         The FFN-up weights are scaled as well (FFN_GAIN) so that the GELU arguments have a spread of order one, as in trained
#         checkpoints: at the init's ~0.2 the tanh form of GELU is indistinguishable from the erf form.
# scaled  ModernBERT: Linear weights x4 (logits away from 0) and LayerNorm gains drawn from U(0.5, 1.5)
LN_OUTLIER = 3.0
LN_OUTLIER_WIDE = 2.0
FFN_GAIN = {128: 4.0, 384: 2.5, 768: 2.0, 1024: 1.5}


def regime_kw(family, regime, hidden):
    if family == "modernbert":
        assert regime == "scaled"
        return {"init_scale": 4.0, "norm_jitter": 0.5}
    if regime == "flat":
        return {}
    assert regime in ("peaked", "peaked_wide") and family in ("bert", "electra", "distilbert")
    assert (regime == "peaked_wide") == (hidden >= 768)
    return {"qk_scale": 10.0 if hidden < 256 else 5.0, "ln_outlier": LN_OUTLIER_WIDE if hidden >= 768 else LN_OUTLIER}


@dataclass(frozen=True)
class ModelSpec:
    family: str
    hidden: int
    layers: int
    heads: int
    inter: int
    regime: str
    local: int = 0                  # ModernBERT: local_attention (the window is |q - k| <= local / 2)
    global_every: int = 0
    max_pos: int = 0
    seed: int = 0


@functools.lru_cache(maxsize=None)
def make_model(m: ModelSpec):
    model = _make_model(m)
    if m.regime.startswith("peaked"):
        with torch.no_grad():
            for name, p in model.named_parameters():
                if name.endswith("intermediate.dense.weight") or name.endswith("ffn.lin1.weight"):
                    p.mul_(FFN_GAIN[m.hidden])
    return model


def _make_model(m: ModelSpec):
    kw = regime_kw(m.family, m.regime, m.hidden)
    if m.family == "bert":
        return bert_oracle.make_bert(m.hidden, m.layers, m.heads, m.inter, vocab=VOCAB, max_pos=m.max_pos, seed=m.seed, **kw)
    if m.family == "electra":
        return bert_oracle.make_electra(m.hidden, m.layers, m.heads, m.inter, vocab=VOCAB, max_pos=m.max_pos, seed=m.seed, **kw)
    if m.family == "distilbert":
        return bert_oracle.make_distilbert(m.hidden, m.layers, m.heads, m.inter, vocab=VOCAB, max_pos=m.max_pos, seed=m.seed, **kw)
    if m.family in ("roberta", "xlm-roberta"):
        return bert_oracle.make_roberta(m.hidden, m.layers, m.heads, m.inter, vocab=VOCAB, max_pos=m.max_pos, seed=m.seed,
                                        model_type=m.family)
    return bert_oracle.make_modernbert(m.hidden, m.layers, m.heads, m.inter, vocab=VOCAB, max_pos=m.max_pos,
                                       local_attention=m.local, global_every=m.global_every, seed=m.seed, **kw)


@dataclass(frozen=True)
class BatchSpec:
    """b rows of S positions; `lengths` fixes every row's real-token count (None: all S).  mask: "none" (no mask passed; every
    row full), "ones" (all ones passed explicitly; every row full), "right" (right-padded), "left" (left-padded),
    "holes" (right-padded, then the (row, col) positions of `holes` masked out; a row whose `lengths` entry is 0 is all-masked)."""
    family: str
    b: int
    S: int
    lengths: Optional[Tuple[int, ...]] = None
    mask: str = "right"
    holes: Tuple[Tuple[int, int], ...] = ()
    seed: int = 1


PAD = {"roberta": 1, "xlm-roberta": 1}
FIRST = {"roberta": 0, "xlm-roberta": 0, "modernbert": 1}


@functools.lru_cache(maxsize=None)
def make_batch(bs: BatchSpec):
    """-> ids, types (None for the families without), mask (None for "none"); every length as the spec states it"""
    g = torch.Generator().manual_seed(bs.seed)
    b, S = bs.b, bs.S
    lens = torch.tensor(bs.lengths if bs.lengths is not None else (S,) * b)
    assert len(lens) == b and int(lens.max()) <= S and int(lens.min()) >= 0
    ids = torch.randint(1000, VOCAB, (b, S), generator=g)
    ids[:, 0] = FIRST.get(bs.family, 101)
    mask = (torch.arange(S)[None, :] < lens[:, None]).long()
    types = torch.zeros((b, S), dtype=torch.int64)
    for i in range(b):
        types[i, max(1, int(lens[i]) // 2):] = 1          # second "sentence" = the back half of the real tokens
    if bs.family in PAD:
        for i in range(b):
            if lens[i] > 1:
                ids[i, lens[i] - 1] = 2                   # </s>
    ids = torch.where(mask.bool(), ids, torch.full_like(ids, PAD.get(bs.family, 0)))
    if bs.mask in ("none", "ones"):
        assert int(lens.min()) == S
    elif bs.mask == "left":
        ids, types, mask = (torch.flip(t, dims=[1]).contiguous() for t in (ids, types, mask))
    elif bs.mask == "holes":
        for (r, c) in bs.holes:
            assert mask[r, c] == 1 and bs.family not in PAD
            mask[r, c] = 0
    else:
        assert bs.mask == "right" and int(lens.min()) >= 1
    if bs.family not in ("bert", "electra"):
        types = None
    return ids, types, (None if bs.mask == "none" else mask)


def compared_rows(bs: BatchSpec):
    """bool [b]: every row but the all-masked ones"""
    _, _, mask = make_batch(bs)
    return torch.ones(bs.b, dtype=torch.bool) if mask is None else mask.sum(1) > 0


# ------------------------------------------------------------------------------------------------------------------------
# the cases
# ------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    id: str
    model: ModelSpec
    batch: BatchSpec
    branch: str                     # the expected-branch group (see BRANCHES)
    # how the device call is made
    arith: Optional[str] = None     # "f32" | None (the bf16x3 default)
    ln_fusion: int = 1              # ac_gemm_set_ln_fusion
    env: Tuple[Tuple[str, str], ...] = ()
    layered: bool = False           # AC_BERT_LAYERED (force_layered)
    unpad: bool = True
    ldo_extra: int = 0              # output rows this many floats wider than H
    max_tokens: int = 0             # encoder.MAX_TOKENS for the call (0: untouched)
    # what must be observed
    one_launch: bool = False        # used_one_launch of ac_bert_encode_cls_opts
    ln_launches: int = 0            # ac_gemm_ln_fusion_launches delta
    attn_launches: int = 0          # ac_gemm_qkv_attn_launches delta
    path: Optional[str] = None      # path of ac_bert_encode_cls_unpad ("packed" | "padded" | "padded_mask"); None: entry not taken
    tokens: int = -1                # enc.last_tokens (-1: b * S)
    sens: bool = True               # mutant distances are computed on this case's input (off for the wide / long ones: CPU time)
    note: str = ""

    @property
    def group(self):
        return (self.model.family, self.model.regime)


CASES = []


def _lens_sum(lengths, S, b):
    return sum(lengths) if lengths is not None else b * S


def add(id, family, hidden, layers, heads, inter, b, S, lengths, regime, branch, mask="right", holes=(), local=0, global_every=0,
        seed=0, bseed=1, **kw):
    extra = 2 if family in PAD else 0
    m = ModelSpec(family, hidden, layers, heads, inter, regime, local, global_every, max_pos=max(S + 1 + extra, 64), seed=seed)
    bs = BatchSpec(family, b, S, None if lengths is None else tuple(lengths), mask, tuple(holes), bseed)
    packs = kw.get("path") == "packed" or (family == "modernbert" and mask == "right" and kw.get("unpad", True))
    if packs and "tokens" not in kw:
        kw["tokens"] = _lens_sum(lengths, S, b)          # the padding-free path runs the real tokens only
    CASES.append(Case(id, m, bs, branch, **kw))


def cyc(values, n):
    return tuple(values[i % len(values)] for i in range(n))


FUSION_OFF = (("AC_QKV_ATTN_FUSION", "0"),)
XCHG_OFF = (("AC_QKV_ATTN_EXCHANGE", "0"),)
TAIL_OFF = (("AC_BERT_TAIL_FUSED", "0"),)
L = 3            # first, middle and CLS-only last: every layer-loop branch of bert_encode_impl

# Dispatch conditions read off csrc/bert.hip (bert_encode_impl, encode_plan, ac_bert_encode_cls_opts, ac_bert_encode_cls_unpad),
# csrc/gemm_plan.h (the GEMM side: linear_takes_planes, pipe_ln_shape, qkv_attn_shape and the thresholds they share -- the rules
# live there and are not restated here; the lines below only name which counter shows each branch), csrc/gemm_pipe.hip (the
# residency halves of qkv_attn_applies, pipe_ln_applies) and encoder.py (_run_chunks), with T = the token rows of the forward
# (b * S, or the real tokens on the packed path):
#   one launch          b * S <= 32, head dim 64, not AC_BERT_LAYERED                      [used_one_launch]
#   unpad entry         a mask is passed, S > 1, b * S > 32: packed (ones are a prefix of every row, some row short), padded
#                       (every row full), padded_mask (anything else: left padding, holes, an empty row)   [path, total_tokens]
#   planes              gemm_plan.h linear_takes_planes(T, H, H) and (T, H, I)             [no counter: T and arith decide]
#   LayerNorm fusion    planes, layers > 1, fusion on, gemm_plan.h pipe_ln_shape, the grid resident at once
#                       -> 2 launches per layer but the last                               [ac_gemm_ln_fusion_launches]
#   attention fusion    planes, layers > 1, head dim 64, packed or no mask, longest <= 64  -> 1 launch per layer but the last
#                                                                                          [ac_gemm_qkv_attn_launches]
#   in-launch exchange  fusion on, AC_QKV_ATTN_EXCHANGE != 0, ceil(T / 256) * heads <= resident capacity; else the boundary launch
#   last layer          q_cls_only: T >= 4 b; CLS attention on 32-key tiles: head dim 64 and longest <= 32 (no counter: the shapes
#                       below are chosen by these two conditions); AC_BERT_TAIL_FUSED
# ---- one launch against layered ------------------------------------------------------------------------------------------
add("ol_T32_ragged_len1", "bert", 128, L, 2, 512, 4, 8, (8, 5, 1, 7), "peaked", "one_launch", one_launch=True,
    note="T = 32 exactly, a sequence of one token")
add("ol_T32_forced_layered", "bert", 128, L, 2, 512, 4, 8, (8, 5, 1, 7), "peaked", "small_layered", layered=True,
    note="same batch under AC_BERT_LAYERED: fp32 activations, [b, S] rows with the mask; T = 32 = 4 b: q_cls_only, 32-key CLS tiles")
add("ol_T33_packed", "bert", 128, L, 2, 512, 3, 11, (11, 7, 4), "peaked", "small_layered", path="packed",
    note="b * S = 33: layered, packed to 22 rows")
add("ol_b1_S1", "bert", 128, L, 2, 512, 1, 1, None, "peaked", "one_launch", mask="none", one_launch=True, sens=False,
    note="a CLS token alone: one key")
add("ol_768_ragged", "bert", 768, L, 12, 3072, 2, 16, (16, 9), "peaked_wide", "one_launch", one_launch=True, sens=False)
add("ol_768_flat_S32", "bert", 768, L, 12, 3072, 1, 32, None, "flat", "one_launch", mask="none", one_launch=True, sens=False)
add("ol_128_flat", "bert", 128, L, 2, 512, 3, 10, (10, 1, 6), "flat", "one_launch", one_launch=True)
add("dh32_small_is_layered", "bert", 384, L, 12, 1536, 2, 12, (12, 7), "peaked", "small_layered", sens=False,
    note="head dim 32: the one-launch kernel declines, layered on [b, S] rows with the mask; T = 24 >= 4 b")
# ---- without planes against with planes; the T = 191 / 192 edge of planes, LayerNorm fusion and attention fusion ------------
LEN191 = (32, 31, 30, 20, 25, 17, 19, 17)
LEN192 = (32, 31, 30, 20, 25, 17, 19, 18)
add("T191_no_planes", "bert", 128, L, 2, 512, 8, 32, LEN191, "peaked", "small_layered", path="packed",
    note="one row below linear_takes_planes / pipe_ln_applies / qkv_attn_applies (M >= 192)")
add("T192_all_fused", "bert", 128, L, 2, 512, 8, 32, LEN192, "peaked", "attn_fused", path="packed", ln_launches=4, attn_launches=2,
    note="exactly at the row count: planes, both fusions; 1.5 LayerNorm panels (ragged last panel), one column tile per panel")
add("T192_f32_arith", "bert", 128, L, 2, 512, 8, 32, LEN192, "peaked", "no_planes_f32", path="packed", arith="f32",
    note='arith="f32": arith_split() is false, no planes whatever T')
add("T192_ln_off", "bert", 128, L, 2, 512, 8, 32, LEN192, "peaked", "attn_fused", path="packed", ln_fusion=0, attn_launches=2,
    note="LayerNorm fusion off: separate LayerNorm launches on planes; (the in-launch exchange is off with it)")
add("T192_attn_off", "bert", 128, L, 2, 512, 8, 32, LEN192, "peaked", "ln_fused", path="packed", env=FUSION_OFF, ln_launches=4,
    note="attention fusion off: stand-alone attention on planes, longest 32 (one key tile)")
add("T192_both_off", "bert", 128, L, 2, 512, 8, 32, LEN192, "peaked", "planes_unfused", path="packed", env=FUSION_OFF, ln_fusion=0)
add("T150_of_100x2", "bert", 768, L, 12, 3072, 100, 2, cyc((1, 2), 100), "flat", "small_layered", path="packed", sens=False,
    note="100 sequences of <= 2 tokens: 150 rows, no planes, while b * S = 200 would take them (the embedding waits for the count); "
         "T < 4 b: the last layer computes Q for every row")
add("T200_of_100x2", "bert", 768, L, 12, 3072, 100, 2, None, "flat", "attn_fused", mask="ones", path="padded", ln_launches=4,
    attn_launches=2, sens=False, note="every row full: [b, S] forward without a mask, 200 rows on planes, T < 4 b")
# ---- LayerNorm fusion: H 128 (one column tile per panel, above), 768 (6), 1024 (8); outlier channels --------------------------
add("ln_768_T384", "bert", 768, L, 12, 3072, 24, 16, None, "peaked_wide", "attn_fused", mask="none", ln_launches=4, attn_launches=2,
    sens=False, note="exactly 3 panels x 6 column tiles, unpacked without a mask")
add("ln_768_T384_off", "bert", 768, L, 12, 3072, 24, 16, None, "peaked_wide", "planes_unfused", mask="none", ln_fusion=0, env=FUSION_OFF,
    sens=False)
add("ln_768_T384_attn_off", "bert", 768, L, 12, 3072, 24, 16, None, "peaked_wide", "ln_fused", mask="none", env=FUSION_OFF, ln_launches=4,
    sens=False)
add("ln_1024_ragged_panel", "bert", 1024, L, 16, 4096, 10, 24, (24, 20, 24, 13, 24, 24, 17, 24, 24, 9), "peaked_wide", "attn_fused",
    path="packed", ln_launches=4, attn_launches=2, sens=False, note="203 rows: 8 column tiles per panel, ragged last panel; K = 4096")
add("ln_1024_off", "bert", 1024, L, 16, 4096, 10, 24, (24, 20, 24, 13, 24, 24, 17, 24, 24, 9), "peaked_wide", "attn_fused", path="packed",
    ln_fusion=0, attn_launches=2, sens=False)
add("ln_768_flat_f32", "bert", 768, L, 12, 3072, 24, 16, None, "flat", "no_planes_f32", mask="none", arith="f32", sens=False)
# ---- attention fusion: longest 64 / 65, packed / unpacked, the 256-row tile boundary, the exchange, many short sequences -----
LEN64 = (64, 50, 33, 20, 17, 8)                                  # 192 rows
LEN65 = (65, 50, 33, 20, 17, 8)                                  # 193 rows
add("attn_longest64", "bert", 128, L, 2, 512, 6, 64, LEN64, "peaked", "attn_fused", path="packed", ln_launches=4, attn_launches=2,
    note="longest = 64: the last length the fused epilogue takes (two query tiles)")
add("attn_longest65", "bert", 128, L, 2, 512, 6, 65, LEN65, "peaked", "attn_standalone", path="packed", ln_launches=4,
    note="longest = 65: stand-alone attention, three key tiles; the CLS attention on 64-key tiles")
STRADDLE = (40, 40, 40, 40, 40, 40, 30, 20, 40, 33, 7, 40)       # rows 240 .. 269 straddle the boundary at 256
EXACT = (40, 40, 40, 40, 40, 30, 26, 20, 40, 33, 7, 40)          # a sequence ends on row 255, the next starts the second tile
add("attn_straddle_exchange", "bert", 128, L, 2, 512, 12, 40, STRADDLE, "peaked", "attn_fused", path="packed", ln_launches=4,
    attn_launches=2, note="a sequence straddles the 256-row tile boundary: finished by the in-launch exchange")
add("attn_straddle_boundary", "bert", 128, L, 2, 512, 12, 40, STRADDLE, "peaked", "attn_fused_boundary", path="packed",
    env=XCHG_OFF, ln_launches=4, attn_launches=2, note="AC_QKV_ATTN_EXCHANGE=0: finished by the boundary launch")
add("attn_ends_on_boundary", "bert", 128, L, 2, 512, 12, 40, EXACT, "peaked", "attn_fused", path="packed", ln_launches=4,
    attn_launches=2, note="a sequence ends exactly on the boundary: nothing to exchange")
add("attn_ends_on_boundary_bl", "bert", 128, L, 2, 512, 12, 40, EXACT, "peaked", "attn_fused_boundary", path="packed", env=XCHG_OFF,
    ln_launches=4, attn_launches=2)
add("attn_many_short", "bert", 128, L, 2, 512, 60, 8, cyc((2, 8, 3, 7, 4, 6, 5), 60), "peaked", "attn_fused", path="packed",
    ln_launches=4, attn_launches=2, note="sequences of 2 .. 8 tokens, ~50 per tile, one straddler")
add("attn_768_unpacked_straddle", "bert", 768, L, 12, 3072, 6, 50, None, "peaked_wide", "attn_fused", mask="ones", path="padded",
    ln_launches=4, attn_launches=2, sens=False, note="50-token rows unpacked: 300 rows, the sixth sequence straddles")
# ---- stand-alone attention: key-tile edges 32 / 33 / 64 / 65 / 129, head dims 64 and 32, the padded path with a mask ----------
add("sa_longest32", "bert", 128, L, 2, 512, 8, 32, LEN192, "flat", "attn_standalone", path="packed", env=FUSION_OFF, ln_launches=4)
add("sa_longest33", "bert", 128, L, 2, 512, 7, 33, (33, 31, 30, 25, 32, 21, 20), "peaked", "attn_standalone", path="packed",
    env=FUSION_OFF, ln_launches=4, note="one key past a tile; CLS attention on 64-key tiles")
add("sa_longest64", "bert", 128, L, 2, 512, 6, 64, LEN64, "peaked", "attn_standalone", path="packed", env=FUSION_OFF, ln_launches=4)
add("sa_longest129", "bert", 128, L, 2, 512, 3, 129, (129, 40, 66), "peaked", "attn_standalone", path="packed", ln_launches=4,
    note="five key tiles, the last holding one key")
add("sa_dh32_longest33", "bert", 384, L, 12, 1536, 7, 33, (33, 31, 30, 25, 32, 21, 20), "peaked", "attn_standalone", path="packed",
    ln_launches=4, note="head dim 32 never fuses its attention")
add("sa_dh32_longest129", "bert", 384, L, 12, 1536, 3, 129, (129, 40, 66), "peaked", "attn_standalone", path="packed",
    ln_launches=4, sens=False)
add("sa_dh32_longest64_small", "bert", 384, L, 12, 1536, 3, 64, (64, 32, 17), "peaked", "small_layered", path="packed", sens=False,
    note="113 rows: head dim 32 on fp32 activations")
HOLES = ((1, 3), (2, 0 + 5), (2, 6), (4, 1))
add("pm_left_padded", "bert", 128, L, 2, 512, 6, 24, (24, 11, 17, 5, 24, 9), "peaked", "padded_mask", mask="left", path="padded_mask",
    note="left padding (144 rows, fp32 activations): position 0 of the short rows is a padding QUERY over the real keys")
add("pm_holes", "bert", 128, L, 2, 512, 6, 24, (24, 11, 17, 5, 24, 9), "peaked", "padded_mask", mask="holes", holes=HOLES,
    path="padded_mask")
add("pm_empty_row", "bert", 128, L, 2, 512, 6, 24, (24, 11, 0, 5, 24, 9), "peaked", "padded_mask", mask="holes", path="padded_mask",
    note="row 2 is all-masked: legal input, its own output row is not compared")
add("pm_holes_planes", "bert", 128, L, 2, 512, 9, 24, (24, 11, 17, 5, 24, 9, 24, 20, 13), "peaked", "padded_mask_planes", mask="holes",
    holes=HOLES, path="padded_mask", ln_launches=4, note="216 rows on planes; a mask keeps the stand-alone attention")
add("pm_empty_row_planes", "bert", 128, L, 2, 512, 9, 24, (24, 11, 0, 5, 24, 9, 24, 20, 13), "peaked", "padded_mask_planes",
    mask="holes", path="padded_mask", ln_launches=4)
add("ones_explicit", "bert", 128, L, 2, 512, 9, 24, None, "peaked", "attn_fused", mask="ones", path="padded", ln_launches=4,
    attn_launches=2, note="a mask of all ones passed explicitly: the [b, S] forward without a mask")
add("ones_explicit_unpad_off", "bert", 128, L, 2, 512, 9, 24, None, "peaked", "padded_mask_planes", mask="ones", unpad=False,
    ln_launches=4, note="unpad=False: the all-ones mask reaches the kernels as a mask (no attention fusion)")
# ---- last layer ---------------------------------------------------------------------------------------------------------
add("last_T_lt_4b", "bert", 128, L, 2, 512, 100, 3, cyc((3, 2, 3, 1, 3), 100), "peaked", "attn_fused", path="packed", ln_launches=4,
    attn_launches=2, note="240 rows < 4 b: no CLS-only Q; sequences of 1 .. 3 tokens")
add("last_tail_unfused", "bert", 128, L, 2, 512, 8, 32, LEN192, "peaked", "attn_fused", path="packed", env=TAIL_OFF, ln_launches=4,
    attn_launches=2, note="AC_BERT_TAIL_FUSED=0: reduce -> LayerNorm -> normalize")
add("last_tail_unfused_768", "bert", 768, L, 12, 3072, 24, 16, None, "peaked_wide", "attn_fused", mask="none", env=TAIL_OFF, ln_launches=4,
    attn_launches=2, sens=False)
add("last_tail_unfused_dh32", "bert", 384, L, 12, 1536, 7, 33, (33, 31, 30, 25, 32, 21, 20), "peaked", "attn_standalone", path="packed",
    env=TAIL_OFF, ln_launches=4)
add("last_ldo_wide", "bert", 128, L, 2, 512, 8, 32, LEN192, "peaked", "attn_fused", path="packed", ldo_extra=24, ln_launches=4,
    attn_launches=2, note="ldo = H + 24: the padding columns are zeroed")
add("last_ldo_wide_unfused_tail", "bert", 128, L, 2, 512, 8, 32, LEN192, "peaked", "attn_fused", path="packed", ldo_extra=24,
    env=TAIL_OFF, ln_launches=4, attn_launches=2)
add("last_padded_cls_stride", "bert", 128, L, 2, 512, 9, 24, None, "peaked", "planes_unfused", mask="none", env=FUSION_OFF, ln_fusion=0,
    note="padded layout: CLS rows S * H apart (the packed cases gather them)")
add("last_b200", "bert", 128, L, 2, 512, 200, 8, cyc((8, 5, 7, 8, 4), 200), "peaked", "attn_fused", path="packed", ln_launches=4,
    attn_launches=2, note="b >= 192: the CLS rows themselves reach the row count of the planes kernels")
# ---- ModernBERT (local 16: the window |q - k| <= 8 covers a whole sequence up to S = 17 from its middle; 2 * 8 + 1 = 17) ----
MB = dict(local=16, global_every=3)
add("mb_S16_small", "modernbert", 128, L, 2, 192, 3, 16, (16, 9, 12), "scaled", "mb_no_planes", **MB,
    note="S below 2 * (local / 2) + 1; the small-M path; packed")
add("mb_S17", "modernbert", 128, L, 2, 192, 3, 17, (17, 10, 17), "scaled", "mb_no_planes", **MB)
add("mb_S18", "modernbert", 128, L, 2, 192, 3, 18, (18, 10, 18), "scaled", "mb_no_planes", **MB)
add("mb_S40_planes_packed", "modernbert", 128, L, 2, 192, 7, 40, (40, 33, 21, 40, 12, 37, 26), "scaled", "mb_planes", **MB,
    tokens=209, note="209 rows on planes; windows cut inside the ragged sequences")
add("mb_S40_planes_padded", "modernbert", 128, L, 2, 192, 7, 40, (40, 33, 21, 40, 12, 37, 26), "scaled", "mb_planes", unpad=False,
    **MB, note="the same batch padded: [b, S] rows with the mask")
add("mb_S40_f32", "modernbert", 128, L, 2, 192, 7, 40, (40, 33, 21, 40, 12, 37, 26), "scaled", "mb_no_planes", arith="f32", **MB)
add("mb_ge2", "modernbert", 128, L, 2, 192, 7, 40, (40, 33, 21, 40, 12, 37, 26), "scaled", "mb_planes", local=16, global_every=2,
    tokens=209, note="global_every 2: the CLS-only last layer is a global one")
add("mb_L4_ge3", "modernbert", 128, 4, 2, 192, 7, 40, (40, 33, 21, 40, 12, 37, 26), "scaled", "mb_planes", **MB,
    note="four layers: the CLS-only last layer is global again (index 3)")
MB_HOLES = tuple((1, c) for c in (6, 7, 8, 9, 11, 12, 13, 14)) + ((2, 3),)
add("mb_lonely_query", "modernbert", 128, L, 2, 192, 3, 24, (24, 24, 15), "scaled", "mb_no_planes", mask="holes", holes=MB_HOLES,
    local=8, global_every=3, note="local 8: the window of row 1's query 10 holds only itself and masked keys")
add("mb_b200", "modernbert", 128, L, 2, 192, 200, 6, cyc((6, 3, 5, 2, 6), 200), "scaled", "mb_planes", local=4, global_every=3,
    note="b >= 192: the CLS-only last layer on planes")
add("mb_S1024", "modernbert", 128, L, 2, 192, 1, 1024, None, "scaled", "mb_planes", mask="none", local=128, global_every=3, sens=False,
    note="32 key tiles, +-64 windows skip most of them in the local layers")
# ---- DistilBERT, RoBERTa, XLM-R, ELECTRA: weight mappings -----------------------------------------------------------------
FAM_LEN = (24, 11, 17, 5, 24, 9, 24, 20, 13, 24, 16, 22)          # 209 rows
for fam, regime in (("distilbert", "peaked"), ("roberta", "flat"), ("xlm-roberta", "flat"), ("electra", "peaked")):
    add(f"{fam}_packed", fam, 128, L, 2, 512, 12, 24, FAM_LEN, regime, "attn_fused", path="packed", ln_launches=4, attn_launches=2)
    add(f"{fam}_one_launch", fam, 128, L, 2, 512, 2, 12, (12, 7), regime, "one_launch", one_launch=True)
# ---- chunking ----------------------------------------------------------------------------------------------------------
add("chunks_fused_then_not", "bert", 128, L, 2, 512, 24, 16, None, "peaked", "attn_fused", mask="none", max_tokens=14 * 16,
    ln_launches=4, attn_launches=2, note="MAX_TOKENS = 224: 14 sequences (224 rows, fused) then 10 (160 rows, fp32 activations)")

BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)
BRANCHES = sorted({c.branch for c in CASES})


# ------------------------------------------------------------------------------------------------------------------------
# evaluation (cached per input: many cases share a model and a batch and differ only in how the device is called)
# ------------------------------------------------------------------------------------------------------------------------
def _run(m, bs, **kw):
    model = make_model(m)
    ids, types, mask = make_batch(bs)
    return FORWARD[m.family](model.state_dict(), model.config, ids, types, mask, **kw)


@functools.lru_cache(maxsize=None)
def _reference(m, bs):
    return _run(m, bs)


def reference(case):
    """fp64 unit-norm CLS vectors [b, H] of the case (computed once per input, shared; do not modify)"""
    return _reference(case.model, case.batch)


def fp32_instance(case, chunked=False):
    return _run(case.model, case.batch, dtype=torch.float32, mm=mm_chunk16 if chunked else mm_plain)


@torch.no_grad()
def transformers_fp32(case):
    model = make_model(case.model)
    ids, types, mask = make_batch(case.batch)
    kw = dict(input_ids=ids)
    if mask is not None:
        kw["attention_mask"] = mask
    if types is not None:
        kw["token_type_ids"] = types
    return F.normalize(model(**kw).last_hidden_state[:, 0, :], p=2, dim=1)


def applicable(name, case):
    """can this mistake change anything on this case's input?"""
    fams, _ = MUTANTS[name]
    m, bs = case.model, case.batch
    if m.family not in fams:
        return False
    ids, types, mask = make_batch(bs)
    if name == "admit_first_pad":
        return mask is not None and bool((mask == 0).any())
    if name == "drop_last_key":
        return bs.S > 1
    if name == "no_types":
        return bs.S > 1
    if name in ("window_plus", "window_minus", "rope_theta_global"):
        longest = bs.S if mask is None else int(mask.sum(1).max())
        return any(t == "sliding_attention" for t in make_model(m).config.layer_types) and \
            (name == "rope_theta_global" or longest > m.local // 2 + 1)
    return True


@functools.lru_cache(maxsize=None)
def _mutant(m, bs, name):
    rows = compared_rows(bs)
    return float((_run(m, bs, mut=(name,)) - _reference(m, bs))[rows].abs().max())


def mutant_distance(case, name):
    """max-abs distance of the mutant's unit CLS vectors from the reference over the compared rows"""
    return _mutant(case.model, case.batch, name)


def deviation(case, got):
    """max-abs difference of `got` [b, H] (any dtype / device) from the fp64 reference over the compared rows"""
    rows = compared_rows(case.batch)
    return float((got.detach().double().cpu() - reference(case))[rows].abs().max())


@torch.no_grad()
def peak_stats(case):
    """mean over layers of the mean (over heads and valid queries) max attention probability of the fp64 reference"""
    probs = []
    _run(case.model, case.batch, probs_out=probs)
    _, _, mask = make_batch(case.batch)
    valid = torch.ones(case.batch.b, case.batch.S, dtype=torch.bool) if mask is None else mask.bool()
    per_layer = [float(p.max(-1).values.transpose(0, 1)[:, valid].mean()) for p in probs]
    return sum(per_layer) / len(per_layer)


# ------------------------------------------------------------------------------------------------------------------------
# bounds
# ------------------------------------------------------------------------------------------------------------------------
# FP32_DEV[(family, regime)]: worst max-abs deviation from fp64, over the group's cases and over the three fp32 instances
# (this file's forward in fp32, the same with K-chunks of 16, transformers fp32 eager), measured on the CPU and rounded up to
# one digit.  tests/test_encoder_ref_cpu.py asserts every case stays within ADMISSION x its group's figure and prints this
# table; the worst cases at the time of writing (8 CPU threads):
#
#   group                      torch fp32                     K-chunks of 16                 transformers fp32              FP32_DEV  16 x
#   bert        flat           7.4e-08 ol_128_flat            7.3e-08 ol_128_flat            8.0e-08 ol_128_flat            9e-8      1.4e-6
#   bert        peaked         2.2e-07 sa_dh32_longest129     1.2e-07 last_T_lt_4b           1.6e-07 sa_dh32_longest64_sm.  3e-7      4.8e-6
#   bert        peaked_wide    2.0e-07 ln_768_T384            1.8e-07 ln_1024_ragged_panel   2.4e-07 ln_1024_ragged_panel   3e-7      4.8e-6
#   distilbert  peaked         1.3e-07 distilbert_packed      8.3e-08 distilbert_packed      1.3e-07 distilbert_packed      2e-7      3.2e-6
#   electra     peaked         1.2e-07 electra_packed         1.0e-07 electra_packed         1.4e-07 electra_packed         2e-7      3.2e-6
#   modernbert  scaled         9.2e-08 mb_b200                8.6e-08 mb_b200                9.7e-08 mb_b200                1e-7      1.6e-6
#   roberta     flat           7.6e-08 roberta_packed         7.5e-08 roberta_packed         6.7e-08 roberta_packed         8e-8      1.3e-6
#   xlm-roberta flat           7.6e-08 xlm-roberta_packed     7.5e-08 xlm-roberta_packed     6.7e-08 xlm-roberta_packed     8e-8      1.3e-6
FP32_DEV = {
    ("bert", "flat"): 9e-8,
    ("bert", "peaked"): 3e-7,
    ("bert", "peaked_wide"): 3e-7,
    ("distilbert", "peaked"): 2e-7,
    ("electra", "peaked"): 2e-7,
    ("roberta", "flat"): 8e-8,
    ("xlm-roberta", "flat"): 8e-8,
    ("modernbert", "scaled"): 1e-7,
}
ADMISSION = 4
# The device gets KERNEL_FACTOR = 16 over the fp32 figure, by the argument of tests/head_epoch_ref.py: its dot products are serial
# fma chains per lane and wave-strided sums (error growing with K, here up to 4096 in FFN-down) against torch's blocked sums, and
# the bf16x3 GEMMs are allowed 3 x the fp32 error of a product by test_split_gemm_is_fp32_grade.
KERNEL_FACTOR = 16
DEVICE_BOUND_CEILING = 1e-5
PATH_FACTOR = {}                  # branch -> its own factor, with the reason (none needed so far)


def device_bound(case):
    bound = PATH_FACTOR.get(case.branch, KERNEL_FACTOR) * FP32_DEV[case.group]
    assert bound <= DEVICE_BOUND_CEILING, (case.id, bound)
    return bound
