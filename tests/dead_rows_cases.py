"""The fixed cases of the dead-rows fixture (tests/data/dead_rows_parent.json) and the code that runs one of them.

Shared by tools/dead_rows_probe.py (records, with the PARENT commit's library, the sha256 of what every case writes) and
tests/test_dead_rows_gpu.py (runs the cases in this process and compares).  The cases sit where a wave or a PV step of the
matrix-pipe kernels has nothing to do -- token rows past the end of the last row tile (gemm_pipe.hip), keys past the end of a
sequence, masked out, or outside a sliding window (attention_core.h) -- so that leaving that work out must not change one bit.

GEMM inputs are closed-form integer arithmetic (gemm_dispatch_cases._mat); the encoder cases use the seeded models and token
ids of oracle/bert_oracle.py."""
import functools
import hashlib
import os

import numpy as np

import gemm_dispatch_cases as G

BF16X3, F16X2 = 1, 2
# every ring configuration gemm_pipe.hip builds (AC_PIPE_CONFIGS; tests/test_gemm_split_gpu.py PIPE_CFGS): tm tn wmw wnw ring pipe
PIPE_CFGS = [222232, 124261, 124262, 224242, 234232, 322432, 244232]
CANARY_ROWS = 64
CANARY_BITS = 0x7FC0DEAD            # a quiet NaN with a payload no kernel produces


def cfg_tile(cfg):
    tm, tn, wmw, wnw = (cfg // 100000) % 10, (cfg // 10000) % 10, (cfg // 1000) % 10, (cfg // 100) % 10
    return 32 * tm * wmw, 32 * tn * wnw


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


# ---- ring kernels at ragged M ----
def ring_cases():
    out = []
    for arith in (BF16X3, F16X2):
        for cfg in PIPE_CFGS:
            BM, BN = cfg_tile(cfg)
            for M in (BM + 1, BM + 31, BM + 33, 2 * BM - 1, 193):
                for N in (BN, 2 * BN):
                    for K in (64, 192):
                        out.append(dict(id="ring_%s_%d_%dx%dx%d" % ("bf16x3" if arith == BF16X3 else "f16x2", cfg, M, N, K),
                                        arith=arith, cfg=cfg, M=M, N=N, K=K))
    return out


@functools.lru_cache(maxsize=None)
def _ring_inputs(M, N, K):
    A, W, bias, R = G.inputs(dict(M=M, N=N, K=K, res=True, entry="linear"))
    return A, W, bias, R


def run_ring(nv, dev, c, variant):
    """One launch of case c under ac_gemm_set_variant(variant) (a ring cfg, or 1 = the two-buffer kernels), bias + residual, into
    rows [0, M) of an (M + CANARY_ROWS)-row buffer.  Returns (rc, the M x N result or None, canary rows untouched)."""
    import torch
    lib, st = nv.lib(), nv.stream_ptr(dev)
    M, N, K = c["M"], c["N"], c["K"]
    A, W, bias, R = _ring_inputs(M, N, K)
    f16 = c["arith"] == F16X2
    before = lib.ac_gemm_get_arith()
    nv.check(lib.ac_gemm_set_arith(c["arith"]), "ac_gemm_set_arith")
    nv.check(lib.ac_gemm_set_variant(variant), "ac_gemm_set_variant")
    lib.ac_gemm_set_krot(0)
    try:
        Ad, Wd, bd, Rd = (torch.from_numpy(x).to(dev) for x in (A, W, bias, R))
        buf = torch.full(((M + CANARY_ROWS) * N,), CANARY_BITS, dtype=torch.int32, device=dev)
        per = 2 if f16 else 3
        Ap = torch.zeros(per * M * K, dtype=torch.int16, device=dev)
        Wp = torch.zeros(per * N * K, dtype=torch.int16, device=dev)
        if f16:
            nv.check(lib.ac_split_f16x2(nv.ptr(Ad), K, M, K, 6, nv.ptr(Ap), st), "ac_split_f16x2")
            nv.check(lib.ac_split_f16x2(nv.ptr(Wd), K, N, K, 10, nv.ptr(Wp), st), "ac_split_f16x2")
            rc = lib.ac_linear_f16x2(nv.ptr(Ap), nv.ptr(Wp), nv.ptr(bd), nv.ptr(Rd), N, nv.ptr(buf), N, None, M, N, K, 0, st)
        else:
            nv.check(lib.ac_split_bf16x3(nv.ptr(Ad), K, M, K, nv.ptr(Ap), st), "ac_split_bf16x3")
            nv.check(lib.ac_split_bf16x3(nv.ptr(Wd), K, N, K, nv.ptr(Wp), st), "ac_split_bf16x3")
            rc = lib.ac_linear_bf16x3(nv.ptr(Ad), K, nv.ptr(Ap), nv.ptr(Wd), K, nv.ptr(Wp), nv.ptr(bd), nv.ptr(Rd), N,
                                      nv.ptr(buf), N, None, M, N, K, 0, st)
        torch.cuda.synchronize(dev)
        if rc != 0:
            return rc, None, True
        host = buf.cpu().numpy()
        return rc, host[:M * N].reshape(M, N).copy(), bool((host[M * N:] == CANARY_BITS).all())
    finally:
        lib.ac_gemm_set_arith(before)
        lib.ac_gemm_set_variant(0)


# ---- encoder cases: batches with chosen sequence lengths ----
def batch_of_lengths(lens, S, vocab=2000, seed=5, first=101):
    import torch
    g = torch.Generator().manual_seed(seed)
    b = len(lens)
    ids = torch.randint(1000, vocab, (b, S), generator=g)
    ids[:, 0] = first
    mask = torch.zeros((b, S), dtype=torch.int64)
    for i, n in enumerate(lens):
        mask[i, :n] = 1
    ids = ids * mask
    return ids, torch.zeros((b, S), dtype=torch.int64), mask


@functools.lru_cache(maxsize=None)
def bert_model(hidden, layers, heads, inter, seed=5):
    from oracle import bert_oracle
    return bert_oracle.make_bert(hidden, layers, heads, inter, vocab=2000, seed=seed)


@functools.lru_cache(maxsize=None)
def modernbert_model():
    from oracle import bert_oracle
    # 3 layers, global every 3rd: layer 1 is a sliding-window layer (|q - k| <= 8) that runs on every token row (the last layer
    # only serves the CLS query)
    return bert_oracle.make_modernbert(128, 3, 2, 256, vocab=2000, max_pos=1024, local_attention=16, seed=3, init_scale=4.0)


@functools.lru_cache(maxsize=None)
def encoder(kind, *key):
    import torch
    from adaptive_classifier.encoder import HipBertEncoder, HipModernBertEncoder
    dev = torch.device("cuda:0")
    if kind == "modernbert":
        return HipModernBertEncoder(modernbert_model(), device=dev)
    return HipBertEncoder(bert_model(*key), device=dev)


class env:
    """os.environ settings for the duration of a block (the library reads these switches at every call)"""

    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kw}
        for k, v in self.kw.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


# fused LayerNorm at ragged M: (token rows M, width N); 16-token sequences and one short one
LN_CASES = [dict(id="ln_%dx%d" % (M, N), M=M, N=N) for M in (128 + 21, 3 * 128 + 1) for N in (256, 768)]


def ln_batch(c):
    M = c["M"]
    lens = [16] * (M // 16) + ([M % 16] if M % 16 else [])
    return batch_of_lengths(lens, 16, seed=c["N"] + M)


def ln_encoder(c):
    N = c["N"]
    return encoder("bert", N, 2, N // 64, 2 * N)


# fused attention on a 2-layer, 128-wide model: 256 + 5 packed rows
ATTN_FUSED_CASES = [
    dict(id="attn_last_tile_one_5_token_sequence", lens=[32] * 8 + [5], exchange=None),
    dict(id="attn_straddler_into_last_tile_exchange", lens=[32] * 7 + [30, 7], exchange=None),
    dict(id="attn_straddler_into_last_tile_boundary", lens=[32] * 7 + [30, 7], exchange="0"),
]

# attention_tile through attention_mfma_kernel: every sequence of the batch has S tokens
ATTN_S = [1, 3, 4, 5, 8, 9, 12, 13, 16, 31, 32, 33, 40, 64]
ATTN_TILE_CASES = [dict(id="tile_%s_S%d" % (kind, S), kind=kind, S=S) for S in ATTN_S for kind in ("plain", "holes", "window")]
ATTN_ROWS = 40


def tile_batch(c):
    """plain / window: all-ones mask.  holes: the key mask has holes -- keys 4 .. 7 (one whole 4-key group of the PV steps) where
    the sequence has them, and a scatter that differs from row to row; key 0 stays."""
    S = c["S"]
    ids, types, mask = batch_of_lengths([S] * ATTN_ROWS, S, seed=100 + S, first=1 if c["kind"] == "window" else 101)
    if c["kind"] == "holes":
        for i in range(ATTN_ROWS):
            for k in range(1, S):
                if (S >= 8 and 4 <= k <= 7) or (7 * k + 3 * i) % 5 == 0:
                    mask[i, k] = 0
    return ids, types, mask


def run_tile(c):
    """(CLS vectors on the host, what the oracle says) with the attention as its own launch (attention_mfma_kernel)"""
    from oracle import bert_oracle
    ids, types, mask = tile_batch(c)
    with env(AC_QKV_ATTN_FUSION="0"):
        if c["kind"] == "window":
            got = encoder("modernbert").encode_cls(ids, None, mask).cpu()
            want = bert_oracle.encode_cls_modernbert(modernbert_model(), ids, mask)
        else:
            got = encoder("bert", 128, 2, 2, 512).encode_cls(ids, types, mask).cpu()
            want = bert_oracle.encode_cls(bert_model(128, 2, 2, 512), ids, types, mask)
    return got, want.detach()


def run_attn_fused(c, fusion=True):
    ids, types, mask = batch_of_lengths(c["lens"], 32, seed=len(c["lens"]))
    with env(AC_QKV_ATTN_FUSION=None if fusion else "0", AC_QKV_ATTN_EXCHANGE=c["exchange"]):
        return encoder("bert", 128, 2, 2, 512).encode_cls(ids, types, mask).cpu()


def run_ln(nv, c, fused=True):
    ids, types, mask = ln_batch(c)
    lib = nv.lib()
    n0 = lib.ac_gemm_ln_fusion_launches()
    try:
        nv.check(lib.ac_gemm_set_ln_fusion(1 if fused else 0), "ac_gemm_set_ln_fusion")
        enc = ln_encoder(c)
        got = enc.encode_cls(ids, types, mask).cpu()
        assert not enc.ln_fusion_aborted()
    finally:
        lib.ac_gemm_set_ln_fusion(1)
    return got, lib.ac_gemm_ln_fusion_launches() - n0
