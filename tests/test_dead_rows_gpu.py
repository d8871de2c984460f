"""Work the result does not need is left out of the matrix-pipe kernels, and no stored bit changes.

gemm_pipe_nt: a wave whose rows all lie at or past M keeps its DMA share, its counted waits and every barrier, but reads no
fragments and issues no MFMAs.  acattn::attention_tile: a PV step whose two keys are past the end of the sequence, masked out or
outside the sliding window of every query of the tile is skipped together with its V loads, and no K fragment is fetched for a
tile past the last.  Both removals take away exact zeros (or values no store reads), so every case here is checked for EQUALITY:
against the route that does not use the changed code where there is one, and against the sha256 the PARENT commit's library
produced on MI355X (tests/data/dead_rows_parent.json, recorded by tools/dead_rows_probe.py)."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import dead_rows_cases as D

pytestmark = pytest.mark.gpu

FIXTURE = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "dead_rows_parent.json")))
PARENT = FIXTURE["cases"]


def recorded(cid):
    """the parent's record of a case; the hashes hold on the CU count they were recorded on (the GEMM plan depends on it)"""
    from adaptive_classifier import _native as nv
    cus = nv.device_info()["cus"]
    if cus != FIXTURE["cus"]:
        pytest.skip("fixture recorded on %d CUs, this device has %d: the dispatch depends on the count" % (FIXTURE["cus"], cus))
    return PARENT[cid]


@functools.lru_cache(maxsize=None)
def _reference(arith, M, N, K):
    """bf16x3: the two-buffer kernels (ac_gemm_set_variant(1)), which share no loop with the ring kernels.  fp16x2 has ring
    kernels only: the default dispatch's choice stands in (the same products in the same k order whatever the tile)."""
    from adaptive_classifier import _native as nv
    rc, got, canary = D.run_ring(nv, torch.device("cuda:0"), dict(arith=arith, M=M, N=N, K=K), 1 if arith == D.BF16X3 else 0)
    return rc, got, canary


@pytest.mark.parametrize("cfg", D.PIPE_CFGS)
@pytest.mark.parametrize("arith", [D.BF16X3, D.F16X2], ids=["bf16x3", "f16x2"])
def test_ring_kernels_at_ragged_m(arith, cfg, cuda_dev):
    """M = BM + 1, BM + 31, BM + 33, 2 BM - 1 and 193 rows (one live row, one live 32-row block, a block and a row, all but one
    row; 193 = the fewest rows past which every configuration is on its ring kernel), N = one and two column tiles, K = 4 and 12
    stages (shorter and longer than the deepest ring): dead waves in every position the 2 x 2, 4 x 2 and 2 x 4 wave grids have.
    Behind row M lie 64 canary rows of a NaN pattern that must come back untouched.  Shapes under 192 rows go where the planner
    sends them (not a ring kernel; fp16x2 refuses them) and must simply do what the parent did."""
    from adaptive_classifier import _native as nv
    ran = 0
    for c in [c for c in D.ring_cases() if c["arith"] == arith and c["cfg"] == cfg]:
        want = recorded(c["id"])
        for rep in range(2):                                        # (twice: a race would not repeat itself)
            rc, got, canary = D.run_ring(nv, cuda_dev, c, cfg)
            assert rc == want["rc"], (c["id"], rc, nv.lib().ac_last_error())
            if rc != 0:
                continue
            assert canary, (c["id"], "rows past M were written")
            assert np.isfinite(got.view(np.float32)).all(), c["id"]
            assert D.sha(got) == want["sha256"], (c["id"], "differs from the parent's output")
            rrc, ref, rcanary = _reference(arith, c["M"], c["N"], c["K"])
            assert rrc == 0 and rcanary and np.array_equal(got, ref), (c["id"], int((got != ref).sum()))
            ran += 1
    assert ran >= 2 * 8


@pytest.mark.parametrize("case", D.LN_CASES, ids=[c["id"] for c in D.LN_CASES])
def test_fused_layernorm_at_ragged_m(case, cuda_dev):
    """EPI_BIAS_RES_LN with a last row panel of 21 rows / 1 row: the dead waves' zero accumulators still go through the partial
    exchange (finite: bias + the clamped row's residual) and the live rows' statistics do not see them.  149 rows stay under
    the tiled kernels' 192-row floor (no fused launch, as in the parent); 385 rows fuse both LayerNorms of layer 0."""
    from adaptive_classifier import _native as nv
    want = recorded(case["id"])
    fused, launches = D.run_ln(nv, case)
    again, _ = D.run_ln(nv, case)
    separate, none = D.run_ln(nv, case, fused=False)
    assert launches == want["fused_launches"] == (2 if case["M"] >= 192 else 0) and none == 0
    assert torch.isfinite(fused).all()
    assert torch.equal(fused, again)
    assert (fused - separate).abs().max().item() < 5e-6
    assert D.sha(fused.numpy()) == want["sha256"]


@pytest.mark.parametrize("case", D.ATTN_FUSED_CASES, ids=[c["id"] for c in D.ATTN_FUSED_CASES])
def test_fused_attention_with_a_nearly_dead_last_tile(case, cuda_dev):
    """256 + 5 packed rows: six of the eight waves of the last QKV row tile are dead, and they still take part in every staging
    pass and barrier of the attention epilogue; the last tile's only sequence, or the tail of one that straddles into it (finished
    through the in-launch exchange, or by the boundary launch), is served from rows the two live waves wrote."""
    from adaptive_classifier import _native as nv
    lib = nv.lib()
    n0 = lib.ac_gemm_qkv_attn_launches()
    fused = D.run_attn_fused(case)
    assert lib.ac_gemm_qkv_attn_launches() == n0 + 1                 # layer 0; the last layer is the CLS-only one
    separate = D.run_attn_fused(case, fusion=False)
    assert lib.ac_gemm_qkv_attn_launches() == n0 + 1
    assert torch.isfinite(fused).all()
    assert torch.equal(fused, separate), (fused - separate).abs().max().item()
    assert D.sha(fused.numpy()) == recorded(case["id"])["sha256"]


@pytest.mark.parametrize("case", D.ATTN_TILE_CASES, ids=[c["id"] for c in D.ATTN_TILE_CASES])
def test_attention_tile_skips_only_exact_zeros(case, cuda_dev):
    """attention_mfma_kernel over sequences of S tokens: S around every 4-key group edge of the PV steps (keys r, r + 4 of each
    8), one key, one tile, two tiles; with a full mask, with holes (a whole 4-key group gone: steps that die in the middle of a
    live tile) and on a ModernBERT sliding-window layer (|q - k| <= 8: keys no query of the tile can see).  Equal to the parent
    bit for bit, and to the transformers model within the suite's 1e-4 bar."""
    got, want = D.run_tile(case)
    assert torch.isfinite(got).all()
    assert (got - want).abs().max().item() < 1e-4
    assert D.sha(got.numpy()) == recorded(case["id"])["sha256"]
