"""GPU suite: every encoder family and route over a poisoned workspace, scratch and output (tests/poison.py).

Regions of the BERT-family workspace (csrc/bert.hip bert_ws / bert_encode_impl / ac_bert_encode_cls_unpad), read before any
poisoned run:

  [0, 256) verdict words          THE CALLER'S: include/acamd.h -- cleared once for a fresh workspace (encoder.py does it right
                                  after torch.empty), then rolled by ln_verdict_roll_kernel / the packing prologue at every call.
                                  This module never touches them itself: it drops the workspace and the encoder allocates and
                                  clears a new one, which is the product's own path.
  x, qkv, ctx, y, ffn and the operand planes xp, ctxp, ffnp
                                  written by the embedding kernel and by each GEMM / attention / LayerNorm for the T rows of the
                                  call before the next stage reads them; rows past T of the last tile are loaded but masked
  small                           the one-launch kernel's own rows and GridCtl (hipMemsetAsync, bert_small.hip)
  lnctl (panel counters)          hipMemsetAsync when the call fuses LayerNorms, unless the packing prologue already zeroed them
                                  (kPreCtl: pack_prologue_kernel zeroes lnctl and attn_xchg over the SAME layout, bert_ws(c, b, S))
  lnpart                          partial sums written by every tile of a panel before the panel's last tile reads them
  cu, tile_seq                    iota_cu_kernel / the prologue, then qkv_attn_tile_seq or the prologue's table: every tile of T
  attn_xchg                       hipMemsetAsync, or the prologue (kPreCtl); tags grow with the layer number
  pack_src, pack_info             the prologue: src for the real tokens, info whole
  ac_bert_pack's cu / src / info (torch.empty in encoder.py): info by hipMemsetAsync, cu whole, src for the real tokens
  DeBERTa scratch (_dis_scratch)  position_scores_kernel writes c2p | p2c for the T rows x heads x 2 Smax of every layer before
                                  the attention reads them
  ModernBERT workspace            activations and planes only, no control words
  output                          every row of [b, H] and the padding columns up to ldo (zeros)
Every wait of these kernels on another workgroup is bounded and ends in a give-up verdict, which the suites' runners assert absent.

Each case of encoder_ref.CASES, encoder_mpnet_ref.MPNET_CASES, encoder_deberta_ref.DEBERTA_CASES and encoder_pool_ref.POOL_CASES
is run by ITS OWN suite's test function (environment switches, forced layering, ln_fusion, arithmetic, output stride, branch
counters, fp64 bound -- all unchanged) in four states: zero, zero again, ff (fresh workspace / scratch / cu / src / info / output
byte-filled at allocation, a caller's output tensor filled before the call, padding columns included), leftover (the largest
case of the same encoder object first, then the case without reallocating).  (a) the returned rows are bit-identical;
(b) is the suite function's own assertion set, passed in every state.

fp16x2 (no table has it; the family's bar is SURVEY 8c's 1e-4 on the unit embedding, tests/test_gemm_f16x2_gpu.py -- here against
fp64, which sits ~1e-7 from the fp32 reference that bar names): one fused case (768 wide, 384 rows) and one one-launch case.
"""
import time

import pytest
import torch

import encoder_deberta_ref as DB
import encoder_mpnet_ref as MP
import encoder_pool_ref as PL
import encoder_ref as R
import poison
import test_encoder_deberta_gpu as t_db
import test_encoder_mpnet_gpu as t_mp
import test_encoder_pool_gpu as t_pl
import test_encoder_reference_gpu as t_ref

pytestmark = pytest.mark.gpu

_T0 = time.time()


@pytest.fixture(scope="module", autouse=True)
def _wall():
    yield
    for m in (t_ref, t_mp, t_db, t_pl):
        m._ENCODERS.clear()
    print(f"\nMEASURED test_poison_encoder_gpu wall time {time.time() - _T0:.1f} s")


class _Hook:
    """encode_cls of both encoder classes, wrapped: drops the kept buffers (reset), byte-fills a caller's output, records the rows"""

    def __init__(self, monkeypatch):
        from adaptive_classifier.encoder import HipBertEncoder, HipModernBertEncoder
        self.reset, self.byte, self.rows = False, None, []
        for cls in (HipBertEncoder, HipModernBertEncoder):
            real = cls.encode_cls
            monkeypatch.setattr(cls, "encode_cls", self._wrap(real))

    def _wrap(self, real):
        hook = self

        def encode_cls(enc, input_ids, token_type_ids=None, attention_mask=None, out=None, **kw):
            if hook.reset:
                enc._ws = None
                if getattr(enc, "_dis_scratch", None) is not None:
                    enc._dis_scratch = None
            if out is not None and hook.byte is not None:
                poison.fill(out, hook.byte)
            got = real(enc, input_ids, token_type_ids, attention_mask, out=out, **kw)
            hook.rows.append(got.detach().clone())
            return got
        return encode_cls


def _case_of(c):
    return getattr(c, "case", c)


def _largest(table, c):
    """the case of the same table on the same encoder object (model, unpad) with the most token rows"""
    key = (_case_of(c).model, _case_of(c).unpad)
    same = [o for o in table if (_case_of(o).model, _case_of(o).unpad) == key]
    return max(same, key=lambda o: _case_of(o).batch.b * _case_of(o).batch.S)


def _four_states(suite_fn, table, c, cuda_dev, monkeypatch):
    p = poison.poisoned_empty(monkeypatch, None)
    hook = _Hook(monkeypatch)
    res = {}

    def run(case):
        with pytest.MonkeyPatch.context() as mp:              # (the suite function's environment switches end with its run)
            suite_fn(case, cuda_dev, mp)

    for state, byte in (("zero", 0x00), ("zero2", 0x00), ("ff", 0xFF), ("leftover", None)):
        p.byte = hook.byte = byte
        if state == "leftover":
            hook.reset = True
            run(_largest(table, c))
            hook.reset = False
        else:
            hook.reset = True
        hook.rows = []
        run(c)
        res[state] = [r.cpu() for r in hook.rows]
        assert len(res[state]) >= 1
    p.byte = None
    assert p.filled > 0
    assert poison.same_bits(res["zero"], res["zero2"]), "two zero-state runs differ: " + poison.first_difference(res["zero"], res["zero2"])
    for state in ("ff", "leftover"):
        assert poison.same_bits(res["zero"], res[state]), f"the {state} state changed the result: " + poison.first_difference(res["zero"], res[state])


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.id)
def test_bert_families_and_modernbert(case, cuda_dev, monkeypatch):
    _four_states(t_ref.test_encoder_matches_fp64_on_its_branch, R.CASES, case, cuda_dev, monkeypatch)


@pytest.mark.parametrize("mc", MP.MPNET_CASES, ids=lambda c: c.id)
def test_mpnet(mc, cuda_dev, monkeypatch):
    _four_states(t_mp.test_mpnet_matches_fp64_on_its_route, MP.MPNET_CASES, mc, cuda_dev, monkeypatch)


@pytest.mark.parametrize("mc", DB.DEBERTA_CASES, ids=lambda c: c.id)
def test_deberta_with_its_scratch(mc, cuda_dev, monkeypatch):
    _four_states(t_db.test_deberta_matches_fp64_on_its_route, DB.DEBERTA_CASES, mc, cuda_dev, monkeypatch)


@pytest.mark.parametrize("case", PL.POOL_CASES, ids=lambda c: c.id)
def test_mean_pooling(case, cuda_dev, monkeypatch):
    _four_states(t_pl.test_mean_pooling_matches_fp64_on_its_branch, PL.POOL_CASES, case, cuda_dev, monkeypatch)


# ---- fp16x2 ------------------------------------------------------------------------------------------------------------------
F16X2_BAR = 1e-4


def _f16x2_run(case, cuda_dev, monkeypatch):
    """the reference suite's call with arith="f16x2": branch counters of the case, deviation from fp64 within the fp16x2 bar"""
    from adaptive_classifier import _native as nv
    lib = nv.lib()
    enc = t_ref._encoder(case, cuda_dev)
    if not getattr(enc, "_f16x2_on", False):
        enc.enable_f16x2()
        enc._f16x2_on = True
    ids, types, mask = R.make_batch(case.batch)
    n_ln, n_at = lib.ac_gemm_ln_fusion_launches(), lib.ac_gemm_qkv_attn_launches()
    got = enc.encode_cls(ids, types, mask, arith="f16x2")
    torch.cuda.synchronize()
    d_ln, d_at = lib.ac_gemm_ln_fusion_launches() - n_ln, lib.ac_gemm_qkv_attn_launches() - n_at
    assert not enc.ln_fusion_aborted() and enc.f16x2_overflows == 0
    assert enc.last_one_launch == case.one_launch, case.id
    assert (d_ln > 0) == (case.ln_launches > 0) and (d_at > 0) == (case.attn_launches > 0), (case.id, d_ln, d_at)
    got = got.cpu()
    assert torch.isfinite(got).all()
    dev = R.deviation(case, got)
    print(f"[poison encoder] {case.id} f16x2: deviation {dev:.1e} (bar {F16X2_BAR:.0e}), ln {d_ln} attn {d_at}")
    assert dev <= F16X2_BAR, (case.id, dev)
    assert float((got.double().norm(dim=1) - 1).abs().max()) <= 1e-6


@pytest.mark.parametrize("cid", ["ln_768_T384", "ol_768_ragged"])
def test_f16x2_arithmetic(cid, cuda_dev, monkeypatch):
    case = R.BY_ID[cid]
    _four_states(_f16x2_run, [case], case, cuda_dev, monkeypatch)
    if not case.one_launch:                        # the fp16 planes were really used: other bits than the bf16x3 default
        enc = t_ref._encoder(case, cuda_dev)
        ids, types, mask = R.make_batch(case.batch)
        assert not torch.equal(enc.encode_cls(ids, types, mask, arith="f16x2"), enc.encode_cls(ids, types, mask))
