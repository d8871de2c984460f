"""GPU suite: the MPNet family through HipBertEncoder -- the relative position bias of `ac_bert_weights.attn_rel_bias` inside
attention_mfma_kernel / attention_cls_kernel (csrc/attention_core.h, csrc/bert.hip) -- against the fp64 reference of
tests/encoder_mpnet_ref.py.  tests/test_encoder_mpnet_cpu.py proves the reference, the bounds and the sensitivity; nothing here
reads anything but that helper's tables.

  parity          every case under the pooling it names: within the regime's device bound of fp64, with the route observed
                  (never the one launch, no fused-attention launch, the LayerNorm-fused launches of the shape, the token count);
  bias-off        an all-zero table against a NULL table pointer, stand-alone attention in both: the same bits;
  visibility      a table uploaded wrong (heads rolled, reversed along d) is seen; a constant added to one head's row is not;
  determinism, no leak into a BERT encoder of the same process, S > rel_span refused.
"""
import contextlib

import pytest
import torch

import encoder_ref as R
import encoder_mpnet_ref as M

pytestmark = pytest.mark.gpu

_ENCODERS = {}
_SEEN = {}
PATHS = {0: "packed", 1: "padded", 2: "padded_mask"}          # AC_BERT_PATH_*


@pytest.fixture(scope="module", autouse=True)
def _report(cuda_dev):
    yield
    _ENCODERS.clear()
    print(f"\n[encoder mpnet] {'regime':12s} {'FP32_DEV_MPNET':>14s} {'bound':>9s} {'observed':>9s}  worst case")
    for regime in sorted(_SEEN):
        dev, cid = _SEEN[regime]
        print(f"[encoder mpnet] {regime:12s} {M.FP32_DEV_MPNET[regime]:14.0e} {R.KERNEL_FACTOR * M.FP32_DEV_MPNET[regime]:9.1e} {dev:9.1e}  {cid}")


def _encoder(case, dev):
    from adaptive_classifier.encoder import make_encoder
    key = (case.model, case.unpad)
    if key not in _ENCODERS:
        enc = make_encoder(M.make_model(case.model), device=dev)
        enc.unpad = case.unpad
        _ENCODERS[key] = enc
    return _ENCODERS[key]


def _run(mc, dev, monkeypatch, enc=None):
    """the case's device call -> (rows on the host, d_ln, d_at, unpad reports, encoder)"""
    from adaptive_classifier import _native as nv
    lib = nv.lib()
    case = mc.case
    enc = enc or _encoder(case, dev)
    ids, types, mask = R.make_batch(case.batch)
    reports = []
    real_unpad = lib.ac_bert_encode_cls_unpad

    def unpad_spy(*args):
        rc = real_unpad(*args)
        reports.append((args[12]._obj.value, PATHS[args[13]._obj.value]))
        return rc

    monkeypatch.setattr(lib, "ac_bert_encode_cls_unpad", unpad_spy)
    for k, v in case.env:
        monkeypatch.setenv(k, v)
    gave_up = enc.ln_gave_up
    try:
        n_ln, n_at = lib.ac_gemm_ln_fusion_launches(), lib.ac_gemm_qkv_attn_launches()
        got = enc.encode_cls(ids, types, mask, arith=case.arith, pooling=mc.pooling)
        torch.cuda.synchronize()
        d_ln, d_at = lib.ac_gemm_ln_fusion_launches() - n_ln, lib.ac_gemm_qkv_attn_launches() - n_at
        aborted = enc.ln_fusion_aborted()
    finally:
        monkeypatch.setattr(lib, "ac_bert_encode_cls_unpad", real_unpad)
    assert not aborted and enc.ln_gave_up == gave_up, "an in-launch exchange gave up"
    return got.cpu(), d_ln, d_at, reports, enc


@contextlib.contextmanager
def _table(enc, new=None, null=False):
    """the encoder's device table replaced by `new` (same shape), or its pointer taken out of the weights struct"""
    saved, ptr = enc.rel_bias.clone(), enc.weights.attn_rel_bias
    try:
        if new is not None:
            enc.rel_bias.copy_(new.to(enc.rel_bias))
        if null:
            enc.weights.attn_rel_bias = None
        torch.cuda.synchronize()
        yield
    finally:
        torch.cuda.synchronize()
        enc.rel_bias.copy_(saved)
        enc.weights.attn_rel_bias = ptr
        torch.cuda.synchronize()


@pytest.mark.parametrize("mc", M.MPNET_CASES, ids=lambda c: c.id)
def test_mpnet_matches_fp64_on_its_route(mc, cuda_dev, monkeypatch):
    case = mc.case
    got, d_ln, d_at, reports, enc = _run(mc, cuda_dev, monkeypatch)
    b, S = case.batch.b, case.batch.S
    assert enc.weights.attn_rel_bias and enc.weights.rel_span == enc.ccfg.max_pos >= S
    assert enc.last_one_launch is False, mc.id
    assert d_at == 0, (mc.id, "attention-fused launches", d_at)
    assert d_ln == case.ln_launches, (mc.id, "LayerNorm-fused launches", d_ln)
    tokens = b * S if case.tokens < 0 else case.tokens
    assert enc.last_tokens == tokens, (mc.id, enc.last_tokens, tokens)
    if case.path is None:
        assert reports == [], (mc.id, reports)
    else:
        assert reports == [(tokens, case.path)], (mc.id, reports)
    assert torch.isfinite(got).all(), mc.id
    dev = M.deviation(mc, got)
    norm = float((got.double().norm(dim=1) - 1).abs().max())
    if dev >= _SEEN.get(mc.regime, (-1.0, ""))[0]:
        _SEEN[mc.regime] = (dev, mc.id)
    print(f"[encoder mpnet] {mc.id:28s} deviation {dev:.1e} (bound {M.device_bound(mc):.1e})  |norm - 1| {norm:.1e}  ln {d_ln} tokens {tokens}")
    assert dev <= M.device_bound(mc), (mc.id, dev, M.device_bound(mc))
    assert norm <= 1e-6, (mc.id, norm)


@pytest.mark.parametrize("cid", ["mp_S70_packed", "mp_S33_masked", "mp_dh32_S33"])
@pytest.mark.parametrize("pooling", ["cls", "mean"])
def test_zero_table_and_no_table_give_the_same_bits(cid, pooling, cuda_dev, monkeypatch):
    """The biased instantiation is the unbiased one plus one add: x + (+0) changes only -0, which neither the maximum nor 2^x
    sees.  AC_QKV_ATTN_FUSION=0 keeps the NULL-table run on the stand-alone attention the table run always takes."""
    monkeypatch.setenv("AC_QKV_ATTN_FUSION", "0")
    mc = M.BY_ID[f"{cid}-{pooling}"]
    enc = _encoder(mc.case, cuda_dev)
    with _table(enc, new=torch.zeros_like(enc.rel_bias)):
        zero = _run(mc, cuda_dev, monkeypatch)[0]
    with _table(enc, null=True):
        none, _, d_at, _, _ = _run(mc, cuda_dev, monkeypatch)
    assert d_at == 0
    assert torch.equal(zero, none), (mc.id, float((zero - none).abs().max()))
    assert M.mutant_distance(mc, "no_bias") > 8 * M.device_bound(mc)
    assert abs(M.deviation(mc, zero) - M.mutant_distance(mc, "no_bias")) <= M.device_bound(mc)      # ... and it IS the no_bias forward
    assert M.deviation(mc, _run(mc, cuda_dev, monkeypatch)[0]) <= M.device_bound(mc)                 # the table is back


@pytest.mark.parametrize("pooling", ["cls", "mean"])
def test_the_comparison_sees_a_wrong_table_on_the_device(pooling, cuda_dev, monkeypatch):
    mc = M.BY_ID["mp_S70_packed-" + pooling]
    enc = _encoder(mc.case, cuda_dev)
    good = enc.rel_bias.clone()
    for name, table, mutant in (("heads rolled", torch.roll(good, 1, dims=0), "bias_heads_rotated"),
                                ("reversed along d", torch.flip(good, dims=[1]), "bias_transposed")):
        with _table(enc, new=table):
            far = M.deviation(mc, _run(mc, cuda_dev, monkeypatch)[0])
        want = M.mutant_distance(mc, mutant)
        print(f"[encoder mpnet] {mc.id}: table {name}: {far:.6f} from the reference (fp64 mutant {mutant}: {want:.6f})")
        assert far > 8 * M.device_bound(mc), (name, far)
        assert abs(far - want) <= M.device_bound(mc), (name, far, want)       # the device made exactly that mistake


def test_a_constant_on_one_heads_row_changes_nothing(cuda_dev, monkeypatch):
    """softmax shift invariance: catches a bias applied after the running maximum was taken"""
    for pooling in ("cls", "mean"):
        mc = M.BY_ID["mp_S70_packed-" + pooling]
        enc = _encoder(mc.case, cuda_dev)
        shifted = enc.rel_bias.clone()
        shifted[1] += 3.0
        with _table(enc, new=shifted):
            dev = M.deviation(mc, _run(mc, cuda_dev, monkeypatch)[0])
        print(f"[encoder mpnet] {mc.id}: head 1's row + 3.0: deviation {dev:.1e}")
        assert dev <= M.device_bound(mc), dev


@pytest.mark.parametrize("cid", ["mp_S70_packed-cls", "mp_S33_masked-mean", "mp_768_planes-mean", "mp_small_T32-cls"])
def test_the_same_call_twice_gives_the_same_bits(cid, cuda_dev, monkeypatch):
    a = _run(M.BY_ID[cid], cuda_dev, monkeypatch)[0]
    b = _run(M.BY_ID[cid], cuda_dev, monkeypatch)[0]
    assert torch.equal(a, b), cid


def test_the_table_does_not_leak_into_a_bert_encoder(cuda_dev, monkeypatch):
    from adaptive_classifier import _native as nv
    from adaptive_classifier.encoder import HipBertEncoder
    lib = nv.lib()
    bert = R.BY_ID["T192_all_fused"]
    benc = HipBertEncoder(R.make_model(bert.model), device=cuda_dev)
    ids, types, mask = R.make_batch(bert.batch)

    def bert_call():
        n = lib.ac_gemm_qkv_attn_launches()
        out = benc.encode_cls(ids, types, mask).clone()
        torch.cuda.synchronize()
        return out, lib.ac_gemm_qkv_attn_launches() - n

    alone, launches = bert_call()
    assert launches == bert.attn_launches and not benc.weights.attn_rel_bias
    assert R.deviation(bert, alone) <= R.device_bound(bert)
    mc = M.BY_ID["mp_S33_packed-cls"]
    mine = _run(mc, cuda_dev, monkeypatch)[0]
    for _ in range(2):
        got, n = bert_call()
        assert torch.equal(got, alone) and n == launches
        assert torch.equal(_run(mc, cuda_dev, monkeypatch)[0], mine)
    assert M.deviation(mc, mine) <= M.device_bound(mc)


def test_longer_than_the_table_is_refused(cuda_dev):
    from adaptive_classifier import _native as nv
    mc = M.BY_ID["mp_S33_packed-cls"]
    enc = _encoder(mc.case, cuda_dev)
    ids, types, mask = R.make_batch(mc.case.batch)
    span = enc.weights.rel_span
    try:
        enc.weights.rel_span = 20                       # (the constructor's span is the position table's, which refuses first)
        for m in (mask, None):
            with pytest.raises(nv.NativeError, match="rel_span"):
                enc.encode_cls(ids, types, m)
    finally:
        enc.weights.rel_span = span
    assert M.deviation(mc, enc.encode_cls(ids, types, mask)) <= M.device_bound(mc)


# For the record (no bound comes from it): one run on an MI355X, the observed maximum per regime next to the CPU-measured fp32
# figure and the bound in force.
#
#   regime       FP32_DEV_MPNET     bound  observed  worst case
#   flat                  8e-08   1.3e-06   6.1e-08  mp_S140_packed-cls
#   peaked                2e-07   3.2e-06   1.7e-07  mp_T_lt_4b-cls
#   peaked_wide           2e-07   3.2e-06   2.0e-07  mp_768_planes-cls
#
# 38 tests of this module and tests/test_classifier_mpnet_gpu.py in 7.4 s.  Wrong tables on mp_S70_packed-cls: heads rolled 0.010215
# from the reference (fp64 mutant bias_heads_rotated 0.010215), reversed along d 0.015552 (bias_transposed 0.015552).
