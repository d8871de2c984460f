"""GPU suite: the DeBERTa-v2/v3 family through HipBertEncoder -- the position scores of `ac_bert_weights.attn_disentangled`
(position_scores_kernel) and their gather inside attention_mfma_kernel / attention_cls_kernel (csrc/attention_core.h, csrc/bert.hip)
-- against the fp64 reference of tests/encoder_deberta_ref.py.  tests/test_encoder_deberta_cpu.py proves the reference, the bounds
and the sensitivity; nothing here reads anything but that helper's tables.

  parity          every case under the pooling it names: within the regime's device bound of fp64, with the route observed
                  (never the one launch, no fused-attention launch, the LayerNorm-fused launches of the shape, the token count);
  terms off       zero PK / PQ with scale_factor 1 against a NULL attn_disentangled, stand-alone attention in both: the same bits;
  visibility      an index table reversed along d, PK and PQ swapped, heads rolled: each is seen, the first and the last as the
                  fp64 mutant that makes the same mistake;
  determinism, no leak into a BERT and an MPNet encoder of the same process, S > rel_span refused.
"""
import contextlib

import pytest
import torch

import encoder_ref as R
import encoder_deberta_ref as D

pytestmark = pytest.mark.gpu

_ENCODERS = {}
_SEEN = {}
PATHS = {0: "packed", 1: "padded", 2: "padded_mask"}          # AC_BERT_PATH_*


@pytest.fixture(scope="module", autouse=True)
def _report(cuda_dev):
    yield
    _ENCODERS.clear()
    print(f"\n[encoder deberta] {'regime':8s} {'FP32_DEV_DEBERTA':>16s} {'bound':>9s} {'observed':>9s}  worst case")
    for regime in sorted(_SEEN):
        dev, cid = _SEEN[regime]
        print(f"[encoder deberta] {regime:8s} {D.FP32_DEV_DEBERTA[regime]:16.0e} {R.KERNEL_FACTOR * D.FP32_DEV_DEBERTA[regime]:9.1e} {dev:9.1e}  {cid}")


def _encoder(case, dev):
    from adaptive_classifier.encoder import make_encoder
    key = (case.model, case.unpad)
    if key not in _ENCODERS:
        enc = make_encoder(D.make_model(case.model), device=dev)
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
def _tables(enc, pos_key=None, pos_query=None, rel_index=None, scale_factor=None, null=False):
    """the encoder's device tables replaced (same shapes), or the struct's pointer taken out of the weights"""
    saved = ([t.clone() for t in enc.pos_key], [t.clone() for t in enc.pos_query], enc.rel_index.clone(), enc._dis.scale_factor,
             enc.weights.attn_disentangled)
    try:
        for dst, new in ((enc.pos_key, pos_key), (enc.pos_query, pos_query)):
            if new is not None:
                for t, n in zip(dst, new):
                    t.copy_(n.to(t))
        if rel_index is not None:
            enc.rel_index.copy_(rel_index.to(enc.rel_index))
        if scale_factor is not None:
            enc._dis.scale_factor = scale_factor
        if null:
            enc.weights.attn_disentangled = None
        torch.cuda.synchronize()
        yield
    finally:
        torch.cuda.synchronize()
        for dst, old in ((enc.pos_key, saved[0]), (enc.pos_query, saved[1])):
            for t, o in zip(dst, old):
                t.copy_(o)
        enc.rel_index.copy_(saved[2])
        enc._dis.scale_factor = saved[3]
        enc.weights.attn_disentangled = saved[4]
        torch.cuda.synchronize()


@pytest.mark.parametrize("mc", D.DEBERTA_CASES, ids=lambda c: c.id)
def test_deberta_matches_fp64_on_its_route(mc, cuda_dev, monkeypatch):
    case = mc.case
    got, d_ln, d_at, reports, enc = _run(mc, cuda_dev, monkeypatch)
    b, S = case.batch.b, case.batch.S
    assert enc.weights.attn_disentangled and not enc.weights.attn_rel_bias and enc._dis.rel_span == enc.ccfg.max_pos >= S
    assert enc._dis.scale_factor == 1 + len(D._terms(D.make_model(case.model).config)) and enc._dis.rel_rows == 2 * D.POSITION_BUCKETS
    assert enc.last_one_launch is False, mc.id
    assert d_at == 0, (mc.id, "attention-fused launches", d_at)
    assert d_ln == case.ln_launches, (mc.id, "LayerNorm-fused launches", d_ln)
    tokens = b * S if case.tokens < 0 else case.tokens
    assert enc.last_tokens == tokens, (mc.id, enc.last_tokens, tokens)
    if case.path is None:
        assert reports == [], (mc.id, reports)
    else:
        assert reports == [(tokens if case.path == "packed" else b * S, case.path)], (mc.id, reports)
    assert torch.isfinite(got).all(), mc.id
    dev = D.deviation(mc, got)
    norm = float((got.double().norm(dim=1) - 1).abs().max())
    if dev >= _SEEN.get(mc.regime, (-1.0, ""))[0]:
        _SEEN[mc.regime] = (dev, mc.id)
    print(f"[encoder deberta] {mc.id:28s} deviation {dev:.1e} (bound {D.device_bound(mc):.1e})  |norm - 1| {norm:.1e}  ln {d_ln} tokens {tokens}")
    assert dev <= D.device_bound(mc), (mc.id, dev, D.device_bound(mc))
    assert norm <= 1e-6, (mc.id, norm)


@pytest.mark.parametrize("cid", ["db_S40_planes", "db_holes", "db_ragged9"])
@pytest.mark.parametrize("pooling", ["cls", "mean"])
def test_zero_tables_and_no_struct_give_the_same_bits(cid, pooling, cuda_dev, monkeypatch):
    """With PK = PQ = 0 and scale_factor 1 the gathered terms are +0 and the scale is the plain 1 / sqrt(64): x + (+0) changes only
    -0, which neither the maximum nor 2^x sees.  AC_QKV_ATTN_FUSION=0 keeps the run without the struct on the stand-alone attention
    the run with it always takes."""
    monkeypatch.setenv("AC_QKV_ATTN_FUSION", "0")
    mc = D.BY_ID[f"{cid}-{pooling}"]
    enc = _encoder(mc.case, cuda_dev)
    zeros = [torch.zeros_like(t) for t in enc.pos_key]
    with _tables(enc, pos_key=zeros, pos_query=zeros, scale_factor=1):
        zero = _run(mc, cuda_dev, monkeypatch)[0]
    with _tables(enc, null=True):
        none, _, d_at, _, _ = _run(mc, cuda_dev, monkeypatch)
    assert d_at == 0
    assert torch.equal(zero, none), (mc.id, float((zero - none).abs().max()))
    off = ("drop_c2p", "drop_p2c", "scale_sqrt_d")
    want = float((D._pooled(mc, mut=off) - D.reference(mc)).abs().max())
    assert want > 8 * D.device_bound(mc)
    assert abs(D.deviation(mc, zero) - want) <= D.device_bound(mc)                                   # ... and it IS the forward without the terms
    assert D.deviation(mc, _run(mc, cuda_dev, monkeypatch)[0]) <= D.device_bound(mc)                 # the tables are back


@pytest.mark.parametrize("pooling", ["cls", "mean"])
def test_the_comparison_sees_wrong_tables_on_the_device(pooling, cuda_dev, monkeypatch):
    mc = D.BY_ID["db_S40_planes-" + pooling]
    enc = _encoder(mc.case, cuda_dev)
    pk, pq, idx = [t.clone() for t in enc.pos_key], [t.clone() for t in enc.pos_query], enc.rel_index.clone()
    wrong = (("index reversed along d", dict(rel_index=torch.flip(idx, dims=[0])), "index_sign_flipped"),
             ("heads rolled", dict(pos_key=[torch.roll(t, 64, dims=1) for t in pk], pos_query=[torch.roll(t, 64, dims=1) for t in pq]),
              "pos_heads_rolled"),
             ("PK and PQ swapped", dict(pos_key=pq, pos_query=pk), None))
    for name, kw, mutant in wrong:
        with _tables(enc, **kw):
            far = D.deviation(mc, _run(mc, cuda_dev, monkeypatch)[0])
        print(f"[encoder deberta] {mc.id}: {name}: {far:.6f} from the reference" +
              (f" (fp64 mutant {mutant}: {D.mutant_distance(mc, mutant):.6f})" if mutant else ""))
        assert far > 8 * D.device_bound(mc), (name, far)
        if mutant:
            assert abs(far - D.mutant_distance(mc, mutant)) <= D.device_bound(mc), (name, far)       # the device made exactly that mistake
    assert D.deviation(mc, _run(mc, cuda_dev, monkeypatch)[0]) <= D.device_bound(mc)


@pytest.mark.parametrize("cid", ["db_S70_flat-cls", "db_holes-mean", "db_S40_planes-mean", "db_small_T32-cls", "db_T_lt_4b-cls"])
def test_the_same_call_twice_gives_the_same_bits(cid, cuda_dev, monkeypatch):
    a = _run(D.BY_ID[cid], cuda_dev, monkeypatch)[0]
    b = _run(D.BY_ID[cid], cuda_dev, monkeypatch)[0]
    assert torch.equal(a, b), cid


def test_row_chunks_share_one_scratch(cuda_dev, monkeypatch):
    """MAX_TOKENS = 160: the 8 sequences of 40 positions go through as two chunks of 4, each sized (workspace and position-score
    scratch) for 4 x 40; the rows are the one-chunk rows to the bound (a chunk of < 192 token rows runs on fp32 activations)."""
    from adaptive_classifier import encoder as E
    mc = D.BY_ID["db_S40_planes-mean"]
    enc = _encoder(mc.case, cuda_dev)
    ids, types, mask = R.make_batch(mc.case.batch)
    monkeypatch.setattr(E, "MAX_TOKENS", 160)
    got = enc.encode_cls(ids, types, mask, pooling="mean").cpu()
    assert enc.last_tokens == mc.case.tokens
    assert enc._dis.scratch_bytes >= enc.disentangled_scratch_bytes(4, 40)
    assert D.deviation(mc, got) <= D.device_bound(mc)


def test_the_tables_do_not_leak_into_a_bert_or_an_mpnet_encoder(cuda_dev, monkeypatch):
    import encoder_mpnet_ref as M
    from adaptive_classifier import _native as nv
    from adaptive_classifier.encoder import HipBertEncoder, make_encoder
    lib = nv.lib()
    bert = R.BY_ID["T192_all_fused"]
    benc = HipBertEncoder(R.make_model(bert.model), device=cuda_dev)
    ids, types, mask = R.make_batch(bert.batch)
    mp = M.BY_ID["mp_S33_packed-cls"]
    menc = make_encoder(M.make_model(mp.case.model), device=cuda_dev)
    mids, mtypes, mmask = R.make_batch(mp.case.batch)

    def others():
        n = lib.ac_gemm_qkv_attn_launches()
        out = benc.encode_cls(ids, types, mask).clone()
        torch.cuda.synchronize()
        launches = lib.ac_gemm_qkv_attn_launches() - n
        return out, launches, menc.encode_cls(mids, mtypes, mmask).clone()

    alone, launches, malone = others()
    assert launches == bert.attn_launches and not benc.weights.attn_disentangled and not menc.weights.attn_disentangled
    assert R.deviation(bert, alone) <= R.device_bound(bert) and M.deviation(mp, malone) <= M.device_bound(mp)
    mc = D.BY_ID["db_S40_planes-cls"]
    mine = _run(mc, cuda_dev, monkeypatch)[0]
    for _ in range(2):
        got, n, mgot = others()
        assert torch.equal(got, alone) and n == launches and torch.equal(mgot, malone)
        assert torch.equal(_run(mc, cuda_dev, monkeypatch)[0], mine)
    assert D.deviation(mc, mine) <= D.device_bound(mc)


def test_longer_than_rel_span_is_refused(cuda_dev):
    from adaptive_classifier import _native as nv
    mc = D.BY_ID["db_S40_planes-cls"]
    enc = _encoder(mc.case, cuda_dev)
    ids, types, mask = R.make_batch(mc.case.batch)
    span = enc._dis.rel_span
    try:
        enc._dis.rel_span = 20                          # (the constructor's span is ac_bert_config.max_pos, which refuses first)
        for m in (mask, None):
            with pytest.raises(nv.NativeError, match="rel_span"):
                enc.encode_cls(ids, types, m)
    finally:
        enc._dis.rel_span = span
    with pytest.raises(nv.NativeError):                 # ... and the family's own rule: S <= rel_span = max_position_embeddings
        enc.encode_cls(torch.full((2, span + 1), 1000), None, None)
    assert D.deviation(mc, enc.encode_cls(ids, types, mask)) <= D.device_bound(mc)


# For the record (no bound comes from it): one run on an MI355X, the observed maximum per regime next to the CPU-measured fp32
# figure and the bound in force.
#
#   regime   FP32_DEV_DEBERTA     bound  observed  worst case
#   flat                7e-08   1.1e-06   6.2e-08  db_S70_flat-cls
#   peaked              2e-07   3.2e-06   2.8e-07  db_noshare-cls
#
# 40 tests of this module and tests/test_classifier_deberta_gpu.py in 7 s.  Wrong tables on db_S40_planes-cls: index reversed along
# d 0.049112 from the reference (fp64 mutant index_sign_flipped 0.049112), heads rolled 0.047419 (pos_heads_rolled 0.047419), PK and
# PQ swapped 0.041208.
