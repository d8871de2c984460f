"""GPU suite: `pooling="mean"` (AC_POOL_MEAN, pool_mean_normalize_kernel) of the HIP encoders against the fp64 pooled reference
of tests/encoder_pool_ref.py, on the dispatch branches of tests/encoder_ref.py's grid re-run with mean pooling.
tests/test_encoder_pool_cpu.py proves the reference, the bounds and the sensitivity; nothing here reads anything but the tables
of the two *_ref files.

Every case asserts
  - the unit mean-pooled vectors within the group's device bound (16 x the CPU-measured fp32 noise of the POOLED vector) of fp64
    on every compared row, finite everywhere, unit norm to 1e-6, an all-masked row exactly zero;
  - that the last layer took the token layers' route: 2 L fused-LayerNorm and L fused-attention launches where the CLS case
    records 2 (L - 1) and L - 1, never the one persistent launch, path and token count of the CLS case, no exchange gave up.

Observed on an MI355X: see the table at the end of this file (for the record -- no bound comes from it).
"""
import ctypes

import pytest
import torch

import encoder_ref as R
import encoder_pool_ref as P

pytestmark = pytest.mark.gpu

_SEEN = {}
_ENCODERS = {}
PATHS = {0: "packed", 1: "padded", 2: "padded_mask"}          # AC_BERT_PATH_*


@pytest.fixture(scope="module", autouse=True)
def _report(cuda_dev):
    yield
    _ENCODERS.clear()
    print(f"\n[encoder pool] {'family':12s} {'regime':12s} {'branch':20s} {'FP32_DEV_POOL':>13s} {'bound':>9s} {'observed':>9s}  worst case")
    for key in sorted(_SEEN):
        dev, cid = _SEEN[key]
        f = P.FP32_DEV_POOL[key[:2]]
        print(f"[encoder pool] {key[0]:12s} {key[1]:12s} {key[2]:20s} {f:13.0e} {R.KERNEL_FACTOR * f:9.1e} {dev:9.1e}  {cid}")


def _encoder(case, dev):
    from adaptive_classifier.encoder import HipBertEncoder, HipModernBertEncoder
    key = (case.model, case.unpad)
    if key not in _ENCODERS:
        cls = HipModernBertEncoder if case.model.family == "modernbert" else HipBertEncoder
        _ENCODERS[key] = cls(R.make_model(case.model), device=dev, unpad=case.unpad)
    return _ENCODERS[key]


def _run(case, dev, monkeypatch, pooling="mean", mask_override=None):
    """the case's device call with `pooling`; -> (rows on the host, d_ln, d_at, unpad reports, encoder)"""
    from adaptive_classifier import _native as nv, encoder as enc_mod
    lib = nv.lib()
    enc = _encoder(case, dev)
    ids, types, mask = R.make_batch(case.batch)
    if mask_override is not None:
        mask = mask_override
    b, H = case.batch.b, case.model.hidden
    reports = []
    real_unpad = lib.ac_bert_encode_cls_unpad

    def unpad_spy(*args):
        rc = real_unpad(*args)
        reports.append((args[12]._obj.value, PATHS[args[13]._obj.value]))
        return rc

    monkeypatch.setattr(lib, "ac_bert_encode_cls_unpad", unpad_spy)
    for k, v in case.env:
        monkeypatch.setenv(k, v)
    if case.max_tokens:
        monkeypatch.setattr(enc_mod, "MAX_TOKENS", case.max_tokens)
    out = torch.full((b, H + case.ldo_extra), 7.0, device=dev) if case.ldo_extra else None
    gave_up = getattr(enc, "ln_gave_up", 0)
    try:
        nv.check(lib.ac_gemm_set_ln_fusion(case.ln_fusion), "ac_gemm_set_ln_fusion")
        n_ln, n_at = lib.ac_gemm_ln_fusion_launches(), lib.ac_gemm_qkv_attn_launches()
        got = enc.encode_cls(ids, types, mask, out=out, force_layered=case.layered, arith=case.arith, pooling=pooling)
        torch.cuda.synchronize()
        d_ln, d_at = lib.ac_gemm_ln_fusion_launches() - n_ln, lib.ac_gemm_qkv_attn_launches() - n_at
        aborted = case.model.family != "modernbert" and enc.ln_fusion_aborted()
    finally:
        nv.check(lib.ac_gemm_set_ln_fusion(1), "ac_gemm_set_ln_fusion")
        monkeypatch.setattr(lib, "ac_bert_encode_cls_unpad", real_unpad)
    assert not aborted and getattr(enc, "ln_gave_up", 0) == gave_up, "an in-launch exchange gave up"
    return got.cpu(), d_ln, d_at, reports, enc


@pytest.mark.parametrize("case", P.POOL_CASES, ids=lambda c: c.id)
def test_mean_pooling_matches_fp64_on_its_branch(case, cuda_dev, monkeypatch):
    got, d_ln, d_at, reports, enc = _run(case, cuda_dev, monkeypatch)
    b, S, H = case.batch.b, case.batch.S, case.model.hidden

    # the branch: the last layer went the way of the token layers
    if case.model.family != "modernbert":
        assert enc.last_one_launch is False, case.id
    assert d_ln == case.ln_launches, (case.id, "LayerNorm-fused launches", d_ln)
    assert d_at == case.attn_launches, (case.id, "attention-fused launches", d_at)
    tokens = b * S if case.tokens < 0 else case.tokens
    assert enc.last_tokens == tokens, (case.id, enc.last_tokens, tokens)
    if case.path is None:
        assert reports == [], (case.id, reports)
    else:
        assert reports == [(tokens, case.path)], (case.id, reports)

    # the numbers
    if case.ldo_extra:
        assert bool((got[:, H:] == 0).all()), "padding columns of the output rows"
        got = got[:, :H]
    rows = R.compared_rows(case.batch)
    assert torch.isfinite(got).all(), case.id                   # every row, the all-masked ones too
    assert bool((got[~rows] == 0).all()), (case.id, "an all-masked row is exactly zero")
    dev = P.deviation(case, got)
    norm = float((got[rows].double().norm(dim=1) - 1).abs().max())
    key = case.group + (case.branch,)
    if dev >= _SEEN.get(key, (-1.0, ""))[0]:
        _SEEN[key] = (dev, case.id)
    print(f"[encoder pool] {case.id:30s} {case.branch:20s} deviation {dev:.1e} (bound {P.device_bound(case):.1e})  |norm - 1| {norm:.1e}")
    assert dev <= P.device_bound(case), (case.id, dev, P.device_bound(case))
    assert norm <= 1e-6, (case.id, norm)


@pytest.mark.parametrize("cid", ["T192_all_fused", "attn_straddle_exchange", "pm_holes", "mb_S40_planes_packed", "mb_lonely_query",
                                 "sa_longest129", "chunks_fused_then_not"])
def test_the_same_call_twice_gives_the_same_bits(cid, cuda_dev, monkeypatch):
    case = P.POOL_BY_ID[cid]
    a = _run(case, cuda_dev, monkeypatch)[0]
    b = _run(case, cuda_dev, monkeypatch)[0]
    assert torch.equal(a, b), cid


def test_all_masked_row_is_exactly_zero_and_finite(cuda_dev, monkeypatch):
    """pm_empty_row: row 2 has no admitted token -- max(count, 1) keeps the division finite, the row is 0 / 1e-12 = 0 exactly"""
    for cid in ("pm_empty_row", "pm_empty_row_planes"):
        case = P.POOL_BY_ID[cid]
        got = _run(case, cuda_dev, monkeypatch)[0]
        assert torch.isfinite(got).all(), cid
        assert not bool(R.compared_rows(case.batch)[2]) and bool((got[2] == 0).all()), cid
        assert float(got[R.compared_rows(case.batch)].norm(dim=1).min()) > 0.999


def test_padding_columns_are_zeroed(cuda_dev, monkeypatch):
    case = P.POOL_BY_ID["last_ldo_wide"]
    got = _run(case, cuda_dev, monkeypatch)[0]
    H = case.model.hidden
    assert got.shape[1] == H + 24 and bool((got[:, H:] == 0).all())            # (the buffer was filled with 7.0)
    assert P.deviation(case, got[:, :H]) <= P.device_bound(case)


def test_one_token_sequence_mean_equals_its_cls_row(cuda_dev, monkeypatch):
    """A sequence of one token: the mean IS the CLS row -- two routes of the last layer (token layer + pooling against the CLS
    tail), each within its own bound of the same fp64 vector."""
    case = P.POOL_BY_ID["ol_T32_forced_layered"]
    assert case.batch.lengths[2] == 1
    mean = _run(case, cuda_dev, monkeypatch, pooling="mean")[0]
    cls = _run(R.BY_ID[case.id], cuda_dev, monkeypatch, pooling="cls")[0]
    assert float((P.pooled_reference(case)[2] - R.reference(case)[2]).abs().max()) < 1e-15
    d = float((mean[2] - cls[2]).abs().max())
    print(f"[encoder pool] one-token row: |mean - cls| = {d:.1e}")
    assert d <= P.device_bound(case) + R.device_bound(case), d
    assert float((mean[0] - cls[0]).abs().max()) > 1e-2                         # (the longer rows do differ)


@pytest.mark.parametrize("cid", ["T192_all_fused", "ol_T33_packed", "mb_S40_planes_packed"])
def test_explicit_cls_is_the_default_bit_for_bit(cid, cuda_dev, monkeypatch):
    """pool_opt 0 (what every call passed before the field existed) against pool_opt 1 (AC_POOL_CLS, explicit)"""
    from adaptive_classifier import _native as nv
    case = R.BY_ID[cid]
    enc = _encoder(case, cuda_dev)
    default = _run(case, cuda_dev, monkeypatch, pooling="cls")[0]
    assert enc._call_cfg(pooling="cls").pool_opt == nv.AC_POOL_DEFAULT
    real = enc._call_cfg

    def explicit(*a, **k):
        cfg = real(*a, **k)
        cfg.pool_opt = nv.AC_POOL_CLS
        return cfg

    monkeypatch.setattr(enc, "_call_cfg", explicit)
    enc.__dict__.pop("_cfg_cache", None)
    try:
        got = _run(case, cuda_dev, monkeypatch, pooling="cls")[0]
    finally:
        monkeypatch.setattr(enc, "_call_cfg", real)
        enc.__dict__.pop("_cfg_cache", None)
    assert torch.equal(default, got), cid
    assert R.deviation(case, got) <= R.device_bound(case)


def test_poolings_do_not_leak_between_objects(cuda_dev):
    """Pooling is a PER-CALL option inside ac_bert_config (modelled on test_per_call_options_do_not_leak_between_objects): two
    encoders with different poolings, per-call overrides on one of them and two classifiers on ONE shared encoder, interleaved --
    each returns, bit for bit, what its pooling returns alone."""
    from adaptive_classifier import AdaptiveClassifier
    from adaptive_classifier.encoder import HipBertEncoder
    from helpers import HashTokenizer
    case = P.POOL_BY_ID["T192_all_fused"]
    model = R.make_model(case.model)
    ids, types, mask = R.make_batch(case.batch)
    enc_cls = HipBertEncoder(model, device=cuda_dev)
    enc_mean = HipBertEncoder(model, device=cuda_dev, pooling="mean")
    assert enc_cls.pooling == "cls" and enc_mean.pooling == "mean"
    ref = {"cls": enc_cls.encode_cls(ids, types, mask).clone(), "mean": enc_mean.encode_cls(ids, types, mask).clone()}
    assert R.deviation(case, ref["cls"]) <= R.device_bound(case) and P.deviation(case, ref["mean"]) <= P.device_bound(case)
    assert float((ref["cls"] - ref["mean"]).abs().max()) > 1e-2
    for _ in range(2):
        assert torch.equal(enc_mean.encode(ids, types, mask), ref["mean"])
        assert torch.equal(enc_cls.encode(ids, types, mask), ref["cls"])
        for name in ("mean", "cls", "cls", "mean"):
            assert torch.equal(enc_cls.encode_cls(ids, types, mask, pooling=name), ref[name]), name
            assert torch.equal(enc_mean.encode_cls(ids, types, mask, pooling=name), ref[name]), name
    with pytest.raises(ValueError, match="pooling"):
        enc_cls.encode_cls(ids, types, mask, pooling="max")
    clfs = {name: AdaptiveClassifier("synthetic", device="cuda:0", config={"pooling": name}, encoder=enc_cls, tokenizer=HashTokenizer())
            for name in ("cls", "mean")}
    plain = AdaptiveClassifier("synthetic", device="cuda:0", encoder=enc_mean, tokenizer=HashTokenizer())   # the config rules, not the encoder
    for _ in range(2):
        for name in ("mean", "cls"):
            assert torch.equal(clfs[name]._encode_tokens(ids, types, mask), ref[name]), name
        assert torch.equal(plain._encode_tokens(ids, types, mask), ref["cls"])
    assert enc_cls.pooling == "cls" and enc_mean.pooling == "mean"
    with pytest.raises(ValueError, match="pooling"):
        AdaptiveClassifier("synthetic", device="cuda:0", config={"pooling": "max"}, encoder=enc_cls, tokenizer=HashTokenizer())
    # out-of-range words are refused by the encode entries too
    bad = enc_cls._call_cfg()
    bad.pool_opt = 9
    from adaptive_classifier import _native as nv
    out = torch.empty((case.batch.b, case.model.hidden), device=cuda_dev)
    ws = torch.empty(enc_cls.workspace_bytes(case.batch.b, case.batch.S), dtype=torch.uint8, device=cuda_dev)
    rc = nv.lib().ac_bert_encode_cls(ctypes.byref(bad), ctypes.byref(enc_cls.weights), nv.ptr(ids.to(cuda_dev)), None, None, case.batch.b,
                                     case.batch.S, nv.ptr(out), out.stride(0), nv.ptr(ws), ws.numel(), nv.stream_ptr(cuda_dev))
    assert rc == -1 and b"pool_opt" in nv.lib().ac_last_error()


def test_the_comparison_sees_a_mistake_made_on_the_device(cuda_dev, monkeypatch):
    """The harness itself: pm_left_padded called with a mask of all ones is the "mask ignored" mistake made on the device -- the
    padding rows are summed into the mean.  It must sit many bounds from the reference, as far as the CPU's `include_pad` mutant
    says a pooling that ignores the mask sits (0.19 against 0.19), and within ONE bound of the fp64 twin of that very call.

    The twin is the fp64 forward of the same ids with the all-ones mask pooled over every row.  It is NOT the `include_pad`
    mutant to a bound: an all-ones mask cannot reach the pooling without reaching the attention, where it admits the padding
    KEYS too, which moves the hidden states themselves (fp64: twin 0.1904, include_pad 0.1943 from the reference).  So the
    distance is held to the twin within one bound, and to the mutant's distance within the 4e-3 by which the two fp64 figures
    differ, rounded up to 5e-3."""
    case = P.POOL_BY_ID["pm_left_padded"]
    ids, types, mask = R.make_batch(case.batch)
    got = _run(case, cuda_dev, monkeypatch, mask_override=torch.ones_like(mask))[0]
    far = P.deviation(case, got)
    model = R.make_model(case.model)
    hs = []
    R.FORWARD[case.model.family](model.state_dict(), model.config, ids, types, torch.ones_like(mask), hidden_out=hs)
    twin = P.masked_mean_normalize(hs[-1], torch.ones_like(mask).bool())
    rows = R.compared_rows(case.batch)
    twin_far = float((twin - P.pooled_reference(case))[rows].abs().max())
    mutant = P.mutant_distance(case, "include_pad")
    print(f"[encoder pool] all-ones mask on the device: {far:.6f} from the reference; fp64 twin {twin_far:.6f}; include_pad mutant {mutant:.6f}; "
          f"device - twin {float((got.double() - twin)[rows].abs().max()):.1e}")
    assert far > 4 * P.device_bound(case), far
    assert float((got.double() - twin)[rows].abs().max()) <= P.device_bound(case)
    assert abs(far - twin_far) <= P.device_bound(case)
    assert abs(far - mutant) <= 5e-3, (far, mutant)


# For the record (no bound comes from it): one run on an MI355X; the observed maximum per (family, regime, branch) next to the
# CPU-measured fp32 figure of the pooled vector and the bound in force.
#
#   family       regime       branch               FP32_DEV_POOL     bound  observed  worst case
#   bert         peaked       attn_fused                   2e-07   3.2e-06   1.3e-07  last_T_lt_4b
#   bert         peaked       attn_fused_boundary          2e-07   3.2e-06   7.6e-08  attn_straddle_boundary
#   bert         peaked       attn_standalone              2e-07   3.2e-06   1.1e-07  attn_longest65
#   bert         peaked       no_planes_f32                2e-07   3.2e-06   6.3e-08  T192_f32_arith
#   bert         peaked       padded_mask                  2e-07   3.2e-06   6.5e-08  pm_empty_row
#   bert         peaked       padded_mask_planes           2e-07   3.2e-06   6.7e-08  pm_empty_row_planes
#   bert         peaked       planes_unfused               2e-07   3.2e-06   4.3e-08  T192_both_off
#   bert         peaked       small_layered                2e-07   3.2e-06   7.5e-08  ol_T32_forced_layered
#   bert         peaked_wide  attn_fused                   9e-08   1.4e-06   1.9e-07  ln_768_T384
#   distilbert   peaked       attn_fused                   1e-07   1.6e-06   8.9e-08  distilbert_packed
#   distilbert   peaked       one_launch                   1e-07   1.6e-06   3.6e-08  distilbert_one_launch
#   electra      peaked       attn_fused                   2e-07   3.2e-06   6.7e-08  electra_packed
#   electra      peaked       one_launch                   2e-07   3.2e-06   5.5e-08  electra_one_launch
#   modernbert   scaled       mb_no_planes                 1e-07   1.6e-06   4.6e-08  mb_lonely_query
#   modernbert   scaled       mb_planes                    1e-07   1.6e-06   9.2e-08  mb_b200
#   roberta      flat         attn_fused                   7e-08   1.1e-06   5.2e-08  roberta_packed
#   roberta      flat         one_launch                   7e-08   1.1e-06   3.3e-08  roberta_one_launch
#   xlm-roberta  flat         one_launch                   4e-08   6.4e-07   3.3e-08  xlm-roberta_one_launch
#
# 58 tests of this module and tests/test_classifier_pool_gpu.py in 7.3 s.  The device sits at 0.3 .. 2.1 x the fp32 figure of its group
# (ln_768_T384: 1.9e-7 against 9e-8, a seventh of its bound): a correct fp32 forward, nowhere near the bound.  The all-ones call on
# pm_left_padded: 0.190376 from the reference, its fp64 twin 0.190376 (device - twin 4.9e-8), the include_pad mutant 0.194344.
