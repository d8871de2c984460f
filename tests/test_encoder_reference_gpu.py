"""GPU suite: the HIP encoders (`ac_bert_encode_cls*`, `ac_modernbert_encode_cls*`, adaptive_classifier/encoder.py) against the fp64
reference of tests/encoder_ref.py, one case per dispatch branch.  tests/test_encoder_ref_cpu.py proves the reference, the
admission of every case and the grid's sensitivity to a list of plausible kernel mistakes; nothing here reads anything but
tests/encoder_ref.py's tables.

Every case builds the encoder, runs it the way the table says (arithmetic, LayerNorm fusion, environment switches, forced
layering, output stride, chunk size), and asserts
  - the unit CLS vectors within the group's device bound (16 x the measured fp32 noise, at most 1e-5) of fp64 on every compared row
    (an all-masked input row is a legal input and is left out; the OTHER rows of its batch are compared),
  - unit norm to 1e-6,
  - that the expected branch really ran: used_one_launch, the LayerNorm-fusion and attention-fusion launch counters, the path and
    token count ac_bert_encode_cls_unpad reports, enc.last_tokens -- and no exchange gave up.
Branches without a counter (planes, q_cls_only, the 32-key CLS tiles) are fixed by the shapes; tests/encoder_ref.py states the
dispatch conditions they were read off.

Observed on an MI355X: see the table at the end of this file (for the record -- no bound comes from it).
"""
import time

import pytest
import torch

import encoder_ref as R

pytestmark = pytest.mark.gpu

_SEEN = {}                              # (family, regime, branch) -> (observed maximum, case)
_ENCODERS = {}
PATHS = {0: "packed", 1: "padded", 2: "padded_mask"}          # AC_BERT_PATH_*


def _see(case, value):
    key = case.group + (case.branch,)
    if value >= _SEEN.get(key, (-1.0, ""))[0]:
        _SEEN[key] = (float(value), case.id)


@pytest.fixture(scope="module", autouse=True)
def _report(cuda_dev):
    t0 = time.time()
    yield
    _ENCODERS.clear()
    print(f"\n[encoder reference] module wall time {time.time() - t0:.1f} s")
    print(f"[encoder reference] {'family':12s} {'regime':12s} {'branch':20s} {'FP32_DEV':>9s} {'bound':>9s} {'observed':>9s}  worst case")
    for key in sorted(_SEEN):
        dev, cid = _SEEN[key]
        f = R.FP32_DEV[key[:2]]
        print(f"[encoder reference] {key[0]:12s} {key[1]:12s} {key[2]:20s} {f:9.0e} {R.PATH_FACTOR.get(key[2], R.KERNEL_FACTOR) * f:9.1e} "
              f"{dev:9.1e}  {cid}")


def _encoder(case, dev):
    from adaptive_classifier.encoder import HipBertEncoder, HipModernBertEncoder
    key = (case.model, case.unpad)
    if key not in _ENCODERS:
        model = R.make_model(case.model)
        cls = HipModernBertEncoder if case.model.family == "modernbert" else HipBertEncoder
        _ENCODERS[key] = cls(model, device=dev, unpad=case.unpad)
    return _ENCODERS[key]


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.id)
def test_encoder_matches_fp64_on_its_branch(case, cuda_dev, monkeypatch):
    from adaptive_classifier import _native as nv, encoder as enc_mod
    lib = nv.lib()
    enc = _encoder(case, cuda_dev)
    bert = case.model.family != "modernbert"
    ids, types, mask = R.make_batch(case.batch)
    b, S, H = case.batch.b, case.batch.S, case.model.hidden

    reports = []                        # (total_tokens, path) of every ac_bert_encode_cls_unpad call
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
    out = torch.full((b, H + case.ldo_extra), 7.0, device=cuda_dev) if case.ldo_extra else None
    gave_up = getattr(enc, "ln_gave_up", 0)
    try:
        nv.check(lib.ac_gemm_set_ln_fusion(case.ln_fusion), "ac_gemm_set_ln_fusion")
        n_ln, n_at = lib.ac_gemm_ln_fusion_launches(), lib.ac_gemm_qkv_attn_launches()
        got = enc.encode_cls(ids, types, mask, out=out, force_layered=case.layered, arith=case.arith)
        torch.cuda.synchronize()
        d_ln, d_at = lib.ac_gemm_ln_fusion_launches() - n_ln, lib.ac_gemm_qkv_attn_launches() - n_at
        aborted = bert and enc.ln_fusion_aborted()
    finally:
        nv.check(lib.ac_gemm_set_ln_fusion(1), "ac_gemm_set_ln_fusion")
    got = got.cpu()

    # the branch
    assert not aborted and getattr(enc, "ln_gave_up", 0) == gave_up, "an in-launch exchange gave up"
    if bert:
        assert enc.last_one_launch == case.one_launch, (case.id, enc.last_one_launch)
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
    assert torch.isfinite(got[rows]).all(), case.id
    dev = R.deviation(case, got)
    norm = float((got[rows].double().norm(dim=1) - 1).abs().max())
    _see(case, dev)
    print(f"[encoder reference] {case.id:30s} {case.branch:20s} deviation {dev:.1e} (bound {R.device_bound(case):.1e})  |norm - 1| {norm:.1e}")
    assert dev <= R.device_bound(case), (case.id, dev, R.device_bound(case))
    assert norm <= 1e-6, (case.id, norm)


def test_the_comparison_sees_a_mistake_made_on_the_device(cuda_dev):
    """The harness itself: the same encoder called WITHOUT the token types is the "no_types" mutant run on the device -- it must
    sit as far from the reference as the CPU's sensitivity table says (many bounds), and within the device bound of the fp64
    mutant."""
    case = R.BY_ID["T192_all_fused"]
    enc = _encoder(case, cuda_dev)
    ids, types, mask = R.make_batch(case.batch)
    got = enc.encode_cls(ids, None, mask).cpu()
    far = R.deviation(case, got)
    assert far > 4 * R.device_bound(case), far
    assert abs(far - R.mutant_distance(case, "no_types")) <= R.device_bound(case)


# For the record (no bound comes from it): one run on an MI355X, 72 cases in 5.7 s of module wall time; the observed maximum per
# (family, regime, branch) next to the CPU-measured fp32 figure and the bound in force.
#
#   family       regime       branch                FP32_DEV     bound  observed  worst case
#   bert         flat         attn_fused               9e-08   1.4e-06   1.3e-07  T200_of_100x2
#   bert         flat         attn_standalone          9e-08   1.4e-06   5.7e-08  sa_longest32
#   bert         flat         no_planes_f32            9e-08   1.4e-06   6.0e-08  ln_768_flat_f32
#   bert         flat         one_launch               9e-08   1.4e-06   4.9e-08  ol_128_flat
#   bert         flat         small_layered            9e-08   1.4e-06   5.3e-08  T150_of_100x2
#   bert         peaked       attn_fused               3e-07   4.8e-06   1.5e-07  last_b200
#   bert         peaked       attn_fused_boundary      3e-07   4.8e-06   1.3e-07  attn_ends_on_boundary_bl
#   bert         peaked       attn_standalone          3e-07   4.8e-06   1.6e-07  sa_dh32_longest129
#   bert         peaked       ln_fused                 3e-07   4.8e-06   1.1e-07  T192_attn_off
#   bert         peaked       no_planes_f32            3e-07   4.8e-06   6.9e-08  T192_f32_arith
#   bert         peaked       one_launch               3e-07   4.8e-06   8.9e-08  ol_T32_ragged_len1
#   bert         peaked       padded_mask              3e-07   4.8e-06   9.2e-08  pm_holes
#   bert         peaked       padded_mask_planes       3e-07   4.8e-06   1.0e-07  pm_empty_row_planes
#   bert         peaked       planes_unfused           3e-07   4.8e-06   1.0e-07  T192_both_off
#   bert         peaked       small_layered            3e-07   4.8e-06   8.2e-08  dh32_small_is_layered
#   bert         peaked_wide  attn_fused               3e-07   4.8e-06   3.9e-07  ln_1024_ragged_panel
#   bert         peaked_wide  ln_fused                 3e-07   4.8e-06   2.7e-07  ln_768_T384_attn_off
#   bert         peaked_wide  one_launch               3e-07   4.8e-06   9.2e-08  ol_768_ragged
#   bert         peaked_wide  planes_unfused           3e-07   4.8e-06   2.7e-07  ln_768_T384_off
#   distilbert   peaked       attn_fused               2e-07   3.2e-06   1.3e-07  distilbert_packed
#   distilbert   peaked       one_launch               2e-07   3.2e-06   7.3e-08  distilbert_one_launch
#   electra      peaked       attn_fused               2e-07   3.2e-06   1.0e-07  electra_packed
#   electra      peaked       one_launch               2e-07   3.2e-06   6.9e-08  electra_one_launch
#   modernbert   scaled       mb_no_planes             1e-07   1.6e-06   6.1e-08  mb_S17
#   modernbert   scaled       mb_planes                1e-07   1.6e-06   8.8e-08  mb_b200
#   roberta      flat         attn_fused               8e-08   1.3e-06   6.7e-08  roberta_packed
#   roberta      flat         one_launch               8e-08   1.3e-06   4.4e-08  roberta_one_launch
#   xlm-roberta  flat         attn_fused               8e-08   1.3e-06   6.7e-08  xlm-roberta_packed
#   xlm-roberta  flat         one_launch               8e-08   1.3e-06   4.4e-08  xlm-roberta_one_launch
#
# The device sits at 0.5 .. 1.4 x the fp32 figure of its group on every branch: a correct fp32 forward, nowhere near the bound.
