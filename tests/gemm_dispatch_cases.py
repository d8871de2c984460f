"""The fixed case list of the GEMM dispatch fixture (tests/data/gemm_dispatch_parent.json) and the code that runs one case.

Shared by tools/gemm_dispatch_probe.py (records kernel name, grid, block and an output hash per case under a kernel trace) and
tests/test_gemm_dispatch_gpu.py (re-runs the cases and compares the hashes).  One case = one call of a public entry = one
kernel launch, or a refusal.  The cases cover every leaf of csrc/gemm_plan.h and both sides of its thresholds, with K of 8..96
so each stays far under a millisecond; the plan depends on the CU count, which the fixture records (256 on MI355X).

Inputs are closed-form integer arithmetic (no library RNG), so the fixture stays valid across numpy / torch versions."""
import hashlib

import numpy as np

F32, BF16X3 = 0, 1


def case(id, entry, M, N, K, **kw):
    c = dict(id=id, entry=entry, M=M, N=N, K=K, arith=BF16X3, variant=0, table=None, act=0, res=False, planes="", cplanes=False,
             lda_pad=0, transA=0, transB=1, alpha=1.0, beta=0.0)
    assert set(kw) <= set(c), kw
    c.update(kw)
    return c


CASES = [
    # ---- small-M (M <= 64, N >= 16, K >= 8, K % 4 == 0): J = 1 / 2 / 4 row groups, ragged columns, K % 8 != 0 ----
    case("smallm_16x16x8", "linear_f32", 16, 16, 8),
    case("smallm_17x16x8", "linear_f32", 17, 16, 8, act=1),
    case("smallm_33x24x12", "linear_f32", 33, 24, 12, res=True),
    case("smallm_64x24x12", "linear_f32", 64, 24, 12, act=2),
    case("smallm_N15_direct", "linear_f32", 64, 15, 64),
    # ---- few-tile (65 <= M <= 512, K >= 64, K % 8 == 0, 2 * tiles <= CUs) ----
    case("fewtiles_65x8x64", "linear_f32", 65, 8, 64),
    case("fewtiles_512x128x64", "linear_f32", 512, 128, 64, act=1, res=True),
    case("fewtiles_192x128x64_over_tiled", "linear_f32", 192, 128, 64),
    case("fewtiles_K56_direct", "linear_f32", 65, 8, 56),
    case("rows513_split", "linear_f32", 513, 136, 96, act=2),
    case("rows513_tile_f32", "linear_f32", 513, 136, 96, arith=F32, act=2),
    # ---- tiled ----
    case("rows513_misaligned_lda_direct", "linear_f32", 513, 136, 96, lda_pad=1),
    case("tile128_wins_8256x1024x32", "linear_f32", 8256, 1024, 32),
    case("tile64_wins_8256x1024x32_f32", "linear_f32", 8256, 1024, 32, arith=F32, res=True),
    case("tile_relu_f32", "linear_f32", 513, 136, 96, arith=F32, act=1),
    case("split_generic_relu_res", "linear_f32", 513, 136, 96, act=1, res=True),
    case("wplanes_only_A_fp32", "linear_bf16x3", 513, 136, 96, planes="w", res=True),
    # ---- operand planes (ac_linear_bf16x3) ----
    case("planes_192x8x32_below_ring_K", "linear_bf16x3", 192, 8, 32, planes="aw"),
    case("planes_192x8x32_cplanes", "linear_bf16x3", 192, 8, 32, planes="aw", cplanes=True),
    case("rows191_no_planes", "linear_bf16x3", 191, 136, 64, planes="aw"),
    case("ring_bias", "linear_bf16x3", 192, 136, 64, planes="aw"),
    case("ring_bias_res", "linear_bf16x3", 192, 136, 64, planes="aw", res=True),
    case("ring_bias_cplanes", "linear_bf16x3", 192, 136, 64, planes="aw", cplanes=True),
    case("ring_gelu_cplanes", "linear_bf16x3", 192, 136, 64, planes="aw", act=2, cplanes=True),
    case("gelu_fp32_out_planes_kernel", "linear_bf16x3", 192, 136, 64, planes="aw", act=2),
    case("relu_outside_pipe_takes", "linear_bf16x3", 192, 136, 64, planes="aw", act=1),
    case("res_cplanes_refused", "linear_bf16x3", 192, 136, 64, planes="aw", res=True, cplanes=True),
    case("ring_geglu_cplanes_N128", "linear_bf16x3", 192, 128, 64, planes="aw", act=3, cplanes=True),
    case("v1_bias", "linear_bf16x3", 192, 136, 64, planes="aw", variant=1),
    case("v1_bias_res", "linear_bf16x3", 192, 136, 64, planes="aw", res=True, variant=1),
    case("v1_bias_cplanes", "linear_bf16x3", 192, 136, 64, planes="aw", cplanes=True, variant=1),
    case("v1_gelu_cplanes", "linear_bf16x3", 192, 136, 64, planes="aw", act=2, cplanes=True, variant=1),
    case("v1_gelu", "linear_bf16x3", 192, 136, 64, planes="aw", act=2, variant=1),
    case("v1_relu", "linear_bf16x3", 192, 136, 64, planes="aw", act=1, variant=1),
    case("v1_geglu_cplanes_N128", "linear_bf16x3", 192, 128, 64, planes="aw", act=3, cplanes=True, variant=1),
    case("table_empty_ring_off", "linear_bf16x3", 192, 136, 64, planes="aw", table=""),
    case("table_names_cfg", "linear_bf16x3", 192, 136, 64, planes="aw", table="136x64=222232"),
    case("forced_cfg_224242", "linear_bf16x3", 192, 136, 64, planes="aw", variant=224242),
    # 8-wave 256 x 128 tile (below the ring's K): >= 3 CU-rounds of tiles; exactly one residency round
    case("planes8_three_rounds_res", "linear_bf16x3", 8192, 3072, 32, planes="aw", res=True),
    case("planes8_one_round_gelu_cplanes", "linear_bf16x3", 5141, 3072, 32, planes="aw", act=2, cplanes=True),
    case("planes_tm2_below_8wave", "linear_bf16x3", 4096, 3072, 32, planes="aw"),
    # ---- fp16x2 planes: ring kernels only ----
    case("f16x2_bias", "linear_f16x2", 192, 136, 64),
    case("f16x2_bias_res", "linear_f16x2", 192, 136, 64, res=True),
    case("f16x2_gelu_cplanes", "linear_f16x2", 192, 136, 64, act=2, cplanes=True),
    # ---- ac_gemm_f32: the four transpose combinations, alpha and beta set ----
    case("gemm_nt_smallm", "gemm_f32", 40, 24, 20, transA=0, transB=1, alpha=1.5, beta=0.5),
    case("gemm_nn_direct", "gemm_f32", 40, 24, 20, transA=0, transB=0, alpha=1.5, beta=0.5),
    case("gemm_tn_direct", "gemm_f32", 40, 24, 20, transA=1, transB=0, alpha=1.5, beta=0.5),
    case("gemm_tt_direct", "gemm_f32", 40, 24, 20, transA=1, transB=1, alpha=1.5, beta=0.5),
]


def _mat(rows, cols, a, b, scale):
    """x[i, j] = ((a i + b j) mod 65521) / 65521 - 1/2, times scale: full-mantissa fp32 values from integer arithmetic"""
    i = np.arange(rows, dtype=np.int64)[:, None]
    j = np.arange(cols, dtype=np.int64)[None, :]
    return ((((a * i + b * j) % 65521).astype(np.float64) / 65521.0 - 0.5) * scale).astype(np.float32)


def inputs(c):
    M, N, K = c["M"], c["N"], c["K"]
    A = _mat(M, K, 7919, 104729, 2.0)
    W = _mat(N, K, 15485863, 32452843, 2.0 / np.sqrt(K))
    bias = _mat(1, N, 0, 49979687, 1.0)[0].copy()
    R = _mat(M, N, 86028121, 67867967, 4.0) if c["res"] or c["entry"] == "gemm_f32" else None
    return A, W, bias, R


def run_case(nv, dev, c):
    """(rc, sha256 of the output bytes or None).  Sets and restores the process-wide dispatch switches."""
    import torch
    lib, st = nv.lib(), nv.stream_ptr(dev)
    M, N, K = c["M"], c["N"], c["K"]
    A, W, bias, R = inputs(c)
    split = lib.ac_split_bf16x3
    before = lib.ac_gemm_get_arith()
    nv.check(lib.ac_gemm_set_arith(c["arith"]), "ac_gemm_set_arith")
    nv.check(lib.ac_gemm_set_variant(c["variant"]), "ac_gemm_set_variant")
    nv.check(lib.ac_gemm_set_pipe_table(None if c["table"] is None else c["table"].encode()), "ac_gemm_set_pipe_table")
    try:
        bd = torch.from_numpy(bias).to(dev)
        Rd = torch.from_numpy(R).to(dev) if c["res"] else None
        out = torch.zeros((M, N), device=dev)
        if c["entry"] == "gemm_f32":
            Ad = torch.from_numpy(np.ascontiguousarray(A.T if c["transA"] else A)).to(dev)          # (m, k) at A[k lda + m] when transposed
            Bd = torch.from_numpy(np.ascontiguousarray(W if c["transB"] else W.T)).to(dev)          # (k, n) at B[n ldb + k] when transposed
            out = torch.from_numpy(R).to(dev)                                                        # beta reads C
            rc = lib.ac_gemm_f32(c["transA"], c["transB"], M, N, K, c["alpha"], nv.ptr(Ad), Ad.shape[1], nv.ptr(Bd), Bd.shape[1],
                                 c["beta"], nv.ptr(out), N, st)
        elif c["entry"] == "linear_f32":
            lda = K + c["lda_pad"]
            Ad = torch.zeros((M, lda), device=dev)
            Ad[:, :K] = torch.from_numpy(A).to(dev)
            Wd = torch.from_numpy(W).to(dev)
            rc = lib.ac_linear_f32(nv.ptr(Ad), lda, nv.ptr(Wd), K, nv.ptr(bd), nv.ptr(Rd), N, nv.ptr(out), N, M, N, K, c["act"], st)
        else:
            Ad, Wd = torch.from_numpy(A).to(dev), torch.from_numpy(W).to(dev)
            f16 = c["entry"] == "linear_f16x2"
            per = 2 if f16 else 3
            Ap = torch.zeros(per * M * K, dtype=torch.int16, device=dev)
            Wp = torch.zeros(per * N * K, dtype=torch.int16, device=dev)
            NO = N // 2 if c["act"] == 3 else N
            if c["cplanes"]:
                out = torch.zeros(per * M * NO, dtype=torch.int16, device=dev)
            C, Cp = (None, nv.ptr(out)) if c["cplanes"] else (nv.ptr(out), None)
            if f16:                                               # operands x 2^6 and w 2^10 (common.h kF16OutScale)
                nv.check(lib.ac_split_f16x2(nv.ptr(Ad), K, M, K, 6, nv.ptr(Ap), st), "ac_split_f16x2")
                nv.check(lib.ac_split_f16x2(nv.ptr(Wd), K, N, K, 10, nv.ptr(Wp), st), "ac_split_f16x2")
                rc = lib.ac_linear_f16x2(nv.ptr(Ap), nv.ptr(Wp), nv.ptr(bd), nv.ptr(Rd), N, C, N, Cp, M, N, K, c["act"], st)
            else:
                nv.check(split(nv.ptr(Ad), K, M, K, nv.ptr(Ap), st), "ac_split_bf16x3")
                nv.check(split(nv.ptr(Wd), K, N, K, nv.ptr(Wp), st), "ac_split_bf16x3")
                rc = lib.ac_linear_bf16x3(nv.ptr(Ad), K, nv.ptr(Ap) if "a" in c["planes"] else None, nv.ptr(Wd), K,
                                          nv.ptr(Wp) if "w" in c["planes"] else None, nv.ptr(bd), nv.ptr(Rd), N, C, NO, Cp,
                                          M, N, K, c["act"], st)
        torch.cuda.synchronize(dev)
        return rc, (hashlib.sha256(out.cpu().numpy().tobytes()).hexdigest() if rc == 0 else None)
    finally:
        lib.ac_gemm_set_arith(before)
        lib.ac_gemm_set_variant(0)
        lib.ac_gemm_set_pipe_table(None)
