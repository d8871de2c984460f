// Which kernel runs a GEMM: the whole host-side decision as one pure function.  Plain C++17 with no HIP in it, so a host compiler
// builds it alone (tests/test_gemm_plan_cpu.py).  gemm.hip fills a GemmEnv once per call (ac::gemm_env, the only reader of the
// environment, the device and the test hooks for dispatch), launch_gemm switches on the GemmPlan, and every takes / choose /
// applies predicate of gemm.hip and gemm_pipe.hip is a view of the plan or of the constants below: none has a rule of its own.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace acg {

enum { ACT_NONE = 0, ACT_RELU = 1, ACT_GELU = 2, ACT_GEGLU32 = 3 };
// compile-time epilogue classes for the hot encoder/head shapes; EPI_GENERIC keeps the runtime flags
enum { EPI_GENERIC = 0, EPI_BIAS = 1, EPI_BIAS_GELU = 2, EPI_BIAS_RES = 3, EPI_BIAS_RELU = 4,
       // GeGLU over 32-column blocks: output columns [64t, 64t+32) are the inputs and [64t+32, 64t+64) the gates of
       // result columns [32t, 32t+32) -- a wave's two 32x32 tiles hold input_j and gate_j in the same lane/register
       EPI_GEGLU32 = 5,
       EPI_IDENT = 6,          // store the accumulators as they are (second half of the fused-LayerNorm epilogue)
       EPI_BIAS_RES_LN = 7,    // bias + residual, then LayerNorm over the whole row (gemm_pipe.hip)
       EPI_QKV_ATTN = 8 };     // the fused QKV projection's tile = one head's q | k | v: self-attention in the epilogue (gemm_pipe.hip)

// ---- the thresholds ----
constexpr int kTileN = 128;                  // columns of every LDS-tiled block tile
constexpr int kStageK = 32;                  // stage depth of the tiled kernels: K % 32 == 0, K >= 32
constexpr int kTileMinM = 192;               // fewer rows never take a tiled kernel (nor operand planes)
constexpr int kRingMinK = 64;                // the ring-staged kernels (gemm_pipe.hip) need two stages' worth of K
constexpr unsigned kBlock4 = 256, kBlock8 = 512;   // threads of the 4-wave kernels (tile, split, planes, direct) and of the 8-wave ones
constexpr int kSmallM1 = 16, kSmallM2 = 32, kSmallMaxM = 64, kSmallMinN = 16, kSmallMinK = 8;     // small-M kernel: J = 1 / 2 / 4 groups of 16 rows
constexpr int kFewMinM = 65, kFewMaxM = 512, kFewMinK = 64;      // few-tile kernel: latency-bound shapes with 2 * (64 x 128 tiles) <= CUs
constexpr int64_t kFewMaxMac = (int64_t)1 << 30;                 // beyond, the fp32 matrix pipe (1/16 of the bf16 one) is the bound
constexpr int64_t kSplitKFewMaxMac = (int64_t)160 << 20;         // split-K callers prefer the few-tile kernel up to 256 x 768 x 768
constexpr double kTile128Bias = 1.15;        // the 128-row tile does ~15 % more work per staged byte: 64 rows only for a clear win
// 8-wave 256 x 128 tile: >= 3 CU-rounds of such tiles, or (almost) exactly ONE residency round (2 workgroups per CU, >= 85 % full)
// while the 128-row tiles would spill > 10 % into a second one (FFN1 at ~5000 packed token rows: 504 vs 984 tiles)
constexpr int kBigRounds = 3, kBigPerCu = 2, kBigFill10 = 17, kBigSpill10 = 33;
constexpr int kLnCfg = 124262, kLnBM = 128, kLnBN = 128, kLnMaxTilesN = 8;   // the one tile the fused LayerNorm epilogue is built for

enum { GEMM_REFUSE = 0, GEMM_SMALLM, GEMM_FEWTILES, GEMM_RING, GEMM_PLANES8, GEMM_PLANES, GEMM_SPLIT, GEMM_TILE, GEMM_DIRECT };
struct PipeRule { int N, K, cfg; };
struct PipeTable { int n = -1; PipeRule rules[16]; };             // n < 0: no runtime table (ac_gemm_set_pipe_table*)
struct GemmEnv {
    int cus = 0;                 // CUs this process's workgroups can land on
    int arith = 1, variant = 0;  // AC_GEMM_F32 (0) | _BF16X3 | _F16X2; ac_gemm_set_variant: 0 = default, 1 = two-buffer kernels only, >= 1000 = that ring cfg
    int force_tm = 0, force_tile256 = -1;        // AC_GEMM_TM: 1 | 2, else free; AC_GEMM_TILE256: >= 0 forces the 8-wave tile off / on
    bool fewtiles = true;        // AC_GEMM_FEWTILES=0 switches the few-tile kernel off
    PipeTable table, table_f16;
    bool split() const { return arith != 0; }
};
struct GemmQuery {
    int M = 0, N = 0, K = 0;
    bool a_kmaj = true, b_kmaj = true;         // A element (m, k) at A[m lda + k]; B element (k, n) at B[n ldb + k] (nn.Linear weight)
    bool aligned = true;                       // 16-byte aligned bases, lda and ldb multiples of 4
    bool a_planes = false, w_planes = false, c_planes = false, f16 = false;   // operands / result as planes; f16: fp16x2 planes
    int act = ACT_NONE;                        // the inputs of the epilogue classification: act and the next two lines
    float alpha = 1.f, beta = 0.f, drop_p = 0.f;
    bool bias = false, residual = false, mask = false, gate = false;
};
struct GemmPlan {
    int family = GEMM_REFUSE;
    int J = 0, tm = 0, cls = EPI_GENERIC, cfg = 0;       // small-M row groups; 64-row units of the block tile; epilogue class; ring cfg
    bool a_planes = false, c_planes = false;
    unsigned grid_x = 0, grid_y = 1, block = 0;             // in workgroups; threads of one
    const char* refusal = nullptr;                       // printf format; the shape's M, N, K are its arguments
};

inline int64_t tiles_of(int M, int N, int bm, int bn) { return (int64_t)((M + bm - 1) / bm) * ((N + bn - 1) / bn); }
inline bool tiled_shape(int M, int K) { return M >= kTileMinM && K >= kStageK && (K % kStageK) == 0; }
inline bool ring_shape(int M, int K) { return tiled_shape(M, K) && K >= kRingMinK; }
inline bool linear_takes_planes(int M, int N, int K, const GemmEnv& env) { return env.split() && N >= 1 && tiled_shape(M, K); }
inline bool pipe_takes(int M, int N, int K, int cls, bool c_planes) {
    if (!ring_shape(M, K) || N < 1) return false;
    if (c_planes) return (cls == EPI_BIAS || cls == EPI_BIAS_GELU || cls == EPI_GEGLU32) && (N % 8) == 0;
    return cls == EPI_BIAS || cls == EPI_BIAS_RES;
}
inline bool linear_f16x2_takes(int M, int N, int K, const GemmEnv& env) {
    return (env.variant == 0 || env.variant >= 1000) && ring_shape(M, K) && N >= 8 && (N % 8) == 0;
}
inline bool fewtiles_takes(int M, int N, int K, bool aligned, const GemmEnv& env) {
    return env.fewtiles && aligned && M >= kFewMinM && M <= kFewMaxM && (K % 8) == 0 && K >= kFewMinK &&
           2 * tiles_of(M, N, 64, kTileN) <= env.cus && (int64_t)M * N * K <= kFewMaxMac;
}

// Built-in ring configuration (cfg = tm tn wmw wnw ns pipe, one decimal digit each).  Every CU works through ceil(tiles / CUs) tiles
// whatever the residency, so a configuration's time goes as
//     ceil(tiles / CUs) * BM * BN / s(cfg)
// with s = its relative per-CU throughput once the chip is full (8192^3 and 20564-row sweeps of profiles/r03/gemm_sweep3.txt;
// the chip is power-limited at ~0.5 - 0.6 of the bf16x3 ceiling there, and bigger tiles move fewer bytes per MFMA).  The rule
// reproduces the measured best (or a configuration within ~2 % of it) on every bert-base / bert-large shape at ~5 k and ~20 k
// packed token rows.  The two-buffer kernels of gemm.hip are not candidates: no measured shape has them ahead of the best
// ring configuration (they stay for A given as fp32, for epilogues outside pipe_takes, and behind ac_gemm_set_variant(1)).
// f16: the fp16x2 kernels' relative throughputs differ in one place (profiles/r04/f16x2_probe_base.txt: QKV at 5141 rows 256 x 192
// ring of 4 60 us, 192 x 256 68 us) -- their loop is paced by the operand fetch, and 256 x 192 with a ring of 4 fetches best
struct Cand { int cfg, bm, bn; double s; };
constexpr Cand kCands[] = {{244232, 256, 256, 1.05}, {234232, 256, 192, 0.90}, {322432, 192, 256, 0.92},
                           {224242, 256, 128, 0.90}, {124262, 128, 128, 0.82}, {222232, 128, 128, 0.87}};
inline int builtin_choose(int M, int N, int cls, bool f16, int64_t cus) {
    int best = 0;
    double best_cost = 0;
    for (const Cand& c : kCands) {
        if (cls == EPI_GEGLU32 && (c.cfg / 10000) % 10 != 2) continue;       // (fused GeGLU pairs the two column tiles of a 64-column wave tile)
        const int64_t tiles = tiles_of(M, N, c.bm, c.bn);
        double sp = c.s;
        if (f16 && c.cfg == 234232) sp = 0.95;
        if (c.cfg == 222232 && 2 * tiles < 3 * cus) sp = 0.78;               // two-per-CU kernel with mostly one workgroup per CU
        const double t = (double)((tiles + cus - 1) / cus) * c.bm * c.bn / sp;
        if (best == 0 || t < best_cost) { best_cost = t; best = c.cfg; }
    }
    if (f16 && best == 234232) best = 234242;
    return best;
}
// per-shape configuration of the default dispatch (0 = the two-buffer tile kernels): a runtime table takes precedence
inline int pipe_choose(int M, int N, int K, int cls, const GemmEnv& env) {
    if (env.table.n < 0) return builtin_choose(M, N, cls, false, env.cus);
    for (int i = 0; i < env.table.n; ++i) if (env.table.rules[i].N == N && env.table.rules[i].K == K) return env.table.rules[i].cfg;
    return 0;
}
// fp16x2 operands (never 0: there is no other kernel for them): its own table, else the tile the bf16x3 rule picks -- the round
// quantisation argument is the same, and the fused-LayerNorm launches need the same 128 x 128 tile in both arithmetics
inline int pipe_choose_f16(int M, int N, int K, const GemmEnv& env) {
    for (int i = 0; i < env.table_f16.n; ++i) if (const PipeRule& r = env.table_f16.rules[i]; r.N == N && r.K == K && r.cfg) return r.cfg;
    return builtin_choose(M, N, EPI_BIAS, true, env.cus);
}
inline int epilogue_class(const GemmQuery& q) {
    const bool plain = q.alpha == 1.f && q.beta == 0.f && q.bias && !q.mask && !q.gate && q.drop_p == 0.f;
    if (plain && !q.residual && q.act == ACT_NONE) return EPI_BIAS;
    if (plain && !q.residual && q.act == ACT_GELU) return EPI_BIAS_GELU;
    if (plain && !q.residual && q.act == ACT_RELU) return EPI_BIAS_RELU;
    if (plain && q.residual && q.act == ACT_NONE) return EPI_BIAS_RES;
    if (plain && !q.residual && q.act == ACT_GEGLU32) return EPI_GEGLU32;
    return EPI_GENERIC;
}

inline GemmPlan gemm_plan(const GemmQuery& q, const GemmEnv& env) {
    GemmPlan p;
    const int M = q.M, N = q.N, K = q.K;
    const bool nt = q.a_kmaj && q.b_kmaj, cp = q.c_planes;
    auto refuse = [&p](const char* why) { p.family = GEMM_REFUSE; p.refusal = why; return p; };
    auto ring = [&p, M, N](int cfg) {                    // grid and block of a ring configuration, from its digits
        const int tm = cfg / 100000 % 10, tn = cfg / 10000 % 10, wmw = cfg / 1000 % 10, wnw = cfg / 100 % 10;
        p.family = GEMM_RING; p.cfg = cfg; p.block = 64u * wmw * wnw; p.grid_x = tm && tn && p.block ? (unsigned)tiles_of(M, N, 32 * tm * wmw, 32 * tn * wnw) : 0;
        return p;
    };
    p.a_planes = q.a_planes; p.c_planes = cp;
    if (q.f16) {                                         // fp16x2 planes in: ring-staged kernels only (ac::linear_f16x2)
        if (!linear_f16x2_takes(M, N, K, env)) return refuse("linear_f16x2: %d x %d x %d does not take the ring-staged kernel");
        p.cls = q.act == ACT_GELU ? EPI_BIAS_GELU : (q.residual ? EPI_BIAS_RES : EPI_BIAS);
        return ring(env.variant >= 1000 ? env.variant : pipe_choose_f16(M, N, K, env));
    }
    if (q.act == ACT_GEGLU32 && !(cp && q.a_planes)) return refuse("gemm: fused GeGLU needs the pre-split kernel");
    if ((q.a_planes || cp) && !(nt && q.aligned && linear_takes_planes(M, N, K, env) && q.w_planes))
        return refuse("gemm: operand / result planes given for a shape that does not take the pre-split kernel");
    if (nt && q.aligned && M <= kSmallMaxM && K >= kSmallMinK && (K % 4) == 0 && N >= kSmallMinN) {
        p.family = GEMM_SMALLM; p.J = M <= kSmallM1 ? 1 : (M <= kSmallM2 ? 2 : 4);
        p.grid_x = (unsigned)((N + 15) / 16); p.block = kBlock8;
    } else if (nt && !q.a_planes && !cp && fewtiles_takes(M, N, K, q.aligned, env)) {
        p.family = GEMM_FEWTILES; p.grid_x = (unsigned)tiles_of(M, N, 32, 32); p.block = kBlock8;
    } else if (nt && q.aligned && tiled_shape(M, K)) {
        // pick the M-tile that wastes fewer CU-rounds: cost = rounds * (tile rows) * (resident blocks)
        const int64_t cus = env.cus, b256 = tiles_of(M, N, 256, kTileN), b128 = tiles_of(M, N, 128, kTileN), b64 = tiles_of(M, N, 64, kTileN);
        const int r128 = env.split() ? 3 : 2, r64 = r128 + 1;   // resident blocks per CU
        const int64_t cost128 = ((b128 + r128 * cus - 1) / (r128 * cus)) * 128 * r128;
        const int64_t cost64 = ((b64 + r64 * cus - 1) / (r64 * cus)) * 64 * r64;
        p.tm = (double)cost64 * kTile128Bias < (double)cost128 ? 1 : 2;
        if (env.force_tm == 1 || env.force_tm == 2) p.tm = env.force_tm;
        const int cls = p.cls = epilogue_class(q);
        if (q.act == ACT_GEGLU32 && !(cls == EPI_GEGLU32 && (N % 64) == 0))
            return refuse("gemm: the fused GeGLU epilogue needs planes output, a bias vector and N %% 64 == 0");
        const bool planes = env.split() && q.w_planes;   // (K % 32 == 0 here, so K % 16 == 0)
        // ring-staged kernel (gemm_pipe.hip): variant >= 1000 forces one configuration (A/B harness); variant 0 = the measured
        // per-shape choice of pipe_choose(), variant 1 = never
        if (planes && q.a_planes && pipe_takes(M, N, K, cls, cp)) {
            const int cfg = env.variant >= 1000 ? env.variant : (env.variant == 0 ? pipe_choose(M, N, K, cls, env) : 0);
            if (cfg) return ring(cfg);
        }
        const bool one_round256 = b256 <= kBigPerCu * cus && 10 * b256 >= kBigFill10 * cus && 10 * b128 > kBigSpill10 * cus;
        const bool big = planes && q.a_planes && (env.force_tile256 >= 0 ? env.force_tile256 != 0 : (b256 >= kBigRounds * cus || one_round256)) &&
                         (cls == EPI_BIAS || cls == EPI_BIAS_GELU || cls == EPI_BIAS_RES || cls == EPI_GEGLU32) &&
                         !(cls == EPI_GEGLU32 && !cp) && !(cls == EPI_BIAS_RES && cp);
        p.grid_x = (unsigned)(p.tm == 2 ? b128 : b64); p.block = kBlock4;
        if (big) {
            if (cp && (N % 8) != 0) return refuse("gemm: planes output needs N %% 8 == 0");
            p.family = GEMM_PLANES8; p.tm = 2; p.grid_x = (unsigned)b256; p.block = kBlock8;
        } else if (cp) {
            // result emitted as planes for the next GEMM: both operands pre-split, bias (+GELU) epilogues only
            if (!(planes && q.a_planes && (cls == EPI_BIAS || cls == EPI_BIAS_GELU || cls == EPI_GEGLU32) && (N % 8) == 0))
                return refuse("gemm: planes output needs pre-split operands, N %% 8 == 0 and a bias / bias+gelu epilogue");
            p.family = GEMM_PLANES;
        } else p.family = planes ? GEMM_PLANES : (env.split() ? GEMM_SPLIT : GEMM_TILE);
    } else {
        p.family = GEMM_DIRECT; p.grid_x = (unsigned)((N + 31) / 32); p.grid_y = (unsigned)((M + 31) / 32); p.block = kBlock4;
    }
    return p;
}
// shape halves of the fused epilogues' predicates (their switches and residency proofs: gemm_pipe.hip)
inline bool pipe_ln_shape(int M, int N, int K, const GemmEnv& env) {       // one tile per CU, and the default dispatch picks the LN tile anyway
    GemmQuery q;
    q.M = M; q.N = N; q.K = K; q.a_planes = q.w_planes = q.bias = q.residual = true;
    return env.split() && env.variant == 0 && ring_shape(M, K) && (N % kLnBN) == 0 && N / kLnBN <= kLnMaxTilesN &&
           tiles_of(M, N, kLnBM, kLnBN) <= env.cus && gemm_plan(q, env).cfg == kLnCfg;
}
inline bool qkv_attn_shape(int M, int H, int heads, int smax, const GemmEnv& env) {
    GemmQuery q;
    q.M = M; q.N = 3 * H; q.K = H; q.a_planes = q.w_planes = q.bias = true;
    return env.split() && env.variant == 0 && heads >= 1 && H == heads * 64 && ring_shape(M, H) && smax >= 1 && smax <= 64 &&
           gemm_plan(q, env).family == GEMM_RING;          // (not: a table that switches the ring kernels off)
}
// split-K slices of linear_f32_splitk (1 = none): as many as fill ~1.5 workgroups per CU, each at least 6 stages of 16 long and
// dividing the stage count; a_aligned: 16-byte aligned A, lda % 4 == 0; scratch_bytes = 0 without W planes or scratch
inline int splitk_slices(int M, int N, int K, bool a_aligned, size_t scratch_bytes, const GemmEnv& env) {
    const int64_t tiles = tiles_of(M, N, 64, kTileN);
    int ksplit = 1;
    if (scratch_bytes && env.split() && env.variant == 0 && M >= kFewMinM && M <= kFewMaxM && (N % 4) == 0 && (K % kStageK) == 0 &&
        a_aligned && 2 * tiles <= env.cus)
        for (int c = 2, nk = K / 16; c <= 32; ++c)
            if (nk % c == 0 && nk / c >= 6 && tiles * c <= (int64_t)env.cus * 3 / 2 && (size_t)c * M * N * sizeof(float) <= scratch_bytes) ksplit = c;
    return ksplit;
}

}  // namespace acg
