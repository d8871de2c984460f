// The fp32 row-stream core of the kNN sweeps: ONE load path and ONE k-loop for knn_sweep (knn_l2.hip: top-k candidate lists) and
// knn_range_sweep (knn_range.hip: radius classification).  Every store row is read from HBM once per query tile; the rows stream
// HBM -> VGPR (float4 per lane, no LDS round trip: nothing is shared between waves) into v_mfma_f32_16x16x4_f32 as the A operand,
// the query tile sits in LDS pre-scaled by -2 in B-fragment order.  What a sweep does with a finished 16-row tile is its epilogue.
// Both sweeps bound their error by the roundings of THIS chain (knn_sweep_gamma0, common.h): the bound is stated once because the
// chain exists once.
// The FILTERED forms of both sweeps fetch the 16 selection bits of a finished tile the same way (sweep_sel_bits).
// The exact fp64 value of a (row, query) pair -- the bits every search returns -- closes the file: one accumulation step and the two
// summation orders (a wave per pair, a lane per pair) that knn_exact.hip and knn_range.hip share.
// Included by the .hip files of the kNN searches only.  The functions are device code; the constants (kWaves, kGroup, kLdsLimit,
// Shape::KCOLS) are also what the host planners of those files size tiles, grids and LDS with.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace acknn {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kWaves = 8;               // waves per sweep block (2 per SIMD)
constexpr int kThreads = kWaves * 64;
constexpr int kGroup = 8;               // float4 loads in flight per lane per buffer
constexpr int kLdsLimit = 160 * 1024;   // LDS a sweep block may ask for

// One MFMA shape for every query-tile width: v_mfma_f32_16x16x4_f32.  A lane (row i = lane & 15,
// k-slice h = lane >> 4) loads float4 P[row0 + i][16*kb + 4*h ..]: 16 rows x 64 contiguous bytes per
// wave load (two instructions per 128-B line; the 32x32x2 shape would touch 32 rows x 32 B).  A query
// tile is J sub-tiles of 16 queries; the A fragment is reused for the J B-fragments.
struct Shape {
    static constexpr int ROWS = 16, KSPLIT = 4, NACC = 4, KCOLS = 16;
    typedef f32x4 acc_t;
    static __device__ __forceinline__ acc_t mfma(float a, float b, acc_t c) {
        return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
    }
    // C/D layout: col = lane & 15, row = 4 * (lane >> 4) + r
    static __device__ __forceinline__ int acc_row(int r, int lane) { return 4 * (lane >> 4) + r; }
};

// XCD-aware block id remap (cdna guide T1, bijective form): hardware places block b on XCD
// b % 8; give each XCD a contiguous range of virtual ids so that the nqt query-tile blocks
// of one row group (consecutive virtual ids) share one L2.
__device__ __forceinline__ int xcd_remap(int b, int nblk) {
    const int x = b & 7, s = b >> 3;
    const int q = nblk >> 3, r = nblk & 7;
    const int base = (x < r) ? x * (q + 1) : r * (q + 1) + (x - r) * q;
    return base + s;
}

// Stage query tile qt (16 J queries) into LDS: slot (jj, kb, ksub, j) = -2 * Q[qt*TQ + 16*jj + j][16*kb + 4*ksub ..+3], zeros past
// nq and past D.  J * ng * kGroup * 64 float4 slots; the caller's barrier publishes them.
template <int J>
__device__ __forceinline__ void stage_queries(f32x4* Qs, const float* Q, int64_t ldQ, int D, int nq, int ng, int qt, int tid) {
    constexpr int TQ = 16 * J;
    const int c4_per_q = ng * kGroup * Shape::KSPLIT;     // float4 columns per query (padded)
    const int total = TQ * c4_per_q;
    for (int t = tid; t < total; t += kThreads) {
        const int j = t / c4_per_q;
        const int c4 = t - j * c4_per_q;
        const int kb = c4 / Shape::KSPLIT, ksub = c4 - kb * Shape::KSPLIT;
        const int qrow = qt * TQ + j;
        const int col = 4 * c4;
        f32x4 val = {0.f, 0.f, 0.f, 0.f};
        if (qrow < nq && col < D) {
            const float* src = Q + (size_t)qrow * ldQ + col;
            val.x = -2.f * src[0];
            if (col + 1 < D) val.y = -2.f * src[1];
            if (col + 2 < D) val.z = -2.f * src[2];
            if (col + 3 < D) val.w = -2.f * src[3];
        }
        Qs[((j >> 4) * (ng * kGroup) + kb) * 64 + ksub * 16 + (j & 15)] = val;
    }
}

// Stream the 128-row tiles T = it * G + g (it = 0, 1, ...) of row group g through the MFMA chain against the staged query tile.
// Owns the prefetch state, both load buffers, acc[J], the lane's running sum of squares and the driver loop.  At the end of each
// tile this wave's 16 rows are complete: epilogue(acc, nsq, row_base) gets acc[jj][r] = -2 (p.q)~ of row row_base + acc_row(r, lane)
// and query column 16 jj + (lane & 15), and nsq = the lane's quarter (k-slice lane >> 4) of |p|^2 of row row_base + (lane & 15).
// Rows >= N of the last tile hold the last row again: the epilogue masks them.  Dp = round_up(D, 4): float4 loads at col < Dp are
// in bounds (zero padded); zeros = >= 16 B of zeros, 16-byte aligned.
template <int J, typename Epilogue>
__device__ __forceinline__ void stream_tiles(const float* P, int64_t N, int64_t ldP, int Dp, int ng, int G, int g, int64_t ntiles,
                                             const float* zeros, const f32x4* Qs, int lane, int wave, Epilogue&& epilogue) {
    typedef Shape S;
    typedef S::acc_t acc_t;
    const int ksub = lane / S::ROWS;    // k sub-slice this lane feeds in the A/B layout
    const int arow = lane % S::ROWS;    // tile row this lane feeds in the A layout

    const int64_t my_tiles = (ntiles > g) ? (ntiles - 1 - g) / G + 1 : 0;
    const int64_t total = my_tiles * ng;

    f32x4 buf[2][kGroup];
    // prefetch state (flattened group counter -> tile, group)
    int64_t pf_tile = 0;
    int pf_grp = 0;
    const float* pf_ptr;
    auto tile_rowptr = [&](int64_t it) -> const float* {
        int64_t row = (it * G + g) * (int64_t)(kWaves * S::ROWS) + wave * S::ROWS + arow;
        if (row > N - 1) row = N - 1;
        return P + (size_t)row * ldP;
    };
    pf_ptr = tile_rowptr(0);

#define AC_PREFETCH(B)                                                                   \
    do {                                                                                 \
        const int kb0 = pf_grp * kGroup;                                                 \
        if ((kb0 + kGroup) * S::KCOLS <= Dp) { /* wave-uniform: whole group in bounds */ \
            _Pragma("unroll") for (int u = 0; u < kGroup; ++u)                           \
                buf[B][u] = *reinterpret_cast<const f32x4*>(pf_ptr + 4 * ksub + (kb0 + u) * S::KCOLS); \
        } else { /* tail group: out-of-range float4s are fetched from a zero block instead */ \
            _Pragma("unroll") for (int u = 0; u < kGroup; ++u) {                         \
                const int col = (kb0 + u) * S::KCOLS + 4 * ksub;                         \
                const float* src = col < Dp ? pf_ptr + col : zeros;                      \
                buf[B][u] = *reinterpret_cast<const f32x4*>(src);                        \
            }                                                                            \
        }                                                                                \
        if (++pf_grp == ng) { pf_grp = 0; ++pf_tile; pf_ptr = tile_rowptr(pf_tile); }    \
    } while (0)

    acc_t acc[J];
    float nsq = 0.f;
    int64_t cur_tile = 0;
    int cur_grp = 0;

#define AC_COMPUTE(B)                                                                    \
    do {                                                                                 \
        if (cur_grp == 0) {                                                              \
            _Pragma("unroll") for (int jj = 0; jj < J; ++jj)                             \
                _Pragma("unroll") for (int r = 0; r < S::NACC; ++r) acc[jj][r] = 0.f;    \
        }                                                                                \
        const f32x4* qsrc = Qs + (size_t)cur_grp * kGroup * 64 + lane;                   \
        const size_t jstride = (size_t)ng * kGroup * 64;                                 \
        f32x4 bq[J];                                                                     \
        _Pragma("unroll") for (int jj = 0; jj < J; ++jj) bq[jj] = qsrc[jj * jstride];    \
        _Pragma("unroll") for (int u = 0; u < kGroup; ++u) {                             \
            const f32x4 a = buf[B][u];                                                   \
            f32x4 b[J];                                                                  \
            _Pragma("unroll") for (int jj = 0; jj < J; ++jj) b[jj] = bq[jj];             \
            if (u + 1 < kGroup) { /* LDS reads one step ahead */                         \
                _Pragma("unroll") for (int jj = 0; jj < J; ++jj) bq[jj] = qsrc[jj * jstride + (u + 1) * 64]; \
            }                                                                            \
            _Pragma("unroll") for (int jj = 0; jj < J; ++jj) acc[jj] = S::mfma(a.x, b[jj].x, acc[jj]); \
            nsq = fmaf(a.x, a.x, nsq); nsq = fmaf(a.y, a.y, nsq);                        \
            _Pragma("unroll") for (int jj = 0; jj < J; ++jj) acc[jj] = S::mfma(a.y, b[jj].y, acc[jj]); \
            nsq = fmaf(a.z, a.z, nsq); nsq = fmaf(a.w, a.w, nsq);                        \
            _Pragma("unroll") for (int jj = 0; jj < J; ++jj) acc[jj] = S::mfma(a.z, b[jj].z, acc[jj]); \
            _Pragma("unroll") for (int jj = 0; jj < J; ++jj) acc[jj] = S::mfma(a.w, b[jj].w, acc[jj]); \
            __builtin_amdgcn_sched_barrier(0); /* keep the per-load consume order */     \
        }                                                                                \
        if (++cur_grp == ng) {                                                           \
            epilogue(acc, nsq, (cur_tile * G + g) * (int64_t)(kWaves * S::ROWS) + wave * S::ROWS); \
            nsq = 0.f; cur_grp = 0; ++cur_tile;                                          \
        }                                                                                \
    } while (0)

    // Loads are issued unconditionally (past the end they re-read the last row, clamped in
    // tile_rowptr) so that every path has the same number of loads in flight: a load inside a
    // branch makes hipcc's s_waitcnt accounting wait on the buffer it has just issued.
    if (total > 0) {
        AC_PREFETCH(0);
        for (int64_t gg = 0; gg < total; gg += 2) {
            AC_PREFETCH(1);
            AC_COMPUTE(0);
            AC_PREFETCH(0);
            if (gg + 1 < total) AC_COMPUTE(1);
        }
    }
#undef AC_PREFETCH
#undef AC_COMPUTE
}

// ---- FILTERED sweeps (acamd.h "FILTERED search"): local row r is selected iff bit (sel_bit0 + r) of the bitmap is set ----
// The 16 selection bits of a wave's tile (rows row_base .. row_base + 15, bit i = row row_base + i): they sit in at most two
// 64-bit words, fetched wave-uniformly through the SCALAR unit (constant address space, as knn_plane_sweep's norms: off the
// vmcnt queue the prefetched rows / the DMA ring sit in).  Bits of rows >= N are never read as rows: the second word is touched
// only if one of its rows exists, a tile past N reads nothing, and the callers test row < N besides.
__device__ __forceinline__ uint32_t sweep_sel_bits(const uint64_t* sel, int64_t sel_bit0, int64_t N, int64_t row_base) {
    if (row_base >= N) return 0u;
    typedef const uint64_t __attribute__((address_space(4)))* cup;
    const uint32_t rem = __builtin_amdgcn_readfirstlane((uint32_t)((sel_bit0 & 63) + row_base));     // (N < 2^31)
    const cup w = (cup)(uintptr_t)(sel + (sel_bit0 >> 6) + (rem >> 6));
    const int s = (int)(rem & 63u);
    uint64_t bits = w[0] >> s;
    if (s > 48 && row_base + (64 - s) < N) bits |= w[1] << (64 - s);
    return (uint32_t)bits & 0xffffu;
}

// ---- the exact fp64 value of a (row, query) pair ----
// One accumulation step: (p - q)^2, or p q (an fp32 product is exact in fp64, so fma(p, q, acc) is the fp64 sum of the exact
// products).
template <bool IP>
__device__ __forceinline__ double exact_term(float p, float q, double acc) {
    if constexpr (IP) {
        return fma((double)p, (double)q, acc);
    } else {
        const double e = (double)p - (double)q;
        return fma(e, e, acc);
    }
}
// WAVE order (knn_merge_rerank, the exact fallback, the range resolve / fill): four accumulators per lane over the float4 columns
// c4 = lane, lane + 64, ..., then this tail -- the (a0 + a1) + (a2 + a3) fold and the xor-shuffle tree.  Every lane returns the sum.
__device__ __forceinline__ double exact_wave_sum(double a0, double a1, double a2, double a3) {
    double a = (a0 + a1) + (a2 + a3);
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) a += __shfl_xor(a, o);
    return a;
}
// ... of one row: prow = the row (columns D .. 4 nc4 - 1 are zero, the store's contract), q4(c4) = the query's float4 column c4
// with zeros past D.
template <bool IP, typename Q4>
__device__ __forceinline__ double exact_wave(const float* prow, int nc4, int lane, Q4&& q4) {
    double a0 = 0, a1 = 0, a2 = 0, a3 = 0;
    for (int c4 = lane; c4 < nc4; c4 += 64) {
        const f32x4 p = *reinterpret_cast<const f32x4*>(prow + 4 * c4);
        const f32x4 qq = q4(c4);
        a0 = exact_term<IP>(p.x, qq.x, a0); a1 = exact_term<IP>(p.y, qq.y, a1);
        a2 = exact_term<IP>(p.z, qq.z, a2); a3 = exact_term<IP>(p.w, qq.w, a3);
    }
    return exact_wave_sum(a0, a1, a2, a3);
}
// LANE order (knn_small_exact, the small-store range search): one lane walks the D columns, four accumulators, the same fold.
template <bool IP>
__device__ __forceinline__ double exact_lane(const float* p, const float* qv, int D) {
    double a0 = 0, a1 = 0, a2 = 0, a3 = 0;
    int c = 0;
    for (; c + 3 < D; c += 4) {
        a0 = exact_term<IP>(p[c], qv[c], a0); a1 = exact_term<IP>(p[c + 1], qv[c + 1], a1);
        a2 = exact_term<IP>(p[c + 2], qv[c + 2], a2); a3 = exact_term<IP>(p[c + 3], qv[c + 3], a3);
    }
    for (; c < D; ++c) a0 = exact_term<IP>(p[c], qv[c], a0);
    return (a0 + a1) + (a2 + a3);
}

}  // namespace acknn
