// kNN site of the hot path: exact squared-L2 top-k over the prototype store.
// Replaces faiss.IndexFlatL2.search as called at
//   /root/reference/src/adaptive_classifier/memory.py:113-114
// (third-party faiss-cpu>=1.7.4, requirements.txt:4 -- not vendored).
//
// This file: the three sweeps that build the candidate lists, their planners and the search entry points.  Every route ends in
// the exact stages of knn_exact.hip (merge + fp64 re-rank + certificate, exact fallback), all on one stream, no host
// synchronisation.  The planner rule and the host helpers the range search shares (ac::knn_sweep_shape and what follows it in
// common.h) are defined here too:
//
//  knn_sweep<TQ>      the HBM sweep.  Every prototype row is read from HBM exactly once per
//                     query tile of TQ queries.  Load path and k-loop are the fp32 row-stream core of knn_stream.h
//                     (stage_queries + stream_tiles), which the range search's knn_range_sweep (knn_range.hip) runs on too:
//                     the query tile lives in LDS, pre-scaled by -2 and pre-arranged in MFMA B-fragment order; prototype
//                     rows stream HBM -> VGPR (float4 per lane, no LDS round trip: nothing is shared between
//                     waves) and go straight into v_mfma_f32_16x16x4_f32 as the A operand.  What is written here is the
//                     epilogue: acc[row][query] = |p|^2 - 2 q.p  (|p|^2 is folded in by one
//                     extra MFMA whose A operand is the lane's running sum of squares).
//                     Each lane owns ONE query column, so the running threshold tau_q is one
//                     register; a candidate is pushed to the block's per-query LDS list only if
//                     acc < tau_q (rare after warm-up).  Lists are pruned to the k' = k+pad best
//                     by a wave-level rank-by-counting pass, which also tightens tau_q.
//  knn_sweep_ring     the same sweep for <= 16 queries: rows by non-temporal LDS-DMA, queries in registers (see there).
//  knn_plane_sweep    one pass over a PREPARED store's fp16 plane for <= 64 queries (see there); larger batches take the
//                     GEMM-form sweep of knn_batch.hip, launched from ac_knn_l2_topk_batch below.
//
// Inner-product search (ac_knn_ip_topk, faiss.IndexFlatIP.search) runs through the same sweeps and exact stages, instantiated with IP = true:
// the sweep value is -2 (p.q)~ (the |p|^2 fold is dropped), and every later stage ranks by the exact key -(p.q) ascending.
//
// Roofline: algorithmic bytes per sweep = N*D*4; MFMA time at TQ=32 is
// 16 B/clk/CU (> the 10.3 B/clk/CU HBM feed), so the sweep is HBM-bound for nq <= 32.
#include "common.h"
#include "knn_stream.h"

#include <float.h>
#include <math.h>
#include <stdlib.h>

namespace {

using namespace acknn;       // the shared streaming core: f32x4, kWaves / kThreads / kGroup / kLdsLimit, Shape, xcd_remap, stream_tiles
using ac::ExactPlan;
using ac::MergeParams;
using ac::fkey;
using ac::fkey_inv;
using ac::next_pow2;

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kPad = 8;                 // extra candidates kept beyond k
constexpr int kMergeMaxCand = 32768;    // G * k' limit (merge kernel keeps 32-bit keys in LDS)

__device__ __attribute__((aligned(16))) float g_knn_zeros[64];     // zero-initialised; tail-group loads of the sweep read it

struct SweepParams {
    const float* P;
    int64_t N;
    int64_t ldP;
    const float* Q;
    int64_t ldQ;
    int D;        // logical dim
    int Dp;       // round_up(D, 4): float4 loads at col < Dp are in bounds (zero padded)
    int ng;       // k-groups per tile: ceil(Dp / (KCOLS * kGroup))
    int nq;
    int kp;       // candidates kept per block and per query (k + pad)
    int cap;      // list capacity, power of two, >= 2 * kp
    int G;        // row groups (blocks per query tile)
    int nqt;      // query tiles
    int64_t ntiles;   // ceil(N / (kWaves * ROWS))
    float* part_d;    // [nqt*TQ][G][kp]
    int32_t* part_i;  // [nqt*TQ][G][kp]
    float* part_maxnorm;  // [G * nqt]
    const float* zeros;   // >= 16 B of zeros, 16-byte aligned (tail-group loads)
    int32_t* clear_ctr;   // [64] the merge / fallback kernels' slot counter and ...
    int32_t* clear_stats; // [4] the caller's d_stats (or NULL): zeroed by workgroup 0 here instead of by two memset launches
};
// FILTERED search (the SEL instantiations take this struct; the plain ones keep SweepParams, so that their kernarg segment -- the
// hidden arguments behind it included -- stays where it was): row r is a candidate iff bit (sel_bit0 + r) of the bitmap is set
// (acamd.h "FILTERED search")
struct SweepParamsSel : SweepParams {
    const uint64_t* sel;
    int64_t sel_bit0;
};
template <bool SEL> struct sweep_params { typedef SweepParams type; };
template <> struct sweep_params<true> { typedef SweepParamsSel type; };

// (sweep_sel_bits, the 16 selection bits of a wave's tile, lives in knn_stream.h: the range sweep fetches them the same way)
// an unselected row's sweep value becomes +inf BEFORE the `acc < tau` test: it is never pushed, so lists, pruning and tau see
// exactly the selected rows
template <int NACC>
__device__ __forceinline__ void sweep_sel_apply(f32x4& acc, uint32_t bits, int lane) {
#pragma unroll
    for (int r = 0; r < NACC; ++r)
        if (!((bits >> Shape::acc_row(r, lane)) & 1u)) acc[r] = INFINITY;
}


// Wave-level prune of one candidate list: keep the kp smallest by (d, id), compacted to the front (in no particular order --
// nothing downstream reads the lists as sorted: the merge radix-selects over all of them); update cnt and tau.  n <= cap <= 512.
// Round 4: a radix SELECT over the monotone keys (32 ballots per register slot) instead of rank-by-counting (n dependent
// LDS broadcast reads: ~3 us for a 112-entry list, most of what a sweep with many resident queries spent outside its k-loop).
template <int MAXPER>
__device__ __forceinline__ void prune_list(float* ld, int32_t* li, int* cnt_p, float* tau_p,
                                           int cap, int kp, int lane) {
    int n = *cnt_p;
    if (n > cap) n = cap;
    if (n <= kp) {                                    // nothing to drop (final prune of a short list)
        if (lane == 0) *cnt_p = n;
        return;
    }
    uint32_t key[MAXPER];
    int32_t myi[MAXPER];
#pragma unroll
    for (int e = 0; e < MAXPER; ++e) {
        const int s = lane + 64 * e;
        const bool v = s < n;
        key[e] = v ? fkey(ld[s]) : 0xffffffffu;       // (a real key is never 0xffffffff: that would be a NaN)
        myi[e] = v ? li[s] : 0x7fffffff;
    }
    // T = the kp-th smallest key: fix its bits from the top; `want` = its rank among the entries that share the bits fixed so far
    uint32_t T = 0;
    int want = kp;
#pragma unroll 1
    for (int bit = 31; bit >= 0; --bit) {
        const uint32_t hi = bit == 31 ? 0u : ~((2u << bit) - 1u);
        int c0 = 0;
#pragma unroll
        for (int e = 0; e < MAXPER; ++e)
            c0 += __builtin_popcountll(__builtin_amdgcn_ballot_w64(key[e] != 0xffffffffu && (key[e] & hi) == T && !((key[e] >> bit) & 1u)));
        if (want > c0) { want -= c0; T |= 1u << bit; }
    }
    // entries below T stay, entries equal to T: the `want` lowest ids of them (ids are unique)
    int c_eq = 0;
#pragma unroll
    for (int e = 0; e < MAXPER; ++e) c_eq += __builtin_popcountll(__builtin_amdgcn_ballot_w64(key[e] == T));
    uint32_t idT = 0xffffffffu;
    if (c_eq > want) {                                // (wave-uniform, rare: several candidates share the boundary value)
        idT = 0;
        int w2 = want;
#pragma unroll 1
        for (int bit = 30; bit >= 0; --bit) {         // ids are non-negative 31-bit numbers
            const uint32_t hi = ~((2u << bit) - 1u);
            int c0 = 0;
#pragma unroll
            for (int e = 0; e < MAXPER; ++e)
                c0 += __builtin_popcountll(__builtin_amdgcn_ballot_w64(key[e] == T && ((uint32_t)myi[e] & hi) == idT && !(((uint32_t)myi[e] >> bit) & 1u)));
            if (w2 > c0) { w2 -= c0; idT |= 1u << bit; }
        }
    }
    // all reads above are complete for the whole wave before any lane writes (the entries sit in registers)
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    int base = 0;
#pragma unroll
    for (int e = 0; e < MAXPER; ++e) {
        const bool keep = key[e] < T || (key[e] == T && (uint32_t)myi[e] <= idT);
        const unsigned long long m = __builtin_amdgcn_ballot_w64(keep);
        if (keep) {
            const int pos = base + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0));
            ld[pos] = fkey_inv(key[e]);
            li[pos] = myi[e];
        }
        base += __builtin_popcountll(m);
    }
    if (lane == 0) { *cnt_p = kp; *tau_p = fkey_inv(T); }
}

__device__ __forceinline__ void prune_dispatch(float* ld, int32_t* li, int* cnt_p, float* tau_p,
                                               int cap, int kp, int lane) {
    if (cap <= 64) prune_list<1>(ld, li, cnt_p, tau_p, cap, kp, lane);
    else if (cap <= 128) prune_list<2>(ld, li, cnt_p, tau_p, cap, kp, lane);
    else if (cap <= 256) prune_list<4>(ld, li, cnt_p, tau_p, cap, kp, lane);
    else prune_list<8>(ld, li, cnt_p, tau_p, cap, kp, lane);
}

// IP = true is the inner-product form (ac_knn_ip_topk): the sweep value is v = -2 (p.q)~ alone.  The query tile is pre-scaled
// by -2 either way, so "smaller is better" still holds and the lists, prune_list and tau are untouched: they order by `<` on
// floats and by fkey, which is monotone over negative values too, and the padding sentinel +inf stays the largest key.  Only the
// |p|^2 fold of the epilogue goes; the running sum of squares stays, because the certificate needs the largest row norm.
// SEL = true is the FILTERED form (ac_knn_*_topk_sel): rows whose selection bit is clear are taken out in the epilogue.
// (Its 16-query form is held to 128 VGPRs -- 4 waves per SIMD, two blocks per CU, the residency the planner sizes the grid for from
// knn_sweep<1>: left at the bound 2 the L2 instantiation took 129.)
template <int J, bool IP = false, bool SEL = false>
__global__ __launch_bounds__(kThreads, (SEL && J == 1) ? 4 : 2) void knn_sweep(typename sweep_params<SEL>::type prm) {
    typedef Shape S;
    typedef S::acc_t acc_t;
    static_assert(J == 1 || J == 2, "query tile = 1 or 2 sub-tiles of 16 (LDS budget; tau[] reload below)");
    constexpr int TQ = 16 * J;
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int nblk = prm.G * prm.nqt;
    const int v = xcd_remap(blockIdx.x, nblk);
    const int qt = v % prm.nqt;
    const int g = v / prm.nqt;
    if (blockIdx.x == 0 && tid < 64) {          // consumed by the kernels launched after this one
        prm.clear_ctr[tid] = 0;
        if (tid < 4 && prm.clear_stats) prm.clear_stats[tid] = 0;
    }

    // ---- LDS carve-up (all offsets multiples of 16) ----
    const int nslots = J * prm.ng * kGroup * 64;      // float4 slots of the query tile
    f32x4* Qs = reinterpret_cast<f32x4*>(smem);
    float* list_d = reinterpret_cast<float*>(smem + (size_t)nslots * 16);
    int32_t* list_i = reinterpret_cast<int32_t*>(list_d + (size_t)TQ * prm.cap);
    int* cnt = reinterpret_cast<int*>(list_i + (size_t)TQ * prm.cap);
    float* tau_s = reinterpret_cast<float*>(cnt + TQ);
    float* wmax_s = tau_s + TQ;                       // [kWaves]

    stage_queries<J>(Qs, prm.Q, prm.ldQ, prm.D, prm.nq, prm.ng, qt, tid);
    for (int t = tid; t < TQ; t += kThreads) {
        cnt[t] = 0;
        tau_s[t] = (qt * TQ + t < prm.nq) ? INFINITY : -INFINITY;
    }
    __syncthreads();

    const int j = lane & 15;            // query column (within each sub-tile) this lane owns in C/D
    float tau[J];
#pragma unroll
    for (int jj = 0; jj < J; ++jj) tau[jj] = tau_s[16 * jj + j];
    float wave_maxnorm = 0.f;

    // per 16-row tile of this wave: fold, selection, list push / prune
    auto epilogue = [&](acc_t (&acc)[J], float nsq, int64_t row_base) {
        // fold |p|^2 in: A = this lane's partial sum of squares, B = 1  (inner product: v = -2 p.q, nothing to fold)
        if constexpr (!IP) {
#pragma unroll
            for (int jj = 0; jj < J; ++jj) acc[jj] = S::mfma(nsq, 1.0f, acc[jj]);
        }
        // row norm for the error-bound certificate
        float rn = nsq;                     // lanes i, i+16, i+32, i+48 hold the 4 k-slices of row i
        rn += __shfl_xor(rn, 16);
        rn += __shfl_xor(rn, 32);
        wave_maxnorm = fmaxf(wave_maxnorm, rn);

        if constexpr (SEL) {
            const uint32_t sbits = sweep_sel_bits(prm.sel, prm.sel_bit0, prm.N, row_base);
#pragma unroll
            for (int jj = 0; jj < J; ++jj) sweep_sel_apply<S::NACC>(acc[jj], sbits, lane);
        }
        bool maybe = false;
#pragma unroll
        for (int jj = 0; jj < J; ++jj)
#pragma unroll
            for (int r = 0; r < S::NACC; ++r) maybe |= (acc[jj][r] < tau[jj]);
        unsigned done = 0;
        bool pend = __any(maybe) != 0;
        for (;;) {
            bool lane_pend = false;
            if (pend) {
#pragma unroll
                for (int jj = 0; jj < J; ++jj) {
                    const int q = 16 * jj + j;
#pragma unroll
                    for (int r = 0; r < S::NACC; ++r) {
                        const int64_t row = row_base + S::acc_row(r, lane);
                        const float d = acc[jj][r];
                        const unsigned bit = 1u << (jj * S::NACC + r);
                        if (!(done & bit) && d < tau[jj] && row < prm.N) {
                            const int slot = atomicAdd(&cnt[q], 1);
                            if (slot < prm.cap) {
                                list_d[q * prm.cap + slot] = d;
                                list_i[q * prm.cap + slot] = (int32_t)row;
                                done |= bit;
                            } else {
                                lane_pend = true;
                            }
                        }
                    }
                }
            }
            // one barrier per tile: decide (uniformly) whether lists must be pruned
            int over = 0;
            if (tid < TQ) over = cnt[tid] > (prm.cap - prm.cap / 4);
            const int need = __syncthreads_or((int)lane_pend | over);
            if (!need) break;
            for (int q = wave; q < TQ; q += kWaves) {
                if (cnt[q] > prm.kp)
                    prune_dispatch(list_d + q * prm.cap, list_i + q * prm.cap, &cnt[q], &tau_s[q],
                                   prm.cap, prm.kp, lane);
            }
            __syncthreads();
            tau[0] = tau_s[j];
            if (J > 1) tau[J - 1] = tau_s[16 * (J - 1) + j];     // J is 1 or 2
            pend = true;   // re-test un-pushed entries against the tightened tau
        }
    };
    stream_tiles<J>(prm.P, prm.N, prm.ldP, prm.Dp, prm.ng, prm.G, g, prm.ntiles, prm.zeros, Qs, lane, wave, epilogue);

    // ---- final: sort + cut every list to kp, write the block's partial result ----
    __syncthreads();
    for (int q = wave; q < TQ; q += kWaves) {
        prune_dispatch(list_d + q * prm.cap, list_i + q * prm.cap, &cnt[q], &tau_s[q], prm.cap,
                       prm.kp, lane);
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        const int n = cnt[q];
        const size_t base = ((size_t)(qt * TQ + q) * prm.G + g) * prm.kp;
        for (int e = lane; e < prm.kp; e += 64) {
            prm.part_d[base + e] = e < n ? list_d[q * prm.cap + e] : INFINITY;
            prm.part_i[base + e] = e < n ? list_i[q * prm.cap + e] : -1;
        }
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) wave_maxnorm = fmaxf(wave_maxnorm, __shfl_xor(wave_maxnorm, o));
    if (lane == 0) wmax_s[wave] = wave_maxnorm;
    __syncthreads();
    if (tid == 0) {
        float m = 0.f;
        for (int w = 0; w < kWaves; ++w) m = fmaxf(m, wmax_s[w]);
        prm.part_maxnorm[v] = m;
    }
}

// --------------------------------------------------------------------------------------
// knn_sweep_ring: the sweep for <= 16 resident queries (the HBM-bound regime the roofline target is stated for), with the
// store rows staged through wave-private LDS rings by whole-line NON-TEMPORAL LDS-DMA and the query tile held in REGISTERS.
//   Why (profiles/r03/hbm_read_ceiling.txt, tools/sweep_ring_bench.hip): plain 16-byte loads stream at <= 6.1 TB/s on an
//   MI355X whatever the occupancy -- knn_sweep<1> sits at that ceiling (6.13 - 6.19) -- while non-temporal accesses reach
//   6.8 - 7.0.  knn_sweep's operand layout (4 lanes per row: 64 bytes of 16 rows per instruction, the other half of every line
//   with the NEXT instruction out of the L1) cannot use them: a non-temporal load does not stay in the L1 (6.13 -> 5.21 TB/s).
//   Here one DMA instruction moves 8 rows x 128 bytes = eight whole lines (8 consecutive lanes per line) into LDS; the
//   fragments are read back in the MFMA layout.  LDS slot of (row a of the 8, 16-byte piece p) = 8 a + (p ^ a): the four
//   k-slices of a row group spread over the banks.  With the rows in LDS the query tile no longer fits there (48 KB at
//   D = 768) -- its B fragments live in registers for the first 512 dimensions (128 VGPRs; all 192 made hipcc spill and reload
//   inside the k-loop) and in 16 KB of LDS for the rest (16 KB at D <= 768, 32 KB at D <= 1024); hence D <= 1024, D % 32 == 0 and <= 16 queries.
//   Per output element the same MFMA sequence in the same k order as knn_sweep<1>; candidate lists, pruning, the row-norm
//   maximum and the partial results are knn_sweep's, unchanged.
// A chunk = 16 rows x 32 floats (2 DMA instructions); RINGC chunks per wave; each wave waits on its OWN DMA queue
// (counted vmcnt), no barrier in the k-loop; the block meets once per 128-row tile in the list-maintenance barrier.
// MAXCH = chunks per row the instantiation is unrolled for: 24 (D <= 768) or 32 (D <= 1024); the query fragments of the first
// ring_reg_chunks() chunks stay in registers (8 VGPRs per chunk), the rest sit in LDS (the longer unrolled loop of the 32-chunk
// form left hipcc 12 bytes short with 16 chunks in registers)
constexpr int ring_reg_chunks(int maxch) { return maxch <= 24 ? 16 : 14; }
constexpr int ring_qs_bytes(int maxch) { return (maxch - ring_reg_chunks(maxch)) * 2 * 64 * 16; }

template <int N> __device__ __forceinline__ void sweep_wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }

// SEL = true: the FILTERED form, as knn_sweep's (the selection word comes through the scalar unit, so the counted vmcnt waits
// of the DMA ring are untouched).
template <int RINGC, int MAXCH, bool IP = false, bool SEL = false>
__global__ __launch_bounds__(kThreads, 2) void knn_sweep_ring(typename sweep_params<SEL>::type prm) {
    constexpr int kRingMaxChunks = MAXCH, kRingRegChunks = ring_reg_chunks(MAXCH), kRingQsBytes = ring_qs_bytes(MAXCH);
    typedef Shape S;
    typedef S::acc_t acc_t;
    constexpr int J = 1, TQ = 16;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    typedef __attribute__((address_space(3))) void lds_void_t;
    typedef const __attribute__((address_space(1))) void glb_void_t;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int v = xcd_remap(blockIdx.x, prm.G);       // (nqt == 1)
    const int g = v;
    if (blockIdx.x == 0 && tid < 64) {          // consumed by the kernels launched after this one
        prm.clear_ctr[tid] = 0;
        if (tid < 4 && prm.clear_stats) prm.clear_stats[tid] = tid == 1 ? 1 : 0;      // [1] = 1: the rows went through the LDS ring
    }
    // ---- LDS: rings [kWaves][RINGC][2 halves][64 lanes] x 16 B | lists | counters ----
    uint4* ring = reinterpret_cast<uint4*>(smem) + (size_t)wave * RINGC * 128;
    f32x4* Qs = reinterpret_cast<f32x4*>(smem + (size_t)kWaves * RINGC * 2048);      // B fragments of chunks >= kRingRegChunks: [kb][lane]
    float* list_d = reinterpret_cast<float*>(smem + (size_t)kWaves * RINGC * 2048 + kRingQsBytes);
    int32_t* list_i = reinterpret_cast<int32_t*>(list_d + (size_t)TQ * prm.cap);
    int* cnt = reinterpret_cast<int*>(list_i + (size_t)TQ * prm.cap);
    float* tau_s = reinterpret_cast<float*>(cnt + TQ);
    float* wmax_s = tau_s + TQ;                       // [kWaves]
    // [2][8] per-tile verdicts of the waves, accessed with relaxed workgroup-scope atomics (= plain ds_read / ds_write).  As
    // `volatile int*` accesses they were FLAT loads -- address-space inference leaves volatile accesses alone -- and a flat load
    // counts on vmcnt too: every tile waited vmcnt(0), i.e. drained the whole DMA ring, for them.
    __shared__ int need_s[2 * 8];
    int bar_parity = 0;
    for (int t = tid; t < TQ; t += kThreads) {
        cnt[t] = 0;
        tau_s[t] = (t < prm.nq) ? INFINITY : -INFINITY;
    }
    const int nch = prm.D >> 5;                       // chunks per row (D % 32 == 0)
    const int j = lane & 15;            // query column this lane owns in C/D and feeds in B
    const int ksub = lane / S::ROWS;    // k sub-slice this lane feeds in the A/B layout
    const int arow = lane % S::ROWS;    // tile row this lane feeds in the A layout
    // ---- the query tile as B fragments: -2 * Q[j][16 kb + 4 ksub ..] ----
    f32x4 bq[2 * kRingRegChunks];
    const bool q_vec = (prm.ldQ & 3) == 0 && (((uintptr_t)prm.Q) & 15) == 0;        // 16-byte aligned query rows
#pragma unroll
    for (int kb = 0; kb < 2 * kRingMaxChunks; ++kb) {
        f32x4 val = {0.f, 0.f, 0.f, 0.f};
        if (kb < 2 * nch && j < prm.nq) {
            const float* src = prm.Q + (size_t)j * prm.ldQ + 16 * kb + 4 * ksub;
            if (q_vec) val = -2.f * *reinterpret_cast<const f32x4*>(src);
            else { val.x = -2.f * src[0]; val.y = -2.f * src[1]; val.z = -2.f * src[2]; val.w = -2.f * src[3]; }
        }
        if (kb < 2 * kRingRegChunks) bq[kb < 2 * kRingRegChunks ? kb : 0] = val;
        else if (wave == 0) Qs[(kb - 2 * kRingRegChunks) * 64 + lane] = val;
    }
    __syncthreads();
    float tau[J];
    tau[0] = tau_s[j];
    float wave_maxnorm = 0.f;

    const int64_t my_tiles = (prm.ntiles > g) ? (prm.ntiles - 1 - g) / prm.G + 1 : 0;
    const int64_t total = my_tiles * nch;             // chunks this wave streams

    // ---- DMA stream of this wave: lane (a = lane / 8, piece = (lane % 8) ^ a) of instruction h copies 16 bytes of row 8 h + a
    const int da = lane >> 3, dp = (lane & 7) ^ da;
    int64_t is_tile = 0;                              // tile / chunk of the next DMA issue
    int is_ch = 0, is_slot = 0;
    const float* rp0;
    const float* rp1;
    auto tile_rows = [&](int64_t it) {
        int64_t r0 = (it * prm.G + g) * (int64_t)(kWaves * S::ROWS) + wave * S::ROWS + da, r1 = r0 + 8;
        if (r0 > prm.N - 1) r0 = prm.N - 1;
        if (r1 > prm.N - 1) r1 = prm.N - 1;
        rp0 = prm.P + (size_t)r0 * prm.ldP + 4 * dp;
        rp1 = prm.P + (size_t)r1 * prm.ldP + 4 * dp;
    };
    tile_rows(0);
    auto issue = [&]() {                              // always two DMA instructions (exact vmcnt accounting); past the end: the last chunk again
        uint4* dst = ring + (size_t)is_slot * 128;
        __builtin_amdgcn_global_load_lds((glb_void_t*)(rp0 + 32 * is_ch), (lds_void_t*)dst, 16, 0, 2);
        __builtin_amdgcn_global_load_lds((glb_void_t*)(rp1 + 32 * is_ch), (lds_void_t*)(dst + 64), 16, 0, 2);
        is_slot = is_slot + 1 == RINGC ? 0 : is_slot + 1;
        if (is_ch + 1 < nch) ++is_ch;
        else if (is_tile + 1 < my_tiles) { is_ch = 0; ++is_tile; tile_rows(is_tile); }
    };

    acc_t acc[J];
    float nsq = 0.f;
    int64_t cur_tile = 0;

    auto epilogue = [&]() {
        // fold |p|^2 in: A = this lane's partial sum of squares, B = 1  (inner product: v = -2 p.q, nothing to fold)
        if constexpr (!IP) acc[0] = S::mfma(nsq, 1.0f, acc[0]);
        // row norm for the error-bound certificate
        float rn = nsq;                     // lanes i, i+16, i+32, i+48 hold the 4 k-slices of row i
        rn += __shfl_xor(rn, 16);
        rn += __shfl_xor(rn, 32);
        wave_maxnorm = fmaxf(wave_maxnorm, rn);

        const int64_t row_base = (cur_tile * prm.G + g) * (int64_t)(kWaves * S::ROWS) + wave * S::ROWS;
        if constexpr (SEL) sweep_sel_apply<S::NACC>(acc[0], sweep_sel_bits(prm.sel, prm.sel_bit0, prm.N, row_base), lane);
        bool maybe = false;
#pragma unroll
        for (int r = 0; r < S::NACC; ++r) maybe |= (acc[0][r] < tau[0]);
        unsigned done = 0;
        bool pend = __any(maybe) != 0;
        for (;;) {
            bool lane_pend = false;
            if (pend) {
                const int q = j;
#pragma unroll
                for (int r = 0; r < S::NACC; ++r) {
                    const int64_t row = row_base + S::acc_row(r, lane);
                    const float d = acc[0][r];
                    const unsigned bit = 1u << r;
                    if (!(done & bit) && d < tau[0] && row < prm.N) {
                        const int slot = atomicAdd(&cnt[q], 1);
                        if (slot < prm.cap) {
                            list_d[q * prm.cap + slot] = d;
                            list_i[q * prm.cap + slot] = (int32_t)row;
                            done |= bit;
                        } else {
                            lane_pend = true;
                        }
                    }
                }
            }
            // one barrier per tile: decide (uniformly) whether lists must be pruned.  NOT __syncthreads_or: its fence waits
            // vmcnt(0), i.e. drains this wave's DMA ring once per 128 rows.  Only LDS traffic has to be ordered here: every
            // wave posts its verdict in a flag word of this tile's parity, waits for its LDS operations, meets the others at
            // a raw s_barrier and reads the eight words (the other parity is rewritten only after the next barrier).
            int over = 0;
            if (tid < TQ) over = cnt[tid] > (prm.cap - prm.cap / 4);
            const int w_need = __any((int)lane_pend | over) != 0;
            const int fl = 8 * (bar_parity & 1);
            if (lane == 0) __hip_atomic_store(&need_s[fl + wave], w_need, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            int need = 0;
#pragma unroll
            for (int w = 0; w < kWaves; ++w) need |= __hip_atomic_load(&need_s[fl + w], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            ++bar_parity;
            if (!need) break;
            for (int q = wave; q < TQ; q += kWaves) {
                if (cnt[q] > prm.kp)
                    prune_dispatch(list_d + q * prm.cap, list_i + q * prm.cap, &cnt[q], &tau_s[q],
                                   prm.cap, prm.kp, lane);
            }
            __syncthreads();
            tau[0] = tau_s[j];
            pend = true;   // re-test un-pushed entries against the tightened tau
        }
        nsq = 0.f;
    };

    if (total > 0) {
#pragma unroll
        for (int i = 0; i < RINGC - 1; ++i) issue();
        const int rh = arow >> 3, ra = arow & 7;
        int slot = 0;
        for (int64_t it = 0; it < my_tiles; ++it) {
            acc[0] = acc_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ch = 0; ch < kRingMaxChunks; ++ch) {               // (unrolled: bq[] is indexed statically)
                if (ch < nch) {                                         // wave-uniform
                    sweep_wait_vm<(RINGC - 2) * 2>();                   // this chunk has landed (the wave's own DMA queue)
                    __builtin_amdgcn_sched_barrier(0);
                    const uint4* sl = ring + (size_t)slot * 128 + rh * 64 + 8 * ra;
                    const f32x4 a0 = __builtin_bit_cast(f32x4, sl[ksub ^ ra]);
                    const f32x4 a1 = __builtin_bit_cast(f32x4, sl[(4 + ksub) ^ ra]);
                    slot = slot + 1 == RINGC ? 0 : slot + 1;
                    issue();                                            // refills the slot the PREVIOUS chunk used (its reads are consumed)
                    f32x4 b0, b1;
                    if (ch < kRingRegChunks) { b0 = bq[ch < kRingRegChunks ? 2 * ch : 0]; b1 = bq[ch < kRingRegChunks ? 2 * ch + 1 : 0]; }
                    else { b0 = Qs[(2 * (ch - kRingRegChunks)) * 64 + lane]; b1 = Qs[(2 * (ch - kRingRegChunks) + 1) * 64 + lane]; }
                    acc[0] = S::mfma(a0.x, b0.x, acc[0]);
                    nsq = fmaf(a0.x, a0.x, nsq); nsq = fmaf(a0.y, a0.y, nsq);
                    acc[0] = S::mfma(a0.y, b0.y, acc[0]);
                    nsq = fmaf(a0.z, a0.z, nsq); nsq = fmaf(a0.w, a0.w, nsq);
                    acc[0] = S::mfma(a0.z, b0.z, acc[0]);
                    acc[0] = S::mfma(a0.w, b0.w, acc[0]);
                    acc[0] = S::mfma(a1.x, b1.x, acc[0]);
                    nsq = fmaf(a1.x, a1.x, nsq); nsq = fmaf(a1.y, a1.y, nsq);
                    acc[0] = S::mfma(a1.y, b1.y, acc[0]);
                    nsq = fmaf(a1.z, a1.z, nsq); nsq = fmaf(a1.w, a1.w, nsq);
                    acc[0] = S::mfma(a1.z, b1.z, acc[0]);
                    acc[0] = S::mfma(a1.w, b1.w, acc[0]);
                }
            }
            epilogue();
            ++cur_tile;
        }
        sweep_wait_vm<0>();                                             // the over-issued tail chunks must land before LDS is released
    }

    // ---- final: sort + cut every list to kp, write the block's partial result ----
    __syncthreads();
    for (int q = wave; q < TQ; q += kWaves) {
        prune_dispatch(list_d + q * prm.cap, list_i + q * prm.cap, &cnt[q], &tau_s[q], prm.cap,
                       prm.kp, lane);
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        const int n = cnt[q];
        const size_t base = ((size_t)q * prm.G + g) * prm.kp;
        for (int e = lane; e < prm.kp; e += 64) {
            prm.part_d[base + e] = e < n ? list_d[q * prm.cap + e] : INFINITY;
            prm.part_i[base + e] = e < n ? list_i[q * prm.cap + e] : -1;
        }
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) wave_maxnorm = fmaxf(wave_maxnorm, __shfl_xor(wave_maxnorm, o));
    if (lane == 0) wmax_s[wave] = wave_maxnorm;
    __syncthreads();
    if (tid == 0) {
        float m = 0.f;
        for (int w = 0; w < kWaves; ++w) m = fmaxf(m, wmax_s[w]);
        prm.part_maxnorm[v] = m;
    }
}

// --------------------------------------------------------------------------------------
// knn_plane_sweep: the HBM-bound sweep over the PREPARED store's fp16 plane for 1 .. 64 resident queries.
//   The fp32 sweeps above stream 4 B per store element; a prepared store (ac_knn_prepare_store) also holds every row as ONE
//   fp16 plane (2 B per element) whose one-product MFMA dot differs from the exact value by a bound E the merge's certificate
//   knows (knn_batch.hip: |v - exact| <= gamma (max|p| + |q|)^2) -- the machinery the batched search uses from 64 queries up.
//   This kernel is its small-batch, bandwidth-bound form: ONE pass over the plane (half the bytes of the fp32 sweep), the query
//   tile of 32 or 64 columns resident in LDS, v_mfma_f32_32x32x16_f16 at ~20 % of the matrix pipe, the candidate lists, pruning
//   and partial results of knn_sweep (exact results come from knn_merge_rerank's fp64 re-rank + certificate, as everywhere).
//   * The plane is tile-major: a 256-row tile is one contiguous run of 256 * Kp * 2 bytes, [k-slot][row % 256][8 fp16] inside.
//     In that layout the MFMA A fragment of (32 rows, 16 k) is two 512-byte runs -- lane (i = lane & 31, kg = lane >> 5) loads
//     the 16 bytes of row i, k-slot 2 s + kg -- i.e. every load instruction consumes whole 128-byte lines, which is what lets
//     it be NON-TEMPORAL straight into registers (knn_sweep's fp32 operand layout takes half a line per instruction and loses
//     with nt loads; knn_sweep_ring goes through LDS for that reason).  No LDS round trip for the rows, no barrier in the k-loop.
//   * A workgroup = 8 waves x 32 rows = one 256-row tile per step, tiles interleaved over the grid (T = it * G + g), one
//     residency round.  Per wave 16 loads (16 KB) in flight: four register buffers of four k-steps, issued unconditionally.
//   * Query B fragments: LDS [k-step][sub-tile][lane] x 16 B, copied from the query plane knn_prepare_queries builds (same
//     scaling and rounding as the batched path, so the same bound).  Sweep value v = |p|^2 + f_q acc; |p|^2 comes from the
//     prepared norms through SCALAR loads (constant address space: off the vmcnt queue the prefetched rows sit in).
//   * The block meets once per tile at a raw s_barrier to decide about pruning (as knn_sweep_ring does).
// --------------------------------------------------------------------------------------
struct PlaneSweepParams {
    const uint16_t* Pp;       // store plane, tile-major (knn_batch.hip knn_plane_kernel)
    const float* pnorm;       // [round_up(N, 256)] |p|^2, +inf past N
    const uint16_t* Qp;       // query plane [Kp/8][q_rows][8]
    int64_t q_rows;
    const float* qfac;        // [q_rows] -2 2^(e_p + e_q)
    int64_t N;
    int64_t ntiles;           // ceil(N / 256)
    int Kp;                   // multiple of 64
    int q0, nq;               // this launch's query tile: queries q0 .. q0 + nq - 1 (nq <= TQ)
    int kp, cap, G;
    float* part_d;            // [query][G][kp]
    int32_t* part_i;
    int32_t* clear_ctr;       // as SweepParams (first tile's launch only; else NULL)
    int32_t* clear_stats;
};

// FILTERED search over the plane (ac_knn_*_topk_batch_sel, <= 64 queries): the SEL instantiations take this struct, the plain ones
// keep PlaneSweepParams and their kernarg segment (as SweepParamsSel above)
struct PlaneSweepParamsSel : PlaneSweepParams {
    const uint64_t* sel;
    int64_t sel_bit0;
};
template <bool SEL> struct plane_sweep_params { typedef PlaneSweepParams type; };
template <> struct plane_sweep_params<true> { typedef PlaneSweepParamsSel type; };

// The 32 selection bits of a wave's rows row_base .. row_base + 31 (bit i = row row_base + i): sweep_sel_bits for the plane sweep's
// wave tile -- two 64-bit words at most, through the scalar unit, the second one only if one of its rows exists.
__device__ __forceinline__ uint32_t plane_sel_bits(const uint64_t* sel, int64_t sel_bit0, int64_t N, int row_base) {
    if (row_base >= N) return 0u;
    typedef const uint64_t __attribute__((address_space(4)))* cup;
    const uint32_t rem = __builtin_amdgcn_readfirstlane((uint32_t)(sel_bit0 & 63) + (uint32_t)row_base);     // (N < 2^31)
    const cup w = (cup)(uintptr_t)(sel + (sel_bit0 >> 6) + (rem >> 6));
    const int s = (int)(rem & 63u);
    uint64_t bits = w[0] >> s;
    if (s > 32 && row_base + (64 - s) < N) bits |= w[1] << (64 - s);
    return (uint32_t)bits;
}

typedef _Float16 kf16x8 __attribute__((ext_vector_type(8)));
typedef uint32_t ku32x4 __attribute__((ext_vector_type(4)));
// C/D layout of v_mfma_f32_32x32x16_f16: lane owns column (lane & 31) and these 16 rows
__device__ __forceinline__ int plane_acc_row(int r, int lane) { return (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5); }

// IP (the last parameter): the inner-product proposal v = f_q acc ~ -2 p.q.  No norm is loaded; the rows past N, which the L2
// form keeps out through the +inf padding of the norms, are bound-checked here (a zero plane row gives v = 0: the best value
// of all when every product is negative).
// SEL (after IP): the FILTERED form.  An unselected row's value becomes +inf -- through the norm term, like a row past N -- before it
// meets tau or a list, so the per-workgroup lists, pruning and tau see exactly the selected rows (knn_sweep's rule).
template <int TQ, bool IP = false, bool SEL = false>
__global__ __launch_bounds__(kThreads, 2) void knn_plane_sweep(typename plane_sweep_params<SEL>::type prm) {
    constexpr int NJ = TQ / 32;                       // 32-column sub-tiles of the query tile
    constexpr int NB = 4, GK = 4;                     // register buffers x k-steps per buffer (16 loads in flight)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i32 = lane & 31, kg = lane >> 5;
    const int g = xcd_remap(blockIdx.x, prm.G);
    if (blockIdx.x == 0 && tid < 64 && prm.clear_ctr) {            // consumed by the kernels launched after this one
        prm.clear_ctr[tid] = 0;
        if (tid < 4 && prm.clear_stats) prm.clear_stats[tid] = tid == 1 ? 2 : 0;     // [1] = 2: the fp16-plane sweep ran
    }
    const int nk = prm.Kp >> 4;                       // 16-k MFMA steps per row
    const int ngrp = nk / GK;                         // (Kp % 64 == 0)
    // ---- LDS: query fragments [nk][NJ][64] x 16 B | lists | counters ----
    ku32x4* Qs = reinterpret_cast<ku32x4*>(smem);
    float* list_d = reinterpret_cast<float*>(smem + (size_t)nk * NJ * 1024);
    int32_t* list_i = reinterpret_cast<int32_t*>(list_d + (size_t)TQ * prm.cap);
    int* cnt = reinterpret_cast<int*>(list_i + (size_t)TQ * prm.cap);
    float* tau_s = reinterpret_cast<float*>(cnt + TQ);
    __shared__ int need_s[2 * 8];                                  // [2][8] per-tile verdicts of the waves (static LDS: see knn_sweep_ring)
    for (int t = tid; t < nk * NJ * 64; t += kThreads) {
        const int l = t & 63, jj = (t >> 6) % NJ, s = (t >> 6) / NJ;
        const int64_t qrow = prm.q0 + 32 * jj + (l & 31);          // (< q_rows: the plane is padded to 256 queries with zeros)
        Qs[t] = *reinterpret_cast<const ku32x4*>(prm.Qp + ((int64_t)(2 * s + (l >> 5)) * prm.q_rows + qrow) * 8);
    }
    for (int t = tid; t < TQ; t += kThreads) {
        cnt[t] = 0;
        tau_s[t] = (t < prm.nq) ? INFINITY : -INFINITY;
    }
    __syncthreads();
    float tau[NJ], qf[NJ];
#pragma unroll
    for (int jj = 0; jj < NJ; ++jj) { tau[jj] = tau_s[32 * jj + i32]; qf[jj] = prm.qfac[prm.q0 + 32 * jj + i32]; }
    int bar_parity = 0;

    const int64_t my_tiles = (prm.ntiles > g) ? (prm.ntiles - 1 - g) / prm.G + 1 : 0;
    const int64_t total = my_tiles * ngrp;            // groups of GK k-steps this wave consumes
    const size_t tile_bytes = (size_t)prm.Kp * 512;   // 256 rows x Kp x 2 B
    const uint32_t lane_off = (uint32_t)(kg * 256 + 32 * wave + i32) * 16u;    // byte offset of this lane's piece inside a k-slot pair
    // prefetch state: next group to load
    int64_t pf_tile = 0;
    int pf_grp = 0;
    auto tile_base = [&](int64_t it) -> const char* {
        int64_t T = it * prm.G + g;
        if (T > prm.ntiles - 1) T = prm.ntiles - 1;    // past the end: the last tile again (never consumed)
        return reinterpret_cast<const char*>(prm.Pp) + (size_t)T * tile_bytes;
    };
    const char* pf_base = tile_base(0);
    ku32x4 buf[NB][GK];
#define AC_PL_PREFETCH(B)                                                                                     \
    do {                                                                                                      \
        const char* src_ = pf_base + (size_t)pf_grp * (GK * 8192) + lane_off;                                 \
        _Pragma("unroll") for (int u = 0; u < GK; ++u)                                                        \
            buf[B][u] = __builtin_nontemporal_load(reinterpret_cast<const ku32x4*>(src_ + u * 8192));          \
        if (++pf_grp == ngrp) { pf_grp = 0; ++pf_tile; pf_base = tile_base(pf_tile); }                        \
    } while (0)

    f32x16 acc[NJ];
    int64_t cur_tile = 0;
    int cur_grp = 0;

    auto epilogue = [&]() {
        const int row0 = (int)((cur_tile * prm.G + g) * 256) + 32 * wave;      // wave-uniform, multiple of 32 (N < 2^31)
        // |p|^2 of the wave's 32 rows through the scalar unit: lane half kg needs rows (r & 3) + 8 (r >> 2) + 4 kg
        typedef const float __attribute__((address_space(4)))* cfp;
        const cfp pn = (cfp)(uintptr_t)(prm.pnorm + __builtin_amdgcn_readfirstlane(row0));
        bool maybe = false;
        const int left = (int)prm.N - row0 - 4 * kg;                           // (IP) rows (r & 3) + 8 (r >> 2) below it exist
        uint32_t sbits = 0u;                                                   // (SEL) this lane's rows: bit (r & 3) + 8 (r >> 2)
        if constexpr (SEL) sbits = plane_sel_bits(prm.sel, prm.sel_bit0, prm.N, row0) >> (4 * kg);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            float pnr;
            if constexpr (IP) {
                pnr = (r & 3) + 8 * (r >> 2) < left ? 0.f : INFINITY;
            } else {
                const float lo = pn[(r & 3) + 8 * (r >> 2)], hi = pn[(r & 3) + 8 * (r >> 2) + 4];
                pnr = kg ? hi : lo;
            }
            if constexpr (SEL) { if (!((sbits >> ((r & 3) + 8 * (r >> 2))) & 1u)) pnr = INFINITY; }
#pragma unroll
            for (int jj = 0; jj < NJ; ++jj) {
                acc[jj][r] = fmaf(acc[jj][r], qf[jj], pnr);                    // the sweep value, in place
                maybe |= acc[jj][r] < tau[jj];
            }
        }
        unsigned done = 0;
        bool pend = __any(maybe) != 0;
        for (;;) {
            bool lane_pend = false;
            if (pend) {
#pragma unroll
                for (int jj = 0; jj < NJ; ++jj) {
                    const int q = 32 * jj + i32;
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const float d = acc[jj][r];
                        const unsigned bit = 1u << (16 * jj + r);
                        if (!(done & bit) && d < tau[jj]) {                    // (rows past N carry +inf: never below tau)
                            const int slot = atomicAdd(&cnt[q], 1);
                            if (slot < prm.cap) {
                                list_d[q * prm.cap + slot] = d;
                                list_i[q * prm.cap + slot] = row0 + plane_acc_row(r, lane);
                                done |= bit;
                            } else {
                                lane_pend = true;
                            }
                        }
                    }
                }
            }
            // one RAW barrier per tile (knn_sweep_ring: __syncthreads_or would fence vmcnt(0) and drain the prefetched rows)
            int over = 0;
            if (tid < TQ) over = cnt[tid] > (prm.cap - prm.cap / 4);
            const int w_need = __any((int)lane_pend | over) != 0;
            const int fl = 8 * (bar_parity & 1);
            if (lane == 0) __hip_atomic_store(&need_s[fl + wave], w_need, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            int need = 0;
#pragma unroll
            for (int w = 0; w < kWaves; ++w) need |= __hip_atomic_load(&need_s[fl + w], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            ++bar_parity;
            if (!need) break;
            for (int q = wave; q < TQ; q += kWaves) {
                if (cnt[q] > prm.kp)
                    prune_dispatch(list_d + q * prm.cap, list_i + q * prm.cap, &cnt[q], &tau_s[q], prm.cap, prm.kp, lane);
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
#pragma unroll
            for (int jj = 0; jj < NJ; ++jj) tau[jj] = tau_s[32 * jj + i32];
            pend = true;                                  // re-test un-pushed entries against the tightened tau
        }
    };

#define AC_PL_COMPUTE(B)                                                                                      \
    do {                                                                                                      \
        if (cur_grp == 0) {                                                                                   \
            _Pragma("unroll") for (int jj = 0; jj < NJ; ++jj)                                                 \
                _Pragma("unroll") for (int r = 0; r < 16; ++r) acc[jj][r] = 0.f;                              \
        }                                                                                                     \
        const ku32x4* qsrc_ = Qs + (size_t)cur_grp * (GK * NJ * 64) + lane;                                    \
        ku32x4 bq_[NJ];                                                                                        \
        _Pragma("unroll") for (int jj = 0; jj < NJ; ++jj) bq_[jj] = qsrc_[jj * 64];                           \
        _Pragma("unroll") for (int u = 0; u < GK; ++u) {                                                      \
            const kf16x8 a_ = __builtin_bit_cast(kf16x8, buf[B][u]);                                          \
            kf16x8 b_[NJ];                                                                                    \
            _Pragma("unroll") for (int jj = 0; jj < NJ; ++jj) b_[jj] = __builtin_bit_cast(kf16x8, bq_[jj]);   \
            if (u + 1 < GK) { /* LDS reads one step ahead */                                                  \
                _Pragma("unroll") for (int jj = 0; jj < NJ; ++jj) bq_[jj] = qsrc_[((u + 1) * NJ + jj) * 64];  \
            }                                                                                                 \
            _Pragma("unroll") for (int jj = 0; jj < NJ; ++jj)                                                 \
                acc[jj] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_, b_[jj], acc[jj], 0, 0, 0);               \
            __builtin_amdgcn_sched_barrier(0); /* keep the per-load consume order */                          \
        }                                                                                                     \
        if (++cur_grp == ngrp) { epilogue(); cur_grp = 0; ++cur_tile; }                                       \
    } while (0)

    // Loads are issued unconditionally (past the end they re-read the last tile) so that every path has the same number of
    // loads in flight: a load inside a branch makes hipcc's s_waitcnt accounting wait on the buffer it has just issued.
    if (total > 0) {
        AC_PL_PREFETCH(0);
        AC_PL_PREFETCH(1);
        AC_PL_PREFETCH(2);
        for (int64_t gg = 0; gg < total; gg += NB) {      // (ngrp may be odd: the tile boundary falls anywhere in this body)
            AC_PL_PREFETCH(3);
            AC_PL_COMPUTE(0);
            AC_PL_PREFETCH(0);
            if (gg + 1 < total) AC_PL_COMPUTE(1);
            AC_PL_PREFETCH(1);
            if (gg + 2 < total) AC_PL_COMPUTE(2);
            AC_PL_PREFETCH(2);
            if (gg + 3 < total) AC_PL_COMPUTE(3);
        }
    }
#undef AC_PL_PREFETCH
#undef AC_PL_COMPUTE

    // ---- final: sort + cut every list to kp, write the block's partial result ----
    __syncthreads();
    for (int q = wave; q < TQ; q += kWaves) {
        if (q >= prm.nq) continue;
        prune_dispatch(list_d + q * prm.cap, list_i + q * prm.cap, &cnt[q], &tau_s[q], prm.cap, prm.kp, lane);
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        const int n = cnt[q];
        const size_t base = ((size_t)(prm.q0 + q) * prm.G + g) * prm.kp;
        for (int e = lane; e < prm.kp; e += 64) {
            prm.part_d[base + e] = e < n ? list_d[q * prm.cap + e] : INFINITY;
            prm.part_i[base + e] = e < n ? list_i[q * prm.cap + e] : -1;
        }
    }
}

// ---- host-side planning ----
struct Plan {
    bool small;          // knn_small_exact instead of the fused sweep
    int small_pow2;
    int TQ, kp, cap, ng, Dp, G, nqt;
    int ring;            // 0, or the chunks per wave of knn_sweep_ring (<= 16 queries, D % 32 == 0, D <= 768)
    int64_t ntiles;
    size_t sweep_lds;
    size_t off_part_d, off_part_i, off_maxnorm, off_zeros, total;
    ExactPlan ex;
};

// AC_KNN_G (tuning experiments): the sweep grid's row groups; each planner applies its own clamp.  0 = not set
static int64_t env_knn_g() { const char* e = getenv("AC_KNN_G"); const int64_t v = e ? atoll(e) : 0; return v >= 1 ? v : 0; }

// LDS behind the query tile of knn_sweep / knn_sweep_ring: the lists (value + id), cnt[], tau[], the waves' row-norm maxima
static size_t sweep_list_bytes(int TQ, int cap) { return (size_t)TQ * cap * 8 + TQ * 8 + kWaves * 4 + 64; }

static int make_plan(int64_t N, int D, int nq, int k, Plan* pl) {
    *pl = Plan{};
    ac::KnnSweepShape sh;
    const int rc = ac::knn_sweep_shape(N, D, nq, k, &sh);
    if (rc != AC_OK) return rc;
    pl->Dp = sh.Dp; pl->ng = sh.ng; pl->kp = sh.kp; pl->cap = sh.cap;
    if (sh.small) {
        pl->small = true;
        pl->small_pow2 = next_pow2((int)(N > 2 ? N : 2));
        pl->TQ = 16; pl->G = 1; pl->nqt = 1;
        pl->total = 256;
        return AC_OK;
    }
    int TQ = nq > 16 ? 32 : 16;
    for (;;) {
        pl->sweep_lds = ac::knn_query_tile_bytes(TQ, pl->ng) + sweep_list_bytes(TQ, pl->cap);
        if (pl->sweep_lds <= (size_t)kLdsLimit) break;
        AC_REQUIRE(TQ == 32, AC_EUNSUPPORTED,
                   "knn: D=%d with k=%d needs %zu B of LDS (> %d); unsupported", D, k, pl->sweep_lds, kLdsLimit);
        TQ = 16;
    }
    pl->TQ = TQ;
    pl->nqt = nq > 0 ? (nq + TQ - 1) / TQ : 1;
    const int rows_per_tile = kWaves * 16;
    pl->ntiles = (N + rows_per_tile - 1) / rows_per_tile;
    const ac::DevInfo& di = ac::dev_info();
    // <= 16 queries, D a multiple of 32 up to 768: the LDS-ring form (rows by non-temporal DMA, queries in registers)
    static const int ring_env = getenv("AC_KNN_RING") ? atoi(getenv("AC_KNN_RING")) : -1;      // 0 = never (A/B)
    if (TQ == 16 && pl->nqt == 1 && (D % 32) == 0 && D <= 1024 && ring_env != 0) {
        const size_t lists = ring_qs_bytes(D <= 768 ? 24 : 32) + sweep_list_bytes(TQ, pl->cap) + 64;
        // (tools/sweep_ring_bench.hip: 4 chunks per wave stream as fast as 8)
        pl->ring = (size_t)kWaves * 4 * 2048 + lists <= (size_t)kLdsLimit ? 4 : 0;
        if (pl->ring) pl->sweep_lds = (size_t)kWaves * pl->ring * 2048 + lists;
    }
    // One block per CU for the ring form (8 waves at the 256-register budget fill a CU) and for the 32-query tile: this plan also
    // launches the FILTERED knn_sweep<2, *, true>, which needs more than 128 VGPRs, i.e. one block per CU whatever the plain form
    // takes.  Only the 16-query tile, whose every instantiation is held to 128 VGPRs, asks the occupancy query.
    const bool one_per_cu = pl->ring || TQ == 32;
    int64_t G = ac::knn_residency_groups(one_per_cu ? nullptr : (const void*)knn_sweep<1>, pl->sweep_lds, pl->nqt, pl->ntiles);
    if (G > kMergeMaxCand / pl->kp) {
        G = kMergeMaxCand / pl->kp;
        if (pl->nqt == 1 && G > di.cus) G = G / di.cus * di.cus;
    }
    if (const int64_t v = env_knn_g()) G = v;
    if (G > pl->ntiles) G = pl->ntiles;
    if (G > kMergeMaxCand / pl->kp) G = kMergeMaxCand / pl->kp;
    if (G < 1) G = 1;
    pl->G = (int)G;
    const size_t nqpad = (size_t)pl->nqt * TQ;
    const size_t ncand = nqpad * pl->G * pl->kp;
    ac::WsTake take;
    pl->off_part_d = take(ncand * 4);
    pl->off_part_i = take(ncand * 4);
    pl->off_maxnorm = take((size_t)pl->G * pl->nqt * 4);
    pl->ex.off_flags = take((size_t)(nq > 0 ? nq : 1) * 4);
    pl->off_zeros = take(256);
    ac::knn_exact_plan(&pl->ex, take, k, pl->kp, pl->Dp, ac::align_up((size_t)pl->G * pl->kp * 4, 16), nq < 64 ? (nq > 0 ? nq : 1) : 64);
    pl->total = take.off;
    return AC_OK;
}

thread_local hipEvent_t g_prof_start = nullptr, g_prof_stop = nullptr;

}  // namespace

// ---- the planner rule and host helpers every fp32 row-stream sweep shares (common.h) ----
namespace ac {

int knn_sweep_shape(int64_t N, int D, int nq, int k, KnnSweepShape* s) {
    AC_REQUIRE(N >= 0 && N < 2147483647LL, AC_EINVAL, "knn: N=%lld out of range", (long long)N);
    AC_REQUIRE(D >= 1 && nq >= 0 && k >= 1, AC_EINVAL, "knn: bad D=%d nq=%d k=%d", D, nq, k);
    *s = KnnSweepShape{};
    s->Dp = (D + 3) / 4 * 4;
    s->kp = k + kPad;
    s->cap = next_pow2(2 * s->kp);
    if (s->cap < 64) s->cap = 64;
    s->ng = (s->Dp + Shape::KCOLS * kGroup - 1) / (Shape::KCOLS * kGroup);
    // does the fused sweep cover (D, k)?  LDS: one 16-query tile + its candidate lists
    const size_t lds16 = knn_query_tile_bytes(16, s->ng) + sweep_list_bytes(16, s->cap);
    if (k > AC_KNN_MAX_K || lds16 > (size_t)kLdsLimit) {
        AC_REQUIRE(N <= kKnnSmallN, AC_EUNSUPPORTED,
                   "knn: k=%d, D=%d is outside the fused sweep (k <= %d, query tile + lists <= %d B of LDS) and "
                   "N=%lld exceeds the small-store path (N <= %d)", k, D, AC_KNN_MAX_K, kLdsLimit, (long long)N,
                   kKnnSmallN);
        s->small = true;
    }
    return AC_OK;
}

size_t knn_query_tile_bytes(int TQ, int ng) { return (size_t)(TQ / 16) * ng * kGroup * 64 * 16; }

// 1.01 n 2^-24, n = 128 ng + 16 roundings per term of stream_tiles' fp32 fma chain (acamd.h "exactness contract")
double knn_sweep_gamma0(int ng) { return 1.01 * (double)(ng * kGroup * 16 + 16) * 5.9604644775390625e-08; }

// blocks that are actually co-resident on a CU (VGPR/LDS limited); the grid is sized to exactly
// one residency round so that no CU idles in a second, partial round
int64_t knn_residency_groups(const void* kernel, size_t lds, int nqt, int64_t ntiles) {
    int per_cu = 1;
    if (kernel && hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, kThreads, lds) != hipSuccess) { (void)hipGetLastError(); per_cu = 1; }
    if (per_cu < 1) per_cu = 1;
    if (per_cu > 2) per_cu = 2;
    int64_t G = ((int64_t)dev_info().cus * per_cu) / nqt;
    if (G < 1) G = 1;
    if (G > ntiles) G = ntiles;       // (an empty store: 0; its callers launch nothing, or clamp to 1 for the workspace layout)
    return G;
}

const float* knn_zeros_device() {             // a zero-initialised __device__ array: no memset launch per call (the symbol has one address per device)
    static const float* cache[64] = {nullptr};
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (dev < 0 || dev >= 64) dev = 0;
    if (!cache[dev]) { void* q = nullptr; (void)hipGetSymbolAddress(&q, HIP_SYMBOL(g_knn_zeros)); cache[dev] = (const float*)q; }
    return cache[dev];
}

int knn_check_store(const char* who, const float* d_P, int64_t ldP, int Dp) {
    AC_REQUIRE(d_P != nullptr, AC_EINVAL, "%s: d_P is NULL", who);
    AC_REQUIRE(ldP >= Dp && (ldP % 4) == 0, AC_EINVAL, "%s: ldP=%lld must be a multiple of 4 and >= round_up(D,4)=%d", who, (long long)ldP, Dp);
    AC_REQUIRE((((uintptr_t)d_P) & 15) == 0, AC_EINVAL, "%s: d_P must be 16-byte aligned", who);
    return AC_OK;
}

}  // namespace ac

extern "C" int ac_knn_set_profile_events(void* start_event, void* stop_event) {
    g_prof_start = (hipEvent_t)start_event;
    g_prof_stop = (hipEvent_t)stop_event;
    return AC_OK;
}

extern "C" int ac_knn_l2_topk_workspace(int64_t N, int D, int nq, int k, size_t* bytes) {
    AC_REQUIRE(bytes != nullptr, AC_EINVAL, "knn workspace: bytes is NULL");
    Plan pl;
    int rc = make_plan(N, D, nq, k, &pl);
    if (rc != AC_OK) return rc;
    *bytes = pl.total;
    return AC_OK;
}

extern "C" int ac_knn_l2_topk(const float* d_P, int64_t N, int64_t ldP, int D, const float* d_Q,
                              int nq, int64_t ldQ, int k, int64_t row_offset, float* d_outD,
                              int64_t* d_outI, void* d_ws, size_t ws_bytes, int32_t* d_stats,
                              ac_stream_t stream_) {
    return ac_knn_l2_topk_x(d_P, N, ldP, D, d_Q, nq, ldQ, k, row_offset, d_outD, nullptr, d_outI, d_ws, ws_bytes,
                            d_stats, stream_);
}

// the fp32-sweep search of both metrics: ip = false squared L2 (ac_knn_l2_topk_x), true inner product (ac_knn_ip_topk_x).  One
// plan, one workspace layout and one launch sequence; the metric only picks the instantiation of each kernel.
// d_sel != NULL: the FILTERED search (ac_knn_*_topk_sel) -- the same plan, workspace and launch sequence with the SEL
// instantiation of the sweep and of the exact stages.
static int knn_topk(bool ip, const float* d_P, int64_t N, int64_t ldP, int D, const float* d_Q,
                    int nq, int64_t ldQ, int k, int64_t row_offset, float* d_outD, double* d_outD64,
                    int64_t* d_outI, void* d_ws, size_t ws_bytes, int32_t* d_stats, ac_stream_t stream_,
                    const uint64_t* d_sel = nullptr, int64_t sel_bit0 = 0) {
    hipStream_t stream = (hipStream_t)stream_;
    Plan pl;
    int rc = make_plan(N, D, nq, k, &pl);
    if (rc != AC_OK) return rc;
    if (nq == 0) return AC_OK;
    AC_REQUIRE(d_Q && d_outD && d_outI, AC_EINVAL, "knn: null pointer");
    AC_REQUIRE(ldQ >= D, AC_EINVAL, "knn: ldQ=%lld < D=%d", (long long)ldQ, D);
    AC_REQUIRE(ws_bytes >= pl.total && (d_ws || pl.total == 0), AC_EWORKSPACE,
               "knn: workspace %zu < required %zu", ws_bytes, pl.total);
    if (N > 0 && (rc = ac::knn_check_store("knn", d_P, ldP, pl.Dp)) != AC_OK) return rc;
    char* ws = (char*)d_ws;
    ac::SelArgs sa;
    sa.sel = d_sel; sa.sel_bit0 = sel_bit0;
    if (d_stats && (pl.small || N == 0)) AC_HIP_CHECK(hipMemsetAsync(d_stats, 0, 4 * sizeof(int32_t), stream));
    if (pl.small) {
        MergeParams sp;
        sp.P = d_P; sp.N = N; sp.ldP = ldP; sp.Q = d_Q; sp.ldQ = ldQ; sp.D = D; sp.k = k; sp.row_offset = row_offset;
        sp.outD = d_outD; sp.outD64 = d_outD64; sp.outI = d_outI;
        return ac::knn_small_exact_launch(ip, sp, nq, pl.small_pow2, stream, d_sel ? &sa : nullptr);
    }

    MergeParams mp = ac::knn_merge_params(d_P, N, ldP, d_Q, ldQ, D, pl.Dp, k, pl.kp, row_offset, d_outD, d_outD64, d_outI, d_stats, ws, pl.ex);
    mp.G = pl.G; mp.nblk = pl.G * pl.nqt;
    mp.gamma = ac::knn_sweep_gamma0(pl.ng);
    mp.part_d = (const float*)(ws + pl.off_part_d);
    mp.part_i = (const int32_t*)(ws + pl.off_part_i);
    mp.part_maxnorm = (const float*)(ws + pl.off_maxnorm);

    if (N == 0) {
        // empty shard: everything is padding; reuse the merge kernel with all-padding partials
        AC_HIP_CHECK(hipMemsetAsync(ws + pl.ex.off_fb_ctr, 0, 256, stream));      // (otherwise the sweep's workgroup 0 clears it)
        AC_HIP_CHECK(hipMemsetAsync(ws + pl.off_part_i, 0xff, (size_t)pl.nqt * pl.TQ * pl.G * pl.kp * 4, stream));
        AC_HIP_CHECK(hipMemsetAsync(ws + pl.off_maxnorm, 0, (size_t)pl.G * pl.nqt * 4, stream));
    } else {
        SweepParamsSel sp{};                          // (the plain kernels take its SweepParams base)
        sp.P = d_P; sp.N = N; sp.ldP = ldP; sp.Q = d_Q; sp.ldQ = ldQ; sp.D = D; sp.Dp = pl.Dp;
        sp.ng = pl.ng; sp.nq = nq; sp.kp = pl.kp; sp.cap = pl.cap; sp.G = pl.G; sp.nqt = pl.nqt;
        sp.ntiles = pl.ntiles;
        sp.part_d = (float*)(ws + pl.off_part_d);
        sp.part_i = (int32_t*)(ws + pl.off_part_i);
        sp.part_maxnorm = (float*)(ws + pl.off_maxnorm);
        sp.zeros = ac::knn_zeros_device();
        sp.clear_ctr = (int32_t*)(ws + pl.ex.off_fb_ctr);
        sp.clear_stats = d_stats;
        sp.sel = d_sel; sp.sel_bit0 = sel_bit0;
        const int nblk = pl.G * pl.nqt;
        if (g_prof_start && g_prof_stop) AC_HIP_CHECK(hipEventRecord(g_prof_start, stream));
        void (*sweep_fn)(SweepParams) = nullptr;
        void (*sweep_sel_fn)(SweepParamsSel) = nullptr;      // FILTERED search: the SEL instantiation of the same sweep
        if (pl.ring) {
            if (d_sel) {
                if (D <= 768) sweep_sel_fn = ip ? knn_sweep_ring<4, 24, true, true> : knn_sweep_ring<4, 24, false, true>;
                else sweep_sel_fn = ip ? knn_sweep_ring<4, 32, true, true> : knn_sweep_ring<4, 32, false, true>;
            } else if (D <= 768) sweep_fn = ip ? knn_sweep_ring<4, 24, true> : knn_sweep_ring<4, 24, false>;
            else sweep_fn = ip ? knn_sweep_ring<4, 32, true> : knn_sweep_ring<4, 32, false>;
            AC_HIP_CHECK(hipFuncSetAttribute(d_sel ? (const void*)sweep_sel_fn : (const void*)sweep_fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pl.sweep_lds));
        } else {
            if (d_sel) {
                if (pl.TQ == 32) sweep_sel_fn = ip ? knn_sweep<2, true, true> : knn_sweep<2, false, true>;
                else sweep_sel_fn = ip ? knn_sweep<1, true, true> : knn_sweep<1, false, true>;
            } else if (pl.TQ == 32) sweep_fn = ip ? knn_sweep<2, true> : knn_sweep<2, false>;
            else sweep_fn = ip ? knn_sweep<1, true> : knn_sweep<1, false>;
            (void)hipFuncSetAttribute(d_sel ? (const void*)sweep_sel_fn : (const void*)sweep_fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pl.sweep_lds);
        }
        if (d_sel) {
            hipLaunchKernelGGL(sweep_sel_fn, dim3(nblk), dim3(kThreads), pl.sweep_lds, stream, sp);
        } else {
            const SweepParams base = sp;
            hipLaunchKernelGGL(sweep_fn, dim3(nblk), dim3(kThreads), pl.sweep_lds, stream, base);
        }
        AC_LAUNCH_CHECK();
        if (g_prof_start && g_prof_stop) AC_HIP_CHECK(hipEventRecord(g_prof_stop, stream));
    }
    return ac::knn_exact_tail(ip, mp, pl.ex, nq, pl.ex.merge_lds, stream, d_sel && N > 0 ? &sa : nullptr);
}

extern "C" int ac_knn_l2_topk_x(const float* d_P, int64_t N, int64_t ldP, int D, const float* d_Q,
                                int nq, int64_t ldQ, int k, int64_t row_offset, float* d_outD, double* d_outD64,
                                int64_t* d_outI, void* d_ws, size_t ws_bytes, int32_t* d_stats,
                                ac_stream_t stream_) {
    return knn_topk(false, d_P, N, ldP, D, d_Q, nq, ldQ, k, row_offset, d_outD, d_outD64, d_outI, d_ws, ws_bytes, d_stats, stream_);
}

// inner product (faiss.IndexFlatIP.search): the plan, and hence the workspace, is the L2 search's
extern "C" int ac_knn_ip_topk_workspace(int64_t N, int D, int nq, int k, size_t* bytes) {
    return ac_knn_l2_topk_workspace(N, D, nq, k, bytes);
}

extern "C" int ac_knn_ip_topk(const float* d_P, int64_t N, int64_t ldP, int D, const float* d_Q,
                              int nq, int64_t ldQ, int k, int64_t row_offset, float* d_outD,
                              int64_t* d_outI, void* d_ws, size_t ws_bytes, int32_t* d_stats,
                              ac_stream_t stream_) {
    return knn_topk(true, d_P, N, ldP, D, d_Q, nq, ldQ, k, row_offset, d_outD, nullptr, d_outI, d_ws, ws_bytes, d_stats, stream_);
}

extern "C" int ac_knn_ip_topk_x(const float* d_P, int64_t N, int64_t ldP, int D, const float* d_Q,
                                int nq, int64_t ldQ, int k, int64_t row_offset, float* d_outD, double* d_outD64,
                                int64_t* d_outI, void* d_ws, size_t ws_bytes, int32_t* d_stats,
                                ac_stream_t stream_) {
    return knn_topk(true, d_P, N, ldP, D, d_Q, nq, ldQ, k, row_offset, d_outD, d_outD64, d_outI, d_ws, ws_bytes, d_stats, stream_);
}

// FILTERED search (acamd.h "FILTERED search"): the k best rows AMONG the selected ones.  The argument checks return before any
// HIP call; the search itself is knn_topk with the selection (same plan, same workspace as ac_knn_l2_topk_workspace).
static int knn_topk_sel(bool ip, const float* d_P, int64_t N, int64_t ldP, int D, const float* d_Q, int nq, int64_t ldQ, int k,
                        int64_t row_offset, const uint64_t* d_sel, int64_t sel_bit0, float* d_outD, double* d_outD64,
                        int64_t* d_outI, void* d_ws, size_t ws_bytes, int32_t* d_stats, ac_stream_t stream_) {
    AC_REQUIRE(sel_bit0 >= 0, AC_EINVAL, "knn sel: sel_bit0=%lld must be >= 0", (long long)sel_bit0);
    AC_REQUIRE(d_sel != nullptr || N <= 0, AC_EINVAL, "knn sel: d_sel is NULL");
    AC_REQUIRE((((uintptr_t)d_sel) & 7) == 0, AC_EINVAL, "knn sel: d_sel must be 8-byte aligned");
    return knn_topk(ip, d_P, N, ldP, D, d_Q, nq, ldQ, k, row_offset, d_outD, d_outD64, d_outI, d_ws, ws_bytes, d_stats, stream_,
                    N > 0 ? d_sel : nullptr, sel_bit0);
}

extern "C" int ac_knn_l2_topk_sel(const float* d_P, int64_t N, int64_t ldP, int D, const float* d_Q, int nq, int64_t ldQ, int k,
                                  int64_t row_offset, const uint64_t* d_sel, int64_t sel_bit0, float* d_outD, double* d_outD64,
                                  int64_t* d_outI, void* d_ws, size_t ws_bytes, int32_t* d_stats, ac_stream_t stream_) {
    return knn_topk_sel(false, d_P, N, ldP, D, d_Q, nq, ldQ, k, row_offset, d_sel, sel_bit0, d_outD, d_outD64, d_outI, d_ws, ws_bytes,
                        d_stats, stream_);
}

extern "C" int ac_knn_ip_topk_sel(const float* d_P, int64_t N, int64_t ldP, int D, const float* d_Q, int nq, int64_t ldQ, int k,
                                  int64_t row_offset, const uint64_t* d_sel, int64_t sel_bit0, float* d_outD, double* d_outD64,
                                  int64_t* d_outI, void* d_ws, size_t ws_bytes, int32_t* d_stats, ac_stream_t stream_) {
    return knn_topk_sel(true, d_P, N, ldP, D, d_Q, nq, ldQ, k, row_offset, d_sel, sel_bit0, d_outD, d_outD64, d_outI, d_ws, ws_bytes,
                        d_stats, stream_);
}

// Id-list route: the k best among M listed rows (sorted, unique ids), for sparse selections -- the small-store sort with one
// indirection, exact by construction, no workspace.
static int knn_topk_ids(bool ip, const float* d_P, int64_t N, int64_t ldP, int D, const int64_t* d_ids, int64_t M, const float* d_Q,
                        int nq, int64_t ldQ, int k, int64_t row_offset, float* d_outD, double* d_outD64, int64_t* d_outI,
                        ac_stream_t stream_) {
    AC_REQUIRE(M >= 0 && M <= ac::kKnnSmallN, AC_EINVAL, "knn ids: M=%lld outside [0, %d]", (long long)M, ac::kKnnSmallN);
    AC_REQUIRE(d_ids != nullptr || M == 0, AC_EINVAL, "knn ids: d_ids is NULL");
    AC_REQUIRE(N >= 0 && N < 2147483647LL, AC_EINVAL, "knn ids: N=%lld out of range", (long long)N);
    AC_REQUIRE(D >= 1 && nq >= 0 && k >= 1, AC_EINVAL, "knn ids: bad D=%d nq=%d k=%d", D, nq, k);
    if (nq == 0) return AC_OK;
    AC_REQUIRE(d_Q && d_outD && d_outI, AC_EINVAL, "knn ids: null pointer");
    AC_REQUIRE(ldQ >= D && ldP >= D, AC_EINVAL, "knn ids: ldQ=%lld / ldP=%lld < D=%d", (long long)ldQ, (long long)ldP, D);
    AC_REQUIRE(d_P != nullptr || N == 0 || M == 0, AC_EINVAL, "knn ids: d_P is NULL");
    MergeParams sp;
    sp.P = d_P; sp.N = N; sp.ldP = ldP; sp.Q = d_Q; sp.ldQ = ldQ; sp.D = D; sp.k = k; sp.row_offset = row_offset;
    sp.outD = d_outD; sp.outD64 = d_outD64; sp.outI = d_outI;
    ac::SelArgs sa;
    sa.ids = d_ids; sa.n_ids = M; sa.by_ids = 1;
    return ac::knn_small_exact_launch(ip, sp, nq, next_pow2((int)(M > 2 ? M : 2)), (hipStream_t)stream_, &sa);
}

extern "C" int ac_knn_l2_topk_ids(const float* d_P, int64_t N, int64_t ldP, int D, const int64_t* d_ids, int64_t M, const float* d_Q,
                                  int nq, int64_t ldQ, int k, int64_t row_offset, float* d_outD, double* d_outD64, int64_t* d_outI,
                                  ac_stream_t stream_) {
    return knn_topk_ids(false, d_P, N, ldP, D, d_ids, M, d_Q, nq, ldQ, k, row_offset, d_outD, d_outD64, d_outI, stream_);
}

extern "C" int ac_knn_ip_topk_ids(const float* d_P, int64_t N, int64_t ldP, int D, const int64_t* d_ids, int64_t M, const float* d_Q,
                                  int nq, int64_t ldQ, int k, int64_t row_offset, float* d_outD, double* d_outD64, int64_t* d_outI,
                                  ac_stream_t stream_) {
    return knn_topk_ids(true, d_P, N, ldP, D, d_ids, M, d_Q, nq, ldQ, k, row_offset, d_outD, d_outD64, d_outI, stream_);
}

// ---------------------------------------------------------------------------------------------------------
// batched search with a prepared store (fp16 plane + row norms): sample -> thresholds -> GEMM-form filter ->
// the same merge / fp64 re-rank / certificate / exact fallback (knn_exact.hip; knn_batch.hip explains the scheme)
// ---------------------------------------------------------------------------------------------------------
namespace {

constexpr int kBatchPad = 24;            // k' = k + 24 candidates re-ranked per query (the certificate's slack)
constexpr int kBatchMaxK = 100;
constexpr int64_t kBatchMinRows = 65536;

constexpr int kTwoPhaseCtlInts = 512;       // >= sizeof(acp::GridCtl) / 4
struct BatchPlan {
    int kp, cap, Dp;
    int64_t stride, stride_a, S, q_rows;
    int segs;
    size_t off_sD32, off_sD64, off_sI, off_thr, off_qfac, off_cnt, off_ctl, off_wgmin, off_qp, off_cd, off_ci, off_sub, sub_bytes, total;
    ExactPlan ex;
};

int make_batch_plan(int64_t N, int D, int nq, int k, BatchPlan* bp) {
    AC_REQUIRE(N >= kBatchMinRows && N < 2147483647LL, AC_EUNSUPPORTED, "knn batch: N=%lld outside [%lld, 2^31)", (long long)N,
               (long long)kBatchMinRows);
    AC_REQUIRE(D >= 1 && nq >= 1 && k >= 1 && k <= kBatchMaxK, AC_EUNSUPPORTED, "knn batch: D=%d nq=%d k=%d unsupported (k <= %d)",
               D, nq, k, kBatchMaxK);
    bp->kp = k + kBatchPad;
    bp->Dp = (D + 3) / 4 * 4;
    // Thresholds come from strided SAMPLES of the store swept by the same GEMM-form kernel (knn_batch.hip) and re-ranked exactly
    // by the merge kernel: tau_q = the largest exact distance among the k' sample rows with the smallest sweep values -- k' rows
    // of the store within tau_q, so the store's k'-th smallest distance is <= tau_q whatever the sweep's rounding did.
    //   stage A: every `stride_a`-th row (max(4096, 128 k') rows), no threshold yet: every lane offers the best of its 32 rows per query;
    //   stage B (stores beyond ~0.5 M rows): every `stride`-th row filtered by stage A's tau (k' stride_a / stride expected);
    //   main:    all rows filtered by the last tau: k' * stride candidates expected, at most half the candidate buffer.
    // (Round 2 searched ONE sample of N / 64 rows exactly with the fp32 sweep: 10 ms at 4096 x 10M, 0.17 ms of the 0.39 ms a
    //  256 x 100k call takes.)
    int64_t smax = 8192 / bp->kp;
    if (smax > 128) smax = 128;
    if (smax < 1) smax = 1;
    // stage A offers one row per 32 sample rows and query (the best of each lane's rows): with >= 4 k' offers the k' best of them
    // are, up to rare collisions, the sample's k' best, so tau_A is as tight as an exact search of the sample would make it
    const int64_t rows_a = 128 * (int64_t)bp->kp > 4096 ? 128 * (int64_t)bp->kp : 4096;
    int64_t stride_a = (N + rows_a - 1) / rows_a, stride = stride_a;
    if (stride > smax) {                               // stage B's (or, for small stores, stage A's own) stride
        // Stage B keeps the sample rows within tau_A and needs k' of them: k' S_B / S_A are expected, so its sample must be a few
        // times stage A's.  (Round 3 used smax whatever stride_a was: at 0.92 - 1.5 M rows -- stride_a just above smax, e.g. a
        // 10M-row store sharded 8 ways -- that is k' x 1.1 .. 1.4 expected candidates, a good share of the queries came out of
        // stage B with fewer than k', lost their threshold, overflowed their candidate buffer in the main sweep and took the
        // exact fallback: 1.3 s instead of 8 ms per 4096-query batch at 1M rows.)
        stride = smax;
        if (stride > stride_a / 3) stride = stride_a / 3;
        if (stride < 1) stride = 1;
    }
    bp->stride_a = stride_a;
    bp->stride = stride;
    bp->S = ac::knn_sample_rows(N, stride_a);            // rows of the stage-A sample
    const int64_t expect = (int64_t)bp->kp * stride;             // E[candidates per query] of the main sweep = k' * stride
    int cap = 1024;
    while (cap < 2 * expect && cap < 16384) cap <<= 1;
    // Short launches (a sample stage, or the whole sweep of a small store) fire all their appends in one burst, and the
    // device-scope atomics that reserve the slots serialise per address (~0.1 - 0.5 us each: 84 of the 140 us of a 256 x 100k
    // sweep with one counter per query).  Such launches split a query's list into up to 64 segments with a counter each
    // (>= 256 entries per segment: a segment overflows no more easily than the whole list would); long launches keep ONE list
    // -- their workgroups drift apart, and a single hot counter line per query is then the cheaper form (10M x 768 x 4096: 68.8 ms
    // against 75.8 with 16 segments).  batch_segs() picks per launch.
    const int segs_want = nq <= 256 ? 64 : (nq <= 1024 ? 32 : 16);
    if (cap < 256 * segs_want) cap = 256 * segs_want;
    bp->cap = cap;
    bp->segs = cap / 256 < segs_want ? cap / 256 : segs_want;          // the most any launch of this call uses
    bp->q_rows = ((int64_t)nq + 255) / 256 * 256;
    const size_t sub = 256;                                // (the exact sample search of round 2 needed a workspace of its own)
    bp->sub_bytes = sub;
    ac::WsTake take;
    bp->off_sD32 = take((size_t)nq * bp->kp * 4);
    bp->off_sD64 = take((size_t)nq * bp->kp * 8);
    bp->off_sI = take((size_t)nq * bp->kp * 8);
    bp->off_thr = take((size_t)bp->q_rows * 4);
    bp->off_qfac = take((size_t)bp->q_rows * 4);
    bp->off_cnt = take((size_t)bp->q_rows * 4 * bp->segs);
    bp->off_ctl = take(kTwoPhaseCtlInts * 4);             // (right behind the counters: zeroed by the same launch) grid-barrier words
    bp->off_wgmin = take(ac::knn_batch_two_phase_bytes());   // two-phase thresholds (knn_batch.hip): per-workgroup minima
    bp->off_qp = take(ac::knn_planes_bytes(nq, D));
    bp->off_cd = take((size_t)bp->q_rows * cap * 4);
    bp->off_ci = take((size_t)bp->q_rows * cap * 4);
    bp->ex.off_flags = take((size_t)nq * 4);
    // (the merge's LDS in its segmented form: keys + ids; one segment needs cap * 4 less)
    ac::knn_exact_plan(&bp->ex, take, k, bp->kp, bp->Dp, 2 * ac::align_up((size_t)cap * 4, 16), nq < 64 ? nq : 64);
    bp->off_sub = take(sub);
    bp->total = take.off;
    return AC_OK;
}


// ---- the fp16-plane sweep for small batches (knn_plane_sweep): 1 .. kPlaneMaxQueries queries against a prepared store ----
constexpr int kPlaneMaxQueries = 64;

struct PlanePlan {
    int TQ, nqt, kp, cap, G, Dp, Kp;
    int64_t ntiles, q_rows;
    size_t sweep_lds;
    size_t off_part_d, off_part_i, off_qp, off_qfac, off_thr, total;
    ExactPlan ex;
};

// false: the shape does not fit (LDS) or the form is switched off -- the caller uses the GEMM-form path instead
bool make_plane_plan(int64_t N, int D, int nq, int k, PlanePlan* pp) {
    static const int plane_env = getenv("AC_KNN_PLANE") ? atoi(getenv("AC_KNN_PLANE")) : -1;       // 0 = never (A/B)
    if (plane_env == 0 || nq < 1 || nq > kPlaneMaxQueries || N < 1 || N >= 2147483647LL - 512 || k < 1 || k > kBatchMaxK) return false;
    pp->kp = k + kBatchPad;
    pp->Dp = (D + 3) / 4 * 4;
    pp->Kp = (D + 63) / 64 * 64;
    const int nk = pp->Kp / 16;
    auto lds_for = [&](int TQ, int cap) {
        return (size_t)nk * (TQ / 32) * 1024 + (size_t)TQ * cap * 8 + (size_t)TQ * 8 + 2 * 8 * 4 + 64;
    };
    const int cap_full = (2 * pp->kp + 15) / 16 * 16, cap_min = (pp->kp + 32 + 15) / 16 * 16;
    const int tq_first = nq > 32 ? 64 : 32;
    pp->TQ = 0;
    for (int TQ = tq_first; TQ >= 32 && !pp->TQ; TQ -= 32)
        for (int cap = cap_full; cap >= cap_min; cap -= 16)
            if (lds_for(TQ, cap) <= (size_t)kLdsLimit) { pp->TQ = TQ; pp->cap = cap; break; }
    if (!pp->TQ || pp->cap > 512) return false;
    pp->sweep_lds = lds_for(pp->TQ, pp->cap);
    pp->nqt = (nq + pp->TQ - 1) / pp->TQ;
    pp->ntiles = (N + 255) / 256;
    int64_t G = ac::dev_info().cus;                       // one 8-wave workgroup per CU: exactly one residency round
    if (G > pp->ntiles) G = pp->ntiles;
    if (G > kMergeMaxCand / pp->kp) G = kMergeMaxCand / pp->kp;
    if (const int64_t v = env_knn_g()) { if (v <= G) G = v; }
    pp->G = (int)G;
    pp->q_rows = 256;
    ac::WsTake take;
    const size_t ncand = (size_t)pp->nqt * pp->TQ * pp->G * pp->kp;
    pp->off_part_d = take(ncand * 4);
    pp->off_part_i = take(ncand * 4);
    pp->ex.off_flags = take((size_t)nq * 4);
    pp->off_qp = take(ac::knn_planes_bytes(nq, D));
    pp->off_qfac = take((size_t)pp->q_rows * 4);
    pp->off_thr = take((size_t)pp->q_rows * 4);
    ac::knn_exact_plan(&pp->ex, take, k, pp->kp, pp->Dp, ac::align_up((size_t)pp->G * pp->kp * 4, 16), nq);
    pp->total = take.off;
    return true;
}

int plane_search(bool ip, const PlanePlan& pp, const float* d_P, int64_t N, int64_t ldP, int D, const uint16_t* d_planes, const float* d_norms,
                 const float* d_Q, int nq, int64_t ldQ, int k, int64_t row_offset, float* d_outD, double* d_outD64, int64_t* d_outI,
                 char* ws, int32_t* d_stats, hipStream_t stream, const ac::SelArgs* sel = nullptr) {
    const int64_t np = (N + 255) / 256 * 256;
    const uint32_t* d_maxnorm = reinterpret_cast<const uint32_t*>(d_norms + np);
    const double gamma = ac::knn_batch_gamma(D);
    // 1. the queries' fp16 plane (each scaled by its own power of two) and epilogue factors -2 2^(e_p + e_q): the same kernel,
    //    scaling and rounding as the GEMM-form path, hence the same error bound
    int rc = ac::knn_prepare_queries(nullptr, pp.kp, d_Q, ldQ, D, nq, d_maxnorm, gamma, (uint16_t*)(ws + pp.off_qp),
                                     (float*)(ws + pp.off_thr), (float*)(ws + pp.off_qfac), stream);
    if (rc != AC_OK) return rc;
    // 2. one pass over the plane per query tile
    PlaneSweepParamsSel sp{};                         // (the plain kernels take its PlaneSweepParams base)
    if (sel) { sp.sel = sel->sel; sp.sel_bit0 = sel->sel_bit0; }
    sp.Pp = d_planes; sp.pnorm = d_norms; sp.Qp = (const uint16_t*)(ws + pp.off_qp); sp.q_rows = pp.q_rows;
    sp.qfac = (const float*)(ws + pp.off_qfac); sp.N = N; sp.ntiles = pp.ntiles; sp.Kp = pp.Kp;
    sp.kp = pp.kp; sp.cap = pp.cap; sp.G = pp.G;
    sp.part_d = (float*)(ws + pp.off_part_d); sp.part_i = (int32_t*)(ws + pp.off_part_i);
    if (g_prof_start && g_prof_stop) AC_HIP_CHECK(hipEventRecord(g_prof_start, stream));
    for (int qt = 0; qt < pp.nqt; ++qt) {
        sp.q0 = qt * pp.TQ; sp.nq = nq - sp.q0 < pp.TQ ? nq - sp.q0 : pp.TQ;
        sp.clear_ctr = qt == 0 ? (int32_t*)(ws + pp.ex.off_fb_ctr) : nullptr;
        sp.clear_stats = qt == 0 ? d_stats : nullptr;
        if (sel) {                                    // FILTERED search: the SEL instantiation of the same sweep
            void (*sweep_sel_fn)(PlaneSweepParamsSel);
            if (pp.TQ == 64) sweep_sel_fn = ip ? knn_plane_sweep<64, true, true> : knn_plane_sweep<64, false, true>;
            else sweep_sel_fn = ip ? knn_plane_sweep<32, true, true> : knn_plane_sweep<32, false, true>;
            AC_HIP_CHECK(hipFuncSetAttribute((const void*)sweep_sel_fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pp.sweep_lds));
            hipLaunchKernelGGL(sweep_sel_fn, dim3(pp.G), dim3(kThreads), pp.sweep_lds, stream, sp);
        } else {
            void (*sweep_fn)(PlaneSweepParams);
            if (pp.TQ == 64) sweep_fn = ip ? knn_plane_sweep<64, true> : knn_plane_sweep<64, false>;
            else sweep_fn = ip ? knn_plane_sweep<32, true> : knn_plane_sweep<32, false>;
            AC_HIP_CHECK(hipFuncSetAttribute((const void*)sweep_fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pp.sweep_lds));
            const PlaneSweepParams base = sp;
            hipLaunchKernelGGL(sweep_fn, dim3(pp.G), dim3(kThreads), pp.sweep_lds, stream, base);
        }
        AC_LAUNCH_CHECK();
    }
    if (g_prof_start && g_prof_stop) AC_HIP_CHECK(hipEventRecord(g_prof_stop, stream));
    // 3. merge of the G per-workgroup lists + exact fp64 re-rank + certificate with the fp16 bound, then the exact fallback
    MergeParams mp = ac::knn_merge_params(d_P, N, ldP, d_Q, ldQ, D, pp.Dp, k, pp.kp, row_offset, d_outD, d_outD64, d_outI, d_stats, ws, pp.ex);
    mp.G = pp.G; mp.nblk = 1; mp.gamma = gamma;
    mp.part_d = (const float*)(ws + pp.off_part_d); mp.part_i = (const int32_t*)(ws + pp.off_part_i);
    mp.part_maxnorm = reinterpret_cast<const float*>(d_maxnorm);
    // (FILTERED: knn_merge_rerank_sel's per-block rule -- fewer than k' = k + 24 real entries in total => complete -- and the
    //  fallback over the selected rows)
    return ac::knn_exact_tail(ip, mp, pp.ex, nq, pp.ex.merge_lds, stream, sel);
}

}  // namespace

extern "C" int ac_knn_store_bytes(int64_t N, int D, size_t* planes_bytes, size_t* norms_bytes) {
    AC_REQUIRE(planes_bytes && norms_bytes && N >= 0 && D >= 1, AC_EINVAL, "knn_store_bytes: bad arguments");
    *planes_bytes = ac::knn_planes_bytes(N, D);
    *norms_bytes = (size_t)((N + 255) / 256 * 256 + 64) * sizeof(float);      // |p|^2 per row, +inf tile padding, the maximum at [round_up(N, 256)]
    return AC_OK;
}

extern "C" int ac_knn_prepare_store(const float* d_P, int64_t N, int64_t ldP, int D, uint16_t* d_planes, float* d_norms,
                                    ac_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    AC_REQUIRE(d_P && d_planes && d_norms && N >= 1 && D >= 1 && ldP >= D, AC_EINVAL, "knn_prepare_store: bad arguments");
    AC_REQUIRE((((uintptr_t)d_planes) & 15) == 0 && (((uintptr_t)d_norms) & 15) == 0, AC_EINVAL,
               "knn_prepare_store: planes / norms must be 16-byte aligned");
    const int64_t np = (N + 255) / 256 * 256;
    AC_HIP_CHECK(hipMemsetAsync(d_norms + np, 0, 64 * sizeof(float), stream));          // [np] = max |p|^2 (float bits)
    return ac::knn_prepare_store(d_P, ldP, N, D, d_planes, d_norms, reinterpret_cast<uint32_t*>(d_norms + np), stream);
}

extern "C" int ac_knn_update_store(const float* d_P, int64_t N_old, int64_t N_new, int64_t ldP, int D, uint16_t* d_planes,
                                   float* d_norms, int64_t row0, int64_t nrows, int32_t* d_exponent_changed, ac_stream_t stream_) {
    AC_REQUIRE(d_P && d_planes && d_norms && d_exponent_changed && D >= 1 && ldP >= D, AC_EINVAL, "knn_update_store: bad arguments");
    AC_REQUIRE(N_old >= 1 && N_new >= N_old && row0 >= 0 && nrows >= 1 && row0 + nrows <= N_new, AC_EINVAL,
               "knn_update_store: rows [%lld, %lld) outside a store of %lld rows (was %lld)", (long long)row0, (long long)(row0 + nrows),
               (long long)N_new, (long long)N_old);
    AC_REQUIRE(N_new == N_old || (row0 + nrows == N_new && row0 <= N_old), AC_EINVAL,
               "knn_update_store: an append must cover every new row: [row0, row0 + nrows) = [<= N_old, N_new)");
    return ac::knn_update_store(d_P, ldP, N_old, N_new, D, d_planes, d_norms, row0, nrows, d_exponent_changed, (hipStream_t)stream_);
}

extern "C" int ac_knn_l2_topk_batch_workspace(int64_t N, int D, int nq, int k, size_t* bytes) {
    AC_REQUIRE(bytes != nullptr, AC_EINVAL, "knn batch workspace: bytes is NULL");
    BatchPlan bp;
    int rc = make_batch_plan(N, D, nq, k, &bp);
    if (rc != AC_OK) return rc;
    *bytes = bp.total;
    PlanePlan pp;                                       // small batches take the fp16-plane sweep (knn_plane_sweep)
    if (make_plane_plan(N, D, nq, k, &pp) && pp.total > *bytes) *bytes = pp.total;
    return AC_OK;
}

// segments of a query's candidate list for a launch that sweeps `rows` rows (see make_batch_plan)
static int batch_segs(const BatchPlan& bp, int64_t rows, int nq) {
    const int64_t tiles = ((rows + 255) / 256) * (((int64_t)nq + 255) / 256);
    const int64_t per_wg = (tiles + ac::dev_info().cus - 1) / ac::dev_info().cus;
    return per_wg <= 8 ? bp.segs : 1;
}

// the prepared-store search of both metrics: ip = false squared L2 (ac_knn_l2_topk_batch), true inner product
// (ac_knn_ip_topk_batch).  One plan, one workspace layout, one launch sequence over the SAME prepared store; the metric only
// picks the instantiation of the sweeps and of the exact stages.
static int knn_topk_batch(bool ip, const float* d_P, int64_t N, int64_t ldP, int D, const uint16_t* d_planes,
                          const float* d_norms, const float* d_Q, int nq, int64_t ldQ, int k, int64_t row_offset,
                          float* d_outD, double* d_outD64, int64_t* d_outI, void* d_ws, size_t ws_bytes,
                          int32_t* d_stats, ac_stream_t stream_, const uint64_t* d_sel = nullptr, int64_t sel_bit0 = 0) {
    hipStream_t stream = (hipStream_t)stream_;
    BatchPlan bp;
    int rc = make_batch_plan(N, D, nq, k, &bp);
    if (rc != AC_OK) return rc;
    // d_sel != NULL: the FILTERED search (ac_knn_*_topk_batch_sel) -- the same plan, workspace and launch sequence with the SEL
    // instantiations of the sweeps and of the exact stages
    ac::SelArgs sa;
    sa.sel = d_sel; sa.sel_bit0 = sel_bit0;
    const ac::SelArgs* const sel = d_sel ? &sa : nullptr;
    AC_REQUIRE(d_P && d_planes && d_norms && d_Q && d_outD && d_outI, AC_EINVAL, "knn batch: null pointer");
    AC_REQUIRE(ldQ >= D && ldP >= bp.Dp && (ldP % 4) == 0 && (((uintptr_t)d_P) & 15) == 0, AC_EINVAL, "knn batch: bad leading dimension / alignment");
    AC_REQUIRE(d_ws && ws_bytes >= bp.total, AC_EWORKSPACE, "knn batch: workspace %zu < required %zu", ws_bytes, bp.total);
    char* ws = (char*)d_ws;
    {   // <= 64 queries: bandwidth-bound, ONE pass over the fp16 plane with the query tile resident (knn_plane_sweep)
        PlanePlan pp;
        if (make_plane_plan(N, D, nq, k, &pp)) {
            AC_REQUIRE(ws_bytes >= pp.total, AC_EWORKSPACE, "knn batch: workspace %zu < required %zu", ws_bytes, pp.total);
            return plane_search(ip, pp, d_P, N, ldP, D, d_planes, d_norms, d_Q, nq, ldQ, k, row_offset, d_outD, d_outD64, d_outI, ws,
                                d_stats, stream, sel);
        }
    }
    const int64_t np = (N + 255) / 256 * 256;
    const uint32_t* d_maxnorm = reinterpret_cast<const uint32_t*>(d_norms + np);
    // |v - exact| <= gamma (max|p| + |q|)^2 for the one-product fp16 sweep (knn_batch.hip; derivation at the declaration of
    // this entry point in include/acamd.h)
    const double gamma = ac::knn_batch_gamma(D);

    // 1. per query: epilogue factor -2 2^(e_p + e_q), fp16 plane of q 2^-e_q, threshold +inf (keep everything)
    //    (the same launch zeroes the candidate counters of every segmentation this call uses: no memset launches below)
    rc = ac::knn_prepare_queries(nullptr, bp.kp, d_Q, ldQ, D, nq, d_maxnorm, gamma,
                                 (uint16_t*)(ws + bp.off_qp), (float*)(ws + bp.off_thr), (float*)(ws + bp.off_qfac), stream,
                                 (int32_t*)(ws + bp.off_cnt), (int64_t)bp.q_rows * bp.segs + kTwoPhaseCtlInts);
    if (rc != AC_OK) return rc;
    // 2. threshold stages: sweep a strided sample, re-rank its k' best exactly (knn_merge_rerank in candidate mode, asked for
    //    k' results; its certificate is irrelevant here -- ANY k' rows bound the k'-th smallest distance from above)
    //    (N = the stage's sample rows and run_stride are set per stage; no fallback slots: fb_F = 0, a counter word of its own)
    MergeParams sp = ac::knn_merge_params(d_P, 0, ldP, d_Q, ldQ, D, bp.Dp, bp.kp, bp.kp, 0, (float*)(ws + bp.off_sD32), (double*)(ws + bp.off_sD64),
                                          (int64_t*)(ws + bp.off_sI), nullptr, ws, bp.ex);
    sp.G = 1; sp.nblk = 1; sp.gamma = gamma;
    sp.cand_cnt = (const int32_t*)(ws + bp.off_cnt); sp.cand_cap = bp.cap;
    // a threshold stage's merge writes the new threshold itself and zeroes the counters it has read (the next sweep appends
    // into them): round 3 spent a knn_thr_kernel launch and a memset launch per stage on that
    sp.cand_cnt_clear = (int32_t*)(ws + bp.off_cnt); sp.thr_out = (float*)(ws + bp.off_thr);
    sp.part_d = (const float*)(ws + bp.off_cd); sp.part_i = (const int32_t*)(ws + bp.off_ci);
    sp.part_maxnorm = reinterpret_cast<const float*>(d_maxnorm);
    sp.fb_F = 0; sp.fb_d = nullptr; sp.fb_i = nullptr; sp.fb_slotctr += 8;
    static const bool thr_exact = [] { const char* e = getenv("AC_KNN_THR_EXACT"); return e && atoi(e) != 0; }();     // (A/B: the re-ranked form)
    sp.thr_only = thr_exact ? 0 : 1;
    static const bool dbg = getenv("AC_KNN_BATCH_DEBUG") != nullptr;
    const int64_t stage_stride[2] = {bp.stride_a, bp.stride};
    // the main sweep takes its thresholds from its own first tile round where it can (knn_batch.hip two_phase): no sample stages
    const bool two_phase = ac::knn_batch_two_phase_applies(N, nq, bp.kp, batch_segs(bp, N, nq));
    const int nstages = two_phase ? 0 : (bp.stride_a > bp.stride ? 2 : 1);
    for (int st = 0; st < nstages; ++st) {
        const int64_t sst = stage_stride[st];
        const int segs = batch_segs(bp, ac::knn_sample_rows(N, sst), nq);
        const size_t mlds = bp.ex.merge_lds - (segs > 1 ? 0 : ac::align_up((size_t)bp.cap * 4, 16));
        sp.cand_segs = segs;
        rc = ac::knn_batch_launch(ip, d_planes, d_norms, N, D, (const uint16_t*)(ws + bp.off_qp), nq, (const float*)(ws + bp.off_thr),
                                  (const float*)(ws + bp.off_qfac), (float*)(ws + bp.off_cd), (int32_t*)(ws + bp.off_ci),
                                  (int32_t*)(ws + bp.off_cnt), bp.cap, segs, sst, st == 0 ? 1 : 0, stream, nullptr, nullptr, 0, nullptr, nullptr, sel);
        if (rc != AC_OK) return rc;
        sp.N = ac::knn_sample_rows(N, sst); sp.run_stride = sst > 1 ? 8 * sst : 0;   // sample row i = store row (i >> 3) * 8 sst + (i & 7)
        rc = ac::knn_merge_launch(ip, sp, nq, st == 0 ? bp.ex.merge_lds : 0, mlds, stream);      // (the opt-in covers the later stages)
        if (rc != AC_OK) return rc;
        if (dbg) {
            AC_HIP_CHECK(hipStreamSynchronize(stream));
            int32_t cnt[4]; float thr[4]; double tau[4];
            AC_HIP_CHECK(hipMemcpy(cnt, ws + bp.off_cnt, sizeof(cnt), hipMemcpyDeviceToHost));
            AC_HIP_CHECK(hipMemcpy(thr, ws + bp.off_thr, sizeof(thr), hipMemcpyDeviceToHost));
            for (int i = 0; i < 4; ++i)
                AC_HIP_CHECK(hipMemcpy(&tau[i], ws + bp.off_sD64 + ((size_t)(i < nq ? i : 0) * bp.kp + bp.kp - 1) * 8, 8, hipMemcpyDeviceToHost));
            fprintf(stderr, "knn batch stage %d: stride %lld rows %lld cap %d kp %d | cand %d %d %d %d | tau %g %g %g %g | thr %g %g %g %g\n", st,
                    (long long)sst, (long long)sp.N, bp.cap, bp.kp, cnt[0], cnt[1], cnt[2], cnt[3], tau[0], tau[1], tau[2], tau[3], thr[0], thr[1], thr[2], thr[3]);
        }
    }
    const int msegs = batch_segs(bp, N, nq);
    const size_t mlds = bp.ex.merge_lds - (msegs > 1 ? 0 : ac::align_up((size_t)bp.cap * 4, 16));
    // 3. the GEMM-form sweep: candidates (row, v) with v below the query's threshold (its workgroup 0 also zeroes the caller's
    //    d_stats and the fallback's slot counter, which the merge after it increments)
    if (g_prof_start && g_prof_stop) AC_HIP_CHECK(hipEventRecord(g_prof_start, stream));
    rc = ac::knn_batch_launch(ip, d_planes, d_norms, N, D, (const uint16_t*)(ws + bp.off_qp), nq, (const float*)(ws + bp.off_thr),
                              (const float*)(ws + bp.off_qfac), (float*)(ws + bp.off_cd), (int32_t*)(ws + bp.off_ci), (int32_t*)(ws + bp.off_cnt), bp.cap, msegs, 1, 0, stream,
                              (int32_t*)(ws + bp.ex.off_fb_ctr), d_stats, two_phase ? bp.kp : 0, (unsigned*)(ws + bp.off_wgmin), ws + bp.off_ctl, sel);
    if (rc != AC_OK) return rc;
    if (g_prof_start && g_prof_stop) AC_HIP_CHECK(hipEventRecord(g_prof_stop, stream));
    // 4. merge + exact re-rank + certificate, then the exact fallback for uncertified queries
    MergeParams mp = ac::knn_merge_params(d_P, N, ldP, d_Q, ldQ, D, bp.Dp, k, bp.kp, row_offset, d_outD, d_outD64, d_outI, d_stats, ws, bp.ex);
    mp.G = 1; mp.nblk = 1; mp.gamma = gamma;
    mp.cand_cnt = (const int32_t*)(ws + bp.off_cnt); mp.cand_cap = bp.cap; mp.cand_segs = msegs;
    mp.part_d = (const float*)(ws + bp.off_cd); mp.part_i = (const int32_t*)(ws + bp.off_ci);
    mp.part_maxnorm = reinterpret_cast<const float*>(d_maxnorm);
    // (FILTERED: the merge also reads the thresholds the main sweep used -- the candidate-buffer rule of knn_merge_rerank_selc)
    return ac::knn_exact_tail(ip, mp, bp.ex, nq, mlds, stream, sel, sel ? (const float*)(ws + bp.off_thr) : nullptr);
}

extern "C" int ac_knn_l2_topk_batch(const float* d_P, int64_t N, int64_t ldP, int D, const uint16_t* d_planes,
                                    const float* d_norms, const float* d_Q, int nq, int64_t ldQ, int k, int64_t row_offset,
                                    float* d_outD, double* d_outD64, int64_t* d_outI, void* d_ws, size_t ws_bytes,
                                    int32_t* d_stats, ac_stream_t stream_) {
    return knn_topk_batch(false, d_P, N, ldP, D, d_planes, d_norms, d_Q, nq, ldQ, k, row_offset, d_outD, d_outD64, d_outI, d_ws, ws_bytes,
                          d_stats, stream_);
}

// inner product over the same prepared store: the plan, and hence the workspace, is the L2 batch search's
extern "C" int ac_knn_ip_topk_batch_workspace(int64_t N, int D, int nq, int k, size_t* bytes) {
    return ac_knn_l2_topk_batch_workspace(N, D, nq, k, bytes);
}

extern "C" int ac_knn_ip_topk_batch(const float* d_P, int64_t N, int64_t ldP, int D, const uint16_t* d_planes,
                                    const float* d_norms, const float* d_Q, int nq, int64_t ldQ, int k, int64_t row_offset,
                                    float* d_outD, double* d_outD64, int64_t* d_outI, void* d_ws, size_t ws_bytes,
                                    int32_t* d_stats, ac_stream_t stream_) {
    return knn_topk_batch(true, d_P, N, ldP, D, d_planes, d_norms, d_Q, nq, ldQ, k, row_offset, d_outD, d_outD64, d_outI, d_ws, ws_bytes,
                          d_stats, stream_);
}

// FILTERED search over the prepared store (acamd.h "FILTERED search"): the selection checks of ac_knn_*_topk_sel, then the limits
// of ac_knn_l2_topk_batch -- all before any HIP call; the search is knn_topk_batch with the selection.
static int knn_topk_batch_sel(bool ip, const float* d_P, int64_t N, int64_t ldP, int D, const uint16_t* d_planes, const float* d_norms,
                              const float* d_Q, int nq, int64_t ldQ, int k, int64_t row_offset, const uint64_t* d_sel, int64_t sel_bit0,
                              float* d_outD, double* d_outD64, int64_t* d_outI, void* d_ws, size_t ws_bytes, int32_t* d_stats,
                              ac_stream_t stream_) {
    AC_REQUIRE(sel_bit0 >= 0, AC_EINVAL, "knn batch sel: sel_bit0=%lld must be >= 0", (long long)sel_bit0);
    AC_REQUIRE(d_sel != nullptr, AC_EINVAL, "knn batch sel: d_sel is NULL");
    AC_REQUIRE((((uintptr_t)d_sel) & 7) == 0, AC_EINVAL, "knn batch sel: d_sel must be 8-byte aligned");
    return knn_topk_batch(ip, d_P, N, ldP, D, d_planes, d_norms, d_Q, nq, ldQ, k, row_offset, d_outD, d_outD64, d_outI, d_ws, ws_bytes,
                          d_stats, stream_, d_sel, sel_bit0);
}

extern "C" int ac_knn_l2_topk_batch_sel(const float* d_P, int64_t N, int64_t ldP, int D, const uint16_t* d_planes, const float* d_norms,
                                        const float* d_Q, int nq, int64_t ldQ, int k, int64_t row_offset, const uint64_t* d_sel,
                                        int64_t sel_bit0, float* d_outD, double* d_outD64, int64_t* d_outI, void* d_ws, size_t ws_bytes,
                                        int32_t* d_stats, ac_stream_t stream_) {
    return knn_topk_batch_sel(false, d_P, N, ldP, D, d_planes, d_norms, d_Q, nq, ldQ, k, row_offset, d_sel, sel_bit0, d_outD, d_outD64,
                              d_outI, d_ws, ws_bytes, d_stats, stream_);
}

extern "C" int ac_knn_ip_topk_batch_sel(const float* d_P, int64_t N, int64_t ldP, int D, const uint16_t* d_planes, const float* d_norms,
                                        const float* d_Q, int nq, int64_t ldQ, int k, int64_t row_offset, const uint64_t* d_sel,
                                        int64_t sel_bit0, float* d_outD, double* d_outD64, int64_t* d_outI, void* d_ws, size_t ws_bytes,
                                        int32_t* d_stats, ac_stream_t stream_) {
    return knn_topk_batch_sel(true, d_P, N, ldP, D, d_planes, d_norms, d_Q, nq, ldQ, k, row_offset, d_sel, sel_bit0, d_outD, d_outD64,
                              d_outI, d_ws, ws_bytes, d_stats, stream_);
}
