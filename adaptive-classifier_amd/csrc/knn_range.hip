// Exact range search (radius queries) over the flat store: faiss IndexFlatL2.range_search / IndexFlatIP.range_search.
//   ac_knn_{l2,ip}_range_count   membership of every (query, row) pair as a bitmap, per-query totals -> lims[nq + 1]
//   ac_knn_{l2,ip}_range_fill    the bitmap expanded by ascending row id to I, the exact value of every hit to D (and D64)
//   ac_knn_{l2,ip}_range_count_batch[_sel]   the count over a PREPARED store's fp16 plane (knn_plane_range, further down): the
//                                same bitmaps, resolve, scan and fill; only the sweep and its thresholds differ
// Contract (include/acamd.h): row n is a hit of query q iff float32(d64) < r_q (L2) / float32(v64) > r_q (IP), d64 / v64 the fp64
// value ac_knn_*_topk rounds and returns.  Nothing here depends on the order in which atomics land: every bitmap piece is written
// by exactly one wave with plain vector stores; the only atomic is an integer sum into d_stats[0].
//
// Count phase, big stores (the (N, D) the fused top-k sweep covers):
//   knn_range_sweep<J, IP>   the fp32 row-stream core knn_sweep runs on (knn_stream.h: stage_queries + stream_tiles -- float4 rows
//                            HBM -> VGPR, v_mfma_f32_16x16x4_f32, the query tile in LDS pre-scaled by -2) with an epilogue of its
//                            own: |p|^2 folded in by one extra MFMA, then no lists, no pruning, no barrier.  Each lane owns one
//                            query column and classifies its 4 rows x J queries against two thresholds in sweep-value space (see
//                            "The bound" below): certain-in, certain-out, or ambiguous.
//                            Two bitmaps [nq][W] of 64-bit words (W = ceil(N / 64)): `in` and `amb`.  A wave's tile is 16 rows, so
//                            it owns the 16-BIT PIECE (query, row / 16) of each bitmap -- a quarter of a word, written with one
//                            plain 2-byte store by lanes 0..15.  (A whole word per wave would need 64 consecutive rows per wave,
//                            i.e. a different row -> wave mapping than the core's interleaved 128-row tiles, or a trip through LDS
//                            and a barrier.  A 2-byte store touches no neighbouring piece, so "exactly one writer, no atomic"
//                            holds at piece granularity.)  Both bitmaps are zeroed by a memset before the sweep and only NON-ZERO
//                            pieces are stored: for a selective radius the sweep writes next to nothing.
//   knn_range_resolve<IP>    one wave per (query, strip of 64 words = 4096 rows): every ambiguous pair is decided by the exact
//                            fp64 value rounded to fp32 and compared with r_q (knn_stream.h's wave-order value, the one
//                            knn_merge_rerank computes: same bits as the top-k result), the decided bits are merged into `in` by the lane that owns the word,
//                            the strip's popcount is written.  d_stats[0] += pairs decided.
// Count phase, small stores (N <= kKnnSmallN and a D the sweep does not cover):
//   knn_range_small<IP>      one wave per (query, word): lane b computes the fp64 value of row 64 w + b in knn_small_exact's
//                            (lane) order, decides, the ballot IS the word.  A strip is one word here.
// Both:
//   knn_range_scan           exclusive scan of the strip popcounts per query (offsets relative to the query's first hit) and of
//                            the per-query totals across queries -> lims.  One workgroup.
// Fill phase:
//   knn_range_fill<IP, SMALL>  one wave per strip: hits by ascending row id at lims[q] + offset[q][strip] + rank; exact value per
//                            hit (one wave per hit in the big-store form, one lane per hit in the small-store form).
//
// FILTERED range search (ac_knn_*_range_count_sel; acamd.h "FILTERED RANGE search"): a SEL flag on the sweep and on the small-store
// kernel, nothing else.  The sweep's epilogue fetches the 16 selection bits of its tile (sweep_sel_bits, knn_stream.h: scalar
// loads) and ANDs them into BOTH 16-bit pieces before the non-zero test: an unselected pair is neither certain-in nor ambiguous,
// so it never reaches knn_range_resolve -- a sparse selection saves the exact decisions, and d_stats[0] shows it.  Resolve, scan
// and fill are the unfiltered ones: they only see a bitmap with fewer bits.  Still one writer per piece, plain stores, no new atomic.
// Id-list route (ac_knn_*_range_count_ids / _fill_ids): knn_range_ids_count / knn_range_ids_fill, one wave per (query, 64 list
// positions), the listed rows only; membership over list positions, the same scan.  The exact value is summed in the order the
// bitmap route uses for the same store, so both routes return the same bits.
//
// The bound (certain-in implies the fp32-ROUNDED exact value is on the right side of r):
//   Let s be the real value the sweep approximates (L2: |p|^2 - 2 p.q, IP: -2 p.q) and v its fp32 MFMA-chain value.  knn_topk's
//   certificate uses |v - s| <= gamma0 (|p| + |q|)^2, gamma0 = 1.01 n 2^-24, n = the chain's roundings per term (knn_sweep_gamma0); both
//   sweeps run the one k-loop of stream_tiles, so the same bound holds by construction.  x64 (d64 or v64, in ANY summation order) differs from the real value x by at most
//   (D + 3) 2^-53 (|p| + |q|)^2 (L2: x <= (|p| + |q|)^2, all terms non-negative; IP: sum |p_i q_i| <= |p||q|).  The thresholds
//   below use E = gamma (sqrt~(|p|^2~) + |q|~)^2 + 1e-30 with gamma = 1.02 gamma0: the extra 1 % covers the relative error of the
//   fp32 row norm (<= n 2^-24 <~ 2e-4 for every D the sweep takes), of its hardware square root (1 ulp), of the fp64 |q| and the
//   fp64 error of x64 above (<= 2^-28 gamma0).  Hence |x64 - (v + c)| <= E with c = |q|^2 (L2) and |x64 - (-v / 2)| <= E / 2 (IP).
//     L2  in : v <= (r- - |q|^2) - E, r- = the fp32 predecessor of r  =>  d64 <= r-  =>  float32(d64) <= r- < r (rounding is
//              monotone and r- is representable: the half ulp of the final rounding lies inside the one-ulp step from r- to r).
//         out: v >= (r - |q|^2) + E  =>  d64 >= r  =>  float32(d64) >= r: not a hit.
//     IP  in : v <= -2 r+ - E, r+ = the fp32 successor of r  =>  v64 >= r+  =>  float32(v64) >= r+ > r.
//         out: v >= -2 r + E  =>  v64 <= r  =>  float32(v64) <= r: not a hit.
//   Anything else -- NaN or infinite v or E included, every comparison with them is false -- is ambiguous and decided exactly.
//   Queries that can have no hit (NaN radius; L2 r <= 0; IP r = +inf) are switched off in the sweep: no bit, no exact decision.
#include "common.h"
#include "knn_stream.h"

#include <float.h>
#include <math.h>

namespace {

using namespace acknn;       // the shared streaming core and the exact fp64 value (knn_stream.h)

constexpr int kStripWords = 64;         // words per strip of the big-store form (one lane per word)
constexpr int kPostWaves = 4;           // waves per block of resolve / small / fill

// the predicate of the contract, on the fp32 value the user sees; false for a NaN radius or value
template <bool IP>
__device__ __forceinline__ bool is_hit(double x64, float r) { return IP ? (float)x64 > r : (float)x64 < r; }

// Exact value of one (row, query) pair by a whole wave, in the wave order of knn_stream.h: the bits a top-k search returns for the
// pair.  Columns D..Dp-1 of the row are zero (the store's contract), the query is read element-wise with zeros past D.
template <bool IP>
__device__ __forceinline__ double exact_wave_global(const float* prow, const float* qrow, int D, int nc4, int lane) {
    return exact_wave<IP>(prow, nc4, lane, [&](int c4) {
        const int c = 4 * c4;
        f32x4 qq;
        qq.x = qrow[c];                                   // (c < D: c4 < nc4 = ceil(D / 4))
        qq.y = c + 1 < D ? qrow[c + 1] : 0.f;
        qq.z = c + 2 < D ? qrow[c + 2] : 0.f;
        qq.w = c + 3 < D ? qrow[c + 3] : 0.f;
        return qq;
    });
}

__device__ __forceinline__ uint64_t shfl64(uint64_t v, int src) {
    const uint32_t lo = __shfl((uint32_t)v, src), hi = __shfl((uint32_t)(v >> 32), src);
    return ((uint64_t)hi << 32) | lo;
}

struct RangeParams {
    const float* P;
    int64_t N;
    int64_t ldP;
    const float* Q;
    int64_t ldQ;
    const float* radius;  // [nq]
    int D;
    int Dp;       // round_up(D, 4)
    int ng;       // k-groups per tile: ceil(Dp / (16 * kGroup))
    int nq;
    int G;        // row groups (blocks per query tile)
    int nqt;      // query tiles
    int64_t ntiles;   // ceil(N / 128)
    int64_t W;        // words per query: ceil(N / 64)
    int64_t S;        // strips per query
    double gamma;     // 1.02 x knn_topk's gamma
    uint64_t* bm_in;  // [nq][W]
    uint64_t* bm_amb; // [nq][W]
    int32_t* cnt;     // [nq][S] hits per strip
    int64_t* off;     // [nq][S] hits of the query before the strip
    const float* zeros;
    int32_t* stats;   // may be NULL
    // fill
    int64_t row_offset;
    int64_t* lims;    // [nq + 1]
    int64_t capacity;
    float* outD;
    double* outD64;   // may be NULL
    int64_t* outI;
};

// FILTERED range search (the SEL instantiations take this struct; the plain ones keep RangeParams and with it their kernarg
// segment, as SweepParams / SweepParamsSel in knn_l2.hip): row r can be a hit iff bit (sel_bit0 + r) of the bitmap is set
struct RangeParamsSel : RangeParams {
    const uint64_t* sel;
    int64_t sel_bit0;
};
template <bool SEL> struct range_params_of { typedef RangeParams type; };
template <> struct range_params_of<true> { typedef RangeParamsSel type; };

// Id-list route: membership is a bitmap over LIST POSITIONS (word w of a query = positions 64 w .. 64 w + 63 of ids), a strip is
// one word; bm_in / cnt / off / W = S = ceil(M / 64) of the base struct are laid out for that
struct RangeParamsIds : RangeParams {
    const int64_t* ids;   // [M] sorted, unique; an id outside [0, N) is skipped
    int64_t M;
};

template <int J, bool IP, bool SEL = false>
__global__ __launch_bounds__(kThreads, 2) void knn_range_sweep(typename range_params_of<SEL>::type prm) {
    static_assert(J == 1 || J == 2, "query tile = 1 or 2 sub-tiles of 16");
    constexpr int TQ = 16 * J;
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int nblk = prm.G * prm.nqt;
    const int v = xcd_remap(blockIdx.x, nblk);
    const int qt = v % prm.nqt;
    const int g = v / prm.nqt;

    // ---- LDS: the query tile in B-fragment order | per query: c_in, c_out, |q| (fp64), live ----
    const int nslots = J * prm.ng * kGroup * 64;      // float4 slots of the query tile
    f32x4* Qs = reinterpret_cast<f32x4*>(smem);
    double* cin_s = reinterpret_cast<double*>(smem + (size_t)nslots * 16);
    double* cout_s = cin_s + TQ;
    double* qn_s = cout_s + TQ;
    int* live_s = reinterpret_cast<int*>(qn_s + TQ);

    stage_queries<J>(Qs, prm.Q, prm.ldQ, prm.D, prm.nq, prm.ng, qt, tid);
    // per-query constants of the thresholds, in fp64 (a wave per query)
    for (int t = wave; t < TQ; t += kWaves) {
        const int qrow = qt * TQ + t;
        double a = 0;
        float r = NAN;
        if (qrow < prm.nq) {
            const float* src = prm.Q + (size_t)qrow * prm.ldQ;
            for (int c = lane; c < prm.D; c += 64) a = fma((double)src[c], (double)src[c], a);
            r = prm.radius[qrow];
        }
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) a += __shfl_xor(a, o);
        if (lane == 0) {
            const bool live = IP ? (r < INFINITY) : (r > 0.f);            // false for NaN
            if (IP) {
                cin_s[t] = -2.0 * (double)nextafterf(r, INFINITY);
                cout_s[t] = -2.0 * (double)r;
            } else {
                cin_s[t] = (double)nextafterf(r, -INFINITY) - a;
                cout_s[t] = (double)r - a;
            }
            qn_s[t] = sqrt(a);
            live_s[t] = live ? 1 : 0;
        }
    }
    __syncthreads();

    const int j = lane & 15;            // query column (within each sub-tile) this lane owns in C/D
    const int ksub = lane >> 4;         // in C/D the lane owns rows 4 ksub + r of the tile
    double cin[J], cout[J], qn[J];
    bool live[J];
#pragma unroll
    for (int jj = 0; jj < J; ++jj) {
        cin[jj] = cin_s[16 * jj + j]; cout[jj] = cout_s[16 * jj + j]; qn[jj] = qn_s[16 * jj + j];
        live[jj] = live_s[16 * jj + j] != 0;
    }

    const size_t pieces = (size_t)prm.W * 4;          // 16-bit pieces per query
    uint16_t* in16 = reinterpret_cast<uint16_t*>(prm.bm_in);
    uint16_t* amb16 = reinterpret_cast<uint16_t*>(prm.bm_amb);

    // per 16-row tile of this wave: classify 4 rows x J queries per lane, store the non-zero pieces
    auto epilogue = [&](f32x4 (&acc)[J], float nsq, int64_t row_base) {
        // FILTERED: the tile's 16 selection bits, in both halves (certain-in | ambiguous).  A tile without a selected row stores
        // nothing, so it is not classified either (wave-uniform: the bits come through the scalar unit).
        uint32_t selmask = 0xffffffffu;
        if constexpr (SEL) {
            const uint32_t sb = sweep_sel_bits(prm.sel, prm.sel_bit0, prm.N, row_base);
            if (sb == 0u) return;
            selmask = sb | (sb << 16);
        }
        // |p|^2 of the lane's four C/D rows: A = the lane's partial sum of squares, B = 1 (every column gets its row's sum)
        const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
        const f32x4 pn2 = Shape::mfma(nsq, 1.0f, zero4);
        if constexpr (!IP) {                          // the same fold as knn_sweep: v = |p|^2 - 2 p.q
#pragma unroll
            for (int jj = 0; jj < J; ++jj) acc[jj] = Shape::mfma(nsq, 1.0f, acc[jj]);
        }
        double pn[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) pn[r] = (double)__builtin_amdgcn_sqrtf(pn2[r]);
#pragma unroll
        for (int jj = 0; jj < J; ++jj) {
            uint32_t bits = 0;                        // low half: certain-in, high half: ambiguous; bit = row within the 16-row tile
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const double t = pn[r] + qn[jj];
                const double E = prm.gamma * t * t + 1e-30;
                const double dv = (double)acc[jj][r];
                const bool ok = live[jj] && row_base + 4 * ksub + r < prm.N;
                // (a chain that overflowed on the way ends infinite or NaN: the bound is void then, the pair is decided exactly)
                const bool fin = E < (double)INFINITY && fabs(dv) < (double)INFINITY;
                const bool in = fin && dv <= cin[jj] - E;
                const bool out = fin && dv >= cout[jj] + E;
                if (ok && in) bits |= 1u << (4 * ksub + r);
                if (ok && !in && !out) bits |= 0x10000u << (4 * ksub + r);
            }
            bits |= __shfl_xor(bits, 16);
            bits |= __shfl_xor(bits, 32);
            // an unselected pair leaves BOTH pieces before the non-zero test: it is neither a hit nor ever decided exactly
            if constexpr (SEL) bits &= selmask;
            // lanes 0..15 hold the two 16-bit pieces of query column j; rows past N and columns past nq never set a bit
            if (lane < 16 && bits) {
                const size_t at = (size_t)(qt * TQ + 16 * jj + j) * pieces + (size_t)(row_base >> 4);
                if (bits & 0xffffu) in16[at] = (uint16_t)(bits & 0xffffu);
                if (bits >> 16) amb16[at] = (uint16_t)(bits >> 16);
            }
        }
    };
    stream_tiles<J>(prm.P, prm.N, prm.ldP, prm.Dp, prm.ng, prm.G, g, prm.ntiles, prm.zeros, Qs, lane, wave, epilogue);
}

// one wave per (query, strip): decide the ambiguous pairs exactly, merge them into `in`, count the strip's hits
template <bool IP>
__global__ __launch_bounds__(kPostWaves * 64) void knn_range_resolve(RangeParams prm) {
    const int lane = threadIdx.x & 63;
    const int64_t wid = (int64_t)blockIdx.x * kPostWaves + (threadIdx.x >> 6);
    if (wid >= (int64_t)prm.nq * prm.S) return;           // (wave-uniform)
    const int64_t q = wid / prm.S, strip = wid - q * prm.S;
    const int64_t w = strip * kStripWords + lane;
    const bool have = w < prm.W;
    const size_t at = (size_t)q * prm.W + (have ? w : 0);
    uint64_t in = have ? prm.bm_in[at] : 0, amb = have ? prm.bm_amb[at] : 0;
    const uint64_t amb0 = amb;
    unsigned long long pending = __builtin_amdgcn_ballot_w64(amb != 0);
    int decided = 0;
    if (pending) {
        const float r = prm.radius[q];
        const float* qrow = prm.Q + (size_t)q * prm.ldQ;
        const int nc4 = prm.Dp >> 2;
        while (pending) {
            const int l = __builtin_ctzll(pending);
            pending &= pending - 1;
            uint64_t aw = shfl64(amb, l);
            const int64_t row0 = (strip * kStripWords + l) * 64;
            while (aw) {
                const int b = __builtin_ctzll(aw);
                aw &= aw - 1;
                const double x = exact_wave_global<IP>(prm.P + (size_t)(row0 + b) * prm.ldP, qrow, prm.D, nc4, lane);      // (row < N: the sweep masks)
                if (lane == l && is_hit<IP>(x, r)) in |= 1ull << b;
                ++decided;
            }
        }
    }
    if (amb0) prm.bm_in[at] = in;
    int c = __builtin_popcountll(in);
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) c += __shfl_xor(c, o);
    if (lane == 0) {
        prm.cnt[wid] = c;
        if (decided && prm.stats) atomicAdd(&prm.stats[0], decided);        // an integer sum: the same whatever the order
    }
}

// the pairs a kernel that decides EVERY candidate pair exactly reports in d_stats[0]: nq x candidates, saturated
__device__ __forceinline__ int32_t exact_pairs(int64_t candidates, int nq) {
    const int64_t pairs = candidates * (int64_t)nq;
    return pairs > 2147483647LL ? 2147483647 : (int32_t)pairs;
}

// small stores: one wave per (query, word); every pair is decided by its exact value.  SEL: every SELECTED pair -- an unselected
// row is not evaluated (its selection bit is read only for a row < N: no word behind (sel_bit0 + N - 1) / 64 is touched)
template <bool IP, bool SEL = false>
__global__ __launch_bounds__(kPostWaves * 64) void knn_range_small(typename range_params_of<SEL>::type prm) {
    const int lane = threadIdx.x & 63;
    const int64_t wid = (int64_t)blockIdx.x * kPostWaves + (threadIdx.x >> 6);
    auto selected = [&](int64_t row) {
        if constexpr (SEL) {
            const int64_t b = prm.sel_bit0 + row;
            return ((prm.sel[b >> 6] >> (b & 63)) & 1ull) != 0;
        } else {
            return true;
        }
    };
    if constexpr (SEL) {
        if (blockIdx.x == 0 && threadIdx.x < 64 && prm.stats) {        // wave 0 counts the selected rows: no atomic
            int64_t nsel = 0;
            for (int64_t r0 = 0; r0 < prm.N; r0 += 64)                  // (N <= kKnnSmallN)
                nsel += __builtin_popcountll(__builtin_amdgcn_ballot_w64(r0 + lane < prm.N && selected(r0 + lane)));
            if (lane == 0) prm.stats[0] = exact_pairs(nsel, prm.nq);
        }
    } else {
        if (blockIdx.x == 0 && threadIdx.x == 0 && prm.stats) prm.stats[0] = exact_pairs(prm.N, prm.nq);
    }
    if (wid >= (int64_t)prm.nq * prm.W) return;
    const int64_t q = wid / prm.W, w = wid - q * prm.W;
    const int64_t row = w * 64 + lane;
    bool hit = false;
    if (row < prm.N && selected(row)) {
        const double x = exact_lane<IP>(prm.P + (size_t)row * prm.ldP, prm.Q + (size_t)q * prm.ldQ, prm.D);
        hit = is_hit<IP>(x, prm.radius[q]);
    }
    const unsigned long long word = __builtin_amdgcn_ballot_w64(hit);
    if (lane == 0) {
        prm.bm_in[wid] = word;
        prm.cnt[wid] = __builtin_popcountll(word);
    }
}

// cnt[nq][S] -> off[nq][S] (hits of the query before the strip), lims[0] = 0, lims[q + 1] = hits of queries 0..q.  One workgroup.
constexpr int kScanThreads = 1024;
__global__ __launch_bounds__(kScanThreads) void knn_range_scan(const int32_t* cnt, int64_t* off, int64_t* lims, int nq, int64_t S) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    __shared__ int64_t wtot[kScanThreads / 64];
    __shared__ int64_t carry_s;
    for (int q = wave; q < nq; q += kScanThreads / 64) {
        int64_t running = 0;
        for (int64_t s0 = 0; s0 < S; s0 += 64) {
            const int64_t s = s0 + lane;
            const int64_t c = s < S ? (int64_t)cnt[(size_t)q * S + s] : 0;
            int64_t incl = c;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) { const int64_t t = __shfl_up(incl, o); if (lane >= o) incl += t; }
            if (s < S) off[(size_t)q * S + s] = running + incl - c;
            running += __shfl(incl, 63);
        }
        if (lane == 0) lims[q + 1] = running;             // the query's total; scanned in place below
    }
    if (tid == 0) { lims[0] = 0; carry_s = 0; }
    __syncthreads();
    for (int base = 0; base < nq; base += kScanThreads) {
        const int q = base + tid;
        const int64_t c = q < nq ? lims[q + 1] : 0;
        int64_t incl = c;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const int64_t t = __shfl_up(incl, o); if (lane >= o) incl += t; }
        if (lane == 63) wtot[wave] = incl;
        __syncthreads();
        int64_t before = carry_s;
        for (int wv = 0; wv < wave; ++wv) before += wtot[wv];
        if (q < nq) lims[q + 1] = before + incl;
        __syncthreads();
        if (tid == kScanThreads - 1) carry_s = before + incl;
        __syncthreads();
    }
}

// one wave per strip: the hits by ascending row id, with their exact values
template <bool IP, bool SMALL>
__global__ __launch_bounds__(kPostWaves * 64) void knn_range_fill(RangeParams prm) {
    const int lane = threadIdx.x & 63;
    const int64_t wid = (int64_t)blockIdx.x * kPostWaves + (threadIdx.x >> 6);
    const bool overflow = prm.lims[prm.nq] > prm.capacity;
    if (blockIdx.x == 0 && threadIdx.x == 0 && prm.stats) prm.stats[1] = overflow ? 1 : 0;
    if (overflow || wid >= (int64_t)prm.nq * prm.S) return;
    const int64_t q = wid / prm.S, strip = wid - q * prm.S;
    const int64_t first = prm.lims[q] + prm.off[wid];
    const float* qrow = prm.Q + (size_t)q * prm.ldQ;
    if constexpr (SMALL) {                                // a strip is one word; one lane per hit, knn_small_exact's order
        const uint64_t word = prm.bm_in[wid];
        if ((word >> lane) & 1ull) {
            const int64_t row = strip * 64 + lane;
            const int64_t pos = first + __builtin_popcountll(word & ((1ull << lane) - 1ull));
            const double x = exact_lane<IP>(prm.P + (size_t)row * prm.ldP, qrow, prm.D);
            prm.outD[pos] = (float)x;
            if (prm.outD64) prm.outD64[pos] = x;
            prm.outI[pos] = row + prm.row_offset;
        }
    } else {
        const int64_t w = strip * kStripWords + lane;
        const uint64_t in = w < prm.W ? prm.bm_in[(size_t)q * prm.W + w] : 0;
        unsigned long long pending = __builtin_amdgcn_ballot_w64(in != 0);
        const int nc4 = prm.Dp >> 2;
        int64_t pos = first;
        while (pending) {
            const int l = __builtin_ctzll(pending);
            pending &= pending - 1;
            uint64_t iw = shfl64(in, l);
            const int64_t row0 = (strip * kStripWords + l) * 64;
            while (iw) {
                const int b = __builtin_ctzll(iw);
                iw &= iw - 1;
                const double x = exact_wave_global<IP>(prm.P + (size_t)(row0 + b) * prm.ldP, qrow, prm.D, nc4, lane);
                if (lane == 0) {                          // pos < lims[nq] <= capacity
                    prm.outD[pos] = (float)x;
                    if (prm.outD64) prm.outD64[pos] = x;
                    prm.outI[pos] = row0 + b + prm.row_offset;
                }
                ++pos;
            }
        }
    }
}

// ---- the id-list route: M listed rows, membership over list positions ----
// one wave per (query, word of 64 list positions): every listed pair with an id inside [0, N) is decided by its exact value, in
// the summation order the bitmap route uses for the same store (LANE_ORDER = its small-store kernel's, else the wave order of
// resolve / fill) -- the same bits, hence the same verdicts and the same D.  The word is written by the one wave that owns it.
template <bool IP, bool LANE_ORDER>
__global__ __launch_bounds__(kPostWaves * 64) void knn_range_ids_count(RangeParamsIds prm) {
    const int lane = threadIdx.x & 63;
    const int64_t wid = (int64_t)blockIdx.x * kPostWaves + (threadIdx.x >> 6);
    if (blockIdx.x == 0 && threadIdx.x < 64 && prm.stats) {            // wave 0 counts the valid ids: no atomic
        int64_t valid = 0;
        for (int64_t m0 = 0; m0 < prm.M; m0 += 64) {                    // (M <= kKnnSmallN)
            const int64_t id = m0 + lane < prm.M ? prm.ids[m0 + lane] : -1;
            valid += __builtin_popcountll(__builtin_amdgcn_ballot_w64(id >= 0 && id < prm.N));
        }
        if (lane == 0) prm.stats[0] = exact_pairs(valid, prm.nq);
    }
    if (wid >= (int64_t)prm.nq * prm.W) return;                        // (wave-uniform)
    const int64_t q = wid / prm.W, w = wid - q * prm.W;
    const int64_t m = w * 64 + lane;
    int64_t id = m < prm.M ? prm.ids[m] : -1;
    if (id >= prm.N) id = -1;
    const float r = prm.radius[q];
    const float* qrow = prm.Q + (size_t)q * prm.ldQ;
    unsigned long long word;
    if constexpr (LANE_ORDER) {
        bool hit = false;
        if (id >= 0) hit = is_hit<IP>(exact_lane<IP>(prm.P + (size_t)id * prm.ldP, qrow, prm.D), r);
        word = __builtin_amdgcn_ballot_w64(hit);
    } else {
        word = 0;
        unsigned long long todo = __builtin_amdgcn_ballot_w64(id >= 0);
        const int nc4 = prm.Dp >> 2;
        while (todo) {
            const int b = __builtin_ctzll(todo);
            todo &= todo - 1;
            const int64_t row = (int64_t)shfl64((uint64_t)id, b);
            const double x = exact_wave_global<IP>(prm.P + (size_t)row * prm.ldP, qrow, prm.D, nc4, lane);
            if (is_hit<IP>(x, r)) word |= 1ull << b;                    // (every lane holds the sum: the word is wave-uniform)
        }
    }
    if (lane == 0) {
        prm.bm_in[wid] = word;
        prm.cnt[wid] = __builtin_popcountll(word);
    }
}

// one wave per (query, word): the hits by ascending list position = ascending row id (the list is sorted), with their exact values
template <bool IP, bool LANE_ORDER>
__global__ __launch_bounds__(kPostWaves * 64) void knn_range_ids_fill(RangeParamsIds prm) {
    const int lane = threadIdx.x & 63;
    const int64_t wid = (int64_t)blockIdx.x * kPostWaves + (threadIdx.x >> 6);
    const bool overflow = prm.lims[prm.nq] > prm.capacity;
    if (blockIdx.x == 0 && threadIdx.x == 0 && prm.stats) prm.stats[1] = overflow ? 1 : 0;
    if (overflow || wid >= (int64_t)prm.nq * prm.W) return;
    const int64_t q = wid / prm.W, w = wid - q * prm.W;
    const uint64_t word = prm.bm_in[wid];
    if (!word) return;                                                  // (wave-uniform)
    const int64_t first = prm.lims[q] + prm.off[wid];
    const float* qrow = prm.Q + (size_t)q * prm.ldQ;
    const int64_t m = w * 64 + lane;
    const int64_t id = m < prm.M ? prm.ids[m] : 0;                      // (a set bit is a valid id)
    if constexpr (LANE_ORDER) {
        if ((word >> lane) & 1ull) {
            const int64_t pos = first + __builtin_popcountll(word & ((1ull << lane) - 1ull));
            const double x = exact_lane<IP>(prm.P + (size_t)id * prm.ldP, qrow, prm.D);
            prm.outD[pos] = (float)x;
            if (prm.outD64) prm.outD64[pos] = x;
            prm.outI[pos] = id + prm.row_offset;
        }
    } else {
        const int nc4 = prm.Dp >> 2;
        int64_t pos = first;
        uint64_t iw = word;
        while (iw) {
            const int b = __builtin_ctzll(iw);
            iw &= iw - 1;
            const int64_t row = (int64_t)shfl64((uint64_t)id, b);
            const double x = exact_wave_global<IP>(prm.P + (size_t)row * prm.ldP, qrow, prm.D, nc4, lane);
            if (lane == 0) {                                            // pos < lims[nq] <= capacity
                prm.outD[pos] = (float)x;
                if (prm.outD64) prm.outD64[pos] = x;
                prm.outI[pos] = row + prm.row_offset;
            }
            ++pos;
        }
    }
}

// --------------------------------------------------------------------------------------
// Range search over the PREPARED store's fp16 plane (ac_knn_*_range_count_batch): the count phase reads 2 B per store element.
//   knn_plane_range_thresholds<IP>   one wave per query: |q|^2 in fp64, E_q = gamma (|p|max + |q|)^2, the two thresholds of the
//                                    query rounded to fp32 to the safe side, the "can this query hit at all" flag.
//   knn_plane_range<TQ, IP, SEL>     the load path and k-loop of knn_plane_sweep (knn_l2.hip -- a COPY: that kernel is left as it
//                                    is, folding the two into one header is a follow-up) with a range epilogue: no lists, no
//                                    pruning, no tau, no barrier and no LDS traffic after the k-loop.
// After the sweep the launch sequence is the fp32 route's: knn_range_resolve decides every ambiguous pair from the fp32 rows by the
// same fp64 value, knn_range_scan makes lims, and the unchanged knn_range_fill expands the same bitmap.
//
// The bound.  The sweep value is knn_plane_sweep's: L2 v = fmaf(acc, f_q, |p|^2) with |p|^2 from the prepared norms, IP v = f_q acc
// (f_q = -2 2^(e_p + e_q), acc = h_p . h_q in the fp32 accumulator of v_mfma_f32_32x32x16_f16).  include/acamd.h derives
//   |v - s| <= gamma_b (|p|max + |q|)^2,  gamma_b = knn_batch_gamma(D) = 1.01 (2^-11 + (Kp + 18 + sqrt Kp) 2^-24)
// for s = |p|^2 - 2 p.q (L2) and s = -2 p.q (IP), |p|max = the store maximum kept at d_norms[round_up(N, 256)] -- the bound the
// top-k certificate over the plane relies on.  It is a bound PER QUERY: the absolute 2^-25 sqrt(Kp) term of the fp16 rounding does
// not shrink with a row's own norm, so no per-row form is used.  E_q = 1.02 gamma_b (|p|max~ + |q|~)^2 + 1e-30: the 2 % cover the
// fp32 rounding of the stored maximum (2^-24 relative), the fp64 |q| and the (D + 3) 2^-53 (|p| + |q|)^2 of the exact fp64 value
// (the argument at the top of this file, with gamma_b >= 2^-11 in place of gamma0).  With E_q a constant of the query both
// thresholds are constants too, computed once in fp64 and rounded to fp32 so that the fp32 compare implies the fp64 one:
//     L2  in : v <= fl_down((r- - |q|^2) - E)      out: v >= fl_up((r - |q|^2) + E)
//     IP  in : v <= fl_down(-2 r+ - E)             out: v >= fl_up(-2 r + E)
// Everything else is ambiguous: a NaN or infinite v, a NaN threshold (E or |q| not finite), an infinite threshold (no finite v is
// beyond it).  Queries that cannot hit (NaN radius, L2 r <= 0, IP r = +inf) are switched off.  A STALE plane voids the bound.
//
// Bitmap writes.  A wave's tile is 32 consecutive rows: it owns the 32-BIT piece (query, row / 32) of bm_in and of bm_amb -- half a
// word.  In the C/D layout of the 32x32 MFMA a lane holds 16 verdicts of its query column (rows plane_acc_row(r, lane)), the two
// lane halves hold complementary rows: one __shfl_xor(.., 32) of a packed word joins them, lanes 0..31 store the non-zero pieces with
// one plain 4-byte store each.  Exactly one writer per piece, no atomic; the bitmaps are zeroed by the memset before the sweep.
// Rows past N -- zero plane rows whose IP value 0 beats every negative product, and the clamped reloads behind the last tile -- are
// masked explicitly in both metrics; SEL ANDs the tile's 32 selection bits into both pieces and skips a tile without a selected row.
// --------------------------------------------------------------------------------------
struct PlaneRangeParams {
    const uint16_t* Pp;       // store plane, tile-major (knn_batch.hip knn_plane_kernel)
    const float* pnorm;       // [round_up(N, 256)] |p|^2, +inf past N
    const uint16_t* Qp;       // query plane [Kp/8][q_rows][8]
    int64_t q_rows;           // round_up(nq, 256)
    const float* qfac;        // [q_rows] -2 2^(e_p + e_q)
    const float* thr_in;      // [q_rows] certain-in  iff v <= thr_in
    const float* thr_out;     // [q_rows] certain-out iff v >= thr_out
    const int32_t* live;      // [q_rows] 0 = the query cannot hit (or is padding)
    int64_t N;
    int64_t ntiles;           // ceil(N / 256)
    int64_t W;                // 64-bit words per query of each bitmap
    uint64_t* bm_in;          // [nq][W]
    uint64_t* bm_amb;         // [nq][W]
    int32_t* stats;           // first launch of a call: stats[2] = 2 (the plane sweep ran); else NULL
    int Kp;                   // multiple of 64
    int q0, nq;               // this launch's query tile starts at q0; nq = queries of the whole call
    int G;
};
struct PlaneRangeParamsSel : PlaneRangeParams {
    const uint64_t* sel;
    int64_t sel_bit0;
};
template <bool SEL> struct plane_range_params_of { typedef PlaneRangeParams type; };
template <> struct plane_range_params_of<true> { typedef PlaneRangeParamsSel type; };

// (knn_l2.hip plane_sel_bits) the 32 selection bits of a wave's rows row_base .. row_base + 31 (bit i = row row_base + i): two
// 64-bit words at most, through the scalar unit, the second one only if one of its rows exists.  row_base < N.
__device__ __forceinline__ uint32_t plane_range_sel_bits(const uint64_t* sel, int64_t sel_bit0, int64_t N, int row_base) {
    typedef const uint64_t __attribute__((address_space(4)))* cup;
    const uint32_t rem = __builtin_amdgcn_readfirstlane((uint32_t)(sel_bit0 & 63) + (uint32_t)row_base);     // (N < 2^31)
    const cup w = (cup)(uintptr_t)(sel + (sel_bit0 >> 6) + (rem >> 6));
    const int s = (int)(rem & 63u);
    uint64_t bits = w[0] >> s;
    if (s > 32 && row_base + (64 - s) < N) bits |= w[1] << (64 - s);
    return (uint32_t)bits;
}

__device__ __forceinline__ float f32_round_down(double x) {        // the largest fp32 <= x (NaN stays NaN)
    float t = (float)x;
    if ((double)t > x) t = nextafterf(t, -INFINITY);
    return t;
}
__device__ __forceinline__ float f32_round_up(double x) {          // the smallest fp32 >= x
    float t = (float)x;
    if ((double)t < x) t = nextafterf(t, INFINITY);
    return t;
}

// one wave per row of the padded query plane (q_rows rows): rows past nq are switched off
template <bool IP>
__global__ __launch_bounds__(kPostWaves * 64) void knn_plane_range_thresholds(const float* Q, int64_t ldQ, int D, int nq, int64_t q_rows,
                                                                              const float* radius, const float* maxnorm, double gamma,
                                                                              float* thr_in, float* thr_out, int32_t* live) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * kPostWaves + (threadIdx.x >> 6);
    if (row >= q_rows) return;                            // (wave-uniform)
    double a = 0;
    float r = NAN;
    if (row < nq) {
        const float* src = Q + (size_t)row * ldQ;
        for (int c = lane; c < D; c += 64) a = fma((double)src[c], (double)src[c], a);
        r = radius[row];
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) a += __shfl_xor(a, o);
    if (lane == 0) {
        const double t = sqrt((double)maxnorm[0]) + sqrt(a);
        const double E = gamma * t * t + 1e-30;
        double cin, cout;
        if (IP) {
            cin = -2.0 * (double)nextafterf(r, INFINITY) - E;
            cout = -2.0 * (double)r + E;
        } else {
            cin = ((double)nextafterf(r, -INFINITY) - a) - E;
            cout = ((double)r - a) + E;
        }
        thr_in[row] = f32_round_down(cin);
        thr_out[row] = f32_round_up(cout);
        live[row] = (IP ? (r < INFINITY) : (r > 0.f)) ? 1 : 0;          // false for NaN and for the padding rows
    }
}

typedef _Float16 rf16x8 __attribute__((ext_vector_type(8)));
typedef uint32_t ru32x4 __attribute__((ext_vector_type(4)));
typedef float rf32x16 __attribute__((ext_vector_type(16)));

template <int TQ, bool IP, bool SEL = false>
__global__ __launch_bounds__(kThreads, 2) void knn_plane_range(typename plane_range_params_of<SEL>::type prm) {
    constexpr int NJ = TQ / 32;                       // 32-column sub-tiles of the query tile
    constexpr int NB = 4, GK = 4;                     // register buffers x k-steps per buffer (16 loads in flight)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i32 = lane & 31, kg = lane >> 5;
    const int g = xcd_remap(blockIdx.x, prm.G);
    if (blockIdx.x == 0 && tid == 0 && prm.stats) prm.stats[2] = 2;       // (after the count's memset of d_stats, same stream)
    const int nk = prm.Kp >> 4;                       // 16-k MFMA steps per row
    const int ngrp = nk / GK;                         // (Kp % 64 == 0)
    // ---- LDS: the query fragments [nk][NJ][64] x 16 B, nothing else ----
    ru32x4* Qs = reinterpret_cast<ru32x4*>(smem);
    for (int t = tid; t < nk * NJ * 64; t += kThreads) {
        const int l = t & 63, jj = (t >> 6) % NJ, s = (t >> 6) / NJ;
        const int64_t qrow = prm.q0 + 32 * jj + (l & 31);          // (< q_rows: the plane is padded to 256 queries with zeros)
        Qs[t] = *reinterpret_cast<const ru32x4*>(prm.Qp + ((int64_t)(2 * s + (l >> 5)) * prm.q_rows + qrow) * 8);
    }
    // this lane's query columns: factor, thresholds, live (the per-query arrays are q_rows long)
    float qf[NJ], tin[NJ], tout[NJ];
    bool live[NJ];
#pragma unroll
    for (int jj = 0; jj < NJ; ++jj) {
        const int qrow = prm.q0 + 32 * jj + i32;
        qf[jj] = prm.qfac[qrow]; tin[jj] = prm.thr_in[qrow]; tout[jj] = prm.thr_out[qrow];
        live[jj] = qrow < prm.nq && prm.live[qrow] != 0;
    }
    __syncthreads();

    const int64_t my_tiles = (prm.ntiles > g) ? (prm.ntiles - 1 - g) / prm.G + 1 : 0;
    const int64_t total = my_tiles * ngrp;            // groups of GK k-steps this wave consumes
    const size_t tile_bytes = (size_t)prm.Kp * 512;   // 256 rows x Kp x 2 B
    const uint32_t lane_off = (uint32_t)(kg * 256 + 32 * wave + i32) * 16u;    // byte offset of this lane's piece inside a k-slot pair
    int64_t pf_tile = 0;                              // prefetch state: next group to load
    int pf_grp = 0;
    auto tile_base = [&](int64_t it) -> const char* {
        int64_t T = it * prm.G + g;
        if (T > prm.ntiles - 1) T = prm.ntiles - 1;    // past the end: the last tile again (never consumed)
        return reinterpret_cast<const char*>(prm.Pp) + (size_t)T * tile_bytes;
    };
    const char* pf_base = tile_base(0);
    ru32x4 buf[NB][GK];
#define AC_PR_PREFETCH(B)                                                                                     \
    do {                                                                                                      \
        const char* src_ = pf_base + (size_t)pf_grp * (GK * 8192) + lane_off;                                 \
        _Pragma("unroll") for (int u = 0; u < GK; ++u)                                                        \
            buf[B][u] = __builtin_nontemporal_load(reinterpret_cast<const ru32x4*>(src_ + u * 8192));          \
        if (++pf_grp == ngrp) { pf_grp = 0; ++pf_tile; pf_base = tile_base(pf_tile); }                        \
    } while (0)

    rf32x16 acc[NJ];
    int64_t cur_tile = 0;
    int cur_grp = 0;
    const size_t pieces = (size_t)prm.W * 2;          // 32-bit pieces per query
    uint32_t* in32 = reinterpret_cast<uint32_t*>(prm.bm_in);
    uint32_t* amb32 = reinterpret_cast<uint32_t*>(prm.bm_amb);

    // per 32-row tile of this wave: classify 16 rows x NJ queries per lane, store the non-zero pieces
    auto epilogue = [&]() {
        const int row0 = __builtin_amdgcn_readfirstlane((int)((cur_tile * prm.G + g) * 256) + 32 * wave);     // (N < 2^31)
        if (row0 >= prm.N) return;                                             // (wave-uniform) a tile of padding rows
        const int64_t left = prm.N - row0;
        uint32_t rowmask = left >= 32 ? 0xffffffffu : (1u << (int)left) - 1u;   // rows past N never set a bit, in either metric
        if constexpr (SEL) {
            rowmask &= plane_range_sel_bits(prm.sel, prm.sel_bit0, prm.N, row0);
            if (rowmask == 0u) return;                                         // no selected row: nothing to classify or store
        }
        typedef const float __attribute__((address_space(4)))* cfp;
        const cfp pn = (cfp)(uintptr_t)(prm.pnorm + row0);                     // (L2) |p|^2 of the wave's rows through the scalar unit
        uint32_t in_b[NJ], amb_b[NJ];
#pragma unroll
        for (int jj = 0; jj < NJ; ++jj) { in_b[jj] = 0u; amb_b[jj] = 0u; }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int rr = (r & 3) + 8 * (r >> 2);                             // this lane's row: rr + 4 kg (the MFMA's C/D layout)
            float pnr = 0.f;
            if constexpr (!IP) {
                const float lo = pn[rr], hi = pn[rr + 4];
                pnr = kg ? hi : lo;
            }
            const uint32_t bit = (1u << rr) << (4 * kg);
#pragma unroll
            for (int jj = 0; jj < NJ; ++jj) {
                const float v = IP ? acc[jj][r] * qf[jj] : fmaf(acc[jj][r], qf[jj], pnr);      // knn_plane_sweep's value
                const bool fin = fabsf(v) < INFINITY;                          // false for NaN too: the bound is void, decide exactly
                const bool in = fin && v <= tin[jj];
                const bool out = fin && v >= tout[jj];
                if (in) in_b[jj] |= bit;
                if (!in && !out) amb_b[jj] |= bit;
            }
        }
#pragma unroll
        for (int jj = 0; jj < NJ; ++jj) {
            // lane half 0 holds rows {0-3, 8-11, ..} (mask 0x0f0f0f0f), half 1 the others: `in` stays in place, `amb` moves into
            // the free nibbles, ONE shuffle exchanges both
            const uint32_t packed = kg ? (in_b[jj] | (amb_b[jj] >> 4)) : (in_b[jj] | (amb_b[jj] << 4));
            const uint32_t other = __shfl_xor(packed, 32);
            uint32_t in_w = in_b[jj] | (other & 0xf0f0f0f0u);                   // (meaningful in lanes 0..31, which store)
            uint32_t amb_w = amb_b[jj] | ((other & 0x0f0f0f0fu) << 4);
            in_w &= rowmask; amb_w &= rowmask;
            if (kg == 0 && live[jj] && (in_w | amb_w)) {
                const size_t at = (size_t)(prm.q0 + 32 * jj + i32) * pieces + (size_t)(row0 >> 5);
                if (in_w) in32[at] = in_w;
                if (amb_w) amb32[at] = amb_w;
            }
        }
    };

#define AC_PR_COMPUTE(B)                                                                                      \
    do {                                                                                                      \
        if (cur_grp == 0) {                                                                                   \
            _Pragma("unroll") for (int jj = 0; jj < NJ; ++jj)                                                 \
                _Pragma("unroll") for (int r = 0; r < 16; ++r) acc[jj][r] = 0.f;                              \
        }                                                                                                     \
        const ru32x4* qsrc_ = Qs + (size_t)cur_grp * (GK * NJ * 64) + lane;                                    \
        ru32x4 bq_[NJ];                                                                                        \
        _Pragma("unroll") for (int jj = 0; jj < NJ; ++jj) bq_[jj] = qsrc_[jj * 64];                           \
        _Pragma("unroll") for (int u = 0; u < GK; ++u) {                                                      \
            const rf16x8 a_ = __builtin_bit_cast(rf16x8, buf[B][u]);                                          \
            rf16x8 b_[NJ];                                                                                    \
            _Pragma("unroll") for (int jj = 0; jj < NJ; ++jj) b_[jj] = __builtin_bit_cast(rf16x8, bq_[jj]);   \
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
    // loads in flight (knn_plane_sweep: a load inside a branch makes hipcc wait on the buffer it has just issued).
    if (total > 0) {
        AC_PR_PREFETCH(0);
        AC_PR_PREFETCH(1);
        AC_PR_PREFETCH(2);
        for (int64_t gg = 0; gg < total; gg += NB) {      // (ngrp may be odd: the tile boundary falls anywhere in this body)
            AC_PR_PREFETCH(3);
            AC_PR_COMPUTE(0);
            AC_PR_PREFETCH(0);
            if (gg + 1 < total) AC_PR_COMPUTE(1);
            AC_PR_PREFETCH(1);
            if (gg + 2 < total) AC_PR_COMPUTE(2);
            AC_PR_PREFETCH(2);
            if (gg + 3 < total) AC_PR_COMPUTE(3);
        }
    }
#undef AC_PR_PREFETCH
#undef AC_PR_COMPUTE
}

// ---- host side ----
struct RangePlan {
    bool small;
    int Dp, ng, TQ, nqt;
    int64_t ntiles, W, S;
    size_t sweep_lds;
    size_t off_in, off_amb, off_cnt, off_off, total;
    double gamma;
};

// The layout depends on (N, D, nq) alone (count and fill plan it independently and must agree); the sweep's grid is chosen at launch.
int make_range_plan(int64_t N, int D, int nq, RangePlan* pl) {
    // accept / reject, error texts and the small-store verdict are the top-k planner's at k = 1 (the sweep keeps no lists, but a
    // (N, D) that one search takes the other takes too)
    ac::KnnSweepShape sh;
    const int rc = ac::knn_sweep_shape(N, D, nq, 1, &sh);
    if (rc != AC_OK) return rc;
    *pl = RangePlan{};
    pl->Dp = sh.Dp; pl->ng = sh.ng; pl->small = sh.small;
    pl->W = (N + 63) / 64;
    pl->S = pl->small ? pl->W : (pl->W + kStripWords - 1) / kStripWords;
    auto lds_for = [&](int TQ) { return ac::knn_query_tile_bytes(TQ, pl->ng) + (size_t)TQ * 28 + 64; };
    pl->TQ = (nq > 16 && lds_for(32) <= (size_t)kLdsLimit) ? 32 : 16;
    pl->sweep_lds = lds_for(pl->TQ);
    pl->nqt = nq > 0 ? (nq + pl->TQ - 1) / pl->TQ : 1;
    pl->ntiles = (N + kWaves * 16 - 1) / (kWaves * 16);
    pl->gamma = 1.02 * ac::knn_sweep_gamma0(pl->ng);
    const size_t nqs = (size_t)(nq > 0 ? nq : 1);
    ac::WsTake take;
    pl->off_in = take(nqs * pl->W * 8);
    pl->off_amb = take(pl->small ? 0 : nqs * pl->W * 8);
    pl->off_cnt = take(nqs * pl->S * 4);
    pl->off_off = take(nqs * pl->S * 8);
    pl->total = take.off > 256 ? take.off : 256;
    return AC_OK;
}

int range_validate(const RangePlan& pl, const float* d_P, int64_t N, int64_t ldP, int D, const float* d_Q, int64_t ldQ, void* d_ws,
                   size_t ws_bytes) {
    AC_REQUIRE(d_Q != nullptr, AC_EINVAL, "knn range: null pointer");
    AC_REQUIRE(ldQ >= D, AC_EINVAL, "knn range: ldQ=%lld < D=%d", (long long)ldQ, D);
    AC_REQUIRE(ws_bytes >= pl.total && d_ws, AC_EWORKSPACE, "knn range: workspace %zu < required %zu", ws_bytes, pl.total);
    return N > 0 ? ac::knn_check_store("knn range", d_P, ldP, pl.Dp) : AC_OK;
}

RangeParams range_params(const RangePlan& pl, const float* d_P, int64_t N, int64_t ldP, int D, const float* d_Q, int nq, int64_t ldQ,
                         char* ws, int32_t* d_stats) {
    RangeParams p{};
    p.P = d_P; p.N = N; p.ldP = ldP; p.Q = d_Q; p.ldQ = ldQ; p.D = D; p.Dp = pl.Dp; p.ng = pl.ng; p.nq = nq;
    p.nqt = pl.nqt; p.ntiles = pl.ntiles; p.W = pl.W; p.S = pl.S; p.gamma = pl.gamma;
    p.bm_in = (uint64_t*)(ws + pl.off_in); p.bm_amb = (uint64_t*)(ws + pl.off_amb);
    p.cnt = (int32_t*)(ws + pl.off_cnt); p.off = (int64_t*)(ws + pl.off_off);
    p.stats = d_stats;
    return p;
}

unsigned post_blocks(int64_t waves) { return (unsigned)((waves + kPostWaves - 1) / kPostWaves); }

// d_sel != NULL: the FILTERED search (ac_knn_*_range_count_sel) -- the same plan, workspace and launch sequence with the SEL
// instantiations of the sweep / the small-store kernel; resolve, scan and fill do not know about the selection
int range_count(bool ip, const float* d_P, int64_t N, int64_t ldP, int D, const float* d_Q, int nq, int64_t ldQ, const float* d_radius,
                int64_t* d_lims, void* d_ws, size_t ws_bytes, int32_t* d_stats, ac_stream_t stream_, const uint64_t* d_sel = nullptr,
                int64_t sel_bit0 = 0) {
    hipStream_t stream = (hipStream_t)stream_;
    RangePlan pl;
    int rc = make_range_plan(N, D, nq, &pl);
    if (rc != AC_OK) return rc;
    if (nq == 0) return AC_OK;
    AC_REQUIRE(d_radius && d_lims, AC_EINVAL, "knn range: null pointer");
    rc = range_validate(pl, d_P, N, ldP, D, d_Q, ldQ, d_ws, ws_bytes);
    if (rc != AC_OK) return rc;
    AC_REQUIRE((int64_t)nq * pl.S < 2147483647LL * kPostWaves, AC_EUNSUPPORTED, "knn range: nq=%d x %lld strips exceeds one launch", nq,
               (long long)pl.S);
    char* ws = (char*)d_ws;
    if (d_stats) AC_HIP_CHECK(hipMemsetAsync(d_stats, 0, 4 * sizeof(int32_t), stream));
    if (N == 0) {
        AC_HIP_CHECK(hipMemsetAsync(d_lims, 0, ((size_t)nq + 1) * 8, stream));
        return AC_OK;
    }
    RangeParamsSel p{};                               // (the plain kernels take its RangeParams base)
    static_cast<RangeParams&>(p) = range_params(pl, d_P, N, ldP, D, d_Q, nq, ldQ, ws, d_stats);
    p.radius = d_radius;
    p.sel = d_sel; p.sel_bit0 = sel_bit0;
    if (pl.small) {
        if (d_sel) {
            void (*fn)(RangeParamsSel) = ip ? knn_range_small<true, true> : knn_range_small<false, true>;
            hipLaunchKernelGGL(fn, dim3(post_blocks((int64_t)nq * pl.W)), dim3(kPostWaves * 64), 0, stream, p);
        } else {
            void (*fn)(RangeParams) = ip ? knn_range_small<true> : knn_range_small<false>;
            hipLaunchKernelGGL(fn, dim3(post_blocks((int64_t)nq * pl.W)), dim3(kPostWaves * 64), 0, stream, static_cast<RangeParams&>(p));
        }
        AC_LAUNCH_CHECK();
    } else {
        // both bitmaps start at zero (they are adjacent): the sweep stores non-zero pieces only
        AC_HIP_CHECK(hipMemsetAsync(ws + pl.off_in, 0, pl.off_cnt - pl.off_in, stream));
        void (*sweep_fn)(RangeParams) = nullptr;
        void (*sweep_sel_fn)(RangeParamsSel) = nullptr;      // FILTERED search: the SEL instantiation of the same sweep
        if (d_sel) {
            if (pl.TQ == 32) sweep_sel_fn = ip ? knn_range_sweep<2, true, true> : knn_range_sweep<2, false, true>;
            else sweep_sel_fn = ip ? knn_range_sweep<1, true, true> : knn_range_sweep<1, false, true>;
        } else {
            if (pl.TQ == 32) sweep_fn = ip ? knn_range_sweep<2, true> : knn_range_sweep<2, false>;
            else sweep_fn = ip ? knn_range_sweep<1, true> : knn_range_sweep<1, false>;
        }
        const void* kfn = d_sel ? (const void*)sweep_sel_fn : (const void*)sweep_fn;
        AC_HIP_CHECK(hipFuncSetAttribute(kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pl.sweep_lds));
        const int64_t G = ac::knn_residency_groups(kfn, pl.sweep_lds, pl.nqt, pl.ntiles);
        p.G = (int)G;
        p.zeros = ac::knn_zeros_device();
        if (d_sel) hipLaunchKernelGGL(sweep_sel_fn, dim3((unsigned)(G * pl.nqt)), dim3(kThreads), pl.sweep_lds, stream, p);
        else hipLaunchKernelGGL(sweep_fn, dim3((unsigned)(G * pl.nqt)), dim3(kThreads), pl.sweep_lds, stream, static_cast<RangeParams&>(p));
        AC_LAUNCH_CHECK();
        void (*res_fn)(RangeParams) = ip ? knn_range_resolve<true> : knn_range_resolve<false>;
        hipLaunchKernelGGL(res_fn, dim3(post_blocks((int64_t)nq * pl.S)), dim3(kPostWaves * 64), 0, stream, static_cast<RangeParams&>(p));
        AC_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(knn_range_scan, dim3(1), dim3(kScanThreads), 0, stream, (const int32_t*)p.cnt, p.off, d_lims, nq, pl.S);
    AC_LAUNCH_CHECK();
    return AC_OK;
}

int range_fill(bool ip, const float* d_P, int64_t N, int64_t ldP, int D, const float* d_Q, int nq, int64_t ldQ, int64_t row_offset,
               const int64_t* d_lims, int64_t capacity, float* d_outD, double* d_outD64, int64_t* d_outI, void* d_ws, size_t ws_bytes,
               int32_t* d_stats, ac_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    RangePlan pl;
    int rc = make_range_plan(N, D, nq, &pl);
    if (rc != AC_OK) return rc;
    if (nq == 0) return AC_OK;
    AC_REQUIRE(d_lims && capacity >= 0 && (capacity == 0 || (d_outD && d_outI)), AC_EINVAL, "knn range fill: null pointer");
    rc = range_validate(pl, d_P, N, ldP, D, d_Q, ldQ, d_ws, ws_bytes);
    if (rc != AC_OK) return rc;
    if (N == 0) {
        if (d_stats) AC_HIP_CHECK(hipMemsetAsync(d_stats + 1, 0, sizeof(int32_t), stream));
        return AC_OK;
    }
    RangeParams p = range_params(pl, d_P, N, ldP, D, d_Q, nq, ldQ, (char*)d_ws, d_stats);
    p.row_offset = row_offset; p.lims = const_cast<int64_t*>(d_lims); p.capacity = capacity;
    p.outD = d_outD; p.outD64 = d_outD64; p.outI = d_outI;
    void (*fn)(RangeParams);
    if (pl.small) fn = ip ? knn_range_fill<true, true> : knn_range_fill<false, true>;
    else fn = ip ? knn_range_fill<true, false> : knn_range_fill<false, false>;
    hipLaunchKernelGGL(fn, dim3(post_blocks((int64_t)nq * pl.S)), dim3(kPostWaves * 64), 0, stream, p);
    AC_LAUNCH_CHECK();
    return AC_OK;
}

// FILTERED range search, bitmap route: the argument checks return before any HIP call
int range_count_sel(bool ip, const float* d_P, int64_t N, int64_t ldP, int D, const float* d_Q, int nq, int64_t ldQ, const float* d_radius,
                    const uint64_t* d_sel, int64_t sel_bit0, int64_t* d_lims, void* d_ws, size_t ws_bytes, int32_t* d_stats,
                    ac_stream_t stream) {
    AC_REQUIRE(sel_bit0 >= 0, AC_EINVAL, "knn range sel: sel_bit0=%lld must be >= 0", (long long)sel_bit0);
    AC_REQUIRE(d_sel != nullptr || N <= 0, AC_EINVAL, "knn range sel: d_sel is NULL");
    AC_REQUIRE((((uintptr_t)d_sel) & 7) == 0, AC_EINVAL, "knn range sel: d_sel must be 8-byte aligned");
    return range_count(ip, d_P, N, ldP, D, d_Q, nq, ldQ, d_radius, d_lims, d_ws, ws_bytes, d_stats, stream, N > 0 ? d_sel : nullptr,
                       sel_bit0);
}

// ---- the count over the PREPARED store's fp16 plane (ac_knn_*_range_count_batch[_sel]) ----
constexpr int64_t kPlaneRangeMinRows = 65536;         // the limit of ac_knn_*_topk_batch

struct PlaneRangePlan {
    RangePlan rp;             // the fp32 route's plan: the workspace PREFIX (bm_in, bm_amb, cnt, off) is exactly its layout
    int TQ, nqt, Kp;
    int64_t ntiles, q_rows;   // 256-row tiles of the plane; rows of the padded query plane
    size_t lds;
    size_t off_qp, off_qfac, off_thr, off_tin, off_tout, off_live, total;
};

// host only (the workspace planner runs without a device); the grid is chosen at launch
int make_plane_range_plan(int64_t N, int D, int nq, PlaneRangePlan* pl) {
    *pl = PlaneRangePlan{};
    const int rc = make_range_plan(N, D, nq, &pl->rp);                 // validates (N, D, nq); refuses a D the range search does not take
    if (rc != AC_OK) return rc;
    AC_REQUIRE(N >= kPlaneRangeMinRows && N < 2147483647LL - 512 && !pl->rp.small, AC_EUNSUPPORTED,
               "knn range batch: N=%lld outside [%lld, 2^31 - 512): use ac_knn_*_range_count", (long long)N, (long long)kPlaneRangeMinRows);
    pl->Kp = (D + 63) / 64 * 64;
    auto lds_for = [&](int TQ) { return (size_t)(pl->Kp / 16) * (TQ / 32) * 1024; };
    pl->TQ = (nq > 32 && lds_for(64) <= (size_t)kLdsLimit) ? 64 : 32;
    AC_REQUIRE(lds_for(pl->TQ) <= (size_t)kLdsLimit, AC_EUNSUPPORTED, "knn range batch: D=%d: a 32-query tile of the plane exceeds LDS", D);
    pl->lds = lds_for(pl->TQ);
    pl->nqt = nq > 0 ? (nq + pl->TQ - 1) / pl->TQ : 1;
    pl->ntiles = (N + 255) / 256;
    pl->q_rows = ((int64_t)(nq > 0 ? nq : 1) + 255) / 256 * 256;
    ac::WsTake take;
    take.off = ac::align_up(pl->rp.total, 256);
    pl->off_qp = take(ac::knn_planes_bytes(nq > 0 ? nq : 1, D));
    pl->off_qfac = take((size_t)pl->q_rows * 4);
    pl->off_thr = take((size_t)pl->q_rows * 4);                        // knn_prepare_queries' top-k threshold: written, not read
    pl->off_tin = take((size_t)pl->q_rows * 4);
    pl->off_tout = take((size_t)pl->q_rows * 4);
    pl->off_live = take((size_t)pl->q_rows * 4);
    pl->total = take.off;
    return AC_OK;
}

// has_sel: the FILTERED form.  Every argument check returns before any HIP call.
int range_count_batch(bool ip, const float* d_P, int64_t N, int64_t ldP, int D, const uint16_t* d_planes, const float* d_norms,
                      const float* d_Q, int nq, int64_t ldQ, const float* d_radius, bool has_sel, const uint64_t* d_sel, int64_t sel_bit0,
                      int64_t* d_lims, void* d_ws, size_t ws_bytes, int32_t* d_stats, ac_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (has_sel) {
        AC_REQUIRE(sel_bit0 >= 0, AC_EINVAL, "knn range batch sel: sel_bit0=%lld must be >= 0", (long long)sel_bit0);
        AC_REQUIRE(d_sel != nullptr || N <= 0, AC_EINVAL, "knn range batch sel: d_sel is NULL");
        AC_REQUIRE((((uintptr_t)d_sel) & 7) == 0, AC_EINVAL, "knn range batch sel: d_sel must be 8-byte aligned");
    }
    PlaneRangePlan pl;
    int rc = make_plane_range_plan(N, D, nq, &pl);
    if (rc != AC_OK) return rc;
    if (nq == 0) return AC_OK;
    AC_REQUIRE(d_planes != nullptr, AC_EINVAL, "knn range batch: d_planes is NULL");
    AC_REQUIRE(d_norms != nullptr, AC_EINVAL, "knn range batch: d_norms is NULL");
    AC_REQUIRE(d_P != nullptr, AC_EINVAL, "knn range batch: d_P is NULL");
    AC_REQUIRE(d_Q && d_radius && d_lims, AC_EINVAL, "knn range batch: null pointer");
    AC_REQUIRE((((uintptr_t)d_planes) & 15) == 0 && (((uintptr_t)d_norms) & 15) == 0, AC_EINVAL,
               "knn range batch: d_planes / d_norms must be 16-byte aligned");
    AC_REQUIRE(ldQ >= D && ldP >= pl.rp.Dp && (ldP % 4) == 0 && (((uintptr_t)d_P) & 15) == 0, AC_EINVAL,
               "knn range batch: bad leading dimension / alignment (ldP=%lld, ldQ=%lld, d_P)", (long long)ldP, (long long)ldQ);
    AC_REQUIRE(d_ws && ws_bytes >= pl.total, AC_EWORKSPACE, "knn range batch: workspace %zu < required %zu", ws_bytes, pl.total);
    AC_REQUIRE((int64_t)nq * pl.rp.S < 2147483647LL * kPostWaves, AC_EUNSUPPORTED, "knn range batch: nq=%d x %lld strips exceeds one launch",
               nq, (long long)pl.rp.S);
    char* ws = (char*)d_ws;
    if (d_stats) AC_HIP_CHECK(hipMemsetAsync(d_stats, 0, 4 * sizeof(int32_t), stream));
    const int64_t np = (N + 255) / 256 * 256;
    const float* d_maxnorm = d_norms + np;                             // the store maximum |p|^2 (it only ever grows)
    const double gamma_b = ac::knn_batch_gamma(D);
    // 1. the queries' fp16 plane and epilogue factors: the kernel, scaling and rounding of the top-k search over the plane, hence
    //    its bound; then the two thresholds of every query
    rc = ac::knn_prepare_queries(nullptr, 1, d_Q, ldQ, D, nq, reinterpret_cast<const uint32_t*>(d_maxnorm), gamma_b,
                                 (uint16_t*)(ws + pl.off_qp), (float*)(ws + pl.off_thr), (float*)(ws + pl.off_qfac), stream);
    if (rc != AC_OK) return rc;
    void (*thr_fn)(const float*, int64_t, int, int, int64_t, const float*, const float*, double, float*, float*, int32_t*) =
        ip ? knn_plane_range_thresholds<true> : knn_plane_range_thresholds<false>;
    hipLaunchKernelGGL(thr_fn, dim3(post_blocks(pl.q_rows)), dim3(kPostWaves * 64), 0, stream, d_Q, ldQ, D, nq, pl.q_rows, d_radius, d_maxnorm,
                       1.02 * gamma_b, (float*)(ws + pl.off_tin), (float*)(ws + pl.off_tout), (int32_t*)(ws + pl.off_live));
    AC_LAUNCH_CHECK();
    // 2. both bitmaps start at zero (they are adjacent): the sweep stores non-zero pieces only
    AC_HIP_CHECK(hipMemsetAsync(ws + pl.rp.off_in, 0, pl.rp.off_cnt - pl.rp.off_in, stream));
    // 3. one pass over the plane per query tile: one 8-wave workgroup per CU, one residency round
    PlaneRangeParamsSel sp{};                          // (the plain kernels take its PlaneRangeParams base)
    sp.Pp = d_planes; sp.pnorm = d_norms; sp.Qp = (const uint16_t*)(ws + pl.off_qp); sp.q_rows = pl.q_rows;
    sp.qfac = (const float*)(ws + pl.off_qfac); sp.thr_in = (const float*)(ws + pl.off_tin); sp.thr_out = (const float*)(ws + pl.off_tout);
    sp.live = (const int32_t*)(ws + pl.off_live); sp.N = N; sp.ntiles = pl.ntiles; sp.W = pl.rp.W;
    sp.bm_in = (uint64_t*)(ws + pl.rp.off_in); sp.bm_amb = (uint64_t*)(ws + pl.rp.off_amb);
    sp.Kp = pl.Kp; sp.nq = nq;
    int64_t G = ac::dev_info().cus;
    if (G > pl.ntiles) G = pl.ntiles;
    sp.G = (int)G;
    sp.sel = d_sel; sp.sel_bit0 = sel_bit0;
    for (int qt = 0; qt < pl.nqt; ++qt) {
        sp.q0 = qt * pl.TQ;
        sp.stats = qt == 0 ? d_stats : nullptr;
        if (has_sel) {
            void (*fn)(PlaneRangeParamsSel);
            if (pl.TQ == 64) fn = ip ? knn_plane_range<64, true, true> : knn_plane_range<64, false, true>;
            else fn = ip ? knn_plane_range<32, true, true> : knn_plane_range<32, false, true>;
            AC_HIP_CHECK(hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pl.lds));
            hipLaunchKernelGGL(fn, dim3(sp.G), dim3(kThreads), pl.lds, stream, sp);
        } else {
            void (*fn)(PlaneRangeParams);
            if (pl.TQ == 64) fn = ip ? knn_plane_range<64, true> : knn_plane_range<64, false>;
            else fn = ip ? knn_plane_range<32, true> : knn_plane_range<32, false>;
            AC_HIP_CHECK(hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pl.lds));
            hipLaunchKernelGGL(fn, dim3(sp.G), dim3(kThreads), pl.lds, stream, static_cast<PlaneRangeParams&>(sp));
        }
        AC_LAUNCH_CHECK();
    }
    // 4. the fp32 route's tail, unchanged: the ambiguous pairs decided from the fp32 rows, the strip counts scanned into lims
    RangeParams p = range_params(pl.rp, d_P, N, ldP, D, d_Q, nq, ldQ, ws, d_stats);
    p.radius = d_radius;
    void (*res_fn)(RangeParams) = ip ? knn_range_resolve<true> : knn_range_resolve<false>;
    hipLaunchKernelGGL(res_fn, dim3(post_blocks((int64_t)nq * pl.rp.S)), dim3(kPostWaves * 64), 0, stream, p);
    AC_LAUNCH_CHECK();
    hipLaunchKernelGGL(knn_range_scan, dim3(1), dim3(kScanThreads), 0, stream, (const int32_t*)p.cnt, p.off, d_lims, nq, pl.rp.S);
    AC_LAUNCH_CHECK();
    return AC_OK;
}

// ---- id-list route ----
struct RangeIdsPlan {
    bool lane_order;      // the summation order of the bitmap route's small-store kernel (else the wave order)
    int Dp;
    int64_t W;            // words (= strips) per query: max(ceil(M / 64), 1)
    size_t off_in, off_cnt, off_off, total;
};

void range_ids_layout(int64_t M, int nq, RangeIdsPlan* pl) {
    pl->W = M > 64 ? (M + 63) / 64 : 1;
    const size_t n = (size_t)(nq > 0 ? nq : 1) * (size_t)pl->W;
    ac::WsTake take;
    pl->off_in = take(n * 8);
    pl->off_cnt = take(n * 4);
    pl->off_off = take(n * 8);
    pl->total = take.off;
}

// argument checks (before any device work) and the plan; the layout depends on (M, nq) alone
int make_range_ids_plan(const float* d_P, int64_t N, int64_t ldP, int D, const int64_t* d_ids, int64_t M, const float* d_Q, int nq,
                        int64_t ldQ, void* d_ws, size_t ws_bytes, RangeIdsPlan* pl) {
    AC_REQUIRE(M >= 0 && M <= ac::kKnnSmallN, AC_EINVAL, "knn range ids: M=%lld outside [0, %d]", (long long)M, ac::kKnnSmallN);
    AC_REQUIRE(d_ids != nullptr || M == 0, AC_EINVAL, "knn range ids: d_ids is NULL");
    AC_REQUIRE(N >= 0 && N < 2147483647LL, AC_EINVAL, "knn range ids: N=%lld out of range", (long long)N);
    AC_REQUIRE(D >= 1 && nq >= 0, AC_EINVAL, "knn range ids: bad D=%d nq=%d", D, nq);
    *pl = RangeIdsPlan{};
    range_ids_layout(M, nq, pl);
    pl->Dp = (D + 3) / 4 * 4;
    if (nq == 0) return AC_OK;
    AC_REQUIRE(d_Q != nullptr, AC_EINVAL, "knn range ids: null pointer");
    AC_REQUIRE(ldQ >= D, AC_EINVAL, "knn range ids: ldQ=%lld < D=%d", (long long)ldQ, D);
    AC_REQUIRE(ws_bytes >= pl->total && d_ws, AC_EWORKSPACE, "knn range ids: workspace %zu < required %zu", ws_bytes, pl->total);
    if (N > 0 && M > 0) {
        const int rc = ac::knn_check_store("knn range ids", d_P, ldP, pl->Dp);
        if (rc != AC_OK) return rc;
    }
    // the order in which the bitmap route sums this store's exact values: its small-store kernel's iff that route takes it
    // (a D beyond the sweep and N <= 8192); a store that route refuses is summed in the wave order
    ac::KnnSweepShape sh;
    pl->lane_order = ac::knn_sweep_shape(N, D, nq, 1, &sh) == AC_OK && sh.small;
    return AC_OK;
}

RangeParamsIds range_ids_params(const RangeIdsPlan& pl, const float* d_P, int64_t N, int64_t ldP, int D, const int64_t* d_ids, int64_t M,
                                const float* d_Q, int nq, int64_t ldQ, char* ws, int32_t* d_stats) {
    RangeParamsIds p{};
    p.P = d_P; p.N = N; p.ldP = ldP; p.Q = d_Q; p.ldQ = ldQ; p.D = D; p.Dp = pl.Dp; p.nq = nq;
    p.W = pl.W; p.S = pl.W;
    p.bm_in = (uint64_t*)(ws + pl.off_in); p.cnt = (int32_t*)(ws + pl.off_cnt); p.off = (int64_t*)(ws + pl.off_off);
    p.stats = d_stats;
    p.ids = d_ids; p.M = M;
    return p;
}

int range_count_ids(bool ip, const float* d_P, int64_t N, int64_t ldP, int D, const int64_t* d_ids, int64_t M, const float* d_Q, int nq,
                    int64_t ldQ, const float* d_radius, int64_t* d_lims, void* d_ws, size_t ws_bytes, int32_t* d_stats,
                    ac_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    RangeIdsPlan pl;
    const int rc = make_range_ids_plan(d_P, N, ldP, D, d_ids, M, d_Q, nq, ldQ, d_ws, ws_bytes, &pl);
    if (rc != AC_OK) return rc;
    if (nq == 0) return AC_OK;
    AC_REQUIRE(d_radius && d_lims, AC_EINVAL, "knn range ids: null pointer");
    if (d_stats) AC_HIP_CHECK(hipMemsetAsync(d_stats, 0, 4 * sizeof(int32_t), stream));
    if (N == 0 || M == 0) {
        AC_HIP_CHECK(hipMemsetAsync(d_lims, 0, ((size_t)nq + 1) * 8, stream));
        return AC_OK;
    }
    RangeParamsIds p = range_ids_params(pl, d_P, N, ldP, D, d_ids, M, d_Q, nq, ldQ, (char*)d_ws, d_stats);
    p.radius = d_radius;
    void (*fn)(RangeParamsIds);
    if (pl.lane_order) fn = ip ? knn_range_ids_count<true, true> : knn_range_ids_count<false, true>;
    else fn = ip ? knn_range_ids_count<true, false> : knn_range_ids_count<false, false>;
    hipLaunchKernelGGL(fn, dim3(post_blocks((int64_t)nq * pl.W)), dim3(kPostWaves * 64), 0, stream, p);
    AC_LAUNCH_CHECK();
    hipLaunchKernelGGL(knn_range_scan, dim3(1), dim3(kScanThreads), 0, stream, (const int32_t*)p.cnt, p.off, d_lims, nq, pl.W);
    AC_LAUNCH_CHECK();
    return AC_OK;
}

int range_fill_ids(bool ip, const float* d_P, int64_t N, int64_t ldP, int D, const int64_t* d_ids, int64_t M, const float* d_Q, int nq,
                   int64_t ldQ, int64_t row_offset, const int64_t* d_lims, int64_t capacity, float* d_outD, double* d_outD64,
                   int64_t* d_outI, void* d_ws, size_t ws_bytes, int32_t* d_stats, ac_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    RangeIdsPlan pl;
    const int rc = make_range_ids_plan(d_P, N, ldP, D, d_ids, M, d_Q, nq, ldQ, d_ws, ws_bytes, &pl);
    if (rc != AC_OK) return rc;
    if (nq == 0) return AC_OK;
    AC_REQUIRE(d_lims && capacity >= 0 && (capacity == 0 || (d_outD && d_outI)), AC_EINVAL, "knn range ids fill: null pointer");
    if (N == 0 || M == 0) {
        if (d_stats) AC_HIP_CHECK(hipMemsetAsync(d_stats + 1, 0, sizeof(int32_t), stream));
        return AC_OK;
    }
    RangeParamsIds p = range_ids_params(pl, d_P, N, ldP, D, d_ids, M, d_Q, nq, ldQ, (char*)d_ws, d_stats);
    p.row_offset = row_offset; p.lims = const_cast<int64_t*>(d_lims); p.capacity = capacity;
    p.outD = d_outD; p.outD64 = d_outD64; p.outI = d_outI;
    void (*fn)(RangeParamsIds);
    if (pl.lane_order) fn = ip ? knn_range_ids_fill<true, true> : knn_range_ids_fill<false, true>;
    else fn = ip ? knn_range_ids_fill<true, false> : knn_range_ids_fill<false, false>;
    hipLaunchKernelGGL(fn, dim3(post_blocks((int64_t)nq * pl.W)), dim3(kPostWaves * 64), 0, stream, p);
    AC_LAUNCH_CHECK();
    return AC_OK;
}

}  // namespace

extern "C" int ac_knn_l2_range_count_sel(const float* d_P, int64_t N, int64_t ldP, int D, const float* d_Q, int nq, int64_t ldQ,
                                         const float* d_radius, const uint64_t* d_sel, int64_t sel_bit0, int64_t* d_lims, void* d_ws,
                                         size_t ws_bytes, int32_t* d_stats, ac_stream_t stream) {
    return range_count_sel(false, d_P, N, ldP, D, d_Q, nq, ldQ, d_radius, d_sel, sel_bit0, d_lims, d_ws, ws_bytes, d_stats, stream);
}

extern "C" int ac_knn_ip_range_count_sel(const float* d_P, int64_t N, int64_t ldP, int D, const float* d_Q, int nq, int64_t ldQ,
                                         const float* d_radius, const uint64_t* d_sel, int64_t sel_bit0, int64_t* d_lims, void* d_ws,
                                         size_t ws_bytes, int32_t* d_stats, ac_stream_t stream) {
    return range_count_sel(true, d_P, N, ldP, D, d_Q, nq, ldQ, d_radius, d_sel, sel_bit0, d_lims, d_ws, ws_bytes, d_stats, stream);
}

extern "C" int ac_knn_range_batch_workspace(int64_t N, int D, int nq, size_t* bytes) {
    AC_REQUIRE(bytes != nullptr, AC_EINVAL, "knn range batch workspace: bytes is NULL");
    PlaneRangePlan pl;
    const int rc = make_plane_range_plan(N, D, nq, &pl);
    if (rc != AC_OK) return rc;
    *bytes = pl.total;
    return AC_OK;
}

extern "C" int ac_knn_l2_range_count_batch(const float* d_P, int64_t N, int64_t ldP, int D, const uint16_t* d_planes, const float* d_norms,
                                           const float* d_Q, int nq, int64_t ldQ, const float* d_radius, int64_t* d_lims, void* d_ws,
                                           size_t ws_bytes, int32_t* d_stats, ac_stream_t stream) {
    return range_count_batch(false, d_P, N, ldP, D, d_planes, d_norms, d_Q, nq, ldQ, d_radius, false, nullptr, 0, d_lims, d_ws, ws_bytes,
                             d_stats, stream);
}

extern "C" int ac_knn_ip_range_count_batch(const float* d_P, int64_t N, int64_t ldP, int D, const uint16_t* d_planes, const float* d_norms,
                                           const float* d_Q, int nq, int64_t ldQ, const float* d_radius, int64_t* d_lims, void* d_ws,
                                           size_t ws_bytes, int32_t* d_stats, ac_stream_t stream) {
    return range_count_batch(true, d_P, N, ldP, D, d_planes, d_norms, d_Q, nq, ldQ, d_radius, false, nullptr, 0, d_lims, d_ws, ws_bytes,
                             d_stats, stream);
}

extern "C" int ac_knn_l2_range_count_batch_sel(const float* d_P, int64_t N, int64_t ldP, int D, const uint16_t* d_planes,
                                               const float* d_norms, const float* d_Q, int nq, int64_t ldQ, const float* d_radius,
                                               const uint64_t* d_sel, int64_t sel_bit0, int64_t* d_lims, void* d_ws, size_t ws_bytes,
                                               int32_t* d_stats, ac_stream_t stream) {
    return range_count_batch(false, d_P, N, ldP, D, d_planes, d_norms, d_Q, nq, ldQ, d_radius, true, d_sel, sel_bit0, d_lims, d_ws, ws_bytes,
                             d_stats, stream);
}

extern "C" int ac_knn_ip_range_count_batch_sel(const float* d_P, int64_t N, int64_t ldP, int D, const uint16_t* d_planes,
                                               const float* d_norms, const float* d_Q, int nq, int64_t ldQ, const float* d_radius,
                                               const uint64_t* d_sel, int64_t sel_bit0, int64_t* d_lims, void* d_ws, size_t ws_bytes,
                                               int32_t* d_stats, ac_stream_t stream) {
    return range_count_batch(true, d_P, N, ldP, D, d_planes, d_norms, d_Q, nq, ldQ, d_radius, true, d_sel, sel_bit0, d_lims, d_ws, ws_bytes,
                             d_stats, stream);
}

extern "C" int ac_knn_range_ids_workspace(int64_t M, int nq, size_t* bytes) {
    AC_REQUIRE(bytes != nullptr, AC_EINVAL, "knn range ids workspace: bytes is NULL");
    AC_REQUIRE(M >= 0 && M <= ac::kKnnSmallN, AC_EINVAL, "knn range ids: M=%lld outside [0, %d]", (long long)M, ac::kKnnSmallN);
    AC_REQUIRE(nq >= 0, AC_EINVAL, "knn range ids: bad nq=%d", nq);
    RangeIdsPlan pl{};
    range_ids_layout(M, nq, &pl);
    *bytes = pl.total;
    return AC_OK;
}

extern "C" int ac_knn_l2_range_count_ids(const float* d_P, int64_t N, int64_t ldP, int D, const int64_t* d_ids, int64_t M,
                                         const float* d_Q, int nq, int64_t ldQ, const float* d_radius, int64_t* d_lims, void* d_ws,
                                         size_t ws_bytes, int32_t* d_stats, ac_stream_t stream) {
    return range_count_ids(false, d_P, N, ldP, D, d_ids, M, d_Q, nq, ldQ, d_radius, d_lims, d_ws, ws_bytes, d_stats, stream);
}

extern "C" int ac_knn_l2_range_fill_ids(const float* d_P, int64_t N, int64_t ldP, int D, const int64_t* d_ids, int64_t M, const float* d_Q,
                                        int nq, int64_t ldQ, int64_t row_offset, const int64_t* d_lims, int64_t capacity, float* d_outD,
                                        double* d_outD64, int64_t* d_outI, void* d_ws, size_t ws_bytes, int32_t* d_stats,
                                        ac_stream_t stream) {
    return range_fill_ids(false, d_P, N, ldP, D, d_ids, M, d_Q, nq, ldQ, row_offset, d_lims, capacity, d_outD, d_outD64, d_outI, d_ws,
                          ws_bytes, d_stats, stream);
}

extern "C" int ac_knn_ip_range_count_ids(const float* d_P, int64_t N, int64_t ldP, int D, const int64_t* d_ids, int64_t M,
                                         const float* d_Q, int nq, int64_t ldQ, const float* d_radius, int64_t* d_lims, void* d_ws,
                                         size_t ws_bytes, int32_t* d_stats, ac_stream_t stream) {
    return range_count_ids(true, d_P, N, ldP, D, d_ids, M, d_Q, nq, ldQ, d_radius, d_lims, d_ws, ws_bytes, d_stats, stream);
}

extern "C" int ac_knn_ip_range_fill_ids(const float* d_P, int64_t N, int64_t ldP, int D, const int64_t* d_ids, int64_t M, const float* d_Q,
                                        int nq, int64_t ldQ, int64_t row_offset, const int64_t* d_lims, int64_t capacity, float* d_outD,
                                        double* d_outD64, int64_t* d_outI, void* d_ws, size_t ws_bytes, int32_t* d_stats,
                                        ac_stream_t stream) {
    return range_fill_ids(true, d_P, N, ldP, D, d_ids, M, d_Q, nq, ldQ, row_offset, d_lims, capacity, d_outD, d_outD64, d_outI, d_ws,
                          ws_bytes, d_stats, stream);
}

extern "C" int ac_knn_range_workspace(int64_t N, int D, int nq, size_t* bytes) {
    AC_REQUIRE(bytes != nullptr, AC_EINVAL, "knn range workspace: bytes is NULL");
    RangePlan pl;
    const int rc = make_range_plan(N, D, nq, &pl);
    if (rc != AC_OK) return rc;
    *bytes = pl.total;
    return AC_OK;
}

extern "C" int ac_knn_l2_range_count(const float* d_P, int64_t N, int64_t ldP, int D, const float* d_Q, int nq, int64_t ldQ,
                                     const float* d_radius, int64_t* d_lims, void* d_ws, size_t ws_bytes, int32_t* d_stats,
                                     ac_stream_t stream) {
    return range_count(false, d_P, N, ldP, D, d_Q, nq, ldQ, d_radius, d_lims, d_ws, ws_bytes, d_stats, stream);
}

extern "C" int ac_knn_l2_range_fill(const float* d_P, int64_t N, int64_t ldP, int D, const float* d_Q, int nq, int64_t ldQ,
                                    int64_t row_offset, const int64_t* d_lims, int64_t capacity, float* d_outD, double* d_outD64,
                                    int64_t* d_outI, void* d_ws, size_t ws_bytes, int32_t* d_stats, ac_stream_t stream) {
    return range_fill(false, d_P, N, ldP, D, d_Q, nq, ldQ, row_offset, d_lims, capacity, d_outD, d_outD64, d_outI, d_ws, ws_bytes, d_stats,
                      stream);
}

extern "C" int ac_knn_ip_range_count(const float* d_P, int64_t N, int64_t ldP, int D, const float* d_Q, int nq, int64_t ldQ,
                                     const float* d_radius, int64_t* d_lims, void* d_ws, size_t ws_bytes, int32_t* d_stats,
                                     ac_stream_t stream) {
    return range_count(true, d_P, N, ldP, D, d_Q, nq, ldQ, d_radius, d_lims, d_ws, ws_bytes, d_stats, stream);
}

extern "C" int ac_knn_ip_range_fill(const float* d_P, int64_t N, int64_t ldP, int D, const float* d_Q, int nq, int64_t ldQ,
                                    int64_t row_offset, const int64_t* d_lims, int64_t capacity, float* d_outD, double* d_outD64,
                                    int64_t* d_outI, void* d_ws, size_t ws_bytes, int32_t* d_stats, ac_stream_t stream) {
    return range_fill(true, d_P, N, ldP, D, d_Q, nq, ldQ, row_offset, d_lims, capacity, d_outD, d_outD64, d_outI, d_ws, ws_bytes, d_stats,
                      stream);
}
