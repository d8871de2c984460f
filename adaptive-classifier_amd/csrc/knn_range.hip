// Exact range search (radius queries) over the flat store: faiss IndexFlatL2.range_search / IndexFlatIP.range_search.
//   ac_knn_{l2,ip}_range_count   membership of every (query, row) pair as a bitmap, per-query totals -> lims[nq + 1]
//   ac_knn_{l2,ip}_range_fill    the bitmap expanded by ascending row id to I, the exact value of every hit to D (and D64)
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
