// The exact stages every kNN route ends in.  The sweeps (knn_l2.hip: knn_sweep, knn_sweep_ring, knn_plane_sweep; knn_batch.hip:
// knn_batch_sweep) only PROPOSE candidates with a bounded error; what a search returns is decided here, on one stream and
// without host synchronisation:
//
//  1. knn_merge_rerank  per query: radix-select the k' best of the G per-block lists (or of one segmented candidate list),
//                     recompute those k' distances exactly (fp64 sum of (p-q)^2), order by (exact, id),
//                     emit top-k, and certify with an fp32 error bound that no unseen row can
//                     beat the k-th (see acamd.h "exactness contract").
//  2. knn_exact_fallback + knn_exact_fb_merge  only for queries whose certificate failed: a plain fp64
//                     sweep, parallel over row slabs.
//  3. knn_small_exact   stores of <= kKnnSmallN rows with a (k, D) outside the fused sweep: fp64 distances of every row, sorted.
//
// Every kernel is a template over the metric: IP = false squared L2, IP = true inner product (ac_knn_ip_topk).  Host side: the
// workspace plan of stages 1 - 2 (knn_exact_plan) and ONE driver that launches them (knn_exact_tail), used by the fp32, plane and
// batch routes alike; the shard merges and score utilities (ac_topk_merge*, ac_rows_to_class, ac_proto_scores) close the file.
#include "common.h"
#include "knn_stream.h"

#include <float.h>
#include <math.h>

namespace {

using ac::MergeParams;
using ac::SelArgs;
using ac::fkey;
using ac::fkey_inv;
using acknn::f32x4;
// the exact fp64 value of a (row, query) pair, defined once for every search (knn_stream.h)
using acknn::exact_term;
using acknn::exact_wave;
using acknn::exact_wave_sum;
using acknn::exact_lane;

// --------------------------------------------------------------------------------------
// merge + exact re-rank + certificate.  One block (256 threads) per query.
// --------------------------------------------------------------------------------------
// Inner-product search (ac_knn_ip_topk, template flag IP below): every stage after the sweep ranks by the exact KEY -(p.q),
// ascending, ties to the lower id -- the order the L2 stages already implement on their distances.  Negation is exact in fp32
// and fp64, so the key order is the descending order of p.q; none of the stages assumes a non-negative key (they compare
// doubles with `<` / `==`, and their padding, +inf with id 0x7fffffff, stays last).  The key is negated back once, where a
// result is written.
// one output slot: a hit (its exact key, local row id) or faiss-style padding -- (FLT_MAX, -1) for L2, (-FLT_MAX, -1) for IP
template <bool IP>
__device__ __forceinline__ void emit_hit(const MergeParams& prm, size_t at, bool real, double key, int64_t id) {
    const double v = IP ? -key : key;
    prm.outD[at] = real ? (float)v : (IP ? -FLT_MAX : FLT_MAX);
    if (prm.outD64) prm.outD64[at] = real ? v : (IP ? -(double)INFINITY : (double)INFINITY);
    prm.outI[at] = real ? id + prm.row_offset : -1;
}

// FILTERED search (acamd.h): SEL = true instantiations of the bodies below are the kernels *_sel; the plain kernels
// instantiate SEL = false, which compiles every selection statement away.
__device__ __forceinline__ bool row_selected(const SelArgs& sa, int64_t row) {
    const int64_t b = sa.sel_bit0 + row;
    return (sa.sel[b >> 6] >> (b & 63)) & 1ull;
}

constexpr int kMergeThreads = 256;

// Block-wide radix select (8 bits per round) over 32-bit keys held in LDS: returns the `want`-th
// smallest (1-based) among the entries with active(t) != 0.  On return *rank_in_ties is how many of
// the entries equal to the result are needed to reach `want`, *n_ties how many such entries exist.
template <typename KeyFn, typename ActiveFn>
__device__ __forceinline__ uint32_t block_radix_select(int n, int want, KeyFn key_of, ActiveFn active,
                                                       int* hist, int* bcast, int* rank_in_ties, int* n_ties) {
    const int tid = threadIdx.x;
    __shared__ int wave_tot[kMergeThreads / 64];
    uint32_t prefix = 0;
    for (int shift = 24; shift >= 0; shift -= 8) {
        hist[tid] = 0;                       // kMergeThreads == 256 bins
        __syncthreads();
        const uint32_t himask = shift == 24 ? 0u : (0xffffffffu << (shift + 8));
        // distances of one query's candidates share their leading bits, so in the first rounds nearly every key lands in
        // the same bin: run-length aggregation per thread (one LDS atomic per run instead of one per key)
        int run_bin = -1, run_cnt = 0;
        for (int t = tid; t < n; t += kMergeThreads) {
            if (!active(t)) continue;
            const uint32_t key = key_of(t);
            if ((key & himask) != (prefix & himask)) continue;
            const int bin = (int)((key >> shift) & 255u);
            if (bin == run_bin) { ++run_cnt; continue; }
            if (run_cnt) atomicAdd(&hist[run_bin], run_cnt);
            run_bin = bin; run_cnt = 1;
        }
        if (run_cnt) atomicAdd(&hist[run_bin], run_cnt);
        __syncthreads();
        // exclusive prefix of bin `tid`: wave scan + the totals of the waves below (kMergeThreads == 256 = 4 waves)
        const int mine_cnt = hist[tid];
        int c = mine_cnt;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const int v = __shfl_up(c, o); if ((tid & 63) >= o) c += v; }
        if ((tid & 63) == 63) wave_tot[tid >> 6] = c;
        __syncthreads();
        for (int w = 0; w < (tid >> 6); ++w) c += wave_tot[w];
        c -= mine_cnt;
        const int mine = hist[tid];
        if (c < want && want <= c + mine) { bcast[0] = tid; bcast[1] = want - c; bcast[2] = mine; }
        __syncthreads();
        prefix |= (uint32_t)bcast[0] << shift;
        want = bcast[1];
        *n_ties = bcast[2];
        __syncthreads();
    }
    *rank_in_ties = want;
    return prefix;
}

// (Each kernel below is a thin `template <bool IP> __global__` wrapper around a force-inlined body that takes the parameters by
//  reference: written straight into the kernel, hipcc schedules the same code differently.)
template <bool IP, bool SEL = false>
__device__ __forceinline__ void knn_merge_rerank_body(const MergeParams& prm, char* smem, const float* sel_thr = nullptr) {
    const int q = blockIdx.x;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int n = prm.cand_cnt ? prm.cand_cap : prm.G * prm.kp;
    const int kp = prm.kp;
    // candidate mode (knn_batch.hip): the list is cand_segs segments of segcap entries with a count each; the entries in use
    // are compacted into LDS (keys + ids), so the selection below walks the ~k' * stride real candidates, not the capacity
    const int segs = prm.cand_cnt ? prm.cand_segs : 1, segcap = n / segs;
    const bool cand = segs > 1;                            // (one segment: the list is walked in place, like the per-block lists)

    // LDS: keys[n] u32 | (cand) cid[n] i32 | qrow[Dp] f32 | sel[kp] u64 | exact[kp] f64 | hist[256] | misc
    uint32_t* keys = reinterpret_cast<uint32_t*>(smem);
    size_t off = ac::align_up((size_t)n * 4, 16);
    int32_t* cid = reinterpret_cast<int32_t*>(smem + off);
    if (cand) off += ac::align_up((size_t)n * 4, 16);
    float* qrow = reinterpret_cast<float*>(smem + off);
    off += ac::align_up((size_t)prm.Dp * 4, 16);
    unsigned long long* sel = reinterpret_cast<unsigned long long*>(smem + off);
    off += (size_t)kp * 8;
    double* exact = reinterpret_cast<double*>(smem + off);
    off += (size_t)kp * 8;
    int* hist = reinterpret_cast<int*>(smem + off);
    off += 256 * 4;
    int* misc = reinterpret_cast<int*>(smem + off);       // [0..2] radix broadcast, [4] nsel counter, [5] nreal, [6] segment overflow
    double* dmisc = reinterpret_cast<double*>(misc + 8);  // [0] qnorm2, [1] exact k-th

    const float* pd = prm.part_d + (size_t)q * n;
    const int32_t* pi = prm.part_i + (size_t)q * n;
    if (tid < 8) misc[tid] = 0;
    for (int c = tid; c < prm.Dp; c += kMergeThreads)
        qrow[c] = c < prm.D ? prm.Q[(size_t)q * prm.ldQ + c] : 0.f;
    int nkeys = n;                                         // key slots the selection walks
    if (cand) {
        // segment s holds min(count, segcap) entries; exclusive offsets by a block scan (segs <= 256 = one per thread)
        __shared__ int seg_off[kMergeThreads + 1];
        __shared__ int scan_tot[kMergeThreads / 64];
        const int raw = tid < segs ? prm.cand_cnt[(size_t)q * segs + tid] : 0;
        const int mine = raw < segcap ? raw : segcap;
        int c = mine;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const int v = __shfl_up(c, o); if (lane >= o) c += v; }
        if (lane == 63) scan_tot[wave] = c;
        __syncthreads();
        if (raw > segcap) misc[6] = 1;                     // (benign race: every writer stores 1)
        for (int w = 0; w < wave; ++w) c += scan_tot[w];
        seg_off[tid + 1] = c;
        if (tid == 0) seg_off[0] = 0;
        __syncthreads();
        nkeys = seg_off[kMergeThreads];
        for (int j = tid; j < nkeys; j += kMergeThreads) {
            int lo = 0, hi = segs;                         // largest s with seg_off[s] <= j
            while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (seg_off[mid] <= j) lo = mid; else hi = mid; }
            const int t = lo * segcap + (j - seg_off[lo]);
            keys[j] = fkey(pd[t]);
            cid[j] = pi[t];
        }
        if (tid == 0) misc[5] = nkeys;
        if (prm.cand_cnt_clear && tid < segs) prm.cand_cnt_clear[(size_t)q * segs + tid] = 0;       // (read above, before the barriers)
    } else {
        // monotone 32-bit key of the sweep value; padding (id < 0) and slots past the count sort last
        const int raw = prm.cand_cnt ? prm.cand_cnt[q] : n;
        const int nfill = raw < n ? raw : n;
        if (tid == 0 && raw > n) misc[6] = 1;
        int nreal_local = 0;
#pragma unroll 8
        for (int t = tid; t < n; t += kMergeThreads) {      // (unrolled: the loads of several candidates in flight)
            const bool real = t < nfill && pi[t] >= 0;
            keys[t] = real ? fkey(pd[t]) : 0xffffffffu;
            nreal_local += real ? 1 : 0;
        }
        __syncthreads();
        atomicAdd(&misc[5], nreal_local);
        if (prm.cand_cnt_clear && tid == 0) prm.cand_cnt_clear[q] = 0;
    }
    __syncthreads();
    const bool overflow = misc[6] != 0;
    const int nreal = misc[5];
    const int nsel = nreal < kp ? nreal : kp;     // how many candidates we re-rank
    auto id_of = [&](int t) -> int32_t { return cand ? cid[t] : pi[t]; };

    // ---- the nsel-th smallest sweep value T; ties at T are resolved by the lowest ids ----
    uint32_t T = 0xffffffffu;
    int32_t tie_id_max = 0x7fffffff;
    if (nsel > 0) {
        int r = 0, c_eq = 0;
        T = block_radix_select(nkeys, nsel, [&](int t) { return keys[t]; },
                               [&](int t) { return keys[t] != 0xffffffffu; }, hist, misc, &r, &c_eq);
        if (c_eq != r) {     // rare: several candidates share the boundary value -> r lowest ids of them
            int r2 = 0, c2 = 0;
            tie_id_max = (int32_t)block_radix_select(
                nkeys, r, [&](int t) { return (uint32_t)id_of(t); },
                [&](int t) { return keys[t] != 0xffffffffu && keys[t] == T; }, hist, misc, &r2, &c2);
        }
    }
    if (prm.thr_only) {
        if (tid == 0 && prm.thr_out && nreal >= kp && nsel > 0) {
            const float t = nextafterf(fkey_inv(T), INFINITY);
            if (t < prm.thr_out[q]) prm.thr_out[q] = t;
        }
        return;
    }
    // ---- compact the selected candidates ----
    for (int t = tid; t < nkeys; t += kMergeThreads) {
        const uint32_t key0 = keys[t];
        const int32_t id = key0 != 0xffffffffu ? id_of(t) : -1;
        if (nsel > 0 && id >= 0) {
            const uint32_t key = key0;
            if (key < T || (key == T && id <= tie_id_max)) {
                const int s = atomicAdd(&misc[4], 1);
                if (s < kp) sel[s] = ((unsigned long long)key << 32) | (uint32_t)id;
            }
        }
    }
    __syncthreads();
    const int ns = misc[4] < kp ? misc[4] : kp;
    const unsigned long long T64 = (unsigned long long)T << 32;

    // ---- exact fp64 distances of the selected rows; |q|^2 ----
    // Four rows per wave at a time: their loads are issued together, so a wave pays the (random-row, HBM) latency once per
    // group instead of once per row -- the per-row arithmetic (four accumulators over c4 = lane, lane + 64, ..., the
    // (a0 + a1) + (a2 + a3) fold, the xor-shuffle tree) is unchanged, hence the same bits.  (One row at a time this loop was
    // most of the kernel: ~20 of its 27 - 32 us.)
    const int nc4 = prm.Dp >> 2;
    constexpr int RU = 4;
    for (int s0 = wave * RU; s0 < ns; s0 += (kMergeThreads / 64) * RU) {
        const f32x4* prow[RU];
#pragma unroll
        for (int u = 0; u < RU; ++u) {
            const int s = s0 + u < ns ? s0 + u : s0;                  // (a short last group re-reads its first row)
            const int32_t id = (int32_t)(uint32_t)(sel[s] & 0xffffffffull);
            const int64_t prow_i = prm.run_stride ? (int64_t)(id >> 3) * prm.run_stride + (id & 7) : (int64_t)id;     // (threshold stages: sample row -> store row)
            prow[u] = reinterpret_cast<const f32x4*>(prm.P + (size_t)prow_i * prm.ldP);
        }
        double acc[RU][4];
#pragma unroll
        for (int u = 0; u < RU; ++u) { acc[u][0] = 0; acc[u][1] = 0; acc[u][2] = 0; acc[u][3] = 0; }
#pragma unroll 2
        for (int c4 = lane; c4 < nc4; c4 += 64) {
            f32x4 p[RU];
#pragma unroll
            for (int u = 0; u < RU; ++u) p[u] = prow[u][c4];
            const f32x4 qq = *reinterpret_cast<const f32x4*>(qrow + 4 * c4);
#pragma unroll
            for (int u = 0; u < RU; ++u) {
                acc[u][0] = exact_term<IP>(p[u].x, qq.x, acc[u][0]); acc[u][1] = exact_term<IP>(p[u].y, qq.y, acc[u][1]);
                acc[u][2] = exact_term<IP>(p[u].z, qq.z, acc[u][2]); acc[u][3] = exact_term<IP>(p[u].w, qq.w, acc[u][3]);
            }
        }
#pragma unroll
        for (int u = 0; u < RU; ++u) {
            const double a = exact_wave_sum(acc[u][0], acc[u][1], acc[u][2], acc[u][3]);
            if (lane == 0 && s0 + u < ns) exact[s0 + u] = IP ? -a : a;          // (inner product: the key -(p.q))
        }
    }
    if (wave == 0) {
        double a = 0;
        for (int c = lane; c < prm.Dp; c += 64) a = fma((double)qrow[c], (double)qrow[c], a);
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) a += __shfl_xor(a, o);
        if (lane == 0) { dmisc[0] = a; dmisc[1] = INFINITY; }
    }
    __syncthreads();

    // ---- final order by (exact, id); emit top-k ----
    const int kout = prm.k;
    for (int t = tid; t < ns; t += kMergeThreads) {
        const double dt = exact[t];
        const uint32_t it = (uint32_t)(sel[t] & 0xffffffffull);
        int rank = 0;
        for (int s = 0; s < ns; ++s) {
            const double ds = exact[s];
            const uint32_t is = (uint32_t)(sel[s] & 0xffffffffull);
            rank += (ds < dt || (ds == dt && is < it)) ? 1 : 0;
        }
        if (rank < kout) emit_hit<IP>(prm, (size_t)q * kout + rank, true, dt, (int64_t)it);
        if (rank == kout - 1) dmisc[1] = dt;
    }
    for (int t = ns + tid; t < kout; t += kMergeThreads)    // k > N: faiss-style padding
        emit_hit<IP>(prm, (size_t)q * kout + t, false, 0.0, -1);
    __syncthreads();

    // ---- certificate ----
    // largest row norm seen by the sweep: the per-block maxima reduced by the whole workgroup (a one-thread loop over up to
    // 512 global loads was most of this kernel's time for a single query)
    float mx_all = 0.f;
    for (int b = tid; b < prm.nblk; b += kMergeThreads) mx_all = fmaxf(mx_all, prm.part_maxnorm[b]);
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) mx_all = fmaxf(mx_all, __shfl_xor(mx_all, o));
    if (lane == 0) hist[wave] = (int)__float_as_uint(mx_all);           // (norms are non-negative: their bits order like the values)
    __syncthreads();
    if (tid == 0 && prm.thr_out) {
        // threshold stage: the k-th (= k'-th) exact distance of this sample bounds the store's k'-th smallest distance
        float mx = 0.f;
        for (int w = 0; w < kMergeThreads / 64; ++w) mx = fmaxf(mx, __uint_as_float((uint32_t)hist[w]));
        const double qn2 = dmisc[0], tau = dmisc[1];
        const double pn = sqrt((double)mx * 1.001), qn = sqrt(qn2);
        const double E = prm.gamma * (pn + qn) * (pn + qn) + 1e-30;
        // (inner product: tau is the k'-th smallest exact KEY -(p.q) of the sample; a row with key <= tau has -2 p.q = 2 key <= 2 tau,
        //  so its sweep value is <= 2 tau + E: at least k' rows of the store pass that threshold.  No |q|^2 term.)
        const double bound = IP ? 2.0 * tau + E : tau - qn2 + E;
        float t = (float)bound;
        if ((double)t < bound) t = nextafterf(t, INFINITY);
        // a stage that kept fewer than k' rows for this query has no k'-th distance to offer: the threshold of the stage before it
        // (still a valid bound) stays; a valid new bound only ever tightens it
        if (isfinite(tau) && ns >= kout && t < prm.thr_out[q]) prm.thr_out[q] = t;
    }
    if (tid == 0) {
        int ok = 1;
        if (prm.N > (int64_t)kp) {
            float mx = 0.f;
            for (int w = 0; w < kMergeThreads / 64; ++w) mx = fmaxf(mx, __uint_as_float((uint32_t)hist[w]));
            const double qn2 = dmisc[0];
            const double pn = sqrt((double)mx * 1.001), qn = sqrt(qn2);
            // fp32 fma-chain roundoff of |p|^2 - 2 q.p: every term passes through at most
            // nterms roundings, so |err| <= gamma_n * (|p|^2 + 2 sum|q_i p_i|) <= gamma_n (|p|+|q|)^2
            const double E = prm.gamma * (pn + qn) * (pn + qn) + 1e-30;
            const double a_last = (double)fkey_inv((uint32_t)(T64 >> 32));
            // every row that was NOT re-ranked has sweep value >= a_last, hence exact
            // distance >= a_last - E + |q|^2.  The k-th re-ranked must beat that strictly.
            const double kth = dmisc[1];
            if constexpr (IP) {
                // inner product: the sweep value is v = -2 (p.q)~, the same fma chain without the |p|^2 terms, so
                // |v - (-2 p.q)| <= gamma_n * 2 sum|q_i p_i| <= gamma_n * 2 |p||q| <= gamma_n (|p|max + |q|)^2 = E.  Every row that
                // was NOT re-ranked has v >= a_last, hence -2 p.q >= a_last - E, i.e. p.q <= -(a_last - E) / 2: its key -(p.q) is
                // >= (a_last - E) / 2 (halving is exact).  The k-th re-ranked key must lie strictly below that, i.e. the k-th exact
                // inner product strictly above every value an unseen row can have.
                ok = (ns >= kout) && (kth < 0.5 * (a_last - E)) && !overflow;
            } else {
                ok = (ns >= kout) && (kth < a_last - E + qn2) && !overflow;
            }
            if (prm.cand_cnt && nreal < kp) ok = 0;      // fewer than k' candidates kept: the "unseen rows >= a_last" premise is gone
            // FILTERED search over the per-block lists: a block that ever pruned keeps exactly k' entries, so fewer than k' real
            // entries IN TOTAL mean that no block pruned -- every list still holds every selected row of its block (tau stayed
            // +inf), all of them were re-ranked above, and the result is complete however few they are (padding included).
            if constexpr (SEL) { if (!prm.cand_cnt && nreal < kp && !overflow) ok = 1; }
            // FILTERED search in candidate-buffer mode (knn_merge_rerank_selc; sel_thr = the thresholds the main sweep used): a
            // sweep that ran with thr = +inf kept every selected row (v < +inf for every finite v; unselected rows carry +inf and
            // are never kept), so a list that did not overflow holds ALL of them, and with nreal <= k' all of them were re-ranked
            // above: complete, padding included.  A finite threshold or nreal > k' leaves the unfiltered rule as it is.
            // (Premise, shared with the per-block rule above: a selected row has a finite sweep value -- a row whose |p|^2
            //  overflows fp32 is kept by no sweep, filtered or not.)
            if constexpr (SEL) { if (sel_thr && prm.cand_cnt && nreal <= kp && !overflow && sel_thr[q] == INFINITY) ok = 1; }
        }
        int flag = 0;
        if (!ok) {
            const int slot = atomicAdd(prm.fb_slotctr, 1);
            flag = slot < prm.fb_F ? slot + 1 : -1;
            if (prm.stats) atomicAdd(&prm.stats[0], 1);
        }
        prm.flags[q] = flag;
    }
}
template <bool IP>
__global__ __launch_bounds__(kMergeThreads) void knn_merge_rerank(MergeParams prm) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    knn_merge_rerank_body<IP>(prm, smem);
}
template <bool IP>
__global__ __launch_bounds__(kMergeThreads) void knn_merge_rerank_sel(MergeParams prm) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    knn_merge_rerank_body<IP, true>(prm, smem);
}
template <bool IP>
__global__ __launch_bounds__(kMergeThreads) void knn_merge_rerank_selc(MergeParams prm, const float* sel_thr) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    knn_merge_rerank_body<IP, true>(prm, smem, sel_thr);
}

// --------------------------------------------------------------------------------------
// exact fallback: fp64 sweep for the (rare) queries whose certificate failed.
// One block per query; exits immediately unless flagged.
// --------------------------------------------------------------------------------------
constexpr int kFbThreads = 512;
constexpr int kFbWaves = kFbThreads / 64;
constexpr int kFbCap = 1024;          // list capacity (k <= 248 -> prune keeps k)
constexpr int kFbRound = 32;          // rows per wave between barriers

// grid = (fb_S, nq): block (s, q) scans row slab s of a flagged query and writes its exact top-k to the
// query's slot; knn_exact_fb_merge then merges the slabs.  A flagged query without a slot (more than fb_F
// failures in one call) is handled by its s == 0 block alone over the whole store.
// (round 6: the grid is (fb_S, min(nq, kFbQueryGroups)) and a block walks the queries q = blockIdx.y, + gridDim.y, ...: with
//  no query flagged -- every call of an ordinary batch -- dispatching fb_S x nq = 16 384 empty 512-thread blocks cost 8.5 us;
//  fb_S x 8 cost 2.  A device holds <= ~1000 of these blocks at once, so flagged batches lose nothing.)
constexpr int kFbQueryGroups = 8, kFbMergeGroups = 32;
template <bool IP, bool SEL = false>
__device__ __forceinline__ void knn_exact_fallback_query(const MergeParams& prm, const int q, const int slab, char* smem, const SelArgs* sa = nullptr) {
    const int flag = prm.flags[q];
    if (flag == 0 || (flag < 0 && slab != 0)) return;
    const bool direct = flag < 0;
    const int64_t row_lo = direct ? 0 : (prm.N * slab) / prm.fb_S;
    const int64_t row_hi = direct ? prm.N : (prm.N * (slab + 1)) / prm.fb_S;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double* ld = reinterpret_cast<double*>(smem);                  // [kFbCap]
    int32_t* li = reinterpret_cast<int32_t*>(ld + kFbCap);         // [kFbCap]
    float* qrow = reinterpret_cast<float*>(li + kFbCap);           // [Dp]
    int* misc = reinterpret_cast<int*>(qrow + ac::align_up((size_t)prm.Dp, 4));  // [0] cnt
    double* tau_d = reinterpret_cast<double*>(misc + 4);
    int32_t* tau_i = reinterpret_cast<int32_t*>(tau_d + 1);

    for (int c = tid; c < prm.Dp; c += kFbThreads)
        qrow[c] = c < prm.D ? prm.Q[(size_t)q * prm.ldQ + c] : 0.f;
    if (tid == 0) { misc[0] = 0; *tau_d = INFINITY; *tau_i = 0x7fffffff; }
    __syncthreads();
    const int nc4 = prm.Dp >> 2;
    const int k = prm.k;

    auto prune = [&]() {
        // block-wide rank-by-counting over cnt <= kFbCap entries (2 per thread)
        const int n = misc[0] < kFbCap ? misc[0] : kFbCap;
        double myd[2]; int32_t myi[2]; int rank[2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int s = tid + kFbThreads * e;
            myd[e] = s < n ? ld[s] : INFINITY;
            myi[e] = s < n ? li[s] : 0x7fffffff;
            rank[e] = 0;
        }
        for (int s = 0; s < n; ++s) {
            const double d = ld[s]; const int32_t i = li[s];
#pragma unroll
            for (int e = 0; e < 2; ++e) rank[e] += (d < myd[e] || (d == myd[e] && i < myi[e])) ? 1 : 0;
        }
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int s = tid + kFbThreads * e;
            if (s < n && rank[e] < k) {
                ld[rank[e]] = myd[e]; li[rank[e]] = myi[e];
                if (rank[e] == k - 1) { *tau_d = myd[e]; *tau_i = myi[e]; }
            }
        }
        if (tid == 0) misc[0] = n < k ? n : k;
        __syncthreads();
    };

    for (int64_t base = row_lo; base < row_hi; base += (int64_t)kFbWaves * kFbRound) {
        const double td = *tau_d; const int32_t ti = *tau_i;
        for (int m = 0; m < kFbRound; ++m) {
            const int64_t row = base + (int64_t)m * kFbWaves + wave;
            if (row >= row_hi) break;
            if constexpr (SEL) { if (!row_selected(*sa, row)) continue; }      // (wave-uniform: a wave scans one row)
            double a = exact_wave<IP>(prm.P + (size_t)row * prm.ldP, nc4, lane,
                                      [&](int c4) { return *reinterpret_cast<const f32x4*>(qrow + 4 * c4); });      // (the query sits in LDS, zero padded)
            if (IP) a = -a;                 // (inner product: the key -(p.q); the same bits knn_merge_rerank computes for this row)
            if (lane == 0 && (a < td || (a == td && (int32_t)row < ti))) {
                const int s = atomicAdd(&misc[0], 1);
                if (s < kFbCap) { ld[s] = a; li[s] = (int32_t)row; }
            }
        }
        __syncthreads();
        const int c_now = misc[0];      // read between two barriers: identical for every thread
        __syncthreads();
        if (c_now > kFbCap - kFbWaves * kFbRound) prune();
    }
    prune();
    const int n = misc[0];
    if (direct) {
        for (int t = tid; t < k; t += kFbThreads) emit_hit<IP>(prm, (size_t)q * k + t, t < n, ld[t], (int64_t)li[t]);    // (k <= kFbCap)
    } else {
        const size_t base = ((size_t)(flag - 1) * prm.fb_S + slab) * k;
        for (int t = tid; t < k; t += kFbThreads) {
            prm.fb_d[base + t] = t < n ? ld[t] : INFINITY;
            prm.fb_i[base + t] = t < n ? li[t] : 0x7fffffff;
        }
    }
}
template <bool IP>
__global__ __launch_bounds__(kFbThreads) void knn_exact_fallback(MergeParams prm, int nq) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    for (int q = blockIdx.y; q < nq; q += gridDim.y) {
        knn_exact_fallback_query<IP>(prm, q, blockIdx.x, smem);
        __syncthreads();                                            // (the next query reuses the lists)
    }
}
template <bool IP>
__global__ __launch_bounds__(kFbThreads) void knn_exact_fallback_sel(MergeParams prm, int nq, SelArgs sa) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    for (int q = blockIdx.y; q < nq; q += gridDim.y) {
        knn_exact_fallback_query<IP, true>(prm, q, blockIdx.x, smem, &sa);
        __syncthreads();
    }
}

// merge the fb_S slab results of a flagged query: bitonic sort of fb_S * k (<= 4096) exact entries
template <bool IP>
__device__ __forceinline__ void knn_exact_fb_merge_query(const MergeParams& prm, const int npow2, const int q, char* smem) {
    const int tid = threadIdx.x;
    const int flag = prm.flags[q];
    if (flag <= 0) return;
    double* ds = reinterpret_cast<double*>(smem);
    int32_t* is = reinterpret_cast<int32_t*>(ds + npow2);
    const int n = prm.fb_S * prm.k;
    const size_t base = (size_t)(flag - 1) * n;
    for (int t = tid; t < npow2; t += 256) {
        ds[t] = t < n ? prm.fb_d[base + t] : INFINITY;
        is[t] = t < n ? prm.fb_i[base + t] : 0x7fffffff;
    }
    __syncthreads();
    for (int size = 2; size <= npow2; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = tid; t < (npow2 >> 1); t += 256) {
                const int lo = 2 * t - (t & (stride - 1));
                const int hi = lo + stride;
                const bool asc = (lo & size) == 0;
                const double dl = ds[lo], dh = ds[hi];
                const int32_t il = is[lo], ih = is[hi];
                const bool gt = dl > dh || (dl == dh && il > ih);
                if (gt == asc) { ds[lo] = dh; ds[hi] = dl; is[lo] = ih; is[hi] = il; }
            }
            __syncthreads();
        }
    for (int t = tid; t < prm.k; t += 256) emit_hit<IP>(prm, (size_t)q * prm.k + t, is[t] != 0x7fffffff, ds[t], (int64_t)is[t]);
}
template <bool IP>
__global__ __launch_bounds__(256) void knn_exact_fb_merge(MergeParams prm, int npow2, int nq) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    for (int q = blockIdx.x; q < nq; q += gridDim.x) {
        knn_exact_fb_merge_query<IP>(prm, npow2, q, smem);
        __syncthreads();
    }
}

// --------------------------------------------------------------------------------------
// shard merge and prototype scores
// --------------------------------------------------------------------------------------
// DESC = the inner-product form: per-shard DESCENDING lists -> global top-k by (value descending, id ascending); padding
// (id < 0) comes out as (-FLT_MAX, -1).  Pure selection either way.
template <typename DT, bool DESC = false>
__global__ __launch_bounds__(256) void topk_merge_kernel(const DT* Din, const int64_t* Iin,
                                                         int shards, int nq, int k, float* outD,
                                                         int64_t* outI) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int q = blockIdx.x, tid = threadIdx.x;
    const int n = shards * k;
    int64_t* ids = reinterpret_cast<int64_t*>(smem);
    DT* ds = reinterpret_cast<DT*>(ids + n);
    for (int t = tid; t < n; t += 256) {
        const int s = t / k, e = t - s * k;
        ids[t] = Iin[((size_t)s * nq + q) * k + e];
        ds[t] = Din[((size_t)s * nq + q) * k + e];
    }
    for (int t = tid; t < k; t += 256) { outD[(size_t)q * k + t] = DESC ? -FLT_MAX : FLT_MAX; outI[(size_t)q * k + t] = -1; }
    __syncthreads();
    for (int t = tid; t < n; t += 256) {
        const int64_t it = ids[t];
        if (it < 0) continue;
        const DT dt = ds[t];
        int rank = 0;
        for (int s = 0; s < n; ++s) {
            const int64_t is = ids[s];
            if (is < 0) continue;
            const DT d = ds[s];
            rank += ((DESC ? d > dt : d < dt) || (d == dt && (is < it || (is == it && s < t)))) ? 1 : 0;
        }
        if (rank < k) { outD[(size_t)q * k + rank] = (float)dt; outI[(size_t)q * k + rank] = it; }
    }
}

// memory.py:117 (exp(-d)) and :129-130 (softmax over the hits), one wave per query
__global__ __launch_bounds__(64) void proto_scores_kernel(const float* D, const int64_t* I, int nq,
                                                          int k, float* out) {
    const int q = blockIdx.x, lane = threadIdx.x;
    float mx = -INFINITY;
    for (int e = lane; e < k; e += 64)
        if (I[(size_t)q * k + e] >= 0) mx = fmaxf(mx, expf(-D[(size_t)q * k + e]));
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    float sum = 0.f;
    for (int e = lane; e < k; e += 64)
        if (I[(size_t)q * k + e] >= 0) sum += expf(expf(-D[(size_t)q * k + e]) - mx);
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) sum += __shfl_xor(sum, o);
    for (int e = lane; e < k; e += 64) {
        const bool v = I[(size_t)q * k + e] >= 0;
        out[(size_t)q * k + e] = v ? expf(expf(-D[(size_t)q * k + e]) - mx) / sum : 0.f;
    }
}

// row ids of the hits -> class ids through the row->class map (index_to_label, memory.py:123,174;
// generalised int32 map of SURVEY 8a M6); padding (id < 0) and out-of-range ids give -1
__global__ __launch_bounds__(256) void rows_to_class_kernel(const int64_t* I, int64_t n, const int32_t* row_class,
                                                            int64_t nrows, const int64_t* class_lut, int nlut,
                                                            int64_t* out) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    const int64_t id = I[t];
    int64_t c = -1;
    if (id >= 0 && id < nrows) {
        c = row_class ? (int64_t)row_class[id] : id;
        if (class_lut) c = (c >= 0 && c < nlut) ? class_lut[c] : -1;
    }
    out[t] = c;
}

// --------------------------------------------------------------------------------------
// small-store exact path: N <= kKnnSmallN rows, ANY k <= N and ANY D.  The reference searches with
// k = #classes (classifier.py:424-425), so k can exceed the fused sweep's limit while N (= #classes,
// one prototype per class) stays tiny.  One block per query: fp64 distance of every row, full bitonic
// sort of (distance, id) in LDS, emit the first k.  Exact by construction (no certificate needed).
// --------------------------------------------------------------------------------------
constexpr int kSmallThreads = 256;

// MODE 0: every row of the store.  FILTERED search -- MODE 1: the rows whose selection bit is set; MODE 2 (id-list route,
// ac_knn_*_topk_ids): entry r of the sort is row ids[r] of the store (n_ids sorted, unique ids; an id outside [0, N) is skipped)
// and ids[r] is what is emitted.  A skipped entry is padding: (+inf, 0x7fffffff) sorts last.
template <bool IP, int MODE = 0>
__device__ __forceinline__ void knn_small_exact_body(const MergeParams& prm, int npow2, char* smem, const SelArgs* sa = nullptr) {
    double* ds = reinterpret_cast<double*>(smem);                // [npow2]
    int32_t* is = reinterpret_cast<int32_t*>(ds + npow2);        // [npow2]
    const int q = blockIdx.x, tid = threadIdx.x;
    const float* qv = prm.Q + (size_t)q * prm.ldQ;
    for (int r = tid; r < npow2; r += kSmallThreads) {
        double a = INFINITY;
        int64_t row = r;
        bool have = r < prm.N;
        if constexpr (MODE == 1) have = have && row_selected(*sa, r);
        if constexpr (MODE == 2) {
            have = r < sa->n_ids;
            if (have) { row = sa->ids[r]; have = row >= 0 && row < prm.N; }
        }
        if (MODE == 0 ? r < prm.N : have) {
            const float* p = prm.P + (size_t)(MODE == 2 ? row : (int64_t)r) * prm.ldP;
            a = exact_lane<IP>(p, qv, prm.D);
            if (IP) a = -a;                                      // (inner product: the key -(p.q))
        }
        ds[r] = a;
        if constexpr (MODE == 0) is[r] = r < prm.N ? r : 0x7fffffff;
        else is[r] = have ? (int32_t)row : 0x7fffffff;
    }
    __syncthreads();
    for (int size = 2; size <= npow2; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = tid; t < (npow2 >> 1); t += kSmallThreads) {
                const int lo = 2 * t - (t & (stride - 1));       // index with bit `stride` cleared
                const int hi = lo + stride;
                const bool asc = (lo & size) == 0;
                const double dl = ds[lo], dh = ds[hi];
                const int32_t il = is[lo], ih = is[hi];
                const bool gt = dl > dh || (dl == dh && il > ih);
                if (gt == asc) { ds[lo] = dh; ds[hi] = dl; is[lo] = ih; is[hi] = il; }
            }
            __syncthreads();
        }
    for (int t = tid; t < prm.k; t += kSmallThreads) {
        bool real = t < prm.N;                                   // (k may exceed npow2: the lists are read for real hits only)
        if constexpr (MODE != 0) real = t < npow2 && is[t < npow2 ? t : 0] != 0x7fffffff;
        emit_hit<IP>(prm, (size_t)q * prm.k + t, real, real ? ds[t] : 0.0, real ? (int64_t)is[t] : -1);
    }
}
template <bool IP>
__global__ __launch_bounds__(kSmallThreads) void knn_small_exact(MergeParams prm, int npow2) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    knn_small_exact_body<IP>(prm, npow2, smem);
}
template <bool IP>
__global__ __launch_bounds__(kSmallThreads) void knn_small_exact_sel(MergeParams prm, int npow2, SelArgs sa) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    knn_small_exact_body<IP, 1>(prm, npow2, smem, &sa);
}
template <bool IP>
__global__ __launch_bounds__(kSmallThreads) void knn_small_exact_ids(MergeParams prm, int npow2, SelArgs sa) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    knn_small_exact_body<IP, 2>(prm, npow2, smem, &sa);
}

}  // namespace

// ---- host side: the plan and the launches of the exact stages (declared in common.h) ----
namespace ac {

// slab-parallel exact fallback: fb_S * k <= 4096 entries per slot, fb_F slots (the route's rule: at most 64, or one per query).
// list_bytes = the merge kernel's key (+ id) arrays in LDS: the G per-block lists, or the segmented candidate list twice.
void knn_exact_plan(ExactPlan* ep, WsTake& take, int k, int kp, int Dp, size_t list_bytes, int fb_F) {
    ep->fb_S = 4096 / next_pow2(k);
    if (ep->fb_S > 64) ep->fb_S = 64;
    if (ep->fb_S < 1) ep->fb_S = 1;
    ep->fb_F = fb_F;
    const size_t fb_entries = (size_t)fb_F * ep->fb_S * k;
    ep->off_fb_d = take(fb_entries * 8);
    ep->off_fb_i = take(fb_entries * 4);
    ep->off_fb_ctr = take(256);
    // (the static LDS of the merge kernel -- segment offsets, scan totals -- is ~1.1 KB)
    ep->merge_lds = list_bytes + align_up((size_t)Dp * 4, 16) + (size_t)kp * 16 + 256 * 4 + 64;
    ep->fb_lds = (size_t)kFbCap * 12 + align_up((size_t)Dp, 4) * 4 + 64;
}

MergeParams knn_merge_params(const float* P, int64_t N, int64_t ldP, const float* Q, int64_t ldQ, int D, int Dp, int k, int kp,
                             int64_t row_offset, float* outD, double* outD64, int64_t* outI, int32_t* stats, char* ws,
                             const ExactPlan& ep) {
    MergeParams mp;
    mp.P = P; mp.N = N; mp.ldP = ldP; mp.Q = Q; mp.ldQ = ldQ; mp.D = D; mp.Dp = Dp; mp.k = k; mp.kp = kp;
    mp.row_offset = row_offset;
    mp.outD = outD; mp.outD64 = outD64; mp.outI = outI;
    mp.flags = (int32_t*)(ws + ep.off_flags);
    mp.stats = stats;
    mp.fb_S = ep.fb_S; mp.fb_F = ep.fb_F;
    mp.fb_d = (double*)(ws + ep.off_fb_d); mp.fb_i = (int32_t*)(ws + ep.off_fb_i); mp.fb_slotctr = (int32_t*)(ws + ep.off_fb_ctr);
    return mp;
}

// (function attributes are set per call: they are per device, and a cached flag is not)
int knn_merge_launch(bool ip, const MergeParams& mp, int nq, size_t attr_lds, size_t lds, hipStream_t stream, const SelArgs* sel,
                     const float* sel_thr) {
    if (sel && sel_thr) {                             // FILTERED search over a candidate buffer: the rule that reads the thresholds
        void (*cfn)(MergeParams, const float*) = ip ? knn_merge_rerank_selc<true> : knn_merge_rerank_selc<false>;
        if (attr_lds) AC_HIP_CHECK(hipFuncSetAttribute((const void*)cfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)attr_lds));
        hipLaunchKernelGGL(cfn, dim3(nq), dim3(kMergeThreads), lds, stream, mp, sel_thr);
        AC_LAUNCH_CHECK();
        return AC_OK;
    }
    void (*fn)(MergeParams) = ip ? knn_merge_rerank<true> : knn_merge_rerank<false>;
    if (sel) fn = ip ? knn_merge_rerank_sel<true> : knn_merge_rerank_sel<false>;         // FILTERED search: one more certificate rule
    if (attr_lds) AC_HIP_CHECK(hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)attr_lds));
    hipLaunchKernelGGL(fn, dim3(nq), dim3(kMergeThreads), lds, stream, mp);
    AC_LAUNCH_CHECK();
    return AC_OK;
}

int knn_exact_tail(bool ip, const MergeParams& mp, const ExactPlan& ep, int nq, size_t merge_lds, hipStream_t stream, const SelArgs* sel,
                   const float* sel_thr) {
    const int rc = knn_merge_launch(ip, mp, nq, ep.merge_lds, merge_lds, stream, sel, sel_thr);
    if (rc != AC_OK || mp.N == 0) return rc;          // (an empty store: everything is padding, nothing can be flagged)
    const dim3 fb_grid(ep.fb_S, nq < kFbQueryGroups ? nq : kFbQueryGroups);
    if (sel) {                                        // FILTERED search: the fallback scans the selected rows only
        void (*fbs_fn)(MergeParams, int, SelArgs) = ip ? knn_exact_fallback_sel<true> : knn_exact_fallback_sel<false>;
        (void)hipFuncSetAttribute((const void*)fbs_fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ep.fb_lds);
        hipLaunchKernelGGL(fbs_fn, fb_grid, dim3(kFbThreads), ep.fb_lds, stream, mp, nq, *sel);
    } else {
    void (*fb_fn)(MergeParams, int) = ip ? knn_exact_fallback<true> : knn_exact_fallback<false>;
    (void)hipFuncSetAttribute((const void*)fb_fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ep.fb_lds);
    hipLaunchKernelGGL(fb_fn, fb_grid, dim3(kFbThreads), ep.fb_lds, stream, mp, nq);
    }
    AC_LAUNCH_CHECK();
    const int np2 = next_pow2(ep.fb_S * mp.k > 2 ? ep.fb_S * mp.k : 2);
    void (*fbm_fn)(MergeParams, int, int) = ip ? knn_exact_fb_merge<true> : knn_exact_fb_merge<false>;
    (void)hipFuncSetAttribute((const void*)fbm_fn, hipFuncAttributeMaxDynamicSharedMemorySize, np2 * 12);
    hipLaunchKernelGGL(fbm_fn, dim3(nq < kFbMergeGroups ? nq : kFbMergeGroups), dim3(256), (size_t)np2 * 12, stream, mp, np2, nq);
    AC_LAUNCH_CHECK();
    return AC_OK;
}

int knn_small_exact_launch(bool ip, const MergeParams& mp, int nq, int npow2, hipStream_t stream, const SelArgs* sel) {
    const size_t lds = (size_t)npow2 * 12;
    if (sel) {                                        // FILTERED search: the id-list kernel or the bitmap kernel
        void (*sfn)(MergeParams, int, SelArgs);
        if (sel->by_ids) sfn = ip ? knn_small_exact_ids<true> : knn_small_exact_ids<false>;
        else sfn = ip ? knn_small_exact_sel<true> : knn_small_exact_sel<false>;
        (void)hipFuncSetAttribute((const void*)sfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL(sfn, dim3(nq), dim3(kSmallThreads), lds, stream, mp, npow2, *sel);
        AC_LAUNCH_CHECK();
        return AC_OK;
    }
    void (*fn)(MergeParams, int) = ip ? knn_small_exact<true> : knn_small_exact<false>;
    (void)hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(fn, dim3(nq), dim3(kSmallThreads), lds, stream, mp, npow2);
    AC_LAUNCH_CHECK();
    return AC_OK;
}

}  // namespace ac

// ---- C entry points ----
// `name` = the entry point (the error texts name it); an input entry takes its int64 id + its distance of LDS
template <typename DT, bool DESC>
static int topk_merge(const char* name, size_t lds_limit, const DT* d_D_in, const int64_t* d_I_in, int shards, int nq, int k,
                      float* d_outD, int64_t* d_outI, ac_stream_t stream_) {
    AC_REQUIRE(shards >= 1 && nq >= 0 && k >= 1, AC_EINVAL, "%s: bad shape", name);
    AC_REQUIRE(d_D_in && d_I_in && d_outD && d_outI, AC_EINVAL, "%s: null pointer", name);
    if (nq == 0) return AC_OK;
    const size_t lds = (size_t)shards * k * (8 + sizeof(DT));
    AC_REQUIRE(lds <= lds_limit, AC_EUNSUPPORTED, "%s: shards*k=%d too large", name, shards * k);
    (void)hipFuncSetAttribute((const void*)topk_merge_kernel<DT, DESC>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL((topk_merge_kernel<DT, DESC>), dim3(nq), dim3(256), lds, (hipStream_t)stream_, d_D_in, d_I_in, shards, nq, k,
                       d_outD, d_outI);
    AC_LAUNCH_CHECK();
    return AC_OK;
}

extern "C" int ac_topk_merge(const float* d_D_in, const int64_t* d_I_in, int shards, int nq, int k,
                             float* d_outD, int64_t* d_outI, ac_stream_t stream) {
    return topk_merge<float, false>("topk_merge", 96 * 1024, d_D_in, d_I_in, shards, nq, k, d_outD, d_outI, stream);
}

extern "C" int ac_topk_merge_f64(const double* d_D_in, const int64_t* d_I_in, int shards, int nq, int k,
                                 float* d_outD, int64_t* d_outI, ac_stream_t stream) {
    return topk_merge<double, false>("topk_merge_f64", 128 * 1024, d_D_in, d_I_in, shards, nq, k, d_outD, d_outI, stream);
}

extern "C" int ac_topk_merge_ip_f64(const double* d_D_in, const int64_t* d_I_in, int shards, int nq, int k,
                                    float* d_outD, int64_t* d_outI, ac_stream_t stream) {
    return topk_merge<double, true>("topk_merge_ip_f64", 128 * 1024, d_D_in, d_I_in, shards, nq, k, d_outD, d_outI, stream);
}

extern "C" int ac_rows_to_class(const int64_t* d_I, int64_t n, const int32_t* d_row_class, int64_t nrows,
                                const int64_t* d_class_lut, int nlut, int64_t* d_out, ac_stream_t stream_) {
    AC_REQUIRE(d_I && d_out && n >= 0 && nrows >= 0, AC_EINVAL, "rows_to_class: bad arguments");
    if (n == 0) return AC_OK;
    hipLaunchKernelGGL(rows_to_class_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream_,
                       d_I, n, d_row_class, nrows, d_class_lut, nlut, d_out);
    AC_LAUNCH_CHECK();
    return AC_OK;
}

extern "C" int ac_proto_scores(const float* d_D, const int64_t* d_I, int nq, int k, float* d_out,
                               ac_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    AC_REQUIRE(nq >= 0 && k >= 1 && d_D && d_I && d_out, AC_EINVAL, "proto_scores: bad arguments");
    if (nq == 0) return AC_OK;
    hipLaunchKernelGGL(proto_scores_kernel, dim3(nq), dim3(64), 0, stream, d_D, d_I, nq, k, d_out);
    AC_LAUNCH_CHECK();
    return AC_OK;
}
