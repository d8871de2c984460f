// Strategic classification (strategic.py SeparableCostFunction.compute_best_response over the adaptive head) as one
// batched search: b queries x one shared table of M <= 64 single-coordinate moves.
//
// The reference runs one single-row head forward per candidate (b * M forwards).  Here the structure is used:
//   layer 1 is rank-1 per candidate, z1(x + dy e_f) = z1(x) + dy W1[:, f], so W1 x is computed ONCE per query (one
//   [b, D] x [D, H1] GEMM) and the candidate rows are an elementwise kernel (ReLU + dropout mask 1 fused);
//   layer 2 is a real [b M, H1] x [H1, H2] GEMM on the fp32 MFMA pipe (gemm.hip) with bias + ReLU + mask 2 in its epilogue;
//   layer 3, the softmax maximum, the cost, the first-wins argmax and the chosen row y are one kernel, a workgroup per query.
//
// Cost.  The reference evaluates relu(c.y - c.x) (separable) as two fp32 length-D dots and relu(alpha.(y - x)) (linear) as
// one.  For a single-coordinate move both equal relu(c_f dy) with dy = fl(fl(x_f + delta) - x_f), which is what is computed
// here (one product, correctly rounded).  The linear form is then the reference's value exactly (its dot has one non-zero
// term).  The separable form differs by the rounding of the reference's two dots: |cost_ref - cost| <= gamma_D (sum|c_j x_j| +
// sum|c_j y_j|) + u |c_f dy|, gamma_D = D u / (1 - D u), u = 2^-24 -- for unit-norm x, |c_j| <= 1 and |delta| <= 2 at D = 768
// that is <= 2 * 768 * 2^-24 * (1 + 3) ~= 1.9e-4 in the worst case and ~1e-6 typically (random-sign rounding errors).
#include "common.h"

#include <math.h>

namespace {

constexpr int kMaxCand = AC_STRAT_MAX_CANDIDATES;
constexpr int kMaxC = 2048;

struct StratWs {
    size_t z1, a1, a2, total;
};

StratWs strat_ws(const ac_head_dims& d, int b, int M) {
    StratWs w;
    size_t off = 0;
    auto take = [&](size_t n) { size_t o = off; off += ac::align_up(n * sizeof(float), 256); return o; };
    w.z1 = take((size_t)b * d.H1);
    w.a1 = take((size_t)b * M * d.H1);
    w.a2 = take((size_t)b * M * d.H2);
    w.total = off;
    return w;
}

__device__ __forceinline__ float relu_keep_nan(float v) { return v < 0.f ? 0.f : v; }

// candidate rows of layer 1: a1[q M + m, h] = dropout(relu(z1[q, h] + dy W1[h, f]))
__global__ __launch_bounds__(256) void cand_layer1_kernel(const float* __restrict__ z1, const float* __restrict__ X, int64_t ldx,
                                                          const float* __restrict__ W1, int D, int H1,
                                                          const int32_t* __restrict__ feat, const float* __restrict__ delta,
                                                          int M, int mask_mode, const uint8_t* __restrict__ mask1, float p,
                                                          float scale, uint64_t seed, float* __restrict__ a1) {
    const int r = blockIdx.x;                 // q * M + m
    const int q = r / M, m = r - q * M;
    const int f = feat[m];
    const bool ident = f < 0 || f >= D;
    float dy = 0.f;
    if (!ident) {
        const float xf = X[(int64_t)q * ldx + f];
        dy = (xf + delta[m]) - xf;
    }
    const float* zr = z1 + (int64_t)q * H1;
    float* out = a1 + (int64_t)r * H1;
    for (int h = threadIdx.x; h < H1; h += blockDim.x) {
        float v = zr[h];
        if (!ident) v = fmaf(dy, W1[(int64_t)h * D + f], v);
        v = relu_keep_nan(v);                 // (torch.relu keeps NaN; fmaxf would not)
        if (mask_mode == AC_STRAT_MASK_EXPLICIT) v = mask1[(int64_t)r * H1 + h] ? v * scale : 0.f;
        else if (mask_mode == AC_STRAT_MASK_SEED) v = ac::dropout_keep(seed, (uint64_t)r * (uint64_t)H1 + h, p) ? v * scale : 0.f;
        out[h] = v;
    }
}

// lane 0's LDS writes visible to the other lanes of its wave (no workgroup barrier: the waves run different trip counts)
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ float wave_sum(float s) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) s += __shfl_xor(s, o);
    return s;
}

// layer 3 + max softmax + cost + first-wins argmax + y, one workgroup (4 waves) per query; wave w takes candidates w, w + 4, ...
__global__ __launch_bounds__(256) void cand_select_kernel(const float* __restrict__ a2, int H2, const float* __restrict__ W3,
                                                          const float* __restrict__ b3, int C, int has_head,
                                                          const float* __restrict__ X, int64_t ldx, int D,
                                                          const int32_t* __restrict__ feat, const float* __restrict__ delta, int M,
                                                          const float* __restrict__ coef, int32_t* __restrict__ choice,
                                                          float* __restrict__ util, float* __restrict__ util_all,
                                                          float* __restrict__ Y, int64_t ldy, float* __restrict__ logits) {
    __shared__ float lg[4][kMaxC];
    __shared__ float us[kMaxCand];
    __shared__ int best_s;
    const int q = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float* xr = X + (int64_t)q * ldx;
    for (int m = wave; m < M; m += 4) {
        const int f = feat[m];
        const bool ident = f < 0 || f >= D;
        float dy = 0.f;
        if (!ident) {
            const float xf = xr[f];
            dy = (xf + delta[m]) - xf;
        }
        float pmax;
        if (has_head) {
            const float* ar = a2 + ((int64_t)q * M + m) * H2;
            float mx = -INFINITY;
            bool nan = false;
            for (int c = 0; c < C; ++c) {
                const float* wr = W3 + (int64_t)c * H2;
                float s = 0.f;
                for (int h = lane; h < H2; h += 64) s = fmaf(ar[h], wr[h], s);
                s = wave_sum(s) + b3[c];
                if (lane == 0) lg[wave][c] = s;
                mx = fmaxf(mx, s);
                nan |= (s != s);
            }
            wave_sync();
            float se = 0.f;
            for (int c = lane; c < C; c += 64) se += expf(lg[wave][c] - mx);
            se = wave_sum(se);
            pmax = nan ? NAN : 1.f / se;     // softmax at the maximum: exp(0) / sum
            wave_sync();                     // (the next candidate overwrites lg[wave])
        } else {
            pmax = 1.f / (float)C;           // torch.ones(1, C) / C
        }
        const float cost = ident ? 0.f : relu_keep_nan(coef[f] * dy);
        const float u = pmax - cost;
        if (lane == 0) {
            us[m] = u;
            if (util_all) util_all[(int64_t)q * M + m] = u;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int best = 0;
        float bu = -INFINITY;
        bool any = false;
        for (int m = 0; m < M; ++m) {
            if (us[m] > bu) { bu = us[m]; best = m; any = true; }
        }
        best_s = best;
        choice[q] = best;
        util[q] = any ? bu : us[0];
    }
    __syncthreads();
    const int best = best_s;
    const int f = feat[best];
    const bool ident = f < 0 || f >= D;
    float* yr = Y + (int64_t)q * ldy;
    for (int j = threadIdx.x; j < D; j += blockDim.x) yr[j] = (!ident && j == f) ? xr[j] + delta[best] : xr[j];
    if (logits && has_head) {
        const float* ar = a2 + ((int64_t)q * M + best) * H2;
        for (int c = wave; c < C; c += 4) {
            const float* wr = W3 + (int64_t)c * H2;
            float s = 0.f;
            for (int h = lane; h < H2; h += 64) s = fmaf(ar[h], wr[h], s);
            s = wave_sum(s) + b3[c];
            if (lane == 0) logits[(int64_t)q * C + c] = s;
        }
    }
}

int check_dims(const ac_head_dims* d) {
    AC_REQUIRE(d != nullptr, AC_EINVAL, "strategic: dims is NULL");
    AC_REQUIRE(d->D >= 1 && d->H1 >= 1 && d->H2 >= 1 && d->C >= 1 && d->C <= kMaxC, AC_EINVAL,
               "strategic: bad dims %d/%d/%d/%d (C <= %d)", d->D, d->H1, d->H2, d->C, kMaxC);
    return AC_OK;
}

}  // namespace

extern "C" int ac_strategic_workspace(const ac_head_dims* dims, int b, int M, size_t* bytes) {
    int rc = check_dims(dims);
    if (rc) return rc;
    AC_REQUIRE(bytes && b >= 0 && M >= 1 && M <= kMaxCand, AC_EINVAL, "strategic_workspace: bad arguments (M=%d)", M);
    *bytes = strat_ws(*dims, b > 0 ? b : 1, M).total;
    return AC_OK;
}

extern "C" int ac_strategic_best_response(const ac_head_dims* dims, const float* d_params, const float* d_X, int64_t ldx, int b,
                                          const int32_t* d_cand_feat, const float* d_cand_delta, int M,
                                          const float* d_coef, int cost_type, int mask_mode, const uint8_t* d_mask1,
                                          const uint8_t* d_mask2, float dropout_p, uint64_t dropout_seed,
                                          int32_t* d_choice, float* d_util, float* d_util_all, float* d_Y, int64_t ldy,
                                          float* d_logits, void* d_ws, size_t ws_bytes, ac_stream_t stream_) {
    int rc = check_dims(dims);
    if (rc) return rc;
    const ac_head_dims& d = *dims;
    AC_REQUIRE(b >= 0 && M >= 1 && M <= kMaxCand, AC_EINVAL, "strategic_best_response: b=%d M=%d (1 <= M <= %d)", b, M, kMaxCand);
    if (b == 0) return AC_OK;
    AC_REQUIRE(d_X && ldx >= d.D && d_cand_feat && d_cand_delta && d_coef && d_choice && d_util && d_Y && ldy >= d.D,
               AC_EINVAL, "strategic_best_response: bad arguments");
    AC_REQUIRE(cost_type == AC_STRAT_COST_SEPARABLE || cost_type == AC_STRAT_COST_LINEAR, AC_EINVAL,
               "strategic_best_response: cost_type=%d", cost_type);
    AC_REQUIRE(mask_mode >= AC_STRAT_MASK_NONE && mask_mode <= AC_STRAT_MASK_SEED, AC_EINVAL,
               "strategic_best_response: mask_mode=%d", mask_mode);
    AC_REQUIRE(mask_mode != AC_STRAT_MASK_EXPLICIT || (d_mask1 && d_mask2), AC_EINVAL,
               "strategic_best_response: explicit masks need both mask tensors");
    AC_REQUIRE(dropout_p >= 0.f && dropout_p < 1.f, AC_EINVAL, "strategic_best_response: dropout_p=%f", dropout_p);
    hipStream_t stream = (hipStream_t)stream_;
    const int has_head = d_params != nullptr;
    const float* W3 = nullptr;
    const float* b3 = nullptr;
    float* a2 = nullptr;
    if (has_head) {
        const StratWs w = strat_ws(d, b, M);
        AC_REQUIRE(d_ws && ws_bytes >= w.total, AC_EWORKSPACE, "strategic_best_response: workspace %zu < %zu", ws_bytes, w.total);
        char* ws = (char*)d_ws;
        float* z1 = (float*)(ws + w.z1);
        float* a1 = (float*)(ws + w.a1);
        a2 = (float*)(ws + w.a2);
        // flat block layout of include/acamd.h: W1 | b1 | W2 | b2 | W3 | b3
        const float* W1 = d_params;
        const float* b1 = W1 + (int64_t)d.H1 * d.D;
        const float* W2 = b1 + d.H1;
        const float* b2 = W2 + (int64_t)d.H2 * d.H1;
        W3 = b2 + d.H2;
        b3 = W3 + (int64_t)d.C * d.H2;
        const bool drop = mask_mode != AC_STRAT_MASK_NONE && dropout_p > 0.f;
        const int mode = drop ? mask_mode : AC_STRAT_MASK_NONE;
        const float scale = drop ? 1.f / (1.f - dropout_p) : 1.f;
        rc = ac::linear_f32(d_X, ldx, W1, d.D, b1, nullptr, 0, z1, d.H1, b, d.H1, d.D, 0, nullptr, 1.f, stream);
        if (rc) return rc;
        hipLaunchKernelGGL(cand_layer1_kernel, dim3((unsigned)(b * M)), dim3(256), 0, stream, z1, d_X, ldx, W1, d.D, d.H1,
                           d_cand_feat, d_cand_delta, M, mode, d_mask1, dropout_p, scale, dropout_seed, a1);
        AC_LAUNCH_CHECK();
        rc = ac::linear_f32(a1, d.H1, W2, d.H1, b2, nullptr, 0, a2, d.H2, b * M, d.H2, d.H1, 1,
                            mode == AC_STRAT_MASK_EXPLICIT ? d_mask2 : nullptr, scale, stream,
                            mode == AC_STRAT_MASK_SEED ? dropout_p : 0.f, dropout_seed ^ 0xA5A5A5A5A5A5A5A5ull);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(cand_select_kernel, dim3((unsigned)b), dim3(256), 0, stream, a2, d.H2, W3, b3, d.C, has_head, d_X, ldx,
                       d.D, d_cand_feat, d_cand_delta, M, d_coef, d_choice, d_util, d_util_all, d_Y, ldy, d_logits);
    AC_LAUNCH_CHECK();
    return AC_OK;
}
