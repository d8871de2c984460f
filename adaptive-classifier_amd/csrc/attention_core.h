// The fused fp32 attention of one (sequence, head, 32-query tile) by ONE wave -- shared by attention_mfma_kernel (bert.hip: operands
// from the fp32 qkv rows in HBM) and the attention epilogue of the QKV GEMM (gemm_pipe.hip, EPI_QKV_ATTN: operands from the GEMM's
// own output tile staged in LDS).  Same instructions in the same order either way, so the two routes give bit-identical context rows.
// transformers/models/bert/modeling_bert.py:111-203 (BertSelfAttention, eager); modeling_modernbert.py:188-219 for ROPE.
#pragma once
#include "common.h"

#include <math.h>

namespace acattn {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// ---- fused attention on the fp32 MFMA pipe (v_mfma_f32_32x32x2_f32), head dim 64 (or 32) ----
//   S^T tile = K_tile . Q^T  : A = K rows (lane (key j, k-slice h) holds float4 K[j][8kb+4h..]),
//                              B = Q rows (same shape, pre-scaled, resident in registers)
//                              -> C layout: lane & 31 = QUERY, registers = the tile's 32 keys
//   so the online softmax (max / sum over keys) is per-lane register work plus ONE exchange with the
//   partner lane (lane ^ 32) -- no LDS, no row reductions across the wave.
//   O^T += V_tile^T . P^T    : B = P, which is ALREADY in B-operand layout (lane = query, k = lane >> 5:
//                              MFMA step r consumes keys row(r,0) and row(r,1)); A = V^T read as
//                              V[key][32t + (lane & 31)] (128-B coalesced rows).  C layout again has
//                              lane & 31 = query, so the rescale by exp(m_old - m_new) is per lane.
// The k-order inside a tile is whatever the C layout dictates -- a dot product does not care.
__device__ __forceinline__ int crow32(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

__device__ __forceinline__ void rope_rotate(f32x4 (&x)[8], const float* cs, const float* sn, int pos, int h) {
#pragma clang fp contract(off)
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) {
        const f32x4 c = *reinterpret_cast<const f32x4*>(cs + (int64_t)pos * 32 + 8 * kb + 4 * h);
        const f32x4 s = *reinterpret_cast<const f32x4*>(sn + (int64_t)pos * 32 + 8 * kb + 4 * h);
        const f32x4 lo = x[kb], hi = x[kb + 4];
        x[kb] = lo * c + (-hi) * s;          // q * cos + rotate_half(q) * sin, two roundings per term like torch
        x[kb + 4] = hi * c + lo * s;
    }
}

// qb / kb / vb: row 0 of the sequence at this head's Q / K / V columns, `ld` floats between consecutive token rows; S = the
// sequence's length, qt = which 32-query tile.  mask_row (optional): the sequence's key mask (int64, 0 = masked).
// Output: ctx_rows (fp32, row 0 of the sequence at this head's columns, H floats between rows) or, when ctx_planes is given, the
// operand planes of the [rows, H] output-projection input (row0 = the sequence's first row there, headcol = head * DHT).
// ROPE (ModernBERT): q, k rotated by the position's angle before the scores,
//   x'[d] = x[d] cos[d] - x[d+32] sin[d],  x'[d+32] = x[d+32] cos[d] + x[d] sin[d]   (d < 32; cos/sin tables
//   [position][32] computed on the host exactly as transformers does).  Both halves of a pair sit in the same
//   lane (fragment k-blocks kb and kb + 4), so the rotation is register-local.
// window >= 0 (sliding-window layers, masking_utils.py:141-151): key k is visible to query q iff |q - k| <= window.
// FP32_OUT = false: the caller always passes ctx_planes (the fp32-row store path is not compiled: in a kernel whose operands sit
// in LDS its generic destination pointer would become flat stores).
// BIAS (MPNet's relative position bias, modeling_mpnet.py MPNetSelfAttention: scores / sqrt(d) + position_bias + mask): rel_bias is
// this head's row of the [heads][2 span - 1] table, offset so that rel_bias[d] is the bias of (query i, key i + d), |d| < span,
// S <= span.  It is added to the SCALED score (Q is pre-scaled: fl(q k scale) + bias, one rounding each as in the reference) before
// the validity select and the maximum.  Clamped rows -- a query past S, a key past S -- take the table entry of the row they were
// clamped to: the index stays inside (-S, S), the value is discarded with the row.  The 16 entries of a lane and tile are plain
// global loads (the table is <= 49 KB for 12 heads x 1023 and lives in L2), issued ahead of the QK^T MFMAs like the next K fragment.
// DISENT (DeBERTa's disentangled attention, modeling_deberta_v2.py DisentangledSelfAttention; ac_bert_disentangled): the content-to-
// position and position-to-content terms of every (token row, distance) were computed ahead by position_scores_kernel (bert.hip),
// already multiplied by the score scale.  c2p / p2c point at the entry (row 0 of the sequence, this head, distance 0); rows are
// pos_ld floats apart and entry [d] of a row belongs to the pair (query i, key i + d).  The score of (qi, kr) gains
// c2p[qi][kr - qi] + p2c[kr][kr - qi] -- the sum of the two first, then onto the scaled score, as the model adds rel_att -- where
// BIAS adds its table entry.  A lane's 16 c2p entries of a tile lie inside its own row; the p2c entries the 32 lanes of one register
// read are adjacent floats of one key row.  Clamped rows index like the row they were clamped to, so every read stays inside the
// 2 S - 1 distances of the sequence.
struct PosScores {
    const float* c2p;     // [rows][heads][ld]: q_t . PK[idx(d)] * scale at [t][h][d + span - 1]
    const float* p2c;     // the same shape: k_t . PQ[idx(d)] * scale
    int ld, span;         // floats per (row, head) (>= 2 span - 1), span = the call's longest sequence
};
template <bool ROPE, int DHT, bool FP32_OUT = true, bool K_AHEAD = true, bool BIAS = false, bool DISENT = false>
__device__ __forceinline__ void attention_tile(const float* qb, const float* kb_, const float* vb, int64_t ld, int S, int qt, int lane,
                                               float scale, const int64_t* mask_row, const float* rope_cos, const float* rope_sin,
                                               int window, float* ctx_rows, int H, uint16_t* ctx_planes, int64_t rows, int64_t row0,
                                               int headcol, int f16, const float* rel_bias = nullptr, const float* c2p = nullptr,
                                               const float* p2c = nullptr, int64_t pos_ld = 0) {
    // No implicit mul + add fusion in here: whether hipcc contracts `l * corr + psum` or packs two of them into v_pk_fma_f32
    // depends on the surrounding kernel, and the two routes must round alike (the one intended fma is written out).
#pragma clang fp contract(off)
    static_assert(DHT == 64 || (DHT == 32 && !ROPE), "head dim 64, or 32 without RoPE");
    static_assert(!(BIAS && DISENT), "one source of position terms");
    constexpr int NKB = DHT / 8;                                     // 8-dim k-blocks of the QK^T product
    const int j = lane & 31, h = lane >> 5;
    const int qi = qt * 32 + j;
    const bool qvalid = qi < S;

    f32x4 Qf[NKB];
    {
        const float* qp = qb + (int64_t)(qvalid ? qi : S - 1) * ld + 4 * h;
#pragma unroll
        for (int kb = 0; kb < NKB; ++kb) Qf[kb] = *reinterpret_cast<const f32x4*>(qp + 8 * kb);
        if constexpr (ROPE) rope_rotate(Qf, rope_cos, rope_sin, qvalid ? qi : S - 1, h);
#pragma unroll
        for (int kb = 0; kb < NKB; ++kb) Qf[kb] = Qf[kb] * scale;
    }
    f32x16 o0, o1;
#pragma unroll
    for (int r = 0; r < 16; ++r) { o0[r] = 0.f; o1[r] = 0.f; }
    float m = -INFINITY, l = 0.f;

    // K fragment of a tile (keys past S are clamped; they are masked below).  The next tile's fragment is
    // requested right after the QK^T MFMAs have consumed this one, so its latency hides under softmax + PV; after the
    // last tile nothing is requested.  K_AHEAD = false (operands in LDS, the GEMM epilogue): each tile's fragment is read at the
    // top of its own iteration instead -- 32 registers less across softmax + PV in a kernel that sits at its register limit (any
    // branch in here made hipcc spill there), the same loads in front of the same MFMAs for the single-tile sequences (<= 32
    // tokens) that route mostly serves, and no read for a tile that does not exist.  Loads only: the arithmetic is the same.
    f32x4 Kf[NKB];
    auto load_k = [&](int k0) {
        int kr = k0 + j; if (kr > S - 1) kr = S - 1;
        const float* kp = kb_ + (int64_t)kr * ld + 4 * h;
#pragma unroll
        for (int kb = 0; kb < NKB; ++kb) Kf[kb] = *reinterpret_cast<const f32x4*>(kp + 8 * kb);
        if constexpr (ROPE) rope_rotate(Kf, rope_cos, rope_sin, kr, h);
    };
    // key tiles that can hold a visible key for any of this tile's 32 queries (wave-uniform bounds)
    int kbeg = 0, kend = S;
    if (window >= 0) {
        kbeg = qt * 32 - window; kbeg = kbeg < 0 ? 0 : (kbeg / 32) * 32;
        const int last = qt * 32 + 31 + window;
        if (last + 1 < kend) kend = last + 1;
    }
    if constexpr (K_AHEAD) load_k(kbeg);
    for (int k0 = kbeg; k0 < kend; k0 += 32) {
        if constexpr (!K_AHEAD) load_k(k0);
        // key validity as a 32-bit mask shared by the wave
        const int kj = k0 + j;
        const bool kv = kj < S && (!mask_row || mask_row[kj] != 0);
        const unsigned vmask = (unsigned)(__ballot(kv && h == 0) & 0xffffffffull);
        if (vmask == 0u) {                                           // wave-uniform
            if constexpr (K_AHEAD) if (k0 + 32 < kend) load_k(k0 + 32);
            continue;
        }
        float bv[(BIAS || DISENT) ? 16 : 1];
        if constexpr (BIAS) {
            const int qc = qvalid ? qi : S - 1;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                int kr = k0 + crow32(r, h); if (kr > S - 1) kr = S - 1;
                bv[r] = rel_bias[kr - qc];
            }
        }
        if constexpr (DISENT) {
            const int qc = qvalid ? qi : S - 1;
            const float* cq = c2p + (int64_t)qc * pos_ld - qc;       // cq[kr] = c2p[qc][kr - qc]
            const float* pk = p2c - qc;                              // pk[kr * pos_ld + kr] = p2c[kr][kr - qc]
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                int kr = k0 + crow32(r, h); if (kr > S - 1) kr = S - 1;
                bv[r] = cq[kr] + pk[(int64_t)kr * pos_ld + kr];
            }
        }
        f32x16 st;
#pragma unroll
        for (int r = 0; r < 16; ++r) st[r] = 0.f;
#pragma unroll
        for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
            for (int s4 = 0; s4 < 4; ++s4)
                st = __builtin_amdgcn_mfma_f32_32x32x2f32(Kf[kb][s4], Qf[kb][s4], st, 0, 0, 0);
        if constexpr (K_AHEAD) if (k0 + 32 < kend) load_k(k0 + 32);  // (wave-uniform; there is no tile at or past kend to fetch for)
        // online softmax for query `j` (this lane + partner lane hold its 32 keys)
        float cmax = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            bool ok = (vmask >> crow32(r, h)) & 1u;
            if (window >= 0) { const int dk = qi - (k0 + crow32(r, h)); ok = ok && dk <= window && -dk <= window; }
            if constexpr (BIAS || DISENT) st[r] = ok ? st[r] + bv[r] : -INFINITY;
            else st[r] = ok ? st[r] : -INFINITY;
            cmax = fmaxf(cmax, st[r]);
        }
        cmax = fmaxf(cmax, __shfl_xor(cmax, 32));
        const float m_new = fmaxf(m, cmax);
        // with a window a tile may hold no visible key for THIS query: nothing accumulated yet -> keep zeros
        const bool none = m_new == -INFINITY;
        // e^x as 2^(x log2 e) on v_exp_f32 (one multiply + one transcendental instead of ocml's ~25-instruction expf, 17 times per
        // key tile and lane): x <= 0 here, the result's relative error is ~2^-22 (1 + |x|) -- far inside the softmax's own rounding
        constexpr float kLog2e = 1.4426950408889634f;
        const float corr = none ? 1.f : __builtin_amdgcn_exp2f((m - m_new) * kLog2e);            // m = -inf -> 0
        float psum = 0.f;
        float p[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) { p[r] = none ? 0.f : __builtin_amdgcn_exp2f((st[r] - m_new) * kLog2e); psum += p[r]; }
        psum += __shfl_xor(psum, 32);
        l = __builtin_fmaf(l, corr, psum);
        m = m_new;
#pragma unroll
        for (int r = 0; r < 16; ++r) { o0[r] *= corr; o1[r] *= corr; }
        // O^T += V^T P^T -- the LIVE steps only.  MFMA step r multiplies keys crow32(r, 0) and crow32(r, 1) = crow32(r, 0) + 4 of the
        // tile.  A key past S, masked out, or (window) outside [qt 32 - window, qt 32 + 31 + window] -- visible to none of the tile's
        // queries -- has p == +0 exactly in EVERY lane (its score was set to -inf above, and 2^-inf = +0; `none` lanes hold +0 as
        // well), so a step whose two keys are both such adds v * 0 + v' * 0 to each accumulator.  For finite V that is +-0, and
        // x + (+-0) == x bit for bit for every x but -0 (where -0 + +0 = +0).  The accumulators are never -0 at this point short of
        // an fp32 underflow: they start +0, a round-to-nearest sum is -0 only when every term is, o * corr keeps +0 (corr >= 0),
        // and a non-zero o turns into -0 only when corr underflows to 0, i.e. when this tile's maximum exceeds the running one by
        // more than ~87 (e^-87 < 2^-126) -- and then the tile's maximum key itself, p = 1 in a live step, lands on that element.
        // So the live steps run in the order and with the rounding they had, and the dead ones (about a third of them at lengths of
        // 8 .. 32, each 2 x 64 matrix-pipe cycles on the fp32 MFMA) are left out together with their V loads.  The decision is
        // wave-uniform: vmask is a ballot, qt / k0 / window are scalars.  (One visible difference, in the safe direction: a
        // non-finite V row of a key nobody may see no longer reaches the output through 0 * inf.)
        // The V loads of a batch of PVC steps are issued before the batch's first MFMA: a step's branch would otherwise put each
        // load's latency in front of its own MFMA, where the unconditional form had a dozen loads in flight.
        unsigned live = vmask;
        if (window >= 0) {
            const int lo = qt * 32 - window - k0, hi = qt * 32 + 31 + window - k0;       // visible to some query: tile keys lo .. hi
            if (lo > 0) live &= lo < 32 ? 0xffffffffu << lo : 0u;
            if (hi < 31) live &= hi >= 0 ? 0xffffffffu >> (31 - hi) : 0u;
        }
        live = (unsigned)__builtin_amdgcn_readfirstlane((int)(live | (live >> 4)));        // bit crow32(r, 0): step r has a live key
        constexpr int PVC = 8;                                       // steps per batch of V loads (registers: 2 PVC values in flight)
#pragma unroll
        for (int rb = 0; rb < 16; rb += PVC) {
            float v0[PVC], v1[PVC];
#pragma unroll
            for (int u = 0; u < PVC; ++u) {
                const int r = rb + u;
                if (!((live >> crow32(r, 0)) & 1u)) continue;
                int vr = k0 + crow32(r, h); if (vr > S - 1) vr = S - 1;
                const float* vp = vb + (int64_t)vr * ld + j;
                v0[u] = vp[0];
                if constexpr (DHT == 64) v1[u] = vp[32];
            }
#pragma unroll
            for (int u = 0; u < PVC; ++u) {
                const int r = rb + u;
                if (!((live >> crow32(r, 0)) & 1u)) continue;
                o0 = __builtin_amdgcn_mfma_f32_32x32x2f32(v0[u], p[r], o0, 0, 0, 0);
                if constexpr (DHT == 64) o1 = __builtin_amdgcn_mfma_f32_32x32x2f32(v1[u], p[r], o1, 0, 0, 0);
            }
        }
    }
    if (qvalid) {
        const float inv = l > 0.f ? 1.f / l : 0.f;
        // C layout of O^T: lane & 31 = query (this lane), register r = output dim crow32(r, h) (+32 for o1)
        if (!FP32_OUT || ctx_planes) {
            // registers 4g .. 4g+3 are dims 8g + 4h .. +3: half of k-slot (head * 8 + 4t + g); the partner lane
            // (h ^ 1) writes the other half
            const int64_t row = row0 + qi, plane = rows * H;
#pragma unroll
            for (int t = 0; t < DHT / 32; ++t)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    f32x4 v;
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = (t ? o1[4 * g + e] : o0[4 * g + e]) * inv;
                    ac::emit_planes4(ctx_planes + ac::plane_off(rows, row, headcol + 32 * t + 8 * g + 4 * h), plane, v, f16);
                }
        } else if constexpr (FP32_OUT) {
            float* dst = ctx_rows + (int64_t)qi * H;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                dst[crow32(r, h)] = o0[r] * inv;
                if constexpr (DHT == 64) dst[32 + crow32(r, h)] = o1[r] * inv;
            }
        }
    }
}

}  // namespace acattn
