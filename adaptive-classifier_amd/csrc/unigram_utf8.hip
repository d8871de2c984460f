// On-device SentencePiece-style Unigram tokenisation of UTF-8 text (ac_unigram_encode_utf8, ac_version() >= 15): the tokenizer call
// of the classifier for DeBERTa-v2/v3 and XLM-R style tokenizers on texts with accents, Cyrillic, Greek, CJK, kana, Hangul ... and
// on words of any length.  The algorithm -- strict UTF-8 decoding, the probed normaliser table, the character-aware Viterbi rule,
// the piece table and its hash -- is unigram_core.h, shared with ac_unigram_encode_utf8_host.  ac_unigram_encode, unigram_kernel
// and the ASCII tables (unigram.hip) are what they were.
//
// One wave per text, four waves per workgroup, no communication between waves.
//   1. lanes take the text's bytes in chunks of 64; a lane on a lead byte decodes its code point strictly (its own continuation
//      bytes, never past the text's end), looks up its table entry and the bytes it contributes (0 .. 63); one wave prefix sum places
//      them behind one 0x20 in the wave's LDS buffer, whitespace as 0x20.  The same prefix sum adds up the sequence lengths: they
//      cover the text exactly iff no continuation byte stands alone.
//   2. Viterbi.  A lane is a piece END: it keeps best and the winning piece's length for the boundary behind its byte in
//      registers.  Short words go as in unigram_kernel: a window of up to 64 bytes that holds whole words, starts ascending relative
//      to each word's first byte, so a window costs as many steps as its longest word has bytes.  A word of more than 64 bytes goes
//      in BLOCKS of 64 ends: for the ends (e0, e0 + 64] the starts run ascending from e0 + 1 - reach to e0 + 63, reach = min(max_piece,
//      64); best[s] and the prefix polynomial of a start in the block before come by shuffle from the registers that block left
//      behind, those of the block itself as in a window.  At most 64 + reach steps per block; a start on a continuation byte is no
//      start and costs no probe.  The hash of any [s, e] follows in O(1) from the per-byte prefix polynomials, which run on over
//      the whole word (arithmetic mod 2^64), and from B^len, which lane len - 1 holds.  The fp64 adds happen in start-ascending
//      order, as the library's do, so ties resolve identically.  The home-slot key of step k + 1 is read before the probe of
//      step k is resolved.
//      Backtracking: every byte of the normalised text has a walk byte -- the winning length (1 .. 64), or 64 + the character's bytes
//      for the unknown; bit 7 marks a piece end on the winning path.  The last lane of every word (lane 0 for a long word) walks
//      back through LDS; a forward ballot / popcount pass over the segment turns the marks into output slots, fuses unknowns inside
//      a word (across its chunks too) and stops writing at max_length - 2.  The id of an emitted piece is probed again there.
//   3. specials, padding, mask.
// NOT DONE (lens[tx] = -1, the row left unwritten; the wrapper hands the text to the host tokenizer): malformed UTF-8, a host-only
// code point, more than 4096 bytes, a normalised text that does not fit the buffer (5120 bytes with the leading 0x20).
// LDS per workgroup: 4 x 5120 normalised bytes + 4 x 5120 walk bytes = 40 960 bytes, four workgroups per 160 KiB CU; the powers of
// the hash base live in registers.  100 VGPRs, no private segment.  Why not 8 KiB + 8 KiB per wave: with two workgroups per CU
// the compiler pads the kernel's register count to that occupancy (169 in the listing), past the 128 the tokenizer kernels are
// held to; four workgroups per CU keep the listing at what the code uses.  A text of <= 4096 bytes outgrows 5120 only through
// compatibility images (NFKC), and then it defers.  Every loop is bounded by the text's length, the buffer or the reach; the
// hash probe ends because the table is at most half full.
#include <new>

#include "common.h"
#include "unigram_core.h"

namespace {

constexpr int kBuf = unigram::kUtf8BufBytes;
constexpr int kLane = 64;

__device__ __forceinline__ uint64_t below(int l) { return (1ull << l) - 1; }                       // l in [0, 63]
__device__ __forceinline__ uint64_t through(int l) { return (2ull << l) - 1; }                     // l = 63 -> all

struct UniUtf8Params {
    unigram::Table t;
    unigram::Unicode u;
    double unk_score;
    int max_piece, unk_id, cls_id, sep_id, pad_id, trailing_space_piece, ws_controls;
};

__device__ __forceinline__ void lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__global__ __launch_bounds__(256) void unigram_utf8_kernel(const uint8_t* __restrict__ text, const int32_t* __restrict__ offs, int b,
                                                           UniUtf8Params prm, int max_len, int64_t* __restrict__ ids,
                                                           int64_t* __restrict__ mask, int32_t* __restrict__ lens) {
    __shared__ uint8_t norm[4][kBuf];                               // 0x20 + the normalised text
    __shared__ uint8_t walk[4][kBuf];                               // per normalised byte: winning length | 0x80 on the path
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int tx = blockIdx.x * 4 + wv;
    if (tx >= b) return;
    const unigram::Table& t = prm.t;
    const int o0 = offs[tx];
    const int n = offs[tx + 1] - o0;
    const uint8_t* src = text + o0;
    uint8_t* c = norm[wv];
    uint8_t* wk = walk[wv];
    // ---- 1. decode + normalise + compact (everything that decides `ok` is wave-uniform) ----
    bool ok = n >= 0 && n <= unigram::kMaxTextBytes;
    int m = 1, covered = 0;
    if (lane == 0) c[0] = 0x20;
    for (int base = 0; ok && base < n; base += kLane) {
        const int p = base + lane;
        int len = 0, k = 0;
        uint32_t e = 0;
        bool bad = false;
        if (p < n && !unigram::is_cont(src[p])) {
            uint32_t cp;
            len = unigram::decode(src + p, n - p, cp);
            if (len == 0) bad = true;
            else {
                e = unigram::entry(prm.u, cp);
                k = unigram::out_bytes(e, len);
                if (k < 0) { bad = true; k = 0; }
            }
        }
        if (__ballot(bad)) { ok = false; break; }
        int incl = k | (len << 16);                                 // both sums in one scan: <= 64 * 63 and <= 64 + 3
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const int s = __shfl_up(incl, o); if (lane >= o) incl += s; }
        const int tot = __shfl(incl, 63);
        if (m + (tot & 0xffff) > kBuf) { ok = false; break; }
        if (k) unigram::emit(prm.u, e, src + p, len, prm.ws_controls, c + m + (incl & 0xffff) - k);
        m += tot & 0xffff;
        covered += tot >> 16;
    }
    if (!ok || covered != n) {                                      // covered < n: a continuation byte no sequence owns
        if (lane == 0) lens[tx] = -1;
        return;
    }
    lds_sync();
    // ---- 2. Viterbi over windows of whole words and blocks of long words -> ids ----
    int64_t* row = ids + (size_t)tx * max_len;
    const int room = max_len - 2;
    const int maxp = prm.max_piece < unigram::kReach ? prm.max_piece : unigram::kReach;
    const int reach = maxp < 4 ? 4 : maxp;                          // the unknown spans up to 4 bytes
    uint64_t pw = unigram::kPolyBase;                               // B^(lane + 1)
    for (int i = 0; i < lane; ++i) pw *= unigram::kPolyBase;
    int total = 0;
    for (int base = 0; base < m && total < room;) {
        // the segment [base, base + seg): a window of whole words, or one word of more than 64 bytes
        uint64_t starts = __ballot(base + lane < m && unigram::word_start(c, m, base + lane, prm.trailing_space_piece));
        int seg;
        if (base + kLane >= m) seg = m - base;
        else if (c[base + kLane] == 0x20) seg = kLane;              // no word crosses the window's end
        else seg = starts ? 63 - __builtin_clzll(starts) : 0;       // the last word is cut: it opens the next segment
        const bool longw = seg == 0;                                // only lane 0 starts a word, and it runs past the window
        if (longw) {
            int q = base + kLane;                                   // c[q] is a word byte; the word ends at the next 0x20 or at m
            for (;;) {
                const uint64_t sp = __ballot(q + lane < m && c[q + lane] == 0x20);
                if (sp) { q += __builtin_ctzll(sp); break; }
                q += kLane;
                if (q >= m) { q = m; break; }
            }
            seg = q - base;
        }
        const uint64_t live_w = seg >= kLane ? ~0ull : below(seg);
        starts &= live_w;
        const int w0 = (!longw && (starts & through(lane))) ? 63 - __builtin_clzll(starts & through(lane)) : lane;
        double best_prev = 0.0;                                     // the block before: best and prefix polynomial per lane
        uint64_t hv_prev = 0;
        for (int e0 = 0; e0 < seg; e0 += kLane) {                   // a window is one block
            const int p = base + e0 + lane;
            const bool live = e0 + lane < seg;
            const uint8_t ch = live ? c[p] : 0x20;
            bool inw;
            int rel;                                                // this byte's index in its word
            if (longw) { inw = live; rel = e0 + lane; }
            else {
                inw = live && (ch != 0x20 || ((starts >> lane) & 1)) && (starts & through(lane)) != 0;
                rel = lane - w0;
            }
            const bool end_ok = !(p + 1 < m && live && unigram::is_cont(c[p + 1]));      // a piece ends where a character ends
            // inclusive prefix polynomial: of the block's bytes, then carried on from the block before
            uint64_t hv = (uint64_t)ch + 1, bo = unigram::kPolyBase;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const uint64_t left = __shfl_up(hv, o);
                if (lane >= o) hv += left * bo;
                bo *= bo;
            }
            hv += __shfl(hv_prev, 63) * pw;
            // the probe of step k: piece word[k, rel], i.e. bytes [p - len + 1, p]; prefix and best of its start sit in the lane
            // in front of the start, of this block or of the one before
            auto prepare = [&](int k, bool& cand, bool& want, int& len, int& ucl, uint64_t& h, uint32_t& slot, uint64_t& key) {
                len = rel - k + 1;
                const int s = lane - len;
                const uint64_t b1 = __shfl(hv, s & 63), b2 = __shfl(hv_prev, (s + 64) & 63);
                const uint64_t bpow = __shfl(pw, (len - 1) & 63);
                cand = inw && rel >= k && len <= kLane;
                ucl = 0;
                want = false;
                if (cand) {
                    const uint8_t sb = c[p - len + 1];
                    cand = !unigram::is_cont(sb);                   // a start on a character boundary
                    ucl = unigram::char_len(sb);
                    want = cand && end_ok && len <= maxp;
                }
                if (want) {
                    h = unigram::finish(unigram::range_poly(hv, s >= 0 ? b1 : b2, bpow));
                    slot = unigram::home_slot(t, h);
                    key = t.keys[slot];
                }
            };
            double best = 0.0;
            int plen = 0;                                           // the winning piece that ends here: its walk byte (0 = none yet)
            bool cand_n, cand, want_n, want;
            int len_n, len, ucl_n, ucl;
            uint64_t h_n = 0, key_n = 0, h, key;
            uint32_t slot_n = 0, slot;
            int k = 0;
            if (longw && e0 >= reach) k = e0 - (reach - 1);
            prepare(k, cand_n, want_n, len_n, ucl_n, h_n, slot_n, key_n);
            for (;; ++k) {
                if (!__ballot(inw && rel >= k)) break;
                cand = cand_n; want = want_n; len = len_n; ucl = ucl_n; h = h_n; slot = slot_n; key = key_n;
                prepare(k + 1, cand_n, want_n, len_n, ucl_n, h_n, slot_n, key_n);       // in flight while this step's probe resolves
                const int s = lane - len;
                const double s1 = __shfl(best, s & 63), s2 = __shfl(best_prev, (s + 64) & 63);
                const double bs = len == rel + 1 ? 0.0 : (s >= 0 ? s1 : s2);            // best[k]: final, every earlier start is done
                int id = 0;
                double score = 0.0;
                const bool hit = want && unigram::lookup_from(t, h, slot, key, c + p - len + 1, len, id, score);
                if (cand && (hit || len == ucl)) {                  // no piece of exactly this character at this start: the unknown
                    const double v = bs + (hit ? score : prm.unk_score);
                    if (plen == 0 || v > best) { best = v; plen = hit ? len : kLane + ucl; }
                }
            }
            if (live) wk[p] = (uint8_t)plen;
            best_prev = best;
            hv_prev = hv;
        }
        lds_sync();
        // backtracking: the last lane of every word of a window, lane 0 for a long word
        {
            const int p = base + lane;
            bool walker;
            int e, first;
            if (longw) { walker = lane == 0; e = base + seg - 1; first = base; }
            else {
                const bool inw = lane < seg && (c[p] != 0x20 || ((starts >> lane) & 1)) && (starts & through(lane)) != 0;
                walker = inw && !(lane + 1 < seg && c[p + 1] != 0x20);
                e = p;
                first = base + w0;
            }
            if (walker)
                while (e >= first) {
                    const int v = wk[e];
                    wk[e] = (uint8_t)(v | 0x80);
                    const int l = v > kLane ? v - kLane : v;
                    if (l == 0) break;                              // (cannot happen: every character boundary of a word is reachable)
                    e -= l;
                }
        }
        lds_sync();
        // marks -> output slots, chunk by chunk
        bool carry_unk = false;                                     // the last piece end before this chunk is an unknown of the same word
        for (int off = 0; off < seg && total < room; off += kLane) {
            const int p = base + off + lane;
            const int v = off + lane < seg ? wk[p] : 0;
            const bool on_path = (v & 0x80) != 0;
            const int lv = v & 0x7f;
            const bool unk = lv > kLane;
            const uint64_t ends = __ballot(on_path);
            const uint64_t unks = __ballot(on_path && unk);
            const uint64_t ends_below = ends & below(lane);
            const int prev = ends_below ? 63 - __builtin_clzll(ends_below) : -1;        // the piece end before this one
            const bool prev_unk = prev >= 0 ? ((longw || prev >= w0) && ((unks >> prev) & 1)) : carry_unk;
            const bool fused = unk && prev_unk;                     // unknowns fuse inside a word only
            const uint64_t emits = __ballot(on_path && !fused);
            const int slot_out = total + __popcll(emits & below(lane));
            if (((emits >> lane) & 1) && slot_out < room) {
                int id = prm.unk_id;
                if (!unk) {
                    double score;
                    const uint8_t* piece = c + p - lv + 1;
                    if (!unigram::lookup(t, unigram::hash(piece, lv), piece, lv, id, score)) id = prm.unk_id;
                }
                row[1 + slot_out] = id;
            }
            total += __popcll(emits);
            if (longw && ends) carry_unk = (unks >> (63 - __builtin_clzll(ends))) & 1;
        }
        base += seg;
        lds_sync();                                                 // the next segment rewrites walk bytes
    }
    if (total > room) total = room;
    // ---- 3. specials, padding, mask ----
    const int L = total + 2;
    if (lane == 0) { row[0] = prm.cls_id; row[L - 1] = prm.sep_id; lens[tx] = L; }
    int64_t* mrow = mask + (size_t)tx * max_len;
    for (int i = lane; i < max_len; i += 64) {
        if (i >= L) row[i] = prm.pad_id;
        mrow[i] = i < L ? 1 : 0;
    }
}

int check_args(const ac_unigram_vocab* v, const ac_unigram_unicode* u, const void* offsets, const void* ids, const void* mask,
               const void* lens, int b, int max_length) {
    AC_REQUIRE(v && u && offsets && ids && mask && lens && b >= 0 && max_length >= 2, AC_EINVAL, "unigram utf8: bad arguments");
    AC_REQUIRE(v->slots >= 2 && (v->slots & (v->slots - 1)) == 0 && v->keys && v->entries && v->scores && v->blob && v->max_piece >= 1 &&
                   v->max_piece <= unigram::kReach,
               AC_EINVAL, "unigram utf8: piece table must have a power-of-two slot count, all arrays and 1 <= max_piece <= 64");
    AC_REQUIRE(u->page_of && u->entries && u->images && u->n_pages >= 1 && u->n_pages <= 65535 && u->image_bytes >= 0, AC_EINVAL,
               "unigram utf8: unicode table must have all arrays and 1 .. 65535 pages");
    return AC_OK;
}

UniUtf8Params params_of(const ac_unigram_vocab* v, const ac_unigram_unicode* u) {
    UniUtf8Params p;
    p.t.keys = v->keys; p.t.entries = v->entries; p.t.scores = v->scores; p.t.blob = v->blob; p.t.mask = (uint32_t)(v->slots - 1);
    p.u.page_of = u->page_of; p.u.entries = u->entries; p.u.images = u->images; p.u.n_pages = u->n_pages; p.u.image_bytes = u->image_bytes;
    p.unk_score = v->unk_score;
    p.max_piece = v->max_piece; p.unk_id = v->unk_id; p.cls_id = v->cls_id; p.sep_id = v->sep_id; p.pad_id = v->pad_id;
    p.trailing_space_piece = v->trailing_space_piece; p.ws_controls = v->ws_controls;
    return p;
}

}  // namespace

extern "C" int ac_unigram_encode_utf8(const uint8_t* d_text, const int32_t* d_offsets, int b, const ac_unigram_vocab* v,
                                      const ac_unigram_unicode* u, int max_length, int64_t* d_ids, int64_t* d_mask, int32_t* d_lens,
                                      ac_stream_t stream) {
    const int rc = check_args(v, u, d_offsets, d_ids, d_mask, d_lens, b, max_length);
    if (rc != AC_OK) return rc;
    if (b == 0) return AC_OK;
    AC_REQUIRE(d_text, AC_EINVAL, "unigram utf8: text is NULL");
    hipLaunchKernelGGL(unigram_utf8_kernel, dim3((b + 3) / 4), dim3(256), 0, (hipStream_t)stream, d_text, d_offsets, b, params_of(v, u),
                       max_length, d_ids, d_mask, d_lens);
    AC_LAUNCH_CHECK();
    return AC_OK;
}

// The same unigram_core.h routines text by text on the CPU (host pointers everywhere, no GPU call), with the kernel's buffer
// size: exact for every word length, and it reports exactly the texts the kernel reports as not done.
extern "C" int ac_unigram_encode_utf8_host(const uint8_t* h_text, const int32_t* h_offsets, int b, const ac_unigram_vocab* v,
                                           const ac_unigram_unicode* u, int max_length, int64_t* h_ids, int64_t* h_mask,
                                           int32_t* h_lens) {
    const int rc = check_args(v, u, h_offsets, h_ids, h_mask, h_lens, b, max_length);
    if (rc != AC_OK) return rc;
    if (b == 0) return AC_OK;
    AC_REQUIRE(h_text, AC_EINVAL, "unigram utf8: text is NULL");
    const UniUtf8Params prm = params_of(v, u);
    const int room = max_length - 2, cap = kBuf + 2;
    // one block, no exception across the C ABI: best [cap] doubles | three int32 work arrays [cap] each | the text buffer [cap]
    double* best = new (std::nothrow) double[3 * (size_t)cap];
    AC_REQUIRE(best, AC_EWORKSPACE, "unigram utf8: no host memory for the work arrays");
    int32_t* work = reinterpret_cast<int32_t*>(best + cap);
    uint8_t* c = reinterpret_cast<uint8_t*>(work + 3 * cap);
    bool aligned = true;
    for (int tx = 0; tx < b; ++tx) {
        int64_t* row = h_ids + (size_t)tx * max_length;
        int64_t* mrow = h_mask + (size_t)tx * max_length;
        const int k = unigram::encode_text_utf8(prm.u, prm.t, prm.max_piece, prm.unk_score, prm.unk_id, prm.trailing_space_piece,
                                                prm.ws_controls, h_text + h_offsets[tx], h_offsets[tx + 1] - h_offsets[tx], c, kBuf, room,
                                                row + 1, best, work, work + cap, work + 2 * cap, &aligned);
        if (k < 0) { h_lens[tx] = -1; continue; }
        const int L = k + 2;
        row[0] = v->cls_id;
        row[L - 1] = v->sep_id;
        h_lens[tx] = L;
        for (int i = 0; i < max_length; ++i) {
            if (i >= L) row[i] = v->pad_id;
            mrow[i] = i < L ? 1 : 0;
        }
    }
    delete[] best;
    // pieces are whole characters and starts are taken on lead bytes, so no piece of a winning path can cut a character
    AC_REQUIRE(aligned, AC_EINVAL, "unigram utf8: a piece boundary inside a character (the piece table holds bytes that are not UTF-8)");
    return AC_OK;
}
