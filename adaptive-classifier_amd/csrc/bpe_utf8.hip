// On-device GPT-2 byte-level BPE tokenisation of UTF-8 text (ac_bpe_utf8_encode, ac_version() >= 17): the tokenizer call of the
// classifier for RoBERTa-style and ModernBERT-style tokenizers on texts with typographic quotes and dashes, accents, Cyrillic,
// short CJK, emoji.  The algorithm -- strict UTF-8 decoding, the probed class table, pre-token boundaries on characters, merge
// lookup, the hash -- is bpe_core.h, shared with ac_bpe_utf8_encode_host.  ac_bpe_encode, bpe_kernel and bpe.hip are what they were.
//
// The frame is bpe_kernel's: one wave per text, four waves per workgroup, no communication between waves, the text's bytes in LDS
// behind the prefix space, windows of 64 bytes that begin on a pre-token start and end on the last pre-token boundary inside them,
// one byte (one adjacent symbol pair) per lane, one merge per pre-token per round.  What is new is one pass in front:
//   class pass      lanes take the text's bytes in chunks of 64; a lane on a lead byte decodes its character strictly (its own
//                   continuation bytes, never past the text's end), looks up the table entry and writes the class to EVERY byte of
//                   the character in a second LDS array, bpe::kContByte on all but the first.  The sequence lengths add up to the
//                   text's length exactly iff no continuation byte stands alone.
//   fit pass        one more sweep of is_start ballots finds a pre-token of more than 64 bytes BEFORE the first id is written, so a
//                   text that is handed back leaves its row untouched (bpe_kernel may have written the ids of earlier windows).
//                   Only pre-tokens that truncation can let the windows reach count: fewer than max_length - 2 in front.
// Every bpe::is_start_utf8 reads the two LDS arrays only.  Pre-token boundaries are character boundaries, so a window never
// ends inside a character (a character straddling bytes 63 / 64 moves the cut in front of its pre-token) and the merge rounds are
// bpe_kernel's, on the same bytes.
// NOT DONE (lens[tx] = -1, the row left unwritten; the wrapper hands the text to the host tokenizer): a pre-token of more than 64
// bytes, malformed UTF-8, a host-only code point, more than 4096 bytes.
// LDS per workgroup: 4 x 4160 text bytes + 4 x 4160 class bytes = 33 280 bytes.  No private segment, no host wait.  Every loop is
// bounded by the text's length or by the symbols of a window (a round removes at least one); the hash probe ends because the table
// is at most half full.
#include <new>

#include "common.h"
#include "bpe_core.h"

namespace {

constexpr int kBpeMaxBytes = 4096;          // bytes of one text (longer texts: NOT DONE)
constexpr int kWindow = 64;                 // one byte per lane
constexpr int kBuf = kBpeMaxBytes + 64;     // + the prefix space

__device__ __forceinline__ uint64_t lanes_below(int l) { return (1ull << l) - 1; }                 // l in [0, 63]
__device__ __forceinline__ uint64_t lanes_above(int l) { return ~((2ull << l) - 1); }              // l = 63 -> 0

__device__ __forceinline__ void lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

struct BpeUtf8Params {
    bpe::Table t;
    bpe::Unicode u;
    int cls_id, sep_id, pad_id, prefix_space;
};

__global__ __launch_bounds__(256) void bpe_utf8_kernel(const uint8_t* __restrict__ text, const int32_t* __restrict__ offs, int b,
                                                       BpeUtf8Params prm, int max_len, int64_t* __restrict__ ids,
                                                       int64_t* __restrict__ mask, int32_t* __restrict__ lens) {
    __shared__ uint8_t bytes[4][kBuf];                              // the text behind its prefix space
    __shared__ uint8_t classes[4][kBuf];                            // per byte: its character's class | bpe::kContByte
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int tx = blockIdx.x * 4 + wv;
    if (tx >= b) return;
    const bpe::Table& t = prm.t;
    const int o0 = offs[tx];
    int n = offs[tx + 1] - o0;
    if (n < 0 || n > kBpeMaxBytes) {                                // wave-uniform
        if (lane == 0) lens[tx] = -1;
        return;
    }
    uint8_t* c = bytes[wv];
    uint8_t* kc = classes[wv];
    // ---- 1. the text into LDS, behind its prefix space ----
    const int shift = (prm.prefix_space && n > 0 && text[o0] != 0x20) ? 1 : 0;
    if (shift && lane == 0) c[0] = 0x20;
    for (int i = lane; i < n; i += 64) c[shift + i] = text[o0 + i];
    n += shift;
    lds_sync();
    // ---- 2. the class pass (everything that decides `ok` is wave-uniform) ----
    bool ok = true;
    int covered = 0;                                                // this lane's share of the sequence lengths
    for (int base = 0; base < n; base += kWindow) {
        const int p = base + lane;
        bool bad = false;
        if (p < n && !bpe::is_cont(c[p])) {
            uint32_t cp;
            const int len = bpe::decode_utf8(c + p, n - p, cp);     // reads c[p, p + min(len, n - p)) only
            if (len == 0) bad = true;
            else {
                const int e = bpe::entry_of(prm.u, cp);
                if (e & bpe::kHostOnly) bad = true;
                else {
                    kc[p] = (uint8_t)(e & bpe::kClassMask);
                    for (int i = 1; i < len; ++i) kc[p + i] = (uint8_t)((e & bpe::kClassMask) | bpe::kContByte);      // p + i < n
                    covered += len;
                }
            }
        }
        if (__ballot(bad)) { ok = false; break; }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) covered += __shfl_xor(covered, o);
    if (!ok || covered != n) {                                      // covered < n: a continuation byte no sequence owns
        if (lane == 0) lens[tx] = -1;
        return;
    }
    lds_sync();
    int64_t* row = ids + (size_t)tx * max_len;
    const int room = max_len - 2;
    // ---- 3. does every pre-token the windows can reach fit one?  Decided before the first id is written, so that a text that is
    //         handed back leaves its row unwritten.  A pre-token yields at least one id: the one that starts at `last` is reached only
    //         if fewer than `room` pre-tokens stand in front of it (truncation ends the text first otherwise).
    {
        int last = 0, seen = 0;                                     // the last pre-token start so far, the number of starts
        bool fits = true;
        for (int base = 0; base < n && seen <= room; base += kWindow) {
            const uint64_t m = __ballot(base + lane < n && bpe::is_start_utf8(c, kc, n, base + lane));
            if (!m) continue;
            if (base + __builtin_ctzll(m) - last > kWindow) { fits = false; break; }      // (seen <= room: [last, ...) is reachable)
            seen += __popcll(m);
            last = base + 63 - __builtin_clzll(m);
        }
        if (fits && seen <= room && n - last > kWindow) fits = false;
        if (!fits) {
            if (lane == 0) lens[tx] = -1;
            return;
        }
    }
    // ---- 4. windows of whole pre-tokens -> ids (bpe_kernel's rounds) ----
    int total = 0;
    bool done = true;
    for (int base = 0; base < n && total < room;) {
        const int p = base + lane;
        uint64_t pre = __ballot(p < n && bpe::is_start_utf8(c, kc, n, p));      // bit 0 is set: base is a pre-token start
        int wend;                                                   // the window is [base, base + wend)
        if (base + kWindow >= n) wend = n - base;
        else if (bpe::is_start_utf8(c, kc, n, base + kWindow)) wend = kWindow;
        else wend = 63 - __builtin_clzll(pre);                      // the last pre-token is cut: it opens the next window
        if (wend == 0) { done = false; break; }                     // a pre-token longer than the window (pass 3 has seen to it: cannot happen)
        const uint64_t live = wend == 64 ? ~0ull : lanes_below(wend);
        pre &= live;
        uint64_t sym = live;                                        // every byte is a symbol
        int id = lane < wend ? t.byte_id[c[p]] : 0;
        int rank = bpe::kNoRank, merged = 0;                        // of the pair (symbol at this lane, the symbol after it)
        bool look = true;
        // this lane's pre-token is lanes [seg0, seg1): fixed for the window
        const int seg0 = 63 - __builtin_clzll((pre & ~lanes_above(lane)) | 1ull);
        const uint64_t pre_above = pre & lanes_above(lane);
        const int seg1 = pre_above ? __builtin_ctzll(pre_above) : wend;
        for (;;) {
            const bool mine = (sym >> lane) & 1;
            const uint64_t above = sym & lanes_above(lane);
            const int nx = above ? __builtin_ctzll(above) : wend;   // where the next symbol starts
            if (look) {
                rank = bpe::kNoRank;
                if (mine && nx < seg1) {
                    const uint64_t above2 = above & (above - 1);
                    const int end = above2 ? __builtin_ctzll(above2) : wend;       // a pre-token start is a symbol start: end <= seg1
                    bpe::lookup(t, c + p, nx - lane, end - lane, rank, merged);
                }
            }
            // the best pair of every pre-token: inclusive prefix minimum inside the segment, read at the segment's last lane
            const uint32_t key = rank == bpe::kNoRank ? 0xffffffffu : ((uint32_t)rank << 6) | (uint32_t)lane;
            uint32_t k = key;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const uint32_t v = __shfl_up(k, o);
                if (lane - o >= seg0) k = v < k ? v : k;
            }
            const uint32_t best = __shfl(k, seg1 - 1);
            const bool win = mine && key != 0xffffffffu && key == best;
            const uint64_t winners = __ballot(win);
            if (!winners) break;
            const uint64_t below = sym & lanes_below(lane);
            const bool absorbed = mine && below && ((winners >> (63 - __builtin_clzll(below))) & 1);   // the symbol before this one won
            if (win) id = merged;
            look = win || (mine && nx < 64 && ((winners >> nx) & 1));       // the pairs whose left or right symbol grew
            if (absorbed) { rank = bpe::kNoRank; look = false; }
            sym &= ~__ballot(absorbed);
        }
        const int slot = total + __popcll(sym & lanes_below(lane));
        if (((sym >> lane) & 1) && slot < room) row[1 + slot] = id;
        total += __popcll(sym);
        base += wend;
    }
    if (!done) {                                                    // the wrapper re-tokenises this text on the host
        if (lane == 0) lens[tx] = -1;
        return;
    }
    if (total > room) total = room;
    // ---- 5. specials, padding, mask ----
    const int L = total + 2;
    if (lane == 0) { row[0] = prm.cls_id; row[L - 1] = prm.sep_id; lens[tx] = L; }
    int64_t* mrow = mask + (size_t)tx * max_len;
    for (int i = lane; i < max_len; i += 64) {
        if (i >= L) row[i] = prm.pad_id;
        mrow[i] = i < L ? 1 : 0;
    }
}

int check_args(const ac_bpe_vocab* v, const ac_bpe_unicode* u, const void* offsets, const void* ids, const void* mask, const void* lens,
               int b, int max_length) {
    AC_REQUIRE(v && u && offsets && ids && mask && lens && b >= 0 && max_length >= 2, AC_EINVAL, "bpe utf8: bad arguments");
    AC_REQUIRE(v->slots >= 2 && (v->slots & (v->slots - 1)) == 0 && v->keys && v->entries && v->blob && v->byte_id, AC_EINVAL,
               "bpe utf8: merge table must have a power-of-two slot count and all arrays");
    AC_REQUIRE(u->page_of && u->entries && u->n_pages >= 1 && u->n_pages <= 65535, AC_EINVAL,
               "bpe utf8: unicode table must have both arrays and 1 .. 65535 pages");
    return AC_OK;
}

BpeUtf8Params params_of(const ac_bpe_vocab* v, const ac_bpe_unicode* u) {
    BpeUtf8Params p;
    p.t.keys = v->keys; p.t.entries = v->entries; p.t.blob = v->blob; p.t.byte_id = v->byte_id; p.t.mask = (uint32_t)(v->slots - 1);
    p.u.page_of = u->page_of; p.u.entries = u->entries; p.u.n_pages = u->n_pages;
    p.cls_id = v->cls_id; p.sep_id = v->sep_id; p.pad_id = v->pad_id; p.prefix_space = v->add_prefix_space;
    return p;
}

}  // namespace

extern "C" int ac_bpe_utf8_encode(const uint8_t* d_text, const int32_t* d_offsets, int b, const ac_bpe_vocab* v, const ac_bpe_unicode* u,
                                  int max_length, int64_t* d_ids, int64_t* d_mask, int32_t* d_lens, ac_stream_t stream) {
    const int rc = check_args(v, u, d_offsets, d_ids, d_mask, d_lens, b, max_length);
    if (rc != AC_OK) return rc;
    if (b == 0) return AC_OK;
    AC_REQUIRE(d_text, AC_EINVAL, "bpe utf8: text is NULL");
    hipLaunchKernelGGL(bpe_utf8_kernel, dim3((b + 3) / 4), dim3(256), 0, (hipStream_t)stream, d_text, d_offsets, b, params_of(v, u),
                       max_length, d_ids, d_mask, d_lens);
    AC_LAUNCH_CHECK();
    return AC_OK;
}

// The same bpe_core.h routines text by text on the CPU (host pointers everywhere, no GPU call): exact for every pre-token length;
// NOT DONE only for malformed UTF-8, a host-only code point or more than 4096 bytes.
extern "C" int ac_bpe_utf8_encode_host(const uint8_t* h_text, const int32_t* h_offsets, int b, const ac_bpe_vocab* v,
                                       const ac_bpe_unicode* u, int max_length, int64_t* h_ids, int64_t* h_mask, int32_t* h_lens) {
    const int rc = check_args(v, u, h_offsets, h_ids, h_mask, h_lens, b, max_length);
    if (rc != AC_OK) return rc;
    if (b == 0) return AC_OK;
    AC_REQUIRE(h_text, AC_EINVAL, "bpe utf8: text is NULL");
    const BpeUtf8Params prm = params_of(v, u);
    const int room = max_length - 2, cap = kBpeMaxBytes + 1;
    // one block, no exception across the C ABI: four int32 work arrays [cap] | the text [cap] | its classes [cap]
    int32_t* work = new (std::nothrow) int32_t[4 * (size_t)cap + (2 * (size_t)cap + 3) / 4];
    AC_REQUIRE(work, AC_EWORKSPACE, "bpe utf8: no host memory for the work arrays");
    uint8_t* c = reinterpret_cast<uint8_t*>(work + 4 * cap);
    uint8_t* class_at = c + cap;
    for (int tx = 0; tx < b; ++tx) {
        const int n0 = h_offsets[tx + 1] - h_offsets[tx];
        if (n0 < 0 || n0 > kBpeMaxBytes) { h_lens[tx] = -1; continue; }
        const uint8_t* src = h_text + h_offsets[tx];
        const int shift = (v->add_prefix_space && n0 > 0 && src[0] != 0x20) ? 1 : 0;
        c[0] = 0x20;
        for (int i = 0; i < n0; ++i) c[shift + i] = src[i];
        int64_t* row = h_ids + (size_t)tx * max_length;
        int64_t* mrow = h_mask + (size_t)tx * max_length;
        // NOT DONE is decided before the first id is written: such a text's row stays as it was
        const int k = bpe::encode_text_utf8(prm.t, prm.u, c, n0 + shift, room, row + 1, class_at, work, work + cap, work + 2 * cap,
                                            work + 3 * cap);
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
    delete[] work;
    return AC_OK;
}
