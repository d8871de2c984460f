// On-device SentencePiece-style Unigram tokenisation: the `self.tokenizer(texts, max_length, truncation=True, padding=True)`
// call of the classifier for DeBERTa-v2/v3 and XLM-R style tokenizers (tokenizers Metaspace(always) + Unigram), ASCII texts.
// The algorithm -- byte classes, word boundaries, the piece table and its hash, the Viterbi rule -- is unigram_core.h, shared
// with ac_unigram_encode_host.
//
//   words           whitespace-separated; each carries its metaspace in front (stored as the byte 0x20: the whitespace byte
//                   in front of the word IS its metaspace, and the buffer starts with one 0x20)
//   model           per word, Viterbi in fp64, starts ascending, a proposal wins only when strictly greater; unknown bytes
//                   cost unk_score each and consecutive ones are one unk_id
//   post-processor  cls_id ids[: max_length - 2] sep_id, padded with pad_id; attention mask
// Texts with other bytes than 0x20-0x7E \t \n \r, literal special / added-token strings or more than 4096 bytes are tokenised
// by the host tokenizer (the Python wrapper routes them).
//
// One wave per text, four waves per workgroup, the text's bytes in LDS (as bpe_kernel).  The wave walks the text in windows of
// up to 64 bytes that hold whole words.  A lane is a piece END: it keeps best / the winning piece's length and id for the
// boundary behind its byte in registers.  Starts are taken in ascending order RELATIVE TO EACH WORD'S FIRST BYTE, so all words
// of a window advance together and a window costs as many steps as its longest word has bytes, not 64.  At step k lane e probes
// word[k, e] -- its hash comes in O(1) from the per-byte prefix polynomials (one wave scan per window) -- reads best[k] from the
// lane in front of the start and applies the strict-greater rule; the lane of byte k itself proposes the unknown when no
// one-byte piece matched.  The fp64 adds happen in start-ascending order, as the library's do, so ties resolve identically.  The
// home-slot key of step k + 1 is read before the probe of step k is resolved: the table round trips of consecutive steps overlap.
// Backtracking: the last lane of every word walks its word's winning lengths through LDS and marks the piece ends; a ballot
// turns the marks into output slots.
// LDS per workgroup: 4 x (4096 + 64) text bytes + 4 x 2 x 64 walk bytes + 65 x 8 bytes of base powers = 17 680 bytes with
// alignment (nine workgroups' worth per CU; the listing shows 80 VGPRs).  No private segment, no LDS beyond that.
// The price of the window: a word of more than 64 bytes (metaspace included) fits none.  Such a text is marked NOT DONE
// (lens[tx] = -1, its row left unwritten) and the wrapper hands it to the host tokenizer; it never gets a wrong id.
#include <new>

#include "common.h"
#include "unigram_core.h"

namespace {

constexpr int kUniMaxBytes = 4096;          // bytes of one text (longer texts: host tokenizer)
constexpr int kWindow = 64;                 // one byte per lane

__device__ __forceinline__ uint64_t lanes_below(int l) { return (1ull << l) - 1; }                 // l in [0, 63]
__device__ __forceinline__ uint64_t lanes_through(int l) { return (2ull << l) - 1; }               // l = 63 -> all

struct UniParams {
    unigram::Table t;
    double unk_score;
    int max_piece, unk_id, cls_id, sep_id, pad_id, lowercase, trailing_space_piece, ws_controls;
};

__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__global__ __launch_bounds__(256) void unigram_kernel(const uint8_t* __restrict__ text, const int32_t* __restrict__ offs, int b,
                                                      UniParams prm, int max_len, int64_t* __restrict__ ids,
                                                      int64_t* __restrict__ mask, int32_t* __restrict__ lens) {
    __shared__ uint8_t bytes[4][kUniMaxBytes + 64];                 // the leading 0x20 + the text
    __shared__ uint8_t walk_len[4][kWindow], walk_end[4][kWindow];
    __shared__ uint64_t base_pow[kWindow + 1];
    if (threadIdx.x <= kWindow) {
        uint64_t p = 1;
        for (int i = 0; i < (int)threadIdx.x; ++i) p *= unigram::kPolyBase;
        base_pow[threadIdx.x] = p;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int tx = blockIdx.x * 4 + wv;
    if (tx >= b) return;
    const unigram::Table& t = prm.t;
    const int o0 = offs[tx];
    int n = offs[tx + 1] - o0;
    if (n > kUniMaxBytes) n = kUniMaxBytes;                         // (the wrapper never sends longer texts)
    if (n < 0) n = 0;
    uint8_t* c = bytes[wv];
    // ---- 1. the text into LDS behind one 0x20: whitespace -> 0x20, lower case on demand ----
    if (lane == 0) c[0] = 0x20;
    for (int i = lane; i < n; i += 64) c[1 + i] = unigram::norm_byte(text[o0 + i], prm.lowercase, prm.ws_controls);
    n += 1;
    wave_lds_sync();
    // ---- 2. windows of whole words -> ids ----
    int64_t* row = ids + (size_t)tx * max_len;
    const int room = max_len - 2;
    int total = 0;
    bool done = true;
    for (int base = 0; base < n && total < room;) {
        const int p = base + lane;
        const uint8_t ch = p < n ? c[p] : 0x20;
        uint64_t starts = __ballot(p < n && unigram::word_start(c, n, p, prm.trailing_space_piece));
        int wend;                                                   // the window is [base, base + wend)
        if (base + kWindow >= n) wend = n - base;
        else if (c[base + kWindow] == 0x20) wend = kWindow;         // no word crosses the window's end
        else wend = starts ? 63 - __builtin_clzll(starts) : 0;      // the last word is cut: it opens the next window
        if (wend == 0) { done = false; break; }                     // a word longer than the window
        const uint64_t live = wend == 64 ? ~0ull : lanes_below(wend);
        starts &= live;
        const bool is_start = (starts >> lane) & 1;
        const bool inw = lane < wend && (ch != 0x20 || is_start) && (starts & lanes_through(lane)) != 0;
        const int w0 = inw ? 63 - __builtin_clzll(starts & lanes_through(lane)) : lane;
        const int rel = lane - w0;                                  // this byte's index in its word
        // inclusive prefix polynomial of the window's bytes: after the step of distance o a lane's value spans min(lane + 1, 2 o) bytes
        uint64_t hv = (uint64_t)ch + 1, bo = unigram::kPolyBase;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint64_t left = __shfl_up(hv, o);
            if (lane >= o) hv += left * bo;
            bo *= bo;
        }
        // the probe of step k: piece word[k, rel], i.e. bytes [p - len + 1, p]; its prefix sits in the lane in front of the start
        auto prepare = [&](int k, bool& want, int& len, uint64_t& h, uint32_t& slot, uint64_t& key) {
            len = rel - k + 1;
            const int src = lane - len;
            const uint64_t before = __shfl(hv, src & 63);
            want = inw && rel >= k && len <= prm.max_piece;
            if (want) {
                h = unigram::finish(unigram::range_poly(hv, src < 0 ? 0 : before, base_pow[len]));
                slot = unigram::home_slot(t, h);
                key = t.keys[slot];
            }
        };
        double best = 0.0;
        int plen = 0, pid = 0;                                      // the winning piece that ends here: its length (0 = none yet) and id
        bool want_n, want;
        int len_n, len;
        uint64_t h_n = 0, key_n = 0, h, key;
        uint32_t slot_n = 0, slot;
        prepare(0, want_n, len_n, h_n, slot_n, key_n);
        for (int k = 0;; ++k) {
            if (!__ballot(inw && rel >= k)) break;
            want = want_n; len = len_n; h = h_n; slot = slot_n; key = key_n;
            prepare(k + 1, want_n, len_n, h_n, slot_n, key_n);      // in flight while this step's probe resolves
            double bs = __shfl(best, (lane - len) & 63);            // best[k]: final, every earlier start is done
            if (k == 0) bs = 0.0;
            int id = 0;
            double score = 0.0;
            const bool hit = want && unigram::lookup_from(t, h, slot, key, c + p - len + 1, len, id, score);
            if (inw && rel >= k && (hit || len == 1)) {             // no one-byte piece at this start: the unknown
                const double cand = bs + (hit ? score : prm.unk_score);
                if (plen == 0 || cand > best) { best = cand; plen = len; pid = hit ? id : unigram::kUnkPiece; }
            }
        }
        // backtracking: the last lane of every word walks its word's winning lengths
        walk_len[wv][lane] = (uint8_t)plen;
        walk_end[wv][lane] = 0;
        wave_lds_sync();
        const bool next_inside = lane + 1 < wend && c[p + 1] != 0x20;
        if (inw && !next_inside)
            for (int e = lane; e >= w0;) {
                walk_end[wv][e] = 1;
                const int l = walk_len[wv][e];
                if (l == 0) break;                                  // (cannot happen: every boundary of a word is reachable)
                e -= l;
            }
        wave_lds_sync();
        const bool on_path = inw && walk_end[wv][lane] != 0;
        const uint64_t ends = __ballot(on_path);
        const uint64_t unks = __ballot(on_path && pid == unigram::kUnkPiece);
        const uint64_t ends_below = ends & lanes_below(lane);
        const int prev = ends_below ? 63 - __builtin_clzll(ends_below) : -1;       // the piece end before this one
        const bool fused = pid == unigram::kUnkPiece && prev >= w0 && ((unks >> prev) & 1);   // unknowns fuse inside a word only
        const uint64_t emits = __ballot(on_path && !fused);
        const int slot_out = total + __popcll(emits & lanes_below(lane));
        if (((emits >> lane) & 1) && slot_out < room) row[1 + slot_out] = pid == unigram::kUnkPiece ? prm.unk_id : pid;
        total += __popcll(emits);
        base += wend;
        wave_lds_sync();                                            // the next window rewrites the walk bytes
    }
    if (!done) {                                                    // the wrapper re-tokenises this text on the host
        if (lane == 0) lens[tx] = -1;
        return;
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

int check_vocab(const ac_unigram_vocab* v, const void* offsets, const void* ids, const void* mask, const void* lens, int b, int max_length) {
    AC_REQUIRE(v && offsets && ids && mask && lens && b >= 0 && max_length >= 2, AC_EINVAL, "unigram: bad arguments");
    AC_REQUIRE(v->slots >= 2 && (v->slots & (v->slots - 1)) == 0 && v->keys && v->entries && v->scores && v->blob && v->max_piece >= 1,
               AC_EINVAL, "unigram: piece table must have a power-of-two slot count, all arrays and max_piece >= 1");
    return AC_OK;
}

UniParams params_of(const ac_unigram_vocab* v) {
    UniParams p;
    p.t.keys = v->keys; p.t.entries = v->entries; p.t.scores = v->scores; p.t.blob = v->blob; p.t.mask = (uint32_t)(v->slots - 1);
    p.unk_score = v->unk_score;
    p.max_piece = v->max_piece; p.unk_id = v->unk_id; p.cls_id = v->cls_id; p.sep_id = v->sep_id; p.pad_id = v->pad_id;
    p.lowercase = v->lowercase; p.trailing_space_piece = v->trailing_space_piece; p.ws_controls = v->ws_controls;
    return p;
}

}  // namespace

extern "C" int ac_unigram_encode(const uint8_t* d_text, const int32_t* d_offsets, int b, const ac_unigram_vocab* v, int max_length,
                                 int64_t* d_ids, int64_t* d_mask, int32_t* d_lens, ac_stream_t stream) {
    const int rc = check_vocab(v, d_offsets, d_ids, d_mask, d_lens, b, max_length);
    if (rc != AC_OK) return rc;
    if (b == 0) return AC_OK;
    AC_REQUIRE(d_text, AC_EINVAL, "unigram: text is NULL");
    hipLaunchKernelGGL(unigram_kernel, dim3((b + 3) / 4), dim3(256), 0, (hipStream_t)stream, d_text, d_offsets, b, params_of(v),
                       max_length, d_ids, d_mask, d_lens);
    AC_LAUNCH_CHECK();
    return AC_OK;
}

// The same unigram_core.h routines text by text on the CPU (host pointers everywhere, no GPU call): exact for every word
// length, so it never reports a text as not done.
extern "C" int ac_unigram_encode_host(const uint8_t* h_text, const int32_t* h_offsets, int b, const ac_unigram_vocab* v, int max_length,
                                      int64_t* h_ids, int64_t* h_mask, int32_t* h_lens) {
    const int rc = check_vocab(v, h_offsets, h_ids, h_mask, h_lens, b, max_length);
    if (rc != AC_OK) return rc;
    if (b == 0) return AC_OK;
    AC_REQUIRE(h_text, AC_EINVAL, "unigram: text is NULL");
    const UniParams prm = params_of(v);
    const int room = max_length - 2, cap = kUniMaxBytes + 2;
    // one block, no exception across the C ABI: best [cap] doubles | three int32 work arrays [cap] each | the text buffer [cap]
    double* best = new (std::nothrow) double[3 * (size_t)cap];
    AC_REQUIRE(best, AC_EWORKSPACE, "unigram: no host memory for the work arrays");
    int32_t* work = reinterpret_cast<int32_t*>(best + cap);
    uint8_t* c = reinterpret_cast<uint8_t*>(work + 3 * cap);
    for (int tx = 0; tx < b; ++tx) {
        int n = h_offsets[tx + 1] - h_offsets[tx];
        n = n < 0 ? 0 : (n > kUniMaxBytes ? kUniMaxBytes : n);
        const uint8_t* src = h_text + h_offsets[tx];
        c[0] = 0x20;
        for (int i = 0; i < n; ++i) c[1 + i] = unigram::norm_byte(src[i], prm.lowercase, prm.ws_controls);
        n += 1;
        int64_t* row = h_ids + (size_t)tx * max_length;
        int64_t* mrow = h_mask + (size_t)tx * max_length;
        const int L = 2 + unigram::encode_text(prm.t, prm.max_piece, prm.unk_score, prm.unk_id, prm.trailing_space_piece, c, n, room,
                                               row + 1, best, work, work + cap, work + 2 * cap);
        row[0] = v->cls_id;
        row[L - 1] = v->sep_id;
        h_lens[tx] = L;
        for (int i = 0; i < max_length; ++i) {
            if (i >= L) row[i] = v->pad_id;
            mrow[i] = i < L ? 1 : 0;
        }
    }
    delete[] best;
    return AC_OK;
}

// the hash a piece is stored under: the Python table builder restates it, tests/test_unigram_tokenizer_cpu.py compares the two
extern "C" uint64_t ac_unigram_hash(const uint8_t* bytes, int len) { return unigram::hash(bytes, len); }
