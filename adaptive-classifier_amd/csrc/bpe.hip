// On-device GPT-2 byte-level BPE tokenisation: the `self.tokenizer(texts, max_length, truncation=True, padding=True)` call
// of the classifier for RoBERTa-style and ModernBERT-style tokenizers (tokenizers ByteLevel(use_regex) + BPE), ASCII texts.
// The algorithm -- pre-tokeniser boundaries, merge lookup, the hash -- is bpe_core.h, shared with ac_bpe_encode_host.
//
//   prefix space    add_prefix_space: 0x20 in front unless the text is empty or starts with 0x20
//   pre-tokeniser   bpe::is_start on every byte (a function of t[p-4 .. p+2]: all boundaries at once, one ballot)
//   merges          lowest rank first, leftmost on ties, per pre-token, until no adjacent pair is a merge
//   post-processor  cls_id ids[: max_length - 2] sep_id, padded with pad_id; attention mask
// Texts with non-ASCII bytes, literal special / added-token strings or more than 4096 bytes are tokenised by the host
// tokenizer (the Python wrapper routes them).
//
// One wave per text, four waves per workgroup, the text's bytes in LDS (as wordpiece_kernel).  The wave walks the text in
// windows of 64 bytes that begin on a pre-token start and end on the last pre-token boundary inside them: one byte, hence one
// adjacent symbol pair, per lane.  Why not the WordPiece layout (lanes on a pre-token start, each working its own pre-token
// alone): a lane would walk its pre-token's pairs one dependent table probe after the other, again after every merge --
// O(len^2) global round trips in series on a few active lanes, and its symbol list would be a private array (scratch).  Why
// not the wave on ONE pre-token at a time: an English pre-token is ~5 bytes, so 59 lanes would idle and a text's ~25
// pre-tokens would queue up behind one another, one probe latency per merge each.  The window form takes the pair-per-lane
// idea and runs every pre-token of the window at once: merges of different pre-tokens are independent, so one round joins the
// best pair of EACH pre-token (a segmented wave min-reduction on (rank, lane)), all probes of a round are in flight
// together, and only the two pairs next to a merge are looked up again.  Rounds per window = the longest merge chain in
// it.  The symbol state needs no array at all: "a symbol starts here" is one bit per lane of a wave-uniform 64-bit mask, the
// symbol's id and its pair's rank sit in the registers of its first byte's lane -- no scratch, no LDS beyond the text.
// The price: a pre-token of more than 64 bytes fits no window.  Such a text is marked NOT DONE (lens[tx] = -1, its row left
// unwritten) and the wrapper hands it to the host tokenizer; it never gets a wrong id.
#include "common.h"
#include "bpe_core.h"

namespace {

constexpr int kBpeMaxBytes = 4096;          // bytes of one text (longer texts: host tokenizer)
constexpr int kWindow = 64;                 // one byte per lane

__device__ __forceinline__ uint64_t lanes_below(int l) { return (1ull << l) - 1; }                 // l in [0, 63]
__device__ __forceinline__ uint64_t lanes_above(int l) { return ~((2ull << l) - 1); }              // l = 63 -> 0

__global__ __launch_bounds__(256) void bpe_kernel(const uint8_t* __restrict__ text, const int32_t* __restrict__ offs, int b,
                                                  bpe::Table t, int cls_id, int sep_id, int pad_id, int prefix_space, int max_len,
                                                  int64_t* __restrict__ ids, int64_t* __restrict__ mask, int32_t* __restrict__ lens) {
    __shared__ uint8_t bytes[4][kBpeMaxBytes + 64];                 // + the prefix space
    const int lane = threadIdx.x & 63;
    const int tx = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (tx >= b) return;
    const int o0 = offs[tx];
    int n = offs[tx + 1] - o0;
    if (n > kBpeMaxBytes) n = kBpeMaxBytes;                         // (the wrapper never sends longer texts)
    if (n < 0) n = 0;
    uint8_t* c = bytes[threadIdx.x >> 6];
    // ---- 1. the text into LDS, behind its prefix space ----
    const int shift = (prefix_space && n > 0 && text[o0] != 0x20) ? 1 : 0;
    if (shift && lane == 0) c[0] = 0x20;
    for (int i = lane; i < n; i += 64) c[shift + i] = text[o0 + i];
    n += shift;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    // ---- 2. windows of whole pre-tokens -> ids ----
    int64_t* row = ids + (size_t)tx * max_len;
    const int room = max_len - 2;
    int total = 0;
    bool done = true;
    for (int base = 0; base < n && total < room;) {
        const int p = base + lane;
        uint64_t pre = __ballot(p < n && bpe::is_start(c, n, p));   // bit 0 is set: base is a pre-token start
        int wend;                                                   // the window is [base, base + wend)
        if (base + kWindow >= n) wend = n - base;
        else if (bpe::is_start(c, n, base + kWindow)) wend = kWindow;
        else wend = 63 - __builtin_clzll(pre);                      // the last pre-token is cut: it opens the next window
        if (wend == 0) { done = false; break; }                     // a pre-token longer than the window
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
    // ---- 3. specials, padding, mask ----
    const int L = total + 2;
    if (lane == 0) { row[0] = cls_id; row[L - 1] = sep_id; lens[tx] = L; }
    int64_t* mrow = mask + (size_t)tx * max_len;
    for (int i = lane; i < max_len; i += 64) {
        if (i >= L) row[i] = pad_id;
        mrow[i] = i < L ? 1 : 0;
    }
}

int check_vocab(const ac_bpe_vocab* v, const void* offsets, const void* ids, const void* mask, const void* lens, int b, int max_length) {
    AC_REQUIRE(v && offsets && ids && mask && lens && b >= 0 && max_length >= 2, AC_EINVAL, "bpe: bad arguments");
    AC_REQUIRE(v->slots >= 2 && (v->slots & (v->slots - 1)) == 0 && v->keys && v->entries && v->blob && v->byte_id, AC_EINVAL,
               "bpe: merge table must have a power-of-two slot count and all arrays");
    return AC_OK;
}

bpe::Table table_of(const ac_bpe_vocab* v) {
    bpe::Table t;
    t.keys = v->keys; t.entries = v->entries; t.blob = v->blob; t.byte_id = v->byte_id; t.mask = (uint32_t)(v->slots - 1);
    return t;
}

}  // namespace

extern "C" int ac_bpe_encode(const uint8_t* d_text, const int32_t* d_offsets, int b, const ac_bpe_vocab* v, int max_length,
                             int64_t* d_ids, int64_t* d_mask, int32_t* d_lens, ac_stream_t stream) {
    const int rc = check_vocab(v, d_offsets, d_ids, d_mask, d_lens, b, max_length);
    if (rc != AC_OK) return rc;
    if (b == 0) return AC_OK;
    AC_REQUIRE(d_text, AC_EINVAL, "bpe: text is NULL");
    hipLaunchKernelGGL(bpe_kernel, dim3((b + 3) / 4), dim3(256), 0, (hipStream_t)stream, d_text, d_offsets, b, table_of(v), v->cls_id,
                       v->sep_id, v->pad_id, v->add_prefix_space, max_length, d_ids, d_mask, d_lens);
    AC_LAUNCH_CHECK();
    return AC_OK;
}

// The same bpe_core.h routines text by text on the CPU (host pointers everywhere, no GPU call): exact for every pre-token
// length, so it never reports a text as not done.
extern "C" int ac_bpe_encode_host(const uint8_t* h_text, const int32_t* h_offsets, int b, const ac_bpe_vocab* v, int max_length,
                                  int64_t* h_ids, int64_t* h_mask, int32_t* h_lens) {
    const int rc = check_vocab(v, h_offsets, h_ids, h_mask, h_lens, b, max_length);
    if (rc != AC_OK) return rc;
    if (b == 0) return AC_OK;
    AC_REQUIRE(h_text, AC_EINVAL, "bpe: text is NULL");
    const bpe::Table t = table_of(v);
    const int room = max_length - 2;
    uint8_t* c = new uint8_t[kBpeMaxBytes + 1];
    int32_t* work = new int32_t[4 * (kBpeMaxBytes + 1)];
    for (int tx = 0; tx < b; ++tx) {
        int n = h_offsets[tx + 1] - h_offsets[tx];
        n = n < 0 ? 0 : (n > kBpeMaxBytes ? kBpeMaxBytes : n);
        const uint8_t* src = h_text + h_offsets[tx];
        const int shift = (v->add_prefix_space && n > 0 && src[0] != 0x20) ? 1 : 0;
        c[0] = 0x20;
        for (int i = 0; i < n; ++i) c[shift + i] = src[i];
        n += shift;
        int64_t* row = h_ids + (size_t)tx * max_length;
        int64_t* mrow = h_mask + (size_t)tx * max_length;
        const int L = 2 + bpe::encode_text(t, c, n, room, row + 1, work, work + (kBpeMaxBytes + 1), work + 2 * (kBpeMaxBytes + 1),
                                           work + 3 * (kBpeMaxBytes + 1));
        row[0] = v->cls_id;
        row[L - 1] = v->sep_id;
        h_lens[tx] = L;
        for (int i = 0; i < max_length; ++i) {
            if (i >= L) row[i] = v->pad_id;
            mrow[i] = i < L ? 1 : 0;
        }
    }
    delete[] c;
    delete[] work;
    return AC_OK;
}

// the hash a merge is stored under: the Python table builder fills the table with the function the kernel probes with
extern "C" uint64_t ac_bpe_pair_hash(const uint8_t* left, int left_len, const uint8_t* right, int right_len) {
    return bpe::pair_hash(left, left_len, right, right_len);
}
