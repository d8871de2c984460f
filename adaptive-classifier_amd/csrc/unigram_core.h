// SentencePiece-style Unigram tokenisation (tokenizers Metaspace + Unigram) of ASCII text, written once for the kernel
// (unigram.hip), the host entry point (ac_unigram_encode_host) and any plain C++ program: no HIP runtime header is needed,
// UNI_HD is empty without hipcc.
//
//   bytes           0x21-0x7E are word bytes, 0x20 (and \t \n \r with ws_controls) is whitespace; A-Z -> a-z with lowercase
//   words           every maximal run of word bytes is one word, prefixed with the metaspace; the metaspace is stored as the
//                   byte 0x20 -- whitespace never occurs inside a word, so 0x20 is free -- and in the text buffer it IS the
//                   whitespace byte in front of the word (the buffer starts with one 0x20 for a text that starts with a word).
//                   trailing_space_piece: a text that ends in whitespace gets a last word of the metaspace alone
//   model           per word, Viterbi in fp64: starts s ascending; every vocabulary piece equal to word[s, t) proposes
//                   best[s] + score and replaces best[t] only when best[t] is unset or the proposal is STRICTLY greater; where
//                   no one-byte piece starts at s, the unknown proposes best[s] + unk_score for t = s + 1 by the same rule.
//                   Backtracking from the word's end; consecutive unknowns of a word are one unk_id
//   table           open addressing over the pure-ASCII pieces, keyed by a polynomial hash: the hash of any word[s, t) follows
//                   in O(1) from per-byte prefixes (range_poly), which is what lets every lane of the kernel probe its own piece
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define UNI_HD __host__ __device__ __forceinline__
#else
#define UNI_HD inline
#endif

namespace unigram {

constexpr uint64_t kPolyBase = 0x9e3779b97f4a7c15ull;      // odd: arithmetic mod 2^64
constexpr uint64_t kMixMul = 0xbf58476d1ce4e5b9ull;
constexpr int kUnkPiece = -1;                               // id_at value of the unknown inside encode_text

// The piece table (ac_unigram_vocab without the post-processor's ids): open addressing, linear probing, power-of-two slot
// count, filled to at most half.  slot of a piece = (h ^ (h >> 32)) & mask, h = hash(piece bytes).
struct Table {
    const uint64_t* keys;       // [slots] stored hash, 0 = empty
    const int32_t* entries;     // [slots][4]: token id, piece length, blob offset, 0
    const double* scores;       // [slots] the piece's log probability
    const uint8_t* blob;        // the pieces' bytes (metaspace = 0x20)
    uint32_t mask;              // slots - 1
};

// poly(b[0, n)) = sum (b[i] + 1) * B^(n - 1 - i) mod 2^64: one step appends a byte
UNI_HD uint64_t poly_step(uint64_t p, uint8_t c) { return p * kPolyBase + (uint64_t)c + 1; }
// ... so with prefix[i] = poly(b[0, i)):  poly(b[s, t)) = prefix[t] - prefix[s] * B^(t - s)
UNI_HD uint64_t range_poly(uint64_t prefix_t, uint64_t prefix_s, uint64_t base_pow_len) { return prefix_t - prefix_s * base_pow_len; }
// the polynomial's low bits depend on the bytes' low bits only: mix before use as a table key; never 0 (0 marks an empty slot)
UNI_HD uint64_t finish(uint64_t p) {
    p ^= p >> 29;
    p *= kMixMul;
    p ^= p >> 32;
    return p == 0 ? 1 : p;
}
UNI_HD uint64_t hash(const uint8_t* b, int n) {
    uint64_t p = 0;
    for (int i = 0; i < n; ++i) p = poly_step(p, b[i]);
    return finish(p);
}
UNI_HD uint32_t home_slot(const Table& t, uint64_t h) { return (uint32_t)(h ^ (h >> 32)) & t.mask; }

// Is p[0, len) a piece?  h = its hash, (slot, k) = where the probe stands: a slot and the key read from it (the caller may have
// read the home slot's key ahead of time).  A hit is verified against the blob: a hash collision never yields a wrong id.
UNI_HD bool lookup_from(const Table& t, uint64_t h, uint32_t slot, uint64_t k, const uint8_t* p, int len, int& id, double& score) {
    for (;;) {
        if (k == 0) return false;
        if (k == h) {
            const int32_t* e = t.entries + 4 * (uint64_t)slot;
            if (e[1] == len) {
                const uint8_t* b = t.blob + (uint32_t)e[2];
                bool eq = true;
                for (int i = 0; i < len; ++i) eq &= b[i] == p[i];
                if (eq) { id = e[0]; score = t.scores[slot]; return true; }
            }
        }
        slot = (slot + 1) & t.mask;
        k = t.keys[slot];
    }
}
UNI_HD bool lookup(const Table& t, uint64_t h, const uint8_t* p, int len, int& id, double& score) {
    const uint32_t slot = home_slot(t, h);
    return lookup_from(t, h, slot, t.keys[slot], p, len, id, score);
}

// ---- the byte classes -------------------------------------------------------------------------------------------------
UNI_HD bool is_space(uint8_t c, int ws_controls) { return c == 0x20 || (ws_controls && (c == 0x09 || c == 0x0a || c == 0x0d)); }
// a text byte as the model sees it: whitespace -> 0x20 (the metaspace of the word behind it), upper -> lower case on demand
UNI_HD uint8_t norm_byte(uint8_t c, int lowercase, int ws_controls) {
    if (is_space(c, ws_controls)) return 0x20;
    return (lowercase && c >= 'A' && c <= 'Z') ? (uint8_t)(c + 32) : c;
}
// c[0, n): one leading 0x20, then the text's bytes through norm_byte.  Does a word start (with its metaspace) at byte p?
UNI_HD bool word_start(const uint8_t* c, int n, int p, int trailing_space_piece) {
    if (c[p] != 0x20) return false;
    if (p + 1 < n) return c[p + 1] != 0x20;
    return trailing_space_piece && n > 1;                   // the text's last byte is whitespace: the metaspace alone
}

// ---- one word on one thread ---------------------------------------------------------------------------------------------
// w[0, L): the word, metaspace first.  Work arrays of L + 1 entries: best / from_at / id_at are indexed by a piece END, next_at
// by a piece START.  Appends the word's ids to out[total ...] while total < room; returns the new total.
inline int encode_word(const Table& t, int max_piece, double unk_score, int unk_id, const uint8_t* w, int L, int room, int total,
                       int64_t* out, double* best, int32_t* from_at, int32_t* id_at, int32_t* next_at) {
    for (int i = 0; i <= L; ++i) from_at[i] = -1;
    best[0] = 0.0;
    for (int s = 0; s < L; ++s) {
        const double bs = best[s];                          // final: every earlier start is done, and every boundary is reachable
        bool single = false;
        uint64_t p = 0;
        const int tmax = L - s < max_piece ? L : s + max_piece;
        for (int e = s + 1; e <= tmax; ++e) {
            p = poly_step(p, w[e - 1]);
            int id;
            double score;
            if (!lookup(t, finish(p), w + s, e - s, id, score)) continue;
            if (e == s + 1) single = true;
            const double cand = bs + score;
            if (from_at[e] < 0 || cand > best[e]) { best[e] = cand; from_at[e] = s; id_at[e] = id; }
        }
        if (!single) {
            const double cand = bs + unk_score;
            if (from_at[s + 1] < 0 || cand > best[s + 1]) { best[s + 1] = cand; from_at[s + 1] = s; id_at[s + 1] = kUnkPiece; }
        }
    }
    for (int e = L; e > 0; e = from_at[e]) next_at[from_at[e]] = e;
    bool after_unk = false;
    for (int s = 0; s < L && total < room; s = next_at[s]) {
        const int id = id_at[next_at[s]];
        if (id == kUnkPiece) {
            if (!after_unk) out[total++] = unk_id;
            after_unk = true;
        } else {
            out[total++] = id;
            after_unk = false;
        }
    }
    return total;
}

// ---- one text on one thread (the host entry point; any word length) ------------------------------------------------------
// c[0, n): one leading 0x20, then the text's bytes through norm_byte.  Writes up to `room` ids to out, returns how many.
// Work arrays of n + 1 entries each.
inline int encode_text(const Table& t, int max_piece, double unk_score, int unk_id, int trailing_space_piece, const uint8_t* c, int n,
                       int room, int64_t* out, double* best, int32_t* from_at, int32_t* id_at, int32_t* next_at) {
    int total = 0;
    for (int p = 0; p < n && total < room;) {
        if (!word_start(c, n, p, trailing_space_piece)) { ++p; continue; }
        int q = p + 1;
        while (q < n && c[q] != 0x20) ++q;
        total = encode_word(t, max_piece, unk_score, unk_id, c + p, q - p, room, total, out, best, from_at, id_at, next_at);
        p = q;
    }
    return total;
}

}  // namespace unigram
