// SentencePiece-style Unigram tokenisation (tokenizers Metaspace + Unigram) of ASCII text, written once for the kernel
// (unigram.hip), the host entry point (ac_unigram_encode_host) and any plain C++ program: no HIP runtime header is needed,
// UNI_HD is empty without hipcc.  The second half of the file is the same for UTF-8 text (unigram_utf8.hip).
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


// ---- UTF-8 texts (ac_unigram_encode_utf8[_host], ac_version() >= 15) ---------------------------------------------------------
// The same model over Unicode text, written once for unigram_utf8_kernel (unigram_utf8.hip), ac_unigram_encode_utf8_host and any
// plain C++ program.
//   normaliser      the WHOLE normalizer chain of the wrapped tokenizer (Precompiled / NFC / NFKC / Nmt / Lowercase / Replace /
//                   Strip) as a TABLE: code point -> itself | removed | image (UTF-8 bytes in a blob) | host-only, built by probing
//                   the wrapped pipeline (tokenizer.py, build_unigram_unicode_tables); nothing here knows a Unicode property, and
//                   `lowercase` is not read.  Whatever depends on a code point's neighbours or its place in the text (grapheme
//                   clusters of Precompiled, composition under NFC, Strip, runs of Unicode spaces) is kept out by the host-only flag
//   buffer          [0x20][images ...], whitespace bytes of the images (0x20; \t \n \r with ws_controls) stored as 0x20: from here
//                   on words, the metaspace and trailing_space_piece are what they are for ASCII text
//   model           the Viterbi rule above on CHARACTERS: a piece starts and ends on a character boundary only, the unknown at
//                   start s spans the character at s (1-4 bytes) and is proposed only where no piece of exactly that character's
//                   bytes starts at s; consecutive unknowns of a word fuse.  The table holds every piece as its UTF-8 bytes.
// A text that cannot be done here (malformed UTF-8, a host-only code point, more than kMaxTextBytes, a normalised text beyond the
// buffer) is reported as such (-1) and never given a wrong id; nothing is read past the text's own end.
constexpr int kMaxTextBytes = 4096;         // UTF-8 bytes of one text
constexpr int kUtf8BufBytes = 5120;         // the leading 0x20 + the normalised UTF-8 of one text (the kernel's LDS buffer per wave)
constexpr int kReach = 64;                  // longest piece (bytes, metaspace included) the UTF-8 entries match
constexpr int kPages = 0x1100;              // 256 code points per page, U+0000 .. U+10FFFF

// One uint32 per code point: bits 0-1 kind, bits 2-7 image length in bytes (<= 63), bits 8-31 image offset in the blob.
enum { kIdentity = 0, kRemoved = 1, kImage = 2, kHostOnly = 3 };

// ac_unigram_unicode: page_of[cp >> 8] names one of n_pages pages of 256 entries (identical pages are stored once).
struct Unicode {
    const uint16_t* page_of;    // [kPages]
    const uint32_t* entries;    // [n_pages][256]
    const uint8_t* images;      // [image_bytes]
    int n_pages, image_bytes;
};

UNI_HD bool is_cont(uint8_t c) { return (c & 0xC0) == 0x80; }
// bytes of the character whose lead byte is c (normalised text is well-formed; anything else counts as one byte)
UNI_HD int char_len(uint8_t c) { return c < 0xC0 ? 1 : c < 0xE0 ? 2 : c < 0xF0 ? 3 : 4; }

// Strict UTF-8: the length of the sequence that starts at p (`avail` bytes are left of the text) and its code point; 0 for a
// continuation byte, a truncated sequence, an overlong form, an encoded surrogate or a value above U+10FFFF.
UNI_HD int decode(const uint8_t* p, int avail, uint32_t& cp) {
    const uint32_t b0 = p[0];
    if (b0 < 0x80) { cp = b0; return 1; }
    int len;
    uint32_t lo;
    if (b0 >= 0xC2 && b0 <= 0xDF) { len = 2; cp = b0 & 0x1f; lo = 0x80; }
    else if ((b0 & 0xF0) == 0xE0) { len = 3; cp = b0 & 0x0f; lo = 0x800; }
    else if (b0 >= 0xF0 && b0 <= 0xF4) { len = 4; cp = b0 & 0x07; lo = 0x10000; }
    else return 0;
    if (len > avail) return 0;
    for (int i = 1; i < len; ++i) {
        const uint32_t b = p[i];
        if ((b & 0xC0) != 0x80) return 0;
        cp = (cp << 6) | (b & 0x3f);
    }
    if (cp < lo || cp > 0x10FFFF || (cp >= 0xD800 && cp <= 0xDFFF)) return 0;
    return len;
}

UNI_HD int kind_of(uint32_t e) { return (int)(e & 3); }
UNI_HD int image_len(uint32_t e) { return (int)((e >> 2) & 63); }
UNI_HD uint32_t image_off(uint32_t e) { return e >> 8; }

// The entry of a code point <= U+10FFFF.  A page number or an image that points outside the tables reads as host-only.
UNI_HD uint32_t entry(const Unicode& u, uint32_t cp) {
    const uint32_t pg = u.page_of[cp >> 8];
    if (pg >= (uint32_t)u.n_pages) return kHostOnly;
    const uint32_t e = u.entries[pg * 256u + (cp & 255u)];
    if (kind_of(e) == kImage && image_off(e) + (uint32_t)image_len(e) > (uint32_t)u.image_bytes) return kHostOnly;
    return e;
}

// Bytes a code point of `src_len` source bytes puts into the normalised text, -1: host-only.
UNI_HD int out_bytes(uint32_t e, int src_len) {
    const int k = kind_of(e);
    return k == kIdentity ? src_len : k == kRemoved ? 0 : k == kImage ? image_len(e) : -1;
}

// Writes those bytes (out_bytes(e, src_len) > 0 of them) to dst, whitespace as 0x20.
UNI_HD void emit(const Unicode& u, uint32_t e, const uint8_t* src, int src_len, int ws_controls, uint8_t* dst) {
    const bool image = kind_of(e) == kImage;
    const uint8_t* from = image ? u.images + image_off(e) : src;
    const int n = image ? image_len(e) : src_len;
    for (int i = 0; i < n; ++i) dst[i] = is_space(from[i], ws_controls) ? 0x20 : from[i];
}

// The whole normaliser, front to back (the kernel does the same per 64-byte chunk with a prefix sum in between): buf[0] = 0x20,
// the images behind it; bytes written to buf, or -1.
UNI_HD int normalize_utf8(const Unicode& u, const uint8_t* t, int n, int ws_controls, uint8_t* buf, int cap) {
    if (n < 0 || n > kMaxTextBytes || cap < 1) return -1;
    int o = 0;
    buf[o++] = 0x20;
    for (int p = 0; p < n;) {
        uint32_t cp;
        const int len = decode(t + p, n - p, cp);
        if (len == 0) return -1;
        const uint32_t e = entry(u, cp);
        const int k = out_bytes(e, len);
        if (k < 0 || o + k > cap) return -1;
        if (k) emit(u, e, t + p, len, ws_controls, buf + o);
        o += k;
        p += len;
    }
    return o;
}

// encode_word on characters.  w[0, L): the word, metaspace (0x20) first, well-formed UTF-8.  Work arrays as encode_word.
// `aligned` (optional) is cleared if a piece on the winning path starts or ends inside a character: it cannot, starts are taken on
// lead bytes only and pieces are whole characters -- the host entry asserts it.
inline int encode_word_utf8(const Table& t, int max_piece, double unk_score, int unk_id, const uint8_t* w, int L, int room, int total,
                            int64_t* out, double* best, int32_t* from_at, int32_t* id_at, int32_t* next_at, bool* aligned) {
    for (int i = 0; i <= L; ++i) from_at[i] = -1;
    best[0] = 0.0;
    for (int s = 0; s < L; ++s) {
        if (is_cont(w[s])) continue;                        // not a character boundary: no piece starts here
        if (s > 0 && from_at[s] < 0) continue;              // (cannot happen in well-formed text: every boundary is reachable)
        const double bs = best[s];
        int cl = char_len(w[s]);
        if (cl > L - s) cl = L - s;
        bool single = false;
        uint64_t p = 0;
        const int tmax = L - s < max_piece ? L : s + max_piece;
        for (int e = s + 1; e <= tmax; ++e) {
            p = poly_step(p, w[e - 1]);
            if (e < L && is_cont(w[e])) continue;           // inside a character
            int id;
            double score;
            if (!lookup(t, finish(p), w + s, e - s, id, score)) continue;
            if (e == s + cl) single = true;
            const double cand = bs + score;
            if (from_at[e] < 0 || cand > best[e]) { best[e] = cand; from_at[e] = s; id_at[e] = id; }
        }
        if (!single) {
            const double cand = bs + unk_score;
            if (from_at[s + cl] < 0 || cand > best[s + cl]) { best[s + cl] = cand; from_at[s + cl] = s; id_at[s + cl] = kUnkPiece; }
        }
    }
    if (from_at[L] < 0) return total;                       // (a table with a broken image: the word gives nothing)
    for (int e = L; e > 0; e = from_at[e]) {
        if (aligned && ((e < L && is_cont(w[e])) || is_cont(w[from_at[e]]))) *aligned = false;
        next_at[from_at[e]] = e;
    }
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

// One text on one thread (host entry, stand-alone programs; any word length): ids of the pieces between the specials into
// out[0, room); returns their number, or -1 where the text cannot be done.  buf: `cap` bytes for the normalised text; work arrays
// of cap + 1 entries each.
inline int encode_text_utf8(const Unicode& u, const Table& t, int max_piece, double unk_score, int unk_id, int trailing_space_piece,
                            int ws_controls, const uint8_t* text, int n, uint8_t* buf, int cap, int room, int64_t* out, double* best,
                            int32_t* from_at, int32_t* id_at, int32_t* next_at, bool* aligned) {
    const int m = normalize_utf8(u, text, n, ws_controls, buf, cap);
    if (m < 0) return -1;
    int total = 0;
    for (int p = 0; p < m && total < room;) {
        if (!word_start(buf, m, p, trailing_space_piece)) { ++p; continue; }
        int q = p + 1;
        while (q < m && buf[q] != 0x20) ++q;
        total = encode_word_utf8(t, max_piece, unk_score, unk_id, buf + p, q - p, room, total, out, best, from_at, id_at, next_at, aligned);
        p = q;
    }
    return total;
}

}  // namespace unigram
