// GPT-2 byte-level BPE on ASCII text, written once for the kernel (bpe.hip), the host entry point (ac_bpe_encode_host) and any
// plain C++ program: no HIP runtime header is needed, BPE_HD is empty without hipcc.  The second half of the file is the same for
// UTF-8 text (bpe_utf8.hip).
//
//   pre-tokeniser   's|'t|'re|'ve|'m|'ll|'d| ?\p{L}+| ?\p{N}+| ?[^\s\p{L}\p{N}]+|\s+(?!\S)|\s+   restricted to bytes < 128:
//                   whether a token starts at byte p is a function of t[p-4 .. p+2] alone (is_start), so every boundary of a
//                   text can be found in parallel
//   merges          per pre-token: symbols start as single bytes; the adjacent pair of lowest rank (leftmost on ties) is joined
//                   until no adjacent pair is a merge.  A merge is the PAIR (left bytes, right bytes): the table is keyed by
//                   FNV-1a 64 over left, one separator step, right, and a hit is verified byte-exact incl. the split point
//   ids             a single byte: byte_id[byte]; a merged symbol: the id stored with the merge that produced it
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define BPE_HD __host__ __device__ __forceinline__
#else
#define BPE_HD inline
#endif

namespace bpe {

constexpr uint64_t kFnvOffset = 0xcbf29ce484222325ull, kFnvPrime = 0x100000001b3ull;
constexpr uint32_t kPairSeparator = 0x100;      // no byte has this value: ("a","bc") and ("ab","c") hash differently
constexpr int kNoRank = 0x7fffffff;

// The merge table (ac_bpe_vocab without the post-processor's ids): open addressing, linear probing, power-of-two slot count,
// filled to at most half.  slot of a pair = (h ^ (h >> 32)) & mask, h = pair_hash(left, right).
struct Table {
    const uint64_t* keys;       // [slots] stored hash, 0 = empty
    const int32_t* entries;     // [slots][4]: rank, merged id, blob offset of left|right, left_len | total_len << 16
    const uint8_t* blob;        // the merges' bytes (left and right back to back)
    const int32_t* byte_id;     // [256] id of each single-byte symbol
    uint32_t mask;              // slots - 1
};

BPE_HD uint64_t fnv_step(uint64_t h, uint32_t c) { return (h ^ c) * kFnvPrime; }

BPE_HD uint64_t pair_hash(const uint8_t* left, int left_len, const uint8_t* right, int right_len) {
    uint64_t h = kFnvOffset;
    for (int i = 0; i < left_len; ++i) h = fnv_step(h, left[i]);
    h = fnv_step(h, kPairSeparator);
    for (int i = 0; i < right_len; ++i) h = fnv_step(h, right[i]);
    return h == 0 ? 1 : h;
}

// Is (p[0, left_len), p[left_len, total_len)) a merge?  Its rank and the id of the joined symbol.
BPE_HD bool lookup(const Table& t, const uint8_t* p, int left_len, int total_len, int& rank, int& id) {
    const uint64_t h = pair_hash(p, left_len, p + left_len, total_len - left_len);
    const int32_t lens = (int32_t)((uint32_t)left_len | ((uint32_t)total_len << 16));
    uint32_t slot = (uint32_t)(h ^ (h >> 32)) & t.mask;
    for (;;) {
        const uint64_t k = t.keys[slot];
        if (k == 0) return false;
        if (k == h) {
            const int32_t* e = t.entries + 4 * (uint64_t)slot;
            if (e[3] == lens) {
                const uint8_t* b = t.blob + (uint32_t)e[2];
                bool eq = true;
                for (int i = 0; i < total_len; ++i) eq &= b[i] == p[i];
                if (eq) { rank = e[0]; id = e[1]; return true; }
            }
        }
        slot = (slot + 1) & t.mask;
    }
}

// ---- pre-tokeniser ----------------------------------------------------------------------------------------------------
enum { kWs = 0, kLetter = 1, kDigit = 2, kOther = 3 };

BPE_HD int cls(uint8_t c) {
    if (c == 0x20 || (c >= 0x09 && c <= 0x0d)) return kWs;      // \s on bytes < 128; 0x1c-0x1f are not whitespace here
    if ((c >= 'A' && c <= 'Z') || (c >= 'a' && c <= 'z')) return kLetter;
    if (c >= '0' && c <= '9') return kDigit;
    return kOther;
}

// t[p] == '\'': does a token start at this apostrophe?  (After a letter, a digit or a whitespace byte other than 0x20; after
// 0x20 the " ?[^\s\p{L}\p{N}]+" alternative has taken the space and the apostrophe, after an "other" byte the run swallows it.)
BPE_HD bool apos_start(const uint8_t* t, int p) {
    if (p == 0) return true;
    const uint8_t d = t[p - 1];
    const int kd = cls(d);
    return kd == kLetter || kd == kDigit || (kd == kWs && d != 0x20);
}

// t[p] == '\'': bytes of the contraction that begins here ('s 't 'm 'd: 2, 're 've 'll: 3; lower case only), or 0
BPE_HD int contraction_len(const uint8_t* t, int n, int p) {
    if (p + 1 >= n) return 0;
    const uint8_t a = t[p + 1];
    if (a == 's' || a == 't' || a == 'm' || a == 'd') return 2;
    if (p + 2 >= n) return 0;
    const uint8_t b = t[p + 2];
    return ((a == 'r' && b == 'e') || (a == 'v' && b == 'e') || (a == 'l' && b == 'l')) ? 3 : 0;
}

// Does a pre-token start at byte p of t[0, n)?  0 <= p < n.
BPE_HD bool is_start(const uint8_t* t, int n, int p) {
    if (p == 0) return true;
    const uint8_t c = t[p], d = t[p - 1];
    const int k = cls(c), kd = cls(d);
    if (k == kWs) {
        if (kd != kWs) return true;                             // a whitespace run begins
        return p + 1 < n && cls(t[p + 1]) != kWs;               // "\s+(?!\S)" gives the run's last byte back to what follows
    }
    if (kd == kWs) return d != 0x20;                            // " ?X+" takes one 0x20 in front; any other byte stands alone
    if (k != kd)                                                // a run of another class ends here, unless this is 's of a contraction
        return !(d == '\'' && k == kLetter && apos_start(t, p - 1) && contraction_len(t, n, p - 1) != 0);
    if (k == kLetter) {                                         // inside a letter run: a contraction that ended here cuts it
        if (p >= 2 && t[p - 2] == '\'' && apos_start(t, p - 2) && contraction_len(t, n, p - 2) == 2) return true;
        if (p >= 3 && t[p - 3] == '\'' && apos_start(t, p - 3) && contraction_len(t, n, p - 3) == 3) return true;
    }
    return false;
}

// ---- one text on one thread (the host entry point; any pre-token length) ------------------------------------------------
// c[0, n): the text with the prefix space already in place.  Writes up to `room` ids to out, returns how many.
// Work arrays of n entries each: id_at / next_at / rank_at / mid_at, indexed by a symbol's first byte.
inline int encode_text(const Table& t, const uint8_t* c, int n, int room, int64_t* out, int32_t* id_at, int32_t* next_at,
                       int32_t* rank_at, int32_t* mid_at) {
    int total = 0;
    for (int p0 = 0; p0 < n && total < room;) {
        int p1 = p0 + 1;
        while (p1 < n && !is_start(c, n, p1)) ++p1;
        for (int i = p0; i < p1; ++i) { id_at[i] = t.byte_id[c[i]]; next_at[i] = i + 1; }
        auto pair_of = [&](int i) {                             // rank of (symbol at i, symbol after it), kNoRank if none
            rank_at[i] = kNoRank;
            const int j = next_at[i];
            if (j < p1) {
                int r, m;
                if (lookup(t, c + i, j - i, next_at[j] - i, r, m)) { rank_at[i] = r; mid_at[i] = m; }
            }
        };
        for (int i = p0; i < p1; ++i) pair_of(i);
        for (;;) {
            int best = -1, before_best = -1;
            for (int i = p0, prev = -1; i < p1; prev = i, i = next_at[i])
                if (rank_at[i] != kNoRank && (best < 0 || rank_at[i] < rank_at[best])) { best = i; before_best = prev; }
            if (best < 0) break;
            id_at[best] = mid_at[best];
            next_at[best] = next_at[next_at[best]];
            pair_of(best);
            if (before_best >= 0) pair_of(before_best);
        }
        for (int i = p0; i < p1 && total < room; i = next_at[i]) out[total++] = id_at[i];
        p0 = p1;
    }
    return total;
}

// ---- UTF-8 texts (ac_bpe_utf8_encode[_host], ac_version() >= 17) ---------------------------------------------------------------
// The same pipeline over Unicode text, written once for bpe_utf8_kernel (bpe_utf8.hip), ac_bpe_utf8_encode_host and any plain C++
// program.  The merges work on raw bytes and need no change; the only Unicode knowledge of the pipeline is the class of each code
// point in the pre-tokeniser pattern (\s, \p{L}, \p{N}, other), and that comes from a table the host wrapper probes from the
// wrapped pipeline (tokenizer.py, build_bpe_unicode_tables): nothing here knows a Unicode property.
//
//   decoding        strict UTF-8 (decode_utf8): an overlong form, an encoded surrogate, a value above U+10FFFF, a stray
//                   continuation byte or a truncated tail makes the text NOT DONE -- never a guess
//   classes         one byte per text byte (classify_text / the kernel's class pass): bits 0-1 the class of the CHARACTER the byte
//                   belongs to, kContByte on every byte but the character's first.  class_at[p - 1] is thus the class of the
//                   character that ends at p - 1, and every later question is a read of the two arrays
//   host-only       a code point the device does not reproduce (the normalizer changes it or may combine it with its neighbour):
//                   the text is NOT DONE
//   boundaries      is_start_utf8 = is_start stated on characters; pre-token boundaries are character boundaries, so the merge
//                   loop is encode_text's on the same bytes

// ac_bpe_unicode: page_of[cp >> 8] names one of n_pages pages of 256 one-byte entries (identical pages are stored once).
// An entry: bits 0-1 kWs / kLetter / kDigit / kOther, kHostOnly on top.
struct Unicode {
    const uint16_t* page_of;    // [0x1100]
    const uint8_t* entries;     // [n_pages][256]
    int n_pages;
};

constexpr int kClassMask = 3;
constexpr int kHostOnly = 4;    // in a table entry
constexpr int kContByte = 4;    // in a text's class array: not the first byte of its character

BPE_HD bool is_cont(uint8_t c) { return (c & 0xC0) == 0x80; }
// bytes of the character whose lead byte is c (only asked of validated text)
BPE_HD int char_len(uint8_t c) { return c < 0xC0 ? 1 : c < 0xE0 ? 2 : c < 0xF0 ? 3 : 4; }

// Strict UTF-8: the length of the sequence that starts at p (`avail` bytes are left of the text) and its code point; 0 for a
// continuation byte, a truncated sequence, an overlong form, an encoded surrogate or a value above U+10FFFF.  Reads p[0, min(len, avail)).
BPE_HD int decode_utf8(const uint8_t* p, int avail, uint32_t& cp) {
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

// the table entry of a code point <= U+10FFFF; a page number outside the table reads as host-only
BPE_HD int entry_of(const Unicode& u, uint32_t cp) {
    const int page = u.page_of[cp >> 8];
    return page < u.n_pages ? u.entries[(size_t)page * 256 + (cp & 0xff)] : kHostOnly;
}

// t[p] == '\'': does a token start at this apostrophe?  apos_start with the class of the CHARACTER in front.
BPE_HD bool apos_start_utf8(const uint8_t* t, const uint8_t* class_at, int p) {
    if (p == 0) return true;
    const int kd = class_at[p - 1] & kClassMask;
    return kd == kLetter || kd == kDigit || (kd == kWs && t[p - 1] != 0x20);
}

// Does a pre-token start at byte p of t[0, n)?  0 <= p < n; class_at[0, n) as classify_text leaves it.  A continuation byte is
// never a start.  The contraction rules stay on ASCII bytes ('s 't 're ... are ASCII, and 0x27 is no part of a longer
// sequence), with kLetter / kDigit of the neighbours from the table: "é's" cuts like "e's", U+2019 + s is no contraction.
BPE_HD bool is_start_utf8(const uint8_t* t, const uint8_t* class_at, int n, int p) {
    const int kc = class_at[p];
    if (kc & kContByte) return false;
    if (p == 0) return true;
    const uint8_t d = t[p - 1];
    const int k = kc & kClassMask, kd = class_at[p - 1] & kClassMask;
    if (k == kWs) {
        if (kd != kWs) return true;                             // a whitespace run begins
        const int q = p + char_len(t[p]);                       // "\s+(?!\S)" gives the run's last CHARACTER back to what follows
        return q < n && (class_at[q] & kClassMask) != kWs;
    }
    if (kd == kWs) return d != 0x20;                            // " ?X+" takes one 0x20 in front: the byte, no other whitespace
    if (k != kd)
        return !(d == '\'' && k == kLetter && apos_start_utf8(t, class_at, p - 1) && contraction_len(t, n, p - 1) != 0);
    if (k == kLetter) {                                         // a contraction's letters are ASCII: p - 2 / p - 3 are byte offsets
        if (p >= 2 && t[p - 2] == '\'' && apos_start_utf8(t, class_at, p - 2) && contraction_len(t, n, p - 2) == 2) return true;
        if (p >= 3 && t[p - 3] == '\'' && apos_start_utf8(t, class_at, p - 3) && contraction_len(t, n, p - 3) == 3) return true;
    }
    return false;
}

// class_at[0, n) of the text c[0, n); false = NOT DONE (malformed UTF-8 or a host-only code point; class_at is then undefined)
inline bool classify_text(const Unicode& u, const uint8_t* c, int n, uint8_t* class_at) {
    for (int p = 0; p < n;) {
        uint32_t cp;
        const int len = decode_utf8(c + p, n - p, cp);
        if (len == 0) return false;
        const int e = entry_of(u, cp);
        if (e & kHostOnly) return false;
        class_at[p] = (uint8_t)(e & kClassMask);
        for (int i = 1; i < len; ++i) class_at[p + i] = (uint8_t)((e & kClassMask) | kContByte);
        p += len;
    }
    return true;
}

// encode_text over is_start_utf8: one text on one thread, any pre-token length.  c[0, n) with the prefix space in place;
// class_at: n bytes of work space.  Returns the number of ids written, or -1: NOT DONE (nothing of `out` is then meaningful).
inline int encode_text_utf8(const Table& t, const Unicode& u, const uint8_t* c, int n, int room, int64_t* out, uint8_t* class_at,
                            int32_t* id_at, int32_t* next_at, int32_t* rank_at, int32_t* mid_at) {
    if (!classify_text(u, c, n, class_at)) return -1;
    int total = 0;
    for (int p0 = 0; p0 < n && total < room;) {
        int p1 = p0 + 1;
        while (p1 < n && !is_start_utf8(c, class_at, n, p1)) ++p1;
        for (int i = p0; i < p1; ++i) { id_at[i] = t.byte_id[c[i]]; next_at[i] = i + 1; }
        auto pair_of = [&](int i) {                             // as in encode_text
            rank_at[i] = kNoRank;
            const int j = next_at[i];
            if (j < p1) {
                int r, m;
                if (lookup(t, c + i, j - i, next_at[j] - i, r, m)) { rank_at[i] = r; mid_at[i] = m; }
            }
        };
        for (int i = p0; i < p1; ++i) pair_of(i);
        for (;;) {
            int best = -1, before_best = -1;
            for (int i = p0, prev = -1; i < p1; prev = i, i = next_at[i])
                if (rank_at[i] != kNoRank && (best < 0 || rank_at[i] < rank_at[best])) { best = i; before_best = prev; }
            if (best < 0) break;
            id_at[best] = mid_at[best];
            next_at[best] = next_at[next_at[best]];
            pair_of(best);
            if (before_best >= 0) pair_of(before_best);
        }
        for (int i = p0; i < p1 && total < room; i = next_at[i]) out[total++] = id_at[i];
        p0 = p1;
    }
    return total;
}

}  // namespace bpe
