// BERT WordPiece on UTF-8 text, written once for the kernel (wordpiece_utf8_kernel in wordpiece.hip), the host entry point
// (ac_wordpiece_encode_utf8_host) and any plain C++ program: no HIP runtime header is needed, WPU_HD is empty without hipcc.
//
//   normaliser      BertNormalizer (clean_text, CJK spacing, NFD + dropping Mn, per-character lower-casing) acts code point by
//                   code point, so it is a TABLE: code point -> identity | removed | image (bytes in a blob) | " cp " (CJK) |
//                   host-only.  The table is built by probing the wrapped tokenizers pipeline itself (tokenizer.py,
//                   build_wordpiece_unicode_tables); nothing here knows a Unicode property.  The one context dependence -- NFD
//                   reorders combining marks -- is kept out by the host-only flag: a text holding such a code point is not done.
//   pre-tokeniser   BertPreTokenizer: every code point that can occur in normalised text carries its class in the same table
//                   (space | punctuation | word character); punctuation stands alone, word characters run together
//   WordPiece       greedy longest-match-first per word over CHARACTER boundaries, continuation pieces under the "##" hash,
//                   a word of more than 100 characters (not bytes) or with an unmatched remainder -> [UNK].  The vocabulary is
//                   ac_wordpiece_vocab's hash table, unchanged: FNV-1a 64 over the piece's UTF-8 bytes.
// A text that cannot be done here (malformed UTF-8, a host-only code point, a normalised text longer than the caller's buffer, more
// than kMaxTextBytes) is reported as such (-1) and never given a wrong id; nothing is read past the text's own end.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define WPU_HD __host__ __device__ __forceinline__
#else
#define WPU_HD inline
#endif

namespace wpu {

constexpr uint64_t kFnvOffset = 0xcbf29ce484222325ull, kFnvPrime = 0x100000001b3ull;
constexpr int kMaxWordChars = 100;          // tokenizers WordPiece max_input_chars_per_word
constexpr int kMaxTextBytes = 4096;         // UTF-8 bytes of one text
constexpr int kBufBytes = 8192;             // normalised UTF-8 of one text (the kernel's LDS buffer per wave; the host entry uses the same)
constexpr int kPages = 0x1100;              // 256 code points per page, U+0000 .. U+10FFFF

// One uint32 per code point: bits 0-2 kind, bits 3-4 class of the code point where it occurs in normalised text,
// bits 5-8 image length in bytes, bits 9-31 image offset in the blob.
enum { kIdentity = 0, kRemoved = 1, kImage = 2, kHostOnly = 3, kPadded = 4 };      // kPadded: 0x20, the code point, 0x20
enum { kNoClass = 0, kSpace = 1, kPunct = 2, kWord = 3 };

// ac_wordpiece_unicode: page_of[cp >> 8] names one of n_pages pages of 256 entries (identical pages are stored once).
struct Unicode {
    const uint16_t* page_of;    // [kPages]
    const uint32_t* entries;    // [n_pages][256]
    const uint8_t* images;      // [image_bytes]
    int n_pages, image_bytes;
};

// ac_wordpiece_vocab as the matcher reads it
struct Vocab {
    const uint64_t* keys;
    const uint32_t* offs;
    const int32_t* ids;
    const uint16_t* lens;
    const uint8_t* blob;
    uint32_t mask;
    int max_piece;
    int unk_id, cls_id, sep_id, pad_id;
};

WPU_HD uint64_t fnv_step(uint64_t h, uint8_t c) { return (h ^ c) * kFnvPrime; }
WPU_HD bool is_cont(uint8_t c) { return (c & 0xC0) == 0x80; }

// Strict UTF-8: the length of the sequence that starts at p (`avail` bytes are left of the text) and its code point; 0 for a
// continuation byte, a truncated sequence, an overlong form, an encoded surrogate or a value above U+10FFFF.
WPU_HD int decode(const uint8_t* p, int avail, uint32_t& cp) {
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

WPU_HD int kind_of(uint32_t e) { return (int)(e & 7); }
WPU_HD int class_of(uint32_t e) { return (int)((e >> 3) & 3); }
WPU_HD int image_len(uint32_t e) { return (int)((e >> 5) & 15); }
WPU_HD uint32_t image_off(uint32_t e) { return e >> 9; }

// The entry of a code point <= U+10FFFF.  A page number or an image that points outside the tables reads as host-only.
WPU_HD uint32_t entry(const Unicode& u, uint32_t cp) {
    const uint32_t pg = u.page_of[cp >> 8];
    if (pg >= (uint32_t)u.n_pages) return kHostOnly;
    const uint32_t e = u.entries[pg * 256u + (cp & 255u)];
    if (kind_of(e) == kImage && image_off(e) + (uint32_t)image_len(e) > (uint32_t)u.image_bytes) return kHostOnly;
    return e;
}

// Bytes a code point of `src_len` source bytes puts into the normalised text, -1: host-only.
WPU_HD int out_bytes(uint32_t e, int src_len) {
    switch (kind_of(e)) {
        case kIdentity: return src_len;
        case kRemoved: return 0;
        case kImage: return image_len(e);
        case kPadded: return src_len + 2;
        default: return -1;
    }
}

// Writes those bytes (out_bytes(e, src_len) > 0 of them) to dst.
WPU_HD void emit(const Unicode& u, uint32_t e, const uint8_t* src, int src_len, uint8_t* dst) {
    const int k = kind_of(e);
    if (k == kImage) {
        const uint8_t* im = u.images + image_off(e);
        const int n = image_len(e);
        for (int i = 0; i < n; ++i) dst[i] = im[i];
    } else {
        if (k == kPadded) { dst[0] = 0x20; dst[src_len + 1] = 0x20; ++dst; }
        for (int i = 0; i < src_len; ++i) dst[i] = src[i];
    }
}

// The whole normaliser, front to back (the kernel does the same per 64-byte chunk with a prefix sum in between):
// bytes written to buf, or -1.
WPU_HD int normalize(const Unicode& u, const uint8_t* t, int n, uint8_t* buf, int cap) {
    int o = 0;
    for (int p = 0; p < n;) {
        uint32_t cp;
        const int len = decode(t + p, n - p, cp);
        if (len == 0) return -1;
        const uint32_t e = entry(u, cp);
        const int k = out_bytes(e, len);
        if (k < 0 || o + k > cap) return -1;
        if (k) emit(u, e, t + p, len, buf + o);
        o += k;
        p += len;
    }
    return o;
}

// ---- normalised text c[0, n): classes, words -----------------------------------------------------------------------------------
// Class and byte length of the character at c[p] (p on a lead byte).  Normalised text is well-formed and made of code points with
// a class by construction; whatever else a broken table could leave here counts as a one-byte word character.
WPU_HD int class_at(const Unicode& u, const uint8_t* c, int n, int p, int& len) {
    uint32_t cp;
    len = decode(c + p, n - p, cp);
    if (len == 0) { len = 1; return kWord; }
    const int k = class_of(entry(u, cp));
    return k == kNoClass ? kWord : k;
}

// Does a word start at p (class k)?  A punctuation character always, a word character after anything but a word character.
WPU_HD bool is_start(const Unicode& u, const uint8_t* c, int n, int p, int k) {
    if (k == kPunct) return true;
    if (k != kWord) return false;
    if (p == 0) return true;
    int q = p - 1;
    while (q > 0 && p - q < 4 && is_cont(c[q])) --q;
    int len;
    return class_at(u, c, n, q, len) != kWord;
}

// Bytes of the word of word characters that starts at p (its first character is `first_len` bytes); `chars` counts its
// characters and stops at kMaxWordChars + 1 (the word is [UNK] then, its full extent does not matter: the characters behind
// are no word starts).
WPU_HD int word_extent(const Unicode& u, const uint8_t* c, int n, int p, int first_len, int& chars) {
    int q = p + first_len;
    chars = 1;
    while (q < n && chars <= kMaxWordChars) {
        int len;
        if (class_at(u, c, n, q, len) != kWord) break;
        q += len;
        ++chars;
    }
    return q - p;
}

// id of the piece p[0, len) (continuation iff cont), or -1
WPU_HD int lookup(const Vocab& t, uint64_t h, const uint8_t* p, int len, bool cont) {
    if (h == 0) h = 1;
    uint32_t slot = (uint32_t)(h ^ (h >> 32)) & t.mask;
    for (;;) {                                             // ends: the table is at most half full
        const uint64_t k = t.keys[slot];
        if (k == 0) return -1;
        if (k == h && t.lens[slot] == len) {
            const int32_t v = t.ids[slot];
            if (((v >> 30) & 1) == (cont ? 1 : 0)) {
                const uint8_t* b = t.blob + t.offs[slot];
                bool eq = true;
                for (int i = 0; i < len; ++i) eq &= b[i] == p[i];
                if (eq) return v & 0x3fffffff;
            }
        }
        slot = (slot + 1) & t.mask;
    }
}

// Greedy longest-match-first over one word of `len` bytes / `chars` characters; a piece ends only where a character ends.
// out == nullptr: returns the number of pieces (1 for [UNK]).  Otherwise `expect` is that count and up to `room` ids are
// written (a word whose count is 1 is [UNK] unless its first match covers it whole; a count > 1 means every piece matches,
// so ids can be written as they are found).
WPU_HD int match(const Vocab& t, const uint8_t* w, int len, int chars, int64_t* out, int room, int expect) {
    if (chars > kMaxWordChars) { if (out && room > 0) out[0] = t.unk_id; return 1; }
    int n = 0, s = 0;
    while (s < len) {
        uint64_t h = kFnvOffset;
        if (s > 0) { h = fnv_step(h, '#'); h = fnv_step(h, '#'); }
        int best_e = -1, best_id = -1;
        const int emax = len - s < t.max_piece ? len : s + t.max_piece;
        for (int e = s; e < emax; ++e) {
            h = fnv_step(h, w[e]);
            if (e + 1 < len && is_cont(w[e + 1])) continue;          // inside a character
            const int id = lookup(t, h, w + s, e + 1 - s, s > 0);
            if (id >= 0) { best_e = e + 1; best_id = id; }
        }
        if (best_e < 0) { if (out && room > 0) out[0] = t.unk_id; return 1; }      // whole word -> [UNK]
        if (out && expect == 1) {                                                      // single slot: the word or [UNK]
            if (room > 0) out[0] = best_e == len ? best_id : t.unk_id;
            return 1;
        }
        if (out && n < room) out[n] = best_id;
        ++n;
        s = best_e;
    }
    return n;
}

// One text on one thread (host entry, stand-alone programs): ids of the pieces between the specials into out[0, room), at most
// `room`; returns their number, or -1 where the text cannot be done.  buf: `cap` bytes for the normalised text.
inline int encode_text(const Unicode& u, const Vocab& v, const uint8_t* t, int n, uint8_t* buf, int cap, int room, int64_t* out) {
    if (n < 0 || n > kMaxTextBytes) return -1;
    const int m = normalize(u, t, n, buf, cap);
    if (m < 0) return -1;
    int total = 0;
    for (int p = 0; p < m && total < room;) {
        int len;
        const int k = class_at(u, buf, m, p, len);
        if (!is_start(u, buf, m, p, k)) { p += len; continue; }
        int chars = 1;
        const int wb = k == kPunct ? len : word_extent(u, buf, m, p, len, chars);
        const int cnt = match(v, buf + p, wb, chars, nullptr, 0, 0);
        match(v, buf + p, wb, chars, out + total, room - total, cnt);
        total += cnt;
        p += wb;
    }
    return total < room ? total : room;
}

}  // namespace wpu
