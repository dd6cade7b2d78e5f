// Frame filters: a small n-gram Bloom filter a frame of a record archive, consulted BEFORE a frame is decoded - a search for a request id
// that lies in a few dozen of 16 000 frames need not decode the others to learn that they hold nothing.  The filter of an archive is one
// skippable frame the caller keeps BESIDE the archive, as a file or blob of its own.
//   THE RULE.  Content of `size` bytes, frames at content offsets dOff[0 .. N], dOff[N] = size, a delimiter byte delim, a gram length g in
//   {3, 4} and a filter size L = log2 of the bits a frame, 9 .. 16:
//    1. fold(b) = b + 0x20 for b in 'A' .. 'Z', b otherwise - the query calls' fold (zsmi_findquery.h), here ALWAYS applied: one filter
//       serves searches with and without ZSMI_FIND_IGNORE_CASE.  Bytes of 0x80 and above are never touched.
//    2. A GRAM of frame i is g consecutive bytes that lie wholly inside frame i and none of which equals delim, unfolded.
//    3. Its VALUE v is the little-endian integer of its folded bytes.
//    4. Its BITS are h_k = (uint32_t)(v * C_k) >> (32 - L), C_0 = 0x9E3779B1, C_1 = 0x85EBCA77.  Bit h is bit h & 7 of byte h >> 3 of the
//       frame's SLOT of 2^(L - 3) bytes.
//    5. A border x is CLEAN when x == 0, x == size or content[x - 1] == delim.
//    6. A non-empty frame with a border that is not clean is SATURATED: its slot is all ones.  Such a frame holds a piece of a record that
//       another frame holds too; cut records and fixed-size frames over text produce them.
//    7. An empty frame's slot is all zeros.  Every other frame's slot is the OR of its grams' bits.
//    8. A pattern of m >= g bytes, none equal to the delimiter's fold (the query calls' rule 3), PASSES frame i when every bit of every one
//       of its m - g + 1 grams - folded, rule 1 - is set in slot i.
//    9. A pattern with m < g says nothing to the filter: it passes every frame.
//   10. A query passes a frame - any: some pattern passes; all: every pattern passes; none: every frame, because the filter cannot help.
//   11. NO FALSE NEGATIVES.  A record lies inside one clean frame or inside a run of saturated frames: a frame with two clean borders
//       holds whole records only, and a record that crosses a border makes that border unclean for both frames beside it.  An occurrence
//       lies inside one record (rule 8: it holds no delimiter), so inside a clean frame every one of its grams is a gram of that frame
//       and its bits are set; a saturated frame passes everything.  So a frame that holds any part of a record satisfying an `any` or
//       `all` query always passes.
//   Rules 9 and 10 and EMPTY FRAMES.  The filter frame records no frame sizes, and a frame without a gram - "ab\ncd\n" under g = 4 - has
//   the slot of an empty one, all zeros.  A pattern shorter than g can occur in such a frame, so what a filter alone can say of a short
//   pattern or of `none` is "every frame", the empty ones included; an empty frame in a list costs its search nothing.
//   THE FRAME.  A self-contained skippable frame in the style of the record index frame (zsmi_recindex.h), little-endian:
//          0  u32 0x184D2A5C     4  u32 Frame_Size = 32 + N * 2^(L-3)     8  u32 0x52544C46 "FLTR"     12  u8 version = 1, u8 delim, u8 g, u8 L
//         16  u32 N     20  u32 0     24  u64 size     32  u64 check     40  N slots
//      check = sum over the slots' 64-bit words w_k (k counts through all slots) of (w_k + 1) (2 k + 1) 0x9E3779B185EBCA87, + size *
//      0xC2B2AE3D27D4EB4F + delim + (g << 8) + (L << 16), mod 2^64: a sum, so that a grid computes it in any order.
//   NOT COVERED: filters for regular expressions, the filter inside the archive (the record index frame is defined as the table's last
//   entry), Bloom parameters other than two hashes.
// Host and device; a host program may include this header alone, with any C++ compiler (tests/c/frame_filter.cpp does, under the
// sanitizers).  The host forms below are what zsmi_frameFilterSize, zsmi_buildFrameFilter, zsmi_readFrameFilter and zsmi_filterFrames
// run; the kernels of filter.hip share the constants, zs_flt_fold4, zs_flt_bit, zs_flt_term and zs_flt_read_header.
#pragma once
#include "zsmi_findquery.h"       // the query, its checks (zs_findq_check) and ZS_FIND_FN
#include <string.h>

#define ZS_FLT_MAGIC     0x184D2A5Cu              // a skippable frame's magic, variant 0xC (the record index's is 0xD, the seek table's 0xE)
#define ZS_FLT_INNER     0x52544C46u              // "FLTR"
#define ZS_FLT_VERSION   1u
#define ZS_FLT_FIXED     40u                      // the frame without its slots
#define ZS_FLT_C0        0x9E3779B1u
#define ZS_FLT_C1        0x85EBCA77u
#define ZS_FLT_K1        0x9E3779B185EBCA87ull
#define ZS_FLT_K2        0xC2B2AE3D27D4EB4Full
#define ZS_FLT_MIN_LOG   9u
#define ZS_FLT_MAX_LOG   16u
#define ZS_FLT_MAX_GRAMS 254u                     // 8 patterns of 256 bytes together hold at most 256 - 2 grams of 3 bytes

ZS_FIND_FN uint32_t zs_flt_slot_bytes(uint32_t L) { return 1u << (L - 3u); }
ZS_FIND_FN uint64_t zs_flt_frame_size(uint64_t n, uint32_t L) { return ZS_FLT_FIXED + n * zs_flt_slot_bytes(L); }
ZS_FIND_FN bool zs_flt_params_ok(int delim, uint32_t g, uint32_t L) { return delim >= 0 && delim <= 255 && (g == 3u || g == 4u) && L >= ZS_FLT_MIN_LOG && L <= ZS_FLT_MAX_LOG; }
// Frame_Size is a 32-bit field, N too
ZS_FIND_FN bool zs_flt_count_ok(uint64_t n, uint32_t L) { return n <= 0xFFFFFFFFull && 32ull + n * zs_flt_slot_bytes(L) <= 0xFFFFFFFFull; }
// rule 1 on four bytes at once: a byte folds when its high bit is clear and its low seven lie in 'A' .. 'Z' (no sum carries into the next byte)
ZS_FIND_FN uint32_t zs_flt_fold4(uint32_t x)
{
    const uint32_t low = x & 0x7F7F7F7Fu, geA = low + 0x3F3F3F3Fu, gtZ = low + 0x25252525u;
    return x + (((geA & ~gtZ & ~x) & 0x80808080u) >> 2);
}
// rules 3 and 4: the value of g folded bytes (the low g bytes of v4, the others cleared here) and its bit k
ZS_FIND_FN uint32_t zs_flt_value(uint32_t folded4, uint32_t g) { return g == 4u ? folded4 : folded4 & 0xFFFFFFu; }
ZS_FIND_FN uint32_t zs_flt_bit(uint32_t v, uint32_t k, uint32_t L) { return (uint32_t)(v * (k ? ZS_FLT_C1 : ZS_FLT_C0)) >> (32u - L); }
// word k's term of the check, and what the header's fields add
ZS_FIND_FN uint64_t zs_flt_term(uint64_t w, uint64_t k) { return (w + 1ull) * (2ull * k + 1ull) * ZS_FLT_K1; }
ZS_FIND_FN uint64_t zs_flt_check_base(uint64_t size, uint32_t delim, uint32_t g, uint32_t L) { return size * ZS_FLT_K2 + delim + (g << 8) + (L << 16); }

ZS_FIND_FN uint32_t zs_flt_rd32(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
ZS_FIND_FN uint64_t zs_flt_rd64(const uint8_t *p) { return (uint64_t)zs_flt_rd32(p) | ((uint64_t)zs_flt_rd32(p + 4) << 32); }
ZS_FIND_FN void zs_flt_wr32(uint8_t *p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24); }
ZS_FIND_FN void zs_flt_wr64(uint8_t *p, uint64_t v) { zs_flt_wr32(p, (uint32_t)v); zs_flt_wr32(p + 4, (uint32_t)(v >> 32)); }
// the 40 fixed bytes
ZS_FIND_FN void zs_flt_write_header(uint8_t *dst, uint32_t n, uint32_t delim, uint32_t g, uint32_t L, uint64_t size, uint64_t check)
{
    zs_flt_wr32(dst, ZS_FLT_MAGIC); zs_flt_wr32(dst + 4, 32u + n * zs_flt_slot_bytes(L)); zs_flt_wr32(dst + 8, ZS_FLT_INNER);
    zs_flt_wr32(dst + 12, ZS_FLT_VERSION | (delim << 8) | (g << 16) | (L << 24)); zs_flt_wr32(dst + 16, n); zs_flt_wr32(dst + 20, 0);
    zs_flt_wr64(dst + 24, size); zs_flt_wr64(dst + 32, check);
}
// What the fixed bytes say, in zsmi_readFrameFilter's order (srcSize >= ZS_FLT_FIXED: the caller's check): 0 with the fields, or the code.
// The last check holds the frame's bytes against srcSize: every slot the fields name lies inside src
struct ZsFltHeader { uint32_t n, delim, g, L; uint64_t size; };
ZS_FIND_FN int zs_flt_read_header(const uint8_t *src, uint64_t srcSize, ZsFltHeader *h)
{
    if (zs_flt_rd32(src) != ZS_FLT_MAGIC || zs_flt_rd32(src + 8) != ZS_FLT_INNER) return ZSMI_error_prefix_unknown;
    if (src[12] != ZS_FLT_VERSION) return ZSMI_error_version_unsupported;
    const uint32_t g = src[14], L = src[15], n = zs_flt_rd32(src + 16);
    if (!zs_flt_params_ok(src[13], g, L) || zs_flt_rd32(src + 20) || !zs_flt_count_ok(n, L)) return ZSMI_error_corruption_detected;
    if (zs_flt_rd32(src + 4) != 32u + n * zs_flt_slot_bytes(L)) return ZSMI_error_corruption_detected;
    if (srcSize < zs_flt_frame_size(n, L)) return ZSMI_error_srcSize_wrong;
    h->n = n; h->delim = src[13]; h->g = g; h->L = L; h->size = zs_flt_rd64(src + 24);
    return 0;
}
// rule 5 over content[0, size)
ZS_FIND_FN bool zs_flt_clean(const uint8_t *content, uint64_t size, uint64_t x, uint32_t delim) { return x == 0 || x == size || content[x - 1] == (uint8_t)delim; }

// A query against the filter (rules 8 - 10), prepared once a call: the distinct work is the patterns' gram values, folded
struct ZsFltQuery { uint32_t mode, nPatterns, everyFrame, nGrams; uint32_t first[ZSMI_FIND_MAX_PATTERNS + 1]; uint32_t v[ZS_FLT_MAX_GRAMS]; };
// (q checked by zs_findq_check against the filter's delimiter).  everyFrame: the filter says nothing - `none`, an `any` query with a short
// pattern, an `all` query of short patterns only.  Otherwise first[j] .. first[j + 1] are pattern j's grams (none: a short pattern)
static inline void zs_flt_query(const zsmi_findQuery *q, uint32_t g, ZsFltQuery *Q)
{
    Q->mode = q->mode; Q->nPatterns = q->nPatterns; Q->nGrams = 0;
    uint32_t shortOnes = 0;
    for (uint32_t j = 0; j < q->nPatterns; j++) {
        const uint8_t *P = (const uint8_t *)q->patterns[j];
        const uint32_t m = q->patternSizes[j];
        Q->first[j] = Q->nGrams;
        if (m < g) { shortOnes++; continue; }
        for (uint32_t p = 0; p + g <= m; p++) {
            uint32_t x = 0;
            for (uint32_t i = 0; i < g; i++) x |= (uint32_t)P[p + i] << (8u * i);
            Q->v[Q->nGrams++] = zs_flt_value(zs_flt_fold4(x), g);
        }
    }
    Q->first[q->nPatterns] = Q->nGrams;
    Q->everyFrame = q->mode == ZSMI_find_none || (q->mode == ZSMI_find_any && shortOnes) || (q->mode == ZSMI_find_all && shortOnes == q->nPatterns) ? 1u : 0u;
}
// bit h of a slot
ZS_FIND_FN bool zs_flt_has(const uint8_t *slot, uint32_t h) { return ((slot[h >> 3] >> (h & 7u)) & 1u) != 0u; }
// rules 8 - 10 for one slot
ZS_FIND_FN bool zs_flt_passes(const uint8_t *slot, uint32_t L, const ZsFltQuery *Q)
{
    if (Q->everyFrame) return true;
    for (uint32_t j = 0; j < Q->nPatterns; j++) {
        const uint32_t a = Q->first[j], b = Q->first[j + 1];
        bool pass = true;                                                  // (a short pattern: no gram, it passes)
        for (uint32_t k = a; k < b && pass; k++) pass = zs_flt_has(slot, zs_flt_bit(Q->v[k], 0, L)) && zs_flt_has(slot, zs_flt_bit(Q->v[k], 1, L));
        if (Q->mode == ZSMI_find_any ? pass && b > a : !pass) return Q->mode == ZSMI_find_any;
    }
    return Q->mode == ZSMI_find_all;
}
ZS_FIND_FN bool zs_flt_all_ones(const uint8_t *slot, uint32_t bytes)
{
    for (uint32_t i = 0; i < bytes; i++) if (slot[i] != 0xFFu) return false;
    return true;
}

// ---- the host forms ----
#define ZS_FLT_ERR(code) ((size_t)0 - (size_t)(code))
// zsmi_frameFilterSize
static inline size_t zs_flt_size(size_t n, uint32_t L)
{
    if (L < ZS_FLT_MIN_LOG || L > ZS_FLT_MAX_LOG) return ZS_FLT_ERR(ZSMI_error_parameter_outOfBound);
    return zs_flt_count_ok(n, L) ? (size_t)zs_flt_frame_size(n, L) : ZS_FLT_ERR(ZSMI_error_frameIndex_tooLarge);
}
// zsmi_buildFrameFilter: THE RULE over plain text, serially; frame i holds frameSizes[i] bytes.  The frame's size or (size_t)-code;
// nothing is written on failure, nothing behind dst[size), nothing outside src[0, srcSize) is read
static inline size_t zs_flt_build(void *dstv, size_t cap, const void *srcv, uint64_t srcSize, const uint32_t *frameSizes, uint64_t n, int delim, uint32_t g, uint32_t L)
{
    if (!zs_flt_params_ok(delim, g, L)) return ZS_FLT_ERR(ZSMI_error_parameter_outOfBound);
    if (!zs_flt_count_ok(n, L)) return ZS_FLT_ERR(ZSMI_error_frameIndex_tooLarge);
    if (!dstv || (n && !frameSizes)) return ZS_FLT_ERR(ZSMI_error_GENERIC);
    if (srcSize && !srcv) return ZS_FLT_ERR(ZSMI_error_srcSize_wrong);
    uint64_t sum = 0;
    for (uint64_t i = 0; i < n; i++) sum += frameSizes[i];
    if (sum != srcSize) return ZS_FLT_ERR(ZSMI_error_srcSize_wrong);
    const uint64_t total = zs_flt_frame_size(n, L);
    if (cap < total) return ZS_FLT_ERR(ZSMI_error_dstSize_tooSmall);
    const uint8_t *src = (const uint8_t *)srcv;
    uint8_t *dst = (uint8_t *)dstv;
    const uint32_t bytes = zs_flt_slot_bytes(L);
    uint64_t at = 0;
    for (uint64_t i = 0; i < n; i++) {
        uint8_t *slot = dst + ZS_FLT_FIXED + i * bytes;
        const uint64_t end = at + frameSizes[i];
        if (end == at) memset(slot, 0, bytes);
        else if (!zs_flt_clean(src, srcSize, at, (uint32_t)delim) || !zs_flt_clean(src, srcSize, end, (uint32_t)delim)) memset(slot, 0xFF, bytes);
        else {
            memset(slot, 0, bytes);
            for (uint64_t p = at; p + g <= end; p++) {
                uint32_t x = 0; bool holds = false;
                for (uint32_t k = 0; k < g; k++) { holds |= src[p + k] == (uint8_t)delim; x |= (uint32_t)src[p + k] << (8u * k); }
                if (holds) continue;
                const uint32_t v = zs_flt_value(zs_flt_fold4(x), g);
                for (uint32_t k = 0; k < 2; k++) { const uint32_t h = zs_flt_bit(v, k, L); slot[h >> 3] |= (uint8_t)(1u << (h & 7u)); }
            }
        }
        at = end;
    }
    uint64_t check = zs_flt_check_base(srcSize, (uint32_t)delim, g, L);
    for (uint64_t k = 0; k < n * (bytes / 8u); k++) check += zs_flt_term(zs_flt_rd64(dst + ZS_FLT_FIXED + 8u * k), k);
    zs_flt_write_header(dst, (uint32_t)n, (uint32_t)delim, g, L, srcSize, check);
    return (size_t)total;
}
// zsmi_readFrameFilter: 0 with *info, or the code.  Reads only src[0, 40 + N * 2^(L-3))
static inline int zs_flt_read(const void *srcv, size_t srcSize, zsmi_frameFilterInfo *info)
{
    const uint8_t *src = (const uint8_t *)srcv;
    if (!info) return ZSMI_error_GENERIC;
    if (!src || srcSize < ZS_FLT_FIXED) return ZSMI_error_srcSize_wrong;
    ZsFltHeader h;
    if (const int e = zs_flt_read_header(src, srcSize, &h)) return e;
    const uint32_t bytes = zs_flt_slot_bytes(h.L);
    uint64_t check = zs_flt_check_base(h.size, h.delim, h.g, h.L), saturated = 0;
    for (uint64_t k = 0; k < (uint64_t)h.n * (bytes / 8u); k++) check += zs_flt_term(zs_flt_rd64(src + ZS_FLT_FIXED + 8u * k), k);
    if (check != zs_flt_rd64(src + 32)) return ZSMI_error_corruption_detected;
    for (uint32_t i = 0; i < h.n; i++) saturated += zs_flt_all_ones(src + ZS_FLT_FIXED + (uint64_t)i * bytes, bytes) ? 1u : 0u;
    info->nFrames = h.n; info->delim = h.delim; info->gram = h.g; info->log2Bits = h.L; info->size = h.size; info->saturated = saturated;
    return 0;
}
// zsmi_filterFrames: the ascending numbers of the frames of [firstFrame, firstFrame + frameCount) that pass q.  0 or the code; result =
// {total, written, frames tested, the all-ones slots among the total}; nothing is written behind frames[capacity)
static inline int zs_flt_filter(const void *filterv, size_t filterSize, const zsmi_findQuery *q, uint32_t firstFrame, uint32_t frameCount,
                                uint32_t *frames, size_t capacity, uint64_t *result)
{
    const uint8_t *f = (const uint8_t *)filterv;
    if (!q || !result || (capacity && !frames)) return ZSMI_error_GENERIC;
    if (!f || filterSize < ZS_FLT_FIXED) return ZSMI_error_srcSize_wrong;
    ZsFltHeader h;
    if (const int e = zs_flt_read_header(f, filterSize, &h)) return e;
    if (const int e = zs_findq_check((int)h.delim, q)) return e;
    if ((uint64_t)firstFrame + frameCount > h.n) return ZSMI_error_parameter_outOfBound;
    ZsFltQuery Q;
    zs_flt_query(q, h.g, &Q);
    const uint32_t bytes = zs_flt_slot_bytes(h.L);
    uint64_t total = 0, saturated = 0;
    for (uint32_t i = 0; i < frameCount; i++) {
        const uint8_t *slot = f + ZS_FLT_FIXED + (uint64_t)(firstFrame + i) * bytes;
        if (!zs_flt_passes(slot, h.L, &Q)) continue;
        if (total < capacity) frames[total] = firstFrame + i;
        total++; saturated += zs_flt_all_ones(slot, bytes) ? 1u : 0u;
    }
    result[0] = total; result[1] = total < capacity ? total : capacity; result[2] = frameCount; result[3] = saturated;
    return 0;
}
