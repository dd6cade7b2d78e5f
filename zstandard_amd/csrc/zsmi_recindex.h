// The record index of an archive: the firstRecord array the record calls take (zsmi_records.h), rebuilt from content and frame borders
// alone, and the skippable frame that carries it inside the archive.
//   THE RULE.  Content of `size` bytes, a delimiter byte, frames with content offsets dOff[0 .. N], dOff[N] = size.
//      P(x) = the delimiters in content[0, x), + 1 when x == size, size > 0 and content[size - 1] != delim (the unterminated tail record)
//      firstRecord[i] = P(dOff[i]), i = 0 .. N
//      For every array the splitter makes this is rule 4 of zsmi_split.h: it makes no empty frame, so no frame i < N starts at size and the
//      + 1 reaches firstRecord[N] = records alone.  An EMPTY frame at the content's end - what the index frame below becomes in the seek
//      table - starts at size too and gets firstRecord = records.  count[i] = firstRecord[i + 1] - firstRecord[i] <= the frame's bytes
//      (+ 1 for the tail, which needs a byte behind the frame's last delimiter): it never exceeds Decompressed_Size and fits 32 bits.
//   MISALIGNED.  Frame j is misaligned when it holds at least one delimiter, its last byte is not the delimiter, and it does not end at
//      size.  The lookup of zsmi_records.h relies on "a cut record always starts a frame"; that holds for an archive exactly when no
//      frame is misaligned.  If frame j is misaligned, the record of its last byte starts behind j's last delimiter - inside j, not at its
//      start - and goes on into frame j + 1: a cut record that starts no frame.  The other way, by induction over the frames a record r
//      crosses: let r start at s inside frame j (dOff[j] < s) and end behind j.  s > 0, so content[s - 1] is a delimiter and it lies in j;
//      j's last byte belongs to r and is not r's end, so it is no delimiter; r goes on, so j does not end at size: j is misaligned.  With
//      no misaligned frame every cut record therefore starts its first frame f, each frame behind f that r fills or leaves holds no
//      delimiter in front of r's end - step by step they share firstRecord[f + 1] = firstRecord[f] (+ 0) up to the frame g where r ends -
//      and zs_rec_frames finds f .. g.  The splitter's archives have no misaligned frame; fixed-size frames over text have many.
//   THE FRAME.  A skippable frame between the last content frame and the seek table, listed in the table as a last entry
//      {Compressed_Size = 40 + 4 n, Decompressed_Size = 0 [, 0x51D8E999: the low 32 bits of XXH64 of no bytes]} - every reader sees an
//      archive of n + 1 frames whose last is empty.  Little-endian:
//          0  u32 0x184D2A5D     4  u32 Frame_Size = 32 + 4 n     8  u32 0x58444952 "RIDX"     12  u8 version = 1, u8 delim, u16 0
//         16  u32 n (the content entries 0 .. n - 1 it describes)     20  u32 0     24  u64 records     32  u64 check     40  n x u32 count[i]
//      check = sum over i of (count[i] + 1) * (2 i + 1) * 0x9E3779B185EBCA87, + records * 0xC2B2AE3D27D4EB4F + delim, mod 2^64: a sum, so
//      that a grid computes it in any order; the odd factor 2 i + 1 ties a count to its place, the + 1 makes a zero count weigh.
// Host and device; a host program may include this header alone, with any C++ compiler (tests/c/record_index.cpp does, under the
// sanitizers).  The host forms below are what zsmi_writeRecordIndexFrame, zsmi_readRecordIndexFrame, zsmi_indexRecords and
// zsmi_seekableAttachRecordIndex run; the kernels of recindex.hip share the constants, zs_ridx_term and zs_ridx_misaligned.
#pragma once
#include "../../include/zsmi.h"
#include <string.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define ZS_RIDX_FN __host__ __device__ __forceinline__
#else
#define ZS_RIDX_FN static inline
#endif

#define ZS_RIDX_MAGIC       0x184D2A5Du              // a skippable frame's magic, variant 0xD (the seek table's is 0xE)
#define ZS_RIDX_INNER       0x58444952u              // "RIDX"
#define ZS_RIDX_VERSION     1u
#define ZS_RIDX_FIXED       40u                      // the frame without its counts
#define ZS_RIDX_MAX_FRAMES  0x8000000u               // the seekable format's frame limit: n + 1 entries must stay within it
#define ZS_RIDX_K1          0x9E3779B185EBCA87ull
#define ZS_RIDX_K2          0xC2B2AE3D27D4EB4Full
#define ZS_RIDX_EMPTY_HASH  0x51D8E999u              // the low 32 bits of XXH64 (seed 0) of no bytes: the index entry's checksum
#define ZS_RIDX_SEEK_MAGIC  0x8F92EAB1u              // the seek table's two magics, its fixed bytes and its limit of a Decompressed_Size
#define ZS_RIDX_SEEK_SKIP   0x184D2A5Eu
#define ZS_RIDX_SEEK_FIXED  17u
#define ZS_RIDX_SEEK_MAX_DSIZE (1u << 30)

ZS_RIDX_FN uint64_t zs_ridx_frame_size(uint64_t n) { return ZS_RIDX_FIXED + 4ull * n; }
// frame i's term of the check, and what the header's fields add
ZS_RIDX_FN uint64_t zs_ridx_term(uint32_t count, uint32_t i) { return ((uint64_t)count + 1ull) * (2ull * i + 1ull) * ZS_RIDX_K1; }
ZS_RIDX_FN uint64_t zs_ridx_check_base(uint64_t records, uint32_t delim) { return records * ZS_RIDX_K2 + delim; }
// MISALIGNED, from what a frame's end knows: its delimiters, whether its last byte is one, whether it ends at the content's end
ZS_RIDX_FN bool zs_ridx_misaligned(bool holdsDelim, bool lastIsDelim, bool endsAtSize) { return holdsDelim && !lastIsDelim && !endsAtSize; }

ZS_RIDX_FN uint32_t zs_ridx_rd32(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
ZS_RIDX_FN uint64_t zs_ridx_rd64(const uint8_t *p) { return (uint64_t)zs_ridx_rd32(p) | ((uint64_t)zs_ridx_rd32(p + 4) << 32); }
ZS_RIDX_FN void zs_ridx_wr32(uint8_t *p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24); }
ZS_RIDX_FN void zs_ridx_wr64(uint8_t *p, uint64_t v) { zs_ridx_wr32(p, (uint32_t)v); zs_ridx_wr32(p + 4, (uint32_t)(v >> 32)); }
// the 40 fixed bytes
ZS_RIDX_FN void zs_ridx_write_header(uint8_t *dst, uint32_t n, uint32_t delim, uint64_t records, uint64_t check)
{
    zs_ridx_wr32(dst, ZS_RIDX_MAGIC); zs_ridx_wr32(dst + 4, 32u + 4u * n); zs_ridx_wr32(dst + 8, ZS_RIDX_INNER);
    zs_ridx_wr32(dst + 12, ZS_RIDX_VERSION | (delim << 8)); zs_ridx_wr32(dst + 16, n); zs_ridx_wr32(dst + 20, 0);
    zs_ridx_wr64(dst + 24, records); zs_ridx_wr64(dst + 32, check);
}
// What the fixed bytes say, in zsmi_readRecordIndexFrame's order (size >= ZS_RIDX_FIXED: the caller's check): 0 with n and delim, or the code
ZS_RIDX_FN int zs_ridx_read_header(const uint8_t *src, uint32_t *n, uint32_t *delim)
{
    if (zs_ridx_rd32(src) != ZS_RIDX_MAGIC || zs_ridx_rd32(src + 8) != ZS_RIDX_INNER) return ZSMI_error_prefix_unknown;
    if (src[12] != ZS_RIDX_VERSION) return ZSMI_error_version_unsupported;
    if (src[14] || src[15] || zs_ridx_rd32(src + 20)) return ZSMI_error_corruption_detected;
    const uint32_t k = zs_ridx_rd32(src + 16);
    if (k >= ZS_RIDX_MAX_FRAMES || zs_ridx_rd32(src + 4) != 32u + 4u * k) return ZSMI_error_corruption_detected;
    *n = k; *delim = src[13];
    return 0;
}
// firstRecord[0 .. n] as an index frame's caller hands it over: starts at 0, never descends, no count above 32 bits
ZS_RIDX_FN int zs_ridx_check_array(const uint64_t *firstRecord, uint64_t n)
{
    if (firstRecord[0] != 0) return ZSMI_error_corruption_detected;
    for (uint64_t i = 0; i < n; i++)
        if (firstRecord[i + 1] < firstRecord[i] || firstRecord[i + 1] - firstRecord[i] > 0xFFFFFFFFull) return ZSMI_error_corruption_detected;
    return 0;
}

// ---- the host forms ----
#define ZS_RIDX_ERR(code) ((size_t)0 - (size_t)(code))
// zsmi_recordIndexFrameSize
static inline size_t zs_ridx_size(size_t n) { return n >= ZS_RIDX_MAX_FRAMES ? ZS_RIDX_ERR(ZSMI_error_frameIndex_tooLarge) : (size_t)zs_ridx_frame_size(n); }
// zsmi_writeRecordIndexFrame: the frame's size or (size_t)-code; nothing is written on failure
static inline size_t zs_ridx_write(void *dstv, size_t cap, const uint64_t *firstRecord, size_t n, int delim)
{
    if (delim < 0 || delim > 255) return ZS_RIDX_ERR(ZSMI_error_parameter_outOfBound);
    if (n >= ZS_RIDX_MAX_FRAMES) return ZS_RIDX_ERR(ZSMI_error_frameIndex_tooLarge);
    if (!firstRecord || !dstv) return ZS_RIDX_ERR(ZSMI_error_GENERIC);
    if (const int e = zs_ridx_check_array(firstRecord, n)) return ZS_RIDX_ERR(e);
    const size_t size = (size_t)zs_ridx_frame_size(n);
    if (cap < size) return ZS_RIDX_ERR(ZSMI_error_dstSize_tooSmall);
    uint8_t *dst = (uint8_t *)dstv;
    uint64_t check = zs_ridx_check_base(firstRecord[n], (uint32_t)delim);
    for (size_t i = 0; i < n; i++) {
        const uint32_t count = (uint32_t)(firstRecord[i + 1] - firstRecord[i]);
        zs_ridx_wr32(dst + ZS_RIDX_FIXED + 4 * i, count);
        check += zs_ridx_term(count, (uint32_t)i);
    }
    zs_ridx_write_header(dst, (uint32_t)n, (uint32_t)delim, firstRecord[n], check);
    return size;
}
// zsmi_readRecordIndexFrame: n, with firstRecord[0 .. n] (firstRecord[n] = records; NULL: the frame is only judged) and *delim (may be
// NULL), or (size_t)-code.  Fewer than 40 bytes, or fewer than the header's n asks for: srcSize_wrong; capacity < n + 1 entries:
// dstSize_tooSmall.  The array is written only behind the last check.
static inline size_t zs_ridx_read(const void *srcv, size_t size, uint64_t *firstRecord, size_t capacity, int *delim)
{
    const uint8_t *src = (const uint8_t *)srcv;
    if (!src || size < ZS_RIDX_FIXED) return ZS_RIDX_ERR(ZSMI_error_srcSize_wrong);
    uint32_t n, d;
    if (const int e = zs_ridx_read_header(src, &n, &d)) return ZS_RIDX_ERR(e);
    if (size < zs_ridx_frame_size(n)) return ZS_RIDX_ERR(ZSMI_error_srcSize_wrong);
    if (firstRecord && capacity < (size_t)n + 1) return ZS_RIDX_ERR(ZSMI_error_dstSize_tooSmall);
    const uint64_t records = zs_ridx_rd64(src + 24);
    uint64_t check = zs_ridx_check_base(records, d), sum = 0;
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t count = zs_ridx_rd32(src + ZS_RIDX_FIXED + 4 * (size_t)i);
        sum += count; check += zs_ridx_term(count, i);
    }
    if (check != zs_ridx_rd64(src + 32) || sum != records) return ZS_RIDX_ERR(ZSMI_error_corruption_detected);
    if (firstRecord) {
        uint64_t at = 0;
        for (uint32_t i = 0; i < n; i++) { firstRecord[i] = at; at += zs_ridx_rd32(src + ZS_RIDX_FIXED + 4 * (size_t)i); }
        firstRecord[n] = at;
    }
    if (delim) *delim = (int)d;
    return n;
}
// zsmi_indexRecords: THE RULE over plain text, serially; frame i holds frameSizes[i] bytes.  0 or a code: delim outside 0 .. 255:
// parameter_outOfBound; a NULL frameSizes with n > 0, or a NULL firstRecord: GENERIC; a NULL src with bytes, or sizes that do not sum to
// srcSize: srcSize_wrong.  firstRecord[0 .. n]; result (may be NULL) = {0, records, misaligned frames, delimiters}
static inline int zs_ridx_index(const void *srcv, uint64_t srcSize, const uint32_t *frameSizes, uint64_t n, int delim, uint64_t *firstRecord, uint64_t *result)
{
    if (delim < 0 || delim > 255) return ZSMI_error_parameter_outOfBound;
    if ((n && !frameSizes) || !firstRecord) return ZSMI_error_GENERIC;
    if (srcSize && !srcv) return ZSMI_error_srcSize_wrong;
    uint64_t sum = 0;
    for (uint64_t i = 0; i < n; i++) sum += frameSizes[i];
    if (sum != srcSize) return ZSMI_error_srcSize_wrong;
    const uint8_t *src = (const uint8_t *)srcv;
    const uint64_t tail = srcSize && src[srcSize - 1] != (uint8_t)delim ? 1u : 0u;
    uint64_t delims = 0, misaligned = 0, pos = 0;
    for (uint64_t i = 0; i < n; i++) {
        firstRecord[i] = delims + (pos == srcSize ? tail : 0u);
        const uint64_t end = pos + frameSizes[i], before = delims;
        for (uint64_t q = pos; q < end; q++) delims += src[q] == (uint8_t)delim;
        if (end > pos && zs_ridx_misaligned(delims > before, src[end - 1] == (uint8_t)delim, end == srcSize)) misaligned++;
        pos = end;
    }
    firstRecord[n] = delims + tail;
    if (result) { result[0] = 0; result[1] = delims + tail; result[2] = misaligned; result[3] = delims; }
    return 0;
}
// The seek table at an archive's end, as far as attaching needs it: the frame count, the entry size, where the table starts.  The
// rejections are the table's own, in the order the readers of the archive calls apply them.
struct ZsRidxTable { uint32_t n, entry; uint64_t at, tableSize; };
static inline int zs_ridx_parse_table(const uint8_t *src, uint64_t size, ZsRidxTable &t)
{
    if (!src || size < 9) return ZSMI_error_prefix_unknown;
    const uint8_t *footer = src + size - 9;
    if (zs_ridx_rd32(footer + 5) != ZS_RIDX_SEEK_MAGIC) return ZSMI_error_prefix_unknown;
    if (footer[4] & 0x7C) return ZSMI_error_corruption_detected;
    t.n = zs_ridx_rd32(footer);
    if (t.n > ZS_RIDX_MAX_FRAMES) return ZSMI_error_frameIndex_tooLarge;
    t.entry = footer[4] & 0x80 ? 12u : 8u;
    t.tableSize = ZS_RIDX_SEEK_FIXED + (uint64_t)t.n * t.entry;
    if (t.tableSize > size) return ZSMI_error_corruption_detected;
    t.at = size - t.tableSize;
    const uint8_t *tbl = src + t.at;
    if (zs_ridx_rd32(tbl) != ZS_RIDX_SEEK_SKIP) return ZSMI_error_prefix_unknown;
    if (zs_ridx_rd32(tbl + 4) != t.n * t.entry + 9u) return ZSMI_error_corruption_detected;
    uint64_t frames = 0;
    for (uint32_t i = 0; i < t.n; i++) {
        const uint32_t cSize = zs_ridx_rd32(tbl + 8 + (size_t)i * t.entry), dSize = zs_ridx_rd32(tbl + 12 + (size_t)i * t.entry);
        if (cSize == 0 || dSize > ZS_RIDX_SEEK_MAX_DSIZE) return ZSMI_error_corruption_detected;
        frames += cSize;
    }
    return frames == t.at ? 0 : ZSMI_error_corruption_detected;
}
// whether the table's last entry is an index frame: no content, and the bytes it names open with the two magics
static inline bool zs_ridx_last_is_index(const uint8_t *src, const ZsRidxTable &t)
{
    if (t.n == 0) return false;
    const uint8_t *e = src + t.at + 8 + (size_t)(t.n - 1) * t.entry;
    const uint32_t cSize = zs_ridx_rd32(e);
    if (zs_ridx_rd32(e + 4) != 0 || cSize < ZS_RIDX_FIXED) return false;
    const uint8_t *f = src + t.at - cSize;
    return zs_ridx_rd32(f) == ZS_RIDX_MAGIC && zs_ridx_rd32(f + 8) == ZS_RIDX_INNER;
}
// zsmi_seekableAttachRecordIndex: a host archive in place - the table moves back by 40 + 4 n bytes, the index frame takes its place, its
// entry is added behind the others and the footer counts n + 1.  The new size or (size_t)-code; a refused archive is untouched.  In
// order: the table's own rejections; delim outside 0 .. 255 or n not the table's frame count: parameter_outOfBound; a NULL firstRecord:
// GENERIC; firstRecord[0] != 0, a descent, or a count above its entry's Decompressed_Size: corruption_detected; an archive whose last entry
// is an index frame already: parameter_unsupported; n + 1 > 0x8000000: frameIndex_tooLarge; capacity below the new size: dstSize_tooSmall
static inline size_t zs_ridx_attach(void *archivev, size_t archiveSize, size_t capacity, const uint64_t *firstRecord, size_t n, int delim)
{
    uint8_t *a = (uint8_t *)archivev;
    ZsRidxTable t;
    if (const int e = zs_ridx_parse_table(a, archiveSize, t)) return ZS_RIDX_ERR(e);
    if (delim < 0 || delim > 255 || n != t.n) return ZS_RIDX_ERR(ZSMI_error_parameter_outOfBound);
    if (!firstRecord) return ZS_RIDX_ERR(ZSMI_error_GENERIC);
    if (firstRecord[0] != 0) return ZS_RIDX_ERR(ZSMI_error_corruption_detected);
    for (size_t i = 0; i < n; i++)
        if (firstRecord[i + 1] < firstRecord[i] || firstRecord[i + 1] - firstRecord[i] > zs_ridx_rd32(a + t.at + 12 + i * t.entry)) return ZS_RIDX_ERR(ZSMI_error_corruption_detected);
    if (zs_ridx_last_is_index(a, t)) return ZS_RIDX_ERR(ZSMI_error_parameter_unsupported);
    if (n + 1 > ZS_RIDX_MAX_FRAMES) return ZS_RIDX_ERR(ZSMI_error_frameIndex_tooLarge);
    const size_t frame = (size_t)zs_ridx_frame_size(n), grown = archiveSize + frame + t.entry;
    if (capacity < grown) return ZS_RIDX_ERR(ZSMI_error_dstSize_tooSmall);
    const uint8_t desc = a[archiveSize - 5];
    uint8_t *tbl = a + t.at + frame;                                        // the table's new place
    memmove(tbl, a + t.at, 8 + n * t.entry);                                // its header and entries (the places overlap)
    zs_ridx_wr32(tbl + 4, (uint32_t)(n + 1) * t.entry + 9u);
    uint8_t *e = tbl + 8 + n * t.entry;
    zs_ridx_wr32(e, (uint32_t)frame); zs_ridx_wr32(e + 4, 0);
    if (t.entry == 12) zs_ridx_wr32(e + 8, ZS_RIDX_EMPTY_HASH);
    e += t.entry;
    zs_ridx_wr32(e, (uint32_t)(n + 1)); e[4] = desc; zs_ridx_wr32(e + 5, ZS_RIDX_SEEK_MAGIC);
    (void)zs_ridx_write(a + t.at, frame, firstRecord, n, delim);            // (every refusal of its own was checked above)
    return grown;
}
