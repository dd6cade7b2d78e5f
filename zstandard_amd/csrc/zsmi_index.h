// The frame index of a stream of frames that carries no seek table: one entry {compressed size, content size} a frame, zstd and skippable,
// in stream order - what a seek table would state, read from the frames' own headers by the container walker (zs_walk, zsmi_frame.h).
//   The definition is serial: the frame at 0, then the frame where that one ends, and so on to the stream's end.  The host calls
// (zsmi_countFrames, zsmi_buildSeekTable, zsmi_openFrames) run it as written here; the kernels of seekable.hip (k_index_*) reach the same
// entries in parallel and judge a frame with the same zs_index_frame.  Host and device; a host program may include this header alone
// (tests/c/frames_index.cpp does, under the sanitizers).
#pragma once
#include "zsmi_frame.h"
#include <cstring>

#define ZS_SEEK_MAX_FRAMES     0x8000000ull      // the seekable format's limits: the frames of a table,
#define ZS_SEEK_MAX_FRAME_SIZE (1ull << 30)      // a Decompressed_Size
#define ZS_SEEK_TABLE_FIXED    17u               // skippable header (8) + footer (9)

// a place a frame may start at: either magic number (a skippable frame's low nibble is free)
__host__ __device__ __forceinline__ bool zs_index_magic(uint32_t w) { return w == 0xFD2FB528u || (w & 0xFFFFFFF0u) == 0x184D2A50u; }

// The frame at p[0 .. avail): zsmi_findFrameCompressedSize's answer and code first; then the table's field limits, each
// frameParameter_unsupported - no stated content size, one above 1 GiB, a compressed size above 32 bits.  Reads only p[0 .. avail).
// (ZS_WALK_FIRST_FRAME walks one frame, so the walker's content sum is that frame's Frame_Content_Size - zsmi_getFrameContentSize's
// answer - and 0 for a skippable frame; both "unknown" and "error" lie above the limit.)
struct ZsIndexFrame { uint32_t status, dSize; uint64_t cSize; };
__host__ __device__ __forceinline__ ZsIndexFrame zs_index_frame(const uint8_t *p, uint64_t avail)
{
    ZsIndexFrame f = {};
    const ZsWalk w = zs_walk<uint64_t>(p, avail, ZS_WALK_FIRST_FRAME);
    if (w.status) { f.status = w.status; return f; }
    if (!w.nFrames) { f.status = ZSMI_error_srcSize_wrong; return f; }               // (fewer than 5 bytes: no frame)
    if (w.contentSize > ZS_SEEK_MAX_FRAME_SIZE || w.consumed > 0xFFFFFFFFull) { f.status = ZSMI_error_frameParameter_unsupported; return f; }
    f.cSize = w.consumed; f.dSize = (uint32_t)w.contentSize;
    return f;
}

// ---- the host form: the loop itself.  each(index, cSize, dSize) sees every frame in order; n: the frames in front of the stream's end or
// of the first refusal, whose code is the result (0: none).  A frame past the table's count limit: frameIndex_tooLarge.  Bytes said to be
// there behind a null pointer: srcSize_wrong (no byte can be read where the caller states some) ----
template <class Each>
static inline int zs_index_walk_host(const uint8_t *src, uint64_t size, uint64_t &n, Each each)
{
    n = 0;
    if (size && !src) return ZSMI_error_srcSize_wrong;
    for (uint64_t pos = 0; pos < size;) {
        const ZsIndexFrame f = zs_index_frame(src + pos, size - pos);
        if (f.status) return (int)f.status;
        if (n == ZS_SEEK_MAX_FRAMES) return ZSMI_error_frameIndex_tooLarge;
        each(n, (uint32_t)f.cSize, f.dSize);
        n++; pos += f.cSize;
    }
    return 0;
}
static inline void zs_index_st32(uint8_t *p, uint32_t v) { memcpy(p, &v, 4); }             // (the host is little-endian: zsmi_device.h)
// zsmi_countFrames and zsmi_buildSeekTable: a size_t that is the answer or (size_t)-code.  The table is the seekable format's without
// checksums - 0x184D2A5E | 8 n + 9 | n x {Compressed_Size, Decompressed_Size} | n | descriptor 0 | 0x8F92EAB1 - written in a second walk
// once the first has counted the frames and found them whole: nothing is allocated, nothing written for a stream that is refused
static inline size_t zs_index_count(const void *src, size_t size)
{
    uint64_t n;
    const int e = zs_index_walk_host((const uint8_t *)src, size, n, [](uint64_t, uint32_t, uint32_t) {});
    return e ? (size_t)0 - (size_t)e : (size_t)n;
}
static inline size_t zs_index_build_table(void *dst, size_t dstCapacity, const void *src, size_t size)
{
    const size_t n = zs_index_count(src, size);
    if (n > (size_t)ZS_SEEK_MAX_FRAMES) return n;                                            // (an error code)
    const size_t bytes = ZS_SEEK_TABLE_FIXED + 8 * n;
    if (dstCapacity < bytes || !dst) return (size_t)0 - (size_t)ZSMI_error_dstSize_tooSmall;
    uint8_t *t = (uint8_t *)dst; uint64_t again;
    zs_index_st32(t, 0x184D2A5Eu); zs_index_st32(t + 4, (uint32_t)(8 * n + 9));
    (void)zs_index_walk_host((const uint8_t *)src, size, again, [t](uint64_t i, uint32_t c, uint32_t d) { zs_index_st32(t + 8 + 8 * i, c); zs_index_st32(t + 12 + 8 * i, d); });
    uint8_t *f = t + 8 + 8 * n;
    zs_index_st32(f, (uint32_t)n); f[4] = 0; zs_index_st32(f + 5, 0x8F92EAB1u);
    return bytes;
}
