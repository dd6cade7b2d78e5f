// The record splitter's rule: where the frames of a record archive end in a buffer of delimited records (lines, JSON lines, CSV rows).
//   1. RECORDS.  A record ends behind each byte equal to `delim`; bytes behind the last delimiter are a last record without one.
//      records = the delimiters, + 1 for such a tail.
//   2. PIECES.  A record of L <= M bytes (M = maxFrameSize) is one piece; a longer one is cut at multiples of M counted from ITS OWN start:
//      ceil(L / M) pieces, all of M bytes but the last.  Piece ends do not depend on where frames fall.  pieces <= records + srcSize / M.
//   3. FRAMES.  From pos = 0, while pos < srcSize: with T = targetSize == 0 the frame ends at the first piece end behind pos; with T > 0 at
//      the last piece end in (pos, pos + T], or, if there is none, at the first piece end behind pos - greedy: as many whole pieces as fit
//      in T, a piece longer than T alone.  T <= M, so no frame is above M; the sizes sum to srcSize.
//   4. firstRecord[i] = the delimiters in src[0, start_i); firstRecord[n] = records.  THE LOOKUP: the frame record r STARTS in is the first
//      i with firstRecord[i] >= r when that entry equals r, else i - 1 (r starts inside frame i - 1, behind other records).  A cut record
//      always starts a frame, so the first alternative finds it; its later pieces are the frames that follow, up to the next start.
// The definition is serial, and zsmi_splitRecords runs it as written here (zs_split_walk_host).  The kernels of split.hip reach the same
// frames in parallel - record ends by a bit-mask scan, pieces by a scan over the records' extra cuts, frames by pointer doubling over the
// piece ends - and share zs_split_extra_cuts and the argument checks.  Host and device; a host program may include this header alone, with
// any C++ compiler (tests/c/split_records.cpp does, under the sanitizers).
#pragma once
#include "../../include/zsmi.h"
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define ZS_SPLIT_FN __host__ __device__ __forceinline__
#else
#define ZS_SPLIT_FN static inline
#endif

#define ZS_SPLIT_MAX_FRAME_SIZE (1ull << 30)      // the seekable format's limit of a Decompressed_Size (ZS_SEEK_MAX_FRAME_SIZE)
#define ZS_SPLIT_MAX_PIECES     0x80000000ull     // the most a device call is planned for

// what every form of the call checks of these arguments, in the header's order (the device forms check a NULL ctx in front)
ZS_SPLIT_FN int zs_split_check(const void *src, uint64_t srcSize, int delim, uint32_t targetSize, uint32_t maxFrameSize, uint64_t maxPieces)
{
    if (delim < 0 || delim > 255) return ZSMI_error_parameter_outOfBound;
    if (maxFrameSize == 0 || maxFrameSize > ZS_SPLIT_MAX_FRAME_SIZE) return ZSMI_error_parameter_outOfBound;
    if (targetSize > maxFrameSize) return ZSMI_error_parameter_outOfBound;
    if (maxPieces > ZS_SPLIT_MAX_PIECES) return ZSMI_error_parameter_outOfBound;
    if (srcSize && !src) return ZSMI_error_srcSize_wrong;
    return 0;
}
// rule 2: the cuts inside a record of L >= 1 bytes, its pieces less one
ZS_SPLIT_FN uint64_t zs_split_extra_cuts(uint64_t L, uint32_t M) { return (L - 1) / M; }

// the first piece end behind pos, pos < size, in the record that starts at recStart <= pos: the record's end, or its next cut if that
// comes first.  Reads only src[pos, min(cut, size))
ZS_SPLIT_FN uint64_t zs_split_piece_end(const uint8_t *src, uint64_t size, uint8_t delim, uint32_t M, uint64_t pos, uint64_t recStart)
{
    const uint64_t cut = recStart + ((pos - recStart) / M + 1) * M;
    const uint64_t lim = cut < size ? cut : size;
    for (uint64_t q = pos; q < lim; q++) if (src[q] == delim) return q + 1;
    return lim;
}

// ---- the host form: the loop itself (arguments checked by the caller).  each(index, size, firstRecord) sees every frame in order;
// n: the frames, records: rule 1's count ----
template <class Each>
static inline void zs_split_walk_host(const uint8_t *src, uint64_t size, uint8_t delim, uint32_t T, uint32_t M, uint64_t &n, uint64_t &records, Each each)
{
    n = 0;
    uint64_t delims = 0, recStart = 0;                        // the delimiters in front of pos; the start of the record pos lies in
    for (uint64_t pos = 0; pos < size;) {
        const uint64_t first = delims;
        uint64_t end = pos;
        for (;;) {
            const uint64_t e = zs_split_piece_end(src, size, delim, M, end, recStart);
            if (end != pos && e - pos > T) break;             // (the first piece is taken whatever its length; T == 0 takes no second)
            end = e;
            if (src[end - 1] == delim) { delims++; recStart = end; }      // a piece that ends its record (a tail's end is the stream's)
            if (end == size || end - pos >= T) break;
        }
        each(n, (uint32_t)(end - pos), first);
        n++; pos = end;
    }
    records = delims + (size && src[size - 1] != delim ? 1u : 0u);
}
// zsmi_splitRecords: the frame count or (size_t)-code.  frameSizes == NULL only counts; more frames than capacity: dstSize_tooSmall, with
// nothing written behind capacity (firstRecord, which may be NULL, holds capacity + 1 entries); records may be NULL
static inline size_t zs_split_records(const void *srcv, size_t srcSize, int delim, uint32_t targetSize, uint32_t maxFrameSize,
                                      uint32_t *frameSizes, uint64_t *firstRecord, size_t capacity, uint64_t *records)
{
    if (const int e = zs_split_check(srcv, srcSize, delim, targetSize, maxFrameSize, 0)) return (size_t)0 - (size_t)e;
    uint64_t n, recs;
    zs_split_walk_host((const uint8_t *)srcv, srcSize, (uint8_t)delim, targetSize, maxFrameSize, n, recs,
                       [=](uint64_t i, uint32_t size, uint64_t first) {
                           if (!frameSizes || i >= capacity) return;
                           frameSizes[i] = size;
                           if (firstRecord) firstRecord[i] = first;
                       });
    if (records) *records = recs;
    if (!frameSizes) return (size_t)n;
    if (n > capacity) return (size_t)0 - (size_t)ZSMI_error_dstSize_tooSmall;
    if (firstRecord) firstRecord[n] = recs;
    return (size_t)n;
}
