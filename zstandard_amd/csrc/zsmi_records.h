// Records by number: which frames of a record archive hold record r, and which bytes of them are the record.  The two rules
// zsmi_seekableReadRecordsResident / Host apply, stated once - the lookup kernel and the host call run zs_rec_frames as it stands here, the
// measure kernel reaches zs_rec_extent's answer a wavefront a request (records.hip), and tests/c/read_records.cpp runs both serially.
//   FRAMES.  firstRecord[0 .. n] is what the splitter left (zsmi_split.h, rule 4): the delimiters in front of each frame's start, and
//      firstRecord[n] = records.  For r < firstRecord[n]: g = the last frame with firstRecord[g] <= r; lb = the first frame with
//      firstRecord[lb] >= r; f = lb when firstRecord[lb] == r, else g.  Frames f .. g hold the record: f < g only for a record that was cut
//      (its frames in front of g hold no delimiter, so they share their firstRecord), f == g for every other.  skip = r - firstRecord[f]:
//      the delimiters in front of the record inside frame f - 0 when the record starts the frame, and always 0 when f < g.
//   EXTENT.  In the content of frames f .. g as one run of bytes: start = the position behind the skip-th delimiter (0 for skip 0), end =
//      the position behind the first delimiter at or behind start, or the run's end when there is none (the stream's tail record).  Fewer
//      than skip delimiters (skip > 0: the run is frame f alone): corruption_detected - the array or the delimiter is not this archive's.
// Whatever firstRecord holds - not ascending, another archive's - zs_rec_frames reads only firstRecord[0, n) and answers f <= g < n.
// Host and device; a host program may include this header alone, with any C++ compiler.
#pragma once
#include "../../include/zsmi.h"
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define ZS_REC_FN __host__ __device__ __forceinline__
#else
#define ZS_REC_FN static inline
#endif

#define ZS_REC_MAX_FRAME_READS 0x8000000u        // the most frame reads a call is planned for: the seekable format's frame limit

struct ZsRecFrames { uint32_t f, g; uint64_t skip; };
// n >= 1 frames.  (r >= firstRecord[n] names no record: the caller's check)
ZS_REC_FN ZsRecFrames zs_rec_frames(const uint64_t *firstRecord, uint32_t n, uint64_t r)
{
    uint32_t lo = 0, hi = n;                                   // the first frame with firstRecord > r
    while (lo < hi) { const uint32_t mid = lo + (hi - lo) / 2; if (firstRecord[mid] <= r) lo = mid + 1; else hi = mid; }
    ZsRecFrames a;
    a.g = lo ? lo - 1 : 0;                                     // (none at or below r: an array that is not the splitter's)
    lo = 0; hi = n;                                            // lb (n: none below firstRecord[n])
    while (lo < hi) { const uint32_t mid = lo + (hi - lo) / 2; if (firstRecord[mid] < r) lo = mid + 1; else hi = mid; }
    a.f = lo < n && lo <= a.g && firstRecord[lo] == r ? lo : a.g;
    a.skip = r - firstRecord[a.f];
    return a;
}
// the serial statement of EXTENT over run[0, len): 0 with [*start, *end), or corruption_detected
ZS_REC_FN int zs_rec_extent(const uint8_t *run, uint64_t len, uint8_t delim, uint64_t skip, uint64_t *start, uint64_t *end)
{
    uint64_t pos = 0;
    for (uint64_t seen = 0; seen < skip; pos++) {
        if (pos >= len) return ZSMI_error_corruption_detected;
        if (run[pos] == delim) seen++;
    }
    *start = pos;
    while (pos < len && run[pos] != delim) pos++;
    *end = pos < len ? pos + 1 : len;
    return 0;
}
