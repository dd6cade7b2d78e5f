// findframes.hip -- the query search over a LIST of frames that lives in device memory (zsmi_seekableFindQueryFramesResident; the host
// form stages host arrays): what zsmi_filterFramesDevice leaves - ascending frame numbers and their count, a device word - goes straight
// into a search that decodes those frames and no others.  The host is told only maxFrames.  The device calls only queue work.
//   THE RULE.  A RUN is a maximal stretch of the list whose frames follow one another in the archive.  The text searched is the runs'
//   content; an occurrence lies inside one run; its record is firstRecord[f] + the delimiters in front of it inside the frame f it starts
//   in; the answer is the satisfying records, ascending, each once a run.  A list the filter call wrote never separates a record's frames
//   by a frame that holds bytes (zsmi_filter.h, rule 11), so there each record appears once and the answer is the window search's.
// The launch sequence, F = maxFrames list entries whatever the count is (entries at or behind the count name no frame and decode nothing):
//   k_findsel_list     the list judged - a count above maxFrames, a frame number at or above nFrames, a list that does not ascend - and
//                      laid out: an entry's bytes are its frame's Decompressed_Size, + 1 for the last frame of a run that another run
//                      follows: ONE delimiter byte between runs.  A pattern holds no delimiter, so nothing straddles a run border
//   scanOffsets        the frames' places in dWork; k_seek_request_items, decodeItems, k_seek_verify: seekable.hip's frame-list decode on the list
//   k_findsel_code     the call's code: the list's refusal, content above workCapacity, or the first failing frame's code
//   k_findsel_fill     the delimiter between runs, and delimiters from the content's end to the end of the text searched: the text is
//                      S = min(workCapacity, zsmi_seekableFindFramesWorkBound(sk, maxFrames)) bytes, a size the HOST knows; the records
//                      the fill adds are empty, and an `any` or `all` query lists no empty record
//   findqText          the existing query launch sequence over dWork[0, S) with base 0 and the call's code: ordinals of the text
//   k_findsel_prefix   a wavefront a listed frame: the delimiters in front of its place - the tile's base from the search's own scan, +
//                      those between the tile's start and the place
//   k_findsel_renumber every number written: the last listed frame whose prefix is <= the ordinal; + that frame's firstRecord - its
//                      prefix.  An empty frame starts no record and is stepped over (at the content's end its firstRecord counts the
//                      tail record already); a content tail without a delimiter is ended by the fill.  One lane writes dResult = {total, written, occurrences, content bytes decoded},
//                      or {(uint64_t)-code, 0, 0, bytes needed}
// Scratch, all of it context buffers reserved before anything is queued: the frame-list decode's words for F frames, find.hip's for S bytes, 8 bytes a listed frame
// and 64 bytes of words.  Every store is a vector store from plain C++.
// NOT COVERED: `none` mode (parameter_unsupported: the fill's empty records would be listed), the single-pattern and regular-expression
// forms of the list search (the decode half is shared: they are small).

#include "zsmi_status.h"
#include "zsmi_wave.h"            // wave_sum
#include "zsmi_ctx.h"             // the context, LAUNCH, scanOffsets, decodeItems
#include "zsmi_findquery.h"       // the query and its checks
#include <algorithm>
// From the feature files zsmi_api.hip includes in front of this one: split.hip - ZS_SPLIT_TILE; seekable.hip - the handle, ZsSeekEntry, the
// frame-list decode (SeekListWords, seekListHead, seekListWords, seekDecodeList); find.hip - FindTiles, findReserve, FindStaged, findStage;
// findquery.hip - findQuery, findqText, findQueryShortest; recindex.hip - zs_ridx_wave_sum64.

struct ZsFselWords { unsigned long long needed, seps; uint32_t bad, tooMany, code, count; uint64_t tmp[4]; };      // zeroed on the stream in front of the kernels

// list[j], sizes[j] for j < F; words: needed - the bytes the list takes in dWork, seps - the delimiters between runs among them, bad,
// tooMany, count - the entries planned.  frames is read below min(*dCount, maxFrames) only
__global__ void __launch_bounds__(256)
k_findsel_list(const ZsSeekEntry *__restrict__ table, uint32_t nTable, const uint32_t *__restrict__ frames, const uint64_t *__restrict__ dCount, uint32_t maxFrames, uint32_t F,
               uint32_t *__restrict__ list, uint64_t *__restrict__ sizes, ZsFselWords *words)
{
    const uint64_t stated = *dCount;
    const bool tooMany = stated > maxFrames;
    const uint32_t count = tooMany ? 0u : (uint32_t)stated;
    unsigned long long needed = 0, seps = 0;
    bool bad = false;
    for (uint32_t j = blockIdx.x * 256u + threadIdx.x; j < F; j += gridDim.x * 256u) {
        uint32_t f = ~0u; uint64_t size = 0;
        if (j < count) {
            f = frames[j];
            if (f >= nTable || (j && frames[j - 1u] >= f)) { bad = true; f = ~0u; }
            else {
                const uint32_t sep = j + 1u < count && frames[j + 1u] != f + 1u ? 1u : 0u;
                size = (uint64_t)table[f].dSize + sep; seps += sep;
            }
        }
        list[j] = f; sizes[j] = size; needed += size;
    }
    needed = zs_ridx_wave_sum64(needed); seps = zs_ridx_wave_sum64(seps);
    if ((threadIdx.x & 63u) == 0) { if (needed) atomicAdd(&words->needed, needed); if (seps) atomicAdd(&words->seps, seps); }
    if (bad) words->bad = 1u;
    if (blockIdx.x == 0 && threadIdx.x == 0) { words->tooMany = tooMany ? 1u : 0u; words->count = count; }
}
// the call's code, one workgroup: a count above maxFrames, then a list that is refused, then content above the work buffer, then the first
// failing frame's code in list order.  A refusal leaves the bytes needed in words->needed (a count above maxFrames: the work bound of that
// many frames)
__global__ void __launch_bounds__(256)
k_findsel_code(const uint32_t *__restrict__ codes, const uint64_t *__restrict__ dCount, uint32_t maxDSize, uint64_t workCapacity, ZsFselWords *words)
{
    __shared__ uint32_t firsts[4];
    const uint32_t count = words->count;
    uint32_t first = ~0u;
    for (uint32_t j = threadIdx.x; j < count && first == ~0u; j += 256u) if (codes[j]) first = j;
    first = wave_min(first);
    if ((threadIdx.x & 63u) == 0) firsts[threadIdx.x >> 6] = first;
    __syncthreads();
    if (threadIdx.x) return;
    for (uint32_t w = 1; w < 4; w++) first = min(first, firsts[w]);
    uint32_t code = 0;
    if (words->tooMany) { code = ZSMI_error_dstSize_tooSmall; words->needed = *dCount <= 0xFFFFFFFFull ? *dCount * ((uint64_t)maxDSize + 1u) : ~0ull; }
    else if (words->bad) code = ZSMI_error_frameIndex_tooLarge;
    else if (words->needed > workCapacity) code = ZSMI_error_dstSize_tooSmall;
    else if (first != ~0u) code = codes[first];
    words->code = code;
}
// the delimiter behind a run that another run follows (an entry longer than its frame ends with it), and delimiters over [content's end, S)
__global__ void __launch_bounds__(256)
k_findsel_fill(uint8_t *work, uint64_t S, uint32_t delim, const ZsSeekEntry *__restrict__ table, const uint32_t *__restrict__ list, const uint64_t *__restrict__ sizes,
               const uint64_t *__restrict__ listAt, uint32_t F)
{
    const uint64_t stride = (uint64_t)gridDim.x * 256u, gid = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    for (uint64_t j = gid; j < F; j += stride) {
        const uint32_t f = list[j];
        if (f == ~0u || sizes[j] == table[f].dSize) continue;
        const uint64_t at = listAt[j + 1u] - 1u;
        if (at < S) work[at] = (uint8_t)delim;
    }
    for (uint64_t at = listAt[F] + gid; at < S; at += stride) work[at] = (uint8_t)delim;
}
// prefix[j], j < the count: the delimiters of work[0, listAt[j]) - recBase[t], the search's scan, for the tile t of the place, + those of the tile
// in front of the place.  A wavefront a listed frame
__global__ void __launch_bounds__(64)
k_findsel_prefix(const uint8_t *__restrict__ work, uint64_t S, uint32_t delim, const uint64_t *__restrict__ listAt, const uint64_t *__restrict__ recBase,
                 const ZsFselWords *__restrict__ words, uint64_t *__restrict__ prefix)
{
    if (blockIdx.x >= words->count) return;                                // (an entry behind the count: never looked up)
    const uint64_t x = listAt[blockIdx.x] < S ? listAt[blockIdx.x] : S, t = x / ZS_SPLIT_TILE;
    uint32_t n = 0;
    for (uint64_t at = t * ZS_SPLIT_TILE + threadIdx.x; at < x; at += 64u) n += work[at] == (uint8_t)delim ? 1u : 0u;
    n = wave_sum(n);
    if (threadIdx.x == 0) prefix[blockIdx.x] = recBase[t] + n;
}
// tmp: the four words the search left.  records[k], k < written: an ordinal of the text -> a record of the archive.  One lane: result
__global__ void __launch_bounds__(256)
k_findsel_renumber(uint64_t *__restrict__ records, const ZsFselWords *__restrict__ words, const uint64_t *__restrict__ prefix, const uint32_t *__restrict__ list,
                   const ZsSeekEntry *__restrict__ table, const uint64_t *__restrict__ firstRecord, uint64_t *__restrict__ result)
{
    const uint32_t code = words->code, count = words->count;
    const uint64_t written = code ? 0ull : words->tmp[1];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        result[0] = code ? 0ull - (uint64_t)code : words->tmp[0];
        result[1] = written; result[2] = code ? 0ull : words->tmp[2];
        result[3] = code ? words->needed : words->needed - words->seps;
    }
    for (uint64_t k = (uint64_t)blockIdx.x * 256u + threadIdx.x; k < written; k += (uint64_t)gridDim.x * 256u) {
        const uint64_t r = records[k];
        uint32_t lo = 0, hi = count;                                       // the first j with prefix[j] > r; the frame is the one in front (prefix[0] = 0 <= r)
        while (lo < hi) { const uint32_t mid = lo + (hi - lo) / 2u; if (prefix[mid] <= r) lo = mid + 1u; else hi = mid; }
        uint32_t j = lo ? lo - 1u : 0u;
        while (j && table[list[j]].dSize == 0u) j--;                       // no record starts in an empty frame: at the content's end its firstRecord counts the tail record already
        records[k] = r - prefix[j] + firstRecord[list[j]];
    }
}

// ---- host ----
extern "C" size_t zsmi_seekableFindFramesWorkBound(const zsmi_seekable *sk, uint32_t maxFrames)
{
    return sk ? (size_t)maxFrames * ((size_t)sk->maxDSize + 1) : 0;
}
// the checks of both forms, in the query calls' order; work: null for the host form, which brings its own buffer
static int findselCheck(const zsmi_ctx *c, const zsmi_seekable *sk, const void *firstRecord, uint32_t nFrames, int delim, const zsmi_findQuery *q, const void *frames,
                        const void *frameCount, uint32_t maxFrames, bool ownWork, const void *work, uint64_t workCapacity, const void *records, uint64_t capacity, const void *result)
{
    if (!c) return ZSMI_error_init_missing;
    if (!sk || !result || !q || !firstRecord || !frameCount || (maxFrames && !frames) || (capacity && !records)) return ZSMI_error_GENERIC;
    if (sk->device != c->device) return ZSMI_error_parameter_unsupported;
    if (const int e = zs_findq_check(delim, q)) return e;
    if (q->mode == ZSMI_find_none) return ZSMI_error_parameter_unsupported;
    if (nFrames != sk->t.n) return ZSMI_error_parameter_outOfBound;
    if (!ownWork && workCapacity && !work) return ZSMI_error_GENERIC;
    return 0;
}
// the launch sequence, its arguments checked by the caller (context bound)
static int findselRun(zsmi_ctx *c, const zsmi_seekable *sk, const uint64_t *dFirstRecord, int delim, const zsmi_findQuery *q, const uint32_t *dFrames, const uint64_t *dFrameCount,
                      uint32_t maxFrames, void *dWork, uint64_t workCapacity, uint64_t *dRecords, uint8_t *dHits, uint64_t capacity, uint64_t *dResult)
{
    const uint32_t F = std::max(maxFrames, 1u);
    const uint64_t S = std::min<uint64_t>(workCapacity, zsmi_seekableFindFramesWorkBound(sk, maxFrames));
    // scratch: the frame-list decode's words of F frames, then the prefixes [F] and the words; the search's tiles behind them
    const size_t own = seekListHead(F), head = own + ((size_t)F + 1) * sizeof(uint64_t) + sizeof(ZsFselWords);
    FindTiles t;
    if (const int e = findReserve(c, S, head, F, t)) return e;
    if (!c->dItems.reserve(sizeof(ZsDecItem) * (size_t)F)) return ZSMI_error_memory_allocation;
    const SeekListWords d = seekListWords(c->seek.dMeta.p, F);
    uint64_t *dPrefix = (uint64_t *)((uint8_t *)c->seek.dMeta.p + own);
    ZsFselWords *dWords = (ZsFselWords *)(dPrefix + F + 1);
    const ZsSeekEntry *dTable = (const ZsSeekEntry *)sk->dTable.p;
    const uint32_t grid = std::min((F + 255u) / 256u, 4096u);
    if (const int e = c->fill(dWords, 0, sizeof(ZsFselWords))) return e;
    LAUNCH(c, "k_findsel_list", k_findsel_list, dim3(grid), dim3(256), 0, dTable, sk->t.n, dFrames, dFrameCount, maxFrames, F, d.dList, d.dSizes, dWords);
    if (const int e = seekDecodeList(c, sk, d.dList, F, d, "k_find_scan", 1u, dWork, S)) return e;
    LAUNCH(c, "k_findsel_code", k_findsel_code, dim3(1), dim3(256), 0, (const uint32_t *)d.dCodes, dFrameCount, sk->maxDSize, S, dWords);
    LAUNCH(c, "k_findsel_fill", k_findsel_fill, dim3((uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((S + 255) / 256, 8192))), dim3(256), 0, (uint8_t *)dWork, S, (uint32_t)delim,
           dTable, (const uint32_t *)d.dList, (const uint64_t *)d.dSizes, (const uint64_t *)d.dListAt, F);
    if (const int e = findqText(c, dWork, S, delim, findQuery(q), nullptr, &dWords->code, dRecords, dHits, capacity, dWords->tmp, t)) return e;
    LAUNCH(c, "k_findsel_prefix", k_findsel_prefix, dim3(F), dim3(64), 0, (const uint8_t *)dWork, S, (uint32_t)delim, (const uint64_t *)d.dListAt, (const uint64_t *)t.dRecBase,
           (const ZsFselWords *)dWords, dPrefix);
    const uint32_t rgrid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((capacity + 255) / 256, 4096));
    LAUNCH(c, "k_findsel_renumber", k_findsel_renumber, dim3(rgrid), dim3(256), 0, dRecords, (const ZsFselWords *)dWords, (const uint64_t *)dPrefix, (const uint32_t *)d.dList,
           dTable, dFirstRecord, dResult);
    return c->launched();
}
extern "C" int zsmi_seekableFindQueryFramesResident(zsmi_ctx *c, const zsmi_seekable *sk, const uint64_t *dFirstRecord, uint32_t nFrames, int delim, const zsmi_findQuery *q,
                                                    const uint32_t *dFrames, const uint64_t *dFrameCount, uint32_t maxFrames, void *dWork, uint64_t workCapacity,
                                                    uint64_t *dRecords, uint8_t *dHits, uint64_t capacity, uint64_t *dResult)
{
    if (const int e = findselCheck(c, sk, dFirstRecord, nFrames, delim, q, dFrames, dFrameCount, maxFrames, false, dWork, workCapacity, dRecords, capacity, dResult)) return e;
    if (const int e = c->bind()) return e;
    return findselRun(c, sk, dFirstRecord, delim, q, dFrames, dFrameCount, maxFrames, dWork, workCapacity, dRecords, dHits, capacity, dResult);
}
// host arrays in and out (find.hip's findStage): the count goes up in front of the result words and the list behind them, the body above
// runs with a work buffer of the context's of the work bound of frameCount frames.  The staging of the numbers: capacity, or what the
// listed content can hold at most - its bytes / the shortest pattern
extern "C" int zsmi_seekableFindQueryFramesHost(zsmi_ctx *c, const zsmi_seekable *sk, const uint64_t *firstRecord, uint32_t nFrames, int delim, const zsmi_findQuery *q,
                                                const uint32_t *frames, uint32_t frameCount, uint64_t *records, uint8_t *hits, size_t capacity, uint64_t *result)
{
    const uint64_t count = frameCount;
    if (const int e = findselCheck(c, sk, firstRecord, nFrames, delim, q, frames, &count, frameCount, true, nullptr, 0, records, capacity, result)) return e;
    const uint64_t bound = zsmi_seekableFindFramesWorkBound(sk, frameCount);
    const size_t room = (size_t)std::min<uint64_t>(capacity, bound / findQueryShortest(q));
    return findStage(c, firstRecord, nFrames, bound, room, true, 1, (size_t)frameCount * sizeof(uint32_t), records, hits, result, [&](const FindStaged &s) {
        int rc = c->toDevice(s.dFront, &count, sizeof count);
        if (!rc && frameCount) rc = c->toDevice(s.dBack, frames, (size_t)frameCount * sizeof(uint32_t));
        return rc ? rc : findselRun(c, sk, s.dFirst, delim, q, (const uint32_t *)s.dBack, s.dFront, frameCount, s.dWork, bound, s.dRecords, s.dHits, room, s.dResult);
    });
}
