// records.hip -- records by number from a record archive (zsmi_records.h states the two rules): the last step of the pipeline text ->
// zsmi_splitRecordsDevice -> zsmi_compressSeekableFramesResident -> an opened archive.  The archive's handle, the firstRecord array the
// splitter left in device memory and record numbers in device memory become the records' bytes, packed, with offsets and a status a
// request; zsmi_seekableReadRecordsResident only queues work on the context's stream.
//
// The launch sequence, N requests, planned for R = maxFrameReads frame reads:
//   k_rec_lookup      a lane a request: zs_rec_frames over dFirstRecord -> (f, g, skip) or the request's refusal, whether it is a HEAD
//                     (it names frames and is no follower of the request in front: that one names other frames, or none), and for a
//                     head the frame reads (g - f + 1) and the work bytes (the content of frames f .. g) it needs
//   scanOffsets x 3   over the heads' reads, work bytes and flags: the read a head's list starts at, the totals dResult[1] and [2] state
//                     whatever the caps are, and the heads in front of each request - a follower's leader is the last request with fewer
//                     heads in front than the follower has (a binary search in k_rec_measure; the scan of the flags stands for a
//                     running maximum of the heads' positions)
//   k_rec_reads       a lane a FRAME READ: its head by binary search over the scanned reads, its frame number - or 0xFFFFFFFF behind the
//                     total and for a head whose list ends behind R or whose frames end behind workCapacity (from the first such head on
//                     every head is one: both sums only grow)
//   k_seek_request_sizes, scanOffsets, k_seek_request_items, decodeItems, k_seek_verify
//                     seekable.hip's frame-list decode (seekDecodeList) on that list, with dWork as its destination and align 1: a slot
//                     that names no frame is an empty item, the frames of a head lie back to back in dWork, and every read gets a code
//   k_rec_measure     a wavefront a request: its leader's first failing frame, in frame order, or the record's extent inside the
//                     leader's run in dWork (EXTENT, 16 bytes a lane a step)
//   scanOffsets       over the lengths, each rounded up to align: dDstOffsets (the rule of zsmi_layoutOutputsDevice)
//   k_rec_copy        a workgroup a request: the bytes to their place, or dstSize_tooSmall for a place that ends behind dstCapacity;
//                     dWritten, dStatus, dResult
// Scratch, all of it context buffers reserved before anything is queued: 80 bytes a request and 60 bytes a planned frame read in the
// seekable scratch, the decoder's item list and its scratch for R items.  Every store is a vector store from plain C++.

#include "zsmi_status.h"
#include "zsmi_wave.h"            // wave_incl_scan, wave_last, wave_min, zs_block_copy
#include "zsmi_ctx.h"             // the context, LAUNCH, scanOffsets, decodeItems
#include "zsmi_records.h"         // the rules: zs_rec_frames, zs_rec_extent
#include <algorithm>
// From the two feature files zsmi_api.hip includes in front of this one (neither can be included twice): seekable.hip - the handle
// (zsmi_seekable), its table (ZsSeekEntry), k_seek_request_sizes and the frame-list decode (SeekListWords, seekListHead, seekListWords,
// seekDecodeList); split.hip - zs_split_word_mask, the zero-byte test of a word XOR the delimiter, and ZsSplitBytes16, the 16 bytes a lane loads.

static const uint32_t kRecNoFrame = 0xFFFFFFFFu;         // a slot of the planned read list that names no frame

// ---- kernels ----
// what the lookup leaves of a request.  code: 0, or why it names no frames - frameIndex_tooLarge for a number at or above `records`,
// dstSize_tooSmall for frames whose content no size word holds (only an array that is not this archive's asks for that)
struct ZsRecReq { uint64_t skip; uint32_t f, g, code, head; };
struct ZsRecSpan { ZsRecFrames at; uint64_t bytes; uint32_t code; };
__device__ __forceinline__ ZsRecSpan zs_rec_span(const uint64_t *__restrict__ firstRecord, uint32_t nFrames, const uint64_t *__restrict__ content, uint64_t r)
{
    ZsRecSpan s; s.at.f = 0; s.at.g = 0; s.at.skip = 0; s.bytes = 0; s.code = ZSMI_error_frameIndex_tooLarge;
    if (nFrames == 0 || r >= firstRecord[nFrames]) return s;
    s.at = zs_rec_frames(firstRecord, nFrames, r);                                  // (f <= g < nFrames, whatever the array holds)
    s.bytes = content[s.at.g + 1] - content[s.at.f];
    s.code = s.bytes > ZS_ONESHOT_CAP_MAX ? (uint32_t)ZSMI_error_dstSize_tooSmall : 0u;
    return s;
}
__global__ void __launch_bounds__(256)
k_rec_lookup(const uint64_t *__restrict__ firstRecord, uint32_t nFrames, const uint64_t *__restrict__ content, const uint64_t *__restrict__ recordIndex, uint32_t n,
             ZsRecReq *__restrict__ reqs, uint32_t *__restrict__ reads, uint64_t *__restrict__ bytes, uint32_t *__restrict__ heads, uint64_t *__restrict__ result)
{
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k == 0) result[0] = n;                                                      // (k_rec_copy takes one off for every request that ends with a code)
    if (k >= n) return;
    const ZsRecSpan own = zs_rec_span(firstRecord, nFrames, content, recordIndex[k]);
    bool follower = false;
    if (k && !own.code) {
        const ZsRecSpan prev = zs_rec_span(firstRecord, nFrames, content, recordIndex[k - 1]);
        follower = !prev.code && prev.at.f == own.at.f && prev.at.g == own.at.g;
    }
    const bool head = !own.code && !follower;
    ZsRecReq q; q.skip = own.at.skip; q.f = own.at.f; q.g = own.at.g; q.code = own.code; q.head = head;
    reqs[k] = q;
    reads[k] = head ? own.at.g - own.at.f + 1u : 0u;
    bytes[k] = head ? own.bytes : 0ull;
    heads[k] = head;
}
// a head's list and frames fit the caps
__device__ __forceinline__ bool zs_rec_planned(uint64_t readAt, uint32_t reads, uint64_t workAt, uint64_t bytes, uint32_t maxFrameReads, uint64_t workCapacity)
{
    return readAt <= maxFrameReads && reads <= maxFrameReads - readAt && workAt <= workCapacity && bytes <= workCapacity - workAt;
}
// (a record cut into a million frames is a million lanes here, no lane's loop)
__global__ void __launch_bounds__(256)
k_rec_reads(const ZsRecReq *__restrict__ reqs, const uint64_t *__restrict__ readAt, const uint64_t *__restrict__ workAt, uint32_t n, uint32_t maxFrameReads,
            uint64_t workCapacity, uint32_t *__restrict__ list)
{
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= maxFrameReads) return;
    uint32_t frame = kRecNoFrame;
    if (j < readAt[n]) {
        uint32_t lo = 0, hi = n;                                                    // the first request whose list starts behind j: the one before it holds read j
        while (lo < hi) { const uint32_t mid = lo + (hi - lo) / 2; if (readAt[mid] <= j) lo = mid + 1; else hi = mid; }
        const uint32_t k = lo - 1;                                                  // (readAt[0] = 0 <= j; requests without reads share the next one's start: never the last at or below j)
        const ZsRecReq q = reqs[k];
        if (zs_rec_planned(readAt[k], q.g - q.f + 1u, workAt[k], workAt[k + 1] - workAt[k], maxFrameReads, workCapacity)) frame = q.f + (uint32_t)(j - readAt[k]);
    }
    list[j] = frame;
}

// bit k: byte k of the 16 is the delimiter (the idiom of k_split_count's masks, on its 16-byte record)
__device__ __forceinline__ uint32_t zs_rec_mask16(const ZsSplitBytes16 &b, uint32_t delim4)
{
    return zs_split_word_mask(b.w[0], delim4) | (zs_split_word_mask(b.w[1], delim4) << 4) | (zs_split_word_mask(b.w[2], delim4) << 8) | (zs_split_word_mask(b.w[3], delim4) << 12);
}
// the position of the t-th set bit of mask, t in 1 .. popcount
__device__ __forceinline__ uint32_t zs_rec_nth_bit(uint32_t mask, uint32_t t)
{
    for (uint32_t i = 1; i < t; i++) mask &= mask - 1u;
    return (uint32_t)__ffs((int)mask) - 1u;
}
// the lane whose 16 bytes hold delimiter number `need` of the step (1 .. the step's total) gives its place, counted from the step's start
__device__ __forceinline__ uint32_t zs_rec_find(uint32_t mask, uint32_t before, uint32_t incl, uint32_t need, uint32_t lane)
{
    const bool mine = before < need && need <= incl;
    return wave_min(mine ? 16u * lane + zs_rec_nth_bit(mask, need - before) : ~0u);
}
#define ZS_REC_AHEAD 4u                  // steps of 64 lanes x 16 bytes whose loads a wavefront issues together
// A wavefront a request (four to a workgroup).  A request that names frames finds its leader, the leader's place in the read list and in
// dWork; a leader the caps refused, or a frame of it that failed, ends the request with that code and no bytes.  Else EXTENT over the run
// run[0, len): the run is cut into 16-byte GROUPS at the addresses that are multiples of 16, lane i of a step takes group 64 s + i - a
// wavefront's loads are one contiguous, aligned KiB, ZS_REC_AHEAD steps' loads issued together - and counts its delimiters by the
// zero-byte test; the running count over lanes (wave_incl_scan) and steps finds delimiter `skip` (the record starts behind it) and
// delimiter skip + 1 (it ends behind that one).  The first and the last group, where they are not whole, go byte by byte: no byte outside
// the run is read.  start[k]: the record's first byte, counted from dWork; length[k]; status[k].
__global__ void __launch_bounds__(256)
k_rec_measure(const ZsRecReq *__restrict__ reqs, const uint64_t *__restrict__ readAt, const uint64_t *__restrict__ workAt, const uint64_t *__restrict__ headsBefore,
              uint32_t n, uint32_t maxFrameReads, uint64_t workCapacity, const uint64_t *__restrict__ listAt, const uint32_t *__restrict__ codes,
              const uint8_t *__restrict__ work, uint32_t delim, uint64_t *__restrict__ start, uint64_t *__restrict__ length, uint32_t *__restrict__ status)
{
    const uint32_t k = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (k >= n) return;                                                             // (the same for every lane of a wavefront, as everything below but the masks)
    const ZsRecReq q = reqs[k];
    uint32_t code = q.code;
    uint64_t from = 0, len = 0;
    if (!code) {
        uint32_t leader = k;
        if (!q.head) {
            const uint64_t h = headsBefore[k];                                      // (>= 1: a follower has its leader in front)
            uint32_t lo = 0, hi = k;                                                // the first request with h heads in front: the one before it is head h - 1
            while (lo < hi) { const uint32_t mid = lo + (hi - lo) / 2; if (headsBefore[mid] < h) lo = mid + 1; else hi = mid; }
            leader = lo - 1;
        }
        const uint64_t r0 = readAt[leader], bytes = workAt[leader + 1] - workAt[leader];
        const uint32_t reads = q.g - q.f + 1u;
        if (!zs_rec_planned(r0, reads, workAt[leader], bytes, maxFrameReads, workCapacity)) code = ZSMI_error_dstSize_tooSmall;
        for (uint32_t i0 = 0; !code && i0 < reads; i0 += 64u) {                     // the first failing frame, in frame order
            const uint32_t i = i0 + lane;
            const uint32_t c = i < reads ? codes[r0 + i] : 0u;
            const uint32_t first = wave_min(c ? i : ~0u);
            if (first != ~0u) code = codes[r0 + first];
        }
        if (!code && q.skip > bytes) code = ZSMI_error_corruption_detected;        // (more delimiters than bytes)
        const uint64_t at = code ? 0ull : listAt[r0];                               // where the leader's frames start in dWork
        if (!code && (at > workCapacity || bytes > workCapacity - at)) code = ZSMI_error_GENERIC;      // (the planned heads are the first ones, so at is workAt[leader]: never)
        if (!code) {
            const uint8_t *run = work + at;
            const uint32_t lead = (uint32_t)((uintptr_t)run & 15u);                 // the run starts at byte `lead` of group 0
            const uint8_t *group0 = run - lead;
            const uint64_t groups = (lead + bytes + 15u) / 16u;
            const uint64_t wholeLo = lead ? 1u : 0u, wholeHi = (lead + bytes) / 16u;        // groups [wholeLo, wholeHi) lie inside the run
            const uint32_t delim4 = delim * 0x01010101u;
            uint64_t seen = 0, end = bytes;
            bool started = q.skip == 0, ended = false;
            for (uint64_t g0 = 0; g0 < groups && !ended; g0 += 64u * ZS_REC_AHEAD) {
                uint32_t mask[ZS_REC_AHEAD];
                ZsSplitBytes16 own[ZS_REC_AHEAD];
                if (wholeLo < wholeHi) {
                    #pragma unroll
                    for (uint32_t s = 0; s < ZS_REC_AHEAD; s++) {                    // (a group that is not whole loads a whole one in its place and drops it)
                        const uint64_t mine = g0 + 64u * s + lane;
                        const uint64_t g = mine < wholeLo ? wholeLo : (mine < wholeHi ? mine : wholeHi - 1u);
                        __builtin_memcpy(&own[s], __builtin_assume_aligned(group0 + 16u * g, 16), 16);
                    }
                }
                #pragma unroll
                for (uint32_t s = 0; s < ZS_REC_AHEAD; s++) {
                    const uint64_t g = g0 + 64u * s + lane;
                    uint32_t m = 0;
                    if (g >= wholeLo && g < wholeHi) m = zs_rec_mask16(own[s], delim4);
                    else if (g < groups)
                        for (uint32_t j = 0; j < 16; j++) {
                            const uint64_t p = 16u * g + j;                         // (counted from group 0)
                            if (p >= lead && p < lead + bytes && group0[p] == delim) m |= 1u << j;
                        }
                    mask[s] = m;
                }
                #pragma unroll
                for (uint32_t s = 0; s < ZS_REC_AHEAD; s++) {
                    if (ended) break;
                    const uint32_t pop = (uint32_t)__popc(mask[s]), incl = wave_incl_scan(pop), total = wave_last(incl);
                    const uint64_t stepAt = 16u * (g0 + 64u * s);                   // the step's first byte, counted from group 0
                    if (!started && seen + total >= q.skip) {
                        from = stepAt + zs_rec_find(mask[s], incl - pop, incl, (uint32_t)(q.skip - seen), lane) + 1u - lead;
                        started = true;
                    }
                    if (started && seen + total > q.skip) {
                        end = stepAt + zs_rec_find(mask[s], incl - pop, incl, (uint32_t)(q.skip + 1u - seen), lane) + 1u - lead;
                        ended = true;
                    }
                    seen += total;
                }
            }
            if (!started) code = ZSMI_error_corruption_detected;                    // fewer than skip delimiters
            else { len = end - from; from += at; }
        }
    }
    if (lane == 0) { start[k] = code ? 0ull : from; length[k] = code ? 0ull : len; status[k] = code; }
}
// behind the layout scan over the lengths, a workgroup a request
__global__ void __launch_bounds__(256)
k_rec_copy(const uint8_t *__restrict__ work, const uint64_t *__restrict__ start, const uint64_t *__restrict__ length, const uint64_t *__restrict__ dstOffsets,
           const uint64_t *__restrict__ readAt, const uint64_t *__restrict__ workAt, uint32_t n, uint64_t dstCapacity, uint8_t *__restrict__ dst,
           uint64_t *__restrict__ written, uint32_t *__restrict__ status, unsigned long long *result)
{
    const uint32_t k = blockIdx.x;
    const uint64_t len = length[k], at = dstOffsets[k];
    uint32_t code = status[k];
    const bool fits = at <= dstCapacity && len <= dstCapacity - at;
    if (!code && !fits) code = ZSMI_error_dstSize_tooSmall;
    if (!code) zs_block_copy(dst + at, work + start[k], (uint32_t)len, threadIdx.x, 256u);      // (len: at most a size word's, k_rec_lookup)
    if (threadIdx.x) return;
    written[k] = len; status[k] = code;
    if (code) atomicAdd(&result[0], ~0ull);
    if (k == 0) { result[1] = readAt[n]; result[2] = workAt[n]; result[3] = dstOffsets[n]; }
}

// ---- host ----
extern "C" size_t zsmi_seekableRecordsWorkBound(const zsmi_seekable *sk, uint32_t maxFrameReads)
{
    return sk ? (size_t)maxFrameReads * sk->maxDSize : 0;
}
// the header's checks, in its order
static int recordsCheck(const zsmi_ctx *c, const zsmi_seekable *sk, const void *firstRecord, uint32_t nFrames, int delim, const void *recordIndex, uint32_t nRecords,
                        uint32_t maxFrameReads, uint32_t align, const void *work, uint64_t workCapacity, const void *dst, uint64_t dstCapacity,
                        const void *dstOffsets, const void *written, const void *status, const void *result)
{
    if (!c) return ZSMI_error_init_missing;
    if (!sk || !dstOffsets || !result || (nRecords && (!firstRecord || !recordIndex || !written || !status))) return ZSMI_error_GENERIC;
    if (sk->device != c->device) return ZSMI_error_parameter_unsupported;
    if (delim < 0 || delim > 255 || align == 0 || align > 4096 || (align & (align - 1)) || nFrames != sk->t.n) return ZSMI_error_parameter_outOfBound;
    if (maxFrameReads > ZS_REC_MAX_FRAME_READS) return ZSMI_error_frameIndex_tooLarge;
    if (nRecords && ((dstCapacity && !dst) || (workCapacity && !work))) return ZSMI_error_GENERIC;
    return 0;
}
// the launch sequence, its arguments checked by the caller
static int recordsRead(zsmi_ctx *c, const zsmi_seekable *sk, const uint64_t *dFirstRecord, uint32_t nFrames, int delim, const uint64_t *dRecordIndex, uint32_t nRecords,
                       uint32_t maxFrameReads, uint32_t align, void *dWork, uint64_t workCapacity, void *dDst, uint64_t dstCapacity,
                       uint64_t *dDstOffsets, uint64_t *dWritten, uint32_t *dStatus, uint64_t *dResult)
{
    if (const int e = c->bind()) return e;
    if (nRecords == 0) {
        if (const int e = c->fill(dDstOffsets, 0, sizeof(uint64_t))) return e;
        return c->fill(dResult, 0, 4 * sizeof(uint64_t));
    }
    const size_t N = nRecords, R = maxFrameReads;
    // device words, a request: 64 bits - work bytes [N], the three scans [N + 1 each], starts [N], lengths [N]; the lookup's records [N];
    // 32 bits - reads [N], head flags [N] (8 N bytes: what follows is 8-aligned).  Behind them the frame-list decode's words of R frame reads
    const size_t own = (6 * N + 3) * sizeof(uint64_t) + N * sizeof(ZsRecReq) + 2 * N * sizeof(uint32_t);
    if (!c->seek.dMeta.reserve(own + seekListHead(R)) || !c->dItems.reserve(sizeof(ZsDecItem) * std::max<size_t>(R, 1))) return ZSMI_error_memory_allocation;
    uint64_t *dBytes = (uint64_t *)c->seek.dMeta.p, *dReadAt = dBytes + N, *dWorkAt = dReadAt + N + 1, *dHeadsBefore = dWorkAt + N + 1, *dStart = dHeadsBefore + N + 1,
             *dLength = dStart + N;
    ZsRecReq *dReqs = (ZsRecReq *)(dLength + N);
    uint32_t *dReads = (uint32_t *)(dReqs + N), *dHeads = dReads + N;
    const SeekListWords d = seekListWords((uint8_t *)c->seek.dMeta.p + own, R);
    const uint32_t grid = (nRecords + 255) / 256, readGrid = (maxFrameReads + 255) / 256;
    LAUNCH(c, "k_rec_lookup", k_rec_lookup, dim3(grid), dim3(256), 0, dFirstRecord, nFrames, sk->dContent, dRecordIndex, nRecords, dReqs, dReads, dBytes, dHeads, dResult);
    if (const int e = scanOffsets(c, "k_rec_scan", (const uint32_t *)dReads, nullptr, nRecords, 1u, nullptr, dReadAt)) return e;
    if (const int e = scanOffsets(c, "k_rec_scan", (const uint64_t *)dBytes, nullptr, nRecords, 1u, nullptr, dWorkAt)) return e;
    if (const int e = scanOffsets(c, "k_rec_scan", (const uint32_t *)dHeads, nullptr, nRecords, 1u, nullptr, dHeadsBefore)) return e;
    if (maxFrameReads) {
        LAUNCH(c, "k_rec_reads", k_rec_reads, dim3(readGrid), dim3(256), 0, (const ZsRecReq *)dReqs, (const uint64_t *)dReadAt, (const uint64_t *)dWorkAt, nRecords, maxFrameReads,
               workCapacity, d.dList);
        LAUNCH(c, "k_seek_request_sizes", k_seek_request_sizes, dim3(readGrid), dim3(256), 0, (const ZsSeekEntry *)sk->dTable.p, sk->t.n, (const uint32_t *)d.dList, maxFrameReads, d.dSizes);
    }
    if (const int e = seekDecodeList(c, sk, d.dList, maxFrameReads, d, "k_rec_scan", 1u, dWork, workCapacity)) return e;
    LAUNCH(c, "k_rec_measure", k_rec_measure, dim3((nRecords + 3) / 4), dim3(256), 0, (const ZsRecReq *)dReqs, (const uint64_t *)dReadAt, (const uint64_t *)dWorkAt,
           (const uint64_t *)dHeadsBefore, nRecords, maxFrameReads, workCapacity, (const uint64_t *)d.dListAt, (const uint32_t *)d.dCodes, (const uint8_t *)dWork, (uint32_t)delim,
           dStart, dLength, dStatus);
    if (const int e = scanOffsets(c, "k_layout_outputs", (const uint64_t *)dLength, nullptr, nRecords, align, nullptr, dDstOffsets)) return e;
    LAUNCH(c, "k_rec_copy", k_rec_copy, dim3(nRecords), dim3(256), 0, (const uint8_t *)dWork, (const uint64_t *)dStart, (const uint64_t *)dLength, (const uint64_t *)dDstOffsets,
           (const uint64_t *)dReadAt, (const uint64_t *)dWorkAt, nRecords, dstCapacity, (uint8_t *)dDst, dWritten, dStatus, (unsigned long long *)dResult);
    return c->launched();
}
extern "C" int zsmi_seekableReadRecordsResident(zsmi_ctx *c, const zsmi_seekable *sk, const uint64_t *dFirstRecord, uint32_t nFrames, int delim,
                                                const uint64_t *dRecordIndex, uint32_t nRecords, uint32_t maxFrameReads, uint32_t align,
                                                void *dWork, uint64_t workCapacity, void *dDst, uint64_t dstCapacity,
                                                uint64_t *dDstOffsets, uint64_t *dWritten, uint32_t *dStatus, uint64_t *dResult)
{
    if (const int e = recordsCheck(c, sk, dFirstRecord, nFrames, delim, dRecordIndex, nRecords, maxFrameReads, align, dWork, workCapacity, dDst, dstCapacity,
                                   dDstOffsets, dWritten, dStatus, dResult)) return e;
    if (nRecords > 0x7FFFFFFFu) return ZSMI_error_memory_allocation;               // (a workgroup a request: a grid's limit)
    return recordsRead(c, sk, dFirstRecord, nFrames, delim, dRecordIndex, nRecords, maxFrameReads, align, dWork, workCapacity, dDst, dstCapacity,
                       dDstOffsets, dWritten, dStatus, dResult);
}
// host arrays in, a host buffer out.  The host holds firstRecord, so it runs the lookup's rule itself for what the device call is told:
// the frame reads and work bytes of the heads, and the most the records can be - the heads' and followers' runs - for the destination's
// staging (never above dstCapacity).  Uploads, the body above with align 1, the results down, one wait for dResult and one for the bytes.
extern "C" int zsmi_seekableReadRecordsHost(zsmi_ctx *c, const zsmi_seekable *sk, const uint64_t *firstRecord, uint32_t nFrames, int delim,
                                            const uint64_t *recordIndex, uint32_t nRecords, void *dst, size_t dstCapacity, uint64_t *dstOffsets, uint32_t *statuses)
{
    uint64_t result[4] = { 0, 0, 0, 0 };
    // (the host form has no dWritten and takes no dWork: statuses stands in for the one, no capacity for the other)
    if (const int e = recordsCheck(c, sk, firstRecord, nFrames, delim, recordIndex, nRecords, 0, 1, nullptr, 0, dst, dstCapacity, dstOffsets, statuses, statuses, result)) return e;
    if (nRecords == 0) { dstOffsets[0] = 0; return 0; }
    if (nRecords > 0x7FFFFFFFu) return ZSMI_error_memory_allocation;
    uint64_t reads = 0, work = 0, room = 0;
    ZsRecFrames prev = { 0, 0, 0 }; bool prevNamed = false;
    for (uint32_t k = 0; k < nRecords; k++) {
        bool named = nFrames && recordIndex[k] < firstRecord[nFrames];
        ZsRecFrames at = { 0, 0, 0 };
        uint64_t bytes = 0;
        if (named) { at = zs_rec_frames(firstRecord, nFrames, recordIndex[k]); bytes = sk->t.dOff[at.g + 1] - sk->t.dOff[at.f]; named = bytes <= ZS_ONESHOT_CAP_MAX; }
        if (named) {
            room += bytes;
            if (!(prevNamed && prev.f == at.f && prev.g == at.g)) { reads += at.g - at.f + 1u; work += bytes; }
        }
        prev = at; prevNamed = named;
    }
    if (reads > ZS_REC_MAX_FRAME_READS) return ZSMI_error_frameIndex_tooLarge;
    room = std::min<uint64_t>(room, dstCapacity);
    if (const int e = c->bind()) return e;
    // staging: firstRecord [nFrames + 1], numbers [n], offsets [n + 1], lengths [n], dResult [4]; status [n]
    const size_t N = nRecords, words = (size_t)nFrames + 1 + 3 * N + 1 + 4;
    if (!c->sSizes.reserve(words * sizeof(uint64_t) + N * sizeof(uint32_t)) || !c->seek.dDec.reserve(work + 64) || !c->sDst.reserve(room + 64)) return ZSMI_error_memory_allocation;
    uint64_t *dFirst = (uint64_t *)c->sSizes.p, *dIndex = dFirst + nFrames + 1, *dOffsets = dIndex + N, *dWritten = dOffsets + N + 1, *dResult = dWritten + N;
    uint32_t *dStatus = (uint32_t *)(dResult + 4);
    int rc = c->toDevice(dFirst, firstRecord, ((size_t)nFrames + 1) * sizeof(uint64_t));
    if (!rc) rc = c->toDevice(dIndex, recordIndex, N * sizeof(uint64_t));
    if (!rc) rc = recordsRead(c, sk, dFirst, nFrames, delim, dIndex, nRecords, (uint32_t)reads, 1, c->seek.dDec.p, work, c->sDst.p, dstCapacity, dOffsets, dWritten, dStatus, dResult);
    if (!rc) rc = c->toHost(dstOffsets, dOffsets, (N + 1) * sizeof(uint64_t));
    if (!rc) rc = c->toHost(statuses, dStatus, N * sizeof(uint32_t));
    if (!rc) rc = c->toHost(result, dResult, sizeof result);
    const int waited = c->wait();                                                  // (whatever was queued, a failed call included)
    if (rc || waited) return rc ? rc : waited;
    // the bytes of the requests that fit lie in front of the first place that ends behind dstCapacity, at the latest
    uint64_t used = 0;
    for (uint32_t k = 0; k < nRecords; k++) if (!statuses[k]) used = std::max(used, dstOffsets[k + 1]);
    if (used) { if (c->toHost(dst, c->sDst.p, used) || c->wait()) return ZSMI_error_GENERIC; }
    return 0;
}
