// split.hip -- the record splitter: delimited records in device memory -> the frame sizes of a record archive (zsmi_split.h states the
// rule; zsmi_splitRecords runs it serially on the host).  The step in front of the resident calls: what it leaves in device memory is what
// zsmi_compressSeekableFramesResident takes, and firstRecord is the line-number index a reader looks frames up in.
//
// The launch sequence of zsmi_splitRecordsDevice, every kernel a lane an item, modelled on the frame index (seekable.hip, k_index_*):
//   k_split_count   a workgroup a 16 KiB tile: the record ends in it (a bit a byte: the byte is the delimiter, or the stream's last) and
//                   the tile's last record end
//   scanOffsets     over the tiles' counts: the records in front of each tile; the total is `records`
//   k_split_emit    the same masks again: the ascending record ends E[r] and each record's extra cuts (L - 1) / M, for r < maxPieces; the
//                   sum of ALL records' extra cuts, so that pieces = records + that sum is exact however small maxPieces is
//   scanOffsets     over the extra cuts: X[r], the cuts in front of record r - record r's pieces are r + X[r] .. r + X[r + 1]
//   k_split_pieces  a lane a PIECE: its record by binary search over r + X[r], its end (a cut, or the record's end)
//   k_split_succ    a lane a frame-start NODE (node 0: position 0, node i: piece end i - 1): the node its frame ends at, under rule 3, by
//                   binary search over the piece ends
//   k_index_jump    the nodes the head reaches, by pointer doubling: ceil(log2(maxPieces + 1)) rounds.  None with targetSize 0: every
//                   node is a frame
//   scanOffsets     over the marks: a frame's slot
//   k_split_table   a marked node writes its frame's size and firstRecord (the rank of its start among the record ends) at its slot; the
//                   first lane dResult and firstRecord[n]
// When pieces > maxPieces the kernels behind k_split_emit write no list, and k_split_table only dResult.
// Scratch, all of it context buffers reserved before anything is queued: 12 bytes a tile and 16 more (the size staging) and 40 bytes a
// piece of maxPieces (the seekable scratch): 8 a record end, 8 a piece end, 8 for the extra cuts' scan and later the slots, 16 a node for
// the successors, the two jump arrays (the first holds the extra cuts before) and the marks.
// Every store is a vector store from plain C++.

#include "zsmi_status.h"
#include "zsmi_wave.h"            // wave_sum, wave_incl_scan, wave_max
#include "zsmi_ctx.h"             // the context, LAUNCH, scanOffsets
#include "zsmi_split.h"           // the rule: zs_split_check, zs_split_extra_cuts, the host loop
#include "entropy_kernels.hip"    // ZS_SCAN_TILE: the items of a scan's tile
#include <algorithm>

// the frame index's round of pointer doubling (seekable.hip, launched as it is): a successor at or above m is none
__global__ void __launch_bounds__(256) k_index_jump(const uint32_t *__restrict__ jump, uint32_t *__restrict__ squared, uint32_t *mark, uint32_t m);
static const uint32_t kSplitEnd = 0xFFFFFFFFu;           // a successor that is none: the stream's end (kIndexEnd)

#define ZS_SPLIT_TILE 16384u             // the bytes a workgroup scans: 4 steps x 256 threads x 16 bytes
static const uint32_t kSplitExtraMax = 0x80000001u;      // an extra-cut count as the scan sees it: above every maxPieces, below every error word

// ---- kernels ----
// bit k: byte k of the word is zero - exact for every byte (no borrow crosses a byte) - gathered into the low four bits
__device__ __forceinline__ uint32_t zs_split_word_mask(uint32_t w, uint32_t delim4)
{
    const uint32_t x = w ^ delim4;
    const uint32_t zero = ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) & 0x80808080u;
    return (((zero >> 7) * 0x00204081u) >> 21) & 0xFu;
}
// The record ends of tile `tile`: mask[s] bit k stands for the byte at tile * ZS_SPLIT_TILE + s * 4096 + 16 * threadIdx.x + k, a record
// end BEHIND it, so the ends ascend with (s, thread, k).  Lane i reads the 16 bytes at base + 16 i - a wavefront's loads one contiguous
// KiB, the four steps' loads issued together.  The stream's last tile, unless it is a whole one, goes byte by byte: no byte outside
// [src, src + size) is read.  The stream's last byte ends a record whatever it is (rule 1's tail).
struct ZsSplitBytes16 { uint32_t w[4]; };
__device__ __forceinline__ void zs_split_tile_masks(const uint8_t *__restrict__ src, uint64_t size, uint32_t delim, uint64_t tile, uint32_t mask[4])
{
    const uint64_t base = tile * ZS_SPLIT_TILE + 16u * threadIdx.x;
    const uint32_t delim4 = delim * 0x01010101u;
    if (size - tile * ZS_SPLIT_TILE >= ZS_SPLIT_TILE) {
        ZsSplitBytes16 own[4];
        #pragma unroll
        for (uint32_t s = 0; s < 4; s++) __builtin_memcpy(&own[s], src + base + s * 4096u, 16);
        #pragma unroll
        for (uint32_t s = 0; s < 4; s++)
            mask[s] = zs_split_word_mask(own[s].w[0], delim4) | (zs_split_word_mask(own[s].w[1], delim4) << 4) |
                      (zs_split_word_mask(own[s].w[2], delim4) << 8) | (zs_split_word_mask(own[s].w[3], delim4) << 12);
    } else {
        for (uint32_t s = 0; s < 4; s++) {
            const uint64_t b = base + s * 4096u;
            uint32_t m = 0;
            for (uint32_t j = 0; j < 16; j++) if (b + j < size && src[b + j] == delim) m |= 1u << j;
            mask[s] = m;
        }
    }
    const uint64_t last = size - 1;                                       // (size > 0: no tile otherwise)
    if (last / ZS_SPLIT_TILE == tile) {
        const uint32_t r = (uint32_t)(last % ZS_SPLIT_TILE);
        #pragma unroll
        for (uint32_t s = 0; s < 4; s++) if (r / 4096u == s && (r % 4096u) / 16u == threadIdx.x) mask[s] |= 1u << (r % 16u);
    }
}
// the record end, counted from the tile's start, behind the highest bit of step s's mask; 0 for no bit
__device__ __forceinline__ uint32_t zs_split_last_end(uint32_t mask, uint32_t s)
{
    return mask ? s * 4096u + 16u * threadIdx.x + (32u - (uint32_t)__clz((int)mask)) : 0u;
}
// counts[tile]: its record ends; lastEnd[tile]: the last of them, counted from the tile's start (0: the tile has none)
__global__ void __launch_bounds__(256)
k_split_count(const uint8_t *__restrict__ src, uint64_t size, uint32_t delim, uint32_t *__restrict__ counts, uint32_t *__restrict__ lastEnd)
{
    __shared__ uint32_t waves[4], ends[4];
    uint32_t mask[4];
    zs_split_tile_masks(src, size, delim, blockIdx.x, mask);
    const uint32_t n = wave_sum(__popc(mask[0]) + __popc(mask[1]) + __popc(mask[2]) + __popc(mask[3]));
    uint32_t e = 0;
    #pragma unroll
    for (uint32_t s = 0; s < 4; s++) e = max(e, zs_split_last_end(mask[s], s));
    e = wave_max(e);
    if ((threadIdx.x & 63u) == 0) { waves[threadIdx.x >> 6] = n; ends[threadIdx.x >> 6] = e; }
    __syncthreads();
    if (threadIdx.x == 0) {
        counts[blockIdx.x] = waves[0] + waves[1] + waves[2] + waves[3];
        lastEnd[blockIdx.x] = max(max(ends[0], ends[1]), max(ends[2], ends[3]));
    }
}
// the inclusive running maximum over the wavefront's lanes (wave_incl_scan with max: the row shifts' zero fill is its identity)
__device__ __forceinline__ uint32_t zs_split_wave_incl_max(uint32_t v)
{
    v = max(v, ZS_DPP(0, v, 0x111, 0xF, true));
    v = max(v, ZS_DPP(0, v, 0x112, 0xF, true));
    v = max(v, ZS_DPP(0, v, 0x114, 0xF, true));
    v = max(v, ZS_DPP(0, v, 0x118, 0xF, true));
    v = max(v, ZS_DPP(0, v, 0x142, 0xA, false));
    v = max(v, ZS_DPP(0, v, 0x143, 0xC, false));
    return v;
}
// The masks again.  tileBase[tile]: the records in front of the tile (tileBase[tiles]: all).  A step's ends follow the steps before it, a
// wavefront's the wavefronts before it, a thread's the lanes before it; the same order gives every end its PREDECESSOR - the record's
// start: the end before it in the thread, else the last one of the lanes, wavefronts and steps in front, else the last end of the nearest
// tile in front that has one (found in tileBase by binary search: the tile that holds the record before this tile's first), else 0.
// E and extra are written below maxPieces only; the extra cuts of every record are summed, a workgroup's in LDS, into *extraTotal.
__global__ void __launch_bounds__(256)
k_split_emit(const uint8_t *__restrict__ src, uint64_t size, uint32_t delim, const uint64_t *__restrict__ tileBase, const uint32_t *__restrict__ lastEnd,
             uint32_t maxFrameSize, uint64_t *__restrict__ E, uint32_t *__restrict__ extra, uint32_t maxPieces, unsigned long long *extraTotal)
{
    __shared__ uint32_t counts[4][4], ends[4][4];
    __shared__ unsigned long long front, sum;
    uint32_t mask[4], before[4], prev[4];
    zs_split_tile_masks(src, size, delim, blockIdx.x, mask);
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    #pragma unroll
    for (uint32_t s = 0; s < 4; s++) {
        const uint32_t n = __popc(mask[s]), incl = wave_incl_scan(n);
        before[s] = incl - n;
        const uint32_t own = zs_split_last_end(mask[s], s);
        const uint32_t upTo = zs_split_wave_incl_max(own);
        const uint32_t ahead = (uint32_t)__shfl_up((int)upTo, 1);                 // the lanes in front of this one
        prev[s] = lane ? ahead : 0u;
        if (lane == 63u) { counts[s][wave] = incl; ends[s][wave] = upTo; }
    }
    if (threadIdx.x == 0) {
        const uint64_t g = tileBase[blockIdx.x];
        unsigned long long f = 0;
        if (g) {
            uint32_t lo = 0, hi = blockIdx.x;                                      // the first tile with g records in front: the one before it holds record g - 1
            while (lo < hi) { const uint32_t mid = lo + (hi - lo) / 2; if (tileBase[mid] < g) lo = mid + 1; else hi = mid; }
            f = (unsigned long long)(lo - 1) * ZS_SPLIT_TILE + lastEnd[lo - 1];
        }
        front = f; sum = 0;
    }
    __syncthreads();
    const uint64_t tileAt = (uint64_t)blockIdx.x * ZS_SPLIT_TILE;
    uint64_t at = tileBase[blockIdx.x], mine = 0;
    uint32_t tileFront = 0;                                                       // the last end of the steps in front, from the tile's start
    #pragma unroll
    for (uint32_t s = 0; s < 4; s++) {
        uint32_t ahead = 0, all = 0, p = max(tileFront, prev[s]);
        #pragma unroll
        for (uint32_t w = 0; w < 4; w++) {
            ahead += w < wave ? counts[s][w] : 0u; all += counts[s][w];
            p = max(p, w < wave ? ends[s][w] : 0u); tileFront = max(tileFront, ends[s][w]);
        }
        uint64_t out = at + ahead + before[s];
        uint64_t start = p ? tileAt + p : front;
        const uint64_t b = tileAt + s * 4096u + 16u * threadIdx.x;
        for (uint32_t bits = mask[s]; bits; bits &= bits - 1u, out++) {
            const uint64_t end = b + (uint32_t)__ffs((int)bits);
            const uint64_t x = zs_split_extra_cuts(end - start, maxFrameSize);
            mine += x;
            if (out < maxPieces) { E[out] = end; extra[out] = x < kSplitExtraMax ? (uint32_t)x : kSplitExtraMax; }
            start = end;
        }
        at += all;
    }
    if (mine) atomicAdd(&sum, (unsigned long long)mine);
    __syncthreads();
    if (threadIdx.x == 0 && sum) atomicAdd(extraTotal, sum);
}
// what every kernel behind the emit reads first: records, pieces, and whether the lists hold them
struct ZsSplitCounts { uint64_t records, pieces; bool fits; };
__device__ __forceinline__ ZsSplitCounts zs_split_counts(const uint64_t *records, const unsigned long long *extraTotal, uint32_t maxPieces)
{
    ZsSplitCounts c; c.records = *records; c.pieces = c.records + *extraTotal; c.fits = c.pieces <= maxPieces;
    return c;
}
// a lane a piece: k's record is the last r with r + X[r] <= k; inside it piece j ends at the record's start + (j + 1) M, the last one at
// the record's end.  (One record of 1 GiB with M = 1 KiB is a million lanes here, no lane's loop)
__global__ void __launch_bounds__(256)
k_split_pieces(const uint64_t *__restrict__ E, const uint64_t *__restrict__ X, const uint64_t *__restrict__ records, const unsigned long long *__restrict__ extraTotal,
               uint32_t maxFrameSize, uint32_t maxPieces, uint64_t *__restrict__ PE)
{
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    const ZsSplitCounts c = zs_split_counts(records, extraTotal, maxPieces);
    if (!c.fits || k >= c.pieces) return;
    uint32_t lo = 0, hi = (uint32_t)c.records;                                     // (records <= pieces <= maxPieces; lo: the first r with r + X[r] > k)
    while (lo < hi) { const uint32_t mid = lo + (hi - lo) / 2; if (mid + X[mid] <= k) lo = mid + 1; else hi = mid; }
    const uint32_t r = lo - 1;                                                     // (0 + X[0] = 0 <= k: lo >= 1)
    const uint64_t j = k - (r + X[r]), cuts = X[r + 1] - X[r];
    const uint64_t start = r ? E[r - 1] : 0ull;
    PE[k] = j < cuts ? start + (j + 1) * maxFrameSize : E[r];
}
// a lane a node: the node the frame that starts here ends at - rule 3 - or kSplitEnd for the stream's end; nodes at or behind `pieces`
// (and every node when the pieces do not fit) get kSplitEnd and no mark.  T == 0: every node is a frame and is marked here; else the head
__global__ void __launch_bounds__(256)
k_split_succ(const uint64_t *__restrict__ PE, const uint64_t *__restrict__ records, const unsigned long long *__restrict__ extraTotal, uint32_t targetSize,
             uint32_t maxPieces, uint32_t *__restrict__ next, uint32_t *__restrict__ mark)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= maxPieces) return;
    const ZsSplitCounts c = zs_split_counts(records, extraTotal, maxPieces);
    if (!c.fits || i >= c.pieces) { next[i] = kSplitEnd; mark[i] = 0u; return; }
    const uint32_t P = (uint32_t)c.pieces;
    uint32_t j = i + 1;
    if (targetSize) {
        const uint64_t limit = (i ? PE[i - 1] : 0ull) + targetSize;
        uint32_t lo = i, hi = (uint32_t)min((uint64_t)P, (uint64_t)i + targetSize);    // (a piece is a byte at least) lo: the piece ends at or below limit
        while (lo < hi) { const uint32_t mid = lo + (hi - lo) / 2; if (PE[mid] <= limit) lo = mid + 1; else hi = mid; }
        j = max(lo, i + 1);                                                        // (none fits: the first piece alone)
    }
    next[i] = j < P ? j : kSplitEnd;
    mark[i] = targetSize ? i == 0 : 1u;
}
// the marked nodes at the slots the scan over the marks gives them.  slot[maxPieces]: the frames
__global__ void __launch_bounds__(256)
k_split_table(const uint64_t *__restrict__ E, const uint64_t *__restrict__ PE, const uint32_t *__restrict__ next, const uint32_t *__restrict__ mark,
              const uint64_t *__restrict__ slot, const uint64_t *__restrict__ records, const unsigned long long *__restrict__ extraTotal, uint32_t maxPieces,
              uint32_t *__restrict__ frameSizes, uint64_t *__restrict__ firstRecord, uint64_t *__restrict__ result)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const ZsSplitCounts c = zs_split_counts(records, extraTotal, maxPieces);
    if (i == 0) {
        const uint64_t n = slot[maxPieces];
        result[0] = c.fits ? n : 0ull - (uint64_t)ZSMI_error_dstSize_tooSmall; result[1] = c.records; result[2] = c.pieces;
        if (c.fits && firstRecord && n <= maxPieces) firstRecord[n] = c.records;
    }
    if (!c.fits || i >= c.pieces || !mark[i]) return;
    const uint64_t at = slot[i];
    if (at >= maxPieces) return;                                                   // (the marks are below `pieces`: never)
    const uint64_t start = i ? PE[i - 1] : 0ull, end = PE[(next[i] == kSplitEnd ? (uint32_t)c.pieces : next[i]) - 1u];
    frameSizes[at] = (uint32_t)(end - start);
    if (!firstRecord) return;
    uint32_t lo = 0, hi = (uint32_t)c.records;                                     // the record ends at or below start: the delimiters in front of it
    while (lo < hi) { const uint32_t mid = lo + (hi - lo) / 2; if (E[mid] <= start) lo = mid + 1; else hi = mid; }
    firstRecord[at] = lo;
}

// ---- host ----
extern "C" size_t zsmi_splitRecords(const void *src, size_t srcSize, int delim, uint32_t targetSize, uint32_t maxFrameSize,
                                    uint32_t *frameSizes, uint64_t *firstRecord, size_t capacity, uint64_t *records)
{
    return zs_split_records(src, srcSize, delim, targetSize, maxFrameSize, frameSizes, firstRecord, capacity, records);
}
// the tiles of a stream and the size staging both device calls lay over them: counts [tiles], last ends [tiles]; (8-aligned) the records
// in front of each tile [tiles + 1], the sum of the extra cuts.  Reserved here, with the scan's tile sums for `scanned` items
struct SplitTiles { uint32_t tiles; uint32_t *dCounts, *dLastEnd; uint64_t *dTileBase; unsigned long long *dExtraTotal; };
static int splitTiles(zsmi_ctx *c, uint64_t srcSize, uint64_t scanned, SplitTiles &t)
{
    const uint64_t tiles64 = (srcSize + ZS_SPLIT_TILE - 1) / ZS_SPLIT_TILE;
    if (tiles64 > 0x7FFFFFFFull) return ZSMI_error_memory_allocation;
    t.tiles = (uint32_t)tiles64;
    const size_t words = (2 * (size_t)t.tiles * sizeof(uint32_t) + 7) & ~(size_t)7;
    if (!c->sSizes.reserve(words + ((size_t)t.tiles + 2) * sizeof(uint64_t))) return ZSMI_error_memory_allocation;
    if (!c->dScan.reserve(sizeof(uint64_t) * (size_t)((std::max<uint64_t>(scanned, t.tiles) + ZS_SCAN_TILE - 1) / ZS_SCAN_TILE + 1))) return ZSMI_error_memory_allocation;
    t.dCounts = (uint32_t *)c->sSizes.p; t.dLastEnd = t.dCounts + t.tiles;
    t.dTileBase = (uint64_t *)((uint8_t *)c->sSizes.p + words); t.dExtraTotal = (unsigned long long *)(t.dTileBase + t.tiles + 1);
    return 0;
}
// the count kernel and the scan over its counts: t.dTileBase[t.tiles] is `records` (no tile: the scan writes the 0)
static int splitCount(zsmi_ctx *c, const void *dSrc, uint64_t srcSize, int delim, const SplitTiles &t)
{
    if (t.tiles) LAUNCH(c, "k_split_count", k_split_count, dim3(t.tiles), dim3(256), 0, (const uint8_t *)dSrc, srcSize, (uint32_t)delim, t.dCounts, t.dLastEnd);
    return scanOffsets(c, "k_split_scan", (const uint32_t *)t.dCounts, nullptr, t.tiles, 1u, nullptr, t.dTileBase);
}
extern "C" int zsmi_countRecordsDevice(zsmi_ctx *c, const void *dSrc, uint64_t srcSize, int delim, uint64_t *dRecords)
{
    if (!c) return ZSMI_error_init_missing;
    if (const int e = zs_split_check(dSrc, srcSize, delim, 0, 1, 0)) return e;
    if (!dRecords) return ZSMI_error_GENERIC;
    if (const int e = c->bind()) return e;
    SplitTiles t;
    if (const int e = splitTiles(c, srcSize, 0, t)) return e;
    if (const int e = splitCount(c, dSrc, srcSize, delim, t)) return e;
    if (const int e = c->onDevice(dRecords, t.dTileBase + t.tiles, sizeof(uint64_t))) return e;
    return c->launched();
}
extern "C" int zsmi_splitRecordsDevice(zsmi_ctx *c, const void *dSrc, uint64_t srcSize, int delim, uint32_t targetSize, uint32_t maxFrameSize,
                                       uint32_t maxPieces, uint32_t *dFrameSizes, uint64_t *dFirstRecord, uint64_t *dResult)
{
    if (!c) return ZSMI_error_init_missing;
    if (const int e = zs_split_check(dSrc, srcSize, delim, targetSize, maxFrameSize, maxPieces)) return e;
    if (!dResult || (maxPieces && !dFrameSizes)) return ZSMI_error_GENERIC;
    if (const int e = c->bind()) return e;
    const size_t m = maxPieces;
    SplitTiles t;
    if (const int e = splitTiles(c, srcSize, m, t)) return e;
    // device words, 64 bits: record ends [m], piece ends [m], the extra cuts in front of each record and later the slots [m + 1]; 32 bits:
    // successors, the two jump arrays (the first: the extra cuts), marks [m each]
    if (!c->seek.dMeta.reserve((3 * m + 1) * sizeof(uint64_t) + 4 * m * sizeof(uint32_t))) return ZSMI_error_memory_allocation;
    uint64_t *dE = (uint64_t *)c->seek.dMeta.p, *dPE = dE + m, *dX = dPE + m, *dSlot = dX;
    uint32_t *dNext = (uint32_t *)(dX + m + 1), *dJump[2] = { dNext + m, dNext + 2 * m }, *dMark = dNext + 3 * m, *dExtra = dJump[0];
    const uint64_t *dRecords = t.dTileBase + t.tiles;
    const uint32_t grid = (uint32_t)((m + 255) / 256);
    if (const int e = splitCount(c, dSrc, srcSize, delim, t)) return e;
    if (const int e = c->fill(t.dExtraTotal, 0, sizeof(uint64_t))) return e;
    if (m) if (const int e = c->fill(dExtra, 0, m * sizeof(uint32_t))) return e;      // (the records behind `records` have no cuts)
    if (t.tiles)
        LAUNCH(c, "k_split_emit", k_split_emit, dim3(t.tiles), dim3(256), 0, (const uint8_t *)dSrc, srcSize, (uint32_t)delim, (const uint64_t *)t.dTileBase,
               (const uint32_t *)t.dLastEnd, maxFrameSize, dE, dExtra, maxPieces, t.dExtraTotal);
    if (const int e = scanOffsets(c, "k_split_scan", (const uint32_t *)dExtra, nullptr, maxPieces, 1u, nullptr, dX)) return e;
    if (m) {
        LAUNCH(c, "k_split_pieces", k_split_pieces, dim3(grid), dim3(256), 0, (const uint64_t *)dE, (const uint64_t *)dX, dRecords,
               (const unsigned long long *)t.dExtraTotal, maxFrameSize, maxPieces, dPE);
        LAUNCH(c, "k_split_succ", k_split_succ, dim3(grid), dim3(256), 0, (const uint64_t *)dPE, dRecords, (const unsigned long long *)t.dExtraTotal, targetSize,
               maxPieces, dNext, dMark);
        const uint32_t *jump = dNext;
        for (uint32_t round = 0; targetSize && (1ull << round) < (uint64_t)m + 1; round++) {
            LAUNCH(c, "k_index_jump", k_index_jump, dim3(grid), dim3(256), 0, jump, dJump[round & 1u], dMark, maxPieces);
            jump = dJump[round & 1u];
        }
    }
    if (const int e = scanOffsets(c, "k_split_scan", (const uint32_t *)dMark, nullptr, maxPieces, 1u, nullptr, dSlot)) return e;
    LAUNCH(c, "k_split_table", k_split_table, dim3(std::max(grid, 1u)), dim3(256), 0, (const uint64_t *)dE, (const uint64_t *)dPE, (const uint32_t *)dNext,
           (const uint32_t *)dMark, (const uint64_t *)dSlot, dRecords, (const unsigned long long *)t.dExtraTotal, maxPieces, dFrameSizes, dFirstRecord, dResult);
    return c->launched();
}
