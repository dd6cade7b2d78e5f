// find.hip -- find records by content (zsmi_find.h states the rule; zsmi_findRecords runs it serially on the host): the step that selects
// records.  Text in device memory, or a window of frames of a record archive, and a literal pattern -> the ascending numbers of the records
// that hold the pattern, in device memory, as zsmi_seekableReadRecordsResident takes them.  The device calls only queue work.
//
// The launch sequence over text[0, size), a workgroup a 16 KiB tile (the splitter's shape: 256 threads x 16 bytes x 4 steps):
//   k_find_count    the tile and a halo of m - 1 bytes behind it staged in LDS; a bit a byte: the byte is the delimiter (dm), an
//                   occurrence starts at the byte (om: the zero-byte test on the pattern's first two bytes finds candidates, each is
//                   compared with the pattern in LDS).  Per tile: delimiters, occurrences, keptLocal - the occurrences that are the first
//                   of their record as if nothing came in front of the tile - and three flags: the tile holds a delimiter, an occurrence
//                   starts behind its last delimiter (TAIL: the record that leaves the tile holds one), one starts in front of its first
//                   delimiter (HEAD HIT)
//   k_find_carry    ONE workgroup, 4096 tiles a round: CARRY[t] - the record tile t starts in already holds an occurrence.  That is "the
//                   largest occurrence start in front of the tile lies behind the largest delimiter position in front of it"; the tiles'
//                   flags say as much without the positions: walking back from t, a tile with TAIL is met before (or is) the first tile
//                   with a delimiter.  The state behind a tile is TAIL | (no delimiter & the state in front): such steps compose, so a
//                   wavefront resolves 256 tiles (four a lane) from two ballots, the workgroup's 16 wavefronts are chained through LDS, the rounds through
//                   a register.  kept[t] = keptLocal[t] - (HEAD HIT[t] & CARRY[t])
//   scanOffsets x 3 over the delimiters (a tile's record base), over kept (a tile's output slot) and over the occurrences (matches)
//   k_find_emit     the masks again, with CARRY as the state in front of the tile: every kept occurrence with a slot below capacity writes
//                   B + the tile's base + the delimiters in front of it inside the tile.  One lane writes dResult.
// The same three-level chain - lanes by ballots, (step, wavefront) pairs through LDS, tiles by k_find_carry - decides inside a tile which
// occurrence is the first of its record (zs_find_open).
// On an archive (zsmi_seekableFindRecordsResident) the window's frames are first decoded end to end into dWork by seekable.hip's
// frame-list decode on the list firstFrame, firstFrame + 1 ..: k_find_frames, k_seek_request_sizes, then scanOffsets, k_seek_request_items,
// decodeItems, k_seek_verify; k_find_code brings the frames' codes down to the first failing frame's, which k_find_emit honours.
// Scratch, all of it context buffers reserved before anything is queued: 16 bytes a tile and three scans of 8 bytes a tile in the seekable
// scratch, 60 bytes a frame of the window there too, the decoder's item list and scratch.  Every store is a vector store from plain C++.
// This file is the base of the search family (findquery.hip, findregex.hip, findframes.hip): what does not depend on the search rule is
// defined here once and called there - on the device the tile's loads (zs_find_load), the emit kernels' head and tail (zs_find_emit_head,
// zs_find_emit_tail, zs_find_emit_open) and zs_find_open; on the host the tiles' layout (FindTiles, findTileBytes, findLay, findReserve), the
// three scans (findScans), the archive calls' checks (findCheck), the decode half of a window (findDecodeReserve, findDecode), the window
// sequence (findWindow) and the host forms' staging (findStage).  The tile analyses, the count kernels and the carry kernels are each
// search's own: what crosses a border there is a bit, a set, a state function.

#include "zsmi_status.h"
#include "zsmi_wave.h"            // wave_incl_scan, wave_sum, wave_min
#include "zsmi_ctx.h"             // the context, LAUNCH, scanOffsets, decodeItems
#include "zsmi_find.h"            // the rule: zs_find_check, zs_find_records
#include <algorithm>
// From the feature files zsmi_api.hip includes in front of this one (none can be included twice): split.hip - ZS_SPLIT_TILE, ZsSplitBytes16,
// zs_split_word_mask; records.hip - zs_rec_mask16, the 16-bit mask of a lane's 16 bytes; seekable.hip - the handle, ZsSeekEntry,
// k_seek_request_sizes, the frame-list decode (SeekListWords, seekListHead, seekListWords, seekDecodeList), seekWindowCheck,
// zsmi_seekableFindWorkBound.  (zs_split_tile_masks itself is not used: it marks the stream's last byte as
// a record end whatever it is, and here only delimiters count; and the bytes are wanted, not only their mask.)

struct ZsFindPattern { uint32_t m; uint8_t b[ZS_FIND_MAX_PATTERN]; };    // the pattern, by value in the kernels' arguments
static const uint32_t kFindHasDelim = 1u, kFindTail = 2u, kFindHeadHit = 4u, kFindCarry = 8u;      // a tile's flags

// ---- kernels ----
struct ZsFindShared {
    __attribute__((aligned(16))) uint8_t text[ZS_SPLIT_TILE + ZS_FIND_MAX_PATTERN];      // the tile and its halo
    uint8_t pat[ZS_FIND_MAX_PATTERN];
    uint32_t tail[16], delim[16];                                         // the summaries of the (step, wavefront) pairs, in text order
    uint32_t sums[4][8];                                                   // a kernel's own reductions, a row a wavefront
};
// The state in front of lane `lane` of 64 segments in a row.  A segment's summary: delims - it holds a delimiter; tail - an occurrence
// starts behind its last delimiter (anywhere, when it holds none).  The state behind a segment = tail | (no delimiter & the state in
// front).  below: the lanes in front (all 64: the state behind the last lane)
__device__ __forceinline__ bool zs_find_open(uint64_t tail, uint64_t delims, uint64_t below, bool in)
{
    const uint64_t d = delims & below;
    if (!d) return in || (tail & below) != 0;
    const uint32_t j = 63u - (uint32_t)__clzll((long long)d);             // the last segment in front that holds a delimiter
    return (tail & below & ~((1ull << j) - 1ull)) != 0;
}
// the occurrences of om that are the first of their record: dm the delimiters of the same 16 bytes, open the state in front of them
__device__ __forceinline__ uint32_t zs_find_kept(uint32_t om, uint32_t dm, bool open)
{
    uint32_t kept = 0, done = 0;                                          // done: the bits up to the occurrence before
    for (uint32_t bits = om; bits; bits &= bits - 1u) {
        const uint32_t k = (uint32_t)__ffs((int)bits) - 1u, below = (1u << k) - 1u;
        if (dm & below & ~done) open = false;
        if (!open) kept |= 1u << k;
        open = true; done = below | (1u << k);
    }
    return kept;
}
// A tile's loads, the same in the three searches (find.hip, findquery.hip, findregex.hip): lane i loads the 16 bytes at the tile's start +
// s * 4096 + 16 i - a wavefront's loads one contiguous KiB, the four steps' issued together; the text's last tile, unless it is a whole
// one, goes byte by byte: no byte at or behind src + size is read, own holds zeros there.  Returns `whole`
__device__ __forceinline__ bool zs_find_load(const uint8_t *__restrict__ src, uint64_t size, uint64_t tile, ZsSplitBytes16 (&own)[4])
{
    const uint64_t tileAt = tile * ZS_SPLIT_TILE, base = tileAt + 16u * threadIdx.x;
    const bool whole = size - tileAt >= ZS_SPLIT_TILE;
    if (whole) {
        #pragma unroll
        for (uint32_t s = 0; s < 4; s++) __builtin_memcpy(&own[s], src + base + s * 4096u, 16);
    } else {
        for (uint32_t s = 0; s < 4; s++) {
            const uint64_t b = base + s * 4096u;
            for (uint32_t w = 0; w < 4; w++) {
                uint32_t v = 0;
                for (uint32_t j = 0; j < 4; j++) if (b + 4u * w + j < size) v |= (uint32_t)src[b + 4u * w + j] << (8u * j);
                own[s].w[w] = v;
            }
        }
    }
    return whole;
}
// The masks of tile `tile`: bit k of dm[s] / om[s] / km[s] stands for the byte at tile * ZS_SPLIT_TILE + s * 4096 + 16 * threadIdx.x + k -
// it is the delimiter / an occurrence starts there / that occurrence is the first of its record, given `carry` as the state in front of
// the tile.  The loads are zs_find_load's; every halo goes byte by byte too: no byte at or behind src + size is read (LDS holds zeros
// there, and an occurrence must END at or in front of size).  out: the state behind the tile; anyDelim: the tile holds a delimiter.
struct ZsFindMasks { uint32_t dm[4], om[4], km[4]; bool out, anyDelim; };
__device__ __forceinline__ void zs_find_tile(const uint8_t *__restrict__ src, uint64_t size, uint32_t delim, const ZsFindPattern &P, uint64_t tile, bool carry,
                                             ZsFindShared &sh, ZsFindMasks &k)
{
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u, m = P.m;
    const uint64_t tileAt = tile * ZS_SPLIT_TILE;
    ZsSplitBytes16 own[4];
    zs_find_load(src, size, tile, own);
    #pragma unroll
    for (uint32_t s = 0; s < 4; s++) __builtin_memcpy(__builtin_assume_aligned(sh.text + s * 4096u + 16u * tid, 16), &own[s], 16);
    if (tid < m) sh.pat[tid] = P.b[tid];
    if (tid + 1u < m) {                                                    // the halo: the m - 1 bytes behind the tile
        const uint64_t g = tileAt + ZS_SPLIT_TILE + tid;
        sh.text[ZS_SPLIT_TILE + tid] = g < size ? src[g] : (uint8_t)0;
    }
    __syncthreads();
    const uint32_t delim4 = delim * 0x01010101u, first4 = P.b[0] * 0x01010101u, second4 = P.b[m > 1u ? 1u : 0u] * 0x01010101u;
    uint64_t tails[4], delims[4];
    #pragma unroll
    for (uint32_t s = 0; s < 4; s++) {
        const uint32_t b = s * 4096u + 16u * tid;                          // counted from the tile's start
        const uint32_t dm = zs_rec_mask16(own[s], delim4);
        uint32_t cand = zs_rec_mask16(own[s], first4);
        if (m > 1u) {                                                      // the byte behind a candidate is the pattern's second (the 17th: the next lane's first, or the halo's)
            const uint32_t next = zs_rec_mask16(own[s], second4) | (sh.text[b + 16u] == P.b[1] ? 1u << 16 : 0u);
            cand &= next >> 1;
        }
        uint32_t om = 0;
        for (uint32_t bits = cand; bits; bits &= bits - 1u) {              // at most m compares a position
            const uint32_t at = (uint32_t)__ffs((int)bits) - 1u, p = b + at;
            if (tileAt + p + m > size) break;                              // (the candidates ascend)
            uint32_t i = m > 1u ? 2u : 1u;
            while (i < m && sh.text[p + i] == sh.pat[i]) i++;
            if (i == m) om |= 1u << at;
        }
        k.dm[s] = dm; k.om[s] = om;
        const bool segTail = dm ? (om >> (32u - (uint32_t)__clz((int)dm))) != 0u : om != 0u;
        tails[s] = __ballot(segTail); delims[s] = __ballot(dm != 0u);
        if (lane == 0) { sh.tail[s * 4u + wave] = zs_find_open(tails[s], delims[s], ~0ull, false); sh.delim[s * 4u + wave] = delims[s] != 0ull; }
    }
    __syncthreads();
    bool state = carry, anyDelim = false, in[4] = { false, false, false, false };
    #pragma unroll
    for (uint32_t i = 0; i < 16; i++) {                                    // the (step, wavefront) pairs in text order
        if ((i & 3u) == wave) in[i >> 2] = state;
        const bool d = sh.delim[i] != 0u;
        state = sh.tail[i] != 0u || (!d && state);
        anyDelim |= d;
    }
    k.out = state; k.anyDelim = anyDelim;
    #pragma unroll
    for (uint32_t s = 0; s < 4; s++) k.km[s] = zs_find_kept(k.om[s], k.dm[s], zs_find_open(tails[s], delims[s], (1ull << lane) - 1ull, in[s]));
}
// the first set bit of a tile's masks, counted from the tile's start; ~0 for none
__device__ __forceinline__ uint32_t zs_find_first(const uint32_t mask[4])
{
    uint32_t f = ~0u;
    #pragma unroll
    for (uint32_t s = 0; s < 4; s++) if (mask[s]) f = min(f, s * 4096u + 16u * threadIdx.x + (uint32_t)__ffs((int)mask[s]) - 1u);
    return f;
}
__device__ __forceinline__ uint32_t zs_find_pop4(const uint32_t mask[4]) { return (uint32_t)(__popc(mask[0]) + __popc(mask[1]) + __popc(mask[2]) + __popc(mask[3])); }
// delims[tile], occs[tile], kept[tile] (keptLocal: k_find_carry corrects it), flags[tile]
__global__ void __launch_bounds__(256)
k_find_count(const uint8_t *__restrict__ src, uint64_t size, uint32_t delim, const ZsFindPattern P, uint32_t *__restrict__ delims, uint32_t *__restrict__ occs,
             uint32_t *__restrict__ kept, uint32_t *__restrict__ flags)
{
    __shared__ ZsFindShared sh;
    ZsFindMasks k;
    zs_find_tile(src, size, delim, P, blockIdx.x, false, sh, k);
    const uint32_t nd = wave_sum(zs_find_pop4(k.dm)), no = wave_sum(zs_find_pop4(k.om)), nk = wave_sum(zs_find_pop4(k.km));
    const uint32_t firstDelim = wave_min(zs_find_first(k.dm)), firstOcc = wave_min(zs_find_first(k.om));
    const uint32_t wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 0) { sh.sums[wave][0] = nd; sh.sums[wave][1] = no; sh.sums[wave][2] = nk; sh.sums[wave][3] = firstDelim; sh.sums[wave][4] = firstOcc; }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t sum[3] = { 0, 0, 0 }, fd = ~0u, fo = ~0u;
        for (uint32_t w = 0; w < 4; w++) { sum[0] += sh.sums[w][0]; sum[1] += sh.sums[w][1]; sum[2] += sh.sums[w][2]; fd = min(fd, sh.sums[w][3]); fo = min(fo, sh.sums[w][4]); }
        delims[blockIdx.x] = sum[0]; occs[blockIdx.x] = sum[1]; kept[blockIdx.x] = sum[2];
        flags[blockIdx.x] = (k.anyDelim ? kFindHasDelim : 0u) | (k.out ? kFindTail : 0u) | (fo < fd ? kFindHeadHit : 0u);      // (fo < fd: some occurrence, in front of every delimiter)
    }
}
// one workgroup of 1024: the carry into every tile, 4096 tiles a round - a lane takes four tiles in a row, composes their steps into one
// segment for the ballots and walks them again from the state the ballots give it (1 GiB is 16 rounds)
#define ZS_FIND_CARRY_ROUND 4096u
__global__ void __launch_bounds__(1024)
k_find_carry(uint32_t *__restrict__ flags, uint32_t *__restrict__ kept, uint32_t tiles)
{
    __shared__ uint32_t tail[16], delim[16];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    bool state = false;                                                    // the state in front of the round's first tile
    for (uint32_t t0 = 0; t0 < tiles; t0 += ZS_FIND_CARRY_ROUND) {
        const uint32_t t = t0 + 4u * threadIdx.x;                          // (tiles <= 0x7FFFFFFF: no wrap)
        uint32_t f[4];
        #pragma unroll
        for (uint32_t j = 0; j < 4; j++) f[j] = t + j < tiles ? flags[t + j] : 0u;      // (a tile behind the last: neither bit, it passes the state on)
        bool segTail = false, segDelim = false;
        #pragma unroll
        for (uint32_t j = 0; j < 4; j++) {
            const bool d = (f[j] & kFindHasDelim) != 0u;
            segTail = (f[j] & kFindTail) != 0u || (!d && segTail); segDelim |= d;
        }
        const uint64_t tails = __ballot(segTail), delims = __ballot(segDelim);
        if (lane == 0) { tail[wave] = zs_find_open(tails, delims, ~0ull, false); delim[wave] = delims != 0ull; }
        __syncthreads();
        bool in = false;
        #pragma unroll
        for (uint32_t w = 0; w < 16; w++) {
            if (w == wave) in = state;
            state = tail[w] != 0u || (!delim[w] && state);
        }
        bool carry = zs_find_open(tails, delims, (1ull << lane) - 1ull, in);
        #pragma unroll
        for (uint32_t j = 0; j < 4; j++) {
            if (t + j < tiles && carry) { flags[t + j] = f[j] | kFindCarry; if (f[j] & kFindHeadHit) kept[t + j] -= 1u; }
            carry = (f[j] & kFindTail) != 0u || (!(f[j] & kFindHasDelim) && carry);
        }
        __syncthreads();                                                   // (the next round writes tail and delim again)
    }
}
// the first failing frame's code, in frame order, of the window's n > 0 frames: one workgroup, eight loads a lane in flight
__global__ void __launch_bounds__(1024)
k_find_code(const uint32_t *__restrict__ codes, uint32_t n, uint32_t *__restrict__ code)
{
    __shared__ uint32_t firsts[16];
    uint32_t first = ~0u;
    for (uint32_t i0 = threadIdx.x; i0 < n && first == ~0u; i0 += 8192u) {  // (n <= 2^27 frames: no wrap)
        uint32_t v[8];
        #pragma unroll
        for (uint32_t j = 0; j < 8; j++) { const uint32_t i = i0 + 1024u * j; v[j] = i < n ? codes[i] : 0u; }
        #pragma unroll
        for (uint32_t j = 0; j < 8; j++) if (v[j] && first == ~0u) first = i0 + 1024u * j;
    }
    first = wave_min(first);
    if ((threadIdx.x & 63u) == 0) firsts[threadIdx.x >> 6] = first;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (uint32_t w = 1; w < 16; w++) first = min(first, firsts[w]);
        *code = first == ~0u ? 0u : codes[first];
    }
}
// the window's frame list: list[j] = firstFrame + j
__global__ void __launch_bounds__(256)
k_find_frames(uint32_t firstFrame, uint32_t n, uint32_t *__restrict__ list)
{
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j < n) list[j] = firstFrame + j;
}
// ---- what the three emit kernels (k_find_emit, k_findq_emit, k_findre_emit) share ----
// The head: the first lane of the first workgroup writes dResult - code: null, or the window's code; not 0: no number is written and
// dResult states it; third(): dResult[2], the caller's, asked for by that one lane alone (every workgroup would else load its
// words).  Returns whether this workgroup has anything to write, and slot0, its tile's first
// slot: none when the window failed, behind the last tile, at or above capacity (the slots ascend with the tiles; capacity 0: nothing to
// write) and, with skipEmpty, in a tile that lists nothing - most tiles of a rare pattern - which is then not read again.  (k_find_emit
// passes false: DESIGN.md, "Find records".)  The same for the whole workgroup
template <class Third>
__device__ __forceinline__ bool zs_find_emit_head(const uint32_t *__restrict__ code, const uint64_t *__restrict__ slotBase, uint32_t tiles, uint64_t capacity, uint64_t size,
                                                  Third third, bool skipEmpty, uint64_t *__restrict__ result, uint64_t &slot0)
{
    const uint32_t failed = code ? *code : 0u;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const uint64_t total = slotBase[tiles];
        result[0] = failed ? 0ull - (uint64_t)failed : total;
        result[1] = failed ? 0ull : (total < capacity ? total : capacity);
        result[2] = failed ? 0ull : third();
        result[3] = size;
    }
    if (failed || blockIdx.x >= tiles) return false;
    slot0 = slotBase[blockIdx.x];
    return slot0 < capacity && !(skipEmpty && slotBase[blockIdx.x + 1u] == slot0);
}
// The tail: bit k of km[s] is a number to write, bit k of dm[s] a delimiter, for the byte at the tile's start + s * 4096 + 16 *
// threadIdx.x + k.  A step's numbers follow the steps before it, a wavefront's the wavefronts before it, a lane's the lanes before it:
// ranks by wave_incl_scan, the wavefronts' totals through LDS.  The number is first - the tile's first record: the caller's base +
// recBase[tile] - + the delimiters in front of the bit inside the tile; every one with a slot below capacity is written, and
// each(slot, s, at) called for it.  Returns the tile's totals: its numbers and its delimiters
struct ZsFindEmitted { uint32_t kept, delims; };
template <class Each>
__device__ __forceinline__ ZsFindEmitted zs_find_emit_tail(const uint32_t (&dm)[4], const uint32_t (&km)[4], uint64_t slot0, uint64_t first,
                                                           uint64_t capacity, uint64_t *__restrict__ records, Each each)
{
    __shared__ uint32_t keptOf[4][4], delimsOf[4][4];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    uint32_t keptBefore[4], delimsBefore[4];
    #pragma unroll
    for (uint32_t s = 0; s < 4; s++) {
        const uint32_t nk = (uint32_t)__popc(km[s]), nd = (uint32_t)__popc(dm[s]), inclK = wave_incl_scan(nk), inclD = wave_incl_scan(nd);
        keptBefore[s] = inclK - nk; delimsBefore[s] = inclD - nd;
        if (lane == 63u) { keptOf[s][wave] = inclK; delimsOf[s][wave] = inclD; }
    }
    __syncthreads();
    uint32_t keptAt = 0, delimsAt = 0;                                     // those of the steps in front
    #pragma unroll
    for (uint32_t s = 0; s < 4; s++) {
        uint32_t aheadK = 0, aheadD = 0, allK = 0, allD = 0;
        #pragma unroll
        for (uint32_t w = 0; w < 4; w++) {
            aheadK += w < wave ? keptOf[s][w] : 0u; allK += keptOf[s][w];
            aheadD += w < wave ? delimsOf[s][w] : 0u; allD += delimsOf[s][w];
        }
        uint64_t slot = slot0 + keptAt + aheadK + keptBefore[s];
        const uint64_t rec = first + delimsAt + aheadD + delimsBefore[s];
        for (uint32_t bits = km[s]; bits; bits &= bits - 1u, slot++) {
            const uint32_t at = (uint32_t)__ffs((int)bits) - 1u;
            if (slot < capacity) { records[slot] = rec + (uint32_t)__popc(dm[s] & ((1u << at) - 1u)); each(slot, s, at); }
        }
        keptAt += allK; delimsAt += allD;
    }
    return { keptAt, delimsAt };
}
// the text's unterminated last record, where it is listed (the last tile's first lane decides): slot and rec lie behind every number
// and every delimiter of the last tile
template <class Each>
__device__ __forceinline__ void zs_find_emit_open(uint64_t slot, uint64_t rec, uint64_t capacity, uint64_t *__restrict__ records, Each each)
{
    if (slot < capacity) { records[slot] = rec; each(slot); }
}
// The masks again, the tile's carry in front.  recBase[tile]: the delimiters in front of the tile; slotBase[tile]: the kept occurrences in
// front of it (slotBase[tiles]: total); occBase[tiles]: matches.  A step's occurrences follow the steps before it, a wavefront's the
// wavefronts before it, a lane's the lanes before it.  base: one device word, or null for 0.  code: null, or the window's code - not 0:
// no number is written and dResult states it.  The grid is max(tiles, 1): the first lane writes dResult whatever `tiles` is.
__global__ void __launch_bounds__(256)
k_find_emit(const uint8_t *__restrict__ src, uint64_t size, uint32_t delim, const ZsFindPattern P, uint32_t tiles, const uint32_t *__restrict__ flags,
            const uint64_t *__restrict__ recBase, const uint64_t *__restrict__ slotBase, const uint64_t *__restrict__ occBase, const uint64_t *__restrict__ base,
            const uint32_t *__restrict__ code, uint64_t *__restrict__ records, uint64_t capacity, uint64_t *__restrict__ result)
{
    __shared__ ZsFindShared sh;
    uint64_t slot0;
    if (!zs_find_emit_head(code, slotBase, tiles, capacity, size, [&] { return occBase[tiles]; }, false, result, slot0)) return;
    ZsFindMasks k;
    zs_find_tile(src, size, delim, P, blockIdx.x, (flags[blockIdx.x] & kFindCarry) != 0u, sh, k);
    zs_find_emit_tail(k.dm, k.km, slot0, (base ? *base : 0ull) + recBase[blockIdx.x], capacity, records, [](uint64_t, uint32_t, uint32_t) {});
}

// ---- host ----
extern "C" size_t zsmi_findRecords(const void *src, size_t srcSize, int delim, const void *pattern, uint32_t patternSize, uint64_t base,
                                   uint64_t *records, size_t capacity, uint64_t *matches)
{
    if (!pattern || (capacity && !records)) return ZSMI_ERR(ZSMI_error_GENERIC);
    if (const int e = zs_find_check(delim, pattern, patternSize)) return ZSMI_ERR(e);
    if (srcSize && !src) return ZSMI_ERR(ZSMI_error_srcSize_wrong);
    return (size_t)zs_find_records((const uint8_t *)src, srcSize, (uint8_t)delim, (const uint8_t *)pattern, patternSize, base, records, capacity, matches);
}
// the tiles of a text and what the calls lay over them in the seekable scratch, `head` bytes into it (8-aligned): the three scans
// [tiles + 1 each]; delimiters, occurrences, kept, flags [tiles each]; behind them, 16-aligned, extraPerTile bytes a tile of the search's
// own (dExtra; findregex.hip's 72) - findTileBytes: all of them.  findReserve: that, and the scans' tile sums for `scanned` items at
// least - before anything is queued
struct FindTiles { uint32_t tiles; uint32_t *dDelims, *dOccs, *dKept, *dFlags; uint64_t *dRecBase, *dSlotBase, *dOccBase; uint8_t *dExtra; };
static size_t findTileBytes(size_t tiles, size_t extraPerTile = 0) { return 3 * (tiles + 1) * sizeof(uint64_t) + 4 * tiles * sizeof(uint32_t) + (extraPerTile ? 16 + tiles * extraPerTile : 0); }
static int findTilesOf(uint64_t size, FindTiles &t)
{
    const uint64_t tiles64 = (size + ZS_SPLIT_TILE - 1) / ZS_SPLIT_TILE;
    if (tiles64 > 0x7FFFFFFFull) return ZSMI_error_memory_allocation;
    t.tiles = (uint32_t)tiles64;
    return 0;
}
static void findLay(void *meta, size_t head, size_t extraPerTile, FindTiles &t)
{
    const size_t n = t.tiles, words = head + findTileBytes(n);
    t.dRecBase = (uint64_t *)((uint8_t *)meta + head); t.dSlotBase = t.dRecBase + n + 1; t.dOccBase = t.dSlotBase + n + 1;
    t.dDelims = (uint32_t *)(t.dOccBase + n + 1); t.dOccs = t.dDelims + n; t.dKept = t.dOccs + n; t.dFlags = t.dKept + n;
    t.dExtra = extraPerTile ? (uint8_t *)meta + (words + 15) / 16 * 16 : nullptr;
}
static int findReserve(zsmi_ctx *c, uint64_t size, size_t head, uint64_t scanned, FindTiles &t, size_t extraPerTile = 0)
{
    if (const int e = findTilesOf(size, t)) return e;
    if (!c->seek.dMeta.reserve(head + findTileBytes(t.tiles, extraPerTile))) return ZSMI_error_memory_allocation;
    if (!c->dScan.reserve(sizeof(uint64_t) * (size_t)((std::max<uint64_t>(scanned, t.tiles) + ZS_SCAN_TILE - 1) / ZS_SCAN_TILE + 1))) return ZSMI_error_memory_allocation;
    findLay(c->seek.dMeta.p, head, extraPerTile, t);
    return 0;
}
static ZsFindPattern findPattern(const void *pattern, uint32_t m)
{
    ZsFindPattern P;
    memset(&P, 0, sizeof P);
    P.m = m; memcpy(P.b, pattern, m);
    return P;
}
// the scans behind a search's count and carry kernels: over the delimiters (a tile's record base), over kept (a tile's output slot) and,
// where the search counts them, over the occurrences (matches)
static int findScans(zsmi_ctx *c, const FindTiles &t, bool occs)
{
    if (const int e = scanOffsets(c, "k_find_scan", (const uint32_t *)t.dDelims, nullptr, t.tiles, 1u, nullptr, t.dRecBase)) return e;
    if (const int e = scanOffsets(c, "k_find_scan", (const uint32_t *)t.dKept, nullptr, t.tiles, 1u, nullptr, t.dSlotBase)) return e;
    return occs ? scanOffsets(c, "k_find_scan", (const uint32_t *)t.dOccs, nullptr, t.tiles, 1u, nullptr, t.dOccBase) : 0;
}
// the launch sequence over dText[0, size), its arguments checked and its scratch reserved by the caller
static int findText(zsmi_ctx *c, const void *dText, uint64_t size, int delim, const ZsFindPattern &P, const uint64_t *dBase, const uint32_t *dCode,
                    uint64_t *dRecords, uint64_t capacity, uint64_t *dResult, const FindTiles &t)
{
    if (t.tiles) {
        LAUNCH(c, "k_find_count", k_find_count, dim3(t.tiles), dim3(256), 0, (const uint8_t *)dText, size, (uint32_t)delim, P, t.dDelims, t.dOccs, t.dKept, t.dFlags);
        LAUNCH(c, "k_find_carry", k_find_carry, dim3(1), dim3(1024), 0, t.dFlags, t.dKept, t.tiles);
    }
    if (const int e = findScans(c, t, true)) return e;
    LAUNCH(c, "k_find_emit", k_find_emit, dim3(std::max(t.tiles, 1u)), dim3(256), 0, (const uint8_t *)dText, size, (uint32_t)delim, P, t.tiles, (const uint32_t *)t.dFlags,
           (const uint64_t *)t.dRecBase, (const uint64_t *)t.dSlotBase, (const uint64_t *)t.dOccBase, dBase, dCode, dRecords, capacity, dResult);
    return c->launched();
}
extern "C" int zsmi_findRecordsDevice(zsmi_ctx *c, const void *dSrc, uint64_t srcSize, int delim, const void *pattern, uint32_t patternSize,
                                      const uint64_t *dBase, uint64_t *dRecords, uint64_t capacity, uint64_t *dResult)
{
    if (!c) return ZSMI_error_init_missing;
    if (!dResult || !pattern || (capacity && !dRecords)) return ZSMI_error_GENERIC;
    if (const int e = zs_find_check(delim, pattern, patternSize)) return e;
    if (srcSize && !dSrc) return ZSMI_error_srcSize_wrong;
    if (const int e = c->bind()) return e;
    if (srcSize == 0) return c->fill(dResult, 0, 4 * sizeof(uint64_t));
    FindTiles t;
    if (const int e = findReserve(c, srcSize, 0, 0, t)) return e;
    return findText(c, dSrc, srcSize, delim, findPattern(pattern, patternSize), dBase, nullptr, dRecords, capacity, dResult, t);
}
// the header's checks of the archive calls, in its order - seekable.hip's seekWindowCheck with the search's arrays; rule: the pattern,
// query or program, and ruleCheck its check (zs_find_check, zs_findq_check, zs_regex_check), in front of the caller's frame count; work:
// null for the host form, which brings its own buffer
template <class RuleCheck>
static int findCheck(const zsmi_ctx *c, const zsmi_seekable *sk, const void *firstRecord, uint32_t nFrames, const void *rule, RuleCheck ruleCheck,
                     uint32_t firstFrame, uint32_t frameCount, bool ownWork, const void *work, uint64_t workCapacity, const void *records, uint64_t capacity, const void *result)
{
    return seekWindowCheck(c, sk, !result || !rule || !firstRecord || (capacity && !records), [&] {
        const int e = ruleCheck();
        return e ? e : (nFrames != sk->t.n ? (int)ZSMI_error_parameter_outOfBound : 0);
    }, firstFrame, frameCount, ownWork, work, workCapacity);
}
// The decode half of every call on a window of an archive - the three searches, the record index, the frame filter: the window's frames
// into dWork, end to end, verified (seekable.hip's frame-list decode on the list firstFrame, firstFrame + 1 ..), and the first failing
// frame's code in a device word.  In the seekable scratch the list's words (seekListHead) and, behind them, `behind` bytes of the
// caller's own - a search's tiles, the index's; findDecodeReserve: that, the decoder's item list and the scans' tile sums for F items or
// `scanned`, whichever is more.  A call of many windows reserves for the largest before it queues the first
struct FindDecoded { uint64_t bytes; void *dBehind; const uint32_t *dCode; const uint64_t *dListAt; };      // dListAt: the frames' places in dWork [frameCount + 1]
static int findDecodeReserve(zsmi_ctx *c, uint32_t F, size_t behind, uint64_t scanned)
{
    return c->seek.dMeta.reserve(seekListHead(F) + behind) && c->dItems.reserve(sizeof(ZsDecItem) * (size_t)F) &&
           c->dScan.reserve(sizeof(uint64_t) * (size_t)((std::max<uint64_t>(scanned, F) + ZS_SCAN_TILE - 1) / ZS_SCAN_TILE + 1)) ? 0 : ZSMI_error_memory_allocation;
}
// (context bound, frameCount > 0, arguments checked by the caller)
static int findDecode(zsmi_ctx *c, const zsmi_seekable *sk, uint32_t firstFrame, uint32_t frameCount, void *dWork, size_t behind, uint64_t scanned, FindDecoded &w)
{
    if (const int e = findDecodeReserve(c, frameCount, behind, scanned)) return e;
    const SeekListWords d = seekListWords(c->seek.dMeta.p, frameCount);
    const uint32_t grid = (frameCount + 255) / 256;
    w.bytes = zsmi_seekableFindWorkBound(sk, firstFrame, frameCount); w.dBehind = (uint8_t *)c->seek.dMeta.p + seekListHead(frameCount); w.dCode = d.dCode; w.dListAt = d.dListAt;
    LAUNCH(c, "k_find_frames", k_find_frames, dim3(grid), dim3(256), 0, firstFrame, frameCount, d.dList);
    LAUNCH(c, "k_seek_request_sizes", k_seek_request_sizes, dim3(grid), dim3(256), 0, (const ZsSeekEntry *)sk->dTable.p, sk->t.n, (const uint32_t *)d.dList, frameCount, d.dSizes);
    if (const int e = seekDecodeList(c, sk, d.dList, frameCount, d, "k_find_scan", 1u, dWork, w.bytes)) return e;
    LAUNCH(c, "k_find_code", k_find_code, dim3(1), dim3(1024), 0, (const uint32_t *)d.dCodes, frameCount, d.dCode);
    return 0;
}
// the launch sequence of a search on a window of an archive, its arguments checked by the caller: the decode half with the search's tiles
// behind its words - extraPerTile: findReserve's -, then text(w, t) - the search's sequence over the decoded text (findText, findqText,
// findreText)
template <class Text>
static int findWindow(zsmi_ctx *c, const zsmi_seekable *sk, uint32_t firstFrame, uint32_t frameCount, void *dWork, uint64_t *dResult, size_t extraPerTile, Text text)
{
    if (const int e = c->bind()) return e;
    if (frameCount == 0) return c->fill(dResult, 0, 4 * sizeof(uint64_t));
    FindTiles t;
    if (const int e = findTilesOf(zsmi_seekableFindWorkBound(sk, firstFrame, frameCount), t)) return e;
    FindDecoded w;
    if (const int e = findDecode(c, sk, firstFrame, frameCount, dWork, findTileBytes(t.tiles, extraPerTile), t.tiles, w)) return e;
    findLay(c->seek.dMeta.p, seekListHead(frameCount), extraPerTile, t);
    return text(w, t);
}
// The host forms of the archive calls: host arrays in and out around a resident run, one wait.  Staged in device memory: firstRecord
// [nFrames + 1], `front` 64-bit words and, behind the four result words, `back` bytes of the caller's own (the list search's count and
// list), a work buffer of workBytes; the numbers [room] and, for a search with hit sets, a byte of set each behind them.  firstRecord goes
// up, run(s) uploads what else it staged and queues the resident sequence, the result words and the staged numbers (and sets, where
// hits is given) come down behind one wait, and what was written is handed over.  No exception leaves: this runs inside extern "C"
struct FindStaged { uint64_t *dFirst, *dFront, *dResult; uint8_t *dBack; void *dWork; uint64_t *dRecords; uint8_t *dHits; };      // dRecords, dHits: null where nothing is wanted
template <class Run>
static int findStage(zsmi_ctx *c, const uint64_t *firstRecord, uint32_t nFrames, uint64_t workBytes, size_t room, bool sets, size_t front, size_t back,
                     uint64_t *records, uint8_t *hits, uint64_t *result, Run run)
{
    if (const int e = c->bind()) return e;
    const size_t words = (size_t)nFrames + 1 + front + 4;
    if (!c->sSizes.reserve(words * sizeof(uint64_t) + back) || !c->sDst.reserve(room * (sizeof(uint64_t) + (sets ? 1 : 0)) + 64) || !c->seek.dDec.reserve(workBytes + 64))
        return ZSMI_error_memory_allocation;
    uint64_t *dRecords = (uint64_t *)c->sDst.p;
    uint8_t *dHits = (uint8_t *)(dRecords + room);
    FindStaged s;
    s.dFirst = (uint64_t *)c->sSizes.p; s.dFront = s.dFirst + nFrames + 1; s.dResult = s.dFront + front; s.dBack = (uint8_t *)(s.dResult + 4); s.dWork = c->seek.dDec.p;
    s.dRecords = room ? dRecords : nullptr; s.dHits = room && hits ? dHits : nullptr;
    int rc = c->toDevice(s.dFirst, firstRecord, ((size_t)nFrames + 1) * sizeof(uint64_t));
    if (!rc) rc = run(s);
    std::vector<uint64_t> numbers;
    std::vector<uint8_t> hitSets;
    if (!rc) { try { numbers.resize(room); if (hits) hitSets.resize(room); } catch (const std::bad_alloc &) { rc = ZSMI_error_memory_allocation; } }
    if (!rc) rc = c->toHost(result, s.dResult, 4 * sizeof(uint64_t));
    if (!rc && room) rc = c->toHost(numbers.data(), dRecords, room * sizeof(uint64_t));
    if (!rc && room && hits) rc = c->toHost(hitSets.data(), dHits, room);
    const int waited = c->wait();                                                  // (whatever was queued, a failed call included)
    if (rc || waited) return rc ? rc : waited;
    if (result[1] && result[1] <= room) {
        memcpy(records, numbers.data(), (size_t)result[1] * sizeof(uint64_t));
        if (hits) memcpy(hits, hitSets.data(), (size_t)result[1]);
    }
    return 0;
}
extern "C" int zsmi_seekableFindRecordsResident(zsmi_ctx *c, const zsmi_seekable *sk, const uint64_t *dFirstRecord, uint32_t nFrames, int delim,
                                                const void *pattern, uint32_t patternSize, uint32_t firstFrame, uint32_t frameCount,
                                                void *dWork, uint64_t workCapacity, uint64_t *dRecords, uint64_t capacity, uint64_t *dResult)
{
    if (const int e = findCheck(c, sk, dFirstRecord, nFrames, pattern, [&] { return zs_find_check(delim, pattern, patternSize); }, firstFrame, frameCount, false, dWork,
                                workCapacity, dRecords, capacity, dResult)) return e;
    return findWindow(c, sk, firstFrame, frameCount, dWork, dResult, 0, [&](const FindDecoded &w, const FindTiles &t) {
        return findText(c, dWork, w.bytes, delim, findPattern(pattern, patternSize), dFirstRecord + firstFrame, w.dCode, dRecords, capacity, dResult, t);
    });
}
// host arrays in and out (findStage).  A record that holds an occurrence holds m bytes of its own, so the window's bytes / m numbers are
// all there can be: the staging of the numbers is that, or capacity
extern "C" int zsmi_seekableFindRecordsHost(zsmi_ctx *c, const zsmi_seekable *sk, const uint64_t *firstRecord, uint32_t nFrames, int delim,
                                            const void *pattern, uint32_t patternSize, uint32_t firstFrame, uint32_t frameCount,
                                            uint64_t *records, size_t capacity, uint64_t *result)
{
    if (const int e = findCheck(c, sk, firstRecord, nFrames, pattern, [&] { return zs_find_check(delim, pattern, patternSize); }, firstFrame, frameCount, true, nullptr, 0,
                                records, capacity, result)) return e;
    const uint64_t bytes = zsmi_seekableFindWorkBound(sk, firstFrame, frameCount);
    const size_t room = (size_t)std::min<uint64_t>(capacity, bytes / patternSize);
    return findStage(c, firstRecord, nFrames, bytes, room, false, 0, 0, records, nullptr, result, [&](const FindStaged &s) {
        return zsmi_seekableFindRecordsResident(c, sk, s.dFirst, nFrames, delim, pattern, patternSize, firstFrame, frameCount, s.dWork, bytes, s.dRecords, room, s.dResult);
    });
}
