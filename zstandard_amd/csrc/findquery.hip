// findquery.hip -- find records by several patterns (zsmi_findquery.h states the rule; zsmi_findRecordsQuery runs it serially on the
// host): text in device memory, or a window of frames of a record archive, and a query of up to 8 literal patterns, a mode (any, all, none)
// and the ASCII case-folding flag -> the ascending numbers of the records whose hit set satisfies the mode, and the hit sets, in device
// memory.  The device calls only queue work.  find.hip is the family's base: this file calls its tile loads, its emit head and tail,
// zs_find_open, its shared-memory layout (ZsFindShared), its scratch layout and scans and, on an archive, its checks, window sequence and
// staging; the tile analysis, the count kernel and the carry kernel are its own.
//
// What differs from find.hip is WHERE a record is decided: at its END, by the lane that owns its delimiter, not at its first occurrence -
// `none` lists records without any occurrence, `all` needs the whole record's set.  The state that crosses a border is the 8-bit SET of
// the patterns that occur behind the last delimiter in front of it, not one bit: behind a segment it is TAILSET | (no delimiter ? the set
// in front : 0), which composes as find.hip's bit does, a bit of the set at a time.  So the same three levels serve: lanes by K pairs of
// ballots (zs_find_open), the 16 (step, wavefront) pairs through LDS, the tiles by a one-workgroup carry kernel.
//
// The launch sequence over text[0, size), a workgroup a 16 KiB tile (256 threads x 16 bytes x 4 steps):
//   k_findq_count   a lane's 16 bytes are folded in registers (a SWAR range test a word) and stored FOLDED to LDS with a halo of (longest
//                   pattern - 1) folded bytes; the delimiter mask comes from the UNFOLDED registers.  The patterns arrive folded by the
//                   host.  A pattern at a time: candidates by the zero-byte test on its first two bytes, verified in LDS; a byte of set
//                   a position (16 bytes a step) says which patterns occur there.  Per tile: delimiters, occurrences, keptLocal - the
//                   record ends whose set satisfies the mode as if nothing came in front of the tile - and a flags word: has a delimiter,
//                   the text's last byte is no delimiter (last tile), HEADSET (the patterns that occur in front of the first delimiter),
//                   TAILSET (those behind the last)
//   k_findq_carry   ONE workgroup, ZS_FINDQ_CARRY_ROUND tiles a round: the set entering every tile; kept[t] += listed(carry | HEADSET) -
//                   listed(HEADSET) for the tile's first record end (+1 for any and all, -1 for none); the last tile gains the text's
//                   unterminated last record where its set - TAILSET | (no delimiter ? carry : 0) - is listed
//   scanOffsets x 3 over the delimiters (a tile's record base), over kept (a tile's output slot) and over the occurrences (matches)
//   k_findq_emit    tiles that list a record only (kept[t] != 0, read off the scan): the masks again with the carried set in front: every listed record end with a slot below capacity writes B + the
//                   tile's base + the delimiters in front of it inside the tile, and its set where dHits is given; the last tile's first
//                   lane writes the unterminated last record.  One lane writes dResult.
// Scratch: find.hip's 40 bytes a tile in the seekable scratch.  Every store is a vector store from plain C++.

#include "zsmi_status.h"
#include "zsmi_wave.h"            // wave_incl_scan, wave_sum, wave_min
#include "zsmi_ctx.h"             // the context, LAUNCH, scanOffsets
#include "zsmi_findquery.h"       // the rule: zs_findq_check, zs_findq_records, zs_findq_listed
#include <algorithm>
// From the feature files zsmi_api.hip includes in front of this one: split.hip - ZS_SPLIT_TILE, ZsSplitBytes16; records.hip -
// zs_rec_mask16; find.hip - ZsFindShared, zs_find_load, zs_find_open, zs_find_pop4, zs_find_emit_head, zs_find_emit_tail, zs_find_emit_open,
// FindTiles, findReserve, findScans, findCheck, FindDecoded, findWindow, FindStaged, findStage; seekable.hip - zsmi_seekableFindWorkBound.

// the query, by value in the kernels' arguments: pattern j is b[at[j], at[j] + m[j]), folded where the flag is set
struct ZsFindQuery { uint32_t K, mode, fold, longest; uint16_t m[ZSMI_FIND_MAX_PATTERNS], at[ZSMI_FIND_MAX_PATTERNS]; uint8_t b[ZS_FIND_MAX_PATTERN]; };
// a tile's flags word: bits 8 .. 15 HEADSET, 16 .. 23 TAILSET, 24 .. 31 the set entering the tile (k_findq_carry)
static const uint32_t kFindqHasDelim = 1u, kFindqOpenEnd = 2u;

// ---- kernels ----
// rule 1 on four bytes: 0x20 added to every byte in 'A' .. 'Z' (bit 7 of a 7-bit sum says >= 'A', > 'Z'; no carry leaves a byte)
__device__ __forceinline__ uint32_t zs_findq_fold4(uint32_t w)
{
    const uint32_t low = w & 0x7F7F7F7Fu, geA = low + 0x3F3F3F3Fu, gtZ = low + 0x25252525u;
    return w | (((geA & ~gtZ & ~w) & 0x80808080u) >> 2);
}
// the OR of the set bytes of positions [from, to) of a step's 16 (lo: positions 0 .. 7, hi: 8 .. 15), 0 <= from <= to <= 16
__device__ __forceinline__ uint64_t zs_findq_below(uint32_t n) { return n >= 8u ? ~0ull : (1ull << (8u * n)) - 1ull; }
__device__ __forceinline__ uint32_t zs_findq_or(uint64_t lo, uint64_t hi, uint32_t from, uint32_t to)
{
    uint64_t x = (lo & zs_findq_below(to) & ~zs_findq_below(from)) | (hi & zs_findq_below(to > 8u ? to - 8u : 0u) & ~zs_findq_below(from > 8u ? from - 8u : 0u));
    x |= x >> 32; x |= x >> 16; x |= x >> 8;
    return (uint32_t)x & 0xFFu;
}
// the hit set of the record that ends at delimiter bit k of a lane's 16 bytes: dm their delimiters, in the set in front of them
__device__ __forceinline__ uint32_t zs_findq_set(uint64_t lo, uint64_t hi, uint32_t dm, uint32_t k, uint32_t in)
{
    const uint32_t before = dm & ((1u << k) - 1u);
    return before ? zs_findq_or(lo, hi, 32u - (uint32_t)__clz((int)before), k) : zs_findq_or(lo, hi, 0u, k) | in;
}
// The masks of tile `tile`: bit k of dm[s] / km[s] stands for the byte at tile * ZS_SPLIT_TILE + s * 4096 + 16 * threadIdx.x + k - it is
// the delimiter / the record that ends there is listed, given `carry` as the set in front of the tile; byte k of lo[s], hi[s] (k - 8) is
// the set of the patterns that occur at that byte; in[s]: the set in front of the lane's 16 bytes.  The loads are zs_find_load's; every
// halo goes byte by byte too - no byte at or behind src + size is read, is a delimiter or belongs to an occurrence.  out: the set behind
// the tile; occs: the lane's occurrences
struct ZsFindqMasks { uint64_t lo[4], hi[4]; uint32_t dm[4], km[4], in[4], out, occs; bool anyDelim; };
__device__ __forceinline__ void zs_findq_tile(const uint8_t *__restrict__ src, uint64_t size, uint32_t delim, const ZsFindQuery &Q, uint64_t tile, uint32_t carry,
                                              ZsFindShared &sh, ZsFindqMasks &k)
{
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u, K = Q.K;
    const uint64_t tileAt = tile * ZS_SPLIT_TILE;
    ZsSplitBytes16 own[4], low[4];
    const bool whole = zs_find_load(src, size, tile, own);
    #pragma unroll
    for (uint32_t s = 0; s < 4; s++) {
        #pragma unroll
        for (uint32_t w = 0; w < 4; w++) low[s].w[w] = Q.fold ? zs_findq_fold4(own[s].w[w]) : own[s].w[w];
        __builtin_memcpy(__builtin_assume_aligned(sh.text + s * 4096u + 16u * tid, 16), &low[s], 16);
    }
    sh.pat[tid] = Q.b[tid];                                                // (256 threads, ZS_FIND_MAX_PATTERN bytes)
    if (tid + 1u < Q.longest) {                                            // the halo: the longest pattern's m - 1 bytes behind the tile
        const uint64_t g = tileAt + ZS_SPLIT_TILE + tid;
        const uint8_t v = g < size ? src[g] : (uint8_t)0;
        sh.text[ZS_SPLIT_TILE + tid] = zs_findq_fold(v, Q.fold);
    }
    __syncthreads();
    const uint32_t delim4 = delim * 0x01010101u;
    const uint64_t below = (1ull << lane) - 1ull;
    uint32_t pre[4], occs = 0;                                             // pre: the set in front of the lane from the lanes of its wavefront, bit 8: one of them holds a delimiter
    #pragma unroll
    for (uint32_t s = 0; s < 4; s++) {
        uint32_t dm = zs_rec_mask16(own[s], delim4);
        if (!whole) {                                                      // (the zeros behind the text's end are no delimiters)
            const uint64_t at = tileAt + s * 4096u + 16u * tid, left = size > at ? size - at : 0ull;
            if (left < 16u) dm &= (1u << (uint32_t)left) - 1u;
        }
        k.dm[s] = dm; k.lo[s] = 0; k.hi[s] = 0;
    }
    for (uint32_t j = 0; j < K; j++) {                                     // a pattern at a time, its words read once for the four steps
        const uint32_t m = Q.m[j], p0 = Q.at[j], second = Q.b[p0 + (m > 1u ? 1u : 0u)], first4 = Q.b[p0] * 0x01010101u, second4 = second * 0x01010101u;
        #pragma unroll
        for (uint32_t s = 0; s < 4; s++) {
            const uint32_t b = s * 4096u + 16u * tid;                      // counted from the tile's start
            uint32_t cand = zs_rec_mask16(low[s], first4);
            if (m > 1u) {                                                  // the byte behind a candidate is the pattern's second (the 17th: the next lane's first, or the halo's)
                const uint32_t next = zs_rec_mask16(low[s], second4) | (sh.text[b + 16u] == second ? 1u << 16 : 0u);
                cand &= next >> 1;
            }
            for (uint32_t bits = cand; bits; bits &= bits - 1u) {          // at most m compares a position
                const uint32_t at = (uint32_t)__ffs((int)bits) - 1u, p = b + at;
                if (tileAt + p + m > size) break;                          // (the candidates ascend)
                uint32_t i = m > 1u ? 2u : 1u;
                while (i < m && sh.text[p + i] == sh.pat[p0 + i]) i++;
                if (i == m) {
                    const uint64_t bit = (uint64_t)(1u << j) << (8u * (at & 7u));
                    if (at < 8u) k.lo[s] |= bit; else k.hi[s] |= bit;
                    occs++;
                }
            }
        }
    }
    #pragma unroll
    for (uint32_t s = 0; s < 4; s++) {
        const uint32_t dm = k.dm[s], tail = zs_findq_or(k.lo[s], k.hi[s], dm ? 32u - (uint32_t)__clz((int)dm) : 0u, 16u);
        const uint64_t delims = __ballot(dm != 0u);
        uint32_t front = (delims & below) ? 0x100u : 0u, behind = 0;
        for (uint32_t j = 0; j < K; j++) {
            const uint64_t tails = __ballot((tail >> j) & 1u);
            if (!tails) continue;                                          // (the same for the whole wavefront)
            front |= zs_find_open(tails, delims, below, false) ? 1u << j : 0u;
            behind |= zs_find_open(tails, delims, ~0ull, false) ? 1u << j : 0u;
        }
        pre[s] = front;
        if (lane == 0) { sh.tail[s * 4u + wave] = behind; sh.delim[s * 4u + wave] = delims != 0ull; }
    }
    __syncthreads();
    uint32_t state = carry, in[4] = { 0, 0, 0, 0 };
    bool anyDelim = false;
    #pragma unroll
    for (uint32_t i = 0; i < 16; i++) {                                    // the (step, wavefront) pairs in text order
        if ((i & 3u) == wave) in[i >> 2] = state;
        const bool d = sh.delim[i] != 0u;
        state = sh.tail[i] | (d ? 0u : state);
        anyDelim |= d;
    }
    k.out = state; k.anyDelim = anyDelim; k.occs = occs;
    #pragma unroll
    for (uint32_t s = 0; s < 4; s++) {
        const uint32_t mine = (pre[s] & 0xFFu) | ((pre[s] & 0x100u) ? 0u : in[s]);
        uint32_t km = 0;
        for (uint32_t bits = k.dm[s]; bits; bits &= bits - 1u) {
            const uint32_t at = (uint32_t)__ffs((int)bits) - 1u;
            if (zs_findq_listed(zs_findq_set(k.lo[s], k.hi[s], k.dm[s], at, mine), Q.mode, K)) km |= 1u << at;
        }
        k.in[s] = mine; k.km[s] = km;
    }
}
// delims[tile], occs[tile], kept[tile] (keptLocal: k_findq_carry corrects it), flags[tile]
__global__ void __launch_bounds__(256)
k_findq_count(const uint8_t *__restrict__ src, uint64_t size, uint32_t delim, const ZsFindQuery Q, uint32_t tiles, uint32_t *__restrict__ delims,
              uint32_t *__restrict__ occs, uint32_t *__restrict__ kept, uint32_t *__restrict__ flags)
{
    __shared__ ZsFindShared sh;
    ZsFindqMasks k;
    zs_findq_tile(src, size, delim, Q, blockIdx.x, 0u, sh, k);
    uint32_t head = ~0u;                                                   // (the lane's first delimiter, from the tile's start) << 8 | the set of the record it ends
    #pragma unroll
    for (uint32_t s = 0; s < 4; s++)
        if (k.dm[s] && head == ~0u) {
            const uint32_t at = (uint32_t)__ffs((int)k.dm[s]) - 1u;
            head = ((s * 4096u + 16u * threadIdx.x + at) << 8) | zs_findq_set(k.lo[s], k.hi[s], k.dm[s], at, k.in[s]);
        }
    const uint32_t nd = wave_sum(zs_find_pop4(k.dm)), no = wave_sum(k.occs), nk = wave_sum(zs_find_pop4(k.km));
    head = wave_min(head);
    const uint32_t wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 0) { sh.sums[wave][0] = nd; sh.sums[wave][1] = no; sh.sums[wave][2] = nk; sh.sums[wave][3] = head; }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t sum[3] = { 0, 0, 0 }, first = ~0u;
        for (uint32_t w = 0; w < 4; w++) { sum[0] += sh.sums[w][0]; sum[1] += sh.sums[w][1]; sum[2] += sh.sums[w][2]; first = min(first, sh.sums[w][3]); }
        delims[blockIdx.x] = sum[0]; occs[blockIdx.x] = sum[1]; kept[blockIdx.x] = sum[2];
        const uint32_t headSet = k.anyDelim ? first & 0xFFu : k.out;       // (no delimiter: every occurrence of the tile is in front of the first)
        const bool open = blockIdx.x + 1u == tiles && src[size - 1u] != (uint8_t)delim;
        flags[blockIdx.x] = (k.anyDelim ? kFindqHasDelim : 0u) | (open ? kFindqOpenEnd : 0u) | (headSet << 8) | (k.out << 16);
    }
}
// one workgroup of 1024: the set entering every tile, ZS_FINDQ_CARRY_ROUND tiles a round - a lane takes four tiles in a row, composes their
// steps into one segment for the ballots and walks them again from the set the ballots give it (1 GiB is 16 rounds)
#define ZS_FINDQ_CARRY_ROUND 4096u
__global__ void __launch_bounds__(1024)
k_findq_carry(uint32_t *__restrict__ flags, uint32_t *__restrict__ kept, uint32_t tiles, uint32_t K, uint32_t mode)
{
    __shared__ uint32_t tail[16], delim[16];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint64_t below = (1ull << lane) - 1ull;
    uint32_t state = 0;                                                    // the set in front of the round's first tile
    for (uint32_t t0 = 0; t0 < tiles; t0 += ZS_FINDQ_CARRY_ROUND) {
        const uint32_t t = t0 + 4u * threadIdx.x;                          // (tiles <= 0x7FFFFFFF: no wrap)
        uint32_t f[4];
        #pragma unroll
        for (uint32_t j = 0; j < 4; j++) f[j] = t + j < tiles ? flags[t + j] : 0u;      // (a tile behind the last: no delimiter, no set - it passes the state on)
        uint32_t segTail = 0;
        bool segDelim = false;
        #pragma unroll
        for (uint32_t j = 0; j < 4; j++) {
            const bool d = (f[j] & kFindqHasDelim) != 0u;
            segTail = ((f[j] >> 16) & 0xFFu) | (d ? 0u : segTail); segDelim |= d;
        }
        const uint64_t delims = __ballot(segDelim);
        uint32_t front = 0, behind = 0;
        for (uint32_t b = 0; b < K; b++) {                                 // (zs_findq_tile's composition, without its skip of a pattern no lane holds: DESIGN.md, "Find records")
            const uint64_t tails = __ballot((segTail >> b) & 1u);
            front |= zs_find_open(tails, delims, below, false) ? 1u << b : 0u;
            behind |= zs_find_open(tails, delims, ~0ull, false) ? 1u << b : 0u;
        }
        if (lane == 0) { tail[wave] = behind; delim[wave] = delims != 0ull; }
        __syncthreads();
        uint32_t in = 0;
        #pragma unroll
        for (uint32_t w = 0; w < 16; w++) {
            if (w == wave) in = state;
            state = tail[w] | (delim[w] ? 0u : state);
        }
        uint32_t carry = front | ((delims & below) ? 0u : in);
        #pragma unroll
        for (uint32_t j = 0; j < 4; j++) {
            const bool d = (f[j] & kFindqHasDelim) != 0u;
            const uint32_t headSet = (f[j] >> 8) & 0xFFu, behindTile = ((f[j] >> 16) & 0xFFu) | (d ? 0u : carry);
            if (t + j < tiles) {
                uint32_t add = 0;                                          // (modulo 2^32: -1 where a listed first record end is no longer)
                if (d) add = (uint32_t)zs_findq_listed(carry | headSet, mode, K) - (uint32_t)zs_findq_listed(headSet, mode, K);
                if ((f[j] & kFindqOpenEnd) && zs_findq_listed(behindTile, mode, K)) add += 1u;      // (set on the last tile only)
                if (carry) flags[t + j] = f[j] | (carry << 24);
                if (add) kept[t + j] += add;
            }
            carry = behindTile;
        }
        __syncthreads();                                                   // (the next round writes tail and delim again)
    }
}
// The masks again, the carried set in front.  recBase[tile]: the delimiters in front of the tile (recBase[tiles]: all); slotBase[tile]:
// the listed records in front of it (slotBase[tiles]: total); occBase[tiles]: matches.  A step's record ends follow the steps before it, a
// wavefront's the wavefronts before it, a lane's the lanes before it.  base: one device word, or null for 0.  hits: null - not wanted.
// code: null, or the window's code - not 0: nothing is written and dResult states it.  The grid is max(tiles, 1)
__global__ void __launch_bounds__(256)
k_findq_emit(const uint8_t *__restrict__ src, uint64_t size, uint32_t delim, const ZsFindQuery Q, uint32_t tiles, const uint32_t *__restrict__ flags,
             const uint64_t *__restrict__ recBase, const uint64_t *__restrict__ slotBase, const uint64_t *__restrict__ occBase, const uint64_t *__restrict__ base,
             const uint32_t *__restrict__ code, uint64_t *__restrict__ records, uint8_t *__restrict__ hits, uint64_t capacity, uint64_t *__restrict__ result)
{
    __shared__ ZsFindShared sh;
    uint64_t slot0;
    if (!zs_find_emit_head(code, slotBase, tiles, capacity, size, [&] { return occBase[tiles]; }, true, result, slot0)) return;
    ZsFindqMasks k;
    zs_findq_tile(src, size, delim, Q, blockIdx.x, flags[blockIdx.x] >> 24, sh, k);
    const uint64_t first = (base ? *base : 0ull) + recBase[blockIdx.x];
    const ZsFindEmitted n = zs_find_emit_tail(k.dm, k.km, slot0, first, capacity, records, [&](uint64_t slot, uint32_t s, uint32_t at) {
        if (hits) hits[slot] = (uint8_t)zs_findq_set(k.lo[s], k.hi[s], k.dm[s], at, k.in[s]);
    });
    if (blockIdx.x + 1u == tiles && threadIdx.x == 0 && src[size - 1u] != (uint8_t)delim && zs_findq_listed(k.out, Q.mode, Q.K))
        zs_find_emit_open(slot0 + n.kept, first + n.delims, capacity, records, [&](uint64_t slot) { if (hits) hits[slot] = (uint8_t)k.out; });
}

// ---- host ----
extern "C" size_t zsmi_findRecordsQuery(const void *src, size_t srcSize, int delim, const zsmi_findQuery *q, uint64_t base,
                                        uint64_t *records, uint8_t *hits, size_t capacity, uint64_t *matches)
{
    if (!q || (capacity && !records)) return ZSMI_ERR(ZSMI_error_GENERIC);
    if (const int e = zs_findq_check(delim, q)) return ZSMI_ERR(e);
    if (srcSize && !src) return ZSMI_ERR(ZSMI_error_srcSize_wrong);
    return (size_t)zs_findq_records((const uint8_t *)src, srcSize, (uint8_t)delim, q, base, records, hits, capacity, matches);
}
// a checked query as the kernels take it: the patterns end to end, folded once here
static ZsFindQuery findQuery(const zsmi_findQuery *q)
{
    ZsFindQuery Q;
    memset(&Q, 0, sizeof Q);
    Q.K = q->nPatterns; Q.mode = q->mode; Q.fold = q->flags & ZSMI_FIND_IGNORE_CASE;
    uint32_t at = 0;
    for (uint32_t j = 0; j < Q.K; j++) {
        const uint32_t m = q->patternSizes[j];
        Q.m[j] = (uint16_t)m; Q.at[j] = (uint16_t)at; Q.longest = std::max(Q.longest, m);
        for (uint32_t i = 0; i < m; i++) Q.b[at + i] = zs_findq_fold(((const uint8_t *)q->patterns[j])[i], q->flags);
        at += m;
    }
    return Q;
}
static uint32_t findQueryShortest(const zsmi_findQuery *q)
{
    uint32_t m = q->patternSizes[0];
    for (uint32_t j = 1; j < q->nPatterns; j++) m = std::min(m, q->patternSizes[j]);
    return m;
}
// the launch sequence over dText[0, size), its arguments checked and its scratch reserved by the caller
static int findqText(zsmi_ctx *c, const void *dText, uint64_t size, int delim, const ZsFindQuery &Q, const uint64_t *dBase, const uint32_t *dCode,
                     uint64_t *dRecords, uint8_t *dHits, uint64_t capacity, uint64_t *dResult, const FindTiles &t)
{
    if (t.tiles) {
        LAUNCH(c, "k_findq_count", k_findq_count, dim3(t.tiles), dim3(256), 0, (const uint8_t *)dText, size, (uint32_t)delim, Q, t.tiles, t.dDelims, t.dOccs, t.dKept, t.dFlags);
        LAUNCH(c, "k_findq_carry", k_findq_carry, dim3(1), dim3(1024), 0, t.dFlags, t.dKept, t.tiles, Q.K, Q.mode);
    }
    if (const int e = findScans(c, t, true)) return e;
    LAUNCH(c, "k_findq_emit", k_findq_emit, dim3(std::max(t.tiles, 1u)), dim3(256), 0, (const uint8_t *)dText, size, (uint32_t)delim, Q, t.tiles, (const uint32_t *)t.dFlags,
           (const uint64_t *)t.dRecBase, (const uint64_t *)t.dSlotBase, (const uint64_t *)t.dOccBase, dBase, dCode, dRecords, dHits, capacity, dResult);
    return c->launched();
}
extern "C" int zsmi_findRecordsQueryDevice(zsmi_ctx *c, const void *dSrc, uint64_t srcSize, int delim, const zsmi_findQuery *q,
                                           const uint64_t *dBase, uint64_t *dRecords, uint8_t *dHits, uint64_t capacity, uint64_t *dResult)
{
    if (!c) return ZSMI_error_init_missing;
    if (!dResult || !q || (capacity && !dRecords)) return ZSMI_error_GENERIC;
    if (const int e = zs_findq_check(delim, q)) return e;
    if (srcSize && !dSrc) return ZSMI_error_srcSize_wrong;
    if (const int e = c->bind()) return e;
    if (srcSize == 0) return c->fill(dResult, 0, 4 * sizeof(uint64_t));
    FindTiles t;
    if (const int e = findReserve(c, srcSize, 0, 0, t)) return e;
    return findqText(c, dSrc, srcSize, delim, findQuery(q), dBase, nullptr, dRecords, dHits, capacity, dResult, t);
}
extern "C" int zsmi_seekableFindQueryResident(zsmi_ctx *c, const zsmi_seekable *sk, const uint64_t *dFirstRecord, uint32_t nFrames, int delim,
                                              const zsmi_findQuery *q, uint32_t firstFrame, uint32_t frameCount, void *dWork, uint64_t workCapacity,
                                              uint64_t *dRecords, uint8_t *dHits, uint64_t capacity, uint64_t *dResult)
{
    if (const int e = findCheck(c, sk, dFirstRecord, nFrames, q, [&] { return zs_findq_check(delim, q); }, firstFrame, frameCount, false, dWork, workCapacity, dRecords,
                                capacity, dResult)) return e;
    return findWindow(c, sk, firstFrame, frameCount, dWork, dResult, 0, [&](const FindDecoded &w, const FindTiles &t) {
        return findqText(c, dWork, w.bytes, delim, findQuery(q), dFirstRecord + firstFrame, w.dCode, dRecords, dHits, capacity, dResult, t);
    });
}
// host arrays in and out (find.hip's findStage).  A record that holds an occurrence holds the shortest pattern's bytes of its own, so any
// and all name at most bytes / that many records; a `none` query can name a record a byte.  The staged numbers are that, or capacity,
// and a byte of set each behind them
extern "C" int zsmi_seekableFindQueryHost(zsmi_ctx *c, const zsmi_seekable *sk, const uint64_t *firstRecord, uint32_t nFrames, int delim,
                                          const zsmi_findQuery *q, uint32_t firstFrame, uint32_t frameCount,
                                          uint64_t *records, uint8_t *hits, size_t capacity, uint64_t *result)
{
    if (const int e = findCheck(c, sk, firstRecord, nFrames, q, [&] { return zs_findq_check(delim, q); }, firstFrame, frameCount, true, nullptr, 0, records, capacity, result))
        return e;
    const uint64_t bytes = zsmi_seekableFindWorkBound(sk, firstFrame, frameCount);
    const size_t room = (size_t)std::min<uint64_t>(capacity, q->mode == ZSMI_find_none ? bytes : bytes / findQueryShortest(q));
    return findStage(c, firstRecord, nFrames, bytes, room, true, 0, 0, records, hits, result, [&](const FindStaged &s) {
        return zsmi_seekableFindQueryResident(c, sk, s.dFirst, nFrames, delim, q, firstFrame, frameCount, s.dWork, bytes, s.dRecords, s.dHits, room, s.dResult);
    });
}
