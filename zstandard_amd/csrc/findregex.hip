// findregex.hip -- find records by regular expression (zsmi_regex.h states the rule and holds the compiler; zsmi_findRecordsRegex runs the
// rule serially on the host): text in device memory, or a window of frames of a record archive, and a program - the minimal DFA of a
// pattern, compiled on the host - -> the ascending numbers of the records the program accepts (or, inverted, of the others), in device
// memory.  The device calls only queue work.  find.hip is the family's base: this file calls its tile loads, its emit head and tail, its
// scratch layout - with the extra region a tile this search needs - and scans and, on an archive, its checks, window sequence and staging;
// the tile analysis, the count kernel and the carry kernel are its own.
//
// A record is decided at its END, by the lane that owns its delimiter, as in findquery.hip.  What crosses a border is a state FUNCTION
// where the query search carries an 8-bit set: behind a stretch of text the state is hasDelimiter ? TAILSTATE : F(in) - F the stretch's
// transition function, nStates bytes; TAILSTATE the state reached from `start` over the bytes behind the stretch's last delimiter.  Such
// steps compose, so the same three levels serve: lanes, the 16 (step, wavefront) pairs, the tiles.
//
// The launch sequence over text[0, size), a workgroup a 16 KiB tile (256 threads x 16 bytes x 4 steps); the program travels by value in
// the kernels' arguments (3352 bytes) and its tables go to LDS once a workgroup, in the program's own layout:
//   k_findre_count  a step at a time: (a) LANES AS POSITIONS - a lane maps its 16 bytes to classes, walks them up to its first delimiter
//                   from EVERY state, four independent chains at a time, and leaves that function in LDS (fn[state][lane]: a state's row
//                   is written by consecutive lanes, rows 65 dwords apart); behind its last delimiter it walks from `start` alone (tail).  (b) LANES AS STATES -
//                   lane s of a wavefront carries state s through the 64 lane functions, from the wavefront's last delimiter on where it
//                   has one: the wavefront's function; the four of a step compose into the tile's function (a register of lane s of the
//                   first wavefront) and give every wavefront its entry state, and one more walk over the lane functions gives every lane
//                   its own.  (c) LANES AS POSITIONS again - from its entry state a lane re-walks its 16 bytes and decides each record end.
//                   Per tile: the delimiters; keptLocal, as if `start` entered the tile; a flags word: has a delimiter, the open last
//                   record (last tile); HEADMASK, 64 bits: the entry states for which the tile's first record end is listed; the tile's
//                   OUT function, 64 bytes (constant where the tile has a delimiter)
//   k_findre_carry  ONE workgroup of 16 wavefronts, ZS_FINDRE_CARRY_ROUND tiles a round, their OUT functions in LDS: a wavefront takes 32
//                   tiles in a row, lanes as states, from its last tile with a delimiter on - a text WITHOUT delimiters costs 32 + 16 + 32
//                   dependent LDS reads a round, not a step a tile; the state entering every tile goes into its flags word; kept[t] +=
//                   HEADMASK bit of the carry - HEADMASK bit of `start`; the last tile gains the text's unterminated last record
//   scanOffsets x 2 over the delimiters (a tile's record base) and over kept (a tile's output slot)
//   k_findre_emit   k_findq_emit's shape: tiles that list a record below capacity only; the masks again from the carried state; ranks by
//                   wave_incl_scan; one lane writes dResult - [2] is the delimiter total plus the open end
// Scratch: find.hip's 40 bytes a tile in the seekable scratch and, behind them, 72 more - findReserve's extra region: OUT functions [64 a
// tile], HEADMASKs [8 a tile].
// Every store is a vector store from plain C++.

#include "zsmi_status.h"
#include "zsmi_wave.h"            // wave_incl_scan, wave_sum
#include "zsmi_ctx.h"             // the context, LAUNCH, scanOffsets
#include "zsmi_regex.h"           // the rule: zs_regex_check, zs_regex_records, zs_regex_listed; the compiler
#include <algorithm>
// From the feature files zsmi_api.hip includes in front of this one: split.hip - ZS_SPLIT_TILE, ZsSplitBytes16; records.hip -
// zs_rec_mask16; find.hip - zs_find_load, zs_find_pop4, zs_find_emit_head, zs_find_emit_tail, zs_find_emit_open, FindTiles, findReserve,
// findScans, findCheck, FindDecoded, findWindow, FindStaged, findStage; seekable.hip - zsmi_seekableFindWorkBound.

static const uint32_t kFindreHasDelim = 1u, kFindreOpenEnd = 2u;          // a tile's flags word; bits 8 .. 15: the state entering the tile (k_findre_carry)

// ---- kernels ----
// A state's row of lane functions is 256 bytes and a pad dword.  Lanes as states read fn[x * stride + thread] with ONE thread and a state x
// a lane: byte reads bank by (address / 4) mod 32, so rows 64 dwords apart would put every state on one bank (up to 32 distinct addresses
// a half wavefront); 65 dwords apart, state x reads bank (x + thread / 4) mod 32 - 32 states or fewer never collide, above that x and
// x + 32 do (2-way at the worst); lanes that hold the same state read the same address
#define ZS_FINDRE_FN_STRIDE 260u
struct ZsFindreShared {
    uint8_t classOf[256];
    uint8_t next[ZSMI_REGEX_MAX_TABLE];
    uint8_t fn[ZSMI_REGEX_MAX_STATES * ZS_FINDRE_FN_STRIDE];               // a step's lane functions: fn[state * ZS_FINDRE_FN_STRIDE + thread]
    uint8_t tail[256];                                                     // a lane with a delimiter: the state behind it
    uint8_t waveFn[4][64];                                                 // a step's wavefront functions
    uint64_t waveDelims[4];                                                // a step's lanes that hold a delimiter, a wavefront
    uint32_t sums[4][2];
};
// The masks of tile `tile`: bit k of dm[s] / km[s] stands for the byte at tile * ZS_SPLIT_TILE + s * 4096 + 16 * threadIdx.x + k - it is
// the delimiter / the record that ends there is listed, given `entry` as the state in front of the tile.  The loads are zs_find_load's:
// no byte at or behind src + size is read, is a delimiter or is fed to the program.  out: the state behind the tile.  COUNT: besides, fnOut - the tile's
// function of state min(threadIdx.x, nStates - 1), valid in the first wavefront - and headMask, valid there too
struct ZsFindreMasks { uint32_t dm[4], km[4], out, fnOut; uint64_t headMask; bool anyDelim; };
template <bool COUNT>
__device__ __forceinline__ void zs_findre_tile(const uint8_t *__restrict__ src, uint64_t size, uint32_t delim, const zsmi_regexProgram &P, uint64_t tile, uint32_t entry,
                                               ZsFindreShared &sh, ZsFindreMasks &k)
{
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    const uint32_t n = P.nStates, nc = P.nClasses, start = P.start, invert = P.flags & ZSMI_REGEX_INVERT;
    const uint64_t accept = P.accept;
    const uint64_t tileAt = tile * ZS_SPLIT_TILE;
    ZsSplitBytes16 own[4];
    zs_find_load(src, size, tile, own);
    sh.classOf[tid] = P.classOf[tid];
    for (uint32_t i = tid; i < n * nc; i += 256u) sh.next[i] = P.next[i];
    __syncthreads();
    const uint32_t delim4 = delim * 0x01010101u, mine0 = min(lane, n - 1u);
    uint32_t cur = entry, g = mine0;                                       // cur: the state in front of the step (the same in every lane)
    uint64_t headMask = 0;
    bool anyDelim = false;
    #pragma unroll
    for (uint32_t s = 0; s < 4; s++) {
        const uint64_t at = tileAt + s * 4096u + 16u * tid, left = size > at ? size - at : 0ull;
        const uint32_t len = left < 16u ? (uint32_t)left : 16u;
        const uint32_t dm = zs_rec_mask16(own[s], delim4) & ((1u << len) - 1u);       // (the zeros behind the text's end are no delimiters)
        uint32_t cls[4];
        #pragma unroll
        for (uint32_t w = 0; w < 4; w++) {
            const uint32_t v = own[s].w[w];
            cls[w] = (uint32_t)sh.classOf[v & 0xFFu] | ((uint32_t)sh.classOf[(v >> 8) & 0xFFu] << 8) | ((uint32_t)sh.classOf[(v >> 16) & 0xFFu] << 16) |
                     ((uint32_t)sh.classOf[v >> 24] << 24);
        }
        // (a) the lane's function of its bytes in front of its first delimiter, and the state behind its last
        const uint32_t firstD = dm ? (uint32_t)__ffs((int)dm) - 1u : len;
        for (uint32_t s0 = 0; s0 < n; s0 += 4u) {
            uint32_t x[4];
            #pragma unroll
            for (uint32_t j = 0; j < 4; j++) x[j] = min(s0 + j, n - 1u);
            #pragma unroll
            for (uint32_t i = 0; i < 16; i++) {
                const uint32_t c = (cls[i >> 2] >> (8u * (i & 3u))) & 0xFFu;
                if (i < firstD) {
                    #pragma unroll
                    for (uint32_t j = 0; j < 4; j++) x[j] = sh.next[x[j] * nc + c];
                }
            }
            #pragma unroll
            for (uint32_t j = 0; j < 4; j++) sh.fn[min(s0 + j, n - 1u) * ZS_FINDRE_FN_STRIDE + tid] = (uint8_t)x[j];
        }
        if (dm) {
            const uint32_t lastD = 31u - (uint32_t)__clz((int)dm);
            uint32_t y = start;
            #pragma unroll
            for (uint32_t i = 1; i < 16; i++) {
                const uint32_t c = (cls[i >> 2] >> (8u * (i & 3u))) & 0xFFu;
                if (i > lastD && i < len) y = sh.next[y * nc + c];
            }
            sh.tail[tid] = (uint8_t)y;
        }
        const uint64_t delims = __ballot(dm != 0u);
        if (lane == 0) sh.waveDelims[wave] = delims;
        __syncthreads();
        // (b) lanes as states: the wavefront's function
        {
            uint32_t x = mine0, l = 0;
            if (delims) {                                                  // (the same for the whole wavefront: constant behind its last delimiter)
                const uint32_t j = 63u - (uint32_t)__clzll((long long)delims);
                x = sh.tail[wave * 64u + j]; l = j + 1u;
            }
            for (; l < 64u; l++) x = sh.fn[x * ZS_FINDRE_FN_STRIDE + wave * 64u + l];
            sh.waveFn[wave][lane] = (uint8_t)x;
        }
        __syncthreads();
        uint64_t d[4];
        #pragma unroll
        for (uint32_t w = 0; w < 4; w++) d[w] = sh.waveDelims[w];
        const bool stepDelim = (d[0] | d[1] | d[2] | d[3]) != 0ull;
        if (COUNT && !anyDelim && stepDelim && wave == 0) {                // the tile's first record end, from every entry state
            uint32_t x = g, w0 = 0;
            bool found = false;
            #pragma unroll
            for (uint32_t w = 0; w < 4; w++) {                             // through the wavefronts in front of the first that holds a delimiter
                if (!found && d[w]) { found = true; w0 = w; }
                if (!found) x = sh.waveFn[w][x];
            }
            const uint64_t dw = d[0] ? d[0] : d[1] ? d[1] : d[2] ? d[2] : d[3];
            const uint32_t l1 = (uint32_t)__ffsll((long long)dw) - 1u;
            for (uint32_t l = 0; l <= l1; l++) x = sh.fn[x * ZS_FINDRE_FN_STRIDE + w0 * 64u + l];
            headMask = __ballot(lane < n && zs_regex_listed(accept, invert, x));
        }
        uint32_t waveIn = cur;
        #pragma unroll
        for (uint32_t w = 0; w < 4; w++) {
            if (w == wave) waveIn = cur;
            cur = sh.waveFn[w][cur];
            if (COUNT) g = sh.waveFn[w][g];
        }
        anyDelim |= stepDelim;
        // the lane's entry state: the wavefront's, through the lanes in front
        uint32_t mine = waveIn;
        {
            uint32_t x = waveIn;
            for (uint32_t l = 0; l < 63u; l++) {
                x = ((delims >> l) & 1ull) ? sh.tail[wave * 64u + l] : sh.fn[x * ZS_FINDRE_FN_STRIDE + wave * 64u + l];
                if (l + 1u == lane) mine = x;
            }
        }
        // (c) the record ends of the lane's 16 bytes
        uint32_t km = 0, st = mine;
        #pragma unroll
        for (uint32_t i = 0; i < 16; i++) {
            const uint32_t c = (cls[i >> 2] >> (8u * (i & 3u))) & 0xFFu;
            if ((dm >> i) & 1u) {
                if (zs_regex_listed(accept, invert, st)) km |= 1u << i;
                st = start;
            } else if (i < len) st = sh.next[st * nc + c];
        }
        k.dm[s] = dm; k.km[s] = km;
        __syncthreads();                                                   // (the next step writes fn, tail and the wavefronts' words again)
    }
    k.out = cur; k.fnOut = g; k.headMask = headMask; k.anyDelim = anyDelim;
}
// delims[tile], kept[tile] (keptLocal: k_findre_carry corrects it), flags[tile], headMask[tile], outFn[tile * 64 + state]
__global__ void __launch_bounds__(256)
k_findre_count(const uint8_t *__restrict__ src, uint64_t size, uint32_t delim, const zsmi_regexProgram P, uint32_t tiles, uint32_t *__restrict__ delims,
               uint32_t *__restrict__ kept, uint32_t *__restrict__ flags, uint64_t *__restrict__ headMask, uint8_t *__restrict__ outFn)
{
    __shared__ ZsFindreShared sh;
    ZsFindreMasks k;
    zs_findre_tile<true>(src, size, delim, P, blockIdx.x, P.start, sh, k);
    const uint32_t nd = wave_sum(zs_find_pop4(k.dm)), nk = wave_sum(zs_find_pop4(k.km)), wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 0) { sh.sums[wave][0] = nd; sh.sums[wave][1] = nk; }
    __syncthreads();
    if (threadIdx.x < 64u) outFn[(uint64_t)blockIdx.x * 64u + threadIdx.x] = (uint8_t)k.fnOut;
    if (threadIdx.x == 0) {
        uint32_t sum[2] = { 0, 0 };
        for (uint32_t w = 0; w < 4; w++) { sum[0] += sh.sums[w][0]; sum[1] += sh.sums[w][1]; }
        delims[blockIdx.x] = sum[0]; kept[blockIdx.x] = sum[1]; headMask[blockIdx.x] = k.headMask;
        const bool open = blockIdx.x + 1u == tiles && src[size - 1u] != (uint8_t)delim;
        flags[blockIdx.x] = (k.anyDelim ? kFindreHasDelim : 0u) | (open ? kFindreOpenEnd : 0u);
    }
}
// one workgroup of 1024: the state entering every tile, ZS_FINDRE_CARRY_ROUND tiles a round - the round's OUT functions go to LDS (a tile
// behind the last: the identity), wavefront w takes tiles 32 w .. 32 w + 31, lanes as states
#define ZS_FINDRE_CARRY_ROUND 512u
__global__ void __launch_bounds__(1024)
k_findre_carry(const uint8_t *__restrict__ outFn, const uint64_t *__restrict__ headMask, uint32_t *__restrict__ flags, uint32_t *__restrict__ kept, uint32_t tiles,
               uint32_t n, uint32_t start, uint64_t accept, uint32_t invert)
{
    __shared__ __attribute__((aligned(16))) uint8_t fn[ZS_FINDRE_CARRY_ROUND * 64u];
    __shared__ uint8_t chunkFn[16][64];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    uint32_t state = start;                                                // the state in front of the round's first tile
    for (uint32_t t0 = 0; t0 < tiles; t0 += ZS_FINDRE_CARRY_ROUND) {
        const uint32_t cnt = min(ZS_FINDRE_CARRY_ROUND, tiles - t0);
        #pragma unroll
        for (uint32_t j = 0; j < 2; j++) {                                 // 16 bytes a lane, twice
            const uint32_t idx = threadIdx.x + 1024u * j, first = (idx & 3u) * 16u;
            uint4 v;
            if (idx < cnt * 4u) v = *(const uint4 *)(outFn + (uint64_t)t0 * 64u + 16u * idx);
            else { v.x = first * 0x01010101u + 0x03020100u; v.y = v.x + 0x04040404u; v.z = v.y + 0x04040404u; v.w = v.z + 0x04040404u; }
            *(uint4 *)(fn + 16u * idx) = v;
        }
        const uint32_t t = t0 + 32u * wave + lane;                         // lanes 0 .. 31: a tile each (tiles <= 0x7FFFFFFF: no wrap)
        const bool own = lane < 32u && t < tiles;
        const uint32_t f = own ? flags[t] : 0u;
        const uint64_t head = own && (f & kFindreHasDelim) ? headMask[t] : 0ull;
        __syncthreads();
        const uint32_t d = (uint32_t)__ballot((f & kFindreHasDelim) != 0u);
        {
            uint32_t x = min(lane, n - 1u), j = 0;
            if (d) j = 31u - (uint32_t)__clz((int)d);                      // (constant behind the last tile with a delimiter: start there)
            for (; j < 32u; j++) x = fn[(32u * wave + j) * 64u + x];
            chunkFn[wave][lane] = (uint8_t)x;
        }
        __syncthreads();
        uint32_t in = state;
        #pragma unroll
        for (uint32_t w = 0; w < 16; w++) {
            if (w == wave) in = state;
            state = chunkFn[w][state];
        }
        uint32_t carry = in;
        {
            uint32_t x = in;
            for (uint32_t j = 0; j < 31u; j++) {
                x = fn[(32u * wave + j) * 64u + x];
                if (j + 1u == lane) carry = x;
            }
        }
        if (own) {
            uint32_t add = 0;                                              // (modulo 2^32: -1 where a listed first record end is no longer)
            if (f & kFindreHasDelim) add = (uint32_t)((head >> carry) & 1ull) - (uint32_t)((head >> start) & 1ull);
            if ((f & kFindreOpenEnd) && zs_regex_listed(accept, invert, fn[(32u * wave + lane) * 64u + carry])) add += 1u;      // (set on the last tile only)
            flags[t] = f | (carry << 8);
            if (add) kept[t] += add;
        }
        __syncthreads();                                                   // (the next round writes fn and chunkFn again)
    }
}
// The masks again, the carried state in front.  recBase[tile]: the delimiters in front of the tile (recBase[tiles]: all); slotBase[tile]:
// the listed records in front of it (slotBase[tiles]: total).  A step's record ends follow the steps before it, a wavefront's the
// wavefronts before it, a lane's the lanes before it.  base: one device word, or null for 0.  code: null, or the window's code - not 0:
// nothing is written and dResult states it.  The grid is max(tiles, 1)
__global__ void __launch_bounds__(256)
k_findre_emit(const uint8_t *__restrict__ src, uint64_t size, uint32_t delim, const zsmi_regexProgram P, uint32_t tiles, const uint32_t *__restrict__ flags,
              const uint64_t *__restrict__ recBase, const uint64_t *__restrict__ slotBase, const uint64_t *__restrict__ base, const uint32_t *__restrict__ code,
              uint64_t *__restrict__ records, uint64_t capacity, uint64_t *__restrict__ result)
{
    __shared__ ZsFindreShared sh;
    uint64_t slot0;
    if (!zs_find_emit_head(code, slotBase, tiles, capacity, size, [&] { return recBase[tiles] + (tiles && (flags[tiles - 1u] & kFindreOpenEnd) ? 1ull : 0ull); }, true, result, slot0)) return;
    ZsFindreMasks k;
    const uint32_t f = flags[blockIdx.x];
    zs_findre_tile<false>(src, size, delim, P, blockIdx.x, (f >> 8) & 0xFFu, sh, k);
    const uint64_t first = (base ? *base : 0ull) + recBase[blockIdx.x];
    const ZsFindEmitted n = zs_find_emit_tail(k.dm, k.km, slot0, first, capacity, records, [](uint64_t, uint32_t, uint32_t) {});
    if (threadIdx.x == 0 && (f & kFindreOpenEnd) && zs_regex_listed(P.accept, P.flags & ZSMI_REGEX_INVERT, k.out))
        zs_find_emit_open(slot0 + n.kept, first + n.delims, capacity, records, [](uint64_t) {});
}

// ---- host ----
extern "C" int zsmi_compileRegex(const void *pattern, size_t patternSize, uint32_t flags, zsmi_regexProgram *prog, size_t *errorAt)
{
    try { return zs_regex_compile(pattern, patternSize, flags, prog, errorAt); }
    catch (const std::bad_alloc &) { return ZSMI_error_memory_allocation; }
}
extern "C" size_t zsmi_findRecordsRegex(const void *src, size_t srcSize, int delim, const zsmi_regexProgram *prog, uint64_t base,
                                        uint64_t *records, size_t capacity, uint64_t *textRecords)
{
    if (!prog || (capacity && !records)) return ZSMI_ERR(ZSMI_error_GENERIC);
    if (const int e = zs_regex_check(delim, prog)) return ZSMI_ERR(e);
    if (srcSize && !src) return ZSMI_ERR(ZSMI_error_srcSize_wrong);
    return (size_t)zs_regex_records((const uint8_t *)src, srcSize, (uint8_t)delim, prog, base, records, capacity, textRecords);
}
// what the search lays behind find.hip's words of a text's tiles in the seekable scratch, findReserve's extra region: OUT functions
// [64 a tile], HEADMASKs [8 a tile]
static const size_t kFindreExtraPerTile = 64 + sizeof(uint64_t);
// the launch sequence over dText[0, size), its arguments checked and its scratch reserved by the caller
static int findreText(zsmi_ctx *c, const void *dText, uint64_t size, int delim, const zsmi_regexProgram &P, const uint64_t *dBase, const uint32_t *dCode,
                      uint64_t *dRecords, uint64_t capacity, uint64_t *dResult, const FindTiles &t)
{
    uint8_t *dOutFn = t.dExtra;
    uint64_t *dHeadMask = (uint64_t *)(dOutFn + (size_t)t.tiles * 64u);
    if (t.tiles) {
        LAUNCH(c, "k_findre_count", k_findre_count, dim3(t.tiles), dim3(256), 0, (const uint8_t *)dText, size, (uint32_t)delim, P, t.tiles, t.dDelims, t.dKept, t.dFlags,
               dHeadMask, dOutFn);
        LAUNCH(c, "k_findre_carry", k_findre_carry, dim3(1), dim3(1024), 0, (const uint8_t *)dOutFn, (const uint64_t *)dHeadMask, t.dFlags, t.dKept, t.tiles,
               P.nStates, P.start, P.accept, P.flags & ZSMI_REGEX_INVERT);
    }
    if (const int e = findScans(c, t, false)) return e;
    LAUNCH(c, "k_findre_emit", k_findre_emit, dim3(std::max(t.tiles, 1u)), dim3(256), 0, (const uint8_t *)dText, size, (uint32_t)delim, P, t.tiles, (const uint32_t *)t.dFlags,
           (const uint64_t *)t.dRecBase, (const uint64_t *)t.dSlotBase, dBase, dCode, dRecords, capacity, dResult);
    return c->launched();
}
extern "C" int zsmi_findRecordsRegexDevice(zsmi_ctx *c, const void *dSrc, uint64_t srcSize, int delim, const zsmi_regexProgram *prog,
                                           const uint64_t *dBase, uint64_t *dRecords, uint64_t capacity, uint64_t *dResult)
{
    if (!c) return ZSMI_error_init_missing;
    if (!dResult || !prog || (capacity && !dRecords)) return ZSMI_error_GENERIC;
    if (const int e = zs_regex_check(delim, prog)) return e;
    if (srcSize && !dSrc) return ZSMI_error_srcSize_wrong;
    if (const int e = c->bind()) return e;
    if (srcSize == 0) return c->fill(dResult, 0, 4 * sizeof(uint64_t));
    FindTiles t;
    if (const int e = findReserve(c, srcSize, 0, 0, t, kFindreExtraPerTile)) return e;
    return findreText(c, dSrc, srcSize, delim, *prog, dBase, nullptr, dRecords, capacity, dResult, t);
}
extern "C" int zsmi_seekableFindRegexResident(zsmi_ctx *c, const zsmi_seekable *sk, const uint64_t *dFirstRecord, uint32_t nFrames, int delim,
                                              const zsmi_regexProgram *prog, uint32_t firstFrame, uint32_t frameCount, void *dWork, uint64_t workCapacity,
                                              uint64_t *dRecords, uint64_t capacity, uint64_t *dResult)
{
    if (const int e = findCheck(c, sk, dFirstRecord, nFrames, prog, [&] { return zs_regex_check(delim, prog); }, firstFrame, frameCount, false, dWork, workCapacity, dRecords,
                                capacity, dResult)) return e;
    return findWindow(c, sk, firstFrame, frameCount, dWork, dResult, kFindreExtraPerTile, [&](const FindDecoded &w, const FindTiles &t) {
        return findreText(c, dWork, w.bytes, delim, *prog, dFirstRecord + firstFrame, w.dCode, dRecords, capacity, dResult, t);
    });
}
// host arrays in and out (find.hip's findStage).  As with `none`, a program can list a record a byte: the staged numbers are the window's
// bytes, or capacity
extern "C" int zsmi_seekableFindRegexHost(zsmi_ctx *c, const zsmi_seekable *sk, const uint64_t *firstRecord, uint32_t nFrames, int delim,
                                          const zsmi_regexProgram *prog, uint32_t firstFrame, uint32_t frameCount,
                                          uint64_t *records, size_t capacity, uint64_t *result)
{
    if (const int e = findCheck(c, sk, firstRecord, nFrames, prog, [&] { return zs_regex_check(delim, prog); }, firstFrame, frameCount, true, nullptr, 0, records, capacity,
                                result)) return e;
    const uint64_t bytes = zsmi_seekableFindWorkBound(sk, firstFrame, frameCount);
    const size_t room = (size_t)std::min<uint64_t>(capacity, bytes);
    return findStage(c, firstRecord, nFrames, bytes, room, false, 0, 0, records, nullptr, result, [&](const FindStaged &s) {
        return zsmi_seekableFindRegexResident(c, sk, s.dFirst, nFrames, delim, prog, firstFrame, frameCount, s.dWork, bytes, s.dRecords, room, s.dResult);
    });
}
