// seekable.hip -- zstd's seekable format over the batch paths of zsmi_api.hip (zsmi_ctx.h declares them).
//
//   archive    = frame_0 .. frame_{n-1} | seek table
//   seek table = 0x184D2A5E | Frame_Size | entry_0 .. entry_{n-1} | Number_Of_Frames | Seek_Table_Descriptor | 0x8F92EAB1   (little-endian)
//   entry      = Compressed_Size | Decompressed_Size [| Checksum: low 32 bits of XXH64 (seed 0) of the frame's content, when descriptor bit 7]
//
// Compress: the frames are the chunks of one batch compress call - chunk i = src[o_i, o_i + frameSizes[i]), o the running sum of the caller's
// sizes (a record archive: zsmi_compressSeekableFrames*, each frame with the dictionary the caller picks from a CDict set) or of F, F, .., rest
// (zsmi_compressSeekable*: the fixed-size case of the same path) - into context staging at the running sum of compressBound(frameSizes[i]);
// k_seek_hash hashes the INPUT of each frame (checksum flag), the pack kernels close the gaps into dDst, k_seek_table writes the table behind
// them and the archive's size (or the first failing frame's code).
// Decompress: the table is read and checked on the host - once for an opened archive (zsmi_seekable), per call by the single-range calls.  A
// read is a batch of ranges: the union of the frames they overlap are items of the batch decoder with their exact Decompressed_Size as
// capacity, each decoded once - a frame wholly inside the one range that touches it straight into dDst, every other one into context scratch,
// from where k_seek_gather copies its overlaps with the ranges - then k_seek_verify checks every decoded frame's size and checksum against
// its entry and k_seek_range_status gives each range the code of its first failing frame.  A handle opened with a DDict set decodes every
// frame with the dictionary its dictID names (a record archive's reader); a read by frame index is the read of those frames' extents.
// Device-resident record archives: the same two paths planned from device memory.  A write whose sizes and dictionary indices are device
// arrays (zsmi_compressSeekableFramesResident*) cleans the sizes with k_seek_guard, compresses through the body of the resident batch call
// into staging sized for every split of the content, and shares the packing tail (seekPackArchive); a read whose frame numbers are a
// device array (zsmi_seekableReadFramesResident) looks them up in the handle's device copy of the table, lays the outputs out with the
// layout scan and decodes every request straight to its place - no union, no scratch: a frame named twice is decoded twice.  That
// sequence is the frame-list decode (seekDecodeList), which every call that decodes frames by device numbers runs - records by number, the
// searches, the record index, the frame filter; their shared checks (seekWindowCheck) and the host builds' window plan (seekCutWindows)
// stand beside it.
// Streams without a table (zsmi_openFrames*): the frame index (zsmi_index.h) - one entry a frame, read from the frames' own headers, on the
// host by the serial walk, on the device by the k_index_* kernels - fills the same SeekTable, and the handle is the one above.

#include "zsmi_status.h"          // the size word a compressed or decoded frame leaves
#include "zsmi_wave.h"            // zs_block_copy, xxh64_quad, rd32
#include "entropy_kernels.hip"    // k_pack_offsets, k_pack_copy
#include "decode_kernels.hip"     // the decoder's error codes (E_*)
#include "zsmi_ctx.h"
#include "zsmi_index.h"           // the frame index of a stream without a table; the format's limits
#include <algorithm>
#include <cstdlib>
#include <new>

static const uint32_t kSeekSkippableMagic = 0x184D2A5Eu, kSeekableMagic = 0x8F92EAB1u;
static const uint64_t kSeekMaxFrames = ZS_SEEK_MAX_FRAMES, kSeekMaxFrameSize = ZS_SEEK_MAX_FRAME_SIZE;
static const uint64_t kSeekTableFixed = ZS_SEEK_TABLE_FIXED;          // skippable header (8) + footer (9)
static const uint32_t kSeekHashAhead = 16;           // stripes a lane has in flight in k_seek_hash

// ---- kernels ----
__device__ __forceinline__ void seek_st32(uint8_t *p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24); }

// XXH64 of each frame's input (frame f: src[contentOff[f], + frameSizes[f])): one quad a frame (16 a wavefront), kSeekHashAhead stripes a lane
// in flight.  At 64 KiB frames 1 GiB is 16384 quads - one wavefront a SIMD - so the loads of one lane, not the number of wavefronts, are what
// hides the memory latency.
__global__ void __launch_bounds__(64) k_seek_hash(const uint8_t *__restrict__ src, const uint64_t *__restrict__ contentOff, const uint32_t *__restrict__ frameSizes, uint32_t n,
                                                  uint32_t *__restrict__ hashes)
{
    const uint32_t q = blockIdx.x * 16 + (threadIdx.x >> 2);
    const bool real = q < n;
    const uint32_t f = real ? q : n - 1u;
    const uint64_t len = real ? frameSizes[f] : 0ull;
    const uint64_t h = xxh64_quad<kSeekHashAhead>(src + contentOff[f], len);      // (every lane of a quad calls: its four accumulators)
    if (real && (threadIdx.x & 3u) == 0) hashes[f] = (uint32_t)h;
}
// the table behind the packed frames: one entry a thread, the header and the footer from the first; a failed frame's (index << 8 | code) goes to
// *err (set to ~0 before), the lowest wins
__global__ void k_seek_table(const uint32_t *__restrict__ sizes, const uint64_t *__restrict__ packedOffsets, const uint32_t *__restrict__ hashes,
                             const uint32_t *__restrict__ frameSizes, uint32_t n, int checksum, uint8_t *__restrict__ dst, unsigned long long *err)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x, E = checksum ? 12u : 8u;
    uint8_t *t = dst + packedOffsets[n];
    if (i == 0) {
        seek_st32(t, kSeekSkippableMagic); seek_st32(t + 4, n * E + 9u);
        uint8_t *f = t + 8 + (uint64_t)n * E;
        seek_st32(f, n); f[4] = checksum ? 0x80 : 0; seek_st32(f + 5, kSeekableMagic);
    }
    if (i >= n) return;
    const uint32_t s = sizes[i];
    if (zs_word_is_error(s)) atomicMin(err, ((unsigned long long)i << 8) | zs_word_code(s));
    uint8_t *e = t + 8 + (uint64_t)i * E;
    seek_st32(e, zs_word_bytes(s)); seek_st32(e + 4, frameSizes[i]);
    if (checksum) seek_st32(e + 8, hashes[i]);
}
__global__ void k_seek_finish(const uint64_t *__restrict__ packedOffsets, uint32_t n, uint32_t entryBytes, const unsigned long long *__restrict__ err, uint64_t *archiveSize)
{
    const unsigned long long e = *err;
    *archiveSize = e == ~0ull ? packedOffsets[n] + kSeekTableFixed + (uint64_t)n * entryBytes : 0ull - (e & 0xFFu);
}

// ---- the resident compress call's own kernels (zsmi_compressSeekableFramesResident*): the caller's sizes are device memory, so what
// seekFramesBound judges on the host is judged here, a lane a frame.  rawOff: the running sum of the caller's sizes (n + 1 entries) ----
// a frame the archive can hold: no longer than the host was told, and its content inside [0, srcSize)
__device__ __forceinline__ bool zs_seek_frame_ok(uint32_t size, uint64_t off, uint32_t maxFrameSize, uint64_t srcSize)
{
    return size <= maxFrameSize && off <= srcSize && size <= srcSize - off;
}
// the CLEANED size list, which every later kernel reads in place of the caller's: a refused frame is an empty one at content offset 0, so no
// kernel reads dSrc outside [0, srcSize) and the kept frames' bounds add up to no more than zs_compress_bound_split(srcSize, n)
__global__ void __launch_bounds__(256)
k_seek_guard(const uint32_t *__restrict__ frameSizes, const uint64_t *__restrict__ rawOff, uint32_t n, uint32_t maxFrameSize, uint64_t srcSize,
             uint32_t *__restrict__ cleanSizes, uint64_t *__restrict__ cleanOff)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint32_t size = frameSizes[i]; const uint64_t off = rawOff[i];
    const bool ok = zs_seek_frame_ok(size, off, maxFrameSize, srcSize);
    cleanSizes[i] = ok ? size : 0u; cleanOff[i] = ok ? off : 0ull;
}
// behind the compress call, in front of k_seek_table: a refused frame's size word says so (srcSize_wrong: over the dictionary index's
// refusal, as in k_plan_refuse); sizes that end in front of srcSize fail the archive as frame n would - any failing frame's code comes first
__global__ void __launch_bounds__(256)
k_seek_refuse(const uint32_t *__restrict__ frameSizes, const uint64_t *__restrict__ rawOff, uint32_t n, uint32_t maxFrameSize, uint64_t srcSize,
              uint32_t refusal, uint32_t *__restrict__ sizes, unsigned long long *err)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i == 0 && rawOff[n] < srcSize) atomicMin(err, ((unsigned long long)n << 8) | zs_word_code(refusal));
    if (i < n && !zs_seek_frame_ok(frameSizes[i], rawOff[i], maxFrameSize, srcSize)) sizes[i] = refusal;
}

struct ZsSeekItem { uint64_t out; uint32_t size, hash, slot, pad; };     // a decoded frame: where its bytes are, its entry, its status word
struct ZsSeekPiece { uint64_t from, to; uint32_t len, pad; };            // one scratch frame's overlap with one range (a tile of it): scratch + from -> dDst + to
struct ZsSeekSpan { uint32_t firstSlot, count; };                        // a range's frames: consecutive entries of the per-frame code array
static const uint32_t kSeekTile = 64u << 10;         // the most a workgroup of k_seek_gather copies: longer pieces are cut into tiles in the list
static const uint32_t kSeekWavePiece = 4u << 10;     // pieces up to this take one wavefront each (four to a workgroup): 64 lanes x 16 bytes x 4 in flight

// The pieces of the frames that more than one range reads, or one range reads in part: scratch -> dDst.  pieces[0, nSmall) are the short ones
// (records: up to kSeekWavePiece bytes), a wavefront each, four to a workgroup; pieces[nSmall, nPieces) are tiles of up to kSeekTile bytes, a
// workgroup each.  Lane i moves the 16 bytes at 16 i of each 1 KiB (4 KiB a workgroup) step: whatever the two alignments are, a wavefront's
// accesses are one contiguous run.
__global__ void __launch_bounds__(256) k_seek_gather(const uint8_t *__restrict__ scratch, uint8_t *__restrict__ dst, const ZsSeekPiece *__restrict__ pieces,
                                                     uint32_t nSmall, uint32_t nPieces)
{
    const uint32_t gSmall = (nSmall + 3) / 4;
    if (blockIdx.x < gSmall) {
        const uint32_t k = blockIdx.x * 4 + (threadIdx.x >> 6);
        if (k >= nSmall) return;
        const ZsSeekPiece p = pieces[k];
        zs_block_copy(dst + p.to, scratch + p.from, p.len, threadIdx.x & 63u, 64u);
    } else {
        const uint32_t k = nSmall + (blockIdx.x - gSmall);
        if (k >= nPieces) return;
        const ZsSeekPiece p = pieces[k];
        zs_block_copy(dst + p.to, scratch + p.from, p.len, threadIdx.x, 256u);
    }
}
// one quad a decoded frame: its decoder status, its size against the entry (a frame the decoder found longer than its entry failed with
// dstSize_tooSmall: that is the same disagreement), its checksum (flag set).  codes[q]: frame q's code (0: none), the frames in index order.
// refused (null: no item is): the code of an item its planner refused and planned empty (zsmi_seekableReadFramesResident) - that is its
// code, whatever the decoder made of nothing
__global__ void __launch_bounds__(64) k_seek_verify(const ZsSeekItem *__restrict__ items, uint32_t m, const uint32_t *__restrict__ status, int checksum, uint32_t *__restrict__ codes,
                                                    const uint32_t *__restrict__ refused)
{
    const uint32_t q = blockIdx.x * 16 + (threadIdx.x >> 2);
    const bool real = q < m;
    const ZsSeekItem it = items[real ? q : m - 1u];
    const uint32_t s = real ? status[it.slot] : 0u;
    uint32_t code = refused && real ? refused[q] : 0u;
    if (code) { }
    else if (zs_word_is_error(s)) code = zs_word_code(s) == E_dstSize_tooSmall ? (uint32_t)E_corruption_detected : zs_word_code(s);
    else if (s != it.size) code = E_corruption_detected;
    const bool hash = real && checksum && code == 0;
    if (__ballot(hash)) {
        const uint64_t h = xxh64_quad<kSeekHashAhead>((const uint8_t *)it.out, hash ? it.size : 0u);
        if (hash && (uint32_t)h != it.hash) code = E_checksum_wrong;
    }
    if (real && (threadIdx.x & 3u) == 0) codes[q] = code;
}
// one wavefront a range (four to a workgroup): the code of the first failing frame, in content order, among the range's frames - the lanes
// stride over the span, each stops at its first failing entry k, the lowest k of the wavefront decides (k alone is reduced: an archive may
// hold 2^27 frames, so k << 8 | code does not fit the 32 bits of the wave_* primitives).  An empty range: 0.
__global__ void __launch_bounds__(256) k_seek_range_status(const ZsSeekSpan *__restrict__ spans, uint32_t nRanges, const uint32_t *__restrict__ codes, uint32_t *__restrict__ status)
{
    const uint32_t r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (r >= nRanges) return;                                            // (the same for every lane of a wavefront)
    const ZsSeekSpan s = spans[r];
    uint32_t first = ~0u;
    // (eight entries a lane and round.  The whole archive as one range is 16384 entries and takes 0.066 ms here: the compiler still waits for each
    // of the eight guarded loads in turn; loads at a clamped index, none behind a branch, are the next step, not measured yet)
    for (uint32_t k0 = lane; k0 < s.count && first == ~0u; k0 += 64 * 8) {
        uint32_t v[8];
        #pragma unroll
        for (uint32_t j = 0; j < 8; j++) { const uint32_t k = k0 + 64 * j; v[j] = k < s.count ? codes[s.firstSlot + k] : 0u; }
        #pragma unroll
        for (uint32_t j = 0; j < 8; j++) if (v[j] && first == ~0u) first = k0 + 64 * j;
    }
    first = wave_min(first);
    if (lane == 0) status[r] = first == ~0u ? 0u : codes[s.firstSlot + first];
}

// ---- records by numbers that are device memory (zsmi_seekableReadFramesResident): the handle's table in device memory, an entry a frame,
// and the two kernels that plan the read from it, a lane a request ----
struct ZsSeekEntry { uint64_t cOff; uint32_t cSize, dSize, hash, pad; };  // where a frame's compressed bytes start, the entry's two sizes, its checksum (0 without the flag)
// the bytes request k gets - its frame's Decompressed_Size, none for a number at or above the frame count - for the layout scan
__global__ void __launch_bounds__(256)
k_seek_request_sizes(const ZsSeekEntry *__restrict__ table, uint32_t nTable, const uint32_t *__restrict__ frameIndex, uint32_t nFrames, uint64_t *__restrict__ sizes)
{
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= nFrames) return;
    const uint32_t f = frameIndex[k];
    sizes[k] = f < nTable ? table[f].dSize : 0ull;
}
// behind the layout: request k's decode item (its frame's extent -> its place, the entry's Decompressed_Size as capacity), its verify record
// (status word k) and dWritten[k].  A number that names no frame (frameIndex_tooLarge), or a place that ends behind dstCapacity
// (dstSize_tooSmall): refused[k] says so and the item is an EMPTY one - no source, no capacity - so the decoder touches neither a frame nor dDst for it
__global__ void __launch_bounds__(256)
k_seek_request_items(const ZsSeekEntry *__restrict__ table, uint32_t nTable, const uint32_t *__restrict__ frameIndex, uint32_t nFrames,
                     const uint64_t *__restrict__ dstOffsets, uint64_t dstCapacity, uint8_t *dst, ZsDecItem *__restrict__ items,
                     ZsSeekItem *__restrict__ verify, uint32_t *__restrict__ refused, uint32_t *__restrict__ written)
{
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= nFrames) return;
    const uint32_t f = frameIndex[k];
    const bool named = f < nTable;
    ZsSeekEntry e; e.cOff = 0; e.cSize = 0; e.dSize = 0; e.hash = 0; e.pad = 0;
    if (named) e = table[f];
    const uint64_t at = dstOffsets[k];
    const bool fits = at <= dstCapacity && e.dSize <= dstCapacity - at;
    const bool take = named && fits;
    ZsDecItem it; it.srcOff = take ? e.cOff : 0ull; it.dstOff = take ? at : 0ull; it.srcSize = take ? e.cSize : 0u; it.dstCap = take ? e.dSize : 0u;
    items[k] = it;
    ZsSeekItem v; v.out = (uint64_t)(uintptr_t)(dst + it.dstOff); v.size = e.dSize; v.hash = e.hash; v.slot = k; v.pad = 0;
    verify[k] = v;
    refused[k] = !named ? (uint32_t)ZSMI_error_frameIndex_tooLarge : (!fits ? (uint32_t)ZSMI_error_dstSize_tooSmall : 0u);
    written[k] = e.dSize;
}

// ---- the frame index of a stream that carries no table (zsmi_openFramesDevice; zsmi_index.h states the index and judges a frame).  The
// true frames are the chain from offset 0 - each frame starts where the one before it ends - and a chain is serial: two dependent loads
// that miss to HBM a frame.  Every frame starts with a magic number though, so: find every position that holds one (the CANDIDATES, with
// offset 0 whatever its bytes: the chain's head), in ascending order - k_index_count, scanOffsets over the tiles' counts, k_index_emit;
// walk the frame each candidate would start, a lane a candidate, and look its end up among the candidates: its successor - k_index_walk;
// mark what the head reaches by pointer doubling over the successors - k_index_jump, ceil(log2(m + 1)) rounds for m candidates; and
// compact the marked candidates, in order, into the table's entries - scanOffsets over the marks, k_index_table.  A magic number inside
// a block's payload is a candidate like any other; nothing reaches it, even where it opens a whole valid frame, so it is no entry. ----
#define ZS_INDEX_TILE 16384u             // the bytes of the stream a workgroup scans: 4 steps x 256 threads x 16 bytes
static const uint32_t kIndexEnd = 0xFFFFFFFFu, kIndexBad = 0xFFFFFFFEu;      // a successor that is none: the stream's end; no candidate where the frame ends (or no frame)
struct ZsIndexHead { uint64_t marked, err, refused; };     // what k_index_table leaves in front of the entries: the marked candidates (the scan's total),
                                                           // ~0 or (position << 8 | code) of the chain's failure, how many marked candidates are refused frames
// bit k: the four bytes at 16-byte group g's byte k are a magic number.  d: the group's four words and the word behind it
__device__ __forceinline__ uint32_t zs_index_group_mask(const uint32_t d[5])
{
    uint32_t m = 0;
    #pragma unroll
    for (uint32_t k = 0; k < 16; k++) {
        const uint64_t pair = ((uint64_t)d[k / 4 + 1] << 32) | d[k / 4];
        m |= (uint32_t)zs_index_magic((uint32_t)(pair >> (8 * (k % 4)))) << k;
    }
    return m;
}
// The candidates of tile `tile`: mask[s] bit k stands for position tile * ZS_INDEX_TILE + s * 4096 + 16 * threadIdx.x + k, so the positions
// ascend with (s, thread, k).  Thread t reads its 16 bytes and the 4 behind them - lane i at base + 16 i, a wavefront's loads one
// contiguous KiB, the four steps' loads issued together - so a magic number that straddles two threads' or two tiles' bytes belongs to the
// one position it starts at: seen once, by that position's owner.  A tile that ends within 4 bytes of the stream's end takes the slow
// form, byte by byte with zeros behind the end: no byte outside [src, src + size) is read, and a position whose four bytes are not all
// inside is no candidate.
struct ZsIndexBytes16 { uint32_t w[4]; };
__device__ __forceinline__ void zs_index_tile_masks(const uint8_t *__restrict__ src, uint64_t size, uint64_t tile, uint32_t mask[4])
{
    const uint64_t base = tile * ZS_INDEX_TILE + 16u * threadIdx.x;
    if (size - tile * ZS_INDEX_TILE >= ZS_INDEX_TILE + 4u) {
        ZsIndexBytes16 own[4]; uint32_t behind[4];
        #pragma unroll
        for (uint32_t s = 0; s < 4; s++) { const uint8_t *p = src + base + s * 4096u; __builtin_memcpy(&own[s], p, 16); behind[s] = zs_load32(p + 16); }
        #pragma unroll
        for (uint32_t s = 0; s < 4; s++) { const uint32_t d[5] = { own[s].w[0], own[s].w[1], own[s].w[2], own[s].w[3], behind[s] }; mask[s] = zs_index_group_mask(d); }
    } else {
        for (uint32_t s = 0; s < 4; s++) {
            const uint64_t b = base + s * 4096u;
            uint32_t d[5] = { 0, 0, 0, 0, 0 };
            for (uint32_t j = 0; j < 20; j++) if (b + j < size) d[j >> 2] |= (uint32_t)src[b + j] << (8 * (j & 3));
            const uint64_t whole = b + 4 <= size ? size - 3 - b : 0;                   // positions from b on whose four bytes are inside
            mask[s] = zs_index_group_mask(d) & (whole >= 16 ? 0xFFFFu : (1u << whole) - 1u);
        }
    }
    if (tile == 0 && threadIdx.x == 0) mask[0] |= 1u;                                   // offset 0: the head, whatever its bytes
}
__global__ void __launch_bounds__(256) k_index_count(const uint8_t *__restrict__ src, uint64_t size, uint32_t *__restrict__ counts)
{
    __shared__ uint32_t waves[4];
    uint32_t mask[4];
    zs_index_tile_masks(src, size, blockIdx.x, mask);
    const uint32_t n = wave_sum(__popc(mask[0]) + __popc(mask[1]) + __popc(mask[2]) + __popc(mask[3]));
    if ((threadIdx.x & 63u) == 0) waves[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) counts[blockIdx.x] = waves[0] + waves[1] + waves[2] + waves[3];
}
// the same masks again; tileBase[tile]: the candidates in front of the tile (scanOffsets over the counts).  A step's candidates follow the
// steps before it, a wavefront's the wavefronts before it, a thread's the lanes before it
__global__ void __launch_bounds__(256) k_index_emit(const uint8_t *__restrict__ src, uint64_t size, const uint64_t *__restrict__ tileBase, uint64_t *__restrict__ pos, uint64_t m)
{
    __shared__ uint32_t waves[4][4];
    uint32_t mask[4], before[4];
    zs_index_tile_masks(src, size, blockIdx.x, mask);
    const uint32_t wave = threadIdx.x >> 6;
    #pragma unroll
    for (uint32_t s = 0; s < 4; s++) {
        const uint32_t n = __popc(mask[s]), incl = wave_incl_scan(n);
        before[s] = incl - n;
        if ((threadIdx.x & 63u) == 63u) waves[s][wave] = incl;
    }
    __syncthreads();
    uint64_t at = tileBase[blockIdx.x];
    #pragma unroll
    for (uint32_t s = 0; s < 4; s++) {
        uint32_t front = 0, all = 0;
        #pragma unroll
        for (uint32_t w = 0; w < 4; w++) { front += w < wave ? waves[s][w] : 0u; all += waves[s][w]; }
        uint64_t out = at + front + before[s];
        const uint64_t b = (uint64_t)blockIdx.x * ZS_INDEX_TILE + s * 4096u + 16u * threadIdx.x;
        for (uint32_t bits = mask[s]; bits; bits &= bits - 1u, out++) if (out < m) pos[out] = b + (uint32_t)__ffs((int)bits) - 1u;      // (m: the room the counts asked for)
        at += all;
    }
}
// a lane a candidate: the frame it would start (zs_index_frame reads only [src + p, src + size)), and its successor - the candidate at
// p + cSize, by binary search over the ascending positions; kIndexEnd where the frame ends the stream; kIndexBad where no candidate sits
// (the chain fails THERE, should it come this way) or the frame is refused (it fails HERE).  The head starts marked.
__global__ void __launch_bounds__(256)
k_index_walk(const uint8_t *__restrict__ src, uint64_t size, const uint64_t *__restrict__ pos, uint32_t m, uint32_t *__restrict__ status, uint32_t *__restrict__ cSize,
             uint32_t *__restrict__ dSize, uint32_t *__restrict__ next, uint32_t *__restrict__ mark)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= m) return;
    const uint64_t p = pos[i];
    ZsIndexFrame f = {}; f.status = ZSMI_error_GENERIC;                                   // (a position outside the stream: one its owner changed under the call)
    if (p < size) f = zs_index_frame(src + p, size - p);
    uint32_t succ = kIndexBad;
    if (!f.status) {
        const uint64_t end = p + f.cSize;
        if (end == size) succ = kIndexEnd;
        else {
            uint32_t lo = i + 1, hi = m;                                                   // (end > p: the first candidate at or behind end)
            while (lo < hi) { const uint32_t mid = lo + (hi - lo) / 2; if (pos[mid] < end) lo = mid + 1; else hi = mid; }
            if (lo < m && pos[lo] == end) succ = lo;
        }
    }
    status[i] = f.status; cSize[i] = (uint32_t)f.cSize; dSize[i] = f.dSize; next[i] = succ; mark[i] = i == 0;
}
// one round of pointer doubling.  In front of round k jump[i] is the candidate 2^k frames behind i and every candidate fewer than 2^k
// frames behind the head is marked; a marked candidate marks its jump, then the jumps are squared (into the other array: a round reads
// only what the round before wrote).  A mark seen while another lane of the round sets it marks a candidate the head reaches too: marks only grow
__global__ void __launch_bounds__(256) k_index_jump(const uint32_t *__restrict__ jump, uint32_t *__restrict__ squared, uint32_t *mark, uint32_t m)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= m) return;
    const uint32_t j = jump[i];
    if (j >= m) { squared[i] = j; return; }
    if (mark[i]) mark[j] = 1u;
    squared[i] = jump[j];
}
// the marked candidates, at the places the scan over the marks gives them, as the handle's entries.  The chain is one path, so one marked
// candidate at most ends it badly: a refused frame, with its code, or a frame that ends where no frame starts - prefix_unknown if the
// walker would find a word to judge there (5 bytes), else srcSize_wrong, as zsmi_findFrameCompressedSize answers those bytes
__global__ void __launch_bounds__(256)
k_index_table(const uint64_t *__restrict__ pos, const uint32_t *__restrict__ status, const uint32_t *__restrict__ cSize, const uint32_t *__restrict__ dSize,
              const uint32_t *__restrict__ next, const uint32_t *__restrict__ mark, const uint64_t *__restrict__ slot, uint32_t m, uint64_t size,
              ZsIndexHead *head, ZsSeekEntry *__restrict__ entries)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i == 0) head->marked = slot[m];
    if (i >= m || !mark[i]) return;
    const uint64_t p = pos[i];
    ZsSeekEntry e; e.cOff = p; e.cSize = cSize[i]; e.dSize = dSize[i]; e.hash = 0; e.pad = 0;
    entries[slot[i]] = e;
    if (status[i]) {
        atomicMin((unsigned long long *)&head->err, ((unsigned long long)p << 8) | status[i]);
        atomicAdd((unsigned long long *)&head->refused, 1ull);
    } else if (next[i] == kIndexBad) {
        const uint64_t end = p + e.cSize;
        atomicMin((unsigned long long *)&head->err, ((unsigned long long)end << 8) | (size - end >= 5 ? (uint32_t)ZSMI_error_prefix_unknown : (uint32_t)ZSMI_error_srcSize_wrong));
    }
}

// ---- host: parameters, bound, the table ----
static int seekParams(uint64_t srcSize, uint32_t frameSize, uint64_t &F, uint64_t &n)
{
    F = frameSize ? frameSize : ZS_BLOCK_MAX;
    if (F > kSeekMaxFrameSize) return ZSMI_error_parameter_outOfBound;
    n = srcSize / F + (srcSize % F != 0);
    return n > kSeekMaxFrames ? ZSMI_error_frameIndex_tooLarge : 0;
}
static uint64_t seekBound(uint64_t srcSize, uint64_t F, uint64_t n, int checksum)
{
    const uint64_t table = kSeekTableFixed + n * (checksum ? 12 : 8);
    return n ? (n - 1) * zsmi_compressBound(F) + zsmi_compressBound(srcSize - (n - 1) * F) + table : table;
}
extern "C" size_t zsmi_seekableBound(unsigned long long srcSize, uint32_t frameSize, int checksumFlag)
{
    uint64_t F, n;
    if (const int e = seekParams(srcSize, frameSize, F, n)) return ZSMI_ERR(e);
    return seekBound(srcSize, F, n, checksumFlag);
}
// the caller's frame sizes (a record archive): the three checks in the header's order, and the room the frames and the table need
static int seekFramesBound(const uint32_t *frameSizes, uint32_t n, int checksum, uint64_t &bound)
{
    if (n > kSeekMaxFrames) return ZSMI_error_frameIndex_tooLarge;
    if (n && !frameSizes) return ZSMI_error_GENERIC;
    bound = kSeekTableFixed + (uint64_t)n * (checksum ? 12 : 8);
    for (uint32_t i = 0; i < n; i++) {
        if (frameSizes[i] > kSeekMaxFrameSize) return ZSMI_error_parameter_outOfBound;
        bound += zsmi_compressBound(frameSizes[i]);
    }
    return 0;
}
extern "C" size_t zsmi_seekableFramesBound(const uint32_t *frameSizes, uint32_t n, int checksumFlag)
{
    uint64_t bound;
    if (const int e = seekFramesBound(frameSizes, n, checksumFlag, bound)) return ZSMI_ERR(e);
    return bound;
}

struct SeekTable {
    uint32_t n = 0, entry = 8; bool checksum = false;
    uint64_t tableSize = kSeekTableFixed;
    std::vector<uint64_t> cOff, dOff;              // n + 1 each: where frame i starts, compressed and in the content
    std::vector<uint32_t> cSize, dSize, hash;
};
// the footer (the archive's last 9 bytes): the frame count and the table's size
static int seekFooter(const uint8_t *footer, uint64_t srcSize, SeekTable &t)
{
    if (rd32(footer + 5) != kSeekableMagic) return ZSMI_error_prefix_unknown;
    const uint8_t desc = footer[4];
    if (desc & 0x7C) return ZSMI_error_corruption_detected;                 // reserved bits 6 - 2 (bits 1 - 0 are unused: ignored)
    const uint32_t n = rd32(footer);
    if (n > kSeekMaxFrames) return ZSMI_error_frameIndex_tooLarge;
    t.n = n; t.checksum = (desc & 0x80) != 0; t.entry = t.checksum ? 12 : 8;
    t.tableSize = kSeekTableFixed + (uint64_t)n * t.entry;
    return t.tableSize > srcSize ? ZSMI_error_corruption_detected : 0;
}
// the table's bytes (t.tableSize of them, after seekFooter): entries, and their sums against the archive
static int seekEntries(const uint8_t *tbl, uint64_t srcSize, SeekTable &t)
{
    if (rd32(tbl) != kSeekSkippableMagic) return ZSMI_error_prefix_unknown;
    if (rd32(tbl + 4) != t.n * t.entry + 9u) return ZSMI_error_corruption_detected;
    t.cOff.assign((size_t)t.n + 1, 0); t.dOff.assign((size_t)t.n + 1, 0);
    t.cSize.resize(t.n); t.dSize.resize(t.n); t.hash.assign(t.n, 0);
    const uint8_t *e = tbl + 8;
    for (uint32_t i = 0; i < t.n; i++, e += t.entry) {
        t.cSize[i] = rd32(e); t.dSize[i] = rd32(e + 4);
        if (t.checksum) t.hash[i] = rd32(e + 8);
        if (t.cSize[i] == 0 || t.dSize[i] > kSeekMaxFrameSize) return ZSMI_error_corruption_detected;
        t.cOff[i + 1] = t.cOff[i] + t.cSize[i]; t.dOff[i + 1] = t.dOff[i] + t.dSize[i];
    }
    return t.cOff[t.n] == srcSize - t.tableSize ? 0 : ZSMI_error_corruption_detected;
}
static int seekParseHost(const void *srcv, size_t srcSize, SeekTable &t)
{
    const uint8_t *src = (const uint8_t *)srcv;
    if (!src || srcSize < 9) return ZSMI_error_prefix_unknown;
    if (const int e = seekFooter(src + srcSize - 9, srcSize, t)) return e;
    return seekEntries(src + srcSize - t.tableSize, srcSize, t);
}
extern "C" size_t zsmi_seekableNumFrames(const void *src, size_t srcSize)
{
    SeekTable t;
    if (const int e = seekParseHost(src, srcSize, t)) return ZSMI_ERR(e);
    return t.n;
}
extern "C" size_t zsmi_seekableContentSize(const void *src, size_t srcSize)
{
    SeekTable t;
    if (const int e = seekParseHost(src, srcSize, t)) return ZSMI_ERR(e);
    return t.dOff[t.n];
}
extern "C" int zsmi_seekableFrameInfo(const void *src, size_t srcSize, uint32_t index, uint64_t *cOffset, uint64_t *dOffset, uint32_t *cSize, uint32_t *dSize)
{
    SeekTable t;
    if (const int e = seekParseHost(src, srcSize, t)) return e;
    if (index >= t.n) return ZSMI_error_frameIndex_tooLarge;
    if (cOffset) *cOffset = t.cOff[index];
    if (dOffset) *dOffset = t.dOff[index];
    if (cSize) *cSize = t.cSize[index];
    if (dSize) *dSize = t.dSize[index];
    return 0;
}

// ---- compress ----
// checksumFlag: the table's (each entry carries its frame's hash); frameChecksum: the frames' own Content_Checksum (the context's
// ZSMI_c_checksumFlag) - the two are independent
// The tail of both compress paths, all of it device memory: the frames lie in context staging at dStageOff with their size words in dSizes
// (an error word: a failed frame), dFrameSizes are the content sizes the entries state, dHash the entries' checksums (flag set), *dErr is
// ~0 or holds what the caller found wrong already.  The gaps are closed into dDst, the table written behind the frames, and
// *dArchiveSize is the archive's size or the lowest failing frame's code.
static int seekPackArchive(zsmi_ctx *c, const uint64_t *dStageOff, const uint32_t *dFrameSizes, uint32_t n, const uint32_t *dSizes, const uint32_t *dHash,
                           uint64_t *dPacked, unsigned long long *dErr, void *dDst, uint64_t *dArchiveSize, int checksumFlag)
{
    if (const int e = scanOffsets(c, "k_pack_offsets", dSizes, nullptr, n, 1u, nullptr, dPacked)) return e;
    if (n) LAUNCH(c, "k_pack_copy", k_pack_copy, dim3(n), dim3(256), 0, (const uint8_t *)c->seek.dStage.p, dStageOff, dSizes, (const uint64_t *)dPacked, (uint8_t *)dDst);
    LAUNCH(c, "k_seek_table", k_seek_table, dim3(std::max<uint32_t>(1, (n + 255) / 256)), dim3(256), 0, dSizes, (const uint64_t *)dPacked,
           dHash, dFrameSizes, n, checksumFlag ? 1 : 0, (uint8_t *)dDst, dErr);
    LAUNCH(c, "k_seek_finish", k_seek_finish, dim3(1), dim3(1), 0, (const uint64_t *)dPacked, n, checksumFlag ? 12u : 8u, (const unsigned long long *)dErr, dArchiveSize);
    return c->launched();
}
// The one path of every compress call with HOST sizes, its arguments checked by the caller: frame i is chunk i of one batch compress call with the
// selector `dict` (null: plain, at `level`), chunk i = dSrc[o_i, o_i + frameSizes[i]) with o the running sum of frameSizes (host, n entries).
//   The per-frame lists the device needs - the frames' staging offsets (the running sum of their bounds) and their sizes - go up through
// pinned buffers taken in turn (TurnBufs), as a read's lists do: nothing is copied back, nothing waited for.  The frames' content offsets,
// which only k_seek_hash reads, are scanOffsets over the uploaded sizes.
static int seekCompressFrames(zsmi_ctx *c, const void *dSrc, const uint32_t *frameSizes, uint32_t n, void *dDst, uint64_t *dArchiveSize,
                              int level, const ZsCDictSel *dict, int checksumFlag, int frameChecksum)
{
    if (const int e = c->bind()) return e;
    // device words: the uploaded lists - staging offsets [n] (64 bits), frame sizes [n]; (8-aligned) packed offsets [n + 1], content offsets
    // [n + 1], the error word; compressed sizes [n], hashes [n]
    const size_t listBytes = (size_t)n * (sizeof(uint64_t) + sizeof(uint32_t)), lists = (listBytes + 7) & ~(size_t)7;
    if (!c->seek.dMeta.reserve(lists + (2 * (size_t)n + 3) * sizeof(uint64_t) + 2 * (size_t)n * sizeof(uint32_t))) return ZSMI_error_memory_allocation;
    const uint64_t *dStageOff = (const uint64_t *)c->seek.dMeta.p;
    const uint32_t *dFrameSizes = (const uint32_t *)(dStageOff + n);
    uint64_t *dPacked = (uint64_t *)((uint8_t *)c->seek.dMeta.p + lists), *dContent = dPacked + n + 1;
    unsigned long long *dErr = (unsigned long long *)(dContent + n + 1);
    uint32_t *dSizes = (uint32_t *)(dErr + 1), *dHash = dSizes + n;
    if (n) {
        uint64_t *hStageOff;
        if (const int e = c->seek.hLists.take(listBytes, hStageOff)) return e;
        std::vector<uint64_t> so(n);
        uint64_t content = 0, stage = 0;
        for (uint32_t i = 0; i < n; i++) { so[i] = content; content += frameSizes[i]; hStageOff[i] = stage; stage += zsmi_compressBound(frameSizes[i]); }
        memcpy(hStageOff + n, frameSizes, (size_t)n * sizeof(uint32_t));
        if (!c->seek.dStage.reserve(stage)) return ZSMI_error_memory_allocation;
        if (const int e = c->toDevice(c->seek.dMeta.p, hStageOff, listBytes)) return e;
        if (const int e = c->seek.hLists.sent(c->stream)) return e;
        if (const int e = compressBatchDeviceImpl(c, dSrc, so.data(), frameSizes, n, c->seek.dStage.p, hStageOff, dSizes, level, dict, frameChecksum)) return e;
        if (checksumFlag) {
            if (const int e = scanOffsets(c, "k_pack_offsets", dFrameSizes, nullptr, n, 1u, nullptr, dContent)) return e;
            LAUNCH(c, "k_seek_hash", k_seek_hash, dim3((n + 15) / 16), dim3(64), 0, (const uint8_t *)dSrc, (const uint64_t *)dContent, dFrameSizes, n, dHash);
        }
    }
    if (const int e = c->fill(dErr, 0xFF, sizeof(*dErr))) return e;
    return seekPackArchive(c, dStageOff, dFrameSizes, n, dSizes, dHash, dPacked, dErr, dDst, dArchiveSize, checksumFlag);
}
// fixed-size frames: the sizes F, F, .., rest - the fixed-size case of the path above
static int compressSeekableImpl(zsmi_ctx *c, const void *dSrc, uint64_t srcSize, void *dDst, uint64_t dstCapacity, uint64_t *dArchiveSize,
                                int level, uint32_t frameSize, int checksumFlag, int frameChecksum)
{
    if (!c) return ZSMI_error_init_missing;
    uint64_t F, n64;
    if (const int e = seekParams(srcSize, frameSize, F, n64)) return e;
    if (dstCapacity < seekBound(srcSize, F, n64, checksumFlag)) return ZSMI_error_dstSize_tooSmall;
    if (!dArchiveSize || !dDst || (srcSize && !dSrc)) return ZSMI_error_GENERIC;
    std::vector<uint32_t> sizes((size_t)n64, (uint32_t)F);
    if (n64) sizes.back() = (uint32_t)(srcSize - (n64 - 1) * F);
    return seekCompressFrames(c, dSrc, sizes.data(), (uint32_t)n64, dDst, dArchiveSize, level, nullptr, checksumFlag, frameChecksum);
}
// the caller's frames: the header's checks in its order, then the path above.  set: null for the plain form (sel without a table)
static int compressSeekableFramesImpl(zsmi_ctx *c, const void *dSrc, const uint32_t *frameSizes, uint32_t n, void *dDst, uint64_t dstCapacity,
                                      uint64_t *dArchiveSize, int level, int checksumFlag, const zsmi_cdictSet *set, const uint32_t *dictIndex)
{
    if (!c) return ZSMI_error_init_missing;
    uint64_t bound;
    if (const int e = seekFramesBound(frameSizes, n, checksumFlag, bound)) return e;
    ZsCDictSel sel;
    if (set) { if (const int e = resolveCDictSet(c, set, dictIndex, n, level, sel, true)) return e; }
    if (dstCapacity < bound) return ZSMI_error_dstSize_tooSmall;
    bool content = false;
    for (uint32_t i = 0; i < n && !content; i++) content = frameSizes[i] != 0;
    if (!dArchiveSize || !dDst || (content && !dSrc)) return ZSMI_error_GENERIC;
    return seekCompressFrames(c, dSrc, frameSizes, n, dDst, dArchiveSize, level, &sel, checksumFlag, c->checksumFlag);
}
extern "C" int zsmi_compressSeekableFramesDevice(zsmi_ctx *c, const void *dSrc, const uint32_t *frameSizes, uint32_t n, void *dDst, uint64_t dstCapacity,
                                                 uint64_t *dArchiveSize, int level, int checksumFlag)
{
    return compressSeekableFramesImpl(c, dSrc, frameSizes, n, dDst, dstCapacity, dArchiveSize, level, checksumFlag, nullptr, nullptr);
}
extern "C" int zsmi_compressSeekableFramesDevice_usingCDictSet(zsmi_ctx *c, const void *dSrc, const uint32_t *frameSizes, uint32_t n, void *dDst, uint64_t dstCapacity,
                                                               uint64_t *dArchiveSize, int checksumFlag, const zsmi_cdictSet *set, const uint32_t *dictIndex)
{
    return compressSeekableFramesImpl(c, dSrc, frameSizes, n, dDst, dstCapacity, dArchiveSize, 3, checksumFlag, set, dictIndex);
}
// ---- the same archive from sizes (and dictionary indices) that are DEVICE memory: nothing is copied to the host, nothing waited for, no
// pinned buffer touched.  The host knows n, srcSize and maxFrameSize; its room for any split is zs_compress_bound_split (zsmi_device.h) ----
static int seekResidentBound(uint64_t srcSize, uint32_t n, int checksum, uint64_t &bound)
{
    if (n > kSeekMaxFrames) return ZSMI_error_frameIndex_tooLarge;
    if (srcSize > (uint64_t)n * kSeekMaxFrameSize) return ZSMI_error_parameter_outOfBound;       // (no legal split: n == 0 with content too)
    bound = zs_compress_bound_split(srcSize, n) + kSeekTableFixed + (uint64_t)n * (checksum ? 12 : 8);
    return 0;
}
extern "C" size_t zsmi_seekableFramesResidentBound(unsigned long long srcSize, uint32_t n, int checksumFlag)
{
    uint64_t bound;
    if (const int e = seekResidentBound(srcSize, n, checksumFlag, bound)) return ZSMI_ERR(e);
    return bound;
}
// The launch sequence (arguments checked by the caller).  scanOffsets over the caller's sizes gives the content offsets; k_seek_guard the
// cleaned sizes and offsets every later kernel reads; k_compress_bounds and a second scan the staging offsets; the body of
// zsmi_compressBatchResident[_usingCDictSet] compresses into the staging; k_seek_hash (table flag); k_seek_refuse marks what the guard
// refused; the tail is seekCompressFrames'.
static int seekCompressFramesResident(zsmi_ctx *c, const void *dSrc, uint64_t srcSize, const uint32_t *dFrameSizes, uint32_t n, uint32_t maxFrameSize,
                                      void *dDst, uint64_t *dArchiveSize, int level, const ResidentDict *dict, int checksumFlag)
{
    if (const int e = c->bind()) return e;
    // device words, 64 bits: raw content offsets [n + 1], cleaned content offsets [n], bounds [n], staging offsets [n + 1], packed offsets
    // [n + 1], the error word; 32 bits: cleaned sizes [n], compressed sizes [n], hashes [n]
    if (!c->seek.dMeta.reserve((5 * (size_t)n + 4) * sizeof(uint64_t) + 3 * (size_t)n * sizeof(uint32_t))) return ZSMI_error_memory_allocation;
    if (!c->seek.dStage.reserve(zs_compress_bound_split(srcSize, n) + 64)) return ZSMI_error_memory_allocation;
    uint64_t *dRawOff = (uint64_t *)c->seek.dMeta.p, *dCleanOff = dRawOff + n + 1, *dBounds = dCleanOff + n, *dStageOff = dBounds + n, *dPacked = dStageOff + n + 1;
    unsigned long long *dErr = (unsigned long long *)(dPacked + n + 1);
    uint32_t *dCleanSizes = (uint32_t *)(dErr + 1), *dSizes = dCleanSizes + n, *dHash = dSizes + n;
    const uint32_t grid = std::max<uint32_t>(1, (n + 255) / 256);
    if (const int e = scanOffsets(c, "k_pack_offsets", dFrameSizes, nullptr, n, 1u, nullptr, dRawOff)) return e;
    if (n) {
        LAUNCH(c, "k_seek_guard", k_seek_guard, dim3(grid), dim3(256), 0, dFrameSizes, (const uint64_t *)dRawOff, n, maxFrameSize, srcSize, dCleanSizes, dCleanOff);
        LAUNCH(c, "k_compress_bounds", k_compress_bounds, dim3(grid), dim3(256), 0, (const uint32_t *)dCleanSizes, n, dBounds);
        if (const int e = scanOffsets(c, "k_pack_offsets", (const uint64_t *)dBounds, nullptr, n, 1u, nullptr, dStageOff)) return e;
        if (const int e = compressBatchResidentImpl(c, dSrc, dCleanOff, dCleanSizes, n, maxFrameSize, c->seek.dStage.p, dStageOff, dSizes, level, dict)) return e;
        if (checksumFlag) LAUNCH(c, "k_seek_hash", k_seek_hash, dim3((n + 15) / 16), dim3(64), 0, (const uint8_t *)dSrc, (const uint64_t *)dCleanOff, (const uint32_t *)dCleanSizes, n, dHash);
    }
    if (const int e = c->fill(dErr, 0xFF, sizeof(*dErr))) return e;
    LAUNCH(c, "k_seek_refuse", k_seek_refuse, dim3(grid), dim3(256), 0, dFrameSizes, (const uint64_t *)dRawOff, n, maxFrameSize, srcSize,
           zs_error_word(ZSMI_error_srcSize_wrong), dSizes, dErr);
    return seekPackArchive(c, dStageOff, dCleanSizes, n, dSizes, dHash, dPacked, dErr, dDst, dArchiveSize, checksumFlag);
}
// the header's checks in its order, then the sequence above.  set: null for the plain form
static int compressSeekableFramesResidentImpl(zsmi_ctx *c, const void *dSrc, uint64_t srcSize, const uint32_t *dFrameSizes, uint32_t n, uint32_t maxFrameSize,
                                              void *dDst, uint64_t dstCapacity, uint64_t *dArchiveSize, int level, int checksumFlag,
                                              const zsmi_cdictSet *set, const uint32_t *dDictIndex)
{
    if (!c) return ZSMI_error_init_missing;
    if (n > kSeekMaxFrames) return ZSMI_error_frameIndex_tooLarge;
    if (n && !dFrameSizes) return ZSMI_error_GENERIC;
    if (maxFrameSize > kSeekMaxFrameSize) return ZSMI_error_parameter_outOfBound;
    ResidentDict dict;
    if (set) { if (const int e = residentCDictSet(c, set, dDictIndex, n, level, dict)) return e; }      // (the set's level; without one: the caller's)
    uint64_t bound;
    if (const int e = seekResidentBound(srcSize, n, checksumFlag, bound)) return e;
    if (dstCapacity < bound) return ZSMI_error_dstSize_tooSmall;
    if (!dArchiveSize || !dDst || (srcSize && !dSrc)) return ZSMI_error_GENERIC;
    return seekCompressFramesResident(c, dSrc, srcSize, dFrameSizes, n, maxFrameSize, dDst, dArchiveSize, level, set ? &dict : nullptr, checksumFlag);
}
extern "C" int zsmi_compressSeekableFramesResident(zsmi_ctx *c, const void *dSrc, uint64_t srcSize, const uint32_t *dFrameSizes, uint32_t n,
                                                   uint32_t maxFrameSize, void *dDst, uint64_t dstCapacity, uint64_t *dArchiveSize, int level, int checksumFlag)
{
    return compressSeekableFramesResidentImpl(c, dSrc, srcSize, dFrameSizes, n, maxFrameSize, dDst, dstCapacity, dArchiveSize, level, checksumFlag, nullptr, nullptr);
}
extern "C" int zsmi_compressSeekableFramesResident_usingCDictSet(zsmi_ctx *c, const void *dSrc, uint64_t srcSize, const uint32_t *dFrameSizes, uint32_t n,
                                                                 uint32_t maxFrameSize, void *dDst, uint64_t dstCapacity, uint64_t *dArchiveSize,
                                                                 int checksumFlag, const zsmi_cdictSet *set, const uint32_t *dDictIndex)
{
    return compressSeekableFramesResidentImpl(c, dSrc, srcSize, dFrameSizes, n, maxFrameSize, dDst, dstCapacity, dArchiveSize, 3, checksumFlag, set, dDictIndex);
}
// host buffers: the device call's checks on the host's arguments, then staged, run, copied back and waited for
static size_t compressSeekableFramesHost(zsmi_ctx *c, void *dst, size_t dstCapacity, const void *src, const uint32_t *frameSizes, uint32_t n,
                                         int level, int checksumFlag, const zsmi_cdictSet *set, const uint32_t *dictIndex)
{
    if (!c) return ZSMI_ERR(ZSMI_error_init_missing);
    uint64_t bound;
    if (const int e = seekFramesBound(frameSizes, n, checksumFlag, bound)) return ZSMI_ERR(e);
    ZsCDictSel sel;
    if (set) { if (const int e = resolveCDictSet(c, set, dictIndex, n, level, sel, true)) return ZSMI_ERR(e); }
    if (dstCapacity < bound) return ZSMI_ERR(ZSMI_error_dstSize_tooSmall);
    uint64_t srcSize = 0;
    for (uint32_t i = 0; i < n; i++) srcSize += frameSizes[i];
    if (!dst || (srcSize && !src)) return ZSMI_ERR(ZSMI_error_GENERIC);
    if (const int e = c->bind()) return ZSMI_ERR(e);
    if (!c->sSrc.reserve(srcSize + 64) || !c->sDst.reserve(bound + 64) || !c->sSizes.reserve(sizeof(uint64_t))) return ZSMI_ERR(ZSMI_error_memory_allocation);
    if (srcSize) if (const int e = c->toDevice(c->sSrc.p, src, srcSize)) return ZSMI_ERR(e);
    if (const int rc = seekCompressFrames(c, c->sSrc.p, frameSizes, n, c->sDst.p, (uint64_t *)c->sSizes.p, level, &sel, checksumFlag, c->checksumFlag)) { (void)c->wait(); return ZSMI_ERR(rc); }
    uint64_t size = 0;
    if (c->toHost(&size, c->sSizes.p, sizeof size) || c->wait()) return ZSMI_ERR(ZSMI_error_GENERIC);
    if (zsmi_isError(size)) return size;
    if (c->toHost(dst, c->sDst.p, size) || c->wait()) return ZSMI_ERR(ZSMI_error_GENERIC);
    return size;
}
extern "C" size_t zsmi_compressSeekableFramesHost(zsmi_ctx *c, void *dst, size_t dstCapacity, const void *src, const uint32_t *frameSizes, uint32_t n,
                                                  int level, int checksumFlag)
{
    return compressSeekableFramesHost(c, dst, dstCapacity, src, frameSizes, n, level, checksumFlag, nullptr, nullptr);
}
extern "C" size_t zsmi_compressSeekableFramesHost_usingCDictSet(zsmi_ctx *c, void *dst, size_t dstCapacity, const void *src, const uint32_t *frameSizes,
                                                                uint32_t n, int checksumFlag, const zsmi_cdictSet *set, const uint32_t *dictIndex)
{
    return compressSeekableFramesHost(c, dst, dstCapacity, src, frameSizes, n, 3, checksumFlag, set, dictIndex);
}
extern "C" int zsmi_compressSeekableDevice(zsmi_ctx *c, const void *dSrc, uint64_t srcSize, void *dDst, uint64_t dstCapacity,
                                           uint64_t *dArchiveSize, int level, uint32_t frameSize, int checksumFlag)
{
    return compressSeekableImpl(c, dSrc, srcSize, dDst, dstCapacity, dArchiveSize, level, frameSize, checksumFlag, c ? c->checksumFlag : 0);
}
extern "C" size_t zsmi_compressSeekable(void *dst, size_t dstCapacity, const void *src, size_t srcSize, int level, uint32_t frameSize, int checksumFlag)
{
    uint64_t F, n;
    if (const int e = seekParams(srcSize, frameSize, F, n)) return ZSMI_ERR(e);
    const uint64_t bound = seekBound(srcSize, F, n, checksumFlag);
    Borrowed b; zsmi_ctx *c = b.c;
    if (!c) return ZSMI_ERR(ZSMI_error_GENERIC);
    if (const int e = c->bind()) return ZSMI_ERR(e);
    if (!c->sSrc.reserve(srcSize + 64) || !c->sDst.reserve(bound + 64) || !c->sSizes.reserve(sizeof(uint64_t))) return ZSMI_ERR(ZSMI_error_memory_allocation);
    if (srcSize) if (const int e = c->toDevice(c->sSrc.p, src, srcSize)) return ZSMI_ERR(e);
    if (const int rc = compressSeekableImpl(c, c->sSrc.p, srcSize, c->sDst.p, bound, (uint64_t *)c->sSizes.p, level, frameSize, checksumFlag, 0)) { (void)c->wait(); return ZSMI_ERR(rc); }
    uint64_t size = 0;
    if (c->toHost(&size, c->sSizes.p, sizeof size) || c->wait()) return ZSMI_ERR(ZSMI_error_GENERIC);
    if (zsmi_isError(size)) return size;
    if (size > dstCapacity) return ZSMI_ERR(ZSMI_error_dstSize_tooSmall);
    if (c->toHost(dst, c->sDst.p, size) || c->wait()) return ZSMI_ERR(ZSMI_error_GENERIC);
    return size;
}

// ---- range reads ----
// the frames that overlap the content range [a, b) (a < b <= content size): first .. last
static void seekSpan(const SeekTable &t, uint64_t a, uint64_t b, uint32_t &first, uint32_t &last)
{
    first = (uint32_t)(std::upper_bound(t.dOff.begin(), t.dOff.end(), a) - t.dOff.begin()) - 1;
    last = (uint32_t)(std::lower_bound(t.dOff.begin(), t.dOff.end(), b) - t.dOff.begin()) - 1;
}
// the table of an archive in device memory: its tail is read back and the stream waited for
static int seekParseDevice(zsmi_ctx *c, const uint8_t *src, uint64_t srcSize, SeekTable &t)
{
    // the archive's tail, once: it holds the whole table up to 256 KiB (16384 entries with checksums: 1 GiB in 64 KiB frames); a larger
    // table is read again at its size
    std::vector<uint8_t> tail(std::min<uint64_t>(srcSize, 256u << 10));
    if (c->toHost(tail.data(), src + srcSize - tail.size(), tail.size()) || c->wait()) return ZSMI_error_GENERIC;
    if (const int e = seekFooter(tail.data() + tail.size() - 9, srcSize, t)) return e;
    if (t.tableSize > tail.size()) {
        tail.resize(t.tableSize);
        if (c->toHost(tail.data(), src + srcSize - t.tableSize, t.tableSize) || c->wait()) return ZSMI_error_GENERIC;
    }
    return seekEntries(tail.data() + tail.size() - t.tableSize, srcSize, t);
}

// A batch of range reads, queued on the context's stream: content [a, b) (b <= content size; a == b: nothing) lands at dDst + to.  Frame i's
// compressed bytes are at dFrames + t.cOff[i] - base.
//   The plan: every range's frames are seekSpan's first .. last; the union of those index sets, in index order, is what the call decodes -
// each frame once, slot s of the union.  A frame that lies wholly inside the one range that overlaps it is OWNED: it decodes straight to its
// place in dDst.  Every other frame of the union (read in part, or by several ranges) decodes into context scratch, those packed back to back,
// and each of its overlaps with a range is a PIECE {scratch offset, dDst offset, length} for k_seek_gather, cut into tiles of kSeekTile.
// That is one decode call for the owned frames and one for the scratch frames, whatever nRanges is.  k_seek_verify leaves a code per slot; a
// range's frames are consecutive slots {firstSlot, count}, which k_seek_range_status reduces to dStatus[r].
//   The call's lists (verify items, pieces, spans) travel through pinned buffers taken in turn (TurnBufs, zsmi_ctx.h), as the decoder's
// item list does (uploadDecodeItems): nothing here waits for the stream.
struct SeekRange { uint64_t a, b, to; };
static int seekReadRanges(zsmi_ctx *c, const SeekTable &t, const uint8_t *dFrames, uint64_t base, const SeekRange *rg, uint32_t nRanges,
                          uint8_t *dDst, uint32_t *dStatus, uint32_t *framesDecoded, const ZsDictSel *dict = nullptr)
{
    if (framesDecoded) *framesDecoded = 0;
    if (nRanges == 0) return 0;
    // the ranges' spans, and their union as runs of consecutive frames {lo, hi} with the slot of lo
    struct Span { uint32_t first, count; };
    struct Run { uint32_t lo, hi, slot0; };
    std::vector<Span> sp(nRanges, Span{ 0, 0 });
    std::vector<uint32_t> order;
    for (uint32_t r = 0; r < nRanges; r++) {
        if (rg[r].a == rg[r].b) continue;
        uint32_t first, last;
        seekSpan(t, rg[r].a, rg[r].b, first, last);
        sp[r] = { first, last - first + 1 };
        order.push_back(r);
    }
    std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return sp[x].first < sp[y].first; });
    std::vector<Run> runs;
    for (const uint32_t r : order) {
        const uint32_t lo = sp[r].first, hi = lo + sp[r].count - 1;
        if (runs.empty() || lo > runs.back().hi + 1) runs.push_back({ lo, hi, 0 });
        else runs.back().hi = std::max(runs.back().hi, hi);
    }
    uint32_t m = 0;
    for (Run &u : runs) { u.slot0 = m; m += u.hi - u.lo + 1; }
    if (framesDecoded) *framesDecoded = m;
    if (m == 0) return c->fill(dStatus, 0, (size_t)nRanges * sizeof(uint32_t));
    auto slotOf = [&](uint32_t i) {
        const Run &u = *(std::upper_bound(runs.begin(), runs.end(), i, [](uint32_t v, const Run &x) { return v < x.lo; }) - 1);
        return u.slot0 + (i - u.lo);
    };
    // how many ranges overlap each slot; the owned slots and their places in dDst
    std::vector<uint32_t> frameOf(m), firstSlot(nRanges, 0);
    std::vector<int32_t> cover((size_t)m + 1, 0);
    for (const Run &u : runs) for (uint32_t i = u.lo; i <= u.hi; i++) frameOf[u.slot0 + (i - u.lo)] = i;
    for (const uint32_t r : order) { firstSlot[r] = slotOf(sp[r].first); cover[firstSlot[r]]++; cover[firstSlot[r] + sp[r].count]--; }
    for (uint32_t s = 1; s < m; s++) cover[s] += cover[s - 1];
    const uint64_t kScratch = ~0ull;
    std::vector<uint64_t> place(m, kScratch);                 // owned: the offset in dDst; the others: then the offset in the scratch
    uint32_t nOwned = 0;
    for (const uint32_t r : order)
        for (uint32_t k = 0; k < sp[r].count; k++) {
            const uint32_t s = firstSlot[r] + k, i = sp[r].first + k;
            if (cover[s] == 1 && t.dOff[i] >= rg[r].a && t.dOff[i + 1] <= rg[r].b) { place[s] = rg[r].to + (t.dOff[i] - rg[r].a); nOwned++; }
        }
    std::vector<uint8_t> owned(m);
    uint64_t scratchBytes = 0;
    for (uint32_t s = 0; s < m; s++) {
        owned[s] = place[s] != kScratch;
        if (!owned[s]) { place[s] = scratchBytes; scratchBytes += t.dSize[frameOf[s]]; }
    }
    // the pieces: short ones first, then the tiles
    std::vector<ZsSeekPiece> small, tiles;
    for (const uint32_t r : order)
        for (uint32_t k = 0; k < sp[r].count; k++) {
            const uint32_t s = firstSlot[r] + k, i = sp[r].first + k;
            if (owned[s]) continue;
            const uint64_t lo = std::max(rg[r].a, t.dOff[i]), hi = std::min(rg[r].b, t.dOff[i + 1]);
            if (hi <= lo) continue;
            const uint64_t from = place[s] + (lo - t.dOff[i]), to = rg[r].to + (lo - rg[r].a), len = hi - lo;
            if (len <= kSeekWavePiece) small.push_back({ from, to, (uint32_t)len, 0 });
            else for (uint64_t at = 0; at < len; at += kSeekTile) tiles.push_back({ from + at, to + at, (uint32_t)std::min<uint64_t>(kSeekTile, len - at), 0 });
        }
    const size_t nPieces = small.size() + tiles.size();
    if (nPieces > 0x7FFFFFFFull) return ZSMI_error_memory_allocation;
    // device words: decoder status [m] (the owned frames' call, then the scratch frames'), codes [m]; (8-aligned) the lists: items, pieces, spans
    const size_t words = (2 * (size_t)m * sizeof(uint32_t) + 7) & ~(size_t)7;
    const size_t listBytes = (size_t)m * sizeof(ZsSeekItem) + nPieces * sizeof(ZsSeekPiece) + (size_t)nRanges * sizeof(ZsSeekSpan);
    ZsSeekItem *hi;
    if (const int e = c->seek.hLists.take(listBytes, hi)) return e;
    if (!c->seek.dMeta.reserve(words + listBytes)) return ZSMI_error_memory_allocation;
    if (m > nOwned && !c->seek.dDec.reserve(scratchBytes + 64)) return ZSMI_error_memory_allocation;
    uint32_t *dSt = (uint32_t *)c->seek.dMeta.p, *dCodes = dSt + m;
    uint8_t *dLists = (uint8_t *)c->seek.dMeta.p + words, *dS = (uint8_t *)c->seek.dDec.p;
    const ZsSeekItem *dItems = (const ZsSeekItem *)dLists;
    const ZsSeekPiece *dPieces = (const ZsSeekPiece *)(dItems + m);
    const ZsSeekSpan *dSpans = (const ZsSeekSpan *)(dPieces + nPieces);
    ZsSeekPiece *hp = (ZsSeekPiece *)(hi + m);
    ZsSeekSpan *hs = (ZsSeekSpan *)(hp + nPieces);
    // the two decode calls' items: the owned frames (status words [0, nOwned)), then the scratch frames ([nOwned, m)), each in index order
    std::vector<uint64_t> so(m), dof(m); std::vector<uint32_t> ss(m), caps(m);
    uint32_t at[2] = { 0, nOwned };
    for (uint32_t s = 0; s < m; s++) {
        const uint32_t i = frameOf[s], j = at[owned[s] ? 0 : 1]++;
        so[j] = t.cOff[i] - base; ss[j] = t.cSize[i]; caps[j] = t.dSize[i]; dof[j] = place[s];
        hi[s] = { (uint64_t)(uintptr_t)((owned[s] ? dDst : dS) + place[s]), t.dSize[i], t.hash[i], j, 0 };
    }
    if (!small.empty()) memcpy(hp, small.data(), small.size() * sizeof(ZsSeekPiece));
    if (!tiles.empty()) memcpy(hp + small.size(), tiles.data(), tiles.size() * sizeof(ZsSeekPiece));
    for (uint32_t r = 0; r < nRanges; r++) hs[r] = { firstSlot[r], sp[r].count };
    if (const int e = c->toDevice(dLists, hi, listBytes)) return e;
    if (const int e = c->seek.hLists.sent(c->stream)) return e;
    if (nOwned)
        if (const int e = decompressBatchDeviceImpl(c, dFrames, so.data(), ss.data(), nOwned, dDst, dof.data(), caps.data(), dSt, dict)) return e;
    if (m > nOwned) {
        if (const int e = decompressBatchDeviceImpl(c, dFrames, so.data() + nOwned, ss.data() + nOwned, m - nOwned, dS, dof.data() + nOwned, caps.data() + nOwned, dSt + nOwned, dict)) return e;
        if (nPieces) LAUNCH(c, "k_seek_gather", k_seek_gather, dim3((uint32_t)((small.size() + 3) / 4 + tiles.size())), dim3(256), 0, (const uint8_t *)dS, dDst, dPieces,
                            (uint32_t)small.size(), (uint32_t)nPieces);
    }
    LAUNCH(c, "k_seek_verify", k_seek_verify, dim3((m + 15) / 16), dim3(64), 0, dItems, m, (const uint32_t *)dSt, t.checksum ? 1 : 0, dCodes, (const uint32_t *)nullptr);
    LAUNCH(c, "k_seek_range_status", k_seek_range_status, dim3((nRanges + 3) / 4), dim3(256), 0, dSpans, nRanges, (const uint32_t *)dCodes, dStatus);
    return c->launched();
}

// ---- opened archives: the table parsed and checked once, the frames' bytes in device memory (the handle's own copy of a host archive, or the
// caller's device archive).  Read-only after creation. ----
struct zsmi_seekable {
    int device = 0;
    SeekTable t;
    const uint8_t *dFrames = nullptr;    // frame i's compressed bytes: dFrames + t.cOff[i]
    void *dOwned = nullptr;              // a host archive's frames (exactly their bytes + 64: no reserve slack on what may be GiBs)
    ZsDictSel sel = ZsDictSel();         // a handle opened with a DDict set: the set's selector (borrowed: the set outlives the handle); else none
    DevBuf dTable;                       // the table in device memory, a ZsSeekEntry a frame (none for an archive without frames): what the reads by device numbers look up
    uint32_t maxDSize = 0;               // the largest Decompressed_Size: the capacity those reads plan their decode for
    const uint64_t *dContent = nullptr;  // t.dOff behind the table's entries in dTable (frames + 1 words): where a run of frames starts and ends in the content (records.hip)
    ~zsmi_seekable() { if (dOwned) (void)hipFree(dOwned); }
};
// queued on the context's stream, from a list that lives until the caller's wait
static int seekUploadTable(zsmi_ctx *c, zsmi_seekable &sk, std::vector<ZsSeekEntry> &entries)
{
    const SeekTable &t = sk.t;
    if (t.n == 0) return 0;
    // (one list, one copy: the entries, then the content offsets in the words behind them - whole entries' room, the last in part)
    const size_t table = sizeof(ZsSeekEntry) * t.n, offsets = sizeof(uint64_t) * ((size_t)t.n + 1);
    entries.resize(t.n + (offsets + sizeof(ZsSeekEntry) - 1) / sizeof(ZsSeekEntry));
    for (uint32_t i = 0; i < t.n; i++) { entries[i] = { t.cOff[i], t.cSize[i], t.dSize[i], t.hash[i], 0 }; sk.maxDSize = std::max(sk.maxDSize, t.dSize[i]); }
    memcpy(entries.data() + t.n, t.dOff.data(), offsets);
    if (!sk.dTable.reserve(table + offsets)) return ZSMI_error_memory_allocation;
    sk.dContent = (const uint64_t *)((const uint8_t *)sk.dTable.p + table);
    return c->toDevice(sk.dTable.p, entries.data(), table + offsets);
}
extern "C" zsmi_seekable *zsmi_openSeekable(zsmi_ctx *c, const void *archive, size_t size, int *err)
{
    return makeHandle<zsmi_seekable>(err, [&](zsmi_seekable &sk) -> int {
        if (const int e = seekParseHost(archive, size, sk.t)) return e;
        if (!c) return ZSMI_error_init_missing;
        sk.device = c->device;
        const uint64_t bytes = sk.t.cOff[sk.t.n];
        if (bytes == 0) return 0;
        if (const int e = c->bind()) return e;
        if (hipMalloc(&sk.dOwned, bytes + 64) != hipSuccess) { (void)hipGetLastError(); sk.dOwned = nullptr; return ZSMI_error_memory_allocation; }
        sk.dFrames = (const uint8_t *)sk.dOwned;
        std::vector<ZsSeekEntry> entries;
        if (const int e = seekUploadTable(c, sk, entries)) { (void)c->wait(); return e; }
        return c->toDevice(sk.dOwned, archive, bytes) || c->wait() ? ZSMI_error_GENERIC : 0;
    });
}
extern "C" zsmi_seekable *zsmi_openSeekableDevice(zsmi_ctx *c, const void *dArchive, uint64_t size, int *err)
{
    return makeHandle<zsmi_seekable>(err, [&](zsmi_seekable &sk) -> int {
        if (!c) return ZSMI_error_init_missing;
        if (!dArchive || size < 9) return ZSMI_error_prefix_unknown;
        if (const int e = c->bind()) return e;
        if (const int e = seekParseDevice(c, (const uint8_t *)dArchive, size, sk.t)) return e;
        sk.device = c->device; sk.dFrames = (const uint8_t *)dArchive;
        // (the table is known only behind the parse's wait: its copy is waited for here, so a read on any context finds it whole)
        std::vector<ZsSeekEntry> entries;
        const int e = seekUploadTable(c, sk, entries);
        const int waited = sk.t.n ? c->wait() : 0;
        return e ? e : waited;
    });
}
// the open calls with a DDict set: the call without one - its checks, in its order - then the set's own check; the handle keeps the set's selector
static zsmi_seekable *seekWithSet(zsmi_ctx *c, zsmi_seekable *sk, const zsmi_ddictSet *set, int *err)
{
    if (!sk || !set) return sk;
    const int e = ddictSetSel(c, set, sk->sel);
    if (!e) return sk;
    delete sk;
    if (err) *err = e;
    return nullptr;
}
extern "C" zsmi_seekable *zsmi_openSeekable_usingDDictSet(zsmi_ctx *c, const void *archive, size_t size, const zsmi_ddictSet *set, int *err)
{
    return seekWithSet(c, zsmi_openSeekable(c, archive, size, err), set, err);
}
extern "C" zsmi_seekable *zsmi_openSeekableDevice_usingDDictSet(zsmi_ctx *c, const void *dArchive, uint64_t size, const zsmi_ddictSet *set, int *err)
{
    return seekWithSet(c, zsmi_openSeekableDevice(c, dArchive, size, err), set, err);
}

// ---- streams of frames that carry no table: the frame index (zsmi_index.h) in place of the table's parse, then the same handle - its
// table without checksums, its device copy through seekUploadTable, its set through seekWithSet; every read above takes it as it is ----
extern "C" size_t zsmi_countFrames(const void *src, size_t srcSize) { return zs_index_count(src, srcSize); }
extern "C" size_t zsmi_buildSeekTable(void *dst, size_t dstCapacity, const void *src, size_t srcSize) { return zs_index_build_table(dst, dstCapacity, src, srcSize); }
static void seekIndexAdd(SeekTable &t, uint32_t cSize, uint32_t dSize)
{
    t.cSize.push_back(cSize); t.dSize.push_back(dSize); t.hash.push_back(0);
    t.cOff.push_back(t.cOff.back() + cSize); t.dOff.push_back(t.dOff.back() + dSize);
    t.n++;
}
static int seekIndexHost(const void *src, size_t size, SeekTable &t)
{
    t.cOff.assign(1, 0); t.dOff.assign(1, 0);
    uint64_t n;
    return zs_index_walk_host((const uint8_t *)src, size, n, [&t](uint64_t, uint32_t c, uint32_t d) { seekIndexAdd(t, c, d); });
}
// The index of a stream in device memory: the launch sequence above the kernels, with the call's two waits - for the candidate count m,
// which sizes everything behind it (exactly m records: no guessed capacity), and for the result.  The tiles' counts and bases lie in the
// context's size staging, the candidates' words in the seekable scratch; the handle keeps neither.
static int seekIndexDevice(zsmi_ctx *c, const uint8_t *src, uint64_t size, SeekTable &t)
{
    t.cOff.assign(1, 0); t.dOff.assign(1, 0);
    if (size == 0) return 0;
    if (!src) return ZSMI_error_srcSize_wrong;
    const uint64_t tiles64 = (size + ZS_INDEX_TILE - 1) / ZS_INDEX_TILE;
    if (tiles64 > 0x7FFFFFFFull) return ZSMI_error_memory_allocation;
    const uint32_t tiles = (uint32_t)tiles64;
    // device words: the tiles' counts [tiles]; (8-aligned) the candidates in front of each tile [tiles + 1]
    const size_t countBytes = ((size_t)tiles * sizeof(uint32_t) + 7) & ~(size_t)7;
    if (!c->sSizes.reserve(countBytes + ((size_t)tiles + 1) * sizeof(uint64_t))) return ZSMI_error_memory_allocation;
    uint32_t *dCounts = (uint32_t *)c->sSizes.p;
    uint64_t *dTileBase = (uint64_t *)((uint8_t *)c->sSizes.p + countBytes);
    LAUNCH(c, "k_index_count", k_index_count, dim3(tiles), dim3(256), 0, src, size, dCounts);
    if (const int e = scanOffsets(c, "k_index_scan", (const uint32_t *)dCounts, nullptr, tiles, 1u, nullptr, dTileBase)) return e;
    uint64_t m64 = 0;
    if (c->toHost(&m64, dTileBase + tiles, sizeof m64) || c->wait()) return ZSMI_error_GENERIC;
    if (m64 == 0) return ZSMI_error_GENERIC;                                              // (offset 0 is always one)
    if (m64 >= kIndexBad) return ZSMI_error_memory_allocation;
    const uint32_t m = (uint32_t)m64, grid = (m + 255) / 256;
    // device words, 64 bits: positions [m], the marked candidates in front of each [m + 1], the head, the entries [m]; 32 bits: status,
    // the two sizes, successors, the two jump arrays, marks [m each]
    if (!c->seek.dMeta.reserve((2 * (size_t)m + 1) * sizeof(uint64_t) + sizeof(ZsIndexHead) + (size_t)m * sizeof(ZsSeekEntry) + 8 * (size_t)m * sizeof(uint32_t)))
        return ZSMI_error_memory_allocation;
    uint64_t *dPos = (uint64_t *)c->seek.dMeta.p, *dSlot = dPos + m;
    ZsIndexHead *dHead = (ZsIndexHead *)(dSlot + m + 1);
    ZsSeekEntry *dEntries = (ZsSeekEntry *)(dHead + 1);
    uint32_t *dStatus = (uint32_t *)(dEntries + m), *dCSize = dStatus + m, *dDSize = dCSize + m, *dNext = dDSize + m, *dJump[2] = { dNext + m, dNext + 2 * (size_t)m }, *dMark = dNext + 3 * (size_t)m;
    LAUNCH(c, "k_index_emit", k_index_emit, dim3(tiles), dim3(256), 0, src, size, (const uint64_t *)dTileBase, dPos, m64);
    LAUNCH(c, "k_index_walk", k_index_walk, dim3(grid), dim3(256), 0, src, size, (const uint64_t *)dPos, m, dStatus, dCSize, dDSize, dNext, dMark);
    const uint32_t *jump = dNext;
    for (uint32_t round = 0; (1ull << round) < m64 + 1; round++) {
        LAUNCH(c, "k_index_jump", k_index_jump, dim3(grid), dim3(256), 0, jump, dJump[round & 1u], dMark, m);
        jump = dJump[round & 1u];
    }
    if (const int e = scanOffsets(c, "k_index_scan", (const uint32_t *)dMark, nullptr, m, 1u, nullptr, dSlot)) return e;
    if (c->fill(dHead, 0, sizeof(ZsIndexHead)) || c->fill(&dHead->err, 0xFF, sizeof(dHead->err))) return ZSMI_error_GENERIC;
    LAUNCH(c, "k_index_table", k_index_table, dim3(grid), dim3(256), 0, (const uint64_t *)dPos, (const uint32_t *)dStatus, (const uint32_t *)dCSize, (const uint32_t *)dDSize,
           (const uint32_t *)dNext, (const uint32_t *)dMark, (const uint64_t *)dSlot, m, size, dHead, dEntries);
    std::vector<uint8_t> back(sizeof(ZsIndexHead) + (size_t)m * sizeof(ZsSeekEntry));
    if (c->launched() || c->toHost(back.data(), dHead, back.size()) || c->wait()) return ZSMI_error_GENERIC;
    ZsIndexHead head;
    memcpy(&head, back.data(), sizeof head);
    if (head.marked > m64 || head.refused > head.marked) return ZSMI_error_GENERIC;
    if (head.marked - head.refused > kSeekMaxFrames) return ZSMI_error_frameIndex_tooLarge;      // (the frames in front of a failure count first: the serial order)
    if (head.err != ~0ull) return (int)(head.err & 0xFFu);
    for (uint64_t i = 0; i < head.marked; i++) {
        ZsSeekEntry e;
        memcpy(&e, back.data() + sizeof head + i * sizeof e, sizeof e);
        if (e.cOff != t.cOff.back()) return ZSMI_error_GENERIC;                             // (a chain that is none: the stream changed under the call)
        seekIndexAdd(t, e.cSize, e.dSize);
    }
    return t.cOff.back() == size ? 0 : ZSMI_error_GENERIC;
}
// zsmi_openFrames judges the stream on the host before it asks for a context, as zsmi_openSeekable its table; the frames' bytes - all of
// the stream - go to device memory the handle owns
extern "C" zsmi_seekable *zsmi_openFrames(zsmi_ctx *c, const void *src, size_t size, int *err)
{
    return makeHandle<zsmi_seekable>(err, [&](zsmi_seekable &sk) -> int {
        if (const int e = seekIndexHost(src, size, sk.t)) return e;
        if (!c) return ZSMI_error_init_missing;
        sk.device = c->device;
        if (size == 0) return 0;
        if (const int e = c->bind()) return e;
        if (hipMalloc(&sk.dOwned, size + 64) != hipSuccess) { (void)c->launched(); sk.dOwned = nullptr; return ZSMI_error_memory_allocation; }
        sk.dFrames = (const uint8_t *)sk.dOwned;
        std::vector<ZsSeekEntry> entries;
        if (const int e = seekUploadTable(c, sk, entries)) { (void)c->wait(); return e; }
        return c->toDevice(sk.dOwned, src, size) || c->wait() ? ZSMI_error_GENERIC : 0;
    });
}
extern "C" zsmi_seekable *zsmi_openFramesDevice(zsmi_ctx *c, const void *dSrc, uint64_t size, int *err)
{
    return makeHandle<zsmi_seekable>(err, [&](zsmi_seekable &sk) -> int {
        if (!c) return ZSMI_error_init_missing;
        if (const int e = c->bind()) return e;
        if (const int e = seekIndexDevice(c, (const uint8_t *)dSrc, size, sk.t)) return e;
        sk.device = c->device; sk.dFrames = (const uint8_t *)dSrc;
        std::vector<ZsSeekEntry> entries;
        const int e = seekUploadTable(c, sk, entries);
        const int waited = sk.t.n ? c->wait() : 0;
        return e ? e : waited;
    });
}
extern "C" zsmi_seekable *zsmi_openFrames_usingDDictSet(zsmi_ctx *c, const void *src, size_t size, const zsmi_ddictSet *set, int *err)
{
    return seekWithSet(c, zsmi_openFrames(c, src, size, err), set, err);
}
extern "C" zsmi_seekable *zsmi_openFramesDevice_usingDDictSet(zsmi_ctx *c, const void *dSrc, uint64_t size, const zsmi_ddictSet *set, int *err)
{
    return seekWithSet(c, zsmi_openFramesDevice(c, dSrc, size, err), set, err);
}
extern "C" void zsmi_closeSeekable(zsmi_seekable *sk) { delete sk; }
extern "C" int zsmi_getFrameInfo_fromSeekable(const zsmi_seekable *sk, uint32_t index, uint64_t *cOffset, uint64_t *dOffset, uint32_t *cSize, uint32_t *dSize)
{
    if (!sk) return ZSMI_error_GENERIC;
    if (index >= sk->t.n) return ZSMI_error_frameIndex_tooLarge;
    if (cOffset) *cOffset = sk->t.cOff[index];
    if (dOffset) *dOffset = sk->t.dOff[index];
    if (cSize) *cSize = sk->t.cSize[index];
    if (dSize) *dSize = sk->t.dSize[index];
    return 0;
}
extern "C" size_t zsmi_getNumFrames_fromSeekable(const zsmi_seekable *sk) { return sk ? sk->t.n : 0; }
extern "C" unsigned long long zsmi_getContentSize_fromSeekable(const zsmi_seekable *sk) { return sk ? sk->t.dOff[sk->t.n] : 0; }
extern "C" size_t zsmi_sizeofSeekable(const zsmi_seekable *sk) { return sk && sk->dOwned ? sk->t.cOff[sk->t.n] : 0; }

// the host checks of a batch read, in the header's order; rg[r]: the range clipped at the content's end (its place in dDst is the caller's to set)
static int seekCheckRanges(const zsmi_ctx *c, const zsmi_seekable *sk, const uint64_t *offsets, const uint64_t *lengths, uint32_t nRanges, const void *a1, const void *a2,
                           std::vector<SeekRange> &rg)
{
    if (!c) return ZSMI_error_init_missing;
    if (!sk || (nRanges && (!offsets || !lengths || !a1 || !a2))) return ZSMI_error_GENERIC;
    if (sk->device != c->device) return ZSMI_error_parameter_unsupported;
    const uint64_t content = sk->t.dOff[sk->t.n];
    rg.resize(nRanges);
    for (uint32_t r = 0; r < nRanges; r++) {
        if (offsets[r] > content) return ZSMI_error_parameter_outOfBound;
        rg[r] = { offsets[r], offsets[r] + std::min(lengths[r], content - offsets[r]), 0 };
    }
    return 0;
}
extern "C" int zsmi_seekableReadRangesDevice(zsmi_ctx *c, const zsmi_seekable *sk, const uint64_t *offsets, const uint64_t *lengths, uint32_t nRanges,
                                             void *dDst, const uint64_t *dstOffsets, uint64_t *written, uint32_t *dStatus, uint32_t *framesDecoded)
{
    std::vector<SeekRange> rg;
    if (const int e = seekCheckRanges(c, sk, offsets, lengths, nRanges, dstOffsets, written, rg)) return e;
    if (nRanges && !dStatus) return ZSMI_error_GENERIC;
    uint64_t bytes = 0;
    for (uint32_t r = 0; r < nRanges; r++) { rg[r].to = dstOffsets[r]; bytes += rg[r].b - rg[r].a; }
    if (bytes && !dDst) return ZSMI_error_GENERIC;
    if (const int e = c->bind()) return e;
    for (uint32_t r = 0; r < nRanges; r++) written[r] = rg[r].b - rg[r].a;
    return seekReadRanges(c, sk->t, sk->dFrames, 0, rg.data(), nRanges, (uint8_t *)dDst, dStatus, framesDecoded, &sk->sel);
}
extern "C" int zsmi_seekableReadRangesHost(zsmi_ctx *c, const zsmi_seekable *sk, const uint64_t *offsets, const uint64_t *lengths, uint32_t nRanges,
                                           void *dst, size_t dstCapacity, uint64_t *written, uint32_t *statuses)
{
    std::vector<SeekRange> rg;
    if (const int e = seekCheckRanges(c, sk, offsets, lengths, nRanges, written, statuses, rg)) return e;
    uint64_t bytes = 0;
    for (uint32_t r = 0; r < nRanges; r++) { rg[r].to = bytes; bytes += rg[r].b - rg[r].a; }
    if (bytes > dstCapacity) return ZSMI_error_dstSize_tooSmall;
    if (bytes && !dst) return ZSMI_error_GENERIC;
    for (uint32_t r = 0; r < nRanges; r++) written[r] = rg[r].b - rg[r].a;
    if (nRanges == 0) return 0;
    if (const int e = c->bind()) return e;
    if (!c->sDst.reserve(bytes + 64) || !c->sSizes.reserve((size_t)nRanges * sizeof(uint32_t))) return ZSMI_error_memory_allocation;
    int rc = seekReadRanges(c, sk->t, sk->dFrames, 0, rg.data(), nRanges, (uint8_t *)c->sDst.p, (uint32_t *)c->sSizes.p, nullptr, &sk->sel);
    if (!rc) rc = c->toHost(statuses, c->sSizes.p, (size_t)nRanges * sizeof(uint32_t));
    if (!rc && bytes) rc = c->toHost(dst, c->sDst.p, bytes);
    const int waited = c->wait(); return rc ? rc : waited;              // (the wait: whatever was queued, a failed call included)
}
// records by number: the read of the frames' extents {content offset, Decompressed_Size}.  The checks the range calls make in front of their
// offsets' check, then the indices; a1, a2: the arrays the range call would refuse as null
static int seekFrameExtents(const zsmi_ctx *c, const zsmi_seekable *sk, const uint32_t *frameIndex, uint32_t nFrames, const void *a1, const void *a2,
                            std::vector<uint64_t> &offsets, std::vector<uint64_t> &lengths)
{
    if (!c) return ZSMI_error_init_missing;
    if (!sk || (nFrames && (!frameIndex || !a1 || !a2))) return ZSMI_error_GENERIC;
    if (sk->device != c->device) return ZSMI_error_parameter_unsupported;
    offsets.resize(nFrames); lengths.resize(nFrames);
    for (uint32_t k = 0; k < nFrames; k++) {
        if (frameIndex[k] >= sk->t.n) return ZSMI_error_frameIndex_tooLarge;
        offsets[k] = sk->t.dOff[frameIndex[k]]; lengths[k] = sk->t.dSize[frameIndex[k]];
    }
    return 0;
}
extern "C" int zsmi_seekableReadFramesDevice(zsmi_ctx *c, const zsmi_seekable *sk, const uint32_t *frameIndex, uint32_t nFrames,
                                             void *dDst, const uint64_t *dstOffsets, uint64_t *written, uint32_t *dStatus, uint32_t *framesDecoded)
{
    std::vector<uint64_t> offsets, lengths;
    if (const int e = seekFrameExtents(c, sk, frameIndex, nFrames, dstOffsets, written, offsets, lengths)) return e;
    return zsmi_seekableReadRangesDevice(c, sk, offsets.data(), lengths.data(), nFrames, dDst, dstOffsets, written, dStatus, framesDecoded);
}
extern "C" int zsmi_seekableReadFramesHost(zsmi_ctx *c, const zsmi_seekable *sk, const uint32_t *frameIndex, uint32_t nFrames,
                                           void *dst, size_t dstCapacity, uint64_t *written, uint32_t *statuses)
{
    std::vector<uint64_t> offsets, lengths;
    if (const int e = seekFrameExtents(c, sk, frameIndex, nFrames, written, statuses, offsets, lengths)) return e;
    return zsmi_seekableReadRangesHost(c, sk, offsets.data(), lengths.data(), nFrames, dst, dstCapacity, written, statuses);
}

// ---- what every read of an opened archive by frame numbers in DEVICE memory is made of: the frame-list decode and the window plan.  Stated
// here once, beside the kernels they drive; records.hip, find.hip and the files built on it (findframes.hip, recindex.hip, filter.hip) call them ----
// The words of a frame-list decode, a frame of F, `p` 8-aligned in the seekable scratch (seekListHead: their bytes): 64 bits - sizes [F],
// places [F + 1]; verify records [F]; 32 bits - the list, decoder status, refusals, written, codes [F each], the call's code [1, padded to
// 8 bytes].  A caller that owns one of these arrays points the word at its own before the call
struct SeekListWords { uint64_t *dSizes, *dListAt; ZsSeekItem *dVerify; uint32_t *dList, *dSt, *dRefused, *dFrameWritten, *dCodes, *dCode; };
static size_t seekListHead(size_t F) { return (2 * F + 1) * sizeof(uint64_t) + F * sizeof(ZsSeekItem) + ((5 * F + 1) * sizeof(uint32_t) + 7) / 8 * 8; }
static SeekListWords seekListWords(void *p, size_t F)
{
    SeekListWords d;
    d.dSizes = (uint64_t *)p; d.dListAt = d.dSizes + F; d.dVerify = (ZsSeekItem *)(d.dListAt + F + 1);
    d.dList = (uint32_t *)(d.dVerify + F); d.dSt = d.dList + F; d.dRefused = d.dSt + F; d.dFrameWritten = d.dRefused + F; d.dCodes = d.dFrameWritten + F; d.dCode = d.dCodes + F;
    return d;
}
// THE FRAME-LIST DECODE.  The F frames dList names (the caller's list, or d.dList, which the caller's kernel wrote), of d.dSizes bytes
// each (k_seek_request_sizes, or the caller's own), into dDst[0, capacity): the layout scan of the sizes under the caller's label and
// alignment leaves their places in d.dListAt [F + 1], k_seek_request_items writes the decode items into the context's item list - which
// holds F items: the caller reserved it, with everything else, before it queued anything - and the verify records, every frame decodes
// straight to its place through the body of zsmi_decompressBatchResident, planned for the table's largest Decompressed_Size, and
// k_seek_verify leaves a code a frame in d.dCodes; d.dFrameWritten: the bytes each frame holds.  A number that names no frame is an empty
// item; a frame named twice is two items, decoded twice.  F == 0: the scan lays d.dListAt[0] and nothing else is queued
static int seekDecodeList(zsmi_ctx *c, const zsmi_seekable *sk, const uint32_t *dList, uint32_t F, const SeekListWords &d, const char *scanName, uint32_t align,
                          void *dDst, uint64_t capacity)
{
    const ZsSeekEntry *dTable = (const ZsSeekEntry *)sk->dTable.p;
    if (const int e = scanOffsets(c, scanName, (const uint64_t *)d.dSizes, nullptr, F, align, nullptr, d.dListAt)) return e;
    if (F == 0) return 0;
    LAUNCH(c, "k_seek_request_items", k_seek_request_items, dim3((F + 255u) / 256u), dim3(256), 0, dTable, sk->t.n, dList, F, (const uint64_t *)d.dListAt, capacity, (uint8_t *)dDst,
           (ZsDecItem *)c->dItems.p, d.dVerify, d.dRefused, d.dFrameWritten);
    CapStats caps;
    caps.add(sk->maxDSize, F);
    if (const int e = decodeItems(c, sk->dFrames, F, dDst, caps, d.dSt, &sk->sel)) return e;
    LAUNCH(c, "k_seek_verify", k_seek_verify, dim3((F + 15) / 16), dim3(64), 0, (const ZsSeekItem *)d.dVerify, F, (const uint32_t *)d.dSt, sk->t.checksum ? 1 : 0, d.dCodes,
           (const uint32_t *)d.dRefused);
    return 0;
}
// the content of frames [firstFrame, firstFrame + frameCount): what a window of them takes in a work buffer, end to end
extern "C" size_t zsmi_seekableFindWorkBound(const zsmi_seekable *sk, uint32_t firstFrame, uint32_t frameCount)
{
    if (!sk || (uint64_t)firstFrame + frameCount > sk->t.n) return 0;
    return (size_t)(sk->t.dOff[(size_t)firstFrame + frameCount] - sk->t.dOff[firstFrame]);
}
// The head of the checks of every call that decodes a window of an archive into a work buffer, in the headers' order: the context, the
// handle and `nulls` - the call's own arrays, one of them null -, the device, ruleCheck() - the call's own rule, the handle known to be
// there -, the window inside the archive, the work buffer (ownWork: a host form, which brings its own)
template <class RuleCheck>
static int seekWindowCheck(const zsmi_ctx *c, const zsmi_seekable *sk, bool nulls, RuleCheck ruleCheck, uint32_t firstFrame, uint32_t frameCount, bool ownWork, const void *work,
                           uint64_t workCapacity)
{
    if (!c) return ZSMI_error_init_missing;
    if (!sk || nulls) return ZSMI_error_GENERIC;
    if (sk->device != c->device) return ZSMI_error_parameter_unsupported;
    if (const int e = ruleCheck()) return e;
    if ((uint64_t)firstFrame + frameCount > sk->t.n) return ZSMI_error_parameter_outOfBound;
    const uint64_t bound = zsmi_seekableFindWorkBound(sk, firstFrame, frameCount);
    if (!ownWork && bound && !work) return ZSMI_error_GENERIC;
    if (!ownWork && workCapacity < bound) return ZSMI_error_dstSize_tooSmall;
    return 0;
}
// THE WINDOW PLAN of the host forms that decode a whole archive through a work buffer of the context's: windows of consecutive frames, in
// ascending order, of at most `limit` bytes of content each, cut wherever the table allows - a longer frame is a window of its own - with
// the most bytes and the most frames a window holds: what the call reserves before the first window is queued
struct SeekWindows { std::vector<std::pair<uint32_t, uint32_t>> list; uint64_t most = 0; uint32_t mostFrames = 0; };      // list: {firstFrame, frameCount}
static SeekWindows seekCutWindows(const zsmi_seekable *sk, uint64_t limit)
{
    SeekWindows w;
    const uint32_t N = sk->t.n;
    for (uint32_t f = 0; f < N;) {
        uint32_t g = f + 1;
        while (g < N && sk->t.dOff[g + 1] - sk->t.dOff[f] <= limit) g++;
        w.list.push_back({ f, g - f });
        w.most = std::max(w.most, sk->t.dOff[g] - sk->t.dOff[f]); w.mostFrames = std::max(w.mostFrames, g - f);
        f = g;
    }
    return w;
}
static uint64_t seekWindowLimit()
{
#ifdef ZSMI_DEBUG_HOOKS
    if (const char *e = getenv("ZSMI_ARCHIVE_WINDOW")) { const long long v = atoll(e); if (v > 0) return (uint64_t)v; }      // the tests' way to many windows over a small archive
#endif
    return 256ull << 20;
}

// records by numbers that are DEVICE memory: nothing is copied to the host, nothing waited for, no pinned buffer touched.  The requests'
// sizes come from the handle's device table (k_seek_request_sizes); the rest is the frame-list decode on the caller's list, with the
// caller's places - the layout scan of zsmi_layoutOutputsDevice - written and status arrays.
extern "C" int zsmi_seekableReadFramesResident(zsmi_ctx *c, const zsmi_seekable *sk, const uint32_t *dFrameIndex, uint32_t nFrames, uint32_t align,
                                               void *dDst, uint64_t dstCapacity, uint64_t *dDstOffsets, uint32_t *dWritten, uint32_t *dStatus)
{
    if (!c) return ZSMI_error_init_missing;
    if (!sk || !dDstOffsets || (nFrames && (!dFrameIndex || !dWritten || !dStatus))) return ZSMI_error_GENERIC;
    if (sk->device != c->device) return ZSMI_error_parameter_unsupported;
    if (align == 0 || align > 4096 || (align & (align - 1))) return ZSMI_error_parameter_outOfBound;
    if (nFrames && dstCapacity && !dDst) return ZSMI_error_GENERIC;
    if (const int e = c->bind()) return e;
    if (!c->seek.dMeta.reserve(seekListHead(nFrames)) || !c->dItems.reserve(sizeof(ZsDecItem) * (size_t)nFrames)) return ZSMI_error_memory_allocation;
    SeekListWords d = seekListWords(c->seek.dMeta.p, nFrames);
    d.dListAt = dDstOffsets; d.dFrameWritten = dWritten; d.dCodes = dStatus;
    if (nFrames) LAUNCH(c, "k_seek_request_sizes", k_seek_request_sizes, dim3((nFrames + 255) / 256), dim3(256), 0, (const ZsSeekEntry *)sk->dTable.p, sk->t.n, dFrameIndex, nFrames, d.dSizes);
    if (const int e = seekDecodeList(c, sk, dFrameIndex, nFrames, d, "k_layout_outputs", align, dDst, dstCapacity)) return e;
    return c->launched();
}

// ---- the single-range calls: the one-range case of seekReadRanges ----
extern "C" int zsmi_decompressSeekableDevice(zsmi_ctx *c, const void *dSrc, uint64_t srcSize, uint64_t offset, uint64_t length,
                                             void *dDst, uint64_t *written, uint32_t *dStatus)
{
    if (!c) return ZSMI_error_init_missing;
    if (!dSrc || srcSize < 9) return ZSMI_error_prefix_unknown;
    if (!dStatus || !written) return ZSMI_error_GENERIC;
    if (const int e = c->bind()) return e;
    SeekTable t;                                                        // (a table for this call alone: an opened archive keeps it)
    if (const int e = seekParseDevice(c, (const uint8_t *)dSrc, srcSize, t)) return e;
    const uint64_t content = t.dOff[t.n];
    if (offset > content) return ZSMI_error_parameter_outOfBound;
    const SeekRange rg = { offset, offset + std::min(length, content - offset), 0 };
    *written = rg.b - rg.a;
    if (rg.b > rg.a && !dDst) return ZSMI_error_GENERIC;
    return seekReadRanges(c, t, (const uint8_t *)dSrc, 0, &rg, 1, (uint8_t *)dDst, dStatus, nullptr);
}
extern "C" size_t zsmi_decompressSeekable(void *dst, size_t dstCapacity, const void *src, size_t srcSize, unsigned long long offset)
{
    SeekTable t;
    if (const int e = seekParseHost(src, srcSize, t)) return ZSMI_ERR(e);
    const uint64_t content = t.dOff[t.n];
    if (offset > content) return ZSMI_ERR(ZSMI_error_parameter_outOfBound);
    const SeekRange rg = { offset, offset + std::min<uint64_t>(dstCapacity, content - offset), 0 };
    if (rg.a == rg.b) return 0;
    uint32_t first, last;
    seekSpan(t, rg.a, rg.b, first, last);
    const uint64_t base = t.cOff[first], span = t.cOff[last + 1] - base;       // only the overlapping frames' bytes go to the device
    Borrowed bw; zsmi_ctx *c = bw.c;
    if (!c) return ZSMI_ERR(ZSMI_error_GENERIC);
    if (const int e = c->bind()) return ZSMI_ERR(e);
    if (!c->sSrc.reserve(span + 64) || !c->sDst.reserve(rg.b - rg.a + 64) || !c->sSizes.reserve(sizeof(uint32_t))) return ZSMI_ERR(ZSMI_error_memory_allocation);
    if (const int e = c->toDevice(c->sSrc.p, (const uint8_t *)src + base, span)) return ZSMI_ERR(e);
    if (const int rc = seekReadRanges(c, t, (const uint8_t *)c->sSrc.p, base, &rg, 1, (uint8_t *)c->sDst.p, (uint32_t *)c->sSizes.p, nullptr)) { (void)c->wait(); return ZSMI_ERR(rc); }
    uint32_t status = 0;
    if (c->toHost(&status, c->sSizes.p, sizeof status) || c->wait()) return ZSMI_ERR(ZSMI_error_GENERIC);
    if (status) return ZSMI_ERR(status);
    if (c->toHost(dst, c->sDst.p, rg.b - rg.a) || c->wait()) return ZSMI_ERR(ZSMI_error_GENERIC);
    return rg.b - rg.a;
}
