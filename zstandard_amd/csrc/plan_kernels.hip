// The compress plan built ON THE DEVICE (zsmi_compressBatchResident and its dictionary form, _usingCDictSet): the chunk, block and unit
// lists the encoder kernels read, written from offsets, sizes and dictionary indices that are device memory.  The host knows one number,
// maxSrcSize, hence nbMax = the blocks of a chunk of that size; it cuts the call into sub-batches of K chunks each (K * nbMax blocks at
// most: they fit the scratch whatever the sizes turn out to be) and launches every kernel over an upper bound of its work.  The kernels
// here write, per sub-batch, lists that are compact - live entries in front, in the host plan's order - and the live counts; the encoder
// kernels leave at once when their index is at or beyond the count.
//   k_plan_chunks   a workgroup a sub-batch, ONE launch a call: sizes -> zs_chunk_counts (zsmi_plan.h) -> the running sums of blocks, small
//                   units and big units in front of every chunk of the sub-batch -> ZsChunkDesc (firstBlock counts from the sub-batch's
//                   first block: block numbering restarts at 0), the unit sums (ZsPlanBefore), the totals (ZsPlanCounts).
//                   DICT (a set call): the chunk's index -> its record's hasDict -> zs_chunk_counts_dict, a fourth running sum (prefixed
//                   units), and the SANITISED record index a chunk (chunkDict, what the entropy kernels read: ZS_DICT_NONE for no
//                   dictionary, an empty member or a refused chunk)
//   k_plan_blocks   a thread a block slot, a launch a sub-batch (into lists every sub-batch reuses, behind the one before on the stream):
//                   the chunk that owns the block by a search over firstBlock, then ZsBlockDesc, and from a unit's first block its ZsUnitDesc
//                   - a set call's prefixed unit into the prefixed list, with its record index at the same place of unitDict
//   k_plan_refuse   a thread a chunk, last on the stream: the size word of a chunk above maxSrcSize becomes the refusal (srcSize_wrong), that
//                   of a chunk whose index names no member parameter_outOfBound (the size's refusal first).  Such a chunk is
//                   planned as an EMPTY one without a record - one block, no unit, an empty frame at its place - so no list, grid, scratch
//                   or record lookup sees its size or its index
#pragma once
#include "zsmi_device.h"
#include "zsmi_wave.h"
#include "zsmi_plan.h"
static_assert(ZS_PLAN_BLOCK == ZS_BLOCK_MAX && ZS_PLAN_UNIT == ZS_UNIT_MAX, "zsmi_plan.h cuts chunks into the kernels' blocks and units");

struct ZsPlanCounts { uint32_t blocks, smallUnits, bigUnits, pfxUnits; };  // live entries of a sub-batch's lists (a kernel's liveCount points at one word)
struct ZsPlanBefore { uint32_t smallUnits, bigUnits, pfxUnits; };          // units of the sub-batch in front of a chunk's, by kind (small: a set call's tail list)
// the unit list holds [prefixed][small][big] at bases the host knows (the plain call: no prefixed part); unitDict: the record index of
// every prefixed unit, in list order (null: the plain call)
struct ZsPlanLists { ZsBlockDesc *blocks; ZsUnitDesc *units; uint32_t pfxBase, smallBase, bigBase; uint32_t *unitDict; };
// where a chunk's unit goes in the sub-batch's unit list; prefixed: zs_chunk_prefixed of the chunk
__device__ __forceinline__ uint32_t zs_plan_unit_slot(const ZsPlanLists &l, const ZsPlanBefore &before, const ZsChunkUnit &u, bool prefixed)
{
    return u.big ? l.bigBase + before.bigUnits + u.at : (prefixed ? l.pfxBase + before.pfxUnits : l.smallBase + before.smallUnits) + u.at;
}
// the size a chunk is planned with: its own, or 0 where it is above what the host was told
__device__ __forceinline__ uint32_t zs_plan_size(uint32_t size, uint32_t maxSrcSize) { return size > maxSrcSize ? 0u : size; }
// an index that names neither "no dictionary" nor a member of the set: the chunk is refused (k_plan_chunks plans it empty, k_plan_refuse says so)
__device__ __forceinline__ bool zs_plan_index_refused(uint32_t index, uint32_t members) { return index != ZS_DICT_NONE && index >= members; }

#define ZS_PLAN_THREADS 1024u
// the sum of v over the workgroup's threads in front of this one; total: over all.  waveSums: a word a wavefront (LDS).  (The caller
// keeps the calls apart with a barrier of its own before waveSums is written again.)
__device__ __forceinline__ uint32_t zs_plan_excl_scan(uint32_t v, uint32_t *waveSums, uint32_t &total)
{
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t incl = wave_incl_scan(v);
    if (lane == 63) waveSums[wave] = incl;
    __syncthreads();
    uint32_t pre = 0, all = 0;
    for (uint32_t w = 0; w < ZS_PLAN_THREADS / 64; w++) { const uint32_t s = waveSums[w]; all += s; if (w < wave) pre += s; }      // (the same LDS words for a wavefront: broadcast reads)
    total = all;
    return pre + incl - v;
}
// DICT: the set call.  dictIndex (n entries; null: every chunk names member 0 - the host has seen to it that the set has exactly one),
// dictTab, members: the set's records; chunkDict (n entries): written.  Without DICT none of the four is read or written: the plain
// call's kernel is the one it was
template <bool DICT>
__global__ void __launch_bounds__(ZS_PLAN_THREADS)
k_plan_chunks(const uint64_t *__restrict__ srcOffsets, const uint32_t *__restrict__ srcSizes, const uint64_t *__restrict__ dstOffsets,
              uint32_t n, uint32_t K, uint32_t maxSrcSize, ZsChunkDesc *__restrict__ chunks, ZsPlanBefore *__restrict__ before,
              ZsPlanCounts *__restrict__ counts, const uint32_t *__restrict__ dictIndex, const ZsCDictEntry *__restrict__ dictTab,
              uint32_t members, uint32_t *__restrict__ chunkDict)
{
    __shared__ uint32_t waveSums[4][ZS_PLAN_THREADS / 64];
    const uint32_t sub = blockIdx.x, tid = threadIdx.x;
    const uint32_t c0 = sub * K, c1 = min(n, c0 + K);                      // (the host launches ceil(n / K) workgroups: c0 < n)
    uint32_t runBlocks = 0, runSmall = 0, runBig = 0, runPfx = 0;          // of the chunks in front of this tile: the same in every thread
    // a thread a chunk, a tile of ZS_PLAN_THREADS chunks a turn.  (8 consecutive chunks a thread - fewer scans - was measured slower: 0.028 ms
    // against 0.015 at 4096 chunks, 0.060 against 0.038 at 2 x 16384: a thread's loads and stores in a row cost more than the barriers saved.)
    for (uint32_t base = c0; base < c1; base += ZS_PLAN_THREADS) {
        const uint32_t i = base + tid;
        const bool mine = i < c1;
        uint32_t size = mine ? zs_plan_size(srcSizes[i], maxSrcSize) : 0u;
        uint32_t record = ZS_DICT_NONE;                                    // the record the chunk is compressed with
        if constexpr (DICT) {
            if (mine) {
                const uint32_t e = dictIndex ? dictIndex[i] : 0u;
                if (zs_plan_index_refused(e, members)) size = 0;           // (an EMPTY chunk without a record, as one above maxSrcSize)
                else if (e != ZS_DICT_NONE && srcSizes[i] <= maxSrcSize && dictTab[e].hasDict) record = e;
            }
        }
        const ZsChunkDictCounts cc = zs_chunk_counts_dict(size, record != ZS_DICT_NONE);      // (without DICT: zs_chunk_counts, no prefixed unit)
        uint32_t tBlocks, tSmall, tBig, tPfx = 0, p0 = 0;
        const uint32_t b0 = runBlocks + zs_plan_excl_scan(mine ? cc.blocks : 0u, waveSums[0], tBlocks);      // (no chunk: not even the empty chunk's block)
        const uint32_t s0 = runSmall + zs_plan_excl_scan(cc.tailUnits, waveSums[1], tSmall);
        const uint32_t g0 = runBig + zs_plan_excl_scan(cc.bigUnits, waveSums[2], tBig);
        if constexpr (DICT) p0 = runPfx + zs_plan_excl_scan(cc.pfxUnits, waveSums[3], tPfx);
        if (mine) {
            ZsChunkDesc cd;
            cd.srcOff = srcOffsets[i]; cd.dstOff = dstOffsets[i]; cd.size = size; cd.firstBlock = b0; cd.nBlocks = cc.blocks; cd.pad = 0;
            chunks[i] = cd;
            ZsPlanBefore pb; pb.smallUnits = s0; pb.bigUnits = g0; pb.pfxUnits = p0;
            before[i] = pb;
            if constexpr (DICT) chunkDict[i] = record;
        }
        runBlocks += tBlocks; runSmall += tSmall; runBig += tBig; runPfx += tPfx;
        __syncthreads();                                                   // every thread has read the wavefront sums: the next tile may write them
    }
    if (tid == 0) { ZsPlanCounts pc; pc.blocks = runBlocks; pc.smallUnits = runSmall; pc.bigUnits = runBig; pc.pfxUnits = runPfx; counts[sub] = pc; }
}
// chunks, before, chunkDict: the sub-batch's (its first chunk's at [0]); nChunks of them; chunkBase: that chunk's index in the call, which
// the blocks name.  chunkDict: k_plan_chunks' record index a chunk (null: the plain call - no chunk has a dictionary)
__global__ void __launch_bounds__(256)
k_plan_blocks(const ZsChunkDesc *__restrict__ chunks, const ZsPlanBefore *__restrict__ before, const ZsPlanCounts *__restrict__ counts,
              uint32_t nChunks, uint32_t chunkBase, ZsPlanLists lists, const uint32_t *__restrict__ chunkDict)
{
    const uint32_t live = counts->blocks;                                  // (one address a workgroup: a scalar load)
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= live) return;
    // the last chunk whose first block is at or in front of block j (chunk 0's is block 0; every chunk has a block: firstBlock ascends strictly)
    uint32_t lo = 0, hi = nChunks;
    while (hi - lo > 1) { const uint32_t mid = lo + ((hi - lo) >> 1); if (chunks[mid].firstBlock <= j) lo = mid; else hi = mid; }
    const ZsChunkDesc cd = chunks[lo];
    const uint32_t k = j - cd.firstBlock;
    const ZsChunkBlock cb = zs_chunk_block(cd.size, k, cd.nBlocks);
    ZsBlockDesc bd;
    bd.srcOff = cd.srcOff + cb.off; bd.size = cb.size; bd.chunk = chunkBase + lo; bd.firstInChunk = cb.first; bd.lastInChunk = cb.last;
    lists.blocks[j] = bd;
    if (cd.size && !(k & 1u)) {                                            // a unit's first block writes the unit
        const ZsChunkUnit cu = zs_chunk_unit(cd.size, k >> 1);
        ZsUnitDesc ud;
        ud.srcOff = cd.srcOff + cu.off; ud.size = cu.size; ud.firstBlock = cd.firstBlock + cu.block;
        const ZsPlanBefore pb = before[lo];
        const uint32_t record = chunkDict ? chunkDict[lo] : ZS_DICT_NONE;  // (a record here stands for a dictionary: k_plan_chunks kept no other)
        const bool prefixed = zs_chunk_prefixed(cd.size, record != ZS_DICT_NONE);
        lists.units[zs_plan_unit_slot(lists, pb, cu, prefixed)] = ud;
        if (prefixed) lists.unitDict[pb.pfxUnits] = record;                // (the prefixed list starts at unitDict[0], whatever pfxBase is)
    }
}
// dictIndex, members: a set call's choice (null: no index to refuse - the plain call, or a set of one member that every chunk uses)
__global__ void __launch_bounds__(256)
k_plan_refuse(const uint32_t *__restrict__ srcSizes, uint32_t n, uint32_t maxSrcSize, uint32_t refusal, uint32_t *__restrict__ dstSizes,
              const uint32_t *__restrict__ dictIndex, uint32_t members, uint32_t indexRefusal)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    if (srcSizes[i] > maxSrcSize) dstSizes[i] = refusal;
    else if (dictIndex && zs_plan_index_refused(dictIndex[i], members)) dstSizes[i] = indexRefusal;
}
// zsmi_compressBoundsDevice: zs_compress_bound over n sizes
__global__ void __launch_bounds__(256)
k_compress_bounds(const uint32_t *__restrict__ srcSizes, uint32_t n, uint64_t *__restrict__ bounds)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) bounds[i] = zs_compress_bound(srcSizes[i]);
}
