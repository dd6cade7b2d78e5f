// The compress plan's rule for ONE chunk, stated once: how many 64 KiB blocks and LZ units its size gives, and what block k and unit u of
// it are.  CompressPlan::build (zsmi_api.hip: the host-array calls) and k_plan_chunks / k_plan_blocks (plan_kernels.hip: the resident
// calls, plain and with a CDict set) both plan with these functions, so the two paths cannot cut a chunk differently.  Plain C++ with nothing but <stdint.h> behind it:
// a host program may include this header alone (tests/test_resident_compress_host.py does).
//   blocks: every 64 KiB of the chunk; an EMPTY chunk is one block (its frame carries one empty block) and no unit
//   units:  every 128 KiB of the chunk (two blocks: a match window); a unit with more than 64 KiB LEFT is big (the big-unit kernels), else
//           small - so a chunk has at most one small unit, its last, and every unit in front of it is big
//   dictionary calls ("Dictionary prefix"): a chunk of 1 .. 64 KiB whose record stands for a dictionary is one PREFIXED unit
//           (the kernels with PFX: its matches may reach into the dictionary); every other small unit - the tail of a longer chunk, the
//           unit of a chunk without a dictionary or with an empty member's record - goes to the TAIL list, parsed as without a dictionary;
//           big units are unchanged.  zs_chunk_prefixed says which, zs_chunk_counts_dict counts by it
#pragma once
#include <stdint.h>
#if defined(__HIPCC__)
#define ZS_PLAN_FN __host__ __device__ __forceinline__
#else
#define ZS_PLAN_FN static inline
#endif
#define ZS_PLAN_BLOCK 65536u      // = ZS_BLOCK_MAX, ZS_UNIT_MAX (zsmi_device.h; plan_kernels.hip holds them against each other)
#define ZS_PLAN_UNIT  131072u

struct ZsChunkCounts { uint32_t blocks, smallUnits, bigUnits; };
ZS_PLAN_FN ZsChunkCounts zs_chunk_counts(uint32_t size)
{
    ZsChunkCounts c;
    c.blocks = size ? (uint32_t)(((uint64_t)size + ZS_PLAN_BLOCK - 1) / ZS_PLAN_BLOCK) : 1u;
    const uint32_t units = (uint32_t)(((uint64_t)size + ZS_PLAN_UNIT - 1) / ZS_PLAN_UNIT);
    c.smallUnits = (size && size - (units - 1) * ZS_PLAN_UNIT <= ZS_PLAN_BLOCK) ? 1u : 0u;
    c.bigUnits = units - c.smallUnits;
    return c;
}
// dict: the chunk's record stands for a dictionary (ZsCDictEntry::hasDict of the record the chunk picked; false for ZS_DICT_NONE)
ZS_PLAN_FN bool zs_chunk_prefixed(uint32_t size, bool dict) { return dict && size && size <= ZS_PLAN_BLOCK; }
struct ZsChunkDictCounts { uint32_t blocks, pfxUnits, tailUnits, bigUnits; };
ZS_PLAN_FN ZsChunkDictCounts zs_chunk_counts_dict(uint32_t size, bool dict)
{
    const ZsChunkCounts c = zs_chunk_counts(size);
    ZsChunkDictCounts d;
    d.blocks = c.blocks; d.bigUnits = c.bigUnits;
    d.pfxUnits = zs_chunk_prefixed(size, dict) ? c.smallUnits : 0u;       // (such a chunk's one small unit is the chunk)
    d.tailUnits = c.smallUnits - d.pfxUnits;
    return d;
}
// block k (< blocks) of a chunk: where it starts in the chunk, its bytes, whether it is the chunk's first / last
struct ZsChunkBlock { uint64_t off; uint32_t size, first, last; };
ZS_PLAN_FN ZsChunkBlock zs_chunk_block(uint32_t size, uint32_t k, uint32_t blocks)
{
    ZsChunkBlock b;
    b.off = (uint64_t)k * ZS_PLAN_BLOCK;
    const uint64_t left = (uint64_t)size - b.off;
    b.size = (uint32_t)(left < ZS_PLAN_BLOCK ? left : ZS_PLAN_BLOCK);
    b.first = k == 0; b.last = k + 1 == blocks;
    return b;
}
// unit u (< smallUnits + bigUnits) of a chunk: where it starts in the chunk, its bytes, its first block among the chunk's, whether it is
// big, and its place among the chunk's units of its kind (in chunk order: a big unit's is u, the small unit's 0)
struct ZsChunkUnit { uint64_t off; uint32_t size, block, big, at; };
ZS_PLAN_FN ZsChunkUnit zs_chunk_unit(uint32_t size, uint32_t u)
{
    ZsChunkUnit r;
    r.off = (uint64_t)u * ZS_PLAN_UNIT;
    const uint64_t left = (uint64_t)size - r.off;
    r.size = (uint32_t)(left < ZS_PLAN_UNIT ? left : ZS_PLAN_UNIT);
    r.block = 2u * u;
    r.big = left > ZS_PLAN_BLOCK;
    r.at = r.big ? u : 0u;
    return r;
}
