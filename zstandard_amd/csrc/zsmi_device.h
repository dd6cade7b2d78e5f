// Shared definitions for the HIP kernels of the MI355X Zstandard block codec (gfx950 only).
// Format constants follow the reference decoder: csharp/src/ZStdInternal.cs:109-198, ZStd.cs:386-416.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define ZS_BLOCK_MAX   65536u     // bytes per block; block positions fit 16 bits
#define ZS_UNIT_MAX    131072u    // bytes per LZ unit (match window): two consecutive blocks of a chunk
#define ZS_TABLE_LOG_SMALL 13     // slots of each candidate table, units <= 64 KiB
#define ZS_TABLE_LOG_BIG   14     // units <= 128 KiB
#define ZS_WALK_LOG_MIN 8         // the walk cuts a block in ranges of 256 bytes (512 at levels <= 2: the launch says which)
#define ZS_RES_PER_BLOCK 256u     // walk-range results per block (ranges of >= 256 bytes)
#ifndef ZS_CROSS_MAX
#define ZS_CROSS_MAX   1024u      // a match may pass its walk range's end by this much (never the block's end)
#endif
#define ZS_MATCHLESS_SHIFT 11      // a unit with fewer than n >> 11 candidate positions is not parsed (oracle: MATCHLESS_SHIFT)
#define ZS_MINMATCH    5u         // shortest match kept
#define ZS_REPMIN      4u         // shortest match at one of the walker's two recent offsets
#define ZS_WINDOW      32u        // positions looked at per walk step
#define ZS_FCAP        8u         // forward bytes compared when scoring a candidate (the match taken is measured to its end)
#define ZS_BCAP        4u         // backward bytes compared when scoring a candidate
#define ZS_SEQ_MAX     (ZS_BLOCK_MAX / 4u)    // most sequences a block can hold: its matches do not overlap and are >= 4 bytes long
#define ZS_HUF_MAXBITS 11u

// one 64 KiB block of one chunk
struct ZsBlockDesc {
    uint64_t srcOff;      // byte offset of the block in the source arena
    uint32_t size;        // 0..65536
    uint32_t chunk;       // owning chunk (frame)
    uint32_t firstInChunk;
    uint32_t lastInChunk;
};

// one LZ unit: blocks firstBlock, firstBlock + 1 (if size > 64 KiB) of one chunk
struct ZsUnitDesc {
    uint64_t srcOff;      // byte offset of the unit in the source arena
    uint32_t size;        // 1..131072
    uint32_t firstBlock;  // index of its first block in the call's block list
};

// one sequence as the stitch leaves it in a block's list / as the entropy kernels consume it: two 32-bit words
//   x: bits 0-10 unused (zero), bits 11-27 match length (<= 65536: matches found piecewise are joined), bit 28 bit 16 of the offset
//   y: bits 0-15 low 16 bits of the offset, bits 16-31 block position of the match start
// A record carries no literal length: the literals in front of a match run from the end of the record before it (start + match length;
// 0 for a block's first record) to its start, however long that run is.
struct ZsSeqRec { uint32_t x, y; };
__device__ __forceinline__ uint32_t zs_rec_ml(uint32_t x) { return (x >> 11) & 0x1FFFFu; }
__device__ __forceinline__ uint32_t zs_rec_off(uint32_t x, uint32_t y) { return (y & 0xFFFFu) | (((x >> 28) & 1u) << 16); }
__device__ __forceinline__ uint32_t zs_rec_pos(uint32_t y) { return y >> 16; }
__device__ __forceinline__ uint32_t zs_rec_x(uint32_t ml, uint32_t off) { return (ml << 11) | ((off >> 16) << 28); }
__device__ __forceinline__ uint32_t zs_rec_y(uint32_t off, uint32_t pos) { return (off & 0xFFFFu) | (pos << 16); }

// a block after the stitch: records [0, nseq) of its list count, in block order; trailing: literal bytes behind the last match (the whole
// block if there is none); lits: all its literal bytes (the bytes no match covers)
struct ZsBlockHdr { uint32_t nseq, trailing, lits, pad; };

// per-block result of the encode kernel
struct ZsBlockResult { uint32_t payloadSize; uint32_t type; /* 0 raw, 1 rle, 2 compressed */ uint32_t rleByte; uint32_t pad; };

// What the dictionary loader (loadDictEntropy, decode_kernels.hip) found in a dictionary's bytes, as k_dict_load (decode_fast.hip) leaves
// it in device memory for the host: the verdict and the header fields, and a formatted dictionary's entropy section as the decoder reads it,
// which k_cdict_tables (entropy_kernels.hip) turns into encoder tables.
struct ZsCDictEntropy {
    uint8_t weights[256]; uint32_t nWeights, hufLog;           // Huffman weights, the implied last one included
    int16_t norm[3][64]; uint32_t maxSym[3], tableLog[3];      // normalised counts of LL, OF, ML (-1: low probability)
};
struct ZsDictRecord {
    uint32_t status;                 // 0, or 30 (dictionary_corrupted): nothing else is valid then
    uint32_t dictID, contentOff;     // raw content: 0, 0
    uint32_t rep[3];
    ZsCDictEntropy ent;              // contentOff != 0 only
};

// One compression dictionary as the encoder kernels take it: a record of a read-only device table (a zsmi_cdict's own one-entry table, a
// _usingDict call's, a zsmi_cdictSet's with one record a member).  A kernel gets the table and an index array (null: every chunk uses
// record 0; an entry of ZS_DICT_NONE: that chunk has no dictionary) and reads its record once, by a wave-uniform address.
//   pre, pfx: the content's last <= 64 KiB, where a prefixed unit's matches may reach; img: k_lz_dict_tables' candidate-table images of it
//   tables:   a formatted digested dictionary's entropy tables in encoder form, else null
//   rep, dictID: the recent offsets a frame's first block starts from and the ID its header carries ({1, 4, 8} and 0 for raw content)
//   hasDict:  1: the record stands for a dictionary; 0: an empty member of a set (all zeros) - its chunks have none.  The plan reads it
//             (zs_chunk_prefixed, zsmi_plan.h): on the host as zsmi_cdictSet::hasDict says the same, on the device from here
#define ZS_DICT_NONE 0xFFFFFFFFu
struct ZsCDictTables;
struct ZsCDictEntry {
    const uint8_t *pre; const uint32_t *img; const ZsCDictTables *tables;
    uint32_t pfx, dictID, rep[3], hasDict;
};

// zsmi_compressBound: the most a frame of srcSize content bytes takes, header, every block raw and the content checksum included.  Stated
// here because k_frame_checksum holds a frame's size against it before it writes behind the frame
__host__ __device__ __forceinline__ uint64_t zs_compress_bound(uint64_t srcSize)
{
    return srcSize + (srcSize >> 8) + ((srcSize < (128u << 10)) ? (((128u << 10) - srcSize) >> 11) : 0) + 3 * (srcSize / ZS_BLOCK_MAX + 1) + 18;
}
// Room for the frames of EVERY split of at most srcSize content bytes into n chunks s_0 .. s_{n-1}: an upper bound of sum_i zs_compress_bound(s_i),
// for whoever knows the sum and the count but not the sizes (the resident record archives: zsmi_seekableFramesResidentBound and the staging
// behind it).  Term by term over the function above, with S = sum_i s_i <= srcSize:
//   sum s_i = S;  sum (s_i >> 8) <= S >> 8;  the small-chunk term is at most (128 KiB) >> 11 = 64 a chunk;
//   sum 3 * (s_i / 64 KiB + 1) <= 3 * (S >> 16) + 3 n;  18 a chunk
// and every term grows with S, so srcSize stands for any smaller sum
__host__ __device__ __forceinline__ uint64_t zs_compress_bound_split(uint64_t srcSize, uint64_t n)
{
    return srcSize + (srcSize >> 8) + 3 * (srcSize / ZS_BLOCK_MAX) + n * (64 + 3 + 18);
}

// unaligned little-endian loads.  memcpy keeps the alignment-1 fact visible to the compiler: a cast to an over-aligned
// pointer lets it turn a wave-uniform address into a scalar load, which drops the low address bits.  (Host code reads
// container headers with the same loads: the host is little-endian too.)
__host__ __device__ __forceinline__ uint32_t zs_load32(const uint8_t *p) { uint32_t v; __builtin_memcpy(&v, p, 4); return v; }
__host__ __device__ __forceinline__ uint64_t zs_load64(const uint8_t *p) { uint64_t v; __builtin_memcpy(&v, p, 8); return v; }
// unaligned stores (global memory takes them at any byte address)
__device__ __forceinline__ void zs_store16(uint8_t *p, uint16_t v) { __builtin_memcpy(p, &v, 2); }
__device__ __forceinline__ void zs_store32(uint8_t *p, uint32_t v) { __builtin_memcpy(p, &v, 4); }
__device__ __forceinline__ void zs_store64(uint8_t *p, uint64_t v) { __builtin_memcpy(p, &v, 8); }
__device__ __forceinline__ uint32_t zs_highbit(uint32_t v) { return 31u - (uint32_t)__builtin_clz(v); }
__device__ __forceinline__ int zs_lane() { return (int)(threadIdx.x & 63u); }
