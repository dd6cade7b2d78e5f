// Entropy stage of the block encoder: the sequences left by k_lz_walk become one Zstandard compressed block per 64 KiB block.
//   k_encode_sequences  (4 blocks = 4 wavefronts per workgroup)  -> sequences section: recent-offset codes, histograms, FSE tables, bitstream
//   k_encode_literals   (1 block, 4 wavefronts per workgroup)    -> literals section: gather, Huffman lengths / codes / description / streams;
//                                                                    writes the frame of a one-block chunk as its workgroup finishes
//   k_assemble_frames   (1 chunk per workgroup)                  -> frames of chunks of several blocks
//   k_frame_checksum    (1 chunk per quad, 16 per workgroup)     -> checksumFlag: the Content_Checksum behind every frame of a call, once they are final
//   k_train_stats       (1 block per workgroup)                  -> the dictionary trainer's finalize: counts of what the sequences kernel coded
//   k_cdict_tables      (one workgroup)                          -> a digested dictionary's entropy tables in encoder form (ZsCDictTables)
//   k_pack_tile_sums, k_pack_scan_tiles, k_pack_offsets, k_pack_copy                                  -> frames in bound-sized slots packed back to back
// k_encode_sequences and k_encode_literals are templates on CD alone (a record's entropy tables may code a frame's first block); every
// form takes a frame's recent offsets / ID from its chunk's dictionary record ({1, 4, 8} / 0 without one).  Every FSE encoding table - a block's, a predefined one, the
// Huffman weights', a digested dictionary's - is built by buildCTableWave over the shared builder of zsmi_fse.h, which also holds the
// alphabets' constants.  Scalar statement of the same algorithm: oracle/zso_encoder.c (compressBlock and below); the two
// must agree bit for bit.  Every piece is the format-inverse of a function of the reference decoder:
//   literals section        <-> DecodeLiteralsBlock            csharp/src/ZStdDecompress.cs:683-821
//   Huffman table / streams <-> ReadStats, HUF_readDTableX2,   EntropyCommon.cs:198-269, HufDecompress.cs:117-358
//   sequences header/tables <-> DecodeSeqHeaders, BuildFSETable ZStdDecompress.cs:958-1180, EntropyCommon.cs:79-188
//   sequences bitstream     <-> DecodeSequence, decompressSequences_body  ZStdDecompress.cs:1473-1608
#ifndef ZSMI_ENTROPY_KERNELS_HIP        // (dict_train.hip and seekable.hip include this file too)
#define ZSMI_ENTROPY_KERNELS_HIP
#include "zsmi_device.h"
#include "zsmi_status.h"          // the size word a frame leaves: zs_word_is_error, zs_word_bytes
#include "zsmi_scratch.h"         // the scratch slots of a block (its list of records, its header, literals, streams, sections, meta: ZsBlockMeta) and what the sequences kernel borrows
#include "zsmi_wave.h"
#include "zsmi_fse.h"            // the alphabets' constants, FseBuild, the table builder's two routines
// timing aids of the development tools (tools/time_kernels.py): end a kernel after a stage.  Compiled in only with
// -DZSMI_DEBUG_HOOKS (the library the product ships ignores the stopAt argument).
#ifdef ZSMI_DEBUG_HOOKS
#define ZS_STOP_AT(v) (stopAt == (v))
#define ZS_STOPPED (stopAt != 0)     // a stopped kernel writes no frame (its stage time is what is asked for)
#else
#define ZS_STOP_AT(v) false
#define ZS_STOPPED false
#endif

// Codes and extra bits by arithmetic: the values of the format's tables (LL_Code / ML_Code of ZStdInternal.cs:158-192; LL_base / LL_bits,
// ML_base / ML_bits of zsmi_fse.h; checked value by value for every length up to 2^17), without a gather from constant memory in the
// middle of a tile (a memory round trip each, and its wait takes the loop's prefetch along).
__device__ __forceinline__ uint32_t llCodeOf(uint32_t ll)
{
    uint32_t c = zs_highbit(ll | 1u) + 19;                        // ll >= 64
    c = (ll < 64) ? 24u : c;
    c = (ll < 48) ? 22u + ((ll - 32) >> 3) : c;
    c = (ll < 32) ? 20u + ((ll - 24) >> 2) : c;
    c = (ll < 24) ? 16u + ((ll - 16) >> 1) : c;
    return (ll < 16) ? ll : c;
}
__device__ __forceinline__ uint32_t mlCodeOf(uint32_t x)         // x = match length - 3
{
    uint32_t c = zs_highbit(x | 1u) + 36;                         // x >= 128
    c = (x < 128) ? 42u : c;
    c = (x < 96) ? 40u + ((x - 64) >> 4) : c;
    c = (x < 64) ? 38u + ((x - 48) >> 3) : c;
    c = (x < 48) ? 36u + ((x - 40) >> 2) : c;
    c = (x < 40) ? 32u + ((x - 32) >> 1) : c;
    return (x < 32) ? x : c;
}
// extra bits of a literal length / of a match length (x = length - 3): value and count
__device__ __forceinline__ uint32_t llExtraOf(uint32_t ll, uint32_t &bits)
{
    const uint32_t h = zs_highbit(ll | 1u);
    uint32_t v = ll - (1u << h), b = h;                            // ll >= 64
    if (ll < 64) { v = ll - 48; b = 4; }
    if (ll < 48) { v = ll & 7u; b = 3; }
    if (ll < 32) { v = ll & 3u; b = 2; }
    if (ll < 24) { v = ll & 1u; b = 1; }
    if (ll < 16) { v = 0; b = 0; }
    bits = b; return v;
}
__device__ __forceinline__ uint32_t mlExtraOf(uint32_t x, uint32_t &bits)
{
    const uint32_t h = zs_highbit(x | 1u);
    uint32_t v = x - (1u << h), b = h;                             // x >= 128
    if (x < 128) { v = x - 96; b = 5; }
    if (x < 96) { v = x & 15u; b = 4; }
    if (x < 64) { v = x & 7u; b = 3; }
    if (x < 48) { v = x & 3u; b = 2; }
    if (x < 40) { v = x & 1u; b = 1; }
    if (x < 32) { v = 0; b = 0; }
    bits = b; return v;
}

// ---------------------------------------------------------------------------------------------
// per-wavefront LDS workspace
// ---------------------------------------------------------------------------------------------
struct FseCT {                       // encoding table of one symbol type
    uint16_t stateTable[512];
    int32_t  deltaFindState[64];
    uint32_t deltaNbBits[64];
    uint32_t tableLog;
    uint32_t rle;
};
// A digested dictionary (zsmi_cdict): the entropy tables of a formatted dictionary as the decoder loads them (ZsCDictEntropy, zsmi_device.h:
// what the dictionary loader read), in their encoder form (k_cdict_tables), which the _cdict kernels read for a frame's first block:
// Repeat_Mode sequences, Treeless literals.
#define ZS_COST_NONE 0xFFFFu         // a symbol the table cannot code (probability 0)
struct ZsCDictTables {
    FseCT ct[3];                     // LL, OF, ML
    uint16_t cost[3][64];            // bits to code symbol s under ct[t], in 1/256 bit (fseSymbolCost); ZS_COST_NONE
    uint32_t hufCodeNb[256];         // code | length << 16, as K3Lds::codeNb; 0: the byte has no code
    uint32_t hufLog;                 // 0: no Huffman table to code with (codes longer than ZS_HUF_MAXBITS are not used)
};
// bits a symbol of normalised count nv >= 1 costs in a table of 2^tableLog cells, in 1/256 bit: exact where nv is a power of two, linear
// between two of them (the state's low bits are maxBitsOut or maxBitsOut - 1 by where the state lies)
__device__ __forceinline__ uint32_t fseSymbolCost(uint32_t nv, uint32_t tableLog)
{
    nv = max(nv, 1u);
    const uint32_t maxBitsOut = nv > 1 ? tableLog - zs_highbit(nv - 1) : tableLog;
    return maxBitsOut * 256u - ((((nv << maxBitsOut) - (1u << tableLog)) << 8) >> tableLog);
}
// workgroups per CU the literals kernel is compiled for: 8 caps it at 64 VGPRs, so the 16 blocks a CU gets per 4096-block
// batch run in two full rounds (measured alone: 0.89 ms uncapped (88 VGPRs, 5 per CU), 0.74 at 6, 0.57 at 8 despite spills)
#ifndef ZS_LIT_MINWG
#define ZS_LIT_MINWG 8
#endif
struct K3Lds {                       // literals kernel
    uint32_t count[256];             // literal histogram
    uint8_t  nbBits[256];
    uint32_t codeNb[256];            // code | nbBits << 16
    uint32_t leafW[256];
    uint16_t leafSym[256];
    uint8_t  lenOfRank[256];
    uint8_t  weights[256];
    union {
        struct { uint32_t pkg[10][256]; uint32_t S[512]; uint32_t npk[12]; } pm;      // package-merge (levels 2..11)
        struct { FseCT ct; FseBuild build; uint16_t stepOut[256]; uint32_t bits[64]; } fse;   // weights table and its build scratch; per step: state bits out | count << 8; the description's bitstream
        struct { FseCT ct; FseBuild build; } cd[3];      // k_cdict_tables: a digested dictionary's three tables (below pm.S, which its Huffman codes use)
        uint32_t tile[4][208];       // bit-packing tiles, one per wavefront (streams are written after the tables are done)
        uint32_t hist[8][257];       // literal gather: eight private histograms (lane & 7), rows one word apart in the banks
        struct { uint32_t T[2052]; uint32_t wpar[4], wcnt[4]; uint32_t sel[16]; } gm;   // literal gather: a bit per block byte (toggles at match ends -> inside a match -> literal), per-wavefront parities / literal counts, byte-compaction selectors
    } u;
    uint32_t misc[16];
    uint32_t dictID;                 // a one-block chunk's dictionary ID, from where its header is sized to where it is written: the kernel has no register to hold it (63 VGPRs, SGPRs spilled)
    uint32_t wcount[16]; int16_t wnorm[16]; uint32_t rankStart[16], rankCount[16];   // small tables kept out of scratch memory
};
// cd[] lies below pm.S, which huffCodesAndWeights writes before k_cdict_tables builds its tables; fse (wave 0, the table description)
// is done with behind a __syncthreads before the streams' tiles take its place
static_assert(sizeof(((K3Lds *)nullptr)->u.cd) <= offsetof(decltype(((K3Lds *)nullptr)->u.pm), S), "the digested dictionary's tables overlap the Huffman scratch S");
struct SeqLds {                      // sequences kernel.  Kept under 10 KiB: 16 workgroups per CU = one round for 4096 blocks
    uint32_t count[192];             // code counts: [0..63] LL, [64..127] OF, [128..191] ML
    FseCT ct[3];                     // LL, OF, ML
    int16_t norm[64];
    union {
        FseBuild build;                          // while a table is built
        struct { uint32_t op[3][64]; } chain;    // while the state chains run: per table and code, deltaNbBits | (deltaFindState + 1024) << 20 (one read a step)
    } u;
    uint32_t tile[208];              // bit-packing tile
    uint32_t misc[16];
};

// Wave-cooperative forward bit writer.  Each put() appends, lane 0 first, up to 96 bits per lane.
// out32 must be 4-byte aligned; bits are packed little-endian (bit k of the stream = bit k%8 of byte k/8).
struct BitSink {
    uint32_t *out32;
    uint32_t *tile;       // LDS, >= 200 words
    uint32_t bitpos;
};
__device__ __forceinline__ void sink_init(BitSink &b, void *out, uint32_t *tile)
{
    b.out32 = (uint32_t *)out; b.tile = tile; b.bitpos = 0;
    if (zs_lane() == 0) tile[0] = 0;
    wave_sync();
}
__device__ __forceinline__ void sink_put(BitSink &b, uint64_t lo, uint32_t hi, uint32_t nb)
{
    const uint32_t lane = (uint32_t)zs_lane();
    const uint32_t incl = wave_incl_scan(nb);
    const uint32_t total = wave_last(incl);
    const uint32_t base = b.bitpos & 31u;
    const uint32_t nwords = (base + total + 31u) >> 5;
    for (uint32_t i = 1 + lane; i <= nwords; i += 64) b.tile[i] = 0;
    wave_sync();
    if (nb) {
        const uint32_t bit = base + incl - nb;
        const uint32_t w = bit >> 5, sh = bit & 31u;
        // 96-bit value shifted left by sh (< 32) -> up to 4 words
        const uint32_t v0 = (uint32_t)lo, v1 = (uint32_t)(lo >> 32), v2 = hi;
        const uint32_t w0 = v0 << sh;
        const uint32_t w1 = sh ? ((v1 << sh) | (v0 >> (32 - sh))) : v1;
        const uint32_t w2 = sh ? ((v2 << sh) | (v1 >> (32 - sh))) : v2;
        const uint32_t w3 = sh ? (v2 >> (32 - sh)) : 0u;
        if (w0) atomicOr(&b.tile[w], w0);
        if (w1) atomicOr(&b.tile[w + 1], w1);
        if (w2) atomicOr(&b.tile[w + 2], w2);
        if (w3) atomicOr(&b.tile[w + 3], w3);
    }
    wave_sync();
    const uint32_t nfull = (base + total) >> 5;
    uint32_t *dst = b.out32 + (b.bitpos >> 5);
    for (uint32_t i = lane; i < nfull; i += 64) dst[i] = b.tile[i];
    const uint32_t carry = b.tile[nfull];
    wave_sync();
    if (lane == 0) b.tile[0] = ((base + total) & 31u) ? carry : 0u;
    wave_sync();
    b.bitpos += total;
}
// adds the end mark (one 1 bit), flushes; returns the stream size in bytes
__device__ __forceinline__ uint32_t sink_close(BitSink &b)
{
    const uint32_t lane = (uint32_t)zs_lane();
    sink_put(b, lane == 0 ? 1ull : 0ull, 0u, lane == 0 ? 1u : 0u);
    if (lane == 0 && (b.bitpos & 31u)) b.out32[b.bitpos >> 5] = b.tile[0];
    wave_sync();
    return (b.bitpos + 7u) >> 3;
}

// ---------------------------------------------------------------------------------------------
// FSE tables: the count description by one lane (serial by nature), normalisation and the encoding table by all lanes
// (scalar statement in oracle/zso_encoder.c)
// ---------------------------------------------------------------------------------------------
__device__ static uint32_t writeNCount(uint8_t *dst, uint32_t cap, const int16_t *norm, uint32_t maxSym, uint32_t tableLog)
{
    uint8_t *out = dst; uint8_t *const oend = dst + cap;
    const int tableSize = 1 << tableLog;
    int remaining = tableSize + 1, threshold = tableSize, nbBits = (int)tableLog + 1;
    uint32_t bitStream = 0; int bitCount = 0; uint32_t charnum = 0; int previous0 = 0;
    bitStream += (tableLog - 5) << bitCount; bitCount += 4;
    while (remaining > 1) {
        if (previous0) {
            uint32_t start = charnum;
            while (charnum <= maxSym && !norm[charnum]) charnum++;
            while (charnum >= start + 24) {
                start += 24; bitStream += 0xFFFFu << bitCount;
                if (out + 2 > oend) return 0;
                out[0] = (uint8_t)bitStream; out[1] = (uint8_t)(bitStream >> 8); out += 2; bitStream >>= 16;
            }
            while (charnum >= start + 3) { start += 3; bitStream += 3u << bitCount; bitCount += 2; }
            bitStream += (charnum - start) << bitCount; bitCount += 2;
            if (bitCount > 16) {
                if (out + 2 > oend) return 0;
                out[0] = (uint8_t)bitStream; out[1] = (uint8_t)(bitStream >> 8); out += 2; bitStream >>= 16; bitCount -= 16;
            }
        }
        {
            int count = norm[charnum++];
            const int max = (2 * threshold - 1) - remaining;
            remaining -= count < 0 ? -count : count;
            count++;
            if (count >= threshold) count += max;
            bitStream += (uint32_t)count << bitCount;
            bitCount += nbBits;
            bitCount -= (count < max);
            previous0 = (count == 1);
            while (remaining < threshold) { nbBits--; threshold >>= 1; }
        }
        if (bitCount > 16) {
            if (out + 2 > oend) return 0;
            out[0] = (uint8_t)bitStream; out[1] = (uint8_t)(bitStream >> 8); out += 2; bitStream >>= 16; bitCount -= 16;
        }
    }
    if (out + 2 > oend) return 0;
    out[0] = (uint8_t)bitStream; out[1] = (uint8_t)(bitStream >> 8);
    out += (bitCount + 7) / 8;
    return (uint32_t)(out - dst);
}

// normalise counts to 2^tableLog, all lanes (lane s owns symbol s); scalar statement: normalizeCounts in the oracle
__device__ __forceinline__ void normalizeCountsWave(int16_t *norm, uint32_t tableLog, const uint32_t *count, uint32_t total, uint32_t maxSym)
{
    const uint32_t lane = (uint32_t)zs_lane();
    const uint32_t tableSize = 1u << tableLog;
    const uint32_t c = (lane <= maxSym) ? count[lane] : 0u;
    uint32_t p = 0;
    if (c) {
        const uint64_t scaled = (uint64_t)c * tableSize;
        p = (uint32_t)(scaled / total);
        const uint32_t rem = (uint32_t)(scaled % total);
        if (2 * (uint64_t)rem >= total) p++;
        if (p == 0) p = 1;
    }
    int still = (int)tableSize - (int)wave_sum(p);
    // largest: first symbol holding the maximum
    { const uint32_t key = (p << 6) | (63u - lane); const uint32_t best = wave_max(key); const uint32_t li = 63u - (best & 63u);
      if (still > 0 && lane == li) p += (uint32_t)still; }
    while (still < 0) {
        const uint32_t key = (p > 1) ? ((p << 6) | (63u - lane)) : 0u;
        const uint32_t best = wave_max(key);
        const uint32_t li = 63u - (best & 63u);
        if (lane == li) p--;
        still++;
    }
    if (lane <= maxSym) norm[lane] = (int16_t)p;
    wave_sync();
}

// THE encoding table, all lanes, from a distribution that may hold -1 entries (a predefined one, a trained dictionary's): the cells in
// the decoder's order (fseSpreadWave), stateTable[cumul[sym] + (rank of cell u among the cells of sym)] = tableSize + u (fseRankWave);
// a -1 counts as 1 in the cumulative counts and in deltaNbBits / deltaFindState.  Scalar statement: buildCTable in the oracle.
__device__ __forceinline__ void buildCTableWave(FseBuild &B, FseCT &ct, const int16_t *norm, uint32_t maxSym, uint32_t tableLog)
{
    const uint32_t lane = (uint32_t)zs_lane();
    const uint32_t tableSize = 1u << tableLog;
    const int n = (lane <= maxSym) ? (int)norm[lane] : 0;
    const uint32_t nv = n < 0 ? 1u : (uint32_t)n;
    const uint32_t excl = wave_incl_scan(nv) - nv;
    B.symCount[lane] = excl;
    if (lane <= maxSym) {
        if (nv == 0) { ct.deltaNbBits[lane] = ((tableLog + 1) << 16) - (1u << tableLog); ct.deltaFindState[lane] = 0; }
        else if (nv == 1) { ct.deltaNbBits[lane] = (tableLog << 16) - (1u << tableLog); ct.deltaFindState[lane] = (int)excl - 1; }
        else { const uint32_t maxBitsOut = tableLog - zs_highbit(nv - 1); ct.deltaNbBits[lane] = (maxBitsOut << 16) - (nv << maxBitsOut); ct.deltaFindState[lane] = (int)excl - (int)nv; }
    }
    if (lane == 0) { ct.tableLog = tableLog; ct.rle = 0; }
    fseSpreadWave(B.cumul, n, maxSym, tableLog, [&](uint32_t cell, uint32_t sym) __attribute__((always_inline)) { B.tableSymbol[cell] = (uint8_t)sym; });
    fseRankWave(B.symMask, B.symCount, tableSize, [&](uint32_t u) __attribute__((always_inline)) { return (uint32_t)B.tableSymbol[u]; },
                [&](uint32_t u, uint32_t, uint32_t next) __attribute__((always_inline)) { ct.stateTable[next] = (uint16_t)(tableSize + u); });
}
__device__ __forceinline__ uint32_t cstate_init(const FseCT &ct, uint32_t symbol)
{
    const uint32_t dnb = ct.deltaNbBits[symbol];
    const uint32_t nbBitsOut = (dnb + (1u << 15)) >> 16;
    const uint32_t v = (nbBitsOut << 16) - dnb;
    return ct.stateTable[(v >> nbBitsOut) + ct.deltaFindState[symbol]];
}

// weights -> FSE (inverse of FSE_decompress_wksp as used by ReadStats, EntropyCommon.cs:226-231), by one wavefront; the weight
// histogram L.wcount[] (all 16 entries) is already filled.  Lane 0 decides the table's shape (<= 13 symbols, <= 64 cells) and writes its
// description; the counts are normalised and the table is built by all lanes, as every FSE table of the encoder.  The encoder's two
// interleaved states run side by side on lanes 0 and 1 (state "first" takes the symbols nw-3, nw-5, ..., "second" nw-4, nw-6, ...;
// per step: value | bit count << 8 into LDS), then all lanes place the steps' bits by a prefix sum of the counts - the scalar form
// (one lane, a byte-wise bit writer, ~250 dependent steps) was a third of the kernel's time between the code lengths and the streams.
// Same bytes as fseCompressWeights in oracle/zso_encoder.c.
__device__ __forceinline__ uint32_t fseCompressWeightsWave(K3Lds &L, uint8_t *dst, uint32_t cap, const uint8_t *weights, uint32_t nw)
{
    const uint32_t lane = (uint32_t)zs_lane();
    // (misc[12 .. 14] are borrowed: the block's per-wavefront code bits, which every thread has read before the workgroup barriers of
    //  huffCodesAndWeights that lie between that read and this call)
    if (lane == 0) {                                                      // what is scalar by nature: is there an FSE form, and its shape
        uint32_t tl = 0, maxSym = 0;
        do {
            const uint32_t *count = L.wcount;
            uint32_t tableLog;
            if (nw <= 1) break;
            for (uint32_t i = 0; i < 16; i++) if (count[i]) maxSym = i;
            bool one = false;
            for (uint32_t i = 0; i <= maxSym; i++) if (count[i] == nw) one = true;
            if (one) break;
            tableLog = 6;
            while (tableLog > 5 && (1u << (tableLog - 1)) >= nw) tableLog--;
            { uint32_t present = 0; for (uint32_t i = 0; i <= maxSym; i++) present += count[i] != 0; if (present > (1u << tableLog)) break; }
            tl = tableLog;
        } while (0);
        L.misc[13] = tl; L.misc[14] = maxSym;
    }
    L.u.fse.bits[lane] = 0;
    wave_sync();
    const uint32_t tableLog = L.misc[13], maxSym = L.misc[14];
    if (!tableLog) return 0;
    normalizeCountsWave(L.wnorm, tableLog, L.wcount, nw, maxSym);
    if (lane == 0) L.misc[12] = writeNCount(dst, cap, L.wnorm, maxSym, tableLog);
    wave_sync();
    const uint32_t hsize = L.misc[12];
    if (!hsize) return 0;
    buildCTableWave(L.u.fse.build, L.u.fse.ct, L.wnorm, maxSym, tableLog);
    const FseCT &ct = L.u.fse.ct;
    const uint32_t K = nw - 2;                                            // encode steps; step k takes symbol nw - 3 - k
    uint16_t *stepOut = L.u.fse.stepOut;
    uint32_t fin = 0;
    if (lane < 2) {
        uint32_t st = cstate_init(ct, weights[nw - 1 - lane]);
        for (uint32_t k = lane; k < K; k += 2) {
            const uint32_t sym = weights[nw - 3 - k];
            const uint32_t nbo = (st + ct.deltaNbBits[sym]) >> 16;
            stepOut[k] = (uint16_t)((st & ((1u << nbo) - 1u)) | (nbo << 8));
            st = ct.stateTable[(st >> nbo) + ct.deltaFindState[sym]];
        }
        fin = st;
    }
    wave_sync();
    // final states go out st2 first, then st1: with an odd count the first state is st1, with an even count st2
    const uint32_t stFirst = wave_get(fin, 0), stSecond = wave_get(fin, 1);
    const uint32_t st2 = (nw & 1u) ? stSecond : stFirst, st1 = (nw & 1u) ? stFirst : stSecond;
    uint32_t *bits = L.u.fse.bits;
    uint32_t total = 0;
    for (uint32_t k0 = 0; k0 < K + 3; k0 += 64) {
        const uint32_t k = k0 + lane;
        uint32_t val = 0, nb = 0;
        if (k < K) { const uint32_t e = stepOut[k]; val = e & 0xFFu; nb = e >> 8; }
        else if (k == K) { val = st2 & ((1u << tableLog) - 1u); nb = tableLog; }
        else if (k == K + 1) { val = st1 & ((1u << tableLog) - 1u); nb = tableLog; }
        else if (k == K + 2) { val = 1; nb = 1; }                         // the end mark
        const uint32_t incl = wave_incl_scan(nb);
        const uint32_t off = total + incl - nb;
        if (nb) {
            const uint32_t w = off >> 5, sh = off & 31u;
            atomicOr(&bits[w], val << sh);
            if (sh + nb > 32u) atomicOr(&bits[w + 1], val >> (32u - sh));
        }
        total += wave_last(incl);
    }
    wave_sync();
    const uint32_t bytes = (total + 7u) >> 3;
    if (bytes > cap - hsize) return 0;
    const uint8_t *bb = reinterpret_cast<const uint8_t *>(bits);
    for (uint32_t j = lane; j < bytes; j += 64) dst[hsize + j] = bb[j];
    return hsize + bytes;
}

// Huffman table description (inverse of ReadStats, EntropyCommon.cs:198-269), by one wavefront; L.weights[0..maxSym) and the
// histogram of those weights are already filled.
__device__ __forceinline__ uint32_t writeHuffHeaderWave(K3Lds &L, uint8_t *dst, uint32_t cap, uint32_t maxSym, uint32_t tableLog)
{
    const uint32_t lane = (uint32_t)zs_lane();
    uint8_t *weights = L.weights;
    if (maxSym >= 2 && cap > 1) {
        const uint32_t h = fseCompressWeightsWave(L, dst + 1, cap - 1 < 127 ? cap - 1 : 127, weights, maxSym);
        if (h > 1 && h < maxSym / 2 && h < 128) { if (lane == 0) dst[0] = (uint8_t)h; return h + 1; }
    }
    if (maxSym > 128) return 0;
    if ((maxSym + 1) / 2 + 1 > cap) return 0;
    if (lane == 0) { dst[0] = (uint8_t)(128 + (maxSym - 1)); weights[maxSym] = 0; }
    wave_sync();
    for (uint32_t s = 2 * lane; s < maxSym; s += 128) dst[s / 2 + 1] = (uint8_t)((weights[s] << 4) + weights[s + 1]);
    return (maxSym + 1) / 2 + 1;
}

// ---------------------------------------------------------------------------------------------
// package-merge code lengths, wave-parallel (scalar statement: huffLengths in oracle/zso_encoder.c)
// returns the longest code length (= Huffman tableLog)
// ---------------------------------------------------------------------------------------------
__device__ static uint32_t lowerBound(const uint32_t *a, uint32_t n, uint32_t key)   // #elements < key
{ uint32_t lo = 0, hi = n; while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (a[mid] < key) lo = mid + 1; else hi = mid; } return lo; }
__device__ static uint32_t upperBound(const uint32_t *a, uint32_t n, uint32_t key)   // #elements <= key
{ uint32_t lo = 0, hi = n; while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (a[mid] <= key) lo = mid + 1; else hi = mid; } return lo; }

__device__ static uint32_t huffLengths(K3Lds &L, uint32_t maxSym, uint32_t maxBits)
{
    // 256 threads: thread s owns symbol s, later leaf rank s / package index s
    const uint32_t tid = threadIdx.x;
    const uint32_t c = (tid <= maxSym) ? L.count[tid] : 0u;
    L.nbBits[tid] = 0;
    // leaves in ascending (count, symbol) order.  The symbols that occur are packed first (key = count << 8 | symbol, in S), so a
    // symbol's rank is a count over the ~90 keys of a text block, not a test of all 256 counters
    uint32_t *keys = L.u.pm.S;
    const uint32_t lane_ = tid & 63u, wave_ = tid >> 6;
    const uint64_t pres = __ballot(c != 0);
    if (lane_ == 0) L.u.pm.npk[4 + wave_] = (uint32_t)__popcll(pres);      // npk[0..11] is free until the levels start
    __syncthreads();
    uint32_t before = 0, n = 0;
    #pragma unroll
    for (uint32_t v = 0; v < 4; v++) { const uint32_t k = L.u.pm.npk[4 + v]; if (v < wave_) before += k; n += k; }
    const uint32_t key = (c << 8) | tid;
    if (c) keys[before + (uint32_t)__popcll(pres & ((1ull << lane_) - 1ull))] = key;
    __syncthreads();
    if (c) {
        uint32_t rank = 0;
        for (uint32_t t = 0; t < n; t++) rank += (keys[t] < key) ? 1u : 0u;
        L.leafW[rank] = c; L.leafSym[rank] = (uint16_t)tid;
    }
    __syncthreads();
    if (n == 1) { if (tid == 0) L.nbBits[L.leafSym[0]] = 1; __syncthreads(); return 1; }
    uint32_t (*pkg)[256] = L.u.pm.pkg;         // pkg[level - 2]
    uint32_t *S = L.u.pm.S;
    uint32_t *npk = L.u.pm.npk;                // npk[level]
    if (tid == 0) npk[1] = 0;
    __syncthreads();
    for (uint32_t level = 2; level <= maxBits; level++) {
        const uint32_t np = npk[level - 1];
        const uint32_t *prev = (level >= 3) ? pkg[level - 3] : nullptr;
        if (tid < n) { const uint32_t w = L.leafW[tid]; S[tid + (np ? lowerBound(prev, np, w) : 0u)] = w; }
        if (tid < np) { const uint32_t w = prev[tid]; S[tid + upperBound(L.leafW, n, w)] = w; }
        __syncthreads();
        const uint32_t have = (n + np) >> 1;
        if (tid < have) pkg[level - 2][tid] = S[2 * tid] + S[2 * tid + 1];
        if (tid == 0) npk[level] = have;
        __syncthreads();
    }
    L.lenOfRank[tid] = 0;
    __syncthreads();
    uint32_t m = 2 * n - 2;
    for (uint32_t level = maxBits; level >= 1; level--) {
        const uint32_t np = npk[level];
        const uint32_t *cur = (level >= 2) ? pkg[level - 2] : nullptr;
        if (m > n + np) m = n + np;
        bool in = false;
        if (tid < n) { const uint32_t pos = tid + (np ? lowerBound(cur, np, L.leafW[tid]) : 0u); in = pos < m; }
        const uint32_t li = (uint32_t)__syncthreads_count(in);
        if (in) L.lenOfRank[tid]++;
        const uint32_t pi = m - li;
        m = 2 * pi;
        if (!m) break;
    }
    __syncthreads();
    if (tid < n) L.nbBits[L.leafSym[tid]] = L.lenOfRank[tid];
    __syncthreads();
    return L.lenOfRank[0];
}

// code values in the decoder's table order (HufDecompress.cs:148-176), weights and their histogram; 256 threads
// (thread s owns symbol s).  code[s] = rankStart[w] / 2^(w-1) + (number of lower symbols with the same weight).
__device__ static void huffCodesAndWeights(K3Lds &L, uint32_t maxSym, uint32_t tableLog)
{
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t nb = (tid <= maxSym) ? L.nbBits[tid] : 0u;
    const uint32_t w = nb ? tableLog + 1 - nb : 0u;
    if (tid < 16) { L.rankCount[tid] = 0; L.wcount[tid] = 0; }
    __syncthreads();
    if (nb) atomicAdd(&L.rankCount[w], 1u);
    if (tid < maxSym) { L.weights[tid] = (uint8_t)w; atomicAdd(&L.wcount[w], 1u); }       // the last symbol's weight is implied
    __syncthreads();
    if (tid == 0) { uint32_t next = 0; for (uint32_t k = 1; k <= tableLog; k++) { L.rankStart[k] = next; next += L.rankCount[k] << (k - 1); } }
    // index among the symbols of equal weight: lower lanes of my wavefront + whole lower wavefronts (counted per weight)
    uint32_t idx = 0;
    for (uint32_t k = 1; k <= tableLog; k++) {
        const uint64_t m = __ballot(w == k);
        if (w == k) idx = (uint32_t)__popcll(m & ((1ull << lane) - 1));
        if (lane == 0) L.u.pm.S[wave * 16 + k] = (uint32_t)__popcll(m);                    // S is free again after the code lengths
    }
    __syncthreads();
    if (nb) {
        for (uint32_t v = 0; v < wave; v++) idx += L.u.pm.S[v * 16 + w];
        L.codeNb[tid] = ((L.rankStart[w] >> (w - 1)) + idx) | (nb << 16);
    }
    __syncthreads();
}

// one Huffman stream of lits[from .. from+len) into tmp (4-byte aligned); last symbol first. returns bytes.
__device__ __forceinline__ uint32_t huffEncodeStream(K3Lds &L, uint32_t *tile, uint8_t *tmp, const uint8_t *lits, uint32_t from, uint32_t len)
{
    const uint32_t lane = (uint32_t)zs_lane();
    BitSink sink; sink_init(sink, tmp, tile);
    uint32_t remaining = len;
    // lane l takes symbols k = 8l .. 8l+7 of the tile, i.e. the 8 literals ending at position from + remaining - 1 - 8l, last first
    const uint32_t k0 = lane * 8;
    auto fetch = [&](uint32_t rem) -> uint64_t {
        const uint32_t T = min(512u, rem);
        uint64_t e = 0;
        if (k0 + 8 <= T) e = zs_load64(lits + from + rem - 8 - k0);
        else for (uint32_t j = 0; j < 8; j++) if (k0 + j < T) e |= (uint64_t)lits[from + rem - 1 - k0 - j] << (8 * (7 - j));
        return e;
    };
    uint64_t next = remaining ? fetch(remaining) : 0ull;                   // the next tile's bytes travel while this one is packed
    while (remaining) {
        const uint32_t T = min(512u, remaining);
        const uint64_t eight = next;
        if (remaining > T) next = fetch(remaining - T);
        // the eight codes are looked up as one batch (one wait), a symbol beyond the tile counts as code 0 of length 0 by a select, and the
        // codes are merged as a tree: pairs in 32 bits (<= 22), fours in 64 (<= 44), the two fours into lo / hi (<= 88).  (Appended one
        // by one, each symbol was a divergent region with its own LDS round trip and a ladder of exec masks around a 64-bit shift.)
        uint32_t cn[8];
        #pragma unroll
        for (uint32_t j = 0; j < 8; j++) cn[j] = L.codeNb[(uint32_t)(eight >> (8 * (7 - j))) & 0xFFu];
        #pragma unroll
        for (uint32_t j = 0; j < 8; j++) cn[j] = (k0 + j < T) ? cn[j] : 0u;
        uint32_t pv[4], pn[4];
        #pragma unroll
        for (uint32_t j = 0; j < 4; j++) {
            const uint32_t b0 = cn[2 * j] >> 16;
            pv[j] = (cn[2 * j] & 0xFFFFu) | ((cn[2 * j + 1] & 0xFFFFu) << b0);
            pn[j] = b0 + (cn[2 * j + 1] >> 16);
        }
        const uint64_t q0 = (uint64_t)pv[0] | ((uint64_t)pv[1] << pn[0]), q1 = (uint64_t)pv[2] | ((uint64_t)pv[3] << pn[2]);
        const uint32_t n0 = pn[0] + pn[1];                                  // <= 44
        const uint64_t lo = q0 | (q1 << n0);
        const uint32_t hi = (uint32_t)((q1 >> 1) >> (63u - n0));            // q1's bits from 64 - n0 up (n0 = 0: none)
        const uint32_t nb = n0 + pn[2] + pn[3];
        sink_put(sink, lo, hi, nb);
        remaining -= T;
    }
    return sink_close(sink);
}

// exclusive "last lane below me with flag" : returns lane index or -1
__device__ __forceinline__ int lastFlagBelow(bool flag)
{
    const uint64_t m = __ballot(flag);
    const uint32_t lane = (uint32_t)zs_lane();
    const uint64_t below = lane ? (m & ((1ull << lane) - 1)) : 0ull;
    return below ? 63 - __builtin_clzll(below) : -1;
}

struct ZsChunkDesc { uint64_t srcOff; uint64_t dstOff; uint32_t size; uint32_t firstBlock; uint32_t nBlocks; uint32_t pad; };

// frame header of a chunk (magic + FHD + FCS, single segment); returns its size.  One thread writes it.
// dictID != 0 (dictionary calls): the dictionary ID field between FHD and FCS, in 1, 2 or 4 bytes (the fewest that hold it, as libzstd)
// the dictionary ID of a chunk's frame: its record's (dictTab[chunkDict[chunk]], one address a workgroup), 0 without a table or a record
__device__ __forceinline__ uint32_t zs_chunk_dict_id(const ZsCDictEntry *__restrict__ dictTab, const uint32_t *__restrict__ chunkDict, uint32_t chunk)
{
    const uint32_t e = dictTab ? (chunkDict ? chunkDict[chunk] : 0u) : ZS_DICT_NONE;
    return e != ZS_DICT_NONE ? dictTab[e].dictID : 0u;
}
__device__ __forceinline__ uint32_t zs_frame_header(uint8_t *out, uint32_t size, bool writer, uint32_t dictID = 0)
{
    const uint32_t didCode = (dictID != 0) + (dictID >= 256) + (dictID >= 65536), didSize = didCode == 3 ? 4 : didCode;
    if (writer) {
        out[0] = 0x28; out[1] = 0xB5; out[2] = 0x2F; out[3] = 0xFD;
        for (uint32_t k = 0; k < didSize; k++) out[5 + k] = (uint8_t)(dictID >> (8 * k));
        uint8_t *f = out + didSize;
        if (size < 256) { out[4] = 0x20 | didCode; f[5] = (uint8_t)size; }
        else if (size < 65536 + 256) { out[4] = 0x60 | didCode; const uint32_t v = size - 256; f[5] = (uint8_t)v; f[6] = (uint8_t)(v >> 8); }
        else { out[4] = 0xA0 | didCode; f[5] = (uint8_t)size; f[6] = (uint8_t)(size >> 8); f[7] = (uint8_t)(size >> 16); f[8] = (uint8_t)(size >> 24); }
    }
    return ((size < 256) ? 6 : (size < 65536 + 256 ? 7 : 9)) + didSize;
}
// one block into its frame at out + pos (all threads of the workgroup); returns the bytes written.  A block is emitted compressed
// iff both sections exist and literal section + sequence section < block size (else raw; RLE if flagged).
__device__ __forceinline__ uint32_t zs_emit_block(uint8_t *out, uint32_t pos, const uint8_t *blockSrc, uint32_t n, uint32_t last, const ZsBlockMeta m,
                                                 const uint8_t *p1, const uint8_t *p2, uint32_t tid, uint32_t nthreads)
{
    uint32_t type = m.type;
    uint32_t total = 0;
    if (type == 2) {
        // same decisions as the scalar statement: room left after the literals, section failures, final size test
        if (m.seqSecSize == 0xFFFFFFFFu || m.litSecSize + 4 > n + 512) type = 0;
        else { total = m.litSecSize + m.seqSecSize; if (total > n + 512 || total >= n) type = 0; }
    }
    if (type == 1) {
        if (tid == 0) { const uint32_t h = last + (1u << 1) + (n << 3); out[pos] = (uint8_t)h; out[pos + 1] = (uint8_t)(h >> 8); out[pos + 2] = (uint8_t)(h >> 16); out[pos + 3] = (uint8_t)m.rleByte; }
        return 4;
    }
    if (type == 2) {
        if (tid == 0) { const uint32_t h = last + (2u << 1) + (total << 3); out[pos] = (uint8_t)h; out[pos + 1] = (uint8_t)(h >> 8); out[pos + 2] = (uint8_t)(h >> 16); }
        if (p1 != out + pos + 3) zs_block_copy(out + pos + 3, p1, m.litSecSize, tid, nthreads);       // (the literals kernel builds a one-block chunk's section in place)
        zs_block_copy(out + pos + 3 + m.litSecSize, p2, m.seqHdrSize, tid, nthreads);
        zs_block_copy(out + pos + 3 + m.litSecSize + m.seqHdrSize, p2 + m.seqHdrSize + m.seqGap, m.seqSecSize - m.seqHdrSize, tid, nthreads);
        return 3 + total;
    }
    if (tid == 0) { const uint32_t h = last + (0u << 1) + (n << 3); out[pos] = (uint8_t)h; out[pos + 1] = (uint8_t)(h >> 8); out[pos + 2] = (uint8_t)(h >> 16); }
    zs_block_copy(out + pos + 3, blockSrc, n, tid, nthreads);
    return 3 + n;
}

// ---------------------------------------------------------------------------------------------
// k_encode_literals : one workgroup of 4 wavefronts per block.  Block type (raw for tiny blocks, RLE block),
// literal gather (a stream compaction of the block) + histogram, Huffman lengths by package-merge (256 threads),
// table description (one lane), the 4 Huffman streams (one wavefront each)  -> litSec[], meta.{type, rleByte, litSecSize}
// ---------------------------------------------------------------------------------------------
// (dictTab, chunkDict: the call's dictionary records (ZsCDictEntry; null: none) and the record index a chunk (null: record 0; ZS_DICT_NONE:
//  none).  The frame header carries the ID of the chunk's record, 0 without one.  CD: with a digested dictionary's Huffman codes in the record's tables the
//  first block of a frame is coded as Treeless literals (type 3) iff every literal byte has a code and that section is strictly smaller than the rules' below)
#define ZS_LIT_PARAMS const uint8_t *__restrict__ src, const ZsBlockDesc *__restrict__ blocks, \
                      const ZsSeqRec *__restrict__ seqAll, const uint32_t *__restrict__ hdrAll, \
                      uint8_t *__restrict__ litsAll, uint8_t *__restrict__ streamAll, uint8_t *__restrict__ litSecAll, \
                      ZsBlockMeta *__restrict__ metas, int stopAt, \
                      const ZsChunkDesc *__restrict__ chunks, const uint8_t *__restrict__ seqSecAll, uint8_t *__restrict__ dst, uint32_t *__restrict__ dstSizes
#define ZS_LIT_ARGS src, blocks, seqAll, hdrAll, litsAll, streamAll, litSecAll, metas, stopAt, chunks, seqSecAll, dst, dstSizes
template <bool CD>
__device__ __forceinline__ void encode_literals_block(ZS_LIT_PARAMS, const ZsCDictEntry *__restrict__ dictTab, const uint32_t *__restrict__ chunkDict)
{
    __shared__ K3Lds L;
    const uint32_t blk = blockIdx.x;
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    const ZsBlockDesc bd = blocks[blk];
    // CD: a frame's first block takes the tables of its chunk's record (the workgroup's one address); no record, or one without tables:
    // cdt stays null and the block is coded as by the form without CD
    const ZsCDictTables *__restrict__ cdt = nullptr;
    if constexpr (CD) {
        if (dictTab && bd.firstInChunk) {
            const uint32_t e = chunkDict ? chunkDict[bd.chunk] : 0u;
            if (e != ZS_DICT_NONE) cdt = dictTab[e].tables;
        }
    }
    const uint8_t *s = src + bd.srcOff;
    const uint32_t n = bd.size;
    const ZsSeqRec *seqBase = zs_block_seqs(seqAll, blk);
    uint8_t *lits = zs_block_lits(litsAll, blk);
    uint8_t *streams = zs_block_streams(streamAll, blk);
    // the literal section of a one-block chunk is built where its frame wants it (behind the frame header and the 3-byte block header: the
    // slot holds zsmi_compressBound(n) >= n + 27 bytes, the section never more than n + 3), every other block's in the section buffer
    const bool solo = bd.firstInChunk && bd.lastInChunk && !ZS_STOPPED;
    uint8_t *payload = zs_block_lit_section(litSecAll, blk);
    if (solo) {                                      // (the ID waits in LDS for FINISH, which reads it behind its barrier)
        const uint32_t id0 = zs_chunk_dict_id(dictTab, chunkDict, bd.chunk);
        if (tid == 0) L.dictID = id0;
        const ZsChunkDesc cd0 = chunks[bd.chunk]; payload = dst + cd0.dstOff + zs_frame_header(nullptr, cd0.size, false, id0) + 3;
    }
    const uint32_t cap = n + 512;

    // The block's literal side is done: its meta goes out; a chunk of ONE block is assembled right here (the sequences kernel ran before this
    // one on the stream, its section and meta fields are there) - k_assemble_frames is launched only for batches with longer chunks
    #define FINISH(tp, lsz, rb) do { \
        if (tid == 0) { ZsBlockMeta &mo_ = zs_block_meta(metas, blk); mo_.type = (tp); mo_.rleByte = (rb); mo_.litSecSize = (lsz); } \
        if (bd.firstInChunk && bd.lastInChunk && !ZS_STOPPED) { \
            __syncthreads();                         /* the literal section was written by all wavefronts */ \
            ZsBlockMeta m_ = zs_block_meta(metas, blk); m_.type = (tp); m_.rleByte = (rb); m_.litSecSize = (lsz); \
            const ZsChunkDesc cd_ = chunks[bd.chunk]; \
            uint8_t *out_ = dst + cd_.dstOff; \
            uint32_t pos_ = zs_frame_header(out_, cd_.size, tid == 0, L.dictID); \
            pos_ += zs_emit_block(out_, pos_, s, n, 1u, m_, payload, zs_block_seq_section(seqSecAll, blk), tid, 256); \
            if (tid == 0) dstSizes[bd.chunk] = pos_; \
        } \
        return; } while (0)

    if (n == 0) FINISH(0, 0, 0);
    {   // RLE block: every byte equal (ZStdDecompress.cs:1945-1950 on the decode side)
        // 16 bytes per thread and load; most blocks fail within the first 4 KiB
        const uint32_t b0 = s[0];
        const uint64_t rep = 0x0101010101010101ull * b0;
        bool diff = false;
        for (uint32_t base = 0; base < n; base += 256 * 16) {
            const uint32_t i = base + tid * 16;
            if (i + 16 <= n) { const uint64_t a = zs_load64(s + i), b = zs_load64(s + i + 8); diff |= (a != rep) | (b != rep); }
            else for (uint32_t j = i; j < n; j++) diff |= (s[j] != b0);
            if (__syncthreads_or(diff)) { diff = true; break; }
        }
        if (!diff) FINISH(1, 0, b0);
    }
    if (n < 16) FINISH(0, 0, 0);

    const ZsBlockHdr bh = zs_block_hdr(hdrAll, blk);                       // (the workgroup's one address)
    const uint32_t nseq = bh.nseq, nlit = bh.lits;

    // ---- literals: gather into lits[], histogram ----
    uint32_t *hist = L.u.hist[lane & 7u];                                  // this lane's private histogram
    // a block without a match (a matchless unit: noise, packed data) has its literals where they are: no gather, the source is read in its place
    const bool ungathered = nlit == n;
    const uint8_t *litp = ungathered ? s : lits;
    // The literals of a block are its bytes outside every match, in order.  So: a bit per byte, toggled at every match start and
    // end (LDS atomics, lane = sequence); a prefix xor turns the toggles into "inside a match"; the rest is a stream compaction of
    // the source, 16 bytes a lane and round, every lane busy with contiguous, coalesced bytes.  (Taking the literal runs sequence by
    // sequence - a run of ~3 bytes per lane, its own load and store pieces - was ~300 instructions per 64 sequences, issue-bound.)
    if (!ungathered) {
        uint32_t *T = L.u.gm.T;
        for (uint32_t i = tid; i < 2052; i += 256) T[i] = 0;
        if (tid < 16) {                                                   // byte selectors of v_perm for a 4-bit mask: the set bytes in order, then zeros
            uint32_t sel = 0, k = 0;
            for (uint32_t bsel = 0; bsel < 4; bsel++) if (tid & (1u << bsel)) { sel |= bsel << (8 * k); k++; }
            for (; k < 4; k++) sel |= 0x0Cu << (8 * k);
            L.u.gm.sel[tid] = sel;
        }
        __syncthreads();
        // 1. toggles, a lane a record of the block's list: tile 4 q + w of a sweep of 64 tiles is wavefront w's; its 16 record loads are issued together
        for (uint32_t g0 = 0; g0 < nseq; g0 += 64u * 64u) {
            uint2 rec[16];
            #pragma unroll
            for (uint32_t q = 0; q < 16; q++) {
                const uint32_t t0 = g0 + 64u * (4u * q + wave);
                rec[q] = make_uint2(0, 0);
                if (t0 < nseq && t0 + lane < nseq) rec[q] = *reinterpret_cast<const uint2 *>(seqBase + t0 + lane);
            }
            #pragma unroll
            for (uint32_t q = 0; q < 16; q++) {
                const uint32_t t0 = g0 + 64u * (4u * q + wave);
                if (t0 < nseq && t0 + lane < nseq) {
                    const uint32_t p0 = zs_rec_pos(rec[q].y), p1 = p0 + zs_rec_ml(rec[q].x);
                    atomicXor(&T[p0 >> 5], 1u << (p0 & 31u));
                    atomicXor(&T[p1 >> 5], 1u << (p1 & 31u));
                }
            }
        }
        __syncthreads();
        // 2. prefix xor over the 65536 bits (thread t: dwords 8 t .. 8 t + 7), literal bits = its complement below n, literals per wavefront region
        uint32_t x[8];
        {
            uint32_t carry = 0;
            #pragma unroll
            for (uint32_t d = 0; d < 8; d++) {
                uint32_t y = T[8 * tid + d];
                y ^= y << 1; y ^= y << 2; y ^= y << 4; y ^= y << 8; y ^= y << 16;
                y ^= 0u - carry;                                          // the dwords before end inside a match: all flipped
                carry = y >> 31;
                x[d] = y;
            }
            const uint64_t pm = __ballot(carry != 0);
            const uint32_t pin = (uint32_t)__popcll(pm & ((1ull << lane) - 1ull)) & 1u;
            if (lane == 0) L.u.gm.wpar[wave] = (uint32_t)__popcll(pm) & 1u;
            __syncthreads();
            uint32_t flip = pin;
            for (uint32_t v = 0; v < wave; v++) flip ^= L.u.gm.wpar[v];
            uint32_t cnt = 0;
            #pragma unroll
            for (uint32_t d = 0; d < 8; d++) {
                const uint32_t bitBase = (8 * tid + d) * 32;
                uint32_t lm = ~(x[d] ^ (0u - flip));
                if (bitBase + 32 > n) lm = (bitBase < n) ? (lm & ((1u << (n - bitBase)) - 1u)) : 0u;
                T[8 * tid + d] = lm;
                cnt += (uint32_t)__popc(lm);
            }
            const uint32_t tot = wave_sum(cnt);
            if (lane == 0) L.u.gm.wcnt[wave] = tot;
        }
        __syncthreads();
        // 3. compaction: wavefront w takes the bytes [16384 w, 16384 (w + 1)), 1 KiB a round (two rounds' loads in flight)
        uint32_t running = 0;
        for (uint32_t v = 0; v < wave; v++) running += L.u.gm.wcnt[v];
        const uint32_t regionEnd = min(n, 16384u * (wave + 1));
        for (uint32_t p0 = 16384u * wave; p0 < regionEnd; p0 += 2048) {
            uint64_t a[2], b[2]; uint32_t m16[2];
            #pragma unroll
            for (uint32_t h = 0; h < 2; h++) {
                const uint32_t p = p0 + 1024 * h + 16 * lane;
                a[h] = 0; b[h] = 0; m16[h] = 0;
                if (p < n) {
                    m16[h] = (T[p >> 5] >> (p & 31u)) & 0xFFFFu;
                    if (p + 16 <= n) { a[h] = zs_load64(s + p); b[h] = zs_load64(s + p + 8); }
                    else for (uint32_t j = 0; p + j < n; j++) { const uint64_t c = s[p + j]; if (j < 8) a[h] |= c << (8 * j); else b[h] |= c << (8 * (j - 8)); }
                }
            }
            #pragma unroll
            for (uint32_t h = 0; h < 2; h++) {
                if (p0 + 1024 * h >= regionEnd) continue;
                const uint32_t m = m16[h];
                const uint32_t c0 = (uint32_t)__popc(m & 0xFu), c1 = (uint32_t)__popc(m & 0xF0u), c2 = (uint32_t)__popc(m & 0xF00u), c3 = (uint32_t)__popc(m & 0xF000u);
                const uint32_t q0 = __builtin_amdgcn_perm(0u, (uint32_t)a[h], L.u.gm.sel[m & 15u]);
                const uint32_t q1 = __builtin_amdgcn_perm(0u, (uint32_t)(a[h] >> 32), L.u.gm.sel[(m >> 4) & 15u]);
                const uint32_t q2 = __builtin_amdgcn_perm(0u, (uint32_t)b[h], L.u.gm.sel[(m >> 8) & 15u]);
                const uint32_t q3 = __builtin_amdgcn_perm(0u, (uint32_t)(b[h] >> 32), L.u.gm.sel[(m >> 12) & 15u]);
                const uint64_t lo = (uint64_t)q0 | ((uint64_t)q1 << (8 * c0)), hi = (uint64_t)q2 | ((uint64_t)q3 << (8 * c2));   // <= 8 bytes each
                const uint32_t cl = c0 + c1, cnt = cl + c2 + c3;
                // 16 compacted bytes (w0 low, w1 high): lo, then hi from byte cl
                const uint64_t w0 = (cl < 8) ? (lo | (hi << (8 * cl))) : lo;
                const uint64_t w1 = (cl == 0) ? 0ull : ((cl < 8) ? (hi >> (64 - 8 * cl)) : hi);
                const uint32_t incl = wave_incl_scan(cnt);
                uint8_t *dp = lits + running + incl - cnt;
                if (cnt == 16) { zs_store64(dp, w0); zs_store64(dp + 8, w1); }
                else {
                    uint64_t t = w0; uint32_t at = 0;
                    if (cnt & 8) { zs_store64(dp, t); t = w1; at = 8; }
                    if (cnt & 4) { zs_store32(dp + at, (uint32_t)t); t >>= 32; at += 4; }
                    if (cnt & 2) { zs_store16(dp + at, (uint16_t)t); t >>= 16; at += 2; }
                    if (cnt & 1) dp[at] = (uint8_t)t;
                }
                running += wave_last(incl);
            }
        }
        __syncthreads();                                                  // the bit plane is done with: the histograms take its place
    }
    #pragma unroll
    for (uint32_t k = 0; k < 8; k++) L.u.hist[k][tid] = 0;
    __syncthreads();
    // 4. histogram of the gathered literals, four bytes a thread and round
    for (uint32_t j = 4 * tid; j < nlit; j += 1024) {
        const uint32_t k = min(4u, nlit - j);
        uint32_t w;
        if (k == 4 || !ungathered) w = zs_load32(litp + j);               // (the literal buffer has 64 bytes of slack; the source has none)
        else { w = 0; for (uint32_t q = 0; q < k; q++) w |= (uint32_t)litp[j + q] << (8 * q); }
        atomicAdd(&hist[w & 0xFFu], 1u);
        if (k > 1) atomicAdd(&hist[(w >> 8) & 0xFFu], 1u);
        if (k > 2) atomicAdd(&hist[(w >> 16) & 0xFFu], 1u);
        if (k > 3) atomicAdd(&hist[w >> 24], 1u);
    }
    __syncthreads();
    {
        uint32_t c = 0;
        #pragma unroll
        for (uint32_t k = 0; k < 8; k++) c += L.u.hist[k][tid];
        L.count[tid] = c;
    }
    __syncthreads();
    if (ZS_STOP_AT(1)) FINISH(0, 0, 0);            // timing aid (ZSMI_STOP_LIT): stop after the literal gather

    // ---- literals section (inverse of DecodeLiteralsBlock, ZStdDecompress.cs:683-821) ----
    if (wave == 0) {
        uint32_t maxSym = 0, largest = 0, smallest = 0xFFFFFFFFu;
        for (uint32_t b = 0; b < 256; b += 64) {
            const uint32_t c = L.count[b + lane];
            const uint64_t present = __ballot(c != 0);
            if (present) maxSym = b + 63u - (uint32_t)__builtin_clzll(present);
            largest = max(largest, wave_max(c));
            smallest = min(smallest, ~wave_max(~c));
        }
        if (lane == 0) { L.misc[3] = maxSym; L.misc[4] = largest; L.misc[5] = smallest; }
    }
    __syncthreads();
    const uint32_t maxSym = L.misc[3], largest = L.misc[4];
    // all 256 byte values occur and the most frequent less than twice as often as the rarest (noise, packed data in blocks of 64 KiB): every
    // Huffman merge then pairs two nodes of one level before any node of the next - the code is the complete tree, 8 bits a symbol, and
    // the section cannot be smaller than the literals: no code is built
    const bool flatCounts = L.misc[5] != 0 && largest < 2u * L.misc[5];
    uint32_t litSecSize = 0;
    bool done = false;
    if (nlit > 0 && largest == nlit && nlit > 4) {
        if (tid == 0) {
            const uint8_t b0 = litp[0];
            if (nlit < 32) { payload[0] = (uint8_t)(1 + (nlit << 3)); payload[1] = b0; }
            else if (nlit < 4096) { const uint32_t h = 1 + (1 << 2) + (nlit << 4); payload[0] = (uint8_t)h; payload[1] = (uint8_t)(h >> 8); payload[2] = b0; }
            else { const uint32_t h = 1 + (3 << 2) + (nlit << 4); payload[0] = (uint8_t)h; payload[1] = (uint8_t)(h >> 8); payload[2] = (uint8_t)(h >> 16); payload[3] = b0; }
        }
        litSecSize = (nlit < 32) ? 2 : (nlit < 4096 ? 3 : 4);
        done = true;
    }
    // CD, a frame's first block: the size of the section as Treeless literals, exact - the histogram says whether every byte has a code, a pass
    // over the literals gives each stream its bits (a stream: its bits and the end mark, in whole bytes).  0: not to be had, or not smaller
    // than the literals themselves
    uint32_t tlSize = 0;
    if constexpr (CD) {
        const uint32_t lhSize = 3 + (nlit >= 1024) + (nlit >= 16384);
        const bool single = nlit < 256;
        if (!done && cdt && nlit > 0 && !ZS_STOPPED && cdt->hufLog) {
            const uint32_t cn = cdt->hufCodeNb[tid];
            L.nbBits[tid] = (uint8_t)(cn >> 16);                         // (free until the code lengths are made)
            if (__syncthreads_and(L.count[tid] == 0 || (cn >> 16) != 0)) {
                const uint32_t seg = (nlit + 3) / 4;
                const uint32_t from = single ? 0u : wave * seg, len = single ? (wave == 0 ? nlit : 0u) : ((wave < 3) ? seg : nlit - 3 * seg);
                uint32_t bits = 0;
                for (uint32_t j = 4 * lane; j < len; j += 256) {
                    if (j + 4 <= len) { const uint32_t w = zs_load32(litp + from + j); bits += L.nbBits[w & 0xFFu] + L.nbBits[(w >> 8) & 0xFFu] + L.nbBits[(w >> 16) & 0xFFu] + L.nbBits[w >> 24]; }
                    else for (uint32_t q = j; q < len; q++) bits += L.nbBits[litp[from + q]];
                }
                bits = wave_sum(bits);
                if (lane == 0) L.misc[8 + wave] = (bits + 8u) >> 3;
                __syncthreads();
                const uint32_t csz = single ? L.misc[8] : 6u + L.misc[8] + L.misc[9] + L.misc[10] + L.misc[11];
                if (lhSize + csz <= cap && csz + lhSize < nlit + (3 - (nlit < 32) - (nlit < 4096)) && (single || csz >= 10)) tlSize = lhSize + csz;
            }
            __syncthreads();
        }
    }
    if (!done && nlit >= 64 && !flatCounts) {
        const uint32_t tableLog = huffLengths(L, maxSym, ZS_HUF_MAXBITS);
        if (ZS_STOP_AT(2)) FINISH(0, 0, 0);    // stop after the code lengths
        const uint32_t lhSize = 3 + (nlit >= 1024) + (nlit >= 16384);
        const bool single = nlit < 256;
        // The code lengths say how many bits the streams will hold: when the section cannot come out smaller than the literals themselves
        // (noise, packed data: 8 bits a symbol) the codes, the table description and the four streams are not made at all - the same
        // outcome as the size test behind them (the streams are at least their bits, the description at least a byte), 0.37 -> 0.15 ms a
        // launch of 4096 blocks of noise
        {
            const uint32_t mine = (tid <= maxSym) ? L.count[tid] * (uint32_t)L.nbBits[tid] : 0u;
            const uint32_t ws = wave_sum(mine);
            if (lane == 0) L.misc[12 + wave] = ws;
            __syncthreads();
        }
        const uint32_t codeBits = L.misc[12] + L.misc[13] + L.misc[14] + L.misc[15];
        const bool hopeless = lhSize + 1u + (single ? 0u : 6u) + (codeBits >> 3) >= nlit + (3 - (nlit < 32) - (nlit < 4096));
        // CD: a section of this block's own code holds at least its header, a description of two bytes and the code's bits; where the Treeless
        // section is smaller than that, it is smaller than whatever would be made here
        bool beaten = false;
        if constexpr (CD) beaten = tlSize && tlSize < lhSize + 2u + (single ? 0u : 6u) + (codeBits >> 3);
        if (!hopeless && !beaten) {
        huffCodesAndWeights(L, maxSym, tableLog);
        if (wave == 0) { const uint32_t hs_ = writeHuffHeaderWave(L, payload + lhSize, cap - lhSize, maxSym, tableLog); if (lane == 0) L.misc[0] = hs_; }
        __syncthreads();
        const uint32_t hsz = L.misc[0];
        if (ZS_STOP_AT(3)) FINISH(0, 0, 0);    // stop after codes + table description
        if (hsz) {
            const uint32_t seg = (nlit + 3) / 4;
            if (single) { if (wave == 0) { const uint32_t z = huffEncodeStream(L, L.u.tile[0], streams, litp, 0, nlit); if (lane == 0) L.misc[8] = z; } }
            else {
                const uint32_t len = (wave < 3) ? seg : nlit - 3 * seg;
                const uint32_t z = huffEncodeStream(L, L.u.tile[wave], zs_stream(streams, wave), litp, wave * seg, len);
                if (lane == 0) L.misc[8 + wave] = z;
            }
            __syncthreads();
            const uint32_t ssz0 = L.misc[8], ssz1 = single ? 0 : L.misc[9], ssz2 = single ? 0 : L.misc[10], ssz3 = single ? 0 : L.misc[11];
            const bool ok = single || (ssz0 <= 65535 && ssz1 <= 65535 && ssz2 <= 65535 && ssz3 <= 65535);
            const uint32_t csz = hsz + (single ? ssz0 : 6 + ssz0 + ssz1 + ssz2 + ssz3);
            if (ok && lhSize + csz <= cap && csz + lhSize < nlit + (3 - (nlit < 32) - (nlit < 4096)) && (single || csz >= 10)) {
                uint8_t *op = payload + lhSize + hsz;
                if (!single) {
                    if (tid == 0) { op[0] = (uint8_t)ssz0; op[1] = (uint8_t)(ssz0 >> 8); op[2] = (uint8_t)ssz1; op[3] = (uint8_t)(ssz1 >> 8); op[4] = (uint8_t)ssz2; op[5] = (uint8_t)(ssz2 >> 8); }
                    op += 6;
                }
                const uint32_t ssz[4] = { ssz0, ssz1, ssz2, ssz3 };
                for (uint32_t k = 0; k < (single ? 1u : 4u); k++) {
                    const uint8_t *from = zs_stream(streams, k);
                    zs_block_copy(op, from, ssz[k], tid, 256);
                    op += ssz[k];
                }
                if (tid == 0) {
                    if (lhSize == 3) { const uint32_t h = 2 + ((single ? 0u : 1u) << 2) + (nlit << 4) + (csz << 14); payload[0] = (uint8_t)h; payload[1] = (uint8_t)(h >> 8); payload[2] = (uint8_t)(h >> 16); }
                    else if (lhSize == 4) { const uint32_t h = 2 + (2 << 2) + (nlit << 4) + (csz << 18); payload[0] = (uint8_t)h; payload[1] = (uint8_t)(h >> 8); payload[2] = (uint8_t)(h >> 16); payload[3] = (uint8_t)(h >> 24); }
                    else { const uint32_t h = 2 + (3 << 2) + (nlit << 4) + (csz << 22); payload[0] = (uint8_t)h; payload[1] = (uint8_t)(h >> 8); payload[2] = (uint8_t)(h >> 16); payload[3] = (uint8_t)(h >> 24); payload[4] = (uint8_t)(csz >> 10); }
                }
                litSecSize = lhSize + csz;
                done = true;
            }
        }
        }
    }
    if constexpr (CD) {
        if (tlSize && (!done || tlSize < litSecSize)) {                // (no section of its own: raw literals, larger by tlSize's making)
            // the streams under the dictionary's codes, as the section above lays them out, behind no description
            const uint32_t lhSize = 3 + (nlit >= 1024) + (nlit >= 16384);
            const bool single = nlit < 256;
            L.codeNb[tid] = cdt->hufCodeNb[tid];
            done = false;
            __syncthreads();
            const uint32_t seg = (nlit + 3) / 4;
            if (single) { if (wave == 0) { const uint32_t z = huffEncodeStream(L, L.u.tile[0], streams, litp, 0, nlit); if (lane == 0) L.misc[8] = z; } }
            else {
                const uint32_t len = (wave < 3) ? seg : nlit - 3 * seg;
                const uint32_t z = huffEncodeStream(L, L.u.tile[wave], zs_stream(streams, wave), litp, wave * seg, len);
                if (lane == 0) L.misc[8 + wave] = z;
            }
            __syncthreads();
            const uint32_t ssz0 = L.misc[8], ssz1 = single ? 0 : L.misc[9], ssz2 = single ? 0 : L.misc[10], ssz3 = single ? 0 : L.misc[11];
            const bool ok = single || (ssz0 <= 65535 && ssz1 <= 65535 && ssz2 <= 65535 && ssz3 <= 65535);
            const uint32_t csz = (single ? ssz0 : 6 + ssz0 + ssz1 + ssz2 + ssz3);
            if (ok && lhSize + csz <= cap && csz + lhSize < nlit + (3 - (nlit < 32) - (nlit < 4096)) && (single || csz >= 10)) {
                uint8_t *op = payload + lhSize;
                if (!single) {
                    if (tid == 0) { op[0] = (uint8_t)ssz0; op[1] = (uint8_t)(ssz0 >> 8); op[2] = (uint8_t)ssz1; op[3] = (uint8_t)(ssz1 >> 8); op[4] = (uint8_t)ssz2; op[5] = (uint8_t)(ssz2 >> 8); }
                    op += 6;
                }
                const uint32_t ssz[4] = { ssz0, ssz1, ssz2, ssz3 };
                for (uint32_t k = 0; k < (single ? 1u : 4u); k++) {
                    const uint8_t *from = zs_stream(streams, k);
                    zs_block_copy(op, from, ssz[k], tid, 256);
                    op += ssz[k];
                }
                if (tid == 0) {
                    if (lhSize == 3) { const uint32_t h = 3 + ((single ? 0u : 1u) << 2) + (nlit << 4) + (csz << 14); payload[0] = (uint8_t)h; payload[1] = (uint8_t)(h >> 8); payload[2] = (uint8_t)(h >> 16); }
                    else if (lhSize == 4) { const uint32_t h = 3 + (2 << 2) + (nlit << 4) + (csz << 18); payload[0] = (uint8_t)h; payload[1] = (uint8_t)(h >> 8); payload[2] = (uint8_t)(h >> 16); payload[3] = (uint8_t)(h >> 24); }
                    else { const uint32_t h = 3 + (3 << 2) + (nlit << 4) + (csz << 22); payload[0] = (uint8_t)h; payload[1] = (uint8_t)(h >> 8); payload[2] = (uint8_t)(h >> 16); payload[3] = (uint8_t)(h >> 24); payload[4] = (uint8_t)(csz >> 10); }
                }
                litSecSize = lhSize + csz;
                done = true;
            }
        }
    }
    if (!done) {
        const uint32_t lh = 1 + (nlit > 31) + (nlit > 4095);
        if (tid == 0) {
            if (lh == 1) payload[0] = (uint8_t)(nlit << 3);
            else if (lh == 2) { const uint32_t h = (1 << 2) + (nlit << 4); payload[0] = (uint8_t)h; payload[1] = (uint8_t)(h >> 8); }
            else { const uint32_t h = (3 << 2) + (nlit << 4); payload[0] = (uint8_t)h; payload[1] = (uint8_t)(h >> 8); payload[2] = (uint8_t)(h >> 16); }
        }
        zs_block_copy(payload + lh, litp, nlit, tid, 256);
        litSecSize = lh + nlit;
    }
    FINISH(2, litSecSize, 0);
    #undef FINISH
}
// liveBlocks (a plan built on the device, plan_kernels.hip: the grid is the host's upper bound): the blocks the list holds - a workgroup at
// or beyond them leaves.  Null: the grid is the list
template <bool CD>
__global__ void __launch_bounds__(256, ZS_LIT_MINWG) k_encode_literals(ZS_LIT_PARAMS, const ZsCDictEntry *__restrict__ dictTab, const uint32_t *__restrict__ chunkDict,
                                                                       const uint32_t *__restrict__ liveBlocks)
{
    if (liveBlocks && blockIdx.x >= *liveBlocks) return;
    encode_literals_block<CD>(ZS_LIT_ARGS, dictTab, chunkDict);
}

// ---------------------------------------------------------------------------------------------
// k_encode_sequences : one wavefront per block.  Repcodes (parallel: two last-index scans), code
// histograms, tables (normalisation and encoding tables built by all lanes), bitstream
// -> seqSec[], meta.seqSecSize
// ---------------------------------------------------------------------------------------------
#ifndef ZS_SEQ_GROUP
#define ZS_SEQ_GROUP 4             // blocks (= wavefronts) per workgroup of the sequences kernel
#endif
#ifndef ZS_SEQ_TB
#define ZS_SEQ_TB 4                // tiles of 64 sequences whose records are requested together (pass 1, packing)
#endif
#ifndef ZS_CHAIN_WARM
#define ZS_CHAIN_WARM 512u         // steps a chain segment starts ahead of its first output (a multiple of 16)
#endif
#ifndef ZS_CHAIN_MAXSEG
#define ZS_CHAIN_MAXSEG 21u        // most segments a chain is cut in (3 chains a wavefront: <= 21)
#endif
#ifndef ZS_CHAIN_MINSEG
#define ZS_CHAIN_MINSEG 4u         // shortest segment, in blocks of 16 steps
#endif
// (dictTab, chunkDict: as k_encode_literals'.  A chunk's first block starts from its record's recent offsets, {1, 4, 8} without one)
#define ZS_SEQ_PARAMS const ZsBlockDesc *__restrict__ blocks, uint32_t nBlocks, const ZsSeqRec *__restrict__ seqAll, const uint32_t *__restrict__ hdrAll, \
                      uint8_t *__restrict__ seqSecAll, ZsBlockMeta *__restrict__ metas, int stopAt, uint8_t *__restrict__ litsAll, uint8_t *__restrict__ streamAll, \
                      uint2 *__restrict__ packRecAll
#define ZS_SEQ_ARGS blocks, nBlocks, seqAll, hdrAll, seqSecAll, metas, stopAt, litsAll, streamAll, packRecAll
// CD (a digested dictionary's tables in cdt, the record's; none: nullptr): for the first block of a frame each of LL / OF / ML is coded in
// Repeat_Mode (3) with the dictionary's table iff that table codes every code present and its estimate, the sum of count x cost, is strictly
// below the estimate of what the rules below pick: RLE one byte, the predefined table its own sum of count x cost, a new table its
// description's bytes plus that sum over its normalised counts (in 1/256 bit throughout)
template <int G, bool CD>
__device__ __forceinline__ void encode_sequences_block(ZS_SEQ_PARAMS, const ZsCDictEntry *__restrict__ dictTab, const uint32_t *__restrict__ chunkDict)
{
    __shared__ SeqLds LS[G];
    const uint32_t wave = threadIdx.x >> 6;
    SeqLds &L = LS[wave];
    const uint32_t blk = blockIdx.x * G + wave;
    const uint32_t lane = (uint32_t)zs_lane();
    const bool exists = blk < nBlocks;
    const ZsBlockDesc bd = blocks[exists ? blk : 0];
    // A frame's first block reads its chunk's record (the wavefront's one address; none: ZS_DICT_NONE): its recent offsets where pass 1 starts from
    // them ({1, 4, 8} without a record), and, CD, its tables - no tables: cdt stays null and the block is coded as by the form without CD
    const uint32_t dictEntry = (dictTab && bd.firstInChunk) ? (uint32_t)__builtin_amdgcn_readfirstlane((int)(chunkDict ? chunkDict[bd.chunk] : 0u)) : ZS_DICT_NONE;
    const ZsCDictTables *__restrict__ cdt = nullptr;
    if constexpr (CD) { if (dictEntry != ZS_DICT_NONE) cdt = dictTab[dictEntry].tables; }
    const uint32_t n = bd.size;
    const ZsSeqRec *seqBase = zs_block_seqs(seqAll, blk);
    uint8_t *out = zs_block_seq_section(seqSecAll, blk);
    const uint32_t cap = n + 512;
    // scratch of part 2's state chains and of the packing, borrowed (zsmi_scratch.h says from whom and until when)
    uint8_t *chainCodes = zs_lits_lend_chain_codes(litsAll, blk);
    uint16_t *chainOuts = zs_streams_lend_chain_outs(streamAll, blk);
    uint2 *packRec = zs_dist_lend_pack_records(packRecAll, blk);

    // ======== part 1, each wavefront on its own block (no workgroup barrier inside): header, recent-offset codes,
    //          histograms, tables.  result: section size so far / 0xFFFFFFFF = no compressed sequences section ========
    uint32_t result = 0xFFFFFFFFu, nseq = 0, bitstreamOff = 0;
    uint32_t secHdr = 0xFFFFFFFFu, secGap = 0;        // where the bitstream lies behind the headers (0xFFFFFFFF: no bitstream, the section is all headers)
    bool live = false;                                  // this wavefront has a bitstream to write in part 2
    do {
        if (!exists || n < 16) break;
        nseq = (uint32_t)__builtin_amdgcn_readfirstlane((int)zs_block_hdr(hdrAll, blk).nseq);
        for (uint32_t i = lane; i < 192; i += 64) L.count[i] = 0;
        wave_sync();

        // ---- sequences section header (inverse of DecodeSeqHeaders, ZStdDecompress.cs:1110-1180) ----
        uint32_t hdrBytes = (nseq < 128) ? 1 : (nseq < 0x7F00 ? 2 : 3);
        if (lane == 0) {
            if (nseq < 128) out[0] = (uint8_t)nseq;
            else if (nseq < 0x7F00) { out[0] = (uint8_t)((nseq >> 8) + 0x80); out[1] = (uint8_t)nseq; }
            else { out[0] = 0xFF; out[1] = (uint8_t)(nseq - 0x7F00); out[2] = (uint8_t)((nseq - 0x7F00) >> 8); }
        }
        if (nseq == 0) { result = hdrBytes; break; }

        // ---- pass 1: recent-offset codes + code histograms.  Rules (inverse of ZStdDecompress.cs:1509-1530):
        //   the state changes unless (ll > 0 and off == rep0); a change gives [off, rep0, off == rep1 ? rep2 : rep1].
        //   rep0 before a sequence is always the previous sequence's offset, so
        //   rep1 = previous offset of the last changing sequence, rep2 = rep1 as seen by the last changing sequence
        //   whose offset differed from its rep1: two "last index below me" scans per 64 sequences. ----
        {
            uint32_t cPrev, cA, cB;                       // carried: previous offset (= rep0), rep1, rep2
            if (!bd.firstInChunk) { cPrev = 0xFFFFFFF1u; cA = 0xFFFFFFF2u; cB = 0xFFFFFFF3u; }
            else if (dictEntry == ZS_DICT_NONE) { cPrev = 1u; cA = 4u; cB = 8u; }
            else { const ZsCDictEntry &de = dictTab[dictEntry]; cPrev = de.rep[0]; cA = de.rep[1]; cB = de.rep[2]; }
            uint32_t cEnd = 0;                            // carried: where the sequence before ends in the block (its literals start there)
            // tile t is the records [64 t, 64 t + 64) of the block's list; the records of the next tiles are loaded while these are worked on
            // (a record travels as its two raw words and is taken apart only where it is used: unpacked next to the load, the
            // compiler waits for the load on the spot).  ZS_SEQ_TB tiles of 64 are requested together and worked through one after the other:
            // a request a tile was a memory round trip a tile (the kernel's wavefronts spent half their time in s_waitcnt).
            constexpr uint32_t TB = ZS_SEQ_TB;
            uint2 rawN[TB];
            auto request = [&](uint32_t base) {
                #pragma unroll
                for (uint32_t t = 0; t < TB; t++) {
                    const uint32_t g = base + 64u * t + lane;
                    rawN[t] = make_uint2(0, 0);
                    if (g < nseq) rawN[t] = *reinterpret_cast<const uint2 *>(seqBase + g);
                }
            };
            request(0);
            #pragma unroll
            for (uint32_t t = 0; t < TB; t++) asm volatile("" : "+v"(rawN[t].x), "+v"(rawN[t].y));     // the first records are waited for here, not inside the loop
            for (uint32_t base0 = 0; base0 < nseq; base0 += 64u * TB) {
                uint2 rawC[TB];
                #pragma unroll
                for (uint32_t t = 0; t < TB; t++) rawC[t] = rawN[t];
                if (base0 + 64u * TB < nseq) request(base0 + 64u * TB);
                #pragma unroll
                for (uint32_t t = 0; t < TB; t++) {
                const uint32_t base = base0 + 64u * t;
                if (base >= nseq) break;
                const uint32_t g = base + lane;
                const bool in = g < nseq;
                const uint2 raw = rawC[t];
                uint32_t off = 0, ll = 0, ml = 0, st = 0;
                if (in) { off = zs_rec_off(raw.x, raw.y); ml = zs_rec_ml(raw.x); st = zs_rec_pos(raw.y); }
                const uint32_t end = st + ml;
                uint32_t prevEnd = ZS_DPP(0, end, 0x138, 0xF, true); if (lane == 0) prevEnd = cEnd;  // wave_shr:1        // where the sequence before me ends
                if (in) ll = st - prevEnd;                                                            // the literals in front of me, however many
                uint32_t prev = ZS_DPP(0, off, 0x138, 0xF, true); if (lane == 0) prev = cPrev;      // wave_shr:1        // rep0 before me
                const bool change = in && !(ll > 0 && off == prev);
                const int j = lastFlagBelow(change);                                                  // last changing sequence before me
                const uint32_t aSh = (uint32_t)__shfl((int)prev, max(j, 0));                          // every lane takes part: a source lane must be active
                const uint32_t a = (j >= 0) ? aSh : cA;                                               // rep1 before me
                const bool reset = change && (off != a);                                              // sequences after which rep2 = their rep1
                const int kk = lastFlagBelow(reset);
                const uint32_t bSh = (uint32_t)__shfl((int)a, max(kk, 0));
                const uint32_t b = (kk >= 0) ? bSh : cB;                                              // rep2 before me
                if (in) {
                    uint32_t val;
                    if (ll) { val = (off == prev) ? 1u : (off == a) ? 2u : (off == b) ? 3u : 0u; }
                    else    { val = (off == a) ? 1u : (off == b) ? 2u : 0u; }
                    const uint32_t v = val ? val : off + 3;
                    const uint32_t llc = llCodeOf(ll), ofc = zs_highbit(v), mlc = mlCodeOf(ml - 3);
                    atomicAdd(&L.count[llc], 1u);
                    atomicAdd(&L.count[64 + ofc], 1u);
                    atomicAdd(&L.count[128 + mlc], 1u);
                    // for part 2, in encoding order (last sequence first): the codes the state chains walk along, and the sequence's extra bits
                    // as they follow its three state outputs in the stream (literal length, match length, offset: <= 16 + 16 + 17 bits) with their count
                    const uint32_t je = nseq - 1u - g;
                    chainCodes[je] = (uint8_t)llc; chainCodes[ZS_CHAIN_CODES + je] = (uint8_t)ofc; chainCodes[2u * ZS_CHAIN_CODES + je] = (uint8_t)mlc;
                    uint32_t xbL, xbM;
                    const uint32_t xvL = llExtraOf(ll, xbL), xvM = mlExtraOf(ml - 3, xbM);
                    const uint64_t E = (uint64_t)xvL | ((uint64_t)xvM << xbL) | ((uint64_t)(v - (1u << ofc)) << (xbL + xbM));
                    packRec[je] = make_uint2((uint32_t)E, (uint32_t)(E >> 32) | ((xbL + xbM + ofc) << 24));
                }
                // carries for the next 64: state after the last sequence of this batch
                const uint32_t cnt = min(64u, nseq - base);
                const uint64_t chm = __ballot(change), rsm = __ballot(reset);
                const uint32_t lastOff = wave_get(off, (int)(cnt - 1));
                if (chm) { const int jl = 63 - __builtin_clzll(chm); cA = wave_get(prev, jl); }
                if (rsm) { const int kl = 63 - __builtin_clzll(rsm); cB = wave_get(a, kl); }
                cPrev = lastOff; cEnd = wave_get(end, (int)(cnt - 1));
                }
            }
        }
        wave_sync();
        if (ZS_STOP_AT(1)) break;                         // timing aid (ZSMI_STOP_SEQ): stop after repcodes + histograms

        // ---- modes and tables ----
        uint32_t pos = hdrBytes + 1;                        // after nbSeq and the modes byte
        uint32_t modeByte = 0;
        bool fail = false;
        // (CD) the dictionary's table t beats an estimate of est: it is loaded in place of the one that would be built
        auto repeatBeats = [&](uint32_t t, uint32_t c, uint32_t est) -> bool {
            const uint32_t dc = cdt->cost[t][lane];
            if (__any(c != 0 && dc == ZS_COST_NONE)) return false;
            if (wave_sum(c * dc) >= est) return false;
            const uint32_t *from = reinterpret_cast<const uint32_t *>(&cdt->ct[t]); uint32_t *to = reinterpret_cast<uint32_t *>(&L.ct[t]);
            for (uint32_t i = lane; i < sizeof(FseCT) / 4; i += 64) to[i] = from[i];
            return true;
        };
        #pragma unroll 1
        for (uint32_t t = 0; t < 3; t++) {
            const uint32_t *count = L.count + 64 * t;
            const uint32_t maxCode = t == 0 ? MaxLL : (t == 1 ? MaxOff : MaxML);
            const uint32_t maxLog = t == 0 ? LLFSELog : (t == 1 ? OffFSELog : MLFSELog);
            const uint32_t defLog = t == 0 ? LL_defaultNormLog : (t == 1 ? OF_defaultNormLog : ML_defaultNormLog), defMax = t == 0 ? MaxLL : (t == 1 ? DefaultMaxOff : MaxML);
            FseCT &ct = L.ct[t];
            const uint32_t c = (lane <= maxCode) ? count[lane] : 0u;
            const uint64_t present = __ballot(c != 0);
            const uint32_t maxSym = 63u - (uint32_t)__builtin_clzll(present);       // nseq > 0: at least one symbol
            const uint32_t largest = wave_max(c);
            uint32_t mode;
            if (largest == nseq) {
                mode = 1;
                if (pos >= cap) { fail = true; break; }
                if constexpr (CD) { if (cdt && repeatBeats(t, c, 8u * 256u)) mode = 3; }
                if (mode == 1) {
                if (lane == 0) { out[pos] = (uint8_t)maxSym; ct.rle = 1; ct.tableLog = 0; }
                pos += 1;
                }
            } else if (nseq < 64 && maxSym <= defMax) {
                mode = 0;
                if constexpr (CD) {
                    if (cdt) {
                        const int16_t *defNorm = t == 0 ? LL_defaultNorm : (t == 1 ? OF_defaultNorm : ML_defaultNorm);
                        const int nv = lane <= defMax ? defNorm[lane] : 1;
                        if (repeatBeats(t, c, wave_sum(c * fseSymbolCost((uint32_t)(nv < 0 ? 1 : nv), defLog)))) mode = 3;
                    }
                }
                if (mode == 0) buildCTableWave(L.u.build, ct, t == 0 ? LL_defaultNorm : (t == 1 ? OF_defaultNorm : ML_defaultNorm), defMax, defLog);
            } else {
                uint32_t tableLog = maxLog;
                { const uint32_t hb = zs_highbit(nseq - 1); const uint32_t want = hb > 2 ? hb - 2 : 5; if (want < tableLog) tableLog = want; }
                { const uint32_t minBits = zs_highbit(maxSym) + 2; const uint32_t npresent = (uint32_t)__popcll(present);
                  if (tableLog < minBits) tableLog = minBits; while ((1u << tableLog) < npresent) tableLog++; }
                if (tableLog < 5) tableLog = 5;
                if (tableLog > maxLog) tableLog = maxLog;
                normalizeCountsWave(L.norm, tableLog, count, nseq, maxSym);
                if (lane == 0) L.misc[0] = writeNCount(out + pos, cap - pos, L.norm, maxSym, tableLog);
                wave_sync();
                const uint32_t h = L.misc[0];
                if (!h) { fail = true; break; }
                mode = 2;
                if constexpr (CD) {
                    if (cdt && repeatBeats(t, c, h * 8u * 256u + wave_sum(c ? c * fseSymbolCost((uint32_t)L.norm[lane], tableLog) : 0u))) mode = 3;
                }
                if (mode == 2) {
                pos += h;
                buildCTableWave(L.u.build, ct, L.norm, maxSym, tableLog);
                }
            }
            modeByte |= mode << (6 - 2 * t);
            wave_sync();
        }
        if (fail) break;
        if (ZS_STOP_AT(2)) break;                         // stop after the tables
        if (lane == 0) out[hdrBytes] = (uint8_t)modeByte;
        bitstreamOff = pos;
        live = true;
    } while (0);

    // ======== part 2: sequences bitstream (inverse of ZStdDecompress.cs:1473-1608), last sequence first; each wavefront on its own block,
    //   no workgroup barrier.  An FSE state chain is a dependent table look-up per sequence (~3600 a block and table), and the format fixes
    //   ONE chain per table.  But chains over the same symbols COUPLE: started from any state they agree with the true chain after some
    //   steps for good (a step keeps state >> nbBits: tools/lab/coupling.c measures half of them coupled after 60 steps, 99.5 % after 512 on
    //   the Zipf log, 96.5 % on the mixed corpus).  So a table's chain is cut in K <= 21 SEGMENTS of whole blocks of 16 steps; lane c K + k runs
    //   segment k of table c, started ZS_CHAIN_WARM steps early from the state its first symbol alone gives (the rule of the block's true
    //   first step), silent until its own segment begins; then the seams are checked in order - entry state of segment k == exit
    //   state of segment k - 1 - and a segment that fails is run again from the right state (its outputs overwritten) before the
    //   next seam is looked at, so the result is exactly the serial chain's.  63 lanes run ~(nseq / K + 512) steps instead of 3 lanes nseq.
    //   Codes come from pass 1 (a byte a step and table, in encoding order), outputs go to scratch as 16 bits a step
    //   (state bits | count << 12); both live in the literals kernel's scratch (streams, literals), which that kernel writes after this one.
    //   Then the tiles of 64 sequences are packed, all lanes. ========
    uint8_t *bsTmp = out + ((bitstreamOff + 3u) & ~3u);                // aligned start inside the section buffer
    BitSink sink; sink_init(sink, bsTmp, L.tile);
    const uint32_t bsCap = ZS_SEQSEC_STRIDE - ((bitstreamOff + 3u) & ~3u) - 1024u;
    bool overflow = false;
    if (live && !ZS_STOP_AT(3)) {                                      // stopAt 3: timing aid, no chains
        const uint32_t nFull = nseq >> 4, tail = nseq & 15u;           // whole blocks of 16 steps; the steps behind them belong to the last segment
        uint32_t Sb = max((nFull + ZS_CHAIN_MAXSEG - 1u) / ZS_CHAIN_MAXSEG, (uint32_t)ZS_CHAIN_MINSEG);   // blocks a segment
        const uint32_t K = max((nFull + Sb - 1u) / Sb, 1u);            // segments a chain (<= 21)
        const uint32_t c = (lane >= K ? 1u : 0u) + (lane >= 2u * K ? 1u : 0u), k = lane - c * K;
        const bool chainLane = lane < 3u * K && !L.ct[min(c, 2u)].rle;
        const FseCT &ct = L.ct[min(c, 2u)];
        const uint8_t *codes = chainCodes + (size_t)min(c, 2u) * ZS_CHAIN_CODES;
        uint16_t *outs = chainOuts + (size_t)min(c, 2u) * ZS_CHAIN_CODES;
        typedef const __attribute__((address_space(3))) uint16_t *LdsU16;
        typedef const __attribute__((address_space(3))) uint32_t *LdsU32;
        // a code's two operands in one word: deltaNbBits < 2^20 (a state added to it stays below), deltaFindState + 1024 in the bits above
        #pragma unroll
        for (uint32_t t = 0; t < 3; t++) L.u.chain.op[t][lane] = L.ct[t].deltaNbBits[lane] | ((uint32_t)(L.ct[t].deltaFindState[lane] + 1024) << 20);
        wave_sync();
        const uint32_t tabAddr = (uint32_t)(uintptr_t)(LdsU16)ct.stateTable - 2048u, opAddr = (uint32_t)(uintptr_t)(LdsU32)L.u.chain.op[min(c, 2u)];
        const uint32_t firstOut = k * Sb, bEnd = min(firstOut + Sb, nFull);
        const bool lastSeg = k + 1u == K;
        const uint32_t bWarm = firstOut > ZS_CHAIN_WARM / 16u ? firstOut - ZS_CHAIN_WARM / 16u : 0u;
        // one step: the state's low bits leave (their count from the sum's high half), the rest picks the next state from the symbol's stretch of the table
        #define CHAIN_STEP(sym, o) { \
            const uint32_t op_ = *(LdsU32)(uintptr_t)(opAddr + ((sym) << 2)); \
            const uint32_t nbo_ = __builtin_amdgcn_ubfe(state + op_, 16, 4); \
            (o) = __builtin_amdgcn_ubfe(state, 0, nbo_) | (nbo_ << 12); \
            state = *(LdsU16)(uintptr_t)(tabAddr + (((state >> nbo_) + (op_ >> 20)) << 1)); }
        // the blocks [from, to) with the state carried; outputs stored for blocks >= outFrom; entry: the state in front of block `mark`.
        // Loads and stores share the wavefront's vmcnt, and the compiler waits vmcnt(0) for a load it sees - behind a round's stores that is their
        // whole trip to L2, every round.  So the codes of round r + 1 are requested BEFORE round r's two stores, by a load the compiler does not
        // see, and waited for by count: vmcnt(2) leaves exactly those stores in flight (in-order return: DESIGN section 6).  For the count to
        // hold every lane stores every round - where it has nothing to store, into a junk slot of the section buffer (written by the packing later).
        typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
        uint8_t *junk = zs_seqsec_lend_junk_store(out, lane);
        auto runBlocks = [&](uint32_t from, uint32_t to, uint32_t outFrom, uint32_t mark, uint32_t &state, uint32_t &entry, uint32_t rounds) {
            u32x4 cw;
            {
                const uint8_t *a0 = codes + 16u * min(from, nFull ? nFull - 1u : 0u);
                asm volatile("global_load_dwordx4 %0, %1, off\n\ts_waitcnt vmcnt(0)" : "=&v"(cw) : "v"(a0) : "memory");
            }
            for (uint32_t it = 0; it < rounds; it++) {
                const uint32_t blkI = from + it;
                const bool act = blkI < to;
                const u32x4 cur = cw;
                {
                    const uint8_t *a1 = codes + 16u * min(blkI + 1u, nFull ? nFull - 1u : 0u);
                    asm volatile("global_load_dwordx4 %0, %1, off" : "=&v"(cw) : "v"(a1) : "memory");
                }
                if (act && blkI == mark) entry = state;
                uint32_t o[16] = {};
                if (act) {
                    const uint32_t w4[4] = { cur.x, cur.y, cur.z, cur.w };
                    #pragma unroll
                    for (uint32_t t = 0; t < 16; t++) { const uint32_t sym = (w4[t >> 2] >> (8u * (t & 3u))) & 0xFFu; CHAIN_STEP(sym, o[t]) }
                }
                uint4 *op_ = reinterpret_cast<uint4 *>((act && blkI >= outFrom) ? reinterpret_cast<uint8_t *>(outs + 16u * blkI) : junk);
                op_[0] = make_uint4(o[0] | (o[1] << 16), o[2] | (o[3] << 16), o[4] | (o[5] << 16), o[6] | (o[7] << 16));
                op_[1] = make_uint4(o[8] | (o[9] << 16), o[10] | (o[11] << 16), o[12] | (o[13] << 16), o[14] | (o[15] << 16));
                asm volatile("s_waitcnt vmcnt(2)" : "+v"(cw) :: "memory");
            }
        };
        // the same without outputs (a segment's warm-up: most of a lane's steps): lanes run the LAST `n` of `rounds` rounds, blocks [to - n, to)
        auto warmBlocks = [&](uint32_t to, uint32_t n, uint32_t &state, uint32_t rounds) {
            u32x4 cw;
            {
                const uint8_t *a0 = codes + 16u * min(to - n, nFull ? nFull - 1u : 0u);
                asm volatile("global_load_dwordx4 %0, %1, off\n\ts_waitcnt vmcnt(0)" : "=&v"(cw) : "v"(a0) : "memory");
            }
            for (uint32_t it = 0; it < rounds; it++) {
                const bool act = it + n >= rounds;                      // my first round is rounds - n
                const uint32_t blkI = to - rounds + it;                 // (meaningful where act)
                const u32x4 cur = cw;
                {
                    const uint8_t *a1 = codes + 16u * (act ? min(blkI + 1u, nFull ? nFull - 1u : 0u) : min(to - n, nFull ? nFull - 1u : 0u));
                    asm volatile("global_load_dwordx4 %0, %1, off" : "=&v"(cw) : "v"(a1) : "memory");
                }
                if (act) {
                    const uint32_t w4[4] = { cur.x, cur.y, cur.z, cur.w };
                    #pragma unroll
                    for (uint32_t t = 0; t < 16; t++) {
                        const uint32_t sym = (w4[t >> 2] >> (8u * (t & 3u))) & 0xFFu;
                        const uint32_t op_ = *(LdsU32)(uintptr_t)(opAddr + (sym << 2));
                        const uint32_t nbo_ = __builtin_amdgcn_ubfe(state + op_, 16, 4);
                        state = *(LdsU16)(uintptr_t)(tabAddr + (((state >> nbo_) + (op_ >> 20)) << 1));
                    }
                }
                asm volatile("s_waitcnt vmcnt(0)" : "+v"(cw) :: "memory");
            }
        };
        auto runTail = [&](uint32_t &state) {                           // the steps behind the whole blocks, one by one
            for (uint32_t t = 0; t < tail; t++) { const uint32_t sym = codes[16u * nFull + t]; uint32_t o; CHAIN_STEP(sym, o) outs[16u * nFull + t] = (uint16_t)o; }
        };
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");          // pass 1's code bytes (other lanes' stores) are read below
#ifdef ZS_CHAIN_COUNT
        if (lane == 0) { zs_meta_lend_chain_counts(metas, blk).pad[0] = 0; zs_meta_lend_chain_counts(metas, blk).pad[1] = K | (Sb << 8) | (nseq << 16); }
#endif
        uint32_t state = 0, entry = 0;
        const bool runs = chainLane && (firstOut < nFull || k == 0);
        if (runs) {
            // the first step of a chain takes its state from the symbol alone (ZStdCompress' first-symbol rule; the decoder's final state); as a
            // step from a made-up state: nbBits = (deltaNbBits + 2^15) >> 16, state = (nbBits << 16) - deltaNbBits
            const uint32_t sym0 = codes[16u * bWarm];
            const uint32_t dnb0 = ct.deltaNbBits[sym0], nb0 = (dnb0 + (1u << 15)) >> 16;
            state = (nb0 << 16) - dnb0;
        }
        const uint32_t warmN = runs ? firstOut - bWarm : 0u;            // silent blocks in front of my segment
        const uint32_t warmRounds = wave_max(warmN), rounds = wave_max(runs ? bEnd - firstOut : 0u);
        if (warmRounds) warmBlocks(firstOut, warmN, state, warmRounds);
        entry = state;
        if (runs) {
            uint32_t dummy = 0;
            runBlocks(firstOut, bEnd, firstOut, 0xFFFFFFFFu, state, dummy, rounds);
            if (lastSeg && tail) runTail(state);
        }
        // the seams, in order
        for (uint32_t kk = 1; kk < K; kk++) {
            const uint32_t prevExit = ZS_DPP(0, state, 0x138, 0xF, true);           // wave_shr:1: lane c K + kk - 1
            const bool bad = runs && k == kk && entry != prevExit;
            if (__any(bad)) {
#ifdef ZS_CHAIN_COUNT
                if (lane == 0) zs_meta_lend_chain_counts(metas, blk).pad[0] += (uint32_t)__popcll(__ballot(bad)) | (1u << 16);      // development aid: seams that failed / rounds of repair
#endif
                // (a repair is the chain run serially with one to three lanes: its wavefront issues ahead of the others on its SIMD, as the shared chain
                //  wavefront of rounds 1 - 3 did)
                __builtin_amdgcn_s_setprio(3);
                if (bad) {
                    uint32_t dummy = 0;
                    state = prevExit;
                    runBlocks(firstOut, bEnd, firstOut, 0xFFFFFFFFu, state, dummy, bEnd - firstOut);
                    if (lastSeg && tail) runTail(state);
                }
                __builtin_amdgcn_s_setprio(0);
            }
        }
        #undef CHAIN_STEP
        if (chainLane && k == 0) outs[0] = 0;                           // the first step of all writes no bits
        // final states of the three tables -> misc[4..6] (an RLE table has none)
        if (lane < 3u * K && k + 1u == K) L.misc[4 + c] = state;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");          // the outputs (other lanes' stores) are read below
        wave_sync();
    }
    if (live && !ZS_STOP_AT(3) && !ZS_STOP_AT(4)) {                     // stopAt 4: timing aid, no packing
        // per sequence: the three chains' outputs of its step and its extra bits (pass 1), all in encoding order: consecutive lanes, consecutive
        // addresses.  ZS_SEQ_TB tiles are requested together (clamped, branch-free) and packed one after the other.
        constexpr uint32_t TB = ZS_SEQ_TB;
        const bool rle0 = L.ct[0].rle != 0, rle1 = L.ct[1].rle != 0, rle2 = L.ct[2].rle != 0;
        uint2 prN[TB]; uint32_t sN[TB][3];
        auto request = [&](uint32_t j0) {
            #pragma unroll
            for (uint32_t t = 0; t < TB; t++) {
                const uint32_t j = min(j0 + 64u * t + lane, nseq - 1u);
                prN[t] = packRec[j];
                sN[t][0] = chainOuts[j]; sN[t][1] = chainOuts[ZS_CHAIN_CODES + j]; sN[t][2] = chainOuts[2u * ZS_CHAIN_CODES + j];
            }
        };
        request(0);
        for (uint32_t j0 = 0; j0 < nseq && !overflow; j0 += 64u * TB) {
            uint2 pr[TB]; uint32_t sC[TB][3];
            #pragma unroll
            for (uint32_t t = 0; t < TB; t++) { pr[t] = prN[t]; sC[t][0] = sN[t][0]; sC[t][1] = sN[t][1]; sC[t][2] = sN[t][2]; }
            if (j0 + 64u * TB < nseq) request(j0 + 64u * TB);
            #pragma unroll
            for (uint32_t t = 0; t < TB; t++) {
                const uint32_t jt = j0 + 64u * t;
                if (jt >= nseq || overflow) break;
                uint64_t lo = 0; uint32_t hi = 0, nb = 0;
                if (jt + lane < nseq) {
                    const uint32_t sLL = rle0 ? 0u : sC[t][0], sOF = rle1 ? 0u : sC[t][1], sML = rle2 ? 0u : sC[t][2];
                    // the three state outputs (<= 9 bits each, nothing above their count) side by side in 32 bits, the extra bits (<= 49) behind
                    // them: no branch (huffEncodeStream's merge)
                    const uint32_t bOF = sOF >> 12, bML = sML >> 12, n3 = bOF + bML + (sLL >> 12);         // n3 <= 27
                    const uint32_t st = (sOF & 0xFFFu) | ((sML & 0xFFFu) << bOF) | ((sLL & 0xFFFu) << (bOF + bML));
                    const uint64_t x = (uint64_t)pr[t].x | ((uint64_t)(pr[t].y & 0xFFFFFFu) << 32);
                    lo = (uint64_t)st | (x << n3);
                    hi = (uint32_t)((x >> 1) >> (63u - n3));                                            // x's bits from 64 - n3 up (n3 = 0: none)
                    nb = n3 + (pr[t].y >> 24);
                }
                if (sink.bitpos / 8 + 1024 > bsCap) overflow = true;
                else sink_put(sink, lo, hi, nb);
            }
        }
    }
    if (live && !overflow) {
        {
            // final states: ML, OF, LL (ZStdDecompress.cs:1578-1580 reads LL, OF, ML)
            const uint32_t tlLL = L.ct[0].rle ? 0 : L.ct[0].tableLog;
            const uint32_t tlOF = L.ct[1].rle ? 0 : L.ct[1].tableLog;
            const uint32_t tlML = L.ct[2].rle ? 0 : L.ct[2].tableLog;
            const uint32_t stLL = L.misc[4], stOF = L.misc[5], stML = L.misc[6];
            uint64_t lo = 0; uint32_t nb = 0;
            if (lane == 0) {
                if (tlML) { lo |= (uint64_t)(stML & ((1u << tlML) - 1)) << nb; nb += tlML; }
                if (tlOF) { lo |= (uint64_t)(stOF & ((1u << tlOF) - 1)) << nb; nb += tlOF; }
                if (tlLL) { lo |= (uint64_t)(stLL & ((1u << tlLL) - 1)) << nb; nb += tlLL; }
            }
            sink_put(sink, lo, 0u, nb);
        }
        const uint32_t bsSize = sink_close(sink);
        // the stream stays where it was built (4-byte aligned, up to 3 bytes behind the headers): the frame assembly copies the two
        // pieces next to each other (moving it down here was ~160 dependent load -> store rounds per block)
        const uint32_t gap = (uint32_t)(bsTmp - (out + bitstreamOff));
        secHdr = bitstreamOff; secGap = gap;
        const uint32_t total = bitstreamOff + bsSize;
        result = total > cap ? 0xFFFFFFFFu : total;
    }
    if (lane == 0 && exists) { ZsBlockMeta &mo = zs_block_meta(metas, blk); mo.seqSecSize = result; mo.seqHdrSize = (secHdr == 0xFFFFFFFFu) ? result : secHdr; mo.seqGap = secGap; }
}
// liveBlocks: as k_encode_literals' - it stands in for nBlocks, and a workgroup none of whose G blocks is live leaves
template <int G, bool CD>
__global__ void __launch_bounds__(64 * G) k_encode_sequences(ZS_SEQ_PARAMS, const ZsCDictEntry *__restrict__ dictTab, const uint32_t *__restrict__ chunkDict,
                                                             const uint32_t *__restrict__ liveBlocks)
{
    if (liveBlocks) { nBlocks = *liveBlocks; if (blockIdx.x * G >= nBlocks) return; }
    encode_sequences_block<G, CD>(ZS_SEQ_ARGS, dictTab, chunkDict);
}

// ---------------------------------------------------------------------------------------------
// k_assemble_frames : one workgroup per chunk.  frame = magic + FHD + FCS (single segment)
// + blocks  (inverse of ZStdDecompress.cs:421-499, 646-659, 2008-2091).  A block is emitted compressed
// iff both sections exist and literal section + sequence section < block size (else raw; RLE if flagged).
// ---------------------------------------------------------------------------------------------

#define ZS_ASM_PARAMS const uint8_t *__restrict__ src, const ZsChunkDesc *__restrict__ chunks, const ZsBlockDesc *__restrict__ blocks, \
                      const ZsBlockMeta *__restrict__ metas, const uint8_t *__restrict__ litSecAll, const uint8_t *__restrict__ seqSecAll, \
                      uint32_t blockBase, uint8_t *__restrict__ dst, uint32_t *__restrict__ dstSizes, uint32_t chunkBase
// (dictTab, chunkDict: as k_encode_literals' - the dictionary ID the frame header carries is the chunk's record's, 0 without one)
extern "C" __global__ void __launch_bounds__(256) k_assemble_frames(ZS_ASM_PARAMS, const ZsCDictEntry *__restrict__ dictTab, const uint32_t *__restrict__ chunkDict)
{
    const ZsChunkDesc cd = chunks[chunkBase + blockIdx.x];
    if (cd.nBlocks <= 1) return;                               // one-block chunks were assembled by the literals kernel
    uint8_t *out = dst + cd.dstOff;
    const uint32_t tid = threadIdx.x;
    uint32_t pos = zs_frame_header(out, cd.size, tid == 0, zs_chunk_dict_id(dictTab, chunkDict, chunkBase + blockIdx.x));
    for (uint32_t b = 0; b < cd.nBlocks; b++) {
        const uint32_t gb = cd.firstBlock + b;             // global block index
        const uint32_t lb = gb - blockBase;                // index inside this sub-batch's scratch
        const ZsBlockDesc bd = blocks[gb];
        pos += zs_emit_block(out, pos, src + bd.srcOff, bd.size, (b + 1 == cd.nBlocks) ? 1u : 0u, zs_block_meta(metas, lb),
                             zs_block_lit_section(litSecAll, lb), zs_block_seq_section(seqSecAll, lb), tid, blockDim.x);
    }
    if (tid == 0) dstSizes[chunkBase + blockIdx.x] = pos;
}

// ---------------------------------------------------------------------------------------------
// k_frame_checksum : the Content_Checksum of a call's frames (checksumFlag), a post-pass over frames that are already final: the low 32 bits
// of XXH64 (seed 0) of the chunk's content go behind the last block, bit 2 of the Frame_Header_Descriptor is set and the size grows by 4 -
// no other byte of the frame changes, so a checksummed frame is the plain frame plus these two edits whatever kernel assembled it.
// One quad a chunk (16 a wavefront, as k_seek_hash); a chunk whose size is an error code is left as it is.  A chunk's hash is one serial
// chain: the launch takes as long as the call's largest chunk, whatever the batch.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64) k_frame_checksum(const uint8_t *__restrict__ src, const ZsChunkDesc *__restrict__ chunks, uint32_t n,
                                                       uint8_t *__restrict__ dst, uint32_t *__restrict__ dstSizes)
{
    const uint32_t q = blockIdx.x * 16 + (threadIdx.x >> 2);
    const bool real = q < n;
    ZsChunkDesc cd = {};
    if (real) cd = chunks[q];
    const uint32_t written = real ? dstSizes[q] : 0xFFFFFFFFu;
    // a frame to close: not an error code, and - always, the bound holds the 4 bytes - one that leaves them room in its slot
    const bool work = !zs_word_is_error(written) && (uint64_t)written + 4 <= zs_compress_bound(cd.size);
    const uint64_t h = xxh64_quad<16>(src + cd.srcOff, work ? cd.size : 0u);           // (every lane of a quad calls; a quad without work hashes nothing)
    if (!work || (threadIdx.x & 3u) != 0) return;
    uint8_t *out = dst + cd.dstOff, *t = out + written;
    t[0] = (uint8_t)h; t[1] = (uint8_t)(h >> 8); t[2] = (uint8_t)(h >> 16); t[3] = (uint8_t)(h >> 24);
    out[4] |= 0x04;
    dstSizes[q] = written + 4;
}

static const uint32_t kTrainStatWords = 448;                                // literal bytes [0, 256), LL codes [256, 320), OF [320, 384), ML [384, 448)
// finalize statistics of one compressed sub-batch, between k_encode_sequences and k_encode_literals: the codes the sequences kernel left in the
// block's literal buffer (LL, OF with the recent-offset codes applied, ML; ZS_CHAIN_CODES apart), and the literal bytes - every block byte no match
// of the block's records covers.  One workgroup a block, counts added to stats[kTrainStatWords].
__global__ void __launch_bounds__(256) k_train_stats(const uint8_t *__restrict__ src, const ZsBlockDesc *__restrict__ blocks, const ZsSeqRec *__restrict__ seqAll,
                                                     const uint32_t *__restrict__ hdrAll, const uint8_t *__restrict__ litsAll, uint32_t *__restrict__ stats)
{
    __shared__ uint32_t cov[ZS_BLOCK_MAX / 32], hist[kTrainStatWords];
    const uint32_t blk = blockIdx.x, tid = threadIdx.x;
    const ZsBlockDesc bd = blocks[blk];
    const uint32_t n = bd.size;
    for (uint32_t i = tid; i < ZS_BLOCK_MAX / 32; i += 256) cov[i] = 0;
    for (uint32_t i = tid; i < kTrainStatWords; i += 256) hist[i] = 0;
    __syncthreads();
    const uint32_t nseq = n >= 16 ? zs_block_hdr(hdrAll, blk).nseq : 0u;
    const ZsSeqRec *seqBase = zs_block_seqs(seqAll, blk);
    const uint8_t *codes = zs_lits_lend_chain_codes_to_stats(litsAll, blk);
    for (uint32_t g = tid; g < nseq; g += 256) {
        const ZsSeqRec rec = seqBase[g];
        const uint32_t pos = zs_rec_pos(rec.y), end = min(pos + zs_rec_ml(rec.x), n);
        for (uint32_t b = pos; b < end;) {                                  // the match's bytes in the coverage bitmap
            const uint32_t w = b >> 5, lo = b & 31u, cnt = min(32u - lo, end - b);
            atomicOr(&cov[w], (cnt == 32u ? 0xFFFFFFFFu : ((1u << cnt) - 1u)) << lo);
            b += cnt;
        }
        atomicAdd(&hist[256 + codes[g]], 1u);
        atomicAdd(&hist[320 + codes[ZS_CHAIN_CODES + g]], 1u);
        atomicAdd(&hist[384 + codes[2u * ZS_CHAIN_CODES + g]], 1u);
    }
    __syncthreads();
    const uint8_t *s = src + bd.srcOff;
    for (uint32_t b = tid; b < n; b += 256) if (!((cov[b >> 5] >> (b & 31u)) & 1u)) atomicAdd(&hist[s[b]], 1u);
    __syncthreads();
    for (uint32_t i = tid; i < kTrainStatWords; i += 256) if (hist[i]) atomicAdd(&stats[i], hist[i]);
}

// A digested dictionary's entropy tables in encoder form, once per dictionary, by the encoder's own routines: the Huffman codes in the decoder's
// order from the weights (huffCodesAndWeights), the three encoding tables (buildCTableWave: a trained dictionary's counts hold -1 entries),
// and the cost of every symbol.  One workgroup of 256 threads; wavefront t < 3 makes table t.
__global__ void __launch_bounds__(256) k_cdict_tables(const ZsCDictEntropy *__restrict__ ent, ZsCDictTables *__restrict__ out)
{
    const ZsCDictEntropy &e = *ent;                  // (in the dictionary loader's record, device memory)
    __shared__ K3Lds L;
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    const bool huf = e.hufLog != 0 && e.hufLog <= ZS_HUF_MAXBITS;
    const uint32_t w = (huf && tid < e.nWeights) ? e.weights[tid] : 0u;
    L.nbBits[tid] = (uint8_t)(w ? e.hufLog + 1 - w : 0u);
    __syncthreads();
    if (huf) huffCodesAndWeights(L, 255, e.hufLog);
    out->hufCodeNb[tid] = w ? L.codeNb[tid] : 0u;
    if (tid == 0) out->hufLog = huf ? e.hufLog : 0u;
    if (wave < 3) {
        const uint32_t t = (uint32_t)__builtin_amdgcn_readfirstlane((int)wave);      // (in a scalar register: so are the table's log and size)
        const uint32_t maxSym = e.maxSym[t], tableLog = e.tableLog[t];
        FseCT &ct = L.u.cd[wave].ct;
        buildCTableWave(L.u.cd[wave].build, ct, e.norm[t], maxSym, tableLog);
        const int nv = lane <= maxSym ? e.norm[t][lane] : 0;
        const uint32_t *from = reinterpret_cast<const uint32_t *>(&ct); uint32_t *to = reinterpret_cast<uint32_t *>(&out->ct[t]);
        for (uint32_t i = lane; i < sizeof(FseCT) / 4; i += 64) to[i] = from[i];
        out->cost[t][lane] = (uint16_t)(nv == 0 ? ZS_COST_NONE : fseSymbolCost((uint32_t)(nv < 0 ? 1 : nv), tableLog));
    }
}

// ---------------------------------------------------------------------------------------------
// pack frames: compressed frames in bound-sized slots -> back to back
// ---------------------------------------------------------------------------------------------
// The bytes item i gets: its size, or 0 for an error word (zsmi_status.h) or an item whose status (may be null) is not 0.
// Size: uint32_t, the sizes a compress call leaves (zsmi_packFramesDevice: align 1, no status, no caps); uint64_t, the sizes k_frame_sizes
// leaves (zsmi_layoutOutputsDevice), which also wants the items' bytes themselves: caps (may be null).
template <class Size>
__device__ __forceinline__ uint32_t zs_layout_cap(const Size *sizes, const uint32_t *status, uint32_t i)
{
    const Size v = sizes[i];
    return (v > (Size)zs_word_max_size() || (status && status[i])) ? 0u : (uint32_t)v;
}
// The exclusive scan of n such sizes, each rounded up to `align` (a power of two); offsets[n]: the total.  Three launches (scanOffsets in
// zsmi_api.hip): k_pack_tile_sums, a workgroup a tile of ZS_SCAN_TILE items - its sum; k_pack_scan_tiles, ONE workgroup - the exclusive
// scan of the tile sums, in place, and the total; k_pack_offsets, a workgroup a tile again - the scan inside the tile from the tile's base.
// (One workgroup over all n items, the first form, took 2.56 ms for 1 048 576 sizes: 1.7 % of the decode call they lay out.)
#define ZS_SCAN_TILE 2048u            // 256 threads x 8 items
// a workgroup of 256 threads: the sum of v over the threads in front of this one; total: over all.  part: 256 words of LDS
__device__ __forceinline__ uint64_t zs_block_excl_scan256(uint64_t v, uint64_t *part, uint64_t &total)
{
    const uint32_t t = threadIdx.x;
    part[t] = v;
    __syncthreads();
    for (uint32_t d = 1; d < 256u; d <<= 1) {
        const uint64_t add = t >= d ? part[t - d] : 0;
        __syncthreads();
        part[t] += add;
        __syncthreads();
    }
    total = part[255];
    return part[t] - v;
}
// the eight items of a thread: their bytes (0 behind n) and the sum of their rounded sizes
template <class Size>
__device__ __forceinline__ uint64_t zs_layout_thread_items(const Size *sizes, const uint32_t *status, uint32_t n, uint64_t up, uint64_t first, uint32_t cap[8])
{
    uint64_t s = 0;
    for (uint32_t k = 0; k < 8; k++) {
        cap[k] = first + k < n ? zs_layout_cap(sizes, status, (uint32_t)(first + k)) : 0u;
        if (first + k < n) s += ((uint64_t)cap[k] + up) & ~up;
    }
    return s;
}
template <class Size>
__global__ void __launch_bounds__(256)
k_pack_tile_sums(const Size *sizes, const uint32_t *status, uint32_t n, uint32_t align, uint64_t *tileSums)
{
    __shared__ uint64_t part[256];
    uint32_t cap[8]; uint64_t total;
    const uint64_t s = zs_layout_thread_items(sizes, status, n, (uint64_t)align - 1u, (uint64_t)blockIdx.x * ZS_SCAN_TILE + threadIdx.x * 8u, cap);
    (void)zs_block_excl_scan256(s, part, total);
    if (threadIdx.x == 0) tileSums[blockIdx.x] = total;
}
__global__ void k_pack_scan_tiles(uint64_t *tileSums, uint32_t tiles, uint64_t *totalOut)
{
    // single workgroup exclusive scan over the tile sums, in place
    __shared__ uint64_t part[1024];
    const uint32_t tid = threadIdx.x, per = (tiles + blockDim.x - 1) / blockDim.x;
    const uint32_t lo = min(tiles, tid * per), hi = min(tiles, lo + per);
    uint64_t s = 0;
    for (uint32_t i = lo; i < hi; i++) s += tileSums[i];
    part[tid] = s;
    __syncthreads();
    if (tid == 0) { uint64_t run = 0; for (uint32_t t = 0; t < blockDim.x; t++) { const uint64_t v = part[t]; part[t] = run; run += v; } *totalOut = run; }
    __syncthreads();
    uint64_t run = part[tid];
    for (uint32_t i = lo; i < hi; i++) { const uint64_t v = tileSums[i]; tileSums[i] = run; run += v; }
}
template <class Size>
__global__ void __launch_bounds__(256)
k_pack_offsets(const Size *sizes, const uint32_t *status, uint32_t n, uint32_t align, const uint64_t *tileBases, uint32_t *caps, uint64_t *offsets)
{
    __shared__ uint64_t part[256];
    uint32_t cap[8]; uint64_t total;
    const uint64_t up = (uint64_t)align - 1u, first = (uint64_t)blockIdx.x * ZS_SCAN_TILE + threadIdx.x * 8u;
    const uint64_t s = zs_layout_thread_items(sizes, status, n, up, first, cap);
    uint64_t run = tileBases[blockIdx.x] + zs_block_excl_scan256(s, part, total);
    for (uint32_t k = 0; k < 8 && first + k < n; k++) { offsets[first + k] = run; if (caps) caps[first + k] = cap[k]; run += ((uint64_t)cap[k] + up) & ~up; }
}
__global__ void k_pack_copy(const uint8_t *frames, const uint64_t *srcOffsets, const uint32_t *sizes, const uint64_t *packedOffsets, uint8_t *packed)
{
    const uint32_t i = blockIdx.x;
    const uint32_t sz = zs_word_bytes(sizes[i]);
    const uint8_t *s = frames + srcOffsets[i]; uint8_t *d = packed + packedOffsets[i];
    zs_block_copy(d, s, sz, threadIdx.x, blockDim.x);
}

#endif
