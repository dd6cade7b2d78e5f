// The FSE side of the format that the encoder, the dictionary code and the decoder share: the constants of the three sequence-code
// alphabets, and THE table builder - "normalised counts -> spread the symbols over the cells -> number each symbol's cells in ascending
// cell order" (BuildFSETable, ZStdDecompress.cs:958-1034; FSE_buildCTable is its inverse view) - as two wavefront routines which the
// encoding table (buildCTableWave, entropy_kernels.hip) and the decoding table (buildSeqTableWave, decode_kernels.hip) are made of.
// Both are force-inlined and take their per-cell actions as always_inline lambdas: nothing that touches LDS may sit behind a real call
// (the LDS pointers would become generic pointers and the accesses flat_* instructions; see decode_kernels.hip).
#pragma once
#include "zsmi_device.h"
#include "zsmi_wave.h"

// ---- alphabets (ZStdInternal.cs:140-198): largest code, largest table log, the predefined distribution with its largest code and log ----
#define MaxLL 35
#define MaxML 52
#define MaxOff 31
#define LLFSELog 9
#define MLFSELog 9
#define OffFSELog 8
#define LL_defaultNormLog 6
#define ML_defaultNormLog 6
#define OF_defaultNormLog 5
#define DefaultMaxOff 28
__constant__ int16_t LL_defaultNorm[MaxLL + 1] = { 4,3,2,2,2,2,2,2, 2,2,2,2,2,1,1,1, 2,2,2,2,2,2,2,2, 2,3,2,1,1,1,1,1, -1,-1,-1,-1 };
__constant__ int16_t ML_defaultNorm[MaxML + 1] = { 1,4,3,2,2,2,2,2, 2,1,1,1,1,1,1,1, 1,1,1,1,1,1,1,1, 1,1,1,1,1,1,1,1,
                                                   1,1,1,1,1,1,1,1, 1,1,1,1,1,1,-1,-1, -1,-1,-1,-1,-1 };
__constant__ int16_t OF_defaultNorm[DefaultMaxOff + 1] = { 1,1,1,1,1,1,2,2, 2,1,1,1,1,1,1,1, 1,1,1,1,1,1,1,1, -1,-1,-1,-1,-1 };
// base value and extra bits of a literal-length / match-length code (the decoder's tables; the encoder derives codes and extra bits by
// arithmetic: llCodeOf and its kin in entropy_kernels.hip)
__constant__ uint8_t LL_bits[MaxLL + 1] = { 0,0,0,0,0,0,0,0, 0,0,0,0,0,0,0,0, 1,1,1,1,2,2,3,3, 4,6,7,8,9,10,11,12, 13,14,15,16 };
__constant__ uint8_t ML_bits[MaxML + 1] = { 0,0,0,0,0,0,0,0, 0,0,0,0,0,0,0,0, 0,0,0,0,0,0,0,0, 0,0,0,0,0,0,0,0,
                                            1,1,1,1,2,2,3,3, 4,4,5,7,8,9,10,11, 12,13,14,15,16 };
__constant__ uint32_t LL_base[MaxLL + 1] = { 0,1,2,3,4,5,6,7, 8,9,10,11,12,13,14,15, 16,18,20,22,24,28,32,40,
                                             48,64,0x80,0x100,0x200,0x400,0x800,0x1000, 0x2000,0x4000,0x8000,0x10000 };
__constant__ uint32_t ML_base[MaxML + 1] = { 3,4,5,6,7,8,9,10, 11,12,13,14,15,16,17,18, 19,20,21,22,23,24,25,26,
                                             27,28,29,30,31,32,33,34, 35,37,39,41,43,47,51,59, 67,83,99,0x83,0x103,0x203,0x403,0x803,
                                             0x1003,0x2003,0x4003,0x8003,0x10003 };

// ---- the build scratch of one table (LDS, one wavefront) ----
struct FseBuild {
    uint8_t  tableSymbol[512];       // the symbol of every cell
    uint32_t cumul[64];              // spread: index of a symbol's first entry in the expanded symbol list
    uint32_t symCount[64];           // rank: the number the symbol's next cell gets
    uint32_t symMask[128];           // rank: a 64-bit lane mask per symbol
};

// ---- spread, by all 64 lanes.  Lane s holds n = norm[s]: a count, -1 (low probability) or 0 (always 0 above maxSym).
// The reference walks the cells in the order p_k = (k * step) & mask, skipping the low-probability area at the top, and hands them to the
// symbols in turn; step is odd, so p_k is a permutation: the k-th visit is valid iff p_k <= highThreshold and takes the j-th entry of the
// expanded symbol list, j = valid visits before k (with no -1 present every visit is valid: cell (j * step) & mask).  The low-probability
// symbols, ascending, take the cells from the top downwards (:975-978).  put(cell, symbol) is called once for every cell.
// start: 64 entries of LDS scratch. ----
template <class T, class Put>
__device__ __forceinline__ void fseSpreadWave(T *start, int n, uint32_t maxSym, uint32_t tableLog, Put put)
{
    const uint32_t lane = (uint32_t)zs_lane();
    const uint32_t tableSize = 1u << tableLog, tableMask = tableSize - 1, step = (tableSize >> 1) + (tableSize >> 3) + 3;
    const uint64_t below = (1ull << lane) - 1ull;
    const bool low = n == -1;
    const uint64_t lowMask = __ballot(low);
    const uint32_t highThreshold = tableSize - 1 - (uint32_t)__popcll(lowMask);
    if (low) put(tableSize - 1 - (uint32_t)__popcll(lowMask & below), lane);
    const uint32_t cnt = n > 0 ? (uint32_t)n : 0u;
    const uint32_t incl = wave_incl_scan(cnt);
    start[lane] = (T)(incl - cnt);
    wave_sync();
    uint32_t validBefore = 0;
    for (uint32_t base = 0; base < tableSize; base += 64) {
        const uint32_t k = base + lane, p = (k * step) & tableMask;
        const bool valid = k < tableSize && p <= highThreshold;
        const uint64_t vm = __ballot(valid);
        if (valid) {
            const uint32_t j = validBefore + (uint32_t)__popcll(vm & below);
            uint32_t lo = 0, hi = maxSym + 1;                                        // last symbol whose first entry index is <= j
            while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (start[mid] <= j) lo = mid; else hi = mid; }
            put(p, lo);
        }
        validBefore += (uint32_t)__popcll(vm);
    }
    wave_sync();
}

// ---- rank, by all 64 lanes: emit(cell, symbol, next) for every cell in ascending cell order per symbol, next = next[symbol] + (rank of
// the cell among the cells of its symbol); next[] is advanced as the cells are numbered.  The encoder seeds next[] with the cumulative
// counts and stores stateTable[next]; the decoder seeds it with the counts and derives nextState / nbBits from next (:1017-1027).
// 64 cells at a time: every lane ors its bit into its symbol's 64-bit lane mask (LDS); the mask read back gives the lane its rank among
// the chunk's cells of that symbol (bits below it) and the symbol's count in the chunk, which the symbol's first lane adds to next[].
// (A loop over the chunk's distinct symbols, a ballot each, was ~25 rounds of three LDS round trips per chunk.) ----
template <class T, class SymOf, class Emit>
__device__ __forceinline__ void fseRankWave(uint32_t *symMask, T *next, uint32_t tableSize, SymOf symOf, Emit emit)
{
    const uint32_t lane = (uint32_t)zs_lane();
    const uint64_t below = (1ull << lane) - 1ull;
    for (uint32_t base = 0; base < tableSize; base += 64) {
        const uint32_t u = base + lane;
        const bool in = u < tableSize;
        const uint32_t sym = in ? symOf(u) : 0u;
        symMask[2 * lane] = 0; symMask[2 * lane + 1] = 0;
        wave_sync();
        if (in) atomicOr(&symMask[2 * sym + (lane >> 5)], 1u << (lane & 31u));
        wave_sync();
        uint32_t first = 0, rank = 1, cnt = 0;
        if (in) {
            const uint32_t lo = symMask[2 * sym], hi = symMask[2 * sym + 1];
            rank = (uint32_t)__popc(lo & (uint32_t)below) + (uint32_t)__popc(hi & (uint32_t)(below >> 32));
            cnt = (uint32_t)__popc(lo) + (uint32_t)__popc(hi);
            first = next[sym];
            emit(u, sym, first + rank);
        }
        wave_sync();
        if (in && rank == 0) next[sym] = (T)(first + cnt);
        wave_sync();
    }
    wave_sync();
}
