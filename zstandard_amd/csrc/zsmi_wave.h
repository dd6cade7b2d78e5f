// Device primitives that more than one kernel file uses: wavefront cross-lane operations and ordering points, the workgroup copy,
// little-endian reads, XXH64 by a quad of lanes.  What only one file uses stays in that file.
#pragma once
#include "zsmi_device.h"

// ---------------------------------------------------------------------------------------------
// wave helpers
// ---------------------------------------------------------------------------------------------
// Cross-lane moves by data-parallel primitives (DPP): vector-ALU operand modifiers, no LDS round trip (a __shfl is a
// ds_bpermute: ~100 cycles of latency each, six in a row for a scan).  Control codes (gfx9): row_shr:n = 0x110 + n
// (zero fill with bound_ctrl), row_bcast15 = 0x142 (lane 15 of a row to the next row), row_bcast31 = 0x143.
#define ZS_DPP(old, v, ctrl, rowMask, boundCtrl) ((uint32_t)__builtin_amdgcn_update_dpp((int)(old), (int)(v), (ctrl), (rowMask), 0xF, (boundCtrl)))
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v)
{
    v += ZS_DPP(0, v, 0x111, 0xF, true);
    v += ZS_DPP(0, v, 0x112, 0xF, true);
    v += ZS_DPP(0, v, 0x114, 0xF, true);
    v += ZS_DPP(0, v, 0x118, 0xF, true);            // inclusive within each row of 16
    v += ZS_DPP(0, v, 0x142, 0xA, false);           // rows 1, 3 += total of the row before
    v += ZS_DPP(0, v, 0x143, 0xC, false);           // rows 2, 3 += total of rows 0..1
    return v;
}
// value of lane l, l the same for the whole wavefront
__device__ __forceinline__ uint32_t wave_get(uint32_t v, int l) { return (uint32_t)__builtin_amdgcn_readlane((int)v, __builtin_amdgcn_readfirstlane(l)); }
__device__ __forceinline__ uint32_t wave_last(uint32_t v) { return (uint32_t)__builtin_amdgcn_readlane((int)v, 63); }
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) { return wave_last(wave_incl_scan(v)); }
__device__ __forceinline__ uint32_t wave_max(uint32_t v)
{
    v = max(v, ZS_DPP(0, v, 0x111, 0xF, true));
    v = max(v, ZS_DPP(0, v, 0x112, 0xF, true));
    v = max(v, ZS_DPP(0, v, 0x114, 0xF, true));
    v = max(v, ZS_DPP(0, v, 0x118, 0xF, true));
    v = max(v, ZS_DPP(0, v, 0x142, 0xA, false));
    v = max(v, ZS_DPP(0, v, 0x143, 0xC, false));
    return wave_last(v);
}
__device__ __forceinline__ uint32_t wave_min(uint32_t v) { return ~wave_max(~v); }     // (the zero fill of the row shifts is max's identity, not min's)

// ordering point between LDS accesses of different lanes of ONE wavefront: LDS instructions of a wave execute in issue
// order, so only the compiler has to be kept from moving them across
__device__ __forceinline__ void wave_sync() { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier(); }
// Bytes handed from lane to lane through GLOBAL memory additionally need the stores to have completed before the loads are
// issued (loads and stores of a wavefront may complete out of order with respect to each other): wave_mem_sync() waits for
// the outstanding vector-memory operations of the wavefront.
__device__ __forceinline__ void wave_mem_sync() { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup"); __builtin_amdgcn_wave_barrier(); }

// a workgroup copies n bytes: 16-byte pieces (two unaligned 8-byte accesses), four pieces a thread in flight, then the tail.
// (A byte a thread and iteration was 100 dependent load -> store rounds per section.)
__device__ __forceinline__ void zs_block_copy(uint8_t *__restrict__ d, const uint8_t *__restrict__ s, uint32_t n, uint32_t tid, uint32_t nthreads)
{
    const uint32_t n16 = n >> 4;
    for (uint32_t i = tid; i < n16; i += 4 * nthreads) {
        uint64_t a[4], b[4];
        #pragma unroll
        for (uint32_t k = 0; k < 4; k++) { const uint32_t idx = min(i + k * nthreads, n16 - 1); a[k] = zs_load64(s + 16 * idx); b[k] = zs_load64(s + 16 * idx + 8); }
        #pragma unroll
        for (uint32_t k = 0; k < 4; k++) { const uint32_t idx = i + k * nthreads; if (idx < n16) { zs_store64(d + 16 * idx, a[k]); zs_store64(d + 16 * idx + 8, b[k]); } }
    }
    for (uint32_t j = (n16 << 4) + tid; j < n; j += nthreads) d[j] = s[j];
}

__host__ __device__ __forceinline__ uint32_t rd16(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
__host__ __device__ __forceinline__ uint32_t rd24(const uint8_t *p) { return rd16(p) | ((uint32_t)p[2] << 16); }
__host__ __device__ __forceinline__ uint32_t rd32(const uint8_t *p) { return zs_load32(p); }

__device__ static uint64_t rotl64(uint64_t x, int r) { return (x << r) | (x >> (64 - r)); }

// XXH64 seed 0 (XxHash.cs:896-1161) by FOUR lanes (a quad of the wavefront, r = lane & 3): the stripe loop is four independent accumulators, lane r runs the r-th (the 8 bytes at 8 r of
// every 32-byte stripe), the quad's first lane merges them and finishes the tail.  Every lane of the quad must call; the result is valid in its first lane.
// (k_dec_checksum hashed an item's whole output on one lane: 1 MiB frames are 32768 dependent rounds there.)
// AHEAD > 1: the stripe loop loads AHEAD stripes before it folds them in (AHEAD loads a lane in flight instead of one dependent load a stripe:
// k_seek_hash, whose quads are few and long).  AHEAD = 1 is the plain loop the decode kernels use.
template <int AHEAD = 1>
__device__ __forceinline__ uint64_t xxh64_quad(const uint8_t *p, uint64_t len)
{
    const uint64_t P1 = 11400714785074694791ULL, P2 = 14029467366897019727ULL, P3 = 1609587929392839161ULL, P4 = 9650029242287828579ULL, P5 = 2870177450012600261ULL;
    const uint32_t r = (uint32_t)zs_lane() & 3u;
    const uint8_t *const bEnd = p + len; uint64_t h64 = P5;
    #define XXR(acc, in) { acc += (in) * P2; acc = rotl64(acc, 31); acc *= P1; }
    const uint64_t stripes = len >> 5;
    if (stripes) {
        uint64_t v = r == 0 ? P1 + P2 : (r == 1 ? P2 : (r == 2 ? 0ull : 0ull - P1));
        const uint8_t *q = p + 8u * r;
        uint64_t i = 0;
        if constexpr (AHEAD > 1) {
            for (; i + AHEAD <= stripes; i += AHEAD) {
                uint64_t in[AHEAD];
                #pragma unroll
                for (int k = 0; k < AHEAD; k++) in[k] = zs_load64(q + 32 * k);
                #pragma unroll
                for (int k = 0; k < AHEAD; k++) XXR(v, in[k]);
                q += 32 * AHEAD;
            }
        }
        for (; i < stripes; i++) { XXR(v, zs_load64(q)); q += 32; }
        const int base = zs_lane() & ~3;
        uint64_t vv[4];
        #pragma unroll
        for (int k = 0; k < 4; k++) vv[k] = ((uint64_t)(uint32_t)__shfl((int)(uint32_t)(v >> 32), base + k) << 32) | (uint32_t)__shfl((int)(uint32_t)v, base + k);
        h64 = rotl64(vv[0], 1) + rotl64(vv[1], 7) + rotl64(vv[2], 12) + rotl64(vv[3], 18);
        #pragma unroll
        for (int k = 0; k < 4; k++) { uint64_t t_ = 0; XXR(t_, vv[k]); h64 ^= t_; h64 = h64 * P1 + P4; }
        p += stripes << 5;
    }
    h64 += len;
    while (p + 8 <= bEnd) { uint64_t k1 = 0; XXR(k1, zs_load64(p)); h64 ^= k1; h64 = rotl64(h64, 27) * P1 + P4; p += 8; }
    if (p + 4 <= bEnd) { h64 ^= (uint64_t)zs_load32(p) * P1; h64 = rotl64(h64, 23) * P2 + P3; p += 4; }
    while (p < bEnd) { h64 ^= (*p) * P5; h64 = rotl64(h64, 11) * P1; p++; }
    #undef XXR
    h64 ^= h64 >> 33; h64 *= P2; h64 ^= h64 >> 29; h64 *= P3; h64 ^= h64 >> 32;
    return h64;
}
