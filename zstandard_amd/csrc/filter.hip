// filter.hip -- frame filters (zsmi_filter.h states the rule, the filter frame and its check; zsmi_buildFrameFilter, zsmi_readFrameFilter
// and zsmi_filterFrames run them serially on the host): a Bloom filter a frame of a record archive, built from text at one pass, judged,
// and asked which frames of a window can hold a query's records - before any of them is decoded.  The device calls only queue work.
//
// Build (zsmi_buildFrameFilterDevice) over text[0, size) and places[0 .. n] - the frames' borders in the text, ascending, 0 first, size
// last - a workgroup a 16 KiB tile (the splitter's shape: 256 threads x 16 bytes x 4 steps):
//   (fill)           the slots zeroed on the stream: an empty frame's slot is done
//   k_filter_tiles   the tile and a halo of g - 1 bytes behind it staged in LDS; two binary searches over places find the frames that
//                    overlap the tile (k_recidx_tiles' searches).  A frame segment at a time, the whole workgroup: the borders' cleanliness
//                    from the text (rule 5: one byte in front of each border) - a SATURATED frame is stored as all ones by the tile its
//                    first byte lies in and hashed by none; of a clean frame each lane takes aligned groups of four positions (two LDS
//                    words, four grams by shifts), drops the grams that hold the delimiter or leave the frame (a gram may END in the
//                    halo, it must START in the tile), folds four bytes at once and sets two bits a gram in an LDS bitset of 2^L bits
//                    (ds_or); then the bitset's non-zero words go to the frame's slot by vector atomicOr and are cleared on the way.  OR
//                    commutes, so the slot does not depend on the order the tiles of a long frame arrive in.  A frame over many tiles is
//                    many workgroups' segments; a tile of hundreds of tiny frames is one workgroup's loop.
//   k_filter_check   one pass over the slots' 64-bit words: the check's terms and the all-ones slots, added up by wavefront into two words
//   k_filter_built   one lane: the header, its check, dResult
// On an archive (zsmi_seekableBuildFrameFilterResident) the frames are decoded end to end into dWork by find.hip's findDecode as it
// stands - the whole archive one window - and its layout scan is the body's places.  The host form walks seekable.hip's window plan
// (windows of at most 256 MiB of content; frames never cross a window); what the next window's first border needs is ONE byte, the
// text's last, copied to a scratch word on the stream before dWork is written again.
// Check (zsmi_checkFrameFilterDevice): the header judged on the device against filterSize, k_filter_check over the slots it names,
// k_filter_judged - zsmi_readFrameFilter's verdict.
// Filter (zsmi_filterFramesDevice): the patterns travel by value, folded as the query calls fold them (ZsFindQuery, findquery.hip); g, L
// and the delimiter lie in the filter's header in DEVICE memory, which the host never reads, so each workgroup of k_filter_test judges the
// header, holds the patterns against the delimiter and hashes their grams once into LDS (at most 256 values); then a lane a frame tests
// them.  scanOffsets over the verdicts, k_filter_list writes the passing frames, ascending, and dResult.
// Scratch, all of it context buffers reserved before anything is queued: four words of sums and a carry word; 12 bytes a frame of the
// window for the filter call; findDecode's for the archive call.  Every store is a vector store from plain C++.

#include "zsmi_status.h"
#include "zsmi_wave.h"            // wave_sum
#include "zsmi_ctx.h"             // the context, LAUNCH, scanOffsets
#include "zsmi_filter.h"          // the rule, the frame, the host forms
#include <algorithm>
// From the feature files zsmi_api.hip includes in front of this one: split.hip - ZS_SPLIT_TILE, ZsSplitBytes16; seekable.hip - the handle,
// seekWindowCheck, the window plan (SeekWindows, seekCutWindows, seekWindowLimit); find.hip - the decode half of a window
// (findDecodeReserve, findDecode, FindDecoded); findquery.hip - ZsFindQuery, findQuery; recindex.hip - zs_ridx_lower, zs_ridx_block_sum,
// zs_ridx_wave_sum64.

struct ZsFltSums { unsigned long long check, saturated, grams, status; };  // zeroed on the stream in front of the kernels; status: the first window's that failed
struct ZsFltShared { uint32_t text[ZS_SPLIT_TILE / 4u + 2u]; uint32_t bits[1u << (ZS_FLT_MAX_LOG - 5u)]; uint32_t slots[4]; };

// ---- kernels: build ----
// rule 5 for a border x of text[0, size): prev - null: the text starts the content; else the content's byte in front of the text.  atEnd:
// `size` is the content's end.  (x > size - places that do not ascend: not clean, and nothing is read)
__device__ __forceinline__ bool zs_flt_border_clean(const uint8_t *__restrict__ src, uint64_t size, uint64_t x, uint32_t delim, const uint8_t *__restrict__ prev, uint32_t atEnd)
{
    if (x == 0) return prev ? *prev == delim : true;
    if (x == size && atEnd) return true;
    return x <= size && src[x - 1u] == delim;
}
// the first j of v[0, count) with v[j] > x (count: none)
__device__ __forceinline__ uint32_t zs_flt_upper(const uint64_t *__restrict__ v, uint32_t count, uint64_t x)
{
    uint32_t lo = 0, hi = count;
    while (lo < hi) { const uint32_t mid = lo + (hi - lo) / 2u; if (v[mid] <= x) lo = mid + 1u; else hi = mid; }
    return lo;
}
// slots: the first frame's slot (4-byte words), zeroed on the stream in front of the kernel.  code: null, or the window's code (find.hip)
__global__ void __launch_bounds__(256)
k_filter_tiles(const uint8_t *__restrict__ src, uint64_t size, uint32_t delim, uint32_t g, uint32_t L, const uint64_t *__restrict__ places, uint32_t n,
               const uint8_t *__restrict__ prev, uint32_t atEnd, const uint32_t *__restrict__ code, uint32_t *slots, ZsFltSums *sums)
{
    __shared__ ZsFltShared sh;
    const uint32_t tid = threadIdx.x;
    const uint64_t tileAt = (uint64_t)blockIdx.x * ZS_SPLIT_TILE, base = tileAt + 16u * tid;
    if (blockIdx.x == 0 && tid == 0) {
        uint32_t s = code ? *code : 0u;
        if (!s && (places[0] != 0 || places[n] != size)) s = ZSMI_error_parameter_outOfBound;
        if (s && !sums->status) sums->status = s;                          // (the windows of one call follow one another on the stream)
    }
    // the tile: whole tiles by four 16-byte loads a lane, the text's last tile byte by byte - no byte at or behind src + size is read
    if (size >= tileAt + ZS_SPLIT_TILE) {
        ZsSplitBytes16 own[4];
        #pragma unroll
        for (uint32_t s = 0; s < 4; s++) __builtin_memcpy(&own[s], src + base + s * 4096u, 16);
        #pragma unroll
        for (uint32_t s = 0; s < 4; s++)
            #pragma unroll
            for (uint32_t w = 0; w < 4; w++) sh.text[s * 1024u + 4u * tid + w] = own[s].w[w];
    } else {
        for (uint32_t s = 0; s < 4; s++)
            for (uint32_t w = 0; w < 4; w++) {
                const uint64_t b = base + s * 4096u + 4u * w;
                uint32_t v = 0;
                for (uint32_t j = 0; j < 4; j++) if (b + j < size) v |= (uint32_t)src[b + j] << (8u * j);
                sh.text[s * 1024u + 4u * tid + w] = v;
            }
    }
    if (tid == 0) {                                                        // the halo: the g - 1 <= 3 bytes behind the tile, zeros behind the text
        uint32_t v = 0;
        for (uint32_t j = 0; j < 3; j++) if (tileAt + ZS_SPLIT_TILE + j < size) v |= (uint32_t)src[tileAt + ZS_SPLIT_TILE + j] << (8u * j);
        sh.text[ZS_SPLIT_TILE / 4u] = v; sh.text[ZS_SPLIT_TILE / 4u + 1u] = 0;
    }
    const uint32_t words = 1u << (L - 5u);
    for (uint32_t w = tid; w < words; w += 256u) sh.bits[w] = 0;
    __syncthreads();
    const uint64_t tileEnd = size < tileAt + ZS_SPLIT_TILE ? size : tileAt + ZS_SPLIT_TILE;
    uint32_t hashed = 0;
    if (tileEnd > tileAt) {
        // the frames that overlap the tile: the first that ends behind its start .. the first that starts at or behind its end
        const uint32_t lo = zs_flt_upper(places + 1, n, tileAt), hi = zs_ridx_lower(places, n, tileEnd);
        const uint32_t delim4 = delim * 0x01010101u, beyond = g == 4u ? 0u : 0xFF000000u;
        for (uint32_t j = lo; j < hi; j++) {                               // (the same for the whole workgroup)
            const uint64_t fa = places[j], fb = places[j + 1u];
            const uint64_t a = fa > tileAt ? fa : tileAt, b = fb < tileEnd ? fb : tileEnd;
            if (a >= b) continue;                                          // (an empty frame; or places that do not ascend)
            uint32_t *slot = slots + (uint64_t)j * words;
            if (!zs_flt_border_clean(src, size, fa, delim, prev, atEnd) || !zs_flt_border_clean(src, size, fb, delim, prev, atEnd)) {
                if (fa >= tileAt) for (uint32_t w = tid; w < words; w += 256u) slot[w] = ~0u;      // rule 6, by the tile of the frame's first byte
                continue;
            }
            const uint64_t lastStart = fb >= g ? fb - g + 1u : 0u, stop = lastStart < b ? lastStart : b;      // a gram starts in [a, stop)
            if (stop > a) {
                const uint32_t oa = (uint32_t)(a - tileAt), oe = (uint32_t)(stop - tileAt);
                for (uint32_t q = (oa >> 2) + tid; 4u * q < oe; q += 256u) {
                    const uint64_t pair = (uint64_t)sh.text[q] | ((uint64_t)sh.text[q + 1u] << 32);
                    #pragma unroll
                    for (uint32_t k = 0; k < 4; k++) {
                        const uint32_t o = 4u * q + k, x = (uint32_t)(pair >> (8u * k)), y = (x ^ delim4) | beyond;
                        if (o < oa || o >= oe || ((y - 0x01010101u) & ~y & 0x80808080u)) continue;      // outside the segment; a byte of the gram is the delimiter
                        const uint32_t v = zs_flt_value(zs_flt_fold4(x), g), h0 = zs_flt_bit(v, 0, L), h1 = zs_flt_bit(v, 1, L);
                        atomicOr(&sh.bits[h0 >> 5], 1u << (h0 & 31u));
                        atomicOr(&sh.bits[h1 >> 5], 1u << (h1 & 31u));
                        hashed++;
                    }
                }
            }
            __syncthreads();
            for (uint32_t w = tid; w < words; w += 256u) {
                const uint32_t v = sh.bits[w];
                if (v) { atomicOr(slot + w, v); sh.bits[w] = 0; }
            }
            __syncthreads();
        }
    }
    hashed = zs_ridx_block_sum(hashed, sh.slots);
    if (tid == 0 && hashed) atomicAdd(&sums->grams, (unsigned long long)hashed);
}
// The slots' 64-bit words k = 0 .. n * 2^(L-6): the check's terms and the all-ones slots, added to sums.  L == 0: n and L are the
// header's - a header that zs_flt_read_header refuses against filterSize: nothing is read.  A round is max(2^(L-6), 256) words: whole slots
__global__ void __launch_bounds__(256)
k_filter_check(const uint8_t *__restrict__ filter, uint64_t filterSize, uint32_t n, uint32_t L, ZsFltSums *sums)
{
    __shared__ uint32_t bad[32];
    const uint32_t tid = threadIdx.x;
    if (L == 0) {
        ZsFltHeader h;
        if (filterSize < ZS_FLT_FIXED || zs_flt_read_header(filter, filterSize, &h)) return;
        n = h.n; L = h.L;
    }
    const uint64_t *w64 = (const uint64_t *)(filter + ZS_FLT_FIXED);
    const uint32_t W = 1u << (L - 6u), span = W > 256u ? W : 256u, S = span / W;
    const uint64_t words = (uint64_t)n * W, rounds = (words + span - 1u) / span;
    unsigned long long check = 0, saturated = 0;
    for (uint64_t i = blockIdx.x; i < rounds; i += gridDim.x) {
        if (tid < 32u) bad[tid] = 0;
        __syncthreads();
        for (uint32_t r = 0; r < span; r += 256u) {
            const uint64_t k = i * span + r + tid;
            if (k >= words) continue;
            const uint64_t w = w64[k];
            check += zs_flt_term(w, k);
            if (w != ~0ull) bad[(r + tid) / W] = 1u;
        }
        __syncthreads();
        if (tid < S && i * S + tid < n && !bad[tid]) saturated++;
        __syncthreads();
    }
    check = zs_ridx_wave_sum64(check); saturated = zs_ridx_wave_sum64(saturated);
    if ((tid & 63u) == 0) { atomicAdd(&sums->check, check); if (saturated) atomicAdd(&sums->saturated, saturated); }
}
// behind the sums: the header and dResult = {status, the frame's bytes, all-ones slots, grams hashed}
__global__ void k_filter_built(uint8_t *filter, uint32_t n, uint32_t delim, uint32_t g, uint32_t L, uint64_t size, const ZsFltSums *__restrict__ sums, uint64_t *__restrict__ result)
{
    if (blockIdx.x || threadIdx.x) return;
    zs_flt_write_header(filter, n, delim, g, L, size, sums->check + zs_flt_check_base(size, delim, g, L));
    result[0] = sums->status; result[1] = zs_flt_frame_size(n, L); result[2] = sums->saturated; result[3] = sums->grams;
}
// zsmi_readFrameFilter's verdict from the header and the sums: result = {status, N, delim, g, L, size, all-ones slots, 0}
__global__ void k_filter_judged(const uint8_t *__restrict__ filter, uint64_t filterSize, const ZsFltSums *__restrict__ sums, uint64_t *__restrict__ result)
{
    if (blockIdx.x || threadIdx.x) return;
    ZsFltHeader h; h.n = h.delim = h.g = h.L = 0; h.size = 0;
    uint32_t status = filterSize < ZS_FLT_FIXED ? (uint32_t)ZSMI_error_srcSize_wrong : (uint32_t)zs_flt_read_header(filter, filterSize, &h);
    if (!status && sums->check + zs_flt_check_base(h.size, h.delim, h.g, h.L) != zs_flt_rd64(filter + 32)) status = ZSMI_error_corruption_detected;
    result[0] = status;
    result[1] = status ? 0u : h.n; result[2] = status ? 0u : h.delim; result[3] = status ? 0u : h.g; result[4] = status ? 0u : h.L;
    result[5] = status ? 0ull : h.size; result[6] = status ? 0ull : sums->saturated; result[7] = 0;
}

// ---- kernels: filter ----
// pass[i]: frame firstFrame + i passes Q, i < frameCount; sums->status: what zsmi_filterFrames refuses of these bytes and this query
// (then no frame passes), sums->saturated: the all-ones slots among the passing
__global__ void __launch_bounds__(256)
k_filter_test(const uint8_t *__restrict__ filter, uint64_t filterSize, const ZsFindQuery Q, uint32_t firstFrame, uint32_t frameCount, uint32_t *__restrict__ pass, ZsFltSums *sums)
{
    __shared__ uint32_t val[ZS_FIND_MAX_PATTERN], withDelim, slots[4];
    const uint32_t tid = threadIdx.x, i = blockIdx.x * 256u + tid;
    ZsFltHeader h; h.n = h.delim = 0; h.g = 4; h.L = ZS_FLT_MIN_LOG; h.size = 0;
    uint32_t status = filterSize < ZS_FLT_FIXED ? (uint32_t)ZSMI_error_srcSize_wrong : (uint32_t)zs_flt_read_header(filter, filterSize, &h);
    uint32_t total = 0;
    for (uint32_t j = 0; j < Q.K; j++) total += Q.m[j];
    if (tid == 0) withDelim = 0;
    __syncthreads();
    if (!status) {                                                         // the query calls' rule 3; the patterns' grams, a lane a byte of the patterns
        if (tid < total && Q.b[tid] == zs_findq_fold((uint8_t)h.delim, Q.fold ? ZSMI_FIND_IGNORE_CASE : 0u)) withDelim = 1u;
        uint32_t x = 0;
        for (uint32_t k = 0; k < h.g; k++) x |= (tid + k < total ? (uint32_t)Q.b[tid + k] : 0u) << (8u * k);
        val[tid] = zs_flt_value(zs_flt_fold4(x), h.g);
    }
    __syncthreads();
    if (!status && (withDelim || (uint64_t)firstFrame + frameCount > h.n)) status = ZSMI_error_parameter_outOfBound;
    if (blockIdx.x == 0 && tid == 0 && status) sums->status = status;
    bool passes = false, ones = false;
    if (!status && i < frameCount) {
        const uint32_t bytes = zs_flt_slot_bytes(h.L);
        const uint8_t *slot = filter + ZS_FLT_FIXED + (uint64_t)(firstFrame + i) * bytes;
        uint32_t shortOnes = 0;
        bool some = false, every = true;
        for (uint32_t j = 0; j < Q.K; j++) {
            const uint32_t m = Q.m[j], at = Q.at[j];
            if (m < h.g) { shortOnes++; continue; }
            bool p = true;
            for (uint32_t k = at; k + h.g <= at + m && p; k++) p = zs_flt_has(slot, zs_flt_bit(val[k], 0, h.L)) && zs_flt_has(slot, zs_flt_bit(val[k], 1, h.L));
            some |= p; every &= p;
        }
        passes = Q.mode == ZSMI_find_none || (Q.mode == ZSMI_find_any ? some || shortOnes : every);      // rules 9, 10: a short pattern passes every frame
        if (passes) {
            const uint32_t *w = (const uint32_t *)slot;                    // (the filter is 8-byte aligned, the slots behind 40 bytes)
            ones = true;
            for (uint32_t k = 0; k < bytes / 4u && ones; k++) ones = w[k] == ~0u;
        }
    }
    if (i < frameCount) pass[i] = passes ? 1u : 0u;
    const uint32_t saturated = zs_ridx_block_sum(ones ? 1u : 0u, slots);
    if (tid == 0 && saturated) atomicAdd(&sums->saturated, (unsigned long long)saturated);
}
// offsets[0 .. frameCount]: the scan of pass.  The passing frames, ascending, to frames[0, capacity); one lane: result = {total, written,
// frames tested, all-ones slots among the total}, or {(uint64_t)-code, 0, 0, 0}.  The grid is max(the frames' blocks, 1)
__global__ void __launch_bounds__(256)
k_filter_list(const uint32_t *__restrict__ pass, const uint64_t *__restrict__ offsets, uint32_t firstFrame, uint32_t frameCount, const ZsFltSums *__restrict__ sums,
              uint32_t *__restrict__ frames, uint64_t capacity, uint64_t *__restrict__ result)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const uint32_t status = (uint32_t)sums->status;
    if (i == 0) {
        const uint64_t total = offsets[frameCount];
        result[0] = status ? 0ull - (uint64_t)status : total;
        result[1] = status ? 0ull : (total < capacity ? total : capacity);
        result[2] = status ? 0ull : frameCount;
        result[3] = status ? 0ull : sums->saturated;
    }
    if (status || i >= frameCount || !pass[i]) return;
    const uint64_t at = offsets[i];
    if (at < capacity) frames[at] = firstFrame + i;
}

// ---- host ----
extern "C" size_t zsmi_frameFilterSize(size_t n, unsigned log2Bits) { return zs_flt_size(n, log2Bits); }
extern "C" size_t zsmi_buildFrameFilter(void *dst, size_t dstCapacity, const void *src, size_t srcSize, const uint32_t *frameSizes, size_t n, int delim, unsigned gram, unsigned log2Bits)
{
    return zs_flt_build(dst, dstCapacity, src, srcSize, frameSizes, n, delim, gram, log2Bits);
}
extern "C" int zsmi_readFrameFilter(const void *src, size_t srcSize, zsmi_frameFilterInfo *info) { return zs_flt_read(src, srcSize, info); }
extern "C" int zsmi_filterFrames(const void *filter, size_t filterSize, const zsmi_findQuery *q, uint32_t firstFrame, uint32_t frameCount,
                                 uint32_t *frames, size_t capacity, uint64_t *result)
{
    return zs_flt_filter(filter, filterSize, q, firstFrame, frameCount, frames, capacity, result);
}
// the words every build keeps in context staging: the sums, then the carry - the content's byte in front of the next window
struct FltWords { ZsFltSums *dSums; uint8_t *dCarry; };
static int fltWords(zsmi_ctx *c, size_t more, FltWords &w)
{
    if (!c->sSizes.reserve(sizeof(ZsFltSums) + 8 + more)) return ZSMI_error_memory_allocation;
    w.dSums = (ZsFltSums *)c->sSizes.p; w.dCarry = (uint8_t *)(w.dSums + 1);
    return 0;
}
// what the builds check of the filter's place, behind their own arguments
static int fltRoomCheck(uint64_t n, int delim, unsigned g, unsigned L)
{
    if (!zs_flt_params_ok(delim, g, L)) return ZSMI_error_parameter_outOfBound;
    return zs_flt_count_ok(n, L) ? 0 : ZSMI_error_frameIndex_tooLarge;
}
// the body's tiles over dText[0, size) whose first frame is frame0 of the filter; the slots zeroed by the caller
static int fltText(zsmi_ctx *c, const void *dText, uint64_t size, const uint64_t *dPlaces, uint32_t n, uint32_t frame0, int delim, uint32_t g, uint32_t L,
                   const uint8_t *dPrev, bool atEnd, const uint32_t *dCode, void *dFilter, ZsFltSums *dSums)
{
    const uint64_t tiles64 = std::max<uint64_t>((size + ZS_SPLIT_TILE - 1) / ZS_SPLIT_TILE, 1);
    if (tiles64 > 0x7FFFFFFFull) return ZSMI_error_memory_allocation;
    uint32_t *slots = (uint32_t *)((uint8_t *)dFilter + ZS_FLT_FIXED + (uint64_t)frame0 * zs_flt_slot_bytes(L));
    LAUNCH(c, "k_filter_tiles", k_filter_tiles, dim3((uint32_t)tiles64), dim3(256), 0, (const uint8_t *)dText, size, (uint32_t)delim, g, L, dPlaces, n, dPrev, atEnd ? 1u : 0u,
           dCode, slots, dSums);
    return 0;
}
// the reduction and the header behind every tile of the content
static int fltFinish(zsmi_ctx *c, void *dFilter, uint32_t n, int delim, uint32_t g, uint32_t L, uint64_t size, ZsFltSums *dSums, uint64_t *dResult)
{
    const uint64_t words = (uint64_t)n << (L - 6u);
    const uint32_t grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((words + 255) / 256, 4096));
    LAUNCH(c, "k_filter_check", k_filter_check, dim3(grid), dim3(256), 0, (const uint8_t *)dFilter, zs_flt_frame_size(n, L), n, L, dSums);
    LAUNCH(c, "k_filter_built", k_filter_built, dim3(1), dim3(64), 0, (uint8_t *)dFilter, n, (uint32_t)delim, g, L, size, (const ZsFltSums *)dSums, dResult);
    return c->launched();
}
extern "C" int zsmi_buildFrameFilterDevice(zsmi_ctx *c, const void *dText, uint64_t size, const uint64_t *dPlaces, uint32_t n, int delim, unsigned gram, unsigned log2Bits,
                                           void *dFilter, uint64_t capacity, uint64_t *dResult)
{
    if (!c) return ZSMI_error_init_missing;
    if (!dResult || !dPlaces || !dFilter) return ZSMI_error_GENERIC;
    if (const int e = fltRoomCheck(n, delim, gram, log2Bits)) return e;
    if (size && !dText) return ZSMI_error_srcSize_wrong;
    if ((uintptr_t)dFilter & 7u) return ZSMI_error_parameter_outOfBound;
    if (capacity < zs_flt_frame_size(n, log2Bits)) return ZSMI_error_dstSize_tooSmall;
    if (const int e = c->bind()) return e;
    FltWords w;
    if (const int e = fltWords(c, 0, w)) return e;
    if (const int e = c->fill(w.dSums, 0, sizeof(ZsFltSums))) return e;
    if (n) if (const int e = c->fill((uint8_t *)dFilter + ZS_FLT_FIXED, 0, (size_t)n * zs_flt_slot_bytes(log2Bits))) return e;
    if (const int e = fltText(c, dText, size, dPlaces, n, 0, delim, gram, log2Bits, nullptr, true, nullptr, dFilter, w.dSums)) return e;
    return fltFinish(c, dFilter, n, delim, gram, log2Bits, size, w.dSums, dResult);
}
// one window of an archive: findDecode with nothing behind its words, whose layout scan - the places of the frames in dWork - is the
// body's places (recindex.hip's recidxWindow); then the text's last byte to the carry word, for the window behind
static int fltWindow(zsmi_ctx *c, const zsmi_seekable *sk, int delim, uint32_t g, uint32_t L, uint32_t firstFrame, uint32_t frameCount, void *dWork, void *dFilter, const FltWords &w)
{
    FindDecoded d;
    if (const int e = findDecode(c, sk, firstFrame, frameCount, dWork, 0, 0, d)) return e;
    const bool atStart = sk->t.dOff[firstFrame] == 0, atEnd = sk->t.dOff[(size_t)firstFrame + frameCount] == sk->t.dOff[sk->t.n];
    if (const int e = fltText(c, dWork, d.bytes, d.dListAt, frameCount, firstFrame, delim, g, L, atStart ? nullptr : w.dCarry, atEnd, d.dCode, dFilter, w.dSums)) return e;
    return d.bytes ? c->onDevice(w.dCarry, (const uint8_t *)dWork + d.bytes - 1, 1) : 0;
}
// the checks of the archive builds, in the rebuild's order (seekable.hip's seekWindowCheck over the whole archive, the filter's shape as
// the rule) with the filter where firstRecord stood, then the filter's place
static int fltArchiveCheck(const zsmi_ctx *c, const zsmi_seekable *sk, int delim, unsigned g, unsigned L, bool ownWork, const void *work, uint64_t workCapacity,
                           const void *filter, uint64_t capacity, const void *result)
{
    if (const int e = seekWindowCheck(c, sk, !result || !filter, [&] { return fltRoomCheck(sk->t.n, delim, g, L); }, 0, sk ? sk->t.n : 0, ownWork, work, workCapacity)) return e;
    if (!ownWork && ((uintptr_t)filter & 7u)) return ZSMI_error_parameter_outOfBound;
    if (capacity < zs_flt_frame_size(sk->t.n, L)) return ZSMI_error_dstSize_tooSmall;
    return 0;
}
extern "C" int zsmi_seekableBuildFrameFilterResident(zsmi_ctx *c, const zsmi_seekable *sk, int delim, unsigned gram, unsigned log2Bits, void *dWork, uint64_t workCapacity,
                                                     void *dFilter, uint64_t capacity, uint64_t *dResult)
{
    if (const int e = fltArchiveCheck(c, sk, delim, gram, log2Bits, false, dWork, workCapacity, dFilter, capacity, dResult)) return e;
    if (const int e = c->bind()) return e;
    const uint32_t N = sk->t.n;
    FltWords w;
    if (const int e = fltWords(c, 0, w)) return e;
    if (const int e = findDecodeReserve(c, N, 0, 0)) return e;              // the one window's scratch, before the fills are queued
    if (const int e = c->fill(w.dSums, 0, sizeof(ZsFltSums))) return e;
    if (N) {
        if (const int e = c->fill((uint8_t *)dFilter + ZS_FLT_FIXED, 0, (size_t)N * zs_flt_slot_bytes(log2Bits))) return e;
        if (const int e = fltWindow(c, sk, delim, gram, log2Bits, 0, N, dWork, dFilter, w)) return e;
    }
    return fltFinish(c, dFilter, N, delim, gram, log2Bits, sk->t.dOff[N], w.dSums, dResult);
}
// host buffers out, one wait: seekable.hip's window plan, the windows in ascending order on the stream; the filter grows in context
// staging, the work buffer is the context's
extern "C" int zsmi_seekableBuildFrameFilterHost(zsmi_ctx *c, const zsmi_seekable *sk, int delim, unsigned gram, unsigned log2Bits, void *filter, size_t capacity, uint64_t *result)
{
    if (const int e = fltArchiveCheck(c, sk, delim, gram, log2Bits, true, nullptr, 0, filter, capacity, result)) return e;
    if (const int e = c->bind()) return e;
    const uint32_t N = sk->t.n;
    const SeekWindows plan = seekCutWindows(sk, seekWindowLimit());
    // every window's scratch at once, before the first is queued: the largest text, the most frames
    const size_t total = (size_t)zs_flt_frame_size(N, log2Bits);
    FltWords w;
    if (const int e = fltWords(c, 4 * sizeof(uint64_t), w)) return e;
    if (!c->sDst.reserve(total + 64) || !c->seek.dDec.reserve(plan.most + 64)) return ZSMI_error_memory_allocation;
    if (const int e = findDecodeReserve(c, plan.mostFrames, 0, 0)) return e;
    uint64_t *dResult = (uint64_t *)(w.dCarry + 8);
    std::vector<uint8_t> staged(total);
    int rc = c->fill(w.dSums, 0, sizeof(ZsFltSums));
    if (!rc && N) rc = c->fill((uint8_t *)c->sDst.p + ZS_FLT_FIXED, 0, total - ZS_FLT_FIXED);
    for (size_t k = 0; k < plan.list.size() && !rc; k++) rc = fltWindow(c, sk, delim, gram, log2Bits, plan.list[k].first, plan.list[k].second, c->seek.dDec.p, c->sDst.p, w);
    if (!rc) rc = fltFinish(c, c->sDst.p, N, delim, gram, log2Bits, sk->t.dOff[N], w.dSums, dResult);
    if (!rc) rc = c->toHost(result, dResult, 4 * sizeof(uint64_t));
    if (!rc) rc = c->toHost(staged.data(), c->sDst.p, total);
    const int waited = c->wait();
    if (rc || waited) return rc ? rc : waited;
    memcpy(filter, staged.data(), total);
    return 0;
}
extern "C" int zsmi_checkFrameFilterDevice(zsmi_ctx *c, const void *dFilter, uint64_t filterSize, uint64_t *dResult)
{
    if (!c) return ZSMI_error_init_missing;
    if (!dFilter || !dResult) return ZSMI_error_GENERIC;
    if ((uintptr_t)dFilter & 7u) return ZSMI_error_parameter_outOfBound;
    if (const int e = c->bind()) return e;
    FltWords w;
    if (const int e = fltWords(c, 0, w)) return e;
    if (const int e = c->fill(w.dSums, 0, sizeof(ZsFltSums))) return e;
    const uint64_t words = filterSize > ZS_FLT_FIXED ? (filterSize - ZS_FLT_FIXED) / 8 : 0;
    const uint32_t grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((words + 255) / 256, 4096));
    LAUNCH(c, "k_filter_check", k_filter_check, dim3(grid), dim3(256), 0, (const uint8_t *)dFilter, filterSize, 0u, 0u, w.dSums);
    LAUNCH(c, "k_filter_judged", k_filter_judged, dim3(1), dim3(64), 0, (const uint8_t *)dFilter, filterSize, (const ZsFltSums *)w.dSums, dResult);
    return c->launched();
}
// what the host can check of a query without the filter's delimiter: zs_findq_check's shape checks, in its order
static int fltQueryShape(const zsmi_findQuery *q)
{
    if (q->nPatterns == 0 || q->nPatterns > ZSMI_FIND_MAX_PATTERNS || q->mode > ZSMI_find_none || (q->flags & ~ZSMI_FIND_IGNORE_CASE)) return ZSMI_error_parameter_outOfBound;
    uint32_t sum = 0;
    for (uint32_t j = 0; j < q->nPatterns; j++) {
        if (!q->patterns[j]) return ZSMI_error_GENERIC;
        if (q->patternSizes[j] == 0 || q->patternSizes[j] > ZS_FIND_MAX_PATTERN) return ZSMI_error_parameter_outOfBound;
        sum += q->patternSizes[j];
        if (sum > ZS_FIND_MAX_PATTERN) return ZSMI_error_parameter_outOfBound;
    }
    return 0;
}
extern "C" int zsmi_filterFramesDevice(zsmi_ctx *c, const void *dFilter, uint64_t filterSize, const zsmi_findQuery *q, uint32_t firstFrame, uint32_t frameCount,
                                       uint32_t *dFrames, uint64_t capacity, uint64_t *dResult)
{
    if (!c) return ZSMI_error_init_missing;
    if (!dFilter || !q || !dResult || (capacity && !dFrames)) return ZSMI_error_GENERIC;
    if (const int e = fltQueryShape(q)) return e;
    if ((uintptr_t)dFilter & 7u) return ZSMI_error_parameter_outOfBound;
    if (const int e = c->bind()) return e;
    // scratch: the sums; the offsets [frameCount + 1], the verdicts [frameCount]; the scan's tile sums
    FltWords w;
    if (const int e = fltWords(c, 0, w)) return e;
    if (!c->seek.dMeta.reserve(((size_t)frameCount + 1) * sizeof(uint64_t) + (size_t)frameCount * sizeof(uint32_t)) ||
        !c->dScan.reserve(sizeof(uint64_t) * ((size_t)frameCount / ZS_SCAN_TILE + 2))) return ZSMI_error_memory_allocation;
    uint64_t *dOffsets = (uint64_t *)c->seek.dMeta.p;
    uint32_t *dPass = (uint32_t *)(dOffsets + frameCount + 1);
    const uint32_t grid = std::max(1u, (uint32_t)(((uint64_t)frameCount + 255) / 256));
    if (const int e = c->fill(w.dSums, 0, sizeof(ZsFltSums))) return e;
    LAUNCH(c, "k_filter_test", k_filter_test, dim3(grid), dim3(256), 0, (const uint8_t *)dFilter, filterSize, findQuery(q), firstFrame, frameCount, dPass, w.dSums);
    if (const int e = scanOffsets(c, "k_filter_scan", (const uint32_t *)dPass, nullptr, frameCount, 1u, nullptr, dOffsets)) return e;
    LAUNCH(c, "k_filter_list", k_filter_list, dim3(grid), dim3(256), 0, (const uint32_t *)dPass, (const uint64_t *)dOffsets, firstFrame, frameCount, (const ZsFltSums *)w.dSums,
           dFrames, capacity, dResult);
    return c->launched();
}
