// seekable.hip -- zstd's seekable format over the batch paths of zsmi_api.hip (zsmi_ctx.h declares them).
//
//   archive    = frame_0 .. frame_{n-1} | seek table
//   seek table = 0x184D2A5E | Frame_Size | entry_0 .. entry_{n-1} | Number_Of_Frames | Seek_Table_Descriptor | 0x8F92EAB1   (little-endian)
//   entry      = Compressed_Size | Decompressed_Size [| Checksum: low 32 bits of XXH64 (seed 0) of the frame's content, when descriptor bit 7]
//
// Compress: the frames are the chunks of one zsmi_compressBatchDevice call (chunk i = src[i F, min((i + 1) F, size))) into context staging at
// compressBound(F) spacing; k_seek_hash hashes the INPUT of each frame (checksum flag), the pack kernels close the gaps into dDst, k_seek_table
// writes the table behind them and the archive's size (or the first failing frame's code).
// Decompress: the table is read and checked on the host; the frames that overlap the range are items of the batch decoder with their exact
// Decompressed_Size as capacity - the ones wholly inside the range decode straight into dDst, a partial first / last one into context scratch
// and is copied in slices - then k_seek_verify checks every decoded frame's size and checksum against its entry.

#include "zsmi_wave.h"            // zs_block_copy, xxh64_quad, rd32
#include "entropy_kernels.hip"    // k_pack_offsets
#include "decode_kernels.hip"     // the decoder's error codes (E_*)
#include "zsmi_ctx.h"
#include <algorithm>

static const uint32_t kSeekSkippableMagic = 0x184D2A5Eu, kSeekableMagic = 0x8F92EAB1u;
static const uint64_t kSeekMaxFrames = 0x8000000ull, kSeekMaxFrameSize = 1ull << 30;
static const uint64_t kSeekTableFixed = 17;          // skippable header (8) + footer (9)
static const uint32_t kSeekHashAhead = 16;           // stripes a lane has in flight in k_seek_hash

// ---- kernels ----
__device__ __forceinline__ void seek_st32(uint8_t *p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24); }
__device__ __forceinline__ bool seek_isErr(uint32_t s) { return s > 0xFFFFFF88u; }

// XXH64 of each frame's input: one quad a frame (16 a wavefront), kSeekHashAhead stripes a lane in flight.  At 64 KiB frames 1 GiB is 16384
// quads - one wavefront a SIMD - so the loads of one lane, not the number of wavefronts, are what hides the memory latency.
__global__ void __launch_bounds__(64) k_seek_hash(const uint8_t *__restrict__ src, uint64_t srcSize, uint64_t frameSize, uint32_t n, uint32_t *__restrict__ hashes)
{
    const uint32_t q = blockIdx.x * 16 + (threadIdx.x >> 2);
    const bool real = q < n;
    const uint32_t f = real ? q : n - 1u;
    const uint64_t off = (uint64_t)f * frameSize;
    const uint64_t len = real ? min(frameSize, srcSize - off) : 0ull;
    const uint64_t h = xxh64_quad<kSeekHashAhead>(src + off, len);      // (every lane of a quad calls: its four accumulators)
    if (real && (threadIdx.x & 3u) == 0) hashes[f] = (uint32_t)h;
}
// frame i from staging (at i * stride) to its packed place; a failed frame (an error code for its size) moves nothing
__global__ void k_seek_pack(const uint8_t *__restrict__ stage, uint64_t stride, const uint32_t *__restrict__ sizes, const uint64_t *__restrict__ packedOffsets, uint8_t *__restrict__ dst)
{
    const uint32_t i = blockIdx.x;
    const uint32_t sz = seek_isErr(sizes[i]) ? 0u : sizes[i];
    zs_block_copy(dst + packedOffsets[i], stage + (uint64_t)i * stride, sz, threadIdx.x, blockDim.x);
}
// the table behind the packed frames: one entry a thread, the header and the footer from the first; a failed frame's (index << 8 | code) goes to
// *err (set to ~0 before), the lowest wins
__global__ void k_seek_table(const uint32_t *__restrict__ sizes, const uint64_t *__restrict__ packedOffsets, const uint32_t *__restrict__ hashes, uint64_t srcSize,
                             uint64_t frameSize, uint32_t n, int checksum, uint8_t *__restrict__ dst, unsigned long long *err)
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
    if (seek_isErr(s)) atomicMin(err, ((unsigned long long)i << 8) | (0u - s));
    uint8_t *e = t + 8 + (uint64_t)i * E;
    const uint64_t off = (uint64_t)i * frameSize;
    seek_st32(e, seek_isErr(s) ? 0u : s); seek_st32(e + 4, (uint32_t)min(frameSize, srcSize - off));
    if (checksum) seek_st32(e + 8, hashes[i]);
}
__global__ void k_seek_finish(const uint64_t *__restrict__ packedOffsets, uint32_t n, uint32_t entryBytes, const unsigned long long *__restrict__ err, uint64_t *archiveSize)
{
    const unsigned long long e = *err;
    *archiveSize = e == ~0ull ? packedOffsets[n] + kSeekTableFixed + (uint64_t)n * entryBytes : 0ull - (e & 0xFFu);
}

struct ZsSeekItem { uint64_t out; uint32_t size, hash, slot, pad; };     // a decoded frame: where its bytes are, its entry, its status word
struct ZsSeekSlices { uint64_t from[2], to[2], len[2]; };               // partial frames: scratch -> dDst
__global__ void k_seek_slice(const uint8_t *__restrict__ scratch, uint8_t *__restrict__ dst, ZsSeekSlices s)
{
    const uint32_t k = blockIdx.x;
    zs_block_copy(dst + s.to[k], scratch + s.from[k], (uint32_t)s.len[k], threadIdx.x, blockDim.x);
}
// one quad a decoded frame: its decoder status, its size against the entry (a frame the decoder found longer than its entry failed with
// dstSize_tooSmall: that is the same disagreement), its checksum (flag set).  The first failing frame in content order wins (*err, set to ~0 before).
__global__ void __launch_bounds__(64) k_seek_verify(const ZsSeekItem *__restrict__ items, uint32_t m, const uint32_t *__restrict__ status, int checksum, unsigned long long *err)
{
    const uint32_t q = blockIdx.x * 16 + (threadIdx.x >> 2);
    const bool real = q < m;
    const ZsSeekItem it = items[real ? q : m - 1u];
    const uint32_t s = real ? status[it.slot] : 0u;
    uint32_t code = 0;
    if (seek_isErr(s)) code = (0u - s) == E_dstSize_tooSmall ? (uint32_t)E_corruption_detected : 0u - s;
    else if (s != it.size) code = E_corruption_detected;
    const bool hash = real && checksum && code == 0;
    if (__ballot(hash)) {
        const uint64_t h = xxh64_quad<kSeekHashAhead>((const uint8_t *)it.out, hash ? it.size : 0u);
        if (hash && (uint32_t)h != it.hash) code = E_checksum_wrong;
    }
    if (real && code && (threadIdx.x & 3u) == 0) atomicMin(err, ((unsigned long long)q << 8) | code);
}
__global__ void k_seek_status(const unsigned long long *__restrict__ err, uint32_t *status)
{
    const unsigned long long e = *err;
    *status = e == ~0ull ? 0u : (uint32_t)(e & 0xFFu);
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
static int compressSeekableImpl(zsmi_ctx *c, const void *dSrc, uint64_t srcSize, void *dDst, uint64_t dstCapacity, uint64_t *dArchiveSize,
                                int level, uint32_t frameSize, int checksumFlag)
{
    if (!c) return ZSMI_error_init_missing;
    uint64_t F, n64;
    if (const int e = seekParams(srcSize, frameSize, F, n64)) return e;
    if (dstCapacity < seekBound(srcSize, F, n64, checksumFlag)) return ZSMI_error_dstSize_tooSmall;
    if (!dArchiveSize || !dDst || (srcSize && !dSrc)) return ZSMI_error_GENERIC;
    if (hipSetDevice(c->device) != hipSuccess) return ZSMI_error_GENERIC;
    const uint32_t n = (uint32_t)n64, E = checksumFlag ? 12u : 8u;
    const uint64_t stride = zsmi_compressBound(F);
    // per-frame words: sizes [n], hashes [n], then (8-aligned) packed offsets [n + 1] and the error word
    const size_t words = 2 * (size_t)n * sizeof(uint32_t);
    if (!c->seek.dMeta.reserve(words + ((size_t)n + 2) * sizeof(uint64_t))) return ZSMI_error_memory_allocation;
    uint32_t *dSizes = (uint32_t *)c->seek.dMeta.p, *dHash = dSizes + n;
    uint64_t *dPacked = (uint64_t *)((uint8_t *)c->seek.dMeta.p + words);
    unsigned long long *dErr = (unsigned long long *)(dPacked + n + 1);
    if (n) {
        if (!c->seek.dStage.reserve((n - 1) * stride + zsmi_compressBound(srcSize - (n64 - 1) * F))) return ZSMI_error_memory_allocation;
        std::vector<uint64_t> so(n), dof(n);
        std::vector<uint32_t> ss(n);
        for (uint32_t i = 0; i < n; i++) { so[i] = (uint64_t)i * F; ss[i] = (uint32_t)std::min<uint64_t>(F, srcSize - so[i]); dof[i] = (uint64_t)i * stride; }
        if (const int e = compressBatchDeviceImpl(c, dSrc, so.data(), ss.data(), n, c->seek.dStage.p, dof.data(), dSizes, level, nullptr)) return e;
        if (checksumFlag) LAUNCH(c, "k_seek_hash", k_seek_hash, dim3((n + 15) / 16), dim3(64), 0, (const uint8_t *)dSrc, srcSize, F, n, dHash);
    }
    LAUNCH(c, "k_pack_offsets", k_pack_offsets, dim3(1), dim3(1024), 0, (const uint32_t *)dSizes, n, dPacked);
    if (n) LAUNCH(c, "k_seek_pack", k_seek_pack, dim3(n), dim3(256), 0, (const uint8_t *)c->seek.dStage.p, stride, (const uint32_t *)dSizes, (const uint64_t *)dPacked, (uint8_t *)dDst);
    if (hipMemsetAsync(dErr, 0xFF, sizeof(*dErr), c->stream) != hipSuccess) return ZSMI_error_GENERIC;
    LAUNCH(c, "k_seek_table", k_seek_table, dim3(std::max<uint32_t>(1, (n + 255) / 256)), dim3(256), 0, (const uint32_t *)dSizes, (const uint64_t *)dPacked,
           (const uint32_t *)dHash, srcSize, F, n, checksumFlag ? 1 : 0, (uint8_t *)dDst, dErr);
    LAUNCH(c, "k_seek_finish", k_seek_finish, dim3(1), dim3(1), 0, (const uint64_t *)dPacked, n, E, (const unsigned long long *)dErr, dArchiveSize);
    return hipGetLastError() == hipSuccess ? 0 : ZSMI_error_GENERIC;
}
extern "C" int zsmi_compressSeekableDevice(zsmi_ctx *c, const void *dSrc, uint64_t srcSize, void *dDst, uint64_t dstCapacity,
                                           uint64_t *dArchiveSize, int level, uint32_t frameSize, int checksumFlag)
{
    return compressSeekableImpl(c, dSrc, srcSize, dDst, dstCapacity, dArchiveSize, level, frameSize, checksumFlag);
}
extern "C" size_t zsmi_compressSeekable(void *dst, size_t dstCapacity, const void *src, size_t srcSize, int level, uint32_t frameSize, int checksumFlag)
{
    uint64_t F, n;
    if (const int e = seekParams(srcSize, frameSize, F, n)) return ZSMI_ERR(e);
    const uint64_t bound = seekBound(srcSize, F, n, checksumFlag);
    Borrowed b; zsmi_ctx *c = b.c;
    if (!c) return ZSMI_ERR(ZSMI_error_GENERIC);
    if (hipSetDevice(c->device) != hipSuccess) return ZSMI_ERR(ZSMI_error_GENERIC);
    if (!c->sSrc.reserve(srcSize + 64) || !c->sDst.reserve(bound + 64) || !c->sSizes.reserve(sizeof(uint64_t))) return ZSMI_ERR(ZSMI_error_memory_allocation);
    if (srcSize && hipMemcpyAsync(c->sSrc.p, src, srcSize, hipMemcpyHostToDevice, c->stream) != hipSuccess) return ZSMI_ERR(ZSMI_error_GENERIC);
    if (const int rc = compressSeekableImpl(c, c->sSrc.p, srcSize, c->sDst.p, bound, (uint64_t *)c->sSizes.p, level, frameSize, checksumFlag)) {
        (void)hipStreamSynchronize(c->stream);
        return ZSMI_ERR(rc);
    }
    uint64_t size = 0;
    if (hipMemcpyAsync(&size, c->sSizes.p, sizeof size, hipMemcpyDeviceToHost, c->stream) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) return ZSMI_ERR(ZSMI_error_GENERIC);
    if (zsmi_isError(size)) return size;
    if (size > dstCapacity) return ZSMI_ERR(ZSMI_error_dstSize_tooSmall);
    if (hipMemcpyAsync(dst, c->sDst.p, size, hipMemcpyDeviceToHost, c->stream) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) return ZSMI_ERR(ZSMI_error_GENERIC);
    return size;
}

// ---- range reads ----
// the frames that overlap the content range [a, b) (a < b <= content size): first .. last
static void seekSpan(const SeekTable &t, uint64_t a, uint64_t b, uint32_t &first, uint32_t &last)
{
    first = (uint32_t)(std::upper_bound(t.dOff.begin(), t.dOff.end(), a) - t.dOff.begin()) - 1;
    last = (uint32_t)(std::lower_bound(t.dOff.begin(), t.dOff.end(), b) - t.dOff.begin()) - 1;
}
// Queue the decode of [a, b) on the context's stream.  Frame i's compressed bytes are at dFrames + t.cOff[i] - base.  The context must be idle
// on the host side (seek.hItems is refilled): the callers have waited for its stream.
static int seekReadQueue(zsmi_ctx *c, const SeekTable &t, const uint8_t *dFrames, uint64_t base, uint64_t a, uint64_t b, uint8_t *dDst, uint32_t *dStatus)
{
    if (hipMemsetAsync(dStatus, 0, sizeof(uint32_t), c->stream) != hipSuccess) return ZSMI_error_GENERIC;
    if (a == b) return 0;
    uint32_t first, last;
    seekSpan(t, a, b, first, last);
    const uint32_t m = last - first + 1;
    // frames wholly inside the range: items [in0, in1) of the span, straight into dDst; the first and the last may be partial (scratch)
    const bool partFirst = t.dOff[first] < a || t.dOff[first + 1] > b, partLast = last != first && t.dOff[last + 1] > b;
    const uint32_t in0 = partFirst ? 1 : 0, in1 = partLast ? m - 1 : m;
    // status words: [m] for the span in content order, [2] behind them for the partial frames' decode call; (8-aligned) the error word; the verify list
    const size_t words = (((size_t)m + 3) & ~(size_t)1) * sizeof(uint32_t);
    if (!c->seek.dMeta.reserve(words + sizeof(uint64_t) + (size_t)m * sizeof(ZsSeekItem)) || !c->seek.hItems.reserve((size_t)m * sizeof(ZsSeekItem))) return ZSMI_error_memory_allocation;
    uint32_t *dSt = (uint32_t *)c->seek.dMeta.p;
    unsigned long long *dErr = (unsigned long long *)((uint8_t *)c->seek.dMeta.p + words);
    ZsSeekItem *dItems = (ZsSeekItem *)(dErr + 1);
    ZsSeekItem *hi = (ZsSeekItem *)c->seek.hItems.p;
    std::vector<uint64_t> so, dof; std::vector<uint32_t> ss, caps;
    auto item = [&](uint32_t k, uint8_t *dBase, uint64_t at, uint32_t slot) {
        const uint32_t i = first + k;
        so.push_back(t.cOff[i] - base); ss.push_back(t.cSize[i]); caps.push_back(t.dSize[i]); dof.push_back(at);
        hi[k] = { (uint64_t)(uintptr_t)(dBase + at), t.dSize[i], t.hash[i], slot, 0 };
    };
    if (in1 > in0) {
        for (uint32_t k = in0; k < in1; k++) item(k, dDst, t.dOff[first + k] - a, k);
        if (const int e = decompressBatchDeviceImpl(c, dFrames, so.data(), ss.data(), in1 - in0, dDst, dof.data(), caps.data(), dSt + in0, nullptr)) return e;
    }
    if (partFirst || partLast) {
        uint32_t parts[2], np = 0;
        if (partFirst) parts[np++] = 0;
        if (partLast) parts[np++] = m - 1;
        const uint64_t partBytes = (uint64_t)t.dSize[first + parts[0]] + (np > 1 ? t.dSize[first + parts[1]] : 0u);
        if (!c->seek.dDec.reserve(partBytes + 64)) return ZSMI_error_memory_allocation;
        uint8_t *dS = (uint8_t *)c->seek.dDec.p;
        so.clear(); dof.clear(); ss.clear(); caps.clear();
        ZsSeekSlices sl = {};
        uint64_t pos = 0;
        for (uint32_t j = 0; j < np; j++) {
            const uint32_t i = first + parts[j];
            item(parts[j], dS, pos, m + j);
            const uint64_t lo = std::max(a, t.dOff[i]), hi2 = std::min(b, t.dOff[i + 1]);
            sl.from[j] = pos + (lo - t.dOff[i]); sl.to[j] = lo - a; sl.len[j] = hi2 - lo;
            pos += t.dSize[i];
        }
        if (const int e = decompressBatchDeviceImpl(c, dFrames, so.data(), ss.data(), np, dS, dof.data(), caps.data(), dSt + m, nullptr)) return e;
        LAUNCH(c, "k_seek_slice", k_seek_slice, dim3(np), dim3(256), 0, (const uint8_t *)dS, dDst, sl);
    }
    if (hipMemcpyAsync(dItems, hi, (size_t)m * sizeof(ZsSeekItem), hipMemcpyHostToDevice, c->stream) != hipSuccess) return ZSMI_error_GENERIC;
    if (hipMemsetAsync(dErr, 0xFF, sizeof(*dErr), c->stream) != hipSuccess) return ZSMI_error_GENERIC;
    LAUNCH(c, "k_seek_verify", k_seek_verify, dim3((m + 15) / 16), dim3(64), 0, (const ZsSeekItem *)dItems, m, (const uint32_t *)dSt, t.checksum ? 1 : 0, dErr);
    LAUNCH(c, "k_seek_status", k_seek_status, dim3(1), dim3(1), 0, (const unsigned long long *)dErr, dStatus);
    return hipGetLastError() == hipSuccess ? 0 : ZSMI_error_GENERIC;
}
extern "C" int zsmi_decompressSeekableDevice(zsmi_ctx *c, const void *dSrc, uint64_t srcSize, uint64_t offset, uint64_t length,
                                             void *dDst, uint64_t *written, uint32_t *dStatus)
{
    if (!c) return ZSMI_error_init_missing;
    if (!dSrc || srcSize < 9) return ZSMI_error_prefix_unknown;
    if (!dStatus || !written) return ZSMI_error_GENERIC;
    if (hipSetDevice(c->device) != hipSuccess) return ZSMI_error_GENERIC;
    // the archive's tail, once: it holds the whole table up to 256 KiB (16384 entries with checksums: 1 GiB in 64 KiB frames); a larger
    // table is read again at its size
    std::vector<uint8_t> tail(std::min<uint64_t>(srcSize, 256u << 10));
    const uint8_t *src = (const uint8_t *)dSrc;
    if (hipMemcpyAsync(tail.data(), src + srcSize - tail.size(), tail.size(), hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess) return ZSMI_error_GENERIC;
    SeekTable t;
    if (const int e = seekFooter(tail.data() + tail.size() - 9, srcSize, t)) return e;
    if (t.tableSize > tail.size()) {
        tail.resize(t.tableSize);
        if (hipMemcpyAsync(tail.data(), src + srcSize - t.tableSize, t.tableSize, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
            hipStreamSynchronize(c->stream) != hipSuccess) return ZSMI_error_GENERIC;
    }
    if (const int e = seekEntries(tail.data() + tail.size() - t.tableSize, srcSize, t)) return e;
    const uint64_t content = t.dOff[t.n];
    if (offset > content) return ZSMI_error_parameter_outOfBound;
    const uint64_t b = offset + std::min(length, content - offset);
    *written = b - offset;
    if (b > offset && !dDst) return ZSMI_error_GENERIC;
    return seekReadQueue(c, t, src, 0, offset, b, (uint8_t *)dDst, dStatus);
}
extern "C" size_t zsmi_decompressSeekable(void *dst, size_t dstCapacity, const void *src, size_t srcSize, unsigned long long offset)
{
    SeekTable t;
    if (const int e = seekParseHost(src, srcSize, t)) return ZSMI_ERR(e);
    const uint64_t content = t.dOff[t.n];
    if (offset > content) return ZSMI_ERR(ZSMI_error_parameter_outOfBound);
    const uint64_t a = offset, b = a + std::min<uint64_t>(dstCapacity, content - a);
    if (a == b) return 0;
    uint32_t first, last;
    seekSpan(t, a, b, first, last);
    const uint64_t base = t.cOff[first], span = t.cOff[last + 1] - base;       // only the overlapping frames' bytes go to the device
    Borrowed bw; zsmi_ctx *c = bw.c;
    if (!c) return ZSMI_ERR(ZSMI_error_GENERIC);
    if (hipSetDevice(c->device) != hipSuccess) return ZSMI_ERR(ZSMI_error_GENERIC);
    if (!c->sSrc.reserve(span + 64) || !c->sDst.reserve(b - a + 64) || !c->sSizes.reserve(sizeof(uint32_t))) return ZSMI_ERR(ZSMI_error_memory_allocation);
    // (a borrowed context is idle: its last user waited for its stream)
    if (hipMemcpyAsync(c->sSrc.p, (const uint8_t *)src + base, span, hipMemcpyHostToDevice, c->stream) != hipSuccess) return ZSMI_ERR(ZSMI_error_GENERIC);
    if (const int rc = seekReadQueue(c, t, (const uint8_t *)c->sSrc.p, base, a, b, (uint8_t *)c->sDst.p, (uint32_t *)c->sSizes.p)) {
        (void)hipStreamSynchronize(c->stream);
        return ZSMI_ERR(rc);
    }
    uint32_t status = 0;
    if (hipMemcpyAsync(&status, c->sSizes.p, sizeof status, hipMemcpyDeviceToHost, c->stream) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) return ZSMI_ERR(ZSMI_error_GENERIC);
    if (status) return ZSMI_ERR(status);
    if (hipMemcpyAsync(dst, c->sDst.p, b - a, hipMemcpyDeviceToHost, c->stream) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) return ZSMI_ERR(ZSMI_error_GENERIC);
    return b - a;
}
