// libzsmi.so : C ABI (include/zsmi.h) over the HIP kernels.  Host side of the codec: contexts, device
// workspaces, block planning, kernel launches, staging for host-buffer calls.  No CPU codec path exists
// in this library: every compress/decompress call launches the gfx950 kernels or fails.
//
// Single translation unit: the kernel sources are included so that launches and kernels share one code object.  Every file includes what
// it uses; the list is the library's table of contents.
#include "zsmi_status.h"          // the size word: a byte count or an error code, host and device
#include "zsmi_device.h"          // format constants, block / unit / sequence records, unaligned loads and stores
#include "zsmi_scratch.h"         // the scratch layouts: the table of the compress buffers, the slot accessors and borrowings of both pipelines, DecLists
#include "zsmi_wave.h"            // device primitives of more than one kernel file: wave_*, zs_block_copy, rd16/24/32, xxh64_quad
#include "zsmi_plan.h"            // the compress plan's rule for one chunk: blocks and units of a size, host and device
#include "zsmi_frame.h"           // the readers of the container headers (frame, block, literals section, stream split) and the container walker: device and host
#include "lz_kernels.hip"         // encoder, LZ stage: k_lz_candidates, k_lz_walk, k_lz_stitch, k_lz_dict_tables
#include "entropy_kernels.hip"    // encoder, entropy stage: k_encode_sequences, k_encode_literals, k_assemble_frames, k_frame_checksum; k_train_stats, k_pack_*
#include "plan_kernels.hip"       // encoder, the plan built on the device (the resident call): k_plan_chunks, k_plan_blocks, k_plan_refuse; k_compress_bounds
#include "decode_kernels.hip"     // general decoder: k_decode_frames, and the decoder routines the fast path shares; loadDictEntropy, the one reader of a dictionary; k_frame_sizes, k_dec_items
#include "decode_fast.hip"        // fast decode path: k_dec_prep, k_dec_huffman, k_dec_sequences, k_dec_entropy, k_dec_execute, k_dec_checksum, k_dec_collect; k_dict_load (a dictionary -> its record for the host, a DDict's image)
#include "zsmi_ctx.h"             // host: zsmi_ctx with its buffers and stream verbs, LAUNCH, makeHandle, the batch entry points the features call
#include "seekable.hip"           // feature: seekable archives (kernels and host)
#include "dict_train.hip"         // feature: dictionary training and finalize (kernels and host)
#include "split.hip"              // feature: the record splitter - delimited records -> frame sizes and line numbers (kernels and host; the rule: zsmi_split.h)
#include "records.hip"            // feature: records by number from a record archive - firstRecord and record numbers -> the records' bytes (kernels and host; the rules: zsmi_records.h)
#include "find.hip"               // feature: find records by content - text or a window of a record archive and a literal pattern -> ascending record numbers (kernels and host; the rule: zsmi_find.h)
#include "findquery.hip"          // feature: find records by several patterns - any, all, none of up to 8 patterns, ASCII case folding -> ascending record numbers and hit sets (kernels and host; the rule: zsmi_findquery.h)
#include "findregex.hip"          // feature: find records by regular expression - a pattern compiled on the host into a minimal DFA, a state function carried across lanes, wavefronts and tiles -> ascending record numbers (kernels and host; the rule and the compiler: zsmi_regex.h)
#include "recindex.hip"           // feature: the record index of an archive - firstRecord rebuilt from text and frame borders, stored in the archive as a skippable frame, loaded from it (kernels and host; the rule and the frame: zsmi_recindex.h)
#include "filter.hip"             // feature: frame filters - an n-gram Bloom filter a frame of a record archive, built from text, judged, and asked which frames can hold a query's records before any is decoded (kernels and host; the rule and the frame: zsmi_filter.h)
#include "findframes.hip"         // feature: the query search over a list of frames in device memory - what the filter call leaves goes straight into a search that decodes those frames and no others (kernels and host; the rule: its head)

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <condition_variable>
#include <map>
#include <mutex>
#include <new>
#include <algorithm>
#include <string>
#include <vector>

extern "C" unsigned zsmi_isError(size_t code) { return code > ZSMI_ERR(ZSMI_error_maxCode); }     // ZStdErrors.cs:95-98
extern "C" unsigned zsmi_getErrorCode(size_t code) { return zsmi_isError(code) ? (unsigned)(0 - code) : 0; }
extern "C" const char *zsmi_getErrorName(size_t code)
{
    switch (zsmi_getErrorCode(code)) {
    case 0: return "No error detected";
    case ZSMI_error_GENERIC: return "Error (generic)";
    case ZSMI_error_prefix_unknown: return "Unknown frame descriptor";
    case ZSMI_error_version_unsupported: return "Version not supported";
    case ZSMI_error_frameParameter_unsupported: return "Unsupported frame parameter";
    case ZSMI_error_frameParameter_windowTooLarge: return "Frame requires too much memory for decoding";
    case ZSMI_error_corruption_detected: return "Corrupted block detected";
    case ZSMI_error_checksum_wrong: return "Restored data doesn't match checksum";
    case ZSMI_error_dictionary_corrupted: return "Dictionary is corrupted";
    case ZSMI_error_dictionary_wrong: return "Dictionary mismatch";
    case ZSMI_error_parameter_unsupported: return "Unsupported parameter";
    case ZSMI_error_parameter_outOfBound: return "Parameter is out of bound";
    case ZSMI_error_tableLog_tooLarge: return "tableLog requires too much memory : unsupported";
    case ZSMI_error_maxSymbolValue_tooLarge: return "Unsupported max Symbol Value : too large";
    case ZSMI_error_maxSymbolValue_tooSmall: return "Specified maxSymbolValue is too small";
    case ZSMI_error_stage_wrong: return "Operation not authorized at current processing stage";
    case ZSMI_error_init_missing: return "Context should be init first";
    case ZSMI_error_memory_allocation: return "Allocation error : not enough memory";
    case ZSMI_error_workSpace_tooSmall: return "workSpace buffer is not large enough";
    case ZSMI_error_dstSize_tooSmall: return "Destination buffer is too small";
    case ZSMI_error_srcSize_wrong: return "Src size is incorrect";
    case ZSMI_error_frameIndex_tooLarge: return "Frame index is too large";
    case ZSMI_error_seekableIO: return "An I/O error occurred when reading/seeking";
    default: return "Unspecified error code";
    }
}
// ZSMI_SOURCE_FP: fingerprint of zstandard_amd/csrc the library was built from (zstandard_amd/_lib.py passes it; a library that ships with the
// sources is rebuilt when they differ, so a measurement can name the code it ran)
#ifndef ZSMI_SOURCE_FP
#define ZSMI_SOURCE_FP "unknown"
#endif
extern "C" const char *zsmi_versionString(void) { return "zsmi 0.3 (gfx950 HIP kernels; zstd frame format, decoder semantics of epam/Zstandard = zstd v1.3.4; sources " ZSMI_SOURCE_FP ")"; }

extern "C" size_t zsmi_compressBound(size_t srcSize)
{
    return (size_t)zs_compress_bound(srcSize);
}

// ---- ZStdDecompress.cs:518-532, 617-622: the content size the first frame's header states; 0 where it states none, is no zstd frame
//      (a skippable one too) or is refused ----
extern "C" unsigned long long zsmi_getDecompressedSize(const void *srcv, size_t srcSize)
{
    const uint8_t *src = (const uint8_t *)srcv;
    if (srcSize < 5 || rd32(src) != 0xFD2FB528u) return 0;
    const ZsFrameHeader fh = zs_read_frame_header(src, srcSize, 0);
    return (fh.status || fh.contentSize >= 0xFFFFFFFFFFFFFFFEull) ? 0 : fh.contentSize;
}

// ---- the size queries of a host buffer, every one the container walker's answer (zs_walk, zsmi_frame.h) - no device is touched.
//      zsmi_getFrameContentSize  GetFrameContentSize :518-531: what the first frame's header states (no block is looked at)
//      zsmi_findFrameCompressedSize  FindFrameCompressedSize :1957-2004: the bytes the first frame takes, a skippable one included
//      zsmi_findDecompressedSize  FindDecompressedSize :538-580, and zsmi_decompressBound (ZSTD_decompressBound): over every frame of src ----
extern "C" unsigned long long zsmi_getFrameContentSize(const void *src, size_t srcSize)
{
    const ZsWalk w = zs_walk<uint64_t>((const uint8_t *)src, srcSize, ZS_WALK_FIRST_HEADER);
    return w.nFrames ? w.contentSize : ZSMI_CONTENTSIZE_ERROR;              // (fewer than 5 bytes: no header)
}
extern "C" size_t zsmi_findFrameCompressedSize(const void *src, size_t srcSize)
{
    const ZsWalk w = zs_walk<uint64_t>((const uint8_t *)src, srcSize, ZS_WALK_FIRST_FRAME);
    if (w.status) return ZSMI_ERR(w.status);
    return w.nFrames ? (size_t)w.consumed : ZSMI_ERR(ZSMI_error_srcSize_wrong);
}
extern "C" unsigned long long zsmi_findDecompressedSize(const void *src, size_t srcSize)
{
    return zs_walk<uint64_t>((const uint8_t *)src, srcSize, ZS_WALK_ITEM).contentSize;
}
extern "C" unsigned long long zsmi_decompressBound(const void *src, size_t srcSize)
{
    return zs_walk<uint64_t>((const uint8_t *)src, srcSize, ZS_WALK_ITEM).bound;
}

// ---- the LZ kernels of a level: k_lz_candidates and k_lz_walk for small units (<= 64 KiB), big units and a dictionary call's prefixed units ----
// level <= 2: short table only ("fast"), walk ranges of 512 bytes; level >= 3: short + long table ("double"), ranges of 256 bytes;
// level >= 4 scores 8 candidates a step instead of 4 (paramsForLevel in oracle/zso_encoder.c)
typedef void (*CandFn)(const uint8_t *, const ZsUnitDesc *, uint32_t, uint16_t *, uint8_t *, uint32_t *, const ZsCDictEntry *, const uint32_t *, const uint32_t *);
typedef void (*WalkFn)(const uint8_t *, const ZsUnitDesc *, uint32_t, const uint16_t *, const uint8_t *, uint2 *, uint32_t, uint4 *, int,
                       const uint32_t *, const ZsCDictEntry *, const uint32_t *, const uint32_t *);
template <class Fn> struct LzKernel { const char *name; Fn fn; uint32_t threads; size_t lds; };
enum { kUnitsPfx, kUnitsSmall, kUnitsBig };       // (the order the kernels are launched in)
struct LzShape { LzKernel<CandFn> cand[3]; LzKernel<WalkFn> walk[3]; int walkLog; bool useLong; };
#define ZS_CAND_SHAPES(NT) { { "k_lz_candidates_dict", k_lz_candidates<ZS_TABLE_LOG_BIG, NT, true>, 64 * ZS_CAND_WAVES(NT), ZS_CAND_LDS(ZS_TABLE_LOG_BIG, NT) }, \
                             { "k_lz_candidates", k_lz_candidates<ZS_TABLE_LOG_SMALL, NT>, 64 * ZS_CAND_WAVES(NT), ZS_CAND_LDS(ZS_TABLE_LOG_SMALL, NT) }, \
                             { "k_lz_candidates_big", k_lz_candidates<ZS_TABLE_LOG_BIG, NT>, 64 * ZS_CAND_WAVES(NT), ZS_CAND_LDS(ZS_TABLE_LOG_BIG, NT) } }
#define ZS_WALK_SHAPES(LOOK, REPW, WLOG) { { "k_lz_walk_dict", ZS_WALK_KERNEL_PFX(LOOK, REPW, WLOG), ZS_WALK_THREADS(false, WLOG), ZS_WALK_LDS(ZS_UNIT_MAX) }, \
                                           { "k_lz_walk", ZS_WALK_KERNEL(LOOK, REPW, false, WLOG), ZS_WALK_THREADS(false, WLOG), ZS_WALK_LDS(ZS_BLOCK_MAX) }, \
                                           { "k_lz_walk_big", ZS_WALK_KERNEL(LOOK, REPW, true, WLOG), ZS_WALK_THREADS(true, WLOG), ZS_WALK_LDS(ZS_UNIT_MAX) } }
static const LzShape kLzShapes[3] = {
    { ZS_CAND_SHAPES(1), ZS_WALK_SHAPES(4, 8, 9), 9, false },     // level <= 2
    { ZS_CAND_SHAPES(2), ZS_WALK_SHAPES(4, 4, 8), 8, true },      // level 3
    { ZS_CAND_SHAPES(2), ZS_WALK_SHAPES(8, 8, 8), 8, true },      // level >= 4
};
#undef ZS_CAND_SHAPES
#undef ZS_WALK_SHAPES
static const LzShape &lzShape(int level) { return kLzShapes[level <= 2 ? 0 : (level == 3 ? 1 : 2)]; }

extern "C" zsmi_ctx *zsmi_createCtx(int device, void *hipStream)
{
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count == 0) return nullptr;
    zsmi_ctx *c = new zsmi_ctx();
    if (device < 0) { if (hipGetDevice(&c->device) != hipSuccess) { delete c; return nullptr; } }
    else { c->device = device; if (hipSetDevice(device) != hipSuccess) { delete c; return nullptr; } }
    if (hipStream) { c->stream = (hipStream_t)hipStream; c->ownStream = false; }
    else { if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) { delete c; return nullptr; } c->ownStream = true; }
    bool ok = true;
    // dynamic LDS beyond the 64 KiB default: refused requests fail here, not at the first launch.  k_lz_walk addresses its (dynamic) LDS
    // from 0: that holds as long as the kernel has no static LDS in front of it
    for (const LzShape &s : kLzShapes)
        for (int k = 0; k < 3; k++) {
            hipFuncAttributes fa;
            ok &= hipFuncSetAttribute((const void *)s.cand[k].fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)s.cand[k].lds) == hipSuccess;
            ok &= hipFuncSetAttribute((const void *)s.walk[k].fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)s.walk[k].lds) == hipSuccess &&
                  hipFuncGetAttributes(&fa, (const void *)s.walk[k].fn) == hipSuccess && fa.sharedSizeBytes == 0;
        }
    for (TurnBufs *t : { &c->hItems, &c->seek.hLists, &c->plan.hDictList }) ok &= t->create();
    if (!ok) { (void)hipGetLastError(); zsmi_freeCtx(c); return nullptr; }
    if (const char *e = getenv("ZSMI_BLOCKS_IN_FLIGHT")) { long v = atol(e); if (v >= 64) c->maxBlocksInFlight = (uint32_t)v; }
    if (const char *e = getenv("ZSMI_DEC_FAST")) c->decodeFast = atoi(e) != 0;
    { int v = 0; if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, c->device) == hipSuccess && v > 0) c->cus = (uint32_t)v; }
    if (const char *e = getenv("ZSMI_DEC_POOL")) { long v = atol(e); if (v >= 2 && v <= (1 << 20)) c->decodePool = (uint32_t)v; }
    if (const char *e = getenv("ZSMI_ITEMS_IN_FLIGHT")) { long v = atol(e); if (v >= 64 && v <= (1 << 20)) c->maxItemsInFlight = (uint32_t)v; }
#ifdef ZSMI_DEBUG_HOOKS
    if (const char *e = getenv("ZSMI_STOP_LIT")) c->stopLit = atoi(e);
    if (const char *e = getenv("ZSMI_STOP_AFTER_WALK")) c->stopAfterWalk = atoi(e);
    if (const char *e = getenv("ZSMI_STOP_SEQ")) c->stopSeq = atoi(e);
#endif
    return c;
}
extern "C" void zsmi_freeCtx(zsmi_ctx *c)
{
    if (!c) return;
    (void)hipStreamSynchronize(c->stream);
    for (auto &tl : c->launches) { (void)hipEventDestroy(tl.a); (void)hipEventDestroy(tl.b); }
    for (auto e : c->eventPool) (void)hipEventDestroy(e);
    if (c->ownStream) (void)hipStreamDestroy(c->stream);
    delete c;                                    // (and with it every buffer the context holds, and the turn buffers' events)
}
extern "C" int zsmi_sync(zsmi_ctx *c)
{
    if (!c) return ZSMI_error_init_missing;
    return c->wait();
}
// ---- sticky compression parameters (ZSTD_CCtx_setParameter): read on the host when a compress call is made, they govern what is queued after ----
extern "C" int zsmi_setParameter(zsmi_ctx *c, int param, int value)
{
    if (!c) return ZSMI_error_init_missing;
    if (param != ZSMI_c_checksumFlag) return ZSMI_error_parameter_unsupported;
    if (value != 0 && value != 1) return ZSMI_error_parameter_outOfBound;
    c->checksumFlag = value;
    return 0;
}
extern "C" int zsmi_getParameter(const zsmi_ctx *c, int param, int *value)
{
    if (!c) return ZSMI_error_init_missing;
    if (param != ZSMI_c_checksumFlag) return ZSMI_error_parameter_unsupported;
    if (!value) return ZSMI_error_GENERIC;
    *value = c->checksumFlag;
    return 0;
}
extern "C" int zsmi_enableKernelTiming(zsmi_ctx *c, int on)
{
    if (!c) return ZSMI_error_init_missing;
    c->timing = (on == 2) ? 2 : (on != 0);
    for (auto &tl : c->launches) { c->eventPool.push_back(tl.a); c->eventPool.push_back(tl.b); }
    c->launches.clear();
    return 0;
}
extern "C" int zsmi_getKernelTimes(zsmi_ctx *c, zsmi_kernel_time *out, int maxEntries)
{
    if (!c) return 0;
    (void)hipStreamSynchronize(c->stream);
    int n = 0;
    for (auto &tl : c->launches) {
        float ms = 0; (void)hipEventElapsedTime(&ms, tl.a, tl.b);
        int k = 0;
        for (; k < n; k++) if (!strcmp(out[k].name, tl.name)) break;
        if (k == n) { if (n >= maxEntries) continue; memset(&out[n], 0, sizeof out[n]); strncpy(out[n].name, tl.name, sizeof(out[n].name) - 1); n++; }
        out[k].seconds += ms * 1e-3; out[k].launches++;
        c->eventPool.push_back(tl.a); c->eventPool.push_back(tl.b);
    }
    c->launches.clear();
    return n;
}

// ---------------------------------------------------------------------------------------------
// dictionaries: what a usingDict DECODE of the frames will load (ZSTD_decompress_insertDictionary :2452-2475).
// A formatted dictionary (magic 0xEC30A437, >= 8 bytes) gives the frames its ID and their first blocks its recent offsets; any other
// bytes are raw content: offsets {1, 4, 8}, no ID.  The host parses nothing: the one reader of a dictionary's bytes is the device's
// (loadDictEntropy in decode_kernels.hip, the general decoder's own, which refuses exactly what LoadEntropy :2378-2450 refuses), and
// k_dict_load (decode_fast.hip) runs it for the host, so the compressor and the decoder cannot disagree about a dictionary.  The _usingDict
// calls use none of the dictionary's tables; a digested dictionary takes them from the same run - zsmi_createCDict the entropy section as
// read (ZsCDictEntropy, in the record), zsmi_createDDict the fast kernels' image (img).
// ---------------------------------------------------------------------------------------------
// dDict[0 .. dictSize): device memory.  One launch on the context's stream, the record (a few hundred bytes) copied back, ONE wait.
// 0 with `out` filled (dBytes = dDict), or ZSMI_error_dictionary_corrupted; the record stays in c->dDictRec until the context's next load.
static int loadDict(zsmi_ctx *c, const void *dDict, size_t dictSize, ZsCompressDict &out, ZsDDictImage *img = nullptr)
{
    if (!c->dDictRec.reserve(sizeof(ZsDictRecord)) || !c->hDictRec.reserve(sizeof(ZsDictRecord))) return ZSMI_error_memory_allocation;
    LAUNCH(c, "k_dict_load", k_dict_load, dim3(1), dim3(64), 0, (const uint8_t *)dDict, (uint32_t)dictSize, (ZsDictRecord *)c->dDictRec.p, img);
    if (c->toHost(c->hDictRec.p, c->dDictRec.p, sizeof(ZsDictRecord)) || c->wait()) return ZSMI_error_GENERIC;
    const ZsDictRecord &r = *(const ZsDictRecord *)c->hDictRec.p;
    if (r.status) return (int)r.status;
    out = ZsCompressDict();
    out.dBytes = (const uint8_t *)dDict; out.contentOff = r.contentOff; out.contentSize = (uint32_t)dictSize - r.contentOff; out.dictID = r.dictID;
    for (int i = 0; i < 3; i++) out.rep[i] = r.rep[i];
    return 0;
}

// ---------------------------------------------------------------------------------------------
// compress
// ---------------------------------------------------------------------------------------------
// the scratch of a sub-batch of cap blocks: every buffer of ZS_SCRATCH_TABLE (zsmi_scratch.h) at cap slots and its fixed tail
bool zsmi_ctx::Scratch::reserve(uint32_t cap)
{
    for (int i = 0; i < kZsScratchCount; i++)
        if (!buf[i].reserve((size_t)cap * kZsScratchRows[i].slotBytes + kZsScratchRows[i].tailBytes)) return false;
    return true;
}
// The plan of a call: chunks -> blocks (ZsChunkDesc, ZsBlockDesc) and LZ units, built on the host and copied to the device.  It is reused
// while the chunk layout repeats (steady-state batches; compared in place: such a call allocates and copies nothing).  A dictionary call
// adds a unit list of its own, kept while the layout and the chunks' choice of dictionary repeat.
int CompressPlan::build(zsmi_ctx *c, const uint64_t *srcOffsets, const uint32_t *srcSizes, uint32_t n, const uint64_t *dstOffsets, bool dict,
                        const uint32_t *dictIndex, const uint8_t *memberHasDict)
{
    bool same = key.size() == (size_t)n * 3 + 1 && key[0] == n;
    for (uint32_t i = 0; same && i < n; i++) same = key[1 + i] == srcOffsets[i] && key[1 + n + i] == dstOffsets[i] && key[1 + 2 * (size_t)n + i] == srcSizes[i];
    if (!same) {
        std::vector<uint64_t> newKey((size_t)n * 3 + 1);
        newKey[0] = n;
        for (uint32_t i = 0; i < n; i++) { newKey[1 + i] = srcOffsets[i]; newKey[1 + n + i] = dstOffsets[i]; newKey[1 + 2 * (size_t)n + i] = srcSizes[i]; }
        uint64_t nBlocks = 0;
        for (uint32_t i = 0; i < n; i++) nBlocks += zs_chunk_counts(srcSizes[i]).blocks;
        if (nBlocks > 0x7FFFFFFFull) return ZSMI_error_srcSize_wrong;
        if (!dChunks.reserve(sizeof(ZsChunkDesc) * n) || !dBlocks.reserve(sizeof(ZsBlockDesc) * nBlocks) || !dUnits.reserve(sizeof(ZsUnitDesc) * nBlocks)) return ZSMI_error_memory_allocation;
        if (const int e = c->idleReserve({ { &hChunks, sizeof(ZsChunkDesc) * n }, { &hBlocks, sizeof(ZsBlockDesc) * nBlocks }, { &hUnits, sizeof(ZsUnitDesc) * nBlocks } })) return e;      // (they may still feed the previous layout's copies)
        // a chunk's blocks and units: the rule of zsmi_plan.h, which the resident call's plan kernels apply too
        ZsChunkDesc *hc0 = (ZsChunkDesc *)hChunks.p; ZsBlockDesc *hb = (ZsBlockDesc *)hBlocks.p;
        uint32_t b = 0, maxNb = 1;
        small.before.assign((size_t)n + 1, 0); big.before.assign((size_t)n + 1, 0);
        uint32_t nSmall = 0, nBig = 0;
        for (uint32_t i = 0; i < n; i++) {
            const ZsChunkCounts cc = zs_chunk_counts(srcSizes[i]);
            const uint32_t nb = cc.blocks;
            hc0[i].srcOff = srcOffsets[i]; hc0[i].dstOff = dstOffsets[i]; hc0[i].size = srcSizes[i]; hc0[i].firstBlock = b; hc0[i].nBlocks = nb; hc0[i].pad = 0;
            for (uint32_t k = 0; k < nb; k++, b++) {
                const ZsChunkBlock cb = zs_chunk_block(srcSizes[i], k, nb);
                hb[b].srcOff = srcOffsets[i] + cb.off; hb[b].size = cb.size;
                hb[b].chunk = i; hb[b].firstInChunk = cb.first; hb[b].lastInChunk = cb.last;
            }
            if (nb > maxNb) maxNb = nb;
            small.before[i] = nSmall; big.before[i] = nBig;
            nSmall += cc.smallUnits; nBig += cc.bigUnits;
        }
        small.before[n] = nSmall; big.before[n] = nBig;
        // the units in two runs, [small][big], each in chunk order
        ZsUnitDesc *hu = (ZsUnitDesc *)hUnits.p;
        for (uint32_t i = 0; i < n; i++) {
            const ZsChunkCounts cc = zs_chunk_counts(srcSizes[i]);
            for (uint32_t k = 0; k < cc.smallUnits + cc.bigUnits; k++) {
                const ZsChunkUnit cu = zs_chunk_unit(srcSizes[i], k);
                ZsUnitDesc &u = hu[cu.big ? nSmall + big.before[i] + cu.at : small.before[i] + cu.at];
                u.srcOff = srcOffsets[i] + cu.off; u.size = cu.size; u.firstBlock = hc0[i].firstBlock + cu.block;
            }
        }
        if (nSmall + nBig) if (const int e = c->toDevice(dUnits.p, hu, sizeof(ZsUnitDesc) * (nSmall + nBig))) return e;
        small.base = 0; big.base = nSmall;
        if (const int e = c->toDevice(dChunks.p, hc0, sizeof(ZsChunkDesc) * n)) return e;
        if (const int e = c->toDevice(dBlocks.p, hb, sizeof(ZsBlockDesc) * nBlocks)) return e;
        key.swap(newKey); blocks = nBlocks; maxChunkBlocks = maxNb;
        dictKind = kDictNone;
    }
    // dictionary calls: the small units again, in a list of their own - [chunks of <= 64 KiB that have a dictionary, one unit each
    // (prefixed)][the other small units: tails of longer chunks, chunks without a dictionary]
    if (!dict) return 0;
    const int kind = dictIndex ? kDictPerChunk : kDictAll;
    // the record chunk i uses (ZS_DICT_NONE: no dictionary; an empty member is none)
    auto choice = [&](uint32_t i) -> uint32_t {
        if (!dictIndex) return 0u;
        const uint32_t e = dictIndex[i];
        return (e == ZS_DICT_NONE || (memberHasDict && !memberHasDict[e])) ? ZS_DICT_NONE : e;
    };
    bool have = dictKind == kind && (kind == kDictAll || dictKey.size() == (size_t)n);
    if (kind == kDictPerChunk) for (uint32_t i = 0; have && i < n; i++) have = dictKey[i] == choice(i);
    if (have) return 0;
    dictKind = kDictNone;
    whole.before.assign((size_t)n + 1, 0); tail.before.assign((size_t)n + 1, 0);
    if (kind == kDictPerChunk) dictKey.resize(n); else dictKey.clear();
    uint32_t nWhole = 0, nTail = 0;
    for (uint32_t i = 0; i < n; i++) {
        whole.before[i] = nWhole; tail.before[i] = nTail;
        const uint32_t e = choice(i);
        if (kind == kDictPerChunk) dictKey[i] = e;
        const ZsChunkDictCounts dc = zs_chunk_counts_dict(srcSizes[i], e != ZS_DICT_NONE);      // the dictionary rule of zsmi_plan.h, the plan kernels' too
        nWhole += dc.pfxUnits; nTail += dc.tailUnits;                        // (a chunk has at most one small unit: itself, or its last unit when that is one block)
    }
    whole.before[n] = nWhole; tail.before[n] = nTail;
    const size_t unitBytes = sizeof(ZsUnitDesc) * ((size_t)nWhole + nTail);
    const size_t bytes = unitBytes + (kind == kDictPerChunk ? sizeof(uint32_t) * ((size_t)n + nWhole) : 0);
    ZsUnitDesc *hu;
    if (const int e = hDictList.take(bytes + 16, hu)) return e;
    if (!dDictList.reserve(bytes + 16)) return ZSMI_error_memory_allocation;
    uint32_t *hChunkDict = (uint32_t *)((uint8_t *)hu + unitBytes), *hUnitDict = hChunkDict + n;
    const ZsUnitDesc *all = (const ZsUnitDesc *)hUnits.p;
    uint32_t iw = 0, it = nWhole;
    for (uint32_t i = 0; i < n; i++) {                                       // the small units are in chunk order
        const uint32_t e = choice(i);
        const bool prefixed = zs_chunk_prefixed(srcSizes[i], e != ZS_DICT_NONE);
        if (kind == kDictPerChunk) { hChunkDict[i] = e; if (prefixed) hUnitDict[iw] = e; }
        for (uint32_t k = small.before[i]; k < small.before[i + 1]; k++) hu[prefixed ? iw++ : it++] = all[k];
    }
    if (bytes) {
        if (const int e = c->toDevice(dDictList.p, hu, bytes)) return e;
        if (const int e = hDictList.sent(c->stream)) return e;
    }
    whole.base = 0; tail.base = nWhole; chunkDictOff = unitBytes; unitDictOff = unitBytes + sizeof(uint32_t) * (size_t)n;
    dictKind = kind;
    return 0;
}
CompressPlan::Cut CompressPlan::cut(uint32_t chunk0, uint32_t cap) const
{
    const ZsChunkDesc *hc = (const ZsChunkDesc *)hChunks.p;
    Cut s = { chunk0, 0, hc[chunk0].firstBlock };
    for (; s.chunk1 < key[0] && (s.nb == 0 || s.nb + hc[s.chunk1].nBlocks <= cap); s.chunk1++) s.nb += hc[s.chunk1].nBlocks;
    return s;
}
// the sub-batch's LZ units of a kernel shape: prefixed (dictionary calls only), small (a dictionary call: the tails in its own list), big
CompressPlan::Units CompressPlan::units(int kind, bool dict, uint32_t chunk0, uint32_t chunk1) const
{
    if (kind == kUnitsPfx && !dict) return { nullptr, 0 };
    const bool ownList = dict && kind != kUnitsBig;
    const Run &r = kind == kUnitsBig ? big : (!dict ? small : (kind == kUnitsPfx ? whole : tail));
    return { (const ZsUnitDesc *)(ownList ? dDictList : dUnits).p + r.base + r.before[chunk0], r.before[chunk1] - r.before[chunk0] };
}

// a dictionary's record as the kernels read it, its images at dImg.  The prefix: the content's last <= 64 KiB, where a prefixed unit's
// matches may reach
static ZsCDictEntry dictEntry(const ZsCompressDict &d, const uint32_t *dImg)
{
    ZsCDictEntry e;
    e.pfx = std::min<uint32_t>(d.contentSize, ZS_BLOCK_MAX); e.pre = d.dBytes + d.contentOff + d.contentSize - e.pfx;
    e.img = dImg; e.tables = d.dTables; e.dictID = d.dictID; e.hasDict = 1;
    for (int i = 0; i < 3; i++) e.rep[i] = d.rep[i];
    return e;
}
// the prefix's candidate-table images for a level's LZ shape (the short table's and the long table's), into dImg, and the dictionary's
// record into dEntry: its one-entry table
static const size_t kDictImgBytes = (size_t)2 << (ZS_TABLE_LOG_BIG + 2);
static void launchDictTables(zsmi_ctx *c, const ZsCompressDict &d, int level, void *dImg, void *dEntry)
{
    LAUNCH(c, "k_lz_dict_tables", k_lz_dict_tables, dim3(lzShape(level).useLong ? 2 : 1), dim3(1024), 0, dictEntry(d, (const uint32_t *)dImg), (ZsCDictEntry *)dEntry);
}
// a dictionary in host memory -> the context's staging buffer; dict: then its device copy
static int stageDict(zsmi_ctx *c, const void *&dict, size_t dictSize)
{
    if (!c->sDict.reserve(dictSize + 64)) return ZSMI_error_memory_allocation;
    if (const int e = c->toDevice(c->sDict.p, dict, dictSize)) return e;
    dict = c->sDict.p; return 0;
}
static int dictFromBytes(zsmi_ctx *c, const void *dict, size_t dictSize, DictBytes kind, int level, uint32_t n, ZsCDictSel &sel)
{
    if (!dict || dictSize == 0) return 0;
    if (!c) return ZSMI_error_init_missing;
    if (dictSize > 0xFFFFFFFFull) return ZSMI_error_dictionary_corrupted;
    if (const int e = c->bind()) return e;
    if (kind == kDictOnHost) if (const int e = stageDict(c, dict, dictSize)) return e;
    ZsCompressDict d;
    d.dBytes = (const uint8_t *)dict; d.contentSize = (uint32_t)dictSize;
    if (kind != kDictContent) if (const int e = loadDict(c, dict, dictSize, d)) return e;
    if (n == 0) return 0;                                            // (an empty call gives the dictionary its verdict and builds nothing)
    if (!c->dDictImg.reserve(kDictImgBytes + sizeof(ZsCDictEntry))) return ZSMI_error_memory_allocation;
    sel.dTable = (const ZsCDictEntry *)((const uint8_t *)c->dDictImg.p + kDictImgBytes);
    launchDictTables(c, d, level, c->dDictImg.p, const_cast<ZsCDictEntry *>(sel.dTable));
    return 0;
}
// One sub-batch of a compress call as its kernels take it, whoever planned it - the host (CompressPlan) or the device (plan_kernels.hip).
//   dChunks: the call's chunk list; dBlocks: the block list a chunk's firstBlock counts in; block0: the sub-batch's first block there
//   (scratch slot = block - block0); nb, units[k].n: its blocks and units - or, with `live`, the host's upper bounds of them: the grids
//   live: null, or the device's counts of what the lists really hold (a ZsPlanCounts: blocks, small units, big units, prefixed units); the kernels whose
//   index is a block or a unit leave at or beyond their count.  k_assemble_frames is indexed by chunks, which the host knows
struct SubBatch {
    const ZsChunkDesc *dChunks; const ZsBlockDesc *dBlocks;
    uint32_t chunk0, nChunks, block0, nb, cap;
    CompressPlan::Units units[3]; const uint32_t *dUnitDict = nullptr;
    const uint32_t *live = nullptr;
    bool assemble;                                   // chunks of several blocks may be among them
    const ZsCDictEntry *dTable = nullptr; const uint32_t *dChunkDict = nullptr;      // the dictionary records (null: none) and the record index a chunk (null: record 0)
    bool cdt = false;                                // some record has entropy tables: the CD forms of the entropy kernels
};
static void launchSubBatch(zsmi_ctx *c, const LzShape &shape, const SubBatch &sb, const void *dSrc, void *dDst, uint32_t *dDstSizes, uint32_t *dStats)
{
    zsmi_ctx::Scratch &S = c->scratch;
    const uint32_t nb = sb.nb, block0 = sb.block0;
    const ZsBlockDesc *dB = sb.dBlocks + block0;
    const CompressPlan::Units *units = sb.units;
    const uint32_t *liveBlocks = sb.live, *liveUnits[3] = { sb.live ? sb.live + 3 : nullptr, sb.live ? sb.live + 1 : nullptr, sb.live ? sb.live + 2 : nullptr };
    for (int k = 0; k < 3; k++) {
        const LzKernel<CandFn> &K = shape.cand[k];
        const bool p = k == kUnitsPfx;
        if (units[k].n)
            LAUNCH(c, K.name, K.fn, dim3(units[k].n), dim3(K.threads), K.lds, (const uint8_t *)dSrc, units[k].d, block0, S.dist(),
                   S.distHi(), S.cand(), p ? sb.dTable : nullptr, p ? sb.dUnitDict : nullptr, liveUnits[k]);
    }
    for (int k = 0; k < 3; k++) {
        const LzKernel<WalkFn> &K = shape.walk[k];
        const bool p = k == kUnitsPfx;
        if (units[k].n)
            LAUNCH(c, K.name, K.fn, dim3(units[k].n), dim3(K.threads), K.lds, (const uint8_t *)dSrc, units[k].d, block0, S.dist(),
                   S.distHi(), S.recs(), zs_walk_records_end(sb.cap), S.res(), shape.walkLog, S.cand(),
                   p ? sb.dTable : nullptr, p ? sb.dUnitDict : nullptr, liveUnits[k]);
    }
    LAUNCH(c, "k_lz_stitch", k_lz_stitch, dim3(nb), dim3(256), 0, dB, S.recs(), S.res(), S.seqs(), S.hdrs(), shape.walkLog, liveBlocks);
    if (c->stopAfterWalk) return;
    // The entropy stage.  Sequences first: the literals kernel assembles the frames of one-block chunks as its workgroups finish, and
    // reads the sequence sections then.  (The two side by side on two streams was measured slower: both want the whole LDS.)  Every
    // kernel takes a frame's recent offsets and ID from its chunk's record ({1, 4, 8} and 0 without one); in the CD forms the record's
    // entropy tables may code the frame's first block besides.
    const auto seqKernel = sb.cdt ? k_encode_sequences<ZS_SEQ_GROUP, true> : k_encode_sequences<ZS_SEQ_GROUP, false>;
    const auto litKernel = sb.cdt ? k_encode_literals<true> : k_encode_literals<false>;
    LAUNCH(c, "k_encode_sequences", seqKernel, dim3((nb + ZS_SEQ_GROUP - 1) / ZS_SEQ_GROUP), dim3(64 * ZS_SEQ_GROUP), 0, dB, nb, S.seqs(),
           S.hdrs(), S.seqSec(), S.metas(), c->stopSeq, S.lits(), S.streams(),
           S.distAsPackRecords(), sb.dTable, sb.dChunkDict, liveBlocks);
    if (dStats)                                                  // (the codes it reads are in the literal buffers until the literals kernel)
        LAUNCH(c, "k_train_stats", k_train_stats, dim3(nb), dim3(256), 0, (const uint8_t *)dSrc, dB, S.seqs(),
               S.hdrs(), S.lits(), dStats);
    LAUNCH(c, "k_encode_literals", litKernel, dim3(nb), dim3(256), 0, (const uint8_t *)dSrc, dB, S.seqs(), S.hdrs(),
           S.lits(), S.streams(), S.litSec(), S.metas(), c->stopLit,
           sb.dChunks, S.seqSec(), (uint8_t *)dDst, dDstSizes, sb.dTable, sb.dChunkDict, liveBlocks);
    if (sb.assemble)                                             // chunks of several blocks
        LAUNCH(c, "k_assemble_frames", k_assemble_frames, dim3(sb.nChunks), dim3(256), 0, (const uint8_t *)dSrc, sb.dChunks,
               sb.dBlocks, S.metas(), S.litSec(), S.seqSec(), block0,
               (uint8_t *)dDst, dDstSizes, sb.chunk0, sb.dTable, sb.dChunkDict);
}
// What both planners share.  The blocks of a sub-batch (its scratch slots): the blocks in flight - never below 64, never more than the call
// has - and at least the largest chunk's, which goes whole
static uint32_t subBatchCap(const zsmi_ctx *c, uint64_t blocks, uint32_t maxChunkBlocks)
{
    const uint64_t inFlight = std::min<uint64_t>(blocks, std::max<uint32_t>(64, c->maxBlocksInFlight));
    return std::max<uint32_t>((uint32_t)inFlight, maxChunkBlocks);
}
// behind the last sub-batch, when every frame and size is final on the stream: with checksum, ONE k_frame_checksum launch over all n chunks; without it, none
static void closeFrames(zsmi_ctx *c, const void *dSrc, const ZsChunkDesc *dChunks, uint32_t n, void *dDst, uint32_t *dDstSizes, int checksum)
{
    if (checksum && !c->stopAfterWalk && !c->stopLit && !c->stopSeq)     // (a stopped stage leaves no frames to close)
        LAUNCH(c, "k_frame_checksum", k_frame_checksum, dim3((n + 15) / 16), dim3(64), 0, (const uint8_t *)dSrc, dChunks, n, (uint8_t *)dDst, dDstSizes);
}
// The launch sequence of a call, over the plan's sub-batches.  dict: the call's selector (ZsCDictSel, zsmi_ctx.h) - nullptr or without a
// table: the plain call, which is a dictionary call with no prefixed units.  A chunk with a dictionary carries its record's ID and its
// first block starts from the record's recent offsets; one of <= 64 KiB is a PREFIXED unit (k_lz_candidates / k_lz_walk with PFX: matches
// may reach into the record's prefix, through the table images that came with the record), the units of longer chunks are parsed as
// without a dictionary; and a record's entropy tables (a digested, formatted dictionary's) may code the first block.  The kernels take the
// table and an index a chunk; a single dictionary is the one-entry table with no index.  dStats (the dictionary trainer's finalize; nullptr on every
// other path): device counters of the literal bytes and LL / OF / ML codes, added to by k_train_stats after each sub-batch's sequences kernel.
static int compressBatchDeviceImpl(zsmi_ctx *c, const void *dSrc, const uint64_t *srcOffsets, const uint32_t *srcSizes,
                                   uint32_t n, void *dDst, const uint64_t *dstOffsets, uint32_t *dDstSizes, int level,
                                   const ZsCDictSel *dict, int checksum, uint32_t *dStats)
{
    if (!c) return ZSMI_error_init_missing;
    if (n == 0) return 0;
    if (const int e = c->bind()) return e;
    const LzShape &shape = lzShape(level);
    CompressPlan &P = c->plan;
    const ZsCDictSel sel = dict && dict->dTable ? *dict : ZsCDictSel();
    const bool useDict = sel.dTable != nullptr;
    if (const int e = P.build(c, srcOffsets, srcSizes, n, dstOffsets, useDict, sel.dictIndex, sel.memberHasDict)) return e;
    // sub-batches of whole chunks, one after the other through one scratch set.  Every kernel goes to the caller's stream: a stream of
    // the context's own costs two queue crossings a call (~0.01 - 0.09 ms each: a bench line of 126 GiB/s where the kernels added up to 137).
    const uint32_t cap = subBatchCap(c, P.blocks, P.maxChunkBlocks);
    zsmi_ctx::Scratch &S = c->scratch;
    if (!S.reserve(cap)) return ZSMI_error_memory_allocation;
    SubBatch sb;
    sb.dChunks = (const ZsChunkDesc *)P.dChunks.p; sb.dBlocks = (const ZsBlockDesc *)P.dBlocks.p; sb.cap = cap; sb.assemble = P.maxChunkBlocks > 1;
    sb.dTable = sel.dTable; sb.dChunkDict = sel.dictIndex ? P.chunkDict() : nullptr; sb.cdt = sel.tables;
    for (uint32_t chunk0 = 0, chunk1; chunk0 < n; chunk0 = chunk1) {
        const CompressPlan::Cut sub = P.cut(chunk0, cap);
        chunk1 = sub.chunk1;
        sb.chunk0 = chunk0; sb.nChunks = chunk1 - chunk0; sb.block0 = sub.block0; sb.nb = sub.nb;
        for (int k = 0; k < 3; k++) sb.units[k] = P.units(k, useDict, chunk0, chunk1);
        sb.dUnitDict = P.unitDict(chunk0);
        launchSubBatch(c, shape, sb, dSrc, dDst, dDstSizes, dStats);
    }
    closeFrames(c, dSrc, sb.dChunks, n, dDst, dDstSizes, checksum);
    return c->launched();
}
extern "C" int zsmi_compressBatchDevice(zsmi_ctx *c, const void *dSrc, const uint64_t *srcOffsets, const uint32_t *srcSizes,
                                        uint32_t n, void *dDst, const uint64_t *dstOffsets, uint32_t *dDstSizes, int level)
{
    return compressBatchDeviceImpl(c, dSrc, srcOffsets, srcSizes, n, dDst, dstOffsets, dDstSizes, level, nullptr, c ? c->checksumFlag : 0);
}

// ---- device-resident compress: the call above with its three descriptor arrays in device memory.  The plan is built by kernels
// (plan_kernels.hip) into buffers of its own (zsmi_ctx::ResidentPlan): the host-array calls' plan, its key, pinned buffers and events are
// not touched, nothing is copied to the host, nothing waited for.  The host knows maxSrcSize alone:
//   nbMax = blocks of a chunk of maxSrcSize; cap = the blocks in flight, as above, with n * nbMax for the call's blocks;
//   sub-batches are fixed runs of K = cap / nbMax chunks - never more than cap blocks, whatever the sizes are;
//   grids are upper bounds (K * nbMax blocks, K small units, K * ceil(nbMax / 2) big units: none when nbMax is 1), the live counts reach
//   the kernels through SubBatch::live.  With every chunk maxSrcSize long the bounds are the counts: no workgroup is launched in vain.
//   The set form (zsmi_compressBatchResident_usingCDictSet, behind the CDict sets below) takes the chunks' choice of dictionary from device
//   memory too: the same body with a prefixed unit list of K slots in front. ----
extern "C" int zsmi_compressBoundsDevice(zsmi_ctx *c, const uint32_t *dSrcSizes, uint32_t n, uint64_t *dBounds)
{
    if (!c) return ZSMI_error_init_missing;
    if (n && (!dSrcSizes || !dBounds)) return ZSMI_error_GENERIC;
    if (n == 0) return 0;
    if (const int e = c->bind()) return e;
    LAUNCH(c, "k_compress_bounds", k_compress_bounds, dim3((n + 255) / 256), dim3(256), 0, dSrcSizes, n, dBounds);
    return c->launched();
}
// What the two resident compress calls check first, in this order, before anything is queued
static int residentCompressArgs(const zsmi_ctx *c, const void *dSrc, const uint64_t *dSrcOffsets, const uint32_t *dSrcSizes, uint32_t n,
                                const void *dDst, const uint64_t *dDstOffsets, const uint32_t *dDstSizes)
{
    if (!c) return ZSMI_error_init_missing;
    return n && (!dSrc || !dSrcOffsets || !dSrcSizes || !dDst || !dDstOffsets || !dDstSizes) ? ZSMI_error_GENERIC : 0;
}
// The body of both (the arguments checked).  dict: null for the plain call; a set call's records and its choice in DEVICE memory - the
// host knows neither which chunks pick a dictionary nor whether any does, so there is no "no chunk has one: plain call" shortcut: the unit
// slots are [prefixed: K][small: K][big: K * bigMax], the prefixed-unit kernels go over their upper bound (a unit a chunk) and leave on a
// live count that may be 0.  Everything a sub-batch's kernels take about dictionaries is device memory the plan kernels wrote.
// (ResidentDict: zsmi_ctx.h - the resident record archives of seekable.hip run this body too)
static int compressBatchResidentImpl(zsmi_ctx *c, const void *dSrc, const uint64_t *dSrcOffsets, const uint32_t *dSrcSizes, uint32_t n,
                                     uint32_t maxSrcSize, void *dDst, const uint64_t *dDstOffsets, uint32_t *dDstSizes, int level, const ResidentDict *dict)
{
    if (n == 0) return 0;
    if (const int e = c->bind()) return e;
    const LzShape &shape = lzShape(level);
    const uint32_t nbMax = zs_chunk_counts(maxSrcSize).blocks, bigMax = (nbMax + 1) / 2;
    const uint32_t cap = subBatchCap(c, (uint64_t)n * nbMax, nbMax);
    const uint32_t K = std::min(n, cap / nbMax), subs = (n + K - 1) / K;
    zsmi_ctx::Scratch &S = c->scratch;
    if (!S.reserve(cap)) return ZSMI_error_memory_allocation;
    zsmi_ctx::ResidentPlan &R = c->resident;
    const uint32_t pfxSlots = dict ? K : 0u;
    const size_t nUnitSlots = (size_t)pfxSlots + K + (nbMax > 1 ? (size_t)K * bigMax : 0);
    if (!R.dChunks.reserve(sizeof(ZsChunkDesc) * n) || !R.dBefore.reserve(sizeof(ZsPlanBefore) * n) || !R.dCounts.reserve(sizeof(ZsPlanCounts) * subs) ||
        !R.dBlocks.reserve(sizeof(ZsBlockDesc) * (size_t)K * nbMax) || !R.dUnits.reserve(sizeof(ZsUnitDesc) * nUnitSlots)) return ZSMI_error_memory_allocation;
    if (dict && (!R.dChunkDict.reserve(sizeof(uint32_t) * n) || !R.dUnitDict.reserve(sizeof(uint32_t) * K))) return ZSMI_error_memory_allocation;
    ZsChunkDesc *dChunks = (ZsChunkDesc *)R.dChunks.p;
    const ZsPlanBefore *dBefore = (const ZsPlanBefore *)R.dBefore.p;
    const ZsPlanCounts *dCounts = (const ZsPlanCounts *)R.dCounts.p;
    uint32_t *dChunkDict = dict ? (uint32_t *)R.dChunkDict.p : nullptr;
    ZsPlanLists lists = { (ZsBlockDesc *)R.dBlocks.p, (ZsUnitDesc *)R.dUnits.p, 0u, pfxSlots, pfxSlots + K, dict ? (uint32_t *)R.dUnitDict.p : nullptr };
    if (dict)
        LAUNCH(c, "k_plan_chunks", k_plan_chunks<true>, dim3(subs), dim3(ZS_PLAN_THREADS), 0, dSrcOffsets, dSrcSizes, dDstOffsets, n, K, maxSrcSize,
               dChunks, (ZsPlanBefore *)R.dBefore.p, (ZsPlanCounts *)R.dCounts.p, dict->dDictIndex, dict->dTable, dict->members, dChunkDict);
    else
        LAUNCH(c, "k_plan_chunks", k_plan_chunks<false>, dim3(subs), dim3(ZS_PLAN_THREADS), 0, dSrcOffsets, dSrcSizes, dDstOffsets, n, K, maxSrcSize,
               dChunks, (ZsPlanBefore *)R.dBefore.p, (ZsPlanCounts *)R.dCounts.p, (const uint32_t *)nullptr, (const ZsCDictEntry *)nullptr, 0u, (uint32_t *)nullptr);
    SubBatch sb;
    sb.dChunks = dChunks; sb.dBlocks = lists.blocks; sb.block0 = 0; sb.cap = cap; sb.assemble = nbMax > 1;
    if (dict) { sb.dTable = dict->dTable; sb.dChunkDict = dChunkDict; sb.dUnitDict = lists.unitDict; sb.cdt = dict->tables; }
    for (uint32_t s = 0; s < subs; s++) {
        const uint32_t chunk0 = s * K, nChunks = std::min(K, n - chunk0);
        // the lists are the sub-batch's alone: every sub-batch writes them again, behind the kernels that read the one before's
        LAUNCH(c, "k_plan_blocks", k_plan_blocks, dim3((nChunks * nbMax + 255) / 256), dim3(256), 0, (const ZsChunkDesc *)dChunks + chunk0, dBefore + chunk0,
               dCounts + s, nChunks, chunk0, lists, dict ? (const uint32_t *)dChunkDict + chunk0 : nullptr);
        sb.chunk0 = chunk0; sb.nChunks = nChunks; sb.nb = nChunks * nbMax; sb.live = &dCounts[s].blocks;
        sb.units[kUnitsPfx] = { dict ? lists.units + lists.pfxBase : nullptr, dict ? nChunks : 0u };
        sb.units[kUnitsSmall] = { lists.units + lists.smallBase, nChunks };
        sb.units[kUnitsBig] = { lists.units + lists.bigBase, nbMax > 1 ? nChunks * bigMax : 0u };
        launchSubBatch(c, shape, sb, dSrc, dDst, dDstSizes, nullptr);
    }
    closeFrames(c, dSrc, dChunks, n, dDst, dDstSizes, c->checksumFlag);
    // last: a chunk above maxSrcSize, or one whose index names no member, was planned as an empty one, and its size word says so only now
    LAUNCH(c, "k_plan_refuse", k_plan_refuse, dim3((n + 255) / 256), dim3(256), 0, dSrcSizes, n, maxSrcSize, zs_error_word(ZSMI_error_srcSize_wrong), dDstSizes,
           dict ? dict->dDictIndex : nullptr, dict ? dict->members : 0u, zs_error_word(ZSMI_error_parameter_outOfBound));
    return c->launched();
}
extern "C" int zsmi_compressBatchResident(zsmi_ctx *c, const void *dSrc, const uint64_t *dSrcOffsets, const uint32_t *dSrcSizes, uint32_t n,
                                          uint32_t maxSrcSize, void *dDst, const uint64_t *dDstOffsets, uint32_t *dDstSizes, int level)
{
    if (const int e = residentCompressArgs(c, dSrc, dSrcOffsets, dSrcSizes, n, dDst, dDstOffsets, dDstSizes)) return e;
    return compressBatchResidentImpl(c, dSrc, dSrcOffsets, dSrcSizes, n, maxSrcSize, dDst, dDstOffsets, dDstSizes, level, nullptr);
}
// dDict: device memory.  The dictionary loader runs over it and its record (a formatted dictionary's ID, recent offsets and content
// offset, or the refusal) is read back: the call waits for the context's stream once.  (Its tables are queued before the plan: a new layout's wait in build covers them)
extern "C" int zsmi_compressBatchDevice_usingDict(zsmi_ctx *c, const void *dSrc, const uint64_t *srcOffsets, const uint32_t *srcSizes,
                                                  uint32_t n, void *dDst, const uint64_t *dstOffsets, uint32_t *dDstSizes, int level,
                                                  const void *dDict, size_t dictSize)
{
    ZsCDictSel sel;
    if (const int e = dictFromBytes(c, dDict, dictSize, kDictOnDevice, level, n, sel)) return e;
    return compressBatchDeviceImpl(c, dSrc, srcOffsets, srcSizes, n, dDst, dstOffsets, dDstSizes, level, &sel, c ? c->checksumFlag : 0);
}

// ---- digested dictionaries (ZSTD_createCDict / ZSTD_compress_usingCDict): loaded once, everything a call needs kept in device memory - the
// bytes, the prefix's candidate-table images for the bound level's LZ shape, and for a formatted dictionary its entropy tables in encoder
// form (k_cdict_tables, from the loader's record).  Read-only after creation: any context of the same device may use it, from any thread. ----
struct zsmi_cdict {
    int device = 0, level = 3;
    bool empty = false;                  // no bytes: its calls are the plain calls at its level
    ZsCompressDict d;                    // (dBytes, dTables: into the buffers below)
    DevBuf dBytes, dImg, dTables, dEntry;
};
extern "C" zsmi_cdict *zsmi_createCDict(zsmi_ctx *c, const void *dict, size_t dictSize, int level, int *err)
{
    return makeHandle<zsmi_cdict>(err, [&](zsmi_cdict &cd) -> int {
        if (!c) return ZSMI_error_init_missing;
        if (dictSize > 0xFFFFFFFFull) return ZSMI_error_dictionary_corrupted;
        cd.device = c->device; cd.level = level;
        if (!dict || dictSize == 0) { cd.empty = true; return 0; }
        if (const int e = c->bind()) return e;
        if (!cd.dBytes.reserve(dictSize + 64) || !cd.dImg.reserve(kDictImgBytes) || !cd.dEntry.reserve(sizeof(ZsCDictEntry))) return ZSMI_error_memory_allocation;
        if (const int e = c->toDevice(cd.dBytes.p, dict, dictSize)) return e;
        if (const int e = loadDict(c, cd.dBytes.p, dictSize, cd.d)) return e;
        const bool formatted = cd.d.contentOff != 0;
        if (formatted && !cd.dTables.reserve(sizeof(ZsCDictTables))) return ZSMI_error_memory_allocation;
        if (formatted) {
            LAUNCH(c, "k_cdict_tables", k_cdict_tables, dim3(1), dim3(256), 0, &((const ZsDictRecord *)c->dDictRec.p)->ent, (ZsCDictTables *)cd.dTables.p);
            cd.d.dTables = (const ZsCDictTables *)cd.dTables.p;
        }
        launchDictTables(c, cd.d, level, cd.dImg.p, cd.dEntry.p);            // (and the one-entry table its calls pass)
        return c->wait() || c->launched() ? ZSMI_error_GENERIC : 0;
    });
}
extern "C" void zsmi_freeCDict(zsmi_cdict *cd) { delete cd; }
extern "C" unsigned zsmi_getDictID_fromCDict(const zsmi_cdict *cd) { return cd ? cd->d.dictID : 0; }
extern "C" size_t zsmi_sizeofCDict(const zsmi_cdict *cd) { return cd ? cd->dBytes.cap + cd->dImg.cap + cd->dTables.cap + cd->dEntry.cap : 0; }
// What a zsmi_cdict * argument asks of a call on context c - 0, with level and sel set: compress at `level`, plainly (no table: a null cdict at
// level 3, one without bytes at its own) or with the dictionary's one-entry table; or the error (digested on another device: parameter_unsupported)
static int resolveCDict(const zsmi_ctx *c, const zsmi_cdict *cd, int &level, ZsCDictSel &sel)
{
    level = cd ? cd->level : 3; sel = ZsCDictSel();
    if (cd && !cd->empty) { sel.dTable = (const ZsCDictEntry *)cd->dEntry.p; sel.tables = cd->d.dTables != nullptr; }
    if (!cd) return 0;
    if (!c) return ZSMI_error_init_missing;
    return cd->device == c->device ? 0 : ZSMI_error_parameter_unsupported;
}
// queues the work and returns: nothing is read back, nothing waited for (the dictionary call's parse, wait and table build were done at creation)
extern "C" int zsmi_compressBatchDevice_usingCDict(zsmi_ctx *c, const void *dSrc, const uint64_t *srcOffsets, const uint32_t *srcSizes,
                                                   uint32_t n, void *dDst, const uint64_t *dstOffsets, uint32_t *dDstSizes, const zsmi_cdict *cd)
{
    int level; ZsCDictSel sel;
    if (const int e = resolveCDict(c, cd, level, sel)) return e;
    return compressBatchDeviceImpl(c, dSrc, srcOffsets, srcSizes, n, dDst, dstOffsets, dDstSizes, level, &sel, c ? c->checksumFlag : 0);
}

// ---- CDict sets: a read-only device table with one record (ZsCDictEntry) per member, in the caller's order; a call with a set gives chunk i
// the member dictIndex[i] names, on the device, inside the kernels.  The set copies nothing from its members: a record points into its
// member's buffers.  Every check is the host's, before anything touches the device; the one upload is waited for, once. ----
struct zsmi_cdictSet {
    int device = 0, level = 3;
    uint32_t members = 0;
    bool tables = false;                 // some member is formatted: its calls take the CD forms of the entropy kernels
    std::vector<uint8_t> hasDict;        // per member: 0 for an empty CDict (its chunks have no dictionary)
    DevBuf dTable;
};
#define ZSMI_CDICTSET_MAX 4096u
extern "C" zsmi_cdictSet *zsmi_createCDictSet(zsmi_ctx *c, const zsmi_cdict *const *cds, uint32_t n, int level, int *err)
{
    return makeHandle<zsmi_cdictSet>(err, [&](zsmi_cdictSet &set) -> int {
        if (!c) return ZSMI_error_init_missing;
        if (n > ZSMI_CDICTSET_MAX) return ZSMI_error_parameter_outOfBound;
        if (n && !cds) return ZSMI_error_parameter_unsupported;
        std::vector<ZsCDictEntry> table(n);
        set.device = c->device; set.level = level; set.members = n; set.hasDict.resize(n);
        for (uint32_t i = 0; i < n; i++) {
            const zsmi_cdict *cd = cds[i];
            // a member: there, of this device, digested for this level (its images are built for one LZ shape)
            if (!cd || cd->device != c->device || cd->level != level) return ZSMI_error_parameter_unsupported;
            set.hasDict[i] = !cd->empty;
            table[i] = cd->empty ? ZsCDictEntry() : dictEntry(cd->d, (const uint32_t *)cd->dImg.p);
            set.tables |= !cd->empty && cd->d.dTables != nullptr;
        }
        if (n == 0) return 0;
        if (const int e = c->bind()) return e;
        if (!set.dTable.reserve(sizeof(ZsCDictEntry) * n)) return ZSMI_error_memory_allocation;
        return c->toDevice(set.dTable.p, table.data(), sizeof(ZsCDictEntry) * n) || c->wait() ? ZSMI_error_GENERIC : 0;
    });
}
extern "C" void zsmi_freeCDictSet(zsmi_cdictSet *set) { delete set; }
extern "C" uint32_t zsmi_sizeofCDictSetMembers(const zsmi_cdictSet *set) { return set ? set->members : 0; }
// resolveCDict's sibling: what a zsmi_cdictSet * argument and the call's choice ask of a call on context c - 0, with level and sel set
// (without a table for a null set, the plain call at level 3); or the error, before anything is queued or written
static int resolveCDictSet(const zsmi_ctx *c, const zsmi_cdictSet *set, const uint32_t *dictIndex, uint32_t n, int &level, ZsCDictSel &sel, bool nullIsTheOneMember)
{
    level = set ? set->level : 3; sel = ZsCDictSel();
    if (!c) return ZSMI_error_init_missing;
    if (!set) return 0;
    const bool oneMember = !dictIndex && nullIsTheOneMember && set->members == 1;      // (the selector's null dictIndex: every chunk uses record 0)
    if (n && !dictIndex && !oneMember) return ZSMI_error_GENERIC;
    bool any = oneMember && n && set->hasDict[0] != 0;               // (a choice that gives no chunk a dictionary: the plain call)
    for (uint32_t i = 0; dictIndex && i < n; i++) if (dictIndex[i] != ZS_DICT_NONE) {
        if (dictIndex[i] >= set->members) return ZSMI_error_parameter_outOfBound;
        any |= set->hasDict[dictIndex[i]] != 0;
    }
    if (set->device != c->device) return ZSMI_error_parameter_unsupported;
    if (!any) return 0;
    sel.dTable = (const ZsCDictEntry *)set->dTable.p; sel.dictIndex = dictIndex; sel.memberHasDict = set->hasDict.data(); sel.tables = set->tables;
    return 0;
}
// queues the work and returns, as the _usingCDict call: the choice goes up with the plan's dictionary list, through pinned buffers taken in turn
extern "C" int zsmi_compressBatchDevice_usingCDictSet(zsmi_ctx *c, const void *dSrc, const uint64_t *srcOffsets, const uint32_t *srcSizes,
                                                      uint32_t n, void *dDst, const uint64_t *dstOffsets, uint32_t *dDstSizes,
                                                      const zsmi_cdictSet *set, const uint32_t *dictIndex)
{
    int level; ZsCDictSel sel;
    if (const int e = resolveCDictSet(c, set, dictIndex, n, level, sel)) return e;
    return compressBatchDeviceImpl(c, dSrc, srcOffsets, srcSizes, n, dDst, dstOffsets, dDstSizes, level, &sel, c->checksumFlag);
}
// the resident form: the choice is device memory, so what resolveCDictSet judges on the host - an index out of range, a choice that gives
// no chunk a dictionary - is the plan kernels' to find (plan_kernels.hip).  A NULL index: every chunk uses the one member
static int residentCDictSet(const zsmi_ctx *c, const zsmi_cdictSet *set, const uint32_t *dDictIndex, uint32_t n, int &level, ResidentDict &dict)
{
    level = set ? set->level : 3; dict = ResidentDict{ nullptr, 0u, false, nullptr };
    if (!set) return 0;
    if (n && !dDictIndex && set->members != 1) return ZSMI_error_GENERIC;
    if (set->device != c->device) return ZSMI_error_parameter_unsupported;
    dict = ResidentDict{ (const ZsCDictEntry *)set->dTable.p, set->members, set->tables, dDictIndex };
    return 0;
}
extern "C" int zsmi_compressBatchResident_usingCDictSet(zsmi_ctx *c, const void *dSrc, const uint64_t *dSrcOffsets, const uint32_t *dSrcSizes,
                                                        uint32_t n, uint32_t maxSrcSize, void *dDst, const uint64_t *dDstOffsets, uint32_t *dDstSizes,
                                                        const zsmi_cdictSet *set, const uint32_t *dDictIndex)
{
    if (const int e = residentCompressArgs(c, dSrc, dSrcOffsets, dSrcSizes, n, dDst, dDstOffsets, dDstSizes)) return e;
    int level; ResidentDict dict;
    if (const int e = residentCDictSet(c, set, dDictIndex, n, level, dict)) return e;
    return compressBatchResidentImpl(c, dSrc, dSrcOffsets, dSrcSizes, n, maxSrcSize, dDst, dDstOffsets, dDstSizes, level, set ? &dict : nullptr);
}

// ---------------------------------------------------------------------------------------------
// decompress
// ---------------------------------------------------------------------------------------------
// A call runs in sub-batches of `cap` items, one after the other through one scratch set.  The fast path (decode_fast.hip: items that are one
// frame of up to ZS_FAST_MAXBLOCKS blocks) runs k_dec_prep -> entropy stage -> k_dec_execute -> k_dec_checksum -> k_dec_collect; then the general
// kernel (decode_kernels.hip) takes what the fast path left, or every item when it does not run.
//
// Scratch.  The general kernel's wavefronts form a POOL with a literal buffer each (ZS_DEC_LITBUF = 128 KiB + 64; as many as the chip holds at once),
// whatever the call's size.  The fast path keeps per-block scratch in slot = block index * cap + item, sized by the CALL'S LARGEST CAPACITY:
//   literal bytes a slot:  min(capacity, 128 KiB) + 64        (a block regenerates no more than its item may hold)
//   sequences a slot:      min(capacity, 128 KiB) / 3 + 64    (a sequence copies >= 3 bytes), 8 bytes each
//   + Huffman table 4 KiB + sequence tables 2.5 KiB + a descriptor                     -> 32 KiB items: ~125 KiB an item (round 3: 263 KiB whatever the capacity)
// A block that wants more than its slot holds cannot fit its item's capacity: k_dec_prep leaves it to the general kernel, which reports it.
struct DecodePlan {
    bool fast;                                        // the fast path runs: not under ZSMI_DEC_FAST=0, not for a _usingDict call (frames that name a dictionary go to the general
                                                      // kernel; a digested dictionary, zsmi_ddict, brings the image the fast kernels' dictionary forms need)
    uint32_t maxBlocks, descSlots;                    // block slots an item; descriptors an item (>= 2)
    uint32_t blockCap, litStride, litCap, seqCap;     // a slot: the bytes its block may regenerate, its literal stride and bytes, its sequences
    uint32_t pool, cap;                               // wavefronts of the general kernel's pool (whole workgroups); items in flight
};
// Every decode scratch buffer and its bytes for a plan: the one statement of the sizes, which the budget (planDecode), the reservation and
// zsmi_decodeScratchBytes go through.  0: a buffer the plan does not use (the fast path's, on a call without it), left as it is.
template <class F>
void zsmi_ctx::DecodeScratch::each(const DecodePlan &p, F f)
{
    const size_t items = p.fast ? p.cap : 0, slots = items * p.maxBlocks;
    f(dPoolLit, p.pool * ZsDecSlotBytes::poolLit);
    f(dLitScratch, slots * p.litStride);
    f(dFastDesc, items * p.descSlots * sizeof(ZsFastDesc));
    f(dHufTabs, slots * ZsDecSlotBytes::hufTabs);
    f(dSeqTabs, slots * ZsDecSlotBytes::seqTabs);
    f(dSeqOut, slots * p.seqCap * ZsDecSlotBytes::seqOut);
    f(dSeqLists, DecLists::words(slots, items) * sizeof(uint32_t));
}
size_t zsmi_ctx::DecodeScratch::held() { size_t s = 0; each(DecodePlan(), [&](DevBuf &b, size_t) { s += b.cap; }); return s; }
// give back what an earlier, larger call left behind: a buffer more than twice (and 256 MiB) beyond this call's need is released first
bool zsmi_ctx::DecodeScratch::reserve(const DecodePlan &p)
{
    bool ok = true;
    each(p, [&](DevBuf &b, size_t need) { if (ok && need) { if (b.cap > 2 * need + ((size_t)256 << 20)) b.release(); ok = b.reserve(need); } });
    return ok;
}

// The plan of a call, from what it takes of the call's capacities (CapStats, zsmi_ctx.h).  Block slots per item: 1; 2 when some item can hold more than one 64 KiB block; up to ZS_FAST_MAXBLOCKS when at least a
// quarter of the call's items can hold more than two (a call of large frames; a few large frames among many small ones go to the general kernel,
// so the small ones do not pay for slots and launches they do not use).
// The budget: a call whose buffers all fit asks the runtime nothing (the one-shot path).  When any buffer must grow, the scratch gets half of the
// free device memory and of what the context holds: first the slots per item go back to 2 and 1, then the items in flight are cut down (never
// below one sub-batch of 64, never above n).
static DecodePlan planDecode(zsmi_ctx *c, const CapStats &caps, uint32_t n, bool generalOnly)
{
    DecodePlan p;
    p.fast = c->decodeFast && !generalOnly; p.maxBlocks = caps.over1 ? 2 : 1;
    const uint32_t maxCapBytes = caps.maxCap;
    // (the largest item is one of those that hold more than two blocks, when there are any: it states the slots they need)
    const uint32_t needBlocks = std::min<uint32_t>((uint32_t)(((uint64_t)maxCapBytes + ZS_BLOCK_MAX - 1) / ZS_BLOCK_MAX), ZS_FAST_MAXBLOCKS);
    if (caps.over2 && (uint64_t)caps.over2 * 4 >= n) p.maxBlocks = needBlocks;
    p.descSlots = std::max(2u, p.maxBlocks);
    p.blockCap = std::min<uint32_t>(std::max<uint32_t>(maxCapBytes, 64u), 1u << 17);
    p.litStride = ((p.blockCap + 63u) & ~63u) + 64u; p.litCap = p.litStride - 64u;
    p.seqCap = std::min<uint32_t>(ZS_FAST_MAXSEQ, ((p.blockCap / 3u + 64u) & ~63u));
    p.pool = std::min<uint32_t>(std::max<uint32_t>(n, 1u), c->decodePool);
    p.pool = ((p.pool + ZS_DEC_GROUP - 1) / ZS_DEC_GROUP) * ZS_DEC_GROUP;
    p.cap = std::min<uint32_t>(n, c->maxItemsInFlight);
    zsmi_ctx::DecodeScratch &S = c->dec;
    bool grow = false;
    S.each(p, [&](DevBuf &b, size_t need) { grow |= need > b.cap; });
    size_t freeB = 0, totalB = 0;
    if (p.fast && grow && hipMemGetInfo(&freeB, &totalB) == hipSuccess) {
        const size_t budget = (freeB + S.held()) / 2;                 // (what the context holds already counts as available)
        auto bytesAt = [&](uint32_t items) { DecodePlan q = p; q.cap = items; size_t s = 0; S.each(q, [&](DevBuf &, size_t need) { s += need; }); return s; };
        while (p.maxBlocks > 1 && bytesAt(std::min(p.cap, 64u)) > budget) { p.maxBlocks = p.maxBlocks > 2 ? 2 : 1; p.descSlots = std::max(2u, p.maxBlocks); }
        const size_t fixed = bytesAt(0), perItem = bytesAt(1) - fixed;      // (the bytes grow linearly with the items)
        if (bytesAt(p.cap) > budget)
            p.cap = (uint32_t)std::min<size_t>(p.cap, std::max<size_t>(std::min(64u, n), budget > fixed ? (budget - fixed) / perItem : 0));
    }
    return p;
}

// The launch shapes of a sub-batch of cnt items, chosen by its size
struct DecodeShape { bool fused; uint32_t executeWaves, poolWgs; };     // executeWaves: k_dec_execute<4, 6, 7 or 8>
static DecodeShape decodeShape(const DecodePlan &p, uint32_t cnt, uint32_t cus)
{
    DecodeShape s;
    // One launch for the four entropy kernels, or one each?  Both are rounds of workgroups of an item's chain each: fused, a CU holds 4 workgroups of
    // the 37 KiB image and a round is 2 CUs' worth of Huffman AND sequence groups (8192 items on 256 CUs, ~0.48 ms); apart, 5 workgroups of 30 KiB and
    // a round of each kind is 20480 items (~0.55 ms, twice).  The fewer round-milliseconds win - measured over 8192 .. 65536 frames of 32 KiB: fused
    // below 20480 items except right at it, at 22528 .. 32768 (4.42 against 4.64 ms at 28672) and 49152; apart at 20480, 36864 .. 45056, 53248 .. 61440.
    // Items of several blocks (128 KiB frames: 64 KiB blocks, the 2.5 KiB table class at 16 a wavefront) keep the separate launches: 8192 two-block
    // frames of text decoded at 100 GiB/s fused against 135 apart.
    const uint32_t vcnt = cnt * p.maxBlocks, perF = 32u * cus, perS = 80u * cus;     // (item, block) pairs: what a launch's rounds of workgroups count
    s.fused = p.maxBlocks == 1 && ((vcnt + perF - 1) / perF) * 48u < 2u * ((vcnt + perS - 1) / perS) * 55u;
    // one-block items: 7 wavefronts a SIMD (decode_fast.hip) - but a call that fits ONE round of wavefronts at 8 a SIMD and not at 7 (7169 .. 8192 items on 256 CUs)
    // takes the 8 form: a round of it is ~12 % longer (64 VGPRs: more spills), one round instead of two is not (8192 frames: execute 0.67 -> 0.59 ms; at every
    // other size measured, 4096 .. 57344, the 7 form is as fast or faster)
    const bool oneRoundAt8 = cnt > 7u * 4u * cus && cnt <= 8u * 4u * cus;
    s.executeWaves = p.maxBlocks > 1 ? 6 : (oneRoundAt8 ? 8 : 7);
    s.poolWgs = std::min<uint32_t>((cnt + ZS_DEC_GROUP - 1) / ZS_DEC_GROUP, p.pool / ZS_DEC_GROUP);      // (a workgroup takes ZS_DEC_GROUP items)
    return s;
}

// the item list travels through pinned buffers taken in turn (TurnBufs): a call waits only for the copy that last read the buffer it is
// about to fill (two calls back), not for the device to finish the call before it
static int uploadDecodeItems(zsmi_ctx *c, const uint64_t *srcOffsets, const uint32_t *srcSizes, uint32_t n, const uint64_t *dstOffsets, const uint32_t *dstCaps)
{
    ZsDecItem *hi;
    if (const int e = c->hItems.take(sizeof(ZsDecItem) * n, hi)) return e;
    if (!c->dItems.reserve(sizeof(ZsDecItem) * n)) return ZSMI_error_memory_allocation;
    for (uint32_t i = 0; i < n; i++) { hi[i].srcOff = srcOffsets[i]; hi[i].dstOff = dstOffsets[i]; hi[i].srcSize = srcSizes[i]; hi[i].dstCap = dstCaps[i]; }
    if (const int e = c->toDevice(c->dItems.p, hi, sizeof(ZsDecItem) * n)) return e;
    return c->hItems.sent(c->stream);
}

// The fast path's launches for a sub-batch of cnt items (dI) in the context's scratch: k_dec_prep, the entropy stage, k_dec_execute,
// k_dec_checksum.  DD: the call has digested dictionaries - the dictionary forms of the kernels that need them, with the call's selector.
template <bool DD>
static void launchFastDecode(zsmi_ctx *c, const DecodePlan &p, const DecodeShape &shape, const uint8_t *src, const ZsDecItem *dI, uint32_t cnt, void *dDst,
                             uint32_t *dDstSizes, uint32_t *classes, const ZsDictSel &sel)
{
    zsmi_ctx::DecodeScratch &S = c->dec;
    const uint32_t mb = p.maxBlocks;
    ZsFastDesc *dD = S.fastDesc();
    LAUNCH(c, "k_dec_prep", (k_dec_prep<ZS_DEC_GROUP, DD>), dim3((cnt + ZS_DEC_GROUP - 1) / ZS_DEC_GROUP), dim3(64 * ZS_DEC_GROUP), 0, src, dI, cnt, dD,
           S.hufTabs(), S.seqTabs(), p.cap, mb, classes, p.litCap, p.seqCap, sel);
    // every block index of the items in one launch per kernel class (the grid: mb runs of the items' groups; a wavefront whose items have no such
    // block leaves at once)
    const uint32_t gH0 = ((cnt + ZS_FAST_GROUP - 1) / ZS_FAST_GROUP) * mb, gH1 = ((cnt + 7) / 8) * mb;
    const uint32_t gS0 = ((cnt + ZS_FAST_SEQGROUP_SMALL - 1) / ZS_FAST_SEQGROUP_SMALL) * mb, gS1 = ((cnt + 3) / 4) * mb;
    if (shape.fused) {
        // the four entropy launches as one (k_dec_entropy), the 2.5 KiB sequence class at 4 items a wavefront as below
        LAUNCH(c, "k_dec_entropy", k_dec_entropy<DD>, dim3(gH0 + gH1 + gS0 + gS1), dim3(64), 0, src, dI, cnt, dD, S.hufTabs(), S.litScratch(),
               S.seqTabs(), S.seqOut(), mb, p.cap, (const uint32_t *)classes, p.litStride, p.seqCap, gH0, gH1, gS0, sel);
    } else {
        LAUNCH(c, "k_dec_huffman", (k_dec_huffman<false, ZS_FAST_GROUP, DD>), dim3(gH0), dim3(64), 0, src, dI, cnt, dD, S.hufTabs(), S.litScratch(), mb, p.cap, p.litStride, sel);
        LAUNCH(c, "k_dec_huffman", (k_dec_huffman<true, 8u, DD>), dim3(gH1), dim3(64), 0, src, dI, cnt, dD, S.hufTabs(), S.litScratch(), mb, p.cap, p.litStride, sel);
        LAUNCH(c, "k_dec_sequences", (k_dec_sequences<false, ZS_FAST_SEQGROUP_SMALL>), dim3(gS0), dim3(64), 0, src, dI, cnt, dD, S.seqTabs(), S.seqOut(),
               mb, p.cap, (const uint32_t *)classes, p.seqCap, 0u, 0xFFFFFFFFu);
        // the 2.5 KiB table class (blocks of > 2048 sequences: sources, tables, binaries at 32 KiB; the 64 KiB blocks of 128 KiB frames).  How many blocks of a call
        // are in it only the device knows (k_dec_prep's list), and it decides the shape: 16 items a wavefront when the class holds most of a large call (the
        // wavefront's instructions are what the kernel costs: 57344 frames of Python sources 4.00 -> 3.78 ms, of a binary table 4.99 -> 4.00), 4 a wavefront
        // when it is a fraction of it (libzstd's 32 KiB frames: 9 % of the blocks; fewer, emptier wavefronts finish sooner: 3.8 vs 5.2 ms) or the call is small.
        // Both shapes are launched; each looks at the list's length and leaves at once when the other one serves it.
        LAUNCH(c, "k_dec_sequences", (k_dec_sequences<true, ZS_FAST_SEQGROUP>), dim3(((cnt + ZS_FAST_SEQGROUP - 1) / ZS_FAST_SEQGROUP) * mb), dim3(64), 0, src, dI, cnt, dD,
               S.seqTabs(), S.seqOut(), mb, p.cap, (const uint32_t *)classes, p.seqCap, ZS_FAST_SEQGROUP_MANY, 0xFFFFFFFFu);
        LAUNCH(c, "k_dec_sequences", (k_dec_sequences<true, 4u>), dim3(gS1), dim3(64), 0, src, dI, cnt, dD, S.seqTabs(), S.seqOut(),
               mb, p.cap, (const uint32_t *)classes, p.seqCap, 0u, ZS_FAST_SEQGROUP_MANY);
    }
    const auto execute = shape.executeWaves == 6 ? k_dec_execute<4, 6, DD> : (shape.executeWaves == 8 ? k_dec_execute<4, 8, DD> : k_dec_execute<4, 7, DD>);
    LAUNCH(c, "k_dec_execute", execute, dim3((cnt + 3) / 4), dim3(256), 0, src, dI, cnt, dD, S.seqOut(),
           S.litScratch(), (uint8_t *)dDst, dDstSizes, p.cap, p.descSlots, p.litStride, p.seqCap, sel);
    LAUNCH(c, "k_dec_checksum", k_dec_checksum, dim3((cnt + 15) / 16), dim3(64), 0, dI, cnt, (const ZsFastDesc *)dD, (const uint8_t *)dDst, dDstSizes);
}

// the selector of a call with one dictionary, its bytes in device memory (decode_kernels.hip: ZsDictSel).  img: a digested dictionary's image of
// them, with its ID; none (the _usingDict calls): the device is the one to read the ID - anyID
static ZsDictSel oneDictionary(const void *dBytes, uint32_t size, const ZsDDictImage *img = nullptr, uint32_t dictID = 0)
{
    ZsDictSel sel = ZsDictSel();
    if (dBytes && size) { sel.one.bytes = (const uint8_t *)dBytes; sel.one.size = size; sel.one.img = img; sel.one.dictID = dictID; sel.anyID = img == nullptr; }
    return sel;
}
// dictFromBytes for decode: a dictionary given as bytes (none: the plain call) -> the selector of a call with it, anyID: not digested, the
// general kernel's alone.  In host memory: staged first, behind the checks a host-buffer call makes in front of it (its context, an empty call)
static int dictBytesForDecode(zsmi_ctx *c, const void *dict, size_t dictSize, DictBytes kind, uint32_t n, ZsDictSel &sel)
{
    sel = ZsDictSel();
    if (kind == kDictOnHost) { if (!c) return ZSMI_error_init_missing; if (n == 0) return 0; }
    if (dictSize > 0xFFFFFFFFull) return ZSMI_error_dictionary_corrupted;
    if (kind == kDictOnHost && dict && dictSize) {
        if (const int e = c->bind()) return e;
        if (const int e = stageDict(c, dict, dictSize)) return e;
    }
    sel = oneDictionary(dict, (uint32_t)dictSize); return 0;
}
// dict: which dictionary each frame of the call gets (nullptr, or a selector that holds none: the plain call).  Digested dictionaries bring the
// images the fast kernels' dictionary forms need; a call with a dictionary's bare bytes (anyID) is the general kernel's alone.
// The item list is in c->dItems, queued or copied there on the stream by the caller; caps: what the plan takes of the items' capacities.
static int decodeItems(zsmi_ctx *c, const void *dSrc, uint32_t n, void *dDst, const CapStats &caps, uint32_t *dDstSizes, const ZsDictSel *dict)
{
    const bool useDict = dict && (dict->one.size || dict->n);
    const ZsDictSel sel = useDict ? *dict : ZsDictSel();
    const DecodePlan p = planDecode(c, caps, n, useDict && sel.anyID);
    zsmi_ctx::DecodeScratch &S = c->dec;
    if (!S.reserve(p)) return ZSMI_error_memory_allocation;
    const uint8_t *src = (const uint8_t *)dSrc;
    const uint32_t mb = p.maxBlocks;
    ZsFastDesc *dD = S.fastDesc();
    uint32_t *lists = S.seqLists(), *classes = DecLists::classes(lists), *leftCount = DecLists::leftCount(lists);
    for (uint32_t i0 = 0; i0 < n; i0 += p.cap) {
        const uint32_t cnt = std::min(p.cap, n - i0);
        const ZsDecItem *dI = (const ZsDecItem *)c->dItems.p + i0;
        const DecodeShape shape = decodeShape(p, cnt, c->cus);
        uint32_t *left = nullptr;
        if (p.fast) {
            // items that are one frame of up to mb blocks: entropy decoding lane-parallel across 16 items per wavefront (decode_fast.hip); whatever
            // those kernels do not take or reject is left to the general kernel below
            if (const int e = c->fill(lists, 0, DecLists::kClassLists * sizeof(uint32_t))) return e;
            if (useDict) launchFastDecode<true>(c, p, shape, src, dI, cnt, dDst, dDstSizes + i0, classes, sel);
            else launchFastDecode<false>(c, p, shape, src, dI, cnt, dDst, dDstSizes + i0, classes, sel);
            // the items the fast path did not finish, listed for the general kernel
            left = DecLists::leftList(lists, (size_t)p.cap * mb);
            LAUNCH(c, "k_dec_collect", k_dec_collect, dim3((cnt + 255) / 256), dim3(256), 0, &dD->fast, (uint32_t)(sizeof(ZsFastDesc) / sizeof(uint32_t)), cnt, left, leftCount);
        } else if (const int e = c->fill(lists, 0, (DecLists::kLeftCount + 1) * sizeof(uint32_t))) return e;
        // the general kernel: a pool of wavefronts over a queue - of every item, or (behind the fast path) of the list of the items it left
        LAUNCH(c, useDict ? "k_decode_frames_dict" : "k_decode_frames", useDict ? (k_decode_frames<ZS_DEC_GROUP, true>) : (k_decode_frames<ZS_DEC_GROUP, false>),
               dim3(shape.poolWgs), dim3(64 * ZS_DEC_GROUP), 0, src, dI, cnt, (uint8_t *)dDst, dDstSizes + i0, S.poolLit(), (const uint32_t *)left,
               (const uint32_t *)leftCount, sel, DecLists::queue(lists));
    }
    return c->launched();
}

static int decompressBatchDeviceImpl(zsmi_ctx *c, const void *dSrc, const uint64_t *srcOffsets, const uint32_t *srcSizes,
                                     uint32_t n, void *dDst, const uint64_t *dstOffsets, const uint32_t *dstCaps, uint32_t *dDstSizes,
                                     const ZsDictSel *dict)
{
    if (!c) return ZSMI_error_init_missing;
    if (n == 0) return 0;
    if (const int e = c->bind()) return e;
    if (const int e = uploadDecodeItems(c, srcOffsets, srcSizes, n, dstOffsets, dstCaps)) return e;
    CapStats caps;
    for (uint32_t i = 0; i < n; i++) caps.add(dstCaps[i]);
    return decodeItems(c, dSrc, n, dDst, caps, dDstSizes, dict);
}

extern "C" int zsmi_decompressBatchDevice(zsmi_ctx *c, const void *dSrc, const uint64_t *srcOffsets, const uint32_t *srcSizes,
                                          uint32_t n, void *dDst, const uint64_t *dstOffsets, const uint32_t *dstCaps, uint32_t *dDstSizes)
{
    return decompressBatchDeviceImpl(c, dSrc, srcOffsets, srcSizes, n, dDst, dstOffsets, dstCaps, dDstSizes, nullptr);
}
// every frame of every item is decoded with the dictionary dDict[0 .. dictSize) (device memory; ZSTD_decompress_usingDict,
// ZStdDecompress.cs:2162): raw content or a formatted dictionary (magic 0xEC30A437)
extern "C" int zsmi_decompressBatchDevice_usingDict(zsmi_ctx *c, const void *dSrc, const uint64_t *srcOffsets, const uint32_t *srcSizes,
                                                    uint32_t n, void *dDst, const uint64_t *dstOffsets, const uint32_t *dstCaps, uint32_t *dDstSizes,
                                                    const void *dDict, size_t dictSize)
{
    ZsDictSel sel;
    if (const int e = dictBytesForDecode(c, dDict, dictSize, kDictOnDevice, n, sel)) return e;
    return decompressBatchDeviceImpl(c, dSrc, srcOffsets, srcSizes, n, dDst, dstOffsets, dstCaps, dDstSizes, &sel);
}

// ---- digested decode dictionaries (ZSTD_createDDict / ZSTD_decompress_usingDDict): loaded and checked once (loadDict), the bytes and the image
// the fast kernels' dictionary forms read (ZsDDictImage, filled by the same run of k_dict_load) kept in device memory.  Read-only after creation: any context of the
// same device may use it, from any thread.  A call with one queues its work and returns - nothing is read back, nothing waited for - and its
// dictionary frames take the fast path; what the fast kernels give up goes to k_decode_frames_dict with the same bytes, as in a _usingDict call. ----
struct zsmi_ddict {
    int device = 0;
    bool empty = false;                  // no bytes: its calls are the plain calls
    uint32_t dictID = 0, dictSize = 0;
    ZsDictSel sel = ZsDictSel();         // what its calls pass to the kernels (none for one without bytes)
    DevBuf dBytes, dImg;
};
extern "C" zsmi_ddict *zsmi_createDDict(zsmi_ctx *c, const void *dict, size_t dictSize, int *err)
{
    return makeHandle<zsmi_ddict>(err, [&](zsmi_ddict &dd) -> int {
        if (!c) return ZSMI_error_init_missing;
        if (dictSize > 0xFFFFFFFFull) return ZSMI_error_dictionary_corrupted;
        dd.device = c->device;
        if (!dict || dictSize == 0) { dd.empty = true; return 0; }
        if (const int e = c->bind()) return e;
        if (!dd.dBytes.reserve(dictSize + 64) || !dd.dImg.reserve(sizeof(ZsDDictImage))) return ZSMI_error_memory_allocation;
        if (const int e = c->toDevice(dd.dBytes.p, dict, dictSize)) return e;
        ZsCompressDict d;
        if (const int e = loadDict(c, dd.dBytes.p, dictSize, d, (ZsDDictImage *)dd.dImg.p)) return e;
        dd.dictID = d.dictID; dd.dictSize = (uint32_t)dictSize; dd.sel = oneDictionary(dd.dBytes.p, dd.dictSize, (const ZsDDictImage *)dd.dImg.p, dd.dictID);
        return c->launched();
    });
}
extern "C" void zsmi_freeDDict(zsmi_ddict *dd) { delete dd; }
extern "C" unsigned zsmi_getDictID_fromDDict(const zsmi_ddict *dd) { return dd ? dd->dictID : 0; }
extern "C" size_t zsmi_sizeofDDict(const zsmi_ddict *dd) { return dd ? dd->dBytes.cap + dd->dImg.cap : 0; }
// What a zsmi_ddict * or zsmi_ddictSet * argument asks of a call on context c - 0, with the call's selector set: the handle's (one that holds no
// dictionary: the plain call, for a null handle, a ddict without bytes, an empty set); or the error (digested on another device: parameter_unsupported)
template <class Handle> static int resolveDDict(const zsmi_ctx *c, const Handle *h, ZsDictSel &sel)
{
    sel = ZsDictSel();
    if (!h) return 0;
    if (!c) return ZSMI_error_init_missing;
    if (h->device != c->device) return ZSMI_error_parameter_unsupported;
    sel = h->sel; return 0;
}
extern "C" int zsmi_decompressBatchDevice_usingDDict(zsmi_ctx *c, const void *dSrc, const uint64_t *srcOffsets, const uint32_t *srcSizes,
                                                     uint32_t n, void *dDst, const uint64_t *dstOffsets, const uint32_t *dstCaps, uint32_t *dDstSizes,
                                                     const zsmi_ddict *dd)
{
    ZsDictSel sel;
    if (const int e = resolveDDict(c, dd, sel)) return e;
    return decompressBatchDeviceImpl(c, dSrc, srcOffsets, srcSizes, n, dDst, dstOffsets, dstCaps, dDstSizes, &sel);
}

// ---- DDict sets (ZSTD_d_refMultipleDDicts): a read-only device table of digested dictionaries, sorted by ID; a call with a set gives every
// frame the member its dictID names, on the device (zs_dict_index, decode_kernels.hip).  The set copies nothing from its members: the table holds
// {ID, size, image, bytes} of each, and `sel` is the selector its calls pass to the kernels - the table, and `unnamed` for the frames that name no
// dictionary.  Every check is the host's, before anything touches the device; the one upload is waited for, once. ----
struct zsmi_ddictSet {
    int device = 0;
    uint32_t members = 0;                // dictionaries a frame can name: dds[], and a formatted `unnamed`
    ZsDictSel sel = ZsDictSel();
    DevBuf dTable;
};
#define ZSMI_DDICTSET_MAX 4096u
extern "C" zsmi_ddictSet *zsmi_createDDictSet(zsmi_ctx *c, const zsmi_ddict *const *dds, uint32_t n, const zsmi_ddict *unnamed, int *err)
{
    return makeHandle<zsmi_ddictSet>(err, [&](zsmi_ddictSet &set) -> int {
        if (!c) return ZSMI_error_init_missing;
        if (n > ZSMI_DDICTSET_MAX) return ZSMI_error_parameter_outOfBound;
        if (n && !dds) return ZSMI_error_parameter_unsupported;
        std::vector<ZsDictEntry> table(n);
        for (uint32_t i = 0; i < n; i++) {
            const zsmi_ddict *dd = dds[i];
            // a member: there, of this device, formatted (raw content has no ID a frame could name: it can only be `unnamed`)
            if (!dd || dd->device != c->device || dd->empty || dd->dictID == 0) return ZSMI_error_parameter_unsupported;
            table[i].dictID = dd->dictID; table[i].size = dd->dictSize; table[i].img = (const ZsDDictImage *)dd->dImg.p; table[i].bytes = (const uint8_t *)dd->dBytes.p;
        }
        if (unnamed && unnamed->device != c->device) return ZSMI_error_parameter_unsupported;
        std::sort(table.begin(), table.end(), [](const ZsDictEntry &a, const ZsDictEntry &b) { return a.dictID < b.dictID; });
        const uint32_t unnamedID = (unnamed && !unnamed->empty) ? unnamed->dictID : 0;      // (formatted: a member under its own ID)
        for (uint32_t i = 0; i < n; i++)
            if ((i && table[i].dictID == table[i - 1].dictID) || table[i].dictID == unnamedID) return ZSMI_error_parameter_unsupported;
        set.device = c->device; set.members = n + (unnamedID != 0);
        if (unnamed) set.sel = unnamed->sel;
        if (n == 0) return 0;
        if (const int e = c->bind()) return e;
        if (!set.dTable.reserve(sizeof(ZsDictEntry) * n)) return ZSMI_error_memory_allocation;
        if (c->toDevice(set.dTable.p, table.data(), sizeof(ZsDictEntry) * n) || c->wait()) return ZSMI_error_GENERIC;
        set.sel.table = (const ZsDictEntry *)set.dTable.p; set.sel.n = n;
        return 0;
    });
}
static int ddictSetSel(const zsmi_ctx *c, const zsmi_ddictSet *set, ZsDictSel &sel) { return resolveDDict(c, set, sel); }      // (zsmi_ctx.h: what seekable.hip takes of a set)
extern "C" void zsmi_freeDDictSet(zsmi_ddictSet *set) { delete set; }
extern "C" uint32_t zsmi_sizeofDDictSetMembers(const zsmi_ddictSet *set) { return set ? set->members : 0; }
extern "C" int zsmi_decompressBatchDevice_usingDDictSet(zsmi_ctx *c, const void *dSrc, const uint64_t *srcOffsets, const uint32_t *srcSizes,
                                                        uint32_t n, void *dDst, const uint64_t *dstOffsets, const uint32_t *dstCaps, uint32_t *dDstSizes,
                                                        const zsmi_ddictSet *set)
{
    ZsDictSel sel;
    if (const int e = resolveDDict(c, set, sel)) return e;
    return decompressBatchDeviceImpl(c, dSrc, srcOffsets, srcSizes, n, dDst, dstOffsets, dstCaps, dDstSizes, &sel);
}

// ---------------------------------------------------------------------------------------------
// pack frames
// ---------------------------------------------------------------------------------------------
// offsets[0 .. n]: the exclusive scan of the bytes the items get (zs_layout_cap: a size, or 0 for an error word or a status), each rounded up
// to align; caps (may be null): those bytes.  Three launches under one name (entropy_kernels.hip), the tile sums in context scratch.
template <class Size>
static int scanOffsets(zsmi_ctx *c, const char *name, const Size *dSizes, const uint32_t *dStatus, uint32_t n, uint32_t align, uint32_t *dCaps, uint64_t *dOffsets)
{
    const uint32_t tiles = (uint32_t)(((uint64_t)n + ZS_SCAN_TILE - 1) / ZS_SCAN_TILE);
    if (!c->dScan.reserve(sizeof(uint64_t) * std::max(tiles, 1u))) return ZSMI_error_memory_allocation;
    uint64_t *dTiles = (uint64_t *)c->dScan.p;
    if (tiles) LAUNCH(c, name, k_pack_tile_sums<Size>, dim3(tiles), dim3(256), 0, dSizes, dStatus, n, align, dTiles);
    LAUNCH(c, name, k_pack_scan_tiles, dim3(1), dim3(1024), 0, dTiles, tiles, dOffsets + n);
    if (tiles) LAUNCH(c, name, k_pack_offsets<Size>, dim3(tiles), dim3(256), 0, dSizes, dStatus, n, align, (const uint64_t *)dTiles, dCaps, dOffsets);
    return 0;
}
extern "C" int zsmi_packFramesDevice(zsmi_ctx *c, const void *dFrames, const uint64_t *dstOffsets, const uint32_t *dSizes,
                                     uint32_t n, void *dPacked, uint64_t *dPackedOffsets)
{
    if (!c) return ZSMI_error_init_missing;
    if (n == 0) return 0;
    if (!c->sSizes.reserve(sizeof(uint64_t) * n)) return ZSMI_error_memory_allocation;
    if (const int e = c->toDevice(c->sSizes.p, dstOffsets, sizeof(uint64_t) * n)) return e;
    if (const int e = scanOffsets(c, "k_pack_offsets", dSizes, nullptr, n, 1u, nullptr, dPackedOffsets)) return e;
    LAUNCH(c, "k_pack_copy", k_pack_copy, dim3(n), dim3(256), 0, (const uint8_t *)dFrames, (const uint64_t *)c->sSizes.p, dSizes, (const uint64_t *)dPackedOffsets, (uint8_t *)dPacked);
    return c->launched();
}

// ---------------------------------------------------------------------------------------------
// device-resident decode: sizes, output layout and the decode itself from descriptors that stay in device memory.  The three calls queue
// their kernels and return: nothing is copied to the host, nothing waited for, and the pinned item buffers of the host-array calls (and
// their events) are not touched.
// ---------------------------------------------------------------------------------------------
extern "C" int zsmi_getFrameSizesBatchDevice(zsmi_ctx *c, const void *dSrc, const uint64_t *dSrcOffsets, const uint32_t *dSrcSizes, uint32_t n,
                                             uint64_t *dContentSizes, uint64_t *dBounds, uint32_t *dStatus)
{
    if (!c) return ZSMI_error_init_missing;
    if (n == 0) return 0;
    if (!dSrc || !dSrcOffsets || !dSrcSizes || !dStatus) return ZSMI_error_GENERIC;
    if (const int e = c->bind()) return e;
    LAUNCH(c, "k_frame_sizes", k_frame_sizes, dim3((n + 255) / 256), dim3(256), 0, (const uint8_t *)dSrc, dSrcOffsets, dSrcSizes, n, dContentSizes, dBounds, dStatus);
    return c->launched();
}
// the packer's scan in its general form (the packer's: align 1, no status, no caps)
extern "C" int zsmi_layoutOutputsDevice(zsmi_ctx *c, const uint64_t *dSizes, const uint32_t *dStatus, uint32_t n, uint32_t align,
                                        uint32_t *dDstCaps, uint64_t *dDstOffsets)
{
    if (!c) return ZSMI_error_init_missing;
    if (align == 0 || align > 4096 || (align & (align - 1))) return ZSMI_error_parameter_outOfBound;
    if (!dDstOffsets || (n && (!dSizes || !dDstCaps))) return ZSMI_error_GENERIC;
    if (const int e = c->bind()) return e;
    if (const int e = scanOffsets(c, "k_layout_outputs", dSizes, dStatus, n, align, dDstCaps, dDstOffsets)) return e;
    return c->launched();
}
// The plan is the plan of n items of maxDstCap bytes: the one thing the host knows of the capacities.  Item i's result is that of the
// host-array call with capacity min(dDstCaps[i], maxDstCap) - which kernels take an item never shows in its result.
extern "C" int zsmi_decompressBatchResident(zsmi_ctx *c, const void *dSrc, const uint64_t *dSrcOffsets, const uint32_t *dSrcSizes, uint32_t n,
                                            void *dDst, const uint64_t *dDstOffsets, const uint32_t *dDstCaps, uint32_t maxDstCap,
                                            uint32_t *dDstSizes, const zsmi_ddictSet *set)
{
    if (!c) return ZSMI_error_init_missing;
    if (n && (!dSrc || !dSrcOffsets || !dSrcSizes || !dDst || !dDstOffsets || !dDstCaps || !dDstSizes)) return ZSMI_error_GENERIC;
    ZsDictSel sel;
    if (const int e = resolveDDict(c, set, sel)) return e;
    if (n == 0) return 0;
    if (const int e = c->bind()) return e;
    if (!c->dItems.reserve(sizeof(ZsDecItem) * n)) return ZSMI_error_memory_allocation;
    LAUNCH(c, "k_dec_items", k_dec_items, dim3((n + 255) / 256), dim3(256), 0, dSrcOffsets, dSrcSizes, dDstOffsets, dDstCaps, maxDstCap, n, (ZsDecItem *)c->dItems.p);
    CapStats caps;
    caps.add(maxDstCap, n);
    return decodeItems(c, dSrc, n, dDst, caps, dDstSizes, &sel);
}

// ---------------------------------------------------------------------------------------------
// host-buffer forms
// ---------------------------------------------------------------------------------------------
// [lo, hi): the bytes items of len[i] bytes at off[i] span
static void spanOf(const uint64_t *off, const uint32_t *len, uint32_t n, uint64_t &lo, uint64_t &hi)
{
    lo = ~0ull; hi = 0;
    for (uint32_t i = 0; i < n; i++) { const uint64_t a = off[i], b = off[i] + len[i]; if (a < lo) lo = a; if (b > hi) hi = b; }
    if (lo == ~0ull) { lo = 0; hi = 0; }
}
// Results of a host-buffer call go back to the caller's buffer: items that sit back to back are one transfer; a scattered batch (compressed
// frames in bound-sized slots) is packed on the device, crosses PCIe once into pinned memory and is placed from there (a transfer per item costs
// ~10 us each: 4096 frames took longer to return than to compress)
__global__ void k_pack_items(const uint8_t *base, const uint64_t *offs /* [0..n): where, [n..2n): packed position */, const uint32_t *sizes, uint32_t n, uint8_t *packed)
{
    const uint32_t i = blockIdx.x;
    const uint32_t sz = zs_word_bytes(sizes[i]);
    zs_block_copy(packed + offs[n + i], base + offs[i], sz, threadIdx.x, blockDim.x);
}
static int copyBack(zsmi_ctx *c, const uint8_t *dBase, const uint64_t *dof, uint8_t *dst, const uint64_t *dstOffsets, const uint32_t *sizes, uint32_t n)
{
    if (const int e = c->wait()) return e;                           // (for the sizes, whose copy the caller queued)
    struct Run { uint64_t host, dev, len; };
    std::vector<Run> runs;
    uint64_t total = 0;
    for (uint32_t i = 0; i < n; i++) {
        if (zs_word_bytes(sizes[i]) == 0) continue;
        total += sizes[i];
        if (!runs.empty() && runs.back().host + runs.back().len == dstOffsets[i] && runs.back().dev + runs.back().len == dof[i]) runs.back().len += sizes[i];
        else runs.push_back({ dstOffsets[i], dof[i], sizes[i] });
    }
    if (runs.size() <= 16) {
        for (const Run &r : runs)
            if (const int e = c->toHost(dst + r.host, dBase + r.dev, r.len)) return e;
        return c->wait();
    }
    const size_t listBytes = sizeof(uint64_t) * 2 * n + sizeof(uint32_t) * n;      // (hPack may be resized: nothing is queued since the wait above)
    if (!c->sPack.reserve(total + 64) || !c->sPackOff.reserve(listBytes) || !c->hPack.reserve(std::max<uint64_t>(total, listBytes))) return ZSMI_error_memory_allocation;
    uint64_t *ho = (uint64_t *)c->hPack.p; uint32_t *hs = (uint32_t *)(ho + 2 * n);
    uint64_t run = 0;
    for (uint32_t i = 0; i < n; i++) { ho[i] = dof[i]; ho[n + i] = run; hs[i] = sizes[i]; run += zs_word_bytes(sizes[i]); }
    if (c->toDevice(c->sPackOff.p, ho, listBytes) || c->wait()) return ZSMI_error_GENERIC;      // hPack is reused for the payload below
    LAUNCH(c, "k_pack_items", k_pack_items, dim3(n), dim3(256), 0, dBase, (const uint64_t *)c->sPackOff.p, (const uint32_t *)((const uint64_t *)c->sPackOff.p + 2 * n), n, (uint8_t *)c->sPack.p);
    if (c->toHost(c->hPack.p, c->sPack.p, total) || c->wait()) return ZSMI_error_GENERIC;
    const uint8_t *hp = (const uint8_t *)c->hPack.p;
    run = 0;
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t bytes = zs_word_bytes(sizes[i]);
        memcpy(dst + dstOffsets[i], hp + run, bytes); run += bytes;
    }
    return 0;
}
// A host-buffer call through the context's staging buffers: the span of the sources goes to the device (a dictionary given as bytes is there already), run() is
// the device form with the offsets rebased to the spans (dstLen[i]: the bytes item i may write), then the sizes and the results come back.
template <class Run>
static int staged(zsmi_ctx *c, const void *src, const uint64_t *srcOffsets, const uint32_t *srcSizes, uint32_t n, void *dst, const uint64_t *dstOffsets,
                  const uint32_t *dstLen, uint32_t *dstSizes, Run run)
{
    if (const int e = c->bind()) return e;
    uint64_t slo, shi, dlo, dhi;
    spanOf(srcOffsets, srcSizes, n, slo, shi);
    spanOf(dstOffsets, dstLen, n, dlo, dhi);
    if (!c->sSrc.reserve(shi - slo + 64) || !c->sDst.reserve(dhi - dlo + 64) || !c->sSizes.reserve(sizeof(uint32_t) * n)) return ZSMI_error_memory_allocation;
    std::vector<uint64_t> so(n), dof(n);
    for (uint32_t i = 0; i < n; i++) { so[i] = srcOffsets[i] - slo; dof[i] = dstOffsets[i] - dlo; }
    if (shi > slo) if (const int e = c->toDevice(c->sSrc.p, (const uint8_t *)src + slo, shi - slo)) return e;
    if (const int rc = run(so.data(), dof.data(), (uint32_t *)c->sSizes.p)) return rc;
    if (const int e = c->toHost(dstSizes, c->sSizes.p, sizeof(uint32_t) * n)) return e;
    return copyBack(c, (const uint8_t *)c->sDst.p, dof.data(), (uint8_t *)dst, dstOffsets, dstSizes, n);
}
// dict: the call's selector, of dictionaries that are on the device already; checksum: as compressBatchDeviceImpl's
static int compressBatchHostImpl(zsmi_ctx *c, const void *src, const uint64_t *srcOffsets, const uint32_t *srcSizes, uint32_t n, void *dst, const uint64_t *dstOffsets,
                                 uint32_t *dstSizes, int level, const ZsCDictSel *dict, int checksum)
{
    if (!c) return ZSMI_error_init_missing;
    if (n == 0) return 0;
    std::vector<uint32_t> bounds(n);                                 // the destination slots the call is staged with: every chunk's bound
    for (uint32_t i = 0; i < n; i++) bounds[i] = (uint32_t)zsmi_compressBound(srcSizes[i]);
    return staged(c, src, srcOffsets, srcSizes, n, dst, dstOffsets, bounds.data(), dstSizes,
                  [&](const uint64_t *so, const uint64_t *dof, uint32_t *dSizes) {
                      return compressBatchDeviceImpl(c, c->sSrc.p, so, srcSizes, n, c->sDst.p, dof, dSizes, level, dict, checksum);
                  });
}
extern "C" int zsmi_compressBatchHost(zsmi_ctx *c, const void *src, const uint64_t *srcOffsets, const uint32_t *srcSizes,
                                      uint32_t n, void *dst, const uint64_t *dstOffsets, uint32_t *dstSizes, int level)
{
    return compressBatchHostImpl(c, src, srcOffsets, srcSizes, n, dst, dstOffsets, dstSizes, level, nullptr, c ? c->checksumFlag : 0);
}
// The dictionary is staged and loaded first (dictFromBytes: its copy, the loader, the one wait - a refusal comes before anything of the
// sources is allocated or copied), then the sources are staged and the call runs as the _usingCDict form's does
extern "C" int zsmi_compressBatchHost_usingDict(zsmi_ctx *c, const void *src, const uint64_t *srcOffsets, const uint32_t *srcSizes,
                                                uint32_t n, void *dst, const uint64_t *dstOffsets, uint32_t *dstSizes, int level,
                                                const void *dict, size_t dictSize)
{
    ZsCDictSel sel;
    if (const int e = dictFromBytes(c, dict, dictSize, kDictOnHost, level, n, sel)) return e;
    return compressBatchHostImpl(c, src, srcOffsets, srcSizes, n, dst, dstOffsets, dstSizes, level, &sel, c ? c->checksumFlag : 0);
}
extern "C" int zsmi_compressBatchHost_usingCDict(zsmi_ctx *c, const void *src, const uint64_t *srcOffsets, const uint32_t *srcSizes,
                                                 uint32_t n, void *dst, const uint64_t *dstOffsets, uint32_t *dstSizes, const zsmi_cdict *cd)
{
    int level; ZsCDictSel sel;
    if (const int e = resolveCDict(c, cd, level, sel)) return e;
    return compressBatchHostImpl(c, src, srcOffsets, srcSizes, n, dst, dstOffsets, dstSizes, level, &sel, c ? c->checksumFlag : 0);
}
extern "C" int zsmi_compressBatchHost_usingCDictSet(zsmi_ctx *c, const void *src, const uint64_t *srcOffsets, const uint32_t *srcSizes,
                                                    uint32_t n, void *dst, const uint64_t *dstOffsets, uint32_t *dstSizes,
                                                    const zsmi_cdictSet *set, const uint32_t *dictIndex)
{
    int level; ZsCDictSel sel;
    if (const int e = resolveCDictSet(c, set, dictIndex, n, level, sel)) return e;
    return compressBatchHostImpl(c, src, srcOffsets, srcSizes, n, dst, dstOffsets, dstSizes, level, &sel, c->checksumFlag);
}
// dict: the call's selector, of dictionaries that are on the device already (digested ones, or bytes dictBytesForDecode staged)
static int decompressBatchHostImpl(zsmi_ctx *c, const void *src, const uint64_t *srcOffsets, const uint32_t *srcSizes,
                                   uint32_t n, void *dst, const uint64_t *dstOffsets, const uint32_t *dstCaps, uint32_t *dstSizes, const ZsDictSel *dict)
{
    if (!c) return ZSMI_error_init_missing;
    if (n == 0) return 0;
    return staged(c, src, srcOffsets, srcSizes, n, dst, dstOffsets, dstCaps, dstSizes,
                  [&](const uint64_t *so, const uint64_t *dof, uint32_t *dSizes) {
                      return decompressBatchDeviceImpl(c, c->sSrc.p, so, srcSizes, n, c->sDst.p, dof, dstCaps, dSizes, dict);
                  });
}

extern "C" int zsmi_decompressBatchHost(zsmi_ctx *c, const void *src, const uint64_t *srcOffsets, const uint32_t *srcSizes,
                                        uint32_t n, void *dst, const uint64_t *dstOffsets, const uint32_t *dstCaps, uint32_t *dstSizes)
{
    return decompressBatchHostImpl(c, src, srcOffsets, srcSizes, n, dst, dstOffsets, dstCaps, dstSizes, nullptr);
}
extern "C" int zsmi_decompressBatchHost_usingDict(zsmi_ctx *c, const void *src, const uint64_t *srcOffsets, const uint32_t *srcSizes,
                                                  uint32_t n, void *dst, const uint64_t *dstOffsets, const uint32_t *dstCaps, uint32_t *dstSizes,
                                                  const void *dict, size_t dictSize)
{
    ZsDictSel sel;
    if (const int e = dictBytesForDecode(c, dict, dictSize, kDictOnHost, n, sel)) return e;
    return decompressBatchHostImpl(c, src, srcOffsets, srcSizes, n, dst, dstOffsets, dstCaps, dstSizes, &sel);
}
extern "C" int zsmi_decompressBatchHost_usingDDict(zsmi_ctx *c, const void *src, const uint64_t *srcOffsets, const uint32_t *srcSizes,
                                                   uint32_t n, void *dst, const uint64_t *dstOffsets, const uint32_t *dstCaps, uint32_t *dstSizes,
                                                   const zsmi_ddict *dd)
{
    ZsDictSel sel;
    if (const int e = resolveDDict(c, dd, sel)) return e;
    return decompressBatchHostImpl(c, src, srcOffsets, srcSizes, n, dst, dstOffsets, dstCaps, dstSizes, &sel);
}
extern "C" int zsmi_decompressBatchHost_usingDDictSet(zsmi_ctx *c, const void *src, const uint64_t *srcOffsets, const uint32_t *srcSizes,
                                                      uint32_t n, void *dst, const uint64_t *dstOffsets, const uint32_t *dstCaps, uint32_t *dstSizes,
                                                      const zsmi_ddictSet *set)
{
    ZsDictSel sel;
    if (const int e = resolveDDict(c, set, sel)) return e;
    return decompressBatchHostImpl(c, src, srcOffsets, srcSizes, n, dst, dstOffsets, dstCaps, dstSizes, &sel);
}

// ---------------------------------------------------------------------------------------------
// one-shot calls (the reference's public API shape).  The reference's static calls are re-entrant: a fresh DCtx per call
// (ZStdDecompress.cs:2174-2180).  Here a call borrows a context from a per-device pool (created on demand, at most
// ZSMI_ONESHOT_CONTEXTS = 8 per device; further callers wait), so concurrent callers run side by side instead of queueing behind
// one mutex, and a context's device buffers are reused from call to call.  The pool is emptied when the library is unloaded.
// ---------------------------------------------------------------------------------------------
namespace {
struct OneShotPool {
    static const int kMax = 8;
    std::mutex mu;
    std::condition_variable cv;
    struct PerDevice { std::vector<zsmi_ctx *> idle; int created = 0; };
    std::map<int, PerDevice> dev;
    zsmi_ctx *acquire()
    {
        int d = 0;
        if (hipGetDevice(&d) != hipSuccess) return nullptr;
        std::unique_lock<std::mutex> lk(mu);
        PerDevice &p = dev[d];
        for (;;) {
            if (!p.idle.empty()) { zsmi_ctx *c = p.idle.back(); p.idle.pop_back(); return c; }
            if (p.created < kMax) {
                p.created++;
                lk.unlock();
                zsmi_ctx *c = zsmi_createCtx(d, nullptr);
                if (!c) { lk.lock(); p.created--; cv.notify_one(); }
                return c;
            }
            cv.wait(lk);
        }
    }
    void release(zsmi_ctx *c)
    {
        { std::lock_guard<std::mutex> lk(mu); dev[c->device].idle.push_back(c); }
        cv.notify_one();
    }
    // No destructor work: at process exit or dlclose the order against the HIP runtime's own teardown is not defined, and HIP calls from an
    // exit-time destructor are a known source of aborts.  The contexts are left to the process; an embedder that unloads the library
    // calls zsmi_shutdown() first.
    void drain()
    {
        std::lock_guard<std::mutex> lk(mu);
        for (auto &kv : dev) { for (zsmi_ctx *c : kv.second.idle) { zsmi_freeCtx(c); kv.second.created--; } kv.second.idle.clear(); }
    }
};
OneShotPool &g_pool = *new OneShotPool();                  // (never destroyed: see above)
}
Borrowed::Borrowed() : c(g_pool.acquire()) {}
Borrowed::~Borrowed() { if (c) g_pool.release(c); }

extern "C" void zsmi_shutdown(void) { g_pool.drain(); }
extern "C" size_t zsmi_decodeScratchBytes(zsmi_ctx *c)
{
    if (!c) return 0;
    return c->dec.held();
}

// one frame through a borrowed context.  resolve(c, level, sel): the call's dictionary, resolved on that context as the batch forms resolve
// theirs.  checksum: the call's own - the borrowed context's sticky state is neither read nor changed
template <class Resolve>
static size_t compressOneShot(void *dst, size_t dstCapacity, const void *src, size_t srcSize, int level, int checksum, Resolve resolve)
{
    if (srcSize > 0xFFFFFFFFull) return ZSMI_ERR(ZSMI_error_srcSize_wrong);
    Borrowed b; zsmi_ctx *c = b.c;
    if (!c) return ZSMI_ERR(ZSMI_error_GENERIC);
    const size_t bound = zsmi_compressBound(srcSize);
    std::vector<uint8_t> tmp;
    uint8_t *out = (uint8_t *)dst;
    if (dstCapacity < bound) { tmp.resize(bound); out = tmp.data(); }     // compress into a bound-sized buffer, then check the fit
    const uint64_t so = 0, dof = 0; const uint32_t ss = (uint32_t)srcSize; uint32_t ds = 0;
    ZsCDictSel sel;
    int rc = resolve(c, level, sel);
    if (!rc) rc = compressBatchHostImpl(c, src, &so, &ss, 1, out, &dof, &ds, level, &sel, checksum);
    if (rc) return ZSMI_ERR(rc);
    if (zs_word_is_error(ds)) return ZSMI_ERR(zs_word_code(ds));
    if (ds > dstCapacity) return ZSMI_ERR(ZSMI_error_dstSize_tooSmall);
    if (out != dst) memcpy(dst, out, ds);
    return ds;
}
// at `level` with the dictionary's bytes (or with none)
static size_t compressOneShotUsingDict(void *dst, size_t dstCapacity, const void *src, size_t srcSize, const void *dict, size_t dictSize, int level, int checksum)
{
    return compressOneShot(dst, dstCapacity, src, srcSize, level, checksum, [&](zsmi_ctx *c, int &lv, ZsCDictSel &sel) { return dictFromBytes(c, dict, dictSize, kDictOnHost, lv, 1, sel); });
}
// with the digested dictionary cd; a null cd: the plain call at level 3.  (The borrowed context is the current device's: a dictionary of another is parameter_unsupported)
static size_t compressOneShotUsingCDict(void *dst, size_t dstCapacity, const void *src, size_t srcSize, const zsmi_cdict *cd, int checksum)
{
    return compressOneShot(dst, dstCapacity, src, srcSize, 3, checksum, [&](zsmi_ctx *c, int &lv, ZsCDictSel &sel) { return resolveCDict(c, cd, lv, sel); });
}
extern "C" size_t zsmi_compress(void *dst, size_t dstCapacity, const void *src, size_t srcSize, int level)
{
    return compressOneShotUsingDict(dst, dstCapacity, src, srcSize, nullptr, 0, level, 0);
}
extern "C" size_t zsmi_compress_usingDict(void *dst, size_t dstCapacity, const void *src, size_t srcSize, const void *dict, size_t dictSize, int level)
{
    return compressOneShotUsingDict(dst, dstCapacity, src, srcSize, dict, dictSize, level, 0);
}
extern "C" size_t zsmi_compress_usingCDict(void *dst, size_t dstCapacity, const void *src, size_t srcSize, const zsmi_cdict *cd)
{
    return compressOneShotUsingCDict(dst, dstCapacity, src, srcSize, cd, 0);
}
// the one-shot forms with a checksumFlag (0: the frames of the calls above, byte for byte; any other value: 1)
extern "C" size_t zsmi_compress_advanced(void *dst, size_t dstCapacity, const void *src, size_t srcSize, const void *dict, size_t dictSize, int level, int checksumFlag)
{
    return compressOneShotUsingDict(dst, dstCapacity, src, srcSize, dict, dictSize, level, checksumFlag != 0);
}
extern "C" size_t zsmi_compress_usingCDict_advanced(void *dst, size_t dstCapacity, const void *src, size_t srcSize, const zsmi_cdict *cd, int checksumFlag)
{
    return compressOneShotUsingCDict(dst, dstCapacity, src, srcSize, cd, checksumFlag != 0);
}
extern "C" size_t zsmi_decompress(void *dst, size_t dstCapacity, const void *src, size_t srcSize)
{
    return zsmi_decompress_usingDict(dst, dstCapacity, src, srcSize, nullptr, 0);
}

// one frame (or several concatenated) through a borrowed context.  resolve(c, sel): the call's dictionary, resolved on that context as the
// batch forms resolve theirs - its bytes (or none), a digested dictionary, a DDict set
template <class Resolve>
static size_t decompressOneShot(void *dst, size_t dstCapacity, const void *src, size_t srcSize, Resolve resolve)
{
    if (srcSize > 0xFFFFFFFFull) return ZSMI_ERR(ZSMI_error_srcSize_wrong);
    Borrowed b; zsmi_ctx *c = b.c;
    if (!c) return ZSMI_ERR(ZSMI_error_GENERIC);
    const uint64_t so = 0, dof = 0; const uint32_t ss = (uint32_t)srcSize; uint32_t ds = 0;
    const uint32_t cap = (uint32_t)std::min<size_t>(dstCapacity, ZS_ONESHOT_CAP_MAX);
    ZsDictSel sel;
    int rc = resolve(c, sel);
    if (!rc) rc = decompressBatchHostImpl(c, src, &so, &ss, 1, dst, &dof, &cap, &ds, &sel);
    if (rc) return ZSMI_ERR(rc);
    if (zs_word_is_error(ds)) return ZSMI_ERR(zs_word_code(ds));
    return ds;
}
extern "C" size_t zsmi_decompress_usingDict(void *dst, size_t dstCapacity, const void *src, size_t srcSize, const void *dict, size_t dictSize)
{
    return decompressOneShot(dst, dstCapacity, src, srcSize, [&](zsmi_ctx *c, ZsDictSel &sel) { return dictBytesForDecode(c, dict, dictSize, kDictOnHost, 1, sel); });
}
// a null dd: zsmi_decompress.  (The borrowed context is one of the current device: a dictionary digested on another device is parameter_unsupported)
extern "C" size_t zsmi_decompress_usingDDict(void *dst, size_t dstCapacity, const void *src, size_t srcSize, const zsmi_ddict *dd)
{
    return decompressOneShot(dst, dstCapacity, src, srcSize, [&](zsmi_ctx *c, ZsDictSel &sel) { return resolveDDict(c, dd, sel); });
}
// a null set: zsmi_decompress
extern "C" size_t zsmi_decompress_usingDDictSet(void *dst, size_t dstCapacity, const void *src, size_t srcSize, const zsmi_ddictSet *set)
{
    return decompressOneShot(dst, dstCapacity, src, srcSize, [&](zsmi_ctx *c, ZsDictSel &sel) { return resolveDDict(c, set, sel); });
}

#ifdef ZSMI_DEBUG_HOOKS
// ---- test hooks (not in include/zsmi.h) ----
// words of a ZsFastDesc, and the word index of its fields `fast`, `why`, `nbSeq`, `litType`, `hufLog` (tools/fastpath_check.py, tools/dec_why.py)
extern "C" void zsmi_dbg_descLayout(uint32_t out[6])
{
    out[0] = (uint32_t)(sizeof(ZsFastDesc) / 4); out[1] = (uint32_t)(offsetof(ZsFastDesc, fast) / 4); out[2] = (uint32_t)(offsetof(ZsFastDesc, why) / 4);
    out[3] = (uint32_t)(offsetof(ZsFastDesc, nbSeq) / 4); out[4] = (uint32_t)(offsetof(ZsFastDesc, litType) / 4); out[5] = (uint32_t)(offsetof(ZsFastDesc, hufLog) / 4);
}
// The scratch buffers a tool can name: the twelve of the compress side by their names in ZS_SCRATCH_TABLE (zsmi_scratch.h), and the decode
// side's whose stride no plan chooses.  c: nullptr to ask for the layout alone.
static const ZsScratchRow *dbgScratch(zsmi_ctx *c, const char *name, DevBuf **buf)
{
    static const ZsScratchRow dec[] = { { "poolLit", ZsDecSlotBytes::poolLit, 0 }, { "hufTabs", ZsDecSlotBytes::hufTabs, 0 }, { "seqTabs", ZsDecSlotBytes::seqTabs, 0 },
                                        { "fastDesc", sizeof(ZsFastDesc), 0 } };
    if (!name) return nullptr;
    for (int i = 0; i < kZsScratchCount; i++)
        if (!strcmp(name, kZsScratchRows[i].name)) { if (c) *buf = &c->scratch.buf[i]; return &kZsScratchRows[i]; }
    for (int i = 0; i < 4; i++)
        if (!strcmp(name, dec[i].name)) { if (c) *buf = i == 0 ? &c->dec.dPoolLit : i == 1 ? &c->dec.dHufTabs : i == 2 ? &c->dec.dSeqTabs : &c->dec.dFastDesc; return &dec[i]; }
    return nullptr;
}
// out[0]: bytes a slot of the buffer (compress: a block; poolLit: a wavefront; hufTabs, seqTabs: a block slot; fastDesc: a descriptor),
// out[1]: the fixed bytes behind the slots.  Host only.  0, or -1 for a name that is no buffer's.
extern "C" int zsmi_dbg_scratchLayout(const char *name, uint64_t out[2])
{
    const ZsScratchRow *row = dbgScratch(nullptr, name, nullptr);
    if (!row) return -1;
    out[0] = row->slotBytes; out[1] = row->tailBytes;
    return 0;
}
// copies the first `bytes` of the named buffer, as the context's last call left it, to the host (-1: no context or no such buffer)
extern "C" int zsmi_dbg_copyScratch(zsmi_ctx *c, const char *name, void *hostDst, size_t bytes)
{
    DevBuf *b = nullptr;
    if (!c || !dbgScratch(c, name, &b)) return -1;
    (void)hipStreamSynchronize(c->stream);
    if (bytes > b->cap) return -2;
    return hipMemcpy(hostDst, b->p, bytes, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -3;
}

// ---- scratch poisoning (tests/test_gpu_scratch_independence.py): everything a context carries from call to call is overwritten, so that a
// kernel which reads a word nobody wrote for THIS call reads poison and not the well-formed leftovers of the call before.  DESIGN.md, "What a
// context's memory may carry from call to call", states for every buffer below why the next call does not depend on it.
// The groups bytesFilled reports, and every buffer member of zsmi_ctx.h in one list: visit(group, name, buffer).  A TurnBufs is its two buffers.
enum { kFillCompress, kFillResident, kFillDecode, kFillStaging, kFillSeek, kFillTrain, kFillPlan, kFillGroups };
static const char *const kFillGroupNames[kFillGroups] = { "compress", "resident", "decode", "staging", "seek", "train", "plan" };
template <class F> static void eachCtxBuffer(zsmi_ctx *c, F visit)
{
    auto turn = [&](int g, const char *name, TurnBufs &t) { visit(g, name, t.buf[0]); visit(g, name, t.buf[1]); };
    for (int i = 0; i < kZsScratchCount; i++) visit(kFillCompress, "scratch.buf", c->scratch.buf[i]);
    zsmi_ctx::ResidentPlan &R = c->resident;
    visit(kFillResident, "resident.dChunks", R.dChunks); visit(kFillResident, "resident.dBefore", R.dBefore); visit(kFillResident, "resident.dCounts", R.dCounts);
    visit(kFillResident, "resident.dBlocks", R.dBlocks); visit(kFillResident, "resident.dUnits", R.dUnits);
    visit(kFillResident, "resident.dChunkDict", R.dChunkDict); visit(kFillResident, "resident.dUnitDict", R.dUnitDict);
    zsmi_ctx::DecodeScratch &D = c->dec;
    visit(kFillDecode, "dItems", c->dItems); turn(kFillDecode, "hItems", c->hItems);
    visit(kFillDecode, "dec.dPoolLit", D.dPoolLit); visit(kFillDecode, "dec.dLitScratch", D.dLitScratch); visit(kFillDecode, "dec.dFastDesc", D.dFastDesc);
    visit(kFillDecode, "dec.dHufTabs", D.dHufTabs); visit(kFillDecode, "dec.dSeqTabs", D.dSeqTabs); visit(kFillDecode, "dec.dSeqOut", D.dSeqOut);
    visit(kFillDecode, "dec.dSeqLists", D.dSeqLists);
    visit(kFillStaging, "dDictImg", c->dDictImg); visit(kFillStaging, "dDictRec", c->dDictRec); visit(kFillStaging, "hDictRec", c->hDictRec);
    visit(kFillStaging, "sSrc", c->sSrc); visit(kFillStaging, "sDst", c->sDst); visit(kFillStaging, "sSizes", c->sSizes); visit(kFillStaging, "sDict", c->sDict);
    visit(kFillStaging, "sPack", c->sPack); visit(kFillStaging, "sPackOff", c->sPackOff); visit(kFillStaging, "dScan", c->dScan); visit(kFillStaging, "hPack", c->hPack);
    visit(kFillSeek, "seek.dStage", c->seek.dStage); visit(kFillSeek, "seek.dMeta", c->seek.dMeta); visit(kFillSeek, "seek.dDec", c->seek.dDec);
    turn(kFillSeek, "seek.hLists", c->seek.hLists);
    zsmi_ctx::TrainScratch &T = c->train;
    visit(kFillTrain, "train.dSamples", T.dSamples); visit(kFillTrain, "train.dGather", T.dGather); visit(kFillTrain, "train.dEnds", T.dEnds);
    visit(kFillTrain, "train.dKeys", T.dKeys); visit(kFillTrain, "train.dKeysOut", T.dKeysOut); visit(kFillTrain, "train.dSortTmp", T.dSortTmp);
    visit(kFillTrain, "train.dInfo", T.dInfo[0]); visit(kFillTrain, "train.dInfo", T.dInfo[1]);
    visit(kFillTrain, "train.dFreqBase", T.dFreqBase); visit(kFillTrain, "train.dFreq", T.dFreq); visit(kFillTrain, "train.dContent", T.dContent);
    visit(kFillTrain, "train.dCand", T.dCand); visit(kFillTrain, "train.dArena", T.dArena); visit(kFillTrain, "train.dSizes", T.dSizes);
    visit(kFillTrain, "train.dMisc", T.dMisc); visit(kFillTrain, "train.dOut", T.dOut); visit(kFillTrain, "train.hCand", T.hCand);
    CompressPlan &P = c->plan;
    visit(kFillPlan, "plan.hBlocks", P.hBlocks); visit(kFillPlan, "plan.hChunks", P.hChunks); visit(kFillPlan, "plan.hUnits", P.hUnits);
    visit(kFillPlan, "plan.dBlocks", P.dBlocks); visit(kFillPlan, "plan.dChunks", P.dChunks); visit(kFillPlan, "plan.dUnits", P.dUnits);
    visit(kFillPlan, "plan.dDictList", P.dDictList); turn(kFillPlan, "plan.hDictList", P.hDictList);
}
// The member names the fill covers, one a line as "<group> filled <member>", then the plan's words that are valid across calls by design and are
// forgotten with it ("plan forgotten <member>"), then what is kept as state ("<group> state <member>": which of a TurnBufs' two buffers is next, and
// the events behind them - no call reads anything through them).  Host only: c may be null.  Returns the bytes the text takes (with its 0), whatever cap is.
extern "C" size_t zsmi_dbg_scratchInventory(char *out, size_t cap)
{
    std::string text, last;
    zsmi_ctx blank;                                            // (a context as its constructor leaves it holds nothing and touches no device)
    struct Names { std::string &text, &last; void operator()(int g, const char *name, const DevBuf &) { add(g, name); } void operator()(int g, const char *name, const PinBuf &) { add(g, name); }
                   void add(int g, const char *name) { if (last != name) { text += kFillGroupNames[g]; text += " filled "; text += name; text += "\n"; last = name; } } };
    Names names{ text, last };
    eachCtxBuffer(&blank, names);
    for (const char *m : { "plan.key", "plan.dictKey", "plan.dictKind" }) { text += "plan forgotten "; text += m; text += "\n"; }
    for (const char *m : { "decode state hItems.turns", "seek state seek.hLists.turns", "plan state plan.hDictList.turns" }) { text += m; text += "\n"; }
    if (out && cap) { const size_t n = std::min(cap - 1, text.size()); memcpy(out, text.data(), n); out[n] = 0; }
    return text.size() + 1;
}
// a word of the mixed pattern: a hash of the word's offset and the pattern, a quarter of the words cut down to a byte and a quarter to 20 bits -
// values that pass for small counts, slots and positions
__host__ __device__ static inline uint32_t dbgPoisonWord(uint64_t word, uint32_t pattern)
{
    uint32_t h = ((uint32_t)word * 0x9E3779B1u) ^ (uint32_t)(word >> 32) ^ pattern;
    h ^= h >> 15; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
    const uint32_t kind = h >> 30;
    return kind == 0 ? (h & 0xFFu) : kind == 1 ? (h & 0xFFFFFu) : h;
}
__global__ void k_dbg_poison(uint32_t *p, uint64_t words, uint32_t pattern)
{
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < words; i += (uint64_t)gridDim.x * blockDim.x) p[i] = dbgPoisonWord(i, pattern);
}
// Overwrites the whole capacity of every buffer of eachCtxBuffer - growth slack and fixed tails included - behind a wait for the context's stream, and
// forgets the compress plan (its buffers are filled like the rest).  pattern 0 .. 255: that byte; any other value: dbgPoisonWord (the bytes behind a
// buffer's last whole word get the pattern's low byte).  bytesFilled (may be null): kFillGroups sums, in the order of kFillGroupNames.  Handles
// (dictionaries, their sets, open archives) are not the context's and are not touched.  0, or a negative code.
extern "C" int zsmi_dbg_fillScratch(zsmi_ctx *c, uint32_t pattern, uint64_t *bytesFilled)
{
    if (!c) return -1;
    if (c->bind() || c->wait()) return -2;
    uint64_t sums[kFillGroups] = { 0 };
    bool ok = true;
    struct Fill {
        zsmi_ctx *c; uint32_t pattern; uint64_t *sums; bool &ok;
        void operator()(int g, const char *, DevBuf &b)
        {
            if (!b.p || !b.cap) return;
            sums[g] += b.cap;
            if (pattern < 256u) { ok &= c->fill(b.p, (int)pattern, b.cap) == 0; return; }
            const uint64_t words = b.cap / 4;                  // (hipMalloc's blocks are aligned far beyond a word)
            if (words) hipLaunchKernelGGL(k_dbg_poison, dim3((unsigned)std::min<uint64_t>((words + 255) / 256, 4096)), dim3(256), 0, c->stream, (uint32_t *)b.p, words, pattern);
            if (b.cap & 3) ok &= c->fill((uint8_t *)b.p + words * 4, (int)(pattern & 0xFFu), b.cap & 3) == 0;
        }
        void operator()(int g, const char *, PinBuf &b)          // idle: the stream was waited for, and every copy that read it is behind us
        {
            if (!b.p || !b.cap) return;
            sums[g] += b.cap;
            if (pattern < 256u) { memset(b.p, (int)pattern, b.cap); return; }
            uint32_t *w = (uint32_t *)b.p;
            for (uint64_t i = 0; i < b.cap / 4; i++) w[i] = dbgPoisonWord(i, pattern);
            memset((uint8_t *)b.p + (b.cap & ~(size_t)3), (int)(pattern & 0xFFu), b.cap & 3);
        }
    } fill{ c, pattern, sums, ok };
    eachCtxBuffer(c, fill);
    c->plan.key.clear(); c->plan.dictKey.clear(); c->plan.dictKind = CompressPlan::kDictNone;
    ok &= c->launched() == 0;
    ok &= c->wait() == 0;
    if (bytesFilled) for (int g = 0; g < kFillGroups; g++) bytesFilled[g] = sums[g];
    return ok ? 0 : -3;
}
#endif
