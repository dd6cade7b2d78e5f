// Host side that zsmi_api.hip and the feature files (seekable.hip, dict_train.hip) share: the context with its buffers (Buf; TurnBufs, the
// pinned buffers a per-call list goes up through) and stream verbs, the handle maker, the timed launch, and the batch entry points the features are built on (defined in
// zsmi_api.hip) with the one thing they take about dictionaries - the compress calls a ZsCDictSel, the decompress calls a ZsDictSel.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/zsmi.h"
#include "zsmi_status.h"          // the size word the kernels leave and the host reads
#include "zsmi_device.h"
#include "zsmi_scratch.h"         // what the scratch buffers hold: the table Scratch is made of

#include <cstring>
#include <new>
#include <vector>

#define ZSMI_ERR(code) ((size_t)0 - (size_t)(code))

// ---------------------------------------------------------------------------------------------
// context
// ---------------------------------------------------------------------------------------------
// A buffer that grows by 1/8 + 4 KiB beyond the request; device or pinned host memory.  The context owns its buffers: they go with it.
// Growing frees the old block first: a DEVICE buffer relies on the runtime's free waiting for the device.  Nothing else assumes it: a PINNED
// buffer that a queued copy may still read grows only behind a wait for the stream (zsmi_ctx::idleReserve) or that copy's event (TurnBufs).
static hipError_t devAlloc(void **p, size_t n) { return hipMalloc(p, n); }
static hipError_t pinAlloc(void **p, size_t n) { return hipHostMalloc(p, n, hipHostMallocDefault); }
template <hipError_t (*Alloc)(void **, size_t), hipError_t (*Free)(void *)>
struct Buf {
    void *p = nullptr; size_t cap = 0;
    Buf() = default;
    Buf(const Buf &) = delete;
    Buf &operator=(const Buf &) = delete;
    ~Buf() { release(); }
    bool reserve(size_t n) {
        if (n <= cap) return true;
        release();
        size_t want = n + (n >> 3) + 4096;
        if (Alloc(&p, want) != hipSuccess) { p = nullptr; return false; }
        cap = want; return true;
    }
    void release() { if (p) (void)Free(p); p = nullptr; cap = 0; }
};
typedef Buf<devAlloc, hipFree> DevBuf;
typedef Buf<pinAlloc, hipHostFree> PinBuf;
// Two pinned buffers taken in turn, each behind an event (made with the context: create): a list that goes up with every call travels through
// them, and a call waits only for the copy that last read the buffer it is about to fill (two calls back), never for the stream.  take: the next buffer, idle, of
// >= n bytes, in p.  sent: the copy that reads it is queued on the stream; a record that fails is the call's error and leaves it known idle - the stream is waited for
struct TurnBufs {
    PinBuf buf[2]; hipEvent_t ev[2] = { nullptr, nullptr }; bool busy[2] = { false, false }; uint32_t turns = 0;
    ~TurnBufs() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); }
    bool create() { return hipEventCreateWithFlags(&ev[0], hipEventDisableTiming) == hipSuccess && hipEventCreateWithFlags(&ev[1], hipEventDisableTiming) == hipSuccess; }
    template <class T> int take(size_t n, T *&p)
    {
        const int t = (int)(turns++ & 1u);
        if (busy[t]) { if (hipEventSynchronize(ev[t]) != hipSuccess) return ZSMI_error_GENERIC; busy[t] = false; }
        if (!buf[t].reserve(n)) return ZSMI_error_memory_allocation;
        p = (T *)buf[t].p; return 0;
    }
    int sent(hipStream_t stream)
    {
        const int t = (int)((turns - 1u) & 1u);
        if (hipEventRecord(ev[t], stream) != hipSuccess) { (void)hipStreamSynchronize(stream); return ZSMI_error_GENERIC; }
        busy[t] = true; return 0;
    }
};

struct TimedLaunch { const char *name; hipEvent_t a, b; };
struct DecodePlan;

// The plan of a compress call (built in the compress section of zsmi_api.hip): chunks -> blocks and LZ units, on the host and in device
// memory.  Everything here is valid together, for the layout `key` states; the dictionary list for the choice dictKind / dictKey state.
struct CompressPlan {
    std::vector<uint64_t> key;           // n, then the srcOffsets, dstOffsets and srcSizes the plan was built from
    uint64_t blocks = 0; uint32_t maxChunkBlocks = 1;
    PinBuf hBlocks, hChunks, hUnits;
    DevBuf dBlocks, dChunks, dUnits, dDictList;
    // A run of units in chunk order inside one of the two device lists: before[i] (n + 1 entries) units of the run belong to chunks in
    // front of chunk i; the run starts at unit `base` of its list.
    //   dUnits:    [small: units of <= 64 KiB][big]
    //   dDictList: [whole: chunks of <= 64 KiB that have a dictionary, one prefixed unit each][tail: the other small units - tails of longer
    //              chunks, and a set call's chunks without a dictionary] - dictionary calls.  A set call's list is followed by the record
    //              index of every chunk (ZS_DICT_NONE: no dictionary) and of every unit of `whole`: chunkDict(), unitDict()
    struct Run { std::vector<uint32_t> before; uint32_t base = 0; } small, big, whole, tail;
    // Which dictionary list the plan holds: kDictNone; kDictAll, one dictionary for every chunk; kDictPerChunk, the choice dictKey states
    // (a chunk's record, ZS_DICT_NONE for none).  The list depends on the choice: the same layout with another choice builds it again, through
    // pinned buffers taken in turn (hDictList) - no wait for the stream
    enum { kDictNone, kDictAll, kDictPerChunk };
    int dictKind = kDictNone;
    std::vector<uint32_t> dictKey;
    TurnBufs hDictList;
    size_t chunkDictOff = 0, unitDictOff = 0;      // (bytes into dDictList; kDictPerChunk only)
    const uint32_t *chunkDict() const { return dictKind == kDictPerChunk ? (const uint32_t *)((const uint8_t *)dDictList.p + chunkDictOff) : nullptr; }
    const uint32_t *unitDict(uint32_t chunk0) const { return dictKind == kDictPerChunk ? (const uint32_t *)((const uint8_t *)dDictList.p + unitDictOff) + whole.before[chunk0] : nullptr; }
    struct Units { const ZsUnitDesc *d; uint32_t n; };
    struct Cut { uint32_t chunk1, nb, block0; };

    // dict: a dictionary call; dictIndex and memberHasDict: the call's selector's (ZsCDictSel below) - chunk i uses record dictIndex[i], and
    // none for ZS_DICT_NONE or a record that memberHasDict says stands for no dictionary
    int build(struct zsmi_ctx *c, const uint64_t *srcOffsets, const uint32_t *srcSizes, uint32_t n, const uint64_t *dstOffsets, bool dict,
              const uint32_t *dictIndex = nullptr, const uint8_t *memberHasDict = nullptr);
    Cut cut(uint32_t chunk0, uint32_t cap) const;                                      // the sub-batch of whole chunks from chunk0: at most cap blocks (one chunk at least)
    Units units(int kind, bool dict, uint32_t chunk0, uint32_t chunk1) const;          // kind: kUnitsPfx, kUnitsSmall, kUnitsBig
};

struct zsmi_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool ownStream = false;
    int checksumFlag = 0;                 // ZSMI_c_checksumFlag (zsmi_setParameter): the compress calls made on this context close their frames with a Content_Checksum
    uint32_t maxBlocksInFlight = 16384;   // ZSMI_BLOCKS_IN_FLIGHT: 64 KiB blocks per sub-batch (scratch ~0.6 MiB a block, reserved for what a call needs); 2 GiB of 128 KiB chunks: 8192: 86.5, 16384: 88.2, 32768: 89.4 GiB/s
    // compress workspace: the plan of the call's layout and the scratch of a sub-batch (its sizes: the compress section of zsmi_api.hip)
    CompressPlan plan;
    struct Scratch {
        DevBuf buf[kZsScratchCount];           // a buffer a row of ZS_SCRATCH_TABLE (zsmi_scratch.h), and a typed getter by the row's name
        #define X(name, T, perSlot, tail) T *name() const { return (T *)buf[kZsScratch_##name].p; }
        ZS_SCRATCH_TABLE(X)
        #undef X
        uint2 *distAsPackRecords() const { return (uint2 *)buf[kZsScratch_dist].p; }      // (lent to k_encode_sequences: zs_dist_lend_pack_records)
        bool reserve(uint32_t cap);            // cap: blocks of a sub-batch
    } scratch;
    // the resident compress calls' plan (zsmi_compressBatchResident[_usingCDictSet]; plan_kernels.hip writes it): per chunk of the call its ZsChunkDesc and
    // the unit sums in front of it, per sub-batch the live counts; the block and unit lists of ONE sub-batch, which every sub-batch reuses
    // (a set call - _usingCDictSet - besides: the record index of every chunk of the call and of every prefixed unit of the sub-batch)
    struct ResidentPlan { DevBuf dChunks, dBefore, dCounts, dBlocks, dUnits, dChunkDict, dUnitDict; } resident;
    DevBuf dDictImg;                       // a dictionary given as bytes (dictFromBytes): the candidate-table images of its prefix and, behind them, its one-entry table (a digested dictionary holds its own)
    DevBuf dDictRec; PinBuf hDictRec;      // the dictionary loader's record (ZsDictRecord: k_dict_load writes it, loadDict in zsmi_api.hip reads it back)
    int stopAfterWalk = 0;                 // ZSMI_STOP_AFTER_WALK (debug-hooks build, tools/walk_check.py): the entropy kernels are not launched
    int stopLit = 0, stopSeq = 0;          // timing aids of a -DZSMI_DEBUG_HOOKS build (ZSMI_STOP_LIT / ZSMI_STOP_SEQ): end a kernel after a stage; always 0 in the product
    // decompress workspace: the item list (on the host: pinned buffers taken in turn) and the scratch of a sub-batch, whose sizes for a
    // call's plan are stated once, in the decompress section (DecodeScratch::each)
    DevBuf dItems;
    TurnBufs hItems;
    struct DecodeScratch {
        DevBuf dPoolLit;                                                 // the general kernel's literal buffers: one per wavefront of its pool
        DevBuf dLitScratch, dFastDesc, dHufTabs, dSeqTabs, dSeqOut;      // the fast path's block slots: literals, descriptors, tables, sequences
        DevBuf dSeqLists;                                                // the general kernel's queue, the blocks of each table class, the items left (DecLists)
        uint8_t *poolLit() const { return (uint8_t *)dPoolLit.p; }
        uint8_t *litScratch() const { return (uint8_t *)dLitScratch.p; }
        ZsFastDesc *fastDesc() const { return (ZsFastDesc *)dFastDesc.p; }
        uint8_t *hufTabs() const { return (uint8_t *)dHufTabs.p; }
        uint8_t *seqTabs() const { return (uint8_t *)dSeqTabs.p; }
        ZsFastSeq *seqOut() const { return (ZsFastSeq *)dSeqOut.p; }
        uint32_t *seqLists() const { return (uint32_t *)dSeqLists.p; }
        template <class F> void each(const DecodePlan &p, F f);
        size_t held();
        bool reserve(const DecodePlan &p);
    } dec;
    bool decodeFast = true;              // ZSMI_DEC_FAST=0: general kernel only
    uint32_t maxItemsInFlight = 65536;   // ZSMI_ITEMS_IN_FLIGHT: items per decode launch (cut down when the scratch does not fit: planDecode).
                                         // Every decode kernel is a long dependent chain per item: a launch is one to three rounds of workgroups and its
                                         // last round is mostly tail, so big launches pay (16384 frames of 32 KiB: 82 GiB/s, 57344: 104 GiB/s)
    uint32_t cus = 256;                      // compute units of the device (rounds of workgroups a launch takes)
    uint32_t decodePool = 3072;              // wavefronts of the general decode kernel's pool (ZSMI_DEC_POOL): the chip holds 10 a CU x 256
    // staging for host-buffer calls
    DevBuf sSrc, sDst, sSizes, sDict, sPack, sPackOff;
    DevBuf dScan;                        // the tile sums of an offset scan (scanOffsets: zsmi_packFramesDevice, zsmi_layoutOutputsDevice, the seekable packer)
    PinBuf hPack;
    // seekable archives (seekable.hip): compressed frames at the running sum of their bounds before they are packed, per-frame words (frame
    // sizes, staging, packed and content offsets, compressed sizes, hashes, the error word; a read's status words, codes and lists), the decoded
    // bytes of the frames a read does not decode in place, and a call's lists (a read's; a compress call's sizes and staging offsets) on the
    // host: pinned buffers taken in turn, as hItems
    struct SeekScratch { DevBuf dStage, dMeta, dDec; TurnBufs hLists; } seek;
    // dictionary training (dict_train.hip): the samples back to back, sort keys, per-position hash / links (d = 6, 8), base and per-candidate
    // frequency tables, candidate contents and list, compressed sizes and frames of the scoring / statistics calls, stats + header scratch, the result
    struct TrainScratch {
        DevBuf dSamples, dGather, dEnds, dKeys, dKeysOut, dSortTmp, dInfo[2], dFreqBase, dFreq, dContent, dCand, dArena, dSizes, dMisc, dOut;
        PinBuf hCand;
    } train;
    // timing
    int timing = 0;                      // 1: events around every launch; 2: only around the dominant kernels (k_lz_walk*, k_dec_execute)
    std::vector<TimedLaunch> launches;
    std::vector<hipEvent_t> eventPool;

    // ---- the stream verbs: what host code says to the context's device and stream, each 0 or ZSMI_error_GENERIC (what every site returns
    // for a runtime call that fails).  Outside them hipSetDevice, hipMemcpyAsync, hipMemsetAsync, hipStreamSynchronize and hipGetLastError
    // stand in host code only in this file's TurnBufs::sent, zsmi_createCtx and zsmi_freeCtx, zsmi_getKernelTimes, the debug hooks,
    // destructors, and where zsmi_openSeekable clears a failed hipMalloc ----
    static int code(hipError_t e) { return e == hipSuccess ? 0 : ZSMI_error_GENERIC; }
    int bind() const { return code(hipSetDevice(device)); }
    int toDevice(void *d, const void *h, size_t n) const { return code(hipMemcpyAsync(d, h, n, hipMemcpyHostToDevice, stream)); }
    int toHost(void *h, const void *d, size_t n) const { return code(hipMemcpyAsync(h, d, n, hipMemcpyDeviceToHost, stream)); }
    int onDevice(void *d, const void *s, size_t n) const { return code(hipMemcpyAsync(d, s, n, hipMemcpyDeviceToDevice, stream)); }
    int fill(void *p, int byte, size_t n) const { return code(hipMemsetAsync(p, byte, n, stream)); }
    int wait() const { return code(hipStreamSynchronize(stream)); }
    int launched() const { return code(hipGetLastError()); }        // the tail of a call that queued kernels: a launch that failed
    // Idle before resize: pinned buffers that an earlier call's copy may still read are reserved (growing frees the block that copy reads)
    // and written only behind a wait for the stream.  One wait, then every {buffer, bytes} of the list
    int idleReserve(std::initializer_list<std::pair<PinBuf *, size_t>> wants) const
    {
        if (const int e = wait()) return e;
        for (const auto &w : wants) if (!w.first->reserve(w.second)) return ZSMI_error_memory_allocation;
        return 0;
    }
};

// A handle: a T allocated, then filled by build(T &) -> code, which makes the creator's checks in the creator's order; on a code it is
// deleted and null returned; the code goes to *err (may be null)
template <class T, class Build> static T *makeHandle(int *err, Build build)
{
    T *h = new (std::nothrow) T();
    const int code = h ? build(*h) : ZSMI_error_memory_allocation;
    if (code) { delete h; h = nullptr; }
    if (err) *err = code; return h;
}

// ---- the timed launch: events around what is queued while a Timed lives, when the context's timing asks for them.  An event that cannot
// be made is not handed out: the launch runs untimed ----
static hipEvent_t getEvent(zsmi_ctx *c)
{
    if (!c->eventPool.empty()) { hipEvent_t e = c->eventPool.back(); c->eventPool.pop_back(); return e; }
    hipEvent_t e = nullptr;
    return hipEventCreate(&e) == hipSuccess ? e : nullptr;
}
static inline bool dominantKernel(const char *name) { return strncmp(name, "k_lz_walk", 9) == 0 || strncmp(name, "k_dec_execute", 13) == 0; }
struct Timed {
    zsmi_ctx *c; TimedLaunch tl;
    Timed(zsmi_ctx *c, const char *name) : c(c), tl{ name, nullptr, nullptr }
    {
        if (!(c->timing == 1 || (c->timing == 2 && dominantKernel(name)))) return;
        hipEvent_t a = getEvent(c), b = getEvent(c);
        if (a && b) { tl.a = a; tl.b = b; (void)hipEventRecord(a, c->stream); } else for (hipEvent_t e : { a, b }) if (e) c->eventPool.push_back(e);
    }
    ~Timed() { if (tl.b) { (void)hipEventRecord(tl.b, c->stream); c->launches.push_back(tl); } }
};
#define LAUNCH(ctx, name, kernel, grid, block, lds, ...) do { Timed timed_(ctx, name); hipLaunchKernelGGL(kernel, grid, block, lds, (ctx)->stream, __VA_ARGS__); } while (0)

// ---- the batch calls in device memory (zsmi_api.hip: the compress and the decompress section state their arguments) ----
// A dictionary as its loader leaves it (the launch sequence sees none of this: a record says it all).  dBytes: its bytes in device memory;
// contentOff .. rep: what the device's dictionary loader found in them (loadDict in zsmi_api.hip copies its record: the host parses no
// dictionary; raw content: all of it, no ID, offsets {1, 4, 8}); dTables: a digested, formatted dictionary's entropy tables in encoder form
struct ZsCDictTables;
struct ZsCompressDict {
    const uint8_t *dBytes = nullptr;
    uint32_t contentOff = 0, contentSize = 0, dictID = 0, rep[3] = { 1, 4, 8 };
    const ZsCDictTables *dTables = nullptr;
};
// Which dictionary each chunk of a compress call gets: what every form of the call resolves to, and all the launch sequence knows of
// dictionaries (the decoder's ZsDictSel, for the encoder).  nullptr, or a selector without a table: the plain call.
struct ZsCDictSel {
    const ZsCDictEntry *dTable = nullptr;      // the records, in device memory: a digested dictionary's one-entry table, a set's, or the one dictFromBytes builds
    const uint32_t *dictIndex = nullptr;       // the call's choice (host, n entries): chunk i uses record dictIndex[i], ZS_DICT_NONE: none.  Null: every chunk uses record 0
    const uint8_t *memberHasDict = nullptr;    // which records stand for a dictionary (a set's empty member's does not).  Null: every one
    bool tables = false;                       // some record has entropy tables: the CD forms of the entropy kernels
};
// a dictionary given as bytes (none: the plain call) - content alone in device memory (the trainer), or a dictionary the loader reads, the call waiting for its
// record once (the _usingDict calls: in device memory, or in host memory and staged first) -> the selector of its one-entry table, built on the stream in c->dDictImg
enum DictBytes { kDictContent, kDictOnDevice, kDictOnHost };
static int dictFromBytes(zsmi_ctx *c, const void *dict, size_t dictSize, DictBytes kind, int level, uint32_t n, ZsCDictSel &sel);
// checksum: the frames carry a Content_Checksum (k_frame_checksum).  An argument, not the context's flag: the public calls pass c->checksumFlag,
// the one-shot _advanced calls their own, the dictionary trainer 0 - what it trains must not depend on the context's state
static int compressBatchDeviceImpl(zsmi_ctx *c, const void *dSrc, const uint64_t *srcOffsets, const uint32_t *srcSizes,
                                   uint32_t n, void *dDst, const uint64_t *dstOffsets, uint32_t *dDstSizes, int level,
                                   const ZsCDictSel *dict, int checksum, uint32_t *dStats = nullptr);
static int decompressBatchDeviceImpl(zsmi_ctx *c, const void *dSrc, const uint64_t *srcOffsets, const uint32_t *srcSizes,
                                     uint32_t n, void *dDst, const uint64_t *dstOffsets, const uint32_t *dstCaps, uint32_t *dDstSizes,
                                     const struct ZsDictSel *dict);
// what the features take of the two kinds of dictionary set (the structs: zsmi_api.hip).  resolveCDictSet: the checks of a set call's choice and
// its selector; nullIsTheOneMember: a null dictIndex with a set of exactly one member gives every chunk that member (the resident set call's
// rule) instead of GENERIC.  ddictSetSel: a DDict set's selector for a context of its device (a null set: none)
static int resolveCDictSet(const zsmi_ctx *c, const zsmi_cdictSet *set, const uint32_t *dictIndex, uint32_t n, int &level, ZsCDictSel &sel,
                           bool nullIsTheOneMember = false);
static int ddictSetSel(const zsmi_ctx *c, const zsmi_ddictSet *set, struct ZsDictSel &sel);
// ---- the bodies of the device-resident batch calls (zsmi_api.hip), for a feature whose descriptors are device memory too ----
// compress: the body of zsmi_compressBatchResident[_usingCDictSet], its arguments checked by the caller.  dict: null for the plain call; a set
// call's records and its choice in DEVICE memory.  residentCDictSet: what a zsmi_cdictSet * argument and a device choice ask of such a call -
// the NULL-index rule, then the set's device; 0 with level and dict set (a null set: the plain call at level 3, which takes no dict)
struct ResidentDict { const ZsCDictEntry *dTable; uint32_t members; bool tables; const uint32_t *dDictIndex; };
static int residentCDictSet(const zsmi_ctx *c, const zsmi_cdictSet *set, const uint32_t *dDictIndex, uint32_t n, int &level, ResidentDict &dict);
static int compressBatchResidentImpl(zsmi_ctx *c, const void *dSrc, const uint64_t *dSrcOffsets, const uint32_t *dSrcSizes, uint32_t n,
                                     uint32_t maxSrcSize, void *dDst, const uint64_t *dDstOffsets, uint32_t *dDstSizes, int level, const ResidentDict *dict);
// decompress: what a decode plan takes of a call's capacities - the largest, and how many items can hold more than one and more than two
// 64 KiB blocks - and the body of every decode call: the item list (ZsDecItem) is in c->dItems, queued or copied there on the stream by the caller
struct CapStats {
    uint32_t maxCap = 0, over1 = 0, over2 = 0;
    void add(uint32_t cap, uint32_t items = 1)
    {
        const uint32_t nb = (uint32_t)(((uint64_t)cap + ZS_BLOCK_MAX - 1) / ZS_BLOCK_MAX);
        maxCap = maxCap > cap ? maxCap : cap;
        if (nb > 1) over1 += items;
        if (nb > 2) over2 += items;
    }
};
static int decodeItems(zsmi_ctx *c, const void *dSrc, uint32_t n, void *dDst, const CapStats &caps, uint32_t *dDstSizes, const struct ZsDictSel *dict);
template <class Size>
static int scanOffsets(zsmi_ctx *c, const char *name, const Size *dSizes, const uint32_t *dStatus, uint32_t n, uint32_t align, uint32_t *dCaps, uint64_t *dOffsets);
// a context of the one-shot pool (zsmi_api.hip), given back when the handle goes
namespace { struct Borrowed { zsmi_ctx *c; Borrowed(); ~Borrowed(); }; }
