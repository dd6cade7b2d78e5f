/*
 * zsmi.h -- C ABI of the MI355X-native Zstandard block codec (libzsmi.so).
 *
 * This is the drop-in boundary for the reference's public managed surface.  The reference
 * (epam/Zstandard) has no FFI of its own (pure C#/Java), so each entry point
 * below names the reference signature it replaces; a maintainer binds them with DllImport /
 * JNI as shown in INTEGRATION.md.  Plain pointers and sizes only; no torch types.
 *
 * Conventions kept from the reference:
 *   - results are sizes; errors are (size_t)-code with the codes of csharp/src/ZStdErrors.cs:61-90,
 *     tested with zsmi_isError() (ZStdErrors.cs:95-98: code > (size_t)-120);
 *   - nothing is retained past return for the one-shot calls (ZStdDecompress.cs:2174-2180);
 *   - one-shot calls are re-entrant; a zsmi_ctx must not be used from two threads at once.
 *
 * Every compute call runs on the GPU (HIP kernels for gfx950).  There is no CPU fallback:
 * if no device is usable the calls return ZSMI_error_GENERIC / a NULL context.
 */
#ifndef ZSMI_H
#define ZSMI_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* ---- error codes : csharp/src/ZStdErrors.cs:61-90 ---- */
enum {
    ZSMI_error_no_error = 0, ZSMI_error_GENERIC = 1, ZSMI_error_prefix_unknown = 10,
    ZSMI_error_version_unsupported = 12, ZSMI_error_frameParameter_unsupported = 14,
    ZSMI_error_frameParameter_windowTooLarge = 16, ZSMI_error_corruption_detected = 20,
    ZSMI_error_checksum_wrong = 22, ZSMI_error_dictionary_corrupted = 30, ZSMI_error_dictionary_wrong = 32,
    ZSMI_error_parameter_unsupported = 40, ZSMI_error_parameter_outOfBound = 42,
    ZSMI_error_tableLog_tooLarge = 44, ZSMI_error_maxSymbolValue_tooLarge = 46,
    ZSMI_error_maxSymbolValue_tooSmall = 48, ZSMI_error_stage_wrong = 60, ZSMI_error_init_missing = 62,
    ZSMI_error_memory_allocation = 64, ZSMI_error_workSpace_tooSmall = 66,
    ZSMI_error_dstSize_tooSmall = 70, ZSMI_error_srcSize_wrong = 72,
    ZSMI_error_frameIndex_tooLarge = 100, ZSMI_error_seekableIO = 102,       /* ZStdErrors.cs:87-88: the seekable format's codes */
    ZSMI_error_maxCode = 120
};

/* replaces: internal ZStdErrors.IsError (ZStdErrors.cs:95-98) */
unsigned zsmi_isError(size_t code);
/* replaces: commented upstream ZSTD_getErrorName (ZStd.cs:146-148) */
const char *zsmi_getErrorName(size_t code);
/* error code (0 if not an error) */
unsigned zsmi_getErrorCode(size_t code);

/* ------------------------------------------------------------------------------------------
 * One-shot calls on HOST buffers (the reference's public API shape).
 * ------------------------------------------------------------------------------------------ */

/* replaces: EPAM.Deltix.ZStd.ZStdDecompress.Decompress(byte[] dst, uint dstCapacity, byte[] src, uint srcSize)
 *           csharp/src/ZStdDecompress.cs:2182-2191  (and Java ZstdDecompressor.decompress, ZstdDecompressor.java:22)
 * Decodes every frame in src (concatenated and skippable frames included, ZStdDecompress.cs:2096-2160).
 * Returns the number of bytes written, or an error code. */
size_t zsmi_decompress(void *dst, size_t dstCapacity, const void *src, size_t srcSize);

/* replaces: ZSTD_decompress_usingDict(dctx, dst, dstCapacity, src, srcSize, dict, dictSize)  csharp/src/ZStdDecompress.cs:2162-2167
 * (internal in the reference: its public Decompress passes no dictionary, :2171).  dict: raw content, or a formatted dictionary
 * (magic 0xEC30A437: entropy tables + recent offsets + content, LoadEntropy :2378-2450); NULL / 0 = zsmi_decompress.
 * Errors as the reference: dictionary_corrupted (30), dictionary_wrong (32: the frame names another dictionary ID, :632-634). */
size_t zsmi_decompress_usingDict(void *dst, size_t dstCapacity, const void *src, size_t srcSize, const void *dict, size_t dictSize);

/* replaces: ZStdDecompress.GetDecompressedSize(byte[] src, uint srcSize)  csharp/src/ZStdDecompress.cs:590-622
 *           (Java ZstdDecompressor.getDecompressedSize, ZstdDecompressor.java:31)
 * Content size of the first frame; 0 if unknown, on error, or for a skippable frame. Host-only header parse. */
unsigned long long zsmi_getDecompressedSize(const void *src, size_t srcSize);

/* The size queries of a buffer of frames.  Host-only: they read the container's headers - frame headers, block headers, skippable
 * frames - and decode nothing; no device is needed.  They read only inside src[0 .. srcSize); srcSize may pass 4 GiB.
 * Every one is the answer of one container walker, the decoder's own frame / block loop without the decoding, so a frame is refused here
 * with the code the decoder would give it where the headers alone decide: prefix_unknown (10) for a magic that is neither a zstd frame's
 * nor a skippable frame's, frameParameter_unsupported (14) for the reserved header bit, frameParameter_windowTooLarge (16) for a window
 * log above 30, corruption_detected (20) for a block of the reserved type 3, srcSize_wrong (72) for a header, a block, a skippable frame
 * or a checksum that ends behind srcSize (the decoder says checksum_wrong for the last of these) and for bytes left over behind the last frame.
 *   ZSMI_CONTENTSIZE_UNKNOWN: a frame states no content size.   ZSMI_CONTENTSIZE_ERROR: any of the refusals above, or a sum beyond 64 bits. */
#define ZSMI_CONTENTSIZE_UNKNOWN (0ULL - 1)
#define ZSMI_CONTENTSIZE_ERROR   (0ULL - 2)
/* replaces: ZStdDecompress.GetFrameContentSize  csharp/src/ZStdDecompress.cs:518-531 (internal there).  What the header of the first frame
 * states: its Frame_Content_Size, or UNKNOWN; 0 for a skippable frame; ERROR for fewer than 5 bytes or a header that is refused or cut
 * short.  Only the header is read: the frame's blocks need not be there. */
unsigned long long zsmi_getFrameContentSize(const void *src, size_t srcSize);
/* replaces: commented upstream FindFrameCompressedSize  csharp/src/ZStdDecompress.cs:1957-2004.  The bytes the first frame of src takes -
 * header, blocks up to the last-block bit, checksum; a skippable frame: its 8 + Frame_Size bytes - or an error code (zsmi_isError).  What
 * follows the frame is not looked at, so the first frame of a concatenation gives its own length. */
size_t zsmi_findFrameCompressedSize(const void *src, size_t srcSize);
/* replaces: commented upstream FindDecompressedSize  csharp/src/ZStdDecompress.cs:538-580.  src must be exactly some number of frames, as
 * for zsmi_decompress: the sum of their stated content sizes (a skippable frame adds 0; no byte at all: 0), UNKNOWN, or ERROR. */
unsigned long long zsmi_findDecompressedSize(const void *src, size_t srcSize);
/* ZSTD_decompressBound (no counterpart in the reference): room that holds the content of every frame of src whether it states a size or
 * not - a frame's stated size, else its number of blocks x min(window size, 128 KiB) - summed; ZSMI_CONTENTSIZE_ERROR on error. */
unsigned long long zsmi_decompressBound(const void *src, size_t srcSize);

/* replaces: commented upstream declaration  size_t Compress(void* dst, size_t dstCapacity, void* src, size_t srcSize,
 *           int compressionLevel)  csharp/src/ZStd.cs:89-96   (the reference has no live compressor)
 * One frame for the whole input.  level <= 2: fast parameters, level >= 3: default parameters. */
size_t zsmi_compress(void *dst, size_t dstCapacity, const void *src, size_t srcSize, int level);

/* replaces: ZSTD_compress_usingDict(cctx, dst, dstCapacity, src, srcSize, dict, dictSize, level) (no cctx, as zsmi_compress)
 * One frame for the whole input, to be decoded with the same dictionary (zsmi_decompress_usingDict).  dict: raw content, or a formatted
 * dictionary (magic 0xEC30A437): its ID goes into the frame header, its recent offsets start the first block; its entropy tables are not
 * used.  Matches reach into the last 64 KiB of the content for inputs of <= 64 KiB (longer inputs: none).  NULL / 0 = zsmi_compress, byte
 * for byte.  Errors: dictionary_corrupted (30) for a formatted dictionary the decoder would refuse, before anything runs on the device. */
size_t zsmi_compress_usingDict(void *dst, size_t dstCapacity, const void *src, size_t srcSize, const void *dict, size_t dictSize, int level);

/* replaces: commented macro ZSTD_COMPRESSBOUND  csharp/src/ZStd.cs:144-145 (plus this codec's per-64 KiB block headers).  Holds the
 * largest frame this library writes for srcSize bytes, the 4 bytes of a content checksum included. */
size_t zsmi_compressBound(size_t srcSize);

/* The one-shot calls with a checksumFlag (ZSTD_c_checksumFlag).  checksumFlag != 0: the frame is the frame the call writes with 0, byte
 * for byte, but for bit 2 of the Frame_Header_Descriptor (byte 4), set, and 4 more bytes behind the last block: the low 32 bits of XXH64
 * (seed 0) of the content, little-endian.  A decoder (this one, libzstd) then answers checksum_wrong (22) for a frame whose content it cannot
 * restore.  zsmi_compress_advanced with NULL / 0 and checksumFlag 0 is zsmi_compress; with a dictionary, zsmi_compress_usingDict.
 * (zsmi_compress_usingCDict_advanced: declared with the digested dictionaries, below.) */
size_t zsmi_compress_advanced(void *dst, size_t dstCapacity, const void *src, size_t srcSize,
                              const void *dict, size_t dictSize, int level, int checksumFlag);

/* ------------------------------------------------------------------------------------------
 * Batch calls: n independent chunks <-> n frames, the data-parallel hot path (no analogue in the
 * reference).  Chunk i is src[srcOffsets[i] .. +srcSizes[i]); its result goes to
 * dst[dstOffsets[i] ..).  Offsets/sizes arrays are HOST memory; src/dst/dstSizes are DEVICE memory
 * in the *Device calls and host memory in the *Host calls (the device-resident calls, further down, take every array from device memory).
 * Per-chunk status: dstSizes[i] = bytes produced, or (uint32_t)-code on error (same codes as above).
 * ------------------------------------------------------------------------------------------ */
typedef struct zsmi_ctx zsmi_ctx;

/* device < 0: current HIP device.  stream: a hipStream_t (e.g. torch's current stream handle) or NULL
 * for a private stream.  Returns NULL if the device or its HIP runtime is unusable. */
zsmi_ctx *zsmi_createCtx(int device, void *hipStream);
void zsmi_freeCtx(zsmi_ctx *ctx);
/* block until everything queued on the context's stream has finished; returns 0 or an error code value */
int zsmi_sync(zsmi_ctx *ctx);

/* Sticky compression parameters of a context (ZSTD_CCtx_setParameter).  A value is read on the host when a compress call is made and governs
 * the work that call queues; calls queued before keep theirs.
 *   ZSMI_c_checksumFlag (0 or 1; default 0): every frame of the compress calls on this context - zsmi_compressBatchDevice / Host, their
 *   _usingDict, _usingCDict and _usingCDictSet forms, the frames of zsmi_compressSeekableDevice and zsmi_compressSeekableFrames* - carries a Content_Checksum: the frame the call
 *   writes with 0, byte for byte, but for bit 2 of byte 4, set, and the low 32 bits of XXH64 (seed 0) of the chunk behind its last block;
 *   dstSizes[i] grows by exactly 4 (zsmi_compressBound holds them).  A chunk whose dstSizes[i] is an error code is left as it is; an empty
 *   chunk gets its checksum too.  One more kernel a call (k_frame_checksum), whose time is that of hashing the call's largest chunk; with 0 the
 *   calls launch and write exactly what they did without the parameter.  Dictionary training never uses it.
 * Checked in this order - a NULL ctx: init_missing; a param that is none of the above: parameter_unsupported; a value outside the
 * parameter's range: parameter_outOfBound; zsmi_getParameter with a NULL value: GENERIC.  Return 0 or an error code value. */
enum { ZSMI_c_checksumFlag = 201 };                         /* ZSTD_c_checksumFlag's number */
int zsmi_setParameter(zsmi_ctx *ctx, int param, int value);
int zsmi_getParameter(const zsmi_ctx *ctx, int param, int *value);

/* Asynchronous on the context's stream.  dstOffsets[i] must leave zsmi_compressBound(srcSizes[i]) bytes.
 * Chunks may be any size >= 0; the codec cuts them in 64 KiB blocks inside one frame. */
int zsmi_compressBatchDevice(zsmi_ctx *ctx, const void *dSrc, const uint64_t *srcOffsets, const uint32_t *srcSizes,
                             uint32_t n, void *dDst, const uint64_t *dstOffsets, uint32_t *dDstSizes, int level);

/* The same with one dictionary for every chunk of the call (dDict: device memory; rules as zsmi_compress_usingDict: chunks of <= 64 KiB
 * may match into the last 64 KiB of its content).  The dictionary is loaded and checked on the device first and the few fields the host needs are
 * read back: the call waits for the context's stream once.  NULL / 0 = zsmi_compressBatchDevice. */
int zsmi_compressBatchDevice_usingDict(zsmi_ctx *ctx, const void *dSrc, const uint64_t *srcOffsets, const uint32_t *srcSizes,
                                       uint32_t n, void *dDst, const uint64_t *dstOffsets, uint32_t *dDstSizes, int level,
                                       const void *dDict, size_t dictSize);

/* ------------------------------------------------------------------------------------------
 * Digested dictionaries (ZSTD_createCDict / ZSTD_compress_usingCDict): a dictionary parsed, checked and laid out in device memory once,
 * then used by many calls.  Unlike the _usingDict calls, a call with a formatted CDict also uses the dictionary's entropy tables: the
 * first block of a frame may carry Treeless literals and Repeat_Mode sequence tables where those come out smaller, so its frames are
 * not byte for byte the _usingDict frames (with raw content they are).  They decode with the same dictionary.
 * ------------------------------------------------------------------------------------------ */
typedef struct zsmi_cdict zsmi_cdict;
/* dict: raw content or a formatted dictionary (host memory), parsed and checked as zsmi_compress_usingDict does (dictionary_corrupted
 * before anything runs).  The level is bound here.  Builds the device image on ctx's device and stream and waits for it, once.  NULL on
 * failure, with the code in *err if err != NULL.  A CDict is read-only after creation: any context of the same device may use it (a
 * context of another device: parameter_unsupported).  It must outlive the work queued with it: free it after zsmi_sync. */
zsmi_cdict *zsmi_createCDict(zsmi_ctx *ctx, const void *dict, size_t dictSize, int level, int *err);
void zsmi_freeCDict(zsmi_cdict *cd);                   /* NULL: nothing */
unsigned zsmi_getDictID_fromCDict(const zsmi_cdict *cd);   /* 0: raw content, or NULL */
size_t zsmi_sizeofCDict(const zsmi_cdict *cd);         /* device bytes held */
/* zsmi_compressBatchDevice with a digested dictionary for every chunk.  Queues its work and returns: no device-to-host copy, no wait for
 * the stream.  cd == NULL: zsmi_compressBatchDevice at level 3. */
int zsmi_compressBatchDevice_usingCDict(zsmi_ctx *ctx, const void *dSrc, const uint64_t *srcOffsets, const uint32_t *srcSizes,
                                        uint32_t n, void *dDst, const uint64_t *dstOffsets, uint32_t *dDstSizes, const zsmi_cdict *cd);
/* the host-buffer form, and the one-shot form (which runs on the current device) */
int zsmi_compressBatchHost_usingCDict(zsmi_ctx *ctx, const void *src, const uint64_t *srcOffsets, const uint32_t *srcSizes,
                                      uint32_t n, void *dst, const uint64_t *dstOffsets, uint32_t *dstSizes, const zsmi_cdict *cd);
size_t zsmi_compress_usingCDict(void *dst, size_t dstCapacity, const void *src, size_t srcSize, const zsmi_cdict *cd);
/* the one-shot form with a checksumFlag, as zsmi_compress_advanced; 0: zsmi_compress_usingCDict */
size_t zsmi_compress_usingCDict_advanced(void *dst, size_t dstCapacity, const void *src, size_t srcSize,
                                         const zsmi_cdict *cd, int checksumFlag);

/* ------------------------------------------------------------------------------------------
 * CDict sets: a read-only device table of digested compression dictionaries.  A compress call that takes a set gives chunk i the member
 * dictIndex[i] names - on the device, inside the kernels - so one call compresses a batch whose chunks use different dictionaries (the
 * frames a DDict set, below, decodes in one call).
 *
 * The contract: frame i is, byte for byte, the frame zsmi_compressBatchDevice_usingCDict gives chunk i with member dictIndex[i]; for
 * ZSMI_DICT_NONE or an empty member, the frame zsmi_compressBatchDevice gives at `level` - whatever the neighbouring chunks use.
 * What cds[] may be: formatted dictionaries, raw content, empty CDicts (no dictionary for the chunks that pick them), every one digested on
 * ctx's device for `level` (the images in a CDict are built for one level's parse).  Two members may carry one ID and one CDict may stand
 * at two indices: the caller names the dictionary, not the ID.  n may be 0.
 * Creation and lifetime: every check runs on the host before anything touches the device, in this order - a NULL ctx: init_missing; more
 * than 4096 members: parameter_outOfBound; NULL cds with n > 0: parameter_unsupported; then each entry of cds[] in turn: a NULL entry, one
 * of another device than ctx's, one of another level: parameter_unsupported.  The set copies nothing from its members: it holds one device
 * table of {prefix pointer and size, candidate-table images, entropy tables, recent offsets, dictID} in the order of cds[], uploaded on
 * ctx's stream and waited for, once.  The members must outlive the set, and the set the work queued with it (free it after zsmi_sync).
 * Read-only after creation: any context of the same device may use it.  NULL on failure, with the code in *err if err != NULL.
 * ------------------------------------------------------------------------------------------ */
#define ZSMI_DICT_NONE 0xFFFFFFFFu
typedef struct zsmi_cdictSet zsmi_cdictSet;
zsmi_cdictSet *zsmi_createCDictSet(zsmi_ctx *ctx, const zsmi_cdict *const *cds, uint32_t n, int level, int *err);
void zsmi_freeCDictSet(zsmi_cdictSet *set);                     /* NULL: nothing */
uint32_t zsmi_sizeofCDictSetMembers(const zsmi_cdictSet *set);  /* n; 0 for NULL */
/* zsmi_compressBatchDevice at the set's level; chunk i with member dictIndex[i] (a host array of n entries, as the offsets), or with no
 * dictionary for ZSMI_DICT_NONE.  Checked on the host first - on failure nothing is queued or written and the code is returned: a NULL ctx:
 * init_missing; a NULL dictIndex with n > 0: GENERIC; an index that is neither ZSMI_DICT_NONE nor below the number of members:
 * parameter_outOfBound; a set of another device: parameter_unsupported.  set == NULL: zsmi_compressBatchDevice at level 3 (dictIndex is not
 * read).  Like _usingCDict it only queues work: no device-to-host copy, no wait for the stream beyond the plan's own for a new layout. */
int zsmi_compressBatchDevice_usingCDictSet(zsmi_ctx *ctx, const void *dSrc, const uint64_t *srcOffsets, const uint32_t *srcSizes,
                                           uint32_t n, void *dDst, const uint64_t *dstOffsets, uint32_t *dDstSizes,
                                           const zsmi_cdictSet *set, const uint32_t *dictIndex);
/* the host-buffer form */
int zsmi_compressBatchHost_usingCDictSet(zsmi_ctx *ctx, const void *src, const uint64_t *srcOffsets, const uint32_t *srcSizes,
                                         uint32_t n, void *dst, const uint64_t *dstOffsets, uint32_t *dstSizes,
                                         const zsmi_cdictSet *set, const uint32_t *dictIndex);

/* Asynchronous on the context's stream.  Each frame i = src[srcOffsets[i] .. +srcSizes[i]) may hold several
 * concatenated / skippable frames (same rules as zsmi_decompress); dstCaps[i] is the room at dstOffsets[i]. */
int zsmi_decompressBatchDevice(zsmi_ctx *ctx, const void *dSrc, const uint64_t *srcOffsets, const uint32_t *srcSizes,
                               uint32_t n, void *dDst, const uint64_t *dstOffsets, const uint32_t *dstCaps,
                               uint32_t *dDstSizes);

/* The same with one dictionary for every frame of the call (dDict: device memory).  Frames decoded with a dictionary take the
 * general kernel (a digested dictionary, zsmi_createDDict below, puts them on the fast path). */
int zsmi_decompressBatchDevice_usingDict(zsmi_ctx *ctx, const void *dSrc, const uint64_t *srcOffsets, const uint32_t *srcSizes,
                                         uint32_t n, void *dDst, const uint64_t *dstOffsets, const uint32_t *dstCaps,
                                         uint32_t *dDstSizes, const void *dDict, size_t dictSize);

/* ------------------------------------------------------------------------------------------
 * Digested decode dictionaries (ZSTD_createDDict / ZSTD_decompress_usingDDict): a dictionary parsed, checked and laid out in device memory
 * once - its bytes, and for a formatted dictionary its entropy tables in the form the fast decode kernels read - then used by many calls.
 * Results per item (bytes, sizes, error codes) are those of the _usingDict calls with the same dictionary; frames that name the dictionary
 * (or none) decode on the fast path instead of the general kernel.
 * ------------------------------------------------------------------------------------------ */
typedef struct zsmi_ddict zsmi_ddict;
/* dict: raw content or a formatted dictionary (host memory), parsed and checked as zsmi_createCDict does (dictionary_corrupted in *err before
 * anything runs on the device; memory_allocation when memory runs out).  NULL / 0: an empty DDict, whose calls are the plain calls.  Builds
 * the device image on ctx's device and stream and waits for it, once.  NULL on failure, with the code in *err if err != NULL.  A DDict is
 * read-only after creation: any context of the same device may use it (a context of another device: parameter_unsupported).  It must outlive
 * the work queued with it: free it after zsmi_sync. */
zsmi_ddict *zsmi_createDDict(zsmi_ctx *ctx, const void *dict, size_t dictSize, int *err);
void zsmi_freeDDict(zsmi_ddict *dd);                   /* NULL: nothing */
unsigned zsmi_getDictID_fromDDict(const zsmi_ddict *dd);   /* 0: raw content, or NULL */
size_t zsmi_sizeofDDict(const zsmi_ddict *dd);         /* device bytes held */
/* zsmi_decompressBatchDevice with a digested dictionary for every frame.  Queues its work and returns: no device-to-host copy, no wait for
 * the stream.  dd == NULL: zsmi_decompressBatchDevice. */
int zsmi_decompressBatchDevice_usingDDict(zsmi_ctx *ctx, const void *dSrc, const uint64_t *srcOffsets, const uint32_t *srcSizes,
                                          uint32_t n, void *dDst, const uint64_t *dstOffsets, const uint32_t *dstCaps,
                                          uint32_t *dDstSizes, const zsmi_ddict *dd);
/* the host-buffer form, and the one-shot form (which runs on the current device; replaces ZSTD_decompress_usingDDict) */
int zsmi_decompressBatchHost_usingDDict(zsmi_ctx *ctx, const void *src, const uint64_t *srcOffsets, const uint32_t *srcSizes,
                                        uint32_t n, void *dst, const uint64_t *dstOffsets, const uint32_t *dstCaps,
                                        uint32_t *dstSizes, const zsmi_ddict *dd);
size_t zsmi_decompress_usingDDict(void *dst, size_t dstCapacity, const void *src, size_t srcSize, const zsmi_ddict *dd);

/* ------------------------------------------------------------------------------------------
 * DDict sets (ZSTD_d_refMultipleDDicts): a read-only device table of digested decode dictionaries.  A decode call that takes a set gives
 * every frame the dictionary its dictID names - on the device, inside the kernels - so one call decodes a batch whose frames name different
 * dictionaries, dictionary frames on the fast path.
 *
 * Which dictionary a frame gets:
 *  - a frame that names dictID X != 0: the member whose ID is X; no member has that ID: the item's result is dictionary_wrong (32);
 *  - a frame that names no dictionary (field absent or 0): `unnamed`; unnamed NULL or an empty DDict: no dictionary, as the plain call.
 *  This holds per frame, not per item: an item of several concatenated frames may name a different dictionary in each (such items are the
 *  general kernel's, as in every call).  Per item the results (bytes, sizes, error codes) are those of the _usingDDict call with the
 *  dictionary this rule picks.
 * What dds[] and unnamed may be:
 *  - members of dds[] are formatted dictionaries (their ID is not 0): a raw-content or empty DDict in dds[] is parameter_unsupported, raw
 *    content can only be `unnamed`;
 *  - a formatted `unnamed` also counts as a member under its own ID; two members with one ID are parameter_unsupported, this case included.
 *    So zsmi_decompress*_usingDDict(dd) is exactly the call with the set ({}, unnamed = dd);
 *  - n may be 0; more than 4096 members: parameter_outOfBound; a member (or unnamed) of another device than ctx's, a NULL entry, or NULL dds
 *    with n > 0: parameter_unsupported; a NULL ctx: init_missing.
 * Creation and lifetime: every check runs on the host before anything touches the device - ctx, n against 4096, dds, then each entry of dds[]
 * in turn (NULL, its device, formatted), unnamed's device, the IDs.  The set copies nothing from its members: it holds one device table of
 * {dictID, image pointer, bytes pointer, size}, sorted by ID, uploaded on ctx's stream and waited for, once.  The members must outlive the
 * set, and the set the work queued with it (free it after zsmi_sync).  Read-only after creation: any context of the same device may use it
 * (a context of another device: parameter_unsupported).  NULL on failure, with the code in *err if err != NULL.
 * ------------------------------------------------------------------------------------------ */
typedef struct zsmi_ddictSet zsmi_ddictSet;
zsmi_ddictSet *zsmi_createDDictSet(zsmi_ctx *ctx, const zsmi_ddict *const *dds, uint32_t n, const zsmi_ddict *unnamed, int *err);
void zsmi_freeDDictSet(zsmi_ddictSet *set);            /* NULL: nothing */
uint32_t zsmi_sizeofDDictSetMembers(const zsmi_ddictSet *set); /* members by ID: dds[] and a formatted unnamed (0 for NULL) */
/* zsmi_decompressBatchDevice with the set's dictionaries.  Like _usingDDict it only queues work: no device-to-host copy, no wait for the
 * stream.  set == NULL: zsmi_decompressBatchDevice. */
int zsmi_decompressBatchDevice_usingDDictSet(zsmi_ctx *ctx, const void *dSrc, const uint64_t *srcOffsets, const uint32_t *srcSizes,
                                             uint32_t n, void *dDst, const uint64_t *dstOffsets, const uint32_t *dstCaps,
                                             uint32_t *dDstSizes, const zsmi_ddictSet *set);
/* the host-buffer form, and the one-shot form (which runs on the current device) */
int zsmi_decompressBatchHost_usingDDictSet(zsmi_ctx *ctx, const void *src, const uint64_t *srcOffsets, const uint32_t *srcSizes,
                                           uint32_t n, void *dst, const uint64_t *dstOffsets, const uint32_t *dstCaps,
                                           uint32_t *dstSizes, const zsmi_ddictSet *set);
size_t zsmi_decompress_usingDDictSet(void *dst, size_t dstCapacity, const void *src, size_t srcSize, const zsmi_ddictSet *set);

/* Host-buffer forms: stage through device memory, run the device form, copy back, synchronise. */
int zsmi_compressBatchHost(zsmi_ctx *ctx, const void *src, const uint64_t *srcOffsets, const uint32_t *srcSizes,
                           uint32_t n, void *dst, const uint64_t *dstOffsets, uint32_t *dstSizes, int level);
int zsmi_compressBatchHost_usingDict(zsmi_ctx *ctx, const void *src, const uint64_t *srcOffsets, const uint32_t *srcSizes,
                                     uint32_t n, void *dst, const uint64_t *dstOffsets, uint32_t *dstSizes, int level,
                                     const void *dict, size_t dictSize);
int zsmi_decompressBatchHost(zsmi_ctx *ctx, const void *src, const uint64_t *srcOffsets, const uint32_t *srcSizes,
                             uint32_t n, void *dst, const uint64_t *dstOffsets, const uint32_t *dstCaps,
                             uint32_t *dstSizes);
int zsmi_decompressBatchHost_usingDict(zsmi_ctx *ctx, const void *src, const uint64_t *srcOffsets, const uint32_t *srcSizes,
                                       uint32_t n, void *dst, const uint64_t *dstOffsets, const uint32_t *dstCaps,
                                       uint32_t *dstSizes, const void *dict, size_t dictSize);

/* Pack frames that sit at dstOffsets[] (sizes dDstSizes[], device) into one contiguous run at dPacked;
 * dPackedOffsets[n+1] (device, uint64) receives the running offsets.  Asynchronous. */
int zsmi_packFramesDevice(zsmi_ctx *ctx, const void *dFrames, const uint64_t *dstOffsets, const uint32_t *dSizes,
                          uint32_t n, void *dPacked, uint64_t *dPackedOffsets);

/* ------------------------------------------------------------------------------------------
 * Device-resident decode: a batch whose descriptors - offsets, sizes, capacities - are DEVICE memory, as an earlier GPU step left them
 * (dDstSizes of a compress call, dPackedOffsets of zsmi_packFramesDevice, the frames some kernel of the caller's located).  The three
 * calls below only queue work on the context's stream: no device-to-host copy, no wait, and nothing of the host-array calls' pinned
 * staging is touched.  Chained - sizes, layout, decode - they decode frames nobody has looked at on the host.
 * ------------------------------------------------------------------------------------------ */
/* The size queries above for n items at once, on the device: item i is dSrc[dSrcOffsets[i] .. + dSrcSizes[i]), some number of frames.
 * dContentSizes[i]: zsmi_findDecompressedSize of the item; dBounds[i]: its zsmi_decompressBound (either array may be NULL);
 * dStatus[i]: 0 or the code that made them ZSMI_CONTENTSIZE_ERROR.  Every array is device memory; entries [0, n) are written and nothing
 * else; an item is read only inside its own bytes.  Checked on the host before anything is queued - a NULL ctx: init_missing; NULL dSrc,
 * dSrcOffsets, dSrcSizes or dStatus with n > 0: GENERIC.  n == 0 does nothing.  One kernel (k_frame_sizes), a lane an item. */
int zsmi_getFrameSizesBatchDevice(zsmi_ctx *ctx, const void *dSrc, const uint64_t *dSrcOffsets, const uint32_t *dSrcSizes, uint32_t n,
                                  uint64_t *dContentSizes, uint64_t *dBounds, uint32_t *dStatus);
/* Places for n outputs from their sizes (dContentSizes or dBounds of the call above), on the device.
 * dDstCaps[i] = dSizes[i] if dStatus[i] == 0 (a NULL dStatus: every one 0) and dSizes[i] <= 0xFFFFFF88, the largest size that is no error
 * code; 0 otherwise - an unknown size, a refused item, one too large for a batch item: the decode then reports the item's own error, or
 * dstSize_tooSmall (70).  dDstOffsets[0 .. n]: the exclusive running sum of the capacities, each rounded up to `align`; dDstOffsets[n] is
 * the room the outputs take.  align: a power of two in 1 .. 4096 (anything else: parameter_outOfBound); a NULL ctx: init_missing; a NULL
 * dDstOffsets, or NULL dSizes or dDstCaps with n > 0: GENERIC. */
int zsmi_layoutOutputsDevice(zsmi_ctx *ctx, const uint64_t *dSizes, const uint32_t *dStatus, uint32_t n, uint32_t align,
                             uint32_t *dDstCaps, uint64_t *dDstOffsets /* n + 1 */);
/* zsmi_decompressBatchDevice with its four descriptor arrays in device memory.  maxDstCap is the one thing the host is told: no item
 * gets more room than that, and the call's scratch is planned as for n items of maxDstCap bytes each (give the largest
 * capacity the batch can hold, not a loose ceiling).
 * The contract: item i's bytes, dDstSizes[i] and error code are those of zsmi_decompressBatchDevice - with a set,
 * zsmi_decompressBatchDevice_usingDDictSet - called with the same four arrays from the host and the capacities min(dDstCaps[i], maxDstCap).
 * set: NULL for the plain call; one DDict dd is the set ({}, unnamed = dd), so this entry point serves every dictionary form.
 * Checked on the host, in this order, before anything is queued - a NULL ctx: init_missing; a NULL dSrc, dDst, descriptor array or
 * dDstSizes with n > 0: GENERIC; a set of another device: parameter_unsupported.  n == 0 does nothing. */
int zsmi_decompressBatchResident(zsmi_ctx *ctx, const void *dSrc, const uint64_t *dSrcOffsets, const uint32_t *dSrcSizes, uint32_t n,
                                 void *dDst, const uint64_t *dDstOffsets, const uint32_t *dDstCaps, uint32_t maxDstCap,
                                 uint32_t *dDstSizes, const zsmi_ddictSet *set);

/* ------------------------------------------------------------------------------------------
 * Device-resident compress: the head of the same chain.  Chunk boundaries that a GPU step produced - records a kernel located, the rows
 * of a tensor, the dDstSizes / dPackedOffsets of this library - go into a compress call without a trip to the host: bounds, the layout
 * of the destinations (zsmi_layoutOutputsDevice above, over the bounds) and the compress call itself only queue work on the context's
 * stream.  Dictionaries come through zsmi_compressBatchResident_usingCDictSet: a CDict set and an index a chunk in device memory (one
 * digested dictionary: the set of one member).  What still plans on the host, from host arrays: the _usingDict forms with dictionary BYTES
 * (their loader reads a record back and waits), the fixed-size and host-array seekable compress calls and the dictionary trainer.  (Record
 * archives have a resident form of their own: zsmi_compressSeekableFramesResident*, zsmi_seekableReadFramesResident.)
 * ------------------------------------------------------------------------------------------ */
/* dBounds[i] = zsmi_compressBound(dSrcSizes[i]) for n sizes, on the device (both arrays device memory; entries [0, n) are written).
 * zsmi_layoutOutputsDevice(ctx, dBounds, NULL, n, align, dCaps, dDstOffsets) then places the frames.  A NULL ctx: init_missing; a NULL
 * array with n > 0: GENERIC; n == 0 does nothing. */
int zsmi_compressBoundsDevice(zsmi_ctx *ctx, const uint32_t *dSrcSizes, uint32_t n, uint64_t *dBounds);
/* zsmi_compressBatchDevice with its three descriptor arrays in device memory.  maxSrcSize is the one thing the host is told: the call's
 * sub-batches, grids and scratch are planned as for n chunks of maxSrcSize bytes each, and the chunk, block and unit lists are written by
 * kernels on the stream (give the largest size the batch can hold - a loose one costs sub-batches and idle workgroups,
 * never a wrong result or more scratch than the context's blocks in flight).
 * The contract:
 *  - frames: for every chunk with dSrcSizes[i] <= maxSrcSize, frame i and dDstSizes[i] are byte for byte those of zsmi_compressBatchDevice
 *    called with the same three arrays from the host at the same level, with the context's ZSMI_c_checksumFlag.  A chunk's frame does not
 *    depend on its neighbours, on maxSrcSize or on how the call was cut into sub-batches;
 *  - a chunk with dSrcSizes[i] > maxSrcSize: dDstSizes[i] = (uint32_t)-ZSMI_error_srcSize_wrong, at most zsmi_compressBound(0) bytes are
 *    written at its place, its neighbours are not affected;
 *  - no host traffic: the call only queues work - no device-to-host copy, no wait.  It keeps a plan of its own in device memory: the
 *    host-array calls' plan, pinned buffers and events are not touched, and a host-array call with a repeated layout still reuses its
 *    plan after a resident call;
 *  - writes: entries [0, n) of dDstSizes; bytes only inside [dDstOffsets[i], + zsmi_compressBound(dSrcSizes[i])).
 * Checked on the host, in this order, before anything is queued - a NULL ctx: init_missing; a NULL dSrc, dDst, descriptor array or
 * dDstSizes with n > 0: GENERIC.  n == 0 does nothing.  The dictionary form follows. */
int zsmi_compressBatchResident(zsmi_ctx *ctx, const void *dSrc, const uint64_t *dSrcOffsets, const uint32_t *dSrcSizes, uint32_t n,
                               uint32_t maxSrcSize, void *dDst, const uint64_t *dDstOffsets, uint32_t *dDstSizes, int level);
/* zsmi_compressBatchResident at the set's level, chunk i with member dDictIndex[i] of `set` (DEVICE memory, n entries, as the other
 * descriptors), or with no dictionary for ZSMI_DICT_NONE: the pipeline step that located the records picks each record's dictionary too,
 * and nothing of it comes to the host.  The plan kernels read the choice: a third, prefixed unit list and the record index of every chunk
 * and prefixed unit are written in device memory.
 * The contract:
 *  - frames: for every chunk with dSrcSizes[i] <= maxSrcSize and an index that is ZSMI_DICT_NONE or below the set's member count, frame i
 *    and dDstSizes[i] are byte for byte those of zsmi_compressBatchDevice_usingCDictSet called with the same arrays from the host, the same
 *    set and the context's ZSMI_c_checksumFlag (hence the _usingCDict call's frame with that member).  A chunk's frame does not depend on
 *    its neighbours, on maxSrcSize or on how the call was cut into sub-batches;
 *  - refusals the host cannot make: dSrcSizes[i] > maxSrcSize gives dDstSizes[i] = (uint32_t)-ZSMI_error_srcSize_wrong, as above; an index
 *    that is neither ZSMI_DICT_NONE nor below the member count gives (uint32_t)-ZSMI_error_parameter_outOfBound; both at once:
 *    srcSize_wrong.  Such a chunk is planned as an empty one without a dictionary: at most zsmi_compressBound(0) bytes are written at its
 *    place, its neighbours are not affected, and no list, grid, scratch or record lookup sees its size or its index;
 *  - dDictIndex == NULL with a set of exactly one member: every chunk uses member 0.  One CDict cd is the set {cd}, so this entry point
 *    serves the single digested dictionary too, as zsmi_decompressBatchResident does with a DDict.  NULL with any other member count and
 *    n > 0: GENERIC;
 *  - set == NULL: zsmi_compressBatchResident at level 3; dDictIndex is not read;
 *  - no host traffic: the call only queues work - no device-to-host copy, no wait, no pinned staging; the host-array calls' plan is not
 *    touched.  The host does not know whether any chunk picks a dictionary: the prefixed-unit kernels are always launched, over a unit a
 *    chunk, and leave on the device's live count;
 *  - writes: entries [0, n) of dDstSizes; bytes only inside [dDstOffsets[i], + zsmi_compressBound(dSrcSizes[i])).
 * Checked on the host, in this order, before anything is queued - a NULL ctx: init_missing; a NULL dSrc, dDst, descriptor array or
 * dDstSizes with n > 0: GENERIC; the dDictIndex rule above; a set of another device: parameter_unsupported.  n == 0 does nothing. */
int zsmi_compressBatchResident_usingCDictSet(zsmi_ctx *ctx, const void *dSrc, const uint64_t *dSrcOffsets, const uint32_t *dSrcSizes,
                                             uint32_t n, uint32_t maxSrcSize, void *dDst, const uint64_t *dDstOffsets, uint32_t *dDstSizes,
                                             const zsmi_cdictSet *set, const uint32_t *dDictIndex);

/* ------------------------------------------------------------------------------------------
 * Seekable archives (zstd's seekable format): independent frames, then a seek table in a skippable frame
 *   Skippable magic 0x184D2A5E | Frame_Size | n entries {Compressed_Size, Decompressed_Size[, Checksum]} | n | descriptor | 0x8F92EAB1
 * Any zstd decoder reads an archive as concatenated frames (zsmi_decompress included).  Frame i holds src[i F, min((i + 1) F, srcSize)),
 * compressed exactly as chunk i of zsmi_compressBatchDevice at the same level.  frameSize F: 0 = 64 KiB, else 1 .. 1 GiB
 * (parameter_outOfBound otherwise); more than 0x8000000 frames: frameIndex_tooLarge.  checksumFlag: each entry carries the low 32 bits of
 * XXH64 (seed 0) of the frame's content; it is the table's flag alone.  The frames themselves carry a Content_Checksum when the context's
 * ZSMI_c_checksumFlag is set (zsmi_compressSeekableDevice; the one-shot zsmi_compressSeekable writes none): Compressed_Size then includes the
 * 4 bytes, and zsmi_seekableBound holds them either way.  An empty input is an archive of 0 frames (the 17-byte table alone).
 * Reading checks the table before anything runs on the device: prefix_unknown (a magic is wrong), corruption_detected (reserved descriptor
 * bits, Frame_Size against n, compressed sizes that do not add up to the bytes in front of the table, a Compressed_Size of 0, a
 * Decompressed_Size over 1 GiB), frameIndex_tooLarge (more than 0x8000000 frames), parameter_outOfBound (offset past the content).
 * Only the frames that overlap the range are decoded; the first failing one in content order decides the result: its decoder error,
 * corruption_detected when its size is not its entry's, checksum_wrong when its checksum is not.
 * ------------------------------------------------------------------------------------------ */
/* room zsmi_compressSeekable* need: the frames' compress bounds plus the table (an error code for parameters they refuse) */
size_t zsmi_seekableBound(unsigned long long srcSize, uint32_t frameSize, int checksumFlag);
/* one-shot, host buffers (inputs over 4 GiB too).  Returns the archive's size or an error code */
size_t zsmi_compressSeekable(void *dst, size_t dstCapacity, const void *src, size_t srcSize, int level, uint32_t frameSize, int checksumFlag);
/* Device buffers, asynchronous on the context's stream.  Parameters and dstCapacity >= zsmi_seekableBound(...) are checked on the host first;
 * on failure nothing is queued and the code is returned.  *dArchiveSize (device memory) receives the archive's size, or (uint64_t)-code
 * if a frame failed.  The frames are compressed into context staging of about one bound of the input, then packed into dDst.
 * Writes only inside [dDst, dDst + dstCapacity). */
int zsmi_compressSeekableDevice(zsmi_ctx *ctx, const void *dSrc, uint64_t srcSize, void *dDst, uint64_t dstCapacity,
                                uint64_t *dArchiveSize, int level, uint32_t frameSize, int checksumFlag);
/* content bytes [offset, offset + dstCapacity), clipped at the content's end (offset == content size reads 0 bytes).  Only the compressed
 * bytes of the frames that overlap the range go to the device.  Returns the bytes written or an error code. */
size_t zsmi_decompressSeekable(void *dst, size_t dstCapacity, const void *src, size_t srcSize, unsigned long long offset);
/* Device buffers.  Reads back the table (the call waits for the context's stream), checks it, then queues the decode of the frames that
 * overlap [offset, offset + length) (clipped at the content's end) and returns; *written (host) receives the bytes the range holds,
 * *dStatus (device) 0 or the first failing frame's code.  Frames wholly inside the range decode straight into dDst, a partial first or
 * last frame into context scratch.  Writes only inside [dDst, dDst + *written).  (The one-range read of an archive opened for this call
 * alone: many reads of one archive belong to zsmi_openSeekableDevice and zsmi_seekableReadRangesDevice below.) */
int zsmi_decompressSeekableDevice(zsmi_ctx *ctx, const void *dSrc, uint64_t srcSize, uint64_t offset, uint64_t length,
                                  void *dDst, uint64_t *written, uint32_t *dStatus);
/* An opened archive (ZSTD_seekable_init*): the table read and checked once, then many reads through the handle.  A read is a batch of ranges:
 * every frame the batch touches is decoded once, however many ranges touch it.
 * zsmi_openSeekable: a host archive.  archive == NULL or size < 9: prefix_unknown; then the table's own rejections (as above); a NULL ctx:
 * init_missing, only after those - so a host archive's table can be judged without a device.  The frames' bytes (not the table) are copied to
 * device memory the handle owns, on ctx's device and stream, and waited for, once.
 * zsmi_openSeekableDevice: an archive in device memory, borrowed: it must outlive the handle.  A NULL ctx: init_missing, first (the table is in
 * device memory); the table is read back and the stream waited for, once, here.
 * Both keep a copy of the table in device memory for zsmi_seekableReadFramesResident and zsmi_seekableReadRecordsResident (24 bytes a frame,
 * and the frames' content offsets, 8 more; for a borrowed archive the handle's one
 * allocation), uploaded on ctx's stream: by zsmi_openSeekable ahead of its one wait; by zsmi_openSeekableDevice, which knows the table only
 * behind its parse's wait, with a wait of its own, so that a read on any context finds the table whole.
 * NULL on failure, with the code in *err if err != NULL.  A handle is read-only after creation: any context of the same device may use it (a
 * context of another device: parameter_unsupported).  It must outlive the work queued with it: close it after zsmi_sync. */
typedef struct zsmi_seekable zsmi_seekable;
zsmi_seekable *zsmi_openSeekable(zsmi_ctx *ctx, const void *archive, size_t size, int *err);
zsmi_seekable *zsmi_openSeekableDevice(zsmi_ctx *ctx, const void *dArchive, uint64_t size, int *err);
void zsmi_closeSeekable(zsmi_seekable *sk);                        /* NULL: nothing */
size_t zsmi_getNumFrames_fromSeekable(const zsmi_seekable *sk);    /* 0 for NULL */
unsigned long long zsmi_getContentSize_fromSeekable(const zsmi_seekable *sk);   /* 0 for NULL */
/* device bytes held for the ARCHIVE: the frames' bytes of a host archive; 0 for a borrowed archive, or NULL.  The handle's device copy of the
 * table (above) is not counted. */
size_t zsmi_sizeofSeekable(const zsmi_seekable *sk);
/* nRanges reads in one call: content bytes [offsets[r], offsets[r] + lengths[r]), clipped at the content's end, land at dDst + dstOffsets[r];
 * written[r] (host) receives the clipped length, dStatus[r] (device) 0 or the code of the first failing frame, in content order, among the
 * frames range r overlaps (an empty range overlaps none: 0).  offsets, lengths, dstOffsets and written are host arrays, as the batch calls'.
 * Checked on the host first - on failure nothing is queued or written and the code is returned: a NULL ctx: init_missing; a NULL sk, or a NULL
 * array with nRanges > 0: GENERIC; a handle of another device: parameter_unsupported; any offsets[r] past the content size:
 * parameter_outOfBound (offsets[r] == content size reads 0 bytes).  nRanges == 0 is a valid call that does nothing.
 * The call decodes the union of the frames its ranges overlap, each once (*framesDecoded, host, may be NULL: how many).  A frame wholly inside
 * the one range that overlaps it decodes straight to its place in dDst; every other one decodes into context scratch - the sum of the
 * Decompressed_Size of those frames, memory_allocation when that cannot be reserved - from where its pieces are copied out.  Queues its work
 * and returns: no device-to-host copy, no wait for the stream.  Range r writes only inside [dDst + dstOffsets[r], + written[r]), also when it
 * fails (its bytes are then unspecified); the ranges' places must not overlap. */
int zsmi_seekableReadRangesDevice(zsmi_ctx *ctx, const zsmi_seekable *sk, const uint64_t *offsets, const uint64_t *lengths, uint32_t nRanges,
                                  void *dDst, const uint64_t *dstOffsets, uint64_t *written, uint32_t *dStatus, uint32_t *framesDecoded);
/* The host-buffer form: the results land back to back in range order (range r starts at the sum of written[0 .. r)), statuses[r] (host) is
 * range r's code.  The same checks, then dstSize_tooSmall - before anything is queued - when the clipped lengths sum to more than
 * dstCapacity.  Staged through device memory, copied back, synchronised. */
int zsmi_seekableReadRangesHost(zsmi_ctx *ctx, const zsmi_seekable *sk, const uint64_t *offsets, const uint64_t *lengths, uint32_t nRanges,
                                void *dst, size_t dstCapacity, uint64_t *written, uint32_t *statuses);
/* Record archives: the caller's frame boundaries, a dictionary per frame.  One frame per record (or per group the caller chooses), each
 * compressed with the member of a CDict set the caller picks; any zstd decoder that holds the dictionaries reads the archive as concatenated
 * frames, and a handle opened with a DDict set reads it here, decoding exactly the frames asked for.
 * frameSizes and dictIndex are host arrays of n entries, as the batch calls'.  Frame i holds src[o_i, o_i + frameSizes[i]), o_i the running sum
 * of the sizes; the content is their concatenation and may pass 4 GiB.  A size of 0 makes a frame of an empty chunk that no read ever decodes.
 * Frame i and its size are byte for byte those that zsmi_compressBatchDevice (at `level`) or zsmi_compressBatchDevice_usingCDictSet (same set,
 * same choice) gives chunk i on this context, its ZSMI_c_checksumFlag included.  Entry i of the table is {Compressed_Size, frameSizes[i]
 * [, low 32 bits of XXH64 of chunk i]}; checksumFlag is the table's flag alone.  With frameSizes = F, F, .., rest the archive is byte for byte
 * what zsmi_compressSeekableDevice(frameSize = F) writes: that call is the fixed-size case of this path.
 * Dictionaries: set == NULL: the plain form at level 3 (as every _using call).  dictIndex[i]: a member's index, or ZSMI_DICT_NONE.  dictIndex ==
 * NULL with a set of exactly one member: every frame uses member 0 - one CDict cd is the set {cd}; with any other member count and n > 0: GENERIC.
 * Checked on the host, in this order, before anything is queued or written: a NULL ctx: init_missing; n > 0x8000000: frameIndex_tooLarge
 * (frameSizes is not read); a NULL frameSizes with n > 0: GENERIC; any frameSizes[i] > 1 GiB: parameter_outOfBound; the dictIndex rule above;
 * an index that is neither ZSMI_DICT_NONE nor below the member count: parameter_outOfBound; a set of another device: parameter_unsupported;
 * dstCapacity < zsmi_seekableFramesBound(...): dstSize_tooSmall; a NULL dArchiveSize or dDst (dst), or a NULL dSrc (src) with content: GENERIC. */
/* room the calls below need: the sum of zsmi_compressBound(frameSizes[i]) + 17 + n * (checksumFlag ? 12 : 8).  Host only, no device.  Its three
 * checks, in the order above.  Returns the size or an error code (zsmi_isError). */
size_t zsmi_seekableFramesBound(const uint32_t *frameSizes, uint32_t n, int checksumFlag);
/* Device buffers.  The calls only queue work: the per-frame lists go up through pinned buffers, nothing is copied back, nothing waited for.
 * *dArchiveSize (device memory) receives the archive's size, or (uint64_t)-code of the lowest failing frame.  The frames are compressed into
 * context staging of the sum of their bounds, then packed into dDst.  Writes only inside [dDst, dDst + dstCapacity).  n == 0 writes the
 * 17-byte table. */
int zsmi_compressSeekableFramesDevice(zsmi_ctx *ctx, const void *dSrc, const uint32_t *frameSizes, uint32_t n,
                                      void *dDst, uint64_t dstCapacity, uint64_t *dArchiveSize, int level, int checksumFlag);
int zsmi_compressSeekableFramesDevice_usingCDictSet(zsmi_ctx *ctx, const void *dSrc, const uint32_t *frameSizes, uint32_t n,
                                      void *dDst, uint64_t dstCapacity, uint64_t *dArchiveSize, int checksumFlag,
                                      const zsmi_cdictSet *set, const uint32_t *dictIndex);
/* host buffers: staged, run, copied back, synchronised; returns the archive's size or an error code */
size_t zsmi_compressSeekableFramesHost(zsmi_ctx *ctx, void *dst, size_t dstCapacity, const void *src, const uint32_t *frameSizes, uint32_t n,
                                       int level, int checksumFlag);
size_t zsmi_compressSeekableFramesHost_usingCDictSet(zsmi_ctx *ctx, void *dst, size_t dstCapacity, const void *src, const uint32_t *frameSizes,
                                       uint32_t n, int checksumFlag, const zsmi_cdictSet *set, const uint32_t *dictIndex);
/* zsmi_openSeekable / zsmi_openSeekableDevice whose reads decode with the set's dictionaries: every frame gets the dictionary its dictID names,
 * a frame that names none gets `unnamed` (the rule of zsmi_decompressBatchDevice_usingDDictSet); a frame that names an ID the set does not
 * hold makes its ranges dictionary_wrong.  set == NULL: the calls without a set.  The set is borrowed: it must outlive the handle, which must
 * outlive the work queued with it.  One DDict dd is the set ({}, unnamed = dd).
 * Checks as the calls without a set, then a set of another device than ctx's: parameter_unsupported.  The range reads above work unchanged on
 * such a handle; the one-shot and one-range calls (zsmi_decompressSeekable, zsmi_decompressSeekableDevice) have no dictionary form. */
zsmi_seekable *zsmi_openSeekable_usingDDictSet(zsmi_ctx *ctx, const void *archive, size_t size, const zsmi_ddictSet *set, int *err);
zsmi_seekable *zsmi_openSeekableDevice_usingDDictSet(zsmi_ctx *ctx, const void *dArchive, uint64_t size, const zsmi_ddictSet *set, int *err);
/* Streams of frames that carry NO table - the packed output of a batch compress call, a pzstd file, `cat a.zst b.zst`, a log of one frame a
 * record - opened for the same reads: the FRAME INDEX.  A table holds nothing the frames do not state themselves: the index has one entry a
 * frame in stream order, skippable frames included (Decompressed_Size 0, Compressed_Size 8 + the frame's length: entries without content), and is
 * defined by the size queries above.  From pos = 0, while pos < srcSize: c = zsmi_findFrameCompressedSize(src + pos, srcSize - pos), an error
 * code being the result; d = zsmi_getFrameContentSize(src + pos, ..); the entry is {pos, c, d}; pos += c.  Bytes left over behind the last
 * frame are srcSize_wrong, as that query answers them.  Behind the walker's own code, at the same frame, the table's field limits are
 * frameParameter_unsupported: a frame that states no content size, a content size above 1 GiB, a compressed size above 0xFFFFFFFF.  More
 * than 0x8000000 frames: frameIndex_tooLarge.  The first failing frame in stream order decides.  An empty stream is 0 frames.  srcSize > 0
 * behind a NULL src: srcSize_wrong.  Only headers are read: a damaged payload shows when its frame is read.  An archive that has a table
 * opens this way too and shows the table as a last entry of size 0.
 * zsmi_countFrames, zsmi_buildSeekTable: host only, no device - header parses like the size queries.  The table is the seekable format's
 * without checksums, 17 + 8 n bytes: src followed by these bytes is a seekable archive.  Returns the frames / the table's size, or an error
 * code; dstCapacity below the size (or a NULL dst): dstSize_tooSmall, behind the stream's own code. */
size_t zsmi_countFrames(const void *src, size_t srcSize);
size_t zsmi_buildSeekTable(void *dst, size_t dstCapacity, const void *src, size_t srcSize);
/* The handle is an ordinary zsmi_seekable whose table carries no checksums: every read call, zsmi_getFrameInfo_fromSeekable and the size
 * getters work on it unchanged, with the lifetime rules of the open calls above (zsmi_openSeekable* keep refusing a stream without a table).
 * One range over the whole content is the frame-parallel decode of a multi-frame stream.
 * zsmi_openFrames: a host stream, judged on the host before a context is asked for - the stream's code, then a NULL ctx: init_missing - then
 * copied to device memory the handle owns (zsmi_sizeofSeekable: srcSize) and waited for, once.
 * zsmi_openFramesDevice: a stream in device memory, borrowed.  A NULL ctx: init_missing, first.  The index is built on the device, with the
 * same entries and code as the host form: every place a magic number stands at is a candidate, found at memory bandwidth; each candidate's
 * frame is walked by a lane of its own; the frames are the candidates reachable from offset 0, found by pointer doubling - a magic number
 * inside a payload is never reached, even where it opens a whole valid frame.  Reads nothing outside [dSrc, dSrc + size).  The call waits for
 * the stream twice (the candidate count, which sizes its scratch - memory_allocation when that cannot be reserved; the result) and once more
 * for the table's device copy.
 * The _usingDDictSet forms: as zsmi_openSeekable_usingDDictSet. */
zsmi_seekable *zsmi_openFrames(zsmi_ctx *ctx, const void *src, size_t size, int *err);
zsmi_seekable *zsmi_openFramesDevice(zsmi_ctx *ctx, const void *dSrc, uint64_t size, int *err);
zsmi_seekable *zsmi_openFrames_usingDDictSet(zsmi_ctx *ctx, const void *src, size_t size, const zsmi_ddictSet *set, int *err);
zsmi_seekable *zsmi_openFramesDevice_usingDDictSet(zsmi_ctx *ctx, const void *dSrc, uint64_t size, const zsmi_ddictSet *set, int *err);
/* zsmi_seekableFrameInfo from the handle's parsed table (no re-parse); index >= frames: frameIndex_tooLarge; NULL sk: GENERIC */
int zsmi_getFrameInfo_fromSeekable(const zsmi_seekable *sk, uint32_t index, uint64_t *cOffset, uint64_t *dOffset, uint32_t *cSize, uint32_t *dSize);
/* records by number: exactly zsmi_seekableReadRangesDevice / Host with offsets[k] = content offset of frame frameIndex[k] and lengths[k] = its
 * Decompressed_Size - the same bytes, written[], statuses and framesDecoded.  Host checks as that call, with any frameIndex[k] >= frames:
 * frameIndex_tooLarge (nothing queued or written) in the place of parameter_outOfBound. */
int zsmi_seekableReadFramesDevice(zsmi_ctx *ctx, const zsmi_seekable *sk, const uint32_t *frameIndex, uint32_t nFrames,
                                  void *dDst, const uint64_t *dstOffsets, uint64_t *written, uint32_t *dStatus, uint32_t *framesDecoded);
int zsmi_seekableReadFramesHost(zsmi_ctx *ctx, const zsmi_seekable *sk, const uint32_t *frameIndex, uint32_t nFrames,
                                void *dst, size_t dstCapacity, uint64_t *written, uint32_t *statuses);
/* Record archives, device-resident: the frame sizes and dictionary indices of a write, the frame numbers of a read are DEVICE memory - what a
 * GPU step produced goes in without a trip to the host.  The three calls only queue work on the context's stream: no device-to-host copy, no
 * wait, no pinned staging (a context buffer may grow).
 * The host is told n, srcSize (the content bytes at dSrc) and maxFrameSize (no dFrameSizes[i] is above it: what the call's scratch is planned
 * for, as maxSrcSize of zsmi_compressBatchResident; a loose value changes no byte).
 * When every dFrameSizes[i] <= maxFrameSize and the sizes sum to srcSize, the archive and *dArchiveSize are byte for byte those of
 * zsmi_compressSeekableFramesDevice / _usingCDictSet with the same sizes and indices given from the host, on this context, with either table
 * flag.  Dictionaries: the NULL rules of zsmi_compressBatchResident_usingCDictSet - set == NULL: the plain form at level 3; dDictIndex == NULL
 * with a set of exactly one member: every frame uses member 0; with any other member count and n > 0: GENERIC.
 * What the host cannot judge goes to *dArchiveSize as (uint64_t)-code, the code of the lowest failing frame: a size above maxFrameSize, or a
 * frame whose content would end behind srcSize: srcSize_wrong (such a frame is planned as an empty one: nothing of dSrc outside
 * [0, srcSize) is read, nothing outside [dDst, dDst + dstCapacity) written, whatever the sizes say); an index that is neither ZSMI_DICT_NONE
 * nor below the member count: parameter_outOfBound (the size's refusal first); sizes that sum to less than srcSize, when no frame failed:
 * srcSize_wrong.
 * Checked on the host, in this order, before anything is queued: a NULL ctx: init_missing; n > 0x8000000: frameIndex_tooLarge; a NULL
 * dFrameSizes with n > 0: GENERIC; maxFrameSize > 1 GiB: parameter_outOfBound; the dDictIndex rule; a set of another device:
 * parameter_unsupported; what zsmi_seekableFramesResidentBound refuses, with its code; dstCapacity below that bound: dstSize_tooSmall; a NULL
 * dArchiveSize or dDst, or a NULL dSrc with srcSize > 0: GENERIC.  n == 0 with srcSize == 0 writes the 17-byte table. */
/* room for the archive of EVERY split of srcSize content bytes into n frames (the host never sees the sizes):
 *   srcSize + (srcSize >> 8) + 3 * (srcSize >> 16) + n * (64 + 3 + 18)  >=  the sum of zsmi_compressBound(s_i) over any sizes that sum to srcSize
 * plus the table's 17 + n * (checksumFlag ? 12 : 8); never below zsmi_seekableFramesBound of such sizes.  Host only, no device.
 * n > 0x8000000: frameIndex_tooLarge; srcSize > n * 1 GiB (no legal split; n == 0 with content): parameter_outOfBound. */
size_t zsmi_seekableFramesResidentBound(unsigned long long srcSize, uint32_t n, int checksumFlag);
int zsmi_compressSeekableFramesResident(zsmi_ctx *ctx, const void *dSrc, uint64_t srcSize, const uint32_t *dFrameSizes, uint32_t n,
                                        uint32_t maxFrameSize, void *dDst, uint64_t dstCapacity, uint64_t *dArchiveSize, int level, int checksumFlag);
int zsmi_compressSeekableFramesResident_usingCDictSet(zsmi_ctx *ctx, const void *dSrc, uint64_t srcSize, const uint32_t *dFrameSizes, uint32_t n,
                                        uint32_t maxFrameSize, void *dDst, uint64_t dstCapacity, uint64_t *dArchiveSize, int checksumFlag,
                                        const zsmi_cdictSet *set, const uint32_t *dDictIndex);
/* records by numbers in device memory.  dFrameIndex (nFrames entries), dDstOffsets (nFrames + 1), dWritten and dStatus (nFrames) are device
 * memory.  The call lays the outputs out itself: dDstOffsets[0 .. nFrames] is the exclusive running sum of the requested frames'
 * Decompressed_Size, each rounded up to align (the rule of zsmi_layoutOutputsDevice); request k's bytes land at dDst + dDstOffsets[k],
 * dWritten[k] is its frame's Decompressed_Size, dStatus[k] 0, the decoder's code, corruption_detected for a size that is not the entry's or
 * checksum_wrong for a checksum that is not the entry's.  Every request decodes straight to its place, with the handle's dictionaries; a frame
 * number named twice is decoded twice (zsmi_seekableReadFramesDevice decodes it once and copies).
 * Per request, where the host-array call refuses the whole call: a number at or above the frame count: dStatus[k] = frameIndex_tooLarge,
 * dWritten[k] = 0, no room taken; a place that would end behind dstCapacity: dStatus[k] = dstSize_tooSmall, nothing written for it (dWritten[k]
 * still states what it needs).  The other requests are untouched by either.  For numbers below the frame count and enough room, the bytes at
 * place k, dWritten[k] and dStatus[k] are those of zsmi_seekableReadFramesDevice with the same numbers and dstOffsets = the offsets this call
 * computes.  Writes only inside [dDst, dDst + dstCapacity).
 * Checked on the host, in this order: a NULL ctx: init_missing; a NULL sk or dDstOffsets, or another NULL array with nFrames > 0: GENERIC; a
 * handle of another device: parameter_unsupported; align not a power of two in 1 .. 4096: parameter_outOfBound; a NULL dDst with
 * dstCapacity > 0 and nFrames > 0: GENERIC.  nFrames == 0 writes dDstOffsets[0] = 0 and nothing else. */
int zsmi_seekableReadFramesResident(zsmi_ctx *ctx, const zsmi_seekable *sk, const uint32_t *dFrameIndex, uint32_t nFrames, uint32_t align,
                                    void *dDst, uint64_t dstCapacity, uint64_t *dDstOffsets, uint32_t *dWritten, uint32_t *dStatus);
/* The record splitter: the GPU step that locates the records.  A buffer of delimited records (lines, JSON lines, CSV rows) -> the frame
 * sizes of a record archive and, a frame, the number of its first record.  The rule (zstandard_amd/csrc/zsmi_split.h states it in code),
 * for src[0, srcSize), a delimiter byte delim, targetSize T (0: a frame a record) and maxFrameSize M:
 *  1. A record ends behind each byte equal to delim; bytes behind the last delimiter are a last record without one.  records: the
 *     delimiters, + 1 for such a tail.  (One byte: CRLF text splits at LF and the CR stays in the record.)
 *  2. A record of L <= M bytes is one piece; a longer one is cut at multiples of M from its own start: ceil(L / M) pieces.
 *     pieces <= records + srcSize / M.
 *  3. From pos = 0, while pos < srcSize: T == 0: the frame ends at the first piece end behind pos; T > 0: at the last piece end in
 *     (pos, pos + T], or, if there is none, at the first piece end behind pos (greedy: the whole pieces that fit in T, a longer piece
 *     alone).  No frame is above M; the sizes sum to srcSize.
 *  4. firstRecord[i] = the delimiters in src[0, start of frame i); firstRecord[n] = records.  THE LOOKUP: the frame record r starts in is
 *     the first i with firstRecord[i] >= r when that entry equals r, else i - 1.  A cut record always starts a frame.
 * Checked on the host, in this order: a NULL ctx (device calls): init_missing; delim outside 0..255: parameter_outOfBound; maxFrameSize 0
 * or above 1 GiB: parameter_outOfBound; targetSize > maxFrameSize: parameter_outOfBound; maxPieces > 0x80000000: parameter_outOfBound;
 * srcSize > 0 behind a NULL source: srcSize_wrong; a NULL dResult / dRecords, or a NULL dFrameSizes with maxPieces > 0: GENERIC.
 * srcSize == 0: 0 frames, 0 records, firstRecord[0] = 0.
 * zsmi_splitRecords: host only, no device - the rule's loop as written.  Returns the frame count or an error code.  frameSizes == NULL only
 * counts; more frames than capacity: dstSize_tooSmall, nothing written behind capacity.  firstRecord (capacity + 1 entries) and records
 * may be NULL.
 * zsmi_countRecordsDevice: *dRecords (device memory) = records.  Queues a count kernel and a sum: no wait, no host copy.
 * zsmi_splitRecordsDevice: only queues work on the context's stream - no device-to-host copy, no wait, no pinned staging (a context buffer
 * may grow: 12 bytes a 16 KiB of source and 40 bytes a piece of maxPieces; memory_allocation, before anything is queued, when that cannot
 * be reserved).  The host is told maxPieces (zsmi_countRecordsDevice's answer + srcSize / maxFrameSize always suffices): scratch, grids
 * and the rounds of pointer doubling are planned for it.  dFrameSizes: maxPieces entries; dFirstRecord: maxPieces + 1, may be NULL;
 * dResult: three device words - [0] the frame count n or (uint64_t)-code, [1] records, [2] pieces.  pieces > maxPieces: [0] =
 * -dstSize_tooSmall, no list is written, [1] and [2] are valid (exact while pieces <= 0x80000000) so that a second call can be sized.
 * Nothing is written outside the arrays as sized here, nothing read outside [dSrc, dSrc + srcSize).  When it fits, dFrameSizes[0, n),
 * dFirstRecord[0, n] and n are zsmi_splitRecords' for the same bytes. */
size_t zsmi_splitRecords(const void *src, size_t srcSize, int delim, uint32_t targetSize, uint32_t maxFrameSize,
                         uint32_t *frameSizes, uint64_t *firstRecord, size_t capacity, uint64_t *records);
int zsmi_countRecordsDevice(zsmi_ctx *ctx, const void *dSrc, uint64_t srcSize, int delim, uint64_t *dRecords);
int zsmi_splitRecordsDevice(zsmi_ctx *ctx, const void *dSrc, uint64_t srcSize, int delim, uint32_t targetSize, uint32_t maxFrameSize,
                            uint32_t maxPieces, uint32_t *dFrameSizes, uint64_t *dFirstRecord, uint64_t *dResult);
/* Records by number: the pipeline's last step.  A record archive's handle, the firstRecord array zsmi_splitRecordsDevice left in device
 * memory and record numbers in device memory -> the records' bytes, packed, with offsets and a status a request.  The two rules
 * (zstandard_amd/csrc/zsmi_records.h states them in code):
 *   FRAMES of record r < firstRecord[nFrames]: g = the last frame with firstRecord[g] <= r, lb = the first with firstRecord[lb] >= r, f = lb
 *     when firstRecord[lb] == r, else g (rule 4's lookup).  Frames f .. g hold the record - f < g only for a record that was cut - and
 *     skip = r - firstRecord[f] delimiters lie in front of it inside frame f.
 *   EXTENT, in the content of frames f .. g as one run: the record starts behind the skip-th delimiter (at 0 for skip 0) and ends behind
 *     the first delimiter at or behind its start, or at the run's end (the stream's tail record).  Fewer than skip delimiters:
 *     corruption_detected - the array or the delimiter does not belong to this archive.
 * zsmi_seekableReadRecordsResident only queues work on ctx's stream: no device-to-host copy, no wait, no pinned staging (context buffers may
 * grow: 80 bytes a request, 60 a frame read of maxFrameReads, the decoder's scratch for maxFrameReads items; memory_allocation, before
 * anything is queued, when that cannot be reserved).  All arrays are device memory: dFirstRecord nFrames + 1 entries; dRecordIndex, dWritten,
 * dStatus nRecords; dDstOffsets nRecords + 1; dResult four words.  The host is told nFrames (the handle's frame count), nRecords and
 * maxFrameReads, which lists, grids and the decode are planned for (nRecords suffices when no record exceeds the split's maxFrameSize).
 * Request k with dRecordIndex[k] < firstRecord[nFrames]: the record's bytes, its delimiter included, at dDst + dDstOffsets[k]; dWritten[k] its
 * length; dStatus[k] 0.  dDstOffsets is the exclusive running sum of the lengths, each rounded up to align (zsmi_layoutOutputsDevice's
 * rule).  The bytes are the text's, whatever targetSize and maxFrameSize the split had.
 * Followers: request k is a follower of k - 1 when both name frames and have the same (f, g); it reads no frame and uses its leader's decoded
 * bytes, so an ascending run of numbers decodes each frame once.  Any other repeat decodes again.  The leaders' frames are decoded into
 * dWork, end to end, with the handle's dictionaries and checked against their entries as zsmi_seekableReadFramesResident checks them: the
 * first failing frame of a request, in frame order, gives dStatus[k] of the leader and its followers (the decoder's code,
 * corruption_detected, checksum_wrong); such a request has dWritten[k] 0 and takes no room.
 * Per request, the others untouched: a number at or above firstRecord[nFrames]: frameIndex_tooLarge, dWritten 0, no room; a leader whose
 * list would end behind maxFrameReads or whose frames would end behind workCapacity: dstSize_tooSmall, dWritten 0, no room, its followers the
 * same (so is a request whose frames hold 0xFFFFFF00 bytes or more: no array of the splitter's asks for that); a place that would end
 * behind dstCapacity: dstSize_tooSmall, nothing written, dWritten[k] still the length.
 * dResult: [0] the requests with status 0, [1] the frame reads all leaders need, [2] the work bytes those reads need, [3]
 * dDstOffsets[nRecords]; [1] and [2] are exact whatever the caps are, so that a second call can be sized.
 * Whatever dFirstRecord holds, nothing is read outside the arrays as sized here and the handle's frames, nothing written outside
 * [dWork, +workCapacity), [dDst, +dstCapacity) and the arrays.
 * Checked on the host, in this order, before anything is queued: a NULL ctx: init_missing; a NULL sk, dDstOffsets or dResult, or another NULL
 * array with nRecords > 0: GENERIC; a handle of another device: parameter_unsupported; delim outside 0..255, align not a power of two in
 * 1 .. 4096, nFrames != the handle's frame count: parameter_outOfBound; maxFrameReads > 0x8000000: frameIndex_tooLarge; a NULL dDst or dWork
 * with a non-zero capacity and nRecords > 0: GENERIC.  (nRecords above 0x7FFFFFFF: memory_allocation.)  nRecords == 0 writes
 * dDstOffsets[0] = 0 and dResult = {0, 0, 0, 0}, and nothing else.
 * zsmi_seekableRecordsWorkBound: host only - dWork bytes that always suffice for maxFrameReads frame reads of this handle: maxFrameReads * its
 * largest Decompressed_Size (0 for a NULL handle).
 * zsmi_seekableReadRecordsHost: host arrays in, a host buffer out - the same checks on the host's arguments (dstOffsets: nRecords + 1 entries;
 * more than 0x8000000 frame reads: frameIndex_tooLarge), then uploads, the resident body with align 1 and a work buffer of the context's
 * sized from firstRecord by the same rule, the results copied down and waited for.  A record's length is dstOffsets[k + 1] - dstOffsets[k]. */
size_t zsmi_seekableRecordsWorkBound(const zsmi_seekable *sk, uint32_t maxFrameReads);
int zsmi_seekableReadRecordsResident(zsmi_ctx *ctx, const zsmi_seekable *sk, const uint64_t *dFirstRecord, uint32_t nFrames, int delim,
                                     const uint64_t *dRecordIndex, uint32_t nRecords, uint32_t maxFrameReads, uint32_t align,
                                     void *dWork, uint64_t workCapacity, void *dDst, uint64_t dstCapacity,
                                     uint64_t *dDstOffsets, uint64_t *dWritten, uint32_t *dStatus, uint64_t *dResult);
int zsmi_seekableReadRecordsHost(zsmi_ctx *ctx, const zsmi_seekable *sk, const uint64_t *firstRecord, uint32_t nFrames, int delim,
                                 const uint64_t *recordIndex, uint32_t nRecords, void *dst, size_t dstCapacity, uint64_t *dstOffsets, uint32_t *statuses);
/* Find records by content: the step that SELECTS records, in front of zsmi_seekableReadRecordsResident, which takes the answer as it
 * stands (dRecordIndex: ascending numbers decode each frame once).  A literal byte-pattern search; the rule
 * (zstandard_amd/csrc/zsmi_find.h states it in code), for text[0, len), a delimiter byte delim, a pattern of m bytes (1 <= m <= 256) none
 * of which equals delim, and a base B:
 *  1. An occurrence is a position p with p + m <= len and text[p, p + m) == pattern.  Overlapping occurrences all count.
 *  2. The record of p is B + the delimiters in text[0, p) (the splitter's rule 4).  The whole occurrence lies in that record.
 *  3. The answer is the distinct records that hold an occurrence, ascending; total: their count; matches: the occurrence count.
 * On an archive, text is the content of frames [firstFrame, firstFrame + frameCount) as one run and B = firstRecord[firstFrame]; an
 * occurrence that crosses the window's border is not found.  Frame f begins a record exactly when f == 0 or firstRecord[f] !=
 * firstRecord[f - 1], so windows cut at such frames together find what one window over all of them finds.
 * Not covered: patterns that hold the delimiter (several patterns a call and ignoring case: the query calls below; anchors and regular
 * expressions: the regular-expression calls below them).
 * pattern is HOST memory in every form - a parameter like delim, handed to the kernels by value: no upload, no pinned staging, no wait.
 * dResult / result: four words - [0] total or (uint64_t)-code, [1] the numbers written, min(total, capacity), [2] matches, [3] the bytes
 * scanned; [0] and [2] are exact whatever capacity is, so that a second call can be sized.  capacity == 0 with NULL dRecords only counts.
 * Nothing is written behind dRecords[capacity), nothing read outside [dSrc, dSrc + srcSize).
 * zsmi_findRecords: host only, no device - the rule's loop as written.  Returns total or an error code; *matches may be NULL.
 * zsmi_findRecordsDevice: only queues work on the context's stream - no device-to-host copy, no wait, no pinned staging (a context buffer
 * may grow: 40 bytes a 16 KiB of source; memory_allocation, before anything is queued, when that cannot be reserved).  dBase: one device
 * word, NULL: 0.  srcSize == 0: dResult = {0, 0, 0, 0}.  What it leaves is zsmi_findRecords' answer for the same bytes.
 * zsmi_seekableFindRecordsResident: the same contract; the window's frames are decoded end to end into dWork with the handle's dictionaries
 * and checked against their entries as zsmi_seekableReadFramesResident checks them (60 more bytes of context scratch a frame of the window,
 * the decoder's scratch), then searched, with B read on the device from dFirstRecord[firstFrame] (nFrames + 1 entries).  A frame that fails
 * (the decoder's code, corruption_detected, checksum_wrong): the first failing frame in frame order gives dResult = {(uint64_t)-code, 0, 0,
 * bytes} and dRecords is not written.  frameCount == 0: dResult = {0, 0, 0, 0}.
 * zsmi_seekableFindWorkBound: host only - the dWork bytes the window needs: its frames' content, from the handle's table; 0 for a NULL
 * handle or a window outside the archive.
 * zsmi_seekableFindRecordsHost: host arrays in and out - the same checks on the host's arguments, then firstRecord goes up, the resident
 * body runs with a work buffer of the context's, and the results come down behind one wait.
 * Checked on the host, in this order, before anything is queued: a NULL ctx (device calls): init_missing; a NULL sk, dResult, pattern or
 * dFirstRecord, or a NULL dRecords with capacity > 0: GENERIC; a handle of another device: parameter_unsupported; delim outside 0..255,
 * patternSize 0 or above 256, a pattern byte equal to delim, nFrames != the handle's frame count, firstFrame + frameCount > nFrames:
 * parameter_outOfBound; srcSize > 0 behind a NULL source: srcSize_wrong; a NULL dWork with a window that holds bytes: GENERIC; workCapacity
 * below the work bound: dstSize_tooSmall.  (A text of 2^31 tiles of 16 KiB or more: memory_allocation.) */
size_t zsmi_findRecords(const void *src, size_t srcSize, int delim, const void *pattern, uint32_t patternSize, uint64_t base,
                        uint64_t *records, size_t capacity, uint64_t *matches);
int zsmi_findRecordsDevice(zsmi_ctx *ctx, const void *dSrc, uint64_t srcSize, int delim, const void *pattern, uint32_t patternSize,
                           const uint64_t *dBase, uint64_t *dRecords, uint64_t capacity, uint64_t *dResult);
size_t zsmi_seekableFindWorkBound(const zsmi_seekable *sk, uint32_t firstFrame, uint32_t frameCount);
int zsmi_seekableFindRecordsResident(zsmi_ctx *ctx, const zsmi_seekable *sk, const uint64_t *dFirstRecord, uint32_t nFrames, int delim,
                                     const void *pattern, uint32_t patternSize, uint32_t firstFrame, uint32_t frameCount,
                                     void *dWork, uint64_t workCapacity, uint64_t *dRecords, uint64_t capacity, uint64_t *dResult);
int zsmi_seekableFindRecordsHost(zsmi_ctx *ctx, const zsmi_seekable *sk, const uint64_t *firstRecord, uint32_t nFrames, int delim,
                                 const void *pattern, uint32_t patternSize, uint32_t firstFrame, uint32_t frameCount,
                                 uint64_t *records, size_t capacity, uint64_t *result);
/* Find records by several patterns: any of them, all of them or none (grep -e .. -e .., grep -v), with or without ASCII case folding
 * (grep -i) - one search and, on an archive, one decode of the window, beside the single-pattern calls above, which are unchanged.  A
 * query is nPatterns patterns (1 .. 8; HOST memory, handed to the kernels by value like the single pattern) of 1 .. 256 bytes each and at
 * most 256 together, a mode and flags.  The rule (zstandard_amd/csrc/zsmi_findquery.h states it in code):
 *  1. fold(b) = b + 0x20 for b in 'A' .. 'Z' when ZSMI_FIND_IGNORE_CASE is set, b otherwise; bytes of 0x80 and above are never touched.
 *  2. An occurrence of pattern j is a position p with p + m_j <= len and fold(text[p + i]) == fold(P_j[i]) for every i.  Overlapping
 *     occurrences count, and so do occurrences of two patterns at one position.
 *  3. No pattern byte may satisfy fold(P_j[i]) == fold(delim); a text byte is a delimiter exactly when it equals delim, unfolded.
 *  4. The records are the splitter's: one ends behind each delimiter, bytes behind the last delimiter are a last record; numbered from B.
 *  5. H(r): the set of j with an occurrence of P_j in record r, bit j of an 8-bit word.
 *  6. The answer is the records whose H satisfies the mode, ascending - any: H != 0; all: every j < nPatterns; none: H == 0 (empty
 *     records included).  total: their count; matches: the occurrences summed over the patterns; hits[k]: H of the k-th record written.
 * With one pattern, `any` and no flag the answer is the single-pattern call's.  Not covered: patterns that hold the delimiter, Unicode
 * case folding, more than 8 patterns, occurrence counts a pattern (anchors and regular expressions: the regular-expression calls below).
 * The contract is that of the single-pattern calls, word for word: the four result words, capacity == 0 with NULL dRecords only counts,
 * nothing is written behind dRecords[capacity) or dHits[capacity) (a NULL dHits / hits: not wanted), nothing is read outside the source,
 * the device forms only queue work; on an archive the window, B, the failing-frame rule and zsmi_seekableFindWorkBound are as above.
 * Checked on the host in the order above with q where pattern stood (a NULL q: GENERIC), and of the query, where the single pattern's
 * checks stood: delim outside 0..255, nPatterns 0 or above 8, a mode above 2, unknown flag bits: parameter_outOfBound; then a pattern at
 * a time a NULL patterns[j]: GENERIC, patternSizes[j] 0 or above 256 or a sum above 256: parameter_outOfBound; then a pattern byte whose
 * fold is the delimiter's: parameter_outOfBound. */
#define ZSMI_FIND_MAX_PATTERNS 8u
#define ZSMI_FIND_IGNORE_CASE  1u                 /* flags */
enum { ZSMI_find_any = 0, ZSMI_find_all = 1, ZSMI_find_none = 2 };   /* mode */
typedef struct { uint32_t nPatterns, mode, flags; const void *patterns[8]; uint32_t patternSizes[8]; } zsmi_findQuery;
size_t zsmi_findRecordsQuery(const void *src, size_t srcSize, int delim, const zsmi_findQuery *q, uint64_t base,
                             uint64_t *records, uint8_t *hits, size_t capacity, uint64_t *matches);
int zsmi_findRecordsQueryDevice(zsmi_ctx *ctx, const void *dSrc, uint64_t srcSize, int delim, const zsmi_findQuery *q,
                                const uint64_t *dBase, uint64_t *dRecords, uint8_t *dHits, uint64_t capacity, uint64_t *dResult);
int zsmi_seekableFindQueryResident(zsmi_ctx *ctx, const zsmi_seekable *sk, const uint64_t *dFirstRecord, uint32_t nFrames, int delim,
                                   const zsmi_findQuery *q, uint32_t firstFrame, uint32_t frameCount, void *dWork, uint64_t workCapacity,
                                   uint64_t *dRecords, uint8_t *dHits, uint64_t capacity, uint64_t *dResult);
int zsmi_seekableFindQueryHost(zsmi_ctx *ctx, const zsmi_seekable *sk, const uint64_t *firstRecord, uint32_t nFrames, int delim,
                               const zsmi_findQuery *q, uint32_t firstFrame, uint32_t frameCount,
                               uint64_t *records, uint8_t *hits, size_t capacity, uint64_t *result);
/* Find records by regular expression (grep -E): a third search beside the two above, which are unchanged.  A pattern is compiled on the
 * HOST into a small DFA, the program - a POD the caller holds and the calls take by pointer from HOST memory, like a query; it reaches the
 * kernels by value.  The rule (zstandard_amd/csrc/zsmi_regex.h states it in code, with the syntax accepted and the refusals in full):
 *  1. A record - the splitter's: one ends behind each delimiter, bytes behind the last delimiter are a last record, empty records exist;
 *     numbered from B - is a byte string without its delimiter.  It MATCHES exactly when Python's
 *     re.compile(pattern, re.DOTALL | (re.IGNORECASE if ZSMI_FIND_IGNORE_CASE else 0)).search(record) succeeds.  Only existence counts.
 *  2. The delimiter is a parameter of the search, not of the program: a text byte equal to delim, unfolded, ends a record and is never
 *     fed to the program, so a `.`, a negated class or \s never sees it.
 *  3. The answer is the matching records, ascending; with ZSMI_REGEX_INVERT the others, empty records included.
 * The program: next[s * nClasses + classOf[b]] is the state behind byte b from state s; a record starts in `start` and matches when it
 * ends in a state s with bit s of `accept` set.  It is THE minimal complete DFA of the pattern, at most 64 states, 256 byte classes and
 * 3072 table entries.  zsmi_compileRegex: host only; 0, or the code of a refusal with *errorAt (may be NULL) the pattern offset at which it
 * was decided, and prog is not written - a NULL pattern or prog: GENERIC; patternSize 0 or unknown flag bits: parameter_outOfBound; a
 * recognised construct that is left out (^ or $ inside, \b \B \A \Z, backreferences, (? but (?:, lazy and possessive suffixes):
 * parameter_unsupported; malformed input: parameter_outOfBound; a program above the caps: parameter_outOfBound with errorAt = patternSize.
 * Accepted: literals (bytes of 0x80 and above too), \ before a non-alphanumeric byte, \t \n \r \f \v \xHH, \d \D \w \W \s \S (ASCII), `.`,
 * [...] and [^...] with ranges, ( ), (?: ), |, * + ?, {m} {m,} {m,n} with m <= n <= 255, ^ first and $ last in a top-level alternative.
 * Not covered: patterns that hold the delimiter, Unicode, word boundaries, backreferences, more than 64 states.
 * The calls: the contract of the query calls above, word for word, except the third result word - [0] total or (uint64_t)-code, [1]
 * min(total, capacity), [2] the RECORDS of the text searched (the delimiters, plus one for bytes behind the last; there is no occurrence
 * count for a regular expression), [3] the bytes scanned; [0] and [2] are exact whatever capacity is.  capacity == 0 with NULL dRecords
 * only counts; nothing is written behind dRecords[capacity), nothing read outside the source; the device forms only queue work (72 more
 * bytes of context scratch a 16 KiB of text than the other searches); srcSize == 0 and frameCount == 0: four zeros; on an archive the
 * window, B, the failing-frame rule and zsmi_seekableFindWorkBound are the existing ones, and a record the window's border cuts is judged
 * on the part inside the window.  Checked on the host in the order of the query calls with prog where q stood (a NULL prog: GENERIC) and,
 * where the query's checks stood: delim outside 0..255, unknown flag bits, nStates outside 1..64, nClasses outside 1..256, nStates *
 * nClasses above 3072, start >= nStates, a classOf[] >= nClasses, a used next[] >= nStates, an accept bit at or above nStates:
 * parameter_outOfBound - every call makes this check, so a damaged program never indexes outside a table. */
#define ZSMI_REGEX_MAX_STATES 64u
#define ZSMI_REGEX_MAX_TABLE  3072u               /* nStates * nClasses */
#define ZSMI_REGEX_INVERT     2u                  /* flags, beside ZSMI_FIND_IGNORE_CASE = 1 */
typedef struct { uint32_t nStates, nClasses, start, flags; uint64_t accept;
                 uint8_t classOf[256]; uint8_t next[ZSMI_REGEX_MAX_TABLE]; } zsmi_regexProgram;
int zsmi_compileRegex(const void *pattern, size_t patternSize, uint32_t flags, zsmi_regexProgram *prog, size_t *errorAt);
size_t zsmi_findRecordsRegex(const void *src, size_t srcSize, int delim, const zsmi_regexProgram *prog, uint64_t base,
                             uint64_t *records, size_t capacity, uint64_t *textRecords);
int zsmi_findRecordsRegexDevice(zsmi_ctx *ctx, const void *dSrc, uint64_t srcSize, int delim, const zsmi_regexProgram *prog,
                                const uint64_t *dBase, uint64_t *dRecords, uint64_t capacity, uint64_t *dResult);
int zsmi_seekableFindRegexResident(zsmi_ctx *ctx, const zsmi_seekable *sk, const uint64_t *dFirstRecord, uint32_t nFrames, int delim,
                                   const zsmi_regexProgram *prog, uint32_t firstFrame, uint32_t frameCount, void *dWork,
                                   uint64_t workCapacity, uint64_t *dRecords, uint64_t capacity, uint64_t *dResult);
int zsmi_seekableFindRegexHost(zsmi_ctx *ctx, const zsmi_seekable *sk, const uint64_t *firstRecord, uint32_t nFrames, int delim,
                               const zsmi_regexProgram *prog, uint32_t firstFrame, uint32_t frameCount,
                               uint64_t *records, size_t capacity, uint64_t *result);
/* The record index: firstRecord as part of the archive.  Every record call above takes firstRecord; these calls rebuild it from content and
 * frame borders, store it in the archive as a skippable frame, and load it from there - so that an archive written by one process, or by
 * another tool, can be read and searched by record.  The rule (zstandard_amd/csrc/zsmi_recindex.h states it in code): with content of
 * `size` bytes and frames at content offsets dOff[0 .. N], P(x) = the delimiters in content[0, x), + 1 when x == size, size > 0 and the
 * last byte is no delimiter; firstRecord[i] = P(dOff[i]).  For the splitter's frames that is its firstRecord; an empty frame at the
 * content's end gets `records`.  A frame is MISALIGNED when it holds a delimiter, its last byte is none and it does not end at `size`: the
 * lookup of the record calls is valid for an archive exactly when no frame is misaligned (fixed-size frames over text have many).
 * The index frame stands between the last content frame and the seek table and is the table's last entry {40 + 4 n, 0 [, 0x51D8E999]}:
 * every reader sees n + 1 frames whose last is empty.  Little-endian: u32 0x184D2A5D | u32 Frame_Size = 32 + 4 n | u32 0x58444952 | u8
 * version 1, u8 delim, u16 0 | u32 n | u32 0 | u64 records | u64 check | n x u32 count[i] = firstRecord[i + 1] - firstRecord[i];
 * check = sum of (count[i] + 1) (2 i + 1) 0x9E3779B185EBCA87, + records 0xC2B2AE3D27D4EB4F + delim, mod 2^64.
 * Host only, no device:
 * zsmi_recordIndexFrameSize: 40 + 4 n; n >= 0x8000000: frameIndex_tooLarge.
 * zsmi_writeRecordIndexFrame: firstRecord[0 .. n] -> the frame; its size or a code, in this order: delim outside 0..255:
 * parameter_outOfBound; n >= 0x8000000: frameIndex_tooLarge; a NULL dst or firstRecord: GENERIC; firstRecord[0] != 0, a descent or a
 * count above 32 bits: corruption_detected; dstCapacity below the size: dstSize_tooSmall.  Nothing is written on failure.
 * zsmi_readRecordIndexFrame: returns n with firstRecord[0 .. n] (firstRecord[n] = records; NULL: the frame is only judged) and *delim
 * (may be NULL), or a code, in this order: fewer than 40 bytes: srcSize_wrong; either magic: prefix_unknown; the version:
 * version_unsupported; reserved fields, Frame_Size against n: corruption_detected; fewer bytes than n asks for: srcSize_wrong; capacity
 * below n + 1: dstSize_tooSmall; the check, or counts that do not sum to records: corruption_detected.  Reads only src[0, 40 + 4 n).
 * zsmi_indexRecords: the rule over plain text, serially - the statement the device calls are held against.  Frame i holds
 * frameSizes[i] bytes.  firstRecord[0 .. n]; result (may be NULL) = {0, records, misaligned frames, delimiters}.  0 or a code: delim:
 * parameter_outOfBound; a NULL frameSizes with n > 0 or a NULL firstRecord: GENERIC; a NULL src with bytes, sizes that do not sum to
 * srcSize: srcSize_wrong.
 * zsmi_seekableAttachRecordIndex: a host archive in place - the table moves back, the index frame takes its place, its entry is added.
 * Returns the new size (archiveSize + 40 + 4 n + one entry) or a code, in this order: the table's own rejections (as the readers');
 * delim outside 0..255 or n not the table's frame count: parameter_outOfBound; a NULL firstRecord: GENERIC; firstRecord[0] != 0, a
 * descent or a count above its entry's Decompressed_Size: corruption_detected; an archive that already ends in an index frame:
 * parameter_unsupported; n + 1 > 0x8000000: frameIndex_tooLarge; capacity below the new size: dstSize_tooSmall.  A refused archive is
 * untouched.  Writes only inside [archive + the table's old place, archive + the new size).
 * Device, only queued - no copy to the host, no wait, no pinned staging; all scratch is the context's, reserved before anything is queued:
 * zsmi_indexRecordsDevice: the body of the rebuild over text in device memory.  dPlaces: uint64[n + 1], ascending, 0 first, `size` last
 * (the frames' borders in the text); atEnd: `size` is the content's end (the tail record counts, and a frame that ends there is not
 * misaligned).  Writes dFirstRecord[j] = *dBase + P(dPlaces[j]) for j = 1 .. n, and for j = 0 when dBase is NULL (base 0): windows of one
 * content taken in ascending order chain through the array with dBase = their entry 0.  dResult = {status, records in the text,
 * misaligned frames, delimiters}; status: parameter_outOfBound when dPlaces[0] != 0 or dPlaces[n] != size.  Places that do not ascend
 * leave their entries unspecified; nothing outside dFirstRecord[0 .. n] and dResult[0 .. 3] is written, nothing outside the text read.
 * Checked on the host, in this order: a NULL ctx: init_missing; a NULL dResult, dPlaces or dFirstRecord: GENERIC; delim outside 0..255:
 * parameter_outOfBound; n > 0x8000000: frameIndex_tooLarge; size > 0 behind a NULL dText: srcSize_wrong.
 * zsmi_seekableIndexRecordsResident: the rebuild on a window of an opened archive: its frames decoded end to end into dWork
 * (zsmi_seekableFindWorkBound sizes it), the body over the decoded places with dBase = dFirstRecord + firstFrame; the window at 0 writes
 * entry 0.  dFirstRecord holds the handle's frame count + 1 entries; the window writes [firstFrame (+ 1), firstFrame + frameCount].
 * dResult[0]: the window's first failing frame's code, as the find calls report it - when it is not 0 the window's entries and the other
 * three words are NOT to be trusted (they are written all the same).  frameCount == 0: dResult = {0, 0, 0, 0}.  Checked on the host, in
 * the find calls' order less the pattern: a NULL ctx: init_missing; a NULL sk, dResult or dFirstRecord: GENERIC; a handle of another
 * device: parameter_unsupported; delim outside 0..255, firstFrame + frameCount above the handle's frame count: parameter_outOfBound; a NULL
 * dWork with a window that holds bytes: GENERIC; workCapacity below the work bound: dstSize_tooSmall.
 * zsmi_seekableLoadRecordIndexResident: the handle's last entry, read from the handle's frames on the device and judged as
 * zsmi_readRecordIndexFrame judges it, every count held against the handle's table besides (a count above its entry's
 * Decompressed_Size: corruption_detected).  dResult = {status, records, delim, n}.  Status 0: dFirstRecord[0 .. N], N = n + 1 =
 * zsmi_getNumFrames_fromSeekable(sk), is the array the record calls take with nFrames = N; its last two entries are `records`.  A handle
 * with no frames, or whose last entry is no such frame: status prefix_unknown; with any status but 0 the array is untouched.  Checked on
 * the host: a NULL ctx: init_missing; a NULL sk, dFirstRecord or dResult: GENERIC; a handle of another device: parameter_unsupported.
 * zsmi_seekableAttachRecordIndexResident: zsmi_seekableAttachRecordIndex on an archive in device memory whose size is a device word -
 * the one zsmi_compressSeekableFramesResident left: it goes in as the archive's size and comes out as the new size or (uint64_t)-code; an
 * error word that comes in stays as it is and nothing is touched.  The host knows only n: the device reads the table's footer and
 * refuses, in the word and in the host form's order, what the host form refuses (a size above capacity: prefix_unknown).  The result is
 * byte for byte the host form's.  Checked on the host: a NULL ctx: init_missing; a NULL dArchive, dArchiveSize or dFirstRecord: GENERIC;
 * delim outside 0..255: parameter_outOfBound; n > 0x8000000: frameIndex_tooLarge.
 * Host arrays - the resident bodies with context staging, one wait: zsmi_seekableLoadRecordIndexHost (firstRecord[N + 1], written only
 * with status 0; result[4] as dResult) and zsmi_seekableIndexRecordsHost (the whole archive in windows of at most 256 MiB of content, cut
 * wherever the table allows; firstRecord[N + 1]; result = {the first failing frame's code, records, misaligned frames, delimiters}). */
size_t zsmi_recordIndexFrameSize(size_t n);
size_t zsmi_writeRecordIndexFrame(void *dst, size_t dstCapacity, const uint64_t *firstRecord, size_t n, int delim);
size_t zsmi_readRecordIndexFrame(const void *src, size_t srcSize, uint64_t *firstRecord, size_t capacity, int *delim);
int zsmi_indexRecords(const void *src, size_t srcSize, const uint32_t *frameSizes, size_t n, int delim, uint64_t *firstRecord, uint64_t *result);
size_t zsmi_seekableAttachRecordIndex(void *archive, size_t archiveSize, size_t capacity, const uint64_t *firstRecord, size_t n, int delim);
int zsmi_indexRecordsDevice(zsmi_ctx *ctx, const void *dText, uint64_t size, const uint64_t *dPlaces, uint32_t n, int delim, int atEnd,
                            const uint64_t *dBase, uint64_t *dFirstRecord, uint64_t *dResult);
int zsmi_seekableIndexRecordsResident(zsmi_ctx *ctx, const zsmi_seekable *sk, int delim, uint32_t firstFrame, uint32_t frameCount,
                                      void *dWork, uint64_t workCapacity, uint64_t *dFirstRecord, uint64_t *dResult);
int zsmi_seekableLoadRecordIndexResident(zsmi_ctx *ctx, const zsmi_seekable *sk, uint64_t *dFirstRecord, uint64_t *dResult);
int zsmi_seekableAttachRecordIndexResident(zsmi_ctx *ctx, void *dArchive, uint64_t capacity, uint64_t *dArchiveSize,
                                           const uint64_t *dFirstRecord, uint32_t n, int delim);
int zsmi_seekableLoadRecordIndexHost(zsmi_ctx *ctx, const zsmi_seekable *sk, uint64_t *firstRecord, uint64_t *result);
int zsmi_seekableIndexRecordsHost(zsmi_ctx *ctx, const zsmi_seekable *sk, int delim, uint64_t *firstRecord, uint64_t *result);
/* Frame filters: ask which frames of a record archive can hold a query's records BEFORE any frame is decoded - a small n-gram Bloom
 * filter a frame, all of them one skippable frame that the caller keeps BESIDE the archive, as a file or blob of its own.  The rule
 * (zstandard_amd/csrc/zsmi_filter.h states it in code, with the reason for rule 11): content of `size` bytes, frames at content offsets
 * dOff[0 .. N], a delimiter, a gram length g in {3, 4}, log2Bits L in 9 .. 16 - the bits a frame:
 *  1. fold(b) = b + 0x20 for 'A' .. 'Z', b otherwise: the query calls' fold, here ALWAYS applied - one filter serves searches with and
 *     without ZSMI_FIND_IGNORE_CASE.
 *  2. A gram of frame i is g consecutive bytes wholly inside frame i, none of which equals delim, unfolded.
 *  3. Its value v is the little-endian integer of its folded bytes;  4. its bits are h_k = (uint32_t)(v * C_k) >> (32 - L), C_0 = 0x9E3779B1,
 *     C_1 = 0x85EBCA77; bit h is bit h & 7 of byte h >> 3 of the frame's slot of 2^(L-3) bytes.
 *  5. A border x is clean when x == 0, x == size or content[x - 1] == delim.  6. A non-empty frame with a border that is not clean is
 *     SATURATED, its slot all ones (cut records and fixed-size frames over text produce them).  7. An empty frame's slot is all zeros,
 *     every other frame's the OR of its grams' bits.
 *  8. A pattern of m >= g bytes passes frame i when every bit of each of its m - g + 1 folded grams is set in slot i.  9. A pattern with
 *     m < g passes every frame.  10. A query passes a frame - any: some pattern passes; all: every pattern passes; none: every frame.  (The
 *     frame records no frame sizes and a frame without a gram has an empty frame's slot, so "every frame" includes the empty ones.)
 * 11. No false negatives: a record lies inside one clean frame or inside a run of saturated frames, so a frame that holds any part of a
 *     record satisfying an `any` or `all` query always passes.
 * The frame, little-endian: u32 0x184D2A5C | u32 Frame_Size = 32 + N 2^(L-3) | u32 0x52544C46 | u8 version 1, u8 delim, u8 g, u8 L | u32 N |
 * u32 0 | u64 size | u64 check | N slots;  check = sum over the slots' 64-bit words w_k of (w_k + 1) (2 k + 1) 0x9E3779B185EBCA87, + size
 * 0xC2B2AE3D27D4EB4F + delim + (g << 8) + (L << 16), mod 2^64.
 * Not covered: the single-pattern and regular-expression forms of the list search below; filters for regular expressions; `none` mode
 * (every frame passes the filter, and the list search refuses it);
 * the filter inside the archive (the record index frame is defined as the table's last entry); Bloom parameters other than two hashes.
 * Host only, no device - the serial statements the device forms are held against:
 * zsmi_frameFilterSize: 40 + n 2^(L-3); log2Bits outside 9..16: parameter_outOfBound; a Frame_Size beyond 32 bits: frameIndex_tooLarge.
 * zsmi_buildFrameFilter: text whose frame i holds frameSizes[i] bytes -> the frame; its size or a code, in this order: delim outside
 * 0..255, gram not 3 or 4, log2Bits outside 9..16: parameter_outOfBound; a Frame_Size beyond 32 bits: frameIndex_tooLarge; a NULL dst, a
 * NULL frameSizes with n > 0: GENERIC; a NULL src with bytes, sizes that do not sum to srcSize: srcSize_wrong; dstCapacity below the size:
 * dstSize_tooSmall.  Nothing is written on failure, nothing behind dst[size), nothing outside src[0, srcSize) is read.
 * zsmi_readFrameFilter: judges the frame and fills *info; 0 or a code, in this order: a NULL info: GENERIC; fewer than 40 bytes:
 * srcSize_wrong; either magic: prefix_unknown; the version: version_unsupported; delim / g / L out of range, the reserved field, a
 * Frame_Size that is not N's: corruption_detected; fewer bytes than N asks for: srcSize_wrong; the check: corruption_detected.
 * info.saturated counts the slots that are all ones.  Reads only src[0, 40 + N 2^(L-3)).
 * zsmi_filterFrames: the ascending numbers of the frames of [firstFrame, firstFrame + frameCount) that pass q -> frames[0, capacity);
 * result = {total, written = min(total, capacity), frames tested, all-ones slots among the total}; [0] and [3] are exact whatever
 * capacity is (capacity == 0 with NULL frames only counts).  0 or a code, in this order: a NULL q or result, a NULL frames with capacity:
 * GENERIC; the header's judgement as above, without the check (a caller that wants it calls zsmi_readFrameFilter once); the query's
 * checks against the FILTER's delimiter (zsmi_findRecordsQuery's); a window beyond N: parameter_outOfBound.  A list it writes never
 * separates a record's frames by a frame that holds bytes: window searches over the runs of the list - listed frames that follow one
 * another, or have only EMPTY frames between them - find each record of the window once.
 * Device, only queued - no copy to the host, no wait, no pinned staging; all scratch is the context's, reserved before anything is queued;
 * dFilter is 8-byte aligned (otherwise parameter_outOfBound, behind the other argument checks):
 * zsmi_buildFrameFilterDevice: the whole content in device memory, dPlaces as zsmi_indexRecordsDevice takes them (uint64[n + 1],
 * ascending, 0 first, `size` last).  Writes the complete frame, header and check included, byte for byte the host call's.  dResult =
 * {status, bytes written, all-ones slots, grams hashed}; status: parameter_outOfBound when dPlaces[0] != 0 or dPlaces[n] != size.  Places
 * that do not ascend leave their slots unspecified; nothing outside dFilter[0, 40 + n 2^(L-3)) and dResult[0 .. 3] is written, nothing
 * outside the text read.  Checked on the host, in this order: a NULL ctx: init_missing; a NULL dResult, dPlaces or dFilter: GENERIC;
 * delim, gram, log2Bits: parameter_outOfBound; Frame_Size: frameIndex_tooLarge; size > 0 behind a NULL dText: srcSize_wrong; capacity
 * below the frame: dstSize_tooSmall.
 * zsmi_seekableBuildFrameFilterResident: the archive's frames decoded end to end into dWork - the whole archive one window,
 * zsmi_seekableFindWorkBound(sk, 0, N) sizes it - then the body above with the handle's content offsets as places.  dResult[0]: the first
 * failing frame's code, as zsmi_seekableIndexRecordsResident reports it - when it is not 0 the frame is NOT to be trusted (it is written
 * all the same).  Checked on the host, in the rebuild's order: a NULL ctx: init_missing; a NULL sk, dResult or dFilter: GENERIC; a handle
 * of another device: parameter_unsupported; delim, gram, log2Bits: parameter_outOfBound; Frame_Size: frameIndex_tooLarge; a NULL dWork
 * with an archive that holds bytes: GENERIC; workCapacity below the bound, then capacity below the frame: dstSize_tooSmall.
 * zsmi_seekableBuildFrameFilterHost: the same into a host buffer behind one wait, a work buffer of the context's, in windows of at most
 * 256 MiB of content cut wherever the table allows; byte for byte the one-window result.  result[4] as dResult.
 * zsmi_checkFrameFilterDevice: zsmi_readFrameFilter's judgement on the device, check word included, one pass over the slots.  dResult
 * [8] = {status, N, delim, g, L, size, all-ones slots, 0}, the fields 0 with any status but 0.  Reads only inside dFilter[0, filterSize).
 * Checked on the host: a NULL ctx: init_missing; a NULL dFilter or dResult: GENERIC.
 * zsmi_filterFramesDevice: zsmi_filterFrames on a filter in device memory: dFrames uint32[capacity], dResult[4] as result - the host
 * call's answers for the same bytes.  g, L and the delimiter lie in the header the host never reads, so the patterns travel by value and
 * each workgroup hashes their grams once; the header's fields are judged on the device against filterSize, and what the host form
 * refuses of these bytes and this query puts (uint64_t)-code in dResult[0] and zeros behind it; nothing is written to dFrames then.
 * dResult[0] is a device word a later call can take as its frame count.  Checked on the host: a NULL ctx: init_missing; a NULL dFilter, q
 * or dResult, a NULL dFrames with capacity: GENERIC; the query's shape (nPatterns, mode, flags, pointers, sizes): as zsmi_findRecordsQuery.
 * zsmi_seekableFindQueryFramesResident: the query search over a LIST of frames in device memory - dFrames ascending, *dFrameCount a device
 * word, so dResult[0] of zsmi_filterFramesDevice can be passed straight in; the host is told only maxFrames (the entries dFrames holds).
 * The rule: a run is a maximal stretch of the list whose frames follow one another in the archive; the text searched is the runs'
 * content; an occurrence lies inside one run; its record is firstRecord[f] + the delimiters in front of it inside the frame f it starts
 * in; the answer is the satisfying records, ascending, each once a run.  A list the filter call wrote never separates a record's frames
 * by a frame that holds bytes, so there each record appears once, and dRecords, dHits, dResult[0] and [1] are what
 * zsmi_seekableFindQueryResident gives over the window the filter was asked about ([2], the occurrences, too for `any`; an `all` query
 * counts only the occurrences inside the listed frames).  dResult = {total, written, occurrences, content bytes decoded}.  Refused in
 * dResult[0] as (uint64_t)-code with nothing written to dRecords, in this order: *dFrameCount > maxFrames: dstSize_tooSmall, the work
 * bound of that many frames in dResult[3]; a list that does not ascend or names a frame >= nFrames: frameIndex_tooLarge; content (one
 * byte more a run that another follows) above workCapacity: dstSize_tooSmall, the bytes needed in dResult[3]; a frame that fails: its
 * code, as the window searches report it.  zsmi_seekableFindFramesWorkBound(sk, maxFrames) = maxFrames x (the handle's largest
 * Decompressed_Size + 1) always holds the list.  The text searched is min(workCapacity, that bound) bytes, filled with delimiters behind
 * the content.  Checked on the host, in the query calls' order: a NULL ctx: init_missing; a NULL sk, dResult, q, dFirstRecord,
 * dFrameCount, dFrames with maxFrames, dRecords with capacity: GENERIC; a handle of another device: parameter_unsupported; the query's
 * checks; mode `none`: parameter_unsupported; nFrames not the handle's: parameter_outOfBound; a NULL dWork with workCapacity: GENERIC.
 * zsmi_seekableFindQueryFramesHost: host arrays, one wait, a work buffer of the context's of the bound of frameCount frames. */
typedef struct { uint32_t nFrames, delim, gram, log2Bits; uint64_t size, saturated; } zsmi_frameFilterInfo;
size_t zsmi_seekableFindFramesWorkBound(const zsmi_seekable *sk, uint32_t maxFrames);
int zsmi_seekableFindQueryFramesResident(zsmi_ctx *ctx, const zsmi_seekable *sk, const uint64_t *dFirstRecord, uint32_t nFrames, int delim,
                                         const zsmi_findQuery *q, const uint32_t *dFrames, const uint64_t *dFrameCount, uint32_t maxFrames,
                                         void *dWork, uint64_t workCapacity, uint64_t *dRecords, uint8_t *dHits, uint64_t capacity,
                                         uint64_t *dResult);
int zsmi_seekableFindQueryFramesHost(zsmi_ctx *ctx, const zsmi_seekable *sk, const uint64_t *firstRecord, uint32_t nFrames, int delim,
                                     const zsmi_findQuery *q, const uint32_t *frames, uint32_t frameCount,
                                     uint64_t *records, uint8_t *hits, size_t capacity, uint64_t *result);
size_t zsmi_frameFilterSize(size_t n, unsigned log2Bits);
size_t zsmi_buildFrameFilter(void *dst, size_t dstCapacity, const void *src, size_t srcSize, const uint32_t *frameSizes, size_t n,
                             int delim, unsigned gram, unsigned log2Bits);
int zsmi_readFrameFilter(const void *src, size_t srcSize, zsmi_frameFilterInfo *info);
int zsmi_filterFrames(const void *filter, size_t filterSize, const zsmi_findQuery *q, uint32_t firstFrame, uint32_t frameCount,
                      uint32_t *frames, size_t capacity, uint64_t *result);
int zsmi_buildFrameFilterDevice(zsmi_ctx *ctx, const void *dText, uint64_t size, const uint64_t *dPlaces, uint32_t n, int delim,
                                unsigned gram, unsigned log2Bits, void *dFilter, uint64_t capacity, uint64_t *dResult);
int zsmi_seekableBuildFrameFilterResident(zsmi_ctx *ctx, const zsmi_seekable *sk, int delim, unsigned gram, unsigned log2Bits,
                                          void *dWork, uint64_t workCapacity, void *dFilter, uint64_t capacity, uint64_t *dResult);
int zsmi_seekableBuildFrameFilterHost(zsmi_ctx *ctx, const zsmi_seekable *sk, int delim, unsigned gram, unsigned log2Bits,
                                      void *filter, size_t capacity, uint64_t *result);
int zsmi_checkFrameFilterDevice(zsmi_ctx *ctx, const void *dFilter, uint64_t filterSize, uint64_t *dResult);
int zsmi_filterFramesDevice(zsmi_ctx *ctx, const void *dFilter, uint64_t filterSize, const zsmi_findQuery *q, uint32_t firstFrame,
                            uint32_t frameCount, uint32_t *dFrames, uint64_t capacity, uint64_t *dResult);
/* host only: the table at the archive's end (errors as above) */
size_t zsmi_seekableNumFrames(const void *src, size_t srcSize);
size_t zsmi_seekableContentSize(const void *src, size_t srcSize);
/* frame index's place: compressed offset and size, content offset and size.  Returns 0 or an error code value */
int zsmi_seekableFrameInfo(const void *src, size_t srcSize, uint32_t index, uint64_t *cOffset, uint64_t *dOffset,
                           uint32_t *cSize, uint32_t *dSize);

/* ------------------------------------------------------------------------------------------
 * Dictionary training (zstd's fastCover trainer and ZDICT_finalizeDictionary, on the GPU).  The result is a formatted dictionary
 * (magic 0xEC30A437 | dictID | Huffman description | OF, ML, LL NCounts | recent offsets 1, 4, 8 | content) that this library, oracle D and
 * upstream libzstd load.  Parameters as zdict.h of zstd 1.4.x; ZDICT_DICTSIZE_MIN = 256, ZDICT_CONTENTSIZE_MIN = 128.
 * Errors (nothing is written): dictCapacity < 256: dstSize_tooSmall; no samples, total sample bytes below 8 or of 4 GiB or more, a content
 * below 128 bytes: srcSize_wrong; d other than 6 / 8, k < d, k > dictCapacity or k > 65536, f outside 12..26, accel > 1, splitPoint outside
 * (0, 1]: parameter_outOfBound.
 * ------------------------------------------------------------------------------------------ */
typedef struct {
    unsigned k;          /* segment size; 0 = search (with steps) */
    unsigned d;          /* d-mer size, 6 or 8; 0 = search both (8 in zsmi_trainFromBuffer) */
    unsigned f;          /* log2 of the frequency table, 12..26; 0 = 20 */
    unsigned steps;      /* k candidates tried when searching: k = 50, 50 + s, ... <= 2000, s = max(1950 / steps, 1); 0 = 40 (4 in zsmi_trainFromBuffer) */
    unsigned accel;      /* 0 or 1 (others: parameter_outOfBound) */
    double   splitPoint; /* share of samples trained on while searching; 0 = 0.75; 1.0 = train and score on all */
    int      level;      /* compression level used to score candidates and gather the entropy statistics; 0 = 3 */
    unsigned dictID;     /* 0 = derived from the content as ZDICT does: XXH64(content) % ((1u<<31) - 32768) + 32768 */
} zsmi_fastCoverParams;

/* replaces: ZDICT_trainFromBuffer (fastCover, d = 8, steps = 4, split 0.75, level 3).  Returns the dictionary's size or an error code */
size_t zsmi_trainFromBuffer(void *dictBuffer, size_t dictCapacity, const void *samplesBuffer, const size_t *samplesSizes, unsigned nbSamples);
/* replaces: ZDICT_optimizeTrainFromBuffer_fastCover / ZDICT_trainFromBuffer_fastCover: k and d given = no search (trained on all samples);
 * otherwise each candidate (k, d) is trained on the first splitPoint share of the samples and scored by the size of the rest compressed by
 * this library at `level` with the candidate as raw content (ties: smaller k, then smaller d).  The chosen k, d are written back */
size_t zsmi_trainFromBuffer_fastCover(void *dictBuffer, size_t dictCapacity, const void *samplesBuffer, const size_t *samplesSizes,
                                      unsigned nbSamples, zsmi_fastCoverParams *params);
/* the same with the samples in device memory (host offsets / sizes, as the batch calls); the dictionary comes back to the host buffer
 * dictBuffer, its size to *dictSize; the call waits for the context's stream.  Returns 0 or an error code value */
int zsmi_trainFromDevice(zsmi_ctx *ctx, const void *dSamples, const uint64_t *sampleOffsets, const uint32_t *sampleSizes, uint32_t nbSamples,
                         void *dictBuffer, size_t dictCapacity, zsmi_fastCoverParams *params, size_t *dictSize);
/* replaces: ZDICT_finalizeDictionary: entropy tables from compressing the samples with `content` as raw content at `level` (0 = 3; every
 * count starts at 1), header, recent offsets {1, 4, 8}; the content's front is cut when header + content exceed dstCapacity */
size_t zsmi_finalizeDictionary(void *dst, size_t dstCapacity, const void *content, size_t contentSize, const void *samplesBuffer,
                               const size_t *samplesSizes, unsigned nbSamples, int level, unsigned dictID);
/* replaces: ZDICT_getDictID / ZSTD_getDictID_fromDict: host only, 0 for raw content or a buffer too short */
unsigned zsmi_getDictID(const void *dict, size_t dictSize);

/* ---- measurement hooks (bench.py): HIP-event timing of the kernels launched on the context's stream by the
 *      last batch call; one entry per kernel name, seconds are summed over launches.  Returns entries written.
 *      on = 1: events around every launch; on = 2: only around the dominant kernel of each direction (k_lz_walk*, k_dec_execute):
 *      ten event records a step between five short kernels are not free, the timed region of bench.py carries two. ---- */
typedef struct { char name[48]; double seconds; uint32_t launches; } zsmi_kernel_time;
int zsmi_enableKernelTiming(zsmi_ctx *ctx, int on);
int zsmi_getKernelTimes(zsmi_ctx *ctx, zsmi_kernel_time *out, int maxEntries);

/* device memory the context's decode buffers hold (bytes): the capacities of its scratch buffers, each with its reserve slack (1/8 + 4 KiB).
 * A call grows them to its items in flight and largest capacity; a later, much smaller call gives most of it back */
size_t zsmi_decodeScratchBytes(zsmi_ctx *ctx);

/* Releases the per-device contexts the one-shot calls (zsmi_compress / zsmi_decompress*) keep.  For embedders that unload the library: nothing
 * is released from an exit-time destructor (the HIP runtime may be gone by then); call this before dlclose.  No one-shot call may be running. */
void zsmi_shutdown(void);

/* library / device description, for logs */
const char *zsmi_versionString(void);

#ifdef __cplusplus
}
#endif
#endif
