/*
 * ORACLE -- TEST INFRASTRUCTURE ONLY (see zso_decoder.c / zso_encoder.c headers).
 * Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may use it.
 */
#ifndef ZSO_ORACLE_H
#define ZSO_ORACLE_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* error codes: reference csharp/src/ZStdErrors.cs:61-90 */
enum {
    ZSO_no_error = 0, ZSO_GENERIC = 1, ZSO_prefix_unknown = 10, ZSO_version_unsupported = 12,
    ZSO_frameParameter_unsupported = 14, ZSO_frameParameter_windowTooLarge = 16,
    ZSO_corruption_detected = 20, ZSO_checksum_wrong = 22, ZSO_dictionary_corrupted = 30,
    ZSO_dictionary_wrong = 32, ZSO_dictionaryCreation_failed = 34, ZSO_parameter_unsupported = 40,
    ZSO_parameter_outOfBound = 42, ZSO_tableLog_tooLarge = 44, ZSO_maxSymbolValue_tooLarge = 46,
    ZSO_maxSymbolValue_tooSmall = 48, ZSO_stage_wrong = 60, ZSO_init_missing = 62,
    ZSO_memory_allocation = 64, ZSO_workSpace_tooSmall = 66, ZSO_dstSize_tooSmall = 70,
    ZSO_srcSize_wrong = 72, ZSO_frameIndex_tooLarge = 100, ZSO_seekableIO = 102, ZSO_maxCode = 120
};

/* oracle D : restatement of ZStdDecompress.Decompress / GetDecompressedSize */
size_t zso_decompress(void *dst, size_t dstCapacity, const void *src, size_t srcSize);
/* ZSTD_decompress_usingDict (ZStdDecompress.cs:2162): raw-content or formatted (magic 0xEC30A437) dictionary; NULL / 0 = none */
size_t zso_decompress_usingDict(void *dst, size_t dstCapacity, const void *src, size_t srcSize, const void *dict, size_t dictSize);
unsigned long long zso_getDecompressedSize(const void *src, size_t srcSize);
unsigned zso_isError(size_t code);
unsigned zso_errorCode(size_t code);
uint64_t zso_xxh64(const void *input, size_t len, uint64_t seed);
void zso_statsReset(void);
void zso_statsGet(uint32_t *out32);   /* 32 counters, see zso_decoder.c */
/* the dictionary trainer's 448 counters of the compressed blocks the calling thread decodes between the reset (which arms them) and the get
 * (which disarms them): literal bytes, LL, OF, ML codes (64 slots each).  Other threads' decodes, the batch drivers' among them, are not counted */
void zso_trainStatsReset(void);
void zso_trainStatsGet(uint32_t *out448);

/* oracle E : scalar CPU statement of this repo's block encoder (the algorithm the HIP kernels run) */
size_t zso_compressBound(size_t srcSize);
size_t zso_compress(void *dst, size_t dstCapacity, const void *src, size_t srcSize, int level);
/* the frame writer behind both: pre[0 .. pfx) the prefix of chunks of <= 64 KiB, dictID for the header (0: no field), rep the first
 * block's recent offsets (NULL: {1, 4, 8}) */
size_t zso_compressFrame(void *dst, size_t dstCapacity, const void *src, size_t srcSize, int level,
                         const void *pre, uint32_t pfx, uint32_t dictID, const uint32_t *rep);
/* with a dictionary (what zsmi_compress_usingDict does): raw-content or formatted; NULL / 0 bytes = zso_compress.
 * A dictionary oracle D refuses gives dictionary_corrupted (30). */
size_t zso_compress_usingDict(void *dst, size_t dstCapacity, const void *src, size_t srcSize, const void *dict, size_t dictSize, int level);
/* dictionary finalize, the scalar statement of zsmi_finalizeDictionary (zso_encoder.c).  zso_trainStats: the 448 counters over the samples
 * compressed with the content as a raw dictionary.  zso_finalizeDictionary: the dictionary's size, 0 if it cannot be made, or an error. */
size_t zso_trainStats(uint32_t *stats448, const void *content, size_t contentSize, const void *samples, const size_t *sizes, unsigned n, int level);
size_t zso_trainHuffDescription(void *dst256, const uint32_t *stats448, unsigned maxBits);
size_t zso_finalizeDictionary(void *dst, size_t cap, const void *content, size_t contentSize, const void *samples, const size_t *sizes,
                              unsigned n, int level, unsigned dictID);
/* oracle D's dictionary parse (insertDictionary): content offset, ID (0 for raw content), first block's recent offsets */
size_t zso_dictParams(const void *dict, size_t dictSize, size_t *contentOff, uint32_t *dictID, uint32_t rep[3]);
/* multi-threaded drivers used by bench.py's cpu_baseline leg and tests: n independent chunks */
int zso_compressBatch(void *dst, const uint64_t *dstOffsets, uint32_t *dstSizes,
                      const void *src, const uint64_t *srcOffsets, const uint32_t *srcSizes,
                      uint32_t n, int level, int nThreads);
/* the same with one dictionary for every chunk (zso_compress_usingDict) */
int zso_compressBatch_usingDict(void *dst, const uint64_t *dstOffsets, uint32_t *dstSizes,
                                const void *src, const uint64_t *srcOffsets, const uint32_t *srcSizes,
                                uint32_t n, int level, int nThreads, const void *dict, size_t dictSize);
int zso_decompressBatch(void *dst, const uint64_t *dstOffsets, const uint32_t *dstCaps, uint32_t *dstSizes,
                        const void *src, const uint64_t *srcOffsets, const uint32_t *srcSizes,
                        uint32_t n, int nThreads);
/* the same drivers over upstream libzstd loaded with dlopen (a labelled yardstick, NOT the reference); -2: no libzstd.so.1 */
int zso_libzstdCompressBatch(void *dst, const uint64_t *dstOffsets, uint32_t *dstSizes,
                             const void *src, const uint64_t *srcOffsets, const uint32_t *srcSizes,
                             uint32_t n, int level, int nThreads);
int zso_libzstdDecompressBatch(void *dst, const uint64_t *dstOffsets, const uint32_t *dstCaps, uint32_t *dstSizes,
                               const void *src, const uint64_t *srcOffsets, const uint32_t *srcSizes,
                               uint32_t n, int nThreads);
#ifdef __cplusplus
}
#endif
#endif
