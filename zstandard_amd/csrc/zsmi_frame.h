// THE readers of the zstd container headers: frame header, block header, literals section header, four-stream jump table.  The general
// kernel (decode_kernels.hip), k_dec_prep (decode_fast.hip) and the host's zsmi_getDecompressedSize read a header here and nowhere else, so
// an item gets the same answer whichever path takes it.  A reader takes bytes and returns a plain struct: no LDS, no lane logic; status is 0
// or the reference's error code (ZStdErrors.cs:61-90), reported by the caller in its own way.  (seqHeadersT, loadDictEntropy: decode_kernels.hip.)
#pragma once
#include "../../include/zsmi.h"   // the error codes
#include "zsmi_device.h"          // zs_load64
#include "zsmi_wave.h"            // rd16 / rd24 / rd32

// ---- frame header (ZSTD_getFrameHeader_advanced :421-499).  p[0 .. avail), avail >= 5, starts with the magic 0xFD2FB528 (magic and
//      skippable frames are the caller's).  behind: bytes the caller needs after the header (a block header: 3).  Refusals in the
//      reference's order: too few bytes, the reserved bit, a window log above 30 (ZSTD_WINDOWLOG_MAX_32, :468). ----
struct ZsFrameHeader { uint32_t status, headerSize, checksumFlag, singleSegment; uint32_t dictID; uint64_t windowSize, contentSize; };   // dictID 0: none named; contentSize ~0ull: not stated
__host__ __device__ __forceinline__ ZsFrameHeader zs_read_frame_header(const uint8_t *p, uint64_t avail, uint32_t behind)
{
    ZsFrameHeader h = {}; const uint32_t fhd = p[4]; const uint32_t dictIDCode = fhd & 3, fcsID = fhd >> 6;
    h.checksumFlag = (fhd >> 2) & 1; h.singleSegment = (fhd >> 5) & 1; h.contentSize = ~0ull;
    const uint32_t didSize = dictIDCode == 3 ? 4 : dictIDCode, fcsSize = fcsID == 0 ? 0 : (fcsID == 1 ? 2 : (fcsID == 2 ? 4 : 8));
    h.headerSize = 5 + !h.singleSegment + didSize + fcsSize + (h.singleSegment && !fcsID);
    if (avail < h.headerSize + behind) { h.status = ZSMI_error_srcSize_wrong; return h; }
    if (fhd & 0x08) { h.status = ZSMI_error_frameParameter_unsupported; return h; }
    uint32_t pos = 5;
    if (!h.singleSegment) {
        const uint32_t wl = p[pos++], windowLog = (wl >> 3) + 10;
        if (windowLog > 30) { h.status = ZSMI_error_frameParameter_windowTooLarge; return h; }
        h.windowSize = 1ull << windowLog; h.windowSize += (h.windowSize >> 3) * (wl & 7);
    }
    if (dictIDCode) h.dictID = dictIDCode == 1 ? (uint32_t)p[pos] : (dictIDCode == 2 ? rd16(p + pos) : rd32(p + pos));
    pos += didSize;
    if (fcsID == 0) { if (h.singleSegment) h.contentSize = p[pos]; }
    else h.contentSize = fcsID == 1 ? rd16(p + pos) + 256 : (fcsID == 2 ? rd32(p + pos) : zs_load64(p + pos));
    if (h.singleSegment) h.windowSize = h.contentSize;
    return h;
}
// ---- block header (GetcBlockSize :646-659): p[0 .. 3).  payload: the bytes the block takes behind its header (an RLE block: 1) ----
struct ZsBlockHeader { uint32_t last, type, size, payload; };     // type: 0 raw, 1 RLE, 2 compressed, 3 reserved
__host__ __device__ __forceinline__ ZsBlockHeader zs_read_block_header(const uint8_t *p)
{
    const uint32_t bh = rd24(p); ZsBlockHeader b; b.last = bh & 1; b.type = (bh >> 1) & 3; b.size = bh >> 3; b.payload = b.type == 1 ? 1u : b.size; return b;
}
// ---- the container walker: the loop of zs_decode_item (decode_kernels.hip; DecompressMultiFrame :2111-2160, DecompressFrame :2008-2067)
//      without decoding - what an item's headers alone say about it.  It reads only p[0 .. size).  Refusals are the decoder's, in its order,
//      with one difference: a checksum cut short is srcSize_wrong here (FindFrameCompressedSize :1996-1999), checksum_wrong there.
//      mode: the whole item (bytes left over are srcSize_wrong; 0 bytes: 0 frames, sizes 0); its first frame, a skippable one included
//      (consumed: its length); or the first frame's header alone (GetFrameContentSize :518-531: no block is looked at).
//      status: 0 or the code.  nFrames: zstd and skippable frames walked.  consumed: the bytes they take.
//      contentSize: the sum of the stated Frame_Content_Size values (a skippable frame adds 0); ZSMI_CONTENTSIZE_UNKNOWN when a frame states
//      none; ZSMI_CONTENTSIZE_ERROR on any refusal or when a sum passes 64 bits (FindDecompressedSize :538-580).
//      bound: ZSTD_decompressBound - a frame's stated size, else its blocks x min(window size, 128 KiB); ZSMI_CONTENTSIZE_ERROR as above. ----
struct ZsWalk { uint32_t status, nFrames; uint64_t contentSize, bound, consumed; };
enum { ZS_WALK_ITEM = 0, ZS_WALK_FIRST_FRAME = 1, ZS_WALK_FIRST_HEADER = 2 };
template <class Size>        // uint32_t: a batch item (the device); uint64_t: a host buffer, which may pass 4 GiB
__host__ __device__ __forceinline__ ZsWalk zs_walk(const uint8_t *p, Size size, int mode)
{
    ZsWalk w = {}; Size pos = 0; bool unknown = false, overflow = false;
    uint64_t content = 0, bound = 0;
    while (size - pos >= 5) {
        const uint8_t *ip = p + pos; const Size rem = size - pos;
        const uint32_t magic = rd32(ip);
        if (magic != 0xFD2FB528u) {
            if ((magic & 0xFFFFFFF0u) != 0x184D2A50u) { w.status = ZSMI_error_prefix_unknown; break; }
            if (rem < 8) { w.status = ZSMI_error_srcSize_wrong; break; }
            if (mode == ZS_WALK_FIRST_HEADER) { w.nFrames++; break; }
            const uint64_t skip = (uint64_t)rd32(ip + 4) + 8;
            if (rem < skip) { w.status = ZSMI_error_srcSize_wrong; break; }
            pos += (Size)skip; w.nFrames++;
            if (mode != ZS_WALK_ITEM) break;
            continue;
        }
        const ZsFrameHeader fh = zs_read_frame_header(ip, rem, mode == ZS_WALK_FIRST_HEADER ? 0u : 3u);
        if (fh.status) { w.status = fh.status; break; }
        pos += fh.headerSize;
        uint64_t blocks = 0;
        if (mode != ZS_WALK_FIRST_HEADER) {
            for (;;) {                                               // block loop :2033-2067
                if (size - pos < 3) { w.status = ZSMI_error_srcSize_wrong; break; }
                const ZsBlockHeader bh = zs_read_block_header(p + pos);
                if (bh.type == 3) { w.status = ZSMI_error_corruption_detected; break; }
                pos += 3;
                if (bh.payload > size - pos) { w.status = ZSMI_error_srcSize_wrong; break; }
                pos += bh.payload; blocks++;
                if (bh.last) break;
            }
            if (w.status) break;
            if (fh.checksumFlag) { if (size - pos < 4) { w.status = ZSMI_error_srcSize_wrong; break; } pos += 4; }
        }
        const bool stated = fh.contentSize != ~0ull;
        const uint64_t block = fh.windowSize < (1u << 17) ? fh.windowSize : (uint64_t)(1u << 17);
        const uint64_t fb = stated ? fh.contentSize : blocks * block;
        if (stated) { overflow |= content + fh.contentSize < content; content += fh.contentSize; } else unknown = true;
        overflow |= bound + fb < bound; bound += fb;
        w.nFrames++;
        if (mode != ZS_WALK_ITEM) break;
    }
    if (!w.status && mode == ZS_WALK_ITEM && pos != size) w.status = ZSMI_error_srcSize_wrong;
    w.consumed = pos;
    const bool bad = w.status || overflow;
    w.contentSize = bad ? ZSMI_CONTENTSIZE_ERROR : (unknown ? ZSMI_CONTENTSIZE_UNKNOWN : content);
    w.bound = bad ? ZSMI_CONTENTSIZE_ERROR : bound;
    return w;
}
__host__ __device__ __forceinline__ ZsWalk zs_walk_item(const uint8_t *p, uint32_t size) { return zs_walk<uint32_t>(p, size, ZS_WALK_ITEM); }

// ---- literals section header (DecodeLiteralsBlock :683-821) of a compressed block p[0 .. blockSize), blockSize >= 3 (MIN_CBLOCK_SIZE).
//      type: 0 raw, 1 RLE, 2 Huffman, 3 treeless.  compSize: the bytes behind the header (raw: regenSize, RLE: 1); single: one Huffman stream.
//      Refused here (corruption_detected) is what the header and blockSize alone decide: a Huffman section in a block below 5 bytes (:699), a section
//      that ends behind the block (:730, :776; for RLE literals the reference asks, for lhSize == 3, `srcSize < 4`, :808: with blockSize >= 3 that is
//      exactly headerSize + 1 > blockSize).  A caller's own limit on regenSize stays with it. ----
struct ZsLiteralsHeader { uint32_t status, type, headerSize, regenSize, compSize; bool single; };
__host__ __device__ __forceinline__ ZsLiteralsHeader zs_read_literals_header(const uint8_t *p, uint32_t blockSize)
{
    ZsLiteralsHeader h = {}; const uint32_t lhl = (p[0] >> 2) & 3; h.type = p[0] & 3;
    if (h.type >= 2) {
        if (blockSize < 5) { h.status = ZSMI_error_corruption_detected; return h; }
        const uint32_t lhc = rd32(p);
        if (lhl < 2) { h.single = !lhl; h.headerSize = 3; h.regenSize = (lhc >> 4) & 0x3FF; h.compSize = (lhc >> 14) & 0x3FF; }
        else if (lhl == 2) { h.headerSize = 4; h.regenSize = (lhc >> 4) & 0x3FFF; h.compSize = lhc >> 18; }
        else { h.headerSize = 5; h.regenSize = (lhc >> 4) & 0x3FFFF; h.compSize = (lhc >> 22) + ((uint32_t)p[4] << 10); }
    } else {
        if (lhl == 1) { h.headerSize = 2; h.regenSize = rd16(p) >> 4; }
        else if (lhl == 3) { h.headerSize = 3; h.regenSize = rd24(p) >> 4; }
        else { h.headerSize = 1; h.regenSize = p[0] >> 3; }
        h.compSize = h.type == 0 ? h.regenSize : 1u;
    }
    if (h.compSize + h.headerSize > blockSize) h.status = ZSMI_error_corruption_detected;
    return h;
}
// ---- the jump table of a four-stream Huffman section (HufDecompress.cs:269, :303): cs[0 .. csz) is the section behind its tree description.
//      len: the bytes of each stream, the first behind the table's 6; seg: the symbols of each of the first three streams, the fourth has the rest ----
struct ZsStreamSplit { uint32_t status, len[4], seg; };
__host__ __device__ __forceinline__ ZsStreamSplit zs_read_stream_split(const uint8_t *cs, uint32_t csz, uint32_t regenSize)
{
    ZsStreamSplit s = {}; s.status = ZSMI_error_corruption_detected;
    if (csz < 10) return s;
    s.len[0] = rd16(cs); s.len[1] = rd16(cs + 2); s.len[2] = rd16(cs + 4);
    const uint32_t used = s.len[0] + s.len[1] + s.len[2] + 6; if (used > csz) return s;
    s.len[3] = csz - used; s.seg = (regenSize + 3) / 4;
    if (3 * s.seg > regenSize) return s;
    s.status = 0; return s;
}
