// The scratch the compress and decode pipelines pass work through, between kernels: what a slot of each buffer holds, stated once for the
// host (sizes: zsmi_ctx::Scratch::reserve, zsmi_ctx::DecodeScratch::each, the debug hooks) and the kernels (one accessor per use: it takes
// the base pointer the kernel is handed and a slot, and gives the typed pointer).  No kernel, host line, tool or test states a stride of
// its own.  Where one stage keeps its data in another stage's buffer, the BORROWING is an accessor in the lender's section, named
// <lender>_lend_<what>, with a static_assert that the borrowed bytes fit.
#pragma once
#include "zsmi_device.h"
#include <type_traits>

// =============================================================================================
// compress: a slot = one 64 KiB block of the sub-batch (block index - the sub-batch's first); an LZ unit of two blocks owns two
// consecutive slots and addresses them from its first
// =============================================================================================
#define ZS_LITSEC_STRIDE  (ZS_BLOCK_MAX + 1024u)
#define ZS_SEQSEC_STRIDE  (ZS_BLOCK_MAX + 4096u)
#define ZS_STREAM_STRIDE  (24u * 1024u)          // per Huffman stream scratch: 16384 symbols * 11 bits = 22528 B max
#define ZS_CHAIN_CODES 16384u      // most sequences a block can hold (ZS_SEQ_MAX): elements per table in the chain scratch
static_assert(ZS_CHAIN_CODES == ZS_SEQ_MAX, "a chain table holds an element for every record a block's list can hold");
#define ZS_HDR_SLOT_WORDS 256u     // words a block's slot of hdrs takes: its ZsBlockHdr in front, the rest unused (the slot keeps the 1 KiB it
                                   // had as 64 range headers: tests/test_scratch_layout.py states every buffer's sizes)
static_assert(sizeof(ZsBlockHdr) <= ZS_HDR_SLOT_WORDS * sizeof(uint32_t), "a block's header fits its slot");

// per-block result of the two encode kernels, consumed by k_assemble_frames
struct ZsBlockMeta { uint32_t type;       // 0 raw, 1 rle, 2 literal + sequence sections present
                     uint32_t rleByte; uint32_t litSecSize; uint32_t seqSecSize;      // seqSecSize 0xFFFFFFFF: section failed / overflowed
                     uint32_t seqHdrSize, seqGap;     // the sequence section lies in its buffer as seqHdrSize bytes, seqGap (0..3) unused bytes,
                     uint32_t pad[2]; };              // then the bitstream (built 4-byte aligned); k_assemble_frames closes the gap as it copies
                                                      // (pad: a -DZS_CHAIN_COUNT build's counts, below)

// The twelve buffers: X(name, element type, elements a block slot, fixed tail in bytes).  A buffer of a sub-batch of cap blocks is
// cap * elements * sizeof(element) + tail bytes.  (The tails: reads and stores of whole groups may pass a slot's end - the last slot's too;
// the range results' 8 MiB also holds a -DZS_WALK_PROFILE build's stamps.)
//   dist     stage-1 distances, low 16 bits, a position each        k_lz_candidates -> k_lz_walk
//   distHi   bit 16 of the distances, a bit a position (big units)  k_lz_candidates -> k_lz_walk
//   cand     candidate positions of a unit, a word a table          k_lz_candidates -> k_lz_walk
//   recs     the walkers' records: a walk range at block position p owns the slots from p / 4       k_lz_walk -> k_lz_stitch
//   res      a result a walk range: records, last match end, last offset                            k_lz_walk -> k_lz_stitch
//   seqs     a block's records that count: one list, in block order, no holes                      k_lz_stitch -> entropy kernels, k_train_stats
//   hdrs     a block's ZsBlockHdr (sequences, trailing literals, all literals) in front of its slot  k_lz_stitch -> entropy kernels, k_train_stats
//   lits     the block's literals, gathered                          k_encode_literals (lends: chain codes)
//   streams  its four Huffman streams before they are joined        k_encode_literals (lends: chain outputs)
//   litSec   its literal section                                     k_encode_literals -> k_assemble_frames
//   seqSec   its sequence section                                    k_encode_sequences -> k_encode_literals, k_assemble_frames
//   metas    ZsBlockMeta                                             both encode kernels -> k_assemble_frames
#define ZS_SCRATCH_TABLE(X) \
    X(dist,    uint16_t,    ZS_BLOCK_MAX,                      256u) \
    X(distHi,  uint8_t,     ZS_BLOCK_MAX / 8,                  256u) \
    X(cand,    uint32_t,    2u,                                64u) \
    X(recs,    uint2,       ZS_BLOCK_MAX / 4,                  512u) \
    X(res,     uint4,       ZS_RES_PER_BLOCK,                  8u << 20) \
    X(seqs,    ZsSeqRec,    ZS_SEQ_MAX,                        0u) \
    X(hdrs,    uint32_t,    ZS_HDR_SLOT_WORDS,                 0u) \
    X(lits,    uint8_t,     ZS_BLOCK_MAX + 64u,                0u) \
    X(streams, uint8_t,     4u * ZS_STREAM_STRIDE,             0u) \
    X(litSec,  uint8_t,     ZS_LITSEC_STRIDE,                  0u) \
    X(seqSec,  uint8_t,     ZS_SEQSEC_STRIDE,                  0u) \
    X(metas,   ZsBlockMeta, 1u,                                0u)
struct ZsScratchRow { const char *name; size_t slotBytes, tailBytes; };
#define X(name, T, perSlot, tail) kZsScratch_##name,
enum { ZS_SCRATCH_TABLE(X) kZsScratchCount };
#undef X
#define X(name, T, perSlot, tail) { #name, (size_t)(perSlot) * sizeof(T), (size_t)(tail) },
static const ZsScratchRow kZsScratchRows[kZsScratchCount] = { ZS_SCRATCH_TABLE(X) };
#undef X

// An accessor keeps the constness of the pointer it is given (a kernel that only reads a buffer takes it const __restrict__).
#define ZS_SLOT_OF(T, P) static_assert(std::is_same<typename std::remove_const<P>::type, T>::value, "the buffer's element type")

// ---- dist, distHi, cand: a unit's, from its first block's slot ----
template <class P> __device__ __forceinline__ P *zs_block_dist(P *distAll, size_t slot) { ZS_SLOT_OF(uint16_t, P); return distAll + slot * ZS_BLOCK_MAX; }
template <class P> __device__ __forceinline__ P *zs_block_dist_hi(P *distHiAll, size_t slot) { ZS_SLOT_OF(uint8_t, P); return distHiAll + slot * (ZS_BLOCK_MAX / 8); }
template <class P, class S, class T> __device__ __forceinline__ P &zs_block_cand(P *candCount, S slot, T table) { ZS_SLOT_OF(uint32_t, P); return candCount[2 * slot + table]; }
// dist lends: k_encode_sequences' pack records (8 bytes a sequence: its extra bits), to the sequences kernel from the stitch on - the
// distances are dead since the walk, and the next sub-batch's k_lz_candidates writes them first.  (The host hands the buffer over as uint2.)
static_assert(ZS_CHAIN_CODES * sizeof(uint2) <= ZS_BLOCK_MAX * sizeof(uint16_t), "a block's pack records fit its slot of the distances");
__device__ __forceinline__ uint2 *zs_dist_lend_pack_records(uint2 *distAllAsRecords, size_t slot) { return distAllAsRecords + slot * ZS_CHAIN_CODES; }

// ---- recs, res ----
template <class P> __device__ __forceinline__ P *zs_block_walk_records(P *recAll, size_t slot) { ZS_SLOT_OF(uint2, P); return recAll + slot * (ZS_BLOCK_MAX / 4); }
template <class P> __device__ __forceinline__ P *zs_block_range_results(P *resAll, size_t slot) { ZS_SLOT_OF(uint4, P); return resAll + slot * ZS_RES_PER_BLOCK; }
// walk range rr of a UNIT (perBlockLog: log2 of the walk ranges a block has): its index from the unit's first block's results
__device__ __forceinline__ uint32_t zs_unit_range_result(uint32_t rr, uint32_t perBlockLog) { return (rr >> perBlockLog) * ZS_RES_PER_BLOCK + (rr & ((1u << perBlockLog) - 1u)); }
// k_lz_walk's junkSlot argument: the record slots of all cap blocks (the host's side of the profile borrowing below)
__host__ __device__ __forceinline__ uint32_t zs_walk_records_end(uint32_t cap) { return cap * (ZS_BLOCK_MAX / 4); }
// res lends (a -DZS_WALK_PROFILE build): 10 stamp sums a wavefront of k_lz_walk, unit after unit, behind ALL blocks' results - in the fixed
// tail, which every build pays for.  (recordsEnd / 64 = cap * ZS_RES_PER_BLOCK.)  The tail holds the stamps of 6553 units of the widest
// kernel (16 wavefronts); tools/walk_profile.py runs 4096.
static_assert((ZS_BLOCK_MAX / 4) / 64 == ZS_RES_PER_BLOCK && 4096u * 16u * 10u * sizeof(unsigned long long) <= (8u << 20), "the walk profile's stamps lie behind the results, inside the tail");
__device__ __forceinline__ unsigned long long *zs_res_lend_walk_profile(uint4 *resAll, uint32_t recordsEnd) { return reinterpret_cast<unsigned long long *>(resAll + (size_t)(recordsEnd / 64)); }

// ---- seqs, hdrs ----
// a block's list: records [0, ZsBlockHdr::nseq), in block order (a record's literals: from the end of the record before it, zsmi_device.h)
template <class P> __device__ __forceinline__ P *zs_block_seqs(P *seqAll, size_t slot) { ZS_SLOT_OF(ZsSeqRec, P); return seqAll + slot * ZS_SEQ_MAX; }
__device__ __forceinline__ ZsBlockHdr &zs_block_hdr(uint32_t *hdrAll, size_t slot) { return *reinterpret_cast<ZsBlockHdr *>(hdrAll + slot * ZS_HDR_SLOT_WORDS); }
__device__ __forceinline__ const ZsBlockHdr &zs_block_hdr(const uint32_t *hdrAll, size_t slot) { return *reinterpret_cast<const ZsBlockHdr *>(hdrAll + slot * ZS_HDR_SLOT_WORDS); }

// ---- lits, streams ----
template <class P> __device__ __forceinline__ P *zs_block_lits(P *litsAll, size_t slot) { ZS_SLOT_OF(uint8_t, P); return litsAll + slot * (ZS_BLOCK_MAX + 64); }
template <class P> __device__ __forceinline__ P *zs_block_streams(P *streamAll, size_t slot) { ZS_SLOT_OF(uint8_t, P); return streamAll + slot * 4 * ZS_STREAM_STRIDE; }
template <class P> __device__ __forceinline__ P *zs_stream(P *blockStreams, uint32_t k) { ZS_SLOT_OF(uint8_t, P); return blockStreams + k * ZS_STREAM_STRIDE; }                    // of a block's (zs_block_streams), k < 4
// lits and streams lend: the state chains of k_encode_sequences - a code byte a sequence in three tables (LL, OF with the recent-offset codes
// applied, ML) ZS_CHAIN_CODES apart in the block's literal buffer, 16 bits of chain output a sequence in three tables ZS_CHAIN_CODES apart in
// its stream buffers.  To the sequences kernel until k_encode_literals STARTS on the stream: that kernel runs after it and writes both buffers
// before it reads them.  (So the two encoders cannot run side by side as they are.)
static_assert(3u * ZS_CHAIN_CODES <= ZS_BLOCK_MAX + 64u && 3u * 2u * ZS_CHAIN_CODES <= 4u * ZS_STREAM_STRIDE, "the chain scratch fits the buffers it borrows");
__device__ __forceinline__ uint8_t *zs_lits_lend_chain_codes(uint8_t *litsAll, size_t slot) { return zs_block_lits(litsAll, slot); }
__device__ __forceinline__ uint16_t *zs_streams_lend_chain_outs(uint8_t *streamAll, size_t slot) { return reinterpret_cast<uint16_t *>(zs_block_streams(streamAll, slot)); }
// ... and k_train_stats (the dictionary trainer's finalize), launched between the two encoders, reads the codes back where the chains left them
__device__ __forceinline__ const uint8_t *zs_lits_lend_chain_codes_to_stats(const uint8_t *litsAll, size_t slot) { return zs_block_lits(litsAll, slot); }

// ---- litSec, seqSec, metas ----
template <class P> __device__ __forceinline__ P *zs_block_lit_section(P *litSecAll, size_t slot) { ZS_SLOT_OF(uint8_t, P); return litSecAll + slot * ZS_LITSEC_STRIDE; }
template <class P> __device__ __forceinline__ P *zs_block_seq_section(P *seqSecAll, size_t slot) { ZS_SLOT_OF(uint8_t, P); return seqSecAll + slot * ZS_SEQSEC_STRIDE; }         // 4-byte aligned
// seqSec lends, to its own kernel: 32 bytes a lane in the middle of the block's section buffer, where a lane of the chains that has nothing
// to store stores all the same (the packing writes the section's bytes afterwards; the headers in front of the bitstream end far below)
static_assert(32768u + 64u * 32u <= ZS_SEQSEC_STRIDE, "the junk store slots lie inside the section buffer");
__device__ __forceinline__ uint8_t *zs_seqsec_lend_junk_store(uint8_t *blockSeqSection, uint32_t lane) { return blockSeqSection + 32768u + 32u * lane; }
template <class P> __device__ __forceinline__ P &zs_block_meta(P *metas, size_t slot) { ZS_SLOT_OF(ZsBlockMeta, P); return metas[slot]; }
// metas lends (a -DZS_CHAIN_COUNT build) its pad words: pad[0] seams that failed | rounds of repair << 16, pad[1] segments | blocks a segment << 8 | sequences << 16
static_assert(sizeof(((ZsBlockMeta *)nullptr)->pad) == 2 * sizeof(uint32_t), "the chain counts are two words");
__device__ __forceinline__ ZsBlockMeta &zs_meta_lend_chain_counts(ZsBlockMeta *metas, size_t slot) { return metas[slot]; }       // (.pad)

// =============================================================================================
// decode
// =============================================================================================
// The general kernel's wavefronts form a pool with a literal buffer each, whatever the call's size
#define ZS_DEC_LITBUF ((1u << 17) + 64u)                 // a wavefront's literal buffer: the largest block + slack
__device__ __forceinline__ uint8_t *zs_pool_lit_buffer(uint8_t *poolLitAll, size_t wavefront) { return poolLitAll + wavefront * ZS_DEC_LITBUF; }
// poolLit lends (a -DZS_DEC_PROFILE build): cycles per phase of the wavefront's last item, 8 words in the slack behind the largest block
static_assert((1u << 17) + 8u * sizeof(uint64_t) <= ZS_DEC_LITBUF, "the decode profile's words fit the slack");
__device__ __forceinline__ uint64_t *zs_poollit_lend_dec_profile(uint8_t *litBuf) { return reinterpret_cast<uint64_t *>(litBuf + (1u << 17)); }

// The fast path keeps per-block scratch in slot = block index * cap + item (cap: items in flight), sized by the call's plan (litStride,
// seqCap: DecodePlan in zsmi_api.hip).  An item has max(2, block slots) descriptors; the descriptor of block 0 speaks for the item.
#define ZS_FAST_HUFLOG   11u                      // Huffman tables the fast kernel holds: 2^11 entries per item
#define ZS_FAST_MAXSEQ   16384u                   // sequences per block the fast path buffers (8 bytes each)
#define ZS_FAST_HUFTAB_BYTES (2u << ZS_FAST_HUFLOG)                       // uint16 entries
#define ZS_FAST_SEQTAB_BYTES ((512u + 256u + 512u) * 2u)                  // LL, OF, ML cells, 2 bytes each
struct ZsFastDesc;                                // a block's descriptor, written by k_dec_prep (decode_fast.hip)
// what the sequences kernel leaves per sequence, 8 bytes: where its extra bits start in the bitstream (bit position, 20 bits)
// and its three codes (LL 6 bits at 20, ML 6 bits at 26, OF 5 bits at 32).  The execute kernel turns that into lengths and
// offsets, 64 sequences at a time on 64 lanes; only the FSE state chain stays serial.
typedef uint64_t ZsFastSeq;
// bytes a slot of the buffers whose stride no plan chooses (poolLit: a wavefront; a descriptor is sizeof(ZsFastDesc)): the host's sizes and the debug hooks
struct ZsDecSlotBytes { static constexpr size_t poolLit = ZS_DEC_LITBUF, hufTabs = ZS_FAST_HUFTAB_BYTES, seqTabs = ZS_FAST_SEQTAB_BYTES, seqOut = sizeof(ZsFastSeq); };

__device__ __forceinline__ size_t zs_dec_slot(uint32_t blk, uint32_t cap, uint32_t item) { return (size_t)blk * cap + item; }
template <class P> __device__ __forceinline__ P *zs_slot_desc(P *descs, size_t slot) { ZS_SLOT_OF(ZsFastDesc, P); return descs + slot; }
template <class P> __device__ __forceinline__ P *zs_slot_huf_table(P *hufTabs, size_t slot) { ZS_SLOT_OF(uint8_t, P); return hufTabs + slot * ZS_FAST_HUFTAB_BYTES; }
__device__ __forceinline__ size_t zs_slot_seq_tables_at(size_t slot) { return slot * ZS_FAST_SEQTAB_BYTES; }      // (the byte offset alone)
template <class P> __device__ __forceinline__ P *zs_slot_seq_tables(P *seqTabs, size_t slot) { ZS_SLOT_OF(uint8_t, P); return seqTabs + zs_slot_seq_tables_at(slot); }
template <class P> __device__ __forceinline__ P *zs_slot_literals(P *litScratchAll, size_t slot, uint32_t litStride) { ZS_SLOT_OF(uint8_t, P); return litScratchAll + slot * litStride; }
template <class P> __device__ __forceinline__ P *zs_slot_seq_out(P *seqOutAll, size_t slot, uint32_t seqCap) { ZS_SLOT_OF(ZsFastSeq, P); return seqOutAll + slot * seqCap; }
// hufTabs lends (a -DZS_PREP_PROFILE build): ticks of k_dec_prep's 12 phases and the wavefront's whole time, in the second half of the item's
// block-0 table - the two-level table ends at 1280 bytes; a flat one fills the slot, and such an item leaves no stamps
static_assert(2048u + 13u * sizeof(unsigned long long) <= ZS_FAST_HUFTAB_BYTES, "the prep profile's words fit the slot");
__device__ __forceinline__ unsigned long long *zs_huftab_lend_prep_profile(uint8_t *hufTabs, uint32_t item) { return reinterpret_cast<unsigned long long *>(zs_slot_huf_table(hufTabs, (size_t)item) + 2048); }

// dSeqLists, in 32-bit words (slots = cap * block slots an item; "-": unused):
//   [queue][left count][-][-][class count 0][class count 1][class list 0: slots][class list 1: slots][-][-][left list: cap]
// queue, left count, left list: the general kernel's - a counter its wavefronts take items from, and behind the fast path the items that
// path left (k_dec_collect fills the list and its count); without the fast path only the queue and the count are used.  The classes: the
// slots of the blocks with sequences, by table class (k_dec_prep appends, the sequences kernels read).  The host hands the words out
// (queue .. leftList); the fast kernels are handed classes() and reach the counts and lists from there.
struct DecLists {
    static constexpr size_t kQueue = 0, kLeftCount = 1, kClassCounts = 4, kClassLists = kClassCounts + 2;   // (the fast path zeroes every word in front of kClassLists)
    static size_t words(size_t slots, size_t items) { return kClassLists + 2 * slots + 2 + items; }
    static uint32_t *queue(uint32_t *lists) { return lists + kQueue; }
    static uint32_t *leftCount(uint32_t *lists) { return lists + kLeftCount; }
    static uint32_t *classes(uint32_t *lists) { return lists + kClassCounts; }
    static uint32_t *leftList(uint32_t *lists, size_t slots) { return lists + kClassLists + 2 * slots + 2; }
    // from classes(): class cls has its count at word kCountAt + cls and its list at word kListAt + cls * cap * block slots
    static constexpr size_t kCountAt = 0, kListAt = kClassLists - kClassCounts;
    template <class P> __device__ __forceinline__ static P &classCount(P *classes, uint32_t cls) { return classes[kCountAt + cls]; }
    template <class P> __device__ __forceinline__ static P *classList(P *classes, uint32_t cls, uint32_t cap, uint32_t blockSlots) { return classes + kListAt + (size_t)cls * cap * blockSlots; }
    // the general kernel's items: the left list's where there is one (leftList, leftCount), else every item of the call
    __device__ __forceinline__ static uint32_t queued(const uint32_t *leftList, const uint32_t *leftCount, uint32_t nItems) { return leftList ? *leftCount : nItems; }
    __device__ __forceinline__ static uint32_t queuedItem(const uint32_t *leftList, uint32_t at) { return leftList ? leftList[at] : at; }
};
