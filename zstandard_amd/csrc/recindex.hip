// recindex.hip -- the record index of an archive (zsmi_recindex.h states the rule, the index frame and MISALIGNED; zsmi_indexRecords runs
// the rule serially on the host): firstRecord rebuilt from text and frame borders, loaded from an archive's index frame, or attached to
// an archive as that frame.  The device calls only queue work.
//
// The body (zsmi_indexRecordsDevice) over text[0, size) and places[0 .. n] - the frames' borders in the text, ascending, 0 first, size
// last - a workgroup a 16 KiB tile (the splitter's load: 256 threads x 16 bytes x 4 steps), two streaming passes over the text:
//   k_recidx_tiles   the delimiters of each tile, and TAIL[t]: those at or behind the last place that lies in tile t
//   scanOffsets      over the tiles' delimiters: BASE[t], the delimiters in front of tile t
//   k_recidx_places  the tile's delimiter bits into LDS (2 KiB) with a popcount prefix a 32-bit word (2 KiB); two binary searches over
//                    places find the places that lie in the tile (tile t holds [16384 t, 16384 (t + 1)), the last tile `size` too); a lane
//                    a place: firstRecord[j] = *dBase + BASE[t] + the prefix at the place inside the tile (+ 1 for the tail record at
//                    `size` when that is the content's end).  The tile also counts the misaligned frames among those that END in it: the
//                    byte in front of place j is a bit of the tile (the text's byte when the place is the tile's first), and frame j - 1
//                    holds a delimiter when the prefix moved since place j - 1 - inside the tile from the LDS prefix; for a frame that
//                    came in from tile t' < t: the prefix at the place, + BASE[t] - BASE[t' + 1] (the tiles between), + TAIL[t'] (place
//                    j - 1 is the last place of t', as the places ascend).  No lane reads a tile for a place's sake.
//                    One lane of the first workgroup writes dResult, the tiles add their misaligned frames to its third word.
// A tile's places are taken 256 at a time by one workgroup: millions of EMPTY frames at one place are one workgroup's loop.
// On an archive (zsmi_seekableIndexRecordsResident) the window's frames are decoded end to end into dWork by find.hip's findDecode, the
// body's words behind its own; the places are its layout scan.  The host form walks seekable.hip's window plan.  An index frame among them is an entry of no content: k_seek_request_items plans it with no
// capacity, the decoder steps over the skippable frame and k_seek_verify finds no bytes and the hash of none - it stays in the list.
// Load (zsmi_seekableLoadRecordIndexResident): k_recidx_unpack - a lane a count, the check's terms and the counts' sum added up by
// wavefront into four words, each count held against its entry of the handle's table -, scanOffsets over the counts, k_recidx_loaded -
// the verdict of zsmi_readRecordIndexFrame from the header and the four words; only a good verdict copies the offsets out.
// Attach (zsmi_seekableAttachRecordIndexResident): table and index overlap their old places, so the table moves in two steps through
// scratch: k_recidx_table_out - the archive's table judged entry by entry and copied into scratch, the counts judged beside it -,
// k_recidx_verdict - one lane: what the host form refuses, in its order, while the archive is still as it came -, k_recidx_pack - the
// table from scratch to its new place with the new entry and footer, the counts and their terms of the check -, k_recidx_attached -
// the frame's header and the size word.
// Scratch, all of it context buffers reserved before anything is queued: 16 bytes a tile and a scan of 8 in the seekable scratch behind
// findDecode's words; load: 12 bytes a frame; attach: the table's bytes.  Every store is a vector store from plain C++.

#include "zsmi_status.h"
#include "zsmi_wave.h"            // wave_incl_scan, wave_sum
#include "zsmi_ctx.h"             // the context, LAUNCH, scanOffsets
#include "zsmi_recindex.h"        // the rule, the frame, the host forms
#include <algorithm>
// From the feature files zsmi_api.hip includes in front of this one: split.hip - ZS_SPLIT_TILE, ZsSplitBytes16; records.hip -
// zs_rec_mask16; seekable.hip - the handle, ZsSeekEntry, seekWindowCheck, the window plan (SeekWindows, seekCutWindows, seekWindowLimit),
// zsmi_seekableFindWorkBound; find.hip - the decode half of a window (findDecodeReserve, findDecode, FindDecoded).

// ---- kernels: the body ----
// mask[s] bit k: the byte at tile * ZS_SPLIT_TILE + s * 4096 + 16 * threadIdx.x + k is the delimiter.  Whole tiles by four 16-byte loads a
// lane, issued together; the text's last tile, unless it is a whole one, byte by byte: no byte at or behind src + size is read
__device__ __forceinline__ void zs_ridx_tile_masks(const uint8_t *__restrict__ src, uint64_t size, uint32_t delim, uint64_t tile, uint32_t mask[4])
{
    const uint64_t tileAt = tile * ZS_SPLIT_TILE, base = tileAt + 16u * threadIdx.x;
    const uint32_t delim4 = delim * 0x01010101u;
    if (size >= tileAt + ZS_SPLIT_TILE) {
        ZsSplitBytes16 own[4];
        #pragma unroll
        for (uint32_t s = 0; s < 4; s++) __builtin_memcpy(&own[s], src + base + s * 4096u, 16);
        #pragma unroll
        for (uint32_t s = 0; s < 4; s++) mask[s] = zs_rec_mask16(own[s], delim4);
    } else {
        for (uint32_t s = 0; s < 4; s++) {
            const uint64_t b = base + s * 4096u;
            uint32_t m = 0;
            for (uint32_t j = 0; j < 16; j++) if (b + j < size && src[b + j] == delim) m |= 1u << j;
            mask[s] = m;
        }
    }
}
// the first j of places[0, count) with places[j] >= v (count: none)
__device__ __forceinline__ uint32_t zs_ridx_lower(const uint64_t *__restrict__ places, uint32_t count, uint64_t v)
{
    uint32_t lo = 0, hi = count;
    while (lo < hi) { const uint32_t mid = lo + (hi - lo) / 2u; if (places[mid] < v) lo = mid + 1u; else hi = mid; }
    return lo;
}
// the places of tile `tile` are those in [its start, zs_ridx_limit): the next tile's start, or size + 1 for the last tile
__device__ __forceinline__ uint64_t zs_ridx_limit(uint64_t tile, uint32_t tiles, uint64_t size) { return tile + 1u == tiles ? size + 1u : (tile + 1u) * ZS_SPLIT_TILE; }
// the sum of v over the workgroup's 256 threads (every thread calls it; slots: four words of LDS that are free to write)
__device__ __forceinline__ uint32_t zs_ridx_block_sum(uint32_t v, uint32_t *slots)
{
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63u) == 0) slots[threadIdx.x >> 6] = v;
    __syncthreads();
    return slots[0] + slots[1] + slots[2] + slots[3];
}
// counts[tile]: its delimiters; tails[tile]: those at or behind the tile's last place (the tile's count when no place lies in it: not read)
__global__ void __launch_bounds__(256)
k_recidx_tiles(const uint8_t *__restrict__ src, uint64_t size, uint32_t delim, const uint64_t *__restrict__ places, uint32_t n, uint32_t tiles,
               uint32_t *__restrict__ counts, uint32_t *__restrict__ tails)
{
    __shared__ uint32_t slots[4];
    const uint64_t tileAt = (uint64_t)blockIdx.x * ZS_SPLIT_TILE;
    uint32_t mask[4];
    zs_ridx_tile_masks(src, size, delim, blockIdx.x, mask);
    const uint32_t hi = zs_ridx_lower(places, n + 1u, zs_ridx_limit(blockIdx.x, tiles, size));
    uint32_t from = 0;                                                     // the tile's last place, counted from the tile's start
    if (hi) { const uint64_t x = places[hi - 1u]; if (x >= tileAt) from = (uint32_t)(x - tileAt); }
    uint32_t all = 0, behind = 0;
    #pragma unroll
    for (uint32_t s = 0; s < 4; s++) {
        const uint32_t b = s * 4096u + 16u * threadIdx.x;
        all += (uint32_t)__popc(mask[s]);
        behind += from <= b ? (uint32_t)__popc(mask[s]) : (from >= b + 16u ? 0u : (uint32_t)__popc(mask[s] >> (from - b)));
    }
    all = zs_ridx_block_sum(all, slots);
    behind = zs_ridx_block_sum(behind, slots);
    if (threadIdx.x == 0) { counts[blockIdx.x] = all; tails[blockIdx.x] = behind; }
}
struct ZsRidxShared { uint32_t bits[512], pre[513], slots[4]; };
// the delimiters of the tile in front of its byte o, 0 <= o <= ZS_SPLIT_TILE
__device__ __forceinline__ uint32_t zs_ridx_prefix(const ZsRidxShared &sh, uint32_t o)
{
    const uint32_t w = o >> 5, r = o & 31u;
    return sh.pre[w] + (r ? (uint32_t)__popc(sh.bits[w] & ((1u << r) - 1u)) : 0u);
}
// tileBase[0 .. tiles]: the scan of counts.  base: one device word, or null for 0; with a base entry 0 of firstRecord is the caller's.
// code: null, or the window's code (find.hip).  result[2] was zeroed on the stream in front of the kernel.
__global__ void __launch_bounds__(256)
k_recidx_places(const uint8_t *__restrict__ src, uint64_t size, uint32_t delim, const uint64_t *__restrict__ places, uint32_t n, uint32_t atEnd, uint32_t tiles,
                const uint64_t *__restrict__ tileBase, const uint32_t *__restrict__ tails, const uint64_t *__restrict__ base, const uint32_t *__restrict__ code,
                uint64_t *__restrict__ firstRecord, uint64_t *__restrict__ result)
{
    __shared__ ZsRidxShared sh;
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    const uint64_t tileAt = (uint64_t)blockIdx.x * ZS_SPLIT_TILE;
    const bool tailRecord = atEnd && size && src[size - 1u] != delim;       // the + 1 at `size`
    uint32_t mask[4];
    zs_ridx_tile_masks(src, size, delim, blockIdx.x, mask);
    #pragma unroll
    for (uint32_t s = 0; s < 4; s++) {                                      // bit o of the tile: bits[o / 32] >> (o % 32); two lanes a word, the even one stores
        const uint32_t pair = mask[s] | ((uint32_t)__shfl_down((int)mask[s], 1) << 16);
        if (!(tid & 1u)) sh.bits[s * 128u + (tid >> 1)] = pair;
    }
    __syncthreads();
    {                                                                      // pre[w]: the bits of the words in front of word w; pre[512]: all
        const uint32_t p0 = (uint32_t)__popc(sh.bits[2u * tid]), p = p0 + (uint32_t)__popc(sh.bits[2u * tid + 1u]);
        const uint32_t incl = wave_incl_scan(p);
        if (lane == 63u) sh.slots[wave] = incl;
        __syncthreads();
        uint32_t ahead = 0;
        for (uint32_t w = 0; w < wave; w++) ahead += sh.slots[w];
        const uint32_t excl = ahead + incl - p;
        sh.pre[2u * tid] = excl; sh.pre[2u * tid + 1u] = excl + p0;
        if (tid == 255u) sh.pre[512] = excl + p;
    }
    __syncthreads();
    const uint64_t before = tileBase[blockIdx.x], first = (base ? *base : 0ull) + before;
    const uint64_t limit = zs_ridx_limit(blockIdx.x, tiles, size);
    const uint32_t lo = zs_ridx_lower(places, n + 1u, tileAt), hi = zs_ridx_lower(places, n + 1u, limit);
    uint32_t misaligned = 0;
    for (uint32_t j = lo + tid; j < hi; j += 256u) {                       // (j <= n < 2^28: no wrap)
        const uint64_t x = places[j];
        if (x < tileAt || x >= limit) continue;                            // (places that do not ascend: the search's answer is no promise)
        const uint32_t o = (uint32_t)(x - tileAt), d = zs_ridx_prefix(sh, o);
        if (j || !base) firstRecord[j] = first + d + (x == size && tailRecord ? 1u : 0u);
        if (!j) continue;
        const uint64_t xp = places[j - 1u];                                // frame j - 1 = [xp, x) ends in this tile
        if (xp >= x) continue;                                             // (an empty frame; or places that do not ascend)
        bool holds;
        if (xp >= tileAt) holds = d > zs_ridx_prefix(sh, (uint32_t)(xp - tileAt));
        else { const uint64_t tp = xp / ZS_SPLIT_TILE; /* tp < this tile */ holds = d != 0u || before - tileBase[tp + 1u] + tails[tp] != 0ull; }
        const bool lastIsDelim = o ? ((sh.bits[(o - 1u) >> 5] >> ((o - 1u) & 31u)) & 1u) != 0u : src[x - 1u] == delim;
        misaligned += zs_ridx_misaligned(holds, lastIsDelim, atEnd && x == size) ? 1u : 0u;
    }
    misaligned = zs_ridx_block_sum(misaligned, sh.slots);
    if (tid == 0 && misaligned) atomicAdd((unsigned long long *)(result + 2), (unsigned long long)misaligned);
    if (blockIdx.x == 0 && tid == 0) {
        const uint32_t failed = code ? *code : 0u;
        const uint64_t delims = tileBase[tiles];
        result[0] = failed ? failed : (places[0] == 0 && places[n] == size ? 0u : (uint32_t)ZSMI_error_parameter_outOfBound);
        result[1] = delims + (tailRecord ? 1u : 0u);
        result[3] = delims;
    }
}

// ---- kernels: load ----
struct ZsRidxSums { unsigned long long check, sum, bad, pad; };            // the counts' terms of the check, their sum, the counts above their entry's Decompressed_Size
__device__ __forceinline__ unsigned long long zs_ridx_wave_sum64(unsigned long long v)
{
    for (int d = 32; d; d >>= 1) v += (unsigned long long)__shfl_down((long long)v, d);
    return v;                                                              // (lane 0's)
}
// frame: the index frame's bytes, n counts behind its 40 fixed ones (the host holds n and the frame's size against the table's entry, so
// every byte read is the frame's whatever its header says).  counts[i] for the scan; sums: zeroed on the stream in front of the kernel
__global__ void __launch_bounds__(256)
k_recidx_unpack(const uint8_t *__restrict__ frame, uint32_t n, const ZsSeekEntry *__restrict__ table, uint32_t *__restrict__ counts, ZsRidxSums *sums)
{
    unsigned long long check = 0, sum = 0, bad = 0;
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
        const uint32_t count = zs_ridx_rd32(frame + ZS_RIDX_FIXED + 4ull * i);
        counts[i] = count;
        check += zs_ridx_term(count, i); sum += count; bad += count > table[i].dSize ? 1u : 0u;
    }
    check = zs_ridx_wave_sum64(check); sum = zs_ridx_wave_sum64(sum); bad = zs_ridx_wave_sum64(bad);
    if ((threadIdx.x & 63u) == 0) { atomicAdd(&sums->check, check); atomicAdd(&sums->sum, sum); if (bad) atomicAdd(&sums->bad, bad); }
}
// the verdict of zsmi_readRecordIndexFrame on the header and the sums (every lane's the same); then, good: firstRecord[0 .. n] = offsets[0 .. n]
// and firstRecord[n + 1] = records.  frame == null: the handle's last entry is no index frame by its table alone
__global__ void __launch_bounds__(256)
k_recidx_loaded(const uint8_t *__restrict__ frame, uint32_t n, uint32_t sized, const ZsRidxSums *__restrict__ sums, const uint64_t *__restrict__ offsets,
                uint64_t *__restrict__ firstRecord, uint64_t *__restrict__ result)
{
    uint32_t status = ZSMI_error_prefix_unknown, delim = 0, k = 0;
    uint64_t records = 0;
    if (frame) {
        status = (uint32_t)zs_ridx_read_header(frame, &k, &delim);
        if (!status && (k != n || !sized)) status = ZSMI_error_corruption_detected;      // (sized: the entry's Compressed_Size is 40 + 4 n)
        if (!status) {
            records = zs_ridx_rd64(frame + 24);
            if (sums->check + zs_ridx_check_base(records, delim) != zs_ridx_rd64(frame + 32) || sums->sum != records || sums->bad) status = ZSMI_error_corruption_detected;
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) { result[0] = status; result[1] = status ? 0ull : records; result[2] = status ? 0u : delim; result[3] = status ? 0u : n; }
    if (status) return;
    for (uint64_t i = blockIdx.x * 256u + threadIdx.x; i <= (uint64_t)n + 1u; i += gridDim.x * 256u) firstRecord[i] = i <= n ? offsets[i] : records;
}


// ---- kernels: attach ----
struct ZsRidxAttach { unsigned long long cSum, badEntry, badCount, check; };      // zeroed on the stream in front of the kernels
struct ZsRidxVerdict { uint32_t status, entry; uint64_t at, size; uint32_t desc, pad; };      // status ~0: the size word came in as an error
// what the footer says of the archive of `size` bytes: 0 with the frame count, the entry size and the table's place, or the code - the
// order of zs_ridx_parse_table, the entries' own checks left to k_recidx_table_out
__device__ __forceinline__ uint32_t zs_ridx_footer(const uint8_t *__restrict__ a, uint64_t size, uint64_t capacity, uint32_t *k, uint32_t *entry, uint64_t *at)
{
    if (size > capacity || size < 9) return ZSMI_error_prefix_unknown;
    const uint8_t *footer = a + size - 9;
    if (zs_ridx_rd32(footer + 5) != ZS_RIDX_SEEK_MAGIC) return ZSMI_error_prefix_unknown;
    if (footer[4] & 0x7C) return ZSMI_error_corruption_detected;
    *k = zs_ridx_rd32(footer);
    if (*k > ZS_RIDX_MAX_FRAMES) return ZSMI_error_frameIndex_tooLarge;
    *entry = footer[4] & 0x80 ? 12u : 8u;
    const uint64_t tableSize = ZS_RIDX_SEEK_FIXED + (uint64_t)*k * *entry;
    if (tableSize > size) return ZSMI_error_corruption_detected;
    *at = size - tableSize;
    if (zs_ridx_rd32(a + *at) != ZS_RIDX_SEEK_SKIP) return ZSMI_error_prefix_unknown;
    return zs_ridx_rd32(a + *at + 4) != *k * *entry + 9u ? (uint32_t)ZSMI_error_corruption_detected : 0u;
}
// step 1 of the table's move: the table's k entries judged - a Compressed_Size of 0, a Decompressed_Size over 1 GiB: a bad entry; the
// Compressed_Sizes summed - and, when k is the caller's n, copied into scratch (keep[i * entry ..]) with the counts judged beside them: a
// descent or a count above the entry's Decompressed_Size is a bad count.  An error word in *archiveSize, or a footer that is refused:
// nothing is read
__global__ void __launch_bounds__(256)
k_recidx_table_out(const uint8_t *__restrict__ a, uint64_t capacity, const uint64_t *__restrict__ archiveSize, const uint64_t *__restrict__ firstRecord, uint32_t n,
                   uint8_t *__restrict__ keep, ZsRidxAttach *sums)
{
    const uint64_t size = *archiveSize;
    uint32_t k, entry; uint64_t at;
    if (size > 0ull - (uint64_t)ZSMI_error_maxCode || zs_ridx_footer(a, size, capacity, &k, &entry, &at)) return;
    unsigned long long cSum = 0, badEntry = 0, badCount = 0;
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < k; i += gridDim.x * 256u) {
        const uint8_t *e = a + at + 8u + (uint64_t)i * entry;
        const uint32_t cSize = zs_ridx_rd32(e), dSize = zs_ridx_rd32(e + 4);
        cSum += cSize;
        badEntry += cSize == 0 || dSize > ZS_RIDX_SEEK_MAX_DSIZE ? 1u : 0u;
        if (k != n) continue;
        for (uint32_t b = 0; b < entry; b++) keep[(uint64_t)i * entry + b] = e[b];
        const uint64_t r0 = firstRecord[i], r1 = firstRecord[i + 1u];
        badCount += r1 < r0 || r1 - r0 > dSize ? 1u : 0u;
    }
    cSum = zs_ridx_wave_sum64(cSum); badEntry = zs_ridx_wave_sum64(badEntry); badCount = zs_ridx_wave_sum64(badCount);
    if ((threadIdx.x & 63u) == 0) { atomicAdd(&sums->cSum, cSum); if (badEntry) atomicAdd(&sums->badEntry, badEntry); if (badCount) atomicAdd(&sums->badCount, badCount); }
}
// the call's verdict, in zsmi_seekableAttachRecordIndex's order, while the archive is still as it came: one lane
__global__ void k_recidx_verdict(const uint8_t *__restrict__ a, uint64_t capacity, const uint64_t *__restrict__ archiveSize, const uint64_t *__restrict__ firstRecord, uint32_t n,
                                 const uint8_t *__restrict__ keep, const ZsRidxAttach *__restrict__ sums, ZsRidxVerdict *verdict)
{
    if (blockIdx.x || threadIdx.x) return;
    ZsRidxVerdict v; v.status = 0; v.entry = 8; v.at = 0; v.size = *archiveSize; v.desc = 0; v.pad = 0;
    uint32_t k = 0;
    if (v.size > 0ull - (uint64_t)ZSMI_error_maxCode) v.status = ~0u;
    else if (const uint32_t f = zs_ridx_footer(a, v.size, capacity, &k, &v.entry, &v.at)) v.status = f;
    else if (sums->badEntry || sums->cSum != v.at) v.status = ZSMI_error_corruption_detected;
    else if (k != n) v.status = ZSMI_error_parameter_outOfBound;
    else if (firstRecord[0] != 0 || sums->badCount) v.status = ZSMI_error_corruption_detected;
    else {
        v.desc = a[v.size - 5u];
        if (n) {                                                           // the last entry an index frame already
            const uint8_t *e = keep + (uint64_t)(n - 1u) * v.entry;
            const uint32_t cSize = zs_ridx_rd32(e);
            if (zs_ridx_rd32(e + 4) == 0 && cSize >= ZS_RIDX_FIXED && zs_ridx_rd32(a + v.at - cSize) == ZS_RIDX_MAGIC && zs_ridx_rd32(a + v.at - cSize + 8) == ZS_RIDX_INNER)
                v.status = ZSMI_error_parameter_unsupported;
        }
        if (!v.status && n + 1u > ZS_RIDX_MAX_FRAMES) v.status = ZSMI_error_frameIndex_tooLarge;
        if (!v.status && capacity < v.size + zs_ridx_frame_size(n) + v.entry) v.status = ZSMI_error_dstSize_tooSmall;
    }
    *verdict = v;
}
// step 2, a good verdict: the kept entries to their new place, 40 + 4 n bytes on (one lane: the table's header, the new entry, the footer),
// and the counts into the index frame at the old table's place, their terms of the check added up.  The two places do not overlap
__global__ void __launch_bounds__(256)
k_recidx_pack(uint8_t *a, const ZsRidxVerdict *__restrict__ verdict, const uint64_t *__restrict__ firstRecord, uint32_t n, const uint8_t *__restrict__ keep, ZsRidxAttach *sums)
{
    const ZsRidxVerdict v = *verdict;
    if (v.status) return;
    uint8_t *frame = a + v.at, *tbl = frame + zs_ridx_frame_size(n);
    const uint64_t bytes = (uint64_t)n * v.entry;
    for (uint64_t b = blockIdx.x * 256u + threadIdx.x; b < bytes; b += gridDim.x * 256u) tbl[8u + b] = keep[b];
    unsigned long long sum = 0;
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
        const uint32_t count = (uint32_t)(firstRecord[i + 1u] - firstRecord[i]);
        zs_ridx_wr32(frame + ZS_RIDX_FIXED + 4ull * i, count);
        sum += zs_ridx_term(count, i);
    }
    sum = zs_ridx_wave_sum64(sum);
    if ((threadIdx.x & 63u) == 0) atomicAdd(&sums->check, sum);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        zs_ridx_wr32(tbl, ZS_RIDX_SEEK_SKIP); zs_ridx_wr32(tbl + 4, (n + 1u) * v.entry + 9u);
        uint8_t *e = tbl + 8u + bytes;
        zs_ridx_wr32(e, (uint32_t)zs_ridx_frame_size(n)); zs_ridx_wr32(e + 4, 0);
        if (v.entry == 12u) zs_ridx_wr32(e + 8, ZS_RIDX_EMPTY_HASH);
        e += v.entry;
        zs_ridx_wr32(e, n + 1u); e[4] = (uint8_t)v.desc; zs_ridx_wr32(e + 5, ZS_RIDX_SEEK_MAGIC);
    }
}
// behind the sums: the frame's header, and the size word - the new size, (uint64_t)-code, or as it came when it came as an error
__global__ void k_recidx_attached(uint8_t *a, const ZsRidxVerdict *__restrict__ verdict, const uint64_t *__restrict__ firstRecord, uint32_t n, uint32_t delim,
                                  const ZsRidxAttach *__restrict__ sums, uint64_t *archiveSize)
{
    if (blockIdx.x || threadIdx.x) return;
    const ZsRidxVerdict v = *verdict;
    if (v.status == ~0u) return;
    if (v.status) { *archiveSize = 0ull - (uint64_t)v.status; return; }
    const uint64_t records = firstRecord[n];
    zs_ridx_write_header(a + v.at, n, delim, records, sums->check + zs_ridx_check_base(records, delim));
    *archiveSize = v.size + zs_ridx_frame_size(n) + v.entry;
}

// ---- host ----
extern "C" size_t zsmi_recordIndexFrameSize(size_t n) { return zs_ridx_size(n); }
extern "C" size_t zsmi_writeRecordIndexFrame(void *dst, size_t dstCapacity, const uint64_t *firstRecord, size_t n, int delim)
{
    return zs_ridx_write(dst, dstCapacity, firstRecord, n, delim);
}
extern "C" size_t zsmi_readRecordIndexFrame(const void *src, size_t srcSize, uint64_t *firstRecord, size_t capacity, int *delim)
{
    return zs_ridx_read(src, srcSize, firstRecord, capacity, delim);
}
extern "C" int zsmi_indexRecords(const void *src, size_t srcSize, const uint32_t *frameSizes, size_t n, int delim, uint64_t *firstRecord, uint64_t *result)
{
    return zs_ridx_index(src, srcSize, frameSizes, n, delim, firstRecord, result);
}
extern "C" size_t zsmi_seekableAttachRecordIndex(void *archive, size_t archiveSize, size_t capacity, const uint64_t *firstRecord, size_t n, int delim)
{
    return zs_ridx_attach(archive, archiveSize, capacity, firstRecord, n, delim);
}
// the tiles of a text and the body's words in the seekable scratch, `head` bytes into it (8-aligned): the scan [tiles + 1], delimiters and
// tails [tiles each].  A text of no bytes has one tile, which holds the place 0.  recidxReserve: that, and the scan's tile sums for
// `scanned` items at least - before anything is queued
struct RecidxTiles { uint32_t tiles; uint64_t *dBase; uint32_t *dCounts, *dTails; };
static size_t recidxTileBytes(size_t tiles) { return (tiles + 1) * sizeof(uint64_t) + 2 * tiles * sizeof(uint32_t); }
static int recidxLay(uint64_t size, void *at, RecidxTiles &t)
{
    const uint64_t tiles64 = std::max<uint64_t>((size + ZS_SPLIT_TILE - 1) / ZS_SPLIT_TILE, 1);
    if (tiles64 > 0x7FFFFFFFull) return ZSMI_error_memory_allocation;
    t.tiles = (uint32_t)tiles64;
    t.dBase = (uint64_t *)at; t.dCounts = (uint32_t *)(t.dBase + t.tiles + 1); t.dTails = t.dCounts + t.tiles;
    return 0;
}
static int recidxReserve(zsmi_ctx *c, uint64_t size, size_t head, uint64_t scanned, RecidxTiles &t)
{
    if (const int e = recidxLay(size, nullptr, t)) return e;
    if (!c->seek.dMeta.reserve(head + recidxTileBytes(t.tiles))) return ZSMI_error_memory_allocation;
    if (!c->dScan.reserve(sizeof(uint64_t) * (size_t)((std::max<uint64_t>(scanned, t.tiles) + ZS_SCAN_TILE - 1) / ZS_SCAN_TILE + 1))) return ZSMI_error_memory_allocation;
    return recidxLay(size, (uint8_t *)c->seek.dMeta.p + head, t);
}
// the launch sequence over dText[0, size), its arguments checked and its scratch reserved by the caller
static int recidxText(zsmi_ctx *c, const void *dText, uint64_t size, const uint64_t *dPlaces, uint32_t n, int delim, int atEnd, const uint64_t *dBase, const uint32_t *dCode,
                      uint64_t *dFirstRecord, uint64_t *dResult, const RecidxTiles &t)
{
    if (const int e = c->fill(dResult + 2, 0, sizeof(uint64_t))) return e;
    LAUNCH(c, "k_recidx_tiles", k_recidx_tiles, dim3(t.tiles), dim3(256), 0, (const uint8_t *)dText, size, (uint32_t)delim, dPlaces, n, t.tiles, t.dCounts, t.dTails);
    if (const int e = scanOffsets(c, "k_recidx_scan", (const uint32_t *)t.dCounts, nullptr, t.tiles, 1u, nullptr, t.dBase)) return e;
    LAUNCH(c, "k_recidx_places", k_recidx_places, dim3(t.tiles), dim3(256), 0, (const uint8_t *)dText, size, (uint32_t)delim, dPlaces, n, atEnd ? 1u : 0u, t.tiles,
           (const uint64_t *)t.dBase, (const uint32_t *)t.dTails, dBase, dCode, dFirstRecord, dResult);
    return c->launched();
}
extern "C" int zsmi_indexRecordsDevice(zsmi_ctx *c, const void *dText, uint64_t size, const uint64_t *dPlaces, uint32_t n, int delim, int atEnd,
                                       const uint64_t *dBase, uint64_t *dFirstRecord, uint64_t *dResult)
{
    if (!c) return ZSMI_error_init_missing;
    if (!dResult || !dPlaces || !dFirstRecord) return ZSMI_error_GENERIC;
    if (delim < 0 || delim > 255) return ZSMI_error_parameter_outOfBound;
    if (n > ZS_RIDX_MAX_FRAMES) return ZSMI_error_frameIndex_tooLarge;
    if (size && !dText) return ZSMI_error_srcSize_wrong;
    if (const int e = c->bind()) return e;
    RecidxTiles t;
    if (const int e = recidxReserve(c, size, 0, 0, t)) return e;
    return recidxText(c, dText, size, dPlaces, n, delim, atEnd, dBase, nullptr, dFirstRecord, dResult, t);
}
// the header's checks of the rebuild on an archive, in its order: seekable.hip's seekWindowCheck with the delimiter as the rule
static int recidxCheck(const zsmi_ctx *c, const zsmi_seekable *sk, int delim, uint32_t firstFrame, uint32_t frameCount, bool ownWork, const void *work, uint64_t workCapacity,
                       const void *firstRecord, const void *result)
{
    return seekWindowCheck(c, sk, !result || !firstRecord, [&] { return delim < 0 || delim > 255 ? (int)ZSMI_error_parameter_outOfBound : 0; }, firstFrame, frameCount, ownWork, work,
                           workCapacity);
}
// the launch sequence on a window, its arguments checked by the caller: findDecode with the body's words behind its own; its layout scan -
// the places of the frames in dWork - is the body's places
static int recidxWindow(zsmi_ctx *c, const zsmi_seekable *sk, int delim, uint32_t firstFrame, uint32_t frameCount, void *dWork, uint64_t *dFirstRecord, uint64_t *dResult)
{
    if (frameCount == 0) return c->fill(dResult, 0, 4 * sizeof(uint64_t));
    RecidxTiles t;
    if (const int e = recidxLay(zsmi_seekableFindWorkBound(sk, firstFrame, frameCount), nullptr, t)) return e;
    FindDecoded w;
    if (const int e = findDecode(c, sk, firstFrame, frameCount, dWork, recidxTileBytes(t.tiles), t.tiles, w)) return e;
    recidxLay(w.bytes, w.dBehind, t);
    const int atEnd = sk->t.dOff[(size_t)firstFrame + frameCount] == sk->t.dOff[sk->t.n];
    return recidxText(c, dWork, w.bytes, w.dListAt, frameCount, delim, atEnd, firstFrame ? dFirstRecord + firstFrame : nullptr, w.dCode, dFirstRecord + firstFrame, dResult, t);
}
extern "C" int zsmi_seekableIndexRecordsResident(zsmi_ctx *c, const zsmi_seekable *sk, int delim, uint32_t firstFrame, uint32_t frameCount, void *dWork, uint64_t workCapacity,
                                                 uint64_t *dFirstRecord, uint64_t *dResult)
{
    if (const int e = recidxCheck(c, sk, delim, firstFrame, frameCount, false, dWork, workCapacity, dFirstRecord, dResult)) return e;
    if (const int e = c->bind()) return e;
    return recidxWindow(c, sk, delim, firstFrame, frameCount, dWork, dFirstRecord, dResult);
}
// Load.  The handle's table says on the host whether the last entry can be an index frame at all - no content, 40 bytes at least; the
// frame's own bytes are judged on the device.  Scratch in the seekable scratch: the sums [32 bytes], the offsets [n + 1], the counts [n]
static int recidxLoad(zsmi_ctx *c, const zsmi_seekable *sk, uint64_t *dFirstRecord, uint64_t *dResult)
{
    const uint32_t N = sk->t.n;
    const bool candidate = N && sk->t.dSize[N - 1] == 0 && sk->t.cSize[N - 1] >= ZS_RIDX_FIXED;
    const uint32_t n = candidate ? N - 1 : 0;
    const uint32_t have = candidate ? (uint32_t)std::min<uint64_t>(n, (sk->t.cSize[N - 1] - ZS_RIDX_FIXED) / 4u) : 0u;      // the counts the frame's bytes hold
    if (!c->seek.dMeta.reserve(sizeof(ZsRidxSums) + ((size_t)n + 1) * sizeof(uint64_t) + (size_t)n * sizeof(uint32_t))) return ZSMI_error_memory_allocation;
    if (!c->dScan.reserve(sizeof(uint64_t) * ((size_t)n / ZS_SCAN_TILE + 2))) return ZSMI_error_memory_allocation;
    ZsRidxSums *dSums = (ZsRidxSums *)c->seek.dMeta.p;
    uint64_t *dOffsets = (uint64_t *)(dSums + 1);
    uint32_t *dCounts = (uint32_t *)(dOffsets + n + 1);
    const uint8_t *frame = candidate ? sk->dFrames + sk->t.cOff[N - 1] : nullptr;
    const uint32_t grid = std::max(1u, std::min((n + 255u) / 256u, 4096u));
    if (candidate) {
        if (const int e = c->fill(dSums, 0, sizeof(ZsRidxSums))) return e;
        if (have < n) if (const int e = c->fill(dCounts, 0, (size_t)n * sizeof(uint32_t))) return e;
        if (have) LAUNCH(c, "k_recidx_unpack", k_recidx_unpack, dim3(grid), dim3(256), 0, frame, have, (const ZsSeekEntry *)sk->dTable.p, dCounts, dSums);
        if (const int e = scanOffsets(c, "k_recidx_scan", (const uint32_t *)dCounts, nullptr, n, 1u, nullptr, dOffsets)) return e;
    }
    LAUNCH(c, "k_recidx_loaded", k_recidx_loaded, dim3(grid), dim3(256), 0, frame, n, sk->t.cSize.empty() || !candidate ? 0u : (sk->t.cSize[N - 1] == zs_ridx_frame_size(n) ? 1u : 0u),
           (const ZsRidxSums *)dSums, (const uint64_t *)dOffsets, dFirstRecord, dResult);
    return c->launched();
}
extern "C" int zsmi_seekableLoadRecordIndexResident(zsmi_ctx *c, const zsmi_seekable *sk, uint64_t *dFirstRecord, uint64_t *dResult)
{
    if (!c) return ZSMI_error_init_missing;
    if (!sk || !dResult || !dFirstRecord) return ZSMI_error_GENERIC;
    if (sk->device != c->device) return ZSMI_error_parameter_unsupported;
    if (const int e = c->bind()) return e;
    return recidxLoad(c, sk, dFirstRecord, dResult);
}
// Attach.  Scratch in the seekable scratch: the sums and the verdict, then the table's entries (12 bytes a frame at most)
extern "C" int zsmi_seekableAttachRecordIndexResident(zsmi_ctx *c, void *dArchive, uint64_t capacity, uint64_t *dArchiveSize, const uint64_t *dFirstRecord, uint32_t n, int delim)
{
    if (!c) return ZSMI_error_init_missing;
    if (!dArchive || !dArchiveSize || !dFirstRecord) return ZSMI_error_GENERIC;
    if (delim < 0 || delim > 255) return ZSMI_error_parameter_outOfBound;
    if (n > ZS_RIDX_MAX_FRAMES) return ZSMI_error_frameIndex_tooLarge;
    if (const int e = c->bind()) return e;
    if (!c->seek.dMeta.reserve(sizeof(ZsRidxAttach) + sizeof(ZsRidxVerdict) + (size_t)n * 12 + 16)) return ZSMI_error_memory_allocation;
    ZsRidxAttach *dSums = (ZsRidxAttach *)c->seek.dMeta.p;
    ZsRidxVerdict *dVerdict = (ZsRidxVerdict *)(dSums + 1);
    uint8_t *dKeep = (uint8_t *)(dVerdict + 1);
    const uint32_t grid = std::max(1u, std::min((n + 255u) / 256u, 4096u));
    if (const int e = c->fill(dSums, 0, sizeof(ZsRidxAttach))) return e;
    LAUNCH(c, "k_recidx_table_out", k_recidx_table_out, dim3(grid), dim3(256), 0, (const uint8_t *)dArchive, capacity, (const uint64_t *)dArchiveSize, dFirstRecord, n, dKeep, dSums);
    LAUNCH(c, "k_recidx_verdict", k_recidx_verdict, dim3(1), dim3(64), 0, (const uint8_t *)dArchive, capacity, (const uint64_t *)dArchiveSize, dFirstRecord, n,
           (const uint8_t *)dKeep, (const ZsRidxAttach *)dSums, dVerdict);
    LAUNCH(c, "k_recidx_pack", k_recidx_pack, dim3(grid), dim3(256), 0, (uint8_t *)dArchive, (const ZsRidxVerdict *)dVerdict, dFirstRecord, n, (const uint8_t *)dKeep, dSums);
    LAUNCH(c, "k_recidx_attached", k_recidx_attached, dim3(1), dim3(64), 0, (uint8_t *)dArchive, (const ZsRidxVerdict *)dVerdict, dFirstRecord, n, (uint32_t)delim,
           (const ZsRidxAttach *)dSums, dArchiveSize);
    return c->launched();
}
// ---- host arrays ----
// the handle's index frame -> firstRecord[0 .. N] (host, N = the handle's frames) and result[4]: the resident call into context staging, the
// words and - behind a good status - the array copied back behind one wait
extern "C" int zsmi_seekableLoadRecordIndexHost(zsmi_ctx *c, const zsmi_seekable *sk, uint64_t *firstRecord, uint64_t *result)
{
    if (!c) return ZSMI_error_init_missing;
    if (!sk || !result || !firstRecord) return ZSMI_error_GENERIC;
    if (sk->device != c->device) return ZSMI_error_parameter_unsupported;
    if (const int e = c->bind()) return e;
    const size_t words = (size_t)sk->t.n + 1;
    if (!c->sSizes.reserve((words + 4) * sizeof(uint64_t))) return ZSMI_error_memory_allocation;
    uint64_t *dFirst = (uint64_t *)c->sSizes.p, *dResult = dFirst + words;
    std::vector<uint64_t> staged(words);
    int rc = recidxLoad(c, sk, dFirst, dResult);
    if (!rc) rc = c->toHost(result, dResult, 4 * sizeof(uint64_t));
    if (!rc) rc = c->toHost(staged.data(), dFirst, words * sizeof(uint64_t));
    const int waited = c->wait();
    if (rc || waited) return rc ? rc : waited;
    if (result[0] == 0) memcpy(firstRecord, staged.data(), words * sizeof(uint64_t));
    return 0;
}
// the rebuild over the whole archive -> firstRecord[0 .. N] (host) and result[4] = {the first failing frame's code, records, misaligned
// frames, delimiters}: seekable.hip's window plan, the windows in ascending order on the stream - they chain through the array in context
// staging -, a work buffer of the context's, one wait
extern "C" int zsmi_seekableIndexRecordsHost(zsmi_ctx *c, const zsmi_seekable *sk, int delim, uint64_t *firstRecord, uint64_t *result)
{
    if (const int e = recidxCheck(c, sk, delim, 0, 0, true, nullptr, 0, firstRecord, result)) return e;
    if (const int e = c->bind()) return e;
    const uint32_t N = sk->t.n;
    const SeekWindows plan = seekCutWindows(sk, seekWindowLimit());
    // every window's scratch at once, before the first is queued: the largest text, the most frames
    const size_t W = plan.list.size(), words = (size_t)N + 1 + 4 * std::max<size_t>(W, 1);
    RecidxTiles most;
    if (const int e = recidxLay(plan.most, nullptr, most)) return e;
    if (!c->sSizes.reserve(words * sizeof(uint64_t)) || !c->seek.dDec.reserve(plan.most + 64)) return ZSMI_error_memory_allocation;
    if (const int e = findDecodeReserve(c, plan.mostFrames, recidxTileBytes(most.tiles), most.tiles)) return e;
    uint64_t *dFirst = (uint64_t *)c->sSizes.p, *dResults = dFirst + N + 1;
    std::vector<uint64_t> staged((size_t)N + 1), results(4 * std::max<size_t>(W, 1), 0);
    int rc = 0;
    if (N == 0) rc = c->fill(dFirst, 0, sizeof(uint64_t));
    for (size_t k = 0; k < W && !rc; k++) rc = recidxWindow(c, sk, delim, plan.list[k].first, plan.list[k].second, c->seek.dDec.p, dFirst, dResults + 4 * k);
    if (!rc && W) rc = c->toHost(results.data(), dResults, 4 * W * sizeof(uint64_t));
    if (!rc) rc = c->toHost(staged.data(), dFirst, ((size_t)N + 1) * sizeof(uint64_t));
    const int waited = c->wait();
    if (rc || waited) return rc ? rc : waited;
    result[0] = result[2] = result[3] = 0;
    for (size_t k = 0; k < W; k++) { if (!result[0]) result[0] = results[4 * k]; result[2] += results[4 * k + 2]; result[3] += results[4 * k + 3]; }
    result[1] = staged[N];
    memcpy(firstRecord, staged.data(), ((size_t)N + 1) * sizeof(uint64_t));
    return 0;
}
