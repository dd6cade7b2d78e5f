// dict_train.hip -- dictionary training on the GPU: zstd's fastCover trainer and ZDICT_finalizeDictionary, over the batch compressor of
// zsmi_api.hip (zsmi_ctx.h declares it).
//
//   frequencies  k_train_freq:    every d-mer of the training samples hashed to f bits (zstd's 6- / 8-byte multiplicative hash); the d-mers that
//                                 lie inside their sample (8 bytes readable) are counted into a 2^f table by integer atomics (order-independent)
//   links        radix sort of (hash << 32 | position), k_train_links: per position the distance to the previous and the next position of the
//                                 same hash (capped at 65535 = none within reach)
//   segments     k_train_select:  one workgroup a candidate (k, d); epochs one after the other inside it.  An epoch scores every window end e at
//                                 once: score(e) - score(e - 1) depends only on the d-mer entering (e - 1) and the one leaving (e - L - 1) and on
//                                 whether their hash occurs again inside the window, so the scores are a prefix sum of per-position deltas and the
//                                 segment is the first argmax.  Its d-mers' frequencies are zeroed on the device and its bytes fill the content from
//                                 the end.  Only the content's start (one word a candidate) is read back.
//   search       each candidate's content is a raw dictionary for the batch compressor over the held-out samples; the smallest total wins
//   finalize     the samples compressed with the content (compressBatchDeviceImpl with a stats pointer): k_train_stats (entropy_kernels.hip) counts literal bytes and
//                                 LL / OF / ML codes; k_train_id hashes the content (XXH64) into the dictionary ID; k_train_tables builds the
//                                 Huffman description and the three NCounts with the encoder's routines and assembles the dictionary.
#include <hipcub/hipcub.hpp>      // the radix sort of the d-mer keys
#include "zsmi_wave.h"            // zs_block_copy, xxh64_quad, rd32
#include "entropy_kernels.hip"    // k_train_stats and kTrainStatWords; the encoder's routines k_train_tables builds with (K3Lds, huffLengths,
                                  // huffCodesAndWeights, writeHuffHeaderWave, normalizeCountsWave, writeNCount)
#include "zsmi_fse.h"             // MaxLL, MaxML, MaxOff, LLFSELog, MLFSELog, OffFSELog
#include "zsmi_status.h"          // the size word of the scoring calls' frames
#include "zsmi_ctx.h"
#include <algorithm>

static const uint32_t kTrainDefaultF = 20, kTrainMinF = 12, kTrainMaxF = 26;
static const uint32_t kTrainDictSizeMin = 256, kTrainContentMin = 128;       // ZDICT_DICTSIZE_MIN, ZDICT_CONTENTSIZE_MIN
static const uint32_t kTrainMaxZeroRun = 10;                                 // epochs in a row without a segment end the content (zstd >= 1.4.5)
static const uint32_t kTrainThreads = 1024, kTrainPerThread = 8;            // k_train_select: window ends a thread scores per tile

struct ZsTrainCand { uint32_t k, d, pad0, pad1; uint32_t *freq; uint8_t *content; };

__device__ __forceinline__ uint32_t train_hash(const uint8_t *p, uint32_t d, uint32_t f)
{
    const uint64_t v = zs_load64(p);
    if (d == 6) return (uint32_t)(((v << 16) * 227718039650203ull) >> (64 - f));      // ZSTD_hash6Ptr
    return (uint32_t)((v * 0xCF1BBCDCB7A56463ull) >> (64 - f));                          // ZSTD_hash8Ptr
}

// one thread a d-mer start p < nbDmers: its hash (info.x), its sort key, and its count if its 8 bytes lie inside its sample (ends: the training
// samples' end offsets)
__global__ void k_train_freq(const uint8_t *__restrict__ samples, uint32_t nbDmers, uint32_t d, uint32_t f, const uint64_t *__restrict__ ends, uint32_t nTrain,
                             uint2 *__restrict__ info, uint64_t *__restrict__ keys, uint32_t *__restrict__ freq)
{
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= nbDmers) return;
    const uint32_t h = train_hash(samples + p, d, f);
    info[p] = make_uint2(h, 0u);
    keys[p] = ((uint64_t)h << 32) | p;
    uint32_t lo = 0, hi = nTrain;
    while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (ends[mid] <= p) lo = mid + 1; else hi = mid; }
    if (lo < nTrain && (uint64_t)p + 8 <= ends[lo]) atomicAdd(&freq[h], 1u);
}

// sorted keys -> per position: distance to the previous (low 16 bits) and the next (high 16 bits) position of the same hash; 65535 = none nearer
__global__ void k_train_links(const uint64_t *__restrict__ sorted, uint32_t n, uint2 *__restrict__ info)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t key = sorted[i];
    const uint32_t h = (uint32_t)(key >> 32), p = (uint32_t)key;
    uint32_t dp = 65535u, dn = 65535u;
    if (i > 0) { const uint64_t o = sorted[i - 1]; if ((uint32_t)(o >> 32) == h) dp = min(p - (uint32_t)o, 65535u); }
    if (i + 1 < n) { const uint64_t o = sorted[i + 1]; if ((uint32_t)(o >> 32) == h) dn = min((uint32_t)o - p, 65535u); }
    info[p].y = dp | (dn << 16);
}

// exclusive prefix sum of one int64 a thread over the workgroup (kTrainThreads); *total: the sum of all
__device__ __forceinline__ int64_t train_block_scan(int64_t v, int64_t *lds, int64_t &total)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    int64_t x = v;
    #pragma unroll
    for (uint32_t o = 1; o < 64; o <<= 1) { const int64_t y = __shfl_up(x, o); if (lane >= o) x += y; }
    if (lane == 63) lds[wave] = x;
    __syncthreads();
    if (wave == 0) {
        int64_t w = lane < kTrainThreads / 64 ? lds[lane] : 0;
        #pragma unroll
        for (uint32_t o = 1; o < kTrainThreads / 64; o <<= 1) { const int64_t y = __shfl_up(w, o); if (lane >= o) w += y; }
        if (lane < kTrainThreads / 64) lds[16 + lane] = w;
    }
    __syncthreads();
    const int64_t before = wave ? lds[16 + wave - 1] : 0;
    total = lds[16 + kTrainThreads / 64 - 1];
    __syncthreads();
    return before + x - v;
}
__device__ __forceinline__ bool train_better(int64_t s, uint32_t e, int64_t bs, uint32_t be) { return s > bs || (s == bs && e < be); }

// one workgroup a candidate: the whole epoch loop of FASTCOVER_buildDictionary.  Epochs: num = max(1, cap / k / 4), size = nbDmers / num, and at
// least 10 k d-mers an epoch (then num = nbDmers / size); they are visited in turn until the content is full or kTrainMaxZeroRun epochs in a row
// have no segment of positive score.  The window of end e holds the d-mers [max(eb, e - L), e), L = k - d + 1; its score is the summed frequency
// of its distinct hashes.  tails[c]: where the candidate's content starts in its buffer of cap bytes.
__global__ void __launch_bounds__(kTrainThreads) k_train_select(const uint2 *__restrict__ info6, const uint2 *__restrict__ info8, const uint8_t *__restrict__ samples,
                                                                uint32_t nbDmers, uint32_t cap, const ZsTrainCand *__restrict__ cands, uint32_t *__restrict__ tails)
{
    __shared__ int64_t scan[32];
    __shared__ int64_t redS[16];
    __shared__ uint32_t redE[16], seg[2];
    const ZsTrainCand C = cands[blockIdx.x];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t k = C.k, d = C.d, L = k - d + 1;
    const uint2 *info = d == 6 ? info6 : info8;
    uint32_t *freq = C.freq;
    uint8_t *content = C.content;
    uint32_t num = max(1u, cap / k / 4u), size = nbDmers / num;
    if ((uint64_t)size < 10ull * k) { size = (uint32_t)min<uint64_t>(10ull * k, nbDmers); num = nbDmers / size; }
    uint32_t tail = cap, zeroRun = 0;
    for (uint32_t epoch = 0; tail > 0; epoch = (epoch + 1) % num) {
        const uint64_t eb = (uint64_t)epoch * size, ee = eb + size;
        int64_t carry = 0, best = 0;
        uint32_t bestE = 0xFFFFFFFFu;
        for (uint64_t base = eb + 1; base <= ee; base += kTrainThreads * kTrainPerThread) {
            int64_t part[kTrainPerThread], run = 0;
            #pragma unroll
            for (uint32_t v = 0; v < kTrainPerThread; v++) {
                const uint64_t e = base + tid * kTrainPerThread + v;
                int64_t x = 0;
                if (e <= ee) {
                    const uint64_t j = e - 1, be = e >= eb + L ? e - L : eb;
                    const uint2 a = info[j];
                    if ((a.y & 0xFFFFu) > j - be) x += freq[a.x];                   // entering: no earlier occurrence inside the window
                    if (e >= eb + L + 1) {
                        const uint2 q = info[e - L - 1];
                        if ((q.y >> 16) >= L) x -= freq[q.x];                        // leaving: no later occurrence inside the window
                    }
                }
                run += x; part[v] = run;
            }
            int64_t total;
            const int64_t before = train_block_scan(run, scan, total);
            #pragma unroll
            for (uint32_t v = 0; v < kTrainPerThread; v++) {
                const uint64_t e = base + tid * kTrainPerThread + v;
                const int64_t s = carry + before + part[v];
                if (e <= ee && s > best) { best = s; bestE = (uint32_t)e; }
            }
            carry += total;
        }
        // first window end of the largest score
        #pragma unroll
        for (uint32_t o = 32; o >= 1; o >>= 1) {
            const int64_t s = __shfl_xor(best, o); const uint32_t e = (uint32_t)__shfl_xor((int)bestE, o);
            if (train_better(s, e, best, bestE)) { best = s; bestE = e; }
        }
        if (lane == 0) { redS[wave] = best; redE[wave] = bestE; }
        __syncthreads();
        if (tid == 0) {
            for (uint32_t w = 1; w < kTrainThreads / 64; w++) if (train_better(redS[w], redE[w], redS[0], redE[0])) { redS[0] = redS[w]; redE[0] = redE[w]; }
            seg[0] = 0xFFFFFFFFu; seg[1] = 0;
        }
        __syncthreads();
        best = redS[0]; bestE = redE[0];
        __syncthreads();
        if (best <= 0) { if (++zeroRun >= kTrainMaxZeroRun) break; continue; }
        zeroRun = 0;
        // the segment without its zero-frequency head and tail, then its d-mers' frequencies zeroed
        const uint32_t sb = bestE >= eb + L ? bestE - L : (uint32_t)eb;
        for (uint32_t p = sb + tid; p < bestE; p += kTrainThreads)
            if (freq[info[p].x]) { atomicMin(&seg[0], p); atomicMax(&seg[1], p + 1); }
        __syncthreads();
        const uint32_t nb = seg[0], ne = seg[1];
        for (uint32_t p = nb + tid; p < ne; p += kTrainThreads) freq[info[p].x] = 0;
        const uint32_t segSize = min(ne - nb + d - 1, tail);
        __syncthreads();
        if (segSize < d) break;
        tail -= segSize;
        for (uint32_t i = tid; i < segSize; i += kTrainThreads) content[tail + i] = samples[nb + i];
        __syncthreads();
    }
    if (tid == 0) tails[blockIdx.x] = tail;
}

// the dictionary ID: the caller's, or XXH64(content) % ((1 << 31) - 32768) + 32768 as ZDICT derives it
__global__ void __launch_bounds__(64) k_train_id(const uint8_t *__restrict__ content, uint32_t size, uint32_t given, uint32_t *__restrict__ id)
{
    const uint64_t h = xxh64_quad<16>(content, size);                  // (every lane of a quad calls)
    if (threadIdx.x == 0) *id = given ? given : (uint32_t)(h % 2147450880ull) + 32768u;
}

// counts + 1 (every symbol representable), halved until their sum is below `limit`, never below 1
__device__ static uint32_t train_scaled(const uint32_t *raw, uint32_t n, uint32_t *out, uint64_t limit)
{
    uint64_t total = 0;
    for (uint32_t s = 0; s < n; s++) total += (uint64_t)raw[s] + 1;
    uint32_t shift = 0;
    while ((total >> shift) >= limit) shift++;
    uint32_t sum = 0;
    for (uint32_t s = 0; s < n; s++) { out[s] = max(1u, (uint32_t)(((uint64_t)raw[s] + 1) >> shift)); sum += out[s]; }
    return sum;
}

// one workgroup of 256: the entropy section (Huffman description of <= 11 bits, NCounts OF 8 / ML 9 / LL 9), the recent offsets {1, 4, 8},
// then the content behind it, cut at its front to fit cap.  hdr: 1 KiB of scratch.  result[0]: the dictionary's size, 0 if it cannot be made.
__global__ void __launch_bounds__(256) k_train_tables(const uint32_t *__restrict__ stats, const uint8_t *__restrict__ content, uint32_t contentSize, uint32_t cap,
                                                      const uint32_t *__restrict__ dictID, uint8_t *__restrict__ hdr, uint8_t *__restrict__ out, uint32_t *__restrict__ result)
{
    __shared__ K3Lds L;
    __shared__ uint32_t cnt[64], misc[4];           // misc[0]: the Huffman description's size, misc[1]: the entropy section's size (0: no dictionary);
                                                    // not K3Lds's L.misc, two slots of which carry values from lane 0 to wavefront 0 below
    __shared__ int16_t norm[64];
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    const uint32_t hcap = 1024;
    if (tid == 0) { misc[0] = 0; misc[1] = 0; train_scaled(stats, 256, L.count, 1u << 23); }   // (package-merge keys are count << 8 | symbol)
    __syncthreads();
    const uint32_t lit = L.count[tid];
    for (uint32_t maxBits = ZS_HUF_MAXBITS; maxBits >= 8; maxBits--) {     // a description over 127 bytes: flatter codes
        L.count[tid] = lit;
        __syncthreads();
        const uint32_t tableLog = huffLengths(L, 255, maxBits);
        huffCodesAndWeights(L, 255, tableLog);
        if (wave == 0) { const uint32_t hs = writeHuffHeaderWave(L, hdr + 8, 256, 255, tableLog); if (lane == 0) misc[0] = hs; }
        __syncthreads();
        if (misc[0]) break;
        __syncthreads();
    }
    if (wave == 0 && misc[0]) {                     // wavefront 0: counts scaled and written by lane 0, normalised by all lanes
        uint32_t pos = 8 + misc[0];
        const uint32_t ofMax = zs_highbit(contentSize + (128u << 10));
        const uint32_t maxes[3] = { min(ofMax, (uint32_t)MaxOff), MaxML, MaxLL }, logs[3] = { OffFSELog, MLFSELog, LLFSELog }, base[3] = { 320, 384, 256 };
        bool ok = true;
        uint32_t &scaledTotal = L.misc[0], &ncountBytes = L.misc[1];       // lane 0 -> all lanes (the literals workspace is free by now)
        for (uint32_t t = 0; t < 3 && ok; t++) {
            if (lane == 0) scaledTotal = train_scaled(stats + base[t], maxes[t] + 1, cnt, 1u << 30);
            wave_sync();
            normalizeCountsWave(norm, logs[t], cnt, scaledTotal, maxes[t]);
            if (lane == 0) ncountBytes = writeNCount(hdr + pos, hcap - pos, norm, maxes[t], logs[t]);
            wave_sync();
            const uint32_t w = ncountBytes;
            ok = w != 0; pos += w;
        }
        ok = ok && pos + 12 <= hcap;
        if (lane == 0) {
            const uint32_t id = *dictID, words[5] = { 0xEC30A437u, id, 1u, 4u, 8u };
            for (uint32_t i = 0; i < 2; i++) zs_store32(hdr + 4 * i, words[i]);
            if (ok) for (uint32_t i = 0; i < 3; i++) zs_store32(hdr + pos + 4 * i, words[2 + i]);
            pos += 12;
            misc[1] = (ok && pos <= hcap && pos < cap) ? pos : 0u;
        }
    }
    __syncthreads();
    const uint32_t hs = misc[1];
    if (!hs) { if (tid == 0) *result = 0; return; }
    const uint32_t keep = min(contentSize, cap - hs);
    for (uint32_t i = tid; i < hs; i += 256) out[i] = hdr[i];
    zs_block_copy(out + hs, content + (contentSize - keep), keep, tid, 256);
    if (tid == 0) *result = hs + keep;
}

// samples at scattered offsets -> back to back (one workgroup a sample)
__global__ void k_train_gather(const uint8_t *__restrict__ src, const uint64_t *__restrict__ offs /* [0, n): from, [n, 2n): to */, const uint32_t *__restrict__ sizes,
                               uint32_t n, uint8_t *__restrict__ dst)
{
    const uint32_t i = blockIdx.x;
    zs_block_copy(dst + offs[n + i], src + offs[i], sizes[i], threadIdx.x, blockDim.x);
}

// ---- host ----
extern "C" unsigned zsmi_getDictID(const void *dict, size_t dictSize)
{
    const uint8_t *d = (const uint8_t *)dict;
    if (!d || dictSize < 8 || rd32(d) != 0xEC30A437u) return 0;
    return rd32(d + 4);
}

namespace {
struct TrainPlan {
    uint32_t f = kTrainDefaultF, steps = 40;
    int level = 3;
    double split = 0.75;
    std::vector<std::pair<uint32_t, uint32_t>> cands;          // (k, d)
    bool search = false;
};
}

// the parameters the trainer runs with, or an error code; total: the samples' bytes
static int trainParams(const zsmi_fastCoverParams *p, size_t cap, uint64_t total, uint32_t nb, TrainPlan &t)
{
    if (cap < kTrainDictSizeMin) return ZSMI_error_dstSize_tooSmall;
    if (!p) return ZSMI_error_GENERIC;
    if (p->d != 0 && p->d != 6 && p->d != 8) return ZSMI_error_parameter_outOfBound;
    if (p->f != 0 && (p->f < kTrainMinF || p->f > kTrainMaxF)) return ZSMI_error_parameter_outOfBound;
    if (p->accel > 1) return ZSMI_error_parameter_outOfBound;
    if (!(p->splitPoint == 0.0 || (p->splitPoint > 0.0 && p->splitPoint <= 1.0))) return ZSMI_error_parameter_outOfBound;
    if (p->k != 0 && (p->k < (p->d ? p->d : 8u) || p->k > cap || p->k > 65536u)) return ZSMI_error_parameter_outOfBound;
    if (nb == 0 || total < 8 || total >= (1ull << 32)) return ZSMI_error_srcSize_wrong;
    t.f = p->f ? p->f : kTrainDefaultF;
    t.steps = p->steps ? p->steps : 40;
    t.split = p->splitPoint > 0.0 ? p->splitPoint : 0.75;
    t.level = p->level ? p->level : 3;
    t.search = p->k == 0 || p->d == 0;
    std::vector<uint32_t> ds, ks;
    if (p->d) ds.push_back(p->d); else { ds.push_back(6); ds.push_back(8); }
    if (p->k) ks.push_back(p->k);
    else {
        const uint32_t step = std::max<uint32_t>((2000 - 50) / t.steps, 1);             // ZDICT_optimizeTrainFromBuffer_fastCover's k range
        for (uint32_t k = 50; k <= 2000; k += step) if (k <= cap) ks.push_back(k);
    }
    for (uint32_t d : ds) for (uint32_t k : ks) if (k >= d) t.cands.push_back({ k, d });
    if (t.cands.empty()) return ZSMI_error_parameter_outOfBound;
    return 0;
}

static int trainLaunchSort(zsmi_ctx *c, uint32_t n, uint32_t f)
{
    size_t tmp = 0;
    if (hipcub::DeviceRadixSort::SortKeys(nullptr, tmp, (const uint64_t *)nullptr, (uint64_t *)nullptr, (int)n, 0, 32 + (int)f, c->stream) != hipSuccess) return ZSMI_error_GENERIC;
    if (!c->train.dSortTmp.reserve(tmp)) return ZSMI_error_memory_allocation;
    Timed timed(c, "radix_sort");
    return hipcub::DeviceRadixSort::SortKeys(c->train.dSortTmp.p, tmp, (const uint64_t *)c->train.dKeys.p, (uint64_t *)c->train.dKeysOut.p, (int)n, 0, 32 + (int)f, c->stream) == hipSuccess ? 0 : ZSMI_error_GENERIC;
}

// content (device, contentSize bytes) + the samples (device, back to back at offs / sizes) -> a formatted dictionary at dOut (device, cap bytes);
// *dResult (device): its size or 0.  Asynchronous.
static int finalizeQueue(zsmi_ctx *c, const uint8_t *dSamples, const std::vector<uint64_t> &offs, const std::vector<uint32_t> &sizes, const uint8_t *dContent,
                         uint32_t contentSize, uint32_t cap, int level, uint32_t dictID, uint8_t *dOut, uint32_t *dResult)
{
    const uint32_t n = (uint32_t)sizes.size();
    std::vector<uint64_t> dof(n);
    uint64_t at = 0;
    for (uint32_t i = 0; i < n; i++) { dof[i] = at; at += zsmi_compressBound(sizes[i]); }
    if (!c->train.dArena.reserve(at + 64) || !c->train.dMisc.reserve(sizeof(uint32_t) * (kTrainStatWords + 8) + 1024) || !c->train.dSizes.reserve(sizeof(uint32_t) * n + 64)) return ZSMI_error_memory_allocation;
    uint32_t *dStats = (uint32_t *)c->train.dMisc.p, *dId = dStats + kTrainStatWords;
    uint8_t *dHdr = (uint8_t *)(dId + 8);
    if (const int e = c->fill(dStats, 0, sizeof(uint32_t) * kTrainStatWords)) return e;
    ZsCDictSel dict;
    if (const int e = dictFromBytes(c, dContent, contentSize, kDictContent, level, n, dict)) return e;
    if (const int e = compressBatchDeviceImpl(c, dSamples, offs.data(), sizes.data(), n, c->train.dArena.p, dof.data(), (uint32_t *)c->train.dSizes.p, level, &dict, 0, dStats)) return e;
    LAUNCH(c, "k_train_id", k_train_id, dim3(1), dim3(64), 0, dContent, contentSize, dictID, dId);
    LAUNCH(c, "k_train_tables", k_train_tables, dim3(1), dim3(256), 0, (const uint32_t *)dStats, dContent, contentSize, cap, (const uint32_t *)dId, dHdr, dOut, dResult);
    return c->launched();
}

// what finalizeQueue left: *dResult, the dictionary's size (0: it could not be made), then the dictionary from c->train.dOut -> hostDict
static int finalizeFetch(zsmi_ctx *c, const uint32_t *dResult, void *hostDict, size_t *dictSize)
{
    uint32_t size = 0;
    if (c->toHost(&size, dResult, sizeof size) || c->wait()) return ZSMI_error_GENERIC;
    if (!size) return ZSMI_error_dstSize_tooSmall;
    if (hipMemcpy(hostDict, c->train.dOut.p, size, hipMemcpyDeviceToHost) != hipSuccess) return ZSMI_error_GENERIC;
    *dictSize = size; return 0;
}
// samples back to back in device memory (sizes on the host) -> the dictionary in hostDict; the chosen k, d go back into *params
static int trainImpl(zsmi_ctx *c, const uint8_t *dSamples, const std::vector<uint32_t> &sizes, void *hostDict, size_t cap, zsmi_fastCoverParams *params, size_t *dictSize)
{
    const uint32_t n = (uint32_t)sizes.size();
    uint64_t total = 0;
    for (uint32_t s : sizes) total += s;
    TrainPlan t;
    if (const int e = trainParams(params, cap, total, n, t)) return e;
    if (!hostDict) return ZSMI_error_GENERIC;
    if (const int e = c->bind()) return e;
    const uint32_t cap32 = (uint32_t)std::min<size_t>(cap, 0xFFFFFFFFu - 4096);
    // training share: the first split of the samples while searching (at least one, and at least 8 bytes), all of them otherwise
    uint32_t nTrain = n;
    if (t.search && t.split < 1.0) nTrain = std::max<uint32_t>(1, (uint32_t)(n * t.split));
    uint64_t trainBytes = 0;
    for (uint32_t i = 0; i < nTrain; i++) trainBytes += sizes[i];
    if (trainBytes < 8) { nTrain = n; trainBytes = total; }
    const uint32_t nbDmers = (uint32_t)(trainBytes - 7);
    std::vector<uint64_t> offs(n), ends(nTrain);
    { uint64_t at = 0; for (uint32_t i = 0; i < n; i++) { offs[i] = at; at += sizes[i]; if (i < nTrain) ends[i] = at; } }
    // d-mer hashes, counts and links, once per d
    const size_t table = (size_t)4 << t.f;
    bool needD[2] = { false, false };
    for (auto &kd : t.cands) needD[kd.second == 8] = true;
    if (!c->train.dKeys.reserve((size_t)8 * nbDmers) || !c->train.dKeysOut.reserve((size_t)8 * nbDmers) || !c->train.dEnds.reserve(8 * (size_t)nTrain) || !c->train.dFreqBase.reserve(2 * table)) return ZSMI_error_memory_allocation;
    for (int w = 0; w < 2; w++) if (needD[w] && !c->train.dInfo[w].reserve((size_t)8 * nbDmers)) return ZSMI_error_memory_allocation;
    if (const int e = c->toDevice(c->train.dEnds.p, ends.data(), 8 * (size_t)nTrain)) return e;
    if (const int e = c->fill(c->train.dFreqBase.p, 0, 2 * table)) return e;
    for (int w = 0; w < 2; w++) {
        if (!needD[w]) continue;
        uint32_t *freqBase = (uint32_t *)((uint8_t *)c->train.dFreqBase.p + w * table);
        LAUNCH(c, "k_train_freq", k_train_freq, dim3((nbDmers + 255) / 256), dim3(256), 0, dSamples, nbDmers, w ? 8u : 6u, t.f, (const uint64_t *)c->train.dEnds.p, nTrain,
               (uint2 *)c->train.dInfo[w].p, (uint64_t *)c->train.dKeys.p, freqBase);
        if (const int e = trainLaunchSort(c, nbDmers, t.f)) return e;
        LAUNCH(c, "k_train_links", k_train_links, dim3((nbDmers + 255) / 256), dim3(256), 0, (const uint64_t *)c->train.dKeysOut.p, nbDmers, (uint2 *)c->train.dInfo[w].p);
    }
    // the candidates, in groups whose frequency tables fit 2 GiB
    const uint32_t nc = (uint32_t)t.cands.size();
    const uint32_t group = (uint32_t)std::max<size_t>(1, std::min<size_t>(nc, ((size_t)2 << 30) / table));
    if (!c->train.dFreq.reserve(table * group) || !c->train.dContent.reserve((size_t)cap32 * nc) || !c->train.dCand.reserve(sizeof(ZsTrainCand) * nc + sizeof(uint32_t) * nc)) return ZSMI_error_memory_allocation;
    if (const int e = c->idleReserve({ { &c->train.hCand, sizeof(ZsTrainCand) * nc + sizeof(uint32_t) * nc } })) return e;      // (the pinned candidate list may feed an earlier copy)
    ZsTrainCand *hc = (ZsTrainCand *)c->train.hCand.p;
    uint32_t *dTails = (uint32_t *)((ZsTrainCand *)c->train.dCand.p + nc);
    for (uint32_t i = 0; i < nc; i++) {
        hc[i].k = t.cands[i].first; hc[i].d = t.cands[i].second; hc[i].pad0 = hc[i].pad1 = 0;
        hc[i].freq = (uint32_t *)((uint8_t *)c->train.dFreq.p + table * (i % group));
        hc[i].content = (uint8_t *)c->train.dContent.p + (size_t)cap32 * i;
    }
    if (const int e = c->toDevice(c->train.dCand.p, hc, sizeof(ZsTrainCand) * nc)) return e;
    for (uint32_t g0 = 0; g0 < nc; g0 += group) {
        const uint32_t g1 = std::min(nc, g0 + group);
        for (uint32_t i = g0; i < g1; i++)
            if (const int e = c->onDevice(hc[i].freq, (uint8_t *)c->train.dFreqBase.p + (hc[i].d == 8) * table, table)) return e;
        LAUNCH(c, "k_train_select", k_train_select, dim3(g1 - g0), dim3(kTrainThreads), 0, (const uint2 *)c->train.dInfo[0].p, (const uint2 *)c->train.dInfo[1].p, dSamples, nbDmers, cap32,
               (const ZsTrainCand *)c->train.dCand.p + g0, dTails + g0);
    }
    uint32_t *hTails = (uint32_t *)(hc + nc);
    if (c->toHost(hTails, dTails, sizeof(uint32_t) * nc) || c->wait()) return ZSMI_error_GENERIC;
    uint32_t win = 0;
    if (nc > 1) {
        // each candidate as raw content for the held-out samples (the samples behind the training share; all of them if there are none)
        const uint32_t t0 = nTrain < n ? nTrain : 0, nt = n - t0;
        std::vector<uint64_t> so(offs.begin() + t0, offs.end()), dof(nt);
        std::vector<uint32_t> ss(sizes.begin() + t0, sizes.end());
        uint64_t at = 0;
        for (uint32_t i = 0; i < nt; i++) { dof[i] = at; at += zsmi_compressBound(ss[i]); }
        if (!c->train.dArena.reserve(at + 64) || !c->train.dSizes.reserve(sizeof(uint32_t) * (size_t)nt * nc + 64)) return ZSMI_error_memory_allocation;
        for (uint32_t i = 0; i < nc; i++) {
            ZsCDictSel dict;                                                    // (no content: the plain call)
            if (const int e = dictFromBytes(c, hc[i].content + hTails[i], cap32 - hTails[i], kDictContent, t.level, nt, dict)) return e;
            uint32_t *dSizes = (uint32_t *)c->train.dSizes.p + (size_t)nt * i;
            if (const int e = compressBatchDeviceImpl(c, dSamples, so.data(), ss.data(), nt, c->train.dArena.p, dof.data(), dSizes, t.level, &dict, 0)) return e;
        }
        std::vector<uint32_t> hs((size_t)nt * nc);
        if (c->toHost(hs.data(), c->train.dSizes.p, sizeof(uint32_t) * hs.size()) || c->wait()) return ZSMI_error_GENERIC;
        uint64_t bestTotal = ~0ull;
        for (uint32_t i = 0; i < nc; i++) {
            uint64_t sum = 0;
            for (uint32_t j = 0; j < nt; j++) { const uint32_t v = hs[(size_t)nt * i + j]; if (zs_word_is_error(v)) return (int)zs_word_code(v); sum += v; }
            const bool better = sum < bestTotal || (sum == bestTotal && (hc[i].k < hc[win].k || (hc[i].k == hc[win].k && hc[i].d < hc[win].d)));
            if (better) { bestTotal = sum; win = i; }
        }
    }
    params->k = hc[win].k; params->d = hc[win].d;
    const uint32_t contentSize = cap32 - hTails[win];
    if (contentSize < kTrainContentMin) return ZSMI_error_srcSize_wrong;
    if (!c->train.dOut.reserve(cap32 + 64)) return ZSMI_error_memory_allocation;
    uint32_t *dResult = dTails + win;                                       // (its tail is read already)
    if (const int e = finalizeQueue(c, dSamples, offs, sizes, hc[win].content + hTails[win], contentSize, cap32, t.level, params->dictID, (uint8_t *)c->train.dOut.p, dResult)) return e;
    return finalizeFetch(c, dResult, hostDict, dictSize);
}

// trainImpl over the context's samples, into a buffer of its own: nothing reaches the caller's buffer or params unless the call succeeds
static int trainGuarded(zsmi_ctx *c, const std::vector<uint32_t> &sizes, void *dictBuffer, size_t cap, zsmi_fastCoverParams *params, size_t *dictSize)
{
    std::vector<uint8_t> tmp(cap); zsmi_fastCoverParams p = *params;
    if (const int e = trainImpl(c, (const uint8_t *)c->train.dSamples.p, sizes, tmp.data(), cap, &p, dictSize)) return e;
    memcpy(dictBuffer, tmp.data(), *dictSize); params->k = p.k; params->d = p.d;
    return 0;
}
// host samples -> the context's device copy
static int trainStageHost(zsmi_ctx *c, const void *samples, const size_t *samplesSizes, unsigned nb, std::vector<uint32_t> &sizes)
{
    uint64_t total = 0;
    sizes.resize(nb);
    for (unsigned i = 0; i < nb; i++) { if (samplesSizes[i] > 0xFFFFFFFFull) return ZSMI_error_srcSize_wrong; sizes[i] = (uint32_t)samplesSizes[i]; total += samplesSizes[i]; }
    if (total >= (1ull << 32)) return ZSMI_error_srcSize_wrong;
    if (const int e = c->bind()) return e;
    if (!c->train.dSamples.reserve(total + 64)) return ZSMI_error_memory_allocation;
    if (const int e = c->fill((uint8_t *)c->train.dSamples.p + total, 0, 64)) return e;
    return c->toDevice(c->train.dSamples.p, samples, total);
}

extern "C" size_t zsmi_trainFromBuffer_fastCover(void *dictBuffer, size_t dictCapacity, const void *samplesBuffer, const size_t *samplesSizes,
                                                 unsigned nbSamples, zsmi_fastCoverParams *params)
{
    uint64_t total = 0;
    for (unsigned i = 0; i < nbSamples; i++) total += samplesSizes[i];
    { TrainPlan t; if (const int e = trainParams(params, dictCapacity, total, nbSamples, t)) return ZSMI_ERR(e); }
    Borrowed b; zsmi_ctx *c = b.c;
    if (!c) return ZSMI_ERR(ZSMI_error_GENERIC);
    std::vector<uint32_t> sizes;
    if (const int e = trainStageHost(c, samplesBuffer, samplesSizes, nbSamples, sizes)) return ZSMI_ERR(e);
    size_t size = 0;
    if (const int e = trainGuarded(c, sizes, dictBuffer, dictCapacity, params, &size)) return ZSMI_ERR(e);
    return size;
}

extern "C" size_t zsmi_trainFromBuffer(void *dictBuffer, size_t dictCapacity, const void *samplesBuffer, const size_t *samplesSizes, unsigned nbSamples)
{
    zsmi_fastCoverParams p;
    memset(&p, 0, sizeof p);
    p.d = 8; p.steps = 4; p.splitPoint = 0.75; p.level = 3;
    return zsmi_trainFromBuffer_fastCover(dictBuffer, dictCapacity, samplesBuffer, samplesSizes, nbSamples, &p);
}

extern "C" int zsmi_trainFromDevice(zsmi_ctx *c, const void *dSamples, const uint64_t *sampleOffsets, const uint32_t *sampleSizes, uint32_t nbSamples,
                                    void *dictBuffer, size_t dictCapacity, zsmi_fastCoverParams *params, size_t *dictSize)
{
    if (!c) return ZSMI_error_init_missing;
    uint64_t total = 0;
    for (uint32_t i = 0; i < nbSamples; i++) total += sampleSizes[i];
    { TrainPlan t; if (const int e = trainParams(params, dictCapacity, total, nbSamples, t)) return e; }
    if (!dictSize || !dSamples) return ZSMI_error_GENERIC;
    if (const int e = c->bind()) return e;
    // the samples back to back in the context's buffer (one gather launch)
    const size_t gatherBytes = sizeof(uint64_t) * 2 * nbSamples + sizeof(uint32_t) * nbSamples;
    if (!c->train.dSamples.reserve(total + 64) || !c->train.dGather.reserve(gatherBytes)) return ZSMI_error_memory_allocation;
    if (const int e = c->idleReserve({ { &c->train.hCand, gatherBytes } })) return e;      // (the pinned offsets may feed an earlier copy)
    uint64_t *ho = (uint64_t *)c->train.hCand.p;
    uint32_t *hs = (uint32_t *)(ho + 2 * (size_t)nbSamples);
    std::vector<uint32_t> sizes(sampleSizes, sampleSizes + nbSamples);
    uint64_t at = 0;
    for (uint32_t i = 0; i < nbSamples; i++) { ho[i] = sampleOffsets[i]; ho[nbSamples + i] = at; hs[i] = sampleSizes[i]; at += sampleSizes[i]; }
    if (const int e = c->toDevice(c->train.dGather.p, ho, gatherBytes)) return e;
    if (const int e = c->fill((uint8_t *)c->train.dSamples.p + total, 0, 64)) return e;
    LAUNCH(c, "k_train_gather", k_train_gather, dim3(nbSamples), dim3(256), 0, (const uint8_t *)dSamples, (const uint64_t *)c->train.dGather.p,
           (const uint32_t *)((const uint64_t *)c->train.dGather.p + 2 * (size_t)nbSamples), nbSamples, (uint8_t *)c->train.dSamples.p);
    if (const int e = c->wait()) return e;                                              // (the pinned offsets are reused below)
    return trainGuarded(c, sizes, dictBuffer, dictCapacity, params, dictSize);
}

extern "C" size_t zsmi_finalizeDictionary(void *dst, size_t dstCapacity, const void *content, size_t contentSize, const void *samplesBuffer,
                                          const size_t *samplesSizes, unsigned nbSamples, int level, unsigned dictID)
{
    if (dstCapacity < kTrainDictSizeMin) return ZSMI_ERR(ZSMI_error_dstSize_tooSmall);
    if (!content || contentSize < kTrainContentMin || contentSize > 0xFFFFFFFFull - (128u << 10) || nbSamples == 0) return ZSMI_ERR(ZSMI_error_srcSize_wrong);
    uint64_t total = 0;
    for (unsigned i = 0; i < nbSamples; i++) total += samplesSizes[i];
    if (total >= (1ull << 32)) return ZSMI_ERR(ZSMI_error_srcSize_wrong);
    Borrowed b; zsmi_ctx *c = b.c;
    if (!c) return ZSMI_ERR(ZSMI_error_GENERIC);
    std::vector<uint32_t> sizes;
    if (const int e = trainStageHost(c, samplesBuffer, samplesSizes, nbSamples, sizes)) return ZSMI_ERR(e);
    const uint32_t cap32 = (uint32_t)std::min<size_t>(dstCapacity, 0xFFFFFFFFu - 4096);
    if (!c->train.dContent.reserve(contentSize) || !c->train.dOut.reserve((size_t)cap32 + 64) || !c->train.dCand.reserve(64)) return ZSMI_ERR(ZSMI_error_memory_allocation);
    if (const int e = c->toDevice(c->train.dContent.p, content, contentSize)) return ZSMI_ERR(e);
    std::vector<uint64_t> offs(nbSamples);
    { uint64_t at = 0; for (unsigned i = 0; i < nbSamples; i++) { offs[i] = at; at += sizes[i]; } }
    uint32_t *dResult = (uint32_t *)c->train.dCand.p;
    if (const int e = finalizeQueue(c, (const uint8_t *)c->train.dSamples.p, offs, sizes, (const uint8_t *)c->train.dContent.p, (uint32_t)contentSize, cap32, level ? level : 3, dictID,
                                    (uint8_t *)c->train.dOut.p, dResult)) return ZSMI_ERR(e);
    size_t size = 0;
    if (const int e = finalizeFetch(c, dResult, dst, &size)) return ZSMI_ERR(e);
    return size;
}
