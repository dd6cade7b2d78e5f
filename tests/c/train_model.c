/* Scalar statement of the GPU fastCover trainer's segment selection (zstandard_amd/csrc/dict_train.hip, steps 1 - 2 of the trainer) for
 * fixed k, d, f and splitPoint 1.0: zstd's FASTCOVER_computeFrequency, FASTCOVER_selectSegment (sliding window, first best, trimmed,
 * frequencies zeroed) and FASTCOVER_buildDictionary (epochs of max(1, cap / k / 4), at least 10 k d-mers each, visited in turn until the
 * content is full or 10 epochs in a row give nothing), with 64-bit scores.  Built by the tests with gcc as a shared library.
 * model_train returns where the content starts in dict[0, cap); the content is dict[tail, cap). */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

static uint32_t hash_at(const uint8_t *p, unsigned d, unsigned f)
{
    uint64_t v;
    memcpy(&v, p, 8);
    if (d == 6) return (uint32_t)(((v << 16) * 227718039650203ull) >> (64 - f));
    return (uint32_t)((v * 0xCF1BBCDCB7A56463ull) >> (64 - f));
}

size_t model_train(const uint8_t *samples, const size_t *sizes, unsigned n, uint8_t *dict, size_t cap, unsigned k, unsigned d, unsigned f)
{
    size_t total = 0, off = 0;
    for (unsigned i = 0; i < n; i++) total += sizes[i];
    if (total < 8) return cap;
    const size_t nbDmers = total - 7, L = k - d + 1;
    uint32_t *freq = calloc((size_t)1 << f, sizeof(uint32_t)), *win = calloc((size_t)1 << f, sizeof(uint32_t));
    for (unsigned i = 0; i < n; i++) {
        const size_t end = off + sizes[i];
        for (size_t s = off; s + 8 <= end; s++) freq[hash_at(samples + s, d, f)]++;
        off = end;
    }
    size_t num = cap / k / 4, size;
    if (num < 1) num = 1;
    size = nbDmers / num;
    if (size < 10 * (size_t)k) { size = 10 * (size_t)k < nbDmers ? 10 * (size_t)k : nbDmers; num = nbDmers / size; }
    size_t tail = cap, zeroRun = 0;
    for (size_t epoch = 0; tail > 0; epoch = (epoch + 1) % num) {
        const size_t eb = epoch * size, ee = eb + size;
        size_t ab = eb, ae = eb, bb = 0, be = 0;
        uint64_t as = 0, bs = 0;
        while (ae < ee) {
            const uint32_t h = hash_at(samples + ae, d, f);
            if (win[h] == 0) as += freq[h];
            ae++; win[h]++;
            if (ae - ab == L + 1) {
                const uint32_t g = hash_at(samples + ab, d, f);
                if (--win[g] == 0) as -= freq[g];
                ab++;
            }
            if (as > bs) { bs = as; bb = ab; be = ae; }
        }
        for (; ab < ee; ab++) win[hash_at(samples + ab, d, f)]--;
        if (bs == 0) { if (++zeroRun >= 10) break; continue; }
        zeroRun = 0;
        size_t nb = be, ne = bb;
        for (size_t p = bb; p < be; p++) if (freq[hash_at(samples + p, d, f)]) { if (p < nb) nb = p; ne = p + 1; }
        for (size_t p = nb; p < ne; p++) freq[hash_at(samples + p, d, f)] = 0;
        size_t seg = ne - nb + d - 1;
        if (seg > tail) seg = tail;
        if (seg < d) break;
        tail -= seg;
        memcpy(dict + tail, samples + nb, seg);
    }
    free(freq); free(win);
    return tail;
}
