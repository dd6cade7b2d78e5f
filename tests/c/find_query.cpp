// Stand-alone host program over the rule of find records by several patterns (zstandard_amd/csrc/zsmi_findquery.h, included alone).  For
// every group of arguments <text file> <delim> <base> <mode> <flags> <K> <pattern file> x K: zs_findq_check, then zs_findq_records three
// times - only counting (capacity 0, no arrays), with arrays of exactly `total` entries, and, where total > 0, with arrays of total - 1
// and no hit sets - and one line -
//   <total> <matches> then <number>:<hit set> for every record
// The text, each pattern and each array sit in heap blocks of exactly their sizes, so that a read or a write past any end is the address
// sanitizer's to see.  tests/test_find_query_host.py builds it with -fsanitize=address,undefined and holds the lines against
// tests/_findq.py.
#include "zsmi_findquery.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>

static uint8_t *slurp(const char *name, size_t &size)
{
    FILE *file = fopen(name, "rb");
    if (!file) { fprintf(stderr, "cannot open %s\n", name); exit(2); }
    fseek(file, 0, SEEK_END);
    size = (size_t)ftell(file);
    fseek(file, 0, SEEK_SET);
    uint8_t *p = (uint8_t *)malloc(size ? size : 1);
    if (!p || fread(p, 1, size, file) != size) { fprintf(stderr, "cannot read %s\n", name); exit(2); }
    fclose(file);
    if (size == 0) { free(p); p = nullptr; }                              // (an empty text is no block at all)
    return p;
}

int main(int argc, char **argv)
{
    int a = 1;
    while (a + 5 < argc) {
        const char *name = argv[a];
        size_t size;
        uint8_t *text = slurp(argv[a], size);
        const int delim = atoi(argv[a + 1]);
        const uint64_t base = strtoull(argv[a + 2], nullptr, 10);
        zsmi_findQuery q;
        memset(&q, 0, sizeof q);
        q.mode = (uint32_t)atoi(argv[a + 3]); q.flags = (uint32_t)atoi(argv[a + 4]); q.nPatterns = (uint32_t)atoi(argv[a + 5]);
        a += 6;
        if (q.nPatterns > ZSMI_FIND_MAX_PATTERNS || a + (int)q.nPatterns > argc) { fprintf(stderr, "%s: bad arguments\n", name); return 2; }
        uint8_t *blocks[ZSMI_FIND_MAX_PATTERNS] = {};
        for (uint32_t j = 0; j < q.nPatterns; j++, a++) {
            size_t m;
            blocks[j] = slurp(argv[a], m);
            q.patterns[j] = blocks[j]; q.patternSizes[j] = (uint32_t)m;
        }
        if (const int e = zs_findq_check(delim, &q)) { fprintf(stderr, "%s: refused with %d\n", name, e); return 1; }
        uint64_t matches = 0, again = 0;
        const uint64_t total = zs_findq_records(text, size, (uint8_t)delim, &q, base, nullptr, nullptr, 0, &matches);
        uint64_t *out = (uint64_t *)malloc(total ? total * sizeof(uint64_t) : 1);
        uint8_t *hits = (uint8_t *)malloc(total ? total : 1);
        if (!out || !hits) return 2;
        if (zs_findq_records(text, size, (uint8_t)delim, &q, base, out, hits, total, &again) != total || again != matches) { fprintf(stderr, "%s: two answers\n", name); return 1; }
        if (total) {
            uint64_t *fewer = (uint64_t *)malloc(total > 1 ? (total - 1) * sizeof(uint64_t) : 1);
            if (!fewer) return 2;
            if (zs_findq_records(text, size, (uint8_t)delim, &q, base, fewer, nullptr, total - 1, nullptr) != total) { fprintf(stderr, "%s: the count depends on capacity\n", name); return 1; }
            if (memcmp(fewer, out, (total - 1) * sizeof(uint64_t))) { fprintf(stderr, "%s: the prefix differs\n", name); return 1; }
            free(fewer);
        }
        printf("%llu %llu", (unsigned long long)total, (unsigned long long)matches);
        for (uint64_t i = 0; i < total; i++) printf(" %llu:%u", (unsigned long long)out[i], (unsigned)hits[i]);
        printf("\n");
        free(out); free(hits); free(text);
        for (uint32_t j = 0; j < q.nPatterns; j++) free(blocks[j]);
    }
    return 0;
}
