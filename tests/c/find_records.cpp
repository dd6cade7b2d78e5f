// Stand-alone host program over the rule of find records by content (zstandard_amd/csrc/zsmi_find.h, included alone).  For every group
// of four arguments <text file> <pattern file> <delim> <base>: zs_find_check, then zs_find_records three times - only counting (capacity
// 0, no array), with an array of exactly `total` entries, and, where total > 0, with one of total - 1 - and one line -
//   <total> <matches> then the numbers
// The text, the pattern and each array sit in heap blocks of exactly their sizes, so that a read or a write past any end is the address
// sanitizer's to see.  tests/test_find_records_host.py builds it with -fsanitize=address,undefined and holds the lines against
// tests/_find.py.
#include "zsmi_find.h"
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
    for (int a = 1; a + 3 < argc; a += 4) {
        size_t size, m;
        uint8_t *text = slurp(argv[a], size), *pattern = slurp(argv[a + 1], m);
        const int delim = atoi(argv[a + 2]);
        const uint64_t base = strtoull(argv[a + 3], nullptr, 10);
        if (const int e = zs_find_check(delim, pattern, (uint32_t)m)) { fprintf(stderr, "%s: refused with %d\n", argv[a], e); return 1; }
        uint64_t matches = 0, again = 0;
        const uint64_t total = zs_find_records(text, size, (uint8_t)delim, pattern, (uint32_t)m, base, nullptr, 0, &matches);
        uint64_t *out = (uint64_t *)malloc(total ? total * sizeof(uint64_t) : 1);
        if (!out) return 2;
        if (zs_find_records(text, size, (uint8_t)delim, pattern, (uint32_t)m, base, out, total, &again) != total || again != matches) { fprintf(stderr, "%s: two answers\n", argv[a]); return 1; }
        if (total) {
            uint64_t *fewer = (uint64_t *)malloc(total > 1 ? (total - 1) * sizeof(uint64_t) : 1);
            if (!fewer) return 2;
            if (zs_find_records(text, size, (uint8_t)delim, pattern, (uint32_t)m, base, fewer, total - 1, nullptr) != total) { fprintf(stderr, "%s: the count depends on capacity\n", argv[a]); return 1; }
            if (memcmp(fewer, out, (total - 1) * sizeof(uint64_t))) { fprintf(stderr, "%s: the prefix differs\n", argv[a]); return 1; }
            free(fewer);
        }
        printf("%llu %llu", (unsigned long long)total, (unsigned long long)matches);
        for (uint64_t i = 0; i < total; i++) printf(" %llu", (unsigned long long)out[i]);
        printf("\n");
        free(out); free(text); free(pattern);
    }
    return 0;
}
