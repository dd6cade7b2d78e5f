// Stand-alone host program over find records by regular expression (zstandard_amd/csrc/zsmi_regex.h, included alone: the compiler, the
// program check and the rule's loop).  For every group of arguments <text file> <delim> <base> <flags> <pattern file>: zs_regex_compile,
// zs_regex_check, then zs_regex_records three times - only counting (capacity 0, no array), with an array of exactly `total` entries,
// and, where total > 0, with one of total - 1 - and one line -
//   <nStates> <nClasses> <total> <textRecords> then every number
// or, for a pattern the compiler refuses, `refused <code> <errorAt>`.  The pattern, the text and each array sit in heap blocks of exactly
// their sizes, so that a read or a write past any end is the address sanitizer's to see.  tests/test_find_regex_host.py builds it with
// -fsanitize=address,undefined and holds the lines against tests/_findre.py.
#include "zsmi_regex.h"
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
    for (int a = 1; a + 4 < argc; a += 5) {
        const char *name = argv[a + 4];
        size_t size, m;
        uint8_t *text = slurp(argv[a], size);
        const int delim = atoi(argv[a + 1]);
        const uint64_t base = strtoull(argv[a + 2], nullptr, 10);
        const uint32_t flags = (uint32_t)atoi(argv[a + 3]);
        uint8_t *pattern = slurp(argv[a + 4], m);
        zsmi_regexProgram *prog = (zsmi_regexProgram *)malloc(sizeof(zsmi_regexProgram));
        if (!prog) return 2;
        size_t at = 0;
        if (const int e = zs_regex_compile(pattern, m, flags, prog, &at)) {
            printf("refused %d %llu\n", e, (unsigned long long)at);
            free(prog); free(pattern); free(text);
            continue;
        }
        if (const int e = zs_regex_check(delim, prog)) { fprintf(stderr, "%s: the compiler's program is refused with %d\n", name, e); return 1; }
        uint64_t records = 0, again = 0;
        const uint64_t total = zs_regex_records(text, size, (uint8_t)delim, prog, base, nullptr, 0, &records);
        uint64_t *out = (uint64_t *)malloc(total ? total * sizeof(uint64_t) : 1);
        if (!out) return 2;
        if (zs_regex_records(text, size, (uint8_t)delim, prog, base, out, total, &again) != total || again != records) { fprintf(stderr, "%s: two answers\n", name); return 1; }
        if (total) {
            uint64_t *fewer = (uint64_t *)malloc(total > 1 ? (total - 1) * sizeof(uint64_t) : 1);
            if (!fewer) return 2;
            if (zs_regex_records(text, size, (uint8_t)delim, prog, base, fewer, total - 1, nullptr) != total) { fprintf(stderr, "%s: the count depends on capacity\n", name); return 1; }
            if (memcmp(fewer, out, (total - 1) * sizeof(uint64_t))) { fprintf(stderr, "%s: the prefix differs\n", name); return 1; }
            free(fewer);
        }
        printf("%u %u %llu %llu", prog->nStates, prog->nClasses, (unsigned long long)total, (unsigned long long)records);
        for (uint64_t i = 0; i < total; i++) printf(" %llu", (unsigned long long)out[i]);
        printf("\n");
        free(out); free(prog); free(pattern); free(text);
    }
    return 0;
}
