// Stand-alone host program over the record splitter's CPU form (zstandard_amd/csrc/zsmi_split.h, included alone): the rule's loop, as
// zsmi_splitRecords runs it.  For every group of four arguments <file> <delim> <targetSize> <maxFrameSize> one line -
//   <frames or -code> <records> <the sizes, comma-separated, or -> <firstRecord, comma-separated, or -> <the count-only call's answer>
//   <-code of a capacity one entry short, or - for no frame>
// - with the input held in a heap block of exactly its size, the sizes in one of exactly n entries and firstRecord in one of exactly
// n + 1, so that a read or a write past any end is the address sanitizer's to see.  tests/test_split_records_host.py builds it with
// -fsanitize=address,undefined, runs it over the inputs of tests/_split.py and holds the lines against the Python statement of the rule.
#include "zsmi_split.h"
#include <cstdio>
#include <cstdlib>

static long long shown(size_t r) { return r > (size_t)0 - (size_t)ZSMI_error_maxCode ? -(long long)((size_t)0 - r) : (long long)r; }

int main(int argc, char **argv)
{
    for (int a = 1; a + 3 < argc; a += 4) {
        FILE *f = fopen(argv[a], "rb");
        if (!f) { fprintf(stderr, "cannot open %s\n", argv[a]); return 2; }
        fseek(f, 0, SEEK_END);
        const size_t size = (size_t)ftell(f);
        fseek(f, 0, SEEK_SET);
        uint8_t *src = (uint8_t *)malloc(size ? size : 1);
        if (!src || fread(src, 1, size, f) != size) { fprintf(stderr, "cannot read %s\n", argv[a]); return 2; }
        fclose(f);
        const int delim = atoi(argv[a + 1]);
        const uint32_t T = (uint32_t)strtoul(argv[a + 2], nullptr, 10), M = (uint32_t)strtoul(argv[a + 3], nullptr, 10);
        const uint8_t *in = size ? src : nullptr;
        uint64_t records = 0;
        const size_t counted = zs_split_records(in, size, delim, T, M, nullptr, nullptr, 0, &records);
        if (shown(counted) < 0) { printf("%lld 0 - - %lld -\n", shown(counted), shown(counted)); free(src); continue; }
        uint32_t *sizes = (uint32_t *)malloc(counted ? counted * sizeof(uint32_t) : 1);
        uint64_t *first = (uint64_t *)malloc((counted + 1) * sizeof(uint64_t));
        if (!sizes || !first) return 2;
        uint64_t again = 0;
        const size_t n = zs_split_records(in, size, delim, T, M, sizes, first, counted, &again);
        if (n != counted || again != records) { fprintf(stderr, "%s: the two calls disagree\n", argv[a]); return 1; }
        printf("%lld %llu ", shown(n), (unsigned long long)records);
        for (size_t i = 0; i < n; i++) printf("%s%u", i ? "," : "", sizes[i]);
        printf(n ? " " : "- ");
        for (size_t i = 0; i <= n; i++) printf("%s%llu", i ? "," : "", (unsigned long long)first[i]);
        printf(" %lld ", shown(counted));
        if (n) {
            uint32_t *fewer = (uint32_t *)malloc(n > 1 ? (n - 1) * sizeof(uint32_t) : 1);
            uint64_t *fewerFirst = (uint64_t *)malloc(n * sizeof(uint64_t));
            if (!fewer || !fewerFirst) return 2;
            printf("%lld\n", shown(zs_split_records(in, size, delim, T, M, fewer, fewerFirst, n - 1, nullptr)));
            free(fewer); free(fewerFirst);
        } else printf("-\n");
        free(sizes); free(first); free(src);
    }
    return 0;
}
