// Stand-alone host program over the two rules of records by number (zstandard_amd/csrc/zsmi_records.h, included alone next to the
// splitter's zsmi_split.h).  For every group of four arguments <file> <delim> <targetSize> <maxFrameSize>: the file is split by the
// splitter's host loop, then every record r of it goes through zs_rec_frames and zs_rec_extent; one line -
//   <records> <frames> then, a record, <f>,<g>,<start>,<end>   (start and end counted from the file's first byte)
// The text, firstRecord (n + 1 entries), the frames' content offsets and each record's run - the content of its frames f .. g, copied out -
// sit in heap blocks of exactly their sizes, so that a read past any end is the address sanitizer's to see.
// tests/test_read_records_host.py builds it with -fsanitize=address,undefined and holds the lines against tests/_split.py.
#include "zsmi_split.h"
#include "zsmi_records.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>

int main(int argc, char **argv)
{
    for (int a = 1; a + 3 < argc; a += 4) {
        FILE *file = fopen(argv[a], "rb");
        if (!file) { fprintf(stderr, "cannot open %s\n", argv[a]); return 2; }
        fseek(file, 0, SEEK_END);
        const size_t size = (size_t)ftell(file);
        fseek(file, 0, SEEK_SET);
        uint8_t *src = (uint8_t *)malloc(size ? size : 1);
        if (!src || fread(src, 1, size, file) != size) { fprintf(stderr, "cannot read %s\n", argv[a]); return 2; }
        fclose(file);
        const int delim = atoi(argv[a + 1]);
        const uint32_t T = (uint32_t)strtoul(argv[a + 2], nullptr, 10), M = (uint32_t)strtoul(argv[a + 3], nullptr, 10);
        const uint8_t *in = size ? src : nullptr;
        const size_t n = zs_split_records(in, size, delim, T, M, nullptr, nullptr, 0, nullptr);
        if (n > (size_t)0 - (size_t)ZSMI_error_maxCode) { fprintf(stderr, "%s: the split is refused\n", argv[a]); return 1; }
        uint32_t *sizes = (uint32_t *)malloc(n ? n * sizeof(uint32_t) : 1);
        uint64_t *first = (uint64_t *)malloc((n + 1) * sizeof(uint64_t)), *at = (uint64_t *)malloc((n + 1) * sizeof(uint64_t));
        if (!sizes || !first || !at) return 2;
        if (zs_split_records(in, size, delim, T, M, sizes, first, n, nullptr) != n) return 1;
        at[0] = 0;
        for (size_t i = 0; i < n; i++) at[i + 1] = at[i] + sizes[i];
        const uint64_t records = first[n];
        printf("%llu %llu", (unsigned long long)records, (unsigned long long)n);
        for (uint64_t r = 0; r < records; r++) {
            const ZsRecFrames q = zs_rec_frames(first, (uint32_t)n, r);
            if (q.f > q.g || q.g >= n) { fprintf(stderr, "%s: record %llu names frames %u .. %u of %llu\n", argv[a], (unsigned long long)r, q.f, q.g, (unsigned long long)n); return 1; }
            const uint64_t len = at[q.g + 1] - at[q.f];
            uint8_t *run = (uint8_t *)malloc(len ? len : 1);
            if (!run) return 2;
            memcpy(run, src + at[q.f], len);
            uint64_t start = 0, end = 0;
            const int code = zs_rec_extent(len ? run : nullptr, len, (uint8_t)delim, q.skip, &start, &end);
            if (code) { fprintf(stderr, "%s: record %llu: code %d\n", argv[a], (unsigned long long)r, code); return 1; }
            printf(" %u,%u,%llu,%llu", q.f, q.g, (unsigned long long)(at[q.f] + start), (unsigned long long)(at[q.f] + end));
            // one delimiter more than the frame holds in front of the record is the rule's refusal (where the run has that few)
            uint64_t s2, e2, delims = 0;
            for (uint64_t i = 0; i < len; i++) delims += run[i] == (uint8_t)delim;
            if (zs_rec_extent(len ? run : nullptr, len, (uint8_t)delim, delims + 1, &s2, &e2) != ZSMI_error_corruption_detected) { fprintf(stderr, "%s: record %llu: no refusal\n", argv[a], (unsigned long long)r); return 1; }
            free(run);
        }
        printf("\n");
        free(sizes); free(first); free(at); free(src);
    }
    return 0;
}
