// Stand-alone host program over the frame index's CPU form (zstandard_amd/csrc/zsmi_index.h, included alone): the walk loop and the table
// writer, as zsmi_countFrames and zsmi_buildSeekTable run them.  For every file given as an argument one line -
//   <frames or -code> <table size or -code> <the table in hex, or -> <-code of a capacity one byte short, or ->
// - with the stream held in a heap block of exactly its size and the table written into one of exactly its size, so that a read or a write
// past either end is the address sanitizer's to see.  tests/test_frames_index_host.py builds it with -fsanitize=address,undefined, runs it
// over the good and the bad streams of tests/_frames_index.py and holds the lines against the Python statement of the index.
#include "zsmi_index.h"
#include <cstdio>
#include <cstdlib>

static long long shown(size_t r) { return r > (size_t)0 - (size_t)ZSMI_error_maxCode ? -(long long)((size_t)0 - r) : (long long)r; }

int main(int argc, char **argv)
{
    for (int a = 1; a < argc; a++) {
        FILE *f = fopen(argv[a], "rb");
        if (!f) { fprintf(stderr, "cannot open %s\n", argv[a]); return 2; }
        fseek(f, 0, SEEK_END);
        const size_t size = (size_t)ftell(f);
        fseek(f, 0, SEEK_SET);
        uint8_t *src = (uint8_t *)malloc(size ? size : 1);
        if (!src || fread(src, 1, size, f) != size) { fprintf(stderr, "cannot read %s\n", argv[a]); return 2; }
        fclose(f);
        const size_t n = zs_index_count(size ? src : nullptr, size);
        const size_t want = zs_index_build_table(nullptr, 0, size ? src : nullptr, size);      // (a stream's own code comes first; else dstSize_tooSmall)
        printf("%lld ", shown(n));
        if (shown(n) < 0) {
            if (want != n) { fprintf(stderr, "%s: the table's code is not the count's\n", argv[a]); return 1; }
            printf("%lld - -\n", shown(want));
        } else {
            const size_t bytes = ZS_SEEK_TABLE_FIXED + 8 * n;
            uint8_t *table = (uint8_t *)malloc(bytes);
            if (!table) return 2;
            const size_t wrote = zs_index_build_table(table, bytes, size ? src : nullptr, size);
            printf("%lld ", shown(wrote));
            for (size_t i = 0; i < bytes && wrote == bytes; i++) printf("%02x", table[i]);
            printf(" %lld\n", shown(zs_index_build_table(table, bytes - 1, size ? src : nullptr, size)));
            free(table);
        }
        free(src);
    }
    return 0;
}
