// Stand-alone host program over the compress plan's per-chunk rule (zstandard_amd/csrc/zsmi_plan.h, included alone): for every size given
// as an argument one line - size blocks smallUnits bigUnits - then a line per block (B k off size first last) and per unit
// (U u off size block big at) of the sizes that have at most 8 blocks.  tests/test_resident_compress_host.py holds them against a few lines of Python.
#include "zsmi_plan.h"
#include <cstdio>
#include <cstdlib>

int main(int argc, char **argv)
{
    for (int a = 1; a < argc; a++) {
        const uint32_t size = (uint32_t)strtoull(argv[a], nullptr, 0);
        const ZsChunkCounts c = zs_chunk_counts(size);
        printf("%u %u %u %u\n", size, c.blocks, c.smallUnits, c.bigUnits);
        if (c.blocks > 8) continue;
        for (uint32_t k = 0; k < c.blocks; k++) {
            const ZsChunkBlock b = zs_chunk_block(size, k, c.blocks);
            printf("B %u %llu %u %u %u\n", k, (unsigned long long)b.off, b.size, b.first, b.last);
        }
        for (uint32_t u = 0; u < c.smallUnits + c.bigUnits; u++) {
            const ZsChunkUnit r = zs_chunk_unit(size, u);
            printf("U %u %llu %u %u %u %u\n", u, (unsigned long long)r.off, r.size, r.block, r.big, r.at);
        }
    }
    return 0;
}
