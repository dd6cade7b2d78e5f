// Stand-alone host program over the compress plan's dictionary rule (zstandard_amd/csrc/zsmi_plan.h, included alone): for every size given
// as an argument two lines, without and with a dictionary -
//   size dict blocks pfxUnits tailUnits bigUnits prefixed | blocks smallUnits bigUnits
// the part behind the bar being zs_chunk_counts of the size.  tests/test_resident_cdict_set_host.py holds them against a few lines of Python.
#include "zsmi_plan.h"
#include <cstdio>
#include <cstdlib>

int main(int argc, char **argv)
{
    for (int a = 1; a < argc; a++) {
        const uint32_t size = (uint32_t)strtoull(argv[a], nullptr, 0);
        const ZsChunkCounts c = zs_chunk_counts(size);
        for (int dict = 0; dict < 2; dict++) {
            const ZsChunkDictCounts d = zs_chunk_counts_dict(size, dict != 0);
            printf("%u %d %u %u %u %u %d | %u %u %u\n", size, dict, d.blocks, d.pfxUnits, d.tailUnits, d.bigUnits, (int)zs_chunk_prefixed(size, dict != 0),
                   c.blocks, c.smallUnits, c.bigUnits);
        }
    }
    return 0;
}
