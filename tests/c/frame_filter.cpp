// Stand-alone host program over the frame filter's CPU forms (zstandard_amd/csrc/zsmi_filter.h, included alone): what zsmi_frameFilterSize,
// zsmi_buildFrameFilter, zsmi_readFrameFilter and zsmi_filterFrames run.  Every input and every output sits in a heap block of exactly its
// size, so that a read or a write past any end is the address sanitizer's to see.
//   frame_filter case <text> <delim> <sizes: u32 each> <g> <L> <pattern> <out prefix>
//       build -> read -> filter (one pattern, mode any); prints
//       <frame size> <-code of a build one byte short, its block untouched: 1> <n> <delim> <g> <L> <size> <saturated>
//       <-code of a read one byte short> <total> <written with capacity total> <tested> <saturated among them> <the list, comma-separated, or ->
//       <written with capacity total - 1, or - when total is 0> <total with capacity 0 and no array>
//       and leaves the frame in <out prefix>.frame
//   frame_filter rejections
//       prints a line "<name> <-code>" for every refusal of the four calls
// tests/test_frame_filter_host.py builds it with -fsanitize=address,undefined and holds the lines and files against tests/_filter.py.
#include "zsmi_filter.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>

static long long shown(size_t r) { return r > (size_t)0 - (size_t)ZSMI_error_maxCode ? -(long long)((size_t)0 - r) : (long long)r; }
template <class T> static T *block(size_t count) { T *p = (T *)malloc(count ? count * sizeof(T) : 1); if (!p) exit(2); return p; }
static uint8_t *slurp(const char *name, size_t &size)
{
    FILE *f = fopen(name, "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", name); exit(2); }
    fseek(f, 0, SEEK_END); size = (size_t)ftell(f); fseek(f, 0, SEEK_SET);
    uint8_t *p = block<uint8_t>(size);
    if (fread(p, 1, size, f) != size) { fprintf(stderr, "cannot read %s\n", name); exit(2); }
    fclose(f);
    return p;
}
static void spill(const char *prefix, const char *suffix, const uint8_t *p, size_t size)
{
    char name[4096];
    snprintf(name, sizeof name, "%s%s", prefix, suffix);
    FILE *f = fopen(name, "wb");
    if (!f || fwrite(p, 1, size, f) != size) { fprintf(stderr, "cannot write %s\n", name); exit(2); }
    fclose(f);
}
static zsmi_findQuery query_of(const uint8_t *pattern, uint32_t m, uint32_t mode, uint32_t flags)
{
    zsmi_findQuery q;
    memset(&q, 0, sizeof q);
    q.nPatterns = 1; q.mode = mode; q.flags = flags; q.patterns[0] = pattern; q.patternSizes[0] = m;
    return q;
}

static int one_case(char **a)
{
    size_t size, sizesBytes, m;
    uint8_t *text = slurp(a[0], size);
    const int delim = atoi(a[1]);
    uint8_t *rawSizes = slurp(a[2], sizesBytes);
    const size_t n = sizesBytes / 4;
    uint32_t *sizes = block<uint32_t>(n);
    memcpy(sizes, rawSizes, n * 4); free(rawSizes);
    const uint32_t g = (uint32_t)atoi(a[3]), L = (uint32_t)atoi(a[4]);
    uint8_t *pattern = slurp(a[5], m);
    // build: exactly the frame's size, then one byte short - refused, nothing written
    const size_t fsize = zs_flt_size(n, L);
    uint8_t *frame = block<uint8_t>(fsize), *tight = block<uint8_t>(fsize - 1);
    if (zs_flt_build(frame, fsize, size ? text : nullptr, size, n ? sizes : nullptr, n, delim, g, L) != fsize) { fprintf(stderr, "build failed\n"); return 1; }
    memset(tight, 0x5A, fsize - 1);
    const size_t refused = zs_flt_build(tight, fsize - 1, size ? text : nullptr, size, n ? sizes : nullptr, n, delim, g, L);
    bool untouched = true;
    for (size_t i = 0; i + 1 < fsize; i++) untouched &= tight[i] == 0x5A;
    printf("%zu %lld %d", fsize, shown(refused), (int)untouched);
    spill(a[6], ".frame", frame, fsize);
    // read: the whole frame, then one byte short
    zsmi_frameFilterInfo info;
    if (zs_flt_read(frame, fsize, &info)) { fprintf(stderr, "read failed\n"); return 1; }
    memcpy(tight, frame, fsize - 1);
    printf(" %u %u %u %u %llu %llu %d", info.nFrames, info.delim, info.gram, info.log2Bits, (unsigned long long)info.size, (unsigned long long)info.saturated,
           -zs_flt_read(tight, fsize - 1, &info));
    // filter: an array of exactly the total, of one entry less, and none
    const zsmi_findQuery q = query_of(pattern, (uint32_t)m, ZSMI_find_any, 0);
    uint64_t result[4];
    if (zs_flt_filter(frame, fsize, &q, 0, (uint32_t)n, nullptr, 0, result)) { fprintf(stderr, "filter failed\n"); return 1; }
    const size_t total = (size_t)result[0];
    uint32_t *list = block<uint32_t>(total);
    if (zs_flt_filter(frame, fsize, &q, 0, (uint32_t)n, total ? list : nullptr, total, result)) { fprintf(stderr, "filter failed\n"); return 1; }
    printf(" %llu %llu %llu %llu ", (unsigned long long)result[0], (unsigned long long)result[1], (unsigned long long)result[2], (unsigned long long)result[3]);
    for (size_t i = 0; i < total; i++) printf("%s%u", i ? "," : "", list[i]);
    if (!total) printf("-");
    if (total) {
        uint32_t *fewer = block<uint32_t>(total - 1);
        if (zs_flt_filter(frame, fsize, &q, 0, (uint32_t)n, total > 1 ? fewer : nullptr, total - 1, result)) { fprintf(stderr, "filter failed\n"); return 1; }
        if (result[0] != total || memcmp(fewer, list, (total - 1) * 4)) { fprintf(stderr, "a shorter list differs\n"); return 1; }
        printf(" %llu", (unsigned long long)result[1]);
        free(fewer);
    } else printf(" -");
    if (zs_flt_filter(frame, fsize, &q, 0, (uint32_t)n, nullptr, 0, result)) { fprintf(stderr, "filter failed\n"); return 1; }
    printf(" %llu\n", (unsigned long long)result[0]);
    free(text); free(sizes); free(pattern); free(frame); free(tight); free(list);
    return 0;
}

static void say(const char *name, size_t r) { printf("%s %lld\n", name, shown(r)); }
static void sayc(const char *name, int code) { printf("%s %d\n", name, -code); }
static const char kText[] = "abcdef\nghijkl\nmnopqr\n";                    // three frames of 7 bytes, all clean
// the frame of kText (g = 4, L = 9: 40 + 3 * 64 bytes) in a block of exactly `size` bytes, one byte at `at` XORed with `flip`
static uint8_t *damaged(size_t size, size_t at, uint8_t flip)
{
    const uint32_t sizes[3] = { 7, 7, 7 };
    uint8_t whole[232];
    if (zs_flt_build(whole, sizeof whole, kText, 21, sizes, 3, 10, 4, 9) != 232) exit(1);
    whole[at] ^= flip;
    uint8_t *p = block<uint8_t>(size);
    memcpy(p, whole, size);
    return p;
}
static void read_refusal(const char *name, size_t size, size_t at, uint8_t flip)
{
    uint8_t *f = damaged(size, at, flip);
    zsmi_frameFilterInfo info;
    sayc(name, zs_flt_read(f, size, &info));
    free(f);
}
static void filter_refusal(const char *name, size_t size, size_t at, uint8_t flip, const zsmi_findQuery *q, uint32_t first, uint32_t count, bool nullFrames = false, bool nullResult = false)
{
    uint8_t *f = damaged(size, at, flip);
    uint32_t *out = block<uint32_t>(3);
    uint64_t result[4];
    sayc(name, zs_flt_filter(f, size, q, first, count, nullFrames ? nullptr : out, 3, nullResult ? nullptr : result));
    free(f); free(out);
}
static int rejections()
{
    uint8_t *text = block<uint8_t>(21);
    memcpy(text, kText, 21);
    uint32_t *sizes = block<uint32_t>(3);
    sizes[0] = sizes[1] = sizes[2] = 7;
    uint8_t *dst = block<uint8_t>(232);
    say("size_log_low", zs_flt_size(3, 8)); say("size_log_high", zs_flt_size(3, 17)); say("size_too_many", zs_flt_size(0x4000000, 9)); say("size_good", zs_flt_size(3, 9));
    say("build_delim", zs_flt_build(dst, 232, text, 21, sizes, 3, 256, 4, 9));
    say("build_gram", zs_flt_build(dst, 232, text, 21, sizes, 3, 10, 5, 9));
    say("build_log", zs_flt_build(dst, 232, text, 21, sizes, 3, 10, 4, 17));
    say("build_too_many", zs_flt_build(dst, 232, text, 21, sizes, 0x4000000, 10, 4, 9));
    say("build_null_dst", zs_flt_build(nullptr, 232, text, 21, sizes, 3, 10, 4, 9));
    say("build_null_sizes", zs_flt_build(dst, 232, text, 21, nullptr, 3, 10, 4, 9));
    say("build_null_text", zs_flt_build(dst, 232, nullptr, 21, sizes, 3, 10, 4, 9));
    sizes[2] = 6; say("build_sum", zs_flt_build(dst, 232, text, 21, sizes, 3, 10, 4, 9)); sizes[2] = 7;
    say("build_short", zs_flt_build(dst, 231, text, 21, sizes, 3, 10, 4, 9));
    say("build_good", zs_flt_build(dst, 232, text, 21, sizes, 3, 10, 4, 9));
    { uint8_t *f = damaged(232, 0, 0); sayc("read_null_info", zs_flt_read(f, 232, nullptr)); free(f); }
    read_refusal("read_39_bytes", 39, 0, 0);
    read_refusal("read_outer_magic", 232, 0, 1);
    read_refusal("read_inner_magic", 232, 9, 0x40);
    read_refusal("read_version", 232, 12, 3);
    read_refusal("read_gram", 232, 14, 1);
    read_refusal("read_log", 232, 15, 0x10);
    read_refusal("read_reserved", 232, 20, 1);
    read_refusal("read_frame_size", 232, 4, 4);
    read_refusal("read_n", 232, 16, 1);
    read_refusal("read_cut", 231, 0, 0);
    read_refusal("read_delim", 232, 13, 1);
    read_refusal("read_size", 232, 24, 1);
    read_refusal("read_check", 232, 39, 0x80);
    read_refusal("read_slot_bit", 232, 100, 0x10);
    read_refusal("read_good", 232, 0, 0);
    // filter
    uint8_t *pat = block<uint8_t>(4), *withDelim = block<uint8_t>(4);
    memcpy(pat, "ghij", 4); memcpy(withDelim, "gh\nj", 4);
    zsmi_findQuery q = query_of(pat, 4, ZSMI_find_any, 0), bad;
    filter_refusal("filter_null_query", 232, 0, 0, nullptr, 0, 3);
    filter_refusal("filter_null_result", 232, 0, 0, &q, 0, 3, false, true);
    filter_refusal("filter_null_frames", 232, 0, 0, &q, 0, 3, true);
    filter_refusal("filter_39_bytes", 39, 0, 0, &q, 0, 3);
    filter_refusal("filter_outer_magic", 232, 3, 1, &q, 0, 3);
    filter_refusal("filter_version", 232, 12, 2, &q, 0, 3);
    filter_refusal("filter_log", 232, 15, 0x10, &q, 0, 3);
    filter_refusal("filter_cut", 231, 0, 0, &q, 0, 3);
    bad = q; bad.nPatterns = 9; filter_refusal("filter_patterns", 232, 0, 0, &bad, 0, 3);
    bad = q; bad.mode = 3; filter_refusal("filter_mode", 232, 0, 0, &bad, 0, 3);
    bad = q; bad.flags = 2; filter_refusal("filter_flags", 232, 0, 0, &bad, 0, 3);
    bad = q; bad.patterns[0] = nullptr; filter_refusal("filter_null_pattern", 232, 0, 0, &bad, 0, 3);
    bad = q; bad.patternSizes[0] = 0; filter_refusal("filter_pattern_size", 232, 0, 0, &bad, 0, 3);
    bad = query_of(withDelim, 4, ZSMI_find_any, 0); filter_refusal("filter_pattern_delim", 232, 0, 0, &bad, 0, 3);
    filter_refusal("filter_window", 232, 0, 0, &q, 2, 2);
    filter_refusal("filter_check_not_judged", 232, 39, 0x80, &q, 0, 3);
    filter_refusal("filter_good", 232, 0, 0, &q, 0, 3);
    free(text); free(sizes); free(dst); free(pat); free(withDelim);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 2 && !strcmp(argv[1], "rejections")) return rejections();
    for (int a = 1; a + 7 < argc && !strcmp(argv[a], "case"); a += 8)
        if (const int rc = one_case(argv + a + 1)) return rc;
    return 0;
}
