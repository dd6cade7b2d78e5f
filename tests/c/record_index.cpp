// Stand-alone host program over the record index's CPU forms (zstandard_amd/csrc/zsmi_recindex.h, included alone): what
// zsmi_indexRecords, zsmi_writeRecordIndexFrame, zsmi_readRecordIndexFrame and zsmi_seekableAttachRecordIndex run.  Every input and every
// output sits in a heap block of exactly its size, so that a read or a write past any end is the address sanitizer's to see.
//   record_index case <text> <delim> <sizes: u32 each> <archive> <out prefix>
//       index -> write -> read -> attach; prints
//       <rc> <records> <misaligned> <delimiters> <firstRecord, comma-separated> <frame size> <-code one byte short> <n read> <delim read>
//       <-code of a read one byte short> <attached size> <-code of an attach one byte short, archive untouched: 1>
//       and leaves the frame in <out prefix>.frame and the attached archive in <out prefix>.attached
//   record_index rejections <archive of 3 frames with Decompressed_Size 4, 4, 4>
//       prints a line "<name> <-code>" for every refusal of the four calls
// tests/test_record_index_host.py builds it with -fsanitize=address,undefined and holds the lines and files against tests/_recindex.py.
#include "zsmi_recindex.h"
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

static int one_case(char **a)
{
    size_t size, sizesBytes, archiveSize;
    uint8_t *text = slurp(a[0], size);
    const int delim = atoi(a[1]);
    uint8_t *rawSizes = slurp(a[2], sizesBytes);
    const size_t n = sizesBytes / 4;
    uint32_t *sizes = block<uint32_t>(n);
    memcpy(sizes, rawSizes, n * 4); free(rawSizes);
    uint8_t *archive = slurp(a[3], archiveSize);
    uint64_t *first = block<uint64_t>(n + 1), result[4];
    const int rc = zs_ridx_index(size ? text : nullptr, size, n ? sizes : nullptr, n, delim, first, result);
    if (rc) { printf("%d\n", -rc); return 0; }
    printf("0 %llu %llu %llu ", (unsigned long long)result[1], (unsigned long long)result[2], (unsigned long long)result[3]);
    for (size_t i = 0; i <= n; i++) printf("%s%llu", i ? "," : "", (unsigned long long)first[i]);
    // write: exactly the frame's size, then one byte short
    const size_t fsize = zs_ridx_size(n);
    uint8_t *frame = block<uint8_t>(fsize), *shortFrame = block<uint8_t>(fsize - 1);
    if (zs_ridx_write(frame, fsize, first, n, delim) != fsize) { fprintf(stderr, "write failed\n"); return 1; }
    printf(" %zu %lld", fsize, shown(zs_ridx_write(shortFrame, fsize - 1, first, n, delim)));
    spill(a[4], ".frame", frame, fsize);
    // read: exactly n + 1 entries; then the frame one byte short
    uint64_t *again = block<uint64_t>(n + 1);
    int delimRead = -1;
    const size_t nRead = zs_ridx_read(frame, fsize, again, n + 1, &delimRead);
    if (nRead != n || memcmp(again, first, (n + 1) * sizeof(uint64_t))) { fprintf(stderr, "read differs\n"); return 1; }
    memcpy(shortFrame, frame, fsize - 1);
    printf(" %lld %d %lld", shown(nRead), delimRead, shown(zs_ridx_read(shortFrame, fsize - 1, again, n + 1, nullptr)));
    // attach: a block of exactly the new size; then one byte short, which must leave the archive as it was
    const size_t entry = archive[archiveSize - 5] & 0x80 ? 12 : 8, grown = archiveSize + fsize + entry;
    uint8_t *room = block<uint8_t>(grown), *tight = block<uint8_t>(grown - 1);
    memcpy(room, archive, archiveSize); memcpy(tight, archive, archiveSize);
    const size_t got = zs_ridx_attach(room, archiveSize, grown, first, n, delim);
    const size_t refused = zs_ridx_attach(tight, archiveSize, grown - 1, first, n, delim);
    printf(" %lld %lld %d\n", shown(got), shown(refused), memcmp(tight, archive, archiveSize) == 0);
    if (got == grown) spill(a[4], ".attached", room, grown);
    free(text); free(sizes); free(archive); free(first); free(frame); free(shortFrame); free(again); free(room); free(tight);
    return 0;
}

static void say(const char *name, size_t r) { printf("%s %lld\n", name, shown(r)); }
static void sayc(const char *name, int code) { printf("%s %d\n", name, -code); }
// a frame of first = {0, 2, 2, 5}, delim 10, in a block of exactly `size` bytes, one byte at `at` XORed with `flip`
static uint8_t *damaged(size_t size, size_t at, uint8_t flip)
{
    const uint64_t first[4] = { 0, 2, 2, 5 };
    uint8_t whole[52];
    if (zs_ridx_write(whole, sizeof whole, first, 3, 10) != 52) exit(1);
    whole[at] ^= flip;
    uint8_t *p = block<uint8_t>(size);
    memcpy(p, whole, size);
    return p;
}
static void read_refusal(const char *name, size_t size, size_t at, uint8_t flip, size_t capacity)
{
    uint8_t *f = damaged(size, at, flip);
    uint64_t *out = block<uint64_t>(capacity);
    say(name, zs_ridx_read(f, size, out, capacity, nullptr));
    free(f); free(out);
}
static int rejections(char **a)
{
    uint64_t *first = block<uint64_t>(4);
    first[0] = 0; first[1] = 2; first[2] = 2; first[3] = 5;
    uint8_t *dst = block<uint8_t>(52);
    say("write_delim", zs_ridx_write(dst, 52, first, 3, 256));
    say("write_too_many", zs_ridx_write(dst, 52, first, ZS_RIDX_MAX_FRAMES, 10));
    say("write_null", zs_ridx_write(dst, 52, nullptr, 3, 10));
    first[0] = 1; say("write_first_not_0", zs_ridx_write(dst, 52, first, 3, 10)); first[0] = 0;
    first[2] = 1; say("write_descends", zs_ridx_write(dst, 52, first, 3, 10)); first[2] = 2;
    say("write_short", zs_ridx_write(dst, 51, first, 3, 10));
    say("size_too_many", zs_ridx_size(ZS_RIDX_MAX_FRAMES));
    read_refusal("read_39_bytes", 39, 0, 0, 4);
    read_refusal("read_outer_magic", 52, 0, 1, 4);
    read_refusal("read_inner_magic", 52, 9, 0x40, 4);
    read_refusal("read_version", 52, 12, 3, 4);
    read_refusal("read_reserved_16", 52, 15, 0x80, 4);
    read_refusal("read_reserved_32", 52, 20, 1, 4);
    read_refusal("read_frame_size", 52, 4, 4, 4);
    read_refusal("read_n", 52, 16, 1, 4);
    read_refusal("read_cut", 51, 0, 0, 4);
    read_refusal("read_capacity", 52, 0, 0, 3);
    read_refusal("read_count", 52, 44, 1, 4);
    read_refusal("read_records", 52, 24, 1, 4);
    read_refusal("read_check", 52, 39, 0x80, 4);
    read_refusal("read_delim", 52, 13, 1, 4);
    read_refusal("read_good", 52, 0, 0, 4);
    // index
    uint8_t *text = block<uint8_t>(12);
    memcpy(text, "ab\ncd\nef\ngh\n", 12);
    uint32_t *sizes = block<uint32_t>(3);
    sizes[0] = sizes[1] = sizes[2] = 4;
    uint64_t *out = block<uint64_t>(4);
    sayc("index_delim", zs_ridx_index(text, 12, sizes, 3, -1, out, nullptr));
    sayc("index_null_sizes", zs_ridx_index(text, 12, nullptr, 3, 10, out, nullptr));
    sayc("index_null_first", zs_ridx_index(text, 12, sizes, 3, 10, nullptr, nullptr));
    sayc("index_null_text", zs_ridx_index(nullptr, 12, sizes, 3, 10, out, nullptr));
    sizes[2] = 3; sayc("index_sum", zs_ridx_index(text, 12, sizes, 3, 10, out, nullptr)); sizes[2] = 4;
    sayc("index_good", zs_ridx_index(text, 12, sizes, 3, 10, out, nullptr));
    // attach: out = {0, 1, 2, 4} fits the archive's entries (Decompressed_Size 4 each)
    size_t archiveSize;
    uint8_t *archive = slurp(a[0], archiveSize);
    const size_t entry = archive[archiveSize - 5] & 0x80 ? 12 : 8, grown = archiveSize + 52 + entry;
    uint8_t *room = block<uint8_t>(grown + 52 + entry);
    auto fresh = [&]() { memcpy(room, archive, archiveSize); };
    fresh(); room[archiveSize - 1] ^= 1; say("attach_table_magic", zs_ridx_attach(room, archiveSize, grown, out, 3, 10));
    fresh(); room[archiveSize - 5] |= 4; say("attach_table_reserved", zs_ridx_attach(room, archiveSize, grown, out, 3, 10));
    fresh(); say("attach_n", zs_ridx_attach(room, archiveSize, grown, out, 2, 10));
    fresh(); say("attach_delim", zs_ridx_attach(room, archiveSize, grown, out, 3, 300));
    fresh(); say("attach_null", zs_ridx_attach(room, archiveSize, grown, nullptr, 3, 10));
    fresh(); out[1] = 5; out[2] = 5; out[3] = 5; say("attach_count_above_frame", zs_ridx_attach(room, archiveSize, grown, out, 3, 10));
    out[1] = 2; out[2] = 1; out[3] = 4; say("attach_descends", zs_ridx_attach(room, archiveSize, grown, out, 3, 10));
    out[1] = 1; out[2] = 2;
    say("attach_short", zs_ridx_attach(room, archiveSize, grown - 1, out, 3, 10));
    printf("attach_untouched %d\n", memcmp(room, archive, archiveSize) == 0);
    say("attach_good", zs_ridx_attach(room, archiveSize, grown, out, 3, 10));
    uint64_t *longer = block<uint64_t>(5);
    longer[0] = 0; longer[1] = 1; longer[2] = 2; longer[3] = 4; longer[4] = 4;
    say("attach_twice", zs_ridx_attach(room, grown, grown + 52 + entry, longer, 4, 10));
    free(first); free(dst); free(text); free(sizes); free(out); free(archive); free(room); free(longer);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 3 && !strcmp(argv[1], "rejections")) return rejections(argv + 2);
    for (int a = 1; a + 5 < argc && !strcmp(argv[a], "case"); a += 6)
        if (const int rc = one_case(argv + a + 1)) return rc;
    return 0;
}
