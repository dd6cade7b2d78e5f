// Stand-alone host program over the size word (zstandard_amd/csrc/zsmi_status.h, included alone): the uint32_t that is a byte count or
// (uint32_t)-code.  It checks the header against itself - every code 1 .. 119 makes an error word that gives the code back and has no
// bytes, the boundary lies where zsmi_isError has it, the one-shot capacity clamp is a size - and prints a line per word it looked at
// (word verdict code bytes), which tests/test_size_word.py holds against the library's zsmi_isError of the code widened to size_t.
#include "zsmi_status.h"
#include <cstdio>
#include <cstdlib>

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "size_word.cpp:%d: %s\n", __LINE__, #cond); failures++; } } while (0)

static void show(uint32_t w) { printf("%u %d %u %u\n", w, zs_word_is_error(w) ? 1 : 0, zs_word_code(w), zs_word_bytes(w)); }

int main()
{
    static_assert(zs_error_word(ZSMI_error_maxCode) == 0u - 120u, "the boundary is (uint32_t)-120");
    for (uint32_t code = 1; code < ZSMI_error_maxCode; code++) {
        const uint32_t w = zs_error_word(code);
        CHECK(zs_word_is_error(w));
        CHECK(zs_word_code(w) == code);
        CHECK(zs_word_bytes(w) == 0);
        CHECK(w == (uint32_t)((size_t)0 - (size_t)code));            // the low 32 bits of what the C ABI returns
        show(w);
    }
    const uint32_t last = zs_error_word(ZSMI_error_maxCode);         // the largest size
    CHECK(ZSMI_error_maxCode == 120 && last == 0xFFFFFF88u);
    CHECK(!zs_word_is_error(0xFFFFFF88u) && zs_word_is_error(0xFFFFFF89u));
    CHECK(!zs_word_is_error(last) && zs_word_code(last) == 0 && zs_word_bytes(last) == last);
    CHECK(zs_word_is_error(last + 1) && zs_word_code(last + 1) == ZSMI_error_maxCode - 1 && zs_word_bytes(last + 1) == 0);
    CHECK(!zs_word_is_error(0) && zs_word_code(0) == 0 && zs_word_bytes(0) == 0);
    CHECK(!zs_word_is_error(1) && zs_word_bytes(1) == 1);
    CHECK(zs_word_is_error(~0u) && zs_word_code(~0u) == ZSMI_error_GENERIC);
    CHECK(zs_word_max_size() == last);
    CHECK(ZS_ONESHOT_CAP_MAX < zs_error_word(ZSMI_error_maxCode - 1));      // below the first error word
    CHECK(!zs_word_is_error(ZS_ONESHOT_CAP_MAX) && zs_word_bytes(ZS_ONESHOT_CAP_MAX) == ZS_ONESHOT_CAP_MAX);
    show(last); show(last + 1); show(0); show(ZS_ONESHOT_CAP_MAX);
    return failures ? 1 : 0;
}
