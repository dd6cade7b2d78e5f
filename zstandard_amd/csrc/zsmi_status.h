// The size word, stated once: the uint32_t a kernel leaves per item and the host reads back is a byte count or (uint32_t)-code, the 32-bit
// form of what the C ABI returns as a size_t (zsmi_isError).  Everything derives from the enum of include/zsmi.h; no other file of the
// library spells the boundary out.  Host and device; a host program may include this header alone (tests/c/size_word.cpp does).
#pragma once
#include "../../include/zsmi.h"
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define ZS_STATUS_FN __host__ __device__ __forceinline__ constexpr
#else
#define ZS_STATUS_FN static inline constexpr
#endif
#define ZS_ERROR_WORD(code) (0u - (uint32_t)(code))
ZS_STATUS_FN uint32_t zs_error_word(uint32_t code) { return ZS_ERROR_WORD(code); }      // (the macro: a constant where a code is written out, the decoder's ZE())
// the largest word that is a size: a word above it is an error word (zsmi_isError: code > (size_t)-ZSMI_error_maxCode)
ZS_STATUS_FN uint32_t zs_word_max_size() { return zs_error_word(ZSMI_error_maxCode); }
ZS_STATUS_FN bool zs_word_is_error(uint32_t w) { return w > zs_word_max_size(); }
ZS_STATUS_FN uint32_t zs_word_code(uint32_t w) { return zs_word_is_error(w) ? 0u - w : 0u; }      // 0: no error
ZS_STATUS_FN uint32_t zs_word_bytes(uint32_t w) { return zs_word_is_error(w) ? 0u : w; }          // the bytes an item has: none behind an error
// the largest capacity a one-shot decode passes down for its destination (the caller's may be any size_t): below every error word
#define ZS_ONESHOT_CAP_MAX 0xFFFFFF00u
static_assert(ZS_ONESHOT_CAP_MAX <= zs_error_word(ZSMI_error_maxCode), "the one-shot capacity clamp must be a size, not an error word");
