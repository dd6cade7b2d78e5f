// Find records by content: which records of a buffer of delimited records hold a literal byte pattern - the step that SELECTS records, in
// front of zsmi_seekableReadRecordsResident, which takes the answer as it stands (ascending uint64 record numbers).  The rule, for
// text[0, len), a delimiter byte delim, a pattern P of m bytes (1 <= m <= ZS_FIND_MAX_PATTERN) none of which equals delim, and a base B:
//   1. An OCCURRENCE is a position p with p + m <= len and text[p, p + m) == P.  Overlapping occurrences all count ("aa" in "aaaa": 3).
//   2. The RECORD of p is B + the delimiters in text[0, p) - the splitter's rule 4 (zsmi_split.h).  P holds no delimiter, so the whole
//      occurrence lies in that record.
//   3. The ANSWER is the distinct records that hold an occurrence, ascending; total = their count; matches = the occurrence count.
// zs_find_records is the serial statement, and zsmi_findRecords runs it as written here.  The kernels of find.hip reach the same answer a
// workgroup a 16 KiB tile - occurrence and delimiter bit masks, a carry over the tiles for a record that holds occurrences in several of
// them, three scans - and share the argument checks.
// ON AN ARCHIVE the text is the content of frames [firstFrame, firstFrame + frameCount) as one run and B = firstRecord[firstFrame]; an
// occurrence that crosses the window's border is not found.  A frame f BEGINS a record exactly when f == 0 or firstRecord[f] !=
// firstRecord[f - 1]: the leading frames of a cut record hold no delimiter and share their entry (zsmi_split.h, rule 4), so only the first
// of them starts where a record starts.  Windows cut at such frames cut no record, hence no occurrence: together they find exactly what
// one window over all of them finds.  A window cut anywhere else may lose the occurrences across its border, and the record it begins
// inside is numbered as the one its first frame's entry names.
// NOT COVERED: patterns that hold the delimiter.  (Several patterns a call and ignoring case: zsmi_findquery.h; anchors and regular
// expressions: zsmi_regex.h.)
// Host and device; a host program may include this header alone, with any C++ compiler (tests/c/find_records.cpp does, under the
// sanitizers).
#pragma once
#include "../../include/zsmi.h"
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define ZS_FIND_FN __host__ __device__ __forceinline__
#else
#define ZS_FIND_FN static inline
#endif

#define ZS_FIND_MAX_PATTERN 256u          // the most bytes a pattern has: it travels by value in the kernels' arguments

// what every form of the call checks of these arguments, in the header's order (a NULL ctx, NULL arrays and the handle come in front)
ZS_FIND_FN int zs_find_check(int delim, const void *pattern, uint32_t m)
{
    if (delim < 0 || delim > 255) return ZSMI_error_parameter_outOfBound;
    if (m == 0 || m > ZS_FIND_MAX_PATTERN) return ZSMI_error_parameter_outOfBound;
    for (uint32_t i = 0; i < m; i++) if (((const uint8_t *)pattern)[i] == (uint8_t)delim) return ZSMI_error_parameter_outOfBound;
    return 0;
}

// the rule's loop (arguments checked by the caller): total.  out[0, min(total, capacity)) receives the first numbers, nothing is written
// behind them (capacity 0: out may be null); *matches (may be null) the occurrences.  Reads text[0, len) and P[0, m) only
ZS_FIND_FN uint64_t zs_find_records(const uint8_t *text, uint64_t len, uint8_t delim, const uint8_t *P, uint32_t m, uint64_t B,
                                    uint64_t *out, uint64_t capacity, uint64_t *matches)
{
    uint64_t total = 0, found = 0, record = B, last = 0;
    bool any = false;                                                     // `last` names a record
    for (uint64_t p = 0; p < len; p++) {
        if (len - p >= m) {
            uint32_t i = 0;
            while (i < m && text[p + i] == P[i]) i++;
            if (i == m) {
                found++;
                if (!any || last != record) {
                    if (total < capacity) out[total] = record;
                    total++; last = record; any = true;
                }
            }
        }
        if (text[p] == delim) record++;
    }
    if (matches) *matches = found;
    return total;
}
