// Find records by several patterns: which records of a buffer of delimited records hold ANY of K literal patterns, ALL of them or NONE
// (grep -e .. -e .., "both a request id and `timeout`", grep -v), with or without ASCII case folding (grep -i) - one search, one decode of
// an archive's window, beside the single-pattern search of zsmi_find.h, which it leaves as it is.  A query (zsmi_findQuery, include/zsmi.h)
// is K patterns, 1 <= K <= ZSMI_FIND_MAX_PATTERNS, of 1 .. 256 bytes each and at most ZS_FIND_MAX_PATTERN together, a mode and flags.  The
// rule, for text[0, len), a delimiter byte delim and a base B:
//   1. FOLDING.  fold(b) = b + 0x20 for b in 'A' .. 'Z' when ZSMI_FIND_IGNORE_CASE is set, b otherwise.  Only ASCII letters fold; bytes of
//      0x80 and above are never touched.
//   2. OCCURRENCES.  An occurrence of pattern j is a position p with p + m_j <= len and fold(text[p + i]) == fold(P_j[i]) for every i.
//      Overlapping occurrences count, and so do occurrences of two patterns at one position.
//   3. PATTERN BYTES AND DELIMITERS.  No pattern byte may satisfy fold(P_j[i]) == fold(delim).  A text byte is a delimiter exactly when it
//      equals delim, UNFOLDED ('a' is none of delimiter 'A', and no pattern may hold either).  So an occurrence holds no delimiter and
//      lies in one record.
//   4. RECORDS.  The splitter's (zsmi_split.h, rule 1): one ends behind each delimiter, bytes behind the last delimiter are a last record;
//      they are numbered B, B + 1, ...
//   5. HIT SETS.  H(r): the j with an occurrence of P_j in record r, an 8-bit word with bit j.
//   6. THE ANSWER.  The records whose H satisfies the mode, ascending - any: H != 0; all: H holds every j < K; none: H == 0 (grep -v; empty
//      records satisfy it).  total = their count; matches = the occurrences summed over the patterns; hits[k] = H of the k-th record
//      written, where asked for.
// Two consequences the tests use: with K = 1, `any` and no flag the answer is zs_find_records'; `any` is the union and `all` the
// intersection of the K single-pattern answers (folded), `none` the complement of `any` within the text's records.
// zs_findq_records is the serial statement, and zsmi_findRecordsQuery runs it as written here; the kernels of findquery.hip reach the same
// answer a workgroup a 16 KiB tile.  On an archive the window, B and the record-beginning frames are those of zsmi_find.h.
// NOT COVERED: patterns that hold the delimiter, Unicode case folding, more than 8 patterns, and occurrence counts a pattern.  (Anchors
// and regular expressions: zsmi_regex.h.)
// Host and device; a host program may include this header alone, with any C++ compiler (tests/c/find_query.cpp does, under the
// sanitizers).
#pragma once
#include "zsmi_find.h"

ZS_FIND_FN uint8_t zs_findq_fold(uint8_t b, uint32_t flags)
{
    return (uint8_t)((flags & ZSMI_FIND_IGNORE_CASE) && b >= (uint8_t)'A' && b <= (uint8_t)'Z' ? b + 0x20u : b);
}
// rule 6: does a record with hit set H belong to the answer
ZS_FIND_FN bool zs_findq_listed(uint32_t H, uint32_t mode, uint32_t K)
{
    return mode == ZSMI_find_any ? H != 0u : mode == ZSMI_find_all ? H == (1u << K) - 1u : H == 0u;
}

// what every form of the call checks of a non-NULL query, in this order (a NULL ctx, NULL arrays, a NULL q and the handle come in front):
// delim; nPatterns, mode, flags; then a pattern at a time its pointer, its size and the sum of the sizes so far; then, with every size
// known to be in range, the pattern bytes against the delimiter (rule 3) - zs_find_check's checks for every pattern, folded
ZS_FIND_FN int zs_findq_check(int delim, const zsmi_findQuery *q)
{
    if (delim < 0 || delim > 255) return ZSMI_error_parameter_outOfBound;
    if (q->nPatterns == 0 || q->nPatterns > ZSMI_FIND_MAX_PATTERNS || q->mode > ZSMI_find_none || (q->flags & ~ZSMI_FIND_IGNORE_CASE)) return ZSMI_error_parameter_outOfBound;
    uint32_t sum = 0;
    for (uint32_t j = 0; j < q->nPatterns; j++) {
        if (!q->patterns[j]) return ZSMI_error_GENERIC;
        if (q->patternSizes[j] == 0 || q->patternSizes[j] > ZS_FIND_MAX_PATTERN) return ZSMI_error_parameter_outOfBound;
        sum += q->patternSizes[j];
        if (sum > ZS_FIND_MAX_PATTERN) return ZSMI_error_parameter_outOfBound;
    }
    const uint8_t d = zs_findq_fold((uint8_t)delim, q->flags);
    for (uint32_t j = 0; j < q->nPatterns; j++)
        for (uint32_t i = 0; i < q->patternSizes[j]; i++)
            if (zs_findq_fold(((const uint8_t *)q->patterns[j])[i], q->flags) == d) return ZSMI_error_parameter_outOfBound;
    return 0;
}

// the rule's loop (arguments checked by the caller): total.  out[0, min(total, capacity)) receives the first numbers and hits[..] (may be
// null) their hit sets, nothing is written behind them (capacity 0: out may be null); *matches (may be null) the occurrences.  Reads
// text[0, len) and the patterns' bytes only
ZS_FIND_FN uint64_t zs_findq_records(const uint8_t *text, uint64_t len, uint8_t delim, const zsmi_findQuery *q, uint64_t B,
                                     uint64_t *out, uint8_t *hits, uint64_t capacity, uint64_t *matches)
{
    const uint32_t K = q->nPatterns;
    uint64_t total = 0, found = 0, record = B;
    uint32_t H = 0;
    for (uint64_t p = 0; p < len; p++) {
        for (uint32_t j = 0; j < K; j++) {
            const uint8_t *P = (const uint8_t *)q->patterns[j];
            const uint32_t m = q->patternSizes[j];
            if (len - p < m) continue;
            uint32_t i = 0;
            while (i < m && zs_findq_fold(text[p + i], q->flags) == zs_findq_fold(P[i], q->flags)) i++;
            if (i == m) { found++; H |= 1u << j; }
        }
        const bool last = p + 1 == len;
        if (text[p] == delim || last) {                                    // the record ends here: behind its delimiter, or with the text
            if (zs_findq_listed(H, q->mode, K)) {
                if (total < capacity) { out[total] = record; if (hits) hits[total] = (uint8_t)H; }
                total++;
            }
            record++; H = 0;
        }
    }
    if (matches) *matches = found;
    return total;
}
