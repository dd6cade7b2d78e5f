// Find records by regular expression: which records of a buffer of delimited records a regular expression matches (grep -E), a third
// search beside zsmi_find.h and zsmi_findquery.h, which it leaves as they are.  A pattern is compiled on the HOST (zs_regex_compile) into
// a program (zsmi_regexProgram, include/zsmi.h): THE minimal complete DFA over byte classes.  The rule, for text[0, len), a delimiter byte
// delim, a program and a base B:
//   1. RECORDS.  The splitter's (zsmi_split.h, rule 1): one ends behind each delimiter, bytes behind the last delimiter are a last record,
//      empty records exist; they are numbered B, B + 1, ...  A record is a byte string WITHOUT its delimiter.
//   2. MATCH.  A record matches exactly when Python's re.compile(pattern, re.DOTALL | (re.IGNORECASE if the flag is set else 0))
//      .search(record) succeeds.  Only existence counts, so greedy against lazy and leftmost priority play no part and a DFA is exact.
//   3. THE DELIMITER is a parameter of the search, not of the program: a text byte equal to delim, UNFOLDED, ends a record and is never
//      fed to the program.  A `.`, a negated class or \s that could match it therefore never sees it; nothing is refused for it.
//   4. THE PROGRAM.  next[s * nClasses + classOf[b]] is the state behind byte b from state s; a record starts in `start`; it matches when
//      it ends in a state s with bit s of `accept` set.
//   5. THE ANSWER.  The matching records, ascending; with ZSMI_REGEX_INVERT the others (grep -v; empty records included where they do not
//      match).  total = their count; textRecords = the records of the text: the delimiters, + 1 for bytes behind the last.
// SYNTAX.  Patterns are bytes; a byte of 0x80 or above is a literal.  Literals; `\` before a non-alphanumeric byte stands for that byte;
// \t \n \r \f \v \xHH; \d \D \w \W \s \S with the ASCII sets of Python's bytes patterns; `.` (any byte); classes [...] and [^...] with
// ranges and the escapes above inside - a `]` directly behind `[` or `[^` is a literal, a `-` first or last is a literal (an item, then
// `-`, then an item is a range, as Python reads it), a `[` inside is a literal; ( ), (?: ) and | - an empty alternative matches the empty
// string; * + ?; {m}, {m,} and {m,n} with m <= n <= 255; ^ only as the first item of a top-level alternative (the record's start); $ only
// as the last item of a top-level alternative (the record's end).  Under ZSMI_FIND_IGNORE_CASE a literal or a positive class is closed
// under swapping ASCII case BEFORE a class is negated; bytes outside the letters are untouched.
// REFUSALS, in this order (errorAt: the pattern offset at which the refusal was decided):
//   1. a NULL pattern or prog: GENERIC.
//   2. patternSize 0, or unknown flag bits: parameter_outOfBound (errorAt 0).
//   3. a recognised construct that is left out: parameter_unsupported, found by one pass over the pattern's tokens before anything is
//      parsed, so that it comes in front of every refusal of 4 - ^ or $ elsewhere (errorAt: the anchor); \b \B \A \Z, backreferences and
//      any other `\` followed by a letter or digit (the `\`); (? followed by anything but `:` (the `(`); the lazy and possessive suffixes
//      *? +? ?? {..}? *+ ++ ?+ {..}+ (the suffix).
//   4. malformed input: parameter_outOfBound - an unbalanced ( or [ (errorAt: the bracket), an unbalanced ) (the bracket); a quantifier
//      with nothing to repeat or on top of another quantifier (the quantifier); a { that does not open one of the three forms above (the
//      brace; Python's fallback of reading it as a literal is deliberately not mimicked); a reversed range, a range that starts or ends in
//      a class escape (the range's first item); a trailing `\`; bad hex in \xHH (the `\`); groups nested deeper than 200 (the bracket).
//   5. a program above the caps, after minimisation: parameter_outOfBound with errorAt = patternSize.  The caps: nStates <= 64, nClasses
//      <= 256, nStates * nClasses <= 3072.  The construction gives up with the same refusal when it holds more than 32768 NFA states,
//      more than 4096 DFA states, more than 64 classes of states while minimising, or once the subset construction has touched more
//      than 2 * 10^8 NFA-state entries (the members of every set it stepped from and to: a time bound, about a second, that a pattern
//      within the other three can still reach - 4096 sets of thousands of NFA states over 256 classes), so that a pattern like a.{20}b
//      ends quickly.
// CONSTRUCTION.  A Thompson NFA over the record framed by two virtual symbols, begin and end: ^ and $ consume them, and the search wrapper
// .*(R).* spans them.  Subset construction over byte classes - bytes that every atom treats alike share a class, numbered in the order
// of their first byte.  Minimisation (Moore) to the minimal complete DFA; a dead state is kept only where it is reachable; the states are
// numbered in breadth-first order from `start`, classes ascending.  `start` is the state behind the begin symbol, `accept` the states from
// which the end symbol accepts.  The device never sees the virtual symbols.  So the size of a program is a fact: abc 4, abc$ 4, ^abc 5,
// ^abc$ 5, a|b 2, a* 1.
// zs_regex_records is the serial statement, and zsmi_findRecordsRegex runs it as written here; the kernels of findregex.hip reach the same
// answer a workgroup a 16 KiB tile.  On an archive the window, B and the record-beginning frames are those of zsmi_find.h; a record that
// the window's border cuts is judged on the part inside the window.
// NOT COVERED: patterns that hold the delimiter, Unicode, word boundaries, backreferences, more than 64 states.
// zs_regex_check and zs_regex_records: host and device.  The compiler: host only, C++11; a host program may include this header alone, with
// any C++ compiler (tests/c/find_regex.cpp does, under the sanitizers).
#pragma once
#include "zsmi_find.h"            // include/zsmi.h, ZS_FIND_FN
#include <algorithm>
#include <cstring>
#include <map>
#include <vector>

#define ZS_REGEX_FLAGS (ZSMI_FIND_IGNORE_CASE | ZSMI_REGEX_INVERT)

// what every form of the call checks of a non-NULL program (a NULL ctx, NULL arrays, a NULL prog and the handle come in front): delim and
// the flags, then that no index the program holds can leave a table
ZS_FIND_FN int zs_regex_check(int delim, const zsmi_regexProgram *prog)
{
    if (delim < 0 || delim > 255) return ZSMI_error_parameter_outOfBound;
    if (prog->flags & ~ZS_REGEX_FLAGS) return ZSMI_error_parameter_outOfBound;
    const uint32_t n = prog->nStates, nc = prog->nClasses;
    if (n == 0 || n > ZSMI_REGEX_MAX_STATES || nc == 0 || nc > 256u || n * nc > ZSMI_REGEX_MAX_TABLE) return ZSMI_error_parameter_outOfBound;
    if (prog->start >= n) return ZSMI_error_parameter_outOfBound;
    for (uint32_t b = 0; b < 256u; b++) if (prog->classOf[b] >= nc) return ZSMI_error_parameter_outOfBound;
    for (uint32_t i = 0; i < n * nc; i++) if (prog->next[i] >= n) return ZSMI_error_parameter_outOfBound;
    if (n < 64u && (prog->accept >> n)) return ZSMI_error_parameter_outOfBound;
    return 0;
}
// rule 5: does a record that ends in state s belong to the answer
ZS_FIND_FN bool zs_regex_listed(uint64_t accept, uint32_t invert, uint32_t s) { return (((accept >> s) & 1ull) != 0ull) != (invert != 0u); }

// the rule's loop (arguments checked by the caller): total.  out[0, min(total, capacity)) receives the first numbers, nothing is written
// behind them (capacity 0: out may be null); *textRecords (may be null) the records of the text.  Reads text[0, len) and the program only
ZS_FIND_FN uint64_t zs_regex_records(const uint8_t *text, uint64_t len, uint8_t delim, const zsmi_regexProgram *prog, uint64_t B,
                                     uint64_t *out, uint64_t capacity, uint64_t *textRecords)
{
    const uint32_t nc = prog->nClasses, invert = prog->flags & ZSMI_REGEX_INVERT;
    uint64_t total = 0, record = B;
    uint32_t s = prog->start;
    for (uint64_t p = 0; p < len; p++) {
        const bool isDelim = text[p] == delim;
        if (!isDelim) s = prog->next[s * nc + prog->classOf[text[p]]];
        if (isDelim || p + 1 == len) {                                     // the record ends here: at its delimiter, or with the text
            if (zs_regex_listed(prog->accept, invert, s)) {
                if (total < capacity) out[total] = record;
                total++;
            }
            record++; s = prog->start;
        }
    }
    if (textRecords) *textRecords = record - B;
    return total;
}

// ---------------------------------------------------------------------------------------------
// the compiler (host)
// ---------------------------------------------------------------------------------------------
struct ZsReSet {                                                           // a set of bytes
    uint64_t w[4];
    bool has(uint32_t b) const { return (w[b >> 6] >> (b & 63u)) & 1ull; }
    void add(uint32_t b) { w[b >> 6] |= 1ull << (b & 63u); }
    void range(uint32_t lo, uint32_t hi) { for (uint32_t b = lo; b <= hi; b++) add(b); }
    void join(const ZsReSet &o) { for (int i = 0; i < 4; i++) w[i] |= o.w[i]; }
    void negate() { for (int i = 0; i < 4; i++) w[i] = ~w[i]; }
    void closeCase()                                                       // with a letter its other case
    {
        for (uint32_t b = 'a'; b <= 'z'; b++) {
            if (has(b)) add(b - 0x20u);
            else if (has(b - 0x20u)) add(b);
        }
    }
    bool same(const ZsReSet &o) const { return w[0] == o.w[0] && w[1] == o.w[1] && w[2] == o.w[2] && w[3] == o.w[3]; }
};
static inline ZsReSet zs_re_empty() { ZsReSet s; s.w[0] = s.w[1] = s.w[2] = s.w[3] = 0; return s; }
static inline bool zs_re_alnum(uint32_t b) { return (b >= '0' && b <= '9') || (b >= 'a' && b <= 'z') || (b >= 'A' && b <= 'Z'); }
static inline bool zs_re_digit(uint32_t b) { return b >= '0' && b <= '9'; }
static inline int zs_re_hex(uint32_t b) { return zs_re_digit(b) ? (int)(b - '0') : b >= 'a' && b <= 'f' ? (int)(b - 'a' + 10) : b >= 'A' && b <= 'F' ? (int)(b - 'A' + 10) : -1; }
// a brace quantifier {m} {m,} {m,n} at p[at] == '{': its length in bytes, 0 where the braces do not hold one of the three forms (the
// values are checked by the parser); lo, hi (-1: none) as read, capped
static inline size_t zs_re_braces(const uint8_t *p, size_t n, size_t at, int *lo, int *hi)
{
    size_t i = at + 1;
    int v[2] = { 0, -1 };
    if (i >= n || !zs_re_digit(p[i])) return 0;
    for (; i < n && zs_re_digit(p[i]); i++) v[0] = std::min(v[0] * 10 + (int)(p[i] - '0'), 100000);
    if (i < n && p[i] == ',') {
        i++;
        if (i < n && zs_re_digit(p[i])) { v[1] = 0; for (; i < n && zs_re_digit(p[i]); i++) v[1] = std::min(v[1] * 10 + (int)(p[i] - '0'), 100000); }
    } else v[1] = v[0];
    if (i >= n || p[i] != '}') return 0;
    if (lo) *lo = v[0];
    if (hi) *hi = v[1];
    return i + 1 - at;
}
// the end of the class that opens at p[at] == '[' (the offset behind its `]`; n where none closes it), as both passes read it
static inline size_t zs_re_class_end(const uint8_t *p, size_t n, size_t at)
{
    size_t i = at + 1;
    if (i < n && p[i] == '^') i++;
    if (i < n && p[i] == ']') i++;
    for (; i < n; i++) {
        if (p[i] == '\\') { i++; continue; }
        if (p[i] == ']') return i + 1;
    }
    return n;
}
// refusal 3: the constructs that are recognised and left out, by the pattern's tokens alone.  0, or parameter_unsupported with *where
static inline int zs_re_unsupported(const uint8_t *p, size_t n, size_t *where)
{
    static const char kEscapes[] = "tnrfvxdDwWsS";
    size_t depth = 0;
    bool altStart = true, prevQuant = false;
    for (size_t i = 0; i < n; ) {
        const uint8_t c = p[i];
        bool quant = false;
        size_t step = 1;
        if (c == '\\') {
            if (i + 1 < n && zs_re_alnum(p[i + 1]) && !memchr(kEscapes, p[i + 1], sizeof kEscapes - 1)) { *where = i; return ZSMI_error_parameter_unsupported; }
            step = 2;
        } else if (c == '[') {
            for (size_t j = i + 1, end = zs_re_class_end(p, n, i); j + 1 < end; j++)
                if (p[j] == '\\') {
                    if (zs_re_alnum(p[j + 1]) && !memchr(kEscapes, p[j + 1], sizeof kEscapes - 1)) { *where = j; return ZSMI_error_parameter_unsupported; }
                    j++;
                }
            step = zs_re_class_end(p, n, i) - i;
        } else if (c == '(') {
            if (i + 1 < n && p[i + 1] == '?') {
                if (!(i + 2 < n && p[i + 2] == ':')) { *where = i; return ZSMI_error_parameter_unsupported; }
                step = 3;
            }
            depth++;
        } else if (c == ')') {
            if (depth) depth--;
        } else if (c == '^') {
            if (depth || !altStart) { *where = i; return ZSMI_error_parameter_unsupported; }
        } else if (c == '$') {
            if (depth || !(i + 1 == n || p[i + 1] == '|')) { *where = i; return ZSMI_error_parameter_unsupported; }
        } else if (c == '*' || c == '+' || c == '?') {
            if (prevQuant && c != '*') { *where = i; return ZSMI_error_parameter_unsupported; }
            quant = true;
        } else if (c == '{') {
            const size_t len = zs_re_braces(p, n, i, nullptr, nullptr);
            if (len) { quant = true; step = len; }
        }
        altStart = c == '|' && depth == 0;
        prevQuant = quant;
        i += step;
    }
    return 0;
}

enum { kZsReSet, kZsReBegin, kZsReEnd, kZsReCat, kZsReAlt, kZsReRep };
struct ZsReNode { int kind, set, lo, hi; std::vector<int> kids; };        // a set's index; a repeat's bounds (hi -1: none)
struct ZsReParser {
    const uint8_t *p; size_t n; uint32_t flags; size_t at; int err; size_t errAt;
    std::vector<ZsReNode> nodes;
    std::vector<ZsReSet> sets;
    int fail(size_t where) { if (!err) { err = ZSMI_error_parameter_outOfBound; errAt = where; } return -1; }
    int node(int kind, int set = -1, int lo = 0, int hi = 0)
    {
        ZsReNode nd; nd.kind = kind; nd.set = set; nd.lo = lo; nd.hi = hi;
        nodes.push_back(nd);
        return (int)nodes.size() - 1;
    }
    int setNode(const ZsReSet &s)
    {
        for (size_t i = 0; i < sets.size(); i++) if (sets[i].same(s)) return node(kZsReSet, (int)i);
        sets.push_back(s);
        return node(kZsReSet, (int)sets.size() - 1);
    }
    // an escape at p[at] == '\\' -> its set; *byte: the byte it stands for, -1 for a class escape
    bool escape(ZsReSet &s, int *byte)
    {
        const size_t open = at;
        s = zs_re_empty(); *byte = -1;
        if (at + 1 >= n) { fail(open); return false; }
        const uint8_t e = p[at + 1];
        at += 2;
        switch (e) {
        case 't': *byte = 9; break;
        case 'n': *byte = 10; break;
        case 'v': *byte = 11; break;
        case 'f': *byte = 12; break;
        case 'r': *byte = 13; break;
        case 'x': {
            const int h = at < n ? zs_re_hex(p[at]) : -1, l = at + 1 < n ? zs_re_hex(p[at + 1]) : -1;
            if (h < 0 || l < 0) { fail(open); return false; }
            *byte = h * 16 + l; at += 2; break;
        }
        case 'd': case 'D': s.range('0', '9'); break;
        case 'w': case 'W': s.range('0', '9'); s.range('a', 'z'); s.range('A', 'Z'); s.add('_'); break;
        case 's': case 'S': s.range(9, 13); s.add(' '); break;
        default:
            if (zs_re_alnum(e)) { if (!err) { err = ZSMI_error_parameter_unsupported; errAt = open; } return false; }   // (the first pass refuses these)
            *byte = e;
        }
        if (*byte >= 0) s.add((uint32_t)*byte);
        else if (e == 'D' || e == 'W' || e == 'S') s.negate();
        return true;
    }
    int klass()
    {
        const size_t open = at;
        ZsReSet s = zs_re_empty();
        at++;
        const bool neg = at < n && p[at] == '^';
        if (neg) at++;
        for (bool first = true; ; first = false) {
            if (at >= n) return fail(open);
            if (p[at] == ']' && !first) { at++; break; }
            const size_t item = at;
            ZsReSet a; int lo = p[at];
            if (p[at] == '\\') { if (!escape(a, &lo)) return -1; } else { a = zs_re_empty(); a.add((uint32_t)lo); at++; }
            if (at < n && p[at] == '-' && !(at + 1 < n && p[at + 1] == ']') && at + 1 < n) {      // a range
                at++;
                ZsReSet b; int hi = p[at];
                if (p[at] == '\\') { if (!escape(b, &hi)) return -1; } else at++;
                if (lo < 0 || hi < 0 || hi < lo) return fail(item);
                s.range((uint32_t)lo, (uint32_t)hi);
            } else s.join(a);
        }
        if (flags & ZSMI_FIND_IGNORE_CASE) s.closeCase();
        if (neg) s.negate();
        return setNode(s);
    }
    int regex(size_t depth)                                                // alternatives up to a `)` or the pattern's end
    {
        std::vector<int> alts;
        for (;;) {
            const int a = sequence(depth);
            if (a < 0) return -1;
            alts.push_back(a);
            if (at < n && p[at] == '|') { at++; continue; }
            break;
        }
        if (alts.size() == 1) return alts[0];
        const int r = node(kZsReAlt);
        nodes[(size_t)r].kids = alts;
        return r;
    }
    int sequence(size_t depth)
    {
        std::vector<int> items;
        while (at < n && p[at] != '|' && p[at] != ')') {
            const uint8_t c = p[at];
            int atom;
            if (c == '^') { items.push_back(node(kZsReBegin)); at++; continue; }      // (the first pass: a top-level alternative's first item)
            if (c == '$') { items.push_back(node(kZsReEnd)); at++; continue; }        // (its last)
            if (c == '(') {
                const size_t open = at;
                at += at + 2 < n && p[at + 1] == '?' && p[at + 2] == ':' ? 3 : 1;
                if (depth + 1 > 200) return fail(open);
                atom = regex(depth + 1);
                if (atom < 0) return -1;
                if (at >= n || p[at] != ')') return fail(open);
                at++;
            } else if (c == '[') {
                atom = klass();
                if (atom < 0) return -1;
            } else if (c == '.') {
                ZsReSet s = zs_re_empty(); s.negate(); atom = setNode(s); at++;
            } else if (c == '\\') {
                ZsReSet s; int byte;
                if (!escape(s, &byte)) return -1;
                if (byte >= 0 && (flags & ZSMI_FIND_IGNORE_CASE)) s.closeCase();
                atom = setNode(s);
            } else if (c == '*' || c == '+' || c == '?' || c == '{') {
                return fail(at);                                           // nothing to repeat, or a brace that opens no quantifier
            } else {
                ZsReSet s = zs_re_empty(); s.add(c);
                if (flags & ZSMI_FIND_IGNORE_CASE) s.closeCase();
                atom = setNode(s); at++;
            }
            if (at < n && (p[at] == '*' || p[at] == '+' || p[at] == '?' || p[at] == '{')) {
                int lo = 0, hi = -1;
                if (p[at] == '{') {
                    const size_t len = zs_re_braces(p, n, at, &lo, &hi);
                    if (!len || lo > 255 || hi > 255 || (hi >= 0 && hi < lo)) return fail(at);
                    at += len;
                } else {
                    if (p[at] == '+') lo = 1;
                    if (p[at] == '?') hi = 1;
                    at++;
                }
                const int r = node(kZsReRep, -1, lo, hi);
                nodes[(size_t)r].kids.push_back(atom);
                atom = r;
                if (at < n && (p[at] == '*' || p[at] == '+' || p[at] == '?' || p[at] == '{')) return fail(at);      // on top of another quantifier
            }
            items.push_back(atom);
        }
        const int r = node(kZsReCat);
        nodes[(size_t)r].kids = items;
        return r;
    }
};

// the NFA: a state consumes one symbol (a byte of a set, begin, end, or any of them) towards out1, or passes on for nothing to out1 and out2
enum { kZsNfaEps, kZsNfaSet, kZsNfaBegin, kZsNfaEnd, kZsNfaAny, kZsNfaFinal };
struct ZsNfaState { int kind, set, out1, out2; };
struct ZsNfa {
    std::vector<ZsNfaState> st;
    bool over;
    int add(int kind, int set = -1) { if (st.size() > 32768u) { over = true; return 0; } ZsNfaState s = { kind, set, -1, -1 }; st.push_back(s); return (int)st.size() - 1; }
    // the fragment of a node: (first state, last state - an eps state nothing leaves yet)
    void emit(const std::vector<ZsReNode> &nodes, int id, int &first, int &last)
    {
        const ZsReNode &nd = nodes[(size_t)id];
        if (over) { first = last = 0; return; }
        switch (nd.kind) {
        case kZsReSet: case kZsReBegin: case kZsReEnd:
            first = add(nd.kind == kZsReSet ? kZsNfaSet : nd.kind == kZsReBegin ? kZsNfaBegin : kZsNfaEnd, nd.set);
            last = add(kZsNfaEps); st[(size_t)first].out1 = last;
            return;
        case kZsReCat:
            first = last = add(kZsNfaEps);
            for (size_t i = 0; i < nd.kids.size() && !over; i++) {
                int f, l;
                emit(nodes, nd.kids[i], f, l);
                st[(size_t)last].out1 = f; last = l;
            }
            return;
        case kZsReAlt: {
            first = add(kZsNfaEps); last = add(kZsNfaEps);
            int fork = first;
            for (size_t i = 0; i < nd.kids.size() && !over; i++) {
                int f, l;
                emit(nodes, nd.kids[i], f, l);
                st[(size_t)l].out1 = last;
                st[(size_t)fork].out1 = f;
                if (i + 1 < nd.kids.size()) { const int more = add(kZsNfaEps); st[(size_t)fork].out2 = more; fork = more; }
            }
            return;
        }
        default: {                                                         // a repeat: lo copies, then a loop or hi - lo copies that may each be left out
            first = last = add(kZsNfaEps);
            for (int i = 0; i < nd.lo && !over; i++) {
                int f, l;
                emit(nodes, nd.kids[0], f, l);
                st[(size_t)last].out1 = f; last = l;
            }
            if (nd.hi < 0) {
                int f, l;
                emit(nodes, nd.kids[0], f, l);
                const int loop = add(kZsNfaEps), end = add(kZsNfaEps);
                st[(size_t)last].out1 = loop;
                st[(size_t)loop].out1 = f; st[(size_t)loop].out2 = end;
                st[(size_t)l].out1 = loop;
                last = end;
            } else {
                const int end = add(kZsNfaEps);
                for (int i = nd.lo; i < nd.hi && !over; i++) {
                    int f, l;
                    emit(nodes, nd.kids[0], f, l);
                    const int fork = add(kZsNfaEps);
                    st[(size_t)last].out1 = fork;
                    st[(size_t)fork].out1 = f; st[(size_t)fork].out2 = end;
                    last = l;
                }
                st[(size_t)last].out1 = end; last = end;
            }
            return;
        }
        }
    }
};
// subset construction: the states that can be reached for nothing from those of `from`, kept as the sorted list of the ones that consume
// a symbol or accept
struct ZsReSubsets {
    const ZsNfa &nfa;
    std::vector<uint32_t> mark, stack;
    uint32_t stamp;
    explicit ZsReSubsets(const ZsNfa &a) : nfa(a), mark(a.st.size(), 0u), stamp(0) {}
    void close(const std::vector<int> &from, std::vector<int> &out)
    {
        stamp++; out.clear(); stack.clear();
        for (size_t i = 0; i < from.size(); i++) if (mark[(size_t)from[i]] != stamp) { mark[(size_t)from[i]] = stamp; stack.push_back((uint32_t)from[i]); }
        while (!stack.empty()) {
            const uint32_t s = stack.back(); stack.pop_back();
            const ZsNfaState &q = nfa.st[s];
            if (q.kind != kZsNfaEps) { out.push_back((int)s); continue; }
            const int outs[2] = { q.out1, q.out2 };
            for (int k = 0; k < 2; k++) if (outs[k] >= 0 && mark[(size_t)outs[k]] != stamp) { mark[(size_t)outs[k]] = stamp; stack.push_back((uint32_t)outs[k]); }
        }
        std::sort(out.begin(), out.end());
    }
    // behind a symbol: a byte (sets: the pattern's, with the byte's membership), or begin / end (byte -1, the state kind that consumes it)
    void step(const std::vector<int> &from, const std::vector<ZsReSet> &sets, int byte, int kind, std::vector<int> &out)
    {
        std::vector<int> moved;
        for (size_t i = 0; i < from.size(); i++) {
            const ZsNfaState &q = nfa.st[(size_t)from[i]];
            const bool takes = q.kind == kZsNfaAny || (byte >= 0 ? q.kind == kZsNfaSet && sets[(size_t)q.set].has((uint32_t)byte) : q.kind == kind);
            if (takes) moved.push_back(q.out1);
        }
        close(moved, out);
    }
};

// pattern -> program: 0, or the code of a refusal (the list in this file's head) with *errorAt, and prog is not written
static inline int zs_regex_compile(const void *pattern, size_t patternSize, uint32_t flags, zsmi_regexProgram *prog, size_t *errorAt)
{
    size_t unused;
    size_t &where = errorAt ? *errorAt : unused;
    where = 0;
    if (!pattern || !prog) return ZSMI_error_GENERIC;
    if (patternSize == 0 || (flags & ~ZS_REGEX_FLAGS)) return ZSMI_error_parameter_outOfBound;
    const uint8_t *p = (const uint8_t *)pattern;
    if (const int e = zs_re_unsupported(p, patternSize, &where)) return e;
    ZsReParser ps;
    ps.p = p; ps.n = patternSize; ps.flags = flags; ps.at = 0; ps.err = 0; ps.errAt = 0;
    const int root = ps.regex(0);
    if (root >= 0 && ps.at < patternSize) ps.fail(ps.at);                  // a `)` that closes nothing
    if (ps.err) { where = ps.errAt; return ps.err; }
    where = patternSize;                                                   // from here on: the size refusal
    // the NFA of any* R any* over the framed record
    ZsNfa nfa; nfa.over = false;
    const int s0 = nfa.add(kZsNfaEps), front = nfa.add(kZsNfaAny), t0 = nfa.add(kZsNfaEps), back = nfa.add(kZsNfaAny), fin = nfa.add(kZsNfaFinal);
    int f, l;
    nfa.emit(ps.nodes, root, f, l);
    if (nfa.over) return ZSMI_error_parameter_outOfBound;
    nfa.st[(size_t)s0].out1 = front; nfa.st[(size_t)s0].out2 = f; nfa.st[(size_t)front].out1 = s0;
    nfa.st[(size_t)l].out1 = t0;
    nfa.st[(size_t)t0].out1 = back; nfa.st[(size_t)t0].out2 = fin; nfa.st[(size_t)back].out1 = t0;
    // byte classes: bytes that every set treats alike, in the order of their first byte
    uint8_t classOf[256], rep[256];
    uint32_t nc = 0;
    {
        std::map<std::vector<bool>, uint32_t> seen;
        for (uint32_t b = 0; b < 256u; b++) {
            std::vector<bool> sig(ps.sets.size());
            for (size_t i = 0; i < ps.sets.size(); i++) sig[i] = ps.sets[i].has(b);
            std::map<std::vector<bool>, uint32_t>::iterator it = seen.find(sig);
            if (it == seen.end()) { rep[nc] = (uint8_t)b; it = seen.insert(std::make_pair(sig, nc++)).first; }
            classOf[b] = (uint8_t)it->second;
        }
    }
    // the DFA behind the begin symbol, over the byte classes; acc: the end symbol accepts
    ZsReSubsets sub(nfa);
    std::vector<int> cur, nxt;
    std::map<std::vector<int>, uint32_t> ids;
    std::vector<std::vector<int> > members;
    std::vector<uint32_t> table;                                           // [state * nc + class]
    std::vector<uint8_t> acc;
    sub.close(std::vector<int>(1, s0), cur);
    sub.step(cur, ps.sets, -1, kZsNfaBegin, nxt);
    ids[nxt] = 0; members.push_back(nxt);
    uint64_t work = 0;                                                     // NFA-state entries stepped from and to: the header's time bound
    for (size_t s = 0; s < members.size(); s++) {
        if (members.size() > 4096u || work > 200000000ull) return ZSMI_error_parameter_outOfBound;
        cur = members[s];                                                  // (a copy: members grows)
        sub.step(cur, ps.sets, -1, kZsNfaEnd, nxt);
        acc.push_back(std::binary_search(nxt.begin(), nxt.end(), fin) ? 1 : 0);
        for (uint32_t c = 0; c < nc; c++) {
            sub.step(cur, ps.sets, rep[c], 0, nxt);
            work += cur.size() + nxt.size() + 1;
            std::map<std::vector<int>, uint32_t>::iterator it = ids.find(nxt);
            if (it == ids.end()) { it = ids.insert(std::make_pair(nxt, (uint32_t)members.size())).first; members.push_back(nxt); }
            table.push_back(it->second);
        }
    }
    // Moore: states in one block until a byte class tells them apart.  Blocks only split, so above 64 of them the program is above the cap
    const size_t n = members.size();
    std::vector<uint32_t> block(n), next(n);
    uint32_t blocks = 0;
    {
        bool any[2] = { false, false };
        for (size_t s = 0; s < n; s++) any[acc[s]] = true;
        for (size_t s = 0; s < n; s++) block[s] = any[0] && any[1] ? acc[s] : 0u;
        blocks = any[0] && any[1] ? 2u : 1u;
    }
    for (;;) {
        std::map<std::vector<uint32_t>, uint32_t> sigs;
        std::vector<uint32_t> sig(nc + 1);
        for (size_t s = 0; s < n; s++) {
            sig[0] = block[s];
            for (uint32_t c = 0; c < nc; c++) sig[c + 1] = block[table[s * nc + c]];
            std::map<std::vector<uint32_t>, uint32_t>::iterator it = sigs.find(sig);
            if (it == sigs.end()) { const uint32_t id = (uint32_t)sigs.size(); it = sigs.insert(std::make_pair(sig, id)).first; }
            next[s] = it->second;
        }
        const uint32_t now = (uint32_t)sigs.size();
        block.swap(next);
        if (now > ZSMI_REGEX_MAX_STATES) return ZSMI_error_parameter_outOfBound;
        if (now == blocks) break;
        blocks = now;
    }
    if (blocks * nc > ZSMI_REGEX_MAX_TABLE) return ZSMI_error_parameter_outOfBound;
    // number the blocks breadth first from the start state's, classes ascending
    std::vector<int> number(blocks, -1), member(blocks, -1);
    std::vector<uint32_t> order;
    for (size_t s = 0; s < n; s++) if (member[block[s]] < 0) member[block[s]] = (int)s;
    number[block[0]] = 0; order.push_back(block[0]);
    for (size_t i = 0; i < order.size(); i++)
        for (uint32_t c = 0; c < nc; c++) {
            const uint32_t to = block[table[(size_t)member[order[i]] * nc + c]];
            if (number[to] < 0) { number[to] = (int)order.size(); order.push_back(to); }
        }
    memset(prog, 0, sizeof *prog);
    prog->nStates = (uint32_t)order.size(); prog->nClasses = nc; prog->start = 0; prog->flags = flags;
    memcpy(prog->classOf, classOf, 256);
    for (size_t i = 0; i < order.size(); i++) {
        const size_t s = (size_t)member[order[i]];
        if (acc[s]) prog->accept |= 1ull << i;
        for (uint32_t c = 0; c < nc; c++) prog->next[i * nc + c] = (uint8_t)number[block[table[s * nc + c]]];
    }
    where = 0;
    return 0;
}
