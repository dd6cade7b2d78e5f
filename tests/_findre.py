"""Find records by regular expression: the rule of include/zsmi.h restated in plain Python (test infrastructure) over `re` - split at the
delimiter, re.search a record, invert, base - never through the library.  The yardstick of zsmi_compileRegex and zsmi_findRecordsRegex
(tests/test_find_regex_host.py), of zsmi_findRecordsRegexDevice (tests/test_gpu_find_regex.py) and of the archive calls
(tests/test_gpu_find_regex_archive.py) alike, with the catalogue of patterns and the seeded generator they are held against it on."""
import ctypes, re, warnings
import numpy as np
import _find as F

IGNORE_CASE, INVERT = 1, 2
NAMES = ("zsmi_compileRegex", "zsmi_findRecordsRegex", "zsmi_findRecordsRegexDevice", "zsmi_seekableFindRegexResident", "zsmi_seekableFindRegexHost")
SENTINEL = 0xA5A5A5A5A5A5A5A5
TILE = F.TILE


def records_of(data, delim):
    """the splitter's records without their delimiters: one ends behind each delimiter, bytes behind the last are a last record"""
    parts = bytes(data).split(bytes([delim]))
    if parts[-1] == b"":
        parts.pop()                                                    # (nothing behind the last delimiter, or no text at all)
    return parts


def record_count(data, delim):
    return data.count(bytes([delim])) + (1 if data and data[-1] != delim else 0)


def uses_dollar(pattern):
    return b"$" in pattern


def python_regex(pattern, flags=0):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                                # ("possible nested set": a `[` inside a class is a literal here)
        return re.compile(pattern, re.DOTALL | (re.IGNORECASE if flags & IGNORE_CASE else 0))


def find(data, pattern, flags=0, delim=10, base=0):
    """(records, text records): the records re.search succeeds on - with INVERT the others - ascending from base"""
    if delim != 10 and uses_dollar(pattern):
        assert b"\n" not in data, "Python's $ also matches in front of a final newline: a text for it holds none"
    rx = python_regex(pattern, flags)
    parts = records_of(data, delim)
    assert len(parts) == record_count(data, delim)
    return [base + i for i, r in enumerate(parts) if (rx.search(r) is not None) != bool(flags & INVERT)], len(parts)


def text_for(data, pattern, delim):
    """the text a pattern with $ is tried on under a delimiter other than the newline: its newlines turned into ';'"""
    return data.replace(b"\n", b";") if delim != 10 and uses_dollar(pattern) else data


def check_rule():
    assert records_of(b"", 10) == [] and records_of(b"\n", 10) == [b""] and records_of(b"a\n\nb", 10) == [b"a", b"", b"b"]
    assert find(b"ab\n\nAB\nb", b"^a", 0, 10, 5) == ([5], 4)
    assert find(b"ab\n\nAB\nb", b"^a", IGNORE_CASE) == ([0, 2], 4)
    assert find(b"ab\n\nAB\nb", b"^a", INVERT) == ([1, 2, 3], 4)
    assert find(b"ab\n\nAB\nb\n", b"^$") == ([1], 4)
    assert find(b"a.b,a\nb,", b"a.b", 0, 44) == ([0, 1], 2)           # the dot takes the newline: it is no delimiter here


check_rule()

# ---- the catalogue: (pattern, flags), every construct the compiler accepts ----
CATALOGUE = [
    (b"e", 0), (b"ab", 0), (b"needle", 0), (b"two", 0), (b"\\.", 0), (b"\\\\|\\$|\\^", 0), (b"\\x61\\x62", 0), (b"\\x0a|\\x2C|\\x41", 0),
    (b"\\t|\\r|\\f|\\v", 0), (b"a\\nb", 0), (b"\\d", 0), (b"\\D", 0), (b"\\w+", 0), (b"\\W", 0), (b"\\s", 0), (b"\\S\\s\\S", 0),
    (b".", 0), (b"a.b", 0), (b"e.*t", 0), (b"[abc]", 0), (b"[^abc]", 0), (b"[a-e][f-z]", 0), (b"[]a]", 0), (b"[^]a]", 0), (b"[a-]", 0), (b"[-a]", 0),
    (b"[a\\-z]", 0), (b"[x[]", 0), (b"[\\d\\s]", 0), (b"[^\\w]", 0), (b"[\\x41-\\x43]", 0), (b"[\\]]", 0), (b"[+--]", 0), (b"[a-c-e]", 0),
    (b"(ab)+", 0), (b"(?:ab|cd|wo)e", 0), (b"a|b|", 0), (b"(|a)b", 0), (b"()", 0), (b"((a|b)(c|d))", 0),
    (b"ab*c", 0), (b"ab+c", 0), (b"ab?c", 0), (b"a{3}", 0), (b"a{2,}", 0), (b"a{1,3}b", 0), (b"(ab){2}", 0), (b"x{0}y", 0), (b"a{0,}", 0), (b"q{60}", 0), (b"ba{0,255}", 0),
    (b"[0-9]{1,3}(\\.[0-9]{1,3}){3}", 0), (b"^a", 0), (b"a$", 0), (b"^$", 0), (b"^a.*e$", 0), (b"^a|b$", 0), (b"^", 0), (b"$", 0), (b"^.{5}$", 0),
    (b"^\\d+$|^two", 0), (b"}|]", 0), (b"\xff", 0), (b"[\x80-\xff]", 0), (b"\\\xff", 0),
    (b"error", IGNORE_CASE), (b"[a-c]x", IGNORE_CASE), (b"[^a-c]", IGNORE_CASE), (b"[Z-a]", IGNORE_CASE), (b"@|\\[|`|\\{", IGNORE_CASE), (b"TWO", IGNORE_CASE),
    (b"^NEEDLE$", IGNORE_CASE), (b"\\W", IGNORE_CASE), (b"e", INVERT), (b"^$", INVERT), (b"A", IGNORE_CASE | INVERT),
    # unbounded repeats of a group that holds an alternative or a quantifier of its own: the loop runs over an alternation or a repeat.
    # Each body parses a text in one way only, so `re` stays linear in the record
    (b"(a|b)*c", 0), (b"(a*b)+", 0), (b"(?:ab|c)+$", 0), (b"a(b|c)*d$", 0), (b"(ab?)*c", 0), (b"^(\\w+ )*two", 0), (b"([a-c]|x{2})+,", 0),
    (b"(a|b){2,}c", 0), (b"(?:e+,){2,}", 0), (b"(e|o)+r", IGNORE_CASE), (b"(o|e)*t$", INVERT), (b"((a|b)c?,)+$", 0),
]


# ---- the seeded generator: patterns of the accepted grammar over the bytes a b \n , . A and a few classes ----
def generated(count, seed, depth=3):
    rng = np.random.default_rng(seed)
    literals = (b"a", b"b", b"\\n", b",", b"\\.", b"A", b".")
    classes = (b"[ab]", b"[^a]", b"[a-b,]", b"\\d", b"\\s", b"\\w", b"[^,\\n]", b"[A.]", b"\\W")
    quants = (b"", b"", b"", b"", b"*", b"+", b"?", b"{2}", b"{1,2}", b"{2,}")
    bounded = (b"", b"", b"?", b"{2}", b"{1,2}")

    def pick(seq):
        return seq[int(rng.integers(len(seq)))]

    # (a group takes * + {2,} only where it holds neither a quantifier nor an alternative: `re` backtracks, and nested repeats of
    # ambiguous bodies would cost it a time that is exponential in the text)
    def atom(d):
        r = rng.random()
        if d > 0 and r < 0.25:
            inner = alternatives(d - 1)
            plain = not any(c in inner for c in b"*+?{|")
            return b"(" + (b"?:" if rng.random() < 0.3 else b"") + inner + b")" + pick(quants if plain else bounded)
        return (pick(classes) if r < 0.45 else pick(literals)) + pick(quants)

    def sequence(d):
        return b"".join(atom(d) for _ in range(int(rng.integers(0 if d < depth else 1, 4))))

    def alternatives(d):
        return b"|".join(sequence(d) for _ in range(int(rng.integers(1, 3))))

    out = []
    for _ in range(count):
        tops = []
        for _ in range(int(rng.integers(1, 3))):
            tops.append((b"^" if rng.random() < 0.2 else b"") + sequence(depth) + (b"$" if rng.random() < 0.2 else b""))
        out.append((b"|".join(tops), int(rng.integers(4))))
    return out


def generated_text(rng, size):
    return bytes(np.frombuffer(b"ab\n,.Aab 1", dtype=np.uint8)[rng.integers(0, 10, size)])


# ---- the library's program ----
def compile(L, pattern, flags=0):
    """(code, program, errorAt)"""
    from zstandard_amd._lib import RegexProgram
    prog = RegexProgram()
    at = ctypes.c_size_t(0xDEAD)
    rc = L.zsmi_compileRegex(bytes(pattern), len(pattern), flags, ctypes.byref(prog), ctypes.byref(at))
    return rc, prog, at.value


def program(L, pattern, flags=0):
    rc, prog, at = compile(L, pattern, flags)
    assert rc == 0, (pattern, flags, rc, at)
    return prog


def copy_of(prog):
    from zstandard_amd._lib import RegexProgram
    out = RegexProgram()
    ctypes.memmove(ctypes.byref(out), ctypes.byref(prog), ctypes.sizeof(RegexProgram))
    return out


def damaged(L):
    """name -> a program that zs_regex_check refuses, made from a good one"""
    good = program(L, b"ab+c")
    out = {}
    p = copy_of(good); p.next[good.nStates * good.nClasses - 1] = good.nStates; out["next out of range"] = p
    p = copy_of(good); p.start = good.nStates; out["start out of range"] = p
    p = copy_of(good); p.nStates, p.nClasses = 64, 49; out["product above 3072"] = p
    p = copy_of(good); p.accept |= 1 << good.nStates; out["accept bit above nStates"] = p
    p = copy_of(good); p.classOf[200] = good.nClasses; out["class out of range"] = p
    p = copy_of(good); p.nStates = 0; out["no state"] = p
    p = copy_of(good); p.nStates = 65; p.nClasses = 1; out["65 states"] = p
    p = copy_of(good); p.flags = 4; out["unknown flag"] = p
    return out


def host(L, data, prog, delim=10, base=0, capacity=None):
    """zsmi_findRecordsRegex into an array of exactly `capacity` entries (default: the count-only call's answer) with a sentinel behind
    it: (total or -code, the numbers written, textRecords, whether the sentinel is intact)"""
    text_records = ctypes.c_uint64(0xDEAD)
    if capacity is None:
        capacity = L.zsmi_findRecordsRegex(data, len(data), delim, ctypes.byref(prog), base, None, 0, None)
        assert not L.zsmi_isError(capacity), F.code(L, capacity)
    out = np.full(capacity + 1, SENTINEL, dtype=np.uint64)
    r = L.zsmi_findRecordsRegex(data, len(data), delim, ctypes.byref(prog), base, ctypes.c_void_p(out.ctypes.data), capacity, ctypes.byref(text_records))
    intact = int(out[capacity]) == SENTINEL
    if L.zsmi_isError(r):
        return -F.code(L, r), out[:capacity].tolist(), text_records.value, intact
    return int(r), out[:min(int(r), capacity)].tolist(), text_records.value, intact


# ---- the device call on plain text (tests/test_gpu_find_regex.py) ----
class Device:
    """what one zsmi_findRecordsRegexDevice call left: rc, result (four words), records (the whole array, a list), untouched"""


def device(L, H, codec, data, prog, want_total, delim=10, base=None, capacity=None, null_records=False):
    """the call with dRecords exactly `capacity` entries (default: want_total, the rule's) and dResult four words, canaries on both sides
    of each (tests/_hip.py), checked here, and the source unchanged.  base: None for a NULL dBase, else the device word's value"""
    from _hip import Dev, CANARY
    from _resident import down, up
    p = ctypes.c_void_p
    cap = want_total if capacity is None else capacity
    src = Dev(H, max(len(data), 1), data)
    rec, res = Dev(H, max(8 * cap, 1)), Dev(H, 32)
    word = up(H, np.asarray([base], dtype=np.uint64)) if base is not None else None
    d = Device()
    try:
        d.rc = L.zsmi_findRecordsRegexDevice(codec.ctx, p(src.p), len(data), delim, ctypes.byref(prog) if prog is not None else None, p(word.p) if word else None,
                                             None if null_records else p(rec.p), cap, p(res.p))
        codec.sync()
        vals = []
        for name, dev, t in (("dResult", res, np.uint64), ("dRecords", rec, np.uint64), ("the source", src, np.uint8)) + ((("dBase", word, np.uint64),) if word else ()):
            v, ok = down(dev, t)
            assert ok, "a guard word in front of or behind " + name + " is gone"
            vals.append(v.copy())
        assert vals[2].tobytes()[:len(data)] == data, "the source changed"
        d.result = [int(v) for v in vals[0]]
        d.records = [int(v) for v in vals[1][:cap]]
        d.untouched = bool((vals[0].view(np.uint8) == CANARY).all() and (vals[1].view(np.uint8) == CANARY).all())
        if cap == 0 or null_records:
            assert (vals[1].view(np.uint8) == CANARY).all(), "wrote through dRecords with nothing to write"
        return d
    finally:
        for dev in (src, rec, res, word):
            if dev is not None:
                dev.free()


def same_as_rule(d, data, pattern, flags=0, delim=10, base=0, capacity=None, what=""):
    """a call that was not refused against the rule: dResult, the ascending prefix, and the canary fill behind it"""
    records, text_records = find(data, pattern, flags, delim, base)
    cap = len(records) if capacity is None else capacity
    written = min(len(records), cap)
    assert d.rc == 0, (what, d.rc)
    assert d.result == [len(records), written, text_records, len(data)], (what, d.result, [len(records), written, text_records, len(data)])
    assert d.records[:written] == records[:written], (what, [(i, a, b) for i, (a, b) in enumerate(zip(d.records, records)) if a != b][:8])
    assert all(v == SENTINEL for v in d.records[written:]), (what, "written behind the numbers")


def run(L, H, codec, data, pattern, flags=0, delim=10, base=None, capacity=None, null_records=False, what=""):
    """compile, search on the device, hold against the rule"""
    prog = program(L, pattern, flags)
    total = len(find(data, pattern, flags, delim, base or 0)[0])
    d = device(L, H, codec, data, prog, total, delim, base, capacity, null_records)
    same_as_rule(d, data, pattern, flags, delim, base or 0, capacity, what or (pattern, flags, delim, len(data)))
    return d


# ---- windows of an archive (tests/test_gpu_find_regex_archive.py) ----
def window(data, sizes, first_record, a, b, pattern, flags, delim):
    """the rule on the content of frames [a, b) with B = first_record[a]"""
    at = [0] + np.cumsum(sizes, dtype=np.int64).tolist()
    return find(data[at[a]:at[b]], pattern, flags, delim, int(first_record[a]) if a < len(first_record) else 0)


def boundary_windows(data, sizes, first_record, pattern, flags, delim):
    """the windows cut at the frames that begin a record, [(a, b)], after checking on the CPU that together they give the whole window's
    answer"""
    starts = F.record_starts(first_record) + [len(sizes)]
    cuts = list(zip(starts, starts[1:]))
    records, text_records = [], 0
    for a, b in cuts:
        r, n = window(data, sizes, first_record, a, b, pattern, flags, delim)
        records += r; text_records += n
    assert (records, text_records) == find(data, pattern, flags, delim, 0), "windows cut where records begin lose or double a record"
    return cuts
