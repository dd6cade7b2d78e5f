"""Find records by content: the rule of include/zsmi.h restated in plain Python (test infrastructure) over bytes.find and bytes.count,
never through the library.  The yardstick of zsmi_findRecords (tests/test_find_records_host.py), of zsmi_findRecordsDevice
(tests/test_gpu_find_records.py) and of the archive calls (tests/test_gpu_find_archive.py) alike, with the inputs they are held against
it on."""
import ctypes
import numpy as np
import _split as S

E_GENERIC, E_CORRUPT, E_CHECKSUM, E_UNSUPPORTED, E_PARAM, E_INIT, E_TOO_SMALL, E_SRC_SIZE = 1, 20, 22, 40, 42, 62, 70, 72
NAMES = ("zsmi_findRecords", "zsmi_findRecordsDevice", "zsmi_seekableFindWorkBound", "zsmi_seekableFindRecordsResident", "zsmi_seekableFindRecordsHost")
LANE, STEP, TILE = 16, 4096, 16384                                     # the borders of the kernels' tile shape
SIZES = (1, 2, 5, 16, 17, 256)                                         # pattern lengths: below, at and above a lane's 16 bytes, the longest


def find(data, pattern, delim=10, base=0):
    """(records, matches): the distinct records that hold an occurrence, ascending, and the occurrences, overlapping ones included"""
    assert 1 <= len(pattern) <= 256 and delim not in pattern
    d = bytes([delim])
    records, matches, at, seen, counted = [], 0, 0, 0, 0               # seen: the delimiters in data[0, counted)
    while True:
        p = data.find(pattern, at)
        if p < 0:
            return records, matches
        seen += data.count(d, counted, p); counted = p
        if not records or records[-1] != base + seen:
            records.append(base + seen)
        matches += 1; at = p + 1


def pattern_of(m, delim=10):
    """m seeded bytes that are neither the delimiter nor the filler b'a' nor equal to their neighbours' start: no occurrence overlaps another"""
    rng = np.random.default_rng(100 + m)
    body = rng.integers(0x30, 0x5B, m, dtype=np.uint8)                 # '0' .. 'Z'
    body[0] = 0x21                                                     # '!' occurs nowhere else in the pattern: it cannot overlap itself
    out = body.tobytes()
    assert delim not in out and b"a" not in out and out.count(b"!") == 1
    return out


def place(size, pattern, starts, delims=(), fill=b"a"):
    """`size` filler bytes with the pattern at every start and a newline at every position of `delims`"""
    b = bytearray(fill * size)
    for p in delims:
        b[p] = 10
    for p in starts:
        assert 0 <= p and p + len(pattern) <= size
        b[p:p + len(pattern)] = pattern
    return bytes(b)


def inputs():
    """name -> (data, pattern, delim, base): what the host call and the sanitizer program are held against the rule on, besides the
    texts of tests/_split.py"""
    c = {}
    c["empty"] = (b"", b"x", 10, 0)
    c["longer_than_text"] = (b"abc", b"abcd", 10, 0)
    c["exactly_the_text"] = (b"abcd", b"abcd", 10, 7)
    c["overlaps"] = (b"aaaa", b"aa", 10, 0)
    c["overlaps_in_lines"] = (b"aaaa\naa\na\naaa", b"aa", 10, 3)
    c["ends_at_the_end"] = (b"x\nyy\nneedle", b"needle", 10, 0)
    c["false_tail"] = (b"x\nyy\nneedl", b"needle", 10, 0)
    c["every_line"] = (b"ab\n" * 50, b"ab", 10, 1 << 40)
    c["delim_0"] = (b"one\0two\0three\0two", b"two", 0, 0)
    c["delim_255"] = (b"one\xfftwo\xffthree\xfftwo\xff", b"t", 255, 5)
    c["pattern_has_zero"] = (b"a\0b\na\0b\0\n\0b", b"\0b", 10, 0)
    c["one_byte_256"] = (b"q" * 600 + b"\n" + b"q" * 255 + b"\n" + b"q" * 256, b"q" * 256, 10, 0)
    text = S.text_lines(6000, seed=9)
    c["lines_common"] = (text, b"e", 10, 0)
    c["lines_rare"] = (text, text[3000:3007].replace(b"\n", b"x"), 10, 2)
    return c


def split_inputs():
    """the texts of tests/_split.py's cases() with a pattern cut from each (its first byte that is no delimiter, and two bytes where the
    text has them): name -> (data, pattern, delim, base)"""
    c = {}
    for name, (data, delim, T, M) in S.cases().items():
        body = bytes(b for b in data if b != delim)
        c[name] = (data, body[:1] or b"x", delim, 0)
        pair = next((data[i:i + 2] for i in range(len(data) - 1) if delim not in data[i:i + 2]), None)
        if pair:
            c[name + "_pair"] = (data, pair, delim, 11)
    return c


def code(L, r):
    return int(L.zsmi_getErrorCode(r)) if L.zsmi_isError(r) else 0


def host(L, data, pattern, delim=10, base=0, capacity=None, sentinel=0xA5A5A5A5A5A5A5A5):
    """zsmi_findRecords into an array of exactly `capacity` entries (default: the count-only call's answer) with a sentinel behind it:
    (total or -code, the numbers written, matches, whether the sentinel is intact)"""
    matches = ctypes.c_uint64(0xDEAD)
    if capacity is None:
        capacity = L.zsmi_findRecords(data, len(data), delim, pattern, len(pattern), base, None, 0, None)
        assert not L.zsmi_isError(capacity), code(L, capacity)
    out = np.full(capacity + 1, sentinel, dtype=np.uint64)
    r = L.zsmi_findRecords(data, len(data), delim, pattern, len(pattern), base, out.ctypes.data_as(ctypes.c_void_p), capacity, ctypes.byref(matches))
    intact = int(out[capacity]) == sentinel
    if L.zsmi_isError(r):
        return -code(L, r), out[:capacity].tolist(), matches.value, intact
    return int(r), out[:min(int(r), capacity)].tolist(), matches.value, intact


# ---- windows of an archive (tests/test_gpu_find_archive.py) ----
def record_starts(first_record):
    """the frames that begin a record: f == 0 or first_record[f] != first_record[f - 1] (first_record: n + 1 entries)"""
    n = len(first_record) - 1
    return [f for f in range(n) if f == 0 or first_record[f] != first_record[f - 1]]


def window(data, sizes, first_record, a, b, pattern, delim):
    """the rule on the content of frames [a, b) with B = first_record[a]"""
    at = [0] + np.cumsum(sizes, dtype=np.int64).tolist()
    return find(data[at[a]:at[b]], pattern, delim, first_record[a] if a < len(first_record) else 0)


# ---- the device call on plain text (tests/test_gpu_find_records.py) ----
class Device:
    """what one zsmi_findRecordsDevice call left: rc, result (four words), records (the whole array, a list), untouched (dRecords and
    dResult still hold their canary fill)"""


def device(L, H, codec, data, pattern, delim=10, base=None, capacity=None, offset=0, behind=b"", null_records=False):
    """the call with dRecords exactly `capacity` entries (default: the rule's total) and dResult four words, canaries on both sides of
    each (tests/_hip.py), checked here; the source `offset` bytes into its buffer, with `behind` in the allocation behind srcSize.
    base: None for a NULL dBase, else the value of the device word.  The test synchronises before it reads anything back."""
    from _hip import Dev, CANARY
    from _resident import down, up
    p = ctypes.c_void_p
    want, _ = find(data, pattern, delim, base or 0)
    cap = len(want) if capacity is None else capacity
    src = Dev(H, max(offset + len(data) + len(behind), 1), bytes(offset) + data + behind)
    rec, res = Dev(H, max(8 * cap, 1)), Dev(H, 32)
    word = up(H, np.asarray([base], dtype=np.uint64)) if base is not None else None
    d = Device()
    try:
        d.rc = L.zsmi_findRecordsDevice(codec.ctx, p(src.p + offset), len(data), delim, pattern, len(pattern), p(word.p) if word else None,
                                        None if null_records else p(rec.p), cap, p(res.p))
        codec.sync()
        vals = []
        for name, dev, t in (("dResult", res, np.uint64), ("dRecords", rec, np.uint64), ("the source", src, np.uint8)) + ((("dBase", word, np.uint64),) if word else ()):
            v, ok = down(dev, t)
            assert ok, "a guard word in front of or behind " + name + " is gone"
            vals.append(v.copy())
        assert vals[2].tobytes()[:offset + len(data) + len(behind)] == bytes(offset) + data + behind, "the source changed"
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


def same_as_rule(d, data, pattern, delim=10, base=0, capacity=None, what=""):
    """a call that was not refused against the rule: dResult, the ascending prefix, and the canary fill behind it"""
    records, matches = find(data, pattern, delim, base)
    cap = len(records) if capacity is None else capacity
    written = min(len(records), cap)
    assert d.rc == 0, (what, d.rc)
    assert d.result == [len(records), written, matches, len(data)], (what, d.result, [len(records), written, matches, len(data)])
    assert d.records[:written] == records[:written], (what, [(i, a, b) for i, (a, b) in enumerate(zip(d.records, records)) if a != b][:8])
    assert all(v == 0xA5A5A5A5A5A5A5A5 for v in d.records[written:]), (what, "written behind the numbers")


def boundary_windows(data, sizes, first_record, pattern, delim):
    """the windows cut at the frames that begin a record, [(a, b)], after checking on the CPU that together they find what the whole
    window finds: the same numbers in the same order, the same occurrences"""
    n = len(sizes)
    starts = record_starts(first_record) + [n]
    cuts = [(a, b) for a, b in zip(starts, starts[1:])]
    records, matches = [], 0
    for a, b in cuts:
        r, m = window(data, sizes, first_record, a, b, pattern, delim)
        records += r; matches += m
    assert (records, matches) == find(data, pattern, delim, 0), "windows cut where records begin lose or double an occurrence"
    return cuts
