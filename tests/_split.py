"""The record splitter's rule restated in plain Python (test infrastructure): rules 1 - 4 of include/zsmi.h over bytes.find, never through
the library.  The yardstick of zsmi_splitRecords (tests/test_split_records_host.py) and of zsmi_splitRecordsDevice
(tests/test_gpu_split_records.py) alike, with the inputs both are held against it on and the one way both call the host form."""
import bisect, ctypes
import numpy as np

E_GENERIC, E_PARAM, E_INIT, E_TOO_SMALL, E_SRC_SIZE = 1, 42, 62, 70, 72
NAMES = ("zsmi_splitRecords", "zsmi_countRecordsDevice", "zsmi_splitRecordsDevice")


def record_ends(data, delim):
    """rule 1: (the end behind every delimiter, the same with len(data) appended for a tail without one)"""
    d = bytes([delim])
    ends, at = [], 0
    while True:
        k = data.find(d, at)
        if k < 0:
            break
        ends.append(k + 1); at = k + 1
    return ends, ends + ([len(data)] if at < len(data) else [])


def piece_ends(ends, M):
    """rule 2: a record longer than M is cut at multiples of M from its own start"""
    pieces, start = [], 0
    for e in ends:
        pieces.extend(range(start + M, e, M))
        pieces.append(e); start = e
    return pieces


class Split:
    """sizes, first_record (n + 1 entries), records, pieces"""

    def __init__(self, data, delim=10, T=0, M=1 << 16):
        delims, ends = record_ends(data, delim)
        pieces = piece_ends(ends, M)
        self.records, self.pieces = len(ends), len(pieces)
        self.sizes, starts, pos, k = [], [], 0, 0                     # k: the first piece end behind pos
        while pos < len(data):                                        # rule 3
            j = k
            if T > 0:
                j = max(bisect.bisect_right(pieces, pos + T) - 1, k)  # the last piece end in (pos, pos + T], else the first behind pos
            starts.append(pos); self.sizes.append(pieces[j] - pos)
            pos, k = pieces[j], j + 1
        self.first_record = [bisect.bisect_right(delims, s) for s in starts] + [self.records]      # rule 4: the delimiters in front of a start
        assert sum(self.sizes) == len(data) and all(0 < s <= M for s in self.sizes)

    @property
    def n(self):
        return len(self.sizes)

    def frame_of(self, r):
        """rule 4's lookup: the frame record r starts in"""
        i = bisect.bisect_left(self.first_record, r)
        return i if self.first_record[i] == r else i - 1


def lines(seed, n=200, hi=300, delim=10):
    """n seeded records of 0 .. hi bytes that hold no delimiter, each with one behind it"""
    rng = np.random.default_rng(seed)
    out = []
    for length in rng.integers(0, hi + 1, n):
        body = rng.integers(0, 255, int(length), dtype=np.uint8)
        body[body == delim] = (delim + 1) % 255
        out.append(body.tobytes() + bytes([delim]))
    return b"".join(out)


def cases():
    """name -> (data, delim, T, M): the inputs the issue lists"""
    c = {}
    c["empty"] = (b"", 10, 0, 1 << 16)
    c["one_delimiter"] = (b"\n", 10, 0, 1 << 16)
    c["one_other_byte"] = (b"x", 10, 0, 1 << 16)
    c["all_delimiters_5000"] = (b"\n" * 5000, 10, 0, 1 << 16)
    c["all_delimiters_5000_T7"] = (b"\n" * 5000, 10, 7, 1 << 16)
    for size in (2500, 3000, 3001):
        c["no_delimiter_%d" % size] = (b"a" * size, 10, 0, 1000)
        c["no_delimiter_%d_T1000" % size] = (b"a" * size, 10, 1000, 1000)
    c["tail_without_delimiter"] = (b"ab\ncd\nef", 10, 0, 1 << 16)
    c["tail_with_delimiter"] = (b"ab\ncd\nef\n", 10, 0, 1 << 16)
    text = lines(3, 60, 40)
    c["T0"] = (text, 10, 0, 64)
    c["T1"] = (text, 10, 1, 64)
    c["T_is_M"] = (text, 10, 64, 64)
    c["long_piece_between_short"] = (b"a\nbb\n" + b"c" * 40 + b"\nd\nee\n", 10, 8, 100)
    # a record of 2 M + 5 bytes: two cut pieces, and a last piece of 5 that shares its frame with the records behind it
    c["cut_record_shares_its_last_piece"] = (b"x\n" + b"y" * 24 + b"\nz\nw\n" + b"tail", 10, 10, 10)
    for T in (64, 1000, 4096):
        c["random_T%d" % T] = (lines(11 + T), 10, T, 4096)
        c["random_T%d_M256" % T] = (lines(12 + T), 10, min(T, 256), 256)
    c["delim_0"] = (lines(5, 80, 50, delim=0), 0, 100, 1 << 16)
    c["delim_255"] = (lines(6, 80, 50, delim=255), 255, 100, 1 << 16)
    return c


def code(L, r):
    return int(L.zsmi_getErrorCode(r)) if L.zsmi_isError(r) else 0


def host(L, data, delim=10, T=0, M=1 << 16, capacity=None, sentinel=0xA5A5A5A5):
    """zsmi_splitRecords into arrays of exactly `capacity` (default: the count-only call's answer) and capacity + 1 entries, one sentinel
    behind each: (n or -code, sizes, first_record, records, whether both sentinels are intact)"""
    records = ctypes.c_uint64(0xDEAD)
    if capacity is None:
        capacity = L.zsmi_splitRecords(data, len(data), delim, T, M, None, None, 0, None)
        assert not L.zsmi_isError(capacity), code(L, capacity)
    sizes = np.full(capacity + 1, sentinel, dtype=np.uint32)
    first = np.full(capacity + 2, sentinel, dtype=np.uint64)
    r = L.zsmi_splitRecords(data, len(data), delim, T, M, sizes.ctypes.data_as(ctypes.c_void_p), first.ctypes.data_as(ctypes.c_void_p), capacity, ctypes.byref(records))
    intact = int(sizes[capacity]) == sentinel and int(first[capacity + 1]) == sentinel
    if L.zsmi_isError(r):
        return -code(L, r), sizes[:capacity], first[:capacity + 1], records.value, intact
    return int(r), sizes[:r].tolist(), first[:r + 1].tolist(), records.value, intact


# ---- the device call (tests/test_gpu_split_records.py) ----
def border_buffer(size, last):
    """`size` bytes of 'a' with a delimiter on the first byte, on the last byte of a lane's 16 and the first of the next lane's, on either
    side of every 4096-byte step (so of every 16384-byte tile border too), and - with `last` - on the very last byte"""
    b = bytearray(b"a" * size)
    at = {0, 15, 16, 31, 32}
    for k in range(4096, size + 4096, 4096):
        at |= {k - 1, k}
    for p in at:
        if p < size:
            b[p] = 10
    if size:
        b[size - 1] = 10 if last else 98
    return bytes(b)


def text_lines(size, seed=21):
    """about `size` bytes of seeded lower-case lines of 20 .. 200 bytes, each ended by a newline"""
    rng = np.random.default_rng(seed)
    out, total = [], 0
    while total < size:
        line = bytes(rng.integers(97, 123, int(rng.integers(20, 201)), dtype=np.uint8)) + b"\n"
        out.append(line); total += len(line)
    return b"".join(out)


class Device:
    """what one zsmi_splitRecordsDevice call left: rc, result (three words), sizes and first (the whole arrays, as lists)"""


def device(L, H, codec, data, delim=10, T=0, M=1 << 16, max_pieces=None, want_first=True, offset=0):
    """the call with every array exactly as long as the header sizes it, canaries on both sides of each (tests/_hip.py), checked here.
    offset > 0: the source is a slice at that byte offset of a larger device buffer whose every other byte is the delimiter.  The count
    call runs on the same source first and must give the records.  The test synchronises before it reads anything back."""
    from _hip import Dev, CANARY
    from _resident import down
    p = ctypes.c_void_p
    want = Split(data, delim, T, M)
    mp = want.pieces if max_pieces is None else max_pieces
    around = bytes([delim])
    src = Dev(H, max(len(data), 1) + (offset + 64 if offset else 0), (around * offset + data + around * 64) if offset else data)
    fs, fr, res, cnt = Dev(H, max(4 * mp, 1)), Dev(H, 8 * (mp + 1)), Dev(H, 24), Dev(H, 8)
    d = Device()
    try:
        assert L.zsmi_countRecordsDevice(codec.ctx, p(src.p + offset), len(data), delim, p(cnt.p)) == 0
        d.rc = L.zsmi_splitRecordsDevice(codec.ctx, p(src.p + offset), len(data), delim, T, M, mp, p(fs.p), p(fr.p) if want_first else None, p(res.p))
        codec.sync()
        counted, ok = down(cnt, np.uint64)
        assert ok and int(counted[0]) == want.records, ("zsmi_countRecordsDevice", int(counted[0]), want.records)
        vals = []
        for name, dev, t in (("dResult", res, np.uint64), ("dFrameSizes", fs, np.uint32), ("dFirstRecord", fr, np.uint64), ("the source", src, np.uint8)):
            v, ok = down(dev, t)
            assert ok, "a guard word in front of or behind " + name + " is gone"
            vals.append(v.copy())
        d.result = [int(v) for v in vals[0]]
        d.sizes, d.first = vals[1], vals[2]
        if mp == 0:
            assert (vals[1].view(np.uint8) == CANARY).all()
        if not want_first:
            assert (vals[2].view(np.uint8) == CANARY).all(), "wrote through a NULL dFirstRecord's stand-in"
        d.untouched = bool((vals[1].view(np.uint8) == CANARY).all() and (vals[2].view(np.uint8) == CANARY).all())
        return d, want
    finally:
        for dev in (src, fs, fr, res, cnt):
            dev.free()


def same_as_host(L, d, want, data, delim, T, M, want_first=True):
    """a fitting device call against the host call (and both against the restatement): n, sizes, firstRecord[0, n], records, pieces"""
    n, sizes, first, records, _ = host(L, data, delim, T, M)
    assert (n, sizes, first, records) == (want.n, want.sizes, want.first_record, want.records)
    assert d.rc == 0 and d.result == [n, records, want.pieces], (d.rc, d.result, [n, records, want.pieces])
    assert d.sizes[:n].tolist() == sizes
    if want_first:
        assert d.first[:n + 1].tolist() == first
