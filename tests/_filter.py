"""Frame filters restated in plain Python (test infrastructure): rules 1 - 11 of include/zsmi.h, the filter frame's layout and its check -
never through the library.  The yardstick of the host calls (tests/test_frame_filter_host.py), of the device calls
(tests/test_gpu_frame_filter.py) and of the searches that use a filter (tests/test_gpu_find_frames.py)."""
import bisect, ctypes, struct
import numpy as np
import _findq as Q

MAGIC, INNER, VERSION, FIXED = 0x184D2A5C, 0x52544C46, 1, 40
C0, C1 = 0x9E3779B1, 0x85EBCA77
K1, K2 = 0x9E3779B185EBCA87, 0xC2B2AE3D27D4EB4F
M32, M64 = (1 << 32) - 1, (1 << 64) - 1
E_GENERIC, E_PREFIX, E_VERSION, E_CORRUPT, E_UNSUPPORTED, E_PARAM, E_INIT, E_TOO_SMALL, E_SRC_SIZE, E_FRAME_INDEX = 1, 10, 12, 20, 40, 42, 62, 70, 72, 100
TILE = 16384
NAMES = ("zsmi_frameFilterSize", "zsmi_buildFrameFilter", "zsmi_readFrameFilter", "zsmi_filterFrames", "zsmi_buildFrameFilterDevice",
         "zsmi_seekableBuildFrameFilterResident", "zsmi_seekableBuildFrameFilterHost", "zsmi_checkFrameFilterDevice", "zsmi_filterFramesDevice",
         "zsmi_seekableFindFramesWorkBound", "zsmi_seekableFindQueryFramesResident", "zsmi_seekableFindQueryFramesHost")


def fold(b):
    """rule 1: 'A' .. 'Z' and nothing else"""
    return bytes(c + 0x20 if 0x41 <= c <= 0x5A else c for c in bytes(b))


def bits_of(gram, L):
    """rules 3 and 4: the two bits of a gram's folded bytes"""
    v = int.from_bytes(fold(gram), "little")
    return [((v * c) & M32) >> (32 - L) for c in (C0, C1)]


def offsets_of(sizes):
    return [0] + np.cumsum(np.asarray(sizes, dtype=np.int64)).tolist() if len(sizes) else [0]


def clean(data, x, delim):
    """rule 5"""
    return x == 0 or x == len(data) or data[x - 1] == delim


def saturated_frames(data, sizes, delim):
    """rule 6: the non-empty frames with a border that is not clean"""
    at = offsets_of(sizes)
    return [i for i in range(len(sizes)) if at[i + 1] > at[i] and not (clean(data, at[i], delim) and clean(data, at[i + 1], delim))]


def slots_of(data, sizes, delim, g, L):
    """rules 2 - 7: ([a frame's slot as an int of 2^L bits], the grams hashed).  A frame at a time, its positions all at once (numpy):
    the value of the g folded bytes at p, whether any of them is the delimiter, the two bits"""
    at, sat = offsets_of(sizes), set(saturated_frames(data, sizes, delim))
    raw = np.frombuffer(bytes(data), dtype=np.uint8)
    folded = np.where((raw >= 0x41) & (raw <= 0x5A), raw + 0x20, raw).astype(np.uint64)
    slots, hashed = [], 0
    for i in range(len(sizes)):
        if i in sat:
            slots.append((1 << (1 << L)) - 1)
            continue
        a, count = at[i], at[i + 1] - at[i] - g + 1                      # the grams start at a .. a + count - 1
        bits = np.zeros(1 << L, dtype=np.uint8)
        if count > 0:
            v = np.zeros(count, dtype=np.uint64)
            holds = np.zeros(count, dtype=bool)
            for k in range(g):
                v |= folded[a + k:a + k + count] << np.uint64(8 * k)
                holds |= raw[a + k:a + k + count] == delim
            v = v[~holds]
            hashed += len(v)
            for c in (C0, C1):
                bits[((v * np.uint64(c)) & np.uint64(M32)) >> np.uint64(32 - L)] = 1
        slots.append(int.from_bytes(np.packbits(bits, bitorder="little").tobytes(), "little"))
    return slots, hashed


def check_of(words, size, delim, g, L):
    total = (size * K2 + delim + (g << 8) + (L << 16)) & M64
    for k, w in enumerate(words):
        total = (total + (int(w) + 1) * (2 * k + 1) * K1) & M64
    return total


def frame(data, sizes, delim=10, g=4, L=13, slots=None):
    """the filter frame: bit h of a slot is bit h & 7 of its byte h >> 3 - the slot's int, little-endian.  slots: slots_of's, when at hand"""
    slots = slots_of(data, sizes, delim, g, L)[0] if slots is None else slots
    body = b"".join(s.to_bytes(1 << (L - 3), "little") for s in slots)
    words = struct.unpack("<%dQ" % (len(body) // 8), body)
    return struct.pack("<IIIBBBBIIQQ", MAGIC, 32 + len(body), INNER, VERSION, delim, g, L, len(sizes), 0, len(data), check_of(words, len(data), delim, g, L)) + body


def parse(buf):
    """the fields of a frame that holds, asserted one by one: {n, delim, g, L, size, slots (ints), saturated}"""
    magic, frame_size, inner, version, delim, g, L, n, r32, size, check = struct.unpack_from("<IIIBBBBIIQQ", buf)
    assert (magic, inner, version, r32) == (MAGIC, INNER, VERSION, 0) and g in (3, 4) and 9 <= L <= 16
    sb = 1 << (L - 3)
    assert frame_size == 32 + n * sb and len(buf) == FIXED + n * sb
    words = struct.unpack_from("<%dQ" % (n * sb // 8), buf, FIXED)
    assert check == check_of(words, size, delim, g, L)
    slots = [int.from_bytes(buf[FIXED + i * sb:FIXED + (i + 1) * sb], "little") for i in range(n)]
    return {"n": n, "delim": delim, "g": g, "L": L, "size": size, "slots": slots, "saturated": sum(1 for s in slots if s == (1 << (1 << L)) - 1)}


def pattern_passes(slot, pattern, g, L):
    """rules 8 and 9"""
    if len(pattern) < g:
        return True
    return all(slot >> h & 1 for p in range(len(pattern) - g + 1) for h in bits_of(pattern[p:p + g], L))


def filter_frames(buf, patterns, mode=Q.ANY, first=0, count=None):
    """rule 10 over the frames [first, first + count) of a frame that holds: (the passing frames, ascending; the all-ones slots among them)"""
    f = parse(buf)
    count = f["n"] - first if count is None else count
    full = (1 << (1 << f["L"])) - 1
    out = []
    for i in range(first, first + count):
        verdicts = [pattern_passes(f["slots"][i], p, f["g"], f["L"]) for p in patterns]
        if mode == Q.NONE or (any(verdicts) if mode == Q.ANY else all(verdicts)):
            out.append(i)
    return out, sum(1 for i in out if f["slots"][i] == full)


def record_ends(data, delim):
    """the splitter's rule 1: the end behind every delimiter, and len(data) for a tail without one"""
    ends = (np.flatnonzero(np.frombuffer(bytes(data), dtype=np.uint8) == delim) + 1).tolist()
    return ends + ([len(data)] if data and data[-1] != delim else [])


def frames_of_records(data, sizes, records, delim, ends=None):
    """the frames that hold any part of the records numbered `records` (from 0), ascending.  ends: record_ends(data, delim), when at hand"""
    ends = record_ends(data, delim) if ends is None else ends
    at = offsets_of(sizes)
    out = set()
    for r in records:
        a, b = (ends[r - 1] if r else 0), ends[r]                        # the record's bytes [a, b): frame i holds some when at[i] < b and at[i + 1] > a
        for i in range(max(bisect.bisect_right(at, a) - 1, 0), len(sizes)):
            if at[i] >= b:
                break
            if at[i + 1] > a:
                out.add(i)
    return sorted(out)


def runs_of(frames, sizes):
    """the runs [(first, count)] of an ascending frame list: frames that follow one another, and frames with only empty frames between"""
    at, runs = offsets_of(sizes), []
    for f in frames:
        if runs and (f == runs[-1][0] + runs[-1][1] or at[f] == at[runs[-1][0] + runs[-1][1]]):
            runs[-1][1] = f + 1 - runs[-1][0]
        else:
            runs.append([f, 1])
    return [tuple(r) for r in runs]


# ---- layouts the tests share ----
def tokens(size, seed, delim=10, every=48, upper=0.0):
    """about `size` bytes of seeded lower-case tokens (3 .. 9 letters, a space between), a delimiter about every `every` bytes and one
    at the end; upper: the share of letters in upper case"""
    rng = np.random.default_rng(seed)
    out = bytearray()
    while len(out) < size:
        word = rng.integers(97, 123, int(rng.integers(3, 10)), dtype=np.uint8)
        word[rng.random(len(word)) < upper] -= 32
        out += word.tobytes()
        out += bytes([delim]) if rng.random() < 6.0 / every else b" "
    out[-1] = delim
    return bytes(out)


def fixed(size, step):
    return [step] * (size // step) + ([size % step] if size % step else [])


NEEDLE, NEEDLE_HOME, NEEDLE_SEED = b"qzjxvkqwzjpx", 37, 2


def needle_text():
    """the fixture that keeps the filter honest: (text, frame sizes) - about 64 frames of about 4 KiB of seeded lower-case tokens, NEEDLE
    in one record of frame NEEDLE_HOME.  NEEDLE_SEED was chosen on the CPU with this file alone, among seeds 1 .. 7, as one where the
    statement's list for g = 4, L = 13 holds a false positive besides the needle's frame ([37, 57]) and still no more than 3 others"""
    import _split as S
    text = bytearray(tokens(64 * 4096, NEEDLE_SEED))
    sizes = S.Split(bytes(text), 10, 4096, 1 << 16).sizes
    at = offsets_of(sizes)
    frame_bytes = bytes(text[at[NEEDLE_HOME]:at[NEEDLE_HOME + 1]])
    record = max(frame_bytes.split(b"\n"), key=len)
    assert len(record) >= len(NEEDLE) and NEEDLE not in text
    where = at[NEEDLE_HOME] + frame_bytes.index(record)
    text[where:where + len(NEEDLE)] = NEEDLE
    return bytes(text), sizes


def cases():
    """name -> (data, delim, frame sizes): layouts that reach each rule"""
    import _split as S
    c = {}
    text = tokens(6000, 1)
    c["split_T400"] = (text, 10, S.Split(text, 10, 400, 1 << 16).sizes)
    c["split_T64_M64_cut_records"] = (text, 10, S.Split(text, 10, 64, 64).sizes)
    c["fixed_100_over_text"] = (text, 10, fixed(len(text), 100))
    mixed = tokens(3000, 2, upper=0.4) + bytes(range(0x80, 0x100)) + b"\xC1\xDA\xE1\n"
    c["upper_case_and_high_bytes"] = (mixed, 10, S.Split(mixed, 10, 500, 1 << 16).sizes)
    c["gram_with_delimiter_and_border"] = (b"abcdefgh\nij\nklmnop\n" + b"qrstuvwx\n", 10, [9, 10, 9])      # "gh\ni": not hashed; "p\nqr" straddles frames 1 | 2
    c["empty_frames"] = (b"abcdef\nghijkl\n", 10, [0, 7, 0, 0, 7, 0])
    c["unclean_left_only"] = (b"abcdefgh\nijklmnop\n", 10, [4, 5, 9])               # frame 1 starts inside a record and ends on a delimiter
    c["unclean_right_only"] = (b"abcdefgh\nijklmnop\n", 10, [9, 4, 5])
    c["unclean_both"] = (b"abcdefghijklmnop\n", 10, [4, 8, 5])
    c["tail_without_delimiter"] = (b"abcdef\nghijklm", 10, [7, 7])                  # the last border is the content's end: clean
    c["frame_shorter_than_g"] = (b"ab\ncdefgh\n", 10, [3, 7])
    c["no_frames"] = (b"", 10, [])
    c["only_empty_frames"] = (b"", 10, [0, 0])
    z = tokens(2000, 3, delim=0)
    c["delim_0"] = (z, 0, S.Split(z, 0, 256, 1 << 16).sizes)
    a = tokens(2000, 4, delim=ord("A"))
    c["delim_A_and_lower_a"] = (a, ord("A"), S.Split(a, ord("A"), 256, 1 << 16).sizes)   # 'a' is text, hashed; 'A' ends a record
    return c


def queries(data, delim, rng):
    """seeded (patterns, mode, flags) for a text: pieces cut from it, pieces that are absent, short ones, mixed case"""
    pool = [p for p in Q.pattern_sets(data, delim)]
    out = []
    for pats in pool:
        pats = [p for p in pats if p][:8]
        if not pats or sum(len(p) for p in pats) > 256:
            continue
        for mode in (Q.ANY, Q.ALL):
            out.append((pats, mode, 0))
            out.append(([p.swapcase() for p in pats], mode, Q.IGNORE_CASE))
    bad = set(bytes([delim]).lower() + bytes([delim]).upper())
    absent = bytes(b for b in b"zqxjkvwzqy" if b not in bad)
    out.append(([absent], Q.ANY, 0))
    if len(data) > 40:
        at = int(rng.integers(0, len(data) - 12))
        piece = bytes(b for b in data[at:at + 12] if b not in bad and b != delim)
        if piece:
            out += [([piece], Q.ANY, 0), ([piece, absent], Q.ALL, 0), ([piece[:2]], Q.ANY, 0), ([piece, piece[:2]], Q.ALL, Q.IGNORE_CASE)]
    return out


# ---- the library's calls ----
def host_build(L, data, sizes, delim=10, g=4, Lg=13, capacity=None, sentinel=0x5A):
    """zsmi_buildFrameFilter into a buffer of exactly `capacity` bytes (default: the frame's) with sentinel bytes behind it: (size or
    -code, the bytes written, whether the sentinels are intact)"""
    n = len(sizes)
    need = FIXED + n * (1 << (Lg - 3)) if 9 <= Lg <= 16 else 0
    capacity = need if capacity is None else capacity
    out = np.full(capacity + 64, sentinel, dtype=np.uint8)
    arr = np.ascontiguousarray(sizes, dtype=np.uint32)
    p = ctypes.c_void_p
    r = L.zsmi_buildFrameFilter(p(out.ctypes.data), capacity, bytes(data), len(data), p(arr.ctypes.data) if n else None, n, delim, g, Lg)
    intact = bool((out[capacity:] == sentinel).all())
    if L.zsmi_isError(r):
        return -int(L.zsmi_getErrorCode(r)), out[:capacity].tobytes(), intact and bool((out == sentinel).all())
    return int(r), out[:int(r)].tobytes(), intact


def host_read(L, buf, size=None):
    """zsmi_readFrameFilter: the code, or the info as parse() names it"""
    from zstandard_amd._lib import FrameFilterInfo
    info = FrameFilterInfo()
    raw = np.frombuffer(bytes(buf), dtype=np.uint8).copy()                    # a heap block of exactly the frame's bytes
    rc = L.zsmi_readFrameFilter(ctypes.c_void_p(raw.ctypes.data) if len(raw) else None, len(raw) if size is None else size, ctypes.byref(info))
    if rc:
        return rc
    return {"n": info.nFrames, "delim": info.delim, "g": info.gram, "L": info.log2Bits, "size": info.size, "saturated": info.saturated}


def host_filter(L, buf, patterns, mode=Q.ANY, flags=0, first=0, count=None, capacity=None):
    """zsmi_filterFrames into an array of exactly `capacity` entries with a sentinel behind it: (rc, the list written, the four result
    words, whether the sentinel is intact)"""
    q, keep = Q.query(L, patterns, mode, flags)
    if count is None:
        count = struct.unpack_from("<I", buf, 16)[0] - first
    capacity = count if capacity is None else capacity
    out = np.full(capacity + 1, 0xA5A5A5A5, dtype=np.uint32)
    res = np.full(4, 0xDEAD, dtype=np.uint64)
    p = ctypes.c_void_p
    rc = L.zsmi_filterFrames(bytes(buf), len(buf), ctypes.byref(q), first, count, p(out.ctypes.data) if capacity else None, capacity, p(res.ctypes.data))
    result = [int(v) for v in res]
    written = min(result[1], capacity) if rc == 0 else 0
    return rc, out[:written].tolist(), result, int(out[capacity]) == 0xA5A5A5A5 and bool((out[written:] == 0xA5A5A5A5).all())


# ---- the device calls (tests/test_gpu_frame_filter.py) ----
def device_build(L, H, codec, data, sizes, delim=10, g=4, Lg=13, places=None, slack=0):
    """zsmi_buildFrameFilterDevice with every array exactly as long as the header sizes it (the filter `slack` bytes longer), canaries on
    both sides of each (tests/_hip.py), checked here: (rc, the four result words, the filter's bytes).  places: instead of the sizes' sums"""
    from _hip import Dev
    from _resident import down, up
    p = ctypes.c_void_p
    places = np.ascontiguousarray(offsets_of(sizes) if places is None else places, dtype=np.uint64)
    n = len(places) - 1
    total = FIXED + n * (1 << (Lg - 3)) + slack
    flt, res = Dev(H, total), Dev(H, 32)
    src, d_places = Dev(H, max(len(data), 1), bytes(data)), up(H, places)
    assert H.hipDeviceSynchronize() == 0
    try:
        rc = L.zsmi_buildFrameFilterDevice(codec.ctx, p(src.p), len(data), p(d_places.p), n, delim, g, Lg, p(flt.p), total, p(res.p))
        codec.sync()
        vals = []
        for name, dev, t in (("dResult", res, np.uint64), ("dFilter", flt, np.uint8), ("the text", src, np.uint8), ("dPlaces", d_places, np.uint64)):
            v, ok = down(dev, t)
            assert ok, "a guard word in front of or behind " + name + " is gone"
            vals.append(v.copy())
        assert vals[2].tobytes()[:len(data)] == bytes(data) and (vals[3] == places).all(), "an input changed"
        return rc, [int(v) for v in vals[0]], vals[1].tobytes()
    finally:
        for dev in (flt, res, src, d_places):
            dev.free()


def same_build(L, H, codec, data, sizes, delim=10, g=4, Lg=13, what=""):
    """a device build against the statement: status 0, the frame byte for byte, its size, the all-ones slots, the grams hashed"""
    slots, hashed = slots_of(data, sizes, delim, g, Lg)
    want = frame(data, sizes, delim, g, Lg, slots)
    full = sum(1 for v in slots if v == (1 << (1 << Lg)) - 1)
    rc, result, got = device_build(L, H, codec, data, sizes, delim, g, Lg, slack=24)
    assert rc == 0 and result == [0, len(want), full, hashed], (what, rc, result, [0, len(want), full, hashed])
    bad = np.flatnonzero(np.frombuffer(got[:len(want)], dtype=np.uint8) != np.frombuffer(want, dtype=np.uint8)).tolist()
    assert not bad, (what, "bytes differ, first at", bad[:8], "frames", [(i - FIXED) // (1 << (Lg - 3)) for i in bad[:8]])
    assert got[len(want):] == b"\xA5" * 24, (what, "written behind the frame")
    return want


def device_check(L, H, codec, buf, size=None):
    """zsmi_checkFrameFilterDevice on exactly the bytes of buf: (rc, the eight result words)"""
    from _hip import Dev
    from _resident import down
    flt, res = Dev(H, max(len(buf), 1), bytes(buf)), Dev(H, 64)
    assert H.hipDeviceSynchronize() == 0
    try:
        rc = L.zsmi_checkFrameFilterDevice(codec.ctx, ctypes.c_void_p(flt.p), len(buf) if size is None else size, ctypes.c_void_p(res.p))
        codec.sync()
        v, ok = down(res, np.uint64)
        assert ok and down(flt)[1], "a guard word is gone"
        return rc, [int(x) for x in v]
    finally:
        flt.free(); res.free()


def device_filter(L, H, codec, buf, patterns, mode=Q.ANY, flags=0, first=0, count=None, capacity=None):
    """zsmi_filterFramesDevice with dFrames exactly `capacity` entries: (rc, the list as far as written, the four result words, whether
    everything behind the written entries is untouched)"""
    from _hip import Dev, CANARY
    from _resident import down
    p = ctypes.c_void_p
    q, keep = Q.query(L, patterns, mode, flags)
    if count is None:
        count = struct.unpack_from("<I", buf, 16)[0] - first
    capacity = count if capacity is None else capacity
    flt, out, res = Dev(H, max(len(buf), 1), bytes(buf)), Dev(H, max(4 * capacity, 1)), Dev(H, 32)
    assert H.hipDeviceSynchronize() == 0
    try:
        rc = L.zsmi_filterFramesDevice(codec.ctx, p(flt.p), len(buf), ctypes.byref(q), first, count, p(out.p) if capacity else None, capacity, p(res.p))
        codec.sync()
        r, ok0 = down(res, np.uint64)
        v, ok1 = down(out, np.uint32)
        assert ok0 and ok1 and down(flt)[1], "a guard word is gone"
        result = [int(x) for x in r]
        written = min(result[1], capacity) if rc == 0 and result[0] < 1 << 63 else 0
        rest = v[written:capacity].view(np.uint8) if capacity else v.view(np.uint8)
        return rc, [int(x) for x in v[:written]], result, bool((rest == CANARY).all())
    finally:
        flt.free(); out.free(); res.free()


def poison_child():
    """run in a process of its own on the debug-hook library (ZSMI_DEBUG_LIB=1): the three device calls on a context whose scratch is
    overwritten before every call (zsmi_dbg_fillScratch: zeros, ones, a seeded mix), each result held against the statement"""
    from zstandard_amd import BatchCodec, _lib
    from _hip import hip_of
    import _split as S
    assert _lib.DEBUG
    L, H, codec = _lib.lib(), hip_of(), BatchCodec(0)
    text = tokens(3 * TILE + 500, 31)
    shapes = [(text, S.Split(text, 10, 4096, 1 << 16).sizes, 4, 13), (text, fixed(len(text), 1000), 3, 9), (b"", [0, 0], 4, 9)]

    def once(poke, what):
        for data, sizes, g, Lg in shapes:
            poke()
            want = same_build(L, H, codec, data, sizes, 10, g, Lg, what)
            n = len(sizes)
            poke()
            assert device_check(L, H, codec, want) == (0, [0, n, 10, g, Lg, len(data), parse(want)["saturated"], 0]), what
            for patterns, mode in (([text[100:108].replace(b"\n", b" ")], Q.ANY), ([b"ab"], Q.ALL), ([b"zqzqzq", text[5000:5006].replace(b"\n", b" ")], Q.ANY)):
                w, s = filter_frames(want, patterns, mode)
                poke()
                assert device_filter(L, H, codec, want, patterns, mode) == (0, w, [len(w), len(w), n, s], True), (what, patterns)
    once(lambda: None, "as the context was")                             # the buffers exist from here on
    for pattern in (0x00, 0xFF, 0x5EED0BAD):
        def poke():
            filled = _lib.fill_scratch(codec.ctx, pattern)
            assert filled["seek"] > 0 and filled["staging"] >= 40, ("the fill is vacuous", filled)
        once(poke, "scratch filled with %#x" % pattern)
    # the host form in many windows over a small archive (the debug-hook library reads ZSMI_ARCHIVE_WINDOW; the product's windows hold
    # 256 MiB of content): a frame a window, a few frames a window, one window - byte for byte the statement's frame
    import os
    from zstandard_amd import SeekableArchive
    for sizes, g, Lg in ((shapes[0][1], 4, 13), (fixed(len(text), 1000), 3, 9), ([0, 0, 700, 0, 0, len(text) - 700, 0], 4, 9)):
        archive = codec.compress_seekable_frames_host(np.frombuffer(text, dtype=np.uint8), sizes, 3, True)
        want = frame(text, sizes, 10, g, Lg)
        for window in ("1", "9000", "20000", "0"):
            os.environ["ZSMI_ARCHIVE_WINDOW"] = window
            sa = SeekableArchive(archive)
            try:
                sa._open()
                _lib.fill_scratch(sa.codec.ctx, 0x5EED0BAD)
                assert sa.build_frame_filter(b"\n", g, Lg) == want, ("windows of", window, len(sizes), g, Lg)
            finally:
                sa.close()
    codec.close()
    print("poison ok")

# ---- the list search (tests/test_gpu_find_frames.py) ----
def list_search(data, sizes, first_record, frames, patterns, mode=Q.ANY, flags=0, delim=10):
    """the run rule: (records, hits, matches, content bytes) of the query search over the listed frames - a run is a maximal stretch of
    the list whose frames follow one another; an occurrence lies inside one run; its record is first_record[f] + the delimiters in
    front of it inside the frame f it starts in (no record starts in an empty frame); each satisfying record once a run"""
    at = offsets_of(sizes)
    runs = []
    for f in frames:
        if runs and runs[-1][1] == f:
            runs[-1][1] = f + 1
        else:
            runs.append([f, f + 1])
    records, hits, matches = [], [], 0
    for a, b in runs:
        text = data[at[a]:at[b]]
        r, h, m = Q.find(text, patterns, mode, flags, delim, 0)
        starts = [0] + [i + 1 for i, c in enumerate(text) if c == delim]                # where ordinal k of the run starts
        for k, hk in zip(r, h):
            start = at[a] + starts[k]
            f = max(i for i in range(a, b) if at[i] <= start and sizes[i] > 0)
            records.append(int(first_record[f]) + data[at[f]:start].count(bytes([delim])))
            hits.append(hk)
        matches += m
    return records, hits, matches, sum(sizes[f] for f in frames)


if __name__ == "__main__":
    import os, sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    if sys.argv[1:] == ["poison"]:
        poison_child()

