"""The record index restated in numpy (test infrastructure): the rule P(x), MISALIGNED, the index frame's layout, its check and the attached
archive, as include/zsmi.h states them - never through the library.  The yardstick of the host calls (tests/test_record_index_host.py),
of the text form on the device (tests/test_gpu_record_index.py) and of the archive calls (tests/test_gpu_record_index_archive.py)."""
import struct
import numpy as np

MAGIC, INNER, VERSION = 0x184D2A5D, 0x58444952, 1
K1, K2 = 0x9E3779B185EBCA87, 0xC2B2AE3D27D4EB4F
EMPTY_HASH = 0x51D8E999
SEEK_SKIP, SEEK_MAGIC = 0x184D2A5E, 0x8F92EAB1
M64 = (1 << 64) - 1
E_GENERIC, E_PREFIX, E_VERSION, E_CORRUPT, E_UNSUPPORTED, E_PARAM, E_INIT, E_TOO_SMALL, E_SRC_SIZE, E_FRAME_INDEX = 1, 10, 12, 20, 40, 42, 62, 70, 72, 100
TILE = 16384
NAMES = ("zsmi_recordIndexFrameSize", "zsmi_writeRecordIndexFrame", "zsmi_readRecordIndexFrame", "zsmi_indexRecords", "zsmi_seekableAttachRecordIndex",
         "zsmi_indexRecordsDevice", "zsmi_seekableIndexRecordsResident", "zsmi_seekableLoadRecordIndexResident", "zsmi_seekableAttachRecordIndexResident",
         "zsmi_seekableLoadRecordIndexHost", "zsmi_seekableIndexRecordsHost")


def _delims_before(data, delim):
    """D[x] = the delimiters in data[0, x), x = 0 .. len(data)"""
    is_delim = np.frombuffer(bytes(data), dtype=np.uint8) == delim
    return np.concatenate([[0], np.cumsum(is_delim, dtype=np.uint64)]).astype(np.uint64)


def offsets_of(sizes):
    return np.concatenate([[0], np.cumsum(np.asarray(sizes, dtype=np.uint64), dtype=np.uint64)]).astype(np.uint64)


class Index:
    """first_record[0 .. n] = P(places[j]), records (P(size)), delimiters, misaligned - over data with the frames' borders `places`
    (ascending, 0 first, len(data) last).  at_end False: len(data) is not the content's end - no tail record, and a frame that ends
    there can be misaligned"""

    def __init__(self, data, delim, places, at_end=True):
        size = len(data)
        places = np.asarray(places, dtype=np.uint64)
        assert int(places[0]) == 0 and int(places[-1]) == size and (np.diff(places.astype(np.int64)) >= 0).all()
        D = _delims_before(data, delim)
        tail = 1 if (at_end and size and data[size - 1] != delim) else 0
        p = D[places.astype(np.int64)]
        self.first_record = (p + np.where(places == size, tail, 0).astype(np.uint64)).astype(np.uint64)
        self.delimiters = int(D[size])
        self.records = self.delimiters + tail
        a, b = places[:-1].astype(np.int64), places[1:].astype(np.int64)
        holds = D[b] > D[a]
        raw = np.frombuffer(bytes(data), dtype=np.uint8)
        last_is = np.zeros(len(a), dtype=bool)
        full = b > a
        last_is[full] = raw[b[full] - 1] == delim
        ends = (b == size) & bool(at_end)
        self.misaligned_frames = np.flatnonzero(holds & ~last_is & ~ends)
        self.misaligned = len(self.misaligned_frames)
        self.counts = np.diff(self.first_record.astype(np.int64))


def check_of(counts, records, delim):
    total = (records * K2 + delim) & M64
    for i, c in enumerate(counts):
        total = (total + (int(c) + 1) * (2 * i + 1) * K1) & M64
    return total


def check_of_np(counts, records, delim):
    """the same sum with numpy's wrapping 64-bit arithmetic: for millions of counts"""
    c = np.asarray(counts, dtype=np.uint64)
    with np.errstate(over="ignore"):
        terms = (c + np.uint64(1)) * (np.uint64(2) * np.arange(len(c), dtype=np.uint64) + np.uint64(1)) * np.uint64(K1)
        return (int(terms.sum(dtype=np.uint64)) + records * K2 + delim) & M64


def frame(first_record, delim):
    """the index frame of first_record[0 .. n]"""
    fr = [int(v) for v in first_record]
    n = len(fr) - 1
    counts = [fr[i + 1] - fr[i] for i in range(n)]
    assert fr[0] == 0 and all(0 <= c < 1 << 32 for c in counts)
    return struct.pack("<IIIBBHIIQQ", MAGIC, 32 + 4 * n, INNER, VERSION, delim, 0, n, 0, fr[n], check_of(counts, fr[n], delim)) + struct.pack("<%dI" % n, *counts)


def parse(buf):
    """(first_record, delim) of a frame that holds: its fields asserted one by one"""
    magic, frame_size, inner, version, delim, r16, n, r32, records, check = struct.unpack_from("<IIIBBHIIQQ", buf)
    assert (magic, inner, version, r16, r32) == (MAGIC, INNER, VERSION, 0, 0) and frame_size == 32 + 4 * n and len(buf) == 40 + 4 * n
    counts = struct.unpack_from("<%dI" % n, buf, 40)
    assert sum(counts) == records and check == check_of(counts, records, delim)
    return [0] + np.cumsum(counts, dtype=np.uint64).tolist() if n else [0], delim


def table_of(archive):
    """(n, entry bytes, the table's place, [(cSize, dSize[, hash])]) of a seekable archive's table"""
    n, desc, magic = struct.unpack_from("<IBI", archive, len(archive) - 9)
    assert magic == SEEK_MAGIC
    entry = 12 if desc & 0x80 else 8
    at = len(archive) - 17 - n * entry
    assert struct.unpack_from("<II", archive, at) == (SEEK_SKIP, n * entry + 9)
    rows = [struct.unpack_from("<III" if entry == 12 else "<II", archive, at + 8 + i * entry) for i in range(n)]
    return n, entry, at, rows


def attached(archive, first_record, delim):
    """the archive with the index frame between its last frame and its table, and the frame's entry in the table"""
    n, entry, at, rows = table_of(archive)
    assert len(first_record) == n + 1
    f = frame(first_record, delim)
    rows = rows + [(len(f), 0, EMPTY_HASH) if entry == 12 else (len(f), 0)]
    table = struct.pack("<II", SEEK_SKIP, (n + 1) * entry + 9) + b"".join(struct.pack("<III" if entry == 12 else "<II", *r) for r in rows)
    return archive[:at] + f + table + struct.pack("<IBI", n + 1, archive[len(archive) - 5], SEEK_MAGIC)


def raw_frame(content):
    """a zstd frame of one raw block (Single_Segment, a one-byte Frame_Content_Size): content of 0 .. 255 bytes"""
    assert len(content) < 256
    return struct.pack("<IBB", 0xFD2FB528, 0x20, len(content)) + struct.pack("<I", (len(content) << 3) | 1)[:3] + content


def text_archive(parts, checksum=False):
    """a seekable archive of raw-block frames, one a part, with its table (no checksums unless asked: then the entries carry 0 - such an
    archive is for the host calls alone, which judge the table and never a frame)"""
    frames = [raw_frame(p) for p in parts]
    entry = 12 if checksum else 8
    rows = b"".join(struct.pack("<II", len(f), len(p)) + (b"\0\0\0\0" if checksum else b"") for f, p in zip(frames, parts))
    return b"".join(frames) + struct.pack("<II", SEEK_SKIP, len(parts) * entry + 9) + rows + struct.pack("<IBI", len(parts), 0x80 if checksum else 0, SEEK_MAGIC)


def cases():
    """name -> (data, delim, frame sizes)"""
    import _split as S
    c = {}
    for name, (data, delim, T, M) in S.cases().items():
        c["split_" + name] = (data, delim, S.Split(data, delim, T, M).sizes)
    c["empty_text_no_frames"] = (b"", 10, [])
    c["empty_text_three_empty_frames"] = (b"", 10, [0, 0, 0])
    c["delimiters_only_fixed_7"] = (b"\n" * 100, 10, [7] * 14 + [2])
    c["no_delimiter_fixed_10"] = (b"a" * 95, 10, [10] * 9 + [5])
    c["unterminated_tail_misaligned"] = (b"ab\ncd\nef", 10, [4, 4])
    c["empty_frames_at_the_start"] = (b"ab\ncd\n", 10, [0, 0, 3, 3])
    c["empty_frames_at_the_end"] = (b"ab\ncd\n", 10, [3, 3, 0, 0])
    c["empty_frames_at_the_end_behind_a_tail"] = (b"ab\ncd", 10, [3, 2, 0, 0])
    c["empty_frames_in_the_middle"] = (b"ab\ncd\nef\n", 10, [2, 0, 0, 1, 0, 6])
    text = S.lines(77, 120, 90)
    c["fixed_64_over_lines"] = (text, 10, [64] * (len(text) // 64) + ([len(text) % 64] if len(text) % 64 else []))
    c["delim_0_fixed"] = (S.lines(5, 40, 30, delim=0), 0, None)
    c["delim_255_fixed"] = (S.lines(6, 40, 30, delim=255), 255, None)
    for k in ("delim_0_fixed", "delim_255_fixed"):
        d, delim, _ = c[k]
        c[k] = (d, delim, [50] * (len(d) // 50) + ([len(d) % 50] if len(d) % 50 else []))
    return c


# ---- the device call on text (tests/test_gpu_record_index.py) ----
class Device:
    """what one zsmi_indexRecordsDevice call left: rc, result (four words), first (the whole array)"""


def device(L, H, codec, data, places, delim=10, at_end=True, base=None, offset=0):
    """the call with every array exactly as long as the header sizes it, canaries on both sides of each (tests/_hip.py), checked here.
    base: the value of a device word handed over as dBase (None: NULL).  offset > 0: the text is a slice at that byte offset of a larger
    device buffer whose every other byte is the delimiter.  The test synchronises before it reads anything back."""
    import ctypes
    from _hip import Dev, CANARY
    from _resident import down, up
    p = ctypes.c_void_p
    places = np.ascontiguousarray(places, dtype=np.uint64)
    n = len(places) - 1
    around = bytes([delim])
    # (the outputs first: their canary fills run on the null stream, and the blocking copies of the inputs behind them have waited for those)
    first, res = Dev(H, 8 * (n + 1)), Dev(H, 32)
    src = Dev(H, max(len(data), 1) + (offset + 64 if offset else 0), (around * offset + bytes(data) + around * 64) if offset else bytes(data))
    d_places = up(H, places)
    d_base = up(H, np.array([base], dtype=np.uint64)) if base is not None else None
    assert H.hipDeviceSynchronize() == 0
    d = Device()
    try:
        d.rc = L.zsmi_indexRecordsDevice(codec.ctx, p(src.p + offset), len(data), p(d_places.p), n, delim, 1 if at_end else 0, p(d_base.p) if d_base else None,
                                         p(first.p), p(res.p))
        codec.sync()
        vals = []
        for name, dev, t in (("dResult", res, np.uint64), ("dFirstRecord", first, np.uint64), ("the text", src, np.uint8), ("dPlaces", d_places, np.uint64)):
            v, ok = down(dev, t)
            assert ok, "a guard word in front of or behind " + name + " is gone"
            vals.append(v.copy())
        assert (vals[3] == places).all()
        d.result, d.first = [int(v) for v in vals[0]], vals[1]
        d.entry0_untouched = bool((vals[1][:1].view(np.uint8) == CANARY).all())
        return d
    finally:
        for dev in (src, d_places, first, res, d_base):
            if dev is not None:
                dev.free()


def same_as_rule(d, data, places, delim=10, at_end=True, base=None, what=""):
    """a device call against the restatement: status 0, the three counts, every entry (entry 0 is the caller's when there is a base)"""
    want = Index(data, delim, places, at_end)
    assert d.rc == 0 and d.result == [0, want.records, want.misaligned, want.delimiters], (what, d.rc, d.result, [0, want.records, want.misaligned, want.delimiters])
    b = 0 if base is None else base
    expect = (want.first_record + np.uint64(b)).astype(np.uint64)
    if base is None:
        bad = np.flatnonzero(d.first != expect)
    else:
        assert d.entry0_untouched, (what, "entry 0 is the caller's when there is a base")
        bad = np.flatnonzero(d.first[1:] != expect[1:]) + 1
    assert not len(bad), (what, "entries differ, first at", bad[:5].tolist(), d.first[bad[:5]].tolist(), expect[bad[:5]].tolist())
    return want


def seeded_text(size, seed, every=60, delim=10):
    """`size` seeded lower-case bytes with a delimiter on about one byte in `every`"""
    rng = np.random.default_rng(seed)
    b = rng.integers(97, 123, size, dtype=np.uint8)
    b[rng.random(size) < 1.0 / every] = delim
    return b.tobytes()


def poison_child():
    """run in a process of its own on the debug-hook library (ZSMI_DEBUG_LIB=1): the text form on a context whose scratch is overwritten
    before every call (zsmi_dbg_fillScratch: zeros, ones, a seeded mix of small and large words), each result held against the rule.  The
    fill must reach the seekable scratch and the scan's tile sums the call before it reserved: it cannot be vacuous."""
    from zstandard_amd import BatchCodec, _lib
    from _hip import hip_of
    assert _lib.DEBUG
    L, H, codec = _lib.lib(), hip_of(), BatchCodec(0)
    size = 40 * TILE + 321
    data = seeded_text(size, 17)
    rng = np.random.default_rng(18)
    shapes = [(data, np.sort(np.concatenate([[0, 0, size, size], np.arange(0, size, 1000), rng.integers(0, size + 1, 500)])), True, None),
              (data[:3 * TILE], [0, TILE - 100, 2 * TILE + 50, 3 * TILE], False, (1 << 32) - 3),
              (b"", [0, 0, 0], True, None)]
    for text, places, at_end, base in shapes:                                # the buffers exist from here on
        same_as_rule(device(L, H, codec, text, places, 10, at_end, base), text, places, 10, at_end, base, "as the context was")
    for pattern in (0x00, 0xFF, 0x5EED0BAD):
        for text, places, at_end, base in shapes:
            filled = _lib.fill_scratch(codec.ctx, pattern)
            assert filled["seek"] >= 16 * 41 and sum(filled.values()) > filled["seek"], ("the fill is vacuous", filled)
            same_as_rule(device(L, H, codec, text, places, 10, at_end, base), text, places, 10, at_end, base, ("scratch filled with %#x" % pattern, len(text)))
    codec.close()
    print("poison ok")


def windows_of(sizes, limit):
    """the window plan restated: [(first frame, frames)] in ascending order - a window takes frames while its content stays at or below
    `limit` bytes, and one frame at least (a longer frame is a window of its own)"""
    at = [int(v) for v in offsets_of(sizes)]
    n, out, f = len(sizes), [], 0
    while f < n:
        g = f + 1
        while g < n and at[g + 1] - at[f] <= limit:
            g += 1
        out.append((f, g - f))
        f = g
    return out


def windows_child():
    """run in a process of its own on the debug-hook library (ZSMI_DEBUG_LIB=1), which reads ZSMI_ARCHIVE_WINDOW (the product's windows
    hold 256 MiB of content): the host rebuild (zsmi_seekableIndexRecordsHost) of archives without an index frame in a frame a window, a
    few frames a window and one window, on poisoned scratch - the status, the three counts and every entry of the array against the
    rule; the windows chain through the array and add up the counts.  The launches of k_find_frames - one a window - say that the
    windows were the plan's: the override cannot be vacuous"""
    import ctypes, os
    import _split as S
    from zstandard_amd import BatchCodec, SeekableArchive, _lib
    assert _lib.DEBUG
    L, codec = _lib.lib(), BatchCodec(0)
    p = ctypes.c_void_p
    text = seeded_text(3 * TILE + 500, 41)
    size = len(text)
    shapes = [("split at 4096", S.Split(text, 10, 4096, 1 << 16).sizes), ("fixed 1000", [1000] * (size // 1000) + ([size % 1000] if size % 1000 else [])),
              ("empty frames at the borders", [0, 0, 700, 0, 0, size - 700, 0])]
    for what, sizes in shapes:
        assert sum(sizes) == size
        want = Index(text, 10, offsets_of(sizes), True)
        assert (want.misaligned == 0) == (what == "split at 4096"), (what, want.misaligned)          # (the fixture: only frames that end on delimiters are aligned)
        archive = codec.compress_seekable_frames_host(np.frombuffer(text, dtype=np.uint8), sizes, 3, True)
        for window in ("1", "9000", "20000", "0"):
            os.environ["ZSMI_ARCHIVE_WINDOW"] = window
            plan = windows_of(sizes, int(window) or 256 << 20)
            assert (len(plan) == 1) == (window == "0"), (what, window, plan)
            sa = SeekableArchive(archive)
            try:
                sa._open()
                assert sa.num_frames == len(sizes)
                _lib.fill_scratch(sa.codec.ctx, 0x5EED0BAD)
                sa.codec.enable_timing(True)
                first, result = np.full(len(sizes) + 1, M64, dtype=np.uint64), np.full(4, M64, dtype=np.uint64)
                rc = L.zsmi_seekableIndexRecordsHost(sa.codec.ctx, sa.handle, 10, p(first.ctypes.data), p(result.ctypes.data))
                got = [int(v) for v in result]
                print(what, "windows of", window, "->", len(plan), "rc", rc, "result", got, flush=True)
                assert rc == 0, (what, window, rc)
                assert got == [0, want.records, want.misaligned, want.delimiters], (what, window, got, [0, want.records, want.misaligned, want.delimiters])
                bad = np.flatnonzero(first != want.first_record)
                assert not len(bad), (what, window, "entries differ, first at", bad[:5].tolist(), first[bad[:5]].tolist(), want.first_record[bad[:5]].tolist())
                assert sa.codec.kernel_times()["k_find_frames"][1] == len(plan), (what, window, "the windows are not the plan's")
            finally:
                sa.close()
    codec.close()
    print("windows ok")


if __name__ == "__main__":
    import os, sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    if sys.argv[1:] == ["poison"]:
        poison_child()
    if sys.argv[1:] == ["windows"]:
        windows_child()
