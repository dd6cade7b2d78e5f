"""Find records by content on plain text in device memory (zsmi_findRecordsDevice).  The yardstick is tests/_find.py's Python statement of
the rule on the same bytes, never another call of the library.  dRecords and dResult are exactly as long as the header sizes them,
between canaries (F.device checks them and that the source is unchanged); nothing depends on a wait inside the call.  The shapes are the
smallest at which the kernels can go wrong: the borders of a lane's 16 bytes, of a 4096-byte step and of a 16384-byte tile, the buffer's
end, a record over several tiles, and texts of more than 1024 and more than 4096 tiles for the scans' and the carry's later rounds."""
import ctypes
import numpy as np
import pytest
import _find as F, _split as S
from _hip import hip_of

pytestmark = pytest.mark.gpu
LANE, STEP, TILE = F.LANE, F.STEP, F.TILE


@pytest.fixture(scope="module")
def L():
    from zstandard_amd import _lib
    return _lib.lib()


@pytest.fixture(scope="module")
def H():
    return hip_of()


@pytest.fixture(scope="module")
def codec():
    from zstandard_amd import BatchCodec
    bc = BatchCodec(0)
    yield bc
    bc.close()


def run(L, H, codec, data, pattern, delim=10, base=None, what="", **kw):
    d = F.device(L, H, codec, data, pattern, delim, base, **kw)
    F.same_as_rule(d, data, pattern, delim, base or 0, kw.get("capacity"), what)
    return d


# ------------------------------------------------------------------ 1. an occurrence on every side of every border
def borders(kind, count):
    """`count` borders of one kind, 1024 bytes apart at least: a lane border that is no step's, a step border that is no tile's, a tile's"""
    if kind == "lane":
        return [1024 * (j + 1) + LANE * (1 + j % 5) for j in range(count)]
    if kind == "step":
        return [TILE * j + STEP * (1 + j % 3) for j in range(count)]
    return [TILE * (j + 1) for j in range(count)]


@pytest.mark.parametrize("kind", ("lane", "step", "tile"))
@pytest.mark.parametrize("m", F.SIZES)
def test_border_shifts(L, H, codec, m, kind):
    """shift j of -m .. 0 at border j: the occurrence ends at the border (-m), crosses it with every split of its bytes, starts at it (0).
    A delimiter in front of each start: every occurrence is a record of its own, so that a lost or doubled one shows in the numbers"""
    pattern = F.pattern_of(m)
    shifts = list(range(-m, 1))
    at = borders(kind, len(shifts))
    assert all(b % LANE == 0 for b in at) and (kind != "lane" or all(b % STEP for b in at)) and (kind != "step" or all(b % STEP == 0 and b % TILE for b in at))
    starts = [b + s for b, s in zip(at, shifts)]
    size = at[-1] + 2 * m + 37                                                     # (odd: the last tile goes byte by byte)
    data = F.place(size, pattern, starts, delims=[p - 1 for p in starts if p > 0])
    records, matches = F.find(data, pattern)
    assert matches == len(shifts) and len(records) == len(shifts)
    run(L, H, codec, data, pattern, what=(m, kind))


# ------------------------------------------------------------------ 2. the buffer's end
@pytest.mark.parametrize("m", F.SIZES)
def test_end_of_buffer_and_false_tail(L, H, codec, m):
    """an occurrence that ends exactly at srcSize is found; a buffer whose last m - 1 bytes start the pattern, with the bytes BEHIND srcSize in
    the allocation completing it, holds none - whole tiles (the vector loads and the halo) and odd sizes (the byte loop) alike"""
    pattern = F.pattern_of(m)
    for size in (m, 1000 + m, TILE, TILE + 5, 2 * TILE, 2 * TILE + m - 1):
        if size < m:
            continue
        data = F.place(size, pattern, [size - m], delims=[3] if size - m > 3 else [])
        d = run(L, H, codec, data, pattern, what=("ends at srcSize", m, size))
        assert d.result[2] == 1
        if m > 1:
            cut = data[:size - 1]                                                  # its last m - 1 bytes: the pattern less its last byte
            d = run(L, H, codec, cut, pattern, behind=data[size - 1:] + pattern * 2, what=("false tail", m, size))
            assert d.result[:3] == [0, 0, 0]
            if size + m - 1 <= 3 * TILE:
                whole = F.place(size, pattern, [])                                 # nothing inside; the pattern starts right at srcSize
                d = run(L, H, codec, whole, pattern, behind=pattern * 2, what=("behind the end", m, size))
                assert d.result[:3] == [0, 0, 0]


@pytest.mark.parametrize("offset", range(1, 16))
def test_odd_sizes_and_alignment(L, H, codec, offset):
    text = S.text_lines(3 * TILE + 1000, seed=offset)
    size = 3 * TILE + 16 * offset + offset                                         # no multiple of 16, more than three tiles
    data = text[:size]
    for pattern in (data[500:502].replace(b"\n", b"q"), b"e", data[TILE - 3:TILE + 4].replace(b"\n", b"q")):
        run(L, H, codec, data, pattern, offset=offset, behind=b"e" * 40, what=(offset, pattern))


# ------------------------------------------------------------------ 3. records and tiles
def test_a_record_of_three_tiles(L, H, codec):
    pattern = F.pattern_of(5)
    data = F.place(40000, pattern, [100, TILE + 7000, 2 * TILE + 2000])
    d = run(L, H, codec, data, pattern, what="one record")
    assert d.result[:3] == [1, 1, 3] and d.records == [0]
    data = F.place(40000, pattern, [100, TILE, 2 * TILE + 2000], delims=[TILE - 1])  # a delimiter as a tile's last byte, an occurrence as the next one's first bytes
    d = run(L, H, codec, data, pattern, what="two records")
    assert d.result[:3] == [2, 2, 3] and d.records == [0, 1]
    data = F.place(40000, pattern, [TILE - 2, 2 * TILE + 2000], delims=[50, 2 * TILE + 1999])      # crosses the border; the third tile's head holds none
    d = run(L, H, codec, data, pattern, base=1 << 33, what="across and behind")
    assert d.records == [(1 << 33) + 1, (1 << 33) + 2]
    data = F.place(5 * TILE, pattern, [10, 4 * TILE + 9], delims=[4])              # tiles without either between the two: the state passes through them
    d = run(L, H, codec, data, pattern, what="through empty tiles")
    assert d.result[:3] == [1, 1, 2] and d.records == [1]


def test_two_neighbours_in_one_lane_group(L, H, codec):
    data = b"a!X\n!Xaa\naa!X\n!X" * 3 + b"\n" + b"!X!X\n\n!X" * 2000                 # 16 bytes: four records; then several occurrences a record, empty records
    run(L, H, codec, data, b"!X", what="neighbours")
    run(L, H, codec, data, b"!", what="neighbours, one byte")


def test_overlaps(L, H, codec):
    data = b"a" * 20001
    d = run(L, H, codec, data, b"aa", what="aa in aaaa...")
    assert d.result[:3] == [1, 1, 20000]
    lines = bytearray(data)
    for p in (0, 15, 16, 17, STEP - 1, STEP, TILE - 1, TILE, TILE + 1, 20000):
        lines[p] = 10
    run(L, H, codec, bytes(lines), b"aa", what="aa in lines of a")
    run(L, H, codec, bytes(lines), b"aaa", what="aaa in lines of a")


def test_one_repeated_byte(L, H, codec):
    """every position is a candidate and every compare runs to the pattern's end"""
    data = b"q" * (64 << 10)
    d = run(L, H, codec, data, b"q" * 256, what="64 KiB of q")
    assert d.result[:3] == [1, 1, (64 << 10) - 255]


@pytest.mark.parametrize("edge", (1024, 4096))
def test_more_than_1024_tiles(L, H, codec, edge):
    """about 17 MiB and about 65 MiB: the scans' later tiles, and the carry kernel's second round, which begins at tile 4096.  One record runs
    from tile edge - 2 into tile edge + 2 - across tile `edge` - with occurrences on both sides of it"""
    block = S.text_lines(1 << 16, seed=3)
    size = (edge + 64) * TILE + 333
    data = bytearray(block * (size // len(block) + 1))[:size]
    pattern = b"!XY7"
    a, b = (edge - 2) * TILE + 100, (edge + 2) * TILE + 50
    data[a:b] = b"a" * (b - a)
    for p in ((edge - 1) * TILE + 5, edge * TILE - 2, (edge + 1) * TILE + 9, 5000, (edge + 40) * TILE + 7777):
        data[p:p + 4] = pattern
    data = bytes(data)
    assert len(data) > edge * TILE and b"\n" not in data[a:b]
    d = run(L, H, codec, data, pattern, what="rare")
    assert d.result[:3] == [3, 3, 5]
    if edge == 1024:
        run(L, H, codec, data, b"ab", base=5, what="common")


@pytest.mark.parametrize("delim", (0, 255))
def test_delimiters_0_and_255(L, H, codec, delim):
    data = S.lines(40 + delim, 400, 120, delim=delim)
    pattern = bytes([1, 2]) if delim == 255 else bytes([254, 253])
    one = bytes(b for b in data if b != delim)[:1]
    for base in (None, 0, 12345678901234):
        run(L, H, codec, data, one, delim, base, what=(delim, base, "one byte"))
        run(L, H, codec, data + pattern + data[:100] + pattern, pattern, delim, base, what=(delim, base, "two bytes"))


def test_empty_text_and_a_pattern_longer_than_the_text(L, H, codec):
    d = run(L, H, codec, b"", b"x", what="empty")
    assert d.result == [0, 0, 0, 0]
    d = run(L, H, codec, b"abc", b"abcd", what="longer")
    assert d.result == [0, 0, 0, 3]
    d = run(L, H, codec, b"abc\n" * 3, b"abc\x00" * 64, what="256 in 12")
    assert d.result == [0, 0, 0, 12]


def test_capacity(L, H, codec):
    data = S.text_lines(5 * TILE, seed=12)
    records, matches = F.find(data, b"e")
    assert len(records) > 300 and matches > len(records)
    run(L, H, codec, data, b"e", capacity=0, null_records=True, what="only count")
    for cap in (1, 7, len(records) - 1, len(records), len(records) + 5):
        run(L, H, codec, data, b"e", capacity=cap, base=9, what=("capacity", cap))


# ------------------------------------------------------------------ 4. the host checks
def test_refusals_in_order(L, H, codec):
    """each refusal with every later one present too, so that the order shows; a refused call queues nothing and leaves every array as it
    was"""
    from _hip import Dev, CANARY
    from _resident import down
    p = ctypes.c_void_p
    src, rec, res = Dev(H, 64, b"ab\n" * 21), Dev(H, 64), Dev(H, 32)
    find = L.zsmi_findRecordsDevice
    try:
        assert find(None, None, 5, 256, None, 0, None, None, 3, None) == F.E_INIT
        assert find(codec.ctx, None, 5, 256, b"\n", 0, None, p(rec.p), 3, None) == F.E_GENERIC               # dResult
        assert find(codec.ctx, None, 5, 256, None, 0, None, p(rec.p), 3, p(res.p)) == F.E_GENERIC            # pattern
        assert find(codec.ctx, None, 5, 256, b"\n", 0, None, None, 3, p(res.p)) == F.E_GENERIC               # dRecords with capacity > 0
        assert find(codec.ctx, None, 5, 256, b"\n", 0, None, p(rec.p), 3, p(res.p)) == F.E_PARAM             # delim
        assert find(codec.ctx, None, 5, -1, b"\n", 0, None, p(rec.p), 3, p(res.p)) == F.E_PARAM
        assert find(codec.ctx, None, 5, 10, b"\n", 0, None, p(rec.p), 3, p(res.p)) == F.E_PARAM              # patternSize 0
        assert find(codec.ctx, None, 5, 10, b"a" * 257, 257, None, p(rec.p), 3, p(res.p)) == F.E_PARAM       # patternSize 257
        assert find(codec.ctx, None, 5, 10, b"a\nb", 3, None, p(rec.p), 3, p(res.p)) == F.E_PARAM            # a delimiter in the pattern
        assert find(codec.ctx, None, 5, 10, b"ab", 2, None, p(rec.p), 3, p(res.p)) == F.E_SRC_SIZE           # a NULL source
        codec.sync()
        for dev in (rec, res):
            v, ok = down(dev)
            assert ok and (v == CANARY).all()
        assert find(codec.ctx, p(src.p), 63, 10, b"ab", 2, None, p(rec.p), 8, p(res.p)) == 0                 # and the call they all refuse
        codec.sync()
        assert down(res, np.uint64)[0].tolist() == [21, 8, 21, 63] and down(rec, np.uint64)[0].tolist() == list(range(8))
    finally:
        for dev in (src, rec, res):
            dev.free()


def test_the_python_method(L, H, codec):
    from _hip import Dev
    from _resident import down
    data = S.text_lines(TILE + 500, seed=2)
    records, matches = F.find(data, b"zz")
    src, rec, res = Dev(H, len(data), data), Dev(H, 8 * max(len(records), 1)), Dev(H, 32)
    try:
        codec.find_records_device(src.p, len(data), b"zz", rec.p, len(records), res.p)
        codec.sync()
        assert down(res, np.uint64)[0].tolist() == [len(records), len(records), matches, len(data)]
        assert down(rec, np.uint64)[0][:len(records)].tolist() == records
        with pytest.raises(RuntimeError):
            codec.find_records_device(src.p, len(data), b"z\nz", rec.p, len(records), res.p)
    finally:
        for dev in (src, rec, res):
            dev.free()
