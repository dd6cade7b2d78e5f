"""The seek table on the host (no GPU): zsmi_seekableNumFrames / ContentSize / FrameInfo on archives built in Python (tests/_seekable.py)
from oracle E's frames and from upstream libzstd's, every rejection rule with its code, the footer's unused bits, the parameter checks of
the compress calls and the range checks of the read, which all answer before anything runs on a device."""
import ctypes, struct
import pytest
import _data as D
import _oracle as O
import _seekable as S

E_PREFIX, E_CORRUPT, E_CHECKSUM, E_OUT_OF_BOUND, E_INDEX, E_IO = 10, 20, 22, 42, 100, 102


@pytest.fixture(scope="module")
def L():
    from zstandard_amd import _lib
    _lib.build()
    return _lib.lib()


def code(L, r):
    return int(L.zsmi_getErrorCode(r)) if L.zsmi_isError(r) else 0


def info(L, arc, i):
    co, do, cs, ds = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint32(), ctypes.c_uint32()
    rc = L.zsmi_seekableFrameInfo(arc, len(arc), i, ctypes.byref(co), ctypes.byref(do), ctypes.byref(cs), ctypes.byref(ds))
    return rc, (co.value, do.value, cs.value, ds.value)


def archives():
    data = D.zipf_log(300000).tobytes()
    out = {"oracle_64k_ck": (S.oracle_archive(data, 0, 3, True), S.slices(data)),
           "oracle_100000_nock": (S.oracle_archive(data, 100000, 1, False), S.slices(data, 100000)),
           "oracle_1": (S.oracle_archive(data[:40], 1, 3, True), S.slices(data[:40], 1)),
           "empty": (S.table([], True), [])}
    parts = S.slices(data, 70000)
    z = S.zstd_archive(parts, True, frame_checksums=(1, 3))
    if z is not None:
        out["libzstd_ck"] = (z, parts)
    return out


def test_error_names(L):
    assert L.zsmi_getErrorName((1 << 64) - E_INDEX) == b"Frame index is too large"
    assert L.zsmi_getErrorName((1 << 64) - E_IO) == b"An I/O error occurred when reading/seeking"


@pytest.mark.parametrize("name", ["oracle_64k_ck", "oracle_100000_nock", "oracle_1", "empty", "libzstd_ck"])
def test_counts_and_frame_info(L, name):
    arcs = archives()
    if name not in arcs:
        pytest.skip("libzstd 1.4.8 is not on this machine")
    arc, parts = arcs[name]
    rows, _ = S.parse(arc)
    assert L.zsmi_seekableNumFrames(arc, len(arc)) == len(parts) == len(rows)
    assert L.zsmi_seekableContentSize(arc, len(arc)) == sum(len(p) for p in parts)
    co = do = 0
    for i, (c, d, _) in enumerate(rows):
        assert info(L, arc, i) == (0, (co, do, c, d)), i
        assert d == len(parts[i])
        co += c; do += d
    assert info(L, arc, len(rows))[0] == E_INDEX
    assert info(L, arc, 0xFFFFFFFF)[0] == E_INDEX


def rebuilt(arc, rows=None, ck=None, descriptor=None, lead=b""):
    """the archive's frames (with `lead` in front) and a table written again from `rows`"""
    r0, c0 = S.parse(arc)
    ck = c0 if ck is None else ck
    tsize = 17 + len(r0) * (12 if c0 else 8)
    return lead + arc[:len(arc) - tsize] + S.table(r0 if rows is None else rows, ck, descriptor)


def fsize_says(t, value):
    return t[:4] + struct.pack("<I", value) + t[8:]


def bad_archives():
    data = D.zipf_log(200000, seed_lo=0x77).tobytes()
    arc = S.oracle_archive(data, 50000, 3, True)
    rows, _ = S.parse(arc)
    n = len(rows)
    tsize = 17 + n * 12
    t0 = len(arc) - tsize
    cases = {
        "footer_magic": (arc[:-4] + struct.pack("<I", S.SEEKABLE_MAGIC ^ 1), E_PREFIX),
        "skippable_magic": (arc[:t0] + struct.pack("<I", 0x184D2A50) + arc[t0 + 4:], E_PREFIX),
        "frame_size_field": (arc[:t0 + 4] + struct.pack("<I", n * 12 + 10) + arc[t0 + 8:], E_CORRUPT),
        "frame_count_disagrees": (arc[:t0] + fsize_says(S.table(rows[:-1], True), n * 12 + 9), E_CORRUPT),      # n - 1 entries, Frame_Size of n
        "sizes_short": (rebuilt(arc, lead=b"\x00"), E_CORRUPT),
        "sizes_long": (rebuilt(arc, rows=[(rows[0][0] + 1,) + rows[0][1:]] + rows[1:]), E_CORRUPT),
        "csize_zero": (rebuilt(arc, rows=rows[:-1] + [(0, 5, 0)], lead=bytes(rows[-1][0])), E_CORRUPT),
        "dsize_over_1gib": (rebuilt(arc, rows=rows[:-1] + [(rows[-1][0], (1 << 30) + 1, 0)]), E_CORRUPT),
        "too_many_frames": (arc[:-9] + struct.pack("<IBI", S.MAX_FRAMES + 1, 0x80, S.SEEKABLE_MAGIC), E_INDEX),
        "table_longer_than_archive": (arc[-(17 + 12 * 2):][:-9] + struct.pack("<IBI", n, 0x80, S.SEEKABLE_MAGIC), E_CORRUPT),
        "short": (arc[-8:], E_PREFIX),
        "plain_frame": (O.compress(data[:1000]), E_PREFIX),
    }
    for bit in range(2, 7):
        cases[f"reserved_bit{bit}"] = (arc[:-5] + bytes([0x80 | (1 << bit)]) + arc[-4:], E_CORRUPT)
    return arc, cases


def test_rejections(L):
    """each rule with its code, from every host call that reads a table; the read refuses before a device is touched"""
    from zstandard_amd import SeekableArchive
    _, cases = bad_archives()
    dst = ctypes.create_string_buffer(1 << 16)
    for name, (arc, want) in cases.items():
        assert code(L, L.zsmi_seekableNumFrames(arc, len(arc))) == want, name
        assert code(L, L.zsmi_seekableContentSize(arc, len(arc))) == want, name
        assert info(L, arc, 0)[0] == want, name
        assert code(L, L.zsmi_decompressSeekable(dst, 1 << 16, arc, len(arc), 0)) == want, name
        with pytest.raises(RuntimeError) as e:
            SeekableArchive(arc)
        assert str(e.value) == L.zsmi_getErrorName((1 << 64) - want).decode(), name


def test_unused_descriptor_bits_are_ignored(L):
    arc, _ = bad_archives()
    rows, _ = S.parse(arc)
    for low in (1, 2, 3):
        a = arc[:-5] + bytes([0x80 | low]) + arc[-4:]
        assert L.zsmi_seekableNumFrames(a, len(a)) == len(rows)
        assert L.zsmi_seekableContentSize(a, len(a)) == sum(r[1] for r in rows)
    a = rebuilt(arc, ck=False, descriptor=0x03)
    assert L.zsmi_seekableNumFrames(a, len(a)) == len(rows) and info(L, a, 1)[1][3] == rows[1][1]


def test_range_checks_before_the_device(L):
    arc, _ = bad_archives()
    content = L.zsmi_seekableContentSize(arc, len(arc))
    dst = ctypes.create_string_buffer(16)
    assert code(L, L.zsmi_decompressSeekable(dst, 16, arc, len(arc), content + 1)) == E_OUT_OF_BOUND
    assert L.zsmi_decompressSeekable(dst, 16, arc, len(arc), content) == 0               # offset == content size: 0 bytes
    assert L.zsmi_decompressSeekable(dst, 0, arc, len(arc), 5) == 0                      # length 0
    empty = S.table([], False)
    assert L.zsmi_decompressSeekable(dst, 16, empty, len(empty), 0) == 0


def test_bound_and_compress_parameters(L):
    bound = lambda n: int(L.zsmi_compressBound(n))
    assert L.zsmi_seekableBound(0, 0, 1) == 17 and L.zsmi_seekableBound(0, 0, 0) == 17
    assert L.zsmi_seekableBound(200000, 0, 1) == 3 * bound(65536) + bound(200000 - 3 * 65536) + 17 + 4 * 12
    assert L.zsmi_seekableBound(200000, 100000, 0) == 2 * bound(100000) + 17 + 2 * 8
    assert L.zsmi_seekableBound(1 << 30, 1 << 30, 0) == bound(1 << 30) + 25
    assert code(L, L.zsmi_seekableBound(100, (1 << 30) + 1, 0)) == E_OUT_OF_BOUND
    assert code(L, L.zsmi_seekableBound(S.MAX_FRAMES + 1, 1, 0)) == E_INDEX
    assert L.zsmi_seekableBound(S.MAX_FRAMES, 1, 0) == S.MAX_FRAMES * (bound(1) + 8) + 17
    dst = ctypes.create_string_buffer(64)
    src = b"x" * 100
    assert code(L, L.zsmi_compressSeekable(dst, 64, src, 100, 3, (1 << 30) + 1, 1)) == E_OUT_OF_BOUND
    assert code(L, L.zsmi_compressSeekable(dst, 64, src, 100, 3, 0xFFFFFFFF, 0)) == E_OUT_OF_BOUND
    from zstandard_amd import ZstdCompressor
    with pytest.raises(RuntimeError, match="Parameter is out of bound"):
        ZstdCompressor().compress_seekable(src, frame_size=(1 << 30) + 1)


def test_python_archive_surface(L):
    from zstandard_amd import SeekableArchive
    arc, parts = archives()["oracle_100000_nock"]
    a = SeekableArchive(arc)
    rows, _ = S.parse(arc)
    assert a.num_frames == len(parts) and a.content_size == sum(map(len, parts))
    assert a.frame_info(1) == (rows[0][0], 100000, rows[1][0], rows[1][1])
    assert a.frame_info(-1) == a.frame_info(len(parts) - 1)
    with pytest.raises(RuntimeError, match="Frame index is too large"):
        a.frame_info(len(parts))
    with pytest.raises(RuntimeError, match="Parameter is out of bound"):
        a.read(a.content_size + 1, 1)
    assert a.read(a.content_size) == b"" and a.read(3, 0) == b""
