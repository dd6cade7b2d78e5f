"""Seekable archives on the GPU (zsmi_compressSeekable*, zsmi_decompressSeekable*).  Every archive must equal oracle E's frames of the
slices followed by the table tests/_seekable.py writes, byte for byte (levels 1 and 3, frame sizes from 1 byte to more than the input,
checksums on and off, an empty input, several corpus classes); it must decode to its input under oracle D, under zsmi_decompress (the
archive as one item) and under libzstd.  Range reads through both forms must equal slices of the input; only the frames that overlap a
range are decoded (a damaged frame fails exactly the ranges that touch it, the earliest damaged frame decides the code); archives of
libzstd's frames (content checksums, more than 16 blocks) read correctly; the device forms write nothing outside their output."""
import ctypes
import numpy as np
import pytest
import _corpus as C
import _data as D
import _oracle as O
import _seekable as S
from _hip import hip_of, Dev, CANARY, PAD

pytestmark = pytest.mark.gpu
E_PREFIX, E_CORRUPT, E_CHECKSUM, E_OUT_OF_BOUND = 10, 20, 22, 42


@pytest.fixture(scope="module")
def L():
    from zstandard_amd import _lib
    return _lib.lib()


@pytest.fixture(scope="module")
def hip():
    return hip_of()


@pytest.fixture(scope="module")
def codec():
    from zstandard_amd import BatchCodec
    return BatchCodec(0)


def compress(L, data: bytes, level, frame_size, checksum) -> bytes:
    cap = L.zsmi_seekableBound(len(data), frame_size, checksum)
    out = ctypes.create_string_buffer(max(cap, 1))
    r = L.zsmi_compressSeekable(out, cap, data, len(data), level, frame_size, checksum)
    assert not L.zsmi_isError(r), L.zsmi_getErrorName(r)
    return out.raw[:r]


def read(L, arc, offset, length):
    """one-shot range read: bytes, or the error code"""
    out = ctypes.create_string_buffer(max(length, 1))
    r = L.zsmi_decompressSeekable(out, length, arc, len(arc), offset)
    return int(L.zsmi_getErrorCode(r)) if L.zsmi_isError(r) else out.raw[:r]


def read_device(L, H, codec, arc, offset, length, cap=None):
    """device range read into a canary-guarded buffer: (bytes or the code, written); checks that nothing outside [dDst, dDst + written) changed"""
    cap = length if cap is None else cap
    src = Dev(H, len(arc), arc)
    dst = Dev(H, max(cap, 1))
    st = Dev(H, 4)
    written = ctypes.c_uint64(0)
    try:
        rc = L.zsmi_decompressSeekableDevice(codec.ctx, ctypes.c_void_p(src.p), len(arc), offset, length, ctypes.c_void_p(dst.p), ctypes.byref(written),
                                             ctypes.c_void_p(st.p))
        if rc:
            return rc, 0
        codec.sync()
        w = written.value
        buf = dst.all()
        assert buf[:PAD] == bytes([CANARY]) * PAD and buf[PAD + w:] == bytes([CANARY]) * (len(buf) - PAD - w), "device read wrote outside its range"
        status = int.from_bytes(st.all()[PAD:PAD + 4], "little")
        return (status if status else buf[PAD:PAD + w]), w
    finally:
        for b in (src, dst, st):
            b.free()


def compress_device(L, H, codec, data, level, frame_size, checksum):
    """device compress into a canary-guarded buffer of exactly the bound: the archive, checked against the bound and the canaries"""
    bound = L.zsmi_seekableBound(len(data), frame_size, checksum)
    src = Dev(H, max(len(data), 1), data)
    dst = Dev(H, bound)
    sz = Dev(H, 8)
    try:
        rc = L.zsmi_compressSeekableDevice(codec.ctx, ctypes.c_void_p(src.p), len(data), ctypes.c_void_p(dst.p), bound, ctypes.c_void_p(sz.p),
                                           level, frame_size, checksum)
        assert rc == 0, rc
        codec.sync()
        size = int.from_bytes(sz.all()[PAD:PAD + 8], "little")
        assert size <= bound
        buf = dst.all()
        assert buf[:PAD] == bytes([CANARY]) * PAD and buf[PAD + bound:] == bytes([CANARY]) * PAD, "device compress wrote outside dDst + bound"
        return buf[PAD:PAD + size]
    finally:
        for b in (src, dst, sz):
            b.free()


# ------------------------------------------------------------------ byte identity and compatibility
def check_compatible(L, arc, data):
    assert O.decompress(arc, len(data)) == data, "oracle D"
    out = ctypes.create_string_buffer(max(len(data), 1))
    r = L.zsmi_decompress(out, len(data), arc, len(arc))
    assert r == len(data) and out.raw[:r] == data, "zsmi_decompress"
    if O.libzstd():
        assert O.zstd_decompress(arc, len(data)) == data, "libzstd"


@pytest.mark.parametrize("level", [1, 3])
def test_archive_equals_oracle_frames_and_python_table(L, level):
    big = D.zipf_log(1300000).tobytes()
    for frame_size, data in ((1, big[:1500]), (4095, big[:70000]), (65536, big), (100000, big), (131072, big), (1 << 20, big),
                             (len(big), big), (len(big) + 7, big), (0, big[:200000])):
        for checksum in (1, 0):
            arc = compress(L, data, level, frame_size, checksum)
            assert arc == S.oracle_archive(data, frame_size, level, bool(checksum)), (frame_size, checksum)
            assert len(arc) <= L.zsmi_seekableBound(len(data), frame_size, checksum)
        check_compatible(L, arc, data)


def test_empty_input(L, hip, codec):
    for ck in (0, 1):
        arc = compress(L, b"", 3, 0, ck)
        assert arc == S.table([], bool(ck)) and len(arc) == 17
        assert compress_device(L, hip, codec, b"", 3, 0, ck) == arc
        assert L.zsmi_seekableNumFrames(arc, 17) == 0 and read(L, arc, 0, 100) == b""


def test_corpus_classes(L, hip, codec):
    for gen in (C.pysrc, C.json_records, C.binary_table, C.repetitive):
        data = gen(400000)
        arc = compress(L, data, 3, 0, 1)
        assert arc == S.oracle_archive(data, 0, 3, True), gen.__name__
        assert compress_device(L, hip, codec, data, 3, 0, 1) == arc, gen.__name__
        check_compatible(L, arc, data)


def test_device_compress_matches_one_shot(L, hip, codec):
    data = D.zipf_log(900000, seed_lo=0x99).tobytes()
    for level, fs, ck in ((3, 0, 1), (1, 100000, 0), (3, 4095, 1)):
        assert compress_device(L, hip, codec, data, level, fs, ck) == compress(L, data, level, fs, ck)
    # refused on the host, nothing queued: capacity under the bound, bad frame size
    bound = L.zsmi_seekableBound(len(data), 0, 1)
    rc = L.zsmi_compressSeekableDevice(codec.ctx, None, len(data), None, bound - 1, None, 3, 0, 1)
    assert rc == 70
    assert L.zsmi_compressSeekableDevice(codec.ctx, None, len(data), None, 1 << 40, None, 3, (1 << 30) + 1, 1) == E_OUT_OF_BOUND


# ------------------------------------------------------------------ range reads
def ranges(data_len, f):
    r = [(0, data_len), (0, 0), (5, 0), (0, 1), (1, 10), (f - 1, 2), (f, 1), (f + 1, 3), (f - 1, f + 2), (2 * f - 1, 1), (3 * f + 17, 4096),
         (f // 2, 5 * f), (100, data_len), (data_len - 10, 100), (data_len - 1, 1), (data_len, 10), (data_len - f - 1, f + 1), (f, f), (f, 3 * f)]
    return [(o, n) for o, n in r if 0 <= o <= data_len]


def test_range_reads_both_forms(L, hip, codec):
    data = D.zipf_log(1000000, seed_lo=0x44).tobytes()
    for fs, ck in ((65536, 1), (100000, 0), (4095, 1)):
        arc = compress(L, data, 3, fs, ck)
        for off, n in ranges(len(data), fs):
            want = data[off:off + n]
            assert read(L, arc, off, n) == want, (fs, off, n)
            got, w = read_device(L, hip, codec, arc, off, n)
            assert got == want and w == len(want), (fs, off, n)
        assert read(L, arc, len(data) + 1, 1) == E_OUT_OF_BOUND
        assert read_device(L, hip, codec, arc, len(data) + 1, 1)[0] == E_OUT_OF_BOUND


def damaged(arc, frame, at, xor):
    co = S.parse(arc)[0]
    pos = sum(r[0] for r in co[:frame]) + at
    return arc[:pos] + bytes([arc[pos] ^ xor]) + arc[pos + 1:]


def test_only_overlapping_frames_are_decoded(L, hip, codec):
    data = D.zipf_log(640000, seed_lo=0x55).tobytes()
    f = 65536
    arc = compress(L, data, 3, f, 1)
    rows, _ = S.parse(arc)
    bad_magic = damaged(arc, 3, 0, 0xFF)                                   # frame 3: content [3f, 4f)
    bad_payload = damaged(arc, 6, rows[6][0] // 2, 0x10)                   # frame 6: content [6f, 7f)
    both = damaged(bad_magic, 6, rows[6][0] // 2, 0x10)
    for off, n in ((0, 3 * f), (3 * f - 1, 1), (4 * f, 2 * f), (7 * f, len(data)), (2 * f + 5, 100), (4 * f, 1)):
        for a in (bad_magic, bad_payload):
            assert read(L, a, off, n) == data[off:off + n], (off, n)
            assert read_device(L, hip, codec, a, off, n)[0] == data[off:off + n], (off, n)
    for off, n in ((3 * f, 1), (3 * f - 1, 2), (4 * f - 1, 1), (0, len(data)), (3 * f + 100, 4096)):
        assert read(L, bad_magic, off, n) == E_PREFIX, (off, n)
        assert read_device(L, hip, codec, bad_magic, off, n)[0] == E_PREFIX, (off, n)
    for off, n in ((6 * f, 1), (7 * f - 1, 1), (5 * f, 3 * f), (6 * f + 100, 4096)):
        assert read(L, bad_payload, off, n) in (E_CORRUPT, E_CHECKSUM), (off, n)
        assert read_device(L, hip, codec, bad_payload, off, n)[0] in (E_CORRUPT, E_CHECKSUM), (off, n)
    # two damaged frames: the earlier one decides, whichever the failing kernel
    assert read(L, both, 0, len(data)) == E_PREFIX and read_device(L, hip, codec, both, 0, len(data))[0] == E_PREFIX
    assert read(L, both, 4 * f, len(data)) in (E_CORRUPT, E_CHECKSUM)
    # a frame whose entry says one byte less than it holds, and one whose checksum entry is wrong
    t0 = len(arc) - (17 + 12 * len(rows))
    short = arc[:t0] + S.table([(c, d - (i == 2), h) for i, (c, d, h) in enumerate(rows)], True)
    assert read(L, short, 2 * f, 10) == E_CORRUPT and read(L, short, 0, 10) == data[:10]
    wrong = arc[:t0] + S.table([(c, d, h ^ (i == 4)) for i, (c, d, h) in enumerate(rows)], True)
    assert read(L, wrong, 4 * f, 10) == E_CHECKSUM and read_device(L, hip, codec, wrong, 4 * f, 10)[0] == E_CHECKSUM
    assert read(L, wrong, 5 * f, 10) == data[5 * f:5 * f + 10]


# ------------------------------------------------------------------ archives of libzstd's frames
def test_foreign_archives(L, hip, codec):
    if O.libzstd() is None:
        pytest.skip("libzstd is not on this machine")
    text = C.json_records(2800000)
    parts = [text[:70000], text[70000:70001], text[70001:200000], text[200000:2700000], b"", text[:5000]]   # part 3: > 16 blocks (general kernel)
    data = b"".join(parts)
    for ck_table in (True, False):
        arc = S.zstd_archive(parts, ck_table, frame_checksums=(0, 2, 3))
        for off, n in ((0, len(data)), (69999, 3), (150000, 100000), (len(data) - 4999, 4999), (300000, 4096)):
            assert read(L, arc, off, n) == data[off:off + n], (ck_table, off, n)
            assert read_device(L, hip, codec, arc, off, n)[0] == data[off:off + n], (ck_table, off, n)
        check_compatible(L, arc, data)
    bad = damaged(S.zstd_archive(parts, False, frame_checksums=(2,)), 2, 5000, 0x01)     # libzstd's own content checksum catches it
    assert read(L, bad, 80000, 10) in (E_CORRUPT, E_CHECKSUM) and read(L, bad, 0, 10) == data[:10]


# ------------------------------------------------------------------ Python surface
def test_python_api(codec):
    from zstandard_amd import SeekableArchive, ZstdCompressor
    data = D.zipf_log(300000, seed_lo=0x66).tobytes()
    arc = ZstdCompressor(3).compress_seekable(data, frame_size=50000)
    assert arc == S.oracle_archive(data, 50000, 3, True)
    assert ZstdCompressor(1).compress_seekable(data, checksum=False) == S.oracle_archive(data, 0, 1, False)
    a = SeekableArchive(arc)
    assert a.num_frames == 6 and a.content_size == len(data)
    assert a.read() == data and a.read(49999, 3) == data[49999:50002] and a.read(299990) == data[299990:]
    with pytest.raises(RuntimeError, match="Unknown frame descriptor"):
        SeekableArchive(damaged(arc, 1, 0, 0xFF)).read(50000, 1)
    with pytest.raises(RuntimeError):
        ZstdCompressor(3, dictionary=b"abc" * 100).compress_seekable(data)
    H = hip_of()
    bound = codec.seekable_bound(len(data), 50000, True)
    src, dst, size = Dev(H, len(data), data), Dev(H, bound), Dev(H, 8)
    codec.compress_seekable_device(src.p, len(data), dst.p, bound, size.p, 3, 50000, True)
    codec.sync()
    n = int.from_bytes(size.all()[PAD:PAD + 8], "little")
    assert dst.all()[PAD:PAD + n] == arc
    out, st = Dev(H, 1000), Dev(H, 4)
    assert codec.decompress_seekable_device(dst.p, n, 120000, 1000, out.p, st.p) == 1000
    codec.sync()
    assert st.all()[PAD:PAD + 4] == bytes(4) and out.all()[PAD:PAD + 1000] == data[120000:121000]
    with pytest.raises(RuntimeError, match="Parameter is out of bound"):
        codec.decompress_seekable_device(dst.p, n, len(data) + 1, 1, out.p, st.p)
    for b in (src, dst, size, out, st):
        b.free()
