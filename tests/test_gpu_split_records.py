"""The record splitter on the device (zsmi_countRecordsDevice, zsmi_splitRecordsDevice) against the host call and the Python statement of
the rule (tests/_split.py): every host input; buffers that end on and around a lane's 16 bytes, a 4096-byte step and a 16384-byte tile,
with delimiters on both sides of each border; slices borrowed at odd offsets of a buffer full of delimiters; long records cut into many
pieces; chains of tens of thousands of frames; the piece counts around a scan tile with tight and loose maxPieces; maxPieces one short;
a NULL dFirstRecord; the host checks that need a context; and the pipeline from text in device memory to lines read back by number.
Every array is exactly as long as the header sizes it, between canaries.  Nothing depends on a wait inside the calls: the helper
synchronises before it reads back."""
import ctypes
import numpy as np
import pytest
import _split as S, _seekable_resident as SR
from _hip import hip_of, Dev
from _resident import down

pytestmark = pytest.mark.gpu
CASES = S.cases()
TOO_SMALL = (1 << 64) - S.E_TOO_SMALL


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


# ------------------------------------------------------------------ 1. parity with the host call
@pytest.mark.parametrize("name", sorted(CASES))
def test_host_inputs(L, H, codec, name):
    data, delim, T, M = CASES[name]
    d, want = S.device(L, H, codec, data, delim, T, M)
    S.same_as_host(L, d, want, data, delim, T, M)


@pytest.mark.parametrize("size", (0, 1, 15, 16, 17, 4095, 4096, 4097, 16383, 16384, 16385, 3 * 16384 + 5))
def test_borders(L, H, codec, size):
    for last in (True, False):
        data = S.border_buffer(size, last)
        for T, M in ((0, 1 << 16), (5000, 6000), (3, 1000)):
            d, want = S.device(L, H, codec, data, 10, T, M)
            S.same_as_host(L, d, want, data, 10, T, M)


@pytest.mark.parametrize("offset", (1, 3, 7, 13))
def test_borrowed_slices(L, H, codec, offset):
    """every byte outside the slice is the delimiter: a kernel that looks outside counts wrong"""
    for size in (1, 16, 4097, 16384, 16385, 2 * 16384 + 100):
        for last in (True, False):
            data = S.border_buffer(size, last)
            d, want = S.device(L, H, codec, data, 10, 300, 4000, offset=offset)
            S.same_as_host(L, d, want, data, 10, 300, 4000)


# ------------------------------------------------------------------ 2. long records, chains, the piece counts around a scan tile
def test_long_records(L, H, codec):
    for data, T, M, pieces in ((b"r" * 50000, 0, 1000, 50), (b"q\n" + b"r" * 49997 + b"\n", 900, 1000, 51), (b"r" * (1 << 20), 0, 64, 16384), (b"r" * (1 << 20), 64, 64, 16384)):
        d, want = S.device(L, H, codec, data, 10, T, M)
        assert want.pieces == pieces
        S.same_as_host(L, d, want, data, 10, T, M)


@pytest.mark.parametrize("T,frames", ((1, 70000), (3, 23334)))
def test_chains(L, H, codec, T, frames):
    """70000 one-byte records: 17 rounds of pointer doubling"""
    data = b"\n" * 70000
    d, want = S.device(L, H, codec, data, 10, T, 1 << 16)
    assert want.n == frames and want.pieces == 70000
    S.same_as_host(L, d, want, data, 10, T, 1 << 16)


@pytest.mark.parametrize("pieces", (1023, 1024, 1025))
def test_piece_counts_and_room(L, H, codec, pieces):
    data = S.lines(pieces, pieces, 20)
    for mp in (pieces, pieces + 1, 4 * pieces):
        d, want = S.device(L, H, codec, data, 10, 50, 1 << 16, max_pieces=mp)
        assert want.pieces == pieces
        S.same_as_host(L, d, want, data, 10, 50, 1 << 16)


# ------------------------------------------------------------------ 3. overflow, the other forms, the host checks
@pytest.mark.parametrize("name", ["random_T1000", "random_T64_M256", "no_delimiter_3001", "all_delimiters_5000_T7", "one_other_byte", "cut_record_shares_its_last_piece"])
def test_max_pieces_one_short(L, H, codec, name):
    data, delim, T, M = CASES[name]
    want = S.Split(data, delim, T, M)
    d, _ = S.device(L, H, codec, data, delim, T, M, max_pieces=want.pieces - 1)
    assert d.rc == 0 and d.result == [TOO_SMALL, want.records, want.pieces]
    assert d.untouched, "a list was written though the pieces do not fit"


def test_overflow_of_the_long_records_and_the_chain(L, H, codec):
    for data, T, M in ((b"r" * (1 << 20), 0, 64), (b"\n" * 70000, 3, 1 << 16), (S.border_buffer(3 * 16384 + 5, False), 3, 1000)):
        want = S.Split(data, 10, T, M)
        for mp in (want.pieces - 1, want.pieces // 2, 0):
            d, _ = S.device(L, H, codec, data, 10, T, M, max_pieces=mp)
            assert d.rc == 0 and d.result == [TOO_SMALL, want.records, want.pieces] and d.untouched


@pytest.mark.parametrize("name", ["random_T1000", "T0", "empty", "cut_record_shares_its_last_piece"])
def test_null_first_record(L, H, codec, name):
    data, delim, T, M = CASES[name]
    d, want = S.device(L, H, codec, data, delim, T, M, want_first=False)
    S.same_as_host(L, d, want, data, delim, T, M, want_first=False)


def test_host_checks_in_order(L, H, codec):
    """each refusal with every later one present too; a refused call queues nothing and writes nothing"""
    p = ctypes.c_void_p
    out = Dev(H, 64)
    GiB = 1 << 30

    def split(src, size, delim, T, M, mp, fs, res):
        return L.zsmi_splitRecordsDevice(codec.ctx, src, size, delim, T, M, mp, fs, None, res)
    try:
        o = p(out.p)
        assert L.zsmi_splitRecordsDevice(None, None, 5, -1, 9, 0, 0xFFFFFFFF, None, None, None) == S.E_INIT
        assert split(None, 5, -1, 9, 0, 0xFFFFFFFF, None, None) == S.E_PARAM and split(None, 5, 256, 9, 0, 0xFFFFFFFF, None, None) == S.E_PARAM
        assert split(None, 5, 10, 9, 0, 0xFFFFFFFF, None, None) == S.E_PARAM and split(None, 5, 10, 0, GiB + 1, 0xFFFFFFFF, None, None) == S.E_PARAM
        assert split(None, 5, 10, 9, 8, 0xFFFFFFFF, None, None) == S.E_PARAM
        assert split(None, 5, 10, 8, 8, 0x80000001, None, None) == S.E_PARAM
        assert split(None, 5, 10, 8, 8, 4, None, None) == S.E_SRC_SIZE
        assert split(o, 5, 10, 8, 8, 4, None, None) == S.E_GENERIC and split(o, 5, 10, 8, 8, 4, o, None) == S.E_GENERIC
        assert split(o, 5, 10, 8, 8, 4, None, o) == S.E_GENERIC
        assert L.zsmi_countRecordsDevice(None, None, 5, 256, None) == S.E_INIT
        assert L.zsmi_countRecordsDevice(codec.ctx, None, 5, 256, None) == S.E_PARAM
        assert L.zsmi_countRecordsDevice(codec.ctx, None, 5, 10, None) == S.E_SRC_SIZE
        assert L.zsmi_countRecordsDevice(codec.ctx, o, 5, 10, None) == S.E_GENERIC
        codec.sync()
        _, ok = down(out)
        assert ok and (np.frombuffer(out.all(), dtype=np.uint8) == 0xA5).all()
    finally:
        out.free()


# ------------------------------------------------------------------ 4. end to end: text in device memory -> a record archive -> lines by number
def test_text_to_archive_to_lines(L, H, codec):
    from zstandard_amd import BatchCodec
    text = S.text_lines(256 << 10)
    T, M = 4096, 65536
    want = S.Split(text, 10, T, M)
    lines = text.splitlines(True)
    assert len(lines) == want.records
    p = ctypes.c_void_p
    src, cnt, res = Dev(H, len(text), text), Dev(H, 8), Dev(H, 24)
    held = [src, cnt, res]
    try:
        codec.count_records_device(src.p, len(text), cnt.p)
        codec.sync()                                                               # read back 8 bytes
        records = int(down(cnt, np.uint64)[0][0])
        assert records == want.records
        mp = BatchCodec.split_pieces_bound(records, len(text), M)
        fs, fr = Dev(H, 4 * mp), Dev(H, 8 * (mp + 1))
        held += [fs, fr]
        codec.split_records_device(src.p, len(text), mp, fs.p, fr.p, res.p, target_size=T, max_frame_size=M)
        codec.sync()                                                               # read back dResult: n is the compress call's host argument
        result, ok = down(res, np.uint64)
        assert ok and result.tolist() == [want.n, want.records, want.pieces]
        n = int(result[0])
        bound = codec.seekable_frames_resident_bound(len(text), n, True)
        arc, size = Dev(H, bound), Dev(H, 8)
        held += [arc, size]
        codec.compress_seekable_frames_resident(src.p, len(text), fs.p, n, M, arc.p, bound, size.p, level=3, checksum=True)
        codec.sync()
        m = int(down(size, np.uint64)[0][0])
        assert 0 < m <= bound, hex(m)
        archive = down(arc)[0][:m].tobytes()
        # the archive of the host-array call given the host call's sizes
        _, host_sizes, host_first, _, _ = S.host(L, text, 10, T, M)
        cap = codec.seekable_frames_bound(host_sizes, True)
        arc2, size2 = Dev(H, cap), Dev(H, 8)
        held += [arc2, size2]
        codec.compress_seekable_frames_device(src.p, host_sizes, arc2.p, cap, size2.p, level=3, checksum=True)
        codec.sync()
        m2 = int(down(size2, np.uint64)[0][0])
        assert m2 == m and down(arc2)[0][:m2].tobytes() == archive
        # lines by number: the firstRecord lookup, then one resident read
        first = down(fr, np.uint64)[0][:n + 1]
        assert first.tolist() == host_first
        rng = np.random.default_rng(8)
        picks = [0, records - 1] + [int(v) for v in rng.integers(0, records, 62)]
        frames = []
        for r in picks:
            i = int(np.searchsorted(first, r))
            frames.append(i if first[i] == r else i - 1)
        assert frames == [want.frame_of(r) for r in picks]
        sk = codec.open_seekable_device(arc.p, m)
        try:
            rd = SR.read(L, H, codec, sk.handle, frames, 1, sum(host_sizes[f] for f in frames))
            assert rd.rc == 0 and not rd.status.any()
            for k, (r, f) in enumerate(zip(picks, frames)):
                got = rd.out(k, host_sizes[f])
                assert got.splitlines(True)[r - int(first[f])] == lines[r], (k, r, f)
        finally:
            codec.sync()
            sk.close()
    finally:
        for d in held:
            d.free()
