"""The record index on archives, on the device, against tests/_recindex.py and the splitter's own array: text split, compressed and given
its index frame without leaving the device or waiting in between (the resident calls are chained on the stream and synchronised once,
behind the last); the attached archive byte for byte the host attach's; the index loaded back, and rebuilt from the content in one
window and in three chained ones; lines read and found through the loaded array, with the find window over ALL frames, the index
frame's entry included; a handle with a DDict set; fixed-size frames, which are misaligned; 2 097 153 one-byte frames, where the
counts' scan takes its second level; damage - a count, the inner magic, a content frame inside a rebuild window; an archive without an
index; the host rebuild in many windows (a child process on the debug-hook library).  Every device array is exactly as long as the
header sizes it, between canaries."""
import ctypes, os, subprocess, sys
import numpy as np
import pytest
import _recindex as R, _split as S, _find as FD, _borders as BD, _seekable_resident as SR, _resident_cdict_set as RS
from _hip import hip_of, Dev, CANARY
from _resident import up, down

pytestmark = pytest.mark.gpu
p = ctypes.c_void_p
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


@pytest.fixture(scope="module")
def text():
    """about 1 MiB of seeded lines, three of them longer than any maxFrameSize used here"""
    body = S.text_lines(1 << 20, seed=33)
    cut = [len(body) // 5, len(body) // 2, 4 * len(body) // 5]
    cut = [body.index(b"\n", c) + 1 for c in cut]
    long_line = lambda k: bytes([97 + k]) * (9000 + 1000 * k) + b"\n"
    return body[:cut[0]] + long_line(0) + body[cut[0]:cut[1]] + long_line(1) + body[cut[1]:cut[2]] + long_line(2) + body[cut[2]:]


def words(dev, dtype=np.uint64):
    v, ok = down(dev, dtype)
    assert ok, "a guard word around a device array is gone"
    return v.copy()


def table_offsets(archive):
    """the frames' content offsets, from the archive's table"""
    _, _, _, rows = R.table_of(archive)
    return R.offsets_of([r[1] for r in rows])


class Opened:
    """an archive's bytes in device memory and a handle on them"""

    def __init__(self, H, codec, archive, ddict_set=None):
        self.dev = up(H, np.frombuffer(archive, dtype=np.uint8))
        assert H.hipDeviceSynchronize() == 0
        self.h = codec.open_seekable_device(self.dev.p, len(archive), ddict_set=ddict_set)
        self.N = self.h.num_frames

    def close(self, codec):
        codec.sync(); self.h.close(); self.dev.free()


def load(H, codec, o):
    """zsmi_seekableLoadRecordIndexResident -> (result words, the array: N + 1 entries, its canaries checked)"""
    first, res = Dev(H, 8 * (o.N + 1)), Dev(H, 32)
    assert H.hipDeviceSynchronize() == 0
    try:
        o.h.load_record_index_resident(first.p, res.p)
        codec.sync()
        return [int(v) for v in words(res)], words(first)
    finally:
        first.free(); res.free()


def rebuild(H, codec, o, windows, delim=10):
    """zsmi_seekableIndexRecordsResident over the windows, in order, chained on the stream and synchronised once -> ([result words a
    window], the array)"""
    bounds = [o.h.find_work_bound(a, c) for a, c in windows]
    first, work = Dev(H, 8 * (o.N + 1)), Dev(H, max(max(bounds), 1))
    res = [Dev(H, 32) for _ in windows]
    assert H.hipDeviceSynchronize() == 0
    try:
        for (a, c), r, b in zip(windows, res, bounds):
            o.h.index_records_resident(a, c, work.p, b, first.p, r.p, delimiter=bytes([delim]))
        codec.sync()
        assert (np.frombuffer(work.all(), dtype=np.uint8)[4096 + max(max(bounds), 1):] == CANARY).all(), "written behind dWork"
        return [[int(v) for v in words(r)] for r in res], words(first)
    finally:
        for d in [first, work] + res:
            d.free()


def write_and_attach(L, H, codec, text, T, M, want):
    """split -> compress -> attach, every array in device memory, nothing waited for until the end: (the plain archive, the attached one).
    The host knows the frame count from the reference alone."""
    n, mp = want.n, want.pieces
    bound = L.zsmi_seekableFramesResidentBound(len(text), n, 1)
    room = bound + 40 + 4 * n + 12
    d_sizes, d_first, d_res = Dev(H, 4 * mp), Dev(H, 8 * (mp + 1)), Dev(H, 24)
    plain, plain_size, dst, dst_size = Dev(H, bound), Dev(H, 8), Dev(H, room), Dev(H, 8)
    src = Dev(H, len(text), text)
    assert H.hipDeviceSynchronize() == 0
    try:
        codec.split_records_device(src.p, len(text), mp, d_sizes.p, d_first.p, d_res.p, b"\n", T, M)
        for d, cap, size in ((plain, bound, plain_size), (dst, room, dst_size)):
            assert L.zsmi_compressSeekableFramesResident(codec.ctx, p(src.p), len(text), p(d_sizes.p), n, M, p(d.p), cap, p(size.p), 3, 1) == 0
        codec.attach_record_index_resident(dst.p, room, dst_size.p, d_first.p, n)
        codec.sync()
        assert [int(v) for v in words(d_res)] == [n, want.records, want.pieces]
        a, b = int(words(plain_size)[0]), int(words(dst_size)[0])
        assert a <= bound and b == a + 40 + 4 * n + 12, (hex(a), hex(b))
        body = words(dst, np.uint8)
        assert (body[b:] == CANARY).all(), "written behind the attached archive's end"
        return words(plain, np.uint8)[:a].tobytes(), body[:b].tobytes()
    finally:
        for d in (d_sizes, d_first, d_res, plain, plain_size, dst, dst_size, src):
            d.free()


@pytest.mark.parametrize("T,M", ((0, 128), (4096, 4096)))
def test_end_to_end(L, H, codec, text, T, M):
    from zstandard_amd import SeekableArchive, api
    want = S.Split(text, 10, T, M)
    assert max(want.sizes) == M and want.pieces > want.records                       # records are cut
    plain, attached = write_and_attach(L, H, codec, text, T, M, want)
    extended = want.first_record + [want.records]
    # the attached archive is the host attach's, and the restatement's
    assert attached == api.attach_record_index(plain, want.first_record) == R.attached(plain, want.first_record, 10)
    offsets = table_offsets(attached)
    assert len(offsets) == want.n + 2 and int(offsets[-1]) == int(offsets[-2]) == len(text)
    rule = R.Index(text, 10, offsets)
    assert rule.first_record.tolist() == extended and rule.misaligned == 0
    o = Opened(H, codec, attached)
    try:
        assert o.N == want.n + 1
        result, loaded = load(H, codec, o)
        assert result == [0, want.records, 10, want.n] and loaded.tolist() == extended
        results, rebuilt = rebuild(H, codec, o, [(0, o.N)])
        assert results == [[0, want.records, 0, rule.delimiters]] and rebuilt.tolist() == extended
        a, b = o.N // 3, 2 * o.N // 3 + 1
        results, chained = rebuild(H, codec, o, [(0, a), (a, b - a), (b, o.N - b)])
        assert [r[0] for r in results] == [0, 0, 0] and sum(r[2] for r in results) == 0 and sum(r[3] for r in results) == rule.delimiters
        assert chained.tolist() == extended
    finally:
        o.close(codec)
    # lines through the loaded array; the find window spans all frames, the index frame's entry included
    lines = text.split(b"\n")[:-1]
    with_index, without = SeekableArchive(attached), SeekableArchive(plain)
    try:
        first = with_index.first_record()
        assert first.tolist() == extended and with_index.num_frames == want.n + 1
        assert without.first_record().tolist() == want.first_record                # no index frame: rebuilt from the content
        picks = [0, 1, want.records - 1, want.records // 2] + [text[:text.index(bytes([97 + k]) * 9000)].count(b"\n") for k in range(3)]
        assert with_index.read_records(first, picks) == [lines[r] + b"\n" for r in picks] == without.read_records(want.first_record, picks)
        for pattern in (b"qz", b"a" * 256, lines[5][3:12]):
            found = with_index.find_records(first, pattern)
            assert found == FD.find(text, pattern)[0] == without.find_records(want.first_record, pattern), pattern
        assert with_index.find_records_regex(first, b"^[a-f]+x.*z$") == without.find_records_regex(want.first_record, b"^[a-f]+x.*z$") == \
            api.find_records_regex(text, b"^[a-f]+x.*z$")
    finally:
        with_index.close(); without.close()


def test_a_handle_with_a_ddict_set(L, H, codec):
    """frames written with a CDict set and read back through a DDict set: load and rebuild decode with the dictionaries"""
    from zstandard_amd import api
    parts, index = SR.records()
    content, sizes = b"".join(parts), [len(c) for c in parts]
    cset, cds = RS.make_set(codec, 3)
    dset, dds = SR.ddict_set(codec)
    try:
        w = SR.write(L, H, codec, content, sizes, 3, 1, cset, index)
        assert w.rc == 0 and w.archive is not None
        want = R.Index(content, 10, R.offsets_of(sizes))
        attached = api.attach_record_index(w.archive, want.first_record)
        rule = R.Index(content, 10, table_offsets(attached))
        o = Opened(H, codec, attached, ddict_set=dset)
        try:
            result, loaded = load(H, codec, o)
            assert result == [0, want.records, 10, len(sizes)] and loaded.tolist() == rule.first_record.tolist()
            results, rebuilt = rebuild(H, codec, o, [(0, o.N)])
            assert results == [[0, rule.records, rule.misaligned, rule.delimiters]] and rebuilt.tolist() == rule.first_record.tolist()
        finally:
            o.close(codec)
    finally:
        codec.sync(); cset.close(); dset.close()
        for d in list(set(cds)) + dds:
            d.close()


def test_fixed_size_frames_are_misaligned(L, H, codec, text):
    from zstandard_amd import SeekableArchive
    data = text[:300000]
    bound = codec.seekable_bound(len(data), 4096, True)
    src, dst, size = up(H, np.frombuffer(data, dtype=np.uint8)), Dev(H, bound), Dev(H, 8)
    assert H.hipDeviceSynchronize() == 0
    try:
        codec.compress_seekable_device(src.p, len(data), dst.p, bound, size.p, 3, 4096, True)
        codec.sync()
        archive = words(dst, np.uint8)[:int(words(size)[0])].tobytes()
    finally:
        for d in (src, dst, size):
            d.free()
    rule = R.Index(data, 10, table_offsets(archive))
    assert rule.misaligned > 0
    o = Opened(H, codec, archive)
    try:
        results, rebuilt = rebuild(H, codec, o, [(0, o.N)])
        assert results == [[0, rule.records, rule.misaligned, rule.delimiters]] and rebuilt.tolist() == rule.first_record.tolist()
        result, loaded = load(H, codec, o)                                             # an archive without an index: the array is untouched
        assert result == [R.E_PREFIX, 0, 0, 0] and (loaded.view(np.uint8) == CANARY).all()
    finally:
        o.close(codec)
    arc = SeekableArchive(archive)
    try:
        with pytest.raises(ValueError):
            arc.first_record()
        assert arc.first_record(allow_misaligned=True).tolist() == rule.first_record.tolist()
    finally:
        arc.close()


def test_the_counts_scan_at_its_second_level(L, H, codec):
    """2 097 153 raw one-byte frames with table and index, written by numpy: load needs no decode"""
    n = BD.SCAN_LEVEL + 1
    rng = np.random.default_rng(77)
    content = np.where(rng.random(n) < 0.3, 10, 120).astype(np.uint8)
    content[-1] = 120                                                                 # a tail record
    frames = np.tile(np.frombuffer(R.raw_frame(b"x"), dtype=np.uint8), (n, 1))
    frames[:, -1] = content
    rule = R.Index(content.tobytes(), 10, np.arange(n + 1, dtype=np.uint64))
    counts = rule.counts.astype(np.uint32)
    assert int(counts[-1]) == 1 and int(counts.sum()) == rule.records
    import struct
    index = struct.pack("<IIIBBHIIQQ", R.MAGIC, 32 + 4 * n, R.INNER, R.VERSION, 10, 0, n, 0, rule.records, R.check_of_np(counts, rule.records, 10)) + counts.tobytes()
    rows = np.empty((n + 1, 2), dtype=np.uint32)
    rows[:n, 0], rows[:n, 1] = frames.shape[1], 1
    rows[n] = (len(index), 0)
    archive = frames.tobytes() + index + struct.pack("<II", R.SEEK_SKIP, (n + 1) * 8 + 9) + rows.tobytes() + struct.pack("<IBI", n + 1, 0, R.SEEK_MAGIC)
    o = Opened(H, codec, archive)
    try:
        assert o.N == n + 1 > BD.SCAN_LEVEL
        result, loaded = load(H, codec, o)
        assert result == [0, rule.records, 10, n]
        assert (loaded[:n + 1] == rule.first_record).all() and int(loaded[n + 1]) == rule.records
    finally:
        o.close(codec)


def test_damage(L, H, codec, text):
    from zstandard_amd import api
    data = text[:200000]
    sizes, first = api.split_records(data, b"\n", 4096, 4096)
    archive = api.attach_record_index(codec.compress_seekable_frames_host(np.frombuffer(data, dtype=np.uint8), sizes, 3, True), first)
    n, entry, at, rows = R.table_of(archive)
    index_at = at - rows[-1][0]
    assert n == len(sizes) + 1 and archive[index_at + 8:index_at + 12] == b"RIDX"

    def loaded_status(damaged):
        o = Opened(H, codec, bytes(damaged))
        try:
            result, array = load(H, codec, o)
            return result, bool((array.view(np.uint8) == CANARY).all())
        finally:
            o.close(codec)
    good, untouched = loaded_status(archive)
    assert good == [0, int(first[-1]), 10, len(sizes)] and not untouched
    b = bytearray(archive); b[index_at + 40 + 4 * 7] ^= 1                            # a count
    assert loaded_status(b) == ([R.E_CORRUPT, 0, 0, 0], True)
    b = bytearray(archive); b[index_at + 10] ^= 0x20                                 # the inner magic
    assert loaded_status(b) == ([R.E_PREFIX, 0, 0, 0], True)
    b = bytearray(archive); b[index_at + 12] = 2                                     # the version
    assert loaded_status(b)[0][0] == R.E_VERSION
    # a content frame inside a rebuild window: the window's code is that frame's, as the find calls report it
    victim = 5
    frame_at = sum(r[0] for r in rows[:victim])
    b = bytearray(archive); b[frame_at + rows[victim][0] // 2] ^= 0x55
    o = Opened(H, codec, bytes(b))
    try:
        results, _ = rebuild(H, codec, o, [(0, 3), (3, 6), (9, o.N - 9)])
        d_first, work, found, res = up(H, np.zeros(o.N + 1, dtype=np.uint64)), Dev(H, o.h.find_work_bound(3, 6)), Dev(H, 8), Dev(H, 32)
        assert H.hipDeviceSynchronize() == 0
        try:
            o.h.find_records_resident(d_first.p, o.N, b"qz", 3, 6, work.p, o.h.find_work_bound(3, 6), found.p, 1, res.p)
            codec.sync()
            code = (1 << 64) - int(words(res)[0])
        finally:
            for d in (d_first, work, found, res):
                d.free()
        assert 0 < code < 120 and [r[0] for r in results] == [0, code, 0], (code, results)
    finally:
        o.close(codec)


def test_attach_refusals_on_the_device(L, H, codec, text):
    """the word carries what the host form returns; a refused archive is untouched; an error word that comes in stays"""
    from zstandard_amd import api
    data = text[:50000]
    sizes, first = api.split_records(data, b"\n", 4096, 4096)
    archive = codec.compress_seekable_frames_host(np.frombuffer(data, dtype=np.uint8), sizes, 3, True)
    n = len(sizes)
    grown = len(archive) + 40 + 4 * n + 12

    def attach(arc, fr, n_arg, capacity, word=None):
        dev, size, d_first = Dev(H, capacity, bytes(arc)), up(H, np.array([len(arc) if word is None else word], dtype=np.uint64)), up(H, np.asarray(fr, dtype=np.uint64))
        assert H.hipDeviceSynchronize() == 0
        try:
            codec.attach_record_index_resident(dev.p, capacity, size.p, d_first.p, n_arg)
            codec.sync()
            return int(words(size)[0]), words(dev, np.uint8).tobytes()
        finally:
            for d in (dev, size, d_first):
                d.free()
    err = lambda c: (1 << 64) - c
    canary = bytes([CANARY])
    ok, out = attach(archive, first, n, grown)
    assert ok == grown and out == api.attach_record_index(archive, first)
    for what, (arc, fr, n_arg, cap, word), code in (
            ("one byte short", (archive, first, n, grown - 1, None), R.E_TOO_SMALL),
            ("another frame count", (archive, first[:-1], n - 1, grown, None), R.E_PARAM),
            ("a count above its frame", (archive, [0] + [int(first[-1]) + 5000] * n, n, grown, None), R.E_CORRUPT),
            ("descending", (archive, list(first[:3]) + [0] + list(first[4:]), n, grown, None), R.E_CORRUPT),
            ("the table's magic", (archive[:-1] + b"\0", first, n, grown, None), R.E_PREFIX),
            ("an index frame already", (out, list(first) + [first[-1]], n + 1, grown + 100 + 4 * n, None), R.E_UNSUPPORTED),
            ("a size above the capacity", (archive, first, n, grown, grown + 1), R.E_PREFIX)):
        got, after = attach(arc, fr, n_arg, cap, word)
        assert got == err(code), (what, hex(got))
        assert after == bytes(arc) + canary * (cap - len(arc)), (what, "a refused archive was touched")
    got, after = attach(archive, first, n, grown, err(R.E_SRC_SIZE))                 # the word came in as an error
    assert got == err(R.E_SRC_SIZE) and after == archive + canary * (grown - len(archive))


def test_host_checks(L, H, codec):
    one = p(8)
    ctx = codec.ctx
    archive = R.text_archive([b"ab\n", b"cd\n"])
    o = Opened(H, codec, archive)
    try:
        sk = o.h.handle
        assert L.zsmi_seekableIndexRecordsResident(None, None, 999, 0, 9, None, 0, None, None) == R.E_INIT
        assert L.zsmi_seekableIndexRecordsResident(ctx, None, 999, 0, 9, None, 0, one, one) == R.E_GENERIC
        assert L.zsmi_seekableIndexRecordsResident(ctx, sk, 999, 0, 9, None, 0, None, one) == R.E_GENERIC
        assert L.zsmi_seekableIndexRecordsResident(ctx, sk, 999, 0, 9, None, 0, one, None) == R.E_GENERIC
        assert L.zsmi_seekableIndexRecordsResident(ctx, sk, 999, 0, 9, None, 0, one, one) == R.E_PARAM
        assert L.zsmi_seekableIndexRecordsResident(ctx, sk, 10, 0, 3, None, 0, one, one) == R.E_PARAM
        assert L.zsmi_seekableIndexRecordsResident(ctx, sk, 10, 0, 2, None, 0, one, one) == R.E_GENERIC
        assert L.zsmi_seekableIndexRecordsResident(ctx, sk, 10, 0, 2, one, 5, one, one) == R.E_TOO_SMALL
        assert L.zsmi_seekableLoadRecordIndexResident(ctx, None, one, one) == R.E_GENERIC and L.zsmi_seekableLoadRecordIndexResident(ctx, sk, None, one) == R.E_GENERIC
        assert L.zsmi_seekableAttachRecordIndexResident(ctx, None, 0, one, one, 0, 10) == R.E_GENERIC
        assert L.zsmi_seekableAttachRecordIndexResident(ctx, one, 0, one, one, 0x8000001, 256) == R.E_PARAM
        assert L.zsmi_seekableAttachRecordIndexResident(ctx, one, 0, one, one, 0x8000001, 10) == R.E_FRAME_INDEX
        # raw frames without checksums decode and index like any other
        results, rebuilt = rebuild(H, codec, o, [(0, 2)])
        assert results == [[0, 2, 0, 2]] and rebuilt.tolist() == [0, 1, 2]
        first = np.zeros(3, dtype=np.uint64); result = np.zeros(4, dtype=np.uint64)
        assert L.zsmi_seekableIndexRecordsHost(ctx, sk, 10, p(first.ctypes.data), p(result.ctypes.data)) == 0
        assert first.tolist() == [0, 1, 2] and result.tolist() == [0, 2, 0, 2]
        assert L.zsmi_seekableLoadRecordIndexHost(ctx, sk, p(first.ctypes.data), p(result.ctypes.data)) == 0 and result.tolist() == [R.E_PREFIX, 0, 0, 0]
    finally:
        o.close(codec)


def test_the_host_rebuild_in_many_windows():
    """zsmi_seekableIndexRecordsHost with the window plan cut at one frame, 9000 and 20000 bytes and at its default, over frames that end
    on delimiters, frames that cut records and empty frames on both sides of a window border (tests/_recindex.py, windows_child)"""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_recindex.py"), "windows"], env=dict(os.environ, ZSMI_DEBUG_LIB="1"), cwd=ROOT,
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "windows ok" in out.stdout, (out.stdout[-2000:], out.stderr[-4000:])
