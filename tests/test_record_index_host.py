"""The record index on the host (no GPU): zsmi_indexRecords, zsmi_writeRecordIndexFrame, zsmi_readRecordIndexFrame and
zsmi_seekableAttachRecordIndex against the numpy statement of the rule, the frame and the check (tests/_recindex.py) - on the splitter's
inputs (tests/_split.py), where the rule must give the splitter's own firstRecord and no misaligned frame; on empty text, delimiters
only, no delimiter, the delimiters 0 and 255, an unterminated tail, and empty frames in a row at the start and at the end; every refusal
with its code; an attached archive as every reader sees it (n + 1 frames, the text's size, oracle D decodes the whole file to the text).
The four CPU forms also run alone, in a host program under the address and undefined-behaviour sanitizers (tests/c/record_index.cpp)."""
import ctypes, os, re, subprocess
import numpy as np
import pytest
import _recindex as R, _split as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zstandard_amd", "csrc")
p = ctypes.c_void_p


CASES = R.cases()


@pytest.fixture(scope="module")
def L():
    from zstandard_amd import _lib
    _lib.build()
    return _lib.lib()


def code(L, r):
    return int(L.zsmi_getErrorCode(r)) if L.zsmi_isError(r) else 0


def fake_archive(sizes, checksum=False):
    """a table over one-byte stand-ins for the frames: the host calls judge the table, never a frame"""
    import _seekable as SE
    return b"F" * len(sizes) + SE.table([(1, s, 0) for s in sizes], checksum)


def test_the_restatement_on_inputs_worked_by_hand():
    x = R.Index(b"ab\ncd\nef", 10, [0, 3, 6, 8])
    assert (x.first_record.tolist(), x.records, x.delimiters, x.misaligned) == ([0, 1, 2, 3], 3, 2, 0)
    x = R.Index(b"ab\ncd\nef", 10, [0, 4, 8])                      # "ab\nc" holds a delimiter, ends on 'c', not at the end
    assert (x.first_record.tolist(), x.misaligned, x.misaligned_frames.tolist()) == ([0, 1, 3], 1, [0])
    x = R.Index(b"ab\ncd\nef", 10, [0, 4, 8], at_end=False)        # the same bytes as a window: no tail record, and the last frame counts
    assert (x.first_record.tolist(), x.records, x.misaligned) == ([0, 1, 2], 2, 2)
    x = R.Index(b"ab\ncd", 10, [0, 3, 5, 5, 5])                    # empty frames at the content's end get `records`
    assert x.first_record.tolist() == [0, 1, 2, 2, 2] and x.misaligned == 0
    x = R.Index(b"", 10, [0, 0])
    assert x.first_record.tolist() == [0, 0] and x.records == 0
    f = R.frame([0, 2, 2, 5], 10)
    assert len(f) == 52 and f[:16] == bytes.fromhex("5d2a4d18" "2c000000" "52494458" "010a0000") and R.parse(f) == ([0, 2, 2, 5], 10)
    check = (3 * 1 * R.K1 + 1 * 3 * R.K1 + 4 * 5 * R.K1 + 5 * R.K2 + 10) & R.M64
    assert int.from_bytes(f[32:40], "little") == check == R.check_of_np([2, 0, 3], 5, 10)
    import _seekable as SE
    assert SE.xxh32(b"") == R.EMPTY_HASH


@pytest.mark.parametrize("name", sorted(k for k in CASES if k.startswith("split_")))
def test_the_rule_is_the_splitters_rule_4(name):
    """the issue's claim, on the CPU: over every array the splitter makes, P(dOff[i]) is its firstRecord and no frame is misaligned"""
    data, delim, sizes = CASES[name]
    _, _, T, M = S.cases()[name[len("split_"):]]
    want = S.Split(data, delim, T, M)
    x = R.Index(data, delim, R.offsets_of(sizes))
    assert x.first_record.tolist() == want.first_record and x.records == want.records and x.misaligned == 0
    assert (x.counts <= np.asarray(sizes, dtype=np.int64)).all() if sizes else True


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_host_calls_are_the_restatement(L, name):
    data, delim, sizes = CASES[name]
    n = len(sizes)
    want = R.Index(data, delim, R.offsets_of(sizes))
    sz = np.asarray(sizes, dtype=np.uint32)
    first = np.full(n + 2, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    result = np.full(5, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    assert L.zsmi_indexRecords(data, len(data), p(sz.ctypes.data) if n else None, n, delim, p(first.ctypes.data), p(result.ctypes.data)) == 0
    assert first[:n + 1].tolist() == want.first_record.tolist() and int(first[n + 1]) == 0xA5A5A5A5A5A5A5A5
    assert result.tolist() == [0, want.records, want.misaligned, want.delimiters, 0xA5A5A5A5A5A5A5A5]
    # write, exactly sized between two guard bytes
    frame = R.frame(want.first_record, delim)
    assert L.zsmi_recordIndexFrameSize(n) == len(frame) == 40 + 4 * n
    buf = np.full(len(frame) + 2, 0xA5, dtype=np.uint8)
    assert L.zsmi_writeRecordIndexFrame(p(buf.ctypes.data + 1), len(frame), p(first.ctypes.data), n, delim) == len(frame)
    assert buf[1:-1].tobytes() == frame and buf[0] == buf[-1] == 0xA5
    assert code(L, L.zsmi_writeRecordIndexFrame(p(buf.ctypes.data + 1), len(frame) - 1, p(first.ctypes.data), n, delim)) == R.E_TOO_SMALL
    # read
    back = np.full(n + 2, 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
    d = ctypes.c_int(-1)
    assert L.zsmi_readRecordIndexFrame(frame, len(frame), p(back.ctypes.data), n + 1, ctypes.byref(d)) == n and d.value == delim
    assert back[:n + 1].tolist() == want.first_record.tolist() and int(back[n + 1]) == 0x5A5A5A5A5A5A5A5A
    assert L.zsmi_readRecordIndexFrame(frame, len(frame), None, 0, None) == n
    # attach: a table over stand-in frames, with and without checksums
    for checksum in (False, True):
        arc = fake_archive(sizes, checksum)
        grown = len(arc) + len(frame) + (12 if checksum else 8)
        room = np.full(grown + 1, 0xA5, dtype=np.uint8)
        room[:len(arc)] = np.frombuffer(arc, dtype=np.uint8)
        assert L.zsmi_seekableAttachRecordIndex(p(room.ctypes.data), len(arc), grown, p(first.ctypes.data), n, delim) == grown
        assert room[:grown].tobytes() == R.attached(arc, want.first_record, delim) and room[grown] == 0xA5
        assert L.zsmi_seekableNumFrames(p(room.ctypes.data), grown) == n + 1 and L.zsmi_seekableContentSize(p(room.ctypes.data), grown) == len(data)


def test_an_attached_archive_as_every_reader_sees_it(L):
    """real frames (oracle E's): n + 1 frames, the text's content size, and oracle D decodes the whole file - the index frame and the table
    skipped - to the text"""
    import _oracle as O, _seekable as SE
    data = S.lines(9, 150, 120)
    sp = S.Split(data, 10, 1000, 4096)
    parts = [data[int(a):int(b)] for a, b in zip(R.offsets_of(sp.sizes)[:-1], R.offsets_of(sp.sizes)[1:])]
    for checksum in (False, True):
        arc = SE.archive([O.compress(c, 3) for c in parts], parts, checksum)
        first = np.asarray(sp.first_record, dtype=np.uint64)
        grown = len(arc) + 40 + 4 * sp.n + (12 if checksum else 8)
        room = np.zeros(grown, dtype=np.uint8)
        room[:len(arc)] = np.frombuffer(arc, dtype=np.uint8)
        assert L.zsmi_seekableAttachRecordIndex(p(room.ctypes.data), len(arc), grown, p(first.ctypes.data), sp.n, 10) == grown
        out = room.tobytes()
        assert out == R.attached(arc, sp.first_record, 10)
        assert L.zsmi_seekableNumFrames(out, len(out)) == sp.n + 1 and L.zsmi_seekableContentSize(out, len(out)) == len(data)
        rows, ck = SE.parse(out)
        assert ck == checksum and rows[-1] == (40 + 4 * sp.n, 0, R.EMPTY_HASH if checksum else None)
        assert O.decompress(out, len(data)) == data
        info = [ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint32(), ctypes.c_uint32()]
        assert L.zsmi_seekableFrameInfo(out, len(out), sp.n, *[ctypes.byref(v) for v in info]) == 0
        at = info[0].value
        assert (info[1].value, info[2].value, info[3].value) == (len(data), 40 + 4 * sp.n, 0)
        back = np.zeros(sp.n + 1, dtype=np.uint64)
        assert L.zsmi_readRecordIndexFrame(out[at:], 40 + 4 * sp.n, p(back.ctypes.data), sp.n + 1, None) == sp.n and back.tolist() == sp.first_record


def test_refusals_with_their_codes(L):
    first = np.array([0, 2, 2, 5], dtype=np.uint64)
    fp = p(first.ctypes.data)
    dst = np.zeros(52, dtype=np.uint8)
    dp = p(dst.ctypes.data)
    assert code(L, L.zsmi_recordIndexFrameSize(0x8000000)) == R.E_FRAME_INDEX and L.zsmi_recordIndexFrameSize(0x7FFFFFF) == 40 + 4 * 0x7FFFFFF
    assert code(L, L.zsmi_writeRecordIndexFrame(dp, 52, fp, 3, 256)) == R.E_PARAM and code(L, L.zsmi_writeRecordIndexFrame(dp, 52, fp, 3, -1)) == R.E_PARAM
    assert code(L, L.zsmi_writeRecordIndexFrame(dp, 52, fp, 0x8000000, 10)) == R.E_FRAME_INDEX
    assert code(L, L.zsmi_writeRecordIndexFrame(dp, 52, None, 3, 10)) == R.E_GENERIC and code(L, L.zsmi_writeRecordIndexFrame(None, 52, fp, 3, 10)) == R.E_GENERIC
    for bad in ([1, 2, 2, 5], [0, 2, 1, 5], [0, 1 << 32, 1 << 32, 1 << 32]):
        assert code(L, L.zsmi_writeRecordIndexFrame(dp, 52, p(np.array(bad, dtype=np.uint64).ctypes.data), 3, 10)) == R.E_CORRUPT, bad
    assert code(L, L.zsmi_writeRecordIndexFrame(dp, 51, fp, 3, 10)) == R.E_TOO_SMALL and not dst.any()
    good = R.frame([0, 2, 2, 5], 10)
    out = np.zeros(4, dtype=np.uint64)

    def read(frame, capacity=4):
        return code(L, L.zsmi_readRecordIndexFrame(bytes(frame), len(frame), p(out.ctypes.data), capacity, None))

    def flipped(at, bit=1):
        b = bytearray(good); b[at] ^= bit
        return b
    assert read(good) == 0 and read(good[:39]) == R.E_SRC_SIZE and read(good[:51]) == R.E_SRC_SIZE and read(good, 3) == R.E_TOO_SMALL
    assert read(flipped(0)) == R.E_PREFIX and read(flipped(3, 0x80)) == R.E_PREFIX                       # the outer magic
    assert all(read(flipped(at)) == R.E_PREFIX for at in (8, 9, 10, 11))                                # the inner magic
    assert read(flipped(12, 3)) == R.E_VERSION and read(flipped(12)) == R.E_VERSION                     # version 2, version 0
    assert read(flipped(14)) == R.E_CORRUPT and read(flipped(15, 0x80)) == R.E_CORRUPT and read(flipped(23, 0x40)) == R.E_CORRUPT      # reserved
    assert read(flipped(4, 4)) == R.E_CORRUPT and read(flipped(16)) == R.E_CORRUPT                       # Frame_Size against n
    assert all(read(flipped(at)) == R.E_CORRUPT for at in (13, 24, 31, 32, 39, 40, 44, 51))             # delim, records, check, counts
    swapped = bytearray(good); swapped[40:44], swapped[48:52] = good[48:52], good[40:44]                # the same counts in other places
    assert read(swapped) == R.E_CORRUPT
    assert code(L, L.zsmi_readRecordIndexFrame(None, 52, None, 0, None)) == R.E_SRC_SIZE
    # index
    text, sizes = b"ab\ncd\nef\ngh\n", np.array([4, 4, 4], dtype=np.uint32)
    sp, res = p(sizes.ctypes.data), p(out.ctypes.data)
    assert L.zsmi_indexRecords(text, 12, sp, 3, -1, res, None) == R.E_PARAM and L.zsmi_indexRecords(text, 12, sp, 3, 256, res, None) == R.E_PARAM
    assert L.zsmi_indexRecords(text, 12, None, 3, 10, res, None) == R.E_GENERIC and L.zsmi_indexRecords(text, 12, sp, 3, 10, None, None) == R.E_GENERIC
    assert L.zsmi_indexRecords(None, 12, sp, 3, 10, res, None) == R.E_SRC_SIZE and L.zsmi_indexRecords(text, 11, sp, 3, 10, res, None) == R.E_SRC_SIZE
    assert L.zsmi_indexRecords(text, 12, sp, 3, 10, res, None) == 0 and out.tolist() == [0, 1, 2, 4]
    # attach: each refusal leaves the archive as it was
    arc = fake_archive([4, 4, 4])
    grown = len(arc) + 52 + 8

    def attach(archive, fr, n=3, delim=10, capacity=None, size=None):
        room = np.zeros(grown + 60, dtype=np.uint8)
        room[:len(archive)] = np.frombuffer(bytes(archive), dtype=np.uint8)
        r = L.zsmi_seekableAttachRecordIndex(p(room.ctypes.data), len(archive) if size is None else size, grown if capacity is None else capacity,
                                             p(np.array(fr, dtype=np.uint64).ctypes.data) if fr is not None else None, n, delim)
        if L.zsmi_isError(r):
            assert room[:len(archive)].tobytes() == bytes(archive) and not room[len(archive):].any(), "a refused archive was touched"
        return code(L, r), room
    ok = [0, 1, 2, 4]
    broken = bytearray(arc); broken[-1] ^= 1
    assert attach(broken, ok)[0] == R.E_PREFIX and attach(arc, ok, size=8)[0] == R.E_PREFIX
    broken = bytearray(arc); broken[-5] |= 4
    assert attach(broken, ok)[0] == R.E_CORRUPT
    broken = bytearray(arc); broken[len(arc) - 17 - 24 + 8] = 2                                         # a Compressed_Size that does not add up
    assert attach(broken, ok)[0] == R.E_CORRUPT
    assert attach(arc, ok, n=2)[0] == R.E_PARAM and attach(arc, ok + [4], n=4)[0] == R.E_PARAM and attach(arc, ok, delim=256)[0] == R.E_PARAM
    assert attach(arc, None)[0] == R.E_GENERIC
    assert attach(arc, [0, 5, 5, 5])[0] == R.E_CORRUPT and attach(arc, [0, 2, 1, 4])[0] == R.E_CORRUPT and attach(arc, [1, 1, 2, 4])[0] == R.E_CORRUPT
    assert attach(arc, ok, capacity=grown - 1)[0] == R.E_TOO_SMALL
    c, room = attach(arc, ok)
    assert c == 0 and room[:grown].tobytes() == R.attached(arc, ok, 10)
    assert attach(room[:grown].tobytes(), ok + [4], n=4, capacity=grown + 60)[0] == R.E_UNSUPPORTED        # it carries an index frame already
    # the device calls: a NULL ctx in front of everything; the later checks need a context and are the GPU tests'
    one = p(8)
    assert L.zsmi_indexRecordsDevice(None, None, 5, None, 0, 999, 0, None, None, None) == R.E_INIT
    assert L.zsmi_seekableIndexRecordsResident(None, None, 999, 0, 0, None, 0, None, None) == R.E_INIT
    assert L.zsmi_seekableLoadRecordIndexResident(None, one, one, one) == R.E_INIT
    assert L.zsmi_seekableAttachRecordIndexResident(None, one, 0, one, one, 0, 999) == R.E_INIT
    assert L.zsmi_seekableLoadRecordIndexHost(None, one, one, one) == R.E_INIT and L.zsmi_seekableIndexRecordsHost(None, one, 999, one, one) == R.E_INIT


def test_names(L):
    from zstandard_amd import _lib, api
    hdr = open(os.path.join(ROOT, "include", "zsmi.h")).read()
    so = ctypes.CDLL(_lib.LIB_PATH)
    for name in R.NAMES:
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in _lib.EXPORTS and hasattr(so, name), name
    for name in ("index_records", "write_record_index_frame", "read_record_index_frame", "attach_record_index"):
        assert hasattr(api, name), name
    for name in ("index_records_device", "attach_record_index_resident"):
        assert hasattr(api.BatchCodec, name), name
    for name in ("load_record_index_resident", "index_records_resident"):
        assert hasattr(api.SeekableHandle, name), name
    assert hasattr(api.SeekableArchive, "first_record")


def test_python_surface(L):
    from zstandard_amd import api
    for name in ("split_random_T1000", "empty_frames_at_the_end_behind_a_tail", "empty_text_no_frames", "delim_255_fixed", "fixed_64_over_lines"):
        data, delim, sizes = CASES[name]
        want = R.Index(data, delim, R.offsets_of(sizes))
        first, info = api.index_records(data, sizes, bytes([delim]))
        assert first.dtype == np.uint64 and first.tolist() == want.first_record.tolist()
        assert info == {"records": want.records, "misaligned": want.misaligned, "delimiters": want.delimiters}
        frame = api.write_record_index_frame(first, bytes([delim]))
        assert frame == R.frame(want.first_record, delim)
        back, d = api.read_record_index_frame(frame)
        assert back.tolist() == first.tolist() and d == bytes([delim])
        arc = fake_archive(sizes, True)
        assert api.attach_record_index(arc, first, bytes([delim])) == R.attached(arc, want.first_record, delim)
    with pytest.raises(RuntimeError):
        api.read_record_index_frame(b"\0" * 40)
    with pytest.raises(ValueError):
        api.index_records(b"abc", [3], b"\r\n")


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="the sanitizer build is a CPU-side check: it runs on machines without a GPU, never next to one")
def test_the_cpu_forms_under_sanitizers(L, tmp_path):
    """the header alone, host code only, with -fsanitize=address,undefined: every input and every output in a heap block of exactly its size"""
    exe = str(tmp_path / "record_index")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, os.path.join(ROOT, "tests", "c", "record_index.cpp"), "-o", exe])
    args, names = [], sorted(CASES)
    for k, name in enumerate(names):
        data, delim, sizes = CASES[name]
        stem = str(tmp_path / ("case%d" % k))
        open(stem + ".text", "wb").write(data)
        open(stem + ".sizes", "wb").write(np.asarray(sizes, dtype=np.uint32).tobytes())
        open(stem + ".archive", "wb").write(fake_archive(sizes, k % 2 == 1))
        args += ["case", stem + ".text", str(delim), stem + ".sizes", stem + ".archive", stem]
    out = subprocess.run([exe] + args, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-4000:]
    rows = out.stdout.splitlines()
    assert len(rows) == len(names)
    for k, (name, row) in enumerate(zip(names, rows)):
        data, delim, sizes = CASES[name]
        n, stem = len(sizes), str(tmp_path / ("case%d" % k))
        want = R.Index(data, delim, R.offsets_of(sizes))
        arc = fake_archive(sizes, k % 2 == 1)
        grown = len(arc) + 40 + 4 * n + (12 if k % 2 == 1 else 8)
        assert row.split() == ["0", str(want.records), str(want.misaligned), str(want.delimiters), ",".join(str(v) for v in want.first_record.tolist()),
                               str(40 + 4 * n), str(-R.E_TOO_SMALL), str(n), str(delim), str(-R.E_SRC_SIZE), str(grown), str(-R.E_TOO_SMALL), "1"], name
        assert open(stem + ".frame", "rb").read() == R.frame(want.first_record, delim), name
        assert open(stem + ".attached", "rb").read() == R.attached(arc, want.first_record, delim), name
    open(str(tmp_path / "three"), "wb").write(fake_archive([4, 4, 4]))
    out = subprocess.run([exe, "rejections", str(tmp_path / "three")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-4000:]
    got = dict(line.split() for line in out.stdout.splitlines())
    want = {"write_delim": -R.E_PARAM, "write_too_many": -R.E_FRAME_INDEX, "write_null": -R.E_GENERIC, "write_first_not_0": -R.E_CORRUPT, "write_descends": -R.E_CORRUPT,
            "write_short": -R.E_TOO_SMALL, "size_too_many": -R.E_FRAME_INDEX,
            "read_39_bytes": -R.E_SRC_SIZE, "read_outer_magic": -R.E_PREFIX, "read_inner_magic": -R.E_PREFIX, "read_version": -R.E_VERSION, "read_reserved_16": -R.E_CORRUPT,
            "read_reserved_32": -R.E_CORRUPT, "read_frame_size": -R.E_CORRUPT, "read_n": -R.E_CORRUPT, "read_cut": -R.E_SRC_SIZE, "read_capacity": -R.E_TOO_SMALL,
            "read_count": -R.E_CORRUPT, "read_records": -R.E_CORRUPT, "read_check": -R.E_CORRUPT, "read_delim": -R.E_CORRUPT, "read_good": 3,
            "index_delim": -R.E_PARAM, "index_null_sizes": -R.E_GENERIC, "index_null_first": -R.E_GENERIC, "index_null_text": -R.E_SRC_SIZE, "index_sum": -R.E_SRC_SIZE,
            "index_good": 0,
            "attach_table_magic": -R.E_PREFIX, "attach_table_reserved": -R.E_CORRUPT, "attach_n": -R.E_PARAM, "attach_delim": -R.E_PARAM, "attach_null": -R.E_GENERIC,
            "attach_count_above_frame": -R.E_CORRUPT, "attach_descends": -R.E_CORRUPT, "attach_short": -R.E_TOO_SMALL, "attach_untouched": 1,
            "attach_good": len(fake_archive([4, 4, 4])) + 52 + 8, "attach_twice": -R.E_UNSUPPORTED}
    assert {k: int(v) for k, v in got.items()} == want
