"""Find records by regular expression in a record archive (zsmi_seekableFindRegexResident, zsmi_seekableFindRegexHost,
SeekableArchive.find_records_regex, SeekableHandle.find_regex_resident).  The yardstick is tests/_findre.py's Python statement of the rule
(`re` on every record) on the source text, or on the slice of it a window of frames holds, with B = first_record[firstFrame] from the
splitter's Python rule (tests/_split.py) - never another call of the library.  The archive is small: a few hundred short lines in mixed
case, empty ones among them, a targetSize of 4 KiB and one record cut into several frames.  dWork, dRecords, dResult and dFirstRecord lie
between canaries; a window's call gets exactly its work bound of dWork and must leave everything behind it as it was."""
import ctypes
import numpy as np
import pytest
import _find as F, _findre as R, _split as S, _seekable as SK
from _hip import hip_of, Dev, CANARY, PAD
from _resident import up, down

pytestmark = pytest.mark.gpu
T, M = 4096, 4096
PATTERNS = ((b"error", 0), (b"error", R.IGNORE_CASE), (b"^(Error|WARN) .*id=[78]$", 0), (b"timeout.*id=7|^$", 0), (b"^y+ ERROR y*z{3}$", 0), (b"y{40}.*z", R.INVERT),
            (b"nowhere", 0), (b"^[a-z =0-9]*$", R.IGNORE_CASE | R.INVERT))


def text():
    """about 300 short lines, empty ones among them, and one record of 10000 bytes that M cuts into three frames; no delimiter at the end"""
    rng = np.random.default_rng(78)
    words = (b"Error", b"error", b"WARN", b"warn", b"timeout", b"id=7", b"id=8", b"ok", b"debug", b"z")
    lines = []
    for i in range(300):
        if i % 23 == 5:
            lines.append(b"")
        else:
            lines.append(b" ".join(words[j] for j in rng.integers(0, len(words), int(rng.integers(3, 20)))))
    lines[150] = b"y" * 5000 + b" ERROR " + b"y" * 4990 + b"zzz"
    return b"\n".join(lines)


TEXT = text()


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


class Opened:
    """a text, its split by the Python rule, its archive opened, and buffers every window's call shares: dFirstRecord as the rule leaves
    it, dWork of the whole content, dRecords of a number a record, dResult - each between canaries, filled with the canary before a call"""

    def __init__(self, L, H, codec, data, delim=10, arc=None, T=T, M=M):
        self.L, self.H, self.codec, self.data, self.delim = L, H, codec, data, delim
        self.split = S.Split(data, delim, T, M)
        self.n = self.split.n
        self.at = [0] + np.cumsum(self.split.sizes, dtype=np.int64).tolist()
        self.arc = arc if arc is not None else codec.compress_seekable_frames_host(data, self.split.sizes, 3, True)
        err = ctypes.c_int(-1)
        self.sk = L.zsmi_openSeekable(codec.ctx, self.arc, len(self.arc), ctypes.byref(err))
        assert self.sk and err.value == 0, err.value
        self.room = max(self.split.records, 1)
        self.first = up(H, np.asarray(self.split.first_record, dtype=np.uint64))
        self.work, self.rec, self.res = Dev(H, max(len(data), 1)), Dev(H, 8 * self.room), Dev(H, 32)

    def close(self):
        self.codec.sync(); self.L.zsmi_closeSeekable(self.sk)
        for d in (self.first, self.work, self.rec, self.res):
            d.free()

    def find(self, pattern, flags, a=0, b=None, capacity=None, work_capacity=None):
        """one zsmi_seekableFindRegexResident call over frames [a, b): (rc, dResult, the numbers written, whether dRecords kept its
        fill).  workCapacity: the window's bound, exactly"""
        L, H, p = self.L, self.H, ctypes.c_void_p
        b = self.n if b is None else b
        bound = L.zsmi_seekableFindWorkBound(self.sk, a, b - a)
        assert bound == self.at[b] - self.at[a]
        cap = self.room if capacity is None else capacity
        wcap = bound if work_capacity is None else work_capacity
        for d in (self.work, self.rec, self.res):
            assert H.hipMemset(ctypes.c_void_p(d.p), CANARY, d.n) == 0
        prog = R.program(L, pattern, flags)
        rc = L.zsmi_seekableFindRegexResident(self.codec.ctx, self.sk, p(self.first.p), self.n, self.delim, ctypes.byref(prog), a, b - a, p(self.work.p), wcap,
                                              p(self.rec.p) if cap else None, cap, p(self.res.p))
        self.codec.sync()
        res, ok = down(self.res, np.uint64)
        assert ok, "wrote outside dResult"
        rec, ok = down(self.rec, np.uint64)
        assert ok, "wrote outside dRecords"
        first, ok = down(self.first, np.uint64)
        assert ok and first.tolist() == self.split.first_record, "dFirstRecord changed"
        raw = np.frombuffer(self.work.all(), dtype=np.uint8)
        assert (raw[:PAD] == CANARY).all() and (raw[PAD + min(wcap, bound):] == CANARY).all(), "wrote outside [dWork, dWork + the window's bound)"
        result = [int(v) for v in res]
        untouched = bool((rec.view(np.uint8) == CANARY).all())
        if rc or result[0] >= 1 << 63 or cap == 0:
            assert untouched, "dRecords written by a call that has nothing to write"
            return rc, result, [], untouched
        written = result[1]
        assert written <= cap and (rec[written:].view(np.uint8) == CANARY).all(), "written behind the numbers"
        return rc, result, [int(v) for v in rec[:written]], untouched

    def check(self, pattern, flags, a=0, b=None, what=""):
        b = self.n if b is None else b
        records, text_records = R.window(self.data, self.split.sizes, self.split.first_record, a, b, pattern, flags, self.delim)
        rc, result, got, _ = self.find(pattern, flags, a, b)
        assert rc == 0 and result == [len(records), len(records), text_records, self.at[b] - self.at[a]], (what, pattern, flags, a, b, rc, result, len(records), text_records)
        assert got == records, (what, pattern, flags, a, b, got[:8], records[:8])
        return records, text_records


@pytest.fixture(scope="module")
def opened(L, H, codec):
    o = Opened(L, H, codec, TEXT)
    yield o
    o.close()


def test_the_archive_is_the_one_described(opened):
    o = opened
    starts = F.record_starts(o.split.first_record)
    assert o.split.records == 300 and 5 < o.n < 40 and 1 < len(starts) < o.n       # frames that begin a record, and frames that do not
    f = o.split.frame_of(150)
    assert o.split.first_record[f] == o.split.first_record[f + 1] == o.split.first_record[f + 2] == 150
    answers = [R.find(TEXT, pattern, flags)[0] for pattern, flags in PATTERNS]
    assert sum(1 for a in answers if 0 < len(a) < 300) >= 6 and 150 in answers[4] and answers[6] == []


def test_the_whole_window(opened):
    for pattern, flags in PATTERNS:
        assert opened.check(pattern, flags, what="whole") == R.find(TEXT, pattern, flags)


def test_windows_cut_where_records_begin(opened):
    """together they give the whole window's answer (checked on the CPU first)"""
    o = opened
    for pattern, flags in PATTERNS[1:6]:
        cuts = R.boundary_windows(o.data, o.split.sizes, o.split.first_record, pattern, flags, o.delim)
        records, text_records = [], 0
        for a, b in cuts:
            r, n = o.check(pattern, flags, a, b, what="cut")
            records += r; text_records += n
        assert (records, text_records) == o.check(pattern, flags, what="whole")


def test_windows_cut_anywhere(opened):
    """a window that begins or ends inside the cut record: the record is judged on the part inside the window"""
    o = opened
    f = o.split.frame_of(150)
    for a, b in ((f, f + 1), (f + 1, f + 3), (f + 2, o.n), (0, f + 2), (f - 1, f + 1)):
        for pattern, flags in PATTERNS[4:6] + ((b"^y*$", 0), (b"ERROR", R.INVERT)):
            o.check(pattern, flags, a, b, what="inside the cut record")


def test_capacity_the_work_bound_and_no_frame(opened):
    o = opened
    pattern, flags = b"error|warn", R.IGNORE_CASE
    bound = len(o.data)
    records, text_records = R.find(TEXT, pattern, flags)
    assert len(records) > 4
    rc, result, got, untouched = o.find(pattern, flags, capacity=0)
    assert rc == 0 and result == [len(records), 0, text_records, bound] and untouched
    rc, result, got, _ = o.find(pattern, flags, capacity=len(records) - 2)
    assert rc == 0 and result == [len(records), len(records) - 2, text_records, bound] and got == records[:-2]
    for a, b in ((o.n, o.n), (3, 3)):                                              # frameCount 0
        rc, result, got, untouched = o.find(pattern, flags, a, b)
        assert rc == 0 and result == [0, 0, 0, 0] and untouched
    rc, result, got, untouched = o.find(pattern, flags, work_capacity=bound - 1)
    assert rc == F.E_TOO_SMALL and untouched and result == [0xA5A5A5A5A5A5A5A5] * 4      # nothing was queued
    a, b = 2, o.n - 1
    rc, result, got, untouched = o.find(pattern, flags, a, b, work_capacity=o.at[b] - o.at[a] - 1)
    assert rc == F.E_TOO_SMALL and untouched


def test_a_damaged_frame(L, H, codec):
    """the first failing frame's code in dResult[0], nothing written, from every window that holds the frame"""
    data = S.lines(31, 90, 120)                                                    # seeded bytes: the frames' blocks are stored, a payload bit is a content bit
    o = Opened(L, H, codec, data, T=2048)
    pattern = b"[" + bytes(b for b in data if b not in b"\n]\\^-")[:3] + b"]{2}"
    try:
        assert o.n >= 3
        rows, flag = SK.parse(o.arc)
        assert flag and len(rows) == o.n
        assert 0 < len(o.check(pattern, 0)[0]) and o.check(pattern, R.INVERT)
    finally:
        o.close()
    bad = bytearray(o.arc)
    bad[rows[0][0] + rows[1][0] // 2] ^= 0x10                                      # in the middle of frame 1's compressed bytes
    o = Opened(L, H, codec, data, T=2048, arc=bytes(bad))
    try:
        for flags in (0, R.INVERT):
            for a, b in ((0, o.n), (1, 2), (0, 2), (1, o.n)):
                rc, result, got, untouched = o.find(pattern, flags, a, b)
                assert rc == 0 and result == [(1 << 64) - F.E_CHECKSUM, 0, 0, o.at[b] - o.at[a]] and untouched, (a, b, result)
            o.check(pattern, flags, 0, 1); o.check(pattern, flags, 2, o.n)         # windows that do not touch the damaged frame
    finally:
        o.close()


def test_host_form_and_python_surface(L, H, codec, opened):
    """the host form equals the resident form's answer, which check() holds against the rule"""
    from zstandard_amd import SeekableArchive, compile_regex
    o = opened
    first = np.asarray(o.split.first_record, dtype=np.uint64)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    sa = SeekableArchive(o.arc)
    try:
        for pattern, flags in PATTERNS[1:6]:
            prog = R.program(L, pattern, flags)
            for a, b in ((0, o.n), (1, o.n), (0, o.n - 1)):
                records, text_records = o.check(pattern, flags, a, b)
                for cap in (len(records), max(len(records) - 1, 0), len(records) + 2):
                    out = np.full(cap + 1, R.SENTINEL, dtype=np.uint64); result = np.zeros(4, dtype=np.uint64)
                    rc = L.zsmi_seekableFindRegexHost(codec.ctx, o.sk, p(first), o.n, o.delim, ctypes.byref(prog), a, b - a, p(out) if cap else None, cap, p(result))
                    w = min(cap, len(records))
                    assert rc == 0 and result.tolist() == [len(records), w, text_records, o.at[b] - o.at[a]], (pattern, a, b, cap, rc, result.tolist())
                    assert out[:w].tolist() == records[:w] and (out[w:] == R.SENTINEL).all()
                program = compile_regex(pattern, ignore_case=bool(flags & 1), invert=bool(flags & 2))
                assert sa.find_records_regex(o.split.first_record, program, b"\n", a, b - a) == records
            if not flags:
                assert sa.find_records_regex(o.split.first_record, pattern) == R.find(TEXT, pattern)[0]
        with pytest.raises(RuntimeError):
            sa.find_records_regex(o.split.first_record[:-1], b"error")              # not the archive's frame count
        with pytest.raises(ValueError):
            sa.find_records_regex(o.split.first_record, b"error(")
    finally:
        sa.close()


def test_the_answer_feeds_the_record_reader(L, H, codec):
    """find_regex_resident's numbers, as they stand in device memory, into read_records_resident: the lines returned are the source's"""
    data = TEXT
    split = S.Split(data, 10, T, M)
    arc = codec.compress_seekable_frames_host(data, split.sizes, 3, True)
    pattern = b"^(error|warn) .*z$"
    records, text_records = R.find(data, pattern, R.IGNORE_CASE)
    lines = data.split(b"\n")
    k = len(records)
    assert k > 3 and text_records == 300
    d_arc = Dev(H, len(arc), arc)
    first = up(H, np.asarray(split.first_record, dtype=np.uint64))
    sk = codec.open_seekable_device(d_arc.p, len(arc))
    reads = k + split.n
    wcap = max(sk.records_work_bound(reads), len(data))
    work, rec, res = Dev(H, wcap), Dev(H, 8 * k), Dev(H, 32)
    dst, off, wrote, status, res2 = Dev(H, len(data) + k), Dev(H, 8 * (k + 1)), Dev(H, 8 * k), Dev(H, 4 * k), Dev(H, 32)
    try:
        sk.find_regex_resident(first.p, split.n, R.program(L, pattern, R.IGNORE_CASE), 0, split.n, work.p, len(data), rec.p, k, res.p)
        sk.read_records_resident(first.p, split.n, rec.p, k, reads, work.p, wcap, dst.p, len(data) + k, off.p, wrote.p, status.p, res2.p)
        codec.sync()
        assert down(res, np.uint64)[0].tolist() == [k, k, 300, len(data)] and down(rec, np.uint64)[0].tolist() == records
        assert int(down(res2, np.uint64)[0][0]) == k and not down(status, np.uint32)[0].any()
        offsets, lengths, out = down(off, np.uint64)[0].tolist(), down(wrote, np.uint64)[0].tolist(), down(dst)[0].tobytes()
        for j, r in enumerate(records):
            want = lines[r] + (b"\n" if r + 1 < len(lines) else b"")
            assert out[offsets[j]:offsets[j] + lengths[j]] == want, (j, r)
        with pytest.raises(RuntimeError):
            sk.find_regex_resident(first.p, split.n + 1, pattern, 0, split.n, work.p, len(data), rec.p, k, res.p)
    finally:
        codec.sync(); sk.close()
        for d in (d_arc, first, work, rec, res, dst, off, wrote, status, res2):
            d.free()


def test_host_checks_in_order(L, H, codec, opened):
    """each refusal with every later one present too, so that the order shows; nothing is queued or written by a refused call"""
    o = opened
    n = o.n
    p = ctypes.c_void_p
    one = p(8)                                                                    # a non-NULL pointer no refused call looks behind
    good, bad = ctypes.byref(R.program(L, b"ab")), ctypes.byref(R.damaged(L)["accept bit above nStates"])
    find = L.zsmi_seekableFindRegexResident
    assert find(None, None, None, n + 1, 256, None, 2, n, None, 0, None, 3, None) == F.E_INIT
    assert find(codec.ctx, None, one, n + 1, 256, bad, 2, n, None, 0, one, 3, one) == F.E_GENERIC                    # sk
    assert find(codec.ctx, o.sk, one, n + 1, 256, bad, 2, n, None, 0, one, 3, None) == F.E_GENERIC                   # dResult
    assert find(codec.ctx, o.sk, one, n + 1, 256, None, 2, n, None, 0, one, 3, one) == F.E_GENERIC                   # prog
    assert find(codec.ctx, o.sk, None, n + 1, 256, bad, 2, n, None, 0, one, 3, one) == F.E_GENERIC                   # dFirstRecord
    assert find(codec.ctx, o.sk, one, n + 1, 256, bad, 2, n, None, 0, None, 3, one) == F.E_GENERIC                   # dRecords with capacity > 0
    assert find(codec.ctx, o.sk, one, n + 1, 256, bad, 2, n, None, 0, one, 3, one) == F.E_PARAM                      # delim
    assert find(codec.ctx, o.sk, one, n + 1, 10, bad, 2, n, None, 0, one, 3, one) == F.E_PARAM                       # the program
    assert find(codec.ctx, o.sk, one, n + 1, 10, good, 2, n, None, 0, one, 3, one) == F.E_PARAM                      # nFrames
    assert find(codec.ctx, o.sk, one, n, 10, good, 2, n, None, 0, one, 3, one) == F.E_PARAM                          # firstFrame + frameCount
    assert find(codec.ctx, o.sk, one, n, 10, good, 0xFFFFFFFF, 2, None, 0, one, 3, one) == F.E_PARAM                 # (no wrap)
    assert find(codec.ctx, o.sk, one, n, 10, good, 2, n - 2, None, 0, one, 3, one) == F.E_GENERIC                    # dWork
    assert find(codec.ctx, o.sk, one, n, 10, good, 2, n - 2, one, 0, one, 3, one) == F.E_TOO_SMALL                   # workCapacity
    host = L.zsmi_seekableFindRegexHost
    assert host(codec.ctx, None, one, n, 10, good, 0, n, one, 3, one) == F.E_GENERIC
    assert host(codec.ctx, o.sk, one, n, 10, None, 0, n, one, 3, one) == F.E_GENERIC
    assert host(codec.ctx, o.sk, one, n, 300, good, 0, n, one, 3, one) == F.E_PARAM
    assert host(codec.ctx, o.sk, one, n, 10, bad, 0, n, one, 3, one) == F.E_PARAM
    assert host(codec.ctx, o.sk, one, n + 1, 10, good, 0, n, one, 3, one) == F.E_PARAM
    assert host(codec.ctx, o.sk, one, n, 10, good, 1, n, one, 3, one) == F.E_PARAM
    codec.sync()
