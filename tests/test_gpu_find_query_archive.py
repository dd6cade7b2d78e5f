"""Find records by several patterns in a record archive (zsmi_seekableFindQueryResident, zsmi_seekableFindQueryHost,
SeekableArchive.find_records_query, SeekableHandle.find_query_resident).  The yardstick is tests/_findq.py's Python statement of the rule
on the source text, or on the slice of it a window of frames holds, with B = first_record[firstFrame] from the splitter's Python rule -
never another call of the library.  The archive is small: a few hundred short lines in mixed case, empty ones among them, a targetSize of
4 KiB and one record cut into several frames.  dWork, dRecords, dHits, dResult and dFirstRecord lie between canaries; a window's call
gets exactly its work bound of dWork and must leave everything behind it, and behind what it writes, as it was."""
import ctypes
import numpy as np
import pytest
import _find as F, _findq as Q, _split as S, _seekable as SK, _seekable_resident as SR, _resident_cdict_set as RS
from _hip import hip_of, Dev, CANARY, PAD
from _resident import up, down

pytestmark = pytest.mark.gpu
T, M = 4096, 4096
QUERIES = (([b"error"], 0), ([b"error"], 1), ([b"Error", b"warn"], 1), ([b"timeout", b"id=7"], 0), ([b"y" * 40, b"ERROR", b"z"], 1), ([b"nowhere"], 0))
MODES = (Q.ANY, Q.ALL, Q.NONE)


def text():
    """about 300 short lines, empty ones among them, and one record of 10000 bytes that M cuts into three frames; no delimiter at the end"""
    rng = np.random.default_rng(77)
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


def open_host(L, codec, arc, dset=None):
    err = ctypes.c_int(-1)
    sk = L.zsmi_openSeekable_usingDDictSet(codec.ctx, arc, len(arc), dset.handle if dset is not None else None, ctypes.byref(err))
    assert sk and err.value == 0, err.value
    return sk


class Opened:
    """a text, its split by the Python rule, its archive opened, and buffers every window's call shares: dFirstRecord as the rule leaves
    it, dWork of the whole content, dRecords and dHits of a number a record, dResult - each between canaries, filled with the canary
    before a call"""

    def __init__(self, L, H, codec, data, delim=10, arc=None, dset=None, T=T, M=M):
        self.L, self.H, self.codec, self.data, self.delim = L, H, codec, data, delim
        self.split = S.Split(data, delim, T, M)
        self.n = self.split.n
        self.at = [0] + np.cumsum(self.split.sizes, dtype=np.int64).tolist()
        self.arc = arc if arc is not None else codec.compress_seekable_frames_host(data, self.split.sizes, 3, True)
        self.sk = open_host(L, codec, self.arc, dset)
        self.room = max(self.split.records, 1)
        self.first = up(H, np.asarray(self.split.first_record, dtype=np.uint64))
        self.work, self.rec, self.hit, self.res = Dev(H, max(len(data), 1)), Dev(H, 8 * self.room), Dev(H, self.room), Dev(H, 32)

    def close(self):
        self.codec.sync(); self.L.zsmi_closeSeekable(self.sk)
        for d in (self.first, self.work, self.rec, self.hit, self.res):
            d.free()

    def find(self, patterns, mode, flags, a=0, b=None, capacity=None, work_capacity=None, want_hits=True):
        """one zsmi_seekableFindQueryResident call over frames [a, b): (rc, dResult, the numbers written, their hit sets, whether
        dRecords and dHits kept their fill).  workCapacity: the window's bound, exactly"""
        L, H, p = self.L, self.H, ctypes.c_void_p
        b = self.n if b is None else b
        bound = L.zsmi_seekableFindWorkBound(self.sk, a, b - a)
        assert bound == self.at[b] - self.at[a]
        cap = self.room if capacity is None else capacity
        wcap = bound if work_capacity is None else work_capacity
        for d in (self.work, self.rec, self.hit, self.res):
            assert H.hipMemset(ctypes.c_void_p(d.p), CANARY, d.n) == 0
        q, keep = Q.query(L, patterns, mode, flags)
        rc = L.zsmi_seekableFindQueryResident(self.codec.ctx, self.sk, p(self.first.p), self.n, self.delim, ctypes.byref(q), a, b - a, p(self.work.p), wcap,
                                              p(self.rec.p) if cap else None, p(self.hit.p) if cap and want_hits else None, cap, p(self.res.p))
        self.codec.sync()
        res, ok = down(self.res, np.uint64)
        assert ok, "wrote outside dResult"
        rec, ok = down(self.rec, np.uint64)
        assert ok, "wrote outside dRecords"
        hit, ok = down(self.hit, np.uint8)
        assert ok, "wrote outside dHits"
        first, ok = down(self.first, np.uint64)
        assert ok and first.tolist() == self.split.first_record, "dFirstRecord changed"
        raw = np.frombuffer(self.work.all(), dtype=np.uint8)
        assert (raw[:PAD] == CANARY).all() and (raw[PAD + min(wcap, bound):] == CANARY).all(), "wrote outside [dWork, dWork + the window's bound)"
        result = [int(v) for v in res]
        untouched = bool((rec.view(np.uint8) == CANARY).all() and (hit == CANARY).all())
        if rc or result[0] >= 1 << 63 or cap == 0:
            assert untouched, "dRecords or dHits written by a call that has nothing to write"
            return rc, result, [], [], untouched
        written = result[1]
        assert written <= cap and (rec[written:].view(np.uint8) == CANARY).all() and (hit[written if want_hits else 0:] == CANARY).all(), "written behind the numbers"
        return rc, result, [int(v) for v in rec[:written]], [int(v) for v in hit[:written]] if want_hits else [], untouched

    def check(self, patterns, mode, flags, a=0, b=None, what=""):
        b = self.n if b is None else b
        records, hits, matches = Q.window(self.data, self.split.sizes, self.split.first_record, a, b, patterns, mode, flags, self.delim)
        rc, result, got, sets, _ = self.find(patterns, mode, flags, a, b)
        assert rc == 0 and result == [len(records), len(records), matches, self.at[b] - self.at[a]], (what, patterns, mode, flags, a, b, rc, result, len(records), matches)
        assert got == records and sets == hits, (what, patterns, mode, flags, a, b, got[:8], records[:8], sets[:8], hits[:8])
        return records, hits, matches


@pytest.fixture(scope="module")
def opened(L, H, codec):
    o = Opened(L, H, codec, TEXT)
    yield o
    o.close()


# ------------------------------------------------------------------ 1. windows
def test_the_archive_is_the_one_described(opened):
    o = opened
    starts = F.record_starts(o.split.first_record)
    assert o.split.records == 300 and 5 < o.n < 40 and 1 < len(starts) < o.n       # frames that begin a record, and frames that do not
    f = o.split.frame_of(150)
    assert o.split.first_record[f] == o.split.first_record[f + 1] == o.split.first_record[f + 2] == 150      # the cut record's leading frames share their entry
    for patterns, flags in QUERIES:
        answers = [Q.find(TEXT, patterns, mode, flags) for mode in MODES]
        assert len(answers[0][0]) + len(answers[2][0]) == 300 and len(answers[1][0]) <= len(answers[0][0])
    assert Q.find(TEXT, [b"y" * 40, b"ERROR", b"z"], Q.ALL, 1)[0] and 150 in Q.find(TEXT, [b"y" * 40, b"ERROR", b"z"], Q.ALL, 0)[0]


@pytest.mark.parametrize("mode", MODES)
def test_the_whole_window(opened, mode):
    for patterns, flags in QUERIES:
        records, hits, matches = opened.check(patterns, mode, flags, what="whole")
        assert (records, hits, matches) == Q.find(TEXT, patterns, mode, flags)


@pytest.mark.parametrize("mode", MODES)
def test_windows_cut_where_records_begin(opened, mode):
    """together they give the whole window's answer in every mode, `none` included (checked on the CPU first)"""
    o = opened
    for patterns, flags in QUERIES[1:5]:
        cuts = Q.boundary_windows(o.data, o.split.sizes, o.split.first_record, patterns, mode, flags, o.delim)
        records, hits, matches = [], [], 0
        for a, b in cuts:
            r, h, m = o.check(patterns, mode, flags, a, b, what="cut")
            records += r; hits += h; matches += m
        assert (records, hits, matches) == o.check(patterns, mode, flags, what="whole")


def test_windows_cut_anywhere(opened):
    """a window that begins or ends inside the cut record: the rule on its bytes, numbered from its first frame's entry"""
    o = opened
    f = o.split.frame_of(150)
    for a, b in ((f, f + 1), (f + 1, f + 3), (f + 2, o.n), (0, f + 2), (f - 1, f + 1)):
        for mode in MODES:
            o.check([b"y" * 40, b"ERROR", b"z"], mode, 1, a, b, what="inside the cut record")


def test_capacity_the_work_bound_and_no_frame(opened):
    o = opened
    patterns, flags = [b"error", b"warn"], 1
    bound = len(o.data)
    for mode in MODES:
        records, hits, matches = Q.find(TEXT, patterns, mode, flags)
        assert len(records) > 4
        rc, result, got, sets, untouched = o.find(patterns, mode, flags, capacity=0)
        assert rc == 0 and result == [len(records), 0, matches, bound] and untouched
        rc, result, got, sets, _ = o.find(patterns, mode, flags, capacity=len(records) - 2)
        assert rc == 0 and result == [len(records), len(records) - 2, matches, bound] and got == records[:-2] and sets == hits[:-2]
        rc, result, got, sets, _ = o.find(patterns, mode, flags, want_hits=False)
        assert rc == 0 and got == records and sets == []
        rc, result, got, sets, untouched = o.find(patterns, mode, flags, o.n, o.n)     # frameCount 0
        assert rc == 0 and result == [0, 0, 0, 0] and untouched
        rc, result, got, sets, untouched = o.find(patterns, mode, flags, 3, 3)
        assert rc == 0 and result == [0, 0, 0, 0] and untouched
    rc, result, got, sets, untouched = o.find(patterns, Q.NONE, flags, work_capacity=bound - 1)
    assert rc == F.E_TOO_SMALL and untouched and result == [0xA5A5A5A5A5A5A5A5] * 4      # nothing was queued
    a, b = 2, o.n - 1
    rc, result, got, sets, untouched = o.find(patterns, Q.NONE, flags, a, b, work_capacity=o.at[b] - o.at[a] - 1)
    assert rc == F.E_TOO_SMALL and untouched


# ------------------------------------------------------------------ 2. damage, dictionaries
def test_a_damaged_frame(L, H, codec):
    """the first failing frame's code in dResult[0], nothing written, from every window that holds the frame"""
    data = S.lines(31, 90, 120)                                                    # seeded bytes: the frames' blocks are stored, a payload bit is a content bit
    o = Opened(L, H, codec, data, T=2048)
    try:
        assert o.n >= 3
        rows, flag = SK.parse(o.arc)
        assert flag and len(rows) == o.n
        one = bytes(b for b in data if b != 10)[:1]
        patterns = [one, bytes(b for b in data if b != 10)[7:9]]
        for mode in MODES:
            o.check(patterns, mode, 0)
    finally:
        o.close()
    bad = bytearray(o.arc)
    bad[rows[0][0] + rows[1][0] // 2] ^= 0x10                                      # in the middle of frame 1's compressed bytes
    o = Opened(L, H, codec, data, T=2048, arc=bytes(bad))
    try:
        for mode in MODES:
            for a, b in ((0, o.n), (1, 2), (0, 2), (1, o.n)):
                rc, result, got, sets, untouched = o.find(patterns, mode, 0, a, b)
                assert rc == 0 and result == [(1 << 64) - F.E_CHECKSUM, 0, 0, o.at[b] - o.at[a]] and untouched, (a, b, result)
            o.check(patterns, mode, 0, 0, 1); o.check(patterns, mode, 0, 2, o.n)   # windows that do not touch the damaged frame
    finally:
        o.close()


def test_a_handle_with_a_ddict_set(L, H, codec):
    data = S.text_lines(24 << 10, seed=4)
    split = S.Split(data, 10, 1024, 4096)
    n = split.n
    assert n >= 8
    two = (SR.PICKS[0], SR.PICKS[1])
    index = SR.u32([two[i % 2] for i in range(n)])
    cset, cds = RS.make_set(codec, 3)
    dset, dds = SR.ddict_set(codec)
    try:
        wrote = SR.write(L, H, codec, data, split.sizes, 3, 1, cset, index)
        assert wrote.rc == 0 and wrote.archive is not None
        assert RS.frame_dict_id(wrote.archive[:SK.parse(wrote.archive)[0][0][0]]) != 0     # the frames name their dictionaries
        o = Opened(L, H, codec, data, arc=wrote.archive, dset=dset, T=1024, M=4096)
        try:
            for mode in MODES:
                for patterns, flags in (([b"qu", b"E"], 1), ([b"e", data[5000:5009].replace(b"\n", b"x")], 0)):
                    o.check(patterns, mode, flags, what="dictionaries")
                    o.check(patterns, mode, flags, 3, n - 2, what="dictionaries, a window")
        finally:
            o.close()
    finally:
        codec.sync(); dset.close(); cset.close()
        for h in dds + list(set(cds)):
            h.close()


# ------------------------------------------------------------------ 3. the host form, the Python surface, the host checks
def test_host_form_and_python_surface(L, H, codec, opened):
    from zstandard_amd import SeekableArchive
    o = opened
    first = np.asarray(o.split.first_record, dtype=np.uint64)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    names = {Q.ANY: "any", Q.ALL: "all", Q.NONE: "none"}
    sa = SeekableArchive(o.arc)
    try:
        for patterns, flags in QUERIES[1:5]:
            for mode in MODES:
                q, keep = Q.query(L, patterns, mode, flags)
                for a, b in ((0, o.n), (1, o.n), (0, o.n - 1)):
                    records, hits, matches = Q.window(o.data, o.split.sizes, o.split.first_record, a, b, patterns, mode, flags, o.delim)
                    for cap in (len(records), max(len(records) - 1, 0), len(records) + 2):
                        out = np.full(cap + 1, Q.SENTINEL, dtype=np.uint64); sets = np.full(cap + 1, 0xA5, dtype=np.uint8); result = np.zeros(4, dtype=np.uint64)
                        rc = L.zsmi_seekableFindQueryHost(codec.ctx, o.sk, p(first), o.n, o.delim, ctypes.byref(q), a, b - a, p(out) if cap else None, p(sets) if cap else None, cap, p(result))
                        w = min(cap, len(records))
                        assert rc == 0 and result.tolist() == [len(records), w, matches, o.at[b] - o.at[a]], (patterns, mode, a, b, cap, rc, result.tolist())
                        assert out[:w].tolist() == records[:w] and (out[w:] == Q.SENTINEL).all() and sets[:w].tolist() == hits[:w] and (sets[w:] == 0xA5).all()
                    assert sa.find_records_query(o.split.first_record, patterns, names[mode], bool(flags), b"\n", a, b - a) == records
                assert sa.find_records_query(o.split.first_record, patterns, names[mode], bool(flags), return_hits=True) == Q.find(TEXT, patterns, mode, flags)[:2]
        out = np.full(4, Q.SENTINEL, dtype=np.uint64); result = np.zeros(4, dtype=np.uint64)       # hits not wanted
        q, keep = Q.query(L, [b"error"], Q.ANY, 1)
        assert L.zsmi_seekableFindQueryHost(codec.ctx, o.sk, p(first), o.n, 10, ctypes.byref(q), 0, o.n, p(out), None, 3, p(result)) == 0
        assert out[:3].tolist() == Q.find(TEXT, [b"error"], Q.ANY, 1)[0][:3] and int(out[3]) == Q.SENTINEL
        with pytest.raises(RuntimeError):
            sa.find_records_query(o.split.first_record[:-1], [b"error"])            # not the archive's frame count
    finally:
        sa.close()


def test_the_resident_python_method(L, H, codec):
    data = TEXT
    split = S.Split(data, 10, T, M)
    arc = codec.compress_seekable_frames_host(data, split.sizes, 3, True)
    d_arc = Dev(H, len(arc), arc)
    first = up(H, np.asarray(split.first_record, dtype=np.uint64))
    records, hits, matches = Q.find(data, [b"error", b"timeout"], Q.ALL, 1)
    work, rec, hit, res = Dev(H, len(data)), Dev(H, 8 * len(records)), Dev(H, len(records)), Dev(H, 32)
    sk = codec.open_seekable_device(d_arc.p, len(arc))
    try:
        assert records and sk.find_work_bound(0, split.n) == len(data)
        sk.find_query_resident(first.p, split.n, [b"error", b"timeout"], 0, split.n, work.p, len(data), rec.p, hit.p, len(records), res.p, mode="all", ignore_case=True)
        codec.sync()
        assert down(res, np.uint64)[0].tolist() == [len(records), len(records), matches, len(data)]
        assert down(rec, np.uint64)[0][:len(records)].tolist() == records and down(hit, np.uint8)[0][:len(records)].tolist() == hits
        assert down(work)[0].tobytes()[:len(data)] == data
        with pytest.raises(RuntimeError):
            sk.find_query_resident(first.p, split.n, [b"a\nb"], 0, split.n, work.p, len(data), rec.p, hit.p, len(records), res.p)
    finally:
        codec.sync(); sk.close()
        for d in (d_arc, first, work, rec, hit, res):
            d.free()


def test_host_checks_in_order(L, H, codec, opened):
    """each refusal with every later one present too, so that the order shows; nothing is queued or written by a refused call"""
    o = opened
    n = o.n
    p = ctypes.c_void_p
    one = p(8)                                                                    # a non-NULL pointer no refused call looks behind
    keep = []

    def q(patterns, mode=0, flags=0, **kw):
        keep.append(Q.query(L, patterns, mode, flags, **kw))
        return ctypes.byref(keep[-1][0])
    worst = q([b"\n"] * 9, 7, 6, null=(0,))
    find = L.zsmi_seekableFindQueryResident
    assert find(None, None, None, n + 1, 256, None, 2, n, None, 0, None, None, 3, None) == F.E_INIT
    assert find(codec.ctx, None, one, n + 1, 256, worst, 2, n, None, 0, one, one, 3, one) == F.E_GENERIC             # sk
    assert find(codec.ctx, o.sk, one, n + 1, 256, worst, 2, n, None, 0, one, one, 3, None) == F.E_GENERIC            # dResult
    assert find(codec.ctx, o.sk, one, n + 1, 256, None, 2, n, None, 0, one, one, 3, one) == F.E_GENERIC              # q
    assert find(codec.ctx, o.sk, None, n + 1, 256, worst, 2, n, None, 0, one, one, 3, one) == F.E_GENERIC            # dFirstRecord
    assert find(codec.ctx, o.sk, one, n + 1, 256, worst, 2, n, None, 0, None, one, 3, one) == F.E_GENERIC            # dRecords with capacity > 0
    assert find(codec.ctx, o.sk, one, n + 1, 256, worst, 2, n, None, 0, one, one, 3, one) == F.E_PARAM               # delim
    assert find(codec.ctx, o.sk, one, n + 1, 10, worst, 2, n, None, 0, one, one, 3, one) == F.E_PARAM                # nPatterns 9
    assert find(codec.ctx, o.sk, one, n + 1, 10, q([b"\n"], 3, null=(0,)), 2, n, None, 0, one, one, 3, one) == F.E_PARAM      # mode 3
    assert find(codec.ctx, o.sk, one, n + 1, 10, q([b"\n"], 0, 2, null=(0,)), 2, n, None, 0, one, one, 3, one) == F.E_PARAM   # an unknown flag
    assert find(codec.ctx, o.sk, one, n + 1, 10, q([b"\n"], null=(0,)), 2, n, None, 0, one, one, 3, one) == F.E_GENERIC       # a NULL patterns[0]
    assert find(codec.ctx, o.sk, one, n + 1, 10, q([b"a", b"\n"], sizes=[1, 0]), 2, n, None, 0, one, one, 3, one) == F.E_PARAM      # a size of 0
    assert find(codec.ctx, o.sk, one, n + 1, 10, q([b"a" * 255, b"\n\n"]), 2, n, None, 0, one, one, 3, one) == F.E_PARAM      # a sum of 257
    assert find(codec.ctx, o.sk, one, n + 1, 10, q([b"a", b"\n"]), 2, n, None, 0, one, one, 3, one) == F.E_PARAM              # a delimiter in a pattern
    assert find(codec.ctx, o.sk, one, n + 1, 10, q([b"ab"]), 2, n, None, 0, one, one, 3, one) == F.E_PARAM                    # nFrames
    assert find(codec.ctx, o.sk, one, n, 10, q([b"ab"]), 2, n, None, 0, one, one, 3, one) == F.E_PARAM                        # firstFrame + frameCount
    assert find(codec.ctx, o.sk, one, n, 10, q([b"ab"]), 0xFFFFFFFF, 2, None, 0, one, one, 3, one) == F.E_PARAM               # (no wrap)
    assert find(codec.ctx, o.sk, one, n, 10, q([b"ab"]), 2, n - 2, None, 0, one, one, 3, one) == F.E_GENERIC                  # dWork
    assert find(codec.ctx, o.sk, one, n, 10, q([b"ab"]), 2, n - 2, one, 0, one, one, 3, one) == F.E_TOO_SMALL                 # workCapacity
    host = L.zsmi_seekableFindQueryHost
    assert host(codec.ctx, None, one, n, 10, q([b"ab"]), 0, n, one, one, 3, one) == F.E_GENERIC
    assert host(codec.ctx, o.sk, one, n, 10, None, 0, n, one, one, 3, one) == F.E_GENERIC
    assert host(codec.ctx, o.sk, one, n, 300, q([b"ab"]), 0, n, one, one, 3, one) == F.E_PARAM
    assert host(codec.ctx, o.sk, one, n, 10, q([b"ab"], 3), 0, n, one, one, 3, one) == F.E_PARAM
    assert host(codec.ctx, o.sk, one, n + 1, 10, q([b"ab"]), 0, n, one, one, 3, one) == F.E_PARAM
    assert host(codec.ctx, o.sk, one, n, 10, q([b"ab"]), 1, n, one, one, 3, one) == F.E_PARAM
    codec.sync()
