"""Find records by content in a record archive (zsmi_seekableFindRecordsResident, zsmi_seekableFindRecordsHost,
SeekableArchive.find_records).  The yardstick is tests/_find.py's Python statement of the rule on the source text, or on the slice of it
a window of frames holds, with B = first_record[firstFrame] from the splitter's Python rule - never another call of the library.
Archives are made with the host-array compress call from S.Split(...).sizes.  dWork, dRecords, dResult and dFirstRecord lie between
canaries; a window's call gets exactly its work bound of dWork and must leave everything behind it, and behind the numbers it writes,
as it was."""
import ctypes
import numpy as np
import pytest
import _find as F, _split as S, _seekable as SK, _seekable_resident as SR, _resident_cdict_set as RS
from _hip import hip_of, Dev, CANARY, PAD
from _resident import up, down

pytestmark = pytest.mark.gpu
CASES = S.cases()
LISTED = ("cut_record_shares_its_last_piece", "no_delimiter_2500", "tail_without_delimiter", "T1", "delim_255", "long_piece_between_short")
EXTRA = {"cut_record_shares_its_last_piece": [b"y" * 12, b"y" * 24, b"tail", b"z"], "no_delimiter_2500": [b"a" * 5, b"a" * 256], "tail_without_delimiter": [b"ef", b"c"],
         "long_piece_between_short": [b"c" * 9, b"e"]}


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


FOUND = F.split_inputs()


def patterns(name):
    return [FOUND[k][1] for k in (name, name + "_pair") if k in FOUND] + EXTRA.get(name, [])


def open_host(L, codec, arc, dset=None):
    err = ctypes.c_int(-1)
    sk = L.zsmi_openSeekable_usingDDictSet(codec.ctx, arc, len(arc), dset.handle if dset is not None else None, ctypes.byref(err))
    assert sk and err.value == 0, err.value
    return sk


class Opened:
    """a text, its split by the Python rule, its archive opened, and buffers every window's call shares: dFirstRecord as the rule leaves it,
    dWork of the whole content, dRecords of `room` numbers, dResult - each between canaries and filled with the canary before a call"""

    def __init__(self, L, H, codec, data, delim, T, M, checksum=True, arc=None, dset=None, room=None):
        self.L, self.H, self.codec, self.data, self.delim = L, H, codec, data, delim
        self.split = S.Split(data, delim, T, M)
        self.n = self.split.n
        self.at = [0] + np.cumsum(self.split.sizes, dtype=np.int64).tolist()
        self.arc = arc if arc is not None else codec.compress_seekable_frames_host(data, self.split.sizes, 3, checksum)
        self.sk = open_host(L, codec, self.arc, dset)
        self.room = max(self.split.records, 1) if room is None else room
        self.first = up(H, np.asarray(self.split.first_record, dtype=np.uint64))
        self.work, self.rec, self.res = Dev(H, max(len(data), 1)), Dev(H, 8 * self.room), Dev(H, 32)

    def close(self):
        self.codec.sync(); self.L.zsmi_closeSeekable(self.sk)
        for d in (self.first, self.work, self.rec, self.res):
            d.free()

    def find(self, pattern, a=0, b=None, capacity=None, work_capacity=None, delim=None):
        """one zsmi_seekableFindRecordsResident call over frames [a, b): (rc, dResult, the numbers written, whether dRecords kept its fill).
        workCapacity: the window's bound, exactly"""
        L, H, p = self.L, self.H, ctypes.c_void_p
        b = self.n if b is None else b
        bound = L.zsmi_seekableFindWorkBound(self.sk, a, b - a)
        assert bound == self.at[b] - self.at[a]
        cap = self.room if capacity is None else capacity
        wcap = bound if work_capacity is None else work_capacity
        for d in (self.work, self.rec, self.res):
            assert H.hipMemset(ctypes.c_void_p(d.p), CANARY, d.n) == 0
        rc = L.zsmi_seekableFindRecordsResident(self.codec.ctx, self.sk, p(self.first.p), self.n, self.delim if delim is None else delim, pattern, len(pattern), a, b - a,
                                                p(self.work.p), wcap, p(self.rec.p) if cap else None, cap, p(self.res.p))
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
            assert untouched, "dRecords written by a call that has no numbers to write"
            return rc, result, [], untouched
        written = result[1]
        assert written <= cap and (rec[written:].view(np.uint8) == CANARY).all(), "written behind the numbers"
        return rc, result, [int(v) for v in rec[:written]], untouched

    def check(self, pattern, a=0, b=None, what=""):
        b = self.n if b is None else b
        records, matches = F.window(self.data, self.split.sizes, self.split.first_record, a, b, pattern, self.delim)
        rc, result, got, _ = self.find(pattern, a, b)
        assert rc == 0 and result == [len(records), len(records), matches, self.at[b] - self.at[a]] and got == records, (what, pattern, a, b, rc, result, got[:8], records[:8])
        return records, matches


@pytest.fixture(scope="module")
def opened(L, H, codec):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Opened(L, H, codec, *CASES[name])
        return made[name]
    yield get
    for o in made.values():
        o.close()


# ------------------------------------------------------------------ 1. windows
def test_the_listed_inputs_are_in_the_set():
    for name in LISTED:
        assert name in CASES and patterns(name)
    data, delim, T, M = CASES["cut_record_shares_its_last_piece"]
    first = S.Split(data, delim, T, M).first_record
    starts = F.record_starts(first)
    assert 0 < len(starts) - 1 < len(first) - 2                                    # frames that begin a record behind the first, and frames that do not


@pytest.mark.parametrize("name", LISTED)
def test_the_whole_window(opened, name):
    o = opened(name)
    for pattern in patterns(name):
        records, matches = o.check(pattern, what=name)
        assert (records, matches) == F.find(o.data, pattern, o.delim, 0)


def test_a_pattern_across_the_frames_of_a_cut_record(opened):
    o = opened("cut_record_shares_its_last_piece")
    f, last = o.split.frame_of(1), o.split.frame_of(2)                            # record 1: 25 bytes in frames of 10 and 10; its last 5 share frame `last`
    assert last - f == 2 and o.split.sizes[f:last] == [10, 10]
    assert o.check(b"y" * 24) == ([1], 1) and o.check(b"y" * 12) == ([1], 13)
    assert o.check(b"y" * 24, f, last) == ([], 0)                                  # the window ends inside the record: the occurrence crosses its border
    assert o.check(b"y" * 12, f + 1, last + 1) == ([1], 3)                         # 14 of its bytes; a window that begins inside the record counts from its frame's entry
    o = opened("no_delimiter_2500")
    assert o.n == 3 and o.check(b"a" * 256) == ([0], 2500 - 255)


@pytest.mark.parametrize("name", LISTED)
def test_every_window(opened, name):
    o = opened(name)
    pats = patterns(name)[:3]
    for a in range(o.n + 1):
        for b in range(a, o.n + 1):
            o.check(pats[(a + b) % len(pats)], a, b, what=name)
    rc, result, got, _ = o.find(pats[0], o.n, o.n)                                 # no frame at all
    assert rc == 0 and result == [0, 0, 0, 0] and got == []


@pytest.mark.parametrize("name", LISTED)
def test_windows_cut_where_records_begin(opened, name):
    o = opened(name)
    for pattern in patterns(name):
        cuts = F.boundary_windows(o.data, o.split.sizes, o.split.first_record, pattern, o.delim)       # (the CPU check of the claim)
        records, matches = [], 0
        for a, b in cuts:
            r, m = o.check(pattern, a, b, what=name)
            records += r; matches += m
        assert (records, matches) == o.check(pattern, what=name)


def test_capacity_and_the_work_bound(opened):
    o = opened("T1")
    body = bytes(b for b in o.data if b != o.delim)
    pattern = bytes([max(set(body), key=body.count)])                              # the text's most frequent byte
    records, matches = F.find(o.data, pattern, o.delim)
    assert len(records) > 4 and matches >= len(records)
    bound = len(o.data)
    rc, result, got, untouched = o.find(pattern, capacity=0)
    assert rc == 0 and result == [len(records), 0, matches, bound] and untouched
    rc, result, got, _ = o.find(pattern, capacity=len(records) - 2)
    assert rc == 0 and result == [len(records), len(records) - 2, matches, bound] and got == records[:-2]
    rc, result, got, untouched = o.find(pattern, work_capacity=bound - 1)
    assert rc == F.E_TOO_SMALL and untouched and result == [0xA5A5A5A5A5A5A5A5] * 4      # nothing was queued
    a, b = 2, o.n - 1
    rc, result, got, untouched = o.find(pattern, a, b, work_capacity=o.at[b] - o.at[a] - 1)
    assert rc == F.E_TOO_SMALL and untouched


# ------------------------------------------------------------------ 2. damage, dictionaries
def test_one_flipped_content_bit(L, H, codec):
    data = S.lines(31, 90, 120)                                                    # seeded bytes: the frames' blocks are stored, a payload bit is a content bit
    o = Opened(L, H, codec, data, 10, 2048, 4096)
    try:
        assert o.n >= 3
        rows, flag = SK.parse(o.arc)
        assert flag and len(rows) == o.n
        pattern = bytes(b for b in data if b != 10)[:1]
        whole = o.check(pattern)
    finally:
        o.close()
    bad = bytearray(o.arc)
    bad[rows[0][0] + rows[1][0] // 2] ^= 0x10                                      # in the middle of frame 1's compressed bytes
    o = Opened(L, H, codec, data, 10, 2048, 4096, arc=bytes(bad))
    try:
        for a, b in ((0, o.n), (1, 2), (0, 2), (1, o.n)):
            rc, result, got, untouched = o.find(pattern, a, b)
            assert rc == 0 and result == [(1 << 64) - F.E_CHECKSUM, 0, 0, o.at[b] - o.at[a]] and untouched, (a, b, result)
        o.check(pattern, 0, 1); o.check(pattern, 2, o.n)                           # windows that do not touch the damaged frame
    finally:
        o.close()


def test_a_damaged_frame_among_thousands(L, H, codec):
    """5000 frames of one byte, frame 4000 damaged: the reduction over the frames' codes finds it from every window that holds it.  (Which
    code a flipped bit of so small a frame earns - corruption_detected or checksum_wrong - is the decoder's to say; the frame read's own
    tests pin that, and test_one_flipped_content_bit pins checksum_wrong for a content bit)"""
    data, delim, T, M = CASES["all_delimiters_5000"]
    o = Opened(L, H, codec, data, delim, T, M, room=8)
    try:
        assert o.n == 5000
        rows, flag = SK.parse(o.arc)
        assert flag and len(rows) == 5000
    finally:
        o.close()
    bad = bytearray(o.arc)
    bad[sum(r[0] for r in rows[:4001]) - 5] ^= 0x01                                # in frame 4000, in front of its checksum
    o = Opened(L, H, codec, data, delim, T, M, arc=bytes(bad), room=8)
    try:
        codes = set()
        for a, b in ((0, 5000), (4000, 4001), (3999, 4002), (17, 4001)):
            rc, result, got, untouched = o.find(b"x", a, b)
            assert rc == 0 and result[1:] == [0, 0, b - a] and untouched, (a, b, result)
            codes.add((1 << 64) - result[0])
        assert len(codes) == 1 and codes <= {F.E_CORRUPT, F.E_CHECKSUM}, codes
        for a, b in ((0, 4000), (4001, 5000)):
            rc, result, got, untouched = o.find(b"x", a, b)
            assert rc == 0 and result == [0, 0, 0, b - a] and untouched, (a, b, result)
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
        o = Opened(L, H, codec, data, 10, 1024, 4096, arc=wrote.archive, dset=dset)
        try:
            for pattern in (b"qu", b"e", data[5000:5009].replace(b"\n", b"x")):
                o.check(pattern, what="dictionaries")
                o.check(pattern, 3, n - 2, what="dictionaries, a window")
        finally:
            o.close()
    finally:
        codec.sync(); dset.close(); cset.close()
        for h in dds + list(set(cds)):
            h.close()


# ------------------------------------------------------------------ 3. the pipeline, the host form, the host checks
def test_text_to_archive_to_grep_to_lines(L, H, codec):
    """split_records_device -> compress_seekable_frames_resident -> open -> find_records_resident -> read_records_resident: the numbers the
    search left are read where they lie, and the bytes delivered are the lines of the text that hold the pattern, in order"""
    from zstandard_amd import BatchCodec
    text = S.text_lines(256 << 10)
    T, M = 4096, 65536
    lines = text.splitlines(True)
    pattern = b"qz"
    wanted = [ln for ln in lines if pattern in ln]
    assert 2 < len(wanted) < len(lines)
    src, cnt, res = Dev(H, len(text), text), Dev(H, 8), Dev(H, 24)
    held = [src, cnt, res]
    try:
        codec.count_records_device(src.p, len(text), cnt.p)
        codec.sync()
        records = int(down(cnt, np.uint64)[0][0])
        assert records == len(lines)
        mp = BatchCodec.split_pieces_bound(records, len(text), M)
        fs, fr = Dev(H, 4 * mp), Dev(H, 8 * (mp + 1))
        held += [fs, fr]
        codec.split_records_device(src.p, len(text), mp, fs.p, fr.p, res.p, target_size=T, max_frame_size=M)
        codec.sync()                                                               # dResult: n is the next calls' host argument
        n = int(down(res, np.uint64)[0][0])
        bound = codec.seekable_frames_resident_bound(len(text), n, True)
        arc, size = Dev(H, bound), Dev(H, 8)
        held += [arc, size]
        codec.compress_seekable_frames_resident(src.p, len(text), fs.p, n, M, arc.p, bound, size.p, level=3, checksum=True)
        codec.sync()
        m = int(down(size, np.uint64)[0][0])
        sk = codec.open_seekable_device(arc.p, m)
        try:
            work_cap = sk.find_work_bound(0, n)
            assert work_cap == len(text)
            work, found, out = Dev(H, work_cap), Dev(H, 8 * records), Dev(H, 32)
            held += [work, found, out]
            sk.find_records_resident(fr.p, n, pattern, 0, n, work.p, work_cap, found.p, records, out.p)      # fr: as the splitter left it
            codec.sync()                                                           # dResult: the total is the next call's host argument
            total, written, matches, scanned = (int(v) for v in down(out, np.uint64)[0])
            assert (total, written, scanned) == (len(wanted), len(wanted), len(text)) and matches == sum(ln.count(pattern) for ln in wanted)
            k = total
            room = sum(len(ln) for ln in wanted)
            rwork_cap = sk.records_work_bound(k)
            rwork, dst, off, wr, st, rout = Dev(H, rwork_cap), Dev(H, room), Dev(H, 8 * (k + 1)), Dev(H, 8 * k), Dev(H, 4 * k), Dev(H, 32)
            held += [rwork, dst, off, wr, st, rout]
            sk.read_records_resident(fr.p, n, found.p, k, k, rwork.p, rwork_cap, dst.p, room, off.p, wr.p, st.p, rout.p)       # found: as the search left it
            codec.sync()
            buf, ok = down(dst)
            assert ok and not down(st, np.uint32)[0].any()
            assert buf.tobytes() == b"".join(wanted)
            assert down(found, np.uint64)[1], "wrote outside dRecords"
        finally:
            codec.sync(); sk.close()
    finally:
        for d in held:
            d.free()


@pytest.mark.parametrize("name", LISTED[:4])
def test_host_form_and_python_surface(L, H, codec, opened, name):
    from zstandard_amd import SeekableArchive
    o = opened(name)
    first = np.asarray(o.split.first_record, dtype=np.uint64)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    sa = SeekableArchive(o.arc)
    try:
        for pattern in patterns(name):
            for a, b in ((0, o.n), (min(1, o.n), o.n), (0, max(o.n - 1, 0))):
                records, matches = F.window(o.data, o.split.sizes, o.split.first_record, a, b, pattern, o.delim)
                for cap in (len(records), max(len(records) - 1, 0), len(records) + 2):
                    out = np.full(cap + 1, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64); result = np.zeros(4, dtype=np.uint64)
                    rc = L.zsmi_seekableFindRecordsHost(codec.ctx, o.sk, p(first), o.n, o.delim, pattern, len(pattern), a, b - a, p(out) if cap else None, cap, p(result))
                    w = min(cap, len(records))
                    assert rc == 0 and result.tolist() == [len(records), w, matches, o.at[b] - o.at[a]], (name, pattern, a, b, cap, rc, result.tolist())
                    assert out[:w].tolist() == records[:w] and (out[w:] == 0xA5A5A5A5A5A5A5A5).all()
                assert sa.find_records(o.split.first_record, pattern, bytes([o.delim]), a, b - a) == records
            assert sa.find_records(o.split.first_record, pattern, bytes([o.delim])) == F.find(o.data, pattern, o.delim)[0]
        with pytest.raises(RuntimeError):
            sa.find_records(o.split.first_record[:-1], patterns(name)[0], bytes([o.delim]))      # not the archive's frame count
    finally:
        sa.close()


def test_host_checks_in_order(L, H, codec, opened):
    """each refusal with every later one present too, so that the order shows; nothing is queued or written by a refused call"""
    o = opened("T1")
    n = o.n
    p = ctypes.c_void_p
    one = p(8)                                                                    # a non-NULL pointer no refused call looks behind
    find = L.zsmi_seekableFindRecordsResident
    assert find(None, None, None, n + 1, 256, None, 0, 2, n, None, 0, None, 3, None) == F.E_INIT
    assert find(codec.ctx, None, one, n + 1, 256, b"\n", 0, 2, n, None, 0, one, 3, one) == F.E_GENERIC          # sk
    assert find(codec.ctx, o.sk, one, n + 1, 256, b"\n", 0, 2, n, None, 0, one, 3, None) == F.E_GENERIC         # dResult
    assert find(codec.ctx, o.sk, one, n + 1, 256, None, 0, 2, n, None, 0, one, 3, one) == F.E_GENERIC           # pattern
    assert find(codec.ctx, o.sk, None, n + 1, 256, b"\n", 0, 2, n, None, 0, one, 3, one) == F.E_GENERIC         # dFirstRecord
    assert find(codec.ctx, o.sk, one, n + 1, 256, b"\n", 0, 2, n, None, 0, None, 3, one) == F.E_GENERIC         # dRecords with capacity > 0
    assert find(codec.ctx, o.sk, one, n + 1, 256, b"\n", 0, 2, n, None, 0, one, 3, one) == F.E_PARAM            # delim
    assert find(codec.ctx, o.sk, one, n + 1, 10, b"\n", 0, 2, n, None, 0, one, 3, one) == F.E_PARAM             # patternSize 0
    assert find(codec.ctx, o.sk, one, n + 1, 10, b"a" * 257, 257, 2, n, None, 0, one, 3, one) == F.E_PARAM      # patternSize 257
    assert find(codec.ctx, o.sk, one, n + 1, 10, b"a\n", 2, 2, n, None, 0, one, 3, one) == F.E_PARAM            # a delimiter in the pattern
    assert find(codec.ctx, o.sk, one, n + 1, 10, b"ab", 2, 2, n, None, 0, one, 3, one) == F.E_PARAM             # nFrames
    assert find(codec.ctx, o.sk, one, n, 10, b"ab", 2, 2, n, None, 0, one, 3, one) == F.E_PARAM                 # firstFrame + frameCount
    assert find(codec.ctx, o.sk, one, n, 10, b"ab", 2, 0xFFFFFFFF, 2, None, 0, one, 3, one) == F.E_PARAM        # (no wrap)
    assert find(codec.ctx, o.sk, one, n, 10, b"ab", 2, 2, n - 2, None, 0, one, 3, one) == F.E_GENERIC           # dWork
    assert find(codec.ctx, o.sk, one, n, 10, b"ab", 2, 2, n - 2, one, 0, one, 3, one) == F.E_TOO_SMALL          # workCapacity
    host = L.zsmi_seekableFindRecordsHost
    assert host(codec.ctx, None, one, n, 10, b"ab", 2, 0, n, one, 3, one) == F.E_GENERIC
    assert host(codec.ctx, o.sk, one, n, 300, b"ab", 2, 0, n, one, 3, one) == F.E_PARAM
    assert host(codec.ctx, o.sk, one, n + 1, 10, b"ab", 2, 0, n, one, 3, one) == F.E_PARAM
    assert host(codec.ctx, o.sk, one, n, 10, b"ab", 2, 1, n, one, 3, one) == F.E_PARAM
    assert L.zsmi_seekableFindWorkBound(o.sk, 0, n) == len(o.data) and L.zsmi_seekableFindWorkBound(o.sk, 1, n) == 0
    assert L.zsmi_seekableFindWorkBound(o.sk, n, 0) == 0 and L.zsmi_seekableFindWorkBound(o.sk, 0xFFFFFFFF, 1) == 0
    codec.sync()
