"""Records by number on the device (zsmi_seekableReadRecordsResident, zsmi_seekableReadRecordsHost, SeekableArchive.read_records).  The
yardstick is the source text: record r is data[ends[r - 1]:ends[r]] with ends from tests/_split.py's record_ends, and what the call must
leave - lengths, offsets, statuses, dResult, and which requests the caps refuse - is worked out here from the splitter's Python rule
(expect()), never through the library.  Archives are made with the host-array compress call from S.Split(...).sizes.  Every array is
exactly as long as the header sizes it, between canaries; nothing depends on a wait inside the calls."""
import bisect, ctypes
import numpy as np
import pytest
import _split as S, _seekable as SK, _seekable_resident as SR, _resident_cdict_set as RS
from _hip import hip_of, Dev, CANARY, PAD
from _resident import up, down

pytestmark = pytest.mark.gpu
CASES = S.cases()
E_GENERIC, E_CORRUPT, E_CHECKSUM, E_UNSUPPORTED, E_PARAM, E_INIT, E_TOO_SMALL, E_FRAME_INDEX = 1, 20, 22, 40, 42, 62, 70, 100
LISTED = ("cut_record_shares_its_last_piece", "no_delimiter_2500", "tail_without_delimiter", "all_delimiters_5000_T7", "delim_255", "empty")


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


# ------------------------------------------------------------------ the yardstick
class Text:
    """a text, its split by the Python rule, and its records as slices of the text"""

    def __init__(self, data, delim=10, T=0, M=1 << 16):
        self.data, self.delim = data, delim
        self.split = S.Split(data, delim, T, M)
        self.ends = S.record_ends(data, delim)[1]
        self.at = [0] + np.cumsum(self.split.sizes, dtype=np.int64).tolist()      # the frames' content offsets
        assert len(self.ends) == self.split.records

    def record(self, r):
        return self.data[self.ends[r - 1] if r else 0:self.ends[r]]

    def frames(self, r):
        """(f, g): f is rule 4's lookup, g the last frame that starts with at most r delimiters in front"""
        first = self.split.first_record
        return self.split.frame_of(r), bisect.bisect_right(first, r, 0, self.split.n) - 1


class Want:
    """offsets (n + 1), written, status, result, leaders (the requests that read frames)"""


def expect(text, idx, align=1, max_reads=None, work_cap=None, dst_cap=None):
    n, records = len(idx), text.split.records
    w = Want()
    w.status, w.written, w.leaders = [0] * n, [0] * n, []
    reads = work = 0
    prev = lead_code = None
    for k, r in enumerate(idx):
        if r >= records:
            w.status[k], prev = E_FRAME_INDEX, None
            continue
        f, g = text.frames(r)
        if prev != (f, g):                                                         # a leader
            need, size = g - f + 1, text.at[g + 1] - text.at[f]
            lead_code = E_TOO_SMALL if (max_reads is not None and reads + need > max_reads) or (work_cap is not None and work + size > work_cap) else 0
            reads += need; work += size
            w.leaders.append(k)
        prev = (f, g)
        w.status[k] = lead_code
        w.written[k] = 0 if lead_code else len(text.record(r))
    w.offsets = SR.rounded_offsets(w.written, align)
    for k in range(n):
        if not w.status[k] and dst_cap is not None and int(w.offsets[k]) + w.written[k] > dst_cap:
            w.status[k] = E_TOO_SMALL
    w.result = [w.status.count(0), reads, work, int(w.offsets[n])]
    return w


def archive_of(codec, text, checksum=True):
    return codec.compress_seekable_frames_host(text.data, text.split.sizes, 3, checksum)


def open_host(L, codec, arc, dset=None):
    err = ctypes.c_int(-1)
    sk = L.zsmi_openSeekable_usingDDictSet(codec.ctx, arc, len(arc), dset.handle if dset is not None else None, ctypes.byref(err))
    assert sk and err.value == 0, err.value
    return sk


class Got:
    pass


def call(L, H, codec, sk, first, n_frames, delim, idx, max_reads, align, work_cap, dst_cap, work_shift=0, d_first=None, d_idx=None):
    """one zsmi_seekableReadRecordsResident call: dFirstRecord n_frames + 1 entries, dRecordIndex / dWritten / dStatus len(idx), dDstOffsets
    len(idx) + 1, dResult four words, dWork work_cap bytes (work_shift bytes into its buffer) and dDst dst_cap bytes, each between canaries
    that are checked here.  d_first / d_idx: device pointers somebody else filled"""
    n = len(idx)
    p = ctypes.c_void_p
    own_first = up(H, np.asarray(first, dtype=np.uint64)) if d_first is None else None
    own_idx = up(H, np.asarray(idx if n else [0], dtype=np.uint64)) if d_idx is None else None
    work, dst = Dev(H, max(work_cap + work_shift, 1)), Dev(H, max(dst_cap, 1))
    off, wr, st, res = Dev(H, 8 * (n + 1)), Dev(H, 8 * max(n, 1)), Dev(H, 4 * max(n, 1)), Dev(H, 32)
    g = Got()
    try:
        g.rc = L.zsmi_seekableReadRecordsResident(codec.ctx, sk, p(own_first.p if own_first else d_first), n_frames, delim, p(own_idx.p if own_idx else d_idx), n,
                                                  max_reads, align, p(work.p + work_shift), work_cap, p(dst.p), dst_cap, p(off.p), p(wr.p), p(st.p), p(res.p))
        codec.sync()
        raw = np.frombuffer(dst.all(), dtype=np.uint8)
        assert (raw[:PAD] == CANARY).all() and (raw[PAD + dst_cap:] == CANARY).all(), "wrote outside [dDst, dDst + dstCapacity)"
        g.buf = raw[PAD:PAD + dst_cap].copy()
        raw = np.frombuffer(work.all(), dtype=np.uint8)
        assert (raw[:PAD + work_shift] == CANARY).all() and (raw[PAD + work_shift + work_cap:] == CANARY).all(), "wrote outside [dWork, dWork + workCapacity)"
        vals = []
        for name, d, t in (("dDstOffsets", off, np.uint64), ("dWritten", wr, np.uint64), ("dStatus", st, np.uint32), ("dResult", res, np.uint64),
                           ("dFirstRecord", own_first, np.uint64), ("dRecordIndex", own_idx, np.uint64)):
            if d is not None:
                v, ok = down(d, t)
                assert ok, "wrote outside " + name
                vals.append(v.copy())
        g.offsets, g.written, g.status, g.result = vals[0], vals[1][:n].tolist(), vals[2][:n].tolist(), vals[3].tolist()
        if n == 0:
            assert (vals[1].view(np.uint8) == CANARY).all() and (vals[2].view(np.uint8) == CANARY).all()
        return g
    finally:
        for d in (own_first, own_idx, work, dst, off, wr, st, res):
            if d is not None:
                d.free()


def check(g, w, text, idx, what=""):
    """everything the call left against the yardstick: the four arrays, the bytes at every place that has any, the canary everywhere else"""
    assert g.rc == 0, (what, g.rc)
    assert g.status == w.status, (what, "dStatus", [(k, a, b) for k, (a, b) in enumerate(zip(g.status, w.status)) if a != b][:8])
    assert g.written == w.written, (what, "dWritten", [(k, a, b) for k, (a, b) in enumerate(zip(g.written, w.written)) if a != b][:8])
    assert (g.offsets == w.offsets).all(), (what, "dDstOffsets")
    assert g.result == w.result, (what, "dResult", g.result, w.result)
    inside = np.zeros(len(g.buf), dtype=bool)
    for k, r in enumerate(idx):
        if w.status[k] == 0:
            a = int(w.offsets[k])
            assert g.buf[a:a + w.written[k]].tobytes() == text.record(r), (what, k, r)
            inside[a:a + w.written[k]] = True
    assert (g.buf[~inside] == CANARY).all(), (what, "written outside the places")


def roomy(L, H, codec, sk, text, idx, align=1, what="", **kw):
    """a call with caps that suffice, checked; returns (got, want)"""
    w = expect(text, idx, align)
    work = L.zsmi_seekableRecordsWorkBound(sk, w.result[1])
    assert work >= w.result[2]
    g = call(L, H, codec, sk, text.split.first_record, text.split.n, text.delim, idx, w.result[1], align, work, w.result[3], **kw)
    check(g, w, text, idx, what)
    return g, w


# ------------------------------------------------------------------ 1. every input of the splitter's tests
@pytest.mark.parametrize("name", sorted(CASES))
def test_split_inputs(L, H, codec, name):
    data, delim, T, M = CASES[name]
    text = Text(data, delim, T, M)
    records = text.split.records
    sk = open_host(L, codec, archive_of(codec, text))
    try:
        rng = np.random.default_rng(17)
        picks = [int(v) for v in rng.integers(0, max(records, 1), 64)] + [records, 2 ** 63]
        picks[5] = picks[4]; picks[9] = picks[7]                                   # repeats in a row and apart
        for what, idx in (("ascending", list(range(records))), ("descending", list(range(records))[::-1]), ("picks", picks)):
            g, w = roomy(L, H, codec, sk, text, idx, what=(name, what))
            if what == "picks":
                assert w.status[-2:] == [E_FRAME_INDEX] * 2
                if records == 0:
                    assert w.status == [E_FRAME_INDEX] * len(idx) and w.result == [0, 0, 0, 0]
    finally:
        codec.sync(); L.zsmi_closeSeekable(sk)


def test_the_listed_inputs_are_in_the_set():
    for name in LISTED:
        assert name in CASES
    assert any(Text(*CASES[n]).frames(0)[0] < Text(*CASES[n]).frames(0)[1] for n in CASES if n.startswith("no_delimiter_"))      # f < g


# ------------------------------------------------------------------ 2. the borders of k_rec_measure
def border_text(last):
    """one frame of 3 x 1024 + 40 bytes: delimiters on 15, 16, 17, 1023, 1024, 1025, 2047, 2048, 2049 and - with `last` - on the last two
    bytes, so that records start and end on both sides of a lane's 16 bytes and of a 1024-byte step, one-byte records lie on the borders,
    and the records between them span steps"""
    size = 3 * 1024 + 40
    b = bytearray(b"a" * size)
    for p in (15, 16, 17, 1023, 1024, 1025, 2047, 2048, 2049):
        b[p] = 10
    b[size - 2] = 10
    b[size - 1] = 10 if last else 98
    return bytes(b)


@pytest.mark.parametrize("offset", (1, 3, 7, 13))
def test_measure_borders(L, H, codec, offset):
    for last in (True, False):
        text = Text(border_text(last), 10, 4096, 4096)
        assert text.split.n == 1 and text.split.records == 11
        assert max(len(text.record(r)) for r in range(text.split.records)) > 1024
        arc = archive_of(codec, text)
        buf = Dev(H, len(arc) + 16, bytes(offset) + arc)                           # the archive at an odd offset of a buffer
        err = ctypes.c_int(-1)
        sk = L.zsmi_openSeekableDevice(codec.ctx, ctypes.c_void_p(buf.p + offset), len(arc), ctypes.byref(err))
        assert sk and err.value == 0
        try:
            records = text.split.records
            for shift in (0, offset):                                              # the run 16-byte aligned in dWork, and at the odd offset
                roomy(L, H, codec, sk, text, list(range(records)), what=(offset, last, shift, "ascending"), work_shift=shift)
                roomy(L, H, codec, sk, text, list(range(records))[::-1], what=(offset, last, shift, "descending"), work_shift=shift)
        finally:
            codec.sync(); L.zsmi_closeSeekable(sk); buf.free()


# ------------------------------------------------------------------ 3. followers
@pytest.fixture(scope="module")
def three_frames(L, codec):
    text = Text(S.lines(31, 90, 120), 10, 2048, 4096)
    assert text.split.n == 3
    sk = open_host(L, codec, archive_of(codec, text))
    yield text, sk
    codec.sync(); L.zsmi_closeSeekable(sk)


def test_followers(L, H, codec, three_frames):
    text, sk = three_frames
    idx = list(range(text.split.records))
    g, w = roomy(L, H, codec, sk, text, idx, what="ascending")
    assert g.result[1] == 3
    rng = np.random.default_rng(5)
    mixed = [idx[i] for i in rng.permutation(len(idx))]
    changes = sum(1 for k, r in enumerate(mixed) if k == 0 or text.frames(r) != text.frames(mixed[k - 1]))
    g2, w2 = roomy(L, H, codec, sk, text, mixed, what="shuffled")
    assert g2.result[1] == changes > 3
    for k, r in enumerate(mixed):                                                  # the bytes are the same both ways
        a, b = int(g2.offsets[k]), int(g.offsets[r])
        assert g2.buf[a:a + g2.written[k]].tobytes() == g.buf[b:b + g.written[r]].tobytes()


# ------------------------------------------------------------------ 4. caps, align, no requests
def test_caps_one_short_and_exact(L, H, codec, three_frames):
    text, sk = three_frames
    idx = list(range(text.split.records))
    full = expect(text, idx)
    reads, work, room = full.result[1:]
    first, n = text.split.first_record, text.split.n
    last_leader = full.leaders[-1]
    for what, caps in (("maxFrameReads", (reads - 1, work, room)), ("workCapacity", (reads, work - 1, room)), ("dstCapacity", (reads, work, room - 1))):
        w = expect(text, idx, 1, caps[0], caps[1], caps[2])
        g = call(L, H, codec, sk, first, n, 10, idx, caps[0], 1, caps[1], caps[2])
        check(g, w, text, idx, what + " one short")
        assert g.result[1:3] == [reads, work]
        if what == "dstCapacity":
            assert g.status == [0] * (len(idx) - 1) + [E_TOO_SMALL] and g.written == full.written and g.result[3] == room
        else:
            assert g.status == [0] * last_leader + [E_TOO_SMALL] * (len(idx) - last_leader) and g.written[last_leader:] == [0] * (len(idx) - last_leader)
            assert g.written[:last_leader] == full.written[:last_leader]
    g = call(L, H, codec, sk, first, n, 10, idx, reads, 1, work, room)            # exactly enough of each
    check(g, full, text, idx, "exact")


@pytest.mark.parametrize("align", (1, 8, 4096))
def test_align(L, H, codec, three_frames, align):
    text, sk = three_frames
    idx = [3, 4, 40, 5, 5, text.split.records, 0]
    g, w = roomy(L, H, codec, sk, text, idx, align, what=align)
    assert all(int(o) % align == 0 for o in g.offsets)


def test_no_requests(L, H, codec, three_frames):
    text, sk = three_frames
    g = call(L, H, codec, sk, text.split.first_record, text.split.n, 10, [], 0, 1, 0, 0)
    assert g.rc == 0 and g.offsets.tolist() == [0] and g.result == [0, 0, 0, 0]
    assert (g.buf == CANARY).all()


# ------------------------------------------------------------------ 5. a record cut into 16384 frames
def test_a_cut_record_of_a_mebibyte(L, H, codec):
    data = b"one\ntwo\n" + b"x" * ((1 << 20) - 1) + b"\n" + b"four\nfive"
    text = Text(data, 10, 64, 64)
    f, g = text.frames(2)
    assert g - f + 1 == 16384 and len(text.record(2)) == 1 << 20
    sk = open_host(L, codec, archive_of(codec, text, checksum=False))
    try:
        got, w = roomy(L, H, codec, sk, text, [0, 2, 1, 3, 4, 2], what="cut")
        assert w.result[1] == 2 * 16384 + 3
    finally:
        codec.sync(); L.zsmi_closeSeekable(sk)


# ------------------------------------------------------------------ 6. dictionaries, damage, a foreign firstRecord
def test_a_handle_with_a_ddict_set(L, H, codec):
    text = Text(S.text_lines(24 << 10, seed=4), 10, 1024, 4096)
    n = text.split.n
    assert n >= 8
    two = (SR.PICKS[0], SR.PICKS[1])
    index = SR.u32([two[i % 2] for i in range(n)])
    cset, cds = RS.make_set(codec, 3)
    dset, dds = SR.ddict_set(codec)
    try:
        wrote = SR.write(L, H, codec, text.data, text.split.sizes, 3, 1, cset, index)
        assert wrote.rc == 0 and wrote.archive is not None
        ids = {RS.frame_dict_id(wrote.archive[:SK.parse(wrote.archive)[0][0][0]])}
        assert ids != {0}                                                          # the frames name their dictionaries
        sk = open_host(L, codec, wrote.archive, dset)
        try:
            rng = np.random.default_rng(2)
            roomy(L, H, codec, sk, text, [int(v) for v in rng.integers(0, text.split.records, 200)], what="dictionaries")
        finally:
            codec.sync(); L.zsmi_closeSeekable(sk)
    finally:
        codec.sync(); dset.close(); cset.close()
        for h in dds + list(set(cds)):
            h.close()


def test_one_flipped_payload_bit(L, H, codec, three_frames):
    text, _ = three_frames
    arc = archive_of(codec, text)
    rows, flag = SK.parse(arc)
    assert flag and len(rows) == 3
    bad = bytearray(arc)
    bad[rows[0][0] + rows[1][0] // 2] ^= 0x10                                      # in the middle of frame 1's compressed bytes
    sk = open_host(L, codec, bytes(bad))
    try:
        frames_read = SR.read(L, H, codec, sk, [0, 1, 2], 1, sum(r[1] for r in rows))
        code = int(frames_read.status[1])
        assert frames_read.status.tolist() == [0, code, 0] and code in (E_CORRUPT, E_CHECKSUM)
        idx = list(range(text.split.records))[::3] + [0, text.split.records - 1]
        w = expect(text, idx)
        for k, r in enumerate(idx):
            if 1 in range(text.frames(r)[0], text.frames(r)[1] + 1):
                w.status[k], w.written[k] = code, 0
        assert code in w.status and 0 in w.status
        w.offsets = SR.rounded_offsets(w.written, 1)
        w.result = [w.status.count(0), w.result[1], w.result[2], int(w.offsets[-1])]
        g = call(L, H, codec, sk, text.split.first_record, 3, 10, idx, w.result[1], 1, w.result[2], w.result[3])
        check(g, w, text, idx, "a flipped bit")
    finally:
        codec.sync(); L.zsmi_closeSeekable(sk)


def test_a_foreign_first_record(L, H, codec, three_frames):
    """another split's array, and one that does not ascend: statuses 0 or corruption_detected, every canary intact (call() checks them)"""
    text, sk = three_frames
    other = S.Split(text.data, 10, 64, 4096).first_record
    n, records = text.split.n, text.split.records
    assert len(other) > n + 1
    idx = list(range(records)) + [records - 1, 0]
    room = sum(text.split.sizes) * len(idx)
    for what, first in (("another split", other[:n] + [records]), ("another split's tail", other[-(n + 1):]), ("descending", [records, 7, 3, records])):
        g = call(L, H, codec, sk, first, n, 10, idx, n * len(idx), 1, L.zsmi_seekableRecordsWorkBound(sk, n * len(idx)), room)
        assert g.rc == 0 and set(g.status) <= {0, E_CORRUPT}, (what, sorted(set(g.status)))
        assert g.result[0] == g.status.count(0) and g.result[3] == int(g.offsets[-1])


# ------------------------------------------------------------------ 7. the pipeline, the host call, the host checks
def test_text_to_archive_to_lines_by_number(L, H, codec):
    from zstandard_amd import BatchCodec
    text = S.text_lines(256 << 10)
    T, M = 4096, 65536
    want = S.Split(text, 10, T, M)
    lines = text.splitlines(True)
    src, cnt, res = Dev(H, len(text), text), Dev(H, 8), Dev(H, 24)
    held = [src, cnt, res]
    try:
        codec.count_records_device(src.p, len(text), cnt.p)
        codec.sync()
        records = int(down(cnt, np.uint64)[0][0])
        assert records == want.records == len(lines)
        mp = BatchCodec.split_pieces_bound(records, len(text), M)
        fs, fr = Dev(H, 4 * mp), Dev(H, 8 * (mp + 1))
        held += [fs, fr]
        codec.split_records_device(src.p, len(text), mp, fs.p, fr.p, res.p, target_size=T, max_frame_size=M)
        codec.sync()                                                               # dResult: n is the next calls' host argument
        n = int(down(res, np.uint64)[0][0])
        assert n == want.n
        bound = codec.seekable_frames_resident_bound(len(text), n, True)
        arc, size = Dev(H, bound), Dev(H, 8)
        held += [arc, size]
        codec.compress_seekable_frames_resident(src.p, len(text), fs.p, n, M, arc.p, bound, size.p, level=3, checksum=True)
        codec.sync()
        m = int(down(size, np.uint64)[0][0])
        assert 0 < m <= bound
        sk = codec.open_seekable_device(arc.p, m)
        try:
            rng = np.random.default_rng(8)
            picks = [int(v) for v in rng.integers(0, records, 4096)]
            d_idx = up(H, np.asarray(picks, dtype=np.uint64))                      # uploaded once
            k = len(picks)
            work_cap = sk.records_work_bound(k)
            room = sum(len(lines[r]) for r in picks)
            work, dst, off, wr, st, out = Dev(H, work_cap), Dev(H, room), Dev(H, 8 * (k + 1)), Dev(H, 8 * k), Dev(H, 4 * k), Dev(H, 32)
            held += [d_idx, work, dst, off, wr, st, out]
            sk.read_records_resident(fr.p, n, d_idx.p, k, k, work.p, work_cap, dst.p, room, off.p, wr.p, st.p, out.p)      # fr: as the splitter left it
            codec.sync()
            offsets, status, written = down(off, np.uint64)[0], down(st, np.uint32)[0], down(wr, np.uint64)[0]
            buf, ok = down(dst)
            assert ok and not status.any()
            assert written.tolist() == [len(lines[r]) for r in picks] and int(offsets[k]) == room
            for q, r in enumerate(picks):
                assert buf[int(offsets[q]):int(offsets[q]) + len(lines[r])].tobytes() == lines[r], (q, r)
            assert int(down(out, np.uint64)[0][0]) == k
        finally:
            codec.sync(); sk.close()
    finally:
        for d in held:
            d.free()


@pytest.mark.parametrize("name", LISTED[:3])
def test_host_call_and_python_surface(L, H, codec, name):
    from zstandard_amd import SeekableArchive
    data, delim, T, M = CASES[name]
    text = Text(data, delim, T, M)
    records = text.split.records
    arc = archive_of(codec, text)
    idx = list(range(records)) + [records - 1, 0, 0, records]
    sk = open_host(L, codec, arc)
    try:
        g, w = roomy(L, H, codec, sk, text, idx, what=name)
        first = np.asarray(text.split.first_record, dtype=np.uint64); ix = np.asarray(idx, dtype=np.uint64)
        room = int(w.offsets[-1])
        out = np.full(room + 8, CANARY, dtype=np.uint8); off = np.zeros(len(idx) + 1, dtype=np.uint64); st = np.zeros(len(idx), dtype=np.uint32)
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        assert L.zsmi_seekableReadRecordsHost(codec.ctx, sk, p(first), text.split.n, delim, p(ix), len(idx), p(out), room, p(off), p(st)) == 0
        assert (off == g.offsets).all() and st.tolist() == g.status
        assert out[:room].tobytes() == g.buf.tobytes() and (out[room:] == CANARY).all()
    finally:
        codec.sync(); L.zsmi_closeSeekable(sk)
    sa = SeekableArchive(arc)
    try:
        got, codes = sa.read_records(text.split.first_record, idx, bytes([delim]), return_codes=True)
        assert codes == w.status and got[:-1] == [text.record(r) for r in idx[:-1]] and got[-1] == b""
        assert sa.read_records(text.split.first_record, idx[:-1], bytes([delim])) == got[:-1]
        with pytest.raises(RuntimeError):
            sa.read_records(text.split.first_record, idx, bytes([delim]))
        with pytest.raises(RuntimeError):
            sa.read_records(text.split.first_record[:-1], idx, bytes([delim]))     # not the archive's frame count
    finally:
        sa.close()


def test_host_checks_in_order(L, H, codec, three_frames):
    """each refusal with every later one present too, so that the order shows; nothing is queued or written by a refused call"""
    text, sk = three_frames
    p = ctypes.c_void_p
    one = p(8)                                                                    # a non-NULL pointer no refused call looks behind
    read = L.zsmi_seekableReadRecordsResident
    n = text.split.n
    assert read(None, None, None, n + 1, 256, None, 5, 0xFFFFFFFF, 3, None, 10, None, 10, None, None, None, None) == E_INIT
    assert read(codec.ctx, None, one, n + 1, 256, one, 5, 0xFFFFFFFF, 3, None, 10, None, 10, one, one, one, one) == E_GENERIC          # sk
    assert read(codec.ctx, sk, one, n + 1, 256, one, 5, 0xFFFFFFFF, 3, None, 10, None, 10, None, one, one, one) == E_GENERIC           # dDstOffsets
    assert read(codec.ctx, sk, one, n + 1, 256, one, 5, 0xFFFFFFFF, 3, None, 10, None, 10, one, one, one, None) == E_GENERIC           # dResult
    for hole in range(4):                                                          # dFirstRecord, dRecordIndex, dWritten, dStatus with requests
        a = [one] * 4
        a[hole] = None
        assert read(codec.ctx, sk, a[0], n + 1, 256, a[1], 5, 0xFFFFFFFF, 3, None, 10, None, 10, one, a[2], a[3], one) == E_GENERIC
    assert read(codec.ctx, sk, one, n + 1, 256, one, 5, 0xFFFFFFFF, 3, None, 10, None, 10, one, one, one, one) == E_PARAM              # delim
    assert read(codec.ctx, sk, one, n + 1, -1, one, 5, 0xFFFFFFFF, 1, None, 10, None, 10, one, one, one, one) == E_PARAM
    for align in (0, 3, 8192):
        assert read(codec.ctx, sk, one, n + 1, 10, one, 5, 0xFFFFFFFF, align, None, 10, None, 10, one, one, one, one) == E_PARAM
    assert read(codec.ctx, sk, one, n + 1, 10, one, 5, 0xFFFFFFFF, 1, None, 10, None, 10, one, one, one, one) == E_PARAM               # nFrames
    assert read(codec.ctx, sk, one, n, 10, one, 5, 0x8000001, 1, None, 10, None, 10, one, one, one, one) == E_FRAME_INDEX
    assert read(codec.ctx, sk, one, n, 10, one, 5, 0x8000000, 1, one, 10, None, 10, one, one, one, one) == E_GENERIC                   # dDst
    assert read(codec.ctx, sk, one, n, 10, one, 5, 0x8000000, 1, None, 10, one, 10, one, one, one, one) == E_GENERIC                   # dWork
    host = L.zsmi_seekableReadRecordsHost
    assert host(codec.ctx, None, one, n, 10, one, 5, None, 10, one, one) == E_GENERIC
    assert host(codec.ctx, sk, one, n, 300, one, 5, None, 10, one, one) == E_PARAM
    assert host(codec.ctx, sk, one, n + 1, 10, one, 5, None, 10, one, one) == E_PARAM
    assert host(codec.ctx, sk, one, n, 10, one, 5, None, 10, one, one) == E_GENERIC                                                     # dst
    codec.sync()
