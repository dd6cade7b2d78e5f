"""Words wider than 32 bits on the GPU: every 64-bit offset, size, record number and total of include/zsmi.h driven across 2^31 and 2^32.

Part A - virtual bigness, no large allocation.  The stream of tests/_wide.py (4400 frames, content past 4 GiB, a few hundred KB of
stream) is opened by every open call; the index, range reads, frames by number and the one-range read are held against its closed form
(content_at), which tests/test_wide_words_host.py holds against oracle D.  Record numbers above 2^31, 2^32 and at 2^63 come from shifting
a small record archive's firstRecord[] and the requests by K: the header defines the lookup over whatever non-decreasing array the caller
hands in, so the shifted call must leave exactly what the K = 0 call leaves, and that one is held against the Python rules of
tests/_split.py and tests/_find.py.  Sizes and layout: header-only frames that state 2^30 bytes each, summed past 2^32 on the device.

Part B - real places: one device buffer of 2^32 + 64 MiB (tests/_hip.py BigDev) and the places of tests/_places.py, for the offset
arrays of the batch, pack and range calls, once with the sources and once with the destinations there; the host forms on lazily mapped
host buffers.  Its own comment, further down, says what is held against what.

Every device call writes into canary-guarded buffers; no call decodes, compresses or copies more than 64 MiB."""
import ctypes, mmap
import numpy as np
import pytest
import _batch as B
import _data as D
import _dicts as X
import _edge_catalogue as C
import _find as FD
import _framewriter as W
import _oracle as O
import _places as PL
import _resident as RD
import _seekable_ranges as R
import _seekable_resident as RR
import _sizes as SZ
import _split as SP
import _wide as WD
import test_gpu_find_archive as GA
import test_gpu_read_records as GR
import test_gpu_seekable_frames as GF
from _hip import hip_of, Dev, BigDev, OutOfDeviceMemory, BIG_BYTES, CANARY, PAD

pytestmark = pytest.mark.gpu
E_CORRUPT, E_OUT_OF_BOUND, E_FRAME_INDEX = 20, 42, 100
T31, T32, T63 = 1 << 31, 1 << 32, 1 << 63
p = ctypes.c_void_p


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


# ================================================================== part A
class Wide:
    """the stream in device memory and its handles: host = zsmi_openFrames, device = zsmi_openFramesDevice, table = zsmi_openSeekableDevice
    on stream + zsmi_buildSeekTable's table"""


@pytest.fixture(scope="module")
def wide(L, H, codec):
    w = Wide()
    s = WD.stream()
    cap = 17 + 8 * WD.N
    t = ctypes.create_string_buffer(cap)
    assert L.zsmi_buildSeekTable(t, cap, s, len(s)) == cap
    w.archive = s + t.raw
    w.dev = Dev(H, len(w.archive), w.archive)
    w.handles = {}
    err = ctypes.c_int(-1)
    w.handles["host"] = L.zsmi_openFrames(codec.ctx, s, len(s), ctypes.byref(err)); assert err.value == 0
    w.handles["device"] = L.zsmi_openFramesDevice(codec.ctx, p(w.dev.p), len(s), ctypes.byref(err)); assert err.value == 0
    w.handles["table"] = L.zsmi_openSeekableDevice(codec.ctx, p(w.dev.p), len(w.archive), ctypes.byref(err)); assert err.value == 0
    assert all(w.handles.values())
    w.rows = [(c, d, None) for _, c, d in WD.entries()]
    yield w
    codec.sync()
    for h in w.handles.values():
        L.zsmi_closeSeekable(h)
    raw = np.frombuffer(w.dev.all(), dtype=np.uint8)
    assert (raw[:PAD] == CANARY).all() and (raw[PAD + len(w.archive):] == CANARY).all() and raw[PAD:PAD + len(w.archive)].tobytes() == w.archive
    w.dev.free()


FORMS = ("host", "device", "table")


def info(L, sk, i):
    v = (ctypes.c_uint64(7), ctypes.c_uint64(7), ctypes.c_uint32(7), ctypes.c_uint32(7))
    rc = L.zsmi_getFrameInfo_fromSeekable(sk, i, *[ctypes.byref(x) for x in v])
    return rc, tuple(x.value for x in v)


# ------------------------------------------------------------------ A1. the index
@pytest.mark.parametrize("form", FORMS)
def test_index_across_both_crossings(L, wide, form):
    sk = wide.handles[form]
    assert L.zsmi_getNumFrames_fromSeekable(sk) == WD.N
    assert L.zsmi_getContentSize_fromSeekable(sk) == WD.CONTENT > T32
    e = WD.entries()
    for f in WD.CROSSING_FRAMES + [0, WD.N - 1]:
        assert info(L, sk, f) == (0, (e[f][0], f * WD.S, e[f][1], e[f][2])), (form, f)
    assert info(L, sk, WD.frame_of(T31))[1][1] < T31 < info(L, sk, WD.frame_of(T31) + 1)[1][1]
    assert info(L, sk, WD.frame_of(T32))[1][1] < T32 < info(L, sk, WD.frame_of(T32) + 1)[1][1]
    assert info(L, sk, WD.N)[0] == E_FRAME_INDEX


# ------------------------------------------------------------------ A2. ranges
def check_places(b, ranges, what):
    assert b.rc == 0 and b.status == [0] * len(ranges), (what, b.rc, b.status)
    assert b.written == [n for _, n in ranges], what
    for r, (o, n) in enumerate(ranges):
        want = WD.content_at(o, n)
        assert b.out[r] == want, (what, r, hex(o), n, next(i for i in range(n) if b.out[r][i] != want[i]))


@pytest.mark.parametrize("form", FORMS)
def test_ranges_at_the_places_device(L, H, codec, wide, form):
    sk = wide.handles[form]
    for what, ranges in (("in order", WD.PLACES), ("reversed", WD.PLACES[::-1])):
        b = R.read_ranges(L, H, codec, sk, ranges, WD.CONTENT, seed=3)
        check_places(b, ranges, (form, what))
        assert b.frames_decoded == len(R.frames_touched([(WD.FRAME_BYTES, WD.S)] * WD.N, ranges)[1])


@pytest.mark.parametrize("form", FORMS)
def test_ranges_at_the_places_host(L, codec, wide, form):
    sk = wide.handles[form]
    for what, ranges in (("in order", WD.PLACES), ("reversed", WD.PLACES[::-1])):
        n = len(ranges)
        total = sum(ln for _, ln in ranges)
        off, ln = R.u64([r[0] for r in ranges]), R.u64([r[1] for r in ranges])
        written, codes = np.full(n, 0xDEAD, dtype=np.uint64), np.full(n, 9, dtype=np.uint32)
        out = np.full(total + 64, CANARY, dtype=np.uint8)
        assert L.zsmi_seekableReadRangesHost(codec.ctx, sk, R.ptr(off), R.ptr(ln), n, R.ptr(out), total, R.ptr(written), R.ptr(codes)) == 0, (form, what)
        assert written.tolist() == [r[1] for r in ranges] and not codes.any(), (form, what)
        assert (out[total:] == CANARY).all()
        at = 0
        for o, m in ranges:
            assert out[at:at + m].tobytes() == WD.content_at(o, m), (form, what, hex(o), m)
            at += m


def test_ranges_at_the_contents_end(L, H, codec, wide):
    """a range that ends one byte behind the content is clipped, one that begins at the content size reads nothing, one that begins behind
    it refuses the call with parameter_outOfBound and writes nothing: what the same shapes give on a small archive
    (tests/test_gpu_seekable_ranges.py test_call_edges, test_per_range_status)"""
    sk, C = wide.handles["device"], WD.CONTENT
    ranges = [(C - 10, 11), (C, 10), (C, 0), (T32 - 3, 6)]
    b = R.read_ranges(L, H, codec, sk, ranges, C)                              # (written == the clipped lengths: asserted there)
    assert b.rc == 0 and b.status == [0] * 4 and b.written == [10, 0, 0, 6]
    assert b.out[0] == WD.content_at(C - 10, 10) and b.out[3] == WD.content_at(T32 - 3, 6)
    b = R.read_ranges(L, H, codec, sk, [(0, 10), (C + 1, 1), (T32, 100)], C)
    assert b.rc == E_OUT_OF_BOUND and b.written == [0xDEAD] * 3 and b.status_raw == bytes([CANARY]) * 12 and b.frames_decoded == 0xDEAD


def test_one_range_read_across_4_gib(L, H, codec, wide):
    """zsmi_decompressSeekableDevice on stream + table: offset and length as 64-bit arguments of the call that opens, reads and closes"""
    o, n = WD.PLACES[6]
    assert o < T32 < o + n
    for o, n in ((o, n), (T32 - 100, 200), (WD.CONTENT - 1000, 5000)):
        want = WD.content_at(o, min(n, WD.CONTENT - o))
        dst, st = Dev(H, n), Dev(H, 4)
        written = ctypes.c_uint64(0xDEAD)
        try:
            assert L.zsmi_decompressSeekableDevice(codec.ctx, p(wide.dev.p), len(wide.archive), o, n, p(dst.p), ctypes.byref(written), p(st.p)) == 0
            codec.sync()
            assert written.value == len(want)
            buf, ok = RD.down(dst)
            assert ok and buf[:len(want)].tobytes() == want and (buf[len(want):] == CANARY).all(), hex(o)
            status, ok = RD.down(st, np.uint32)
            assert ok and status.tolist() == [0]
        finally:
            dst.free(); st.free()


# ------------------------------------------------------------------ A3. frames by number
def frame_numbers():
    return WD.CROSSING_FRAMES + [WD.N - 1]


def check_frame(f, got, what):
    assert len(got) == WD.S and got[:16] == WD.head(f), (what, f, "the head does not name the frame", got[:16].hex())
    assert got == WD.content_at(f * WD.S, WD.S), (what, f)


@pytest.mark.parametrize("form", FORMS)
def test_frames_by_number(L, H, codec, wide, form):
    sk, idx = wide.handles[form], frame_numbers()
    b = GF.read_frames(L, H, codec, sk, idx, wide.rows, seed=4)
    assert b.rc == 0 and b.status == [0] * len(idx) and b.written == [WD.S] * len(idx) and b.frames_decoded == len(idx)
    for f, got in zip(idx, b.out):
        check_frame(f, got, form)


@pytest.mark.parametrize("align", [1, 4096])
@pytest.mark.parametrize("form", FORMS)
def test_frames_by_number_resident(L, H, codec, wide, form, align):
    sk, idx = wide.handles[form], frame_numbers()[::-1]
    want_off = RR.rounded_offsets([WD.S] * len(idx), align)
    r = RR.read(L, H, codec, sk, idx, align, int(want_off[-1]))
    assert r.rc == 0 and r.status.tolist() == [0] * len(idx) and r.written.tolist() == [WD.S] * len(idx)
    assert (r.offsets == want_off).all()
    inside = np.zeros(len(r.buf), dtype=bool)
    for k, f in enumerate(idx):
        check_frame(f, r.out(k, WD.S), (form, align))
        inside[int(want_off[k]):int(want_off[k]) + WD.S] = True
    assert (r.buf[~inside] == CANARY).all()


# ------------------------------------------------------------------ A4. record numbers above 2^31, 2^32 and at 2^63
def record_text():
    """lines, one record of 9000 bytes that M = 4096 cuts into three pieces, lines"""
    return SP.lines(31, 60, 120) + b"y" * 9000 + b"\n" + SP.lines(32, 60, 120)


@pytest.fixture(scope="module")
def rec(L, codec):
    text = GR.Text(record_text(), 10, 2048, 4096)
    cut = 60
    assert text.split.n >= 5 and text.frames(cut)[0] < text.frames(cut)[1], "record 60 must be cut"
    sk = GR.open_host(L, codec, GR.archive_of(codec, text))
    yield text, sk
    codec.sync(); L.zsmi_closeSeekable(sk)


def shifts(first):
    mid = first[len(first) // 2]
    assert first[0] < mid < first[-1]
    return [T31 - mid, T32 - mid, T63]


def record_requests(text):
    records, cut = text.split.records, 60
    # an ascending run (followers), the cut record and its neighbours, repeats, the last record, one request at firstRecord[nFrames]
    return list(range(0, 12)) + [cut - 1, cut, cut + 1, cut, 5, 5, records - 1, records, 3]


def test_read_records_with_wide_numbers(L, H, codec, rec):
    text, sk = rec
    idx = record_requests(text)
    first, n = text.split.first_record, text.split.n
    g0, w0 = GR.roomy(L, H, codec, sk, text, idx, what="K = 0")              # held against the Python rule there
    assert w0.status.count(E_FRAME_INDEX) == 1 and len(w0.leaders) < len(idx) - 1
    work = L.zsmi_seekableRecordsWorkBound(sk, w0.result[1])
    for K in shifts(first):
        fk, ik = [v + K for v in first], [r + K for r in idx]
        cross = T31 if K < T31 else T32 if K < T32 else None
        assert cross is None or fk[0] < cross <= fk[-1], "the shifted array must cross"
        g = GR.call(L, H, codec, sk, fk, n, 10, ik, w0.result[1], 1, work, w0.result[3])
        assert g.rc == 0 and g.status == g0.status and g.written == g0.written and g.result == g0.result, (hex(K), g.status, g.result)
        assert (g.offsets == g0.offsets).all() and g.buf.tobytes() == g0.buf.tobytes(), hex(K)
        # the host form
        fa, ia = np.asarray(fk, dtype=np.uint64), np.asarray(ik, dtype=np.uint64)
        room = int(w0.offsets[-1])
        out = np.full(room + 8, CANARY, dtype=np.uint8); off = np.zeros(len(idx) + 1, dtype=np.uint64); st = np.full(len(idx), 9, dtype=np.uint32)
        assert L.zsmi_seekableReadRecordsHost(codec.ctx, sk, R.ptr(fa), n, 10, R.ptr(ia), len(idx), R.ptr(out), room, R.ptr(off), R.ptr(st)) == 0
        assert (off == g0.offsets).all() and st.tolist() == g0.status, hex(K)
        assert out[:room].tobytes() == g0.buf.tobytes() and (out[room:] == CANARY).all(), hex(K)


def find_patterns(data):
    first = bytes([next(b for b in data if b != 10)])
    return [first, b"yy", b"y" * 256]


def test_find_records_with_wide_numbers(L, H, codec):
    data = record_text()
    o = GA.Opened(L, H, codec, data, 10, 2048, 4096)
    try:
        first0 = list(o.split.first_record)
        mid = o.n // 2
        windows = [(0, o.n), (mid, o.n), (mid - 1, mid + 1), (0, mid)]
        base = {}
        for pat in find_patterns(data):
            for a, b in windows:
                base[pat, a, b] = o.check(pat, a, b, what="K = 0")               # held against tests/_find.py there
        assert len(base[find_patterns(data)[0], 0, o.n][0]) >= 3
        for K in shifts(first0):
            fk = [v + K for v in first0]
            o.first.free()
            o.first = RD.up(H, np.asarray(fk, dtype=np.uint64))
            o.split.first_record = fk                                            # (find() checks that the call left dFirstRecord alone)
            fa = np.asarray(fk, dtype=np.uint64)
            for (pat, a, b), (records, matches) in base.items():
                rc, result, got, _ = o.find(pat, a, b)
                want = [r + K for r in records]
                assert rc == 0 and result == [len(records), len(records), matches, o.at[b] - o.at[a]], (hex(K), pat[:4], a, b, rc, result)
                assert got == want and all(x < y for x, y in zip(got, got[1:])), (hex(K), pat[:4], a, b, got[:6], want[:6])
                cap = len(records)
                out = np.full(cap + 1, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64); res = np.zeros(4, dtype=np.uint64)
                rc = L.zsmi_seekableFindRecordsHost(codec.ctx, o.sk, R.ptr(fa), o.n, 10, pat, len(pat), a, b - a, R.ptr(out) if cap else None, cap, R.ptr(res))
                assert rc == 0 and res.tolist() == result and out[:cap].tolist() == want and int(out[cap]) == 0xA5A5A5A5A5A5A5A5, (hex(K), pat[:4], a, b)
            got_all = [r + K for r in base[find_patterns(data)[0], 0, o.n][0]]
            if K < T32:
                t = T31 if K < T31 else T32
                assert got_all[0] < t <= got_all[-1], "the numbers must cross"
    finally:
        o.split.first_record = first0
        o.close()


@pytest.mark.parametrize("base", [T32 - 2, T31 - 2, T63])
def test_find_records_device_with_a_wide_base(L, H, codec, base):
    text = SP.text_lines(6000, seed=9)
    for pat in (b"e", b"th"):
        records, matches = FD.find(text, pat, 10, 0)
        assert records[0] < 2 <= records[-1] or pat != b"e"
        d = FD.device(L, H, codec, text, pat, 10, base=base)
        FD.same_as_rule(d, text, pat, 10, base)
        total, got, m, intact = FD.host(L, text, pat, 10, base)
        assert intact and (total, m) == (d.result[0], d.result[2]) and got == d.records[:total] == [r + base for r in records]


# ------------------------------------------------------------------ A5. sizes and layout past 2^32
STATED = [1 << 30, (1 << 30) - 1, 1, 1 << 30, 1 << 30]


def header_only_frames():
    """single-segment frames of one short raw block whose Frame_Content_Size field states STATED[i] (4-byte fields, the last one 8, the
    third 1): the shape of tests/_sizes.py's sized_frame; the size calls walk headers only"""
    widths = [4, 4, 1, 4, 8]
    return [W.frame([W.raw(b"body %d" % i)], fcs=s, fcs_bytes=w)[0] for i, (s, w) in enumerate(zip(STATED, widths))]


def test_frame_sizes_of_a_gibibyte_each(L, H, codec):
    items = header_only_frames()
    want = np.array([SZ.host_answers(L, it) for it in items], dtype=np.uint64)
    assert want[:, 0].tolist() == STATED and want[:, 1].tolist() == STATED and not want[:, 2].any()
    n = len(items)
    gap = 13
    offs = np.cumsum([5] + [len(it) + gap for it in items])[:n].astype(np.uint64)
    src_np = np.full(int(offs[-1]) + len(items[-1]) + gap, CANARY, dtype=np.uint8)
    for o_, it in zip(offs, items):
        src_np[int(o_):int(o_) + len(it)] = np.frombuffer(it, dtype=np.uint8)
    sizes = np.array([len(it) for it in items], dtype=np.uint32)
    src, d_off, d_sz = RD.up(H, src_np), RD.up(H, offs), RD.up(H, sizes)
    content, bounds, status = Dev(H, 8 * n), Dev(H, 8 * n), Dev(H, 4 * n)
    try:
        codec.frame_sizes_device(src.p, d_off.p, d_sz.p, n, content.p, bounds.p, status.p)
        codec.sync()
        for dev, t, k in ((content, np.uint64, 0), (bounds, np.uint64, 1), (status, np.uint32, 2)):
            got, ok = RD.down(dev, t)
            assert ok and got.tolist() == want[:, k].tolist(), (k, got.tolist())
        # the layout over what the sizes call left, in device memory
        for align in (1, 4096):
            for failed in (None, 1):
                st = np.zeros(n, dtype=np.uint32)
                if failed is not None:
                    st[failed] = E_CORRUPT
                caps_w = np.where(st == 0, np.array(STATED, dtype=np.uint64), 0).astype(np.uint64)
                step = (caps_w + np.uint64(align - 1)) // np.uint64(align) * np.uint64(align)
                off_w = np.concatenate([[0], np.cumsum(step, dtype=np.uint64)]).astype(np.uint64)
                assert int(off_w[-1]) == sum(-(-int(c) // align) * align for c in caps_w)       # Python ints
                assert failed is not None or int(off_w[-1]) >= T32
                d_st = RD.up(H, st)
                caps, offsets = Dev(H, 4 * n), Dev(H, 8 * (n + 1))
                try:
                    codec.layout_outputs_device(content.p, d_st.p if failed is not None else 0, n, caps.p, offsets.p, align=align)
                    codec.sync()
                    gc, ok1 = RD.down(caps, np.uint32)
                    go, ok2 = RD.down(offsets, np.uint64)
                    assert ok1 and ok2 and gc.tolist() == caps_w.tolist() and go.tolist() == off_w.tolist(), (align, failed, gc.tolist(), [hex(int(v)) for v in go])
                finally:
                    for d in (d_st, caps, offsets):
                        d.free()
        # align 2^31: include/zsmi.h admits a power of two in 1 .. 4096, and tests/test_gpu_resident.py pins the refusal of 1 << 31
        # (parameter_outOfBound); nothing is written by the refused call
        caps, offsets = Dev(H, 4 * n), Dev(H, 8 * (n + 1))
        try:
            assert L.zsmi_layoutOutputsDevice(codec.ctx, p(content.p), None, n, 1 << 31, p(caps.p), p(offsets.p)) == E_OUT_OF_BOUND
            codec.sync()
            assert (RD.down(caps)[0] == CANARY).all() and (RD.down(offsets)[0] == CANARY).all()
        finally:
            caps.free(); offsets.free()
    finally:
        for d in (src, d_off, d_sz, content, bounds, status):
            d.free()


def test_compress_bounds_of_the_largest_sizes(L, H, codec):
    sizes = np.array([0xFFFFFF00, 0xFFFFFFFF, 0, 65536, 0x80000000, 0x7FFFFFFF], dtype=np.uint32)
    want = [int(L.zsmi_compressBound(int(s))) for s in sizes]
    assert want[0] > T32 and want[1] > T32 and want[1] > want[0]
    d_sz, out = RD.up(H, sizes), Dev(H, 8 * len(sizes))
    try:
        codec.compress_bounds_device(d_sz.p, len(sizes), out.p)
        codec.sync()
        got, ok = RD.down(out, np.uint64)
        assert ok and got.tolist() == want, [hex(int(v)) for v in got]
    finally:
        d_sz.free(); out.free()


# ================================================================== part B: real places above 2 GiB and 4 GiB
# One allocation of 2^32 + 64 MiB (tests/_hip.py BigDev), never filled from the host, never copied whole.  One side of a call is big at a
# time.  Every call runs with all offsets low first - held against oracle D's bytes or code, oracle E's frames - and then with its
# sources, and with its destinations, at the places of tests/_places.py: placement must not change an output byte or a size word, the 4 KiB
# in front of and behind every item keep the canary, and so do the windows at off mod 2^32 and off mod 2^31, where a truncated store lands.
class Small:
    """a Dev of n bytes seen through BigDev's window calls"""

    def __init__(self, H, n):
        self.H, self.dev = H, Dev(H, max(n, 1))
        self.p = self.dev.p

    def write(self, off, data):
        if data:
            assert self.H.hipMemcpy(p(self.p + off), bytes(data), len(data), 1) == 0

    def read(self, off, n):
        out = ctypes.create_string_buffer(max(n, 1))
        if n:
            assert self.H.hipMemcpy(out, p(self.p + off), n, 2) == 0
        return out.raw[:n]

    def free(self):
        self.dev.free()


@pytest.fixture(scope="module")
def big(H):
    try:
        b = BigDev(H)
    except OutOfDeviceMemory as e:
        pytest.skip(str(e))
    yield b
    b.free()


def small_offsets(lens):
    out, pos = [], PAD
    for ln in lens:
        out.append(pos)
        pos += ln + PAD + 3
    return out


def u64(a):
    return np.ascontiguousarray(a, dtype=np.uint64)


def u32(a):
    return np.ascontiguousarray(a, dtype=np.uint32)


def run_placed(H, codec, big, side, layout, src_items, dst_lens, call, what=""):
    """one call with its sources (side "src") or its destinations (side "dst") at the places in the big buffer, or everything low
    (side "low") -> (size words, the bytes each item produced).  call(src pointer, srcOffsets, srcSizes, dst pointer, dstOffsets, dDstSizes)
    queues the work and returns the device buffers it wants freed behind the wait"""
    n = len(src_items)
    src_lens = [len(s) for s in src_items]
    so = PL.geometry(src_lens, layout) if side == "src" else small_offsets(src_lens)
    do = PL.geometry(dst_lens, layout) if side == "dst" else small_offsets(dst_lens)
    if side != "low":
        PL.holds_what_it_is_for(so if side == "src" else do, src_lens if side == "src" else dst_lens, layout)
    src = big if side == "src" else Small(H, so[-1] + src_lens[-1] + PAD)
    dst = big if side == "dst" else Small(H, do[-1] + dst_lens[-1] + PAD)
    dsz = Dev(H, 4 * n)
    held = []
    try:
        for o, s in zip(so, src_items):
            src.write(o, s)
        held = call(src.p, u64(so), u32(src_lens), dst.p, u64(do), dsz.p) or []
        codec.sync()
        words, ok = RD.down(dsz, np.uint32)
        assert ok, (what, "wrote outside dDstSizes")
        words = [int(w) for w in words]
        for i, (w, ln) in enumerate(zip(words, dst_lens)):
            assert w >= B.ERR or w <= ln, (what, i, "a size above the item's room", w, ln)
        out = [dst.read(o, w if w < B.ERR else 0) for o, w in zip(do, words)]
        PL.assert_guards(dst.read, do, dst_lens, what=(what, side, layout, "destination"))
        for i, (o, s) in enumerate(zip(so, src_items)):
            assert src.read(o, len(s)) == s, (what, side, layout, "source item changed", i)
        PL.assert_guards(src.read, so, src_lens, what=(what, side, layout, "source"))
        return words, out
    finally:
        codec.sync()
        if side != "low":
            offs, lens = (so, src_lens) if side == "src" else (do, dst_lens)
            for o, ln in list(zip(offs, lens)) + [(o, ln) for o, ln, _ in PL.guard_windows(offs, lens)]:
                big.refill(o, ln)
        for d in [dsz] + list(held) + [b for b in (src, dst) if b is not big]:
            d.free()


# ------------------------------------------------------------------ the items
def texts():
    z = D.zipf_log(1 << 20, seed_lo=0x61, single=True).tobytes()
    sizes = [131072, 100000, 65536, 5000, 70000, 33333, 200, 1000, 4097, 65537, 300, 2048, 12345, 257, 20000, 777, 9000]
    return [z[7919 * i:7919 * i + s] for i, s in enumerate(sizes)]


EDGE_IDS = ("literals/huf4s_6", "sequences/all_rep_second", "header/fcs4_65792_single",          # the fast path's, at exact capacities
            "frames/two_frames", "sequences/nbseq0x7f00",                                        # the general kernel's
            "offsets/match_before_frame_start")                                                  # fails: corruption_detected, pinned


def oracle_d(frame, cap, dic=None):
    """oracle D at this capacity: the bytes, or the word the batch calls write for its code"""
    try:
        return O.decompress_using_dict(frame, cap, dic) if dic else O.decompress(frame, cap)
    except O.OracleError as e:
        return (1 << 32) - e.code


class Case:
    """src: the items of the call; room: the bytes each destination may take; want: oracle's answer an item (bytes, or an error word);
    call(codec) -> the closure run_placed takes"""


def decode_items():
    cat = {e.id: e for e in C.catalogue()}
    chunks = texts()
    frames = [O.compress(c, 3) for c in chunks]
    assert len(list(W.blocks(frames[1]))) == 2
    items = [(f, len(c)) for f, c in zip(frames, chunks)] + [(cat[k].frame, cat[k].cap) for k in EDGE_IDS] + [(O.compress(b"", 3), 0)]
    assert cat[EDGE_IDS[-1]].expect == 20 and len(items) == 24 and all(max(len(f), cap) <= 128 << 10 for f, cap in items)
    return items


def dict_chunks():
    data = X.class_data("json_records")
    sizes = [65536, 40000, 5000, 30000, 1000, 20000, 300, 2500, 64, 8000, 0]
    return [data[9973 * i:9973 * i + s] for i, s in enumerate(sizes)]


@pytest.fixture(scope="module")
def cases(L, H, codec):
    from zstandard_amd import CompressionDict, DecompressionDict
    dic = X.trained("json_records")
    dd, cd = DecompressionDict(codec, dic), CompressionDict(codec, dic, 3)
    out = {}

    def add(name, src, room, want, make):
        c = Case()
        c.name, c.src, c.room, c.want, c.call = name, src, room, want, make
        out[name] = c

    # ---- decode
    items = decode_items()
    frames, caps = [f for f, _ in items], [c for _, c in items]
    want = [oracle_d(f, c) for f, c in items]
    assert want[-2] == (1 << 32) - 20 and sum(isinstance(w, int) for w in want) == 1
    add("decompressBatchDevice", frames, caps, want,
        lambda sp, so, ss, dp, do, zp: codec.decompress_device(sp, so, ss, dp, do, u32(caps), zp))

    def dec_resident(sp, so, ss, dp, do, zp):
        held = [RD.up(H, a) for a in (so, ss, do, u32(caps))]
        codec.decompress_resident(sp, held[0].p, held[1].p, len(caps), dp, held[2].p, held[3].p, max(caps), zp)
        return held
    add("decompressBatchResident", frames, caps, want, dec_resident)
    dchunks = dict_chunks()
    ditems = [(O.compress_using_dict(c, dic, 3), len(c)) for c in dchunks] + items[17:23]
    dframes, dcaps = [f for f, _ in ditems], [c for _, c in ditems]
    add("decompressBatchDevice_usingDDict", dframes, dcaps, [oracle_d(f, c, dic) for f, c in ditems],
        lambda sp, so, ss, dp, do, zp: codec.decompress_device(sp, so, ss, dp, do, u32(dcaps), zp, ddict=dd))
    # ---- compress
    chunks = texts() + [b""]
    bounds = [int(L.zsmi_compressBound(len(c))) for c in chunks]
    for level in (1, 3):
        add(f"compressBatchDevice_l{level}", chunks, bounds, [O.compress(c, level) for c in chunks],
            lambda sp, so, ss, dp, do, zp, level=level: codec.compress_device(sp, so, ss, dp, do, zp, level))

    def comp_resident(sp, so, ss, dp, do, zp):
        held = [RD.up(H, a) for a in (so, ss, do)]
        codec.compress_resident(sp, held[0].p, held[1].p, len(chunks), max(len(c) for c in chunks), dp, held[2].p, zp, 3)
        return held
    add("compressBatchResident", chunks, bounds, [O.compress(c, 3) for c in chunks], comp_resident)
    # a formatted CDict's frames use the dictionary's entropy tables: no oracle states them byte for byte (include/zsmi.h).  They are held
    # to oracle D - each decodes to its chunk with the dictionary - and to the call with all offsets low
    add("compressBatchDevice_usingCDict", dchunks, [int(L.zsmi_compressBound(len(c))) for c in dchunks], None,
        lambda sp, so, ss, dp, do, zp: codec.compress_device(sp, so, ss, dp, do, zp, cdict=cd))
    out["compressBatchDevice_usingCDict"].decodes_to = (dchunks, dic)
    yield out
    codec.sync()
    dd.close(); cd.close()


CASES = ("decompressBatchDevice", "decompressBatchResident", "decompressBatchDevice_usingDDict", "compressBatchDevice_l1", "compressBatchDevice_l3",
         "compressBatchResident", "compressBatchDevice_usingCDict")
_low = {}


def result_of(words, out):
    return [w if w >= B.ERR else o for w, o in zip(words, out)]


def low_result(H, codec, case):
    """the call with all offsets low, held against the oracle (once a case)"""
    if case.name not in _low:
        words, out = run_placed(H, codec, None, "low", "edges", case.src, case.room, case.call, what=case.name)
        got = result_of(words, out)
        if case.want is not None:
            bad = [i for i, (g, w) in enumerate(zip(got, case.want)) if g != w]
            assert not bad, (case.name, "against the oracle", bad)
        else:
            chunks, dic = case.decodes_to
            for i, (f, c) in enumerate(zip(got, chunks)):
                assert not isinstance(f, int) and O.decompress_using_dict(f, len(c), dic) == c, (case.name, "oracle D", i)
        _low[case.name] = (words, out)
    return _low[case.name]


@pytest.mark.parametrize("layout", PL.LAYOUTS)
@pytest.mark.parametrize("side", ["src", "dst"])
@pytest.mark.parametrize("name", CASES)
def test_batch_call_at_the_places(H, codec, big, cases, name, side, layout):
    case = cases[name]
    low_words, low_out = low_result(H, codec, case)
    words, out = run_placed(H, codec, big, side, layout, case.src, case.room, case.call, what=name)
    assert words == low_words, (name, side, layout, [(i, hex(a), hex(b)) for i, (a, b) in enumerate(zip(words, low_words)) if a != b])
    for i, (a, b) in enumerate(zip(out, low_out)):                               # every placed item, none left out
        assert a == b, (name, side, layout, "bytes of item", i, B.first_difference(a, b))
    assert len(out) == len(case.src)


# ------------------------------------------------------------------ zsmi_packFramesDevice
@pytest.mark.parametrize("layout", PL.LAYOUTS)
def test_pack_frames_from_the_places(H, codec, big, layout):
    frames = [O.compress(c, 3) for c in texts() + [b""]]
    n, lens = len(frames), [len(f) for f in frames]
    offs = PL.geometry(lens, layout)
    PL.holds_what_it_is_for(offs, lens, layout)
    total = sum(lens)
    d_sz, packed, poff = RD.up(H, u32(lens)), Dev(H, total), Dev(H, 8 * (n + 1))
    try:
        for o, f in zip(offs, frames):
            big.write(o, f)
        codec.pack_device(big.p, u64(offs), d_sz.p, n, packed.p, poff.p)
        codec.sync()
        got, ok = RD.down(packed)
        assert ok and got.tobytes() == b"".join(frames)
        got, ok = RD.down(poff, np.uint64)
        assert ok and got.tolist() == [0] + np.cumsum(lens).tolist()
        for o, f in zip(offs, frames):
            assert big.read(o, len(f)) == f
        PL.assert_guards(big.read, offs, lens, what=("pack", layout))
    finally:
        codec.sync()
        for o, ln in zip(offs, lens):
            big.refill(o, ln)
        for d in (d_sz, packed, poff):
            d.free()


@pytest.mark.parametrize("crossing", [T31, T32])
def test_pack_frames_into_a_run_across_a_crossing(H, codec, big, crossing):
    frames = [O.compress(c, 3) for c in texts() + [b""]]
    n, lens = len(frames), [len(f) for f in frames]
    total = sum(lens)
    base = crossing - total // 2 - 1
    so = small_offsets(lens)
    src, d_sz, poff = Small(H, so[-1] + lens[-1] + PAD), RD.up(H, u32(lens)), Dev(H, 8 * (n + 1))
    try:
        for o, f in zip(so, frames):
            src.write(o, f)
        codec.pack_device(src.p, u64(so), d_sz.p, n, big.p + base, poff.p)
        codec.sync()
        assert big.read(base, total) == b"".join(frames)
        got, ok = RD.down(poff, np.uint64)
        assert ok and got.tolist() == [0] + np.cumsum(lens).tolist()
        PL.assert_guards(big.read, [base], [total], what=("pack into", hex(crossing)))
    finally:
        codec.sync()
        for o, ln in [(base, total)] + [(o, ln) for o, ln, _ in PL.guard_windows([base], [total])]:
            big.refill(o, ln)
        for d in (src, d_sz, poff):
            d.free()


# ------------------------------------------------------------------ zsmi_seekableReadRangesDevice with dstOffsets at the places
@pytest.mark.parametrize("layout", PL.LAYOUTS)
def test_ranges_to_the_places(L, H, codec, big, wide, layout):
    ranges = WD.PLACES
    n, lens = len(ranges), [ln for _, ln in ranges]
    offs = PL.geometry(lens, layout)
    PL.holds_what_it_is_for(offs, lens, layout)
    st = Dev(H, 4 * n)
    written, frames = np.full(n, 0xDEAD, dtype=np.uint64), ctypes.c_uint32(0xDEAD)
    off_a, len_a, dst_a = u64([o for o, _ in ranges]), u64(lens), u64(offs)
    try:
        rc = L.zsmi_seekableReadRangesDevice(codec.ctx, wide.handles["device"], R.ptr(off_a), R.ptr(len_a), n, p(big.p), R.ptr(dst_a), R.ptr(written), p(st.p),
                                             ctypes.byref(frames))
        codec.sync()
        assert rc == 0 and written.tolist() == lens
        status, ok = RD.down(st, np.uint32)
        assert ok and not status.any()
        for (o, ln), at in zip(ranges, offs):
            assert big.read(at, ln) == WD.content_at(o, ln), (layout, hex(o), hex(at))
        PL.assert_guards(big.read, offs, lens, what=("ranges", layout))
    finally:
        codec.sync()
        for o, ln in list(zip(offs, lens)) + [(o, ln) for o, ln, _ in PL.guard_windows(offs, lens)]:
            big.refill(o, ln)
        st.free()


# ------------------------------------------------------------------ the host forms: lazily mapped host buffers, touched in windows only
class HostBig:
    """an anonymous mapping of 2^32 + 64 MiB: pages exist only where a window was written or read"""

    def __init__(self):
        try:
            self.mm = mmap.mmap(-1, BIG_BYTES, flags=mmap.MAP_PRIVATE | mmap.MAP_ANONYMOUS | getattr(mmap, "MAP_NORESERVE", 0x4000))
        except (OSError, ValueError, OverflowError) as e:
            pytest.skip(f"the mapping of {BIG_BYTES} bytes was refused: {e}")
        self.anchor = ctypes.c_char.from_buffer(self.mm)
        self.p = ctypes.addressof(self.anchor)

    def write(self, off, data):
        self.mm[off:off + len(data)] = bytes(data)

    def read(self, off, n):
        return self.mm[off:off + n]

    def close(self):
        del self.anchor
        self.mm.close()


@pytest.mark.parametrize("layout", PL.LAYOUTS)
@pytest.mark.parametrize("name", ["decompressBatchDevice", "compressBatchDevice_l1", "compressBatchDevice_l3"])
def test_host_forms_around_4_gib(L, H, codec, cases, name, layout):
    """zsmi_decompressBatchHost / zsmi_compressBatchHost with the items of the device cases, sources and destinations both around 2^32 of
    their host buffers and within 64 MiB of each other"""
    case = cases[name]
    low_words, low_out = low_result(H, codec, case)
    n = len(case.src)
    src_lens = [len(s) for s in case.src]
    so, do = PL.geometry(src_lens, layout, host=True), PL.geometry(case.room, layout, host=True)
    PL.holds_what_it_is_for(so, src_lens, layout, host=True); PL.holds_what_it_is_for(do, case.room, layout, host=True)
    src, dst = HostBig(), HostBig()
    try:
        for buf, offs, lens in ((src, so, src_lens), (dst, do, case.room)):
            for o, ln in list(zip(offs, lens)) + [(o, ln) for o, ln, _ in PL.guard_windows(offs, lens)]:
                buf.write(o, bytes([CANARY]) * ln)
        for o, s in zip(so, case.src):
            src.write(o, s)
        words = np.full(n, 0xDEAD, dtype=np.uint32)
        so_a, ss_a, do_a = u64(so), u32(src_lens), u64(do)
        if name.startswith("decompress"):
            caps = u32(case.room)
            rc = L.zsmi_decompressBatchHost(codec.ctx, p(src.p), R.ptr(so_a), R.ptr(ss_a), n, p(dst.p), R.ptr(do_a), R.ptr(caps), R.ptr(words))
        else:
            rc = L.zsmi_compressBatchHost(codec.ctx, p(src.p), R.ptr(so_a), R.ptr(ss_a), n, p(dst.p), R.ptr(do_a), R.ptr(words), int(name[-1]))
        assert rc == 0
        words = [int(w) for w in words]
        assert words == low_words, (name, layout, [(i, hex(a), hex(b)) for i, (a, b) in enumerate(zip(words, low_words)) if a != b])
        for i, (o, w) in enumerate(zip(do, words)):
            assert dst.read(o, w if w < B.ERR else 0) == low_out[i], (name, layout, "bytes of item", i)
        PL.assert_guards(dst.read, do, case.room, what=(name, layout, "host destination"))
        for i, (o, s) in enumerate(zip(so, case.src)):
            assert src.read(o, len(s)) == s, (name, layout, "host source changed", i)
        PL.assert_guards(src.read, so, src_lens, what=(name, layout, "host source"))
    finally:
        codec.sync()
        src.close(); dst.close()
