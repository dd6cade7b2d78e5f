"""Batches of range reads through an opened seekable archive (zsmi_openSeekable*, zsmi_seekableReadRanges*).  Expected bytes are slices of
the input, expected codes the constants test_gpu_seekable.py pins for the same damage, the expected number of decoded frames comes from the
Python statement of the span rule (tests/_seekable_ranges.py); nothing is compared with another call of the library.  Every device read
lands in one buffer with a canary gap around every range (R.read_ranges checks the gaps)."""
import ctypes
import numpy as np
import pytest
import _corpus as C
import _data as D
import _oracle as O
import _seekable as S
import _seekable_ranges as R
import test_gpu_seekable as G
from _hip import hip_of, Dev, CANARY, PAD

pytestmark = pytest.mark.gpu
E_PREFIX, E_CORRUPT, E_CHECKSUM, E_OUT_OF_BOUND, E_TOO_SMALL = 10, 20, 22, 42, 70
F = 65536


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


@pytest.fixture(scope="module")
def data():
    return D.zipf_log(1000000).tobytes()


@pytest.fixture(scope="module")
def arcs(L, data):
    """the archives of 1 000 000 bytes that several tests read, made once"""
    return {(fs, ck): G.compress(L, data, 3, fs, ck) for fs, ck in ((65536, 1), (100000, 0), (4095, 1))}


def opened(L, codec, arc):
    sk, err = R.open_host(L, codec.ctx, arc)
    assert sk and err == 0, err
    return sk


def check_batch(b, data, ranges, rows):
    assert b.rc == 0
    for r, (o, n) in enumerate(ranges):
        assert b.out[r] == data[o:o + n], (r, o, n)
    assert b.status == [0] * len(ranges)
    assert b.frames_decoded == len(R.frames_touched(rows, ranges)[1])


# ------------------------------------------------------------------ 1. equality, both open forms
@pytest.mark.parametrize("fs,ck", [(65536, 1), (100000, 0), (4095, 1)])
def test_batch_equals_slices_both_open_forms(L, hip, codec, data, arcs, fs, ck):
    arc = arcs[(fs, ck)]
    rows, _ = S.parse(arc)
    ranges = G.ranges(len(data), fs)
    ranges = ranges + ranges[::-1]                                   # every range twice, many overlap
    table = 17 + len(rows) * (12 if ck else 8)
    sk = opened(L, codec, arc)
    dev = Dev(hip, len(arc), arc)
    skd, err = R.open_device(L, codec.ctx, dev.p, len(arc))
    try:
        assert skd and err == 0
        for h in (sk, skd):
            assert L.zsmi_getNumFrames_fromSeekable(h) == len(rows) and L.zsmi_getContentSize_fromSeekable(h) == len(data)
        assert L.zsmi_sizeofSeekable(sk) == len(arc) - table and L.zsmi_sizeofSeekable(skd) == 0
        for h in (sk, skd):
            check_batch(R.read_ranges(L, hip, codec, h, ranges, len(data)), data, ranges, rows)
            one = [(0, len(data))]                                   # every frame owned: straight into dDst
            check_batch(R.read_ranges(L, hip, codec, h, one, len(data)), data, one, rows)
    finally:
        codec.sync()
        L.zsmi_closeSeekable(sk); L.zsmi_closeSeekable(skd)
        dev.free()


# ------------------------------------------------------------------ 2. gather edges
def test_gather_edges(L, hip, codec):
    mib = 1 << 20
    big = D.zipf_log(3 * mib + 5, seed_lo=0x21).tobytes()
    arc = G.compress(L, big, 3, mib, 1)
    rows, _ = S.parse(arc)
    ranges, res = [], []
    for n in (0, 1, 15, 16, 17, 63, 64, 65, 4095, 4096, 4097, 65535, 65536, 65537, 200001):
        for k in range(16):
            ranges.append((mib + k, n)); res.append((5 * k + 3) % 16)
    ranges.append((7, 2 * mib + 3)); res.append(0)                   # a partial frame on each side of a whole one: pieces of many tiles
    sk = opened(L, codec, arc)
    try:
        b = R.read_ranges(L, hip, codec, sk, ranges, len(big), residue=lambda r: res[r])
        check_batch(b, big, ranges, rows)
        assert b.frames_decoded == 3
        # the long range alone: the middle frame is its own (decoded in place), the outer two go through the gather
        alone = [(7, 2 * mib + 3)]
        for shift in (0, 9):
            check_batch(R.read_ranges(L, hip, codec, sk, alone, len(big), residue=lambda r: shift), big, alone, rows)
    finally:
        codec.sync()
        L.zsmi_closeSeekable(sk)


# ------------------------------------------------------------------ 3. decode once
def test_shared_frames_decode_once(L, hip, codec, data, arcs):
    arc = arcs[(65536, 1)]
    rows, _ = S.parse(arc)
    rng = np.random.default_rng(3)
    sk = opened(L, codec, arc)
    try:
        in2 = [(int(o), 1) for o in rng.integers(2 * F, 3 * F, 4096)]
        b = R.read_ranges(L, hip, codec, sk, in2, len(data))
        check_batch(b, data, in2, rows)
        assert b.frames_decoded == 1
        in25 = [(2 * F, 1), (3 * F + 5, 1), (4 * F + 7, 1), (6 * F - 1, 1)] + [(int(o), 1) for o in rng.integers(2 * F, 6 * F, 4092)]
        few = R.read_ranges(L, hip, codec, sk, in25[:8], len(data))
        held = (L.zsmi_decodeScratchBytes(codec.ctx), L.zsmi_sizeofSeekable(sk))
        many = R.read_ranges(L, hip, codec, sk, in25, len(data))
        check_batch(few, data, in25[:8], rows)
        check_batch(many, data, in25, rows)
        assert few.frames_decoded == 4 and many.frames_decoded == 4
        assert (L.zsmi_decodeScratchBytes(codec.ctx), L.zsmi_sizeofSeekable(sk)) == held, "scratch grew with the number of ranges"
    finally:
        codec.sync()
        L.zsmi_closeSeekable(sk)


# ------------------------------------------------------------------ 4. many short reads, and the host form
def test_many_short_reads_device_and_host(L, hip, codec, data, arcs):
    arc = arcs[(4095, 1)]
    rows, _ = S.parse(arc)
    assert len(rows) == 245
    rng = np.random.default_rng(4)
    ranges = [(int(o), int(n)) for o, n in zip(rng.integers(0, len(data), 4096), rng.integers(1, 5001, 4096))]
    sk = opened(L, codec, arc)
    try:
        check_batch(R.read_ranges(L, hip, codec, sk, ranges, len(data)), data, ranges, rows)
        want = [data[o:o + n] for o, n in ranges]
        total = sum(map(len, want))
        off, ln = R.u64([r[0] for r in ranges]), R.u64([r[1] for r in ranges])
        written, codes = np.zeros(4096, dtype=np.uint64), np.full(4096, 9, dtype=np.uint32)
        out = np.full(total, CANARY, dtype=np.uint8)
        assert L.zsmi_seekableReadRangesHost(codec.ctx, sk, R.ptr(off), R.ptr(ln), 4096, R.ptr(out), total - 1, R.ptr(written), R.ptr(codes)) == E_TOO_SMALL
        assert bool(np.all(out == CANARY)) and not written.any() and bool(np.all(codes == 9))
        assert L.zsmi_seekableReadRangesHost(codec.ctx, sk, R.ptr(off), R.ptr(ln), 4096, R.ptr(out), total, R.ptr(written), R.ptr(codes)) == 0
        assert [int(w) for w in written] == [len(w) for w in want] and int(written.sum()) == total
        assert out.tobytes() == b"".join(want) and not codes.any()
    finally:
        L.zsmi_closeSeekable(sk)


# ------------------------------------------------------------------ 5. per-range status
def test_per_range_status(L, hip, codec):
    data = D.zipf_log(640000, seed_lo=0x55).tobytes()
    arc = G.compress(L, data, 3, F, 1)
    rows, _ = S.parse(arc)
    f = F
    ranges = [(0, 3 * f), (3 * f - 1, 1), (4 * f, 2 * f), (7 * f, len(data)), (2 * f + 5, 100), (4 * f, 1),
              (3 * f, 1), (3 * f - 1, 2), (4 * f - 1, 1), (0, len(data)), (3 * f + 100, 4096),
              (6 * f, 1), (7 * f - 1, 1), (5 * f, 3 * f), (6 * f + 100, 4096), (4 * f, len(data)), (2 * f, 10), (0, 10), (4 * f, 10), (5 * f, 10)]
    bad_magic = G.damaged(arc, 3, 0, 0xFF)
    bad_payload = G.damaged(arc, 6, rows[6][0] // 2, 0x10)
    both = G.damaged(bad_magic, 6, rows[6][0] // 2, 0x10)
    t0 = len(arc) - (17 + 12 * len(rows))
    short = arc[:t0] + S.table([(c, d - (i == 2), h) for i, (c, d, h) in enumerate(rows)], True)
    wrong = arc[:t0] + S.table([(c, d, h ^ (i == 4)) for i, (c, d, h) in enumerate(rows)], True)
    payload = (E_CORRUPT, E_CHECKSUM)
    cases = [(bad_magic, {3: (E_PREFIX,)}), (bad_payload, {6: payload}), (both, {3: (E_PREFIX,), 6: payload}),
             (short, {2: (E_CORRUPT,)}), (wrong, {4: (E_CHECKSUM,)})]
    for a, bad in cases:
        arows, _ = S.parse(a)
        # the content the table states: frame i's first Decompressed_Size bytes (the short entry moves everything behind it by one byte)
        content = b"".join(data[i * f:i * f + r[1]] for i, r in enumerate(arows))
        rs = [(o, n) for o, n in ranges if o <= len(content)]
        per, union = R.frames_touched(arows, rs)
        sk = opened(L, codec, a)
        try:
            b = R.read_ranges(L, hip, codec, sk, rs, len(content))       # (the canaries: a failed range wrote nothing outside its own span)
        finally:
            codec.sync()
            L.zsmi_closeSeekable(sk)
        assert b.rc == 0 and b.frames_decoded == len(union)
        seen = set()
        for r, (o, n) in enumerate(rs):
            hit = [i for i in per[r] if i in bad]
            if hit:
                assert b.status[r] in bad[hit[0]], (r, o, n, b.status[r])      # the earliest damaged frame decides
                seen.add(hit[0])
            else:
                assert b.status[r] == 0 and b.out[r] == content[o:o + n], (r, o, n)
        assert seen == set(bad) and any(not set(p) & set(bad) for p in per)


# ------------------------------------------------------------------ 6. edges of the call
def test_call_edges(L, hip, codec, data, arcs):
    arc = arcs[(65536, 1)]
    rows, _ = S.parse(arc)
    sk = opened(L, codec, arc)
    try:
        b = R.read_ranges(L, hip, codec, sk, [], len(data))
        assert b.rc == 0 and b.frames_decoded == 0
        empty = [(0, 0), (5, 0), (len(data), 10)]
        b = R.read_ranges(L, hip, codec, sk, empty, len(data))
        assert b.rc == 0 and b.written == [0, 0, 0] and b.status == [0, 0, 0] and b.frames_decoded == 0
        b = R.read_ranges(L, hip, codec, sk, [(0, 10), (len(data) + 1, 1), (F, 100)], len(data))
        assert b.rc == E_OUT_OF_BOUND and b.written == [0xDEAD] * 3 and b.status_raw == bytes([CANARY]) * 12 and b.frames_decoded == 0xDEAD
        z = R.u64([0])
        assert L.zsmi_seekableReadRangesDevice(codec.ctx, None, R.ptr(z), R.ptr(z), 1, None, R.ptr(z), R.ptr(z), None, None) == 1
        assert L.zsmi_seekableReadRangesDevice(codec.ctx, sk, None, R.ptr(z), 1, None, R.ptr(z), R.ptr(z), None, None) == 1
    finally:
        codec.sync()
        L.zsmi_closeSeekable(sk)
    table = S.table([], True)
    assert len(table) == 17
    sk = opened(L, codec, table)
    try:
        assert L.zsmi_getNumFrames_fromSeekable(sk) == 0 and L.zsmi_getContentSize_fromSeekable(sk) == 0 and L.zsmi_sizeofSeekable(sk) == 0
        b = R.read_ranges(L, hip, codec, sk, [(0, 100)], 0)
        assert b.rc == 0 and b.written == [0] and b.status == [0] and b.out == [b""]
    finally:
        L.zsmi_closeSeekable(sk)


# ------------------------------------------------------------------ 7. archives of libzstd's frames
def test_foreign_archives_in_one_call(L, hip, codec):
    if O.libzstd() is None:
        pytest.skip("libzstd is not on this machine")
    text = C.json_records(2800000)
    parts = [text[:70000], text[70000:70001], text[70001:200000], text[200000:2700000], b"", text[:5000]]   # part 3: > 16 blocks (general kernel)
    data = b"".join(parts)
    at = 2700000                                                            # where the empty part sits
    ranges = [(0, len(data)), (69999, 3), (150000, 100000), (len(data) - 4999, 4999), (300000, 4096),
              (at, 0), (at, 10), (at - 10, 10), (at - 10, 20), (at, len(data))]
    for ck_table in (True, False):
        arc = S.zstd_archive(parts, ck_table, frame_checksums=(0, 2, 3))
        rows, _ = S.parse(arc)
        sk = opened(L, codec, arc)
        try:
            check_batch(R.read_ranges(L, hip, codec, sk, ranges, len(data)), data, ranges, rows)
            for alone in ((at - 10, 20), (0, len(data))):                  # the empty part between the frames of a single range
                check_batch(R.read_ranges(L, hip, codec, sk, [alone], len(data)), data, [alone], rows)
        finally:
            codec.sync()
            L.zsmi_closeSeekable(sk)


# ------------------------------------------------------------------ 8. Python surface
def test_python_surface(L, hip, codec):
    from zstandard_amd import SeekableArchive, ZstdCompressor
    data = D.zipf_log(300000, seed_lo=0x66).tobytes()
    arc = ZstdCompressor(3).compress_seekable(data, frame_size=50000)
    ranges = [(0, 10), (49999, 3), (299990, 100), (120000, 100000), (300000, 5), (7, 0), (0, len(data)), (49999, 3)]
    a = SeekableArchive(arc)
    assert a.read_many(ranges) == [data[o:o + n] for o, n in ranges]
    assert a.read_many([]) == []
    with pytest.raises(RuntimeError, match="Parameter is out of bound"):
        a.read_many([(0, 1), (len(data) + 1, 1)])
    a.close()
    bad = SeekableArchive(G.damaged(arc, 1, 0, 0xFF))                       # frame 1: content [50000, 100000)
    got, codes = bad.read_many(ranges[:6], return_codes=True)
    assert codes == [0, E_PREFIX, 0, 0, 0, 0]
    assert [g for g, c in zip(got, codes) if not c] == [data[o:o + n] for (o, n), c in zip(ranges, codes) if not c]
    with pytest.raises(RuntimeError, match=r"Unknown frame descriptor \(range 1\)"):
        bad.read_many(ranges[:6])
    bad.close()
    dev = Dev(hip, len(arc), arc)
    h = codec.open_seekable_device(dev.p, len(arc))
    assert (h.num_frames, h.content_size, h.device_bytes) == (6, len(data), 0)
    out, st = Dev(hip, 200000), Dev(hip, 4 * 3)
    rs = [(49999, 3), (120000, 100000), (299990, 100)]
    written, frames = h.read_ranges_device([r[0] for r in rs], [r[1] for r in rs], out.p, [0, 100, 150000], st.p)
    codec.sync()
    buf = out.all()[PAD:]
    assert list(written) == [3, 100000, 10] and frames == len(R.frames_touched(S.parse(arc)[0], rs)[1]) == 6 and st.all()[PAD:PAD + 12] == bytes(12)
    for (o, n), to in zip(rs, (0, 100, 150000)):
        assert buf[to:to + len(data[o:o + n])] == data[o:o + n]
    h.close()
    for b in (dev, out, st):
        b.free()
