"""The frame index on the GPU: zsmi_openFramesDevice builds on the device the table the Python statement of the index gives
(tests/_frames_index.py) and zsmi_openFrames builds on the host - for the good stream with its false magic numbers, every bad stream with
its code, 5000 small frames (more than two scan tiles, 13 doubling rounds), and the same stream at an odd address between junk that starts
with a magic number.  The handles are ordinary ones: ranges, frames by number and resident reads are checked against the frames' contents,
a stream packed by zsmi_packFramesDevice from a CDict set's frames reads back through a DDict set, and a damaged payload fails exactly the
ranges that touch it.  Every device call writes into canary-guarded buffers."""
import ctypes
import numpy as np
import pytest
import _batch as B
import _dicts as X
import _frames_index as F
import _seekable_ranges as R
import _seekable_resident as RR
import test_gpu_seekable_frames as GF
from _hip import hip_of, Dev, CANARY, PAD

pytestmark = pytest.mark.gpu
E_CORRUPT, E_CHECKSUM, E_DICT_WRONG = 20, 22, 32
NO_DICT = 0xFFFFFFFF


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
def records():
    stream, contents = F.records_stream()
    return stream, contents


def open_host(L, codec, stream, dset=None):
    err = ctypes.c_int(-1)
    sk = L.zsmi_openFrames_usingDDictSet(codec.ctx, stream, len(stream), dset.handle if dset is not None else None, ctypes.byref(err))
    return sk, err.value


def open_device(L, codec, d_ptr, size, dset=None):
    err = ctypes.c_int(-1)
    sk = L.zsmi_openFramesDevice_usingDDictSet(codec.ctx, ctypes.c_void_p(d_ptr), size, dset.handle if dset is not None else None, ctypes.byref(err))
    return sk, err.value


def table_of(L, sk):
    """[(pos, cSize, dSize)] from the handle, with the content offsets checked to be the running sum"""
    rows, do = [], 0
    for i in range(L.zsmi_getNumFrames_fromSeekable(sk)):
        v = (ctypes.c_uint64(7), ctypes.c_uint64(7), ctypes.c_uint32(7), ctypes.c_uint32(7))
        assert L.zsmi_getFrameInfo_fromSeekable(sk, i, *[ctypes.byref(x) for x in v]) == 0
        assert v[1].value == do, i
        rows.append((v[0].value, v[2].value, v[3].value))
        do += v[3].value
    assert L.zsmi_getContentSize_fromSeekable(sk) == do
    return rows


def rows_for_reads(rows):
    return [(c, d, None) for _, c, d in rows]


# ------------------------------------------------------------------ 1. the same table from both open calls
def test_good_stream_same_table_from_both_open_calls(L, hip, codec):
    good = F.good_stream()
    want, c = F.index(L, good)
    assert c == 0
    dev = Dev(hip, len(good), good)
    sk, e1 = open_host(L, codec, good)
    skd, e2 = open_device(L, codec, dev.p, len(good))
    try:
        assert sk and skd and (e1, e2) == (0, 0)
        assert table_of(L, skd) == want and table_of(L, sk) == want
        assert L.zsmi_sizeofSeekable(sk) == len(good) and L.zsmi_sizeofSeekable(skd) == 0
        raw = np.frombuffer(dev.all(), dtype=np.uint8)
        assert (raw[:PAD] == CANARY).all() and (raw[PAD + len(good):] == CANARY).all() and raw[PAD:PAD + len(good)].tobytes() == good
    finally:
        codec.sync()
        L.zsmi_closeSeekable(sk); L.zsmi_closeSeekable(skd)
        dev.free()


def test_bad_streams_same_code_from_the_device(L, hip, codec):
    bad = F.bad_streams()
    total = sum(len(s) + 64 for s in bad.values())
    dev = Dev(hip, total)
    try:
        at = 0
        for name in sorted(bad):
            s = bad[name]
            _, want = F.index(L, s)
            assert want, name
            assert hip.hipMemcpy(ctypes.c_void_p(dev.p + at), s, len(s), 1) == 0
            sk, e = open_device(L, codec, dev.p + at, len(s))
            assert not sk and e == want, (name, e, want)
            sk, e = open_host(L, codec, s)
            assert not sk and e == want, (name, e, want)
            at += len(s) + 61                                                # (odd distances: every alignment of a stream's start)
        sk, e = open_device(L, codec, dev.p, 0)                              # the empty stream: a handle of 0 frames
        assert sk and e == 0 and L.zsmi_getNumFrames_fromSeekable(sk) == 0 and L.zsmi_getContentSize_fromSeekable(sk) == 0
        L.zsmi_closeSeekable(sk)
        sk, e = open_device(L, codec, 0, 12)
        assert not sk and e == F.E_SRC_SIZE
    finally:
        codec.sync()
        dev.free()


# ------------------------------------------------------------------ 2. reads on the good stream
def test_reads_on_the_good_stream(L, hip, codec):
    good, parts = F.good_stream(), F.good_parts()
    content = b"".join(c for _, c in parts)
    want, _ = F.index(L, good)
    rows = rows_for_reads(want)
    dev = Dev(hip, len(good), good)
    skd, e = open_device(L, codec, dev.p, len(good))
    try:
        assert skd and e == 0
        b = R.read_ranges(L, hip, codec, skd, [(0, len(content))], len(content))
        assert b.rc == 0 and b.status == [0] and b.out[0] == content
        assert b.frames_decoded == len(R.frames_touched(rows, [(0, len(content))])[1])
        out = ctypes.create_string_buffer(len(content))
        assert L.zsmi_decompress(out, len(content), good, len(good)) == len(content) and out.raw == content
        idx = [int(i) for i in np.random.default_rng(3).permutation(len(want))]
        f = GF.read_frames(L, hip, codec, skd, idx, rows, seed=2)
        assert f.rc == 0 and f.status == [0] * len(idx) and f.written == [want[i][2] for i in idx]
        assert f.out == [parts[i][1] for i in idx]
        cap = int(RR.rounded_offsets([want[i][2] for i in idx], 16)[-1])
        r = RR.read(L, hip, codec, skd, idx, 16, cap)
        assert r.rc == 0 and r.status.tolist() == [0] * len(idx) and r.written.tolist() == [want[i][2] for i in idx]
        assert (r.offsets == RR.rounded_offsets([want[i][2] for i in idx], 16)).all()
        for k, i in enumerate(idx):
            assert r.out(k, want[i][2]) == parts[i][1], (k, i)
    finally:
        codec.sync()
        L.zsmi_closeSeekable(skd)
        dev.free()


# ------------------------------------------------------------------ 3. scale, and nothing outside [dSrc, dSrc + size)
def test_5000_frames(L, hip, codec, records):
    stream, contents = records
    want, c = F.index(L, stream)
    assert c == 0 and len(want) == len(contents) == 5000
    dev = Dev(hip, len(stream), stream)
    skd, e = open_device(L, codec, dev.p, len(stream))
    try:
        assert skd and e == 0
        assert table_of(L, skd) == want
        idx = [int(i) for i in np.random.default_rng(8).integers(0, len(want), 512)]
        f = GF.read_frames(L, hip, codec, skd, idx, rows_for_reads(want), seed=6)
        assert f.rc == 0 and not any(f.status) and f.out == [contents[i] for i in idx]
    finally:
        codec.sync()
        L.zsmi_closeSeekable(skd)
        dev.free()


@pytest.mark.parametrize("shift", [1, 7, 13])
def test_odd_address_between_junk(L, hip, codec, records, shift):
    stream, _ = records
    want, _ = F.index(L, stream)
    junk = lambda m: (m.to_bytes(4, "little") + bytes(range(60)))
    front, behind = junk(F.ZSTD_MAGIC), junk(F.SKIP_MAGIC + 2)
    image = bytes(shift) + front + stream + behind
    dev = Dev(hip, len(image), image)
    skd, e = open_device(L, codec, dev.p + shift + len(front), len(stream))
    try:
        assert skd and e == 0
        assert table_of(L, skd) == want
    finally:
        codec.sync()
        L.zsmi_closeSeekable(skd)
        dev.free()


# ------------------------------------------------------------------ 4. dictionaries: a CDict set's frames, packed, no table
def test_packed_frames_of_a_cdict_set(L, hip, codec):
    from zstandard_amd import CompressionDict, CompressionDictSet, DecompressionDict, DecompressionDictSet
    classes = ("json_records", "zipf")
    dicts = [X.trained(c) for c in classes]
    rng = np.random.default_rng(17)
    choice, chunks = [], []
    for i in range(60):
        ch = (0, 1, NO_DICT)[i % 3]
        data = X.class_data(classes[ch] if ch != NO_DICT else "csv_records")
        size = int(rng.integers(1, 5000)); o = int(rng.integers(0, len(data) - size))
        choice.append(ch); chunks.append(data[o:o + size])
    cds = [CompressionDict(codec, d, 3) for d in dicts]
    cset = CompressionDictSet(codec, cds, 3)
    dds = [DecompressionDict(codec, d) for d in dicts]
    dset = DecompressionDictSet(codec, dds)
    src_b, so, ss = B.batch(chunks)
    bounds = np.array([L.zsmi_compressBound(int(s)) for s in ss], dtype=np.uint64)
    do = B.layout(bounds)
    total = int(bounds.sum())
    n = len(chunks)
    src, dst, szs, packed, poff = Dev(hip, len(src_b), src_b.tobytes()), Dev(hip, total), Dev(hip, 4 * n), Dev(hip, total), Dev(hip, 8 * (n + 1))
    sk = sk0 = None
    try:
        codec.compress_device(src.p, so, ss, dst.p, do, szs.p, cdict_set=cset, dict_index=np.array(choice, dtype=np.uint32))
        codec.pack_device(dst.p, do, szs.p, n, packed.p, poff.p)
        codec.sync()
        size = int(np.frombuffer(poff.all()[PAD:PAD + 8 * (n + 1)], dtype=np.uint64)[n])
        sk, e = open_device(L, codec, packed.p, size, dset)
        assert sk and e == 0 and L.zsmi_getNumFrames_fromSeekable(sk) == n
        rows = table_of(L, sk)
        assert [d for _, _, d in rows] == [len(c) for c in chunks]
        idx = list(range(n))
        f = GF.read_frames(L, hip, codec, sk, idx, rows_for_reads(rows))
        assert f.rc == 0 and not any(f.status) and f.out == chunks
        sk0, e = open_device(L, codec, packed.p, size)                        # the same stream without the set
        assert sk0 and e == 0 and table_of(L, sk0) == rows
        f = GF.read_frames(L, hip, codec, sk0, idx, rows_for_reads(rows))
        assert f.rc == 0 and f.status == [E_DICT_WRONG if ch != NO_DICT else 0 for ch in choice]
        assert all(f.out[i] == chunks[i] for i in idx if choice[i] == NO_DICT)
    finally:
        codec.sync()
        for h in (sk, sk0):
            if h:
                L.zsmi_closeSeekable(h)
        dset.close(); cset.close()
        for h in cds + dds:
            h.close()
        for d in (src, dst, szs, packed, poff):
            d.free()


# ------------------------------------------------------------------ 5. damage: the index saw only headers
def test_damage_fails_exactly_the_ranges_that_touch_it(L, hip, codec, records):
    stream, contents = records
    want, _ = F.index(L, stream)
    n = 40
    k = 22                                                                   # a raw-block frame with a Content_Checksum (i & 1 == 0, i & 2)
    part = bytearray(stream[:want[n][0]])
    assert k & 3 == 2
    part[want[k][0] + want[k][1] // 2] ^= 0x10                               # a payload byte: the frame's header and its block header stay
    part = bytes(part)
    assert F.index(L, part) == (want[:n], 0)
    d = [0]
    for c in contents[:n]:
        d.append(d[-1] + len(c))
    content = b"".join(contents[:n])
    sk, e = open_host(L, codec, part)
    try:
        assert sk and e == 0
        extent = lambda i: (d[i], d[i + 1] - d[i])
        ranges = [extent(k - 1), extent(k), (d[k] - 1, 2), (d[k + 1] - 1, 2), (d[k] + 5, 1), extent(k + 1), (0, d[k]), (d[k + 1], d[-1] - d[k + 1]), (0, d[-1])]
        touch = [False, True, True, True, True, False, False, False, True]
        b = R.read_ranges(L, hip, codec, sk, ranges, len(content))
        assert b.rc == 0
        for j, ((o, ln), t) in enumerate(zip(ranges, touch)):
            if t:
                assert b.status[j] in (E_CORRUPT, E_CHECKSUM), (j, b.status[j])
            else:
                assert b.status[j] == 0 and b.out[j] == content[o:o + ln], j
    finally:
        codec.sync()
        L.zsmi_closeSeekable(sk)


# ------------------------------------------------------------------ 6. the Python surface
def test_python_surface(L, hip, codec):
    from zstandard_amd import SeekableArchive
    good, parts = F.good_stream(), F.good_parts()
    content = b"".join(c for _, c in parts)
    arc = SeekableArchive.from_frames(good)
    try:
        assert arc.read() == content and arc.read(5, 100) == content[5:105]
        assert arc.read_frames([2, 0, -1]) == [parts[2][1], parts[0][1], parts[-1][1]]
        assert arc.read_many([(0, 10), (100000, 70000)]) == [content[:10], content[100000:170000]]
    finally:
        arc.close()
    dev = Dev(hip, len(good), good)
    h = codec.open_frames_device(dev.p, len(good))
    try:
        assert h.num_frames == len(parts) and h.content_size == len(content) and h.device_bytes == 0
        assert h.frame_info(1) == (len(parts[0][0]), 0, len(parts[1][0]), 1)
        with pytest.raises(RuntimeError, match="zsmi_openFramesDevice"):
            codec.open_frames_device(dev.p, len(good) - 1)
    finally:
        codec.sync()
        h.close()
        dev.free()
