"""Record archives on the GPU: the caller's frame sizes and a dictionary per frame (zsmi_compressSeekableFrames*), read back through a handle
that decodes with a DDict set (zsmi_openSeekable*_usingDDictSet) and by frame index (zsmi_seekableReadFrames*).  An archive must equal, byte
for byte, the frames the batch compress call gives the same chunks followed by the table tests/_seekable.py writes; where an oracle can state
a frame (no dictionary, raw content) it must equal oracle E's, and every frame must decode under oracle D with its own dictionary.  Reads
must equal slices of the content; the expected number of decoded frames comes from the Python statement of the span rule
(tests/_seekable_ranges.py).  Every device call writes into canary-guarded buffers.  (A set of another device needs a second GPU: that one
refusal is not exercised here.)"""
import ctypes
import numpy as np
import pytest
import _batch as B
import _cdict_set as CS
import _data as D
import _dicts as X
import _oracle as O
import _seekable as S
import _seekable_ranges as R
import test_gpu_seekable as G
from _hip import hip_of, Dev, CANARY, PAD

pytestmark = pytest.mark.gpu
E_GENERIC, E_CORRUPT, E_CHECKSUM, E_DICT_WRONG, E_OUT_OF_BOUND, E_TOO_SMALL, E_FRAME_INDEX = 1, 20, 22, 32, 42, 70, 100
NO_DICT = CS.NO_DICT


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


def u32(a):
    return np.ascontiguousarray(a, dtype=np.uint32)


def frames_bound(L, sizes, flag):
    fs = u32(sizes)
    r = L.zsmi_seekableFramesBound(R.ptr(fs) if len(fs) else None, len(fs), flag)
    assert not L.zsmi_isError(r)
    return r


def compress_frames(L, H, codec, parts, level, flag, cset=None, index=None):
    """the device call into a canary-guarded buffer of exactly the bound: the archive; nothing outside [0, archive size) may change"""
    content = b"".join(parts)
    fs = u32([len(p) for p in parts])
    n = len(parts)
    bound = frames_bound(L, fs, flag)
    src, dst, sz = Dev(H, max(len(content), 1), content), Dev(H, bound), Dev(H, 8)
    fp = R.ptr(fs) if n else None
    try:
        if cset is None:
            rc = L.zsmi_compressSeekableFramesDevice(codec.ctx, ctypes.c_void_p(src.p), fp, n, ctypes.c_void_p(dst.p), bound, ctypes.c_void_p(sz.p), level, flag)
        else:
            ip = R.ptr(u32(index)) if index is not None else None
            rc = L.zsmi_compressSeekableFramesDevice_usingCDictSet(codec.ctx, ctypes.c_void_p(src.p), fp, n, ctypes.c_void_p(dst.p), bound, ctypes.c_void_p(sz.p),
                                                                   flag, cset.handle, ip)
        assert rc == 0, rc
        codec.sync()
        sbuf = sz.all()
        size = int.from_bytes(sbuf[PAD:PAD + 8], "little")
        assert size <= bound, hex(size)
        assert sbuf[:PAD] == bytes([CANARY]) * PAD and sbuf[PAD + 8:] == bytes([CANARY]) * PAD, "wrote outside *dArchiveSize"
        buf = np.frombuffer(dst.all(), dtype=np.uint8)
        assert bool(np.all(buf[:PAD] == CANARY)) and bool(np.all(buf[PAD + size:] == CANARY)), "wrote outside [dDst, dDst + archive size)"
        return buf[PAD:PAD + size].tobytes()
    finally:
        for b in (src, dst, sz):
            b.free()


def batch_frames(L, H, codec, parts, level, cset=None, index=None):
    """frame i of zsmi_compressBatchDevice (at level) or zsmi_compressBatchDevice_usingCDictSet over the same chunks, each in a slot of its bound"""
    src_b, so, ss = B.batch(parts)
    bounds = np.array([L.zsmi_compressBound(int(s)) for s in ss], dtype=np.uint64)
    do = B.layout(bounds)
    total = int(bounds.sum())
    src, dst, szs = Dev(H, len(src_b), src_b.tobytes()), Dev(H, total), Dev(H, 4 * len(parts))
    try:
        if cset is None:
            codec.compress_device(src.p, so, ss, dst.p, do, szs.p, level)
        else:
            codec.compress_device(src.p, so, ss, dst.p, do, szs.p, cdict_set=cset, dict_index=u32(index))
        codec.sync()
        sizes = np.frombuffer(szs.all()[PAD:PAD + 4 * len(parts)], dtype=np.uint32)
        assert bool(np.all(sizes <= bounds)), "a chunk failed"
        return B.cut(np.frombuffer(dst.all(), dtype=np.uint8)[PAD:PAD + total], do, sizes)
    finally:
        for b in (src, dst, szs):
            b.free()


# ------------------------------------------------------------------ 1. the mixed batch, byte for byte
_cdicts = {}


def member_cdicts(codec, level):
    from zstandard_amd import CompressionDict
    if level not in _cdicts:
        names = [n for n, _ in CS.members()]
        cds = [None if n == "again" else CompressionDict(codec, d, level) for n, d in CS.members()]
        cds[names.index("again")] = cds[names.index(CS.AGAIN_OF)]
        _cdicts[level] = cds
    return _cdicts[level]


@pytest.mark.parametrize("level", [1, 3])
def test_mixed_batch_byte_for_byte(L, hip, codec, level):
    from zstandard_amd import CompressionDictSet
    chunks, index = CS.chunks(), CS.choices()
    cset = CompressionDictSet(codec, member_cdicts(codec, level), level)
    try:
        F = batch_frames(L, hip, codec, chunks, level, cset, index)
        for i, e in CS.oracle_frames(level).items():                              # oracle E: raw members, NO_DICT, the empty member
            assert F[i] == e, (level, i, CS.kind(index[i]), len(chunks[i]))
        for i, (f, c) in enumerate(zip(F, chunks)):                               # oracle D: every frame with its own dictionary
            dic = CS.dictionary(index[i])
            assert (O.decompress_using_dict(f, len(c), dic) if dic else O.decompress(f, len(c))) == c, (level, i, len(c))
        for flag in (0, 1):
            arc = compress_frames(L, hip, codec, chunks, level, flag, cset, index)
            want = S.archive(F, chunks, bool(flag))
            assert len(arc) == len(want) and arc == want, (level, flag, B.first_difference(arc, want))
            rows, ck = S.parse(arc)
            assert ck == bool(flag) and [r[1] for r in rows] == [len(c) for c in chunks]
        if level == 3:                                                            # the context's ZSMI_c_checksumFlag: the batch call's frames with it
            codec.set_parameter("checksum", 1)
            try:
                Fc = batch_frames(L, hip, codec, chunks, level, cset, index)
                arc = compress_frames(L, hip, codec, chunks, level, 1, cset, index)
            finally:
                codec.set_parameter("checksum", 0)
            assert [len(f) for f in Fc] == [len(f) + 4 for f in F]
            assert arc == S.archive(Fc, chunks, True)
    finally:
        codec.sync()
        cset.close()


# ------------------------------------------------------------------ 2. the plain form and the edges
def oracle_archive(parts, level, flag):
    return S.archive([O.compress(p, level) for p in parts], parts, bool(flag))


def test_plain_form_sizes_and_counts(L, hip, codec):
    data = D.zipf_log(400000, seed_lo=0x31).tobytes()
    sizes = (0, 1, 63, 65536, 65537, 131073)
    orders = [sizes, sizes[::-1], (65537, 0, 131073, 1, 0, 63, 65536), (0, 0, 1, 0), (0,)]
    for level, flag in ((3, 1), (1, 0)):
        for order in orders:
            at = np.concatenate([[0], np.cumsum(order)])
            parts = [data[int(a):int(a) + s] for a, s in zip(at, order)]
            assert compress_frames(L, hip, codec, parts, level, flag) == oracle_archive(parts, level, flag), (level, flag, order)
        assert compress_frames(L, hip, codec, [], level, flag) == S.table([], bool(flag))              # n = 0: the 17-byte table
        assert compress_frames(L, hip, codec, [data[:3000]], level, flag) == oracle_archive([data[:3000]], level, flag)
    rng = np.random.default_rng(5)
    for n in (15, 16, 17, 255, 256, 257):                  # both sides of 16 frames a wavefront (hash) and 256 threads a workgroup (table)
        lens = rng.integers(100, 2001, n)
        at = np.concatenate([[0], np.cumsum(lens)])
        parts = [data[int(a):int(a) + int(s)] for a, s in zip(at, lens)]
        for flag in (1, 0):
            assert compress_frames(L, hip, codec, parts, 3, flag) == oracle_archive(parts, 3, flag), (n, flag)


def test_fixed_sizes_are_the_fixed_size_call(L, hip, codec):
    data = D.zipf_log(300000).tobytes()
    for F in (4095, 50000, 65536):
        parts = S.slices(data, F)
        for flag in (0, 1):
            arc = compress_frames(L, hip, codec, parts, 3, flag)
            assert arc == G.compress_device(L, hip, codec, data, 3, F, flag), (F, flag)
            assert frames_bound(L, [len(p) for p in parts], flag) == L.zsmi_seekableBound(len(data), F, flag)
    # the host form, and a set nobody picks / a NULL set: the plain form
    parts = S.slices(data, 50000)
    fs = u32([len(p) for p in parts])
    bound = frames_bound(L, fs, 1)
    out = ctypes.create_string_buffer(bound)
    r = L.zsmi_compressSeekableFramesHost(codec.ctx, out, bound, data, R.ptr(fs), len(fs), 3, 1)
    assert not L.zsmi_isError(r) and out.raw[:r] == S.oracle_archive(data, 50000, 3, True)
    r = L.zsmi_compressSeekableFramesHost_usingCDictSet(codec.ctx, out, bound, data, R.ptr(fs), len(fs), 1, None, None)
    assert not L.zsmi_isError(r) and out.raw[:r] == S.oracle_archive(data, 50000, 3, True)


# ------------------------------------------------------------------ 3. refusals, in their order
def test_refusals_in_order(L, hip, codec):
    from zstandard_amd import CompressionDict, CompressionDictSet
    data = D.zipf_log(20000).tobytes()
    cd = [CompressionDict(codec, X.TRAINED8K, 3), CompressionDict(codec, X.STREAM[:6000], 3)]
    two, one = CompressionDictSet(codec, cd, 3), CompressionDictSet(codec, cd[:1], 3)
    fs, big = u32([5000, 0, 15000]), u32([5000, (1 << 30) + 1, 3])
    zero = u32([0, 0])
    bound = frames_bound(L, fs, 1)
    src, dst, sz = Dev(hip, len(data), data), Dev(hip, bound), Dev(hip, 8)
    S_, D_, Z_ = ctypes.c_void_p(src.p), ctypes.c_void_p(dst.p), ctypes.c_void_p(sz.p)
    ctx = codec.ctx

    def plain(sizes, n, cap=bound, s=S_, d=D_, z=Z_):
        return L.zsmi_compressSeekableFramesDevice(ctx, s, R.ptr(sizes) if sizes is not None else None, n, d, cap, z, 3, 1)

    def using(sizes, n, cset, idx, cap=bound, s=S_, d=D_, z=Z_):
        return L.zsmi_compressSeekableFramesDevice_usingCDictSet(ctx, s, R.ptr(sizes) if sizes is not None else None, n, d, cap, z, 1,
                                                                 cset.handle, R.ptr(u32(idx)) if idx is not None else None)
    try:
        # the bound's three checks
        assert plain(fs, 0x8000001) == E_FRAME_INDEX and plain(None, 0x8000001) == E_FRAME_INDEX       # too many frames, before the NULL array
        assert plain(None, 1) == E_GENERIC
        assert plain(big, 3) == E_OUT_OF_BOUND
        assert plain(big, 3, cap=0, d=None) == E_OUT_OF_BOUND                                          # ... before the capacity and the NULLs
        # the dictionary choice, behind the bound's checks and in front of the capacity's
        assert using(big, 3, two, None) == E_OUT_OF_BOUND and using(None, 1, two, None) == E_GENERIC
        assert using(fs, 3, two, None) == E_GENERIC                                                    # a NULL choice with two members
        assert using(fs, 3, two, None, cap=0) == E_GENERIC
        assert using(fs, 3, two, [0, 2, 1]) == E_OUT_OF_BOUND and using(fs, 3, two, [0, 1, 0xFFFFFFFE]) == E_OUT_OF_BOUND
        assert using(fs, 3, one, [0, 1, 0]) == E_OUT_OF_BOUND
        assert using(fs, 3, two, [0, 2, 1], cap=bound - 1, d=None) == E_OUT_OF_BOUND
        # the capacity, in front of the NULLs
        assert plain(fs, 3, cap=bound - 1) == E_TOO_SMALL and plain(fs, 3, cap=bound - 1, d=None, z=None) == E_TOO_SMALL
        assert using(fs, 3, two, [0, NO_DICT, 1], cap=bound - 1) == E_TOO_SMALL and using(fs, 3, one, None, cap=0) == E_TOO_SMALL
        # the NULLs
        assert plain(fs, 3, z=None) == E_GENERIC and plain(fs, 3, d=None) == E_GENERIC and plain(fs, 3, s=None) == E_GENERIC
        assert using(fs, 3, two, [0, NO_DICT, 1], s=None) == E_GENERIC
        codec.sync()
        assert dst.all() == bytes([CANARY]) * (bound + 2 * PAD) and sz.all() == bytes([CANARY]) * (8 + 2 * PAD), "a refused call wrote"
        # what is no refusal: a NULL source without content; a NULL choice with a set of one
        assert plain(zero, 2, s=None) == 0
        codec.sync()
        n = int.from_bytes(sz.all()[PAD:PAD + 8], "little")
        assert dst.all()[PAD:PAD + n] == oracle_archive([b"", b""], 3, 1)
        parts = [data[:5000], b"", data[5000:]]
        assert compress_frames(L, hip, codec, parts, 3, 1, one, None) == compress_frames(L, hip, codec, parts, 3, 1, one, [0, 0, 0])
        assert compress_frames(L, hip, codec, parts, 3, 1, one, None) == S.archive(batch_frames(L, hip, codec, parts, 3, one, [0, 0, 0]), parts, True)
    finally:
        codec.sync()
        for b in (src, dst, sz):
            b.free()
        two.close(); one.close()
        for c in cd:
            c.close()


# ------------------------------------------------------------------ 4 - 7. reading with a DDict set
FORMATTED = ("json_records", "zipf", "binary_table")
RAW, EMPTY = 3, 4                      # the set's members: the three trained dictionaries, raw content, an empty CDict
CHOICES = (0, RAW, 1, NO_DICT, 2, EMPTY)


class Records:
    pass


@pytest.fixture(scope="module")
def recs(L, hip, codec):
    """about 200 records of 0 .. 70 KiB, their choices dealt over three formatted dictionaries, a raw-content one, an empty member and
    NO_DICT (neighbours differ), compressed into one archive with table checksums"""
    from zstandard_amd import CompressionDict, CompressionDictSet, DecompressionDict, DecompressionDictSet
    r = Records()
    rng = np.random.default_rng(11)
    n = 204
    sizes = [int(s) for s in rng.integers(50, 4001, n)]
    for k, s in ((7, 65537), (20, 70 * 1024), (45, 66000), (100, 69999), (13, 0), (14, 0), (101, 0), (n - 1, 0), (150, 65536), (30, 1)):
        sizes[k] = s
    r.choice = [CHOICES[i % len(CHOICES)] for i in range(n)]
    assert all(a != b for a, b in zip(r.choice, r.choice[1:]))
    r.dicts = [X.trained(c) for c in FORMATTED] + [X.STREAM[:6000], b""]
    assert len({O.dict_params(d)[1] for d in r.dicts[:3]}) == 3 and all(O.dict_params(d)[1] for d in r.dicts[:3])       # distinct IDs
    r.parts = []
    for i, (s, ch) in enumerate(zip(sizes, r.choice)):
        if ch == RAW:                                          # a raw-content record copies the dictionary: its frame cannot decode without it
            o = (37 * i) % 1500
            r.parts.append(X.STREAM[o:o + s])
        else:
            data = X.class_data(FORMATTED[ch] if ch < 3 else "csv_records")
            o = (i * 7919) % (len(data) - s + 1)
            r.parts.append(data[o:o + s])
    r.content = b"".join(r.parts)
    r.cds = [CompressionDict(codec, d, 3) for d in r.dicts]
    r.cset = CompressionDictSet(codec, r.cds, 3)
    r.arc = compress_frames(L, hip, codec, r.parts, 3, 1, r.cset, r.choice)
    r.rows, ck = S.parse(r.arc)
    assert ck and [row[1] for row in r.rows] == sizes
    r.d = R.content_offsets(r.rows)
    r.dds = [DecompressionDict(codec, d) for d in r.dicts[:4]]
    r.dset = DecompressionDictSet(codec, r.dds[:3], unnamed=r.dds[3])
    r.sets = [r.dset]
    yield r
    codec.sync()
    for s in r.sets:
        s.close()
    r.cset.close()
    for h in r.cds + r.dds:
        h.close()


def open_host_set(L, codec, arc, dset):
    err = ctypes.c_int(-1)
    sk = L.zsmi_openSeekable_usingDDictSet(codec.ctx, arc, len(arc), dset.handle if dset is not None else None, ctypes.byref(err))
    assert sk and err.value == 0, err.value
    return sk


def open_device_set(L, codec, dev, size, dset):
    err = ctypes.c_int(-1)
    sk = L.zsmi_openSeekableDevice_usingDDictSet(codec.ctx, ctypes.c_void_p(dev.p), size, dset.handle if dset is not None else None, ctypes.byref(err))
    assert sk and err.value == 0, err.value
    return sk


def batches(r):
    """the range batches of test 4: the whole content; every frame alone and a byte on each side of every frame edge; a sparse batch of
    ranges over two or three neighbouring frames and of ranges that share a frame"""
    d, n = r.d, len(r.rows)
    alone = [(d[i], d[i + 1] - d[i]) for i in range(n)]
    edges = [(e - 1, 1) for e in sorted(set(d[1:-1]))] + [(e, 1) for e in sorted(set(d[1:-1])) if e < d[-1]]
    sparse = []
    for i in range(2, n - 5, 17):
        sparse.append((d[i], d[i + 2] - d[i]))                                     # two whole neighbours
        a, b = d[i + 2] + (d[i + 3] - d[i + 2]) // 3, d[i + 5] - (d[i + 5] - d[i + 4]) // 3
        sparse.append((a, b - a))                                                  # three, the outer two in part
    k = 50
    half = (d[k + 1] - d[k]) // 2
    sparse += [(d[k], half), (d[k] + half, d[k + 1] - d[k] - half), (d[k] + 1, 5), (d[k], half)]      # one frame, four ranges
    return {"whole": [(0, d[-1])], "alone_and_edges": alone + edges, "sparse": sparse}


def check(b, r, ranges):
    assert b.rc == 0
    bad = [(k, s) for k, s in enumerate(b.status) if s]
    assert not bad, bad[:8]
    for k, (o, n) in enumerate(ranges):
        assert b.out[k] == r.content[o:o + n], (k, o, n)
    assert b.frames_decoded == len(R.frames_touched(r.rows, ranges)[1])


def test_read_with_a_ddict_set_both_open_forms(L, hip, codec, recs):
    r = recs
    at = 0
    for i, (row, p) in enumerate(zip(r.rows, r.parts)):                           # oracle D: every frame with its own dictionary
        f = r.arc[at:at + row[0]]
        at += row[0]
        dic = b"" if r.choice[i] == NO_DICT else r.dicts[r.choice[i]]
        assert (O.decompress_using_dict(f, len(p), dic) if dic else O.decompress(f, len(p))) == p, i
    dev = Dev(hip, len(r.arc), r.arc)
    sk, skd = open_host_set(L, codec, r.arc, r.dset), open_device_set(L, codec, dev, len(r.arc), r.dset)
    try:
        for h in (sk, skd):
            assert L.zsmi_getNumFrames_fromSeekable(h) == len(r.rows) and L.zsmi_getContentSize_fromSeekable(h) == len(r.content)
            for name, ranges in batches(r).items():
                check(R.read_ranges(L, hip, codec, h, ranges, len(r.content), seed=len(ranges)), r, ranges)
        sparse = batches(r)["sparse"]
        assert len(R.frames_touched(r.rows, sparse)[1]) < len(r.rows) // 2
        # the host form
        off, ln = R.u64([x[0] for x in sparse]), R.u64([x[1] for x in sparse])
        total = sum(x[1] for x in sparse)
        out = np.full(total + 64, CANARY, dtype=np.uint8)
        written, st = np.zeros(len(sparse), dtype=np.uint64), np.full(len(sparse), 0xDEAD, dtype=np.uint32)
        for h in (sk, skd):
            assert L.zsmi_seekableReadRangesHost(codec.ctx, h, R.ptr(off), R.ptr(ln), len(sparse), R.ptr(out), total, R.ptr(written), R.ptr(st)) == 0
            assert out[:total].tobytes() == b"".join(r.content[o:o + n] for o, n in sparse) and bool(np.all(out[total:] == CANARY))
            assert [int(w) for w in written] == [n for _, n in sparse] and not st.any()
    finally:
        codec.sync()
        L.zsmi_closeSeekable(sk); L.zsmi_closeSeekable(skd)
        dev.free()


def frames_of_choice(r, ch, lo=1, hi=1 << 30):
    return [i for i, c in enumerate(r.choice) if c == ch and lo <= r.rows[i][1] <= hi]


def test_missing_dictionaries(L, hip, codec, recs):
    from zstandard_amd import DecompressionDictSet
    r, d = recs, recs.d
    extent = lambda i: (d[i], d[i + 1] - d[i])
    free = frames_of_choice(r, NO_DICT) + frames_of_choice(r, EMPTY)
    # without a set: the frames that use no dictionary read as ever; a frame that names one: dictionary_wrong
    sk = R.open_host(L, codec.ctx, r.arc)[0]
    lacks = DecompressionDictSet(codec, [r.dds[0], r.dds[2]], unnamed=r.dds[3])               # no member for the zipf dictionary's ID
    unnamed_less = DecompressionDictSet(codec, r.dds[:3])
    r.sets += [lacks, unnamed_less]
    sk2, sk3 = open_host_set(L, codec, r.arc, lacks), open_host_set(L, codec, r.arc, unnamed_less)
    try:
        ranges = [extent(i) for i in free] + [(d[i] + 1, 1) for i in free if r.rows[i][1] > 2]
        check(R.read_ranges(L, hip, codec, sk, ranges, len(r.content)), r, ranges)
        named = frames_of_choice(r, 0)[:5]
        b = R.read_ranges(L, hip, codec, sk, [extent(i) for i in named], len(r.content))
        assert b.rc == 0 and b.status == [E_DICT_WRONG] * len(named)
        # a set that lacks one formatted member: its frames' ranges give dictionary_wrong, their neighbours' 0
        ranges, want = [], []
        for i in frames_of_choice(r, 1):
            if 0 < i < len(r.rows) - 1:
                ranges += [extent(i - 1), extent(i), (d[i] - 1, 2), extent(i + 1)]
                want += [0, E_DICT_WRONG, E_DICT_WRONG, 0]
        b = R.read_ranges(L, hip, codec, sk2, ranges, len(r.content))
        assert b.rc == 0 and b.status == want
        for k, (o, n) in enumerate(ranges):
            if want[k] == 0:
                assert b.out[k] == r.content[o:o + n], k
        # a set without `unnamed`: a raw-content frame decodes without its dictionary - its references point nowhere, or its bytes are others
        raw = frames_of_choice(r, RAW, 64, 4000)
        assert len(raw) > 10
        ranges = [extent(i) for i in raw] + [extent(i + 1) for i in raw if i + 1 < len(r.rows) and r.choice[i + 1] != RAW]
        b = R.read_ranges(L, hip, codec, sk3, ranges, len(r.content))
        assert b.rc == 0
        assert all(s in (E_CORRUPT, E_CHECKSUM) for s in b.status[:len(raw)]), b.status[:len(raw)]
        assert not any(b.status[len(raw):])
    finally:
        codec.sync()
        for h in (sk, sk2, sk3):
            L.zsmi_closeSeekable(h)


def read_frames(L, H, codec, sk, indices, rows, seed=1):
    """zsmi_seekableReadFramesDevice into one canary-guarded buffer, laid out as R.read_ranges lays its ranges out -> the same Batch"""
    n = len(indices)
    want = [rows[i][1] if i < len(rows) else 0 for i in indices]
    order = np.random.default_rng(seed).permutation(n)
    dst_off = np.zeros(max(n, 1), dtype=np.uint64)
    pos = PAD
    for k in order:
        dst_off[k] = pos
        pos += want[k] + PAD
    total = pos + 16
    dst, st = Dev(H, total), Dev(H, 4 * max(n, 1))
    idx = u32(indices or [0])
    written = np.full(max(n, 1), 0xDEAD, dtype=np.uint64)
    frames = ctypes.c_uint32(0xDEAD)
    b = R.Batch()
    try:
        b.rc = L.zsmi_seekableReadFramesDevice(codec.ctx, sk, R.ptr(idx), n, ctypes.c_void_p(dst.p), R.ptr(dst_off), R.ptr(written), ctypes.c_void_p(st.p),
                                               ctypes.byref(frames))
        codec.sync()
        buf = np.frombuffer(dst.all(), dtype=np.uint8)
        sbuf = st.all()
    finally:
        dst.free(); st.free()
    b.frames_decoded = frames.value
    b.written = [int(w) for w in written[:n]]
    b.status_raw = sbuf[PAD:PAD + 4 * n]
    assert sbuf[:PAD] == bytes([CANARY]) * PAD and sbuf[PAD + 4 * n:] == bytes([CANARY]) * (len(sbuf) - PAD - 4 * n), "wrote outside dStatus[nFrames]"
    outside = np.ones(len(buf), dtype=bool)
    if b.rc == 0:
        for k in range(n):
            outside[PAD + int(dst_off[k]):PAD + int(dst_off[k]) + want[k]] = False
    assert bool(np.all(buf[outside] == CANARY)), "a frame's read wrote outside its place"
    b.status = [int.from_bytes(b.status_raw[4 * k:4 * k + 4], "little") for k in range(n)]
    b.out = [buf[PAD + int(dst_off[k]):PAD + int(dst_off[k]) + want[k]].tobytes() for k in range(n)] if b.rc == 0 else None
    return b


def test_records_by_number(L, hip, codec, recs):
    r, d, n = recs, recs.d, len(recs.rows)
    sk = open_host_set(L, codec, r.arc, r.dset)
    try:
        rng = np.random.default_rng(9)
        idx = [int(i) for i in rng.permutation(n)[:60]] + [13, n - 1, 7, 7, 20, 0, n - 2, 20]     # shuffled, an empty frame, the last, duplicates
        ranges = [(d[i], d[i + 1] - d[i]) for i in idx]
        a = read_frames(L, hip, codec, sk, idx, r.rows, seed=4)
        b = R.read_ranges(L, hip, codec, sk, ranges, len(r.content), seed=4)
        assert a.rc == 0 and b.rc == 0
        assert a.out == b.out == [r.parts[i] for i in idx]
        assert a.written == b.written == [len(r.parts[i]) for i in idx]
        assert a.status == b.status == [0] * len(idx) and a.status_raw == b.status_raw
        assert a.frames_decoded == b.frames_decoded == len({i for i in idx if r.rows[i][1]})
        # an index that is no frame's: refused, nothing written (read_frames checks the canaries); nothing to do: nothing done
        bad = read_frames(L, hip, codec, sk, [3, n, 5], r.rows)
        assert bad.rc == E_FRAME_INDEX and bad.written == [0xDEAD] * 3 and bad.frames_decoded == 0xDEAD
        assert bad.status_raw == bytes([CANARY]) * 12
        none = read_frames(L, hip, codec, sk, [], r.rows)
        assert none.rc == 0 and none.frames_decoded == 0
        assert L.zsmi_seekableReadFramesDevice(codec.ctx, sk, None, 0, None, None, None, None, None) == 0
        # the host form against the ranges' host form
        ix, off, ln = u32(idx), R.u64([x[0] for x in ranges]), R.u64([x[1] for x in ranges])
        total = sum(x[1] for x in ranges)
        got = []
        for call, args in ((L.zsmi_seekableReadFramesHost, (R.ptr(ix),)), (L.zsmi_seekableReadRangesHost, (R.ptr(off), R.ptr(ln)))):
            out = np.full(total + 64, CANARY, dtype=np.uint8)
            written, st = np.zeros(len(idx), dtype=np.uint64), np.full(len(idx), 0xDEAD, dtype=np.uint32)
            assert call(codec.ctx, sk, *args, len(idx), R.ptr(out), total, R.ptr(written), R.ptr(st)) == 0
            got.append((out.tobytes(), written.tolist(), st.tolist()))
        assert got[0] == got[1] and got[0][0][:total] == b"".join(r.parts[i] for i in idx) and not any(got[0][2])
        out = np.full(64, CANARY, dtype=np.uint8)
        written, st = np.full(len(idx), 0xDEAD, dtype=np.uint64), np.full(len(idx), 0xDEAD, dtype=np.uint32)
        assert L.zsmi_seekableReadFramesHost(codec.ctx, sk, R.ptr(u32([1, n])), 2, R.ptr(out), 1 << 30, R.ptr(written), R.ptr(st)) == E_FRAME_INDEX
        assert L.zsmi_seekableReadFramesHost(codec.ctx, sk, R.ptr(ix), len(idx), R.ptr(out), total - 1, R.ptr(written), R.ptr(st)) == E_TOO_SMALL
        assert bool(np.all(out == CANARY)) and written.tolist() == [0xDEAD] * len(idx) and st.tolist() == [0xDEAD] * len(idx)
        # the handle's table against the archive's
        for i in list(range(n)) + [n, n + 1]:
            vals = [(ctypes.c_uint64(7), ctypes.c_uint64(7), ctypes.c_uint32(7), ctypes.c_uint32(7)) for _ in range(2)]
            refs = [[ctypes.byref(v) for v in vs] for vs in vals]
            rc = (L.zsmi_getFrameInfo_fromSeekable(sk, i, *refs[0]), L.zsmi_seekableFrameInfo(r.arc, len(r.arc), i, *refs[1]))
            assert rc[0] == rc[1] == (0 if i < n else E_FRAME_INDEX), i
            assert [v.value for v in vals[0]] == [v.value for v in vals[1]], i
            if i < n:
                assert (vals[0][1].value, vals[0][3].value) == (d[i], r.rows[i][1])
    finally:
        codec.sync()
        L.zsmi_closeSeekable(sk)


def test_damage_fails_exactly_the_ranges_that_touch_it(L, hip, codec, recs):
    r, d = recs, recs.d
    k = next(i for i in frames_of_choice(r, 0, 1500, 4000) if 2 <= i < len(r.rows) - 2)          # a frame of a formatted dictionary
    bad = G.damaged(r.arc, k, r.rows[k][0] // 2, 0x10)
    sk = open_host_set(L, codec, bad, r.dset)
    try:
        extent = lambda i: (d[i], d[i + 1] - d[i])
        ranges = [extent(k - 1), extent(k), (d[k] - 1, 2), (d[k + 1] - 1, 2), (d[k] + 5, 1), extent(k + 1), (0, d[k]), (d[k + 1], d[-1] - d[k + 1]), (0, d[-1])]
        touch = [False, True, True, True, True, False, False, False, True]
        b = R.read_ranges(L, hip, codec, sk, ranges, len(r.content))
        assert b.rc == 0
        for j, ((o, n), t) in enumerate(zip(ranges, touch)):
            if t:
                assert b.status[j] in (E_CORRUPT, E_CHECKSUM), (j, b.status[j])
            else:
                assert b.status[j] == 0 and b.out[j] == r.content[o:o + n], j
        f = read_frames(L, hip, codec, sk, [k - 1, k, k + 1], r.rows)
        assert f.rc == 0 and f.status[0] == 0 and f.status[2] == 0 and f.status[1] in (E_CORRUPT, E_CHECKSUM)
        assert f.out[0] == r.parts[k - 1] and f.out[2] == r.parts[k + 1]
    finally:
        codec.sync()
        L.zsmi_closeSeekable(sk)


# ------------------------------------------------------------------ 8. the Python surface
def test_python_surface(L, hip, codec, recs):
    from zstandard_amd import SeekableArchive, ZstdCompressor, CompressionDict, DecompressionDict
    r, n = recs, len(recs.rows)
    sizes = [len(p) for p in r.parts]
    assert codec.seekable_frames_bound(sizes, True) == frames_bound(L, sizes, 1) and codec.seekable_frames_bound([], False) == 17
    arc = codec.compress_seekable_frames_host(r.content, sizes, checksum=True, cdict_set=r.cset, dict_index=r.choice)
    assert arc == r.arc
    a = SeekableArchive(arc, ddict_set=r.dset)
    try:
        assert a.num_frames == n and a.content_size == len(r.content)
        idx = [5, 0, n - 1, 13, 5, 20, -2]
        assert a.read_frames(idx) == [r.parts[i] for i in idx]
        got, codes = a.read_frames([3, 4], return_codes=True)
        assert got == [r.parts[3], r.parts[4]] and codes == [0, 0]
        assert a.read_many([(0, len(r.content)), (r.d[7] - 3, 10)]) == [r.content, r.content[r.d[7] - 3:r.d[7] + 7]]
        assert a.frame_info(7) == (sum(row[0] for row in r.rows[:7]), r.d[7], r.rows[7][0], r.rows[7][1])
        with pytest.raises(RuntimeError):
            a.read_frames([n])
    finally:
        a.close()
    plain = SeekableArchive(arc)                                                   # no dictionaries: a frame that names one fails
    try:
        k = frames_of_choice(r, 0)[0]
        assert plain.read_frames([k], return_codes=True)[1] == [E_DICT_WRONG]
        with pytest.raises(RuntimeError):
            plain.read_frames([k])
    finally:
        plain.close()
    # one dictionary for every frame: cdict= on the way in, ddict= on the way out (the sets of one)
    data = X.class_data("json_records")
    parts = [data[o:o + 1500] for o in range(0, 45000, 1500)] + [b"", data[45000:45001]]
    fs = [len(p) for p in parts]
    cd, dd = CompressionDict(codec, X.trained("json_records"), 3), DecompressionDict(codec, X.trained("json_records"))
    try:
        one = codec.compress_seekable_frames_host(b"".join(parts), fs, cdict=cd)
        assert one == S.archive(B.compress_many(codec, parts, cdict=cd), parts, True)
        assert len(one) < len(codec.compress_seekable_frames_host(b"".join(parts), fs))            # (the dictionary pays on records)
        assert codec.compress_seekable_frames_host(b"".join(parts), fs, level=1, checksum=False) == oracle_archive(parts, 1, 0)
        bound = codec.seekable_frames_bound(fs)
        src, dst, size = Dev(hip, sum(fs), b"".join(parts)), Dev(hip, bound), Dev(hip, 8)
        out, st = Dev(hip, 4000), Dev(hip, 12)
        try:
            codec.compress_seekable_frames_device(src.p, fs, dst.p, bound, size.p, cdict=cd)
            codec.sync()
            m = int.from_bytes(size.all()[PAD:PAD + 8], "little")
            assert dst.all()[PAD:PAD + m] == one
            h = codec.open_seekable_device(dst.p, m, ddict=dd)
            assert h.num_frames == len(parts) and h.frame_info(2) == (sum(S.parse(one)[0][i][0] for i in range(2)), 3000, S.parse(one)[0][2][0], 1500)
            written, frames = h.read_frames_device([3, 30, 1], dst_offsets=[0, 1500, 1500], d_dst_ptr=out.p, d_status_ptr=st.p)
            codec.sync()
            assert written.tolist() == [1500, 0, 1500] and frames == 2
            assert out.all()[PAD:PAD + 3000] == parts[3] + parts[1] and st.all()[PAD:PAD + 12] == bytes(12)
            h.close()
            assert SeekableArchive(one, ddict=dd).read_frames([31, 0]) == [parts[31], parts[0]]
        finally:
            for b in (src, dst, size, out, st):
                b.free()
    finally:
        cd.close(); dd.close()
    # a raw-content dictionary the same way: a set of one that has no member a frame could name
    raw = X.STREAM[:6000]
    parts = [raw[100:1100], raw[2000:2500], b"", raw[3000:5000]]
    cd, dd = CompressionDict(codec, raw, 3), DecompressionDict(codec, raw)
    try:
        arc = codec.compress_seekable_frames_host(b"".join(parts), [len(p) for p in parts], cdict=cd)
        assert arc == S.archive(B.oracle_frames(parts, 3, raw), parts, True)
        assert SeekableArchive(arc, ddict=dd).read_frames([3, 0, 1, 2]) == [parts[3], parts[0], parts[1], parts[2]]
        assert all(c in (E_CORRUPT, E_CHECKSUM) for c in SeekableArchive(arc).read_frames([0, 1, 3], return_codes=True)[1])
        dev, out, st = Dev(hip, len(arc), arc), Dev(hip, 2000), Dev(hip, 4)
        try:
            h = codec.open_seekable_device(dev.p, len(arc), ddict=dd)
            assert h.read_frames_device([3], out.p, [0], st.p)[0].tolist() == [2000]
            codec.sync()
            assert out.all()[PAD:PAD + 2000] == parts[3] and st.all()[PAD:PAD + 4] == bytes(4)
            h.close()
        finally:
            for b in (dev, out, st):
                b.free()
    finally:
        cd.close(); dd.close()
    with pytest.raises(RuntimeError):                                              # compress_seekable keeps refusing a dictionary
        ZstdCompressor(3, dictionary=b"abc" * 100).compress_seekable(r.content[:100000])
