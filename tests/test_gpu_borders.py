"""Plans, launch loops and the index kernels across their tile and limit borders (the inputs: tests/_borders.py, held against the source's
constants and checked on the host by tests/test_borders_host.py).
A. k_plan_chunks over more than one tile of 1024 chunks, k_plan_blocks over more than 1024 chunks: the resident compress calls against the
   host-array calls and oracle E - tiny chunks, uneven counts across tile and sub-batch borders, the set form, a record archive of 3000.
B. the scan's second level is in tests/test_gpu_frame_sizes.py (test_layout_equals_numpy_at_the_scans_second_level).
C. the default limits: the compress cut at 16 384 blocks against oracle E, 66 000 items in one decode call against oracle D (host arrays,
   resident, with a digested dictionary), 66 000 record numbers in one read.
D. frames whose magic numbers lie across every lane, step and tile border of k_index_count / k_index_emit, at every kind of stream end."""
import ctypes, os
import numpy as np
import pytest
import _batch as B, _borders as BD, _oracle as O, _resident_compress as RC, _resident_cdict_set as RS, _seekable_resident as SR
import _resident as R
import test_gpu_frames_index as GI, test_gpu_seekable_frames as GF
from _hip import hip_of, Dev, CANARY, PAD

pytestmark = pytest.mark.gpu
KIB = 1 << 10
E_FRAME_INDEX = 100
_CHILD = "import sys, os; sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], 'tests')); import _borders; _borders.plan_child(sys.argv[2])"


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
def set3(codec):
    cset, cds = BD.make_set3(codec)
    yield cset
    codec.sync(); cset.close()
    for cd in cds:
        cd.close()


@pytest.fixture(scope="module")
def dset3(codec):
    """the DDict set that reads what the set of three wrote: the formatted member by its ID, the raw content as the unnamed member"""
    from zstandard_amd import DecompressionDict, DecompressionDictSet
    dds = [DecompressionDict(codec, BD.SET3[0]), DecompressionDict(codec, BD.SET3[1])]
    s = DecompressionDictSet(codec, dds[:1], unnamed=dds[1])
    yield s
    codec.sync(); s.close()
    for dd in dds:
        dd.close()


# ------------------------------------------------------------------ A.1 one sub-batch of tiny chunks: K = n, one block a chunk
@pytest.mark.parametrize("n", BD.TINY_N)
def test_plan_of_tiny_chunks_over_tiles(codec, H, n):
    chunks = BD.tiny_chunks(n)
    batch = RC.Batch(codec, H, chunks)
    try:
        ref = batch.run(False)
        assert (ref[0] < B.ERR).all()
        got = batch.run(True, 64 * KIB)
        RC.assert_equal_to_host_call(batch, ref, got, 64 * KIB, f"{n} tiny chunks")
        for i, (f, e) in enumerate(zip(batch.frames(*got), B.oracle_frames(chunks, 3))):
            assert f == e, ("oracle E", n, i, len(chunks[i]))
        told = batch.run(True, BD.TOLD)                                              # the chunks above 300 bytes refused in place
        RC.assert_equal_to_host_call(batch, ref, told, BD.TOLD, f"{n} tiny chunks, maxSrcSize {BD.TOLD}")
        assert int((told[0] == RC.REFUSED).sum()) == int((batch.ss > BD.TOLD).sum()) > 0
    finally:
        batch.free()


# ------------------------------------------------------------------ A.3 the same through the set of three (k_plan_chunks<true>: four sums)
@pytest.mark.parametrize("n", BD.TINY_N)
def test_plan_of_tiny_chunks_over_tiles_with_a_set(codec, H, set3, n):
    batch = RS.Batch(codec, H, BD.with_choices(BD.tiny_chunks(n)))
    try:
        BD.assert_set_call(batch, set3, 64 * KIB, f"{n} tiny chunks, a set")
        BD.assert_set_call(batch, set3, BD.TOLD, f"{n} tiny chunks, a set, maxSrcSize {BD.TOLD}")
    finally:
        batch.free()


# ------------------------------------------------------------------ A.2, A.3 uneven counts across tile and sub-batch borders
@pytest.mark.parametrize("form", ("plain", "set"))
def test_plan_of_uneven_chunks_over_tiles_and_sub_batches(form):
    """ZSMI_BLOCKS_IN_FLIGHT=4400 in a child process, maxSrcSize 200 KiB: sub-batches of 1100 chunks - a tile of 1024 and one of 76 - with
    chunks of two to four blocks on both sides of every border: _borders.plan_child"""
    B.run_child("-c", _CHILD, B.ROOT, form, env=dict(os.environ, ZSMI_BLOCKS_IN_FLIGHT=str(BD.UNEVEN_IN_FLIGHT)))


# ------------------------------------------------------------------ A.4 a resident record archive of 3000 records, C.4 66 000 numbers read
class Archive:
    pass


@pytest.fixture(scope="module")
def archive(L, H, codec, set3, dset3):
    """the host-array set call's archive of the 3000 records in device memory, opened with the DDict set"""
    a = Archive()
    a.parts, a.index = BD.records()
    a.bytes = GF.compress_frames(L, H, codec, a.parts, 3, 1, set3, a.index)
    a.dev = Dev(H, len(a.bytes), a.bytes)
    a.sk = GF.open_device_set(L, codec, a.dev, len(a.bytes), dset3)
    yield a
    codec.sync()
    L.zsmi_closeSeekable(a.sk)
    a.dev.free()


@pytest.mark.parametrize("form", ("plain", "set"))
def test_resident_archive_of_3000_records(L, H, codec, set3, archive, form):
    parts = archive.parts
    sizes = [len(p) for p in parts]
    want = archive.bytes if form == "set" else GF.compress_frames(L, H, codec, parts, 3, 1)
    got = SR.write(L, H, codec, b"".join(parts), sizes, 3, 1, set3 if form == "set" else None, archive.index if form == "set" else None)
    assert got.rc == 0 and got.word == len(want), (got.rc, hex(got.word), len(want))
    assert got.archive == want, B.first_difference(got.archive, want)


def assert_records_read(L, H, codec, archive, idx, align):
    parts, n = archive.parts, len(archive.parts)
    sizes = [len(parts[i]) if i < n else 0 for i in idx]
    off = SR.rounded_offsets(sizes, align)
    got = SR.read(L, H, codec, archive.sk, idx, align, int(off[-1]))
    assert got.rc == 0 and (got.offsets == off).all()
    assert got.written.tolist() == sizes
    assert got.status.tolist() == [0 if i < n else E_FRAME_INDEX for i in idx]
    inside = np.zeros(len(got.buf), dtype=bool)
    for k, i in enumerate(idx):
        if i < n:
            assert got.out(k, sizes[k]) == parts[i], (k, i)
            inside[int(off[k]):int(off[k]) + sizes[k]] = True
    assert (got.buf[~inside] == CANARY).all(), "written between the places"


def test_all_3000_records_read_by_number(L, H, codec, archive):
    assert_records_read(L, H, codec, archive, [int(i) for i in np.random.default_rng(30).permutation(len(archive.parts))], 16)


def test_read_of_66000_record_numbers(L, H, codec, archive):
    """more than 65 536 requests in one call; repeats, and numbers at and above the frame count - on both sides of the second launch too"""
    n = len(archive.parts)
    rng = np.random.default_rng(66)
    idx = [int(i) for i in rng.integers(0, n, BD.DECODE_N)]
    for at, i in ((0, n), (7, 0xFFFFFFFF), (BD.ITEMS_IN_FLIGHT - 1, n - 1), (BD.ITEMS_IN_FLIGHT, n), (BD.ITEMS_IN_FLIGHT + 1, 0), (BD.DECODE_N - 1, n + 5)):
        idx[at] = i
    for at in rng.integers(0, BD.DECODE_N, 40):
        idx[int(at)] = n + int(at) % 3
    assert len(set(idx)) < len(idx)
    assert_records_read(L, H, codec, archive, idx, 1)


# ------------------------------------------------------------------ C.1 the compress cut at the default blocks in flight
def test_compress_cut_at_the_default_blocks_in_flight(codec):
    """16 500 chunks in one host-array call, no environment variable: the chunk of three blocks at index 16 383 does not fit the first
    sub-batch of 16 384 blocks, which is cut in front of it.  Every frame is oracle E's"""
    chunks = BD.cut_chunks()
    frames = B.compress_many(codec, chunks, 3)
    for i, (f, e) in enumerate(zip(frames, B.oracle_frames(chunks, 3))):
        assert f == e, ("oracle E", i, len(chunks[i]), B.first_difference(f, e))
    some = sorted(set(range(BD.CUT_AT - 20, BD.CUT_AT + 21)) | {0, len(chunks) - 1} | {int(i) for i in np.random.default_rng(5).integers(0, len(chunks), 160)})
    assert len(some) >= 200
    for i in some:
        assert O.decompress(frames[i], len(chunks[i])) == chunks[i], ("oracle D", i)


# ------------------------------------------------------------------ C.2, C.3 the second decode launch at the default items in flight
def assert_items_equal_oracle_d(got, want, what):
    assert len(got) == len(want)
    bad = [i for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad, (what, len(bad), [(i, hex(got[i][0]), hex(want[i][0])) for i in bad[:6]])


def test_decode_66000_frames_in_one_call(codec):
    items, contents, want = BD.decode_items()
    BD.assert_decode_condition(items, contents, want)
    got = B.decode_many(codec, items, [len(c) for c in contents], min_cap=0)
    assert_items_equal_oracle_d(got, want, "zsmi_decompressBatchHost")


def resident_decode(codec, H, items, caps, max_cap, ddict_set=None):
    """zsmi_decompressBatchResident over items laid back to back into places of their capacities with gaps: [(size word, bytes)]; nothing
    outside the places, nor around any buffer, may be written"""
    n = len(items)
    src_np, so, ss = B.batch(items)
    caps = np.asarray(caps, dtype=np.uint32)
    do = B.layout(caps, 1 + np.arange(n) % 5)
    total = int(do[-1]) + int(caps[-1]) + 64
    bufs = [R.up(H, a) for a in (src_np, so, ss, do, caps)]
    dst, dsz = Dev(H, total), Dev(H, 4 * n)
    try:
        codec.decompress_resident(bufs[0].p, bufs[1].p, bufs[2].p, n, dst.p, bufs[3].p, bufs[4].p, max_cap, dsz.p, ddict_set=ddict_set)
        codec.sync()
        host, ok1 = R.down(dst)
        sz, ok2 = R.down(dsz, np.uint32)
        assert ok1 and ok2 and all(R.down(b)[1] for b in bufs), "a canary around a buffer is gone"
        inside = np.zeros(total, dtype=bool)
        for o, c in zip(do.tolist(), caps.tolist()):
            inside[o:o + c] = True
        assert (host[~inside] == CANARY).all(), "written outside the items' places"
        return [(s, host[o:o + (s if s < B.ERR else 0)].tobytes()) for o, s in zip(do.tolist(), sz.tolist())]
    finally:
        for d in bufs + [dst, dsz]:
            d.free()


def test_resident_decode_of_66000_frames(codec, H):
    items, contents, want = BD.decode_items()
    got = resident_decode(codec, H, items, [len(c) for c in contents], 120)
    assert_items_equal_oracle_d(got, want, "zsmi_decompressBatchResident")


def test_resident_decode_of_66000_dictionary_frames(codec, H):
    """the same count as frames of a formatted dictionary through its DecompressionDict: the dictionary form of the fast kernels in the
    second launch too.  Against oracle D with the dictionary"""
    from zstandard_amd import DecompressionDict, DecompressionDictSet
    dic = BD.SET3[0]
    items, contents, want = BD.decode_items(dic)
    BD.assert_decode_condition(items, contents, want)
    dd = DecompressionDict(codec, dic)
    one = DecompressionDictSet(codec, [dd])
    try:
        assert all(RS.frame_dict_id(items[i]) == dd.dict_id != 0 for i in (1, BD.ITEMS_IN_FLIGHT, BD.DECODE_N - 1))
        got = resident_decode(codec, H, items, [len(c) for c in contents], 120, one)
        assert_items_equal_oracle_d(got, want, "zsmi_decompressBatchResident, a DDict")
    finally:
        codec.sync(); one.close(); dd.close()


# ------------------------------------------------------------------ D. magic numbers on every border of the index kernels
@pytest.mark.parametrize("name", sorted(BD.STREAMS))
def test_index_of_frames_on_every_border(L, H, codec, name):
    stream, entries, contents = BD.index_stream(name)
    real = [k for k, (p, _, _) in enumerate(entries) if p in contents]
    rows = GI.rows_for_reads(entries)
    junk = lambda m: (m.to_bytes(4, "little") + bytes(range(60)))
    front, behind = junk(BD.SKIP_MAGIC + 2), b"\xfd" + junk(BD.ZSTD_MAGIC)      # (0xFD behind the end: the last byte of a magic number cut off there)
    for shift in (0, 1, 15):
        image = bytes(shift) + front + stream + behind
        dev = Dev(H, len(image), image)
        skd, e = GI.open_device(L, codec, dev.p + shift + len(front), len(stream))
        try:
            assert skd and e == 0, (name, shift, e)
            got = GI.table_of(L, skd)
            assert got == entries, (name, shift, len(got), len(entries), next((a, b) for a, b in zip(got + [None], entries + [None]) if a != b))
            f = GF.read_frames(L, H, codec, skd, real, rows, seed=shift)
            assert f.rc == 0 and not any(f.status) and f.out == [contents[entries[k][0]] for k in real]
            raw = np.frombuffer(dev.all(), dtype=np.uint8)
            assert (raw[:PAD] == CANARY).all() and (raw[PAD + len(image):] == CANARY).all() and raw[PAD:PAD + len(image)].tobytes() == image
        finally:
            codec.sync()
            if skd:
                L.zsmi_closeSeekable(skd)
            dev.free()
