"""Record archives whose frame sizes, dictionary indices and frame numbers are device memory (zsmi_compressSeekableFramesResident
[_usingCDictSet], zsmi_seekableReadFramesResident): the archive byte for byte against the host-array call (plain and with a CDict set, both
table flags, the context's checksum flag, a tight and a loose maxFrameSize), one member without an index, sub-batches planned on the device,
the refusals only the device can make; reads against zsmi_seekableReadFramesDevice and the records themselves, the per-request refusals,
damage; one chain from sizes a torch op produced to the records read back; the host checks in their order; the Python surface.
Helpers: tests/_seekable_resident.py."""
import ctypes, os
import numpy as np
import pytest
import _batch as B, _resident_cdict_set as RS, _seekable as S, _seekable_resident as SR
import test_gpu_seekable as G, test_gpu_seekable_frames as F, test_seekable_table as T
from _hip import hip_of, Dev, CANARY, PAD
from _resident import up, down

pytestmark = pytest.mark.gpu
E_GENERIC, E_CORRUPT, E_CHECKSUM, E_OUT_OF_BOUND, E_INIT, E_TOO_SMALL, E_SRC_WRONG, E_FRAME_INDEX = 1, 20, 22, 42, 62, 70, 72, 100
NO_DICT = SR.NO_DICT
MIB = 1 << 20


def refusal(code):
    return (1 << 64) - code


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
def sets(codec):
    """level -> (CompressionDictSet, its CompressionDicts), made once"""
    made = {}

    def get(level):
        if level not in made:
            made[level] = RS.make_set(codec, level)
        return made[level]
    yield get
    codec.sync()
    for cset, cds in made.values():
        cset.close()
        for cd in set(cds):
            cd.close()


@pytest.fixture(scope="module")
def recs():
    return SR.records()


@pytest.fixture(scope="module")
def dict_archive(L, H, codec, sets, recs):
    """the host-array set call's archive of the records at level 3 with table checksums: what test 1 compares with, what the reads open"""
    parts, index = recs
    return F.compress_frames(L, H, codec, parts, 3, 1, sets(3)[0], index)


# ------------------------------------------------------------------ 1. byte for byte against the host-array call
@pytest.mark.parametrize("level", (1, 3))
@pytest.mark.parametrize("form", ("plain", "set"))
def test_archive_equals_the_host_array_call(L, H, codec, sets, recs, dict_archive, form, level):
    parts, index = recs
    sizes = [len(p) for p in parts]
    assert sizes[:9] == list(SR.EDGE_SIZES) and len(sizes) == 49 and sum(sizes) <= 2 * MIB
    cset = sets(level)[0] if form == "set" else None
    ix = index if form == "set" else None
    for flag in (0, 1):
        want = dict_archive if (form, level, flag) == ("set", 3, 1) else F.compress_frames(L, H, codec, parts, level, flag, cset, ix)
        for max_frame in (max(sizes), MIB):                                        # a loose bound changes no byte
            got = SR.write(L, H, codec, b"".join(parts), sizes, level, flag, cset, ix, max_frame=max_frame)
            assert got.rc == 0 and got.word == len(want), (form, level, flag, max_frame, got.rc, hex(got.word))
            assert got.archive == want, (form, level, flag, max_frame, B.first_difference(got.archive, want))
    if form == "set":                                                              # the frames name the members their records picked
        rows, _ = S.parse(want)
        ids = [cd.dict_id for cd in sets(level)[1]]
        at = 0
        for i, row in enumerate(rows):
            assert RS.frame_dict_id(want[at:at + row[0]]) == (0 if index[i] == NO_DICT else ids[index[i]]), i
            at += row[0]


def test_archive_with_the_contexts_checksum_flag(L, H, codec, sets, recs, dict_archive):
    parts, index = recs
    sizes = [len(p) for p in parts]
    codec.set_parameter("checksum", 1)
    try:
        want = F.compress_frames(L, H, codec, parts, 3, 1, sets(3)[0], index)
        got = SR.write(L, H, codec, b"".join(parts), sizes, 3, 1, sets(3)[0], index)
        plain = SR.write(L, H, codec, b"".join(parts), sizes, 3, 0)
        want_plain = F.compress_frames(L, H, codec, parts, 3, 0)
    finally:
        codec.set_parameter("checksum", 0)
    assert got.rc == 0 and got.archive == want and len(want) == len(dict_archive) + 4 * len(parts)
    assert plain.rc == 0 and plain.archive == want_plain


# ------------------------------------------------------------------ 2. one member without an index; nothing to write
def test_one_member_null_index_and_no_frames(L, H, codec, sets, recs):
    from zstandard_amd import CompressionDictSet
    parts = recs[0][9:30] + [b""] + recs[0][3:5]
    sizes = [len(p) for p in parts]
    cd = sets(3)[1][RS.KINDS["formatted"]]
    one = CompressionDictSet(codec, [cd], 3)
    try:
        want = F.compress_frames(L, H, codec, parts, 3, 1, one, None)               # the host-array call with that CDict: the set of one
        got = SR.write(L, H, codec, b"".join(parts), sizes, 3, 1, one, None)
        assert got.rc == 0 and got.archive == want
        again = SR.write(L, H, codec, b"".join(parts), sizes, 3, 1, one, [0] * len(parts))
        assert again.archive == want
        at = 0
        for row in S.parse(want)[0]:
            assert RS.frame_dict_id(want[at:at + row[0]]) == cd.dict_id != 0
            at += row[0]
        for flag in (0, 1):                                                        # n == 0: the 17-byte table, with and without a set
            for cset in (None, one, sets(3)[0]):
                none = SR.write(L, H, codec, b"", [], 3, flag, cset, None, use_set_call=cset is None and flag)
                assert none.rc == 0 and none.archive == S.table([], bool(flag)) and len(none.archive) == 17
        nul = SR.write(L, H, codec, b"".join(parts), sizes, 3, 1, None, None, use_set_call=True)      # set == NULL: the plain form at level 3
        assert nul.rc == 0 and nul.archive == F.compress_frames(L, H, codec, parts, 3, 1)
    finally:
        codec.sync(); one.close()


# ------------------------------------------------------------------ 3. sub-batches planned on the device
def test_sub_batches_planned_on_the_device():
    """ZSMI_BLOCKS_IN_FLIGHT=64 in a child process: 40 frames of 131073 bytes, three blocks each - two sub-batches"""
    B.run_child("-c", "import sys, os; sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], 'tests')); import _seekable_resident; _seekable_resident.child(40)",
                B.ROOT, env=dict(os.environ, ZSMI_BLOCKS_IN_FLIGHT="64"))


# ------------------------------------------------------------------ 4. what only the device can refuse
def test_device_refusals(L, H, codec, sets, recs):
    """each goes to *dArchiveSize as (uint64_t)-code; SR.write checks the canaries around the destination, the size word, the sizes, the
    indices and the source - which is exactly as long as srcSize says, so a kernel that followed the sizes past it would have read the
    canary behind it: the frames that are kept are checked against the content"""
    parts, _ = recs
    parts = parts[9:21]                                                            # twelve records of 1 .. 8 KiB
    sizes = [len(p) for p in parts]
    content = b"".join(parts)
    cset = sets(3)[0]
    index = [SR.PICKS[k % len(SR.PICKS)] for k in range(len(parts))]
    ok = SR.write(L, H, codec, content, sizes, 3, 1, cset, index)
    assert ok.rc == 0 and ok.archive == F.compress_frames(L, H, codec, parts, 3, 1, cset, index)
    # the sizes sum to more than srcSize: the last frame would end behind it
    for form in ((None, None), (cset, index)):
        w = SR.write(L, H, codec, content[:-1], sizes, 3, 1, *form)
        assert w.rc == 0 and w.word == refusal(E_SRC_WRONG), hex(w.word)
        more = sizes[:5] + [sizes[5] + 100000] + sizes[6:]                          # ... and every frame from the sixth on lies behind it
        w = SR.write(L, H, codec, content, more, 3, 0, *form)
        assert w.rc == 0 and w.word == refusal(E_SRC_WRONG), hex(w.word)
        # to fewer bytes than srcSize
        w = SR.write(L, H, codec, content, sizes[:-1], 3, 1, *(form[0], form[1][:-1] if form[1] else None))
        assert w.rc == 0 and w.word == refusal(E_SRC_WRONG), hex(w.word)
        w = SR.write(L, H, codec, content[:100], [], 3, 1, *(form[0], None), max_frame=0, src_size=0)
        assert w.rc == 0 and w.archive == S.table([], True)                        # (srcSize 0 and no frame: nothing is short)
        # one size above maxFrameSize
        w = SR.write(L, H, codec, content, sizes, 3, 1, *form, max_frame=max(sizes) - 1)
        assert w.rc == 0 and w.word == refusal(E_SRC_WRONG), hex(w.word)
    # one index out of range; the lowest failing frame's code
    for bad in (len(RS.SET), 0xFFFFFFFE):
        w = SR.write(L, H, codec, content, sizes, 3, 1, cset, index[:4] + [bad] + index[5:])
        assert w.rc == 0 and w.word == refusal(E_OUT_OF_BOUND), hex(w.word)
    longest = int(np.argmax(sizes))                                                # (the first of the longest frames)
    for at in (0, len(sizes) - 1):                                                 # a bad index in front of and behind a frame too long
        if at != longest:
            w = SR.write(L, H, codec, content, sizes, 3, 1, cset, index[:at] + [len(RS.SET)] + index[at + 1:], max_frame=max(sizes) - 1)
            assert w.rc == 0 and w.word == refusal(E_OUT_OF_BOUND if at < longest else E_SRC_WRONG), (at, longest, hex(w.word))
    w = SR.write(L, H, codec, content, sizes, 3, 1, cset, index[:longest] + [len(RS.SET)] + index[longest + 1:], max_frame=max(sizes) - 1)
    assert w.rc == 0 and w.word == refusal(E_SRC_WRONG), hex(w.word)               # both faults on one frame: the size's


# ------------------------------------------------------------------ 5. reading records by numbers in device memory
@pytest.fixture(scope="module")
def dset(codec):
    s, dds = SR.ddict_set(codec)
    yield s
    codec.sync(); s.close()
    for dd in dds:
        dd.close()


def requests(n, rows):
    rng = np.random.default_rng(3)
    idx = [int(i) for i in rng.permutation(n)[:30]] + [0, n - 1, 0, 7, 7, 8, 5, 7]
    assert rows[0][1] == 0 and idx.count(7) == 3 and rows[7][1] == 131073          # the empty frame, frame 0, the last, a number thrice
    return idx


@pytest.mark.parametrize("align", (1, 256))
@pytest.mark.parametrize("opened", ("host", "device"))
def test_read_equals_the_host_array_call_and_the_records(L, H, codec, recs, dict_archive, dset, opened, align):
    parts, _ = recs
    rows, _ = S.parse(dict_archive)
    n = len(rows)
    dev = Dev(H, len(dict_archive), dict_archive) if opened == "device" else None
    sk = F.open_host_set(L, codec, dict_archive, dset) if opened == "host" else F.open_device_set(L, codec, dev, len(dict_archive), dset)
    try:
        sized = L.zsmi_sizeofSeekable(sk)
        assert sized == (sum(r[0] for r in rows) if opened == "host" else 0)        # the archive's bytes alone, as before
        idx = requests(n, rows)
        want_off = SR.rounded_offsets([rows[i][1] for i in idx], align)
        ref = F.read_frames(L, H, codec, sk, idx, rows, seed=6)
        got = SR.read(L, H, codec, sk, idx, align, int(want_off[-1]))
        assert ref.rc == 0 and got.rc == 0
        assert (got.offsets == want_off).all()
        assert got.written.tolist() == ref.written == [len(parts[i]) for i in idx]
        assert got.status.tolist() == ref.status == [0] * len(idx)
        inside = np.zeros(len(got.buf), dtype=bool)
        for k, i in enumerate(idx):
            assert got.out(k, len(parts[i])) == ref.out[k] == parts[i], (k, i)
            inside[int(want_off[k]):int(want_off[k]) + len(parts[i])] = True
        assert (got.buf[~inside] == CANARY).all(), "written between the places"
        none = SR.read(L, H, codec, sk, [], align, 0)                              # nothing asked: dDstOffsets[0] = 0 and nothing else
        assert none.rc == 0 and none.offsets.tolist() == [0]
    finally:
        codec.sync()
        L.zsmi_closeSeekable(sk)
        if dev is not None:
            dev.free()


# ------------------------------------------------------------------ 6. per-request refusals, damage
def test_read_refusals_and_damage(L, H, codec, recs, dict_archive, dset):
    parts, _ = recs
    rows, _ = S.parse(dict_archive)
    n = len(rows)
    sk = F.open_host_set(L, codec, dict_archive, dset)
    try:
        # a number that names no frame: that request alone
        idx = [3, n, 5, 0xFFFFFFFF, 12]
        sizes = [rows[i][1] if i < n else 0 for i in idx]
        off = SR.rounded_offsets(sizes, 64)
        got = SR.read(L, H, codec, sk, idx, 64, int(off[-1]))
        assert got.rc == 0 and (got.offsets == off).all()
        assert got.status.tolist() == [0, E_FRAME_INDEX, 0, E_FRAME_INDEX, 0] and got.written.tolist() == sizes
        assert [got.out(k, sizes[k]) for k in (0, 2, 4)] == [parts[3], parts[5], parts[12]]
        # no room for the last two: 70 on those, nothing written for them, the others right (SR.read checks the canary behind the capacity)
        idx = [9, 6, 20, 4, 5, 6]
        sizes = [rows[i][1] for i in idx]
        off = SR.rounded_offsets(sizes, 1)
        cap = int(off[4]) + sizes[4] - 1
        got = SR.read(L, H, codec, sk, idx, 1, cap)
        assert got.rc == 0 and (got.offsets == off).all() and got.written.tolist() == sizes
        assert got.status.tolist() == [0, 0, 0, 0, E_TOO_SMALL, E_TOO_SMALL]
        assert [got.out(k, sizes[k]) for k in range(4)] == [parts[i] for i in idx[:4]]
        assert (got.buf[int(off[4]):] == CANARY).all()
        assert SR.read(L, H, codec, sk, idx, 1, 0).status.tolist() == [E_TOO_SMALL] * 6          # no room at all, a NULL-free call
    finally:
        codec.sync(); L.zsmi_closeSeekable(sk)
    # one flipped byte in frame k: exactly the requests that name it fail, with the host-array call's code
    k = 7
    bad = G.damaged(dict_archive, k, rows[k][0] // 2, 0x10)
    # a table checksum that is not the content's
    j = 11
    lied = T.rebuilt(dict_archive, rows=rows[:j] + [(rows[j][0], rows[j][1], rows[j][2] ^ 0x100)] + rows[j + 1:])
    for arc, at, codes in ((bad, k, (E_CORRUPT, E_CHECKSUM)), (lied, j, (E_CHECKSUM,))):
        sk = F.open_host_set(L, codec, arc, dset)
        try:
            idx = [at - 1, at, at + 1, 20, at]
            sizes = [rows[i][1] for i in idx]
            off = SR.rounded_offsets(sizes, 16)
            ref = F.read_frames(L, H, codec, sk, idx, rows)
            got = SR.read(L, H, codec, sk, idx, 16, int(off[-1]))
            assert got.rc == 0 and ref.rc == 0
            assert got.status.tolist() == ref.status and ref.status[1] in codes, (ref.status, got.status.tolist())
            assert [s != 0 for s in got.status.tolist()] == [False, True, False, False, True]
            assert [got.out(m, sizes[m]) for m in (0, 2, 3)] == [parts[idx[m]] for m in (0, 2, 3)]
        finally:
            codec.sync(); L.zsmi_closeSeekable(sk)


# ------------------------------------------------------------------ 7. one chain
def test_chain_from_device_made_sizes_to_records():
    """a process of its own, because torch must be the first to load the HIP runtime: see _seekable_resident.chain_child"""
    B.run_child("-c", "import torch, sys, os; sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], 'tests')); import _seekable_resident; _seekable_resident.chain_child()",
                B.ROOT)


# ------------------------------------------------------------------ 8. the host checks, in their order
def test_host_checks_in_order(L, H, codec, sets, recs, dict_archive, dset):
    cset = sets(3)[0]
    buf = Dev(H, 4096)
    b = ctypes.c_void_p(buf.p)
    ctx = codec.ctx
    plain, using = L.zsmi_compressSeekableFramesResident, L.zsmi_compressSeekableFramesResident_usingCDictSet
    big = L.zsmi_seekableFramesResidentBound(1000, 3, 1)
    try:
        # write: ctx, n, dFrameSizes, maxFrameSize, the index rule, (the set's device: needs a second GPU), the capacity, the NULLs
        assert plain(None, None, 1000, None, 0x8000001, (1 << 30) + 1, None, 0, None, 3, 1) == E_INIT
        assert plain(ctx, None, 1000, None, 0x8000001, (1 << 30) + 1, None, 0, None, 3, 1) == E_FRAME_INDEX
        assert plain(ctx, None, 1000, None, 3, (1 << 30) + 1, None, 0, None, 3, 1) == E_GENERIC
        assert plain(ctx, None, 1000, b, 3, (1 << 30) + 1, None, 0, None, 3, 1) == E_OUT_OF_BOUND
        assert using(ctx, None, 1000, b, 3, (1 << 30) + 1, None, 0, None, 1, cset.handle, None) == E_OUT_OF_BOUND
        assert using(ctx, None, 1000, b, 3, 1000, None, 0, None, 1, cset.handle, None) == E_GENERIC          # a NULL index and seven members
        assert using(ctx, None, 1000, b, 3, 1000, None, 0, None, 1, cset.handle, b) == E_TOO_SMALL
        assert using(ctx, None, 1000, None, 0, 1000, None, 1 << 40, None, 1, cset.handle, None) == E_OUT_OF_BOUND   # content and no frame: the bound's refusal
        assert plain(ctx, None, 1000, b, 3, 1000, None, big - 1, None, 3, 1) == E_TOO_SMALL
        assert plain(ctx, None, 1000, b, 3, 1000, b, big, b, 3, 1) == E_GENERIC                                # a NULL dSrc with content
        assert plain(ctx, b, 1000, b, 3, 1000, None, big, b, 3, 1) == E_GENERIC and plain(ctx, b, 1000, b, 3, 1000, b, big, None, 3, 1) == E_GENERIC
        # read: ctx, sk and the arrays, (the handle's device), align, dDst
        read = L.zsmi_seekableReadFramesResident
        sk = F.open_host_set(L, codec, dict_archive, dset)
        try:
            assert read(None, None, None, 2, 3, None, 10, None, None, None) == E_INIT
            assert read(ctx, None, b, 2, 3, None, 10, b, b, b) == E_GENERIC
            for at in range(4):
                arrays = [b, b, b, b]
                arrays[at] = None
                assert read(ctx, sk, arrays[0], 2, 3, None, 10, arrays[1], arrays[2], arrays[3]) == E_GENERIC, at
            for align in (0, 3, 8192):
                assert read(ctx, sk, b, 2, align, None, 10, b, b, b) == E_OUT_OF_BOUND, align
            assert read(ctx, sk, b, 2, 64, None, 10, b, b, b) == E_GENERIC
        finally:
            codec.sync(); L.zsmi_closeSeekable(sk)
        codec.sync()
        raw = np.frombuffer(buf.all(), dtype=np.uint8)
        assert (raw == CANARY).all(), "a refused call wrote"
    finally:
        buf.free()


# ------------------------------------------------------------------ 9. the Python surface
def test_python_surface(L, H, codec, sets, recs, dict_archive, dset):
    parts, index = recs
    sizes = SR.u32([len(p) for p in parts])
    content = b"".join(parts)
    n = len(parts)
    assert codec.seekable_frames_resident_bound(len(content), n, True) == L.zsmi_seekableFramesResidentBound(len(content), n, 1)
    assert codec.seekable_frames_resident_bound(0, 0, False) == 17
    with pytest.raises(RuntimeError):
        codec.seekable_frames_resident_bound(1, 0)
    bound = codec.seekable_frames_resident_bound(len(content), n)
    src, d_fs, d_ix, dst, size = up(H, np.frombuffer(content, dtype=np.uint8)), up(H, sizes), up(H, index), Dev(H, bound), Dev(H, 8)
    try:
        codec.compress_seekable_frames_resident(src.p, len(content), d_fs.p, n, int(sizes.max()), dst.p, bound, size.p, cdict_set=sets(3)[0], d_dict_index_ptr=d_ix.p)
        codec.sync()
        m = int(down(size, np.uint64)[0][0])
        assert down(dst)[0][:m].tobytes() == dict_archive
        with pytest.raises(ValueError):
            codec.compress_seekable_frames_resident(src.p, len(content), d_fs.p, n, 1, dst.p, bound, size.p, d_dict_index_ptr=d_ix.p)
        with pytest.raises(ValueError):
            codec.compress_seekable_frames_resident(src.p, len(content), d_fs.p, n, 1, dst.p, bound, size.p, cdict=sets(3)[1][0], cdict_set=sets(3)[0])
        with pytest.raises(RuntimeError):
            codec.compress_seekable_frames_resident(src.p, len(content), d_fs.p, n, 1, dst.p, bound - 1, size.p)
        cd = sets(3)[1][0]
        codec.compress_seekable_frames_resident(src.p, len(content), d_fs.p, n, int(sizes.max()), dst.p, bound, size.p, cdict=cd)
        codec.sync()
        m1 = int(down(size, np.uint64)[0][0])
        assert down(dst)[0][:m1].tobytes() == codec.compress_seekable_frames_host(content, sizes, cdict=cd)
        codec.compress_seekable_frames_resident(src.p, len(content), d_fs.p, n, int(sizes.max()), dst.p, bound, size.p, level=1, checksum=False)
        codec.sync()
        m2 = int(down(size, np.uint64)[0][0])
        assert down(dst)[0][:m2].tobytes() == codec.compress_seekable_frames_host(content, sizes, level=1, checksum=False)
        # read through a SeekableHandle
        arc = up(H, np.frombuffer(dict_archive, dtype=np.uint8))
        h = codec.open_seekable_device(arc.p, len(dict_archive), ddict_set=dset)
        idx = SR.u32([4, 1, 4, 48])
        want = SR.rounded_offsets([len(parts[i]) for i in idx], 32)
        d_req, out, off, wr, st = up(H, idx), Dev(H, int(want[-1])), Dev(H, 8 * 5), Dev(H, 16), Dev(H, 16)
        try:
            h.read_frames_resident(d_req.p, 4, out.p, int(want[-1]), off.p, wr.p, st.p, align=32)
            codec.sync()
            assert (down(off, np.uint64)[0] == want).all() and down(wr, np.uint32)[0].tolist() == [len(parts[i]) for i in idx] and not down(st, np.uint32)[0].any()
            host = down(out)[0]
            for q, i in enumerate(idx):
                assert host[int(want[q]):int(want[q]) + len(parts[i])].tobytes() == parts[i]
            with pytest.raises(RuntimeError):
                h.read_frames_resident(d_req.p, 4, out.p, int(want[-1]), off.p, wr.p, st.p, align=3)
        finally:
            codec.sync(); h.close()
            for d in (arc, d_req, out, off, wr, st):
                d.free()
    finally:
        for d in (src, d_fs, d_ix, dst, size):
            d.free()
