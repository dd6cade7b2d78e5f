"""Record archives (zsmi_compressSeekableFrames*, zsmi_openSeekable*_usingDDictSet, zsmi_seekableReadFrames*), the part that needs no GPU:
zsmi_seekableFramesBound against the Python sum over zsmi_compressBound, its three refusals in their order, the NULL context of every new
compress call, the check order of the open call that takes a DDict set, and the oracle's side of the byte-exact statement the GPU test
makes: oracle E's frames of the mixed batch of tests/_cdict_set.py and the table of tests/_seekable.py are an archive whose rows are the
chunks' sizes."""
import ctypes
import numpy as np
import pytest
import _cdict_set as CS
import _seekable as S
import _seekable_ranges as R
import test_seekable_table as T

E_GENERIC, E_OUT_OF_BOUND, E_INIT_MISSING, E_FRAME_INDEX = 1, 42, 62, 100
NEW = ["zsmi_seekableFramesBound", "zsmi_compressSeekableFramesDevice", "zsmi_compressSeekableFramesDevice_usingCDictSet",
       "zsmi_compressSeekableFramesHost", "zsmi_compressSeekableFramesHost_usingCDictSet", "zsmi_openSeekable_usingDDictSet",
       "zsmi_openSeekableDevice_usingDDictSet", "zsmi_getFrameInfo_fromSeekable", "zsmi_seekableReadFramesDevice", "zsmi_seekableReadFramesHost"]


@pytest.fixture(scope="module")
def L():
    from zstandard_amd import _lib
    _lib.build()
    return _lib.lib()


def code(L, r):
    return L.zsmi_getErrorCode(r) if L.zsmi_isError(r) else 0


def u32(a):
    return np.ascontiguousarray(a, dtype=np.uint32)


def test_new_names_are_exported(L):
    from zstandard_amd import _lib
    import zstandard_amd as Z
    for name in NEW:
        assert name in _lib.EXPORTS and hasattr(L, name), name
    for name in ("seekable_frames_bound", "compress_seekable_frames_device", "compress_seekable_frames_host", "open_seekable_device"):
        assert hasattr(Z.BatchCodec, name), name
    assert hasattr(Z.SeekableHandle, "read_frames_device") and hasattr(Z.SeekableHandle, "frame_info")
    assert hasattr(Z.SeekableArchive, "read_frames")


@pytest.mark.parametrize("flag", [0, 1])
def test_bound_is_the_sum_of_the_frames_bounds(L, flag):
    entry = 12 if flag else 8
    assert L.zsmi_seekableFramesBound(None, 0, flag) == 17
    sizes = u32([0, 1, 65536, 65537, 1 << 30])
    want = sum(L.zsmi_compressBound(int(s)) for s in sizes) + 17 + len(sizes) * entry
    assert L.zsmi_seekableFramesBound(R.ptr(sizes), len(sizes), flag) == want
    for k in range(1, len(sizes) + 1):                                          # every prefix, and the sizes one by one
        assert L.zsmi_seekableFramesBound(R.ptr(sizes), k, flag) == sum(L.zsmi_compressBound(int(s)) for s in sizes[:k]) + 17 + k * entry
        one = u32([sizes[k - 1]])
        assert L.zsmi_seekableFramesBound(R.ptr(one), 1, flag) == L.zsmi_compressBound(int(one[0])) + 17 + entry
    # fixed sizes F, F, .., rest: the bound of the fixed-size call
    for size, F in ((300000, 4095), (300000, 65536), (65536, 65536), (1, 50000)):
        fs = u32([min(F, size - o) for o in range(0, size, F)])
        assert L.zsmi_seekableFramesBound(R.ptr(fs), len(fs), flag) == L.zsmi_seekableBound(size, F, flag)


def test_bound_refusals_in_order(L):
    one = u32([5])
    assert code(L, L.zsmi_seekableFramesBound(R.ptr(one), 0x8000001, 1)) == E_FRAME_INDEX          # (the one-entry array is not read)
    assert code(L, L.zsmi_seekableFramesBound(None, 0x8000001, 1)) == E_FRAME_INDEX                # too many frames comes before the NULL array
    assert code(L, L.zsmi_seekableFramesBound(None, 1, 0)) == E_GENERIC
    big = u32([7, (1 << 30) + 1, 9])
    assert code(L, L.zsmi_seekableFramesBound(R.ptr(big), 3, 0)) == E_OUT_OF_BOUND
    assert code(L, L.zsmi_seekableFramesBound(R.ptr(big), 1, 0)) == 0                               # (only the entries below n count)
    assert code(L, L.zsmi_seekableFramesBound(R.ptr(u32([1 << 30])), 1, 0)) == 0


def test_null_context_comes_first(L):
    """every new compress call: init_missing in front of everything else that is wrong with the call; nothing is written"""
    sizes, bad = u32([4, 4]), u32([(1 << 30) + 1])
    out = ctypes.create_string_buffer(b"\xa5" * 64, 64)
    size = (ctypes.c_uint64 * 1)(0xDEAD)
    src = b"abcdefgh"
    for fs, n in ((sizes, 2), (bad, 1), (None, 1), (sizes, 0x8000001)):
        p = R.ptr(fs) if fs is not None else None
        assert L.zsmi_compressSeekableFramesDevice(None, None, p, n, None, 0, None, 3, 1) == E_INIT_MISSING
        assert L.zsmi_compressSeekableFramesDevice_usingCDictSet(None, None, p, n, None, 0, None, 1, None, None) == E_INIT_MISSING
        assert L.zsmi_compressSeekableFramesDevice(None, src, p, n, out, 64, size, 3, 1) == E_INIT_MISSING
        assert code(L, L.zsmi_compressSeekableFramesHost(None, out, 64, src, p, n, 3, 1)) == E_INIT_MISSING
        assert code(L, L.zsmi_compressSeekableFramesHost_usingCDictSet(None, out, 64, src, p, n, 1, None, None)) == E_INIT_MISSING
    assert out.raw == b"\xa5" * 64 and size[0] == 0xDEAD


def open_with_set(L, ctx, arc, dset=None):
    err = ctypes.c_int(-1)
    sk = L.zsmi_openSeekable_usingDDictSet(ctx, arc, len(arc) if arc is not None else 100, dset, ctypes.byref(err))
    return sk, err.value


def variable_archive():
    """a hand-built archive of frames of different sizes, an empty one among them (oracle E's frames, the table of tests/_seekable.py)"""
    import _data as D
    import _oracle as O
    data = D.zipf_log(90000).tobytes()
    parts = [data[:50], data[50:50], data[50:70000], data[70000:70001], data[70001:]]
    return S.archive([O.compress(p, 3) for p in parts], parts, True), parts


def test_open_with_a_set_judges_the_table_before_the_context(L):
    arc, parts = variable_archive()
    rows, ck = S.parse(arc)
    assert [r[1] for r in rows] == [len(p) for p in parts] and ck
    assert open_with_set(L, None, arc) == (None, E_INIT_MISSING)                # a valid table: only the context is missing
    assert open_with_set(L, None, arc) == R.open_host(L, None, arc)
    for what, bad in R.table_damages(arc).items():                               # a damaged table: its own code, as the call without a set
        want = T.code(L, L.zsmi_seekableNumFrames(bad, len(bad)))
        assert want != 0, what
        assert open_with_set(L, None, bad) == (None, want), what
        assert R.open_host(L, None, bad) == (None, want), what
    assert open_with_set(L, None, None) == (None, 10)
    assert L.zsmi_openSeekable_usingDDictSet(None, arc, len(arc), None, None) is None      # err may be NULL
    err = ctypes.c_int(-1)                                                        # the device form: the context first
    assert L.zsmi_openSeekableDevice_usingDDictSet(None, None, 100, None, ctypes.byref(err)) is None and err.value == E_INIT_MISSING


def test_null_handle_and_null_context_of_the_frame_calls(L):
    co, do = ctypes.c_uint64(7), ctypes.c_uint64(7)
    cs, ds = ctypes.c_uint32(7), ctypes.c_uint32(7)
    assert L.zsmi_getFrameInfo_fromSeekable(None, 0, ctypes.byref(co), ctypes.byref(do), ctypes.byref(cs), ctypes.byref(ds)) == E_GENERIC
    idx = u32([0])
    z, w = (ctypes.c_uint64 * 1)(0), (ctypes.c_uint64 * 1)(7)
    s, n = (ctypes.c_uint32 * 1)(7), ctypes.c_uint32(7)
    dst = ctypes.create_string_buffer(16)
    assert L.zsmi_seekableReadFramesDevice(None, None, R.ptr(idx), 1, None, z, w, None, ctypes.byref(n)) == E_INIT_MISSING
    assert L.zsmi_seekableReadFramesHost(None, None, R.ptr(idx), 1, dst, 16, w, s) == E_INIT_MISSING
    assert L.zsmi_seekableReadFramesDevice(None, None, None, 0, None, None, None, None, None) == E_INIT_MISSING
    assert (co.value, do.value, cs.value, ds.value, w[0], s[0], n.value) == (7,) * 7


@pytest.mark.parametrize("level", [1, 3])
def test_oracle_frames_of_the_mixed_batch_make_an_archive(level):
    """oracle E's frames of the mixed batch's chunks that use raw content, no dictionary or the empty member, with the table of
    tests/_seekable.py behind them: a variable-size archive whose rows are the chunks' sizes - what tests/test_gpu_seekable_frames.py
    compares the library's archive with, frame by frame"""
    items = CS.deal()
    frames = CS.oracle_frames(level)
    ks = sorted(frames)
    assert ks and all(CS.kind(items[k][1]) != "formatted" for k in ks)
    assert {CS.kind(items[k][1]) for k in ks} == {"none", "raw"}
    chunks = [items[k][0] for k in ks]
    assert len({len(c) for c in chunks}) > 10 and any(len(c) == 0 for c in chunks) and any(len(c) > 65536 for c in chunks)
    for flag in (False, True):
        arc = S.archive([frames[k] for k in ks], chunks, flag)
        rows, ck = S.parse(arc)
        assert ck == flag and len(rows) == len(ks)
        assert [r[1] for r in rows] == [len(c) for c in chunks]
        assert [r[0] for r in rows] == [len(frames[k]) for k in ks]
        if flag:
            assert [r[2] for r in rows] == [S.xxh32(c) for c in chunks]
