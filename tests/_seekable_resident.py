"""Record archives with device-resident sizes, dictionary indices and frame numbers in the GPU tests (test infrastructure): one call of
zsmi_compressSeekableFramesResident[_usingCDictSet] and one of zsmi_seekableReadFramesResident with every buffer canary-guarded, the
records and choices tests/test_gpu_seekable_resident.py writes, and the child processes of its sub-batch test and of its chain.  The host-array calls they are
held against are those of tests/test_gpu_seekable_frames.py (compress_frames, read_frames)."""
import ctypes
import numpy as np
import _resident_cdict_set as RS, _resident_compress as RC
from _hip import Dev, CANARY, PAD
from _resident import up, down

NO_DICT = RS.NO_DICT
EDGE_SIZES = (0, 1, 255, 4096, 65535, 65536, 65537, 131073, 200000)
# the members a frame can be read back with through ONE DDict set: the formatted ones by their IDs, one raw-content dictionary as the
# set's unnamed member, and the choices without a dictionary
FORMATTED = ("trained8k", "id_0xffffffff", "trained64k_json_records")
PICKS = tuple(RS.SET.index(name) for name in FORMATTED + ("raw6000", "empty", "again")) + (NO_DICT,)


def u32(a):
    return np.ascontiguousarray(a, dtype=np.uint32)


def records(seed=41, extra=40):
    """(parts, choices): the edge sizes and `extra` seeded sizes of 1 .. 8 KiB cut from the stream, the choices dealt over PICKS"""
    rng = np.random.default_rng(seed)
    data = RC.stream_bytes()
    sizes = list(EDGE_SIZES) + [int(v) for v in rng.integers(1, 8193, extra)]
    parts = [data[at:at + s] for at, s in ((int(rng.integers(0, len(data) - s)), s) for s in sizes)]
    return parts, u32([PICKS[k % len(PICKS)] for k in range(len(parts))])


def ddict_set(codec):
    """(DecompressionDictSet that reads what PICKS wrote, its DecompressionDicts)"""
    from zstandard_amd import DecompressionDict, DecompressionDictSet
    dics = RS.dictionaries()
    dds = [DecompressionDict(codec, dics[RS.SET.index(name)]) for name in FORMATTED + ("raw6000",)]
    return DecompressionDictSet(codec, dds[:3], unnamed=dds[3]), dds


class Written:
    """what one resident compress call left: rc, word (*dArchiveSize), archive (its bytes when word is a size)"""


def write(L, H, codec, content, sizes, level=3, flag=1, cset=None, index=None, max_frame=None, src_size=None, use_set_call=None):
    """the call with its sizes (and index, unless None) in device memory.  The source is exactly len(content) bytes with canaries the test
    owns on both sides; the destination is exactly the resident bound; every buffer's canaries are checked, and nothing behind the
    archive's end may be written."""
    sizes = u32(sizes)
    n = len(sizes)
    src_size = len(content) if src_size is None else src_size
    max_frame = (int(sizes.max()) if n else 0) if max_frame is None else max_frame
    bound = L.zsmi_seekableFramesResidentBound(src_size, n, flag)
    assert not L.zsmi_isError(bound)
    src, dst, sz = Dev(H, max(len(content), 1), content), Dev(H, bound), Dev(H, 8)
    d_fs = up(H, sizes)
    d_ix = up(H, u32(index)) if index is not None else None
    p = ctypes.c_void_p
    w = Written()
    try:
        if cset is None and not use_set_call:
            w.rc = L.zsmi_compressSeekableFramesResident(codec.ctx, p(src.p), src_size, p(d_fs.p) if n else None, n, max_frame, p(dst.p), bound, p(sz.p), level, flag)
        else:
            w.rc = L.zsmi_compressSeekableFramesResident_usingCDictSet(codec.ctx, p(src.p), src_size, p(d_fs.p) if n else None, n, max_frame, p(dst.p), bound, p(sz.p),
                                                                       flag, cset.handle if cset is not None else None, p(d_ix.p) if d_ix is not None else None)
        codec.sync()
        word, ok = down(sz, np.uint64)
        assert ok, "wrote outside *dArchiveSize"
        w.word = int(word[0])
        for name, d in (("the source", src), ("the sizes", d_fs), ("the indices", d_ix)):
            if d is not None:
                raw = np.frombuffer(d.all(), dtype=np.uint8)
                assert (raw[:PAD] == CANARY).all() and (raw[PAD + d.n:] == CANARY).all(), name
        buf, ok = down(dst)
        assert ok, "wrote outside [dDst, dDst + dstCapacity)"
        w.archive = None
        if w.rc == 0 and w.word <= bound:
            assert (buf[w.word:] == CANARY).all(), "wrote behind the archive's end"
            w.archive = buf[:w.word].tobytes()
        return w
    finally:
        for d in (src, dst, sz, d_fs, d_ix):
            if d is not None:
                d.free()


def rounded_offsets(sizes, align):
    """dDstOffsets as the call must lay them out: the exclusive running sum of the sizes, each rounded up to align; n + 1 entries"""
    r = (np.asarray(sizes, dtype=np.uint64) + np.uint64(align - 1)) // np.uint64(align) * np.uint64(align)
    return np.concatenate([[0], np.cumsum(r, dtype=np.uint64)]).astype(np.uint64)


class Read:
    """what one resident read left: rc, offsets (n + 1), written, status, buf (the destination, capacity bytes)"""

    def out(self, k, size):
        return self.buf[int(self.offsets[k]):int(self.offsets[k]) + size].tobytes()


def read(L, H, codec, sk, indices, align, capacity, d_idx=None):
    """zsmi_seekableReadFramesResident with its numbers in device memory (d_idx: a device pointer somebody else filled) into a destination
    of exactly `capacity` bytes; the canaries around every buffer are checked"""
    n = len(indices)
    own = up(H, u32(indices if n else [0])) if d_idx is None else None
    dst, off, wr, st = Dev(H, max(capacity, 1)), Dev(H, 8 * (n + 1)), Dev(H, 4 * max(n, 1)), Dev(H, 4 * max(n, 1))
    p = ctypes.c_void_p
    r = Read()
    try:
        r.rc = L.zsmi_seekableReadFramesResident(codec.ctx, sk, p(own.p if own is not None else d_idx), n, align, p(dst.p), capacity, p(off.p), p(wr.p), p(st.p))
        codec.sync()
        raw = np.frombuffer(dst.all(), dtype=np.uint8)
        assert (raw[:PAD] == CANARY).all() and (raw[PAD + capacity:] == CANARY).all(), "wrote outside [dDst, dDst + dstCapacity)"
        r.buf = raw[PAD:PAD + capacity].copy()
        vals = []
        for name, d, t in (("dDstOffsets", off, np.uint64), ("dWritten", wr, np.uint32), ("dStatus", st, np.uint32)):
            v, ok = down(d, t)
            assert ok, "wrote outside " + name
            vals.append(v.copy())
        r.offsets, r.written, r.status = vals[0], vals[1][:n], vals[2][:n]
        if n == 0:
            assert (vals[1].view(np.uint8) == CANARY).all() and (vals[2].view(np.uint8) == CANARY).all()
        return r
    finally:
        for d in (own, dst, off, wr, st):
            if d is not None:
                d.free()


def child(n=40, size=131073):
    """run in a process of its own (ZSMI_BLOCKS_IN_FLIGHT=64): n frames of `size` bytes - three blocks a frame, 21 frames a sub-batch - with
    seeded choices: the archive of the resident call, whose sub-batches are planned on the device, is the host-array call's"""
    import test_gpu_seekable_frames as F
    from _hip import hip_of
    from zstandard_amd import BatchCodec, _lib
    bc = BatchCodec(0); H = hip_of(); L = _lib.lib()
    rng = np.random.default_rng(77)
    data = RC.stream_bytes()
    parts = [data[at:at + size] for at in (int(rng.integers(0, len(data) - size)) for _ in range(n))]
    index = u32([PICKS[int(rng.integers(0, len(PICKS)))] for _ in range(n)])
    cset, cds = RS.make_set(bc, 3)
    want = F.compress_frames(L, H, bc, parts, 3, 1, cset, index)
    got = write(L, H, bc, b"".join(parts), [size] * n, 3, 1, cset, index)
    assert got.rc == 0 and got.archive == want, (got.rc, hex(got.word), len(want))
    plain = write(L, H, bc, b"".join(parts), [size] * n, 1, 0)
    assert plain.rc == 0 and plain.archive == F.compress_frames(L, H, bc, parts, 1, 0)
    bc.sync(); cset.close()
    for cd in set(cds):
        cd.close()
    bc.close()
    print("CHILD-OK")


def chain_child(n=64, step=1500):
    """run in a process of its own, `import torch` its first statement (torch must be the first to load the HIP runtime): sizes, dictionary
    indices and frame numbers are made by torch ops on the codec's stream; the resident write, the open call and the resident read follow
    them there.  The host reads the archive's size - an argument of the open call, which waits once itself, as documented - and, at the
    end, the results it compares."""
    import torch
    import test_gpu_seekable_frames as F
    from zstandard_amd import BatchCodec, _lib
    L = _lib.lib()
    stream = torch.cuda.Stream()
    bc = BatchCodec(0, stream.cuda_stream)
    cset, cds = RS.make_set(bc, 3)
    dset, dds = ddict_set(bc)
    sizes = [step + 16 * i for i in range(n)]                                  # record k: 1500 + 16 k bytes
    data = RC.stream_bytes()[:sum(sizes)]
    p = ctypes.c_void_p
    with torch.cuda.stream(stream):
        src = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
        k = torch.arange(n, device="cuda", dtype=torch.int64)
        d_sizes = (step + 16 * k).to(torch.int32)
        picks = torch.tensor([int(v) for v in PICKS], device="cuda", dtype=torch.int64)
        d_index = picks[k % len(PICKS)].to(torch.int32)                         # (NO_DICT as int32 is -1: the same 32 bits)
        bound = L.zsmi_seekableFramesResidentBound(len(data), n, 1)
        arc = torch.full((bound,), CANARY, device="cuda", dtype=torch.uint8)
        size = torch.zeros(1, device="cuda", dtype=torch.int64)
        rc = L.zsmi_compressSeekableFramesResident_usingCDictSet(bc.ctx, p(src.data_ptr()), len(data), p(d_sizes.data_ptr()), n, max(sizes), p(arc.data_ptr()),
                                                                 bound, p(size.data_ptr()), 1, cset.handle, p(d_index.data_ptr()))
        assert rc == 0, rc
        m = int(size.item())                                                   # the open call's argument
        assert 0 < m <= bound, hex(m)
        err = ctypes.c_int(-1)
        sk = L.zsmi_openSeekableDevice_usingDDictSet(bc.ctx, p(arc.data_ptr()), m, dset.handle, ctypes.byref(err))
        assert sk and err.value == 0, err.value
        want_idx = (k * 37 + 11) % n
        d_req = want_idx.to(torch.int32)
        room = n * (max(sizes) + 64)
        out = torch.full((room,), CANARY, device="cuda", dtype=torch.uint8)
        off = torch.zeros(n + 1, device="cuda", dtype=torch.int64)
        wr = torch.zeros(n, device="cuda", dtype=torch.int32)
        st = torch.full((n,), -1, device="cuda", dtype=torch.int32)
        rc = L.zsmi_seekableReadFramesResident(bc.ctx, sk, p(d_req.data_ptr()), n, 64, p(out.data_ptr()), room, p(off.data_ptr()), p(wr.data_ptr()), p(st.data_ptr()))
        assert rc == 0, rc
        h_out, h_off, h_wr, h_st, h_idx = out.cpu().numpy(), off.cpu().numpy(), wr.cpu().numpy(), st.cpu().numpy(), want_idx.cpu().numpy()
        h_arc = arc.cpu().numpy()[:m].tobytes()
    starts = np.concatenate([[0], np.cumsum(sizes)])
    parts = [data[starts[i]:starts[i + 1]] for i in range(n)]
    assert not h_st.any(), h_st.tolist()
    assert h_wr.tolist() == [sizes[i] for i in h_idx]
    want_off = rounded_offsets([sizes[i] for i in h_idx], 64)
    assert (h_off.astype(np.uint64) == want_off).all()
    inside = np.zeros(room, dtype=bool)
    for q, i in enumerate(h_idx):
        assert h_out[int(want_off[q]):int(want_off[q]) + sizes[i]].tobytes() == parts[i], (q, i)
        inside[int(want_off[q]):int(want_off[q]) + sizes[i]] = True
    assert (h_out[~inside] == CANARY).all()
    from _hip import hip_of
    H = hip_of()
    index = u32([PICKS[i % len(PICKS)] for i in range(n)])
    assert h_arc == F.compress_frames(L, H, bc, parts, 3, 1, cset, index)        # the archive of the host-array call
    bc.sync()
    L.zsmi_closeSeekable(sk)
    dset.close(); cset.close()
    for h in dds + list(set(cds)):
        h.close()
    bc.close()
    print("CHILD-OK")

