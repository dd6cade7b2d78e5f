"""Content checksums on the frames this library writes (zsmi_setParameter(ZSMI_c_checksumFlag), BatchCodec.set_parameter("checksum"), the two
_advanced one-shots, ZstdCompressor(checksum=True)).  The contract, tests/_checksum.py: the frame of a flag-on call is the frame of the same
flag-off call, byte for byte, with bit 2 of byte 4 set and the low 32 bits of the chunk's XXH64 behind the last block - so the flag-off
pins (oracle E parity) carry over.  The reference for the bytes is not this change's: the flag-off frames are oracle E's, the trailer is
oracle D's zso_xxh64, and oracle D, libzstd and the library's decoder must all accept the frames and refuse the damaged ones.
Layouts and children: tests/_batch.py."""
import ctypes, os
import numpy as np
import pytest
import _oracle as O
import _data as D
import _corpus as C
import _dicts as X
import _batch as B
import _checksum as CK
import _seekable as SK
from _hip import hip_of, Dev, PAD

pytestmark = pytest.mark.gpu
GENERIC, UNSUPPORTED, OUT_OF_BOUND, FLAG = 1, 40, 42, 201
WRONG_WORD = (1 << 32) - CK.WRONG

# one mixed call: quads of one wavefront hash different lengths.  XXH64's tail and stripe edges; the FCS widths; one block (assembled in the
# literals kernel) and several (k_assemble_frames); two LZ units
SIZES = (0, 1, 3, 4, 7, 8, 31, 32, 33, 63, 64, 255, 256, 4096, 65535, 65536, 65537, 65791, 65792, 131072, 131073, 200000)
ONE_BLOCK, TWO_BLOCK = SIZES.index(65536), SIZES.index(65537)

_chunks = None


def chunks():
    """the 22 sizes cut from a Zipf log at different places, then a record stream, an all-equal chunk (RLE blocks) and a uniform-random
    chunk of one block (a raw block: the frame closest to the bound).  25 chunks: the last workgroup of the checksum kernel has idle quads"""
    global _chunks
    if _chunks is None:
        z = D.zipf_log(600000, single=True).tobytes()
        rng = np.random.default_rng(17)
        _chunks = [z[977 * i:977 * i + s] for i, s in enumerate(SIZES)]
        _chunks += [C.json_records(40000, seed=5)[:40000], bytes([0x5A]) * 70000, rng.integers(0, 256, 65536, dtype=np.uint8).tobytes()]
        assert len(_chunks) == 25
    return _chunks


RAW_BLOCK = 24


@pytest.fixture(scope="module")
def codec():
    from zstandard_amd import BatchCodec
    return BatchCodec(0)


@pytest.fixture()
def flag_on(codec):
    codec.set_parameter("checksum", 1)
    yield codec
    codec.set_parameter("checksum", 0)


def host_frames(codec, chunks, level=3, **form):
    return B.frames_of(codec.compress_host(*B.batch(chunks), level, **form), len(chunks))


def on_and_off(codec, chunks, level=3, **form):
    """the frames of one host-form call with the flag off and of the same call with it on"""
    assert codec.get_parameter("checksum") == 0
    off = host_frames(codec, chunks, level, **form)
    codec.set_parameter("checksum", 1)
    try:
        on = host_frames(codec, chunks, level, **form)
    finally:
        codec.set_parameter("checksum", 0)
    return off, on


def assert_identity(off, on, chunks, what=""):
    for i, (a, b, c) in enumerate(zip(off, on, chunks)):
        assert len(b) == len(a) + 4, (what, i, len(c), len(a), len(b))
        assert b == CK.with_checksum(a, c), (what, i, len(c), B.first_difference(b, CK.with_checksum(a, c)))


def device_compress(codec, H, chunks, level):
    """zsmi_compressBatchDevice into a canary-filled buffer, ragged layout -> (the whole buffer with its pads, dst offsets in it, sizes, bounds)"""
    src_np, so, sizes = B.batch(chunks)
    so, do, bounds, total = B.ragged_device_layout(codec.L, sizes, np.random.default_rng(9))
    src, dst, dsz = Dev(H, len(src_np), src_np.tobytes()), Dev(H, total), Dev(H, 4 * len(sizes))
    try:
        codec.compress_device(src.p, so, sizes, dst.p, do, dsz.p, level)
        codec.sync()
        host = np.frombuffer(dst.all(), dtype=np.uint8)
        sz = np.frombuffer(dsz.all()[PAD:PAD + 4 * len(sizes)], dtype=np.uint32)
    finally:
        for b in (src, dst, dsz):
            b.free()
    return host, do + np.uint64(PAD), sz, bounds


def device_decode(codec, H, frames, caps):
    """zsmi_decompressBatchDevice -> [(size or error word, bytes)]"""
    src_np, so, ss = B.batch(frames)
    caps = np.maximum(np.array(caps, dtype=np.uint32), 1)
    do = B.layout(caps)
    src, dst, dsz = Dev(H, len(src_np), src_np.tobytes()), Dev(H, int(caps.sum())), Dev(H, 4 * len(ss))
    try:
        codec.decompress_device(src.p, so, ss, dst.p, do, caps, dsz.p)
        codec.sync()
        out = dst.all()[PAD:]
        sz = np.frombuffer(dsz.all()[PAD:PAD + 4 * len(ss)], dtype=np.uint32)
    finally:
        for b in (src, dst, dsz):
            b.free()
    return [(int(s), out[int(o):int(o) + (int(s) if s < B.ERR else 0)]) for o, s in zip(do, sz)]


_mixed = {}


def mixed(codec, level):
    """the mixed batch through the device form, flag off and flag on, once a level"""
    if level not in _mixed:
        H = hip_of()
        assert codec.get_parameter("checksum") == 0
        off = device_compress(codec, H, chunks(), level)
        codec.set_parameter("checksum", 1)
        try:
            on = device_compress(codec, H, chunks(), level)
        finally:
            codec.set_parameter("checksum", 0)
        _mixed[level] = (off, on)
    return _mixed[level]


# ------------------------------------------------------------------ 1. the contract, one mixed call
@pytest.mark.parametrize("level", [1, 3])
def test_mixed_call_frames_are_the_plain_frames_with_a_checksum(codec, level):
    ch = chunks()
    (h0, do0, sz0, bounds), (h1, do1, sz1, _) = mixed(codec, level)
    assert (sz0 < B.ERR).all() and (sz1 < B.ERR).all()
    off, on = B.cut(h0, do0, sz0), B.cut(h1, do1, sz1)
    assert off == B.oracle_frames(ch, level)                                      # flag off: oracle E's frames, as ever
    assert (sz1 == sz0 + 4).all(), (sz0.tolist(), sz1.tolist())
    assert_identity(off, on, ch, level)
    assert on[0][-4:] == CK.EMPTY_TRAILER and len(on[0]) == len(off[0]) + 4       # the empty chunk
    assert len(on[RAW_BLOCK]) == 65536 + 7 + 3 + 4                                # the raw block: header, block header, content, checksum
    # canaries: a chunk of several blocks and an empty one touch nothing but the frame; a one-block chunk's literals kernel works inside the
    # chunk's zsmi_compressBound slot, with and without the flag (tests/test_gpu_cdict_set.py states the same of every call form)
    sizes = np.array([len(c) for c in ch])
    for host, do, sz in ((h0, do0, sz0), (h1, do1, sz1)):
        B.assert_only_frames_written(host, do, np.where((sizes > 65536) | (sizes == 0), sz, bounds), bounds, B.CANARY, level)
    for i, (f, c) in enumerate(zip(on, ch)):
        assert O.decompress(f, len(c)) == c, (level, "oracle D", i, len(c))
        if O.libzstd():
            assert O.zstd_decompress(f, len(c)) == c, (level, "libzstd", i, len(c))
    got = device_decode(codec, hip_of(), on, [len(c) for c in ch])
    for i, ((s, b), c) in enumerate(zip(got, ch)):
        assert s == len(c) and b == c, (level, "zsmi_decompressBatchDevice", i, len(c), hex(s))


# ------------------------------------------------------------------ 2. the same identity through the other forms
def dict_chunks(cls="json_records"):
    data = X.class_data(cls)
    return [data[3000 * i:3000 * i + s] for i, s in enumerate((0, 1, 255, 256, 4096, 40000, 65536, 65537, 65792, 131073))]


def test_host_form_and_using_dict(codec):
    ch = chunks()
    off, on = on_and_off(codec, ch)
    assert off == B.oracle_frames(ch, 3)
    assert_identity(off, on, ch, "host form")
    assert on == B.cut(*mixed(codec, 3)[1][:3])                                   # (the device form's frames)
    dic, dch = X.trained("json_records"), dict_chunks()
    off, on = on_and_off(codec, dch, dictionary=dic)
    assert off == B.oracle_frames(dch, 3, dic)
    assert_identity(off, on, dch, "_usingDict")
    did = O.dict_params(dic)[1]
    for f in on:                                                                  # the ID field shifts byte 4's neighbours, not byte 4
        code = f[4] & 3
        assert code and f[4] & 4 and int.from_bytes(f[5:5 + (0, 1, 2, 4)[code]], "little") == did
    B.assert_round_trip(codec, on, dch, dic, "_usingDict, checksummed")


def test_using_cdict_and_using_cdict_set(codec):
    from zstandard_amd import CompressionDict, CompressionDictSet, DecompressionDict, DecompressionDictSet, NO_DICT
    dics = [X.trained("json_records"), X.trained("zipf")]
    cds = [CompressionDict(codec, d, 3) for d in dics]
    dch = dict_chunks()
    off, on = on_and_off(codec, dch, cdict=cds[0])
    assert_identity(off, on, dch, "_usingCDict")
    B.assert_round_trip(codec, on, dch, dics[0], "_usingCDict, checksummed")
    # two members and chunks without a dictionary, interleaved; decoded by ONE _usingDDictSet call
    both = [c for pair in zip(dict_chunks("json_records"), dict_chunks("zipf"), dict_chunks("xml_records")) for c in pair]
    index = np.array([(0, 1, NO_DICT)[i % 3] for i in range(len(both))], dtype=np.uint32)
    cset = CompressionDictSet(codec, cds, 3)
    off, on = on_and_off(codec, both, cdict_set=cset, dict_index=index)
    assert_identity(off, on, both, "_usingCDictSet")
    dds = [DecompressionDict(codec, d) for d in dics]
    dset = DecompressionDictSet(codec, dds)
    out, oo, osz = codec.decompress_host(*B.batch(on), np.maximum(np.array([len(c) for c in both], dtype=np.uint32), 1), ddict_set=dset)
    assert [int(s) for s in osz] == [len(c) for c in both] and B.cut(out, oo, osz) == both
    for i, (f, c) in enumerate(zip(on, both)):
        dic = dics[index[i]] if index[i] != NO_DICT else b""
        assert CK.oracle_code(f, len(c), dic) == 0, i
    cset.close(); dset.close()
    for x in cds + dds:
        x.close()


def test_one_shot_advanced_calls(codec):
    from zstandard_amd import ZstdCompressor, CompressionDict
    L = codec.L

    def shot(fn, data, *tail):
        cap = L.zsmi_compressBound(len(data))
        out = ctypes.create_string_buffer(cap)
        r = fn(out, cap, data, len(data), *tail)
        assert not L.zsmi_isError(r), L.zsmi_getErrorName(r)
        return out.raw[:r]

    dic = X.trained("json_records")
    cd = CompressionDict(codec, dic, 3)
    for c in (chunks()[i] for i in (0, 1, ONE_BLOCK, TWO_BLOCK, RAW_BLOCK)):
        plain = shot(L.zsmi_compress, c, 3)
        assert plain == O.compress(c, 3)
        assert shot(L.zsmi_compress_advanced, c, None, 0, 3, 0) == plain
        assert shot(L.zsmi_compress_advanced, c, None, 0, 3, 1) == CK.with_checksum(plain, c)
        assert ZstdCompressor(3, checksum=True).compress(c) == CK.with_checksum(plain, c)
        assert shot(L.zsmi_compress, c, 3) == plain                                # (the pooled context kept no flag)
    for c in dict_chunks()[:7]:
        plain = shot(L.zsmi_compress_usingDict, c, dic, len(dic), 3)
        assert shot(L.zsmi_compress_advanced, c, dic, len(dic), 3, 0) == plain
        assert shot(L.zsmi_compress_advanced, c, dic, len(dic), 3, 1) == CK.with_checksum(plain, c)
        assert ZstdCompressor(3, dictionary=dic, checksum=True).compress(c) == CK.with_checksum(plain, c)
        plain = shot(L.zsmi_compress_usingCDict, c, cd.handle)
        assert shot(L.zsmi_compress_usingCDict_advanced, c, cd.handle, 0) == plain
        assert shot(L.zsmi_compress_usingCDict_advanced, c, cd.handle, 1) == CK.with_checksum(plain, c)
        assert ZstdCompressor(dictionary=cd, checksum=True).compress(c) == CK.with_checksum(plain, c)
        assert O.decompress_using_dict(CK.with_checksum(plain, c), len(c), dic) == c
    cd.close()


# ------------------------------------------------------------------ 3. corruption
def test_a_flipped_bit_is_checksum_wrong_on_that_item_alone(codec):
    ch = chunks()
    on = B.cut(*mixed(codec, 3)[1][:3])
    targets = (ONE_BLOCK, TWO_BLOCK, RAW_BLOCK)
    caps = [len(c) for c in ch]
    H = hip_of()
    for what in ("trailer", "payload"):
        bad = list(on)
        for i in targets:
            if what == "trailer":
                at = (len(on[i]) - 3, 6)
            else:                                                                 # a bit of the last block's payload, chosen on the CPU: oracle D itself says checksum_wrong
                at = CK.payload_flip_oracle_calls_checksum_wrong(on[i], caps[i])
                assert at is not None and CK.last_block(on[i]).pos <= at[0] < CK.last_block(on[i]).end, (i, at)
            bad[i] = CK.flip(on[i], *at)
            assert CK.oracle_code(bad[i], caps[i]) == CK.WRONG, (what, i)
            if O.libzstd():
                assert O.zstd_decompress(bad[i], caps[i]) is None, (what, i)
        for how, got in (("device", device_decode(codec, H, bad, caps)), ("host", B.decode_many(codec, bad, caps))):
            for i, ((s, b), c) in enumerate(zip(got, ch)):
                if i in targets:
                    assert s == WRONG_WORD, (what, how, i, hex(s))
                else:
                    assert s == len(c) and b == c, (what, how, i, hex(s))


# ------------------------------------------------------------------ 4. sub-batches
_SUB_CHILD = r'''
import sys, os
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import numpy as np
import _data as D, _batch as B, _checksum as CK
from zstandard_amd import BatchCodec
bc = BatchCodec(0)
z = D.zipf_log(131073 + 40 * 1013, single=True).tobytes()
chunks = [z[1013 * i:1013 * i + 131073] for i in range(40)]                # 3 blocks each: 120 blocks, two sub-batches of <= 64
off = B.frames_of(bc.compress_host(*B.batch(chunks), 3))
assert off == B.oracle_frames(chunks, 3)
bc.set_parameter("checksum", 1)
bc.enable_timing(True)
on = B.frames_of(bc.compress_host(*B.batch(chunks), 3))
times = bc.kernel_times()
assert times["k_lz_stitch"][1] == 2, times                                # (two sub-batches)
assert times["k_frame_checksum"][1] == 1, times                            # one launch over all 40 chunks
for i, (a, b, c) in enumerate(zip(off, on, chunks)):
    assert b == CK.with_checksum(a, c), i
print("CHILD-OK")
'''


def test_sub_batches_get_one_checksum_launch():
    """ZSMI_BLOCKS_IN_FLIGHT=64 in a child process: 40 chunks of 131073 bytes are 120 blocks in two sub-batches; the identity holds for all
    40 and the call launches k_frame_checksum exactly once, behind the last sub-batch"""
    B.run_child("-c", _SUB_CHILD, B.ROOT, env=dict(os.environ, ZSMI_BLOCKS_IN_FLIGHT="64"))


# ------------------------------------------------------------------ 5. the parameter; flag off is untouched
def test_parameter_checks_and_flag_off_launches_nothing_new():
    from zstandard_amd import BatchCodec
    bc = BatchCodec(0)
    L = bc.L
    v = ctypes.c_int(-1)
    assert bc.get_parameter("checksum") == 0 and bc.get_parameter(FLAG) == 0      # the default
    assert L.zsmi_setParameter(bc.ctx, 200, 1) == UNSUPPORTED
    assert L.zsmi_setParameter(bc.ctx, 200, 7) == UNSUPPORTED                      # (the parameter is judged before the value)
    assert L.zsmi_setParameter(bc.ctx, FLAG, 2) == OUT_OF_BOUND and L.zsmi_setParameter(bc.ctx, FLAG, -1) == OUT_OF_BOUND
    assert L.zsmi_getParameter(bc.ctx, 200, None) == UNSUPPORTED
    assert L.zsmi_getParameter(bc.ctx, FLAG, None) == GENERIC
    assert L.zsmi_getParameter(bc.ctx, FLAG, ctypes.byref(v)) == 0 and v.value == 0    # (the refusals changed nothing)
    with pytest.raises(RuntimeError, match="out of bound"):
        bc.set_parameter("checksum", 2)
    with pytest.raises(ValueError):
        bc.set_parameter("checksums", 1)
    ch = chunks()
    want = B.oracle_frames(ch, 3)
    bc.enable_timing(True)

    def call(flag):
        frames = host_frames(bc, ch)
        times = bc.kernel_times()
        assert ("k_frame_checksum" in times) == bool(flag), (flag, sorted(times))
        assert "k_encode_literals" in times and "k_assemble_frames" in times
        if flag:
            assert times["k_frame_checksum"][1] == 1
            assert_identity(want, frames, ch, "sticky")
        else:
            assert frames == want                                                 # oracle E's
        return sorted(times)

    fresh = call(0)                                                               # a fresh context
    bc.set_parameter("checksum", 1); assert bc.get_parameter("checksum") == 1
    on = call(1)
    assert [k for k in on if k != "k_frame_checksum"] == fresh                    # (the launches of the flag-off call, and one more)
    bc.set_parameter(FLAG, 0); assert bc.get_parameter(FLAG) == 0
    assert call(0) == fresh
    bc.set_parameter("checksum", True)
    call(1)
    bc.close()


# ------------------------------------------------------------------ 6. seekable archives
@pytest.mark.parametrize("table_checksum", [True, False])
def test_seekable_frames_carry_the_checksum(flag_on, table_checksum):
    from zstandard_amd import SeekableArchive
    codec = flag_on
    data = D.zipf_log(300 << 10, seed_lo=23, single=True).tobytes()
    parts = SK.slices(data, 65536)
    assert len(parts) == 5
    H = hip_of()
    bound = codec.seekable_bound(len(data), 65536, table_checksum)
    src, dst, size = Dev(H, len(data), data), Dev(H, bound), Dev(H, 8)
    try:
        codec.compress_seekable_device(src.p, len(data), dst.p, bound, size.p, 3, 65536, table_checksum)
        codec.sync()
        n = int.from_bytes(size.all()[PAD:PAD + 8], "little")
        assert n <= bound
        whole = dst.all()
        arc = whole[PAD:PAD + n]
        assert whole[:PAD] == bytes([B.CANARY]) * PAD and whole[PAD + bound:] == bytes([B.CANARY]) * PAD
    finally:
        for b in (src, dst, size):
            b.free()
    # the archive with plain frames, frame for frame with a checksum: the table's sizes include the 4 bytes, its own flag is the call's
    frames = [CK.with_checksum(O.compress(p, 3), p) for p in parts]
    assert arc == SK.archive(frames, parts, table_checksum)
    rows, ck = SK.parse(arc)                                                      # (the sizes add up, or parse refuses)
    assert ck == table_checksum and [r[0] for r in rows] == [len(f) for f in frames]
    pos = 0
    for r in rows:
        assert arc[pos + 4] & CK.CHECKSUM_BIT, pos
        pos += r[0]
    sa = SeekableArchive(arc)
    assert sa.read() == data
    if O.libzstd():
        assert O.zstd_decompress(arc, len(data)) == data                          # concatenated frames, then a skippable one
    # a content bit of frame 2: the frame's own checksum catches it, with or without the table's
    start = sum(len(f) for f in frames[:2])
    at = CK.payload_flip_oracle_calls_checksum_wrong(frames[2], len(parts[2]))
    assert at is not None
    bad = SeekableArchive(CK.flip(arc, start + at[0], at[1]))
    with pytest.raises(RuntimeError, match="doesn't match checksum"):
        bad.read(2 * 65536 + 100, 1000)
    with pytest.raises(RuntimeError, match="doesn't match checksum"):
        bad.read(65536 + 60000, 10000)                                            # (a range that ends in frame 2)
    assert bad.read(65536, 65536) == parts[1] and bad.read(3 * 65536, 1 << 20) == data[3 * 65536:]
    res, codes = bad.read_many([(0, 1000), (2 * 65536, 10), (4 * 65536, 500)], return_codes=True)
    assert codes == [0, CK.WRONG, 0] and res[0] == data[:1000] and res[2] == data[4 * 65536:4 * 65536 + 500]
    sa.close(); bad.close()


def test_one_shot_seekable_is_unchanged(flag_on):
    from zstandard_amd import ZstdCompressor
    data = D.zipf_log(150000, seed_lo=29, single=True).tobytes()
    assert ZstdCompressor(3).compress_seekable(data, 65536, True) == SK.oracle_archive(data, 65536, 3, True)


# ------------------------------------------------------------------ 7. the trainer does not see the parameter
def test_trained_dictionary_does_not_depend_on_the_flag(codec):
    data = X.class_data("json_records")[:256 << 10]
    sizes = np.full(256, 1024, dtype=np.uint32)
    offs = B.layout(sizes)
    dev = Dev(hip_of(), len(data), data)
    try:
        assert codec.get_parameter("checksum") == 0
        a = codec.train_device(dev.p, offs, sizes, 8192, k=0, d=8, steps=3)       # (k searched: the scoring calls and the finalize call both compress)
        codec.set_parameter("checksum", 1)
        try:
            b = codec.train_device(dev.p, offs, sizes, 8192, k=0, d=8, steps=3)
        finally:
            codec.set_parameter("checksum", 0)
    finally:
        dev.free()
    assert a == b and len(a[0]) > 256 and a[0][:4] == bytes([0x37, 0xA4, 0x30, 0xEC])


# ------------------------------------------------------------------ 8. the decoder's fast path takes them
_FAST_CHILD = r'''
import os; os.environ["ZSMI_DEBUG_LIB"] = "1"
import sys, ctypes
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import numpy as np
import _data as D, _batch as B
from zstandard_amd import BatchCodec, _lib
if _lib.built_fingerprint() != _lib.source_fingerprint():
    _lib.build()
bc = BatchCodec(0); Z = _lib.lib()
lay = (ctypes.c_uint32 * 6)(); Z.zsmi_dbg_descLayout(lay)
WORDS, FAST_AT, WHY_AT = int(lay[0]), int(lay[1]), int(lay[2])
text = D.zipf_log(48 * 32768, seed_lo=41, single=True).tobytes()
chunks = [text[i * 32768:(i + 1) * 32768] for i in range(48)]
bc.set_parameter("checksum", 1)
frames = B.frames_of(bc.compress_host(*B.batch(chunks), 3))
assert all(f[4] & 4 for f in frames)
frames[7] = frames[7][:-1] + bytes([frames[7][-1] ^ 0x10])               # one damaged trailer: the fast path itself reports it
got = B.decode_many(bc, frames, [len(c) for c in chunks], min_cap=0)
buf = np.zeros(len(chunks) * WORDS, dtype=np.uint32)
assert Z.zsmi_dbg_copyScratch(bc.ctx, b"fastDesc", buf.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(buf.nbytes)) == 0
desc = buf.reshape(-1, WORDS)
for i, ((s, b), c) in enumerate(zip(got, chunks)):
    assert desc[i, FAST_AT] == 1, (i, "left the fast path", int(desc[i, WHY_AT]))
    assert (s == (1 << 32) - 22) if i == 7 else (s == len(c) and b == c), (i, hex(s))
print("CHILD-OK")
'''


def test_checksummed_frames_decode_on_the_fast_path():
    """a child with the debug-hook library (the hook tools/fastpath_check.py reads): 48 checksummed frames of 32 KiB are decoded by the fast
    kernels, ZsFastDesc.fast says so for every item, and the one with a damaged trailer is checksum_wrong there"""
    B.run_child("-c", _FAST_CHILD, B.ROOT)
