"""Digested dictionaries on the GPU (zsmi_createCDict, zsmi_compress*_usingCDict; CompressionDict).  With raw content a CDict's frames are
the _usingDict frames byte for byte (and so oracle E's).  With a formatted dictionary the first block of a frame may be coded with the
dictionary's own entropy tables - Treeless literals (type 3), Repeat_Mode (3) sequence tables - where that is smaller: every frame must
decode to its input with the dictionary under oracle D, the library's decoder and upstream libzstd; a frame that uses neither is the
_usingDict frame; no later block uses them; the batch never grows and shrinks at 1 KiB; symbols the dictionary cannot code are never
coded with it.  Dictionaries and chunks: tests/_dicts.py; batches and round trips: tests/_batch.py; frame structure: tests/_cdict.py."""
import ctypes, os
import numpy as np
import pytest
import _oracle as O
import _data as D
import _dicts as X
import _batch as B
import _cdict as K
import _framewriter as W

pytestmark = pytest.mark.gpu
SIZES_FIX = os.path.join(D.GOLDEN, "libzstd_fixtures_cdict_sizes.npz")


@pytest.fixture(scope="module")
def codec():
    from zstandard_amd import BatchCodec
    return BatchCodec(0)


def assert_structure(frames, plain, what=""):
    """a frame that uses none of the dictionary's tables is the _usingDict frame; only a frame's first block may use them"""
    used = 0
    for i, (f, p) in enumerate(zip(frames, plain)):
        blocks = K.blocks_of(f)
        assert not any(K.uses_dictionary_tables(b) for b in blocks[1:]), (what, i, blocks)
        if K.uses_dictionary_tables(blocks[0]):
            used += 1
        else:
            assert f == p, (what, i, len(f), len(p), B.first_difference(f, p))
    return used


def formatted_dictionaries():
    return {k: v for k, v in X.identity_dictionaries().items() if not k.startswith("raw")}


# ------------------------------------------------------------------ 1. raw content: the _usingDict frames
@pytest.mark.parametrize("level", [1, 3, 4])
def test_raw_content_frames_equal_usingdict(codec, level):
    from zstandard_amd import CompressionDict
    for name, dic in X.identity_dictionaries().items():
        if not name.startswith("raw"):
            continue
        chunks = X.prefix_chunks(dic)
        cd = CompressionDict(codec, dic, level)
        assert cd.dict_id == 0 and cd.device_bytes >= len(dic)
        frames = B.compress_many(codec, chunks, cdict=cd)
        cd.close()
        plain = B.compress_many(codec, chunks, level, dic)
        expect = B.oracle_frames(chunks, level, dic)
        for i, (f, p, e) in enumerate(zip(frames, plain, expect)):
            assert f == p == e, (name, level, i, len(chunks[i]), len(f), len(p), len(e))


# ------------------------------------------------------------------ 2., 3. formatted dictionaries: round trip and structure
@pytest.mark.parametrize("level", [1, 3, 4])
def test_formatted_dictionaries_round_trip(codec, level):
    from zstandard_amd import CompressionDict
    used = 0
    for name, dic in formatted_dictionaries().items():
        chunks = X.prefix_chunks(dic)
        cd = CompressionDict(codec, dic, level)
        assert cd.dict_id == int.from_bytes(dic[4:8], "little")
        frames = B.compress_many(codec, chunks, cdict=cd)
        cd.close()
        B.assert_round_trip(codec, frames, chunks, dic, name)
        cd_id = int.from_bytes(dic[4:8], "little")
        for f in frames:
            code = f[4] & 3
            assert code and int.from_bytes(f[5:5 + (4 if code == 3 else code)], "little") == cd_id
        used += assert_structure(frames, B.compress_many(codec, chunks, level, dic), name)
    assert used > 0


def test_small_records_use_the_dictionarys_tables(codec):
    """1 KiB chunks of each record class with its trained dictionary: Treeless literals and at least one Repeat_Mode occur"""
    from zstandard_amd import CompressionDict
    for cls in X.RECORD_CLASSES:
        dic, chunks = X.trained(cls), K.size_chunks(cls, 1024)
        cd = CompressionDict(codec, dic, 3)
        frames = B.compress_many(codec, chunks, cdict=cd)
        cd.close()
        first = [K.blocks_of(f)[0] for f in frames]
        assert any(b[1] == 3 for b in first), (cls, "no treeless literals")
        assert any(b[2] is not None and any(((b[2] >> s) & 3) == 3 for s in (6, 4, 2)) for b in first), (cls, "no repeat mode")
        assert_structure(frames, B.compress_many(codec, chunks, 3, dic), cls)
        B.assert_round_trip(codec, frames, chunks, dic, cls)


# ------------------------------------------------------------------ 4. size
def test_sizes_against_usingdict_and_libzstd(codec):
    """per (class, chunk size): the CDict batch is never larger than the _usingDict batch, and strictly smaller at 1 KiB; against libzstd
    1.4.8's sizes for the same chunks (the fixture) the CDict ratio is not worse than the _usingDict ratio.  The largest growth of a single
    frame is reported, not asserted: the sequence tables are chosen by estimates."""
    from zstandard_amd import CompressionDict
    fix = np.load(SIZES_FIX)
    table, worst = {}, (0, None)
    for cls in X.RECORD_CLASSES:
        dic = X.trained(cls)
        cd = CompressionDict(codec, dic, 3)
        for cs in K.SIZE_CHUNKS:
            chunks = K.size_chunks(cls, cs)
            a = B.compress_many(codec, chunks, cdict=cd)
            b = B.compress_many(codec, chunks, 3, dic)
            ta, tb, tz = sum(map(len, a)), sum(map(len, b)), int(fix[f"{cls}_{cs}"])
            table[(cls, cs)] = (tb, ta, tz, round(tb / tz, 4), round(ta / tz, 4))
            grow = max(len(x) - len(y) for x, y in zip(a, b))
            if grow > worst[0]:
                worst = (grow, (cls, cs))
        cd.close()
    for k, v in table.items():
        print("cdict sizes", k, "usingDict %d cdict %d libzstd %d  ours/libzstd %.4f -> %.4f" % v)
    print("largest growth of one frame:", worst)
    for (cls, cs), (tb, ta, tz, rb, ra) in table.items():
        assert ta <= tb, (cls, cs, ta, tb)
        assert ta / tz <= tb / tz, (cls, cs)
        if cs == 1024:
            assert ta < tb, (cls, cs, ta, tb)


# ------------------------------------------------------------------ 5. symbols the dictionary cannot code
def test_symbols_the_dictionary_cannot_code(codec):
    from zstandard_amd import CompressionDict
    dic = K.narrow_dictionary()
    assert O.dict_params(dic)[1] == 77                                    # oracle D accepts the dictionary
    probe = b"abcdefgh" * 8
    assert O.decompress_using_dict(O.compress_using_dict(probe, dic, 3), len(probe), dic) == probe
    rng = np.random.default_rng(11)
    text = lambda k, alphabet: bytes(rng.choice(np.frombuffer(alphabet, dtype=np.uint8), k).tolist())
    covered = [text(k, b"abcdefgh") for k in (100, 300, 1000, 5000)]                        # literals the table codes; long literal runs (LL codes > 3)
    foreign = [text(k, b"abcdefghXYZ012") for k in (100, 300, 1000, 5000)] + [bytes(range(256)) * 3, X.class_data("json_records")[:3000]]
    far = [text(200, b"abcdefgh") + bytes(range(256)) + text(50, b"abcdefgh") + bytes(range(256))[::-1] * 2]   # long matches, far offsets
    chunks = covered + foreign + far
    for level in (1, 3):
        cd = CompressionDict(codec, dic, level)
        frames = B.compress_many(codec, chunks, cdict=cd)
        cd.close()
        B.assert_round_trip(codec, frames, chunks, dic, "narrow")
        assert_structure(frames, B.compress_many(codec, chunks, level, dic), "narrow")
        for f, c in zip(frames[len(covered):len(covered) + 4], foreign[:4]):              # bytes without a code: never treeless
            b0 = K.blocks_of(f)[0]
            assert b0[1] != 3, b0


# ------------------------------------------------------------------ 6. the frames themselves
def test_formatted_dictionary_frames_are_pinned(codec):
    """no oracle writes Repeat_Mode or treeless blocks: the frames of a fixed set of records under formatted dictionaries (trained ones,
    whose counts hold -1 entries, and the narrow one) are pinned by the digests of tests/golden/cdict_frame_digests.json (made by
    gen_fixtures_cdict_frames.py before the encoder's table builders were unified); the frames' own bytes say that the pin covers a first
    block with a Repeat_Mode and one with treeless literals"""
    import json
    from zstandard_amd import CompressionDict
    want = json.load(open(os.path.join(D.GOLDEN, "cdict_frame_digests.json")))
    got, repeat, treeless = {}, 0, 0
    for name, (dic, records) in K.pin_cases().items():
        for level in K.PIN_LEVELS:
            cd = CompressionDict(codec, dic, level)
            frames = B.compress_many(codec, records, cdict=cd)
            cd.close()
            first = [K.blocks_of(f)[0] for f in frames]
            repeat += sum(K.uses_repeat_mode(b) for b in first); treeless += sum(b[1] == 3 for b in first)
            got[f"{name}_l{level}"] = K.frames_digest(frames)
    assert repeat > 0 and treeless > 0, (repeat, treeless)
    assert got == want, sorted(k for k in want if got.get(k) != want[k])


# ------------------------------------------------------------------ 7. lifecycle
def test_one_cdict_many_calls_and_two_in_alternation(codec):
    from zstandard_amd import CompressionDict
    da, db = X.trained("json_records"), X.trained("zipf")
    ca, cb = CompressionDict(codec, da, 3), CompressionDict(codec, db, 1)
    data = X.class_data("json_records")
    layouts = [[data[i:i + 1024] for i in range(0, 64 * 1024, 1024)],
               [data[0:300], data[1000:66536], data[70000:70000 + 65537], data[200000:200000 + 150000], b"", b"x", data[5:4101]],
               [data[i:i + 4096] for i in range(4096, 40 * 4096, 4096)]]
    first = {}
    for rnd in range(2):
        for k, chunks in enumerate(layouts):
            plain = B.compress_many(codec, chunks, 3)
            ud = B.compress_many(codec, chunks, 3, da)
            fa = B.compress_many(codec, chunks, cdict=ca)
            fb = B.compress_many(codec, chunks, cdict=cb)
            fa2 = B.compress_many(codec, chunks, cdict=ca)
            assert fa == fa2
            assert B.compress_many(codec, chunks, 3) == plain and B.compress_many(codec, chunks, 3, da) == ud      # the older calls: unchanged
            if rnd == 0:
                first[k] = (plain, ud, fa, fb)
                assert plain == B.oracle_frames(chunks, 3)
                assert ud == B.oracle_frames(chunks, 3, da)
                B.assert_round_trip(codec, fa, chunks, da, "A")
                B.assert_round_trip(codec, fb, chunks, db, "B")
                assert_structure(fa, ud, "A")
                assert_structure(fb, B.compress_many(codec, chunks, 1, db), "B")
            else:
                assert first[k] == (plain, ud, fa, fb)
    ca.close(); cb.close()


def test_corrupted_dictionaries_give_null_with_code_30(codec):
    from zstandard_amd import CompressionDict
    L = codec.L
    for d in X.bad_dictionaries():
        err = ctypes.c_int(0)
        assert not L.zsmi_createCDict(codec.ctx, d, len(d), 3, ctypes.byref(err)) and err.value == 30
        assert not L.zsmi_createCDict(codec.ctx, d, len(d), 3, None)
        with pytest.raises(RuntimeError, match="error 30"):
            CompressionDict(codec, d)


def test_every_entry_point_gives_a_dictionary_the_same_verdict(codec):
    """one loader decides: for every dictionary of tests/_dicts.py (valid, with each ID field size, refused) zsmi_createCDict,
    zsmi_createDDict, the device and the host _usingDict compress of one 100-byte chunk and the _usingDict decode of one plain 100-byte
    frame (its per-item code) answer 30 together or succeed together, as oracle D does; on success the three IDs agree"""
    from _hip import hip_of, Dev
    L, H = codec.L, hip_of()
    vp, p = ctypes.c_void_p, lambda a: a.ctypes.data_as(ctypes.c_void_p)
    chunk = X.class_data("json_records")[:100]
    frame = O.compress(chunk, 3)
    src, so, ss = B.batch([chunk])
    bound = L.zsmi_compressBound(len(chunk))
    dsrc, ddst, dsz = Dev(H, len(chunk), chunk), Dev(H, bound), Dev(H, 4)
    do = np.zeros(1, dtype=np.uint64)
    dicts = list(X.identity_dictionaries().values()) + list(X.id_dictionaries().values()) + X.bad_dictionaries()
    refused = 0
    for k, d in enumerate(dicts):
        try:
            want, want_id = 0, O.dict_params(d)[1]
        except O.OracleError as e:
            want, want_id = e.code, None
        err = ctypes.c_int(-1)
        cd = L.zsmi_createCDict(codec.ctx, d, len(d), 3, ctypes.byref(err))
        verdicts = {"createCDict": err.value}
        dd = L.zsmi_createDDict(codec.ctx, d, len(d), ctypes.byref(err))
        verdicts["createDDict"] = err.value
        ddic = Dev(H, len(d), d)
        verdicts["device compress"] = L.zsmi_compressBatchDevice_usingDict(codec.ctx, vp(dsrc.p), p(so), p(ss), 1, vp(ddst.p), p(do), vp(dsz.p), 3, vp(ddic.p), len(d))
        codec.sync(); ddic.free()
        hsz, out = np.zeros(1, dtype=np.uint32), np.zeros(bound, dtype=np.uint8)
        dbuf = np.frombuffer(d, dtype=np.uint8)
        verdicts["host compress"] = L.zsmi_compressBatchHost_usingDict(codec.ctx, p(src), p(so), p(ss), 1, p(out), p(do), p(hsz), 3, p(dbuf), len(d))
        (sz, got), = B.decode_many(codec, [frame], [len(chunk)], d)
        verdicts["decode"] = 0x100000000 - sz if sz > B.ERR else 0
        assert set(verdicts.values()) == {want} and want in (0, 30), (k, len(d), want, verdicts)
        assert bool(cd) == bool(dd) == (want == 0), (k, len(d))
        if want == 0:
            assert got == chunk and hsz[0] < B.ERR and O.decompress_using_dict(out[:int(hsz[0])].tobytes(), len(chunk), d) == chunk, (k, len(d))
            assert L.zsmi_getDictID_fromCDict(cd) == L.zsmi_getDictID_fromDDict(dd) == want_id, (k, len(d), want_id)
        refused += want == 30
        L.zsmi_freeCDict(cd); L.zsmi_freeDDict(dd)
    assert refused == len(X.bad_dictionaries()) >= 9
    for b in (dsrc, ddst, dsz):
        assert b.all()[:4096] == bytes([B.CANARY]) * 4096 and b.all()[-4096:] == bytes([B.CANARY]) * 4096
        b.free()


def test_one_shot_null_and_compressor_forms(codec):
    from zstandard_amd import CompressionDict, ZstdCompressor
    L = codec.L
    dic = X.trained("xml_records")
    cd = CompressionDict(codec, dic, 3)
    data = X.class_data("xml_records")
    chunks = [data[:1024], data[2000:2000 + 4096], b"", b"q", data[10000:10000 + 70000]]
    batch = B.compress_many(codec, chunks, cdict=cd)
    for c, f in zip(chunks, batch):
        out = ctypes.create_string_buffer(L.zsmi_compressBound(len(c)))
        r = L.zsmi_compress_usingCDict(out, len(out), c, len(c), cd.handle)
        assert not L.zsmi_isError(r) and out.raw[:r] == f
        assert ZstdCompressor(dictionary=cd).compress(c) == f
        r = L.zsmi_compress_usingCDict(out, len(out), c, len(c), None)              # NULL: the plain call at level 3
        assert out.raw[:r] == O.compress(c, 3)
    small = ctypes.create_string_buffer(8)
    assert L.zsmi_getErrorCode(L.zsmi_compress_usingCDict(small, 8, chunks[1], len(chunks[1]), cd.handle)) == 70
    src, offs, sizes = B.batch(chunks)
    assert B.frames_of(codec.compress_host(src, offs, sizes, cdict=None), len(chunks)) == B.compress_many(codec, chunks, 3)
    cd.close()


_DEVICE_CHILD = r'''
import sys, os, ctypes
import torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import numpy as np
import _oracle as O, _dicts as X, _cdict as K, _batch as B
from zstandard_amd import BatchCodec, CompressionDict
bc = BatchCodec(0)
L = bc.L
dic = X.trained("json_records")
data = X.class_data("json_records", 3 << 20)
rng = np.random.default_rng(4)
sizes = np.concatenate([rng.integers(0, 70000, 40), [1024] * 40, [65536, 65537, 131072, 131073, 200000, 1, 0, 17]]).astype(np.uint32)
assert int(sizes.sum()) <= len(data)
src_np = np.frombuffer(data[:int(sizes.sum())], dtype=np.uint8)
so, do, bounds, total = B.ragged_device_layout(L, sizes, rng)
chunks = B.cut(src_np, so, sizes)
src = torch.from_numpy(src_np.copy()).cuda()
for level in (1, 3, 4):
    cd = CompressionDict(bc, dic, level)
    dst = torch.full((total,), B.CANARY, dtype=torch.uint8, device="cuda")
    dsz = torch.zeros(len(sizes), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    bc.compress_device(src.data_ptr(), so, sizes, dst.data_ptr(), do, dsz.data_ptr(), cdict=cd)
    bc.sync()
    host = dst.cpu().numpy(); sz = dsz.cpu().numpy().view(np.uint32)
    B.assert_only_frames_written(host, do, sz, bounds, B.CANARY, level)
    host_form = B.cut(*bc.compress_host(src_np, so, sizes, cdict=cd))
    using_dict = B.cut(*bc.compress_host(src_np, so, sizes, level, dic))
    used = 0
    for i, (f, c) in enumerate(zip(B.cut(host, do, sz), chunks)):
        assert O.decompress_using_dict(f, len(c), dic) == c, (level, i)
        assert f == host_form[i], ("host form", level, i)
        blocks = K.blocks_of(f)
        assert not any(K.uses_dictionary_tables(b) for b in blocks[1:]), (level, i)
        if K.uses_dictionary_tables(blocks[0]):
            used += 1
        else:
            assert f == using_dict[i], ("usingDict", level, i)
    assert used > 0
    cd.close()
# a context of another device is refused where there is one; NULL is the plain call at level 3
dst0 = torch.full((total,), B.CANARY, dtype=torch.uint8, device="cuda"); dst1 = dst0.clone()
s0 = torch.zeros(len(sizes), dtype=torch.int32, device="cuda"); s1 = s0.clone()
bc.compress_device(src.data_ptr(), so, sizes, dst0.data_ptr(), do, s0.data_ptr(), 3)
p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
assert L.zsmi_compressBatchDevice_usingCDict(bc.ctx, ctypes.c_void_p(src.data_ptr()), p(so), p(sizes), len(sizes), ctypes.c_void_p(dst1.data_ptr()), p(do),
                                             ctypes.c_void_p(s1.data_ptr()), None) == 0
bc.sync()
assert torch.equal(dst0, dst1) and torch.equal(s0, s1)
print("CHILD-OK")
'''


def test_device_pointer_form_stays_in_bounds():
    """zsmi_compressBatchDevice_usingCDict: canary-filled output, ragged chunks around the 64 KiB limit and over it; every frame within
    zsmi_compressBound, nothing written outside the frames; the frames of the host form; they decode under oracle D"""
    B.run_child("-c", _DEVICE_CHILD, B.ROOT)


_SUB_CHILD = r'''
import sys, os
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import numpy as np
import _oracle as O, _data as D, _dicts as X, _cdict as K, _batch as B
from zstandard_amd import BatchCodec, CompressionDict
dic = X.trained("zipf")
bc = BatchCodec()
data = D.zipf_log(16 << 20, seed_lo=4343)
rng = np.random.default_rng(22)
sizes = np.concatenate([rng.integers(0, 190000, 120), [65536] * 40, [1024] * 60, [131072] * 6]).astype(np.uint32)
rng.shuffle(sizes)
offs = B.layout(sizes)
chunks = B.cut(data, offs, sizes)
for level in (3, 1):
    cd = CompressionDict(bc, dic, level)
    frames = B.frames_of(bc.compress_host(data, offs, sizes, cdict=cd))
    using_dict = B.cut(*bc.compress_host(data, offs, sizes, level, dic))
    used = 0
    for i, (f, c) in enumerate(zip(frames, chunks)):
        assert O.decompress_using_dict(f, len(c), dic) == c, (level, i)
        blocks = K.blocks_of(f)
        assert not any(K.uses_dictionary_tables(b) for b in blocks[1:]), (level, i)
        if K.uses_dictionary_tables(blocks[0]):
            used += 1
        else:
            assert f == using_dict[i], (level, i)
    assert used > 0
    cd.close()
print("CHILD-OK")
'''


def test_sub_batches_with_a_cdict():
    """ZSMI_BLOCKS_IN_FLIGHT=64 in a child process: a mixed batch is cut in many sub-batches"""
    env = dict(os.environ, ZSMI_BLOCKS_IN_FLIGHT="64")
    B.run_child("-c", _SUB_CHILD, B.ROOT, env=env)
