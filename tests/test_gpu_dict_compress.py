"""Compression with a dictionary on the GPU (zsmi_compress_usingDict, zsmi_compressBatch{Host,Device}_usingDict).  Every frame must
equal oracle E's (zso_compress_usingDict, the scalar statement of the prefixed units, the dictionary's recent offsets and its ID) byte
for byte: at levels 1 - 4 and above, for raw, tiny, trained, re-offset and re-numbered dictionaries, chunk sizes around every limit
and contents aimed at the prefix rules, across plan reuse, through device pointers and in sub-batches.  The frames must also decode to
their input with the same dictionary under oracle D, under the library's own decoder and under upstream libzstd; the dictionary must
really be used (ratio, dictID, recent offsets); corrupted dictionaries are refused as oracle D refuses them; no dictionary gives exactly
the frames of the calls without one.  Dictionaries and chunks: tests/_dicts.py; batches and round trips: tests/_batch.py."""
import ctypes, os
import numpy as np
import pytest
import _oracle as O
import _data as D
import _corpus as C
import _dicts as X
import _batch as B

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def codec():
    from zstandard_amd import BatchCodec
    return BatchCodec(0)


def dictionaries():
    raw = D.zipf_log(200000, seed_lo=0x515).tobytes()
    jraw = C.json_records(120000, seed=303)
    return {"trained8k": X.TRAINED8K, "trained64k_json": X.trained("json_records"), "raw6000": raw[:6000], "raw65536": jraw[:65536],
            "raw100k": jraw[:100000], "raw5": raw[:5]}


# ------------------------------------------------------------------ round trip
@pytest.mark.parametrize("level", [1, 3, 4])
def test_round_trip(codec, level):
    """six classes x chunk sizes 300 B .. 64 KiB (prefixed units) and 65537 / 200 KiB (no references into the dictionary), six dictionaries"""
    classes = ["json_records", "csv_records", "xml_records", "zipf", "binary_table", "repetitive"]
    for name, dic in dictionaries().items():
        chunks = []
        for k, cls in enumerate(classes):
            data = X.class_data(cls)
            for j, cs in enumerate((300, 1024, 4096, 16384, 65536)):
                o = (k * 7919 + j * 40009) % (len(data) - cs)
                chunks.append(data[o:o + cs])
        big = X.class_data("json_records")
        chunks += [big[1000:1000 + 65537], X.class_data("zipf")[5000:5000 + 200 * 1024], b"", b"x"]
        frames = B.compress_many(codec, chunks, level, dic)
        B.assert_round_trip(codec, frames, chunks, dic)


# ------------------------------------------------------------------ byte for byte: oracle E
def assert_matches_oracle(codec, chunks, level, dic, what):
    """the HIP frames of one batch call (BatchCodec.compress_host) against oracle E's batch form, frame by frame"""
    frames = B.compress_many(codec, chunks, level, dic)
    expect = B.oracle_frames(chunks, level, dic)
    for i, (f, e) in enumerate(zip(frames, expect)):
        assert f == e, (what, level, i, len(chunks[i]), len(f), len(e), B.first_difference(f, e))
    return frames


@pytest.mark.parametrize("level", [1, 2, 3, 4, 7])
def test_frames_match_oracle(codec, level):
    """levels 1 - 4 and 7 (every row of the LZ shape table and the level-to-class mapping) x every dictionary kind
    (tests/_dicts.py: raw content of 1 - 100 000 bytes, the trained ones, other recent offsets) x chunk sizes 0 .. 200 KiB around every
    limit, every corpus class and the prefix-rule contents; the frames also decode under oracle D"""
    for name, dic in X.identity_dictionaries().items():
        chunks = X.prefix_chunks(dic)
        frames = assert_matches_oracle(codec, chunks, level, dic, name)
        for i, (f, c) in enumerate(zip(frames, chunks)):
            assert O.decompress_using_dict(f, len(c), dic) == c, (name, i)


def test_dictionary_ids_match_oracle(codec):
    """the 8 KiB trained dictionary with IDs 0, 1, 255, 256, 65535, 65536 and 0xFFFFFFFF: every header field size"""
    chunks = X.prefix_chunks(X.TRAINED8K, (0, 1, 17, 255, 4096, 65535, 65536, 65537, 65791, 65792, 131073))
    for did, dic in X.id_dictionaries().items():
        for level in (1, 3):
            frames = assert_matches_oracle(codec, chunks, level, dic, did)
            size = 0 if did == 0 else (1 if did < 256 else (2 if did < 65536 else 4))
            assert all(f[4] & 3 == (3 if size == 4 else size) and int.from_bytes(f[5:5 + size], "little") == did for f in frames)


def test_plan_reuse_matches_oracle(codec):
    """one chunk layout called again and again on one context: no dictionary, dictionary A, dictionary B with another prefix length,
    no dictionary again, A again - the cached CompressPlan and its dictionary unit list, the table images rebuilt every call"""
    a, b = X.identity_dictionaries()["trained64k_zipf"], X.identity_dictionaries()["raw6000"]
    chunks = X.prefix_chunks(X.identity_dictionaries()["raw65536"])
    for level in (3, 1):
        for name, dic in (("none", b""), ("A", a), ("B", b), ("none", b""), ("A", a)):
            if dic:
                assert_matches_oracle(codec, chunks, level, dic, name)
            else:
                assert B.compress_many(codec, chunks, level) == B.oracle_frames(chunks, level), (name, level)


# ------------------------------------------------------------------ the dictionary is used
def test_trained_dictionary_shrinks_small_chunks(codec):
    for cls in ("json_records", "xml_records", "zipf"):
        data, dic = X.class_data(cls), X.trained(cls)
        for cs in (1024, 4096):
            chunks = [data[i:i + cs] for i in range(0, 256 * 1024, cs)]
            with_d = sum(len(f) for f in B.compress_many(codec, chunks, 3, dic))
            without = sum(len(f) for f in B.compress_many(codec, chunks, 3))
            assert with_d <= 0.9 * without, (cls, cs, with_d / without)


def test_frames_need_their_dictionary(codec):
    data, dic = X.class_data("json_records"), X.trained("json_records")
    chunks = [data[i:i + 4096] for i in range(0, 64 * 4096, 4096)]
    frames = B.compress_many(codec, chunks, 3, dic)
    dict_id = int.from_bytes(dic[4:8], "little")
    for f in frames:                                                      # the ID in every header (FHD's dictionary-ID field)
        did = f[4] & 3
        assert did and int.from_bytes(f[5:5 + (4 if did == 3 else did)], "little") == dict_id
    wrong = 0
    for f, c in zip(frames, chunks):
        try:
            wrong += O.decompress(f, len(c)) != c
        except O.OracleError:
            wrong += 1
        with pytest.raises(O.OracleError) as e:                           # another formatted dictionary: dictionary_wrong
            O.decompress_using_dict(f, len(c), X.TRAINED8K)
        assert e.value.code == 32
    assert wrong > 0
    # raw content: no ID, but the frames reach into it
    raw = dictionaries()["raw65536"]
    frames = B.compress_many(codec, chunks, 3, raw)
    assert all(f[4] & 3 == 0 for f in frames)
    bad = 0
    for f, c in zip(frames, chunks):
        try:
            bad += O.decompress(f, len(c)) != c
        except O.OracleError:
            bad += 1
    assert bad > 0


def test_first_block_starts_from_the_dictionarys_recent_offsets(codec):
    """a dictionary whose recent offsets are not {1, 4, 8}: chunks whose first sequences repeat at offsets 1, 4 and 8 decode right only if
    the encoder's repcodes start from the dictionary's offsets"""
    base = X.trained("json_records")
    assert base[-len(X.content_of(base)) - 12:-len(X.content_of(base))] == bytes([1, 0, 0, 0, 4, 0, 0, 0, 8, 0, 0, 0])   # ZDICT's defaults
    rng = np.random.default_rng(3)
    chunks = []
    for period in (1, 4, 8, 4, 8, 1):
        for lead in (0, 1, 3, 17):
            head = rng.integers(0, 256, lead, dtype=np.uint8).tobytes()
            unit = rng.integers(0, 256, period, dtype=np.uint8).tobytes()
            tail = rng.integers(0, 256, 64, dtype=np.uint8).tobytes()
            chunks.append(head + unit * (200 // period) + tail + unit * 4 + tail[:8] + unit * 10)
    for reps in ((4, 8, 1), (8, 1, 4), (2, 3, 5), (1000, 40000, 7)):
        dic = X.with_reps(base, reps)
        for level in (1, 3, 4):
            frames = B.compress_many(codec, chunks, level, dic)
            B.assert_round_trip(codec, frames, chunks, dic)


@pytest.mark.parametrize("level", [1, 3])
def test_every_frame_kind_takes_offsets_and_id_from_the_dictionary_record(codec, level):
    """one call over an empty chunk, a one-block chunk (the literals kernel writes its frame) and chunks of two and three blocks
    (k_assemble_frames), with a formatted dictionary whose recent offsets are not {1, 4, 8} and whose ID is not 0: oracle E's frames.  The
    same chunks through a CompressionDict and through a set of it and a raw-content one, chosen 0, 1, NO_DICT, 0: every chunk gets the frame
    of the call with its dictionary alone"""
    from zstandard_amd import CompressionDict, CompressionDictSet, NO_DICT
    dic = X.with_reps(X.trained("json_records"), (2, 3, 5))
    assert int.from_bytes(dic[4:8], "little") != 0
    raw = dictionaries()["raw6000"]
    data = X.class_data("json_records")
    chunks = [b"", data[5000:6000], data[70000:70000 + 65537], data[200000:200000 + 140000]]
    frames = assert_matches_oracle(codec, chunks, level, dic, "by bytes")
    B.assert_round_trip(codec, frames, chunks, dic)
    cd, cd_raw = CompressionDict(codec, dic, level), CompressionDict(codec, raw, level)
    digested = B.compress_many(codec, chunks, cdict=cd)
    B.assert_round_trip(codec, digested, chunks, dic)
    with_raw, plain = B.compress_many(codec, chunks, cdict=cd_raw), B.compress_many(codec, chunks, level)
    assert with_raw == B.oracle_frames(chunks, level, raw) and plain == B.oracle_frames(chunks, level)
    src, offs, sizes = B.batch(chunks)
    index = np.array([0, 1, NO_DICT, 0], dtype=np.uint32)
    mixed = B.frames_of(codec.compress_host(src, offs, sizes, cdict_set=CompressionDictSet(codec, [cd, cd_raw], level), dict_index=index), len(chunks))
    assert mixed == [digested[0], with_raw[1], plain[2], digested[3]]


# ------------------------------------------------------------------ errors
def test_corrupted_dictionaries_are_refused(codec):
    L = codec.L
    data = X.class_data("json_records")[:4096]
    for d in X.bad_dictionaries():
        with pytest.raises(O.OracleError) as e:                           # what oracle D says of the same dictionary
            O.decompress_using_dict(O.compress(data, 3), len(data), d)
        assert e.value.code == 30
        out = ctypes.create_string_buffer(L.zsmi_compressBound(len(data)))
        r = L.zsmi_compress_usingDict(out, len(out), data, len(data), d, len(d), 3)
        assert L.zsmi_getErrorCode(r) == 30
        with pytest.raises(RuntimeError, match="error 30"):
            B.compress_many(codec, [data, data[:100]], 3, d)


# ------------------------------------------------------------------ equivalence
def test_no_dictionary_is_the_plain_call(codec):
    from zstandard_amd import ZstdCompressor
    L = codec.L
    data = X.class_data("zipf")
    chunks = [data[0:300], data[1000:66536], data[70000:70000 + 65537], data[200000:200000 + 150000], b""]
    for level in (1, 3, 4):
        plain = B.compress_many(codec, chunks, level)
        src, so, ss = B.batch(chunks)
        bounds = [L.zsmi_compressBound(len(c)) for c in chunks]
        do = B.layout(bounds)
        arena = np.zeros(sum(bounds), dtype=np.uint8); dsz = np.zeros(len(chunks), dtype=np.uint32)
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        for d, dn in ((None, 0), (b"abc", 0), (None, 100)):
            assert L.zsmi_compressBatchHost_usingDict(codec.ctx, p(src), p(so), p(ss), len(chunks), p(arena), p(do), p(dsz), level, d, dn) == 0
            assert B.cut(arena, do, dsz) == plain
        for c, f in zip(chunks, plain):
            out = ctypes.create_string_buffer(L.zsmi_compressBound(len(c)))
            r = L.zsmi_compress_usingDict(out, len(out), c, len(c), None, 0, level)
            assert out.raw[:r] == f
            assert ZstdCompressor(level, dictionary=b"").compress(c) == f
        for c in chunks:                                                  # oracle E: the same holds for the scalar statement
            assert O.compress_using_dict(c, None, level) == O.compress_using_dict(c, b"", level) == O.compress(c, level)
    dic = X.trained("json_records")
    c = X.class_data("json_records")[:3000]
    out = ctypes.create_string_buffer(L.zsmi_compressBound(len(c)))
    r = L.zsmi_compress_usingDict(out, len(out), c, len(c), dic, len(dic), 3)
    assert not L.zsmi_isError(r) and ZstdCompressor(3, dictionary=dic).compress(c) == out.raw[:r]
    assert out.raw[:r] == B.compress_many(codec, [c], 3, dic)[0] == O.compress_using_dict(c, dic, 3)
    assert O.decompress_using_dict(out.raw[:r], len(c), dic) == c


# ------------------------------------------------------------------ device calls: bounds, errors, sub-batches (child processes: torch first)
_DEVICE_CHILD = r'''
import sys, os, ctypes
import torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import numpy as np
import _oracle as O, _corpus as C, _dicts as X, _batch as B
from zstandard_amd import BatchCodec
bc = BatchCodec(0)
L = bc.L
data = C.json_records(3 << 20, seed=99)
rng = np.random.default_rng(4)
sizes = np.concatenate([rng.integers(0, 70000, 40), [65536, 65537, 131072, 131073, 200000, 1, 0, 17]]).astype(np.uint32)
assert int(sizes.sum()) <= len(data)
src_np = np.frombuffer(data[:int(sizes.sum())], dtype=np.uint8)
so, do, bounds, total = B.ragged_device_layout(L, sizes, rng)
chunks = B.cut(src_np, so, sizes)
src = torch.from_numpy(src_np.copy()).cuda()
for name, dic in (("trained", X.trained("json_records")), ("raw", data[500000:600000])):
    ddict = torch.from_numpy(np.frombuffer(dic, dtype=np.uint8).copy()).cuda()
    for level in (1, 3, 4):
        dst = torch.full((total,), B.CANARY, dtype=torch.uint8, device="cuda")
        dsz = torch.zeros(len(sizes), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        bc.compress_device(src.data_ptr(), so, sizes, dst.data_ptr(), do, dsz.data_ptr(), level, ddict.data_ptr(), len(dic))
        bc.sync()
        host = dst.cpu().numpy(); sz = dsz.cpu().numpy().view(np.uint32)
        B.assert_only_frames_written(host, do, sz, bounds, B.CANARY, (name, level))
        frames = B.cut(host, do, sz)
        for i, (f, c, e) in enumerate(zip(frames, chunks, B.oracle_frames(chunks, level, dic))):
            assert O.decompress_using_dict(f, len(c), dic) == c, (name, level, i)
            assert f == e, ("oracle E", name, level, i)
        # the host form gives the same frames
        arena, hdo, hsz = bc.compress_host(src_np, so, sizes, level, dic)
        assert (hsz == sz).all() and B.cut(arena, hdo, hsz) == frames
    # NULL / 0 bytes: the plain call
    dst0 = torch.full((total,), B.CANARY, dtype=torch.uint8, device="cuda"); dst1 = dst0.clone()
    s0 = torch.zeros(len(sizes), dtype=torch.int32, device="cuda"); s1 = s0.clone()
    bc.compress_device(src.data_ptr(), so, sizes, dst0.data_ptr(), do, s0.data_ptr(), 3)
    bc.compress_device(src.data_ptr(), so, sizes, dst1.data_ptr(), do, s1.data_ptr(), 3, ddict.data_ptr(), 0)
    bc.sync()
    assert torch.equal(dst0, dst1) and torch.equal(s0, s1)
# corrupted dictionaries: 30 before anything runs
dst = torch.zeros(total, dtype=torch.uint8, device="cuda"); dsz = torch.zeros(len(sizes), dtype=torch.int32, device="cuda")
p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
for d in X.bad_dictionaries():
    dd = torch.from_numpy(np.frombuffer(d, dtype=np.uint8).copy()).cuda()
    rc = L.zsmi_compressBatchDevice_usingDict(bc.ctx, ctypes.c_void_p(src.data_ptr()), p(so), p(sizes), len(sizes), ctypes.c_void_p(dst.data_ptr()), p(do),
                                              ctypes.c_void_p(dsz.data_ptr()), 3, ctypes.c_void_p(dd.data_ptr()), len(d))
    assert rc == 30, rc
print("CHILD-OK")
'''


def test_device_calls_stay_in_bounds_and_refuse_bad_dictionaries():
    """zsmi_compressBatchDevice_usingDict: canary-filled output, ragged chunks around the 64 KiB limit; every frame within
    zsmi_compressBound and nothing written outside the frames; frames equal to the host form's and oracle E's and decode under oracle D; a NULL /
    0-byte dictionary is the plain call; corrupted dictionaries return 30"""
    B.run_child("-c", _DEVICE_CHILD, B.ROOT)


_SUB_CHILD = r'''
import sys, os
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import numpy as np
import _oracle as O, _data as D, _dicts as X, _batch as B
from zstandard_amd import BatchCodec
dic = X.trained("zipf")
bc = BatchCodec()
data = D.zipf_log(16 << 20, seed_lo=4343)
rng = np.random.default_rng(22)
sizes = np.concatenate([rng.integers(0, 190000, 120), [65536] * 40, [1024] * 60, [131072] * 6]).astype(np.uint32)
rng.shuffle(sizes)
offs = B.layout(sizes)
chunks = B.cut(data, offs, sizes)
for level in (3, 1):
    frames = B.frames_of(bc.compress_host(data, offs, sizes, level, dic))
    expect = B.cut(*O.compress_batch_using_dict(data, offs, sizes, dic, level, 8))
    for i, (f, c, e) in enumerate(zip(frames, chunks, expect)):
        assert O.decompress_using_dict(f, len(c), dic) == c, (level, i)
        assert f == e, ("oracle E", level, i)
    assert [sz for sz, _ in B.decode_many(bc, frames, sizes, dic)] == sizes.tolist()
print("CHILD-OK")
'''


def test_sub_batches_with_a_dictionary():
    """ZSMI_BLOCKS_IN_FLIGHT=64 in a child process: a mixed batch (prefixed units, tails of long chunks, big units) is cut in many
    sub-batches; every frame equals oracle E's and round-trips"""
    env = dict(os.environ, ZSMI_BLOCKS_IN_FLIGHT="64")
    B.run_child("-c", _SUB_CHILD, B.ROOT, env=env)


# ------------------------------------------------------------------ ratio contract
def test_ratio_against_libzstd_with_the_same_dictionary(codec):
    """level 3, chunks of 1 / 4 / 16 KiB: <= 1.03 x libzstd with the same raw-content dictionary (the trained dictionary's content);
    <= 1.10 x libzstd with the trained dictionary at >= 4 KiB, <= 1.25 x at 1 KiB (libzstd also uses its tables, this encoder does not)"""
    if not X.zstd():
        pytest.skip("libzstd not available")
    table = {}
    for cls in X.RECORD_CLASSES:
        data, dic = X.class_data(cls), X.trained(cls)
        raw = X.content_of(dic)
        assert len(raw) <= 65536
        for cs in (1024, 4096, 16384):
            chunks = [data[i:i + cs] for i in range(0, 256 * 1024, cs)]
            ours_raw = sum(len(f) for f in B.compress_many(codec, chunks, 3, raw))
            ours_tr = sum(len(f) for f in B.compress_many(codec, chunks, 3, dic))
            z_raw = sum(len(X.zstd_compress_dict(c, raw, 3)) for c in chunks)
            z_tr = sum(len(X.zstd_compress_dict(c, dic, 3)) for c in chunks)
            table[(cls, cs)] = (round(ours_raw / z_raw, 3), round(ours_tr / z_tr, 3))
    print(table)
    assert all(v[0] <= 1.03 for v in table.values()), table
    assert all(v[1] <= (1.25 if cs == 1024 else 1.10) for (cls, cs), v in table.items()), table
