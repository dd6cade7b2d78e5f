"""Oracle E with a dictionary (zso_compress_usingDict, zso_compressBatch_usingDict: the scalar statement of zsmi_compress_usingDict):
its frames decode under oracle D and libzstd with the same dictionary; no dictionary is the plain call; the ID is written at every field
size; dictionaries D refuses are refused with 30; nothing in front of the content's last 64 KiB is referenced; the ratio contract against
libzstd with the same dictionary.  CPU only."""
import numpy as np
import pytest
import _oracle as O
import _dicts as X
import _batch as B

SIZES = (0, 1, 7, 8, 16, 17, 255, 256, 1024, 4096, 65535, 65536, 65537, 65792, 131073)


def assert_decodes(frames, chunks, dic, what):
    for i, (f, c) in enumerate(zip(frames, chunks)):
        assert len(f) <= O.lib().zso_compressBound(len(c)), (what, i)
        assert O.decompress_using_dict(f, len(c), dic) == c, ("oracle D", what, i, len(c))
        if X.zstd():
            assert X.zstd_decompress_dict(f, len(c), dic) == c, ("libzstd", what, i, len(c))


@pytest.mark.parametrize("level", [1, 3, 4])
def test_round_trip(level):
    """every dictionary kind x chunk sizes around every limit, every corpus class, contents aimed at the prefix rules"""
    for name, dic in X.identity_dictionaries().items():
        chunks = X.prefix_chunks(dic, SIZES)
        frames = B.oracle_frames(chunks, level, dic)
        assert_decodes(frames, chunks, dic, name)
        assert frames[3] == O.compress_using_dict(chunks[3], dic, level)           # the one-shot form is the batch form


def test_no_dictionary_is_the_plain_call():
    chunks = X.prefix_chunks(X.TRAINED8K, SIZES)
    src, offs, sizes = B.batch(chunks)
    for level in (1, 3):
        plain = B.cut(*O.compress_batch(src, offs, sizes, level, 4))
        for d in (None, b""):
            assert B.cut(*O.compress_batch_using_dict(src, offs, sizes, d, level, 4)) == plain
            assert all(O.compress_using_dict(c, d, level) == f for c, f in zip(chunks, plain))


def test_dictionary_id_at_every_field_size():
    chunks = [X.STREAM[:300], X.STREAM[1000:1000 + 70000], b"", X.STREAM[:65536]]
    for did, dic in X.id_dictionaries().items():
        size = 0 if did == 0 else (1 if did < 256 else (2 if did < 65536 else 4))
        for f, c in zip(B.oracle_frames(chunks, 3, dic), chunks):
            assert f[4] & 3 == (3 if size == 4 else size)
            assert int.from_bytes(f[5:5 + size], "little") == did
            assert O.decompress_using_dict(f, len(c), dic) == c
            if did:
                with pytest.raises(O.OracleError) as e:                     # another ID: dictionary_wrong
                    O.decompress_using_dict(f, len(c), X.with_id(dic, did ^ 1))
                assert e.value.code == 32


def test_refused_dictionaries():
    data = X.STREAM[:4096]
    src, offs, sizes = B.batch([data, data[:100]])
    for d in X.bad_dictionaries():
        with pytest.raises(O.OracleError) as e:
            O.compress_using_dict(data, d, 3)
        assert e.value.code == 30
        with pytest.raises(O.OracleError) as e:
            O.compress_batch_using_dict(src, offs, sizes, d, 3, 2)
        assert e.value.code == 30


def test_only_the_last_64k_of_the_content_is_referenced():
    """frames made with content of 100 000 bytes decode the same with the bytes in front of its last 64 KiB replaced: the prefix is the
    last 64 KiB (and chunks > 64 KiB reference no dictionary bytes at all)"""
    for dic in (X.identity_dictionaries()["raw100000"], X.identity_dictionaries()["reps_70000_content100k"]):
        off = O.dict_params(dic)[0]
        other = dic[:off] + bytes(len(dic) - off - 65536) + dic[-65536:]
        chunks = X.prefix_chunks(dic, SIZES)
        for level in (1, 3):
            for f, c in zip(B.oracle_frames(chunks, level, dic), chunks):
                assert O.decompress_using_dict(f, len(c), other) == c
        cut = [c for c in chunks if len(c) > 65536]
        for f, c in zip(B.oracle_frames(cut, 3, dic), cut):
            assert O.decompress_using_dict(f, len(c), dic[:off] + bytes(len(dic) - off)) == c


def test_first_block_starts_from_the_dictionarys_recent_offsets():
    """chunks whose first sequences repeat at offsets 1, 4, 8 under dictionaries whose recent offsets are not {1, 4, 8}: they decode
    only if stage 3b starts from the dictionary's offsets"""
    rng = np.random.default_rng(3)
    chunks = []
    for period in (1, 4, 8):
        for lead in (0, 1, 17):
            unit = rng.integers(0, 256, period, dtype=np.uint8).tobytes()
            tail = rng.integers(0, 256, 64, dtype=np.uint8).tobytes()
            chunks.append(rng.integers(0, 256, lead, dtype=np.uint8).tobytes() + unit * (200 // period) + tail + unit * 4 + tail[:8] + unit * 10)
    chunks.append(X.STREAM[:70000] + X.STREAM[:70000])
    for reps in ((4, 8, 1), (8, 1, 4), (2, 3, 5), (1000, 40000, 7)):
        dic = X.with_reps(X.trained("json_records"), reps)
        for level in (1, 3, 4):
            assert_decodes(B.oracle_frames(chunks, level, dic), chunks, dic, reps)


@pytest.mark.skipif(not X.zstd(), reason="libzstd not present")
def test_ratio_against_libzstd_with_the_same_dictionary():
    """level 3, chunks of 1 / 4 / 16 KiB: <= 1.03 x libzstd with the same raw-content dictionary (the trained dictionary's content);
    <= 1.10 x libzstd with the trained dictionary at >= 4 KiB, <= 1.25 x at 1 KiB (libzstd also uses its tables, this encoder does not)"""
    table = {}
    for cls in X.RECORD_CLASSES:
        data, dic = X.class_data(cls), X.trained(cls)
        raw = X.content_of(dic)
        for cs in (1024, 4096, 16384):
            chunks = [data[i:i + cs] for i in range(0, 256 * 1024, cs)]
            ours_raw = sum(len(f) for f in B.oracle_frames(chunks, 3, raw))
            ours_tr = sum(len(f) for f in B.oracle_frames(chunks, 3, dic))
            z_raw = sum(len(X.zstd_compress_dict(c, raw, 3)) for c in chunks)
            z_tr = sum(len(X.zstd_compress_dict(c, dic, 3)) for c in chunks)
            table[(cls, cs)] = (round(ours_raw / z_raw, 3), round(ours_tr / z_tr, 3))
    assert all(v[0] <= 1.03 for v in table.values()), table
    assert all(v[1] <= (1.25 if cs == 1024 else 1.10) for (cls, cs), v in table.items()), table
