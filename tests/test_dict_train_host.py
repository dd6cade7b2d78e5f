"""Dictionary training, host side: zsmi_getDictID against libzstd's ZDICT_getDictID, and the scalar model of the fastCover trainer
(tests/c/train_model.c) against libzstd's own fastCover: its content, finalized by libzstd, compresses held-out chunks within 1.03x of
ZDICT_trainFromBuffer_fastCover's dictionary at the same k, d, f (no GPU needed)."""
import pytest
import _dicts
import _train as T


def test_get_dict_id_committed_dictionaries():
    from zstandard_amd import get_dict_id
    Z = T.zdict()
    dics = [_dicts.trained(c) for c in _dicts.RECORD_CLASSES] + [_dicts.TRAINED8K]
    for dic in dics:
        want = int.from_bytes(dic[4:8], "little")
        assert get_dict_id(dic) == want
        if Z:
            assert Z.ZDICT_getDictID(dic, len(dic)) == want


def test_get_dict_id_raw_and_short():
    from zstandard_amd import get_dict_id
    dic = _dicts.TRAINED8K
    assert get_dict_id(_dicts.content_of(dic)) == 0            # raw content
    assert get_dict_id(dic[:7]) == 0                            # shorter than magic + ID
    assert get_dict_id(dic[:8]) == int.from_bytes(dic[4:8], "little")
    assert get_dict_id(b"") == 0
    assert get_dict_id(b"\x37\xa4\x30\xec" + (12345).to_bytes(4, "little")) == 12345


def test_model_builds_and_is_deterministic():
    parts = T.samples("json_records", 1 << 18)
    a = T.model_content(parts, 8192, 200, 8, 16)
    assert len(a) == 8192 and a == T.model_content(parts, 8192, 200, 8, 16)
    b = T.model_content(parts, 8192, 200, 6, 16)
    assert len(b) == 8192 and a != b
    assert T.model_content([b"abc"], 1024, 50, 8, 12) == b""     # fewer than 8 bytes: nothing


@pytest.mark.parametrize("cls", ["json_records", "binary_table"])
@pytest.mark.parametrize("k", [200, 1000])
def test_model_is_a_faithful_fastcover(cls, k):
    if not T.zdict():
        pytest.skip("libzstd (>= 1.4.5) with ZDICT is not on this machine")
    parts, held = T.samples(cls), T.held_out(cls)
    content = T.model_content(parts, 65536, k, 8, 20)
    assert len(content) == 65536
    ours = T.zstd_total(held, T.zdict_finalize(content, parts, 65536))
    theirs = T.zstd_total(held, T.zdict_fastcover(parts, 65536, k, 8, 20))
    print(cls, k, ours, theirs, ours / theirs)
    assert ours <= 1.03 * theirs
