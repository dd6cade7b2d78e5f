"""The hand-built dictionary frames of tests/_ddict.py under oracle D (CPU): every valid frame gives its intended bytes, every invalid one
its intended code.  This pins the fixtures that tests/test_gpu_ddict.py decodes with a digested dictionary (zsmi_createDDict) where they can
be checked without a GPU; the dictionaries themselves must be ones oracle D loads."""
import pytest
import _oracle as O
import _ddict as DD
import _framewriter as W


def test_the_dictionaries_load():
    for name, dic in DD.dictionaries().items():
        off, did, reps = O.dict_params(dic)
        if name == "raw":
            assert (off, did, reps) == (0, 0, (1, 4, 8))
        else:
            assert did == DD.DICT_ID and dic[off:] == DD.CONTENT, name
            assert reps == ((7, 33, 120) if name == "reps" else (1, 4, 8)), name


def test_huffman_table_classes():
    """the wide dictionary's table needs more sub-tables than the two-level form has (32) at 11 bits; the log12 one is 12 bits"""
    assert DD.long_prefixes(DD.wide_lengths()) > 32 and max(DD.wide_lengths().values()) == 11
    assert max(DD.log12_lengths().values()) == 12
    assert DD.long_prefixes(W.flat_lengths(DD.ALPHABET)) == 0


def test_every_letter_of_the_catalogue_is_there():
    letters = {name[0] for name, *_ in DD.cases()}
    assert letters >= set("abcdefghijkl"), sorted(letters)


@pytest.mark.parametrize("case", DD.cases(), ids=[c[0] for c in DD.cases()])
def test_frame_under_oracle_d(case):
    name, dname, frame, content, code = case
    dic = DD.dictionaries()[dname]
    if code:
        with pytest.raises(O.OracleError) as e:
            O.decompress_using_dict(frame, 4096, dic)
        assert e.value.code == code, (name, e.value.code)
    else:
        assert O.decompress_using_dict(frame, len(content), dic) == content, name
        assert O.decompress_using_dict(frame, len(content) + 100, dic) == content, name


def test_frames_need_their_dictionary():
    """the frames that reach into the dictionary or use its tables do not decode to their content without it"""
    needing = 0
    for name, dname, frame, content, code in DD.cases():
        if code or name[0] in "l":
            continue
        try:
            got = O.decompress(frame, len(content) + 100)
        except O.OracleError:
            got = None
        needing += got != content
    assert needing >= 40
