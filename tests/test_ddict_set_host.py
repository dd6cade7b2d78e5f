"""The mixed batch of tests/_ddict_set.py under oracle D (CPU): every item, decoded frame by frame with the dictionary the DDict-set rule
picks for it, gives the content or the code the helper states - for every set tests/test_gpu_ddict_set.py decodes it with.  This pins the
fixtures before any GPU sees them.  And the part of the set's C ABI that needs no device."""
import ctypes
import pytest
import _oracle as O
import _ddict as DD
import _ddict_set as S
import _framewriter as W


def test_the_dictionaries_load_under_their_ids():
    D = S.dictionaries()
    assert len(D) == 4 + S.N_SMALL + 1
    ids = set()
    for name, dic in D.items():
        off, did, reps = O.dict_params(dic)
        assert did == S.dict_id(dic) and (did == 0) == (name == "raw"), name
        ids.add(did)
        if name.startswith("small"):
            content, want_reps = S.small_parts(int(name[5:]))
            assert dic[off:] == content and reps == want_reps, name
    assert set(S.EDGE_IDS) < ids and len(ids) == len(D)
    widths = {1 if i < 256 else 2 if i < 65536 else 4 for i in ids if i}
    assert widths == {1, 2, 4}
    order = S.member_order()
    assert sorted(order) == sorted(n for n in D if n != "raw")


def test_renamed_frames_differ_only_in_the_id_field():
    want = {c[0]: c for c in DD.cases()}
    renamed = 0
    for it in S.items():
        if it["name"] not in want or it["cut"]:
            continue
        old, new = want[it["name"]][2], it["frames"][0]
        at, n = S.id_field(old)
        at2, n2 = S.id_field(new)
        assert old[:4] == new[:4] and old[at + n:] == new[at2 + n2:] and (old[4] | 3) == (new[4] | 3), it["name"]
        assert n2 == (n or (1 if new != old else 0)), it["name"]
        assert [(b.type, b.size) for b in W.blocks(new)] == [(b.type, b.size) for b in W.blocks(old)], it["name"]
        renamed += new != old
    assert renamed >= 50


def test_the_batch_holds_what_it_should():
    its = S.items()
    names = [it["name"] for it in its]
    assert len(set(names)) == len(names)
    assert {c[0] for c in DD.cases()} <= set(names)                               # the whole catalogue, valid and invalid
    assert sum(it["cut"] for it in its) >= 8 and sum(0 in it["ids"] for it in its) >= 20
    assert any(it["ids"] == [S.UNKNOWN_ID] for it in its) and sum(it["ids"] in ([77], [78]) for it in its) >= 4
    two = [it for it in its if not S.single_frame(it)]
    assert len(two) == 1 and len(set(two[0]["ids"])) == 2
    h = next(it for it in its if it["name"] == "h raw block, then treeless [narrow]")       # a raw first block, a second one Treeless on its dictionary's table
    first, second = W.blocks(h["frames"][0])
    assert (first.type, second.type, second.lit_type) == (0, 2, 3) and h["ids"] == [S.IDS["narrow"]]
    # neighbours name different dictionaries: every group of 2 (prep and the general kernel: ZS_DEC_GROUP), 4 (execute) and 16 items (Huffman, sequences) mixes them
    for g in (2, 4, 16):
        for at in range(0, len(its) - g + 1, g):
            assert len({tuple(it["ids"]) for it in its[at:at + g]}) >= 2, (g, at)


@pytest.mark.parametrize("config", S.configurations(), ids=["%d members, unnamed %s" % (len(m), u) for m, u in S.configurations()])
def test_items_under_oracle_d_with_the_picked_dictionary(config):
    members, unnamed = config
    stated = 0
    for it in S.items():
        got = S.oracle_item(it, members, unnamed)
        want = S.stated(it, members, unnamed)
        if want is None:
            assert got[0] <= it["cap"] or got[0] > 0xFFFFFF88, it["name"]           # a definite result either way
            continue
        content, code = want
        assert got == ((0x100000000 - code, b"") if code else (len(content), content)), (it["name"], hex(got[0]))
        stated += 1
    assert stated >= 130


def test_set_calls_that_need_no_device():
    from zstandard_amd import _lib
    L = _lib.lib()
    err = ctypes.c_int(7)
    assert not L.zsmi_createDDictSet(None, None, 0, None, ctypes.byref(err)) and err.value == 62        # init_missing
    assert not L.zsmi_createDDictSet(None, None, 0, None, None)
    L.zsmi_freeDDictSet(None)
    assert L.zsmi_sizeofDDictSetMembers(None) == 0
