"""CDict sets on the CPU: the mixed batch of tests/_cdict_set.py holds what the GPU test (tests/test_gpu_cdict_set.py) relies on, the
frames oracle E states for its raw-content and NO_DICT items decode under oracle D, and the set calls that need no device answer as
include/zsmi.h says."""
import ctypes
import numpy as np
import pytest
import _oracle as O
import _cdict_set as S


def test_the_batch_holds_what_it_should():
    items, M = S.deal(), S.members()
    assert S.groups_ok(items) is None
    # neighbours differ; every aligned group of 4 chunks and of 4 blocks holds two choices (restated, not by the helper's own routine)
    owner = [i for i, (c, _) in enumerate(items) for _ in range(max((len(c) + 65535) // 65536, 1))]
    for g in range(0, len(items) - 3, 4):
        assert len({ch for _, ch in items[g:g + 4]}) >= 2, g
    for g in range(0, len(owner) - 3, 4):
        assert len({items[i][1] for i in owner[g:g + 4]}) >= 2, g
    assert all(items[i][1] != items[i + 1][1] for i in range(len(items) - 1))
    # while raw members last, a group of 4 chunks holds a formatted member, a raw one and NO_DICT together
    raw_members = sum(S.kind(k) == "raw" for k in range(len(M)))
    together = sum({S.kind(ch) for _, ch in items[g:g + 4]} >= {"formatted", "raw", "none"} for g in range(0, len(items) - 3, 4))
    assert raw_members == 7 and together >= len(items) // 4 // 5, (raw_members, together)
    used = {ch for _, ch in items}
    assert used == set(range(len(M))) | {S.NO_DICT}
    assert sum(ch == S.NO_DICT for _, ch in items) == sum(ch != S.NO_DICT for _, ch in items)
    for kind in ("formatted", "raw", "none"):
        sizes = {len(c) for c, ch in items if S.kind(ch) == kind and (kind != "none" or ch == S.NO_DICT)}
        assert sizes >= set(S.SIZES_EVERY_KIND_HAS), (kind, sorted(set(S.SIZES_EVERY_KIND_HAS) - sizes))
    names = [n for n, _ in M]
    assert M[names.index("again")][1] == M[names.index(S.AGAIN_OF)][1] and M[names.index("empty")][1] == b""
    ids = [O.dict_params(d)[1] for _, d in M if d]
    assert {0, 1, 255, 256, 65535, 65536, 0xFFFFFFFF, 77} <= set(ids) and len(set(ids)) < len(ids)      # every ID field size; two members with one ID
    total = sum(len(c) for c, _ in items)
    assert 10 << 20 <= total <= 32 << 20, total


@pytest.mark.parametrize("level", [1, 3, 4])
def test_oracle_frames_decode_under_oracle_d(level):
    items, frames = S.deal(), S.oracle_frames(level)
    assert set(frames) == {i for i, (_, ch) in enumerate(items) if S.kind(ch) != "formatted"}
    for i, f in frames.items():
        c, dic = items[i][0], S.dictionary(items[i][1])
        got = O.decompress_using_dict(f, len(c), dic) if dic else O.decompress(f, len(c))
        assert got == c, (level, i, len(c))
        assert (f[4] & 3) == 0, (level, i, "a raw-content or plain frame names no dictionary")


def test_set_calls_that_need_no_device():
    from zstandard_amd import _lib
    L = _lib.lib()
    err = ctypes.c_int(-1)
    assert not L.zsmi_createCDictSet(None, None, 0, 3, ctypes.byref(err)) and err.value == 62        # init_missing
    assert not L.zsmi_createCDictSet(None, None, 0, 3, None)
    err = ctypes.c_int(-1)
    assert not L.zsmi_createCDictSet(None, None, 4097, 3, ctypes.byref(err)) and err.value == 62     # the order of the checks: ctx first
    L.zsmi_freeCDictSet(None)
    assert L.zsmi_sizeofCDictSetMembers(None) == 0
    z64, z32 = np.zeros(1, dtype=np.uint64), np.zeros(1, dtype=np.uint32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    for entry in (L.zsmi_compressBatchDevice_usingCDictSet, L.zsmi_compressBatchHost_usingCDictSet):
        assert entry(None, None, p(z64), p(z32), 1, None, p(z64), None, None, p(z32)) == 62
    import zstandard_amd
    assert zstandard_amd.NO_DICT == S.NO_DICT == 0xFFFFFFFF and zstandard_amd.CompressionDictSet
