"""A whole training call against its reference, byte for byte: tests/_train.py states the reference once (reference_train: the model's
content over the training share, oracle E's held-out totals as scores, the smallest total then the smaller k then the smaller d, oracle
E's finalize over all samples).  zsmi_trainFromBuffer_fastCover and zsmi_trainFromDevice must return exactly that dictionary and that
(k, d): over the search (tests/_dictfin.py: SEARCH - k, d or both searched, the splits, one and three samples, both levels, and f = 26,
whose ten candidates take two groups of frequency tables) and over the borders of k_train_select with k and d fixed (SELECT).  That each
case reaches its border is shown without a GPU by tests/test_dict_finalize_host.py.

f = 26 (two_groups_f26): ten candidates, eight 256 MiB frequency tables to a group, so two groups.  The model's two 256 MiB tables cost the
CPU side 1.3 s for the ten candidates (measured), which a test can afford, so the group path is held at f = 26 itself."""
import ctypes
import numpy as np
import pytest
import _train as T
import _dictfin as F
from _hip import hip_of, Dev

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def codec():
    from zstandard_amd import BatchCodec
    return BatchCodec(0)


def L():
    from zstandard_amd import _lib
    return _lib.lib()


def gpu_train(parts, cap, k=0, d=0, f=0, steps=0, split=0.0, level=0, dict_id=0):
    """(the dictionary or the error's code - the destination and the parameters checked untouched -, k, d)"""
    from zstandard_amd import _lib
    p = _lib.FastCoverParams(k=k, d=d, f=f, steps=steps, accel=0, splitPoint=split, level=level, dictID=dict_id)
    buf, sizes = T.flat(parts)
    out = ctypes.create_string_buffer(b"\xAA" * cap, cap)
    r = L().zsmi_trainFromBuffer_fastCover(out, cap, buf, sizes, len(parts), ctypes.byref(p))
    if L().zsmi_isError(r):
        assert out.raw == b"\xAA" * cap and (p.k, p.d) == (k, d)
        return int(L().zsmi_getErrorCode(r)), p.k, p.d
    return out.raw[:r], p.k, p.d


def same(got, want):
    (gd, gk, gdd), (wd, wk, wdd) = got, want[:3]
    assert (gk, gdd) == (wk, wdd), f"chose k {gk} d {gdd}, the reference k {wk} d {wdd} (scores {want[4]})"
    if isinstance(gd, bytes) and isinstance(wd, bytes) and gd != wd:
        at = next((i for i, (a, b) in enumerate(zip(gd, wd)) if a != b), min(len(gd), len(wd)))
        raise AssertionError(f"sizes {len(gd)} / {len(wd)}, first difference at byte {at} (the reference's content starts at {len(wd) - len(want[3])})")
    assert gd == wd


@pytest.mark.parametrize("case", sorted(F.SEARCH))
def test_search_equals_reference(case):
    parts, cap, kw = F.SEARCH[case]()
    same(gpu_train(parts, cap, **kw), F.search_reference(case))


def test_device_form_equals_reference(codec):
    """the samples in reverse order behind 4 KiB of other bytes, named by their offsets"""
    case = "k_searched"
    parts, cap, kw = F.SEARCH[case]()
    rev = b"".join(reversed(parts))
    dev = Dev(hip_of(), len(rev), rev)
    try:
        sizes = np.array([len(x) for x in parts], dtype=np.uint32)
        ends = np.cumsum(sizes[::-1].astype(np.uint64))[::-1]
        offs = (ends - sizes).astype(np.uint64)
        got = codec.train_device(dev.p, offs, sizes, cap, k=kw["k"], d=kw["d"], steps=kw["steps"])
    finally:
        dev.free()
    same(got, F.search_reference(case))


@pytest.mark.parametrize("case", sorted(F.SELECT))
def test_selection_border_equals_reference(case):
    parts, cap, k, d, f = F.SELECT[case]()
    want = F.select_reference(case)
    got = gpu_train(parts, cap, k=k, d=d, f=f, split=1.0, level=3)
    same(got, want)
    content = T.check_format(got[0], cap)
    assert want[3].endswith(content) and len(content) == min(len(want[3]), cap - (len(got[0]) - len(content)))     # the model's content, cut only by cap
