"""Record archives with device-resident sizes and frame numbers, what holds without a device: the four names in the header, _lib.EXPORTS and
the library; zsmi_seekableFramesResidentBound against zsmi_seekableFramesBound of the splits it must cover, its refusals; the NULL-ctx
refusal of the three device calls in front of every other check."""
import ctypes, os, re
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("zsmi_seekableFramesResidentBound", "zsmi_compressSeekableFramesResident", "zsmi_compressSeekableFramesResident_usingCDictSet",
         "zsmi_seekableReadFramesResident")
E_GENERIC, E_INIT_MISSING, E_OUT_OF_BOUND, E_FRAME_INDEX = 1, 62, 42, 100
GIB = 1 << 30


@pytest.fixture(scope="module")
def L():
    from zstandard_amd import _lib
    return _lib.lib()


def test_names_in_header_exports_and_library(L):
    from zstandard_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "zsmi.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(zsmi_[A-Za-z0-9_]+)\s*\(", hdr))
    for name in NAMES:
        assert name in declared and name in _lib.EXPORTS and hasattr(L, name), name


def frames_bound(L, sizes, flag):
    fs = np.ascontiguousarray(sizes, dtype=np.uint32)
    r = L.zsmi_seekableFramesBound(fs.ctypes.data_as(ctypes.c_void_p) if len(fs) else None, len(fs), flag)
    assert not L.zsmi_isError(r), sizes
    return r


def splits():
    rng = np.random.default_rng(23)
    out = [[], [0], [0] * 7, [1], [5000000], [0, 0, 123456789, 0]]
    edges = [65535, 65536, 65537, 131071, 131072, 131073]
    out += [[e] for e in edges] + [edges, edges[::-1], edges * 3 + [0, 1]]
    out += [[GIB], [GIB] * 5]
    for n in (1, 2, 17, 300):
        for hi in (10, 4096, 70000, 200000, 3000000):
            out.append([int(v) for v in rng.integers(0, hi + 1, n)])
    for n in (3, 50):                                          # sizes just under and over each term's step: 256 bytes, 2 KiB, 64 KiB
        out.append([int(k * 256 + d) for k, d in zip(rng.integers(0, 600, n), rng.integers(-1, 2, n) % 256)])
        out.append([int(k * 65536 - 1) for k in rng.integers(1, 40, n)])
        out.append([int(131072 - 2048 * k - 1) for k in rng.integers(0, 64, n)])
    return out


@pytest.mark.parametrize("flag", (0, 1))
def test_bound_covers_every_split(L, flag):
    for sizes in splits():
        total, n = sum(sizes), len(sizes)
        r = L.zsmi_seekableFramesResidentBound(total, n, flag)
        assert not L.zsmi_isError(r), (total, n)
        assert r >= frames_bound(L, sizes, flag), (sizes[:8], n, flag)
        # the stated expression, term by term over zsmi_compressBound
        assert r == total + (total >> 8) + 3 * (total >> 16) + n * (64 + 3 + 18) + 17 + n * (12 if flag else 8)
    assert L.zsmi_seekableFramesResidentBound(0, 0, flag) == 17


def test_bound_refusals(L):
    code = lambda r: L.zsmi_getErrorCode(r) if L.zsmi_isError(r) else 0
    B = L.zsmi_seekableFramesResidentBound
    assert code(B(0, 0x8000001, 1)) == E_FRAME_INDEX and code(B(1 << 62, 0x8000001, 0)) == E_FRAME_INDEX      # the count first
    assert code(B(0, 0x8000000, 1)) == 0
    assert code(B(1, 0, 1)) == E_OUT_OF_BOUND                                      # content and no frame to hold it
    assert code(B(GIB + 1, 1, 0)) == E_OUT_OF_BOUND and code(B(GIB, 1, 0)) == 0
    assert code(B(7 * GIB + 1, 7, 1)) == E_OUT_OF_BOUND and code(B(7 * GIB, 7, 1)) == 0


def test_null_ctx_comes_first(L):
    """every other argument wrong as well: init_missing all the same, and nothing is dereferenced"""
    assert L.zsmi_compressSeekableFramesResident(None, None, 5, None, 0x8000001, (1 << 30) + 1, None, 0, None, 3, 1) == E_INIT_MISSING
    assert L.zsmi_compressSeekableFramesResident_usingCDictSet(None, None, 5, None, 0x8000001, (1 << 30) + 1, None, 0, None, 1, None, None) == E_INIT_MISSING
    assert L.zsmi_seekableReadFramesResident(None, None, None, 3, 3, None, 10, None, None, None) == E_INIT_MISSING
