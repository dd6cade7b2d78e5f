"""The host-only size queries (zsmi_getFrameContentSize, zsmi_findFrameCompressedSize, zsmi_findDecompressedSize, zsmi_decompressBound:
the container walker, csrc/zsmi_frame.h zs_walk) against libzstd's recorded answers (tests/golden/libzstd_sizes.json), against oracle D on
every prefix of a two-frame item, and on the frames the walker must refuse.  No device is needed."""
import os, struct
import pytest
import _data as D
import _framewriter as W
import _oracle as O
import _sizes as S
from zstandard_amd import _lib, api

UNKNOWN, ERROR = S.UNKNOWN, S.ERROR


@pytest.fixture(scope="module")
def L():
    _lib.build()
    return _lib.lib()


@pytest.fixture(scope="module")
def items():
    return S.items()


def first_code(L, item):
    r = L.zsmi_findFrameCompressedSize(item, len(item))
    return L.zsmi_getErrorCode(r) if L.zsmi_isError(r) else 0


def oracle_code(item, cap=1 << 16):
    """0, or the code oracle D gives the item with ample room"""
    try:
        O.decompress(item, cap)
        return 0
    except O.OracleError as e:
        return e.code


def test_constants_and_python_surface():
    assert api.CONTENTSIZE_UNKNOWN == UNKNOWN and api.CONTENTSIZE_ERROR == ERROR
    f = S.sized_frame(9, 50)
    assert api.frame_content_size(f) == 50 and api.find_frame_compressed_size(f) == len(f)
    assert api.find_decompressed_size(f + f) == 100 and api.decompress_bound(f + f) == 100
    with pytest.raises(RuntimeError, match="Unknown frame descriptor"):
        api.find_frame_compressed_size(b"garbage!")


def test_fixture_matches_its_items(items):
    rec = S.recorded()
    assert [n for n, _ in items] == list(rec)
    for name, item in items:
        assert S.sha(item) == rec[name]["sha256"], name
    # the kinds of item the fixture is there for
    names = [n for n, _ in items]
    assert sum(n.startswith("fx_") for n in names) >= 30 and sum(n.startswith("unsized_") for n in names) == 27
    assert any(r["find_decompressed_size"] == UNKNOWN for r in rec.values()) and all(r["decompress_bound"] < ERROR for r in rec.values())


def test_host_calls_equal_libzstd(L, items):
    rec = S.recorded()
    for name, item in items:
        r = rec[name]
        assert int(L.zsmi_findDecompressedSize(item, len(item))) == r["find_decompressed_size"], name
        assert int(L.zsmi_findFrameCompressedSize(item, len(item))) == r["find_frame_compressed_size"], name
        assert int(L.zsmi_decompressBound(item, len(item))) == r["decompress_bound"], name
        # the first frame's header: what libzstd sums for an item of one zstd frame; 0 for a skippable frame in front
        first = item[:r["find_frame_compressed_size"]]
        want = 0 if (struct.unpack("<I", item[:4])[0] & 0xFFFFFFF0) == 0x184D2A50 else int(L.zsmi_findDecompressedSize(first, len(first)))
        assert int(L.zsmi_getFrameContentSize(item, len(item))) == want, name
        assert S.host_answers(L, item)[2] == 0, name


def test_reference_golden_frames(L):
    for n, size in (("csharp_alphabet", 3409), ("java_a2z", 100000)):
        f = open(os.path.join(D.GOLDEN, n + ".zst"), "rb").read()
        assert L.zsmi_getFrameContentSize(f, len(f)) == size and L.zsmi_findDecompressedSize(f, len(f)) == size
        assert L.zsmi_decompressBound(f, len(f)) == size and L.zsmi_findFrameCompressedSize(f, len(f)) == len(f)


def test_first_frame_of_a_concatenation(L):
    a, b = S.sized_frame(3, 10), S.unsized_frame("16k", "rle", 5, checksum=True)
    skip = W.skippable(b"xyz")
    for first, rest in ((a, b), (b, a), (skip, a), (a, skip), (a, b"garbage behind the frame")):
        item = first + rest
        assert L.zsmi_findFrameCompressedSize(item, len(item)) == len(first)
    # the header alone: the frame's blocks need not be there
    assert L.zsmi_getFrameContentSize(a[:6], 6) == 10 and L.zsmi_getFrameContentSize(a[:5], 5) == ERROR
    assert L.zsmi_getFrameContentSize(b, len(b)) == UNKNOWN and L.zsmi_getFrameContentSize(skip, len(skip)) == 0
    assert L.zsmi_getFrameContentSize(skip[:8], 8) == 0 and L.zsmi_getFrameContentSize(skip[:7], 7) == ERROR
    assert L.zsmi_getFrameContentSize(b"", 0) == ERROR and first_code(L, b"") == 72 and first_code(L, a[:4]) == 72


def test_every_prefix_against_oracle_d(L):
    item = S.two_frame_item()
    assert oracle_code(item) == 0 and L.zsmi_findDecompressedSize(item, len(item)) == 21 + 34
    cut_in_checksum = []
    for n in range(len(item)):
        p = item[:n]
        content, bound, status = S.host_answers(L, p)
        d = oracle_code(p)
        if len(item) - 4 <= n:                                   # set A: the cut is inside the checksum's 4 bytes
            cut_in_checksum.append(n)
            assert (status, d) == (72, 22), n                    # srcSize_wrong here (FindFrameCompressedSize :1996-1999), checksum_wrong there
            assert content == ERROR and bound == ERROR, n
        else:                                                    # set B
            assert (content == ERROR) == (d != 0), (n, content, d)
            assert (bound == ERROR) == (d != 0), (n, bound, d)
            assert status == d, (n, status, d)
    assert len(cut_in_checksum) == 4


def test_refusals(L):
    good = S.sized_frame(6, 40)
    cases = {
        "reserved bit": (W.frame([W.raw(b"abc")], reserved=True)[0], 14),
        "window log 31": (W.frame([W.raw(b"abc")], fcs=None, single=False, window=(21, 0))[0], 16),
        "wrong magic": (W.frame([W.raw(b"abc")], magic=0xFD2FB527)[0], 10),
        "block type 3": (W.frame([W.Block("reserved", b"abc")])[0], 20),
    }
    for k in range(1, 5):
        cases[f"{k} bytes behind a frame"] = (good + b"\0" * k, 72)
    for what, (item, code) in cases.items():
        content, bound, status = S.host_answers(L, item)
        assert status == code, what
        assert content == ERROR and bound == ERROR, what
    # (the trailing bytes are the item's fault, not the frame's; a window log of 30 is the largest taken)
    assert first_code(L, good + b"\0\0") == 0
    w30 = W.frame([W.raw(b"abc")], fcs=None, single=False, window=(20, 0))[0]
    assert S.host_answers(L, w30) == (UNKNOWN, 1 << 17, 0)
    for what in ("reserved bit", "window log 31", "wrong magic"):
        assert L.zsmi_getFrameContentSize(cases[what][0], len(cases[what][0])) == ERROR, what


def test_content_size_sum_overflow(L):
    half = W.frame([W.raw(b"")], fcs=1 << 63, fcs_bytes=8)[0]
    assert L.zsmi_findDecompressedSize(half, len(half)) == 1 << 63 and L.zsmi_decompressBound(half, len(half)) == 1 << 63
    both = half + half
    assert L.zsmi_findDecompressedSize(both, len(both)) == ERROR and L.zsmi_decompressBound(both, len(both)) == ERROR
    assert S.host_answers(L, both)[2] == 0                       # (no frame is refused: the sum is)
