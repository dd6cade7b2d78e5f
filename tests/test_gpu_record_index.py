"""The record index on the device over plain text (zsmi_indexRecordsDevice) against the numpy statement of the rule (tests/_recindex.py),
at the smallest shapes at which the tile kernels can go wrong: every host input; places on a tile border and one byte to either side; a
place on every byte of one tile; empty frames across a border; one frame over three tiles whose only delimiter lies in the middle tile,
in front of the frame or behind its start in the first tile - aligned and not; delimiters on both sides of a tile border; sizes of
16384 k + {0, 1, 15, 16, 16383} with atEnd 0 and 1, with and without a tail; 2049 tiles, where the tile scan takes its second tile sum; a
base of 2^32 - 3; slices borrowed at odd offsets of a buffer full of delimiters; the host checks that need a context; and context
scratch poisoned before the call (a child process on the debug-hook library).  Every array is exactly as long as the header sizes it,
between canaries.  Nothing depends on a wait inside the call: the helper synchronises before it reads back."""
import ctypes, os, subprocess, sys
import numpy as np
import pytest
import _recindex as R, _borders as BD
from _hip import hip_of

pytestmark = pytest.mark.gpu
T = R.TILE
CASES = R.cases()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    from zstandard_amd import _lib
    return _lib.lib()


@pytest.fixture(scope="module")
def H():
    return hip_of()


@pytest.fixture(scope="module")
def codec():
    from zstandard_amd import BatchCodec
    bc = BatchCodec(0)
    yield bc
    bc.close()


def hold(L, H, codec, data, places, delim=10, at_end=True, base=None, offset=0, what=""):
    d = R.device(L, H, codec, data, places, delim, at_end, base, offset)
    return R.same_as_rule(d, data, places, delim, at_end, base, what)


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_inputs(L, H, codec, name):
    data, delim, sizes = CASES[name]
    places = R.offsets_of(sizes)
    for at_end in (True, False):
        hold(L, H, codec, data, places, delim, at_end, what=(name, at_end))
    hold(L, H, codec, data, places, delim, True, base=7, what=(name, "a base"))


def test_places_at_a_tile_border(L, H, codec):
    data = R.seeded_text(3 * T + 77, 5)
    places = [0, 1, T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1, 3 * T - 1, 3 * T, 3 * T + 1, len(data)]
    for at_end in (True, False):
        want = hold(L, H, codec, data, places, 10, at_end)
        assert want.misaligned > 0
    for k in (1, 2, 3):                                                    # each border alone: the frame in front of it came in from the tile before
        hold(L, H, codec, data, [0, k * T, len(data)], what=("one border", k))
        hold(L, H, codec, data, [0, k * T - 1, len(data)], what=("one border - 1", k))
        hold(L, H, codec, data, [0, k * T + 1, len(data)], what=("one border + 1", k))


def test_a_place_on_every_byte_of_one_tile(L, H, codec):
    """16 384 one-byte frames in the middle tile: 64 rounds of the workgroup's place loop"""
    data = R.seeded_text(3 * T, 6, every=7)
    places = [0] + list(range(T, 2 * T + 1)) + [len(data)]
    want = hold(L, H, codec, data, places)
    assert len(places) == T + 3 and want.misaligned <= 2
    hold(L, H, codec, b"\n" * (3 * T), places, what="delimiters only")


def test_empty_frames_across_a_border(L, H, codec):
    data = R.seeded_text(2 * T + 300, 7)
    places = [0, 0, 0, T - 3, T - 3, T - 3, T, T, T, T + 2, T + 2, 2 * T, 2 * T, len(data), len(data), len(data)]
    for at_end in (True, False):
        hold(L, H, codec, data, places, 10, at_end)
    tail = data[:-1] + b"x"                                                # empty frames at the content's end behind a tail: all get `records`
    want = hold(L, H, codec, tail, places)
    assert want.first_record[-3:].tolist() == [want.records] * 3 and want.records == want.delimiters + 1


@pytest.mark.parametrize("where,misaligned", (("middle tile", 1), ("first tile, behind the frame's start", 1), ("first tile, in front of the frame", 0), ("nowhere", 0)))
def test_one_frame_over_three_tiles(L, H, codec, where, misaligned):
    """the frame's delimiter count where it ends comes from the tiles' sums and the first tile's count behind its last place"""
    size = 2 * T + 200
    b = bytearray(b"a" * size)
    at = {"middle tile": T + 5000, "first tile, behind the frame's start": T - 50, "first tile, in front of the frame": T - 150, "nowhere": None}[where]
    if at is not None:
        b[at] = 10
    data = bytes(b)
    front = 1 if where == "first tile, in front of the frame" else 0       # there the frame IN FRONT holds the delimiter and ends on an 'a'
    aligned = hold(L, H, codec, data, [0, T - 100, size], at_end=True, what=(where, "the frame ends the content"))
    assert aligned.misaligned == front and aligned.misaligned_frames.tolist() == [0] * front
    cut = hold(L, H, codec, data, [0, T - 100, size], at_end=False, what=(where, "the frame ends a window"))
    assert cut.misaligned == front + misaligned and cut.misaligned_frames.tolist() == [0] * front + [1] * misaligned
    more = hold(L, H, codec, data + b"tail\n", [0, T - 100, size, size + 5], what=(where, "another frame follows"))
    assert more.misaligned == front + misaligned
    ended = bytes(b[:size - 1]) + b"\n"                                    # the same frame ending on a delimiter
    assert hold(L, H, codec, ended, [0, T - 100, size], at_end=False, what=(where, "ends on a delimiter")).misaligned == front


def test_delimiters_on_both_sides_of_a_tile_border(L, H, codec):
    for at in ((T - 1,), (T,), (T - 1, T)):
        b = bytearray(b"a" * (2 * T))
        for k in at:
            b[k] = 10
        for places in ([0, T - 1, T, T + 1, 2 * T], [0, T, 2 * T], [0, T - 1, 2 * T], [0, T + 1, 2 * T]):
            for at_end in (True, False):
                hold(L, H, codec, bytes(b), places, 10, at_end, what=(at, places, at_end))


@pytest.mark.parametrize("k", (0, 1, 2))
def test_sizes_around_a_tile(L, H, codec, k):
    rng = np.random.default_rng(40 + k)
    for extra in (0, 1, 15, 16, 16383):
        size = T * k + extra
        for tail in (True, False):
            b = bytearray(R.seeded_text(size, 50 + extra))
            if size:
                b[size - 1] = 98 if tail else 10
            inner = np.sort(rng.integers(0, size + 1, 40)) if size else np.zeros(3, dtype=np.int64)
            places = np.concatenate([[0], inner, [size]])
            for at_end in (True, False):
                hold(L, H, codec, bytes(b), places, 10, at_end, what=(size, tail, at_end))
            hold(L, H, codec, bytes(b), [0, size], what=(size, tail, "one frame"))


@pytest.fixture(scope="module")
def big():
    """2049 tiles of seeded text, its borders - fixed 4093-byte frames, 3000 seeded places, empty frames - and the rule's answer, once"""
    size = (BD.SCAN_TILE + 1) * T - 5
    data = R.seeded_text(size, 91)
    rng = np.random.default_rng(92)
    places = np.sort(np.concatenate([np.arange(0, size, 4093), rng.integers(0, size + 1, 3000), [size, size, size]])).astype(np.uint64)
    return data, places


def test_2049_tiles(L, H, codec, big):
    """the tile scan's second tile sum"""
    data, places = big
    want = hold(L, H, codec, data, places)
    assert (len(data) + T - 1) // T == BD.SCAN_TILE + 1 and want.misaligned > 1000


def test_a_base_across_32_bits(L, H, codec, big):
    data, places = big
    base = (1 << 32) - 3
    want = hold(L, H, codec, data, places, base=base, at_end=False)
    assert int(want.first_record[-1]) + base > 1 << 32
    small = b"abcde" + R.seeded_text(T + 4, 3)                               # the entry at 5 stays below 2^32, the later ones pass it
    want = hold(L, H, codec, small, [0, 5, T, T + 9], base=base)
    assert int(want.first_record[1]) + base < 1 << 32 < int(want.first_record[2]) + base


@pytest.mark.parametrize("offset", (1, 3, 7, 13))
def test_borrowed_slices(L, H, codec, offset):
    """every byte outside the slice is the delimiter: a kernel that looks outside counts wrong"""
    for size in (1, 16, 4097, T, T + 1, 2 * T + 100):
        for last in (10, 98):
            b = bytearray(R.seeded_text(size, size))
            b[size - 1] = last
            hold(L, H, codec, bytes(b), [0, size // 2, size], offset=offset, what=(size, last, "atEnd"))
            hold(L, H, codec, bytes(b), [0, size // 2, size], at_end=False, offset=offset, what=(size, last, "a window"))


def test_places_the_call_refuses_in_its_status(L, H, codec):
    """dPlaces[0] != 0 or dPlaces[n] != size: status parameter_outOfBound; nothing outside the arrays is written (the helper's canaries)"""
    data = R.seeded_text(T + 100, 8)
    for places in ([1, 50, len(data)], [0, 50, len(data) - 1], [0, 50, len(data) + 1]):
        d = R.device(L, H, codec, data, places)
        assert d.rc == 0 and d.result[0] == R.E_PARAM, (places, d.result)


def test_host_checks(L, H, codec):
    p = ctypes.c_void_p
    one = p(8)                                                             # a non-NULL pointer no refused call looks behind
    ctx = codec.ctx
    assert L.zsmi_indexRecordsDevice(None, None, 5, None, 0, 999, 0, None, None, None) == R.E_INIT
    assert L.zsmi_indexRecordsDevice(ctx, None, 5, one, 0, 999, 0, None, one, None) == R.E_GENERIC
    assert L.zsmi_indexRecordsDevice(ctx, None, 5, None, 0, 999, 0, None, one, one) == R.E_GENERIC
    assert L.zsmi_indexRecordsDevice(ctx, None, 5, one, 0, 999, 0, None, None, one) == R.E_GENERIC
    assert L.zsmi_indexRecordsDevice(ctx, None, 5, one, 0x8000001, 999, 0, None, one, one) == R.E_PARAM
    assert L.zsmi_indexRecordsDevice(ctx, None, 5, one, 0x8000001, 10, 0, None, one, one) == R.E_FRAME_INDEX
    assert L.zsmi_indexRecordsDevice(ctx, None, 5, one, 1, 10, 0, None, one, one) == R.E_SRC_SIZE
    from zstandard_amd import api
    assert hasattr(api.BatchCodec, "index_records_device")


def test_poisoned_context_scratch():
    """the call on a context whose scratch was overwritten first (zsmi_dbg_fillScratch of the debug-hook library: a child process)"""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_recindex.py"), "poison"], env=dict(os.environ, ZSMI_DEBUG_LIB="1"), cwd=ROOT,
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "poison ok" in out.stdout, (out.stdout[-2000:], out.stderr[-4000:])
