"""The walk step (k_lz_walk, zstandard_amd/csrc/lz_kernels.hip) where its addresses and bit counts have borders: a candidate's distance
read from the walker's run of the exchange buffer at every `ip & 7` and every window offset, the skewed rows of the staged source
(a row every 256 bytes, the front pad in front of position 0) on both sides of a match, recent-offset hits at ip .. ip + 3, and the
extension round's 16-byte pieces (matches of 8, 9, 23, 24, 39, 40 and 41 bytes: 8 scored, then 1, 15, 16 = a whole piece, 31, 32 and 33).
Chunks of 4 KiB and 8 KiB at levels 1 and 3 (walk ranges of 512 and 256 bytes: 4 and 2 lanes a walker), one of 64 KiB and one of
128 KiB (a unit of two blocks: distances with bit 16), and one call with a dictionary prefix (matches that start at positions 0 .. 3 and
reach into the dictionary).  Every frame is compared byte for byte with oracle E's and decoded back (oracle D, the library, libzstd).
What the chunks are for is asserted too: every placed copy keeps its length to the end of the construction (border_chunk), the 128 KiB
chunk's second block has offsets of code 16, and each dictionary chunk's first match is found whole from position 0 .. 3 (on oracle E's frames)."""
import functools
import numpy as np
import pytest
import _batch as B
import _framewriter as W

pytestmark = pytest.mark.gpu

LENGTHS = (8, 9, 23, 24, 39, 40, 41)
DELTAS = tuple(range(-4, 5))


@pytest.fixture(scope="module")
def codec():
    from zstandard_amd import BatchCodec
    return BatchCodec(0)


def _copy(buf, at, src, length):
    """a copy of exactly `length` bytes at `at` from `src` (< at): the bytes in front of and behind the two differ"""
    assert 0 <= src < at and at + length < len(buf)
    buf[at:at + length] = buf[src:src + length] if src + length <= at else np.resize(buf[src:at], length)
    if buf[at + length] == buf[src + length]:
        buf[at + length] ^= 0x55
    if src > 0 and buf[at - 1] == buf[src - 1]:
        buf[at - 1] ^= 0x55


def periodic_chunk(seed, size):
    """pieces of 0 .. 7 bytes of noise and then a phrase of period p, for every p in 9 .. 23 and every amount of noise (in an order the
    seed turns): first candidates at every ip & 7 and window offset, and behind each taken match its offset again at ip .. ip + 3"""
    rng = np.random.default_rng(seed)
    combos = [(p, k) for p in range(9, 24) for k in range(8)]
    out, i = [], seed * 37
    while sum(map(len, out)) < size:
        p, k = combos[i % len(combos)]; i += 1
        phrase = rng.integers(0, 256, p, dtype=np.uint8)
        reps = 3 + (i % 5)
        body = np.resize(phrase, p * reps + (i % p))
        if i % 3 == 0:                                               # one byte changed inside the run: the walker tries its last offset again
            body[p * 2 + (i % p)] ^= 0xFF
        out += [rng.integers(0, 256, k, dtype=np.uint8), body]
    return np.concatenate(out)[:size]


def border_chunk(seed, size, delta, far=0, front=True):
    """noise with exact copies: at every multiple b of 256 one copy STARTS at b + delta (from an earlier place of any alignment), and a
    second one, in the middle of the row, has its SOURCE at b + delta; the first copy of the chunk has its source at 0 .. 3 (read
    backwards through the front pad).  The lengths take turns through LENGTHS.  far: sources of the rows above `far` lie at least
    65536 bytes back (the 128 KiB unit: bit 16 of a distance).  front = False: without the first copy, and no source in the chunk's first
    64 bytes (the caller puts something else there)"""
    rng = np.random.default_rng(seed)
    buf = rng.integers(0, 256, size, dtype=np.uint8)
    placed = []

    def _place(buf, at, src, length):
        placed.append((at, src, length))
        _copy(buf, at, src, length)
    if front:
        _place(buf, 100 + seed % 7, seed % 4, LENGTHS[seed % 7])
    for k, b in enumerate(range(256, size - 255, 256)):
        n1, n2 = LENGTHS[(k + seed) % 7], LENGTHS[(k + 3 * seed + 2) % 7]
        at = b + delta
        back = int(rng.integers(60, min(at - (0 if front else 64), 1900)))
        src = at - back
        if far and b >= far:
            src = int(rng.integers(8, at - 65536 - 64)) if k % 2 else (at - 65536 - (k % 5))
        _place(buf, at, src, n1)
        _place(buf, b + 120 + (k % 9), b + delta + (k % 2), n2)      # (k % 2: the source itself, or one byte into it)
    for at, src, n in placed:                                        # no later copy or patched byte has changed an earlier copy's length
        assert (buf[at:at + n] == buf[src:src + n]).all() and buf[at + n] != buf[src + n] and (src == 0 or buf[at - 1] != buf[src - 1]), (seed, at, src, n)
    return buf


@functools.lru_cache(maxsize=None)
def chunks():
    out = []
    for size in (4096, 8192):
        out += [periodic_chunk(s + size, size).tobytes() for s in range(5)]
        out += [border_chunk(size + 11 * i, size, d).tobytes() for i, d in enumerate(DELTAS)]
    big = np.concatenate([periodic_chunk(77, 32768), border_chunk(78, 32768, 3)])
    out.append(big.tobytes())                                       # 64 KiB
    wide = np.concatenate([periodic_chunk(79, 16384), border_chunk(80, 131072 - 16384, -2, far=65536 + 4096)])
    out.append(wide.tobytes())                                      # 128 KiB
    assert [len(c) for c in out[-2:]] == [65536, 131072]
    return out


@functools.lru_cache(maxsize=None)
def dictionary():
    return np.random.default_rng(4242).integers(0, 256, 3072, dtype=np.uint8).tobytes()          # (whole rows: the chunk's rows are the staged rows)


def _dictionary_case(i, d, src, n):
    """(chunk, control): border_chunk with n bytes of the dictionary from src at position lead = i % 4; the control has noise there"""
    dic = np.frombuffer(dictionary(), dtype=np.uint8)
    seed, lead = 900 + i, i % 4
    c = border_chunk(seed, 4096 if i % 2 else 8192, d, front=False)
    noise = np.random.default_rng(seed).integers(0, 256, 64, dtype=np.uint8)
    c[lead:lead + n] = dic[src:src + n]
    c[lead + n] = dic[src + n] ^ 0x55 if src + n < len(dic) else c[lead + n]
    control = c.copy()
    control[lead:lead + n] = noise[:n]
    return c.tobytes(), control.tobytes()


def _literals_saved(chunk, control):
    a, b = (W.section_shapes(f) for f in B.oracle_frames([chunk, control], 3, dictionary()))
    return b[0].regen - a[0].regen if len(a) == len(b) == 1 and a[0].type == b[0].type == 2 else None


@functools.lru_cache(maxsize=None)
def dictionary_cases():
    """[(chunk, control, lead, n)]: chunks whose first match starts at position lead = 0 .. 3 and is n bytes of the dictionary, from
    delta = -4 .. 4 bytes beside one of the dictionary's rows or (every third) 0 .. 4 bytes in front of its end; behind it the border
    copies of a plain chunk.  control: the same chunk with those n bytes left as noise.  Whether the parse finds a given copy is chance
    (a false candidate of the long table hides the true one of the short table): of the rows and lengths in turn the first is taken that
    oracle E matches whole - n literals fewer than in the control"""
    size = len(dictionary())
    out = []
    for i, d in enumerate(DELTAS):
        lengths = [LENGTHS[(i + k) % 7] for k in range(7)]
        if i % 3 == 0:
            tries = [(size - n - e, n) for n in lengths for e in ((i + k) % 5 for k in range(5))]
        else:
            tries = [(256 * m + d, n) for n in lengths for m in range(1, 11)]
        for src, n in tries:
            chunk, control = _dictionary_case(i, d, src, n)
            if _literals_saved(chunk, control) == n:
                out.append((chunk, control, i % 4, n)); break
        else:
            raise AssertionError(("no copy from the dictionary is matched whole", i, d))
    return out


def dictionary_chunks():
    return [c[0] for c in dictionary_cases()]


@functools.lru_cache(maxsize=None)
def oracle(level, with_dictionary=False):
    return B.oracle_frames(dictionary_chunks() if with_dictionary else chunks(), level, dictionary() if with_dictionary else b"")


def _compare(got, expect, what):
    differ = [(i, len(g), len(x), B.first_difference(g, x)) for i, (g, x) in enumerate(zip(got, expect)) if g != x]
    assert not differ, (what, "frames differ from oracle E's: (chunk, sizes, first difference)", differ[:12])


def _has_offset_code(block, code):
    t = block.of
    return (t.mode == "rle" and t.symbol == code) or (t.mode == "fse" and bool(t.norm[code]))


def test_the_chunks_reach_their_borders():
    """on oracle E's frames at level 3 (needs no GPU, but belongs with the comparisons below): the 128 KiB chunk's second block has
    sequences of offset code 16 (offsets from 65533: its far copies lie 65536 and more back, bit 16 of a distance), and every dictionary
    chunk's first n bytes from position lead <= 3 are matched whole: it has n literals fewer than its control, whose bytes there are noise"""
    second = W.section_shapes(oracle(3)[-1])[1]
    assert second.type == 2 and second.nseq > 100 and _has_offset_code(second, 16), (second.type, second.nseq)
    cases = dictionary_cases()
    controls = B.oracle_frames([c[1] for c in cases], 3, dictionary())
    for i, ((chunk, _, lead, n), frame, control) in enumerate(zip(cases, oracle(3, True), controls)):
        a, b = W.section_shapes(frame), W.section_shapes(control)
        assert len(a) == len(b) == 1 and a[0].type == b[0].type == 2 and lead <= 3, i
        assert b[0].regen - a[0].regen == n, (i, lead, n, a[0].regen, b[0].regen)


@pytest.mark.parametrize("level", [1, 3])
def test_walk_borders_match_the_oracle(codec, level):
    expect = oracle(level)
    assert sum(map(len, expect)) < 0.9 * sum(map(len, chunks()))     # the copies are found: the walk runs
    got = B.compress_many(codec, chunks(), level)
    _compare(got, expect, f"level {level}")
    B.assert_round_trip(codec, got, chunks(), b"", f"level {level}")


def test_walk_borders_with_a_dictionary_prefix(codec):
    expect = oracle(3, True)
    got = B.compress_many(codec, dictionary_chunks(), 3, dictionary())
    _compare(got, expect, "dictionary prefix")
    B.assert_round_trip(codec, got, dictionary_chunks(), dictionary(), "dictionary prefix")
