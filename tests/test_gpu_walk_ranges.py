"""k_lz_walk gives every walker ONE walk range, decided in front of its loop (walker w = range w: no queue), and ends a step in
straight-line code that every lane runs, walkers at rest included.  Every frame must be oracle E's, byte for byte, on chunk sizes at the
edges of that assignment - 1, 31, 32, 33 ranges (a wavefront of the level-3 kernel holds 32 walkers), the full unit, ranges of 512 bytes,
units of 128 KiB, prefixed units of a dictionary call - and on contents whose walkers finish far apart, so that most lanes of a wavefront
rest through most of its steps.  Batches, frames and the first difference: tests/_batch.py."""
import numpy as np
import pytest
import _data as D, _batch as B, _cdict as K, _dicts as X

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def codec():
    from zstandard_amd import BatchCodec
    bc = BatchCodec(0)
    yield bc
    bc.close()


@pytest.fixture(scope="module")
def text():
    return D.zipf_log(300000, single=True).tobytes()


def assert_oracles(codec, chunks, level, dic=b"", what=""):
    """one compress_host call against oracle E's batch form, frame by frame"""
    got, want = B.compress_many(codec, chunks, level, dic), B.oracle_frames(chunks, level, dic)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (what, level, i, len(chunks[i]), len(g), len(w), B.first_difference(g, w))
    return want


# ------------------------------------------------------------------ range-count edges of the static assignment
@pytest.mark.parametrize("what, level, sizes", [
    ("1, 31, 32, 33 ranges of 256 bytes; 256 less one byte; the full unit", 3, (200, 7936, 8192, 8193, 65535, 65536)),
    ("127 and 128 ranges of 512 bytes", 1, (65024, 65536)),
    ("units of 128 KiB: 257, 512 less one byte, 512 ranges", 3, (65537, 131071, 131072)),
])
def test_range_count_edges(codec, text, what, level, sizes):
    assert_oracles(codec, [text[1009 * i:1009 * i + n] for i, n in enumerate(sizes)], level, what=what)


@pytest.mark.parametrize("level", [1, 3])
def test_prefixed_units(codec, level):
    """chunks of 4096 and 65536 bytes with the dictionary trained on their class: _usingDict against oracle E.  _usingCDict: a digested
    trained dictionary may code a frame's first block with its own entropy tables, which no oracle writes - such a frame must round-trip
    (oracle D, the library, libzstd), every other one is oracle E's; and the dictionary's content as a raw dictionary, whose _usingCDict
    frames are all oracle E's: the same prefixed kernels at the same positions"""
    from zstandard_amd import CompressionDict
    dic, data = X.trained("json_records"), X.class_data("json_records")
    chunks = [data[3001:3001 + 4096], data[70001:70001 + 65536]]
    want = assert_oracles(codec, chunks, level, dic, "_usingDict")
    cd = CompressionDict(codec, dic, level)
    frames = B.compress_many(codec, chunks, cdict=cd)
    cd.close()
    B.assert_round_trip(codec, frames, chunks, dic, "_usingCDict")
    for i, (f, w) in enumerate(zip(frames, want)):
        if not K.uses_dictionary_tables(K.blocks_of(f)[0]):
            assert f == w, ("_usingCDict", level, i, len(f), len(w), B.first_difference(f, w))
    raw = X.content_of(dic)
    cd = CompressionDict(codec, raw, level)
    frames = B.compress_many(codec, chunks, cdict=cd)
    cd.close()
    for i, (f, w) in enumerate(zip(frames, B.oracle_frames(chunks, level, raw))):
        assert f == w, ("_usingCDict, raw content", level, i, len(f), len(w), B.first_difference(f, w))


# ------------------------------------------------------------------ walkers that finish far apart
def test_walkers_finish_far_apart(codec):
    """ranges of noise (a step takes nothing and moves a whole window on: done in ~16 steps) next to ranges of one repeated 16-byte phrase
    (a long match a step, found at once, or none: done in a few); and a chunk where only the last walkers find anything"""
    rng = np.random.default_rng(77)
    noise = lambda n: rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    phrase = noise(16) * 16
    a = b"".join(noise(256) + phrase for _ in range(128))
    b = b"".join(phrase + noise(256) for _ in range(128))
    tail = noise(65536 - 300) + (b"the quick brown fox " * 15)
    assert len(a) == len(b) == len(tail) == 65536
    for level in (1, 3):
        assert_oracles(codec, [a, b, tail], level, what="alternating ranges, swapped, a compressible tail")
