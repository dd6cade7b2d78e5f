"""The hand-over between the LZ stage and the entropy stage: k_lz_stitch leaves a block's sequences as ONE list in block order and a header a
block (zsmi_scratch.h: seqs, hdrs); a record carries no literal length, the entropy kernels take it from the end of the record before.  Every
frame must be oracle E's, byte for byte, on inputs chosen for the list's edges: lists shorter than one tile of 64, longer than 4096, empty;
literal runs far longer than the 2047 the old record field held; dozens of walk ranges in a row without a record; first records dropped and
cut, chains joined over many ranges; 128 walk ranges a block (levels <= 2) and 256; slots reused by a second sub-batch."""
import os
import numpy as np
import pytest
import _oracle as O, _data as D, _batch as B, _framewriter as FW

pytestmark = pytest.mark.gpu

LEVELS = (1, 3, 4)
ZIPF_SIZES = (16, 17, 255, 256, 257, 1023, 1024, 1025, 65535, 65536, 65537, 131072, 131073)


def _inputs():
    """name -> the chunks of one batch"""
    rng = np.random.default_rng(20)
    z = D.zipf_log(400000, single=True).tobytes()
    noise = lambda n: rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    period = noise(1000)
    return {
        # block and unit edges, a last block of one byte, lists shorter than one tile
        "zipf_sizes": [z[997 * i:997 * i + n] for i, n in enumerate(ZIPF_SIZES)],
        # dozens of consecutive walk ranges without a record; a literal run far longer than 2047 in mid-list
        "text_noise_text": [z[:65536] + noise(20 * 1024) + z[65536:65536 + 45000]],
        # matches run to the crossing limit: first records dropped and cut, chains joined over many ranges
        "period_and_zero_run": [(period * 140)[:137000], z[:30000] + bytes(3000) + z[30000:70000]],
        # a matchless chunk (empty list, block left raw), literals alone (a compressed block without a sequence), text, and short matches
        # packed densely (more than 4096 sequences a block) in one batch
        "noise_sixbit_text_dense": [noise(65536), (rng.integers(0, 64, 3000, dtype=np.uint8) + 32).astype(np.uint8).tobytes(), z[100000:165536],
                                    rng.integers(0, 4, 65536, dtype=np.uint8).tobytes()],
    }


@pytest.fixture(scope="module")
def inputs():
    return _inputs()


@pytest.fixture(scope="module")
def oracle(inputs):
    """(batch, level) -> oracle E's frames, computed once"""
    return {(name, level): B.oracle_frames(chunks, level) for name, chunks in inputs.items() for level in LEVELS}


@pytest.fixture(scope="module")
def codec():
    from zstandard_amd import BatchCodec
    bc = BatchCodec(0)
    yield bc
    bc.close()


def test_inputs_reach_the_list_edges(oracle):
    """Number_of_Sequences of every compressed block of the oracle's frames: the set holds an empty list, one shorter than a tile of 64 and
    one longer than 4096; and a raw block (the matchless chunk)"""
    nseq, raw = [], 0
    for frames in oracle.values():
        for f in frames:
            for b in FW.blocks(f):
                if b.type == 2: nseq.append(b.nseq)
                raw += b.type == 0
    print("sequences a compressed block: min", min(nseq), "max", max(nseq), "blocks", len(nseq), "raw blocks", raw)
    assert 0 in nseq and any(0 < v < 64 for v in nseq) and any(v > 4096 for v in nseq) and raw > 0


@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("name", ["zipf_sizes", "text_noise_text", "period_and_zero_run", "noise_sixbit_text_dense"])
def test_frames_are_the_oracles(codec, inputs, oracle, name, level):
    chunks = inputs[name]
    got = B.compress_many(codec, chunks, level)
    want = oracle[(name, level)]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (name, level, i, len(chunks[i]), len(g), len(w), B.first_difference(g, w))
    for i in sorted({0, len(chunks) // 2, len(chunks) - 1}):              # a sample under oracle D
        assert O.decompress(got[i], len(chunks[i])) == chunks[i], (name, level, i)


_SUB_CHILD = r'''
import sys, os
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import _data as D, _batch as B, _oracle as O
from zstandard_amd import BatchCodec
bc = BatchCodec(0)
z = D.zipf_log(200000, single=True).tobytes()
# 96 blocks in two sub-batches of <= 64: the second reuses the first's slots, with lists of other lengths (long, short, empty, long)
chunks = [z[1013 * i:1013 * i + 65536] for i in range(64)] + [z[5000:5100], bytes(range(256)) * 8, z[:131073]] + [z[700 * i:700 * i + 40000 + 800 * i] for i in range(27)]
for level in (1, 3):
    got = B.compress_many(bc, chunks, level)
    want = B.oracle_frames(chunks, level)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (level, i, len(g), len(w), B.first_difference(g, w))
    assert O.decompress(got[66], len(chunks[66])) == chunks[66]
print("CHILD-OK")
'''


def test_slots_reused_by_a_second_sub_batch():
    """ZSMI_BLOCKS_IN_FLIGHT=64 in a child process: a sub-batch packs its lists into the slots the one before used"""
    B.run_child("-c", _SUB_CHILD, B.ROOT, env=dict(os.environ, ZSMI_BLOCKS_IN_FLIGHT="64"))
