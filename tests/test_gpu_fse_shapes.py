"""Every shape the encoder's one FSE table builder takes (buildCTableWave, zstandard_amd/csrc/entropy_kernels.hip over zsmi_fse.h), in one
batch of small chunks against oracle E byte for byte, without a dictionary and with a raw-content one.  Each chunk is named for the shape
it is meant to reach; oracle E's own frame is parsed on the CPU (tests/_framewriter.py entropy_shapes) to see that it does, so a shape that
stops being reached fails the test instead of shrinking it."""
import numpy as np
import pytest
import _batch as B
import _dicts as X
import _framewriter as W

pytestmark = pytest.mark.gpu
DICT = X.STREAM[:6000]


def chunks():
    """{name: (chunk, what the first block of oracle E's frame must show)}"""
    corpus = dict(X.corpus_classes())
    rng = np.random.default_rng(9)
    # 33 byte values, two of them half as frequent as the rest: 31 codes of 5 bits and 2 of 6, so 32 weights (table log 5) of two values
    few = np.repeat(np.arange(33, dtype=np.uint8), [32 if s in (5, 17) else 64 for s in range(33)])
    rng.shuffle(few)
    noise = rng.integers(0, 256, 150, dtype=np.uint8).tobytes()
    return {
        # 1 .. 63 sequences: the three predefined distributions, each with -1 entries
        "predefined": (corpus["json"][:800], lambda s: 1 <= s.nseq < 64 and s.tables == ["pre", "pre", "pre"]),
        # just over 64 sequences: the smallest computed table log for the offset and match-length codes (the literal-length codes reach
        # past 15, whose table needs log 6)
        "log5": (corpus["bintable"][:800], lambda s: 64 <= s.nseq < 128 and s.tables == [6, 5, 5]),
        # a full block of text: the largest table logs; its literals' weights as an FSE table of log 6
        "log9_weights6": (corpus["json"][:65536], lambda s: s.tables == [9, 8, 9] and s.weights == 6),
        # one sequence (noise and a copy of its start): every table a single symbol
        "rle": (noise + noise[:80], lambda s: s.nseq == 1 and s.tables == ["rle", "rle", "rle"]),
        "weights5": (few.tobytes(), lambda s: s.weights == 5),
        # 16 byte values, all as frequent: one weight throughout, which has no FSE form
        "weights4bit": (rng.integers(0, 16, 2000, dtype=np.uint8).tobytes(), lambda s: s.weights == "4bit"),
    }


@pytest.fixture(scope="module")
def codec():
    from zstandard_amd import BatchCodec
    return BatchCodec(0)


@pytest.mark.parametrize("dic", [b"", DICT], ids=["plain", "raw_dictionary"])
def test_every_table_shape_against_oracle_e(codec, dic):
    cases = chunks()
    data = [c for c, _ in cases.values()]
    expect = B.oracle_frames(data, 3, dic)
    for (name, (_, reached)), f in zip(cases.items(), expect):
        first = W.entropy_shapes(f)[0]
        assert first is not None and reached(first), (name, first)
    got = B.compress_many(codec, data, 3, dic)
    for name, g, e in zip(cases, got, expect):
        assert g == e, (name, len(g), len(e), B.first_difference(g, e))
