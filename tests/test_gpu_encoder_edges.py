"""The entropy kernels (k_encode_literals, k_encode_sequences, zs_emit_block / k_assemble_frames; zstandard_amd/csrc/entropy_kernels.hip) at
every border of their section rules: the encoder edge catalogue (tests/_encoder_edges.py) as one batch per level against oracle E byte for
byte, once more in reverse order (other neighbours, workgroup numbers and scratch slots for every entry), and its dictionary entries through
the dictionary batch call.  Each entry is named for the decision it reaches, and the predicate is asserted again on the very oracle frame the
kernel's is compared with (as tests/test_gpu_fse_shapes.py does), so an entry that stops reaching its border fails instead of passing for
nothing.  A mismatch names its entries."""
import functools
import pytest
import _batch as B
import _encoder_edges as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def codec():
    from zstandard_amd import BatchCodec
    return BatchCodec(0)


@functools.lru_cache(maxsize=None)
def oracle(level):
    """{entry id: oracle E's frame}, once per level"""
    entries, _ = C.catalogue()
    return {e.id: f for e, f in zip(entries, C.oracle_frames(entries, level))}


def check(codec, entries, level, dic, what):
    expect = [oracle(level)[e.id] for e in entries]
    chunks = [e.chunk for e in entries]
    assert sum(map(len, chunks)) <= C.MAX_BYTES
    unreached = [e.id for e, f in zip(entries, expect) if not (e.level3_only and level != 3) and not e.holds(f)]
    assert not unreached, (what, "oracle E's frame no longer shows the decision", unreached)
    got = B.compress_many(codec, chunks, level, dic)
    differ = [(e.id, e.what, len(g), len(x), B.first_difference(g, x)) for e, g, x in zip(entries, got, expect) if g != x]
    assert not differ, (what, len(differ), "frames differ from oracle E's: (entry, its decision, sizes, first difference)", differ[:12])
    B.assert_round_trip(codec, got, chunks, dic, what)


@pytest.mark.parametrize("level, reverse", [(1, False), (3, False), (4, False), (3, True)], ids=["level1", "level3", "level4", "level3_reversed"])
def test_plain_catalogue_in_one_batch(codec, level, reverse):
    plain = [e for e in C.catalogue()[0] if not e.dic]
    # each batch ends in another of the whole-block chunks with len % 4 = 1, 2, 3: the literal histogram's tail reads end with the buffer
    entries = C.ordered(plain, turn=C.LEVELS.index(level) + 3 * reverse, reverse=reverse)
    assert entries[-1].last and len(entries) == len(plain)
    check(codec, entries, level, b"", f"level {level}{', reversed' * reverse}")


@pytest.mark.parametrize("level", [1, 3])
def test_dictionary_entries_by_dictionary(codec, level):
    with_dic = [e for e in C.catalogue()[0] if e.dic]
    assert with_dic
    for dic in sorted({e.dic for e in with_dic}):
        check(codec, [e for e in with_dic if e.dic == dic], level, dic, f"level {level}, raw dictionary of {len(dic)}")
