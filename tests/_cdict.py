"""What the digested-dictionary tests share (tests/test_gpu_cdict.py) with the generator of their libzstd fixture
(tests/golden/gen_fixtures_cdict_sizes.py): the chunks of the size test, and a parser of a frame's block structure."""
import _dicts as X
import _framewriter as W

SIZE_CHUNKS = (1024, 4096, 16384, 65536)
SIZE_BYTES = 256 * 1024


def size_chunks(cls, cs):
    """the first 256 KiB of the class's data, cut in chunks of cs bytes"""
    data = X.class_data(cls)
    return [data[i:i + cs] for i in range(0, SIZE_BYTES, cs)]


def blocks_of(frame):
    """[(block type, literals type or None, sequence modes byte or None)] of a single-segment frame as this library writes them.  The
    modes byte is None where the block has no sequences.  RFC 8878 3.1.1.1 - 3.1.1.3."""
    assert W.frame_header(frame).single, "single segment"
    found = list(W.blocks(frame))
    assert found[-1].end == len(frame), (found[-1].end, len(frame))
    return [(b.type, b.lit_type, b.modes) if b.type == 2 else (b.type, None, None) for b in found]


def uses_dictionary_tables(block):
    """Treeless literals (type 3) or a Repeat_Mode (3) among the block's three sequence modes"""
    _, lt, modes = block
    return lt == 3 or (modes is not None and any(((modes >> s) & 3) == 3 for s in (6, 4, 2)))
