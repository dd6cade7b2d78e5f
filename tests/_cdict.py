"""What the digested-dictionary tests share (tests/test_gpu_cdict.py) with the generators of their fixtures
(tests/golden/gen_fixtures_cdict_sizes.py, gen_fixtures_cdict_frames.py): the chunks of the size test, a parser of a frame's block
structure, the narrow dictionary, and the dictionaries and records whose frames are pinned by digest."""
import hashlib
import numpy as np
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


def uses_repeat_mode(block):
    """a Repeat_Mode (3) among the block's three sequence modes"""
    modes = block[2]
    return modes is not None and any(((modes >> s) & 3) == 3 for s in (6, 4, 2))


def uses_dictionary_tables(block):
    """Treeless literals (type 3) or a Repeat_Mode"""
    return block[1] == 3 or uses_repeat_mode(block)


def narrow_dictionary():
    """a formatted dictionary whose Huffman table covers only 'a'..'h' and whose FSE tables cover few codes: offsets codes 0 - 3, match
    length codes 0 - 3, literal length codes 0 - 3"""
    lengths = W.flat_lengths(range(ord("a"), ord("i")))
    weights, _ = W.lengths_to_weights(lengths)
    of = ([8, 8, 8, 8], 5)
    ml = ([16, 16, 16, 16], 6)
    ll = ([16, 16, 16, 16], 6)
    content = (b"abcdefgh" * 40 + bytes(range(256)) * 4 + b"hgfedcba" * 40)
    return (0xEC30A437).to_bytes(4, "little") + (77).to_bytes(4, "little") + W.huf_description(weights) + W.ncount(*of) + W.ncount(*ml) + W.ncount(*ll) + \
        b"".join(r.to_bytes(4, "little") for r in (1, 4, 8)) + content


PIN_LEVELS = (1, 3)


def pin_cases():
    """{name: (dictionary, records)} of the frames pinned in tests/golden/cdict_frame_digests.json: formatted dictionaries whose counts
    hold -1 entries (the trained ones) and the narrow one, 32 records of 150 .. 770 bytes each"""
    rng = np.random.default_rng(5)
    text = lambda k, alphabet: bytes(rng.choice(np.frombuffer(alphabet, dtype=np.uint8), k).tolist())
    cut = lambda data: [data[7000 * i:7000 * i + 150 + 20 * i] for i in range(32)]
    narrow = [text(150 + 20 * i, b"abcdefgh" if i % 2 else b"abcdefghXYZ012") for i in range(32)]
    return {"trained8k": (X.TRAINED8K, cut(X.class_data("json_records"))),
            "trained64k_json_records": (X.trained("json_records"), cut(X.class_data("json_records"))),
            "trained64k_binary_table": (X.trained("binary_table"), cut(X.class_data("binary_table"))),
            "narrow": (narrow_dictionary(), narrow)}


def frames_digest(frames):
    """SHA-256 over the frames of one batch, each behind its length"""
    h = hashlib.sha256()
    for f in frames:
        h.update(len(f).to_bytes(4, "little")); h.update(f)
    return h.hexdigest()
