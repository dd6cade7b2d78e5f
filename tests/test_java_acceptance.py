"""The reference's SECOND decoder (Java, aircompressor lineage) is stricter than the C# one that oracle D restates.  No JVM exists in
this image, so its acceptance rules are stated here and checked on the frames this codec emits (oracle E's frames, which the HIP encoder
reproduces byte for byte: tests/test_gpu_codec.py), over the frame walker of tests/_framewriter.py (blocks, read_ncount).

Rules, from java/src/main/java/com/epam/deltix/zstd/ZstdFrameDecompressor.java:
  :843-920  readFrameHeader: no dictionary id (:891); a frame WITH a window descriptor has windowSize = base + base/8*mantissa,
            a single-segment frame has windowSize = -1 (:857, the field is never set from the content size)
  :309      windowSize <= MAX_WINDOW_SIZE = 8 MiB (:38) -- so a single-segment frame of ANY content size passes (-1 <= 8 MiB); only a
            windowed frame can fail.  Every frame of this codec is single-segment.
  :157-225  one frame per call, no skippable frames; the output buffer must be exactly the content (checksum over outputLimit, :216)
  :36,:279  blocks: compressed block size 3 .. 128 KiB
  :62       offset code <= 28; :60-61 literal-length code <= 35, match-length code <= 52; table logs <= 9 / 9 / 8 (:64-66)
  Huffman.java:45  table log <= 12, and only 1- or 4-stream literals with the sizes of the format
"""
import numpy as np
import pytest

import _oracle as O
import _data as D
import _framewriter as W

MAX_WINDOW = 1 << 23
LL_DEFAULT_MAX, ML_DEFAULT_MAX, OF_DEFAULT_MAX = 35, 52, 28


def walk_frame(frame, content_size):
    """asserts the Java decoder's rules on one frame; returns (blocks, compressed blocks)"""
    h = W.frame_header(frame)                                                 # verifyMagic :928 (no skippable frames)
    assert h.dict_desc == 0                                                   # :891 "Custom dictionaries not supported"
    assert not h.reserved
    assert h.window <= MAX_WINDOW                                             # :309 (a single-segment frame: -1)
    assert h.content_size == content_size                                     # the caller sizes the output buffer from it (:216 needs the exact size)
    nblocks = ncomp = 0
    for b in W.blocks(frame):
        nblocks += 1
        assert b.type in (0, 1, 2)
        if b.type in (0, 1):
            assert b.size <= 128 * 1024
        else:
            assert 3 <= b.size <= 128 * 1024                                  # :279-283
            ncomp += 1
            walk_compressed_block(frame, b)
    assert b.end + 4 * h.checksum == len(frame)                               # one frame, nothing behind it
    return nblocks, ncomp


def walk_compressed_block(frame, b):
    assert b.regen <= 128 * 1024
    if b.lit_type >= 2:                                                       # (raw / RLE literals :692-760)
        assert b.lit_type == 2                                                # 3 = repeat: "Dictionary is corrupted" unless a table is loaded; never emitted
        assert b.csize <= b.size
        if b.size_format != 0:
            assert b.csize >= 10                                              # 4 streams: 6-byte jump table + a byte each (Huffman.java:155)
        # Huffman table description: header byte < 128: FSE-compressed weights, else (byte - 127) weights, 4 bits each
        hb = frame[b.huf_pos]
        if hb >= 128:
            weights = []
            for i in range(hb - 127):
                byte = frame[b.huf_pos + 1 + i // 2]
                weights.append(byte >> 4 if i % 2 == 0 else byte & 15)
            assert max(weights) <= 12
            total = sum((1 << w) >> 1 for w in weights)
            log = total.bit_length()                                          # the last weight completes the power of two above
            assert log <= 12                                                  # Huffman.java:45 / Huf.cs:148
    assert b.seq_pos < b.end
    # sequences header :317-360
    if frame[b.seq_pos] == 0:
        assert b.tables_pos == b.end
        return
    assert b.nseq > 0
    assert b.modes & 3 == 0
    pos = b.tables_pos
    for name, mode, dmax, max_log in (("LL", b.modes >> 6, LL_DEFAULT_MAX, 9), ("OF", (b.modes >> 4) & 3, OF_DEFAULT_MAX, 8), ("ML", (b.modes >> 2) & 3, ML_DEFAULT_MAX, 9)):
        assert mode != 3, "repeat mode in a block that has no earlier table"  # this codec never emits repeat mode
        limit = 28 if name == "OF" else dmax
        if mode == 1:
            assert frame[pos] <= limit; pos += 1                              # RLE: the one symbol
        elif mode == 2:
            norm, log, pos = W.read_ncount(frame, pos, dmax if name != "OF" else 31)
            assert log <= max_log and max(s for s, c in enumerate(norm) if c) <= limit
    assert pos < b.end                                                        # the bitstream has at least a byte


def _check(data, level):
    f = O.compress(data, level)
    assert O.decompress(f, len(data)) == data
    return walk_frame(f, len(data))


@pytest.mark.parametrize("level", [1, 3, 4])
def test_emitted_frames_meet_the_java_decoders_rules(level):
    inputs = D.mixed_inputs()
    seen_comp = 0
    for name, data in inputs.items():
        if len(data) == 0:
            continue                                                          # (an empty frame: the Java decoder returns 0 before reading it when the output is empty, :164)
        nblocks, ncomp = _check(data, level)
        seen_comp += ncomp
    assert seen_comp > 10


def test_frame_above_8_mib_is_single_segment_and_passes():
    """zsmi_compress on a large input emits ONE single-segment frame: the Java decoder's window check (:309) sees windowSize = -1 for it
    (:857), whatever the content size; the C# decoder needs windowLog <= 30 only for windowed frames (ZStdDecompress.cs:468)."""
    data = D.zipf_log((9 << 20) + 12345, seed_lo=3).tobytes()
    f = O.compress(data, 3)
    assert (f[4] >> 5) & 1 == 1
    nblocks, ncomp = walk_frame(f, len(data))
    assert nblocks == (len(data) + 65535) // 65536 and ncomp == nblocks
    assert O.decompress(f, len(data)) == data


def test_walker_rejects_what_the_java_decoder_rejects():
    """the walker is not vacuous: a windowed frame above 8 MiB, a dictionary id, a second frame behind the first all fail"""
    data = D.zipf_log(70000, seed_lo=9).tobytes()
    f = bytearray(O.compress(data, 3))
    walk_frame(bytes(f), len(data))
    with pytest.raises(AssertionError):
        walk_frame(bytes(f) + bytes(f), len(data))
    g = bytearray(f); g[4] |= 1
    with pytest.raises(AssertionError):
        walk_frame(bytes(g), len(data))
    # a windowed header with window 16 MiB: FHD without the single-segment bit, window descriptor exponent 14
    fcs = f[5:9] if (f[4] >> 6) == 2 else None
    assert fcs is not None
    w = bytes(f[:4]) + bytes([f[4] & ~0x20 & 0xFF, 14 << 3]) + bytes(f[5:])
    with pytest.raises(AssertionError):
        walk_frame(w, len(data))
