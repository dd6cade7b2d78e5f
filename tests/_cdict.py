"""What the digested-dictionary tests share (tests/test_gpu_cdict.py) with the generator of their libzstd fixture
(tests/golden/gen_fixtures_cdict_sizes.py): the chunks of the size test, and a parser of a frame's block structure."""
import _dicts as X

SIZE_CHUNKS = (1024, 4096, 16384, 65536)
SIZE_BYTES = 256 * 1024


def size_chunks(cls, cs):
    """the first 256 KiB of the class's data, cut in chunks of cs bytes"""
    data = X.class_data(cls)
    return [data[i:i + cs] for i in range(0, SIZE_BYTES, cs)]


def blocks_of(frame):
    """[(block type, literals type or None, sequence modes byte or None)] of a single-segment frame as this library writes them.  The
    modes byte is None where the block has no sequences.  RFC 8878 3.1.1.1 - 3.1.1.3."""
    assert frame[:4] == b"\x28\xb5\x2f\xfd"
    fhd = frame[4]
    assert fhd & 0x20, "single segment"
    did = (0, 1, 2, 4)[fhd & 3]
    fcs = (1, 2, 4, 8)[fhd >> 6]
    pos = 5 + did + fcs
    out = []
    while True:
        h = int.from_bytes(frame[pos:pos + 3], "little"); pos += 3
        last, btype, bsize = h & 1, (h >> 1) & 3, h >> 3
        if btype == 2:
            b = frame[pos:pos + bsize]
            lt, sf = b[0] & 3, (b[0] >> 2) & 3
            if lt < 2:                                       # raw, RLE
                lh = (1, 2, 1, 3)[sf]
                regen = (b[0] >> 3) if lh == 1 else (int.from_bytes(b[:lh], "little") >> 4)
                lsz = lh + (regen if lt == 0 else 1)
            else:                                            # compressed, treeless
                lh = (3, 3, 4, 5)[sf]
                bits = (10, 10, 14, 18)[sf]
                v = int.from_bytes(b[:lh], "little")
                lsz = lh + ((v >> (4 + bits)) & ((1 << bits) - 1))
            q = lsz
            nseq = b[q]; q += 1
            if nseq >= 128:
                if nseq == 255:
                    nseq = b[q] + (b[q + 1] << 8) + 0x7F00; q += 2
                else:
                    nseq = ((nseq - 128) << 8) + b[q]; q += 1
            out.append((2, lt, b[q] if nseq else None))
            pos += bsize
        else:
            out.append((btype, None, None))
            pos += 1 if btype == 1 else bsize
        if last:
            break
    assert pos == len(frame), (pos, len(frame))
    return out


def uses_dictionary_tables(block):
    """Treeless literals (type 3) or a Repeat_Mode (3) among the block's three sequence modes"""
    _, lt, modes = block
    return lt == 3 or (modes is not None and any(((modes >> s) & 3) == 3 for s in (6, 4, 2)))
