"""The frame index in Python (test infrastructure): the serial definition - the loop over zsmi_findFrameCompressedSize and
zsmi_getFrameContentSize, two calls pinned to libzstd (tests/golden/libzstd_sizes.json) - and the streams the index tests walk, built from
tests/_framewriter.py, the golden libzstd frames and oracle E.

    pos = 0; while pos < size: c = findFrameCompressedSize(src + pos) (an error: the result); d = getFrameContentSize(src + pos);
    then, at the same frame, frameParameter_unsupported for no stated size, d > 1 GiB or c > 0xFFFFFFFF; entry {pos, c, d}; pos += c
    more than 0x8000000 frames: frameIndex_tooLarge"""
import ctypes, os, struct
import numpy as np
import _data as D
import _framewriter as W
import _oracle as O

E_PREFIX, E_PARAM, E_CORRUPT, E_INIT, E_TOO_SMALL, E_SRC_SIZE, E_FRAME_INDEX = 10, 14, 20, 62, 70, 72, 100
UNKNOWN = (1 << 64) - 1
MAX_FRAMES, MAX_DSIZE, MAX_CSIZE = 0x8000000, 1 << 30, 0xFFFFFFFF
ZSTD_MAGIC, SKIP_MAGIC = 0xFD2FB528, 0x184D2A50


def index(L, stream):
    """-> ([(pos, cSize, dSize)], code): the entries in front of the stream's end or of the first refused frame, and 0 or that frame's code"""
    stream = bytes(stream)
    size = len(stream)
    buf = ctypes.create_string_buffer(stream, max(size, 1))
    base = ctypes.addressof(buf)
    rows, pos = [], 0
    while pos < size:
        c = L.zsmi_findFrameCompressedSize(ctypes.c_void_p(base + pos), size - pos)
        if L.zsmi_isError(c):
            return rows, int(L.zsmi_getErrorCode(c))
        d = int(L.zsmi_getFrameContentSize(ctypes.c_void_p(base + pos), size - pos))
        if d > MAX_DSIZE or c > MAX_CSIZE:                                  # (unknown and error are the two largest values)
            return rows, E_PARAM
        if len(rows) == MAX_FRAMES:
            return rows, E_FRAME_INDEX
        rows.append((pos, int(c), d))
        pos += int(c)
    return rows, 0


def table(rows):
    """the seek table zsmi_buildSeekTable writes for these entries: no checksums"""
    import _seekable as S
    return S.table([(c, d, 0) for _, c, d in rows], False)


# ------------------------------------------------------------------ the good stream: (frame, content) in order; a skippable frame's content is b""
def _text(n, seed):
    return D.zipf_log(n, seed_lo=seed, single=True).tobytes()


def golden_frame():
    """a libzstd 1.4.8 frame whose header states its content size (ZSTD_compress always does): the first such fixture by name"""
    fx = D.fixtures()
    for name in sorted(fx):
        frame, want = fx[name]
        frame, want = bytes(frame), bytes(want)
        if len(want) and W.frame_header(frame).content_size == len(want):
            return frame, want
    raise AssertionError("no golden frame states its size")


_good = None


def good_parts():
    global _good
    if _good is not None:
        return _good
    magics = (struct.pack("<I", ZSTD_MAGIC) + struct.pack("<I", SKIP_MAGIC + 3)) * 32        # 64 magic numbers back to back, both kinds
    inner = W.frame([W.raw(b"a whole valid frame")])[0]
    two, four = _text(100000, 0x21), _text(200000, 0x22)
    e2, e4 = O.compress(two, 3), O.compress(four, 3)
    assert len(list(W.blocks(e2))) == 2 and len(list(W.blocks(e4))) == 4
    alphabet = (open(os.path.join(D.GOLDEN, "csharp_alphabet.zst"), "rb").read(), D.alphabet_data())
    parts = [W.frame([W.raw(b"")]),                                                         # 1. empty content
             W.frame([W.raw(b"Z")]),                                                        # 2. one byte
             W.frame([W.raw(_text(200, 0x23))], checksum=True),                             # 3. a checksum
             (e2, two), (e4, four),                                                         # 4. two blocks, four blocks (oracle E)
             W.frame([W.raw(_text(70, 0x24)), W.rle(0x41, 300), W.raw(_text(9, 0x25)), W.rle(0, 1)]),
             (W.skippable(b""), b""), (W.skippable(b"eleven byte", nibble=7), b""),         # 5. skippable: empty, 11 bytes
             W.frame([W.raw(magics)]),                                                      # 6. a payload of magic numbers
             W.frame([W.raw(b"in front of it: " + inner)]),                                 # 7. a payload that ENDS with a whole valid frame
             golden_frame(), alphabet]                                                      # 8. libzstd's, and the reference's golden vector
    assert all(c is not None for _, c in parts)
    _good = [(bytes(f), bytes(c)) for f, c in parts]
    return _good


def good_stream():
    return b"".join(f for f, _ in good_parts())


def starts(parts):
    out, at = [], 0
    for f, _ in parts:
        out.append(at)
        at += len(f)
    return out


# ------------------------------------------------------------------ bad streams: name -> bytes; the expected code is index()'s
def bad_streams():
    parts = good_parts()
    good = good_stream()
    last = starts(parts)[-1]
    out = {}
    for k in (1, 2, 3, 4):
        out[f"cut_{k}_into_last"] = good[:last + k]
        out[f"cut_{k}_off_the_end"] = good[:-k]
        out[f"junk_{k}_behind"] = good + b"\x28\xb5\x2f\xfd"[:k]
    out["junk_5_behind"] = good + b"junk!"
    third = starts(parts)[2]
    out["wrong_magic_third_frame"] = good[:third] + b"\x29" + good[third + 1:]
    head, tail = b"".join(f for f, _ in parts[:3]), b"".join(f for f, _ in parts[5:9])
    out["reserved_block_type"] = head + W.frame([W.raw(b"ok"), W.Block("reserved", b"abc")])[0] + tail
    out["reserved_header_bit"] = head + W.frame([W.raw(b"abc")], reserved=True)[0] + tail
    out["no_content_size"] = head + W.frame([W.raw(b"ten bytes.")], fcs=None, single=False, window=(0, 0))[0] + tail
    out["content_size_over_1gib"] = head + W.frame([W.raw(b"abc")], fcs=(1 << 30) + 1, fcs_bytes=4)[0] + tail
    out["not_a_frame_at_0"] = b"plain text, no frame" + head
    out["three_bytes"] = b"\x28\xb5\x2f"
    return out


def records_stream(n=5000, seed=5):
    """n frames of 20 .. 300 content bytes, seeded: oracle E's and raw-block frames in turn -> (stream, contents)"""
    rng = np.random.default_rng(seed)
    data = _text(1 << 20, 0x31)
    frames, contents = [], []
    for i in range(n):
        size = int(rng.integers(20, 301)); o = int(rng.integers(0, len(data) - size))
        c = data[o:o + size]
        frames.append(O.compress(c, 3) if i & 1 else W.frame([W.raw(c)], checksum=bool(i & 2))[0])
        contents.append(c)
    return b"".join(frames), contents
