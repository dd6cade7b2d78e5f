"""A stream of zstd frames whose CONTENT passes 4 GiB while the stream itself is a few hundred KB (test infrastructure): what drives the
64-bit offsets, sizes and totals of the index, the range reads and the size queries across 2^31 and 2^32 without anybody holding the content.

N frames, written with tests/_framewriter.py.  Frame f: one raw block of 16 bytes, struct.pack("<QQ", f, f * 0x9E3779B97F4A7C15 mod 2^64) -
the frame's name - then 8 RLE blocks of RLE_SIZES[j] bytes whose byte is rle_byte(f, j).  Every frame holds S content bytes, S no power of
two, so frame borders fall on no round address; every frame is the same FRAME_BYTES long: one template, patched (the head's 16 bytes, the 8
RLE bytes).  The content is a closed form - content_at(offset, length) - and is never materialised; neither is a list of frame contents.
Neither 2^31 nor 2^32 falls on a frame border or within 64 bytes of a block border (asserted below)."""
import struct
import numpy as np
import _framewriter as W

M64 = (1 << 64) - 1
GOLD = 0x9E3779B97F4A7C15
S = 999983                                                  # content bytes a frame (a prime)
N = 4400                                                    # frames
HEAD = 16
NRLE = 8
RLE_SIZES = [(S - HEAD) // NRLE + (1 if j < (S - HEAD) % NRLE else 0) for j in range(NRLE)]
BLOCK_STARTS = [0, HEAD] + [HEAD + sum(RLE_SIZES[:j + 1]) for j in range(NRLE)]          # within a frame; the last one is S
CONTENT = N * S
T31, T32 = 1 << 31, 1 << 32

assert sum(RLE_SIZES) + HEAD == S and max(RLE_SIZES) <= 128 << 10 and S & (S - 1)
assert CONTENT > T32 + (64 << 20)
for _t in (T31, T32):
    assert all(abs(_t % S - b) > 64 for b in BLOCK_STARTS), "a crossing within 64 bytes of a block border (frame borders are block borders)"


def rle_byte(f, j):
    """the byte of RLE block j of frame f: neighbouring blocks and neighbouring frames differ (steps 37 and 101 are odd and differ from
    each other and from 0 mod 256; asserted over every frame by test_wide_words_host.py's model check and the aliasing condition)"""
    return (f * 101 + j * 37 + 11) & 0xFF


def head(f):
    return struct.pack("<QQ", f, f * GOLD & M64)


# ------------------------------------------------------------------ the template
_T, _T_CONTENT = W.frame([W.raw(bytes(HEAD))] + [W.rle(0, n) for n in RLE_SIZES])
assert len(_T_CONTENT) == S
FRAME_BYTES = len(_T)
_HDR = W.frame_header(_T).end
_HEAD_AT = _HDR + 3                                          # the raw block's payload
_RLE_AT = [_HEAD_AT + HEAD + 4 * j + 3 for j in range(NRLE)]  # the byte behind each RLE block's 3-byte header
assert _RLE_AT[-1] + 1 == FRAME_BYTES
del _T_CONTENT


def frame(f):
    b = bytearray(_T)
    b[_HEAD_AT:_HEAD_AT + HEAD] = head(f)
    for j, at in enumerate(_RLE_AT):
        b[at] = rle_byte(f, j)
    return bytes(b)


_stream = None


def stream():
    """the N frames, concatenated (no seek table)"""
    global _stream
    if _stream is None:
        a = np.tile(np.frombuffer(_T, dtype=np.uint8), (N, 1))
        f = np.arange(N, dtype=np.uint64)
        a[:, _HEAD_AT:_HEAD_AT + 8] = f.astype("<u8").view(np.uint8).reshape(N, 8)
        a[:, _HEAD_AT + 8:_HEAD_AT + 16] = (f * np.uint64(GOLD)).astype("<u8").view(np.uint8).reshape(N, 8)     # (uint64 wraps: mod 2^64)
        for j, at in enumerate(_RLE_AT):
            a[:, at] = ((f * np.uint64(101) + np.uint64(j * 37 + 11)) & np.uint64(0xFF)).astype(np.uint8)
        _stream = a.tobytes()
        assert _stream[:FRAME_BYTES] == frame(0) and _stream[-FRAME_BYTES:] == frame(N - 1)
    return _stream


def entries():
    """[(pos, cSize, dSize)] a frame, Python ints: the index of the stream"""
    return [(f * FRAME_BYTES, FRAME_BYTES, S) for f in range(N)]


def frame_of(offset):
    return offset // S


def content_at(offset, length):
    """content bytes [offset, offset + length) in closed form (bytes); the range must lie inside the content"""
    assert 0 <= offset and offset + length <= CONTENT and length <= 64 << 20
    p = np.arange(offset, offset + length, dtype=np.uint64)
    f, w = p // np.uint64(S), p % np.uint64(S)
    j = np.searchsorted(np.asarray(BLOCK_STARTS[1:], dtype=np.uint64), w, side="right").astype(np.uint64)   # 0: the head; 1 .. 8: RLE j - 1
    out = ((f * np.uint64(101) + (j - np.uint64(1)) * np.uint64(37) + np.uint64(11)) & np.uint64(0xFF)).astype(np.uint8)
    in_head = w < HEAD
    if in_head.any():
        fh, wh = f[in_head], w[in_head]
        word = np.where(wh < 8, fh, fh * np.uint64(GOLD))
        out[in_head] = ((word >> (np.uint64(8) * (wh & np.uint64(7)))) & np.uint64(0xFF)).astype(np.uint8)
    return out.tobytes()


# ------------------------------------------------------------------ the ranges under test
_f32 = frame_of(T32)
PLACES = [
    (T31 - 5000, 5000),                                     # ends exactly at 2^31
    (T31, 5000),                                            # begins exactly at 2^31
    (T31 - 100, 200),
    (T32 - 5000, 5000),
    (T32, 5000),
    (T32 - 100, 200),
    ((_f32 - 1) * S + S - 3000, 3000 + S + 3000),          # three frames: the tail of one, the whole frame that holds 2^32, a head and more
    (CONTENT - 1000, 1000),                                 # the last bytes of the content
    (3 * S - 70, 4321),                                     # low control: across a frame border
]
assert PLACES[6][0] < T32 < PLACES[6][0] + PLACES[6][1] and frame_of(PLACES[6][0]) + 2 == frame_of(PLACES[6][0] + PLACES[6][1] - 1)
CROSSING_FRAMES = sorted({frame_of(t) + k for t in (T31, T32) for k in (-1, 0, 1)})     # on both sides of each crossing
