"""Content checksums on frames (test infrastructure): the contract of the checksum parameter stated in Python, independently of the library.
A checksummed frame is the plain frame with bit 2 of the Frame_Header_Descriptor (byte 4) set and, behind the last block, the low 32 bits of
XXH64 (seed 0) of the content, little-endian - oracle D's zso_xxh64.  Nothing else differs, so the frame a flag-on call writes must be
with_checksum(the frame the flag-off call writes, the chunk)."""
import struct
import _oracle as O
import _framewriter as W

CHECKSUM_BIT = 0x04
WRONG = 22                      # checksum_wrong
EMPTY_TRAILER = bytes([0x99, 0xE9, 0xD8, 0x51])          # XXH64 of nothing is 0xEF46DB3751D8E999


def trailer(content: bytes) -> bytes:
    return struct.pack("<I", int(O.lib().zso_xxh64(content, len(content), 0)) & 0xFFFFFFFF)


def last_block(frame: bytes):
    """the last block of the one frame `frame` holds (its pos / end: the block's bytes behind its 3-byte header)"""
    return list(W.blocks(frame))[-1]


def with_checksum(frame: bytes, content: bytes) -> bytes:
    """the checksummed form of a frame that carries no checksum (one frame, ending with its last block)"""
    assert not frame[4] & CHECKSUM_BIT and last_block(frame).end == len(frame)
    return frame[:4] + bytes([frame[4] | CHECKSUM_BIT]) + frame[5:] + trailer(content)


def without_checksum(frame: bytes) -> bytes:
    """the inverse: the trailer cut off and the bit cleared (one frame, ending with its checksum)"""
    assert frame[4] & CHECKSUM_BIT and last_block(frame).end + 4 == len(frame)
    return frame[:4] + bytes([frame[4] & ~CHECKSUM_BIT]) + frame[5:-4]


def oracle_code(frame: bytes, capacity: int, dictionary: bytes = b"") -> int:
    """oracle D's answer for a frame: 0, or its error code"""
    try:
        if dictionary:
            O.decompress_using_dict(frame, capacity, dictionary)
        else:
            O.decompress(frame, capacity)
        return 0
    except O.OracleError as e:
        return e.code


def flip(frame: bytes, byte: int, bit: int) -> bytes:
    return frame[:byte] + bytes([frame[byte] ^ (1 << bit)]) + frame[byte + 1:]


def payload_flip_oracle_calls_checksum_wrong(frame: bytes, capacity: int):
    """(byte, bit) inside the last block's payload whose flip leaves a frame that oracle D still parses and answers checksum_wrong for;
    searched from the payload's end backwards (the last bytes of a bit stream or of raw literals change content without breaking the
    parse most often).  None if no flip of the last 64 payload bytes does."""
    b = last_block(frame)
    for byte in range(b.end - 1, max(b.pos, b.end - 64) - 1, -1):
        for bit in range(8):
            if oracle_code(flip(frame, byte, bit), capacity) == WRONG:
                return byte, bit
    return None
