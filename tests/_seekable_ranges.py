"""Batch range reads through an opened seekable archive (test infrastructure): a Python statement of which frames a range overlaps and
how many distinct frames a batch decodes, the seek-table damages of test_seekable_table.py applied to any archive, and one device read of
a batch into a single canary-guarded buffer."""
import ctypes, struct
from bisect import bisect_left, bisect_right
import numpy as np
import _seekable as S
import test_seekable_table as T
from _hip import Dev, CANARY, PAD


# ------------------------------------------------------------------ the span rule
def content_offsets(rows):
    """prefix sums of Decompressed_Size: frame i holds content [d[i], d[i + 1])"""
    d = [0]
    for r in rows:
        d.append(d[-1] + r[1])
    return d


def clip(ranges, content):
    """(offset, length) -> [a, b) clipped at the content's end (offset <= content)"""
    return [(o, o + max(0, min(n, content - o))) for o, n in ranges]


def span(d, a, b):
    """the frames content [a, b) overlaps: (first, last), zero-size frames in between included; None for an empty range"""
    if a == b:
        return None
    return bisect_right(d, a) - 1, bisect_left(d, b) - 1


def frames_touched(rows, ranges):
    """per range the list of frame indices it overlaps, and the union of them all"""
    d = content_offsets(rows)
    per, union = [], set()
    for a, b in clip(ranges, d[-1]):
        sp = span(d, a, b)
        fr = list(range(sp[0], sp[1] + 1)) if sp else []
        per.append(fr)
        union.update(fr)
    return per, union


# ------------------------------------------------------------------ table damages, on any archive
def table_damages(arc):
    """name -> the archive with one rule of the table broken (the damages of test_seekable_table.bad_archives, for this archive)"""
    rows, ck = S.parse(arc)
    n, e = len(rows), 12 if ck else 8
    t0 = len(arc) - (17 + n * e)
    desc = 0x80 if ck else 0
    out = {
        "footer_magic": arc[:-4] + struct.pack("<I", S.SEEKABLE_MAGIC ^ 1),
        "skippable_magic": arc[:t0] + struct.pack("<I", 0x184D2A50) + arc[t0 + 4:],
        "frame_size_field": arc[:t0 + 4] + struct.pack("<I", n * e + 10) + arc[t0 + 8:],
        "sizes_short": T.rebuilt(arc, lead=b"\x00"),
        "too_many_frames": arc[:-9] + struct.pack("<IBI", S.MAX_FRAMES + 1, desc, S.SEEKABLE_MAGIC),
    }
    for bit in range(2, 7):
        out[f"reserved_bit{bit}"] = arc[:-5] + bytes([desc | (1 << bit)]) + arc[-4:]
    if n:
        out["frame_count_disagrees"] = arc[:t0] + T.fsize_says(S.table(rows[:-1], ck), n * e + 9)
        out["sizes_long"] = T.rebuilt(arc, rows=[(rows[0][0] + 1,) + rows[0][1:]] + rows[1:])
        out["csize_zero"] = T.rebuilt(arc, rows=rows[:-1] + [(0, 5, 0)], lead=bytes(rows[-1][0]))
        out["dsize_over_1gib"] = T.rebuilt(arc, rows=rows[:-1] + [(rows[-1][0], (1 << 30) + 1, 0)])
    return out


# ------------------------------------------------------------------ handles and one batch read on the device
def open_host(L, ctx, arc):
    err = ctypes.c_int(-1)
    sk = L.zsmi_openSeekable(ctx, arc, len(arc), ctypes.byref(err))
    return sk, err.value


def open_device(L, ctx, d_ptr, size):
    err = ctypes.c_int(-1)
    sk = L.zsmi_openSeekableDevice(ctx, ctypes.c_void_p(d_ptr), size, ctypes.byref(err))
    return sk, err.value


def u64(a):
    return np.ascontiguousarray(a, dtype=np.uint64)


def ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


class Batch:
    """what one zsmi_seekableReadRangesDevice call gave: rc, out[r] (bytes at range r's place), written, status, frames_decoded"""


def read_ranges(L, H, codec, sk, ranges, content, seed=1, residue=None):
    """every range of the batch into ONE device buffer: range r sits at a dstOffsets[r] assigned in shuffled order, with a PAD-byte canary
    gap before and after every range (residue: r -> dstOffsets[r] % 16).  Asserts that every gap and the outer pads still hold CANARY."""
    n = len(ranges)
    want = [max(0, min(ln, content - o)) for o, ln in ranges]                  # (o > content: the call refuses, nothing is placed)
    order = np.random.default_rng(seed).permutation(n)
    dst_off = np.zeros(max(n, 1), dtype=np.uint64)
    pos = PAD
    for r in order:
        if residue is not None:
            pos += (residue(int(r)) - pos) % 16
        dst_off[r] = pos
        pos += want[r] + PAD
    total = pos + 16
    dst, st = Dev(H, total), Dev(H, 4 * max(n, 1))
    off, ln = u64([r[0] for r in ranges] or [0]), u64([r[1] for r in ranges] or [0])
    written = np.full(max(n, 1), 0xDEAD, dtype=np.uint64)
    frames = ctypes.c_uint32(0xDEAD)
    b = Batch()
    try:
        b.rc = L.zsmi_seekableReadRangesDevice(codec.ctx, sk, ptr(off), ptr(ln), n, ctypes.c_void_p(dst.p), ptr(dst_off), ptr(written),
                                               ctypes.c_void_p(st.p), ctypes.byref(frames))
        codec.sync()
        buf = np.frombuffer(dst.all(), dtype=np.uint8)
        sbuf = st.all()
    finally:
        dst.free(); st.free()
    b.frames_decoded = frames.value
    b.written = [int(w) for w in written[:n]]
    b.status_raw = sbuf[PAD:PAD + 4 * n]
    assert sbuf[:PAD] == bytes([CANARY]) * PAD and sbuf[PAD + 4 * n:] == bytes([CANARY]) * (len(sbuf) - PAD - 4 * n), "wrote outside dStatus[nRanges]"
    outside = np.ones(len(buf), dtype=bool)
    if b.rc == 0:
        assert b.written == want, "written[] is not the clipped length"
        for r in range(n):
            outside[PAD + int(dst_off[r]):PAD + int(dst_off[r]) + want[r]] = False
    assert bool(np.all(buf[outside] == CANARY)), "a range wrote outside its own span"
    b.status = [int.from_bytes(b.status_raw[4 * r:4 * r + 4], "little") for r in range(n)]
    b.out = [buf[PAD + int(dst_off[r]):PAD + int(dst_off[r]) + want[r]].tobytes() for r in range(n)] if b.rc == 0 else None
    return b
