"""An independent Python statement of zstd's seekable format (test infrastructure): writes a seek table from (Compressed_Size,
Decompressed_Size, Checksum) rows, parses one, and builds reference archives from oracle E's frames of the slices.

    archive    = frame_0 .. frame_{n-1} | seek table                               (little-endian integers)
    seek table = 0x184D2A5E (4) | Frame_Size (4) | entry_0 .. entry_{n-1} | footer (9)
    entry_i    = Compressed_Size (4) | Decompressed_Size (4) | [Checksum (4), only if Checksum_Flag]
    footer     = Number_Of_Frames (4) | Seek_Table_Descriptor (1) | 0x8F92EAB1 (4)
    Frame_Size = n * (8 or 12) + 9;  descriptor bit 7 = Checksum_Flag, bits 6-2 reserved (0), bits 1-0 unused
    Checksum   = low 32 bits of XXH64 (seed 0) of the frame's decompressed bytes (oracle D's zso_xxh64)"""
import struct
import _oracle as O

SKIPPABLE_MAGIC, SEEKABLE_MAGIC = 0x184D2A5E, 0x8F92EAB1
MAX_FRAMES, MAX_FRAME_SIZE = 0x8000000, 1 << 30
DEFAULT_FRAME = 65536


def xxh32(data: bytes) -> int:
    return int(O.lib().zso_xxh64(data, len(data), 0)) & 0xFFFFFFFF


def table(rows, checksum: bool, descriptor=None) -> bytes:
    """rows: (cSize, dSize, checksum) - the checksum is written only with the flag.  descriptor: the byte as is (default: the flag alone)"""
    e = 12 if checksum else 8
    body = b"".join(struct.pack("<II", r[0], r[1]) + (struct.pack("<I", r[2]) if checksum else b"") for r in rows)
    desc = (0x80 if checksum else 0) if descriptor is None else descriptor
    return struct.pack("<II", SKIPPABLE_MAGIC, len(rows) * e + 9) + body + struct.pack("<IBI", len(rows), desc, SEEKABLE_MAGIC)


def archive(frames, contents, checksum: bool) -> bytes:
    return b"".join(frames) + table([(len(f), len(c), xxh32(c)) for f, c in zip(frames, contents)], checksum)


def parse(arc: bytes):
    """-> (rows [(cSize, dSize, checksum or None)], checksum flag); ValueError for a table this statement does not accept"""
    if len(arc) < 9:
        raise ValueError("short")
    n, desc, magic = struct.unpack("<IBI", arc[-9:])
    if magic != SEEKABLE_MAGIC or desc & 0x7C or n > MAX_FRAMES:
        raise ValueError("footer")
    ck = bool(desc & 0x80)
    e = 12 if ck else 8
    size = 17 + n * e
    if size > len(arc):
        raise ValueError("table size")
    t = arc[len(arc) - size:]
    skip, fsize = struct.unpack("<II", t[:8])
    if skip != SKIPPABLE_MAGIC or fsize != n * e + 9:
        raise ValueError("header")
    rows = []
    for i in range(n):
        c, d = struct.unpack("<II", t[8 + i * e:16 + i * e])
        rows.append((c, d, struct.unpack("<I", t[16 + i * e:20 + i * e])[0] if ck else None))
    if any(r[0] == 0 for r in rows) or sum(r[0] for r in rows) != len(arc) - size:
        raise ValueError("sizes")
    return rows, ck


def slices(data: bytes, frame_size=0):
    f = frame_size or DEFAULT_FRAME
    return [data[i:i + f] for i in range(0, len(data), f)]


def oracle_archive(data: bytes, frame_size=0, level=3, checksum=True) -> bytes:
    """oracle E's frame of every slice + the table: what zsmi_compressSeekable must produce byte for byte"""
    parts = slices(data, frame_size)
    return archive([O.compress(p, level) for p in parts], parts, checksum)


def zstd_frame(data: bytes, level=3, checksum=False, block_size_log=0) -> bytes:
    """one frame by upstream libzstd (ZSTD_compress2; checksum: ZSTD_c_checksumFlag = 201, its own content checksum).  None without libzstd"""
    import ctypes
    Z = O.libzstd()
    if Z is None:
        return None
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    Z.ZSTD_createCCtx.restype = vp
    Z.ZSTD_freeCCtx.argtypes = [vp]
    Z.ZSTD_CCtx_setParameter.restype = sz; Z.ZSTD_CCtx_setParameter.argtypes = [vp, ctypes.c_int, ctypes.c_int]
    Z.ZSTD_compress2.restype = sz; Z.ZSTD_compress2.argtypes = [vp, vp, sz, vp, sz]
    c = Z.ZSTD_createCCtx()
    Z.ZSTD_CCtx_setParameter(c, 100, level)                   # ZSTD_c_compressionLevel
    Z.ZSTD_CCtx_setParameter(c, 201, int(checksum))           # ZSTD_c_checksumFlag
    cap = Z.ZSTD_compressBound(len(data))
    out = ctypes.create_string_buffer(cap)
    r = Z.ZSTD_compress2(c, out, cap, data, len(data))
    Z.ZSTD_freeCCtx(c)
    assert not Z.ZSTD_isError(r), r
    return out.raw[:r]


def zstd_archive(parts, checksum_table: bool, frame_checksums=(), level=3) -> bytes:
    """libzstd's frames of `parts` (frame i with its own content checksum when i is in frame_checksums) + the table.  None without libzstd"""
    frames = [zstd_frame(p, level, i in frame_checksums) for i, p in enumerate(parts)]
    return None if any(f is None for f in frames) else archive(frames, parts, checksum_table)
