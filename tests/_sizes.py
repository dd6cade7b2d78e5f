"""The items of the size-query tests (test infrastructure): a deterministic list of (name, bytes) built from sources already in the
tree - the libzstd fixture frames and _framewriter - that tests/golden/gen_fixtures_sizes.py puts to libzstd and the tests rebuild;
the recorded answers (tests/golden/libzstd_sizes.json); the two-frame item whose prefixes the tests cut; the walker's answers through
the library's own host calls."""
import glob, hashlib, json, os
import numpy as np
import _framewriter as W
from _data import GOLDEN

UNKNOWN, ERROR = (1 << 64) - 1, (1 << 64) - 2
SIZES_JSON = os.path.join(GOLDEN, "libzstd_sizes.json")
WINDOWS = {"1k": (0, 0), "16k": (4, 0), "8m": (13, 0)}            # (exponent, mantissa): 1 KiB, 16 KiB, 8 MiB


def _payload(k, n):
    return bytes((k * 37 + j * 11) & 0xFF for j in range(n))


def _blocks(kind, count):
    """`count` blocks of one kind, every one a different size below 1 KiB (the smallest window)"""
    if kind == "raw":
        return [W.raw(_payload(k, 40 + 13 * k)) for k in range(count)]
    if kind == "rle":
        return [W.rle(0x41 + k, 100 + 50 * k) for k in range(count)]
    return [W.comp(W.Lit("raw", _payload(k, 60 + 7 * k))) for k in range(count)]


def unsized_frame(window, kind, count, checksum=False):
    """a frame that states no content size: not single-segment, its window from the descriptor"""
    return W.frame(_blocks(kind, count), fcs=None, single=False, window=WINDOWS[window], checksum=checksum)[0]


def sized_frame(k, n, checksum=False):
    """a small single-segment frame of one raw block that states its n bytes"""
    return W.frame([W.raw(_payload(k, n))], checksum=checksum)[0]


def fixture_frames():
    """name -> frame: every frame of the libzstd fixture files"""
    out = {}
    for fn in sorted(glob.glob(os.path.join(GOLDEN, "libzstd_fixtures*.npz"))):
        z = np.load(fn)
        tag = os.path.basename(fn)[len("libzstd_fixtures"):-len(".npz")].strip("_") or "base"
        for k in z.files:
            if k.startswith("frame_") or k.endswith("_frame"):
                out[f"fx_{tag}_{k}"] = z[k].tobytes()
    return out


def two_frame_item():
    """two small frames, the second with a checksum: the item whose prefixes the tests cut"""
    return sized_frame(1, 21) + sized_frame(2, 34, checksum=True)


def items():
    """[(name, bytes)]: the items libzstd was asked about, in a fixed order"""
    out = list(fixture_frames().items())
    for w in WINDOWS:
        for kind in ("raw", "rle", "comp"):
            for count in (1, 2, 5):
                out.append((f"unsized_{w}_{kind}_{count}", unsized_frame(w, kind, count)))
    a, b, c = sized_frame(3, 10), unsized_frame("16k", "raw", 2), sized_frame(4, 300)
    skip = W.skippable(b"skipped bytes", nibble=7)
    out += [("concat2_sized", a + c), ("concat2_mixed", a + b), ("concat3", a + c + a), ("concat3_unsized_last", c + a + b),
            ("skip_before", skip + a), ("skip_between", a + skip + c), ("skip_after", a + skip), ("skip_every", skip + a + skip + b + skip),
            ("skip_alone", skip), ("skip_empty", W.skippable(b"")),
            ("checksum_sized", sized_frame(5, 77, checksum=True)), ("checksum_unsized", unsized_frame("1k", "comp", 2, checksum=True)),
            ("two_frames_second_checksum", two_frame_item())]
    assert len({n for n, _ in out}) == len(out)
    return out


def recorded():
    """name -> {"sha256", "find_decompressed_size", "find_frame_compressed_size", "decompress_bound"}: libzstd's answers"""
    return {r["name"]: r for r in json.load(open(SIZES_JSON))["items"]}


def sha(b):
    return hashlib.sha256(b).hexdigest()


# ------------------------------------------------------------------ the library's host calls
def host_answers(L, item):
    """(content size, bound, status) of an item as the library's host calls give them: the two sums, and the code of the first frame
    zsmi_findFrameCompressedSize refuses going through the item frame by frame (72 for bytes left over) - the walker's status"""
    content, bound = int(L.zsmi_findDecompressedSize(item, len(item))), int(L.zsmi_decompressBound(item, len(item)))
    pos, status = 0, 0
    while len(item) - pos >= 5:
        rest = item[pos:]
        r = L.zsmi_findFrameCompressedSize(rest, len(rest))
        if L.zsmi_isError(r):
            status = L.zsmi_getErrorCode(r)
            break
        pos += r
    if not status and pos != len(item):
        status = 72
    return content, bound, status
