"""The one place the GPU tests (and the tools they run as children) lay a batch out and read it back: chunks -> one source buffer with
offsets and sizes -> a BatchCodec call -> frames, and the way back; the round-trip checks every dictionary test makes; the canary
checks of the device-pointer children; the launch of a child process.  ERR is the library's own limit: a size above it is an error
code, and a frame counts as written only below it."""
import os, subprocess, sys
import numpy as np
import _oracle as O
from zstandard_amd.api import ERROR_MAX as ERR
from _hip import CANARY

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ layout
def layout(sizes, gaps=None):
    """uint64 offsets of items laid one behind the other (the exclusive scan of sizes); gaps[i] bytes are left in front of item i"""
    sizes = np.asarray(sizes, dtype=np.uint64)
    step = sizes if gaps is None else sizes + np.asarray(gaps, dtype=np.uint64)
    return (np.cumsum(step, dtype=np.uint64) - sizes).astype(np.uint64)


def batch(chunks):
    """(src uint8, offsets, sizes) of chunks laid back to back; a batch without a byte still gets a source buffer of one"""
    sizes = np.array([len(c) for c in chunks], dtype=np.uint32)
    return np.frombuffer(b"".join(chunks) or b"\0", dtype=np.uint8), layout(sizes), sizes


def cut(arena, offs, sizes):
    """[bytes] of the items at offs / sizes in arena"""
    return [arena[int(o):int(o) + int(s)].tobytes() for o, s in zip(offs, sizes)]


def frames_of(result, n=None):
    """the first n frames of a compress_host result (arena, offsets, sizes): every size must be a success"""
    arena, do, dsz = result
    n = len(dsz) if n is None else n
    failed = np.flatnonzero(dsz[:n] >= ERR)
    assert failed.size == 0, [(int(i), hex(int(dsz[i]))) for i in failed[:5]]
    return cut(arena, do[:n], dsz[:n])


def first_difference(a, b):
    return next((k for k in range(min(len(a), len(b))) if a[k] != b[k]), min(len(a), len(b)))


# ------------------------------------------------------------------ chunks -> frames -> chunks
def compress_many(codec, chunks, level=3, dic=b"", cdict=None):
    """one compress_host call: with a dictionary for every chunk, or with a CompressionDict (whose level holds)"""
    src, offs, sizes = batch(chunks)
    res = codec.compress_host(src, offs, sizes, level, dic) if cdict is None else codec.compress_host(src, offs, sizes, cdict=cdict)
    return frames_of(res, len(chunks))


def decode_many(codec, frames, caps, dic=b"", min_cap=1):
    """one decompress_host call -> [(size or error word, bytes)]; an error gives b"".  Capacities are raised to min_cap (0: as given)"""
    src, offs, sizes = batch(frames)
    out, oo, osz = codec.decompress_host(src, offs, sizes, np.maximum(np.array(caps, dtype=np.uint32), min_cap), dic)
    return [(int(s), out[int(o):int(o) + (int(s) if s < ERR else 0)].tobytes()) for o, s in zip(oo, osz)]


def oracle_frames(chunks, level, dic=b"", threads=8):
    """oracle E's frames for a batch, through its batch form (with one dictionary for every chunk, or none)"""
    src, offs, sizes = batch(chunks)
    return cut(*O.compress_batch(src, offs, sizes, level, threads, dic or None))


def assert_round_trip(codec, frames, chunks, dic, what=""):
    """every frame within zsmi_compressBound; decodes to its chunk with the dictionary under oracle D, the library's decoder and libzstd"""
    import _dicts as X                                   # (here, not at the top: the tools that use layout / cut need none of its fixtures)
    bound = codec.L.zsmi_compressBound
    for i, (f, c) in enumerate(zip(frames, chunks)):
        assert len(f) <= bound(len(c)), (what, i)
        assert O.decompress_using_dict(f, len(c), dic) == c, (what, "oracle D", i, len(c))
    for i, ((sz, got), c) in enumerate(zip(decode_many(codec, frames, [len(c) for c in chunks], dic), chunks)):
        assert sz == len(c) and got == c, (what, "zsmi_decompressBatchHost_usingDict", i, len(c), hex(sz))
    if X.zstd():
        for i, (f, c) in enumerate(zip(frames, chunks)):
            assert X.zstd_decompress_dict(f, len(c), dic) == c, (what, "libzstd", i, len(c))


# ------------------------------------------------------------------ device-pointer children
def ragged_device_layout(L, sizes, rng):
    """(src offsets, dst offsets, bounds, total) for chunks of these sizes: sources back to back, every destination zsmi_compressBound
    long with a gap of 0 .. 299 bytes in front of every second one, 4 KiB behind the last"""
    bounds = np.array([L.zsmi_compressBound(int(s)) for s in sizes], dtype=np.uint64)
    do = layout(bounds, rng.integers(0, 300, len(sizes)) * (np.arange(len(sizes)) % 2))
    return layout(sizes), do, bounds, int(do[-1]) + int(bounds[-1]) + 4096


def assert_only_frames_written(host, dst_offs, sizes, bounds, canary=CANARY, what=""):
    """every size within its bound, and no byte of host outside [dst_offs[i], dst_offs[i] + sizes[i]) differs from the canary"""
    inside = np.zeros(len(host), dtype=bool)
    for i, (o, s, b) in enumerate(zip(dst_offs, sizes, bounds)):
        assert int(s) <= int(b), (what, i, "size above its bound", int(s), int(b))
        inside[int(o):int(o) + int(s)] = True
    bad = np.flatnonzero(~inside & (host != canary))
    assert bad.size == 0, (what, "written outside the frames", bad[:10].tolist())


# ------------------------------------------------------------------ child processes
class ChildFailed(AssertionError):
    """a child that did not end as it must; returncode: its exit status (negative: ended by that signal)"""

    def __init__(self, returncode, detail):
        super().__init__(returncode, *detail)
        self.returncode = returncode


def run_child(*argv, env=None, timeout=600, marker="CHILD-OK", cwd=None):
    """a fresh Python process with these arguments: a file's path and its arguments, or "-c", a script's text and its arguments.  It must
    exit with 0 and, unless marker is None, print the marker (else ChildFailed, an AssertionError; a child that outlives `timeout` is
    killed and subprocess.TimeoutExpired raised).  Returns its stdout."""
    r = subprocess.run([sys.executable, *argv], env=env, cwd=cwd, capture_output=True, text=True, timeout=timeout)
    if not (r.returncode == 0 and (marker is None or marker in r.stdout)):
        raise ChildFailed(r.returncode, (r.stdout[-2000:], r.stderr[-3000:]))
    return r.stdout
