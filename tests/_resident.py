"""Device-resident decode in the GPU tests (test infrastructure): numpy arrays to device buffers with canaries and back, and the one
comparison tests/test_gpu_resident.py makes in every setting - zsmi_decompressBatchResident, its descriptors in device memory, against
zsmi_decompressBatchDevice[_usingDDictSet] with the same descriptors from the host and the capacities min(caps, max_cap): item by item the
same size or error word, the same bytes, and nothing written outside an item's place."""
import numpy as np
import _batch as B
from _hip import Dev, CANARY, PAD


def up(H, arr):
    """a numpy array's bytes in a canary-padded device buffer"""
    a = np.ascontiguousarray(arr)
    return Dev(H, max(a.nbytes, 1), a.tobytes())


def down(dev, dtype=np.uint8):
    """(the buffer's own bytes as dtype, whether the canaries on both sides of it are intact)"""
    raw = np.frombuffer(dev.all(), dtype=np.uint8)
    body = raw[PAD:PAD + dev.n]
    pads_ok = bool((raw[:PAD] == CANARY).all() and (raw[PAD + dev.n:] == CANARY).all())
    vals = body[:dev.n - dev.n % np.dtype(dtype).itemsize].view(dtype)
    return vals, pads_ok


def assert_tail_untouched(dev, used_bytes, what=""):
    """nothing of the buffer behind its first used_bytes, nor its pads, differs from the canary"""
    raw = np.frombuffer(dev.all(), dtype=np.uint8)
    assert (raw[:PAD] == CANARY).all() and (raw[PAD + used_bytes:] == CANARY).all(), (what, "written outside its entries")


def mix(frames, contents, rng, max_cap):
    """(items, caps) from good frames and their contents: every fifth frame also with one byte flipped, every seventh cut short, and
    capacities that are ample, exact, one byte short (dstSize_tooSmall, 70) or above max_cap (clamped)"""
    items, caps = [], []
    for i, (f, c) in enumerate(zip(frames, contents)):
        kind = i % 4
        cap = len(c) + 100 if kind == 0 else len(c) if kind == 1 else max(len(c) - 1, 0) if kind == 2 else max_cap + 1 + 977 * i
        items.append(f); caps.append(cap)
        if i % 5 == 0 and len(f) > 12:
            g = bytearray(f); at = int(rng.integers(4, len(f))); g[at] ^= 1 << int(rng.integers(0, 8))
            items.append(bytes(g)); caps.append(len(c) + 64)
        if i % 7 == 0 and len(f) > 12:
            items.append(f[:int(rng.integers(1, len(f)))]); caps.append(len(c) + 64)
    return items, np.array(caps, dtype=np.uint32)


def compare(codec, H, items, caps, max_cap, ddict_set=None, what=""):
    """both calls on the same items; returns the size words.  The places are min(caps, max_cap) long with gaps between them."""
    n = len(items)
    src_np, so, ss = B.batch(items)
    caps = np.asarray(caps, dtype=np.uint32)
    eff = np.minimum(caps, np.uint32(max_cap))
    do = B.layout(eff, [7 + 3 * (i % 5) for i in range(n)])
    total = int(do[-1]) + int(eff[-1]) + 64
    src = up(H, src_np)
    d_so, d_ss, d_do, d_caps = up(H, so), up(H, ss), up(H, do), up(H, caps)
    results = []
    for resident in (False, True):
        dst, dsz = Dev(H, total), Dev(H, 4 * n)
        if resident:
            codec.decompress_resident(src.p, d_so.p, d_ss.p, n, dst.p, d_do.p, d_caps.p, max_cap, dsz.p, ddict_set=ddict_set)
        else:
            codec.decompress_device(src.p, so, ss, dst.p, do, eff, dsz.p, ddict_set=ddict_set)
        codec.sync()
        host, ok1 = down(dst)
        sz, ok2 = down(dsz, np.uint32)
        assert ok1 and ok2, (what, resident, "a canary around a buffer is gone")
        inside = np.zeros(total, dtype=bool)
        for o, c in zip(do, eff):
            inside[int(o):int(o) + int(c)] = True
        bad = np.flatnonzero(~inside & (host != CANARY))
        assert bad.size == 0, (what, resident, "written outside the items' places", bad[:8].tolist())
        results.append((sz.copy(), [host[int(o):int(o) + (int(s) if s < B.ERR else 0)].tobytes() for o, s in zip(do, sz)]))
        dst.free(); dsz.free()
    for d in (src, d_so, d_ss, d_do, d_caps):
        d.free()
    (hsz, hbytes), (rsz, rbytes) = results
    differ = np.flatnonzero(hsz != rsz)
    assert differ.size == 0, (what, "size or error word", [(int(i), hex(int(hsz[i])), hex(int(rsz[i]))) for i in differ[:8]])
    for i in range(n):
        assert hbytes[i] == rbytes[i], (what, "bytes of item", i)
    return rsz


def child(n=200):
    """run in a process of its own (ZSMI_ITEMS_IN_FLIGHT=64): n items, so that the sub-batch loop turns over device-built items"""
    import _data as D
    from _hip import hip_of
    from zstandard_amd import BatchCodec
    bc = BatchCodec(0); H = hip_of()
    z = D.zipf_log(300000, single=True).tobytes()
    chunks = [z[911 * i:911 * i + 200 + 157 * i] for i in range(n)]
    frames = B.compress_many(bc, chunks)
    caps = np.array([len(c) - (i % 9 == 4) for i, c in enumerate(chunks)], dtype=np.uint32)
    sz = compare(bc, H, frames, caps, 32768, what="sub-batches of 64")
    want = np.array([len(c) if i % 9 != 4 else 0x100000000 - 70 for i, c in enumerate(chunks)], dtype=np.uint32)
    assert (sz == want).all(), np.flatnonzero(sz != want)[:8].tolist()
    bc.close()
    print("CHILD-OK")
