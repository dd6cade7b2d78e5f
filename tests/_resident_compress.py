"""Device-resident compress in the GPU tests (test infrastructure): the chunk batches of tests/test_gpu_resident_compress.py and the one
comparison it makes in every setting - zsmi_compressBatchResident, its three descriptor arrays in device memory, against
zsmi_compressBatchDevice with the same arrays from the host: chunk by chunk the same size word and the same frame, nothing written
outside a chunk's place, and for a chunk above max_src_size the refusal's word and no byte beyond zsmi_compressBound(0)."""
import numpy as np
import _batch as B, _corpus as C, _data as D
from _hip import Dev, CANARY
from _resident import up, down

KIB = 1 << 10
REFUSED = 0x100000000 - 72           # (uint32_t)-ZSMI_error_srcSize_wrong
_stream = []


def stream_bytes():
    """a few MiB of record classes and text to cut chunks from (made once)"""
    if not _stream:
        _stream.append(C.json_records(1 << 20) + C.csv_records(1 << 20) + C.binary_table(1 << 20) + D.zipf_log(1 << 20, single=True).tobytes())
    return _stream[0]


# max_src_size -> the sizes of its batch: the edges of the plan's rule (empty chunk, one block, two blocks = one big unit, a big and a
# small unit, two big units) and of the kernels (tiny blocks are raw), then seeded ones
def sizes_of(max_src):
    rng = np.random.default_rng(max_src)
    if max_src == 64 * KIB:
        return [0, 1, 7, 8, 15, 16, 17, 255, 256, 257, 65535, 65536] + [int(v) for v in rng.integers(0, 65537, 20)]
    if max_src == 128 * KIB:
        return [0, 65536, 65537, 131071, 131072] + [int(v) for v in rng.integers(0, 131073, 20)]
    assert max_src == 1 << 20
    big, small, out = [131073, 196608, 196609, 262144, 300001, 1 << 20], [int(v) for v in rng.integers(0, 70000, 20)], []
    for i, s in enumerate(small):                          # the long chunks with small ones between them
        out.append(s)
        if i % 3 == 1 and big:
            out.append(big.pop(0))
    return out + big


def chunks_of(max_src):
    """the batch of max_src: cut from the stream at seeded places; the first seeded chunk of 4 .. 70 KiB is all zeros (RLE blocks), the second
    random bytes (no match: raw blocks, a matchless unit)"""
    rng = np.random.default_rng(max_src + 1)
    data, sizes = stream_bytes(), sizes_of(max_src)
    chunks = [data[at:at + s] for at, s in ((int(rng.integers(0, len(data) - s)), s) for s in sizes)]
    seeded = range(len(sizes) - 20, len(sizes)) if max_src < (1 << 20) else range(len(sizes))
    zeros, noise = [i for i in seeded if 4096 <= sizes[i] <= 70000][:2]
    chunks[zeros] = bytes(sizes[zeros]); chunks[noise] = rng.integers(0, 256, sizes[noise], dtype=np.uint8).tobytes()
    return chunks


class Batch:
    """chunks in device memory with ragged bound-sized places, the descriptors on the host and on the device"""

    def __init__(self, codec, H, chunks, seed=5):
        self.codec, self.H, self.chunks, self.n = codec, H, chunks, len(chunks)
        src_np, self.so, self.ss = B.batch(chunks)
        _, self.do, self.bounds, self.total = B.ragged_device_layout(codec.L, self.ss, np.random.default_rng(seed))
        self.src, self.d_so, self.d_ss, self.d_do = up(H, src_np), up(H, self.so), up(H, self.ss), up(H, self.do)

    def run(self, resident, max_src=0, level=3):
        """(size words, the whole destination buffer) of one call"""
        dst, dsz = Dev(self.H, self.total), Dev(self.H, 4 * self.n)
        if resident:
            self.codec.compress_resident(self.src.p, self.d_so.p, self.d_ss.p, self.n, max_src, dst.p, self.d_do.p, dsz.p, level)
        else:
            self.codec.compress_device(self.src.p, self.so, self.ss, dst.p, self.do, dsz.p, level)
        self.codec.sync()
        host, ok1 = down(dst)
        sz, ok2 = down(dsz, np.uint32)
        assert ok1 and ok2, ("resident" if resident else "host arrays", "a canary around a buffer is gone")
        dst.free(); dsz.free()
        return sz.copy(), host.copy()

    def frames(self, sz, host):
        return [host[int(o):int(o) + (int(s) if s < B.ERR else 0)].tobytes() for o, s in zip(self.do, sz)]

    def free(self):
        for d in (self.src, self.d_so, self.d_ss, self.d_do):
            d.free()


def assert_equal_to_host_call(batch, ref, got, max_src, what=""):
    """got = (sizes, buffer) of the resident call at max_src, ref = the host-array call's on the same batch"""
    (hsz, hbuf), (rsz, rbuf) = ref, got
    bound0 = batch.codec.L.zsmi_compressBound(0)
    inside = np.zeros(batch.total, dtype=bool)
    for o, b in zip(batch.do, batch.bounds):
        inside[int(o):int(o) + int(b)] = True
    bad = np.flatnonzero(~inside & (rbuf != CANARY))
    assert bad.size == 0, (what, "written outside the chunks' places", bad[:8].tolist())
    for i, (o, s, b) in enumerate(zip(batch.do, batch.ss, batch.bounds)):
        o, b = int(o), int(b)
        if int(s) > max_src:
            assert int(rsz[i]) == REFUSED, (what, "chunk above max_src_size", i, hex(int(rsz[i])))
            assert (rbuf[o + bound0:o + b] == CANARY).all(), (what, "a refused chunk's place written beyond compressBound(0)", i)
        else:
            assert int(rsz[i]) == int(hsz[i]) < B.ERR, (what, "size word of chunk", i, int(s), hex(int(hsz[i])), hex(int(rsz[i])))
            # the whole place: the frame, and behind it whatever the host-array call leaves there (nothing: the canary)
            same = rbuf[o:o + b] == hbuf[o:o + b]
            assert same.all(), (what, "frame of chunk", i, int(s), "first difference at", int(np.flatnonzero(~same)[0]))


def child(n=150):
    """run in a process of its own (ZSMI_BLOCKS_IN_FLIGHT=64): n chunks of 0 .. 200 KiB, max_src_size 200 KiB - four blocks a chunk at
    most, so sub-batches of 16 chunks, ten of them, each planned on the device into the lists the one before used"""
    from _hip import hip_of
    from zstandard_amd import BatchCodec
    bc = BatchCodec(0); H = hip_of()
    rng = np.random.default_rng(150)
    data = stream_bytes()
    sizes = [0, 200 * KIB, 1, 65536, 65537, 131072, 131073] + [int(v) for v in rng.integers(0, 200 * KIB + 1, n - 7)]
    order = rng.permutation(n)
    chunks = [data[at:at + s] for at, s in ((int(rng.integers(0, len(data) - s)), s) for s in (sizes[i] for i in order))]
    batch = Batch(bc, H, chunks)
    ref = batch.run(False)
    got = batch.run(True, 200 * KIB)
    assert_equal_to_host_call(batch, ref, got, 200 * KIB, "sub-batches of 16 chunks")
    assert (ref[0] < B.ERR).all()
    batch.free(); bc.close()
    print("CHILD-OK")
