"""Device-resident compress (zsmi_compressBoundsDevice, zsmi_compressBatchResident; the plan built by k_plan_chunks / k_plan_blocks):
chunk-by-chunk equality with the host-array call at three levels and three plans, with the checksum flag, with chunks above
maxSrcSize, over ten sub-batches; the chain bounds -> layout -> compress -> pack -> sizes -> layout -> decode with no host step; a
resident call between two host-array calls; the host checks."""
import ctypes, os
import numpy as np
import pytest
import _batch as B, _checksum as CK, _oracle as O, _resident as R, _resident_compress as RC
from _hip import hip_of, Dev, CANARY

pytestmark = pytest.mark.gpu
KIB = 1 << 10
PLANS = (64 * KIB, 128 * KIB, 1 << 20)


@pytest.fixture(scope="module")
def codec():
    from zstandard_amd import BatchCodec
    bc = BatchCodec(0)
    yield bc
    bc.close()


@pytest.fixture(scope="module")
def H():
    return hip_of()


@pytest.fixture(scope="module")
def batches(codec, H):
    """max_src_size -> its batch in device memory, and (level, checksum) -> the host-array call's result on it: computed once, shared"""
    made = {m: RC.Batch(codec, H, RC.chunks_of(m)) for m in PLANS}
    refs = {}

    def get(max_src, level=3, checksum=0):
        key = (max_src, level, checksum)
        if key not in refs:
            assert codec.get_parameter("checksum") == checksum
            refs[key] = made[max_src].run(False, level=level)
        return made[max_src], refs[key]
    yield get
    for b in made.values():
        b.free()


@pytest.mark.parametrize("level", (1, 3, 4))
@pytest.mark.parametrize("max_src", PLANS)
def test_frames_equal_the_host_array_call(codec, batches, max_src, level):
    batch, ref = batches(max_src, level)
    assert int(batch.ss.max()) == max_src and (ref[0] < B.ERR).all()
    got = batch.run(True, max_src, level)
    RC.assert_equal_to_host_call(batch, ref, got, max_src, f"maxSrcSize {max_src}, level {level}")
    if level == 3:
        for i, (f, c) in enumerate(zip(batch.frames(*got), batch.chunks)):
            assert O.decompress(f, len(c)) == c, ("oracle D", max_src, i, len(c))


@pytest.mark.parametrize("max_src", PLANS)
def test_frames_equal_the_host_array_call_with_checksums(codec, batches, max_src):
    plain = batches(max_src)[1]
    codec.set_parameter("checksum", 1)
    try:
        batch, ref = batches(max_src, 3, 1)
        got = batch.run(True, max_src)
    finally:
        codec.set_parameter("checksum", 0)
    RC.assert_equal_to_host_call(batch, ref, got, max_src, f"checksums, maxSrcSize {max_src}")
    for i, (f, p, c) in enumerate(zip(batch.frames(*got), batch.frames(*plain), batch.chunks)):
        assert f == CK.with_checksum(p, c), (max_src, i, len(c))


@pytest.mark.parametrize("max_src,told", ((128 * KIB, 64 * KIB), (1 << 20, 128 * KIB), (64 * KIB, 255), (64 * KIB, 0)))
def test_chunks_above_max_src_size(codec, batches, max_src, told):
    """the batch of max_src with a smaller number told to the call: the chunks above it are refused in place, every other chunk's frame is
    the reference's"""
    batch, ref = batches(max_src)
    above = int((batch.ss > told).sum())
    assert 0 < above < batch.n
    got = batch.run(True, told)
    RC.assert_equal_to_host_call(batch, ref, got, told, f"maxSrcSize {told} over the batch of {max_src}")
    assert int((got[0] == RC.REFUSED).sum()) == above


def test_chunks_above_max_src_size_with_checksums(codec, batches):
    codec.set_parameter("checksum", 1)
    try:
        batch, ref = batches(128 * KIB, 3, 1)
        got = batch.run(True, 64 * KIB)
    finally:
        codec.set_parameter("checksum", 0)
    RC.assert_equal_to_host_call(batch, ref, got, 64 * KIB, "checksums, chunks above maxSrcSize")


def test_sub_batches_planned_on_the_device():
    """ZSMI_BLOCKS_IN_FLIGHT=64 in a child process, 150 chunks of up to 200 KiB: ten sub-batches of 16 chunks"""
    B.run_child("-c", "import sys, os; sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], 'tests')); import _resident_compress; _resident_compress.child(150)",
                B.ROOT, env=dict(os.environ, ZSMI_BLOCKS_IN_FLIGHT="64"))


def test_chain_without_a_host_step(codec, H):
    """sizes and offsets go up once; bounds, layout, compress, pack, frame sizes, layout, decode are queued one behind the other and
    waited for once.  (pack_device takes the frames' offsets from the host: this test computes them as the device does.)"""
    rng = np.random.default_rng(96)
    sizes = [0, 1, 65535, 65536, 65537, 131072, 131073, 204800] + [int(v) for v in rng.integers(0, 204801, 88)]
    data = RC.stream_bytes()
    chunks = [data[at:at + s] for at, s in ((int(rng.integers(0, len(data) - s)), s) for s in sizes)]
    n, L = len(chunks), codec.L
    assert n == 96
    src_np, so, ss = B.batch(chunks)
    align = 64
    bounds = np.array([L.zsmi_compressBound(int(s)) for s in ss], dtype=np.uint64)
    want_fo = B.layout((bounds + align - 1) // align * align)
    frame_room = int(want_fo[-1]) + int(bounds[-1]) + align
    room = int(((ss.astype(np.uint64) + align - 1) // align * align).sum())
    src, d_so, d_ss = R.up(H, src_np), R.up(H, so), R.up(H, ss)
    d_bounds, fcaps, foff = Dev(H, 8 * n), Dev(H, 4 * n), Dev(H, 8 * (n + 1))
    frames, fsz = Dev(H, frame_room), Dev(H, 4 * n)
    packed, poff = Dev(H, int(bounds.sum())), Dev(H, 8 * (n + 1))
    content, status = Dev(H, 8 * n), Dev(H, 4 * n)
    caps, ooff = Dev(H, 4 * n), Dev(H, 8 * (n + 1))
    arena, osz = Dev(H, room + 1000), Dev(H, 4 * n)
    codec.compress_bounds_device(d_ss.p, n, d_bounds.p)
    codec.layout_outputs_device(d_bounds.p, 0, n, fcaps.p, foff.p, align=align)
    codec.compress_resident(src.p, d_so.p, d_ss.p, n, 204800, frames.p, foff.p, fsz.p)
    codec.pack_device(frames.p, want_fo, fsz.p, n, packed.p, poff.p)
    codec.frame_sizes_device(packed.p, poff.p, fsz.p, n, content.p, 0, status.p)
    codec.layout_outputs_device(content.p, status.p, n, caps.p, ooff.p, align=align)
    codec.decompress_resident(packed.p, poff.p, fsz.p, n, arena.p, ooff.p, caps.p, 204800, osz.p)
    codec.sync()
    got_bounds, ok = R.down(d_bounds, np.uint64)
    assert ok and (got_bounds == bounds).all()
    got_fcaps, ok = R.down(fcaps, np.uint32)
    assert ok and (got_fcaps == bounds).all()
    got_fo, ok = R.down(foff, np.uint64)
    assert ok and (got_fo[:n] == want_fo).all()
    got_fsz, ok = R.down(fsz, np.uint32)
    assert ok and (got_fsz <= bounds).all()
    got_status, ok = R.down(status, np.uint32)
    assert ok and not got_status.any()
    got_content, ok = R.down(content, np.uint64)
    assert ok and (got_content == ss).all()
    got_sz, ok = R.down(osz, np.uint32)
    assert ok and (got_sz == ss).all(), np.flatnonzero(got_sz != ss)[:8].tolist()
    got_off, ok = R.down(ooff, np.uint64)
    want_off = B.layout((ss.astype(np.uint64) + align - 1) // align * align)
    assert ok and (got_off[:n] == want_off).all() and int(got_off[n]) == room
    host, ok = R.down(arena)
    assert ok
    inside = np.zeros(len(host), dtype=bool)
    for i, (o, c) in enumerate(zip(want_off, chunks)):
        assert host[int(o):int(o) + len(c)].tobytes() == c, ("chunk", i, len(c))
        inside[int(o):int(o) + len(c)] = True
    assert (host[~inside] == CANARY).all(), "written outside the laid-out places"
    fhost, ok = R.down(frames)
    assert ok
    B.assert_only_frames_written(fhost, want_fo, got_fsz, bounds, what="the frames of the chain")
    for d in (src, d_so, d_ss, d_bounds, fcaps, foff, frames, fsz, packed, poff, content, status, caps, ooff, arena, osz):
        d.free()


def test_resident_call_between_two_host_array_calls(codec, batches):
    """a host-array call, a resident call with another layout, the first host-array call again (its plan is still the context's): all
    three right"""
    a, ref_a = batches(64 * KIB)
    b, ref_b = batches(128 * KIB)
    first = a.run(False)
    between = b.run(True, 128 * KIB)
    again = a.run(False)
    RC.assert_equal_to_host_call(b, ref_b, between, 128 * KIB, "the resident call in between")
    for what, got in (("before", first), ("after", again)):
        assert (got[0] == ref_a[0]).all() and (got[1] == ref_a[1]).all(), ("the host-array call", what)
    for f, c in zip(a.frames(*again), a.chunks):
        assert O.decompress(f, len(c)) == c


def test_host_checks_in_order(codec, H):
    L = codec.L
    buf = Dev(H, 64)
    p = ctypes.c_void_p(buf.p)
    call = L.zsmi_compressBatchResident
    assert call(None, None, None, None, 1, 100, None, None, None, 3) == 62                      # init_missing before anything else
    for k in (0, 1, 2, 5, 6, 7):                                                                # each pointer in turn: GENERIC
        args = [p, p, p, 1, 100, p, p, p, 3]
        args[k] = None
        assert call(codec.ctx, *args) == 1, k
    assert call(codec.ctx, None, None, None, 0, 100, None, None, None, 3) == 0                  # n == 0: nothing to do, nothing read
    assert L.zsmi_compressBoundsDevice(None, p, 1, p) == 62
    assert L.zsmi_compressBoundsDevice(codec.ctx, None, 1, p) == 1
    assert L.zsmi_compressBoundsDevice(codec.ctx, p, 1, None) == 1
    assert L.zsmi_compressBoundsDevice(codec.ctx, None, 0, None) == 0
    codec.sync()
    R.assert_tail_untouched(buf, 0, "the refused calls")
    buf.free()
