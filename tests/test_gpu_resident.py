"""Device-resident decode (zsmi_decompressBatchResident, k_dec_items): the chain compress -> pack -> sizes -> layout -> decode with no host
step between its calls; item-by-item equality with the host-array call over good, damaged and truncated frames and capacities that are
short or above maxDstCap, at plans of one, two and many block slots; the same with a DDict set; sub-batches over device-built items; the
host checks."""
import ctypes, os
import numpy as np
import pytest
import _batch as B, _corpus as C, _data as D, _dicts as X, _ddict_set as DS, _resident as R
from _hip import hip_of, Dev, CANARY

pytestmark = pytest.mark.gpu


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
def stream_bytes():
    """a few MiB of record classes and text to cut chunks from"""
    return C.json_records(1 << 20) + C.csv_records(1 << 20) + C.binary_table(1 << 20) + D.zipf_log(1 << 20, single=True).tobytes()


def chunks_of(data, sizes, rng):
    return [data[at:at + s] for at, s in ((int(rng.integers(0, len(data) - s)), s) for s in sizes)]


def test_chain_without_a_host_step(codec, H, stream_bytes):
    rng = np.random.default_rng(96)
    sizes = [0, 1, 65535, 65536, 65537, 131072, 131073, 204800] + [int(v) for v in rng.integers(0, 204801, 88)]
    chunks = chunks_of(stream_bytes, sizes, rng)
    n, L = len(chunks), codec.L
    assert n == 96
    src_np, so, ss = B.batch(chunks)
    _, do, bounds, total = B.ragged_device_layout(L, ss, rng)
    align = 64
    room = int(((ss.astype(np.uint64) + align - 1) // align * align).sum())
    src, frames, fsz = R.up(H, src_np), Dev(H, total), Dev(H, 4 * n)
    packed, poff = Dev(H, int(bounds.sum())), Dev(H, 8 * (n + 1))
    content, status = Dev(H, 8 * n), Dev(H, 4 * n)
    caps, ooff = Dev(H, 4 * n), Dev(H, 8 * (n + 1))
    arena, osz = Dev(H, room + 1000), Dev(H, 4 * n)
    # the five calls: the host reads nothing, and waits for nothing, until the last one is queued
    codec.compress_device(src.p, so, ss, frames.p, do, fsz.p)
    codec.pack_device(frames.p, do, fsz.p, n, packed.p, poff.p)
    codec.frame_sizes_device(packed.p, poff.p, fsz.p, n, content.p, 0, status.p)
    codec.layout_outputs_device(content.p, status.p, n, caps.p, ooff.p, align=align)
    codec.decompress_resident(packed.p, poff.p, fsz.p, n, arena.p, ooff.p, caps.p, 204800, osz.p)
    codec.sync()
    got_status, ok = R.down(status, np.uint32)
    assert ok and not got_status.any()
    got_content, ok = R.down(content, np.uint64)
    assert ok and (got_content == ss).all()
    got_caps, ok = R.down(caps, np.uint32)
    assert ok and (got_caps == ss).all()
    got_off, ok = R.down(ooff, np.uint64)
    want_off = B.layout((ss.astype(np.uint64) + align - 1) // align * align)
    assert ok and (got_off[:n] == want_off).all() and int(got_off[n]) == room
    got_sz, ok = R.down(osz, np.uint32)
    assert ok and (got_sz == ss).all(), np.flatnonzero(got_sz != ss)[:8].tolist()
    host, ok = R.down(arena)
    assert ok
    inside = np.zeros(len(host), dtype=bool)
    for i, (o, c) in enumerate(zip(want_off, chunks)):
        assert host[int(o):int(o) + len(c)].tobytes() == c, ("chunk", i, len(c))
        inside[int(o):int(o) + len(c)] = True
    assert (host[~inside] == CANARY).all(), "written outside the laid-out places"
    for d in (src, frames, fsz, packed, poff, content, status, caps, ooff, arena, osz):
        d.free()


# max_cap -> the chunk sizes of its batch: 32 KiB is a plan of one block slot an item, 128 KiB of two, 1 MiB with a quarter of the items
# above 128 KiB of many (the uniform plan takes ZS_FAST_MAXBLOCKS, the host-array call's plan what its own capacities ask)
PLANS = {
    32 << 10: [0, 1, 100, 4097, 20000, 32767, 32768, 32769, 40000] + [3000 + 1237 * i for i in range(23)],
    128 << 10: [0, 7, 65536, 65537, 100000, 131071, 131072, 131073, 150000] + [1000 + 5333 * i for i in range(23)],
    1 << 20: [200000, 300001, 524288, 600000, 1 << 20, (1 << 20) + 1, 262145, 131073] + [50 + 4111 * i for i in range(24)],
}


@pytest.mark.parametrize("max_cap", sorted(PLANS))
def test_items_equal_the_host_array_call(codec, H, stream_bytes, max_cap):
    rng = np.random.default_rng(max_cap)
    chunks = chunks_of(stream_bytes, PLANS[max_cap], rng)
    frames = B.compress_many(codec, chunks)
    items, caps = R.mix(frames, chunks, rng, max_cap)
    sz = R.compare(codec, H, items, caps, max_cap, what=f"maxDstCap {max_cap}")
    # the mix holds what it is there for: successes, dstSize_tooSmall from short and from clamped capacities, other refusals
    codes = {0x100000000 - int(s) for s in sz if s >= B.ERR}
    assert 70 in codes and len(codes) >= 2 and sum(int(s) < B.ERR for s in sz) >= len(chunks) // 2, sorted(codes)
    assert (caps > max_cap).any() and (np.array([len(c) for c in chunks]) > max_cap).any()


def test_items_equal_the_host_array_call_with_a_ddict_set(codec, H):
    from zstandard_amd import DecompressionDict, DecompressionDictSet
    rng = np.random.default_rng(2)
    classes = ("json_records", "xml_records")
    dics = [X.trained(c) for c in classes]
    assert DS.dict_id(dics[0]) != DS.dict_id(dics[1]) and all(DS.dict_id(d) for d in dics)
    frames, chunks = [], []
    for k, cls in enumerate(classes + ("csv_records",)):           # (the third class: frames that name no dictionary)
        cs = chunks_of(X.class_data(cls), [300 + 911 * i for i in range(14)], rng)
        fs = B.compress_many(codec, cs, dic=dics[k] if k < 2 else b"")
        assert all((DS.named_id(f) == DS.dict_id(dics[k])) if k < 2 else DS.id_field(f)[1] == 0 for f in fs)
        frames += fs; chunks += cs
    order = rng.permutation(len(frames))                             # neighbours name different dictionaries
    frames, chunks = [frames[i] for i in order], [chunks[i] for i in order]
    dds = [DecompressionDict(codec, d) for d in dics]
    dset = DecompressionDictSet(codec, dds)
    items, caps = R.mix(frames, chunks, rng, 32 << 10)
    sz = R.compare(codec, H, items, caps, 32 << 10, ddict_set=dset, what="DDict set")
    assert sum(int(s) < B.ERR for s in sz) >= len(chunks) // 2
    # without the set the dictionary frames fail: the set is what decoded them
    plain = R.compare(codec, H, frames, [len(c) for c in chunks], 32 << 10, what="no set")
    assert sum(int(s) >= B.ERR for s in plain) >= 28
    dset.close()
    for dd in dds:
        dd.close()


def test_sub_batches_over_device_built_items():
    """ZSMI_ITEMS_IN_FLIGHT=64 in a child process, 200 items: four sub-batches read the item list k_dec_items wrote"""
    B.run_child("-c", "import sys, os; sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], 'tests')); import _resident; _resident.child(200)",
                B.ROOT, env=dict(os.environ, ZSMI_ITEMS_IN_FLIGHT="64"))


def test_host_checks_in_order(codec, H):
    L = codec.L
    vp = ctypes.c_void_p
    buf = Dev(H, 64)
    p = vp(buf.p)
    call = L.zsmi_decompressBatchResident
    assert call(None, None, None, None, 1, None, None, None, 100, None, None) == 62            # init_missing before anything else
    for k in (0, 1, 2, 4, 5, 6, 8):                                                             # each array in turn: GENERIC
        args = [p, p, p, 1, p, p, p, 100, p]
        args[k] = None
        assert call(codec.ctx, *args, None) == 1, k
    assert call(codec.ctx, None, None, None, 0, None, None, None, 100, None, None) == 0         # n == 0: nothing to do, nothing read
    # a set of another device, where the box has one: after the arrays (GENERIC with a NULL one), before anything is queued
    count = ctypes.c_int(0)
    assert H.hipGetDeviceCount(ctypes.byref(count)) == 0
    if count.value > 1:
        from zstandard_amd import BatchCodec, DecompressionDictSet
        other = BatchCodec(1)
        foreign = DecompressionDictSet(other, [])
        assert call(codec.ctx, p, p, None, 1, p, p, p, 100, p, foreign.handle) == 1
        assert call(codec.ctx, p, p, p, 1, p, p, p, 100, p, foreign.handle) == 40
        foreign.close(); other.close()
    assert L.zsmi_getFrameSizesBatchDevice(None, None, None, None, 1, None, None, None) == 62
    assert L.zsmi_getFrameSizesBatchDevice(codec.ctx, p, p, None, 1, None, None, p) == 1
    assert L.zsmi_getFrameSizesBatchDevice(codec.ctx, p, p, p, 1, None, None, None) == 1
    assert L.zsmi_getFrameSizesBatchDevice(codec.ctx, None, None, None, 0, None, None, None) == 0
    assert L.zsmi_layoutOutputsDevice(None, p, None, 1, 1, p, p) == 62
    for align in (0, 3, 48, 8192, 1 << 31):
        assert L.zsmi_layoutOutputsDevice(codec.ctx, p, None, 1, align, p, p) == 42, align
    codec.sync()
    R.assert_tail_untouched(buf, 0, "the refused calls")
    buf.free()
