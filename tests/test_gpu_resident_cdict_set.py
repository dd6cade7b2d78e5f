"""Device-resident compress with a CDict set (zsmi_compressBatchResident_usingCDictSet; the plan with a prefixed unit list built by
k_plan_chunks / k_plan_blocks from a dictionary index in device memory): chunk-by-chunk equality with the host-array set call at two
levels and two plans, the refusals only the device can make, one member without an index against the _usingCDict call, the checksum
flag, ten sub-batches, the chain bounds -> layout -> compress -> pack -> sizes -> layout -> decode with a DDict set and no host step,
the plain resident call on the shared kernels, the host checks.  Helpers: tests/_resident_cdict_set.py."""
import ctypes, os
import numpy as np
import pytest
import _batch as B, _checksum as CK, _dicts as X, _resident as R, _resident_compress as RC, _resident_cdict_set as RS
from _hip import hip_of, Dev, CANARY

pytestmark = pytest.mark.gpu
KIB = 1 << 10
PLANS = (64 * KIB, 200 * KIB)
NO_DICT = RS.NO_DICT


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
def sets(codec):
    """level -> (CompressionDictSet, its CompressionDicts), made once"""
    made = {}

    def get(level):
        if level not in made:
            made[level] = RS.make_set(codec, level)
        return made[level]
    yield get
    codec.sync()
    for cset, cds in made.values():
        cset.close()
        for cd in set(cds):
            cd.close()


@pytest.fixture(scope="module")
def batches(codec, H, sets):
    """max_src_size -> its batch in device memory, and (level, checksum) -> the host-array set call's result on it: computed once, shared"""
    made = {m: RS.Batch(codec, H, RS.every_kind_at_every_size(m)) for m in PLANS}
    refs = {}

    def get(max_src, level=3, checksum=0):
        key = (max_src, level, checksum)
        if key not in refs:
            assert codec.get_parameter("checksum") == checksum
            refs[key] = made[max_src].run_set(False, sets(level)[0])
        return made[max_src], refs[key]
    yield get
    for b in made.values():
        b.free()


# ------------------------------------------------------------------ 1. byte identity with the host-array call
@pytest.mark.parametrize("level", (1, 3))
@pytest.mark.parametrize("max_src", PLANS)
def test_frames_equal_the_host_array_set_call(codec, batches, sets, max_src, level):
    batch, ref = batches(max_src, level)
    assert int(batch.ss.max()) == max_src and (ref[0] < B.ERR).all()
    for s in (s for s in RS.S.SIZES_EVERY_KIND_HAS if s <= max_src):               # every kind of choice meets every size that fits
        assert {int(i) for i in batch.index[batch.ss == s]} >= set(RS.KINDS.values()), s
    got = batch.run_set(True, sets(level)[0], max_src)
    RC.assert_equal_to_host_call(batch, ref, got, max_src, f"a set, maxSrcSize {max_src}, level {level}")
    # the frames name their dictionaries: a formatted member's ID, none for the others
    ids = [cd.dict_id for cd in sets(level)[1]]
    for i, f in enumerate(batch.frames(*got)):
        ch = int(batch.index[i])
        assert RS.frame_dict_id(f) == (0 if ch == NO_DICT else ids[ch]), (i, ch)
    assert ids[RS.KINDS["formatted"]] != 0 and ids[RS.KINDS["raw"]] == 0 and ids[RS.KINDS["empty"]] == 0


# ------------------------------------------------------------------ 2. refusals
def test_refusals_of_size_and_index(codec, batches, sets):
    """the batch of 200 KiB told 131073: its 200 KiB chunks are above it.  One of them, and three chunks that fit, get other indices: the
    member count, 0xFFFFFFFE, and the member count on a chunk above max_src_size (both faults: the size's word)"""
    batch, _ = batches(200 * KIB)
    cset = sets(3)[0]
    told = 131073
    above = [int(i) for i in np.flatnonzero(batch.ss > told)]
    fits = [int(i) for i in np.flatnonzero((batch.ss > 0) & (batch.ss <= 65536))]
    assert len(above) >= 5 and len(fits) > 20
    index = batch.index.copy()
    count_at, big_at, both_at = fits[3], fits[10], above[1]
    index[count_at] = len(RS.SET); index[big_at] = 0xFFFFFFFE; index[both_at] = len(RS.SET)
    accepted = index.copy()
    accepted[[count_at, big_at, both_at]] = NO_DICT                                  # (what the host-array call takes: it refuses such an index whole)
    ref = batch.run_set(False, cset, index=accepted)
    got = batch.run_set(True, cset, told, index=index)
    refused = {i: RS.SIZE_REFUSED for i in above}
    refused.update({count_at: RS.INDEX_REFUSED, big_at: RS.INDEX_REFUSED})
    assert refused[above[0]] == 0x100000000 - 72 and refused[count_at] == 0x100000000 - 42 and refused[both_at] == 0x100000000 - 72
    RS.assert_equal_with_refusals(batch, ref, got, refused, "refusals")
    assert int((got[0] >= B.ERR).sum()) == len(above) + 2


# ------------------------------------------------------------------ 3. one member, no index
def test_one_member_and_a_null_index_is_the_cdict_call(codec, H, sets):
    from zstandard_amd import CompressionDictSet
    cd = sets(3)[1][RS.KINDS["formatted"]]
    dic = RS.dictionaries()[RS.KINDS["formatted"]]
    chunks = X.prefix_chunks(dic, (1024, 4096, 65536, 65537))
    assert [len(c) for c in chunks[:4]] == [1024, 4096, 65536, 65537]
    one = CompressionDictSet(codec, [cd], 3)
    batch = RS.Batch(codec, H, [(c, 0) for c in chunks])
    ref = batch.run_set(False, None, cdict=cd)                                        # zsmi_compressBatchDevice_usingCDict
    got = batch.run_set(True, one, 65537, null_index=True)
    RC.assert_equal_to_host_call(batch, ref, got, 65537, "one member, NULL index")
    assert all(RS.frame_dict_id(f) == cd.dict_id != 0 for f in batch.frames(*got))
    # the same with the index spelled out
    again = batch.run_set(True, one, 65537)
    assert (again[0] == got[0]).all() and (again[1] == got[1]).all()
    # a NULL index with another member count: GENERIC, before anything is queued
    dst, dsz = Dev(H, batch.total), Dev(H, 4 * batch.n)
    call = codec.L.zsmi_compressBatchResident_usingCDictSet
    p = ctypes.c_void_p
    assert call(codec.ctx, p(batch.src.p), p(batch.d_so.p), p(batch.d_ss.p), batch.n, 65537, p(dst.p), p(batch.d_do.p), p(dsz.p), sets(3)[0].handle, None) == 1
    codec.sync()
    R.assert_tail_untouched(dst, 0, "a refused call"); R.assert_tail_untouched(dsz, 0, "a refused call")
    dst.free(); dsz.free()
    codec.sync(); one.close(); batch.free()


# ------------------------------------------------------------------ 4. checksum flag
def test_frames_equal_the_host_array_set_call_with_checksums(codec, batches, sets):
    max_src = 64 * KIB
    plain = batches(max_src)[1]
    codec.set_parameter("checksum", 1)
    try:
        batch, ref = batches(max_src, 3, 1)
        got = batch.run_set(True, sets(3)[0], max_src)
    finally:
        codec.set_parameter("checksum", 0)
    RC.assert_equal_to_host_call(batch, ref, got, max_src, "a set, checksums")
    assert (got[0] == plain[0] + 4).all()                                             # each frame 4 bytes longer than with the flag off
    for i, (f, p, c) in enumerate(zip(batch.frames(*got), batch.frames(*plain), batch.chunks)):
        assert f == CK.with_checksum(p, c), (i, len(c))                               # the flag in the descriptor, the same frame, XXH64's low 4 bytes behind it


# ------------------------------------------------------------------ 5. sub-batches
def test_sub_batches_planned_on_the_device_with_a_set():
    """ZSMI_BLOCKS_IN_FLIGHT=64 in a child process, 150 chunks of up to 200 KiB with seeded choices: ten sub-batches of 16 chunks"""
    B.run_child("-c", "import sys, os; sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], 'tests')); import _resident_cdict_set; _resident_cdict_set.child(150)",
                B.ROOT, env=dict(os.environ, ZSMI_BLOCKS_IN_FLIGHT="64"))


# ------------------------------------------------------------------ 6. the chain
def test_chain_with_dictionaries_and_no_host_step(codec, H, sets):
    """sizes, offsets and the choice go up once; bounds, layout, compress with the CDict set, pack, frame sizes, layout, decode with the
    matching DDict set are queued one behind the other and waited for once.  (pack_device takes the frames' offsets from the host: this
    test computes them as the device does.)  The choices: the formatted members (the frames name them), NO_DICT and the empty member"""
    from zstandard_amd import DecompressionDict, DecompressionDictSet
    cset, cds = sets(3)
    dics = RS.dictionaries()
    formatted = [k for k, name in enumerate(RS.SET) if name in ("trained8k", "id_0xffffffff", "trained64k_json_records")]
    assert len({cds[k].dict_id for k in formatted} - {0}) == 3
    dds = [DecompressionDict(codec, dics[k]) for k in formatted]
    dset = DecompressionDictSet(codec, dds)
    picks = formatted + [RS.SET.index("again"), RS.SET.index("empty"), NO_DICT]
    rng = np.random.default_rng(97)
    sizes = [0, 1, 65535, 65536, 65537, 131072, 131073, 204800] + [int(v) for v in rng.integers(0, 65537, 60)] + [int(v) for v in rng.integers(0, 204801, 28)]
    data = RC.stream_bytes()
    chunks = [data[at:at + s] for at, s in ((int(rng.integers(0, len(data) - s)), s) for s in sizes)]
    index = np.array([picks[k % len(picks)] for k in range(len(chunks))], dtype=np.uint32)
    n, L = len(chunks), codec.L
    assert n == 96
    src_np, so, ss = B.batch(chunks)
    align = 64
    bounds = np.array([L.zsmi_compressBound(int(s)) for s in ss], dtype=np.uint64)
    want_fo = B.layout((bounds + align - 1) // align * align)
    frame_room = int(want_fo[-1]) + int(bounds[-1]) + align
    room = int(((ss.astype(np.uint64) + align - 1) // align * align).sum())
    src, d_so, d_ss, d_index = R.up(H, src_np), R.up(H, so), R.up(H, ss), R.up(H, index)
    d_bounds, fcaps, foff = Dev(H, 8 * n), Dev(H, 4 * n), Dev(H, 8 * (n + 1))
    frames, fsz = Dev(H, frame_room), Dev(H, 4 * n)
    packed, poff = Dev(H, int(bounds.sum())), Dev(H, 8 * (n + 1))
    content, status = Dev(H, 8 * n), Dev(H, 4 * n)
    caps, ooff = Dev(H, 4 * n), Dev(H, 8 * (n + 1))
    arena, osz = Dev(H, room + 1000), Dev(H, 4 * n)
    codec.compress_bounds_device(d_ss.p, n, d_bounds.p)
    codec.layout_outputs_device(d_bounds.p, 0, n, fcaps.p, foff.p, align=align)
    codec.compress_resident(src.p, d_so.p, d_ss.p, n, 204800, frames.p, foff.p, fsz.p, cdict_set=cset, d_dict_index_ptr=d_index.p)
    codec.pack_device(frames.p, want_fo, fsz.p, n, packed.p, poff.p)
    codec.frame_sizes_device(packed.p, poff.p, fsz.p, n, content.p, 0, status.p)
    codec.layout_outputs_device(content.p, status.p, n, caps.p, ooff.p, align=align)
    codec.decompress_resident(packed.p, poff.p, fsz.p, n, arena.p, ooff.p, caps.p, 204800, osz.p, ddict_set=dset)
    codec.sync()
    got_fo, ok = R.down(foff, np.uint64)
    assert ok and (got_fo[:n] == want_fo).all()
    got_fsz, ok = R.down(fsz, np.uint32)
    assert ok and (got_fsz <= bounds).all()
    got_status, ok = R.down(status, np.uint32)
    assert ok and not got_status.any()
    got_content, ok = R.down(content, np.uint64)
    assert ok and (got_content == ss).all()
    got_sz, ok = R.down(osz, np.uint32)
    assert ok and (got_sz == ss).all(), [(int(i), hex(int(got_sz[i]))) for i in np.flatnonzero(got_sz != ss)[:8]]
    want_off = B.layout((ss.astype(np.uint64) + align - 1) // align * align)
    host, ok = R.down(arena)
    assert ok
    inside = np.zeros(len(host), dtype=bool)
    for i, (o, c) in enumerate(zip(want_off, chunks)):
        assert host[int(o):int(o) + len(c)].tobytes() == c, ("chunk", i, len(c), int(index[i]))
        inside[int(o):int(o) + len(c)] = True
    assert (host[~inside] == CANARY).all(), "written outside the laid-out places"
    fhost, ok = R.down(frames)
    assert ok
    B.assert_only_frames_written(fhost, want_fo, np.where((ss > 65536) | (ss == 0), got_fsz, bounds), bounds, what="the frames of the chain")
    named = 0
    for i, (o, s) in enumerate(zip(want_fo, got_fsz)):                                # each frame names the member its chunk picked
        ch = int(index[i])
        want_id = cds[ch].dict_id if ch != NO_DICT else 0
        assert RS.frame_dict_id(fhost[int(o):int(o) + int(s)].tobytes()) == want_id, (i, ch)
        named += want_id != 0
    assert named >= 60
    _, ok = R.down(d_index, np.uint32)
    assert ok
    for d in (src, d_so, d_ss, d_index, d_bounds, fcaps, foff, frames, fsz, packed, poff, content, status, caps, ooff, arena, osz):
        d.free()
    dset.close()
    for dd in dds:
        dd.close()


# ------------------------------------------------------------------ 7. the plain calls did not move
def test_plain_resident_call_on_the_shared_kernels(codec, batches, sets):
    """compress_resident without a set on the 64 KiB batch, after a set call on the same context: still compress_device's frames; and a
    NULL set through the new entry point is that call at level 3"""
    batch, _ = batches(64 * KIB)
    batch.run_set(True, sets(3)[0], 64 * KIB)
    ref = batch.run(False)
    got = batch.run(True, 64 * KIB)
    RC.assert_equal_to_host_call(batch, ref, got, 64 * KIB, "the plain resident call")
    assert all(RS.frame_dict_id(f) == 0 for f in batch.frames(*got))
    dst, dsz = Dev(batch.H, batch.total), Dev(batch.H, 4 * batch.n)
    p = ctypes.c_void_p
    assert codec.L.zsmi_compressBatchResident_usingCDictSet(codec.ctx, p(batch.src.p), p(batch.d_so.p), p(batch.d_ss.p), batch.n, 64 * KIB, p(dst.p),
                                                            p(batch.d_do.p), p(dsz.p), None, None) == 0
    codec.sync()
    host, ok1 = R.down(dst)
    sz, ok2 = R.down(dsz, np.uint32)
    assert ok1 and ok2
    RC.assert_equal_to_host_call(batch, ref, (sz, host), 64 * KIB, "a NULL set")
    dst.free(); dsz.free()


# ------------------------------------------------------------------ 8. the host checks
def test_host_checks_in_order(codec, H, sets):
    L = codec.L
    cset = sets(3)[0]
    buf = Dev(H, 64)
    p = ctypes.c_void_p(buf.p)
    call = L.zsmi_compressBatchResident_usingCDictSet
    assert call(None, None, None, None, 1, 100, None, None, None, cset.handle, None) == 62      # init_missing before anything else
    for k in (0, 1, 2, 5, 6, 7):                                                                # each pointer in turn: GENERIC, before the index rule
        args = [p, p, p, 1, 100, p, p, p, cset.handle, None]
        args[k] = None
        assert call(codec.ctx, *args) == 1, k
    assert call(codec.ctx, p, p, p, 1, 100, p, p, p, cset.handle, None) == 1                     # a NULL index and seven members
    assert call(codec.ctx, None, None, None, 0, 100, None, None, None, cset.handle, None) == 0  # n == 0: nothing to do, nothing read
    assert call(codec.ctx, None, None, None, 0, 100, None, None, None, None, None) == 0
    with pytest.raises(ValueError):
        codec.compress_resident(buf.p, buf.p, buf.p, 1, 100, buf.p, buf.p, buf.p, level=1, cdict_set=cset, d_dict_index_ptr=buf.p)
    with pytest.raises(ValueError):
        codec.compress_resident(buf.p, buf.p, buf.p, 1, 100, buf.p, buf.p, buf.p, d_dict_index_ptr=buf.p)
    codec.sync()
    R.assert_tail_untouched(buf, 0, "the refused calls")
    buf.free()
