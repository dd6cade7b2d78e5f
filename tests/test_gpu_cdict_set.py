"""CDict sets on the GPU (zsmi_createCDictSet, zsmi_compress*_usingCDictSet; CompressionDictSet): one compress call whose chunks use
different dictionaries.  Frame i is, byte for byte, the frame the _usingCDict call gives chunk i with the member it picks (the plain call
for NO_DICT or an empty member) - whatever its neighbours use, wherever the sub-batch cuts fall, whatever the context's last call was.
The references are not this change's: oracle E for raw-content and NO_DICT items, oracle D for every item, the digests of
tests/golden/cdict_frame_digests.json for the pinned records.  The mixed batch: tests/_cdict_set.py (pinned on the CPU by
tests/test_cdict_set_host.py); batches and children: tests/_batch.py."""
import ctypes, json, os
import numpy as np
import pytest
import _oracle as O
import _data as D
import _dicts as X
import _batch as B
import _cdict as K
import _cdict_set as S

pytestmark = pytest.mark.gpu
GENERIC, UNSUPPORTED, OUT_OF_BOUND = 1, 40, 42
NO_DICT = S.NO_DICT


@pytest.fixture(scope="module")
def codec():
    from zstandard_amd import BatchCodec
    return BatchCodec(0)


_made = {}


def member_cdicts(codec, level):
    """the members' CompressionDicts at a level, made once; the member listed twice is one object at two indices"""
    from zstandard_amd import CompressionDict
    if level not in _made:
        names = [n for n, _ in S.members()]
        cds = [None if n == "again" else CompressionDict(codec, d, level) for n, d in S.members()]
        cds[names.index("again")] = cds[names.index(S.AGAIN_OF)]
        _made[level] = cds
    return _made[level]


def compress_set(codec, chunks, cset, index):
    """one compress_host call through a CompressionDictSet -> frames"""
    src, offs, sizes = B.batch(chunks)
    return B.frames_of(codec.compress_host(src, offs, sizes, cdict_set=cset, dict_index=np.asarray(index, dtype=np.uint32)), len(chunks))


def per_member_frames(codec, cds, level, chunks, index):
    """what the set call replaces: a _usingCDict call per member over its own chunks, the plain call at `level` over the NO_DICT ones"""
    frames = [None] * len(chunks)
    for m in sorted(set(int(i) for i in index)):
        ks = [k for k, i in enumerate(index) if i == m]
        part = B.compress_many(codec, [chunks[k] for k in ks], level) if m == NO_DICT else B.compress_many(codec, [chunks[k] for k in ks], cdict=cds[m])
        for k, f in zip(ks, part):
            frames[k] = f
    return frames


_reference = {}


def reference(codec, level):
    """per_member_frames of the whole mixed batch, once a level"""
    if level not in _reference:
        _reference[level] = per_member_frames(codec, member_cdicts(codec, level), level, S.chunks(), S.choices())
    return _reference[level]


# ------------------------------------------------------------------ 1. the contract
@pytest.mark.parametrize("level", [1, 3, 4])
def test_mixed_batch_in_one_call(codec, level):
    from zstandard_amd import CompressionDict, CompressionDictSet
    cds = member_cdicts(codec, level)
    chunks, index = S.chunks(), S.choices()
    cset = CompressionDictSet(codec, cds, level)
    assert len(cset) == len(S.members())
    frames = compress_set(codec, chunks, cset, index)
    cset.close()
    for i, e in S.oracle_frames(level).items():                                   # oracle E: raw members, NO_DICT, the empty member
        assert frames[i] == e, (level, i, S.kind(index[i]), len(chunks[i]), B.first_difference(frames[i], e))
    for i, (f, c) in enumerate(zip(frames, chunks)):                              # oracle D: every item with its dictionary
        dic = S.dictionary(index[i])
        assert (O.decompress_using_dict(f, len(c), dic) if dic else O.decompress(f, len(c))) == c, (level, i, len(c))
        want_id = O.dict_params(dic)[1] if dic else 0
        code = f[4] & 3
        assert (int.from_bytes(f[5:5 + (4 if code == 3 else code)], "little") if code else 0) == want_id, (level, i)
    used = sum(K.uses_dictionary_tables(K.blocks_of(f)[0]) for f, i in zip(frames, index) if S.kind(i) == "formatted")
    assert used > 0                                                               # (the formatted members' tables are in play)
    for i, (f, r) in enumerate(zip(frames, reference(codec, level))):             # the _usingCDict call's frame, item by item
        assert f == r, (level, i, int(index[i]), len(chunks[i]), B.first_difference(f, r))
    if level in K.PIN_LEVELS:                                                     # the pinned records, four dictionaries interleaved in one call
        want = json.load(open(os.path.join(D.GOLDEN, "cdict_frame_digests.json")))
        cases = list(K.pin_cases().items())
        pins = [CompressionDict(codec, dic, level) for _, (dic, _) in cases]
        pset = CompressionDictSet(codec, pins, level)
        records = [cases[k % 4][1][1][k // 4] for k in range(4 * 32)]
        got = compress_set(codec, records, pset, [k % 4 for k in range(4 * 32)])
        pset.close()
        for k, (name, _) in enumerate(cases):
            assert K.frames_digest(got[k::4]) == want[f"{name}_l{level}"], (name, level)
        for cd in pins:
            cd.close()


# ------------------------------------------------------------------ 2. sets of 1, 2, 4 and all members
def test_sets_of_1_2_4_and_all_members_over_sub_selections(codec):
    from zstandard_amd import CompressionDictSet
    level = 3
    cds, chunks, index, ref = member_cdicts(codec, level), S.chunks(), S.choices(), reference(codec, level)
    names = [n for n, _ in S.members()]
    picks = [names.index(n) for n in ("trained64k_zipf", "raw65536", "reps_70000_content100k", "id_0xffffffff")]     # (set order: not the batch's)
    for k in (1, 2, 4):
        sub = picks[:k]
        ks = [i for i, ch in enumerate(index) if ch in sub] + [i for i, ch in enumerate(index) if ch == NO_DICT][:60]
        ks.sort()
        cset = CompressionDictSet(codec, [cds[m] for m in sub], level)
        assert len(cset) == k
        got = compress_set(codec, [chunks[i] for i in ks], cset, [NO_DICT if index[i] == NO_DICT else sub.index(index[i]) for i in ks])
        cset.close()
        assert got == [ref[i] for i in ks], (k, next(j for j, i in enumerate(ks) if got[j] != ref[i]))
    every = CompressionDictSet(codec, cds, level)
    ks = list(range(1, len(chunks), 3))                                           # (another layout, so other neighbours and groups)
    got = compress_set(codec, [chunks[i] for i in ks], every, index[ks])
    assert got == [ref[i] for i in ks]
    # a set nobody picks, and a set of no members: the plain call
    ks = list(range(0, 400))
    plain = B.compress_many(codec, [chunks[i] for i in ks], level)
    assert plain == B.oracle_frames([chunks[i] for i in ks], level)
    assert compress_set(codec, [chunks[i] for i in ks], every, [NO_DICT] * len(ks)) == plain
    every.close()
    none = CompressionDictSet(codec, [], level)
    assert len(none) == 0
    assert compress_set(codec, [chunks[i] for i in ks], none, [NO_DICT] * len(ks)) == plain
    assert compress_set(codec, [], none, []) == []
    none.close()


# ------------------------------------------------------------------ 3. plan reuse
def test_one_layout_other_choices_and_other_calls_in_alternation(codec):
    """the plan of a layout is kept from call to call: the same layout with another index array, and through the plain call and a
    _usingCDict call in between, must give each call its own frames"""
    from zstandard_amd import CompressionDictSet
    level = 3
    cds, chunks, index = member_cdicts(codec, level), S.chunks()[:240], S.choices()[:240]
    members = sorted(set(int(i) for i in index) - {NO_DICT})
    other = np.array([members[(k * 5) % len(members)] if k % 3 else NO_DICT for k in range(len(chunks))], dtype=np.uint32)
    assert (other != index).sum() > 150
    one = [n for n, _ in S.members()].index("trained64k_json_records")
    want_a, want_b = per_member_frames(codec, cds, level, chunks, index), per_member_frames(codec, cds, level, chunks, other)
    want_plain, want_one = B.compress_many(codec, chunks, level), B.compress_many(codec, chunks, cdict=cds[one])
    assert want_a != want_b and want_plain != want_one
    cset = CompressionDictSet(codec, cds, level)
    assert compress_set(codec, chunks, cset, index) == want_a                     # (the layout's first call)
    assert compress_set(codec, chunks, cset, other) == want_b                     # the same layout, another choice
    assert compress_set(codec, chunks, cset, other) == want_b
    assert compress_set(codec, chunks, cset, index) == want_a
    for rnd in range(2):
        assert B.compress_many(codec, chunks, level) == want_plain
        assert compress_set(codec, chunks, cset, index) == want_a
        assert B.compress_many(codec, chunks, cdict=cds[one]) == want_one
        assert compress_set(codec, chunks, cset, other) == want_b
        assert compress_set(codec, chunks, cset, [one] * len(chunks)) == want_one
        assert B.compress_many(codec, chunks, cdict=cds[one]) == want_one
        assert compress_set(codec, chunks, cset, [NO_DICT] * len(chunks)) == want_plain
        assert compress_set(codec, chunks, cset, index) == want_a
    cset.close()


# ------------------------------------------------------------------ 4. sub-batches
_COMMON = r'''
import sys, os, ctypes
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import numpy as np
import _oracle as O, _dicts as X, _batch as B, _cdict_set as S
from zstandard_amd import BatchCodec, CompressionDict, CompressionDictSet, NO_DICT
bc = BatchCodec(0)
L = bc.L
level = 3
names = [n for n, _ in S.members()]
cds = [None if n == "again" else CompressionDict(bc, d, level) for n, d in S.members()]
cds[names.index("again")] = cds[names.index(S.AGAIN_OF)]
cset = CompressionDictSet(bc, cds, level)
chunks, index = S.chunks(), S.choices()

def per_member(chunks, index):
    frames = [None] * len(chunks)
    for m in sorted(set(int(i) for i in index)):
        ks = [k for k, i in enumerate(index) if i == m]
        part = B.compress_many(bc, [chunks[k] for k in ks], level) if m == NO_DICT else B.compress_many(bc, [chunks[k] for k in ks], cdict=cds[m])
        for k, f in zip(ks, part):
            frames[k] = f
    return frames
'''

_SUB_CHILD = _COMMON + r'''
src, offs, sizes = B.batch(chunks)
frames = B.frames_of(bc.compress_host(src, offs, sizes, cdict_set=cset, dict_index=index))
blocks = sum(S.blocks_of_size(len(c)) for c in chunks)
assert blocks > 8 * 64                                    # (more than eight sub-batches)
for i, e in S.oracle_frames(level).items():
    assert frames[i] == e, (i, len(chunks[i]))
for i, (f, c) in enumerate(zip(frames, chunks)):
    dic = S.dictionary(index[i])
    assert (O.decompress_using_dict(f, len(c), dic) if dic else O.decompress(f, len(c))) == c, i
want = per_member(chunks, index)
for i, (f, w) in enumerate(zip(frames, want)):
    assert f == w, (i, int(index[i]), len(chunks[i]))
print("CHILD-OK")
'''


def test_sub_batches_with_a_set():
    """ZSMI_BLOCKS_IN_FLIGHT=64 in a child process: the mixed batch takes more than eight sub-batches, whose cuts fall between chunks of
    different members - the frames are those of test 1: oracle E's, oracle D's chunks, the _usingCDict calls'"""
    B.run_child("-c", _SUB_CHILD, B.ROOT, env=dict(os.environ, ZSMI_BLOCKS_IN_FLIGHT="64"))


# ------------------------------------------------------------------ 5. device-pointer form
_DEVICE_CHILD = "import torch\n" + _COMMON + r'''
rng = np.random.default_rng(9)
chunks, index = chunks[:600], index[:600]
sizes = np.array([len(c) for c in chunks], dtype=np.uint32)
assert {0, 1, 65536, 65537, 131073, 200 * 1024} <= set(int(s) for s in sizes)
so, do, bounds, total = B.ragged_device_layout(L, sizes, rng)
src_np = np.frombuffer(b"".join(chunks), dtype=np.uint8)
src = torch.from_numpy(src_np.copy()).cuda()
dst = torch.full((total,), B.CANARY, dtype=torch.uint8, device="cuda")
dsz = torch.zeros(len(sizes), dtype=torch.int32, device="cuda")
torch.cuda.synchronize()
bc.compress_device(src.data_ptr(), so, sizes, dst.data_ptr(), do, dsz.data_ptr(), cdict_set=cset, dict_index=index)
bc.sync()
host = dst.cpu().numpy(); sz = dsz.cpu().numpy().view(np.uint32)
assert (sz <= bounds).all()
# what a chunk's call may touch: a chunk of several blocks (k_assemble_frames) and an empty one nothing but the frame; a one-block chunk its slot
# of zsmi_compressBound bytes - the literals kernel of every call form builds such a chunk's literal section inside the slot (entropy_kernels.hip)
# and leaves up to 3 bytes of it behind the end of a frame whose block goes out raw (seen here: 1 - 3 bytes behind 16-byte, 3000-byte and 64 KiB
# chunks of noise, with and without a dictionary)
extent = np.where((sizes > 65536) | (sizes == 0), sz, bounds)
assert ((sizes > 65536).sum() > 40) and ((sizes == 0).sum() >= 2)
B.assert_only_frames_written(host, do, extent, bounds, B.CANARY, "set")
got = B.cut(host, do, sz)
assert got == B.frames_of(bc.compress_host(src_np, so, sizes, cdict_set=cset, dict_index=index)), "host form"
assert got == per_member(chunks, index)
# NULL set: the plain call at level 3 (the index array is not read)
dst1 = torch.full((total,), B.CANARY, dtype=torch.uint8, device="cuda"); s1 = torch.zeros(len(sizes), dtype=torch.int32, device="cuda")
p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
assert L.zsmi_compressBatchDevice_usingCDictSet(bc.ctx, ctypes.c_void_p(src.data_ptr()), p(so), p(sizes), len(sizes), ctypes.c_void_p(dst1.data_ptr()), p(do),
                                                ctypes.c_void_p(s1.data_ptr()), None, None) == 0
bc.sync()
assert B.cut(dst1.cpu().numpy(), do, s1.cpu().numpy().view(np.uint32)) == B.oracle_frames(chunks, 3)
print("CHILD-OK")
'''


def test_device_pointer_form_stays_in_bounds():
    """zsmi_compressBatchDevice_usingCDictSet: canary-filled output, a ragged layout of the batch's first 600 chunks (0 bytes to 200 KiB);
    every frame within zsmi_compressBound; nothing written outside the frames of the chunks of several blocks and the empty ones, nothing
    outside the zsmi_compressBound slot of a one-block chunk (whose literal section every call form builds inside that slot: up to 3 bytes of
    it stay behind the end of a raw-block frame, which the helper's frame-exact form reports); the frames of the host form and of the
    _usingCDict calls"""
    B.run_child("-c", _DEVICE_CHILD, B.ROOT)


# ------------------------------------------------------------------ 6. errors and lifecycle
def test_refusals_leave_the_destination_alone(codec):
    from zstandard_amd import BatchCodec, CompressionDict, CompressionDictSet
    L = codec.L
    cds = member_cdicts(codec, 3)
    h = [cd.handle for cd in cds]
    level1 = CompressionDict(codec, X.TRAINED8K, 1)

    def create(handles, n=None, level=3):
        arr = (ctypes.c_void_p * max(len(handles), 1))(*handles)
        err = ctypes.c_int(-1)
        got = L.zsmi_createCDictSet(codec.ctx, arr, len(handles) if n is None else n, level, ctypes.byref(err))
        if not got:                                                               # (refused without an err pointer too)
            assert not L.zsmi_createCDictSet(codec.ctx, arr, len(handles) if n is None else n, level, None)
        return got, err.value

    for what, handles, level, code in (("a NULL entry", [h[0], None, h[1]], 3, UNSUPPORTED), ("a member of another level", [h[0], level1.handle], 3, UNSUPPORTED),
                                       ("the set's level is not the members'", h[:3], 1, UNSUPPORTED), ("4097 entries", [h[0]] * 4097, 3, OUT_OF_BOUND),
                                       ("4097 entries, the first NULL: the count is judged first", [None] + [h[0]] * 4096, 3, OUT_OF_BOUND)):
        got, err = create(handles, level=level)
        assert not got and err == code, (what, err)
    err = ctypes.c_int(-1)
    assert not L.zsmi_createCDictSet(codec.ctx, None, 3, 3, ctypes.byref(err)) and err.value == UNSUPPORTED          # NULL cds with n > 0
    ok, err = create([h[0]] * 4096)
    assert ok and err == 0 and L.zsmi_sizeofCDictSetMembers(ok) == 4096
    L.zsmi_freeCDictSet(ok)
    ok, err = create([None, None], n=0)                                           # n = 0: the entries are not looked at
    assert ok and err == 0 and L.zsmi_sizeofCDictSetMembers(ok) == 0
    L.zsmi_freeCDictSet(ok)
    level1.close()
    # the call's refusals: nothing is queued, nothing written
    cset = CompressionDictSet(codec, cds[:4], 3)
    chunks = S.chunks()[:16]
    src, offs, sizes = B.batch(chunks)
    bounds = np.array([L.zsmi_compressBound(int(s)) for s in sizes], dtype=np.uint64)
    do = B.layout(bounds)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a is not None else None
    for what, index, code in (("no index array", None, GENERIC), ("an index of 4 in a set of 4", [0, 1, 2, 3] * 3 + [NO_DICT, 0, 4, 1], OUT_OF_BOUND),
                              ("an index just below NO_DICT", [NO_DICT] * 15 + [NO_DICT - 1], OUT_OF_BOUND)):
        dst, dsz = np.full(int(bounds.sum()), B.CANARY, dtype=np.uint8), np.full(len(chunks), 0xABABABAB, dtype=np.uint32)
        idx = None if index is None else np.array(index, dtype=np.uint32)
        rc = L.zsmi_compressBatchHost_usingCDictSet(codec.ctx, p(src), p(offs), p(sizes), len(chunks), p(dst), p(do), p(dsz), cset.handle, p(idx))
        assert rc == code, (what, rc)
        assert (dst == B.CANARY).all() and (dsz == 0xABABABAB).all(), what
        with pytest.raises((RuntimeError, ValueError)):
            codec.compress_host(src, offs, sizes, cdict_set=cset, dict_index=idx)
    assert L.zsmi_compressBatchHost_usingCDictSet(None, p(src), p(offs), p(sizes), len(chunks), None, p(do), None, cset.handle, p(np.zeros(16, dtype=np.uint32))) == 62
    assert L.zsmi_compressBatchHost_usingCDictSet(codec.ctx, p(src), p(offs), p(sizes), 0, None, p(do), None, cset.handle, None) == 0       # n = 0: a valid call that does nothing
    # the context and the set still work
    index = [0, NO_DICT, 1, 2, 3, NO_DICT, 0, 1, 2, 3, NO_DICT, 0, 3, 2, 1, 0]
    assert compress_set(codec, chunks, cset, index) == per_member_frames(codec, cds, 3, chunks, index)
    cset.close()


def test_second_context_two_sets_and_close_after_sync(codec):
    from zstandard_amd import BatchCodec, CompressionDictSet
    level = 3
    cds, chunks, index = member_cdicts(codec, level), S.chunks()[:200], S.choices()[:200]
    want = per_member_frames(codec, cds, level, chunks, index)
    members = sorted(set(int(i) for i in index) - {NO_DICT})
    a = CompressionDictSet(codec, cds, level)
    rev = list(reversed(range(len(cds))))
    b = CompressionDictSet(codec, [cds[m] for m in rev], level)                  # the same members, another order
    index_b = np.array([NO_DICT if i == NO_DICT else rev.index(int(i)) for i in index], dtype=np.uint32)
    second = BatchCodec(0)                                                        # another context of the same device
    for rnd in range(2):
        assert compress_set(codec, chunks, a, index) == want
        assert compress_set(codec, chunks, b, index_b) == want
        assert compress_set(second, chunks, b, index_b) == want
        assert compress_set(second, chunks, a, index) == want
    codec.sync(); second.sync()
    a.close(); b.close(); a.close()                                               # the sets first (twice: harmless), their members stay
    assert per_member_frames(codec, cds, level, chunks[:40], index[:40]) == want[:40]
    assert per_member_frames(second, cds, level, chunks[:40], index[:40]) == want[:40]
    second.close()


# ------------------------------------------------------------------ 7. end to end: one call each way
_E2E_CHILD = r'''
import os; os.environ["ZSMI_DEBUG_LIB"] = "1"
import sys, ctypes
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import numpy as np
import _oracle as O, _batch as B, _cdict_set as S
from zstandard_amd import BatchCodec, CompressionDict, CompressionDictSet, DecompressionDict, DecompressionDictSet, NO_DICT, _lib
if _lib.built_fingerprint() != _lib.source_fingerprint():
    _lib.build()
bc = BatchCodec(0); Z = _lib.lib()
lay = (ctypes.c_uint32 * 6)(); Z.zsmi_dbg_descLayout(lay)
WORDS, FAST_AT, WHY_AT = int(lay[0]), int(lay[1]), int(lay[2])
# the formatted members a DDict set can hold: an ID of their own, not 0
ids, keep = set(), []
for m, (name, dic) in enumerate(S.members()):
    if S.kind(m) == "formatted" and O.dict_params(dic)[1] not in ids | {0}:
        ids.add(O.dict_params(dic)[1]); keep.append(m)
assert len(keep) >= 12
dics = [S.members()[m][1] for m in keep]
cds = [CompressionDict(bc, d, 3) for d in dics]
dds = [DecompressionDict(bc, d) for d in dics]
cset, dset = CompressionDictSet(bc, cds, 3), DecompressionDictSet(bc, list(reversed(dds)))
items = [(c, keep.index(ch) if ch != NO_DICT else NO_DICT) for c, ch in S.deal() if ch in keep or ch == NO_DICT]
chunks, index = [c for c, _ in items], np.array([i for _, i in items], dtype=np.uint32)
assert (index == NO_DICT).sum() > 500 and (index != NO_DICT).sum() > 500
frames = B.frames_of(bc.compress_host(*B.batch(chunks), cdict_set=cset, dict_index=index))
caps = np.array([len(c) for c in chunks], dtype=np.uint32)
out, oo, osz = bc.decompress_host(*B.batch(frames), caps, ddict_set=dset)
buf = np.zeros(len(chunks) * WORDS, dtype=np.uint32)
assert Z.zsmi_dbg_copyScratch(bc.ctx, b"fastDesc", buf.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(buf.nbytes)) == 0
desc = buf.reshape(-1, WORDS)
assert (osz == caps).all(), [(int(i), hex(int(osz[i]))) for i in np.flatnonzero(osz != caps)[:5]]
assert B.cut(out, oo, osz) == chunks
checked = 0
for i, c in enumerate(chunks):
    if 0 < len(c) <= 65536:                                # single-block items
        assert desc[i, FAST_AT] == 1, (i, len(c), int(index[i]), "left the fast path", int(desc[i, WHY_AT]))
        checked += 1
cset.close(); dset.close()
for x in cds + dds:
    x.close()
assert checked > 800, checked
print("CHILD-OK", checked)
'''


def test_compressed_with_a_cdict_set_decoded_with_the_ddict_set():
    """a child with the debug-hook library: the chunks of the formatted members (those a DDict set may hold: an ID of their own) and the
    NO_DICT chunks, compressed in ONE _usingCDictSet call and decoded in ONE _usingDDictSet call with the same dictionaries, are the input
    again; ZsFastDesc.fast says the single-block items were decoded by the fast kernels"""
    B.run_child("-c", _E2E_CHILD, B.ROOT)
