"""DDict sets on the GPU (zsmi_createDDictSet, zsmi_decompress*_usingDDictSet; DecompressionDictSet): one decode call whose frames name
different dictionaries.  Per item the results - bytes, sizes, error codes - are oracle D's with the dictionary the rule picks for it, and
those of the _usingDDict call with that dictionary; dictionary frames stay on the fast path.  The mixed batch and its dictionaries:
tests/_ddict_set.py (pinned on the CPU by tests/test_ddict_set_host.py); trained dictionaries and chunks: tests/_dicts.py; batches and
children: tests/_batch.py."""
import ctypes, os
import numpy as np
import pytest
import _dicts as X
import _batch as B
import _ddict as DD
import _ddict_set as S

pytestmark = pytest.mark.gpu
UNSUPPORTED, OUT_OF_BOUND = 40, 42


@pytest.fixture(scope="module")
def codec():
    from zstandard_amd import BatchCodec
    return BatchCodec(0)


@pytest.fixture(scope="module")
def ddicts(codec):
    """name -> DecompressionDict of every dictionary of the helper, made once"""
    from zstandard_amd import DecompressionDict
    made = {name: DecompressionDict(codec, dic) for name, dic in S.dictionaries().items()}
    for name, dd in made.items():
        assert dd.dict_id == S.dict_id(S.dictionaries()[name]), name
    yield made
    for dd in made.values():
        dd.close()


def decode_set(codec, frames, caps, dset):
    """one decompress_host call through a DecompressionDictSet -> [(size or error word, bytes)]"""
    src, offs, sizes = B.batch(frames)
    out, oo, osz = codec.decompress_host(src, offs, sizes, np.array(caps, dtype=np.uint32), ddict_set=dset)
    return [(int(s), out[int(o):int(o) + (int(s) if s < B.ERR else 0)].tobytes()) for o, s in zip(oo, osz)]


class NullSet:
    handle = None


def create_raw(L, ctx, handles, unnamed=None, n=None):
    """zsmi_createDDictSet itself -> (handle or None, code)"""
    arr = (ctypes.c_void_p * max(len(handles), 1))(*handles)
    err = ctypes.c_int(-1)
    h = L.zsmi_createDDictSet(ctx, arr, len(handles) if n is None else n, unnamed, ctypes.byref(err))
    return h, err.value


# ------------------------------------------------------------------ 1. the mixed batch, host form
@pytest.mark.parametrize("config", S.configurations(), ids=["%d members, unnamed %s" % (len(m), u) for m, u in S.configurations()])
def test_mixed_batch_equals_oracle_and_usingddict(codec, ddicts, config):
    """item by item: oracle D with the picked dictionary, and the _usingDDict call with it (one call per dictionary)"""
    from zstandard_amd import DecompressionDictSet
    members, unnamed = config
    its = S.items()
    dset = DecompressionDictSet(codec, [ddicts[m] for m in members], ddicts[unnamed] if unnamed else None)
    assert len(dset) == len(members) + (unnamed == "narrow")
    frames, caps = [b"".join(it["frames"]) for it in its], [it["cap"] for it in its]
    got = decode_set(codec, frames, caps, dset)
    dset.close()
    for it, g in zip(its, got):
        assert g == S.oracle_item(it, members, unnamed), (it["name"], hex(g[0]))
    groups = {}
    for k, it in enumerate(its):
        picks = {S.pick(i, members, unnamed) for i in it["ids"]}
        if len(picks) == 1 and "wrong" not in picks:                       # (an ID nobody has: there is no dictionary to call _usingDDict with)
            groups.setdefault(picks.pop(), []).append(k)
    assert len(groups) >= min(len(members), 4)
    for name, ks in groups.items():
        one = DD.decode_many(codec, [frames[k] for k in ks], [caps[k] for k in ks], ddicts[name]) if name else \
            B.decode_many(codec, [frames[k] for k in ks], [caps[k] for k in ks], min_cap=0)
        for k, r in zip(ks, one):
            assert got[k] == r, (its[k]["name"], name, hex(got[k][0]), hex(r[0]))


# ------------------------------------------------------------------ 2. the fast path
_FAST_CHILD = r'''
import os; os.environ["ZSMI_DEBUG_LIB"] = "1"
import sys, ctypes
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import numpy as np, torch
import _batch as B, _ddict as DD, _ddict_set as S
from zstandard_amd import BatchCodec, DecompressionDict, DecompressionDictSet, _lib
if _lib.built_fingerprint() != _lib.source_fingerprint():
    _lib.build()
bc = BatchCodec(0); Z = _lib.lib()
lay = (ctypes.c_uint32 * 6)(); Z.zsmi_dbg_descLayout(lay)
WORDS, FAST_AT, WHY_AT = int(lay[0]), int(lay[1]), int(lay[2])
members, unnamed = S.member_order(), "raw"
dds = {name: DecompressionDict(bc, dic) for name, dic in S.dictionaries().items()}
dset = DecompressionDictSet(bc, [dds[m] for m in members], dds[unnamed])
assert len(dset) == 74
its = S.items()
frames, caps = [b"".join(it["frames"]) for it in its], [it["cap"] for it in its]
n = len(its)
src_np, so, ss = B.batch(frames)
do = B.layout(caps, [16] * n)
src = torch.from_numpy(src_np.copy()).cuda()
dst = torch.full((int(do[-1]) + caps[-1] + 64,), B.CANARY, dtype=torch.uint8, device="cuda")
dsz = torch.zeros(n, dtype=torch.int32, device="cuda")
torch.cuda.synchronize()
bc.decompress_device(src.data_ptr(), so, ss, dst.data_ptr(), do, np.array(caps, dtype=np.uint32), dsz.data_ptr(), ddict_set=dset)
bc.sync()
buf = np.zeros(n * WORDS, dtype=np.uint32)
assert Z.zsmi_dbg_copyScratch(bc.ctx, b"fastDesc", buf.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(buf.nbytes)) == 0
desc = buf.reshape(-1, WORDS)
host = dst.cpu().numpy(); sz = dsz.cpu().numpy().view(np.uint32)
inside = np.zeros(len(host), dtype=bool)
for o, c in zip(do, caps):
    inside[int(o):int(o) + int(c)] = True
assert np.flatnonzero(~inside & (host != B.CANARY)).size == 0
checked = 0
for i, it in enumerate(its):
    got = (int(sz[i]), host[int(do[i]):int(do[i]) + (int(sz[i]) if sz[i] < B.ERR else 0)].tobytes())
    want = S.oracle_item(it, members, unnamed)
    assert got == want, (it["name"], hex(got[0]), hex(want[0]))
    if want[0] > B.ERR or not S.single_frame(it) or DD.may_fall_back(it["name"]) or it["dnames"] == ["log12"]:
        continue
    assert desc[i, FAST_AT] == 1, (it["name"], "left the fast path", int(desc[i, WHY_AT]))
    checked += 1
dset.close()
for dd in dds.values():
    dd.close()
assert checked >= 60, checked
print("CHILD-OK", checked)
'''


def test_mixed_batch_device_form_on_the_fast_path():
    """a child with the debug-hook library: the device form with the set of 74 and raw content as `unnamed` gives oracle D's results, and
    ZsFastDesc.fast of block 0 says that every valid single-frame item was decoded by the fast kernels.  Exempt: what
    tests/test_gpu_ddict.py exempts ("m treeless ..."), and the other items of the log12 dictionary"""
    B.run_child("-c", _FAST_CHILD, B.ROOT)


# ------------------------------------------------------------------ 3. equivalence with the calls that were there
@pytest.mark.parametrize("dname", sorted(DD.dictionaries()))
def test_set_of_unnamed_alone_is_the_usingddict_call(codec, dname):
    """set({}, unnamed = dd) on the catalogue's own frames (which name 77, another ID, or none)"""
    from zstandard_amd import DecompressionDict, DecompressionDictSet
    names, frames, caps = DD.cases_of(dname)
    dd = DecompressionDict(codec, DD.dictionaries()[dname])
    dset = DecompressionDictSet(codec, [], dd)
    assert len(dset) == (0 if dname == "raw" else 1)
    got = decode_set(codec, frames, caps, dset)
    dset.close()
    want = DD.decode_many(codec, frames, caps, dd)
    dd.close()
    for name, g, w in zip(names, got, want):
        assert g == w, (name, hex(g[0]), hex(w[0]))
    assert got == DD.oracle_many(frames, caps, DD.dictionaries()[dname])


def test_null_and_empty_set_are_the_plain_call(codec):
    from zstandard_amd import DecompressionDict, DecompressionDictSet
    data = X.class_data("json_records")
    chunks = [data[:1024], data[2000:2000 + 4096], b"", b"q", data[10000:10000 + 70000], data[90000:90000 + 131073]]
    its = S.items()
    frames = B.compress_many(codec, chunks, 3) + [b"".join(it["frames"]) for it in its[:40]]
    caps = [len(c) for c in chunks] + [it["cap"] for it in its[:40]]
    src, offs, sizes = B.batch(frames)
    plain = codec.decompress_host(src, offs, sizes, np.array(caps, dtype=np.uint32))
    assert B.cut(plain[0], plain[1], plain[2][:len(chunks)]) == chunks
    empty_dd = DecompressionDict(codec, b"")
    for dset in (NullSet(), DecompressionDictSet(codec, []), DecompressionDictSet(codec, [], empty_dd)):
        got = codec.decompress_host(src, offs, sizes, np.array(caps, dtype=np.uint32), ddict_set=dset)
        assert all(np.array_equal(a, b) for a, b in zip(plain, got))
        if dset.handle:
            assert len(dset) == 0
            dset.close()
    empty_dd.close()
    with pytest.raises(ValueError):
        codec.decompress_host(src, offs, sizes, np.array(caps, dtype=np.uint32), ddict=empty_dd, ddict_set=NullSet())
    with pytest.raises(ValueError):
        codec.decompress_host(src, offs, sizes, np.array(caps, dtype=np.uint32), dictionary=b"abc", ddict_set=NullSet())
    with pytest.raises(ValueError):
        codec.decompress_device(0, offs, sizes, 0, offs, caps, 0, ddict=empty_dd, ddict_set=NullSet())


# ------------------------------------------------------------------ 4. creation errors
def test_creation_errors(codec, ddicts):
    from zstandard_amd import DecompressionDict
    L = codec.L
    h = lambda name: ddicts[name].handle
    twin = DecompressionDict(codec, S.dictionaries()["reps"])                 # the same ID in another DDict
    empty = DecompressionDict(codec, b"")
    cases = [("a duplicate ID", [h("narrow"), h("reps"), h("wide"), twin.handle], None, None, UNSUPPORTED),
             ("a raw-content member", [h("narrow"), h("raw")], None, None, UNSUPPORTED),
             ("an empty member", [empty.handle, h("narrow")], None, None, UNSUPPORTED),
             ("a NULL entry", [h("narrow"), None, h("reps")], None, None, UNSUPPORTED),
             ("4097 entries", [h("narrow")] * 4097, None, None, OUT_OF_BOUND),
             ("unnamed duplicating a member's ID", [h("narrow"), h("reps")], twin.handle, None, UNSUPPORTED)]
    for what, handles, unnamed, n, code in cases:
        got, err = create_raw(L, codec.ctx, handles, unnamed, n)
        assert not got and err == code, (what, err)
        assert not L.zsmi_createDDictSet(codec.ctx, (ctypes.c_void_p * len(handles))(*handles), len(handles), unnamed, None), what
    err = ctypes.c_int(-1)
    assert not L.zsmi_createDDictSet(codec.ctx, None, 3, None, ctypes.byref(err)) and err.value == UNSUPPORTED      # NULL dds with n > 0
    ok, err = create_raw(L, codec.ctx, [h("narrow")] * 4096, None, 0)              # n = 0: the entries are not looked at
    assert ok and err == 0 and L.zsmi_sizeofDDictSetMembers(ok) == 0
    L.zsmi_freeDDictSet(ok)
    twin.close(); empty.close()
    # the context still works: the first configuration of test 1
    from zstandard_amd import DecompressionDictSet
    members, unnamed = S.configurations()[1]
    its = S.items()[:32]
    dset = DecompressionDictSet(codec, [ddicts[m] for m in members])
    got = decode_set(codec, [b"".join(it["frames"]) for it in its], [it["cap"] for it in its], dset)
    dset.close()
    assert got == [S.oracle_item(it, members, None) for it in its]


# ------------------------------------------------------------------ 5. device-pointer form
_COMMON = r'''
import sys, os, ctypes
import torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import numpy as np
import _dicts as X, _batch as B, _ddict as DD, _ddict_set as S
from zstandard_amd import BatchCodec, CompressionDict, DecompressionDict, DecompressionDictSet
CLASSES = ("json_records", "zipf", "xml_records")
bc = BatchCodec(0)
L = bc.L

def trained_frames(sizes):
    """chunk i of class i % 3, compressed with that class's CDict: (chunks, frames, class index per item)"""
    cls = np.arange(len(sizes)) % 3
    chunks = [None] * len(sizes)
    for c, name in enumerate(CLASSES):
        data = X.class_data(name, 3 << 20)
        at = 0
        for i in np.flatnonzero(cls == c):
            chunks[i] = data[at:at + int(sizes[i])]; at += int(sizes[i])
            assert len(chunks[i]) == sizes[i]
    frames = [None] * len(sizes)
    for c, name in enumerate(CLASSES):
        cd = CompressionDict(bc, X.trained(name), 3)
        ks = np.flatnonzero(cls == c)
        for k, f in zip(ks, B.compress_many(bc, [chunks[k] for k in ks], cdict=cd)):
            frames[k] = f
        cd.close()
    return chunks, frames, cls

dds = [DecompressionDict(bc, X.trained(name)) for name in CLASSES]
assert len({d.dict_id for d in dds}) == 3
dset = DecompressionDictSet(bc, [dds[2], dds[0], dds[1]])
assert len(dset) == 3
'''

_DEVICE_CHILD = _COMMON + r'''
rng = np.random.default_rng(5)
sizes = np.array([0, 1, 17] + [1024] * 24 + [4096] * 12 + [65536, 65537, 131073], dtype=np.uint32)
rng.shuffle(sizes)
chunks, frames, cls = trained_frames(sizes)
src_np, so, ss = B.batch(frames)
src = torch.from_numpy(src_np.copy()).cuda()
p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
for short in (0, 1):
    caps = np.maximum(sizes.astype(np.int64) - short, 0).astype(np.uint32)
    # ragged destinations: each capacity long, a gap of 0 .. 299 bytes in front of every second one
    do = B.layout(caps, rng.integers(0, 300, len(caps)) * (np.arange(len(caps)) % 2))
    total = int(do[-1]) + int(caps[-1]) + 4096
    outs = []
    for form in ("set", "ddicts"):
        dst = torch.full((total,), B.CANARY, dtype=torch.uint8, device="cuda")
        dsz = torch.zeros(len(sizes), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        if form == "set":
            bc.decompress_device(src.data_ptr(), so, ss, dst.data_ptr(), do, caps, dsz.data_ptr(), ddict_set=dset)
        else:                                                  # what the set call replaces: a _usingDDict call per dictionary over its own frames
            for c in range(3):
                ks = np.flatnonzero(cls == c)
                part = torch.zeros(len(ks), dtype=torch.int32, device="cuda")
                bc.decompress_device(src.data_ptr(), so[ks], ss[ks], dst.data_ptr(), do[ks], caps[ks], part.data_ptr(), ddict=dds[c])
                bc.sync()
                dsz[torch.from_numpy(ks).cuda()] = part
        bc.sync()
        host = dst.cpu().numpy(); sz = dsz.cpu().numpy().view(np.uint32)
        inside = np.zeros(len(host), dtype=bool)
        for o, c in zip(do, caps):
            inside[int(o):int(o) + int(c)] = True
        bad = np.flatnonzero(~inside & (host != B.CANARY))
        assert bad.size == 0, (form, short, "written outside the capacities", bad[:10].tolist())
        outs.append((sz.copy(), [host[int(o):int(o) + int(s)].tobytes() if s < B.ERR else b"" for o, s in zip(do, sz)]))
    (sa, ba), (sb, bb) = outs
    assert (sa == sb).all(), (short, [(int(i), hex(int(sa[i])), hex(int(sb[i]))) for i in np.flatnonzero(sa != sb)[:5]])
    assert ba == bb, short
    if short == 0:
        assert ba == chunks
    else:
        for i, s in enumerate(sizes):
            assert (sa[i] == 0) if s == 0 else (sa[i] > B.ERR), (i, int(s), hex(int(sa[i])))
dset.close()
for d in dds:
    d.close()
print("CHILD-OK")
'''


def test_device_pointer_form_stays_in_bounds():
    """zsmi_decompressBatchDevice_usingDDictSet on CDict frames of three trained dictionaries, interleaved, of 0 bytes to 128 KiB + 1:
    canary-filled output, ragged destinations, exact capacities and then one byte short - nothing is written outside
    [dstOffsets[i], + dstCaps[i]); sizes, bytes and codes are those of the three zsmi_decompressBatchDevice_usingDDict calls"""
    B.run_child("-c", _DEVICE_CHILD, B.ROOT)


# ------------------------------------------------------------------ 6. sub-batches
_SUB_CHILD = _COMMON + r'''
rng = np.random.default_rng(23)
sizes = np.concatenate([rng.integers(0, 100000, 60), [65536] * 20, [1024] * 150, [4096] * 64, [131072] * 6]).astype(np.uint32)
rng.shuffle(sizes)
assert len(sizes) == 300
chunks, frames, cls = trained_frames(sizes)
mixed = list(frames)
caps = [len(c) for c in chunks]
unknown = [b"".join(it["frames"]) for it in S.items() if it["ids"] in ([77], [78], [S.UNKNOWN_ID])]
for k in range(0, 300, 37):                                 # frames that name an ID nobody has, and cut ones, among them
    mixed[k] = unknown[k % len(unknown)]
for k in range(5, 300, 41):
    mixed[k] = frames[k][:len(frames[k]) // 2]
src, offs, ssz = B.batch(mixed)
out, oo, osz = bc.decompress_host(src, offs, ssz, np.array(caps, dtype=np.uint32), ddict_set=dset)
got = [(int(s), out[int(o):int(o) + (int(s) if s < B.ERR else 0)].tobytes()) for o, s in zip(oo, osz)]
for c in range(3):
    ks = [k for k in range(300) if cls[k] == c]
    one = DD.decode_many(bc, [mixed[k] for k in ks], [caps[k] for k in ks], dds[c])
    for k, r in zip(ks, one):
        assert got[k] == r, (k, c, hex(got[k][0]), hex(r[0]))
wrong = 0
for k, (g, c) in enumerate(zip(got, chunks)):
    if mixed[k] is frames[k]:
        assert g == (len(c), c), (k, len(c), hex(g[0]))
    else:
        assert g[0] > B.ERR or len(c) == 0 or g[1] != c, k
        wrong += g[0] == 0x100000000 - 32
assert wrong >= 8
dset.close()
for d in dds:
    d.close()
print("CHILD-OK")
'''


def test_sub_batches_with_a_set():
    """ZSMI_ITEMS_IN_FLIGHT=64 in a child process: 300 shuffled frames of three trained dictionaries (0 to 128 KiB; frames that name an ID
    nobody has and cut ones among them) take five sub-batches - every item must get its own dictionary in each of them: the results are
    those of the three _usingDDict calls"""
    B.run_child("-c", _SUB_CHILD, B.ROOT, env=dict(os.environ, ZSMI_ITEMS_IN_FLIGHT="64"))


# ------------------------------------------------------------------ 7. lifecycle
def test_one_set_many_calls_two_sets_one_shot_and_free(codec):
    from zstandard_amd import CompressionDict, DecompressionDict, DecompressionDictSet
    L = codec.L
    names = ("json_records", "zipf", "xml_records")
    dics = [X.trained(n) for n in names]
    data = X.class_data("json_records")
    chunks = [data[i:i + 1024] for i in range(0, 24 * 1024, 1024)] + [data[70000:70000 + 65537], b"", b"x", data[5:4101]]
    caps = [len(c) for c in chunks]
    want = [(len(c), c) for c in chunks]
    frames = []
    for k, dic in enumerate(dics):
        cd = CompressionDict(codec, dic, 3)
        frames.append(B.compress_many(codec, chunks, cdict=cd))
        cd.close()
    plain = B.compress_many(codec, chunks, 3)
    dds = [DecompressionDict(codec, dic) for dic in dics]
    inter = [frames[i % 3][i] for i in range(len(chunks))]                     # item i names dictionary i % 3
    older = lambda: (B.decode_many(codec, plain, caps, min_cap=0), DD.decode_many(codec, frames[0], caps, dds[0]), B.decode_many(codec, frames[1], caps, dics[1], min_cap=0))
    before = older()
    assert before == (want, want, want)
    all3 = DecompressionDictSet(codec, dds)
    ab, bc_ = DecompressionDictSet(codec, [dds[1], dds[0]]), DecompressionDictSet(codec, [dds[2]], dds[1])      # overlapping members; B is `unnamed` of the second
    assert (len(all3), len(ab), len(bc_)) == (3, 2, 2)
    wrong = (0x100000000 - 32, b"")
    for rnd in range(3):
        assert decode_set(codec, inter, caps, all3) == want                     # one set, many calls
        assert decode_set(codec, inter, caps, ab) == [w if i % 3 != 2 else wrong for i, w in enumerate(want)]
        assert decode_set(codec, inter, caps, bc_) == [w if i % 3 != 0 else wrong for i, w in enumerate(want)]
        assert decode_set(codec, plain, caps, ab) == want
        assert older() == before
    for i, (c, f) in enumerate(zip(chunks, inter)):                              # the one-shot form, frame by frame
        out = ctypes.create_string_buffer(max(len(c), 1))
        r = L.zsmi_decompress_usingDDictSet(out, len(c), f, len(f), all3.handle)
        assert not L.zsmi_isError(r) and r == len(c) and out.raw[:r] == c, i
        assert L.zsmi_getErrorCode(L.zsmi_decompress_usingDDictSet(out, len(c), f, len(f), None)) == 32          # NULL: zsmi_decompress, and the frame names a dictionary
        assert L.zsmi_getErrorCode(L.zsmi_decompress_usingDDictSet(out, len(c), f, len(f), ab.handle)) == (32 if i % 3 == 2 else 0)
        if len(c) > 1:
            assert L.zsmi_getErrorCode(L.zsmi_decompress_usingDDictSet(out, len(c) - 1, f, len(f), all3.handle)) == 70
    codec.sync()
    for s in (all3, ab, bc_):                                                    # the sets first, then their members
        s.close()
    assert older() == before
    for dd in dds[1:]:
        dd.close()
    assert DD.decode_many(codec, frames[0], caps, dds[0]) == want
    dds[0].close()
    assert B.decode_many(codec, plain, caps, min_cap=0) == want and B.decode_many(codec, frames[1], caps, dics[1], min_cap=0) == want
