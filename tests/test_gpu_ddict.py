"""Digested decode dictionaries on the GPU (zsmi_createDDict, zsmi_decompress*_usingDDict; DecompressionDict): per item the results of the
_usingDict calls with the same dictionary - bytes, sizes, error codes - with dictionary frames decoded on the fast path.  The edge frames are
those of tests/_ddict.py (pinned under oracle D by tests/test_ddict_frames_host.py); dictionaries and chunks: tests/_dicts.py; batches and
children: tests/_batch.py."""
import ctypes, os
import numpy as np
import pytest
import _oracle as O
import _data as D
import _dicts as X
import _batch as B
import _ddict as DD
from _batch import ERR

pytestmark = pytest.mark.gpu
FIX = X.FIX
NAMES = sorted(k[:-6] for k in FIX.files if k.endswith("_frame"))


@pytest.fixture(scope="module")
def codec():
    from zstandard_amd import BatchCodec
    return BatchCodec(0)


def same(a, b, what):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert x == y, (what, i, hex(x[0]), hex(y[0]), len(x[1]), len(y[1]), B.first_difference(x[1], y[1]))


# ------------------------------------------------------------------ 1. the edge frames
@pytest.mark.parametrize("dname", sorted(DD.dictionaries()))
def test_edge_frames_equal_usingdict_and_oracle(codec, dname):
    """valid and invalid frames of one dictionary in ONE batch: the host form with a DDict gives what _usingDict and oracle D give"""
    from zstandard_amd import DecompressionDict
    dic = DD.dictionaries()[dname]
    names, frames, caps = DD.cases_of(dname)
    assert len(frames) >= 2
    dd = DecompressionDict(codec, dic)
    assert dd.dict_id == (0 if dname == "raw" else DD.DICT_ID) and dd.device_bytes >= len(dic)
    got = DD.decode_many(codec, frames, caps, dd)
    dd.close()
    same(got, B.decode_many(codec, frames, caps, dic, min_cap=0), names)
    same(got, DD.oracle_many(frames, caps, dic), names)
    want = {c[0]: c for c in DD.cases()}
    for name, (sz, data) in zip(names, got):
        _, _, _, content, code = want[name]
        assert (sz, data) == ((0x100000000 - code, b"") if code else (len(content), content)), name


_FAST_CHILD = r'''
import os; os.environ["ZSMI_DEBUG_LIB"] = "1"
import sys, ctypes
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import numpy as np, torch
import _batch as B, _ddict as DD
from zstandard_amd import BatchCodec, DecompressionDict, _lib
if _lib.built_fingerprint() != _lib.source_fingerprint():
    _lib.build()
bc = BatchCodec(0); Z = _lib.lib()
lay = (ctypes.c_uint32 * 6)(); Z.zsmi_dbg_descLayout(lay)
WORDS, FAST_AT, WHY_AT = int(lay[0]), int(lay[1]), int(lay[2])
checked = 0
for dname, dic in sorted(DD.dictionaries().items()):
    names, frames, caps = DD.cases_of(dname)
    n = len(frames)
    dd = DecompressionDict(bc, dic)
    # the device form: frames and outputs in device memory, canary behind every output
    src_np, so, ss = B.batch(frames)
    do = B.layout(caps, [16] * n)
    src = torch.from_numpy(src_np.copy()).cuda()
    dst = torch.full((int(do[-1]) + caps[-1] + 64,), B.CANARY, dtype=torch.uint8, device="cuda")
    dsz = torch.zeros(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    bc.decompress_device(src.data_ptr(), so, ss, dst.data_ptr(), do, np.array(caps, dtype=np.uint32), dsz.data_ptr(), ddict=dd)
    bc.sync()
    buf = np.zeros(n * WORDS, dtype=np.uint32)
    assert Z.zsmi_dbg_copyScratch(bc.ctx, b"fastDesc", buf.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(buf.nbytes)) == 0
    desc = buf.reshape(-1, WORDS)
    host = dst.cpu().numpy(); sz = dsz.cpu().numpy().view(np.uint32)
    got = [(int(s), host[int(o):int(o) + (int(s) if s < B.ERR else 0)].tobytes()) for o, s in zip(do, sz)]
    assert got == DD.oracle_many(frames, caps, dic), dname
    assert got == DD.decode_many(bc, frames, caps, dd), dname
    want = {c[0]: c for c in DD.cases()}
    for i, name in enumerate(names):
        if want[name][4] or DD.may_fall_back(name):
            continue
        assert desc[i, FAST_AT] == 1, (name, "left the fast path", int(desc[i, WHY_AT]))
        checked += 1
    dd.close()
assert checked >= 60, checked
print("CHILD-OK", checked)
'''


def test_edge_frames_device_form_on_the_fast_path():
    """a child with the debug-hook library: the device form gives oracle D's results, and ZsFastDesc.fast of block 0 says that every valid
    frame of (a) - (l) was decoded by the fast kernels.  Exempt by name: "m treeless with a table of 12 bits" (its dictionary's Huffman table
    has more than 11 bits, the fast kernels hold none)"""
    B.run_child("-c", _FAST_CHILD, B.ROOT)


# ------------------------------------------------------------------ 2. the committed libzstd fixtures
@pytest.mark.parametrize("kind", ["raw", "trained"])
def test_libzstd_dictionary_frames_decode_in_one_batch(codec, kind):
    from zstandard_amd import DecompressionDict
    names = [n for n in NAMES if n.startswith(kind)]
    dic = FIX[names[0] + "_dict"].tobytes()
    frames = [FIX[n + "_frame"].tobytes() for n in names]; wants = [FIX[n + "_want"].tobytes() for n in names]
    dd = DecompressionDict(codec, dic)
    for n, (sz, got), want in zip(names, DD.decode_many(codec, frames, [len(w) for w in wants], dd), wants):
        assert sz == len(want) and got == want, (n, hex(sz))
    dd.close()


def test_dictionary_errors_through_a_ddict(codec):
    """the cases of test_gpu_dictionary.py::test_dictionary_errors_are_the_references: a wrong dictionary is 32 per item, a corrupt one is
    refused at creation with 30"""
    from zstandard_amd import DecompressionDict
    L = codec.L
    name = "trained_small_l3"
    dic, frame, want = FIX[name + "_dict"].tobytes(), FIX[name + "_frame"].tobytes(), FIX[name + "_want"].tobytes()
    other = bytearray(dic); other[4] ^= 1
    for d, code in [(b"", 32), (FIX["raw_small_l3_dict"].tobytes(), 32), (bytes(other), 32)]:
        dd = DecompressionDict(codec, d)
        (sz, _), = DD.decode_many(codec, [frame], [len(want)], dd)
        dd.close()
        assert sz > ERR and (0x100000000 - sz) == code, (len(d), hex(sz))
    for d in [dic[:9], dic[:40], dic[:120]] + X.bad_dictionaries():
        with pytest.raises(O.OracleError) as e:
            O.decompress_using_dict(frame, len(want), d)
        assert e.value.code == 30
        err = ctypes.c_int(0)
        assert not L.zsmi_createDDict(codec.ctx, d, len(d), ctypes.byref(err)) and err.value == 30
        assert not L.zsmi_createDDict(codec.ctx, d, len(d), None)
        with pytest.raises(RuntimeError, match="error 30"):
            DecompressionDict(codec, d)
    rname = "raw_text_l19"
    dd = DecompressionDict(codec, b"")
    (sz, got), = DD.decode_many(codec, [FIX[rname + "_frame"].tobytes()], [len(FIX[rname + "_want"])], dd)
    dd.close()
    assert (sz, got) == B.decode_many(codec, [FIX[rname + "_frame"].tobytes()], [len(FIX[rname + "_want"])], b"", min_cap=0)[0]


# ------------------------------------------------------------------ 3. round trips
SIZES = ((1024, 48), (4096, 24), (65536, 4), (131073, 2))


def class_chunks(cls):
    data = X.class_data(cls)
    out = []
    for cs, n in SIZES:
        out += [data[(7 * k * cs) % (len(data) - cs):][:cs] for k in range(n)]
    return out


@pytest.mark.parametrize("cls", X.RECORD_CLASSES)
def test_cdict_frames_round_trip(codec, cls):
    from zstandard_amd import CompressionDict, DecompressionDict
    dic, chunks = X.trained(cls), class_chunks(cls)
    dd = DecompressionDict(codec, dic)
    assert dd.dict_id == int.from_bytes(dic[4:8], "little")
    for level in (1, 3):
        cd = CompressionDict(codec, dic, level)
        frames = B.compress_many(codec, chunks, cdict=cd)
        cd.close()
        for i, ((sz, got), c) in enumerate(zip(DD.decode_many(codec, frames, [len(c) for c in chunks], dd), chunks)):
            assert sz == len(c) and got == c, (cls, level, i, len(c), hex(sz))
    dd.close()


def test_raw_content_usingdict_frames_round_trip(codec):
    from zstandard_amd import DecompressionDict
    for name, dic in X.identity_dictionaries().items():
        if not name.startswith("raw"):
            continue
        chunks = X.prefix_chunks(dic)
        frames = B.compress_many(codec, chunks, 3, dic)
        dd = DecompressionDict(codec, dic)
        for i, ((sz, got), c) in enumerate(zip(DD.decode_many(codec, frames, [len(c) for c in chunks], dd), chunks)):
            assert sz == len(c) and got == c, (name, i, len(c), hex(sz))
        dd.close()


def test_frames_without_a_dictionary_decode_with_any_ddict(codec):
    from zstandard_amd import DecompressionDict
    chunks = class_chunks("json_records")
    frames = B.compress_many(codec, chunks, 3)
    plain = B.decode_many(codec, frames, [len(c) for c in chunks], min_cap=0)
    assert plain == [(len(c), c) for c in chunks]
    for dic in (X.trained("zipf"), X.STREAM[:6000], DD.dictionaries()["log12"]):
        dd = DecompressionDict(codec, dic)
        assert DD.decode_many(codec, frames, [len(c) for c in chunks], dd) == plain
        dd.close()


# ------------------------------------------------------------------ 4. device-pointer form
_DEVICE_CHILD = r'''
import sys, os, ctypes
import torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import numpy as np
import _dicts as X, _batch as B, _ddict as DD
from zstandard_amd import BatchCodec, CompressionDict, DecompressionDict
bc = BatchCodec(0)
L = bc.L
dic = X.trained("json_records")
data = X.class_data("json_records", 3 << 20)
rng = np.random.default_rng(4)
sizes = np.concatenate([rng.integers(0, 70000, 40), [1024] * 40, [65536, 65537, 131072, 131073, 200000, 1, 0, 17]]).astype(np.uint32)
chunks = B.cut(np.frombuffer(data[:int(sizes.sum())], dtype=np.uint8), B.layout(sizes), sizes)
cd = CompressionDict(bc, dic, 3)
frames = B.compress_many(bc, chunks, cdict=cd)
cd.close()
src_np, so, ss = B.batch(frames)
src = torch.from_numpy(src_np.copy()).cuda()
dd = DecompressionDict(bc, dic)
ddict_bytes = torch.from_numpy(np.frombuffer(dic, dtype=np.uint8).copy()).cuda()
p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
for short in (0, 1):
    caps = np.maximum(sizes.astype(np.int64) - short, 0).astype(np.uint32)
    # ragged destinations: each capacity long, a gap of 0 .. 299 bytes in front of every second one
    do = B.layout(caps, rng.integers(0, 300, len(caps)) * (np.arange(len(caps)) % 2))
    total = int(do[-1]) + int(caps[-1]) + 4096
    outs = []
    for form in ("ddict", "dict"):
        dst = torch.full((total,), B.CANARY, dtype=torch.uint8, device="cuda")
        dsz = torch.zeros(len(sizes), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        if form == "ddict":
            bc.decompress_device(src.data_ptr(), so, ss, dst.data_ptr(), do, caps, dsz.data_ptr(), ddict=dd)
        else:
            assert L.zsmi_decompressBatchDevice_usingDict(bc.ctx, ctypes.c_void_p(src.data_ptr()), p(so), p(ss), len(ss), ctypes.c_void_p(dst.data_ptr()), p(do), p(caps),
                                                          ctypes.c_void_p(dsz.data_ptr()), ctypes.c_void_p(ddict_bytes.data_ptr()), len(dic)) == 0
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
# NULL is the plain call, byte for byte; an empty DDict too
plain_frames = B.compress_many(bc, chunks, 3)
src2_np, so2, ss2 = B.batch(plain_frames)
src2 = torch.from_numpy(src2_np.copy()).cuda()
do = B.layout(sizes, [8] * len(sizes)); total = int(do[-1]) + int(sizes[-1]) + 64
empty = DecompressionDict(bc, b"")
res = []
for handle in ("plain", None, empty.handle):
    dst = torch.full((total,), B.CANARY, dtype=torch.uint8, device="cuda"); dsz = torch.zeros(len(sizes), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    if handle == "plain":
        bc.decompress_device(src2.data_ptr(), so2, ss2, dst.data_ptr(), do, sizes, dsz.data_ptr())
    else:
        assert L.zsmi_decompressBatchDevice_usingDDict(bc.ctx, ctypes.c_void_p(src2.data_ptr()), p(so2), p(ss2), len(ss2), ctypes.c_void_p(dst.data_ptr()), p(do), p(sizes),
                                                       ctypes.c_void_p(dsz.data_ptr()), handle) == 0
    bc.sync()
    res.append((dst.cpu(), dsz.cpu()))
assert all(torch.equal(res[0][0], r[0]) and torch.equal(res[0][1], r[1]) for r in res[1:])
assert B.cut(res[0][0].numpy(), do, sizes) == chunks
empty.close(); dd.close()
print("CHILD-OK")
'''


def test_device_pointer_form_stays_in_bounds():
    """zsmi_decompressBatchDevice_usingDDict: canary-filled output, ragged capacities, then capacities one byte short - nothing is written
    outside [dstOffsets[i], + dstCaps[i]), sizes, bytes and error codes are those of zsmi_decompressBatchDevice_usingDict; dd == NULL and an
    empty DDict are zsmi_decompressBatchDevice byte for byte"""
    B.run_child("-c", _DEVICE_CHILD, B.ROOT)


# ------------------------------------------------------------------ 5. sub-batches
_SUB_CHILD = r'''
import sys, os
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import numpy as np
import _dicts as X, _batch as B, _ddict as DD
from zstandard_amd import BatchCodec, CompressionDict, DecompressionDict
dic = X.trained("zipf")
bc = BatchCodec()
data = X.class_data("zipf", 4 << 20)
rng = np.random.default_rng(22)
sizes = np.concatenate([rng.integers(0, 100000, 60), [65536] * 20, [1024] * 150, [4096] * 64, [131072] * 6]).astype(np.uint32)
rng.shuffle(sizes)
assert len(sizes) == 300
chunks = B.cut(np.frombuffer(data, dtype=np.uint8), B.layout(sizes) % (len(data) - 131072), sizes)
cd = CompressionDict(bc, dic, 3)
frames = B.compress_many(bc, chunks, cdict=cd)
cd.close()
names, bad_frames, _ = DD.cases_of("narrow")
mixed = list(frames)
caps = [len(c) for c in chunks]
for k in range(0, 300, 37):                                 # frames of another dictionary, and broken ones, among them
    mixed[k] = bad_frames[k % len(bad_frames)]
for k in range(5, 300, 41):
    mixed[k] = frames[k][:len(frames[k]) // 2]
dd = DecompressionDict(bc, dic)
got = DD.decode_many(bc, mixed, caps, dd)
assert got == B.decode_many(bc, mixed, caps, dic, min_cap=0)
for k, (g, c) in enumerate(zip(got, chunks)):
    if mixed[k] is frames[k]:
        assert g == (len(c), c), (k, len(c), hex(g[0]))
    else:
        assert g[0] > B.ERR or len(c) == 0 or g[1] != c, k
dd.close()
print("CHILD-OK")
'''


def test_sub_batches_with_a_ddict():
    """ZSMI_ITEMS_IN_FLIGHT=64 in a child process: 300 mixed frames (sizes from 0 to 128 KiB, frames of another dictionary and cut ones
    among them) take five sub-batches"""
    B.run_child("-c", _SUB_CHILD, B.ROOT, env=dict(os.environ, ZSMI_ITEMS_IN_FLIGHT="64"))


# ------------------------------------------------------------------ 6. lifecycle, 7. the empty DDict
def test_one_ddict_many_calls_and_two_in_alternation(codec):
    from zstandard_amd import CompressionDict, DecompressionDict
    da, db = X.trained("json_records"), X.trained("zipf")
    data = X.class_data("json_records")
    layouts = [[data[i:i + 1024] for i in range(0, 64 * 1024, 1024)],
               [data[0:300], data[1000:66536], data[70000:70000 + 65537], data[200000:200000 + 150000], b"", b"x", data[5:4101]],
               [data[i:i + 4096] for i in range(4096, 40 * 4096, 4096)]]
    ca, cb = CompressionDict(codec, da, 3), CompressionDict(codec, db, 1)
    sets = [(c, B.compress_many(codec, c, 3), B.compress_many(codec, c, cdict=ca), B.compress_many(codec, c, cdict=cb)) for c in layouts]
    ca.close(); cb.close()
    dda, ddb = DecompressionDict(codec, da), DecompressionDict(codec, db)
    assert dda.device_bytes >= len(da) and codec.L.zsmi_sizeofDDict(None) == 0 and codec.L.zsmi_getDictID_fromDDict(None) == 0
    first = {}
    for rnd in range(2):
        for k, (chunks, plain, fa, fb) in enumerate(sets):
            caps = [len(c) for c in chunks]
            want = [(len(c), c) for c in chunks]
            r_plain = B.decode_many(codec, plain, caps, min_cap=0)
            r_a = DD.decode_many(codec, fa, caps, dda)
            r_ud = B.decode_many(codec, fa, caps, da, min_cap=0)
            r_b = DD.decode_many(codec, fb, caps, ddb)
            r_a2 = DD.decode_many(codec, fa, caps, dda)
            r_cross = DD.decode_many(codec, fa, caps, ddb)                 # A's frames with B: dictionary_wrong, every one
            assert r_plain == want and r_a == want and r_ud == want and r_b == want and r_a2 == want
            assert all(sz == 0x100000000 - 32 for sz, _ in r_cross)
            assert B.decode_many(codec, plain, caps, min_cap=0) == r_plain and B.decode_many(codec, fa, caps, da, min_cap=0) == r_ud    # the older calls: unchanged
            if rnd == 0:
                first[k] = (r_plain, r_a, r_ud, r_b, r_cross)
            else:
                assert first[k] == (r_plain, r_a, r_ud, r_b, r_cross)
    codec.L.zsmi_freeDDict(None)
    dda.close(); ddb.close()


def test_one_shot_null_and_empty_forms(codec):
    from zstandard_amd import CompressionDict, DecompressionDict
    L = codec.L
    dic = X.trained("xml_records")
    data = X.class_data("xml_records")
    chunks = [data[:1024], data[2000:2000 + 4096], b"", b"q", data[10000:10000 + 70000]]
    cd = CompressionDict(codec, dic, 3)
    frames = B.compress_many(codec, chunks, cdict=cd)
    cd.close()
    dd = DecompressionDict(codec, dic)
    batch = DD.decode_many(codec, frames, [len(c) for c in chunks], dd)
    for c, f, (sz, got) in zip(chunks, frames, batch):
        out = ctypes.create_string_buffer(max(len(c), 1))
        r = L.zsmi_decompress_usingDDict(out, len(c), f, len(f), dd.handle)
        assert not L.zsmi_isError(r) and r == sz == len(c) and out.raw[:r] == got == c
        assert L.zsmi_getErrorCode(L.zsmi_decompress_usingDDict(out, len(c), f, len(f), None)) == (32 if True else 0)      # NULL: the plain call - the frame names a dictionary
        if len(c) > 1:
            assert L.zsmi_getErrorCode(L.zsmi_decompress_usingDDict(out, len(c) - 1, f, len(f), dd.handle)) == 70
    # dd == NULL and an empty DDict: the plain call, also for frames that need no dictionary
    plain = B.compress_many(codec, chunks, 3)
    caps = [len(c) for c in chunks]
    want = B.decode_many(codec, plain, caps, min_cap=0)
    empty = DecompressionDict(codec, b"")
    assert empty.dict_id == 0
    assert DD.decode_many(codec, plain, caps, empty) == want == [(len(c), c) for c in chunks]
    assert DD.decode_many(codec, frames, caps, empty) == B.decode_many(codec, frames, caps, min_cap=0)
    for c, f in zip(chunks, plain):
        out = ctypes.create_string_buffer(max(len(c), 1))
        for h in (None, empty.handle):
            r = L.zsmi_decompress_usingDDict(out, len(c), f, len(f), h)
            assert r == len(c) and out.raw[:r] == c
    err = ctypes.c_int(7)
    h = L.zsmi_createDDict(codec.ctx, None, 0, ctypes.byref(err))
    assert h and err.value == 0 and L.zsmi_getDictID_fromDDict(h) == 0
    L.zsmi_freeDDict(h)
    empty.close(); dd.close()
