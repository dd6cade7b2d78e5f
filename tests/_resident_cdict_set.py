"""Device-resident compress with a CDict set in the GPU tests (test infrastructure): the members and batches of
tests/test_gpu_resident_cdict_set.py and the one comparison it makes in every setting - zsmi_compressBatchResident_usingCDictSet, its
descriptors and the dictionary index of every chunk in device memory, against zsmi_compressBatchDevice_usingCDictSet with the same arrays
from the host: chunk by chunk the same size word and the same place, nothing written outside a chunk's place, and for a refused chunk
(above max_src_size, or an index that names no member) the refusal's word and no byte beyond zsmi_compressBound(0).
Built on tests/_resident_compress.py (Batch, assert_equal_to_host_call) and tests/_cdict_set.py (members(), NO_DICT, SIZES_EVERY_KIND_HAS)."""
import numpy as np
import _batch as B, _cdict_set as S, _dicts as X, _resident_compress as RC
from _hip import Dev, CANARY
from _resident import up, down

KIB = 1 << 10
NO_DICT = S.NO_DICT
SIZE_REFUSED = RC.REFUSED                # (uint32_t)-ZSMI_error_srcSize_wrong
INDEX_REFUSED = 0x100000000 - 42         # (uint32_t)-ZSMI_error_parameter_outOfBound

# the set of the tests, by the names of _cdict_set.members(): two formatted members (IDs in a 4-byte and in a shorter field), raw content
# of 6000 and of 100 000 bytes (only its last 64 KiB are a prefix), a third formatted one, the empty CDict, and the first once more
SET = ("trained8k", "raw6000", "id_0xffffffff", "raw100000", "trained64k_json_records", "empty", "again")
KINDS = {"formatted": SET.index("trained8k"), "raw": SET.index("raw6000"), "empty": SET.index("empty"), "none": NO_DICT, "again": SET.index("again")}


def dictionaries():
    """the bytes of the set's members, in set order (b"": the empty CDict)"""
    by_name = dict(S.members())
    return [by_name[name] for name in SET]


def make_set(codec, level):
    """(CompressionDictSet, its CompressionDicts): `again` is the CDict of `trained8k`, one object at two indices"""
    from zstandard_amd import CompressionDict, CompressionDictSet
    cds = [None if name == "again" else CompressionDict(codec, d, level) for name, d in zip(SET, dictionaries())]
    cds[SET.index("again")] = cds[SET.index(S.AGAIN_OF)]
    return CompressionDictSet(codec, cds, level), cds


def every_kind_at_every_size(max_src):
    """[(chunk, choice)]: every kind of choice with _dicts.prefix_chunks of its dictionary at every size of SIZES_EVERY_KIND_HAS that fits
    max_src (an empty member and NO_DICT: those of the raw dictionary) - the sizes, the small record sizes of every corpus class, the
    contents aimed at the prefix - dealt round robin so that neighbours differ; then 20 seeded chunks of the stream with seeded choices"""
    dics = dictionaries()
    sizes = tuple(s for s in S.SIZES_EVERY_KIND_HAS if s <= max_src)
    per = []
    for kind, choice in KINDS.items():
        dic = dics[choice] if choice != NO_DICT and dics[choice] else dics[KINDS["raw"]]
        per.append([(c, choice) for c in X.prefix_chunks(dic, sizes) if len(c) <= max_src])
    items = [lst[j] for j in range(max(len(lst) for lst in per)) for lst in per if j < len(lst)]
    for s in sizes:
        for choice in KINDS.values():
            assert any(len(c) == s and ch == choice for c, ch in items), (s, choice)
    rng = np.random.default_rng(max_src + 7)
    data = RC.stream_bytes()
    picks = list(range(len(SET))) + [NO_DICT]
    for s in rng.integers(0, max_src + 1, 20):
        at = int(rng.integers(0, len(data) - int(s)))
        items.append((data[at:at + int(s)], picks[int(rng.integers(0, len(picks)))]))
    return items


class Batch(RC.Batch):
    """RC.Batch with a dictionary index a chunk, on the host and on the device"""

    def __init__(self, codec, H, items, seed=5):
        super().__init__(codec, H, [c for c, _ in items], seed)
        self.index = np.array([ch for _, ch in items], dtype=np.uint32)
        self.d_index = up(H, self.index)

    def run_set(self, resident, cset, max_src=0, index=None, null_index=False, cdict=None):
        """(size words, the whole destination buffer) of one call with the set.  index: another choice than the batch's (host array: it goes
        up for the resident call); null_index: the resident call without an index array; cdict: the host-array call with this CDict instead"""
        dst, dsz = Dev(self.H, self.total), Dev(self.H, 4 * self.n)
        idx = self.index if index is None else np.ascontiguousarray(index, dtype=np.uint32)
        d_idx = self.d_index if index is None else up(self.H, idx)
        if resident:
            self.codec.compress_resident(self.src.p, self.d_so.p, self.d_ss.p, self.n, max_src, dst.p, self.d_do.p, dsz.p, cdict_set=cset,
                                         d_dict_index_ptr=0 if null_index else d_idx.p)
        elif cdict is not None:
            self.codec.compress_device(self.src.p, self.so, self.ss, dst.p, self.do, dsz.p, cdict=cdict)
        else:
            self.codec.compress_device(self.src.p, self.so, self.ss, dst.p, self.do, dsz.p, cdict_set=cset, dict_index=idx)
        self.codec.sync()
        host, ok1 = down(dst)
        sz, ok2 = down(dsz, np.uint32)
        _, ok3 = down(d_idx, np.uint32)
        assert ok1 and ok2 and ok3, ("resident" if resident else "host arrays", "a canary around a buffer is gone")
        dst.free(); dsz.free()
        if index is not None:
            d_idx.free()
        return sz.copy(), host.copy()

    def free(self):
        super().free()
        self.d_index.free()


def assert_equal_with_refusals(batch, ref, got, refused, what=""):
    """RC.assert_equal_to_host_call where chunks may be refused for their index too.  refused: {chunk: its word}; got = (sizes, buffer) of
    the resident call, ref = the host-array call's on the same batch with a choice it accepts for the refused chunks"""
    (hsz, hbuf), (rsz, rbuf) = ref, got
    bound0 = batch.codec.L.zsmi_compressBound(0)
    inside = np.zeros(batch.total, dtype=bool)
    for o, b in zip(batch.do, batch.bounds):
        inside[int(o):int(o) + int(b)] = True
    bad = np.flatnonzero(~inside & (rbuf != CANARY))
    assert bad.size == 0, (what, "written outside the chunks' places", bad[:8].tolist())
    for i, (o, s, b) in enumerate(zip(batch.do, batch.ss, batch.bounds)):
        o, b = int(o), int(b)
        if i in refused:
            assert int(rsz[i]) == refused[i], (what, "refused chunk", i, hex(int(rsz[i])))
            assert (rbuf[o + min(bound0, b):o + b] == CANARY).all(), (what, "a refused chunk's place written beyond compressBound(0)", i)
        else:
            assert int(rsz[i]) == int(hsz[i]) < B.ERR, (what, "size word of chunk", i, int(s), hex(int(hsz[i])), hex(int(rsz[i])))
            same = rbuf[o:o + b] == hbuf[o:o + b]
            assert same.all(), (what, "frame of chunk", i, int(s), int(batch.index[i]), "first difference at", int(np.flatnonzero(~same)[0]))


def frame_dict_id(frame):
    """the Dictionary_ID a frame header carries (0: none)"""
    code = frame[4] & 3
    return int.from_bytes(frame[5:5 + (4 if code == 3 else code)], "little") if code else 0


def child(n=150):
    """run in a process of its own (ZSMI_BLOCKS_IN_FLIGHT=64): n chunks of 0 .. 200 KiB with seeded choices, max_src_size 200 KiB - four
    blocks a chunk at most, so sub-batches of 16 chunks, ten of them, each planned on the device into the lists the one before used"""
    from _hip import hip_of
    from zstandard_amd import BatchCodec
    bc = BatchCodec(0); H = hip_of()
    rng = np.random.default_rng(151)
    data = RC.stream_bytes()
    edge = [0, 200 * KIB, 1, 65536, 65537, 131072, 131073]
    # most chunks of at most 64 KiB (the prefixed units), the rest up to 200 KiB (small tails and big units)
    sizes = edge + [int(rng.integers(0, 65537)) if k % 3 else int(rng.integers(65537, 200 * KIB + 1)) for k in range(n - len(edge))]
    order = rng.permutation(n)
    picks = list(range(len(SET))) + [NO_DICT]
    items = []
    for i in order:
        s = sizes[i]
        at = int(rng.integers(0, len(data) - s))
        items.append((data[at:at + s], picks[int(rng.integers(0, len(picks)))]))
    cset, cds = make_set(bc, 3)
    batch = Batch(bc, H, items)
    ref = batch.run_set(False, cset)
    got = batch.run_set(True, cset, 200 * KIB)
    RC.assert_equal_to_host_call(batch, ref, got, 200 * KIB, "sub-batches of 16 chunks, a set")
    assert (ref[0] < B.ERR).all()
    # every kind of unit list in most sub-batches
    kinds = [0, 0, 0]
    for g in range(0, n, 16):
        part = items[g:g + 16]
        kinds[0] += any(0 < len(c) <= 65536 and ch != NO_DICT and SET[ch] != "empty" for c, ch in part)
        kinds[1] += any(0 < len(c) <= 65536 and (ch == NO_DICT or SET[ch] == "empty") or 0 < len(c) % 131072 <= 65536 < len(c) for c, ch in part)
        kinds[2] += any(len(c) > 65536 for c, _ in part)
    assert min(kinds) >= 8, kinds
    batch.free(); cset.close()
    for cd in set(cds):
        cd.close()
    bc.close()
    print("CHILD-OK")
