"""The adversary of tests/test_gpu_scratch_independence.py (test infrastructure): every call family of the library is held against its
existing oracle on a context whose scratch was overwritten first (zsmi_dbg_fillScratch of the debug-hook library: every buffer a
zsmi_ctx keeps from call to call, DESIGN.md "What a context's memory may carry from call to call").

A family is one child process: `python tests/_poison.py <family>` with ZSMI_DEBUG_LIB=1.  Its schedule, for every case (hold()):
  1. the case on the context as it is (for the first case: fresh);
  2. for each pattern of PATTERNS - 0x00, 0xFF, a seeded mix of small and large words -: fill, then the case;
  3. fill, the case's hostile predecessors, the case;
  4. the case with its output buffers prefilled with 0x00 and with 0xFF instead of the canary.
Every run is compared in full with the family's independent reference (oracle E, oracle D, the Python statements of tests/_split.py
and tests/_seekable.py, the scalar trainer of tests/c/train_model.c) - never with another run -, and what lies around and
between the outputs must still hold what it was prefilled with.  After each fill the bytes the hook reports for the family's group must
reach what zsmi_dbg_scratchLayout predicts for the call before it: the poison cannot be vacuous.

The same module states the compress batch (chunks()), which tests/test_scratch_poison_host.py parses on the CPU."""
import ctypes, json, os, sys, time
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANARY, PAD = 0xA5, 4096
PATTERNS = (0x00, 0xFF, 0x5EED0BAD)         # (the last: any value above 255 asks for the mix; this one seeds it)
PREFILLS = (0x00, 0xFF)
LEVELS = (1, 3, 4)
KIB = 1 << 10
BLOCK = 64 * KIB
COMPRESS_ROWS = ("dist", "distHi", "cand", "recs", "res", "seqs", "hdrs", "lits", "streams", "litSec", "seqSec", "metas")

# ================================================================================================ the compress batch
_made = {}


def _text():
    if "text" not in _made:
        import _data as D
        _made["text"] = D.zipf_log(600000, single=True).tobytes()
    return _made["text"]


def _noise(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def chunks():
    """[(name, bytes)] of the compress batch, in its first order.  What each is there for is in its name's comment; that oracle E's frames
    really have these shapes is asserted on the CPU (tests/test_scratch_poison_host.py)."""
    if "chunks" not in _made:
        text, noise = _text(), _noise(BLOCK, 20261020)
        rng = np.random.default_rng(7)
        js = json.dumps([{"id": i, "name": "n%d" % i, "ok": bool(i & 1)} for i in range(20)]).encode()[:200]
        _made["chunks"] = [
            ("empty", b""),                                             # a frame of one empty raw block
            ("one byte", b"Z"),                                         # no hashable position: the unit's parse is skipped
            ("json 200", js),                                           # few sequences: the three predefined tables
            ("text 8193", text[:8193]),                                 # 33 walk ranges of 256 positions
            ("noise 64 KiB", noise),                                    # a matchless unit: no walk, a raw block
            ("one byte x 64 KiB", b"\x37" * BLOCK),                     # candidates and walk skipped, an RLE block
            ("noise with one repeat", noise[:3000] + noise[:1000]),     # a single sequence: three RLE tables
            ("text 65537", text[:65537]),                               # a big unit whose second block is 1 byte
            ("text 128 KiB", text[1000:1000 + 2 * BLOCK]),              # a big unit, two full blocks
            ("text 200 KiB", text[5000:5000 + 200 * KIB]),              # a big unit plus a tail unit: four blocks
            ("six-bit noise 64 KiB", (rng.integers(0, 64, BLOCK, dtype=np.uint8) + 32).astype(np.uint8).tobytes()),   # matchless, but Huffman pays: a compressed block without sequences
        ]
    return _made["chunks"]


def orders(n):
    """the orders a batch of n chunks is run in: as listed, reversed, rotated by three - a slot that held a long sequence list then holds a
    block with none, and so on for the other kinds"""
    fwd = list(range(n))
    return {"as listed": fwd, "reversed": fwd[::-1], "rotated by three": fwd[3:] + fwd[:3]}


def hostile(parts, kind):
    """the same layout with other contents: noise, or text"""
    if kind == "noise":
        return [_noise(len(c), 1000 + i) for i, c in enumerate(parts)]
    text = _text()
    return [text[(7919 * i) % 1000:][:len(c)] for i, c in enumerate(parts)]


def dict_chunks():
    """the batch trimmed to chunks of 64 KiB or less, plus the one of 65537 bytes (a dictionary call parses it as without a dictionary)"""
    return [(n, c) for n, c in chunks() if len(c) <= BLOCK or len(c) == 65537]


def blocks_of(parts):
    return sum(max((len(c) + BLOCK - 1) // BLOCK, 1) for c in parts)


# ================================================================================================ the hook
def fill(codec, pattern):
    from zstandard_amd import _lib
    return _lib.fill_scratch(codec.ctx, pattern)


def compress_scratch_bytes(blocks_in_call, largest_chunk_blocks, in_flight=16384):
    """the bytes Scratch::reserve asks for a call: every row of ZS_SCRATCH_TABLE at the sub-batch's blocks, and its fixed tail"""
    from zstandard_amd import _lib
    cap = max(min(blocks_in_call, max(64, in_flight)), largest_chunk_blocks)
    return sum(cap * slot + tail for slot, tail in (_lib.scratch_layout(r) for r in COMPRESS_ROWS))


def decode_scratch_bytes(items, fast=True):
    """a lower bound of what DecodeScratch::each asks for a call of `items` items (fewer than the general kernel's pool): a literal
    buffer an item, and with the fast path a Huffman table, the sequence tables and two descriptors an item at least"""
    from zstandard_amd import _lib
    per = _lib.scratch_layout("poolLit")[0]
    if fast:
        per += _lib.scratch_layout("hufTabs")[0] + _lib.scratch_layout("seqTabs")[0] + 2 * _lib.scratch_layout("fastDesc")[0]
    return items * per


class Case:
    """run(prefill) -> whatever check(result, what) compares IN FULL with the reference; hostile: callables run in front of the case in
    step 3; group, predicted: the hook's group the calls use and the bytes it must have filled after the case ran"""

    def __init__(self, name, run, check, hostile=(), group="compress", predicted=1):
        self.name, self.run, self.check, self.hostile, self.group, self.predicted = name, run, check, hostile, group, predicted


def not_vacuous(case, filled):
    """the hook filled, in every group the case's calls use, at least what their layouts predict (predicted: bytes of case.group, or
    {group: bytes})"""
    want = case.predicted if isinstance(case.predicted, dict) else {case.group: case.predicted}
    for group, least in want.items():
        assert least > 0 and filled[group] >= least, (case.name, "the fill is vacuous", group, filled, want)


def hold(codec, case, log):
    """the schedule of the module's docstring for one case"""
    t0 = time.time()
    case.check(case.run(CANARY), (case.name, "as the context was"))
    for pattern in PATTERNS:
        not_vacuous(case, fill(codec, pattern))
        case.check(case.run(CANARY), (case.name, "scratch filled with %#x" % pattern))
    not_vacuous(case, fill(codec, PATTERNS[2]))
    for h in case.hostile:
        h()
    case.check(case.run(CANARY), (case.name, "behind its hostile predecessor"))
    for prefill in PREFILLS:
        case.check(case.run(prefill), (case.name, "output prefilled with %#x" % prefill))
    log.append((case.name, round(time.time() - t0, 3)))


# ================================================================================================ host-array calls, every buffer guarded
def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def host_call(fn, ctx, items, lens, tail, prefill, gaps=True):
    """one host-array batch call (compress or decompress: fn(ctx, src, srcOffsets, srcSizes, n, dst, dstOffsets, [dstCaps,] dstSizes, *tail))
    -> [(size or error word, the bytes written for a size)].  Item i's place is lens[i] bytes; the places lie PAD bytes into a buffer
    prefilled with `prefill`, with gaps between them, and nothing outside [place, place + size) may change; the size words lie between two
    guard words"""
    import _batch as B
    n = len(items)
    src, so, ss = B.batch(items)
    lens = np.asarray(lens, dtype=np.uint64)
    do = (B.layout(lens, [(5 + 11 * (i % 7)) if gaps else 0 for i in range(n)]) + np.uint64(PAD)).astype(np.uint64)
    total = int(do[-1]) + int(lens[-1]) + PAD if n else 2 * PAD
    arena = np.full(total, prefill, dtype=np.uint8)
    words = np.full(n + 2, 0xA5A5A5A5, dtype=np.uint32)
    rc = fn(ctx, _p(src), _p(so), _p(ss), n, _p(arena), _p(do), *tail(lens), ctypes.c_void_p(words.ctypes.data + 4))
    assert rc == 0, ("the call's code", rc)
    assert words[0] == 0xA5A5A5A5 and words[-1] == 0xA5A5A5A5, "written outside the size words"
    out, spans = [], []
    for i in range(n):
        w, o = int(words[1 + i]), int(do[i])
        size = w if w < B.ERR else 0
        assert size <= int(lens[i]), ("item", i, "a size above its place", size, int(lens[i]))
        spans.append((o, o + size))
        out.append((w, arena[o:o + size].tobytes()))
    bad = outside_untouched(arena, spans, prefill)
    assert not bad, ("written outside the results", bad, [int(v) for v in do[:8]])
    return out


def outside_untouched(buf, spans, prefill):
    """the offsets (at most 8) of bytes of buf outside every [start, end) of spans - ascending, disjoint - that differ from prefill"""
    bad, at = [], 0
    for a, b in list(spans) + [(len(buf), len(buf))]:
        seg = buf[at:a]
        if seg.size and not (seg == prefill).all():
            bad += (np.flatnonzero(seg != prefill)[:8] + at).tolist()
        at = max(at, b)
    return bad[:8]


def compress_host(codec, parts, prefill, level=3, dictionary=b"", cdict=None, cdict_set=None, dict_index=None):
    L = codec.L
    dbuf = np.frombuffer(bytes(dictionary), dtype=np.uint8) if dictionary else np.zeros(1, dtype=np.uint8)
    di = None if dict_index is None else np.ascontiguousarray(dict_index, dtype=np.uint32)
    name, tail = codec._compress_form("zsmi_compressBatchHost", level, _p(dbuf), len(dictionary), cdict, cdict_set, di)
    bounds = [L.zsmi_compressBound(len(c)) for c in parts]
    # (the C argument order: ..., dst, dstOffsets, dstSizes, then the form's tail)
    return host_call(lambda ctx, s, so, ss, n, d, do, dsz: getattr(L, name)(ctx, s, so, ss, n, d, do, dsz, *tail), codec.ctx, parts, bounds, lambda lens: (), prefill)


def decompress_host(codec, frames, caps, prefill, dictionary=b"", ddict=None, ddict_set=None):
    L = codec.L
    caps32 = np.ascontiguousarray(caps, dtype=np.uint32)
    if ddict_set is not None:
        fn = lambda ctx, s, so, ss, n, d, do, dc, dsz: L.zsmi_decompressBatchHost_usingDDictSet(ctx, s, so, ss, n, d, do, dc, dsz, ddict_set.handle)
    elif ddict is not None:
        fn = lambda ctx, s, so, ss, n, d, do, dc, dsz: L.zsmi_decompressBatchHost_usingDDict(ctx, s, so, ss, n, d, do, dc, dsz, ddict.handle)
    elif dictionary:
        dbuf = np.frombuffer(bytes(dictionary), dtype=np.uint8)
        fn = lambda ctx, s, so, ss, n, d, do, dc, dsz: L.zsmi_decompressBatchHost_usingDict(ctx, s, so, ss, n, d, do, dc, dsz, _p(dbuf), len(dbuf))
    else:
        fn = L.zsmi_decompressBatchHost
    return host_call(fn, codec.ctx, frames, caps32, lambda lens: (_p(caps32),), prefill)


def same(got, want, what):
    """item by item the same word and the same bytes; want: [(word, bytes)]"""
    import _batch as B
    assert len(got) == len(want), what
    for i, (g, w) in enumerate(zip(got, want)):
        assert g[0] == w[0], (what, "item", i, "size or error word", hex(g[0]), hex(w[0]))
        assert g[1] == w[1], (what, "item", i, "bytes differ at", B.first_difference(g[1], w[1]), len(w[1]))


def as_frames(frames):
    return [(len(f), f) for f in frames]


# ================================================================================================ device buffers with any prefill
class Guarded:
    """a device buffer of n bytes prefilled with `prefill` between two canary pads; fill: bytes copied to its start"""

    def __init__(self, H, n, prefill=CANARY, fill=b""):
        from _hip import Dev
        self.d, self.n, self.prefill = Dev(H, max(n, 1), b""), max(n, 1), prefill
        if prefill != CANARY:
            assert H.hipMemset(ctypes.c_void_p(self.d.p), prefill, self.n) == 0
        if fill:
            assert H.hipMemcpy(ctypes.c_void_p(self.d.p), bytes(fill), len(fill), 1) == 0
        # the fills run on the null stream and the codec's stream does not wait for that one: a fill of hundreds of MiB still under way
        # when the call's kernels store their results would overwrite them
        assert H.hipDeviceSynchronize() == 0
        self.p = self.d.p

    def body(self, dtype=np.uint8):
        raw = np.frombuffer(self.d.all(), dtype=np.uint8)
        assert (raw[:PAD] == CANARY).all() and (raw[PAD + self.n:] == CANARY).all(), "a canary around a device buffer is gone"
        b = raw[PAD:PAD + self.n]
        return b[:self.n - self.n % np.dtype(dtype).itemsize].view(dtype).copy()

    def free(self):
        self.d.free()


def up(H, arr):
    a = np.ascontiguousarray(arr)
    return Guarded(H, a.nbytes, CANARY, a.tobytes())


# ================================================================================================ family: compress, host arrays
def family_compress(in_flight=None):
    """levels 1, 3 and 4, the batch in three orders, against oracle E byte for byte.  in_flight (ZSMI_BLOCKS_IN_FLIGHT=64 in the
    environment): enough copies of the batch for three sub-batches, so that slots are reused inside one call - and enough frames for the
    packed way back (copyBack's second path)"""
    import _batch as B
    from zstandard_amd import BatchCodec
    bc = BatchCodec(0)
    log = []
    base = [c for _, c in chunks()]
    copies = 1
    if in_flight:
        assert os.environ.get("ZSMI_BLOCKS_IN_FLIGHT") == str(in_flight)
        while blocks_of(base) * copies <= 2 * in_flight:
            copies += 1
    for level in LEVELS:
        for oname, order in orders(len(base)).items():
            parts = [base[i] for i in order] * copies
            want = as_frames(B.oracle_frames(parts, level))
            if in_flight:
                assert 2 * in_flight < blocks_of(parts) <= 3 * in_flight + 4, blocks_of(parts)
            hold(bc, Case("level %d, %s%s" % (level, oname, ", %d copies" % copies if copies > 1 else ""),
                          lambda prefill, parts=parts, level=level: compress_host(bc, parts, prefill, level),
                          lambda got, what, want=want: same(got, want, what),
                          hostile=[lambda parts=parts, level=level, k=k: compress_host(bc, hostile(parts, k), CANARY, level) for k in ("noise", "text")],
                          group="compress", predicted=compress_scratch_bytes(blocks_of(parts), 4, in_flight or 16384)), log)
    bc.close()
    return log


# ================================================================================================ family: compress with dictionaries
DIGESTS = os.path.join(ROOT, "tests", "golden", "scratch_poison_cdict_digests.json")


def check_digest(name, got, what):
    """the frames of a digested formatted dictionary may use its tables, and no oracle writes those: beside the oracle D round trip they are
    pinned by digest (tests/_cdict.py frames_digest; tests/golden/scratch_poison_cdict_digests.json, taken from frames that passed the
    round trip), so that a frame that is wrong and still decodes shows"""
    import _cdict as K
    pinned = json.load(open(DIGESTS))
    assert K.frames_digest([f for _, f in got]) == pinned[name], (what, name, "the frames differ from the pinned ones")


def family_compress_dict():
    """_usingDict (raw content and a formatted dictionary), _usingCDict, a CDict set with formatted, raw, empty and NO_DICT choices, and the
    checksum flag.  Reference: oracle E wherever it states the frame - every _usingDict frame, and the frames of raw-content, empty and
    absent dictionaries of the digested forms.  A digested FORMATTED dictionary's frames may use its tables, which no oracle writes and
    whose pinned digests (tests/golden/cdict_frame_digests.json) are of other records: those are held to an oracle D round trip with the
    dictionary, to the compress bound, and to digests of their own for this batch (check_digest)."""
    import _batch as B, _checksum as CK, _dicts as X, _oracle as O
    from zstandard_amd import BatchCodec, CompressionDict, CompressionDictSet, NO_DICT
    bc = BatchCodec(0)
    log = []
    parts = [c for _, c in dict_chunks()]
    raw, formatted = X.STREAM[:6000], X.TRAINED8K
    nb = blocks_of(parts)
    predicted = compress_scratch_bytes(nb, 2)
    pre = lambda level, dic="": [lambda k=k: compress_host(bc, hostile(parts, k), CANARY, level, dic) for k in ("noise", "text")]

    def round_trip(got, dics, what):
        for i, ((w, f), c, dic) in enumerate(zip(got, parts, dics)):
            assert w == len(f) <= bc.L.zsmi_compressBound(len(c)), (what, i, hex(w))
            assert (O.decompress_using_dict(f, len(c), dic) if dic else O.decompress(f, len(c))) == c, (what, "oracle D", i)

    for level in LEVELS:
        for dname, dic in (("raw content", raw), ("a formatted dictionary", formatted)):
            want = as_frames(B.oracle_frames(parts, level, dic))
            hold(bc, Case("_usingDict, %s, level %d" % (dname, level), lambda prefill, level=level, dic=dic: compress_host(bc, parts, prefill, level, dic),
                          lambda got, what, want=want: same(got, want, what), hostile=pre(level, dic), predicted=predicted), log)
    for level in LEVELS:
        cd_raw, cd_fmt, cd_empty = CompressionDict(bc, raw, level), CompressionDict(bc, formatted, level), CompressionDict(bc, b"", level)
        want = as_frames(B.oracle_frames(parts, level, raw))
        hold(bc, Case("_usingCDict, raw content, level %d" % level, lambda prefill, cd=cd_raw: compress_host(bc, parts, prefill, cdict=cd),
                      lambda got, what, want=want: same(got, want, what), hostile=pre(level), predicted=predicted), log)
        hold(bc, Case("_usingCDict, formatted, level %d" % level, lambda prefill, cd=cd_fmt: compress_host(bc, parts, prefill, cdict=cd),
                      lambda got, what, level=level: (round_trip(got, [formatted] * len(parts), what), check_digest("usingCDict formatted, level %d" % level, got, what)),
                      hostile=pre(level, raw), predicted=predicted), log)
        # the set: formatted, raw, empty and no dictionary, neighbours differ
        cset = CompressionDictSet(bc, [cd_fmt, cd_raw, cd_empty], level)
        index = np.array([(0, 1, 2, NO_DICT)[i % 4] for i in range(len(parts))], dtype=np.uint32)
        dics = [(formatted, raw, b"", b"")[i % 4] for i in range(len(parts))]
        stated = {i: O.compress_using_dict(c, dics[i], level) if dics[i] else O.compress(c, level) for i, c in enumerate(parts) if i % 4 != 0}

        def check_set(got, what, stated=stated, dics=dics, level=level):
            round_trip(got, dics, what)
            check_digest("usingCDictSet, level %d" % level, got, what)
            for i, f in stated.items():
                assert got[i] == (len(f), f), (what, "oracle E", i)
        hold(bc, Case("_usingCDictSet, level %d" % level, lambda prefill, cset=cset, index=index: compress_host(bc, parts, prefill, cdict_set=cset, dict_index=index),
                      check_set, hostile=pre(level, formatted), predicted=predicted), log)
        if level == 3:
            bc.set_parameter("checksum", 1)
            want = [(len(f) + 4, CK.with_checksum(f, c)) for f, c in zip(B.oracle_frames(parts, level, raw), parts)]
            hold(bc, Case("checksum flag, _usingCDict raw content", lambda prefill, cd=cd_raw: compress_host(bc, parts, prefill, cdict=cd),
                          lambda got, what, want=want: same(got, want, what), hostile=pre(level), predicted=predicted), log)
            want = [(len(f) + 4, CK.with_checksum(f, c)) for f, c in zip(B.oracle_frames(parts, level), parts)]
            hold(bc, Case("checksum flag, plain", lambda prefill: compress_host(bc, parts, prefill, level),
                          lambda got, what, want=want: same(got, want, what), hostile=pre(level, raw), predicted=predicted), log)
            bc.set_parameter("checksum", 0)
        bc.sync(); cset.close()
        for cd in (cd_raw, cd_fmt, cd_empty):
            cd.close()
    bc.close()
    return log


# ================================================================================================ family: resident compress
REFUSED_SRC = 0x100000000 - 72           # (uint32_t)-ZSMI_error_srcSize_wrong


def resident_compress(bc, H, parts, prefill, max_src, level=3, cset=None, index=None):
    """bounds -> layout -> compress, every descriptor in device memory -> [(word, frame bytes)]; nothing outside the chunks' places may change"""
    import _batch as B
    L, n = bc.L, len(parts)
    src_np, so, ss = B.batch(parts)
    src, d_so, d_ss = up(H, src_np), up(H, so), up(H, ss)
    d_bounds, d_caps, d_off = Guarded(H, 8 * n, prefill), Guarded(H, 4 * n, prefill), Guarded(H, 8 * (n + 1), prefill)
    bounds = np.array([L.zsmi_compressBound(len(c)) for c in parts], dtype=np.uint64)
    align = 64
    want_off = B.layout((bounds + align - 1) // align * align)
    room = int(want_off[-1]) + int(bounds[-1]) + align
    dst, dsz = Guarded(H, room, prefill), Guarded(H, 4 * n, prefill)
    d_ix = up(H, np.ascontiguousarray(index, dtype=np.uint32)) if index is not None else None
    bufs = [src, d_so, d_ss, d_bounds, d_caps, d_off, dst, dsz] + ([d_ix] if d_ix else [])
    try:
        bc.compress_bounds_device(d_ss.p, n, d_bounds.p)
        bc.layout_outputs_device(d_bounds.p, 0, n, d_caps.p, d_off.p, align=align)
        if cset is None:
            bc.compress_resident(src.p, d_so.p, d_ss.p, n, max_src, dst.p, d_off.p, dsz.p, level)
        else:
            bc.compress_resident(src.p, d_so.p, d_ss.p, n, max_src, dst.p, d_off.p, dsz.p, cdict_set=cset, d_dict_index_ptr=d_ix.p)
        bc.sync()
        assert (d_bounds.body(np.uint64) == bounds).all() and (d_caps.body(np.uint32) == bounds).all(), "zsmi_compressBoundsDevice / the layout's capacities"
        off = d_off.body(np.uint64)
        assert (off[:n] == want_off).all() and int(off[n]) == int(want_off[-1]) + int((bounds[-1] + align - 1) // align * align), "zsmi_layoutOutputsDevice"
        for b in (src, d_so, d_ss):
            b.body()                                                     # (the inputs' canaries)
        words, host = dsz.body(np.uint32), dst.body()
        out, spans = [], []
        for i in range(n):
            w, o = int(words[i]), int(want_off[i])
            size = w if w < B.ERR else 0
            assert size <= int(bounds[i]), ("chunk", i, "a size above its bound")
            # a chunk's place is its bound: a one-block frame is built in place, and a literal section that lost to the raw block ends a few
            # bytes behind it.  A refused chunk was planned as an empty one: its place may hold that frame, no more
            keep = int(bounds[i]) if w < B.ERR else (L.zsmi_compressBound(0) if w == REFUSED_SRC else 0)
            spans.append((o, o + keep))
            out.append((w, host[o:o + size].tobytes()))
        bad = outside_untouched(host, spans, prefill)
        assert not bad, ("written outside the chunks' places", bad)
        return out
    finally:
        for b in bufs:
            b.free()


def resident_bytes(n, blocks_a_chunk, with_set=False):
    """what a resident compress call of n chunks of at most blocks_a_chunk blocks (one sub-batch) reserves: the plan kernels' lists in
    the `resident` group - a chunk descriptor (32 bytes), the unit sums (12) and the counts of a sub-batch (16), a block descriptor (24)
    a block slot, a unit descriptor (16) a unit slot, with a set a record index a chunk and a prefixed unit besides - and the compress
    scratch of n * blocks_a_chunk block slots"""
    units = n + (n * ((blocks_a_chunk + 1) // 2) if blocks_a_chunk > 1 else 0) + (n if with_set else 0)
    plan = n * 32 + n * 12 + 16 + n * blocks_a_chunk * 24 + units * 16 + (8 * n if with_set else 0)
    return {"resident": plan, "compress": compress_scratch_bytes(n * blocks_a_chunk, blocks_a_chunk)}


def family_resident():
    """the batch through zsmi_compressBoundsDevice, zsmi_layoutOutputsDevice and zsmi_compressBatchResident, plainly and with a CDict set;
    one case with chunks above maxSrcSize.  Reference: oracle E, and the refusal's word"""
    import _batch as B, _dicts as X, _oracle as O
    from _hip import hip_of
    from zstandard_amd import BatchCodec, CompressionDict, CompressionDictSet, NO_DICT
    bc = BatchCodec(0); H = hip_of()
    log = []
    base = [c for _, c in chunks()]
    top = max(len(c) for c in base)
    for level in LEVELS:
        for oname, order in orders(len(base)).items():
            parts = [base[i] for i in order]
            want = as_frames(B.oracle_frames(parts, level))
            hold(bc, Case("resident, level %d, %s" % (level, oname), lambda prefill, parts=parts, level=level: resident_compress(bc, H, parts, prefill, top, level),
                          lambda got, what, want=want: same(got, want, what),
                          hostile=[lambda parts=parts, level=level, k=k: resident_compress(bc, H, hostile(parts, k), CANARY, top, level) for k in ("noise", "text")],
                          group="resident", predicted=resident_bytes(len(parts), 4)), log)
    # chunks above maxSrcSize: refused in place, every other chunk's frame is oracle E's
    parts = base
    want = [(REFUSED_SRC, b"") if len(c) > BLOCK else (len(f), f) for f, c in zip(B.oracle_frames(parts, 3), parts)]
    assert sum(w == REFUSED_SRC for w, _ in want) == 3
    hold(bc, Case("resident, maxSrcSize 64 KiB under chunks of up to 200 KiB", lambda prefill: resident_compress(bc, H, parts, prefill, BLOCK, 3),
                  lambda got, what, want=want: same(got, want, what),
                  hostile=[lambda k=k: resident_compress(bc, H, hostile(parts, k), CANARY, top, 3) for k in ("noise", "text")], group="resident", predicted=resident_bytes(len(parts), 1)), log)
    # the set form over the dictionary batch: raw content, empty member, no dictionary -> oracle E; the formatted member -> oracle D with it
    parts = [c for _, c in dict_chunks()]
    raw, formatted = X.STREAM[:6000], X.TRAINED8K
    cds = [CompressionDict(bc, formatted, 3), CompressionDict(bc, raw, 3), CompressionDict(bc, b"", 3)]
    cset = CompressionDictSet(bc, cds, 3)
    index = np.array([(0, 1, 2, NO_DICT)[i % 4] for i in range(len(parts))], dtype=np.uint32)
    dics = [(formatted, raw, b"", b"")[i % 4] for i in range(len(parts))]
    stated = {i: O.compress_using_dict(c, dics[i], 3) if dics[i] else O.compress(c, 3) for i, c in enumerate(parts) if i % 4 != 0}

    def check_set(got, what):
        for i, ((w, f), c) in enumerate(zip(got, parts)):
            assert w == len(f) <= bc.L.zsmi_compressBound(len(c)), (what, i, hex(w))
            assert (O.decompress_using_dict(f, len(c), dics[i]) if dics[i] else O.decompress(f, len(c))) == c, (what, "oracle D", i)
        for i, f in stated.items():
            assert got[i] == (len(f), f), (what, "oracle E", i)
    hold(bc, Case("resident with a CDict set", lambda prefill: resident_compress(bc, H, parts, prefill, 65537, cset=cset, index=index), check_set,
                  hostile=[lambda k=k: resident_compress(bc, H, hostile(parts, k), CANARY, 65537, cset=cset, index=index[::-1].copy()) for k in ("noise", "text")],
                  group="resident", predicted=resident_bytes(len(parts), 2, True)), log)
    bc.sync(); cset.close()
    for cd in cds:
        cd.close()
    bc.close()
    return log


# ================================================================================================ family: decode
def catalogue_reference(cat, caps):
    """oracle D over the catalogue at these capacities, in the library's words: [(size, bytes) or (the error word, b"")]"""
    import _oracle as O
    out = []
    for e, cap in zip(cat, caps):
        try:
            w = O.decompress(e.frame, cap)
            out.append((len(w), w))
        except O.OracleError as x:
            out.append(((1 << 32) - x.code, b""))
    return out


def resident_decode(bc, H, frames, caps, prefill, max_cap, ddict_set=None):
    """frame sizes are not asked here: the places are the capacities, laid out by zsmi_layoutOutputsDevice -> [(word, bytes)]"""
    import _batch as B
    n = len(frames)
    src_np, so, ss = B.batch(frames)
    caps32 = np.ascontiguousarray(caps, dtype=np.uint32)
    eff = np.minimum(caps32, np.uint32(max_cap)).astype(np.uint64)
    do = B.layout(eff, [3 + 5 * (i % 4) for i in range(n)])
    room = int(do[-1]) + int(eff[-1]) + 64
    src, d_so, d_ss, d_do, d_caps = up(H, src_np), up(H, so), up(H, ss), up(H, do), up(H, caps32)
    dst, dsz = Guarded(H, room, prefill), Guarded(H, 4 * n, prefill)
    try:
        bc.decompress_resident(src.p, d_so.p, d_ss.p, n, dst.p, d_do.p, d_caps.p, max_cap, dsz.p, ddict_set=ddict_set)
        bc.sync()
        for b in (src, d_so, d_ss, d_do, d_caps):
            b.body()
        words, host = dsz.body(np.uint32), dst.body()
        out, spans = [], []
        for i in range(n):
            w, o = int(words[i]), int(do[i])
            size = w if w < B.ERR else 0
            assert size <= int(eff[i]), ("item", i, "a size above its capacity", hex(w), int(eff[i]), [hex(int(v)) for v in words[:8]])
            spans.append((o, o + int(eff[i])))                                # (a failed item's place holds what it got to: never beyond its capacity)
            out.append((w, host[o:o + size].tobytes()))
        bad = outside_untouched(host, spans, prefill)
        assert not bad, ("written outside the items' places", bad)
        return out
    finally:
        for b in (src, d_so, d_ss, d_do, d_caps, dst, dsz):
            b.free()


def family_decode(fast=True):
    """the whole edge catalogue (tests/_edge_catalogue.py) at exact and at 1 MiB capacities through the host-array call and the resident
    call, and - with the fast path - the mixed batch of tests/_ddict_set.py through a DDict set; the catalogue in reverse is the
    predecessor.  Reference: oracle D, item by item.  fast False: ZSMI_DEC_FAST=0 in the environment, the general kernel alone."""
    import _ddict_set as S, _edge_catalogue as C
    from _hip import hip_of
    from zstandard_amd import BatchCodec, DecompressionDict, DecompressionDictSet
    assert (os.environ.get("ZSMI_DEC_FAST") == "0") == (not fast)
    bc = BatchCodec(0); H = hip_of()
    log = []
    cat = C.catalogue()
    frames = [e.frame for e in cat]
    kinds = {e.expect for e in cat}
    assert "ok" in kinds and len(kinds) > 5
    for pname, caps in (("exact capacities", [e.cap for e in cat]), ("1 MiB capacities", [1 << 20] * len(cat))):
        want = catalogue_reference(cat, caps)
        assert sum(w >= (1 << 32) - 120 for w, _ in want) > 50 and sum(w < (1 << 32) - 120 for w, _ in want) > 150          # failing items matter most here
        rev = lambda: decompress_host(bc, frames[::-1], caps[::-1], CANARY)
        hold(bc, Case("catalogue, host arrays, " + pname, lambda prefill, caps=caps: decompress_host(bc, frames, caps, prefill),
                      lambda got, what, want=want: same(got, want, what), hostile=[rev], group="decode", predicted=decode_scratch_bytes(len(cat), fast)), log)
        hold(bc, Case("catalogue, resident, " + pname, lambda prefill, caps=caps: resident_decode(bc, H, frames, caps, prefill, max(caps)),
                      lambda got, what, want=want: same(got, want, what), hostile=[lambda caps=caps: resident_decode(bc, H, frames[::-1], caps[::-1], CANARY, max(caps))],
                      group="decode", predicted=decode_scratch_bytes(len(cat), fast)), log)
    # dictionary frames through a DDict set: the first four members and the raw-content dictionary for the frames that name none
    members, unnamed = S.configurations()[6]
    assert len(members) == 4 and unnamed == "raw"
    dds = {name: DecompressionDict(bc, S.dictionaries()[name]) for name in members + [unnamed]}
    dset = DecompressionDictSet(bc, [dds[m] for m in members], dds[unnamed])
    its = S.items()
    dframes, dcaps = [b"".join(it["frames"]) for it in its], [it["cap"] for it in its]
    want = [S.oracle_item(it, members, unnamed) for it in its]
    hold(bc, Case("dictionary frames, a DDict set", lambda prefill: decompress_host(bc, dframes, dcaps, prefill, ddict_set=dset),
                  lambda got, what: same(got, want, what), hostile=[lambda: decompress_host(bc, dframes[::-1], dcaps[::-1], CANARY, ddict_set=dset),
                                                                    lambda: decompress_host(bc, frames[::-1], [e.cap for e in cat][::-1], CANARY)],
                  group="decode", predicted=decode_scratch_bytes(len(its), fast)), log)
    bc.sync(); dset.close()
    for dd in dds.values():
        dd.close()
    bc.close()
    return log


# ================================================================================================ family: the one-shot pool (product library)
def family_one_shot():
    """the product library, no hook: one thread, so one pooled context, serves these calls in order - 1 MiB of noise compressed, 200 bytes
    compressed, a catalogue frame that fails midway decoded, sequences/of_rep_second decoded, a chunk compressed with a dictionary and
    then without.  Each result is oracle E's frame or oracle D's verdict; twice over, the second time behind the first."""
    import _dicts as X, _edge_catalogue as C, _oracle as O
    from zstandard_amd import _lib
    assert not _lib.DEBUG
    L = _lib.lib()
    assert not hasattr(L, "zsmi_dbg_fillScratch"), "the product library carries no hook"
    log = []
    cat = {e.id: e for e in C.catalogue()}
    # a frame that fails midway: its first block decodes, a later one is refused (the verdict is oracle D's)
    midway, rep = cat["sequences/of_rep_after_nbseq0"], cat["sequences/of_rep_second"]
    noise, small, text = _noise(1 << 20, 3), chunks()[2][1], _text()[:5000]
    dic = X.TRAINED8K

    def compress(data, level=3, dictionary=None, prefill=CANARY):
        cap = L.zsmi_compressBound(len(data))
        out = np.full(cap + 2 * PAD, prefill, dtype=np.uint8)
        src = np.frombuffer(data, dtype=np.uint8)
        dst = ctypes.c_void_p(out.ctypes.data + PAD)
        if dictionary is None:
            r = L.zsmi_compress(dst, cap, _p(src), len(data), level)
        else:
            d = np.frombuffer(dictionary, dtype=np.uint8)
            r = L.zsmi_compress_usingDict(dst, cap, _p(src), len(data), _p(d), len(d), level)
        assert not L.zsmi_isError(r), L.zsmi_getErrorName(r)
        assert (out[:PAD] == prefill).all() and (out[PAD + r:] == prefill).all(), "written outside the frame"
        return out[PAD:PAD + r].tobytes()

    def decompress(frame, cap, prefill=CANARY):
        out = np.full(cap + 2 * PAD, prefill, dtype=np.uint8)
        src = np.frombuffer(frame, dtype=np.uint8)
        r = L.zsmi_decompress(ctypes.c_void_p(out.ctypes.data + PAD), cap, _p(src), len(frame))
        assert (out[:PAD] == prefill).all() and (out[PAD + cap:] == prefill).all(), "written outside the capacity"
        if L.zsmi_isError(r):
            return (1 << 32) - L.zsmi_getErrorCode(r), b""
        assert (out[PAD + r:] == prefill).all(), "written behind the content"
        return r, out[PAD:PAD + r].tobytes()

    def oracle_d(e):
        try:
            w = O.decompress(e.frame, e.cap)
            return len(w), w
        except O.OracleError as x:
            return (1 << 32) - x.code, b""
    assert oracle_d(midway)[0] >= (1 << 32) - 120 and oracle_d(rep) == (len(rep.content), rep.content)
    t0 = time.time()
    for rnd, prefill in enumerate((CANARY, CANARY) + PREFILLS):
        what = "round %d, prefill %#x" % (rnd, prefill)
        assert compress(noise, prefill=prefill) == O.compress(noise, 3), (what, "1 MiB of noise")
        assert compress(small, prefill=prefill) == O.compress(small, 3), (what, "200 bytes behind 1 MiB of noise")
        assert decompress(midway.frame, midway.cap, prefill) == oracle_d(midway), (what, midway.id)
        assert decompress(rep.frame, rep.cap, prefill) == oracle_d(rep), (what, rep.id)
        assert compress(text, 3, dic, prefill) == O.compress_using_dict(text, dic, 3), (what, "with a dictionary")
        assert compress(text, prefill=prefill) == O.compress(text, 3), (what, "the same chunk without it")
    log.append(("one-shot calls on one pooled context, four rounds (failing frame: %s)" % midway.id, round(time.time() - t0, 3)))
    L.zsmi_shutdown()
    return log


# ================================================================================================ family: seekable archives and records
PATCHED = ("_hip", "_resident", "_seekable_resident", "_seekable_ranges", "_find", "_split", "test_gpu_read_records", "test_gpu_find_archive",
           "test_gpu_frames_index", "test_gpu_seekable_frames")


class prefilled:
    """with prefilled(H, value): the builders of the other GPU test modules (PATCHED) allocate their guarded device buffers filled with
    `value` - body and guard pads alike - and hold what the call must leave alone against `value` instead of the canary: their `Dev`
    and `CANARY` are replaced while the block runs.  The fill is waited for (Guarded says why)."""

    def __init__(self, H, value):
        import _hip
        self.value = value
        base = _hip.Dev

        class Filled(base):
            def __init__(d, H_, n, fill=b""):
                base.__init__(d, H_, n, b"")
                if value != CANARY:
                    assert H_.hipMemset(d.base, value, n + 2 * PAD) == 0
                if fill:
                    assert H_.hipMemcpy(ctypes.c_void_p(d.p), bytes(fill), len(fill), 1) == 0
                assert H_.hipDeviceSynchronize() == 0
        self.dev = Filled

    def __enter__(self):
        self.saved = []
        for name in PATCHED:
            m = sys.modules.get(name)
            for attr, new in (("Dev", self.dev), ("CANARY", self.value)):
                if m is not None and hasattr(m, attr):
                    self.saved.append((m, attr, getattr(m, attr))); setattr(m, attr, new)

    def __exit__(self, *exc):
        for m, attr, old in self.saved:
            setattr(m, attr, old)


def family_seekable():
    """the archive calls with host arrays, each against its Python statement: the fixed-size write (tests/_seekable.py: oracle E's frames and
    the table), open + a batch of ranges (slices of the source), a record archive of the caller's frame sizes written with a CDict set -
    host arrays and resident - and read back by frame number with a dictionary - host arrays and resident -, zsmi_openFramesDevice on a
    stream with skippable frames and on streams with a junk magic (tests/_frames_index.py), records by number with followers and a refused
    request (tests/test_gpu_read_records.py's yardstick), find - literal and by regular expression - in a text across tile borders and in windows of an archive
    (tests/_find.py), and zsmi_splitRecordsDevice at targetSize 0 and 4096 with one record above maxFrameSize (tests/_split.py).  The
    last six go through the builders of those modules' own tests, under prefilled()."""
    import _seekable as S, _split as SP
    import _find as FD, _findre as FR, _frames_index as FI, _seekable_ranges as SRG, _seekable_resident as SR
    import test_gpu_find_archive as TFA, test_gpu_frames_index as TFI, test_gpu_read_records as TRR
    from _hip import hip_of
    from zstandard_amd import BatchCodec
    bc = BatchCodec(0); H = hip_of(); L = bc.L
    log = []
    data = _text()[3000:3000 + 70001]
    fs = 16384
    base = [c for _, c in chunks()]
    other = lambda: compress_host(bc, hostile(base, "noise"), CANARY, 3)

    def write(content, prefill, level=3, frame=fs, checksum=True):
        bound = bc.seekable_bound(len(content), frame, checksum)
        src, dst, size = up(H, np.frombuffer(content, dtype=np.uint8)), Guarded(H, bound, prefill), Guarded(H, 8, prefill)
        try:
            bc.compress_seekable_device(src.p, len(content), dst.p, bound, size.p, level, frame, checksum)
            bc.sync()
            src.body()
            n, buf = int(size.body(np.uint64)[0]), dst.body()
            assert n <= bound, hex(n)
            assert (buf[n:] == prefill).all(), "written behind the archive's end"
            return buf[:n].tobytes()
        finally:
            for b in (src, dst, size):
                b.free()

    for level in (1, 3):
        want = S.oracle_archive(data, fs, level, True)
        hold(bc, Case("fixed-size write, level %d" % level, lambda prefill, level=level: write(data, prefill, level),
                      lambda got, what, want=want: same([(len(got), got)], [(len(want), want)], what),
                      hostile=[lambda: write(_noise(50000, 9), CANARY, 3, 4096, False), other],
                      predicted={"seek": len(data), "compress": compress_scratch_bytes(5, 1)}), log)

    arc = S.oracle_archive(data, fs, 3, True)
    n = len(data)
    ranges = [(0, n), (fs - 5, 10), (3 * fs - 1, fs + 2), (n - 7, 100), (12345, 0), (0, 1), (2 * fs, fs)]       # whole, across borders, clipped at the end, empty, one frame exactly

    def read(prefill):
        lens = [max(min(o + l, n) - o, 0) for o, l in ranges]
        do = np.concatenate([[0], np.cumsum([l + 13 for l in lens])])[:-1].astype(np.uint64) + np.uint64(7)
        room = int(do[-1]) + lens[-1] + 64
        src, dst, st = up(H, np.frombuffer(arc, dtype=np.uint8)), Guarded(H, room, prefill), Guarded(H, 4 * len(ranges), prefill)
        h = bc.open_seekable_device(src.p, len(arc))
        try:
            written, frames = h.read_ranges_device([o for o, _ in ranges], [l for _, l in ranges], dst.p, do, st.p)
            bc.sync()
            src.body()
            assert written.tolist() == lens and frames == 5, (written.tolist(), frames)
            assert not st.body(np.uint32).any(), st.body(np.uint32).tolist()
            buf, inside = dst.body(), np.zeros(room, dtype=bool)
            out = []
            for (o, _), l, d in zip(ranges, lens, do):
                out.append((l, buf[int(d):int(d) + l].tobytes())); inside[int(d):int(d) + l] = True
            assert (buf[~inside] == prefill).all(), "written outside the ranges' places"
            return out
        finally:
            bc.sync(); h.close()
            for b in (src, dst, st):
                b.free()

    want = [(max(min(o + l, n) - o, 0), data[o:o + l]) for o, l in ranges]
    hold(bc, Case("open, a batch of ranges", read, lambda got, what: same(got, want, what),
                  hostile=[lambda: write(_noise(50000, 9), CANARY, 3, 4096, False), other],
                  predicted={"seek": 5 * 8 + len(ranges) * 8, "decode": decode_scratch_bytes(5)}), log)         # (status and code words a frame, a span a range; five frames decoded)

    # a record archive: the caller's frame sizes, a CDict set whose choices oracle E states (raw content, the empty member, none)
    import _dicts as X, _oracle as O
    from zstandard_amd import CompressionDict, CompressionDictSet, DecompressionDict, NO_DICT
    raw = X.STREAM[:6000]
    stream = X.STREAM[6000:]
    rsizes = [0, 1, 255, 4096, 65535, 65537, 3000, 131073, 17, 9000]
    starts = np.concatenate([[0], np.cumsum(rsizes)])
    recs = [stream[int(starts[i]):int(starts[i + 1])] for i in range(len(rsizes))]
    cds = [CompressionDict(bc, raw, 3), CompressionDict(bc, b"", 3)]
    cset = CompressionDictSet(bc, cds, 3)
    index = np.array([(0, 1, NO_DICT)[i % 3] for i in range(len(recs))], dtype=np.uint32)
    rarc = S.archive([O.compress_using_dict(c, raw, 3) if i % 3 == 0 else O.compress(c, 3) for i, c in enumerate(recs)], recs, True)

    def write_frames(prefill, parts=recs, idx=index):
        content = b"".join(parts)
        bound = bc.seekable_frames_bound([len(c) for c in parts], True)
        src, dst, size = up(H, np.frombuffer(content, dtype=np.uint8)), Guarded(H, bound, prefill), Guarded(H, 8, prefill)
        try:
            bc.compress_seekable_frames_device(src.p, [len(c) for c in parts], dst.p, bound, size.p, 3, True, cdict_set=cset, dict_index=idx)
            bc.sync()
            src.body()
            k, buf = int(size.body(np.uint64)[0]), dst.body()
            assert k <= bound, hex(k)
            assert (buf[k:] == prefill).all(), "written behind the archive's end"
            return buf[:k].tobytes()
        finally:
            for b in (src, dst, size):
                b.free()
    hold(bc, Case("record archive write, a CDict set", write_frames, lambda got, what: same([(len(got), got)], [(len(rarc), rarc)], what),
                  hostile=[lambda: write_frames(CANARY, hostile(recs, "noise"), index[::-1].copy()), other],
                  predicted={"seek": len(b"".join(recs)), "compress": compress_scratch_bytes(blocks_of(recs), 3)}), log)

    dd = DecompressionDict(bc, raw)
    picks = [5, 0, 9, 9, 3, 7, 1, 4, 2, 8, 6, 0]

    def read_frames(prefill):
        lens = [len(recs[i]) for i in picks]
        do = np.concatenate([[0], np.cumsum([l + 9 for l in lens])])[:-1].astype(np.uint64) + np.uint64(3)
        room = int(do[-1]) + lens[-1] + 64
        src, dst, st = up(H, np.frombuffer(rarc, dtype=np.uint8)), Guarded(H, room, prefill), Guarded(H, 4 * len(picks), prefill)
        h = bc.open_seekable_device(src.p, len(rarc), ddict=dd)
        try:
            written, frames = h.read_frames_device(picks, dst.p, do, st.p)
            bc.sync()
            src.body()
            assert written.tolist() == lens and frames == len({i for i in picks if recs[i]}), (written.tolist(), frames)      # (a frame without content is not decoded)
            assert not st.body(np.uint32).any(), st.body(np.uint32).tolist()
            buf = dst.body()
            bad = outside_untouched(buf, [(int(d), int(d) + l) for d, l in zip(do, lens)], prefill)
            assert not bad, ("written outside the records' places", bad)
            return [(l, buf[int(d):int(d) + l].tobytes()) for d, l in zip(do, lens)]
        finally:
            bc.sync(); h.close()
            for b in (src, dst, st):
                b.free()
    hold(bc, Case("records by frame number, a dictionary", read_frames, lambda got, what: same(got, [(len(recs[i]), recs[i]) for i in picks], what),
                  hostile=[lambda: write_frames(CANARY, hostile(recs, "noise"), index[::-1].copy()), other],
                  predicted={"seek": 9 * 8 + len(picks) * 8, "decode": decode_scratch_bytes(9)}), log)

    # ---- the same archive with every descriptor in device memory: the resident write, frames by number resident
    from zstandard_amd import DecompressionDictSet
    dset = DecompressionDictSet(bc, [], unnamed=dd)
    content = b"".join(recs)

    def write_resident(prefill, parts=recs, idx=index):
        with prefilled(H, prefill):
            w = SR.write(L, H, bc, b"".join(parts), [len(c) for c in parts], 3, 1, cset, idx)
        assert w.rc == 0 and w.archive is not None, (w.rc, hex(w.word))
        return w.archive
    plan = resident_bytes(len(recs), 3, True)
    hold(bc, Case("record archive write, resident, a CDict set", write_resident, lambda got, what: same([(len(got), got)], [(len(rarc), rarc)], what),
                  hostile=[lambda: write_resident(CANARY, hostile(recs, "noise"), index[::-1].copy()), other],
                  predicted=dict(plan, seek=len(content) + (5 * len(recs) + 4) * 8 + 12 * len(recs))), log)

    def open_host(arc, ds=None):
        err = ctypes.c_int(-1)
        sk = L.zsmi_openSeekable_usingDDictSet(bc.ctx, arc, len(arc), ds.handle if ds is not None else None, ctypes.byref(err))
        assert sk and err.value == 0, err.value
        return sk

    def read_resident(prefill):
        lens = [len(recs[i]) for i in picks]
        want_off = SR.rounded_offsets(lens, 16)
        sk = open_host(rarc, dset)
        try:
            with prefilled(H, prefill):
                r = SR.read(L, H, bc, sk, picks, 16, int(want_off[-1]))
            assert r.rc == 0 and not r.status.any() and (r.offsets == want_off).all(), (r.rc, r.status.tolist())
            bad = outside_untouched(r.buf, [(int(o), int(o) + l) for o, l in zip(want_off, lens)], prefill)
            assert not bad, ("written outside the records' places", bad)
            return [(int(w), r.out(k, int(w))) for k, w in enumerate(r.written)]
        finally:
            bc.sync(); L.zsmi_closeSeekable(sk)
    hold(bc, Case("records by frame number, resident", read_resident, lambda got, what: same(got, [(len(recs[i]), recs[i]) for i in picks], what),
                  hostile=[lambda: write_resident(CANARY, hostile(recs, "noise"), index[::-1].copy()), other],
                  predicted={"seek": 9 * 8 + len(picks) * 8, "decode": decode_scratch_bytes(9)}), log)

    # ---- zsmi_openFramesDevice: a stream with skippable frames and false magic numbers; streams with a junk magic are refused with their code
    good, gparts = FI.good_stream(), FI.good_parts()
    gcontent = b"".join(c for _, c in gparts)
    want_rows, code0 = FI.index(L, good)
    bad_streams = {k: v for k, v in FI.bad_streams().items() if k in ("wrong_magic_third_frame", "junk_5_behind", "junk_3_behind", "not_a_frame_at_0")}
    assert code0 == 0 and len(want_rows) == len(gparts) and sum(1 for f, c in gparts if f[:4] != good[:4]) == 2 and len(bad_streams) == 4
    assert [d for _, _, d in want_rows] == [len(c) for _, c in gparts] and [c for _, c, _ in want_rows] == [len(f) for f, _ in gparts]

    def open_frames(prefill):
        out = {}
        with prefilled(H, prefill):
            from _hip import Dev
            for name, stream in sorted(bad_streams.items()):
                dev = Dev(H, len(stream), stream)
                sk, e = TFI.open_device(L, bc, dev.p, len(stream))
                bc.sync(); dev.free()
                assert not sk, name
                out[name] = e
            dev = Dev(H, len(good), good)
            sk, e = TFI.open_device(L, bc, dev.p, len(good))
            try:
                assert sk and e == 0, e
                out["table"] = TFI.table_of(L, sk)
                b = SRG.read_ranges(L, H, bc, sk, [(0, len(gcontent)), (len(gparts[0][1]) + 1, 250)], len(gcontent))
                assert b.rc == 0 and b.status == [0, 0], (b.rc, b.status)
                out["content"] = b.out
                raw = np.frombuffer(dev.all(), dtype=np.uint8)
                assert (raw[:PAD] == prefill).all() and (raw[PAD + len(good):] == prefill).all() and raw[PAD:PAD + len(good)].tobytes() == good, "the stream changed"
            finally:
                bc.sync(); L.zsmi_closeSeekable(sk); dev.free()
        return out

    def check_frames(got, what):
        assert got["table"] == want_rows, (what, "the frame index")
        assert got["content"] == [gcontent, gcontent[len(gparts[0][1]) + 1:][:250]], (what, "the content read through the index")
        for name, stream in bad_streams.items():
            assert got[name] == FI.index(L, stream)[1] != 0, (what, name, got[name])
    m = len(gparts)
    hold(bc, Case("open a stream of frames on the device", open_frames, check_frames, hostile=[lambda: write(_noise(50000, 9), CANARY, 3, 4096, False), other],
                  predicted={"seek": (2 * m + 1) * 8 + m * 8 * 4, "decode": decode_scratch_bytes(m - 3)}), log)          # (positions and slots, eight words a candidate; every frame with content decoded)

    # ---- records by number: three frames, followers of a leader, a request nobody can serve
    text3 = TRR.Text(SP.lines(31, 90, 120), 10, 2048, 4096)
    assert text3.split.n == 3
    parts3 = [text3.data[text3.at[i]:text3.at[i + 1]] for i in range(3)]
    arc3 = S.archive([O.compress(c, 3) for c in parts3], parts3, True)
    nrec = text3.split.records
    ridx = [5, 6, 7, nrec + 3, 0, nrec - 1, nrec - 2, 40, 5]
    want3 = TRR.expect(text3, ridx)
    assert want3.status.count(TRR.E_FRAME_INDEX) == 1 and len(want3.leaders) < len(ridx) - 1 and want3.result[0] == len(ridx) - 1      # one refused (frameIndex_tooLarge), followers

    def read_records(prefill):
        sk = open_host(arc3)
        try:
            with prefilled(H, prefill):
                g, w = TRR.roomy(L, H, bc, sk, text3, ridx, what="records by number")       # (checks bytes, words and everything around them itself)
                # and with five read slots to spare: the list's entries behind the planned reads must name no frame
                spare = w.result[1] + 5
                g2 = TRR.call(L, H, bc, sk, text3.split.first_record, text3.split.n, 10, ridx, spare, 1, L.zsmi_seekableRecordsWorkBound(sk, spare), w.result[3])
                TRR.check(g2, w, text3, ridx, "records by number, read slots to spare")
            return g.status, g.written, g.result, [int(v) for v in g.offsets]
        finally:
            bc.sync(); L.zsmi_closeSeekable(sk)
    hold(bc, Case("records by number, followers and a refused request", read_records,
                  lambda got, what: same([(0, repr(got).encode())], [(0, repr((want3.status, want3.written, want3.result, [int(v) for v in want3.offsets])).encode())], what),
                  hostile=[lambda: write_resident(CANARY, hostile(recs, "noise"), index[::-1].copy()), other],
                  predicted={"seek": (6 * len(ridx) + 3 + 2 * want3.result[1] + 1) * 8, "decode": decode_scratch_bytes(1)}), log)

    # ---- find: a text with occurrences across the borders of a lane's 16 bytes, a step and a tile; windows of an archive
    pat = FD.pattern_of(17)
    size = 3 * FD.TILE + 100
    fstarts = [40, FD.STEP - 3, FD.TILE - 5, FD.TILE + 16 + 7, 2 * FD.TILE - 17, 2 * FD.TILE, size - 17]
    ftext = FD.place(size, pat, fstarts, delims=[7, FD.STEP + 100, FD.TILE - 40, FD.TILE + 60, 2 * FD.TILE - 40, 2 * FD.TILE + 40, size - 30])
    frecords, fmatches = FD.find(ftext, pat, 10, 1000)
    assert fmatches == len(fstarts) and len(frecords) == 4

    def find_text(prefill):
        with prefilled(H, prefill):
            d = FD.device(L, H, bc, ftext, pat, 10, base=1000, capacity=len(frecords) + 3)
        assert d.rc == 0, d.rc
        assert all(v == int.from_bytes(bytes([prefill]) * 8, "little") for v in d.records[len(frecords):]), "written behind the numbers"
        return d.result, d.records[:len(frecords)]
    tiles = (size + FD.TILE - 1) // FD.TILE
    hold(bc, Case("find in a text across tile borders", find_text,
                  lambda got, what: same([(0, repr(got).encode())], [(0, repr(([len(frecords), len(frecords), fmatches, size], frecords)).encode())], what),
                  hostile=[lambda: write(_noise(50000, 9), CANARY, 3, 4096, False), other], predicted={"seek": 3 * (tiles + 1) * 8 + 16 * tiles}), log)

    # the regular-expression search over the same text: an occurrence of 17 bytes across the border of the first two tiles, the last
    # record - listed - without a delimiter; behind the tiles' words, 16-aligned, 72 bytes a tile more (OUT functions, HEADMASKs)
    rx = b"![0-Z]{16}"                                                    # ('!' and 16 of the pattern's other bytes: 18 states)
    rrecords, rtext = FR.find(ftext, rx, 0, 10, 1000)
    assert len(rrecords) == 4 and rrecords[-1] == 1000 + rtext - 1 and ftext[-1] != 10 and ftext[FD.TILE - 5] == 0x21
    rprog = FR.program(L, rx)

    def find_regex_text(prefill):
        with prefilled(H, prefill):
            d = FR.device(L, H, bc, ftext, rprog, len(rrecords), base=1000, capacity=len(rrecords) + 3)
        assert d.rc == 0, d.rc
        assert all(v == int.from_bytes(bytes([prefill]) * 8, "little") for v in d.records[len(rrecords):]), "written behind the numbers"
        return d.result, d.records[:len(rrecords)]
    hold(bc, Case("find by regular expression in a text across tile borders", find_regex_text,
                  lambda got, what: same([(0, repr(got).encode())], [(0, repr(([len(rrecords), len(rrecords), rtext, size], rrecords)).encode())], what),
                  hostile=[lambda: write(_noise(50000, 9), CANARY, 3, 4096, False), other],
                  predicted={"seek": (3 * (tiles + 1) * 8 + 16 * tiles + 15) // 16 * 16 + 72 * tiles}), log)

    wdata, wdelim, wT, wM = SP.cases()["cut_record_shares_its_last_piece"]
    wsplit = SP.Split(wdata, wdelim, wT, wM)
    wat = [0] + np.cumsum(wsplit.sizes, dtype=np.int64).tolist()
    warc = S.archive([O.compress(wdata[wat[i]:wat[i + 1]], 3) for i in range(wsplit.n)], [wdata[wat[i]:wat[i + 1]] for i in range(wsplit.n)], True)
    f1, f2 = wsplit.frame_of(1), wsplit.frame_of(2)
    windows = [(b"y" * 12, 0, wsplit.n), (b"y" * 24, 0, wsplit.n), (b"y" * 24, f1, f2), (b"y" * 12, f1 + 1, f2 + 1), (b"tail", wsplit.n - 1, wsplit.n), (b"z", 1, wsplit.n)]

    def find_windows(prefill):
        with prefilled(H, prefill):
            o = TFA.Opened(L, H, bc, wdata, wdelim, wT, wM, arc=warc)
            try:
                return [o.find(p_, a, b)[:3] for p_, a, b in windows]
            finally:
                o.close()

    def check_windows(got, what):
        for (p_, a, b), (rc, result, numbers) in zip(windows, got):
            records, matches = FD.window(wdata, wsplit.sizes, wsplit.first_record, a, b, p_, wdelim)
            assert rc == 0 and result == [len(records), len(records), matches, wat[b] - wat[a]] and numbers == records, (what, p_, a, b, rc, result, numbers, records)
        assert got[2][2] == [] and got[3][1][2] == 3                       # (an occurrence across the window's border is not found; a window that begins inside a record)
    hold(bc, Case("find in windows of an archive", find_windows, check_windows, hostile=[lambda: write_resident(CANARY, hostile(recs, "noise"), index[::-1].copy()), other],
                  predicted={"seek": 3 * 2 * 8 + 16, "decode": decode_scratch_bytes(wsplit.n)}), log)
    bc.sync(); dset.close(); dd.close(); cset.close()
    for cd in cds:
        cd.close()

    M = 1 << 16
    text = SP.lines(31, n=400, hi=300) + b"x" * (M + 4464) + b"\n" + SP.lines(32, n=300, hi=200) + b"tail without a delimiter"
    for T in (0, 4096):
        def split(prefill, T=T):
            want = SP.Split(text, 10, T, M)
            mp = want.pieces
            src = up(H, np.frombuffer(text, dtype=np.uint8))
            fsz, fr, res = Guarded(H, 4 * mp, prefill), Guarded(H, 8 * (mp + 1), prefill), Guarded(H, 24, prefill)
            try:
                bc.split_records_device(src.p, len(text), mp, fsz.p, fr.p, res.p, b"\n", T, M)
                bc.sync()
                src.body()
                result = [int(v) for v in res.body(np.uint64)]
                k = result[0]
                sizes, first = fsz.body(np.uint32), fr.body(np.uint64)
                assert k <= mp and (sizes[k:].view(np.uint8) == prefill).all() and (first[k + 1:].view(np.uint8) == prefill).all(), "written behind the lists"
                return result, sizes[:k].tolist(), first[:k + 1].tolist()
            finally:
                for b in (src, fsz, fr, res):
                    b.free()

        def check(got, what, T=T):
            want = SP.Split(text, 10, T, M)
            assert want.pieces > want.records > 700                                            # (the long record is cut: more pieces than records)
            assert got == ([want.n, want.records, want.pieces], want.sizes, want.first_record), (what, got[0], [want.n, want.records, want.pieces])
        hold(bc, Case("split records on the device, targetSize %d" % T, split, check,
                      hostile=[lambda: write(_noise(50000, 9), CANARY, 3, 4096, False), other],
                      predicted={"seek": (3 * SP.Split(text, 10, T, M).pieces + 1) * 8 + 16 * SP.Split(text, 10, T, M).pieces}), log)      # (split.hip's words a piece)
    bc.close()
    return log


# ================================================================================================ family: dictionary training
def family_training():
    """zsmi_trainFromDevice on the context: the `short_samples` case of tests/test_gpu_dict_train.py::test_content_equals_model.  The
    dictionary's CONTENT is held against the scalar model (tests/c/train_model.c) byte for byte in every run, and the whole DICTIONARY -
    the header with the entropy tables the finalize step counts from the samples compressed with that content - against the reference of a
    training call (tests/_train.py: reference_train, which finalizes with the oracle's scalar zso_finalizeDictionary), byte for byte in
    every run: a dependence on scratch that showed on fresh scratch already would fail it too."""
    import _batch as B, _train as T
    import test_gpu_dict_train as TD
    from _hip import hip_of
    from zstandard_amd import BatchCodec, _lib
    bc = BatchCodec(0); H = hip_of(); L = bc.L
    log = []
    name, make, cap, k, d, f = next(c for c in TD.CASES if c[0] == "short_samples")
    parts = make()
    want = T.model_content(parts, cap, k, d, f)
    other = T.samples("json_records", 1 << 18)
    ref = T.reference_train(parts, cap, k, d, f, 0, 1.0, 3)[0]

    def train(samples, prefill, cap, k, d, f):
        src_np, so, ss = B.batch(samples)
        src = up(H, src_np)
        out = np.full(cap + 2 * PAD, prefill, dtype=np.uint8)
        p = _lib.FastCoverParams(k=k, d=d, f=f, steps=0, accel=0, splitPoint=1.0, level=0, dictID=0)
        size = ctypes.c_size_t(0)
        try:
            rc = L.zsmi_trainFromDevice(bc.ctx, ctypes.c_void_p(src.p), _p(so), _p(ss), len(ss), ctypes.c_void_p(out.ctypes.data + PAD), cap, ctypes.byref(p), ctypes.byref(size))
            assert rc == 0, rc
            src.body()
        finally:
            src.free()
        assert (out[:PAD] == prefill).all() and (out[PAD + cap:] == prefill).all(), "written outside the dictionary's capacity"
        assert (p.k, p.d) == (k, d)
        return out[PAD:PAD + size.value].tobytes()

    def check(dic, what):
        content = TD.check_format(dic, cap)
        assert len(want) >= len(content) and want.endswith(content), (what, "the content is the scalar model's", len(want), len(content))
        assert len(content) == min(len(want), cap - (len(dic) - len(content))), what
        assert dic == ref, (what, "the dictionary differs from the reference's at", B.first_difference(dic, ref))

    hold(bc, Case("trainFromDevice, short samples", lambda prefill: train(parts, prefill, cap, k, d, f), check,
                  hostile=[lambda: train(other, CANARY, 65536, 200, 8, 20), lambda: compress_host(bc, [c for _, c in chunks()], CANARY, 3)],
                  group="train", predicted=sum(map(len, parts))), log)
    bc.close()
    return log


FAMILIES = {
    "compress": lambda: family_compress(),
    "compress_sub_batches": lambda: family_compress(64),
    "compress_dict": family_compress_dict,
    "resident": family_resident,
    "decode": lambda: family_decode(True),
    "decode_general": lambda: family_decode(False),
    "seekable": family_seekable,
    "training": family_training,
    "one_shot": family_one_shot,
}
# what a family's child is started with besides ZSMI_DEBUG_LIB=1 (one_shot: the product library)
ENVIRONMENT = {"compress_sub_batches": {"ZSMI_BLOCKS_IN_FLIGHT": "64"}, "decode_general": {"ZSMI_DEC_FAST": "0"}}


def main(family):
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
    from zstandard_amd import _lib
    if _lib.built_fingerprint() != _lib.source_fingerprint():
        _lib.build()
    t0 = time.time()
    log = FAMILIES[family]()
    print(json.dumps({"family": family, "seconds": round(time.time() - t0, 2), "cases": log}))
    print("CHILD-OK")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
