"""Inputs that sit on the borders of the host and plan code (test infrastructure): the item counts at which k_plan_chunks starts its second
tile, the offset scan takes its second level and a call starts its second launch, and the stream positions at which a magic number
straddles a lane, step or tile of the index kernels.  The borders are literals here; tests/test_borders_host.py reads the constants they
come from out of the source text and fails when one of them moved.  tests/test_gpu_borders.py runs the inputs on the GPU; the child
processes of its sub-batch tests are plan_child() below."""
import os, re, struct
import numpy as np
import _batch as B, _dicts as X, _framewriter as W, _oracle as O, _resident_compress as RC, _resident_cdict_set as RS

KIB = 1 << 10
PLAN_TILE = 1024                 # ZS_PLAN_THREADS (plan_kernels.hip): the chunks k_plan_chunks plans a turn
SCAN_TILE = 2048                 # ZS_SCAN_TILE (entropy_kernels.hip): the items of one tile sum
SCAN_THREADS = 1024              # dim3(1024) of the k_pack_scan_tiles launch (zsmi_api.hip): tile sums a thread = ceil(tiles / 1024)
INDEX_TILE = 16384               # ZS_INDEX_TILE (seekable.hip): 4 steps of 4096 bytes, a lane 16 bytes
INDEX_STEP, INDEX_LANE = 4096, 16
ITEMS_IN_FLIGHT = 65536          # maxItemsInFlight (zsmi_ctx.h): the items of one decode launch
BLOCKS_IN_FLIGHT = 16384         # maxBlocksInFlight (zsmi_ctx.h): the blocks of one compress sub-batch
SCAN_LEVEL = SCAN_THREADS * SCAN_TILE                      # 2 097 152 items: up to here a thread of k_pack_scan_tiles has one tile sum
NO_DICT = RS.NO_DICT
CSRC = os.path.join(B.ROOT, "zstandard_amd", "csrc")


def source_constants():
    """the six numbers above as the source text states them"""
    def find(name, pattern):
        m = re.search(pattern, open(os.path.join(CSRC, name)).read())
        assert m, (name, pattern)
        return int(m.group(1))
    return {"PLAN_TILE": find("plan_kernels.hip", r"#define ZS_PLAN_THREADS (\d+)u"),
            "SCAN_TILE": find("entropy_kernels.hip", r"#define ZS_SCAN_TILE (\d+)u"),
            "SCAN_THREADS": find("zsmi_api.hip", r"k_pack_scan_tiles, dim3\(1\), dim3\((\d+)\)"),
            "INDEX_TILE": find("seekable.hip", r"#define ZS_INDEX_TILE (\d+)u"),
            "ITEMS_IN_FLIGHT": find("zsmi_ctx.h", r"uint32_t maxItemsInFlight = (\d+);"),
            "BLOCKS_IN_FLIGHT": find("zsmi_ctx.h", r"uint32_t maxBlocksInFlight = (\d+);")}


def counts(size):
    """(blocks, small units, big units) of a chunk: zs_chunk_counts (zsmi_plan.h)"""
    blocks = (size + 65535) // 65536 if size else 1
    units = (size + 131071) // 131072
    small = 1 if size and size - (units - 1) * 131072 <= 65536 else 0
    return blocks, small, units - small


def _cut(data, sizes, rng):
    return [data[at:at + s] for at, s in ((int(rng.integers(0, len(data) - s)), int(s)) for s in sizes)]


# ------------------------------------------------------------------ A. the device-built plan over more than one tile of chunks
TOLD = 300                       # the smaller maxSrcSize of the second call: the chunks above it are refused in place
TINY_N = (PLAN_TILE, PLAN_TILE + 1, 2 * PLAN_TILE + 1)     # K = n: exactly one tile, a tile and one chunk, two tiles and one chunk
# around both tile borders: an empty chunk, zeros, a chunk above TOLD - the last thread of a tile (1023, 2047) and the first of the next
# (1024, 2048) carry no unit in one of the two calls
_TINY_SPECIAL = {1022: "zeros", 1023: "empty", 1024: "above", 1025: "zeros", 1026: "empty", 2046: "zeros", 2047: "above", 2048: "empty", 2049: "zeros"}


def tiny_chunks(n):
    """n chunks of 0 .. 400 bytes cut from the stream, seeded; the special ones where n reaches them"""
    rng = np.random.default_rng(n)
    chunks = _cut(RC.stream_bytes(), rng.integers(0, 401, n), rng)
    for i, kind in _TINY_SPECIAL.items():
        if i < n:
            chunks[i] = b"" if kind == "empty" else bytes(200 + i % 7) if kind == "zeros" else RC.stream_bytes()[3 * i:3 * i + 400]
    return chunks


UNEVEN_N, UNEVEN_IN_FLIGHT, UNEVEN_MAX = 2500, 4400, 200 * KIB   # nbMax = 4: sub-batches of K = 1100 chunks - 1100, 1100 and 300
UNEVEN_K = UNEVEN_IN_FLIGHT // 4
LONG = (65536, 65537, 131072, 131073, 200 * KIB)                 # one block; a big unit; a big unit; a big and a small unit; two big units
# on both sides of the tile border of the first two sub-batches (1024, 1100 + 1024) and of the first sub-batch border (1100)
_UNEVEN_AT = {1023: 65537, 1024: 131073, 1099: 200 * KIB, 1100: 131072, 2123: 131073, 2124: 200 * KIB}


def uneven_sizes():
    rng = np.random.default_rng(2500)
    sizes = [int(v) for v in rng.integers(0, 401, UNEVEN_N)]
    for k, i in enumerate(range(7, UNEVEN_N, 60)):
        sizes[i] = LONG[k % len(LONG)]
    for i, s in _UNEVEN_AT.items():
        sizes[i] = s
    return sizes


def uneven_chunks():
    return _cut(RC.stream_bytes(), uneven_sizes(), np.random.default_rng(2501))


# the set of three: a formatted member, raw content, an empty one.  A chunk's index cycles through them, NO_DICT and one beyond the set,
# so any five neighbours - those around a tile border too - hold one of each kind
SET3 = (X.TRAINED8K, X.STREAM[:6000], b"")
BEYOND = len(SET3)
CYCLE = (0, 1, 2, NO_DICT, BEYOND)


def with_choices(chunks):
    """[(chunk, choice)]: choice i % 5 of CYCLE; a short chunk that picks a member with bytes is cut from the member's content instead, so
    that its frame depends on the record its unit was given"""
    rng = np.random.default_rng(len(chunks))
    items = []
    for i, c in enumerate(chunks):
        ch = CYCLE[i % len(CYCLE)]
        if ch in (0, 1) and 0 < len(c) <= 400:
            cont = X.content_of(SET3[0]) if ch == 0 else SET3[1]
            at = int(rng.integers(0, len(cont) - len(c)))
            c = cont[at:at + len(c)]
        items.append((c, ch))
    return items


def make_set3(codec):
    from zstandard_amd import CompressionDict, CompressionDictSet
    cds = [CompressionDict(codec, d, 3) for d in SET3]
    return CompressionDictSet(codec, cds, 3), cds


def assert_set_call(batch, cset, max_src, what):
    """the resident set call at max_src against the host-array set call (which takes NO_DICT where the resident call is to refuse the
    index), and oracle E where it can state the frame: no dictionary, the empty member, the raw content"""
    accepted = np.where(batch.index == BEYOND, NO_DICT, batch.index).astype(np.uint32)
    ref = batch.run_set(False, cset, index=accepted)
    got = batch.run_set(True, cset, max_src)
    refused = {i: RS.SIZE_REFUSED if int(s) > max_src else RS.INDEX_REFUSED for i, (s, ch) in enumerate(zip(batch.ss, batch.index))
               if int(s) > max_src or ch == BEYOND}
    RS.assert_equal_with_refusals(batch, ref, got, refused, what)
    assert int((got[0] >= B.ERR).sum()) == len(refused) and (ref[0] < B.ERR).all()
    frames = batch.frames(*got)
    for choices, dic in (((2, NO_DICT), b""), ((1,), SET3[1])):
        at = [i for i in range(batch.n) if int(batch.index[i]) in choices and i not in refused]
        for i, e in zip(at, B.oracle_frames([batch.chunks[i] for i in at], 3, dic)):
            assert frames[i] == e, (what, "oracle E", i, len(batch.chunks[i]), int(batch.index[i]))
    return ref, got


def plan_child(form):
    """run in a process of its own with ZSMI_BLOCKS_IN_FLIGHT=4400: the uneven batch, plain or with the set of three"""
    from _hip import hip_of
    from zstandard_amd import BatchCodec
    bc = BatchCodec(0); H = hip_of()
    chunks = uneven_chunks()
    what = f"sub-batches of {UNEVEN_K} chunks, {form}"
    if form == "plain":
        batch = RC.Batch(bc, H, chunks)
        ref = batch.run(False)
        got = batch.run(True, UNEVEN_MAX)
        RC.assert_equal_to_host_call(batch, ref, got, UNEVEN_MAX, what)
        assert (ref[0] < B.ERR).all()
        for i, (f, e) in enumerate(zip(batch.frames(*got), B.oracle_frames(chunks, 3))):
            assert f == e, (what, "oracle E", i, len(chunks[i]))
    else:
        cset, cds = make_set3(bc)
        batch = RS.Batch(bc, H, with_choices(chunks))
        assert_set_call(batch, cset, UNEVEN_MAX, what)
        bc.sync(); cset.close()
        for cd in cds:
            cd.close()
    batch.free(); bc.close()
    print("CHILD-OK")


RECORDS_N = 3000                 # one sub-batch of three tiles: 1024, 1024 and 952 records


def records():
    """(parts, choices): 3000 records of 1 .. 300 bytes, their choices dealt over the set of three and NO_DICT"""
    rng = np.random.default_rng(3000)
    items = with_choices(_cut(RC.stream_bytes(), rng.integers(1, 301, RECORDS_N), rng))
    picks = (0, 1, 2, NO_DICT)
    return [c for c, _ in items], np.array([picks[i % 4] for i in range(RECORDS_N)], dtype=np.uint32)


# ------------------------------------------------------------------ C.1 compress: the cut at the default blocks in flight
CUT_N, CUT_LONG = 16500, 131073                            # the long chunk: three blocks
CUT_AT = BLOCKS_IN_FLIGHT - 1                              # every chunk in front of it is one block: its blocks are 16 383 .. 16 385
_cut_chunks = []


def cut_chunks():
    if not _cut_chunks:
        rng = np.random.default_rng(16500)
        sizes = rng.integers(64, 701, CUT_N)
        sizes[CUT_AT] = CUT_LONG
        _cut_chunks.extend(_cut(RC.stream_bytes(), sizes, rng))
    return _cut_chunks


# ------------------------------------------------------------------ C.2 decode: the second launch at the default items in flight
DECODE_N, DAMAGE_EVERY = 66000, 499
DECODE_BORDER = (ITEMS_IN_FLIGHT - 1, ITEMS_IN_FLIGHT, ITEMS_IN_FLIGHT + 1)   # a damaged frame, a frame and a skippable frame, a valid frame
_decode = {}


def damaged(i):
    return i % DAMAGE_EVERY == 0 or i == DECODE_BORDER[0]


def _damage(frame):
    b = bytearray(frame); b[len(b) // 2] ^= 0x5A
    return bytes(b)


def decode_items(dic=b""):
    """(items, contents, want): 66 000 frames of 20 .. 120 content bytes - oracle E's and raw-block frames in turn, some with checksums
    (with a dictionary: oracle E's alone) - every 499th damaged in its middle, and oracle D's answer to each at the capacity of its
    content: (size or error word, bytes)"""
    if dic not in _decode:
        import _frames_index as F
        rng = np.random.default_rng(66000)
        data = X.content_of(dic) * 4 if dic else F._text(1 << 20, 0x31)
        sizes = rng.integers(20, 121, DECODE_N)
        contents = _cut(data, sizes, rng)
        if dic:
            items = B.oracle_frames(contents, 3, dic)
        else:
            items = [O.compress(c, 3) if i & 1 else W.frame([W.raw(c)], checksum=bool(i & 2))[0] for i, c in enumerate(contents)]
            items[DECODE_BORDER[1]] += W.skippable(b"behind the frame", nibble=5)
        want = []
        for i, c in enumerate(contents):
            if damaged(i):
                items[i] = _damage(items[i])
            try:
                out = O.decompress_using_dict(items[i], len(c), dic) if dic else O.decompress(items[i], len(c))
                want.append((len(out), out))
            except O.OracleError as e:
                want.append(((1 << 32) - e.code, b""))
        _decode[dic] = (items, contents, want)
    return _decode[dic]


def assert_decode_condition(items, contents, want):
    """what the input must be for the test to mean something: oracle D rejects at least 30 damaged frames and accepts every other"""
    rejected = [i for i, (sz, _) in enumerate(want) if sz >= B.ERR]
    assert all(damaged(i) for i in rejected), [i for i in rejected if not damaged(i)][:5]
    assert len(rejected) >= 30, len(rejected)
    assert all(want[i] == (len(c), c) for i, c in enumerate(contents) if not damaged(i))
    assert damaged(DECODE_BORDER[0]) and not damaged(DECODE_BORDER[1]) and not damaged(DECODE_BORDER[2])


# ------------------------------------------------------------------ D. magic numbers on every border of the index kernels
ZSTD_MAGIC, SKIP_MAGIC = 0xFD2FB528, 0x184D2A50
# (border, m): a frame starts at border * m - d for d = 0 .. 4, its magic number's four bytes across the border in every way.  The 4096
# cases are no multiples of 16 384, the 16 cases none of 4096
BORDER_M = {INDEX_TILE: (1, 2, 3, 4, 5), INDEX_STEP: (7, 6, 11, 13, 18), INDEX_LANE: (100, 700, 1500, 2301, 3400)}
TARGETS = sorted(b * m - d for b, ms in BORDER_M.items() for d, m in enumerate(ms))
# in the last whole tile (the byte-wise path when the stream ends within 4 bytes of its end) and across its two borders
TAIL_TARGETS = [11 * INDEX_TILE - 1, 11 * INDEX_TILE + 16 * 300 - 1, 11 * INDEX_TILE + 2 * INDEX_STEP - 2, 12 * INDEX_TILE - 2]
SMALL_TARGETS = [16 * 100 - 1, INDEX_STEP - 2, 2 * INDEX_STEP - 1, 16 * 700 - 3, 3 * INDEX_STEP - 4]
# name -> (total size, the frame starts aimed at)
STREAMS = {f"mod_{r}": (12 * INDEX_TILE + r, TARGETS + TAIL_TARGETS) for r in (0, 1, 3, 4, 5, INDEX_TILE - 1)}
STREAMS["ends_with_3_magic_bytes"] = (12 * INDEX_TILE + 777, TARGETS + TAIL_TARGETS)
STREAMS["one_tile"] = (INDEX_TILE, SMALL_TARGETS)


def _false_magics(payload_at, size, rng, inner=b""):
    """a skippable frame's payload of `size` bytes that starts at absolute offset payload_at: seeded bytes, and false magic numbers of
    both kinds across the lane, step and tile borders it covers; `inner`: a whole valid frame, one byte in front of a lane border"""
    p = bytearray(rng.integers(0, 200, size, dtype=np.uint8).tobytes())        # (no byte of a magic number's upper half by chance)
    end = payload_at + size
    spots = {INDEX_TILE * m - m % 5 for m in range(payload_at // INDEX_TILE, end // INDEX_TILE + 2)}
    spots |= {INDEX_STEP * m - m % 5 for m in range(payload_at // INDEX_STEP, end // INDEX_STEP + 2) if m % 4}
    spots |= {INDEX_LANE * m - (m % 5) for m in range(payload_at // 16 + 1, end // 16, 13)}
    free = payload_at
    if inner and size > len(inner) + 32:
        at = (payload_at // 16 + 2) * 16 - 1
        p[at - payload_at:at - payload_at + len(inner)] = inner
        free = at + len(inner)
    for k, q in enumerate(sorted(spots)):
        if q >= free and q + 4 <= end:
            p[q - payload_at:q - payload_at + 4] = struct.pack("<I", ZSTD_MAGIC if k & 1 else SKIP_MAGIC + k % 16)
            free = q + 4
    return bytes(p)


_streams = {}


def index_stream(name):
    """-> (stream, entries [(pos, cSize, dSize)], {pos: content} of the frames that are not skippable).  A skippable frame in front of
    every aimed frame puts it where it belongs; the last one, or the last frame itself, ends the stream at its total size"""
    if name in _streams:
        return _streams[name]
    import _frames_index as F
    total, targets = STREAMS[name]
    rng = np.random.default_rng(total)
    text = F._text(1 << 16, 0x41)
    inner = W.frame([W.raw(b"a whole valid frame")])[0]
    out, entries, contents = bytearray(), [], {}

    def fill(upto, tail=b""):
        gap = upto - len(out)
        if gap == 0:
            return
        assert gap >= 8, (name, len(out), upto)
        payload = _false_magics(len(out) + 8, gap - 8 - len(tail), rng, inner if not entries else b"") + tail
        entries.append((len(out), gap, 0))
        out.extend(W.skippable(payload, nibble=len(entries) % 16))
    for k, t in enumerate(t for t in targets if t + 300 <= total):          # (room for the frame and a skippable frame behind it)
        fill(t)
        size = 20 + 37 * k % 180
        c = text[911 * k:911 * k + size]
        frame = O.compress(c, 3) if k % 3 == 0 else W.frame([W.raw(c)], checksum=bool(k & 1))[0]
        entries.append((t, len(frame), len(c))); contents[t] = c
        out.extend(frame)
    fill(total, struct.pack("<I", ZSTD_MAGIC)[:3] if name == "ends_with_3_magic_bytes" else b"")
    assert len(out) == total
    _streams[name] = (bytes(out), entries, contents)
    return _streams[name]
