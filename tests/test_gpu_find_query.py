"""Find records by several patterns on plain text in device memory (zsmi_findRecordsQueryDevice).  The yardstick is tests/_findq.py's Python
statement of the rule on the same bytes, never another call of the library.  dRecords, dHits and dResult are exactly as long as the header
sizes them, between canaries (Q.device checks them and that the source is unchanged); nothing depends on a wait inside the call.  The
shapes are the smallest at which the kernels can go wrong: the borders of a lane's 16 bytes, of a 4096-byte step and of a 16384-byte
tile, records over several tiles whose patterns sit in different tiles, texts that end with and without a delimiter, and texts of more
than 1024 tiles (the scans' later tiles) and of more than ROUND tiles (the carry kernel's second round)."""
import ctypes
import numpy as np
import pytest
import _find as F, _findq as Q, _split as S
from _hip import hip_of

pytestmark = pytest.mark.gpu
LANE, STEP, TILE = F.LANE, F.STEP, F.TILE
ROUND = 4096                                                                       # ZS_FINDQ_CARRY_ROUND: the tiles k_findq_carry takes a round
ANY, ALL, NONE = Q.ANY, Q.ALL, Q.NONE


@pytest.fixture(scope="module")
def L():
    from zstandard_amd import _lib
    return _lib.lib()


@pytest.fixture(scope="module")
def H():
    return hip_of()


@pytest.fixture(scope="module")
def codec():
    from zstandard_amd import BatchCodec
    bc = BatchCodec(0)
    yield bc
    bc.close()


def run(L, H, codec, data, patterns, mode=ANY, flags=0, delim=10, base=None, what="", **kw):
    d = Q.device(L, H, codec, data, patterns, mode, flags, delim, base, **kw)
    Q.same_as_rule(d, data, patterns, mode, flags, delim, base or 0, kw.get("capacity"), kw.get("null_hits", False), what)
    return d


def modes(L, H, codec, data, patterns, flags=0, delim=10, base=None, what=""):
    return [run(L, H, codec, data, patterns, mode, flags, delim, base, what=(what, mode)) for mode in (ANY, ALL, NONE)]


def place(size, placed, delims=(), fill=b"a"):
    """`size` filler bytes with pattern at start for (pattern, start) in placed and a newline at every position of `delims`"""
    b = bytearray(fill * size)
    for p in delims:
        b[p] = 10
    for pattern, p in placed:
        assert 0 <= p and p + len(pattern) <= size and 10 not in b[p:p + len(pattern)]
        b[p:p + len(pattern)] = pattern
    return bytes(b)


# ------------------------------------------------------------------ 1. occurrences of two patterns on every side of every border
P2, P17 = F.pattern_of(2), b"#" + F.pattern_of(17)[1:]                             # different first bytes: neither occurs inside the other


def borders(kind, count):
    """`count` borders of one kind, 1024 bytes apart at least: a lane border that is no step's, a step border that is no tile's, a tile's"""
    if kind == "lane":
        return [1024 * (j + 1) + LANE * (1 + j % 5) for j in range(count)]
    if kind == "step":
        return [TILE * j + STEP * (1 + j % 3) for j in range(count)]
    return [TILE * (j + 1) for j in range(count)]


@pytest.mark.parametrize("mode", (ANY, ALL))
@pytest.mark.parametrize("kind", ("lane", "step", "tile"))
def test_border_shifts(L, H, codec, kind, mode):
    """at border j the 17-byte pattern starts at shift -17 .. 0 - it ends at the border, crosses it with every split of its bytes, starts
    at it - and the 2-byte pattern follows it in the same record at the shifts -2 .. 0 of the border 512 bytes on (a lane border too),
    every third record without it.  A delimiter in front of each record: a lost or doubled occurrence shows in the numbers and the sets"""
    shifts = list(range(-17, 1))
    at = borders(kind, len(shifts))
    assert all(b % LANE == 0 for b in at) and (kind != "lane" or all(b % STEP for b in at)) and (kind != "step" or all(b % STEP == 0 and b % TILE for b in at))
    placed, delims = [], []
    for j, (b, s) in enumerate(zip(at, shifts)):
        placed.append((P17, b + s))
        if b + s > 0:
            delims.append(b + s - 1)
        if j % 3:
            placed.append((P2, b + 512 + (-2, -1, 0)[j % 3]))
    size = at[-1] + 600 + 37                                                       # (odd: the last tile goes byte by byte)
    data = place(size, placed, delims)
    records, hits, matches = Q.find(data, [P2, P17], mode)
    assert matches == len(placed) and len(records) == (len(shifts) if mode == ANY else sum(1 for j in range(len(shifts)) if j % 3))
    run(L, H, codec, data, [P2, P17], mode, what=(kind, mode))
    run(L, H, codec, data, [P17, P2], mode, what=(kind, mode, "swapped"))


# ------------------------------------------------------------------ 2. records and tiles
def test_a_record_of_three_tiles(L, H, codec):
    """P_0 only in the first tile, P_1 only in the third: all lists the record, any once, none not"""
    A, B = b"!alpha", b"#be"
    data = place(40000, [(A, 100), (B, 2 * TILE + 2000)])
    d = modes(L, H, codec, data, [A, B], what="one record")
    assert [x.records for x in d] == [[0], [0], []] and d[0].hits == [3] and d[0].result[2] == 2
    data = place(40000, [(A, 100), (B, 2 * TILE + 2000)], delims=[39999])
    d = modes(L, H, codec, data, [A, B], what="one record, terminated")
    assert [x.records for x in d] == [[0], [0], []]
    data = place(40000, [(A, 100), (B, 2 * TILE + 2000)], delims=[TILE - 1])         # a delimiter as a tile's last byte: two records, one pattern each
    d = modes(L, H, codec, data, [A, B], what="cut at a tile's last byte")
    assert [x.records for x in d] == [[0, 1], [], []] and d[0].hits == [1, 2]
    data = place(40000, [(A, 100), (B, TILE), (A, 2 * TILE + 2000)], delims=[TILE - 1, 2 * TILE])     # ... an occurrence as the next tile's first bytes, a record end as the third's first
    d = modes(L, H, codec, data, [A, B], base=1 << 33, what="two records and a tail")
    assert d[0].records == [1 << 33, (1 << 33) + 1, (1 << 33) + 2] and d[0].hits == [1, 2, 1] and d[2].records == []
    data = place(40000, [(A, TILE - 3), (B, 2 * TILE + 2000)], delims=[50, 2 * TILE + 1999, 39000])   # crosses the border; the third tile's head holds none
    d = modes(L, H, codec, data, [A, B], what="across and behind")
    assert d[0].records == [1, 2] and d[1].records == [] and d[2].records == [0, 3]


def test_a_record_of_five_tiles(L, H, codec):
    """nothing in the middle three tiles: the set passes through them"""
    A, B = b"!alpha", b"#be"
    data = place(5 * TILE, [(A, 10), (B, 4 * TILE + 9)], delims=[4, 4 * TILE + 100])
    d = modes(L, H, codec, data, [A, B], what="through empty tiles")
    assert [x.records for x in d] == [[1], [1], [0, 2]] and d[1].hits == [3] and d[2].hits == [0, 0]
    data = place(5 * TILE, [(A, 10), (B, 4 * TILE + 9)], delims=[4, 2 * TILE + 5])   # ... and is dropped by a delimiter in the middle tile
    d = modes(L, H, codec, data, [A, B], what="cut in the middle tile")
    assert [x.records for x in d] == [[1, 2], [], [0]]


# ------------------------------------------------------------------ 3. none
def test_none_lists_empty_records(L, H, codec):
    data = b"\n\nx\n\n" + b"y\n" * 3 + b"\n" * 40 + b"x" + b"\n" * 9000 + b"x\n\n"
    for patterns in ([b"x"], [b"x", b"y"], [b"q"]):
        modes(L, H, codec, data, patterns, what=("empty records", patterns))
    d = run(L, H, codec, b"\n\n", [b"x"], NONE, what="two empty records")
    assert d.records == [0, 1] and d.result == [2, 2, 0, 2]


@pytest.mark.parametrize("size", (1, 15, 16, 17, 4097, TILE - 1, TILE, TILE + 5, 2 * TILE, 3 * TILE + 1001))
def test_the_text_ends_with_and_without_a_delimiter(L, H, codec, size):
    text = S.text_lines(3 * TILE + 2000, seed=size)
    word = b"Z!"                                                                   # (the text is small letters and newlines)
    for last in (b"\n", b"x"):
        data = text[:size - 1] + last
        for patterns in ([b"e"], [b"e", b"th"], [word]):
            modes(L, H, codec, data, patterns, what=("ends with", last, size, patterns))
        if size > 3:
            tail = data[:size - 3] + word + b"x"                                        # only the unterminated last record holds the word
            d = modes(L, H, codec, tail, [word], what=("the word in the tail", size))
            assert d[0].result[0] == 1 and d[0].hits == [1]


def test_no_delimiter_at_all(L, H, codec):
    for size in (5, TILE, TILE + 5, 3 * TILE + 77):
        data = place(size, [(b"#be", size - 3)])
        d = modes(L, H, codec, data, [b"!alpha", b"#be"], what=("one record", size))
        assert [x.records for x in d] == [[0], [], []] and d[0].hits == [2]
        d = modes(L, H, codec, data, [b"!alpha"], base=7, what=("one record without", size))
        assert [x.records for x in d] == [[], [], [7]] and d[2].hits == [0]


def test_the_empty_text(L, H, codec):
    for mode in (ANY, ALL, NONE):
        d = run(L, H, codec, b"", [b"x", b"y"], mode, what="empty")
        assert d.result == [0, 0, 0, 0]
    d = run(L, H, codec, b"abc", [b"abcd"], NONE, what="longer than the text")
    assert d.result == [1, 1, 0, 3] and d.records == [0]


# ------------------------------------------------------------------ 4. folding
CASE_TEXT = b"an ErRoR here\nerror\nERROR\nA\xc1a\xe1@[`{ z\nEr\nror\n" * 900 + b"tail ERRor"


def test_folding(L, H, codec):
    assert len(CASE_TEXT) > 2 * TILE
    for patterns in ([b"error"], [b"ErRoR"], [b"error", b"HERE", b"Z"]):
        on = modes(L, H, codec, CASE_TEXT, patterns, flags=1, what=("flag on", patterns))
        off = modes(L, H, codec, CASE_TEXT, patterns, flags=0, what=("flag off", patterns))
        assert on[0].result[0] > off[0].result[0]
    d = run(L, H, codec, CASE_TEXT, [b"error"], ANY, 1)
    assert d.result[0] == 3 * 900 + 1


def test_bytes_next_to_the_letters_do_not_fold(L, H, codec):
    """'@' 0x40 and '[' 0x5B around 'A' .. 'Z', '`' 0x60 and '{' 0x7B around 'a' .. 'z', 0xC1 / 0xE1 = 'A' / 'a' with bit 7"""
    pairs = ((b"@", b"`"), (b"[", b"{"), (b"\xc1", b"\xe1"))
    text = b"".join(x + b"A\n" + y + b"a\n" for x, y in pairs) * 600
    for x, y in pairs:
        for patterns in ([x], [y], [x + b"a"], [y + b"A"], [x, y]):
            modes(L, H, codec, text, patterns, flags=1, what=("flag on", patterns))
        d = run(L, H, codec, text, [x + b"A", y + b"A"], ANY, 1)
        assert d.result[0] == 1200 and set(d.hits) == {1, 2}                       # the letters fold, their neighbours keep the two apart
    data = bytes(range(256)) * 70
    modes(L, H, codec, data, [bytes([b]) for b in (0x40, 0x5B, 0x60, 0x7B, 0xC1, 0xE1, 0x41, 0x7A)], flags=1, what="every byte value")
    modes(L, H, codec, data, [b"@A", b"Z[", b"`a", b"z{", b"\xc0\xc1", b"\xe0\xe1"], flags=1, what="every byte value, pairs")


def test_a_letter_as_delimiter(L, H, codec):
    """delimiter 'A': 'a' in the text is no delimiter, with the flag and without; no pattern may hold either under the flag"""
    text = (b"xxAyyazzAbbbaaaaA" * 1100)[:TILE + 333]
    for flags in (0, 1):
        d = modes(L, H, codec, text, [b"yy", b"ZZ", b"b"], flags=flags, delim=ord("A"), what=("delimiter A", flags))
        assert d[0].result[3] == len(text)
    d = run(L, H, codec, text, [b"yya"], ANY, 0, ord("A"), what="the flag off: 'a' is a pattern byte like another")
    assert d.result[0] > 900
    assert Q.device(L, H, codec, text, [b"yya"], ANY, 1, ord("A"), capacity=0).rc == F.E_PARAM


# ------------------------------------------------------------------ 5. pattern sets
def test_two_equal_patterns_set_two_bits(L, H, codec):
    data = S.text_lines(TILE + 900, seed=4)
    d = run(L, H, codec, data, [b"th", b"th"], ANY, what="equal")
    assert set(d.hits) == {3} and d.result[2] == 2 * data.count(b"th")
    assert run(L, H, codec, data, [b"th", b"th"], ALL).records == d.records


def test_a_prefix_of_another(L, H, codec):
    data = S.text_lines(2 * TILE + 900, seed=5)
    for patterns in ([b"th", b"the"], [b"the", b"th"], [b"e", b"er", b"ere"], [b"a", b"a" * 2]):
        modes(L, H, codec, data, patterns, what=("prefixes", patterns))
    d = run(L, H, codec, data, [b"th", b"the"], ANY)
    assert {1, 3} == set(d.hits)                                                   # never the longer one alone


def test_eight_patterns_of_32_bytes(L, H, codec):
    """the byte limit: 8 x 32 = 256"""
    rng = np.random.default_rng(8)
    patterns = [bytes([0x30 + j]) + rng.integers(0x41, 0x5B, 31, dtype=np.uint8).tobytes() for j in range(8)]
    text = bytearray(S.text_lines(3 * TILE, seed=6))
    for i, p in enumerate(range(700, 3 * TILE - 100, 1777)):
        j = i % 9
        if j < 8 and 10 not in text[p:p + 32]:
            text[p:p + 32] = patterns[j]
    last = bytes(text).rfind(b"\n")
    text[last + 1:last + 1] = b"".join(patterns)                                   # one record with all eight
    for flags in (0, 1):
        d = modes(L, H, codec, bytes(text), patterns, flags=flags, what=("8 x 32", flags))
        assert d[1].result[0] == 1 and d[1].hits == [255]
    lower = [p.lower() for p in patterns]
    assert run(L, H, codec, bytes(text), lower, ALL, 1).hits == [255] and run(L, H, codec, bytes(text), lower, ALL, 0).result[0] == 0


def test_one_repeated_byte(L, H, codec):
    """64 KiB of q against 8 patterns of q x 32: every position is a candidate of every pattern and every compare runs to the end"""
    data = b"q" * (64 << 10)
    d = modes(L, H, codec, data, [b"q" * 32] * 8, what="64 KiB of q")
    assert d[0].result[:3] == [1, 1, 8 * ((64 << 10) - 31)] and d[0].hits == [255]
    lines = bytearray(data)
    for p in (0, 31, 32, 33, STEP - 1, STEP + 31, TILE - 32, TILE, TILE + 33, (64 << 10) - 1):
        lines[p] = 10
    modes(L, H, codec, bytes(lines), [b"q" * 32] * 8, what="in lines")
    modes(L, H, codec, bytes(lines), [b"Q" * (32 - j) for j in range(8)], flags=1, what="in lines, lengths 25 .. 32, folded")


# ------------------------------------------------------------------ 6. hits, capacity, wide words
def test_hits_and_a_null_dhits(L, H, codec):
    data = S.text_lines(4 * TILE + 123, seed=14)
    patterns = [b"e", b"th", b"zz", b"a", b"in"]
    for mode in (ANY, ALL, NONE):
        d = run(L, H, codec, data, patterns, mode, what=("hits", mode))
        assert len(set(d.hits)) > (4 if mode == ANY else 0)
        run(L, H, codec, data, patterns, mode, null_hits=True, what=("no hits", mode))


def test_capacity(L, H, codec):
    data = S.text_lines(5 * TILE, seed=12)
    patterns = [b"e", b"th"]
    for mode in (ANY, ALL, NONE):
        total = len(Q.find(data, patterns, mode)[0])
        assert total > 30
        run(L, H, codec, data, patterns, mode, capacity=0, null_records=True, null_hits=True, what="only count")
        for cap in (0, 1, total - 1, total, total + 5):
            run(L, H, codec, data, patterns, mode, capacity=cap, base=9, what=("capacity", mode, cap))
    tail = data.rstrip(b"\n") + b" the end"                                         # the unterminated last record is the one capacity cuts off
    total = len(Q.find(tail, patterns, ALL)[0])
    for cap in (total - 1, total):
        run(L, H, codec, tail, patterns, ALL, capacity=cap, what=("capacity at the tail", cap))


def test_a_base_above_2_to_the_32(L, H, codec):
    data = S.text_lines(TILE + 77, seed=15)
    for base in ((1 << 32) + 5, (1 << 63) + 11):
        for d in modes(L, H, codec, data, [b"e", b"th"], base=base, what=("base", base)):
            assert all(v >= base for v in d.records)


# ------------------------------------------------------------------ 7. long texts
@pytest.mark.parametrize("edge", (1024, ROUND))
def test_more_than_1024_tiles(L, H, codec, edge):
    """about 17 MiB and about 65 MiB: the scans' later tiles, and k_findq_carry's second round, which begins at tile ROUND.  One record runs
    from tile edge - 2 into tile edge + 2 - across tile `edge` - and holds P_0 only in front of the border and P_1 only behind it"""
    block = S.text_lines(1 << 16, seed=3)
    size = (edge + 64) * TILE + 333
    data = bytearray(block * (size // len(block) + 1))[:size]
    A, B = b"!XY7", b"#QQ"
    a, b = (edge - 2) * TILE + 100, (edge + 2) * TILE + 50
    data[a:b] = b"a" * (b - a)
    for pattern, p in ((A, (edge - 1) * TILE + 5), (B, (edge + 1) * TILE + 9), (A, 5000), (B, (edge + 40) * TILE + 7777), (A, edge * TILE - 2)):
        data[p:p + len(pattern)] = pattern
    data = bytes(data)
    assert len(data) > edge * TILE and b"\n" not in data[a:b] and data.count(A) == 3 and data.count(B) == 2
    d = run(L, H, codec, data, [A, B], ALL, what="the record across the border")
    assert d.result[:3] == [1, 1, 5] and d.hits == [3]
    d = run(L, H, codec, data, [A, B], ANY, what="any")
    assert d.result[0] == 3 and d.hits == [1, 3, 2]
    if edge == 1024:
        run(L, H, codec, data, [A, B], NONE, base=5, what="none: nearly every record")
        run(L, H, codec, data, [b"ab", b"THE"], ANY, 1, what="common, folded")
    else:
        total = len(Q.find(data, [A, B], NONE)[0])
        run(L, H, codec, data, [A, B], NONE, capacity=total, null_hits=True, what="none behind the second round")


# ------------------------------------------------------------------ 8. the host checks
def test_refusals_in_order(L, H, codec):
    """each refusal with every later one present too, so that the order shows; a refused call queues nothing and leaves every array as it
    was"""
    from _hip import Dev, CANARY
    from _resident import down
    p = ctypes.c_void_p
    src, rec, hit, res = Dev(H, 64, b"ab\n" * 21), Dev(H, 64), Dev(H, 8), Dev(H, 32)
    find = L.zsmi_findRecordsQueryDevice

    def q(patterns, mode=0, flags=0, **kw):
        made = Q.query(L, patterns, mode, flags, **kw)
        q.keep.append(made)
        return ctypes.byref(made[0])
    q.keep = []
    worst = lambda: q([b"\n"] * 9, 7, 6)
    try:
        assert find(None, None, 5, 256, None, None, None, None, 3, None) == F.E_INIT
        assert find(codec.ctx, None, 5, 256, worst(), None, p(rec.p), p(hit.p), 3, None) == F.E_GENERIC            # dResult
        assert find(codec.ctx, None, 5, 256, None, None, p(rec.p), p(hit.p), 3, p(res.p)) == F.E_GENERIC           # q
        assert find(codec.ctx, None, 5, 256, worst(), None, None, p(hit.p), 3, p(res.p)) == F.E_GENERIC            # dRecords with capacity > 0
        assert find(codec.ctx, None, 5, 256, worst(), None, p(rec.p), p(hit.p), 3, p(res.p)) == F.E_PARAM          # delim
        assert find(codec.ctx, None, 5, -1, q([b"a"]), None, p(rec.p), p(hit.p), 3, p(res.p)) == F.E_PARAM
        assert find(codec.ctx, None, 5, 10, q([b"\n"] * 9, null=(0,)), None, p(rec.p), p(hit.p), 3, p(res.p)) == F.E_PARAM       # nPatterns 9
        assert find(codec.ctx, None, 5, 10, q([], null=(0,)), None, p(rec.p), p(hit.p), 3, p(res.p)) == F.E_PARAM                # nPatterns 0
        assert find(codec.ctx, None, 5, 10, q([b"\n"], 3, null=(0,)), None, p(rec.p), p(hit.p), 3, p(res.p)) == F.E_PARAM        # mode 3
        assert find(codec.ctx, None, 5, 10, q([b"\n"], 2, 2, null=(0,)), None, p(rec.p), p(hit.p), 3, p(res.p)) == F.E_PARAM     # an unknown flag
        assert find(codec.ctx, None, 5, 10, q([b"a", b"\n"], sizes=[0, 1], null=(0,)), None, p(rec.p), p(hit.p), 3, p(res.p)) == F.E_GENERIC     # a NULL patterns[0]
        assert find(codec.ctx, None, 5, 10, q([b"a", b"b"], sizes=[0, 1], null=(1,)), None, p(rec.p), p(hit.p), 3, p(res.p)) == F.E_PARAM        # a size of 0
        assert find(codec.ctx, None, 5, 10, q([b"a" * 200, b"b" * 57, b"\n"]), None, p(rec.p), p(hit.p), 3, p(res.p)) == F.E_PARAM               # a sum of 257
        assert find(codec.ctx, None, 5, 10, q([b"a", b"b\nc"]), None, p(rec.p), p(hit.p), 3, p(res.p)) == F.E_PARAM              # a delimiter in a pattern
        assert find(codec.ctx, None, 5, ord("a"), q([b"x", b"bAc"], flags=1), None, p(rec.p), p(hit.p), 3, p(res.p)) == F.E_PARAM     # ... folded
        assert find(codec.ctx, None, 5, 10, q([b"ab"]), None, p(rec.p), p(hit.p), 3, p(res.p)) == F.E_SRC_SIZE                   # a NULL source
        codec.sync()
        for dev in (rec, hit, res):
            v, ok = down(dev)
            assert ok and (v == CANARY).all()
        assert find(codec.ctx, p(src.p), 63, 10, q([b"ab", b"B"], 1, 1), None, p(rec.p), p(hit.p), 8, p(res.p)) == 0              # and the call they all refuse
        codec.sync()
        assert down(res, np.uint64)[0].tolist() == [21, 8, 42, 63] and down(rec, np.uint64)[0].tolist() == list(range(8)) and down(hit, np.uint8)[0].tolist() == [3] * 8
    finally:
        for dev in (src, rec, hit, res):
            dev.free()


def test_the_python_method(L, H, codec):
    from _hip import Dev
    from _resident import down
    data = S.text_lines(TILE + 500, seed=2)
    records, hits, matches = Q.find(data, [b"ZZ", b"e"], Q.ALL, 1)
    assert records
    src, rec, hit, res = Dev(H, len(data), data), Dev(H, 8 * len(records)), Dev(H, len(records)), Dev(H, 32)
    try:
        codec.find_records_query_device(src.p, len(data), [b"ZZ", b"e"], rec.p, hit.p, len(records), res.p, mode="all", ignore_case=True)
        codec.sync()
        assert down(res, np.uint64)[0].tolist() == [len(records), len(records), matches, len(data)]
        assert down(rec, np.uint64)[0][:len(records)].tolist() == records and down(hit, np.uint8)[0][:len(records)].tolist() == hits
        with pytest.raises(RuntimeError):
            codec.find_records_query_device(src.p, len(data), [b"z\nz"], rec.p, hit.p, len(records), res.p)
    finally:
        for dev in (src, rec, hit, res):
            dev.free()
