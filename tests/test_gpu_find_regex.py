"""Find records by regular expression on plain text in device memory (zsmi_findRecordsRegexDevice).  The yardstick is tests/_findre.py's
Python statement of the rule (`re` on every record) on the same bytes, never another call of the library.  dRecords and dResult are exactly
as long as the header sizes them, between canaries (R.device checks them and that the source is unchanged).  The shapes are the smallest
at which the kernels can go wrong: the borders of a lane's 16 bytes, of a 4096-byte step and of a 16384-byte tile, records over several
tiles, texts that end with and without a delimiter, programs at the state and table caps, and texts of more than ROUND tiles (the carry
kernel's second round), with newlines and without any delimiter."""
import ctypes, re
import numpy as np
import pytest
import _find as F, _findre as R, _split as S
from _hip import hip_of

pytestmark = pytest.mark.gpu
LANE, STEP, TILE = F.LANE, F.STEP, F.TILE
ROUND = 512                                                                        # ZS_FINDRE_CARRY_ROUND: the tiles k_findre_carry takes a round
LONG = 3 * TILE + 1001


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


def lines(size, seed, final_delimiter=True):
    """`size` bytes of seeded lines of 0 .. 90 bytes over a small alphabet"""
    rng = np.random.default_rng(seed)
    b = bytearray(bytes(np.frombuffer(b"abcxyzERROR timeout=503 .,@[`{AZ", dtype=np.uint8)[rng.integers(0, 32, size)]))
    at = int(rng.integers(0, 90))
    while at < size:
        b[at] = 10
        at += 1 + int(rng.integers(0, 90)) * int(rng.integers(0, 2) + rng.integers(0, 2) > 0)
    if size:
        b[-1] = 10 if final_delimiter else ord("q")
    return bytes(b)


@pytest.mark.parametrize("border", (1024 + LANE * 3, STEP * 2, TILE))
def test_a_repeated_middle_across_a_border(L, H, codec, border):
    """ab+c with the b run across a lane border, a step border and a tile border, at shifts -1, 0 and +1, the record end on either side"""
    for shift in (-1, 0, 1):
        for run in (1, 2, 40):
            for end in ("before", "behind", "none"):
                b = bytearray(b"x" * (2 * TILE + 100))
                first = border + shift - run // 2                              # the run's first b
                b[first - 1:first + run + 1] = b"a" + b"b" * run + b"c"
                if end == "before":
                    b[border + shift - 1 if run > 1 else first - 2] = 10       # inside the run (it cuts the match), or in front of it
                elif end == "behind":
                    b[first + run + 1] = 10
                b[50] = 10
                R.run(L, H, codec, bytes(b), b"ab+c", what=(border, shift, run, end))
                R.run(L, H, codec, bytes(b), b"ab+c", R.INVERT, what=(border, shift, run, end, "inverted"))


@pytest.mark.parametrize("tiles", (3, 5))
def test_anchors_on_a_record_of_several_tiles(L, H, codec, tiles):
    """^x.*y$ on a record of three tiles and of five: nothing wrong, a wrong first byte, a wrong last byte"""
    n = tiles * TILE + 37
    for first, last in ((b"x", b"y"), (b"z", b"y"), (b"x", b"z")):
        body = first + b"m" * (n - 2) + last
        for text in (b"y\n" + body + b"\nx\n", body, body + b"\n", b"\n" + body):
            R.run(L, H, codec, text, b"^x.*y$", what=(tiles, first, last, len(text)))


@pytest.mark.parametrize("final_delimiter", (True, False))
@pytest.mark.parametrize("size", (1, 15, 16, 17, 4097, TILE - 1, TILE, TILE + 5, 2 * TILE, LONG))
def test_text_sizes(L, H, codec, size, final_delimiter):
    data = lines(size, size, final_delimiter)
    for pattern, flags in ((b"ERROR.*[0-9]{3}", 0), (b"^[a-c]|z$", 0), (b"error", R.IGNORE_CASE), (b"t", R.INVERT)):
        R.run(L, H, codec, data, pattern, flags)


def test_no_delimiter_and_the_empty_text(L, H, codec):
    for size in (1, 100, TILE, LONG):
        data = lines(size, 3, False).replace(b"\n", b"-")
        for pattern, flags in ((b"ERROR.*503", 0), (b"^a", R.INVERT), (b"q$", 0), (b"^$", 0)):
            d = R.run(L, H, codec, data, pattern, flags)
            assert d.result[2] == 1
    for pattern, flags in ((b"a*", 0), (b"a", R.INVERT)):
        d = R.device(L, H, codec, b"", R.program(L, pattern, flags), 0)
        assert d.rc == 0 and d.result == [0, 0, 0, 0]
        d = R.device(L, H, codec, b"", R.program(L, pattern, flags), 0, capacity=3)
        assert d.rc == 0 and d.result == [0, 0, 0, 0] and all(v == R.SENTINEL for v in d.records)


def test_empty_records(L, H, codec):
    """a* lists every record, empty ones too; invert lists the empty ones where the pattern needs a byte; ^$ exactly the empty ones"""
    data = b"\n\nab\n\n" + b"\n" * (TILE - 3) + b"x\n\n" + lines(TILE + 77, 5) + b"\n\n"
    for tail in (b"", b"z"):
        text = data + tail
        everything = list(range(R.record_count(text, 10)))
        empty = [i for i, r in enumerate(R.records_of(text, 10)) if not r]
        assert R.run(L, H, codec, text, b"a*").records == everything
        assert R.run(L, H, codec, text, b".", R.INVERT).records == empty
        assert R.run(L, H, codec, text, b"^$").records == empty and len(empty) > TILE


def test_ignore_case_and_a_letter_as_delimiter(L, H, codec):
    data = b"Error: Disk\nwarn\n\nerror AND WARN\nA\xc1a\xe1@[`{ z\nERROR" * 700
    for pattern in (b"error", b"[@-\\[]", b"[`-{]", b"[^a-z]", b"\xc1a|\xe1A", b"z$"):
        for delim in (10, ord("A"), ord("a")):
            R.run(L, H, codec, R.text_for(data, pattern, delim), pattern, R.IGNORE_CASE, delim)
            R.run(L, H, codec, R.text_for(data, pattern, delim), pattern, 0, delim)


def test_programs_at_the_caps(L, H, codec):
    """a 63-byte literal (64 states) and a program of 64 states x 48 classes (the table cap), both also across a tile border"""
    literal = bytes(0x41 + i % 7 for i in range(62)) + b"!"
    cap = bytes(range(0x30, 0x30 + 47)) + bytes(range(0x30, 0x30 + 16))
    for needle in (literal, cap):
        pattern = re.escape(needle)
        prog = R.program(L, pattern)
        assert prog.nStates == 64 and (needle is literal or prog.nStates * prog.nClasses == 3072)
        b = bytearray(lines(LONG, 11))
        for at in (100, TILE - 30, 2 * TILE - 63, 2 * TILE + STEP - 1, 3 * TILE):
            b[at:at + 63] = needle
        b[TILE + 500:TILE + 562] = needle[:62]                                     # all but the last byte
        R.run(L, H, codec, bytes(b), pattern)
        R.run(L, H, codec, bytes(b), pattern, R.INVERT)


def test_a_class_heavy_pattern(L, H, codec):
    b = bytearray(lines(LONG, 13))
    for at, address in ((10, b"10.0.0.255"), (TILE - 4, b"192.168.1.1"), (TILE + STEP - 6, b"1.2.3"), (2 * TILE + 9, b"1.22.333.4444"), (3 * TILE - 2, b"7.7.7.7")):
        b[at:at + len(address)] = address
    R.run(L, H, codec, bytes(b), b"[0-9]{1,3}(\\.[0-9]{1,3}){3}")
    R.run(L, H, codec, bytes(b), b"^[^0-9]*$")


def test_generated_patterns(L, H, codec):
    """thirty patterns of the seeded generator on one text of 3 tiles + 1001 bytes"""
    rng = np.random.default_rng(5)
    data = R.generated_text(rng, LONG)
    done = 0
    for pattern, flags in R.generated(60, seed=99):
        if R.compile(L, pattern, flags)[0] or done == 30:
            continue
        R.run(L, H, codec, data, pattern, flags)
        done += 1
    assert done == 30


def test_capacities_and_a_high_base(L, H, codec):
    data = lines(LONG, 17, False)
    pattern = b"ERROR|x.z"
    records, text_records = R.find(data, pattern)
    n = len(records)
    assert n > 20
    for cap in (0, 1, n // 2, n - 1, n, n + 5):
        R.run(L, H, codec, data, pattern, capacity=cap)
    d = R.run(L, H, codec, data, pattern, capacity=0, null_records=True)
    assert d.result == [n, 0, text_records, len(data)]
    R.run(L, H, codec, data, pattern, base=(1 << 32) + 5)
    R.run(L, H, codec, data, pattern, R.INVERT, base=(1 << 40) + 1, capacity=7)


def test_more_than_one_carry_round(L, H, codec):
    """ROUND + 1 tiles: once with newline text, once WITHOUT any delimiter - the carry's hard case, a state through every tile"""
    size = (ROUND + 1) * TILE
    body = np.frombuffer(lines(TILE * 4, 19), dtype=np.uint8)
    text = bytearray(np.tile(body, (ROUND + 1 + 3) // 4)[:size].tobytes())
    text[ROUND * TILE - 5:ROUND * TILE + 7] = b"ERROR xx 503"
    R.run(L, H, codec, bytes(text), b"ERROR.*[0-9]{3}")
    R.run(L, H, codec, bytes(text), b"^a.*z$")
    flat = bytearray(b"m" * size)
    flat[0:1] = b"x"; flat[-1:] = b"y"
    for first, last in ((b"x", b"y"), (b"z", b"y"), (b"x", b"z")):
        flat[0:1] = first; flat[-1:] = last
        d = R.run(L, H, codec, bytes(flat), b"^x.*y$")
        assert d.result[:3] == [int(first + last == b"xy"), int(first + last == b"xy"), 1]
    flat[0:1] = b"m"; flat[7 * TILE + 3:7 * TILE + 4] = b"x"; flat[(ROUND - 1) * TILE:(ROUND - 1) * TILE + 1] = b"q"; flat[-1:] = b"y"
    assert R.run(L, H, codec, bytes(flat), b"xm*qm*y$").result[0] == 1
    assert R.run(L, H, codec, bytes(flat), b"xm*y$").result[0] == 0


def test_refusals_in_order_with_nothing_queued(L, H, codec):
    from _hip import Dev, CANARY
    from _resident import down
    p = ctypes.c_void_p
    good, bad = R.program(L, b"a"), R.damaged(L)
    src, rec, res = Dev(H, 64, b"a\n" * 32), Dev(H, 64), Dev(H, 32)
    try:
        call = lambda ctx, s, size, delim, prog, records, cap, result: L.zsmi_findRecordsRegexDevice(
            ctx, s, size, delim, ctypes.byref(prog) if prog is not None else None, None, records, cap, result)
        assert call(None, None, 64, 300, None, None, 3, None) == F.E_INIT
        assert call(codec.ctx, None, 64, 300, bad["start out of range"], None, 3, None) == F.E_GENERIC                 # dResult
        assert call(codec.ctx, None, 64, 300, None, None, 3, p(res.p)) == F.E_GENERIC                                 # prog
        assert call(codec.ctx, None, 64, 300, bad["start out of range"], None, 3, p(res.p)) == F.E_GENERIC             # dRecords with capacity > 0
        assert call(codec.ctx, None, 64, 300, bad["start out of range"], p(rec.p), 3, p(res.p)) == F.E_PARAM           # delim
        assert call(codec.ctx, None, 64, -1, good, p(rec.p), 3, p(res.p)) == F.E_PARAM
        for name, prog in bad.items():
            assert call(codec.ctx, None, 64, 10, prog, p(rec.p), 3, p(res.p)) == F.E_PARAM, name                      # the program, in front of the source
        assert call(codec.ctx, None, 64, 10, good, p(rec.p), 3, p(res.p)) == F.E_SRC_SIZE
        codec.sync()
        for dev in (rec, res):
            v, ok = down(dev, np.uint8)
            assert ok and (v == CANARY).all()
        assert call(codec.ctx, p(src.p), 64, 10, good, p(rec.p), 8, p(res.p)) == 0
        codec.sync()
        assert down(res, np.uint64)[0].tolist() == [32, 8, 32, 64] and down(rec, np.uint64)[0].tolist() == list(range(8))
    finally:
        for dev in (src, rec, res):
            dev.free()


def test_the_python_method(L, H, codec):
    from _hip import Dev
    from _resident import down
    import zstandard_amd
    data = lines(LONG, 23)
    pattern = b"(error|TIMEOUT)=?5[0-9][0-9]"
    prog = zstandard_amd.compile_regex(pattern, ignore_case=True)
    records, text_records = R.find(data, pattern, R.IGNORE_CASE)
    src, rec, res = Dev(H, len(data), data), Dev(H, 8 * max(len(records), 1)), Dev(H, 32)
    try:
        for regex in (prog, pattern):
            codec.find_records_regex_device(src.p, len(data), regex, rec.p, len(records), res.p)
            codec.sync()
            want = R.find(data, pattern, R.IGNORE_CASE if regex is prog else 0)
            assert down(res, np.uint64)[0].tolist()[::2] == [len(want[0]), text_records]
            assert down(rec, np.uint64)[0].tolist()[:min(len(want[0]), len(records))] == want[0][:len(records)]
        with pytest.raises(ValueError):
            codec.find_records_regex_device(src.p, len(data), b"a\\b", rec.p, len(records), res.p)
        with pytest.raises(RuntimeError):
            codec.find_records_regex_device(src.p, len(data), prog, rec.p, len(records), res.p, delimiter=300)
    finally:
        for dev in (src, rec, res):
            dev.free()
