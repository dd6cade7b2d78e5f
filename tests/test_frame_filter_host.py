"""Frame filters, the host calls: zsmi_frameFilterSize, zsmi_buildFrameFilter, zsmi_readFrameFilter and zsmi_filterFrames against the plain
Python statement of the rule, the frame and the check (tests/_filter.py), bit for bit - on layouts that reach each rule, with every
refusal in its documented order, header damage a field at a time, the query rules, and the property the filter exists for: no frame that
holds part of a satisfying record (tests/_findq.py) is ever missing from the list.
The four CPU forms also run alone, in a host program under the address and undefined-behaviour sanitizers (tests/c/frame_filter.cpp)."""
import ctypes, os, re, struct, subprocess
import numpy as np
import pytest
import _filter as F, _findq as Q, _split as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zstandard_amd", "csrc")
CASES = F.cases()
PARAMS = [(3, 9), (4, 9), (3, 16), (4, 16), (4, 13)]


@pytest.fixture(scope="module")
def L():
    from zstandard_amd import _lib
    return _lib.lib()


def test_the_statement_reaches_each_rule(L):
    """the layouts do what their names say, by the statement - and the library agrees where a layout was built to reach a rule"""
    for name in ("gram_with_delimiter_and_border", "unclean_both", "frame_shorter_than_g", "empty_frames"):
        data, delim, sizes = CASES[name]
        assert F.host_build(L, data, sizes, delim, 4, 16)[1] == F.frame(data, sizes, delim, 4, 16), name
    sat = {name: F.saturated_frames(*[CASES[name][k] for k in (0, 2, 1)]) for name in CASES}
    assert sat["unclean_left_only"] == [0, 1] and sat["unclean_right_only"] == [1, 2] and sat["unclean_both"] == [0, 1, 2]
    assert sat["tail_without_delimiter"] == [] and sat["empty_frames"] == [] and sat["gram_with_delimiter_and_border"] == []
    assert sat["split_T400"] == [] and len(sat["split_T64_M64_cut_records"]) > 4 and len(sat["fixed_100_over_text"]) > 40
    data, delim, sizes = CASES["gram_with_delimiter_and_border"]
    slots, hashed = F.slots_of(data, sizes, delim, 4, 16)
    assert hashed == 5 + (0 + 3) + 5                                     # "abcdefgh": 5; "ij": none, "klmnop": 3; "qrstuvwx": 5 - none with "\n", none across a border
    for gram in (b"gh\ni", b"p\nqr", b"op\nq"):
        assert not all(slots[i] >> h & 1 for i in range(3) for h in F.bits_of(gram, 16))
    assert F.bits_of(b"ABCD", 13) == F.bits_of(b"abcd", 13) and F.bits_of(b"\xC1bcd", 13) != F.bits_of(b"\xE1bcd", 13)
    data, delim, sizes = CASES["frame_shorter_than_g"]
    assert F.slots_of(data, sizes, delim, 4, 9)[0][0] == 0 and F.slots_of(data, sizes, delim, 4, 9)[0][1] != 0
    assert F.slots_of(*[CASES["empty_frames"][k] for k in (0, 2, 1)], 3, 9)[0][0] == 0


@pytest.mark.parametrize("name", sorted(CASES))
def test_build_and_read_equal_the_statement(L, name):
    data, delim, sizes = CASES[name]
    for g, Lg in PARAMS:
        want = F.frame(data, sizes, delim, g, Lg)
        size, got, intact = F.host_build(L, data, sizes, delim, g, Lg)
        assert size == len(want) == L.zsmi_frameFilterSize(len(sizes), Lg) and intact, (name, g, Lg)
        assert got == want, (name, g, Lg, [i for i in range(len(want)) if got[i] != want[i]][:8])
        parsed = F.parse(want)
        info = F.host_read(L, got)
        assert info == {k: parsed[k] for k in ("n", "delim", "g", "L", "size", "saturated")}, (name, g, Lg)
        assert parsed["saturated"] >= len(F.saturated_frames(data, sizes, delim))
        # a longer buffer reads the same; nothing behind the frame is looked at
        assert F.host_read(L, got + b"\xFF" * 9) == info
        # one byte short: refused, nothing written
        code, _, untouched = F.host_build(L, data, sizes, delim, g, Lg, capacity=len(want) - 1)
        assert code == -F.E_TOO_SMALL and untouched


def test_build_refusals_in_order(L):
    data, delim, sizes = CASES["split_T400"]
    n = len(sizes)
    arr = np.ascontiguousarray(sizes, dtype=np.uint32)
    out = np.zeros(F.FIXED + n * 64, dtype=np.uint8)
    p = ctypes.c_void_p

    def build(dst=True, cap=None, src=data, size=len(data), szs=True, count=n, d=10, g=4, lg=9):
        r = L.zsmi_buildFrameFilter(p(out.ctypes.data) if dst else None, len(out) if cap is None else cap, src, size, p(arr.ctypes.data) if szs else None, count, d, g, lg)
        return -int(L.zsmi_getErrorCode(r)) if L.zsmi_isError(r) else int(r)
    # each refusal with every later one present too
    assert build(d=256, g=5, lg=8, count=1 << 26, dst=False, size=len(data) + 1, cap=0) == -F.E_PARAM
    assert build(d=-1) == build(g=2) == build(g=5) == build(lg=8) == build(lg=17) == -F.E_PARAM
    assert build(count=1 << 26, dst=False, size=len(data) + 1, cap=0) == -F.E_FRAME_INDEX
    assert build(dst=False, size=len(data) + 1, cap=0) == build(szs=False, size=len(data) + 1, cap=0) == -F.E_GENERIC
    assert build(src=None, cap=0) == build(size=len(data) - 1, cap=0) == -F.E_SRC_SIZE
    assert build(cap=len(out) - 1) == -F.E_TOO_SMALL
    assert not out.any(), "a refused build wrote"
    assert build() == len(out)
    assert L.zsmi_isError(L.zsmi_frameFilterSize(3, 8)) and L.zsmi_getErrorCode(L.zsmi_frameFilterSize(3, 17)) == F.E_PARAM
    assert L.zsmi_getErrorCode(L.zsmi_frameFilterSize(1 << 26, 9)) == F.E_FRAME_INDEX and L.zsmi_frameFilterSize((1 << 26) - 1, 9) == 40 + 64 * ((1 << 26) - 1)
    assert L.zsmi_frameFilterSize(0, 16) == 40 and L.zsmi_getErrorCode(L.zsmi_frameFilterSize(1 << 19, 16)) == F.E_FRAME_INDEX


def test_header_damage_a_field_at_a_time(L):
    data, delim, sizes = CASES["split_T400"]
    good = F.frame(data, sizes, delim, 4, 9)
    assert isinstance(F.host_read(L, good), dict)

    def flipped(at, bit):
        b = bytearray(good); b[at] ^= bit
        return bytes(b)
    assert F.host_read(L, good[:39]) == F.E_SRC_SIZE and F.host_read(L, b"") == F.E_SRC_SIZE
    assert F.host_read(L, flipped(0, 1)) == F.host_read(L, flipped(3, 0x80)) == F.host_read(L, flipped(8, 1)) == F.host_read(L, flipped(11, 2)) == F.E_PREFIX
    assert F.host_read(L, flipped(12, 1)) == F.host_read(L, flipped(12, 2)) == F.E_VERSION
    for at, bit in ((14, 1), (14, 4), (15, 0x10), (15, 8), (20, 1), (23, 0x80), (4, 1), (7, 0x40), (16, 1)):
        assert F.host_read(L, flipped(at, bit)) == F.E_CORRUPT, (at, bit)
    assert F.host_read(L, good[:-1]) == F.E_SRC_SIZE
    grown = bytearray(good); struct.pack_into("<I", grown, 16, len(sizes) + 1); struct.pack_into("<I", grown, 4, 32 + 64 * (len(sizes) + 1))
    assert F.host_read(L, bytes(grown)) == F.E_SRC_SIZE                  # a consistent header that names more slots than there are bytes
    for at, bit in ((13, 1), (24, 1), (31, 0x80), (32, 1), (39, 0x80), (40, 1), (len(good) - 1, 0x80), (40 + 64 * 3 + 17, 4)):
        assert F.host_read(L, flipped(at, bit)) == F.E_CORRUPT, (at, bit)
    # order: the magic before the version before the fields before the size before the check
    both = bytearray(flipped(0, 1)); both[12] ^= 1; both[14] = 9
    assert F.host_read(L, bytes(both)) == F.E_PREFIX
    both = bytearray(flipped(12, 1)); both[14] = 9
    assert F.host_read(L, bytes(both[:-1])) == F.E_VERSION
    both = bytearray(flipped(14, 1))
    assert F.host_read(L, bytes(both[:-1])) == F.E_CORRUPT
    assert F.host_read(L, flipped(40, 1)[:-1]) == F.E_SRC_SIZE
    from zstandard_amd._lib import FrameFilterInfo
    assert L.zsmi_readFrameFilter(good, len(good), None) == F.E_GENERIC and L.zsmi_readFrameFilter(None, 100, ctypes.byref(FrameFilterInfo())) == F.E_SRC_SIZE


def test_filter_refusals_in_order(L):
    data, delim, sizes = CASES["split_T400"]
    good = F.frame(data, sizes, delim, 4, 9)
    n = len(sizes)
    q, keep = Q.query(L, [b"abcd"])
    out = np.zeros(n, dtype=np.uint32); res = np.zeros(4, dtype=np.uint64)
    p = ctypes.c_void_p

    def call(buf=good, size=None, query=q, first=0, count=n, frames=True, cap=n, result=True):
        return L.zsmi_filterFrames(buf, len(buf) if size is None else size, ctypes.byref(query) if query is not None else None, first, count,
                                   p(out.ctypes.data) if frames else None, cap, p(res.ctypes.data) if result else None)
    bad_magic = bytes([good[0] ^ 1]) + good[1:]
    bad_q = Q.query(L, [b"ab\ncd"])[0]
    assert call(query=None, buf=bad_magic) == call(result=False, buf=bad_magic) == call(frames=False, buf=bad_magic) == F.E_GENERIC
    assert call(frames=False, cap=0) == 0
    assert call(buf=None, size=100, query=bad_q) == call(size=39, query=bad_q) == F.E_SRC_SIZE
    assert call(buf=bad_magic, query=bad_q, first=n) == F.E_PREFIX
    assert call(buf=good[:12] + b"\x02" + good[13:], query=bad_q) == F.E_VERSION
    assert call(buf=good[:15] + b"\x11" + good[16:], query=bad_q) == F.E_CORRUPT
    assert call(buf=good[:-1], query=bad_q) == F.E_SRC_SIZE
    assert call(query=bad_q, first=n, count=1) == F.E_PARAM
    for patterns, mode, flags, sizes_, null in (([], 0, 0, None, ()), ([b"a"] * 9, 0, 0, None, ()), ([b"ab"], 3, 0, None, ()), ([b"ab"], 0, 2, None, ()),
                                                ([b"ab"], 0, 0, [0], ()), ([b"ab"], 0, 0, [257], ()), ([b"a" * 200, b"b" * 57], 0, 0, None, ())):
        assert call(query=Q.query(L, patterns, mode, flags, sizes_, null)[0]) == F.E_PARAM, (patterns, mode, flags)
    assert call(query=Q.query(L, [b"ab", b"cd"], null=(1,))[0]) == F.E_GENERIC
    assert call(query=Q.query(L, [b"ab", b"c\n"])[0]) == F.E_PARAM                       # the FILTER's delimiter
    zero = F.frame(*[CASES["delim_0"][k] for k in (0, 2, 1)], 4, 9)
    assert call(buf=zero, query=Q.query(L, [b"ab", b"c\n"])[0], count=0) == 0 and call(buf=zero, query=Q.query(L, [b"a\0"])[0], count=0) == F.E_PARAM
    assert call(first=1, count=n) == call(first=n + 1, count=0) == call(first=0xFFFFFFFF, count=2) == F.E_PARAM
    assert call(first=n, count=0) == 0 and [int(v) for v in res] == [0, 0, 0, 0]
    damaged = bytearray(good); damaged[39] ^= 0x80                                       # the check is zsmi_readFrameFilter's to judge
    assert call(buf=bytes(damaged)) == 0


@pytest.mark.parametrize("name", sorted(CASES))
def test_filter_frames_equals_the_statement(L, name):
    data, delim, sizes = CASES[name]
    rng = np.random.default_rng(7)
    n = len(sizes)
    for g, Lg in ((4, 9), (3, 13)):
        buf = F.frame(data, sizes, delim, g, Lg)
        for patterns, mode, flags in F.queries(data, delim, rng) + [([b"x"], Q.NONE, 0), ([b"Q", b"zz"], Q.NONE, Q.IGNORE_CASE)]:
            if any(bytes([delim]) in p or (flags and (bytes([delim]).lower() in p.lower())) for p in patterns):
                continue
            want, sat = F.filter_frames(buf, patterns, mode)
            rc, got, result, intact = F.host_filter(L, buf, patterns, mode, flags)
            assert (rc, got, result, intact) == (0, want, [len(want), len(want), n, sat], True), (name, g, Lg, patterns, mode, flags)
            # IGNORE_CASE gives the list of the folded pattern: one filter serves both
            assert F.host_filter(L, buf, [F.fold(p) for p in patterns], mode, 0)[1] == want
            for first, count in ((0, 0), (n // 3, n - n // 3), (n // 2, min(1, n - n // 2)), (0, n // 2)):
                w, s = F.filter_frames(buf, patterns, mode, first, count)
                for cap in {0, max(len(w) - 1, 0), len(w), count}:
                    rc, got, result, intact = F.host_filter(L, buf, patterns, mode, flags, first, count, cap)
                    assert (rc, got, result, intact) == (0, w[:cap], [len(w), min(len(w), cap), count, s], True), (name, patterns, first, count, cap)


def test_query_rules(L):
    data, delim, sizes = CASES["split_T400"]
    n = len(sizes)
    buf = F.frame(data, sizes, delim, 4, 13)
    at = F.offsets_of(sizes)
    piece = max(data[at[5]:at[6]].split(b"\n"), key=len)[:8]             # a frame of whole records: the piece lies in one of them
    assert len(piece) == 8
    every = list(range(n))
    hit = F.host_filter(L, buf, [piece])[1]
    assert 5 in hit and len(hit) < n // 2
    assert F.host_filter(L, buf, [piece[:3]])[1] == every                               # m < g: every frame
    assert F.host_filter(L, buf, [piece, piece[:3]], Q.ANY)[1] == every                  # any: the short pattern passes
    assert F.host_filter(L, buf, [piece, piece[:3]], Q.ALL)[1] == hit                    # all: the long one decides
    assert F.host_filter(L, buf, [piece[:2], piece[:3]], Q.ALL)[1] == every
    assert F.host_filter(L, buf, [piece], Q.NONE)[1] == every                           # none: the filter cannot help
    assert F.host_filter(L, buf, [b"zqzqzqzq"])[1] == [] and F.host_filter(L, buf, [piece, b"zqzqzqzq"], Q.ALL)[1] == []
    assert F.host_filter(L, buf, [piece, b"zqzqzqzq"], Q.ANY)[1] == hit
    assert F.host_filter(L, buf, [piece.upper()], Q.ANY, Q.IGNORE_CASE)[1] == hit == F.host_filter(L, buf, [piece.upper()], Q.ANY, 0)[1]
    # a saturated frame passes everything, an empty frame nothing but what passes every frame
    data, delim, sizes = CASES["unclean_both"]
    assert F.host_filter(L, F.frame(data, sizes, delim, 4, 9), [b"zqzqzqzq"])[1:3] == ([0, 1, 2], [3, 3, 3, 3])
    data, delim, sizes = CASES["empty_frames"]
    buf = F.frame(data, sizes, delim, 4, 9)
    assert F.host_filter(L, buf, [b"cdef"])[1] == [1] and F.host_filter(L, buf, [b"cd"])[1] == [0, 1, 2, 3, 4, 5]


def layouts():
    """(name, data, delim, sizes): the cases, and seeded splitter and fixed-size layouts with cut records"""
    out = [(name,) + CASES[name] for name in sorted(CASES)]
    for seed in range(4):
        text = F.tokens(5000 + 700 * seed, 20 + seed, every=30 + 40 * seed, upper=0.2 * (seed % 2))
        out.append(("seeded_split_%d" % seed, text, 10, S.Split(text, 10, min(200 + 90 * seed, 96 << seed), 96 << seed).sizes))
        out.append(("seeded_fixed_%d" % seed, text, 10, F.fixed(len(text), 97 + 31 * seed)))
    return out


@pytest.mark.parametrize("layout", layouts(), ids=lambda v: v[0])
def test_no_false_negatives(L, layout):
    """every frame that holds any part of a record that satisfies the query is in the list"""
    name, data, delim, sizes = layout
    rng = np.random.default_rng(len(data))
    tried, ends = 0, F.record_ends(data, delim)
    for g, Lg in ((4, 9), (3, 10), (4, 13)):
        size, buf, _ = F.host_build(L, data, sizes, delim, g, Lg)
        assert size > 0
        for patterns, mode, flags in F.queries(data, delim, rng):
            records, _, _ = Q.find(data, patterns, mode, flags, delim)
            need = F.frames_of_records(data, sizes, records, delim, ends)
            rc, got, result, _ = F.host_filter(L, buf, patterns, mode, flags)
            assert rc == 0 and set(need) <= set(got), (name, g, Lg, patterns, mode, flags, sorted(set(need) - set(got)))
            tried += len(need)
            # a list never separates a record's frames: they lie in one run
            runs = F.runs_of(got, sizes)
            for r in records:
                fr = F.frames_of_records(data, sizes, [r], delim, ends)
                assert len({k for k, (a, c) in enumerate(runs) for f in fr if a <= f < a + c}) == 1, (name, patterns, r, fr, runs)
    assert tried or not data.strip(bytes([delim]))


def test_names(L):
    from zstandard_amd import _lib, api
    import zstandard_amd
    hdr = open(os.path.join(ROOT, "include", "zsmi.h")).read()
    so = ctypes.CDLL(_lib.LIB_PATH)
    for name in F.NAMES:
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in _lib.EXPORTS and hasattr(so, name), name
    for name in ("frame_filter_size", "build_frame_filter", "read_frame_filter", "filter_frames"):
        assert hasattr(api, name) and hasattr(zstandard_amd, name), name
    for name in ("build_frame_filter_device", "check_frame_filter_device", "filter_frames_device"):
        assert hasattr(api.BatchCodec, name), name
    for name in ("build_frame_filter_resident", "find_query_frames_resident", "find_frames_work_bound"):
        assert hasattr(api.SeekableHandle, name), name
    assert hasattr(api.SeekableArchive, "build_frame_filter")
    one = ctypes.c_void_p(8)
    q, keep = Q.query(L, [b"ab"])
    assert L.zsmi_buildFrameFilterDevice(None, None, 5, None, 0, 999, 9, 99, None, 0, None) == F.E_INIT
    assert L.zsmi_seekableBuildFrameFilterResident(None, None, 999, 9, 99, None, 0, None, 0, None) == F.E_INIT
    assert L.zsmi_seekableBuildFrameFilterHost(None, None, 999, 9, 99, None, 0, None) == F.E_INIT
    assert L.zsmi_seekableFindQueryFramesResident(None, one, one, 1, 999, ctypes.byref(q), one, one, 1, one, 8, one, None, 1, one) == F.E_INIT
    assert L.zsmi_seekableFindQueryFramesHost(None, one, one, 1, 999, ctypes.byref(q), one, 1, one, None, 1, one) == F.E_INIT and L.zsmi_seekableFindFramesWorkBound(None, 5) == 0
    assert L.zsmi_checkFrameFilterDevice(None, one, 40, one) == F.E_INIT and L.zsmi_filterFramesDevice(None, one, 40, ctypes.byref(q), 0, 0, None, 0, one) == F.E_INIT


def test_python_surface(L):
    from zstandard_amd import api
    for name in ("split_T64_M64_cut_records", "empty_frames", "no_frames", "delim_0", "upper_case_and_high_bytes"):
        data, delim, sizes = CASES[name]
        want = F.frame(data, sizes, delim, 3, 10)
        assert api.frame_filter_size(len(sizes), 10) == len(want)
        buf = api.build_frame_filter(data, sizes, bytes([delim]), gram=3, log2_bits=10)
        assert buf == want
        parsed = F.parse(want)
        assert api.read_frame_filter(buf) == {"frames": len(sizes), "delimiter": bytes([delim]), "gram": 3, "log2_bits": 10, "size": len(data), "saturated": parsed["saturated"]}
        for patterns, mode in (([b"the"], "any"), ([b"zqzq", b"ab"], "all"), ([b"x"], "none")):
            w, s = F.filter_frames(want, patterns, Q.MODES[mode])
            assert api.filter_frames(buf, patterns, mode) == w
            assert api.filter_frames(buf, patterns, mode, return_info=True) == (w, {"tested": len(sizes), "saturated": s})
            half = len(sizes) // 2
            assert api.filter_frames(buf, patterns, mode, ignore_case=True, first_frame=half) == F.filter_frames(want, patterns, Q.MODES[mode], half)[0]
    with pytest.raises(RuntimeError):
        api.read_frame_filter(b"\0" * 40)
    with pytest.raises(RuntimeError):
        api.filter_frames(F.frame(b"ab\n", [3]), [b"a\nb"])
    with pytest.raises(RuntimeError):
        api.build_frame_filter(b"abc", [2])
    with pytest.raises(ValueError):
        api.build_frame_filter(b"abc", [3], b"\r\n")


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="the sanitizer build is a CPU-side check: it runs on machines without a GPU, never next to one")
def test_the_cpu_forms_under_sanitizers(L, tmp_path):
    """the header alone, host code only, with -fsanitize=address,undefined: every input and every output in a heap block of exactly its size"""
    exe = str(tmp_path / "frame_filter")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, os.path.join(ROOT, "tests", "c", "frame_filter.cpp"), "-o", exe])
    args, names, wants = [], sorted(CASES), []
    for k, name in enumerate(names):
        data, delim, sizes = CASES[name]
        g, Lg = PARAMS[k % len(PARAMS)]
        at = F.offsets_of(sizes)
        inner = bytes(b for b in data[at[len(sizes) // 2]:][:7] if b != delim) or b"q"      # a piece of the middle frame, or a byte that is none of these texts'
        stem = str(tmp_path / ("case%d" % k))
        open(stem + ".text", "wb").write(data)
        open(stem + ".sizes", "wb").write(np.asarray(sizes, dtype=np.uint32).tobytes())
        open(stem + ".pattern", "wb").write(inner)
        args += ["case", stem + ".text", str(delim), stem + ".sizes", str(g), str(Lg), stem + ".pattern", stem]
        wants.append((g, Lg, inner))
    out = subprocess.run([exe] + args, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-4000:]
    rows = out.stdout.splitlines()
    assert len(rows) == len(names)
    for k, (name, row) in enumerate(zip(names, rows)):
        data, delim, sizes = CASES[name]
        g, Lg, inner = wants[k]
        want = F.frame(data, sizes, delim, g, Lg)
        parsed = F.parse(want)
        w, s = F.filter_frames(want, [inner])
        assert row.split() == [str(len(want)), str(-F.E_TOO_SMALL), "1", str(len(sizes)), str(delim), str(g), str(Lg), str(len(data)), str(parsed["saturated"]),
                               str(-F.E_SRC_SIZE), str(len(w)), str(len(w)), str(len(sizes)), str(s), ",".join(str(v) for v in w) or "-",
                               str(len(w) - 1) if w else "-", str(len(w))], name
        assert open(str(tmp_path / ("case%d" % k)) + ".frame", "rb").read() == want, name
    out = subprocess.run([exe, "rejections"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-4000:]
    got = dict(line.split() for line in out.stdout.splitlines())
    want = {"size_log_low": -F.E_PARAM, "size_log_high": -F.E_PARAM, "size_too_many": -F.E_FRAME_INDEX, "size_good": 232,
            "build_delim": -F.E_PARAM, "build_gram": -F.E_PARAM, "build_log": -F.E_PARAM, "build_too_many": -F.E_FRAME_INDEX, "build_null_dst": -F.E_GENERIC,
            "build_null_sizes": -F.E_GENERIC, "build_null_text": -F.E_SRC_SIZE, "build_sum": -F.E_SRC_SIZE, "build_short": -F.E_TOO_SMALL, "build_good": 232,
            "read_null_info": -F.E_GENERIC, "read_39_bytes": -F.E_SRC_SIZE, "read_outer_magic": -F.E_PREFIX, "read_inner_magic": -F.E_PREFIX, "read_version": -F.E_VERSION,
            "read_gram": -F.E_CORRUPT, "read_log": -F.E_CORRUPT, "read_reserved": -F.E_CORRUPT, "read_frame_size": -F.E_CORRUPT, "read_n": -F.E_CORRUPT,
            "read_cut": -F.E_SRC_SIZE, "read_delim": -F.E_CORRUPT, "read_size": -F.E_CORRUPT, "read_check": -F.E_CORRUPT, "read_slot_bit": -F.E_CORRUPT, "read_good": 0,
            "filter_null_query": -F.E_GENERIC, "filter_null_result": -F.E_GENERIC, "filter_null_frames": -F.E_GENERIC, "filter_39_bytes": -F.E_SRC_SIZE,
            "filter_outer_magic": -F.E_PREFIX, "filter_version": -F.E_VERSION, "filter_log": -F.E_CORRUPT, "filter_cut": -F.E_SRC_SIZE, "filter_patterns": -F.E_PARAM,
            "filter_mode": -F.E_PARAM, "filter_flags": -F.E_PARAM, "filter_null_pattern": -F.E_GENERIC, "filter_pattern_size": -F.E_PARAM, "filter_pattern_delim": -F.E_PARAM,
            "filter_window": -F.E_PARAM, "filter_check_not_judged": 0, "filter_good": 0}
    assert {k: int(v) for k, v in got.items()} == want
