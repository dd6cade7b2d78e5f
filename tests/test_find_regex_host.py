"""Find records by regular expression, what holds without a device: the names in the header, _lib.EXPORTS, the library and the Python
classes; a NULL ctx refused first; zsmi_compileRegex and zsmi_findRecordsRegex through ctypes against the Python statement of the rule
(tests/_findre.py: `re` on every record) - a catalogue of hand-written patterns that reaches every construct, on every input of
tests/_find.py under the delimiters newline, comma, 'A' and 0, and a seeded generator of random patterns on short random texts; every
refusal of the compiler in the header's order with its offset; the pinned sizes of minimal programs; damaged programs refused before
use; capacities 0, partial and exact; textRecords; a literal against zsmi_findRecords; invert as the complement; and the header compiled
ALONE into a host program (tests/c/find_regex.cpp) under the address and undefined-behaviour sanitizers."""
import ctypes, os, re, subprocess
import numpy as np
import pytest
import _find as F, _findre as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zstandard_amd", "csrc")
INPUTS = dict(F.inputs(), **{"split_" + k: v for k, v in F.split_inputs().items()})
DELIMS = (10, ord(","), ord("A"), 0)
CASE_TEXT = b"Error: Disk\nwarn\n\nerror AND WARN\nA\xc1a\xe1@[`{ z\nERROR,needle\nxNEEDLE\n10.0.0.255 two\n1.2.3\nabbbc abc ac\n\\ $ ^ } ]\tq\na\nb,\n\n"
TEXTS = dict({name: v[0] for name, v in INPUTS.items()}, case=CASE_TEXT)             # every input, whole
PROGRAMS, RULE = {}, {}


def program(L, pattern, flags=0):
    """a pattern's program, compiled once"""
    if (pattern, flags) not in PROGRAMS:
        PROGRAMS[(pattern, flags)] = R.program(L, pattern, flags)
    return PROGRAMS[(pattern, flags)]


@pytest.fixture(scope="module")
def L():
    from zstandard_amd import _lib
    _lib.build()
    return _lib.lib()


def test_names(L):
    import zstandard_amd
    from zstandard_amd import _lib, api
    hdr = open(os.path.join(ROOT, "include", "zsmi.h")).read()
    assert "ZSMI_REGEX_MAX_STATES 64u" in hdr and "ZSMI_REGEX_MAX_TABLE  3072u" in hdr and "ZSMI_REGEX_INVERT     2u" in hdr
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    so = ctypes.CDLL(_lib.LIB_PATH)
    for name in R.NAMES:
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in _lib.EXPORTS and hasattr(so, name), name
    assert hasattr(api.SeekableHandle, "find_regex_resident") and hasattr(api.SeekableArchive, "find_records_regex")
    assert hasattr(api.BatchCodec, "find_records_regex_device") and callable(zstandard_amd.find_records_regex) and callable(zstandard_amd.compile_regex)
    assert os.path.exists(os.path.join(CSRC, "zsmi_regex.h")) and os.path.exists(os.path.join(CSRC, "findregex.hip"))
    assert ctypes.sizeof(_lib.RegexProgram) == 3352


def test_a_null_ctx_is_refused_first(L):
    one = ctypes.c_void_p(8)                                                      # a non-NULL pointer no refused call looks behind
    prog = R.program(L, b"x")
    bad = R.damaged(L)["start out of range"]
    assert L.zsmi_findRecordsRegexDevice(None, None, 5, 256, None, None, None, 3, None) == F.E_INIT
    assert L.zsmi_findRecordsRegexDevice(None, one, 5, 10, ctypes.byref(prog), None, one, 3, one) == F.E_INIT
    assert L.zsmi_seekableFindRegexResident(None, None, None, 3, -1, ctypes.byref(bad), 2, 9, None, 0, None, 3, None) == F.E_INIT
    assert L.zsmi_seekableFindRegexResident(None, one, one, 3, 10, ctypes.byref(prog), 0, 3, one, 10, one, 3, one) == F.E_INIT
    assert L.zsmi_seekableFindRegexHost(None, None, None, 3, 300, None, 2, 9, None, 3, None) == F.E_INIT
    assert L.zsmi_seekableFindRegexHost(None, one, one, 3, 10, ctypes.byref(prog), 0, 3, one, 3, one) == F.E_INIT


def rule(data, pattern, flags, delim, base):
    """the rule's answer, computed once a (text, pattern, flags, delimiter): many inputs share a text"""
    key = (data, pattern, flags, delim)
    if key not in RULE:
        RULE[key] = R.find(data, pattern, flags, delim, 0)
    records, text_records = RULE[key]
    return [base + r for r in records], text_records


def test_the_catalogue_reaches_every_construct(L):
    """about 60 patterns and a dozen more for repeats over groups; each construct of the syntax stands in one, Python reads every one of
    them and the compiler accepts every one of them"""
    joined = b" ".join(p for p, _ in R.CATALOGUE)
    assert 55 <= len(R.CATALOGUE) <= 90
    for piece in (b"\\.", b"\\x", b"\\t", b"\\n", b"\\d", b"\\D", b"\\w", b"\\W", b"\\s", b"\\S", b"[^", b"[]", b"[^]", b"-]", b"[-", b"[x[", b"(?:", b"|", b"*", b"+", b"?",
                  b"{3}", b"{2,}", b"{1,3}", b"^", b"$", b"()", b"\xff"):
        assert piece in joined, piece
    assert {f for _, f in R.CATALOGUE} == {0, 1, 2, 3}
    for pattern, flags in R.CATALOGUE:
        R.python_regex(pattern, flags)
        assert R.compile(L, pattern, flags)[::2] == (0, 0), (pattern, flags)
    # an unbounded repeat on a group that holds an alternative, and on one that holds a quantifier
    loops = [p for p, _ in R.CATALOGUE if re.search(rb"\([^()]*\|[^()]*\)(\*|\+|\{\d+,\})", p)], [p for p, _ in R.CATALOGUE if re.search(rb"\([^()]*[*+?}][^()]*\)(\*|\+|\{\d+,\})", p)]
    assert len(loops[0]) >= 5 and len(loops[1]) >= 5, loops


@pytest.mark.parametrize("delim", DELIMS)
@pytest.mark.parametrize("name", sorted(TEXTS))
def test_the_catalogue_against_re(L, name, delim):
    """every pattern of the catalogue on one text under one delimiter: the host call's numbers and textRecords are the rule's"""
    for pattern, flags in R.CATALOGUE:
        data = R.text_for(TEXTS[name], pattern, delim)
        prog = program(L, pattern, flags)
        records, text_records = rule(data, pattern, flags, delim, 7)
        assert R.host(L, data, prog, delim, 7) == (len(records), records, text_records, True), (pattern, flags)


def test_generated_patterns_against_re(L):
    """300 seeded patterns of the accepted grammar, each on short random texts under the newline and the comma.  A pattern the compiler
    refuses for its size is skipped, and at most a tenth of them may be"""
    rng = np.random.default_rng(77)
    patterns = R.generated(300, seed=2026)
    assert len(set(patterns)) > 250
    too_big = 0
    for pattern, flags in patterns:
        rc, prog, at = R.compile(L, pattern, flags)
        if rc:
            assert (rc, at) == (F.E_PARAM, len(pattern)), (pattern, rc, at)        # nothing but the size refusal: the grammar is the accepted one
            too_big += 1
            continue
        for delim in (10, 44):
            for size in (0, 1, 7, 40, 120):
                data = R.text_for(R.generated_text(rng, size), pattern, delim)
                records, text_records = R.find(data, pattern, flags, delim, 3)
                assert R.host(L, data, prog, delim, 3) == (len(records), records, text_records, True), (pattern, flags, delim, data)
    assert too_big <= len(patterns) // 10, too_big


def test_pinned_program_sizes(L):
    """the minimal DFA is unique, so its size is a fact"""
    for pattern, states in ((b"abc", 4), (b"abc$", 4), (b"^abc", 5), (b"^abc$", 5), (b"a|b", 2), (b"a*", 1), (b"a" * 63, 64), (b"^$", 2), (b".", 2)):
        prog = R.program(L, pattern)
        assert prog.nStates == states and prog.start < states, (pattern, prog.nStates)
    prog = R.program(L, b"abc")
    assert prog.nClasses == 4 and [prog.classOf[b] for b in b"abcz\x00\xff"] == [0 + 1, 2, 3, 0, 0, 0] and prog.accept == 1 << 3 and prog.flags == 0
    assert R.program(L, b"abc", R.IGNORE_CASE).classOf[ord("B")] == R.program(L, b"abc", R.IGNORE_CASE).classOf[ord("b")]
    assert R.program(L, b"abc", 3).flags == 3
    cap = bytes(range(0x30, 0x30 + 47)) + bytes(range(0x30, 0x30 + 16))                # 63 bytes, 47 of them distinct: 64 states x 48 classes
    prog = R.program(L, re.escape(cap))
    assert (prog.nStates, prog.nClasses) == (64, 48)


REFUSALS = [
    # 2. parameter_outOfBound in front of everything the pattern holds
    (b"a\\b(", 4, F.E_PARAM, 0),
    # 3. recognised and left out: parameter_unsupported, in front of every malformation
    (b"a^b", 0, F.E_UNSUPPORTED, 1), (b"(^a)", 0, F.E_UNSUPPORTED, 1), (b"^^a", 0, F.E_UNSUPPORTED, 1), (b"a|b^", 0, F.E_UNSUPPORTED, 3),
    (b"a$b", 0, F.E_UNSUPPORTED, 1), (b"(a$)", 0, F.E_UNSUPPORTED, 2), (b"$a", 0, F.E_UNSUPPORTED, 0), (b"a$*", 0, F.E_UNSUPPORTED, 1),
    (b"a\\b", 0, F.E_UNSUPPORTED, 1), (b"\\Ba", 0, F.E_UNSUPPORTED, 0), (b"\\Aa", 0, F.E_UNSUPPORTED, 0), (b"a\\Z", 0, F.E_UNSUPPORTED, 1),
    (b"(a)\\1", 0, F.E_UNSUPPORTED, 3), (b"\\0", 0, F.E_UNSUPPORTED, 0), (b"\\z", 0, F.E_UNSUPPORTED, 0), (b"[a\\b]", 0, F.E_UNSUPPORTED, 2),
    (b"(?=a)", 0, F.E_UNSUPPORTED, 0), (b"(?P<n>a)", 0, F.E_UNSUPPORTED, 0), (b"a(?i)", 0, F.E_UNSUPPORTED, 1), (b"(?", 0, F.E_UNSUPPORTED, 0),
    (b"a*?", 0, F.E_UNSUPPORTED, 2), (b"a+?", 0, F.E_UNSUPPORTED, 2), (b"a??", 0, F.E_UNSUPPORTED, 2), (b"a{2}?", 0, F.E_UNSUPPORTED, 4),
    (b"a*+", 0, F.E_UNSUPPORTED, 2), (b"a++", 0, F.E_UNSUPPORTED, 2), (b"a?+", 0, F.E_UNSUPPORTED, 2), (b"a{1,2}+", 0, F.E_UNSUPPORTED, 6),
    (b"(a\\b", 0, F.E_UNSUPPORTED, 2), (b")[\\A", 0, F.E_UNSUPPORTED, 2), (b"*a{x}b\\1", 0, F.E_UNSUPPORTED, 6),
    # 4. malformed: parameter_outOfBound
    (b"(a", 0, F.E_PARAM, 0), (b"a(b(c)", 0, F.E_PARAM, 1), (b"a)", 0, F.E_PARAM, 1), (b"[a", 0, F.E_PARAM, 0), (b"a[]", 0, F.E_PARAM, 1), (b"a(b[c)", 0, F.E_PARAM, 3),
    (b"*a", 0, F.E_PARAM, 0), (b"a|*", 0, F.E_PARAM, 2), (b"(*a)", 0, F.E_PARAM, 1), (b"(?:+)", 0, F.E_PARAM, 3), (b"a**", 0, F.E_PARAM, 2),
    (b"a{2}{3}", 0, F.E_PARAM, 4), (b"a{2}*", 0, F.E_PARAM, 4), (b"a*{2}", 0, F.E_PARAM, 2), (b"^*", 0, F.E_PARAM, 1),
    (b"a{", 0, F.E_PARAM, 1), (b"a{x}", 0, F.E_PARAM, 1), (b"a{,2}", 0, F.E_PARAM, 1), (b"a{2", 0, F.E_PARAM, 1), (b"{2}", 0, F.E_PARAM, 0),
    (b"a{2,1}", 0, F.E_PARAM, 1), (b"a{256}", 0, F.E_PARAM, 1), (b"a{1,256}", 0, F.E_PARAM, 1), (b"a{3,}x{99999999999}", 0, F.E_PARAM, 6),
    (b"[b-a]", 0, F.E_PARAM, 1), (b"[a-\\d]", 0, F.E_PARAM, 1), (b"[\\d-z]", 0, F.E_PARAM, 1), (b"[^z-\\x41]", 0, F.E_PARAM, 2),
    (b"a\\", 0, F.E_PARAM, 1), (b"[a\\", 0, F.E_PARAM, 2), (b"\\xg1", 0, F.E_PARAM, 0), (b"a\\x1", 0, F.E_PARAM, 1), (b"[\\x]", 0, F.E_PARAM, 1),
    (b"(" * 201 + b"a" + b")" * 201, 0, F.E_PARAM, 200),
    # 5. above the caps: parameter_outOfBound at the pattern's end
    (b"a.{20}b", 0, F.E_PARAM, 7), (b"a" * 64, 0, F.E_PARAM, 64), (b"(a{255}){255}", 0, F.E_PARAM, 13), (re.escape(bytes(range(0x30, 0x30 + 55))), 0, F.E_PARAM, len(re.escape(bytes(range(0x30, 0x30 + 55))))),
    (b"(a|b)*a(a|b){7}$", 0, F.E_PARAM, 16),
]


def test_the_compiler_refusals(L):
    """every refusal of the header, in its order, with the offset at which it was decided; a refused call leaves prog as it was"""
    from zstandard_amd._lib import RegexProgram
    prog = RegexProgram()
    at = ctypes.c_size_t(99)
    assert L.zsmi_compileRegex(None, 0, 4, ctypes.byref(prog), ctypes.byref(at)) == F.E_GENERIC            # 1. in front of the size and the flags
    assert L.zsmi_compileRegex(b"\\b", 0, 4, None, None) == F.E_GENERIC
    assert L.zsmi_compileRegex(b"\\b", 0, 0, ctypes.byref(prog), None) == F.E_PARAM                        # 2. (errorAt may be NULL)
    for pattern, flags, code, where in REFUSALS:
        ctypes.memset(ctypes.byref(prog), 0x5A, ctypes.sizeof(prog))
        assert R.compile(L, pattern, flags)[::2] == (code, where), (pattern, R.compile(L, pattern, flags)[::2], (code, where))
        assert L.zsmi_compileRegex(pattern, len(pattern), flags, ctypes.byref(prog), None) == code
        assert bytes(prog) == b"\x5a" * ctypes.sizeof(prog), pattern
    assert R.compile(L, b"(" * 200 + b"a" + b")" * 200)[0] == 0 and R.compile(L, b"a{255}")[0] == F.E_PARAM and R.compile(L, b"a{0,63}b")[0] == 0


def test_a_damaged_program_is_refused_before_use(L):
    out = np.full(4, 7, dtype=np.uint64)
    p = out.ctypes.data_as(ctypes.c_void_p)
    for name, prog in R.damaged(L).items():
        assert F.code(L, L.zsmi_findRecordsRegex(b"abbc\n", 5, 10, ctypes.byref(prog), 0, p, 4, None)) == F.E_PARAM, name
    assert out.tolist() == [7] * 4
    good = R.program(L, b"ab+c")
    assert L.zsmi_findRecordsRegex(b"abbc\n", 5, 10, ctypes.byref(good), 0, p, 4, None) == 1 and int(out[0]) == 0


def test_the_host_call_refusals(L):
    """each refusal with every later one present too: NULL arrays and a NULL prog; delim; the program; the source"""
    out = np.full(4, 7, dtype=np.uint64)
    p = out.ctypes.data_as(ctypes.c_void_p)
    good, bad = R.program(L, b"a"), R.damaged(L)["next out of range"]
    call = lambda src, delim, prog, records=p: F.code(L, L.zsmi_findRecordsRegex(src, 3, delim, ctypes.byref(prog) if prog is not None else None, 0, records, 4, None))
    assert call(None, 300, bad, records=None) == F.E_GENERIC
    assert call(None, 300, None) == F.E_GENERIC
    assert call(None, 300, bad) == F.E_PARAM and call(None, -1, good) == F.E_PARAM and call(None, 256, good) == F.E_PARAM
    assert call(None, 10, bad) == F.E_PARAM
    assert call(None, 10, good) == F.E_SRC_SIZE
    assert out.tolist() == [7] * 4


@pytest.mark.parametrize("name", sorted(TEXTS))
def test_capacities_and_text_records(L, name):
    data = TEXTS[name]
    for pattern, flags, delim in ((b"e", 0, 10), (b"^$", R.INVERT, 10), (b"[a-z]+\\d|two", R.IGNORE_CASE, 0), (b"a*", 0, 44)):
        prog = R.program(L, pattern, flags)
        records, text_records = R.find(data, pattern, flags, delim, 1 << 40)
        n = len(records)
        assert text_records == R.record_count(data, delim)
        assert R.host(L, data, prog, delim, 1 << 40, capacity=0) == (n, [], text_records, True)
        if n:
            assert R.host(L, data, prog, delim, 1 << 40, capacity=n - 1) == (n, records[:-1], text_records, True)
            assert R.host(L, data, prog, delim, 1 << 40, capacity=n // 2) == (n, records[:n // 2], text_records, True)
        assert R.host(L, data, prog, delim, 1 << 40, capacity=n) == (n, records, text_records, True)
        assert R.host(L, data, prog, delim, 1 << 40, capacity=n + 3) == (n, records, text_records, True)


@pytest.mark.parametrize("name", sorted(INPUTS))
def test_a_literal_gives_the_single_pattern_answer(L, name):
    """a pattern without metacharacters, escaped: zsmi_findRecords' records"""
    data, pattern, delim, base = INPUTS[name]
    if len(pattern) > 63:
        pattern = pattern[:63]                                                     # (64 states at the most)
    total, records, _, intact = F.host(L, data, pattern, delim, base)
    prog = R.program(L, re.escape(pattern))
    assert intact and R.host(L, data, prog, delim, base)[:2] == (total, records)
    assert prog.nStates == len(pattern) + 1


@pytest.mark.parametrize("name", sorted(TEXTS))
def test_invert_is_the_complement(L, name):
    data = TEXTS[name]
    for pattern, flags in ((b"e", 0), (b"^.{0,3}$", 0), (b"[^a]", R.IGNORE_CASE)):
        yes = R.host(L, data, R.program(L, pattern, flags), 10, 5)
        no = R.host(L, data, R.program(L, pattern, flags | R.INVERT), 10, 5)
        assert yes[2] == no[2] and sorted(yes[1] + no[1]) == list(range(5, 5 + yes[2])) and not set(yes[1]) & set(no[1])


def test_the_python_calls(L):
    import zstandard_amd
    from zstandard_amd import _lib
    for pattern, flags in R.CATALOGUE[::5]:
        for delim in (10, 44):
            data = R.text_for(CASE_TEXT, pattern, delim)
            prog = zstandard_amd.compile_regex(pattern, ignore_case=bool(flags & 1), invert=bool(flags & 2))
            assert isinstance(prog, _lib.RegexProgram)
            assert zstandard_amd.find_records_regex(data, prog, bytes([delim]), 9) == R.find(data, pattern, flags, delim, 9)[0]
    assert zstandard_amd.find_records_regex(b"GET /api/v12/x\nPUT /api/v1/\nPOST /api/v/", b"(GET|POST) /api/v[0-9]+/") == [0]
    with pytest.raises(ValueError, match="Unsupported parameter.*offset 1|parameter_unsupported.*offset 1"):
        zstandard_amd.compile_regex(b"a\\b")
    with pytest.raises(ValueError, match="offset 0"):
        zstandard_amd.find_records_regex(b"abc", b"(a")
    with pytest.raises(RuntimeError):
        zstandard_amd.find_records_regex(b"abc", R.damaged(L)["start out of range"])


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="the sanitizer build is a CPU-side check: it runs on machines without a GPU, never next to one")
def test_the_header_under_sanitizers(L, tmp_path):
    """the header alone, host code only, with -fsanitize=address,undefined: the pattern, the text and the arrays in heap blocks of exactly
    their sizes; the catalogue on four texts, and every refusal"""
    exe = str(tmp_path / "find_regex")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, os.path.join(ROOT, "tests", "c", "find_regex.cpp"), "-o", exe])
    args, want = [], []
    texts = [(CASE_TEXT, 10), (TEXTS["lines_common"][:4000], 10), (TEXTS["delim_0"], 0), (b"", 10)]
    patterns = [(p, f) for p, f in R.CATALOGUE] + [(p, f) for p, f, _, _ in REFUSALS]
    for j, (pattern, flags) in enumerate(patterns):
        open(str(tmp_path / ("p%d" % j)), "wb").write(pattern)
    for i, (data, delim) in enumerate(texts):
        for j, (pattern, flags) in enumerate(patterns):
            text = R.text_for(data, pattern, delim)
            name = str(tmp_path / ("t%d_%d" % (i, int(text is not data and text != data))))
            open(name, "wb").write(text)
            args += [name, str(delim), "11", str(flags), str(tmp_path / ("p%d" % j))]
            rc, prog, at = R.compile(L, pattern, flags)
            want.append((pattern, flags, "refused %d %d" % (rc, at) if rc else (prog.nStates, prog.nClasses) + R.find(text, pattern, flags, delim, 11)))
    out = subprocess.run([exe] + args, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-4000:]
    rows = out.stdout.splitlines()
    assert len(rows) == len(want) > 500
    for (pattern, flags, answer), row in zip(want, rows):
        if isinstance(answer, str):
            assert row == answer, (pattern, flags)
        else:
            words = [int(w) for w in row.split()]
            assert (words[0], words[1], words[4:], words[3]) == answer and words[2] == len(answer[2]), (pattern, flags)
