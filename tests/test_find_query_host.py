"""Find records by several patterns, what holds without a device: the four names in the header, _lib.EXPORTS, the library and the Python
classes; a NULL ctx refused first; zsmi_findRecordsQuery through ctypes against the Python statement of the rule (tests/_findq.py) on
every input of tests/_find.py - with K = 1 and with pattern sets cut from each text, in all three modes, the flag off and on, hit sets
asked for, capacities 0, partial and exact with a sentinel behind both arrays - and its refusals in the header's order; K = 1 / any /
no flag against zsmi_findRecords on the same bytes; and the rule of csrc/zsmi_findquery.h compiled ALONE into a host program
(tests/c/find_query.cpp) under the address and undefined-behaviour sanitizers."""
import ctypes, os, re, subprocess
import numpy as np
import pytest
import _find as F, _findq as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zstandard_amd", "csrc")
INPUTS = dict(F.inputs(), **{"split_" + k: v for k, v in F.split_inputs().items()})
CASE_TEXT = b"Error: Disk\nwarn\n\nerror AND WARN\nA\xc1a\xe1@[`{ z\nERROR"


def queries():
    """name -> (data, patterns, delim, base): every input with its own pattern alone and with the pattern sets cut from its text, and
    texts where folding matters (mixed case, bytes next to the letters' range, the delimiter a letter)"""
    c = {}
    for name, (data, pattern, delim, base) in INPUTS.items():
        c[name + "/K1"] = (data, [pattern], delim, base)
        for i, patterns in enumerate(Q.pattern_sets(data, delim)):
            c["%s/set%d" % (name, i)] = (data, patterns, delim, base)
    c["case/words"] = (CASE_TEXT, [b"error", b"WARN"], 10, 3)
    c["case/not_letters"] = (CASE_TEXT, [b"\xc1a", b"\xe1", b"@", b"[", b"`", b"{", b"Z"], 10, 0)
    c["case/delimiter_a_letter"] = (b"xAyaz\nAbA" + b"a" * 5 + b"A", [b"y", b"z\n", b"b"], ord("A"), 0)
    c["case/delimiter_a_small_letter"] = (b"xAyaz\nAbA", [b"y", b"z\n", b"b"], ord("a"), 9)
    c["eight_of_32"] = (b"q" * 100 + b"\n" + b"q" * 31 + b"\n" + b"Q" * 32, [b"q" * 32] * 8, 10, 0)
    return c


QUERIES = queries()


@pytest.fixture(scope="module")
def L():
    from zstandard_amd import _lib
    _lib.build()
    return _lib.lib()


def test_names(L):
    import zstandard_amd
    from zstandard_amd import _lib, api
    hdr = open(os.path.join(ROOT, "include", "zsmi.h")).read()
    assert "ZSMI_FIND_MAX_PATTERNS 8u" in hdr and "ZSMI_FIND_IGNORE_CASE  1u" in hdr and "ZSMI_find_any = 0, ZSMI_find_all = 1, ZSMI_find_none = 2" in hdr
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    so = ctypes.CDLL(_lib.LIB_PATH)
    for name in Q.NAMES:
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in _lib.EXPORTS and hasattr(so, name), name
    assert hasattr(api.SeekableHandle, "find_query_resident") and hasattr(api.SeekableArchive, "find_records_query")
    assert hasattr(api.BatchCodec, "find_records_query_device") and callable(zstandard_amd.find_records_query)
    assert os.path.exists(os.path.join(CSRC, "zsmi_findquery.h")) and os.path.exists(os.path.join(CSRC, "findquery.hip"))
    assert ctypes.sizeof(_lib.FindQuery) == 16 + 8 * 8 + 8 * 4                     # three words and the padding in front of the pointers


def test_a_null_ctx_is_refused_first(L):
    one = ctypes.c_void_p(8)                                                      # a non-NULL pointer no refused call looks behind
    q, keep = Q.query(L, [b"x"])
    bad, keep2 = Q.query(L, [b"\n"] * 9, mode=7, flags=6)
    assert L.zsmi_findRecordsQueryDevice(None, None, 5, 256, None, None, None, None, 3, None) == F.E_INIT
    assert L.zsmi_findRecordsQueryDevice(None, one, 5, 10, ctypes.byref(q), None, one, one, 3, one) == F.E_INIT
    assert L.zsmi_seekableFindQueryResident(None, None, None, 3, -1, ctypes.byref(bad), 2, 9, None, 0, None, None, 3, None) == F.E_INIT
    assert L.zsmi_seekableFindQueryResident(None, one, one, 3, 10, ctypes.byref(q), 0, 3, one, 10, one, one, 3, one) == F.E_INIT
    assert L.zsmi_seekableFindQueryHost(None, None, None, 3, 300, None, 2, 9, None, None, 3, None) == F.E_INIT
    assert L.zsmi_seekableFindQueryHost(None, one, one, 3, 10, ctypes.byref(q), 0, 3, one, one, 3, one) == F.E_INIT


def test_the_rule_restated_agrees_with_itself():
    """union, intersection and complement of the single-pattern answers on every query of this file (tests/_findq.py checks its own
    inputs on import)"""
    for name, (data, patterns, delim, base) in QUERIES.items():
        for flags in (0, Q.IGNORE_CASE):
            if Q.fold(data, flags).count(Q.fold(bytes([delim]), flags)) != data.count(bytes([delim])):
                continue                                                           # (a letter as delimiter, folded: the single-pattern rule would count its other case)
            if any(Q.fold(bytes([delim]), flags) in Q.fold(p, flags) for p in patterns):
                continue
            for mode in (Q.ANY, Q.ALL, Q.NONE):
                assert Q.find(data, patterns, mode, flags, delim, base)[0] == Q.by_single_patterns(data, patterns, mode, flags, delim, base), (name, mode, flags)


@pytest.mark.parametrize("flags", (0, Q.IGNORE_CASE))
@pytest.mark.parametrize("mode", sorted(Q.MODES))
@pytest.mark.parametrize("name", sorted(QUERIES))
def test_the_host_call_against_the_rule(L, name, mode, flags):
    data, patterns, delim, base = QUERIES[name]
    mode = Q.MODES[mode]
    if any(Q.fold(bytes([delim]), flags) in Q.fold(p, flags) for p in patterns):   # rule 3 refuses this query with the flag: the refusal is the answer
        q, keep = Q.query(L, patterns, mode, flags)
        assert flags and F.code(L, L.zsmi_findRecordsQuery(data, len(data), delim, ctypes.byref(q), base, None, None, 0, None)) == F.E_PARAM
        return
    records, hits, matches = Q.find(data, patterns, mode, flags, delim, base)
    n = len(records)
    assert Q.host(L, data, patterns, mode, flags, delim, base) == (n, records, hits, matches, True)
    assert Q.host(L, data, patterns, mode, flags, delim, base, capacity=0) == (n, [], [], matches, True)
    if n:
        assert Q.host(L, data, patterns, mode, flags, delim, base, capacity=n - 1) == (n, records[:-1], hits[:-1], matches, True)
        assert Q.host(L, data, patterns, mode, flags, delim, base, capacity=n // 2, want_hits=False)[:2] + (True,) == (n, records[:n // 2], True)
    assert Q.host(L, data, patterns, mode, flags, delim, base, capacity=n + 3)[:4] == (n, records, hits, matches)


def test_the_queries_reach_the_rule():
    """all three modes list something somewhere, `all` less than `any`, folding changes an answer, two bits in one hit set"""
    answers = {(name, mode, flags): Q.find(data, patterns, mode, flags, delim, base) for name, (data, patterns, delim, base) in QUERIES.items()
               if not name.startswith("case/delimiter") for mode in (0, 1, 2) for flags in (0, 1)}
    for mode in (0, 1, 2):
        assert sum(1 for (n, m, f), (r, h, c) in answers.items() if m == mode and len(r) > 1) > 5
    assert any(len(answers[(n, 1, f)][0]) < len(answers[(n, 0, f)][0]) and answers[(n, 1, f)][0] for (n, m, f) in answers)
    assert answers[("case/words", 0, 0)][0] != answers[("case/words", 0, 1)][0]
    assert any(h & (h - 1) for (r, hits, c) in answers.values() for h in hits)
    assert Q.find(CASE_TEXT, [b"error", b"WARN"], Q.ALL, 1, 10, 3) == ([6], [3], 5)
    assert Q.find(CASE_TEXT, [b"\xc1a", b"\xe1", b"@", b"[", b"`", b"{", b"Z"], Q.ANY, 1)[1] == [0b1111111]
    assert Q.find(CASE_TEXT, [b"\xe1A"], Q.ANY, 1)[0] == [] and Q.find(CASE_TEXT, [b"\xc1A"], Q.ANY, 1)[0] == [4]


@pytest.mark.parametrize("name", sorted(INPUTS))
def test_one_pattern_any_no_flag_is_the_single_pattern_call(L, name):
    data, pattern, delim, base = INPUTS[name]
    total, records, matches, intact = F.host(L, data, pattern, delim, base)
    got = Q.host(L, data, [pattern], Q.ANY, 0, delim, base)
    assert intact and got == (total, records, [1] * total, matches, True)


def test_the_host_call_refusals(L):
    """each refusal with every later one present too, so that the order shows: NULL arrays and a NULL q; delim; nPatterns, mode, flags;
    a pattern at a time its pointer, its size, the sum; the bytes against the delimiter; the source"""
    out = np.full(4, 7, dtype=np.uint64)
    hits = np.full(4, 7, dtype=np.uint8)
    p, ph = out.ctypes.data_as(ctypes.c_void_p), hits.ctypes.data_as(ctypes.c_void_p)

    def call(src, delim, patterns, mode=0, flags=0, records=p, null_q=False, **kw):
        q, keep = Q.query(L, patterns, mode, flags, **kw)
        return F.code(L, L.zsmi_findRecordsQuery(src, 3, delim, None if null_q else ctypes.byref(q), 0, records, ph, 4, None))

    assert call(None, 300, [b"\n"] * 9, 7, 6, records=None) == F.E_GENERIC         # dRecords with capacity > 0
    assert call(None, 300, [b"\n"] * 9, 7, 6, null_q=True) == F.E_GENERIC          # q
    assert call(None, 300, [b"\n"] * 9, 7, 6) == F.E_PARAM                         # delim (E_PARAM from here on: the next lines take one cause away each)
    assert call(None, -1, [b"a"]) == F.E_PARAM
    assert call(None, 10, [b"\n"] * 9, null=(0,)) == F.E_PARAM                     # nPatterns 9, in front of the NULL pointer
    assert call(None, 10, [], null=(0,)) == F.E_PARAM                              # nPatterns 0
    assert call(None, 10, [b"\n"], 3, null=(0,)) == F.E_PARAM                      # a mode above 2
    assert call(None, 10, [b"\n"], 2, 2, null=(0,)) == F.E_PARAM                   # an unknown flag bit
    assert call(None, 10, [b"a", b"\n"], sizes=[0, 1], null=(0,)) == F.E_GENERIC   # a NULL patterns[0], in front of its size
    assert call(None, 10, [b"a", b"b"], sizes=[0, 1], null=(1,)) == F.E_PARAM      # patternSizes[0] = 0, in front of the NULL patterns[1]
    assert call(None, 10, [b"a", b"b"], sizes=[257, 1], null=(1,)) == F.E_PARAM    # 257
    assert call(None, 10, [b"a" * 200, b"b" * 57, b"c"], null=(2,)) == F.E_PARAM   # a sum of 257, in front of the NULL patterns[2]
    assert call(None, 10, [b"a" * 200, b"b" * 56, b"c"], null=(2,)) == F.E_GENERIC
    assert call(None, 10, [b"a", b"b\nc"]) == F.E_PARAM                            # a delimiter inside a pattern, in front of the source
    assert call(None, ord("a"), [b"xyz", b"bAc"], flags=1) == F.E_PARAM            # ... folded
    assert call(None, ord("A"), [b"xyz", b"bac"], flags=1) == F.E_PARAM
    assert call(None, ord("A"), [b"xyz", b"bac"], flags=0) == F.E_SRC_SIZE         # without the flag 'a' is no delimiter 'A'
    assert call(None, 10, [b"a"]) == F.E_SRC_SIZE
    assert out.tolist() == [7] * 4 and hits.tolist() == [7] * 4
    q, keep = Q.query(L, [b"a" * 32] * 8, Q.ANY, 1)                                # 8 x 32 = 256 is in range
    assert L.zsmi_findRecordsQuery(b"A" * 32, 32, 10, ctypes.byref(q), 0, p, ph, 4, None) == 1 and int(out[0]) == 0 and int(hits[0]) == 255
    q, keep = Q.query(L, [b"a" * 256])
    assert L.zsmi_findRecordsQuery(b"a" * 256, 256, 10, ctypes.byref(q), 0, p, ph, 4, None) == 1


def test_the_python_call(L):
    import zstandard_amd
    for name in ("overlaps_in_lines/K1", "delim_255/set1", "lines_common/set1", "empty/K1", "case/words"):
        data, patterns, delim, base = QUERIES[name]
        for mode in Q.MODES:
            for ignore in (False, True):
                records, hits, _ = Q.find(data, patterns, Q.MODES[mode], int(ignore), delim, base)
                assert zstandard_amd.find_records_query(data, patterns, mode, ignore, bytes([delim]), base) == records, (name, mode, ignore)
                assert zstandard_amd.find_records_query(data, patterns, mode, ignore, bytes([delim]), base, return_hits=True) == (records, hits)
    with pytest.raises(RuntimeError):
        zstandard_amd.find_records_query(b"abc", [b"a", b""])
    with pytest.raises(ValueError):
        zstandard_amd.find_records_query(b"abc", [b"a"], mode="some")


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="the sanitizer build is a CPU-side check: it runs on machines without a GPU, never next to one")
def test_the_rule_under_sanitizers(tmp_path):
    """the header alone, host code only, with -fsanitize=address,undefined: the text, the patterns and the arrays in heap blocks of
    exactly their sizes; every query, mode and flag of this file"""
    exe = str(tmp_path / "find_query")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, os.path.join(ROOT, "tests", "c", "find_query.cpp"), "-o", exe])
    args, want = [], []
    for i, name in enumerate(sorted(QUERIES)):
        data, patterns, delim, base = QUERIES[name]
        open(str(tmp_path / ("t%d" % i)), "wb").write(data)
        for j, pattern in enumerate(patterns):
            open(str(tmp_path / ("p%d_%d" % (i, j))), "wb").write(pattern)
        for mode in (Q.ANY, Q.ALL, Q.NONE):
            for flags in (0, Q.IGNORE_CASE):
                if any(Q.fold(bytes([delim]), flags) in Q.fold(p, flags) for p in patterns):
                    continue
                args += [str(tmp_path / ("t%d" % i)), str(delim), str(base), str(mode), str(flags), str(len(patterns))]
                args += [str(tmp_path / ("p%d_%d" % (i, j))) for j in range(len(patterns))]
                want.append((name, mode, flags, Q.find(data, patterns, mode, flags, delim, base)))
    out = subprocess.run([exe] + args, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-4000:]
    rows = out.stdout.splitlines()
    assert len(rows) == len(want) > 300
    for (name, mode, flags, (records, hits, matches)), row in zip(want, rows):
        words = row.split()
        assert [int(w) for w in words[:2]] == [len(records), matches], (name, mode, flags)
        assert [tuple(int(v) for v in w.split(":")) for w in words[2:]] == list(zip(records, hits)), (name, mode, flags)
