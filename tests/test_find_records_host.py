"""Find records by content, what holds without a device: the five names in the header, _lib.EXPORTS, the library and the Python classes;
the first host check (a NULL ctx is refused in front of every later refusal; the order behind it needs a context and is the GPU files');
the work bound of no handle; zsmi_findRecords through ctypes against the Python statement of the rule (tests/_find.py) on every input,
with capacities 0 and total - 1 and its refusals; and the rule of csrc/zsmi_find.h compiled ALONE into a host program
(tests/c/find_records.cpp) under the address and undefined-behaviour sanitizers."""
import ctypes, os, re, subprocess
import numpy as np
import pytest
import _find as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zstandard_amd", "csrc")
INPUTS_OF_SPLIT = F.split_inputs()
INPUTS = dict(F.inputs(), **{"split_" + k: v for k, v in INPUTS_OF_SPLIT.items()})


@pytest.fixture(scope="module")
def L():
    from zstandard_amd import _lib
    _lib.build()
    return _lib.lib()


def test_names(L):
    import zstandard_amd
    from zstandard_amd import _lib, api
    hdr = open(os.path.join(ROOT, "include", "zsmi.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    so = ctypes.CDLL(_lib.LIB_PATH)
    for name in F.NAMES:
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in _lib.EXPORTS and hasattr(so, name), name
    for name in ("find_records_resident", "find_work_bound"):
        assert hasattr(api.SeekableHandle, name), name
    assert hasattr(api.SeekableArchive, "find_records") and hasattr(api.BatchCodec, "find_records_device")
    assert callable(zstandard_amd.find_records)
    assert os.path.exists(os.path.join(CSRC, "zsmi_find.h")) and os.path.exists(os.path.join(CSRC, "find.hip"))


def test_a_null_ctx_is_refused_first(L):
    """init_missing with every later refusal present too: NULL arrays, a delimiter, pattern sizes and a window out of range"""
    one = ctypes.c_void_p(8)                                                      # a non-NULL pointer no refused call looks behind
    assert L.zsmi_findRecordsDevice(None, None, 5, 256, None, 0, None, None, 3, None) == F.E_INIT
    assert L.zsmi_findRecordsDevice(None, one, 5, 10, b"x", 1, None, one, 3, one) == F.E_INIT
    assert L.zsmi_seekableFindRecordsResident(None, None, None, 3, -1, None, 257, 2, 9, None, 0, None, 3, None) == F.E_INIT
    assert L.zsmi_seekableFindRecordsResident(None, one, one, 3, 10, b"x", 1, 0, 3, one, 10, one, 3, one) == F.E_INIT
    assert L.zsmi_seekableFindRecordsHost(None, None, None, 3, 300, None, 0, 2, 9, None, 3, None) == F.E_INIT
    assert L.zsmi_seekableFindRecordsHost(None, one, one, 3, 10, b"x", 1, 0, 3, one, 3, one) == F.E_INIT
    assert L.zsmi_seekableFindWorkBound(None, 0, 0) == 0 and L.zsmi_seekableFindWorkBound(None, 7, 3) == 0


@pytest.mark.parametrize("name", sorted(INPUTS))
def test_the_host_call_against_the_rule(L, name):
    data, pattern, delim, base = INPUTS[name]
    records, matches = F.find(data, pattern, delim, base)
    assert F.host(L, data, pattern, delim, base) == (len(records), records, matches, True)
    assert F.host(L, data, pattern, delim, base, capacity=0) == (len(records), [], matches, True)
    if records:
        assert F.host(L, data, pattern, delim, base, capacity=len(records) - 1) == (len(records), records[:-1], matches, True)
    assert F.host(L, data, pattern, delim, base, capacity=len(records) + 3)[:3] == (len(records), records, matches)


def test_the_inputs_reach_the_rule():
    """several records, several occurrences a record, overlaps and no occurrence at all are among the inputs"""
    answers = [F.find(*INPUTS[name]) for name in INPUTS]
    assert any(len(r) > 1 for r, _ in answers) and any(m > len(r) > 0 for r, m in answers) and any(m == 0 for _, m in answers)
    assert F.find(b"aaaa", b"aa") == ([0], 3) and F.find(b"x\nyy\nneedl", b"needle") == ([], 0)


def test_windows_cut_where_records_begin_find_what_the_whole_window_finds():
    """the header's claim about windows of an archive, on the CPU: every input of the splitter's tests has its frames cut at the frames f
    with f == 0 or first_record[f] != first_record[f - 1]; the windows between them together give the whole text's answer.  The cut
    record's input has frames on both sides of the rule: some begin a record behind the first, some do not"""
    import _split as S
    both = 0
    for name, (data, delim, T, M) in S.cases().items():
        split = S.Split(data, delim, T, M)
        starts = F.record_starts(split.first_record)
        both += 1 < len(starts) < split.n
        for key in (name, name + "_pair"):
            if key in INPUTS_OF_SPLIT:
                cuts = F.boundary_windows(data, split.sizes, split.first_record, INPUTS_OF_SPLIT[key][1], delim)
                assert [a for a, _ in cuts] == starts
    assert both >= 3


def test_the_host_call_refusals(L):
    out = np.full(4, 7, dtype=np.uint64)
    p = out.ctypes.data_as(ctypes.c_void_p)
    call = lambda *a: F.code(L, L.zsmi_findRecords(*a))
    assert call(b"abc", 3, 10, b"", 0, 0, p, 4, None) == F.E_PARAM                 # patternSize 0
    assert call(b"abc", 3, 10, b"a" * 257, 257, 0, p, 4, None) == F.E_PARAM        # patternSize 257
    assert call(b"abc", 3, 10, b"a\nb", 3, 0, p, 4, None) == F.E_PARAM             # a delimiter inside the pattern
    assert call(b"abc", 3, 256, b"a", 1, 0, p, 4, None) == F.E_PARAM and call(b"abc", 3, -1, b"a", 1, 0, p, 4, None) == F.E_PARAM
    assert call(None, 3, 10, b"a", 1, 0, p, 4, None) == F.E_SRC_SIZE
    assert call(b"abc", 3, 10, None, 1, 0, p, 4, None) == F.E_GENERIC and call(b"abc", 3, 10, b"a", 1, 0, None, 4, None) == F.E_GENERIC
    assert call(None, 3, 300, None, 0, 0, None, 4, None) == F.E_GENERIC            # the order: NULL arrays, then the ranges, then the source
    assert call(None, 3, 300, b"a", 1, 0, p, 4, None) == F.E_PARAM
    assert out.tolist() == [7] * 4
    assert L.zsmi_findRecords(b"a" * 256, 256, 10, b"a" * 256, 256, 0, p, 4, None) == 1 and int(out[0]) == 0      # 256 is in range


def test_the_python_call(L):
    import zstandard_amd
    for name in ("overlaps_in_lines", "delim_255", "lines_common", "empty"):
        data, pattern, delim, base = INPUTS[name]
        assert zstandard_amd.find_records(data, pattern, bytes([delim]), base) == F.find(data, pattern, delim, base)[0], name
    with pytest.raises(RuntimeError):
        zstandard_amd.find_records(b"abc", b"")


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="the sanitizer build is a CPU-side check: it runs on machines without a GPU, never next to one")
def test_the_rule_under_sanitizers(tmp_path):
    """the header alone, host code only, with -fsanitize=address,undefined: the text, the pattern and the arrays in heap blocks of exactly
    their sizes"""
    exe = str(tmp_path / "find_records")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, os.path.join(ROOT, "tests", "c", "find_records.cpp"), "-o", exe])
    args, names = [], sorted(INPUTS)
    for i, name in enumerate(names):
        data, pattern, delim, base = INPUTS[name]
        open(str(tmp_path / ("t%d" % i)), "wb").write(data)
        open(str(tmp_path / ("p%d" % i)), "wb").write(pattern)
        args += [str(tmp_path / ("t%d" % i)), str(tmp_path / ("p%d" % i)), str(delim), str(base)]
    out = subprocess.run([exe] + args, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-4000:]
    rows = out.stdout.splitlines()
    assert len(rows) == len(names)
    for name, row in zip(names, rows):
        records, matches = F.find(*INPUTS[name])
        assert [int(v) for v in row.split()] == [len(records), matches] + records, name
