"""Records by number, what holds without a device: the three names in the header, _lib.EXPORTS, the library and the Python classes; the
first host check (a NULL ctx is refused in front of every later refusal; the order behind it needs a context and is
tests/test_gpu_read_records.py's); the work bound of no handle; and the two rules of csrc/zsmi_records.h, compiled ALONE into a host
program (tests/c/read_records.cpp) under the address and undefined-behaviour sanitizers, over every input of tests/_split.py and every
record of each, against the Python statement of the splitter's rule: the frame is frame_of's, the bytes are the text's slice."""
import ctypes, os, re, subprocess
import pytest
import _split as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zstandard_amd", "csrc")
NAMES = ("zsmi_seekableRecordsWorkBound", "zsmi_seekableReadRecordsResident", "zsmi_seekableReadRecordsHost")
CASES = S.cases()


@pytest.fixture(scope="module")
def L():
    from zstandard_amd import _lib
    _lib.build()
    return _lib.lib()


def test_names(L):
    from zstandard_amd import _lib, api
    hdr = open(os.path.join(ROOT, "include", "zsmi.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    so = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in _lib.EXPORTS and hasattr(so, name), name
    for name in ("read_records_resident", "records_work_bound"):
        assert hasattr(api.SeekableHandle, name), name
    assert hasattr(api.SeekableArchive, "read_records")
    assert os.path.exists(os.path.join(CSRC, "zsmi_records.h"))


def test_a_null_ctx_is_refused_first(L):
    """init_missing with every later refusal present too: NULL arrays, a delimiter, an alignment and a read count out of range"""
    one = ctypes.c_void_p(8)                                                      # a non-NULL pointer no refused call looks behind
    assert L.zsmi_seekableReadRecordsResident(None, None, None, 3, 256, None, 5, 0xFFFFFFFF, 3, None, 10, None, 10, None, None, None, None) == S.E_INIT
    assert L.zsmi_seekableReadRecordsResident(None, one, one, 3, 10, one, 5, 5, 1, one, 10, one, 10, one, one, one, one) == S.E_INIT
    assert L.zsmi_seekableReadRecordsHost(None, None, None, 3, -1, None, 5, None, 10, None, None) == S.E_INIT
    assert L.zsmi_seekableReadRecordsHost(None, one, one, 3, 10, one, 5, one, 10, one, one) == S.E_INIT
    assert L.zsmi_seekableRecordsWorkBound(None, 7) == 0


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="the sanitizer build is a CPU-side check: it runs on machines without a GPU, never next to one")
def test_the_two_rules_under_sanitizers(tmp_path):
    """the header alone, host code only, with -fsanitize=address,undefined: firstRecord, the content offsets and every record's run in heap
    blocks of exactly their sizes"""
    exe = str(tmp_path / "read_records")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, os.path.join(ROOT, "tests", "c", "read_records.cpp"), "-o", exe])
    args, names = [], sorted(CASES)
    for name in names:
        data, delim, T, M = CASES[name]
        open(str(tmp_path / name), "wb").write(data)
        args += [str(tmp_path / name), str(delim), str(T), str(M)]
    out = subprocess.run([exe] + args, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-4000:]
    rows = out.stdout.splitlines()
    assert len(rows) == len(names)
    cut = 0
    for name, row in zip(names, rows):
        data, delim, T, M = CASES[name]
        want = S.Split(data, delim, T, M)
        ends = S.record_ends(data, delim)[1]
        words = row.split()
        assert words[:2] == [str(want.records), str(want.n)] and len(words) == 2 + want.records, name
        for r, word in enumerate(words[2:]):
            f, g, start, end = (int(v) for v in word.split(","))
            assert f == want.frame_of(r), (name, r)
            assert f <= g < want.n and (start, end) == (ends[r - 1] if r else 0, ends[r]), (name, r, word)
            assert sum(want.sizes[:f]) <= start and end <= sum(want.sizes[:g + 1]), (name, r)
            cut += f < g
    assert cut >= 6                                                                # (the no_delimiter_* inputs and the cut record: f < g is on the path)
