"""The record splitter on the host (no GPU): zsmi_splitRecords against the Python statement of its rule (tests/_split.py: a loop over
bytes.find) on empty and one-byte inputs, delimiters only, no delimiter at all, tails, T of 0, 1 and M, long pieces between short ones, a
cut record whose last piece shares a frame, seeded lines and the delimiters 0 and 255; the count-only form and the capacities n and
n - 1; every refusal in the header's order; the names; the Python surface.  The rule's loop also runs alone, in a host program under the
address and undefined-behaviour sanitizers (tests/c/split_records.cpp)."""
import ctypes, os, re, subprocess
import numpy as np
import pytest
import _split as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zstandard_amd", "csrc")
CASES = S.cases()


@pytest.fixture(scope="module")
def L():
    from zstandard_amd import _lib
    _lib.build()
    return _lib.lib()


def test_the_restatement_on_inputs_worked_by_hand():
    """the yardstick itself, where the answer can be written down"""
    s = S.Split(b"ab\ncd\nef", 10, 0)
    assert (s.sizes, s.first_record, s.records, s.pieces) == ([3, 3, 2], [0, 1, 2, 3], 3, 3)
    s = S.Split(b"x\n" + b"y" * 24 + b"\nz\nw\n" + b"tail", 10, 10, 10)            # pieces end at 2; 12, 22, 27; 29; 31; 35
    assert (s.sizes, s.first_record, s.records, s.pieces) == ([2, 10, 10, 9, 4], [0, 1, 1, 1, 4, 5], 5, 7)
    assert [s.frame_of(r) for r in range(5)] == [0, 1, 3, 3, 4]                    # the cut record starts frame 1; z and w start inside frame 3
    s = S.Split(b"a" * 3001, 10, 0, 1000)
    assert (s.sizes, s.first_record, s.records) == ([1000, 1000, 1000, 1], [0, 0, 0, 0, 1], 1)
    s = S.Split(b"a\nbb\n" + b"c" * 40 + b"\nd\nee\n", 10, 8, 100)
    assert s.sizes == [5, 41, 5] and s.first_record == [0, 2, 3, 5]
    assert S.Split(b"", 10, 5, 9).first_record == [0] and S.Split(b"\n" * 5000, 10, 7).sizes == [7] * 714 + [2]


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_host_call_is_the_restatement(L, name):
    data, delim, T, M = CASES[name]
    want = S.Split(data, delim, T, M)
    n, sizes, first, records, intact = S.host(L, data, delim, T, M)
    assert intact and (n, records) == (want.n, want.records)
    assert sizes == want.sizes and first == want.first_record
    assert want.pieces <= want.records + len(data) // M                           # rule 2's bound, which sizes the device call


@pytest.mark.parametrize("name", ["random_T1000", "cut_record_shares_its_last_piece", "all_delimiters_5000", "one_other_byte"])
def test_count_only_and_capacity(L, name):
    data, delim, T, M = CASES[name]
    want = S.Split(data, delim, T, M)
    records = ctypes.c_uint64(77)
    assert L.zsmi_splitRecords(data, len(data), delim, T, M, None, None, 0, ctypes.byref(records)) == want.n and records.value == want.records
    assert L.zsmi_splitRecords(data, len(data), delim, T, M, None, None, 0, None) == want.n
    n, sizes, first, records, intact = S.host(L, data, delim, T, M, capacity=want.n)          # exactly n
    assert intact and (n, sizes, first) == (want.n, want.sizes, want.first_record)
    sizes_only = np.full(want.n + 1, 7, dtype=np.uint32)                                      # firstRecord NULL
    assert L.zsmi_splitRecords(data, len(data), delim, T, M, sizes_only.ctypes.data_as(ctypes.c_void_p), None, want.n, None) == want.n
    assert sizes_only.tolist() == want.sizes + [7]
    n, sizes, first, _, intact = S.host(L, data, delim, T, M, capacity=want.n - 1)            # one short: nothing behind capacity is written
    assert n == -S.E_TOO_SMALL and intact
    n, _, _, _, intact = S.host(L, data, delim, T, M, capacity=0)
    assert n == -S.E_TOO_SMALL and intact


def test_refusals_in_order(L):
    """each refusal with every later one present too, so that the order shows"""
    def split(src, size, delim, T, M):
        out = np.zeros(8, dtype=np.uint32)
        return -S.code(L, L.zsmi_splitRecords(src, size, delim, T, M, out.ctypes.data_as(ctypes.c_void_p), None, 0, None))
    GiB = 1 << 30
    assert split(None, 5, -1, 9, 0) == -S.E_PARAM and split(None, 5, 256, 9, 0) == -S.E_PARAM                 # delim
    assert split(None, 5, 10, 9, 0) == -S.E_PARAM and split(None, 5, 10, 0, GiB + 1) == -S.E_PARAM            # maxFrameSize
    assert split(None, 5, 10, 9, 8) == -S.E_PARAM                                                             # targetSize > maxFrameSize
    assert split(None, 5, 10, 8, 8) == -S.E_SRC_SIZE and split(None, 5, 10, GiB, GiB) == -S.E_SRC_SIZE        # a NULL source that states bytes
    assert split(None, 0, 10, 8, 8) == 0 and split(b"abc", 3, 10, 8, 8) == -S.E_TOO_SMALL                     # (capacity 0)
    p = ctypes.c_void_p
    one = p(8)                                                                    # a non-NULL pointer no refused call looks behind
    # the device calls: a NULL ctx in front of everything; the later checks need a context and are tests/test_gpu_split_records.py's
    assert L.zsmi_countRecordsDevice(None, None, 5, 999, None) == S.E_INIT
    assert L.zsmi_splitRecordsDevice(None, None, 5, 999, 9, 0, 0xFFFFFFFF, None, None, None) == S.E_INIT
    assert L.zsmi_splitRecordsDevice(None, one, 5, 10, 0, 64, 16, one, one, one) == S.E_INIT


def test_names(L):
    from zstandard_amd import _lib, api
    hdr = open(os.path.join(ROOT, "include", "zsmi.h")).read()
    so = ctypes.CDLL(_lib.LIB_PATH)
    for name in S.NAMES:
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in _lib.EXPORTS and hasattr(so, name), name
    for name in ("count_records_device", "split_records_device", "split_pieces_bound"):
        assert hasattr(api.BatchCodec, name), name
    assert api.BatchCodec.split_pieces_bound(10, 1000, 64) == 25


def test_python_surface(L):
    from zstandard_amd import api
    for name in ("random_T1000", "cut_record_shares_its_last_piece", "empty", "delim_255"):
        data, delim, T, M = CASES[name]
        want = S.Split(data, delim, T, M)
        sizes, first = api.split_records(data, bytes([delim]), T, M)
        assert sizes.dtype == np.uint32 and first.dtype == np.uint64
        assert sizes.tolist() == want.sizes and first.tolist() == want.first_record
        for r in range(want.records):                                             # the lookup as the docstring states it
            i = int(np.searchsorted(first, r))
            assert (i if first[i] == r else i - 1) == want.frame_of(r)
    sizes, first = api.split_records(b"a\nb\n")
    assert sizes.tolist() == [2, 2] and first.tolist() == [0, 1, 2]
    with pytest.raises(RuntimeError):
        api.split_records(b"abc", b"\n", 9, 8)
    with pytest.raises(ValueError):
        api.split_records(b"abc", b"\r\n")


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="the sanitizer build is a CPU-side check: it runs on machines without a GPU, never next to one")
def test_the_rule_loop_under_sanitizers(L, tmp_path):
    """the header alone, host code only, with -fsanitize=address,undefined: every input and every output in a heap block of exactly its size"""
    exe = str(tmp_path / "split_records")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, os.path.join(ROOT, "tests", "c", "split_records.cpp"), "-o", exe])
    args, names = [], sorted(CASES)
    for name in names:
        data, delim, T, M = CASES[name]
        open(str(tmp_path / name), "wb").write(data)
        args += [str(tmp_path / name), str(delim), str(T), str(M)]
    args += [str(tmp_path / "empty"), "256", "0", "64", str(tmp_path / "T0"), "10", "65", "64"]          # two refusals
    out = subprocess.run([exe] + args, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-4000:]
    rows = out.stdout.splitlines()
    assert len(rows) == len(names) + 2
    for name, row in zip(names, rows):
        data, delim, T, M = CASES[name]
        want = S.Split(data, delim, T, M)
        join = lambda v: ",".join(str(x) for x in v) or "-"
        assert row.split() == [str(want.n), str(want.records), join(want.sizes), join(want.first_record), str(want.n), str(-S.E_TOO_SMALL) if want.n else "-"], name
    assert rows[-2].split() == rows[-1].split() == [str(-S.E_PARAM), "0", "-", "-", str(-S.E_PARAM), "-"]
