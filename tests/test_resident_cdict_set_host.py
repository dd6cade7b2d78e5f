"""Device-resident compress with a CDict set, the part that needs no device: the dictionary rule both plans apply (csrc/zsmi_plan.h:
zs_chunk_prefixed / zs_chunk_counts_dict - CompressPlan::build on the host, k_plan_chunks / k_plan_blocks on the device) compiled ALONE
into a host program (tests/c/plan_dict_rule.cpp) against the rule in a few lines of Python; the new entry point declared, exported and
bound; and the one host check that needs no device."""
import ctypes, os, re, subprocess
import pytest
from zstandard_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCK, UNIT = 1 << 16, 1 << 17
SIZES = [0, 1, 65535, 65536, 65537, 131072, 131073, 196608, 196609, 1 << 20]
NAME = "zsmi_compressBatchResident_usingCDictSet"


def counts(size, has_dict):
    """(blocks, prefixed, small, big).  DESIGN.md, "Dictionary prefix": a chunk of 1 .. 64 KiB with a dictionary is one prefixed unit; every
    other unit with at most 64 KiB left is a small (tail) unit; a unit with more left is big"""
    blocks = max(1, -(-size // BLOCK))
    lefts = [size - o for o in range(0, size, UNIT)]
    big = sum(left > BLOCK for left in lefts)
    small = len(lefts) - big
    pfx = 1 if has_dict and 1 <= size <= BLOCK else 0
    return blocks, pfx, small - pfx, big


@pytest.fixture(scope="module")
def rule(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plan_dict_rule") / "plan_dict_rule")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "zstandard_amd", "csrc"),
                           os.path.join(ROOT, "tests", "c", "plan_dict_rule.cpp"), "-o", exe])
    out = subprocess.run([exe] + [str(s) for s in SIZES], capture_output=True, text=True, timeout=60, check=True).stdout
    got = {}
    for line in out.splitlines():
        left, right = line.split("|")
        f = [int(v) for v in left.split()]
        got[(f[0], bool(f[1]))] = {"counts": tuple(f[2:6]), "prefixed": bool(f[6]), "plain": tuple(int(v) for v in right.split())}
    return got


def test_counts_with_and_without_a_dictionary(rule):
    assert sorted(rule) == sorted((s, d) for s in SIZES for d in (False, True))
    for (s, d), r in rule.items():
        assert r["counts"] == counts(s, d), (s, d)
    # spelled out, so that the Python above is held to something too: (blocks, prefixed, small, big)
    assert [rule[(s, True)]["counts"] for s in SIZES] == [(1, 0, 0, 0), (1, 1, 0, 0), (1, 1, 0, 0), (1, 1, 0, 0), (2, 0, 0, 1), (2, 0, 0, 1),
                                                          (3, 0, 1, 1), (3, 0, 1, 1), (4, 0, 0, 2), (16, 0, 0, 8)]
    assert [rule[(s, False)]["counts"] for s in SIZES] == [(1, 0, 0, 0), (1, 0, 1, 0), (1, 0, 1, 0), (1, 0, 1, 0), (2, 0, 0, 1), (2, 0, 0, 1),
                                                           (3, 0, 1, 1), (3, 0, 1, 1), (4, 0, 0, 2), (16, 0, 0, 8)]


def test_a_last_unit_of_one_block_is_prefixed_or_small_never_both(rule):
    for (s, d), r in rule.items():
        blocks, pfx, small, big = r["counts"]
        last_is_one_block = s > 0 and (s - 1) % UNIT < BLOCK              # the last unit holds at most 64 KiB
        assert pfx + small == (1 if last_is_one_block else 0), (s, d)
        assert r["prefixed"] == (pfx == 1), (s, d)
        assert pfx == 0 or (d and s <= BLOCK), (s, d)                      # prefixed: a dictionary, and the chunk is the unit
        assert pfx + small + big == -(-s // UNIT), (s, d)                  # every unit is in exactly one list


def test_without_a_dictionary_it_is_the_plain_rule(rule):
    for s in SIZES:
        blocks, pfx, small, big = rule[(s, False)]["counts"]
        assert pfx == 0 and (blocks, small, big) == rule[(s, False)]["plain"], s
        # with one: the blocks and big units stay, and the small unit moves or stays
        b1, p1, s1, g1 = rule[(s, True)]["counts"]
        assert (b1, p1 + s1, g1) == rule[(s, True)]["plain"], s


def test_declared_exported_and_bound():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "zsmi.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+" + NAME + r"\s*\(([^;]*)\)\s*;", hdr)
    assert m, "not declared in include/zsmi.h"
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 11 and args[0].startswith("zsmi_ctx") and "zsmi_cdictSet" in args[9] and args[10].startswith("const uint32_t")
    assert NAME in _lib.EXPORTS
    so = ctypes.CDLL(_lib.build())
    assert hasattr(so, NAME)
    L = _lib.lib()
    assert len(getattr(L, NAME).argtypes) == 11 and ctypes.sizeof(getattr(L, NAME).restype) == 4


def test_null_context():
    _lib.build()
    L = _lib.lib()
    call = getattr(L, NAME)
    assert call(None, None, None, None, 1, 65536, None, None, None, None, None) == 62           # init_missing before anything else
    assert call(None, None, None, None, 0, 0, None, None, None, None, None) == 62
