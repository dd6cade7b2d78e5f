"""Device-resident compress, the part that needs no device: the two calls refuse a NULL context, and the per-chunk rule both plans apply
(csrc/zsmi_plan.h: CompressPlan::build on the host, k_plan_chunks / k_plan_blocks on the device) compiled ALONE into a host program
(tests/c/plan_rule.cpp) against the same rule in a few lines of Python."""
import os, subprocess
import pytest
from zstandard_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCK, UNIT = 1 << 16, 1 << 17
SIZES = [0, 1, 65535, 65536, 65537, 131072, 131073, 196608, 196609, 262144, 0xFFFFFFFF]


def counts(size):
    """(blocks, small units, big units): an empty chunk is one block and no unit; a unit per 128 KiB; a unit with more than 64 KiB left is big"""
    blocks = max(1, -(-size // BLOCK))
    lefts = [size - o for o in range(0, size, UNIT)]
    big = sum(left > BLOCK for left in lefts)
    return blocks, len(lefts) - big, big


@pytest.fixture(scope="module")
def rule(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plan_rule") / "plan_rule")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "zstandard_amd", "csrc"),
                           os.path.join(ROOT, "tests", "c", "plan_rule.cpp"), "-o", exe])
    out = subprocess.run([exe] + [str(s) for s in SIZES], capture_output=True, text=True, timeout=60, check=True).stdout
    got, cur = {}, None
    for line in out.splitlines():
        f = line.split()
        if f[0] in "BU":
            got[cur][f[0]].append(tuple(int(v) for v in f[1:]))
        else:
            cur = int(f[0]); got[cur] = {"counts": tuple(int(v) for v in f[1:]), "B": [], "U": []}
    return got


def test_null_context():
    _lib.build()
    L = _lib.lib()
    assert L.zsmi_compressBoundsDevice(None, None, 1, None) == 62
    assert L.zsmi_compressBatchResident(None, None, None, None, 1, 65536, None, None, None, 3) == 62
    assert L.zsmi_compressBoundsDevice(None, None, 0, None) == 62 and L.zsmi_compressBatchResident(None, None, None, None, 0, 0, None, None, None, 3) == 62


def test_counts_of_the_edge_sizes(rule):
    assert sorted(rule) == sorted(SIZES)
    for s in SIZES:
        assert rule[s]["counts"] == counts(s), s
    # spelled out, so that the Python above is held to something too
    assert [rule[s]["counts"] for s in SIZES] == [(1, 0, 0), (1, 1, 0), (1, 1, 0), (1, 1, 0), (2, 0, 1), (2, 0, 1), (3, 1, 1), (3, 1, 1), (4, 0, 2),
                                                  (4, 0, 2), (65536, 0, 32768)]


def test_blocks_and_units_of_the_edge_sizes(rule):
    for s in SIZES[:-1]:
        blocks, small, big = counts(s)
        want_b = [(k, k * BLOCK, min(BLOCK, s - k * BLOCK), int(k == 0), int(k + 1 == blocks)) for k in range(blocks)]
        assert rule[s]["B"] == want_b, s
        want_u, bigs = [], 0
        for u, o in enumerate(range(0, s, UNIT)):
            left = s - o
            is_big = left > BLOCK
            want_u.append((u, o, min(UNIT, left), 2 * u, int(is_big), bigs if is_big else 0))      # at: its place among the chunk's units of its kind
            bigs += is_big
        assert rule[s]["U"] == want_u, s
        assert sum(b[2] for b in want_b) == s == sum(u[2] for u in want_u)
