"""No call's result depends on what the context's scratch, or the caller's output buffer, held before it.

A zsmi_ctx keeps about sixty device buffers from call to call and the host clears a handful of words of them; everything else is
"written before it is read" ("What a context's memory may carry from call to call").  Here that is tested: each call family runs
in a child process of its own (tests/_poison.py, the debug-hook library) on fresh scratch, behind a fill of ALL the context's memory with
0x00, with 0xFF and with a seeded mix of small and large words (zsmi_dbg_fillScratch), behind a hostile predecessor, and into output
buffers prefilled with 0x00 and 0xFF - and every one of those runs is compared in full with the family's independent reference (oracle E
byte for byte, oracle D item by item), never with another run.  If the library is right every poisoned run is an ordinary run.

Not held here: zsmi_finalizeDictionary alone - it runs on a pooled context the hook cannot reach; the trainer's own finalize step is
covered through zsmi_trainFromDevice.

Each child has a time limit of its own: LIMITS, beside the time the child took on an MI355X when the limit was set.  A child that ends by
its limit or by a signal has faulted or hung the device: the module remembers it and every later test fails at once, without starting
another process on the GPU."""
import json, os, subprocess, time
import pytest
import _batch as B
import _poison as P

pytestmark = pytest.mark.gpu

# family -> (time limit of its child in seconds, seconds the child took when the limit was set - imports, oracles and all; the slowest of
# three runs).  The limits are ten to twenty times that: room for a busy machine, while a hung child holds the GPU for half a minute at
# most; they are not sized for a child that has to build the library first.  The two decode children move 363 items of 1 MiB capacity
# through host and device buffers some forty times each: that, not the kernels, is their time
LIMITS = {
    "compress": (30, 1.4),
    "compress_sub_batches": (30, 2.7),
    "compress_dict": (30, 1.4),
    "resident": (30, 1.8),
    "decode": (60, 8.0),
    "decode_general": (60, 7.8),
    "seekable": (30, 1.5),
    "training": (30, 1.9),
    "one_shot": (30, 2.2),
}
_ended_badly = []


@pytest.fixture(autouse=True)
def no_child_after_a_fault():
    if _ended_badly:
        pytest.fail("not started: an earlier child of this module ended by %s" % (_ended_badly[0],), pytrace=False)


def run_family(family, capsys):
    env = dict(os.environ, **P.ENVIRONMENT.get(family, {}))
    if family == "one_shot":
        env.pop("ZSMI_DEBUG_LIB", None)                    # the product library: no hook
    else:
        env["ZSMI_DEBUG_LIB"] = "1"
    t0 = time.time()
    try:
        out = B.run_child(os.path.join(B.ROOT, "tests", "_poison.py"), family, env=env, cwd=B.ROOT, timeout=LIMITS[family][0])
    except subprocess.TimeoutExpired:
        _ended_badly.append("its time limit (%s, %d s)" % (family, LIMITS[family][0]))
        raise
    except B.ChildFailed as e:
        if e.returncode < 0:
            _ended_badly.append("signal %d (%s)" % (-e.returncode, family))
        raise
    report = json.loads(out.strip().splitlines()[-2])
    assert report["family"] == family and report["cases"]
    with capsys.disabled():
        print("\n[scratch independence] %s: %d cases, child %.1f s of which %.1f s in its calls and references (limit %d s)"
              % (family, len(report["cases"]), time.time() - t0, report["seconds"], LIMITS[family][0]))
    return report


def test_compress_host_arrays(capsys):
    """levels 1, 3 and 4; the batch as listed, reversed and rotated by three; oracle E byte for byte"""
    rep = run_family("compress", capsys)
    assert len(rep["cases"]) == 9


def test_compress_three_sub_batches(capsys):
    """ZSMI_BLOCKS_IN_FLIGHT=64 and enough copies of the batch for three sub-batches: slots are reused inside one call"""
    rep = run_family("compress_sub_batches", capsys)
    assert len(rep["cases"]) == 9


def test_compress_with_dictionaries(capsys):
    """_usingDict raw and formatted, _usingCDict, a CDict set of formatted, raw, empty and NO_DICT choices, the checksum flag"""
    rep = run_family("compress_dict", capsys)
    assert len(rep["cases"]) == 6 + 3 * 3 + 2


def test_resident_compress(capsys):
    """bounds -> layout -> compress_resident, plainly and with a CDict set; chunks above maxSrcSize are refused in place"""
    rep = run_family("resident", capsys)
    assert len(rep["cases"]) == 9 + 1 + 1


def test_decode(capsys):
    """the edge catalogue at exact and at 1 MiB capacities, host arrays and resident; dictionary frames through a DDict set"""
    rep = run_family("decode", capsys)
    assert len(rep["cases"]) == 5


def test_decode_general_kernel_only(capsys):
    """the same with ZSMI_DEC_FAST=0"""
    rep = run_family("decode_general", capsys)
    assert len(rep["cases"]) == 5


def test_seekable_write_ranges_and_split(capsys):
    """the fixed-size archive write, open + a batch of ranges, a record archive written with a CDict set and read back by frame number
    with a dictionary (host arrays and resident), zsmi_openFramesDevice on a stream with skippable frames and on junk magics, records by
    number with followers and a refused request, find in a text across tile borders - literal and by regular expression - and in windows of an archive,
    zsmi_splitRecordsDevice at targetSize 0 and 4096 with a record above maxFrameSize - each against its Python statement"""
    rep = run_family("seekable", capsys)
    assert len(rep["cases"]) == 2 + 1 + 2 + 2 + 7


def test_dictionary_training(capsys):
    """zsmi_trainFromDevice, the short_samples case: the content against the scalar model, the header against check_format and the
    fresh-scratch run (the weaker part: tests/_poison.py says why)"""
    rep = run_family("training", capsys)
    assert len(rep["cases"]) == 1


def test_one_shot_pool(capsys):
    """the product library: one pooled context serves 1 MiB of noise, 200 bytes, a frame that fails midway, sequences/of_rep_second, a
    dictionary call and the same chunk without"""
    run_family("one_shot", capsys)
