"""zsmi_finalizeDictionary against the oracle's scalar finalize (zso_finalizeDictionary, oracle/zso_encoder.c), byte for byte: the dictionary,
or the same error code with the destination untouched.  The cases and what each exercises: tests/_dictfin.py (FINALIZE); that each reaches
its border is shown without a GPU by tests/test_dict_finalize_host.py.  Where the two differ the arbiter is, for compressed blocks, oracle
D's counters of the frames (test_encoder_counters_equal_decoder_counters) and, for blocks whose frames hide the parse, the rule in the
comment above k_train_stats.

Not held here: the halving of the LL / OF / ML counts at 2^30 (no test can count a billion sequences) and the retry of the Huffman
description with flatter codes (case h: no literal distribution found that needs it; tests/test_dict_finalize_host.py has the search)."""
import ctypes, os
import pytest
import _train as T
import _batch as B
import _dictfin as F

pytestmark = pytest.mark.gpu


def L():
    from zstandard_amd import _lib
    return _lib.lib()


def gpu_finalize(content, parts, cap, level, dict_id):
    """the dictionary, or the error's code (the destination checked untouched)"""
    buf, sizes = T.flat(parts)
    out = ctypes.create_string_buffer(b"\xAA" * cap, cap)
    r = L().zsmi_finalizeDictionary(out, cap, content, len(content), buf, sizes, len(parts), level, dict_id)
    if L().zsmi_isError(r):
        assert out.raw == b"\xAA" * cap
        return int(L().zsmi_getErrorCode(r))
    assert out.raw[r:] == b"\xAA" * (cap - r)
    return out.raw[:r]


def explain(got, want):
    if isinstance(got, int) or isinstance(want, int):
        return f"GPU {got if isinstance(got, int) else len(got)} oracle {want if isinstance(want, int) else len(want)} (an int: the error code)"
    at = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
    return f"sizes {len(got)} / {len(want)}, first difference at byte {at}: {got[at:at + 16].hex()} / {want[at:at + 16].hex()}"


@pytest.mark.parametrize("case", sorted(F.FINALIZE))
def test_finalize_equals_oracle(case):
    want = F.outcome(case)
    got = gpu_finalize(*F.FINALIZE[case]())
    assert got == want, explain(got, want)


def test_hidden_parses_twice_on_one_context():
    """blocks whose frames hide their parse (raw, RLE, no sequences, 20 bytes), each behind a sample with many sequences, then the same
    samples in reverse order through the same scratch: no header or code bytes of the call before are counted"""
    for case in ("f_hidden_parses", "f_hidden_parses_reversed", "f_hidden_parses"):
        got = gpu_finalize(*F.FINALIZE[case]())
        assert got == F.outcome(case), (case, explain(got, F.outcome(case)))


_SUB_CHILD = r'''
import sys, os
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import _dictfin as F
from zstandard_amd import finalize_dictionary
content, parts, cap, level, did = F.FINALIZE[sys.argv[2]]()
assert len(parts) > 64                                                   # more blocks than one sub-batch takes
sys.stdout.write("DICT " + finalize_dictionary(content, parts, cap, level, did).hex() + "\n")
'''


def test_counters_add_up_over_sub_batches():
    case = "a_json_records_cap65536_l3"
    env = dict(os.environ, ZSMI_BLOCKS_IN_FLIGHT="64")
    got = bytes.fromhex(B.run_child("-c", _SUB_CHILD, B.ROOT, case, env=env, marker="DICT ").split("DICT ")[1].strip())
    assert got == F.outcome(case), explain(got, F.outcome(case))
