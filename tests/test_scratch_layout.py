"""The scratch layouts (zstandard_amd/csrc/zsmi_scratch.h) as the debug-hook library reports them: bytes a slot and fixed bytes of every
buffer a tool can name.  No GPU: zsmi_dbg_scratchLayout is host code.  The numbers are written out here, from the size expressions of
Scratch::reserve and DecodeScratch::each as they stood before the header existed - a layout change has to say so in this file."""
import ctypes, os, subprocess, sys
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# buffer -> (bytes a slot, fixed bytes).  compress: a slot is a 64 KiB block of the sub-batch
COMPRESS = {
    "dist":    (65536 * 2, 256),                  # cap * ZS_BLOCK_MAX * 2 + 256
    "distHi":  (65536 // 8, 256),                 # cap * (ZS_BLOCK_MAX / 8) + 256
    "cand":    (2 * 4, 64),                       # cap * 2 * sizeof(uint32_t) + 64
    "recs":    (65536 // 4 * 8, 64 * 8),          # (cap * (ZS_BLOCK_MAX / 4) + 64) * sizeof(uint2)
    "res":     (256 * 16, 8 << 20),               # cap * ZS_RES_PER_BLOCK * sizeof(uint4) + 8 MiB
    "seqs":    (64 * 256 * 8, 0),                 # cap * ZS_WALK_RANGES * ZS_SEQ_PER_RANGE * sizeof(ZsSeqRec)
    "hdrs":    (64 * 16, 0),                      # cap * ZS_WALK_RANGES * sizeof(ZsRangeHdr)
    "lits":    (65536 + 64, 0),                   # cap * (ZS_BLOCK_MAX + 64)
    "streams": (4 * 24 * 1024, 0),                # cap * 4 * ZS_STREAM_STRIDE
    "litSec":  (65536 + 1024, 0),                 # cap * ZS_LITSEC_STRIDE
    "seqSec":  (65536 + 4096, 0),                 # cap * ZS_SEQSEC_STRIDE
    "metas":   (8 * 4, 0),                        # cap * sizeof(ZsBlockMeta): eight words
}
# decode: poolLit a wavefront of the general kernel's pool; hufTabs, seqTabs a block slot of the fast path
DECODE = {
    "poolLit": ((1 << 17) + 64, 0),               # pool * ZS_DEC_LITBUF
    "hufTabs": (2 << 11, 0),                      # slots * ZS_FAST_HUFTAB_BYTES
    "seqTabs": ((512 + 256 + 512) * 2, 0),        # slots * ZS_FAST_SEQTAB_BYTES
}


@pytest.fixture(scope="module")
def hooks():
    # the library __graft_entry__.build() makes with -DZSMI_DEBUG_HOOKS (made here if it is missing or stale; loaded beside the product
    # library, which this process may hold already)
    env = dict(os.environ, ZSMI_DEBUG_LIB="1")
    path = subprocess.check_output([sys.executable, "-c", "from zstandard_amd import _lib; print(_lib.build())"], env=env, cwd=ROOT, text=True).strip().splitlines()[-1]
    so = ctypes.CDLL(path)
    so.zsmi_dbg_scratchLayout.restype = ctypes.c_int
    so.zsmi_dbg_scratchLayout.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint64)]
    so.zsmi_dbg_descLayout.restype = None
    return so


def layout(so, name):
    out = (ctypes.c_uint64 * 2)(~0, ~0)
    rc = so.zsmi_dbg_scratchLayout(name.encode(), out)
    return rc, int(out[0]), int(out[1])


@pytest.mark.parametrize("name", sorted(COMPRESS) + sorted(DECODE))
def test_slot_and_fixed_bytes(hooks, name):
    assert layout(hooks, name) == (0,) + {**COMPRESS, **DECODE}[name]


def test_the_table_holds_twelve_compress_buffers():
    assert len(COMPRESS) == 12


def test_descriptor_slot_is_the_descriptor(hooks):
    words = (ctypes.c_uint32 * 6)()
    hooks.zsmi_dbg_descLayout(words)
    assert layout(hooks, "fastDesc") == (0, 4 * int(words[0]), 0)


@pytest.mark.parametrize("name", ["", "nope", "Dist", "dist ", "dDist", "litScratch", "seqOut", "seqLists", "3"])
def test_unknown_name_is_refused(hooks, name):
    # (the buffers whose stride a call's plan chooses are not exported either)
    rc, a, b = layout(hooks, name)
    assert rc != 0 and (a, b) == ((1 << 64) - 1, (1 << 64) - 1)
