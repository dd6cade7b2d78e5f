#!/usr/bin/env python3
"""Development aid (GPU box; library built with -DZSMI_DEBUG_HOOKS -DZS_PREP_PROFILE, named by ZSMI_LIB_FILE): s_memtime ticks per phase of
k_dec_prep, averaged over the frames of a decode call."""
import sys, os, ctypes
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import _data as D, _batch as B
from zstandard_amd import BatchCodec, _lib
n, cs = 8192, 32768
host = D.zipf_log(n * cs)
bc = BatchCodec(0); Z = _lib.lib()
offs = np.arange(n, dtype=np.uint64) * cs; sizes = np.full(n, cs, dtype=np.uint32)
arena, do, dsz = bc.compress_host(host, offs, sizes, 3)
frames = np.concatenate([arena[int(do[i]):int(do[i]) + int(dsz[i])] for i in range(n)])
fo = B.layout(dsz)
out, oo, osz = bc.decompress_host(frames, fo, dsz, sizes)
assert (osz == cs).all()
names = ["headers up to the Huffman description", "huf: stage the description", "huf: weight counts (readNCount)", "huf: weight FSE table", "huf: weights (two FSE states)",
         "huf: ranks, start cells", "huf: table fill", "seq: between tables", "seq: stage a description", "seq: parse (readNCount)", "seq: build", "seq: emit 16-bit cells", "whole wavefront"]
# the items' block-0 Huffman table slots (one-block frames: slot = item); the stamps, a word a name, start at the middle of a slot
# (zs_huftab_lend_prep_profile, csrc/zsmi_scratch.h)
tabs = _lib.copy_scratch(bc.ctx, "hufTabs", n).reshape(n, -1)
half = tabs.shape[1] // 2
prof = np.ascontiguousarray(tabs[:, half:half + 8 * len(names)]).view(np.uint64).astype(np.float64)
m = prof.mean(axis=0)
for k, nm in enumerate(names):
    print(f"{nm:40s} {m[k]:10.0f} ticks  {100 * m[k] / m[12]:5.1f} %")
print("whole item = %.0f s_memtime ticks (shader-clock cycles on this part: k_dec_prep at 163 K ticks an item and 16 items a CU at a time is its measured 0.97 ms per 57344 frames at ~2.4 GHz)" % m[12])
