#!/usr/bin/env python3
"""Development aid (GPU box): cycles per phase of the general decode kernel (k_decode_frames), averaged over the last frame of each wavefront of
its pool.  Needs a library built with -DZSMI_DEBUG_HOOKS -DZS_DEC_PROFILE (tools/build_variants.sh decprof:"-DZSMI_DEBUG_HOOKS -DZS_DEC_PROFILE"):
ZSMI_LIB_FILE=$PWD/zstandard_amd/lib/var_decprof.so python tools/dec_profile.py"""
import os; os.environ["ZSMI_DEBUG_LIB"] = "1"          # the library built with -DZSMI_DEBUG_HOOKS (zstandard_amd/_lib.py)
pool = 256                                             # every frame to the general kernel, whose pool is small enough that each wavefront takes frames
os.environ["ZSMI_DEC_FAST"] = "0"; os.environ["ZSMI_DEC_POOL"] = str(pool)
import sys, os, ctypes
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import _data as D, _batch as B
from zstandard_amd import BatchCodec, _lib
n, cs = 2048, 32768
host = D.zipf_log(n * cs)
bc = BatchCodec(0); Z = _lib.lib()
offs = np.arange(n, dtype=np.uint64) * cs; sizes = np.full(n, cs, dtype=np.uint32)
arena, do, dsz = bc.compress_host(host, offs, sizes, 3)
frames = np.concatenate([arena[int(do[i]):int(do[i]) + int(dsz[i])] for i in range(n)])
fo = B.layout(dsz)
out, oo, osz = bc.decompress_host(frames, fo, dsz, sizes)
assert (osz == cs).all() and (out[:n * cs] == host).all()
names = ["literals", "seq tables", "seq decode", "seq execute", "checksum", "whole item", "  huf table", "  huf symbol loops"]
# the pool's literal buffers: a wavefront's counts, a word a name, are the last bytes of its own (zs_poollit_lend_dec_profile, csrc/zsmi_scratch.h)
bufs = _lib.copy_scratch(bc.ctx, "poolLit", pool).reshape(pool, -1)
prof = np.ascontiguousarray(bufs[:, -8 * len(names):]).view(np.uint64)
m = prof.mean(axis=0)
for k, nm in enumerate(names):
    print(f"{nm:12s} {m[k]:12.0f} ticks  {100 * m[k] / m[5]:5.1f} %")
print("literals per frame (mean):", float(np.mean([0])) )
print("whole item = %.0f s_memtime ticks (shader-clock cycles on this part: k_dec_prep at 163 K ticks an item and 16 items a CU at a time is its measured 0.97 ms per 57344 frames at ~2.4 GHz)" % m[5])
