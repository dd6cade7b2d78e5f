#!/usr/bin/env python3
"""GPU check (run by tests/test_gpu_decode_edges.py::test_edge_shapes_stay_on_the_fast_path, in a process of its own because it loads the
library built with the debug hooks): the edge catalogue (tests/_edge_catalogue.py) is decoded in placement (a) exact capacities and (b)
1 MiB capacities, and each item's descriptor (ZsFastDesc.fast) is read back.  Prints one JSON object:
{placement: {entry id: 1 fast path / 0 general kernel / -1 decoded wrongly}}."""
import os; os.environ["ZSMI_DEBUG_LIB"] = "1"
import sys, ctypes, json
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import _oracle as O, _edge_catalogue as C, _batch as B
from zstandard_amd import BatchCodec, _lib
from fastpath_check import desc_layout


def main():
    if _lib.built_fingerprint() != _lib.source_fingerprint():
        _lib.build()
    bc = BatchCodec(0); Z = _lib.lib()
    DESC_WORDS, FAST_AT = desc_layout(Z)
    cat = C.catalogue()
    res = {}
    for placement, caps in (("a", [e.cap for e in cat]), ("b", [1 << 20] * len(cat))):
        out, oo, osz = bc.decompress_host(*B.batch([e.frame for e in cat]), np.array(caps, dtype=np.uint32))
        buf = np.zeros(len(cat) * DESC_WORDS, dtype=np.uint32)
        rc = Z.zsmi_dbg_copyScratch(bc.ctx, b"fastDesc", buf.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(buf.nbytes)); assert rc == 0, rc
        fast = buf.reshape(-1, DESC_WORDS)[:len(cat), FAST_AT]
        r = {}
        for i, e in enumerate(cat):
            try:
                w = O.decompress(e.frame, caps[i]); ok = int(osz[i]) == len(w) and out[int(oo[i]):int(oo[i]) + len(w)].tobytes() == w
            except O.OracleError as x:
                ok = int(osz[i]) == (1 << 32) - x.code
            r[e.id] = int(fast[i] == 1) if ok else -1
        res[placement] = r
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
