#!/usr/bin/env python3
"""Generates tests/golden/libzstd_fixtures_cdict_sizes.npz: upstream libzstd's ZSTD_compress_usingDict sizes at level 3 for the exact
chunks of the digested-dictionary size test (tests/test_gpu_cdict.py::test_sizes_against_libzstd; chunks: tests/_cdict.py size_chunks), each
record class with its trained dictionary of tests/golden/libzstd_fixtures_dict_compress.npz.  Entry <class>_<chunk size>: the total
bytes of the class's frames; `version`: ZSTD_versionNumber of the library that made them (1.4.8 = 10408).
Run from the repo root: python tests/golden/gen_fixtures_cdict_sizes.py"""
import os, sys
import numpy as np
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _dicts as X
import _cdict as K

assert X.zstd(), "libzstd.so.1 is needed to make this fixture"
out = {"version": np.array(X.zstd().ZSTD_versionNumber(), dtype=np.uint32)}
for cls in X.RECORD_CLASSES:
    dic = X.trained(cls)
    for cs in K.SIZE_CHUNKS:
        out[f"{cls}_{cs}"] = np.array(sum(len(X.zstd_compress_dict(c, dic, 3)) for c in K.size_chunks(cls, cs)), dtype=np.uint64)
        print(cls, cs, int(out[f"{cls}_{cs}"]))
np.savez(os.path.join(HERE, "libzstd_fixtures_cdict_sizes.npz"), **out)
