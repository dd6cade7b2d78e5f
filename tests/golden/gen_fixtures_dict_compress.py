#!/usr/bin/env python3
"""Generates tests/golden/libzstd_fixtures_dict_compress.npz: 64 KiB dictionaries trained by upstream libzstd (ZDICT_trainFromBuffer)
for the dictionary compressor's tests (tests/test_gpu_dict_compress.py).  One per record class of tests/_corpus.py the ratio contract
names - json_records, xml_records, zipf, csv_records, binary_table -, each from the class's generator at a seed (or a region) the tests
do not use, cut in samples of 1 - 4 KiB.  Entry: trained_<class>.
Run from the repo root: python tests/golden/gen_fixtures_dict_compress.py"""
import ctypes, os, sys
import numpy as np
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _corpus as C
import _data as D

Z = ctypes.CDLL("libzstd.so.1")
sz, vp, cp = ctypes.c_size_t, ctypes.c_void_p, ctypes.c_char_p
Z.ZDICT_trainFromBuffer.restype = sz; Z.ZDICT_trainFromBuffer.argtypes = [vp, sz, cp, ctypes.POINTER(sz), ctypes.c_uint]
Z.ZDICT_isError.restype = ctypes.c_uint; Z.ZDICT_isError.argtypes = [sz]

TRAIN_BYTES = 3 << 20
TRAINING = {                                    # data the tests never compress: other seeds of the same generators
    "json_records": lambda: C.json_records(TRAIN_BYTES, seed=1011),
    "xml_records": lambda: C.xml_records(TRAIN_BYTES, seed=1013),
    "csv_records": lambda: C.csv_records(TRAIN_BYTES, seed=1012),
    "binary_table": lambda: C.binary_table(TRAIN_BYTES, seed=1014),
    "zipf": lambda: D.zipf_log(TRAIN_BYTES, seed_lo=0xD1C7).tobytes(),
}


def train(data, cap=65536):
    rng = np.random.default_rng(5)
    samples, o = [], 0
    while o < len(data):
        k = int(rng.integers(1024, 4097))
        samples.append(data[o:o + k]); o += k
    buf = b"".join(samples); sizes = (sz * len(samples))(*[len(x) for x in samples])
    dbuf = ctypes.create_string_buffer(cap)
    r = Z.ZDICT_trainFromBuffer(dbuf, cap, buf, sizes, len(samples)); assert not Z.ZDICT_isError(r), r
    d = dbuf.raw[:r]; assert d[:4] == bytes([0x37, 0xA4, 0x30, 0xEC])
    return d


if __name__ == "__main__":
    out = {"trained_" + k: np.frombuffer(train(f()), dtype=np.uint8) for k, f in TRAINING.items()}
    np.savez_compressed(os.path.join(HERE, "libzstd_fixtures_dict_compress.npz"), **out)
    print({k: len(v) for k, v in out.items()})
