import ctypes, sys
import os; sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _corpus as C, _data as D
L = ctypes.CDLL(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'oracle', '_build', 'libzso_asan.so'))
L.zso_compress.restype = ctypes.c_size_t; L.zso_compress.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int]
L.zso_decompress.restype = ctypes.c_size_t; L.zso_decompress.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t]
L.zso_compressBound.restype = ctypes.c_size_t; L.zso_compressBound.argtypes = [ctypes.c_size_t]
import numpy as np
rng = np.random.default_rng(1)
n = 0
items = list(D.mixed_inputs().values())
for name, data in C.corpus(1 << 19).items():
    for cs in (65536, 131072, 200000, 33333):
        items += [data[i:i + cs] for i in range(0, len(data), cs)][:3]
for c in items:
    for level in (1, 3):
        cap = L.zso_compressBound(len(c)); out = ctypes.create_string_buffer(cap)
        r = L.zso_compress(out, cap, c, len(c), level)
        assert r < (1 << 62)
        back = ctypes.create_string_buffer(max(len(c), 1))
        d = L.zso_decompress(back, len(c), out.raw[:r], r)
        assert d == len(c) and back.raw[:d] == c
        # damaged copies through the decoder (both Huffman decoders, error paths)
        fr = bytearray(out.raw[:r])
        for _ in range(6):
            b = bytearray(fr); b[int(rng.integers(0, len(b)))] ^= int(rng.integers(1, 256))
            L.zso_decompress(back, len(c), bytes(b), len(b))
        n += 1
# with dictionaries: raw, tiny, formatted and > 64 KiB content (prefixed units, content in front of the prefix, the ID field)
import _dicts as X
L.zso_compress_usingDict.restype = ctypes.c_size_t
L.zso_compress_usingDict.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int]
L.zso_decompress_usingDict.restype = ctypes.c_size_t
L.zso_decompress_usingDict.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t]
dicts = X.identity_dictionaries()
for name in ("raw1", "raw7", "raw9", "raw6000", "trained8k", "trained64k_zipf", "raw100000", "reps_70000_content100k"):
    dic = bytes(dicts[name])                                              # (a copy of its own: the sanitizer sees its exact bounds)
    for k, c in enumerate(X.prefix_chunks(dic, (0, 1, 8, 17, 4096, 65536, 65537, 131073))):
        level = (1, 3, 4)[k % 3]
        cap = L.zso_compressBound(len(c)); out = ctypes.create_string_buffer(cap)
        r = L.zso_compress_usingDict(out, cap, c, len(c), dic, len(dic), level)
        assert r < (1 << 62), (name, k)
        back = ctypes.create_string_buffer(max(len(c), 1))
        d = L.zso_decompress_usingDict(back, len(c), out.raw[:r], r, dic, len(dic))
        assert d == len(c) and back.raw[:d] == c, (name, k)
        fr = bytearray(out.raw[:r])
        for _ in range(3):
            b = bytearray(fr); b[int(rng.integers(0, len(b)))] ^= int(rng.integers(1, 256))
            L.zso_decompress_usingDict(back, len(c), bytes(b), len(b), dic, len(dic))
        n += 1
for d in X.bad_dictionaries():
    out = ctypes.create_string_buffer(L.zso_compressBound(100))
    r = L.zso_compress_usingDict(out, len(out), bytes(100), 100, d, len(d), 3)
    assert r == (1 << 64) - 30
print("asan/ubsan clean over", n, "compress + decode rounds")
