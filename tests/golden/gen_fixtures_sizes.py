#!/usr/bin/env python3
"""Generates tests/golden/libzstd_sizes.json: upstream libzstd's ZSTD_findDecompressedSize, ZSTD_findFrameCompressedSize and
ZSTD_decompressBound for the items of tests/_sizes.py items() - every frame of the libzstd fixture files, hand-built frames that state no
content size (windows of 1 KiB, 16 KiB and 8 MiB; 1, 2 and 5 raw, RLE and compressed blocks), concatenations, skippable frames, checksums.
An entry holds the item's name, the sha256 of its bytes (the tests rebuild the bytes and compare) and the three answers as integers
(2^64 - 1: unknown; 2^64 - 2: error); `version`: ZSTD_versionNumber of the library that made them (1.4.8 = 10408).
No item has a window above 2^30: libzstd accepts a window log of 31, this library, like its reference, refuses above 30.
Run from the repo root: python tests/golden/gen_fixtures_sizes.py"""
import ctypes, json, os, sys
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _oracle as O
import _sizes as S

Z = O.libzstd()
assert Z, "libzstd.so.1 is needed to make this fixture"
ull, sz, vp = ctypes.c_ulonglong, ctypes.c_size_t, ctypes.c_char_p
Z.ZSTD_findDecompressedSize.restype = ull; Z.ZSTD_findDecompressedSize.argtypes = [vp, sz]
Z.ZSTD_findFrameCompressedSize.restype = sz; Z.ZSTD_findFrameCompressedSize.argtypes = [vp, sz]
Z.ZSTD_decompressBound.restype = ull; Z.ZSTD_decompressBound.argtypes = [vp, sz]

records = []
for name, item in S.items():
    first = Z.ZSTD_findFrameCompressedSize(item, len(item))
    assert not Z.ZSTD_isError(first), name
    records.append({"name": name, "sha256": S.sha(item), "find_decompressed_size": int(Z.ZSTD_findDecompressedSize(item, len(item))),
                    "find_frame_compressed_size": int(first), "decompress_bound": int(Z.ZSTD_decompressBound(item, len(item)))})
    print(name, len(item), records[-1]["find_decompressed_size"], records[-1]["find_frame_compressed_size"], records[-1]["decompress_bound"])
with open(S.SIZES_JSON, "w") as f:
    json.dump({"version": int(Z.ZSTD_versionNumber()), "items": records}, f, indent=0)
    f.write("\n")
