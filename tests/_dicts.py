"""Dictionaries and chunks for the tests of compression with a dictionary (oracle E: tests/test_oracle_dict_encoder.py; the HIP path:
tests/test_gpu_dict_compress.py), and upstream libzstd's usingDict calls when the box has libzstd.  Fixtures:
tests/golden/libzstd_fixtures_dict.npz (an 8 KiB trained dictionary) and tests/golden/libzstd_fixtures_dict_compress.npz (64 KiB
dictionaries trained per record class)."""
import ctypes, os
import numpy as np
import _oracle as O
import _data as D
import _corpus as C

FIX = np.load(os.path.join(D.GOLDEN, "libzstd_fixtures_dict.npz"))
FIXC = np.load(os.path.join(D.GOLDEN, "libzstd_fixtures_dict_compress.npz"))
TRAINED8K = FIX["trained_small_l3_dict"].tobytes()
RECORD_CLASSES = ["json_records", "xml_records", "zipf", "csv_records", "binary_table"]
# the stream the raw-content dictionaries are cut from; chunks that continue a dictionary are cut from behind it
STREAM = C.json_records(400000, seed=303)


def trained(cls):
    return FIXC["trained_" + cls].tobytes()


def content_of(dic):
    """the content part of a ZDICT-trained dictionary: what follows its recent offsets, which ZDICT leaves at {1, 4, 8}
    (libzstd's ZDICT_getDictHeaderSize agrees where it is exported)"""
    at = dic.find(bytes([1, 0, 0, 0, 4, 0, 0, 0, 8, 0, 0, 0]), 8)
    assert at > 8
    return dic[at + 12:]


def with_reps(dic, reps, content=None):
    """a trained dictionary with other recent offsets (and, if given, other content)"""
    old = content_of(dic)
    at = len(dic) - len(old) - 12
    return dic[:at] + b"".join(r.to_bytes(4, "little") for r in reps) + (old if content is None else content)


def with_id(dic, dict_id):
    return dic[:4] + dict_id.to_bytes(4, "little") + dic[8:]


def content(dic):
    """the bytes a frame may reference: all of a raw dictionary, the content of a formatted one (oracle D's parse)"""
    return dic[O.dict_params(dic)[0]:]


_data_cache = {}


def class_data(cls, n=1 << 19):
    if (cls, n) not in _data_cache:
        if cls == "zipf":
            b = D.zipf_log(n, seed_lo=0x77).tobytes()
        elif cls == "repetitive":
            b = C.repetitive(n)
        else:
            b = getattr(C, cls)(n)
        _data_cache[(cls, n)] = b[:n]
    return _data_cache[(cls, n)]


def entropy_layout(dic):
    """where the parts of a formatted dictionary's entropy section start: [offset-code counts, match-length counts, literal-length
    counts, recent offsets] (the Huffman description starts at 8)"""
    import _framewriter as W
    h = dic[8]
    p = 8 + ((h - 127 + 1) // 2 + 1 if h >= 128 else h + 1)
    marks = [p]
    for max_symbol in (31, 52, 35):
        p = W.read_ncount(dic, p, max_symbol)[2]
        marks.append(p)
    assert marks[3] == len(dic) - len(content_of(dic)) - 12
    return marks


def bad_entropy_sections():
    """the 8 KiB trained dictionary with one part of its entropy section replaced or cut, by name: what LoadEntropy's own checks refuse
    (the Huffman description's, the limits of each count header, the section's end) - every one is refused by oracle D with 30
    (tests/test_oracle_dict_encoder.py::test_refused_dictionaries checks the list on the CPU)"""
    import _framewriter as W
    dic = TRAINED8K
    of, ml, ll, reps = entropy_layout(dic)
    huf = lambda weights: dic[:8] + W.huf_description(weights) + dic[of:]     # (weights: the last one is implied, not written)
    return {
        "magic and ID, nothing else": dic[:8],
        "offset-code counts at accuracy log 9": dic[:of] + W.ncount([128] * 4, 9) + dic[ml:],
        "match-length counts that declare symbol 53": dic[:ml] + W.ncount([2] * 10 + [1] * 44, 6) + dic[ll:],
        "literal-length counts that declare symbol 36": dic[:ll] + W.ncount([2] * 27 + [1] * 10, 6) + dic[reps:],
        "literal-length counts at accuracy log 10": dic[:ll] + W.ncount([256] * 4, 10) + dic[reps:],
        "Huffman weights that do not complete to a power of two": huf([3, 1, 0]),          # 4 + 1 = 5 of 8: 3 are left
        "Huffman table log 13": huf([11, 11, 11, 11, 0]),                                      # 4 * 1024: a total of 2^12 asks for 13 bits
        "Huffman weights without a pair of weight 1": huf([2, 0]),                             # 2 of 4, the implied weight is 2 as well
        "cut inside the third count header": dic[:ll + 2],
        "cut inside the twelve offset bytes": dic[:reps + 6],
    }


def bad_dictionaries():
    """dictionaries oracle D refuses (dictionary_corrupted): cut entropy sections, a recent offset of 0, one past the content, and the
    hand-built entropy sections of bad_entropy_sections()"""
    dic = TRAINED8K
    rep0 = with_reps(dic, (0, 4, 8))
    past = with_reps(dic, (1, len(content_of(dic)), 8))
    return [dic[:9], dic[:40], dic[:120], rep0, past] + list(bad_entropy_sections().values())


def identity_dictionaries():
    """every kind of dictionary the prefix rules treat differently: raw content of 1, 7, 8 and 9 bytes (fewer than 8: no table entries),
    6000 bytes, exactly 64 KiB and 100 000 bytes (only the last 64 KiB are a prefix); the 8 KiB and the five 64 KiB trained ones; formatted
    ones with other recent offsets (one above 64 KiB, inside content of 100 000 bytes)"""
    out = {f"raw{k}": STREAM[:k] for k in (1, 7, 8, 9, 6000, 65536, 100000)}
    out["trained8k"] = TRAINED8K
    out.update({"trained64k_" + cls: trained(cls) for cls in RECORD_CLASSES})
    out["reps_2_3_5"] = with_reps(trained("json_records"), (2, 3, 5))
    out["reps_70000_content100k"] = with_reps(TRAINED8K, (70000, 4, 99999), STREAM[:100000])
    return out


def id_dictionaries():
    """the 8 KiB trained dictionary with IDs at each header field size (0: no field, 1, 2, 4 bytes)"""
    return {i: with_id(TRAINED8K, i) for i in (0, 1, 255, 256, 65535, 65536, 0xFFFFFFFF)}


IDENTITY_SIZES = (0, 1, 7, 8, 15, 16, 17, 255, 256, 257, 1024, 4096, 65535, 65536, 65537, 65791, 65792, 131072, 131073, 200 * 1024)


_corpus = []


def corpus_classes():
    if not _corpus:
        _corpus.extend(sorted(C.corpus(1 << 18).items()))
    return _corpus


def prefix_chunks(dic, sizes=IDENTITY_SIZES):
    """chunks for one dictionary: the sizes around every limit, cut from the corpus classes in turn, and contents aimed at the prefix
    rules (names in the comments)"""
    classes = corpus_classes()
    rng = np.random.default_rng(len(dic))
    cont = content(dic)
    pre = cont[-65536:]
    noise = lambda k: rng.integers(0, 256, k, dtype=np.uint8).tobytes()
    chunks = []
    for j, cs in enumerate(sizes):
        data = classes[j % len(classes)][1]
        o = (j * 7919) % (len(data) - cs + 1)
        chunks.append(data[o:o + cs])
    for name, data in classes:                                          # every class at the small chunk sizes
        chunks += [data[5000:5000 + 1024], data[70000:70000 + 4096]]
    tail = pre[-100:]
    chunks += [
        pre[-300:] + noise(200) + pre[-1000:-700],                      # copies of the prefix's last bytes
        tail * 3 + noise(64),                                           # sources that straddle the prefix's end, from chunk position 0
        (STREAM[len(dic):len(dic) + 4096] if len(cont) == len(dic) else cont[-7:] + noise(40) + cont[-50:]),   # continues the dictionary
        noise(49) + b"\0" + pre[:200] + noise(100),                     # only the prefix's first bytes: distance p + P, no byte before them
        noise(3) + pre[:64] + noise(30) + pre[:64],                     # the same, then a repeat inside the chunk
        (cont[:-65536][-3000:] if len(cont) > 65536 else b"") + noise(50),   # content in front of the last 64 KiB only: never referenced
        cont[-1:], cont[-1:] * 40, cont[-1:] * 40 + noise(20),         # the dictionary's trailing byte (one, a run)
        noise(3000), noise(65536),                                      # matchless
    ]
    return chunks


# ---- upstream libzstd with dictionaries (optional yardstick) ----
_Z = None


def zstd():
    global _Z
    if _Z is None:
        Z = O.libzstd()
        if Z:
            sz, vp, cp = ctypes.c_size_t, ctypes.c_void_p, ctypes.c_char_p
            Z.ZSTD_createCCtx.restype = vp; Z.ZSTD_createDCtx.restype = vp
            Z.ZSTD_compress_usingDict.restype = sz; Z.ZSTD_compress_usingDict.argtypes = [vp, vp, sz, cp, sz, cp, sz, ctypes.c_int]
            Z.ZSTD_decompress_usingDict.restype = sz; Z.ZSTD_decompress_usingDict.argtypes = [vp, vp, sz, cp, sz, cp, sz]
            Z.cctx = Z.ZSTD_createCCtx(); Z.dctx = Z.ZSTD_createDCtx()
        _Z = Z or False
    return _Z or None


def zstd_compress_dict(data, dic, level):
    Z = zstd()
    cap = Z.ZSTD_compressBound(len(data)); out = ctypes.create_string_buffer(cap)
    r = Z.ZSTD_compress_usingDict(Z.cctx, out, cap, data, len(data), dic, len(dic), level)
    assert not Z.ZSTD_isError(r)
    return out.raw[:r]


def zstd_decompress_dict(frame, cap, dic):
    Z = zstd()
    out = ctypes.create_string_buffer(max(cap, 1))
    r = Z.ZSTD_decompress_usingDict(Z.dctx, out, cap, frame, len(frame), dic, len(dic))
    return None if Z.ZSTD_isError(r) else out.raw[:r]
