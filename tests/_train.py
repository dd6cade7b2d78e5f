"""Samples, held-out chunks, the scalar model of the fastCover trainer (tests/c/train_model.c) and libzstd's ZDICT calls for the tests of
dictionary training (tests/test_dict_train_host.py, tests/test_gpu_dict_train.py).  Training samples are made exactly as
tests/golden/gen_fixtures_dict_compress.py makes them for the committed libzstd dictionaries: the class generator at its seed, cut in
1 - 4 KiB by default_rng(5).  Held-out data is _dicts.class_data(cls) cut in 1 - 4 KiB chunks."""
import ctypes, os, subprocess, tempfile
import numpy as np
import _corpus as C
import _data as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRAIN_BYTES = 3 << 20
TRAINING = {
    "json_records": lambda n: C.json_records(n, seed=1011),
    "xml_records": lambda n: C.xml_records(n, seed=1013),
    "csv_records": lambda n: C.csv_records(n, seed=1012),
    "binary_table": lambda n: C.binary_table(n, seed=1014),
    "zipf": lambda n: D.zipf_log(n, seed_lo=0xD1C7).tobytes(),
}


def cut(data, seed):
    rng = np.random.default_rng(seed)
    out, o = [], 0
    while o < len(data):
        k = int(rng.integers(1024, 4097))
        out.append(data[o:o + k]); o += k
    return out


_cache = {}


def samples(cls, nbytes=TRAIN_BYTES):
    if (cls, nbytes) not in _cache:
        _cache[(cls, nbytes)] = cut(TRAINING[cls](nbytes), 5)
    return _cache[(cls, nbytes)]


def held_out(cls):
    import _dicts
    return cut(_dicts.class_data(cls), 9)


def flat(parts):
    """(buffer bytes, size_t array) of samples laid back to back"""
    sizes = (ctypes.c_size_t * len(parts))(*[len(p) for p in parts])
    return b"".join(parts), sizes


_model = None


def model():
    """tests/c/train_model.c built with gcc into a temporary directory"""
    global _model
    if _model is None:
        out = os.path.join(tempfile.mkdtemp(prefix="train_model_"), "libtrain_model.so")
        subprocess.check_call(["gcc", "-std=gnu99", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", os.path.join(ROOT, "tests", "c", "train_model.c"), "-o", out])
        M = ctypes.CDLL(out)
        M.model_train.restype = ctypes.c_size_t
        M.model_train.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_size_t), ctypes.c_uint, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint, ctypes.c_uint, ctypes.c_uint]
        _model = M
    return _model


def model_content(parts, cap, k, d, f):
    buf, sizes = flat(parts)
    out = ctypes.create_string_buffer(cap)
    tail = model().model_train(buf, sizes, len(parts), out, cap, k, d, f)
    return out.raw[tail:cap]


# finalize from this library's parse, in libzstd on libzstd's own content, against the committed libzstd dictionary: 1.01 x, and the two
# classes where this encoder's statistics differ from libzstd's parse (tests/test_gpu_dict_train.py says why; measured 1.0137 x and 1.0462 x)
FINALIZE_BOUND = {"csv_records": 1.02, "binary_table": 1.05}


# ---- the reference of a whole training call: the model's content, oracle E's scores, oracle E's finalize ----
MAGIC = bytes([0x37, 0xA4, 0x30, 0xEC])
E_DST_TOO_SMALL, E_SRC_WRONG = 70, 72
CONTENT_MIN = 128


def candidates(cap, k, d, steps):
    """the (k, d) the trainer tries, in its order (trainParams in dict_train.hip): d given or 6 then 8; k given or 50 .. 2000 in `steps` steps"""
    steps = steps or 40
    ds = [d] if d else [6, 8]
    ks = [k] if k else [kk for kk in range(50, 2001, max((2000 - 50) // steps, 1)) if kk <= cap]
    return [(kk, dd) for dd in ds for kk in ks if kk >= dd]


def training_share(parts, k, d, split):
    """(number of training samples, held-out samples) of a call"""
    n = len(parts)
    split = split if split > 0 else 0.75
    nt = max(1, int(n * split)) if (k == 0 or d == 0) and split < 1.0 else n
    if sum(map(len, parts[:nt])) < 8:
        nt = n
    return nt, (parts[nt:] if nt < n else parts)


def content_frame_size(sample, content, level):
    """oracle E's frame of one sample with the content as a raw dictionary, whatever bytes the content starts with: its size"""
    import _oracle as O
    L = O.lib()
    L.zso_compressFrame.restype = ctypes.c_size_t
    L.zso_compressFrame.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_char_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p]
    pre = content[-65536:]
    cap = L.zso_compressBound(len(sample))
    out = ctypes.create_string_buffer(cap)
    r = L.zso_compressFrame(out, cap, sample, len(sample), level, pre, len(pre), 0, None)
    assert not L.zso_isError(r)
    return r


def reference_train(parts, cap, k=0, d=0, f=0, steps=0, split=0.0, level=0, dict_id=0):
    """What zsmi_trainFromBuffer_fastCover must return, stated once: (dictionary, k, d, content, scores).
    1. the training share: the first max(1, floor(n * split)) samples while searching (k == 0 or d == 0) with split below 1; all samples if
       that share has fewer than 8 bytes, and all samples otherwise
    2. the candidates of trainParams, in its order
    3. each candidate's content: the model's (tests/c/train_model.c) over the share
    4. its score: oracle E's frame sizes summed over the held-out samples (those behind the share; all samples if there are none) with the
       content as a raw dictionary
    5. the winner: the smallest sum, then the smaller k, then the smaller d
    6. the dictionary: zso_finalizeDictionary over all samples with the winner's content; an error code (int) where the call must fail:
       72 for a content under 128 bytes, 70 where finalize cannot make the dictionary"""
    import _oracle as O
    f, level = f or 20, level or 3
    nt, held = training_share(parts, k, d, split)
    cands = candidates(cap, k, d, steps)
    contents = [model_content(parts[:nt], cap, kk, dd, f) for kk, dd in cands]
    scores = [sum(content_frame_size(s, c, level) for s in held) if c else sum(len(O.compress(s, level)) for s in held) for c in contents] if len(cands) > 1 else [0]
    win = min(range(len(cands)), key=lambda i: (scores[i], cands[i][0], cands[i][1]))
    (kk, dd), content = cands[win], contents[win]
    if len(content) < CONTENT_MIN:
        return E_SRC_WRONG, kk, dd, content, scores
    dic = O.finalize_dictionary(content, parts, cap, level, dict_id)
    return (E_DST_TOO_SMALL if dic is None else dic), kk, dd, content, scores


def check_format(dic, cap):
    """what tests/test_gpu_dict_train.py's check_format asks of a dictionary, without the GPU library: magic, ID, recent offsets, oracle D's
    parse, three NCounts of the right logs without a zero count; returns the content"""
    import _oracle as O
    import _framewriter as W
    assert 0 < len(dic) <= cap and dic[:4] == MAGIC
    did = int.from_bytes(dic[4:8], "little")
    off, pid, reps = O.dict_params(dic)
    assert pid == did and reps == (1, 4, 8)
    content = dic[off:]
    assert dic[off - 12:off] == bytes([1, 0, 0, 0, 4, 0, 0, 0, 8, 0, 0, 0])
    h = dic[8]
    assert h < 128, "256 weights only fit an FSE-compressed description"
    p = 8 + 1 + h
    of_max = min((len(content) + (128 << 10)).bit_length() - 1, 31)
    for max_sym, log in ((of_max, 8), (52, 9), (35, 9)):
        norm, tl, p = W.read_ncount(dic, p, max_sym)
        assert tl == log and len(norm) == max_sym + 1 and all(v != 0 for v in norm), (max_sym, norm)
    assert p + 12 == off
    return content


def derived_id(content):
    import _framewriter as W
    return W.xxh64(content) % ((1 << 31) - 32768) + 32768


# ---- libzstd's ZDICT (optional yardstick) ----
class ZParams(ctypes.Structure):
    _fields_ = [("compressionLevel", ctypes.c_int), ("notificationLevel", ctypes.c_uint), ("dictID", ctypes.c_uint)]


class ZFastCover(ctypes.Structure):        # ZDICT_fastCover_params_t, zstd 1.4.5 .. 1.5
    _fields_ = [("k", ctypes.c_uint), ("d", ctypes.c_uint), ("f", ctypes.c_uint), ("steps", ctypes.c_uint), ("nbThreads", ctypes.c_uint),
                ("splitPoint", ctypes.c_double), ("accel", ctypes.c_uint), ("shrinkDict", ctypes.c_uint), ("shrinkDictMaxRegression", ctypes.c_uint),
                ("zParams", ZParams)]


_z = None


def zdict():
    """libzstd with its ZDICT calls, or None"""
    global _z
    if _z is None:
        try:
            Z = ctypes.CDLL("libzstd.so.1")
            Z.ZSTD_versionNumber.restype = ctypes.c_uint
            if Z.ZSTD_versionNumber() < 10405:
                raise OSError("ZDICT_fastCover_params_t of zstd >= 1.4.5 expected")
        except (OSError, AttributeError):
            _z = False
            return None
        sz, vp, cp = ctypes.c_size_t, ctypes.c_void_p, ctypes.c_char_p
        psz = ctypes.POINTER(sz)
        Z.ZDICT_isError.restype = ctypes.c_uint; Z.ZDICT_isError.argtypes = [sz]
        Z.ZDICT_getDictID.restype = ctypes.c_uint; Z.ZDICT_getDictID.argtypes = [cp, sz]
        Z.ZDICT_trainFromBuffer.restype = sz; Z.ZDICT_trainFromBuffer.argtypes = [vp, sz, cp, psz, ctypes.c_uint]
        Z.ZDICT_trainFromBuffer_fastCover.restype = sz; Z.ZDICT_trainFromBuffer_fastCover.argtypes = [vp, sz, cp, psz, ctypes.c_uint, ZFastCover]
        Z.ZDICT_optimizeTrainFromBuffer_fastCover.restype = sz
        Z.ZDICT_optimizeTrainFromBuffer_fastCover.argtypes = [vp, sz, cp, psz, ctypes.c_uint, ctypes.POINTER(ZFastCover)]
        Z.ZDICT_finalizeDictionary.restype = sz; Z.ZDICT_finalizeDictionary.argtypes = [vp, sz, cp, sz, cp, psz, ctypes.c_uint, ZParams]
        _z = Z
    return _z or None


def zdict_finalize(content, parts, cap, level=3):
    Z = zdict()
    buf, sizes = flat(parts)
    out = ctypes.create_string_buffer(cap)
    r = Z.ZDICT_finalizeDictionary(out, cap, content, len(content), buf, sizes, len(parts), ZParams(level, 0, 0))
    assert not Z.ZDICT_isError(r), r
    return out.raw[:r]


def zdict_fastcover(parts, cap, k, d, f):
    Z = zdict()
    buf, sizes = flat(parts)
    out = ctypes.create_string_buffer(cap)
    p = ZFastCover(k=k, d=d, f=f, steps=0, nbThreads=1, splitPoint=1.0, accel=1, zParams=ZParams(3, 0, 0))
    r = Z.ZDICT_trainFromBuffer_fastCover(out, cap, buf, sizes, len(parts), p)
    assert not Z.ZDICT_isError(r), r
    return out.raw[:r]


def zstd_total(chunks, dic, level=3):
    """libzstd's total over the chunks with a dictionary"""
    import _dicts
    return sum(len(_dicts.zstd_compress_dict(c, dic, level)) for c in chunks)
