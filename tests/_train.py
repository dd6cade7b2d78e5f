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
