"""Loads libzsmi.so (HIP kernels + C ABI).  The library is built in-tree by __graft_entry__.build()
(hipcc --offload-arch=gfx950).  There is no fallback: if the library is missing the import fails."""
import ctypes, os, subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
# development tools (tools/gpu_debug.py, tools/time_kernels.py) set ZSMI_DEBUG_LIB=1: a second library built with
# -DZSMI_DEBUG_HOOKS (scratch read-back, stage-stop timing aids); the product library has neither
DEBUG = os.environ.get("ZSMI_DEBUG_LIB", "") == "1"
LIB_PATH = os.environ.get("ZSMI_LIB_FILE") or os.path.join(_HERE, "lib", "libzsmi_debug.so" if DEBUG else "libzsmi.so")   # ZSMI_LIB_FILE: kernel-shape experiments
CSRC = os.path.join(_HERE, "csrc")


def extra_flags():
    """compile flags beyond the fixed ones: kernel-shape experiments (ZSMI_HIPCC_FLAGS) and the debug-hook switch - part of the fingerprint, so
    that a variant build is never taken for the tree's product library"""
    return os.environ.get("ZSMI_HIPCC_FLAGS", "").split() + (["-DZSMI_DEBUG_HOOKS"] if DEBUG else [])


def source_fingerprint():
    """sha256 over the kernel sources (*.hip, *.h; comments and white space do not count) and the extra compile flags: the library carries
    the one it was built from (zsmi_versionString), profiles/*_traffic.json the one it was measured at"""
    import hashlib, re
    h = hashlib.sha256()
    names = sorted(f for f in os.listdir(CSRC) if f.endswith((".hip", ".h")) and os.path.isfile(os.path.join(CSRC, f)))
    for f in names + [os.path.join("..", "..", "include", "zsmi.h")]:
        text = open(os.path.join(CSRC, f), "r", errors="replace").read()
        text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
        text = re.sub(r"//[^\n]*", "", text)
        text = re.sub(r"\s+", "", text)
        h.update(f.encode()); h.update(text.encode())
    flags = extra_flags()
    if flags:
        h.update(" ".join(flags).encode())
    return h.hexdigest()[:16]


def built_fingerprint(path=None):
    """the fingerprint inside a built library (None: no library, or one from before the fingerprint existed)"""
    path = path or LIB_PATH
    if not os.path.exists(path):
        return None
    import re
    m = re.search(rb"sources ([0-9a-f]{16}|unknown)\)", open(path, "rb").read())
    return m.group(1).decode() if m else None


def build(force=False):
    """hipcc --offload-arch=gfx950 -> the in-tree library.  Rebuilds when the library is missing or was built from other sources than the
    tree holds (the fingerprint inside it differs: a library that travelled with the snapshot is checked, not trusted; file times say
    nothing after a copy)."""
    fp = source_fingerprint()
    if not force and not os.environ.get("ZSMI_LIB_FILE") and os.path.exists(LIB_PATH) and built_fingerprint() == fp:
        return LIB_PATH
    if os.environ.get("ZSMI_LIB_FILE") and os.path.exists(LIB_PATH) and not force:
        return LIB_PATH                                                # a variant build named by hand: left alone
    os.makedirs(os.path.dirname(LIB_PATH), exist_ok=True)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-shared", "-fPIC", '-DZSMI_SOURCE_FP="%s"' % fp, "-o", LIB_PATH, os.path.join(CSRC, "zsmi_api.hip")]
    cmd += extra_flags()                                           # kernel-shape experiments (-DZS_CAND_G=4 ...), the debug hooks
    subprocess.check_call(cmd)
    return LIB_PATH


_lib = None


class FastCoverParams(ctypes.Structure):
    _fields_ = [("k", ctypes.c_uint), ("d", ctypes.c_uint), ("f", ctypes.c_uint), ("steps", ctypes.c_uint), ("accel", ctypes.c_uint),
                ("splitPoint", ctypes.c_double), ("level", ctypes.c_int), ("dictID", ctypes.c_uint)]


class FindQuery(ctypes.Structure):
    """zsmi_findQuery: up to 8 patterns (host bytes, kept alive by the caller), a mode (0 any, 1 all, 2 none) and flags (1: ignore ASCII case)"""
    _fields_ = [("nPatterns", ctypes.c_uint32), ("mode", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("patterns", ctypes.c_void_p * 8),
                ("patternSizes", ctypes.c_uint32 * 8)]


class FrameFilterInfo(ctypes.Structure):
    """zsmi_frameFilterInfo: what zsmi_readFrameFilter finds in a filter frame that holds - its frames, delimiter, gram length, log2 of the
    bits a frame, the content's size and the slots that are all ones"""
    _fields_ = [("nFrames", ctypes.c_uint32), ("delim", ctypes.c_uint32), ("gram", ctypes.c_uint32), ("log2Bits", ctypes.c_uint32),
                ("size", ctypes.c_uint64), ("saturated", ctypes.c_uint64)]


class RegexProgram(ctypes.Structure):
    """zsmi_regexProgram: the minimal DFA of a pattern (zsmi_compileRegex) - next[s * nClasses + classOf[b]], a start state, the accepting
    states as a 64-bit word, flags (1: compiled ignoring ASCII case, 2: list the records that do NOT match)"""
    _fields_ = [("nStates", ctypes.c_uint32), ("nClasses", ctypes.c_uint32), ("start", ctypes.c_uint32), ("flags", ctypes.c_uint32),
                ("accept", ctypes.c_uint64), ("classOf", ctypes.c_uint8 * 256), ("next", ctypes.c_uint8 * 3072)]


class KernelTime(ctypes.Structure):
    _fields_ = [("name", ctypes.c_char * 48), ("seconds", ctypes.c_double), ("launches", ctypes.c_uint32)]


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: run __graft_entry__.build() (hipcc --offload-arch=gfx950); there is no CPU fallback")
    L = ctypes.CDLL(LIB_PATH)
    vp, sz, u32, i32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_int
    L.zsmi_isError.restype = ctypes.c_uint; L.zsmi_isError.argtypes = [sz]
    L.zsmi_getErrorCode.restype = ctypes.c_uint; L.zsmi_getErrorCode.argtypes = [sz]
    L.zsmi_getErrorName.restype = ctypes.c_char_p; L.zsmi_getErrorName.argtypes = [sz]
    L.zsmi_versionString.restype = ctypes.c_char_p
    L.zsmi_compressBound.restype = sz; L.zsmi_compressBound.argtypes = [sz]
    L.zsmi_getDecompressedSize.restype = ctypes.c_ulonglong; L.zsmi_getDecompressedSize.argtypes = [vp, sz]
    L.zsmi_compress.restype = sz; L.zsmi_compress.argtypes = [vp, sz, vp, sz, i32]
    L.zsmi_compress_usingDict.restype = sz; L.zsmi_compress_usingDict.argtypes = [vp, sz, vp, sz, vp, sz, i32]
    L.zsmi_decompress.restype = sz; L.zsmi_decompress.argtypes = [vp, sz, vp, sz]
    L.zsmi_decompress_usingDict.restype = sz; L.zsmi_decompress_usingDict.argtypes = [vp, sz, vp, sz, vp, sz]
    L.zsmi_createCtx.restype = vp; L.zsmi_createCtx.argtypes = [i32, vp]
    L.zsmi_freeCtx.restype = None; L.zsmi_freeCtx.argtypes = [vp]
    L.zsmi_sync.restype = i32; L.zsmi_sync.argtypes = [vp]
    L.zsmi_setParameter.restype = i32; L.zsmi_setParameter.argtypes = [vp, i32, i32]
    L.zsmi_getParameter.restype = i32; L.zsmi_getParameter.argtypes = [vp, i32, ctypes.POINTER(i32)]
    L.zsmi_compress_advanced.restype = sz; L.zsmi_compress_advanced.argtypes = [vp, sz, vp, sz, vp, sz, i32, i32]
    L.zsmi_compress_usingCDict_advanced.restype = sz; L.zsmi_compress_usingCDict_advanced.argtypes = [vp, sz, vp, sz, vp, i32]
    L.zsmi_compressBatchDevice.restype = i32; L.zsmi_compressBatchDevice.argtypes = [vp, vp, vp, vp, u32, vp, vp, vp, i32]
    L.zsmi_decompressBatchDevice.restype = i32; L.zsmi_decompressBatchDevice.argtypes = [vp, vp, vp, vp, u32, vp, vp, vp, vp]
    L.zsmi_compressBatchHost.restype = i32; L.zsmi_compressBatchHost.argtypes = [vp, vp, vp, vp, u32, vp, vp, vp, i32]
    L.zsmi_compressBatchDevice_usingDict.restype = i32; L.zsmi_compressBatchDevice_usingDict.argtypes = [vp, vp, vp, vp, u32, vp, vp, vp, i32, vp, sz]
    L.zsmi_compressBatchHost_usingDict.restype = i32; L.zsmi_compressBatchHost_usingDict.argtypes = [vp, vp, vp, vp, u32, vp, vp, vp, i32, vp, sz]
    L.zsmi_createCDict.restype = vp; L.zsmi_createCDict.argtypes = [vp, vp, sz, i32, ctypes.POINTER(i32)]
    L.zsmi_freeCDict.restype = None; L.zsmi_freeCDict.argtypes = [vp]
    L.zsmi_getDictID_fromCDict.restype = ctypes.c_uint; L.zsmi_getDictID_fromCDict.argtypes = [vp]
    L.zsmi_sizeofCDict.restype = sz; L.zsmi_sizeofCDict.argtypes = [vp]
    L.zsmi_compressBatchDevice_usingCDict.restype = i32; L.zsmi_compressBatchDevice_usingCDict.argtypes = [vp, vp, vp, vp, u32, vp, vp, vp, vp]
    L.zsmi_compressBatchHost_usingCDict.restype = i32; L.zsmi_compressBatchHost_usingCDict.argtypes = [vp, vp, vp, vp, u32, vp, vp, vp, vp]
    L.zsmi_compress_usingCDict.restype = sz; L.zsmi_compress_usingCDict.argtypes = [vp, sz, vp, sz, vp]
    L.zsmi_createCDictSet.restype = vp; L.zsmi_createCDictSet.argtypes = [vp, vp, u32, i32, ctypes.POINTER(i32)]
    L.zsmi_freeCDictSet.restype = None; L.zsmi_freeCDictSet.argtypes = [vp]
    L.zsmi_sizeofCDictSetMembers.restype = u32; L.zsmi_sizeofCDictSetMembers.argtypes = [vp]
    L.zsmi_compressBatchDevice_usingCDictSet.restype = i32; L.zsmi_compressBatchDevice_usingCDictSet.argtypes = [vp, vp, vp, vp, u32, vp, vp, vp, vp, vp]
    L.zsmi_compressBatchHost_usingCDictSet.restype = i32; L.zsmi_compressBatchHost_usingCDictSet.argtypes = [vp, vp, vp, vp, u32, vp, vp, vp, vp, vp]
    L.zsmi_createDDict.restype = vp; L.zsmi_createDDict.argtypes = [vp, vp, sz, ctypes.POINTER(i32)]
    L.zsmi_freeDDict.restype = None; L.zsmi_freeDDict.argtypes = [vp]
    L.zsmi_getDictID_fromDDict.restype = ctypes.c_uint; L.zsmi_getDictID_fromDDict.argtypes = [vp]
    L.zsmi_sizeofDDict.restype = sz; L.zsmi_sizeofDDict.argtypes = [vp]
    L.zsmi_decompressBatchDevice_usingDDict.restype = i32; L.zsmi_decompressBatchDevice_usingDDict.argtypes = [vp, vp, vp, vp, u32, vp, vp, vp, vp, vp]
    L.zsmi_decompressBatchHost_usingDDict.restype = i32; L.zsmi_decompressBatchHost_usingDDict.argtypes = [vp, vp, vp, vp, u32, vp, vp, vp, vp, vp]
    L.zsmi_decompress_usingDDict.restype = sz; L.zsmi_decompress_usingDDict.argtypes = [vp, sz, vp, sz, vp]
    L.zsmi_createDDictSet.restype = vp; L.zsmi_createDDictSet.argtypes = [vp, vp, u32, vp, ctypes.POINTER(i32)]
    L.zsmi_freeDDictSet.restype = None; L.zsmi_freeDDictSet.argtypes = [vp]
    L.zsmi_sizeofDDictSetMembers.restype = u32; L.zsmi_sizeofDDictSetMembers.argtypes = [vp]
    L.zsmi_decompressBatchDevice_usingDDictSet.restype = i32; L.zsmi_decompressBatchDevice_usingDDictSet.argtypes = [vp, vp, vp, vp, u32, vp, vp, vp, vp, vp]
    L.zsmi_decompressBatchHost_usingDDictSet.restype = i32; L.zsmi_decompressBatchHost_usingDDictSet.argtypes = [vp, vp, vp, vp, u32, vp, vp, vp, vp, vp]
    L.zsmi_decompress_usingDDictSet.restype = sz; L.zsmi_decompress_usingDDictSet.argtypes = [vp, sz, vp, sz, vp]
    L.zsmi_decompressBatchHost.restype = i32; L.zsmi_decompressBatchHost.argtypes = [vp, vp, vp, vp, u32, vp, vp, vp, vp]
    L.zsmi_decompressBatchHost_usingDict.restype = i32; L.zsmi_decompressBatchHost_usingDict.argtypes = [vp, vp, vp, vp, u32, vp, vp, vp, vp, vp, sz]
    L.zsmi_decompressBatchDevice_usingDict.restype = i32; L.zsmi_decompressBatchDevice_usingDict.argtypes = [vp, vp, vp, vp, u32, vp, vp, vp, vp, vp, sz]
    L.zsmi_packFramesDevice.restype = i32; L.zsmi_packFramesDevice.argtypes = [vp, vp, vp, vp, u32, vp, vp]
    ull_ = ctypes.c_ulonglong
    L.zsmi_getFrameContentSize.restype = ull_; L.zsmi_getFrameContentSize.argtypes = [vp, sz]
    L.zsmi_findFrameCompressedSize.restype = sz; L.zsmi_findFrameCompressedSize.argtypes = [vp, sz]
    L.zsmi_findDecompressedSize.restype = ull_; L.zsmi_findDecompressedSize.argtypes = [vp, sz]
    L.zsmi_decompressBound.restype = ull_; L.zsmi_decompressBound.argtypes = [vp, sz]
    L.zsmi_getFrameSizesBatchDevice.restype = i32; L.zsmi_getFrameSizesBatchDevice.argtypes = [vp, vp, vp, vp, u32, vp, vp, vp]
    L.zsmi_layoutOutputsDevice.restype = i32; L.zsmi_layoutOutputsDevice.argtypes = [vp, vp, vp, u32, u32, vp, vp]
    L.zsmi_decompressBatchResident.restype = i32; L.zsmi_decompressBatchResident.argtypes = [vp, vp, vp, vp, u32, vp, vp, vp, u32, vp, vp]
    L.zsmi_compressBoundsDevice.restype = i32; L.zsmi_compressBoundsDevice.argtypes = [vp, vp, u32, vp]
    L.zsmi_compressBatchResident.restype = i32; L.zsmi_compressBatchResident.argtypes = [vp, vp, vp, vp, u32, u32, vp, vp, vp, i32]
    L.zsmi_compressBatchResident_usingCDictSet.restype = i32; L.zsmi_compressBatchResident_usingCDictSet.argtypes = [vp, vp, vp, vp, u32, u32, vp, vp, vp, vp, vp]
    L.zsmi_enableKernelTiming.restype = i32; L.zsmi_enableKernelTiming.argtypes = [vp, i32]
    L.zsmi_getKernelTimes.restype = i32; L.zsmi_getKernelTimes.argtypes = [vp, ctypes.POINTER(KernelTime), i32]
    L.zsmi_decodeScratchBytes.restype = sz; L.zsmi_decodeScratchBytes.argtypes = [vp]
    L.zsmi_shutdown.restype = None; L.zsmi_shutdown.argtypes = []
    u64, ull, pu64 = ctypes.c_uint64, ctypes.c_ulonglong, ctypes.POINTER(ctypes.c_uint64)
    L.zsmi_seekableBound.restype = sz; L.zsmi_seekableBound.argtypes = [ull, u32, i32]
    L.zsmi_compressSeekable.restype = sz; L.zsmi_compressSeekable.argtypes = [vp, sz, vp, sz, i32, u32, i32]
    L.zsmi_compressSeekableDevice.restype = i32; L.zsmi_compressSeekableDevice.argtypes = [vp, vp, u64, vp, u64, vp, i32, u32, i32]
    L.zsmi_decompressSeekable.restype = sz; L.zsmi_decompressSeekable.argtypes = [vp, sz, vp, sz, ull]
    L.zsmi_decompressSeekableDevice.restype = i32; L.zsmi_decompressSeekableDevice.argtypes = [vp, vp, u64, u64, u64, vp, pu64, vp]
    L.zsmi_seekableNumFrames.restype = sz; L.zsmi_seekableNumFrames.argtypes = [vp, sz]
    L.zsmi_seekableContentSize.restype = sz; L.zsmi_seekableContentSize.argtypes = [vp, sz]
    L.zsmi_seekableFrameInfo.restype = i32; L.zsmi_seekableFrameInfo.argtypes = [vp, sz, u32, pu64, pu64, ctypes.POINTER(u32), ctypes.POINTER(u32)]
    L.zsmi_openSeekable.restype = vp; L.zsmi_openSeekable.argtypes = [vp, vp, sz, ctypes.POINTER(i32)]
    L.zsmi_openSeekableDevice.restype = vp; L.zsmi_openSeekableDevice.argtypes = [vp, vp, u64, ctypes.POINTER(i32)]
    L.zsmi_closeSeekable.restype = None; L.zsmi_closeSeekable.argtypes = [vp]
    L.zsmi_getNumFrames_fromSeekable.restype = sz; L.zsmi_getNumFrames_fromSeekable.argtypes = [vp]
    L.zsmi_getContentSize_fromSeekable.restype = ull; L.zsmi_getContentSize_fromSeekable.argtypes = [vp]
    L.zsmi_sizeofSeekable.restype = sz; L.zsmi_sizeofSeekable.argtypes = [vp]
    L.zsmi_seekableReadRangesDevice.restype = i32; L.zsmi_seekableReadRangesDevice.argtypes = [vp, vp, vp, vp, u32, vp, vp, vp, vp, ctypes.POINTER(u32)]
    L.zsmi_seekableReadRangesHost.restype = i32; L.zsmi_seekableReadRangesHost.argtypes = [vp, vp, vp, vp, u32, vp, sz, vp, vp]
    L.zsmi_seekableFramesBound.restype = sz; L.zsmi_seekableFramesBound.argtypes = [vp, u32, i32]
    L.zsmi_compressSeekableFramesDevice.restype = i32; L.zsmi_compressSeekableFramesDevice.argtypes = [vp, vp, vp, u32, vp, u64, vp, i32, i32]
    L.zsmi_compressSeekableFramesDevice_usingCDictSet.restype = i32
    L.zsmi_compressSeekableFramesDevice_usingCDictSet.argtypes = [vp, vp, vp, u32, vp, u64, vp, i32, vp, vp]
    L.zsmi_compressSeekableFramesHost.restype = sz; L.zsmi_compressSeekableFramesHost.argtypes = [vp, vp, sz, vp, vp, u32, i32, i32]
    L.zsmi_compressSeekableFramesHost_usingCDictSet.restype = sz
    L.zsmi_compressSeekableFramesHost_usingCDictSet.argtypes = [vp, vp, sz, vp, vp, u32, i32, vp, vp]
    L.zsmi_openSeekable_usingDDictSet.restype = vp; L.zsmi_openSeekable_usingDDictSet.argtypes = [vp, vp, sz, vp, ctypes.POINTER(i32)]
    L.zsmi_openSeekableDevice_usingDDictSet.restype = vp; L.zsmi_openSeekableDevice_usingDDictSet.argtypes = [vp, vp, u64, vp, ctypes.POINTER(i32)]
    L.zsmi_countFrames.restype = sz; L.zsmi_countFrames.argtypes = [vp, sz]
    L.zsmi_buildSeekTable.restype = sz; L.zsmi_buildSeekTable.argtypes = [vp, sz, vp, sz]
    L.zsmi_openFrames.restype = vp; L.zsmi_openFrames.argtypes = [vp, vp, sz, ctypes.POINTER(i32)]
    L.zsmi_openFramesDevice.restype = vp; L.zsmi_openFramesDevice.argtypes = [vp, vp, u64, ctypes.POINTER(i32)]
    L.zsmi_openFrames_usingDDictSet.restype = vp; L.zsmi_openFrames_usingDDictSet.argtypes = [vp, vp, sz, vp, ctypes.POINTER(i32)]
    L.zsmi_openFramesDevice_usingDDictSet.restype = vp; L.zsmi_openFramesDevice_usingDDictSet.argtypes = [vp, vp, u64, vp, ctypes.POINTER(i32)]
    L.zsmi_getFrameInfo_fromSeekable.restype = i32
    L.zsmi_getFrameInfo_fromSeekable.argtypes = [vp, u32, pu64, pu64, ctypes.POINTER(u32), ctypes.POINTER(u32)]
    L.zsmi_seekableReadFramesDevice.restype = i32; L.zsmi_seekableReadFramesDevice.argtypes = [vp, vp, vp, u32, vp, vp, vp, vp, ctypes.POINTER(u32)]
    L.zsmi_seekableReadFramesHost.restype = i32; L.zsmi_seekableReadFramesHost.argtypes = [vp, vp, vp, u32, vp, sz, vp, vp]
    L.zsmi_seekableFramesResidentBound.restype = sz; L.zsmi_seekableFramesResidentBound.argtypes = [ull, u32, i32]
    L.zsmi_compressSeekableFramesResident.restype = i32; L.zsmi_compressSeekableFramesResident.argtypes = [vp, vp, u64, vp, u32, u32, vp, u64, vp, i32, i32]
    L.zsmi_compressSeekableFramesResident_usingCDictSet.restype = i32
    L.zsmi_compressSeekableFramesResident_usingCDictSet.argtypes = [vp, vp, u64, vp, u32, u32, vp, u64, vp, i32, vp, vp]
    L.zsmi_seekableReadFramesResident.restype = i32; L.zsmi_seekableReadFramesResident.argtypes = [vp, vp, vp, u32, u32, vp, u64, vp, vp, vp]
    L.zsmi_splitRecords.restype = sz; L.zsmi_splitRecords.argtypes = [vp, sz, i32, u32, u32, vp, vp, sz, pu64]
    L.zsmi_countRecordsDevice.restype = i32; L.zsmi_countRecordsDevice.argtypes = [vp, vp, u64, i32, vp]
    L.zsmi_splitRecordsDevice.restype = i32; L.zsmi_splitRecordsDevice.argtypes = [vp, vp, u64, i32, u32, u32, u32, vp, vp, vp]
    L.zsmi_seekableRecordsWorkBound.restype = sz; L.zsmi_seekableRecordsWorkBound.argtypes = [vp, u32]
    L.zsmi_seekableReadRecordsResident.restype = i32
    L.zsmi_seekableReadRecordsResident.argtypes = [vp, vp, vp, u32, i32, vp, u32, u32, u32, vp, u64, vp, u64, vp, vp, vp, vp]
    L.zsmi_seekableReadRecordsHost.restype = i32; L.zsmi_seekableReadRecordsHost.argtypes = [vp, vp, vp, u32, i32, vp, u32, vp, sz, vp, vp]
    L.zsmi_findRecords.restype = sz; L.zsmi_findRecords.argtypes = [vp, sz, i32, vp, u32, u64, vp, sz, pu64]
    L.zsmi_findRecordsDevice.restype = i32; L.zsmi_findRecordsDevice.argtypes = [vp, vp, u64, i32, vp, u32, vp, vp, u64, vp]
    L.zsmi_seekableFindWorkBound.restype = sz; L.zsmi_seekableFindWorkBound.argtypes = [vp, u32, u32]
    L.zsmi_seekableFindRecordsResident.restype = i32
    L.zsmi_seekableFindRecordsResident.argtypes = [vp, vp, vp, u32, i32, vp, u32, u32, u32, vp, u64, vp, u64, vp]
    L.zsmi_seekableFindRecordsHost.restype = i32; L.zsmi_seekableFindRecordsHost.argtypes = [vp, vp, vp, u32, i32, vp, u32, u32, u32, vp, sz, vp]
    pq = ctypes.POINTER(FindQuery)
    L.zsmi_findRecordsQuery.restype = sz; L.zsmi_findRecordsQuery.argtypes = [vp, sz, i32, pq, u64, vp, vp, sz, pu64]
    L.zsmi_findRecordsQueryDevice.restype = i32; L.zsmi_findRecordsQueryDevice.argtypes = [vp, vp, u64, i32, pq, vp, vp, vp, u64, vp]
    L.zsmi_seekableFindQueryResident.restype = i32
    L.zsmi_seekableFindQueryResident.argtypes = [vp, vp, vp, u32, i32, pq, u32, u32, vp, u64, vp, vp, u64, vp]
    L.zsmi_seekableFindQueryHost.restype = i32; L.zsmi_seekableFindQueryHost.argtypes = [vp, vp, vp, u32, i32, pq, u32, u32, vp, vp, sz, vp]
    pr = ctypes.POINTER(RegexProgram)
    L.zsmi_compileRegex.restype = i32; L.zsmi_compileRegex.argtypes = [vp, sz, u32, pr, ctypes.POINTER(sz)]
    L.zsmi_findRecordsRegex.restype = sz; L.zsmi_findRecordsRegex.argtypes = [vp, sz, i32, pr, u64, vp, sz, pu64]
    L.zsmi_findRecordsRegexDevice.restype = i32; L.zsmi_findRecordsRegexDevice.argtypes = [vp, vp, u64, i32, pr, vp, vp, u64, vp]
    L.zsmi_seekableFindRegexResident.restype = i32
    L.zsmi_seekableFindRegexResident.argtypes = [vp, vp, vp, u32, i32, pr, u32, u32, vp, u64, vp, u64, vp]
    L.zsmi_seekableFindRegexHost.restype = i32; L.zsmi_seekableFindRegexHost.argtypes = [vp, vp, vp, u32, i32, pr, u32, u32, vp, sz, vp]
    L.zsmi_recordIndexFrameSize.restype = sz; L.zsmi_recordIndexFrameSize.argtypes = [sz]
    L.zsmi_writeRecordIndexFrame.restype = sz; L.zsmi_writeRecordIndexFrame.argtypes = [vp, sz, vp, sz, i32]
    L.zsmi_readRecordIndexFrame.restype = sz; L.zsmi_readRecordIndexFrame.argtypes = [vp, sz, vp, sz, ctypes.POINTER(i32)]
    L.zsmi_indexRecords.restype = i32; L.zsmi_indexRecords.argtypes = [vp, sz, vp, sz, i32, vp, vp]
    L.zsmi_seekableAttachRecordIndex.restype = sz; L.zsmi_seekableAttachRecordIndex.argtypes = [vp, sz, sz, vp, sz, i32]
    L.zsmi_indexRecordsDevice.restype = i32; L.zsmi_indexRecordsDevice.argtypes = [vp, vp, u64, vp, u32, i32, i32, vp, vp, vp]
    L.zsmi_seekableIndexRecordsResident.restype = i32; L.zsmi_seekableIndexRecordsResident.argtypes = [vp, vp, i32, u32, u32, vp, u64, vp, vp]
    L.zsmi_seekableLoadRecordIndexResident.restype = i32; L.zsmi_seekableLoadRecordIndexResident.argtypes = [vp, vp, vp, vp]
    L.zsmi_seekableAttachRecordIndexResident.restype = i32; L.zsmi_seekableAttachRecordIndexResident.argtypes = [vp, vp, u64, vp, vp, u32, i32]
    L.zsmi_seekableLoadRecordIndexHost.restype = i32; L.zsmi_seekableLoadRecordIndexHost.argtypes = [vp, vp, vp, vp]
    L.zsmi_seekableIndexRecordsHost.restype = i32; L.zsmi_seekableIndexRecordsHost.argtypes = [vp, vp, i32, vp, vp]
    L.zsmi_frameFilterSize.restype = sz; L.zsmi_frameFilterSize.argtypes = [sz, ctypes.c_uint]
    L.zsmi_buildFrameFilter.restype = sz; L.zsmi_buildFrameFilter.argtypes = [vp, sz, vp, sz, vp, sz, i32, ctypes.c_uint, ctypes.c_uint]
    L.zsmi_readFrameFilter.restype = i32; L.zsmi_readFrameFilter.argtypes = [vp, sz, ctypes.POINTER(FrameFilterInfo)]
    L.zsmi_filterFrames.restype = i32; L.zsmi_filterFrames.argtypes = [vp, sz, pq, u32, u32, vp, sz, vp]
    L.zsmi_buildFrameFilterDevice.restype = i32; L.zsmi_buildFrameFilterDevice.argtypes = [vp, vp, u64, vp, u32, i32, ctypes.c_uint, ctypes.c_uint, vp, u64, vp]
    L.zsmi_seekableBuildFrameFilterResident.restype = i32
    L.zsmi_seekableBuildFrameFilterResident.argtypes = [vp, vp, i32, ctypes.c_uint, ctypes.c_uint, vp, u64, vp, u64, vp]
    L.zsmi_seekableBuildFrameFilterHost.restype = i32; L.zsmi_seekableBuildFrameFilterHost.argtypes = [vp, vp, i32, ctypes.c_uint, ctypes.c_uint, vp, sz, vp]
    L.zsmi_checkFrameFilterDevice.restype = i32; L.zsmi_checkFrameFilterDevice.argtypes = [vp, vp, u64, vp]
    L.zsmi_filterFramesDevice.restype = i32; L.zsmi_filterFramesDevice.argtypes = [vp, vp, u64, pq, u32, u32, vp, u64, vp]
    L.zsmi_seekableFindFramesWorkBound.restype = sz; L.zsmi_seekableFindFramesWorkBound.argtypes = [vp, u32]
    L.zsmi_seekableFindQueryFramesResident.restype = i32
    L.zsmi_seekableFindQueryFramesResident.argtypes = [vp, vp, vp, u32, i32, pq, vp, vp, u32, vp, u64, vp, vp, u64, vp]
    L.zsmi_seekableFindQueryFramesHost.restype = i32; L.zsmi_seekableFindQueryFramesHost.argtypes = [vp, vp, vp, u32, i32, pq, vp, u32, vp, vp, sz, vp]
    pfc, psz = ctypes.POINTER(FastCoverParams), ctypes.POINTER(sz)
    L.zsmi_trainFromBuffer.restype = sz; L.zsmi_trainFromBuffer.argtypes = [vp, sz, vp, psz, ctypes.c_uint]
    L.zsmi_trainFromBuffer_fastCover.restype = sz; L.zsmi_trainFromBuffer_fastCover.argtypes = [vp, sz, vp, psz, ctypes.c_uint, pfc]
    L.zsmi_trainFromDevice.restype = i32; L.zsmi_trainFromDevice.argtypes = [vp, vp, vp, vp, u32, vp, sz, pfc, psz]
    L.zsmi_finalizeDictionary.restype = sz; L.zsmi_finalizeDictionary.argtypes = [vp, sz, vp, sz, vp, psz, ctypes.c_uint, i32, ctypes.c_uint]
    L.zsmi_getDictID.restype = ctypes.c_uint; L.zsmi_getDictID.argtypes = [vp, sz]
    if DEBUG or hasattr(L, "zsmi_dbg_copyScratch"):            # (a variant build named by ZSMI_LIB_FILE may carry the hooks too)
        L.zsmi_dbg_copyScratch.restype = i32; L.zsmi_dbg_copyScratch.argtypes = [vp, ctypes.c_char_p, vp, sz]
        L.zsmi_dbg_scratchLayout.restype = i32; L.zsmi_dbg_scratchLayout.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint64)]
    if hasattr(L, "zsmi_dbg_fillScratch"):
        L.zsmi_dbg_fillScratch.restype = i32; L.zsmi_dbg_fillScratch.argtypes = [vp, u32, ctypes.POINTER(ctypes.c_uint64)]
        L.zsmi_dbg_scratchInventory.restype = sz; L.zsmi_dbg_scratchInventory.argtypes = [ctypes.c_char_p, sz]
    _lib = L
    return L


FILL_GROUPS = ("compress", "resident", "decode", "staging", "seek", "train", "plan")      # zsmi_dbg_fillScratch's bytesFilled, in this order


def fill_scratch(ctx, pattern):
    """debug-hook library: every buffer the context keeps from call to call is overwritten (0 .. 255: that byte; any other value: a mix of
    small and large words made from it) and the compress plan forgotten.  Returns {group: bytes filled}"""
    out = (ctypes.c_uint64 * len(FILL_GROUPS))()
    rc = lib().zsmi_dbg_fillScratch(ctx, pattern, out)
    if rc != 0:
        raise RuntimeError("zsmi_dbg_fillScratch: %d" % rc)
    return dict(zip(FILL_GROUPS, (int(v) for v in out)))


def scratch_inventory(so=None):
    """debug-hook library (host code only): [(group, "filled" | "forgotten" | "state", member of zsmi_ctx.h)] - what fill_scratch covers and
    what it leaves as state.  so: the library as a ctypes.CDLL (default: the one lib() loads)"""
    so = so or lib()
    so.zsmi_dbg_scratchInventory.restype = ctypes.c_size_t; so.zsmi_dbg_scratchInventory.argtypes = [ctypes.c_char_p, ctypes.c_size_t]
    n = so.zsmi_dbg_scratchInventory(None, 0)
    buf = ctypes.create_string_buffer(n)
    so.zsmi_dbg_scratchInventory(buf, n)
    return [tuple(line.split()) for line in buf.value.decode().splitlines()]


def scratch_layout(name):
    """debug-hook library: (bytes a slot, fixed bytes behind the slots) of the scratch buffer `name` - the names and the numbers are
    csrc/zsmi_scratch.h's; KeyError for a name that is no buffer's"""
    out = (ctypes.c_uint64 * 2)()
    if lib().zsmi_dbg_scratchLayout(name.encode(), out) != 0:
        raise KeyError(name)
    return int(out[0]), int(out[1])


def copy_scratch(ctx, name, slots, extra=0):
    """debug-hook library: the first `slots` slots of the scratch buffer `name` (+ `extra` bytes behind them) as the context's last call left
    them: a uint8 array of slots * (bytes a slot) + extra"""
    import numpy as np
    buf = np.zeros(slots * scratch_layout(name)[0] + extra, dtype=np.uint8)
    rc = lib().zsmi_dbg_copyScratch(ctx, name.encode(), buf.ctypes.data_as(ctypes.c_void_p), buf.nbytes)
    if rc != 0:
        raise RuntimeError("zsmi_dbg_copyScratch(%s): %d" % (name, rc))
    return buf


EXPORTS = ["zsmi_isError", "zsmi_getErrorName", "zsmi_getErrorCode", "zsmi_decompress", "zsmi_getDecompressedSize",
           "zsmi_compress", "zsmi_compressBound", "zsmi_createCtx", "zsmi_freeCtx", "zsmi_sync",
           "zsmi_compressBatchDevice", "zsmi_decompressBatchDevice", "zsmi_compressBatchHost", "zsmi_decompressBatchHost",
           "zsmi_decompress_usingDict", "zsmi_decompressBatchDevice_usingDict", "zsmi_decompressBatchHost_usingDict",
           "zsmi_compress_usingDict", "zsmi_compressBatchDevice_usingDict", "zsmi_compressBatchHost_usingDict",
           "zsmi_createCDict", "zsmi_freeCDict", "zsmi_getDictID_fromCDict", "zsmi_sizeofCDict",
           "zsmi_compressBatchDevice_usingCDict", "zsmi_compressBatchHost_usingCDict", "zsmi_compress_usingCDict",
           "zsmi_createCDictSet", "zsmi_freeCDictSet", "zsmi_sizeofCDictSetMembers",
           "zsmi_compressBatchDevice_usingCDictSet", "zsmi_compressBatchHost_usingCDictSet",
           "zsmi_createDDict", "zsmi_freeDDict", "zsmi_getDictID_fromDDict", "zsmi_sizeofDDict",
           "zsmi_decompressBatchDevice_usingDDict", "zsmi_decompressBatchHost_usingDDict", "zsmi_decompress_usingDDict",
           "zsmi_createDDictSet", "zsmi_freeDDictSet", "zsmi_sizeofDDictSetMembers",
           "zsmi_decompressBatchDevice_usingDDictSet", "zsmi_decompressBatchHost_usingDDictSet", "zsmi_decompress_usingDDictSet",
           "zsmi_packFramesDevice", "zsmi_enableKernelTiming", "zsmi_getKernelTimes", "zsmi_versionString", "zsmi_decodeScratchBytes", "zsmi_shutdown",
           "zsmi_seekableBound", "zsmi_compressSeekable", "zsmi_compressSeekableDevice", "zsmi_decompressSeekable", "zsmi_decompressSeekableDevice",
           "zsmi_seekableNumFrames", "zsmi_seekableContentSize", "zsmi_seekableFrameInfo",
           "zsmi_openSeekable", "zsmi_openSeekableDevice", "zsmi_closeSeekable", "zsmi_getNumFrames_fromSeekable", "zsmi_getContentSize_fromSeekable",
           "zsmi_sizeofSeekable", "zsmi_seekableReadRangesDevice", "zsmi_seekableReadRangesHost",
           "zsmi_seekableFramesBound", "zsmi_compressSeekableFramesDevice", "zsmi_compressSeekableFramesDevice_usingCDictSet",
           "zsmi_compressSeekableFramesHost", "zsmi_compressSeekableFramesHost_usingCDictSet",
           "zsmi_openSeekable_usingDDictSet", "zsmi_openSeekableDevice_usingDDictSet", "zsmi_getFrameInfo_fromSeekable",
           "zsmi_countFrames", "zsmi_buildSeekTable", "zsmi_openFrames", "zsmi_openFramesDevice",
           "zsmi_openFrames_usingDDictSet", "zsmi_openFramesDevice_usingDDictSet",
           "zsmi_seekableReadFramesDevice", "zsmi_seekableReadFramesHost",
           "zsmi_seekableFramesResidentBound", "zsmi_compressSeekableFramesResident", "zsmi_compressSeekableFramesResident_usingCDictSet",
           "zsmi_seekableReadFramesResident",
           "zsmi_splitRecords", "zsmi_countRecordsDevice", "zsmi_splitRecordsDevice",
           "zsmi_seekableRecordsWorkBound", "zsmi_seekableReadRecordsResident", "zsmi_seekableReadRecordsHost",
           "zsmi_findRecords", "zsmi_findRecordsDevice", "zsmi_seekableFindWorkBound", "zsmi_seekableFindRecordsResident", "zsmi_seekableFindRecordsHost",
           "zsmi_findRecordsQuery", "zsmi_findRecordsQueryDevice", "zsmi_seekableFindQueryResident", "zsmi_seekableFindQueryHost",
           "zsmi_compileRegex", "zsmi_findRecordsRegex", "zsmi_findRecordsRegexDevice", "zsmi_seekableFindRegexResident", "zsmi_seekableFindRegexHost",
           "zsmi_recordIndexFrameSize", "zsmi_writeRecordIndexFrame", "zsmi_readRecordIndexFrame", "zsmi_indexRecords", "zsmi_seekableAttachRecordIndex",
           "zsmi_indexRecordsDevice", "zsmi_seekableIndexRecordsResident", "zsmi_seekableLoadRecordIndexResident", "zsmi_seekableAttachRecordIndexResident",
           "zsmi_seekableLoadRecordIndexHost", "zsmi_seekableIndexRecordsHost",
           "zsmi_frameFilterSize", "zsmi_buildFrameFilter", "zsmi_readFrameFilter", "zsmi_filterFrames", "zsmi_buildFrameFilterDevice",
           "zsmi_seekableBuildFrameFilterResident", "zsmi_seekableBuildFrameFilterHost", "zsmi_checkFrameFilterDevice", "zsmi_filterFramesDevice",
           "zsmi_seekableFindFramesWorkBound", "zsmi_seekableFindQueryFramesResident", "zsmi_seekableFindQueryFramesHost",
           "zsmi_trainFromBuffer", "zsmi_trainFromBuffer_fastCover", "zsmi_trainFromDevice", "zsmi_finalizeDictionary", "zsmi_getDictID",
           "zsmi_setParameter", "zsmi_getParameter", "zsmi_compress_advanced", "zsmi_compress_usingCDict_advanced",
           "zsmi_getFrameContentSize", "zsmi_findFrameCompressedSize", "zsmi_findDecompressedSize", "zsmi_decompressBound",
           "zsmi_getFrameSizesBatchDevice", "zsmi_layoutOutputsDevice", "zsmi_decompressBatchResident",
           "zsmi_compressBoundsDevice", "zsmi_compressBatchResident", "zsmi_compressBatchResident_usingCDictSet"]
