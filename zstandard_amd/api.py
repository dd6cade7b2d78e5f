"""Host-side mirror of the reference's public surface, over the C ABI of libzsmi.so.

  ZStdDecompress      static class of csharp/src/ZStdDecompress.cs:37-42 (Decompress :2182-2191, GetDecompressedSize :590-622):
                      never raises on corrupt input, returns the size or the reference's error value (uint)(-code).
  ZstdDecompressor    Java class java/src/main/java/com/epam/deltix/zstd/ZstdDecompressor.java:18-34: raises RuntimeError
                      like Util.java:32-40.
  ZstdCompressor      the compressor the reference lacks (north_star), same calling conventions.
  SeekableArchive     random access into a seekable archive (zstd's seekable format: independent frames + a seek table), made by
                      ZstdCompressor.compress_seekable or BatchCodec.compress_seekable_device - or a record archive (the caller's frame
                      sizes, a dictionary per frame: BatchCodec.compress_seekable_frames_*), read with ddict_set= / ddict= by frame number.
  SeekableHandle      an archive in device memory opened once (zsmi_openSeekableDevice): batches of range reads, every frame decoded once;
                      with a DecompressionDictSet a record archive's reader (read_frames_device).
  BatchCodec          the batch hot path on device memory (torch tensors are only a handle to device memory here).
  CompressionDict     a digested dictionary (zsmi_createCDict): parsed and laid out on the device once, used by many calls; with a
                      formatted dictionary its entropy tables code the first block of a frame where that is smaller.
  DecompressionDict   a digested decode dictionary (zsmi_createDDict): the dictionary's bytes and, for a formatted one, its entropy tables in
                      the fast decode kernels' form, on the device once; its calls decode dictionary frames on the fast path.
  DecompressionDictSet
                      a DDict set (zsmi_createDDictSet): a device table of DecompressionDicts; a decode call with it gives every frame
                      the dictionary its dictID names, so one call decodes a batch whose frames name different dictionaries.
  frame_content_size, find_frame_compressed_size, find_decompressed_size, decompress_bound
                      the size queries of a buffer of frames (zsmi_getFrameContentSize ...): host only, the container's headers alone.
                      On the device, for a batch: BatchCodec.frame_sizes_device, and with layout_outputs_device and decompress_resident
                      a decode whose descriptors never leave device memory.
  index_records, write_record_index_frame, read_record_index_frame, attach_record_index
                      the record index of a record archive (first_record, which every record call takes) as part of the archive: host
                      only.  On the device: BatchCodec.index_records_device, attach_record_index_resident, SeekableHandle.
                      load_record_index_resident, index_records_resident; SeekableArchive.first_record() loads or rebuilds it.
  train_dictionary, finalize_dictionary, get_dict_id
                      zstd dictionaries made on the GPU (fastCover and ZDICT_finalizeDictionary; zdict.h's parameters).

Everything computes on the GPU through libzsmi.so; nothing here falls back to a CPU codec.
"""
import ctypes
import numpy as np
from . import _lib

ERROR_MAX_CODE = 120            # ZSMI_error_maxCode (include/zsmi.h)
ERROR_MAX = (1 << 32) - ERROR_MAX_CODE      # ZStdErrors.cs:95-98 : IsError(c) = c > (uint)-120; csrc/zsmi_status.h states it for the library
ERROR_PREFIX_UNKNOWN = 10                   # ZSMI_error_prefix_unknown
ERROR_PARAMETER_UNSUPPORTED = 40            # ZSMI_error_parameter_unsupported
ERROR_PARAMETER_OUT_OF_BOUND = 42           # ZSMI_error_parameter_outOfBound
ERROR_FRAME_INDEX_TOO_LARGE = 100           # ZSMI_error_frameIndex_tooLarge


def _raise_if_error(L, r):
    """r: a size_t result; an error code raises RuntimeError with its name"""
    if L.zsmi_isError(r):
        raise RuntimeError(L.zsmi_getErrorName(r).decode())
    return int(r)


def _error_name(L, code: int) -> str:
    return L.zsmi_getErrorName((1 << 64) - code).decode()


def _check(rc, name):
    """rc: the int result of the C function `name`; non-zero raises RuntimeError"""
    if rc:
        raise RuntimeError(f"{name}: error {rc}")


def _buf(b):
    """bytes-like -> (ctypes pointer/obj, length)"""
    if isinstance(b, np.ndarray):
        return b.ctypes.data_as(ctypes.c_void_p), b.nbytes
    if isinstance(b, (bytes, bytearray, memoryview)):
        mv = memoryview(b)
        if isinstance(b, bytes):
            return ctypes.c_char_p(b), len(b)
        return (ctypes.c_char * len(mv)).from_buffer(b), len(mv)
    raise TypeError(type(b))


CONTENTSIZE_UNKNOWN = (1 << 64) - 1      # ZSMI_CONTENTSIZE_UNKNOWN: a frame states no content size
CONTENTSIZE_ERROR = (1 << 64) - 2        # ZSMI_CONTENTSIZE_ERROR: the frames are refused (or their sizes sum beyond 64 bits)


def frame_content_size(src) -> int:
    """what the header of the first frame of src states (zsmi_getFrameContentSize; GetFrameContentSize, ZStdDecompress.cs:518): its content
    size, CONTENTSIZE_UNKNOWN, 0 for a skippable frame, or CONTENTSIZE_ERROR.  Host only, like the three below: no device is needed."""
    s, n = _buf(src)
    return int(_lib.lib().zsmi_getFrameContentSize(s, n))


def find_frame_compressed_size(src) -> int:
    """the bytes the first frame of src takes, a skippable one included (zsmi_findFrameCompressedSize); RuntimeError with the error's name
    for a frame the container walker refuses"""
    L = _lib.lib()
    s, n = _buf(src)
    return _raise_if_error(L, L.zsmi_findFrameCompressedSize(s, n))


def find_decompressed_size(src) -> int:
    """the sum of the content sizes the frames of src state (zsmi_findDecompressedSize), CONTENTSIZE_UNKNOWN or CONTENTSIZE_ERROR"""
    s, n = _buf(src)
    return int(_lib.lib().zsmi_findDecompressedSize(s, n))


def decompress_bound(src) -> int:
    """room that holds the content of every frame of src, stated or not (zsmi_decompressBound), or CONTENTSIZE_ERROR"""
    s, n = _buf(src)
    return int(_lib.lib().zsmi_decompressBound(s, n))


def count_frames(stream) -> int:
    """the frames of a stream of frames, zstd and skippable (zsmi_countFrames: the frame index, host only); RuntimeError with the error's
    name for a stream the index refuses"""
    L = _lib.lib()
    s, n = _buf(stream)
    return _raise_if_error(L, L.zsmi_countFrames(s, n))


def build_seek_table(stream) -> bytes:
    """the seek table of the stream's frames, without checksums (zsmi_buildSeekTable, host only): stream + these bytes is a seekable archive"""
    L = _lib.lib()
    s, n = _buf(stream)
    cap = 17 + 8 * count_frames(stream)
    out = ctypes.create_string_buffer(cap)
    size = _raise_if_error(L, L.zsmi_buildSeekTable(out, cap, s, n))
    return out.raw[:size]


def _delimiter(delimiter) -> int:
    """a delimiter given as one byte (b"\\n") or as its value"""
    if isinstance(delimiter, (bytes, bytearray)):
        if len(delimiter) != 1:
            raise ValueError("the delimiter is one byte")
        return delimiter[0]
    return int(delimiter)


def split_records(data, delimiter=b"\n", target_size=0, max_frame_size=1 << 16):
    """the frames of a record archive over delimited records (zsmi_splitRecords, host only): (sizes uint32[n], first_record uint64[n + 1]).
    A record ends behind each delimiter byte; a frame holds the whole records that fit in target_size (0: a frame a record), a record above
    max_frame_size is cut at multiples of it.  first_record[i]: the records in front of frame i, first_record[n]: all.  The frame record
    r starts in: i = searchsorted(first_record, r), and i - 1 where first_record[i] != r."""
    L = _lib.lib()
    s, n = _buf(data)
    d = _delimiter(delimiter)
    records = ctypes.c_uint64(0)
    frames = _raise_if_error(L, L.zsmi_splitRecords(s, n, d, target_size, max_frame_size, None, None, 0, ctypes.byref(records)))
    sizes = np.zeros(frames, dtype=np.uint32); first = np.zeros(frames + 1, dtype=np.uint64)
    if frames:                                                             # (no frame: no record either)
        p = ctypes.c_void_p
        _raise_if_error(L, L.zsmi_splitRecords(s, n, d, target_size, max_frame_size, p(sizes.ctypes.data), p(first.ctypes.data), frames, None))
    return sizes, first


def index_records(data, frame_sizes, delimiter=b"\n"):
    """the record index of delimited text cut into frames of frame_sizes bytes (zsmi_indexRecords, host only): (first_record uint64[n + 1],
    {"records", "misaligned", "delimiters"}).  first_record[i]: the delimiters in front of frame i (+ 1 at the text's end for a tail
    without one).  misaligned: the frames that hold a delimiter, do not end on one and do not end the text - with any, a record that
    is cut need not start a frame, and the lookup of read_records / find_records does not hold."""
    L = _lib.lib()
    s, n = _buf(data)
    sizes = np.ascontiguousarray(frame_sizes, dtype=np.uint32)
    first = np.zeros(len(sizes) + 1, dtype=np.uint64); result = np.zeros(4, dtype=np.uint64)
    p = ctypes.c_void_p
    rc = L.zsmi_indexRecords(s, n, p(sizes.ctypes.data) if len(sizes) else None, len(sizes), _delimiter(delimiter), p(first.ctypes.data), p(result.ctypes.data))
    if rc:
        raise RuntimeError(_error_name(L, rc))
    return first, {"records": int(result[1]), "misaligned": int(result[2]), "delimiters": int(result[3])}


def write_record_index_frame(first_record, delimiter=b"\n") -> bytes:
    """the index frame of first_record (n + 1 entries, from 0, ascending): the skippable frame an archive carries between its last frame
    and its seek table (zsmi_writeRecordIndexFrame, host only)"""
    L = _lib.lib()
    first = np.ascontiguousarray(first_record, dtype=np.uint64)
    n = max(len(first) - 1, 0)
    cap = _raise_if_error(L, L.zsmi_recordIndexFrameSize(n))
    out = ctypes.create_string_buffer(cap)
    size = _raise_if_error(L, L.zsmi_writeRecordIndexFrame(out, cap, ctypes.c_void_p(first.ctypes.data) if len(first) else None, n, _delimiter(delimiter)))
    return out.raw[:size]


def read_record_index_frame(frame):
    """(first_record uint64[n + 1], the delimiter as one byte) of an index frame (zsmi_readRecordIndexFrame, host only); RuntimeError with
    the error's name for bytes that are no such frame, or a damaged one"""
    L = _lib.lib()
    s, size = _buf(frame)
    n = _raise_if_error(L, L.zsmi_readRecordIndexFrame(s, size, None, 0, None))
    first = np.zeros(n + 1, dtype=np.uint64)
    d = ctypes.c_int(0)
    _raise_if_error(L, L.zsmi_readRecordIndexFrame(s, size, ctypes.c_void_p(first.ctypes.data), n + 1, ctypes.byref(d)))
    return first, bytes([d.value])


def attach_record_index(archive, first_record, delimiter=b"\n") -> bytes:
    """the seekable archive with its record index attached (zsmi_seekableAttachRecordIndex, host only): first_record has the archive's
    frame count + 1 entries.  Every reader sees one more frame, an empty one; SeekableArchive.first_record() loads the index back."""
    L = _lib.lib()
    first = np.ascontiguousarray(first_record, dtype=np.uint64)
    n = max(len(first) - 1, 0)
    frame = _raise_if_error(L, L.zsmi_recordIndexFrameSize(n))
    room = np.zeros(len(archive) + frame + 12, dtype=np.uint8)
    room[:len(archive)] = np.frombuffer(bytes(archive), dtype=np.uint8)
    size = _raise_if_error(L, L.zsmi_seekableAttachRecordIndex(ctypes.c_void_p(room.ctypes.data), len(archive), len(room),
                                                               ctypes.c_void_p(first.ctypes.data) if len(first) else None, n, _delimiter(delimiter)))
    return room[:size].tobytes()


def frame_filter_size(n, log2_bits=13) -> int:
    """the bytes of a filter frame of n frames with 2^log2_bits bits each (zsmi_frameFilterSize, host only): 40 + n * 2^(log2_bits - 3)"""
    L = _lib.lib()
    return _raise_if_error(L, L.zsmi_frameFilterSize(n, log2_bits))


def build_frame_filter(data, frame_sizes, delimiter=b"\n", gram=4, log2_bits=13) -> bytes:
    """the filter frame of delimited text cut into frames of frame_sizes bytes (zsmi_buildFrameFilter, host only): a Bloom filter of
    2^log2_bits bits (9 .. 16) a frame over the frame's folded grams of `gram` bytes (3 or 4); a frame that shares a record with another is
    saturated - all ones.  filter_frames asks it which frames can hold a query's records; keep it beside the archive."""
    L = _lib.lib()
    s, n = _buf(data)
    sizes = np.ascontiguousarray(frame_sizes, dtype=np.uint32)
    cap = _raise_if_error(L, L.zsmi_frameFilterSize(len(sizes), log2_bits))
    out = ctypes.create_string_buffer(cap)
    size = _raise_if_error(L, L.zsmi_buildFrameFilter(out, cap, s, n, ctypes.c_void_p(sizes.ctypes.data) if len(sizes) else None, len(sizes), _delimiter(delimiter),
                                                      gram, log2_bits))
    return out.raw[:size]


def read_frame_filter(frame):
    """what a filter frame says of itself (zsmi_readFrameFilter, host only; magic, version, fields, size and check are judged):
    {"frames", "delimiter" (one byte), "gram", "log2_bits", "size" (the content's), "saturated" (the slots that are all ones)};
    RuntimeError with the error's name for bytes that are no such frame, or a damaged one"""
    L = _lib.lib()
    s, size = _buf(frame)
    info = _lib.FrameFilterInfo()
    rc = L.zsmi_readFrameFilter(s, size, ctypes.byref(info))
    if rc:
        raise RuntimeError(_error_name(L, rc))
    return {"frames": int(info.nFrames), "delimiter": bytes([info.delim]), "gram": int(info.gram), "log2_bits": int(info.log2Bits), "size": int(info.size),
            "saturated": int(info.saturated)}


def filter_frames(frame_filter, patterns, mode="any", ignore_case=False, first_frame=0, frame_count=None, return_info=False):
    """the frames of [first_frame, first_frame + frame_count) (None: to the filter's end) that can hold a record satisfying the query
    (find_records_query's patterns, mode, ignore_case), by the filter alone: the ascending list of their numbers - never a frame too few;
    a pattern shorter than the filter's gram, and mode 'none', pass every frame (zsmi_filterFrames, host only).  With return_info (list,
    {"tested", "saturated"}): the frames tested and the saturated ones among the list."""
    L = _lib.lib()
    s, size = _buf(frame_filter)
    q, keep = _find_query(patterns, mode, ignore_case)
    if frame_count is None:
        frame_count = max(read_frame_filter(frame_filter)["frames"] - first_frame, 0)
    result = np.zeros(4, dtype=np.uint64)
    out = np.zeros(max(frame_count, 1), dtype=np.uint32)
    rc = L.zsmi_filterFrames(s, size, ctypes.byref(q), first_frame, frame_count, ctypes.c_void_p(out.ctypes.data), frame_count, ctypes.c_void_p(result.ctypes.data))
    if rc:
        raise RuntimeError(_error_name(L, rc))
    frames = [int(v) for v in out[:int(result[1])]]
    return (frames, {"tested": int(result[2]), "saturated": int(result[3])}) if return_info else frames


def find_records(data, pattern, delimiter=b"\n", base=0):
    """the records of delimited text that hold `pattern`, a literal byte string of 1 .. 256 bytes without the delimiter (zsmi_findRecords,
    host only): the list of their numbers, ascending - base + the delimiters in front of an occurrence.  Overlapping occurrences all
    count, a record with several is listed once."""
    L = _lib.lib()
    s, n = _buf(data)
    pat = bytes(pattern)
    d = _delimiter(delimiter)
    total = _raise_if_error(L, L.zsmi_findRecords(s, n, d, pat, len(pat), base, None, 0, None))
    out = np.zeros(max(total, 1), dtype=np.uint64)
    _raise_if_error(L, L.zsmi_findRecords(s, n, d, pat, len(pat), base, ctypes.c_void_p(out.ctypes.data), total, None))
    return [int(v) for v in out[:total]]


FIND_MODES = {"any": 0, "all": 1, "none": 2}


def _find_query(patterns, mode, ignore_case):
    """(zsmi_findQuery, the buffers its pointers name - keep them until the call returns): the patterns are HOST bytes, read during the call"""
    if mode not in FIND_MODES:
        raise ValueError("mode is one of 'any', 'all', 'none'")
    pats = [bytes(p) for p in patterns]
    q = _lib.FindQuery()
    q.nPatterns, q.mode, q.flags = len(pats), FIND_MODES[mode], 1 if ignore_case else 0
    keep = [ctypes.create_string_buffer(p, max(len(p), 1)) for p in pats[:8]]
    for j, buf in enumerate(keep):
        q.patterns[j] = ctypes.cast(buf, ctypes.c_void_p)
        q.patternSizes[j] = len(pats[j])
    return q, keep


def find_records_query(data, patterns, mode="any", ignore_case=False, delimiter=b"\n", base=0, return_hits=False):
    """the records of delimited text that hold any of `patterns`, all of them, or none (mode; 'none' is grep -v and lists empty records
    too): 1 .. 8 literal byte strings of 256 bytes together, none with the delimiter; ignore_case folds 'A' .. 'Z' only (zsmi_findRecordsQuery,
    host only).  The list of their numbers, ascending; with return_hits (numbers, hits): hits[k] has bit j set where pattern j occurs in
    record numbers[k]."""
    L = _lib.lib()
    s, n = _buf(data)
    d = _delimiter(delimiter)
    q, keep = _find_query(patterns, mode, ignore_case)
    total = _raise_if_error(L, L.zsmi_findRecordsQuery(s, n, d, ctypes.byref(q), base, None, None, 0, None))
    out = np.zeros(max(total, 1), dtype=np.uint64); hits = np.zeros(max(total, 1), dtype=np.uint8)
    _raise_if_error(L, L.zsmi_findRecordsQuery(s, n, d, ctypes.byref(q), base, ctypes.c_void_p(out.ctypes.data), ctypes.c_void_p(hits.ctypes.data), total, None))
    records = [int(v) for v in out[:total]]
    return (records, [int(v) for v in hits[:total]]) if return_hits else records


def compile_regex(pattern, ignore_case=False, invert=False):
    """a regular expression (bytes: literals, escapes, \\d \\w \\s, `.`, classes, groups, |, * + ?, {m,n}, ^ first and $ last in a
    top-level alternative) compiled into the program the regular-expression searches take - the minimal DFA, at most 64 states
    (zsmi_compileRegex, host only): a _lib.RegexProgram.  ignore_case folds ASCII letters only; invert lists the records that do NOT
    match.  A pattern the compiler refuses raises ValueError with the error's name and the offset at which it was decided."""
    L = _lib.lib()
    pat = bytes(pattern)
    prog = _lib.RegexProgram()
    at = ctypes.c_size_t(0)
    rc = L.zsmi_compileRegex(pat, len(pat), (1 if ignore_case else 0) | (2 if invert else 0), ctypes.byref(prog), ctypes.byref(at))
    if rc:
        raise ValueError(f"zsmi_compileRegex: {_error_name(L, rc)} at offset {at.value}")
    return prog


def _regex(regex):
    """a compiled program as it is, bytes compiled on the spot"""
    return regex if isinstance(regex, _lib.RegexProgram) else compile_regex(regex)


def find_records_regex(data, regex, delimiter=b"\n", base=0):
    """the records of delimited text that `regex` matches - a compile_regex program, or bytes that are compiled on the spot - as
    re.compile(pattern, re.DOTALL).search on each record without its delimiter would (zsmi_findRecordsRegex, host only): the list of
    their numbers, ascending; an inverted program lists the others, empty records included."""
    L = _lib.lib()
    s, n = _buf(data)
    d = _delimiter(delimiter)
    prog = _regex(regex)
    total = _raise_if_error(L, L.zsmi_findRecordsRegex(s, n, d, ctypes.byref(prog), base, None, 0, None))
    out = np.zeros(max(total, 1), dtype=np.uint64)
    _raise_if_error(L, L.zsmi_findRecordsRegex(s, n, d, ctypes.byref(prog), base, ctypes.c_void_p(out.ctypes.data), total, None))
    return [int(v) for v in out[:total]]


class ZStdDecompress:
    """EPAM.Deltix.ZStd.ZStdDecompress (static). Sizes are 32-bit in the reference (size_t = UInt32, ZStdDecompress.cs:14)."""

    @staticmethod
    def Decompress(dst, src, dstCapacity=None, srcSize=None) -> int:
        L = _lib.lib()
        d, dn = _buf(dst)
        s, sn = _buf(src)
        r = L.zsmi_decompress(d, dn if dstCapacity is None else dstCapacity, s, sn if srcSize is None else srcSize)
        return r & 0xFFFFFFFF

    @staticmethod
    def GetDecompressedSize(src, srcSize=None) -> int:
        L = _lib.lib()
        s, sn = _buf(src)
        return int(L.zsmi_getDecompressedSize(s, sn if srcSize is None else srcSize))

    @staticmethod
    def IsError(code: int) -> bool:
        return (code & 0xFFFFFFFF) > ERROR_MAX


class ZstdDecompressor:
    """com.epam.deltix.zstd.ZstdDecompressor"""

    def decompress(self, input, inputOffset, inputLength, output, outputOffset, maxOutputLength) -> int:
        L = _lib.lib()
        src = bytes(memoryview(input)[inputOffset:inputOffset + inputLength])
        tmp = ctypes.create_string_buffer(max(maxOutputLength, 1))
        r = L.zsmi_decompress(tmp, maxOutputLength, src, len(src))
        if L.zsmi_isError(r):
            raise RuntimeError(f"{L.zsmi_getErrorName(r).decode()}: offset={inputOffset}")     # Util.java:32-40
        memoryview(output)[outputOffset:outputOffset + r] = tmp.raw[:r]
        return int(r)

    @staticmethod
    def getDecompressedSize(input, offset, length) -> int:
        L = _lib.lib()
        src = bytes(memoryview(input)[offset:offset + length])
        if len(src) < 5 or src[:4] != b"\x28\xb5\x2f\xfd":
            raise RuntimeError("Invalid magic prefix: offset=%d" % offset)                      # ZstdFrameDecompressor.java:928
        fhd = src[4]
        if (fhd >> 6) == 0 and not (fhd >> 5) & 1:
            return -1                                                                             # :922 returns -1 when absent
        return int(L.zsmi_getDecompressedSize(src, len(src)))


class CompressionDict:
    """A digested dictionary (ZSTD_createCDict): `dictionary` (raw content or a formatted dictionary) parsed, checked and laid out in the
    device memory of `codec`'s device once, with the level bound.  Any BatchCodec of that device may use it (cdict=); it must stay open
    until the work queued with it is done (BatchCodec.sync)."""

    def __init__(self, codec, dictionary, level=3):
        self.L = codec.L
        self.level = level
        err = ctypes.c_int(0)
        dic = bytes(dictionary)
        self.handle = self.L.zsmi_createCDict(codec.ctx, dic, len(dic), level, ctypes.byref(err))
        if not self.handle:
            raise RuntimeError(f"zsmi_createCDict: error {err.value} ({_error_name(self.L, err.value)})")

    @property
    def dict_id(self) -> int:
        return int(self.L.zsmi_getDictID_fromCDict(self.handle))

    @property
    def device_bytes(self) -> int:
        return int(self.L.zsmi_sizeofCDict(self.handle))

    def as_set(self, codec):
        """the set {self} (made once, kept and closed with the dictionary): what a call that takes sets alone is given for cdict="""
        if getattr(self, "_set", None) is None:
            self._set = CompressionDictSet(codec, [self], level=self.level)
        return self._set

    def close(self):
        if getattr(self, "_set", None) is not None:
            self._set.close()
            self._set = None
        if self.handle:
            self.L.zsmi_freeCDict(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


NO_DICT = 0xFFFFFFFF            # ZSMI_DICT_NONE: a dict_index entry for a chunk that uses no dictionary


class CompressionDictSet:
    """A CDict set: a read-only device table of the CompressionDicts `cdicts` (formatted, raw content or empty; all of `level`), in their
    order.  A compress call with it (cdict_set=, dict_index=) compresses chunk i with member dict_index[i], or without a dictionary for
    NO_DICT or an empty member: each frame is the one the cdict= call with that member gives.  The set copies nothing: the members are
    kept alive with it, and it must stay open until the work queued with it is done (BatchCodec.sync).  len(): its members."""

    def __init__(self, codec, cdicts, level=3):
        self.L = codec.L
        self.level = level
        self.members = list(cdicts)                  # (kept alive with the set)
        arr = (ctypes.c_void_p * max(len(self.members), 1))(*[d.handle for d in self.members])
        err = ctypes.c_int(0)
        self.handle = self.L.zsmi_createCDictSet(codec.ctx, arr, len(self.members), level, ctypes.byref(err))
        if not self.handle:
            raise RuntimeError(f"zsmi_createCDictSet: error {err.value} ({_error_name(self.L, err.value)})")

    def __len__(self) -> int:
        return int(self.L.zsmi_sizeofCDictSetMembers(self.handle))

    def close(self):
        if self.handle:
            self.L.zsmi_freeCDictSet(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DecompressionDict:
    """A digested decode dictionary (ZSTD_createDDict): `dictionary` (raw content or a formatted dictionary) parsed, checked and laid out in
    the device memory of `codec`'s device once.  Any BatchCodec of that device may use it (ddict=): results are those of the call with the
    dictionary's bytes, and frames that name it decode on the fast path.  It must stay open until the work queued with it is done
    (BatchCodec.sync).  An empty dictionary makes a DecompressionDict whose calls are the plain calls."""

    def __init__(self, codec, dictionary):
        self.L = codec.L
        err = ctypes.c_int(0)
        dic = bytes(dictionary or b"")
        self.handle = self.L.zsmi_createDDict(codec.ctx, dic if dic else None, len(dic), ctypes.byref(err))
        if not self.handle:
            raise RuntimeError(f"zsmi_createDDict: error {err.value} ({_error_name(self.L, err.value)})")

    @property
    def dict_id(self) -> int:
        return int(self.L.zsmi_getDictID_fromDDict(self.handle))

    @property
    def device_bytes(self) -> int:
        return int(self.L.zsmi_sizeofDDict(self.handle))

    def close(self):
        if self.handle:
            self.L.zsmi_freeDDict(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DecompressionDictSet:
    """A DDict set (ZSTD_d_refMultipleDDicts): a read-only device table of the formatted DecompressionDicts `ddicts`.  A decode call with it
    (ddict_set=) decodes every frame with the member its dictID names (no such member: dictionary_wrong for that item) and a frame that names
    no dictionary with `unnamed` (None: without one); a formatted `unnamed` is also a member under its own ID.  The set copies nothing: the
    members must stay open as long as the set, and the set until the work queued with it is done (BatchCodec.sync).  len(): its members."""

    def __init__(self, codec, ddicts, unnamed=None):
        self.L = codec.L
        self.members = list(ddicts)                  # (kept alive with the set)
        self.unnamed = unnamed
        arr = (ctypes.c_void_p * max(len(self.members), 1))(*[d.handle for d in self.members])
        err = ctypes.c_int(0)
        self.handle = self.L.zsmi_createDDictSet(codec.ctx, arr, len(self.members), unnamed.handle if unnamed is not None else None, ctypes.byref(err))
        if not self.handle:
            raise RuntimeError(f"zsmi_createDDictSet: error {err.value} ({_error_name(self.L, err.value)})")

    def __len__(self) -> int:
        return int(self.L.zsmi_sizeofDDictSetMembers(self.handle))

    def close(self):
        if self.handle:
            self.L.zsmi_freeDDictSet(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ZstdCompressor:
    """One frame per call; level <= 2 fast parameters, level >= 3 default parameters.  dictionary: raw content or a formatted
    dictionary (ZSTD_compress_usingDict), or a CompressionDict (ZSTD_compress_usingCDict: its level holds); the frames decode with the
    same dictionary (zsmi_decompress_usingDict).  checksum: the frames of compress() carry a Content_Checksum (ZSTD_c_checksumFlag: the
    low 32 bits of the content's XXH64 behind the last block, which every zstd decoder verifies); nothing else about them changes."""

    def __init__(self, level=3, dictionary=None, checksum=False):
        self.level = level
        self.checksum = bool(checksum)
        self.cdict = dictionary if isinstance(dictionary, CompressionDict) else None
        self.dictionary = bytes(dictionary) if dictionary and not self.cdict else b""

    @staticmethod
    def compressBound(n: int) -> int:
        return int(_lib.lib().zsmi_compressBound(n))

    def compress(self, src) -> bytes:
        L = _lib.lib()
        s, sn = _buf(src)
        cap = L.zsmi_compressBound(sn)
        out = ctypes.create_string_buffer(cap)
        call = (L.zsmi_compress_usingCDict_advanced, self.cdict.handle, 1) if self.cdict and self.checksum else \
               (L.zsmi_compress_advanced, self.dictionary or None, len(self.dictionary), self.level, 1) if self.checksum else \
               (L.zsmi_compress_usingCDict, self.cdict.handle) if self.cdict else \
               (L.zsmi_compress_usingDict, self.dictionary, len(self.dictionary), self.level) if self.dictionary else \
               (L.zsmi_compress, self.level)
        r = call[0](out, cap, s, sn, *call[1:])
        if L.zsmi_isError(r):
            raise RuntimeError(L.zsmi_getErrorName(r).decode())
        return out.raw[:r]

    def compress_seekable(self, src, frame_size=0, checksum=True) -> bytes:
        """a seekable archive: frame i holds src[i * frame_size, (i + 1) * frame_size) (frame_size 0: 64 KiB), each compressed as
        compress() would compress that slice, then the seek table (checksum: each entry carries the low 32 bits of the slice's XXH64).
        Any zstd decoder reads it as concatenated frames; SeekableArchive reads ranges of it."""
        L = _lib.lib()
        if self.dictionary or self.cdict:
            raise RuntimeError(_error_name(L, ERROR_PARAMETER_UNSUPPORTED))                     # parameter_unsupported: no dictionaries in seekable archives
        s, sn = _buf(src)
        cap = _raise_if_error(L, L.zsmi_seekableBound(sn, frame_size, int(bool(checksum))))
        out = ctypes.create_string_buffer(cap)
        r = _raise_if_error(L, L.zsmi_compressSeekable(out, cap, s, sn, self.level, frame_size, int(bool(checksum))))
        return out.raw[:r]


class SeekableArchive:
    """A seekable archive in host memory.  The table is checked when the object is made (RuntimeError with the error's name, as every
    read); read() decodes on the GPU only the frames that overlap the range.  read_many() reads a batch of ranges through an opened
    archive (zsmi_openSeekable: the frames go to device memory once, at the first call; close() frees them), every frame the batch
    touches decoded once."""

    def __init__(self, archive, ddict=None, ddict_set=None, frames=False):
        """ddict_set: a DecompressionDictSet the batch reads (read_many, read_frames) decode with - a record archive's dictionaries; ddict:
        one DecompressionDict instead, the set ({}, unnamed=ddict).  Either must stay open as long as this object; read() takes none.
        frames: `archive` is a stream of frames without a table, opened through its frame index (from_frames)."""
        if ddict is not None and ddict_set is not None:
            raise ValueError("ddict_set= excludes ddict=")
        self.L = _lib.lib()
        self.codec = self.handle = self._own_set = self._index = self._filter_key = self._filter_ref = None
        self.ddict, self.ddict_set = ddict, ddict_set
        self.archive = bytes(archive)
        self.frames = bool(frames)
        if self.frames:
            self.num_frames = count_frames(self.archive)
            self.content_size = find_decompressed_size(self.archive)         # (every frame states its size: the index refuses one that does not)
        else:
            self.num_frames = _raise_if_error(self.L, self.L.zsmi_seekableNumFrames(self.archive, len(self.archive)))
            self.content_size = _raise_if_error(self.L, self.L.zsmi_seekableContentSize(self.archive, len(self.archive)))

    @classmethod
    def from_frames(cls, stream, ddict=None, ddict_set=None):
        """any stream of frames - no seek table needed: the packed output of a batch compress call, concatenated .zst files, a log of one
        frame a record.  The frames are found by the frame index (zsmi_openFrames), skippable frames are entries of size 0; read_many /
        read_frames / frame_info as for an archive, and read() is read_many's one range.  The index is checked when the object is made."""
        return cls(stream, ddict=ddict, ddict_set=ddict_set, frames=True)

    def close(self):
        if self.handle:
            self.L.zsmi_closeSeekable(self.handle)
            self.handle = None
        if self._own_set is not None:
            self._own_set.close()
            self._own_set = None
        if self.codec is not None:
            self.codec.close()
            self.codec = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _open(self):
        if self.handle is not None:
            return
        self.codec = self.codec or BatchCodec()
        dset = self.ddict_set
        if self.ddict is not None:
            if self._own_set is None:
                self._own_set = DecompressionDictSet(self.codec, [], unnamed=self.ddict)
            dset = self._own_set
        err = ctypes.c_int(0)
        open_call = self.L.zsmi_openFrames_usingDDictSet if self.frames else self.L.zsmi_openSeekable_usingDDictSet
        self.handle = open_call(self.codec.ctx, self.archive, len(self.archive), dset.handle if dset is not None else None, ctypes.byref(err))
        if not self.handle:
            self.handle = None
            raise RuntimeError(_error_name(self.L, err.value))

    def _results(self, out, written, codes, n, what, return_codes):
        codes = [int(c) for c in codes[:n]]
        if not return_codes:
            for r, c in enumerate(codes):
                if c:
                    raise RuntimeError(f"{_error_name(self.L, c)} ({what} {r})")
        ends = np.cumsum(written[:n]).astype(np.int64)
        res = [out[int(e) - int(w):int(e)].tobytes() for e, w in zip(ends, written[:n])]
        return (res, codes) if return_codes else res

    def read_frames(self, indices, return_codes=False):
        """records by number: the list of the contents of the frames `indices` name, one call for all of them (zsmi_seekableReadFramesHost);
        every frame is decoded once, however often it is named.  Errors and return_codes as read_many; an index that is no frame's raises
        RuntimeError (frameIndex_tooLarge) before anything is read."""
        self._open()
        idx = [int(i) + self.num_frames if int(i) < 0 else int(i) for i in indices]
        idx = np.array([i if 0 <= i <= 0xFFFFFFFF else 0xFFFFFFFF for i in idx], dtype=np.uint32)
        n = len(idx)
        if n and int(idx.max()) >= self.num_frames:
            raise RuntimeError(_error_name(self.L, ERROR_FRAME_INDEX_TOO_LARGE))                     # frameIndex_tooLarge (before the capacity is worked out)
        cap = int(sum(self.frame_info(int(i))[3] for i in idx))
        out = np.empty(max(cap, 1), dtype=np.uint8)
        written = np.zeros(max(n, 1), dtype=np.uint64); codes = np.zeros(max(n, 1), dtype=np.uint32)
        p = BatchCodec._p
        rc = self.L.zsmi_seekableReadFramesHost(self.codec.ctx, self.handle, p(idx), n, p(out), cap, p(written), p(codes))
        if rc:
            raise RuntimeError(_error_name(self.L, rc))
        return self._results(out, written, codes, n, "frame", return_codes)

    def read_records(self, first_record, indices, delimiter=b"\n", return_codes=False):
        """records by number from a record archive: first_record is split_records' second array for the text the archive was made from
        (num_frames + 1 entries), indices the record numbers -> the list of the records' bytes, each with its delimiter, one call for all
        of them (zsmi_seekableReadRecordsHost).  Numbers in a row that lie in the same frames decode them once.  The records' lengths are
        known only behind the decode, so a first call without a destination sizes the second.  Errors and return_codes as read_many
        (frameIndex_tooLarge, 100, for a number that is no record's)."""
        self._open()
        first = np.ascontiguousarray(first_record, dtype=np.uint64)
        idx = np.ascontiguousarray([int(i) for i in indices], dtype=np.uint64)
        n, d = len(idx), _delimiter(delimiter)
        off = np.zeros(n + 1, dtype=np.uint64); codes = np.zeros(max(n, 1), dtype=np.uint32)
        p = BatchCodec._p
        out = np.empty(1, dtype=np.uint8)
        for cap in (0, None):
            cap = int(off[n]) if cap is None else cap
            out = np.empty(max(cap, 1), dtype=np.uint8)
            rc = self.L.zsmi_seekableReadRecordsHost(self.codec.ctx, self.handle, p(first), max(len(first) - 1, 0), d, p(idx), n, p(out), cap, p(off), p(codes))
            if rc:
                raise RuntimeError(_error_name(self.L, rc))
        return self._results(out, np.diff(off), codes, n, "record", return_codes)

    def first_record(self, delimiter=b"\n", allow_misaligned=False):
        """the array read_records and the find calls take (uint64[num_frames + 1]): loaded from the archive's index frame when it
        carries one (zsmi_seekableLoadRecordIndexHost; written for another delimiter: ValueError), else rebuilt from the content
        (zsmi_seekableIndexRecordsHost: one decode of the archive).  A rebuilt index with misaligned frames - frames that hold a
        delimiter, do not end on one and do not end the content, as fixed-size frames over text do - does not support the lookup of
        the record calls: ValueError, unless allow_misaligned.  A frame that fails raises RuntimeError with the error's name."""
        self._open()
        d = _delimiter(delimiter)
        first = np.zeros(self.num_frames + 1, dtype=np.uint64)
        result = np.zeros(4, dtype=np.uint64)
        p = BatchCodec._p
        rc = self.L.zsmi_seekableLoadRecordIndexHost(self.codec.ctx, self.handle, p(first), p(result))
        if rc:
            raise RuntimeError(_error_name(self.L, rc))
        if int(result[0]) == 0:
            if int(result[2]) != d:
                raise ValueError("the archive's record index was written for delimiter %d" % int(result[2]))
            return first
        if int(result[0]) != ERROR_PREFIX_UNKNOWN:
            raise RuntimeError(_error_name(self.L, int(result[0])))
        rc = self.L.zsmi_seekableIndexRecordsHost(self.codec.ctx, self.handle, d, p(first), p(result))
        if rc or int(result[0]):
            raise RuntimeError(_error_name(self.L, rc or int(result[0])))
        if int(result[2]) and not allow_misaligned:
            raise ValueError("%d frames are misaligned: records that are cut need not start a frame (allow_misaligned=True returns the array all the same)" % int(result[2]))
        return first

    def find_records(self, first_record, pattern, delimiter=b"\n", first_frame=0, frame_count=None):
        """the records of a record archive that hold `pattern` (a literal byte string of 1 .. 256 bytes without the delimiter): the list
        of their numbers, ascending, as read_records takes them.  first_record is split_records' second array for the text the archive
        was made from; first_frame and frame_count (None: to the archive's end) name a window of frames - an occurrence across its
        border is not found, and windows that start where first_record changes cut none.  A first call counts, the second is sized by
        it (zsmi_seekableFindRecordsHost); a frame that fails raises RuntimeError with the error's name."""
        self._open()
        first = np.ascontiguousarray(first_record, dtype=np.uint64)
        pat, d = bytes(pattern), _delimiter(delimiter)
        count = self.num_frames - first_frame if frame_count is None else frame_count
        p = BatchCodec._p
        return self._find_sized(lambda out, hits, cap, result: self.L.zsmi_seekableFindRecordsHost(
            self.codec.ctx, self.handle, p(first), max(len(first) - 1, 0), d, pat, len(pat), first_frame, count, out, cap, result))[0]

    def _find_sized(self, call, sets=False):
        """the host forms of the searches, whose answer's size only the search knows: a first call counts (capacity 0), the second is
        sized by the count.  call(out, hits, cap, result) -> rc makes the C call with these four arguments (pointers; out and hits None
        at capacity 0; hits a byte a number, asked for with sets).  (numbers, hit sets); a refusal or a frame that fails raises
        RuntimeError with the error's name"""
        p = BatchCodec._p
        result = np.zeros(4, dtype=np.uint64)
        for cap in (0, None):
            cap = int(result[0]) if cap is None else cap
            out = np.zeros(max(cap, 1), dtype=np.uint64); hits = np.zeros(max(cap, 1), dtype=np.uint8)
            rc = call(p(out) if cap else None, p(hits) if cap and sets else None, cap, p(result))
            if rc:
                raise RuntimeError(_error_name(self.L, rc))
            if int(result[0]) > (1 << 64) - ERROR_MAX_CODE:
                raise RuntimeError(_error_name(self.L, (1 << 64) - int(result[0])))
            if int(result[0]) == 0:
                return [], []
        n = int(result[1])
        return [int(v) for v in out[:n]], [int(v) for v in hits[:n]]

    def build_frame_filter(self, delimiter=b"\n", gram=4, log2_bits=13) -> bytes:
        """the archive's filter frame (build_frame_filter states it), built on the GPU from one decode of the archive in windows of at
        most 256 MiB of content (zsmi_seekableBuildFrameFilterHost): bytes to keep beside the archive and hand to
        find_records_query(frame_filter=...).  A frame that fails raises RuntimeError with the error's name."""
        self._open()
        cap = frame_filter_size(self.num_frames, log2_bits)
        out = np.zeros(cap, dtype=np.uint8)
        result = np.zeros(4, dtype=np.uint64)
        p = BatchCodec._p
        rc = self.L.zsmi_seekableBuildFrameFilterHost(self.codec.ctx, self.handle, _delimiter(delimiter), gram, log2_bits, p(out), cap, p(result))
        if rc or int(result[0]):
            raise RuntimeError(_error_name(self.L, rc or int(result[0])))
        return out[:int(result[1])].tobytes()

    def _filter_frames(self, frame_filter, patterns, mode, ignore_case, delimiter, first_frame, count):
        """the window's frames that pass the filter (uint32, ascending).  The filter is judged - check word included - once an object and
        filter, not once a search"""
        key = (id(frame_filter), len(frame_filter))
        if self._filter_key != key:
            info = read_frame_filter(frame_filter)
            if (info["frames"], info["size"], info["delimiter"][0]) != (self.num_frames, self.content_size, _delimiter(delimiter)):
                raise ValueError("the frame filter was built for another archive or delimiter")
            self._filter_key, self._filter_ref = key, frame_filter         # (the reference keeps the id the filter's)
        return np.asarray(filter_frames(frame_filter, patterns, mode, ignore_case, first_frame, count), dtype=np.uint32)

    def find_records_query(self, first_record, patterns, mode="any", ignore_case=False, delimiter=b"\n", first_frame=0, frame_count=None, return_hits=False,
                           frame_filter=None):
        """find_records for a query of 1 .. 8 patterns: the records of the window that hold any of them, all of them or none (mode), with
        or without ASCII case folding, after ONE decode of the window (find_records_query states the rule; the window as in find_records).
        The list of their numbers, ascending; with return_hits (numbers, hits).  zsmi_seekableFindQueryHost
        frame_filter: the archive's filter frame (build_frame_filter) - the filter is asked first and only the frames that pass are
        decoded and searched, in one call (zsmi_seekableFindQueryFramesHost); the answer is exactly the one without it (a list the
        filter writes never separates a record's frames).  Mode 'none', which no filter can help, takes the window search."""
        self._open()
        first = np.ascontiguousarray(first_record, dtype=np.uint64)
        q, keep = _find_query(patterns, mode, ignore_case)
        d = _delimiter(delimiter)
        count = self.num_frames - first_frame if frame_count is None else frame_count
        p = BatchCodec._p
        frames = None
        if frame_filter is not None and mode != "none":
            frames = self._filter_frames(frame_filter, patterns, mode, ignore_case, delimiter, first_frame, count)
        n = max(len(first) - 1, 0)
        if frames is not None:
            def call(out, hits, cap, result):
                return self.L.zsmi_seekableFindQueryFramesHost(self.codec.ctx, self.handle, p(first), n, d, ctypes.byref(q), p(frames) if len(frames) else None, len(frames),
                                                               out, hits, cap, result)
        else:
            def call(out, hits, cap, result):
                return self.L.zsmi_seekableFindQueryHost(self.codec.ctx, self.handle, p(first), n, d, ctypes.byref(q), first_frame, count, out, hits, cap, result)
        records, hits = self._find_sized(call, sets=True)
        return (records, hits) if return_hits else records

    def find_records_regex(self, first_record, regex, delimiter=b"\n", first_frame=0, frame_count=None):
        """find_records for a regular expression: the records of the window that `regex` (a compile_regex program, or bytes compiled on
        the spot) matches, after ONE decode of the window (find_records_regex states the rule; the window as in find_records - a record
        its border cuts is judged on the part inside).  The list of their numbers, ascending.  zsmi_seekableFindRegexHost"""
        self._open()
        first = np.ascontiguousarray(first_record, dtype=np.uint64)
        prog = _regex(regex)
        d = _delimiter(delimiter)
        count = self.num_frames - first_frame if frame_count is None else frame_count
        p = BatchCodec._p
        return self._find_sized(lambda out, hits, cap, result: self.L.zsmi_seekableFindRegexHost(
            self.codec.ctx, self.handle, p(first), max(len(first) - 1, 0), d, ctypes.byref(prog), first_frame, count, out, cap, result))[0]

    def read_many(self, ranges, return_codes=False):
        """ranges: (offset, length) pairs -> the list of their bytes (each clipped at the content's end), one call for all of them
        (zsmi_seekableReadRangesHost).  A failing range raises RuntimeError with the error's name and the range's index; with
        return_codes=True nothing raises for a range and the result is (list, codes): codes[r] is 0 or range r's error code, whose
        bytes are then unspecified."""
        self._open()
        ranges = list(ranges)
        n = len(ranges)
        off = np.array([r[0] for r in ranges], dtype=np.uint64); ln = np.array([r[1] for r in ranges], dtype=np.uint64)
        if n and int(off.max()) > self.content_size:
            raise RuntimeError(_error_name(self.L, ERROR_PARAMETER_OUT_OF_BOUND))                    # parameter_outOfBound (before the capacity is worked out)
        cap = int(sum(min(int(l), self.content_size - int(o)) for o, l in zip(off, ln)))
        out = np.empty(max(cap, 1), dtype=np.uint8)
        written = np.zeros(max(n, 1), dtype=np.uint64); codes = np.zeros(max(n, 1), dtype=np.uint32)
        p = BatchCodec._p
        rc = self.L.zsmi_seekableReadRangesHost(self.codec.ctx, self.handle, p(off), p(ln), n, p(out), cap, p(written), p(codes))
        if rc:
            raise RuntimeError(_error_name(self.L, rc))
        return self._results(out, written, codes, n, "range", return_codes)

    def frame_info(self, index):
        """(compressed offset, content offset, compressed size, content size) of frame `index`"""
        co, do, cs, ds = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint32(), ctypes.c_uint32()
        if index < 0:
            index += self.num_frames
        index = index if 0 <= index <= 0xFFFFFFFF else 0xFFFFFFFF          # (out of range either way: frameIndex_tooLarge)
        if self.handle is not None:                                          # (an opened archive: its parsed table, no re-parse)
            rc = self.L.zsmi_getFrameInfo_fromSeekable(self.handle, index, ctypes.byref(co), ctypes.byref(do), ctypes.byref(cs), ctypes.byref(ds))
        elif self.frames:                                                    # (a stream not opened yet: the table the index writes, once)
            if self._index is None:
                self._index = np.frombuffer(build_seek_table(self.archive), dtype="<u4", count=2 * self.num_frames, offset=8).reshape(-1, 2).astype(np.uint64)
            if index >= self.num_frames:
                raise RuntimeError(_error_name(self.L, ERROR_FRAME_INDEX_TOO_LARGE))
            c, d = self._index[:index, 0].sum(), self._index[:index, 1].sum()
            return int(c), int(d), int(self._index[index, 0]), int(self._index[index, 1])
        else:
            rc = self.L.zsmi_seekableFrameInfo(self.archive, len(self.archive), index, ctypes.byref(co),
                                               ctypes.byref(do), ctypes.byref(cs), ctypes.byref(ds))
        if rc:
            raise RuntimeError(_error_name(self.L, rc))
        return co.value, do.value, cs.value, ds.value

    def read(self, offset=0, length=None) -> bytes:
        """content bytes [offset, offset + length), clipped at the content's end (length None: to the end)"""
        if length is None:
            length = max(self.content_size - offset, 0)
        if self.frames:
            return self.read_many([(offset, length)])[0]
        out = ctypes.create_string_buffer(max(length, 1))
        r = _raise_if_error(self.L, self.L.zsmi_decompressSeekable(out, length, self.archive, len(self.archive), offset))
        return out.raw[:r]


def _samples(samples):
    """a list of bytes-likes, or (buffer, sizes) -> (contiguous uint8 array, size_t array)"""
    if isinstance(samples, tuple):
        buf, sizes = samples
        buf = np.frombuffer(bytes(buf), dtype=np.uint8) if not isinstance(buf, np.ndarray) else np.ascontiguousarray(buf, dtype=np.uint8)
        sizes = np.ascontiguousarray(sizes, dtype=np.uintp)
    else:
        parts = [bytes(x) for x in samples]
        buf = np.frombuffer(b"".join(parts) or b"\0", dtype=np.uint8)
        sizes = np.array([len(x) for x in parts], dtype=np.uintp)
    return buf, sizes


def _params(k, d, f, steps, split_point, level, dict_id, accel):
    return _lib.FastCoverParams(k=k, d=d, f=f, steps=steps, accel=accel, splitPoint=split_point, level=level, dictID=dict_id)


def train_dictionary(samples, capacity=65536, k=0, d=0, level=3, dict_id=0, f=0, steps=0, split_point=0.0, accel=0, return_params=False):
    """A zstd dictionary trained on the GPU (zsmi_trainFromBuffer_fastCover).  samples: a list of bytes-likes or (buffer, sizes).  k = 0 or
    d = 0 searches (steps k values in [50, 2000], d in {6, 8} when d = 0), scoring on the samples behind the split_point share.  Returns the
    dictionary, or (dictionary, k, d) with return_params."""
    L = _lib.lib()
    buf, sizes = _samples(samples)
    p = _params(k, d, f, steps, split_point, level, dict_id, accel)
    out = ctypes.create_string_buffer(max(int(capacity), 1))
    r = _raise_if_error(L, L.zsmi_trainFromBuffer_fastCover(out, capacity, buf.ctypes.data_as(ctypes.c_void_p),
                                                            sizes.ctypes.data_as(ctypes.POINTER(ctypes.c_size_t)), len(sizes), ctypes.byref(p)))
    return (out.raw[:r], p.k, p.d) if return_params else out.raw[:r]


def finalize_dictionary(content, samples, capacity, level=3, dict_id=0) -> bytes:
    """ZDICT_finalizeDictionary on the GPU: entropy tables from the samples compressed with `content`, the header, recent offsets {1, 4, 8}"""
    L = _lib.lib()
    buf, sizes = _samples(samples)
    content = bytes(content)
    out = ctypes.create_string_buffer(max(int(capacity), 1))
    r = _raise_if_error(L, L.zsmi_finalizeDictionary(out, capacity, content, len(content), buf.ctypes.data_as(ctypes.c_void_p),
                                                     sizes.ctypes.data_as(ctypes.POINTER(ctypes.c_size_t)), len(sizes), level, dict_id))
    return out.raw[:r]


def get_dict_id(dic) -> int:
    """the ID of a formatted dictionary; 0 for raw content (host only)"""
    dic = bytes(dic)
    return int(_lib.lib().zsmi_getDictID(dic, len(dic)))


class SeekableHandle:
    """An opened seekable archive in device memory (zsmi_openSeekableDevice; BatchCodec.open_seekable_device makes it), or a stream of
    frames without a table opened through its frame index (zsmi_openFramesDevice; BatchCodec.open_frames_device: frames=True).  Read-only:
    any BatchCodec of the same device may read through it.  It must stay open until the work queued with it is done (BatchCodec.sync)."""

    def __init__(self, codec, d_ptr, size, ddict=None, ddict_set=None, frames=False):
        if ddict is not None and ddict_set is not None:
            raise ValueError("ddict_set= excludes ddict=")
        self.L, self.codec = codec.L, codec
        self.ddict, self.ddict_set = ddict, ddict_set                       # (kept alive with the handle)
        self._own_set = DecompressionDictSet(codec, [], unnamed=ddict) if ddict is not None else None
        dset = self._own_set if ddict is not None else ddict_set
        err = ctypes.c_int(0)
        name = "zsmi_openFramesDevice" if frames else "zsmi_openSeekableDevice"
        self.handle = getattr(self.L, name + "_usingDDictSet")(codec.ctx, ctypes.c_void_p(d_ptr), size, dset.handle if dset is not None else None,
                                                               ctypes.byref(err))
        if not self.handle:
            raise RuntimeError(f"{name}: {_error_name(self.L, err.value)}")

    @property
    def num_frames(self) -> int:
        return int(self.L.zsmi_getNumFrames_fromSeekable(self.handle))

    @property
    def content_size(self) -> int:
        return int(self.L.zsmi_getContentSize_fromSeekable(self.handle))

    @property
    def device_bytes(self) -> int:
        return int(self.L.zsmi_sizeofSeekable(self.handle))

    def read_ranges_device(self, offsets, lengths, d_dst_ptr, dst_offsets, d_status_ptr, codec=None):
        """content [offsets[r], offsets[r] + lengths[r]) to d_dst + dst_offsets[r], for every r in one call (asynchronous, on `codec`'s
        stream: the one the handle was opened with unless given); d_status_ptr: device uint32[n], 0 or range r's error code.  Returns
        (written: the lengths clipped at the content's end, frames_decoded: distinct frames the call decodes)."""
        codec = codec or self.codec
        off = np.ascontiguousarray(offsets, dtype=np.uint64); ln = np.ascontiguousarray(lengths, dtype=np.uint64)
        do = np.ascontiguousarray(dst_offsets, dtype=np.uint64)
        written = np.zeros(len(off), dtype=np.uint64)
        frames = ctypes.c_uint32(0)
        p = BatchCodec._p
        rc = self.L.zsmi_seekableReadRangesDevice(codec.ctx, self.handle, p(off), p(ln), len(off), ctypes.c_void_p(d_dst_ptr), p(do), p(written),
                                                  ctypes.c_void_p(d_status_ptr), ctypes.byref(frames))
        if rc:
            raise RuntimeError(f"zsmi_seekableReadRangesDevice: {_error_name(self.L, rc)}")
        return written, frames.value

    def read_frames_device(self, indices, d_dst_ptr, dst_offsets, d_status_ptr, codec=None):
        """records by number: the content of frame indices[k] to d_dst + dst_offsets[k], for every k in one call (asynchronous, as
        read_ranges_device: zsmi_seekableReadFramesDevice); d_status_ptr: device uint32[n].  Returns (written: the frames' content
        sizes, frames_decoded)."""
        codec = codec or self.codec
        idx = np.ascontiguousarray(indices, dtype=np.uint32); do = np.ascontiguousarray(dst_offsets, dtype=np.uint64)
        written = np.zeros(len(idx), dtype=np.uint64)
        frames = ctypes.c_uint32(0)
        p = BatchCodec._p
        rc = self.L.zsmi_seekableReadFramesDevice(codec.ctx, self.handle, p(idx), len(idx), ctypes.c_void_p(d_dst_ptr), p(do), p(written),
                                                  ctypes.c_void_p(d_status_ptr), ctypes.byref(frames))
        if rc:
            raise RuntimeError(f"zsmi_seekableReadFramesDevice: {_error_name(self.L, rc)}")
        return written, frames.value

    def read_frames_resident(self, d_frame_index_ptr, n, d_dst_ptr, dst_capacity, d_dst_offsets_ptr, d_written_ptr, d_status_ptr, align=1, codec=None):
        """records by numbers that are DEVICE memory (uint32, n entries): nothing goes to the host.  The call lays the outputs out itself:
        d_dst_offsets (device uint64[n + 1]) receives the running sum of the frames' content sizes, each rounded up to `align`; request
        k's content lands at d_dst + d_dst_offsets[k], d_written (device uint32[n]) receives its size, d_status (device uint32[n]) 0 or
        its code - frameIndex_tooLarge (100) for a number that names no frame, dstSize_tooSmall (70) for a place that ends behind
        dst_capacity; neither touches its neighbours.  A number named twice is decoded twice.  zsmi_seekableReadFramesResident"""
        codec = codec or self.codec
        rc = self.L.zsmi_seekableReadFramesResident(codec.ctx, self.handle, ctypes.c_void_p(d_frame_index_ptr), n, align, ctypes.c_void_p(d_dst_ptr),
                                                    dst_capacity, ctypes.c_void_p(d_dst_offsets_ptr), ctypes.c_void_p(d_written_ptr),
                                                    ctypes.c_void_p(d_status_ptr))
        if rc:
            raise RuntimeError(f"zsmi_seekableReadFramesResident: {_error_name(self.L, rc)}")

    def records_work_bound(self, max_frame_reads) -> int:
        """d_work bytes that always suffice for max_frame_reads frame reads of this handle (zsmi_seekableRecordsWorkBound)"""
        return int(self.L.zsmi_seekableRecordsWorkBound(self.handle, max_frame_reads))

    def read_records_resident(self, d_first_record_ptr, n_frames, d_record_index_ptr, n_records, max_frame_reads, d_work_ptr, work_capacity, d_dst_ptr,
                              dst_capacity, d_dst_offsets_ptr, d_written_ptr, d_status_ptr, d_result_ptr, delimiter=b"\n", align=1, codec=None):
        """records by numbers that are DEVICE memory (uint64, n_records entries) from a record archive and the first_record array
        split_records_device left in device memory (uint64[n_frames + 1]): nothing goes to the host.  Request k's record, its delimiter
        included, lands at d_dst + d_dst_offsets[k] (device uint64[n_records + 1]: the running sum of the lengths, each rounded up to
        `align`), d_written (device uint64[n_records]) receives its length, d_status (device uint32[n_records]) 0 or its code, d_result
        (device uint64[4]) the requests with status 0, the frame reads and work bytes the call needs whatever its caps are, and
        d_dst_offsets[n_records].  The frames are decoded into d_work (records_work_bound(max_frame_reads) always suffices); requests
        in a row that name the same frames decode them once.  zsmi_seekableReadRecordsResident"""
        codec = codec or self.codec
        p = ctypes.c_void_p
        rc = self.L.zsmi_seekableReadRecordsResident(codec.ctx, self.handle, p(d_first_record_ptr), n_frames, _delimiter(delimiter), p(d_record_index_ptr), n_records,
                                                     max_frame_reads, align, p(d_work_ptr), work_capacity, p(d_dst_ptr), dst_capacity, p(d_dst_offsets_ptr),
                                                     p(d_written_ptr), p(d_status_ptr), p(d_result_ptr))
        if rc:
            raise RuntimeError(f"zsmi_seekableReadRecordsResident: {_error_name(self.L, rc)}")

    def find_work_bound(self, first_frame, frame_count) -> int:
        """the d_work bytes find_records_resident needs for this window: its frames' content (zsmi_seekableFindWorkBound; 0 for a window
        outside the archive)"""
        return int(self.L.zsmi_seekableFindWorkBound(self.handle, first_frame, frame_count))

    def find_records_resident(self, d_first_record_ptr, n_frames, pattern, first_frame, frame_count, d_work_ptr, work_capacity, d_records_ptr, capacity,
                              d_result_ptr, delimiter=b"\n", codec=None):
        """the records of frames [first_frame, first_frame + frame_count) of a record archive that hold `pattern` (HOST bytes, 1 .. 256 of
        them, none the delimiter), everything else in device memory and nothing going to the host: d_records (uint64[capacity]; 0 with
        capacity 0: only count) receives their numbers, ascending - what read_records_resident takes as d_record_index - and d_result
        (uint64[4]) the total or (uint64)-code, the numbers written, the occurrences and the bytes searched.  The window's frames are
        decoded into d_work (find_work_bound bytes) and the numbers count from d_first_record[first_frame] (uint64[n_frames + 1], as
        split_records_device left it).  zsmi_seekableFindRecordsResident"""
        codec = codec or self.codec
        p = ctypes.c_void_p
        pat = bytes(pattern)
        rc = self.L.zsmi_seekableFindRecordsResident(codec.ctx, self.handle, p(d_first_record_ptr), n_frames, _delimiter(delimiter), pat, len(pat), first_frame,
                                                     frame_count, p(d_work_ptr), work_capacity, p(d_records_ptr), capacity, p(d_result_ptr))
        if rc:
            raise RuntimeError(f"zsmi_seekableFindRecordsResident: {_error_name(self.L, rc)}")

    def find_query_resident(self, d_first_record_ptr, n_frames, patterns, first_frame, frame_count, d_work_ptr, work_capacity, d_records_ptr, d_hits_ptr,
                            capacity, d_result_ptr, mode="any", ignore_case=False, delimiter=b"\n", codec=None):
        """find_records_resident for a query of 1 .. 8 patterns (HOST bytes; mode 'any', 'all' or 'none', ignore_case folds 'A' .. 'Z'):
        one decode of the window into d_work, then d_records (uint64[capacity]) receives the numbers of the records whose hit set
        satisfies the mode, d_hits (uint8[capacity]; 0: not wanted) their hit sets, d_result (uint64[4]) the words of
        find_records_resident.  Nothing goes to the host.  zsmi_seekableFindQueryResident"""
        codec = codec or self.codec
        p = ctypes.c_void_p
        q, keep = _find_query(patterns, mode, ignore_case)
        rc = self.L.zsmi_seekableFindQueryResident(codec.ctx, self.handle, p(d_first_record_ptr), n_frames, _delimiter(delimiter), ctypes.byref(q), first_frame,
                                                   frame_count, p(d_work_ptr), work_capacity, p(d_records_ptr), p(d_hits_ptr), capacity, p(d_result_ptr))
        if rc:
            raise RuntimeError(f"zsmi_seekableFindQueryResident: {_error_name(self.L, rc)}")

    def find_regex_resident(self, d_first_record_ptr, n_frames, regex, first_frame, frame_count, d_work_ptr, work_capacity, d_records_ptr, capacity,
                            d_result_ptr, delimiter=b"\n", codec=None):
        """find_records_resident for a regular expression (a compile_regex program, or bytes compiled on the spot; HOST memory): one
        decode of the window into d_work, then d_records (uint64[capacity]) receives the numbers of the records the program lists and
        d_result (uint64[4]) the total or (uint64)-code, the numbers written, the RECORDS of the window and the bytes searched.  Nothing
        goes to the host.  zsmi_seekableFindRegexResident"""
        codec = codec or self.codec
        p = ctypes.c_void_p
        prog = _regex(regex)
        rc = self.L.zsmi_seekableFindRegexResident(codec.ctx, self.handle, p(d_first_record_ptr), n_frames, _delimiter(delimiter), ctypes.byref(prog), first_frame,
                                                   frame_count, p(d_work_ptr), work_capacity, p(d_records_ptr), capacity, p(d_result_ptr))
        if rc:
            raise RuntimeError(f"zsmi_seekableFindRegexResident: {_error_name(self.L, rc)}")

    def load_record_index_resident(self, d_first_record_ptr, d_result_ptr, codec=None):
        """the record index the archive carries (its last entry, an index frame) into d_first_record (uint64[num_frames + 1]): the array
        the record calls above take with n_frames = num_frames.  d_result (uint64[4]) = {status, records, delimiter, n}; a status other
        than 0 - prefix_unknown for an archive without an index - leaves the array untouched.  Nothing goes to the host.
        zsmi_seekableLoadRecordIndexResident"""
        codec = codec or self.codec
        p = ctypes.c_void_p
        rc = self.L.zsmi_seekableLoadRecordIndexResident(codec.ctx, self.handle, p(d_first_record_ptr), p(d_result_ptr))
        if rc:
            raise RuntimeError(f"zsmi_seekableLoadRecordIndexResident: {_error_name(self.L, rc)}")

    def index_records_resident(self, first_frame, frame_count, d_work_ptr, work_capacity, d_first_record_ptr, d_result_ptr, delimiter=b"\n", codec=None):
        """the record index rebuilt from the content of frames [first_frame, first_frame + frame_count): they are decoded into d_work
        (find_work_bound bytes) and d_first_record (uint64[num_frames + 1]) receives the entries behind first_frame (entry 0 too for the
        window at 0), counted from d_first_record[first_frame] - windows taken in ascending order chain.  d_result (uint64[4]) = {the
        first failing frame's code, records, misaligned frames, delimiters}.  Nothing goes to the host.
        zsmi_seekableIndexRecordsResident"""
        codec = codec or self.codec
        p = ctypes.c_void_p
        rc = self.L.zsmi_seekableIndexRecordsResident(codec.ctx, self.handle, _delimiter(delimiter), first_frame, frame_count, p(d_work_ptr), work_capacity,
                                                      p(d_first_record_ptr), p(d_result_ptr))
        if rc:
            raise RuntimeError(f"zsmi_seekableIndexRecordsResident: {_error_name(self.L, rc)}")

    def find_frames_work_bound(self, max_frames) -> int:
        """the d_work bytes that hold any list of max_frames frames for find_query_frames_resident: max_frames x (the largest frame's
        content + 1) (zsmi_seekableFindFramesWorkBound)"""
        return int(self.L.zsmi_seekableFindFramesWorkBound(self.handle, max_frames))

    def find_query_frames_resident(self, d_first_record_ptr, n_frames, patterns, d_frames_ptr, d_frame_count_ptr, max_frames, d_work_ptr, work_capacity,
                                   d_records_ptr, d_hits_ptr, capacity, d_result_ptr, mode="any", ignore_case=False, delimiter=b"\n", codec=None):
        """find_query_resident over a LIST of frames in device memory: d_frames (uint32[max_frames], ascending) and d_frame_count (one
        uint64: d_result of filter_frames_device can be passed as it is) - only those frames are decoded into d_work
        (find_frames_work_bound(max_frames) bytes always suffice) and searched; d_records, d_hits as find_query_resident, d_result
        (uint64[4]) = {total or (uint64)-code, written, occurrences, content bytes decoded}; a refusal leaves the bytes needed in
        d_result[3].  Mode 'none' is refused.  Nothing goes to the host.  zsmi_seekableFindQueryFramesResident"""
        codec = codec or self.codec
        p = ctypes.c_void_p
        q, keep = _find_query(patterns, mode, ignore_case)
        rc = self.L.zsmi_seekableFindQueryFramesResident(codec.ctx, self.handle, p(d_first_record_ptr), n_frames, _delimiter(delimiter), ctypes.byref(q), p(d_frames_ptr),
                                                         p(d_frame_count_ptr), max_frames, p(d_work_ptr), work_capacity, p(d_records_ptr), p(d_hits_ptr), capacity, p(d_result_ptr))
        if rc:
            raise RuntimeError(f"zsmi_seekableFindQueryFramesResident: {_error_name(self.L, rc)}")

    def build_frame_filter_resident(self, d_work_ptr, work_capacity, d_filter_ptr, capacity, d_result_ptr, delimiter=b"\n", gram=4, log2_bits=13, codec=None):
        """the archive's filter frame (build_frame_filter states it) into d_filter (8-byte aligned, frame_filter_size(num_frames,
        log2_bits) bytes): the frames are decoded end to end into d_work (find_work_bound(0, num_frames) bytes) and hashed there.
        d_result (uint64[4]) = {the first failing frame's code, bytes written, saturated frames, grams hashed}.  Nothing goes to the
        host.  zsmi_seekableBuildFrameFilterResident"""
        codec = codec or self.codec
        p = ctypes.c_void_p
        rc = self.L.zsmi_seekableBuildFrameFilterResident(codec.ctx, self.handle, _delimiter(delimiter), gram, log2_bits, p(d_work_ptr), work_capacity,
                                                          p(d_filter_ptr), capacity, p(d_result_ptr))
        if rc:
            raise RuntimeError(f"zsmi_seekableBuildFrameFilterResident: {_error_name(self.L, rc)}")

    def frame_info(self, index):
        """(compressed offset, content offset, compressed size, content size) of frame `index`, from the handle's table"""
        co, do, cs, ds = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint32(), ctypes.c_uint32()
        if index < 0:
            index += self.num_frames
        index = index if 0 <= index <= 0xFFFFFFFF else 0xFFFFFFFF          # (out of range either way: frameIndex_tooLarge)
        rc = self.L.zsmi_getFrameInfo_fromSeekable(self.handle, index, ctypes.byref(co), ctypes.byref(do), ctypes.byref(cs), ctypes.byref(ds))
        if rc:
            raise RuntimeError(_error_name(self.L, rc))
        return co.value, do.value, cs.value, ds.value

    def close(self):
        if self.handle:
            self.L.zsmi_closeSeekable(self.handle)
            self.handle = None
        if getattr(self, "_own_set", None) is not None:
            self._own_set.close()
            self._own_set = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class BatchCodec:
    """n independent chunks <-> n frames on one GPU.  Arrays of offsets/sizes live on the host (numpy);
    data lives on the device.  `stream` is a raw hipStream_t handle (e.g. torch.cuda.current_stream().cuda_stream)."""

    def __init__(self, device=-1, stream=None):
        self.L = _lib.lib()
        self.ctx = self.L.zsmi_createCtx(device, ctypes.c_void_p(stream) if stream else None)
        if not self.ctx:
            raise RuntimeError("zsmi_createCtx failed: no usable HIP device (this codec has no CPU path)")

    def close(self):
        if self.ctx:
            self.L.zsmi_freeCtx(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sync(self):
        rc = self.L.zsmi_sync(self.ctx)
        if rc:
            raise RuntimeError(f"device error {rc}")

    PARAMETERS = {"checksum": 201}      # ZSMI_c_checksumFlag

    def _parameter(self, name_or_id):
        if isinstance(name_or_id, str):
            if name_or_id not in self.PARAMETERS:
                raise ValueError(f"no such parameter: {name_or_id!r} (known: {sorted(self.PARAMETERS)})")
            return self.PARAMETERS[name_or_id]
        return int(name_or_id)

    def set_parameter(self, name_or_id, value):
        """a sticky compression parameter of this codec (zsmi_setParameter), by name or by its number.  "checksum" (0 / 1): every frame
        of the compress calls made after it carries a Content_Checksum - the same frames otherwise, 4 bytes longer - and a decoder
        answers checksum_wrong (22) for a frame whose content it cannot restore.  RuntimeError with the error's name for a number or a
        value the library refuses."""
        rc = self.L.zsmi_setParameter(self.ctx, self._parameter(name_or_id), int(value))
        if rc:
            raise RuntimeError(f"zsmi_setParameter: {_error_name(self.L, rc)}")

    def get_parameter(self, name_or_id) -> int:
        v = ctypes.c_int(0)
        rc = self.L.zsmi_getParameter(self.ctx, self._parameter(name_or_id), ctypes.byref(v))
        if rc:
            raise RuntimeError(f"zsmi_getParameter: {_error_name(self.L, rc)}")
        return v.value

    @staticmethod
    def _p(a):
        return a.ctypes.data_as(ctypes.c_void_p)

    @staticmethod
    def _compress_form(name, level, dict_ptr, dict_size, cdict, cdict_set=None, dict_index=None):
        """the C function of a batch compress call and its arguments behind the common ones: a CompressionDictSet comes first, then a
        CompressionDict, then a dictionary"""
        if cdict_set is not None:
            if cdict is not None or dict_size:
                raise ValueError("cdict_set= excludes cdict= and a dictionary")
            if dict_index is None:
                raise ValueError("cdict_set= needs dict_index=")
            return name + "_usingCDictSet", (cdict_set.handle, BatchCodec._p(dict_index))
        if dict_index is not None:
            raise ValueError("dict_index= needs cdict_set=")
        if cdict is not None:
            return name + "_usingCDict", (cdict.handle,)
        if dict_size:
            return name + "_usingDict", (level, dict_ptr, dict_size)
        return name, (level,)

    @staticmethod
    def _dict_index(dict_index, n):
        if dict_index is None:
            return None
        di = np.ascontiguousarray(dict_index, dtype=np.uint32)
        if di.shape != (n,):
            raise ValueError("dict_index= holds one entry a chunk")
        return di

    def compress_device(self, d_src_ptr, src_offsets, src_sizes, d_dst_ptr, dst_offsets, d_dst_sizes_ptr, level=3, d_dict_ptr=0, dict_size=0, cdict=None,
                        cdict_set=None, dict_index=None):
        """d_dict_ptr / dict_size: one dictionary (device memory) for every chunk of the call (zsmi_compressBatchDevice_usingDict).
        cdict: a CompressionDict instead (zsmi_compressBatchDevice_usingCDict: its level holds; queued without a wait).
        cdict_set, dict_index: a CompressionDictSet instead, chunk i with its member dict_index[i] or, for NO_DICT, with none
        (zsmi_compressBatchDevice_usingCDictSet: the set's level holds; queued without a wait)"""
        so = np.ascontiguousarray(src_offsets, dtype=np.uint64); ss = np.ascontiguousarray(src_sizes, dtype=np.uint32)
        do = np.ascontiguousarray(dst_offsets, dtype=np.uint64)
        di = self._dict_index(dict_index, len(ss))
        name, tail = self._compress_form("zsmi_compressBatchDevice", level, ctypes.c_void_p(d_dict_ptr), d_dict_ptr and dict_size, cdict, cdict_set, di)
        _check(getattr(self.L, name)(self.ctx, ctypes.c_void_p(d_src_ptr), self._p(so), self._p(ss), len(ss), ctypes.c_void_p(d_dst_ptr), self._p(do),
                                     ctypes.c_void_p(d_dst_sizes_ptr), *tail), name)

    def decompress_device(self, d_src_ptr, src_offsets, src_sizes, d_dst_ptr, dst_offsets, dst_caps, d_dst_sizes_ptr, ddict=None, ddict_set=None):
        """ddict: a DecompressionDict for every frame of the call (zsmi_decompressBatchDevice_usingDDict: queued without a wait).
        ddict_set: a DecompressionDictSet instead - each frame's dictID picks its dictionary (zsmi_decompressBatchDevice_usingDDictSet)"""
        if ddict_set is not None and ddict is not None:
            raise ValueError("ddict_set= and ddict= exclude each other")
        so = np.ascontiguousarray(src_offsets, dtype=np.uint64); ss = np.ascontiguousarray(src_sizes, dtype=np.uint32)
        do = np.ascontiguousarray(dst_offsets, dtype=np.uint64); dc = np.ascontiguousarray(dst_caps, dtype=np.uint32)
        args = (self.ctx, ctypes.c_void_p(d_src_ptr), self._p(so), self._p(ss), len(ss), ctypes.c_void_p(d_dst_ptr), self._p(do), self._p(dc), ctypes.c_void_p(d_dst_sizes_ptr))
        if ddict_set is not None:
            _check(self.L.zsmi_decompressBatchDevice_usingDDictSet(*args, ddict_set.handle), "zsmi_decompressBatchDevice_usingDDictSet")
        elif ddict is not None:
            _check(self.L.zsmi_decompressBatchDevice_usingDDict(*args, ddict.handle), "zsmi_decompressBatchDevice_usingDDict")
        else:
            _check(self.L.zsmi_decompressBatchDevice(*args), "zsmi_decompressBatchDevice")

    def pack_device(self, d_frames_ptr, dst_offsets, d_sizes_ptr, n, d_packed_ptr, d_packed_offsets_ptr):
        """frames sitting at dst_offsets (sizes on the device) -> one contiguous run at d_packed; d_packed_offsets[n + 1] (device, uint64)"""
        do = np.ascontiguousarray(dst_offsets, dtype=np.uint64)
        _check(self.L.zsmi_packFramesDevice(self.ctx, ctypes.c_void_p(d_frames_ptr), self._p(do), ctypes.c_void_p(d_sizes_ptr), n,
                                            ctypes.c_void_p(d_packed_ptr), ctypes.c_void_p(d_packed_offsets_ptr)), "zsmi_packFramesDevice")

    # ---- device-resident decode: every array is device memory (pointers), the calls only queue work.  Chained - pack_device's offsets and
    # compress_device's sizes -> frame_sizes_device -> layout_outputs_device -> decompress_resident - nothing comes to the host in between
    def frame_sizes_device(self, d_src_ptr, d_src_offsets_ptr, d_src_sizes_ptr, n, d_content_sizes_ptr, d_bounds_ptr, d_status_ptr):
        """per item: find_decompressed_size -> d_content_sizes (uint64), decompress_bound -> d_bounds (uint64; either may be 0: not
        wanted), 0 or the refusal's code -> d_status (uint32).  zsmi_getFrameSizesBatchDevice"""
        rc = self.L.zsmi_getFrameSizesBatchDevice(self.ctx, ctypes.c_void_p(d_src_ptr), ctypes.c_void_p(d_src_offsets_ptr), ctypes.c_void_p(d_src_sizes_ptr), n,
                                                  ctypes.c_void_p(d_content_sizes_ptr), ctypes.c_void_p(d_bounds_ptr), ctypes.c_void_p(d_status_ptr))
        if rc:
            raise RuntimeError(f"zsmi_getFrameSizesBatchDevice: {_error_name(self.L, rc)}")

    def layout_outputs_device(self, d_sizes_ptr, d_status_ptr, n, d_dst_caps_ptr, d_dst_offsets_ptr, align=1):
        """sizes (uint64) and statuses (uint32; 0: none) -> d_dst_caps (uint32: the size, or 0 for an item with a status or a size that is
        unknown or no batch item's) and d_dst_offsets (uint64, n + 1: the running sum of the caps rounded up to align; the last is the
        room they take).  zsmi_layoutOutputsDevice"""
        rc = self.L.zsmi_layoutOutputsDevice(self.ctx, ctypes.c_void_p(d_sizes_ptr), ctypes.c_void_p(d_status_ptr), n, align,
                                             ctypes.c_void_p(d_dst_caps_ptr), ctypes.c_void_p(d_dst_offsets_ptr))
        if rc:
            raise RuntimeError(f"zsmi_layoutOutputsDevice: {_error_name(self.L, rc)}")

    def decompress_resident(self, d_src_ptr, d_src_offsets_ptr, d_src_sizes_ptr, n, d_dst_ptr, d_dst_offsets_ptr, d_dst_caps_ptr, max_dst_cap,
                            d_dst_sizes_ptr, ddict_set=None):
        """decompress_device with its four descriptor arrays in device memory; max_dst_cap: no item gets more room, and the scratch is
        planned for n items of it.  ddict_set: a DecompressionDictSet (one dictionary: DecompressionDictSet(codec, [], unnamed=ddict)).
        zsmi_decompressBatchResident"""
        rc = self.L.zsmi_decompressBatchResident(self.ctx, ctypes.c_void_p(d_src_ptr), ctypes.c_void_p(d_src_offsets_ptr), ctypes.c_void_p(d_src_sizes_ptr), n,
                                                 ctypes.c_void_p(d_dst_ptr), ctypes.c_void_p(d_dst_offsets_ptr), ctypes.c_void_p(d_dst_caps_ptr), max_dst_cap,
                                                 ctypes.c_void_p(d_dst_sizes_ptr), ddict_set.handle if ddict_set is not None else None)
        if rc:
            raise RuntimeError(f"zsmi_decompressBatchResident: {_error_name(self.L, rc)}")

    # ---- device-resident compress: the head of the chain.  compress_bounds_device -> layout_outputs_device (over the bounds) ->
    # compress_resident; its d_dst_offsets / d_dst_sizes are what frame_sizes_device and decompress_resident take
    def compress_bounds_device(self, d_src_sizes_ptr, n, d_bounds_ptr):
        """compress_bound of n sizes (uint32, device) -> d_bounds (uint64, device).  zsmi_compressBoundsDevice"""
        rc = self.L.zsmi_compressBoundsDevice(self.ctx, ctypes.c_void_p(d_src_sizes_ptr), n, ctypes.c_void_p(d_bounds_ptr))
        if rc:
            raise RuntimeError(f"zsmi_compressBoundsDevice: {_error_name(self.L, rc)}")

    def compress_resident(self, d_src_ptr, d_src_offsets_ptr, d_src_sizes_ptr, n, max_src_size, d_dst_ptr, d_dst_offsets_ptr, d_dst_sizes_ptr, level=3,
                          cdict_set=None, d_dict_index_ptr=0):
        """compress_device with its three descriptor arrays in device memory; max_src_size: the call is planned for n chunks of it, and a
        chunk above it gets the size word of srcSize_wrong (72) instead of a frame.  The frames are compress_device's, byte for byte; the
        codec's "checksum" parameter holds.  zsmi_compressBatchResident.
        cdict_set, d_dict_index_ptr: a CompressionDictSet, chunk i with its member d_dict_index[i] (uint32, DEVICE memory, n entries) or,
        for NO_DICT, with none; any other index gives the chunk the size word of parameter_outOfBound (42).  The set's level holds (a
        `level` that disagrees raises).  d_dict_index_ptr = 0 with a set of one member: every chunk uses it - one CompressionDict cd is
        CompressionDictSet(codec, [cd], level).  zsmi_compressBatchResident_usingCDictSet"""
        common = (self.ctx, ctypes.c_void_p(d_src_ptr), ctypes.c_void_p(d_src_offsets_ptr), ctypes.c_void_p(d_src_sizes_ptr), n,
                  max_src_size, ctypes.c_void_p(d_dst_ptr), ctypes.c_void_p(d_dst_offsets_ptr), ctypes.c_void_p(d_dst_sizes_ptr))
        if cdict_set is None:
            if d_dict_index_ptr:
                raise ValueError("d_dict_index_ptr= needs cdict_set=")
            name, rc = "zsmi_compressBatchResident", self.L.zsmi_compressBatchResident(*common, level)
        else:
            if level != 3 and level != cdict_set.level:
                raise ValueError("cdict_set= compresses at the set's level")
            name = "zsmi_compressBatchResident_usingCDictSet"
            rc = self.L.zsmi_compressBatchResident_usingCDictSet(*common, cdict_set.handle, ctypes.c_void_p(d_dict_index_ptr))
        if rc:
            raise RuntimeError(f"{name}: {_error_name(self.L, rc)}")

    def seekable_bound(self, src_size, frame_size=0, checksum=True) -> int:
        return _raise_if_error(self.L, self.L.zsmi_seekableBound(src_size, frame_size, int(bool(checksum))))

    def compress_seekable_device(self, d_src_ptr, src_size, d_dst_ptr, dst_capacity, d_archive_size_ptr, level=3, frame_size=0, checksum=True):
        """a seekable archive of d_src[0, src_size) at d_dst (asynchronous); *d_archive_size_ptr (device uint64) receives its size, or
        (uint64)-code if a frame failed.  dst_capacity must be at least seekable_bound(src_size, frame_size, checksum).  checksum is the
        table's; the frames carry their own Content_Checksum when the codec's "checksum" parameter is set."""
        rc = self.L.zsmi_compressSeekableDevice(self.ctx, ctypes.c_void_p(d_src_ptr), src_size, ctypes.c_void_p(d_dst_ptr), dst_capacity,
                                                ctypes.c_void_p(d_archive_size_ptr), level, frame_size, int(bool(checksum)))
        if rc:
            raise RuntimeError(f"zsmi_compressSeekableDevice: {_error_name(self.L, rc)}")

    def decompress_seekable_device(self, d_src_ptr, src_size, offset, length, d_dst_ptr, d_status_ptr) -> int:
        """content bytes [offset, offset + length) of the archive at d_src into d_dst; returns how many (the range clipped at the content's
        end).  The table is read and checked at once (RuntimeError); the frames decode asynchronously, *d_status_ptr (device uint32)
        receives 0 or the first failing frame's code."""
        written = ctypes.c_uint64(0)
        rc = self.L.zsmi_decompressSeekableDevice(self.ctx, ctypes.c_void_p(d_src_ptr), src_size, offset, length, ctypes.c_void_p(d_dst_ptr),
                                                  ctypes.byref(written), ctypes.c_void_p(d_status_ptr))
        if rc:
            raise RuntimeError(f"zsmi_decompressSeekableDevice: {_error_name(self.L, rc)}")
        return written.value

    def _frames_form(self, name, level, cdict, cdict_set, dict_index, n):
        """the C function of a record-archive compress call and its arguments behind checksumFlag: a CompressionDictSet with the frames'
        choice, or a CompressionDict as the set of one (a null choice: every frame uses it); else the plain form at `level`"""
        if cdict is not None and cdict_set is not None:
            raise ValueError("cdict_set= excludes cdict=")
        if cdict is not None:
            if dict_index is not None:
                raise ValueError("dict_index= needs cdict_set=")
            return name + "_usingCDictSet", (), (cdict.as_set(self).handle, None)
        if cdict_set is not None:
            di = self._dict_index(dict_index, n)
            return name + "_usingCDictSet", (), (cdict_set.handle, self._p(di) if di is not None else None)
        if dict_index is not None:
            raise ValueError("dict_index= needs cdict_set=")
        return name, (level,), ()

    def seekable_frames_bound(self, frame_sizes, checksum=True) -> int:
        """room a record archive of these frame sizes needs (zsmi_seekableFramesBound)"""
        fs = np.ascontiguousarray(frame_sizes, dtype=np.uint32)
        return _raise_if_error(self.L, self.L.zsmi_seekableFramesBound(self._p(fs) if len(fs) else None, len(fs), int(bool(checksum))))

    def compress_seekable_frames_device(self, d_src_ptr, frame_sizes, d_dst_ptr, dst_capacity, d_archive_size_ptr, level=3, checksum=True, cdict=None,
                                        cdict_set=None, dict_index=None):
        """a record archive at d_dst (asynchronous): frame i holds the next frame_sizes[i] bytes of d_src, compressed with member
        dict_index[i] of cdict_set (NO_DICT: none), with cdict, or plainly at `level`; *d_archive_size_ptr (device uint64) receives
        its size, or (uint64)-code of the lowest failing frame.  dst_capacity must be at least seekable_frames_bound(frame_sizes, checksum).
        checksum is the table's flag; the frames carry a Content_Checksum when the codec's "checksum" parameter is set."""
        fs = np.ascontiguousarray(frame_sizes, dtype=np.uint32)
        name, head, tail = self._frames_form("zsmi_compressSeekableFramesDevice", level, cdict, cdict_set, dict_index, len(fs))
        rc = getattr(self.L, name)(self.ctx, ctypes.c_void_p(d_src_ptr), self._p(fs) if len(fs) else None, len(fs), ctypes.c_void_p(d_dst_ptr), dst_capacity,
                                   ctypes.c_void_p(d_archive_size_ptr), *head, int(bool(checksum)), *tail)
        if rc:
            raise RuntimeError(f"{name}: {_error_name(self.L, rc)}")

    def compress_seekable_frames_host(self, src, frame_sizes, level=3, checksum=True, cdict=None, cdict_set=None, dict_index=None) -> bytes:
        """the record archive of `src` (host bytes) cut at frame_sizes, as compress_seekable_frames_device makes it: staged, run, copied back"""
        s, sn = _buf(src)
        fs = np.ascontiguousarray(frame_sizes, dtype=np.uint32)
        if int(fs.sum(dtype=np.uint64)) != sn:
            raise ValueError("frame_sizes must add up to len(src)")
        cap = self.seekable_frames_bound(fs, checksum)
        out = np.empty(cap, dtype=np.uint8)
        name, head, tail = self._frames_form("zsmi_compressSeekableFramesHost", level, cdict, cdict_set, dict_index, len(fs))
        r = _raise_if_error(self.L, getattr(self.L, name)(self.ctx, self._p(out), cap, s, self._p(fs) if len(fs) else None, len(fs), *head,
                                                          int(bool(checksum)), *tail))
        return out[:r].tobytes()

    def seekable_frames_resident_bound(self, src_size, n, checksum=True) -> int:
        """room the record archive of ANY split of src_size content bytes into n frames needs (zsmi_seekableFramesResidentBound): what
        compress_seekable_frames_resident asks of dst_capacity, since the host never sees the sizes"""
        return _raise_if_error(self.L, self.L.zsmi_seekableFramesResidentBound(src_size, n, int(bool(checksum))))

    def compress_seekable_frames_resident(self, d_src_ptr, src_size, d_frame_sizes_ptr, n, max_frame_size, d_dst_ptr, dst_capacity, d_archive_size_ptr,
                                          level=3, checksum=True, cdict=None, cdict_set=None, d_dict_index_ptr=0):
        """compress_seekable_frames_device with its frame sizes (uint32, n entries) and dictionary indices in DEVICE memory: nothing goes
        to the host.  src_size: the content bytes at d_src, which the sizes must add up to; max_frame_size: no size is above it (the call
        is planned for it).  The archive is compress_seekable_frames_device's, byte for byte.  What the sizes or indices make impossible
        goes to *d_archive_size_ptr as (uint64)-code: srcSize_wrong (72) for a size above max_frame_size, a frame that ends behind
        src_size or sizes that sum to less; parameter_outOfBound (42) for an index that names no member.  dst_capacity must be at least
        seekable_frames_resident_bound(src_size, n, checksum).
        cdict_set, d_dict_index_ptr: frame i with member d_dict_index[i] (uint32, device, n entries; NO_DICT: none); d_dict_index_ptr = 0
        with a set of one member, or cdict=: every frame uses it.  zsmi_compressSeekableFramesResident[_usingCDictSet]"""
        if cdict is not None and cdict_set is not None:
            raise ValueError("cdict_set= excludes cdict=")
        if d_dict_index_ptr and cdict_set is None:
            raise ValueError("d_dict_index_ptr= needs cdict_set=")
        common = (self.ctx, ctypes.c_void_p(d_src_ptr), src_size, ctypes.c_void_p(d_frame_sizes_ptr), n, max_frame_size, ctypes.c_void_p(d_dst_ptr),
                  dst_capacity, ctypes.c_void_p(d_archive_size_ptr))
        if cdict is None and cdict_set is None:
            name, rc = "zsmi_compressSeekableFramesResident", self.L.zsmi_compressSeekableFramesResident(*common, level, int(bool(checksum)))
        else:
            dset = cdict.as_set(self) if cdict is not None else cdict_set
            name = "zsmi_compressSeekableFramesResident_usingCDictSet"
            rc = self.L.zsmi_compressSeekableFramesResident_usingCDictSet(*common, int(bool(checksum)), dset.handle, ctypes.c_void_p(d_dict_index_ptr))
        if rc:
            raise RuntimeError(f"{name}: {_error_name(self.L, rc)}")

    @staticmethod
    def split_pieces_bound(records, src_size, max_frame_size) -> int:
        """a max_pieces that always suffices for split_records_device: the records (count_records_device) + a cut every max_frame_size bytes"""
        return records + src_size // max_frame_size

    def count_records_device(self, d_src_ptr, src_size, d_records_ptr, delimiter=b"\n"):
        """*d_records_ptr (device uint64) = the records of d_src[0, src_size): its delimiters, + 1 for a tail without one (asynchronous:
        a count kernel and a sum are queued, nothing waited for).  zsmi_countRecordsDevice"""
        rc = self.L.zsmi_countRecordsDevice(self.ctx, ctypes.c_void_p(d_src_ptr), src_size, _delimiter(delimiter), ctypes.c_void_p(d_records_ptr))
        if rc:
            raise RuntimeError(f"zsmi_countRecordsDevice: {_error_name(self.L, rc)}")

    def split_records_device(self, d_src_ptr, src_size, max_pieces, d_frame_sizes_ptr, d_first_record_ptr, d_result_ptr, delimiter=b"\n", target_size=0,
                             max_frame_size=1 << 16):
        """split_records on the device, everything in device memory (asynchronous: only queued): d_frame_sizes (uint32[max_pieces]) and
        d_first_record (uint64[max_pieces + 1]; 0: not wanted) receive what split_records returns for the same bytes, d_result
        (uint64[3]) the frame count or (uint64)-code, the records and the pieces.  More pieces than max_pieces (split_pieces_bound always
        suffices): d_result[0] = -dstSize_tooSmall (70) and no list.  What it leaves is what compress_seekable_frames_resident takes:
        n = d_result[0] read back is that call's host argument.  zsmi_splitRecordsDevice"""
        rc = self.L.zsmi_splitRecordsDevice(self.ctx, ctypes.c_void_p(d_src_ptr), src_size, _delimiter(delimiter), target_size, max_frame_size, max_pieces,
                                            ctypes.c_void_p(d_frame_sizes_ptr), ctypes.c_void_p(d_first_record_ptr), ctypes.c_void_p(d_result_ptr))
        if rc:
            raise RuntimeError(f"zsmi_splitRecordsDevice: {_error_name(self.L, rc)}")

    def find_records_device(self, d_src_ptr, src_size, pattern, d_records_ptr, capacity, d_result_ptr, delimiter=b"\n", d_base_ptr=0):
        """find_records on the device, the text in device memory (asynchronous: only queued): d_records (uint64[capacity]; 0 with capacity
        0: only count) receives the ascending numbers of the records of d_src[0, src_size) that hold `pattern` (HOST bytes, 1 .. 256 of
        them, none the delimiter), d_result (uint64[4]) the total, the numbers written, the occurrences and the bytes searched; total and
        occurrences are exact whatever capacity is.  d_base_ptr: one device uint64 the numbers count from (0: from 0).
        zsmi_findRecordsDevice"""
        pat = bytes(pattern)
        rc = self.L.zsmi_findRecordsDevice(self.ctx, ctypes.c_void_p(d_src_ptr), src_size, _delimiter(delimiter), pat, len(pat), ctypes.c_void_p(d_base_ptr),
                                           ctypes.c_void_p(d_records_ptr), capacity, ctypes.c_void_p(d_result_ptr))
        if rc:
            raise RuntimeError(f"zsmi_findRecordsDevice: {_error_name(self.L, rc)}")

    def find_records_query_device(self, d_src_ptr, src_size, patterns, d_records_ptr, d_hits_ptr, capacity, d_result_ptr, mode="any", ignore_case=False,
                                  delimiter=b"\n", d_base_ptr=0):
        """find_records_query on the device, the text in device memory (asynchronous: only queued): d_records (uint64[capacity]; 0 with
        capacity 0: only count) receives the ascending numbers of the records of d_src[0, src_size) whose hit set satisfies the mode,
        d_hits (uint8[capacity]; 0: not wanted) the hit sets, d_result (uint64[4]) the total, the numbers written, the occurrences summed
        over the patterns and the bytes searched.  patterns: 1 .. 8 HOST byte strings.  zsmi_findRecordsQueryDevice"""
        q, keep = _find_query(patterns, mode, ignore_case)
        p = ctypes.c_void_p
        rc = self.L.zsmi_findRecordsQueryDevice(self.ctx, p(d_src_ptr), src_size, _delimiter(delimiter), ctypes.byref(q), p(d_base_ptr), p(d_records_ptr),
                                                p(d_hits_ptr), capacity, p(d_result_ptr))
        if rc:
            raise RuntimeError(f"zsmi_findRecordsQueryDevice: {_error_name(self.L, rc)}")

    def find_records_regex_device(self, d_src_ptr, src_size, regex, d_records_ptr, capacity, d_result_ptr, delimiter=b"\n", d_base_ptr=0):
        """find_records_regex on the device, the text in device memory (asynchronous: only queued): d_records (uint64[capacity]; 0 with
        capacity 0: only count) receives the ascending numbers of the records of d_src[0, src_size) that the program lists, d_result
        (uint64[4]) the total, the numbers written, the RECORDS of the text and the bytes searched.  regex: a compile_regex program, or
        bytes compiled on the spot (HOST memory: it reaches the kernels by value).  zsmi_findRecordsRegexDevice"""
        prog = _regex(regex)
        p = ctypes.c_void_p
        rc = self.L.zsmi_findRecordsRegexDevice(self.ctx, p(d_src_ptr), src_size, _delimiter(delimiter), ctypes.byref(prog), p(d_base_ptr), p(d_records_ptr),
                                                capacity, p(d_result_ptr))
        if rc:
            raise RuntimeError(f"zsmi_findRecordsRegexDevice: {_error_name(self.L, rc)}")

    def index_records_device(self, d_text_ptr, size, d_places_ptr, n, d_first_record_ptr, d_result_ptr, delimiter=b"\n", at_end=True, d_base_ptr=0):
        """index_records on the device, text and frame borders in device memory (asynchronous: only queued): d_places (uint64[n + 1],
        ascending, 0 first, size last) are the frames' borders in d_text[0, size); d_first_record (uint64[n + 1]) receives *d_base + the
        delimiters in front of each border (+ 1 at `size` for a tail without a delimiter when at_end says that `size` ends the content) -
        entry 0 only without a base -, d_result (uint64[4]) the status, the records, the misaligned frames and the delimiters.
        zsmi_indexRecordsDevice"""
        p = ctypes.c_void_p
        rc = self.L.zsmi_indexRecordsDevice(self.ctx, p(d_text_ptr), size, p(d_places_ptr), n, _delimiter(delimiter), 1 if at_end else 0, p(d_base_ptr),
                                            p(d_first_record_ptr), p(d_result_ptr))
        if rc:
            raise RuntimeError(f"zsmi_indexRecordsDevice: {_error_name(self.L, rc)}")

    def attach_record_index_resident(self, d_archive_ptr, capacity, d_archive_size_ptr, d_first_record_ptr, n, delimiter=b"\n"):
        """attach_record_index on an archive in device memory whose size is a device word, as compress_seekable_frames_resident left both
        (asynchronous: only queued): the index frame of d_first_record (uint64[n + 1]) goes between the last frame and the table, and the
        word becomes the new size or (uint64)-code; an error word that comes in stays.  capacity: the bytes at d_archive (the new size
        is 40 + 4 n + one table entry above the old).  zsmi_seekableAttachRecordIndexResident"""
        p = ctypes.c_void_p
        rc = self.L.zsmi_seekableAttachRecordIndexResident(self.ctx, p(d_archive_ptr), capacity, p(d_archive_size_ptr), p(d_first_record_ptr), n, _delimiter(delimiter))
        if rc:
            raise RuntimeError(f"zsmi_seekableAttachRecordIndexResident: {_error_name(self.L, rc)}")

    def build_frame_filter_device(self, d_text_ptr, size, d_places_ptr, n, d_filter_ptr, capacity, d_result_ptr, delimiter=b"\n", gram=4, log2_bits=13):
        """build_frame_filter on the device, text and frame borders in device memory (asynchronous: only queued): d_places (uint64[n + 1],
        ascending, 0 first, size last) are the frames' borders in d_text[0, size); d_filter (8-byte aligned, frame_filter_size(n,
        log2_bits) bytes) receives the complete frame, byte for byte the host call's; d_result (uint64[4]) the status, the bytes written,
        the saturated frames and the grams hashed.  zsmi_buildFrameFilterDevice"""
        p = ctypes.c_void_p
        rc = self.L.zsmi_buildFrameFilterDevice(self.ctx, p(d_text_ptr), size, p(d_places_ptr), n, _delimiter(delimiter), gram, log2_bits, p(d_filter_ptr), capacity,
                                                p(d_result_ptr))
        if rc:
            raise RuntimeError(f"zsmi_buildFrameFilterDevice: {_error_name(self.L, rc)}")

    def check_frame_filter_device(self, d_filter_ptr, filter_size, d_result_ptr):
        """read_frame_filter's judgement of a filter frame in device memory, check word included (asynchronous: only queued): d_result
        (uint64[8]) = {status, frames, delimiter, gram, log2_bits, the content's size, saturated frames, 0}.  zsmi_checkFrameFilterDevice"""
        p = ctypes.c_void_p
        rc = self.L.zsmi_checkFrameFilterDevice(self.ctx, p(d_filter_ptr), filter_size, p(d_result_ptr))
        if rc:
            raise RuntimeError(f"zsmi_checkFrameFilterDevice: {_error_name(self.L, rc)}")

    def filter_frames_device(self, d_filter_ptr, filter_size, patterns, first_frame, frame_count, d_frames_ptr, capacity, d_result_ptr, mode="any", ignore_case=False):
        """filter_frames on a filter frame in device memory (asynchronous: only queued): d_frames (uint32[capacity]) receives the ascending
        numbers of the frames of the window that pass the query, d_result (uint64[4]) = {total or (uint64)-code, written, frames tested,
        saturated frames among the total}.  zsmi_filterFramesDevice"""
        p = ctypes.c_void_p
        q, keep = _find_query(patterns, mode, ignore_case)
        rc = self.L.zsmi_filterFramesDevice(self.ctx, p(d_filter_ptr), filter_size, ctypes.byref(q), first_frame, frame_count, p(d_frames_ptr), capacity, p(d_result_ptr))
        if rc:
            raise RuntimeError(f"zsmi_filterFramesDevice: {_error_name(self.L, rc)}")

    def open_seekable_device(self, d_ptr, size, ddict=None, ddict_set=None):
        """the archive at d_ptr[0, size) (device memory, borrowed: it must outlive the handle) opened for reads: a SeekableHandle.  The
        table is read back and checked here, once (RuntimeError with the error's name).  ddict_set: a DecompressionDictSet its reads
        decode with (a record archive's dictionaries); ddict: one DecompressionDict instead.  Either must outlive the handle."""
        return SeekableHandle(self, d_ptr, size, ddict=ddict, ddict_set=ddict_set)

    def open_frames_device(self, d_ptr, size, ddict=None, ddict_set=None):
        """any stream of frames at d_ptr[0, size) (device memory, borrowed) opened for the same reads: a SeekableHandle over the frame
        index, which is built on the device here (zsmi_openFramesDevice; RuntimeError with the error's name for a stream it refuses).  One
        range over the whole content is the frame-parallel decode of a multi-frame stream.  ddict, ddict_set: as open_seekable_device."""
        return SeekableHandle(self, d_ptr, size, ddict=ddict, ddict_set=ddict_set, frames=True)

    def compress_host(self, src: np.ndarray, src_offsets, src_sizes, level=3, dictionary: bytes = b"", cdict=None, cdict_set=None, dict_index=None):
        """returns (arena uint8, dst_offsets uint64, dst_sizes uint32).  dictionary: one for every chunk (raw content or a formatted
        dictionary; zsmi_compressBatchHost_usingDict).  cdict: a CompressionDict instead (zsmi_compressBatchHost_usingCDict: its level holds).
        cdict_set, dict_index: a CompressionDictSet instead, chunk i with its member dict_index[i] or, for NO_DICT, with none
        (zsmi_compressBatchHost_usingCDictSet: the set's level holds)"""
        so = np.ascontiguousarray(src_offsets, dtype=np.uint64); ss = np.ascontiguousarray(src_sizes, dtype=np.uint32)
        n = len(ss)
        bounds = np.array([self.L.zsmi_compressBound(int(s)) for s in ss], dtype=np.uint64) if n < 4096 else \
            (ss.astype(np.uint64) + (ss.astype(np.uint64) >> 8) + 3 * (ss.astype(np.uint64) // 65536 + 1) + 18 + 64)
        do = np.zeros(n, dtype=np.uint64)
        if n > 1:
            do[1:] = np.cumsum(bounds)[:-1]
        arena = np.zeros(int(bounds.sum()), dtype=np.uint8)
        dsz = np.zeros(n, dtype=np.uint32)
        dbuf = np.frombuffer(bytes(dictionary or b""), dtype=np.uint8)
        name, tail = self._compress_form("zsmi_compressBatchHost", level, self._p(dbuf), len(dbuf), cdict, cdict_set, self._dict_index(dict_index, n))
        _check(getattr(self.L, name)(self.ctx, self._p(src), self._p(so), self._p(ss), n, self._p(arena), self._p(do), self._p(dsz), *tail), name)
        return arena, do, dsz

    def decompress_host(self, src: np.ndarray, src_offsets, src_sizes, dst_caps, dictionary: bytes = b"", ddict=None, ddict_set=None):
        """dictionary: every frame is decoded with it (raw content or a formatted dictionary; ZSTD_decompress_usingDict,
        ZStdDecompress.cs:2162).  ddict: a DecompressionDict instead (zsmi_decompressBatchHost_usingDDict).  ddict_set: a
        DecompressionDictSet instead - each frame's dictID picks its dictionary (zsmi_decompressBatchHost_usingDDictSet)"""
        if ddict_set is not None and (ddict is not None or dictionary):
            raise ValueError("ddict_set= excludes ddict= and dictionary=")
        so = np.ascontiguousarray(src_offsets, dtype=np.uint64); ss = np.ascontiguousarray(src_sizes, dtype=np.uint32)
        dc = np.ascontiguousarray(dst_caps, dtype=np.uint32)
        n = len(ss)
        do = np.zeros(n, dtype=np.uint64)
        if n > 1:
            do[1:] = np.cumsum(dc.astype(np.uint64))[:-1]
        arena = np.zeros(max(int(dc.astype(np.uint64).sum()), 1), dtype=np.uint8)
        dsz = np.zeros(n, dtype=np.uint32)
        if ddict_set is not None:
            rc = self.L.zsmi_decompressBatchHost_usingDDictSet(self.ctx, self._p(src), self._p(so), self._p(ss), n, self._p(arena), self._p(do), self._p(dc), self._p(dsz),
                                                               ddict_set.handle)
        elif ddict is not None:
            rc = self.L.zsmi_decompressBatchHost_usingDDict(self.ctx, self._p(src), self._p(so), self._p(ss), n, self._p(arena), self._p(do), self._p(dc), self._p(dsz),
                                                            ddict.handle)
        elif dictionary:
            dbuf = np.frombuffer(dictionary, dtype=np.uint8)
            rc = self.L.zsmi_decompressBatchHost_usingDict(self.ctx, self._p(src), self._p(so), self._p(ss), n, self._p(arena), self._p(do), self._p(dc), self._p(dsz),
                                                           self._p(dbuf), len(dbuf))
        else:
            rc = self.L.zsmi_decompressBatchHost(self.ctx, self._p(src), self._p(so), self._p(ss), n, self._p(arena), self._p(do), self._p(dc), self._p(dsz))
        _check(rc, "zsmi_decompressBatchHost")
        return arena, do, dsz

    def train_device(self, d_samples_ptr, offsets, sizes, capacity=65536, k=0, d=0, level=3, dict_id=0, f=0, steps=0, split_point=0.0, accel=0):
        """a dictionary trained on samples in device memory (zsmi_trainFromDevice; host offsets / sizes).  Returns (dictionary, k, d)"""
        so = np.ascontiguousarray(offsets, dtype=np.uint64); ss = np.ascontiguousarray(sizes, dtype=np.uint32)
        p = _params(k, d, f, steps, split_point, level, dict_id, accel)
        out = ctypes.create_string_buffer(max(int(capacity), 1))
        size = ctypes.c_size_t(0)
        rc = self.L.zsmi_trainFromDevice(self.ctx, ctypes.c_void_p(d_samples_ptr), self._p(so), self._p(ss), len(ss), out, capacity, ctypes.byref(p), ctypes.byref(size))
        if rc:
            raise RuntimeError(f"zsmi_trainFromDevice: {_error_name(self.L, rc)}")
        return out.raw[:size.value], p.k, p.d

    def kernel_times(self):
        out = (_lib.KernelTime * 64)()                                     # (a list search names more than 16 kernels)
        k = self.L.zsmi_getKernelTimes(self.ctx, out, 64)
        return {out[i].name.decode(): (out[i].seconds, out[i].launches) for i in range(k)}

    def enable_timing(self, on=True):
        """True / 1: events around every launch; 2: only around the dominant kernel (k_lz_walk*, k_dec_execute); False: off"""
        self.L.zsmi_enableKernelTiming(self.ctx, 2 if on == 2 else (1 if on else 0))
