"""MI355X-native Zstandard block codec: HIP kernels (csrc/) behind a C ABI (include/zsmi.h), with a host-side
mirror of the reference's public API (api.py)."""
from .api import ZStdDecompress, ZstdDecompressor, ZstdCompressor, SeekableArchive, SeekableHandle, BatchCodec, CompressionDict, CompressionDictSet, NO_DICT, DecompressionDict, DecompressionDictSet, train_dictionary, finalize_dictionary, get_dict_id   # noqa: F401
from .api import frame_content_size, find_frame_compressed_size, find_decompressed_size, decompress_bound, CONTENTSIZE_UNKNOWN, CONTENTSIZE_ERROR   # noqa: F401
from .api import count_frames, build_seek_table   # noqa: F401
from .api import split_records, find_records, find_records_query, compile_regex, find_records_regex   # noqa: F401
from .api import index_records, write_record_index_frame, read_record_index_frame, attach_record_index   # noqa: F401
from .api import frame_filter_size, build_frame_filter, read_frame_filter, filter_frames   # noqa: F401
