"""ctypes binding of libxlz.so (the C ABI declared in include/xlz.h).

There is no Python or CPU decode path behind this module: if the HIP library is
missing or no GPU is usable, calls fail loudly.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_SO = os.path.join(_HERE, "libxlz.so")
SO_PATH = os.environ.get("XLZ_SO") or DEFAULT_SO  # XLZ_SO: A/B builds (announced on stderr when used; bench.py refuses it)

# status codes (include/xlz.h)
OK = 0
OK_INPUT_EOF = 1
ERR_RESULT = -1
ERR_PROPS = -2
ERR_HEADER_EOF = -3
ERR_RC_INIT = -4
ERR_UNEXPECTED_EOF = -5
ERR_OUT_CAP = -6
ERR_BAD_ARG = -7
ERR_DEVICE = -8
ERR_UNSUPPORTED = -9
ERR_CLOSED = -10
ERR_NEED_ONE_READER = -11
ERR_INSUFFICIENT_PROPS = -12
EOF = 100
NEED_INPUT = 101

FMT_LZMA_ALONE = 0
FMT_LZMA_RAW = 1
FMT_LZMA2_RAW = 2

UNKNOWN_SIZE = 0xFFFFFFFFFFFFFFFF

CHECK_NONE = 0
CHECK_CRC32 = 1
CHECK_CRC64 = 4
CHECK_SHA256 = 10

# every symbol include/xlz.h declares (tests check the .so exports all of them)
EXPORTS = [
    "xlz_version", "xlz_build_id", "xlz_kernel_id", "xlz_strerror", "xlz_device_count", "xlz_decode_prop", "xlz_decode_dict_size",
    "xlz_decode_dict_size2", "xlz_decode_unpack_size", "xlz_ctx_create", "xlz_ctx_destroy",
    "xlz_ctx_device", "xlz_ctx_event_record", "xlz_ctx_event_elapsed_ms", "xlz_ctx_enable_batching",
    "xlz_ctx_batching_stats", "xlz_decode_batch", "xlz_ctx_last_call_stats", "xlz_batch_create", "xlz_batch_run", "xlz_batch_sync",
    "xlz_batch_results", "xlz_batch_download", "xlz_batch_device_output", "xlz_batch_last_kernel_ms",
    "xlz_batch_stats", "xlz_batch_destroy", "xlz_new_reader1", "xlz_new_reader2",
    "xlz_new_lzma_decompressor_for_sevenzip", "xlz_new_lzma2_decompressor_for_sevenzip",
    "xlz_reader_read", "xlz_reader_close", "xlz_reader_free", "xlz_xz_index", "xlz_xz_decode",
    "xlz_decode_batch_multi", "xlz_decode_batch_multi_plan", "xlz_xz_decode_multi", "xlz_7z_decode_multi", "xlz_batch_unit_trace", "xlz_reader_stats", "xlz_reader_memory", "xlz_batch_advice", "xlz_batch_launch_info", "xlz_reader_reset", "xlz_reader_reopen", "xlz_reader_expect_more", "xlz_reader_feed", "xlz_reader_feed_eof", "xlz_7z_index", "xlz_7z_decode",
    "xlz_lzma2_units", "xlz_ctx_set_slicing", "xlz_ctx_trim", "xlz_batch_kernel_name", "xlz_decode_batch_plan",
    "xlz_batch_checks", "xlz_decode_batch_checked", "xlz_crc32_combine", "xlz_crc64_combine", "xlz_ctx_set_check_mode",
    "xlz_ctx_check_mode", "xlz_ctx_last_check_stats",
    "xlz_filter_host", "xlz_batch_filter", "xlz_decode_batch_filtered", "xlz_ctx_set_filter_mode", "xlz_ctx_filter_mode",
    "xlz_ctx_last_filter_stats", "xlz_xz_index_chains", "xlz_7z_index_chains",
    "xlz_batch_digests", "xlz_decode_batch_digests", "xlz_sha256_plan", "xlz_ctx_last_sha256_stats",
    "xlz_batch_pack", "xlz_ctx_last_pack_stats", "xlz_xz_decode_device", "xlz_7z_decode_device",
    "xlz_bcj2_host", "xlz_batch_bcj2", "xlz_ctx_set_bcj2_mode", "xlz_ctx_bcj2_mode", "xlz_ctx_last_bcj2_stats", "xlz_7z_index_bcj2",
    "xlz_xz_open", "xlz_xz_close", "xlz_xz_file_info", "xlz_xz_file_blocks", "xlz_xz_cover", "xlz_xz_read", "xlz_xz_read_device",
    "xlz_ctx_last_xz_read_stats",
    "xlz_xz_many_layout", "xlz_xz_decode_many", "xlz_xz_decode_many_device", "xlz_ctx_last_xz_many_stats",
    "xlz_7z_open", "xlz_7z_close", "xlz_7z_archive_info", "xlz_7z_archive_entries", "xlz_7z_archive_folders", "xlz_7z_cover",
    "xlz_7z_extract_layout", "xlz_7z_extract", "xlz_7z_extract_device", "xlz_ctx_last_7z_extract_stats",
    "xlz_tar_parse_host", "xlz_tar_scan_device", "xlz_xz_tar_list", "xlz_tar_info", "xlz_tar_entries", "xlz_tar_close",
    "xlz_ctx_last_tar_stats",
    "xlz_zip_open", "xlz_zip_close", "xlz_zip_archive_info", "xlz_zip_archive_entries", "xlz_zip_extract_layout", "xlz_zip_extract",
    "xlz_zip_extract_device", "xlz_ctx_last_zip_extract_stats",
    "xlz_inflate_host", "xlz_inflate_batch", "xlz_ctx_set_deflate_mode", "xlz_ctx_deflate_mode", "xlz_ctx_last_inflate_stats",
    "xlz_adler32_device", "xlz_adler32_host", "xlz_adler32_combine",
    "xlz_gz_probe", "xlz_gz_decode_host", "xlz_gz_decode_many_device", "xlz_gz_decode_many", "xlz_ctx_last_gz_stats",
    "xlz_bz2_probe", "xlz_bz2_decode_host", "xlz_bz2_decode_many_device", "xlz_bz2_decode_many", "xlz_ctx_last_bz2_stats",
    "xlz_ctx_set_bz2_mode", "xlz_ctx_bz2_mode", "xlz_ctx_set_bz2_scratch", "xlz_crc32_bzip2_host",
]


class StreamDesc(ctypes.Structure):
    _fields_ = [
        ("inp", ctypes.c_void_p),
        ("in_len", ctypes.c_size_t),
        ("out", ctypes.c_void_p),
        ("out_cap", ctypes.c_size_t),
        ("format", ctypes.c_uint32),
        ("dict_size", ctypes.c_uint32),
        ("unpack_size", ctypes.c_uint64),
        ("props", ctypes.c_uint8),
        ("flags", ctypes.c_uint8),
        ("reserved", ctypes.c_uint8 * 6),
    ]


class Result(ctypes.Structure):
    _fields_ = [
        ("out_len", ctypes.c_uint64),
        ("in_consumed", ctypes.c_uint64),
        ("status", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
    ]


class CallStats(ctypes.Structure):
    _fields_ = [("upload_ms", ctypes.c_double), ("decode_ms", ctypes.c_double), ("download_ms", ctypes.c_double),
                ("total_ms", ctypes.c_double), ("kernel_span_ms", ctypes.c_double), ("slot_occupancy", ctypes.c_double),
                ("streams", ctypes.c_uint64), ("units", ctypes.c_uint64), ("wave_slots", ctypes.c_uint32),
                ("sub_batches", ctypes.c_uint32), ("slices", ctypes.c_uint32), ("refetched", ctypes.c_uint32)]


class CheckRange(ctypes.Structure):
    _fields_ = [("stream", ctypes.c_uint64), ("off", ctypes.c_uint64), ("len", ctypes.c_uint64), ("kind", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32)]


class CheckStats(ctypes.Structure):
    _fields_ = [("device_ranges", ctypes.c_uint64), ("device_bytes", ctypes.c_uint64), ("host_ranges", ctypes.c_uint64),
                ("host_bytes", ctypes.c_uint64), ("empty_ranges", ctypes.c_uint64), ("kernel_ms", ctypes.c_double),
                ("launches", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class Digest(ctypes.Structure):
    _fields_ = [("b", ctypes.c_uint8 * 32)]


class Sha256Stats(ctypes.Structure):
    _fields_ = [("device_ranges", ctypes.c_uint64), ("device_bytes", ctypes.c_uint64), ("host_ranges", ctypes.c_uint64),
                ("host_bytes", ctypes.c_uint64), ("empty_ranges", ctypes.c_uint64), ("threshold", ctypes.c_uint64),
                ("kernel_ms", ctypes.c_double), ("launches", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class FilterStep(ctypes.Structure):
    _fields_ = [("stream", ctypes.c_uint64), ("id", ctypes.c_uint32), ("param", ctypes.c_uint32), ("reserved", ctypes.c_uint32 * 2)]


class FilterStats(ctypes.Structure):
    _fields_ = [("device_steps", ctypes.c_uint64), ("device_bytes", ctypes.c_uint64), ("host_steps", ctypes.c_uint64),
                ("host_bytes", ctypes.c_uint64), ("empty_steps", ctypes.c_uint64), ("kernel_ms", ctypes.c_double),
                ("launches", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class PackItem(ctypes.Structure):
    _fields_ = [("stream", ctypes.c_uint64), ("off", ctypes.c_uint64), ("len", ctypes.c_uint64), ("dst_off", ctypes.c_uint64)]


class PackStats(ctypes.Structure):
    _fields_ = [("items", ctypes.c_uint64), ("bytes", ctypes.c_uint64), ("congruent_items", ctypes.c_uint64),
                ("empty_items", ctypes.c_uint64), ("kernel_ms", ctypes.c_double), ("launches", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32)]


BCJ2_RAW = 0xFFFFFFFFFFFFFFFF
SZ_BCJ2 = 4  # xlz_7z_folder.method of a BCJ2 folder (xlz_7z_index_bcj2 only)


class Bcj2Src(ctypes.Structure):
    _fields_ = [("stream", ctypes.c_uint64), ("raw", ctypes.c_void_p), ("raw_len", ctypes.c_uint64)]


class Bcj2Item(ctypes.Structure):
    _fields_ = [("main_s", Bcj2Src), ("call_s", Bcj2Src), ("jump_s", Bcj2Src), ("rc", ctypes.c_void_p), ("rc_len", ctypes.c_uint64),
                ("out_len", ctypes.c_uint64), ("dst_off", ctypes.c_uint64)]


class Bcj2Result(ctypes.Structure):
    _fields_ = [("produced", ctypes.c_uint64), ("status", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class Bcj2Stats(ctypes.Structure):
    _fields_ = [("device_items", ctypes.c_uint64), ("device_bytes", ctypes.c_uint64), ("host_items", ctypes.c_uint64),
                ("host_bytes", ctypes.c_uint64), ("failed_items", ctypes.c_uint64), ("kernel_ms", ctypes.c_double),
                ("launches", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class SzBcj2Sub(ctypes.Structure):
    _fields_ = [("pack_off", ctypes.c_uint64), ("pack_len", ctypes.c_uint64), ("unpack_len", ctypes.c_uint64), ("method", ctypes.c_uint32),
                ("dict_size", ctypes.c_uint32), ("props", ctypes.c_uint8), ("reserved", ctypes.c_uint8 * 7)]


class SzBcj2(ctypes.Structure):
    _fields_ = [("folder", ctypes.c_uint64), ("main_s", SzBcj2Sub), ("call_s", SzBcj2Sub), ("jump_s", SzBcj2Sub), ("rc_off", ctypes.c_uint64),
                ("rc_len", ctypes.c_uint64)]


class XzBlock(ctypes.Structure):
    _fields_ = [
        ("comp_off", ctypes.c_uint64),
        ("comp_len", ctypes.c_uint64),
        ("uncomp_off", ctypes.c_uint64),
        ("uncomp_len", ctypes.c_uint64),
        ("check_off", ctypes.c_uint64),
        ("dict_size", ctypes.c_uint32),
        ("check_type", ctypes.c_uint32),
    ]


class XzRange(ctypes.Structure):
    _fields_ = [("off", ctypes.c_uint64), ("len", ctypes.c_uint64), ("dst_off", ctypes.c_uint64)]


class XzReadStats(ctypes.Structure):
    _fields_ = [("ranges", ctypes.c_uint64), ("empty_ranges", ctypes.c_uint64), ("blocks", ctypes.c_uint64),
                ("comp_bytes", ctypes.c_uint64), ("decoded_bytes", ctypes.c_uint64), ("copied_bytes", ctypes.c_uint64)]


class XzManyFile(ctypes.Structure):
    _fields_ = [("file", ctypes.c_void_p), ("len", ctypes.c_size_t), ("dst_off", ctypes.c_uint64), ("dst_cap", ctypes.c_uint64)]


class XzManyResult(ctypes.Structure):
    _fields_ = [("status", ctypes.c_int32), ("unverified", ctypes.c_uint32), ("out_len", ctypes.c_uint64), ("blocks", ctypes.c_uint64),
                ("comp_bytes", ctypes.c_uint64)]


class XzManyStats(ctypes.Structure):
    _fields_ = [("files", ctypes.c_uint64), ("failed_files", ctypes.c_uint64), ("blocks", ctypes.c_uint64),
                ("comp_bytes", ctypes.c_uint64), ("decoded_bytes", ctypes.c_uint64)]


SZ_NO_FOLDER = 0xFFFFFFFFFFFFFFFF
SZ_ENTRY_HAS_STREAM, SZ_ENTRY_HAS_CRC, SZ_ENTRY_IS_DIR, SZ_ENTRY_IS_ANTI, SZ_ENTRY_HAS_MTIME, SZ_ENTRY_HAS_ATTRIBUTES = 1, 2, 4, 8, 16, 32


class SzEntry(ctypes.Structure):
    _fields_ = [("size", ctypes.c_uint64), ("folder", ctypes.c_uint64), ("folder_off", ctypes.c_uint64), ("substream", ctypes.c_uint64),
                ("mtime", ctypes.c_uint64), ("name_off", ctypes.c_uint64), ("name_len", ctypes.c_uint32), ("crc", ctypes.c_uint32),
                ("attributes", ctypes.c_uint32), ("flags", ctypes.c_uint32)]


class SzWant(ctypes.Structure):
    _fields_ = [("entry", ctypes.c_uint64), ("dst_off", ctypes.c_uint64), ("dst_cap", ctypes.c_uint64)]


class SzFileResult(ctypes.Structure):
    _fields_ = [("status", ctypes.c_int32), ("unverified", ctypes.c_uint32), ("out_len", ctypes.c_uint64)]


class SzCoverItem(ctypes.Structure):
    _fields_ = [("folder", ctypes.c_uint64), ("decode_len", ctypes.c_uint64), ("in_len", ctypes.c_uint64)]


class SzExtractStats(ctypes.Structure):
    _fields_ = [("entries", ctypes.c_uint64), ("empty_entries", ctypes.c_uint64), ("failed_entries", ctypes.c_uint64),
                ("folders", ctypes.c_uint64), ("comp_bytes", ctypes.c_uint64), ("decoded_bytes", ctypes.c_uint64),
                ("folder_bytes", ctypes.c_uint64), ("copied_bytes", ctypes.c_uint64)]


ZIP_ENTRY_SUPPORTED, ZIP_ENTRY_IS_DIR, ZIP_ENTRY_UTF8, ZIP_ENTRY_ENCRYPTED = 1, 2, 4, 8
ZIP_ENTRY_HAS_DESCRIPTOR, ZIP_ENTRY_ZIP64, ZIP_ENTRY_BAD, ZIP_ENTRY_END_MARKER = 16, 32, 64, 128
ZIP_ENTRY_DEFLATE = 256  # method 8 and well formed: what deflate mode 1 / 2 inflates (beside the classes, which it leaves alone)


class InflateItem(ctypes.Structure):
    _fields_ = [("inp", ctypes.c_void_p), ("in_len", ctypes.c_uint64), ("dst_off", ctypes.c_uint64), ("dst_cap", ctypes.c_uint64)]


class InflateResult(ctypes.Structure):
    _fields_ = [("produced", ctypes.c_uint64), ("in_consumed", ctypes.c_uint64), ("status", ctypes.c_int32), ("reserved", ctypes.c_uint32)]


class InflateStats(ctypes.Structure):
    _fields_ = [("device_items", ctypes.c_uint64), ("device_bytes", ctypes.c_uint64), ("host_items", ctypes.c_uint64),
                ("host_bytes", ctypes.c_uint64), ("failed_items", ctypes.c_uint64), ("uploads", ctypes.c_uint32),
                ("launches", ctypes.c_uint32)]


class AdlerRange(ctypes.Structure):
    _fields_ = [("off", ctypes.c_uint64), ("len", ctypes.c_uint64)]


GZ_AUTO, GZ_GZIP, GZ_ZLIB = 0, 1, 2
GZ_F_BGZF, GZ_F_NAME, GZ_F_COMMENT, GZ_F_HCRC = 1, 2, 4, 8


class GzInfo(ctypes.Structure):
    _fields_ = [("format", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("members", ctypes.c_uint64), ("size_hint", ctypes.c_uint64),
                ("mtime", ctypes.c_uint32), ("name_off", ctypes.c_uint32), ("name_len", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class GzFile(ctypes.Structure):
    _fields_ = [("inp", ctypes.c_void_p), ("in_len", ctypes.c_uint64), ("dst_off", ctypes.c_uint64), ("dst_cap", ctypes.c_uint64),
                ("format", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class GzResult(ctypes.Structure):
    _fields_ = [("status", ctypes.c_int32), ("members", ctypes.c_uint32), ("out_len", ctypes.c_uint64), ("in_consumed", ctypes.c_uint64)]


class GzStats(ctypes.Structure):
    _fields_ = [("files", ctypes.c_uint64), ("failed_files", ctypes.c_uint64), ("bgzf_files", ctypes.c_uint64), ("members", ctypes.c_uint64),
                ("device_items", ctypes.c_uint64), ("host_items", ctypes.c_uint64), ("crc_ranges", ctypes.c_uint64),
                ("adler_ranges", ctypes.c_uint64), ("rounds", ctypes.c_uint32), ("uploads", ctypes.c_uint32),
                ("adler_kernel_ms", ctypes.c_double)]


class Bz2Info(ctypes.Structure):
    _fields_ = [("level", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("candidates", ctypes.c_uint64), ("streams", ctypes.c_uint64),
                ("size_hint", ctypes.c_uint64), ("size_bound", ctypes.c_uint64)]


class Bz2File(ctypes.Structure):
    _fields_ = [("inp", ctypes.c_void_p), ("in_len", ctypes.c_uint64), ("dst_off", ctypes.c_uint64), ("dst_cap", ctypes.c_uint64)]


class Bz2Result(ctypes.Structure):
    _fields_ = [("status", ctypes.c_int32), ("blocks", ctypes.c_uint32), ("out_len", ctypes.c_uint64), ("in_consumed", ctypes.c_uint64),
                ("streams", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class Bz2Stats(ctypes.Structure):
    _fields_ = [("files", ctypes.c_uint64), ("failed_files", ctypes.c_uint64), ("candidates", ctypes.c_uint64), ("chain_blocks", ctypes.c_uint64),
                ("discarded_blocks", ctypes.c_uint64), ("device_blocks", ctypes.c_uint64), ("host_blocks", ctypes.c_uint64),
                ("device_bytes", ctypes.c_uint64), ("host_bytes", ctypes.c_uint64), ("rounds", ctypes.c_uint32), ("uploads", ctypes.c_uint32),
                ("symbols_ms", ctypes.c_double), ("walk_ms", ctypes.c_double), ("expand_ms", ctypes.c_double), ("crc_ms", ctypes.c_double)]


class ZipEntry(ctypes.Structure):
    _fields_ = [("size", ctypes.c_uint64), ("comp_size", ctypes.c_uint64), ("header_off", ctypes.c_uint64), ("data_off", ctypes.c_uint64),
                ("name_off", ctypes.c_uint64), ("name_len", ctypes.c_uint32), ("crc", ctypes.c_uint32), ("dos_time_date", ctypes.c_uint32),
                ("external_attr", ctypes.c_uint32), ("dict_size", ctypes.c_uint32), ("method", ctypes.c_uint16), ("gp_flags", ctypes.c_uint16),
                ("props", ctypes.c_uint8), ("reserved", ctypes.c_uint8 * 3), ("flags", ctypes.c_uint32)]


class ZipWant(ctypes.Structure):
    _fields_ = [("entry", ctypes.c_uint64), ("dst_off", ctypes.c_uint64), ("dst_cap", ctypes.c_uint64)]


class ZipFileResult(ctypes.Structure):
    _fields_ = [("status", ctypes.c_int32), ("reserved", ctypes.c_uint32), ("out_len", ctypes.c_uint64)]


class ZipExtractStats(ctypes.Structure):
    _fields_ = [("entries", ctypes.c_uint64), ("empty_entries", ctypes.c_uint64), ("failed_entries", ctypes.c_uint64),
                ("lzma_entries", ctypes.c_uint64), ("stored_entries", ctypes.c_uint64), ("comp_bytes", ctypes.c_uint64),
                ("copied_bytes", ctypes.c_uint64), ("stored_uploads", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class TarEntry(ctypes.Structure):
    _fields_ = [("hdr_off", ctypes.c_uint64), ("data_off", ctypes.c_uint64), ("size", ctypes.c_uint64), ("mtime_s", ctypes.c_int64),
                ("mtime_ns", ctypes.c_uint32), ("mode", ctypes.c_uint32), ("uid", ctypes.c_uint32), ("gid", ctypes.c_uint32),
                ("name_off", ctypes.c_uint32), ("name_len", ctypes.c_uint32), ("link_off", ctypes.c_uint32), ("link_len", ctypes.c_uint32),
                ("type", ctypes.c_uint8), ("reserved", ctypes.c_uint8 * 7)]


class TarStats(ctypes.Structure):
    _fields_ = [("blocks", ctypes.c_uint64), ("zero_blocks", ctypes.c_uint64), ("candidate_blocks", ctypes.c_uint64),
                ("header_blocks", ctypes.c_uint64), ("meta_bytes", ctypes.c_uint64), ("downloaded_bytes", ctypes.c_uint64),
                ("kernel_ms", ctypes.c_double), ("launches", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class Lzma2Unit(ctypes.Structure):
    _fields_ = [
        ("in_off", ctypes.c_uint64),
        ("in_len", ctypes.c_uint64),
        ("out_off", ctypes.c_uint64),
        ("out_len", ctypes.c_uint64),
        ("have_reader", ctypes.c_uint32),
        ("reserved", ctypes.c_uint32),
    ]


class MultiItem(ctypes.Structure):
    _fields_ = [
        ("stream", ctypes.c_uint64),
        ("in_off", ctypes.c_uint64),
        ("in_len", ctypes.c_uint64),
        ("out_off", ctypes.c_uint64),
        ("out_len", ctypes.c_uint64),
        ("context", ctypes.c_uint32),
        ("flags", ctypes.c_uint32),
    ]


class Advice(ctypes.Structure):
    _fields_ = [
        ("units", ctypes.c_uint64),
        ("in_bytes", ctypes.c_uint64),
        ("wave_slots", ctypes.c_uint32),
        ("break_even_units", ctypes.c_uint32),
        ("fill", ctypes.c_double),
        ("prefer_cpu", ctypes.c_int32),
        ("reserved", ctypes.c_uint32),
        ("cpu_cost", ctypes.c_double),
        ("gpu_cost", ctypes.c_double),
    ]


class SzFolder(ctypes.Structure):
    _fields_ = [
        ("pack_off", ctypes.c_uint64),
        ("pack_len", ctypes.c_uint64),
        ("unpack_off", ctypes.c_uint64),
        ("unpack_len", ctypes.c_uint64),
        ("method", ctypes.c_uint32),
        ("dict_size", ctypes.c_uint32),
        ("crc", ctypes.c_uint32),
        ("first_substream", ctypes.c_uint32),
        ("n_substreams", ctypes.c_uint32),
        ("props", ctypes.c_uint8),
        ("has_crc", ctypes.c_uint8),
        ("reserved", ctypes.c_uint8 * 2),
    ]


class SzSubstream(ctypes.Structure):
    _fields_ = [("size", ctypes.c_uint64), ("crc", ctypes.c_uint32), ("has_crc", ctypes.c_uint32)]


_lib = None


def lib():
    """Load libxlz.so; raises if it has not been built (lzma_amd.build.build())."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(SO_PATH):
        raise RuntimeError(
            "lzma_amd: %s is missing -- build the HIP extension first "
            "(python -m lzma_amd.build); there is no CPU fallback" % SO_PATH)
    if SO_PATH != DEFAULT_SO:
        import sys
        print("lzma_amd: XLZ_SO is set -- loading %s instead of the in-tree library" % SO_PATH, file=sys.stderr)
    L = ctypes.CDLL(SO_PATH)
    vp, sz, i32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
    L.xlz_version.restype = ctypes.c_char_p
    L.xlz_build_id.restype = ctypes.c_char_p
    L.xlz_kernel_id.restype = ctypes.c_char_p
    L.xlz_strerror.restype = ctypes.c_char_p
    L.xlz_strerror.argtypes = [i32]
    L.xlz_device_count.restype = i32
    L.xlz_decode_prop.argtypes = [ctypes.c_uint8] + [ctypes.POINTER(ctypes.c_uint8)] * 3
    L.xlz_decode_dict_size.restype = ctypes.c_uint32
    L.xlz_decode_dict_size.argtypes = [ctypes.c_char_p]
    L.xlz_decode_dict_size2.restype = ctypes.c_uint32
    L.xlz_decode_dict_size2.argtypes = [ctypes.c_uint8]
    L.xlz_decode_unpack_size.restype = ctypes.c_uint64
    L.xlz_decode_unpack_size.argtypes = [ctypes.c_char_p]
    L.xlz_ctx_create.argtypes = [i32, ctypes.POINTER(vp)]
    L.xlz_ctx_destroy.argtypes = [vp]
    L.xlz_ctx_destroy.restype = None
    L.xlz_ctx_device.argtypes = [vp]
    L.xlz_ctx_enable_batching.argtypes = [vp, ctypes.c_uint32, ctypes.c_uint32]
    L.xlz_ctx_batching_stats.argtypes = [vp, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]
    L.xlz_ctx_event_record.argtypes = [vp, i32]
    L.xlz_ctx_event_elapsed_ms.argtypes = [vp, i32, i32, ctypes.POINTER(ctypes.c_float)]
    L.xlz_decode_batch.argtypes = [vp, ctypes.POINTER(StreamDesc), sz, ctypes.POINTER(Result)]
    L.xlz_ctx_last_call_stats.argtypes = [vp, ctypes.POINTER(CallStats)]
    L.xlz_ctx_set_slicing.argtypes = [vp, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32]
    L.xlz_ctx_trim.argtypes = [vp, ctypes.POINTER(ctypes.c_uint64)]
    L.xlz_decode_batch_plan.argtypes = [ctypes.POINTER(StreamDesc), sz, ctypes.POINTER(sz), sz, ctypes.POINTER(sz), ctypes.POINTER(i32)]
    L.xlz_batch_kernel_name.argtypes = [vp]
    L.xlz_batch_checks.argtypes = [vp, ctypes.POINTER(CheckRange), sz, ctypes.POINTER(ctypes.c_uint64)]
    L.xlz_decode_batch_checked.argtypes = [vp, ctypes.POINTER(StreamDesc), sz, ctypes.POINTER(Result), ctypes.POINTER(CheckRange), sz,
                                           ctypes.POINTER(ctypes.c_uint64)]
    L.xlz_crc32_combine.restype = ctypes.c_uint32
    L.xlz_crc32_combine.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint64]
    L.xlz_crc64_combine.restype = ctypes.c_uint64
    L.xlz_crc64_combine.argtypes = [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64]
    L.xlz_ctx_set_check_mode.argtypes = [vp, i32]
    L.xlz_ctx_check_mode.argtypes = [vp]
    L.xlz_ctx_last_check_stats.argtypes = [vp, ctypes.POINTER(CheckStats)]
    L.xlz_batch_kernel_name.restype = ctypes.c_char_p
    L.xlz_batch_create.argtypes = [vp, ctypes.POINTER(StreamDesc), sz, ctypes.POINTER(vp)]
    L.xlz_batch_run.argtypes = [vp]
    L.xlz_batch_sync.argtypes = [vp]
    L.xlz_batch_results.argtypes = [vp, ctypes.POINTER(Result)]
    L.xlz_batch_download.argtypes = [vp, sz, vp, sz]
    L.xlz_batch_device_output.argtypes = [vp, sz, ctypes.POINTER(vp), ctypes.POINTER(sz)]
    L.xlz_batch_last_kernel_ms.argtypes = [vp, ctypes.POINTER(ctypes.c_float)]
    L.xlz_batch_stats.argtypes = [vp] + [ctypes.POINTER(ctypes.c_uint64)] * 3
    L.xlz_batch_destroy.argtypes = [vp]
    L.xlz_batch_destroy.restype = None
    L.xlz_new_reader1.restype = vp
    L.xlz_new_reader1.argtypes = [vp, ctypes.c_char_p, sz, ctypes.POINTER(i32)]
    L.xlz_new_reader2.restype = vp
    L.xlz_new_reader2.argtypes = [vp, ctypes.c_char_p, sz, i32, ctypes.POINTER(i32)]
    for f in (L.xlz_new_lzma_decompressor_for_sevenzip, L.xlz_new_lzma2_decompressor_for_sevenzip):
        f.restype = vp
        f.argtypes = [vp, ctypes.c_char_p, sz, ctypes.c_uint64, ctypes.POINTER(ctypes.c_char_p),
                      ctypes.POINTER(sz), sz, ctypes.POINTER(i32)]
    L.xlz_reader_read.restype = ctypes.c_long
    L.xlz_reader_read.argtypes = [vp, vp, sz, ctypes.POINTER(i32)]
    L.xlz_reader_close.argtypes = [vp]
    L.xlz_reader_free.argtypes = [vp]
    L.xlz_reader_free.restype = None
    L.xlz_reader_reset.argtypes = [vp]
    L.xlz_reader_reopen.argtypes = [vp, ctypes.c_char_p, sz, ctypes.c_uint64]
    L.xlz_reader_expect_more.argtypes = [vp]
    L.xlz_reader_feed.argtypes = [vp, ctypes.c_char_p, sz]
    L.xlz_reader_feed_eof.argtypes = [vp]
    L.xlz_reader_stats.argtypes = [vp] + [ctypes.POINTER(ctypes.c_uint64)] * 3
    L.xlz_reader_memory.argtypes = [vp] + [ctypes.POINTER(ctypes.c_uint64)] * 2
    L.xlz_batch_advice.argtypes = [vp, ctypes.POINTER(StreamDesc), sz, ctypes.c_uint32, ctypes.POINTER(Advice)]
    L.xlz_batch_launch_info.argtypes = [vp, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32)]
    L.xlz_batch_unit_trace.argtypes = [vp, vp, vp, vp, sz, ctypes.POINTER(sz)]
    L.xlz_decode_batch_multi.argtypes = [ctypes.POINTER(vp), sz, ctypes.POINTER(StreamDesc), sz, ctypes.POINTER(Result)]
    L.xlz_decode_batch_multi_plan.argtypes = [sz, ctypes.POINTER(StreamDesc), sz, ctypes.POINTER(MultiItem), sz, ctypes.POINTER(sz)]
    L.xlz_xz_index.argtypes = [vp, sz, ctypes.POINTER(XzBlock), sz, ctypes.POINTER(sz), ctypes.POINTER(ctypes.c_uint64)]
    L.xlz_lzma2_units.argtypes = [ctypes.c_char_p, sz, ctypes.POINTER(Lzma2Unit), sz, ctypes.POINTER(sz)]
    L.xlz_7z_index.argtypes = [vp, vp, sz, ctypes.POINTER(SzFolder), sz, ctypes.POINTER(sz), ctypes.POINTER(SzSubstream), sz,
                               ctypes.POINTER(sz), ctypes.POINTER(ctypes.c_uint64)]
    L.xlz_7z_decode.argtypes = [vp, vp, sz, vp, sz, ctypes.POINTER(ctypes.c_uint64), i32, ctypes.POINTER(sz)]
    L.xlz_xz_decode.argtypes = [vp, vp, sz, vp, sz, ctypes.POINTER(ctypes.c_uint64), i32, ctypes.POINTER(sz)]
    L.xlz_xz_decode_multi.argtypes = [ctypes.POINTER(vp), sz, vp, sz, vp, sz, ctypes.POINTER(ctypes.c_uint64), i32, ctypes.POINTER(sz)]
    L.xlz_7z_decode_multi.argtypes = [ctypes.POINTER(vp), sz, vp, sz, vp, sz, ctypes.POINTER(ctypes.c_uint64), i32, ctypes.POINTER(sz)]
    if hasattr(L, "xlz_filter_host"):  # (an older library loaded through XLZ_SO for an A/B run has no filters)
        L.xlz_filter_host.argtypes = [ctypes.c_uint32, ctypes.c_uint32, vp, sz]
        L.xlz_batch_filter.argtypes = [vp, ctypes.POINTER(FilterStep), sz]
        L.xlz_decode_batch_filtered.argtypes = [vp, ctypes.POINTER(StreamDesc), sz, ctypes.POINTER(Result), ctypes.POINTER(FilterStep), sz,
                                                ctypes.POINTER(CheckRange), sz, ctypes.POINTER(ctypes.c_uint64)]
        L.xlz_ctx_set_filter_mode.argtypes = [vp, i32]
        L.xlz_ctx_filter_mode.argtypes = [vp]
        L.xlz_ctx_last_filter_stats.argtypes = [vp, ctypes.POINTER(FilterStats)]
        L.xlz_xz_index_chains.argtypes = [vp, sz, ctypes.POINTER(XzBlock), sz, ctypes.POINTER(sz), ctypes.POINTER(FilterStep), sz,
                                          ctypes.POINTER(sz), ctypes.POINTER(ctypes.c_uint64)]
        L.xlz_7z_index_chains.argtypes = [vp, vp, sz, ctypes.POINTER(SzFolder), sz, ctypes.POINTER(sz), ctypes.POINTER(SzSubstream), sz,
                                          ctypes.POINTER(sz), ctypes.POINTER(FilterStep), sz, ctypes.POINTER(sz),
                                          ctypes.POINTER(ctypes.c_uint64)]
    if hasattr(L, "xlz_batch_digests"):  # (an older library loaded through XLZ_SO has no SHA-256 on the device)
        L.xlz_batch_digests.argtypes = [vp, ctypes.POINTER(CheckRange), sz, ctypes.POINTER(Digest)]
        L.xlz_decode_batch_digests.argtypes = [vp, ctypes.POINTER(StreamDesc), sz, ctypes.POINTER(Result), ctypes.POINTER(FilterStep), sz,
                                               ctypes.POINTER(CheckRange), sz, ctypes.POINTER(Digest)]
        L.xlz_sha256_plan.argtypes = [ctypes.POINTER(ctypes.c_uint64), sz, ctypes.c_uint32, ctypes.c_double, ctypes.c_double,
                                      ctypes.POINTER(ctypes.c_uint8)]
        L.xlz_ctx_last_sha256_stats.argtypes = [vp, ctypes.POINTER(Sha256Stats)]
    if hasattr(L, "xlz_batch_pack"):  # (an older library loaded through XLZ_SO has no pack into device memory)
        L.xlz_batch_pack.argtypes = [vp, ctypes.POINTER(PackItem), sz, vp, sz, ctypes.POINTER(ctypes.c_uint64)]
        L.xlz_ctx_last_pack_stats.argtypes = [vp, ctypes.POINTER(PackStats)]
        L.xlz_xz_decode_device.argtypes = [vp, vp, sz, vp, sz, ctypes.POINTER(ctypes.c_uint64), i32, ctypes.POINTER(sz)]
        L.xlz_7z_decode_device.argtypes = [vp, vp, sz, vp, sz, ctypes.POINTER(ctypes.c_uint64), i32, ctypes.POINTER(sz)]
    if hasattr(L, "xlz_bcj2_host"):  # (an older library loaded through XLZ_SO knows no BCJ2 folders)
        L.xlz_bcj2_host.argtypes = [vp, sz, vp, sz, vp, sz, vp, sz, vp, sz]
        L.xlz_batch_bcj2.argtypes = [vp, ctypes.POINTER(Bcj2Item), sz, vp, sz, ctypes.POINTER(Bcj2Result)]
        L.xlz_ctx_set_bcj2_mode.argtypes = [vp, i32]
        L.xlz_ctx_bcj2_mode.argtypes = [vp]
        L.xlz_ctx_last_bcj2_stats.argtypes = [vp, ctypes.POINTER(Bcj2Stats)]
        L.xlz_7z_index_bcj2.argtypes = [vp, vp, sz, ctypes.POINTER(SzFolder), sz, ctypes.POINTER(sz), ctypes.POINTER(SzSubstream), sz,
                                        ctypes.POINTER(sz), ctypes.POINTER(FilterStep), sz, ctypes.POINTER(sz), ctypes.POINTER(SzBcj2), sz,
                                        ctypes.POINTER(sz), ctypes.POINTER(ctypes.c_uint64)]
    if hasattr(L, "xlz_xz_open"):  # (an older library loaded through XLZ_SO reads no byte ranges of a file)
        L.xlz_xz_open.argtypes = [vp, sz, ctypes.POINTER(vp)]
        L.xlz_xz_close.argtypes = [vp]
        L.xlz_xz_close.restype = None
        L.xlz_xz_file_info.argtypes = [vp, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(sz), ctypes.POINTER(sz)]
        L.xlz_xz_file_blocks.argtypes = [vp, ctypes.POINTER(XzBlock), sz]
        L.xlz_xz_cover.argtypes = [vp, ctypes.POINTER(XzRange), sz, ctypes.POINTER(sz), sz, ctypes.POINTER(sz)]
        L.xlz_xz_read.argtypes = [vp, vp, ctypes.POINTER(XzRange), sz, vp, sz, ctypes.POINTER(ctypes.c_uint64), i32, ctypes.POINTER(sz)]
        L.xlz_xz_read_device.argtypes = L.xlz_xz_read.argtypes
        L.xlz_ctx_last_xz_read_stats.argtypes = [vp, ctypes.POINTER(XzReadStats)]
    if hasattr(L, "xlz_xz_decode_many"):  # (an older library loaded through XLZ_SO decodes one file per call)
        L.xlz_xz_many_layout.argtypes = [ctypes.POINTER(XzManyFile), sz, i32, ctypes.c_uint64, ctypes.POINTER(XzManyResult),
                                         ctypes.POINTER(ctypes.c_uint64)]
        L.xlz_xz_decode_many.argtypes = [vp, ctypes.POINTER(XzManyFile), sz, vp, sz, i32, ctypes.POINTER(XzManyResult)]
        L.xlz_xz_decode_many_device.argtypes = L.xlz_xz_decode_many.argtypes
        L.xlz_ctx_last_xz_many_stats.argtypes = [vp, ctypes.POINTER(XzManyStats)]
    if hasattr(L, "xlz_7z_open"):  # (an older library loaded through XLZ_SO has no file table)
        L.xlz_7z_open.argtypes = [vp, vp, sz, ctypes.POINTER(vp)]
        L.xlz_7z_close.argtypes = [vp]
        L.xlz_7z_close.restype = None
        L.xlz_7z_archive_info.argtypes = [vp, ctypes.POINTER(sz), ctypes.POINTER(sz), ctypes.POINTER(sz), ctypes.POINTER(ctypes.c_uint64)]
        L.xlz_7z_archive_entries.argtypes = [vp, ctypes.POINTER(SzEntry), sz, vp, sz]
        L.xlz_7z_archive_folders.argtypes = [vp, ctypes.POINTER(SzFolder), sz]
        L.xlz_7z_cover.argtypes = [vp, ctypes.POINTER(ctypes.c_uint64), sz, ctypes.POINTER(SzCoverItem), sz, ctypes.POINTER(sz)]
        L.xlz_7z_extract_layout.argtypes = [vp, ctypes.POINTER(SzWant), sz, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64)]
        L.xlz_7z_extract.argtypes = [vp, vp, ctypes.POINTER(SzWant), sz, vp, sz, i32, ctypes.POINTER(SzFileResult)]
        L.xlz_7z_extract_device.argtypes = L.xlz_7z_extract.argtypes
        L.xlz_ctx_last_7z_extract_stats.argtypes = [vp, ctypes.POINTER(SzExtractStats)]
    if hasattr(L, "xlz_tar_parse_host"):  # (an older library loaded through XLZ_SO lists no .tar members)
        L.xlz_tar_parse_host.argtypes = [vp, ctypes.c_uint64, ctypes.POINTER(vp)]
        L.xlz_tar_scan_device.argtypes = [vp, vp, ctypes.c_uint64, ctypes.POINTER(vp)]
        L.xlz_xz_tar_list.argtypes = [vp, vp, i32, ctypes.POINTER(vp), ctypes.POINTER(sz)]
        L.xlz_tar_info.argtypes = [vp, ctypes.POINTER(sz), ctypes.POINTER(sz), ctypes.POINTER(i32), ctypes.POINTER(ctypes.c_uint64)]
        L.xlz_tar_info.restype = None
        L.xlz_tar_entries.argtypes = [vp, ctypes.POINTER(TarEntry), sz, vp, sz]
        L.xlz_tar_close.argtypes = [vp]
        L.xlz_tar_close.restype = None
        L.xlz_ctx_last_tar_stats.argtypes = [vp, ctypes.POINTER(TarStats)]
        L.xlz_internal_tar_classify_device.argtypes = [vp, vp, ctypes.c_uint64, vp, ctypes.POINTER(ctypes.c_double)]
    if hasattr(L, "xlz_inflate_host"):  # (an older library loaded through XLZ_SO inflates nothing)
        L.xlz_inflate_host.argtypes = [vp, sz, vp, sz, ctypes.POINTER(sz), ctypes.POINTER(sz)]
        L.xlz_inflate_batch.argtypes = [vp, ctypes.POINTER(InflateItem), sz, vp, sz, ctypes.POINTER(InflateResult)]
        L.xlz_ctx_set_deflate_mode.argtypes = [vp, i32]
        L.xlz_ctx_deflate_mode.argtypes = [vp]
        L.xlz_ctx_last_inflate_stats.argtypes = [vp, ctypes.POINTER(InflateStats)]
    if hasattr(L, "xlz_zip_open"):  # (an older library loaded through XLZ_SO reads no .zip archives)
        L.xlz_zip_open.argtypes = [vp, sz, ctypes.POINTER(vp)]
        L.xlz_zip_close.argtypes = [vp]
        L.xlz_zip_close.restype = None
        L.xlz_zip_archive_info.argtypes = [vp, ctypes.POINTER(sz), ctypes.POINTER(sz), ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]
        L.xlz_zip_archive_entries.argtypes = [vp, ctypes.POINTER(ZipEntry), sz, vp, sz]
        L.xlz_zip_extract_layout.argtypes = [vp, ctypes.POINTER(ZipWant), sz, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64)]
        L.xlz_zip_extract.argtypes = [vp, vp, ctypes.POINTER(ZipWant), sz, vp, sz, i32, ctypes.POINTER(ZipFileResult)]
        L.xlz_zip_extract_device.argtypes = L.xlz_zip_extract.argtypes
        L.xlz_ctx_last_zip_extract_stats.argtypes = [vp, ctypes.POINTER(ZipExtractStats)]
    if hasattr(L, "xlz_gz_probe"):  # (an older library loaded through XLZ_SO reads no gzip)
        L.xlz_adler32_device.argtypes = [vp, vp, sz, ctypes.POINTER(AdlerRange), sz, ctypes.POINTER(ctypes.c_uint32)]
        L.xlz_adler32_host.restype = ctypes.c_uint32
        L.xlz_adler32_host.argtypes = [ctypes.c_uint32, vp, sz]
        L.xlz_adler32_combine.restype = ctypes.c_uint32
        L.xlz_adler32_combine.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint64]
        L.xlz_gz_probe.argtypes = [vp, sz, ctypes.c_uint32, ctypes.POINTER(GzInfo)]
        L.xlz_gz_decode_host.argtypes = [vp, sz, ctypes.c_uint32, vp, sz, i32, ctypes.POINTER(GzResult)]
        L.xlz_gz_decode_many_device.argtypes = [vp, ctypes.POINTER(GzFile), sz, vp, sz, i32, ctypes.POINTER(GzResult)]
        L.xlz_gz_decode_many.argtypes = L.xlz_gz_decode_many_device.argtypes
        L.xlz_ctx_last_gz_stats.argtypes = [vp, ctypes.POINTER(GzStats)]
    if hasattr(L, "xlz_bz2_probe"):  # (an older library loaded through XLZ_SO reads no .bz2)
        L.xlz_bz2_probe.argtypes = [vp, sz, ctypes.POINTER(Bz2Info)]
        L.xlz_bz2_decode_host.argtypes = [vp, sz, vp, sz, i32, ctypes.POINTER(Bz2Result)]
        L.xlz_bz2_decode_many_device.argtypes = [vp, ctypes.POINTER(Bz2File), sz, vp, sz, i32, ctypes.POINTER(Bz2Result)]
        L.xlz_bz2_decode_many.argtypes = L.xlz_bz2_decode_many_device.argtypes
        L.xlz_ctx_last_bz2_stats.argtypes = [vp, ctypes.POINTER(Bz2Stats)]
        L.xlz_ctx_set_bz2_mode.argtypes = [vp, i32]
        L.xlz_ctx_bz2_mode.argtypes = [vp]
        L.xlz_ctx_set_bz2_scratch.argtypes = [vp, ctypes.c_uint64]
        L.xlz_crc32_bzip2_host.restype = ctypes.c_uint32
        L.xlz_crc32_bzip2_host.argtypes = [ctypes.c_uint32, vp, sz]
    _lib = L
    return L


def strerror(status):
    return lib().xlz_strerror(status).decode()


def library_info():
    """which binary is loaded: path, SHA-256 of the file, the source hash compiled into it and the hash of the
    sources in the tree now (equal unless the library is stale or was swapped with XLZ_SO)"""
    import hashlib
    from . import build
    with open(SO_PATH, "rb") as f:
        sha = hashlib.sha256(f.read()).hexdigest()
    bid = lib().xlz_build_id().decode()
    tree = build.source_id()
    return {"path": os.path.relpath(SO_PATH, os.path.dirname(_HERE)) if SO_PATH.startswith(os.path.dirname(_HERE)) else SO_PATH,
            "sha256": sha, "build_id": bid, "kernel_id": lib().xlz_kernel_id().decode(), "tree_source_id": tree,
            "built_from_tree": bid == tree,
            "xlz_so_override": SO_PATH != DEFAULT_SO}
