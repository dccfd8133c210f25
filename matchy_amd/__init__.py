"""matchy_amd — MI355X-native `matchy match` engine (host mirror over the C ABI in include/matchy_amd.h).

The classes mirror the reference's operator interface for this path:
  DatabaseBuilder  ~ matchy::DatabaseBuilder   (crates/matchy-format/src/mmdb_builder.rs)
  Database         ~ matchy::Database          (crates/matchy/src/database.rs)         — lookups run on the GPU
  Extractor        ~ matchy::extractor::Extractor (crates/matchy-extractor/src/lib.rs) — extraction runs on the GPU
  Scanner          ~ processing::Worker        (crates/matchy/src/processing/mod.rs:318-448), the bulk scan entry

There is no CPU fallback anywhere in this package: if libmatchy_amd.so is missing the import of the native
layer raises, and without a HIP device Database()/Extractor() raise RuntimeError.
"""
import ctypes as C
import os
import json
from pathlib import Path

from . import build as _build

__all__ = ["DatabaseBuilder", "Database", "Extractor", "Scanner", "lib", "ITEM_TYPE_NAMES", "EXTRACT_ALL", "last_error"]

PKG = Path(__file__).resolve().parent
LIB_PATH = PKG / "lib" / "libmatchy_amd.so"

ITEM_TYPE_NAMES = ["Domain", "Email", "IPv4", "IPv6", "MD5", "SHA1", "SHA256", "SHA384", "SHA512", "Bitcoin", "Ethereum", "Monero"]
EXTRACT_DOMAINS, EXTRACT_EMAILS, EXTRACT_IPV4, EXTRACT_IPV6 = 1, 2, 4, 8
EXTRACT_HASHES, EXTRACT_BITCOIN, EXTRACT_ETHEREUM, EXTRACT_MONERO = 16, 32, 64, 128
EXTRACT_ALL = 255
EXTRACT_FORMATS = {"json": 0, "csv": 1, "text": 2}   # MATCHY_AMD_EXTRACT_FORMAT_*

# every symbol include/matchy_amd.h declares
EXPORTED_SYMBOLS = [
    "matchy_builder_new", "matchy_builder_set_case_insensitive", "matchy_builder_add", "matchy_builder_set_description",
    "matchy_builder_save", "matchy_builder_build", "matchy_builder_free", "matchy_init_open_options",
    "matchy_open_with_options", "matchy_open", "matchy_open_buffer", "matchy_close", "matchy_query", "matchy_query_into",
    "matchy_free_result", "matchy_free_string", "matchy_result_to_json", "matchy_version", "matchy_format",
    "matchy_has_ip_data", "matchy_has_string_data", "matchy_has_literal_data", "matchy_has_glob_data", "matchy_metadata",
    "matchy_get_pattern_string", "matchy_pattern_count", "matchy_extractor_create", "matchy_extractor_extract_chunk",
    "matchy_matches_free", "matchy_extractor_free", "matchy_item_type_name", "matchy_scanner_create", "matchy_scanner_free",
    "matchy_scanner_scan", "matchy_scanner_scan_device", "matchy_scan_result_free", "matchy_scan_hit_to_json",
    "matchy_scanner_set_profile", "matchy_scanner_get_timing", "matchy_amd_last_error", "matchy_builder_set_build_epoch",
    "matchy_get_stats", "matchy_clear_cache", "matchy_has_pattern_data", "matchy_result_get_entry", "matchy_aget_value",
    "matchy_get_entry_data_list", "matchy_free_entry_data_list", "matchy_validate", "matchy_builder_set_schema",
    "matchy_amd_query_json", "matchy_amd_extractor_create", "matchy_amd_device_count", "matchy_scanner_submit_device",
    "matchy_scanner_wait", "matchy_scanner_set_slices", "matchy_scanner_last_slices", "matchy_scan_result_on_device",
    "matchy_amd_ac_dfa_states", "matchy_amd_suffix_filter", "matchy_amd_pinned_alloc", "matchy_amd_pinned_free",
    "matchy_amd_host_register", "matchy_amd_host_unregister",
    "matchy_amd_device_numa_node", "matchy_amd_bind_thread_to_device", "matchy_amd_numa_cpus",
    "matchy_multi_scanner_create", "matchy_multi_scanner_free", "matchy_multi_scanner_workers", "matchy_multi_scanner_worker_scanner",
    "matchy_multi_scanner_set_batch_hook", "matchy_multi_scanner_submit", "matchy_multi_scanner_next", "matchy_multi_scanner_scan",
    "matchy_multi_scanner_pending", "matchy_multi_scanner_max_pending", "matchy_multi_scanner_submit_near", "matchy_multi_scanner_worker_numa",
    "matchy_amd_unbind_thread",
    "matchy_multi_scanner_scan_file", "matchy_scan_result_to_ndjson",
    "matchy_scanner_set_line_context", "matchy_scanner_line_context", "matchy_scan_result_lines", "matchy_multi_scanner_set_line_context",
    "matchy_scan_result_to_ndjson_lines", "matchy_scanner_get_line_timing",
    "matchy_amd_extractor_set_unique", "matchy_amd_extractor_unique", "matchy_amd_extractor_reset_unique", "matchy_amd_extractor_unique_count",
    "matchy_amd_extractor_extract_rendered", "matchy_amd_extractor_get_render_timing", "matchy_amd_extractor_render_allocations",
    "matchy_scanner_set_tally", "matchy_scanner_tally", "matchy_scanner_reset_tally", "matchy_scanner_tally_top",
    "matchy_multi_scanner_set_tally", "matchy_multi_scanner_tally_top", "matchy_multi_scanner_reset_tally", "matchy_tally_free",
    "matchy_scanner_set_segments", "matchy_scan_result_segments", "matchy_scan_result_to_ndjson_segments",
    "matchy_multi_scanner_submit_segments", "matchy_scanner_get_segment_timing",
    "matchy_scanner_scan_gz", "matchy_scan_result_gz", "matchy_scanner_get_gz_timing", "matchy_multi_scanner_submit_gz",
    "matchy_scanner_scan_gz_files", "matchy_scan_result_gz_files", "matchy_multi_scanner_submit_gz_files",
    "matchy_scanner_scan_gz_window", "matchy_scan_result_gz_window", "matchy_multi_scanner_submit_gz_window", "matchy_scanner_get_gz_window_timing",
    "matchy_scanner_set_gz_pieces", "matchy_scanner_get_gz_pieces", "matchy_scan_result_gz_pieces", "matchy_scanner_get_gz_pieces_timing",
    "matchy_multi_scanner_set_gz_pieces",
    "matchy_scanner_scan_gz_stream", "matchy_scan_result_gz_stream", "matchy_scanner_get_gz_stream_timing", "matchy_multi_scanner_submit_gz_stream",
    "matchy_scanner_set_hit_lines", "matchy_scanner_hit_lines", "matchy_scan_result_hit_lines", "matchy_scanner_get_hit_lines_timing",
    "matchy_multi_scanner_set_hit_lines",
    "matchy_scanner_set_render", "matchy_scan_result_ndjson", "matchy_scanner_get_render_timing", "matchy_scanner_get_render_counters",
    "matchy_multi_scanner_set_render",
    "matchy_scanner_set_whole_lines", "matchy_scanner_whole_lines", "matchy_scanner_get_whole_lines_counters",
    "matchy_scanner_get_whole_lines_timing", "matchy_multi_scanner_set_whole_lines",
    "matchy_scanner_scan_utf16", "matchy_scan_result_utf16", "matchy_scanner_get_utf16_timing", "matchy_amd_utf16_geometry",
    "matchy_multi_scanner_submit_utf16",
    "matchy_scanner_scan_escaped", "matchy_scan_result_unescaped", "matchy_scanner_get_unescape_timing", "matchy_amd_unescape_geometry",
    "matchy_multi_scanner_submit_escaped",
]

UTF16_LE, UTF16_BE = 0, 1   # MATCHY_UTF16_*: the byte order of a UTF-16 scan (Scanner.scan_utf16)
UNESCAPE_PERCENT, UNESCAPE_JSON = 1, 2   # MATCHY_UNESCAPE_*: the grammars of an escaped scan (Scanner.scan_escaped); both: percent(json(x))

# MATCHY_GZ_*: the status of one member of a gz scan (ScanResult.gz_status)
GZ_OK, GZ_BAD_HEADER, GZ_TRUNCATED, GZ_BAD_BLOCK, GZ_BAD_CODES, GZ_BAD_SYMBOL, GZ_BAD_DISTANCE = 0, 1, 2, 3, 4, 5, 6
GZ_OVERFLOW, GZ_SIZE_MISMATCH, GZ_CRC_MISMATCH, GZ_TRAILING_DATA = 7, 8, 9, 10
GZ_STATUS_NAMES = ["OK", "BAD_HEADER", "TRUNCATED", "BAD_BLOCK", "BAD_CODES", "BAD_SYMBOL", "BAD_DISTANCE", "OVERFLOW", "SIZE_MISMATCH",
                   "CRC_MISMATCH", "TRAILING_DATA"]

# bytes per tile of the '\n' count array and tiles per workgroup of its prefix sum (csrc/line_index.h): the sizes at which the line
# kernels take another path
LINE_TILE = 1024
LINE_SCAN_CHUNK = 2048
# bytes of the block of hit lines one wave of the copy kernel owns, and entries per workgroup of its prefix sums (csrc/hit_lines.h)
HIT_LINES_SLICE = 4096
HIT_LINES_SCAN_CHUNK = 2048


RENDER_LINE_NUMBERS, RENDER_INPUT_LINE = 1, 2   # matchy_render_params_t.flags
RENDER_OK, RENDER_TOO_LARGE = 0, 1


class RenderTooLarge(RuntimeError):
    """ScanResult.rendered_ndjson: the pass ended with MATCHY_RENDER_TOO_LARGE"""


class _Result(C.Structure):
    _fields_ = [("found", C.c_bool), ("prefix_len", C.c_uint8), ("_data_cache", C.c_void_p), ("_db_ref", C.c_void_p)]


class _Stats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("total_queries", "queries_with_match", "queries_without_match", "cache_hits",
                                          "cache_misses", "ip_queries", "string_queries")]


class _Entry(C.Structure):
    _fields_ = [("db", C.c_void_p), ("data_ptr", C.c_void_p)]


class _EntryValue(C.Union):
    _fields_ = [("pointer", C.c_uint32), ("utf8_string", C.c_char_p), ("double_value", C.c_double), ("bytes", C.POINTER(C.c_uint8)),
                ("uint16", C.c_uint16), ("uint32", C.c_uint32), ("int32", C.c_int32), ("uint64", C.c_uint64),
                ("uint128", C.c_uint8 * 16), ("boolean", C.c_bool), ("float_value", C.c_float)]


class _EntryData(C.Structure):
    _fields_ = [("has_data", C.c_bool), ("type_", C.c_uint32), ("value", _EntryValue), ("data_size", C.c_uint32), ("offset", C.c_uint32)]


class _EntryDataList(C.Structure):
    pass


_EntryDataList._fields_ = [("entry_data", _EntryData), ("next", C.POINTER(_EntryDataList))]


class _Match(C.Structure):
    _fields_ = [("item_type", C.c_uint8), ("value", C.c_char_p), ("start", C.c_size_t), ("end", C.c_size_t)]


class _Matches(C.Structure):
    _fields_ = [("items", C.POINTER(_Match)), ("count", C.c_size_t), ("_internal", C.c_void_p)]


class _ExtractText(C.Structure):
    # matchy_amd_extract_text_t
    _fields_ = [("text", C.c_void_p), ("text_len", C.c_uint64), ("n_records", C.c_uint64), ("by_type", C.c_uint64 * 12),
                ("status", C.c_uint32), ("reserved", C.c_uint32)]


class _ScanHit(C.Structure):
    # matchy_scan_hit_t (16 bytes): length in bits 0..23 of len_type, item type in bits 24..31
    _fields_ = [("start", C.c_uint32), ("len_type", C.c_uint32), ("value", C.c_uint32), ("kind", C.c_uint8),
                ("prefix_len", C.c_uint8), ("n_ids", C.c_uint16)]


class _ScanResult(C.Structure):
    _fields_ = [("hits", C.POINTER(_ScanHit)), ("n_hits", C.c_size_t), ("pattern_ids", C.POINTER(C.c_uint32)),
                ("data_offsets", C.POINTER(C.c_int64)), ("n_ids", C.c_size_t), ("lines", C.c_uint64),
                ("candidates", C.c_uint64), ("bytes", C.c_uint64), ("ip4_hits", C.POINTER(C.c_uint32 * 2)),
                ("n_ip4_hits", C.c_size_t), ("_internal", C.c_void_p)]


class _ScanHitLines(C.Structure):
    # matchy_scan_hit_lines_t
    _fields_ = [("text", C.c_void_p), ("text_len", C.c_uint64), ("n_lines", C.c_uint32), ("line_off", C.c_void_p), ("line_no", C.c_void_p),
                ("line_of_hit", C.c_void_p), ("line_of_ip4_hit", C.c_void_p)]


class _RenderParams(C.Structure):
    # matchy_render_params_t
    _fields_ = [("flags", C.c_uint32), ("source", C.c_char_p), ("sources", C.POINTER(C.c_char_p)), ("n_sources", C.c_size_t),
                ("line_base", C.c_uint64), ("line_bases", C.POINTER(C.c_uint64))]


class _ScanLine(C.Structure):
    # matchy_scan_line_t (16 bytes)
    _fields_ = [("line", C.c_uint32), ("line_start", C.c_uint32), ("line_end", C.c_uint32), ("reserved", C.c_uint32)]


class _ScanSegment(C.Structure):
    # matchy_scan_segment_t (32 bytes)
    _fields_ = [("start", C.c_uint32), ("len", C.c_uint32), ("hits", C.c_uint32), ("line_base", C.c_uint32), ("lines", C.c_uint32),
                ("lines_with_matches", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class _GzMember(C.Structure):
    # matchy_gz_member_t (16 bytes)
    _fields_ = [("offset", C.c_uint64), ("len", C.c_uint32), ("out_len", C.c_uint32)]


# MATCHY_WINDOW_*: the flag and the statuses of a gz window (Scanner.scan_gz_window, ScanResult.gz_window)
WINDOW_LAST = 1
WINDOW_OK, WINDOW_NO_LINE_END = 0, 1
GZ_WINDOW_TAIL_BLOCK = 4096   # csrc/inflate.h GZ_TAIL_BLOCK: the bytes k_gz_window_tail looks at per turn of its walk


class _GzWindow(C.Structure):
    # matchy_gz_window_t (24 bytes)
    _fields_ = [("carry", C.c_void_p), ("carry_len", C.c_uint32), ("carry_cap", C.c_uint32), ("flags", C.c_uint32)]


# MATCHY_STREAM_*: the flags and the statuses of a stream window (Scanner.scan_gz_stream, ScanResult.gz_stream)
STREAM_FIRST, STREAM_FILE_END = 1, 2
STREAM_OK, STREAM_NO_LINE_END, STREAM_NO_PROGRESS, STREAM_FAILED = 0, 1, 2, 3
GZ_STREAM_PASSES = ("find", "count", "chain", "symbols", "windows", "resolve", "verdict", "tail")


class GzStreamState(C.Structure):
    """matchy_gz_stream_state_t: what the windows in front of a stream window produced — the text's length, its CRC-32, the bit of the
    next window's first byte at which its first block starts, and the text's last history_len <= 32768 bytes"""
    _fields_ = [("text_bytes", C.c_uint64), ("crc", C.c_uint32), ("bit", C.c_uint32), ("history_len", C.c_uint32), ("history", C.c_uint8 * 32768)]

    def history_bytes(self):
        return bytes(self.history[:self.history_len])


class _GzStreamWindow(C.Structure):
    # matchy_gz_stream_window_t (32 bytes)
    _fields_ = [("state", C.POINTER(GzStreamState)), ("carry", C.c_void_p), ("carry_len", C.c_uint32), ("carry_cap", C.c_uint32), ("text_cap", C.c_uint32),
                ("flags", C.c_uint32)]


class GzStreamWalker:
    """csrc/gz_stream.h GzStreamWalker, line by line: where the next window of a chain of stream windows starts, how many compressed
    bytes it gets, and when the chain is over. next() -> (offset, length, bit, flags); accept(window, consumed_bits, text_len, ended)
    behind an OK window, refuse() behind any other."""
    MIN_PIECES = 4

    def __init__(self, file_len, window_bytes, piece_bytes, text_cap, first_bytes=0):
        self.file_len, self.window_bytes, self.piece_bytes, self.text_cap = file_len, window_bytes, piece_bytes, text_cap
        self.at = self.text_bytes = self.bit = self.windows = 0
        self.want = first_bytes or window_bytes
        self.over, self.ended = file_len == 0, False

    def _clamp(self, n):
        return max(min(self.MIN_PIECES * self.piece_bytes, self.window_bytes), min(n, self.window_bytes))

    def next(self):
        left, w = self.file_len - self.at, self._clamp(self.want)
        flags = STREAM_FIRST if self.windows == 0 else 0
        if left <= w + w // 4:
            return self.at, left, self.bit, flags | STREAM_FILE_END
        return self.at, w, self.bit, flags

    def accept(self, window, consumed_bits, text_len, ended):
        offset, length, bit, _ = window
        self.windows += 1
        if consumed_bits <= bit or consumed_bits > length * 8:
            self.over = True
            return False
        nbytes = consumed_bits // 8
        self.at, self.bit = offset + nbytes, consumed_bits % 8
        self.text_bytes += text_len
        fill = (max(nbytes, 1) * self.text_cap + text_len - 1) // text_len if text_len else self.window_bytes
        self.want = self._clamp(fill + fill // 8 + self.piece_bytes)
        if ended:
            self.over = self.ended = True
        return True

    def refuse(self):
        self.windows += 1
        self.over = True


class _GzPiece(C.Structure):
    # matchy_gz_piece_t (32 bytes)
    _fields_ = [("start_bit", C.c_uint64), ("end_bit", C.c_uint64), ("member", C.c_uint32), ("produced", C.c_uint32), ("out_pos", C.c_uint32),
                ("flags", C.c_uint32)]


# MATCHY_PIECE_*: flags of a piece (ScanResult.gz_pieces)
GZ_PIECE_HAS_START, GZ_PIECE_LIVE, GZ_PIECE_HANDED_OVER = 1, 2, 4


class _GzFile(C.Structure):
    # matchy_gz_file_t (16 bytes)
    _fields_ = [("offset", C.c_uint64), ("len", C.c_uint64)]


class _TallyEntry(C.Structure):
    # matchy_tally_entry_t
    _fields_ = [("text", C.POINTER(C.c_uint8)), ("len", C.c_uint32), ("item_type", C.c_uint8), ("count", C.c_uint64)]


class _Tally(C.Structure):
    _fields_ = [("entries", C.POINTER(_TallyEntry)), ("n_entries", C.c_size_t), ("distinct", C.c_uint64), ("matches", C.c_uint64),
                ("_internal", C.c_void_p)]


_lib = None


class _MultiBatch(C.Structure):
    _fields_ = [("seq", C.c_size_t), ("status", C.c_int32), ("result", _ScanResult), ("data", C.c_void_p), ("len", C.c_size_t),
                ("tag", C.c_void_p), ("payload", C.c_void_p), ("worker", C.c_size_t)]


class _MultiTotals(C.Structure):
    _fields_ = [("batches", C.c_uint64), ("bytes", C.c_uint64), ("lines", C.c_uint64), ("candidates", C.c_uint64), ("matches", C.c_uint64)]


_MULTI_ORDERED_FN = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.POINTER(_MultiBatch))


def lib():
    """Load libmatchy_amd.so (built in-tree by matchy_amd.build). Raises if it is missing — no fallback."""
    global _lib
    if _lib is not None:
        return _lib
    # MATCHY_AMD_LIB: another build of the same library (kernel A/B experiments: tools/ab.sh); never a fallback
    path = Path(os.environ["MATCHY_AMD_LIB"]) if os.environ.get("MATCHY_AMD_LIB") else LIB_PATH
    if not path.exists():
        raise ImportError(f"{path} is missing: run `python -m matchy_amd.build` (hipcc, gfx950) first")
    L = C.CDLL(str(path))
    vp, cp, u8p = C.c_void_p, C.c_char_p, C.POINTER(C.c_uint8)
    sig = {
        "matchy_builder_new": (vp, []),
        "matchy_builder_set_case_insensitive": (C.c_int32, [vp, C.c_bool]),
        "matchy_builder_add": (C.c_int32, [vp, cp, cp]),
        "matchy_builder_set_description": (C.c_int32, [vp, cp]),
        "matchy_builder_save": (C.c_int32, [vp, cp]),
        "matchy_builder_build": (C.c_int32, [vp, C.POINTER(vp), C.POINTER(C.c_size_t)]),
        "matchy_builder_free": (None, [vp]),
        "matchy_builder_set_build_epoch": (C.c_int32, [vp, C.c_uint64]),
        "matchy_open": (vp, [cp]),
        "matchy_open_with_options": (vp, [cp, vp]),
        "matchy_open_buffer": (vp, [cp, C.c_size_t]),
        "matchy_close": (None, [vp]),
        "matchy_query": (_Result, [vp, cp]),
        "matchy_query_into": (None, [vp, cp, C.POINTER(_Result)]),
        "matchy_free_result": (None, [C.POINTER(_Result)]),
        "matchy_free_string": (None, [vp]),
        "matchy_result_to_json": (vp, [C.POINTER(_Result)]),
        "matchy_version": (cp, []),
        "matchy_format": (cp, [vp]),
        "matchy_has_ip_data": (C.c_bool, [vp]),
        "matchy_has_string_data": (C.c_bool, [vp]),
        "matchy_has_literal_data": (C.c_bool, [vp]),
        "matchy_has_glob_data": (C.c_bool, [vp]),
        "matchy_metadata": (vp, [vp]),
        "matchy_get_pattern_string": (vp, [vp, C.c_uint32]),
        "matchy_pattern_count": (C.c_size_t, [vp]),
        "matchy_extractor_create": (vp, [C.c_uint32]),
        "matchy_amd_extractor_create": (vp, [C.c_uint32, C.c_uint32]),
        "matchy_extractor_extract_chunk": (C.c_int32, [vp, cp, C.c_size_t, C.POINTER(_Matches)]),
        "matchy_matches_free": (None, [C.POINTER(_Matches)]),
        "matchy_extractor_free": (None, [vp]),
        "matchy_amd_extractor_set_unique": (None, [vp, C.c_bool]),
        "matchy_amd_extractor_unique": (C.c_bool, [vp]),
        "matchy_amd_extractor_reset_unique": (None, [vp]),
        "matchy_amd_extractor_unique_count": (C.c_uint64, [vp]),
        "matchy_amd_extractor_extract_rendered": (C.c_int32, [vp, cp, C.c_size_t, C.c_uint32, C.POINTER(_ExtractText)]),
        "matchy_amd_extractor_get_render_timing": (None, [vp, C.POINTER(C.c_float)]),
        "matchy_amd_extractor_render_allocations": (C.c_uint64, [vp]),
        "matchy_item_type_name": (cp, [C.c_uint8]),
        "matchy_scanner_create": (vp, [vp, C.c_uint32, C.c_int32]),
        "matchy_scanner_free": (None, [vp]),
        "matchy_scanner_scan": (C.c_int32, [vp, vp, C.c_size_t, C.POINTER(_ScanResult)]),
        "matchy_scanner_scan_device": (C.c_int32, [vp, vp, C.c_size_t, vp, C.c_uint32, C.POINTER(_ScanResult)]),
        "matchy_scanner_submit_device": (C.c_int32, [vp, vp, C.c_size_t, vp, C.c_uint32]),
        "matchy_scanner_wait": (C.c_int32, [vp, C.POINTER(_ScanResult)]),
        "matchy_scan_result_free": (None, [C.POINTER(_ScanResult)]),
        "matchy_scan_hit_to_json": (vp, [vp, C.POINTER(_ScanResult), C.c_size_t, cp, cp]),
        "matchy_scan_result_to_ndjson": (C.c_int32, [vp, C.POINTER(_ScanResult), cp, cp, C.POINTER(vp), C.POINTER(C.c_size_t)]),
        "matchy_scanner_set_profile": (None, [vp, C.c_bool]),
        "matchy_amd_ac_dfa_states": (C.c_int32, [vp]),
        "matchy_amd_suffix_filter": (C.c_int32, [vp]),
        "matchy_amd_pinned_alloc": (vp, [C.c_size_t]),
        "matchy_amd_pinned_free": (None, [vp]),
        "matchy_amd_host_register": (C.c_int32, [vp, C.c_size_t]),
        "matchy_amd_host_unregister": (None, [vp]),
        "matchy_scanner_set_slices": (None, [vp, C.c_int32]),
        "matchy_scanner_last_slices": (C.c_int32, [vp]),
        "matchy_scan_result_on_device": (C.c_bool, [C.POINTER(_ScanResult)]),
        "matchy_scanner_get_timing": (None, [vp, C.POINTER(C.c_float)]),
        "matchy_amd_last_error": (cp, []),
        "matchy_get_stats": (None, [vp, C.POINTER(_Stats)]),
        "matchy_clear_cache": (None, [vp]),
        "matchy_has_pattern_data": (C.c_bool, [vp]),
        "matchy_result_get_entry": (C.c_int32, [C.POINTER(_Result), C.POINTER(_Entry)]),
        "matchy_aget_value": (C.c_int32, [C.POINTER(_Entry), C.POINTER(_EntryData), C.POINTER(cp)]),
        "matchy_get_entry_data_list": (C.c_int32, [C.POINTER(_Entry), C.POINTER(C.POINTER(_EntryDataList))]),
        "matchy_free_entry_data_list": (None, [C.POINTER(_EntryDataList)]),
        "matchy_validate": (C.c_int32, [cp, C.c_int32, C.POINTER(vp)]),
        "matchy_builder_set_schema": (C.c_int32, [vp, cp]),
        "matchy_amd_device_count": (C.c_int32, []),
        "matchy_amd_device_numa_node": (C.c_int32, [C.c_int32]),
        "matchy_amd_bind_thread_to_device": (C.c_int32, [C.c_int32]),
        "matchy_amd_numa_cpus": (C.c_int32, [cp, cp, C.POINTER(C.c_int32), C.c_size_t]),
        "matchy_multi_scanner_create": (vp, [vp, C.c_uint32, C.POINTER(C.c_int32), C.c_size_t]),
        "matchy_multi_scanner_free": (None, [vp]),
        "matchy_multi_scanner_workers": (C.c_size_t, [vp]),
        "matchy_multi_scanner_worker_scanner": (vp, [vp, C.c_size_t]),
        "matchy_multi_scanner_submit": (C.c_int32, [vp, vp, C.c_size_t, vp, vp]),
        "matchy_multi_scanner_next": (C.c_int32, [vp, C.POINTER(_MultiBatch)]),
        "matchy_multi_scanner_submit_near": (C.c_int32, [vp, vp, C.c_size_t, vp, vp, C.c_int32]),
        "matchy_multi_scanner_worker_numa": (C.c_int32, [vp, C.c_size_t, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
        "matchy_multi_scanner_pending": (C.c_size_t, [vp]),
        "matchy_multi_scanner_max_pending": (C.c_size_t, [vp]),
        "matchy_amd_unbind_thread": (C.c_int32, []),
        "matchy_multi_scanner_scan": (C.c_int32, [vp, vp, C.c_size_t, C.c_size_t, C.POINTER(_ScanResult)]),
        "matchy_multi_scanner_scan_file": (C.c_int32, [vp, cp, C.c_size_t, _MULTI_ORDERED_FN, vp, C.POINTER(_MultiTotals)]),
        "matchy_scanner_set_line_context": (None, [vp, C.c_bool]),
        "matchy_scanner_line_context": (C.c_bool, [vp]),
        "matchy_scan_result_lines": (C.c_int32, [C.POINTER(_ScanResult), C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_uint64)]),
        "matchy_multi_scanner_set_line_context": (None, [vp, C.c_bool]),
        "matchy_scan_result_to_ndjson_lines": (C.c_int32, [vp, C.POINTER(_ScanResult), cp, cp, C.c_uint64, C.c_bool, C.POINTER(vp), C.POINTER(C.c_size_t)]),
        "matchy_scanner_get_line_timing": (None, [vp, C.POINTER(C.c_float)]),
        "matchy_scanner_set_hit_lines": (None, [vp, C.c_bool]),
        "matchy_scanner_hit_lines": (C.c_bool, [vp]),
        "matchy_scan_result_hit_lines": (C.c_int32, [C.POINTER(_ScanResult), C.POINTER(_ScanHitLines)]),
        "matchy_scanner_get_hit_lines_timing": (None, [vp, C.POINTER(C.c_float)]),
        "matchy_multi_scanner_set_hit_lines": (None, [vp, C.c_bool]),
        "matchy_scanner_set_render": (C.c_int32, [vp, C.POINTER(_RenderParams)]),
        "matchy_scan_result_ndjson": (C.c_int32, [C.POINTER(_ScanResult), C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), C.POINTER(C.c_int32)]),
        "matchy_scanner_get_render_timing": (None, [vp, C.POINTER(C.c_float)]),
        "matchy_scanner_get_render_counters": (None, [vp, C.POINTER(C.c_uint64)]),
        "matchy_multi_scanner_set_render": (C.c_int32, [vp, C.POINTER(_RenderParams)]),
        "matchy_scanner_set_segments": (C.c_int32, [vp, C.POINTER(C.c_uint32), C.c_size_t]),
        "matchy_scan_result_segments": (C.c_int32, [C.POINTER(_ScanResult), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_size_t)]),
        "matchy_scan_result_to_ndjson_segments": (C.c_int32, [vp, C.POINTER(_ScanResult), cp, C.POINTER(cp), C.POINTER(C.c_uint64), C.c_bool,
                                                              C.POINTER(vp), C.POINTER(C.c_size_t)]),
        "matchy_multi_scanner_submit_segments": (C.c_int32, [vp, vp, C.c_size_t, C.POINTER(C.c_uint32), C.c_size_t, vp, vp]),
        "matchy_scanner_get_segment_timing": (None, [vp, C.POINTER(C.c_float)]),
        "matchy_scanner_scan_gz": (C.c_int32, [vp, vp, C.c_size_t, C.POINTER(_GzMember), C.c_size_t, C.c_uint32, C.c_bool, C.POINTER(_ScanResult)]),
        "matchy_scan_result_gz": (C.c_int32, [C.POINTER(_ScanResult), C.POINTER(vp), C.POINTER(C.c_size_t), C.POINTER(vp), C.POINTER(C.c_size_t)]),
        "matchy_scanner_get_gz_timing": (None, [vp, C.POINTER(C.c_float)]),
        "matchy_scanner_scan_utf16": (C.c_int32, [vp, vp, C.c_size_t, C.c_uint32, C.c_uint32, C.c_bool, C.POINTER(_ScanResult)]),
        "matchy_scan_result_utf16": (C.c_int32, [C.POINTER(_ScanResult), C.POINTER(vp), C.POINTER(C.c_size_t), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
        "matchy_scanner_get_utf16_timing": (None, [vp, C.POINTER(C.c_float)]),
        "matchy_amd_utf16_geometry": (None, [C.POINTER(C.c_uint32)]),
        "matchy_multi_scanner_submit_utf16": (C.c_int32, [vp, vp, C.c_size_t, C.c_uint32, C.c_bool, vp, vp]),
        "matchy_scanner_scan_escaped": (C.c_int32, [vp, vp, C.c_size_t, C.c_uint32, C.c_uint32, C.c_bool, C.POINTER(_ScanResult)]),
        "matchy_scan_result_unescaped": (C.c_int32, [C.POINTER(_ScanResult), C.POINTER(vp), C.POINTER(C.c_size_t), C.POINTER(C.c_uint64)]),
        "matchy_scanner_get_unescape_timing": (None, [vp, C.POINTER(C.c_float)]),
        "matchy_amd_unescape_geometry": (None, [C.POINTER(C.c_uint32)]),
        "matchy_multi_scanner_submit_escaped": (C.c_int32, [vp, vp, C.c_size_t, C.c_uint32, C.c_bool, vp, vp]),
        "matchy_multi_scanner_submit_gz": (C.c_int32, [vp, vp, C.c_size_t, C.POINTER(_GzMember), C.c_size_t, C.c_bool, vp]),
        "matchy_scanner_scan_gz_files": (C.c_int32, [vp, vp, C.c_size_t, C.POINTER(_GzFile), C.c_size_t, C.c_uint32, C.c_bool, C.POINTER(_ScanResult)]),
        "matchy_scan_result_gz_files": (C.c_int32, [C.POINTER(_ScanResult), C.POINTER(vp), C.POINTER(C.c_size_t), C.POINTER(vp)]),
        "matchy_multi_scanner_submit_gz_files": (C.c_int32, [vp, vp, C.c_size_t, C.POINTER(_GzFile), C.c_size_t, C.c_bool, vp]),
        "matchy_scanner_scan_gz_window": (C.c_int32, [vp, vp, C.c_size_t, C.POINTER(_GzWindow), C.c_uint32, C.c_bool, C.POINTER(_ScanResult)]),
        "matchy_scan_result_gz_window": (C.c_int32, [C.POINTER(_ScanResult), C.POINTER(C.c_int32), C.POINTER(vp), C.POINTER(C.c_size_t)]),
        "matchy_multi_scanner_submit_gz_window": (C.c_int32, [vp, vp, C.c_size_t, C.POINTER(_GzWindow), C.c_bool, vp]),
        "matchy_scanner_get_gz_window_timing": (None, [vp, C.POINTER(C.c_float)]),
        "matchy_scanner_scan_gz_stream": (C.c_int32, [vp, vp, C.c_size_t, C.POINTER(_GzStreamWindow), C.c_uint32, C.c_bool, C.POINTER(_ScanResult)]),
        "matchy_scan_result_gz_stream": (C.c_int32, [C.POINTER(_ScanResult), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32),
                                                     C.POINTER(C.c_bool), C.POINTER(C.POINTER(GzStreamState)), C.POINTER(vp), C.POINTER(C.c_size_t)]),
        "matchy_scanner_get_gz_stream_timing": (None, [vp, C.POINTER(C.c_float)]),
        "matchy_multi_scanner_submit_gz_stream": (C.c_int32, [vp, vp, C.c_size_t, C.POINTER(_GzStreamWindow), C.c_bool, vp]),
        "matchy_scanner_set_gz_pieces": (C.c_int32, [vp, C.c_uint32]),
        "matchy_scanner_get_gz_pieces": (C.c_uint32, [vp]),
        "matchy_scan_result_gz_pieces": (C.c_int32, [C.POINTER(_ScanResult), C.POINTER(C.POINTER(_GzPiece)), C.POINTER(C.c_size_t), C.POINTER(vp)]),
        "matchy_scanner_get_gz_pieces_timing": (None, [vp, C.POINTER(C.c_float)]),
        "matchy_multi_scanner_set_gz_pieces": (C.c_int32, [vp, C.c_uint32]),
        "matchy_scanner_set_whole_lines": (None, [vp, C.c_bool]),
        "matchy_scanner_whole_lines": (C.c_bool, [vp]),
        "matchy_scanner_get_whole_lines_counters": (None, [vp, C.POINTER(C.c_uint64)]),
        "matchy_scanner_get_whole_lines_timing": (None, [vp, C.POINTER(C.c_float)]),
        "matchy_multi_scanner_set_whole_lines": (C.c_int32, [vp, C.c_bool]),
        "matchy_scanner_set_tally": (None, [vp, C.c_bool]),
        "matchy_scanner_tally": (C.c_bool, [vp]),
        "matchy_scanner_reset_tally": (None, [vp]),
        "matchy_scanner_tally_top": (C.c_int32, [vp, C.c_size_t, C.POINTER(_Tally)]),
        "matchy_multi_scanner_set_tally": (C.c_int32, [vp, C.c_bool]),
        "matchy_multi_scanner_tally_top": (C.c_int32, [vp, C.c_size_t, C.POINTER(_Tally)]),
        "matchy_multi_scanner_reset_tally": (None, [vp]),
        "matchy_tally_free": (None, [C.POINTER(_Tally)]),
    }
    for name, (res, args) in sig.items():
        f = getattr(L, name)
        f.restype = res
        f.argtypes = args
    _lib = L
    return L


def last_error() -> str:
    return lib().matchy_amd_last_error().decode("utf-8", "replace")


def _take_string(ptr) -> str:
    if not ptr:
        return None
    s = C.string_at(ptr).decode("utf-8", "replace")
    lib().matchy_free_string(ptr)
    return s


class DatabaseBuilder:
    """Mirror of the reference builder behind matchy_builder_* (host-side, no GPU needed)."""

    def __init__(self, build_epoch=None, case_insensitive=False):
        self._h = lib().matchy_builder_new()
        if build_epoch is not None:
            lib().matchy_builder_set_build_epoch(self._h, build_epoch)
        if case_insensitive:
            lib().matchy_builder_set_case_insensitive(self._h, True)

    def add_entry(self, key: str, data: dict):
        rc = lib().matchy_builder_add(self._h, key.encode("utf-8"), json.dumps(data).encode("utf-8"))
        if rc != 0:
            raise ValueError(f"matchy_builder_add({key!r}) failed: rc={rc} {last_error()}")

    def set_description(self, text: str):
        lib().matchy_builder_set_description(self._h, text.encode("utf-8"))

    def build(self) -> bytes:
        buf = C.c_void_p()
        size = C.c_size_t()
        rc = lib().matchy_builder_build(self._h, C.byref(buf), C.byref(size))
        if rc != 0:
            raise ValueError(f"matchy_builder_build failed: rc={rc} {last_error()}")
        try:
            return C.string_at(buf, size.value)
        finally:
            C.CDLL(None).free(buf)

    def save(self, path: str):
        rc = lib().matchy_builder_save(self._h, str(path).encode())
        if rc != 0:
            raise OSError(f"matchy_builder_save failed: rc={rc} {last_error()}")

    def close(self):
        if self._h:
            lib().matchy_builder_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Database:
    """An opened .mxy database, uploaded once to device memory (matchy_open / matchy_open_buffer)."""

    def __init__(self, source):
        L = lib()
        if isinstance(source, (bytes, bytearray, memoryview)):
            b = bytes(source)
            self._h = L.matchy_open_buffer(b, len(b))
        else:
            self._h = L.matchy_open(str(source).encode())
        if not self._h:
            raise RuntimeError("matchy_open failed: " + last_error())

    def close(self):
        if self._h:
            lib().matchy_close(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    def lookup(self, query: str):
        """Database::lookup → None | {'found': True, 'prefix_len': n, 'data': {...}} (matchy_query semantics)."""
        L = lib()
        r = L.matchy_query(self._h, query.encode("utf-8") if isinstance(query, str) else bytes(query))
        try:
            if not r.found:
                return None
            js = _take_string(L.matchy_result_to_json(C.byref(r)))
            return {"found": True, "prefix_len": r.prefix_len, "data": json.loads(js) if js else None}
        finally:
            L.matchy_free_result(C.byref(r))

    def query_json(self, query: str):
        """what `matchy query DB QUERY` prints (matchy_amd_query_json): (found, list) — one object per pattern that carries data
        (literal first, then globs by id), or one object for an IP hit with "cidr" and "prefix_len" added; [] when nothing matches"""
        L = lib()
        found = C.c_int32(0)
        L.matchy_amd_query_json.restype = C.c_void_p
        L.matchy_amd_query_json.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_int32)]
        p = L.matchy_amd_query_json(self._h, query.encode("utf-8") if isinstance(query, str) else bytes(query), C.byref(found))
        if not p:
            raise RuntimeError("matchy_amd_query_json failed: " + last_error())
        return bool(found.value), json.loads(_take_string(p))

    @staticmethod
    def _entry_value(ed):
        """matchy_entry_data_t -> (type, python value); maps / arrays yield their element count."""
        t = ed.type_
        v = ed.value
        if t == 2:
            return t, C.string_at(v.utf8_string, ed.data_size).decode("utf-8")
        if t == 4:
            return t, bytes(v.bytes[i] for i in range(ed.data_size))
        return t, {1: v.pointer, 3: v.double_value, 5: v.uint16, 6: v.uint32, 7: ed.data_size, 8: v.int32, 9: v.uint64,
                   10: int.from_bytes(bytes(v.uint128), "big"), 11: ed.data_size, 14: bool(v.boolean), 15: v.float_value}[t]

    def get_value(self, query: str, *path):
        """matchy_query + matchy_result_get_entry + matchy_aget_value -> (rc, type, value)."""
        L = lib()
        r = L.matchy_query(self._h, query.encode("utf-8"))
        try:
            e = _Entry()
            rc = L.matchy_result_get_entry(C.byref(r), C.byref(e))
            if rc != 0:
                return rc, None, None
            arr = (C.c_char_p * (len(path) + 1))(*[str(x).encode("utf-8") for x in path], None)
            ed = _EntryData()
            rc = L.matchy_aget_value(C.byref(e), C.byref(ed), arr)
            if rc != 0 or not ed.has_data:
                return rc, None, None
            t, v = self._entry_value(ed)
            return rc, t, v
        finally:
            L.matchy_free_result(C.byref(r))

    def entry_data_list(self, query: str):
        """matchy_get_entry_data_list flattened to [(type, value)], or None when the query has no result."""
        L = lib()
        r = L.matchy_query(self._h, query.encode("utf-8"))
        try:
            e = _Entry()
            if L.matchy_result_get_entry(C.byref(r), C.byref(e)) != 0:
                return None
            head = C.POINTER(_EntryDataList)()
            if L.matchy_get_entry_data_list(C.byref(e), C.byref(head)) != 0:
                return None
            out, node = [], head
            while node:
                out.append(self._entry_value(node.contents.entry_data))
                node = node.contents.next
            L.matchy_free_entry_data_list(head)
            return out
        finally:
            L.matchy_free_result(C.byref(r))

    def stats(self):
        st = _Stats()
        lib().matchy_get_stats(self._h, C.byref(st))
        return {n: getattr(st, n) for n, _ in _Stats._fields_}

    def has_ip_data(self):
        return bool(lib().matchy_has_ip_data(self._h))

    def has_literal_data(self):
        return bool(lib().matchy_has_literal_data(self._h))

    def has_glob_data(self):
        return bool(lib().matchy_has_glob_data(self._h))

    def format(self):
        return lib().matchy_format(self._h).decode()

    def metadata(self):
        return json.loads(_take_string(lib().matchy_metadata(self._h)))

    def pattern_count(self):
        return lib().matchy_pattern_count(self._h)

    def pattern_string(self, pid):
        return _take_string(lib().matchy_get_pattern_string(self._h, pid))


class Extractor:
    """Extractor::extract_from_chunk on the GPU (matchy_extractor_*). Returns (type_name, start, end, value).

    unique: only the first occurrence of every candidate text (the raw bytes data[start:end]) since creation or reset_unique() is
    returned; the set of texts lives on the GPU, across calls (matchy_amd_extractor_set_unique)."""

    def __init__(self, flags=EXTRACT_ALL, min_domain_labels=2, unique=False):
        # min_domain_labels: ExtractorBuilder::min_domain_labels (matchy-extractor/src/lib.rs:101-104), through the additive entry
        self._h = (lib().matchy_extractor_create(flags) if min_domain_labels == 2
                   else lib().matchy_amd_extractor_create(flags, min_domain_labels))
        if not self._h:
            raise RuntimeError("matchy_extractor_create failed: " + last_error())
        if unique:
            self.set_unique(True)

    def set_unique(self, on=True):
        lib().matchy_amd_extractor_set_unique(self._h, bool(on))

    @property
    def unique(self):
        return bool(lib().matchy_amd_extractor_unique(self._h))

    def reset_unique(self):
        lib().matchy_amd_extractor_reset_unique(self._h)

    @property
    def unique_count(self):
        return int(lib().matchy_amd_extractor_unique_count(self._h))

    def extract_from_chunk(self, data: bytes):
        L = lib()
        m = _Matches()
        rc = L.matchy_extractor_extract_chunk(self._h, bytes(data), len(data), C.byref(m))
        if rc != 0:
            raise RuntimeError(f"matchy_extractor_extract_chunk failed: rc={rc} {last_error()}")
        try:
            return [(ITEM_TYPE_NAMES[m.items[i].item_type], m.items[i].start, m.items[i].end, m.items[i].value.decode("utf-8"))
                    for i in range(m.count)]
        finally:
            L.matchy_matches_free(C.byref(m))

    def extract_rendered(self, data: bytes, fmt="json"):
        """The output of `matchy extract` for the candidates of `data`, ordered and written on the GPU (matchy_amd_extractor_extract_rendered):
        (text, counts) with counts a dict item type name -> records. fmt: "json", "csv" (without the header line) or "text"."""
        L = lib()
        out = _ExtractText()
        rc = L.matchy_amd_extractor_extract_rendered(self._h, bytes(data), len(data), EXTRACT_FORMATS[fmt] if isinstance(fmt, str) else fmt, C.byref(out))
        if rc != 0:
            raise RuntimeError(f"matchy_amd_extractor_extract_rendered failed: rc={rc} {last_error()}")
        if out.status != 0:
            raise RuntimeError(f"matchy_amd_extractor_extract_rendered: status {out.status}")
        text = C.string_at(out.text, out.text_len) if out.text_len else b""
        counts = {ITEM_TYPE_NAMES[t]: int(out.by_type[t]) for t in range(12) if out.by_type[t]}
        assert sum(counts.values()) == out.n_records
        return text, counts

    def render_timing(self):
        """device milliseconds of keys + sort, measure, write and the block's copy of the last extract_rendered"""
        ms = (C.c_float * 4)()
        lib().matchy_amd_extractor_get_render_timing(self._h, ms)
        return tuple(ms)

    @property
    def render_allocations(self):
        return int(lib().matchy_amd_extractor_render_allocations(self._h))

    def close(self):
        if self._h:
            lib().matchy_extractor_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ScanResult:
    def __init__(self, scanner, raw):
        self._scanner = scanner
        self._raw = raw
        self.lines = raw.lines
        self.candidates = raw.candidates
        self.bytes = raw.bytes
        self.n_ip4_hits = raw.n_ip4_hits   # fetch_mode 1 | 8: IPv4 results as compact records (not in _raw.hits)
        self.n_hits = raw.n_hits + raw.n_ip4_hits
        self._on_device = None

    @property
    def on_device(self):
        """fetch_mode 4: the arrays of the result are device pointers"""
        if self._on_device is None:
            self._on_device = bool(lib().matchy_scan_result_on_device(C.byref(self._raw))) if self._raw is not None else False
        return self._on_device

    def hits(self):
        """list of dict(start,end,type,kind,prefix_len,ip_data_offset,ids,offs) in canonical order."""
        r = self._raw
        out = []
        if self.on_device:
            raise RuntimeError("the hit records of this result are in device memory (fetch_mode 4): read them on the GPU")
        for i in range(r.n_ip4_hits if r.ip4_hits else 0):   # matchy_scan_ip4_hit_expand
            start, packed = r.ip4_hits[i]
            out.append(dict(start=start, end=start + ((packed >> 22) & 15) + 7, type=ITEM_TYPE_NAMES[2], kind="ip", prefix_len=packed >> 26,
                            ip_data_offset=packed & 0x3FFFFF, ids=[], offs=[]))
        if not r.hits:
            return out
        for i in range(r.n_hits):
            h = r.hits[i]
            ids = [r.pattern_ids[h.value + k] for k in range(h.n_ids)] if h.kind == 3 else []
            offs = [r.data_offsets[h.value + k] for k in range(h.n_ids)] if h.kind == 3 else []
            out.append(dict(start=h.start, end=h.start + (h.len_type & 0xFFFFFF), type=ITEM_TYPE_NAMES[h.len_type >> 24],
                            kind="ip" if h.kind == 2 else "pattern", prefix_len=h.prefix_len,
                            ip_data_offset=h.value if h.kind == 2 else 0, ids=ids, offs=offs))
        return out

    def _segment_arrays(self):
        """(segment_of_hit pointer, segment_of_ip4_hit pointer, table pointer, n_segments) of a segmented scan, else None"""
        if self._raw is None:
            raise RuntimeError("the result is closed")
        a, b, t, n = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_size_t()
        if lib().matchy_scan_result_segments(C.byref(self._raw), C.byref(a), C.byref(b), C.byref(t), C.byref(n)) != 0:
            return None
        return a.value or 0, b.value or 0, t.value or 0, int(n.value)

    @property
    def has_segments(self):
        return self._segment_arrays() is not None

    @property
    def segments(self):
        """[dict(start, len, hits, line_base, lines, lines_with_matches)] per segment (host memory for every fetch mode); None for a
        scan without segments"""
        sa = self._segment_arrays()
        if sa is None:
            return None
        arr = C.cast(sa[2], C.POINTER(_ScanSegment))
        return [dict(start=arr[i].start, len=arr[i].len, hits=arr[i].hits, line_base=arr[i].line_base, lines=arr[i].lines,
                     lines_with_matches=arr[i].lines_with_matches) for i in range(sa[3])]

    def _segment_list(self, ptr, n):
        if n and self.on_device:
            raise RuntimeError("the segment indices of this result are in device memory (fetch_mode 4): read them on the GPU (segment_of_ptr)")
        if not ptr or not n:
            return []
        arr = C.cast(ptr, C.POINTER(C.c_uint32))
        return [arr[i] for i in range(n)]

    @property
    def segment_of_ptr(self):
        """address of the uint32 array parallel to the hit records (a device address when on_device), 0 when there is none"""
        sa = self._segment_arrays()
        return None if sa is None else sa[0]

    @property
    def segment_of(self):
        """segment index per 16-byte hit record (hits() lists them behind the compact ones); None for a scan without segments"""
        sa = self._segment_arrays()
        return None if sa is None else self._segment_list(sa[0], self._raw.n_hits if self._raw.hits else 0)

    @property
    def segment_of_ip4(self):
        """segment index per compact IPv4 record"""
        sa = self._segment_arrays()
        return None if sa is None else self._segment_list(sa[1], self._raw.n_ip4_hits if self._raw.ip4_hits else 0)

    def ndjson_segments_text(self, text: bytes, sources, line_bases=None, with_input_line=False) -> bytes:
        """ndjson_text with sources[segment] as the source of every record; line_bases (one per segment) adds "line_number" counted
        inside the segment (matchy_scan_result_to_ndjson_segments)"""
        L = lib()
        out, n = C.c_void_p(), C.c_size_t()
        src = (C.c_char_p * len(sources))(*[x.encode() if isinstance(x, str) else x for x in sources])
        lb = None if line_bases is None else (C.c_uint64 * len(line_bases))(*line_bases)
        rc = L.matchy_scan_result_to_ndjson_segments(self._scanner._h, C.byref(self._raw), text, src, lb, with_input_line, C.byref(out), C.byref(n))
        if rc != 0:
            raise RuntimeError(f"matchy_scan_result_to_ndjson_segments failed ({rc}): " + last_error())
        try:
            return C.string_at(out.value, n.value)
        finally:
            L.matchy_free_string(out)

    def _gz_arrays(self):
        """(status pointer, n_members, text pointer, text_len) of a gz scan, else None"""
        if self._raw is None:
            raise RuntimeError("the result is closed")
        st, n, t, tn = C.c_void_p(), C.c_size_t(), C.c_void_p(), C.c_size_t()
        if lib().matchy_scan_result_gz(C.byref(self._raw), C.byref(st), C.byref(n), C.byref(t), C.byref(tn)) != 0:
            return None
        return st.value or 0, int(n.value), t.value or 0, int(tn.value)

    def gz_status(self):
        """one GZ_* status per member of a gz scan (Scanner.scan_gz); None for any other scan"""
        ga = self._gz_arrays()
        if ga is None:
            return None
        arr = C.cast(ga[0], C.POINTER(C.c_int32))
        return [arr[i] for i in range(ga[1])]

    def gz_text(self):
        """the inflated batch of a gz scan with want_text as bytes (a copy); None without want_text or for any other scan"""
        ga = self._gz_arrays()
        if ga is None or not ga[2]:
            return None
        return C.string_at(ga[2], ga[3])

    def gz_text_len(self):
        """length of the inflated batch of a gz scan, with or without want_text; None for any other scan"""
        ga = self._gz_arrays()
        return None if ga is None else ga[3]

    def utf16(self):
        """what a UTF-16 scan (Scanner.scan_utf16; matchy_scan_result_utf16) says about its batch, as a dict: text (the UTF-8 batch as
        bytes, a copy; None without want_text), text_len, code_units and replaced (U+FFFD written); None for any other scan"""
        if self._raw is None:
            raise RuntimeError("the result is closed")
        t, n, units, repl = C.c_void_p(), C.c_size_t(), C.c_uint64(), C.c_uint64()
        if lib().matchy_scan_result_utf16(C.byref(self._raw), C.byref(t), C.byref(n), C.byref(units), C.byref(repl)) != 0:
            return None
        return dict(text=C.string_at(t.value, n.value) if t.value else None, text_len=int(n.value), code_units=int(units.value), replaced=int(repl.value))

    def unescaped(self):
        """what an escaped scan (Scanner.scan_escaped; matchy_scan_result_unescaped) says about its batch, as a dict: text (the decoded
        batch as bytes, a copy; None without want_text), text_len, escapes (valid escapes decoded), replaced (U+FFFD written) and
        lf_escapes (escapes for LF written as a space); None for any other scan"""
        if self._raw is None:
            raise RuntimeError("the result is closed")
        t, n, ctr = C.c_void_p(), C.c_size_t(), (C.c_uint64 * 3)()
        if lib().matchy_scan_result_unescaped(C.byref(self._raw), C.byref(t), C.byref(n), ctr) != 0:
            return None
        return dict(text=C.string_at(t.value, n.value) if t.value else None, text_len=int(n.value), escapes=int(ctr[0]), replaced=int(ctr[1]),
                    lf_escapes=int(ctr[2]))

    def gz_window(self):
        """(WINDOW_* status, carry bytes) of a gz scan of a window (Scanner.scan_gz_window): the carry is the partial line behind the
        window's last newline, to be handed to the next window; None for any other scan"""
        if self._raw is None:
            raise RuntimeError("the result is closed")
        st, p, n = C.c_int32(0), C.c_void_p(), C.c_size_t(0)
        if lib().matchy_scan_result_gz_window(C.byref(self._raw), C.byref(st), C.byref(p), C.byref(n)) != 0:
            return None
        return st.value, (C.string_at(p.value, n.value) if n.value else b"")

    def gz_stream(self):
        """the verdict of a gz scan of a stream window (Scanner.scan_gz_stream) as a dict: status (STREAM_*), gz_status (GZ_*),
        consumed_bits (from bit 0 of the window's first byte, the gzip header of the first window included), text_len, ended, state (a
        GzStreamState of its own for the next window; None unless the status is STREAM_OK) and carry (bytes); None for any other scan"""
        if self._raw is None:
            raise RuntimeError("the result is closed")
        st, gst, bits, tl, ended = C.c_int32(0), C.c_int32(0), C.c_uint64(0), C.c_uint32(0), C.c_bool(False)
        state, p, n = C.POINTER(GzStreamState)(), C.c_void_p(), C.c_size_t(0)
        if lib().matchy_scan_result_gz_stream(C.byref(self._raw), C.byref(st), C.byref(gst), C.byref(bits), C.byref(tl), C.byref(ended), C.byref(state), C.byref(p),
                                              C.byref(n)) != 0:
            return None
        own = None
        if state:
            own = GzStreamState()
            C.memmove(C.byref(own), state, C.sizeof(GzStreamState))
        return dict(status=st.value, gz_status=gst.value, consumed_bits=bits.value, text_len=tl.value, ended=bool(ended.value), state=own,
                    carry=C.string_at(p.value, n.value) if n.value else b"")

    def _gz_file_arrays(self):
        """(file status pointer, n_files, first_member pointer) of a gz scan of files, else None"""
        if self._raw is None:
            raise RuntimeError("the result is closed")
        st, n, fm = C.c_void_p(), C.c_size_t(), C.c_void_p()
        if lib().matchy_scan_result_gz_files(C.byref(self._raw), C.byref(st), C.byref(n), C.byref(fm)) != 0:
            return None
        return st.value or 0, int(n.value), fm.value or 0

    def gz_file_status(self):
        """one GZ_* verdict per file of a gz scan of files (Scanner.scan_gz_files): OK, or the status of the file's first member in
        stream order that is not; None for any other scan"""
        ga = self._gz_file_arrays()
        if ga is None:
            return None
        arr = C.cast(ga[0], C.POINTER(C.c_int32))
        return [arr[i] for i in range(ga[1])]

    def gz_first_member(self):
        """n_files + 1 indices into gz_status(): the members of file f are [first[f], first[f + 1]); None for any other scan"""
        ga = self._gz_file_arrays()
        if ga is None:
            return None
        arr = C.cast(ga[2], C.POINTER(C.c_uint32))
        return [arr[i] for i in range(ga[1] + 1)]

    def gz_pieces(self):
        """(pieces, first_piece) of a gz scan with pieces on (Scanner.set_gz_pieces; matchy_scan_result_gz_pieces): pieces is a list of
        tuples (start_bit, end_bit, member, produced, out_pos, flags), the pieces of member i are pieces[first_piece[i]:first_piece[i + 1]].
        ([], None) with pieces off; None for any other scan"""
        ga = self._gz_arrays()
        if ga is None:
            return None
        p, n, fp = C.POINTER(_GzPiece)(), C.c_size_t(), C.c_void_p()
        if lib().matchy_scan_result_gz_pieces(C.byref(self._raw), C.byref(p), C.byref(n), C.byref(fp)) != 0:
            return None
        pieces = [(p[i].start_bit, p[i].end_bit, p[i].member, p[i].produced, p[i].out_pos, p[i].flags) for i in range(n.value)]
        if not fp.value:
            return pieces, None
        arr = C.cast(fp, C.POINTER(C.c_uint32))
        return pieces, [arr[i] for i in range(ga[1] + 1)]

    def hit_lines(self):
        """the block of the distinct lines with a hit (Scanner.set_hit_lines; matchy_scan_result_hit_lines) as a dict: text (bytes),
        text_len, n_lines and the uint32 numpy arrays line_off (n_lines + 1), line_no, line_of_hit, line_of_ip4_hit (None where the
        result has none: a counts-only fetch). For a device result (fetch_mode 4) text and the arrays are raw device addresses (0 =
        none). None for a result scanned with the setting off."""
        if self._raw is None:
            raise RuntimeError("the result is closed")
        h = _ScanHitLines()
        if lib().matchy_scan_result_hit_lines(C.byref(self._raw), C.byref(h)) != 0:
            return None
        n_hits = self._raw.n_hits if self._raw.hits else 0
        n_ip4 = self._raw.n_ip4_hits if self._raw.ip4_hits else 0
        out = dict(text_len=int(h.text_len), n_lines=int(h.n_lines), on_device=self.on_device)
        if self.on_device:
            out.update(text=h.text or 0, line_off=h.line_off or 0, line_no=h.line_no or 0, line_of_hit=h.line_of_hit or 0, line_of_ip4_hit=h.line_of_ip4_hit or 0)
            return out
        import numpy as np

        def arr(ptr, n):
            if not ptr:
                return None
            return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint32)), shape=(n,)).copy() if n else np.zeros(0, np.uint32)
        gathered = bool(h.line_off)   # false: a counts-only fetch, which carries n_lines alone
        out.update(text=C.string_at(h.text, h.text_len) if h.text else (b"" if gathered else None),
                   line_off=arr(h.line_off, h.n_lines + 1), line_no=arr(h.line_no, h.n_lines),
                   line_of_hit=arr(h.line_of_hit, n_hits), line_of_ip4_hit=arr(h.line_of_ip4_hit, n_ip4))
        return out

    def rendered_ndjson(self):
        """the NDJSON block of a result whose scan was armed with Scanner.set_render (matchy_scan_result_ndjson): bytes, or for a
        device result (fetch_mode 4) the tuple (device address, length). Raises RenderTooLarge when the pass ended with
        MATCHY_RENDER_TOO_LARGE and ValueError for a result whose scan was not armed."""
        if self._raw is None:
            raise RuntimeError("the result is closed")
        text, n, status = C.c_void_p(), C.c_uint64(), C.c_int32()
        if lib().matchy_scan_result_ndjson(C.byref(self._raw), C.byref(text), C.byref(n), C.byref(status)) != 0:
            raise ValueError("matchy_scan_result_ndjson failed: " + last_error())
        if status.value != RENDER_OK:
            raise RenderTooLarge("the rendered records exceed a limit of the renderer (MATCHY_RENDER_TOO_LARGE)")
        if self.on_device:
            return (text.value or 0, int(n.value))
        return C.string_at(text.value, n.value) if text.value else b""

    def _line_arrays(self):
        """(lines pointer, ip4_lines pointer, lines_with_matches) of a result scanned with line context, else None"""
        if self._raw is None:
            raise RuntimeError("the result is closed")
        a, b, n = C.c_void_p(), C.c_void_p(), C.c_uint64()
        if lib().matchy_scan_result_lines(C.byref(self._raw), C.byref(a), C.byref(b), C.byref(n)) != 0:
            return None
        return a.value or 0, b.value or 0, int(n.value)

    @property
    def has_lines(self):
        return self._line_arrays() is not None

    @property
    def lines_with_matches(self):
        """distinct lines with at least one hit (line context); None for a result scanned without it"""
        la = self._line_arrays()
        return None if la is None else la[2]

    @property
    def lines_ptr(self):
        """address of the matchy_scan_line_t array parallel to the hit records (a device address when on_device), 0 when there is none"""
        la = self._line_arrays()
        return 0 if la is None else la[0]

    @property
    def ip4_lines_ptr(self):
        la = self._line_arrays()
        return 0 if la is None else la[1]

    def _line_list(self, ptr, n):
        if self.on_device:
            raise RuntimeError("the line records of this result are in device memory (fetch_mode 4): read them on the GPU (lines_ptr)")
        if not ptr or not n:
            return []
        arr = C.cast(ptr, C.POINTER(_ScanLine))
        return [(arr[i].line, arr[i].line_start, arr[i].line_end) for i in range(n)]

    @property
    def line_records(self):
        """[(line, line_start, line_end)] parallel to the 16-byte hit records (hits() lists them behind the compact ones); None without
        line context. (`lines` is taken: it is the '\\n' count of the scan.)"""
        la = self._line_arrays()
        return None if la is None else self._line_list(la[0], self._raw.n_hits if self._raw.hits else 0)

    @property
    def ip4_lines(self):
        """[(line, line_start, line_end)] parallel to the compact IPv4 records"""
        la = self._line_arrays()
        return None if la is None else self._line_list(la[1], self._raw.n_ip4_hits if self._raw.ip4_hits else 0)

    def ndjson_lines_text(self, text: bytes, source="-", line_base=0, with_input_line=False) -> bytes:
        """ndjson_text with "line_number" (and "input_line") in every record (matchy_scan_result_to_ndjson_lines)"""
        L = lib()
        out, n = C.c_void_p(), C.c_size_t()
        rc = L.matchy_scan_result_to_ndjson_lines(self._scanner._h, C.byref(self._raw), text, source.encode(), line_base, with_input_line, C.byref(out), C.byref(n))
        if rc != 0:
            raise RuntimeError(f"matchy_scan_result_to_ndjson_lines failed ({rc}): " + last_error())
        try:
            return C.string_at(out.value, n.value)
        finally:
            L.matchy_free_string(out)

    def ndjson(self, text: bytes, source="-"):
        L = lib()
        if self.on_device:
            raise RuntimeError("the hit records of this result are in device memory (fetch_mode 4): read them on the GPU")
        n = (self._raw.n_hits if self._raw.hits else 0) + (self._raw.n_ip4_hits if self._raw.ip4_hits else 0)
        if not self._raw.hits and self._raw.n_hits:
            return []   # counters only
        return [_take_string(L.matchy_scan_hit_to_json(self._scanner._h, C.byref(self._raw), i, text, source.encode())) for i in range(n)]

    def ndjson_text(self, text: bytes, source="-") -> bytes:
        """all matches as one NDJSON text in one call (matchy_scan_result_to_ndjson: what `matchy match` prints)"""
        L = lib()
        out, n = C.c_void_p(), C.c_size_t()
        rc = L.matchy_scan_result_to_ndjson(self._scanner._h, C.byref(self._raw), text, source.encode(), C.byref(out), C.byref(n))
        if rc != 0:
            raise RuntimeError(f"matchy_scan_result_to_ndjson failed ({rc}): " + last_error())
        try:
            return C.string_at(out.value, n.value)
        finally:
            L.matchy_free_string(out)

    def close(self):
        if self._raw is not None:
            if self._raw._internal:   # borrowed results (fetch_mode 0 / 1 / 9) own nothing: no call needed
                lib().matchy_scan_result_free(C.byref(self._raw))
            self._raw = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _read_tally(fn, handle, limit, what):
    """[(text bytes, item type name, count)] in read-out order through matchy_*_tally_top; .distinct / .matches ride on the list"""
    t = _Tally()
    rc = fn(handle, int(limit), C.byref(t))
    if rc != 0:
        raise RuntimeError(f"{what} failed ({rc}): " + last_error())
    try:
        out = TallyList((C.string_at(t.entries[i].text, t.entries[i].len), ITEM_TYPE_NAMES[t.entries[i].item_type], int(t.entries[i].count))
                        for i in range(t.n_entries))
        out.distinct, out.matches = int(t.distinct), int(t.matches)
        return out
    finally:
        lib().matchy_tally_free(C.byref(t))


class TallyList(list):
    """what Scanner.tally() returns: a list of (bytes, item_type, count) with the totals of the whole table as attributes"""
    distinct = 0
    matches = 0


def _render_params(flags, source, sources, line_base, line_bases):
    """matchy_render_params_t of Scanner.set_render / MultiScanner.set_render (None: disarm); the arrays stay alive with the struct"""
    if flags is None:
        return None
    p = _RenderParams(flags=flags, line_base=line_base)
    if sources is not None:
        enc = [None if s is None else (s if isinstance(s, bytes) else s.encode()) for s in sources]
        p.sources = (C.c_char_p * max(len(enc), 1))(*enc)
        p.n_sources = len(enc)
        if line_bases is not None:
            p.line_bases = (C.c_uint64 * max(len(line_bases), 1))(*line_bases)
    elif source is not None:
        p.source = source if isinstance(source, bytes) else source.encode()
    return p


class Scanner:
    """Bulk scan session (the device-side Worker). One per thread / stream."""

    def __init__(self, db: Database, extract_flags=0, device=0, profile=False):
        self._db = db
        self._h = lib().matchy_scanner_create(db.handle, extract_flags, device)
        if not self._h:
            raise RuntimeError("matchy_scanner_create failed: " + last_error())
        if profile:
            lib().matchy_scanner_set_profile(self._h, True)

    def scan(self, data: bytes) -> ScanResult:
        raw = _ScanResult()
        rc = lib().matchy_scanner_scan(self._h, bytes(data), len(data), C.byref(raw))
        if rc != 0:
            raise RuntimeError(f"matchy_scanner_scan failed: rc={rc} {last_error()}")
        return ScanResult(self, raw)

    def scan_ptr(self, host_ptr: int, nbytes: int) -> ScanResult:
        """Like scan() for a host buffer given by address (e.g. numpy / torch CPU storage) — no Python-side copy."""
        raw = _ScanResult()
        rc = lib().matchy_scanner_scan(self._h, host_ptr, nbytes, C.byref(raw))
        if rc != 0:
            raise RuntimeError(f"matchy_scanner_scan failed: rc={rc} {last_error()}")
        return ScanResult(self, raw)

    def scan_device(self, device_ptr: int, nbytes: int, stream: int = 0, fetch_mode=1) -> ScanResult:
        """fetch_mode: 0 counters only, 1 hit records in device order (borrowed from the scanner's pinned buffers), 3 hit records
        in canonical order (owned copy), 1 | 8 like 1 with the IPv4 results as 8-byte records (n_ip4_hits; hits() / ndjson() read
        both arrays), 4 the records stay in device memory (result.on_device: `_raw.hits` / `pattern_ids` /
        `data_offsets` are device addresses; hits() raises)."""
        raw = _ScanResult()
        rc = lib().matchy_scanner_scan_device(self._h, device_ptr, nbytes, stream, fetch_mode, C.byref(raw))
        if rc != 0:
            raise RuntimeError(f"matchy_scanner_scan_device failed: rc={rc} {last_error()}")
        return ScanResult(self, raw)

    def submit_device(self, device_ptr: int, nbytes: int, stream: int = 0, fetch_mode=1):
        rc = lib().matchy_scanner_submit_device(self._h, device_ptr, nbytes, stream, fetch_mode)
        if rc != 0:
            raise RuntimeError(f"matchy_scanner_submit_device failed: rc={rc} {last_error()}")

    def wait(self) -> ScanResult:
        raw = _ScanResult()
        rc = lib().matchy_scanner_wait(self._h, C.byref(raw))
        if rc != 0:
            raise RuntimeError(f"matchy_scanner_wait failed: rc={rc} {last_error()}")
        return ScanResult(self, raw)

    def set_line_context(self, on: bool):
        """line context for the next scans: ScanResult.line_records / ip4_lines / lines_with_matches (off by default)"""
        lib().matchy_scanner_set_line_context(self._h, bool(on))

    def line_context(self) -> bool:
        return bool(lib().matchy_scanner_line_context(self._h))

    def set_hit_lines(self, on: bool):
        """hit lines for the next scans: ScanResult.hit_lines(), and the NDJSON calls render with text=None (off by default; turns
        line context on for those scans)"""
        lib().matchy_scanner_set_hit_lines(self._h, bool(on))

    def hit_lines_enabled(self) -> bool:
        return bool(lib().matchy_scanner_hit_lines(self._h))

    def set_whole_lines(self, on=True):
        """whole-line queries for the next lookup scans: every line of the buffer is one query, looked up like Database.query does a
        single value (off by default; not together with segments, gz scans, hit lines or rendered records)"""
        lib().matchy_scanner_set_whole_lines(self._h, bool(on))

    def whole_lines_enabled(self) -> bool:
        return bool(lib().matchy_scanner_whole_lines(self._h))

    def whole_lines_counters(self):
        """of the last scan in whole-line mode: queries, address queries, string queries, queries that are not valid UTF-8"""
        out = (C.c_uint64 * 4)()
        lib().matchy_scanner_get_whole_lines_counters(self._h, out)
        return dict(queries=int(out[0]), address=int(out[1]), string=int(out[2]), invalid_utf8=int(out[3]))

    def whole_lines_timing_ms(self):
        out = (C.c_float * 3)()
        lib().matchy_scanner_get_whole_lines_timing(self._h, out)
        return dict(count_prefix=out[0], scatter_classify=out[1], lookup=out[2])

    def set_render(self, flags=0, source=None, sources=None, line_base=0, line_bases=None):
        """arms the NEXT scan / scan_device / submit_device / scan_gz: its result answers rendered_ndjson() with the NDJSON text of its
        records, written on the GPU (matchy_scanner_set_render). flags: RENDER_LINE_NUMBERS / RENDER_INPUT_LINE (need line context).
        sources (one str per segment of a segmented scan, with line_bases) or source (one for the buffer, with line_base).
        flags=None disarms."""
        p = _render_params(flags, source, sources, line_base, line_bases)
        rc = lib().matchy_scanner_set_render(self._h, None if p is None else C.byref(p))
        if rc != 0:
            raise RuntimeError(f"matchy_scanner_set_render failed ({rc}): " + last_error())

    def render_timing_ms(self):
        out = (C.c_float * 3)()
        lib().matchy_scanner_get_render_timing(self._h, out)
        return dict(measure=out[0], write=out[1], d2h=out[2])

    def render_counters(self):
        """of the last scan that rendered: repeats of the pass, payload-table misses, payloads rendered by the host, bytes copied"""
        out = (C.c_uint64 * 6)()
        lib().matchy_scanner_get_render_counters(self._h, out)
        return dict(rounds=int(out[0]), misses=int(out[1]), payloads_added=int(out[2]), copied=int(out[3]), rehashes=int(out[4]), pool_regrows=int(out[5]))

    def hit_lines_timing_ms(self):
        out = (C.c_float * 3)()
        lib().matchy_scanner_get_hit_lines_timing(self._h, out)
        return dict(index=out[0], copy_kernel=out[1], d2h=out[2])

    def line_timing_ms(self):
        out = (C.c_float * 3)()
        lib().matchy_scanner_get_line_timing(self._h, out)
        return dict(count=out[0], prefix=out[1], resolve=out[2])

    def set_segments(self, starts):
        """the NEXT scan's buffer is len(starts) segments that begin at these offsets (matchy_scanner_set_segments): the result then
        has .segments / .segment_of / .segment_of_ip4. An empty list clears a pending table."""
        arr = (C.c_uint32 * len(starts))(*starts)
        rc = lib().matchy_scanner_set_segments(self._h, arr, len(starts))
        if rc != 0:
            raise RuntimeError(f"matchy_scanner_set_segments failed ({rc}): " + last_error())

    def segment_timing_ms(self):
        out = (C.c_float * 3)()
        lib().matchy_scanner_get_segment_timing(self._h, out)
        return dict(build=out[0], records=out[1], lines=out[2])

    def scan_gz(self, blobs, want_text=False, out_lens=None, fetch_mode=1) -> ScanResult:
        """inflate the gzip files `blobs` (bytes each) on the GPU and scan them as one batch of len(blobs) segments
        (matchy_scanner_scan_gz). out_lens: the inflated length of every file the caller vouches for (0 or None = take ISIZE). The
        result has .segments / .segment_of like a segmented scan, and gz_status() / gz_text()."""
        packed, table = _gz_pack(blobs, out_lens)
        raw = _ScanResult()
        rc = lib().matchy_scanner_scan_gz(self._h, packed, len(packed), table, len(table), fetch_mode, bool(want_text), C.byref(raw))
        if rc != 0:
            raise RuntimeError(f"matchy_scanner_scan_gz failed: rc={rc} {last_error()}")
        return ScanResult(self, raw)

    def scan_utf16(self, data, byte_order=UTF16_LE, want_text=False, fetch_mode=1, nbytes=None) -> ScanResult:
        """transcode the UTF-16 batch `data` to UTF-8 on the GPU and scan the text (matchy_scanner_scan_utf16). data: bytes, or an
        address (host or device memory) together with nbytes. The result's offsets are offsets into the UTF-8 text; utf16() has the
        text (with want_text), its length, the code units and the U+FFFD written. No BOM handling."""
        if isinstance(data, int):
            ptr, n = data, int(nbytes)
        else:
            data = bytes(data)
            ptr, n = C.cast(C.c_char_p(data), C.c_void_p), len(data)
        raw = _ScanResult()
        rc = lib().matchy_scanner_scan_utf16(self._h, ptr, n, byte_order, fetch_mode, bool(want_text), C.byref(raw))
        if rc != 0:
            raise RuntimeError(f"matchy_scanner_scan_utf16 failed: rc={rc} {last_error()}")
        return ScanResult(self, raw)

    def utf16_timing_ms(self):
        """(count, prefix, write) milliseconds of the last UTF-16 scan; zeros before the first"""
        out = (C.c_float * 3)()
        lib().matchy_scanner_get_utf16_timing(self._h, out)
        return tuple(out)

    def scan_escaped(self, data, modes=UNESCAPE_PERCENT, want_text=False, fetch_mode=1, nbytes=None) -> ScanResult:
        """decode the percent- and/or JSON-escaped batch `data` on the GPU and scan the text (matchy_scanner_scan_escaped). data: bytes,
        or an address (host or device memory) together with nbytes. modes: UNESCAPE_PERCENT, UNESCAPE_JSON or both (percent(json(x))).
        The result's offsets are offsets into the decoded text; unescaped() has the text (with want_text), its length and the
        counters. An escape for LF becomes a space: the text has the line ends of the input."""
        if isinstance(data, int):
            ptr, n = data, int(nbytes)
        else:
            data = bytes(data)
            ptr, n = C.cast(C.c_char_p(data), C.c_void_p), len(data)
        raw = _ScanResult()
        rc = lib().matchy_scanner_scan_escaped(self._h, ptr, n, modes, fetch_mode, bool(want_text), C.byref(raw))
        if rc != 0:
            raise RuntimeError(f"matchy_scanner_scan_escaped failed: rc={rc} {last_error()}")
        return ScanResult(self, raw)

    def unescape_timing_ms(self):
        """(count, prefix, write) milliseconds of the last escaped scan, summed over its runs; zeros before the first"""
        out = (C.c_float * 3)()
        lib().matchy_scanner_get_unescape_timing(self._h, out)
        return tuple(out)

    def scan_gz_files(self, blobs, want_text=False, fetch_mode=1) -> ScanResult:
        """inflate the gzip files `blobs` (bytes each, of one member or many) on the GPU, one wave per member, and scan them as one batch
        of len(blobs) segments (matchy_scanner_scan_gz_files). The result has .segments / .segment_of like a segmented scan,
        gz_file_status() / gz_first_member(), and gz_status() / gz_text() per member."""
        packed, table = _gz_pack_files(blobs)
        raw = _ScanResult()
        rc = lib().matchy_scanner_scan_gz_files(self._h, packed, len(packed), table, len(table), fetch_mode, bool(want_text), C.byref(raw))
        if rc != 0:
            raise RuntimeError(f"matchy_scanner_scan_gz_files failed: rc={rc} {last_error()}")
        return ScanResult(self, raw)

    def scan_gz_window(self, blob, carry=b"", carry_cap=1 << 20, last=False, want_text=False, fetch_mode=1) -> ScanResult:
        """inflate and scan one window of a multi-member gzip file that is larger than a batch (matchy_scanner_scan_gz_window): `blob` are
        the window's whole members, `carry` the partial line the window in front left behind. The result has gz_window() -> (status,
        carry for the next window), one segment, gz_file_status() (one file), and gz_status() / gz_text() (the carry included)."""
        keep = C.create_string_buffer(bytes(carry), len(carry)) if carry else None
        w = _GzWindow(C.addressof(keep) if keep is not None else None, len(carry), carry_cap, WINDOW_LAST if last else 0)
        raw = _ScanResult()
        rc = lib().matchy_scanner_scan_gz_window(self._h, bytes(blob), len(blob), C.byref(w), fetch_mode, bool(want_text), C.byref(raw))
        if rc != 0:
            raise RuntimeError(f"matchy_scanner_scan_gz_window failed: rc={rc} {last_error()}")
        return ScanResult(self, raw)

    def scan_gz_stream(self, blob, state=None, carry=b"", carry_cap=1 << 20, text_cap=1 << 20, first=False, file_end=False, want_text=False, fetch_mode=1) -> ScanResult:
        """inflate and scan one window of ONE DEFLATE stream that is larger than a batch (matchy_scanner_scan_gz_stream; set_gz_pieces
        comes first): `blob` are the window's compressed bytes — with `first` they begin with the gzip header —, `state` the GzStreamState
        the window in front handed out (None with `first`), `carry` its partial line, text_cap the most text the window may give. The
        result has gz_stream() (status, consumed_bits, text_len, ended, the next state and carry), one segment, gz_status() / gz_text()
        (the carry included) and gz_pieces(). GzStreamWalker decides where the next window starts."""
        keep = C.create_string_buffer(bytes(carry), len(carry)) if carry else None
        w = _GzStreamWindow(C.pointer(state) if state is not None else None, C.addressof(keep) if keep is not None else None, len(carry), carry_cap, text_cap,
                            (STREAM_FIRST if first else 0) | (STREAM_FILE_END if file_end else 0))
        raw = _ScanResult()
        rc = lib().matchy_scanner_scan_gz_stream(self._h, bytes(blob), len(blob), C.byref(w), fetch_mode, bool(want_text), C.byref(raw))
        if rc != 0:
            raise RuntimeError(f"matchy_scanner_scan_gz_stream failed: rc={rc} {last_error()}")
        return ScanResult(self, raw)

    def gz_stream_timing_ms(self):
        """with set_profile: milliseconds per pass of the last stream window (GZ_STREAM_PASSES)"""
        out = (C.c_float * len(GZ_STREAM_PASSES))()
        lib().matchy_scanner_get_gz_stream_timing(self._h, out)
        return dict(zip(GZ_STREAM_PASSES, out))

    def set_gz_pieces(self, piece_bytes=0):
        """pieces of one stream for the next gz scans (matchy_scanner_set_gz_pieces): every member of at least 2 * piece_bytes compressed
        bytes is inflated by one wave per piece. 0 = off (the default); otherwise a power of two from 512 to 1 MiB, else ValueError"""
        if lib().matchy_scanner_set_gz_pieces(self._h, piece_bytes) != 0:
            raise ValueError(f"matchy_scanner_set_gz_pieces failed: {last_error()}")

    def gz_pieces(self) -> int:
        return int(lib().matchy_scanner_get_gz_pieces(self._h))

    def gz_pieces_timing_ms(self):
        out = (C.c_float * 6)()
        lib().matchy_scanner_get_gz_pieces_timing(self._h, out)
        return dict(find=out[0], count=out[1], chain=out[2], symbols=out[3], resolve=out[4], handover=out[5])

    def gz_window_timing_ms(self):
        out = (C.c_float * 4)()
        lib().matchy_scanner_get_gz_window_timing(self._h, out)
        return dict(inflate=out[0], crc=out[1], seal=out[2], tail=out[3])

    def gz_timing_ms(self):
        out = (C.c_float * 3)()
        lib().matchy_scanner_get_gz_timing(self._h, out)
        return dict(inflate=out[0], crc=out[1], seal=out[2])

    def set_tally(self, on=True):
        """hit tally for the next scans: matches per distinct (item type, matched text), counted on the GPU across scans (off by default)"""
        lib().matchy_scanner_set_tally(self._h, bool(on))

    def tally_enabled(self) -> bool:
        return bool(lib().matchy_scanner_tally(self._h))

    def reset_tally(self):
        lib().matchy_scanner_reset_tally(self._h)

    def tally(self, limit=0):
        """the first `limit` entries (0 = all) as (bytes, item_type, count): count descending, extractor order of the type, text ascending"""
        return _read_tally(lib().matchy_scanner_tally_top, self._h, limit, "matchy_scanner_tally_top")

    def set_slices(self, n: int):
        """scan_device cuts large batches into slices (tail of one slice beside the streaming pass of the next): 0 = default, 1 = never, n = n equal slices."""
        lib().matchy_scanner_set_slices(self._h, n)

    def last_slices(self) -> int:
        return lib().matchy_scanner_last_slices(self._h)

    def timing_ms(self):
        out = (C.c_float * 5)()
        lib().matchy_scanner_get_timing(self._h, out)
        return dict(anchor=out[0], validate=out[1], rare=out[2], lookup=out[3], total=out[4])

    def close(self):
        if self._h:
            lib().matchy_scanner_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _gz_pack(blobs, out_lens=None):
    """the files end to end as one bytes object, and their matchy_gz_member_t table"""
    table = (_GzMember * len(blobs))()
    pos = 0
    for i, b in enumerate(blobs):
        table[i].offset, table[i].len = pos, len(b)
        table[i].out_len = int(out_lens[i]) if out_lens is not None and out_lens[i] else 0
        pos += len(b)
    return b"".join(bytes(b) for b in blobs), table


def _gz_pack_files(blobs):
    """the files end to end as one bytes object, and their matchy_gz_file_t table"""
    table = (_GzFile * len(blobs))()
    pos = 0
    for i, b in enumerate(blobs):
        table[i].offset, table[i].len = pos, len(b)
        pos += len(b)
    return b"".join(bytes(b) for b in blobs), table


class _WorkerScanner:
    """the scanner of one worker of a MultiScanner, as far as ScanResult needs it (matchy_scan_hit_to_json)"""

    def __init__(self, h):
        self._h = h


class MultiScanner:
    """One scan session over several devices (matchy_multi_scanner_*): the reader -> per-device workers -> ordered gather of the
    reference's process_files_parallel (processing/parallel.rs:494-505) behind the C ABI. `devices` may repeat an ordinal (several
    batches of one GPU in flight)."""

    def __init__(self, db: Database, devices=(0,), extract_flags=0):
        self._db = db
        arr = (C.c_int32 * len(devices))(*devices)
        self._h = lib().matchy_multi_scanner_create(db.handle, extract_flags, arr, len(devices))
        if not self._h:
            raise RuntimeError("matchy_multi_scanner_create failed: " + last_error())
        self.workers = lib().matchy_multi_scanner_workers(self._h)

    def scan(self, data: bytes, batch_bytes: int = 0) -> ScanResult:
        """one buffer through all workers; the merged result has offsets into `data` (= Scanner.scan of the same bytes)"""
        raw = _ScanResult()
        rc = lib().matchy_multi_scanner_scan(self._h, bytes(data), len(data), batch_bytes, C.byref(raw))
        if rc != 0:
            raise RuntimeError(f"matchy_multi_scanner_scan failed ({rc}): " + last_error())
        return ScanResult(_WorkerScanner(lib().matchy_multi_scanner_worker_scanner(self._h, 0)), raw)

    def set_line_context(self, on: bool):
        """line context for every worker's scanner, from the next batch on"""
        lib().matchy_multi_scanner_set_line_context(self._h, bool(on))

    def set_hit_lines(self, on: bool):
        """hit lines for every worker's scanner, from the next batch on: batches from next() answer hit_lines() and render without text"""
        lib().matchy_multi_scanner_set_hit_lines(self._h, bool(on))

    def set_gz_pieces(self, piece_bytes=0):
        """Scanner.set_gz_pieces on every worker's scanner, from the next gz batch on"""
        if lib().matchy_multi_scanner_set_gz_pieces(self._h, piece_bytes) != 0:
            raise ValueError(f"matchy_multi_scanner_set_gz_pieces failed: {last_error()}")

    def set_render(self, flags=0, source=None, sources=None, line_base=0, line_bases=None):
        """arms the NEXT batch submitted (submit_ptr / submit_segments_ptr / submit_gz_ptr) like Scanner.set_render: next() then carries
        "rendered", the NDJSON text of the batch written on the GPU (matchy_multi_scanner_set_render). flags=None disarms."""
        p = _render_params(flags, source, sources, line_base, line_bases)
        rc = lib().matchy_multi_scanner_set_render(self._h, None if p is None else C.byref(p))
        if rc != 0:
            raise RuntimeError(f"matchy_multi_scanner_set_render failed ({rc}): " + last_error())

    def set_whole_lines(self, on=True):
        """whole-line queries on every worker's scanner, from the next batch on; needs pending() == 0"""
        rc = lib().matchy_multi_scanner_set_whole_lines(self._h, bool(on))
        if rc != 0:
            raise RuntimeError(f"matchy_multi_scanner_set_whole_lines failed ({rc}): " + last_error())

    def set_tally(self, on=True):
        """hit tally on every worker's scanner, from the next batch on"""
        rc = lib().matchy_multi_scanner_set_tally(self._h, bool(on))
        if rc != 0:
            raise RuntimeError(f"matchy_multi_scanner_set_tally failed ({rc}): " + last_error())

    def reset_tally(self):
        lib().matchy_multi_scanner_reset_tally(self._h)

    def tally(self, limit=0):
        """the workers' tallies merged by (type, text), then ordered and cut like Scanner.tally; needs pending() == 0"""
        return _read_tally(lib().matchy_multi_scanner_tally_top, self._h, limit, "matchy_multi_scanner_tally_top")

    def submit_ptr(self, host_ptr: int, nbytes: int, tag: int = 0, numa_node: int = -1):
        """queue one newline-aligned batch that lives at a host address (e.g. a pinned torch tensor); take it back with next().
        Blocks while max_pending() batches are out: a caller that submits and gathers on one thread calls next() when
        pending() has reached max_pending(). numa_node: the node the bytes live on (-1 = anywhere)."""
        rc = lib().matchy_multi_scanner_submit_near(self._h, host_ptr, nbytes, tag, None, numa_node)
        if rc != 0:
            raise RuntimeError(f"matchy_multi_scanner_submit failed ({rc}): " + last_error())

    def submit_segments_ptr(self, host_ptr: int, nbytes: int, starts, tag: int = 0):
        """submit_ptr of a batch of len(starts) segments (matchy_multi_scanner_submit_segments); next() then carries the segment table"""
        arr = (C.c_uint32 * len(starts))(*starts)
        rc = lib().matchy_multi_scanner_submit_segments(self._h, host_ptr, nbytes, arr, len(starts), tag, None)
        if rc != 0:
            raise RuntimeError(f"matchy_multi_scanner_submit_segments failed ({rc}): " + last_error())

    def submit_gz_stream_ptr(self, host_ptr: int, nbytes: int, state=None, carry=b"", carry_cap=1 << 20, text_cap=1 << 20, first=False, file_end=False, want_text=False,
                             tag: int = 0):
        """queue one window of one large DEFLATE stream whose compressed bytes live at a host address (matchy_multi_scanner_submit_gz_stream;
        set_gz_pieces comes first). next() then carries "gz_stream" (ScanResult.gz_stream) and, with want_text, the batch"""
        keep = C.create_string_buffer(bytes(carry), len(carry)) if carry else None
        w = _GzStreamWindow(C.pointer(state) if state is not None else None, C.addressof(keep) if keep is not None else None, len(carry), carry_cap, text_cap,
                            (STREAM_FIRST if first else 0) | (STREAM_FILE_END if file_end else 0))
        rc = lib().matchy_multi_scanner_submit_gz_stream(self._h, host_ptr, nbytes, C.byref(w), bool(want_text), tag)
        if rc != 0:
            raise RuntimeError(f"matchy_multi_scanner_submit_gz_stream failed ({rc}): " + last_error())

    def submit_utf16_ptr(self, host_ptr: int, nbytes: int, byte_order=UTF16_LE, want_text=False, tag: int = 0):
        """queue one UTF-16 batch that lives at a host address (matchy_multi_scanner_submit_utf16). next() then carries "utf16" (code
        units and U+FFFD written) and "text": the UTF-8 batch with want_text, else None"""
        rc = lib().matchy_multi_scanner_submit_utf16(self._h, host_ptr, nbytes, byte_order, bool(want_text), tag, None)
        if rc != 0:
            raise RuntimeError(f"matchy_multi_scanner_submit_utf16 failed ({rc}): " + last_error())

    def submit_escaped(self, host_ptr: int, nbytes: int, modes=UNESCAPE_PERCENT, want_text=False, tag: int = 0):
        """queue one escaped batch that lives at a host address (matchy_multi_scanner_submit_escaped). next() then carries "unescaped"
        (text_len and the counters) and "text": the decoded batch with want_text, else None"""
        rc = lib().matchy_multi_scanner_submit_escaped(self._h, host_ptr, nbytes, modes, bool(want_text), tag, None)
        if rc != 0:
            raise RuntimeError(f"matchy_multi_scanner_submit_escaped failed ({rc}): " + last_error())

    def submit_gz_ptr(self, host_ptr: int, nbytes: int, members, want_text=False, tag: int = 0):
        """queue a pack of gzip files that lives at a host address: members = [(offset, len, out_len)] (matchy_multi_scanner_submit_gz).
        next() then carries gz_status, the segment table and, with want_text, the inflated text"""
        table = (_GzMember * len(members))()
        for i, (off, ln, out_len) in enumerate(members):
            table[i].offset, table[i].len, table[i].out_len = off, ln, out_len
        rc = lib().matchy_multi_scanner_submit_gz(self._h, host_ptr, nbytes, table, len(members), bool(want_text), tag)
        if rc != 0:
            raise RuntimeError(f"matchy_multi_scanner_submit_gz failed ({rc}): " + last_error())

    def submit_gz_files_ptr(self, host_ptr: int, nbytes: int, files, want_text=False, tag: int = 0):
        """queue a pack of gzip files of one member or many that lives at a host address: files = [(offset, len)]
        (matchy_multi_scanner_submit_gz_files). next() then carries gz_file_status and gz_first_member as well"""
        table = (_GzFile * len(files))()
        for i, (off, ln) in enumerate(files):
            table[i].offset, table[i].len = off, ln
        rc = lib().matchy_multi_scanner_submit_gz_files(self._h, host_ptr, nbytes, table, len(files), bool(want_text), tag)
        if rc != 0:
            raise RuntimeError(f"matchy_multi_scanner_submit_gz_files failed ({rc}): " + last_error())

    def submit_gz_window_ptr(self, host_ptr: int, nbytes: int, carry=b"", carry_cap=1 << 20, last=False, want_text=False, tag: int = 0):
        """queue one window of a large multi-member gzip file whose members live at a host address (matchy_multi_scanner_submit_gz_window;
        the carry is copied). next() then carries window_status and carry as well"""
        keep = C.create_string_buffer(bytes(carry), len(carry)) if carry else None
        w = _GzWindow(C.addressof(keep) if keep is not None else None, len(carry), carry_cap, WINDOW_LAST if last else 0)
        rc = lib().matchy_multi_scanner_submit_gz_window(self._h, host_ptr, nbytes, C.byref(w), bool(want_text), tag)
        if rc != 0:
            raise RuntimeError(f"matchy_multi_scanner_submit_gz_window failed ({rc}): " + last_error())

    def pending(self) -> int:
        return lib().matchy_multi_scanner_pending(self._h)

    def max_pending(self) -> int:
        return lib().matchy_multi_scanner_max_pending(self._h)

    def worker_numa(self):
        """[(NUMA node of the worker's GPU, CPUs its thread is bound to)] per worker"""
        out = []
        for w in range(self.workers):
            node, cpus = C.c_int32(-1), C.c_int32(0)
            lib().matchy_multi_scanner_worker_numa(self._h, w, C.byref(node), C.byref(cpus))
            out.append((node.value, cpus.value))
        return out

    def next(self, want_hits=False):
        """the next batch in submission order: dict(seq, tag, worker, lines, candidates, n_hits[, hits]) or None when nothing is pending"""
        b = _MultiBatch()
        rc = lib().matchy_multi_scanner_next(self._h, C.byref(b))
        if rc == 0:
            return None
        if rc != 1 or b.status != 0:
            raise RuntimeError(f"matchy_multi_scanner_next failed ({rc}, batch status {b.status}): " + last_error())
        out = dict(seq=b.seq, tag=int(b.tag or 0), worker=b.worker, lines=int(b.result.lines), candidates=int(b.result.candidates),
                   n_hits=int(b.result.n_hits + b.result.n_ip4_hits), nbytes=int(b.len))
        r = ScanResult(_WorkerScanner(lib().matchy_multi_scanner_worker_scanner(self._h, b.worker)), b.result)
        if want_hits:
            out["hits"] = r.hits()
        if r.has_lines:   # relative to the batch
            out["lines_with_matches"] = r.lines_with_matches
            if want_hits:
                out["line_records"] = r.line_records
        if r.has_segments:
            out["segments"] = r.segments
            if want_hits:
                out["segment_of"] = r.segment_of
        hl = r.hit_lines()
        if hl is not None:   # set_hit_lines: the block, and with want_hits the records rendered from it alone
            out["hit_lines"] = hl
            if want_hits:
                out["ndjson_lines"] = r.ndjson_lines_text(None, with_input_line=True)
        if lib().matchy_scan_result_ndjson(C.byref(r._raw), None, None, None) == 0:   # the batch was armed with set_render
            out["rendered"] = r.rendered_ndjson()
        gz = r.gz_status()
        if gz is not None:   # a gz batch: data / len are the inflated text (NULL without want_text) and its length
            out["gz_status"] = gz
            out["text"] = C.string_at(b.data, b.len) if b.data else None
            if r.gz_file_status() is not None:
                out["gz_file_status"], out["gz_first_member"] = r.gz_file_status(), r.gz_first_member()
            if r.gz_window() is not None:
                out["window_status"], out["carry"] = r.gz_window()
            if r.gz_stream() is not None:
                out["gz_stream"] = r.gz_stream()
        u = r.utf16()
        if u is not None:   # a UTF-16 batch: data / len are the UTF-8 text (NULL without want_text) and its length
            out["text"] = C.string_at(b.data, b.len) if b.data else None
            out["utf16"] = dict(text_len=u["text_len"], code_units=u["code_units"], replaced=u["replaced"])
        u = r.unescaped()
        if u is not None:   # an escaped batch: data / len are the decoded text (NULL without want_text) and its length
            out["text"] = C.string_at(b.data, b.len) if b.data else None
            out["unescaped"] = {k: u[k] for k in ("text_len", "escapes", "replaced", "lf_escapes")}
        r.close()
        return out

    def scan_file(self, path: str, batch_bytes: int = 0, on_batch=None):
        """scan one file (or "-"); on_batch(offset, nbytes, hits, lines, candidates) is called per batch in file order. Returns the totals."""
        L = lib()
        me = self

        def cb(_user, bp):
            b = bp.contents
            if on_batch is not None:
                r = ScanResult(_WorkerScanner(L.matchy_multi_scanner_worker_scanner(me._h, b.worker)), b.result)
                try:
                    on_batch(int(b.tag or 0), int(b.len), r.hits(), int(b.result.lines), int(b.result.candidates))
                finally:
                    r._raw = None   # the library releases the result when the callback returns
            return 0

        fn = _MULTI_ORDERED_FN(cb)
        tot = _MultiTotals()
        rc = L.matchy_multi_scanner_scan_file(self._h, os.fsencode(path), batch_bytes, fn, None, C.byref(tot))
        if rc != 0:
            raise RuntimeError(f"matchy_multi_scanner_scan_file failed ({rc}): " + last_error())
        return dict(batches=tot.batches, bytes=tot.bytes, lines=tot.lines, candidates=tot.candidates, matches=tot.matches)

    def close(self):
        if self._h:
            lib().matchy_multi_scanner_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def utf16_geometry():
    """(input bytes per tile, tiles per workgroup of the prefix step) of the UTF-16 passes (matchy_amd_utf16_geometry)"""
    out = (C.c_uint32 * 2)()
    lib().matchy_amd_utf16_geometry(out)
    return int(out[0]), int(out[1])


def unescape_geometry():
    """(input bytes per tile, tiles per workgroup of the prefix step, tiles per workgroup of the state scan) of the unescape passes
    (matchy_amd_unescape_geometry)"""
    out = (C.c_uint32 * 3)()
    lib().matchy_amd_unescape_geometry(out)
    return int(out[0]), int(out[1]), int(out[2])


def numa_cpus(sysfs_root: str, pci_bus_id: str):
    """CPUs on the NUMA node of a PCI device under any sysfs root (matchy_amd_numa_cpus: the mapping the workers bind with)"""
    out = (C.c_int32 * 4096)()
    n = lib().matchy_amd_numa_cpus(os.fsencode(sysfs_root), pci_bus_id.encode(), out, 4096)
    return [out[i] for i in range(max(0, min(n, 4096)))]
