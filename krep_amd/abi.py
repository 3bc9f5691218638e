"""ctypes mirror of include/krep_gpu.h (== reference krep.h:49-101 layouts).

Only plumbing: struct layouts, a `make_params()` factory that reads like the reference tests'
`create_literal_params()` (test/test_krep.c:239-249), and numpy views of match_result_t.
No search logic lives here.
"""
from __future__ import annotations

import ctypes as C
from typing import Iterable, Sequence

import numpy as np

SIZE_MAX = (1 << 64) - 1

# enum krep_ref_simd
REF_SCALAR, REF_SSE42, REF_AVX2, REF_AVX512, REF_NEON = 0, 1, 2, 3, 4
# enum krep_ref_algo
(RA_NONE, RA_BMH, RA_KMP, RA_MEMCHR, RA_MEMCHR_SHORT, RA_SSE42, RA_AVX2, RA_AVX512, RA_NEON,
 RA_AHO_CORASICK, RA_REGEX) = range(11)
ALGO_AUTO, ALGO_BM, ALGO_KMP = 0, 1, 2

RA_NAMES = {RA_BMH: "boyer_moore_search", RA_KMP: "kmp_search", RA_MEMCHR: "memchr_search",
            RA_MEMCHR_SHORT: "memchr_short_search", RA_SSE42: "simd_sse42_search",
            RA_AVX2: "simd_avx2_search", RA_AVX512: "simd_avx512_search", RA_NEON: "neon_search",
            RA_AHO_CORASICK: "aho_corasick_search"}


class MatchPosition(C.Structure):
    _fields_ = [("start_offset", C.c_size_t), ("end_offset", C.c_size_t)]


class MatchResult(C.Structure):
    _fields_ = [("positions", C.POINTER(MatchPosition)), ("count", C.c_uint64),
                ("capacity", C.c_uint64)]


class SearchParams(C.Structure):
    _fields_ = [
        ("pattern", C.c_char_p), ("pattern_len", C.c_size_t),
        ("patterns", C.POINTER(C.c_char_p)), ("pattern_lens", C.POINTER(C.c_size_t)),
        ("num_patterns", C.c_size_t),
        ("case_sensitive", C.c_bool), ("use_regex", C.c_bool), ("count_lines_mode", C.c_bool),
        ("count_matches_mode", C.c_bool), ("track_positions", C.c_bool), ("whole_word", C.c_bool),
        ("compiled_regex", C.c_void_p), ("ac_trie", C.c_void_p), ("max_count", C.c_size_t),
    ]


assert C.sizeof(SearchParams) == 72 and C.sizeof(MatchPosition) == 16 and C.sizeof(MatchResult) == 24


class ScanOut(C.Structure):
    _fields_ = [("count", C.c_uint64), ("stored", C.c_uint64), ("total_matches", C.c_uint64),
                ("line_count", C.c_uint64), ("head_line_hit", C.c_uint8), ("tail_line_hit", C.c_uint8),
                ("has_newline", C.c_uint8), ("overflow", C.c_uint8), ("kernel_ms", C.c_float)]


class LinesOut(C.Structure):
    """krep_gpu_lines_out_t: what krep_gpu_matching_lines / krep_gpu_format_lines report"""
    _fields_ = [("lines", C.c_uint64), ("lines_total", C.c_uint64), ("out_bytes", C.c_uint64), ("capped_lines", C.c_uint64),
                ("overflow", C.c_int)]


class LineFormat(C.Structure):
    """krep_gpu_line_format_t: the four host strings krep_gpu_format_lines_ex puts around a line and its matches"""
    _fields_ = [("prefix", C.c_char_p), ("prefix_len", C.c_size_t), ("before_match", C.c_char_p), ("before_match_len", C.c_size_t),
                ("after_match", C.c_char_p), ("after_match_len", C.c_size_t), ("line_close", C.c_char_p), ("line_close_len", C.c_size_t)]

    def __init__(self, prefix: bytes = b"", before_match: bytes = b"", after_match: bytes = b"", line_close: bytes = b""):
        super().__init__(prefix, len(prefix), before_match, len(before_match), after_match, len(after_match), line_close,
                         len(line_close))


class LinesWindow(C.Structure):
    """krep_gpu_lines_window_t: which part of a text the buffer of krep_gpu_format_lines_window holds and which lines the call owns"""
    _fields_ = [("global_base", C.c_size_t), ("global_len", C.c_size_t), ("own_lo", C.c_size_t), ("own_hi", C.c_size_t),
                ("records_hi", C.c_size_t)]


class LinesWindowOut(C.Structure):
    """krep_gpu_lines_window_out_t: LinesOut of the owned, complete lines, and the owned line that could not be completed"""
    _fields_ = [("lines", LinesOut), ("incomplete_line_start1", C.c_uint64), ("incomplete_first_record", C.c_uint64)]


class MatchFormat(C.Structure):
    """krep_gpu_match_format_t: the four host strings krep_gpu_format_matches puts around LINE and the match"""
    _fields_ = [("prefix", C.c_char_p), ("prefix_len", C.c_size_t), ("before_number", C.c_char_p), ("before_number_len", C.c_size_t),
                ("after_number", C.c_char_p), ("after_number_len", C.c_size_t), ("after_match", C.c_char_p), ("after_match_len", C.c_size_t)]

    def __init__(self, prefix: bytes = b"", before_number: bytes = b"", after_number: bytes = b"", after_match: bytes = b""):
        super().__init__(prefix, len(prefix), before_number, len(before_number), after_number, len(after_number), after_match,
                         len(after_match))


class MatchesOut(C.Structure):
    """krep_gpu_matches_out_t: what krep_gpu_format_matches reports"""
    _fields_ = [("items", C.c_uint64), ("out_bytes", C.c_uint64), ("overflow", C.c_int)]


class MatchesWindow(C.Structure):
    """krep_gpu_matches_window_t: which part of a text the buffer of krep_gpu_format_matches_window holds, and the two carries in"""
    _fields_ = [("global_base", C.c_size_t), ("global_len", C.c_size_t), ("count_to", C.c_size_t), ("newlines_before", C.c_uint64),
                ("last_newline1", C.c_uint64), ("stale_line", C.c_uint64), ("stale_rule", C.c_int), ("reserved", C.c_int)]


class MatchesWindowOut(C.Structure):
    """krep_gpu_matches_window_out_t: MatchesOut of the call's records, and the two carries out"""
    _fields_ = [("matches", MatchesOut), ("newlines_before_count_to", C.c_uint64), ("stale_line", C.c_uint64)]


class Config(C.Structure):
    """krep_gpu_config_t: the reference's build level and file-static option globals, explicit."""
    _fields_ = [("reference_simd", C.c_int), ("only_matching", C.c_int), ("force_no_simd", C.c_int),
                ("algo_override", C.c_int), ("result_order", C.c_int), ("device", C.c_int),
                ("stream_chunk_bytes", C.c_size_t), ("num_gpus", C.c_int), ("min_text_bytes", C.c_size_t)]


class CostRates(C.Structure):
    """krep_gpu_cost_rates_t"""
    _fields_ = [("enabled", C.c_int), ("gpu_host_path_gbps", C.c_double), ("gpu_launch_us", C.c_double), ("gpu_init_ms", C.c_double),
                ("cpu_memchr_gbps", C.c_double), ("cpu_memchr_cap_gbps", C.c_double), ("cpu_simd_gbps", C.c_double),
                ("cpu_simd_cap_gbps", C.c_double), ("cpu_scalar_gbps", C.c_double), ("cpu_scalar_cap_gbps", C.c_double),
                ("cpu_ac_gbps", C.c_double), ("cpu_ac_cap_gbps", C.c_double), ("cpu_ac_cache_bytes", C.c_double),
                ("cpu_ac_exponent", C.c_double)]


class Cost(C.Structure):
    """krep_gpu_cost_t"""
    _fields_ = [("gpu_seconds", C.c_double), ("cpu_seconds", C.c_double), ("gpu_host_path_gbps", C.c_double),
                ("cpu_threads", C.c_int), ("cpu_algo", C.c_int), ("device_ready", C.c_int)]


class RegexInfo(C.Structure):
    """krep_gpu_regex_info_t: what krep_gpu_regex_compile() makes of an -E pattern"""
    _fields_ = [("L", C.c_uint32), ("classes", (C.c_uint8 * 32) * 16), ("self_overlap", C.c_int), ("anchor", C.c_uint32),
                ("anchor_bytes", C.c_uint8 * 4), ("n_anchor", C.c_uint32)]

    def class_bytes(self, j: int) -> bytes:
        """the bytes of class j, ascending"""
        return bytes(b for b in range(256) if (self.classes[j][b >> 3] >> (b & 7)) & 1)


class RegexAnchored(C.Structure):
    """krep_gpu_regex_anchored_t: what krep_gpu_regex_compile_anchored() makes of an -E pattern with an optional ^ in front and $ behind"""
    _fields_ = [("seq", RegexInfo), ("bol", C.c_int), ("eol", C.c_int)]


class RegexAlt(C.Structure):
    """krep_gpu_regex_alt_t: what krep_gpu_regex_compile_alt() makes of an alternation of class sequences (a|b, several -e patterns)"""
    _fields_ = [("n_branches", C.c_uint32), ("Lmin", C.c_uint32), ("Lmax", C.c_uint32), ("total_L", C.c_uint32),
                ("cross_overlap", C.c_int), ("reserved", C.c_uint32), ("branch", RegexInfo * 8)]


class RegexExt(C.Structure):
    """krep_gpu_regex_ext_t: what krep_gpu_regex_compile_ext() expands ?, {n,m}, inner groups and anchored alternations into: an
    alternation over the real classes between the line anchors bol / eol"""
    _fields_ = [("alt", RegexAlt), ("bol", C.c_int), ("eol", C.c_int)]


class RegexLoops(C.Structure):
    """krep_gpu_regex_loops_t: what krep_gpu_regex_compile_loops() makes of an expression with *, + or {n,} behind an atom: the expanded
    sequences of places (alt; L counts places), the line anchors, per branch the mask of the places that repeat, and the filter"""
    _fields_ = [("alt", RegexAlt), ("bol", C.c_int), ("eol", C.c_int), ("repeat", C.c_uint16 * 8), ("filter", RegexAlt)]


class RegexGroups(C.Structure):
    """krep_gpu_regex_groups_t: what krep_gpu_regex_compile_groups() makes of an expression with repeated or nested groups: its
    position automaton (one position per atom occurrence: classes, first, last, follow), the line anchors and the filter"""
    _fields_ = [("n_pos", C.c_uint32), ("classes", (C.c_uint8 * 32) * 32), ("first", C.c_uint32), ("last", C.c_uint32),
                ("follow", C.c_uint32 * 32), ("bol", C.c_int), ("eol", C.c_int), ("filter", RegexAlt)]

    def class_bytes(self, i: int) -> bytes:
        """the bytes of position i's class, ascending"""
        return bytes(b for b in range(256) if (self.classes[i][b >> 3] >> (b & 7)) & 1)


class ShardInfo(C.Structure):
    """krep_gpu_shard_info_t: where the calling thread's last sharded host search ran."""
    _fields_ = [("shards", C.c_int), ("devices_used", C.c_int), ("device_ids", C.c_int * 16), ("comm_ranks", C.c_int),
                ("reduced_by", C.c_int)]


class BatchItem(C.Structure):
    """krep_gpu_batch_item_t: one text of a batch (a host pointer and its length)"""
    _fields_ = [("text", C.c_void_p), ("len", C.c_size_t)]


class BatchResult(C.Structure):
    """krep_gpu_batch_result_t: what krep_gpu_search_batch reports per item"""
    _fields_ = [("count", C.c_uint64), ("first_record", C.c_uint64), ("n_records", C.c_uint64)]


class BatchInfo(C.Structure):
    """krep_gpu_batch_info_t: what a whole krep_gpu_search_batch call took"""
    _fields_ = [("packed_bytes", C.c_uint64), ("scans", C.c_uint64), ("total_records", C.c_uint64), ("kernel_ms", C.c_float)]


class PackView(C.Structure):
    """krep_gpu_pack_view_t: the offset table and the per-item prefixes of a pack, all device pointers"""
    _fields_ = [("d_item_off", C.c_void_p), ("n_items", C.c_uint64), ("d_prefix_bytes", C.c_void_p), ("d_prefix_off", C.c_void_p)]


class GrepFormat(C.Structure):
    """krep_gpu_grep_format_t: the per-item prefixes (host strings) and the other strings of both output forms"""
    _fields_ = [("prefixes", C.POINTER(C.c_char_p)), ("prefix_lens", C.POINTER(C.c_size_t)), ("line", LineFormat), ("match", MatchFormat)]


class GrepItem(C.Structure):
    """krep_gpu_grep_item_t: an item's count and where its bytes lie in the output, relative to out->len at entry"""
    _fields_ = [("count", C.c_uint64), ("out_offset", C.c_uint64), ("out_bytes", C.c_uint64)]


class GrepOutput(C.Structure):
    """krep_gpu_grep_output_t: a malloc-family block krep_gpu_grep_batch appends to"""
    _fields_ = [("bytes", C.c_void_p), ("len", C.c_size_t), ("capacity", C.c_size_t)]


STATUS_OK, STATUS_FELL_BACK, STATUS_FAILED = 0, 1, 2
SPLIT_WHOLE, SPLIT_PIECES, SPLIT_CHAIN = 0, 1, 2


class SeqCarry(C.Structure):
    """krep_gpu_seq_carry_t: the boundary record of the sequential match-set families."""
    _fields_ = [("resume", C.c_uint64), ("q1", C.c_uint64), ("nl1", C.c_uint64), ("local_q1", C.c_uint64),
                ("local_nl1", C.c_uint64), ("local_first_nl1", C.c_uint64), ("g0", C.c_uint64), ("local_g0", C.c_uint64),
                ("local_g0_kind", C.c_uint64), ("nl_before", C.c_uint64), ("last_line", C.c_uint64), ("local_nl", C.c_uint64),
                ("local_last", C.c_uint64), ("local_lines", C.c_uint64)]


class AcScan(C.Structure):
    """krep_gpu_debug_ac_scan_t (include/krep_gpu_debug.h): which multi-pattern kernel answered a dictionary's last scan"""
    _fields_ = [("road", C.c_uint32), ("ci", C.c_uint32), ("lines", C.c_uint32), ("shorts", C.c_uint32), ("stride", C.c_uint32),
                ("anch", C.c_uint32), ("ww_filter", C.c_uint32), ("exact", C.c_uint32), ("g4x_mode", C.c_uint32),
                ("stage_cap", C.c_uint32), ("upt", C.c_uint32), ("n_units", C.c_uint64), ("overflow_units", C.c_uint64),
                ("emit", C.c_uint32), ("next_stage_cap", C.c_uint32), ("short_lens", C.c_uint32), ("scans", C.c_uint64)]

    def as_dict(self):
        return {name: int(getattr(self, name)) for name, _ in self._fields_}


SEARCH_FUNC = C.CFUNCTYPE(C.c_uint64, C.POINTER(SearchParams), C.c_char_p, C.c_size_t,
                          C.POINTER(MatchResult))


class Placement(C.Structure):
    """krep_gpu_placement_t (include/krep_gpu.h): what krep_gpu_alloc_placed() drew"""
    _fields_ = [("tries", C.c_uint32), ("kept", C.c_uint32), ("count_only_ms", C.c_float * 8), ("records_ms", C.c_float * 8)]


class Params:
    """Owns the Python-side buffers a search_params_t points into.  regex=True sets use_regex (krep -E): the library takes such a search
    only in the C locale — Python enters the environment's locale at start-up, so call locale.setlocale(locale.LC_CTYPE, "C") before
    Engine.search / Engine.plan / Engine.regex_compile, or every pattern is refused (Engine.regex_compile says why)."""

    def __init__(self, patterns: Sequence[bytes], *, case_sensitive=True, count_lines=False,
                 only_match=False, whole_word=False, max_count=SIZE_MAX, track_positions=None, regex=False):
        pats = [bytes(p) for p in patterns]
        self._pats = pats
        n = len(pats)
        self._arr = (C.c_char_p * max(n, 1))(*pats) if n else (C.c_char_p * 1)()
        self._lens = (C.c_size_t * max(n, 1))(*[len(p) for p in pats]) if n else (C.c_size_t * 1)()
        s = SearchParams()
        s.patterns = C.cast(self._arr, C.POINTER(C.c_char_p)) if n else None
        s.pattern_lens = C.cast(self._lens, C.POINTER(C.c_size_t)) if n else None
        s.num_patterns = n
        if n:
            # legacy single-pattern fields (test_krep.c:233-235); c_char_p keeps embedded NULs
            # because pattern_len carries the length
            s.pattern = pats[0]
            s.pattern_len = len(pats[0])
        s.case_sensitive = case_sensitive
        s.use_regex = bool(regex)
        # create_base_params(), test/test_krep.c:225-229
        s.count_lines_mode = bool(count_lines and not only_match)
        s.count_matches_mode = bool(count_lines and only_match)
        s.track_positions = (not (count_lines and not only_match)) if track_positions is None \
            else bool(track_positions)
        s.whole_word = whole_word
        s.max_count = max_count
        self.s = s

    @property
    def ref(self):
        return C.byref(self.s)


def make_params(pattern, **kw) -> Params:
    if isinstance(pattern, (bytes, bytearray)):
        return Params([bytes(pattern)], **kw)
    return Params(list(pattern), **kw)


def result_positions(res_ptr) -> np.ndarray:
    """(count, 2) uint64 copy of a match_result_t*'s positions."""
    r = res_ptr.contents if hasattr(res_ptr, "contents") else res_ptr
    n = int(r.count)
    if n == 0:
        return np.zeros((0, 2), dtype=np.uint64)
    buf = C.cast(r.positions, C.POINTER(C.c_uint64 * (2 * n))).contents
    return np.frombuffer(buf, dtype=np.uint64).reshape(n, 2).copy()


def as_char_p(buf) -> C.c_char_p:
    """Pointer to a bytes / numpy uint8 buffer without copying (bytes) or via ctypes (ndarray)."""
    if isinstance(buf, np.ndarray):
        assert buf.dtype == np.uint8 and buf.flags["C_CONTIGUOUS"]
        return C.cast(buf.ctypes.data, C.c_char_p)
    return C.c_char_p(bytes(buf)) if not isinstance(buf, bytes) else C.c_char_p(buf)
