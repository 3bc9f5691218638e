"""ctypes binding of include/krep_gpu.h.  Plumbing only — every search runs in libkrep_gpu.so."""
from __future__ import annotations

import contextlib
import ctypes as C
import os

import numpy as np

from . import abi

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "lib", "libkrep_gpu.so")


def _libc_free(ptr: int):
    """free() of a malloc-family block the library handed out (krep_gpu_grep_output_t.bytes)"""
    libc = C.CDLL(None)
    libc.free.restype = None
    libc.free.argtypes = [C.c_void_p]
    libc.free(C.c_void_p(ptr))


class KrepGpuError(RuntimeError):
    pass


@contextlib.contextmanager
def _borrowed_trie(params: "abi.Params"):
    """"caller pre-built the trie" (krep.c:2528) for the calls inside: a multi-pattern search without ac_trie is answered with no
    match (aho_corasick.c:306), so params.s.ac_trie points at a dummy meanwhile and is NULL again afterwards"""
    dummy = C.c_int(0)
    if params.s.num_patterns > 1 and not params.s.ac_trie:
        params.s.ac_trie = C.cast(C.pointer(dummy), C.c_void_p)
    try:
        yield
    finally:
        params.s.ac_trie = None


class Engine:
    """Thin face over the C-ABI.  Host-buffer operators mirror krep's search_func_t; the device path
    takes raw device pointers (e.g. torch tensors' data_ptr())."""

    def __init__(self, path: str = LIB_PATH):
        path = os.environ.get("KREP_GPU_LIB", path)  # development aid: A/B two builds of the library in one GPU session
        if not os.path.exists(path):
            raise KrepGpuError(f"{path} is missing: build it with `python -m krep_amd.build` "
                               "(hipcc --offload-arch=gfx950); there is no CPU fallback")
        # When torch is used in the same process (tests, bench.py: device memory + torch.distributed), its
        # bundled HIP runtime must be the one the process binds first; loading ours first makes torch see
        # "No HIP GPUs".  Importing torch here is plumbing only — nothing in the library needs it.
        if not os.environ.get("KREP_GPU_NO_TORCH"):  # (tools/notorch_bench.py: the library on the system HIP runtime alone)
            try:
                import torch  # noqa: F401
            except Exception:
                pass
        L = self.lib = C.CDLL(path)
        sf = [C.POINTER(abi.SearchParams), C.c_void_p, C.c_size_t, C.POINTER(abi.MatchResult)]
        for n in ("krep_gpu_literal_search", "krep_gpu_aho_corasick_search", "krep_gpu_regex_search"):
            getattr(L, n).restype = C.c_uint64
            getattr(L, n).argtypes = sf
        L.krep_gpu_select_search_algorithm.restype = C.c_void_p
        L.krep_gpu_select_search_algorithm.argtypes = [C.POINTER(abi.SearchParams)]
        L.search_buffer.restype = C.c_int
        L.search_buffer.argtypes = [C.POINTER(abi.SearchParams), C.c_void_p, C.c_size_t, C.c_int, C.c_int,
                                    C.POINTER(abi.MatchResult), C.POINTER(C.c_uint64)]
        L.search_buffer_ex.restype = C.c_int
        L.search_buffer_ex.argtypes = [C.POINTER(abi.SearchParams), C.c_void_p, C.c_size_t, C.POINTER(abi.Config), C.c_int,
                                       C.POINTER(abi.MatchResult), C.POINTER(C.c_uint64)]
        L.krep_gpu_regex_compile.restype = C.c_int
        L.krep_gpu_regex_compile.argtypes = [C.POINTER(abi.SearchParams), C.POINTER(abi.RegexInfo)]
        if hasattr(L, "krep_gpu_regex_compile_anchored"):  # (an older build loaded as an A/B partner lacks it: tools/ab_bench.py)
            L.krep_gpu_regex_compile_anchored.restype = C.c_int
            L.krep_gpu_regex_compile_anchored.argtypes = [C.POINTER(abi.SearchParams), C.POINTER(abi.RegexAnchored)]
        if hasattr(L, "krep_gpu_regex_compile_alt"):  # (likewise)
            L.krep_gpu_regex_compile_alt.restype = C.c_int
            L.krep_gpu_regex_compile_alt.argtypes = [C.POINTER(abi.SearchParams), C.POINTER(abi.RegexAlt)]
        if hasattr(L, "krep_gpu_regex_compile_ext"):  # (likewise)
            L.krep_gpu_regex_compile_ext.restype = C.c_int
            L.krep_gpu_regex_compile_ext.argtypes = [C.POINTER(abi.SearchParams), C.POINTER(abi.RegexExt)]
        L.krep_gpu_can_accelerate.restype = C.c_int
        L.krep_gpu_can_accelerate.argtypes = [C.POINTER(abi.SearchParams)]
        L.krep_gpu_config_default.restype = None
        L.krep_gpu_config_default.argtypes = [C.POINTER(abi.Config)]
        L.krep_gpu_set_thread_config.restype = None
        L.krep_gpu_set_thread_config.argtypes = [C.POINTER(abi.Config)]
        L.krep_gpu_set_stream_chunk.restype = None
        L.krep_gpu_set_stream_chunk.argtypes = [C.c_size_t]
        L.krep_gpu_release_device_resources.restype = None
        L.krep_gpu_plan_create_ex.restype = C.c_void_p
        L.krep_gpu_plan_create_ex.argtypes = [C.POINTER(abi.SearchParams), C.POINTER(abi.Config)]
        L.krep_gpu_scan_device_ex.restype = C.c_int
        L.krep_gpu_scan_device_ex.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t,
                                              C.c_void_p, C.c_uint64, C.c_void_p, C.c_int, C.POINTER(abi.ScanOut)]
        L.krep_gpu_scan_device_seq.restype = C.c_int
        L.krep_gpu_scan_device_seq.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t,
                                               C.c_void_p, C.c_uint64, C.c_void_p, C.c_int, C.POINTER(abi.SeqCarry),
                                               C.POINTER(abi.SeqCarry), C.POINTER(abi.ScanOut)]
        L.krep_gpu_split_mode.restype = C.c_int
        L.krep_gpu_split_mode.argtypes = [C.POINTER(abi.SearchParams), C.c_size_t]
        L.krep_gpu_match_result_init.restype = C.POINTER(abi.MatchResult)
        L.krep_gpu_match_result_init.argtypes = [C.c_uint64]
        L.krep_gpu_match_result_free.restype = None
        L.krep_gpu_match_result_free.argtypes = [C.POINTER(abi.MatchResult)]
        L.krep_gpu_plan_create.restype = C.c_void_p
        L.krep_gpu_plan_create.argtypes = [C.POINTER(abi.SearchParams), C.c_int, C.c_int]
        L.krep_gpu_plan_destroy.restype = None
        L.krep_gpu_plan_destroy.argtypes = [C.c_void_p]
        L.krep_gpu_plan_ref_algo.restype = C.c_int
        L.krep_gpu_plan_ref_algo.argtypes = [C.c_void_p]
        L.krep_gpu_scan_device.restype = C.c_int
        L.krep_gpu_scan_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t,
                                           C.c_void_p, C.c_uint64, C.c_void_p, C.c_int, C.POINTER(abi.ScanOut)]
        L.krep_gpu_generate.restype = C.c_int
        L.krep_gpu_generate.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_uint64, C.c_void_p,
                                        C.c_size_t, C.c_uint64, C.c_void_p]
        L.krep_gpu_generate_host.restype = None
        L.krep_gpu_generate_host.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_uint64, C.c_void_p,
                                             C.c_size_t, C.c_uint64]
        L.krep_gpu_combine_line_counts.restype = C.c_uint64
        L.krep_gpu_combine_line_counts.argtypes = [C.POINTER(abi.ScanOut), C.c_int]
        L.krep_gpu_mirror_select.restype = C.c_int
        L.krep_gpu_mirror_select.argtypes = [C.POINTER(abi.SearchParams), C.c_size_t]
        L.krep_gpu_algorithm_name.restype = C.c_char_p
        L.krep_gpu_algorithm_name.argtypes = [C.c_int]
        L.krep_gpu_order_by_start.restype = C.c_int
        L.krep_gpu_order_by_start.argtypes = [C.c_void_p, C.c_uint64, C.c_size_t, C.c_void_p]
        L.krep_gpu_line_numbers.restype = C.c_int
        L.krep_gpu_line_numbers.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
        L.krep_gpu_line_numbers_ex.restype = C.c_int
        L.krep_gpu_line_numbers_ex.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
        if hasattr(L, "krep_gpu_debug_scan_exclusive"):  # (an older build of the library as an A/B partner lacks it)
            L.krep_gpu_debug_scan_exclusive.restype = C.c_int
            L.krep_gpu_debug_scan_exclusive.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_int, C.c_void_p]
        if hasattr(L, "krep_gpu_format_lines"):  # (an older build of the library as an A/B partner lacks them)
            L.krep_gpu_matching_lines.restype = C.c_int
            L.krep_gpu_matching_lines.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p,
                                                  C.c_uint64, C.POINTER(abi.LinesOut), C.c_void_p]
            L.krep_gpu_format_lines.restype = C.c_int
            L.krep_gpu_format_lines.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint64, C.c_uint64, C.c_char_p, C.c_size_t,
                                                C.c_void_p, C.c_size_t, C.POINTER(abi.LinesOut), C.c_void_p]
        if hasattr(L, "krep_gpu_format_lines_ex"):
            L.krep_gpu_format_lines_ex.restype = C.c_int
            L.krep_gpu_format_lines_ex.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(abi.LineFormat),
                                                   C.c_void_p, C.c_size_t, C.POINTER(abi.LinesOut), C.c_void_p]
        if hasattr(L, "krep_gpu_format_lines_window"):
            L.krep_gpu_format_lines_window.restype = C.c_int
            L.krep_gpu_format_lines_window.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(abi.LinesWindow), C.c_void_p, C.c_uint64,
                                                       C.c_uint64, C.POINTER(abi.LineFormat), C.c_void_p, C.c_size_t,
                                                       C.POINTER(abi.LinesWindowOut), C.c_void_p]
        if hasattr(L, "krep_gpu_format_matches"):
            L.krep_gpu_format_matches.restype = C.c_int
            L.krep_gpu_format_matches.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(abi.MatchFormat),
                                                  C.c_void_p, C.c_size_t, C.POINTER(abi.MatchesOut), C.c_void_p]
        if hasattr(L, "krep_gpu_format_matches_window"):
            L.krep_gpu_format_matches_window.restype = C.c_int
            L.krep_gpu_format_matches_window.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(abi.MatchesWindow), C.c_void_p, C.c_uint64,
                                                         C.c_uint64, C.POINTER(abi.MatchFormat), C.c_void_p, C.c_size_t,
                                                         C.POINTER(abi.MatchesWindowOut), C.c_void_p]
        for n in ("krep_gpu_set_reference_simd", "krep_gpu_set_only_matching", "krep_gpu_set_force_no_simd",
                  "krep_gpu_set_algo_override", "krep_gpu_debug_force_rounds", "krep_gpu_debug_force_stage_cap",
                  "krep_gpu_set_result_order", "krep_gpu_set_device", "krep_gpu_set_num_gpus", "krep_gpu_debug_inject_failure"):
            getattr(L, n).restype = None
            getattr(L, n).argtypes = [C.c_int]
        L.krep_gpu_get_reference_simd.restype = C.c_int
        L.krep_gpu_comm_unique_id.restype = C.c_int
        L.krep_gpu_comm_unique_id.argtypes = [C.c_void_p]
        L.krep_gpu_comm_init_rank.restype = C.c_int
        L.krep_gpu_comm_init_rank.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
        L.krep_gpu_comm_allreduce_u64.restype = C.c_int
        L.krep_gpu_comm_allreduce_u64.argtypes = [C.POINTER(C.c_uint64), C.c_int]
        L.krep_gpu_comm_allreduce_device_u64.restype = C.c_int
        L.krep_gpu_comm_allreduce_device_u64.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.krep_gpu_comm_destroy.restype = None
        L.krep_gpu_rccl_calls.restype = C.c_uint64
        L.krep_gpu_rccl_version.restype = C.c_int
        L.krep_gpu_debug_force_single_grid.restype = None
        L.krep_gpu_debug_force_single_grid.argtypes = [C.c_int]
        L.krep_gpu_debug_single_failovers.restype = C.c_uint64
        L.krep_gpu_debug_single_launches.restype = C.c_uint64
        L.krep_gpu_debug_tiny_launches.restype = C.c_uint64
        L.krep_gpu_debug_chain_fixups.restype = None
        L.krep_gpu_debug_chain_fixups.argtypes = [C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.krep_gpu_debug_tiny_dense_launches.restype = C.c_uint64
        if hasattr(L, "krep_gpu_debug_anchor_info"):  # (an older build of the library as an A/B partner, tools/ab_bench.py, lacks the round-6 hooks)
            L.krep_gpu_debug_anchored_launches.restype = C.c_uint64
            L.krep_gpu_debug_literal_dma_launches.restype = C.c_uint64
            L.krep_gpu_debug_runs_launches.restype = C.c_uint64
            L.krep_gpu_debug_anchor_info.restype = C.c_int
            L.krep_gpu_debug_anchor_info.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_uint32), C.POINTER(C.c_double),
                                                     C.POINTER(C.c_double)]
        if hasattr(L, "krep_gpu_debug_literal_dma_one_pass_launches"):
            L.krep_gpu_debug_literal_dma_one_pass_launches.restype = C.c_uint64
            L.krep_gpu_debug_literal_dma_one_pass_failovers.restype = C.c_uint64
            L.krep_gpu_debug_force_literal_dma_grid.restype = None
            L.krep_gpu_debug_force_literal_dma_grid.argtypes = [C.c_int]
        if hasattr(L, "krep_gpu_debug_force_literal_dma_tickets"):
            L.krep_gpu_debug_force_literal_dma_tickets.restype = None
            L.krep_gpu_debug_force_literal_dma_tickets.argtypes = [C.c_int, C.c_uint64]
            L.krep_gpu_debug_literal_dma_last_tickets.restype = None
            L.krep_gpu_debug_literal_dma_last_tickets.argtypes = [C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
            L.krep_gpu_debug_ticket_map.restype = C.c_int
            L.krep_gpu_debug_ticket_map.argtypes = [C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64),
                                                    C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
            L.krep_gpu_debug_ticket_map_long_tickets.restype = C.c_uint64
            L.krep_gpu_debug_ticket_map_long_tickets.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint64]
        if hasattr(L, "krep_gpu_regex_compile_loops"):  # (likewise)
            L.krep_gpu_regex_compile_loops.restype = C.c_int
            L.krep_gpu_regex_compile_loops.argtypes = [C.POINTER(abi.SearchParams), C.POINTER(abi.RegexLoops)]
            L.krep_gpu_set_regex_loops.restype = None
            L.krep_gpu_set_regex_loops.argtypes = [C.c_int]
            L.krep_gpu_get_regex_loops.restype = C.c_int
            L.krep_gpu_get_regex_loops.argtypes = []
            L.krep_gpu_debug_force_regex_loops_road.restype = None
            L.krep_gpu_debug_force_regex_loops_road.argtypes = [C.c_int]
            L.krep_gpu_debug_regex_loops_roads.restype = None
            L.krep_gpu_debug_regex_loops_roads.argtypes = [C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        if hasattr(L, "krep_gpu_regex_compile_groups"):  # (likewise)
            L.krep_gpu_regex_compile_groups.restype = C.c_int
            L.krep_gpu_regex_compile_groups.argtypes = [C.POINTER(abi.SearchParams), C.POINTER(abi.RegexGroups)]
            L.krep_gpu_set_regex_groups.restype = None
            L.krep_gpu_set_regex_groups.argtypes = [C.c_int]
            L.krep_gpu_get_regex_groups.restype = C.c_int
            L.krep_gpu_get_regex_groups.argtypes = []
            L.krep_gpu_debug_force_regex_general.restype = None
            L.krep_gpu_debug_force_regex_general.argtypes = [C.c_int]
            L.krep_gpu_debug_regex_general_walks.restype = C.c_uint64
            L.krep_gpu_debug_regex_general_walks.argtypes = []
        if hasattr(L, "krep_gpu_set_regex_loops_windows"):  # (likewise)
            L.krep_gpu_set_regex_loops_windows.restype = None
            L.krep_gpu_set_regex_loops_windows.argtypes = [C.c_int]
            L.krep_gpu_get_regex_loops_windows.restype = C.c_int
            L.krep_gpu_get_regex_loops_windows.argtypes = []
        if hasattr(L, "krep_gpu_set_regex_long_lines"):  # (likewise)
            L.krep_gpu_set_regex_long_lines.restype = None
            L.krep_gpu_set_regex_long_lines.argtypes = [C.c_int]
            L.krep_gpu_get_regex_long_lines.restype = C.c_int
            L.krep_gpu_get_regex_long_lines.argtypes = []
            L.krep_gpu_debug_set_regex_long_budget.restype = None
            L.krep_gpu_debug_set_regex_long_budget.argtypes = [C.c_uint64]
            L.krep_gpu_debug_regex_long_walks.restype = C.c_uint64
            L.krep_gpu_debug_regex_long_walks.argtypes = []
        if hasattr(L, "krep_gpu_debug_force_regex_grid"):
            L.krep_gpu_debug_force_regex_grid.restype = None
            L.krep_gpu_debug_force_regex_grid.argtypes = [C.c_int]
        if hasattr(L, "krep_gpu_search_batch"):  # (an older build loaded as an A/B partner lacks it: tools/ab_bench.py)
            L.krep_gpu_batch_can_accelerate.restype = C.c_int
            L.krep_gpu_batch_can_accelerate.argtypes = [C.POINTER(abi.SearchParams)]
            L.krep_gpu_search_batch.restype = C.c_int
            L.krep_gpu_search_batch.argtypes = [C.POINTER(abi.SearchParams), C.POINTER(abi.Config), C.POINTER(abi.BatchItem), C.c_size_t,
                                                C.POINTER(abi.BatchResult), C.POINTER(abi.MatchResult), C.POINTER(abi.BatchInfo)]
            L.krep_gpu_debug_batch_pack_limit.restype = None
            L.krep_gpu_debug_batch_pack_limit.argtypes = [C.c_size_t]
            L.krep_gpu_debug_batch_times.restype = None
            L.krep_gpu_debug_batch_times.argtypes = [C.POINTER(C.c_double)] * 4
        if hasattr(L, "krep_gpu_debug_batch_fill_host"):  # (likewise)
            L.krep_gpu_debug_batch_fill_host.restype = C.c_int
            L.krep_gpu_debug_batch_fill_host.argtypes = [C.POINTER(abi.BatchItem), C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p]
            L.krep_gpu_debug_batch_rebase_launches.restype = None
            L.krep_gpu_debug_batch_rebase_launches.argtypes = [C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        if hasattr(L, "krep_gpu_set_batch_max_count"):  # (likewise)
            L.krep_gpu_set_batch_max_count.restype = None
            L.krep_gpu_set_batch_max_count.argtypes = [C.c_int]
            L.krep_gpu_get_batch_max_count.restype = C.c_int
            L.krep_gpu_get_batch_max_count.argtypes = []
            L.krep_gpu_debug_batch_cut_launches.restype = None
            L.krep_gpu_debug_batch_cut_launches.argtypes = [C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        if hasattr(L, "krep_gpu_grep_batch"):  # (likewise)
            L.krep_gpu_format_lines_items.restype = C.c_int
            L.krep_gpu_format_lines_items.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(abi.PackView), C.c_void_p, C.c_uint64,
                                                      C.POINTER(abi.LineFormat), C.c_void_p, C.c_size_t, C.c_void_p,
                                                      C.POINTER(abi.LinesOut), C.c_void_p]
            L.krep_gpu_format_matches_items.restype = C.c_int
            L.krep_gpu_format_matches_items.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(abi.PackView), C.c_void_p, C.c_uint64,
                                                        C.POINTER(abi.MatchFormat), C.c_void_p, C.c_size_t, C.c_void_p,
                                                        C.POINTER(abi.MatchesOut), C.c_void_p]
            L.krep_gpu_grep_batch.restype = C.c_int
            L.krep_gpu_grep_batch.argtypes = [C.POINTER(abi.SearchParams), C.POINTER(abi.Config), C.POINTER(abi.BatchItem), C.c_size_t,
                                              C.POINTER(abi.GrepFormat), C.POINTER(abi.GrepItem), C.POINTER(abi.GrepOutput),
                                              C.POINTER(abi.BatchInfo)]
            L.krep_gpu_debug_grep_batch_times.restype = None
            L.krep_gpu_debug_grep_batch_times.argtypes = [C.POINTER(C.c_double)] * 5
            L.krep_gpu_debug_batch_format_launches.restype = None
            L.krep_gpu_debug_batch_format_launches.argtypes = [C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        if hasattr(L, "krep_gpu_alloc_placed"):
            L.krep_gpu_alloc_placed.restype = C.c_int
            L.krep_gpu_alloc_placed.argtypes = [C.c_int, C.c_size_t, C.c_size_t, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                                C.POINTER(abi.Placement)]
            L.krep_gpu_free_placed.restype = C.c_int
            L.krep_gpu_free_placed.argtypes = [C.c_int, C.c_void_p]
        if hasattr(L, "krep_gpu_debug_literal_dma_state"):
            L.krep_gpu_debug_literal_dma_state.restype = C.c_int
            L.krep_gpu_debug_literal_dma_state.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_double)]
        if hasattr(L, "krep_gpu_debug_anchor_measured"):
            L.krep_gpu_debug_anchor_measured.restype = C.c_int
            L.krep_gpu_debug_anchor_measured.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int)]
        if hasattr(L, "krep_gpu_debug_ac_last_scan"):
            L.krep_gpu_debug_ac_last_scan.restype = C.c_int
            L.krep_gpu_debug_ac_last_scan.argtypes = [C.c_void_p, C.c_int, C.POINTER(abi.AcScan)]
        L.krep_gpu_last_shard_info.restype = None
        L.krep_gpu_last_shard_info.argtypes = [C.POINTER(abi.ShardInfo)]
        L.krep_gpu_available.restype = C.c_int
        L.krep_gpu_unavailable_reason.restype = C.c_char_p
        L.krep_gpu_last_status.restype = C.c_int
        L.krep_gpu_set_cpu_fallback.restype = None
        L.krep_gpu_set_cpu_fallback.argtypes = [C.c_void_p]
        L.krep_gpu_worthwhile.restype = C.c_int
        L.krep_gpu_worthwhile.argtypes = [C.POINTER(abi.SearchParams), C.c_size_t]
        L.krep_gpu_worthwhile_ex.restype = C.c_int
        L.krep_gpu_worthwhile_ex.argtypes = [C.POINTER(abi.SearchParams), C.c_size_t, C.c_int]
        L.krep_gpu_cost_estimate.restype = C.c_int
        L.krep_gpu_cost_estimate.argtypes = [C.POINTER(abi.SearchParams), C.c_size_t, C.c_int, C.POINTER(abi.Cost)]
        L.krep_gpu_get_cost_rates.restype = None
        L.krep_gpu_get_cost_rates.argtypes = [C.POINTER(abi.CostRates)]
        L.krep_gpu_set_cost_rates.restype = None
        L.krep_gpu_set_cost_rates.argtypes = [C.POINTER(abi.CostRates)]
        L.krep_gpu_set_min_text_bytes.restype = None
        L.krep_gpu_set_min_text_bytes.argtypes = [C.c_size_t]
        L.krep_gpu_device_count.restype = C.c_int
        L.krep_gpu_last_error.restype = C.c_char_p
        L.krep_gpu_clear_error.restype = None
        L.krep_gpu_version.restype = C.c_char_p

    # ---- configuration of the reference mirror ----
    def set_reference_simd(self, level: int):
        self.lib.krep_gpu_set_reference_simd(level)

    def set_only_matching(self, on: bool):
        self.lib.krep_gpu_set_only_matching(int(on))

    def set_force_no_simd(self, on: bool):
        self.lib.krep_gpu_set_force_no_simd(int(on))

    def set_algo_override(self, a: int):
        self.lib.krep_gpu_set_algo_override(a)

    def force_rounds(self, r: int):
        self.lib.krep_gpu_debug_force_rounds(r)

    def force_single_grid(self, blocks: int):
        self.lib.krep_gpu_debug_force_single_grid(blocks)

    def single_failovers(self) -> int:
        return int(self.lib.krep_gpu_debug_single_failovers())

    def single_launches(self) -> int:
        return int(self.lib.krep_gpu_debug_single_launches())

    def chain_fixups(self):
        """(pieces scanned again, end pieces that only re-ran the end-of-text replay) since the process started"""
        a, b = C.c_uint64(0), C.c_uint64(0)
        self.lib.krep_gpu_debug_chain_fixups(C.byref(a), C.byref(b))
        return int(a.value), int(b.value)

    def tiny_dense_launches(self) -> int:
        return int(self.lib.krep_gpu_debug_tiny_dense_launches())

    def runs_launches(self) -> int:
        return int(self.lib.krep_gpu_debug_runs_launches())

    def literal_dma_launches(self) -> int:
        return int(self.lib.krep_gpu_debug_literal_dma_launches())

    def literal_dma_one_pass_launches(self) -> int:
        """launches of the LDS-DMA literal kernel in its one-pass records mode (no ordering post-pass)"""
        return int(self.lib.krep_gpu_debug_literal_dma_one_pass_launches())

    def literal_dma_one_pass_failovers(self) -> int:
        return int(self.lib.krep_gpu_debug_literal_dma_one_pass_failovers())

    def force_literal_dma_grid(self, blocks: int):
        self.lib.krep_gpu_debug_force_literal_dma_grid(blocks)

    def force_literal_dma_tickets(self, long_units: int, n_long: int = 0):
        """the one-pass mode's ticket map forced: the first n_long tickets take long_units (8, 16, 32) units, the rest 8; 0 = the library's choice"""
        self.lib.krep_gpu_debug_force_literal_dma_tickets(long_units, n_long)

    def literal_dma_last_tickets(self):
        """(units of a long ticket, number of long tickets) of the last one-pass launch; (8, 0): every ticket short"""
        u, k = C.c_uint32(0), C.c_uint64(0)
        self.lib.krep_gpu_debug_literal_dma_last_tickets(C.byref(u), C.byref(k))
        return int(u.value), int(k.value)

    def ticket_map(self, upt_long: int, upt: int, n_long: int, n_units: int, ticket: int):
        """(first unit, units) of `ticket` and the number of tickets under the map {upt_long, upt, n_long} (kg_tickets.h); None: refused"""
        f, c, k = C.c_uint64(0), C.c_uint32(0), C.c_uint64(0)
        if self.lib.krep_gpu_debug_ticket_map(upt_long, upt, n_long, n_units, ticket, C.byref(f), C.byref(c), C.byref(k)):
            return None
        return int(f.value), int(c.value), int(k.value)

    def ticket_map_long_tickets(self, n_units: int, upt_long: int, upt: int, waves: int) -> int:
        return int(self.lib.krep_gpu_debug_ticket_map_long_tickets(n_units, upt_long, upt, waves))

    def force_regex_grid(self, blocks: int):
        """at most `blocks` workgroups for the regex scan (0 = auto): every wave then takes several 32-KiB units"""
        self.lib.krep_gpu_debug_force_regex_grid(blocks)

    def alloc_placed(self, text_bytes: int, record_bytes: int, tries: int = 3, device: int = 0):
        """krep_gpu_alloc_placed(): (d_text, d_records, abi.Placement) — one block, its placement drawn for; free_placed(d_text)"""
        t, r, info = C.c_void_p(0), C.c_void_p(0), abi.Placement()
        if self.lib.krep_gpu_alloc_placed(device, text_bytes, record_bytes, tries, C.byref(t), C.byref(r), C.byref(info)):
            raise KrepGpuError("krep_gpu_alloc_placed failed: " + self.last_error())
        return int(t.value), int(r.value or 0), info

    def free_placed(self, d_text: int, device: int = 0):
        if self.lib.krep_gpu_free_placed(device, C.c_void_p(d_text)):
            raise KrepGpuError("krep_gpu_free_placed failed: " + self.last_error())

    def anchored_launches(self) -> int:
        return int(self.lib.krep_gpu_debug_anchored_launches())

    def tiny_launches(self) -> int:
        return int(self.lib.krep_gpu_debug_tiny_launches())

    def force_stage_cap(self, c: int):
        self.lib.krep_gpu_debug_force_stage_cap(c)

    def default_config(self) -> abi.Config:
        c = abi.Config()
        self.lib.krep_gpu_config_default(C.byref(c))
        return c

    def set_thread_config(self, cfg: "abi.Config | None"):
        self.lib.krep_gpu_set_thread_config(C.byref(cfg) if cfg is not None else None)

    def set_stream_chunk(self, nbytes: int):
        self.lib.krep_gpu_set_stream_chunk(nbytes)

    def regex_compile(self, params: abi.Params) -> "abi.RegexInfo":
        """krep_gpu_regex_compile: the byte classes of an -E pattern (host only); KrepGpuError with the reason when it is refused.
        Python puts the process into the environment's locale at start-up; in a multibyte one (UTF-8) libc matches characters, not
        bytes, and every pattern is refused: locale.setlocale(locale.LC_CTYPE, "C") is the locale krep itself runs in."""
        info = abi.RegexInfo()
        if self.lib.krep_gpu_regex_compile(params.ref, C.byref(info)):
            raise KrepGpuError(self.last_error())
        return info

    def regex_compile_anchored(self, params: abi.Params) -> "abi.RegexAnchored":
        """krep_gpu_regex_compile_anchored: the same with a ^ in front and a $ behind taken as line anchors (bol / eol; seq holds the
        real classes).  This is the compiler every search goes through; regex_compile() keeps refusing both anchors."""
        info = abi.RegexAnchored()
        if self.lib.krep_gpu_regex_compile_anchored(params.ref, C.byref(info)):
            raise KrepGpuError(self.last_error())
        return info

    def regex_compile_alt(self, params: abi.Params) -> "abi.RegexAlt":
        """krep_gpu_regex_compile_alt: an alternation of class sequences (a|b, (a)|(b), several patterns): its merged branches, each
        what regex_compile() makes of the branch alone, and cross_overlap.  Every search asks regex_compile_anchored() first and this
        compiler only for what that one refuses."""
        info = abi.RegexAlt()
        if self.lib.krep_gpu_regex_compile_alt(params.ref, C.byref(info)):
            raise KrepGpuError(self.last_error())
        return info

    def regex_compile_ext(self, params: abi.Params) -> "abi.RegexExt":
        """krep_gpu_regex_compile_ext: ?, {n}, {n,m}, inner groups and a ^ / $ around every top-level branch, expanded into up to 8
        class sequences (alt, over the real classes) between the line anchors bol / eol.  Every search asks regex_compile_anchored()
        first, then regex_compile_alt(), then this compiler."""
        info = abi.RegexExt()
        if self.lib.krep_gpu_regex_compile_ext(params.ref, C.byref(info)):
            raise KrepGpuError(self.last_error())
        return info

    def regex_compile_loops(self, params: abi.Params) -> "abi.RegexLoops":
        """krep_gpu_regex_compile_loops: the expanding compiler's grammar with *, + and {n,} behind an atom: sequences of places of which
        some repeat (alt, repeat[i] the mask of branch i), the line anchors, and the filter (the fixed-length factors the candidate
        lines are found with).  It always works; a search asks it, last, only after set_regex_loops(True)."""
        info = abi.RegexLoops()
        if self.lib.krep_gpu_regex_compile_loops(params.ref, C.byref(info)):
            raise KrepGpuError(self.last_error())
        return info

    def regex_compile_groups(self, params: abi.Params) -> dict:
        """krep_gpu_regex_compile_groups: repeated and nested groups ((ab)+, ((GET|POST) |HEAD )/api, [0-9]{1,3}\\.[0-9]{1,3}...) held
        unexpanded as a position automaton.  Returned as Python values: n_pos; classes (a list of bytes objects, one per position);
        first and last (sets of positions); follow (a list of sets); bol, eol; filter (a list of class sequences, each a list of bytes
        objects: every match holds an occurrence of one of them as consecutive bytes); and raw, the abi.RegexGroups itself.  It always
        works; a search asks it, fifth, only after set_regex_groups(True)."""
        info = abi.RegexGroups()
        if self.lib.krep_gpu_regex_compile_groups(params.ref, C.byref(info)):
            raise KrepGpuError(self.last_error())
        n = int(info.n_pos)
        bits = lambda m: {i for i in range(32) if (int(m) >> i) & 1}  # noqa: E731
        return {"n_pos": n, "classes": [info.class_bytes(i) for i in range(n)], "first": bits(info.first), "last": bits(info.last),
                "follow": [bits(info.follow[i]) for i in range(n)], "bol": bool(info.bol), "eol": bool(info.eol),
                "filter": [[br.class_bytes(j) for j in range(int(br.L))] for br in info.filter.branch[: int(info.filter.n_branches)]],
                "raw": info}

    def set_regex_groups(self, on: bool):
        """krep_gpu_set_regex_groups: whether a search asks the groups compiler after the four older ones have refused (process-wide,
        off by default, $KREP_GPU_REGEX_GROUPS=1 at load; independent of set_regex_loops)"""
        self.lib.krep_gpu_set_regex_groups(1 if on else 0)

    def get_regex_groups(self) -> bool:
        return bool(self.lib.krep_gpu_get_regex_groups())

    def force_regex_general(self, on: bool):
        """test hook: with both switches on, a plan made while this is on walks a loops-compiler expression by the general step"""
        self.lib.krep_gpu_debug_force_regex_general(1 if on else 0)

    def regex_general_walks(self) -> int:
        """launches of the line walk's general step since the process started"""
        return int(self.lib.krep_gpu_debug_regex_general_walks())

    def set_regex_loops(self, on: bool):
        """krep_gpu_set_regex_loops: whether a search asks the loops compiler after the three older ones have refused (process-wide,
        off by default, $KREP_GPU_REGEX_LOOPS=1 at load)"""
        self.lib.krep_gpu_set_regex_loops(1 if on else 0)

    def get_regex_loops(self) -> bool:
        return bool(self.lib.krep_gpu_get_regex_loops())

    def set_regex_loops_windows(self, on: bool):
        """krep_gpu_set_regex_loops_windows: whether a search the loops compiler took may be cut into windows (split_mode() PIECES,
        4096 bytes of context on both sides of what a window owns) instead of taking the whole text in one (process-wide, off by
        default, $KREP_GPU_REGEX_LOOPS_WINDOWS=1 at load)"""
        self.lib.krep_gpu_set_regex_loops_windows(1 if on else 0)

    def get_regex_loops_windows(self) -> bool:
        return bool(self.lib.krep_gpu_get_regex_loops_windows())

    def set_regex_long_lines(self, on: bool):
        """krep_gpu_set_regex_long_lines: whether the one-window scan of a search the loops or the groups compiler took walks a
        candidate line of more than 4096 bytes (two linear passes, kg_regex_loops.hip) instead of refusing the text (process-wide, off
        by default, $KREP_GPU_REGEX_LONG_LINES=1 at load)"""
        self.lib.krep_gpu_set_regex_long_lines(1 if on else 0)

    def get_regex_long_lines(self) -> bool:
        return bool(self.lib.krep_gpu_get_regex_long_lines())

    def set_regex_long_budget(self, nbytes: int):
        """test hook: the bytes of scratch words a round of long lines may hold (0: the default); the cap of one line is
        min(1 MiB, nbytes / 4)"""
        self.lib.krep_gpu_debug_set_regex_long_budget(int(nbytes))

    def regex_long_walks(self) -> int:
        """launches of the long-line walk since the process started"""
        return int(self.lib.krep_gpu_debug_regex_long_walks())

    def force_regex_loops_road(self, road: int):
        """which road the loops scan finds its candidate lines by: 0 its own choice, 1 sparse (the filter's records), 2 dense (all lines)"""
        self.lib.krep_gpu_debug_force_regex_loops_road(int(road))

    def regex_loops_roads(self):
        """(sparse, dense): loops scans that took each road since the process started"""
        a, b = C.c_uint64(0), C.c_uint64(0)
        self.lib.krep_gpu_debug_regex_loops_roads(C.byref(a), C.byref(b))
        return int(a.value), int(b.value)

    def can_accelerate(self, params: abi.Params) -> bool:
        return bool(self.lib.krep_gpu_can_accelerate(params.ref))

    def select(self, params: abi.Params):
        """krep_gpu_select_search_algorithm(): the operator's address, or None (the caller keeps its CPU function)."""
        return self.lib.krep_gpu_select_search_algorithm(params.ref)

    # ---- availability, failure status, CPU fallback (SURVEY §8b "Errors") ----
    def available(self) -> bool:
        return bool(self.lib.krep_gpu_available())

    def unavailable_reason(self) -> str:
        return (self.lib.krep_gpu_unavailable_reason() or b"").decode()

    def last_status(self) -> int:
        return int(self.lib.krep_gpu_last_status())

    def set_cpu_fallback(self, selector_address):
        """selector_address: address of a `search_func_t (*)(const search_params_t *)` (or None to unregister)."""
        self.lib.krep_gpu_set_cpu_fallback(C.c_void_p(selector_address) if selector_address else None)

    def worthwhile(self, params: abi.Params, text_len: int) -> bool:
        return bool(self.lib.krep_gpu_worthwhile(params.ref, text_len))

    def worthwhile_ex(self, params: abi.Params, text_len: int, cpu_threads: int) -> bool:
        return bool(self.lib.krep_gpu_worthwhile_ex(params.ref, text_len, cpu_threads))

    def cost_estimate(self, params: abi.Params, text_len: int, cpu_threads: int = 0) -> "abi.Cost":
        c = abi.Cost()
        if self.lib.krep_gpu_cost_estimate(params.ref, text_len, cpu_threads, C.byref(c)):
            raise KrepGpuError("krep_gpu_cost_estimate failed")
        return c

    def cost_rates(self) -> "abi.CostRates":
        r = abi.CostRates()
        self.lib.krep_gpu_get_cost_rates(C.byref(r))
        return r

    def set_cost_rates(self, rates: "abi.CostRates | None"):
        self.lib.krep_gpu_set_cost_rates(C.byref(rates) if rates is not None else None)

    def inject_failure(self, kind: int):
        self.lib.krep_gpu_debug_inject_failure(kind)

    def set_num_gpus(self, n: int):
        self.lib.krep_gpu_set_num_gpus(n)

    # ---- the collective of the multi-GPU path, C level (kg_comm.hip: RCCL, dlopen'd on first use) ----
    def comm_unique_id(self) -> bytes:
        buf = C.create_string_buffer(128)
        if self.lib.krep_gpu_comm_unique_id(buf):
            raise KrepGpuError("krep_gpu_comm_unique_id failed: " + self.last_error())
        return buf.raw

    def comm_init_rank(self, id128: bytes, nranks: int, rank: int, device: int):
        assert len(id128) == 128
        buf = C.create_string_buffer(id128, 128)
        if self.lib.krep_gpu_comm_init_rank(buf, nranks, rank, device):
            raise KrepGpuError("krep_gpu_comm_init_rank failed: " + self.last_error())

    def comm_allreduce(self, values):
        """ONE ncclAllReduce(uint64, sum) of the rank's counters; returns the summed values."""
        arr = (C.c_uint64 * len(values))(*[int(v) for v in values])
        if self.lib.krep_gpu_comm_allreduce_u64(arr, len(values)):
            raise KrepGpuError("krep_gpu_comm_allreduce_u64 failed: " + self.last_error())
        return [int(v) for v in arr]

    def comm_destroy(self):
        self.lib.krep_gpu_comm_destroy()

    def rccl_calls(self) -> int:
        return int(self.lib.krep_gpu_rccl_calls())

    def rccl_version(self) -> int:
        return int(self.lib.krep_gpu_rccl_version())

    def last_shard_info(self) -> "abi.ShardInfo":
        """Shards / physical devices / communicator ranks of the calling thread's last sharded host search."""
        info = abi.ShardInfo()
        self.lib.krep_gpu_last_shard_info(C.byref(info))
        return info

    def split_mode(self, params: abi.Params, text_len: int) -> int:
        return int(self.lib.krep_gpu_split_mode(params.ref, text_len))

    def release_device_resources(self):
        self.lib.krep_gpu_release_device_resources()

    def mirror_select(self, params: abi.Params, text_len: int) -> int:
        return int(self.lib.krep_gpu_mirror_select(params.ref, text_len))

    def last_error(self) -> str:
        return (self.lib.krep_gpu_last_error() or b"").decode()

    def device_count(self) -> int:
        return int(self.lib.krep_gpu_device_count())

    # ---- formatter-side post-processing on the device (krep.c:3018-3023, :589-668) ----
    def set_result_order(self, by_start: bool):
        self.lib.krep_gpu_set_result_order(int(by_start))

    def order_by_start(self, d_positions: int, n: int, text_len: int, stream: int = 0):
        if self.lib.krep_gpu_order_by_start(C.c_void_p(d_positions), n, text_len, C.c_void_p(stream)):
            raise KrepGpuError("krep_gpu_order_by_start failed: " + self.last_error())

    def line_numbers(self, d_text: int, text_len: int, d_positions: int, n: int, d_lines: int, stream: int = 0, global_base: int = 0):
        """krep_gpu_line_numbers_ex(): the text_len bytes at d_text are text[global_base:], the records carry global offsets; the line
        numbers count from the buffer's first byte, and a record that starts outside the buffer gets 0"""
        if self.lib.krep_gpu_line_numbers_ex(C.c_void_p(d_text), text_len, global_base, C.c_void_p(d_positions), n, C.c_void_p(d_lines),
                                             C.c_void_p(stream)):
            raise KrepGpuError("krep_gpu_line_numbers_ex failed: " + self.last_error())

    def scan_exclusive(self, d_in: int, n: int, d_out: int, take_max: bool = False, stream: int = 0):
        """test hook: the formatters' exclusive prefix scan of n 64-bit device words (the sum mod 2^64, or the running maximum), d_in
        into d_out, a buffer of its own"""
        if self.lib.krep_gpu_debug_scan_exclusive(C.c_void_p(d_in) if d_in else None, n, C.c_void_p(d_out) if d_out else None,
                                                  int(bool(take_max)), C.c_void_p(stream) if stream else None):
            raise KrepGpuError("krep_gpu_debug_scan_exclusive failed: " + self.last_error())

    # ---- the matching lines themselves (print_matching_items(), full-line mode without colour, krep.c:797-1071) ----
    def matching_lines(self, d_text: int, text_len: int, d_positions: int, n: int, max_lines: int = abi.SIZE_MAX, d_lines: int = 0,
                       d_first_record: int = 0, line_capacity: int = 0, stream: int = 0) -> "abi.LinesOut":
        """krep_gpu_matching_lines(): {line_start, line_end} and first record of every distinct line the records (in (start, end)
        order) start on.  d_lines = 0 asks for the sizes; a capacity that is too small comes back as .overflow."""
        out = abi.LinesOut()
        if self.lib.krep_gpu_matching_lines(C.c_void_p(d_text), text_len, C.c_void_p(d_positions), n, max_lines,
                                            C.c_void_p(d_lines) if d_lines else None,
                                            C.c_void_p(d_first_record) if d_first_record else None, line_capacity, C.byref(out),
                                            C.c_void_p(stream) if stream else None):
            raise KrepGpuError("krep_gpu_matching_lines failed: " + self.last_error())
        return out

    def format_lines(self, d_text: int, text_len: int, d_positions: int, n: int, max_lines: int = abi.SIZE_MAX, prefix: bytes = b"",
                     d_out: int = 0, out_capacity: int = 0, stream: int = 0) -> "abi.LinesOut":
        """krep_gpu_format_lines(): the bytes the reference prints for these records, into d_out.  d_out = 0 asks for .out_bytes."""
        out = abi.LinesOut()
        if self.lib.krep_gpu_format_lines(C.c_void_p(d_text), text_len, C.c_void_p(d_positions), n, max_lines, prefix, len(prefix),
                                          C.c_void_p(d_out) if d_out else None, out_capacity, C.byref(out),
                                          C.c_void_p(stream) if stream else None):
            raise KrepGpuError("krep_gpu_format_lines failed: " + self.last_error())
        return out

    def format_lines_ex(self, d_text: int, text_len: int, d_positions: int, n: int, max_lines: int = abi.SIZE_MAX,
                        fmt: "abi.LineFormat | None" = None, d_out: int = 0, out_capacity: int = 0, stream: int = 0) -> "abi.LinesOut":
        """krep_gpu_format_lines_ex(): the same lines with the caller's strings in them (--color=always), into d_out.  fmt: prefix,
        before_match, after_match, line_close (None: none).  d_out = 0 asks for .out_bytes."""
        out = abi.LinesOut()
        if self.lib.krep_gpu_format_lines_ex(C.c_void_p(d_text), text_len, C.c_void_p(d_positions), n, max_lines,
                                             C.byref(fmt) if fmt is not None else None, C.c_void_p(d_out) if d_out else None,
                                             out_capacity, C.byref(out), C.c_void_p(stream) if stream else None):
            raise KrepGpuError("krep_gpu_format_lines_ex failed: " + self.last_error())
        return out

    def format_lines_window(self, d_text: int, text_len: int, win: "abi.LinesWindow", d_positions: int, n: int,
                            max_lines: int = abi.SIZE_MAX, fmt: "abi.LineFormat | None" = None, d_out: int = 0, out_capacity: int = 0,
                            stream: int = 0) -> "abi.LinesWindowOut":
        """krep_gpu_format_lines_window(): format_lines_ex for a WINDOW of a text.  The text_len bytes at d_text are
        text[win.global_base:], the records carry global offsets, the call emits the lines that start in [win.own_lo, win.own_hi)
        and are complete in front of win.records_hi, and reports the one that is not (.incomplete_line_start1)."""
        out = abi.LinesWindowOut()
        if self.lib.krep_gpu_format_lines_window(C.c_void_p(d_text), text_len, C.byref(win), C.c_void_p(d_positions), n, max_lines,
                                                 C.byref(fmt) if fmt is not None else None, C.c_void_p(d_out) if d_out else None,
                                                 out_capacity, C.byref(out), C.c_void_p(stream) if stream else None):
            raise KrepGpuError("krep_gpu_format_lines_window failed: " + self.last_error())
        return out

    # ---- the matches themselves, one per line (print_matching_items(), only-matching mode, krep.c:517-793) ----
    def format_matches(self, d_text: int, text_len: int, d_positions: int, n: int, max_items: int = abi.SIZE_MAX,
                       fmt: "abi.MatchFormat | None" = None, d_out: int = 0, out_capacity: int = 0, stream: int = 0) -> "abi.MatchesOut":
        """krep_gpu_format_matches(): the bytes the reference prints under -o for these records, into d_out.  fmt: the strings around
        LINE and the match (None: none).  d_out = 0 asks for .out_bytes; a capacity that is too small comes back as .overflow."""
        out = abi.MatchesOut()
        if self.lib.krep_gpu_format_matches(C.c_void_p(d_text), text_len, C.c_void_p(d_positions), n, max_items,
                                            C.byref(fmt) if fmt is not None else None, C.c_void_p(d_out) if d_out else None,
                                            out_capacity, C.byref(out), C.c_void_p(stream) if stream else None):
            raise KrepGpuError("krep_gpu_format_matches failed: " + self.last_error())
        return out

    def format_matches_window(self, d_text: int, text_len: int, win: "abi.MatchesWindow", d_positions: int, n: int,
                              max_items: int = abi.SIZE_MAX, fmt: "abi.MatchFormat | None" = None, d_out: int = 0, capacity: int = 0,
                              stream: int = 0) -> "abi.MatchesWindowOut":
        """krep_gpu_format_matches_window(): format_matches for a WINDOW of a text.  The text_len bytes at d_text are
        text[win.global_base:], the n records (global offsets) are a consecutive run of the text's list; win carries the newlines in
        front of the buffer and the stale line number in, the result carries them out (.newlines_before_count_to, .stale_line)."""
        out = abi.MatchesWindowOut()
        if self.lib.krep_gpu_format_matches_window(C.c_void_p(d_text) if d_text else None, text_len, C.byref(win),
                                                   C.c_void_p(d_positions) if d_positions else None, n, max_items,
                                                   C.byref(fmt) if fmt is not None else None, C.c_void_p(d_out) if d_out else None,
                                                   capacity, C.byref(out), C.c_void_p(stream) if stream else None):
            raise KrepGpuError("krep_gpu_format_matches_window failed: " + self.last_error())
        return out

    # ---- search_func_t-shaped operators on host buffers ----
    def _ptr(self, text):
        if isinstance(text, np.ndarray):
            assert text.dtype == np.uint8 and text.flags["C_CONTIGUOUS"]
            return C.c_void_p(text.ctypes.data), text.size, text
        raw = bytes(text)
        cp = C.c_char_p(raw)
        return C.cast(cp, C.c_void_p), len(raw), (raw, cp)

    def search(self, params: abi.Params, text, want_result=True):
        """krep_gpu_select_search_algorithm(params)(params, text, len, result) -> (ret, positions).  A regex search (use_regex) is
        taken in the C locale only: see regex_compile()."""
        ptr, n, keep = self._ptr(text)
        fn = (self.lib.krep_gpu_regex_search if params.s.use_regex else
              self.lib.krep_gpu_aho_corasick_search if params.s.num_patterns > 1 else self.lib.krep_gpu_literal_search)
        res = self.lib.krep_gpu_match_result_init(16) if want_result else None
        try:
            with _borrowed_trie(params):
                self.lib.krep_gpu_clear_error()
                ret = fn(params.ref, ptr, n, res)
            if self.last_status() == abi.STATUS_FAILED:
                raise KrepGpuError(self.last_error() or "krep-gpu operator failed")
            pos = abi.result_positions(res) if res else None
        finally:
            if res:
                self.lib.krep_gpu_match_result_free(res)
        del keep
        return int(ret), pos

    # ---- a batch of texts in one scan (krep -r) ----
    def batch_can_accelerate(self, params: abi.Params) -> bool:
        """krep_gpu_batch_can_accelerate(): is the search newline-separable (and taken at all); last_error() says why not."""
        return bool(self.lib.krep_gpu_batch_can_accelerate(params.ref))

    def set_batch_max_count(self, on: bool):
        """krep_gpu_set_batch_max_count: whether the batch calls take a finite params.max_count and cut every item's record list on
        the device (process-wide, off by default: a batch with max_count is refused then)"""
        self.lib.krep_gpu_set_batch_max_count(1 if on else 0)

    def get_batch_max_count(self) -> bool:
        return bool(self.lib.krep_gpu_get_batch_max_count())

    def batch_cut_launches(self):
        """(with the summed kept-record table in LDS, with the table in global memory): launches of the batch's max_count cut so far"""
        a, b = C.c_uint64(0), C.c_uint64(0)
        self.lib.krep_gpu_debug_batch_cut_launches(C.byref(a), C.byref(b))
        return int(a.value), int(b.value)

    def batch_pack_limit(self, nbytes: int):
        """test hook: the packed size at which a batch is cut into a further pack (0: the default)"""
        self.lib.krep_gpu_debug_batch_pack_limit(nbytes)

    def batch_times(self):
        """(pack, scan, segment, read-back) milliseconds of the calling thread's last search_batch"""
        t = [C.c_double(0) for _ in range(4)]
        self.lib.krep_gpu_debug_batch_times(*[C.byref(x) for x in t])
        return tuple(x.value for x in t)

    def search_batch(self, params: abi.Params, items, cfg=None, want_info=False):
        """krep_gpu_search_batch(params, items): [(count, positions[(n, 2) uint64])] in item order, every position relative to its
        item's first byte; `items` are bytes or np.uint8 arrays.  Raises KrepGpuError with the library's reason on 2 (a refused
        search included: there is no CPU fallback).  want_info: -> (that list, abi.BatchInfo)."""
        arr, n, keep = self.batch_items(items)
        res = (abi.BatchResult * max(n, 1))()
        rec = self.lib.krep_gpu_match_result_init(16)
        info = abi.BatchInfo()
        try:
            with _borrowed_trie(params):
                rc = self.lib.krep_gpu_search_batch(params.ref, C.byref(cfg) if cfg is not None else None, arr, n, res, rec, C.byref(info))
            if rc:
                raise KrepGpuError(self.last_error() or "krep_gpu_search_batch failed")
            pos = abi.result_positions(rec)
        finally:
            self.lib.krep_gpu_match_result_free(rec)
        del keep
        out = [(int(r.count), pos[int(r.first_record):int(r.first_record) + int(r.n_records)]) for r in res[:n]]
        return (out, info) if want_info else out

    def batch_rebase_launches(self):
        """(with the items' offset table in LDS, with the table in global memory): launches of the batch's record rebase so far"""
        a, b = C.c_uint64(0), C.c_uint64(0)
        self.lib.krep_gpu_debug_batch_rebase_launches(C.byref(a), C.byref(b))
        return int(a.value), int(b.value)

    # ---- the grep output of a batch (krep -r): the formatters over a pack, and the host call ----
    def format_lines_items(self, d_pack: int, packed_len: int, view: "abi.PackView", d_positions: int, n: int,
                           fmt: "abi.LineFormat | None" = None, d_out: int = 0, out_capacity: int = 0, d_item_out_off: int = 0,
                           stream: int = 0) -> "abi.LinesOut":
        """krep_gpu_format_lines_items(): format_lines_ex over a PACK of items (pack-relative records in (start, end) order), every
        item with the prefix `view` names for it.  d_out = 0 asks for .out_bytes; d_item_out_off: n_items + 1 device words, or 0."""
        out = abi.LinesOut()
        if self.lib.krep_gpu_format_lines_items(C.c_void_p(d_pack) if d_pack else None, packed_len, C.byref(view),
                                                C.c_void_p(d_positions) if d_positions else None, n,
                                                C.byref(fmt) if fmt is not None else None, C.c_void_p(d_out) if d_out else None,
                                                out_capacity, C.c_void_p(d_item_out_off) if d_item_out_off else None, C.byref(out),
                                                C.c_void_p(stream) if stream else None):
            raise KrepGpuError("krep_gpu_format_lines_items failed: " + self.last_error())
        return out

    def format_matches_items(self, d_pack: int, packed_len: int, view: "abi.PackView", d_positions: int, n: int,
                             fmt: "abi.MatchFormat | None" = None, d_out: int = 0, out_capacity: int = 0, d_item_out_off: int = 0,
                             stream: int = 0) -> "abi.MatchesOut":
        """krep_gpu_format_matches_items(): format_matches over a PACK of items: LINE restarts at 1 in every item and the stale
        number is applied per item.  d_out = 0 asks for .out_bytes; d_item_out_off: n_items + 1 device words, or 0."""
        out = abi.MatchesOut()
        if self.lib.krep_gpu_format_matches_items(C.c_void_p(d_pack) if d_pack else None, packed_len, C.byref(view),
                                                  C.c_void_p(d_positions) if d_positions else None, n,
                                                  C.byref(fmt) if fmt is not None else None, C.c_void_p(d_out) if d_out else None,
                                                  out_capacity, C.c_void_p(d_item_out_off) if d_item_out_off else None, C.byref(out),
                                                  C.c_void_p(stream) if stream else None):
            raise KrepGpuError("krep_gpu_format_matches_items failed: " + self.last_error())
        return out

    def batch_format_launches(self):
        """(with the items' offset table in LDS, with the table in global memory): calls of the pack formatters so far"""
        a, b = C.c_uint64(0), C.c_uint64(0)
        self.lib.krep_gpu_debug_batch_format_launches(C.byref(a), C.byref(b))
        return int(a.value), int(b.value)

    def grep_batch_times(self):
        """(pack, scan, segment, format, read-back) milliseconds of the calling thread's last grep_batch"""
        t = [C.c_double(0) for _ in range(5)]
        self.lib.krep_gpu_debug_grep_batch_times(*[C.byref(x) for x in t])
        return tuple(x.value for x in t)

    def grep_format(self, names, mode: str, color: bool = False):
        """(abi.GrepFormat, what keeps its strings alive) for items called `names` (bytes; None: no FILE: in front): the per-item
        prefixes from line_format(name, color).prefix (mode "lines"), match_format(name, color).prefix ("matches") or the plain
        "FILE:" the reference puts in front of a count ("count"), the other strings from the same two helpers"""
        n = len(names)
        if mode == "lines":
            pre = [bytes(line_format(nm, color).prefix or b"") for nm in names]
        elif mode == "matches":
            pre = [bytes(match_format(nm, color).prefix or b"") for nm in names]
        else:
            pre = [b"" if nm is None else nm + b":" for nm in names]
        arr = (C.c_char_p * max(n, 1))(*pre)
        lens = (C.c_size_t * max(n, 1))(*[len(p) for p in pre])
        lf, mf = line_format(None, color), match_format(None, color)
        lf.prefix, lf.prefix_len, mf.prefix, mf.prefix_len = None, 0, None, 0
        g = abi.GrepFormat(C.cast(arr, C.POINTER(C.c_char_p)), C.cast(lens, C.POINTER(C.c_size_t)), lf, mf)
        return g, (arr, lens, pre, lf, mf)

    def grep_batch(self, params: abi.Params, items, names, color=False, cfg=None, want_info=False):
        """krep_gpu_grep_batch(params, items): what `krep [-o | -c] PATTERN` prints for every item, the items called `names` (bytes)
        -> (bytes, [(count, offset, nbytes)]): item i's text is bytes[offset:offset + nbytes].  The mode is the reference's: -c when
        params count, -o when cfg.only_matching, else matching lines.  cfg None: the process-wide defaults (a thread configuration
        is passed as cfg).  Raises KrepGpuError with the library's reason on 2.  want_info: one more, the abi.BatchInfo."""
        if cfg is None:
            cfg = self.default_config()
        n = len(items)
        names = [None if nm is None else (nm if isinstance(nm, bytes) else str(nm).encode()) for nm in names]
        assert len(names) == n
        mode = ("count" if params.s.count_lines_mode or params.s.count_matches_mode else
                "matches" if cfg.only_matching else "lines")
        fmt, keep_fmt = self.grep_format(names, mode, color)
        arr, _, keep = self.batch_items(items)
        per = (abi.GrepItem * max(n, 1))()
        out = abi.GrepOutput(None, 0, 0)
        info = abi.BatchInfo()
        try:
            with _borrowed_trie(params):
                rc = self.lib.krep_gpu_grep_batch(params.ref, C.byref(cfg), arr, n, C.byref(fmt), per, C.byref(out), C.byref(info))
            if rc:
                raise KrepGpuError(self.last_error() or "krep_gpu_grep_batch failed")
            data = C.string_at(out.bytes, out.len) if out.len else b""
        finally:
            if out.bytes:
                _libc_free(out.bytes)
        del keep, keep_fmt
        res = [(int(p.count), int(p.out_offset), int(p.out_bytes)) for p in per[:n]]
        return (data, res, info) if want_info else (data, res)

    def batch_items(self, items):
        """(krep_gpu_batch_item_t[n], n, what keeps the texts alive) for `items` (bytes or np.uint8 arrays): for batch_fill_host()"""
        arr = (abi.BatchItem * max(len(items), 1))()
        keep = []
        for i, it in enumerate(items):
            ptr, ln, k = self._ptr(it)
            keep.append(k)
            arr[i].text, arr[i].len = (ptr.value if ln else None), ln
        return arr, len(items), keep

    def batch_fill_host(self, held, lo: int, cnt: int, guard: int = 0):
        """test hook (host only, no GPU needed): bytes [lo, lo + cnt) of the pack of `held` (from batch_items()) exactly as the
        staging ring of search_batch gets them -> np.uint8[guard + cnt + guard], the guard bytes 0xA5 on both sides of the
        destination; None when the slice leaves the pack."""
        arr, n, _ = held
        out = np.full(cnt + 2 * guard, 0xA5, dtype=np.uint8)
        rc = self.lib.krep_gpu_debug_batch_fill_host(arr, n, lo, cnt, C.c_void_p(out.ctypes.data + guard))
        return out if rc == 0 else None

    def search_buffer(self, params: abi.Params, text, only_matching=False, num_gpus=1, want_result=True, cfg=None):
        ptr, n, keep = self._ptr(text)
        res = self.lib.krep_gpu_match_result_init(16) if want_result else None
        cnt = C.c_uint64(0)
        try:
            if cfg is not None:
                rc = self.lib.search_buffer_ex(params.ref, ptr, n, C.byref(cfg), num_gpus, res, C.byref(cnt))
            else:
                rc = self.lib.search_buffer(params.ref, ptr, n, int(only_matching), num_gpus, res, C.byref(cnt))
            pos = abi.result_positions(res) if res else None
        finally:
            if res:
                self.lib.krep_gpu_match_result_free(res)
        del keep
        return int(rc), int(cnt.value), pos

    # ---- device-resident path ----
    def plan(self, params: abi.Params, only_matching=False, device=0) -> "Plan":
        h = self.lib.krep_gpu_plan_create(params.ref, int(only_matching), device)
        if not h:
            raise KrepGpuError("krep_gpu_plan_create failed: " + self.last_error())
        return Plan(self, h, params, bool(only_matching))

    def generate(self, d_ptr: int, length: int, global_off: int, kind: int, seed: int, plant: bytes = b"",
                 period: int = 0, stream: int = 0):
        rc = self.lib.krep_gpu_generate(C.c_void_p(d_ptr), length, global_off, kind, seed, plant, len(plant), period,
                                        C.c_void_p(stream))
        if rc:
            raise KrepGpuError("krep_gpu_generate failed: " + self.last_error())

    def generate_host(self, length: int, global_off: int, kind: int, seed: int, plant: bytes = b"",
                      period: int = 0) -> np.ndarray:
        out = np.empty(length, dtype=np.uint8)
        self.lib.krep_gpu_generate_host(C.c_void_p(out.ctypes.data), length, global_off, kind, seed, plant, len(plant),
                                        period)
        return out


class Plan:
    def __init__(self, eng: Engine, handle, params, only_matching=False):
        self.eng, self.h, self.params, self.only_matching = eng, handle, params, only_matching

    @property
    def ref_algo(self) -> int:
        return int(self.eng.lib.krep_gpu_plan_ref_algo(self.h))

    def scan(self, d_text: int, text_len: int, own_lo=0, own_hi=None, global_base=0, d_positions: int = 0,
             capacity: int = 0, stream: int = 0, time_it=False, global_len=0) -> abi.ScanOut:
        out = abi.ScanOut()
        rc = self.eng.lib.krep_gpu_scan_device_ex(self.h, C.c_void_p(d_text), text_len, own_lo,
                                                  text_len if own_hi is None else own_hi, global_base, global_len,
                                                  C.c_void_p(d_positions) if d_positions else None, capacity,
                                                  C.c_void_p(stream) if stream else None, int(time_it), C.byref(out))
        if rc:
            raise KrepGpuError("krep_gpu_scan_device failed: " + self.eng.last_error())
        return out

    def longest_match(self) -> int:
        """The most text bytes that decide one match of the plan: what the output drivers size a halo, a staging length, records_hi
        and a per-item guess by.  A literal plan: its longest pattern.  A regex plan (krep -E): NOT the length of the pattern string
        (`q[a-c]{15}` is 10 pattern bytes and 16 text bytes) but L / Lmax of the compiler that takes the search, asked in the order
        every search asks them (anchored, then alternation, then the expanding one), plus the newline a `$` looks at behind the
        match: a window must hold that byte too, or the scan refuses it.  With set_regex_loops(True) a search the loops compiler takes
        says 4097: a match lies inside one line, and no line of more than 4096 bytes is walked."""
        s = self.params.s
        if not s.use_regex:
            return max(int(x) for x in s.pattern_lens[: s.num_patterns]) if s.num_patterns else int(s.pattern_len)
        eng = self.eng
        try:
            info = eng.regex_compile_anchored(self.params)
            return int(info.seq.L) + int(bool(info.eol))
        except KrepGpuError:
            pass
        try:
            return int(eng.regex_compile_alt(self.params).Lmax)
        except KrepGpuError:
            pass
        try:
            info = eng.regex_compile_ext(self.params)
            return int(info.alt.Lmax) + int(bool(info.eol))
        except KrepGpuError:
            if not (eng.get_regex_loops() or eng.get_regex_groups()):  # (no search asks those compilers: no plan exists either)
                raise
            if not self.is_loops():
                (eng.regex_compile_groups if eng.get_regex_groups() else eng.regex_compile_loops)(self.params)  # (raises the refusal)
            return 4096 + 1  # a match of a loops program lies inside one line, and no line of more than 4096 bytes is walked

    def is_loops(self) -> bool:
        """whether the plan's search is walked line by line (kg_regex_loops.hip): the three older compilers refuse it, and the loops
        compiler (-E with *, + or {n,} behind an atom) or the groups compiler (repeated and nested groups) takes it, each asked only
        when its own switch is on"""
        s, eng = self.params.s, self.eng
        if not s.use_regex or not (eng.get_regex_loops() or eng.get_regex_groups()):
            return False
        for older in (eng.regex_compile_anchored, eng.regex_compile_alt, eng.regex_compile_ext):
            try:
                older(self.params)
                return False
            except KrepGpuError:
                pass
        for newer, on in ((eng.regex_compile_loops, eng.get_regex_loops()), (eng.regex_compile_groups, eng.get_regex_groups())):
            try:
                if on:
                    newer(self.params)
                    return True
            except KrepGpuError:
                pass
        return False

    def left_context(self, own_lo: int) -> int:
        """The bytes of the text the pieces drivers stage in front of what a window owns: one (the byte -w and ^ look at), for a
        loops plan min(own_lo, longest_match() - 1) = up to 4096: the line walk starts at the first byte of every line that meets the
        owned range, and the scan refuses a buffer that begins inside such a line."""
        return min(int(own_lo), self.longest_match() - 1 if self.is_loops() else 1)

    def grep_lines(self, d_text: int, n: int, filename=None, max_count=None, stream: int = 0, color=False) -> bytes:
        """What `krep [-m N] PATTERN FILE` prints (colour off) for the n bytes at d_text: the scan with records, the cut to the
        first max_count records in emission order (search_file()), the (start, end) order for a multi-pattern list, and the
        lines from krep_gpu_format_lines.  filename: str / bytes in front of every line ("FILE:"), None as for search_string().
        max_count: None takes the plan's.  color=True: what `krep --color=always` prints (`--color=always -s` without a filename),
        from krep_gpu_format_lines_ex with the strings of line_format().  Device buffers come from torch (the current device)."""
        import torch
        eng = self.eng
        limit = int(self.params.s.max_count)
        if max_count is not None:
            limit = min(limit, int(max_count))
        if limit == 0 or n == 0:
            return b""
        found = self.scan(d_text, n, stream=stream)
        cap = int(max(found.count, found.total_matches))
        if cap == 0:
            return b""
        pos = torch.empty(2 * (cap + 1), dtype=torch.int64, device="cuda")
        out = self.scan(d_text, n, d_positions=pos.data_ptr(), capacity=cap + 1, stream=stream)
        if out.overflow:
            raise KrepGpuError("grep_lines: the record list outgrew the count of the scan before it")
        m = min(int(out.stored), limit)
        if m == 0:
            return b""
        if self.params.s.num_patterns > 1:
            eng.order_by_start(pos.data_ptr(), m, n, stream)
        name = None if filename is None else (filename if isinstance(filename, bytes) else str(filename).encode())
        if color:
            fmt = line_format(name, True)
            extra = fmt.prefix_len + fmt.line_close_len + fmt.before_match_len + fmt.after_match_len  # (at most a line per record)

            def call(d_out, capacity):
                return eng.format_lines_ex(d_text, n, pos.data_ptr(), m, limit, fmt, d_out, capacity, stream)
        else:
            prefix = b"" if name is None else name + b":"
            extra = len(prefix)

            def call(d_out, capacity):
                return eng.format_lines(d_text, n, pos.data_ptr(), m, limit, prefix, d_out, capacity, stream)
        guess = m * (extra + 256) + 4096  # one call when the lines are short; the sizes it reports serve the second
        buf = torch.empty(guess, dtype=torch.uint8, device="cuda")
        res = call(buf.data_ptr(), guess)
        if res.overflow:
            buf = torch.empty(int(res.out_bytes), dtype=torch.uint8, device="cuda")
            res = call(buf.data_ptr(), int(res.out_bytes))
            assert not res.overflow
        return buf[: int(res.out_bytes)].cpu().numpy().tobytes()

    def grep_lines_pieces(self, text, piece_bytes: int, filename=None, color=False, halo_bytes: int = 4096) -> bytes:
        """grep_lines for a text on the HOST that never lies on the device as a whole: it is staged piece by piece into ONE device
        buffer of 1 + piece_bytes + halo bytes (the byte of left context — left_context(): up to 4096 for a loops plan —, the piece,
        the halo), every piece is scanned with start
        ownership up to records_hi = buffer end - (longest_match() - 1) (the text's end where the buffer ends it), a multi-pattern
        list is put in (start, end) order, and krep_gpu_format_lines_window formats the lines that START in the piece.  A line the
        call reports as incomplete (it outruns the halo) is staged again as a window of its own, its reach doubled until it is
        complete.  A line of the piece that outruns the halo and holds no record in front of records_hi is one the call cannot
        know of: the driver finds the line that is open at records_hi on the host and stages it whole.  Returns the concatenated
        bytes: those of grep_lines on the resident text.
        text: bytes, a numpy uint8 array or a CPU uint8 tensor.  The plan's max_count holds: a single literal's list is in emission
        order, so it is cut by counting records across the pieces; a multi-pattern plan with a finite max_count is refused (the
        cut to the first max_count records in emission order is a property of the whole list).  So are the classes whose match
        set cannot be cut into independent pieces (krep_gpu_split_mode() != PIECES)."""
        import torch
        eng, s = self.eng, self.params.s
        if isinstance(text, torch.Tensor):
            host = text.contiguous().view(torch.uint8).reshape(-1)
        else:
            a = np.ascontiguousarray(text, dtype=np.uint8).reshape(-1) if isinstance(text, np.ndarray) \
                else np.frombuffer(bytes(text), dtype=np.uint8)
            host = torch.from_numpy(a if a.flags.writeable else a.copy())  # (torch takes no read-only array; nothing writes to it)
        total = int(host.numel())
        piece_bytes = int(piece_bytes)
        if piece_bytes <= 0:
            raise KrepGpuError("grep_lines_pieces: piece_bytes must be positive")
        limit = int(s.max_count)
        multi = s.num_patterns > 1
        if multi and limit != abi.SIZE_MAX:
            raise KrepGpuError("grep_lines_pieces: a multi-pattern plan with max_count: the cut to the first max_count records in "
                               "emission order needs the whole record list")
        if limit == 0 or total == 0:
            return b""
        if eng.split_mode(self.params, total) != abi.SPLIT_PIECES:
            raise KrepGpuError("grep_lines_pieces: the match set of this search cannot be cut into independent pieces "
                               "(krep_gpu_split_mode)")
        longest = self.longest_match()
        halo = max(int(halo_bytes), longest)  # (records_hi >= own_hi)
        lctx = self.left_context(total)  # one byte; a loops plan: 4096 (a window holds the lines that meet its owned range, whole)
        name = None if filename is None else (filename if isinstance(filename, bytes) else str(filename).encode())
        fmt = line_format(name, bool(color))
        extra = fmt.prefix_len + fmt.line_close_len + fmt.before_match_len + fmt.after_match_len
        state = {"buf": torch.empty(lctx + piece_bytes + halo + 64, dtype=torch.uint8, device="cuda")}
        parts = []
        view, step = memoryview(host.numpy()), 1 << 20

        def newline_before(pos):
            """the last newline in front of pos on the host (-1: none): a line's length at the most is looked at"""
            while pos > 0:
                lo_ = max(pos - step, 0)
                k = bytes(view[lo_:pos]).rfind(b"\n")
                if k >= 0:
                    return lo_ + k
                pos = lo_
            return -1

        def newline_from(pos):
            """the first newline at or behind pos on the host (total: none)"""
            while pos < total:
                k = bytes(view[pos:pos + step]).find(b"\n")
                if k >= 0:
                    return pos + k
                pos += step
            return total

        def window(own_lo, own_hi, reach, records_left, lines_left):
            """stage [own_lo - lctx, own_hi + reach), scan and format it -> (LinesWindowOut, records the scan stored)"""
            base, end = max(own_lo - lctx, 0), min(own_hi + reach, total)
            if state["buf"].numel() < end - base + 64:
                state["buf"] = torch.empty(end - base + 64, dtype=torch.uint8, device="cuda")
            buf = state["buf"]
            buf[: end - base].copy_(host[base:end])
            d_text, blen = buf.data_ptr(), end - base
            records_hi = total if end == total else end - (longest - 1)
            lo, hi = own_lo - base, records_hi - base
            found = self.scan(d_text, blen, lo, hi, base, global_len=total)
            cap = int(max(found.count, found.total_matches))
            if cap == 0:
                return None, 0
            pos = torch.empty(2 * (cap + 1), dtype=torch.int64, device="cuda")
            got = self.scan(d_text, blen, lo, hi, base, pos.data_ptr(), cap + 1, global_len=total)
            if got.overflow:
                raise KrepGpuError("grep_lines_pieces: the record list outgrew the count of the scan before it")
            m = min(int(got.stored), records_left)
            if m == 0:
                return None, 0
            if multi:
                eng.order_by_start(pos.data_ptr(), m, total)
            win = abi.LinesWindow(base, total, own_lo, own_hi, records_hi)
            guess = m * (extra + 256) + 4096
            out = torch.empty(guess, dtype=torch.uint8, device="cuda")
            res = eng.format_lines_window(d_text, blen, win, pos.data_ptr(), m, lines_left, fmt, out.data_ptr(), guess)
            if res.lines.overflow:
                out = torch.empty(int(res.lines.out_bytes), dtype=torch.uint8, device="cuda")
                res = eng.format_lines_window(d_text, blen, win, pos.data_ptr(), m, lines_left, fmt, out.data_ptr(),
                                              int(res.lines.out_bytes))
                assert not res.lines.overflow
            if res.lines.out_bytes:
                parts.append(out[: int(res.lines.out_bytes)].cpu().numpy().tobytes())
            return res, m

        before, lines_left = 0, limit  # records in front of the piece (counted under a finite max_count only); lines still to emit
        for lo in range(0, total, piece_bytes):
            hi = min(lo + piece_bytes, total)
            left = limit - before
            if left <= 0 or lines_left <= 0:
                break
            res, stored = window(lo, hi, halo, left, lines_left)
            records_hi = total if hi + halo >= total else hi + halo - (longest - 1)
            if limit != abi.SIZE_MAX and hi < total:  # the records that START in the piece, on the buffer as it still stands
                base = max(lo - lctx, 0)
                before += int(self.scan(state["buf"].data_ptr(), min(hi + halo, total) - base, lo - base, hi - base, base,
                                        global_len=total).total_matches)
            if res is not None and lines_left != abi.SIZE_MAX:
                lines_left -= int(res.lines.lines)
            if res is not None and res.incomplete_line_start1:
                start = int(res.incomplete_line_start1) - 1
                reach = 2 * (min(hi + halo, total) - (start + 1))  # the line outruns what the piece's buffer held of it: twice that
                ahead = int(res.incomplete_first_record)  # records of the piece's list in front of the line
                while True:
                    again, _ = window(start, start + 1, reach, left - ahead, 1)
                    if again is None:
                        raise KrepGpuError("grep_lines_pieces: a line reported incomplete holds no record when staged again")
                    if not again.incomplete_line_start1:
                        break
                    if start + 1 + reach >= total:
                        raise KrepGpuError("grep_lines_pieces: a line is incomplete in a buffer that ends the text")
                    reach *= 2
                assert again.lines.lines == 1
                if lines_left != abi.SIZE_MAX:
                    lines_left -= 1
            elif records_hi < total and lines_left > 0:
                # A call cannot report an owned line whose FIRST record lies at or behind records_hi: no record of it is in its
                # list.  That can only be the line that is open at records_hi; where the piece owns it, it is staged whole.
                start = newline_before(records_hi) + 1
                if lo <= start < hi:
                    whole, _ = window(start, start + 1, newline_from(records_hi) + longest - (start + 1), left - stored, 1)
                    if whole is not None:
                        assert whole.lines.lines == 1 and not whole.incomplete_line_start1
                        if lines_left != abi.SIZE_MAX:
                            lines_left -= 1
        return b"".join(parts)

    def grep_only_matching(self, d_text: int, n: int, filename=None, max_count=None, color=False, stream: int = 0) -> bytes:
        """What `krep -o [-m N] [--color=always] PATTERN FILE` prints for the n bytes at d_text: one FILE:LINE:match per match.  The
        scan with records, the cut to the first max_count records in emission order (search_file()), the (start, end) order for a
        multi-pattern list, and the bytes from krep_gpu_format_matches.  The plan must have been made with only_matching=True: under
        -o the reference's match set is another one.  filename, max_count: as for grep_lines."""
        import torch
        eng = self.eng
        if not self.only_matching:
            raise KrepGpuError("grep_only_matching: the plan was not created with only_matching=True (the match set of -o differs)")
        limit = int(self.params.s.max_count)
        if max_count is not None:
            limit = min(limit, int(max_count))
        if limit == 0 or n == 0:
            return b""
        found = self.scan(d_text, n, stream=stream)
        cap = int(max(found.count, found.total_matches))
        if cap == 0:
            return b""
        pos = torch.empty(2 * (cap + 1), dtype=torch.int64, device="cuda")
        out = self.scan(d_text, n, d_positions=pos.data_ptr(), capacity=cap + 1, stream=stream)
        if out.overflow:
            raise KrepGpuError("grep_only_matching: the record list outgrew the count of the scan before it")
        m = min(int(out.stored), limit)
        if m == 0:
            return b""
        if self.params.s.num_patterns > 1:
            eng.order_by_start(pos.data_ptr(), m, n, stream)
        name = b"" if filename is None else (filename if isinstance(filename, bytes) else str(filename).encode())
        fmt = match_format(name if filename is not None else None, color)
        longest = self.longest_match()
        per_item = fmt.prefix_len + fmt.before_number_len + fmt.after_number_len + fmt.after_match_len + 20 + 2 + longest
        guess = m * per_item + 4096  # enough by construction (no record is longer than longest_match()); the second call is a backstop
        buf = torch.empty(guess, dtype=torch.uint8, device="cuda")
        res = eng.format_matches(d_text, n, pos.data_ptr(), m, limit, fmt, buf.data_ptr(), guess, stream)
        if res.overflow:
            buf = torch.empty(int(res.out_bytes), dtype=torch.uint8, device="cuda")
            res = eng.format_matches(d_text, n, pos.data_ptr(), m, limit, fmt, buf.data_ptr(), int(res.out_bytes), stream)
            assert not res.overflow
        return buf[: int(res.out_bytes)].cpu().numpy().tobytes()

    def grep_only_matching_pieces(self, text, piece_bytes: int, filename=None, color=False) -> bytes:
        """grep_only_matching for a text on the HOST that never lies on the device as a whole; returns the bytes of
        grep_only_matching on the resident text.  The text is cut into pieces of piece_bytes; piece [lo, hi) is staged as
        [max(lo - left_context(), 0), min(hi + longest_match(), total)) into ONE reused device buffer (the byte of left context for -w
        — up to 4096 for a loops plan, whose line walks start at each line's first byte —, and
        behind the piece a match that starts on its last byte with the byte -w looks at behind it).  Under -o many single
        literals couple a match to the one before it (krep_gpu_split_mode() = CHAIN), so the pieces are scanned IN TEXT ORDER
        through scan_seq, each taking the carry of the one before it (the counting scan and the recording scan of a piece take the
        same carry); families without that dependency pass the carry through, so one road serves both classes.  A multi-pattern
        list is put in (start, end) order, and krep_gpu_format_matches_window formats the piece's records with count_to = the
        next piece's base (hi - 1: its byte of left context; hi - 4096 for a loops plan), the newline count and the stale line number chained from call to call.
        last_newline1 is looked up once on the host, backwards from the end of the text.  stale_rule (more than 10 records in the
        whole list) is false when max_count <= 10 and true as soon as the running count passes 10.  Until then only records that
        start at or behind last_newline1 depend on it: those are HELD BACK (StaleSchedule: at most 10 (start, end) pairs on the
        host, nothing emitted behind them) while everything in front of them is formatted at once.  When the rule is decided (the
        count passes 10, or the text ends) each held record is formatted by a call of its own on a buffer staged from the host
        text: global_base = its start, newlines_before = the text's newline total (known by then: the chain has passed the last
        newline), the chained stale_line.  Then the pieces go on normally.
        text: bytes, a numpy uint8 array or a CPU uint8 tensor.  The plan's max_count holds: a single literal's list is in emission
        order, so it is cut by counting records across the pieces.  Refused: a plan made without only_matching=True, a
        multi-pattern plan with a finite max_count (the cut to the first max_count records in emission order needs the whole
        list), and a search krep_gpu_split_mode() calls WHOLE."""
        import torch
        eng, s = self.eng, self.params.s
        if not self.only_matching:
            raise KrepGpuError("grep_only_matching_pieces: the plan was not created with only_matching=True (the match set of -o "
                               "differs)")
        if isinstance(text, torch.Tensor):
            host = text.contiguous().view(torch.uint8).reshape(-1)
        else:
            a = np.ascontiguousarray(text, dtype=np.uint8).reshape(-1) if isinstance(text, np.ndarray) \
                else np.frombuffer(bytes(text), dtype=np.uint8)
            host = torch.from_numpy(a if a.flags.writeable else a.copy())  # (torch takes no read-only array; nothing writes to it)
        total = int(host.numel())
        piece_bytes = int(piece_bytes)
        if piece_bytes <= 0:
            raise KrepGpuError("grep_only_matching_pieces: piece_bytes must be positive")
        limit = int(s.max_count)
        multi = s.num_patterns > 1
        if multi and limit != abi.SIZE_MAX:
            raise KrepGpuError("grep_only_matching_pieces: a multi-pattern plan with max_count: the cut to the first max_count "
                               "records in emission order needs the whole record list")
        cfg = eng.default_config()  # the class of the search under -o (the plan carries only_matching; the process default may not)
        cfg.only_matching = 1
        eng.set_thread_config(cfg)
        try:
            mode = eng.split_mode(self.params, total)
        finally:
            eng.set_thread_config(None)
        if mode == abi.SPLIT_WHOLE:
            raise KrepGpuError("grep_only_matching_pieces: this search takes the whole text in one window (krep_gpu_split_mode)")
        if limit == 0 or total == 0:
            return b""
        longest = self.longest_match()
        lctx = self.left_context(total)  # one byte; a loops plan: 4096 (a window holds the lines that meet its owned range, whole)
        name = None if filename is None else (filename if isinstance(filename, bytes) else str(filename).encode())
        fmt = match_format(name, bool(color))
        per_item = fmt.prefix_len + fmt.before_number_len + fmt.after_number_len + fmt.after_match_len + 20 + 2 + longest
        buf = torch.empty(lctx + piece_bytes + longest + 64, dtype=torch.uint8, device="cuda")
        view, step = memoryview(host.numpy()), 1 << 20
        last_nl1, at = 0, total  # the last newline of the text + 1, looked for backwards from its end
        while at > 0 and not last_nl1:
            lo_ = max(at - step, 0)
            k = bytes(view[lo_:at]).rfind(b"\n")
            last_nl1 = lo_ + k + 1 if k >= 0 else 0
            at = lo_
        sched = StaleSchedule(limit, last_nl1)
        parts = []
        chain = {"nl": 0, "stale": 0}  # the two carries of krep_gpu_format_matches_window

        # reused like the text buffer: the output of one call, and the text and the record of a held one
        dev = {"out": torch.empty(4096, dtype=torch.uint8, device="cuda"), "one": torch.empty(longest + 64, dtype=torch.uint8, device="cuda"),
               "rec": torch.empty(2, dtype=torch.int64, device="cuda")}

        def grown(key, nbytes):
            if dev[key].numel() < nbytes:
                dev[key] = torch.empty(max(nbytes, 2 * dev[key].numel()), dtype=torch.uint8, device="cuda")
            return dev[key]

        def fmt_call(d_text, blen, base, count_to, d_pos, n, rule):
            win = abi.MatchesWindow(base, total, count_to, chain["nl"], last_nl1, chain["stale"], int(rule))
            out = grown("out", n * per_item + 4096)
            res = eng.format_matches_window(d_text, blen, win, d_pos, n, abi.SIZE_MAX, fmt, out.data_ptr(), out.numel())
            if res.matches.overflow:  # (a backstop: per_item holds the longest match)
                out = grown("out", int(res.matches.out_bytes))
                res = eng.format_matches_window(d_text, blen, win, d_pos, n, abi.SIZE_MAX, fmt, out.data_ptr(), out.numel())
                assert not res.matches.overflow
            if res.matches.out_bytes:
                parts.append(out[: int(res.matches.out_bytes)].cpu().numpy().tobytes())
            return res

        def held_calls(records, rule):
            """every held record in a call of its own: they lie behind the last newline, where chain["nl"] is the text's total"""
            for start, end in records:
                stop = max(min(end, total), start + 1)
                one = grown("one", stop - start + 64)
                one[: stop - start].copy_(host[start:stop])
                dev["rec"].copy_(torch.tensor([start, end], dtype=torch.int64))
                chain["stale"] = int(fmt_call(one.data_ptr(), stop - start, start, start, dev["rec"].data_ptr(), 1, rule).stale_line)

        carry = None
        for lo in range(0, total, piece_bytes):
            left = limit - sched.count
            if left <= 0:
                break
            hi = min(lo + piece_bytes, total)
            base, end = max(lo - lctx, 0), min(hi + longest, total)
            buf[: end - base].copy_(host[base:end])
            d_text, blen = buf.data_ptr(), end - base
            found, carry_out = self.scan_seq(d_text, blen, lo - base, hi - base, base, global_len=total, carry_in=carry)
            cap, m, pos = int(max(found.count, found.total_matches)), 0, None
            if cap:
                pos = torch.empty(2 * (cap + 1), dtype=torch.int64, device="cuda")
                got, carry_out = self.scan_seq(d_text, blen, lo - base, hi - base, base, pos.data_ptr(), cap + 1, global_len=total,
                                               carry_in=carry)
                if got.overflow:
                    raise KrepGpuError("grep_only_matching_pieces: the record list outgrew the count of the scan before it")
                m = min(int(got.stored), left)
                if multi and m:
                    eng.order_by_start(pos.data_ptr(), m, total)
            carry = carry_out
            flush, now, rule = sched.add(m, lambda: pos[: 2 * m].view(-1, 2).cpu().tolist())
            held_calls(flush, rule)
            # (a piece without records is formatted too: its call carries the newline count on)
            res = fmt_call(d_text, blen, base, max(hi - lctx, 0) if hi < total else total, pos.data_ptr() if now else 0, now, rule)
            chain["nl"], chain["stale"] = int(res.newlines_before_count_to), int(res.stale_line)
        flush, rule = sched.end()
        held_calls(flush, rule)
        return b"".join(parts)

    def anchor_info(self):
        """(state 0 undecided / 1 end grams / 2 anchored, patterns moved, est. candidate rate end grams, ... anchors) — multi-pattern plans"""
        st, mv, r0, r1 = C.c_int(0), C.c_uint32(0), C.c_double(0), C.c_double(0)
        if self.eng.lib.krep_gpu_debug_anchor_info(self.h, C.byref(st), C.byref(mv), C.byref(r0), C.byref(r1)):
            return None
        return int(st.value), int(mv.value), float(r0.value), float(r1.value)

    def literal_dma_state(self):
        """(text sampled?, LDS-DMA kernel barred for it?, share of 1-KiB cells its prefilter passed) — kg_scan.hip lit_pass"""
        a, b, r = C.c_int(0), C.c_int(0), C.c_double(0)
        if self.eng.lib.krep_gpu_debug_literal_dma_state(self.h, C.byref(a), C.byref(b), C.byref(r)):
            return None
        return bool(a.value), bool(b.value), float(r.value)

    def split_state(self) -> int:
        """0 undecided / 1 one dictionary / 2 split into a >= 4-byte part and a 1..3-byte part (kg_scan_ac.hip scan_ac_split)"""
        f = self.eng.lib.krep_gpu_debug_split_state
        f.restype = C.c_int
        f.argtypes = [C.c_void_p]
        return int(f(self.h))

    def anchor_measured(self):
        """(candidates per tested position the last general-kernel scan counted, decisions re-opened so far)"""
        m, r = C.c_double(0), C.c_int(0)
        if self.eng.lib.krep_gpu_debug_anchor_measured(self.h, C.byref(m), C.byref(r)):
            return None
        return float(m.value), int(r.value)

    def ac_last_scan(self, part: int = 0):
        """krep_gpu_debug_ac_last_scan(): the report of the last multi-pattern scan as a dict (road, ci, lines, shorts, stride, anch,
        ww_filter, exact, g4x_mode, stage_cap, upt, n_units, overflow_units, emit, next_stage_cap, short_lens, scans); part 1: the short
        part of a split plan.  None: a single-literal plan, or no such part."""
        rep = abi.AcScan()
        if self.eng.lib.krep_gpu_debug_ac_last_scan(self.h, int(part), C.byref(rep)):
            return None
        return rep.as_dict()

    def scan_seq(self, d_text: int, text_len: int, own_lo, own_hi, global_base=0, d_positions: int = 0, capacity: int = 0,
                 global_len=0, carry_in: "abi.SeqCarry | None" = None):
        """krep_gpu_scan_device_seq(): one piece of a text scanned in text order -> (ScanOut, SeqCarry it leaves)."""
        out, cout = abi.ScanOut(), abi.SeqCarry()
        rc = self.eng.lib.krep_gpu_scan_device_seq(self.h, C.c_void_p(d_text), text_len, own_lo, own_hi, global_base, global_len,
                                                   C.c_void_p(d_positions) if d_positions else None, capacity, None, 0,
                                                   C.byref(carry_in) if carry_in is not None else None, C.byref(cout),
                                                   C.byref(out))
        if rc:
            raise KrepGpuError("krep_gpu_scan_device_seq failed: " + self.eng.last_error())
        return out, cout

    def close(self):
        if self.h:
            self.eng.lib.krep_gpu_plan_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# the escape codes of the reference's coloured output (data: krep.h:34-39)
COLOR_RESET, COLOR_FILENAME, COLOR_SEPARATOR = b"\033[0m", b"\033[1;38;5;81m", b"\033[38;5;244m"
COLOR_LINE_NUMBER, COLOR_MATCH = b"\033[1;38;5;111m", b"\033[1;38;5;222m"
COLOR_TEXT = b"\033[38;5;252m"
STALE_AFTER = 10  # -o: with more than this many records the reference prints stale line numbers behind the last newline (krep.c:531)


def match_format(filename: "bytes | None" = None, color: bool = False) -> "abi.MatchFormat":
    """the strings of `krep -o` around LINE and the match (krep.c:565, :719-766): filename None prints no FILE: in front"""
    if not color:
        return abi.MatchFormat(b"" if filename is None else filename + b":")
    prefix = b"" if filename is None else COLOR_FILENAME + filename + COLOR_RESET + COLOR_SEPARATOR + b":"
    return abi.MatchFormat(prefix, COLOR_LINE_NUMBER, COLOR_RESET + COLOR_MATCH, COLOR_RESET)


def line_format(filename: "bytes | None" = None, color: bool = False) -> "abi.LineFormat":
    """the strings of the default line output around a line and its matches (krep.c:940-1018): filename None prints no FILE: in front"""
    if not color:
        return abi.LineFormat(b"" if filename is None else filename + b":")
    prefix = COLOR_TEXT if filename is None else COLOR_FILENAME + filename + COLOR_RESET + COLOR_SEPARATOR + b":" + COLOR_TEXT
    return abi.LineFormat(prefix, COLOR_MATCH, COLOR_TEXT, COLOR_RESET)


class StaleSchedule:
    """When Plan.grep_only_matching_pieces may format the records of a piece.  The reference's stale line number (more than 10
    records in the whole list, after its max_count cut) touches only the records that start at or behind last_newline1; until the
    running count has passed 10 or the text has ended nobody knows whether it applies.  So while the rule is undecided those
    records (at most 10) are HELD on the host, in order, and nothing is emitted behind them; everything in front of them is
    formatted at once.  Host logic only."""

    def __init__(self, max_count: int, last_newline1: int):
        self.count, self.held, self.last_newline1 = 0, [], int(last_newline1)
        # never applies: a list of at most 10 records, or a text without a newline
        self.rule = False if (max_count <= STALE_AFTER or not last_newline1) else None

    def add(self, m: int, fetch):
        """the next piece brought m records; fetch() -> their (start, end) pairs, asked for only while undecided (then m <= 10).
        -> (held records to format first, each in a call of its own; how many of the piece's records to format now;
        stale_rule for both)"""
        self.count += int(m)
        if self.rule is None and self.count > STALE_AFTER:
            self.rule = True
        if self.rule is not None:
            flush, self.held = self.held, []
            return flush, int(m), self.rule
        recs = [(int(s), int(e)) for s, e in fetch()] if m else []
        now = 0 if self.held else sum(1 for s, _ in recs if s < self.last_newline1)  # (ascending: a prefix)
        self.held += recs[now:]
        return [], now, False

    def end(self):
        """the text has ended -> (held records to format, stale_rule): undecided until now means at most 10 records"""
        if self.rule is None:
            self.rule = False
        flush, self.held = self.held, []
        return flush, self.rule


_engine = None


def load() -> Engine:
    global _engine
    if _engine is None:
        _engine = Engine()
    return _engine
