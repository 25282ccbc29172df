"""ctypes binding of include/metheor_hip.h (one Python method per C entry point)."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

MTH_MEM_HOST, MTH_MEM_DEVICE = 0, 1

# every symbol include/metheor_hip.h declares (checked by tests/test_capi_symbols.py)
SYMBOLS = [
    "mth_abi_version", "mth_ctx_create", "mth_ctx_destroy", "mth_ctx_set_stream", "mth_ctx_sync",
    "mth_strerror", "mth_last_error", "mth_notes", "mth_batch_prepare", "mth_batch_release", "mth_reset", "mth_pdr_lpmd_accumulate", "mth_pdr_count",
    "mth_pdr_fetch", "mth_result_buffer_alloc", "mth_result_buffer_free", "mth_pdr_device_view", "mth_lpmd_global", "mth_lpmd_add_unbatched", "mth_lpmd_from_counts",
    "mth_lpmd_export_device", "mth_device_count", "mth_allreduce_lpmd", "mth_rccl_unique_id", "mth_rccl_init_rank",
    "mth_allreduce_lpmd_rank", "mth_quartet_accumulate", "mth_quartet_fetch", "mth_mhl_accumulate", "mth_mhl_fetch", "mth_fdrp_accumulate", "mth_fdrp_fetch", "mth_multi_accumulate", "mth_multi_stats", "mth_lpmd_pairs_accumulate", "mth_lpmd_pairs_fetch", "mth_lpmd_intervals_fetch",
    "mth_mhl_regions_begin", "mth_mhl_regions_accumulate", "mth_mhl_regions_counts", "mth_mhl_regions_finalise", "mth_mhl_regions_fetch", "mth_mhl_regions_stats",
    "mth_pdr_regions_begin", "mth_pdr_regions_accumulate", "mth_pdr_regions_counts", "mth_pdr_regions_finalise", "mth_pdr_regions_fetch",
    "mth_quartet_regions_begin", "mth_quartet_regions_accumulate", "mth_quartet_regions_counts", "mth_quartet_regions_finalise", "mth_quartet_regions_fetch",
    "mth_decode_records", "mth_decode_set_cpg_filter", "mth_decode_set_xm_min_mapq", "mth_bgzf_inflate", "mth_bgzf_deflate", "mth_bgzf_decode", "mth_bgzf_decode_straddle", "mth_bgzf_straddle_scan", "mth_bgzf_straddle_rescan", "mth_bgzf_stage", "mth_decode_reserve", "mth_load_stats", "mth_decoded_fetch", "mth_decoded_contigs", "mth_decoded_sort", "mth_decoded_group", "mth_decoded_group_each", "mth_group_define", "mth_group_clear", "mth_fileorder_run", "mth_fileorder_fetch", "mth_decoded_batch", "mth_tag_set_genome", "mth_tag_records", "mth_tag_records_bam", "mth_bai_begin", "mth_bai_add_records", "mth_bai_finish", "mth_tag_set_genome_fasta", "mth_tag_genome_fetch", "mth_decode_set_genome", "mth_decode_set_modtags",
    "mth_timing_enable", "mth_timing_reset", "mth_timing_get", "mth_timing_num_kernels",
    "mth_timing_kernel_name",
]


class MthError(RuntimeError):
    def __init__(self, status, msg):
        super().__init__("metheor_hip error %d: %s" % (status, msg))
        self.status = status


class mth_batch_t(C.Structure):
    _fields_ = [("tid", C.c_int32), ("region_beg", C.c_int32), ("region_end", C.c_int32),
                ("max_span", C.c_int32), ("n_reads", C.c_uint32), ("n_cpgs", C.c_uint32),
                ("mem", C.c_int32),
                ("read_start", C.c_void_p), ("read_end", C.c_void_p), ("read_mapq", C.c_void_p),
                ("read_fwd", C.c_void_p), ("cpg_off", C.c_void_p), ("cpg_pos", C.c_void_p),
                ("cpg_rel", C.c_void_p), ("cpg_rel16", C.c_void_p)]


class mth_decoded_t(C.Structure):
    _fields_ = [("n_reads", C.c_uint64), ("n_cpgs", C.c_uint64), ("tid", C.c_void_p), ("start", C.c_void_p),
                ("end", C.c_void_p), ("mapq", C.c_void_p), ("fwd", C.c_void_p), ("cpg_off", C.c_void_p),
                ("cpg_pos", C.c_void_p), ("cpg_rel", C.c_void_p)]


class mth_fasta_blocks_t(C.Structure):
    _fields_ = [("coff", C.c_void_p), ("csize", C.c_void_p), ("isize", C.c_void_p), ("n_blocks", C.c_uint64)]


class mth_fasta_row_t(C.Structure):
    _fields_ = [("src_off", C.c_uint64), ("n_bases", C.c_int64), ("line_bases", C.c_int64), ("line_width", C.c_int64),
                ("name", C.c_char_p)]


class mth_pdr_lpmd_params_t(C.Structure):
    _fields_ = [("pdr_min_depth", C.c_uint32), ("pdr_min_cpgs", C.c_uint32),
                ("pdr_min_qual", C.c_uint8), ("lpmd_min_qual", C.c_uint8),
                ("want_pdr", C.c_uint8), ("want_lpmd", C.c_uint8),
                ("lpmd_min_distance", C.c_int32), ("lpmd_max_distance", C.c_int32)]


class mth_quartet_params_t(C.Structure):
    _fields_ = [("min_qual", C.c_uint8)]


class mth_mhl_params_t(C.Structure):
    _fields_ = [("min_depth", C.c_uint32), ("min_cpgs", C.c_uint32), ("min_qual", C.c_uint8)]


class mth_fdrp_params_t(C.Structure):
    _fields_ = [("min_depth", C.c_uint64), ("seed", C.c_uint64), ("max_depth", C.c_uint32),
                ("min_overlap", C.c_int32), ("min_qual", C.c_uint8)]


class mth_fileorder_params_t(C.Structure):
    _fields_ = [("measure", C.c_int32), ("min_depth", C.c_uint32), ("min_cpgs", C.c_uint32), ("max_depth", C.c_uint32),
                ("min_overlap", C.c_int32), ("min_qual", C.c_uint8), ("seed", C.c_uint64)]


class mth_lpmd_pairs_params_t(C.Structure):
    _fields_ = [("min_distance", C.c_int32), ("max_distance", C.c_int32), ("min_qual", C.c_uint8)]


MTH_MULTI_PDR, MTH_MULTI_LPMD, MTH_MULTI_QUARTET, MTH_MULTI_MHL, MTH_MULTI_FDRP, MTH_MULTI_PAIRS = 1, 2, 4, 8, 16, 32
MTH_MULTI_AUTO, MTH_MULTI_FUSED, MTH_MULTI_SPLIT = 0, 1, 2
MULTI_BITS = dict(pdr=MTH_MULTI_PDR, lpmd=MTH_MULTI_LPMD, quartet=MTH_MULTI_QUARTET, mhl=MTH_MULTI_MHL, fdrp=MTH_MULTI_FDRP,
                  pairs=MTH_MULTI_PAIRS)
MULTI_FORMS = dict(auto=MTH_MULTI_AUTO, fused=MTH_MULTI_FUSED, split=MTH_MULTI_SPLIT)


class mth_multi_params_t(C.Structure):
    _fields_ = [("want", C.c_uint32), ("pdr_lpmd", mth_pdr_lpmd_params_t), ("quartet", mth_quartet_params_t),
                ("mhl", mth_mhl_params_t), ("fdrp", mth_fdrp_params_t), ("pairs", mth_lpmd_pairs_params_t), ("form", C.c_int32)]


class mth_straddle_info_t(C.Structure):
    _fields_ = [("rounds", C.c_uint32), ("repaired_blocks", C.c_uint32), ("carry_bytes", C.c_uint64)]


class mth_load_stats_t(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("staged_calls", "inline_calls", "pieced_calls", "pieced_launches", "stage_misses", "decode_reallocs")]


MTH_STRADDLE_APPEND, MTH_STRADDLE_LAST, MTH_STRADDLE_DROP_TAIL = 1, 2, 4
MTH_STRADDLE_MAX_ROUNDS = 64
MTH_STRADDLE_ENTRY_GUESS = MTH_STRADDLE_EXIT_BAD = (1 << 64) - 1
MTH_STRADDLE_NO_START = 0xffffffff
MTH_STRADDLE_LOOKAHEAD = 36
# mth_straddle_row_t (and mth_host_straddle_row_t: one layout), as a numpy record
STRADDLE_ROW = np.dtype([("start", np.uint32), ("ref_id", np.int32), ("pos", np.int32), ("pad_", np.uint32), ("exit", np.uint64)])


class mth_straddle_run_t(C.Structure):
    _fields_ = [("entry", C.c_uint64), ("exit", C.c_uint64)]


class mth_tag_out_t(C.Structure):
    _fields_ = [("n_records", C.c_uint64), ("xm_off", C.c_void_p), ("xm_len", C.c_void_p), ("xm", C.c_void_p)]


class mth_tag_bam_out_t(C.Structure):
    _fields_ = [("n_records", C.c_uint64), ("n_blocks", C.c_uint64), ("stream_bytes", C.c_uint64), ("n_bytes", C.c_uint64),
                ("bytes", C.c_void_p), ("block_off", C.c_void_p)]


class mth_bai_out_t(C.Structure):
    _fields_ = [("n_refs", C.c_int32), ("n_records", C.c_uint64), ("n_chunks", C.c_uint64), ("chunk_beg", C.c_void_p), ("chunk_end", C.c_void_p),
                ("n_bins", C.c_uint64), ("bin_ref", C.c_void_p), ("bin_id", C.c_void_p), ("bin_n_chunks", C.c_void_p),
                ("ref_n_bins", C.c_void_p), ("ref_n_intv", C.c_void_p), ("lin_off", C.c_void_p), ("lin", C.c_void_p),
                ("meta", C.c_void_p), ("n_no_coor", C.c_uint64)]


BGZF_MAX_BLOCK = 0xff00


def library_path():
    # METHEOR_HIP_LIB: another build of the same library (A/B timing of kernel variants on one box)
    return os.environ.get("METHEOR_HIP_LIB") or os.path.join(_HERE, "libmetheor_hip.so")


def lib():
    """load libmetheor_hip.so; fails loudly when it has not been built (no fallback)"""
    global _LIB
    if _LIB is None:
        p = library_path()
        if not os.path.exists(p):
            raise ImportError("%s is missing: build it with `python -m metheor_amd.build` "
                              "(hipcc, gfx950). There is no CPU fallback." % p)
        # In a Python process PyTorch brings its own bundled ROCm runtime (libamdhip64.so.7 under
        # torch/lib).  Two HIP/HSA runtimes in one process break each other, so make sure torch's
        # is the one already loaded before this library's NEEDED libamdhip64.so.7 is resolved.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(p)
        vp = C.c_void_p
        L.mth_abi_version.restype = C.c_int
        L.mth_ctx_create.argtypes = [C.c_int, C.POINTER(vp)]
        L.mth_ctx_destroy.argtypes = [vp]; L.mth_ctx_destroy.restype = None
        L.mth_ctx_set_stream.argtypes = [vp, vp]
        L.mth_ctx_sync.argtypes = [vp]
        L.mth_strerror.restype = C.c_char_p; L.mth_strerror.argtypes = [C.c_int]
        L.mth_last_error.restype = C.c_char_p; L.mth_last_error.argtypes = [vp]
        L.mth_notes.restype = C.c_uint32; L.mth_notes.argtypes = [vp]
        L.mth_batch_prepare.argtypes = [vp, C.POINTER(mth_batch_t), C.POINTER(mth_batch_t)]
        L.mth_batch_release.argtypes = [vp, C.POINTER(mth_batch_t)]
        L.mth_reset.argtypes = [vp]
        L.mth_pdr_lpmd_accumulate.argtypes = [vp, C.POINTER(mth_batch_t), C.POINTER(mth_pdr_lpmd_params_t)]
        L.mth_pdr_count.argtypes = [vp, C.POINTER(C.c_uint64)]
        L.mth_pdr_fetch.argtypes = [vp] * 6
        L.mth_result_buffer_alloc.argtypes = [vp, C.c_size_t, C.POINTER(C.c_void_p)]
        L.mth_result_buffer_free.argtypes = [vp, vp]
        L.mth_pdr_device_view.argtypes = [vp, C.POINTER(C.c_uint64)] + [C.POINTER(vp)] * 4
        L.mth_lpmd_global.argtypes = [vp, C.POINTER(C.c_int64 * 4), C.POINTER(C.c_float)]
        L.mth_lpmd_add_unbatched.argtypes = [vp, C.c_uint64, C.c_uint64]
        L.mth_lpmd_from_counts.restype = C.c_float
        L.mth_lpmd_from_counts.argtypes = [C.c_int64, C.c_int64]
        L.mth_lpmd_export_device.argtypes = [vp, vp]
        L.mth_device_count.argtypes = [C.POINTER(C.c_int)]
        L.mth_allreduce_lpmd.argtypes = [C.POINTER(vp), C.c_int]
        L.mth_rccl_unique_id.argtypes = [vp]
        L.mth_rccl_init_rank.argtypes = [vp, vp, C.c_int, C.c_int]
        L.mth_allreduce_lpmd_rank.argtypes = [vp]
        L.mth_quartet_accumulate.argtypes = [vp, C.POINTER(mth_batch_t), C.POINTER(mth_quartet_params_t)]
        L.mth_quartet_fetch.argtypes = [vp, C.c_uint32, C.POINTER(C.c_uint64)] + [vp] * 5
        L.mth_mhl_accumulate.argtypes = [vp, C.POINTER(mth_batch_t), C.POINTER(mth_mhl_params_t)]
        L.mth_mhl_fetch.argtypes = [vp, C.POINTER(C.c_uint64)] + [vp] * 4
        L.mth_fdrp_accumulate.argtypes = [vp, C.POINTER(mth_batch_t), C.POINTER(mth_fdrp_params_t)]
        L.mth_fdrp_fetch.argtypes = [vp, C.POINTER(C.c_uint64)] + [vp] * 5
        L.mth_multi_accumulate.argtypes = [vp, C.POINTER(mth_batch_t), C.POINTER(mth_multi_params_t)]
        L.mth_multi_stats.argtypes = [vp, C.POINTER(C.c_uint64 * 4)]
        L.mth_lpmd_pairs_accumulate.argtypes = [vp, C.POINTER(mth_batch_t), C.POINTER(mth_lpmd_pairs_params_t)]
        L.mth_lpmd_pairs_fetch.argtypes = [vp, C.POINTER(C.c_uint64)] + [vp] * 6
        L.mth_lpmd_intervals_fetch.argtypes = [vp, C.c_uint64] + [vp] * 5
        L.mth_mhl_regions_begin.argtypes = [vp, C.c_uint64] + [vp] * 3
        L.mth_mhl_regions_accumulate.argtypes = [vp, C.POINTER(mth_batch_t), C.POINTER(mth_mhl_params_t)]
        L.mth_mhl_regions_counts.argtypes = [vp, C.POINTER(C.c_uint64)] + [vp] * 4
        L.mth_mhl_regions_finalise.restype = C.c_float
        L.mth_mhl_regions_finalise.argtypes = [C.c_uint64, vp, vp, vp, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]
        L.mth_mhl_regions_fetch.argtypes = [vp, C.c_uint32] + [vp] * 3
        L.mth_mhl_regions_stats.argtypes = [vp, C.POINTER(C.c_uint64 * 4)]
        L.mth_pdr_regions_begin.argtypes = [vp, C.c_uint64] + [vp] * 3
        L.mth_pdr_regions_accumulate.argtypes = [vp, C.POINTER(mth_batch_t), C.POINTER(mth_mhl_params_t)]
        L.mth_pdr_regions_counts.argtypes = [vp] + [vp] * 3
        L.mth_pdr_regions_finalise.restype = C.c_float
        L.mth_pdr_regions_finalise.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32]
        L.mth_pdr_regions_fetch.argtypes = [vp, C.c_uint32] + [vp] * 4
        L.mth_quartet_regions_begin.argtypes = [vp, C.c_uint64] + [vp] * 3
        L.mth_quartet_regions_accumulate.argtypes = [vp, C.POINTER(mth_batch_t), C.POINTER(mth_quartet_params_t)]
        L.mth_quartet_regions_counts.argtypes = [vp] + [vp] * 2
        L.mth_quartet_regions_finalise.restype = None
        L.mth_quartet_regions_finalise.argtypes = [vp, C.c_uint32] + [vp] * 3
        L.mth_quartet_regions_fetch.argtypes = [vp, C.c_uint32] + [vp] * 4
        L.mth_decode_records.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint64, C.c_int, C.c_int, C.POINTER(mth_decoded_t)]
        L.mth_decode_set_cpg_filter.argtypes = [vp, vp, C.c_uint64, C.c_int]
        L.mth_decode_set_xm_min_mapq.argtypes = [vp, C.c_uint32]
        L.mth_bgzf_inflate.argtypes = [vp, vp, C.c_uint64, vp, vp, vp, C.c_uint64, vp, C.POINTER(C.c_uint64)]
        L.mth_bgzf_deflate.argtypes = [vp, vp, C.c_uint64, C.c_int, vp, C.c_uint64, C.POINTER(vp), C.POINTER(C.c_uint64), C.POINTER(vp)]
        L.mth_bgzf_decode.argtypes = [vp, vp, C.c_uint64, vp, vp, vp, C.c_uint64, C.c_uint64, C.c_int, C.POINTER(mth_decoded_t)]
        L.mth_bgzf_decode_straddle.argtypes = [vp, vp, C.c_uint64, vp, vp, vp, C.c_uint64, C.c_uint64, C.c_uint, C.POINTER(mth_decoded_t),
                                               C.POINTER(mth_straddle_info_t)]
        L.mth_bgzf_straddle_scan.argtypes = [vp, vp, C.c_uint64, vp, vp, vp, C.c_uint64, C.c_uint64, C.c_uint64, vp, C.POINTER(mth_straddle_run_t),
                                             C.POINTER(mth_straddle_info_t)]
        L.mth_bgzf_straddle_rescan.argtypes = [vp, C.c_uint64, vp, C.POINTER(mth_straddle_run_t), C.POINTER(mth_straddle_info_t)]
        L.mth_bgzf_stage.argtypes = [vp, vp, C.c_uint64]
        L.mth_decode_reserve.argtypes = [vp, C.c_uint64, C.c_uint64]
        L.mth_load_stats.argtypes = [vp, C.POINTER(mth_load_stats_t)]
        L.mth_tag_set_genome.argtypes = [vp, C.c_int32, vp, vp, vp]
        L.mth_tag_set_genome_fasta.argtypes = [vp, vp, C.c_uint64, vp, C.c_int32, vp, vp]
        L.mth_tag_genome_fetch.argtypes = [vp, C.c_int32, C.c_int64, C.c_int64, vp]
        L.mth_tag_records.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint64, C.c_int, C.c_int, C.POINTER(mth_tag_out_t)]
        L.mth_tag_records_bam.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint64, C.c_int, C.c_int, C.POINTER(mth_tag_bam_out_t)]
        L.mth_bai_begin.argtypes = [vp, C.c_int32, vp, C.c_uint64]
        L.mth_bai_add_records.argtypes = [vp, vp, vp, C.c_uint64, C.c_int, vp, vp, C.c_uint64]
        L.mth_bai_finish.argtypes = [vp, C.POINTER(mth_bai_out_t)]
        L.mth_decode_set_genome.argtypes = [vp, C.c_int, C.c_int]
        L.mth_decode_set_modtags.argtypes = [vp, C.c_int, C.c_uint32]
        L.mth_decoded_fetch.argtypes = [vp] * 9
        L.mth_decoded_contigs.argtypes = [vp, C.c_uint32, vp, vp, vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        L.mth_decoded_sort.argtypes = [vp]
        L.mth_decoded_group.argtypes = [vp, C.c_uint32, vp, vp, vp, C.POINTER(C.c_uint32), vp, vp]
        if hasattr(L, "mth_decoded_group_each"):      # (METHEOR_HIP_LIB may name an older build: A/B runs)
            L.mth_decoded_group_each.argtypes = L.mth_decoded_group.argtypes
        L.mth_group_define.argtypes = [vp, C.c_uint32, vp, vp, C.POINTER(C.c_int32)]
        L.mth_group_clear.argtypes = [vp]
        L.mth_fileorder_run.argtypes = [vp, C.POINTER(mth_fileorder_params_t)]
        L.mth_fileorder_fetch.argtypes = [vp, C.POINTER(C.c_uint64)] + [vp] * 6
        L.mth_decoded_batch.argtypes = [vp, C.c_uint64, C.c_uint64, C.c_int32, C.c_int32, C.c_int32, C.POINTER(mth_batch_t)]
        L.mth_timing_enable.argtypes = [vp, C.c_int]
        L.mth_timing_reset.argtypes = [vp]
        L.mth_timing_get.argtypes = [vp, C.c_char_p, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
        L.mth_timing_num_kernels.restype = C.c_int
        L.mth_timing_kernel_name.restype = C.c_char_p; L.mth_timing_kernel_name.argtypes = [C.c_int]
        _LIB = L
    return _LIB


def mhl_regions_finalise(length, runs, reads, min_depth=10):
    """the host finaliser (mth_regions_host.h) of ONE interval from its sparse histogram rows of ascending length -> (mhl, n_reads,
    max_cpgs); no context, no device"""
    ln, ru, re_ = np.ascontiguousarray(length, np.uint32), np.ascontiguousarray(runs, np.uint64), np.ascontiguousarray(reads, np.uint64)
    assert ln.shape == ru.shape == re_.shape and ln.ndim == 1
    n, mx = C.c_uint64(0), C.c_uint32(0)
    v = lib().mth_mhl_regions_finalise(len(ln), *[x.ctypes.data_as(C.c_void_p) for x in (ln, ru, re_)], min_depth, C.byref(n), C.byref(mx))
    return np.float32(v), int(n.value), int(mx.value)


def pdr_regions_finalise(n_concordant, n_discordant, min_depth=10):
    """the host finaliser (mth_regions_host.h) of ONE interval's counters: pdr.rs:47-49 as float32, NaN below max(min_depth, 1)
    contributing reads; no context, no device"""
    return np.float32(lib().mth_pdr_regions_finalise(int(n_concordant), int(n_discordant), min_depth))


def quartet_regions_finalise(bins, min_depth=10):
    """the host finaliser (mth_regions_host.h) of ONE interval's sixteen bins: me.rs:42-55 and pm.rs:42-51 as float32, NaN below
    max(min_depth, 1) patterns -> (me, pm, n_patterns); no context, no device"""
    b = np.ascontiguousarray(bins, np.uint64)
    assert b.shape == (16,)
    me, pm, n = C.c_float(0), C.c_float(0), C.c_uint64(0)
    lib().mth_quartet_regions_finalise(b.ctypes.data_as(C.c_void_p), min_depth, C.byref(me), C.byref(pm), C.byref(n))
    return np.float32(me.value), np.float32(pm.value), int(n.value)


class PdrLpmdParams:
    """pdr.rs:82-89 / lpmd.rs:125-133 arguments with the reference's clap defaults (lib.rs)"""

    def __init__(self, min_depth=10, min_cpgs=4, min_qual=10, min_distance=2, max_distance=16,
                 lpmd_min_qual=10, want_pdr=True, want_lpmd=True):
        self.c = mth_pdr_lpmd_params_t(min_depth, min_cpgs, min_qual, lpmd_min_qual,
                                       int(want_pdr), int(want_lpmd), min_distance, max_distance)


def _is_torch(x):
    return type(x).__module__.startswith("torch")


class DeviceBatch:
    """an mth_batch_t filled in by the library (device pointers it owns)"""

    def __init__(self):
        self.c = mth_batch_t()


class PreparedBatch:
    """what Engine.batch_prepare returns: a batch (mem = MTH_MEM_PREPARED) every *_accumulate method takes in place of the original --
    device-resident, its read index built once and shared by the measures.  Keeps the original alive; release() frees the index and the
    device copies of a host batch; what is not released, the engine's close frees (the context keeps a registry of its prepared
    batches and validates a handle by look-up)."""

    def __init__(self, eng, orig):
        self.eng, self.orig = eng, orig
        self.c = mth_batch_t()
        eng._check(eng.L.mth_batch_prepare(eng.h, C.byref(orig.c), C.byref(self.c)))
        self.n_reads, self.n_cpgs, self.tid = orig.n_reads, orig.n_cpgs, orig.tid

    def release(self):
        if self.eng is not None and getattr(self.eng, "h", None):
            self.eng._check(self.eng.L.mth_batch_release(self.eng.h, C.byref(self.c)))
        self.eng = None


class Batch:
    """mth_batch_t over numpy arrays (host) or torch CUDA tensors (device); keeps them alive"""

    def __init__(self, tid, region_beg, region_end, read_start, read_end, read_mapq, cpg_off,
                 cpg_pos, cpg_rel, read_fwd=None, max_span=None):
        arrs = dict(read_start=read_start, read_end=read_end, read_mapq=read_mapq, cpg_off=cpg_off,
                    cpg_pos=cpg_pos, cpg_rel=cpg_rel, read_fwd=read_fwd)
        dev = _is_torch(read_start)
        self.keep = []
        ptr = {}
        want = dict(read_start=("int32", 4), read_end=("int32", 4), read_mapq=("uint8", 1),
                    cpg_off=("uint32", 4), cpg_pos=("uint32", 4), read_fwd=("uint8", 1))
        for k, a in arrs.items():
            if a is None:
                ptr[k] = None
                continue
            if dev:
                assert a.is_cuda and a.is_contiguous(), k
                if k == "cpg_rel":
                    assert a.element_size() in (1, 2)
                else:
                    assert a.element_size() == want[k][1], (k, a.dtype)
                self.keep.append(a)
                ptr[k] = a.data_ptr() if a.numel() else None
            else:
                if k == "cpg_rel":
                    a = np.ascontiguousarray(a)
                    assert a.dtype in (np.uint8, np.uint16), a.dtype
                else:
                    a = np.ascontiguousarray(a, dtype=want[k][0])
                self.keep.append(a)
                ptr[k] = a.ctypes.data if a.size else None
        rel = self.keep[[k for k, v in arrs.items() if v is not None].index("cpg_rel")]
        rel16 = (rel.element_size() if dev else rel.dtype.itemsize) == 2
        n_reads = int(read_start.shape[0])
        n_cpgs = int(cpg_pos.shape[0])
        if max_span is None:
            if dev:
                max_span = int((read_end - read_start).max().item()) + 1 if n_reads else 0
            else:
                max_span = int((np.asarray(read_end, np.int64) - np.asarray(read_start, np.int64)).max()) + 1 if n_reads else 0
        # a zero-length cpg_rel still has to say which width it is
        dummy = self.keep[0].data_ptr() if dev else self.keep[0].ctypes.data
        relp = ptr["cpg_rel"] or (dummy if n_reads else None)
        self.c = mth_batch_t(tid, region_beg, region_end, max(max_span, 0), n_reads, n_cpgs,
                             MTH_MEM_DEVICE if dev else MTH_MEM_HOST,
                             ptr["read_start"], ptr["read_end"], ptr["read_mapq"], ptr["read_fwd"],
                             ptr["cpg_off"], ptr["cpg_pos"],
                             None if rel16 else relp, relp if rel16 else None)
        self.n_reads, self.n_cpgs, self.tid = n_reads, n_cpgs, tid


class Engine:
    """one mth_ctx_t (one GPU).  Methods map 1:1 onto the C entry points."""

    def __init__(self, device=0, stream=None):
        self.L = lib()
        self.h = C.c_void_p()
        rc = self.L.mth_ctx_create(device, C.byref(self.h))
        if rc != 0:
            raise MthError(rc, self.L.mth_strerror(rc).decode())
        if stream is not None:
            self._check(self.L.mth_ctx_set_stream(self.h, C.c_void_p(stream)))
        # Batches whose kernels may still be queued or may be REPLAYED from their arrays at a later entry point (pipelined PDR + LPMD
        # batches; queued ME / PM and pairs batches: include/metheor_hip.h).  The engine keeps them alive until its next synchronising
        # call, so that a caller who drops or recycles a temporary batch right after the accumulate call cannot have the replay read
        # freed memory.  Keyed by id: a loop over one resident batch holds it once.
        self._inflight = {}
        self._stage_next = self._stage_flying = None     # bgzf_stage: the announced array, and the one a helper thread is reading

    def _hold(self, batch):
        self._inflight[id(batch)] = batch

    def _settled(self):
        self._inflight.clear()

    def close(self):
        if getattr(self, "h", None) and self.h:
            self.L.mth_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            msg = self.L.mth_strerror(rc).decode()
            last = self.L.mth_last_error(self.h).decode()
            raise MthError(rc, msg + (" (" + last + ")" if last else ""))

    def reset(self):
        self._check(self.L.mth_reset(self.h))

    def batch_prepare(self, batch):
        """one device-resident copy and ONE read index for all the measures of this batch (include/metheor_hip.h, "prepared batches")"""
        return PreparedBatch(self, batch)

    def notes(self):
        """non-fatal findings of the device decode so far (bit 0: a CIGAR P operation was decoded; bit 1: under
        decode_set_modtags a record without SEQ, with a hard clip or with MN != l_seq contributed no call)"""
        return int(self.L.mth_notes(self.h))

    def sync(self):
        self._check(self.L.mth_ctx_sync(self.h))
        self._settled()

    def pdr_lpmd_accumulate(self, batch, params):
        self._hold(batch)
        self._check(self.L.mth_pdr_lpmd_accumulate(self.h, C.byref(batch.c), C.byref(params.c)))

    def pdr_count(self):
        n = C.c_uint64(0)
        self._check(self.L.mth_pdr_count(self.h, C.byref(n)))
        self._settled()
        return n.value

    def pdr_fetch(self):
        n = self.pdr_count()
        out = dict(tid=np.zeros(n, np.int32), pos=np.zeros(n, np.int32), pdr=np.zeros(n, np.float32),
                   n_concordant=np.zeros(n, np.uint32), n_discordant=np.zeros(n, np.uint32))
        self._check(self.L.mth_pdr_fetch(self.h, *[out[k].ctypes.data_as(C.c_void_p) for k in
                                                   ("tid", "pos", "pdr", "n_concordant", "n_discordant")]))
        return out

    def lpmd_global(self):
        g = (C.c_int64 * 4)()
        v = C.c_float(0)
        self._check(self.L.mth_lpmd_global(self.h, C.byref(g), C.byref(v)))
        self._settled()
        return dict(n_concordant=g[0], n_discordant=g[1], n_read=g[2], n_valid_read=g[3],
                    lpmd=np.float32(v.value))

    def lpmd_add_unbatched(self, n_read, n_valid_read):
        """records left out of the batches (no contig / no aligned base): lpmd.rs:176-179 still counts them"""
        self._check(self.L.mth_lpmd_add_unbatched(self.h, int(n_read), int(n_valid_read)))

    def lpmd_export_device(self, dst_ptr):
        """dst_ptr: device address of 4 x int64 (e.g. torch_tensor.data_ptr())"""
        self._check(self.L.mth_lpmd_export_device(self.h, C.c_void_p(dst_ptr)))

    # ---- the exchange step (mth_rccl.hip): one RCCL all-reduce of the four LPMD counters ----
    @staticmethod
    def rccl_unique_id():
        """128 bytes made by rank 0; ship them to every rank (torch.distributed.broadcast, MPI, a file)"""
        buf = (C.c_uint8 * 128)()
        rc = lib().mth_rccl_unique_id(C.cast(buf, C.c_void_p))
        if rc != 0:
            raise MthError(rc, lib().mth_strerror(rc).decode())
        return bytes(buf)

    def rccl_init_rank(self, unique_id, rank, world):
        assert len(unique_id) == 128
        buf = (C.c_uint8 * 128).from_buffer_copy(unique_id)
        self._check(self.L.mth_rccl_init_rank(self.h, C.cast(buf, C.c_void_p), int(rank), int(world)))

    def allreduce_lpmd_rank(self):
        """collective over the ranks of rccl_init_rank, enqueued on this context's stream; afterwards lpmd_global()
        returns the node-wide counters"""
        self._check(self.L.mth_allreduce_lpmd_rank(self.h))

    def lpmd_from_counts(self, n_conc, n_disc):
        return np.float32(self.L.mth_lpmd_from_counts(int(n_conc), int(n_disc)))

    def quartet_accumulate(self, batch, min_qual=10):
        p = mth_quartet_params_t(min_qual)
        self._hold(batch)
        self._check(self.L.mth_quartet_accumulate(self.h, C.byref(batch.c), C.byref(p)))

    def quartet_fetch(self, min_depth=10):
        """rows (depth >= min_depth) of the HashMap<Quartet,...>: tid, pos[n,4], cnt[n,16], me, pm"""
        n = C.c_uint64(0)
        self._check(self.L.mth_quartet_fetch(self.h, min_depth, C.byref(n), None, None, None, None, None))
        self._settled()
        k = n.value
        out = dict(tid=np.zeros(k, np.int32), pos=np.zeros((k, 4), np.int32), cnt=np.zeros((k, 16), np.uint32),
                   me=np.zeros(k, np.float32), pm=np.zeros(k, np.float32))
        self._check(self.L.mth_quartet_fetch(self.h, min_depth, C.byref(n), *[out[x].ctypes.data_as(C.c_void_p) for x in
                                                                              ("tid", "pos", "cnt", "me", "pm")]))
        return out

    def mhl_accumulate(self, batch, min_depth=10, min_cpgs=4, min_qual=10):
        p = mth_mhl_params_t(min_depth, min_cpgs, min_qual)
        self._check(self.L.mth_mhl_accumulate(self.h, C.byref(batch.c), C.byref(p)))

    def mhl_fetch(self):
        n = C.c_uint64(0)
        self._check(self.L.mth_mhl_fetch(self.h, C.byref(n), None, None, None, None))
        k = n.value
        out = dict(tid=np.zeros(k, np.int32), pos=np.zeros(k, np.int32), mhl=np.zeros(k, np.float32), cov=np.zeros(k, np.uint32))
        self._check(self.L.mth_mhl_fetch(self.h, C.byref(n), *[out[x].ctypes.data_as(C.c_void_p) for x in ("tid", "pos", "mhl", "cov")]))
        return out

    def fdrp_accumulate(self, batch, min_qual=10, min_depth=10, max_depth=40, min_overlap=35, seed=0):
        p = mth_fdrp_params_t(min_depth, seed, max_depth, min_overlap, min_qual)
        self._check(self.L.mth_fdrp_accumulate(self.h, C.byref(batch.c), C.byref(p)))

    def fdrp_fetch(self):
        n = C.c_uint64(0)
        self._check(self.L.mth_fdrp_fetch(self.h, C.byref(n), None, None, None, None, None))
        k = n.value
        out = dict(tid=np.zeros(k, np.int32), pos=np.zeros(k, np.int32), fdrp=np.zeros(k, np.float32),
                   qfdrp=np.zeros(k, np.float32), n_reads=np.zeros(k, np.uint32))
        self._check(self.L.mth_fdrp_fetch(self.h, C.byref(n), *[out[x].ctypes.data_as(C.c_void_p) for x in
                                                                ("tid", "pos", "fdrp", "qfdrp", "n_reads")]))
        return out

    def multi_accumulate(self, batch, want=("pdr", "lpmd", "quartet", "mhl", "fdrp"), form="auto", min_depth=10, min_cpgs=4,
                         min_qual=10, min_distance=2, max_distance=16, max_depth=40, min_overlap=35, seed=0):
        """every measure of `want` (names of MULTI_BITS) over ONE batch, the read index built once (mth_multi_accumulate): the results are
        read with the measures' own *_fetch / lpmd_global methods.  The parameters are the CLI's, shared by the measures that have them
        (`metheor all`); ME / PM take their min_depth at the fetch.  Synchronous."""
        bits = 0
        for w in ([want] if isinstance(want, str) else want):
            bits |= MULTI_BITS[w]
        p = mth_multi_params_t()
        p.want = bits
        p.pdr_lpmd = mth_pdr_lpmd_params_t(min_depth, min_cpgs, min_qual, min_qual, 0, 0, min_distance, max_distance)
        p.quartet = mth_quartet_params_t(min_qual)
        p.mhl = mth_mhl_params_t(min_depth, min_cpgs, min_qual)
        p.fdrp = mth_fdrp_params_t(min_depth, seed, max_depth, min_overlap, min_qual)
        p.pairs = mth_lpmd_pairs_params_t(min_distance, max_distance, min_qual)
        p.form = MULTI_FORMS[form] if isinstance(form, str) else int(form)
        self._check(self.L.mth_multi_accumulate(self.h, C.byref(batch.c), C.byref(p)))
        self._settled()

    def multi_stats(self):
        """batches fused / split, tiles fused / handed back by multi_accumulate since the last reset"""
        out = (C.c_uint64 * 4)()
        self._check(self.L.mth_multi_stats(self.h, C.byref(out)))
        return dict(batches_fused=out[0], batches_split=out[1], tiles_fused=out[2], tiles_handed_back=out[3])

    def lpmd_pairs_accumulate(self, batch, min_distance=2, max_distance=16, min_qual=10):
        p = mth_lpmd_pairs_params_t(min_distance, max_distance, min_qual)
        self._hold(batch)
        self._check(self.L.mth_lpmd_pairs_accumulate(self.h, C.byref(batch.c), C.byref(p)))

    def lpmd_pairs_fetch(self):
        n = C.c_uint64(0)
        self._check(self.L.mth_lpmd_pairs_fetch(self.h, C.byref(n), None, None, None, None, None, None))
        self._settled()
        k = n.value
        out = dict(tid=np.zeros(k, np.int32), pos1=np.zeros(k, np.int32), pos2=np.zeros(k, np.int32),
                   lpmd=np.zeros(k, np.float32), n_concordant=np.zeros(k, np.uint32), n_discordant=np.zeros(k, np.uint32))
        self._check(self.L.mth_lpmd_pairs_fetch(self.h, C.byref(n), *[out[x].ctypes.data_as(C.c_void_p) for x in
                                                                      ("tid", "pos1", "pos2", "lpmd", "n_concordant", "n_discordant")]))
        return out

    def lpmd_intervals_fetch(self, tid, beg, end):
        """the pairs table accumulated so far, reduced on the device by interval [beg, end) of contig tid (0-based, half-open): exact
        int64 sums of the rows with beg <= cpg1 and cpg2 < end, and lpmd = lpmd_from_counts of the two (lpmd.rs:51-55)"""
        t, b, e = (np.ascontiguousarray(x, np.int32) for x in (tid, beg, end))
        assert t.ndim == 1 and t.shape == b.shape == e.shape
        k = len(t)
        out = dict(n_concordant=np.zeros(k, np.int64), n_discordant=np.zeros(k, np.int64))
        self._check(self.L.mth_lpmd_intervals_fetch(self.h, k, *[x.ctypes.data_as(C.c_void_p) for x in
                                                                 (t, b, e, out["n_concordant"], out["n_discordant"])]))
        self._settled()
        out["lpmd"] = np.array([self.L.mth_lpmd_from_counts(int(c), int(d)) for c, d in zip(out["n_concordant"], out["n_discordant"])],
                               np.float32)
        return out

    # ---- MHL per interval (mth_mhl_regions.hip) ----
    def mhl_regions_begin(self, tid, beg, end):
        """declare the intervals [beg, end) of contig tid (0-based, half-open; any order, overlap, nesting, duplicates) and clear the sums"""
        t, b, e = (np.ascontiguousarray(x, np.int32) for x in (tid, beg, end))
        assert t.ndim == 1 and t.shape == b.shape == e.shape
        self._mr_n = len(t)
        self._check(self.L.mth_mhl_regions_begin(self.h, len(t), *[x.ctypes.data_as(C.c_void_p) for x in (t, b, e)]))
        self._settled()

    def mhl_regions_accumulate(self, batch, min_cpgs=4, min_qual=10):
        """the batch's OWNED reads (region_beg <= read_start < region_end) into the histograms of every declared interval (mhl.rs:176-183
        after readutil.rs:87-94 with the interval's positions); synchronous"""
        p = mth_mhl_params_t(0, min_cpgs, min_qual)
        self._check(self.L.mth_mhl_regions_accumulate(self.h, C.byref(batch.c), C.byref(p)))
        self._settled()

    def mhl_regions_counts(self):
        """the two histograms as sparse rows sorted by (interval, length): runs = maximal methylated runs of that length, reads =
        contributing reads with that many kept calls.  Shards add these."""
        n = C.c_uint64(0)
        self._check(self.L.mth_mhl_regions_counts(self.h, C.byref(n), None, None, None, None))
        k = n.value
        out = dict(interval=np.empty(k, np.uint32), length=np.empty(k, np.uint32), runs=np.empty(k, np.uint64), reads=np.empty(k, np.uint64))
        if k:
            self._check(self.L.mth_mhl_regions_counts(self.h, C.byref(n), *[out[c].ctypes.data_as(C.c_void_p) for c in ("interval", "length", "runs", "reads")]))
        self._settled()
        return out

    def mhl_regions_fetch(self, min_depth=10):
        """per declared interval: mhl (compute_mhl, mhl.rs:43-73; NaN below max(min_depth, 1) contributing reads), n_reads, max_cpgs"""
        k = self._mr_n
        out = dict(mhl=np.empty(k, np.float32), n_reads=np.empty(k, np.uint64), max_cpgs=np.empty(k, np.uint32))
        self._check(self.L.mth_mhl_regions_fetch(self.h, min_depth, *[out[c].ctypes.data_as(C.c_void_p) for c in ("mhl", "n_reads", "max_cpgs")]))
        self._settled()
        return out

    def mhl_regions_stats(self):
        """overflow-list entries so far, batches run a second time for a list that was too short, batches, reads of those batches"""
        out = (C.c_uint64 * 4)()
        self._check(self.L.mth_mhl_regions_stats(self.h, C.byref(out)))
        return [int(x) for x in out]

    # ---- PDR per interval (mth_pdr_regions.hip) ----
    def pdr_regions_begin(self, tid, beg, end):
        """declare the intervals [beg, end) of contig tid (0-based, half-open; any order, overlap, nesting, duplicates) and clear the sums"""
        t, b, e = (np.ascontiguousarray(x, np.int32) for x in (tid, beg, end))
        assert t.ndim == 1 and t.shape == b.shape == e.shape
        self._pr_n = len(t)
        self._check(self.L.mth_pdr_regions_begin(self.h, len(t), *[x.ctypes.data_as(C.c_void_p) for x in (t, b, e)]))
        self._settled()

    def pdr_regions_accumulate(self, batch, min_cpgs=4, min_qual=10):
        """the batch's OWNED reads (region_beg <= read_start < region_end) into the three counters of every declared interval
        (pdr.rs:147-157 after readutil.rs:87-94 with the interval's positions, then readutil.rs:134-145); queued, not waited for:
        data errors surface at the counts / fetch"""
        p = mth_mhl_params_t(0, min_cpgs, min_qual)
        self._hold(batch)
        self._check(self.L.mth_pdr_regions_accumulate(self.h, C.byref(batch.c), C.byref(p)))

    def pdr_regions_counts(self):
        """per declared interval: contributing reads that are methylated, unmethylated, discordant.  Shards add these."""
        k = self._pr_n
        out = dict(methylated=np.empty(k, np.uint64), unmethylated=np.empty(k, np.uint64), discordant=np.empty(k, np.uint64))
        self._check(self.L.mth_pdr_regions_counts(self.h, *[out[c].ctypes.data_as(C.c_void_p) for c in ("methylated", "unmethylated", "discordant")]))
        self._settled()
        return out

    def pdr_regions_fetch(self, min_depth=10):
        """per declared interval: pdr (pdr.rs:47-49; NaN below max(min_depth, 1) contributing reads), n_concordant, n_discordant,
        n_methylated (the methylated among the concordant)"""
        k = self._pr_n
        out = dict(pdr=np.empty(k, np.float32), n_concordant=np.empty(k, np.uint64), n_discordant=np.empty(k, np.uint64), n_methylated=np.empty(k, np.uint64))
        self._check(self.L.mth_pdr_regions_fetch(self.h, min_depth, *[out[c].ctypes.data_as(C.c_void_p) for c in ("pdr", "n_concordant", "n_discordant", "n_methylated")]))
        self._settled()
        return out

    # ---- ME / PM per interval (mth_quartet_regions.hip) ----
    def quartet_regions_begin(self, tid, beg, end):
        """declare the intervals [beg, end) of contig tid (0-based, half-open; any order, overlap, nesting, duplicates) and clear the sums"""
        t, b, e = (np.ascontiguousarray(x, np.int32) for x in (tid, beg, end))
        assert t.ndim == 1 and t.shape == b.shape == e.shape
        self._qr_n = len(t)
        self._check(self.L.mth_quartet_regions_begin(self.h, len(t), *[x.ctypes.data_as(C.c_void_p) for x in (t, b, e)]))
        self._settled()

    def quartet_regions_accumulate(self, batch, min_qual=10):
        """the batch's OWNED reads (region_beg <= read_start < region_end) into the sixteen bins and the reads word of every declared
        interval (me.rs:115-125 after readutil.rs:87-94 with the interval's positions, then readutil.rs:97-132); queued, not waited
        for: data errors surface at the counts / fetch"""
        p = mth_quartet_params_t(min_qual)
        self._hold(batch)
        self._check(self.L.mth_quartet_regions_accumulate(self.h, C.byref(batch.c), C.byref(p)))

    def quartet_regions_counts(self):
        """per declared interval: bins[i, p] = windows of pattern p, reads[i] = contributing reads.  Shards add these."""
        k = self._qr_n
        out = dict(bins=np.empty((k, 16), np.uint64), reads=np.empty(k, np.uint64))
        self._check(self.L.mth_quartet_regions_counts(self.h, *[out[c].ctypes.data_as(C.c_void_p) for c in ("bins", "reads")]))
        self._settled()
        return out

    def quartet_regions_fetch(self, min_depth=10):
        """per declared interval: me (me.rs:42-55) and pm (pm.rs:42-51) of its pooled histogram, NaN below max(min_depth, 1)
        patterns; n_patterns, n_reads"""
        k = self._qr_n
        out = dict(me=np.empty(k, np.float32), pm=np.empty(k, np.float32), n_patterns=np.empty(k, np.uint64), n_reads=np.empty(k, np.uint64))
        self._check(self.L.mth_quartet_regions_fetch(self.h, min_depth, *[out[c].ctypes.data_as(C.c_void_p) for c in ("me", "pm", "n_patterns", "n_reads")]))
        self._settled()
        return out

    # ---- device-side BAM record decode (mth_decode.hip) ----
    def decode_records(self, raw, rec_off, append=False):
        """raw: the inflated BAM record stream (numpy uint8 / bytes, or a torch CUDA uint8 tensor); rec_off: uint64
        byte offsets of the records (n + 1).  The decoded SoA stays on the device; returns (n_reads, n_cpgs)."""
        dev = _is_torch(raw)
        if dev:
            assert raw.is_cuda and raw.is_contiguous() and rec_off.is_cuda and rec_off.is_contiguous()
            self._dec_keep = (raw, rec_off)
            rp, op, nb, nr = raw.data_ptr(), rec_off.data_ptr(), raw.numel(), rec_off.numel() - 1
        else:
            raw = np.frombuffer(raw, np.uint8) if isinstance(raw, (bytes, bytearray, memoryview)) else np.ascontiguousarray(raw, np.uint8)
            rec_off = np.ascontiguousarray(rec_off, np.uint64)
            self._dec_keep = (raw, rec_off)
            rp, op, nb, nr = raw.ctypes.data, rec_off.ctypes.data, raw.size, rec_off.size - 1
        d = mth_decoded_t()
        self._check(self.L.mth_decode_records(self.h, rp, nb, op, max(nr, 0), 1 if dev else 0, int(bool(append)), C.byref(d)))
        self._decoded = d
        return int(d.n_reads), int(d.n_cpgs)

    def bgzf_inflate(self, file_bytes, coff, csize, isize):
        """inflate the given BGZF blocks on the device; returns the concatenated inflated bytes (numpy uint8)"""
        fb = np.frombuffer(file_bytes, np.uint8) if isinstance(file_bytes, (bytes, bytearray, memoryview)) else np.ascontiguousarray(file_bytes, np.uint8)
        coff = np.ascontiguousarray(coff, np.uint64); csize = np.ascontiguousarray(csize, np.uint32); isize = np.ascontiguousarray(isize, np.uint32)
        out = np.zeros(int(isize.astype(np.uint64).sum()), np.uint8)
        n = C.c_uint64(0)
        self._stage_started()
        self._check(self.L.mth_bgzf_inflate(self.h, fb.ctypes.data, fb.size, coff.ctypes.data, csize.ctypes.data, isize.ctypes.data,
                                            len(coff), out.ctypes.data, C.byref(n)))
        assert n.value == len(out)
        return out

    def bgzf_deflate(self, data, cuts=None):
        """data (bytes / uint8 array, host) as BGZF blocks made on the device (k_deflate), back to back, without the EOF block;
        cuts: ascending offsets from 0 to len(data), at most 0xff00 apart (default: every 0xff00 bytes).  -> bytes"""
        src = np.frombuffer(data, np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else np.ascontiguousarray(data, np.uint8)
        if cuts is None:
            cuts = list(range(0, src.size, BGZF_MAX_BLOCK)) + [src.size] if src.size else [0]
        cut = np.ascontiguousarray(cuts, np.uint64)
        out, n, boff = C.c_void_p(), C.c_uint64(0), C.c_void_p()
        self._check(self.L.mth_bgzf_deflate(self.h, src.ctypes.data if src.size else None, src.size, MTH_MEM_HOST, cut.ctypes.data,
                                            len(cut) - 1, C.byref(out), C.byref(n), C.byref(boff)))
        return C.string_at(out.value, n.value) if n.value else b""

    def bgzf_decode(self, file_bytes, coff, csize, isize, first_byte, append=False):
        """file_bytes: the BAM file (bytes / uint8 array, host); coff/csize/isize: per-BGZF-block payload offset, payload
        size, inflated size.  Inflate + record walk + decode on the device; returns (n_reads, n_cpgs)."""
        fb = np.frombuffer(file_bytes, np.uint8) if isinstance(file_bytes, (bytes, bytearray, memoryview)) else np.ascontiguousarray(file_bytes, np.uint8)
        coff = np.ascontiguousarray(coff, np.uint64); csize = np.ascontiguousarray(csize, np.uint32); isize = np.ascontiguousarray(isize, np.uint32)
        d = mth_decoded_t()
        self._stage_started()
        self._check(self.L.mth_bgzf_decode(self.h, fb.ctypes.data, fb.size, coff.ctypes.data, csize.ctypes.data, isize.ctypes.data,
                                           len(coff), int(first_byte), int(bool(append)), C.byref(d)))
        self._decoded = d
        return int(d.n_reads), int(d.n_cpgs)

    def bgzf_stage(self, file_bytes, n_bytes=None):
        """announce file_bytes as the chunk AFTER the one the next bgzf_decode / bgzf_inflate call is given (mth_bgzf_stage): that
        call starts a helper thread that copies it to the device on a side stream, and the call after it, given the SAME pointer and
        size, takes the copy.  file_bytes must be a contiguous np.uint8 array -- a slice of one array keeps base + offset, so pass
        the very view (or an equal slice of the same array) to the following bgzf_decode; a `bytes` slice is a copy somewhere else
        and would never match, so bytes are refused.  n_bytes: announce only the first n_bytes of it (default: all); 0, or
        file_bytes None, withdraws the announcement.  The engine holds the array while the helper thread may read it: from here
        until the inflating call after next has joined the thread (_stage_started)."""
        if file_bytes is None:
            fb, n = None, 0
        else:
            if not (isinstance(file_bytes, np.ndarray) and file_bytes.dtype == np.uint8 and file_bytes.flags["C_CONTIGUOUS"]):
                raise TypeError("bgzf_stage takes a contiguous np.uint8 array (a view of the array the next chunk is decoded from)")
            fb, n = file_bytes, file_bytes.size if n_bytes is None else int(n_bytes)
            assert 0 <= n <= fb.size
        self._stage_next = fb
        self._check(self.L.mth_bgzf_stage(self.h, fb.ctypes.data if n else None, n))

    def _stage_started(self):
        """at every call that inflates: the library joins the helper thread of the call before and starts one for the announcement"""
        self._stage_flying, self._stage_next = self._stage_next, None

    def decode_reserve(self, n_reads, n_cpgs):
        """size the decoded arrays for n_reads / n_cpgs in total; what is decoded so far is kept (mth_decode_reserve)"""
        self._check(self.L.mth_decode_reserve(self.h, int(n_reads), int(n_cpgs)))

    def load_stats(self):
        """which way the load calls went since the engine's creation or the last reset (mth_load_stats): inflate calls that took
        the staged buffer / copied in line / copied in pieces, k_inflate launches of the pieced calls, announcements copied but not
        taken, growths of the decoded arrays"""
        st = mth_load_stats_t()
        self._check(self.L.mth_load_stats(self.h, C.byref(st)))
        return {k: int(getattr(st, k)) for k, _ in mth_load_stats_t._fields_}

    def bgzf_decode_straddle(self, file_bytes, coff, csize, isize, first_byte, append=False, last=False, drop_tail=False):
        """bgzf_decode for a file whose records straddle BGZF blocks (mth_bgzf_decode_straddle).  A call whose stream ends inside a
        record keeps that record's bytes on the device for the next append=True call; last=True: the stream ends here (an unfinished
        record is an error); drop_tail=True: it ends here and an unfinished last record is dropped.
        -> (n_reads, n_cpgs, dict(rounds, repaired_blocks, carry_bytes)); the dict is also self.straddle_info, set before an error is
        raised"""
        fb = np.frombuffer(file_bytes, np.uint8) if isinstance(file_bytes, (bytes, bytearray, memoryview)) else np.ascontiguousarray(file_bytes, np.uint8)
        coff = np.ascontiguousarray(coff, np.uint64); csize = np.ascontiguousarray(csize, np.uint32); isize = np.ascontiguousarray(isize, np.uint32)
        flags = (MTH_STRADDLE_APPEND if append else 0) | (MTH_STRADDLE_LAST if last else 0) | (MTH_STRADDLE_DROP_TAIL if drop_tail else 0)
        d, info = mth_decoded_t(), mth_straddle_info_t()
        self._stage_started()
        rc = self.L.mth_bgzf_decode_straddle(self.h, fb.ctypes.data, fb.size, coff.ctypes.data, csize.ctypes.data, isize.ctypes.data,
                                             len(coff), int(first_byte), flags, C.byref(d), C.byref(info))
        self.straddle_info = dict(rounds=int(info.rounds), repaired_blocks=int(info.repaired_blocks), carry_bytes=int(info.carry_bytes))
        self._check(rc)
        self._decoded = d
        return int(d.n_reads), int(d.n_cpgs), self.straddle_info

    def bgzf_straddle_scan(self, file_bytes, coff, csize, isize, n_run, entry=None):
        """mth_bgzf_straddle_scan: the record chain of the first n_run of the given blocks (the rest is look-ahead), nothing decoded.
        entry: offset in the run's stream, None = a guess.
        -> (rows: STRADDLE_ROW array of n_run, dict(entry -- None: the first block found no guess --, exit -- None: the chain does
        not go on --, rounds, repaired_blocks)); the context keeps the run for bgzf_straddle_rescan"""
        fb = np.frombuffer(file_bytes, np.uint8) if isinstance(file_bytes, (bytes, bytearray, memoryview)) else np.ascontiguousarray(file_bytes, np.uint8)
        coff = np.ascontiguousarray(coff, np.uint64); csize = np.ascontiguousarray(csize, np.uint32); isize = np.ascontiguousarray(isize, np.uint32)
        rows = np.zeros(int(n_run), STRADDLE_ROW)
        run, info = mth_straddle_run_t(), mth_straddle_info_t()
        self._scan_rows = int(n_run)
        self._stage_started()
        self._check(self.L.mth_bgzf_straddle_scan(self.h, fb.ctypes.data, fb.size, coff.ctypes.data, csize.ctypes.data, isize.ctypes.data, len(coff),
                                                  int(n_run), MTH_STRADDLE_ENTRY_GUESS if entry is None else int(entry), rows.ctypes.data,
                                                  C.byref(run), C.byref(info)))
        return rows, self._scan_summary(run, info)

    def bgzf_straddle_rescan(self, entry):
        """mth_bgzf_straddle_rescan: the run of the latest bgzf_straddle_scan again, from the exact entry -> as bgzf_straddle_scan"""
        rows = np.zeros(self._scan_rows, STRADDLE_ROW)
        run, info = mth_straddle_run_t(), mth_straddle_info_t()
        self._check(self.L.mth_bgzf_straddle_rescan(self.h, int(entry), rows.ctypes.data, C.byref(run), C.byref(info)))
        return rows, self._scan_summary(run, info)

    @staticmethod
    def _scan_summary(run, info):
        return dict(entry=None if run.entry == MTH_STRADDLE_ENTRY_GUESS else int(run.entry), exit=None if run.exit == MTH_STRADDLE_EXIT_BAD else int(run.exit),
                    rounds=int(info.rounds), repaired_blocks=int(info.repaired_blocks))

    def tag_set_genome(self, contigs):
        """contigs: [(header LN, bases as bytes)] in tid order (mth_tag_set_genome; tag.rs:419-431)"""
        n = len(contigs)
        ln = (C.c_int64 * max(n, 1))(*[int(c[0]) for c in contigs])
        got = (C.c_int64 * max(n, 1))(*[len(c[1]) for c in contigs])
        bufs = [np.frombuffer(bytes(c[1]), np.uint8) for c in contigs]
        ptr = (C.c_void_p * max(n, 1))(*[b.ctypes.data if len(b) else None for b in bufs])
        self._check(self.L.mth_tag_set_genome(self.h, n, ln, ptr, got))

    def tag_set_genome_fasta(self, file_bytes, ref_len, rows, blocks=None):
        """mth_tag_set_genome_fasta: the genome packed on the device from the FASTA file's bytes (bytes / uint8 array, host).
        ref_len: the header's LN per contig; rows: per contig (src_off, n_bases, line_bases, line_width[, name]) or objects with
        those attributes (hostapi.FastaRow); blocks: None for plain text, (coff, csize, isize) of a BGZF file"""
        fb = np.frombuffer(file_bytes, np.uint8) if isinstance(file_bytes, (bytes, bytearray, memoryview)) else np.ascontiguousarray(file_bytes, np.uint8)
        n = len(rows)
        ln = (C.c_int64 * max(n, 1))(*[int(x) for x in ref_len])
        rr = (mth_fasta_row_t * max(n, 1))()
        for i, r in enumerate(rows):
            t = r if isinstance(r, (tuple, list)) else (r.src_off, r.n_bases, r.line_bases, r.line_width, r.name)
            rr[i].src_off, rr[i].n_bases, rr[i].line_bases, rr[i].line_width = int(t[0]), int(t[1]), int(t[2]), int(t[3])
            nm = t[4] if len(t) > 4 else None
            rr[i].name = nm.encode() if isinstance(nm, str) else nm
        bp, keep = None, None
        if blocks is not None:
            coff = np.ascontiguousarray(blocks[0], np.uint64); csize = np.ascontiguousarray(blocks[1], np.uint32); isize = np.ascontiguousarray(blocks[2], np.uint32)
            keep = (coff, csize, isize)
            b = mth_fasta_blocks_t(coff.ctypes.data, csize.ctypes.data, isize.ctypes.data, len(coff))
            bp = C.addressof(b)
        self._check(self.L.mth_tag_set_genome_fasta(self.h, fb.ctypes.data if fb.size else None, fb.size, bp, n, ln, rr))
        del keep

    def tag_genome_fetch(self, tid, beg, n):
        """mth_tag_genome_fetch: n bases of contig tid from base beg on, as the device genome holds them -> bytes"""
        out = np.zeros(int(n), np.uint8)
        self._check(self.L.mth_tag_genome_fetch(self.h, int(tid), int(beg), int(n), out.ctypes.data if n else None))
        return out.tobytes()

    def tag_records(self, raw, rec_off, is_paired_end=False):
        """raw: the inflated BAM records (bytes), rec_off: uint64[n_rec + 1]; -> list of XM strings (bytes), tag.rs:130-384"""
        rb = np.frombuffer(raw, np.uint8)
        off = np.ascontiguousarray(rec_off, np.uint64)
        t = mth_tag_out_t()
        n = len(off) - 1
        self._check(self.L.mth_tag_records(self.h, rb.ctypes.data if len(rb) else None, len(rb), off.ctypes.data, max(n, 0), 0,
                                           int(bool(is_paired_end)), C.byref(t)))
        if n <= 0:
            return []
        xo = np.ctypeslib.as_array(C.cast(t.xm_off, C.POINTER(C.c_uint64)), shape=(n + 1,))
        xl = np.ctypeslib.as_array(C.cast(t.xm_len, C.POINTER(C.c_uint32)), shape=(n,))
        return [C.string_at(t.xm + int(xo[i]), int(xl[i])) for i in range(n)]

    def tag_records_bam(self, raw, rec_off, is_paired_end=False):
        """tag_records' arguments; -> (the window's tagged records as BGZF blocks (bytes, no EOF block), size of the tagged record
        stream, number of blocks): every record with XM:Z appended as its last field, assembled and deflated on the device"""
        rb = np.frombuffer(raw, np.uint8)
        off = np.ascontiguousarray(rec_off, np.uint64)
        t = mth_tag_bam_out_t()
        n = len(off) - 1
        self._check(self.L.mth_tag_records_bam(self.h, rb.ctypes.data if len(rb) else None, len(rb), off.ctypes.data, max(n, 0), 0,
                                               int(bool(is_paired_end)), C.byref(t)))
        return (C.string_at(t.bytes, t.n_bytes) if t.n_bytes else b""), int(t.stream_bytes), int(t.n_blocks)

    def bai_begin(self, ref_len, file_off=0):
        """mth_bai_begin: start a .bai index over references of these lengths; file_off: where the next block tag_records_bam makes
        will lie in the file (every tag_records_bam call up to bai_finish indexes its window)"""
        ln = np.ascontiguousarray(ref_len, np.int64)
        self._check(self.L.mth_bai_begin(self.h, len(ln), ln.ctypes.data if len(ln) else None, int(file_off)))

    def bai_add_records(self, raw, rec_off, cuts, block_coff):
        """mth_bai_add_records: records (bytes + uint64[n_rec + 1] offsets, host) cut into blocks at the stream offsets `cuts`
        (n_blocks + 1), block b at file offset block_coff[b]"""
        rb = np.frombuffer(raw, np.uint8) if isinstance(raw, (bytes, bytearray, memoryview)) else np.ascontiguousarray(raw, np.uint8)
        off = np.ascontiguousarray(rec_off, np.uint64)
        cut = np.ascontiguousarray(cuts, np.uint64); coff = np.ascontiguousarray(block_coff, np.uint64)
        assert len(cut) == len(coff) + 1
        n = max(len(off) - 1, 0)
        self._check(self.L.mth_bai_add_records(self.h, rb.ctypes.data if rb.size else None, off.ctypes.data if n else None, n, MTH_MEM_HOST,
                                               cut.ctypes.data, coff.ctypes.data if len(coff) else None, len(coff)))

    def bai_finish(self):
        """mth_bai_finish -> dict: n_refs, n_records, n_no_coor and the tables as numpy arrays (copies) -- chunk_beg / chunk_end
        (sorted by (refID, bin)), bin_ref / bin_id / bin_n_chunks, ref_n_bins, ref_n_intv, lin_off, lin, meta (n_refs x 4)"""
        t = mth_bai_out_t()
        self._check(self.L.mth_bai_finish(self.h, C.byref(t)))
        def arr(p, ct, dt, k):
            return np.ctypeslib.as_array(C.cast(p, C.POINTER(ct)), shape=(k,)).astype(dt, copy=True) if k and p else np.zeros(0, dt)
        nr, nc, nb = int(t.n_refs), int(t.n_chunks), int(t.n_bins)
        lin_off = arr(t.lin_off, C.c_uint64, np.uint64, nr + 1)
        return dict(n_refs=nr, n_records=int(t.n_records), n_no_coor=int(t.n_no_coor),
                    chunk_beg=arr(t.chunk_beg, C.c_uint64, np.uint64, nc), chunk_end=arr(t.chunk_end, C.c_uint64, np.uint64, nc),
                    bin_ref=arr(t.bin_ref, C.c_int32, np.int32, nb), bin_id=arr(t.bin_id, C.c_uint32, np.uint32, nb),
                    bin_n_chunks=arr(t.bin_n_chunks, C.c_uint32, np.uint32, nb), ref_n_bins=arr(t.ref_n_bins, C.c_uint32, np.uint32, nr),
                    ref_n_intv=arr(t.ref_n_intv, C.c_uint32, np.uint32, nr), lin_off=lin_off if nr else np.zeros(1, np.uint64),
                    lin=arr(t.lin, C.c_uint64, np.uint64, int(lin_off[-1]) if nr else 0), meta=arr(t.meta, C.c_uint64, np.uint64, nr * 4).reshape(nr, 4))

    def decode_set_genome(self, enabled, is_paired_end=False):
        """derive the calls of the following decode_records / bgzf_decode calls from the genome of tag_set_genome instead of
        the records' XM:Z -- what `metheor tag` followed by the decode computes (mth_decode_set_genome)"""
        self._check(self.L.mth_decode_set_genome(self.h, int(bool(enabled)), int(bool(is_paired_end))))

    def decode_set_modtags(self, enabled, threshold=128):
        """take the calls of the following decode_records / bgzf_decode calls from the records' MM:Z / ML:B:C base-modification
        tags instead of XM:Z; a listed C with ML >= threshold (0..255) is methylated (mth_decode_set_modtags)"""
        self._check(self.L.mth_decode_set_modtags(self.h, int(bool(enabled)), int(threshold)))

    def decoded_fetch(self):
        d = self._decoded
        nr, nc = int(d.n_reads), int(d.n_cpgs)
        out = dict(tid=np.zeros(nr, np.int32), start=np.zeros(nr, np.int32), end=np.zeros(nr, np.int32),
                   mapq=np.zeros(nr, np.uint8), fwd=np.zeros(nr, np.uint8), cpg_off=np.zeros(nr + 1, np.uint64),
                   cpg_pos=np.zeros(nc, np.uint32), cpg_rel=np.zeros(nc, np.uint16))
        self._check(self.L.mth_decoded_fetch(self.h, *[out[k].ctypes.data_as(C.c_void_p) for k in
                                                       ("tid", "start", "end", "mapq", "fwd", "cpg_off", "cpg_pos", "cpg_rel")]))
        return out

    def decode_set_cpg_filter(self, sites):
        """sites: iterable of (tid, pos) or None (no filter); an empty iterable filters every call"""
        if sites is None:
            self._check(self.L.mth_decode_set_cpg_filter(self.h, None, 0, 0))
            return
        keys = np.array(sorted({(int(t) << 32) | (int(p) & 0xffffffff) for t, p in sites}), np.uint64)
        self._check(self.L.mth_decode_set_cpg_filter(self.h, keys.ctypes.data if len(keys) else None, len(keys), 1))

    def decoded_contigs(self, cap=65536):
        """runs of equal tid in the decoded stream: (tids, read_beg, read_end, flags)"""
        tids, beg, end = np.zeros(cap, np.int32), np.zeros(cap, np.uint64), np.zeros(cap, np.uint64)
        n, fl = C.c_uint32(0), C.c_uint32(0)
        self._check(self.L.mth_decoded_contigs(self.h, cap, tids.ctypes.data, beg.ctypes.data, end.ctypes.data, C.byref(n), C.byref(fl)))
        k = min(n.value, cap)
        return tids[:k], beg[:k], end[:k], fl.value

    def group_define(self, tids, voff):
        """contigs `tids` laid out at virtual offsets `voff` (ascending): the handle to use as the tid of their one batch"""
        t, v = np.ascontiguousarray(tids, np.int32), np.ascontiguousarray(voff, np.int64)
        assert len(t) == len(v)
        h = C.c_int32(0)
        self._check(self.L.mth_group_define(self.h, len(t), t.ctypes.data, v.ctypes.data, C.byref(h)))
        self.__dict__.setdefault("_groups", {})[h.value] = (t.copy(), v.copy())
        return h.value

    def group_copy(self, other, handle):
        """define on this engine the group `handle` of engine `other` (must come out under the same handle)"""
        g = other._groups[handle]
        assert self.group_define(*g) == handle

    def group_clear(self):
        self._check(self.L.mth_group_clear(self.h))

    def decoded_group(self, tids, read_beg, read_end, each=False):
        """pack the decoded stream's contigs into groups (positions shifted in place): [(batch_tid, read_beg, read_end, [tids])], [] if not grouped;
        each: one contig per group (mth_decoded_group_each)"""
        t = np.ascontiguousarray(tids, np.int32); b = np.ascontiguousarray(read_beg, np.uint64); e = np.ascontiguousarray(read_end, np.uint64)
        n = len(t)
        first, bt, ng = np.zeros(n + 1, np.uint32), np.zeros(max(n, 1), np.int32), C.c_uint32(0)
        self._check((self.L.mth_decoded_group_each if each else self.L.mth_decoded_group)(self.h, n, t.ctypes.data, b.ctypes.data, e.ctypes.data, C.byref(ng), first.ctypes.data, bt.ctypes.data))
        return [(int(bt[g]), int(b[first[g]]), int(e[first[g + 1] - 1]), [int(x) for x in t[first[g]:first[g + 1]]]) for g in range(ng.value)]

    def decoded_sort(self):
        """the decoded stream re-ordered by (tid, start) on the device (order-free measures on unsorted input)"""
        self._check(self.L.mth_decoded_sort(self.h))

    def fileorder(self, measure, min_depth=10, min_cpgs=4, min_qual=10, max_depth=40, min_overlap=35, seed=0):
        """PDR (0) / MHL (1) / FDRP + qFDRP (2) of the decoded stream in FILE order: the reference's stream semantics on input that is
        not coordinate-sorted (mth_fileorder.hip); rows sorted by (tid, pos)"""
        p = mth_fileorder_params_t(int(measure), int(min_depth), int(min_cpgs), int(max_depth), int(min_overlap), int(min_qual), int(seed))
        self._check(self.L.mth_fileorder_run(self.h, C.byref(p)))
        n = C.c_uint64(0)
        self._check(self.L.mth_fileorder_fetch(self.h, C.byref(n), None, None, None, None, None, None))
        k = n.value
        out = dict(tid=np.zeros(k, np.int32), pos=np.zeros(k, np.int32), v0=np.zeros(k, np.float32), v1=np.zeros(k, np.float32),
                   c0=np.zeros(k, np.uint32), c1=np.zeros(k, np.uint32))
        self._check(self.L.mth_fileorder_fetch(self.h, C.byref(n), *[out[x].ctypes.data_as(C.c_void_p) for x in ("tid", "pos", "v0", "v1", "c0", "c1")]))
        return out

    def decoded_batch(self, read_beg, read_end, tid, region_beg, region_end):
        """device-resident batch over reads [read_beg, read_end) of the decoded stream (one contig)"""
        b = DeviceBatch()
        self._check(self.L.mth_decoded_batch(self.h, int(read_beg), int(read_end), int(tid), int(region_beg), int(region_end), C.byref(b.c)))
        return b

    def timing_enable(self, on=True):
        self._check(self.L.mth_timing_enable(self.h, int(on)))

    def timing_reset(self):
        self._check(self.L.mth_timing_reset(self.h))

    def timing(self):
        out = {}
        for i in range(self.L.mth_timing_num_kernels()):
            name = self.L.mth_timing_kernel_name(i)
            ms, n = C.c_double(0), C.c_uint64(0)
            self._check(self.L.mth_timing_get(self.h, name, C.byref(ms), C.byref(n)))
            out[name.decode()] = (ms.value, n.value)
        return out


def device_count():
    n = C.c_int(0)
    lib().mth_device_count(C.byref(n))
    return n.value


def allreduce_lpmd(engines):
    """one process, one Engine per GPU (or several per GPU): one RCCL all-reduce of the four LPMD counters between the
    distinct devices; afterwards every engine's lpmd_global() returns the totals"""
    arr = (C.c_void_p * len(engines))(*[e.h for e in engines])
    rc = lib().mth_allreduce_lpmd(arr, len(engines))
    if rc != 0:
        engines[0]._check(rc)
