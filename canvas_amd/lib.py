"""ctypes binding of libcanvas_hip.so.  Device memory is handled with torch tensors (plumbing only)."""
import sys
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(HERE, "libcanvas_hip.so")
_SYNTH_SO = os.path.join(HERE, "libcanvas_synth.so")

MODE_BINARY, MODE_TDR, MODE_GCW = 0, 3, 5
SELECT_MEDIAN_F32, SELECT_MEDIAN_F64, SELECT_UPPER = 0, 1, 2
LOGISTIC_GERMLINE = (-5.0123, 4.9801, -5.5472, -1.7914)      # QualityScoreParameters.cs: LogisticGermline{Intercept, LogBinCount, ModelDistance, DistanceRatio}
FILTER_Q10, FILTER_L10KB = 1, 2
CLEAN_GCNORM, CLEAN_FILTSIZE, CLEAN_OUTLIERS, CLEAN_LOCALSD, CLEAN_LOESS = 1, 2, 4, 8, 16

# every symbol include/canvas_hip.h declares (checked by tests/test_abi.py)
ABI_SYMBOLS = [
    "canvas_create", "canvas_destroy", "canvas_last_error", "canvas_version", "canvas_set_stream", "canvas_set_one_shot", "canvas_synchronize",
    "canvas_device_malloc", "canvas_device_free", "canvas_memcpy_h2d", "canvas_memcpy_d2h", "canvas_host_register", "canvas_host_unregister", "canvas_upload_genome_begin", "canvas_upload_genome_wait",
    "canvas_packed_plane_bytes", "canvas_pack_reference_host", "canvas_pack_hits_host", "canvas_pack_genome_device", "canvas_upload_packed_begin", "canvas_bin_sample_packed", "canvas_sample_pipeline_packed", "canvas_pack_hits2_host", "canvas_upload_packed2_begin",
    "canvas_mask_from_fasta", "canvas_mask_exclude_intervals", "canvas_screen_hits",
    "canvas_bin_rates", "canvas_bin_size_from_rates", "canvas_bin_count_upper_bound", "canvas_bin_genome", "canvas_bin_sample", "canvas_bin_sample_gcweighted", "canvas_bin_predefined", "canvas_bin_predefined_gcweighted",
    "canvas_clean", "canvas_clean2", "canvas_clean_batch", "canvas_merge_cleaned", "canvas_chromosome_offsets", "canvas_quantize_f2", "canvas_hmm_per_sample", "canvas_hmm_joint", "canvas_segment_ids", "canvas_segment_ids_filtered", "canvas_segment_ids_ploidy", "canvas_evenness_score", "canvas_split_overlapping", "canvas_cbs", "canvas_cbs_undo", "canvas_cbs_device_stats", "canvas_cbs_tailp_stats", "canvas_cbs_tail_probe", "canvas_cbs_boundary", "canvas_cbs_seeds", "canvas_cbs_prefetch", "canvas_cbs_stream_read", "canvas_cbs_cache_stats", "canvas_wavelets", "canvas_wavelets_stats", "canvas_wavelets_decisions", "canvas_wavelets_inputs", "canvas_wavelets_prefix_probe", "canvas_wavelets_bound_probe", "canvas_wavelets_level_probe", "canvas_wavelets_chain_probe", "canvas_wavelets_subtree_probe", "canvas_wavelets_median_probe", "canvas_normalize_reference", "canvas_normalize_ratio", "canvas_normalize_best_normal", "canvas_normalize_pca_reference", "canvas_sample_pipeline",
    "canvas_comm_unique_id", "canvas_comm_init", "canvas_comm_init_host", "canvas_allgather_boundaries", "canvas_sample_pipeline_sharded", "canvas_sample_pipeline_sharded_packed", "canvas_sharded_stats", "canvas_cbs_sharded", "canvas_wavelets_sharded", "canvas_allgather_host", "canvas_merge_cleaned_sharded", "canvas_profile_enable", "canvas_profile_get", "canvas_bin_gcw_stats", "canvas_cbs_tpermp_stats", "canvas_comm_split", "canvas_comm_restore", "canvas_comm_rank", "canvas_bin_sample_sharded", "canvas_hmm_per_sample_sharded", "canvas_cbs_perm_probe", "canvas_cbs_arc_probe", "canvas_stale_reads", "canvas_select_probe", "canvas_hmm_backbone_probe",
    "canvas_memcpy_h2d_async", "canvas_snv_count", "canvas_flag_unique_kmers", "canvas_fasta_case_from_mask",
    "canvas_smooth", "canvas_smooth_lengths", "canvas_smooth_plan",
    "canvas_segment_select", "canvas_segment_select_plan", "canvas_call_diploid",
    "canvas_somatic_model_fit", "canvas_call_somatic",
    "canvas_segment_tables", "canvas_call_diploid_ids",
    "canvas_partition_states_cbs", "canvas_partition_states_breakpoints", "canvas_reference_copy_numbers", "canvas_call_somatic_ids",
    "canvas_hits_from_bam", "canvas_fragments_from_bam",
    "canvas_bgzf_inflate", "canvas_bgzf_scan",
    "canvas_bam_frame", "canvas_memcpy_d2d_async",
    "canvas_bgzf_crc32",
]


SOMATIC_TILE, SOMATIC_MAX_CN = 256, 10                        # CANVAS_SOMATIC_TILE (segments per tile of the model-fit kernel), CANVAS_SOMATIC_MAX_CN
ERR_SOMATIC_NO_MODEL, ERR_SOMATIC_NO_SCORE = -6, -7
SOMATIC_INFO_CLUSTER_TERM, SOMATIC_INFO_INDEX_CUTOFF = 1, 2
SOMATIC_MODEL_VALID, SOMATIC_MODEL_SCORED = 1, 2
# SomaticCallerParameters.json, as far as Canvas.somatic_model_fit reads it
SOMATIC_DEFAULTS = dict(maximum_copy_number=8, deviation_index_cutoff=11, maximum_related_models=5, min_allowed_ploidy=0.5, max_allowed_ploidy=8.0, deviation_factor=1.75,
                        cn2_weighting_factor=0.175, deviation_score_weighting_factor=0.375, diploid_distance_score_weighting_factor=0.125,
                        heterogeneity_score_weighting_factor=0.202)


class SomaticParams(C.Structure):
    _fields_ = [("maximum_copy_number", C.c_int32), ("deviation_index_cutoff", C.c_int32), ("maximum_related_models", C.c_int32),
                ("min_allowed_ploidy", C.c_float), ("max_allowed_ploidy", C.c_float), ("deviation_factor", C.c_float),
                ("cn2_weighting_factor", C.c_double), ("deviation_score_weighting_factor", C.c_double), ("diploid_distance_score_weighting_factor", C.c_double),
                ("heterogeneity_score_weighting_factor", C.c_double)]


class SomaticGrid(C.Structure):
    _fields_ = [("min_coverage", C.c_int32), ("max_coverage", C.c_int32), ("minimum_purity_hard_limit", C.c_int32), ("fixed_percent_purity", C.c_int32),
                ("fixed_coverage", C.c_int32), ("is_enrichment", C.c_int32), ("min_minor_allele_coverage", C.c_double), ("coverage_weighting_factor", C.c_double),
                ("genome_length", C.c_int64)]


class SomaticResult(C.Structure):
    _fields_ = [("best_model", C.c_int32), ("best_coverage", C.c_int32), ("best_percent_purity", C.c_int32), ("info", C.c_uint32),
                ("nmodels", C.c_int32), ("nvalid", C.c_int32), ("nscored", C.c_int32), ("reserved", C.c_int32),
                ("diploid_coverage", C.c_double), ("purity", C.c_double), ("deviation", C.c_double), ("precision_deviation", C.c_double), ("accuracy_deviation", C.c_double),
                ("ploidy", C.c_double), ("percent_normal", C.c_double), ("diploid_distance", C.c_double), ("percent_cn", C.c_double * (SOMATIC_MAX_CN + 1)),
                ("score", C.c_double), ("inter_model_distance", C.c_double), ("best_deviation", C.c_double), ("worst_allowed_deviation", C.c_double),
                ("host_table_ms", C.c_double), ("upload_ms", C.c_double), ("device_ms", C.c_double), ("selection_ms", C.c_double)]


class SomaticModels(C.Structure):
    _fields_ = [("capacity", C.c_int64), ("coverage", C.c_void_p), ("percent_purity", C.c_void_p), ("deviation", C.c_void_p), ("precision_deviation", C.c_void_p),
                ("accuracy_deviation", C.c_void_p), ("ploidy", C.c_void_p), ("percent_normal", C.c_void_p), ("percent_cn", C.c_void_p), ("diploid_distance", C.c_void_p),
                ("flags", C.c_void_p), ("score", C.c_void_p)]


ERR_SOMATIC_FEW_SEGMENTS = -8                                  # CANVAS_ERR_SOMATIC_FEW_SEGMENTS
SOMATIC_MEAN_NONE, SOMATIC_MEAN_WALK, SOMATIC_MEAN_EXACT = -1, 0, 1
# what Canvas.call_somatic reads beside SOMATIC_DEFAULTS: SomaticCallerParameters.json, QualityScoreParameters.cs:9-12, SomaticCaller.cs:70
SOMATIC_CALL_DEFAULTS = dict(minimum_variant_frequencies=50, minimum_call_size=50000, quality_filter_threshold=10, merge_span=1, is_enrichment=0, minimum_purity_hard_limit=20,
                             lower_coverage_level_weighting_factor=4.0, upper_coverage_level_weighting_factor=2.355, user_purity=-1.0, user_ploidy=-1.0,
                             coverage_weighting=0.333, coverage_weighting_with_maf_segmentation=0.20, evenness_score_threshold=94.5, min_evenness_score=88.0,
                             logistic_intercept=-0.5143, logistic_log_bin_count=0.8596, logistic_model_distance=-50.4366, logistic_distance_ratio=-0.6511,
                             evenness_score=float("nan"), snv_purity_estimate=float("nan"), min_minor_allele_coverage=0.0, genome_length=0)


class SomaticCallParams(C.Structure):
    _fields_ = [("fit", SomaticParams), ("minimum_variant_frequencies", C.c_int32), ("minimum_call_size", C.c_int32), ("quality_filter_threshold", C.c_int32),
                ("merge_span", C.c_int32), ("is_enrichment", C.c_int32), ("minimum_purity_hard_limit", C.c_int32),
                ("lower_coverage_level_weighting_factor", C.c_float), ("upper_coverage_level_weighting_factor", C.c_float), ("user_purity", C.c_float), ("user_ploidy", C.c_float),
                ("coverage_weighting", C.c_double), ("coverage_weighting_with_maf_segmentation", C.c_double), ("evenness_score_threshold", C.c_double),
                ("min_evenness_score", C.c_double), ("logistic_intercept", C.c_double), ("logistic_log_bin_count", C.c_double), ("logistic_model_distance", C.c_double),
                ("logistic_distance_ratio", C.c_double), ("evenness_score", C.c_double), ("snv_purity_estimate", C.c_double), ("min_minor_allele_coverage", C.c_double),
                ("genome_length", C.c_int64)]


# (field, numpy dtype, "seg" | "seg1" (nseg + 1) | "run") in the order of canvas_somatic_call_out
SOMATIC_CALL_OUT = [("seg_median_count", np.float64, "seg"), ("seg_site_offset", np.int64, "seg1"), ("seg_maf_upper", np.float64, "seg"), ("seg_usable", np.int32, "seg"),
                    ("seg_coverage", np.float64, "seg"), ("seg_maf", np.float64, "seg"), ("seg_weight", np.float64, "seg"), ("seg_cn", np.int32, "seg"), ("seg_cn2", np.int32, "seg"),
                    ("seg_mcc", np.int32, "seg"), ("seg_dist", np.float64, "seg"), ("seg_dist2", np.float64, "seg"), ("seg_mean_count", np.float64, "seg"),
                    ("seg_mean_route", np.int32, "seg"), ("seg_qscore", np.int32, "seg"), ("seg_run", np.int64, "seg"), ("run_owner", np.int64, "run"), ("run_begin", np.int32, "run"),
                    ("run_end", np.int32, "run"), ("run_bin_count", np.int64, "run"), ("run_qscore", np.int32, "run"), ("run_filter", np.int32, "run")]


class SomaticCallOut(C.Structure):
    _fields_ = [(name, C.c_void_p) for name, _, _ in SOMATIC_CALL_OUT]


class SomaticCallScalars(C.Structure):
    _fields_ = [("nruns", C.c_int64), ("nusable", C.c_int64), ("kept_sites", C.c_int64), ("stages", C.c_int32), ("threshold_used", C.c_int32),
                ("median_coverage_level", C.c_int32), ("min_coverage", C.c_int32), ("max_coverage", C.c_int32), ("fixed_percent_purity", C.c_int32),
                ("overall_median_coverage", C.c_float), ("deviation_factor", C.c_float), ("mean_coverage", C.c_double), ("coverage_weighting_factor", C.c_double),
                ("reported_purity", C.c_double), ("purity_model_fit", C.c_double), ("inter_model_distance", C.c_double), ("estimated_chromosome_count", C.c_double),
                ("heterogeneity_proportion", C.c_double), ("stage1_ms", C.c_double), ("stage23_ms", C.c_double), ("stage4_ms", C.c_double), ("stage5_ms", C.c_double),
                ("stage6_ms", C.c_double)]


def somatic_grid(min_coverage, max_coverage, minimum_purity_hard_limit, min_minor_allele_coverage, fixed_percent_purity=-1, fixed_coverage=-1):
    """the (diploid coverage, percent purity) models of the search in its order (SomaticCaller.cs:1899-1914), as canvas_somatic_model_fit lays them out"""
    lo, hi = (fixed_coverage, fixed_coverage) if fixed_coverage >= 0 else (min_coverage, max_coverage)
    models = []
    for cov in range(lo, hi + 1):
        p0 = int(max(float(minimum_purity_hard_limit), 100 * (1 - 2 * min_minor_allele_coverage / cov) - 10))
        p0, p1 = (fixed_percent_purity, fixed_percent_purity) if fixed_percent_purity >= 0 else (p0, 100)
        models += [(cov, p) for p in range(p0, p1 + 1)]
    return models


BACKBONE_PROBE_UNTOUCHED = 0x7FF8C0DEC0DEC0DE     # bits of the carries canvas_hmm_backbone_probe leaves alone (a quiet NaN no sum produces)


class CanvasError(RuntimeError):
    pass


# canvas_bgzf_block (24 bytes) and the block statuses of canvas_bgzf_inflate
BGZF_BLOCK = np.dtype([("src_offset", "<u8"), ("dst_offset", "<u8"), ("src_bytes", "<u4"), ("out_bytes", "<u4")])
INFLATE_OK, INFLATE_DESCRIPTOR, INFLATE_HEADER, INFLATE_INPUT, INFLATE_OVERRUN, INFLATE_SHORT, INFLATE_DISTANCE, INFLATE_CODE = range(8)
BGZF_SCAN_LIMIT, BGZF_SCAN_END, BGZF_SCAN_DAMAGED = 0, 1, 2
CRC_OK, CRC_MISMATCH, CRC_DESCRIPTOR, CRC_SKIPPED = range(4)                  # the block statuses of canvas_bgzf_crc32
# canvas_bam_frame_rule (16 bytes), its kinds, and the events of canvas_bam_frame
BAM_FRAME_RULE = np.dtype([("kind", "<i4"), ("ref_id", "<i4"), ("paired_end", "<i4"), ("sorted", "<i4")])
BAM_FRAME_ALL, BAM_FRAME_SNV, BAM_FRAME_HITS, BAM_FRAME_FRAGMENTS = 0, 1, 2, 3
BAM_FRAME_NONE, BAM_FRAME_STOPPED, BAM_FRAME_MALFORMED, BAM_FRAME_UNSORTED, BAM_FRAME_CAPACITY = 0, 1, 2, 3, 4


def bgzf_scan(buf, at=0, max_out_bytes=None):
    """The descriptors of the consecutive BGZF blocks of `buf` (bytes-like or a uint8 array, host memory) from byte `at` on, until their inflated sizes reach
    max_out_bytes (None: no bound).  Returns (blocks, info): a numpy array of BGZF_BLOCK, ready for Canvas.bgzf_inflate with `buf` as the source, and info[4] = blocks,
    the file offset the walk stopped at, their inflated bytes, and why it stopped (BGZF_SCAN_LIMIT / _END / _DAMAGED).  Host code: no context, no device call."""
    lib = load_library()
    a = np.frombuffer(buf, np.uint8) if not isinstance(buf, np.ndarray) else np.ascontiguousarray(buf).view(np.uint8).reshape(-1)
    if not 0 <= int(at) <= a.size:
        raise CanvasError("bgzf_scan: `at` lies outside the buffer")
    cap = (a.size - int(at)) // 26 + 1            # the walk takes a block of 26 bytes (18 of header, no data, 8 of trailer)
    blocks = np.zeros(cap, BGZF_BLOCK)
    info = np.zeros(4, np.int64)
    limit = (1 << 64) - 1 if max_out_bytes is None else int(max_out_bytes)
    rc = lib.canvas_bgzf_scan(C.c_void_p(a.ctypes.data), C.c_uint64(a.size), C.c_uint64(int(at)), C.c_uint64(limit), _np_ptr(blocks), C.c_int64(cap), _np_ptr(info))
    if rc != 0:
        raise CanvasError("canvas_bgzf_scan failed (%d)" % rc)
    return blocks[:int(info[0])].copy(), info


_lib = None


def load_library():
    """Loads the HIP library; fails loudly if it has not been built (python -m canvas_amd.build)."""
    global _lib
    if _lib is not None:
        return _lib
    # torch wheels bundle their own HIP runtime (SONAME libamdhip64.so.7): load torch FIRST so that the dynamic loader binds
    # this library to the runtime torch already loaded (one runtime per process, shared device pointers and streams).
    import torch  # noqa: F401
    if not os.path.exists(_SO):
        raise CanvasError(f"{_SO} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(there is no CPU fallback)")
    lib = C.CDLL(_SO)
    lib.canvas_create.restype = C.c_void_p
    lib.canvas_create.argtypes = [C.c_int]
    lib.canvas_destroy.argtypes = [C.c_void_p]
    lib.canvas_last_error.restype = C.c_char_p
    lib.canvas_last_error.argtypes = [C.c_void_p]
    lib.canvas_version.restype = C.c_char_p
    lib.canvas_set_stream.argtypes = [C.c_void_p, C.c_void_p]
    lib.canvas_synchronize.argtypes = [C.c_void_p]
    lib.canvas_device_malloc.restype = C.c_void_p
    lib.canvas_device_malloc.argtypes = [C.c_void_p, C.c_int64]
    lib.canvas_device_free.argtypes = [C.c_void_p, C.c_void_p]
    lib.canvas_memcpy_h2d.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]
    lib.canvas_memcpy_d2h.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]
    lib.canvas_bin_count_upper_bound.restype = C.c_int64
    lib.canvas_bin_count_upper_bound.argtypes = [C.c_int32, C.c_void_p, C.c_int32]
    lib.canvas_bin_size_from_rates.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
    lib.canvas_packed_plane_bytes.argtypes = [C.c_int64, C.c_void_p, C.c_void_p]
    lib.canvas_pack_reference_host.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32]
    lib.canvas_pack_hits_host.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32]
    lib.canvas_pack_hits2_host.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32]
    _lib = lib
    return lib


def _ptr_table(tensors):
    T = C.c_void_p * len(tensors)
    return T(*[t.data_ptr() for t in tensors])


def _np_ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def packed_plane_words(length):
    """64-position words of the packed planes of one chromosome (whole tiles of 4096 positions): the reference planes hold 2 u64 per word, the hit planes 4"""
    return ((int(length) + 4095) // 4096) * 64


def _host_addr(a):
    return C.c_void_p(a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data)


def pack_reference_host(bases, mask, length, out=None, threads=0):
    """canvas_pack_reference_host (plain host code, no GPU): (bases u8[len], mask u64[ceil(len/64)]) -> ({possible, gc} u64 pairs, pos0).
    Arrays are numpy arrays or (pinned) CPU torch tensors; `out` = u64[2 * packed_plane_words(len)]"""
    lib = load_library()
    if out is None:
        out = np.zeros(2 * packed_plane_words(length), np.uint64)
    p0 = C.c_int64(0)
    rc = lib.canvas_pack_reference_host(_host_addr(bases), _host_addr(mask), C.c_int64(int(length)), _host_addr(out), C.byref(p0), int(threads))
    if rc:
        raise CanvasError(f"canvas_pack_reference_host: error {rc}")
    return out, p0.value


def pack_hits_host(hits, length, out=None, threads=0):
    """canvas_pack_hits_host (plain host code, no GPU): hits u8[len] -> bit-sliced 4-bit planes u64[4 * packed_plane_words(len)]; returns (planes, #saturated positions)"""
    lib = load_library()
    if out is None:
        out = np.zeros(4 * packed_plane_words(length), np.uint64)
    sat = C.c_int64(0)
    rc = lib.canvas_pack_hits_host(_host_addr(hits), C.c_int64(int(length)), _host_addr(out), C.byref(sat), int(threads))
    if rc:
        raise CanvasError(f"canvas_pack_hits_host: error {rc}")
    return out, sat.value


def pack_hits2_host(hits, length, lo=None, hdr=None, extras=None, threads=0):
    """canvas_pack_hits2_host (plain host code): hits u8[len] -> the two-bit wire form (lo u64[2 W], hdr u64[2 W / 64], extras u64[2 n_extras]); returns
    (lo, hdr, extras, n_extras, #saturated).  The extras buffer is sized W / 16 entries unless given; it is grown once if the sample needs more."""
    lib = load_library()
    W = packed_plane_words(length)
    lo = np.zeros(2 * W, np.uint64) if lo is None else lo
    hdr = np.zeros(2 * (W // 64), np.uint64) if hdr is None else hdr
    extras = np.zeros(2 * (W // 16 + 64), np.uint64) if extras is None else extras
    for attempt in range(2):
        nx = C.c_int64(0); sat = C.c_int64(0)
        cap = int((extras.numel() if hasattr(extras, "numel") else len(extras)) // 2)
        rc = lib.canvas_pack_hits2_host(_host_addr(hits), C.c_int64(int(length)), _host_addr(lo), _host_addr(hdr), _host_addr(extras), C.c_int64(cap), C.byref(nx), C.byref(sat), int(threads))
        if rc == -4 and attempt == 0 and not hasattr(extras, "numel"):           # CANVAS_ERR_CAPACITY: more words with four hits and more than the default holds
            extras = np.zeros(2 * (nx.value + 64), np.uint64); continue
        if rc:
            raise CanvasError(f"canvas_pack_hits2_host: error {rc} (extras needed: {nx.value})")
        return lo, hdr, extras, nx.value, sat.value


def snv_allele_codes(alleles):
    """the site codes canvas_snv_count compares a read's 4-bit base code with: index of the allele's character in "=ACMGRSVTWYHKDBN", 255 for anything else"""
    return np.array([("=ACMGRSVTWYHKDBN".find(a) if len(a) == 1 else -1) & 0xFF for a in alleles], np.uint8)


def smooth_lengths(n, max_half_window):
    """canvas_smooth_lengths (plain host code, no GPU): the number of bins CanvasSmooth -w max_half_window leaves of chromosomes of n bins each (int64 array)"""
    lib = load_library()
    hn = np.ascontiguousarray(n, np.int64).reshape(-1)
    out = np.zeros(len(hn), np.int64)
    rc = lib.canvas_smooth_lengths(C.c_int32(len(hn)), _np_ptr(hn), C.c_int32(int(max_half_window)), _np_ptr(out))
    if rc:
        raise CanvasError(f"canvas_smooth_lengths: error {rc}")
    return out


def smooth_plan(max_half_window):
    """canvas_smooth_plan (plain host code, no GPU): dict(fused, tile, halo, launches) — how Canvas.smooth runs for this half window"""
    lib = load_library()
    out = np.zeros(4, np.int64)
    rc = lib.canvas_smooth_plan(C.c_int32(int(max_half_window)), _np_ptr(out))
    if rc:
        raise CanvasError(f"canvas_smooth_plan: error {rc}")
    return dict(fused=bool(out[0]), tile=int(out[1]), halo=int(out[2]), launches=int(out[3]))


def segment_select_plan():
    """canvas_segment_select_plan (plain host code, no GPU): dict(wave_max, lds_max, tile, launches, forced) — the size classes of Canvas.segment_select and the class the
    CANVAS_CALL_CLASS test hook forces (None, "wave", "lds" or "tiled")"""
    lib = load_library()
    out = np.zeros(6, np.int64)
    rc = lib.canvas_segment_select_plan(_np_ptr(out))
    if rc:
        raise CanvasError(f"canvas_segment_select_plan: error {rc}")
    return dict(wave_max=int(out[0]), lds_max=int(out[1]), tile=int(out[2]), launches=int(out[3]), forced=(None, "wave", "lds", "tiled")[int(out[4])])


def reference_copy_numbers(chr_seg_offset, seg_begin, seg_end, ploidy=None):
    """canvas_reference_copy_numbers (plain host code, no GPU): PloidyInfo.GetReferenceCopyNumber per segment.  Segments grouped by chromosome (chr_seg_offset[nchr + 1],
    zero-based begins / ends); ploidy = per chromosome (one-based starts, ends, copy numbers) as Canvas.segment_ids takes it, None: 2 everywhere.  Returns an int32 array."""
    lib = load_library()
    cso = np.ascontiguousarray(chr_seg_offset, np.int64); beg = np.ascontiguousarray(seg_begin, np.int32); end = np.ascontiguousarray(seg_end, np.int32)
    nchr = len(cso) - 1
    if nchr < 0 or len(beg) != len(end) or int(cso[-1]) != len(beg):
        raise CanvasError("reference_copy_numbers: one begin / end per segment, nchr + 1 chromosome offsets that end at the number of segments")
    po, ps, pe, pc = Canvas._interval_tables(ploidy, nchr, columns=3)
    out = np.zeros(len(beg), np.int32)
    opt = lambda a: _np_ptr(a) if a is not None else None
    rc = lib.canvas_reference_copy_numbers(C.c_int32(nchr), _np_ptr(cso), _np_ptr(beg), _np_ptr(end), opt(po), opt(ps), opt(pe), opt(pc), _np_ptr(out))
    if rc:
        raise CanvasError(f"canvas_reference_copy_numbers: error {rc} (offsets that do not start at 0 or decrease, or a copy number outside 0..4)")
    return out


class Canvas:
    """One context = one GPU + one stream.  Method names follow the reference functions they replace."""

    def __init__(self, device=0, stream=None):
        import torch
        self.torch = torch
        self.lib = load_library()
        if not torch.cuda.is_available():
            raise CanvasError("no GPU visible: canvas_amd has no CPU fallback")
        self.device = torch.device("cuda", device)
        torch.cuda.set_device(device)
        raw = self.lib.canvas_create(device)
        if not raw:
            raise CanvasError("canvas_create failed: no usable GPU (no CPU fallback)")
        self.ctx = C.c_void_p(raw)   # always pass as a 64-bit pointer
        self.comm_size = 1           # ranks of the library communicator (parallel.init_library_comm / init_host_comm set it)
        if stream is not None:
            self._check(self.lib.canvas_set_stream(self.ctx, C.c_void_p(stream)))

    def close(self):
        if getattr(self, "ctx", None) is not None:
            self.lib.canvas_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        # not at interpreter shutdown: the HIP runtime (and a profiler attached to it) may already be finalised, and the process exit frees everything anyway
        try:
            if not sys.is_finalizing():
                self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise CanvasError(f"libcanvas_hip error {rc}: {self.lib.canvas_last_error(self.ctx).decode()}")

    def use_torch_stream(self):
        """run on torch's current stream so torch.cuda.Event timing sees the kernels"""
        s = self.torch.cuda.current_stream(self.device).cuda_stream
        self._check(self.lib.canvas_set_stream(self.ctx, C.c_void_p(s)))

    def synchronize(self):
        self._check(self.lib.canvas_synchronize(self.ctx))
        self.__dict__.pop("_queued_inputs", None)                 # (bgzf_inflate: what queued calls read has been read)

    def upload_genome_begin(self, lens, h_bases, d_bases, h_mask, d_mask, h_hits, d_hits):
        """queue the per-chromosome upload of host arrays (pinned torch tensors / numpy arrays; None = already resident) on the context's copy stream;
        the next binning call on the same destination tensors overlaps it (canvas_upload_genome_begin)"""
        n = len(d_bases)
        hl = np.ascontiguousarray(lens, np.int64)
        hp = lambda ts: None if ts is None else (C.c_void_p * n)(*[None if t is None else C.c_void_p(t.data_ptr() if hasattr(t, "data_ptr") else t.ctypes.data) for t in ts])
        self._check(self.lib.canvas_upload_genome_begin(self.ctx, n, _np_ptr(hl), hp(h_bases), _ptr_table(d_bases), hp(h_mask), _ptr_table(d_mask), hp(h_hits), _ptr_table(d_hits)))

    def upload_packed_begin(self, lens, h_ref, d_ref, h_planes, d_planes):
        """canvas_upload_packed_begin: the packed planes, chromosome by chromosome on the copy stream (h_ref None = reference planes already resident)"""
        n = len(d_ref)
        hl = np.ascontiguousarray(lens, np.int64)
        hp = lambda ts: None if ts is None else (C.c_void_p * n)(*[None if t is None else _host_addr(t) for t in ts])
        self._check(self.lib.canvas_upload_packed_begin(self.ctx, n, _np_ptr(hl), hp(h_ref), _ptr_table(d_ref), hp(h_planes), _ptr_table(d_planes)))

    def upload_packed2_begin(self, lens, h_ref, d_ref, h_lo, h_hdr, h_extras, n_extras, d_planes):
        """canvas_upload_packed2_begin: the hit planes in their two-bit wire form (pack_hits2_host), expanded into d_planes on the device behind each chromosome's transfer"""
        n = len(d_ref)
        hl = np.ascontiguousarray(lens, np.int64); nx = np.ascontiguousarray(n_extras, np.int64)
        hp = lambda ts: None if ts is None else (C.c_void_p * n)(*[None if t is None else _host_addr(t) for t in ts])
        self._check(self.lib.canvas_upload_packed2_begin(self.ctx, n, _np_ptr(hl), hp(h_ref), _ptr_table(d_ref), hp(h_lo), hp(h_hdr), hp(h_extras), _np_ptr(nx), _ptr_table(d_planes)))

    def pack_genome_device(self, bases, masks, hits, lens):
        """canvas_pack_genome_device: per-base arrays in HBM -> (ref planes, hit planes, pos0, #saturated); bases/masks or hits may be None"""
        torch = self.torch
        n = len(lens)
        hl = np.ascontiguousarray(lens, np.int64)
        ref = [torch.empty(2 * packed_plane_words(L), dtype=torch.int64, device=self.device) for L in lens] if bases is not None else None
        planes = [torch.empty(4 * packed_plane_words(L), dtype=torch.int64, device=self.device) for L in lens] if hits is not None else None
        pos0 = np.zeros(n, np.int64); sat = C.c_int64(0)
        tab = lambda ts: None if ts is None else _ptr_table(ts)
        self._check(self.lib.canvas_pack_genome_device(self.ctx, n, tab(bases), tab(masks), tab(hits), _np_ptr(hl), tab(ref), tab(planes),
                                                       _np_ptr(pos0) if bases is not None else None, C.byref(sat)))
        return ref, planes, (pos0 if bases is not None else None), sat.value

    def bin_sample_packed(self, ref, planes, lens, pos0, is_autosome, counts_per_bin=100, bin_size=-1, mode=MODE_TDR, out=None):
        """canvas_bin_sample over the packed planes (bit-identical outputs)"""
        n = len(ref)
        lens = np.ascontiguousarray(lens, np.int64); p0 = np.ascontiguousarray(pos0, np.int64)
        ia = np.ascontiguousarray(is_autosome, np.uint8)
        per = np.zeros(n, np.int64); total = C.c_int64(0); bs = C.c_int32(0)
        self._check(self.lib.canvas_bin_sample_packed(self.ctx, n, _ptr_table(ref), _ptr_table(planes), _np_ptr(lens), _np_ptr(p0), _np_ptr(ia), counts_per_bin, bin_size, mode,
                                                      C.c_void_p(out["chr"].data_ptr()), C.c_void_p(out["start"].data_ptr()), C.c_void_p(out["stop"].data_ptr()),
                                                      C.c_void_p(out["gc"].data_ptr()), C.c_void_p(out["count"].data_ptr()), C.c_int64(out["chr"].numel()),
                                                      C.byref(bs), _np_ptr(per), C.byref(total)))
        self.synchronize()
        return out, per, total.value, bs.value

    def upload_genome_wait(self):
        self._check(self.lib.canvas_upload_genome_wait(self.ctx))

    def memcpy_d2h(self, h_dst, d_src, nbytes):
        self._check(self.lib.canvas_memcpy_d2h(self.ctx, C.c_void_p(h_dst.data_ptr() if hasattr(h_dst, "data_ptr") else h_dst.ctypes.data), C.c_void_p(d_src.data_ptr()), C.c_int64(nbytes)))

    # ---- CanvasBin
    def mask_from_fasta(self, bases, length):
        """InitializeAlignmentArrays (CanvasBin.cs:183-200)"""
        mask = self.torch.empty((length + 63) // 64, dtype=self.torch.int64, device=self.device)
        self._check(self.lib.canvas_mask_from_fasta(self.ctx, C.c_void_p(bases.data_ptr()), C.c_int64(length), C.c_void_p(mask.data_ptr())))
        self.synchronize()
        return mask

    def mask_exclude_intervals(self, mask, length, starts, stops):
        """ExcludeTagsOverlappingFilterFile (CanvasBin.cs:668-692)"""
        a = np.ascontiguousarray(starts, np.int32); b = np.ascontiguousarray(stops, np.int32)
        self._check(self.lib.canvas_mask_exclude_intervals(self.ctx, C.c_void_p(mask.data_ptr()), C.c_int64(length), len(a), _np_ptr(a), _np_ptr(b)))

    def screen_hits(self, hits, mask, length):
        """ScreenObservedTags (CanvasBin.cs:699-716)"""
        self._check(self.lib.canvas_screen_hits(self.ctx, C.c_void_p(hits.data_ptr()), C.c_void_p(mask.data_ptr()), C.c_int64(length)))
        self.synchronize()

    def bin_rates(self, hits, masks, lens):
        """SampleHitArrays.GetRates (CanvasBin.cs:30-71)"""
        n = len(hits)
        lens = np.ascontiguousarray(lens, np.int64)
        obs = np.zeros(n, np.int64); poss = np.zeros(n, np.int64); rate = np.zeros(n, np.float64)
        self._check(self.lib.canvas_bin_rates(self.ctx, n, _ptr_table(hits), _ptr_table(masks), _np_ptr(lens), _np_ptr(obs), _np_ptr(poss), _np_ptr(rate)))
        return obs, poss, rate

    def bin_size_from_rates(self, rates, counts_per_bin):
        """SampleHitArrays.GetBinSize (CanvasBin.cs:73-83)"""
        r = np.ascontiguousarray(rates, np.float64)
        return int(self.lib.canvas_bin_size_from_rates(_np_ptr(r), len(r), counts_per_bin))

    def bin_genome(self, bases, masks, hits, lens, bin_size, mode=MODE_TDR, out=None):
        """BinCounts (CanvasBin.cs:416-550): returns dict(chr,start,stop,gc,count) device tensors trimmed to the bin count"""
        torch = self.torch
        n = len(bases)
        lens = np.ascontiguousarray(lens, np.int64)
        cap = int(self.lib.canvas_bin_count_upper_bound(n, _np_ptr(lens), bin_size))
        if cap < 0:
            raise CanvasError("bad bin size")
        if out is None:
            out = dict(chr=torch.empty(cap + 1, dtype=torch.int32, device=self.device), start=torch.empty(cap + 1, dtype=torch.int32, device=self.device),
                       stop=torch.empty(cap + 1, dtype=torch.int32, device=self.device), gc=torch.empty(cap + 1, dtype=torch.int32, device=self.device),
                       count=torch.empty(cap + 1, dtype=torch.float32, device=self.device))
        per = np.zeros(n, np.int64); total = C.c_int64(0)
        self._check(self.lib.canvas_bin_genome(self.ctx, n, _ptr_table(bases), _ptr_table(masks), _ptr_table(hits), _np_ptr(lens), bin_size, mode,
                                               C.c_void_p(out["chr"].data_ptr()), C.c_void_p(out["start"].data_ptr()), C.c_void_p(out["stop"].data_ptr()),
                                               C.c_void_p(out["gc"].data_ptr()), C.c_void_p(out["count"].data_ptr()), C.c_int64(out["chr"].numel()),
                                               _np_ptr(per), C.byref(total)))
        self.synchronize()   # own non-blocking stream: make the bins visible to torch's stream before handing tensors back
        return out, per, total.value

    def bin_sample(self, bases, masks, hits, lens, is_autosome, counts_per_bin=100, bin_size=-1, mode=MODE_TDR, out=None):
        """CanvasBin.RunSingleSample (CanvasBin.cs:914-931): rates -> bin size -> bins in one call"""
        n = len(bases)
        lens = np.ascontiguousarray(lens, np.int64)
        ia = np.ascontiguousarray(is_autosome, np.uint8)
        per = np.zeros(n, np.int64); total = C.c_int64(0); bs = C.c_int32(0)
        self._check(self.lib.canvas_bin_sample(self.ctx, n, _ptr_table(bases), _ptr_table(masks), _ptr_table(hits), _np_ptr(lens), _np_ptr(ia), counts_per_bin, bin_size, mode,
                                               C.c_void_p(out["chr"].data_ptr()), C.c_void_p(out["start"].data_ptr()), C.c_void_p(out["stop"].data_ptr()),
                                               C.c_void_p(out["gc"].data_ptr()), C.c_void_p(out["count"].data_ptr()), C.c_int64(out["chr"].numel()),
                                               C.byref(bs), _np_ptr(per), C.byref(total)))
        self.synchronize()
        return out, per, total.value, bs.value

    def bin_sample_gcweighted(self, bases, masks, hits, fraglens, lens, is_autosome, counts_per_bin=100, bin_size=-1, out=None):
        """CanvasBin -m GCContentWeighted (CanvasBin.cs:416-506,626-636)"""
        n = len(bases)
        lens = np.ascontiguousarray(lens, np.int64)
        ia = np.ascontiguousarray(is_autosome, np.uint8)
        per = np.zeros(n, np.int64); total = C.c_int64(0); bs = C.c_int32(0)
        self._check(self.lib.canvas_bin_sample_gcweighted(self.ctx, n, _ptr_table(bases), _ptr_table(masks), _ptr_table(hits), _ptr_table(fraglens), _np_ptr(lens), _np_ptr(ia),
                                                          counts_per_bin, bin_size, C.c_void_p(out["chr"].data_ptr()), C.c_void_p(out["start"].data_ptr()),
                                                          C.c_void_p(out["stop"].data_ptr()), C.c_void_p(out["gc"].data_ptr()), C.c_void_p(out["count"].data_ptr()),
                                                          C.c_int64(out["chr"].numel()), C.byref(bs), _np_ptr(per), C.byref(total)))
        self.synchronize()
        return out, per, total.value, bs.value

    def bin_sample_sharded(self, owner, bases, masks, hits, lens, is_autosome, out, counts_per_bin=100, bin_size=-1, mode=MODE_TDR, fraglens=None):
        """canvas_bin_sample_sharded: CanvasBin with the chromosomes sharded over the ranks (entries of chromosomes this rank does not own may be None); every rank gets the
        whole genome's bins in `out`.  fraglens: mode 5 (GCContentWeighted).  Returns (bin size, number of bins)."""
        n = len(bases)
        lens = np.ascontiguousarray(lens, np.int64); ia = np.ascontiguousarray(is_autosome, np.uint8); ow = np.ascontiguousarray(owner, np.int32)
        bs = C.c_int32(0); total = C.c_int64(0)
        tab = lambda ts: (C.c_void_p * n)(*[None if t is None else C.c_void_p(t.data_ptr()) for t in ts])
        self._check(self.lib.canvas_bin_sample_sharded(self.ctx, n, _np_ptr(ow), tab(bases), tab(masks), tab(hits), tab(fraglens) if fraglens is not None else None,
                                                       _np_ptr(lens), _np_ptr(ia), counts_per_bin, bin_size, mode, C.c_void_p(out["chr"].data_ptr()), C.c_void_p(out["start"].data_ptr()),
                                                       C.c_void_p(out["stop"].data_ptr()), C.c_void_p(out["gc"].data_ptr()), C.c_void_p(out["count"].data_ptr()),
                                                       C.c_int64(out["chr"].numel()), C.byref(bs), C.byref(total)))
        self.synchronize()
        return bs.value, total.value

    def bin_gcw_stats(self):
        """last bin_sample_gcweighted: (bins whose weighted count was decided from the exact sum + error interval, bins replayed in the reference's order)"""
        v = np.zeros(2, np.int64)
        self._check(self.lib.canvas_bin_gcw_stats(self.ctx, _np_ptr(v)))
        return int(v[0]), int(v[1])

    def bin_predefined(self, bases, masks, hits, lens, bin_starts, bin_stops, mode=MODE_TDR, fraglens=None):
        """CanvasBin -n (BinCountsForChromosome with predefined bins): bin_starts / bin_stops = one array per chromosome; returns (gc, count) tensors over the concatenated bins.
        mode 5 (GCContentWeighted) needs fraglens (int16 per base, per chromosome): canvas_bin_predefined_gcweighted"""
        torch = self.torch
        n = len(bases)
        lens = np.ascontiguousarray(lens, np.int64)
        off = np.concatenate([[0], np.cumsum([len(b) for b in bin_starts])]).astype(np.int64)
        hs = np.ascontiguousarray(np.concatenate([np.asarray(b, np.int32) for b in bin_starts] + [np.zeros(0, np.int32)]), np.int32)
        he = np.ascontiguousarray(np.concatenate([np.asarray(b, np.int32) for b in bin_stops] + [np.zeros(0, np.int32)]), np.int32)
        ds = torch.from_numpy(hs if len(hs) else np.zeros(1, np.int32)).to(self.device); de = torch.from_numpy(he if len(he) else np.zeros(1, np.int32)).to(self.device)
        gc = torch.empty(max(1, len(hs)), dtype=torch.int32, device=self.device); cnt = torch.empty(max(1, len(hs)), dtype=torch.float32, device=self.device)
        self.torch.cuda.synchronize()
        if fraglens is not None:
            self._check(self.lib.canvas_bin_predefined_gcweighted(self.ctx, n, _ptr_table(bases), _ptr_table(masks), _ptr_table(hits), _ptr_table(fraglens), _np_ptr(lens), _np_ptr(off), _np_ptr(hs),
                                                                  _np_ptr(he), C.c_void_p(ds.data_ptr()), C.c_void_p(de.data_ptr()), C.c_void_p(gc.data_ptr()), C.c_void_p(cnt.data_ptr())))
            return gc[:len(hs)], cnt[:len(hs)]
        self._check(self.lib.canvas_bin_predefined(self.ctx, n, _ptr_table(bases), _ptr_table(masks), _ptr_table(hits), _np_ptr(lens), int(mode), _np_ptr(off), _np_ptr(hs), _np_ptr(he),
                                                   C.c_void_p(ds.data_ptr()), C.c_void_p(de.data_ptr()), C.c_void_p(gc.data_ptr()), C.c_void_p(cnt.data_ptr())))
        return gc[:len(hs)], cnt[:len(hs)]

    def chromosome_offsets(self, chr_ids, n, nchr):
        off = np.zeros(nchr + 1, np.int64)
        self._check(self.lib.canvas_chromosome_offsets(self.ctx, C.c_void_p(chr_ids.data_ptr()), C.c_int64(n), nchr, _np_ptr(off)))
        return off

    # ---- CanvasClean
    def clean(self, bins, n, is_autosome, flags, min_bins_per_gc=100, is_y=None):
        """CanvasClean.Main (CanvasClean.cs:415-533) in place on device SoA; returns (n_out, local_sd, info)"""
        ia = np.ascontiguousarray(is_autosome, np.uint8)
        iy = np.ascontiguousarray(is_y if is_y is not None else np.zeros(len(ia)), np.uint8)
        lsd = C.c_double(-1.0); nout = C.c_int64(0); info = np.zeros(8, np.int32)
        self._check(self.lib.canvas_clean2(self.ctx, C.c_int64(n), C.c_void_p(bins["chr"].data_ptr()), C.c_void_p(bins["start"].data_ptr()),
                                           C.c_void_p(bins["stop"].data_ptr()), C.c_void_p(bins["count"].data_ptr()), C.c_void_p(bins["gc"].data_ptr()),
                                           len(ia), _np_ptr(ia), _np_ptr(iy), C.c_uint32(flags), min_bins_per_gc, C.byref(lsd), C.byref(nout), _np_ptr(info)))
        return nout.value, lsd.value, info

    def clean_batch(self, samples, ns, is_autosome, flags, min_bins_per_gc=100, is_y=None):
        """canvas_clean_batch: CanvasClean of several samples at once (list of SoA dicts, bins per sample); returns ([n_out], [local_sd], info[S][8])"""
        S = len(samples)
        ia = np.ascontiguousarray(is_autosome, np.uint8)
        iy = np.ascontiguousarray(is_y if is_y is not None else np.zeros(len(ia)), np.uint8)
        arr = lambda key: (C.c_void_p * S)(*[C.c_void_p(s[key].data_ptr()) for s in samples])
        hn = np.ascontiguousarray(ns, np.int64); lsd = np.full(S, -1.0, np.float64); nout = np.zeros(S, np.int64); info = np.zeros((S, 8), np.int32)
        self.torch.cuda.synchronize()
        self._check(self.lib.canvas_clean_batch(self.ctx, S, _np_ptr(hn), arr("chr"), arr("start"), arr("stop"), arr("count"), arr("gc"), len(ia), _np_ptr(ia), _np_ptr(iy),
                                                C.c_uint32(flags), int(min_bins_per_gc), _np_ptr(lsd), _np_ptr(nout), _np_ptr(info)))
        return nout, lsd, info

    def merge_cleaned(self, samples, ns):
        """MergeMultiSampleCleanedBedFile (Utilities.cs:834-920): bins every sample still has.  samples = list of SoA dicts (chr, start, stop,
        count), ns = bins per sample.  Returns (chr, start, stop, [count per sample], n_out)."""
        torch = self.torch
        S = len(samples); n0 = int(ns[0])
        oc = torch.empty(max(n0, 1), dtype=torch.int32, device=self.device); os_ = torch.empty_like(oc); oe = torch.empty_like(oc)
        ocnt = [torch.empty(max(n0, 1), dtype=torch.float32, device=self.device) for _ in range(S)]
        arr = lambda key: (C.c_void_p * S)(*[C.c_void_p(s[key].data_ptr()) for s in samples])
        hn = np.ascontiguousarray(ns, np.int64); nout = C.c_int64(0)
        self._check(self.lib.canvas_merge_cleaned(self.ctx, S, _np_ptr(hn), arr("chr"), arr("start"), arr("stop"), arr("count"), C.c_void_p(oc.data_ptr()),
                                                  C.c_void_p(os_.data_ptr()), C.c_void_p(oe.data_ptr()), (C.c_void_p * S)(*[C.c_void_p(t.data_ptr()) for t in ocnt]), C.byref(nout)))
        k = nout.value
        return oc[:k], os_[:k], oe[:k], [t[:k] for t in ocnt], k

    def quantize_f2(self, count, n, out=None):
        """count.ToString("F2") -> Convert.ToDouble (IO.cs:21 -> CanvasSegment.cs:1146), in memory"""
        cov = out[:n] if out is not None else self.torch.empty(n, dtype=self.torch.float64, device=self.device)
        self._check(self.lib.canvas_quantize_f2(self.ctx, C.c_void_p(count.data_ptr()), C.c_int64(n), C.c_void_p(cov.data_ptr())))
        self.synchronize()   # the library runs on its own non-blocking stream; make the result visible to torch's stream
        return cov

    def profile_enable(self, on=True):
        self._check(self.lib.canvas_profile_enable(self.ctx, int(on)))      # True / 1: every scope; 2: only the dominant kernel's scope

    def profile_get(self, name, reset=True):
        ms = C.c_double(0); k = C.c_int32(0)
        self._check(self.lib.canvas_profile_get(self.ctx, name.encode(), C.byref(ms), C.byref(k), int(reset)))
        return ms.value, k.value

    # ---- CanvasPartition
    def hmm_per_sample(self, cov, chr_offset, out=None):
        """HiddenMarkovModelsRunner.Run(isPerSample) (HiddenMarkovModelsRunner.cs:23-109): Viterbi state per bin"""
        torch = self.torch
        off = np.ascontiguousarray(chr_offset, np.int64)
        state = out[:int(off[-1])] if out is not None else torch.empty(int(off[-1]), dtype=torch.int32, device=self.device)
        self._check(self.lib.canvas_hmm_per_sample(self.ctx, len(off) - 1, C.c_void_p(cov.data_ptr()), _np_ptr(off), C.c_void_p(state.data_ptr())))
        return state

    def cbs_device_stats(self):
        """[device permutations, host permutations, exact re-evaluations, device batches, verified, violations] of the last cbs() call"""
        out = np.zeros(6, np.int64)
        self._check(self.lib.canvas_cbs_device_stats(self.ctx, _np_ptr(out)))
        return out

    def cbs_tail_probe(self, xs, tol=1e-6):
        """TailProbability.Nu of up to 100 arguments through the device series (canvas_cbs_tail_probe): (nu, flags)"""
        xs = np.ascontiguousarray(xs, np.float64); nu = np.zeros(len(xs), np.float64); fl = np.zeros(len(xs), np.int32)
        self._check(self.lib.canvas_cbs_tail_probe(self.ctx, _np_ptr(xs), len(xs), C.c_double(tol), _np_ptr(nu), _np_ptr(fl)))
        return nu, fl

    def cbs_cache_stats(self):
        """[draws read out of the stream cache, draws generated inside batches, draws the cache's generator produced, states fetched for host code] of the last cbs() call,
        then [bytes of device memory the cache holds, draws it holds]"""
        out = np.zeros(6, np.int64)
        self._check(self.lib.canvas_cbs_cache_stats(self.ctx, _np_ptr(out)))
        return out

    def cbs_stream_read(self, chromosome, position, nwords):
        """nwords draws of the chromosome-th generator's output stream from `position` on, out of the context's cache (canvas_cbs_stream_read)"""
        out = np.zeros(int(nwords), np.uint32)
        self._check(self.lib.canvas_cbs_stream_read(self.ctx, int(chromosome), C.c_int64(int(position)), C.c_int64(int(nwords)), _np_ptr(out)))
        return out

    def cbs_prefetch(self, nchr, words_per_chromosome=0):
        """start generating the draw streams of the first nchr chromosomes in the background (canvas_cbs_prefetch)"""
        self._check(self.lib.canvas_cbs_prefetch(self.ctx, int(nchr), C.c_int64(int(words_per_chromosome))))

    def cbs_perm_probe(self, x, seed, nb, kernel, tss):
        """one batch of nb permutations of the centred segment x through the device permutation engine (canvas_cbs_perm_probe): (lohi[nb, 2], ms[3])"""
        x = np.ascontiguousarray(x, np.float64)
        lohi = np.zeros((nb, 2), np.float64); ms = np.zeros(3, np.float64)
        self._check(self.lib.canvas_cbs_perm_probe(self.ctx, _np_ptr(x), C.c_int32(len(x)), C.c_uint32(seed & 0xFFFFFFFF), C.c_int32(nb), C.c_int32(kernel), C.c_double(tss), _np_ptr(lohi), _np_ptr(ms)))
        return lohi, ms

    def cbs_arc_probe(self, segments, al0=2, mode=0, pair_cap=0):
        """TMaxO of centred segments through the device arc search (canvas_cbs_arc_probe), all in shared launches.  mode 0: pruned search, 1: exhaustive kernel; pair_cap 0: the
        library's.  Returns a dict: off[nseg + 1], sx, tau[nseg], stat[nseg], iseg[nseg, 2], path[nseg], words[nseg, 6] (uint64), dmax, first (sx, dmax, first: concatenated like the input)"""
        segs = [np.ascontiguousarray(s, np.float64).ravel() for s in segments]
        off = np.zeros(len(segs) + 1, np.int64); off[1:] = np.cumsum([len(s) for s in segs])
        x = np.ascontiguousarray(np.concatenate(segs)) if segs else np.zeros(0, np.float64)
        ns, tot = len(segs), max(1, len(x))
        out = dict(off=off, sx=np.zeros(tot, np.float64), tau=np.zeros(ns, np.float64), stat=np.zeros(ns, np.float64), iseg=np.zeros((ns, 2), np.int32), path=np.zeros(ns, np.int32),
                   words=np.zeros((ns, 6), np.uint64), dmax=np.zeros(tot, np.float64), first=np.zeros(tot, np.int32))
        self._check(self.lib.canvas_cbs_arc_probe(self.ctx, C.c_int32(mode), C.c_int32(ns), _np_ptr(off), _np_ptr(x), C.c_int32(al0), C.c_int32(pair_cap), _np_ptr(out["sx"]), _np_ptr(out["tau"]),
                                                  _np_ptr(out["stat"]), _np_ptr(out["iseg"]), _np_ptr(out["path"]), _np_ptr(out["words"]), _np_ptr(out["dmax"]), _np_ptr(out["first"])))
        return out

    def select_probe(self, variant, dtype, values, seg_off, seg_lo, seg_hi, k):
        """the order-statistics engine of select.hpp on its own (canvas_select_probe).  values: numpy array of float32 / float64 / uint32 / uint64 for dtype 0 / 1 / 2 / 3;
        variant 0 / 1: radix_select with host / device results, k[nq] -> keys u64[nq]; variant 2: wg_select2, k[nq, 2] -> keys u64[nq, 2]"""
        want = (np.float32, np.float64, np.uint32, np.uint64)[dtype]
        values = np.ascontiguousarray(values)
        if values.dtype != want:
            raise CanvasError(f"select_probe: dtype {dtype} takes {np.dtype(want).name} values, not {values.dtype.name}")
        off = np.ascontiguousarray(seg_off, np.int64); lo = np.ascontiguousarray(seg_lo, np.int32); hi = np.ascontiguousarray(seg_hi, np.int32)
        kk = np.ascontiguousarray(k, np.int64)
        nq = len(lo)
        if len(hi) != nq or kk.shape != ((nq, 2) if variant == 2 else (nq,)):
            raise CanvasError("select_probe: one (seg_lo, seg_hi, k) per query; k is a pair per query with variant 2")
        if len(off) < 2 or off.max() > len(values):
            raise CanvasError("select_probe: the segment offsets reach past the values")
        bits = values.view(np.int32 if values.itemsize == 4 else np.int64)             # (torch has no unsigned 32 / 64-bit tensors to speak of: the bits travel as signed)
        dev = self.torch.from_numpy(bits if len(bits) else np.zeros(1, bits.dtype)).to(self.device)
        out = np.zeros(kk.shape, np.uint64)
        self._check(self.lib.canvas_select_probe(self.ctx, C.c_int32(variant), C.c_int32(dtype), C.c_void_p(dev.data_ptr()), C.c_int32(len(off) - 1), _np_ptr(off), C.c_int32(nq),
                                                 _np_ptr(lo), _np_ptr(hi), _np_ptr(kk), _np_ptr(out)))
        return out

    def backbone_probe(self, mode, v, chr_offset):
        """the exact backbone of the speculative Viterbi pass on its own (canvas_hmm_backbone_probe).  v: numpy float64 increments, chr_offset: the chromosomes' offsets into
        them; mode 0 chain / 1 parity scan / 2 predicted pieces -> (carry float64[len(v)], fail int32[nchr]): carry[begin + t] is the running sum in front of step t for every
        multiple t of 64 of a chromosome of more than ten steps, every other element keeps the NaN pattern BACKBONE_PROBE_UNTOUCHED"""
        v = np.ascontiguousarray(v)
        if v.dtype != np.float64:
            raise CanvasError(f"backbone_probe: float64 increments, not {v.dtype.name}")
        off = np.ascontiguousarray(chr_offset, np.int64)
        if len(off) < 2 or off[0] != 0 or off[-1] != len(v) or (np.diff(off) < 0).any():
            raise CanvasError("backbone_probe: the offsets start at 0, do not decrease and end at len(v)")
        torch = self.torch
        n = len(v)
        dv = torch.from_numpy(v.view(np.int64) if n else np.zeros(1, np.int64)).to(self.device)             # (the bits travel as integers: NaN payloads stay as they are)
        dc = torch.full((max(n, 1),), BACKBONE_PROBE_UNTOUCHED, dtype=torch.int64, device=self.device)
        torch.cuda.synchronize(self.device)      # the library runs on its own stream
        fail = np.zeros(len(off) - 1, np.int32)
        self._check(self.lib.canvas_hmm_backbone_probe(self.ctx, C.c_int32(mode), C.c_int32(len(off) - 1), _np_ptr(off), C.c_void_p(dv.data_ptr()), C.c_void_p(dc.data_ptr()), _np_ptr(fail)))
        return dc.cpu().numpy()[:n].view(np.float64), fail

    def stale_reads(self):
        """process-wide [pinned results looked at, looks that came before the result had arrived (polled until it did)] (canvas_stale_reads)"""
        out = np.zeros(2, np.int64)
        self._check(self.lib.canvas_stale_reads(_np_ptr(out)))
        return out

    def cbs_tpermp_stats(self):
        """[edge tests (TPermP) run by the device kernel, swaps of all edge tests] of the last cbs() call"""
        out = np.zeros(2, np.int64)
        self._check(self.lib.canvas_cbs_tpermp_stats(self.ctx, _np_ptr(out)))
        return out

    def cbs_tailp_stats(self):
        """[TailP calls decided from the device series, calls recomputed by the host series] of the last cbs() call"""
        out = np.zeros(2, np.int64)
        self._check(self.lib.canvas_cbs_tailp_stats(self.ctx, _np_ptr(out)))
        return out

    def hmm_joint(self, covs, chr_offset, out=None):
        """-m HMM: joint Viterbi over several samples (HiddenMarkovModelsRunner.Run(isPerSample=false), Distributions.cs:257-323)"""
        torch = self.torch
        off = np.ascontiguousarray(chr_offset, np.int64)
        state = out[:int(off[-1])] if out is not None else torch.empty(int(off[-1]), dtype=torch.int32, device=self.device)
        ptrs = (C.c_void_p * len(covs))(*[C.c_void_p(c.data_ptr()) for c in covs])
        self._check(self.lib.canvas_hmm_joint(self.ctx, len(covs), len(off) - 1, ptrs, _np_ptr(off), C.c_void_p(state.data_ptr())))
        return state

    def evenness_score(self, cov, chr_offset, window=100000):
        """SegmentationInput.GetEvennessScore (Segmentation.cs:260-296): the value of --evenness-metric-file, or None when the reference writes no file"""
        off = np.ascontiguousarray(chr_offset, np.int64)
        score = C.c_double(0); valid = C.c_int32(0)
        self._check(self.lib.canvas_evenness_score(self.ctx, len(off) - 1, C.c_void_p(cov.data_ptr()), _np_ptr(off), int(window), C.byref(score), C.byref(valid)))
        return score.value if valid.value else None

    def snv_count(self, records, offsets, ref_id, site_pos, site_ref, site_alt, ref_counts=None, alt_counts=None, min_mapq=0, min_base_q=20, nbytes=None, want_info=True):
        """SNVReviewer.ProcessBamFile + ProcessReadBases (SNVReviewer.cs:172-271) over one chunk of raw BAM records.  records: uint8 tensor (record bytes, each with
        its block_size word), offsets: int64 tensor (byte offset of every record); site_pos int32 (one-based, sorted), site_ref / site_alt uint8 codes (snv_allele_codes);
        ref_counts / alt_counts int32 are added to (created as zeros when None).  Returns (ref_counts, alt_counts, info[5] or None: seen, passed, walked, stopped at an
        unsupported CIGAR operation, malformed).  want_info=False only queues the work."""
        torch = self.torch
        ns = int(site_pos.numel())
        if ref_counts is None:
            ref_counts = torch.zeros(max(ns, 1), dtype=torch.int32, device=self.device)
        if alt_counts is None:
            alt_counts = torch.zeros(max(ns, 1), dtype=torch.int32, device=self.device)
        assert records.dtype == torch.uint8 and offsets.dtype == torch.int64 and site_pos.dtype == torch.int32 and site_ref.dtype == torch.uint8 and site_alt.dtype == torch.uint8
        assert ref_counts.dtype == torch.int32 and alt_counts.dtype == torch.int32 and ref_counts.numel() >= ns and alt_counts.numel() >= ns
        for t in (records, offsets, site_pos, site_ref, site_alt, ref_counts, alt_counts):      # the kernel reads dense arrays on this context's device
            assert t.is_contiguous() and t.dim() == 1 and (t.numel() == 0 or t.device == self.device), "snv_count: tensors must be dense, one-dimensional and on the context's device"
        nb = int(records.numel()) if nbytes is None else int(nbytes)
        assert 0 <= nb <= records.numel()
        info = np.zeros(5, np.int64) if want_info else None
        self._check(self.lib.canvas_snv_count(self.ctx, C.c_void_p(records.data_ptr()), C.c_uint64(nb), C.c_void_p(offsets.data_ptr()), C.c_int64(int(offsets.numel())),
                                              int(ref_id), int(min_mapq), int(min_base_q), C.c_void_p(site_pos.data_ptr()), C.c_void_p(site_ref.data_ptr()),
                                              C.c_void_p(site_alt.data_ptr()), ns, C.c_void_p(ref_counts.data_ptr()), C.c_void_p(alt_counts.data_ptr()),
                                              _np_ptr(info) if want_info else None))
        return ref_counts, alt_counts, info

    def bgzf_inflate(self, src, blocks, out=None, status=None, want_info=True):
        """BGZF blocks inflated on the device.  src: uint8 tensor holding the compressed bytes; blocks: the descriptors as a numpy array of BGZF_BLOCK (bgzf_scan's), or a
        device tensor of n x 24 uint8 (any dense shape of 24 n bytes).  out (uint8) is created to hold the farthest destination range when None, status (int32 per
        block) likewise.  Returns (out, status, info): info[4] = blocks, failed blocks, bytes written by good blocks, first failed block or -1; want_info=False only
        queues the work and returns None for it.  status[i] is 0 exactly where zlib's raw inflate accepts the block for its recorded size (INFLATE_* otherwise)."""
        torch = self.torch
        if isinstance(blocks, np.ndarray):
            host = np.ascontiguousarray(blocks.astype(BGZF_BLOCK, copy=False))
            n = int(host.size)
            if out is None:
                out = torch.empty(max(int((host["dst_offset"] + host["out_bytes"]).max()) if n else 0, 1), dtype=torch.uint8, device=self.device)
            blocks = torch.from_numpy(host.view(np.uint8).reshape(-1).copy()).to(self.device)
        else:
            assert blocks.dtype == torch.uint8 and blocks.numel() % 24 == 0, "bgzf_inflate: blocks is n x 24 bytes"
            n = int(blocks.numel()) // 24
            assert out is not None, "bgzf_inflate: descriptors on the device need `out`"
        if status is None:
            status = torch.zeros(max(n, 1), dtype=torch.int32, device=self.device)
        assert src.dtype == torch.uint8 and out.dtype == torch.uint8 and status.dtype == torch.int32 and status.numel() >= n
        for t in (src, blocks, out, status):
            assert t.is_contiguous() and (t.numel() == 0 or t.device == self.device), "bgzf_inflate: tensors must be dense and on the context's device"
        torch.cuda.current_stream(self.device).synchronize()      # torch fills and copies on its own stream; the kernel runs on the context's
        info = np.zeros(4, np.int64) if want_info else None
        self._check(self.lib.canvas_bgzf_inflate(self.ctx, C.c_void_p(src.data_ptr()), C.c_uint64(int(src.numel())), C.c_void_p(blocks.data_ptr()), C.c_int64(n),
                                                 C.c_void_p(out.data_ptr()), C.c_uint64(int(out.numel())), C.c_void_p(status.data_ptr()),
                                                 _np_ptr(info) if want_info else None))
        if not want_info:
            self.__dict__.setdefault("_queued_inputs", []).append((src, blocks))      # every queued call reads its own until synchronize() has waited for the stream
        return out, status, info

    def bgzf_crc32(self, src, blocks, out, inflate_status=None, crc=None, status=None, want_info=True):
        """The CRC32 of every inflated BGZF block, held against the word of the block's trailer.  src, blocks: as for bgzf_inflate (src=None: compute only, nothing is
        compared); out: the uint8 tensor bgzf_inflate filled; inflate_status: its statuses (int32 per block; a block whose status is not 0 is CRC_SKIPPED), None: every
        block is summed.  crc (uint32 per block; an int32 tensor is taken as the same bits) and status (int32 per block) are created when None.  Returns (crc, status,
        info): info[4] = blocks, blocks neither CRC_OK nor CRC_SKIPPED, bytes summed, first such block or -1; want_info=False only queues the work and returns None
        for it.  crc[i] equals zlib.crc32 of the block's bytes wherever status[i] is CRC_OK or CRC_MISMATCH."""
        torch = self.torch
        if isinstance(blocks, np.ndarray):
            host = np.ascontiguousarray(blocks.astype(BGZF_BLOCK, copy=False))
            n = int(host.size)
            blocks = torch.from_numpy(host.view(np.uint8).reshape(-1).copy()).to(self.device)
        else:
            assert blocks.dtype == torch.uint8 and blocks.numel() % 24 == 0, "bgzf_crc32: blocks is n x 24 bytes"
            n = int(blocks.numel()) // 24
        if crc is None:
            crc = torch.zeros(max(n, 1), dtype=torch.int32, device=self.device).view(torch.uint32)      # (filled as int32: torch fills few unsigned types)
        if status is None:
            status = torch.zeros(max(n, 1), dtype=torch.int32, device=self.device)
        assert out.dtype == torch.uint8 and status.dtype == torch.int32 and status.numel() >= n
        assert src is None or src.dtype == torch.uint8
        assert inflate_status is None or (inflate_status.dtype == torch.int32 and inflate_status.numel() >= n)
        assert crc.dtype in (torch.uint32, torch.int32) and crc.numel() >= n
        for t in (src, blocks, out, status, inflate_status, crc):
            assert t is None or (t.is_contiguous() and (t.numel() == 0 or t.device == self.device)), "bgzf_crc32: tensors must be dense and on the context's device"
        torch.cuda.current_stream(self.device).synchronize()      # torch fills and copies on its own stream; the kernel runs on the context's
        info = np.zeros(4, np.int64) if want_info else None
        self._check(self.lib.canvas_bgzf_crc32(self.ctx, C.c_void_p(src.data_ptr()) if src is not None else None, C.c_uint64(int(src.numel()) if src is not None else 0),
                                               C.c_void_p(blocks.data_ptr()), C.c_int64(n), C.c_void_p(out.data_ptr()), C.c_uint64(int(out.numel())),
                                               C.c_void_p(inflate_status.data_ptr()) if inflate_status is not None else None, C.c_void_p(crc.data_ptr()),
                                               C.c_void_p(status.data_ptr()), _np_ptr(info) if want_info else None))
        if not want_info:
            self.__dict__.setdefault("_queued_inputs", []).append((src, blocks, out, inflate_status))      # every queued call reads its own until synchronize() has waited for the stream
        return crc, status, info

    def bam_frame(self, records, first, rule, offsets=None, state=None, nbytes=None):
        """The block_size chain of one chunk of raw BAM record bytes (uint8 tensor; what bgzf_inflate leaves) from byte `first` on, under `rule`: a BAM_FRAME_RULE
        record, a tuple (kind, ref_id, paired_end, sorted) or a bare kind.  offsets (int64) takes the offsets of the taken records and is created to hold every record
        the bytes can hold when None; state (int64[4], zeroed when None) carries the sortedness from chunk to chunk: pass self.bam_frame_state, the tensor the last call used.
        Returns (offsets[:taken], info): info[8] = records classified, taken, `used` (where the next chunk's carry starts), the event (BAM_FRAME_NONE / _STOPPED /
        _MALFORMED / _UNSORTED / _CAPACITY: info[1] offsets are needed, nothing was written), the event's offset or -1, the pos an unsorted record was compared with,
        tiles walked twice, the tile size.  The state tensor used is left in self.bam_frame_state."""
        torch = self.torch
        r = np.zeros(1, BAM_FRAME_RULE)
        if isinstance(rule, np.ndarray) or isinstance(rule, np.void):
            r[0] = rule if isinstance(rule, np.void) else rule.reshape(-1)[0]
        else:
            vals = tuple(rule) if isinstance(rule, (tuple, list)) else (rule,)
            r[0] = tuple(int(v) for v in vals) + (0,) * (4 - len(vals))
        nb = int(records.numel()) if nbytes is None else int(nbytes)
        assert records.dtype == torch.uint8 and 0 <= nb <= records.numel()
        if offsets is None:
            offsets = torch.empty(max((nb - min(int(first), nb)) // 36 + 2, 1), dtype=torch.int64, device=self.device)
        if state is None:
            state = torch.zeros(4, dtype=torch.int64, device=self.device)
        assert offsets.dtype == torch.int64 and state.dtype == torch.int64 and state.numel() >= 4
        for t in (records, offsets, state):
            assert t.is_contiguous() and t.dim() == 1 and (t.numel() == 0 or t.device == self.device), "bam_frame: tensors must be dense, one-dimensional and on the context's device"
        torch.cuda.current_stream(self.device).synchronize()      # torch fills and copies on its own stream; the kernels run on the context's
        info = np.zeros(8, np.int64)
        self._check(self.lib.canvas_bam_frame(self.ctx, C.c_void_p(records.data_ptr()), C.c_uint64(nb), C.c_uint64(int(first)), _np_ptr(r), C.c_void_p(offsets.data_ptr()),
                                              C.c_int64(int(offsets.numel())), C.c_void_p(state.data_ptr()), _np_ptr(info)))
        self.bam_frame_state = state
        return offsets[:0 if info[3] == BAM_FRAME_CAPACITY else int(info[1])], info

    def hits_from_bam(self, records, offsets, ref_id, length, mode=MODE_TDR, paired_end=False, hits=None, frag=None, state=None, nbytes=None, want_info=True):
        """LoadObservedAlignmentsBAM (CanvasBin.cs:207-275) over one chunk of raw BAM records (the chunk format of snv_count: uint8 record bytes, int64 offsets).
        hits (uint8, `length` positions), frag (int16, mode 5 only) and state (int64[8]) are updated; zeroed tensors are created when None — pass the returned ones
        to the next chunk of the chromosome.  Returns (hits, frag or None, state, info[8] or None: stopped, seen, kept, kept out of range, malformed, position of the
        last kept record, two reserved words).  want_info=False only queues the work."""
        torch = self.torch
        L = int(length)
        created = hits is None or state is None or (frag is None and mode == MODE_GCW)
        if hits is None:
            hits = torch.zeros(max(L, 1), dtype=torch.uint8, device=self.device)
        if frag is None and mode == MODE_GCW:
            frag = torch.zeros(max(L, 1), dtype=torch.int16, device=self.device)
        if state is None:
            state = torch.zeros(8, dtype=torch.int64, device=self.device)
        if created:                  # torch zeroes on its own stream; the kernels update the arrays on the context's
            torch.cuda.current_stream(self.device).synchronize()
        assert records.dtype == torch.uint8 and offsets.dtype == torch.int64 and hits.dtype == torch.uint8 and state.dtype == torch.int64
        assert hits.numel() >= L and state.numel() >= 8 and (frag is None or (frag.dtype == torch.int16 and frag.numel() >= L))
        for t in (records, offsets, hits, state) + (() if frag is None else (frag,)):      # the kernels read and write dense arrays on this context's device
            assert t.is_contiguous() and t.dim() == 1 and (t.numel() == 0 or t.device == self.device), "hits_from_bam: tensors must be dense, one-dimensional and on the context's device"
        nb = int(records.numel()) if nbytes is None else int(nbytes)
        assert 0 <= nb <= records.numel()
        info = np.zeros(8, np.int64) if want_info else None
        self._check(self.lib.canvas_hits_from_bam(self.ctx, C.c_void_p(records.data_ptr()), C.c_uint64(nb), C.c_void_p(offsets.data_ptr()), C.c_int64(int(offsets.numel())),
                                                  C.c_int32(int(ref_id)), C.c_int32(1 if paired_end else 0), C.c_int32(int(mode)), C.c_int64(L), C.c_void_p(hits.data_ptr()),
                                                  C.c_void_p(frag.data_ptr()) if frag is not None else None, C.c_void_p(state.data_ptr()),
                                                  _np_ptr(info) if want_info else None))
        return hits, frag, state, info

    def fragments_from_bam(self, records, offsets, ref_id, bin_start, bin_stop, quality_threshold=3, counts=None, carry=None, state=None, nbytes=None, carry_capacity=None):
        """FragmentBinner.BinTask (FragmentBinner.cs:186-369) over one chunk of raw BAM records of one chromosome (the chunk format of snv_count); bin_start / bin_stop
        (int32) are the chromosome's BED bins in file order.  counts (int32 per bin), carry (uint8, the library's list of open read names) and state (int64[16]) are
        updated; zeroed counts / state and a carry of carry_capacity bytes (default 1 MiB) are created when None — pass the returned ones to the next chunk.  A carry
        that is too small is replaced by a larger one with the old contents and the call is repeated once.  Returns (counts, carry, state, info[16]: stopped, seen,
        paired, usable, malformed, last position, unsorted, carried entries, carry bytes, groups split by a byte comparison, longest group, ...)."""
        torch = self.torch
        nbins = int(bin_start.numel())
        created = counts is None or state is None or carry is None
        if counts is None:
            counts = torch.zeros(max(nbins, 1), dtype=torch.int32, device=self.device)
        if state is None:
            state = torch.zeros(16, dtype=torch.int64, device=self.device)
        if carry is None:
            carry = torch.zeros(max(int(carry_capacity) if carry_capacity is not None else 1 << 20, 8), dtype=torch.uint8, device=self.device)
        if created:                  # torch zeroes on its own stream; the kernels update the arrays on the context's
            torch.cuda.current_stream(self.device).synchronize()
        assert records.dtype == torch.uint8 and offsets.dtype == torch.int64 and bin_start.dtype == torch.int32 and bin_stop.dtype == torch.int32
        assert counts.dtype == torch.int32 and carry.dtype == torch.uint8 and state.dtype == torch.int64
        assert bin_stop.numel() == nbins and counts.numel() >= nbins and state.numel() >= 16
        for t in (records, offsets, bin_start, bin_stop, counts, carry, state):      # the kernels read and write dense arrays on this context's device
            assert t.is_contiguous() and t.dim() == 1 and (t.numel() == 0 or t.device == self.device), "fragments_from_bam: tensors must be dense, one-dimensional and on the context's device"
        nb = int(records.numel()) if nbytes is None else int(nbytes)
        assert 0 <= nb <= records.numel()
        cap = int(carry.numel()) if carry_capacity is None else int(carry_capacity)
        assert 0 <= cap <= carry.numel()
        info = np.zeros(16, np.int64)

        def call(carry, cap):
            return self.lib.canvas_fragments_from_bam(self.ctx, C.c_void_p(records.data_ptr()), C.c_uint64(nb), C.c_void_p(offsets.data_ptr()), C.c_int64(int(offsets.numel())),
                                                      C.c_int32(int(ref_id)), C.c_void_p(bin_start.data_ptr()), C.c_void_p(bin_stop.data_ptr()), C.c_int64(nbins),
                                                      C.c_int32(int(quality_threshold)), C.c_void_p(counts.data_ptr()), C.c_void_p(carry.data_ptr()), C.c_uint64(cap),
                                                      C.c_void_p(state.data_ptr()), _np_ptr(info))
        rc = call(carry, cap)
        if rc == -4:                 # CANVAS_ERR_CAPACITY: info[8] bytes are needed
            grown = torch.zeros(max(int(info[8]), 2 * int(carry.numel())), dtype=torch.uint8, device=self.device)
            grown[:carry.numel()] = carry
            torch.cuda.current_stream(self.device).synchronize()
            carry, cap = grown, int(grown.numel())
            rc = call(carry, cap)
        self._check(rc)
        return counts, carry, state, info

    # ---- reference preparation (Tools/FlagUniqueKmers)
    def flag_unique_kmers(self, bases, lens, masks=None, max_table_bytes=0):
        """KmerChecker (Tools/FlagUniqueKmers/KmerChecker.cs): bases = one uint8 device tensor per contig (ASCII, any case, not modified), lens = their lengths.
        Returns (masks, stats): masks = one int64 tensor of ceil(len / 64) words per contig (BitArray layout; created unless given), bit p set iff position p starts a
        35-mer that occurs once in the whole input, both strands counted; stats = dict(positions, keyed, unique, passes, table_slots, longest_probe, table_bytes).
        max_table_bytes bounds the working table (0: chosen from free device memory); the masks do not depend on it."""
        torch = self.torch
        n = len(bases)
        hl = np.ascontiguousarray(lens, np.int64)
        assert len(hl) == n
        if masks is None:
            masks = [torch.empty((int(L) + 63) // 64, dtype=torch.int64, device=self.device) for L in hl]
        for t, m, L in zip(bases, masks, hl):
            assert t.dtype == torch.uint8 and t.is_contiguous() and t.numel() >= L and (L == 0 or t.device == self.device), "flag_unique_kmers: bases must be dense uint8 tensors on the context's device"
            assert m.dtype == torch.int64 and m.is_contiguous() and m.numel() >= (int(L) + 63) // 64 and (L == 0 or m.device == self.device), "flag_unique_kmers: masks must be dense int64 tensors on the context's device"
        st = np.zeros(8, np.int64)
        torch.cuda.synchronize(self.device)        # the tensors may have been written on torch's stream
        self._check(self.lib.canvas_flag_unique_kmers(self.ctx, n, _ptr_table(bases), _np_ptr(hl), _ptr_table(masks), C.c_int64(int(max_table_bytes)), _np_ptr(st)))
        return masks, dict(positions=int(st[0]), keyed=int(st[1]), unique=int(st[2]), passes=int(st[3]), table_slots=int(st[4]), longest_probe=int(st[5]), table_bytes=int(st[6]))

    def fasta_case_from_mask(self, bases, length, mask):
        """inverse of mask_from_fasta, in place: ASCII letters of bases[:length] become upper case where the mask bit is 1 and lower case where it is 0"""
        torch = self.torch
        assert bases.dtype == torch.uint8 and bases.is_contiguous() and bases.numel() >= length and mask.dtype == torch.int64 and mask.numel() >= (int(length) + 63) // 64
        torch.cuda.synchronize(self.device)
        self._check(self.lib.canvas_fasta_case_from_mask(self.ctx, C.c_void_p(bases.data_ptr()), C.c_int64(int(length)), C.c_void_p(mask.data_ptr())))
        self.synchronize()
        return bases

    def smooth(self, counts, chr_offset, max_half_window, out=None):
        """RepeatedMedianSmoother.Smooth (CanvasSmooth.cs:46-77) of every chromosome: counts = float32 device tensor, chr_offset[nchr + 1] = where each chromosome's
        bins start.  Returns (out, out_n): out[chr_offset[c] + k] for k < out_n[c] are the smoothed counts, the rest of `out` (created unless given) is not written;
        out_n[c] < the chromosome's length where the reference drops bins (fewer than 2h + 1 bins at some pass)."""
        torch = self.torch
        off = np.ascontiguousarray(chr_offset, np.int64)
        assert off.ndim == 1 and len(off) >= 1
        assert counts.dtype == torch.float32 and counts.is_contiguous() and counts.dim() == 1 and (counts.numel() == 0 or counts.device == self.device), "smooth: counts must be a dense float32 tensor on the context's device"
        assert int(off[-1]) <= counts.numel(), "smooth: the offsets reach past the counts"
        if out is None:
            out = torch.empty_like(counts)
        assert out.dtype == torch.float32 and out.is_contiguous() and out.dim() == 1 and out.numel() >= int(off[-1]) and (out.numel() == 0 or out.device == self.device)
        out_n = np.zeros(max(len(off) - 1, 1), np.int64)
        torch.cuda.synchronize(self.device)        # the tensors may have been written on torch's stream
        self._check(self.lib.canvas_smooth(self.ctx, C.c_int32(len(off) - 1), _np_ptr(off), C.c_void_p(counts.data_ptr()), C.c_int32(int(max_half_window)), C.c_void_p(out.data_ptr()), _np_ptr(out_n)))
        return out, out_n[:len(off) - 1]

    def segment_select(self, values, seg_offset, mode, out=None):
        """exact order statistics of many segments at once (canvas_segment_select): values = float32 device tensor, segment s = values[seg_offset[s]:seg_offset[s + 1]],
        mode = SELECT_MEDIAN_F32 / SELECT_MEDIAN_F64 (Median() with the even-length average in float / in double) / SELECT_UPPER (a[n/2]).  Returns (out, n_empty): out =
        float64 device tensor with one value per segment (0 for an empty one, created unless given)"""
        torch = self.torch
        off = np.ascontiguousarray(seg_offset, np.int64)
        assert off.ndim == 1 and len(off) >= 1
        assert values.dtype == torch.float32 and values.is_contiguous() and values.dim() == 1 and (values.numel() == 0 or values.device == self.device), "segment_select: values must be a dense float32 tensor on the context's device"
        assert int(off.max()) <= values.numel(), "segment_select: the offsets reach past the values"
        nseg = len(off) - 1
        if out is None:
            out = torch.empty(max(nseg, 1), dtype=torch.float64, device=self.device)
        assert out.dtype == torch.float64 and out.is_contiguous() and out.dim() == 1 and out.numel() >= nseg and out.device == self.device
        nempty = C.c_int64(0)
        torch.cuda.synchronize(self.device)        # the tensors may have been written on torch's stream
        self._check(self.lib.canvas_segment_select(self.ctx, C.c_void_p(values.data_ptr()), C.c_int64(nseg), _np_ptr(off), C.c_int32(int(mode)), C.c_void_p(out.data_ptr()), C.byref(nempty)))
        return out[:nseg], nempty.value

    def call_diploid(self, counts, chr_seg_offset, seg_begin, seg_end, seg_bin_offset, chr_site_offset, site_pos, site_ref, site_alt, logistic=LOGISTIC_GERMLINE,
                     seg_start_ci=None, seg_end_ci=None):
        """CanvasDiploidCaller.CallVariants between the parsed files and the written ones (canvas_call_diploid).  counts: float32 device tensor of every bin; segments
        grouped by chromosome (chr_seg_offset[nchr + 1]) with zero-based seg_begin / seg_end and the bins seg_bin_offset[s] .. seg_bin_offset[s + 1]; sites grouped the same
        way (chr_site_offset) as int32 device tensors site_pos (one-based) / site_ref / site_alt.  Returns a dict of numpy arrays: per segment bin_count, median_count,
        site_count, informative, median_maf, cn, mcc (-1 = null), dist, dist2, qscore; per merged run run_first, run_last, run_begin, run_end, run_cn, run_mcc, run_qscore,
        run_filter (FILTER_Q10 | FILTER_L10KB), run_bin_count, run_median_count (and run_start_ci / run_end_ci when the segments' confidence intervals are given: the first
        segment's start interval, the last segment's end interval); diploid_coverage, mean_coverage, kept_sites, integer_sum (whether the mean came from the device)"""
        torch = self.torch
        cso = np.ascontiguousarray(chr_seg_offset, np.int64); csi = np.ascontiguousarray(chr_site_offset, np.int64)
        beg = np.ascontiguousarray(seg_begin, np.int32); end = np.ascontiguousarray(seg_end, np.int32); sbo = np.ascontiguousarray(seg_bin_offset, np.int64)
        nchr, nseg = len(cso) - 1, len(beg)
        if nchr < 0 or len(csi) != nchr + 1 or len(end) != nseg or len(sbo) != nseg + 1 or (nchr >= 0 and len(cso) and int(cso[-1]) != nseg):
            raise CanvasError("call_diploid: one begin / end per segment, nseg + 1 bin offsets, nchr + 1 chromosome offsets that end at the number of segments / sites")
        assert counts.dtype == torch.float32 and counts.is_contiguous() and counts.dim() == 1 and (counts.numel() == 0 or counts.device == self.device)
        for t in (site_pos, site_ref, site_alt):
            assert t.dtype == torch.int32 and t.is_contiguous() and t.dim() == 1 and t.numel() == site_pos.numel() and (t.numel() == 0 or t.device == self.device)
        if int(csi[-1]) != site_pos.numel():
            raise CanvasError("call_diploid: the chromosomes' site offsets must end at the number of sites")
        b4 = np.ascontiguousarray(logistic, np.float64)
        assert b4.shape == (4,)
        o, outs = self._diploid_outputs(max(nseg, 1))
        torch.cuda.synchronize(self.device)        # the tensors may have been written on torch's stream
        self._check(self.lib.canvas_call_diploid(self.ctx, C.c_int64(counts.numel()), C.c_void_p(counts.data_ptr()), C.c_int32(nchr), _np_ptr(cso), _np_ptr(beg), _np_ptr(end), _np_ptr(sbo),
                                                 _np_ptr(csi), C.c_void_p(site_pos.data_ptr()), C.c_void_p(site_ref.data_ptr()), C.c_void_p(site_alt.data_ptr()), _np_ptr(b4), *outs))
        return self._diploid_result(o, nseg, beg, end, sbo, seg_start_ci, seg_end_ci)

    @staticmethod
    def _diploid_outputs(n1):
        """the host arrays canvas_call_diploid / canvas_call_diploid_ids fill (room for n1 segments) and their pointers in the order of the C signature"""
        o = dict(median_count=np.zeros(n1, np.float64), site_offset=np.zeros(n1 + 1, np.int64), informative=np.zeros(n1, np.int32), median_maf=np.zeros(n1, np.float64),
                 cn=np.zeros(n1, np.int32), mcc=np.zeros(n1, np.int32), dist=np.zeros(n1, np.float64), dist2=np.zeros(n1, np.float64), qscore=np.zeros(n1, np.int32),
                 run_first=np.zeros(n1, np.int64), run_last=np.zeros(n1, np.int64), run_qscore=np.zeros(n1, np.int32), run_filter=np.zeros(n1, np.int32), run_median_count=np.zeros(n1, np.float64))
        o["_nruns"] = C.c_int64(0); o["_scal"] = np.zeros(2, np.float64); o["_info"] = np.zeros(4, np.int64)
        outs = [_np_ptr(o[k]) for k in ("median_count", "site_offset", "informative", "median_maf", "cn", "mcc", "dist", "dist2", "qscore")] + [C.byref(o["_nruns"])] + \
               [_np_ptr(o[k]) for k in ("run_first", "run_last", "run_qscore", "run_filter", "run_median_count", "_scal", "_info")]
        return o, outs

    @staticmethod
    def _diploid_result(o, nseg, beg, end, sbo, seg_start_ci, seg_end_ci):
        r, scal, info = o["_nruns"].value, o["_scal"], o["_info"]
        out = {k: (v[:r] if k.startswith("run_") else v[:nseg]) for k, v in o.items() if k != "site_offset" and not k.startswith("_")}
        out["site_count"] = np.diff(o["site_offset"][:nseg + 1]); out["bin_count"] = np.diff(sbo)
        f, l = out["run_first"], out["run_last"]
        out.update(run_begin=beg[f], run_end=end[l], run_cn=out["cn"][f], run_mcc=out["mcc"][f], run_bin_count=sbo[l + 1] - sbo[f],
                   diploid_coverage=float(scal[0]), mean_coverage=float(scal[1]), kept_sites=int(info[0]), integer_sum=bool(info[1]))
        if seg_start_ci is not None and seg_end_ci is not None:
            out.update(run_start_ci=np.asarray(seg_start_ci)[f], run_end_ci=np.asarray(seg_end_ci)[l])
        return out

    SEGMENT_TABLES_CAP = 65536                  # room Canvas.segment_tables / call_diploid_ids offer first when no cap_seg is given (a refused call reports the count: one repeat)

    def _segment_table_args(self, what, chr_offset, start, stop, segment_id, cov, cap_seg, counts):
        """checks the bins' tensors and picks the room for the tables: (n, nchr, cap, off, counts)"""
        torch = self.torch
        off = np.ascontiguousarray(chr_offset, np.int64)
        if off.ndim != 1 or len(off) < 2:
            raise CanvasError(what + ": chr_offset holds nchr + 1 entries, at least one chromosome")
        n, nchr = int(off[-1]), len(off) - 1
        for t in (start, stop, segment_id):
            assert t.dtype == torch.int32 and t.is_contiguous() and t.dim() == 1 and t.numel() >= n and (t.numel() == 0 or t.device == self.device), what + ": start / stop / segment_id must be dense int32 tensors on the context's device"
        if cov is not None:
            assert cov.dtype == torch.float64 and cov.is_contiguous() and cov.dim() == 1 and cov.numel() >= n and cov.device == self.device, what + ": cov must be a dense float64 tensor on the context's device"
            if counts is None:
                counts = torch.empty(max(n, 1), dtype=torch.float32, device=self.device)
            assert counts.dtype == torch.float32 and counts.is_contiguous() and counts.dim() == 1 and counts.numel() >= n and counts.device == self.device
        cap = max(0, min(n, self.SEGMENT_TABLES_CAP)) if cap_seg is None else int(cap_seg)
        return n, nchr, cap, off, counts

    @staticmethod
    def _segment_tables(nchr, cap):
        c1 = max(cap, 1)
        return dict(nseg=C.c_int64(-1), chr_seg_offset=np.zeros(nchr + 1, np.int64), seg_begin=np.zeros(c1, np.int32), seg_end=np.zeros(c1, np.int32), seg_bin_offset=np.zeros(c1 + 1, np.int64),
                    seg_ci4=np.zeros((c1, 4), np.int32))

    @staticmethod
    def _segment_tables_result(t, counts, n):
        s = t["nseg"].value
        ci = t["seg_ci4"][:s]
        return dict(nseg=s, chr_seg_offset=t["chr_seg_offset"], seg_begin=t["seg_begin"][:s], seg_end=t["seg_end"][:s], seg_bin_offset=t["seg_bin_offset"][:s + 1], seg_ci4=ci,
                    seg_start_ci=ci[:, 0:2], seg_end_ci=ci[:, 2:4], counts=None if counts is None else counts[:n])

    def segment_tables(self, chr_offset, start, stop, segment_id, cov=None, cap_seg=None, counts=None):
        """Segments.ReadSegments on device-resident bins (canvas_segment_tables): chr_offset[nchr + 1] as chromosome_offsets returns it, start / stop / segment_id int32 device
        tensors (the first chr_offset[-1] entries count), cov the float64 coverage or None.  A segment starts at the first bin of a chromosome and wherever the id differs from the
        bin before.  Returns dict(nseg, chr_seg_offset, seg_begin, seg_end, seg_bin_offset, seg_ci4 = [start.lo, start.hi, end.lo, end.hi] per segment, seg_start_ci, seg_end_ci,
        counts): the host tables call_diploid / call_somatic take, and counts = float32 device tensor of (float)cov (None without cov; written into `counts` when given).
        cap_seg: room for that many segments, more are refused; None: SEGMENT_TABLES_CAP first and, if the sample has more, once more with the count the refusal reported."""
        n, nchr, cap, off, counts = self._segment_table_args("segment_tables", chr_offset, start, stop, segment_id, cov, cap_seg, counts)
        self.torch.cuda.synchronize(self.device)        # the tensors may have been written on torch's stream
        while True:
            t = self._segment_tables(nchr, cap)
            rc = self.lib.canvas_segment_tables(self.ctx, C.c_int64(n), C.c_int32(nchr), _np_ptr(off), C.c_void_p(start.data_ptr()), C.c_void_p(stop.data_ptr()), C.c_void_p(segment_id.data_ptr()),
                                                C.c_void_p(cov.data_ptr()) if cov is not None else None, C.c_int64(cap), C.byref(t["nseg"]), _np_ptr(t["chr_seg_offset"]), _np_ptr(t["seg_begin"]),
                                                _np_ptr(t["seg_end"]), _np_ptr(t["seg_bin_offset"]), _np_ptr(t["seg_ci4"]), C.c_void_p(counts.data_ptr()) if cov is not None else None)
            if rc == -1 and cap_seg is None and cap < t["nseg"].value <= n:      # more segments than the first offer (any other refusal comes back from the repeat)
                cap = t["nseg"].value
                continue
            self._check(rc)
            return self._segment_tables_result(t, counts, n)

    def call_diploid_ids(self, chr_offset, start, stop, segment_id, cov, chr_site_offset, site_pos, site_ref, site_alt, logistic=LOGISTIC_GERMLINE, cap_seg=None, counts=None):
        """segment_tables, then call_diploid on its tables and float counts, in one library call (canvas_call_diploid_ids): the bins as for segment_tables (cov is required), the
        sites as for call_diploid.  Returns call_diploid's dict (with run_start_ci / run_end_ci) plus `tables`, the dict of segment_tables.  cap_seg as for segment_tables."""
        torch = self.torch
        n, nchr, cap, off, counts = self._segment_table_args("call_diploid_ids", chr_offset, start, stop, segment_id, cov, cap_seg, counts)
        if cov is None:
            raise CanvasError("call_diploid_ids: the coverage is required")
        csi = np.ascontiguousarray(chr_site_offset, np.int64)
        for t in (site_pos, site_ref, site_alt):
            assert t.dtype == torch.int32 and t.is_contiguous() and t.dim() == 1 and t.numel() == site_pos.numel() and (t.numel() == 0 or t.device == self.device)
        if len(csi) != nchr + 1 or int(csi[-1]) != site_pos.numel():
            raise CanvasError("call_diploid_ids: nchr + 1 site offsets that end at the number of sites")
        b4 = np.ascontiguousarray(logistic, np.float64)
        assert b4.shape == (4,)
        torch.cuda.synchronize(self.device)        # the tensors may have been written on torch's stream
        while True:
            t = self._segment_tables(nchr, cap)
            o, outs = self._diploid_outputs(max(cap, 1))
            rc = self.lib.canvas_call_diploid_ids(self.ctx, C.c_int64(n), C.c_int32(nchr), _np_ptr(off), C.c_void_p(start.data_ptr()), C.c_void_p(stop.data_ptr()), C.c_void_p(segment_id.data_ptr()),
                                                  C.c_void_p(cov.data_ptr()), C.c_int64(cap), _np_ptr(csi), C.c_void_p(site_pos.data_ptr()), C.c_void_p(site_ref.data_ptr()),
                                                  C.c_void_p(site_alt.data_ptr()), _np_ptr(b4), C.byref(t["nseg"]), _np_ptr(t["chr_seg_offset"]), _np_ptr(t["seg_begin"]), _np_ptr(t["seg_end"]),
                                                  _np_ptr(t["seg_bin_offset"]), _np_ptr(t["seg_ci4"]), C.c_void_p(counts.data_ptr()), *outs)
            if rc == -1 and cap_seg is None and cap < t["nseg"].value <= n:      # more segments than the first offer (any other refusal comes back from the repeat)
                cap = t["nseg"].value
                continue
            self._check(rc)
            tab = self._segment_tables_result(t, counts, n)
            out = self._diploid_result(o, tab["nseg"], tab["seg_begin"], tab["seg_end"], tab["seg_bin_offset"], tab["seg_start_ci"], tab["seg_end_ci"])
            out["tables"] = tab
            return out

    def germline_flow(self, bases, masks, hits, lens, is_autosome, chr_site_offset, site_pos, site_ref, site_alt, counts_per_bin=100, bin_size=-1, mode=MODE_TDR, flags=0,
                      min_bins_per_gc=100, max_inter_bin_dist=1000000, is_y=None, pos0=None, logistic=LOGISTIC_GERMLINE, cap_bins=None, method="hmm", partition=None,
                      excluded=None, ploidy=None):
        """The germline sample from hit arrays to copy-number calls in one Python call, the counterpart of tumor_normal_flow: sample_pipeline (bin -> clean -> F2 -> PerSampleHMM ->
        segment ids), then call_diploid_ids on the arrays it left on the device — no *.partitioned text and no per-bin array on the host in between.  The per-base inputs and
        options are sample_pipeline's; the sites are call_diploid's (site_ref / site_alt may be the int32 counters snv_count filled).  Returns sample_pipeline's dict (bin_size,
        total, n_out, lsd, off, nseg) plus bins (the cleaned chr / start / stop / gc / count tensors), cov, state, seg (device tensors, n_out entries) and calls =
        call_diploid_ids' dict.
        method "cbs" / "wavelets" (the methods the reference's workflows run): bin_sample -> clean -> quantize_f2 -> chromosome_offsets -> cbs / wavelets with the options in
        `partition` (is_germline=True unless it says otherwise) -> partition_states -> segment_ids with max_inter_bin_dist and the optional excluded / ploidy ->
        call_diploid_ids, stage by stage on the device; `state` then holds the partition states.  excluded / ploidy need one of these two methods."""
        torch = self.torch
        if method not in ("hmm", "cbs", "wavelets"):
            raise CanvasError("germline_flow: method is \"hmm\", \"cbs\" or \"wavelets\"")
        if method == "hmm" and (partition or excluded is not None or ploidy is not None):
            raise CanvasError("germline_flow: partition options, excluded intervals and ploidy records need method \"cbs\" or \"wavelets\"")
        cap = int(cap_bins) if cap_bins is not None else int(sum(int(l) for l in lens) // 50) + 64
        mk = lambda dt: torch.empty(cap, dtype=dt, device=self.device)
        out = dict(chr=mk(torch.int32), start=mk(torch.int32), stop=mk(torch.int32), gc=mk(torch.int32), count=mk(torch.float32))
        cov, state, seg = mk(torch.float64), mk(torch.int32), mk(torch.int32)
        torch.cuda.synchronize(self.device)        # the inputs may have been written on torch's stream
        if method == "hmm":
            r = self.sample_pipeline(bases, masks, hits, lens, is_autosome, out, cov, state, seg, counts_per_bin=counts_per_bin, bin_size=bin_size, mode=mode, flags=flags,
                                     min_bins_per_gc=min_bins_per_gc, max_inter_bin_dist=max_inter_bin_dist, is_y=is_y, pos0=pos0)
        else:
            if pos0 is None:
                _, _, total, bs = self.bin_sample(bases, masks, hits, lens, is_autosome, counts_per_bin, bin_size, mode, out=out)
            else:
                _, _, total, bs = self.bin_sample_packed(bases, hits, lens, pos0, is_autosome, counts_per_bin, bin_size, mode, out=out)
            n_out, lsd, _ = self.clean(out, total, is_autosome, flags, min_bins_per_gc, is_y=is_y)
            self.quantize_f2(out["count"], n_out, out=cov)
            off = self.chromosome_offsets(out["chr"], n_out, len(lens))
            if method == "cbs":
                seg_len, nseg_chr, _ = self.cbs(cov, off, **(partition or {}))
                self.partition_states(off, seg_len=seg_len, nseg=nseg_chr, out=state)
            else:
                self.partition_states(off, breakpoints=self.wavelets(cov, off, **dict(dict(is_germline=True), **(partition or {}))), out=state)
            _, nseg = self.segment_ids(off, state, out["start"], out["stop"], max_inter_bin_dist, excluded, out=seg, ploidy=ploidy)
            r = dict(bin_size=bs, total=total, n_out=n_out, lsd=lsd, off=off, nseg=nseg)
        n = r["n_out"]
        calls = self.call_diploid_ids(r["off"], out["start"], out["stop"], seg, cov, chr_site_offset, site_pos, site_ref, site_alt, logistic=logistic)
        res = {k: r[k] for k in ("bin_size", "total", "n_out", "lsd", "off", "nseg")}
        res.update(bins={k: v[:n] for k, v in out.items()}, cov=cov[:n], state=state[:n], seg=seg[:n], calls=calls)
        return res

    def somatic_model_fit(self, coverage, maf, weight, length, coverage_weighting_factor, genome_length, min_coverage, max_coverage, minimum_purity_hard_limit=20,
                          min_minor_allele_coverage=0.0, is_enrichment=False, fixed_percent_purity=-1, fixed_coverage=-1, all_models=True, **params):
        """CanvasSomaticCaller's purity / ploidy grid search (canvas_somatic_model_fit; ModelOverallCoverageAndPurity, SomaticCaller.cs:1870-2117) over the usable segments:
        coverage / maf (< 0: none) / weight as float64 and length (End - Begin) as int32, all four numpy arrays or all four tensors on the context's device (per-segment median
        count and upper median of the folded frequencies are what Canvas.segment_select gives).  coverage_weighting_factor is CoverageWeightingFactor (already divided by the
        median level); **params override SOMATIC_DEFAULTS.  Returns a dict: the best model (model, coverage, percent_purity, purity, diploid_coverage, deviation,
        precision_deviation, accuracy_deviation, ploidy, percent_normal, diploid_distance, percent_cn, score, inter_model_distance), info, nmodels / nvalid / nscored,
        best_deviation, worst_allowed_deviation, seg_point / seg_distance (the best model's assignment), times_ms (host_table, upload, device, selection) and, with
        all_models, `models`: one array per column of PurityModel.txt in grid order.  CanvasError carries .code (ERR_SOMATIC_NO_MODEL, ERR_SOMATIC_NO_SCORE, -1) and,
        for the two somatic codes, .partial with what was filled."""
        torch = self.torch
        on_device = hasattr(coverage, "data_ptr")
        arrs = (coverage, maf, weight, length)
        if on_device:
            for t, dt in zip(arrs, (torch.float64, torch.float64, torch.float64, torch.int32)):
                assert hasattr(t, "data_ptr") and t.dtype == dt and t.is_contiguous() and t.dim() == 1 and t.numel() == coverage.numel() and t.device == self.device, \
                    "somatic_model_fit: float64 coverage / maf / weight and int32 length, dense and on the context's device"
            nseg = coverage.numel()
            ptrs = [C.c_void_p(t.data_ptr()) for t in arrs]
            torch.cuda.synchronize(self.device)        # the tensors may have been written on torch's stream
        else:
            arrs = tuple(np.ascontiguousarray(a, dt) for a, dt in zip(arrs, (np.float64, np.float64, np.float64, np.int32)))
            nseg = len(arrs[0])
            assert all(a.ndim == 1 and len(a) == nseg for a in arrs), "somatic_model_fit: one coverage, maf, weight and length per segment"
            ptrs = [_np_ptr(a) for a in arrs]
        unknown = set(params) - set(SOMATIC_DEFAULTS)
        if unknown:
            raise TypeError("somatic_model_fit: unknown parameters %s" % sorted(unknown))
        sp = SomaticParams(**dict(SOMATIC_DEFAULTS, **params))
        grid = SomaticGrid(int(min_coverage), int(max_coverage), int(minimum_purity_hard_limit), int(fixed_percent_purity), int(fixed_coverage), int(bool(is_enrichment)),
                           float(min_minor_allele_coverage), float(coverage_weighting_factor), int(genome_length))
        res = SomaticResult()
        n1 = max(nseg, 1)
        seg_point = np.zeros(n1, np.int32); seg_distance = np.zeros(n1, np.float64)
        cols, sm = {}, None
        if all_models:
            cap = 0
            lo, hi = (grid.fixed_coverage, grid.fixed_coverage) if grid.fixed_coverage >= 0 else (grid.min_coverage, grid.max_coverage)
            if 1 <= lo and hi <= 100000 and np.isfinite(grid.min_minor_allele_coverage):      # otherwise the call refuses the grid
                cap = len(somatic_grid(grid.min_coverage, grid.max_coverage, grid.minimum_purity_hard_limit, grid.min_minor_allele_coverage, grid.fixed_percent_purity, grid.fixed_coverage))
            c1 = max(cap, 1)
            cols = dict(coverage=np.zeros(c1, np.int32), percent_purity=np.zeros(c1, np.int32), deviation=np.zeros(c1), precision_deviation=np.zeros(c1), accuracy_deviation=np.zeros(c1),
                        ploidy=np.zeros(c1), percent_normal=np.zeros(c1), percent_cn=np.zeros((c1, SOMATIC_MAX_CN + 1)), diploid_distance=np.zeros(c1), flags=np.zeros(c1, np.int32), score=np.zeros(c1))
            sm = SomaticModels(cap, *[c.ctypes.data for c in cols.values()])
        fn = self.lib.canvas_somatic_model_fit
        fn.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        rc = fn(self.ctx, nseg, *ptrs, int(on_device), C.byref(grid), C.byref(sp), C.byref(res), _np_ptr(seg_point), _np_ptr(seg_distance), C.byref(sm) if sm is not None else None)
        M = res.nmodels
        out = dict(model=res.best_model, coverage=res.best_coverage, percent_purity=res.best_percent_purity, info=res.info, nmodels=M, nvalid=res.nvalid, nscored=res.nscored,
                   diploid_coverage=res.diploid_coverage, purity=res.purity, deviation=res.deviation, precision_deviation=res.precision_deviation,
                   accuracy_deviation=res.accuracy_deviation, ploidy=res.ploidy, percent_normal=res.percent_normal, diploid_distance=res.diploid_distance,
                   percent_cn=np.array(res.percent_cn[:sp.maximum_copy_number + 1]), score=res.score, inter_model_distance=res.inter_model_distance,
                   best_deviation=res.best_deviation, worst_allowed_deviation=res.worst_allowed_deviation, seg_point=seg_point[:nseg], seg_distance=seg_distance[:nseg],
                   times_ms=dict(host_table=res.host_table_ms, upload=res.upload_ms, device=res.device_ms, selection=res.selection_ms))
        if all_models:
            out["models"] = {k: (v[:M, :sp.maximum_copy_number + 1] if k == "percent_cn" else v[:M]) for k, v in cols.items()}
        if rc != 0:
            e = CanvasError(f"libcanvas_hip error {rc}: {self.lib.canvas_last_error(self.ctx).decode()}")
            e.code = rc
            e.partial = out if rc in (ERR_SOMATIC_NO_MODEL, ERR_SOMATIC_NO_SCORE) else None
            raise e
        return out

    def call_somatic(self, counts, chr_seg_offset, seg_begin, seg_end, seg_bin_offset, chr_site_offset, site_pos, site_ref, site_alt, genome_length, seg_ref_cn=None,
                     excluded=None, **params):
        """CanvasSomaticCaller.CallVariants between the parsed files and the written ones, with the model fit in the middle (canvas_call_somatic).  Bins, segments and
        sites as Canvas.call_diploid takes them; seg_ref_cn: the reference copy number per segment (None: 2 everywhere); excluded: per chromosome (starts, stops) of the
        excluded intervals, sorted by start (None: none); **params override SOMATIC_CALL_DEFAULTS and SOMATIC_DEFAULTS.  Returns a dict: every array of
        canvas_somatic_call_out (per segment, and per run cut to nruns), every field of canvas_somatic_call_scalars, site_count, and `fit`: the fields of
        canvas_somatic_result.  CanvasError carries .code (ERR_SOMATIC_FEW_SEGMENTS, ERR_SOMATIC_NO_MODEL, ERR_SOMATIC_NO_SCORE, -1) and .partial, the same dict with the
        stages that were filled (`stages`: 0, 2 or 3)."""
        torch = self.torch
        cso = np.ascontiguousarray(chr_seg_offset, np.int64); csi = np.ascontiguousarray(chr_site_offset, np.int64)
        beg = np.ascontiguousarray(seg_begin, np.int32); end = np.ascontiguousarray(seg_end, np.int32); sbo = np.ascontiguousarray(seg_bin_offset, np.int64)
        nchr, nseg = len(cso) - 1, len(beg)
        if nchr < 0 or len(csi) != nchr + 1 or len(end) != nseg or len(sbo) != nseg + 1 or int(cso[-1]) != nseg:
            raise CanvasError("call_somatic: one begin / end per segment, nseg + 1 bin offsets, nchr + 1 chromosome offsets that end at the number of segments / sites")
        assert counts.dtype == torch.float32 and counts.is_contiguous() and counts.dim() == 1 and (counts.numel() == 0 or counts.device == self.device)
        for t in (site_pos, site_ref, site_alt):
            assert t.dtype == torch.int32 and t.is_contiguous() and t.dim() == 1 and t.numel() == site_pos.numel() and (t.numel() == 0 or t.device == self.device)
        if int(csi[-1]) != site_pos.numel():
            raise CanvasError("call_somatic: the chromosomes' site offsets must end at the number of sites")
        ref = None
        if seg_ref_cn is not None:
            ref = np.ascontiguousarray(seg_ref_cn, np.int32)
            assert ref.shape == (nseg,)
        eo, es, ee = self._interval_tables(excluded, nchr)
        cp = self._somatic_call_params("call_somatic", genome_length, params)
        arrays, co = self._somatic_call_outputs(max(nseg, 1))
        sc = SomaticCallScalars(); res = SomaticResult()
        fn = self.lib.canvas_call_somatic
        fn.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int32] + [C.c_void_p] * 16
        opt = lambda a: _np_ptr(a) if a is not None else None
        torch.cuda.synchronize(self.device)        # the tensors may have been written on torch's stream
        rc = fn(self.ctx, counts.numel(), C.c_void_p(counts.data_ptr()), nchr, _np_ptr(cso), _np_ptr(beg), _np_ptr(end), _np_ptr(sbo), _np_ptr(csi), C.c_void_p(site_pos.data_ptr()),
                C.c_void_p(site_ref.data_ptr()), C.c_void_p(site_alt.data_ptr()), opt(ref), opt(eo), opt(es), opt(ee), C.byref(cp), C.byref(co), C.byref(sc), C.byref(res))
        out = self._somatic_call_result(arrays, sc, res, cp, nseg)
        if rc != 0:
            e = CanvasError(f"libcanvas_hip error {rc}: {self.lib.canvas_last_error(self.ctx).decode()}")
            e.code = rc
            e.partial = out
            raise e
        return out

    @staticmethod
    def _interval_tables(intervals, nchr, columns=2):
        """per chromosome (starts, stops[, values]) -> (offsets int64[nchr + 1], one int32 array per column, never empty); (None, ...) for None"""
        if intervals is None:
            return (None,) * (columns + 1)
        assert len(intervals) == nchr
        off = np.concatenate([[0], np.cumsum([len(e[0]) for e in intervals])]).astype(np.int64)
        return (off,) + tuple(np.ascontiguousarray(np.concatenate([np.asarray(e[k], np.int32) for e in intervals] + [np.zeros(1, np.int32)]), np.int32) for k in range(columns))

    @staticmethod
    def _somatic_call_params(what, genome_length, params):
        unknown = set(params) - set(SOMATIC_DEFAULTS) - set(SOMATIC_CALL_DEFAULTS)
        if unknown:
            raise TypeError("%s: unknown parameters %s" % (what, sorted(unknown)))
        fitp = SomaticParams(**dict(SOMATIC_DEFAULTS, **{k: v for k, v in params.items() if k in SOMATIC_DEFAULTS}))
        own = dict(SOMATIC_CALL_DEFAULTS, genome_length=int(genome_length), **{k: v for k, v in params.items() if k in SOMATIC_CALL_DEFAULTS})
        own["is_enrichment"] = int(bool(own["is_enrichment"]))
        return SomaticCallParams(fit=fitp, **own)

    @staticmethod
    def _somatic_call_outputs(n1):
        """the host arrays of canvas_somatic_call_out (room for n1 segments) and the struct that points at them"""
        arrays = {name: np.zeros(n1 + 1 if kind == "seg1" else n1, dt) for name, dt, kind in SOMATIC_CALL_OUT}
        return arrays, SomaticCallOut(*[arrays[name].ctypes.data for name, _, _ in SOMATIC_CALL_OUT])

    @staticmethod
    def _somatic_call_result(arrays, sc, res, cp, nseg):
        r = sc.nruns
        out = {name: (arrays[name][:r] if kind == "run" else arrays[name][:nseg + 1] if kind == "seg1" else arrays[name][:nseg]) for name, _, kind in SOMATIC_CALL_OUT}
        out["site_count"] = np.diff(out["seg_site_offset"])
        out.update({name: getattr(sc, name) for name, _ in SomaticCallScalars._fields_})
        out["fit"] = {name: (np.array(res.percent_cn[:cp.fit.maximum_copy_number + 1]) if name == "percent_cn" else getattr(res, name)) for name, _ in SomaticResult._fields_}
        return out

    def call_somatic_ids(self, chr_offset, start, stop, segment_id, cov, chr_site_offset, site_pos, site_ref, site_alt, genome_length, ploidy=None, excluded=None, cap_seg=None,
                         counts=None, **params):
        """segment_tables, the reference copy numbers of the segments from the optional ploidy records, then call_somatic on the tables and float counts, in one library call
        (canvas_call_somatic_ids): the bins as for segment_tables (cov is required), the sites, excluded intervals and **params as for call_somatic, ploidy as for segment_ids
        (per chromosome (one-based starts, ends, copy numbers); None: 2 everywhere).  Returns call_somatic's dict plus `tables`, the dict of segment_tables, and `seg_ref_cn`.
        cap_seg as for segment_tables.  CanvasError carries .code and, for the somatic codes, .partial: the same dict with the stages that were filled."""
        torch = self.torch
        n, nchr, cap, off, counts = self._segment_table_args("call_somatic_ids", chr_offset, start, stop, segment_id, cov, cap_seg, counts)
        if cov is None:
            raise CanvasError("call_somatic_ids: the coverage is required")
        csi = np.ascontiguousarray(chr_site_offset, np.int64)
        for t in (site_pos, site_ref, site_alt):
            assert t.dtype == torch.int32 and t.is_contiguous() and t.dim() == 1 and t.numel() == site_pos.numel() and (t.numel() == 0 or t.device == self.device)
        if len(csi) != nchr + 1 or int(csi[-1]) != site_pos.numel():
            raise CanvasError("call_somatic_ids: nchr + 1 site offsets that end at the number of sites")
        eo, es, ee = self._interval_tables(excluded, nchr)
        po, ps, pe, pc = self._interval_tables(ploidy, nchr, columns=3)
        cp = self._somatic_call_params("call_somatic_ids", genome_length, params)
        fn = self.lib.canvas_call_somatic_ids
        fn.argtypes = [C.c_void_p, C.c_int64, C.c_int32] + [C.c_void_p] * 5 + [C.c_int64] + [C.c_void_p] * 23
        opt = lambda a: _np_ptr(a) if a is not None else None
        torch.cuda.synchronize(self.device)        # the tensors may have been written on torch's stream
        while True:
            t = self._segment_tables(nchr, cap)
            arrays, co = self._somatic_call_outputs(max(cap, 1))
            ref = np.zeros(max(cap, 1), np.int32)
            sc = SomaticCallScalars(); res = SomaticResult()
            rc = fn(self.ctx, n, nchr, _np_ptr(off), C.c_void_p(start.data_ptr()), C.c_void_p(stop.data_ptr()), C.c_void_p(segment_id.data_ptr()), C.c_void_p(cov.data_ptr()), cap,
                    _np_ptr(csi), C.c_void_p(site_pos.data_ptr()), C.c_void_p(site_ref.data_ptr()), C.c_void_p(site_alt.data_ptr()), opt(po), opt(ps), opt(pe), opt(pc),
                    opt(eo), opt(es), opt(ee), C.byref(cp), C.byref(t["nseg"]), _np_ptr(t["chr_seg_offset"]), _np_ptr(t["seg_begin"]), _np_ptr(t["seg_end"]),
                    _np_ptr(t["seg_bin_offset"]), _np_ptr(t["seg_ci4"]), C.c_void_p(counts.data_ptr()), _np_ptr(ref), C.byref(co), C.byref(sc), C.byref(res))
            if rc == -1 and cap_seg is None and cap < t["nseg"].value <= n:      # more segments than the first offer (any other refusal comes back from the repeat)
                cap = t["nseg"].value
                continue
            if rc == -1:                      # refused by the tables, the ploidy records or the call's own checks: nothing to hand back
                e = CanvasError(f"libcanvas_hip error {rc}: {self.lib.canvas_last_error(self.ctx).decode()}")
                e.code = rc
                e.partial = None
                raise e
            tab = self._segment_tables_result(t, counts, n)
            out = self._somatic_call_result(arrays, sc, res, cp, tab["nseg"])
            out.update(tables=tab, seg_ref_cn=ref[:tab["nseg"]])
            if rc != 0:
                e = CanvasError(f"libcanvas_hip error {rc}: {self.lib.canvas_last_error(self.ctx).decode()}")
                e.code = rc
                e.partial = out
                raise e
            return out

    def segment_ids(self, chr_offset, state, start, stop, max_inter_bin_dist=1000000, excluded=None, out=None, ploidy=None):
        """DeriveSegments + PostProcessSegments; excluded = per-chromosome list of (starts, stops) of the -b BED file; ploidy = per-chromosome list
        of (one-based starts, ends, copy numbers) of the -p VCF"""
        torch = self.torch
        off = np.ascontiguousarray(chr_offset, np.int64)
        seg = out[:int(off[-1])] if out is not None else torch.empty(int(off[-1]), dtype=torch.int32, device=self.device)
        nseg = C.c_int64(0)
        if ploidy is not None:
            cat = lambda k, src: np.ascontiguousarray(np.concatenate([np.asarray(e[k], np.int32) for e in src] + [np.zeros(1, np.int32)]), np.int32)
            po = np.concatenate([[0], np.cumsum([len(e[0]) for e in ploidy])]).astype(np.int64)
            ps, pe, pc = cat(0, ploidy), cat(1, ploidy), cat(2, ploidy)
            if excluded is not None:
                eo = np.concatenate([[0], np.cumsum([len(e[0]) for e in excluded])]).astype(np.int64); es, ee = cat(0, excluded), cat(1, excluded)
            self._check(self.lib.canvas_segment_ids_ploidy(self.ctx, len(off) - 1, _np_ptr(off), C.c_void_p(state.data_ptr()), C.c_void_p(start.data_ptr()),
                                                           C.c_void_p(stop.data_ptr()), max_inter_bin_dist,
                                                           _np_ptr(eo) if excluded is not None else None, _np_ptr(es) if excluded is not None else None,
                                                           _np_ptr(ee) if excluded is not None else None, _np_ptr(po), _np_ptr(ps), _np_ptr(pe), _np_ptr(pc),
                                                           C.c_void_p(seg.data_ptr()), C.byref(nseg)))
        elif excluded is None:
            self._check(self.lib.canvas_segment_ids(self.ctx, len(off) - 1, _np_ptr(off), C.c_void_p(state.data_ptr()), C.c_void_p(start.data_ptr()),
                                                    C.c_void_p(stop.data_ptr()), max_inter_bin_dist, C.c_void_p(seg.data_ptr()), C.byref(nseg)))
        else:
            eo = np.concatenate([[0], np.cumsum([len(e[0]) for e in excluded])]).astype(np.int64)
            es = np.ascontiguousarray(np.concatenate([np.asarray(e[0], np.int32) for e in excluded]) if eo[-1] else np.zeros(1), np.int32)
            ee = np.ascontiguousarray(np.concatenate([np.asarray(e[1], np.int32) for e in excluded]) if eo[-1] else np.zeros(1), np.int32)
            self._check(self.lib.canvas_segment_ids_filtered(self.ctx, len(off) - 1, _np_ptr(off), C.c_void_p(state.data_ptr()), C.c_void_p(start.data_ptr()),
                                                             C.c_void_p(stop.data_ptr()), max_inter_bin_dist, _np_ptr(eo), _np_ptr(es), _np_ptr(ee),
                                                             C.c_void_p(seg.data_ptr()), C.byref(nseg)))
        return seg, nseg.value

    def partition_states(self, chr_offset, seg_len=None, nseg=None, breakpoints=None, out=None):
        """What cbs (seg_len device tensor + nseg per chromosome) or wavelets (breakpoints: one array of bin indices per chromosome) returned, as the per-bin state segment_ids
        takes (canvas_partition_states_cbs / canvas_partition_states_breakpoints): the zero-based ordinal, within its chromosome, of the segment that holds the bin, -1
        throughout a chromosome for which the method derives no segment.  Returns the int32 device tensor (chr_offset[-1] entries, a view of `out` when given)."""
        torch = self.torch
        off = np.ascontiguousarray(chr_offset, np.int64)
        if off.ndim != 1 or len(off) < 2:
            raise CanvasError("partition_states: chr_offset holds nchr + 1 entries, at least one chromosome")
        if (seg_len is None) != (nseg is None) or (seg_len is None) == (breakpoints is None):
            raise CanvasError("partition_states: either seg_len and nseg (CBS) or breakpoints (Wavelets)")
        n, nchr = max(int(off[-1]), 0), len(off) - 1
        if out is not None:
            assert out.dtype == torch.int32 and out.is_contiguous() and out.dim() == 1 and out.numel() >= n and out.device == self.device, "partition_states: out must be a dense int32 tensor on the context's device"
        state = out[:n] if out is not None else torch.empty(n, dtype=torch.int32, device=self.device)
        torch.cuda.synchronize(self.device)        # the tensors may have been written on torch's stream
        if breakpoints is None:
            assert seg_len.dtype == torch.int32 and seg_len.is_contiguous() and seg_len.dim() == 1 and seg_len.numel() >= n and seg_len.device == self.device, "partition_states: seg_len must be a dense int32 tensor on the context's device"
            hn = np.ascontiguousarray(nseg, np.int32)
            if hn.shape != (nchr,):
                raise CanvasError("partition_states: one nseg per chromosome")
            self._check(self.lib.canvas_partition_states_cbs(self.ctx, C.c_int32(nchr), _np_ptr(off), C.c_void_p(seg_len.data_ptr()), _np_ptr(hn), C.c_void_p(state.data_ptr())))
        else:
            if len(breakpoints) != nchr:
                raise CanvasError("partition_states: one array of breakpoints per chromosome")
            bo = np.concatenate([[0], np.cumsum([len(b) for b in breakpoints])]).astype(np.int64)
            bp = np.ascontiguousarray(np.concatenate([np.asarray(b, np.int32).reshape(-1) for b in breakpoints] + [np.zeros(1, np.int32)]), np.int32)
            self._check(self.lib.canvas_partition_states_breakpoints(self.ctx, C.c_int32(nchr), _np_ptr(off), _np_ptr(bp), _np_ptr(bo), C.c_void_p(state.data_ptr())))
        return state

    def cbs(self, cov, chr_offset, alpha=0.01, nperm=10000, undo=0, undo_sd=3.0):
        """CBSRunner.Run (CBSRunner.cs:40-151); undo: 0 None, 1 Prune, 2 SDUndo"""
        torch = self.torch
        off = np.ascontiguousarray(chr_offset, np.int64)
        seg_len = torch.zeros(int(off[-1]) + 1, dtype=torch.int32, device=self.device)
        nseg = np.zeros(len(off) - 1, np.int32); stats = np.zeros(8, np.int64)
        self._check(self.lib.canvas_cbs_undo(self.ctx, len(off) - 1, C.c_void_p(cov.data_ptr()), _np_ptr(off), C.c_double(alpha), C.c_uint32(nperm), undo, C.c_double(undo_sd),
                                             C.c_void_p(seg_len.data_ptr()), _np_ptr(nseg), _np_ptr(stats)))
        return seg_len, nseg, stats

    def wavelets(self, cov, chr_offset, is_germline=False, threshold_lower=0.05, threshold_upper=80.0, mad_factor=5.0, window=100000, min_size=10):
        """WaveletsRunner.Run up to the breakpoints (WaveletsRunner.cs:52-150): one array of segment-start bin indices per chromosome"""
        off = np.ascontiguousarray(chr_offset, np.int64)
        nchr = len(off) - 1
        out = np.zeros(int(off[-1] - off[0]) + nchr + 1, np.int32); oo = np.zeros(nchr + 1, np.int64)
        self._check(self.lib.canvas_wavelets(self.ctx, nchr, C.c_void_p(cov.data_ptr()), _np_ptr(off), int(bool(is_germline)), C.c_double(threshold_lower),
                                             C.c_double(threshold_upper), C.c_double(mad_factor), int(window), int(min_size), _np_ptr(out), C.c_int64(len(out)), _np_ptr(oo)))
        return [out[oo[c]:oo[c + 1]].copy() for c in range(nchr)]

    def sample_pipeline(self, bases, masks, hits, lens, is_autosome, out, cov, state, seg, counts_per_bin=100, bin_size=-1, mode=3, flags=0, min_bins_per_gc=100,
                        max_inter_bin_dist=1000000, is_y=None, prepared=None, pos0=None):
        """bin_sample -> clean -> quantize_f2 -> chromosome_offsets -> hmm_per_sample -> segment_ids in ONE library call (canvas_sample_pipeline).
        Returns dict(bin_size, total, n_out, lsd, off, nseg, prepared); results are left in `out`, `cov`, `state`, `seg`.  Passing the returned `prepared` back repeats the
        call on the SAME tensors and options without marshalling the arguments again (every other argument is then ignored).
        pos0 given: `bases` / `hits` are the packed reference / hit planes (canvas_sample_pipeline_packed; `masks` is ignored)."""
        nchr = len(bases) if prepared is None else 0
        # the whole marshalled call (pointer tables, scalars, out-parameters) is cached per set of tensors: a native host keeps these arrays anyway, and per pass
        # the Python side is then one foreign call (building ~30 ctypes arguments costs ~0.1 ms, 3 % of a pass)
        if prepared is None:
            arr = lambda ts: (C.c_void_p * nchr)(*[C.c_void_p(t.data_ptr()) for t in ts])
            pb, pm, ph = arr(bases), (arr(masks) if pos0 is None else None), arr(hits)
            hl = np.ascontiguousarray(lens, np.int64); ia = np.ascontiguousarray(is_autosome, np.uint8); iy = None if is_y is None else np.ascontiguousarray(is_y, np.uint8)
            bs = C.c_int32(0); total = C.c_int64(0); nclean = C.c_int64(0); lsd = C.c_double(-1.0); nseg = C.c_int64(0); off = np.zeros(nchr + 1, np.int64)
            p0 = None if pos0 is None else np.ascontiguousarray(pos0, np.int64)
            head = (self.ctx, nchr, pb, pm, ph, _np_ptr(hl)) if p0 is None else (self.ctx, nchr, pb, ph, _np_ptr(hl), _np_ptr(p0))
            args = head + (_np_ptr(ia), None if iy is None else _np_ptr(iy),
                    int(counts_per_bin), int(bin_size), int(mode), C.c_uint32(flags), int(min_bins_per_gc), int(max_inter_bin_dist),
                    C.c_void_p(out["chr"].data_ptr()), C.c_void_p(out["start"].data_ptr()), C.c_void_p(out["stop"].data_ptr()),
                    C.c_void_p(out["gc"].data_ptr()), C.c_void_p(out["count"].data_ptr()), C.c_int64(int(out["chr"].numel())),
                    C.c_void_p(cov.data_ptr()), C.c_void_p(state.data_ptr()), C.c_void_p(seg.data_ptr()),
                    C.byref(bs), C.byref(total), C.byref(nclean), C.byref(lsd), _np_ptr(off), C.byref(nseg))
            prepared = dict(args=args, keep=(pb, pm, ph, hl, ia, iy, p0), outs=(bs, total, nclean, lsd, nseg, off), packed=p0 is not None)     # valid for exactly these tensors and options
        bs, total, nclean, lsd, nseg, off = prepared["outs"]
        self._check((self.lib.canvas_sample_pipeline_packed if prepared["packed"] else self.lib.canvas_sample_pipeline)(*prepared["args"]))
        return dict(bin_size=bs.value, total=total.value, n_out=nclean.value, lsd=lsd.value, off=off.copy(), nseg=nseg.value, prepared=prepared)

    def tumor_normal_flow(self, bases, masks, hits_t, fraglen_t, hits_n, lens, is_autosome, clean_flags, alpha=0.01, nperm=10000, counts_per_bin=100, is_y=None, keep=False, owner=None):
        """BASELINE configs[4] in memory, from the hit arrays of a tumour / normal pair to the CBS segment lengths: see _tumor_normal, whose dict this returns."""
        return self._tumor_normal(bases, masks, hits_t, fraglen_t, hits_n, lens, is_autosome, clean_flags, alpha, nperm, counts_per_bin, is_y, keep, owner)[0]

    def somatic_flow(self, bases, masks, hits_t, fraglen_t, hits_n, lens, is_autosome, clean_flags, chr_site_offset, site_pos, site_ref, site_alt, genome_length, excluded=None,
                     ploidy=None, alpha=0.01, nperm=10000, counts_per_bin=100, is_y=None, keep=False, max_inter_bin_dist=1000000, **somatic_params):
        """The tumour / normal pair from hit arrays to somatic copy-number calls in one Python call: tumor_normal_flow, partition_states on the CBS lengths it left on the
        device, segment_ids (max_inter_bin_dist, the optional excluded intervals and ploidy records) and call_somatic_ids (the sites, genome_length, the same excluded /
        ploidy and **somatic_params, as call_somatic takes them) — no per-bin array on the host in between.  excluded reaches both segment_ids (which walks the intervals
        of a chromosome by their end) and call_somatic (by their start): sort them by both.  Returns tumor_normal_flow's dict plus state and seg (int32 device tensors,
        n_clean entries) and calls = call_somatic_ids' dict."""
        res, dev = self._tumor_normal(bases, masks, hits_t, fraglen_t, hits_n, lens, is_autosome, clean_flags, alpha, nperm, counts_per_bin, is_y, keep, None)
        off, R = dev["off"], dev["bins"]
        state = self.partition_states(off, seg_len=dev["seg_len"], nseg=dev["nseg"])
        seg, _ = self.segment_ids(off, state, R["start"], R["stop"], max_inter_bin_dist, excluded, ploidy=ploidy)
        calls = self.call_somatic_ids(off, R["start"], R["stop"], seg, dev["cov"], chr_site_offset, site_pos, site_ref, site_alt, genome_length, ploidy=ploidy, excluded=excluded,
                                      **somatic_params)
        res.update(state=state, seg=seg, calls=calls)
        return res

    def _tumor_normal(self, bases, masks, hits_t, fraglen_t, hits_n, lens, is_autosome, clean_flags, alpha, nperm, counts_per_bin, is_y, keep, owner):
        """tumor_normal_flow's work: (its dict, the arrays it left on the device: bins = the cleaned SoA, cov, off, seg_len, nseg).
        BASELINE configs[4] in memory, the hand-offs of the reference's tumour / normal flow: CanvasBin -m GCContentWeighted on the tumour (bin size from
        the tumour's own rates) and -m TruncatedDynamicRange -z <that size> on the normal (same mask => same bins), CanvasNormalize's LSNorm ratio x 40
        (LSNormRatioCalculator.cs:31-44, CanvasNormalizeUtilities.cs:23-33), its "{count:F2}" file read back with float.Parse (IO.cs:21,40), CanvasClean,
        the F2 hand-off to CanvasPartition and CBS (alpha, nperm).  Returns a dict; with keep=True every intermediate array is kept for checking.
        owner given (one entry per chromosome): the chromosome-sharded flow over the communicator of the context — this rank holds the arrays of its own chromosomes only (None
        elsewhere); both binnings are canvas_bin_sample_sharded, the ratio and CanvasClean run on the whole genome on every rank, CBS is canvas_cbs_sharded: same result on every rank."""
        import time
        torch = self.torch
        nchr = len(bases)
        cap = int(sum(int(l) for l in lens) // 50) + 64
        mk = lambda dt: torch.empty(cap, dtype=dt, device=self.device)
        stage = {}; t_prev = [time.perf_counter()]

        def tick(name):
            self.synchronize(); torch.cuda.synchronize()
            now = time.perf_counter(); stage[name] = round(now - t_prev[0], 4); t_prev[0] = now
        T = dict(chr=mk(torch.int32), start=mk(torch.int32), stop=mk(torch.int32), gc=mk(torch.int32), count=mk(torch.float32))
        N = dict(chr=mk(torch.int32), start=mk(torch.int32), stop=mk(torch.int32), gc=mk(torch.int32), count=mk(torch.float32))
        if owner is None:
            _, perT, nT, bs = self.bin_sample_gcweighted(bases, masks, hits_t, fraglen_t, lens, is_autosome, counts_per_bin, -1, out=T)
            tick("bin_tumour_gcweighted")
            _, perN, nN, _ = self.bin_sample(bases, masks, hits_n, lens, is_autosome, counts_per_bin, bs, MODE_TDR, out=N)
        else:
            bs, nT = self.bin_sample_sharded(owner, bases, masks, hits_t, lens, is_autosome, T, counts_per_bin, -1, MODE_GCW, fraglens=fraglen_t)
            tick("bin_tumour_gcweighted")
            _, nN = self.bin_sample_sharded(owner, bases, masks, hits_n, lens, is_autosome, N, counts_per_bin, bs, MODE_TDR)
        tick("bin_normal")
        if nN != nT:
            raise CanvasError(f"tumour and normal bins differ ({nT} vs {nN}): they must share the reference mask")
        kidx, ratio, count, lsf = self.normalize_ratio(T["count"][:nT], N["count"][:nN], None, mode=0)
        k = int(kidx.numel())
        ki = kidx.long()
        R = dict(chr=T["chr"][:nT][ki].contiguous(), start=T["start"][:nT][ki].contiguous(), stop=T["stop"][:nT][ki].contiguous(), gc=T["gc"][:nT][ki].contiguous(),
                 count=self.quantize_f2(count, k).float().contiguous())       # the ratio file's F2 text, float.Parse'd by CanvasClean
        tick("normalize_ratio+f2")
        res = dict(bin_size=bs, n_bins=nT, n_ratio=k, library_size_factor=lsf)
        if keep:
            res.update(tumour={a: T[a][:nT].clone() for a in T}, normal_count=N["count"][:nN].clone(), keep_idx=kidx.clone(), ratio=ratio.clone(), ratio_count=count.clone(),
                       to_clean={a: R[a].clone() for a in R})
        n_out, lsd, info = self.clean(R, k, is_autosome, clean_flags, is_y=is_y)
        tick("clean")
        cov = self.quantize_f2(R["count"], n_out)
        off = self.chromosome_offsets(R["chr"], n_out, nchr)
        tick("f2+offsets")
        seg_len, nseg, stats = self.cbs(cov, off, alpha, nperm) if owner is None else self.cbs_sharded(owner, cov, off, alpha, nperm)
        tick("cbs")
        res.update(n_clean=n_out, local_sd=lsd, chr_offset=off, nseg=nseg, cbs_stats=stats, segments=int(nseg.sum()), stage_seconds=stage)
        if keep:
            res.update(cleaned={a: R[a][:n_out].clone() for a in R}, cov=cov.clone(), seg_len=seg_len)
        return res, dict(bins=R, cov=cov, off=off, seg_len=seg_len, nseg=nseg)

    def sample_pipeline_sharded(self, owner, bases, masks, hits, lens, is_autosome, out, cov, state, seg, counts_per_bin=100, bin_size=-1, mode=3, flags=0, min_bins_per_gc=100,
                                max_inter_bin_dist=1000000, is_y=None, pos0=None):
        """canvas_sample_pipeline_sharded: `owner[c]` = rank that holds chromosome c; bases / masks / hits are lists over ALL chromosomes with None for the ones this rank
        does not own.  Every rank gets the whole result (same dict as sample_pipeline)."""
        nchr = len(owner)
        tab = lambda ts: (C.c_void_p * nchr)(*[None if t is None else C.c_void_p(t.data_ptr()) for t in ts])
        ow = np.ascontiguousarray(owner, np.int32); hl = np.ascontiguousarray(lens, np.int64); ia = np.ascontiguousarray(is_autosome, np.uint8)
        iy = None if is_y is None else np.ascontiguousarray(is_y, np.uint8)
        bs = C.c_int32(0); total = C.c_int64(0); nclean = C.c_int64(0); lsd = C.c_double(-1.0); nseg = C.c_int64(0); off = np.zeros(nchr + 1, np.int64)
        if pos0 is not None:       # packed planes: `bases` = reference planes, `hits` = hit planes (None for chromosomes of other ranks), `masks` ignored
            p0 = np.ascontiguousarray(pos0, np.int64)
            self._check(self.lib.canvas_sample_pipeline_sharded_packed(self.ctx, nchr, _np_ptr(ow), tab(bases), tab(hits), _np_ptr(hl), _np_ptr(p0), _np_ptr(ia), None if iy is None else _np_ptr(iy),
                                                                       int(counts_per_bin), int(bin_size), int(mode), C.c_uint32(flags), int(min_bins_per_gc), int(max_inter_bin_dist),
                                                                       C.c_void_p(out["chr"].data_ptr()), C.c_void_p(out["start"].data_ptr()), C.c_void_p(out["stop"].data_ptr()),
                                                                       C.c_void_p(out["gc"].data_ptr()), C.c_void_p(out["count"].data_ptr()), C.c_int64(int(out["chr"].numel())),
                                                                       C.c_void_p(cov.data_ptr()), C.c_void_p(state.data_ptr()), C.c_void_p(seg.data_ptr()),
                                                                       C.byref(bs), C.byref(total), C.byref(nclean), C.byref(lsd), _np_ptr(off), C.byref(nseg)))
            return dict(bin_size=bs.value, total=total.value, n_out=nclean.value, lsd=lsd.value, off=off, nseg=nseg.value)
        self._check(self.lib.canvas_sample_pipeline_sharded(self.ctx, nchr, _np_ptr(ow), tab(bases), tab(masks), tab(hits), _np_ptr(hl), _np_ptr(ia), None if iy is None else _np_ptr(iy),
                                                            int(counts_per_bin), int(bin_size), int(mode), C.c_uint32(flags), int(min_bins_per_gc), int(max_inter_bin_dist),
                                                            C.c_void_p(out["chr"].data_ptr()), C.c_void_p(out["start"].data_ptr()), C.c_void_p(out["stop"].data_ptr()),
                                                            C.c_void_p(out["gc"].data_ptr()), C.c_void_p(out["count"].data_ptr()), C.c_int64(int(out["chr"].numel())),
                                                            C.c_void_p(cov.data_ptr()), C.c_void_p(state.data_ptr()), C.c_void_p(seg.data_ptr()),
                                                            C.byref(bs), C.byref(total), C.byref(nclean), C.byref(lsd), _np_ptr(off), C.byref(nseg)))
        return dict(bin_size=bs.value, total=total.value, n_out=nclean.value, lsd=lsd.value, off=off, nseg=nseg.value)

    def hmm_per_sample_sharded(self, owner, cov, chr_offset):
        """canvas_hmm_per_sample_sharded: every rank holds the whole coverage, decodes the chromosomes it owns and receives everybody's state runs (same return as hmm_per_sample)"""
        torch = self.torch
        off = np.ascontiguousarray(chr_offset, np.int64); ow = np.ascontiguousarray(owner, np.int32)
        state = torch.empty(max(int(off[-1]), 1), dtype=torch.int32, device=self.device)
        self._check(self.lib.canvas_hmm_per_sample_sharded(self.ctx, len(off) - 1, _np_ptr(ow), C.c_void_p(cov.data_ptr()), _np_ptr(off), C.c_void_p(state.data_ptr())))
        return state[:int(off[-1])]

    def cbs_sharded(self, owner, cov, chr_offset, alpha=0.01, nperm=10000, undo=0, undo_sd=3.0):
        """canvas_cbs_sharded: every rank holds the whole coverage, segments the chromosomes it owns and receives everybody's segments (same return as cbs)"""
        torch = self.torch
        off = np.ascontiguousarray(chr_offset, np.int64); ow = np.ascontiguousarray(owner, np.int32)
        seg_len = torch.zeros(int(off[-1]) + 1, dtype=torch.int32, device=self.device)
        nseg = np.zeros(len(off) - 1, np.int32); stats = np.zeros(8, np.int64)
        self._check(self.lib.canvas_cbs_sharded(self.ctx, len(off) - 1, _np_ptr(ow), C.c_void_p(cov.data_ptr()), _np_ptr(off), C.c_double(alpha), C.c_uint32(nperm), int(undo), C.c_double(undo_sd),
                                                C.c_void_p(seg_len.data_ptr()), _np_ptr(nseg), _np_ptr(stats)))
        return seg_len, nseg, stats

    def wavelets_sharded(self, owner, cov, chr_offset, is_germline=False, threshold_lower=0.05, threshold_upper=80.0, mad_factor=5.0, window=100000, min_size=10):
        """canvas_wavelets_sharded: same return as wavelets, on every rank"""
        off = np.ascontiguousarray(chr_offset, np.int64); ow = np.ascontiguousarray(owner, np.int32)
        nchr = len(off) - 1
        out = np.zeros(int(off[-1] - off[0]) + nchr + 1, np.int32); oo = np.zeros(nchr + 1, np.int64)
        self._check(self.lib.canvas_wavelets_sharded(self.ctx, nchr, _np_ptr(ow), C.c_void_p(cov.data_ptr()), _np_ptr(off), int(bool(is_germline)), C.c_double(threshold_lower),
                                                     C.c_double(threshold_upper), C.c_double(mad_factor), int(window), int(min_size), _np_ptr(out), C.c_int64(len(out)), _np_ptr(oo)))
        return [out[oo[c]:oo[c + 1]].copy() for c in range(nchr)]

    def allgather_host(self, arr):
        """canvas_allgather_host: a small numpy array from every rank -> array of shape (ranks,) + arr.shape"""
        a = np.ascontiguousarray(arr)
        out = np.zeros((self.comm_size,) + a.shape, a.dtype)
        self._check(self.lib.canvas_allgather_host(self.ctx, _np_ptr(a), C.c_int64(a.nbytes), _np_ptr(out)))
        return out

    def merge_cleaned_sharded(self, bins, n):
        """canvas_merge_cleaned_sharded: this rank's cleaned SoA (dict chr/start/stop/count, n bins) -> (chr, start, stop, this sample's counts, n_out); one sample per rank"""
        torch = self.torch
        cap = int(bins["chr"].numel())
        mk = lambda dt: torch.empty(cap, dtype=dt, device=self.device)
        oc, os_, oe, ov = mk(torch.int32), mk(torch.int32), mk(torch.int32), mk(torch.float32)
        k = C.c_int64(0)
        self._check(self.lib.canvas_merge_cleaned_sharded(self.ctx, C.c_int64(int(n)), C.c_void_p(bins["chr"].data_ptr()), C.c_void_p(bins["start"].data_ptr()), C.c_void_p(bins["stop"].data_ptr()),
                                                          C.c_void_p(bins["count"].data_ptr()), C.c_void_p(oc.data_ptr()), C.c_void_p(os_.data_ptr()), C.c_void_p(oe.data_ptr()), C.c_void_p(ov.data_ptr()),
                                                          C.c_int64(cap), C.byref(k)))
        return oc[:k.value], os_[:k.value], oe[:k.value], ov[:k.value], k.value

    def sharded_stats(self):
        out = np.zeros(6, np.int64)
        self._check(self.lib.canvas_sharded_stats(self.ctx, _np_ptr(out)))
        return out

    # ---- CanvasNormalize (ratio path)
    def normalize_reference(self, counts, on_target_idx=None):
        """WeightedAverageReferenceGenerator.Run for several control samples: (weighted counts f64 tensor, weights)"""
        torch = self.torch
        n = int(counts[0].numel())
        ptrs = (C.c_void_p * len(counts))(*[C.c_void_p(c.data_ptr()) for c in counts])
        out = torch.empty(n, dtype=torch.float64, device=self.device); w = np.zeros(len(counts), np.float64)
        self._check(self.lib.canvas_normalize_reference(self.ctx, len(counts), ptrs, C.c_int64(n), C.c_void_p(on_target_idx.data_ptr()) if on_target_idx is not None else None,
                                                        C.c_int64(int(on_target_idx.numel()) if on_target_idx is not None else 0), C.c_void_p(out.data_ptr()), _np_ptr(w)))
        self.synchronize()   # the weighted sum is still in flight on the library's stream
        return out, w

    def normalize_ratio(self, sample, reference, on_target_idx=None, mode=0, min_ref=1.0, max_ref=float("inf"), ploidy=None):
        """LSNorm (mode 0) / Raw (mode 1) ratio + RatiosToCounts: (kept bin indices, ratios, counts, library-size factor)"""
        torch = self.torch
        n = int(sample.numel())
        keep = torch.empty(n, dtype=torch.int32, device=self.device); ratio = torch.empty(n, dtype=torch.float32, device=self.device); count = torch.empty(n, dtype=torch.float32, device=self.device)
        n_out = C.c_int64(0); lsf = C.c_double(0)
        self._check(self.lib.canvas_normalize_ratio(self.ctx, C.c_int64(n), C.c_void_p(sample.data_ptr()), C.c_void_p(reference.data_ptr()),
                                                    C.c_void_p(on_target_idx.data_ptr()) if on_target_idx is not None else None, C.c_int64(int(on_target_idx.numel()) if on_target_idx is not None else 0),
                                                    int(mode), C.c_double(min_ref), C.c_double(max_ref), C.c_void_p(ploidy.data_ptr()) if ploidy is not None else None,
                                                    C.c_void_p(keep.data_ptr()), C.c_void_p(ratio.data_ptr()), C.c_void_p(count.data_ptr()), C.byref(n_out), C.byref(lsf)))
        k = n_out.value
        return keep[:k], ratio[:k], count[:k], lsf.value

    def normalize_best_normal(self, tumor, normals, on_target_idx=None):
        """BestLR2ReferenceGenerator.Run for more than one normal (f64 tensors): (index of the chosen normal, mean squared log ratio per normal,
        ignored bins per normal, how many normals were replayed exactly on the host)"""
        n = int(tumor.numel())
        ptrs = (C.c_void_p * len(normals))(*[C.c_void_p(c.data_ptr()) for c in normals])
        best = C.c_int32(-1); replayed = C.c_int32(0)
        msl = np.zeros(len(normals), np.float64); ign = np.zeros(len(normals), np.int64)
        self._check(self.lib.canvas_normalize_best_normal(self.ctx, C.c_void_p(tumor.data_ptr()), len(normals), ptrs, C.c_int64(n),
                                                          C.c_void_p(on_target_idx.data_ptr()) if on_target_idx is not None else None,
                                                          C.c_int64(int(on_target_idx.numel()) if on_target_idx is not None else 0),
                                                          C.byref(best), _np_ptr(msl), _np_ptr(ign), C.byref(replayed)))
        return best.value, msl, ign, replayed.value

    def normalize_pca_reference(self, sample, mu, axes, min_ref=1.0, max_ref=float("inf")):
        """PCAReferenceGenerator.Run: sample / mu f32 tensors of the model's length, axes = list of f64 tensors (raw, not normalised).
        Returns (reference counts f32 tensor, median ratio, projection sizes) or None when the axes are not orthogonal (the reference throws)."""
        torch = self.torch
        n = int(mu.numel())
        ptrs = (C.c_void_p * len(axes))(*[C.c_void_p(a.data_ptr()) for a in axes])
        out = torch.empty(n, dtype=torch.float32, device=self.device)
        med = C.c_double(0); sizes = np.zeros(len(axes), np.float64); orth = C.c_int32(0)
        self._check(self.lib.canvas_normalize_pca_reference(self.ctx, C.c_int64(n), C.c_void_p(sample.data_ptr()), C.c_void_p(mu.data_ptr()), len(axes), ptrs,
                                                            C.c_double(min_ref), C.c_double(max_ref), C.c_void_p(out.data_ptr()), C.byref(med), _np_ptr(sizes), C.byref(orth)))
        if not orth.value:
            return None
        return out, med.value, sizes

    def wavelets_decisions(self):
        """[long nodes decided from the closed form, undecided -> exact chain, chained for their coefficient, closed form in use] of the last wavelets() call"""
        out = np.zeros(4, np.int64)
        self._check(self.lib.canvas_wavelets_decisions(self.ctx, _np_ptr(out)))
        return [int(v) for v in out]

    def wavelets_stats(self):
        """[tree levels processed, nodes recomputed by the exact chain] of the last wavelets() call"""
        out = np.zeros(2, np.int64)
        self._check(self.lib.canvas_wavelets_stats(self.ctx, _np_ptr(out)))
        return out

    def wavelets_inputs(self, nchr):
        """what the last wavelets() call computed its thresholds and its healing step from (canvas_wavelets_inputs): dict(has_cv, cv, f3 float64[9], and per chromosome
        is_root, median, sigma, keep_above), and paths: which code computed them (f3_device, var_device, median_device, median_from_integers: the bits of *h_paths)"""
        has = C.c_int32(0); cvv = C.c_double(0.0); f3 = np.zeros(9, np.float64); paths = C.c_int32(0)
        root = np.zeros(nchr, np.uint8); med = np.zeros(nchr, np.float64); sig = np.zeros(nchr, np.float64); keep = np.zeros(nchr, np.float64)
        self._check(self.lib.canvas_wavelets_inputs(self.ctx, C.c_int32(nchr), C.byref(has), C.byref(cvv), _np_ptr(f3), _np_ptr(root), _np_ptr(med), _np_ptr(sig), _np_ptr(keep), C.byref(paths)))
        return dict(has_cv=bool(has.value), cv=cvv.value, f3=f3, is_root=root.astype(bool), median=med, sigma=sig, keep_above=keep,
                    paths=dict(f3_device=bool(paths.value & 1), var_device=bool(paths.value & 2), median_device=bool(paths.value & 4), median_from_integers=bool(paths.value & 8)))

    def _wv_probe_cov(self, cov, chr_offset=None):
        """coverage (numpy float64, sent bit for bit) and offsets of the Wavelets probe entries -> (device tensor, int64 offsets)"""
        cov = np.ascontiguousarray(cov)
        if cov.dtype != np.float64 or cov.ndim != 1 or len(cov) < 1:
            raise CanvasError("wavelets probe: a non-empty one-dimensional float64 coverage")
        off = np.ascontiguousarray([0, len(cov)] if chr_offset is None else chr_offset, np.int64)
        if len(off) < 2 or off[0] != 0 or off[-1] != len(cov) or (np.diff(off) < 0).any():
            raise CanvasError("wavelets probe: the offsets start at 0, do not decrease and end at len(cov)")
        dev = self.torch.from_numpy(cov.view(np.int64)).to(self.device)      # (the bits travel as integers: NaN payloads and -0.0 stay as they are)
        self.torch.cuda.synchronize(self.device)      # the library runs on its own stream
        return dev, off

    @staticmethod
    def _wv_rows(a, width, what):
        a = np.ascontiguousarray(a, np.int32)
        if a.ndim != 2 or a.shape[1] != width or len(a) < 1:
            raise CanvasError(f"wavelets probe: {what} is an int32 array of shape (n >= 1, {width})")
        return a

    def wavelets_prefix_probe(self, cov, chr_offset):
        """k_wv_prefix_tiles + k_wv_prefix_apply (canvas_wavelets_prefix_probe) -> (P1 int64[N], P2 int64[N], bad int32[2])"""
        dev, off = self._wv_probe_cov(cov, chr_offset)
        p1 = np.zeros(len(cov), np.int64); p2 = np.zeros(len(cov), np.int64); bad = np.zeros(2, np.int32)
        self._check(self.lib.canvas_wavelets_prefix_probe(self.ctx, C.c_int32(len(off) - 1), C.c_void_p(dev.data_ptr()), _np_ptr(off), _np_ptr(p1), _np_ptr(p2), _np_ptr(bad)))
        return p1, p2, bad

    def wavelets_bound_probe(self, cov, chr_offset, nodes):
        """the closed form T[m] and its error bound B[m] as k_wv_level evaluates them (canvas_wavelets_bound_probe).  nodes: int32 (n, 3) = start, len, chromosome ->
        (list of T arrays, list of B arrays), len - 1 values per node, in units of 100 x"""
        dev, off = self._wv_probe_cov(cov, chr_offset)
        nodes = self._wv_rows(nodes, 3, "nodes")
        total = int(np.maximum(nodes[:, 1].astype(np.int64) - 1, 0).sum())
        t = np.zeros(max(total, 1), np.float64); b = np.zeros(max(total, 1), np.float64)
        self._check(self.lib.canvas_wavelets_bound_probe(self.ctx, C.c_int32(len(off) - 1), C.c_void_p(dev.data_ptr()), _np_ptr(off), C.c_int32(len(nodes)), _np_ptr(nodes), _np_ptr(t), _np_ptr(b)))
        cut = np.cumsum(nodes[:, 1].astype(np.int64) - 1)[:-1]
        return np.split(t[:total], cut), np.split(b[:total], cut)

    def wavelets_level_probe(self, cov, chr_offset, nodes, keep_above, wv_long=64):
        """k_wv_list_init + one k_wv_level (canvas_wavelets_level_probe).  nodes: int32 (n, 4) = start, len, chromosome, level -> dict(status int32[n] (0 undecided, 1 decided and
        zeroed, 2 decided and listed for the exact chain), ind int32[n] (the kernel's own for status 2; for status 1 reconstructed by the entry from the children: canvas_hip.h), next int32 (k, 4), roots int32 (r, 6), counts int32[N], overflow)"""
        dev, off = self._wv_probe_cov(cov, chr_offset)
        nodes = self._wv_rows(nodes, 4, "nodes")
        keep = np.ascontiguousarray(keep_above, np.float64)
        if len(keep) != len(off) - 1:
            raise CanvasError("wavelets_level_probe: one keep_above per chromosome")
        n = len(nodes)
        status = np.zeros(n, np.int32); ind = np.zeros(n, np.int32); nxt = np.zeros((2 * n, 4), np.int32); roots = np.zeros((2 * n, 6), np.int32); counts = np.zeros(len(cov), np.int32)
        nn = C.c_int64(0); nr = C.c_int64(0); ov = C.c_int32(0)
        self._check(self.lib.canvas_wavelets_level_probe(self.ctx, C.c_int32(len(off) - 1), C.c_void_p(dev.data_ptr()), _np_ptr(off), C.c_int32(n), _np_ptr(nodes), _np_ptr(keep), C.c_int32(wv_long),
                                                         _np_ptr(status), _np_ptr(ind), _np_ptr(nxt), C.byref(nn), _np_ptr(roots), C.byref(nr), _np_ptr(counts), C.byref(ov)))
        return dict(status=status, ind=ind, next=nxt[:nn.value].copy(), roots=roots[:nr.value].copy(), counts=counts, overflow=ov.value)

    def wavelets_chain_probe(self, cov, nodes, lim=None, fast=True, own_slices=False):
        """k_wv_coeff, k_wv_chain_long, k_wv_chunks, k_wv_reduce (canvas_wavelets_chain_probe).  nodes: int32 (n, 2) = start, len; lim: int32[n] or None ->
        (coef float64[n], ind int32[n], flag int32[n])"""
        dev, _ = self._wv_probe_cov(cov)
        nodes = self._wv_rows(nodes, 2, "nodes")
        n = len(nodes)
        if lim is not None:
            lim = np.ascontiguousarray(lim, np.int32)
            if lim.shape != (n,):
                raise CanvasError("wavelets_chain_probe: one lim per node")
        coef = np.zeros(n, np.float64); ind = np.zeros(n, np.int32); flag = np.zeros(n, np.int32)
        self._check(self.lib.canvas_wavelets_chain_probe(self.ctx, C.c_int64(len(cov)), C.c_void_p(dev.data_ptr()), C.c_int32(n), _np_ptr(nodes), None if lim is None else _np_ptr(lim),
                                                         C.c_int32(int(bool(fast))), C.c_int32(int(bool(own_slices))), _np_ptr(coef), _np_ptr(ind), _np_ptr(flag)))
        return coef, ind, flag

    def wavelets_subtree_probe(self, cov, chr_offset, roots, keep_above, cap_cand, wv_long=64, use_table=True):
        """k_wv_fgh_table + k_wv_subtree (canvas_wavelets_subtree_probe).  roots: int32 (n, 6) = start, len, chromosome, level, s1, cbase -> dict(counts int32[N], cand int32 (k, 5) =
        chromosome, level, s, b, e, coef float64[k], ncand (found; k = min(ncand, cap_cand) were written), overflow)"""
        dev, off = self._wv_probe_cov(cov, chr_offset)
        roots = self._wv_rows(roots, 6, "roots")
        keep = np.ascontiguousarray(keep_above, np.float64)
        if len(keep) != len(off) - 1:
            raise CanvasError("wavelets_subtree_probe: one keep_above per chromosome")
        cap = int(cap_cand)
        counts = np.zeros(len(cov), np.int32); cand = np.zeros((max(cap, 1), 5), np.int32); coef = np.zeros(max(cap, 1), np.float64)
        nc = C.c_int64(0); ov = C.c_int32(0)
        self._check(self.lib.canvas_wavelets_subtree_probe(self.ctx, C.c_int32(len(off) - 1), C.c_void_p(dev.data_ptr()), _np_ptr(off), C.c_int32(len(roots)), _np_ptr(roots), _np_ptr(keep), C.c_int64(cap),
                                                           C.c_int32(wv_long), C.c_int32(int(bool(use_table))), _np_ptr(counts), _np_ptr(cand), _np_ptr(coef), C.byref(nc), C.byref(ov)))
        k = min(nc.value, max(cap, 0))
        return dict(counts=counts, cand=cand[:k].copy(), coef=coef[:k].copy(), ncand=nc.value, overflow=ov.value)

    def wavelets_median_probe(self, cov, start, length, per_workgroup=False):
        """medians of up to 1024 stretches through k_wv_prefix_tiles + three k_wv_rmed_pass launches (canvas_wavelets_median_probe) -> (median float64[n], the same through
        k_wv_segment_median or None, bad int32[2])"""
        dev, _ = self._wv_probe_cov(cov)
        st = np.ascontiguousarray(start, np.int64); ln = np.ascontiguousarray(length, np.int64)
        if st.ndim != 1 or st.shape != ln.shape:
            raise CanvasError("wavelets_median_probe: one (start, length) per stretch")
        med = np.zeros(max(len(st), 1), np.float64); wg = np.zeros(max(len(st), 1), np.float64) if per_workgroup else None; bad = np.zeros(2, np.int32)
        self._check(self.lib.canvas_wavelets_median_probe(self.ctx, C.c_int64(len(cov)), C.c_void_p(dev.data_ptr()), C.c_int32(len(st)), _np_ptr(st), _np_ptr(ln), _np_ptr(med),
                                                          None if wg is None else _np_ptr(wg), _np_ptr(bad)))
        return med[:len(st)], (None if wg is None else wg[:len(st)]), bad


# ---- synthetic generator (bench/test tooling, separate library)
_synth = None


def synth_generate_sample_device(seed, hit_seed, chrom, length, thr_dev, device, with_fraglen=False, bases=None, mask=None):
    """a further sample over the reference of `seed` (tumour / normal pairs): (hits, fraglen or None); mirrors synth.generate_chromosome(hit_seed=...).
    bases / mask tensors are (re)written when given."""
    import torch
    from . import synth
    global _synth
    if _synth is None:
        load_library()
        if not os.path.exists(_SYNTH_SO):
            raise CanvasError(f"{_SYNTH_SO} missing: run build()")
        _synth = C.CDLL(_SYNTH_SO)
    gap0, g1s, g1e, base_cn = synth.chrom_params(chrom, length)
    pad = (length + 63) // 64 * 64
    hits = torch.zeros(pad, dtype=torch.uint8, device=device)
    fl = torch.zeros(pad, dtype=torch.int16, device=device) if with_fraglen else None
    rc = _synth.synth_generate_sample(C.c_uint32(seed), C.c_uint32(hit_seed), C.c_uint32(chrom), C.c_int64(length), C.c_int64(gap0), C.c_int64(g1s), C.c_int64(g1e), C.c_uint32(base_cn),
                                      C.c_void_p(thr_dev.data_ptr()), C.c_void_p(bases.data_ptr()) if bases is not None else None, C.c_void_p(hits.data_ptr()),
                                      C.c_void_p(mask.data_ptr()) if mask is not None else None, C.c_void_p(fl.data_ptr()) if fl is not None else None,
                                      C.c_void_p(torch.cuda.current_stream(device).cuda_stream))
    if rc != 0:
        raise CanvasError(f"synth_generate_sample failed: hip error {rc}")
    return hits, fl


def synth_generate_device(seed, chrom, length, rate, device, thr_dev=None):
    """generate (bases, hits, mask) for one chromosome directly in HBM; mirrors canvas_amd.synth.generate_chromosome"""
    import torch
    from . import synth
    global _synth
    if _synth is None:
        load_library()
        if not os.path.exists(_SYNTH_SO):
            raise CanvasError(f"{_SYNTH_SO} missing: run build()")
        _synth = C.CDLL(_SYNTH_SO)
    if thr_dev is None:
        thr_dev = torch.from_numpy(synth.poisson_thresholds(rate).view(np.int32)).to(device)
    gap0, g1s, g1e, base_cn = synth.chrom_params(chrom, length)
    pad = (length + 63) // 64 * 64
    bases = torch.empty(pad, dtype=torch.uint8, device=device)
    hits = torch.empty(pad, dtype=torch.uint8, device=device)
    mask = torch.empty(pad // 64, dtype=torch.int64, device=device)
    rc = _synth.synth_generate(C.c_uint32(seed), C.c_uint32(chrom), C.c_int64(length), C.c_int64(gap0), C.c_int64(g1s), C.c_int64(g1e), C.c_uint32(base_cn),
                               C.c_void_p(thr_dev.data_ptr()), C.c_void_p(bases.data_ptr()), C.c_void_p(hits.data_ptr()), C.c_void_p(mask.data_ptr()),
                               C.c_void_p(torch.cuda.current_stream(device).cuda_stream))
    if rc != 0:
        raise CanvasError(f"synth_generate failed: hip error {rc}")
    return bases, hits, mask, thr_dev
