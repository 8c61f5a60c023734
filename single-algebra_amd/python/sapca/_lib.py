"""ctypes binding of libsapca.so (include/sapca.h).  No fallbacks: if the HIP library is
missing or there is no GPU, calls fail loudly."""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# SAPCA_LIB_PATH points at another build of the same library (kernel experiments, tools/abl_build.sh)
LIB_PATH = os.environ.get("SAPCA_LIB_PATH") or os.path.normpath(os.path.join(_HERE, "..", "..", "lib", "libsapca.so"))
# the variant that reads the SAPCA_* experiment / route switches (csrc/switches.h; the release library reads none of them)
DEBUG_LIB_PATH = os.path.normpath(os.path.join(_HERE, "..", "..", "lib", "libsapca_dbg.so"))

OK, ERR_ARG, ERR_MASK_LEN, ERR_NOT_FITTED, ERR_SVD, ERR_HIP, ERR_COMM, ERR_NOMEM = range(8)
LANCZOS, RANDOM = 0, 1
NORM_QR, NORM_LU, NORM_NONE = 0, 1, 2
TRANSFORM_REFERENCE, TRANSFORM_CENTERED = 0, 1


class Options(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("random_seed", C.c_uint32), ("n_components", C.c_uint64),
        ("alpha", C.c_double), ("tolerance", C.c_double),
        ("center", C.c_uint8), ("verbose", C.c_uint8), ("collect_timings", C.c_uint8), ("lanczos_center", C.c_uint8),
        ("method", C.c_int32), ("n_oversamples", C.c_uint64), ("n_power_iterations", C.c_uint64),
        ("normalizer", C.c_int32), ("transform_semantics", C.c_int32), ("device_id", C.c_int32),
        ("spmm_variant", C.c_int32), ("stream", C.c_void_p),
    ]


class Timings(C.Structure):
    _fields_ = [
        ("upload_ms", C.c_double), ("prepare_ms", C.c_double), ("stats_ms", C.c_double),
        ("spmm_ms", C.c_double), ("spmmt_ms", C.c_double), ("ortho_ms", C.c_double),
        ("small_svd_ms", C.c_double), ("lanczos_ms", C.c_double), ("transform_ms", C.c_double),
        ("comm_ms", C.c_double), ("fit_total_ms", C.c_double),
        ("n_spmm", C.c_uint32), ("n_spmmt", C.c_uint32),
        ("spmm_sweep_ms", C.c_double * 32), ("spmmt_sweep_ms", C.c_double * 32),
        ("bytes_per_sweep", C.c_double), ("lanczos_steps", C.c_uint64),
        ("sweep_kernel", C.c_uint32), ("at_sweep_pieces", C.c_uint32), ("sweep_slots_a", C.c_uint64), ("sweep_slots_at", C.c_uint64),
    ]


class TsneOptions(C.Structure):
    """sapca_tsne_options"""
    _fields_ = [
        ("struct_size", C.c_uint32), ("random_seed", C.c_uint32), ("output_dim", C.c_uint32), ("init_given", C.c_uint32),
        ("perplexity", C.c_double), ("theta", C.c_double), ("epochs", C.c_uint64),
        ("stop_lying_epoch", C.c_uint64), ("momentum_switch_epoch", C.c_uint64),
        ("exaggeration", C.c_double), ("learning_rate", C.c_double), ("momentum", C.c_double), ("final_momentum", C.c_double),
    ]


class KmeansOptions(C.Structure):
    """sapca_kmeans_options"""
    _fields_ = [
        ("struct_size", C.c_uint32), ("random_seed", C.c_uint32), ("n_clusters", C.c_uint32), ("init", C.c_uint32),
        ("max_iter", C.c_uint64), ("tol", C.c_double),
    ]


class LouvainOptions(C.Structure):
    """sapca_louvain_options"""
    _fields_ = [
        ("struct_size", C.c_uint32), ("random_seed", C.c_uint32), ("max_levels", C.c_uint32), ("max_sweeps", C.c_uint32),
        ("resolution", C.c_double), ("tol", C.c_double),
    ]


class SpectralOptions(C.Structure):
    """sapca_spectral_options"""
    _fields_ = [
        ("struct_size", C.c_uint32), ("random_seed", C.c_uint32), ("kind", C.c_uint32), ("n_eigen", C.c_uint32),
        ("max_steps", C.c_uint32), ("reserved", C.c_uint32), ("tol", C.c_double),
    ]


# sapca_spectral_kind
SPECTRAL_NORMALIZED, SPECTRAL_DIFFMAP = 0, 1
SPECTRAL_KINDS = {"normalized": SPECTRAL_NORMALIZED, "diffmap": SPECTRAL_DIFFMAP}


class HvgOptions(C.Structure):
    """sapca_hvg_options"""
    _fields_ = [
        ("struct_size", C.c_uint32), ("flavor", C.c_int32), ("n_top", C.c_uint64), ("span", C.c_double),
        ("n_bins", C.c_uint32), ("reserved", C.c_uint32),
        ("min_mean", C.c_double), ("max_mean", C.c_double), ("min_disp", C.c_double), ("max_disp", C.c_double),
    ]


class UmapOptions(C.Structure):
    """sapca_umap_options"""
    _fields_ = [
        ("struct_size", C.c_uint32), ("random_seed", C.c_uint32), ("output_dim", C.c_uint32), ("init", C.c_uint32),
        ("n_neighbors", C.c_uint32), ("negative_sample_rate", C.c_uint32), ("epochs", C.c_uint64),
        ("min_dist", C.c_double), ("spread", C.c_double), ("a", C.c_double), ("b", C.c_double),
        ("learning_rate", C.c_double), ("repulsion_strength", C.c_double),
    ]


# sapca_csr_report and its flags (sapca_check_csr_device_*, sapca_canonicalize_csr_device_*)
CSR_BAD_OFFSETS, CSR_COL_RANGE, CSR_UNSORTED, CSR_DUPLICATES, CSR_NONFINITE = 1, 2, 4, 8, 16
CSR_FLAG_NAMES = {CSR_BAD_OFFSETS: "BAD_OFFSETS", CSR_COL_RANGE: "COL_RANGE", CSR_UNSORTED: "UNSORTED",
                  CSR_DUPLICATES: "DUPLICATES", CSR_NONFINITE: "NONFINITE"}


# flags of sapca_select_submatrix_csr_device_*
SELECT_DROP_STORED_ZEROS = 1
# sapca_knn_device_*: metrics, flags, the longest list
KNN_EUCLIDEAN, KNN_COSINE, KNN_PEARSON = 0, 1, 2
KNN_METRICS = {"euclidean": KNN_EUCLIDEAN, "cosine": KNN_COSINE, "pearson": KNN_PEARSON}
KNN_EXCLUDE_SELF = 1
KNN_MAX_NEIGHBORS = 128
RANK_MAX_GROUPS = 1024   # SAPCA_RANK_MAX_GROUPS
# sapca_hvg_*: the most batches, the transforms of the moments, the flavours
HVG_MAX_BATCHES = 1024
HVG_CLIP, HVG_EXPM1 = 0, 1
HVG_TRANSFORMS = {"clip": HVG_CLIP, "expm1": HVG_EXPM1}
HVG_SEURAT_V3, HVG_SEURAT = 0, 1
HVG_FLAVORS = {"seurat_v3": HVG_SEURAT_V3, "seurat": HVG_SEURAT}
# sapca_kmeans_*: the seeding rules, the most clusters
KMEANS_PLUSPLUS, KMEANS_GIVEN = 0, 1
KMEANS_MAX_CLUSTERS = 1024
# sapca_umap_*: how the layout starts
UMAP_INIT_PANEL, UMAP_INIT_RANDOM, UMAP_INIT_GIVEN = 0, 1, 2
UMAP_INITS = {"panel": UMAP_INIT_PANEL, "random": UMAP_INIT_RANDOM}
# covariate columns + the intercept that center = 1 adds (sapca_set_covariates)
MAX_DESIGN_COLUMNS = 16
# sapca_column_scaling (sapca_set_column_scaling)
SCALE_NONE, SCALE_UNIT_VARIANCE, SCALE_WEIGHTS = 0, 1, 2


class CsrReport(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("flags", C.c_uint32),
        ("first_bad_offset_row", C.c_uint64), ("cols_out_of_range", C.c_uint64), ("first_out_of_range_row", C.c_uint64),
        ("unsorted_rows", C.c_uint64), ("first_unsorted_row", C.c_uint64),
        ("duplicate_entries", C.c_uint64), ("first_duplicate_row", C.c_uint64),
        ("nonfinite_values", C.c_uint64), ("first_nonfinite_row", C.c_uint64),
        ("stored_zeros", C.c_uint64),
    ]


ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int32, C.c_void_p)

# every symbol include/sapca.h declares (the CPU test checks the library exports each one)
_TYPED = [
    "sapca_set_omega", "sapca_fit_csr", "sapca_transform_csr", "sapca_fit_transform_csr",
    "sapca_fit_csr_device", "sapca_transform_csr_device", "sapca_fit_transform_csr_device",
    "sapca_transform_csr_device_to_host", "sapca_fit_transform_csr_device_to_host",
    "sapca_get_components", "sapca_get_singular_values", "sapca_get_explained_variance", "sapca_get_mean",
    "sapca_get_explained_variance_ratio", "sapca_get_cumulative_explained_variance_ratio",
    "sapca_get_feature_importances", "sapca_colstats_csr", "sapca_spmm_csr", "sapca_spmmt_csr",
    "sapca_normalize_panel", "sapca_generate_omega", "sapca_project_out_panel", "sapca_scale_panel_rows",
    "sapca_normalize_panel_ex", "sapca_rotate_panel",
    "sapca_upload_csr", "sapca_normalize_csr_device", "sapca_log1p_csr_device", "sapca_stats_csr_device",
    "sapca_batch_stats_csr_device", "sapca_sum_row_n_top_csr_device", "sapca_masked_stats_csr_device",
    "sapca_select_rows_csr_device", "sapca_check_csr_device", "sapca_canonicalize_csr_device",
    "sapca_select_submatrix_csr_device", "sapca_knn_device",
    "sapca_tsne_affinities_device", "sapca_tsne_gradient_device", "sapca_tsne_embed_device", "sapca_tsne_device", "sapca_tsne",
    "sapca_kmeans_seed_device", "sapca_kmeans_assign_device", "sapca_kmeans_update_device", "sapca_kmeans_device", "sapca_kmeans",
    "sapca_umap_graph_device", "sapca_umap_embed_device", "sapca_umap_device", "sapca_umap",
    "sapca_louvain_modularity_device", "sapca_louvain_sweep_device", "sapca_louvain_aggregate_device", "sapca_louvain_device",
    "sapca_louvain", "sapca_rank_sums_csr_device", "sapca_rank_groups_csr_device",
    "sapca_hvg_moments_csr_device", "sapca_hvg_csr_device",
    "sapca_spectral_scale_device", "sapca_spectral_apply_device", "sapca_spectral_device", "sapca_spectral",
    "sapca_umap_spectral_init_device",
    "sapca_multi_fit_csr", "sapca_multi_transform_csr", "sapca_multi_fit_transform_csr",
    "sapca_multi_upload_csr", "sapca_multi_transform_resident", "sapca_multi_fit_transform_resident",
]
_PLAIN = [
    "sapca_options_default", "sapca_abi_version", "sapca_create", "sapca_destroy", "sapca_last_error",
    "sapca_set_mask", "sapca_get_dims", "sapca_get_total_variance", "sapca_get_mask_index_maps",
    "sapca_get_timings", "sapca_partition_rows", "sapca_comm_unique_id", "sapca_comm_rccl_available", "sapca_comm_init_rank",
    "sapca_comm_set_callback", "sapca_comm_allreduce", "sapca_comm_abort", "sapca_comm_async_error", "sapca_comm_has_side_lane",
    "sapca_upload_values_changed", "sapca_measure_copy_gbs", "sapca_multi_fit_resident", "sapca_multi_resident_shard",
    "sapca_multi_create", "sapca_multi_destroy", "sapca_multi_last_error", "sapca_multi_n_devices", "sapca_multi_member",
    "sapca_multi_uses_rccl", "sapca_multi_set_mask",
    "sapca_covariate_basis", "sapca_set_covariates", "sapca_get_covariate_rank",
    "sapca_set_column_scaling", "sapca_get_column_scale",
    "sapca_tsne_options_default", "sapca_kmeans_options_default",
    "sapca_umap_options_default", "sapca_umap_find_ab", "sapca_louvain_options_default",
    "sapca_hvg_options_default", "sapca_loess_f64",
    "sapca_spectral_options_default", "sapca_graph_components_device",
]
EXPORTED_SYMBOLS = _PLAIN + [f"{n}_{s}" for n in _TYPED for s in ("f32", "f64")]

_lib = None


class SapcaError(RuntimeError):
    def __init__(self, status, message):
        super().__init__(message)
        self.status = status


def load():
    """dlopen libsapca.so.  torch (if it is going to be used at all) must be imported first so the
    process shares ONE HIP runtime / RCCL: bench.py and the tests import torch at the top."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH) and not os.environ.get("SAPCA_NO_AUTOBUILD"):
        # building the product is not a fallback: same sources, same gfx950 target
        import shutil
        import subprocess
        if shutil.which("make") and (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
            subprocess.call(["make", "-C", os.path.normpath(os.path.join(_HERE, "..", "..")), "-j", "8"])
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `make -C single-algebra_amd` "
            "(or python -c 'import __graft_entry__ as g; g.build()'). There is no CPU fallback.")
    _lib = _open(LIB_PATH)
    return _lib


_debug_lib = None


def load_debug():
    """The -DSAPCA_DEBUG_SWITCHES build of the same sources (make debug): for tests and tools that steer routes through
    SAPCA_* environment variables.  A second library instance beside the release one (its own handles: objects do not cross)."""
    global _debug_lib
    if _debug_lib is None:
        if not os.path.exists(DEBUG_LIB_PATH):
            raise ImportError(f"{DEBUG_LIB_PATH} is missing: build it with `make -C single-algebra_amd debug`")
        _debug_lib = _open(DEBUG_LIB_PATH)
    return _debug_lib


def _open(path):
    lib = C.CDLL(path)
    lib.sapca_last_error.restype = C.c_char_p
    lib.sapca_last_error.argtypes = [C.c_void_p]
    lib.sapca_create.argtypes = [C.POINTER(Options), C.POINTER(C.c_void_p)]
    lib.sapca_destroy.argtypes = [C.c_void_p]
    lib.sapca_destroy.restype = None
    lib.sapca_options_default.argtypes = [C.POINTER(Options)]
    lib.sapca_options_default.restype = None
    lib.sapca_multi_create.argtypes = [C.POINTER(Options), C.POINTER(C.c_int32), C.c_uint32, C.POINTER(C.c_void_p)]
    lib.sapca_multi_destroy.argtypes = [C.c_void_p]
    lib.sapca_multi_destroy.restype = None
    lib.sapca_multi_last_error.argtypes = [C.c_void_p]
    lib.sapca_multi_last_error.restype = C.c_char_p
    lib.sapca_multi_member.argtypes = [C.c_void_p, C.c_uint32]
    lib.sapca_multi_member.restype = C.c_void_p
    lib.sapca_multi_n_devices.argtypes = [C.c_void_p]
    lib.sapca_multi_n_devices.restype = C.c_uint32
    lib.sapca_multi_uses_rccl.argtypes = [C.c_void_p]
    if hasattr(lib, "sapca_comm_abort"):   # (ABI 4; an older build loaded through SAPCA_LIB_PATH for an A/B run lacks them)
        lib.sapca_multi_fit_resident.argtypes = [C.c_void_p]
        lib.sapca_comm_abort.argtypes = [C.c_void_p]
        lib.sapca_comm_async_error.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
        lib.sapca_comm_has_side_lane.argtypes = [C.c_void_p]
    if hasattr(lib, "sapca_measure_copy_gbs"):
        lib.sapca_measure_copy_gbs.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.POINTER(C.c_double)]
    if hasattr(lib, "sapca_set_covariates"):   # (absent from an older build loaded for an A/B run)
        lib.sapca_covariate_basis.argtypes = [C.POINTER(C.c_double), C.c_uint64, C.c_uint64, C.c_int32, C.POINTER(C.c_double),
                                              C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
        lib.sapca_set_covariates.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.c_uint64, C.c_uint64]
        lib.sapca_get_covariate_rank.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        for suf, ct in (("f32", C.c_float), ("f64", C.c_double)):
            getattr(lib, f"sapca_project_out_panel_{suf}").argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(ct), C.c_uint32,
                                                                       C.POINTER(ct)]
    if hasattr(lib, "sapca_set_column_scaling"):   # (absent from an older build loaded for an A/B run)
        lib.sapca_set_column_scaling.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_double), C.c_uint64]
        lib.sapca_get_column_scale.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_double), C.c_size_t]
        for suf, ct in (("f32", C.c_float), ("f64", C.c_double)):
            getattr(lib, f"sapca_scale_panel_rows_{suf}").argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(ct),
                                                                      C.POINTER(C.c_double)]
    if hasattr(lib, "sapca_rotate_panel_f32"):   # (absent from an older build loaded for an A/B run)
        for suf, ct in (("f32", C.c_float), ("f64", C.c_double)):
            pt, pd = C.POINTER(ct), C.POINTER(C.c_double)
            getattr(lib, f"sapca_normalize_panel_ex_{suf}").argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_uint64, C.c_uint64,
                                                                        C.c_uint32, pt, pt, pt, pt, pt, pt, pd, pd,
                                                                        C.POINTER(C.c_int32)]
            getattr(lib, f"sapca_rotate_panel_{suf}").argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, pt, pd, pt, pd]
    for suf, ct in (("f32", C.c_float), ("f64", C.c_double)):
        fn = getattr(lib, f"sapca_select_submatrix_csr_device_{suf}", None)   # (absent from an older build loaded for an A/B run)
        if fn is not None:
            fn.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                           C.POINTER(C.c_uint64), C.c_uint64, C.POINTER(C.c_uint8), C.c_uint64, C.c_uint32,
                           C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                           C.POINTER(C.c_void_p)]
    for suf in ("f32", "f64"):
        fn = getattr(lib, f"sapca_knn_device_{suf}", None)   # (absent from an older build loaded for an A/B run)
        if fn is not None:
            fn.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint64,
                           C.c_int32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    if hasattr(lib, "sapca_tsne_options_default"):   # (absent from an older build loaded for an A/B run)
        lib.sapca_tsne_options_default.argtypes = [C.POINTER(TsneOptions)]
        lib.sapca_tsne_options_default.restype = None
        csr = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]   # h, m, nnz, offsets, columns, values
        for suf in ("f32", "f64"):
            getattr(lib, f"sapca_tsne_affinities_device_{suf}").argtypes = [
                C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32, C.c_double, C.POINTER(C.c_uint64),
                C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_void_p]
            getattr(lib, f"sapca_tsne_gradient_device_{suf}").argtypes = csr + [
                C.c_void_p, C.c_uint64, C.c_uint32, C.c_double, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)]
            getattr(lib, f"sapca_tsne_embed_device_{suf}").argtypes = csr + [C.POINTER(TsneOptions), C.c_void_p, C.POINTER(C.c_double)]
            getattr(lib, f"sapca_tsne_device_{suf}").argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint64,
                                                                 C.POINTER(TsneOptions), C.c_void_p, C.POINTER(C.c_double)]
            getattr(lib, f"sapca_tsne_{suf}").argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.POINTER(TsneOptions),
                                                          C.c_void_p, C.POINTER(C.c_double)]
    if hasattr(lib, "sapca_kmeans_options_default"):   # (absent from an older build loaded for an A/B run)
        lib.sapca_kmeans_options_default.argtypes = [C.POINTER(KmeansOptions)]
        lib.sapca_kmeans_options_default.restype = None
        panel = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint64]   # h, m, d_x, ldx, d
        for suf in ("f32", "f64"):
            getattr(lib, f"sapca_kmeans_seed_device_{suf}").argtypes = panel + [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
            getattr(lib, f"sapca_kmeans_assign_device_{suf}").argtypes = panel + [
                C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
            getattr(lib, f"sapca_kmeans_update_device_{suf}").argtypes = panel + [C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
            getattr(lib, f"sapca_kmeans_device_{suf}").argtypes = panel + [
                C.POINTER(KmeansOptions), C.c_void_p, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
            getattr(lib, f"sapca_kmeans_{suf}").argtypes = [
                C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.POINTER(KmeansOptions), C.c_void_p, C.c_void_p,
                C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
    if hasattr(lib, "sapca_umap_options_default"):   # (absent from an older build loaded for an A/B run)
        lib.sapca_umap_options_default.argtypes = [C.POINTER(UmapOptions)]
        lib.sapca_umap_options_default.restype = None
        lib.sapca_umap_find_ab.argtypes = [C.c_double, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double)]
        csr = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]   # h, m, nnz, offsets, columns, values
        for suf in ("f32", "f64"):
            getattr(lib, f"sapca_umap_graph_device_{suf}").argtypes = [
                C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64),
                C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p]
            getattr(lib, f"sapca_umap_embed_device_{suf}").argtypes = csr + [C.POINTER(UmapOptions), C.c_void_p]
            getattr(lib, f"sapca_umap_device_{suf}").argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint64,
                                                                 C.POINTER(UmapOptions), C.c_void_p]
            getattr(lib, f"sapca_umap_{suf}").argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.POINTER(UmapOptions),
                                                          C.c_void_p]
    if hasattr(lib, "sapca_louvain_options_default"):   # (absent from an older build loaded for an A/B run)
        lib.sapca_louvain_options_default.argtypes = [C.POINTER(LouvainOptions)]
        lib.sapca_louvain_options_default.restype = None
        csr = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]   # h, m, nnz, offsets, columns, values
        for suf in ("f32", "f64"):
            getattr(lib, f"sapca_louvain_modularity_device_{suf}").argtypes = csr + [C.c_void_p, C.c_double, C.POINTER(C.c_double)]
            getattr(lib, f"sapca_louvain_sweep_device_{suf}").argtypes = csr + [
                C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_double, C.c_void_p, C.POINTER(C.c_uint64)]
            getattr(lib, f"sapca_louvain_aggregate_device_{suf}").argtypes = csr + [
                C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                C.POINTER(C.c_void_p), C.c_void_p]
            for name in (f"sapca_louvain_device_{suf}", f"sapca_louvain_{suf}"):
                getattr(lib, name).argtypes = csr + [C.POINTER(LouvainOptions), C.c_void_p, C.POINTER(C.c_uint64),
                                                     C.POINTER(C.c_double), C.POINTER(C.c_uint32)]
    if hasattr(lib, "sapca_rank_sums_csr_device_f32"):   # (absent from an older build loaded for an A/B run)
        mat = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]   # h, m, n, nnz, offsets, columns, values
        u64p, f64p = C.POINTER(C.c_uint64), C.POINTER(C.c_double)
        for suf in ("f32", "f64"):
            getattr(lib, f"sapca_rank_sums_csr_device_{suf}").argtypes = mat + [C.c_void_p, C.c_uint32, u64p, C.POINTER(C.c_int64), u64p, f64p]
            getattr(lib, f"sapca_rank_groups_csr_device_{suf}").argtypes = mat + [C.c_void_p, C.c_uint32, C.c_int32, u64p, f64p, f64p, u64p,
                                                                                  f64p, f64p, f64p, f64p]
    if hasattr(lib, "sapca_hvg_options_default"):   # (absent from an older build loaded for an A/B run)
        lib.sapca_hvg_options_default.argtypes = [C.POINTER(HvgOptions)]
        lib.sapca_hvg_options_default.restype = None
        mat = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]   # h, m, n, nnz, offsets, columns, values
        u64p, f64p = C.POINTER(C.c_uint64), C.POINTER(C.c_double)
        lib.sapca_loess_f64.argtypes = [C.c_void_p, C.c_uint64, f64p, f64p, C.c_double, f64p]
        for suf in ("f32", "f64"):
            getattr(lib, f"sapca_hvg_moments_csr_device_{suf}").argtypes = mat + [C.c_void_p, C.c_int32, C.c_int32, f64p, f64p, f64p, u64p]
            getattr(lib, f"sapca_hvg_csr_device_{suf}").argtypes = mat + [C.c_void_p, C.c_uint32, C.POINTER(HvgOptions), f64p, f64p, f64p,
                                                                          f64p, f64p, f64p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint8)]
    if hasattr(lib, "sapca_spectral_options_default"):   # (absent from an older build loaded for an A/B run)
        lib.sapca_spectral_options_default.argtypes = [C.POINTER(SpectralOptions)]
        lib.sapca_spectral_options_default.restype = None
        lib.sapca_graph_components_device.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                                                      C.POINTER(C.c_uint64)]
        csr = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]   # h, m, nnz, offsets, columns, values
        for suf in ("f32", "f64"):
            getattr(lib, f"sapca_spectral_scale_device_{suf}").argtypes = csr + [C.c_uint32, C.c_void_p]
            getattr(lib, f"sapca_spectral_apply_device_{suf}").argtypes = csr + [C.c_uint32, C.c_void_p, C.c_void_p]
            for name in (f"sapca_spectral_device_{suf}", f"sapca_spectral_{suf}"):
                getattr(lib, name).argtypes = csr + [C.POINTER(SpectralOptions), C.POINTER(C.c_double), C.c_void_p,
                                                     C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]
            getattr(lib, f"sapca_umap_spectral_init_device_{suf}").argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint64,
                                                                               C.c_uint32, C.c_uint32, C.c_void_p]
    return lib


def default_spectral_options() -> SpectralOptions:
    o = SpectralOptions()
    load().sapca_spectral_options_default(C.byref(o))
    return o


def default_hvg_options() -> HvgOptions:
    o = HvgOptions()
    load().sapca_hvg_options_default(C.byref(o))
    return o


def default_louvain_options() -> LouvainOptions:
    o = LouvainOptions()
    load().sapca_louvain_options_default(C.byref(o))
    return o


def default_umap_options() -> UmapOptions:
    o = UmapOptions()
    load().sapca_umap_options_default(C.byref(o))
    return o


def find_ab_params(spread=1.0, min_dist=0.1):
    """sapca_umap_find_ab: (a, b) of the curve 1 / (1 + a x^(2b)) fitted to (spread, min_dist) as umap-learn's find_ab_params
    does.  Pure host code, no device.  Bad arguments raise SapcaError (ERR_ARG), a fit that does not converge ERR_SVD."""
    a, b = C.c_double(), C.c_double()
    st = load().sapca_umap_find_ab(C.c_double(float(spread)), C.c_double(float(min_dist)), C.byref(a), C.byref(b))
    if st != OK:
        raise SapcaError(st, f"sapca_umap_find_ab(spread={spread}, min_dist={min_dist}): "
                         + ("the fit did not converge in 200 steps" if st == 4 else
                            "spread must be finite and positive, min_dist finite, not negative and below 3 spread"))
    return a.value, b.value


def default_kmeans_options() -> KmeansOptions:
    o = KmeansOptions()
    load().sapca_kmeans_options_default(C.byref(o))
    return o


def default_tsne_options() -> TsneOptions:
    o = TsneOptions()
    load().sapca_tsne_options_default(C.byref(o))
    return o


def default_options() -> Options:
    o = Options()
    load().sapca_options_default(C.byref(o))
    return o


def check(handle, status):
    if status != OK:
        msg = load().sapca_last_error(handle)
        raise SapcaError(status, (msg or b"").decode() or f"sapca status {status}")


def as_u64(a):
    """A CSR offset / index array in the library's u64 (nalgebra_sparse `usize`) layout: int64 arrays -- what scipy holds for
    large matrices -- are reinterpreted in place (a negative entry reads as an index the library refuses), anything else
    is converted (a copy)."""
    import numpy as np
    a = np.asarray(a)
    if a.dtype == np.uint64 and a.flags.c_contiguous:
        return a
    if a.dtype == np.int64 and a.flags.c_contiguous:
        return a.view(np.uint64)
    return np.ascontiguousarray(a, dtype=np.uint64)
