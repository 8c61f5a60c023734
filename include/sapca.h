/*
 * sapca.h -- C ABI of the MI355X-native sparse-PCA hot path (libsapca.so).
 *
 * Drop-in boundary for single-algebra's src/dimred/pca (reference v0.9.2).  The
 * reference has no FFI of its own: its boundary is the Rust generic API
 * (SparsePCABuilder / MaskedSparsePCABuilder / fit / transform / fit_transform)
 * and, one level down, the single-svdlib calls it makes.  Every entry point below
 * names the reference interface it replaces (paths relative to the reference
 * repository root); INTEGRATION.md shows the Rust `extern "C"` binding.
 *
 * Conventions
 *   - plain pointers and sizes only; no C++/torch/HIP types in signatures
 *     (a HIP stream is passed as void*).
 *   - every function returns a sapca_status; nothing throws or aborts across the
 *     ABI.  sapca_last_error(h) gives the message (the reference's anyhow text
 *     where one exists).
 *   - _f32/_f64 pairs mirror the reference's generic T (f32/f64 in practice).
 *   - host CSR inputs use nalgebra_sparse::CsrMatrix's own layout: row_offsets
 *     and col_indices are usize (uint64_t), zero-copy from Rust.  The host entry
 *     points check what keeps every kernel inside the arrays (offsets start at 0,
 *     end at nnz and never decrease; columns < n) and return SAPCA_ERR_ARG otherwise;
 *     columns sorted and unique within a row is CsrMatrix's own invariant and is
 *     relied upon, not checked (unsorted rows give wrong numbers, not stray accesses).
 *   - "device" entry points take HBM-resident CSR (int64 row offsets, int32 column
 *     indices) and device output buffers; they are what bench.py times.  Device
 *     arrays are trusted (no validation pass).  Arrays that did not come from
 *     sapca_upload_csr_* go through sapca_check_csr_device_* (are they safe and
 *     canonical?) or sapca_canonicalize_csr_device_* (make them so) first.
 *   - inputs are borrowed for the duration of a call; outputs are written into
 *     caller-allocated buffers.
 *   - a handle is not thread-safe; distinct handles may be used concurrently.
 *
 * Deviations from the reference (everything else, quirks included, is the reference's behaviour):
 *   1. a fit whose SVD returns fewer than k values gives SAPCA_ERR_SVD where the reference panics on s[i]
 *      (sparse/mod.rs:213-215);
 *   2. mean_ has n_cols zeros when center = false (the reference: n_samples zeros, never read, sparse/mod.rs:116);
 *   3. no unconditional stdout (the reference prints from MaskedSparsePCA::fit, sparse_masked/mod.rs:373-378);
 *   4. n_components + n_oversamples is limited to 1024 (tuned to 128);
 *   5. SVDMethod::Lanczos: svd_las2 of single-svdlib is SVDLIBC's las2, a single-vector Lanczos with SELECTIVE
 *      re-orthogonalisation; csrc/lanczos.hip keeps the recurrence, the end interval [-1e-30, 1e30], kappa and the iteration
 *      cap of the call sites (sparse/mod.rs:135-143, sparse_masked/mod.rs:316-331) but re-orthogonalises every new vector
 *      against all previous ones (two passes of classical Gram-Schmidt on the device: one GEMV pair instead of las2's
 *      bookkeeping of which Ritz vectors have converged).  Converged triplets agree to kappa; the number of Lanczos steps
 *      taken, and triplets that have NOT converged at the cap, can differ.
 *      Repeated values: the Krylov space of one start vector holds one vector per DISTINCT singular value, so a
 *      single-vector Lanczos may return fewer copies of a repeated (or, within kappa, nearly repeated) singular value than its
 *      multiplicity and fill up with the next smaller ones, as las2 may; every returned triplet is a true one.
 *      Rank: a Ritz value of the Gram matrix at or below 1e-12 of the largest (sigma_i <= 1e-6 sigma_1) is a zero with its
 *      rounding, whatever its sign, and is never accepted as a triplet.  When the Krylov space is exhausted (beta_j <= 1e-13 of
 *      the largest Ritz value) with at least n_components values above that floor the fit ends there with exact triplets; with
 *      fewer -- a matrix of rank below n_components, a matrix of zeros -- it is SAPCA_ERR_SVD, "SVD computation failed: the
 *      operator has r singular values above 1e-6 of the largest, k singular triplets were asked for" (deviation 1), on the
 *      tall and the wide side alike and on every call.  The cap reached without k accepted triplets: "SVD computation failed:
 *      Lanczos did not converge k singular triplets within j steps".
 */
#ifndef SAPCA_H
#define SAPCA_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SAPCA_ABI_VERSION 4   /* 2: sapca_timings grew sweep_kernel / sweep_slots_*; sapca_comm_rccl_available
                                 3: sapca_multi_* (one handle, several GPUs), sapca_upload_values_changed
                                 4: *_csr_device_to_host_*, sapca_comm_abort / _async_error / _has_side_lane,
                                    sapca_multi_upload_csr_* and the sapca_multi_*_resident calls
                                 additive, ABI 4: sapca_batch_stats_csr_device_*, sapca_sum_row_n_top_csr_device_*,
                                                  sapca_masked_stats_csr_device_*
                                 additive, ABI 4: sapca_options.reserved0 became lanczos_center (same size and offsets;
                                                  0, the value every caller passed, is the behaviour of before)
                                 additive, ABI 4: sapca_select_rows_csr_device_*
                                 additive, ABI 4: sapca_check_csr_device_*, sapca_canonicalize_csr_device_*
                                 additive, ABI 4: sapca_select_submatrix_csr_device_*
                                 additive, ABI 4: sapca_covariate_basis, sapca_set_covariates, sapca_get_covariate_rank,
                                                  sapca_project_out_panel_*
                                 additive, ABI 4: sapca_knn_device_*
                                 additive, ABI 4: sapca_set_column_scaling, sapca_get_column_scale,
                                                  sapca_scale_panel_rows_*
                                 additive, ABI 4: sapca_tsne_options_default, sapca_tsne_affinities_device_*,
                                                  sapca_tsne_gradient_device_*, sapca_tsne_embed_device_*,
                                                  sapca_tsne_device_*, sapca_tsne_*
                                 additive, ABI 4: sapca_kmeans_options_default, sapca_kmeans_seed_device_*,
                                                  sapca_kmeans_assign_device_*, sapca_kmeans_update_device_*,
                                                  sapca_kmeans_device_*, sapca_kmeans_*
                                 additive, ABI 4: sapca_umap_options_default, sapca_umap_find_ab, sapca_umap_graph_device_*,
                                                  sapca_umap_embed_device_*, sapca_umap_device_*, sapca_umap_*
                                 additive, ABI 4: sapca_louvain_options_default, sapca_louvain_modularity_device_*,
                                                  sapca_louvain_sweep_device_*, sapca_louvain_aggregate_device_*,
                                                  sapca_louvain_device_*, sapca_louvain_*
                                 additive, ABI 4: sapca_rank_sums_csr_device_*, sapca_rank_groups_csr_device_*
                                 additive, ABI 4: sapca_normalize_panel_ex_*, sapca_rotate_panel_*
                                 additive, ABI 4: sapca_graph_components_device, sapca_spectral_options_default,
                                                  sapca_spectral_scale_device_*, sapca_spectral_apply_device_*,
                                                  sapca_spectral_device_*, sapca_spectral_*,
                                                  sapca_umap_spectral_init_device_*
                                 additive, ABI 4: sapca_spectral_options.reserved became single_round (same size and offsets;
                                                  0, what a zeroed or defaulted struct holds, is the default; a value above 1,
                                                  ignored before, is now SAPCA_ERR_ARG)
                                 additive, ABI 4: sapca_harmony_assign_device_*, sapca_harmony_centroids_device_*,
                                                  sapca_harmony_correct_device_*, sapca_harmony_device_*, sapca_harmony_* */

typedef struct sapca_handle_s* sapca_handle;

typedef enum sapca_status {
  SAPCA_OK = 0,
  SAPCA_ERR_ARG = 1,        /* bad argument / unsupported size                                  */
  SAPCA_ERR_MASK_LEN = 2,   /* "The mask vector length and the number of features (columns)
                               have to be the same!"   sparse_masked/mod.rs:258-262, 440-444    */
  SAPCA_ERR_NOT_FITTED = 3, /* "Must be fitted before transform!" sparse/mod.rs:259,263;
                               "Model must be fitted first!"      sparse/mod.rs:299,316          */
  SAPCA_ERR_SVD = 4,        /* "SVD computation failed: .." / "Randomized SVD computation
                               failed: .." sparse/mod.rs:144,180; also returned where the
                               reference would panic on s[i] (rank < k), sparse/mod.rs:213-215   */
  SAPCA_ERR_HIP = 5,        /* HIP runtime error (message carries hipGetErrorString)            */
  SAPCA_ERR_COMM = 6,       /* RCCL / collective error                                          */
  SAPCA_ERR_NOMEM = 7
} sapca_status;

/* SVDMethod                                     src/dimred/pca/mod.rs:49-68 (default Lanczos) */
typedef enum sapca_method { SAPCA_LANCZOS = 0, SAPCA_RANDOM = 1 } sapca_method;
/* PowerIterationNormalizer (re-export)          src/dimred/pca/mod.rs:41                      */
typedef enum sapca_normalizer { SAPCA_NORM_QR = 0, SAPCA_NORM_LU = 1, SAPCA_NORM_NONE = 2 } sapca_normalizer;
/* transform semantics: REFERENCE reproduces quirks Q2/Q3; CENTERED is the
 * mathematically centred projection (A - 1 mu^T) V^T, offered as an opt-in superset; its counterpart on the fit side
 * is sapca_options.lanczos_center (the Lanczos SVD of the centred operator).  Both together: the textbook PCA.      */
typedef enum sapca_transform_semantics { SAPCA_TRANSFORM_REFERENCE = 0, SAPCA_TRANSFORM_CENTERED = 1 } sapca_transform_semantics;

/* Builder fields.  SparsePCABuilder sparse/mod.rs:375-484 (defaults :392-401);
 * MaskedSparsePCABuilder sparse_masked/mod.rs:37-160 (defaults :55-66).
 * alpha and tolerance are stored and never read by the reference; kept for drop-in.          */
typedef struct sapca_options {
  uint32_t struct_size;          /* = sizeof(sapca_options); ABI growth guard                   */
  uint32_t random_seed;          /* .random_seed(u32), default 42                               */
  uint64_t n_components;         /* .n_components(usize), default 50                            */
  double alpha;                  /* .alpha(T), default 1.0 (unused)                             */
  double tolerance;              /* .tolerance(T), default 1e-6 (unused)                        */
  uint8_t center;                /* .center(bool), default 1                                    */
  uint8_t verbose;               /* .verbose(bool), default 0                                   */
  uint8_t collect_timings;       /* record per-stage HIP-event timings (sapca_get_timings)      */
  uint8_t lanczos_center;        /* opt-in, default 0: with center = 1 and SAPCA_LANCZOS the SVD runs on the centred
                                    operator A - 1 mu^T (a real PCA) instead of the raw matrix (the reference's quirk Q1);
                                    mean_, the total variance and transform are what they are without it.  No effect
                                    with center = 0 or SAPCA_RANDOM (which centres anyway)                            */
  int32_t method;                /* sapca_method, default SAPCA_LANCZOS                         */
  uint64_t n_oversamples;        /* SVDMethod::Random.n_oversamples (n_components + this: at most 1024; above 128 block-wise, untuned) */
  uint64_t n_power_iterations;   /* SVDMethod::Random.n_power_iterations                        */
  int32_t normalizer;            /* sapca_normalizer                                            */
  int32_t transform_semantics;   /* sapca_transform_semantics                                   */
  int32_t device_id;             /* HIP device ordinal; -1 = current device                     */
  int32_t spmm_variant;          /* 0 = auto; 1 = L2-gather row kernel; 2 = LDS-tiled kernel    */
  void* stream;                  /* hipStream_t to run on; NULL = library-owned stream          */
} sapca_options;

/* per-stage device timings of the last fit/transform (ms, HIP events on the handle's stream) */
typedef struct sapca_timings {
  double upload_ms;          /* narrowing + H2D (host entry points only)                        */
  double prepare_ms;         /* mask compaction, transpose, tile formats                        */
  double stats_ms;           /* column statistics                                               */
  double spmm_ms;            /* sum over the A*X sweeps                                         */
  double spmmt_ms;           /* sum over the A^T*Y sweeps                                       */
  double ortho_ms;           /* Gram / Cholesky / panel GEMM                                    */
  double small_svd_ms;       /* final factorisation incl. host Jacobi                           */
  double lanczos_ms;
  double transform_ms;
  double comm_ms;            /* collectives: device time (events around every all-reduce) when
                              * timings are collected, host-observed time otherwise            */
  double fit_total_ms;
  uint32_t n_spmm;           /* number of A*X sweeps timed                                      */
  uint32_t n_spmmt;
  double spmm_sweep_ms[32];  /* individual sweeps, in launch order                              */
  double spmmt_sweep_ms[32];
  double bytes_per_sweep;    /* ALGORITHMIC bytes of one sweep (SURVEY.md §8d formula)          */
  uint64_t lanczos_steps;
  uint32_t sweep_kernel;     /* randomized fits: 0 row-gather kernel, 1 staged-entry quad sweep,
                              * 2 DPP-fed quad sweep (spmm_dq.hip)                              */
  uint32_t at_sweep_pieces;  /* multi-rank randomized fits: 2 when the A^T sweeps ran in two pieces with the first
                              * piece's panel all-reduce behind the second piece's sweep; else 1 (0: no sweep) */
  uint64_t sweep_slots_a;    /* entry slots (stored entries + padding) one A*X sweep walks; 0 on
                              * the row-gather kernel.  x 256 B (f32, 64 columns) = LDS gather bytes */
  uint64_t sweep_slots_at;   /* the same for one A^T*Y sweep                                    */
} sapca_timings;

void sapca_options_default(sapca_options* o);
int sapca_abi_version(void);

/* SparsePCABuilder::build / MaskedSparsePCABuilder::build   sparse/mod.rs:470-483, masked :144-159 */
sapca_status sapca_create(const sapca_options* opts, sapca_handle* out);
void sapca_destroy(sapca_handle h);
const char* sapca_last_error(sapca_handle h);   /* valid until the next call on h; h may be NULL (create errors) */

/* MaskedSparsePCABuilder::mask(Vec<bool>)       sparse_masked/mod.rs:111-114.  len is checked
 * against ncols at fit/transform time like the reference (:258-262).  len == 0 clears it.    */
sapca_status sapca_set_mask(sapca_handle h, const uint8_t* mask, size_t len);

/* Test hook: inject the Gaussian test matrix Omega (n_used x (k+p), row-major, host) used by
 * the next randomized fit instead of the built-in generator -- the reference's rand-0.9
 * stream is not reproducible, so parity is checked with a shared Omega.       */
sapca_status sapca_set_omega_f32(sapca_handle h, const float* omega, size_t rows, size_t cols);
sapca_status sapca_set_omega_f64(sapca_handle h, const double* omega, size_t rows, size_t cols);

/* ---- per-row covariates, regressed out implicitly (opt-in; the reference has no counterpart: its consumers build the dense
 * residual matrix on the host) ----
 * A randomized fit with covariates set is the fit of R = (I - Q Q^T) A, where Q is an orthonormal basis of the design matrix
 * D = [1 | z] (options.center = 1: the intercept IS the centring) or D = z (center = 0).  R is never formed: the sweeps run
 * uncentred, every A-sweep's panel is projected (Y <- Y - Q (Q^T Y), csrc/covar.hip) and every A^T-sweep is corrected by
 * G (Q^T Y), G = A^T Q, so that it is A^T (I - Q Q^T) Y whatever rounding left in Y.  Batch labels (one-hot columns),
 * sequencing depth, any regress_out-style covariate and per-batch centring are designs of a few columns; collinear designs
 * (one-hot codes of every batch plus the intercept) are legal: only the span matters.
 *   fit        every fitted quantity is that of R under the same options -- singular values, components (with svd_flip),
 *              explained_variance_ = sigma^2 / (m - 1), the ratios, importances -- except mean_, which stays the column means
 *              of A (zeros for center = 0).  The total variance is sum_j (sumsq_j - |(Q^T A)_j|^2) / (m - 1) over the columns
 *              the fit uses for center = 1, and the reference's quirk unchanged (sum sigma_i^2 / (m - 1), sparse/mod.rs:218-223)
 *              for center = 0.  The denominator stays m - 1 (not m - rank): the results equal those of this library run on
 *              the densified R.  n_components > min(m - rank, n_used) is SAPCA_ERR_SVD ("n_components exceeds the matrix
 *              dimensions").
 *   transform  (SAPCA_TRANSFORM_CENTERED only) scores = A V^T - Q_rows C with C = Q^T A V^T (rank x k, stored at fit) and
 *              Q_rows = D_rows W built from the covariates set at the time of the call: the fitted matrix's (the result is
 *              (I - Q Q^T) A V^T), or a new matrix's own rows for out-of-sample scoring, with `cols` as at fit.  Out-of-sample
 *              results are unique when the new design rows lie in the row space of the fit's design; otherwise the
 *              pivot-column solution W of sapca_covariate_basis applies (dependent design columns have zero coefficients).
 * SAPCA_ERR_ARG, checked on the host before anything is enqueued (the handle stays usable, a fitted model stays fitted):
 * more than SAPCA_MAX_DESIGN_COLUMNS design columns; a non-finite covariate; z == NULL with rows * cols > 0; rows != m at
 * fit or transform ("covariates have R rows, the matrix M"); SAPCA_LANCZOS ("covariates need SVDMethod::Random": the
 * reference's Lanczos branch does not centre at all, quirk Q1); SAPCA_TRANSFORM_REFERENCE at transform / fit_transform (quirks
 * Q2 / Q3 have no meaning on residuals); a handle that belongs to a communicator, sapca_multi_* members included (the
 * projection would need an all-reduce per sweep); a model fitted with covariates transformed without them, or the reverse;
 * a different `cols` than at fit.  A handle on which covariates were never set, or were cleared, takes exactly the code
 * paths it took before this feature existed and launches none of its kernels.                                          */
#define SAPCA_MAX_DESIGN_COLUMNS 16   /* covariate columns + the intercept that center = 1 adds */
/* Pure host code, no handle (like sapca_partition_rows).  z: rows x cols, row-major, finite.  Each design column is scaled to
 * unit norm (a zero column is dropped), then a Householder QR with column pivoting in f64; rank r = #{j : |R_jj| >
 * max(rows, design columns) eps_f64 |R_00|}.  q (rows x 16, row-major) receives the first r columns of Q, zero padded;
 * w ((cols + center) x 16, zero padded) the map Q = D W: the basic solution on the pivot columns, dependent columns get zero
 * rows.  Rank 0 is valid and means "no correction".                                                                    */
sapca_status sapca_covariate_basis(const double* z, uint64_t rows, uint64_t cols, int32_t center, double* q, double* w, uint64_t* rank);
/* Stores z (HOST, rows x cols f64 row-major, copied) on the handle, like sapca_set_mask and sapca_set_omega_*: the next fit or
 * transform uses it, and rows must equal that call's m.  rows == 0 or cols == 0 clears.                                */
sapca_status sapca_set_covariates(sapca_handle h, const double* z, uint64_t rows, uint64_t cols);
/* design columns (cols + center) and rank of the basis of the fitted model; 0, 0 when it was fitted without covariates */
sapca_status sapca_get_covariate_rank(sapca_handle h, uint64_t* design_cols, uint64_t* rank);

/* ---- column scaling, applied implicitly (opt-in; the reference has no counterpart: standardising a sparse matrix on the host
 * makes it dense) ----
 * A randomized fit with a scaling set is the fit of S = (A - 1 mu^T) diag(d) (options.center = 1) or S = A diag(d) (center = 0)
 * over the columns the fit uses (under a mask d is compacted like the columns).  S is never formed and no value of A is
 * rewritten: A (D X) and D (A^T Y) only touch the thin column-side panels (csrc/colscale.hip); the sweeps, the formats, the
 * preparation cache and the statistics gathered at upload do not depend on d.
 *   d          SAPCA_SCALE_WEIGHTS: d_j = weights[j]; a weight of 0 drops the column from the fit.
 *              SAPCA_SCALE_UNIT_VARIANCE: from the fit's own f64 column sums, ss_j = sumsq_j - sum_j^2 / m, var_j = ss_j / (m - 1),
 *              d_j = 1 / sqrt(var_j), and d_j = 0 where ss_j <= 4 m eps_f64 sumsq_j: empty columns, columns constant over all
 *              rows and what rounding leaves of a constant column (ss may even come out negative there).  The variance is
 *              taken about the mean whatever `center` is; m is the global row count on a communicator.
 *   fit        singular values, components (k x n_used, right singular vectors of S, with svd_flip), explained_variance_ =
 *              sigma^2 / (m - 1), the ratios and importances are those of S; mean_ stays the column means of A.  The total
 *              variance for center = 1 is sum_j d_j^2 var_j (under UNIT_VARIANCE: the number of columns with d_j > 0); for
 *              center = 0 the reference's quirk is unchanged.  A component's entry at a column with d_j = 0 is exactly 0.
 *   transform  (SAPCA_TRANSFORM_CENTERED only) scores = (A - 1 mu^T) diag(d) V^T with the d and mu stored at the fit, for the
 *              fitted matrix and for out-of-sample rows alike; what is set on the handle then only concerns the next fit.
 *   with       masks; host, device-resident and *_to_host entry points; handles of a communicator and sapca_multi members
 *              (every rank derives the same d from the all-reduced statistics; no collective is added or changes size; like
 *              sapca_set_omega_*, the setting has to be applied to every member); SAPCA_SCALE_WEIGHTS with covariates, the
 *              operator being (I - Q Q^T) A diag(d) and the total variance (sum_j d_j^2 sumsq_j - |Q^T A D|_F^2) / (m - 1).
 * SAPCA_ERR_ARG, checked on the host before anything is enqueued (the handle stays usable, a fitted model stays fitted): an
 * unknown mode; weights == NULL with mode 2 and len > 0, or a weights pointer with mode 1; a negative or non-finite weight
 * ("column scaling: weight W at column J"); len != n at fit ("column scaling has L weights, the matrix N columns");
 * SAPCA_LANCZOS ("column scaling needs SVDMethod::Random"); SAPCA_TRANSFORM_REFERENCE at transform / fit_transform of a scaled
 * model ("column scaling needs SAPCA_TRANSFORM_CENTERED": quirks Q2 / Q3 have no meaning on scaled columns); UNIT_VARIANCE with
 * m < 2; UNIT_VARIANCE together with covariates ("pass explicit weights").  A handle on which scaling was never set, or was
 * reset to SAPCA_SCALE_NONE, launches none of this feature's kernels and gives bit-identical results.                      */
typedef enum sapca_column_scaling { SAPCA_SCALE_NONE = 0, SAPCA_SCALE_UNIT_VARIANCE = 1, SAPCA_SCALE_WEIGHTS = 2 } sapca_column_scaling;
/* Stored on the handle like the mask and the covariates; used by the NEXT fit.  weights: HOST, f64, len = n (all columns of the
 * matrix, like the mask), copied; only for SAPCA_SCALE_WEIGHTS.  SAPCA_SCALE_NONE clears.                                  */
sapca_status sapca_set_column_scaling(sapca_handle h, int32_t mode, const double* weights, uint64_t len);
/* Of the FITTED model: its mode and the n_used factors the fit applied (aligned with the components' columns).  mode and out
 * may be NULL; a model fitted without scaling reports mode 0 and writes nothing.                                          */
sapca_status sapca_get_column_scale(sapca_handle h, int32_t* mode, double* out, size_t cap);

/* SparsePCA::fit / MaskedSparsePCA::fit          sparse/mod.rs:102-242; masked :255-419
 * Host matrices: the column statistics of the fit (sum_col, sum_col_squared, csr.rs:259-312 and
 * 558-608, and the per-column counts) are gathered behind the upload's DMA as exact sums rounded
 * once -- independent of summation order, hence bit-reproducible; inf/nan values switch to the
 * row sums of the transposed matrix, which device-resident inputs always use.                  */
sapca_status sapca_fit_csr_f32(sapca_handle h, uint64_t m, uint64_t n, uint64_t nnz,
                               const uint64_t* row_offsets, const uint64_t* col_indices, const float* values);
sapca_status sapca_fit_csr_f64(sapca_handle h, uint64_t m, uint64_t n, uint64_t nnz,
                               const uint64_t* row_offsets, const uint64_t* col_indices, const double* values);
/* SparsePCA::transform / MaskedSparsePCA::transform   sparse/mod.rs:255-285; masked :438-546.
 * out: m x n_components, row-major (ndarray Array2 standard layout).                          */
sapca_status sapca_transform_csr_f32(sapca_handle h, uint64_t m, uint64_t n, uint64_t nnz,
                                     const uint64_t* row_offsets, const uint64_t* col_indices, const float* values, float* out);
sapca_status sapca_transform_csr_f64(sapca_handle h, uint64_t m, uint64_t n, uint64_t nnz,
                                     const uint64_t* row_offsets, const uint64_t* col_indices, const double* values, double* out);
/* fit_transform                                   sparse/mod.rs:355-358; masked :616-619        */
sapca_status sapca_fit_transform_csr_f32(sapca_handle h, uint64_t m, uint64_t n, uint64_t nnz,
                                         const uint64_t* row_offsets, const uint64_t* col_indices, const float* values, float* out);
sapca_status sapca_fit_transform_csr_f64(sapca_handle h, uint64_t m, uint64_t n, uint64_t nnz,
                                         const uint64_t* row_offsets, const uint64_t* col_indices, const double* values, double* out);

/* Same three operations on HBM-resident CSR (device pointers: int64 row offsets [m+1],
 * int32 column indices [nnz], values [nnz]); `out` is a device buffer m x n_components.
 * The matrix is borrowed: it must stay valid and unmodified until the call returns.
 * Nothing derived from caller-owned arrays outlives the call: a later sapca_transform_csr_device_*
 * on the same pointers re-derives what it needs (they may hold different values by then); only
 * fit_transform, and the library-owned arrays of sapca_upload_csr_*, reuse the fit's preparation.
 * When the handle belongs to a multi-rank communicator (sapca_comm_*), (m, row_offsets, ..)
 * describe THIS rank's row shard and n is the global column count.                            */
sapca_status sapca_fit_csr_device_f32(sapca_handle h, uint64_t m, uint64_t n, uint64_t nnz,
                                      const int64_t* d_row_offsets, const int32_t* d_col_indices, const float* d_values);
sapca_status sapca_fit_csr_device_f64(sapca_handle h, uint64_t m, uint64_t n, uint64_t nnz,
                                      const int64_t* d_row_offsets, const int32_t* d_col_indices, const double* d_values);
sapca_status sapca_transform_csr_device_f32(sapca_handle h, uint64_t m, uint64_t n, uint64_t nnz,
                                            const int64_t* d_row_offsets, const int32_t* d_col_indices, const float* d_values, float* d_out);
sapca_status sapca_transform_csr_device_f64(sapca_handle h, uint64_t m, uint64_t n, uint64_t nnz,
                                            const int64_t* d_row_offsets, const int32_t* d_col_indices, const double* d_values, double* d_out);
sapca_status sapca_fit_transform_csr_device_f32(sapca_handle h, uint64_t m, uint64_t n, uint64_t nnz,
                                                const int64_t* d_row_offsets, const int32_t* d_col_indices, const float* d_values, float* d_out);
sapca_status sapca_fit_transform_csr_device_f64(sapca_handle h, uint64_t m, uint64_t n, uint64_t nnz,
                                                const int64_t* d_row_offsets, const int32_t* d_col_indices, const double* d_values, double* d_out);
/* The same two calls with the m x n_components projection delivered to HOST memory (through the
 * handle's page-locked ring): what a caller whose matrix is resident (sapca_upload_csr_*) but whose
 * consumer is host code -- the reference's Array2<T> result, sparse/mod.rs:255-285 -- wants.     */
sapca_status sapca_transform_csr_device_to_host_f32(sapca_handle h, uint64_t m, uint64_t n, uint64_t nnz,
                                                    const int64_t* d_row_offsets, const int32_t* d_col_indices, const float* d_values, float* out);
sapca_status sapca_transform_csr_device_to_host_f64(sapca_handle h, uint64_t m, uint64_t n, uint64_t nnz,
                                                    const int64_t* d_row_offsets, const int32_t* d_col_indices, const double* d_values, double* out);
sapca_status sapca_fit_transform_csr_device_to_host_f32(sapca_handle h, uint64_t m, uint64_t n, uint64_t nnz,
                                                        const int64_t* d_row_offsets, const int32_t* d_col_indices, const float* d_values, float* out);
sapca_status sapca_fit_transform_csr_device_to_host_f64(sapca_handle h, uint64_t m, uint64_t n, uint64_t nnz,
                                                        const int64_t* d_row_offsets, const int32_t* d_col_indices, const double* d_values, double* out);

/* Fitted state.  The reference keeps components_/explained_variance_/mean_ private
 * (sparse/mod.rs:41-43); a Rust wrapper needs them to populate those fields.
 * dims: k = n_components, n_used = columns seen by the SVD (n, or n' under a mask),
 * n_cols = columns of the fitted matrix (length of mean_).
 * mean_ and the total variance come from f64 column sums of a and a^2.  The sums of a Lanczos fit on the scatter route
 * (n_used <= m, m >= 4096, n_used doubles fit LDS: csrc/scatter.hip) are fixed-point: exact to rows * max|a| * 2^-61 per stored
 * entry (rows * max|a|^2 * 2^-61 for the squares), max|a| taken over the whole matrix.  That is absolute, not relative to the
 * column: a column whose values are many orders of magnitude below max|a| keeps fewer digits than a floating-point sum would.  */
sapca_status sapca_get_dims(sapca_handle h, uint64_t* k, uint64_t* n_used, uint64_t* n_cols);
sapca_status sapca_get_components_f32(sapca_handle h, float* out, size_t cap);            /* k x n_used   sparse/mod.rs:208 */
sapca_status sapca_get_components_f64(sapca_handle h, double* out, size_t cap);
sapca_status sapca_get_singular_values_f32(sapca_handle h, float* out, size_t cap);       /* k            res.s             */
sapca_status sapca_get_singular_values_f64(sapca_handle h, double* out, size_t cap);
sapca_status sapca_get_explained_variance_f32(sapca_handle h, float* out, size_t cap);    /* k            sparse/mod.rs:210-216 */
sapca_status sapca_get_explained_variance_f64(sapca_handle h, double* out, size_t cap);
sapca_status sapca_get_mean_f32(sapca_handle h, float* out, size_t cap);                  /* n_cols       sparse/mod.rs:106-117 */
sapca_status sapca_get_mean_f64(sapca_handle h, double* out, size_t cap);
sapca_status sapca_get_total_variance(sapca_handle h, double* out);                       /* sparse/mod.rs:119-131, 218-223 */
/* explained_variance_ratio()                      sparse/mod.rs:312-322; masked :574-582       */
sapca_status sapca_get_explained_variance_ratio_f32(sapca_handle h, float* out, size_t cap);
sapca_status sapca_get_explained_variance_ratio_f64(sapca_handle h, double* out, size_t cap);
/* cumulative_explained_variance_ratio()           sparse/mod.rs:333-343; masked :593-603       */
sapca_status sapca_get_cumulative_explained_variance_ratio_f32(sapca_handle h, float* out, size_t cap);
sapca_status sapca_get_cumulative_explained_variance_ratio_f64(sapca_handle h, double* out, size_t cap);
/* feature_importances()                           sparse/mod.rs:295-302; masked :557-564       */
sapca_status sapca_get_feature_importances_f32(sapca_handle h, float* out, size_t cap);   /* k x n_used */
sapca_status sapca_get_feature_importances_f64(sapca_handle h, double* out, size_t cap);
/* cols_to_use (ascending, sparse_masked/mod.rs:264-271) and the col -> masked-index map of
 * :462-466 as a dense table (-1 = column dropped).  Integer, bit-exact.  Either may be NULL.  */
sapca_status sapca_get_mask_index_maps(sapca_handle h, uint64_t* cols_to_use, size_t cap_cols,
                                       int64_t* orig_to_masked, size_t cap_map);
sapca_status sapca_get_timings(sapca_handle h, sapca_timings* out);

/* ---- stage-level operators (host buffers in and out), used by the parity tests ------------ */
/* <CsrMatrix as MatrixSum>::sum_col / sum_col_squared   src/sparse/csr.rs:259-312, 558-608.
 * One fused device pass yields both plus the per-column stored-entry count (any may be NULL). */
sapca_status sapca_colstats_csr_f32(sapca_handle h, uint64_t m, uint64_t n, uint64_t nnz,
                                    const uint64_t* row_offsets, const uint64_t* col_indices, const float* values,
                                    float* sum_col, float* sum_col_squared, uint64_t* nonzero_col);
sapca_status sapca_colstats_csr_f64(sapca_handle h, uint64_t m, uint64_t n, uint64_t nnz,
                                    const uint64_t* row_offsets, const uint64_t* col_indices, const double* values,
                                    double* sum_col, double* sum_col_squared, uint64_t* nonzero_col);
/* The two sweeps inside single_svdlib::randomized::randomized_svd (call sites
 * sparse/mod.rs:170-180): Y = (A - 1 mu^T) X   (X: n x l, Y: m x l) and
 * Z = (A - 1 mu^T)^T Y (Y: m x l, Z: n x l); row-major, mu may be NULL (uncentred).         */
sapca_status sapca_spmm_csr_f32(sapca_handle h, uint64_t m, uint64_t n, uint64_t nnz,
                                const uint64_t* row_offsets, const uint64_t* col_indices, const float* values,
                                const float* mu, uint64_t l, const float* X, float* Y);
sapca_status sapca_spmm_csr_f64(sapca_handle h, uint64_t m, uint64_t n, uint64_t nnz,
                                const uint64_t* row_offsets, const uint64_t* col_indices, const double* values,
                                const double* mu, uint64_t l, const double* X, double* Y);
sapca_status sapca_spmmt_csr_f32(sapca_handle h, uint64_t m, uint64_t n, uint64_t nnz,
                                 const uint64_t* row_offsets, const uint64_t* col_indices, const float* values,
                                 const float* mu, uint64_t l, const float* Y, float* Z);
sapca_status sapca_spmmt_csr_f64(sapca_handle h, uint64_t m, uint64_t n, uint64_t nnz,
                                 const uint64_t* row_offsets, const uint64_t* col_indices, const double* values,
                                 const double* mu, uint64_t l, const double* Y, double* Z);
/* PowerIterationNormalizer applied to a rows x l row-major panel in place (QR: orthonormal
 * basis of the same span; LU: well-conditioned basis of the same span; NONE: untouched).     */
sapca_status sapca_normalize_panel_f32(sapca_handle h, int32_t normalizer, uint64_t rows, uint64_t l, float* panel);
sapca_status sapca_normalize_panel_f64(sapca_handle h, int32_t normalizer, uint64_t rows, uint64_t l, double* panel);
/* The projection of the covariate route on a rows x l row-major panel in place: panel <- panel - Q (Q^T panel), with Q a
 * rows x r panel (r <= 16) taken as given (orthonormal columns make it the orthogonal projection).  Q^T panel is summed in
 * f64 in a fixed order: the same bytes from call to call.                                                             */
sapca_status sapca_project_out_panel_f32(sapca_handle h, uint64_t rows, uint64_t l, float* panel, uint32_t r, const float* q);
sapca_status sapca_project_out_panel_f64(sapca_handle h, uint64_t rows, uint64_t l, double* panel, uint32_t r, const double* q);
/* The row scaling of the column-scaling route on a rows x l row-major panel in place: panel[r][:] *= T(scale[r]); the factor
 * is rounded once to T, each product once (csrc/colscale.hip).                                                           */
sapca_status sapca_scale_panel_rows_f32(sapca_handle h, uint64_t rows, uint64_t l, float* panel, const double* scale);
sapca_status sapca_scale_panel_rows_f64(sapca_handle h, uint64_t rows, uint64_t l, double* panel, const double* scale);
/* The normaliser as a fit calls it, for inspection: the panel arrives as the sum of `nsplit` row-major rows x l slabs (slab s
 * at slabs + s * rows * l; one slab is staged in the panel buffer itself, several in a buffer of their own -- the two shapes
 * the A^T sweeps leave behind) minus the centring term mu sv^T (mu: rows, sv: l; both NULL or both given).  passes: 0 = what
 * the normaliser implies (QR two, LU one), else 1 or 2 CholeskyQR passes.  panel_out (rows x l) receives the normalised panel
 * (SAPCA_NORM_NONE: the summed, centred panel), vec_out (l, nullable) sum_r w[r] panel_out[r][:] (w: rows, NULL = ones) as the
 * Gram's read pass and R^-1 give it, r1 / r2 (l x l f64 row-major, nullable) the upper factors of the first / second pass
 * (zeros for a pass that did not run), *regularised (nullable) the number of pivots the factorisations floored.           */
sapca_status sapca_normalize_panel_ex_f32(sapca_handle h, int32_t normalizer, int32_t passes, uint64_t rows, uint64_t l,
                                          uint32_t nsplit, const float* slabs, const float* mu, const float* sv, const float* w,
                                          float* panel_out, float* vec_out, double* r1, double* r2, int32_t* regularised);
sapca_status sapca_normalize_panel_ex_f64(sapca_handle h, int32_t normalizer, int32_t passes, uint64_t rows, uint64_t l,
                                          uint32_t nsplit, const double* slabs, const double* mu, const double* sv, const double* w,
                                          double* panel_out, double* vec_out, double* r1, double* r2, int32_t* regularised);
/* The rotation a randomized fit ends in, for inspection: components (k x n row-major) = svd_flip((panel factor)^T) for an
 * n x l row-major panel and an l x k f64 row-major factor, 1 <= k <= l <= 1024, n >= 1.  Row c is column c of the product
 * times signs[c] (k doubles, nullable): -1 where the entry of largest magnitude in that column (the first row on ties) is
 * negative, else +1 (a column without a largest entry -- all nan -- keeps +1).  Drops the handle's fitted model.           */
sapca_status sapca_rotate_panel_f32(sapca_handle h, uint64_t n, uint64_t l, uint64_t k, const float* panel, const double* factor,
                                    float* components, double* signs);
sapca_status sapca_rotate_panel_f64(sapca_handle h, uint64_t n, uint64_t l, uint64_t k, const double* panel, const double* factor,
                                    double* components, double* signs);
/* The built-in Omega generator (rows x l standard normal from (seed)), for inspection.        */
sapca_status sapca_generate_omega_f32(sapca_handle h, uint64_t rows, uint64_t l, float* out);
sapca_status sapca_generate_omega_f64(sapca_handle h, uint64_t rows, uint64_t l, double* out);

/* ---- device-resident workflow: upload once, preprocess and analyse in HBM ----
 * The consumer's typical pipeline is normalize -> log1p -> PCA (/root/reference/src/lib.rs:28-33).
 * sapca_upload_csr_* copies a host CsrMatrix (usize indices) into buffers owned by the handle and
 * returns the device arrays (valid until the next host-matrix call on this handle or its
 * destruction); the *_device_* entry points below and sapca_fit*_csr_device_* then work on them
 * without touching PCIe again.  The column statistics gathered during the upload serve a fit of
 * the arrays as uploaded; normalize / log1p on them drop those statistics.                      */
sapca_status sapca_upload_csr_f32(sapca_handle h, uint64_t m, uint64_t n, uint64_t nnz,
                                  const uint64_t* row_offsets, const uint64_t* col_indices, const float* values,
                                  const int64_t** d_row_offsets, const int32_t** d_col_indices, float** d_values);
sapca_status sapca_upload_csr_f64(sapca_handle h, uint64_t m, uint64_t n, uint64_t nnz,
                                  const uint64_t* row_offsets, const uint64_t* col_indices, const double* values,
                                  const int64_t** d_row_offsets, const int32_t** d_col_indices, double** d_values);
/* <CsrMatrix<T> as Normalize<T>>::normalize::<f64>(&sums, target, &direction)
 * (/root/reference/src/sparse/csr.rs:1012-1066): every stored value of row (direction 0) or
 * column (direction 1) i becomes T(f64(value) * (target / sums[i])) where sums[i] > 0; others
 * are left alone.  `sums` is a HOST array of length m (ROW) or n (COLUMN); a wrong length is
 * SAPCA_ERR_ARG (the dense twin's message, src/dense/mod.rs; the CSR impl would index out of
 * bounds).  `values` is the DEVICE value array, modified in place.                             */
sapca_status sapca_normalize_csr_device_f32(sapca_handle h, uint64_t m, uint64_t n, uint64_t nnz,
                                            const int64_t* row_offsets, const int32_t* col_indices, float* values,
                                            const double* sums, uint64_t sums_len, double target, int32_t direction);
sapca_status sapca_normalize_csr_device_f64(sapca_handle h, uint64_t m, uint64_t n, uint64_t nnz,
                                            const int64_t* row_offsets, const int32_t* col_indices, double* values,
                                            const double* sums, uint64_t sums_len, double target, int32_t direction);
/* <CsrMatrix<T> as Log1P<T>>::log1p_normalize (csr.rs:1069-1078): value = ln(1 + value), in
 * place on the DEVICE value array.  The sum 1 + value is T's own, as in the reference (not a true
 * log1p: |value| <= eps/4 and subnormals give +0.0); the logarithm is evaluated in f64 and rounded
 * once to T, within 1 ulp of T of whatever a libm ln returns.  value = -1 gives -inf, value < -1
 * and NaN give NaN, +inf stays +inf, -0.0 gives +0.0.                                            */
sapca_status sapca_log1p_csr_device_f32(sapca_handle h, uint64_t nnz, float* values);
sapca_status sapca_log1p_csr_device_f64(sapca_handle h, uint64_t nnz, double* values);
/* d_values of sapca_upload_csr_* is writable: a caller that edits the uploaded values with its own
 * kernel (anything but the two entry points above) says so here BEFORE the next fit, so that the
 * column statistics gathered during the upload and any cached preparation are dropped and the
 * fit re-derives mean_ / the total variance from the values as they are now.  The reference has
 * no counterpart (a &CsrMatrix is immutable while borrowed, sparse/mod.rs:102).                  */
sapca_status sapca_upload_values_changed(sapca_handle h);
/* The per-row (direction 0) or per-column (direction 1) statistics of the MatrixSum /
 * MatrixNonZero / MatrixMinMax traits in one call on a device-resident CSR: sum_row|col
 * (csr.rs:259-392), sum_row|col_squared (:558-630), nonzero_row|col (:23-134, stored entries),
 * min_max_row|col (:917-1008: over the stored entries; a row/column without any keeps
 * (T::MAX, -T::MAX), the reference's initial values).  min/max compare with `<` and `>` as the
 * reference does, so a NaN never wins a comparison, and each direction starts where the reference
 * starts:
 *   ROW (:987-1005)   from the row's FIRST stored value: a row that begins with a NaN is
 *                     (NaN, NaN); a NaN later in a row is ignored; a row of +inf alone (or +inf
 *                     followed by NaNs) has min +inf, a row of -inf alone has max -inf.
 *   COLUMN (:921-922, :960-967) from (T::MAX, -T::MAX): NaNs are ignored wherever they sit (a
 *                     column of NaNs alone keeps (MAX, -MAX)); a column of +inf alone keeps min
 *                     T::MAX (max +inf), a column of -inf alone keeps max -T::MAX (min -inf).
 * The sign of a zero min or max is not specified.  Sums over a line that holds an inf or a NaN
 * propagate it as an f64 sum does; f32 subnormals are not flushed.  Outputs are HOST arrays of
 * length m or n; any may be NULL.  Sums are accumulated in f64 (the reference accumulates in the caller's T, in
 * storage order).  var_row|col (csr.rs:632-726) is host arithmetic on these:
 *   var = (sumsq/N - (sum/N)^2) * N/(N-1), N = the other dimension.                             */
sapca_status sapca_stats_csr_device_f32(sapca_handle h, uint64_t m, uint64_t n, uint64_t nnz,
                                        const int64_t* row_offsets, const int32_t* col_indices, const float* values,
                                        int32_t direction, double* sum, double* sum_squared, uint64_t* nonzero,
                                        float* min_out, float* max_out);
sapca_status sapca_stats_csr_device_f64(sapca_handle h, uint64_t m, uint64_t n, uint64_t nnz,
                                        const int64_t* row_offsets, const int32_t* col_indices, const double* values,
                                        int32_t direction, double* sum, double* sum_squared, uint64_t* nonzero,
                                        double* min_out, double* max_out);

/* BatchMatrixVariance::var_batch_row|col and BatchMatrixMean::mean_batch_row|col (csr.rs:1081-1344)
 * on a device-resident CSR.  `codes` is a HOST array of dense batch codes in [0, n_batches):
 *   grouped_axis 0: codes label the ROWS (codes_len == m); results per column, each n long
 *                   (var_batch_row, mean_batch_col);
 *   grouped_axis 1: codes label the COLUMNS (codes_len == n); results per row, each m long
 *                   (var_batch_col, mean_batch_row).
 * Outputs are HOST arrays of n_batches x (n or m), code-major; any may be NULL:
 *   count[b][j] = stored entries of line j in group b (implicit zeros are not counted, stored zeros are);
 *   var[b][j]   = sum (x - mu)^2 / (count - 1) over those entries, mu = their sum / count, 0 when count <= 1
 *                 (the reference's two passes, csr.rs:1118-1160, 1212-1237);
 *   mean[b][j]  = (sum of those entries) / (number of rows | columns with code b): implicit zeros count
 *                 (csr.rs:1290-1293, 1337-1340).
 * A code that never occurs gives 0 everywhere.  The reference accumulates in the caller's T; here every
 * sum is accumulated in f64.  A wrong codes_len is SAPCA_ERR_ARG with the message of the reference
 * method: var_*'s ("Batch vector length (..) doesn't match matrix row|column count (..)") when var is
 * requested, mean_*'s ("Number of batch identifiers (..) must match number of rows|columns (..)")
 * otherwise; so are a code outside [0, n_batches) and grouped_axis outside {0, 1}.  grouped_axis 0
 * transposes the matrix into the buffers prepare() uses (a cached preparation is dropped).          */
sapca_status sapca_batch_stats_csr_device_f32(sapca_handle h, uint64_t m, uint64_t n, uint64_t nnz,
                                              const int64_t* row_offsets, const int32_t* col_indices, const float* values,
                                              int32_t grouped_axis, const int32_t* codes, uint64_t codes_len,
                                              uint32_t n_batches, double* mean, double* var, uint64_t* count);
sapca_status sapca_batch_stats_csr_device_f64(sapca_handle h, uint64_t m, uint64_t n, uint64_t nnz,
                                              const int64_t* row_offsets, const int32_t* col_indices, const double* values,
                                              int32_t grouped_axis, const int32_t* codes, uint64_t codes_len,
                                              uint32_t n_batches, double* mean, double* var, uint64_t* count);
/* MatrixNTop::sum_row_n_top (csr.rs:1347-1376) for several n at once: out[i * m + r] (HOST, n_ns x m)
 * = sum of the min(ns[i], stored entries of row r) largest STORED values of row r (negative values and
 * stored zeros compete like any other; n = 0 gives 0), accumulated in f64 (the reference: in T).  NaN
 * values give an unspecified result.  n_ns == 0 is SAPCA_ERR_ARG.                                     */
sapca_status sapca_sum_row_n_top_csr_device_f32(sapca_handle h, uint64_t m, uint64_t n, uint64_t nnz,
                                                const int64_t* row_offsets, const int32_t* col_indices, const float* values,
                                                const uint64_t* ns, uint32_t n_ns, double* out);
sapca_status sapca_sum_row_n_top_csr_device_f64(sapca_handle h, uint64_t m, uint64_t n, uint64_t nnz,
                                                const int64_t* row_offsets, const int32_t* col_indices, const double* values,
                                                const uint64_t* ns, uint32_t n_ns, double* out);

/* MatrixNonZero::nonzero_{col,row}_masked, MatrixSum::sum_{col,row}_masked, MatrixVariance::var_{col,row}_masked
 * (csr.rs:153-252, 418-556, 815-914) and, with mask == NULL, the stored-entry variance of var_{col,row}_chunk
 * (csr.rs:728-813) on a device-resident CSR:
 *   direction 0 (ROW):    m results, one per row, over the stored entries whose COLUMN is kept;
 *   direction 1 (COLUMN): n results, one per column, over the stored entries whose ROW is kept.
 * `mask` is a HOST byte array, non-zero = kept; NULL keeps everything.  A mask_len below the masked dimension is
 * SAPCA_ERR_ARG with the reference's message ("Mask length (..) is less than number of rows (..)" for COLUMN,
 * ".. number of columns (..)" for ROW); a longer mask's tail is ignored (the reference's sum_col_masked /
 * var_col_masked index past the row offsets on a true tail entry).  Outputs are HOST arrays, any may be NULL:
 *   count = kept stored entries (stored zeros count); sum, sum_squared = their sum and sum of squares;
 *   var   = stored-entry variance, no correction, 0 where count is 0: ROW two passes, sum (x - mean)^2 / count
 *           (csr.rs:889-911); COLUMN sum_squared / count - mean^2 (csr.rs:852-859).
 * The reference accumulates in the caller's T; here every sum is f64.  COLUMN sums are order-independent: the
 * correctly rounded exact sums (the upload's accumulators, csrc/upstats.hip), bit-identical from call to call, and no
 * transposition is made; dropped rows are not read.  A kept inf / nan propagates as in an f64 sum (those columns are
 * then summed on a transposition, as is a matrix too wide for the accumulators, which drops a cached preparation);
 * one in a dropped row or column changes nothing.  A direction outside {0, 1} is SAPCA_ERR_ARG.                    */
sapca_status sapca_masked_stats_csr_device_f32(sapca_handle h, uint64_t m, uint64_t n, uint64_t nnz,
                                               const int64_t* row_offsets, const int32_t* col_indices, const float* values,
                                               int32_t direction, const uint8_t* mask, uint64_t mask_len,
                                               double* sum, double* sum_squared, uint64_t* count, double* var);
sapca_status sapca_masked_stats_csr_device_f64(sapca_handle h, uint64_t m, uint64_t n, uint64_t nnz,
                                               const int64_t* row_offsets, const int32_t* col_indices, const double* values,
                                               int32_t direction, const uint8_t* mask, uint64_t mask_len,
                                               double* sum, double* sum_squared, uint64_t* count, double* var);

/* Rows of a device-resident CSR as a CSR of their own (the reference slices on the host: CsrMatrix has no row selection;
 * its consumers filter cells, fit on reference cells, fit per cluster or batch, subsample and bootstrap).  Output row i is
 * source row rows[i]: its entries in stored order, column indices unchanged, values copied bit for bit (NaN payloads, -0.0
 * and stored zeros survive).  `rows` is a HOST array; it may be in any order and may repeat (a mask is the ascending
 * special case), so the output is n_rows x n and *nnz_out may exceed nnz.  n_rows == 0 is valid: a one-element offset
 * array {0} and *nnz_out = 0.
 * SAPCA_ERR_ARG, checked on the host before anything is enqueued (the handle stays usable): rows[i] >= m ("select_rows: row
 * index R at position I is out of range (m = M)"); rows == NULL with n_rows > 0; a null output pointer; a source that is
 * the handle's own selection buffers.
 * The outputs (device int64 offsets [n_rows + 1], int32 column indices, values) live in buffers owned by the handle, distinct
 * from those of sapca_upload_csr_*: the full matrix stays resident beside its subset.  They are valid until the next
 * sapca_select_rows_csr_device_* on this handle or its destruction, complete when the call returns, and writable
 * (sapca_normalize_csr_device_* / sapca_log1p_csr_device_* may run on them); every *_csr_device_* entry point takes them.
 * The source matrix, and the column statistics gathered during its upload, are untouched: a later fit of the uploaded
 * arrays still finds them.  A cached preparation is dropped only if it was made of the previous selection.
 * On a handle that belongs to a communicator the call is local to the rank: it selects from that rank's shard (rows index
 * the shard) and issues no collective.                                                                              */
sapca_status sapca_select_rows_csr_device_f32(sapca_handle h, uint64_t m, uint64_t n, uint64_t nnz,
                                              const int64_t* row_offsets, const int32_t* col_indices, const float* values,
                                              const uint64_t* rows, uint64_t n_rows, uint64_t* nnz_out,
                                              const int64_t** d_row_offsets, const int32_t** d_col_indices, float** d_values);
sapca_status sapca_select_rows_csr_device_f64(sapca_handle h, uint64_t m, uint64_t n, uint64_t nnz,
                                              const int64_t* row_offsets, const int32_t* col_indices, const double* values,
                                              const uint64_t* rows, uint64_t n_rows, uint64_t* nnz_out,
                                              const int64_t** d_row_offsets, const int32_t** d_col_indices, double** d_values);

/* Rows AND columns of a device-resident CSR in one call: A[rows][:, col_mask] as a CSR of its own.  The column half is
 * the reference's MaskedCSRMatrix::new(x, mask) -- cols_to_use ascending, a kept column renumbered by its rank among the
 * kept ones (sparse_masked/mod.rs:264-271, 455-466) -- offered as a resident matrix instead of a private step of one fit:
 * gene filters (min-cells, highly variable genes) then serve the statistics, normalisation and every fit of a sweep,
 * the compaction is paid once, and the dropped columns need not stay in HBM.
 *   rows      HOST; as in sapca_select_rows_csr_device_* (any order, repeats allowed); NULL = rows 0 .. n_rows-1 in
 *             order (n_rows <= m).  Output row i is source row rows[i], its kept entries in stored order.
 *   col_mask  HOST, mask_len == n entries, non-zero = kept; NULL = every column (mask_len ignored).  A kept column c
 *             becomes the number of kept columns below c; *n_cols_out = the kept columns (n without a mask).  A mask,
 *             not a list: ascending by construction, so a canonical source gives a canonical result.
 *   flags     SAPCA_SELECT_DROP_STORED_ZEROS: entries whose value == 0 (either sign) are dropped as well -- the stored
 *             zeros that sapca_check_csr_device_* counts and that the reference's nonzero_* and quirk Q2 count as
 *             entries.  A NaN is kept.  Without the flag stored zeros survive.
 * Values move bit for bit (NaN payloads, -0.0).  n_rows == 0, an all-false mask (*n_cols_out = 0, every offset 0) and a
 * mask that keeps only columns without entries are valid.  With no mask (or one that keeps every column) and no flag the
 * result is byte-identical to sapca_select_rows_csr_device_* of the same rows, by the same kernels.  The result is
 * deterministic: the same bytes from call to call (no atomics; every output word has one writer).
 * SAPCA_ERR_ARG, checked on the host before anything is enqueued (the previous selection stays intact, the handle usable):
 * mask_len != n with a mask ("select_submatrix: the column mask has L entries, the matrix N columns"); rows[i] >= m
 * ("select_submatrix: row index R at position I is out of range (m = M)"); rows == NULL with n_rows > m; unknown flag
 * bits; a null output pointer; a source that is the handle's own selection buffers.
 * The outputs live in the SAME buffers as those of sapca_select_rows_csr_device_*, with the same lifetime and "writable"
 * contract: one selection per handle, either call replaces it.  The source, the column statistics gathered during its
 * upload and any cached preparation not made of the previous selection are untouched.  On a handle that belongs to a
 * communicator the call is local to the rank and issues no collective.                                               */
#define SAPCA_SELECT_DROP_STORED_ZEROS 1u   /* drop entries whose value == 0 (either sign); NaN is kept */
sapca_status sapca_select_submatrix_csr_device_f32(sapca_handle h, uint64_t m, uint64_t n, uint64_t nnz,
                                                   const int64_t* row_offsets, const int32_t* col_indices, const float* values,
                                                   const uint64_t* rows, uint64_t n_rows,
                                                   const uint8_t* col_mask, uint64_t mask_len, uint32_t flags,
                                                   uint64_t* n_cols_out, uint64_t* nnz_out,
                                                   const int64_t** d_row_offsets, const int32_t** d_col_indices, float** d_values);
sapca_status sapca_select_submatrix_csr_device_f64(sapca_handle h, uint64_t m, uint64_t n, uint64_t nnz,
                                                   const int64_t* row_offsets, const int32_t* col_indices, const double* values,
                                                   const uint64_t* rows, uint64_t n_rows,
                                                   const uint8_t* col_mask, uint64_t mask_len, uint32_t flags,
                                                   uint64_t* n_cols_out, uint64_t* nnz_out,
                                                   const int64_t** d_row_offsets, const int32_t** d_col_indices, double** d_values);

/* ---- the gate in front of the device entry points: check and canonicalise a device-resident CSR ----
 * Every kernel relies on offsets that start at 0, end at nnz and never decrease, on columns < n, and on rows whose
 * columns ascend without repeats.  Arrays that came through sapca_upload_csr_* have all of it; anything else (a
 * transposed, multiplied or fancy-indexed scipy result, an .h5ad another tool wrote, a CSR built from COO, a caller's
 * own kernel) is checked here, on the GPU, where it already is.  "Canonical" is (flags & 15) == 0.                  */
#define SAPCA_CSR_BAD_OFFSETS   1u   /* ptr[0] != 0, ptr[m] != nnz, or ptr[r+1] < ptr[r]            */
#define SAPCA_CSR_COL_RANGE     2u   /* a column index < 0 or >= n                                  */
#define SAPCA_CSR_UNSORTED      4u   /* a row with an entry whose column is below its predecessor's */
#define SAPCA_CSR_DUPLICATES    8u   /* an entry whose column equals its predecessor's in the row   */
#define SAPCA_CSR_NONFINITE    16u   /* an inf / nan value (allowed by the fits; reported)          */

typedef struct sapca_csr_report {
  uint32_t struct_size;          /* = sizeof(sapca_csr_report), set by the caller (growth guard)    */
  uint32_t flags;
  uint64_t first_bad_offset_row, cols_out_of_range, first_out_of_range_row;
  uint64_t unsorted_rows, first_unsorted_row;
  uint64_t duplicate_entries, first_duplicate_row;
  uint64_t nonfinite_values, first_nonfinite_row;
  uint64_t stored_zeros;
} sapca_csr_report;

/* Read-only check.  Finding a defect is not an error: the call returns SAPCA_OK and fills *report; SAPCA_ERR_ARG is for
 * a null report or a report->struct_size other than sizeof(sapca_csr_report).  Counts are exact, independent of the
 * launch geometry and the same from call to call; a first_*_row whose count is zero is UINT64_MAX.
 * Two stages.  The offsets are checked by a kernel that reads row_offsets[0 .. m] only, and its verdict reaches the host
 * before anything else runs: with broken offsets the report carries SAPCA_CSR_BAD_OFFSETS and first_bad_offset_row (the
 * first r with ptr[r+1] < ptr[r]; 0 for ptr[0] != 0; m for ptr[m] != nnz) and says nothing about the entries, which are
 * not read.  With sound offsets one pass reads each of the three arrays once, inside [0, nnz).
 * Columns are compared as unsigned numbers (a negative index is out of range and larger than any valid one), and only
 * with the predecessor in the SAME row.  unsorted_rows counts rows, the other counts entries.  duplicate_entries counts
 * duplicates that are adjacent in stored order: that is every duplicate when the row is sorted; an unsorted row can
 * hide duplicates that are not adjacent, and the exact number is what sapca_canonicalize_csr_device_* reports.
 * stored_zeros counts values equal to zero (either sign).  On a handle that belongs to a communicator the call is
 * local to the rank and issues no collective.                                                                        */
sapca_status sapca_check_csr_device_f32(sapca_handle h, uint64_t m, uint64_t n, uint64_t nnz,
                                        const int64_t* row_offsets, const int32_t* col_indices, const float* values,
                                        sapca_csr_report* report);
sapca_status sapca_check_csr_device_f64(sapca_handle h, uint64_t m, uint64_t n, uint64_t nnz,
                                        const int64_t* row_offsets, const int32_t* col_indices, const double* values,
                                        sapca_csr_report* report);

/* The canonical form: output row r holds the entries of input row r in ascending column order, and entries of equal
 * column are merged into one whose value is their sum in T, added left to right in the input's stored order (the sort
 * is stable: scipy's sum_duplicates, nalgebra's COO -> CSR conversion).  An entry that is not merged keeps its value bit
 * for bit: NaN payloads, -0.0 and stored zeros survive; stored zeros are not dropped, and neither is a merged sum that
 * comes to zero.  The result is deterministic.  Rows have fewer than 2^32 entries.
 * Already canonical input: nothing is copied or allocated for it; *d_row_offsets == row_offsets, *d_col_indices ==
 * col_indices, *d_values == values and *nnz_out == nnz, at the cost of the check's one pass.
 * SAPCA_ERR_ARG, with nothing written and the handle usable: broken offsets ("canonicalize: the row offsets are broken at
 * row R ...") or a column out of range ("canonicalize: K column indices are out of range (n = N), the first in row R
 * ...") cannot be repaired; a null output pointer; a source inside this handle's own canonical buffers; a report with
 * the wrong struct_size.
 * Otherwise the outputs (device int64 offsets [m + 1], int32 column indices, values) live in a third set of buffers owned
 * by the handle, distinct from those of sapca_upload_csr_* and sapca_select_rows_csr_device_*: the source -- the upload,
 * the selection or the caller's own arrays -- stays resident and untouched beside them.  They are valid until the next
 * sapca_canonicalize_csr_device_* on this handle or its destruction, complete when the call returns, and writable; every
 * *_csr_device_* entry point takes them.  A cached preparation is dropped only if it was made of the previous canonical
 * result; the statistics gathered at upload stay valid for the uploaded arrays.
 * report (may be NULL; struct_size set by the caller) describes the INPUT: the flags and counts of the check, except
 * that duplicate_entries is exact here, nnz - *nnz_out (first_duplicate_row stays the check's: the first row with an
 * adjacent duplicate).  On a handle that belongs to a communicator the call is local to the rank (it acts on the shard)
 * and issues no collective.                                                                                          */
sapca_status sapca_canonicalize_csr_device_f32(sapca_handle h, uint64_t m, uint64_t n, uint64_t nnz,
                                               const int64_t* row_offsets, const int32_t* col_indices, const float* values,
                                               uint64_t* nnz_out, const int64_t** d_row_offsets, const int32_t** d_col_indices,
                                               float** d_values, sapca_csr_report* report);
sapca_status sapca_canonicalize_csr_device_f64(sapca_handle h, uint64_t m, uint64_t n, uint64_t nnz,
                                               const int64_t* row_offsets, const int32_t* col_indices, const double* values,
                                               uint64_t* nnz_out, const int64_t** d_row_offsets, const int32_t** d_col_indices,
                                               double** d_values, sapca_csr_report* report);

/* ---- the step behind PCA: exact k-nearest neighbours of device-resident score rows ----
 * The fit and the projection leave the m x n_components scores in HBM; the neighbour graph of those rows feeds clustering,
 * UMAP / t-SNE and label transfer.  The reference has no such call: its notion of "near" is the SimilarityMeasure trait of
 * src/similarity/mod.rs (a file its lib.rs does not compile), and this is the neighbour search built on three of its
 * measures, an opt-in superset like row selection and covariates.
 * Both inputs are row-major DEVICE panels of d columns with row strides ldq, ldc >= d (a slice of a wider buffer is legal;
 * nothing beyond column d of a row is read).  d_queries == d_corpus is the usual case, neighbours within one fitted
 * matrix; another query panel is the out-of-sample case.  Row i of the outputs (DEVICE, mq x n_neighbors each) holds the
 * n_neighbors corpus rows nearest to query i, best first: d_indices the corpus row numbers, d_values
 *   SAPCA_KNN_EUCLIDEAN  the distance |a - b| (EuclideanSimilarity's `dist`, similarity/mod.rs:59-64, before its exp(-gamma .));
 *   SAPCA_KNN_COSINE     CosineSimilarity::calculate, similarity/mod.rs:14-36: <a, b> / sqrt(|a|^2 |b|^2);
 *   SAPCA_KNN_PEARSON    PearsonSimilarity::calculate, similarity/mod.rs:69-101: the same on the rows minus their own means.
 * The order is part of the contract: by value (ascending distance, descending similarity), then by ascending corpus index.
 * The result is deterministic, the same bytes from call to call and whatever the launch geometry (no atomics decide an
 * order; every output word has one writer).
 * The search ranks by alpha <a, b> + bias on the f32 / f64 matrix cores and keeps the best n_neighbors under the key
 * (score, -index); the values are then recomputed for the selected pairs from the rows as given, in f64, rounded once to T,
 * and each list is sorted again by (value, index).  The selection is exact up to the rounding of its inner products: where
 * two candidates' scores differ by less than about 4 d eps_T (|a| + max |b|)^2 either may be kept.
 * SAPCA_KNN_EXCLUDE_SELF skips corpus row j == i for query i: by index, not by distance, so a duplicate of a point is still
 * a neighbour at distance 0.
 * Deviation from the reference (the only one): it compares the PAIR's norm product with T::epsilon() (similarity/mod.rs:30,
 * :95); here a ROW whose norm (after centring, for PEARSON) is <= sqrt(eps_T) is the zero vector, and its similarity to
 * everything is 0 -- a property of the row, so that the search can scale every row once.
 * The norm is summed in f64 in one order where the rows are scaled and in another where the values are recomputed: a row
 * whose norm lies within f64 rounding (a relative 1e-15) of sqrt(eps_T) may be zero for one and not for the other -- it is
 * then ranked as the zero vector and reported with its true similarity, or the reverse; the lists stay sorted by value.
 * A non-finite input value gives unspecified neighbours for the rows it touches; a list slot that was never filled holds
 * index -1 and NaN; no index outside [-1, mc) is ever written.
 * Outputs are complete when the call returns.  The call runs on the handle's stream, works in buffers of its own (a fitted
 * model, a cached preparation and the upload's statistics are untouched) and, on a handle that belongs to a communicator,
 * is local to the rank and issues no collective.  mq == 0 is valid and writes nothing (the sizes are still checked, the
 * pointers are not looked at).
 * SAPCA_ERR_ARG, checked on the host before anything is enqueued (the handle stays usable), each with a message that names
 * the offending number: an unknown metric; unknown flag bits; n_neighbors == 0; n_neighbors > SAPCA_KNN_MAX_NEIGHBORS;
 * d == 0 or d > 1024; ldq < d or ldc < d (or a stride >= 2^28); mc >= 2^31 (or mq); n_neighbors > mc - (EXCLUDE_SELF ? 1 : 0); a null pointer
 * with a non-empty shape.                                                                                              */
typedef enum sapca_knn_metric { SAPCA_KNN_EUCLIDEAN = 0, SAPCA_KNN_COSINE = 1, SAPCA_KNN_PEARSON = 2 } sapca_knn_metric;
#define SAPCA_KNN_EXCLUDE_SELF 1u
#define SAPCA_KNN_MAX_NEIGHBORS 128
sapca_status sapca_knn_device_f32(sapca_handle h, uint64_t mq, const float* d_queries, uint64_t ldq,
                                  uint64_t mc, const float* d_corpus, uint64_t ldc,
                                  uint64_t d, int32_t metric, uint32_t n_neighbors, uint32_t flags,
                                  int32_t* d_indices, float* d_values);
sapca_status sapca_knn_device_f64(sapca_handle h, uint64_t mq, const double* d_queries, uint64_t ldq,
                                  uint64_t mc, const double* d_corpus, uint64_t ldc,
                                  uint64_t d, int32_t metric, uint32_t n_neighbors, uint32_t flags,
                                  int32_t* d_indices, double* d_values);

/* ---- the second half of the reference's dimred: t-SNE of device-resident score rows (dimred::tsne) ----
 * The reference's src/dimred/tsne/mod.rs:7-66 holds TSNEConfig { output_dim, perplexity, epochs, theta } and run_f32 /
 * run_f64, which hand a dense row-major panel to bhtsne's Barnes-Hut t-SNE with a Euclidean metric.  These calls replace
 * them on the scores a fit_transform left in HBM.  PARITY STATUS: UNPINNED, as for the PCA: the source of bhtsne is not
 * available to this project, so the algorithm is van der Maaten's bh_tsne (which the crate ports), stated here in full and
 * pinned by a numpy restatement (tests/tsne_ref.py) and by scikit-learn's t-SNE gradient, not by the crate.
 *   1. K = floor(3 perplexity) Euclidean nearest neighbours of every row, itself excluded (sapca_knn_device_*).
 *   2. Per row i, with D_k the squared distances: beta_i from 1, bounds -inf / +inf, doubled or halved while the far bound
 *      is infinite, else bisected, at most 200 steps; a step takes p_k = exp(-beta D_k), s = sum p + DBL_MIN,
 *      H = ln s + beta sum(D_k p_k) / s and stops when |H - ln perplexity| < 1e-5 (H larger: beta rises).  p_k|i = p_k / s
 *      at the beta the search ended on.  All f64 whatever T is.  A slot whose index is outside [0, m) (the search's -1)
 *      contributes nothing.
 *   3. P_ij = (p_j|i + p_i|j) / (2 m), the sum in f64, rounded once to T: bh_tsne's symmetrise-then-divide-by-the-total,
 *      since every conditional row sums to 1.  A canonical CSR: int64 offsets, int32 columns ascending without repeats.
 *   4. q_ij = 1 / (1 + |y_i - y_j|^2), Z = sum_{i != j} q_ij,
 *      g_i = e sum_j P_ij q_ij (y_i - y_j) - (1 / Z) sum_{j != i} q_ij^2 (y_i - y_j)   (the Barnes-Hut form, no factor 4),
 *      KL = sum over stored P_ij of P_ij ln(P_ij Z / q_ij) with the unexaggerated P.  The pair i == j is left out by
 *      index; coincident rows i != j count q = 1 and exert no force.
 *   5. Per epoch t: e = exaggeration for t < stop_lying_epoch, else 1; mu = momentum for t < momentum_switch_epoch, else
 *      final_momentum; gain += 0.2 where sign(g) != sign(v) (sign in {-1, 0, +1}), else gain *= 0.8, then max(gain, 0.01);
 *      v = mu v - learning_rate gain g; y += v; every column of y re-centred to mean zero (the mean summed in f64 in a
 *      fixed order).  Start: gain 1, v 0, y = 1e-4 N(0, 1) from the built-in generator (sapca_generate_omega's, on an
 *      m x output_dim panel) under random_seed, or the caller's panel (init_given), re-centred first.
 * Deviations from the reference:
 *   1. The repulsive term is evaluated exactly, the limit theta -> 0 of the tree: theta is accepted and stored for drop-in
 *      and not read; results are those of barnes_hut(0.0, ..).
 *   2. For T = f32 the affinities (stages 2-3) are computed in f64 and rounded once, and the repulsion folds its f32
 *      per-lane sums into f64 once per 1024 rows j; the crate works in T throughout.
 *   3. The initial embedding comes from this library's counter-based generator, not from the crate's rand stream.
 *   4. Re-centring in f32: the column mean is summed in f64 and y_i - mean is rounded to f32 once, so a stored f32 column has
 *      mean 0 only up to the mean of those roundings, at most 2^-24 max|y| (eps_f32 / 2); an f64 column to f64 rounding.
 * A single row (m == 1) has no pair: Z = 0, and the stage calls define the repulsion and the KL as 0 (no 0 / 0); its embedding
 * is the origin.
 * Deterministic: the same bytes from call to call.  Integer atomics count and hand out positions in stage 3, the rows are
 * then sorted by column and a pair's two terms added (a + b == b + a), so no order reaches a value; every floating-point sum
 * that crosses lanes or workgroups is added in an order fixed by the shape (the rows j are dealt into chunks by m alone,
 * every chunk summed from zero, the chunks added in order, whether one workgroup walks them or one takes each).
 * Outputs are complete when the call returns.  Every call runs on the handle's stream in buffers of its own: a fitted
 * model, a cached preparation, the upload's statistics, the selection and the canonical buffers are untouched; on a handle
 * that belongs to a communicator the call is local to the rank and issues no collective.  The epoch loop enqueues kernels
 * only (Z, the means and the KL terms stay on the device).
 * No index outside the arrays is touched: a neighbour slot or a column of P outside [0, m) is skipped where it is read (the
 * search's contract writes -1 only), the emitted positions are counted before they are written, and the offsets of a
 * caller's P are trusted as in every *_csr_device_* call.  Non-finite input values give an unspecified embedding.
 * SAPCA_ERR_ARG, checked on the host before anything is enqueued (the handle stays usable), each with a message that names
 * the offending number: a wrong struct_size; output_dim outside 1 .. 3; perplexity non-finite or < 1; K = floor(3 perplexity)
 * > SAPCA_KNN_MAX_NEIGHBORS ("perplexity P needs N neighbours, at most 128"); K > m - 1 ("perplexity too large for the number
 * of rows"); m >= 2^31; the d / stride limits of sapca_knn_device_*; a non-finite or negative constant; a null pointer with
 * a non-empty shape.  epochs == 0 is valid: the initial embedding, re-centred, and its KL.                              */
typedef struct sapca_tsne_options {
  uint32_t struct_size;            /* sizeof(sapca_tsne_options)                                       */
  uint32_t random_seed;            /* default 42                                                       */
  uint32_t output_dim;             /* TSNEConfig.output_dim (tsne/mod.rs:8), default 2; 1 .. 3         */
  uint32_t init_given;             /* 1: d_y / y holds the initial embedding                           */
  double perplexity;               /* TSNEConfig.perplexity (tsne/mod.rs:9), default 20 (bhtsne's)     */
  double theta;                    /* TSNEConfig.theta (tsne/mod.rs:11), default 0.5: stored, not read */
  uint64_t epochs;                 /* TSNEConfig.epochs (tsne/mod.rs:10), default 1000                 */
  uint64_t stop_lying_epoch;       /* default 250                                                      */
  uint64_t momentum_switch_epoch;  /* default 250                                                      */
  double exaggeration;             /* default 12                                                       */
  double learning_rate;            /* default 200                                                      */
  double momentum;                 /* default 0.5                                                      */
  double final_momentum;           /* default 0.8                                                      */
} sapca_tsne_options;
void sapca_tsne_options_default(sapca_tsne_options* opts);
/* Stages 2-3 on neighbour lists laid out as sapca_knn_device_* writes them (m x K, DEVICE; d_dist holds distances, not
 * squares; 1 <= K <= SAPCA_KNN_MAX_NEIGHBORS).  The symmetric P comes back in handle-owned DEVICE arrays like the selection's
 * and the canonical result's: valid until the next affinity call (sapca_tsne_device_* and sapca_tsne_* make one) or destroy,
 * and accepted by every *_csr_device_* entry point.  d_beta (m f64, DEVICE, may be NULL) receives beta_i.                  */
sapca_status sapca_tsne_affinities_device_f32(sapca_handle h, uint64_t m, const int32_t* d_indices, const float* d_dist, uint32_t K,
                                              double perplexity, uint64_t* nnz_out, const int64_t** d_row_offsets,
                                              const int32_t** d_col_indices, float** d_values, double* d_beta);
sapca_status sapca_tsne_affinities_device_f64(sapca_handle h, uint64_t m, const int32_t* d_indices, const double* d_dist, uint32_t K,
                                              double perplexity, uint64_t* nnz_out, const int64_t** d_row_offsets,
                                              const int32_t** d_col_indices, double** d_values, double* d_beta);
/* One evaluation of stage 4 (a stage-level operator for parity tests, like sapca_spmm_csr_*): P an m x m DEVICE CSR, d_y the
 * m x output_dim embedding with row stride ldy, d_grad m x output_dim packed (DEVICE); *Z and *kl on the HOST (may be NULL).  */
sapca_status sapca_tsne_gradient_device_f32(sapca_handle h, uint64_t m, uint64_t nnz, const int64_t* row_offsets, const int32_t* col_indices,
                                            const float* values, const float* d_y, uint64_t ldy, uint32_t output_dim,
                                            double exaggeration, float* d_grad, double* Z, double* kl);
sapca_status sapca_tsne_gradient_device_f64(sapca_handle h, uint64_t m, uint64_t nnz, const int64_t* row_offsets, const int32_t* col_indices,
                                            const double* values, const double* d_y, uint64_t ldy, uint32_t output_dim,
                                            double exaggeration, double* d_grad, double* Z, double* kl);
/* Stage 5 on a given P: d_y (m x output_dim packed, DEVICE) is read when opts->init_given and receives the embedding; *kl
 * (HOST, may be NULL) its Kullback-Leibler divergence.  perplexity is not read here.                                       */
sapca_status sapca_tsne_embed_device_f32(sapca_handle h, uint64_t m, uint64_t nnz, const int64_t* row_offsets, const int32_t* col_indices,
                                         const float* values, const sapca_tsne_options* opts, float* d_y, double* kl);
sapca_status sapca_tsne_embed_device_f64(sapca_handle h, uint64_t m, uint64_t nnz, const int64_t* row_offsets, const int32_t* col_indices,
                                         const double* values, const sapca_tsne_options* opts, double* d_y, double* kl);
/* Stages 1-5 on a resident m x d panel with row stride ldx (the scores of sapca_fit_transform_csr_device_*, searched in
 * place): exactly sapca_knn_device_* (EUCLIDEAN, EXCLUDE_SELF, K), sapca_tsne_affinities_device_*, sapca_tsne_embed_device_*.  */
sapca_status sapca_tsne_device_f32(sapca_handle h, uint64_t m, const float* d_x, uint64_t ldx, uint64_t d,
                                   const sapca_tsne_options* opts, float* d_y, double* kl);
sapca_status sapca_tsne_device_f64(sapca_handle h, uint64_t m, const double* d_x, uint64_t ldx, uint64_t d,
                                   const sapca_tsne_options* opts, double* d_y, double* kl);
/* The same with HOST arrays in and out (x: m x d row-major; y: m x output_dim): the drop-in for run_f32 / run_f64
 * (tsne/mod.rs:14-39, :41-66).                                                                                            */
sapca_status sapca_tsne_f32(sapca_handle h, uint64_t m, uint64_t d, const float* x, const sapca_tsne_options* opts, float* y, double* kl);
sapca_status sapca_tsne_f64(sapca_handle h, uint64_t m, uint64_t d, const double* x, const sapca_tsne_options* opts, double* y, double* kl);

/* ---- clustering of device-resident score rows: k-means (Lloyd) with k-means++ seeding ----
 * The reference has no k-means: like the neighbour search, the covariates and the column scaling this is an opt-in superset,
 * the third consumer of the score rows a fit_transform left in HBM.  The algorithm is stated here in full and pinned by a
 * numpy restatement (tests/kmeans_ref.py) that is itself held to scikit-learn's KMeans(algorithm="lloyd"), not by a crate.
 * The input x is a row-major DEVICE panel, m x d, with row stride ldx >= d: nothing beyond column d of a row is read, so a
 * slice of the score buffer is clustered in place.  The centroids C are k x d, packed, of type T; labels are int32.
 *   1. Seeding (init = SAPCA_KMEANS_PLUSPLUS): plain k-means++ (Arthur & Vassilvitskii), one trial per centre.  u_t =
 *      hash_u01(random_seed, 21, t), the counter generator behind sapca_generate_omega_* -- sapca.synth.hash_u01 -- on a
 *      stream of its own.  c_0 = row floor(u_0 m).  For t = 1 .. k-1: D_i = min_{s<t} |x_i - c_s|^2 by the direct formula in f64, S the
 *      inclusive prefix sums of D in f64, c_t = the first row i with S_i > u_t S_{m-1}; S_{m-1} == 0 (every row coincides with
 *      a chosen centre): c_t = row floor(u_t m).  The prefix sums are associated in an order fixed by m alone (blocks of 1024
 *      rows, doubling strides inside a wave), not the running order, so a row whose boundary S_i lies within m eps_f64 S_{m-1}
 *      of u_t S_{m-1} may give way to its neighbour.  Everything stays on the device: no index is read back between centres.
 *      init = SAPCA_KMEANS_GIVEN uses the caller's k x d centroids as they are.
 *   2. Assignment: label_i = argmin_c |x_i - c|^2, ties to the lower c.  The labels are those of the direct formula in f64;
 *      where a row's two smallest squared distances differ by less than 64 d eps_f64 (|x_i| + max_c |c|)^2 either may win.
 *      Mechanism: the rows are ranked by 2 <x, c> - |c|^2 on the f32 / f64 matrix cores, every row keeping its best and its
 *      second-best score; a row whose runner-up lies within 4 d eps_T (|x_i| + max |c|)^2 of its best (the bound of the
 *      neighbour search for an FMA chain of length d) is AMBIGUOUS and is decided by a second pass that evaluates all k direct
 *      distances in f64 and takes the least (distance, index).  The distance of every row to its chosen centroid is then
 *      recomputed by the direct formula in f64 and rounded once to T (d_dist2); the inertia is the f64 sum of the unrounded
 *      values in an order fixed by m.
 *   3. Update: c = (sum_{label_i = c} x_i) / n_c, the sum and the division in f64 whatever T is, rounded once to T.
 *      DEVIATION from scikit-learn: a cluster with no rows keeps its centroid (scikit-learn relocates it).  The rows are
 *      sorted by (label, row) with a counting sort and each cluster's list is summed over fixed slices that are added in
 *      order: the order of every sum is fixed by (m, k, d) and the labels alone; no floating-point atomic is used.
 *   4. The loop, scikit-learn's Lloyd rule:
 *        for i in 0 .. max_iter-1:
 *          labels = assign(C);  C_new = update(labels);  shift = sum |C_new - C|^2 (f64, on the stored T values);  C = C_new
 *          if i > 0 and labels == labels_prev: strict = true; break
 *          if shift <= tol_abs: break
 *        n_iter = i + 1 (0 when max_iter == 0);  if not strict: labels = assign(C)
 *        inertia = sum_i |x_i - C[labels_i]|^2
 *      tol_abs = tol x (the mean over the columns of the column's population variance), computed once on the device in f64
 *      in two passes; tol == 0 gives tol_abs = 0, which leaves the strict test (and a shift of exactly 0).  The loop enqueues
 *      kernels only: convergence sets a device flag that turns the iterations still enqueued into no-ops.  The host looks at
 *      the flag every 8 iterations to stop enqueueing; the result does not depend on when it looks.
 * Deterministic: the same bytes from call to call.  The labels do not depend on the launch geometry (a pair's score is the
 * same k-ordered FMA chain wherever it falls); integer atomics count rows, no order reaches a value.
 * Outputs are complete when the call returns.  Every call runs on the handle's stream in buffers of its own: a fitted model,
 * a cached preparation, the upload's statistics, the selection, the canonical and the t-SNE buffers are untouched; on a
 * handle that belongs to a communicator the call is local to the rank and issues no collective.
 * No address outside the arrays is touched: a label outside [0, n_clusters) given to the update call is skipped where it is
 * read (its row belongs to no cluster).  Non-finite input values give unspecified labels inside [0, n_clusters).
 * SAPCA_ERR_ARG, checked on the host before anything is enqueued (the handle stays usable), each with a message that names the
 * offending number: a wrong struct_size; n_clusters == 0; n_clusters > SAPCA_KMEANS_MAX_CLUSTERS; n_clusters > m when m > 0
 * (seeding and the whole run); an unknown init; tol negative or not finite; the d and stride limits of sapca_knn_device_*
 * (d in 1 .. 1024, ldx >= d, ldx < 2^28); m >= 2^31; a null pointer with a non-empty shape.  m == 0 is valid and writes
 * nothing (*inertia = 0, *n_iter = 0).                                                                                   */
typedef enum sapca_kmeans_init { SAPCA_KMEANS_PLUSPLUS = 0, SAPCA_KMEANS_GIVEN = 1 } sapca_kmeans_init;
#define SAPCA_KMEANS_MAX_CLUSTERS 1024
typedef struct sapca_kmeans_options {
  uint32_t struct_size;   /* sizeof(sapca_kmeans_options)                                         */
  uint32_t random_seed;   /* default 42                                                           */
  uint32_t n_clusters;    /* default 8; 1 .. SAPCA_KMEANS_MAX_CLUSTERS                            */
  uint32_t init;          /* sapca_kmeans_init, default SAPCA_KMEANS_PLUSPLUS                     */
  uint64_t max_iter;      /* default 300                                                          */
  double tol;             /* default 1e-4, relative to the mean column variance (scikit-learn's)  */
} sapca_kmeans_options;
void sapca_kmeans_options_default(sapca_kmeans_options* opts);
/* Stage 1 alone (a stage-level operator for the parity tests, like sapca_tsne_gradient_device_*): d_centroids (k x d, DEVICE)
 * receives the chosen rows, d_rows (k int32, DEVICE, may be NULL) their row numbers.                                      */
sapca_status sapca_kmeans_seed_device_f32(sapca_handle h, uint64_t m, const float* d_x, uint64_t ldx, uint64_t d, uint32_t n_clusters,
                                          uint32_t random_seed, float* d_centroids, int32_t* d_rows);
sapca_status sapca_kmeans_seed_device_f64(sapca_handle h, uint64_t m, const double* d_x, uint64_t ldx, uint64_t d, uint32_t n_clusters,
                                          uint32_t random_seed, double* d_centroids, int32_t* d_rows);
/* Stage 2 alone, which is also the out-of-sample `predict`: d_labels (m int32, DEVICE), d_dist2 (m, DEVICE, may be NULL) the
 * squared distance of every row to its centroid; *inertia and *n_ambiguous (the rows the second pass decided) on the HOST,
 * may be NULL.  n_clusters may exceed m here.                                                                             */
sapca_status sapca_kmeans_assign_device_f32(sapca_handle h, uint64_t m, const float* d_x, uint64_t ldx, uint64_t d, uint32_t n_clusters,
                                            const float* d_centroids, int32_t* d_labels, float* d_dist2, double* inertia,
                                            uint64_t* n_ambiguous);
sapca_status sapca_kmeans_assign_device_f64(sapca_handle h, uint64_t m, const double* d_x, uint64_t ldx, uint64_t d, uint32_t n_clusters,
                                            const double* d_centroids, int32_t* d_labels, double* d_dist2, double* inertia,
                                            uint64_t* n_ambiguous);
/* Stage 3 alone: d_centroids (k x d, DEVICE) is read for the clusters without rows, which keep theirs, and receives the
 * means; d_counts (k int64, DEVICE, may be NULL) the rows of every cluster.                                               */
sapca_status sapca_kmeans_update_device_f32(sapca_handle h, uint64_t m, const float* d_x, uint64_t ldx, uint64_t d, uint32_t n_clusters,
                                            const int32_t* d_labels, float* d_centroids, int64_t* d_counts);
sapca_status sapca_kmeans_update_device_f64(sapca_handle h, uint64_t m, const double* d_x, uint64_t ldx, uint64_t d, uint32_t n_clusters,
                                            const int32_t* d_labels, double* d_centroids, int64_t* d_counts);
/* Stages 1-4 on a resident panel: d_centroids (n_clusters x d, DEVICE) is read when opts->init == SAPCA_KMEANS_GIVEN and
 * receives the centroids, d_labels (m int32, DEVICE) the labels; *inertia and *n_iter on the HOST, may be NULL.            */
sapca_status sapca_kmeans_device_f32(sapca_handle h, uint64_t m, const float* d_x, uint64_t ldx, uint64_t d,
                                     const sapca_kmeans_options* opts, float* d_centroids, int32_t* d_labels, double* inertia,
                                     uint64_t* n_iter);
sapca_status sapca_kmeans_device_f64(sapca_handle h, uint64_t m, const double* d_x, uint64_t ldx, uint64_t d,
                                     const sapca_kmeans_options* opts, double* d_centroids, int32_t* d_labels, double* inertia,
                                     uint64_t* n_iter);
/* The same with HOST arrays in and out (x: m x d row-major; centroids: n_clusters x d; labels: m).                          */
sapca_status sapca_kmeans_f32(sapca_handle h, uint64_t m, uint64_t d, const float* x, const sapca_kmeans_options* opts, float* centroids,
                              int32_t* labels, double* inertia, uint64_t* n_iter);
sapca_status sapca_kmeans_f64(sapca_handle h, uint64_t m, uint64_t d, const double* x, const sapca_kmeans_options* opts, double* centroids,
                              int32_t* labels, double* inertia, uint64_t* n_iter);

/* ---- UMAP of device-resident score rows (sapca_umap_*) ----
 * The third consumer of the neighbour search, beside t-SNE and k-means.  The reference has no UMAP and umap-learn is not
 * available to this project: an opt-in superset.  PARITY STATUS: UNPINNED by any package; the algorithm is umap-learn's
 * (fuzzy_simplicial_set, find_ab_params, optimize_layout_euclidean) with the deviations listed below, stated here in full and
 * pinned by a numpy restatement (tests/umap_ref.py).  x is a row-major DEVICE panel, m x d, row stride ldx >= d, searched in
 * place.  n_neighbors follows umap-learn and counts the point itself: K = n_neighbors - 1 other rows are searched.
 *   1. K Euclidean nearest neighbours of every row, itself excluded (sapca_knn_device_*).
 *   2. Smooth distances, per row i, all f64 whatever T is.  A slot whose index is outside [0, m) (the search's -1) contributes
 *      nothing anywhere.  rho_i = the smallest distance > 0 among the row's valid slots, 0 when there is none
 *      (local_connectivity = 1).  target = log2(n_neighbors).  From lo = 0, hi = +inf, mid = 1, at most 64 steps:
 *      psum = sum_k (d_k - rho > 0 ? exp(-(d_k - rho) / mid) : 1); stop when |psum - target| < 1e-5; psum > target: hi = mid,
 *      mid = (lo + hi) / 2; otherwise lo = mid and mid is doubled while hi is infinite, else mid = (lo + hi) / 2.
 *      sigma_i = mid, then floored: with rho_i > 0 to 1e-3 (sum_k d_k) / n_neighbors, otherwise to 1e-3 (the sum over all valid
 *      slots of the panel) / (m n_neighbors) -- umap-learn's means, which count the point's own zero; both sums f64 in an
 *      order fixed by (m, K).  Membership a_ik = 1 where d_k - rho_i <= 0, else exp(-(d_k - rho_i) / sigma_i), this exp
 *      correctly rounded.
 *   3. Fuzzy union (set_op_mix_ratio = 1): G_ij = (a_ij + a_ji) - a_ij a_ji in f64, a missing direction counting 0 (the value
 *      is then exactly a), rounded once to T.  The expression is symmetric in its two terms: G_ij == G_ji bit for bit.  A
 *      canonical CSR: int64 offsets, int32 columns ascending without repeats.  (A list that names one row twice is outside
 *      the contract of the search; its repeats fold left to right.)
 *   4. Curve: a and b as given (both > 0), or, both 0, fitted as umap-learn's find_ab_params does: x_t = 3 spread t / 299 for
 *      t = 0 .. 299, y_t = 1 for x_t < min_dist, else exp(-(x_t - min_dist) / spread); least squares of 1 / (1 + a x^(2b)) by
 *      Gauss-Newton / Levenberg-Marquardt in f64 from (1, 1) until the step is below 1e-12 relative (sapca_umap_find_ab).
 *   5. Layout: optimize_layout_euclidean made synchronous and deterministic.  w_max = the largest stored value.  A directed
 *      stored entry e = (i -> j, w_e) with w_e < w_max / n_epochs is left out of the layout (not of the graph).
 *      eps_e = w_max / w_e (f64, from the stored T values), next_e = eps_e, epsn_e = eps_e / negative_sample_rate,
 *      nextn_e = epsn_e.  Epoch n = 0 .. n_epochs - 1, alpha = learning_rate (1 - n / n_epochs): every vertex i reads the
 *      previous epoch's Y only and only y_i is written by it (two buffers, no floating-point atomic).  For each of its
 *      entries with next_e <= n: attraction, delta = y_i - y_j, s = |delta|^2, c = s > 0 ? -2 a b s^(b-1) / (a s^b + 1) : 0,
 *      add clip(c delta, -4, 4) componentwise, next_e += eps_e; repulsion, q = floor((n - nextn_e) / epsn_e), for
 *      p = 0 .. q - 1: k = floor(hash_u01(seed, 32, (n nnz + e) 64 + p) m) with e the entry's position in the stored graph,
 *      delta = y_i - y_k, s = |delta|^2, c = s > 0 ? 2 repulsion_strength b / ((0.001 + s)(a s^b + 1)) : 0, add
 *      clip(c delta, -4, 4); nextn_e += q epsn_e (negative_sample_rate = 0: no repulsion).  Then y_i <- y_i + alpha (sum):
 *      everything in f64 from the stored T values, rounded once per epoch to T, the sum added in an order fixed by the graph
 *      alone; a vertex whose sum is exactly 0 keeps its bits.  The graph is symmetric and both directions are stored with the
 *      same weight, so head-only moves act on both ends of an edge in the same epochs.  q <= 2 negative_sample_rate (from
 *      eps >= 1); the rate is limited to 31, so p < 64.  A sample k == i gives s = 0 and no force.
 *      Start: SAPCA_UMAP_INIT_PANEL (default) y[:, c] = 10 (x[:, c] - min_c) / (max_c - min_c) for the first output_dim
 *      columns of x, a constant column giving 0 (needs d >= output_dim); SAPCA_UMAP_INIT_RANDOM
 *      10 hash_u01(seed, 31, i output_dim + c); SAPCA_UMAP_INIT_GIVEN the caller's panel as it is.
 * Deviations from umap-learn: synchronous instead of sequential in-place updates; this library's counter generator instead of
 * tau_rand; no spectral initialisation (a start can be computed by sapca_umap_spectral_init_device_*, below, and given as
 * SAPCA_UMAP_INIT_GIVEN); set_op_mix_ratio = 1 and local_connectivity = 1 only; Euclidean only; no transform of
 * new points.
 * Deterministic: the same bytes from call to call.  Integer atomics count and hand out positions in stage 3 and take the
 * maximum of bit patterns for w_max; the rows are then sorted by column and a pair combined symmetrically, so no order reaches
 * a value; every floating-point sum that crosses lanes is added in an order fixed by the shape or the graph, never by the device.
 * Outputs are complete when the call returns.  Every call runs on the handle's stream in buffers of its own: a fitted model,
 * a cached preparation, the upload's statistics, the selection, the canonical, the t-SNE and the k-means buffers are
 * untouched; on a handle that belongs to a communicator the call is local to the rank and issues no collective.  The epoch
 * loop enqueues kernels only and swaps the two buffers; nothing is read back.  No index outside the arrays is touched: a
 * neighbour slot or a column of G outside [0, m) is skipped where it is read, a sample is below m, the emitted positions are
 * counted before they are written, and the offsets of a caller's G are trusted as in every *_csr_device_* call.  Non-finite
 * input values give an unspecified embedding.
 * SAPCA_ERR_ARG, checked on the host before anything is enqueued (the handle stays usable), each with a message that names
 * the offending number: a wrong struct_size; output_dim outside 1 .. 3; an unknown init; n_neighbors outside 2 .. 129;
 * n_neighbors > m when m > 0; negative_sample_rate > 31; K outside 1 .. 128 or n_neighbors < 2 in the graph call; a non-finite
 * or negative learning_rate / repulsion_strength (0 is valid); exactly one of a, b zero, or either negative or non-finite;
 * the refusals of sapca_umap_find_ab; INIT_PANEL with d < output_dim, or passed to the embed stage; the d / stride limits of
 * sapca_knn_device_*; m >= 2^31; a non-square graph; a null pointer with a non-empty shape.  m == 0 is valid and writes
 * nothing.                                                                                                                */
typedef enum sapca_umap_init { SAPCA_UMAP_INIT_PANEL = 0, SAPCA_UMAP_INIT_RANDOM = 1, SAPCA_UMAP_INIT_GIVEN = 2 } sapca_umap_init;
typedef struct sapca_umap_options {
  uint32_t struct_size;            /* sizeof(sapca_umap_options): 80                                   */
  uint32_t random_seed;            /* default 42                                                       */
  uint32_t output_dim;             /* default 2; 1 .. 3                                                */
  uint32_t init;                   /* sapca_umap_init, default SAPCA_UMAP_INIT_PANEL                   */
  uint32_t n_neighbors;            /* default 15; 2 .. 129 (counts the point itself)                   */
  uint32_t negative_sample_rate;   /* default 5; 0 .. 31                                               */
  uint64_t epochs;                 /* 0 (default): umap-learn's rule, 500 for m <= 10000, else 200     */
  double min_dist;                 /* default 0.1                                                      */
  double spread;                   /* default 1.0                                                      */
  double a;                        /* default 0: fitted from (spread, min_dist) together with b        */
  double b;                        /* default 0                                                        */
  double learning_rate;            /* default 1.0                                                      */
  double repulsion_strength;       /* default 1.0                                                      */
} sapca_umap_options;
void sapca_umap_options_default(sapca_umap_options* opts);
/* Stage 4 alone: pure host code, no handle.  SAPCA_ERR_ARG for non-finite arguments, spread <= 0, min_dist < 0 or
 * min_dist >= 3 spread; SAPCA_ERR_SVD if the fit does not converge in 200 steps.                                           */
sapca_status sapca_umap_find_ab(double spread, double min_dist, double* a, double* b);
/* Stages 2-3 on neighbour lists laid out as sapca_knn_device_* writes them (m x K, DEVICE; 1 <= K <= SAPCA_KNN_MAX_NEIGHBORS).
 * The graph comes back in handle-owned DEVICE arrays like the t-SNE affinities': valid until the next graph call
 * (sapca_umap_device_* and sapca_umap_* make one) or destroy, and accepted by every *_csr_device_* entry point.  d_sigma and
 * d_rho (m f64 each, DEVICE, may be NULL) receive sigma_i and rho_i.                                                        */
sapca_status sapca_umap_graph_device_f32(sapca_handle h, uint64_t m, const int32_t* d_indices, const float* d_dist, uint32_t K,
                                         uint32_t n_neighbors, uint64_t* nnz_out, const int64_t** d_row_offsets,
                                         const int32_t** d_col_indices, float** d_values, double* d_sigma, double* d_rho);
sapca_status sapca_umap_graph_device_f64(sapca_handle h, uint64_t m, const int32_t* d_indices, const double* d_dist, uint32_t K,
                                         uint32_t n_neighbors, uint64_t* nnz_out, const int64_t** d_row_offsets,
                                         const int32_t** d_col_indices, double** d_values, double* d_sigma, double* d_rho);
/* Stage 5 on a given symmetric graph: d_y (m x output_dim packed, DEVICE) is read for SAPCA_UMAP_INIT_GIVEN and receives the
 * embedding.  SAPCA_UMAP_INIT_PANEL is refused here (there is no panel); n_neighbors is not read.                           */
sapca_status sapca_umap_embed_device_f32(sapca_handle h, uint64_t m, uint64_t nnz, const int64_t* row_offsets, const int32_t* col_indices,
                                         const float* values, const sapca_umap_options* opts, float* d_y);
sapca_status sapca_umap_embed_device_f64(sapca_handle h, uint64_t m, uint64_t nnz, const int64_t* row_offsets, const int32_t* col_indices,
                                         const double* values, const sapca_umap_options* opts, double* d_y);
/* Stages 1-5 on a resident m x d panel with row stride ldx: exactly sapca_knn_device_* (EUCLIDEAN, EXCLUDE_SELF,
 * n_neighbors - 1), sapca_umap_graph_device_*, then the layout.                                                              */
sapca_status sapca_umap_device_f32(sapca_handle h, uint64_t m, const float* d_x, uint64_t ldx, uint64_t d,
                                   const sapca_umap_options* opts, float* d_y);
sapca_status sapca_umap_device_f64(sapca_handle h, uint64_t m, const double* d_x, uint64_t ldx, uint64_t d,
                                   const sapca_umap_options* opts, double* d_y);
/* The same with HOST arrays in and out (x: m x d row-major; y: m x output_dim, read for SAPCA_UMAP_INIT_GIVEN).             */
sapca_status sapca_umap_f32(sapca_handle h, uint64_t m, uint64_t d, const float* x, const sapca_umap_options* opts, float* y);
sapca_status sapca_umap_f64(sapca_handle h, uint64_t m, uint64_t d, const double* x, const sapca_umap_options* opts, double* y);

/* ---- Louvain clustering of a resident graph (sapca_louvain_*): an opt-in superset, the reference has no graph clustering ----
 * The step scanpy runs after `neighbors`: communities of the symmetric graph sapca_umap_graph_device_* leaves in the handle (its
 * `connectivities`), without the graph leaving the device.  Sequential Louvain cannot be restated on a GPU bit for bit and a
 * naive synchronous sweep oscillates, so the local moving is restated as hashed half-active sweeps with anchored targets;
 * tests/louvain_ref.py says the same in numpy and is held to networkx's louvain_communities / modularity.
 * Input: an m x m CSR, int64 offsets, int32 columns, values of type T, symmetric and canonical with finite weights >= 0.  A
 * stored diagonal entry is A_ii.  Symmetry is trusted, as the offsets are.  All arithmetic is f64 from the stored T values,
 * products and sums as written, no contraction.
 * Per level (graph A with n vertices; level 0 is the input): k_i = sum_j A_ij, S = sum_i k_i, tot_C = sum_{c_i = C} k_i,
 *   Q(c) = (sum_i s_i) / S - gamma sum_C (tot_C / S)^2,  s_i = sum_{j: c_j = c_i} A_ij (diagonal included).
 * Orders of the sums: a row's k_i and s_i by 64 lanes (lane l adds the entries l, l + 64, .. in stored order) that meet in a
 * butterfly; tot_C over C's members in ascending vertex order; the sums over all vertices / communities (S, sum s_i,
 * sum (tot_C / S)^2) in an order fixed by n; a weight w_iD over the row's entries in stored order.  No floating-point atomic.
 * If S == 0: every vertex is its own community, Q = 0, n_levels = 0.
 * Start: c_i = i, Q = Q(c), misses = 0.  Sweep t = 0, 1, ..:
 *   u_i = hash_u01(seed, 41, ((level 4096 + t) << 32) + i); vertex i is active iff u_i < 0.5; community C is anchored iff some
 *   inactive vertex has c_i = C.  Each active i, with C = c_i, computes from the assignment at the start of the sweep only:
 *   r_i = (gamma k_i) / S; w_iD = sum_{j != i, c_j = D} A_ij; g_C = w_iC - r_i (tot_C - k_i); for every anchored D != C that holds
 *   at least one entry j != i of the row, g_D = w_iD - r_i tot_D.  i moves to the D of largest g_D if g_D > g_C strictly, ties
 *   among D going to the lowest label; otherwise it stays.  Inactive vertices stay: no community that is joined in a sweep can
 *   empty in that sweep.
 *   Keep or undo: no vertex moved: a miss.  Otherwise Q' = Q(c'); Q' > Q + tol: c = c', Q = Q', misses = 0; else a miss and c
 *   is unchanged.  The level ends at 4 consecutive misses or at t = max_sweeps.
 * Between levels: a level that kept no sweep ends the run.  Otherwise communities are renumbered 0 .. n' - 1 in ascending order
 * of label, the labels composed with the earlier levels', and the next graph is A'_CD = sum_{i in C, j in D} A_ij (C == D
 * included; f64; canonical CSR), added first within each row i over its entries in stored order, then over the members i of C
 * in ascending vertex order.  The run also ends at n' == 1 or after max_levels levels.
 * Outputs: labels (m int32 in [0, n_communities)), n_communities, the last kept Q (the start's Q where nothing was kept) and
 * n_levels, the levels that kept a sweep.
 * Deterministic: the same bytes from call to call.  Within a level the loop enqueues kernels only; keep / undo is a word of a
 * device control block that says which of two label generations is current, a device flag turns the sweeps enqueued behind
 * the level's end into no-ops, and the host peeks at it every 8 sweeps, so nothing depends on when it looks.  Between levels the
 * host reads back counts (rows per length class, n', the entries of the coarse graph) to size buffers and launches.  No kernel
 * waits for another workgroup.  Integer atomics count moved vertices and hand out list slots whose order reaches no value.
 * No address outside the arrays is touched: a column or a label outside [0, m) is skipped where it is read; such a vertex is
 * inactive, anchors nothing and its label is copied through (the aggregation leaves it out).  Non-finite or negative weights
 * or an asymmetric graph give unspecified labels inside their range; the call still terminates.
 * All work is in buffers of the handle's own, distinct from the upload's, the selection's, the canonical form's, t-SNE's,
 * k-means' and the UMAP graph's, which stay valid and untouched.  On a handle that belongs to a communicator the calls are
 * local and issue no collective.
 * SAPCA_ERR_ARG, checked on the host before anything is enqueued (the handle stays usable), each with a message that names the
 * offending number: a wrong struct_size; resolution or tol negative or non-finite; max_sweeps outside 1 .. 4096; max_levels
 * above 64; level >= 2^20 or sweep >= 4096 in the sweep call; m >= 2^31; a null pointer with a non-empty shape.  (The entry
 * points take one dimension: a non-square graph cannot be passed.)  m == 0 is valid and writes nothing.                      */
typedef struct sapca_louvain_options {
  uint32_t struct_size;   /* sizeof(sapca_louvain_options): 32                */
  uint32_t random_seed;   /* default 42                                       */
  uint32_t max_levels;    /* default 0: 32; at most 64                        */
  uint32_t max_sweeps;    /* default 256; 1 .. 4096                           */
  double resolution;      /* gamma, default 1.0                               */
  double tol;             /* default 1e-7 (networkx's threshold)              */
} sapca_louvain_options;
void sapca_louvain_options_default(sapca_louvain_options* opts);
/* *modularity = Q(d_labels) at the given resolution (d_labels: m int32, DEVICE): on its own it scores any labels, k-means' for
 * instance, on the graph.                                                                                                   */
sapca_status sapca_louvain_modularity_device_f32(sapca_handle h, uint64_t m, uint64_t nnz, const int64_t* row_offsets,
                                                 const int32_t* col_indices, const float* values, const int32_t* d_labels,
                                                 double resolution, double* modularity);
sapca_status sapca_louvain_modularity_device_f64(sapca_handle h, uint64_t m, uint64_t nnz, const int64_t* row_offsets,
                                                 const int32_t* col_indices, const double* values, const int32_t* d_labels,
                                                 double resolution, double* modularity);
/* One sweep (no keep / undo) from d_labels_in into d_labels_out (m int32 each, DEVICE, distinct); *n_moved = the vertices that
 * moved.                                                                                                                    */
sapca_status sapca_louvain_sweep_device_f32(sapca_handle h, uint64_t m, uint64_t nnz, const int64_t* row_offsets,
                                            const int32_t* col_indices, const float* values, const int32_t* d_labels_in, uint32_t seed,
                                            uint32_t level, uint32_t sweep, double resolution, int32_t* d_labels_out, uint64_t* n_moved);
sapca_status sapca_louvain_sweep_device_f64(sapca_handle h, uint64_t m, uint64_t nnz, const int64_t* row_offsets,
                                            const int32_t* col_indices, const double* values, const int32_t* d_labels_in, uint32_t seed,
                                            uint32_t level, uint32_t sweep, double resolution, int32_t* d_labels_out, uint64_t* n_moved);
/* The coarse graph of d_labels: *n_out communities, *nnz_out entries, in handle-owned DEVICE arrays with f64 values in both
 * variants (it feeds the _f64 stage calls), valid until the next Louvain call.  d_renumbered (m int32, DEVICE, may be NULL)
 * receives every vertex's renumbered label.                                                                                 */
sapca_status sapca_louvain_aggregate_device_f32(sapca_handle h, uint64_t m, uint64_t nnz, const int64_t* row_offsets,
                                                const int32_t* col_indices, const float* values, const int32_t* d_labels, uint64_t* n_out,
                                                uint64_t* nnz_out, const int64_t** d_row_offsets, const int32_t** d_col_indices,
                                                double** d_values, int32_t* d_renumbered);
sapca_status sapca_louvain_aggregate_device_f64(sapca_handle h, uint64_t m, uint64_t nnz, const int64_t* row_offsets,
                                                const int32_t* col_indices, const double* values, const int32_t* d_labels, uint64_t* n_out,
                                                uint64_t* nnz_out, const int64_t** d_row_offsets, const int32_t** d_col_indices,
                                                double** d_values, int32_t* d_renumbered);
/* The whole run on a resident graph: d_labels (m int32, DEVICE) out; n_communities, modularity, n_levels may be NULL.       */
sapca_status sapca_louvain_device_f32(sapca_handle h, uint64_t m, uint64_t nnz, const int64_t* row_offsets, const int32_t* col_indices,
                                      const float* values, const sapca_louvain_options* opts, int32_t* d_labels, uint64_t* n_communities,
                                      double* modularity, uint32_t* n_levels);
sapca_status sapca_louvain_device_f64(sapca_handle h, uint64_t m, uint64_t nnz, const int64_t* row_offsets, const int32_t* col_indices,
                                      const double* values, const sapca_louvain_options* opts, int32_t* d_labels, uint64_t* n_communities,
                                      double* modularity, uint32_t* n_levels);
/* The same with a HOST CSR in (int64 offsets, int32 columns, as on the device) and HOST labels out.                         */
sapca_status sapca_louvain_f32(sapca_handle h, uint64_t m, uint64_t nnz, const int64_t* row_offsets, const int32_t* col_indices,
                               const float* values, const sapca_louvain_options* opts, int32_t* labels, uint64_t* n_communities,
                               double* modularity, uint32_t* n_levels);
sapca_status sapca_louvain_f64(sapca_handle h, uint64_t m, uint64_t nnz, const int64_t* row_offsets, const int32_t* col_indices,
                               const double* values, const sapca_louvain_options* opts, int32_t* labels, uint64_t* n_communities,
                               double* modularity, uint32_t* n_levels);

/* ---- Spectral embedding and diffusion maps of a resident graph (sapca_spectral_*, sapca_graph_components_device): an opt-in
 * superset, the reference has no counterpart ----
 * The leading eigenpairs of S = diag(s) W diag(s) for a symmetric graph W with weights >= 0 (the graph
 * sapca_umap_graph_device_* leaves in the handle, or any m x m CSR with int64 offsets, int32 columns and values of type T):
 * what umap-learn's spectral_layout / scikit-learn's spectral_embedding (NORMALIZED) and scanpy's tl.diffmap (DIFFMAP) compute.
 * tests/spectral_ref.py says the same in numpy and is held to scipy's laplacian, eigsh and connected_components and to
 * scikit-learn's spectral_embedding.  Symmetry is trusted, as the offsets are.  All arithmetic is f64 from the stored T values.
 *   1. Components (sapca_graph_components_device): structure only, every stored entry is an edge, values are not read.
 *      parent_i = i; a round hooks, for every stored (i, j), the larger of the two roots onto the smaller with an integer
 *      atomicMin, then shortens every chain to its root (pointer jumping); rounds repeat until one changes nothing (the host
 *      peeks at a device word between rounds).  parent never exceeds its index, so the fixed point is the smallest vertex of
 *      the component whatever the order: deterministic.  d_labels[i] = the number of roots below parent_i (a prefix count):
 *      components numbered in ascending order of their smallest vertex, as scipy's connected_components(directed=False) does.
 *   2. Scale (sapca_spectral_scale_device_*): a row's sums by a lane group of g lanes (g from the mean row length: the smallest
 *      of 8, 16, 32, 64 that is not below it), lane l adds the entries l, l + g, .. in stored order, alternating between two
 *      partial sums that are added at the end, and the lanes meet in a butterfly: an order fixed by the row's length and g.
 *      SAPCA_SPECTRAL_NORMALIZED: d_i = sum_j W_ij, s_i = 1 / sqrt(d_i): S = D^-1/2 W D^-1/2 = I - L_sym.
 *      SAPCA_SPECTRAL_DIFFMAP: q_i = sum_j W_ij, z_i = sum_j W_ij / (q_i q_j), s_i = 1 / (q_i sqrt(z_i)): S is scanpy's
 *      density-normalised symmetric transition matrix (compute_transitions(density_normalize=True)).
 *      A row whose sum (d_i; q_i or z_i) is not finite and positive has s_i = 0: the vertex drops out of the operator.
 *   3. Operator (sapca_spectral_apply_device_*): Wt_ij = W_ij (s_i s_j) as one f64 copy (the product s_i s_j commutes, so Wt is
 *      symmetric bit for bit), y_i = sum_j Wt_ij x_j by the lane groups of stage 2 with fma in place of the addition.  The
 *      eigen-solve builds the copy once, the stage call per call.  The step of the eigen-solve multiplies the same copy with
 *      the wave-per-row product of the Lanczos SVD (64 lanes to a row, four partial sums a lane, a 64-lane butterfly; for
 *      4096 <= m <= 19200 the same with x staged in LDS): measured on a 200 000-row neighbour graph it is the faster of the
 *      two, and its order is as fixed.  That product does not look at its columns, so the solve hands it a copy of the
 *      columns in which one outside [0, m) is replaced by the row's own number, with the value 0: such an entry adds 0 x_i.
 *   4. Locked pairs.  With t_i = 1 / s_i (= sqrt(d_i)) for NORMALIZED and t_i = 1 / (s_i q_i) (= sqrt(z_i)) for DIFFMAP, and
 *      t_i = 0 where s_i = 0: every component C with a vertex of t_i > 0 has the eigenvalue 1 with the eigenvector
 *      u_C = t 1_C / |t 1_C|.  (1 / s is that vector for NORMALIZED only: S (q sqrt(z)) = 1 / sqrt(z).)  t and the norm (summed
 *      in ascending vertex order) are computed on the host from one read-back of s, q and the labels.  The locked pairs come
 *      first, in label order.  With at least n_eigen of them the first n_eigen are the result and n_steps = 0.
 *   5. Otherwise a single-vector Lanczos iteration on S in the orthogonal complement of the c locked vectors: start vector
 *      gaussian_panel (m x 1) under random_seed; every new vector (the start included) goes through classical Gram-Schmidt
 *      twice against the locked vectors and the whole Lanczos basis, with the fixed-order kernels of the Lanczos SVD; alpha_j
 *      and beta_j are those of the Lanczos part.  A run that wants p pairs: from step p on the host reads alpha and beta back
 *      (every step up to 64, then every 2nd, 4th, 8th as the Lanczos SVD does) and runs implicit QL with the bottom row: the
 *      run stops when the p largest (algebraic) Ritz values all have |beta_j s_ji| <= tol, or when the Krylov space is
 *      exhausted (beta_j <= 1e-13 times the largest |Ritz value|, or j = the dimension of the complement; before step p:
 *      beta_j <= 1e-13 (max_i |alpha_i| + 2 |beta_i|), looked at every step; with a locked pair |S| >= 1 and either scale is at
 *      least 1: in the null space of S the run's own values are rounding noise).  Every Ritz pair of an exhausted run is an
 *      eigenpair; it gives min(p, j) of them and no padded ones.  The one exception is a graph without weights (no vertex with
 *      s_i > 0, c = 0, S the zero matrix, of which every vector is an eigenvector): its single run is all there is, no round
 *      follows it, and exhausted in fewer than n_eigen steps it is SAPCA_ERR_SVD, "spectral: the Krylov space is exhausted
 *      after j steps, k pairs were to be iterated".
 *      Rounds.  The Krylov space of ONE start vector holds one vector per DISTINCT eigenvalue, and full re-orthogonalisation
 *      keeps the further copies of a repeated value (a ring, a grid, a lattice, a complete graph, a star, any graph with a
 *      symmetry) at rounding level: a single run returns each value once and fills up with smaller ones.  So the solve
 *      runs in rounds.  A round locks the Ritz vectors it accepted behind the analytic ones and the next round starts from
 *      gaussian_panel under random_seed + 0x9E3779B9 round (mod 2^32; round 0 is random_seed itself) in the complement of
 *      all of them.  While fewer than n_eigen - c pairs are held a round wants the missing ones (an exhausted run ends its
 *      round, it is no error).  Then a round wants 1 pair, the largest of the complement: if it exceeds the current
 *      (n_eigen - c)-th largest held value by more than tol it is a missed copy and is merged (held values are re-sorted,
 *      ties in the order found) and another round follows, at most n_eigen - c of them; if not, or if the complement is empty,
 *      the solve ends with the n_eigen - c largest held pairs.  On a graph whose leading values are simple the first round's
 *      pairs are the result, bit for bit what a single run gives, and the one closing round is the price of knowing it.
 *      single_round = 1 ends after the round that completes n_eigen - c pairs: the single run, for a caller who knows the
 *      leading values to be simple.  Values closer than tol are one value to the rule: their pairs come in either order.
 *      n_steps is the sum over the rounds.  A round that reaches max_steps: SAPCA_ERR_SVD, "spectral: Lanczos did not
 *      converge k of n pairs in j steps" while pairs are missing (k the missing ones, j the steps of all rounds so far),
 *      "spectral: the round that looks for a missed copy of a repeated eigenvalue did not converge in j steps (t in all)"
 *      afterwards.
 *   6. Output: eigenvalues descending (the locked 1.0s, then the Ritz values); eigenvectors m x n_eigen row-major.  Ritz
 *      vectors are combined on the device in f64, their sign fixed so that the entry of largest magnitude (lowest index on a
 *      tie) is positive, and rounded once to T; the locked vectors are positive already.  n_components counts every
 *      component, isolated vertices included.
 * Deviations: scanpy's eigsh(which="LM") would also admit values near -1; the largest algebraic ones are taken here.
 * Spectral start for UMAP (sapca_umap_spectral_init_device_*): from eigenvectors E (m x n_eigen, row stride ld, NORMALIZED),
 *   y[i][c] = 10 E[i][1 + c] / max|E[:, 1 .. output_dim]| + 1e-4 (2 hash_u01(seed, 51, i output_dim + c) - 1)
 * in f64 with every product, quotient and sum rounded as written, then rounded to T: umap-learn's expansion to +-10 with
 * uniform instead of Gaussian tie-breaking noise.  Pass it to the layout as SAPCA_UMAP_INIT_GIVEN; the layout itself still has
 * no spectral initialisation of its own.  On a disconnected graph the columns are component indicators; umap-learn's
 * per-component meta-layout is not built.  A maximum of 0 gives the noise alone.
 * Deterministic: the same bytes from call to call; no floating-point atomic.  Outputs are complete when the call returns.
 * All work is in buffers of the handle's own: the UMAP graph, Louvain's buffers, the upload, a fitted model and a cached
 * preparation stay valid and untouched; on a handle that belongs to a communicator the calls are local and issue no
 * collective.  A column outside [0, m) is skipped where it is read.  Negative or non-finite weights or an asymmetric graph
 * give unspecified numbers; every round still terminates at max_steps.  The Lanczos basis takes (2 n_eigen - c + max_steps + 1) m
 * doubles (the locked vectors, up to 2 (n_eigen - c) held Ritz vectors, a round's basis);
 * one that cannot be allocated is SAPCA_ERR_NOMEM.
 * SAPCA_ERR_ARG, checked on the host before anything is enqueued (the handle stays usable), each with a message that names the
 * offending number: a wrong struct_size; an unknown kind; n_eigen outside 1 .. 64 or above m; max_steps above 4096; tol
 * negative or non-finite; m >= 2^31; output_dim outside 1 .. 3 or n_eigen <= output_dim or ld < n_eigen in the start; a null
 * pointer with a non-empty shape.  m == 0 is valid and writes nothing.                                                       */
typedef enum sapca_spectral_kind { SAPCA_SPECTRAL_NORMALIZED = 0, SAPCA_SPECTRAL_DIFFMAP = 1 } sapca_spectral_kind;
typedef struct sapca_spectral_options {
  uint32_t struct_size;   /* sizeof(sapca_spectral_options): 32               */
  uint32_t random_seed;   /* default 42                                       */
  uint32_t kind;          /* sapca_spectral_kind, default NORMALIZED          */
  uint32_t n_eigen;       /* default 16; 1 .. 64 and <= m                     */
  uint32_t max_steps;     /* default 0: min(m, 1000); at most 4096            */
  uint32_t single_round;  /* default 0: rounds until no copy is missed; 1: one */
  double tol;             /* default 1e-8                                     */
} sapca_spectral_options;
void sapca_spectral_options_default(sapca_spectral_options* opts);
/* Stage 1: d_labels (m int32, DEVICE) out; n_components may be NULL.                                                         */
sapca_status sapca_graph_components_device(sapca_handle h, uint64_t m, uint64_t nnz, const int64_t* row_offsets,
                                           const int32_t* col_indices, int32_t* d_labels, uint64_t* n_components);
/* Stage 2: d_scale (m f64, DEVICE) receives s.                                                                               */
sapca_status sapca_spectral_scale_device_f32(sapca_handle h, uint64_t m, uint64_t nnz, const int64_t* row_offsets,
                                             const int32_t* col_indices, const float* values, uint32_t kind, double* d_scale);
sapca_status sapca_spectral_scale_device_f64(sapca_handle h, uint64_t m, uint64_t nnz, const int64_t* row_offsets,
                                             const int32_t* col_indices, const double* values, uint32_t kind, double* d_scale);
/* Stage 3: d_y = S d_x (m f64 each, DEVICE, distinct).                                                                       */
sapca_status sapca_spectral_apply_device_f32(sapca_handle h, uint64_t m, uint64_t nnz, const int64_t* row_offsets,
                                             const int32_t* col_indices, const float* values, uint32_t kind, const double* d_x,
                                             double* d_y);
sapca_status sapca_spectral_apply_device_f64(sapca_handle h, uint64_t m, uint64_t nnz, const int64_t* row_offsets,
                                             const int32_t* col_indices, const double* values, uint32_t kind, const double* d_x,
                                             double* d_y);
/* The whole solve on a resident graph: evals (n_eigen f64, HOST), d_evecs (m x n_eigen row-major, DEVICE); n_components and
 * n_steps may be NULL.                                                                                                       */
sapca_status sapca_spectral_device_f32(sapca_handle h, uint64_t m, uint64_t nnz, const int64_t* row_offsets, const int32_t* col_indices,
                                       const float* values, const sapca_spectral_options* opts, double* evals, float* d_evecs,
                                       uint64_t* n_components, uint32_t* n_steps);
sapca_status sapca_spectral_device_f64(sapca_handle h, uint64_t m, uint64_t nnz, const int64_t* row_offsets, const int32_t* col_indices,
                                       const double* values, const sapca_spectral_options* opts, double* evals, double* d_evecs,
                                       uint64_t* n_components, uint32_t* n_steps);
/* The same with a HOST CSR in (int64 offsets, int32 columns, as on the device) and HOST eigenvectors out.                    */
sapca_status sapca_spectral_f32(sapca_handle h, uint64_t m, uint64_t nnz, const int64_t* row_offsets, const int32_t* col_indices,
                                const float* values, const sapca_spectral_options* opts, double* evals, float* evecs,
                                uint64_t* n_components, uint32_t* n_steps);
sapca_status sapca_spectral_f64(sapca_handle h, uint64_t m, uint64_t nnz, const int64_t* row_offsets, const int32_t* col_indices,
                                const double* values, const sapca_spectral_options* opts, double* evals, double* evecs,
                                uint64_t* n_components, uint32_t* n_steps);
/* The spectral start: d_evecs (m rows of stride ld, DEVICE) in, d_y (m x output_dim packed, DEVICE) out.                     */
sapca_status sapca_umap_spectral_init_device_f32(sapca_handle h, uint64_t m, uint32_t output_dim, const float* d_evecs, uint64_t ld,
                                                 uint32_t n_eigen, uint32_t seed, float* d_y);
sapca_status sapca_umap_spectral_init_device_f64(sapca_handle h, uint64_t m, uint32_t output_dim, const double* d_evecs, uint64_t ld,
                                                 uint32_t n_eigen, uint32_t seed, double* d_y);

/* ---- Rank groups: marker columns of a labelled resident CSR (sapca_rank_*): an opt-in superset, the reference has no counterpart ----
 * The step scanpy runs after clustering (rank_genes_groups with method "wilcoxon" or "t-test"): which columns (genes) set each
 * group of rows (cells) apart from the rest, with the labels and the matrix staying on the device.  tests/rank_groups_ref.py
 * says the same in numpy and is held to scipy's rankdata, mannwhitneyu and ttest_ind.
 * Input: a device-resident CSR A (m x n) from any *_csr_device_* source (uploaded, selected or canonical; a row holds a column
 * at most once), d_labels (m int32, DEVICE, as the k-means and Louvain device calls write them) and n_groups = K.  A row whose
 * label is outside [0, K) is excluded altogether: it is in no group and in no "rest", and is skipped where it is read, so a
 * subset is analysed without a selection.  M = the included rows, n_g = those of group g, r_g = M - n_g; group g is always
 * compared with the rest.
 * Ranks, per column j, over the M included rows: the stored entries with value == 0 (+0.0 or -0.0) and the implicit zeros form
 * one block of Z equal values; a = the stored values < 0 of included rows; values are ranked ascending from 1 and ties get
 * their average rank.  f32 subnormals are distinct values and are not flushed; -inf and +inf sort at the ends.  A NaN makes its
 * column's results unspecified; no address outside the arrays is touched.
 * Exact outputs (integers; no floating-point atomic, no order reaches a value):
 *   rank_sum2[g][j] = 2 * (sum of the ranks of group g's rows), int64 below M (M + 1): every non-zero entry of g adds the first
 *                     plus the last 1-based position of its tie run in the full order, the zeros add
 *                     (n_g - c_gj) ((a + 1) + (a + Z));
 *   nonzero[g][j]   = c_gj, the stored non-zero entries of group g in column j;
 *   group_rows[g]   = n_g;
 *   tie_sum[j]      = sum over the tie runs of t^3 - t, the zero block included, in f64: every term and the sum are integers
 *                     below 2^53 whenever M <= 208,063, so the value is exact there; beyond it is rounded, in an order fixed by
 *                     the column's content.
 * Wilcoxon z (scanpy's formula), R_g = rank_sum2 / 2:
 *   z = (R_g - n_g (M + 1) / 2) / sqrt(n_g r_g (M + 1) / 12 * T),  T = 1 - tie_sum / (M^3 - M) with tie_correct = 1, T = 1 with
 *   tie_correct = 0 (scanpy's default);  p = erfc(|z| / sqrt(2));  z = 0 and p = 1 where n_g = 0, r_g = 0 or the denominator is 0.
 * Welch t, with s and q the sum and the sum of squares of the group's stored entries (implicit zeros count in the denominators):
 *   mean_g = s_g / n_g;  var_g = max(0, (q_g - s_g^2 / n_g) / (n_g - 1)), 0 when n_g < 2;  the rest takes s_tot - s_g and
 *   q_tot - q_g over r_g rows, the totals being the sums over g = 0 .. K - 1 in that order, in f64;
 *   t = (mean_g - mean_r) / sqrt(var_g / n_g + var_r / r_g);  df = the Welch-Satterthwaite value
 *   (var_g / n_g + var_r / r_g)^2 / ((var_g / n_g)^2 / (n_g - 1) + (var_r / r_g)^2 / (r_g - 1));
 *   t = 0 and df = 0 where n_g = 0, r_g = 0 or the denominator is 0;  df = 0 where n_g < 2 or r_g < 2.
 *   No p-value for t is returned (it needs the incomplete beta function; the Python layer adds one through scipy).
 * How: group sizes with integer atomics; the matrix is transposed; per column the stored non-zero entries of included rows are
 * kept as (order-preserving unsigned key, label), sorted by key -- in a wave's LDS, in a workgroup's LDS, or for the longest
 * columns by a segmented radix sort in global scratch -- tie runs are found from the sorted keys, and every entry adds first +
 * last position to its group's 64-bit counter in LDS.  The moments come from the labelled statistics of
 * sapca_batch_stats_csr_device_* (s, and q = m2 + s^2 / c over the c stored entries), SAPCA_RANK_MAX_GROUPS codes at most.
 * The host finishes the formulas in f64 on K x n values.
 * Outputs are HOST arrays, code-major K x n like sapca_batch_stats_csr_device_* (group_rows: K; tie_sum: n); any may be NULL,
 * and only what a non-NULL output needs is computed: no rank pass runs when neither z_score nor z_pvalue is asked for, no
 * moment pass when none of mean, var, t_score, t_df is.  m == 0 or n == 0 is valid.
 * SAPCA_ERR_ARG, checked on the host before anything is enqueued (the handle stays usable), each with a message that names the
 * offending number: n_groups == 0 or above SAPCA_RANK_MAX_GROUPS; m >= 2^31; tie_correct outside {0, 1}; a null d_labels with
 * m > 0; and the view checks of the other resident operations (a null CSR array, n >= 2^31).
 * Like sapca_batch_stats_csr_device_* with grouped_axis 0 the call transposes into the buffers prepare() uses: a cached
 * preparation is dropped.  A fitted model, the selection, the canonical form and the k-means, UMAP and Louvain buffers are
 * untouched.  On a handle that belongs to a communicator the call is local to the rank's shard and issues no collective.
 * Deterministic: the same bytes from call to call.                                                                         */
#define SAPCA_RANK_MAX_GROUPS 1024
/* The stage-level operator with the exact quantities: group_rows (K), rank_sum2 (K x n), nonzero (K x n), tie_sum (n).      */
sapca_status sapca_rank_sums_csr_device_f32(sapca_handle h, uint64_t m, uint64_t n, uint64_t nnz, const int64_t* row_offsets,
                                            const int32_t* col_indices, const float* values, const int32_t* d_labels,
                                            uint32_t n_groups, uint64_t* group_rows, int64_t* rank_sum2, uint64_t* nonzero,
                                            double* tie_sum);
sapca_status sapca_rank_sums_csr_device_f64(sapca_handle h, uint64_t m, uint64_t n, uint64_t nnz, const int64_t* row_offsets,
                                            const int32_t* col_indices, const double* values, const int32_t* d_labels,
                                            uint32_t n_groups, uint64_t* group_rows, int64_t* rank_sum2, uint64_t* nonzero,
                                            double* tie_sum);
/* The scores of every group against the rest: group_rows (K); mean, var, nonzero, t_score, t_df, z_score, z_pvalue (K x n).  */
sapca_status sapca_rank_groups_csr_device_f32(sapca_handle h, uint64_t m, uint64_t n, uint64_t nnz, const int64_t* row_offsets,
                                              const int32_t* col_indices, const float* values, const int32_t* d_labels,
                                              uint32_t n_groups, int32_t tie_correct, uint64_t* group_rows, double* mean,
                                              double* var, uint64_t* nonzero, double* t_score, double* t_df, double* z_score,
                                              double* z_pvalue);
sapca_status sapca_rank_groups_csr_device_f64(sapca_handle h, uint64_t m, uint64_t n, uint64_t nnz, const int64_t* row_offsets,
                                              const int32_t* col_indices, const double* values, const int32_t* d_labels,
                                              uint32_t n_groups, int32_t tie_correct, uint64_t* group_rows, double* mean,
                                              double* var, uint64_t* nonzero, double* t_score, double* t_df, double* z_score,
                                              double* z_pvalue);

/* ---- Variable genes: feature selection on the resident CSR (sapca_hvg_*, sapca_loess_f64): an opt-in superset, the reference
 *      has no counterpart ----
 * scanpy's pp.highly_variable_genes between log1p and the fit, flavours "seurat_v3" (on counts) and "seurat" (on log1p data,
 * scanpy's default).  "cell_ranger", "seurat_v3_paper" and "pearson_residuals" are NOT provided.  The result's highly_variable
 * bytes feed sapca_set_mask and the col_mask of sapca_select_submatrix_csr_device_* unchanged.  tests/hvg_ref.py says
 * everything below in numpy.
 * Rows: d_batch (m int32, DEVICE, the convention of sapca_rank_groups_csr_device_*) labels the rows; NULL means one batch of
 * all rows.  A row whose label is outside [0, n_batches) is excluded altogether: its values are not read.
 *
 * 1. Transformed column moments, sapca_hvg_moments_csr_device_*: for every column j, over the stored entries x of the included
 *    rows (d_batch[r] == batch, every row when d_batch is NULL),
 *      sum[j] = sum f_j(x), sum_squared[j] = sum f_j(x)^2, in f64 whatever the matrix's type, with
 *      SAPCA_HVG_CLIP:  f_j(x) = min((double)x, clip[j])  (clip: HOST, n f64; scanpy clips in f64 after astype(float64)),
 *      SAPCA_HVG_EXPM1: f_j(x) = expm1((double)x);
 *      n_clipped[j] = the included stored entries with x > clip[j] (0 for EXPM1), exact.
 *    How: the matrix is transposed (stable: a column's entries in ascending row order); one wave per column sums every 64th
 *    entry per lane in stored order and folds the 64 partial sums by a fixed butterfly.  No floating-point atomic, no order
 *    reaches a value: the same bytes from call to call.  A sum of L terms is within (L / 64 + 7) ulp of the sum of their
 *    magnitudes of the exact sum.  A NaN or inf propagates as in an f64 sum.
 *    Every call of this stage transposes the matrix anew (about the cost of the plain column statistics; the pass itself is a
 *    small fraction of it): nothing is kept between calls.  A loop over K batches through this entry point pays K
 *    transpositions; the chain below transposes once for all its passes, so batched use belongs there.
 * 2. Local quadratic regression, sapca_loess_f64(h, n, x, y, span, fitted): HOST f64 arrays, the arithmetic on the device in
 *    f64.  It is the "direct" surface of Cleveland's loess with degree 2, tricube weights and the gaussian family.
 *    STATED DEVIATION: skmisc's default (surface="interpolate"), which scanpy calls, evaluates the fit at the vertices of a
 *    k-d tree and interpolates between them; this call fits at every point.  How far the two surfaces lie apart on real data
 *    has not been measured, so equality with scanpy's seurat_v3 is not claimed.  The fit at x_i:
 *      q = min(n, max(3, floor(span n + 1e-5)));  h = the q-th smallest |x_j - x_i|, j = i counted;
 *      w_j = (1 - (|x_j - x_i| / h)^3)^3 where |x_j - x_i| < h, else 0;  t_j = (x_j - x_i) / h;
 *      the weighted least squares of y on {1, t, t^2} (normal equations of the sums of w t^k, k = 0 .. 4, and w y t^k,
 *      k = 0 .. 2); fitted[i] = the intercept.  The degree follows the number of distinct x among the points with w > 0:
 *      three or more: quadratic; two: linear on {1, t}; one, or h == 0: the plain mean of y over ALL points with x_j == x_i.
 *    Non-finite x or y give unspecified values.  n == 0 is valid.
 * 3. The chain, sapca_hvg_csr_device_*.  N_b = the rows of batch b; per batch, from sums s and ss over its rows,
 *      mean = s / N_b,  var = (ss / N_b - mean^2) N_b / (N_b - 1)   (scanpy's ddof-1 variance).
 *    s and ss come from the moment kernel of 1. (untransformed), not from the exact accumulators of the masked statistics:
 *    exact on whole counts below 2^53, a plain f64 sum with the error bound of 1. otherwise.
 *    SAPCA_HVG_SEURAT_V3, per batch: loess of log10(var) on log10(mean) over the columns with var > 0, est = 0 elsewhere;
 *      reg_std = sqrt(10^est);  clip = reg_std sqrt(N_b) + mean;  s, ss = the CLIP moments;
 *      norm_var = (N_b mean^2 + ss - 2 s mean) / ((N_b - 1) reg_std^2).
 *      The loess and these n-sized steps run on the device; clip never visits the host.  Across batches (host arithmetic):
 *      the batch's rank of a column = its position in a stable descending sort of norm_var (ties, and NaN last, by column
 *      index); ranks >= n_top become NaN; rank = the median of the non-NaN ranks over the batches (NaN if none);
 *      n_batches_hv = how many there are; variances_norm = the mean of norm_var over the batches; means and variances are
 *      taken over all included rows; highly_variable = the first n_top columns of a stable sort by (rank ascending, NaN last;
 *      n_batches_hv descending; column index).  dispersions and dispersions_norm are written as NaN.
 *    SAPCA_HVG_SEURAT, per batch, host f64 arithmetic on n values behind the EXPM1 moments: mean == 0 becomes 1e-12;
 *      disp = var / mean, 0 becomes NaN; disp = ln(disp); mean = log1p(mean); n_bins equal-width bins of mean as
 *      pandas.cut(mean, bins = n_bins) makes them (edges min + i (max - min) / n_bins, the last one max, the lowest lowered by
 *      0.1 % of the range; right-closed; min == max: the range is widened by 0.1 % of |min| on both sides, by 0.001 when it
 *      is 0); per bin the mean and the ddof-1 standard deviation (two passes) of the non-NaN disp; a bin with fewer than two
 *      of them takes std = its mean and mean = 0;  dispersions_norm = (disp - bin mean) / bin std (IEEE: a bin whose std is 0
 *      gives +-inf or NaN).  Selection with n_top: cutoff = the n_top-th largest non-NaN dispersions_norm (the smallest when
 *      there are fewer; nothing is selected when there is none), selected where nan_to_num(dispersions_norm) >= cutoff
 *      (numpy's nan_to_num: NaN 0, +-inf +-DBL_MAX).  With n_top == 0: min_mean < mean < max_mean and
 *      min_disp < d < max_disp with d = dispersions_norm, NaN taken as 0.  With batches: means, dispersions and
 *      dispersions_norm are the means over the batches of the non-NaN values (NaN if none), n_batches_hv counts the batches
 *      that selected the column; with n_top the selection is the first n_top of a stable sort by (n_batches_hv descending,
 *      averaged dispersions_norm descending with NaN last, column index), else the four cutoffs on the averaged values.
 *      variances = the per-batch var of expm1(x) averaged likewise; variances_norm and rank are written as NaN; without
 *      batches n_batches_hv equals highly_variable.
 * Outputs of the chain are HOST arrays of length n, any may be NULL.  m == 0 writes zeros (NaN where the flavour writes NaN or
 * ranks) and selects nothing; n == 0 writes nothing.
 * SAPCA_ERR_ARG, raised on the host before the first pass over the matrix (the handle stays usable), each with a message that
 * names the offending number: an unknown flavor or transform; SAPCA_HVG_SEURAT_V3 with n_top == 0; n_top > n; span outside
 * (0, 1]; n_bins == 0; n_batches == 0, or above SAPCA_HVG_MAX_BATCHES with non-NULL labels; a batch with fewer than 2 included
 * rows (found from integer counts made on the device); m >= 2^31; a NULL clip for CLIP; a negative batch with labels; a wrong
 * struct_size; and the view checks of the other resident operations.
 * Handle state: like sapca_rank_groups_csr_device_* the matrix calls transpose into the buffers prepare() uses, so a cached
 * preparation is dropped.  A fitted model, a set mask, the selection, the canonical form and the k-means, UMAP, Louvain and
 * rank buffers are untouched; the work arrays are the handle's own.  sapca_loess_f64 touches none of this.  On a handle that
 * belongs to a communicator the calls are local to the rank's shard and issue no collective.                                */
#define SAPCA_HVG_MAX_BATCHES 1024
#define SAPCA_HVG_CLIP 0
#define SAPCA_HVG_EXPM1 1
#define SAPCA_HVG_SEURAT_V3 0
#define SAPCA_HVG_SEURAT 1
typedef struct sapca_hvg_options {
  uint32_t struct_size;   /* sizeof(sapca_hvg_options): 64                          */
  int32_t flavor;         /* SAPCA_HVG_SEURAT_V3 (default) or SAPCA_HVG_SEURAT       */
  uint64_t n_top;         /* default 2000; 0: the four cutoffs (SEURAT only)         */
  double span;            /* loess span, default 0.3; (0, 1]                         */
  uint32_t n_bins;        /* default 20                                             */
  uint32_t reserved;      /* 0                                                      */
  double min_mean;        /* default 0.0125                                         */
  double max_mean;        /* default 3                                              */
  double min_disp;        /* default 0.5                                            */
  double max_disp;        /* default +inf                                           */
} sapca_hvg_options;
void sapca_hvg_options_default(sapca_hvg_options* opts);
sapca_status sapca_hvg_moments_csr_device_f32(sapca_handle h, uint64_t m, uint64_t n, uint64_t nnz, const int64_t* row_offsets,
                                              const int32_t* col_indices, const float* values, const int32_t* d_batch, int32_t batch,
                                              int32_t transform, const double* clip, double* sum, double* sum_squared,
                                              uint64_t* n_clipped);
sapca_status sapca_hvg_moments_csr_device_f64(sapca_handle h, uint64_t m, uint64_t n, uint64_t nnz, const int64_t* row_offsets,
                                              const int32_t* col_indices, const double* values, const int32_t* d_batch, int32_t batch,
                                              int32_t transform, const double* clip, double* sum, double* sum_squared,
                                              uint64_t* n_clipped);
sapca_status sapca_loess_f64(sapca_handle h, uint64_t n, const double* x, const double* y, double span, double* fitted);
sapca_status sapca_hvg_csr_device_f32(sapca_handle h, uint64_t m, uint64_t n, uint64_t nnz, const int64_t* row_offsets,
                                      const int32_t* col_indices, const float* values, const int32_t* d_batch, uint32_t n_batches,
                                      const sapca_hvg_options* opts, double* means, double* variances, double* variances_norm,
                                      double* dispersions, double* dispersions_norm, double* rank, uint32_t* n_batches_hv,
                                      uint8_t* highly_variable);
sapca_status sapca_hvg_csr_device_f64(sapca_handle h, uint64_t m, uint64_t n, uint64_t nnz, const int64_t* row_offsets,
                                      const int32_t* col_indices, const double* values, const int32_t* d_batch, uint32_t n_batches,
                                      const sapca_hvg_options* opts, double* means, double* variances, double* variances_norm,
                                      double* dispersions, double* dispersions_norm, double* rank, uint32_t* n_batches_hv,
                                      uint8_t* highly_variable);

/* ---- Harmony: batch integration of device-resident score rows (sapca_harmony_*): an opt-in superset ----
 * The ninth consumer of the score rows, the step between the fit and the neighbour search on data of several samples:
 * Harmony (Korsunsky et al. 2019; scanpy.external.pp.harmony_integrate).  harmonypy is not available to this project: the
 * algorithm is stated here in full and pinned by a numpy restatement (tests/harmony_ref.py: dense one-hot designs and
 * numpy.linalg.solve) that is itself held to scikit-learn's Ridge and scipy's softmax (tests/test_harmony_cpu.py).
 * Inputs: Z, a row-major DEVICE panel, m x d, row stride ldz >= d (nothing beyond column d of a row is read); batch, m int32
 * DEVICE labels in [0, B); K = n_clusters; theta, sigma, lambda.  N_b = the rows of batch b, Pr_b = N_b / m.  Zc = the rows of
 * the current corrected panel scaled to unit L2 norm (the norm in f64; a row of norm 0 stays 0).
 *   1. Initialisation.  init = SAPCA_HARMONY_KMEANS: Y = the centroids of sapca_kmeans_device_* on Zc (n_clusters = K, the given
 *      seed, max_iter = 25, tol = 1e-4, init = PLUSPLUS); SAPCA_HARMONY_GIVEN: the caller's K x d centroids.  Then the rows of
 *      Y are scaled to unit norm, dist_ik = 2 (1 - <Zc_i, Y_k>), R_ik = exp(-(dist_ik - min_k dist_ik) / sigma) with every row
 *      of R divided by its sum, rs_k = sum_i R_ik, O_bk = sum_{i in b} R_ik, E_bk = Pr_b rs_k.  (harmonypy evaluates the
 *      objective here once; no test of item 4 can reach that value -- see there -- and it is not an output, so it is not formed.)
 *   2. One clustering pass.  Y = normalise_rows(R^T Zc); dist as in 1; S_ik = exp(-(dist_ik - min_k dist_ik) / sigma).  The
 *      update order of pass number c (counted over the whole call, from 0) is the rows sorted by
 *      (hash_u01(random_seed, 61, c m + i), i) -- the counter generator behind sapca_generate_omega_*, sapca.synth.hash_u01,
 *      on a stream of its own -- cut into n_blocks consecutive blocks as numpy.array_split cuts it (the first m mod n_blocks
 *      blocks get one more row; an empty block is a no-op).  For each block in turn: its rows are removed from rs and O (and
 *      hence from E = Pr rs^T); R_ik = S_ik ((E_bk + 1) / (O_bk + 1))^theta with b = batch_i, the row divided by its sum; the
 *      block is added back.  rs, O, E, the sums behind Y and every reduction are f64 whatever T is, in an order fixed by
 *      (m, K, B, n_blocks, seed); no floating-point atomic is used.  Zc, R and Y are stored in T; the inner products run on
 *      the f32 / f64 matrix cores, everything behind them (dist, the exponential, the penalty, the row sum) in f64, and R is
 *      rounded once.
 *   3. The objective after a pass, in f64, three terms: sum_ik R_ik dist_ik;  sigma sum_ik R_ik log R_ik (0 log 0 = 0);
 *      sigma theta sum_ik R_ik log((O_bk + 1) / (E_bk + 1)).  (dist is held in T between the pass and this sum.)
 *   4. cluster(): passes i = 0 .. max_iter_cluster - 1; after pass i > 3, with obj_j the objective after pass j of this call
 *      to cluster(): new = obj_{i-2} + obj_{i-1} + obj_i, old = obj_{i-3} + obj_{i-2} + obj_{i-1} (harmonypy's window-3 sums,
 *      which at i > 3 hold objectives of this call alone); stop when (old - new) / |old| < epsilon_cluster.  The host reads
 *      the three terms back once per pass.
 *   5. Correction (mixture-of-experts ridge), always from the ORIGINAL Z.  For every cluster k, with Phi~ the (B + 1) x m
 *      design (an intercept row over the one-hot batch rows): A_k = Phi~ diag(R_.k) Phi~^T + diag(0, lambda, .., lambda),
 *      W_k = A_k^-1 Phi~ diag(R_.k) Z, the intercept row of W_k set to 0, Zcorr -= diag(R_.k) Phi~^T W_k; Zc is recomputed from
 *      Zcorr.  A_k is an arrow matrix and the solve has a closed form, which is what runs: o_b = sum_{i in b} R_ik,
 *      t_b = sum_{i in b} R_ik z_i, c_b = o_b / (o_b + lambda), a = sum_b (1 - c_b) t_b / sum_b (1 - c_b) o_b,
 *      beta_b = (t_b - o_b a) / (o_b + lambda), Zcorr_i = z_i - sum_k R_ik beta_{k, batch_i}.  A cluster with rs_k = 0
 *      contributes nothing.  All in f64, rounded once to T.  The rows are sorted by (batch, row) with a stable radix sort once per
 *      call and every (cluster, batch) sum runs over fixed slices of the batch's list that are added in order.
 *   6. Outer loop: for it = 1 .. max_iter_harmony: cluster(); record its last objective and its passes; correct(); from the
 *      second iteration on stop (converged = 1) when (obj[it-2] - obj[it-1]) / |obj[it-2]| < epsilon_harmony.
 * DEVIATIONS from harmonypy: one batch variable, not several covariates; scalar theta / sigma / lambda; no tau discount; no
 * automatic lambda; the update order comes from this library's counter generator, not numpy's (results equal harmonypy's in
 * distribution, not bit for bit); the initial k-means is this library's, with one start.
 * Deterministic: the same bytes from call to call.  Outputs are complete when the call returns.  Every call runs on the
 * handle's stream in buffers of its own: a fitted model, a cached preparation, the selection and every other consumer's
 * buffers are untouched (init = KMEANS runs in the k-means buffers); on a handle that belongs to a communicator the call is
 * local to the rank and issues no collective.
 * SAPCA_ERR_ARG, checked before the algorithm starts (the handle stays usable), each with a message that names the offending
 * number: n_clusters == 0; n_clusters > m when m > 0 (the whole run); n_clusters > SAPCA_KMEANS_MAX_CLUSTERS; n_batches == 0
 * or > SAPCA_HARMONY_MAX_BATCHES; n_blocks == 0; max_iter_harmony == 0; max_iter_cluster == 0; sigma <= 0; lambda <= 0; theta < 0; any scalar not finite; an unknown init;
 * the d and stride limits of sapca_knn_device_* (d in 1 .. 1024, strides >= d and < 2^28); m >= 2^31; a null pointer with a
 * non-empty shape; a batch label outside [0, n_batches) -- found by the counting pass that produces N_b (an integer atomic
 * keeps the first offending row, one read-back), the message names that row.  m == 0 is valid and writes nothing (*n_iter =
 * 0, *converged = 0, objective terms 0).  A batch with no rows is valid.                                                  */
typedef enum sapca_harmony_init { SAPCA_HARMONY_KMEANS = 0, SAPCA_HARMONY_GIVEN = 1 } sapca_harmony_init;
#define SAPCA_HARMONY_MAX_BATCHES 1024
/* Item 2 alone, a stage-level operator: d_zc (m x d, DEVICE, unit rows, stride ldz), d_batch (m int32, DEVICE), d_y (K x d,
 * DEVICE, packed: written when recompute_centroids != 0, used as given -- scaled to unit norm by the caller -- otherwise),
 * d_r (m x K, DEVICE, packed, in/out).  pass_index is c of the update order.  On the HOST, any of which may be NULL: o
 * (n_batches x K f64), rs (K f64) after the pass and objective (the three terms of item 3).                                 */
sapca_status sapca_harmony_assign_device_f32(sapca_handle h, uint64_t m, const float* d_zc, uint64_t ldz, uint64_t d,
                                             const int32_t* d_batch, uint32_t n_batches, uint32_t n_clusters, float* d_y,
                                             int32_t recompute_centroids, float* d_r, double theta, double sigma, uint32_t n_blocks,
                                             uint32_t random_seed, uint64_t pass_index, double* o, double* rs, double* objective);
sapca_status sapca_harmony_assign_device_f64(sapca_handle h, uint64_t m, const double* d_zc, uint64_t ldz, uint64_t d,
                                             const int32_t* d_batch, uint32_t n_batches, uint32_t n_clusters, double* d_y,
                                             int32_t recompute_centroids, double* d_r, double theta, double sigma, uint32_t n_blocks,
                                             uint32_t random_seed, uint64_t pass_index, double* o, double* rs, double* objective);
/* d_y (K x d, DEVICE, packed) = normalise_rows(R^T Zc) alone; a cluster whose sum has norm 0 gets zeros.                    */
sapca_status sapca_harmony_centroids_device_f32(sapca_handle h, uint64_t m, const float* d_zc, uint64_t ldz, uint64_t d,
                                                uint32_t n_clusters, const float* d_r, float* d_y);
sapca_status sapca_harmony_centroids_device_f64(sapca_handle h, uint64_t m, const double* d_zc, uint64_t ldz, uint64_t d,
                                                uint32_t n_clusters, const double* d_r, double* d_y);
/* Item 5 alone: d_zcorr (m x d, DEVICE, stride ldc; may not overlap d_z) from d_z, d_r (m x K, packed) and d_batch; beta
 * (HOST, K x n_batches x d f64, may be NULL) receives the coefficients.                                                    */
sapca_status sapca_harmony_correct_device_f32(sapca_handle h, uint64_t m, const float* d_z, uint64_t ldz, uint64_t d,
                                              const int32_t* d_batch, uint32_t n_batches, uint32_t n_clusters, const float* d_r,
                                              double lambda, float* d_zcorr, uint64_t ldc, double* beta);
sapca_status sapca_harmony_correct_device_f64(sapca_handle h, uint64_t m, const double* d_z, uint64_t ldz, uint64_t d,
                                              const int32_t* d_batch, uint32_t n_batches, uint32_t n_clusters, const double* d_r,
                                              double lambda, double* d_zcorr, uint64_t ldc, double* beta);
/* Items 1-6 on resident panels.  d_y (K x d, DEVICE, packed) is read when init == SAPCA_HARMONY_GIVEN and receives the final
 * centroids; d_r (m x K, DEVICE, packed) may be NULL.  On the HOST, may be NULL: objectives and passes (max_iter_harmony
 * entries each: the last objective and the number of passes of every outer iteration; entries from *n_iter on are not
 * written), n_iter, converged.                                                                                             */
sapca_status sapca_harmony_device_f32(sapca_handle h, uint64_t m, const float* d_z, uint64_t ldz, uint64_t d, const int32_t* d_batch,
                                      uint32_t n_batches, uint32_t n_clusters, uint32_t init, double theta, double sigma,
                                      double lambda, uint32_t n_blocks, uint32_t max_iter_harmony, uint32_t max_iter_cluster,
                                      double epsilon_cluster, double epsilon_harmony, uint32_t random_seed, float* d_zcorr,
                                      uint64_t ldc, float* d_r, float* d_y, double* objectives, uint32_t* passes, uint32_t* n_iter,
                                      int32_t* converged);
sapca_status sapca_harmony_device_f64(sapca_handle h, uint64_t m, const double* d_z, uint64_t ldz, uint64_t d, const int32_t* d_batch,
                                      uint32_t n_batches, uint32_t n_clusters, uint32_t init, double theta, double sigma,
                                      double lambda, uint32_t n_blocks, uint32_t max_iter_harmony, uint32_t max_iter_cluster,
                                      double epsilon_cluster, double epsilon_harmony, uint32_t random_seed, double* d_zcorr,
                                      uint64_t ldc, double* d_r, double* d_y, double* objectives, uint32_t* passes, uint32_t* n_iter,
                                      int32_t* converged);
/* The same with HOST arrays in and out (z, zcorr: m x d packed; batch: m; r: m x K, may be NULL; y: K x d).                  */
sapca_status sapca_harmony_f32(sapca_handle h, uint64_t m, uint64_t d, const float* z, const int32_t* batch, uint32_t n_batches,
                               uint32_t n_clusters, uint32_t init, double theta, double sigma, double lambda, uint32_t n_blocks,
                               uint32_t max_iter_harmony, uint32_t max_iter_cluster, double epsilon_cluster, double epsilon_harmony,
                               uint32_t random_seed, float* zcorr, float* r, float* y, double* objectives, uint32_t* passes,
                               uint32_t* n_iter, int32_t* converged);
sapca_status sapca_harmony_f64(sapca_handle h, uint64_t m, uint64_t d, const double* z, const int32_t* batch, uint32_t n_batches,
                               uint32_t n_clusters, uint32_t init, double theta, double sigma, double lambda, uint32_t n_blocks,
                               uint32_t max_iter_harmony, uint32_t max_iter_cluster, double epsilon_cluster, double epsilon_harmony,
                               uint32_t random_seed, double* zcorr, double* r, double* y, double* objectives, uint32_t* passes,
                               uint32_t* n_iter, int32_t* converged);

/* Measurement support: the rate (GB/s, read + write counted) of a 16-byte-per-lane streaming copy of `bytes`
 * bytes on the handle's device, best of `reps` -- the HBM rate a kernel of this library can attain, reported by
 * bench.py beside the data-sheet peak.  Allocates and frees its two buffers.                       */
sapca_status sapca_measure_copy_gbs(sapca_handle h, uint64_t bytes, uint32_t reps, double* gbs);

/* ---- multi-GPU: one process per GPU, rows range-partitioned ---------------- */
/* nnz-balanced contiguous row ranges: bounds[0]=0 <= ... <= bounds[nparts]=m.  Pure host code. */
sapca_status sapca_partition_rows(uint64_t m, const uint64_t* row_offsets, uint32_t nparts, uint64_t* bounds);
/* Built-in collective = RCCL (resolved at run time from librccl.so.1).  Rank 0 creates the
 * 128-byte id and the host program distributes it (torch.distributed broadcast, MPI, a file).  */
/* 1 when librccl and its entry points resolve in this process: every rank checks this BEFORE the
 * collective ncclCommInitRank inside sapca_comm_init_rank, which must not fail on some ranks only. */
int sapca_comm_rccl_available(void);
sapca_status sapca_comm_unique_id(uint8_t id[128]);
sapca_status sapca_comm_init_rank(sapca_handle h, uint32_t nranks, uint32_t rank, const uint8_t id[128]);
/* Or bring your own all-reduce(sum) over all ranks: `buf` is a DEVICE pointer holding `count`
 * elements of dtype (0 = f32, 1 = f64), reduced in place, ordered on `stream` (hipStream_t).
 * Return 0 on success.                                                                        */
typedef int (*sapca_allreduce_fn)(void* ctx, void* buf, uint64_t count, int32_t dtype, void* stream);
sapca_status sapca_comm_set_callback(sapca_handle h, uint32_t nranks, uint32_t rank, sapca_allreduce_fn fn, void* ctx);
/* Invokes the handle's collective once on a caller buffer (plumbing self-test).               */
sapca_status sapca_comm_allreduce(sapca_handle h, void* buf, uint64_t count, int32_t dtype);
/* A rank that fails OUTSIDE a collective (out of memory, a HIP error, a refused argument) never
 * joins the collectives its peers are waiting in.  Under the built-in RCCL transport the way out
 * is ncclCommAbort: sapca_comm_abort ends every collective of THIS handle that is in flight or
 * still to come -- a fit blocked behind one returns SAPCA_ERR_COMM -- and may be called from any
 * thread while a fit of the handle is running.  sapca_multi_* does this for its members; in the
 * one-process-per-GPU deployment the HOST program must: when a rank's call fails, tell the peers
 * (its own control channel) and have each call sapca_comm_abort on its handle, or poll
 * sapca_comm_async_error (0 = healthy; otherwise RCCL's ncclResult_t, -1 after an abort) from a
 * watchdog thread.  The communicator is gone afterwards: sapca_comm_init_rank again.            */
sapca_status sapca_comm_abort(sapca_handle h);
sapca_status sapca_comm_async_error(sapca_handle h, int32_t* state);
/* 1 when collectives issued on the library's side stream have a lane of their own (a callback
 * transport, or RCCL with the duplicate communicator made by ncclCommSplit at init): the A^T
 * sweep of a row-sharded fit then runs in two pieces with the first piece's all-reduce behind
 * the second piece's sweep.  Every rank must see the same answer.                               */
int sapca_comm_has_side_lane(sapca_handle h);


/* ---- one handle, several GPUs, one calling thread (SURVEY.md §8b "Threading", §8e) ----------
 * The reference call is ONE fit_transform(&CsrMatrix) from one thread (sparse/mod.rs:355-358;
 * masked :616-619).  A sapca_multi owns one member handle per listed device; every call below
 * splits the HOST CsrMatrix into nnz-balanced contiguous row ranges (sapca_partition_rows),
 * runs the matching sapca_*_csr_* entry point on every shard from a host thread per device, and
 * blocks until all are done.  The members are the ranks of one communicator: RCCL between
 * distinct devices, an in-process all-reduce through page-locked host memory when a device is
 * listed more than once (a one-GPU box rehearsing the path) or librccl does not resolve.
 * A member that fails (out of memory, a refused shard, a HIP error) ends the call for all: the
 * peers' collectives are abandoned (in-process) or aborted (ncclCommAbort on every member's
 * communicators), every member returns, the call reports the first failure, and the next call
 * builds new communicators -- no call blocks on a peer that has left.
 * `out` (m x n_components, row-major, HOST) receives every shard's rows in place.  The fitted
 * state is replicated and bitwise identical on all members: read it from any member with the
 * sapca_get_* functions (sapca_multi_member(mh, 0)); sapca_set_omega_* must be applied to every
 * member.  A sapca_multi is not thread-safe for concurrent calls, like a handle.                */
typedef struct sapca_multi_s* sapca_multi;
sapca_status sapca_multi_create(const sapca_options* opts /* device_id and stream are ignored */,
                                const int32_t* device_ids, uint32_t n_devices, sapca_multi* out);
void sapca_multi_destroy(sapca_multi mh);
const char* sapca_multi_last_error(sapca_multi mh /* NULL: the last failed sapca_multi_create of this thread */);
uint32_t sapca_multi_n_devices(sapca_multi mh);
sapca_handle sapca_multi_member(sapca_multi mh, uint32_t i);
int sapca_multi_uses_rccl(sapca_multi mh);
sapca_status sapca_multi_set_mask(sapca_multi mh, const uint8_t* mask, size_t n);
sapca_status sapca_multi_fit_csr_f32(sapca_multi mh, uint64_t m, uint64_t n, uint64_t nnz,
                                     const uint64_t* row_offsets, const uint64_t* col_indices, const float* values);
sapca_status sapca_multi_fit_csr_f64(sapca_multi mh, uint64_t m, uint64_t n, uint64_t nnz,
                                     const uint64_t* row_offsets, const uint64_t* col_indices, const double* values);
sapca_status sapca_multi_transform_csr_f32(sapca_multi mh, uint64_t m, uint64_t n, uint64_t nnz,
                                           const uint64_t* row_offsets, const uint64_t* col_indices, const float* values, float* out);
sapca_status sapca_multi_transform_csr_f64(sapca_multi mh, uint64_t m, uint64_t n, uint64_t nnz,
                                           const uint64_t* row_offsets, const uint64_t* col_indices, const double* values, double* out);
sapca_status sapca_multi_fit_transform_csr_f32(sapca_multi mh, uint64_t m, uint64_t n, uint64_t nnz,
                                               const uint64_t* row_offsets, const uint64_t* col_indices, const float* values, float* out);
sapca_status sapca_multi_fit_transform_csr_f64(sapca_multi mh, uint64_t m, uint64_t n, uint64_t nnz,
                                               const uint64_t* row_offsets, const uint64_t* col_indices, const double* values, double* out);
/* Resident shards (SURVEY.md §8f-1 for several devices): sapca_multi_upload_csr_* partitions the HOST
 * CsrMatrix as above and uploads every shard to its device ONCE (the uploads run side by side, one
 * host thread per device); the *_resident calls then fit / project the uploaded shards without
 * touching PCIe for the matrix again -- repeated fits (another k, another mask, another seed)
 * skip the upload, which is where the wall-clock of a one-off call goes (10.8 GB of usize CSR at
 * BASELINE configs[3]).  `out` is HOST memory, m x n_components, as above.  The shards stay valid
 * until the next sapca_multi_upload_csr_* / non-resident call on this sapca_multi.
 * sapca_multi_resident_shard: the row range and the device arrays of member i's shard (for
 * callers that preprocess in HBM with sapca_normalize_csr_device_* / sapca_log1p_csr_device_* on
 * sapca_multi_member(mh, i)); any output may be NULL.                                           */
sapca_status sapca_multi_upload_csr_f32(sapca_multi mh, uint64_t m, uint64_t n, uint64_t nnz,
                                        const uint64_t* row_offsets, const uint64_t* col_indices, const float* values);
sapca_status sapca_multi_upload_csr_f64(sapca_multi mh, uint64_t m, uint64_t n, uint64_t nnz,
                                        const uint64_t* row_offsets, const uint64_t* col_indices, const double* values);
sapca_status sapca_multi_fit_resident(sapca_multi mh);
sapca_status sapca_multi_transform_resident_f32(sapca_multi mh, float* out);
sapca_status sapca_multi_transform_resident_f64(sapca_multi mh, double* out);
sapca_status sapca_multi_fit_transform_resident_f32(sapca_multi mh, float* out);
sapca_status sapca_multi_fit_transform_resident_f64(sapca_multi mh, double* out);
sapca_status sapca_multi_resident_shard(sapca_multi mh, uint32_t i, uint64_t* first_row, uint64_t* rows, uint64_t* nnz,
                                        const int64_t** d_row_offsets, const int32_t** d_col_indices, void** d_values);

#ifdef __cplusplus
}
#endif
#endif /* SAPCA_H */
