// sapca.hpp -- C++ mirror of single-algebra's sparse-PCA API over the C ABI (include/sapca.h).
// Same names and argument meaning as the reference (src/dimred/pca: SVDMethod, SparsePCABuilder,
// MaskedSparsePCABuilder, fit / transform / fit_transform / feature_importances /
// explained_variance_ratio / cumulative_explained_variance_ratio); errors surface as sapca::Error
// carrying the reference's messages.  Header-only; link with -lsapca.
#pragma once
#include <cstdint>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../../include/sapca.h"

namespace sapca {

struct Error : std::runtime_error {
  sapca_status status;
  Error(sapca_status s, const std::string& m) : std::runtime_error(m), status(s) {}
};

enum class PowerIterationNormalizer { QR = SAPCA_NORM_QR, LU = SAPCA_NORM_LU, None = SAPCA_NORM_NONE };

// enum SVDMethod { Lanczos, Random { n_oversamples, n_power_iterations, normalizer } }   (pca/mod.rs:49-68)
struct SVDMethod {
  bool random = false;
  size_t n_oversamples = 10, n_power_iterations = 4;
  PowerIterationNormalizer normalizer = PowerIterationNormalizer::QR;
  static SVDMethod Lanczos() { return {}; }
  static SVDMethod Random(size_t p, size_t q, PowerIterationNormalizer n = PowerIterationNormalizer::QR) { return {true, p, q, n}; }
};

// nalgebra_sparse::CsrMatrix<T> as three borrowed arrays (usize == uint64_t indices)
template <typename T>
struct CsrRef {
  uint64_t nrows, ncols, nnz;
  const uint64_t* row_offsets;
  const uint64_t* col_indices;
  const T* values;
};

template <typename T> struct Abi;
#define SAPCA_ABI(SUF, T)                                                                                        \
  template <> struct Abi<T> {                                                                                    \
    static sapca_status fit(sapca_handle h, const CsrRef<T>& x) { return sapca_fit_csr_##SUF(h, x.nrows, x.ncols, x.nnz, x.row_offsets, x.col_indices, x.values); } \
    static sapca_status transform(sapca_handle h, const CsrRef<T>& x, T* o) { return sapca_transform_csr_##SUF(h, x.nrows, x.ncols, x.nnz, x.row_offsets, x.col_indices, x.values, o); } \
    static sapca_status fit_transform(sapca_handle h, const CsrRef<T>& x, T* o) { return sapca_fit_transform_csr_##SUF(h, x.nrows, x.ncols, x.nnz, x.row_offsets, x.col_indices, x.values, o); } \
    static sapca_status importances(sapca_handle h, T* o, size_t c) { return sapca_get_feature_importances_##SUF(h, o, c); } \
    static sapca_status ratio(sapca_handle h, T* o, size_t c) { return sapca_get_explained_variance_ratio_##SUF(h, o, c); } \
    static sapca_status cumulative(sapca_handle h, T* o, size_t c) { return sapca_get_cumulative_explained_variance_ratio_##SUF(h, o, c); } \
  };
SAPCA_ABI(f32, float)
SAPCA_ABI(f64, double)
#undef SAPCA_ABI

// Direction of the reference's Normalize / statistics traits (single-algebra src/utils.rs)
enum class Direction : int32_t { ROW = 0, COLUMN = 1 };

// A CsrMatrix uploaded once into buffers owned by a handle: Normalize / Log1P / MatrixSum / MatrixNonZero /
// MatrixMinMax (src/sparse/csr.rs:23-134, 259-392, 558-630, 917-1078) run on the resident copy and the device
// entry points of the estimators take the same arrays (src/lib.rs:28-33: normalize -> log1p -> PCA).
// sapca_csr_report: what the check found in a device CSR; canonical: safe offsets and columns, rows ascending without repeats
using CsrReport = sapca_csr_report;
inline bool is_canonical(const CsrReport& r) { return (r.flags & 15u) == 0; }

template <typename T> struct ResidentAbi;
#define SAPCA_RES(SUF, T)                                                                                          \
  template <> struct ResidentAbi<T> {                                                                              \
    static sapca_status upload(sapca_handle h, const CsrRef<T>& x, const int64_t** p, const int32_t** i, T** v) { return sapca_upload_csr_##SUF(h, x.nrows, x.ncols, x.nnz, x.row_offsets, x.col_indices, x.values, p, i, v); } \
    static sapca_status normalize(sapca_handle h, uint64_t m, uint64_t n, uint64_t nnz, const int64_t* p, const int32_t* i, T* v, const double* s, uint64_t sl, double t, int32_t d) { return sapca_normalize_csr_device_##SUF(h, m, n, nnz, p, i, v, s, sl, t, d); } \
    static sapca_status log1p(sapca_handle h, uint64_t nnz, T* v) { return sapca_log1p_csr_device_##SUF(h, nnz, v); } \
    static sapca_status stats(sapca_handle h, uint64_t m, uint64_t n, uint64_t nnz, const int64_t* p, const int32_t* i, const T* v, int32_t d, double* s, double* q, uint64_t* c, T* lo, T* hi) { return sapca_stats_csr_device_##SUF(h, m, n, nnz, p, i, v, d, s, q, c, lo, hi); } \
    static sapca_status batch_stats(sapca_handle h, uint64_t m, uint64_t n, uint64_t nnz, const int64_t* p, const int32_t* i, const T* v, int32_t ax, const int32_t* c, uint64_t cl, uint32_t nb, double* mean, double* var, uint64_t* cnt) { return sapca_batch_stats_csr_device_##SUF(h, m, n, nnz, p, i, v, ax, c, cl, nb, mean, var, cnt); } \
    static sapca_status masked_stats(sapca_handle h, uint64_t m, uint64_t n, uint64_t nnz, const int64_t* p, const int32_t* i, const T* v, int32_t d, const uint8_t* mk, uint64_t ml, double* s, double* q, uint64_t* c, double* var) { return sapca_masked_stats_csr_device_##SUF(h, m, n, nnz, p, i, v, d, mk, ml, s, q, c, var); } \
    static sapca_status n_top(sapca_handle h, uint64_t m, uint64_t n, uint64_t nnz, const int64_t* p, const int32_t* i, const T* v, const uint64_t* ns, uint32_t k, double* out) { return sapca_sum_row_n_top_csr_device_##SUF(h, m, n, nnz, p, i, v, ns, k, out); } \
    static sapca_status rank_sums(sapca_handle h, uint64_t m, uint64_t n, uint64_t nnz, const int64_t* p, const int32_t* i, const T* v, const int32_t* lab, uint32_t k, uint64_t* rows, int64_t* rs2, uint64_t* nz, double* tie) { return sapca_rank_sums_csr_device_##SUF(h, m, n, nnz, p, i, v, lab, k, rows, rs2, nz, tie); } \
    static sapca_status rank_groups(sapca_handle h, uint64_t m, uint64_t n, uint64_t nnz, const int64_t* p, const int32_t* i, const T* v, const int32_t* lab, uint32_t k, int32_t tc, uint64_t* rows, double* mean, double* var, uint64_t* nz, double* t, double* df, double* z, double* pz) { return sapca_rank_groups_csr_device_##SUF(h, m, n, nnz, p, i, v, lab, k, tc, rows, mean, var, nz, t, df, z, pz); } \
    static sapca_status hvg_moments(sapca_handle h, uint64_t m, uint64_t n, uint64_t nnz, const int64_t* p, const int32_t* i, const T* v, const int32_t* bt, int32_t b, int32_t tr, const double* clip, double* s, double* q, uint64_t* nc) { return sapca_hvg_moments_csr_device_##SUF(h, m, n, nnz, p, i, v, bt, b, tr, clip, s, q, nc); } \
    static sapca_status hvg(sapca_handle h, uint64_t m, uint64_t n, uint64_t nnz, const int64_t* p, const int32_t* i, const T* v, const int32_t* bt, uint32_t nb, const sapca_hvg_options* o, double* mean, double* var, double* vn, double* d, double* dn, double* rk, uint32_t* nhv, uint8_t* hv) { return sapca_hvg_csr_device_##SUF(h, m, n, nnz, p, i, v, bt, nb, o, mean, var, vn, d, dn, rk, nhv, hv); } \
    static sapca_status check(sapca_handle h, uint64_t m, uint64_t n, uint64_t nnz, const int64_t* p, const int32_t* i, const T* v, sapca_csr_report* rep) { return sapca_check_csr_device_##SUF(h, m, n, nnz, p, i, v, rep); } \
    static sapca_status canonicalize(sapca_handle h, uint64_t m, uint64_t n, uint64_t nnz, const int64_t* p, const int32_t* i, const T* v, uint64_t* nnz_out, const int64_t** op, const int32_t** oi, T** ov, sapca_csr_report* rep) { return sapca_canonicalize_csr_device_##SUF(h, m, n, nnz, p, i, v, nnz_out, op, oi, ov, rep); } \
    static sapca_status select_rows(sapca_handle h, uint64_t m, uint64_t n, uint64_t nnz, const int64_t* p, const int32_t* i, const T* v, const uint64_t* rows, uint64_t nr, uint64_t* nnz_out, const int64_t** op, const int32_t** oi, T** ov) { return sapca_select_rows_csr_device_##SUF(h, m, n, nnz, p, i, v, rows, nr, nnz_out, op, oi, ov); } \
    static sapca_status select(sapca_handle h, uint64_t m, uint64_t n, uint64_t nnz, const int64_t* p, const int32_t* i, const T* v, const uint64_t* rows, uint64_t nr, const uint8_t* mk, uint64_t ml, uint32_t flags, uint64_t* ncols_out, uint64_t* nnz_out, const int64_t** op, const int32_t** oi, T** ov) { return sapca_select_submatrix_csr_device_##SUF(h, m, n, nnz, p, i, v, rows, nr, mk, ml, flags, ncols_out, nnz_out, op, oi, ov); } \
  };
SAPCA_RES(f32, float)
SAPCA_RES(f64, double)
#undef SAPCA_RES

// Exact k-nearest neighbours of device-resident rows (sapca_knn_device_*): for each of the mq query rows the n_neighbors
// nearest of the mc corpus rows, best first, ties by ascending corpus index, into d_indices / d_values (DEVICE, mq x
// n_neighbors each).  The panels are row-major DEVICE arrays of d columns with row strides ldq, ldc >= d -- the scores a
// fit_transform left in HBM, taken in place.  Values: the distance (EUCLIDEAN) or the similarity of the reference's
// similarity/mod.rs (COSINE, PEARSON).  exclude_self skips corpus row i for query i.
template <typename T> struct KnnAbi;
template <> struct KnnAbi<float> { static constexpr auto call = &sapca_knn_device_f32; };
template <> struct KnnAbi<double> { static constexpr auto call = &sapca_knn_device_f64; };
template <typename T>
inline void knn_device(sapca_handle h, uint64_t mq, const T* d_queries, uint64_t ldq, uint64_t mc, const T* d_corpus, uint64_t ldc,
                       uint64_t d, sapca_knn_metric metric, uint32_t n_neighbors, bool exclude_self, int32_t* d_indices, T* d_values) {
  const sapca_status st = KnnAbi<T>::call(h, mq, d_queries, ldq, mc, d_corpus, ldc, d, (int32_t)metric, n_neighbors,
                                          exclude_self ? SAPCA_KNN_EXCLUDE_SELF : 0u, d_indices, d_values);
  if (st != SAPCA_OK) throw Error(st, sapca_last_error(h));
}

// t-SNE of device-resident rows (sapca_tsne_*; the reference's dimred::tsne, src/dimred/tsne/mod.rs:7-66).  TsneOptions()
// holds the library's defaults (TSNEConfig's output_dim, perplexity, epochs, theta and van der Maaten's constants); theta is
// stored and not read: the repulsive term is evaluated exactly.  Every pointer but `kl` and the options is a DEVICE pointer
// unless the name says host.  Each function returns the Kullback-Leibler divergence of the embedding it wrote.
struct TsneOptions : sapca_tsne_options {
  TsneOptions() { sapca_tsne_options_default(this); }
};
// the symmetric affinity matrix a call left in the handle's t-SNE buffers (valid until the next affinity call)
template <typename T>
struct TsneGraph {
  uint64_t m = 0, nnz = 0;
  const int64_t* row_offsets = nullptr;
  const int32_t* col_indices = nullptr;
  T* values = nullptr;
};
template <typename T> struct TsneAbi;
template <> struct TsneAbi<float> {
  static constexpr auto affinities = &sapca_tsne_affinities_device_f32;
  static constexpr auto gradient = &sapca_tsne_gradient_device_f32;
  static constexpr auto embed = &sapca_tsne_embed_device_f32;
  static constexpr auto device = &sapca_tsne_device_f32;
  static constexpr auto host = &sapca_tsne_f32;
};
template <> struct TsneAbi<double> {
  static constexpr auto affinities = &sapca_tsne_affinities_device_f64;
  static constexpr auto gradient = &sapca_tsne_gradient_device_f64;
  static constexpr auto embed = &sapca_tsne_embed_device_f64;
  static constexpr auto device = &sapca_tsne_device_f64;
  static constexpr auto host = &sapca_tsne_f64;
};
inline void tsne_check(sapca_handle h, sapca_status st) {
  if (st != SAPCA_OK) throw Error(st, sapca_last_error(h));
}
// stages 2-3 on neighbour lists as knn_device writes them (distances, not squares); d_beta (m doubles) may be null
template <typename T>
inline TsneGraph<T> tsne_affinities_device(sapca_handle h, uint64_t m, const int32_t* d_indices, const T* d_dist, uint32_t K,
                                           double perplexity, double* d_beta = nullptr) {
  TsneGraph<T> g;
  g.m = m;
  tsne_check(h, TsneAbi<T>::affinities(h, m, d_indices, d_dist, K, perplexity, &g.nnz, &g.row_offsets, &g.col_indices, &g.values, d_beta));
  return g;
}
// one evaluation of the gradient (m x output_dim, packed) at d_y (row stride ldy); Z and kl may be null
template <typename T>
inline void tsne_gradient_device(sapca_handle h, const TsneGraph<T>& P, const T* d_y, uint64_t ldy, uint32_t output_dim,
                                 double exaggeration, T* d_grad, double* Z, double* kl) {
  tsne_check(h, TsneAbi<T>::gradient(h, P.m, P.nnz, P.row_offsets, P.col_indices, P.values, d_y, ldy, output_dim, exaggeration, d_grad, Z, kl));
}
template <typename T>
inline double tsne_embed_device(sapca_handle h, const TsneGraph<T>& P, const sapca_tsne_options& opts, T* d_y) {
  double kl = 0.0;
  tsne_check(h, TsneAbi<T>::embed(h, P.m, P.nnz, P.row_offsets, P.col_indices, P.values, &opts, d_y, &kl));
  return kl;
}
// neighbours, affinities and embedding of an m x d panel (row stride ldx) in one call; d_y: m x output_dim
template <typename T>
inline double tsne_device(sapca_handle h, uint64_t m, const T* d_x, uint64_t ldx, uint64_t d, const sapca_tsne_options& opts, T* d_y) {
  double kl = 0.0;
  tsne_check(h, TsneAbi<T>::device(h, m, d_x, ldx, d, &opts, d_y, &kl));
  return kl;
}
// the same with host arrays: the drop-in for run_f32 / run_f64
template <typename T>
inline double tsne(sapca_handle h, uint64_t m, uint64_t d, const T* host_x, const sapca_tsne_options& opts, T* host_y) {
  double kl = 0.0;
  tsne_check(h, TsneAbi<T>::host(h, m, d, host_x, &opts, host_y, &kl));
  return kl;
}

// UMAP of device-resident rows (sapca_umap_*; include/sapca.h states the algorithm).  UmapOptions() holds the library's
// defaults (umap-learn's).  Every pointer but the options is a DEVICE pointer unless the name says host.
struct UmapOptions : sapca_umap_options {
  UmapOptions() { sapca_umap_options_default(this); }
};
// the fuzzy union a call left in the handle's UMAP buffers (valid until the next graph call)
template <typename T>
struct UmapGraph {
  uint64_t m = 0, nnz = 0;
  const int64_t* row_offsets = nullptr;
  const int32_t* col_indices = nullptr;
  T* values = nullptr;
};
template <typename T> struct UmapAbi;
template <> struct UmapAbi<float> {
  static constexpr auto graph = &sapca_umap_graph_device_f32;
  static constexpr auto embed = &sapca_umap_embed_device_f32;
  static constexpr auto device = &sapca_umap_device_f32;
  static constexpr auto host = &sapca_umap_f32;
};
template <> struct UmapAbi<double> {
  static constexpr auto graph = &sapca_umap_graph_device_f64;
  static constexpr auto embed = &sapca_umap_embed_device_f64;
  static constexpr auto device = &sapca_umap_device_f64;
  static constexpr auto host = &sapca_umap_f64;
};
inline void umap_check(sapca_handle h, sapca_status st) {
  if (st != SAPCA_OK) throw Error(st, sapca_last_error(h));
}
// (a, b) of the curve fitted to (spread, min_dist): host code, no handle
inline void umap_find_ab(double spread, double min_dist, double* a, double* b) {
  const sapca_status st = sapca_umap_find_ab(spread, min_dist, a, b);
  if (st != SAPCA_OK) throw Error(st, "sapca_umap_find_ab: refused (spread, min_dist), or the fit did not converge");
}
// stages 2-3 on neighbour lists as knn_device writes them; d_sigma, d_rho (m doubles each) may be null
template <typename T>
inline UmapGraph<T> umap_graph_device(sapca_handle h, uint64_t m, const int32_t* d_indices, const T* d_dist, uint32_t K,
                                      uint32_t n_neighbors, double* d_sigma = nullptr, double* d_rho = nullptr) {
  UmapGraph<T> g;
  g.m = m;
  umap_check(h, UmapAbi<T>::graph(h, m, d_indices, d_dist, K, n_neighbors, &g.nnz, &g.row_offsets, &g.col_indices, &g.values, d_sigma, d_rho));
  return g;
}
// the layout alone (opts.init: SAPCA_UMAP_INIT_RANDOM, or SAPCA_UMAP_INIT_GIVEN with d_y holding the start)
template <typename T>
inline void umap_embed_device(sapca_handle h, const UmapGraph<T>& G, const sapca_umap_options& opts, T* d_y) {
  umap_check(h, UmapAbi<T>::embed(h, G.m, G.nnz, G.row_offsets, G.col_indices, G.values, &opts, d_y));
}
// neighbours, graph and layout of an m x d panel (row stride ldx) in one call; d_y: m x output_dim
template <typename T>
inline void umap_device(sapca_handle h, uint64_t m, const T* d_x, uint64_t ldx, uint64_t d, const sapca_umap_options& opts, T* d_y) {
  umap_check(h, UmapAbi<T>::device(h, m, d_x, ldx, d, &opts, d_y));
}
// the same with host arrays
template <typename T>
inline void umap(sapca_handle h, uint64_t m, uint64_t d, const T* host_x, const sapca_umap_options& opts, T* host_y) {
  umap_check(h, UmapAbi<T>::host(h, m, d, host_x, &opts, host_y));
}

// Louvain clustering of a device-resident symmetric graph (sapca_louvain_*; include/sapca.h states the algorithm).
// LouvainOptions() holds the library's defaults.  Every pointer but the options is a DEVICE pointer unless the name says host.
struct LouvainOptions : sapca_louvain_options {
  LouvainOptions() { sapca_louvain_options_default(this); }
};
struct LouvainResult {
  uint64_t n_communities = 0;
  double modularity = 0.0;
  uint32_t n_levels = 0;
};
struct LouvainCoarse {   // handle-owned, f64 values, valid until the next Louvain call
  uint64_t n = 0, nnz = 0;
  const int64_t* row_offsets = nullptr;
  const int32_t* col_indices = nullptr;
  double* values = nullptr;
};
template <typename T> struct LouvainAbi;
template <> struct LouvainAbi<float> {
  static constexpr auto modularity = &sapca_louvain_modularity_device_f32;
  static constexpr auto sweep = &sapca_louvain_sweep_device_f32;
  static constexpr auto aggregate = &sapca_louvain_aggregate_device_f32;
  static constexpr auto device = &sapca_louvain_device_f32;
  static constexpr auto host = &sapca_louvain_f32;
};
template <> struct LouvainAbi<double> {
  static constexpr auto modularity = &sapca_louvain_modularity_device_f64;
  static constexpr auto sweep = &sapca_louvain_sweep_device_f64;
  static constexpr auto aggregate = &sapca_louvain_aggregate_device_f64;
  static constexpr auto device = &sapca_louvain_device_f64;
  static constexpr auto host = &sapca_louvain_f64;
};
inline void louvain_check(sapca_handle h, sapca_status st) {
  if (st != SAPCA_OK) throw Error(st, sapca_last_error(h));
}
template <typename T>
inline double louvain_modularity_device(sapca_handle h, uint64_t m, uint64_t nnz, const int64_t* row_offsets, const int32_t* col_indices,
                                        const T* values, const int32_t* d_labels, double resolution = 1.0) {
  double q = 0.0;
  louvain_check(h, LouvainAbi<T>::modularity(h, m, nnz, row_offsets, col_indices, values, d_labels, resolution, &q));
  return q;
}
template <typename T>
inline uint64_t louvain_sweep_device(sapca_handle h, uint64_t m, uint64_t nnz, const int64_t* row_offsets, const int32_t* col_indices,
                                     const T* values, const int32_t* d_labels_in, uint32_t seed, uint32_t level, uint32_t sweep,
                                     double resolution, int32_t* d_labels_out) {
  uint64_t moved = 0;
  louvain_check(h, LouvainAbi<T>::sweep(h, m, nnz, row_offsets, col_indices, values, d_labels_in, seed, level, sweep, resolution,
                                        d_labels_out, &moved));
  return moved;
}
template <typename T>
inline LouvainCoarse louvain_aggregate_device(sapca_handle h, uint64_t m, uint64_t nnz, const int64_t* row_offsets,
                                              const int32_t* col_indices, const T* values, const int32_t* d_labels,
                                              int32_t* d_renumbered = nullptr) {
  LouvainCoarse c;
  louvain_check(h, LouvainAbi<T>::aggregate(h, m, nnz, row_offsets, col_indices, values, d_labels, &c.n, &c.nnz, &c.row_offsets,
                                            &c.col_indices, &c.values, d_renumbered));
  return c;
}
template <typename T>
inline LouvainResult louvain_device(sapca_handle h, uint64_t m, uint64_t nnz, const int64_t* row_offsets, const int32_t* col_indices,
                                    const T* values, const sapca_louvain_options& opts, int32_t* d_labels) {
  LouvainResult r;
  louvain_check(h, LouvainAbi<T>::device(h, m, nnz, row_offsets, col_indices, values, &opts, d_labels, &r.n_communities, &r.modularity,
                                         &r.n_levels));
  return r;
}
template <typename T>
inline LouvainResult louvain(sapca_handle h, uint64_t m, uint64_t nnz, const int64_t* host_row_offsets, const int32_t* host_col_indices,
                             const T* host_values, const sapca_louvain_options& opts, int32_t* host_labels) {
  LouvainResult r;
  louvain_check(h, LouvainAbi<T>::host(h, m, nnz, host_row_offsets, host_col_indices, host_values, &opts, host_labels, &r.n_communities,
                                       &r.modularity, &r.n_levels));
  return r;
}

// Spectral embedding and diffusion maps of a device-resident symmetric graph (sapca_graph_components_device, sapca_spectral_*,
// sapca_umap_spectral_init_device_*; include/sapca.h states the algorithm).  SpectralOptions() holds the library's defaults.
// Every pointer but the options and the eigenvalues is a DEVICE pointer unless the name says host.
struct SpectralOptions : sapca_spectral_options {
  SpectralOptions() { sapca_spectral_options_default(this); }
};
struct SpectralResult {
  uint64_t n_components = 0;
  uint32_t n_steps = 0;
};
template <typename T> struct SpectralAbi;
template <> struct SpectralAbi<float> {
  static constexpr auto scale = &sapca_spectral_scale_device_f32;
  static constexpr auto apply = &sapca_spectral_apply_device_f32;
  static constexpr auto device = &sapca_spectral_device_f32;
  static constexpr auto host = &sapca_spectral_f32;
  static constexpr auto umap_start = &sapca_umap_spectral_init_device_f32;
};
template <> struct SpectralAbi<double> {
  static constexpr auto scale = &sapca_spectral_scale_device_f64;
  static constexpr auto apply = &sapca_spectral_apply_device_f64;
  static constexpr auto device = &sapca_spectral_device_f64;
  static constexpr auto host = &sapca_spectral_f64;
  static constexpr auto umap_start = &sapca_umap_spectral_init_device_f64;
};
inline void spectral_check(sapca_handle h, sapca_status st) {
  if (st != SAPCA_OK) throw Error(st, sapca_last_error(h));
}
// the number of components; d_labels: m int32
inline uint64_t graph_components_device(sapca_handle h, uint64_t m, uint64_t nnz, const int64_t* row_offsets, const int32_t* col_indices,
                                        int32_t* d_labels) {
  uint64_t n = 0;
  spectral_check(h, sapca_graph_components_device(h, m, nnz, row_offsets, col_indices, d_labels, &n));
  return n;
}
template <typename T>
inline void spectral_scale_device(sapca_handle h, uint64_t m, uint64_t nnz, const int64_t* row_offsets, const int32_t* col_indices,
                                  const T* values, sapca_spectral_kind kind, double* d_scale) {
  spectral_check(h, SpectralAbi<T>::scale(h, m, nnz, row_offsets, col_indices, values, (uint32_t)kind, d_scale));
}
template <typename T>
inline void spectral_apply_device(sapca_handle h, uint64_t m, uint64_t nnz, const int64_t* row_offsets, const int32_t* col_indices,
                                  const T* values, sapca_spectral_kind kind, const double* d_x, double* d_y) {
  spectral_check(h, SpectralAbi<T>::apply(h, m, nnz, row_offsets, col_indices, values, (uint32_t)kind, d_x, d_y));
}
// host_evals: opts.n_eigen doubles on the host; d_evecs: m x opts.n_eigen row-major
template <typename T>
inline SpectralResult spectral_device(sapca_handle h, uint64_t m, uint64_t nnz, const int64_t* row_offsets, const int32_t* col_indices,
                                      const T* values, const sapca_spectral_options& opts, double* host_evals, T* d_evecs) {
  SpectralResult r;
  spectral_check(h, SpectralAbi<T>::device(h, m, nnz, row_offsets, col_indices, values, &opts, host_evals, d_evecs, &r.n_components,
                                           &r.n_steps));
  return r;
}
template <typename T>
inline SpectralResult spectral(sapca_handle h, uint64_t m, uint64_t nnz, const int64_t* host_row_offsets, const int32_t* host_col_indices,
                               const T* host_values, const sapca_spectral_options& opts, double* host_evals, T* host_evecs) {
  SpectralResult r;
  spectral_check(h, SpectralAbi<T>::host(h, m, nnz, host_row_offsets, host_col_indices, host_values, &opts, host_evals, host_evecs,
                                         &r.n_components, &r.n_steps));
  return r;
}
// UMAP's spectral start from NORMALIZED eigenvectors: d_y (m x output_dim) is what umap_embed_device takes with SAPCA_UMAP_INIT_GIVEN
template <typename T>
inline void umap_spectral_init_device(sapca_handle h, uint64_t m, uint32_t output_dim, const T* d_evecs, uint64_t ld, uint32_t n_eigen,
                                      uint32_t seed, T* d_y) {
  spectral_check(h, SpectralAbi<T>::umap_start(h, m, output_dim, d_evecs, ld, n_eigen, seed, d_y));
}

// K-means of device-resident rows (sapca_kmeans_*; include/sapca.h states the algorithm).  KmeansOptions() holds the library's
// defaults.  Every pointer is a DEVICE pointer unless the name says host.
struct KmeansOptions : sapca_kmeans_options {
  KmeansOptions() { sapca_kmeans_options_default(this); }
};
struct KmeansResult {
  double inertia = 0.0;
  uint64_t n_iter = 0;
};
template <typename T> struct KmeansAbi;
template <> struct KmeansAbi<float> {
  static constexpr auto seed = &sapca_kmeans_seed_device_f32;
  static constexpr auto assign = &sapca_kmeans_assign_device_f32;
  static constexpr auto update = &sapca_kmeans_update_device_f32;
  static constexpr auto device = &sapca_kmeans_device_f32;
  static constexpr auto host = &sapca_kmeans_f32;
};
template <> struct KmeansAbi<double> {
  static constexpr auto seed = &sapca_kmeans_seed_device_f64;
  static constexpr auto assign = &sapca_kmeans_assign_device_f64;
  static constexpr auto update = &sapca_kmeans_update_device_f64;
  static constexpr auto device = &sapca_kmeans_device_f64;
  static constexpr auto host = &sapca_kmeans_f64;
};
inline void kmeans_check(sapca_handle h, sapca_status st) {
  if (st != SAPCA_OK) throw Error(st, sapca_last_error(h));
}
// k-means++ centres (k x d) of an m x d panel with row stride ldx; d_rows (k) may be null
template <typename T>
inline void kmeans_seed_device(sapca_handle h, uint64_t m, const T* d_x, uint64_t ldx, uint64_t d, uint32_t k, uint32_t seed,
                               T* d_centroids, int32_t* d_rows = nullptr) {
  kmeans_check(h, KmeansAbi<T>::seed(h, m, d_x, ldx, d, k, seed, d_centroids, d_rows));
}
// the nearest centroid of every row (also `predict`); returns the inertia; d_dist2 and n_ambiguous may be null
template <typename T>
inline double kmeans_assign_device(sapca_handle h, uint64_t m, const T* d_x, uint64_t ldx, uint64_t d, uint32_t k, const T* d_centroids,
                                   int32_t* d_labels, T* d_dist2 = nullptr, uint64_t* n_ambiguous = nullptr) {
  double inertia = 0.0;
  kmeans_check(h, KmeansAbi<T>::assign(h, m, d_x, ldx, d, k, d_centroids, d_labels, d_dist2, &inertia, n_ambiguous));
  return inertia;
}
// the means of the rows under d_labels into d_centroids (a cluster without rows keeps its own); d_counts (k) may be null
template <typename T>
inline void kmeans_update_device(sapca_handle h, uint64_t m, const T* d_x, uint64_t ldx, uint64_t d, uint32_t k, const int32_t* d_labels,
                                 T* d_centroids, int64_t* d_counts = nullptr) {
  kmeans_check(h, KmeansAbi<T>::update(h, m, d_x, ldx, d, k, d_labels, d_centroids, d_counts));
}
// the whole run on a resident panel; d_centroids (n_clusters x d) is read when opts.init == SAPCA_KMEANS_GIVEN
template <typename T>
inline KmeansResult kmeans_device(sapca_handle h, uint64_t m, const T* d_x, uint64_t ldx, uint64_t d, const sapca_kmeans_options& opts,
                                  T* d_centroids, int32_t* d_labels) {
  KmeansResult r;
  kmeans_check(h, KmeansAbi<T>::device(h, m, d_x, ldx, d, &opts, d_centroids, d_labels, &r.inertia, &r.n_iter));
  return r;
}
// the same with host arrays
template <typename T>
inline KmeansResult kmeans(sapca_handle h, uint64_t m, uint64_t d, const T* host_x, const sapca_kmeans_options& opts, T* host_centroids,
                           int32_t* host_labels) {
  KmeansResult r;
  kmeans_check(h, KmeansAbi<T>::host(h, m, d, host_x, &opts, host_centroids, host_labels, &r.inertia, &r.n_iter));
  return r;
}

template <typename T>
class ResidentCsr {
 public:
  ResidentCsr(sapca_handle h, const CsrRef<T>& x) : h_(h), m_(x.nrows), n_(x.ncols), nnz_(x.nnz) {
    check(ResidentAbi<T>::upload(h_, x, &ptr_, &idx_, &val_));
  }
  void normalize(const std::vector<double>& sums, double target, Direction d) {
    check(ResidentAbi<T>::normalize(h_, m_, n_, nnz_, ptr_, idx_, val_, sums.data(), sums.size(), target, (int32_t)d));
  }
  void log1p_normalize() { check(ResidentAbi<T>::log1p(h_, nnz_, val_)); }
  // values() is writable: after editing them with a kernel of your own, say so before the next fit
  void values_changed() { check(sapca_upload_values_changed(h_)); }
  std::vector<double> sum(Direction d) const {
    std::vector<double> s(d == Direction::COLUMN ? n_ : m_);
    check(ResidentAbi<T>::stats(h_, m_, n_, nnz_, ptr_, idx_, val_, (int32_t)d, s.data(), nullptr, nullptr, nullptr, nullptr));
    return s;
  }
  std::vector<uint64_t> nonzero(Direction d) const {
    std::vector<uint64_t> c(d == Direction::COLUMN ? n_ : m_);
    check(ResidentAbi<T>::stats(h_, m_, n_, nnz_, ptr_, idx_, val_, (int32_t)d, nullptr, nullptr, c.data(), nullptr, nullptr));
    return c;
  }
  // BatchMatrixVariance / BatchMatrixMean (csr.rs:1081-1344): B is any hashable label; f64 results keyed by the labels
  // that occur.  var_batch_row / mean_batch_col: batches label the rows (one n-long vector per label); var_batch_col /
  // mean_batch_row: batches label the columns (m-long vectors).
  template <typename B> std::unordered_map<B, std::vector<double>> var_batch_row(const std::vector<B>& b) const { return grouped(b, 0, true); }
  template <typename B> std::unordered_map<B, std::vector<double>> var_batch_col(const std::vector<B>& b) const { return grouped(b, 1, true); }
  template <typename B> std::unordered_map<B, std::vector<double>> mean_batch_row(const std::vector<B>& b) const { return grouped(b, 1, false); }
  template <typename B> std::unordered_map<B, std::vector<double>> mean_batch_col(const std::vector<B>& b) const { return grouped(b, 0, false); }
  // MatrixNTop::sum_row_n_top (csr.rs:1347-1376), f64 accumulation
  std::vector<double> sum_row_n_top(uint64_t n) const {
    std::vector<double> out(m_);
    check(ResidentAbi<T>::n_top(h_, m_, n_, nnz_, ptr_, idx_, val_, &n, 1, out.data()));
    return out;
  }
  // Rank groups (sapca_rank_sums_csr_device_* / sapca_rank_groups_csr_device_*; no reference counterpart): every group of rows
  // against the rest, per column.  d_labels: m int32 on the DEVICE (k-means' or Louvain's), a label outside [0, n_groups)
  // excludes its row.  Every array is code-major n_groups x n; what `want_*` leaves out is not computed and stays empty.
  struct RankSums {
    std::vector<uint64_t> group_rows, nonzero;
    std::vector<int64_t> rank_sum2;   // twice the rank sums
    std::vector<double> tie_sum;      // per column
  };
  RankSums rank_sums(const int32_t* d_labels, uint32_t n_groups) const {
    RankSums r;
    const size_t cells = (size_t)n_groups * n_;
    r.group_rows.resize(n_groups); r.nonzero.resize(cells); r.rank_sum2.resize(cells); r.tie_sum.resize(n_);
    check(ResidentAbi<T>::rank_sums(h_, m_, n_, nnz_, ptr_, idx_, val_, d_labels, n_groups, r.group_rows.data(), r.rank_sum2.data(),
                                    r.nonzero.data(), r.tie_sum.data()));
    return r;
  }
  struct RankGroups {
    std::vector<uint64_t> group_rows, nonzero;
    std::vector<double> mean, var, t_score, t_df, z_score, z_pvalue;
  };
  RankGroups rank_groups(const int32_t* d_labels, uint32_t n_groups, bool want_wilcoxon = true, bool want_t = false,
                         bool tie_correct = false) const {
    RankGroups r;
    const size_t cells = (size_t)n_groups * n_;
    r.group_rows.resize(n_groups); r.nonzero.resize(cells);
    if (want_wilcoxon) { r.z_score.resize(cells); r.z_pvalue.resize(cells); }
    if (want_t) { r.mean.resize(cells); r.var.resize(cells); r.t_score.resize(cells); r.t_df.resize(cells); }
    const auto ptr = [](std::vector<double>& v) { return v.empty() ? nullptr : v.data(); };
    check(ResidentAbi<T>::rank_groups(h_, m_, n_, nnz_, ptr_, idx_, val_, d_labels, n_groups, tie_correct ? 1 : 0, r.group_rows.data(),
                                      ptr(r.mean), ptr(r.var), r.nonzero.data(), ptr(r.t_score), ptr(r.t_df), ptr(r.z_score),
                                      ptr(r.z_pvalue)));
    return r;
  }
  // Variable genes (sapca_hvg_moments_csr_device_* / sapca_hvg_csr_device_*; no reference counterpart): scanpy's
  // highly_variable_genes, flavours seurat_v3 and seurat.  d_batch: m int32 on the DEVICE or null (one batch of all rows); a
  // label outside [0, n_batches) excludes its row.  highly_variable feeds sapca_set_mask and select(col_mask) unchanged.
  struct HvgMoments {
    std::vector<double> sum, sum_squared;
    std::vector<uint64_t> n_clipped;
  };
  HvgMoments hvg_moments(int32_t transform, const double* clip = nullptr, const int32_t* d_batch = nullptr, int32_t batch = 0) const {
    HvgMoments r;
    r.sum.resize(n_); r.sum_squared.resize(n_); r.n_clipped.resize(n_);
    check(ResidentAbi<T>::hvg_moments(h_, m_, n_, nnz_, ptr_, idx_, val_, d_batch, batch, transform, clip, r.sum.data(), r.sum_squared.data(),
                                      r.n_clipped.data()));
    return r;
  }
  struct HvgOptions : sapca_hvg_options {
    HvgOptions() { sapca_hvg_options_default(this); }
  };
  struct Hvg {
    std::vector<double> means, variances, variances_norm, dispersions, dispersions_norm, rank;
    std::vector<uint32_t> n_batches_hv;
    std::vector<uint8_t> highly_variable;
  };
  Hvg highly_variable(const sapca_hvg_options& opts, const int32_t* d_batch = nullptr, uint32_t n_batches = 1) const {
    Hvg r;
    for (auto* v : {&r.means, &r.variances, &r.variances_norm, &r.dispersions, &r.dispersions_norm, &r.rank}) v->resize(n_);
    r.n_batches_hv.resize(n_); r.highly_variable.resize(n_);
    check(ResidentAbi<T>::hvg(h_, m_, n_, nnz_, ptr_, idx_, val_, d_batch, n_batches, &opts, r.means.data(), r.variances.data(),
                              r.variances_norm.data(), r.dispersions.data(), r.dispersions_norm.data(), r.rank.data(),
                              r.n_batches_hv.data(), r.highly_variable.data()));
    return r;
  }
  // *_masked (csr.rs:153-252, 418-556, 815-914): col = per column over the rows with mask[row] (mask.size() >= m),
  // row = per row over the columns with mask[col] (mask.size() >= n); f64 sums, stored-entry variance without correction
  std::vector<uint64_t> nonzero_col_masked(const std::vector<bool>& mask) const { return masked<uint64_t>(Direction::COLUMN, &mask, 2); }
  std::vector<uint64_t> nonzero_row_masked(const std::vector<bool>& mask) const { return masked<uint64_t>(Direction::ROW, &mask, 2); }
  std::vector<double> sum_col_masked(const std::vector<bool>& mask) const { return masked<double>(Direction::COLUMN, &mask, 0); }
  std::vector<double> sum_row_masked(const std::vector<bool>& mask) const { return masked<double>(Direction::ROW, &mask, 0); }
  std::vector<double> var_col_masked(const std::vector<bool>& mask) const { return masked<double>(Direction::COLUMN, &mask, 3); }
  std::vector<double> var_row_masked(const std::vector<bool>& mask) const { return masked<double>(Direction::ROW, &mask, 3); }
  // *_chunk (csr.rs:124-150, 394-416, 728-813, 939-1008): in place on the caller's vectors, as the reference does; where
  // the reference would index out of bounds, Error(SAPCA_ERR_ARG) before anything is written
  template <typename U> void nonzero_col_chunk(std::vector<U>& ref) const { add_into(ref, nonzero(Direction::COLUMN)); }
  template <typename U> void nonzero_row_chunk(std::vector<U>& ref) const { add_into(ref, nonzero(Direction::ROW)); }
  template <typename U> void sum_col_chunk(std::vector<U>& ref) const { add_into(ref, sum(Direction::COLUMN)); }
  template <typename U> void sum_row_chunk(std::vector<U>& ref) const {
    if (ref.size() < m_) throw Error(SAPCA_ERR_ARG, "sum_row_chunk: reference length " + std::to_string(ref.size()) + " is less than number of rows " + std::to_string(m_));
    const std::vector<double> s = sum(Direction::ROW);
    for (uint64_t r = 0; r < m_; ++r) ref[r] = (U)s[r];
  }
  template <typename U> void var_col_chunk(std::vector<U>& ref) const { var_into(ref, Direction::COLUMN, "columns"); }
  template <typename U> void var_row_chunk(std::vector<U>& ref) const { var_into(ref, Direction::ROW, "rows"); }
  template <typename U> void min_max_col_chunk(std::vector<U>& mins, std::vector<U>& maxs) const { min_max_into(mins, maxs, Direction::COLUMN, true); }
  template <typename U> void min_max_row_chunk(std::vector<U>& mins, std::vector<U>& maxs) const { min_max_into(mins, maxs, Direction::ROW, false); }
  // Rows `rows` of this matrix (any order, repeats allowed) as a resident matrix of their own in the same handle, without
  // crossing PCIe (sapca_select_rows_csr_device_*): cell filtering, a fit on reference cells, per-cluster fits, bootstraps.
  // This matrix stays as it is; the result is valid until the next select_rows on the handle and cannot itself be the
  // source of one.
  ResidentCsr select_rows(const std::vector<uint64_t>& rows) const {
    ResidentCsr out(h_, (uint64_t)rows.size(), n_);
    check(ResidentAbi<T>::select_rows(h_, m_, n_, nnz_, ptr_, idx_, val_, rows.data(), rows.size(), &out.nnz_, &out.ptr_, &out.idx_, &out.val_));
    return out;
  }
  // Rows AND columns in one call (sapca_select_submatrix_csr_device_*): this[rows][:, cols].  rows null: every row in order;
  // cols null: every column, otherwise a mask of ncols() entries -- a kept column is renumbered by its rank among the kept
  // ones (MaskedCSRMatrix::new, sparse_masked/mod.rs:264-271, 455-466), so gene filters serve statistics, normalisation and
  // every fit alike.  drop_stored_zeros: entries whose value == 0 go as well (a NaN stays).  Same buffers and lifetime as
  // select_rows: one selection per handle, either call replaces it.
  ResidentCsr select(const std::vector<uint64_t>* rows, const std::vector<bool>* cols = nullptr, bool drop_stored_zeros = false) const {
    std::vector<uint8_t> mk;
    if (cols) mk.assign(cols->begin(), cols->end());
    ResidentCsr out(h_, rows ? (uint64_t)rows->size() : m_, n_);
    check(ResidentAbi<T>::select(h_, m_, n_, nnz_, ptr_, idx_, val_, rows ? rows->data() : nullptr, out.m_, cols ? mk.data() : nullptr,
                                 mk.size(), drop_stored_zeros ? SAPCA_SELECT_DROP_STORED_ZEROS : 0u, &out.n_, &out.nnz_, &out.ptr_,
                                 &out.idx_, &out.val_));
    return out;
  }
  // What the arrays are (sapca_check_csr_device_*): safe offsets and columns, rows ascending without repeats.  Read-only.
  CsrReport check_csr() const {
    CsrReport rep{};
    rep.struct_size = (uint32_t)sizeof(rep);
    check(ResidentAbi<T>::check(h_, m_, n_, nnz_, ptr_, idx_, val_, &rep));
    return rep;
  }
  // The same matrix with every row sorted by column and equal columns summed left to right (sapca_canonicalize_csr_device_*),
  // in the handle's canonical buffers beside this one; this matrix itself when it is canonical already.  `report` (may be
  // null) receives the report of THIS matrix.  Valid until the next canonicalize on the handle.
  ResidentCsr canonicalize(CsrReport* report = nullptr) const {
    ResidentCsr out(h_, m_, n_);
    if (report) report->struct_size = (uint32_t)sizeof(*report);
    check(ResidentAbi<T>::canonicalize(h_, m_, n_, nnz_, ptr_, idx_, val_, &out.nnz_, &out.ptr_, &out.idx_, &out.val_, report));
    return out;
  }
  uint64_t nrows() const { return m_; }
  uint64_t ncols() const { return n_; }
  uint64_t nnz() const { return nnz_; }
  const int64_t* row_offsets() const { return ptr_; }
  const int32_t* col_indices() const { return idx_; }
  T* values() const { return val_; }

 private:
  ResidentCsr(sapca_handle h, uint64_t m, uint64_t n) : h_(h), m_(m), n_(n), nnz_(0) {}   // (filled in by select_rows / select)
  void check(sapca_status st) const {
    if (st != SAPCA_OK) throw Error(st, sapca_last_error(h_));
  }
  // what: 0 sum, 1 sum of squares, 2 count, 3 variance
  template <typename R>
  std::vector<R> masked(Direction d, const std::vector<bool>* mask, int what) const {
    const uint64_t len = d == Direction::COLUMN ? n_ : m_;
    std::vector<uint8_t> mk;
    if (mask) mk.assign(mask->begin(), mask->end());
    std::vector<double> s(len), q(len), var(len);
    std::vector<uint64_t> c(len);
    check(ResidentAbi<T>::masked_stats(h_, m_, n_, nnz_, ptr_, idx_, val_, (int32_t)d, mask ? mk.data() : nullptr, mk.size(), s.data(),
                                       q.data(), c.data(), var.data()));
    const std::vector<double>& f = what == 0 ? s : what == 1 ? q : var;
    return what == 2 ? std::vector<R>(c.begin(), c.end()) : std::vector<R>(f.begin(), f.end());
  }
  template <typename U, typename V>
  static void add_into(std::vector<U>& ref, const std::vector<V>& v) {
    for (size_t j = 0; j < ref.size() && j < v.size(); ++j) ref[j] += (U)v[j];
  }
  template <typename U>
  void var_into(std::vector<U>& ref, Direction d, const char* what) const {
    const uint64_t len = d == Direction::COLUMN ? n_ : m_;
    if (ref.size() != len)
      throw Error(SAPCA_ERR_ARG, "Reference slice length " + std::to_string(ref.size()) + " does not match number of " + what + " " + std::to_string(len));
    const std::vector<double> v = masked<double>(d, nullptr, 3);
    for (uint64_t j = 0; j < len; ++j) ref[j] = (U)v[j];
  }
  template <typename U>
  void min_max_into(std::vector<U>& mins, std::vector<U>& maxs, Direction d, bool narrow) const {
    const uint64_t len = d == Direction::COLUMN ? n_ : m_;
    std::vector<uint64_t> c(len);
    std::vector<T> lo(len), hi(len);
    check(ResidentAbi<T>::stats(h_, m_, n_, nnz_, ptr_, idx_, val_, (int32_t)d, nullptr, nullptr, c.data(), lo.data(), hi.data()));
    for (uint64_t j = 0; j < len; ++j)
      if (c[j] && (j >= mins.size() || j >= maxs.size()))
        throw Error(SAPCA_ERR_ARG, std::string(narrow ? "min_max_col_chunk: column " : "min_max_row_chunk: row ") + std::to_string(j) +
                                       " has stored entries but the reference is shorter");
    for (uint64_t j = 0; j < len; ++j) {
      if (!c[j]) continue;
      const U a = (U)lo[j], b = (U)hi[j];
      if (!narrow || a < mins[j]) mins[j] = a;   // column chunk: a running min / max; row chunk: overwritten
      if (!narrow || b > maxs[j]) maxs[j] = b;
    }
  }
  template <typename B>
  std::unordered_map<B, std::vector<double>> grouped(const std::vector<B>& batches, int32_t axis, bool variance) const {
    std::unordered_map<B, int32_t> code;
    std::vector<const B*> label;
    std::vector<int32_t> codes(batches.size());
    for (size_t j = 0; j < batches.size(); ++j) {
      auto it = code.emplace(batches[j], (int32_t)label.size());
      if (it.second) label.push_back(&batches[j]);
      codes[j] = it.first->second;
    }
    const uint64_t len = axis == 0 ? n_ : m_;
    std::vector<double> res(label.size() * len);
    check(ResidentAbi<T>::batch_stats(h_, m_, n_, nnz_, ptr_, idx_, val_, axis, codes.data(), codes.size(), (uint32_t)label.size(),
                                      variance ? nullptr : res.data(), variance ? res.data() : nullptr, nullptr));
    std::unordered_map<B, std::vector<double>> out;
    for (size_t b = 0; b < label.size(); ++b) out.emplace(*label[b], std::vector<double>(res.begin() + b * len, res.begin() + (b + 1) * len));
    return out;
  }
  sapca_handle h_;
  uint64_t m_, n_, nnz_;
  const int64_t* ptr_ = nullptr;
  const int32_t* idx_ = nullptr;
  T* val_ = nullptr;
};

template <typename T>
class SparsePCA {
 public:
  // lanczos_center: no reference counterpart (sapca_options.lanczos_center: the Lanczos SVD of the centred operator, opt-in)
  SparsePCA(size_t n_components, T alpha, T tolerance, uint32_t seed, bool center, bool verbose, SVDMethod m,
            const std::vector<bool>* mask = nullptr, bool lanczos_center = false)
      : k_(n_components), mask_len_(mask ? mask->size() : 0), masked_(mask != nullptr) {
    sapca_options o;
    sapca_options_default(&o);
    o.n_components = n_components; o.alpha = alpha; o.tolerance = tolerance; o.random_seed = seed;
    o.center = center; o.verbose = verbose; o.lanczos_center = lanczos_center;
    o.method = m.random ? SAPCA_RANDOM : SAPCA_LANCZOS;
    o.n_oversamples = m.n_oversamples; o.n_power_iterations = m.n_power_iterations; o.normalizer = (int32_t)m.normalizer;
    sapca_status st = sapca_create(&o, &h_);
    if (st != SAPCA_OK) throw Error(st, sapca_last_error(nullptr));
    if (mask && !mask->empty()) {
      std::vector<uint8_t> b(mask->begin(), mask->end());
      check(sapca_set_mask(h_, b.data(), b.size()));
    }
  }
  ~SparsePCA() { sapca_destroy(h_); }
  SparsePCA(const SparsePCA&) = delete;
  SparsePCA& operator=(const SparsePCA&) = delete;

  // Per-row covariates of the next fit / transform, regressed out implicitly (sapca_set_covariates; no reference counterpart):
  // z is rows x cols, row-major; rows == 0 or cols == 0 clears.  SVDMethod::Random only.
  SparsePCA& set_covariates(const std::vector<double>& z, size_t rows, size_t cols) {
    if (z.size() != rows * cols) throw Error(SAPCA_ERR_ARG, "covariates: z must hold rows x cols values");
    check(sapca_set_covariates(h_, z.data(), rows, cols));
    return *this;
  }
  // Column scaling of the next fit, applied implicitly (sapca_set_column_scaling; no reference counterpart): the fit is that of
  // (A - 1 mu^T) diag(d).  SAPCA_SCALE_UNIT_VARIANCE takes no weights; SAPCA_SCALE_WEIGHTS one per column of the matrix;
  // SAPCA_SCALE_NONE clears.  SVDMethod::Random only.
  SparsePCA& set_column_scaling(sapca_column_scaling mode, const std::vector<double>& weights = {}) {
    check(sapca_set_column_scaling(h_, (int32_t)mode, mode == SAPCA_SCALE_WEIGHTS && !weights.empty() ? weights.data() : nullptr,
                                   mode == SAPCA_SCALE_WEIGHTS ? weights.size() : 0));
    return *this;
  }
  // the factors the fitted model applied, one per column the fit used; empty for a model fitted without scaling
  std::vector<double> column_scale() const {
    int32_t mode = 0;
    check(sapca_get_column_scale(h_, &mode, nullptr, 0));
    if (mode == SAPCA_SCALE_NONE) return {};
    uint64_t k = 0, n_used = 0, n_cols = 0;
    check(sapca_get_dims(h_, &k, &n_used, &n_cols));
    std::vector<double> d(n_used);
    check(sapca_get_column_scale(h_, &mode, d.data(), d.size()));
    return d;
  }
  SparsePCA& fit(const CsrRef<T>& x) { mask_check(x); check(Abi<T>::fit(h_, x)); return *this; }
  std::vector<T> transform(const CsrRef<T>& x) const {                     // m x k row-major
    mask_check(x);
    std::vector<T> out(x.nrows * k_);
    check(Abi<T>::transform(h_, x, out.data()));
    return out;
  }
  std::vector<T> fit_transform(const CsrRef<T>& x) {
    mask_check(x);
    std::vector<T> out(x.nrows * k_);
    check(Abi<T>::fit_transform(h_, x, out.data()));
    return out;
  }
  std::vector<T> feature_importances() const {                             // k x n_used row-major
    uint64_t k, nu, nc;
    check(sapca_get_dims(h_, &k, &nu, &nc));
    std::vector<T> out(k * nu);
    check(Abi<T>::importances(h_, out.data(), out.size()));
    return out;
  }
  std::vector<T> explained_variance_ratio() const { return vec(&Abi<T>::ratio); }
  std::vector<T> cumulative_explained_variance_ratio() const { return vec(&Abi<T>::cumulative); }
  sapca_handle handle() const { return h_; }

 private:
  void check(sapca_status st) const { if (st != SAPCA_OK) throw Error(st, sapca_last_error(h_)); }
  void mask_check(const CsrRef<T>& x) const {   // the reference rejects any mismatch, an empty mask included (masked :258-262)
    if (masked_ && x.ncols != mask_len_)
      throw Error(SAPCA_ERR_MASK_LEN, "The mask vector length and the number of features (columns) have to be the same!");
  }
  std::vector<T> vec(sapca_status (*get)(sapca_handle, T*, size_t)) const {
    uint64_t k, nu, nc;
    check(sapca_get_dims(h_, &k, &nu, &nc));
    std::vector<T> out(k);
    check(get(h_, out.data(), out.size()));
    return out;
  }
  sapca_handle h_ = nullptr;
  size_t k_, mask_len_;
  bool masked_;
};

// SparsePCABuilder<T> (sparse/mod.rs:375-484) and MaskedSparsePCABuilder<T> (sparse_masked/mod.rs:37-160)
template <typename T, bool Masked>
class BuilderT {
 public:
  BuilderT& n_components(size_t n) { k_ = n; return *this; }
  BuilderT& alpha(T a) { alpha_ = a; return *this; }
  BuilderT& tolerance(T t) { tol_ = t; return *this; }
  BuilderT& random_seed(uint32_t s) { seed_ = s; return *this; }
  BuilderT& center(bool c) { center_ = c; return *this; }
  BuilderT& verbose(bool v) { verbose_ = v; return *this; }
  BuilderT& svd_method(SVDMethod m) { method_ = m; return *this; }
  BuilderT& lanczos_center(bool on = true) { lanczos_center_ = on; return *this; }   // (extension: sapca_options.lanczos_center)
  BuilderT& mask(std::vector<bool> m) { static_assert(Masked, "mask() belongs to MaskedSparsePCABuilder"); mask_ = std::move(m); return *this; }
  SparsePCA<T>* build() const { return new SparsePCA<T>(k_, alpha_, tol_, seed_, center_, verbose_, method_, Masked ? &mask_ : nullptr, lanczos_center_); }

 private:
  size_t k_ = 50; T alpha_ = 1; T tol_ = (T)1e-6; uint32_t seed_ = 42; bool center_ = true, verbose_ = false;   // :392-401
  bool lanczos_center_ = false;
  SVDMethod method_{};
  std::vector<bool> mask_;
};
template <typename T> using SparsePCABuilder = BuilderT<T, false>;
template <typename T> using MaskedSparsePCABuilder = BuilderT<T, true>;

}  // namespace sapca
