// The operations on a device-resident CSR behind the sapca_*_csr_device_* entry points: preprocessing,
// statistics, row selection, check / canonicalise.  Host side only: buffer layouts, launches, the finishing arithmetic.
// They throw sapca::Error; api.cpp turns that into a status.
#pragma once
#include <functional>

#include "checks.h"
#include "engine.h"

namespace sapca {

// The caller's device arrays as a view, NOT checked: every operation below runs check_view() on it, at the point where its
// argument checks reach the matrix (their order is part of the ABI's behaviour).
template <typename T>
CsrView<T> unchecked_view(uint64_t m, uint64_t n, uint64_t nnz, const int64_t* p, const int32_t* i, const T* v) {
  CsrView<T> a;
  a.rows = (int64_t)m; a.cols = (int64_t)n; a.nnz = (int64_t)nnz; a.ptr = p; a.idx = i; a.val = v;
  return a;
}
template <typename T>
void check_view(const CsrView<T>& a) {
  SAPCA_CHECK(a.ptr != nullptr && (a.nnz == 0 || (a.idx && a.val)), SAPCA_ERR_ARG, "null CSR array");
  SAPCA_CHECK((uint64_t)a.cols < (1ull << 31) && (uint64_t)a.rows < (1ull << 31), SAPCA_ERR_ARG,
              "more than 2^31-1 rows or columns is not supported");
}

namespace resident {

using H = sapca_handle_s;

// dst <- the dst.size() elements at `d`, queued on the stream: the caller synchronises once behind its last one
template <typename U>
void fetch(std::vector<U>& dst, const U* d, hipStream_t s) {
  if (dst.empty()) return;
  SAPCA_HIP(hipMemcpyAsync(dst.data(), d, dst.size() * sizeof(U), hipMemcpyDeviceToHost, s));
}

// The code-slice loop of the labelled statistics (batch_stats, rank_groups): k::batch_row_stats on the rows of R for
// batch_codes_per_launch() codes at a time (d_codes: device, one per column of R; a code outside the slice is skipped), into
// h.batch_out.  f(lo, nb, sum, m2, cnt) sees each slice once its results are on the host: [nb][R.rows], code-major.
template <typename T, typename F>
void for_each_code_slice(H& h, const CsrView<T>& R, const int32_t* d_codes, uint32_t n_codes, F&& f) {
  hipStream_t s = h.stream;
  const uint64_t len = (uint64_t)R.rows;
  const int per = k::batch_codes_per_launch();
  const int nb_max = (int)std::min<uint32_t>(n_codes, (uint32_t)per);
  double* d_sum = h.batch_out.as<double>((size_t)nb_max * len * 5 / 2 + 1);   // sum, m2 (f64) and count (u32) per slot
  double* d_m2 = d_sum + (size_t)nb_max * len;
  uint32_t* d_cnt = reinterpret_cast<uint32_t*>(d_m2 + (size_t)nb_max * len);
  std::vector<double> hs, hm;
  std::vector<uint32_t> hc;
  for (uint32_t lo = 0; lo < n_codes; lo += (uint32_t)per) {
    const int nb = (int)std::min<uint32_t>(n_codes - lo, (uint32_t)per);
    const size_t cells = (size_t)nb * len;
    k::batch_row_stats(R, d_codes, (int)lo, nb, d_sum, d_m2, d_cnt, s);
    hs.resize(cells); hm.resize(cells); hc.resize(cells);
    fetch(hs, d_sum, s);
    fetch(hm, d_m2, s);
    fetch(hc, d_cnt, s);
    SAPCA_HIP(hipStreamSynchronize(s));
    f(lo, nb, hs, hm, hc);
  }
}

template <typename T>
void normalize(H& h, const CsrView<T>& A, T* v, const double* sums, uint64_t sums_len, double target, int32_t direction);
template <typename T>
void log1p(H& h, uint64_t nnz, T* v);
// direction 0: per row (sum_row, sum_row_squared, nonzero_row, min_max_row); 1: per column (the same on A^T)
template <typename T>
void stats(H& h, const CsrView<T>& A, int32_t direction, double* sum, double* sumsq, uint64_t* nonzero, T* minv, T* maxv);
template <typename T>
void batch_stats(H& h, const CsrView<T>& A, int32_t grouped_axis, const int32_t* codes, uint64_t codes_len, uint32_t n_batches,
                 double* mean, double* var, uint64_t* count);
template <typename T>
void masked_stats(H& h, const CsrView<T>& A, int32_t direction, const uint8_t* mask, uint64_t mask_len, double* sum, double* sumsq,
                  uint64_t* count, double* var);
// sapca_rank_sums_csr_device_* / sapca_rank_groups_csr_device_* (rankgroups.cpp): the exact quantities of the rank pass, and the
// Wilcoxon / Welch scores of every group against the rest; d_labels: device, one per row; every output: host, may be null
template <typename T>
void rank_sums(H& h, const CsrView<T>& A, const int32_t* d_labels, uint32_t n_groups, uint64_t* group_rows, int64_t* rank_sum2,
               uint64_t* nonzero, double* tie_sum);
template <typename T>
void rank_groups(H& h, const CsrView<T>& A, const int32_t* d_labels, uint32_t n_groups, int32_t tie_correct, uint64_t* group_rows,
                 double* mean, double* var, uint64_t* nonzero, double* t_score, double* t_df, double* z_score, double* z_pvalue);
// sapca_hvg_moments_csr_device_* / sapca_loess_f64 / sapca_hvg_csr_device_* (hvg.cpp): the transformed column moments of one
// batch, the local quadratic regression of host arrays, and the seurat_v3 / seurat selection; d_batch: device, one per row or
// null; clip and every output: host, outputs may be null
template <typename T>
void hvg_moments(H& h, const CsrView<T>& A, const int32_t* d_batch, int32_t batch, int32_t transform, const double* clip, double* sum,
                 double* sumsq, uint64_t* n_clipped);
void loess(H& h, uint64_t n, const double* x, const double* y, double span, double* fitted);
template <typename T>
void hvg(H& h, const CsrView<T>& A, const int32_t* d_batch, uint32_t n_batches, const sapca_hvg_options* opts, double* means,
         double* variances, double* variances_norm, double* dispersions, double* dispersions_norm, double* rank, uint32_t* n_batches_hv,
         uint8_t* highly_variable);
// MatrixNTop::sum_row_n_top (csr.rs:1347-1376) for several n in one pass over the rows: out[i * m + r]
template <typename T>
void top_n(H& h, const CsrView<T>& A, const uint64_t* ns, uint32_t n_ns, double* out);
template <typename T>
void select_rows(H& h, const CsrView<T>& A, const uint64_t* rows, uint64_t n_rows, uint64_t* nnz_out, const int64_t** d_ptr,
                 const int32_t** d_idx, T** d_val);
// A[rows][:, col_mask] (rows null: rows 0 .. n_rows - 1; col_mask null: every column), flags: SAPCA_SELECT_*
template <typename T>
void select_submatrix(H& h, const CsrView<T>& A, const uint64_t* rows, uint64_t n_rows, const uint8_t* col_mask, uint64_t mask_len,
                      uint32_t flags, uint64_t* n_cols_out, uint64_t* nnz_out, const int64_t** d_ptr, const int32_t** d_idx, T** d_val);
template <typename T>
void check(H& h, const CsrView<T>& A, sapca_csr_report* report);
template <typename T>
void canonicalize(H& h, const CsrView<T>& A, uint64_t* nnz_out, const int64_t** d_ptr, const int32_t** d_idx, T** d_val,
                  sapca_csr_report* report);

// sapca_knn_device_*: the n_neighbors nearest corpus rows of every query row of two dense device panels
template <typename T>
void knn(H& h, uint64_t mq, const T* d_queries, uint64_t ldq, uint64_t mc, const T* d_corpus, uint64_t ldc, uint64_t d, int32_t metric,
         uint32_t n_neighbors, uint32_t flags, int32_t* d_indices, T* d_values);

// The front half of the two neighbour-graph builders (tsne.cpp; count / emit are tsne.hip's): the checks on m, K and the lists,
// g's buffers, `weights(p)` (enqueues the m x K per-slot weights), the emitted rows, and the row sort with its merged offsets.
// What it leaves for the caller's finish: the emitted rows, then the rows to read (sorted: g.sort_*, the raw arrays are free to
// take the result; else the raw ones), the offsets and the entry count of the graph (merged != 0: g.out_ptr).  m == 0 gives
// the empty graph, complete.
struct RawGraph {
  CsrView<double> raw;
  const int64_t* ptr = nullptr;
  const int32_t* idx = nullptr;
  const double* val = nullptr;
  uint64_t nnz = 0, merged = 0;
  bool sorted = false;
};
RawGraph neighbour_graph(H& h, H::NeighbourGraph& g, const std::string& who, uint64_t m, uint32_t K, const int32_t* d_indices,
                         bool dist_given, const std::function<void(double*)>& weights);

// sapca_tsne_* (tsne.cpp): the affinity graph of neighbour lists, one gradient evaluation, the optimiser, and the whole chain
// on a device panel or on host arrays
template <typename T>
void tsne_affinities(H& h, uint64_t m, const int32_t* d_indices, const T* d_dist, uint32_t K, double perplexity, uint64_t* nnz_out,
                     const int64_t** d_ptr, const int32_t** d_idx, T** d_val, double* d_beta);
template <typename T>
void tsne_gradient(H& h, const CsrView<T>& P, const T* d_y, uint64_t ldy, uint32_t output_dim, double exaggeration, T* d_grad, double* Z,
                   double* kl);
template <typename T>
void tsne_embed(H& h, const CsrView<T>& P, const sapca_tsne_options* opts, T* d_y, double* kl);
template <typename T>
void tsne_device(H& h, uint64_t m, const T* d_x, uint64_t ldx, uint64_t d, const sapca_tsne_options* opts, T* d_y, double* kl);
template <typename T>
void tsne_host(H& h, uint64_t m, uint64_t d, const T* x, const sapca_tsne_options* opts, T* y, double* kl);

// sapca_kmeans_* (kmeans.cpp): seeding, one assignment, one update, and the whole run on a device panel or on host arrays
template <typename T>
void kmeans_seed(H& h, uint64_t m, const T* d_x, uint64_t ldx, uint64_t d, uint32_t k, uint32_t seed, T* d_centroids, int32_t* d_rows);
template <typename T>
void kmeans_assign(H& h, uint64_t m, const T* d_x, uint64_t ldx, uint64_t d, uint32_t k, const T* d_centroids, int32_t* d_labels, T* d_dist2,
                   double* inertia, uint64_t* n_ambiguous);
template <typename T>
void kmeans_update(H& h, uint64_t m, const T* d_x, uint64_t ldx, uint64_t d, uint32_t k, const int32_t* d_labels, T* d_centroids,
                   int64_t* d_counts);
template <typename T>
void kmeans_device(H& h, uint64_t m, const T* d_x, uint64_t ldx, uint64_t d, const sapca_kmeans_options* opts, T* d_centroids,
                   int32_t* d_labels, double* inertia, uint64_t* n_iter);
template <typename T>
void kmeans_host(H& h, uint64_t m, uint64_t d, const T* x, const sapca_kmeans_options* opts, T* centroids, int32_t* labels, double* inertia,
                 uint64_t* n_iter);

// sapca_harmony_* (harmony.cpp): one clustering pass, the centroids, the correction, and the whole run on device panels or on
// host arrays
template <typename T>
void harmony_assign(H& h, uint64_t m, const T* d_zc, uint64_t ldz, uint64_t d, const int32_t* d_batch, uint32_t B, uint32_t K, T* d_y,
                    int32_t recompute, T* d_r, double theta, double sigma, uint32_t n_blocks, uint32_t seed, uint64_t pass, double* o,
                    double* rs, double* objective);
template <typename T>
void harmony_centroids(H& h, uint64_t m, const T* d_zc, uint64_t ldz, uint64_t d, uint32_t K, const T* d_r, T* d_y);
template <typename T>
void harmony_correct(H& h, uint64_t m, const T* d_z, uint64_t ldz, uint64_t d, const int32_t* d_batch, uint32_t B, uint32_t K, const T* d_r,
                     double lambda, T* d_zcorr, uint64_t ldc, double* beta);
struct HarmonyParams {
  uint32_t B, K, init, n_blocks, max_iter_harmony, max_iter_cluster, seed;
  double theta, sigma, lambda, epsilon_cluster, epsilon_harmony;
};
template <typename T>
void harmony_device(H& h, uint64_t m, const T* d_z, uint64_t ldz, uint64_t d, const int32_t* d_batch, const HarmonyParams& p, T* d_zcorr,
                    uint64_t ldc, T* d_r, T* d_y, double* objectives, uint32_t* passes, uint32_t* n_iter, int32_t* converged);
template <typename T>
void harmony_host(H& h, uint64_t m, uint64_t d, const T* z, const int32_t* batch, const HarmonyParams& p, T* zcorr, T* r, T* y,
                  double* objectives, uint32_t* passes, uint32_t* n_iter, int32_t* converged);

// sapca_umap_* (umap.cpp): the curve fit (host only), the fuzzy union of neighbour lists, the layout, and the whole chain on a
// device panel or on host arrays
void umap_find_ab(double spread, double min_dist, double* a, double* b);
template <typename T>
void umap_graph(H& h, uint64_t m, const int32_t* d_indices, const T* d_dist, uint32_t K, uint32_t n_neighbors, uint64_t* nnz_out,
                const int64_t** d_ptr, const int32_t** d_idx, T** d_val, double* d_sigma, double* d_rho);
template <typename T>
void umap_embed(H& h, const CsrView<T>& G, const sapca_umap_options* opts, T* d_y);
template <typename T>
void umap_device(H& h, uint64_t m, const T* d_x, uint64_t ldx, uint64_t d, const sapca_umap_options* opts, T* d_y);
template <typename T>
void umap_host(H& h, uint64_t m, uint64_t d, const T* x, const sapca_umap_options* opts, T* y);


// sapca_louvain_* (louvain.cpp): the modularity of given labels, one sweep, one aggregation, and the whole run on a resident
// graph or on host arrays
template <typename T>
void louvain_modularity(H& h, const CsrView<T>& G, const int32_t* d_labels, double resolution, double* modularity);
template <typename T>
void louvain_sweep(H& h, const CsrView<T>& G, const int32_t* d_labels_in, uint32_t seed, uint32_t level, uint32_t sweep, double resolution,
                   int32_t* d_labels_out, uint64_t* n_moved);
template <typename T>
void louvain_aggregate(H& h, const CsrView<T>& G, const int32_t* d_labels, uint64_t* n_out, uint64_t* nnz_out, const int64_t** d_ptr,
                       const int32_t** d_idx, double** d_val, int32_t* d_renumbered);
template <typename T>
void louvain_device(H& h, const CsrView<T>& G, const sapca_louvain_options* opts, int32_t* d_labels, uint64_t* n_communities,
                    double* modularity, uint32_t* n_levels);
template <typename T>
void louvain_host(H& h, uint64_t m, uint64_t nnz, const int64_t* ptr, const int32_t* idx, const T* val, const sapca_louvain_options* opts,
                  int32_t* labels, uint64_t* n_communities, double* modularity, uint32_t* n_levels);

// sapca_graph_components_device / sapca_spectral_* / sapca_umap_spectral_init_device_* (spectral.cpp): the components of a graph's
// structure, the scale and one application of S = diag(s) W diag(s), the leading eigenpairs on a resident graph or on host
// arrays, and UMAP's spectral start from eigenvectors
void graph_components(H& h, uint64_t m, uint64_t nnz, const int64_t* ptr, const int32_t* idx, int32_t* d_labels, uint64_t* n_components);
template <typename T>
void spectral_scale(H& h, const CsrView<T>& G, uint32_t kind, double* d_scale);
template <typename T>
void spectral_apply(H& h, const CsrView<T>& G, uint32_t kind, const double* d_x, double* d_y);
template <typename T>
void spectral_device(H& h, const CsrView<T>& G, const sapca_spectral_options* opts, double* evals, T* d_evecs, uint64_t* n_components,
                     uint32_t* n_steps);
template <typename T>
void spectral_host(H& h, uint64_t m, uint64_t nnz, const int64_t* ptr, const int32_t* idx, const T* val, const sapca_spectral_options* opts,
                   double* evals, T* evecs, uint64_t* n_components, uint32_t* n_steps);
template <typename T>
void umap_spectral_init(H& h, uint64_t m, uint32_t output_dim, const T* d_evecs, uint64_t ld, uint32_t n_eigen, uint32_t seed, T* d_y);

}  // namespace resident
}  // namespace sapca
