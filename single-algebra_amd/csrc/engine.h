// The handle behind the C ABI and the typed engine that drives the kernels.
#pragma once
#include <algorithm>
#include <string>
#include <vector>

#include "comm.h"
#include "common.h"
#include "kernels.h"
#include "rowsort.h"

struct sapca_handle_s {
  sapca_options opt{};
  std::string err;
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  hipStream_t stream2 = nullptr;        // side stream: A's format is built beside the transposition (prepare)
  hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_drop = nullptr;
  // third stream: the sums of the columns a mask drops (a sort of the dropped pairs).  Only mean_ reads them, at the end of
  // fit(): single-rank fits let that chain run beside the format builds AND the sweeps, and it copies the statistics to
  // the host itself (ev_kept: the kept columns' sums are in place on the main stream; ev_stats: the host copy has landed)
  hipStream_t stream3 = nullptr;
  hipStream_t stream_comm = nullptr;   // the first piece's all-reduce of an A^T sweep swept in two pieces (multi-rank fits)
  hipEvent_t ev_piece = nullptr, ev_comm = nullptr;
  hipEvent_t ev_kept = nullptr, ev_stats = nullptr;
  bool stats_on_side = false;

  // builder state
  std::vector<uint8_t> mask;
  uint64_t mask_version = 0;
  std::vector<double> omega;  // injected test matrix (rows x cols, row-major)
  size_t omega_rows = 0, omega_cols = 0;

  // per-row covariates (sapca_set_covariates): z as given, rows x cols; empty: none, and nothing below is touched
  std::vector<double> covar_z;
  uint64_t covar_rows = 0, covar_cols = 0;
  // The covariate route of a fit or transform in flight and of the fitted model (engine.cpp, "covariates").  `fit` / `model`
  // describe the design: its columns (z's + the intercept) and the rank of its basis; design == 0: no covariates.
  struct Covar {
    struct Shape { uint64_t cols = 0, design = 0, rank = 0; };
    Shape fit, model;
    std::vector<double> q, w;        // this fit's basis (rows x 16) and its map Q = D W ((cols + center) x 16)
    std::vector<double> w_model;     // ... of the fit that made the model
    int ldc = 0;                     // row stride of covar_c
    std::vector<unsigned char> q_t;  // q, or D_rows W of a transform, in T: what the device copy reads (alive here: no wait for the copy)
    bool active() const { return fit.rank > 0; }   // this fit runs the uncentred sweeps with the projection
  } covar;
  sapca::DevBuf covar_q, covar_g, covar_s;   // Q (m x 16, T), G = A^T Q (n_used x 16, T), S = Q^T Y of a sweep (f64)
  sapca::DevBuf covar_c;                     // C = Q^T A V^T = G^T V^T of the fitted model (16 x ldc, f64)
  sapca::PinnedBuf covar_host;               // G^T G (16 x 16) on its way to the host tail of the fit

  // column scaling (sapca_set_column_scaling): what the NEXT fit applies.  SAPCA_SCALE_NONE: nothing below is touched
  int scale_mode = 0;
  std::vector<double> scale_weights;   // SAPCA_SCALE_WEIGHTS: one per column of the matrix, as given
  // ... of the fit in flight and of the fitted model (engine.cpp, "column scaling"): the factors of the n_used columns stay on the
  // device -- d in f64 (sapca_get_column_scale), d and d mu in T (the sweeps, the projection) -- and only sum_j d_j^2 var_j crosses
  int scale_fit = 0, scale_model = 0;
  sapca::DevBuf scale_in, scale_d64, scale_dt, scale_w, scale_red;   // the weights (full width); d; T(d); T(d mu); partial sums | their total
  sapca::PinnedBuf scale_host;                                        // that total on its way to the host tail of the fit

  // fitted state
  bool fitted = false;
  int dtype = 0;  // 0 = f32, 1 = f64
  uint64_t k = 0, n_used = 0, n_cols = 0, m_fit = 0;
  std::vector<double> sing, expl_var, mean;  // k, k, n_cols
  double total_var = 0;
  std::vector<uint64_t> cols_to_use;
  std::vector<int64_t> orig_to_masked;
  bool has_mask_maps = false;
  int chol_regularised = 0;

  // prepared-operator cache key (the matrix the device-side companions were built from)
  struct PrepKey {
    const void *ptr = nullptr, *idx = nullptr, *val = nullptr;
    uint64_t m = 0, n = 0, nnz = 0, mask_version = 0;
    int dtype = -1;
    bool valid = false;
    bool operator==(const PrepKey& o) const {
      return valid && o.valid && ptr == o.ptr && idx == o.idx && val == o.val && m == o.m && n == o.n && nnz == o.nnz &&
             mask_version == o.mask_version && dtype == o.dtype;
    }
  } prep_key;
  struct RawCsr {
    int64_t rows = 0, cols = 0, nnz = 0;
    const void *ptr = nullptr, *idx = nullptr, *val = nullptr;
  } a_used, at_used;
  uint64_t m_global = 0;
  std::vector<double> prep_mean;  // column means of the prepared matrix (n)
  double prep_total_var = 0;
  uint32_t at_sweep_pieces = 1;   // 2: the last randomized fit swept A^T in two pieces (multi-rank overlap)
  bool lz_scatter = false;        // the prepared Lanczos fit has no transposed operator: its second product scatters into LDS (scatter.hip)
  bool q3_cancels = false;        // a kept column is well filled and of small spread: the masked projection subtracts entry by entry
  // the column sums on the host (sum | sumsq | row count), copied asynchronously: single-rank fits read them at the end
  // of fit() instead of stalling the stream between the preparation and the first sweep
  sapca::PinnedBuf stats_host;
  sapca::PinnedBuf small_host;    // the l x l Gram on its way to the host eigensolver, its factor on the way back
  struct HeldTail {   // fit_transform: fit() returned with its host-side tail (statistics, timings) still to run
    bool pending = false;
    int total_ev = -1;
    int sing_l = 0;   // l: the singular values of the device eigensolver are still on their way (read in finish_fit)
    void reset() { pending = false; sing_l = 0; }
  } held_tail;
  // fit_transform (unmasked f32 randomized fits): fit() returns in front of the host eigensolver of the l x l Gram and
  // transform() runs it once the projection sweep is queued (engine.cpp, finish_small_svd)
  struct HeldSmall {
    bool defer = false, pending = false;
    int l = 0, ld = 0;
    hipEvent_t ev = nullptr;          // the Gram's copy to the host has landed
    std::vector<int> in_transform;    // events of a held-back small SVD that ran inside the projection's span
    void reset() { defer = pending = false; in_transform.clear(); }
  } held_small;
  sapca::PinnedBuf lanczos_host;  // alpha | beta of the Lanczos tridiagonal, read back at each convergence check
  bool stats_pending = false;
  int64_t stats_cols = 0;
  // multi-rank fits: what rides behind the column statistics in their all-reduce -- {this rank's rows, ranks whose vote is
  // in, one vote per rank on the cut of the two-piece A^T sweep} (engine.cpp, column_statistics / fit_randomized)
  static constexpr size_t kStatsTail = 72;
  double stats_tail[kStatsTail] = {};
  bool vote_ready = false;        // every rank's vote came with the statistics: vote_cut is the agreed cut (0: one piece)
  int64_t vote_cut = 0;

  // device buffers (grow-only)
  sapca::DevBuf in_ptr, in_idx, in_val, up64, out_tmp;    // host-entry uploads
  sapca::PinnedBuf up_stage[2];                                   // page-locked ring of the chunked index upload
  hipEvent_t up_done[2] = {nullptr, nullptr};
  // column statistics accumulated chunk by chunk while the upload is in flight (upstats.hip); valid for exactly the
  // matrix in (in_ptr, in_idx, in_val) until one of the library's entry points rewrites its values
  struct UpStats {
    sapca::DevBuf work, out;            // long accumulators; sum | sumsq | count (f64, n each)
    sapca::PinnedBuf flag;              // 1: a value was inf/nan and `out` is void (readable once up_stats_done has passed)
    uint64_t m = 0, n = 0, nnz = 0;
    int dtype = -1;
    bool valid = false;
  } up_stats;
  hipEvent_t up_stats_done = nullptr;
  // the values of the uploaded / the caller's matrix changed: under any cached preparation, and under the upload's statistics
  void values_changed() { prep_key.valid = false; up_stats.valid = false; }
  // a preparation cached for a result (selection, canonical) whose arrays are about to change describes them no longer; any other stays
  template <typename R>
  void drop_preparation_of(const R& result) {
    if (prep_key.valid && (result.owns(prep_key.ptr) || result.owns(prep_key.idx) || result.owns(prep_key.val))) prep_key.valid = false;
  }
  // the row selection of sapca_select_rows_csr_device_*: a CSR of its own beside the upload's, the row list on the device and the
  // scan's work space (nothing else lives in these, so a selection disturbs no cached preparation but one made OF it)
  // (gather / spans / cmap: the gathered offsets, the per-span counts and the column map of sapca_select_submatrix_csr_device_*)
  struct Selection {
    sapca::DevBuf ptr, idx, val, rows, scan, gather, spans, cmap;
    bool owns(const void* q) const { return ptr.contains(q) || idx.contains(q) || val.contains(q); }   // the result's arrays, not the work space
  } selection;
  // the canonical form of sapca_canonicalize_csr_device_*: a third CSR beside the upload's and the selection's (idx2 / val2
  // hold it when duplicates merged: the fill's output), and the work space of the check and the row sort (rowsort.h)
  struct Canonical {
    sapca::DevBuf ptr, idx, val, idx2, val2;
    sapca::resident::RowSort sort;
    bool owns(const void* q) const {
      return ptr.contains(q) || idx.contains(q) || val.contains(q) || idx2.contains(q) || val2.contains(q);
    }
  } canonical;
  // sapca_knn_device_*: the unit rows of the two panels, the corpus bias, the per-split lists and the merged selection
  // (nothing else lives in these: a search disturbs no fitted model, preparation or statistics)
  struct Knn {
    sapca::DevBuf unit_q, unit_c, bias, part_sc, part_ix, merged;
  } knn;
  // a symmetric graph built from neighbour lists (tsne.cpp, neighbour_graph): the per-slot weights (p) and the emitted entries
  // (raw_*), the row sort's copies, work space and merged offsets, and the graph handed back: one of raw_ptr / out_ptr, one of
  // raw_idx / sort_idx, out_val
  struct NeighbourGraph {
    sapca::DevBuf p, raw_ptr, nvalid, cursor, raw_idx, raw_val, sort_idx, sort_val, out_ptr, out_val;
    sapca::resident::RowSort sort;
    bool owns(const void* q) const {
      return raw_ptr.contains(q) || out_ptr.contains(q) || raw_idx.contains(q) || sort_idx.contains(q) || out_val.contains(q);
    }
  };
  // sapca_tsne_*: the symmetric P and what built it, the optimiser's state and sums, and the panels of the host and one-call
  // routes.  Nothing else lives in these.
  struct Tsne {
    NeighbourGraph graph;
    sapca::DevBuf part, rep, sum_part, scal, klrow, grad, v, gain, colpart, knn_idx, knn_dist, x, y;
  } tsne;
  // sapca_kmeans_*: the norms of the centroids and the rows, the list of ambiguous rows, the two label generations of the loop, the
  // counting sort's counts, offsets, scan space and row order, the slices' sums, the control block and the scalars, the seeding's
  // distances and block sums, and the arrays of the host route.  Nothing else lives in these.
  struct Kmeans {
    sapca::DevBuf bias, xb, amb, lab0, lab1, cnt, tab, scan, order, partial, shiftpart, ctl, scal, rowd, sum_part, colpart, cols;
    sapca::DevBuf rows, seed_dist, seed_bsum, x, cen, labels;
  } kmeans;
  // sapca_harmony_*: the unit rows, R, Y, dist and the penalty table, O / rs / Pr, the batch counts, offsets and sorted rows, the
  // update order's keys, permutations and the sort's work space, the slices' sums, beta, the objective's rows, sums and scalars,
  // and the panels of the host route.  Nothing else lives in these (init = KMEANS runs sapca_kmeans_device_* in its own).
  struct Harmony {
    sapca::DevBuf zc, r, y, dist, pen, o, rs, pr, cnt, seg, by_batch, key32, key32_out, val32, hkey, hkey_out, iota, perm, key2, keys,
        list, sort_tmp, partial, colsum, beta, rowd, sum_part, scal, labels, x, zcorr, batch, rhost;
  } harmony;
  // sapca_umap_*: the fuzzy union and what built it (a graph of its own: a t-SNE call never disturbs it), the row sums and their
  // total, the layout's schedule, its second embedding buffer, and the arrays of the host and one-call routes.  Nothing else
  // lives in these.
  struct Umap {
    NeighbourGraph graph;
    sapca::DevBuf rowsum, sum_part, scal, next, nextn, y2, minmax, knn_idx, knn_dist, x, y;
  } umap;
  // sapca_louvain_*: the row lists per length class and the long rows' keys (of the level's graph, and `2` of the coarse rows
  // before their merge), the vertex sort's keys, k, s and (tot / S)^2 per vertex, the two generations of labels and totals, the
  // anchor bytes, the control block, the renumbering and the aggregation's counts, places and unmerged coarse rows, the two
  // coarse graphs that alternate from level to level (the aggregate call's result is set 0), the composed labels of the host
  // route and its graph.  Nothing else lives in these.
  struct Louvain {
    sapca::DevBuf lists, long_off, ctr, keys, skeys, k, srow, sq, sum_part, tot0, tot1, lab0, lab1, anchored, ctl, scan;
    sapca::DevBuf flag, renum, cnt, rawcnt, pos, raw_ptr, raw_idx, raw_val, lists2, long_off2, keys2, cnt2;
    sapca::DevBuf agg_ptr[2], agg_idx[2], agg_val[2], in_ptr, in_idx, in_val, labels;
    bool owns(const void* q) const {
      return agg_ptr[0].contains(q) || agg_idx[0].contains(q) || agg_val[0].contains(q) || agg_ptr[1].contains(q) ||
             agg_idx[1].contains(q) || agg_val[1].contains(q);
    }
  } louvain;
  // sapca_graph_components_device / sapca_spectral_* / sapca_umap_spectral_init_device_*: the parents, the changed word, the root
  // flags and their scan space; the scale (q | t | s), the scaled f64 copy of the values and the solve's safe copy of the columns; the
  // labels of a solve, the locked table (t | 1 / norm | lock_of), the Lanczos basis with the locked vectors in front, w, h1 | h2 |
  // alpha | beta | partial sums, the Ritz matrix and vectors, the signs; the graph and eigenvectors of the host route; the
  // start's maximum.  Nothing else lives in these.
  struct Spectral {
    sapca::DevBuf parent, changed, flag, scan, scale, wt, safe_idx, labels, lock_tab, basis, w, small, ritz_s, ritz_v, signs;
    sapca::DevBuf in_ptr, in_idx, in_val, evecs, mx;
    sapca::PinnedBuf host;
  } spectral;
  // sapca_rank_sums_csr_device_* / sapca_rank_groups_csr_device_*: the group sizes, the rank pass's results (rank sums | tie sums |
  // counts), the long columns' list and segment offsets, and their key scratch (keys, labels, counts, the sort's work space).
  // Nothing else lives in these; the transposition and the moments use at_* and batch_out as sapca_batch_stats_csr_device_* does.
  struct Rank {
    sapca::DevBuf group, out, list, scratch;
  } rank;
  // sapca_hvg_*_csr_device_* / sapca_loess_f64: the batch sizes, the n-sized f64 work arrays of a call with the sort's index
  // arrays and a counter behind them, and the sort's work space.  Nothing else lives in these; the transposition uses at_*.
  struct Hvg {
    sapca::DevBuf group, vec, sort;
  } hvg;
  sapca::DevBuf at_ptr, at_idx, at_val;                          // A^T
  sapca::DevBuf ca_ptr, ca_idx, ca_val, cat_ptr, cat_idx, cat_val;  // mask-compacted A, A^T
  sapca::DevBuf drop_stats, drop_tmp;                              // their sums (sum | sumsq, full width) and the sort's work space
  sapca::DevBuf drop_col, drop_val;                                // the entries the compaction dropped, as (column, value) pairs
  sapca::DevBuf scratch, scratch2;
  sapca::DevBuf panel_x, panel_y, panel_w, panel_xs, panel_wide;   // (panel_wide: the out-of-place product of a panel wider than 128 columns)
  sapca::DevBuf small;                                           // (laid out by sapca::SmallLayout)
  sapca::DevBuf stats;                                           // sum, sumsq, cnt (f64, n each)
  sapca::DevBuf batch_in, batch_out;                             // per-batch statistics / top-n: codes or ns; results
  sapca::DevBuf mean_used_dev, o2m_dev, sel_rows_dev;
  sapca::DevBuf components_dev;                                  // k x n_used, T
  sapca::DevBuf lanczos_buf;
  sapca::DevBuf lz_mu;                                           // f64 column means of the operator's columns (centred Lanczos fits)
  sapca::DevBuf idx16_a, idx16_b;                                 // 2-byte index copies of the two operators of a Lanczos step
  sapca::TiledBuffers tb_a, tb_at;                               // tile-major formats for the LDS-staged sweep
  sapca::TiledOp tiled_a, tiled_at;
  sapca::DevBuf split_scratch, split_scratch2, votes, lz_scalars;

  sapca::EventTimer timer;
  std::vector<std::pair<int, int>> spans;  // (category, event index) of the last fit/transform
  sapca_timings timings{};
  sapca::Comm comm;
};

namespace sapca {

// The handle's small f64 buffer as a view bound to its base address: six ld x ld matrices (slot stride ld * ld), then -- at
// offsets laid out for panels of W = max(ld, 128) columns -- an int, the centring vectors c | s of the sweeps (T, W entries
// each) and W doubles of column sums a Gram pass gathers.  `behind`: doubles wanted behind the layout (Lanczos' Ritz matrix).
// A function acquires the buffer ONCE, by constructing the view.  DevBuf::ensure frees and reallocates when asked for more
// than it holds, so a slot's contents outlive the next acquisition only because that one asks for the same ld: info and c
// across every normalize() of a randomized fit; the Gram across the host eigensolver and M from finish_small_svd() to the
// rotation of the un-rotated projection (both acquire with held_small.ld, the fit's ld).
struct SmallLayout {
  size_t ld, W;
  double* base;
  SmallLayout(DevBuf& buf, int ld_, size_t behind = 0)
      : ld((size_t)ld_), W((size_t)std::max(ld_, 128)), base(buf.as<double>(6 * W * W + 64 + 4 * W + behind)) {}
  double* slot(size_t i) const { return base + i * ld * ld; }
  double* gram() const { return slot(0); }
  double* r_inv() const { return slot(1); }
  double* r_scratch() const { return slot(2); }
  double* r1() const { return slot(3); }
  double* r2() const { return slot(4); }
  double* m() const { return slot(5); }   // the small factor M (ld x ldk)
  int* info() const { return reinterpret_cast<int*>(base + 6 * W * W); }
  template <typename T> T* c() const { return reinterpret_cast<T*>(base + 6 * W * W + 64); }
  template <typename T> T* s() const { return c<T>() + W; }
  double* wsum() const { return base + 6 * W * W + 64 + 2 * W; }
  double* behind() const { return base + 6 * W * W + 64 + 4 * W; }
};

// The three arrays of a CSR with `rows` rows and room for `cap` entries, in grow-only buffers of the handle.
template <typename T>
struct CsrBuf {
  int64_t* ptr; int32_t* idx; T* val;
  sapca_handle_s::RawCsr raw(int64_t rows, int64_t cols, int64_t nnz) const { return {rows, cols, nnz, ptr, idx, val}; }
};
template <typename T>
CsrBuf<T> csr_buffers(DevBuf& ptr, DevBuf& idx, DevBuf& val, int64_t rows, int64_t cap) {
  const size_t entries = (size_t)std::max<int64_t>(cap, 1);
  return {ptr.as<int64_t>((size_t)rows + 1), idx.as<int32_t>(entries), val.as<T>(entries)};
}

// A^T in natural row order in the handle's at_*, on the main stream; no wait.  Those buffers are shared with prepare(), so
// whatever preparation the handle had cached is gone.
template <typename T>
CsrView<T> transpose_into_at(sapca_handle_s& h, const CsrView<T>& A) {
  h.prep_key.valid = false;
  const CsrBuf<T> at = csr_buffers<T>(h.at_ptr, h.at_idx, h.at_val, A.cols, A.nnz);
  k::transpose_csr(A, at.ptr, at.idx, at.val, h.scratch, h.stream);
  return CsrView<T>{A.cols, A.rows, A.nnz, at.ptr, at.idx, at.val};
}

// Covariates: the host-side checks of a fit (fit = true; then_transform: a fit_transform) or a transform of an m-row matrix
// against the covariates set on the handle and those of the fitted model.  Enqueues nothing; throws SAPCA_ERR_ARG.
void covar_check(sapca_handle_s& h, uint64_t m, bool fit, bool then_transform);
// Column scaling: the same for the scaling set on the handle (a fit of an m x n matrix) or the fitted model's (a transform).
void scale_check(sapca_handle_s& h, uint64_t m, uint64_t n, bool fit, bool then_transform);

// What a normalisation takes beyond its panel.
template <typename T>
struct NormalizeExtras {
  double *R1 = nullptr, *R2 = nullptr;       // ld x ld f64 device: receive the upper factor of the first / second CholeskyQR pass
  int passes = 0;                            // 0: what the normaliser implies (QR two, LU one)
  const k::PanelSource<T>* src = nullptr;    // the panel is still as its producer left it: the first Gram applies the rest
  const T* w = nullptr;                      // weights of vec_out (null: ones)
  T* vec_out = nullptr;                      // receives sum_r w[r] Q[r][:] of the normalised panel
  bool behind_sweep = false;                 // timings: nothing was queued since the sweep's Scope closed (Scope, behind_last)
};

template <typename T>
struct Engine {
  using H = sapca_handle_s;
  static constexpr int kDtype = sizeof(T) == 8 ? 1 : 0;
  static void prepare(H& h, const CsrView<T>& A);
  static void finish_statistics(H& h);   // host side of R3 from stats_host (mean, total variance)
  static void fit(H& h, const CsrView<T>& A, bool defer_finish = false);
  static void finish_small_svd(H& h, const double** sign_out);   // host half of the f32 small SVD (R11) + svd_flip
  static void finish_fit(H& h);          // host-side tail of fit(): statistics, timings (after the last wait for the device)
  static void transform(H& h, const CsrView<T>& A, T* d_out);
  static void fit_randomized(H& h);
  static void fit_lanczos(H& h, bool centred);
  static bool vote_rides(const H& h);          // the cut of the two-piece A^T sweep is agreed inside the statistics' all-reduce
  static int64_t piece_vote(H& h, int ld);     // this rank's vote: the first output row of its second piece, 0 = one piece
  // normaliser on a rows x ld panel
  static void normalize(H& h, T* P, int64_t rows, int l, int ld, int normalizer, bool sharded, const NormalizeExtras<T>& x);
  // components (k x n, in components_dev) = svd_flip((X M)^T) of an n x ld panel X and the ld x round_up(k, 16) factor M
  static void rotate_into_components(H& h, const T* X, int64_t n, int ld, int k, const double* Mdev, const double** sign_out = nullptr);
  static CsrView<T> view(const H::RawCsr& r) {
    CsrView<T> v;
    v.rows = r.rows; v.cols = r.cols; v.nnz = r.nnz;
    v.ptr = static_cast<const int64_t*>(r.ptr);
    v.idx = static_cast<const int32_t*>(r.idx);
    v.val = static_cast<const T*>(r.val);
    return v;
  }
};

}  // namespace sapca
