// Host staging of sapca_tsne_* (the kernels are tsne.hip's, the neighbour search knn.hip's, the row sort rowsort.h's): argument
// checks, buffer layouts, launches, and neighbour_graph(), the front half of a graph from neighbour lists that UMAP shares.
// Everything that can be refused is refused before anything is enqueued or a buffer is touched.  All work space lives in
// h.tsne: a fitted model, a cached preparation, the upload's statistics, the selection and the canonical buffers are not touched.
#include "resident.h"

namespace sapca {
namespace resident {

namespace {

void check_perplexity(double perplexity, const std::string& w) {
  SAPCA_CHECK(std::isfinite(perplexity) && perplexity >= 1.0, SAPCA_ERR_ARG,
              w + ": perplexity = " + numd(perplexity) + " must be finite and at least 1");
}

// K = floor(3 perplexity), or the refusal
int neighbours_of(double perplexity, uint64_t m, const char* who) {
  const std::string w(who);
  check_perplexity(perplexity, w);
  check_rows(m, w);
  const double k3 = std::floor(3.0 * perplexity);
  SAPCA_CHECK(k3 <= (double)SAPCA_KNN_MAX_NEIGHBORS, SAPCA_ERR_ARG,
              w + ": perplexity " + numd(perplexity) + " needs " + numd(k3) + " neighbours, at most " + num(SAPCA_KNN_MAX_NEIGHBORS));
  const uint64_t K = (uint64_t)k3;
  SAPCA_CHECK(m == 0 || K + 1 <= m, SAPCA_ERR_ARG,
              w + ": perplexity too large for the number of rows (perplexity " + numd(perplexity) + " needs " + num(K) +
                  " neighbours, m = " + num(m) + " rows have " + num(m ? m - 1 : 0) + ")");
  return (int)K;
}

void check_output_dim(uint64_t d, const char* who) {
  SAPCA_CHECK(d >= 1 && d <= 3, SAPCA_ERR_ARG, std::string(who) + ": output_dim = " + num(d) + " is outside 1 .. 3");
}

void check_options(const sapca_tsne_options* o, const char* who) {
  check_options_header(o, "sapca_tsne_options", who);
  check_output_dim(o->output_dim, who);
  SAPCA_CHECK(o->init_given <= 1, SAPCA_ERR_ARG, std::string(who) + ": init_given = " + num(o->init_given) + " is neither 0 nor 1");
  check_constant(o->exaggeration, "exaggeration", who);
  check_constant(o->learning_rate, "learning_rate", who);
  check_constant(o->momentum, "momentum", who);
  check_constant(o->final_momentum, "final_momentum", who);
  SAPCA_CHECK(!std::isnan(o->theta) && o->theta >= 0.0, SAPCA_ERR_ARG, std::string(who) + ": theta = " + numd(o->theta) + " must not be negative");
}

// the scalars of an evaluation in h.tsne.scal (f64): Z | KL | the column means
constexpr int kScalZ = 0, kScalKl = 1, kScalMean = 2, kScalCount = 8;

// one evaluation of stage 4 into h.tsne.grad, scal[kScalZ] and, with_kl, scal[kScalKl]; nothing is read back
template <typename T>
void evaluate(H& h, const CsrView<T>& P, const T* y, int64_t ldy, int D, double exaggeration, const k::TsnePlan& plan, T* grad, bool with_kl) {
  H::Tsne& w = h.tsne;
  const int64_t m = P.rows;
  hipStream_t s = h.stream;
  double* scal = w.scal.as<double>(kScalCount);
  double* rep = w.rep.as<double>((size_t)m * (D + 1));
  double* part = plan.split ? w.part.as<double>((size_t)plan.nchunk * m * (D + 1)) : nullptr;
  double* sum_part = w.sum_part.as<double>(k::tsne_sum_parts(m) + 1);
  double* klrow = w.klrow.as<double>((size_t)m);
  k::tsne_repulsion<T>(y, ldy, m, D, plan, part, rep, sum_part, scal + kScalZ, s);
  k::tsne_attraction<T>(P, y, ldy, D, exaggeration, rep, scal + kScalZ, grad, klrow, s);
  if (with_kl) k::tsne_sum(klrow, m, sum_part, scal + kScalKl, s);
}

template <typename T>
void check_graph(const CsrView<T>& P, const char* who) {
  check_view(P);
  SAPCA_CHECK(P.rows == P.cols, SAPCA_ERR_ARG, std::string(who) + ": the affinity matrix must be square");
}

}  // namespace

RawGraph neighbour_graph(H& h, H::NeighbourGraph& g, const std::string& who, uint64_t m, uint32_t K, const int32_t* d_indices,
                         bool dist_given, const std::function<void(double*)>& weights) {
  namespace KK = sapca::k;
  check_rows(m, who);
  SAPCA_CHECK(K >= 1 && K <= SAPCA_KNN_MAX_NEIGHBORS, SAPCA_ERR_ARG,
              who + ": K = " + num(K) + " neighbours per row is outside 1 .. " + num(SAPCA_KNN_MAX_NEIGHBORS));
  SAPCA_CHECK(m == 0 || (d_indices && dist_given), SAPCA_ERR_ARG, who + ": a NULL neighbour list with m = " + num(m));
  hipStream_t s = h.stream;
  h.drop_preparation_of(g);
  const int64_t rows = (int64_t)m;
  const size_t cap = std::max<size_t>((size_t)2 * m * K, 1);
  double* p = g.p.as<double>(std::max<size_t>((size_t)m * K, 1));
  int64_t* raw_ptr = g.raw_ptr.as<int64_t>(m + 1);
  int32_t* nvalid = g.nvalid.as<int32_t>(std::max<size_t>(m, 1));
  int32_t* cursor = g.cursor.as<int32_t>(std::max<size_t>(m, 1));
  int32_t* raw_idx = g.raw_idx.as<int32_t>(cap);
  double* raw_val = g.raw_val.as<double>(cap);
  int32_t* s_idx = g.sort_idx.as<int32_t>(cap);
  RawGraph r;
  r.raw.rows = r.raw.cols = rows;
  r.raw.ptr = r.ptr = raw_ptr;
  r.raw.idx = r.idx = raw_idx;
  r.raw.val = r.val = raw_val;
  if (m == 0) {   // valid: an empty graph
    SAPCA_HIP(hipMemsetAsync(raw_ptr, 0, sizeof(int64_t), s));
    SAPCA_HIP(hipStreamSynchronize(s));
    return r;
  }
  weights(p);
  KK::tsne_count(d_indices, rows, (int)K, raw_ptr, nvalid, s);
  KK::exclusive_scan_i64(raw_ptr, rows + 1, g.sort.scan, 0, s);
  SAPCA_HIP(hipMemcpyAsync(&r.raw.nnz, raw_ptr + rows, sizeof(int64_t), hipMemcpyDeviceToHost, s));
  SAPCA_HIP(hipStreamSynchronize(s));
  KK::tsne_emit(d_indices, p, rows, (int)K, raw_ptr, nvalid, cursor, raw_idx, raw_val, s);
  r.nnz = (uint64_t)r.raw.nnz;
  // rows by ascending column; the offsets are this call's own.  (No valid slot at all: an empty graph, nothing to sort.)
  if (r.nnz == 0 || !g.sort.survey(r.raw, true, false, s) || !g.sort.needs_sort()) return r;
  double* s_val = g.sort_val.as<double>(cap);
  SAPCA_HIP(hipMemcpyAsync(s_idx, raw_idx, r.nnz * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
  SAPCA_HIP(hipMemcpyAsync(s_val, raw_val, r.nnz * sizeof(double), hipMemcpyDeviceToDevice, s));
  r.merged = g.sort.sort(r.raw, s_idx, s_val, s);
  r.sorted = true;
  r.idx = s_idx;
  r.val = s_val;
  if (r.merged) {
    int64_t* n_ptr = g.out_ptr.as<int64_t>(m + 1);
    g.sort.merged_offsets(raw_ptr, rows, n_ptr, s);
    r.ptr = n_ptr;
    r.nnz -= r.merged;
  }
  return r;
}

// stages 2-3 on caller-supplied neighbour lists: p_j|i as the weights, p_j|i and p_i|j of a mutual pair added (in f64), / 2m
template <typename T>
void tsne_affinities(H& h, uint64_t m, const int32_t* d_indices, const T* d_dist, uint32_t K, double perplexity, uint64_t* nnz_out,
                     const int64_t** d_ptr, const int32_t** d_idx, T** d_val, double* d_beta) {
  namespace KK = sapca::k;
  const std::string who("tsne_affinities");
  SAPCA_CHECK(nnz_out && d_ptr && d_idx && d_val, SAPCA_ERR_ARG, who + ": null output pointer");
  check_perplexity(perplexity, who);
  H::NeighbourGraph& g = h.tsne.graph;
  hipStream_t s = h.stream;
  RawGraph r = neighbour_graph(h, g, who, m, K, d_indices, d_dist != nullptr, [&](double* p) {
    KK::tsne_perplexity<T>(d_indices, d_dist, (int64_t)m, (int)K, perplexity, p, d_beta, s);
  });
  if (r.merged) {   // (the raw arrays have been gathered from: they take the merged rows)
    KK::canon_merge_fill(r.raw.ptr, r.idx, r.val, r.raw.rows, r.ptr, g.raw_idx.ptr<int32_t>(), g.raw_val.ptr<double>(), s);
    r.idx = r.raw.idx;
    r.val = r.raw.val;
  }
  T* out_val = g.out_val.as<T>(std::max<size_t>(r.nnz, 1));
  if (m) {
    KK::tsne_scale<T>(r.val, (int64_t)r.nnz, 1.0 / (2.0 * (double)m), out_val, s);
    SAPCA_HIP(hipStreamSynchronize(s));   // complete when the call returns
  }
  *nnz_out = r.nnz;
  *d_ptr = r.ptr;
  *d_idx = r.idx;
  *d_val = out_val;
}

// one evaluation of stage 4
template <typename T>
void tsne_gradient(H& h, const CsrView<T>& P, const T* d_y, uint64_t ldy, uint32_t output_dim, double exaggeration, T* d_grad, double* Z,
                   double* kl) {
  const char* who = "tsne_gradient";
  check_output_dim(output_dim, who);
  check_constant(exaggeration, "exaggeration", who);
  check_graph(P, who);
  SAPCA_CHECK(ldy >= output_dim, SAPCA_ERR_ARG, std::string(who) + ": ldy = " + num(ldy) + " is less than output_dim = " + num(output_dim));
  check_stride_limit(ldy, who);
  if (P.rows == 0) {
    if (Z) *Z = 0.0;
    if (kl) *kl = 0.0;
    return;
  }
  SAPCA_CHECK(d_y != nullptr && d_grad != nullptr, SAPCA_ERR_ARG, std::string(who) + ": a NULL panel with m = " + num((uint64_t)P.rows));
  const k::TsnePlan plan = k::tsne_plan(P.rows, cu_count(h));
  evaluate<T>(h, P, d_y, (int64_t)ldy, (int)output_dim, exaggeration, plan, d_grad, true);
  double out[2] = {0.0, 0.0};
  SAPCA_HIP(hipMemcpyAsync(out, h.tsne.scal.ptr<double>(), sizeof(out), hipMemcpyDeviceToHost, h.stream));
  SAPCA_HIP(hipStreamSynchronize(h.stream));
  if (Z) *Z = out[kScalZ];
  if (kl) *kl = out[kScalKl];
}

// stage 5.  The epoch loop enqueues kernels only: Z, the means and the Kullback-Leibler terms stay on the device.
template <typename T>
void tsne_embed(H& h, const CsrView<T>& P, const sapca_tsne_options* opts, T* d_y, double* kl) {
  const char* who = "tsne_embed";
  check_options(opts, who);
  check_graph(P, who);
  const int64_t m = P.rows;
  if (m == 0) {
    if (kl) *kl = 0.0;
    return;
  }
  SAPCA_CHECK(d_y != nullptr, SAPCA_ERR_ARG, std::string(who) + ": d_y is NULL with m = " + num((uint64_t)m));
  const int D = (int)opts->output_dim;
  H::Tsne& w = h.tsne;
  hipStream_t s = h.stream;
  const k::TsnePlan plan = k::tsne_plan(m, cu_count(h));
  const size_t n = (size_t)m * D;
  T* v = w.v.as<T>(n);
  T* gain = w.gain.as<T>(n);
  T* grad = w.grad.as<T>(n);
  double* scal = w.scal.as<double>(kScalCount);
  double* colpart = w.colpart.as<double>((size_t)((m + 255) / 256) * D);
  k::tsne_init_state<T>(opts->init_given ? nullptr : d_y, v, gain, m, D, opts->random_seed, s);
  k::tsne_center<T>(d_y, m, D, colpart, scal + kScalMean, true, s);
  for (uint64_t t = 0; t < opts->epochs; ++t) {
    const double e = t < opts->stop_lying_epoch ? opts->exaggeration : 1.0;
    const double mu = t < opts->momentum_switch_epoch ? opts->momentum : opts->final_momentum;
    evaluate<T>(h, P, d_y, D, D, e, plan, grad, false);
    k::tsne_update<T>(d_y, v, gain, grad, m, D, mu, opts->learning_rate, colpart, scal + kScalMean, s);
  }
  evaluate<T>(h, P, d_y, D, D, 1.0, plan, grad, true);
  double out[2] = {0.0, 0.0};
  SAPCA_HIP(hipMemcpyAsync(out, scal, sizeof(out), hipMemcpyDeviceToHost, s));
  SAPCA_HIP(hipStreamSynchronize(s));
  if (kl) *kl = out[kScalKl];
}

// stages 1-5 on a resident panel
template <typename T>
void tsne_device(H& h, uint64_t m, const T* d_x, uint64_t ldx, uint64_t d, const sapca_tsne_options* opts, T* d_y, double* kl) {
  const char* who = "tsne";
  check_options(opts, who);
  const int K = neighbours_of(opts->perplexity, m, who);
  check_panel(d, ldx, "ldx", who);   // (refused before a buffer is sized; knn<T> checks them again, after)
  if (m == 0) {
    if (kl) *kl = 0.0;
    return;
  }
  SAPCA_CHECK(d_x != nullptr && d_y != nullptr, SAPCA_ERR_ARG, std::string(who) + ": a NULL panel with m = " + num(m));
  H::Tsne& w = h.tsne;
  int32_t* nidx = w.knn_idx.as<int32_t>((size_t)m * K);
  T* ndist = w.knn_dist.as<T>((size_t)m * K);
  knn<T>(h, m, d_x, ldx, m, d_x, ldx, d, SAPCA_KNN_EUCLIDEAN, (uint32_t)K, SAPCA_KNN_EXCLUDE_SELF, nidx, ndist);
  CsrView<T> P;
  uint64_t nnz = 0;
  T* pv = nullptr;
  tsne_affinities<T>(h, m, nidx, ndist, (uint32_t)K, opts->perplexity, &nnz, &P.ptr, &P.idx, &pv, nullptr);
  P.rows = P.cols = (int64_t)m;
  P.nnz = (int64_t)nnz;
  P.val = pv;
  tsne_embed<T>(h, P, opts, d_y, kl);
}

// the same with host arrays: x (m x d, row-major) in, y (m x output_dim) in when init_given, out
template <typename T>
void tsne_host(H& h, uint64_t m, uint64_t d, const T* x, const sapca_tsne_options* opts, T* y, double* kl) {
  const char* who = "tsne";
  check_options(opts, who);
  (void)neighbours_of(opts->perplexity, m, who);
  check_panel(d, d, "ldx", who);
  if (m == 0) {
    if (kl) *kl = 0.0;
    return;
  }
  SAPCA_CHECK(x != nullptr && y != nullptr, SAPCA_ERR_ARG, std::string(who) + ": a NULL array with m = " + num(m));
  host_route<T>(h, h.tsne.x, x, (size_t)m * d, h.tsne.y, y, (size_t)m * opts->output_dim, opts->init_given != 0,
                [&](const T* dx, T* dy) { tsne_device<T>(h, m, dx, d, d, opts, dy, kl); });
  SAPCA_HIP(hipStreamSynchronize(h.stream));
}

#define SAPCA_INSTANTIATE_TSNE(T)                                                                                                    \
  template void tsne_affinities<T>(H&, uint64_t, const int32_t*, const T*, uint32_t, double, uint64_t*, const int64_t**, const int32_t**, \
                                   T**, double*);                                                                                     \
  template void tsne_gradient<T>(H&, const CsrView<T>&, const T*, uint64_t, uint32_t, double, T*, double*, double*);                 \
  template void tsne_embed<T>(H&, const CsrView<T>&, const sapca_tsne_options*, T*, double*);                                        \
  template void tsne_device<T>(H&, uint64_t, const T*, uint64_t, uint64_t, const sapca_tsne_options*, T*, double*);                  \
  template void tsne_host<T>(H&, uint64_t, uint64_t, const T*, const sapca_tsne_options*, T*, double*);
SAPCA_INSTANTIATE_TSNE(float)
SAPCA_INSTANTIATE_TSNE(double)
#undef SAPCA_INSTANTIATE_TSNE

}  // namespace resident
}  // namespace sapca
