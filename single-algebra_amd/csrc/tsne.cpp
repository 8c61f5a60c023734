// Host staging of sapca_tsne_* (the kernels are tsne.hip's, the neighbour search knn.hip's, the row sort canon.hip's): argument
// checks, buffer layouts, launches.  Everything that can be refused is refused before anything is enqueued or a buffer is
// touched.  All work space lives in h.tsne: a fitted model, a cached preparation, the upload's statistics, the selection and
// the canonical buffers are not touched.
#include <cmath>

#include "resident.h"

namespace sapca {
namespace resident {

namespace {

std::string num(uint64_t v) { return std::to_string(v); }
std::string numd(double v) {
  char buf[40];
  std::snprintf(buf, sizeof(buf), "%g", v);
  return buf;
}

// K = floor(3 perplexity), or the refusal
int neighbours_of(double perplexity, uint64_t m, const char* who) {
  const std::string w(who);
  SAPCA_CHECK(std::isfinite(perplexity) && perplexity >= 1.0, SAPCA_ERR_ARG,
              w + ": perplexity = " + numd(perplexity) + " must be finite and at least 1");
  SAPCA_CHECK(m < (1ull << 31), SAPCA_ERR_ARG, w + ": m = " + num(m) + " rows; 2^31 or more are not supported");
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

void check_constant(double v, const char* name, const char* who) {
  SAPCA_CHECK(std::isfinite(v) && v >= 0.0, SAPCA_ERR_ARG,
              std::string(who) + ": " + name + " = " + numd(v) + " must be finite and not negative");
}

void check_options(const sapca_tsne_options* o, const char* who) {
  SAPCA_CHECK(o != nullptr, SAPCA_ERR_ARG, std::string(who) + ": null options");
  SAPCA_CHECK(o->struct_size == sizeof(sapca_tsne_options), SAPCA_ERR_ARG,
              std::string(who) + ": options->struct_size is " + num(o->struct_size) + ", this library's sapca_tsne_options has " +
                  num(sizeof(sapca_tsne_options)) + " bytes");
  check_output_dim(o->output_dim, who);
  SAPCA_CHECK(o->init_given <= 1, SAPCA_ERR_ARG, std::string(who) + ": init_given = " + num(o->init_given) + " is neither 0 nor 1");
  check_constant(o->exaggeration, "exaggeration", who);
  check_constant(o->learning_rate, "learning_rate", who);
  check_constant(o->momentum, "momentum", who);
  check_constant(o->final_momentum, "final_momentum", who);
  SAPCA_CHECK(!std::isnan(o->theta) && o->theta >= 0.0, SAPCA_ERR_ARG, std::string(who) + ": theta = " + numd(o->theta) + " must not be negative");
}

// the limits of the neighbour search on a panel's width and row stride, checked here so that they are refused before a
// buffer is sized (knn<T> checks them again, after)
void check_panel(uint64_t d, uint64_t ld, const char* ldname, const char* who) {
  const std::string w(who);
  SAPCA_CHECK(d != 0, SAPCA_ERR_ARG, w + ": d is 0");
  SAPCA_CHECK(d <= 1024, SAPCA_ERR_ARG, w + ": d = " + num(d) + " exceeds 1024 columns");
  SAPCA_CHECK(ld >= d, SAPCA_ERR_ARG, w + ": " + ldname + " = " + num(ld) + " is less than d = " + num(d));
  SAPCA_CHECK(ld < (1ull << 28), SAPCA_ERR_ARG,
              w + ": a row stride of " + num(ld) + " elements; 2^28 or more are not supported");
}

int cu_count(H& h) {
  int n = 0;
  SAPCA_HIP(hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, h.device));
  return n;
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

// stages 2-3 on caller-supplied neighbour lists
template <typename T>
void tsne_affinities(H& h, uint64_t m, const int32_t* d_indices, const T* d_dist, uint32_t K, double perplexity, uint64_t* nnz_out,
                     const int64_t** d_ptr, const int32_t** d_idx, T** d_val, double* d_beta) {
  namespace KK = sapca::k;
  const char* who = "tsne_affinities";
  SAPCA_CHECK(nnz_out && d_ptr && d_idx && d_val, SAPCA_ERR_ARG, std::string(who) + ": null output pointer");
  SAPCA_CHECK(std::isfinite(perplexity) && perplexity >= 1.0, SAPCA_ERR_ARG,
              std::string(who) + ": perplexity = " + numd(perplexity) + " must be finite and at least 1");
  SAPCA_CHECK(m < (1ull << 31), SAPCA_ERR_ARG, std::string(who) + ": m = " + num(m) + " rows; 2^31 or more are not supported");
  SAPCA_CHECK(K >= 1 && K <= SAPCA_KNN_MAX_NEIGHBORS, SAPCA_ERR_ARG,
              std::string(who) + ": K = " + num(K) + " neighbours per row is outside 1 .. " + num(SAPCA_KNN_MAX_NEIGHBORS));
  SAPCA_CHECK(m == 0 || (d_indices && d_dist), SAPCA_ERR_ARG, std::string(who) + ": a NULL neighbour list with m = " + num(m));
  H::Tsne& w = h.tsne;
  hipStream_t s = h.stream;
  h.drop_preparation_of(w);
  const int64_t rows = (int64_t)m;
  const size_t cap = std::max<size_t>((size_t)2 * m * K, 1);
  double* p = w.p.as<double>(std::max<size_t>((size_t)m * K, 1));
  int64_t* raw_ptr = w.raw_ptr.as<int64_t>(m + 1);
  int32_t* nvalid = w.nvalid.as<int32_t>(std::max<size_t>(m, 1));
  int32_t* cursor = w.cursor.as<int32_t>(std::max<size_t>(m, 1));
  int32_t* raw_idx = w.raw_idx.as<int32_t>(cap);
  double* raw_val = w.raw_val.as<double>(cap);
  if (m == 0) {   // valid: an empty graph
    SAPCA_HIP(hipMemsetAsync(raw_ptr, 0, sizeof(int64_t), s));
    SAPCA_HIP(hipStreamSynchronize(s));
    *nnz_out = 0;
    *d_ptr = raw_ptr;
    *d_idx = raw_idx;
    *d_val = w.out_val.as<T>(1);
    return;
  }
  KK::tsne_perplexity<T>(d_indices, d_dist, rows, (int)K, perplexity, p, d_beta, s);
  KK::tsne_count(d_indices, rows, (int)K, raw_ptr, nvalid, s);
  KK::exclusive_scan_i64(raw_ptr, rows + 1, w.scan, 0, s);
  int64_t nnz_raw = 0;
  SAPCA_HIP(hipMemcpyAsync(&nnz_raw, raw_ptr + rows, sizeof(int64_t), hipMemcpyDeviceToHost, s));
  SAPCA_HIP(hipStreamSynchronize(s));
  KK::tsne_emit(d_indices, p, rows, (int)K, raw_ptr, nvalid, cursor, raw_idx, raw_val, s);

  // rows by ascending column, p_j|i and p_i|j of a mutual pair added (in f64): the sequence of resident::canonicalize, in
  // buffers of this call's own
  CsrView<double> A;
  A.rows = rows; A.cols = rows; A.nnz = nnz_raw; A.ptr = raw_ptr; A.idx = raw_idx; A.val = raw_val;
  unsigned long long ctr_host[KK::kCtrSlots] = {};
  unsigned long long* ctr = w.ctr.as<unsigned long long>(KK::kCtrSlots);
  uint32_t* row_bits = w.rows.as<uint32_t>((size_t)std::max<int64_t>(5 * rows, 1));
  unsigned long long* long_off = w.long_off.as<unsigned long long>((size_t)std::max<int64_t>(rows, 1));
  if (nnz_raw > 0) {   // (no valid slot at all: an empty graph, nothing to sort)
    KK::canon_check_offsets(A.ptr, rows, A.nnz, ctr, s);
    KK::canon_check_entries(A, row_bits, ctr, s);
    KK::canon_list_rows(A.ptr, row_bits, rows, row_bits + 2 * rows, long_off, ctr, s);
    SAPCA_HIP(hipMemcpyAsync(ctr_host, ctr, KK::kCtrSlots * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    SAPCA_HIP(hipStreamSynchronize(s));
  }
  const int64_t* o_ptr = raw_ptr;
  int32_t* o_idx = raw_idx;
  double* o_val = raw_val;
  uint64_t nnz = (uint64_t)nnz_raw;
  if (nnz_raw > 0 && (ctr_host[KK::kCtrUnsortedRows] || ctr_host[KK::kCtrDuplicates])) {
    int32_t* s_idx = w.sort_idx.as<int32_t>(cap);
    double* s_val = w.sort_val.as<double>(cap);
    SAPCA_HIP(hipMemcpyAsync(s_idx, raw_idx, (size_t)nnz_raw * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    SAPCA_HIP(hipMemcpyAsync(s_val, raw_val, (size_t)nnz_raw * sizeof(double), hipMemcpyDeviceToDevice, s));
    const int64_t counts[3] = {(int64_t)ctr_host[KK::kCtrListWave], (int64_t)ctr_host[KK::kCtrListLds], (int64_t)ctr_host[KK::kCtrListLong]};
    unsigned long long* keys = counts[2] ? w.keys.as<unsigned long long>(ctr_host[KK::kCtrLongEntries]) : nullptr;
    KK::canon_sort_rows(A, row_bits + 2 * rows, long_off, counts, keys, s_idx, s_val, row_bits + rows, ctr, s);
    unsigned long long merged = 0;
    SAPCA_HIP(hipMemcpyAsync(&merged, ctr + KK::kCtrMerged, sizeof(merged), hipMemcpyDeviceToHost, s));
    SAPCA_HIP(hipStreamSynchronize(s));
    o_idx = s_idx;
    o_val = s_val;
    if (merged) {
      int64_t* n_ptr = w.out_ptr.as<int64_t>(m + 1);
      KK::canon_new_lengths(A.ptr, row_bits, row_bits + rows, rows, n_ptr, s);
      KK::exclusive_scan_i64(n_ptr, rows + 1, w.scan, 0, s);
      // (the raw arrays have been gathered from: they take the merged rows)
      KK::canon_merge_fill(A.ptr, s_idx, s_val, rows, n_ptr, raw_idx, raw_val, s);
      o_ptr = n_ptr;
      o_idx = raw_idx;
      o_val = raw_val;
      nnz -= merged;
    }
  }
  T* out_val = w.out_val.as<T>(std::max<size_t>(nnz, 1));
  KK::tsne_scale<T>(o_val, (int64_t)nnz, m ? 1.0 / (2.0 * (double)m) : 0.0, out_val, s);
  SAPCA_HIP(hipStreamSynchronize(s));   // complete when the call returns
  *nnz_out = nnz;
  *d_ptr = o_ptr;
  *d_idx = o_idx;
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
  SAPCA_CHECK(ldy < (1ull << 28), SAPCA_ERR_ARG, std::string(who) + ": a row stride of " + num(ldy) + " elements; 2^28 or more are not supported");
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
  check_panel(d, ldx, "ldx", who);
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
  H::Tsne& w = h.tsne;
  hipStream_t s = h.stream;
  const size_t ny = (size_t)m * opts->output_dim;
  T* dx = w.x.as<T>((size_t)m * d);
  T* dy = w.y.as<T>(ny);
  SAPCA_HIP(hipMemcpyAsync(dx, x, (size_t)m * d * sizeof(T), hipMemcpyHostToDevice, s));
  if (opts->init_given) SAPCA_HIP(hipMemcpyAsync(dy, y, ny * sizeof(T), hipMemcpyHostToDevice, s));
  tsne_device<T>(h, m, dx, d, d, opts, dy, kl);
  SAPCA_HIP(hipMemcpyAsync(y, dy, ny * sizeof(T), hipMemcpyDeviceToHost, s));
  SAPCA_HIP(hipStreamSynchronize(s));
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
