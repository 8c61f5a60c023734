// Host staging of sapca_umap_* (the kernels are umap.hip's, the neighbour search knn.hip's, count / emit tsne.hip's, the row sort
// canon.hip's): argument checks, the curve fit, buffer layouts, launches.  Everything that can be refused is refused before
// anything is enqueued or a buffer is touched.  All work space lives in h.umap: a fitted model, a cached preparation, the
// upload's statistics, the selection, the canonical, the t-SNE and the k-means buffers are not touched.
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

void check_rows(uint64_t m, const std::string& w) {
  SAPCA_CHECK(m < (1ull << 31), SAPCA_ERR_ARG, w + ": m = " + num(m) + " rows; 2^31 or more are not supported");
}

void check_constant(double v, const char* name, const std::string& w) {
  SAPCA_CHECK(std::isfinite(v) && v >= 0.0, SAPCA_ERR_ARG, w + ": " + name + " = " + numd(v) + " must be finite and not negative");
}

// everything about the options that needs no shape; the curve (a, b) comes back fitted where both are 0
void check_options(const sapca_umap_options* o, const char* who, double* a, double* b) {
  const std::string w(who);
  SAPCA_CHECK(o != nullptr, SAPCA_ERR_ARG, w + ": null options");
  SAPCA_CHECK(o->struct_size == sizeof(sapca_umap_options), SAPCA_ERR_ARG,
              w + ": options->struct_size is " + num(o->struct_size) + ", this library's sapca_umap_options has " +
                  num(sizeof(sapca_umap_options)) + " bytes");
  SAPCA_CHECK(o->output_dim >= 1 && o->output_dim <= 3, SAPCA_ERR_ARG, w + ": output_dim = " + num(o->output_dim) + " is outside 1 .. 3");
  SAPCA_CHECK(o->init <= SAPCA_UMAP_INIT_GIVEN, SAPCA_ERR_ARG, w + ": init = " + num(o->init) + " is not a sapca_umap_init");
  SAPCA_CHECK(o->n_neighbors >= 2 && o->n_neighbors <= SAPCA_KNN_MAX_NEIGHBORS + 1, SAPCA_ERR_ARG,
              w + ": n_neighbors = " + num(o->n_neighbors) + " is outside 2 .. " + num(SAPCA_KNN_MAX_NEIGHBORS + 1));
  SAPCA_CHECK(o->negative_sample_rate <= 31, SAPCA_ERR_ARG,
              w + ": negative_sample_rate = " + num(o->negative_sample_rate) + " exceeds 31");
  check_constant(o->learning_rate, "learning_rate", w);
  check_constant(o->repulsion_strength, "repulsion_strength", w);
  SAPCA_CHECK(std::isfinite(o->a) && std::isfinite(o->b) && o->a >= 0.0 && o->b >= 0.0, SAPCA_ERR_ARG,
              w + ": a = " + numd(o->a) + ", b = " + numd(o->b) + " must be finite and not negative");
  SAPCA_CHECK((o->a == 0.0) == (o->b == 0.0), SAPCA_ERR_ARG,
              w + ": a = " + numd(o->a) + ", b = " + numd(o->b) + ": give both, or neither (0, 0) to have them fitted");
  if (o->a == 0.0) {
    umap_find_ab(o->spread, o->min_dist, a, b);
  } else {
    *a = o->a;
    *b = o->b;
  }
}

void check_neighbours_fit(uint32_t n_neighbors, uint64_t m, const std::string& w) {
  SAPCA_CHECK(m == 0 || n_neighbors <= m, SAPCA_ERR_ARG,
              w + ": n_neighbors = " + num(n_neighbors) + " exceeds the m = " + num(m) + " rows");
}

// the limits of the neighbour search on a panel's width and row stride (knn<T> checks them again, after)
void check_panel(uint64_t d, uint64_t ld, const std::string& w) {
  SAPCA_CHECK(d != 0, SAPCA_ERR_ARG, w + ": d is 0");
  SAPCA_CHECK(d <= 1024, SAPCA_ERR_ARG, w + ": d = " + num(d) + " exceeds 1024 columns");
  SAPCA_CHECK(ld >= d, SAPCA_ERR_ARG, w + ": ldx = " + num(ld) + " is less than d = " + num(d));
  SAPCA_CHECK(ld < (1ull << 28), SAPCA_ERR_ARG, w + ": a row stride of " + num(ld) + " elements; 2^28 or more are not supported");
}

void check_init_panel(const sapca_umap_options* o, uint64_t d, const std::string& w) {
  SAPCA_CHECK(o->init != SAPCA_UMAP_INIT_PANEL || d >= o->output_dim, SAPCA_ERR_ARG,
              w + ": SAPCA_UMAP_INIT_PANEL takes the first output_dim = " + num(o->output_dim) + " columns, the panel has d = " + num(d));
}

uint64_t epochs_of(const sapca_umap_options* o, uint64_t m) { return o->epochs ? o->epochs : (m <= 10000 ? 500 : 200); }

// the scalars of a call in h.umap.scal (f64): the panel's total distance | w_max
constexpr int kScalTotal = 0, kScalWmax = 1, kScalCount = 4;

// stage 5; x (the panel of INIT_PANEL, row stride ldx) is null on the embed stage
template <typename T>
void layout(H& h, const CsrView<T>& G, const sapca_umap_options* o, double a, double b, const T* x, uint64_t ldx, T* d_y) {
  namespace KK = sapca::k;
  H::Umap& w = h.umap;
  hipStream_t s = h.stream;
  const int64_t m = G.rows;
  const int D = (int)o->output_dim;
  const uint64_t n_epochs = epochs_of(o, (uint64_t)m);
  double* scal = w.scal.as<double>(kScalCount);
  double* next = w.next.as<double>(std::max<size_t>((size_t)G.nnz, 1));
  double* nextn = w.nextn.as<double>(std::max<size_t>((size_t)G.nnz, 1));
  T* other = w.y2.as<T>((size_t)m * D);
  if (o->init == SAPCA_UMAP_INIT_PANEL) KK::umap_init_panel<T>(x, (int64_t)ldx, m, D, w.minmax.as<double>(8), d_y, s);
  else if (o->init == SAPCA_UMAP_INIT_RANDOM) KK::umap_init_random<T>(d_y, m, D, o->random_seed, s);
  KK::umap_schedule<T>(G.val, G.nnz, (int)o->negative_sample_rate, scal + kScalWmax, next, nextn, s);
  KK::UmapEpoch p;
  p.seed = o->random_seed;
  p.n_epochs = (double)n_epochs;
  p.a = a;
  p.b = b;
  p.gamma = o->repulsion_strength;
  p.rate = (double)o->negative_sample_rate;
  T* cur = d_y;
  T* nxt = other;
  for (uint64_t n = 0; n < n_epochs; ++n) {   // kernels only: nothing is read back
    p.epoch = n;
    p.alpha = o->learning_rate * (1.0 - (double)n / (double)n_epochs);
    KK::umap_epoch<T>(G, cur, nxt, D, p, scal + kScalWmax, next, nextn, s);
    std::swap(cur, nxt);
  }
  if (cur != d_y) SAPCA_HIP(hipMemcpyAsync(d_y, cur, (size_t)m * D * sizeof(T), hipMemcpyDeviceToDevice, s));
  SAPCA_HIP(hipStreamSynchronize(s));   // complete when the call returns
}

template <typename T>
void check_graph(const CsrView<T>& G, const std::string& w) {
  check_view(G);
  SAPCA_CHECK(G.rows == G.cols, SAPCA_ERR_ARG, w + ": the graph must be square");
}

// the two by two system (J^T J + lambda diag) delta = -J^T r of the curve fit at (a, b); returns the cost
struct Normal {
  double saa = 0, sab = 0, sbb = 0, ga = 0, gb = 0, cost = 0;
};
Normal normal_equations(const double* x, const double* y, int n, double a, double b) {
  Normal e;
  for (int t = 0; t < n; ++t) {
    const double xb = x[t] > 0.0 ? std::pow(x[t], 2.0 * b) : 0.0;
    const double f = 1.0 / (1.0 + a * xb);
    const double r = f - y[t];
    const double ja = -xb * f * f;
    const double jb = x[t] > 0.0 ? -2.0 * a * xb * std::log(x[t]) * f * f : 0.0;
    e.saa += ja * ja;
    e.sab += ja * jb;
    e.sbb += jb * jb;
    e.ga += ja * r;
    e.gb += jb * r;
    e.cost += r * r;
  }
  return e;
}
bool solve(const Normal& e, double lambda, double* da, double* db) {
  const double maa = e.saa * (1.0 + lambda), mbb = e.sbb * (1.0 + lambda);
  const double det = maa * mbb - e.sab * e.sab;
  if (!(std::fabs(det) > 0.0) || !std::isfinite(det)) return false;
  *da = (-e.ga * mbb + e.gb * e.sab) / det;
  *db = (-e.gb * maa + e.ga * e.sab) / det;
  return std::isfinite(*da) && std::isfinite(*db);
}

}  // namespace

// umap-learn's find_ab_params: least squares of 1 / (1 + a x^(2b)) to the offset exponential on 300 points of [0, 3 spread],
// from (1, 1).  Every step first looks at the plain Gauss-Newton step: below 1e-12 relative it is taken and the fit has
// converged; otherwise a Levenberg-Marquardt step is tried (a step that raises the cost or leaves a, b > 0 is undone and damped).
void umap_find_ab(double spread, double min_dist, double* a_out, double* b_out) {
  const std::string w("umap_find_ab");
  SAPCA_CHECK(a_out && b_out, SAPCA_ERR_ARG, w + ": null output pointer");
  SAPCA_CHECK(std::isfinite(spread) && spread > 0.0, SAPCA_ERR_ARG, w + ": spread = " + numd(spread) + " must be finite and positive");
  SAPCA_CHECK(std::isfinite(min_dist) && min_dist >= 0.0, SAPCA_ERR_ARG,
              w + ": min_dist = " + numd(min_dist) + " must be finite and not negative");
  SAPCA_CHECK(min_dist < 3.0 * spread, SAPCA_ERR_ARG,
              w + ": min_dist = " + numd(min_dist) + " must be below 3 spread = " + numd(3.0 * spread));
  constexpr int n = 300;
  double x[n], y[n];
  for (int t = 0; t < n; ++t) {
    x[t] = 3.0 * spread * (double)t / 299.0;
    y[t] = x[t] < min_dist ? 1.0 : std::exp(-(x[t] - min_dist) / spread);
  }
  double a = 1.0, b = 1.0, lambda = 1e-3;
  for (int step = 0; step < 200; ++step) {
    const Normal e = normal_equations(x, y, n, a, b);
    double da = 0.0, db = 0.0;
    const bool gn = solve(e, 0.0, &da, &db);
    if (gn && std::fabs(da) <= 1e-12 * std::fabs(a) && std::fabs(db) <= 1e-12 * std::fabs(b)) {
      *a_out = a + da;
      *b_out = b + db;
      return;
    }
    if (gn && std::fabs(da) <= 1e-4 * std::fabs(a) && std::fabs(db) <= 1e-4 * std::fabs(b)) {
      a += da;   // (close in: the cost no longer resolves a step this small, and Gauss-Newton contracts on its own)
      b += db;
      continue;
    }
    if (solve(e, lambda, &da, &db) && a + da > 0.0 && b + db > 0.0 && normal_equations(x, y, n, a + da, b + db).cost <= e.cost) {
      a += da;
      b += db;
      lambda *= 0.1;
    } else {
      lambda = lambda < 1e-12 ? 1e-3 : lambda * 10.0;
    }
  }
  throw Error(SAPCA_ERR_SVD, w + ": the curve fit for spread = " + numd(spread) + ", min_dist = " + numd(min_dist) +
                                 " did not converge in 200 steps");
}

// stages 2-3 on caller-supplied neighbour lists
template <typename T>
void umap_graph(H& h, uint64_t m, const int32_t* d_indices, const T* d_dist, uint32_t K, uint32_t n_neighbors, uint64_t* nnz_out,
                const int64_t** d_ptr, const int32_t** d_idx, T** d_val, double* d_sigma, double* d_rho) {
  namespace KK = sapca::k;
  const std::string who("umap_graph");
  SAPCA_CHECK(nnz_out && d_ptr && d_idx && d_val, SAPCA_ERR_ARG, who + ": null output pointer");
  SAPCA_CHECK(n_neighbors >= 2, SAPCA_ERR_ARG, who + ": n_neighbors = " + num(n_neighbors) + " must be at least 2");
  check_rows(m, who);
  SAPCA_CHECK(K >= 1 && K <= SAPCA_KNN_MAX_NEIGHBORS, SAPCA_ERR_ARG,
              who + ": K = " + num(K) + " neighbours per row is outside 1 .. " + num(SAPCA_KNN_MAX_NEIGHBORS));
  SAPCA_CHECK(m == 0 || (d_indices && d_dist), SAPCA_ERR_ARG, who + ": a NULL neighbour list with m = " + num(m));
  H::Umap& w = h.umap;
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
  int32_t* s_idx = w.sort_idx.as<int32_t>(cap);
  if (m == 0) {   // valid: an empty graph
    SAPCA_HIP(hipMemsetAsync(raw_ptr, 0, sizeof(int64_t), s));
    SAPCA_HIP(hipStreamSynchronize(s));
    *nnz_out = 0;
    *d_ptr = raw_ptr;
    *d_idx = raw_idx;
    *d_val = w.out_val.as<T>(1);
    return;
  }
  double* scal = w.scal.as<double>(kScalCount);
  double* rowsum = w.rowsum.as<double>((size_t)m);
  double* sum_part = w.sum_part.as<double>(KK::tsne_sum_parts(rows) + 1);
  KK::umap_row_sums<T>(d_indices, d_dist, rows, (int)K, rowsum, s);
  KK::tsne_sum(rowsum, rows, sum_part, scal + kScalTotal, s);
  KK::umap_smooth<T>(d_indices, d_dist, rows, (int)K, (int)n_neighbors, scal + kScalTotal, p, d_sigma, d_rho, s);
  KK::tsne_count(d_indices, rows, (int)K, raw_ptr, nvalid, s);
  KK::exclusive_scan_i64(raw_ptr, rows + 1, w.scan, 0, s);
  int64_t nnz_raw = 0;
  SAPCA_HIP(hipMemcpyAsync(&nnz_raw, raw_ptr + rows, sizeof(int64_t), hipMemcpyDeviceToHost, s));
  SAPCA_HIP(hipStreamSynchronize(s));
  KK::tsne_emit(d_indices, p, rows, (int)K, raw_ptr, nvalid, cursor, raw_idx, raw_val, s);

  // rows by ascending column (the sequence of resident::canonicalize, in buffers of this call's own), then the two directions
  // of a pair combined by the fill
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
  const int32_t* in_idx = raw_idx;
  const double* in_val = raw_val;
  int32_t* o_idx = s_idx;
  uint64_t nnz = (uint64_t)nnz_raw;
  if (nnz_raw > 0 && (ctr_host[KK::kCtrUnsortedRows] || ctr_host[KK::kCtrDuplicates])) {
    double* s_val = w.sort_val.as<double>(cap);
    SAPCA_HIP(hipMemcpyAsync(s_idx, raw_idx, (size_t)nnz_raw * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    SAPCA_HIP(hipMemcpyAsync(s_val, raw_val, (size_t)nnz_raw * sizeof(double), hipMemcpyDeviceToDevice, s));
    const int64_t counts[3] = {(int64_t)ctr_host[KK::kCtrListWave], (int64_t)ctr_host[KK::kCtrListLds], (int64_t)ctr_host[KK::kCtrListLong]};
    unsigned long long* keys = counts[2] ? w.keys.as<unsigned long long>(ctr_host[KK::kCtrLongEntries]) : nullptr;
    KK::canon_sort_rows(A, row_bits + 2 * rows, long_off, counts, keys, s_idx, s_val, row_bits + rows, ctr, s);
    unsigned long long merged = 0;
    SAPCA_HIP(hipMemcpyAsync(&merged, ctr + KK::kCtrMerged, sizeof(merged), hipMemcpyDeviceToHost, s));
    SAPCA_HIP(hipStreamSynchronize(s));
    in_idx = s_idx;
    in_val = s_val;
    o_idx = raw_idx;   // (the raw arrays have been gathered from: they take the filled rows)
    if (merged) {
      int64_t* n_ptr = w.out_ptr.as<int64_t>(m + 1);
      KK::canon_new_lengths(A.ptr, row_bits, row_bits + rows, rows, n_ptr, s);
      KK::exclusive_scan_i64(n_ptr, rows + 1, w.scan, 0, s);
      o_ptr = n_ptr;
      nnz -= merged;
    }
  }
  T* out_val = w.out_val.as<T>(std::max<size_t>((size_t)nnz_raw, 1));
  KK::umap_union_fill<T>(raw_ptr, in_idx, in_val, rows, o_ptr, o_idx, out_val, s);
  SAPCA_HIP(hipStreamSynchronize(s));   // complete when the call returns
  *nnz_out = nnz;
  *d_ptr = o_ptr;
  *d_idx = o_idx;
  *d_val = out_val;
}

// stage 5 on a given graph
template <typename T>
void umap_embed(H& h, const CsrView<T>& G, const sapca_umap_options* opts, T* d_y) {
  const char* who = "umap_embed";
  double a = 0.0, b = 0.0;
  check_options(opts, who, &a, &b);
  SAPCA_CHECK(opts->init != SAPCA_UMAP_INIT_PANEL, SAPCA_ERR_ARG,
              std::string(who) + ": init = 0 (SAPCA_UMAP_INIT_PANEL) needs the panel; this stage takes INIT_RANDOM or INIT_GIVEN");
  check_graph(G, who);
  if (G.rows == 0) return;
  SAPCA_CHECK(d_y != nullptr, SAPCA_ERR_ARG, std::string(who) + ": d_y is NULL with m = " + num((uint64_t)G.rows));
  layout<T>(h, G, opts, a, b, nullptr, 0, d_y);
}

// stages 1-5 on a resident panel
template <typename T>
void umap_device(H& h, uint64_t m, const T* d_x, uint64_t ldx, uint64_t d, const sapca_umap_options* opts, T* d_y) {
  const std::string who("umap");
  double a = 0.0, b = 0.0;
  check_options(opts, who.c_str(), &a, &b);
  check_rows(m, who);
  check_neighbours_fit(opts->n_neighbors, m, who);
  check_panel(d, ldx, who);
  check_init_panel(opts, d, who);
  if (m == 0) return;
  SAPCA_CHECK(d_x != nullptr && d_y != nullptr, SAPCA_ERR_ARG, who + ": a NULL panel with m = " + num(m));
  H::Umap& w = h.umap;
  const uint32_t K = opts->n_neighbors - 1;
  int32_t* nidx = w.knn_idx.as<int32_t>((size_t)m * K);
  T* ndist = w.knn_dist.as<T>((size_t)m * K);
  knn<T>(h, m, d_x, ldx, m, d_x, ldx, d, SAPCA_KNN_EUCLIDEAN, K, SAPCA_KNN_EXCLUDE_SELF, nidx, ndist);
  CsrView<T> G;
  uint64_t nnz = 0;
  T* gv = nullptr;
  umap_graph<T>(h, m, nidx, ndist, K, opts->n_neighbors, &nnz, &G.ptr, &G.idx, &gv, nullptr, nullptr);
  G.rows = G.cols = (int64_t)m;
  G.nnz = (int64_t)nnz;
  G.val = gv;
  layout<T>(h, G, opts, a, b, d_x, ldx, d_y);
}

// the same with host arrays: x (m x d, row-major) in, y (m x output_dim) in when INIT_GIVEN, out
template <typename T>
void umap_host(H& h, uint64_t m, uint64_t d, const T* x, const sapca_umap_options* opts, T* y) {
  const std::string who("umap");
  double a = 0.0, b = 0.0;
  check_options(opts, who.c_str(), &a, &b);
  check_rows(m, who);
  check_neighbours_fit(opts->n_neighbors, m, who);
  check_panel(d, d, who);
  check_init_panel(opts, d, who);
  if (m == 0) return;
  SAPCA_CHECK(x != nullptr && y != nullptr, SAPCA_ERR_ARG, who + ": a NULL array with m = " + num(m));
  H::Umap& w = h.umap;
  hipStream_t s = h.stream;
  const size_t ny = (size_t)m * opts->output_dim;
  T* dx = w.x.as<T>((size_t)m * d);
  T* dy = w.y.as<T>(ny);
  SAPCA_HIP(hipMemcpyAsync(dx, x, (size_t)m * d * sizeof(T), hipMemcpyHostToDevice, s));
  if (opts->init == SAPCA_UMAP_INIT_GIVEN) SAPCA_HIP(hipMemcpyAsync(dy, y, ny * sizeof(T), hipMemcpyHostToDevice, s));
  umap_device<T>(h, m, dx, d, d, opts, dy);
  SAPCA_HIP(hipMemcpyAsync(y, dy, ny * sizeof(T), hipMemcpyDeviceToHost, s));
  SAPCA_HIP(hipStreamSynchronize(s));
}

#define SAPCA_INSTANTIATE_UMAP(T)                                                                                                   \
  template void umap_graph<T>(H&, uint64_t, const int32_t*, const T*, uint32_t, uint32_t, uint64_t*, const int64_t**, const int32_t**, \
                              T**, double*, double*);                                                                               \
  template void umap_embed<T>(H&, const CsrView<T>&, const sapca_umap_options*, T*);                                                 \
  template void umap_device<T>(H&, uint64_t, const T*, uint64_t, uint64_t, const sapca_umap_options*, T*);                           \
  template void umap_host<T>(H&, uint64_t, uint64_t, const T*, const sapca_umap_options*, T*);
SAPCA_INSTANTIATE_UMAP(float)
SAPCA_INSTANTIATE_UMAP(double)
#undef SAPCA_INSTANTIATE_UMAP

}  // namespace resident
}  // namespace sapca
