// Host staging of sapca_umap_* (the kernels are umap.hip's, the neighbour search knn.hip's, the graph's front half tsne.cpp's
// neighbour_graph): argument checks, the curve fit, buffer layouts, launches.  Everything that can be refused is refused before
// anything is enqueued or a buffer is touched.  All work space lives in h.umap: a fitted model, a cached preparation, the
// upload's statistics, the selection, the canonical, the t-SNE and the k-means buffers are not touched.
#include "resident.h"

namespace sapca {
namespace resident {

namespace {

// everything about the options that needs no shape; the curve (a, b) comes back fitted where both are 0
void check_options(const sapca_umap_options* o, const char* who, double* a, double* b) {
  const std::string w(who);
  check_options_header(o, "sapca_umap_options", w);
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
  H::Umap& w = h.umap;
  H::NeighbourGraph& g = w.graph;
  hipStream_t s = h.stream;
  const int64_t rows = (int64_t)m;
  const RawGraph r = neighbour_graph(h, g, who, m, K, d_indices, d_dist != nullptr, [&](double* p) {   // the memberships
    double* scal = w.scal.as<double>(kScalCount);
    double* rowsum = w.rowsum.as<double>((size_t)m);
    double* sum_part = w.sum_part.as<double>(KK::tsne_sum_parts(rows) + 1);
    KK::umap_row_sums<T>(d_indices, d_dist, rows, (int)K, rowsum, s);
    KK::tsne_sum(rowsum, rows, sum_part, scal + kScalTotal, s);
    KK::umap_smooth<T>(d_indices, d_dist, rows, (int)K, (int)n_neighbors, scal + kScalTotal, p, d_sigma, d_rho, s);
  });
  // the two directions of a pair combined by the fill, into whichever index array the rows are not read from (sorted: the raw
  // arrays have been gathered from)
  int32_t* o_idx = r.sorted || m == 0 ? g.raw_idx.ptr<int32_t>() : g.sort_idx.ptr<int32_t>();
  T* out_val = g.out_val.as<T>(std::max<size_t>((size_t)r.raw.nnz, 1));
  if (m) {
    KK::umap_union_fill<T>(r.raw.ptr, r.idx, r.val, rows, r.ptr, o_idx, out_val, s);
    SAPCA_HIP(hipStreamSynchronize(s));   // complete when the call returns
  }
  *nnz_out = r.nnz;
  *d_ptr = r.ptr;
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
  check_panel(d, ldx, "ldx", who);   // (knn<T> checks them again, after)
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
  check_panel(d, d, "ldx", who);
  check_init_panel(opts, d, who);
  if (m == 0) return;
  SAPCA_CHECK(x != nullptr && y != nullptr, SAPCA_ERR_ARG, who + ": a NULL array with m = " + num(m));
  host_route<T>(h, h.umap.x, x, (size_t)m * d, h.umap.y, y, (size_t)m * opts->output_dim, opts->init == SAPCA_UMAP_INIT_GIVEN,
                [&](const T* dx, T* dy) { umap_device<T>(h, m, dx, d, d, opts, dy); });
  SAPCA_HIP(hipStreamSynchronize(h.stream));
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
