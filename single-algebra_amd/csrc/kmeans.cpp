// Host staging of sapca_kmeans_* (the kernels are kmeans.hip's, the norms knn.hip's prepare, the inertia's sum tsne.hip's):
// argument checks, buffer layouts, launches.  Everything that can be refused is refused before anything is enqueued or a
// buffer is touched.  All work space lives in h.kmeans: a fitted model, a cached preparation, the upload's statistics, the
// selection, the canonical and the t-SNE buffers are not touched.
#include "resident.h"

namespace sapca {
namespace resident {

namespace {

namespace KK = sapca::k;

// n_clusters (at_most_rows: seeding and the whole run pick n_clusters distinct rows)
void check_clusters(uint64_t k, uint64_t m, bool at_most_rows, const std::string& w) {
  SAPCA_CHECK(k != 0, SAPCA_ERR_ARG, w + ": n_clusters is 0");
  SAPCA_CHECK(k <= SAPCA_KMEANS_MAX_CLUSTERS, SAPCA_ERR_ARG,
              w + ": n_clusters = " + num(k) + " exceeds SAPCA_KMEANS_MAX_CLUSTERS = " + num(SAPCA_KMEANS_MAX_CLUSTERS));
  SAPCA_CHECK(!at_most_rows || m == 0 || k <= m, SAPCA_ERR_ARG, w + ": n_clusters = " + num(k) + " exceeds the m = " + num(m) + " rows");
}

void check_stage(uint64_t m, uint64_t d, uint64_t ldx, uint64_t k, bool at_most_rows, const char* who) {
  check_clusters(k, m, at_most_rows, who);
  check_panel(d, ldx, "ldx", who);
  check_rows(m, who);
}

// a whole run: the options, then the shape, in the order the header lists them
void check_run(const sapca_kmeans_options* o, uint64_t m, uint64_t d, uint64_t ldx, const char* who) {
  const std::string w(who);
  check_options_header(o, "sapca_kmeans_options", w);
  check_clusters(o->n_clusters, m, true, w);
  SAPCA_CHECK(o->init == SAPCA_KMEANS_PLUSPLUS || o->init == SAPCA_KMEANS_GIVEN, SAPCA_ERR_ARG,
              w + ": unknown init " + num(o->init) + " (0 PLUSPLUS, 1 GIVEN)");
  check_constant(o->tol, "tol", w);
  check_panel(d, ldx, "ldx", w);
  check_rows(m, w);
}

// the scalars of a call in h.kmeans.scal (f64): the inertia | tol_abs
constexpr int kScalInertia = 0, kScalTol = 1, kScalCount = 2;

template <typename T>
struct Work {
  H::Kmeans& w;
  int64_t m;
  int d, k;
  KK::KmeansPlan plan;
  T *bias, *xb;
  int32_t* amb;
  int64_t *cnt, *tab;
  int32_t* order;
  double *partial, *shiftpart, *scal;
  unsigned long long* ctl;
  Work(H& h, uint64_t m_, uint64_t d_, uint64_t k_) : w(h.kmeans), m((int64_t)m_), d((int)d_), k((int)k_), plan(KK::kmeans_plan(m, k)) {
    const size_t rows = std::max<size_t>(m_, 1);
    bias = w.bias.as<T>(k_);
    xb = w.xb.as<T>(rows);
    amb = w.amb.as<int32_t>(rows);
    cnt = w.cnt.as<int64_t>((size_t)k * plan.nwaves + 1);
    tab = w.tab.as<int64_t>((size_t)k * plan.nwaves + 1);
    order = w.order.as<int32_t>(rows);
    partial = w.partial.as<double>((size_t)k * plan.slices * d);
    shiftpart = w.shiftpart.as<double>(k_);
    scal = w.scal.as<double>(kScalCount);
    ctl = w.ctl.as<unsigned long long>(KK::kKmCtlWords);
  }
};

// labels = assign(cen), nothing read back; xb holds -|x_i|^2 already and ctl[kKmAmbiguous] is 0.  (The centroids' norms come
// from knn.hip's prepare, which knows no skip flag: behind convergence it recomputes the same norms of unchanged centroids.)
template <typename T>
void enqueue_assign(Work<T>& a, const unsigned long long* skip, const T* x, int64_t ldx, const T* cen, int32_t* labels, hipStream_t s) {
  KK::knn_prepare<T>(cen, a.d, a.k, a.d, SAPCA_KNN_EUCLIDEAN, nullptr, a.bias, s);
  KK::kmeans_rank<T>(skip, x, ldx, a.m, cen, a.k, a.bias, a.xb, a.d, labels, a.amb, a.ctl, s);
  KK::kmeans_refine<T>(skip, x, ldx, a.m, cen, a.k, a.d, labels, a.amb, a.ctl, s);
}

// cen = update(labels), shiftpart = the squared shifts per cluster; prev non-null: ctl[kKmChanged] += the labels that differ from it
template <typename T>
void enqueue_update(Work<T>& a, const unsigned long long* skip, const T* x, int64_t ldx, const int32_t* labels, const int32_t* prev, T* cen,
                    int64_t* counts, hipStream_t s) {
  KK::kmeans_sort(skip, labels, a.m, a.k, a.plan, a.cnt, a.tab, a.order, a.w.scan, prev, a.ctl, s);
  KK::kmeans_sums<T>(skip, x, ldx, a.m, a.d, a.order, a.tab, a.plan.nwaves, a.k, a.plan.slices, nullptr, a.partial, s);
  KK::kmeans_finalize<T>(skip, a.partial, a.tab, a.plan.nwaves, a.k, a.d, a.plan.slices, cen, counts, a.shiftpart, s);
}

// scal[kScalInertia] = sum_i |x_i - cen[labels_i]|^2, dist2 (nullable) the rounded terms
template <typename T>
void enqueue_inertia(Work<T>& a, const T* x, int64_t ldx, const T* cen, const int32_t* labels, T* dist2, hipStream_t s) {
  double* rowd = a.w.rowd.template as<double>((size_t)a.m);
  double* sum_part = a.w.sum_part.template as<double>(KK::tsne_sum_parts(a.m) + 1);
  KK::kmeans_distances<T>(x, ldx, a.m, cen, a.k, a.d, labels, dist2, rowd, s);
  KK::tsne_sum(rowd, a.m, sum_part, a.scal + kScalInertia, s);
}

template <typename T>
void enqueue_seed(H& h, uint64_t m, const T* x, uint64_t ldx, uint64_t d, uint64_t k, uint32_t seed, T* cen, int32_t* rows) {
  H::Kmeans& w = h.kmeans;
  if (rows == nullptr) rows = w.rows.as<int32_t>(k);
  double* dist = w.seed_dist.as<double>(m);
  double* bsum = w.seed_bsum.as<double>((m + 1023) / 1024);
  KK::kmeans_seed<T>(x, (int64_t)ldx, (int64_t)m, (int)d, (int)k, seed, cen, rows, dist, bsum, h.stream);
}

}  // namespace

template <typename T>
void kmeans_seed(H& h, uint64_t m, const T* d_x, uint64_t ldx, uint64_t d, uint32_t k, uint32_t seed, T* d_centroids, int32_t* d_rows) {
  const char* who = "kmeans_seed";
  check_stage(m, d, ldx, k, true, who);
  if (m == 0) return;
  SAPCA_CHECK(d_x != nullptr && d_centroids != nullptr, SAPCA_ERR_ARG, std::string(who) + ": a NULL array with m = " + num(m));
  enqueue_seed<T>(h, m, d_x, ldx, d, k, seed, d_centroids, d_rows);
  SAPCA_HIP(hipStreamSynchronize(h.stream));
}

template <typename T>
void kmeans_assign(H& h, uint64_t m, const T* d_x, uint64_t ldx, uint64_t d, uint32_t k, const T* d_centroids, int32_t* d_labels, T* d_dist2,
                   double* inertia, uint64_t* n_ambiguous) {
  const char* who = "kmeans_assign";
  check_stage(m, d, ldx, k, false, who);
  if (m == 0) {
    if (inertia) *inertia = 0.0;
    if (n_ambiguous) *n_ambiguous = 0;
    return;
  }
  SAPCA_CHECK(d_x != nullptr && d_centroids != nullptr && d_labels != nullptr, SAPCA_ERR_ARG,
              std::string(who) + ": a NULL array with m = " + num(m));
  hipStream_t s = h.stream;
  Work<T> a(h, m, d, k);
  SAPCA_HIP(hipMemsetAsync(a.ctl, 0, KK::kKmCtlWords * sizeof(unsigned long long), s));
  KK::knn_prepare<T>(d_x, (int64_t)ldx, a.m, a.d, SAPCA_KNN_EUCLIDEAN, nullptr, a.xb, s);
  enqueue_assign<T>(a, nullptr, d_x, (int64_t)ldx, d_centroids, d_labels, s);
  if (d_dist2 || inertia) enqueue_inertia<T>(a, d_x, (int64_t)ldx, d_centroids, d_labels, d_dist2, s);
  unsigned long long ctl[KK::kKmCtlWords] = {};
  double scal[kScalCount] = {};
  SAPCA_HIP(hipMemcpyAsync(ctl, a.ctl, sizeof(ctl), hipMemcpyDeviceToHost, s));
  if (inertia) SAPCA_HIP(hipMemcpyAsync(scal, a.scal, sizeof(scal), hipMemcpyDeviceToHost, s));
  SAPCA_HIP(hipStreamSynchronize(s));
  if (inertia) *inertia = scal[kScalInertia];
  if (n_ambiguous) *n_ambiguous = ctl[KK::kKmAmbiguous];
}

template <typename T>
void kmeans_update(H& h, uint64_t m, const T* d_x, uint64_t ldx, uint64_t d, uint32_t k, const int32_t* d_labels, T* d_centroids,
                   int64_t* d_counts) {
  const char* who = "kmeans_update";
  check_stage(m, d, ldx, k, false, who);
  if (m == 0) return;
  SAPCA_CHECK(d_x != nullptr && d_labels != nullptr && d_centroids != nullptr, SAPCA_ERR_ARG,
              std::string(who) + ": a NULL array with m = " + num(m));
  Work<T> a(h, m, d, k);
  enqueue_update<T>(a, nullptr, d_x, (int64_t)ldx, d_labels, nullptr, d_centroids, d_counts, h.stream);
  SAPCA_HIP(hipStreamSynchronize(h.stream));
}

template <typename T>
void kmeans_device(H& h, uint64_t m, const T* d_x, uint64_t ldx, uint64_t d, const sapca_kmeans_options* opts, T* d_centroids,
                   int32_t* d_labels, double* inertia, uint64_t* n_iter) {
  const char* who = "kmeans";
  check_run(opts, m, d, ldx, who);
  if (m == 0) {
    if (inertia) *inertia = 0.0;
    if (n_iter) *n_iter = 0;
    return;
  }
  SAPCA_CHECK(d_x != nullptr && d_centroids != nullptr && d_labels != nullptr, SAPCA_ERR_ARG,
              std::string(who) + ": a NULL array with m = " + num(m));
  hipStream_t s = h.stream;
  const uint64_t k = opts->n_clusters;
  const int64_t ld = (int64_t)ldx;
  Work<T> a(h, m, d, k);
  int32_t* lab[2] = {a.w.lab0.template as<int32_t>(m), a.w.lab1.template as<int32_t>(m)};
  SAPCA_HIP(hipMemsetAsync(a.ctl, 0, KK::kKmCtlWords * sizeof(unsigned long long), s));
  SAPCA_HIP(hipMemsetAsync(a.scal, 0, kScalCount * sizeof(double), s));
  if (opts->init == SAPCA_KMEANS_PLUSPLUS) enqueue_seed<T>(h, m, d_x, ldx, d, k, opts->random_seed, d_centroids, nullptr);
  KK::knn_prepare<T>(d_x, ld, a.m, a.d, SAPCA_KNN_EUCLIDEAN, nullptr, a.xb, s);
  if (opts->tol > 0.0 && opts->max_iter > 0) {   // tol_abs = tol * the mean column variance: the means, then the squared deviations
    const int slices = KK::kmeans_column_slices(a.m);
    double* part = a.w.colpart.template as<double>((size_t)slices * d);
    double* cols = a.w.cols.template as<double>(2 * d);
    KK::kmeans_sums<T>(nullptr, d_x, ld, a.m, a.d, nullptr, nullptr, 0, 1, slices, nullptr, part, s);
    KK::kmeans_fold_columns(part, slices, a.d, a.m, cols, 0.0, nullptr, s);
    KK::kmeans_sums<T>(nullptr, d_x, ld, a.m, a.d, nullptr, nullptr, 0, 1, slices, cols, part, s);
    KK::kmeans_fold_columns(part, slices, a.d, a.m, cols + d, opts->tol, a.scal + kScalTol, s);
  }
  const unsigned long long* done = a.ctl + KK::kKmDone;
  for (uint64_t i = 0; i < opts->max_iter; ++i) {
    int32_t* cur = lab[i & 1];
    enqueue_assign<T>(a, done, d_x, ld, d_centroids, cur, s);
    enqueue_update<T>(a, done, d_x, ld, cur, i ? lab[(i & 1) ^ 1] : nullptr, d_centroids, nullptr, s);
    KK::kmeans_step(a.ctl, a.shiftpart, a.k, a.scal + kScalTol, i, s);
    if ((i & 7) == 7 && i + 1 < opts->max_iter) {   // stop enqueueing behind a converged run (what is enqueued already does nothing)
      unsigned long long flag = 0;
      SAPCA_HIP(hipMemcpyAsync(&flag, done, sizeof(flag), hipMemcpyDeviceToHost, s));
      SAPCA_HIP(hipStreamSynchronize(s));
      if (flag) break;
    }
  }
  // a strict run returns the labels of its last iteration; any other the assignment to the final centroids
  KK::kmeans_take_labels(a.ctl, lab[0], lab[1], d_labels, a.m, s);
  enqueue_assign<T>(a, a.ctl + KK::kKmStrict, d_x, ld, d_centroids, d_labels, s);
  enqueue_inertia<T>(a, d_x, ld, d_centroids, d_labels, nullptr, s);
  unsigned long long ctl[KK::kKmCtlWords] = {};
  double scal[kScalCount] = {};
  SAPCA_HIP(hipMemcpyAsync(ctl, a.ctl, sizeof(ctl), hipMemcpyDeviceToHost, s));
  SAPCA_HIP(hipMemcpyAsync(scal, a.scal, sizeof(scal), hipMemcpyDeviceToHost, s));
  SAPCA_HIP(hipStreamSynchronize(s));
  if (inertia) *inertia = scal[kScalInertia];
  if (n_iter) *n_iter = ctl[KK::kKmIter];
}

template <typename T>
void kmeans_host(H& h, uint64_t m, uint64_t d, const T* x, const sapca_kmeans_options* opts, T* centroids, int32_t* labels, double* inertia,
                 uint64_t* n_iter) {
  const char* who = "kmeans";
  check_run(opts, m, d, d, who);
  if (m == 0) {
    if (inertia) *inertia = 0.0;
    if (n_iter) *n_iter = 0;
    return;
  }
  SAPCA_CHECK(x != nullptr && centroids != nullptr && labels != nullptr, SAPCA_ERR_ARG, std::string(who) + ": a NULL array with m = " + num(m));
  H::Kmeans& w = h.kmeans;
  int32_t* dl = w.labels.as<int32_t>(m);
  host_route<T>(h, w.x, x, (size_t)m * d, w.cen, centroids, (size_t)opts->n_clusters * d, opts->init == SAPCA_KMEANS_GIVEN,
                [&](const T* dx, T* dc) { kmeans_device<T>(h, m, dx, d, d, opts, dc, dl, inertia, n_iter); });
  SAPCA_HIP(hipMemcpyAsync(labels, dl, (size_t)m * sizeof(int32_t), hipMemcpyDeviceToHost, h.stream));
  SAPCA_HIP(hipStreamSynchronize(h.stream));
}

#define SAPCA_INSTANTIATE_KMEANS(T)                                                                                                 \
  template void kmeans_seed<T>(H&, uint64_t, const T*, uint64_t, uint64_t, uint32_t, uint32_t, T*, int32_t*);                       \
  template void kmeans_assign<T>(H&, uint64_t, const T*, uint64_t, uint64_t, uint32_t, const T*, int32_t*, T*, double*, uint64_t*); \
  template void kmeans_update<T>(H&, uint64_t, const T*, uint64_t, uint64_t, uint32_t, const int32_t*, T*, int64_t*);               \
  template void kmeans_device<T>(H&, uint64_t, const T*, uint64_t, uint64_t, const sapca_kmeans_options*, T*, int32_t*, double*,    \
                                 uint64_t*);                                                                                        \
  template void kmeans_host<T>(H&, uint64_t, uint64_t, const T*, const sapca_kmeans_options*, T*, int32_t*, double*, uint64_t*);
SAPCA_INSTANTIATE_KMEANS(float)
SAPCA_INSTANTIATE_KMEANS(double)
#undef SAPCA_INSTANTIATE_KMEANS

}  // namespace resident
}  // namespace sapca
