// Host staging of sapca_harmony_* (the kernels are harmony.hip's, the initial k-means kmeans.cpp's, the objective's sums
// tsne.hip's): argument checks, buffer layouts, launches, the two convergence tests.  Every scalar and shape is refused before
// anything is enqueued; a batch label out of range is refused by the counting pass, before the algorithm starts.  All work
// space lives in h.harmony (and, for init = KMEANS, h.kmeans): a fitted model, a cached preparation, the upload's statistics,
// the selection and the other consumers' buffers are not touched.
#include "resident.h"

namespace sapca {
namespace resident {

namespace {

namespace KK = sapca::k;

void check_real(double v, const char* name, bool positive, const std::string& w) {
  SAPCA_CHECK(std::isfinite(v), SAPCA_ERR_ARG, w + ": " + name + " = " + numd(v) + " is not finite");
  if (positive) SAPCA_CHECK(v > 0.0, SAPCA_ERR_ARG, w + ": " + name + " = " + numd(v) + " must be positive");
  else SAPCA_CHECK(v >= 0.0, SAPCA_ERR_ARG, w + ": " + name + " = " + numd(v) + " must not be negative");
}

void check_clusters(uint64_t K, uint64_t m, bool at_most_rows, const std::string& w) {
  SAPCA_CHECK(K != 0, SAPCA_ERR_ARG, w + ": n_clusters is 0");
  SAPCA_CHECK(K <= SAPCA_KMEANS_MAX_CLUSTERS, SAPCA_ERR_ARG,
              w + ": n_clusters = " + num(K) + " exceeds SAPCA_KMEANS_MAX_CLUSTERS = " + num(SAPCA_KMEANS_MAX_CLUSTERS));
  SAPCA_CHECK(!at_most_rows || m == 0 || K <= m, SAPCA_ERR_ARG, w + ": n_clusters = " + num(K) + " exceeds the m = " + num(m) + " rows");
}

void check_batches(uint64_t B, const std::string& w) {
  SAPCA_CHECK(B != 0, SAPCA_ERR_ARG, w + ": n_batches is 0");
  SAPCA_CHECK(B <= SAPCA_HARMONY_MAX_BATCHES, SAPCA_ERR_ARG,
              w + ": n_batches = " + num(B) + " exceeds SAPCA_HARMONY_MAX_BATCHES = " + num(SAPCA_HARMONY_MAX_BATCHES));
}

void check_run(const HarmonyParams& p, uint64_t m, uint64_t d, uint64_t ldz, uint64_t ldc, const std::string& w) {
  check_clusters(p.K, m, true, w);
  check_batches(p.B, w);
  SAPCA_CHECK(p.n_blocks != 0, SAPCA_ERR_ARG, w + ": n_blocks is 0");
  check_real(p.sigma, "sigma", true, w);
  check_real(p.lambda, "lambda", true, w);
  check_real(p.theta, "theta", false, w);
  check_real(p.epsilon_cluster, "epsilon_cluster", false, w);
  check_real(p.epsilon_harmony, "epsilon_harmony", false, w);
  SAPCA_CHECK(p.init == SAPCA_HARMONY_KMEANS || p.init == SAPCA_HARMONY_GIVEN, SAPCA_ERR_ARG,
              w + ": unknown init " + num(p.init) + " (0 KMEANS, 1 GIVEN)");
  SAPCA_CHECK(p.max_iter_harmony != 0, SAPCA_ERR_ARG, w + ": max_iter_harmony is 0");
  SAPCA_CHECK(p.max_iter_cluster != 0, SAPCA_ERR_ARG, w + ": max_iter_cluster is 0");
  check_panel(d, ldz, "ldz", w);
  check_stride_covers(d, ldc, "ldc", w);
  check_stride_limit(ldc, w);
  check_rows(m, w);
}

// The buffers of a call and what the counting pass found.  The host vectors are uploaded from: they live as long as the call,
// and every entry point synchronises before it returns.
template <typename T>
struct Work {
  H& h;
  H::Harmony& w;
  hipStream_t s;
  int64_t m;
  int d, K, B;
  double *O, *rs, *Pr, *pen, *partial, *rowd, *sum_part, *scal;
  int64_t* seg;
  uint32_t* by_batch;
  std::vector<double> pr_host;
  std::vector<int64_t> seg_host;
  Work(H& h_, uint64_t m_, uint64_t d_, uint64_t K_, uint64_t B_)
      : h(h_), w(h_.harmony), s(h_.stream), m((int64_t)m_), d((int)d_), K((int)K_), B((int)B_) {
    O = w.o.as<double>((size_t)B * K);
    rs = w.rs.as<double>(K_);
    Pr = w.pr.as<double>(B_);
    pen = w.pen.as<double>((size_t)B * K);
    seg = w.seg.as<int64_t>(B_ + 1);
    by_batch = w.by_batch.as<uint32_t>(std::max<size_t>(m_, 1));
    rowd = w.rowd.as<double>(3 * std::max<size_t>(m_, 1));
    sum_part = w.sum_part.as<double>(KK::tsne_sum_parts(m) + 1);
    scal = w.scal.as<double>(4);
    partial = nullptr;
  }

  // N_b, the refusal of a label out of range (one read-back), Pr and the batches' offsets on the device, the (batch, row) order
  void batches(const int32_t* d_batch, const std::string& who) {
    unsigned long long* cnt = w.cnt.as<unsigned long long>((size_t)B + 1);
    KK::harmony_count(d_batch, m, B, cnt, s);
    std::vector<unsigned long long> c((size_t)B + 1);
    fetch(c, cnt, s);
    SAPCA_HIP(hipStreamSynchronize(s));
    SAPCA_CHECK(c[B] >= (unsigned long long)m, SAPCA_ERR_ARG,
                who + ": the batch label of row " + num(c[B]) + " lies outside [0, n_batches = " + num((uint64_t)B) + ")");
    pr_host.resize(B);
    seg_host.assign((size_t)B + 1, 0);
    for (int b = 0; b < B; ++b) {
      pr_host[b] = (double)c[b] / (double)m;
      seg_host[b + 1] = seg_host[b] + (int64_t)c[b];
    }
    SAPCA_HIP(hipMemcpyAsync(Pr, pr_host.data(), (size_t)B * sizeof(double), hipMemcpyHostToDevice, s));
    SAPCA_HIP(hipMemcpyAsync(seg, seg_host.data(), ((size_t)B + 1) * sizeof(int64_t), hipMemcpyHostToDevice, s));
    KK::harmony_sort_batches(d_batch, m, B, w.key32.as<uint32_t>(m), w.key32_out.as<uint32_t>(m), w.val32.as<uint32_t>(m), by_batch,
                             w.sort_tmp, s);
  }
  int batch_slices() const { return KK::harmony_slices(m / B); }

  // O, rs = the sums of R as it stands
  void totals(const T* R) {
    const int sl = batch_slices();
    KK::harmony_totals<T>(R, m, K, by_batch, seg, B, sl, w.colsum.as<double>((size_t)B * sl * K), O, rs, s);
  }

  void centroids(const T* zc, int64_t ldz, const T* R, T* Y) {
    const int sl = KK::harmony_slices(m);
    double* part = w.partial.as<double>((size_t)K * sl * d);
    KK::harmony_sums<T>(zc, ldz, m, d, false, R, K, nullptr, nullptr, 1, sl, part, s);
    KK::harmony_centroids<T>(part, K, d, sl, Y, s);
  }

  // item 2 behind its centroids: the order of pass `pass`, then fold | block per block and the closing fold
  void pass(const T* zc, int64_t ldz, const int32_t* d_batch, const T* Y, T* R, T* dist, double theta, double sigma, uint32_t n_blocks,
            uint32_t seed, uint64_t pass) {
    const int64_t nb = (int64_t)n_blocks;
    uint64_t* keys = w.keys.as<uint64_t>(m);
    uint32_t* list = w.list.as<uint32_t>(m);
    KK::harmony_order(d_batch, m, B, nb, seed, pass, w.hkey.as<uint64_t>(m), w.hkey_out.as<uint64_t>(m), w.iota.as<uint32_t>(m),
                      w.perm.as<uint32_t>(m), w.key2.as<uint64_t>(m), keys, list, w.sort_tmp, s);
    const int64_t filled = std::min<int64_t>(nb, m);   // (with more blocks than rows the first m hold one row each, the rest none)
    for (int64_t j = 0; j < filled; ++j) {
      KK::harmony_fold<T>(R, m, K, B, nb, j - 1, j, keys, list, Pr, theta, O, rs, pen, s);
      const int64_t p0 = KK::harmony_block_begin(j, m, nb), p1 = KK::harmony_block_begin(j + 1, m, nb);
      KK::harmony_block<T>(zc, ldz, m, d, Y, K, d_batch, B, list, p0, p1 - p0, pen, sigma, R, dist, s);
    }
    KK::harmony_fold<T>(R, m, K, B, nb, filled - 1, -1, keys, list, Pr, theta, O, rs, pen, s);
  }

  // scal[0 .. 2] = the three terms
  void objective(const T* R, const T* dist, const int32_t* d_batch, double sigma, double theta) {
    KK::harmony_objective<T>(R, dist, d_batch, m, K, B, O, rs, Pr, sigma, theta, rowd, s);
    for (int c = 0; c < 3; ++c) KK::tsne_sum(rowd + (int64_t)c * m, m, sum_part, scal + c, s);
  }

  // item 5: out = z - sum_k R_ik beta[k][batch_i]
  double* correct(const T* z, int64_t ldz, const int32_t* d_batch, const T* R, double lambda, T* out, int64_t ldc) {
    const int sl = batch_slices();
    double* part = w.partial.as<double>((size_t)K * B * sl * (d + 1));
    double* beta = w.beta.as<double>((size_t)K * B * d);
    KK::harmony_sums<T>(z, ldz, m, d, true, R, K, by_batch, seg, B, sl, part, s);
    KK::harmony_beta(part, K, B, d, sl, lambda, beta, s);
    KK::harmony_apply<T>(z, ldz, m, d, R, K, d_batch, B, beta, out, ldc, s);
    return beta;
  }
};

}  // namespace

template <typename T>
void harmony_assign(H& h, uint64_t m, const T* d_zc, uint64_t ldz, uint64_t d, const int32_t* d_batch, uint32_t B, uint32_t K, T* d_y,
                    int32_t recompute, T* d_r, double theta, double sigma, uint32_t n_blocks, uint32_t seed, uint64_t pass, double* o,
                    double* rs, double* objective) {
  const std::string who = "harmony_assign";
  check_clusters(K, m, false, who);
  check_batches(B, who);
  SAPCA_CHECK(n_blocks != 0, SAPCA_ERR_ARG, who + ": n_blocks is 0");
  check_real(sigma, "sigma", true, who);
  check_real(theta, "theta", false, who);
  check_panel(d, ldz, "ldz", who);
  check_rows(m, who);
  if (m == 0) {
    if (objective) objective[0] = objective[1] = objective[2] = 0.0;
    return;
  }
  SAPCA_CHECK(d_zc != nullptr && d_batch != nullptr && d_y != nullptr && d_r != nullptr, SAPCA_ERR_ARG,
              who + ": a NULL array with m = " + num(m));
  Work<T> a(h, m, d, K, B);
  a.batches(d_batch, who);
  a.totals(d_r);
  if (recompute) a.centroids(d_zc, (int64_t)ldz, d_r, d_y);
  T* dist = a.w.dist.template as<T>((size_t)m * K);
  a.pass(d_zc, (int64_t)ldz, d_batch, d_y, d_r, dist, theta, sigma, n_blocks, seed, pass);
  if (objective) a.objective(d_r, dist, d_batch, sigma, theta);
  std::vector<double> ho(o ? (size_t)B * K : 0), hrs(rs ? K : 0), hobj(objective ? 3 : 0);
  fetch(ho, a.O, a.s);
  fetch(hrs, a.rs, a.s);
  fetch(hobj, a.scal, a.s);
  SAPCA_HIP(hipStreamSynchronize(a.s));
  if (o) std::copy(ho.begin(), ho.end(), o);
  if (rs) std::copy(hrs.begin(), hrs.end(), rs);
  if (objective) std::copy(hobj.begin(), hobj.end(), objective);
}

template <typename T>
void harmony_centroids(H& h, uint64_t m, const T* d_zc, uint64_t ldz, uint64_t d, uint32_t K, const T* d_r, T* d_y) {
  const std::string who = "harmony_centroids";
  check_clusters(K, m, false, who);
  check_panel(d, ldz, "ldz", who);
  check_rows(m, who);
  if (m == 0) return;
  SAPCA_CHECK(d_zc != nullptr && d_r != nullptr && d_y != nullptr, SAPCA_ERR_ARG, who + ": a NULL array with m = " + num(m));
  Work<T> a(h, m, d, K, 1);
  a.centroids(d_zc, (int64_t)ldz, d_r, d_y);
  SAPCA_HIP(hipStreamSynchronize(a.s));
}

template <typename T>
void harmony_correct(H& h, uint64_t m, const T* d_z, uint64_t ldz, uint64_t d, const int32_t* d_batch, uint32_t B, uint32_t K, const T* d_r,
                     double lambda, T* d_zcorr, uint64_t ldc, double* beta) {
  const std::string who = "harmony_correct";
  check_clusters(K, m, false, who);
  check_batches(B, who);
  check_real(lambda, "lambda", true, who);
  check_panel(d, ldz, "ldz", who);
  check_stride_covers(d, ldc, "ldc", who);
  check_stride_limit(ldc, who);
  check_rows(m, who);
  if (m == 0) return;
  SAPCA_CHECK(d_z != nullptr && d_batch != nullptr && d_r != nullptr && d_zcorr != nullptr, SAPCA_ERR_ARG,
              who + ": a NULL array with m = " + num(m));
  Work<T> a(h, m, d, K, B);
  a.batches(d_batch, who);
  const double* d_beta = a.correct(d_z, (int64_t)ldz, d_batch, d_r, lambda, d_zcorr, (int64_t)ldc);
  if (beta) SAPCA_HIP(hipMemcpyAsync(beta, d_beta, (size_t)K * B * d * sizeof(double), hipMemcpyDeviceToHost, a.s));
  SAPCA_HIP(hipStreamSynchronize(a.s));
}

template <typename T>
void harmony_device(H& h, uint64_t m, const T* d_z, uint64_t ldz, uint64_t d, const int32_t* d_batch, const HarmonyParams& p, T* d_zcorr,
                    uint64_t ldc, T* d_r, T* d_y, double* objectives, uint32_t* passes, uint32_t* n_iter, int32_t* converged) {
  const std::string who = "harmony";
  check_run(p, m, d, ldz, ldc, who);
  if (n_iter) *n_iter = 0;
  if (converged) *converged = 0;
  if (m == 0) return;
  SAPCA_CHECK(d_z != nullptr && d_batch != nullptr && d_zcorr != nullptr && d_y != nullptr, SAPCA_ERR_ARG,
              who + ": a NULL array with m = " + num(m));
  Work<T> a(h, m, d, p.K, p.B);
  hipStream_t s = a.s;
  const int64_t ld = (int64_t)d;
  a.batches(d_batch, who);
  T* zc = a.w.zc.template as<T>((size_t)m * d);
  T* R = d_r ? d_r : a.w.r.template as<T>((size_t)m * p.K);
  T* dist = a.w.dist.template as<T>((size_t)m * p.K);
  KK::harmony_unit_rows<T>(d_z, (int64_t)ldz, a.m, a.d, zc, ld, s);
  if (p.init == SAPCA_HARMONY_KMEANS) {
    sapca_kmeans_options o;
    sapca_kmeans_options_default(&o);
    o.n_clusters = p.K;
    o.random_seed = p.seed;
    o.max_iter = 25;
    o.tol = 1e-4;
    o.init = SAPCA_KMEANS_PLUSPLUS;
    kmeans_device<T>(h, m, zc, d, d, &o, d_y, a.w.labels.template as<int32_t>(m), nullptr, nullptr);
  }
  KK::harmony_unit_rows<T>(d_y, ld, a.K, a.d, d_y, ld, s);
  KK::harmony_block<T>(zc, ld, a.m, a.d, d_y, a.K, nullptr, a.B, nullptr, 0, a.m, nullptr, p.sigma, R, nullptr, s);
  a.totals(R);

  std::vector<double> outer;
  uint64_t pass = 0;
  bool done = false;
  uint32_t it = 0;
  while (it < p.max_iter_harmony && !done) {
    std::vector<double> obj;
    uint32_t i = 0;
    for (; i < p.max_iter_cluster; ++i) {
      a.centroids(zc, ld, R, d_y);
      a.pass(zc, ld, d_batch, d_y, R, dist, p.theta, p.sigma, p.n_blocks, p.seed, pass++);
      a.objective(R, dist, d_batch, p.sigma, p.theta);
      double terms[3] = {};
      SAPCA_HIP(hipMemcpyAsync(terms, a.scal, sizeof(terms), hipMemcpyDeviceToHost, s));
      SAPCA_HIP(hipStreamSynchronize(s));
      obj.push_back(terms[0] + terms[1] + terms[2]);
      if (i > 3) {
        const double fresh = obj[i - 2] + obj[i - 1] + obj[i], old = obj[i - 3] + obj[i - 2] + obj[i - 1];
        if ((old - fresh) / std::fabs(old) < p.epsilon_cluster) {
          ++i;
          break;
        }
      }
    }
    outer.push_back(obj.back());
    if (objectives) objectives[it] = obj.back();
    if (passes) passes[it] = i;
    a.correct(d_z, (int64_t)ldz, d_batch, R, p.lambda, d_zcorr, (int64_t)ldc);
    KK::harmony_unit_rows<T>(d_zcorr, (int64_t)ldc, a.m, a.d, zc, ld, s);
    ++it;
    if (it >= 2 && (outer[it - 2] - outer[it - 1]) / std::fabs(outer[it - 2]) < p.epsilon_harmony) done = true;
  }
  SAPCA_HIP(hipStreamSynchronize(s));
  if (n_iter) *n_iter = it;
  if (converged) *converged = done ? 1 : 0;
}

template <typename T>
void harmony_host(H& h, uint64_t m, uint64_t d, const T* z, const int32_t* batch, const HarmonyParams& p, T* zcorr, T* r, T* y,
                  double* objectives, uint32_t* passes, uint32_t* n_iter, int32_t* converged) {
  const std::string who = "harmony";
  check_run(p, m, d, d, d, who);
  if (n_iter) *n_iter = 0;
  if (converged) *converged = 0;
  if (m == 0) return;
  SAPCA_CHECK(z != nullptr && batch != nullptr && zcorr != nullptr && y != nullptr, SAPCA_ERR_ARG, who + ": a NULL array with m = " + num(m));
  H::Harmony& w = h.harmony;
  hipStream_t s = h.stream;
  T* dx = w.x.as<T>((size_t)m * d);
  T* dc = w.zcorr.as<T>((size_t)m * d);
  T* dy = w.y.as<T>((size_t)p.K * d);
  T* dr = r ? w.rhost.as<T>((size_t)m * p.K) : nullptr;
  int32_t* db = w.batch.as<int32_t>(m);
  SAPCA_HIP(hipMemcpyAsync(dx, z, (size_t)m * d * sizeof(T), hipMemcpyHostToDevice, s));
  SAPCA_HIP(hipMemcpyAsync(db, batch, (size_t)m * sizeof(int32_t), hipMemcpyHostToDevice, s));
  if (p.init == SAPCA_HARMONY_GIVEN) SAPCA_HIP(hipMemcpyAsync(dy, y, (size_t)p.K * d * sizeof(T), hipMemcpyHostToDevice, s));
  harmony_device<T>(h, m, dx, d, d, db, p, dc, d, dr, dy, objectives, passes, n_iter, converged);
  SAPCA_HIP(hipMemcpyAsync(zcorr, dc, (size_t)m * d * sizeof(T), hipMemcpyDeviceToHost, s));
  SAPCA_HIP(hipMemcpyAsync(y, dy, (size_t)p.K * d * sizeof(T), hipMemcpyDeviceToHost, s));
  if (r) SAPCA_HIP(hipMemcpyAsync(r, dr, (size_t)m * p.K * sizeof(T), hipMemcpyDeviceToHost, s));
  SAPCA_HIP(hipStreamSynchronize(s));
}

#define SAPCA_INSTANTIATE_HARMONY(T)                                                                                                    \
  template void harmony_assign<T>(H&, uint64_t, const T*, uint64_t, uint64_t, const int32_t*, uint32_t, uint32_t, T*, int32_t, T*,      \
                                  double, double, uint32_t, uint32_t, uint64_t, double*, double*, double*);                             \
  template void harmony_centroids<T>(H&, uint64_t, const T*, uint64_t, uint64_t, uint32_t, const T*, T*);                               \
  template void harmony_correct<T>(H&, uint64_t, const T*, uint64_t, uint64_t, const int32_t*, uint32_t, uint32_t, const T*, double,    \
                                   T*, uint64_t, double*);                                                                              \
  template void harmony_device<T>(H&, uint64_t, const T*, uint64_t, uint64_t, const int32_t*, const HarmonyParams&, T*, uint64_t, T*,   \
                                  T*, double*, uint32_t*, uint32_t*, int32_t*);                                                         \
  template void harmony_host<T>(H&, uint64_t, uint64_t, const T*, const int32_t*, const HarmonyParams&, T*, T*, T*, double*, uint32_t*, \
                                uint32_t*, int32_t*);
SAPCA_INSTANTIATE_HARMONY(float)
SAPCA_INSTANTIATE_HARMONY(double)
#undef SAPCA_INSTANTIATE_HARMONY

}  // namespace resident
}  // namespace sapca
