// Host staging of sapca_graph_components_device, sapca_spectral_* and sapca_umap_spectral_init_device_* (the kernels are
// spectral.hip's, the Gram-Schmidt, norm, scale and combination kernels lanczos.hip's, the scan prep.hip's, the tridiagonal QL
// small_svd.cpp's): argument checks, buffer layouts, launches, the convergence test.  Everything that can be refused is refused
// before anything is enqueued or a buffer is touched.  All work space lives in h.spectral: a fitted model, a cached preparation,
// the upload, the UMAP graph and the Louvain buffers are not touched.
#include <algorithm>
#include <cmath>

#include "lanczos_step.h"
#include "resident.h"
#include "small_svd.h"

namespace sapca {
namespace resident {

namespace {

namespace KK = sapca::k;

void check_structure(uint64_t m, uint64_t nnz, const int64_t* ptr, const int32_t* idx, const std::string& w) {
  check_rows(m, w);
  SAPCA_CHECK(m == 0 || ptr != nullptr, SAPCA_ERR_ARG, w + ": NULL row offsets with m = " + num(m));
  SAPCA_CHECK(nnz == 0 || idx != nullptr, SAPCA_ERR_ARG, w + ": a NULL column array with nnz = " + num(nnz));
}

template <typename T>
void check_graph(const CsrView<T>& G, const std::string& w) {
  check_structure((uint64_t)G.rows, (uint64_t)G.nnz, G.ptr, G.idx, w);
  SAPCA_CHECK(G.nnz == 0 || G.val != nullptr, SAPCA_ERR_ARG, w + ": a NULL value array with nnz = " + num((uint64_t)G.nnz));
}

void check_kind(uint32_t kind, const std::string& w) {
  SAPCA_CHECK(kind == SAPCA_SPECTRAL_NORMALIZED || kind == SAPCA_SPECTRAL_DIFFMAP, SAPCA_ERR_ARG, w + ": unknown kind " + num(kind));
}

void check_options(const sapca_spectral_options* o, uint64_t m, const std::string& w) {
  check_options_header(o, "sapca_spectral_options", w);
  check_kind(o->kind, w);
  SAPCA_CHECK(o->n_eigen >= 1 && o->n_eigen <= 64, SAPCA_ERR_ARG, w + ": n_eigen = " + num(o->n_eigen) + " is outside 1 .. 64");
  SAPCA_CHECK(o->max_steps <= 4096, SAPCA_ERR_ARG, w + ": max_steps = " + num(o->max_steps) + " exceeds 4096");
  SAPCA_CHECK(o->single_round <= 1, SAPCA_ERR_ARG, w + ": single_round = " + num(o->single_round) + " is neither 0 nor 1");
  check_constant(o->tol, "tol", w);
  check_rows(m, w);
  SAPCA_CHECK(m == 0 || o->n_eigen <= m, SAPCA_ERR_ARG, w + ": n_eigen = " + num(o->n_eigen) + " exceeds m = " + num(m));
}

// the lanes of a row's group: from the mean row length, or the debug variant's SAPCA_SPECTRAL_GROUP (8 | 16 | 32 | 64)
int group_of(int64_t m, int64_t nnz) {
  const char* e = dbg_env("SAPCA_SPECTRAL_GROUP");
  return KK::spectral_group(m, nnz, e ? atoi(e) : 0);
}

// y = S x.  The stage call runs the short-row product (debug variant, SAPCA_SPECTRAL_SPMV_ROW: k::spmv, the timing tool's
// yardstick).  The step of the solve runs k::spmv: measured on the 200 000-row neighbour graph the short-row kernel is 1.18
// times slower (profiles/spectral_time.txt), so the faster route is the one kept (debug variant, SAPCA_SPECTRAL_STEP_SHORT: the
// short-row product in the step, for the same tool).
void stage_product(const CsrView<double>& S, const double* x, double* y, int g, hipStream_t s) {
  if (dbg_on("SAPCA_SPECTRAL_SPMV_ROW")) KK::spmv<double>(S, x, y, s);
  else KK::spectral_spmv(S, x, y, g, s);
}
void step_product(const CsrView<double>& S, const double* x, double* y, int g, hipStream_t s) {
  if (dbg_on("SAPCA_SPECTRAL_STEP_SHORT")) KK::spectral_spmv(S, x, y, g, s);
  else KK::spmv<double>(S, x, y, s);
}

// stage 1 into `labels` (device); returns the number of components
uint64_t enqueue_components(H& h, int64_t m, const int64_t* ptr, const int32_t* idx, int32_t* labels) {
  H::Spectral& w = h.spectral;
  hipStream_t s = h.stream;
  int32_t* parent = w.parent.as<int32_t>((size_t)m);
  unsigned long long* changed = w.changed.as<unsigned long long>(1);
  KK::components_init(parent, m, changed, s);
  for (int64_t round = 0; round <= m; ++round) {   // (a round that changes something lowers a parent: at most m of them)
    KK::components_round(ptr, idx, m, parent, changed, s);
    unsigned long long flag = 0;
    SAPCA_HIP(hipMemcpyAsync(&flag, changed, sizeof(flag), hipMemcpyDeviceToHost, s));
    SAPCA_HIP(hipStreamSynchronize(s));
    if (!flag) break;
    SAPCA_HIP(hipMemsetAsync(changed, 0, sizeof(flag), s));
  }
  int64_t* scan = w.flag.as<int64_t>((size_t)m + 1);
  KK::components_flag(parent, m, scan, s);
  KK::exclusive_scan_i64(scan, m + 1, w.scan, 0, s);
  KK::components_label(parent, m, scan, labels, s);
  int64_t n = 0;
  SAPCA_HIP(hipMemcpyAsync(&n, scan + m, sizeof(int64_t), hipMemcpyDeviceToHost, s));
  SAPCA_HIP(hipStreamSynchronize(s));
  return (uint64_t)n;
}

// stage 2 into sc (device, m f64); work space: the first 2 m doubles of w.scale
template <typename T>
void enqueue_scale(H& h, const CsrView<T>& G, uint32_t kind, int g, double* sc) {
  hipStream_t s = h.stream;
  double* q = h.spectral.scale.as<double>(2 * (size_t)G.rows);
  double* t = q + G.rows;
  KK::spectral_row_sums<T>(G, nullptr, g, q, s);
  if (kind == SAPCA_SPECTRAL_NORMALIZED) {
    KK::spectral_scale_finish(q, nullptr, G.rows, sc, s);
  } else {
    KK::spectral_row_sums<T>(G, q, g, t, s);
    KK::spectral_scale_finish(t, q, G.rows, sc, s);
  }
}

// stage 3's matrix: the scaled f64 copy of G's values on G's structure.  safe_columns (the solve: its step's k::spmv gathers
// x[column] without looking at the column): on a copy of the columns in which one outside [0, m) names the row itself, value 0.
template <typename T>
CsrView<double> enqueue_scaled_copy(H& h, const CsrView<T>& G, const double* sc, bool safe_columns) {
  double* wt = h.spectral.wt.as<double>((size_t)std::max<int64_t>(G.nnz, 1));
  int32_t* cols = safe_columns ? h.spectral.safe_idx.as<int32_t>((size_t)std::max<int64_t>(G.nnz, 1)) : nullptr;
  KK::spectral_scaled_copy<T>(G, sc, wt, cols, h.stream);
  CsrView<double> S;
  S.rows = S.cols = G.rows; S.nnz = G.nnz; S.ptr = G.ptr; S.idx = cols ? cols : G.idx; S.val = wt;
  return S;
}

// The locked pairs (include/sapca.h, stage 4) from one read-back of s (and q for DIFFMAP) and the labels: t_i = 1 / s_i or
// 1 / (s_i q_i), lock_of[label] = the pair's number or -1, inv_norm[pair] = 1 / |t 1_C|.  At most `want` pairs are numbered.
// Returns their count; the device table is t (m f64) | inv_norm (want f64) | lock_of (ncomp int32).
int locked_pairs(H& h, int64_t m, uint64_t ncomp, const int32_t* d_labels, const double* d_sc, const double* d_q, int want,
                 const double** d_t, const int32_t** d_lock_of, const double** d_inv_norm) {
  H::Spectral& w = h.spectral;
  hipStream_t s = h.stream;
  std::vector<double> sc((size_t)m), q(d_q ? (size_t)m : 0);
  std::vector<int32_t> lab((size_t)m);
  fetch(sc, d_sc, s);
  fetch(q, d_q, s);
  fetch(lab, d_labels, s);
  SAPCA_HIP(hipStreamSynchronize(s));
  const size_t bytes = ((size_t)m + (size_t)want) * sizeof(double) + (size_t)ncomp * sizeof(int32_t);
  char* host = (char*)w.host.ensure(bytes);
  double* t = (double*)host;
  double* inv_norm = t + m;
  int32_t* lock_of = (int32_t*)(inv_norm + want);
  std::vector<double> norm2((size_t)ncomp, 0.0);
  for (int64_t i = 0; i < m; ++i) {
    const double si = sc[(size_t)i];
    const double ti = si > 0.0 ? (d_q ? 1.0 / (si * q[(size_t)i]) : 1.0 / si) : 0.0;
    t[i] = ti > 0.0 && std::isfinite(ti) ? ti : 0.0;
    if (t[i] > 0.0) norm2[(size_t)lab[(size_t)i]] += t[i] * t[i];   // (ascending vertex order)
  }
  int nlock = 0;
  for (uint64_t c = 0; c < ncomp; ++c) {
    const bool take = norm2[(size_t)c] > 0.0 && std::isfinite(norm2[(size_t)c]) && nlock < want;
    lock_of[c] = take ? nlock : -1;
    if (take) inv_norm[nlock++] = 1.0 / std::sqrt(norm2[(size_t)c]);
  }
  char* dev = w.lock_tab.as<char>(bytes);
  SAPCA_HIP(hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, s));
  SAPCA_HIP(hipStreamSynchronize(s));   // (the iteration takes the same page-locked buffer for alpha | beta)
  *d_t = (const double*)dev;
  *d_inv_norm = *d_t + m;
  *d_lock_of = (const int32_t*)(*d_inv_norm + want);
  return nlock;
}

// One round of stage 5 on S in the complement of the c locked vectors that open the basis V (the analytic ones and the Ritz
// vectors of earlier rounds), for the k largest pairs of that complement.  Returns the steps taken; on return theta (ascending)
// and Z (steps x steps, columns) are the eigenpairs of the final tridiagonal.  exhausted: the Krylov space of the start vector
// ended (possibly in fewer than k steps); every Ritz pair of the run is then an eigenpair, and there are `steps` of them.
// floor: a lower bound of |S| (1 when a pair of eigenvalue 1 is locked).  A beta_j is zero against the larger of it and the
// run's own Ritz values: in the null space of S those are rounding noise themselves, and a run that went on there would
// normalise noise into basis vectors.
struct LanczosRun {
  int64_t steps = 0;
  bool converged = false, exhausted = false;
  std::vector<double> theta, Z;
};
LanczosRun run_lanczos(H& h, const CsrView<double>& S, int g, int c, int k, int64_t jmax, double tol, uint32_t seed, double floor,
                       double* V) {
  H::Spectral& wk = h.spectral;
  hipStream_t s = h.stream;
  const int64_t m = S.rows;
  double* w = wk.w.as<double>((size_t)m);
  // h1 | h2 | alpha | beta (c + jmax + 2 each; alpha[c + j] is step j's) | the partial sums
  const size_t L = (size_t)(c + jmax + 2);
  double* h1 = wk.small.as<double>(4 * L + KK::kLanczosPartialSlots);
  double* h2 = h1 + L;
  double* alpha = h2 + L;
  double* beta = alpha + L;
  double* partial = beta + L;
  double* ab_host = (double*)wk.host.ensure(2 * L * sizeof(double));
  double* v0 = V + (size_t)c * m;

  // the start vector, through the two Gram-Schmidt passes against the locked vectors like every later one
  KK::gaussian_panel(w, m, 1, 1, seed, s);
  for (int pass = 0; pass < 2 && c > 0; ++pass) {
    KK::lanczos_gemv_t(V, m, c, w, h1, s);
    KK::lanczos_gemv_n_sub(V, m, c, h1, w, s);
  }
  KK::lanczos_scale(w, m, partial, KK::lanczos_norm2(w, m, partial, s), beta + L - 1, v0, s);

  auto check_due = [](int64_t j) {
    const int every = j <= 64 ? 1 : j <= 128 ? 2 : j <= 256 ? 4 : 8;
    return j % every == 0;
  };
  LanczosRun run;
  for (int64_t j = 0; j < jmax; ++j) {
    const double* vj = v0 + (size_t)j * m;
    step_product(S, vj, w, g, s);
    const int nvec = (int)(c + j + 1);
    KK::lanczos_gemv_t(V, m, nvec, w, h1, s);
    KK::lanczos_gemv_n_sub(V, m, nvec, h1, w, s);
    KK::lanczos_gemv_t(V, m, nvec, w, h2, s);
    const int nparts = KK::lanczos_gemv_n_sub_norm(V, m, nvec, h1, h2, w, partial, (int)(c + j), alpha, s);
    KK::lanczos_scale(w, m, partial, nparts, beta + j, v0 + (size_t)(j + 1) * m, s);
    const int64_t steps = run.steps = j + 1;
    const bool last = steps == jmax;
    if (steps >= k && !(check_due(steps) || last)) continue;
    SAPCA_HIP(hipMemcpyAsync(ab_host, alpha + c, (size_t)steps * sizeof(double), hipMemcpyDeviceToHost, s));
    SAPCA_HIP(hipMemcpyAsync(ab_host + L, beta, (size_t)steps * sizeof(double), hipMemcpyDeviceToHost, s));
    SAPCA_HIP(hipStreamSynchronize(s));
    const double* b_host = ab_host + L;
    if (steps < k) {
      // Fewer steps than wanted pairs: only an exhausted Krylov space matters here.  Behind it the basis would be padded with
      // zero vectors and T with zero rows, whose Ritz pairs are not eigenpairs: the round ends with the `steps` pairs it has.
      double reach = floor;   // (Gershgorin: no eigenvalue of T lies further out)
      for (int64_t i = 0; i < steps; ++i) reach = std::max(reach, std::fabs(ab_host[i]) + 2.0 * std::fabs(b_host[i]));
      if (!(b_host[steps - 1] <= 1e-13 * reach)) continue;
      // Nothing locked (floor == 0): no vertex has a positive scale, S is the zero matrix -- a graph without weights -- and
      // every vector is an "eigenvector" of it: refused as ever, not answered with arbitrary vectors.
      SAPCA_CHECK(floor > 0.0, SAPCA_ERR_SVD,
                  "spectral: the Krylov space is exhausted after " + num((uint64_t)steps) + " steps, " + num((uint64_t)k) +
                      " pairs were to be iterated");
      run.converged = run.exhausted = true;
      break;
    }
    std::vector<double> d(ab_host, ab_host + steps), e((size_t)steps, 0.0), bottom;
    for (int64_t i = 1; i < steps; ++i) e[(size_t)i] = b_host[i - 1];
    SAPCA_CHECK(tridiag_eigh(d, e, (int)steps, bottom, true), SAPCA_ERR_SVD, "spectral: tridiagonal QL did not converge");
    const double bj = b_host[steps - 1];
    double radius = floor;
    for (double t : d) radius = std::max(radius, std::fabs(t));
    bool ok = std::isfinite(bj);
    for (int i = 0; i < k && ok; ++i) ok = std::fabs(bj * bottom[(size_t)(steps - 1 - i)]) <= tol;
    const bool exhausted = steps == m - c || bj <= 1e-13 * radius;
    if (ok || (exhausted && std::isfinite(bj))) {
      run.converged = true;
      run.exhausted = exhausted;
      break;
    }
  }
  if (run.converged) {   // the eigenvectors of the final T (the checks kept their bottom row only)
    const int64_t steps = run.steps;
    const double* b_host = ab_host + L;
    std::vector<double> d(ab_host, ab_host + steps), e((size_t)steps, 0.0);
    for (int64_t i = 1; i < steps; ++i) e[(size_t)i] = b_host[i - 1];
    SAPCA_CHECK(tridiag_eigh(d, e, (int)steps, run.Z), SAPCA_ERR_SVD, "spectral: tridiagonal QL did not converge");
    run.theta = d;
  }
  return run;
}

}  // namespace

void graph_components(H& h, uint64_t m, uint64_t nnz, const int64_t* ptr, const int32_t* idx, int32_t* d_labels, uint64_t* n_components) {
  const std::string who("graph_components");
  check_structure(m, nnz, ptr, idx, who);
  if (n_components) *n_components = 0;
  if (m == 0) return;
  SAPCA_CHECK(d_labels != nullptr, SAPCA_ERR_ARG, who + ": d_labels is NULL with m = " + num(m));
  const uint64_t n = enqueue_components(h, (int64_t)m, ptr, idx, d_labels);
  if (n_components) *n_components = n;
}

template <typename T>
void spectral_scale(H& h, const CsrView<T>& G, uint32_t kind, double* d_scale) {
  const std::string who("spectral_scale");
  check_kind(kind, who);
  check_graph(G, who);
  if (G.rows == 0) return;
  SAPCA_CHECK(d_scale != nullptr, SAPCA_ERR_ARG, who + ": d_scale is NULL with m = " + num((uint64_t)G.rows));
  enqueue_scale<T>(h, G, kind, group_of(G.rows, G.nnz), d_scale);
  SAPCA_HIP(hipStreamSynchronize(h.stream));   // complete when the call returns
}

template <typename T>
void spectral_apply(H& h, const CsrView<T>& G, uint32_t kind, const double* d_x, double* d_y) {
  const std::string who("spectral_apply");
  check_kind(kind, who);
  check_graph(G, who);
  if (G.rows == 0) return;
  SAPCA_CHECK(d_x != nullptr && d_y != nullptr, SAPCA_ERR_ARG, who + ": a NULL vector with m = " + num((uint64_t)G.rows));
  SAPCA_CHECK(d_x != d_y, SAPCA_ERR_ARG, who + ": d_x and d_y are the same array");
  const int g = group_of(G.rows, G.nnz);
  double* sc = h.spectral.scale.as<double>(3 * (size_t)G.rows) + 2 * G.rows;   // (q | t | s)
  enqueue_scale<T>(h, G, kind, g, sc);
  const CsrView<double> S = enqueue_scaled_copy<T>(h, G, sc, false);
  const char* reps = dbg_env("SAPCA_SPECTRAL_APPLY_REPS");   // (the timing tool: the product alone, by difference)
  for (int r = std::max(1, reps ? atoi(reps) : 1); r > 0; --r) stage_product(S, d_x, d_y, g, h.stream);
  SAPCA_HIP(hipStreamSynchronize(h.stream));
}

template <typename T>
void spectral_device(H& h, const CsrView<T>& G, const sapca_spectral_options* opts, double* evals, T* d_evecs, uint64_t* n_components,
                     uint32_t* n_steps) {
  const std::string who("spectral");
  check_options(opts, (uint64_t)G.rows, who);
  check_graph(G, who);
  if (n_components) *n_components = 0;
  if (n_steps) *n_steps = 0;
  if (G.rows == 0) return;
  SAPCA_CHECK(evals != nullptr && d_evecs != nullptr, SAPCA_ERR_ARG, who + ": a NULL output with m = " + num((uint64_t)G.rows));
  H::Spectral& w = h.spectral;
  hipStream_t s = h.stream;
  const int64_t m = G.rows;
  const int n_eigen = (int)opts->n_eigen;
  const int g = group_of(m, G.nnz);

  // stages 1 - 2, then the locked pairs
  int32_t* labels = w.labels.as<int32_t>((size_t)m);
  const uint64_t ncomp = enqueue_components(h, m, G.ptr, G.idx, labels);
  double* sc = w.scale.as<double>(3 * (size_t)m) + 2 * m;
  enqueue_scale<T>(h, G, opts->kind, g, sc);
  const int32_t* lock_of = nullptr;
  const double *inv_norm = nullptr, *t = nullptr;
  const double* q = opts->kind == SAPCA_SPECTRAL_DIFFMAP ? w.scale.ptr<double>() : nullptr;   // (enqueue_scale's layout: q | . | s)
  const int c = locked_pairs(h, m, ncomp, labels, sc, q, n_eigen, &t, &lock_of, &inv_norm);
  const int k = n_eigen - c;   // pairs the iteration owes
  const int64_t max_steps = opts->max_steps ? (int64_t)opts->max_steps : std::min<int64_t>(m, 1000);
  const int64_t jmax = k > 0 ? std::min<int64_t>(max_steps, m - c) : 0;
  // (SAPCA_ERR_NOMEM from here; the rounds lock at most 2 k Ritz vectors: k to fill, and a k-th merged copy ends the merging)
  double* V = w.basis.as<double>((size_t)(c + 2 * std::max(k, 0) + jmax + 1) * (size_t)m);
  KK::spectral_locked(labels, lock_of, inv_norm, t, m, c, V, s);
  int* signs = w.signs.as<int>(64);
  KK::spectral_store<T>(V, m, 1, m, c, false, signs, d_evecs, n_eigen, 0, s);
  for (int i = 0; i < c; ++i) evals[i] = 1.0;

  int64_t steps = 0;
  if (k > 0) {
    SAPCA_CHECK(jmax >= k, SAPCA_ERR_SVD,
                who + ": Lanczos did not converge " + num((uint64_t)k) + " of " + num((uint64_t)n_eigen) + " pairs in " + num((uint64_t)jmax) +
                    " steps");
    const CsrView<double> S = enqueue_scaled_copy<T>(h, G, sc, true);
    const bool verify = opts->single_round == 0 && c > 0;   // (c == 0: S is the zero matrix, one run says all there is to say)
    // Rounds (include/sapca.h, stage 5).  vals[i] belongs to the Ritz vector V[c + i]: the rounds lock what they accept, so the
    // next one iterates in the complement of all of it and finds the copies of a repeated value that one start vector cannot.
    std::vector<double> vals;
    std::vector<int> order;   // of vals, descending (ties in the order found)
    auto sort_vals = [&] {
      order.resize(vals.size());
      for (size_t i = 0; i < order.size(); ++i) order[i] = (int)i;
      std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return vals[(size_t)a] > vals[(size_t)b]; });
    };
    double* R = w.ritz_v.as<double>((size_t)m * k);
    for (uint32_t round = 0;; ++round) {
      const int have = (int)vals.size();
      const int lock = c + have;
      const bool checking = have >= k;   // all pairs are there: is a larger one left in the complement?
      // (merged values come in non-increasing order and each exceeds the k-th held one: the k-th merge is the last, and the
      // basis has room for 2 k held vectors)
      if (lock == m || (checking && (!verify || have >= 2 * k))) break;
      const int want = checking ? 1 : k - have;
      const int64_t jr = std::min<int64_t>(max_steps, m - lock);
      const LanczosRun run = run_lanczos(h, S, g, lock, want, jr, opts->tol, opts->random_seed + 0x9E3779B9u * round, c > 0 ? 1.0 : 0.0, V);
      steps += run.steps;
      SAPCA_CHECK(run.converged, SAPCA_ERR_SVD,
                  checking ? who + ": the round that looks for a missed copy of a repeated eigenvalue did not converge in " +
                                 num((uint64_t)run.steps) + " steps (" + num((uint64_t)steps) + " in all)"
                           : who + ": Lanczos did not converge " + num((uint64_t)want) + " of " + num((uint64_t)n_eigen) + " pairs in " +
                                 num((uint64_t)steps) + " steps");
      const int got = run.exhausted ? (int)std::min<int64_t>(want, run.steps) : want;
      if (checking && !(run.theta[(size_t)(run.steps - 1)] > vals[(size_t)order[(size_t)(k - 1)]] + opts->tol)) break;
      // the Ritz vectors of the `got` largest values, combined in f64 one by one, then moved in behind the locked ones
      std::vector<double> Zk((size_t)run.steps * got);
      for (int i = 0; i < got; ++i) {
        const int64_t col = run.steps - 1 - i;
        vals.push_back(run.theta[(size_t)col]);
        for (int64_t j = 0; j < run.steps; ++j) Zk[(size_t)i * run.steps + j] = run.Z[(size_t)j * run.steps + col];
      }
      double* Zdev = w.ritz_s.as<double>(Zk.size());
      SAPCA_HIP(hipMemcpyAsync(Zdev, Zk.data(), Zk.size() * sizeof(double), hipMemcpyHostToDevice, s));
      double* basis = V + (size_t)lock * m;
      for (int i = 0; i < got; ++i)
        KK::lanczos_combine<double>(basis, m, (int)run.steps, Zdev + (size_t)i * run.steps, 1, 1, R + (size_t)i * m, s);
      SAPCA_HIP(hipMemcpyAsync(basis, R, (size_t)got * m * sizeof(double), hipMemcpyDeviceToDevice, s));
      SAPCA_HIP(hipStreamSynchronize(s));   // (Zk leaves scope)
      sort_vals();
    }
    SAPCA_CHECK((int)vals.size() >= k, SAPCA_ERR_SVD,
                who + ": the complement of the locked vectors is empty with " + num((uint64_t)vals.size()) + " of " + num((uint64_t)k) +
                    " pairs");
    // the k largest, sign-fixed and rounded once
    for (int i = 0; i < k; ++i) {
      evals[c + i] = vals[(size_t)order[(size_t)i]];
      KK::spectral_store<T>(V + (size_t)(c + order[(size_t)i]) * m, m, 1, m, 1, true, signs, d_evecs, n_eigen, c + i, s);
    }
  }
  SAPCA_HIP(hipStreamSynchronize(s));   // complete when the call returns
  if (n_components) *n_components = ncomp;
  if (n_steps) *n_steps = (uint32_t)steps;
}

template <typename T>
void spectral_host(H& h, uint64_t m, uint64_t nnz, const int64_t* ptr, const int32_t* idx, const T* val, const sapca_spectral_options* opts,
                   double* evals, T* evecs, uint64_t* n_components, uint32_t* n_steps) {
  const std::string who("spectral");
  check_options(opts, m, who);
  check_graph(unchecked_view<T>(m, m, nnz, ptr, idx, val), who);
  if (n_components) *n_components = 0;
  if (n_steps) *n_steps = 0;
  if (m == 0) return;
  SAPCA_CHECK(evals != nullptr && evecs != nullptr, SAPCA_ERR_ARG, who + ": a NULL output with m = " + num(m));
  H::Spectral& w = h.spectral;
  hipStream_t s = h.stream;
  int64_t* dp = w.in_ptr.as<int64_t>(m + 1);
  int32_t* di = w.in_idx.as<int32_t>(std::max<size_t>(nnz, 1));
  T* dv = w.in_val.as<T>(std::max<size_t>(nnz, 1));
  T* de = w.evecs.as<T>((size_t)m * opts->n_eigen);
  SAPCA_HIP(hipMemcpyAsync(dp, ptr, (m + 1) * sizeof(int64_t), hipMemcpyHostToDevice, s));
  if (nnz) {
    SAPCA_HIP(hipMemcpyAsync(di, idx, nnz * sizeof(int32_t), hipMemcpyHostToDevice, s));
    SAPCA_HIP(hipMemcpyAsync(dv, val, nnz * sizeof(T), hipMemcpyHostToDevice, s));
  }
  spectral_device<T>(h, unchecked_view<T>(m, m, nnz, dp, di, dv), opts, evals, de, n_components, n_steps);
  SAPCA_HIP(hipMemcpyAsync(evecs, de, (size_t)m * opts->n_eigen * sizeof(T), hipMemcpyDeviceToHost, s));
  SAPCA_HIP(hipStreamSynchronize(s));
}

template <typename T>
void umap_spectral_init(H& h, uint64_t m, uint32_t output_dim, const T* d_evecs, uint64_t ld, uint32_t n_eigen, uint32_t seed, T* d_y) {
  const std::string who("umap_spectral_init");
  SAPCA_CHECK(output_dim >= 1 && output_dim <= 3, SAPCA_ERR_ARG, who + ": output_dim = " + num(output_dim) + " is outside 1 .. 3");
  SAPCA_CHECK(n_eigen > output_dim, SAPCA_ERR_ARG,
              who + ": n_eigen = " + num(n_eigen) + " eigenvectors do not hold output_dim = " + num(output_dim) + " behind the first");
  SAPCA_CHECK(ld >= n_eigen, SAPCA_ERR_ARG, who + ": ld = " + num(ld) + " is less than n_eigen = " + num(n_eigen));
  check_stride_limit(ld, who);
  check_rows(m, who);
  if (m == 0) return;
  SAPCA_CHECK(d_evecs != nullptr && d_y != nullptr, SAPCA_ERR_ARG, who + ": a NULL panel with m = " + num(m));
  unsigned long long* mx = h.spectral.mx.as<unsigned long long>(1);
  KK::umap_spectral_init<T>(d_evecs, (int64_t)ld, (int64_t)m, (int)output_dim, seed, mx, d_y, h.stream);
  SAPCA_HIP(hipStreamSynchronize(h.stream));
}

#define SAPCA_INSTANTIATE_SPECTRAL(T)                                                                                                  \
  template void spectral_scale<T>(H&, const CsrView<T>&, uint32_t, double*);                                                           \
  template void spectral_apply<T>(H&, const CsrView<T>&, uint32_t, const double*, double*);                                            \
  template void spectral_device<T>(H&, const CsrView<T>&, const sapca_spectral_options*, double*, T*, uint64_t*, uint32_t*);           \
  template void spectral_host<T>(H&, uint64_t, uint64_t, const int64_t*, const int32_t*, const T*, const sapca_spectral_options*,      \
                                 double*, T*, uint64_t*, uint32_t*);                                                                   \
  template void umap_spectral_init<T>(H&, uint64_t, uint32_t, const T*, uint64_t, uint32_t, uint32_t, T*);
SAPCA_INSTANTIATE_SPECTRAL(float)
SAPCA_INSTANTIATE_SPECTRAL(double)
#undef SAPCA_INSTANTIATE_SPECTRAL

}  // namespace resident
}  // namespace sapca
