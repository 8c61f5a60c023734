// sapca_covariate_basis (include/sapca.h): an orthonormal basis Q of the span of a covariate design D = [1 | z] (center) or z,
// and the map W with Q = D W.  Pure host code, f64, no handle and no HIP: a Householder QR with column pivoting of the
// design with its columns scaled to unit norm.  engine.cpp calls it once per fit with covariates.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <vector>

#include "../../include/sapca.h"

extern "C" sapca_status sapca_covariate_basis(const double* z, uint64_t rows, uint64_t cols, int32_t center, double* q, double* w,
                                              uint64_t* rank) {
  constexpr uint64_t kMax = SAPCA_MAX_DESIGN_COLUMNS;
  const uint64_t dc = cols + (center ? 1u : 0u);
  if (cols > kMax || dc > kMax || (rows > 0 && !q) || (dc > 0 && !w) || !rank) return SAPCA_ERR_ARG;
  if (rows * cols > 0 && !z) return SAPCA_ERR_ARG;
  for (uint64_t i = 0; i < rows * cols; ++i)
    if (!std::isfinite(z[i])) return SAPCA_ERR_ARG;
  if (rows > 0) std::fill(q, q + rows * kMax, 0.0);
  if (dc > 0) std::fill(w, w + dc * kMax, 0.0);
  *rank = 0;
  if (rows == 0 || dc == 0) return SAPCA_OK;

  // the design, column-major, every column scaled to unit norm (a zero column stays zero and never becomes a pivot)
  const size_t m = (size_t)rows, n = (size_t)dc;
  std::vector<double> a(m * n), scale(n, 0.0);
  for (size_t j = 0; j < n; ++j) {
    double* col = a.data() + j * m;
    if (center && j == 0) {
      std::fill(col, col + m, 1.0);
    } else {
      const size_t zj = j - (center ? 1 : 0);
      for (size_t i = 0; i < m; ++i) col[i] = z[i * (size_t)cols + zj];
    }
    double big = 0;
    for (size_t i = 0; i < m; ++i) big = std::max(big, std::fabs(col[i]));
    if (big == 0) continue;
    double ss = 0;   // (scaled by the largest entry: no overflow or underflow of the squares)
    for (size_t i = 0; i < m; ++i) { const double t = col[i] / big; ss += t * t; }
    const double nrm = big * std::sqrt(ss);
    scale[j] = 1.0 / nrm;
    for (size_t i = 0; i < m; ++i) col[i] *= scale[j];
  }

  // Householder QR with column pivoting: A P = Q R.  Step s: the column of largest remaining norm comes to position s, a
  // reflector H_s = I - tau v v^T (v[s] = 1, stored below the diagonal) zeroes it below the diagonal.
  const size_t steps = std::min(m, n);
  std::vector<size_t> piv(n);
  for (size_t j = 0; j < n; ++j) piv[j] = j;
  std::vector<double> tau(steps, 0.0), rdiag(steps, 0.0);
  size_t done = 0;
  for (size_t s = 0; s < steps; ++s, ++done) {
    size_t best = s;
    double best_nrm = -1;
    for (size_t j = s; j < n; ++j) {   // (remaining norms recomputed, not down-dated: at most 16 columns)
      double ss = 0;
      for (size_t i = s; i < m; ++i) ss += a[j * m + i] * a[j * m + i];
      if (ss > best_nrm) { best_nrm = ss; best = j; }
    }
    if (best != s) {
      std::swap_ranges(a.begin() + s * m, a.begin() + (s + 1) * m, a.begin() + best * m);
      std::swap(piv[s], piv[best]);
    }
    double* x = a.data() + s * m;
    const double alpha = std::sqrt(best_nrm);
    if (alpha == 0) break;   // everything that remains is zero
    const double beta = x[s] >= 0 ? -alpha : alpha;
    tau[s] = (beta - x[s]) / beta;
    const double inv = 1.0 / (x[s] - beta);
    for (size_t i = s + 1; i < m; ++i) x[i] *= inv;
    x[s] = beta;
    rdiag[s] = beta;
    for (size_t j = s + 1; j < n; ++j) {
      double* y = a.data() + j * m;
      double dot = y[s];
      for (size_t i = s + 1; i < m; ++i) dot += x[i] * y[i];
      dot *= tau[s];
      y[s] -= dot;
      for (size_t i = s + 1; i < m; ++i) y[i] -= dot * x[i];
    }
  }

  // r = #{j : |R_jj| > max(rows, design columns) eps |R_00|}
  const double tol = (double)std::max(m, n) * std::numeric_limits<double>::epsilon() * std::fabs(rdiag[0]);
  size_t r = 0;
  while (r < done && std::fabs(rdiag[r]) > tol) ++r;
  *rank = (uint64_t)r;
  if (r == 0) return SAPCA_OK;

  // Q = H_0 .. H_{r-1} applied to the first r unit vectors
  std::vector<double> qc(m);
  for (size_t c = 0; c < r; ++c) {
    std::fill(qc.begin(), qc.end(), 0.0);
    qc[c] = 1.0;
    for (size_t s = r; s-- > 0;) {
      const double* v = a.data() + s * m;
      double dot = qc[s];
      for (size_t i = s + 1; i < m; ++i) dot += v[i] * qc[i];
      dot *= tau[s];
      qc[s] -= dot;
      for (size_t i = s + 1; i < m; ++i) qc[i] -= dot * v[i];
    }
    for (size_t i = 0; i < m; ++i) q[i * kMax + c] = qc[i];
  }

  // W: the basic solution on the pivot columns.  (D S)[:, piv[0..r)] = Q R11 with S = diag(scale), so
  // Q = D W with W[piv[i]][:] = scale[piv[i]] * (R11^-1)[i][:] and zero rows for the dependent columns.
  std::vector<double> rinv(r * r, 0.0);
  for (size_t c = 0; c < r; ++c) {   // back substitution, column c of R11^-1
    for (size_t i = c + 1; i-- > 0;) {
      double acc = i == c ? 1.0 : 0.0;
      for (size_t t = i + 1; t <= c; ++t) acc -= a[t * m + i] * rinv[t * r + c];   // R[i][t] = a[column t][row i]
      rinv[i * r + c] = acc / a[i * m + i];
    }
  }
  for (size_t i = 0; i < r; ++i)
    for (size_t c = 0; c < r; ++c) w[piv[i] * kMax + c] = scale[piv[i]] * rinv[i * r + c];
  return SAPCA_OK;
}
