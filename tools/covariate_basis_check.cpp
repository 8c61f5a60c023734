// Stand-alone check of sapca_covariate_basis (single-algebra_amd/csrc/covariates.cpp: pure host code, no HIP) for runs under
// the host sanitizers:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all tools/covariate_basis_check.cpp
//       single-algebra_amd/csrc/covariates.cpp -o covariate_basis_check && ./covariate_basis_check
// Designs: full rank, one-hot + intercept (collinear), a zero column, a 1e4-scale column beside 0/1 codes, rank 0, sixteen
// design columns, more columns than rows, one row, no rows, and the refusals.  Every design is checked for Q^T Q = I, Q = D W
// and D = Q Q^T D; the output buffers are allocated at their exact sizes so that any write past them is caught.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../include/sapca.h"

static uint64_t lcg = 88172645463325252ull;
static double rnd() {   // uniform in (-1, 1)
  lcg = lcg * 6364136223846793005ull + 1442695040888963407ull;
  return (double)(lcg >> 11) / 4503599627370496.0 - 1.0;
}

static int failures = 0;
static void expect(bool ok, const char* what, const char* name) {
  if (!ok) { std::printf("FAIL %s: %s\n", name, what); ++failures; }
}

static void run(const char* name, const std::vector<double>& z, uint64_t rows, uint64_t cols, int center, uint64_t want_rank) {
  const uint64_t dc = cols + (center ? 1 : 0);
  std::vector<double> q(rows * 16), w(dc * 16);
  uint64_t rank = 99;
  const sapca_status st = sapca_covariate_basis(z.empty() ? nullptr : z.data(), rows, cols, center, q.data(), w.data(), &rank);
  expect(st == SAPCA_OK, "status", name);
  expect(rank == want_rank, "rank", name);
  if (st != SAPCA_OK) return;
  auto d = [&](uint64_t i, uint64_t j) { return center ? (j == 0 ? 1.0 : z[i * cols + j - 1]) : z[i * cols + j]; };
  double e_orth = 0, e_dw = 0, e_span = 0, dmax = 0;
  for (uint64_t a = 0; a < 16; ++a)
    for (uint64_t b = 0; b < 16; ++b) {
      double acc = 0;
      for (uint64_t i = 0; i < rows; ++i) acc += q[i * 16 + a] * q[i * 16 + b];
      e_orth = std::fmax(e_orth, std::fabs(acc - ((a == b && a < rank) ? 1.0 : 0.0)));
    }
  for (uint64_t i = 0; i < rows; ++i)
    for (uint64_t c = 0; c < 16; ++c) {
      double acc = 0;
      for (uint64_t j = 0; j < dc; ++j) acc += d(i, j) * w[j * 16 + c];
      e_dw = std::fmax(e_dw, std::fabs(acc - q[i * 16 + c]));
    }
  for (uint64_t j = 0; j < dc; ++j) {
    double coef[16];
    for (uint64_t c = 0; c < 16; ++c) {
      coef[c] = 0;
      for (uint64_t i = 0; i < rows; ++i) coef[c] += q[i * 16 + c] * d(i, j);
    }
    for (uint64_t i = 0; i < rows; ++i) {
      double acc = d(i, j);
      dmax = std::fmax(dmax, std::fabs(acc));
      for (uint64_t c = 0; c < 16; ++c) acc -= q[i * 16 + c] * coef[c];
      e_span = std::fmax(e_span, std::fabs(acc));
    }
  }
  expect(e_orth <= 1e-13, "Q^T Q = I", name);
  expect(e_dw <= 1e-12, "Q = D W", name);
  expect(e_span <= 1e-12 * std::fmax(dmax, 1.0), "D = Q Q^T D", name);
  std::printf("%-28s rows %4llu design %2llu rank %2llu  |QtQ-I| %.1e  |DW-Q| %.1e  |D-QQtD| %.1e\n", name, (unsigned long long)rows,
              (unsigned long long)dc, (unsigned long long)rank, e_orth, e_dw, e_span);
}

int main() {
  const uint64_t m = 203;
  std::vector<double> z;
  auto fill = [&](uint64_t rows, uint64_t cols) { z.assign(rows * cols, 0.0); for (auto& x : z) x = rnd(); };
  fill(m, 5); run("full rank", z, m, 5, 1, 6);
  run("full rank, no intercept", z, m, 5, 0, 5);
  z.assign(m * 4, 0.0);
  for (uint64_t i = 0; i < m; ++i) z[i * 4 + i % 4] = 1.0;
  run("one-hot + intercept", z, m, 4, 1, 4);
  run("one-hot", z, m, 4, 0, 4);
  fill(m, 4);
  for (uint64_t i = 0; i < m; ++i) z[i * 4 + 2] = 0.0;
  run("zero column", z, m, 4, 1, 4);
  z.assign(m * 5, 0.0);
  for (uint64_t i = 0; i < m; ++i) { z[i * 5 + i % 4] = 1.0; z[i * 5 + 4] = 1e4 * (1.5 + 0.5 * rnd()); }
  run("badly scaled", z, m, 5, 1, 5);
  z.assign(m * 3, 0.0);
  run("rank 0", z, m, 3, 0, 0);
  fill(m, 15);
  for (uint64_t i = 0; i < m; ++i)
    for (uint64_t j = 0; j < 8; ++j) z[i * 15 + j] = (i * 7 + i / 5) % 8 == j ? 1.0 : 0.0;
  run("sixteen design columns", z, m, 15, 1, 15);
  fill(5, 9); run("more columns than rows", z, 5, 9, 1, 5);
  fill(1, 3); run("one row", z, 1, 3, 1, 1);
  z.clear(); run("no rows", z, 0, 3, 1, 0);
  run("intercept alone", z, 40, 0, 1, 1);

  std::vector<double> q(10 * 16), w(17 * 16);
  uint64_t rank = 0;
  fill(10, 16);
  expect(sapca_covariate_basis(z.data(), 10, 16, 1, q.data(), w.data(), &rank) == SAPCA_ERR_ARG, "17 design columns refused", "refusals");
  expect(sapca_covariate_basis(z.data(), 10, 16, 0, q.data(), w.data(), &rank) == SAPCA_OK && rank == 10, "16 design columns taken", "refusals");
  expect(sapca_covariate_basis(nullptr, 10, 2, 1, q.data(), w.data(), &rank) == SAPCA_ERR_ARG, "null z refused", "refusals");
  z[37] = NAN;
  expect(sapca_covariate_basis(z.data(), 10, 16, 0, q.data(), w.data(), &rank) == SAPCA_ERR_ARG, "nan refused", "refusals");
  z[37] = INFINITY;
  expect(sapca_covariate_basis(z.data(), 10, 16, 0, q.data(), w.data(), &rank) == SAPCA_ERR_ARG, "inf refused", "refusals");
  std::printf(failures ? "%d FAILURES\n" : "ok\n", failures);
  return failures ? 1 : 0;
}
