// Stand-alone driver of the host solvers in single-algebra_amd/csrc/small_svd.cpp (pure host code, no HIP): sym_eigh_desc (every
// f32 randomized fit), jacobi_svd (every f64 one) and tridiag_eigh in both last_row_only modes (every Lanczos fit).
//   g++ -std=c++17 -O2 tools/small_svd_check.cpp single-algebra_amd/csrc/small_svd.cpp -o small_svd_check
//   ./small_svd_check cases.bin results.bin      (tests/test_small_svd_cpu.py writes the cases and compares the results)
//   ./small_svd_check                            (a built-in set: graded, equal, rank-deficient, indefinite, zero, diagonal, scaled)
// and for a run under the host sanitizers:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all tools/small_svd_check.cpp
//       single-algebra_amd/csrc/small_svd.cpp -o small_svd_check && ./small_svd_check && ./small_svd_check cases.bin results.bin
// Cases file: records of (int64 kind, int64 n, doubles): kind 0 = sym_eigh_desc, n x n row-major; 1 = jacobi_svd, n x n row-major;
// 2 = tridiag_eigh, d[0..n) then e[0..n) (e[i] couples i - 1 and i, e[0] unused).  Results file, per record:
//   0: int64 converged, w[n] descending, Vt[n x n] (row i: the eigenvector of w[i])
//   1: s[n] descending, U[n x n] row-major (column c: the left vector of s[c])
//   2: int64 converged, d[n] ascending, Z[n x n] (columns), then the same call with last_row_only: int64, d[n], Z[1 x n]
// The vectors handed to the solvers have exactly the sizes the solvers are documented to read.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../single-algebra_amd/csrc/small_svd.h"

static bool get(std::FILE* f, void* p, size_t bytes) { return std::fread(p, 1, bytes, f) == bytes; }
static void put(std::FILE* f, const void* p, size_t bytes) {
  if (std::fwrite(p, 1, bytes, f) != bytes) { std::perror("write"); std::exit(2); }
}
static void put_vec(std::FILE* f, const std::vector<double>& v) { if (!v.empty()) put(f, v.data(), v.size() * sizeof(double)); }

static int run_file(const char* in_path, const char* out_path) {
  std::FILE* in = std::fopen(in_path, "rb");
  std::FILE* out = std::fopen(out_path, "wb");
  if (!in || !out) { std::perror("open"); return 2; }
  int64_t kind = 0, n = 0, records = 0;
  while (get(in, &kind, sizeof kind)) {
    if (!get(in, &n, sizeof n) || n < 0 || n > 4096 || kind < 0 || kind > 2) { std::fprintf(stderr, "bad record header\n"); return 2; }
    const size_t nn = (size_t)n * n;
    if (kind == 2) {
      std::vector<double> d((size_t)n), e((size_t)n);
      if (n && (!get(in, d.data(), n * sizeof(double)) || !get(in, e.data(), n * sizeof(double)))) { std::fprintf(stderr, "short record\n"); return 2; }
      for (int mode = 0; mode < 2; ++mode) {
        std::vector<double> dd(d), ee(e), Z;
        const int64_t ok = sapca::tridiag_eigh(dd, ee, (int)n, Z, mode == 1) ? 1 : 0;
        if (Z.size() != (mode ? (size_t)n : nn) || dd.size() != (size_t)n) { std::fprintf(stderr, "tridiag_eigh: output sizes\n"); return 2; }
        put(out, &ok, sizeof ok);
        put_vec(out, dd);
        put_vec(out, Z);
      }
    } else {
      std::vector<double> A(nn);
      if (nn && !get(in, A.data(), nn * sizeof(double))) { std::fprintf(stderr, "short record\n"); return 2; }
      if (kind == 0) {
        std::vector<double> w, Vt;
        const int64_t ok = sapca::sym_eigh_desc(A, (int)n, w, Vt) ? 1 : 0;
        if (w.size() != (size_t)n || Vt.size() != nn) { std::fprintf(stderr, "sym_eigh_desc: output sizes\n"); return 2; }
        put(out, &ok, sizeof ok);
        put_vec(out, w);
        put_vec(out, Vt);
      } else {
        std::vector<double> U, s;
        sapca::jacobi_svd(A, (int)n, U, s);
        if (s.size() != (size_t)n || U.size() != nn) { std::fprintf(stderr, "jacobi_svd: output sizes\n"); return 2; }
        put_vec(out, s);
        put_vec(out, U);
      }
    }
    ++records;
  }
  std::fclose(in);
  if (std::fclose(out) != 0) { std::perror("close"); return 2; }
  std::printf("%lld records\n", (long long)records);
  return 0;
}

// ---- the built-in set
static uint64_t lcg = 88172645463325252ull;
static double rnd() {   // uniform in (-1, 1)
  lcg = lcg * 6364136223846793005ull + 1442695040888963407ull;
  return (double)(lcg >> 11) / 4503599627370496.0 - 1.0;
}

static int failures = 0;
static void expect(bool ok, const char* what, const char* name, int n) {
  if (!ok) { std::printf("FAIL %s n = %d: %s\n", name, n, what); ++failures; }
}

// A = B diag(sigma) B^T-like symmetric matrix from a random B (not orthogonal: the spectrum is only roughly sigma's)
static std::vector<double> symmetric(int n, const std::vector<double>& sigma) {
  std::vector<double> B((size_t)n * n), A((size_t)n * n, 0.0);
  for (auto& x : B) x = rnd();
  for (int i = 0; i < n; ++i)
    for (int j = 0; j <= i; ++j) {
      double acc = 0;
      for (int t = 0; t < n; ++t) acc += B[(size_t)i * n + t] * sigma[t] * B[(size_t)j * n + t];
      A[(size_t)i * n + j] = A[(size_t)j * n + i] = acc;
    }
  return A;
}

static void check_sym(const char* name, const std::vector<double>& A, int n) {
  std::vector<double> w, Vt;
  expect(sapca::sym_eigh_desc(A, n, w, Vt), "converged", name, n);
  double amax = 0, res = 0, orth = 0;
  for (double x : A) amax = std::fmax(amax, std::fabs(x));
  for (int i = 0; i + 1 < n; ++i) expect(w[i] >= w[i + 1], "descending", name, n);
  for (int i = 0; i < n; ++i)
    for (int r = 0; r < n; ++r) {
      double av = 0, dot = 0;
      for (int c = 0; c < n; ++c) { av += A[(size_t)r * n + c] * Vt[(size_t)i * n + c]; dot += Vt[(size_t)i * n + c] * Vt[(size_t)r * n + c]; }
      res = std::fmax(res, std::fabs(av - w[i] * Vt[(size_t)i * n + r]));
      orth = std::fmax(orth, std::fabs(dot - (i == r ? 1.0 : 0.0)));
    }
  expect(res <= 64.0 * n * n * 2.2e-16 * std::fmax(amax, 1e-300), "A v = w v", name, n);
  expect(orth <= 64.0 * n * 2.2e-16, "V V^T = I", name, n);
  // Jacobi on the same matrix: singular values = |eigenvalues|, U orthonormal where s > 0
  std::vector<double> U, s;
  sapca::jacobi_svd(A, n, U, s);
  for (int i = 0; i + 1 < n; ++i) expect(s[i] >= s[i + 1], "Jacobi descending", name, n);
  for (int c = 0; c < n; ++c) {
    double nrm = 0;
    for (int i = 0; i < n; ++i) nrm += U[(size_t)i * n + c] * U[(size_t)i * n + c];
    expect(s[c] > 0 ? std::fabs(nrm - 1.0) <= 1e-13 : nrm == 0.0, "Jacobi column norm", name, n);
  }
  // the tridiagonal solver on the matrix's own diagonal and first sub-diagonal, both modes
  std::vector<double> d((size_t)n), e((size_t)n, 0.0), Z, d1, e1, Z1;
  for (int i = 0; i < n; ++i) { d[i] = A[(size_t)i * n + i]; if (i) e[i] = A[(size_t)i * n + i - 1]; }
  d1 = d; e1 = e;
  expect(sapca::tridiag_eigh(d, e, n, Z, false) && sapca::tridiag_eigh(d1, e1, n, Z1, true), "tridiagonal converged", name, n);
  expect(d == d1, "tridiagonal: same eigenvalues in both modes", name, n);
  for (int c = 0; c < n; ++c) expect(Z1[c] == Z[(size_t)(n - 1) * n + c], "tridiagonal: last row", name, n);
}

static int run_builtin() {
  for (int n : {1, 2, 3, 16, 61}) {
    std::vector<double> sigma((size_t)n);
    for (int i = 0; i < n; ++i) sigma[i] = std::pow(10.0, -12.0 * i / std::fmax(n - 1, 1));
    check_sym("graded", symmetric(n, sigma), n);
    for (int i = 0; i < n; ++i) sigma[i] = 1.0;
    check_sym("equal", symmetric(n, sigma), n);
    for (int i = 0; i < n; ++i) sigma[i] = i < n / 2 ? 1.0 + i : 0.0;
    check_sym("rank-deficient", symmetric(n, sigma), n);
    for (int i = 0; i < n; ++i) sigma[i] = (i % 2 ? -1.0 : 1.0) * (1.0 + i);
    check_sym("indefinite", symmetric(n, sigma), n);
    std::vector<double> Z((size_t)n * n, 0.0);
    check_sym("zero", Z, n);
    for (int i = 0; i < n; ++i) Z[(size_t)i * n + i] = (double)(i - n / 2);
    check_sym("diagonal", Z, n);
    for (double scale : {1e300, 1e-300}) {   // well conditioned (diagonally dominant), entries up to n * scale
      std::vector<double> S((size_t)n * n);
      for (int i = 0; i < n; ++i)
        for (int j = 0; j <= i; ++j) S[(size_t)i * n + j] = S[(size_t)j * n + i] = scale * (i == j ? n + rnd() : rnd());
      check_sym(scale > 1 ? "scaled 1e300" : "scaled 1e-300", S, n);
    }
  }
  std::printf(failures ? "%d FAILURES\n" : "ok\n", failures);
  return failures ? 1 : 0;
}

int main(int argc, char** argv) {
  if (argc == 3) return run_file(argv[1], argv[2]);
  if (argc == 1) return run_builtin();
  std::fprintf(stderr, "usage: %s [cases.bin results.bin]\n", argv[0]);
  return 2;
}
