// Highly variable genes (include/sapca.h, "Variable genes"): the device side of sapca_hvg_moments_csr_device_*, sapca_loess_f64
// and sapca_hvg_csr_device_*.
//
// Moments.  One wave per row of A^T (a column of A): the stored entries of the included rows are transformed in f64, each lane
// sums every 64th entry in stored order, and the 64 partial sums are folded by a fixed butterfly.  transpose_csr leaves a
// column's entries in ascending row order, so a value depends on the column's content alone: no atomic, no order reaches it,
// the same bytes from call to call.  The error of a sum of L terms is below (L / 64 + 7) ulp of the sum of their magnitudes.
// A row whose label excludes it costs its index and its label, its value is not read.
//
// Loess.  The abscissae are sorted once (rocPRIM, stable), so the q nearest neighbours of a point are a contiguous window whose
// start a bisection finds.  One wave per point walks its window, accumulates the eight weighted moments of {1, t, t^2} against
// {1, t, t^2, y} in f64 and folds them by the same butterfly; every lane then solves the 3 x 3 (or 2 x 2) normal equations.
//
// The n-sized steps of the seurat_v3 chain between the two matrix passes are the small kernels at the end; they are compiled
// without FMA contraction so that they round like the host arithmetic that states them.
#include <algorithm>
#include <cstring>
#include <string>

#include <rocprim/rocprim.hpp>

#include "kernels.h"

namespace sapca {
namespace k {

namespace {

constexpr int WAVE = 64;
constexpr int WAVES = 4;   // rows of A^T / loess points in flight per 256-thread workgroup

__device__ inline double wave_sum(double x) {
#pragma unroll
  for (int off = WAVE / 2; off > 0; off >>= 1) x += __shfl_xor(x, off);
  return x;
}
__device__ inline uint32_t wave_sum_u32(uint32_t x) {
#pragma unroll
  for (int off = WAVE / 2; off > 0; off >>= 1) x += __shfl_xor(x, off);
  return x;
}

// F: kHvgPlain (x), SAPCA_HVG_CLIP (min(x, clip[j])), SAPCA_HVG_EXPM1 (expm1(x)), x the stored value as an f64.
// labels null: every row; batch >= 0: the rows with that label; batch < 0: the rows whose label is in [0, nk).
template <typename T, int F>
__global__ void __launch_bounds__(WAVE * WAVES)
hvg_moments_kernel(const int64_t* __restrict__ ptr, const int32_t* __restrict__ idx, const T* __restrict__ val, int64_t cols,
                   const int32_t* __restrict__ labels, int32_t batch, int nk, const double* __restrict__ clip,
                   double* __restrict__ out_sum, double* __restrict__ out_sumsq, uint32_t* __restrict__ out_clipped) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int64_t j = (int64_t)blockIdx.x * WAVES + threadIdx.x / WAVE;
  if (j >= cols) return;   // (wave-uniform)
  const double cl = F == SAPCA_HVG_CLIP ? clip[j] : 0.0;
  double s = 0.0, q = 0.0;
  uint32_t c = 0;
  const int64_t e1 = ptr[j + 1];
  for (int64_t e = ptr[j] + lane; e < e1; e += WAVE) {
    if (labels != nullptr) {
      const int32_t code = labels[idx[e]];
      if (batch >= 0 ? code != batch : (unsigned)code >= (unsigned)nk) continue;
    }
    double x = (double)val[e];
    if (F == SAPCA_HVG_CLIP) {
      if (x > cl) {
        x = cl;
        ++c;
      }
    } else if (F == SAPCA_HVG_EXPM1) {
      x = expm1(x);
    }
    s += x;
    q += x * x;
  }
  s = wave_sum(s);
  q = wave_sum(q);
  c = wave_sum_u32(c);
  if (lane == 0) {
    out_sum[j] = s;
    out_sumsq[j] = q;
    if (out_clipped) out_clipped[j] = c;
  }
}

__global__ void __launch_bounds__(256) hvg_iota_kernel(uint32_t* __restrict__ v, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) v[i] = (uint32_t)i;
}

__global__ void __launch_bounds__(256) hvg_gather_kernel(const double* __restrict__ y, const uint32_t* __restrict__ perm, int64_t n,
                                                         double* __restrict__ ys) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) ys[i] = y[perm[i]];
}

// The fit at the sorted position i of xs[0 .. nv) (ascending), ys alongside; fit[perm[i]] receives it.
__global__ void __launch_bounds__(WAVE * WAVES)
hvg_loess_kernel(const double* __restrict__ xs, const double* __restrict__ ys, const uint32_t* __restrict__ perm, int64_t nv, int64_t q,
                 double* __restrict__ fit) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int64_t i = (int64_t)blockIdx.x * WAVES + threadIdx.x / WAVE;
  if (i >= nv) return;   // (wave-uniform)
  const double xi = xs[i];
  // the window [lo, lo + q): the first start at which the point behind the window is no nearer than the window's first
  int64_t a = i - q + 1 > 0 ? i - q + 1 : 0, b = i < nv - q ? i : nv - q;
  while (a < b) {
    const int64_t mid = a + ((b - a) >> 1);
    const bool slide = mid + q < nv && xs[mid + q] - xi < xi - xs[mid];
    if (slide) a = mid + 1;
    else b = mid;
  }
  const int64_t lo = a;
  const double h = fmax(xi - xs[lo], xs[lo + q - 1] - xi);   // the q-th smallest distance
  double S0 = 0, S1 = 0, S2 = 0, S3 = 0, S4 = 0, T0 = 0, T1 = 0, T2 = 0;
  uint32_t distinct = 0;
  if (h > 0.0) {
    for (int64_t j = lo + lane; j < lo + q; j += WAVE) {
      const double d = xs[j] - xi;
      const double r = fabs(d) / h;
      if (!(r < 1.0)) continue;
      const double u = 1.0 - r * r * r;
      const double w = u * u * u;
      if (!(w > 0.0)) continue;
      const double t = d / h, y = ys[j];
      const double wt = w * t, wt2 = wt * t;
      S0 += w;
      S1 += wt;
      S2 += wt2;
      S3 += wt2 * t;
      S4 += wt2 * t * t;
      T0 += w * y;
      T1 += wt * y;
      T2 += wt2 * y;
      // the first of a run of equal abscissae (equal abscissae carry equal weights, so the whole run is weighted)
      distinct += (j == lo || xs[j - 1] != xs[j]) ? 1u : 0u;
    }
    S0 = wave_sum(S0); S1 = wave_sum(S1); S2 = wave_sum(S2); S3 = wave_sum(S3); S4 = wave_sum(S4);
    T0 = wave_sum(T0); T1 = wave_sum(T1); T2 = wave_sum(T2);
    distinct = wave_sum_u32(distinct);
  }
  double out;
  if (distinct >= 3) {   // quadratic: the normal equations of {1, t, t^2}, eliminated without pivoting (positive definite)
    double a00 = S0, a01 = S1, a02 = S2, a11 = S2, a12 = S3, a22 = S4, b0 = T0, b1 = T1, b2 = T2;
    const double l10 = a01 / a00, l20 = a02 / a00;
    a11 -= l10 * a01; a12 -= l10 * a02; b1 -= l10 * b0;
    a22 -= l20 * a02; b2 -= l20 * b0;
    const double l21 = a12 / a11;
    a22 -= l21 * a12; b2 -= l21 * b1;
    const double x2 = b2 / a22;
    const double x1 = (b1 - a12 * x2) / a11;
    out = (b0 - a01 * x1 - a02 * x2) / a00;
  } else if (distinct == 2) {   // linear
    out = (T0 * S2 - T1 * S1) / (S0 * S2 - S1 * S1);
  } else {   // h == 0 or one abscissa: the plain mean of y over the points with x == x_i
    int64_t e0 = 0, e1 = i;   // lower bound of xi
    while (e0 < e1) {
      const int64_t mid = e0 + ((e1 - e0) >> 1);
      if (xs[mid] < xi) e0 = mid + 1;
      else e1 = mid;
    }
    int64_t f0 = i + 1, f1 = nv;   // upper bound
    while (f0 < f1) {
      const int64_t mid = f0 + ((f1 - f0) >> 1);
      if (xs[mid] > xi) f1 = mid;
      else f0 = mid + 1;
    }
    double sy = 0.0;
    for (int64_t j = e0 + lane; j < f0; j += WAVE) sy += ys[j];
    sy = wave_sum(sy);
    out = sy / (double)(f0 - e0);
  }
  if (lane == 0) fit[perm[i]] = out;
}

// ---- the n-sized steps of the seurat_v3 chain (no contraction: they round as the host statement does) ----
#pragma clang fp contract(off)

// mean = s / N, var = (ss / N - mean^2) N / (N - 1); lx = log10(mean) where var > 0, +inf elsewhere (sorts behind every fit
// point); ly = log10(var); *n_valid counts the columns with var > 0 (an integer atomic)
__global__ void __launch_bounds__(256)
hvg_mean_var_kernel(const double* __restrict__ s, const double* __restrict__ ss, double N, int64_t n, double* __restrict__ mean,
                    double* __restrict__ var, double* __restrict__ lx, double* __restrict__ ly, uint32_t* __restrict__ n_valid) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const double mu = s[j] / N;
  const double msq = ss[j] / N;
  const double mu2 = mu * mu;
  const double v = (msq - mu2) * (N / (N - 1.0));
  mean[j] = mu;
  var[j] = v;
  const bool ok = v > 0.0;
  lx[j] = ok ? log10(mu) : __builtin_huge_val();
  ly[j] = ok ? log10(v) : 0.0;
  if (ok) atomicAdd(n_valid, 1u);
}

// reg_std = sqrt(10^est), clip = reg_std sqrt(N) + mean
__global__ void __launch_bounds__(256) hvg_clip_kernel(const double* __restrict__ est, const double* __restrict__ mean, double N,
                                                       int64_t n, double* __restrict__ reg_std, double* __restrict__ clip) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const double r = sqrt(pow(10.0, est[j]));
  const double rn = r * sqrt(N);
  reg_std[j] = r;
  clip[j] = rn + mean[j];
}

// norm_var = (N mean^2 + ss - 2 s mean) / ((N - 1) reg_std^2), s and ss the clipped moments
__global__ void __launch_bounds__(256)
hvg_norm_var_kernel(const double* __restrict__ s, const double* __restrict__ ss, const double* __restrict__ mean,
                    const double* __restrict__ reg_std, double N, int64_t n, double* __restrict__ norm_var) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const double mu = mean[j], r = reg_std[j];
  const double t1 = N * (mu * mu);
  const double t2 = 2.0 * s[j] * mu;
  const double num = (t1 + ss[j]) - t2;
  const double den = (N - 1.0) * (r * r);
  norm_var[j] = num / den;
}

unsigned blocks_of(int64_t items, int per_block, const char* who) {
  const int64_t blocks = (items + per_block - 1) / per_block;
  SAPCA_CHECK(blocks < ((int64_t)1 << 31), SAPCA_ERR_ARG, std::string(who) + ": too many items");
  return (unsigned)blocks;
}

}  // namespace

template <typename T>
void hvg_moments(const CsrView<T>& At, const int32_t* labels, int32_t batch, int nk, int transform, const double* d_clip, double* sum,
                 double* sumsq, uint32_t* n_clipped, hipStream_t s) {
  if (At.rows == 0) return;
  const dim3 grid(blocks_of(At.rows, WAVES, "hvg_moments")), block(WAVE * WAVES);
#define SAPCA_HVG_LAUNCH(F)                                                                                                       \
  hipLaunchKernelGGL((hvg_moments_kernel<T, F>), grid, block, 0, s, At.ptr, At.idx, At.val, At.rows, labels, batch, nk, d_clip, sum, \
                     sumsq, n_clipped)
  if (transform == SAPCA_HVG_CLIP) SAPCA_HVG_LAUNCH(SAPCA_HVG_CLIP);
  else if (transform == SAPCA_HVG_EXPM1) SAPCA_HVG_LAUNCH(SAPCA_HVG_EXPM1);
  else SAPCA_HVG_LAUNCH(kHvgPlain);
#undef SAPCA_HVG_LAUNCH
  SAPCA_HIP(hipGetLastError());
}

void hvg_loess(const double* x, const double* y, int64_t n, int64_t nv, int64_t q, double* xs, double* ys, uint32_t* iota, uint32_t* perm,
               double* fit, DevBuf& sort_tmp, hipStream_t s) {
  if (n == 0 || nv == 0) return;
  hipLaunchKernelGGL(hvg_iota_kernel, dim3(blocks_of(n, 256, "hvg_loess")), dim3(256), 0, s, iota, n);
  size_t bytes = 0;
  SAPCA_HIP(rocprim::radix_sort_pairs(nullptr, bytes, (const double*)nullptr, (double*)nullptr, (const uint32_t*)nullptr,
                                      (uint32_t*)nullptr, (size_t)n, 0u, 64u, s));
  void* tmp = sort_tmp.ensure(std::max<size_t>(bytes, 16));
  SAPCA_HIP(rocprim::radix_sort_pairs(tmp, bytes, x, xs, iota, perm, (size_t)n, 0u, 64u, s));
  hipLaunchKernelGGL(hvg_gather_kernel, dim3(blocks_of(nv, 256, "hvg_loess")), dim3(256), 0, s, y, perm, nv, ys);
  hipLaunchKernelGGL(hvg_loess_kernel, dim3(blocks_of(nv, WAVES, "hvg_loess")), dim3(WAVE * WAVES), 0, s, xs, ys, perm, nv, q, fit);
  SAPCA_HIP(hipGetLastError());
}

void hvg_mean_var(const double* s_, const double* ss, double N, int64_t n, double* mean, double* var, double* lx, double* ly,
                  uint32_t* n_valid, hipStream_t s) {
  SAPCA_HIP(hipMemsetAsync(n_valid, 0, sizeof(uint32_t), s));
  if (n == 0) return;
  hipLaunchKernelGGL(hvg_mean_var_kernel, dim3(blocks_of(n, 256, "hvg_mean_var")), dim3(256), 0, s, s_, ss, N, n, mean, var, lx, ly,
                     n_valid);
  SAPCA_HIP(hipGetLastError());
}

void hvg_clip(const double* est, const double* mean, double N, int64_t n, double* reg_std, double* clip, hipStream_t s) {
  if (n == 0) return;
  hipLaunchKernelGGL(hvg_clip_kernel, dim3(blocks_of(n, 256, "hvg_clip")), dim3(256), 0, s, est, mean, N, n, reg_std, clip);
  SAPCA_HIP(hipGetLastError());
}

void hvg_norm_var(const double* s_, const double* ss, const double* mean, const double* reg_std, double N, int64_t n, double* norm_var,
                  hipStream_t s) {
  if (n == 0) return;
  hipLaunchKernelGGL(hvg_norm_var_kernel, dim3(blocks_of(n, 256, "hvg_norm_var")), dim3(256), 0, s, s_, ss, mean, reg_std, N, n,
                     norm_var);
  SAPCA_HIP(hipGetLastError());
}

#define INSTANTIATE(T)                                                                                                              \
  template void hvg_moments<T>(const CsrView<T>&, const int32_t*, int32_t, int, int, const double*, double*, double*, uint32_t*, \
                               hipStream_t);
INSTANTIATE(float)
INSTANTIATE(double)
#undef INSTANTIATE

}  // namespace k
}  // namespace sapca
