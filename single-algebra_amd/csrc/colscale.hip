// Implicit column scaling of a randomized fit (sapca_set_column_scaling): the operator is S = (A - 1 mu^T) diag(d) and only the
// thin column-side panels (n_used rows, one per column of S) ever meet d:
//   column_scale_factors   d (f64 and T), w = d mu (T) and sum_j d_j^2 var_j from the fit's f64 column sums
//   scale_panel_rows       P[r][:] *= d[r] in place: X <- D X in front of an A sweep, W = D V^T of a projection, D G
//   finish_scaled_panel    Z = D (sum of slabs - mu sv^T): the A^T side, from the state the sweep left its panel in
// All three are bound by the bytes they move (one read and one write of an n_used x ld panel that sits in L2 / Infinity Cache
// at the headline sizes); a lane owns one 16-byte vector.  Every output word has one writer and the one reduction adds its
// terms in a fixed order (per thread in index order, a tree in LDS, the workgroups' partials in block order by a second
// kernel): no atomics, the same bits from run to run.
#include <algorithm>

#include "kernels.h"

namespace sapca {
namespace k {

namespace {

constexpr int kThreads = 256;
constexpr int kPerThread = 4;                          // columns a thread of the factor kernel takes
constexpr int kPerBlock = kThreads * kPerThread;
constexpr double kEps64 = 2.220446049250313e-16;       // 2^-52, numpy's finfo(float64).eps

template <typename T> struct Vec16;
template <> struct Vec16<float> { static constexpr int N = 4; using type = float4; };
template <> struct Vec16<double> { static constexpr int N = 2; using type = double2; };

// sum over the workgroup of v, in a fixed order; valid in thread 0
__device__ __forceinline__ double block_sum(double v, double* lds) {
  const int tid = (int)threadIdx.x;
  lds[tid] = v;
  __syncthreads();
#pragma unroll
  for (int half = kThreads / 2; half > 0; half >>= 1) {
    if (tid < half) lds[tid] += lds[tid + half];
    __syncthreads();
  }
  return lds[0];
}

// Column j of the fit (full-width position c = sel ? sel[j] : j):
//   unit variance: ss = sumsq - sum^2 / m, d = 1 / sqrt(ss / (m - 1)), and d = 0 where ss <= 4 m eps sumsq (empty and constant
//   columns, and what rounding leaves of a constant one);   weights: d = weights[c].
// part[block] = sum over the block's columns of d^2 var, var = ss / (m - 1) in both modes.
template <typename T>
__global__ __launch_bounds__(kThreads) void factors_kernel(const double* __restrict__ sum, const double* __restrict__ sumsq, double m,
                                                           const int32_t* __restrict__ sel, const double* __restrict__ weights,
                                                           int64_t n_used, double* __restrict__ d64, T* __restrict__ dt,
                                                           T* __restrict__ w, double* __restrict__ part) {
  __shared__ double lds[kThreads];
  double acc = 0.0;
  const int64_t base = (int64_t)blockIdx.x * kPerBlock + threadIdx.x;
#pragma unroll
  for (int i = 0; i < kPerThread; ++i) {
    const int64_t j = base + (int64_t)i * kThreads;
    if (j >= n_used) break;
    const int64_t c = sel ? (int64_t)sel[j] : j;
    const double s1 = sum[c], s2 = sumsq[c];
    const double mean = s1 / m;
    const double ss = s2 - s1 * s1 / m;
    const double var = ss / (m - 1.0);
    const double d = weights ? weights[c] : ss <= 4.0 * m * kEps64 * s2 ? 0.0 : 1.0 / sqrt(var);
    d64[j] = d;
    dt[j] = (T)d;
    w[j] = (T)(d * mean);
    acc += d * d * var;
  }
  const double total = block_sum(acc, lds);
  if (threadIdx.x == 0) part[blockIdx.x] = total;
}

// *out = sum of part[0 .. count) : thread t adds part[t], part[t + 256], ... in that order, then the tree
__global__ __launch_bounds__(kThreads) void factors_total_kernel(const double* __restrict__ part, int count, double* __restrict__ out) {
  __shared__ double lds[kThreads];
  double acc = 0.0;
  for (int b = (int)threadIdx.x; b < count; b += kThreads) acc += part[b];
  const double total = block_sum(acc, lds);
  if (threadIdx.x == 0) *out = total;
}

// P[r][:] *= d[r]; vpr 16-byte vectors per row, one per lane
template <typename T>
__global__ __launch_bounds__(kThreads) void scale_rows_kernel(T* __restrict__ P, int64_t vectors, int vpr, const T* __restrict__ d) {
  using V = typename Vec16<T>::type;
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= vectors) return;
  const T f = d[i / vpr];
  V v = reinterpret_cast<V*>(P)[i];
  v.x *= f; v.y *= f;
  if constexpr (sizeof(T) == 4) { v.z *= f; v.w *= f; }
  reinterpret_cast<V*>(P)[i] = v;
}

// P[r][c] = d[r] * (sum_s parts[s][r][c] - mu[r] sv[c]): the slabs added in slab order in T, as materialize() adds them
template <typename T>
__global__ __launch_bounds__(kThreads) void finish_scaled_kernel(T* P, int64_t vectors, int vpr, const T* parts, int nsplit,
                                                                 int64_t slab_stride, const T* __restrict__ mu, const T* __restrict__ sv,
                                                                 const T* __restrict__ d) {
  using V = typename Vec16<T>::type;
  constexpr int N = Vec16<T>::N;
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= vectors) return;
  const int64_t r = i / vpr;
  const int c0 = (int)(i % vpr) * N;
  T x[N];
  auto unpack = [](const V& v, T (&o)[N]) {
    o[0] = v.x; o[1] = v.y;
    if constexpr (sizeof(T) == 4) { o[2] = v.z; o[3] = v.w; }
  };
  unpack(*reinterpret_cast<const V*>(parts + i * N), x);
  for (int sp = 1; sp < nsplit; ++sp) {
    T y[N];
    unpack(*reinterpret_cast<const V*>(parts + (int64_t)sp * slab_stride + i * N), y);
#pragma unroll
    for (int e = 0; e < N; ++e) x[e] += y[e];
  }
  if (mu) {
    const T mr = mu[r];
#pragma unroll
    for (int e = 0; e < N; ++e) x[e] -= mr * sv[c0 + e];
  }
  const T f = d[r];
  V out;
  out.x = f * x[0]; out.y = f * x[1];
  if constexpr (sizeof(T) == 4) { out.z = f * x[2]; out.w = f * x[3]; }
  *reinterpret_cast<V*>(P + i * N) = out;
}

// the vectors of a rows x ld panel and the workgroups that take one each per lane
template <typename T>
int64_t panel_vectors(const void* P, int64_t rows, int ld, unsigned* blocks) {
  constexpr int N = Vec16<T>::N;
  SAPCA_CHECK(ld >= N && ld % N == 0 && (reinterpret_cast<uintptr_t>(P) & 15) == 0, SAPCA_ERR_ARG,
              "column scaling: panel rows must be 16-byte vectors");
  const int64_t vectors = rows * (ld / N);
  const int64_t nb = (vectors + kThreads - 1) / kThreads;
  SAPCA_CHECK(nb < ((int64_t)1 << 31), SAPCA_ERR_ARG, "column scaling: panel too large");
  *blocks = (unsigned)nb;
  return vectors;
}

}  // namespace

size_t column_scale_partials(int64_t n_used) { return (size_t)((std::max<int64_t>(n_used, 1) + kPerBlock - 1) / kPerBlock); }

template <typename T>
void column_scale_factors(const double* sum, const double* sumsq, double m, const int32_t* sel, const double* weights, int64_t n_used,
                          double* d64, T* dt, T* w, double* part, double* total, hipStream_t s) {
  if (n_used <= 0) {
    SAPCA_HIP(hipMemsetAsync(total, 0, sizeof(double), s));
    return;
  }
  const size_t nb = column_scale_partials(n_used);
  SAPCA_CHECK(nb < ((size_t)1 << 31), SAPCA_ERR_ARG, "column scaling: too many columns");
  hipLaunchKernelGGL((factors_kernel<T>), dim3((unsigned)nb), dim3(kThreads), 0, s, sum, sumsq, m, sel, weights, n_used, d64, dt, w, part);
  hipLaunchKernelGGL(factors_total_kernel, dim3(1), dim3(kThreads), 0, s, part, (int)nb, total);
  SAPCA_HIP(hipGetLastError());
}

template <typename T>
void scale_panel_rows(T* P, int64_t rows, int ld, const T* d, hipStream_t s) {
  if (rows <= 0) return;
  unsigned blocks = 0;
  const int64_t vectors = panel_vectors<T>(P, rows, ld, &blocks);
  hipLaunchKernelGGL((scale_rows_kernel<T>), dim3(blocks), dim3(kThreads), 0, s, P, vectors, ld / Vec16<T>::N, d);
  SAPCA_HIP(hipGetLastError());
}

template <typename T>
void finish_scaled_panel(T* P, int64_t rows, int ld, const PanelSource<T>& src, const T* d, hipStream_t s) {
  if (rows <= 0) return;
  unsigned blocks = 0;
  const int64_t vectors = panel_vectors<T>(P, rows, ld, &blocks);
  SAPCA_CHECK(src.parts && src.nsplit >= 1 && (reinterpret_cast<uintptr_t>(src.parts) & 15) == 0 &&
                  (src.nsplit == 1 || (src.slab_stride * (int64_t)sizeof(T)) % 16 == 0),
              SAPCA_ERR_ARG, "column scaling: the sweep's slabs must be 16-byte aligned");
  hipLaunchKernelGGL((finish_scaled_kernel<T>), dim3(blocks), dim3(kThreads), 0, s, P, vectors, ld / Vec16<T>::N, src.parts, src.nsplit,
                     src.slab_stride, src.mu, src.sv, d);
  SAPCA_HIP(hipGetLastError());
}

#define SAPCA_INST(T)                                                                                                                  \
  template void column_scale_factors<T>(const double*, const double*, double, const int32_t*, const double*, int64_t, double*, T*, T*, \
                                        double*, double*, hipStream_t);                                                                \
  template void scale_panel_rows<T>(T*, int64_t, int, const T*, hipStream_t);                                                          \
  template void finish_scaled_panel<T>(T*, int64_t, int, const PanelSource<T>&, const T*, hipStream_t);
SAPCA_INST(float)
SAPCA_INST(double)
#undef SAPCA_INST

}  // namespace k
}  // namespace sapca
