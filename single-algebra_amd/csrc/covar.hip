// Implicit row-side correction of a panel by an orthonormal basis Q of per-row covariates (sapca_set_covariates):
//   panel_qt_y   S = Q^T Y            (kCovarCols x ld, f64)
//   panel_sub_qs Y[i][:] -= sum_j Q[i][j] S[j][:]
// Y is a rows x ld panel of T, Q a rows x kCovarCols panel of T whose columns beyond the basis' rank are zero, so both kernels
// always work on all kCovarCols columns and need no rank.  Both are bound by the panel's bytes (16 ld FMAs per row are
// nothing): a lane owns one 16-byte vector of a row's columns and walks the rows of its workgroup's share, 16-byte loads,
// f64 accumulation.  The sums over rows are gathered without floating-point atomics: per workgroup in LDS in row-slot
// order, then over the workgroups in block order by a second kernel -- the same bits from run to run.
// For T = f64 a plain f64 sum over the rows would be the least accurate step of a fit -- its error grows with the row count
// and is relative to sum |q||y|, not to |S|, exactly where the component along Q is large -- so the f64 panels are summed
// in double-double (error-free product and sum, Ogita / Rump / Oishi's Dot2): S is the exact sum rounded once, as it is for
// f32 panels summed in f64.  The arithmetic grows tenfold on that path and stays below its memory time.
#include <algorithm>

#include "kernels.h"

namespace sapca {
namespace k {

namespace {

constexpr int kQ = kCovarCols;
constexpr int kThreads = 256;
constexpr int kJBlock = 4;   // basis columns whose partial sums pass through LDS together

template <typename T> struct Vec16;
template <> struct Vec16<float> { static constexpr int N = 4; using type = float4; };
template <> struct Vec16<double> { static constexpr int N = 2; using type = double2; };

template <typename T>
__device__ __forceinline__ void load16(const T* p, double (&out)[Vec16<T>::N]) {
  const typename Vec16<T>::type v = *reinterpret_cast<const typename Vec16<T>::type*>(p);
  if constexpr (sizeof(T) == 4) { out[0] = v.x; out[1] = v.y; out[2] = v.z; out[3] = v.w; }
  else { out[0] = v.x; out[1] = v.y; }
}

// hi + lo += a * b without losing the product's or the sum's rounding error (hi + lo: an unevaluated double-double)
__device__ __forceinline__ void dd_fma(double& hi, double& lo, double a, double b) {
#pragma clang fp contract(off)
  const double p = a * b;
  const double pe = __builtin_fma(a, b, -p);
  const double sum = hi + p;
  const double t = sum - hi;
  const double se = (hi - (sum - t)) + (p - t);
  hi = sum;
  lo += pe + se;
}
// (hi, lo) += (xh, xl)
__device__ __forceinline__ void dd_add(double& hi, double& lo, double xh, double xl) {
#pragma clang fp contract(off)
  const double sum = hi + xh;
  const double t = sum - hi;
  const double se = (hi - (sum - t)) + (xh - t);
  hi = sum;
  lo += xl + se;
}

// the kQ entries of row i of Q as doubles
template <typename T>
__device__ __forceinline__ void load_q_row(const T* __restrict__ Q, int64_t i, double (&q)[kQ]) {
  constexpr int VEC = Vec16<T>::N;
#pragma unroll
  for (int j = 0; j < kQ; j += VEC) {
    double t[VEC];
    load16<T>(Q + i * kQ + j, t);
#pragma unroll
    for (int e = 0; e < VEC; ++e) q[j + e] = t[e];
  }
}

// The geometry both kernels share: column block `blockIdx.y` of cb columns starting at col0 = blockIdx.y * cb; vpr = cb / VEC
// lanes per row, rpi = kThreads / vpr row slots per pass; lane (slot, v) owns columns col0 + v * VEC .. + VEC of rows
// row_lo + slot, + rpi, ...; lanes with slot >= rpi idle (vpr need not divide kThreads: ld = 48, 80, ...).
//
// part[(blockIdx.x * kQ + j) * ld + c] = sum over the workgroup's rows of Q[i][j] * Y[i][c]
template <typename T>
__global__ __launch_bounds__(kThreads) void qt_y_partial_kernel(const T* __restrict__ Y, const T* __restrict__ Q, int64_t rows,
                                                                 int ld, int cb, int64_t rows_per_block, double* __restrict__ part,
                                                                 double* __restrict__ part_lo) {
  constexpr int VEC = Vec16<T>::N;
  constexpr bool kExact = sizeof(T) == 8;   // double-double sums (part_lo: their low words); f32 panels: plain f64, part_lo unused
  extern __shared__ double lds[];   // [kJBlock][rpi][cb], and once more for the low words
  const int vpr = cb / VEC, rpi = kThreads / vpr;
  const int tid = (int)threadIdx.x, v = tid % vpr, slot = tid / vpr;
  const int col0 = (int)blockIdx.y * cb;
  const int64_t row_lo = (int64_t)blockIdx.x * rows_per_block;
  const int64_t row_hi = row_lo + rows_per_block < rows ? row_lo + rows_per_block : rows;
  double acc[kQ][VEC], low[kExact ? kQ : 1][VEC];
#pragma unroll
  for (int j = 0; j < kQ; ++j)
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      acc[j][e] = 0.0;
      if constexpr (kExact) low[j][e] = 0.0;
    }
  double* const lds_lo = lds + (size_t)kJBlock * rpi * cb;
  if (slot < rpi) {
    for (int64_t i = row_lo + slot; i < row_hi; i += rpi) {
      double y[VEC], q[kQ];
      load16<T>(Y + i * ld + col0 + v * VEC, y);
      load_q_row<T>(Q, i, q);
#pragma unroll
      for (int j = 0; j < kQ; ++j)
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
          if constexpr (kExact) dd_fma(acc[j][e], low[j][e], q[j], y[e]);
          else acc[j][e] = fma(q[j], y[e], acc[j][e]);
        }
    }
  }
  // the row slots' sums, kJBlock basis columns at a time, added in slot order
#pragma unroll
  for (int j0 = 0; j0 < kQ; j0 += kJBlock) {
    if (slot < rpi) {
#pragma unroll
      for (int jj = 0; jj < kJBlock; ++jj)
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
          lds[((size_t)jj * rpi + slot) * cb + v * VEC + e] = acc[j0 + jj][e];
          if constexpr (kExact) lds_lo[((size_t)jj * rpi + slot) * cb + v * VEC + e] = low[j0 + jj][e];
        }
    }
    __syncthreads();
    for (int o = tid; o < kJBlock * cb; o += kThreads) {
      const int jj = o / cb, c = o % cb;
      double sum = 0.0, sum_lo = 0.0;
      for (int sl = 0; sl < rpi; ++sl) {
        const size_t at = ((size_t)jj * rpi + sl) * cb + c;
        if constexpr (kExact) dd_add(sum, sum_lo, lds[at], lds_lo[at]);
        else sum += lds[at];
      }
      const size_t to = ((size_t)blockIdx.x * kQ + j0 + jj) * ld + col0 + c;
      part[to] = sum;
      if constexpr (kExact) part_lo[to] = sum_lo;
    }
    __syncthreads();
  }
}

// S[o] = sum over the workgroups, in block order, of part[b][o]   (o < kQ * ld; part_lo: the low words of double-double partials, or null)
__global__ __launch_bounds__(kThreads) void qt_y_final_kernel(const double* __restrict__ part, const double* __restrict__ part_lo, int nblocks,
                                                              int count, double* __restrict__ S) {
  const int o = (int)(blockIdx.x * kThreads + threadIdx.x);
  if (o >= count) return;
  double sum = 0.0, sum_lo = 0.0;
  if (part_lo) {
    for (int b = 0; b < nblocks; ++b) dd_add(sum, sum_lo, part[(size_t)b * count + o], part_lo[(size_t)b * count + o]);
  } else {
    for (int b = 0; b < nblocks; ++b) sum += part[(size_t)b * count + o];
  }
  S[o] = sum + sum_lo;
}

// Y[i][c] = T(Y[i][c] - sum_j Q[i][j] S[j * lds_ + c]) with the lane's slice of S in registers
template <typename T>
__global__ __launch_bounds__(kThreads) void sub_qs_kernel(T* __restrict__ Y, const T* __restrict__ Q, int64_t rows, int ld, int cb,
                                                           int64_t rows_per_block, const double* __restrict__ S, int lds_) {
  constexpr int VEC = Vec16<T>::N;
  const int vpr = cb / VEC, rpi = kThreads / vpr;
  const int tid = (int)threadIdx.x, v = tid % vpr, slot = tid / vpr;
  if (slot >= rpi) return;
  const int col = (int)blockIdx.y * cb + v * VEC;
  const int64_t row_lo = (int64_t)blockIdx.x * rows_per_block;
  const int64_t row_hi = row_lo + rows_per_block < rows ? row_lo + rows_per_block : rows;
  double s[kQ][VEC];
#pragma unroll
  for (int j = 0; j < kQ; ++j)
#pragma unroll
    for (int e = 0; e < VEC; ++e) s[j][e] = S[(size_t)j * lds_ + col + e];
  for (int64_t i = row_lo + slot; i < row_hi; i += rpi) {
    double y[VEC], q[kQ];
    T* dst = Y + i * ld + col;
    load16<T>(dst, y);
    load_q_row<T>(Q, i, q);
#pragma unroll
    for (int j = 0; j < kQ; ++j)
#pragma unroll
      for (int e = 0; e < VEC; ++e) y[e] = fma(-q[j], s[j][e], y[e]);
    typename Vec16<T>::type out;
    if constexpr (sizeof(T) == 4) { out.x = (float)y[0]; out.y = (float)y[1]; out.z = (float)y[2]; out.w = (float)y[3]; }
    else { out.x = y[0]; out.y = y[1]; }
    *reinterpret_cast<typename Vec16<T>::type*>(dst) = out;
  }
}

// the same update of a panel whose rows are not 16-byte vectors (the m x k projection, row stride k): one element per lane
template <typename T>
__global__ __launch_bounds__(kThreads) void sub_qs_scalar_kernel(T* __restrict__ Y, const T* __restrict__ Q, int64_t rows, int ld, int ncols,
                                                                  const double* __restrict__ S, int lds_) {
  const int64_t o = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (o >= rows * ncols) return;
  const int64_t i = o / ncols;
  const int c = (int)(o % ncols);
  double y = (double)Y[i * ld + c];
#pragma unroll
  for (int j = 0; j < kQ; ++j) y = fma(-(double)Q[i * kQ + j], S[(size_t)j * lds_ + c], y);
  Y[i * ld + c] = (T)y;
}

// column block and workgroup grid of a rows x ld panel (ld a multiple of 16 up to 128, or of 64 up to kMaxPanelWidth)
struct PanelGrid {
  int cb, ncb, nbx;
  int64_t rows_per_block;
};
template <typename T>
PanelGrid panel_grid(int64_t rows, int ld) {
  SAPCA_CHECK(ld >= 16 && ld <= kMaxPanelWidth && (ld <= 128 ? ld % 16 == 0 : ld % 64 == 0), SAPCA_ERR_ARG,
              "covariate projection: panel width must be a multiple of 16 up to 128, or of 64 up to 1024");
  PanelGrid g;
  g.cb = ld <= 128 ? ld : 64;
  g.ncb = ld / g.cb;
  const int rpi = kThreads / (g.cb / Vec16<T>::N);
  // a workgroup per 8 passes of its row slots, at most 512 of them (two per CU): the second stage adds that many partials
  const int64_t want = (rows + (int64_t)rpi * 8 - 1) / ((int64_t)rpi * 8);
  g.nbx = (int)std::min<int64_t>(512, std::max<int64_t>(want, 1));
  g.rows_per_block = (rows + g.nbx - 1) / g.nbx;
  g.nbx = (int)std::max<int64_t>((rows + g.rows_per_block - 1) / std::max<int64_t>(g.rows_per_block, 1), 1);
  return g;
}

}  // namespace

template <typename T>
void panel_qt_y(const T* Y, const T* Q, int64_t rows, int ld, double* S, DevBuf& scratch, hipStream_t s) {
  const PanelGrid g = panel_grid<T>(rows, ld);
  SAPCA_CHECK(((reinterpret_cast<uintptr_t>(Y) | reinterpret_cast<uintptr_t>(Q)) & 15) == 0, SAPCA_ERR_ARG,
              "covariate projection: panels must be 16-byte aligned");
  if (rows <= 0) {
    SAPCA_HIP(hipMemsetAsync(S, 0, (size_t)kQ * ld * sizeof(double), s));
    return;
  }
  constexpr bool exact = sizeof(T) == 8;
  const size_t part_len = (size_t)g.nbx * kQ * ld;
  double* part = scratch.as<double>(part_len * (exact ? 2 : 1));
  double* part_lo = exact ? part + part_len : nullptr;
  const int rpi = kThreads / (g.cb / Vec16<T>::N);
  const size_t lds = (size_t)kJBlock * rpi * g.cb * sizeof(double) * (exact ? 2 : 1);   // 32 KiB at most (rpi * cb <= 256 * VEC)
  hipLaunchKernelGGL((qt_y_partial_kernel<T>), dim3((unsigned)g.nbx, (unsigned)g.ncb), dim3(kThreads), lds, s, Y, Q, rows, ld, g.cb,
                     g.rows_per_block, part, part_lo);
  const int count = kQ * ld;
  hipLaunchKernelGGL(qt_y_final_kernel, dim3((unsigned)((count + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, part, part_lo, g.nbx,
                     count, S);
  SAPCA_HIP(hipGetLastError());
}

template <typename T>
void panel_sub_qs(T* Y, const T* Q, int64_t rows, int ld, int ncols, const double* S, int lds, hipStream_t s) {
  SAPCA_CHECK(ncols >= 1 && ncols <= ld && ncols <= lds, SAPCA_ERR_ARG, "covariate projection: ncols exceeds a leading dimension");
  if (rows <= 0) return;
  const bool vectors = ncols == ld && ld <= kMaxPanelWidth && (ld <= 128 ? ld % 16 == 0 : ld % 64 == 0) &&
                       ((reinterpret_cast<uintptr_t>(Y) | reinterpret_cast<uintptr_t>(Q)) & 15) == 0;
  if (vectors) {
    const PanelGrid g = panel_grid<T>(rows, ld);
    hipLaunchKernelGGL((sub_qs_kernel<T>), dim3((unsigned)g.nbx, (unsigned)g.ncb), dim3(kThreads), 0, s, Y, Q, rows, ld, g.cb,
                       g.rows_per_block, S, lds);
  } else {
    SAPCA_CHECK((reinterpret_cast<uintptr_t>(Q) & 15) == 0, SAPCA_ERR_ARG, "covariate projection: the basis must be 16-byte aligned");
    const int64_t total = rows * ncols;
    SAPCA_CHECK((total + kThreads - 1) / kThreads < ((int64_t)1 << 31), SAPCA_ERR_ARG, "covariate projection: panel too large");
    hipLaunchKernelGGL((sub_qs_scalar_kernel<T>), dim3((unsigned)((total + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, Y, Q, rows,
                       ld, ncols, S, lds);
  }
  SAPCA_HIP(hipGetLastError());
}

#define SAPCA_INST(T)                                                                              \
  template void panel_qt_y<T>(const T*, const T*, int64_t, int, double*, DevBuf&, hipStream_t);   \
  template void panel_sub_qs<T>(T*, const T*, int64_t, int, int, const double*, int, hipStream_t);
SAPCA_INST(float)
SAPCA_INST(double)
#undef SAPCA_INST

}  // namespace k
}  // namespace sapca
