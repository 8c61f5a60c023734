// The small element-wise kernels around the dense panels: the centring rank-1 update, svd_flip's signs and transposes, row
// and column scaling, zero fill, conversion from f64, padding on and off.
#include "dense_common.h"

#include <algorithm>

namespace sapca {
namespace k {

namespace {

template <typename T>
__global__ void rank1_subtract_kernel(T* __restrict__ Z, int64_t rows, int ld, const T* __restrict__ mu,
                                      const T* __restrict__ svec) {
  const int64_t total = rows * ld;
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < total; i += stride) {
    const int64_t r = i / ld;
    Z[i] -= mu[r] * svec[i - r * ld];
  }
}

// sign of the largest-|.| entry of column r of VtT (first row index on ties)
template <typename T>
__global__ void __launch_bounds__(256)
flip_sign_kernel(const T* __restrict__ VtT, int64_t n, int ld, double* __restrict__ sign) {
  __shared__ double best_a[256];
  __shared__ long long best_i[256];
  const int r = blockIdx.x;
  double ba = -1.0;
  long long bi = 0x7fffffffffffffffLL;
  for (int64_t j = threadIdx.x; j < n; j += blockDim.x) {
    const double a = fabs((double)VtT[j * ld + r]);
    if (a > ba) { ba = a; bi = j; }
  }
  best_a[threadIdx.x] = ba;
  best_i[threadIdx.x] = bi;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) {
      const double oa = best_a[threadIdx.x + off];
      const long long oi = best_i[threadIdx.x + off];
      if (oa > best_a[threadIdx.x] || (oa == best_a[threadIdx.x] && oi < best_i[threadIdx.x])) {
        best_a[threadIdx.x] = oa;
        best_i[threadIdx.x] = oi;
      }
    }
    __syncthreads();
  }
  // (best_a[0] < 0: no |v| compared greater than -1 -- a column of nan, or n = 0 -- and best_i[0] is no row: sign +1)
  if (threadIdx.x == 0) sign[r] = (n > 0 && best_a[0] >= 0.0 && (double)VtT[best_i[0] * ld + r] < 0) ? -1.0 : 1.0;
}

// The same in two coalesced stages for the usual leading dimensions (256 % ld == 0): a block scans a run of rows with a thread
// per column (the kernel above walks one column per block, 4 bytes out of every row), leaves (|v|, row) of its best per
// column; the second stage picks the overall best -- larger |v|, the first row on ties -- and reads its sign.
template <typename T>
__global__ void __launch_bounds__(256)
flip_sign_partial_kernel(const T* __restrict__ VtT, int64_t n, int ld, int64_t rows_per_block, double* __restrict__ part_a,
                         long long* __restrict__ part_i) {
  __shared__ double best_a[256];
  __shared__ long long best_i[256];
  const int c = threadIdx.x % ld, g = threadIdx.x / ld, ng = 256 / ld;
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_block, r1 = min(n, r0 + rows_per_block);
  double ba = -1.0;
  long long bi = 0x7fffffffffffffffLL;
  for (int64_t r = r0 + g; r < r1; r += ng) {
    const double a = fabs((double)VtT[r * ld + c]);
    if (a > ba) { ba = a; bi = r; }
  }
  best_a[threadIdx.x] = ba;
  best_i[threadIdx.x] = bi;
  __syncthreads();
  if (g == 0) {
    for (int y = 1; y < ng; ++y) {
      const double oa = best_a[y * ld + c];
      const long long oi = best_i[y * ld + c];
      if (oa > ba || (oa == ba && oi < bi)) { ba = oa; bi = oi; }
    }
    part_a[(int64_t)blockIdx.x * ld + c] = ba;
    part_i[(int64_t)blockIdx.x * ld + c] = bi;
  }
}

template <typename T>
__global__ void __launch_bounds__(64)
flip_sign_final_kernel(const T* __restrict__ VtT, int64_t n, int ld, int k, int nblocks, const double* __restrict__ part_a,
                       const long long* __restrict__ part_i, double* __restrict__ sign) {
  const int c = blockIdx.x;   // a wave per column
  double ba = -1.0;
  long long bi = 0x7fffffffffffffffLL;
  for (int b = threadIdx.x; b < nblocks; b += WAVE) {
    const double oa = part_a[(int64_t)b * ld + c];
    const long long oi = part_i[(int64_t)b * ld + c];
    if (oa > ba || (oa == ba && oi < bi)) { ba = oa; bi = oi; }
  }
#pragma unroll
  for (int off = WAVE / 2; off > 0; off >>= 1) {
    const double oa = __shfl_xor(ba, off);
    const long long oi = __shfl_xor(bi, off);
    if (oa > ba || (oa == ba && oi < bi)) { ba = oa; bi = oi; }   // (larger |v|; the first row on ties)
  }
  if (threadIdx.x == 0) sign[c] = (n > 0 && ba >= 0.0 && (double)VtT[bi * ld + c] < 0) ? -1.0 : 1.0;
}

template <typename T>
__global__ void flip_transpose_kernel(const T* __restrict__ VtT, int64_t n, int ld, int k,
                                      const double* __restrict__ sign, T* __restrict__ comps) {
  const int64_t total = (int64_t)k * n;
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < total; i += stride) {
    const int64_t r = i / n, j = i - r * n;
    comps[i] = (T)(sign[r] * (double)VtT[j * ld + r]);
  }
}

template <typename T>
__global__ void scaled_transpose_kernel(const T* __restrict__ comps, int64_t n, int k, const double* __restrict__ scale,
                                        T* __restrict__ W, int ld) {
  const int64_t total = n * ld;
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < total; i += stride) {
    const int64_t j = i / ld;
    const int r = (int)(i - j * ld);
    W[i] = r < k ? (T)((scale ? scale[j] : 1.0) * (double)comps[(int64_t)r * n + j]) : (T)0;
  }
}

// out[j][c] = scale[j] * P[j][c]  (scale null: a plain copy) -- the un-rotated projection panel diag(cnt) B^T of fit_transform
template <typename T>
__global__ void scale_rows_kernel(const T* __restrict__ P, int64_t rows, int ld, const double* __restrict__ scale, T* __restrict__ out) {
  const int64_t total = rows * ld;
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < total; i += stride) out[i] = scale ? (T)(scale[i / ld] * (double)P[i]) : P[i];
}

// M[i][j] *= sign[j]  (j < k): the svd_flip signs carried into the factor the deferred projection is rotated with
__global__ void scale_columns_kernel(double* __restrict__ M, int rows, int ld, int k, const double* __restrict__ sign) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows * ld) return;
  const int j = i % ld;
  if (j < k) M[i] *= sign[j];
}

template <typename T>
__global__ void fill_zero_kernel(T* p, int64_t count) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < count; i += stride) p[i] = (T)0;
}

template <typename T>
__global__ void convert_kernel(const double* __restrict__ in, T* __restrict__ out, int64_t count) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < count; i += stride) out[i] = (T)in[i];
}

template <typename T>
__global__ void repad_kernel(const T* __restrict__ in, int64_t rows, int ld_in, int ncols, T* __restrict__ out, int ld_out) {
  const int64_t total = rows * ld_out;
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < total; i += stride) {
    const int64_t r = i / ld_out;
    const int c = (int)(i - r * ld_out);
    out[i] = c < ncols ? in[r * ld_in + c] : (T)0;
  }
}

}  // namespace

template <typename T>
void rank1_subtract(T* Z, int64_t rows, int ld, const T* mu, const T* svec, hipStream_t s) {
  if (rows == 0) return;
  hipLaunchKernelGGL((rank1_subtract_kernel<T>), dim3(grid_for(rows * ld, 256)), dim3(256), 0, s, Z, rows, ld, mu, svec);
  SAPCA_HIP(hipGetLastError());
}

template <typename T>
void flip_transpose(const T* VtT, int64_t n, int ld, int k, T* components, DevBuf& scratch, hipStream_t s, const double** sign_out) {
  if (ld <= 256 && 256 % ld == 0 && n >= 4096) {
    int nblocks = (int)std::min<int64_t>(256, (n + 63) / 64);
    const int64_t rpb = (n + nblocks - 1) / nblocks;
    nblocks = (int)((n + rpb - 1) / rpb);
    double* sign = scratch.as<double>((size_t)k + 2 * (size_t)nblocks * ld + 8);
    double* part_a = sign + ((k + 7) & ~7);
    long long* part_i = reinterpret_cast<long long*>(part_a + (size_t)nblocks * ld);
    if (sign_out) *sign_out = sign;
    hipLaunchKernelGGL((flip_sign_partial_kernel<T>), dim3(nblocks), dim3(256), 0, s, VtT, n, ld, rpb, part_a, part_i);
    hipLaunchKernelGGL((flip_sign_final_kernel<T>), dim3(k), dim3(64), 0, s, VtT, n, ld, k, nblocks, part_a, part_i, sign);
    hipLaunchKernelGGL((flip_transpose_kernel<T>), dim3(grid_for((int64_t)k * n, 256)), dim3(256), 0, s, VtT, n, ld, k,
                       sign, components);
    SAPCA_HIP(hipGetLastError());
    return;
  }
  double* sign = scratch.as<double>(k);
  if (sign_out) *sign_out = sign;
  hipLaunchKernelGGL((flip_sign_kernel<T>), dim3(k), dim3(256), 0, s, VtT, n, ld, sign);
  hipLaunchKernelGGL((flip_transpose_kernel<T>), dim3(grid_for((int64_t)k * n, 256)), dim3(256), 0, s, VtT, n, ld, k,
                     sign, components);
  SAPCA_HIP(hipGetLastError());
}

template <typename T>
void scaled_transpose(const T* comps, int64_t n, int k, const double* scale, T* W, int ld, hipStream_t s) {
  if (n == 0) return;
  hipLaunchKernelGGL((scaled_transpose_kernel<T>), dim3(grid_for(n * ld, 256)), dim3(256), 0, s, comps, n, k, scale, W, ld);
  SAPCA_HIP(hipGetLastError());
}

template <typename T>
void scale_rows(const T* P, int64_t rows, int ld, const double* scale, T* out, hipStream_t s) {
  if (rows == 0) return;
  hipLaunchKernelGGL((scale_rows_kernel<T>), dim3(grid_for(rows * ld, 256)), dim3(256), 0, s, P, rows, ld, scale, out);
  SAPCA_HIP(hipGetLastError());
}

void scale_columns(double* M, int rows, int ld, int k, const double* sign, hipStream_t s) {
  hipLaunchKernelGGL(scale_columns_kernel, dim3((rows * ld + 255) / 256), dim3(256), 0, s, M, rows, ld, k, sign);
  SAPCA_HIP(hipGetLastError());
}

template <typename T>
void fill_zero(T* p, int64_t count, hipStream_t s) {
  if (count == 0) return;
  hipLaunchKernelGGL((fill_zero_kernel<T>), dim3(grid_for(count, 256)), dim3(256), 0, s, p, count);
  SAPCA_HIP(hipGetLastError());
}

template <typename T>
void convert_from_f64(const double* in, T* out, int64_t count, hipStream_t s) {
  if (count == 0) return;
  hipLaunchKernelGGL((convert_kernel<T>), dim3(grid_for(count, 256)), dim3(256), 0, s, in, out, count);
  SAPCA_HIP(hipGetLastError());
}

template <typename T>
void strip_padding(const T* in, int64_t rows, int ld, int ncols, T* out, hipStream_t s) {
  if (rows == 0) return;
  hipLaunchKernelGGL((repad_kernel<T>), dim3(grid_for(rows * ncols, 256)), dim3(256), 0, s, in, rows, ld, ncols, out, ncols);
  SAPCA_HIP(hipGetLastError());
}

template <typename T>
void add_padding(const T* in, int64_t rows, int ncols, T* out, int ld, hipStream_t s) {
  if (rows == 0) return;
  hipLaunchKernelGGL((repad_kernel<T>), dim3(grid_for(rows * ld, 256)), dim3(256), 0, s, in, rows, ncols, ncols, out, ld);
  SAPCA_HIP(hipGetLastError());
}

#define INSTANTIATE(T)                                                                            \
  template void rank1_subtract<T>(T*, int64_t, int, const T*, const T*, hipStream_t);             \
  template void flip_transpose<T>(const T*, int64_t, int, int, T*, DevBuf&, hipStream_t, const double**); \
  template void scale_rows<T>(const T*, int64_t, int, const double*, T*, hipStream_t);            \
  template void scaled_transpose<T>(const T*, int64_t, int, const double*, T*, int, hipStream_t); \
  template void fill_zero<T>(T*, int64_t, hipStream_t);                                           \
  template void convert_from_f64<T>(const double*, T*, int64_t, hipStream_t);                     \
  template void strip_padding<T>(const T*, int64_t, int, int, T*, hipStream_t);                   \
  template void add_padding<T>(const T*, int64_t, int, T*, int, hipStream_t);
INSTANTIATE(float)
INSTANTIATE(double)
template void fill_zero<int>(int*, int64_t, hipStream_t);
#undef INSTANTIATE

}  // namespace k
}  // namespace sapca
