// Spectral embedding / diffusion maps of a symmetric neighbour graph (sapca_spectral_*, sapca_graph_components_device):
// the kernels.  include/sapca.h states the algorithm; spectral.cpp stages the calls.
//   components: hooking onto the smaller root with an integer atomicMin, pointer jumping, a prefix count of the roots
//   scale:      the row sums d (NORMALIZED) or q and sum_j W_ij / q_j (DIFFMAP) by lane groups, s from them
//   operator:   y = Wt x on the scaled f64 copy Wt_ij = W_ij (s_i s_j), a short-row product: a wave holds 8, 4, 2 or 1 rows
//               (lane groups of 8, 16, 32 or 64), a row longer than its group loops, and the group meets in a butterfly --
//               no floating-point atomic, the same bytes from call to call
//   output:     the locked vectors, the sign rule and the one rounding to T; UMAP's spectral start
// No address outside the arrays is touched: a column outside [0, m) is skipped where it is read, and the matrix the solve's
// step hands to k::spmv (which does not look at its columns) carries a copy of the columns with such a one replaced.
#include <algorithm>

#include "common.h"
#include "hash_u01.h"
#include "kernels.h"

namespace sapca {
namespace k {

namespace {

inline unsigned blocks_for(int64_t n, int block = 256, int64_t cap = 1 << 20) {
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + block - 1) / block, cap));
}

// ---- components ------------------------------------------------------------------------------------------------------------
__global__ void components_init_kernel(int32_t* __restrict__ parent, int64_t m, unsigned long long* __restrict__ changed) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) *changed = 0;
  if (i < m) parent[i] = (int32_t)i;
}

// parent[x] <= x at all times (atomicMin only lowers it, from x itself), so a chain ends whatever other lanes write meanwhile
__device__ inline int32_t find_root(const int32_t* parent, int32_t x) {
  for (;;) {
    const int32_t p = __atomic_load_n(parent + x, __ATOMIC_RELAXED);
    if (p == x) return x;
    x = p;
  }
}

// one thread per stored entry of a lane group's row; GROUP lanes walk a row
__global__ void __launch_bounds__(256)
components_hook_kernel(const int64_t* __restrict__ ptr, const int32_t* __restrict__ idx, int64_t m, int32_t* __restrict__ parent,
                       unsigned long long* __restrict__ changed) {
  constexpr int GROUP = 16;
  const int lane = threadIdx.x & (GROUP - 1);
  const int64_t group = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / GROUP;
  const int64_t ngroups = (int64_t)gridDim.x * blockDim.x / GROUP;
  bool any = false;
  for (int64_t i = group; i < m; i += ngroups) {
    const int64_t e0 = ptr[i], e1 = ptr[i + 1];
    for (int64_t e = e0 + lane; e < e1; e += GROUP) {
      const int32_t j = idx[e];
      if ((uint32_t)j >= (uint32_t)m || j == (int32_t)i) continue;
      const int32_t ri = find_root(parent, (int32_t)i), rj = find_root(parent, j);
      if (ri == rj) continue;
      atomicMin(parent + max(ri, rj), min(ri, rj));
      any = true;
    }
  }
  if (any) *changed = 1;   // (every writer stores the same word)
}

__global__ void components_jump_kernel(int32_t* __restrict__ parent, int64_t m) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  const int32_t r = find_root(parent, (int32_t)i);
  // (a root keeps itself; a shortened chain only ever points at an ancestor, so concurrent finds stay on their chain)
  if (r != (int32_t)i) __atomic_store_n(parent + i, r, __ATOMIC_RELAXED);
}

__global__ void components_flag_kernel(const int32_t* __restrict__ parent, int64_t m, int64_t* __restrict__ flag) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i <= m) flag[i] = i < m && parent[i] == (int32_t)i ? 1 : 0;
}

__global__ void components_label_kernel(const int32_t* __restrict__ parent, int64_t m, const int64_t* __restrict__ scan,
                                        int32_t* __restrict__ labels) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < m) labels[i] = (int32_t)scan[parent[i]];
}

// ---- lane groups -----------------------------------------------------------------------------------------------------------
// the sum of a over the G lanes of a group, the same bits in every lane: a butterfly inside the group, an order fixed by G
template <int G>
__device__ inline double group_sum(double a) {
#pragma unroll
  for (int off = G / 2; off > 0; off >>= 1) a += __shfl_xor(a, off, G);
  return a;
}

// out[i] = sum_j W_ij / div_j (div null: ones) over the columns inside [0, m)
template <typename T, int G>
__global__ void __launch_bounds__(256)
row_sums_kernel(const int64_t* __restrict__ ptr, const int32_t* __restrict__ idx, const T* __restrict__ val, int64_t m,
                const double* __restrict__ div, double* __restrict__ out) {
  const int lane = threadIdx.x & (G - 1);
  const int64_t group = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / G;
  const int64_t ngroups = (int64_t)gridDim.x * blockDim.x / G;
  for (int64_t i = group; i < m; i += ngroups) {
    const int64_t e0 = ptr[i], e1 = ptr[i + 1];
    double a0 = 0, a1 = 0;
    int64_t e = e0 + lane;
    for (; e + G < e1; e += 2 * G) {
      const int32_t c0 = idx[e], c1 = idx[e + G];
      const double v0 = (double)val[e], v1 = (double)val[e + G];
      if ((uint32_t)c0 < (uint32_t)m) a0 += div ? v0 / div[c0] : v0;
      if ((uint32_t)c1 < (uint32_t)m) a1 += div ? v1 / div[c1] : v1;
    }
    if (e < e1) {
      const int32_t c0 = idx[e];
      const double v0 = (double)val[e];
      if ((uint32_t)c0 < (uint32_t)m) a0 += div ? v0 / div[c0] : v0;
    }
    const double a = group_sum<G>(a0 + a1);
    if (lane == 0) out[i] = a;
  }
}

__device__ inline bool finite_positive(double x) { return x > 0.0 && x <= 1.7976931348623157e308; }

__global__ void scale_finish_kernel(const double* __restrict__ d, const double* __restrict__ q, int64_t m, double* __restrict__ s_out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  double s = 0.0;
  if (q == nullptr) {
    if (finite_positive(d[i])) s = 1.0 / sqrt(d[i]);
  } else if (finite_positive(q[i]) && finite_positive(d[i])) {
    const double z = d[i] / q[i];
    if (finite_positive(z)) s = 1.0 / (q[i] * sqrt(z));
  }
  s_out[i] = finite_positive(s) ? s : 0.0;
}

// wt[e] = W_e (s_i s_j): s_i s_j is one rounded product whichever end computes it, so wt is symmetric bit for bit.
// safe_idx (nullable): a copy of the columns in which one outside [0, m) is replaced by the row's own number (its value is 0):
// a product kernel that does not look at its columns can then take the matrix.
template <typename T>
__global__ void __launch_bounds__(256)
scaled_copy_kernel(const int64_t* __restrict__ ptr, const int32_t* __restrict__ idx, const T* __restrict__ val, int64_t m,
                   const double* __restrict__ sc, double* __restrict__ wt, int32_t* __restrict__ safe_idx) {
#pragma clang fp contract(off)
  constexpr int G = 16;
  const int lane = threadIdx.x & (G - 1);
  const int64_t group = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / G;
  const int64_t ngroups = (int64_t)gridDim.x * blockDim.x / G;
  for (int64_t i = group; i < m; i += ngroups) {
    const int64_t e0 = ptr[i], e1 = ptr[i + 1];
    const double si = sc[i];
    for (int64_t e = e0 + lane; e < e1; e += G) {
      const int32_t c = idx[e];
      const bool inside = (uint32_t)c < (uint32_t)m;
      wt[e] = inside ? (double)val[e] * (si * sc[c]) : 0.0;
      if (safe_idx) safe_idx[e] = inside ? c : (int32_t)i;
    }
  }
}

// y = Wt x: the hot kernel of a Lanczos step on a neighbour graph (10 .. 40 entries per row).  A group of G lanes per row,
// 64 / G rows per wave; two independent (value, column, gather) chains per lane; the group's butterfly fixes the order.
template <int G>
__global__ void __launch_bounds__(256)
group_spmv_kernel(const int64_t* __restrict__ ptr, const int32_t* __restrict__ idx, const double* __restrict__ wt, int64_t m,
                  const double* __restrict__ x, double* __restrict__ y) {
  const int lane = threadIdx.x & (G - 1);
  const int64_t group = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / G;
  const int64_t ngroups = (int64_t)gridDim.x * blockDim.x / G;
  for (int64_t i = group; i < m; i += ngroups) {
    const int64_t e0 = ptr[i], e1 = ptr[i + 1];
    double a0 = 0, a1 = 0;
    int64_t e = e0 + lane;
    for (; e + G < e1; e += 2 * G) {
      const int32_t c0 = __builtin_nontemporal_load(idx + e), c1 = __builtin_nontemporal_load(idx + e + G);
      const double v0 = __builtin_nontemporal_load(wt + e), v1 = __builtin_nontemporal_load(wt + e + G);
      if ((uint32_t)c0 < (uint32_t)m) a0 = fma(v0, x[c0], a0);
      if ((uint32_t)c1 < (uint32_t)m) a1 = fma(v1, x[c1], a1);
    }
    if (e < e1) {
      const int32_t c0 = __builtin_nontemporal_load(idx + e);
      const double v0 = __builtin_nontemporal_load(wt + e);
      if ((uint32_t)c0 < (uint32_t)m) a0 = fma(v0, x[c0], a0);
    }
    const double a = group_sum<G>(a0 + a1);
    if (lane == 0) y[i] = a;
  }
}

// ---- output ----------------------------------------------------------------------------------------------------------------
__global__ void locked_kernel(const int32_t* __restrict__ labels, const int32_t* __restrict__ lock_of, const double* __restrict__ inv_norm,
                              const double* __restrict__ t, int64_t m, int nlock, double* __restrict__ U) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  const int l = lock_of[labels[i]];
  const double ti = t[i];
  for (int p = 0; p < nlock; ++p) U[(int64_t)p * m + i] = (p == l && ti > 0.0) ? ti * inv_norm[p] : 0.0;
}

// signs[l] = -1 where the entry of largest magnitude (lowest index on a tie) of vector l is negative, else +1: one workgroup
// per vector; a thread keeps the first maximum of its strided elements, the threads meet on (magnitude, index)
__global__ void __launch_bounds__(256)
sign_kernel(const double* __restrict__ src, int64_t lds_row, int64_t lds_col, int64_t m, int* __restrict__ signs) {
  __shared__ double bmag[256];
  __shared__ int64_t bidx[256];
  const double* v = src + (int64_t)blockIdx.x * lds_row;
  double mag = -1.0;
  int64_t at = m;
  for (int64_t i = threadIdx.x; i < m; i += blockDim.x) {
    const double a = fabs(v[i * lds_col]);
    if (a > mag) { mag = a; at = i; }   // (ascending i: the first maximum of this thread)
  }
  bmag[threadIdx.x] = mag;
  bidx[threadIdx.x] = at;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) {
      const double om = bmag[threadIdx.x + off];
      const int64_t oi = bidx[threadIdx.x + off];
      if (om > bmag[threadIdx.x] || (om == bmag[threadIdx.x] && oi < bidx[threadIdx.x])) {
        bmag[threadIdx.x] = om;
        bidx[threadIdx.x] = oi;
      }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) signs[blockIdx.x] = (bidx[0] < m && v[bidx[0] * lds_col] < 0.0) ? -1 : 1;
}

template <typename T>
__global__ void __launch_bounds__(256)
store_kernel(const double* __restrict__ src, int64_t lds_row, int64_t lds_col, int64_t m, int nvec, const int* __restrict__ signs,
             T* __restrict__ out, int64_t ldo, int col0) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int l = blockIdx.y;
  if (i >= m || l >= nvec) return;
  const double v = src[(int64_t)l * lds_row + i * lds_col];
  out[i * ldo + col0 + l] = (T)(signs && signs[l] < 0 ? -v : v);
}

// non-negative doubles order like their bit patterns: an integer atomic takes the maximum, whatever the order
template <typename T>
__global__ void __launch_bounds__(256)
start_max_kernel(const T* __restrict__ E, int64_t ld, int64_t m, int od, unsigned long long* __restrict__ mx) {
  double best = 0.0;
  const int64_t n = m * od;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x) {
    best = fmax(best, fabs((double)E[(t / od) * ld + 1 + t % od]));
  }
  if (best != 0.0) atomicMax(mx, (unsigned long long)__double_as_longlong(best));
}

template <typename T>
__global__ void __launch_bounds__(256)
start_kernel(const T* __restrict__ E, int64_t ld, int64_t m, int od, uint32_t seed, const unsigned long long* __restrict__ mx,
             T* __restrict__ y) {
#pragma clang fp contract(off)
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= m * od) return;
  const double top = __longlong_as_double((long long)*mx);
  const double e = (double)E[(t / od) * ld + 1 + t % od];
  const double noise = 1e-4 * (2.0 * hash_u01(seed, 51, (uint64_t)t) - 1.0);
  const double lead = top > 0.0 ? (10.0 * e) / top : 0.0;
  y[t] = (T)(lead + noise);
}

}  // namespace

void components_init(int32_t* parent, int64_t m, unsigned long long* changed, hipStream_t s) {
  hipLaunchKernelGGL(components_init_kernel, dim3(blocks_for(m)), dim3(256), 0, s, parent, m, changed);
  SAPCA_HIP(hipGetLastError());
}

void components_round(const int64_t* ptr, const int32_t* idx, int64_t m, int32_t* parent, unsigned long long* changed, hipStream_t s) {
  if (m == 0) return;
  hipLaunchKernelGGL(components_hook_kernel, dim3(blocks_for(m * 16, 256, 8192)), dim3(256), 0, s, ptr, idx, m, parent, changed);
  hipLaunchKernelGGL(components_jump_kernel, dim3(blocks_for(m)), dim3(256), 0, s, parent, m);
  SAPCA_HIP(hipGetLastError());
}

void components_flag(const int32_t* parent, int64_t m, int64_t* flag, hipStream_t s) {
  hipLaunchKernelGGL(components_flag_kernel, dim3(blocks_for(m + 1)), dim3(256), 0, s, parent, m, flag);
  SAPCA_HIP(hipGetLastError());
}

void components_label(const int32_t* parent, int64_t m, const int64_t* scan, int32_t* labels, hipStream_t s) {
  if (m == 0) return;
  hipLaunchKernelGGL(components_label_kernel, dim3(blocks_for(m)), dim3(256), 0, s, parent, m, scan, labels);
  SAPCA_HIP(hipGetLastError());
}

int spectral_group(int64_t m, int64_t nnz, int forced) {
  if (forced == 8 || forced == 16 || forced == 32 || forced == 64) return forced;
  if (m <= 0) return 8;
  for (int g = 8; g < 64; g *= 2)
    if (nnz <= (int64_t)g * m) return g;   // (mean row length <= g)
  return 64;
}

namespace {
// as many groups as rows, at most 8192 workgroups (a group then walks several rows)
inline unsigned group_grid(int64_t m, int g) { return blocks_for(m * g, 256, 8192); }
}  // namespace

template <typename T>
void spectral_row_sums(const CsrView<T>& W, const double* div, int g, double* out, hipStream_t s) {
  if (W.rows == 0) return;
  const dim3 grid(group_grid(W.rows, g)), block(256);
  switch (g) {
    case 8: hipLaunchKernelGGL((row_sums_kernel<T, 8>), grid, block, 0, s, W.ptr, W.idx, W.val, W.rows, div, out); break;
    case 16: hipLaunchKernelGGL((row_sums_kernel<T, 16>), grid, block, 0, s, W.ptr, W.idx, W.val, W.rows, div, out); break;
    case 32: hipLaunchKernelGGL((row_sums_kernel<T, 32>), grid, block, 0, s, W.ptr, W.idx, W.val, W.rows, div, out); break;
    default: hipLaunchKernelGGL((row_sums_kernel<T, 64>), grid, block, 0, s, W.ptr, W.idx, W.val, W.rows, div, out); break;
  }
  SAPCA_HIP(hipGetLastError());
}
template void spectral_row_sums<float>(const CsrView<float>&, const double*, int, double*, hipStream_t);
template void spectral_row_sums<double>(const CsrView<double>&, const double*, int, double*, hipStream_t);

void spectral_scale_finish(const double* d, const double* q, int64_t m, double* s_out, hipStream_t s) {
  if (m == 0) return;
  hipLaunchKernelGGL(scale_finish_kernel, dim3(blocks_for(m)), dim3(256), 0, s, d, q, m, s_out);
  SAPCA_HIP(hipGetLastError());
}

template <typename T>
void spectral_scaled_copy(const CsrView<T>& W, const double* sc, double* wt, int32_t* safe_idx, hipStream_t s) {
  if (W.rows == 0 || W.nnz == 0) return;
  hipLaunchKernelGGL((scaled_copy_kernel<T>), dim3(group_grid(W.rows, 16)), dim3(256), 0, s, W.ptr, W.idx, W.val, W.rows, sc, wt,
                     safe_idx);
  SAPCA_HIP(hipGetLastError());
}
template void spectral_scaled_copy<float>(const CsrView<float>&, const double*, double*, int32_t*, hipStream_t);
template void spectral_scaled_copy<double>(const CsrView<double>&, const double*, double*, int32_t*, hipStream_t);

void spectral_spmv(const CsrView<double>& Wt, const double* x, double* y, int g, hipStream_t s) {
  if (Wt.rows == 0) return;
  const dim3 grid(group_grid(Wt.rows, g)), block(256);
  switch (g) {
    case 8: hipLaunchKernelGGL((group_spmv_kernel<8>), grid, block, 0, s, Wt.ptr, Wt.idx, Wt.val, Wt.rows, x, y); break;
    case 16: hipLaunchKernelGGL((group_spmv_kernel<16>), grid, block, 0, s, Wt.ptr, Wt.idx, Wt.val, Wt.rows, x, y); break;
    case 32: hipLaunchKernelGGL((group_spmv_kernel<32>), grid, block, 0, s, Wt.ptr, Wt.idx, Wt.val, Wt.rows, x, y); break;
    default: hipLaunchKernelGGL((group_spmv_kernel<64>), grid, block, 0, s, Wt.ptr, Wt.idx, Wt.val, Wt.rows, x, y); break;
  }
  SAPCA_HIP(hipGetLastError());
}

void spectral_locked(const int32_t* labels, const int32_t* lock_of, const double* inv_norm, const double* t, int64_t m, int nlock,
                     double* U, hipStream_t s) {
  if (m == 0 || nlock <= 0) return;
  hipLaunchKernelGGL(locked_kernel, dim3(blocks_for(m)), dim3(256), 0, s, labels, lock_of, inv_norm, t, m, nlock, U);
  SAPCA_HIP(hipGetLastError());
}

template <typename T>
void spectral_store(const double* src, int64_t lds_row, int64_t lds_col, int64_t m, int nvec, bool fix_sign, int* signs, T* out,
                    int64_t ldo, int col0, hipStream_t s) {
  if (m == 0 || nvec <= 0) return;
  if (fix_sign) hipLaunchKernelGGL(sign_kernel, dim3(nvec), dim3(256), 0, s, src, lds_row, lds_col, m, signs);
  hipLaunchKernelGGL((store_kernel<T>), dim3(blocks_for(m), nvec), dim3(256), 0, s, src, lds_row, lds_col, m, nvec,
                     fix_sign ? signs : (const int*)nullptr, out, ldo, col0);
  SAPCA_HIP(hipGetLastError());
}
template void spectral_store<float>(const double*, int64_t, int64_t, int64_t, int, bool, int*, float*, int64_t, int, hipStream_t);
template void spectral_store<double>(const double*, int64_t, int64_t, int64_t, int, bool, int*, double*, int64_t, int, hipStream_t);

template <typename T>
void umap_spectral_init(const T* E, int64_t ld, int64_t m, int od, uint32_t seed, unsigned long long* mx, T* y, hipStream_t s) {
  if (m == 0) return;
  SAPCA_HIP(hipMemsetAsync(mx, 0, sizeof(unsigned long long), s));
  hipLaunchKernelGGL((start_max_kernel<T>), dim3(blocks_for(m * od, 256, 1024)), dim3(256), 0, s, E, ld, m, od, mx);
  hipLaunchKernelGGL((start_kernel<T>), dim3(blocks_for(m * od)), dim3(256), 0, s, E, ld, m, od, seed, mx, y);
  SAPCA_HIP(hipGetLastError());
}
template void umap_spectral_init<float>(const float*, int64_t, int64_t, int, uint32_t, unsigned long long*, float*, hipStream_t);
template void umap_spectral_init<double>(const double*, int64_t, int64_t, int, uint32_t, unsigned long long*, double*, hipStream_t);

}  // namespace k
}  // namespace sapca
