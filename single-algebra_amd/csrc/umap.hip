// UMAP on device-resident rows (sapca_umap_*): umap-learn's fuzzy simplicial set and a synchronous, deterministic restatement
// of its optimize_layout_euclidean; include/sapca.h states the algorithm in full.  Stages:
//   row sums     one wave per row: the sum of a row's valid distances (the floor of sigma needs the panel's total first)
//   smooth       one wave per row, K <= 128 distances in registers (two per lane): rho_i, the 64-step search for sigma_i on
//                wave sums in one order, the floor, and the memberships a_ik through the correctly rounded exp of exp_rn.h
//   union        tsne.hip's count / emit and canon.hip's row sort put both directions of a pair side by side; the fill here
//                combines them as (a + b) - a b in f64 (symmetric in its terms) and rounds once to T
//   schedule     w_max by an integer maximum over the bit patterns, then next_e and nextn_e per stored entry
//   epoch        sixteen lanes per vertex walk its entries: attraction towards the entry's column and the repulsion of the
//                samples that fall due, from the previous epoch's Y only; the lanes' f64 sums meet in a fixed butterfly and
//                y_i is rounded once into the other buffer.  A gather-latency kernel: Y stays in L2 / MALL, the schedule is
//                streamed once.
// No floating-point atomics; nothing is sized by the device, so no summation order depends on it.
#include "exp_rn.h"
#include "hash_u01.h"
#include "kernels.h"

// products and sums as written: the restatement the tests hold this to rounds every product (the schedule's
// nextn + q * epsn decides in which epoch a sample falls due, and (a + b) - a b must round a b)
#pragma clang fp contract(off)

namespace sapca {
namespace k {

namespace {

constexpr int kWave = 64;
constexpr int kSub = 16;   // lanes per vertex in the epoch kernel

__device__ inline double wave_sum(double v) {   // the same value in every lane, one order
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
  return v;
}
__device__ inline double wave_min(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, kWave));
  return v;
}

// the two slots of this lane: distances (0 where the slot does not count) and whether the slot counts
template <typename T>
__device__ inline void load_slots(const int32_t* __restrict__ idx, const T* __restrict__ dist, int64_t row, int64_t m, int K, int lane,
                                  double d[2], bool ok[2]) {
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int slot = lane + t * kWave;
    ok[t] = false;
    d[t] = 0.0;
    if (slot < K) {
      const int32_t j = idx[row * K + slot];
      if (j >= 0 && (int64_t)j < m) {
        d[t] = (double)dist[row * K + slot];
        ok[t] = true;
      }
    }
  }
}

// ---- stage 2 ------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(256) umap_row_sums_kernel(const int32_t* __restrict__ idx, const T* __restrict__ dist, int64_t m, int K,
                                                            double* __restrict__ rowsum) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t row = (int64_t)blockIdx.x * (blockDim.x / kWave) + (threadIdx.x / kWave);
  if (row >= m) return;   // (whole waves leave together)
  double d[2];
  bool ok[2];
  load_slots<T>(idx, dist, row, m, K, lane, d, ok);
  const double s = wave_sum(d[0] + d[1]);
  if (lane == 0) rowsum[row] = s;
}

// a[row * K + slot] = the membership of the slot (0 where it does not count); sigma / rho may be null
template <typename T>
__global__ void __launch_bounds__(256) umap_smooth_kernel(const int32_t* __restrict__ idx, const T* __restrict__ dist, int64_t m, int K,
                                                          double n_neighbors, double target, const double* __restrict__ total,
                                                          double* __restrict__ a_out, double* __restrict__ sigma_out,
                                                          double* __restrict__ rho_out) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t row = (int64_t)blockIdx.x * (blockDim.x / kWave) + (threadIdx.x / kWave);
  if (row >= m) return;
  double d[2];
  bool ok[2];
  load_slots<T>(idx, dist, row, m, K, lane, d, ok);
  double r = INFINITY;
#pragma unroll
  for (int t = 0; t < 2; ++t)
    if (ok[t] && d[t] > 0.0) r = fmin(r, d[t]);
  r = wave_min(r);
  const double rho = r == INFINITY ? 0.0 : r;
  const double rowsum = wave_sum(d[0] + d[1]);
  const double x0 = d[0] - rho, x1 = d[1] - rho;
  double lo = 0.0, hi = INFINITY, mid = 1.0;
  for (int it = 0; it < 64; ++it) {
    const double p0 = ok[0] ? (x0 > 0.0 ? exp(-x0 / mid) : 1.0) : 0.0;
    const double p1 = ok[1] ? (x1 > 0.0 ? exp(-x1 / mid) : 1.0) : 0.0;
    const double psum = wave_sum(p0 + p1);
    if (fabs(psum - target) < 1e-5) break;
    if (psum > target) {
      hi = mid;
      mid = (lo + hi) / 2.0;
    } else {
      lo = mid;
      mid = (hi == INFINITY) ? mid * 2.0 : (lo + hi) / 2.0;
    }
  }
  const double floor_at = rho > 0.0 ? 1e-3 * (rowsum / n_neighbors) : 1e-3 * (total[0] / ((double)m * n_neighbors));
  const double sigma = fmax(mid, floor_at);
  const double a0 = ok[0] ? (x0 > 0.0 ? exp_rn(-x0 / sigma) : 1.0) : 0.0;
  const double a1 = ok[1] ? (x1 > 0.0 ? exp_rn(-x1 / sigma) : 1.0) : 0.0;
  if (lane < K) a_out[row * K + lane] = a0;
  if (lane + kWave < K) a_out[row * K + lane + kWave] = a1;
  if (lane == 0) {
    if (sigma_out) sigma_out[row] = sigma;
    if (rho_out) rho_out[row] = rho;
  }
}

// ---- stage 3: the fill of the union -----------------------------------------------------------------------------------------
__device__ inline double fuzzy_or(double a, double b) { return (a + b) - a * b; }

// (idx, val at the offsets ptr: every row sorted by column) -> (out_idx, out_val at new_ptr): one entry per run of equal
// columns, the run folded by fuzzy_or in f64 (a pair: symmetric in its two terms) and rounded once to T.  new_ptr may be ptr.
template <typename T>
__global__ void __launch_bounds__(256) umap_union_kernel(const int64_t* __restrict__ ptr, const int32_t* __restrict__ idx,
                                                         const double* __restrict__ val, int64_t m, const int64_t* __restrict__ new_ptr,
                                                         int32_t* __restrict__ out_idx, T* __restrict__ out_val) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t r = wave; r < m; r += nwaves) {
    const int64_t e0 = ptr[r], e1 = ptr[r + 1];
    int64_t out = new_ptr[r];
    for (int64_t base = e0; base < e1; base += kWave) {   // (uniform trip count: the ballot sees whole waves)
      const int64_t e = base + lane;
      const int32_t c = e < e1 ? idx[e] : 0;
      const bool head = e < e1 && (e == e0 || idx[e - 1] != c);
      const unsigned long long mask = __ballot(head);
      if (head) {
        double g = val[e];
        for (int64_t j = e + 1; j < e1 && idx[j] == c; ++j) g = fuzzy_or(g, val[j]);
        const int64_t pos = out + __popcll(mask & ((1ull << lane) - 1ull));
        out_idx[pos] = c;
        out_val[pos] = (T)g;
      }
      out += __popcll(mask);
    }
  }
}

// ---- stage 5: the schedule ----------------------------------------------------------------------------------------------------
// the largest positive value by an integer maximum over bit patterns (positive doubles order like their bits): no order
template <typename T>
__global__ void __launch_bounds__(256) umap_wmax_kernel(const T* __restrict__ val, int64_t nnz, unsigned long long* __restrict__ bits) {
  int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  double best = 0.0;
  for (; e < nnz; e += stride) {
    const double w = (double)val[e];
    if (w > best) best = w;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) best = fmax(best, __shfl_xor(best, o, kWave));
  if ((threadIdx.x & (kWave - 1)) == 0 && best > 0.0) atomicMax(bits, (unsigned long long)__double_as_longlong(best));
}

template <typename T>
__global__ void __launch_bounds__(256) umap_schedule_kernel(const T* __restrict__ val, int64_t nnz, const double* __restrict__ wmax, double rate,
                                                            double* __restrict__ next, double* __restrict__ nextn) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= nnz) return;
  const double eps = wmax[0] / (double)val[e];
  next[e] = eps;
  nextn[e] = eps / rate;   // (rate 0: infinite, never due)
}

// ---- stage 5: the start -----------------------------------------------------------------------------------------------------
// minmax[2 c], [2 c + 1] = the smallest and largest of column c = blockIdx.x (order-free)
template <typename T>
__global__ void __launch_bounds__(256) umap_minmax_kernel(const T* __restrict__ x, int64_t ldx, int64_t m, double* __restrict__ minmax) {
  __shared__ double smin[256], smax[256];
  const int c = blockIdx.x;
  double lo = INFINITY, hi = -INFINITY;
  for (int64_t i = threadIdx.x; i < m; i += 256) {
    const double v = (double)x[i * ldx + c];
    lo = fmin(lo, v);
    hi = fmax(hi, v);
  }
  smin[threadIdx.x] = lo;
  smax[threadIdx.x] = hi;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      smin[threadIdx.x] = fmin(smin[threadIdx.x], smin[threadIdx.x + o]);
      smax[threadIdx.x] = fmax(smax[threadIdx.x], smax[threadIdx.x + o]);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    minmax[2 * c] = smin[0];
    minmax[2 * c + 1] = smax[0];
  }
}

template <typename T>
__global__ void umap_init_panel_kernel(const T* __restrict__ x, int64_t ldx, int64_t m, int D, const double* __restrict__ minmax,
                                       T* __restrict__ y) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= m * D) return;
  const int64_t i = e / D;
  const int c = (int)(e - i * D);
  const double lo = minmax[2 * c], range = minmax[2 * c + 1] - lo;
  y[e] = (T)(range > 0.0 ? 10.0 * ((double)x[i * ldx + c] - lo) / range : 0.0);
}

template <typename T>
__global__ void umap_init_random_kernel(T* __restrict__ y, int64_t n, uint64_t seed) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < n) y[e] = (T)(10.0 * hash_u01(seed, 31, (uint64_t)e));
}

// ---- stage 5: one epoch -----------------------------------------------------------------------------------------------------
__device__ inline double clip4(double v) { return v > 4.0 ? 4.0 : (v < -4.0 ? -4.0 : v); }

template <typename T, int D>
__global__ void __launch_bounds__(256) umap_epoch_kernel(const int64_t* __restrict__ ptr, const int32_t* __restrict__ idx, const T* __restrict__ val,
                                                         const T* __restrict__ y_in, T* __restrict__ y_out, int64_t m, uint64_t nnz,
                                                         UmapEpoch p, const double* __restrict__ wmax_p, double* __restrict__ next,
                                                         double* __restrict__ nextn) {
  const int sub = threadIdx.x & (kSub - 1);
  const int64_t i = (int64_t)blockIdx.x * (256 / kSub) + (threadIdx.x / kSub);
  const bool live = i < m;   // (no early exit: the butterfly below takes whole groups, and a wave may hold the panel's end)
  const double wmax = wmax_p[0], thr = wmax / p.n_epochs, nd = (double)p.epoch;
  T yt[D];
  double yi[D], acc[D];
#pragma unroll
  for (int c = 0; c < D; ++c) {
    yt[c] = live ? y_in[i * D + c] : (T)0;
    yi[c] = (double)yt[c];
    acc[c] = 0.0;
  }
  const int64_t lo = live ? ptr[i] : 0, hi = live ? ptr[i + 1] : 0;
  for (int64_t e = lo + sub; e < hi; e += kSub) {
    const double w = (double)val[e];
    if (!(w > 0.0) || w < thr) continue;   // left out of the layout
    const double nx = next[e];
    if (!(nx <= nd)) continue;
    const int32_t j = idx[e];
    if (j < 0 || (int64_t)j >= m) continue;   // (a caller's CSR: nothing outside the panel is read)
    const double eps = wmax / w;
    {
      double dl[D], s = 0.0;
#pragma unroll
      for (int c = 0; c < D; ++c) {
        dl[c] = yi[c] - (double)y_in[(int64_t)j * D + c];
        s += dl[c] * dl[c];
      }
      if (s > 0.0) {
        const double sb = pow(s, p.b);
        const double coef = -2.0 * p.a * p.b * (sb / s) / (p.a * sb + 1.0);
#pragma unroll
        for (int c = 0; c < D; ++c) acc[c] += clip4(coef * dl[c]);
      }
    }
    next[e] = nx + eps;
    if (p.rate > 0.0) {
      const double epsn = eps / p.rate, nn = nextn[e];
      const double q = floor((nd - nn) / epsn);
      const int qi = q > 0.0 ? (q < 64.0 ? (int)q : 64) : 0;   // (q <= 2 rate <= 62 by the schedule; the cap keeps p < 64 on any input)
      const uint64_t ctr = ((uint64_t)p.epoch * nnz + (uint64_t)e) * 64ull;
      for (int t = 0; t < qi; ++t) {
        int64_t kk = (int64_t)floor(hash_u01(p.seed, 32, ctr + (uint64_t)t) * (double)m);
        kk = kk < m ? kk : m - 1;
        double dl[D], s = 0.0;
#pragma unroll
        for (int c = 0; c < D; ++c) {
          dl[c] = yi[c] - (double)y_in[kk * D + c];
          s += dl[c] * dl[c];
        }
        if (s > 0.0) {
          const double sb = pow(s, p.b);
          const double coef = 2.0 * p.gamma * p.b / ((0.001 + s) * (p.a * sb + 1.0));
#pragma unroll
          for (int c = 0; c < D; ++c) acc[c] += clip4(coef * dl[c]);
        }
      }
      if (q > 0.0) nextn[e] = nn + q * epsn;
    }
  }
#pragma unroll
  for (int c = 0; c < D; ++c) {
#pragma unroll
    for (int o = kSub / 2; o > 0; o >>= 1) acc[c] += __shfl_xor(acc[c], o, kSub);
  }
  if (live && sub == 0) {
#pragma unroll
    for (int c = 0; c < D; ++c) y_out[i * D + c] = acc[c] == 0.0 ? yt[c] : (T)(yi[c] + p.alpha * acc[c]);
  }
}

inline unsigned blocks_of(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

}  // namespace

template <typename T>
void umap_row_sums(const int32_t* idx, const T* dist, int64_t m, int K, double* rowsum, hipStream_t s) {
  if (m == 0) return;
  hipLaunchKernelGGL((umap_row_sums_kernel<T>), dim3(blocks_of(m, 4)), dim3(256), 0, s, idx, dist, m, K, rowsum);
  SAPCA_HIP(hipGetLastError());
}

template <typename T>
void umap_smooth(const int32_t* idx, const T* dist, int64_t m, int K, int n_neighbors, const double* total, double* a, double* sigma,
                 double* rho, hipStream_t s) {
  if (m == 0) return;
  hipLaunchKernelGGL((umap_smooth_kernel<T>), dim3(blocks_of(m, 4)), dim3(256), 0, s, idx, dist, m, K, (double)n_neighbors,
                     std::log2((double)n_neighbors), total, a, sigma, rho);
  SAPCA_HIP(hipGetLastError());
}

template <typename T>
void umap_union_fill(const int64_t* ptr, const int32_t* idx, const double* val, int64_t m, const int64_t* new_ptr, int32_t* out_idx,
                     T* out_val, hipStream_t s) {
  if (m <= 0) return;
  const unsigned blocks = (unsigned)std::min<int64_t>((m + 3) / 4, 16384);
  hipLaunchKernelGGL((umap_union_kernel<T>), dim3(blocks), dim3(256), 0, s, ptr, idx, val, m, new_ptr, out_idx, out_val);
  SAPCA_HIP(hipGetLastError());
}

template <typename T>
void umap_schedule(const T* val, int64_t nnz, int rate, double* wmax, double* next, double* nextn, hipStream_t s) {
  SAPCA_HIP(hipMemsetAsync(wmax, 0, sizeof(double), s));
  if (nnz == 0) return;
  unsigned g = blocks_of(nnz, 256);
  if (g > 4096) g = 4096;
  hipLaunchKernelGGL((umap_wmax_kernel<T>), dim3(g), dim3(256), 0, s, val, nnz, reinterpret_cast<unsigned long long*>(wmax));
  hipLaunchKernelGGL((umap_schedule_kernel<T>), dim3(blocks_of(nnz, 256)), dim3(256), 0, s, val, nnz, wmax, (double)rate, next, nextn);
  SAPCA_HIP(hipGetLastError());
}

template <typename T>
void umap_init_panel(const T* x, int64_t ldx, int64_t m, int D, double* minmax, T* y, hipStream_t s) {
  if (m == 0) return;
  hipLaunchKernelGGL((umap_minmax_kernel<T>), dim3((unsigned)D), dim3(256), 0, s, x, ldx, m, minmax);
  hipLaunchKernelGGL((umap_init_panel_kernel<T>), dim3(blocks_of(m * D, 256)), dim3(256), 0, s, x, ldx, m, D, minmax, y);
  SAPCA_HIP(hipGetLastError());
}

template <typename T>
void umap_init_random(T* y, int64_t m, int D, uint32_t seed, hipStream_t s) {
  if (m == 0) return;
  hipLaunchKernelGGL((umap_init_random_kernel<T>), dim3(blocks_of(m * D, 256)), dim3(256), 0, s, y, m * D, (uint64_t)seed);
  SAPCA_HIP(hipGetLastError());
}

template <typename T>
void umap_epoch(const CsrView<T>& G, const T* y_in, T* y_out, int D, const UmapEpoch& p, const double* wmax, double* next, double* nextn,
                hipStream_t s) {
  const int64_t m = G.rows;
  if (m == 0) return;
  const dim3 g(blocks_of(m, 256 / kSub)), b(256);
  const uint64_t nnz = (uint64_t)G.nnz;
  switch (D) {
    case 1: hipLaunchKernelGGL((umap_epoch_kernel<T, 1>), g, b, 0, s, G.ptr, G.idx, G.val, y_in, y_out, m, nnz, p, wmax, next, nextn); break;
    case 2: hipLaunchKernelGGL((umap_epoch_kernel<T, 2>), g, b, 0, s, G.ptr, G.idx, G.val, y_in, y_out, m, nnz, p, wmax, next, nextn); break;
    case 3: hipLaunchKernelGGL((umap_epoch_kernel<T, 3>), g, b, 0, s, G.ptr, G.idx, G.val, y_in, y_out, m, nnz, p, wmax, next, nextn); break;
    default: throw Error(SAPCA_ERR_ARG, "umap_epoch: output_dim outside 1..3");
  }
  SAPCA_HIP(hipGetLastError());
}

#define SAPCA_INSTANTIATE_UMAP(T)                                                                                                          \
  template void umap_row_sums<T>(const int32_t*, const T*, int64_t, int, double*, hipStream_t);                                            \
  template void umap_smooth<T>(const int32_t*, const T*, int64_t, int, int, const double*, double*, double*, double*, hipStream_t);        \
  template void umap_union_fill<T>(const int64_t*, const int32_t*, const double*, int64_t, const int64_t*, int32_t*, T*, hipStream_t);     \
  template void umap_schedule<T>(const T*, int64_t, int, double*, double*, double*, hipStream_t);                                          \
  template void umap_init_panel<T>(const T*, int64_t, int64_t, int, double*, T*, hipStream_t);                                             \
  template void umap_init_random<T>(T*, int64_t, int, uint32_t, hipStream_t);                                                              \
  template void umap_epoch<T>(const CsrView<T>&, const T*, T*, int, const UmapEpoch&, const double*, double*, double*, hipStream_t);
SAPCA_INSTANTIATE_UMAP(float)
SAPCA_INSTANTIATE_UMAP(double)
#undef SAPCA_INSTANTIATE_UMAP

}  // namespace k
}  // namespace sapca
