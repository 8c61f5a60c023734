// t-SNE on device-resident rows (sapca_tsne_*): the replacement of the reference's dimred::tsne (src/dimred/tsne/mod.rs:7-66,
// which hands a dense panel to bhtsne's Barnes-Hut t-SNE).  The algorithm is van der Maaten's bh_tsne with the repulsive
// term evaluated exactly (theta -> 0); include/sapca.h states it in full.  Stages:
//   perplexity   one wave per row: the bisection for beta_i on the K squared neighbour distances, all f64
//   count / emit the 2 m K entries {(i, j, p_j|i), (j, i, p_j|i)} as an unsorted CSR (integer atomics decide positions only;
//                canon.hip sorts every row by column and adds the pairs, so no order survives into a value)
//   scale        T((p_j|i + p_i|j) / (2 m)) from the f64 sums: one rounding
//   repulsion    all pairs: a workgroup owns 256 rows i (y_i and the sums in registers) and walks the rows j through LDS tiles
//                every lane reads at the same address (a broadcast, no bank conflict); pair arithmetic in T, per-lane sums
//                folded into f64 once per tile
//   attraction   a wave per CSR row, f64; writes the gradient and the row's Kullback-Leibler terms
//   update       gains, velocity, step; per-block column sums, then the mean taken off (both in a fixed order)
// Every sum that crosses lanes or workgroups is added in an order fixed by the shape alone: no floating-point atomics.
#include "exp_rn.h"
#include "kernels.h"

namespace sapca {
namespace k {

namespace {

constexpr int kWave = 64;

__device__ inline double wave_sum(double v) {   // the same value in every lane, one order
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
  return v;
}

// The sum of one value per lane to (nearly) the last bit: every butterfly step adds exactly (Knuth's two-sum) and carries the
// rounding errors along; the order is symmetric, so every lane ends with the same bits.  A row's normaliser then carries no
// summation order, and p_k|i only the roundings of exp and of one division.
__device__ inline void wave_sum_exact(double& hi, double& lo) {
#pragma clang fp contract(off)
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double ohi = __shfl_xor(hi, o, kWave), olo = __shfl_xor(lo, o, kWave);
    const double sum = hi + ohi;
    const double bb = sum - hi;
    const double err = (hi - (sum - bb)) + (ohi - bb);
    lo = (lo + olo) + err;
    hi = sum;
  }
}
// a + b of one lane's two slots summed over the wave: the lane's own rounding error joins the carried ones, and the total is
// rounded once
__device__ inline double wave_sum_exact2(double a, double b) {
#pragma clang fp contract(off)
  double hi = a + b;
  const double bb = hi - a;
  double lo = (a - (hi - bb)) + (b - bb);
  wave_sum_exact(hi, lo);
  return hi + lo;
}

// ---- stage 2: conditional affinities ------------------------------------------------------------------------------------
// A slot whose index is outside [0, m) contributes nothing and gets p = 0.
template <typename T>
__global__ void __launch_bounds__(256) tsne_perplexity_kernel(const int32_t* __restrict__ idx, const T* __restrict__ dist, int64_t m, int K,
                                                              double log_perp, double* __restrict__ p_out, double* __restrict__ beta_out) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t row = (int64_t)blockIdx.x * (blockDim.x / kWave) + (threadIdx.x / kWave);
  if (row >= m) return;   // (whole waves leave together)
  double D[2];
  bool ok[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int slot = lane + t * kWave;
    ok[t] = false;
    D[t] = 0.0;
    if (slot < K) {
      const int32_t j = idx[row * K + slot];
      if (j >= 0 && (int64_t)j < m) {
        const double d = (double)dist[row * K + slot];
        D[t] = d * d;
        ok[t] = true;
      }
    }
  }
  double beta = 1.0, lo = -INFINITY, hi = INFINITY;
  for (int it = 0; it < 200; ++it) {
    const double p0 = ok[0] ? exp(-beta * D[0]) : 0.0, p1 = ok[1] ? exp(-beta * D[1]) : 0.0;
    const double s = wave_sum_exact2(p0, p1) + 2.2250738585072014e-308;
    const double dp = wave_sum_exact2(D[0] * p0, D[1] * p1);
    const double diff = log(s) + beta * dp / s - log_perp;
    if (fabs(diff) < 1e-5) break;
    if (diff > 0) {
      lo = beta;
      beta = (hi == INFINITY) ? beta * 2.0 : 0.5 * (beta + hi);
    } else {
      hi = beta;
      beta = (lo == -INFINITY) ? beta * 0.5 : 0.5 * (beta + lo);
    }
  }
  const double p0 = ok[0] ? exp_rn(-beta * D[0]) : 0.0, p1 = ok[1] ? exp_rn(-beta * D[1]) : 0.0;
  const double s = wave_sum_exact2(p0, p1) + 2.2250738585072014e-308;
  if (lane < K) p_out[row * K + lane] = p0 / s;
  if (lane + kWave < K) p_out[row * K + lane + kWave] = p1 / s;
  if (lane == 0 && beta_out) beta_out[row] = beta;
}

// ---- stage 3: the emitted entries as an unsorted CSR ----------------------------------------------------------------------
// len[r] += the valid slots of row r + the rows that list r; nvalid[r] = the former.  len is zeroed by the caller (m + 1 words).
__global__ void __launch_bounds__(256) tsne_count_kernel(const int32_t* __restrict__ idx, int64_t m, int K, int64_t* __restrict__ len,
                                                         int32_t* __restrict__ nvalid) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t row = (int64_t)blockIdx.x * (blockDim.x / kWave) + (threadIdx.x / kWave);
  if (row >= m) return;
  int n = 0;
  for (int slot = lane; slot < K; slot += kWave) {
    const int32_t j = idx[row * K + slot];
    if (j >= 0 && (int64_t)j < m) {
      ++n;
      atomicAdd(reinterpret_cast<unsigned long long*>(len + j), 1ull);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, kWave);
  if (lane == 0) {
    nvalid[row] = n;
    atomicAdd(reinterpret_cast<unsigned long long*>(len + row), (unsigned long long)n);
  }
}

// row i: its valid slots in slot order at ptr[i] .., and (i, p_j|i) into row j behind row j's own, at a position an integer
// cursor hands out.  cursor is zeroed by the caller.  Every position below ptr[m] is written exactly once.
__global__ void __launch_bounds__(256) tsne_emit_kernel(const int32_t* __restrict__ idx, const double* __restrict__ p, int64_t m, int K,
                                                        const int64_t* __restrict__ ptr, const int32_t* __restrict__ nvalid,
                                                        int32_t* __restrict__ cursor, int32_t* __restrict__ out_idx, double* __restrict__ out_val) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t row = (int64_t)blockIdx.x * (blockDim.x / kWave) + (threadIdx.x / kWave);
  if (row >= m) return;
  int before = 0;
  for (int base = 0; base < K; base += kWave) {   // (uniform trip count: the ballot sees whole waves)
    const int slot = base + lane;
    int32_t j = -1;
    if (slot < K) j = idx[row * K + slot];
    const bool ok = j >= 0 && (int64_t)j < m;
    const unsigned long long mask = __ballot(ok);
    if (ok) {
      const double v = p[row * K + slot];
      const int rank = before + __popcll(mask & ((1ull << lane) - 1ull));
      out_idx[ptr[row] + rank] = j;
      out_val[ptr[row] + rank] = v;
      const int64_t at = ptr[j] + nvalid[j] + atomicAdd(cursor + j, 1);
      out_idx[at] = (int32_t)row;
      out_val[at] = v;
    }
    before += __popcll(mask);
  }
}

template <typename T>
__global__ void tsne_scale_kernel(const double* __restrict__ in, int64_t nnz, double inv, T* __restrict__ out) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < nnz; i += stride) out[i] = (T)(in[i] * inv);
}

// ---- stage 4: repulsion ---------------------------------------------------------------------------------------------------
constexpr int kRepBlock = 256;    // rows i per workgroup, one per lane
constexpr int kRepTile = 1024;    // rows j per LDS tile

template <typename T>
__device__ inline T recip(T x);
template <>
__device__ inline float recip<float>(float x) { return __builtin_amdgcn_rcpf(x); }
template <>
__device__ inline double recip<double>(double x) { return 1.0 / x; }

// The chunk c of j tiles [c * tiles_per_chunk, ..) for the rows of i block blockIdx.x; SPLIT: blockIdx.y is the one chunk this
// workgroup takes and its sums go to part[(chunk * m + i) * (D + 1) ..]; otherwise the workgroup walks every chunk, each from
// zero, and adds the chunks' sums in chunk order -- what tsne_rep_merge does with the parts, so the two agree to the bit.
template <typename T, int D, bool SPLIT>
__global__ void __launch_bounds__(kRepBlock) tsne_repulsion_kernel(const T* __restrict__ y, int64_t ldy, int64_t m, int nchunk, int tiles_per_chunk,
                                                                   double* __restrict__ out) {
  __shared__ T tile[kRepTile * D];
  const int64_t i = (int64_t)blockIdx.x * kRepBlock + threadIdx.x;
  const int64_t i_lo = (int64_t)blockIdx.x * kRepBlock, i_hi = i_lo + kRepBlock;
  T yi[D];
#pragma unroll
  for (int c = 0; c < D; ++c) yi[c] = i < m ? y[i * ldy + c] : (T)0;
  const int64_t ntiles = (m + kRepTile - 1) / kRepTile;
  double tot[D + 1];
#pragma unroll
  for (int c = 0; c <= D; ++c) tot[c] = 0.0;
  const int c_lo = SPLIT ? (int)blockIdx.y : 0, c_hi = SPLIT ? (int)blockIdx.y + 1 : nchunk;
  for (int chunk = c_lo; chunk < c_hi; ++chunk) {
    double acc[D + 1];
#pragma unroll
    for (int c = 0; c <= D; ++c) acc[c] = 0.0;
    const int64_t t_lo = (int64_t)chunk * tiles_per_chunk;
    const int64_t t_hi = t_lo + tiles_per_chunk < ntiles ? t_lo + tiles_per_chunk : ntiles;
    for (int64_t t = t_lo; t < t_hi; ++t) {
      const int64_t j0 = t * kRepTile;
      const int jn = (int)(m - j0 < kRepTile ? m - j0 : kRepTile);
      __syncthreads();
      for (int e = threadIdx.x; e < jn * D; e += kRepBlock) {
        const int r = e / D, c = e - r * D;
        tile[e] = y[(j0 + r) * ldy + c];
      }
      __syncthreads();
      T f[D + 1];
#pragma unroll
      for (int c = 0; c <= D; ++c) f[c] = (T)0;
      if (j0 < i_hi && j0 + jn > i_lo) {   // this tile holds rows of the block: the pair i == j is left out by index
        const int self = (int)(i - j0);
        for (int j = 0; j < jn; ++j) {
          T d[D], d2 = (T)1;
#pragma unroll
          for (int c = 0; c < D; ++c) {
            d[c] = yi[c] - tile[j * D + c];
            d2 += d[c] * d[c];
          }
          T q = recip<T>(d2);
          q = (j == self) ? (T)0 : q;
          const T q2 = q * q;
#pragma unroll
          for (int c = 0; c < D; ++c) f[c] += q2 * d[c];
          f[D] += q;
        }
      } else {
#pragma unroll 4
        for (int j = 0; j < jn; ++j) {
          T d[D], d2 = (T)1;
#pragma unroll
          for (int c = 0; c < D; ++c) {
            d[c] = yi[c] - tile[j * D + c];
            d2 += d[c] * d[c];
          }
          const T q = recip<T>(d2);
          const T q2 = q * q;
#pragma unroll
          for (int c = 0; c < D; ++c) f[c] += q2 * d[c];
          f[D] += q;
        }
      }
#pragma unroll
      for (int c = 0; c <= D; ++c) acc[c] += (double)f[c];
    }
    if (SPLIT) {
#pragma unroll
      for (int c = 0; c <= D; ++c) tot[c] = acc[c];
    } else {
#pragma unroll
      for (int c = 0; c <= D; ++c) tot[c] += acc[c];
    }
  }
  if (i < m) {
    double* o = SPLIT ? out + ((int64_t)blockIdx.y * m + i) * (D + 1) : out + i * (D + 1);
#pragma unroll
    for (int c = 0; c <= D; ++c) o[c] = tot[c];
  }
}

// rep[i][0 .. D] = the chunks' parts of row i, added in chunk order from zero
__global__ void tsne_rep_merge_kernel(const double* __restrict__ part, int64_t m, int width, int nchunk, double* __restrict__ rep) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= m * width) return;
  double v = 0.0;
  for (int c = 0; c < nchunk; ++c) v += part[(int64_t)c * m * width + e];
  rep[e] = v;
}

// ---- sums in a fixed order ------------------------------------------------------------------------------------------------
// A block's 256 lanes each add their elements (stride 256 inside the block's span of kSumSpan), then a tree in LDS.
constexpr int kSumSpan = 8192;

__device__ inline double block_tree_sum(double v, double* sh) {
  sh[threadIdx.x] = v;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
    __syncthreads();
  }
  const double r = sh[0];
  __syncthreads();
  return r;
}

// part[b * ncol + c] = sum over the block's span of in[e * stride + offset + c]
__global__ void __launch_bounds__(256) tsne_sum1_kernel(const double* __restrict__ in, int64_t n, int stride, int offset, int ncol,
                                                        double* __restrict__ part) {
  __shared__ double sh[256];
  const int64_t lo = (int64_t)blockIdx.x * kSumSpan;
  const int64_t hi = lo + kSumSpan < n ? lo + kSumSpan : n;
  for (int c = 0; c < ncol; ++c) {
    double v = 0.0;
    for (int64_t e = lo + threadIdx.x; e < hi; e += 256) v += in[e * stride + offset + c];
    const double r = block_tree_sum(v, sh);
    if (threadIdx.x == 0) part[(int64_t)blockIdx.x * ncol + c] = r;
  }
}
// out[c] = scale * sum_b part[b * ncol + c]; one workgroup
__global__ void __launch_bounds__(256) tsne_sum2_kernel(const double* __restrict__ part, int64_t nb, int ncol, double scale, double* __restrict__ out) {
  __shared__ double sh[256];
  for (int c = 0; c < ncol; ++c) {
    double v = 0.0;
    for (int64_t b = threadIdx.x; b < nb; b += 256) v += part[b * ncol + c];
    const double r = block_tree_sum(v, sh);
    if (threadIdx.x == 0) out[c] = scale * r;
  }
}

// ---- stage 4: attraction, the gradient and the Kullback-Leibler terms -----------------------------------------------------
// grad[i][c] = T(e * sum_j P_ij q_ij (y_i - y_j)[c] - rep[i][c] / Z) (a single row: Z = 0, no repulsion, no KL term); klrow[i] = sum_j P_ij ln(P_ij Z / q_ij) (P_ij > 0 only)
template <typename T, int D>
__global__ void __launch_bounds__(256) tsne_attraction_kernel(const int64_t* __restrict__ ptr, const int32_t* __restrict__ idx, const T* __restrict__ val,
                                                              const T* __restrict__ y, int64_t ldy, int64_t m, double exaggeration,
                                                              const double* __restrict__ rep, const double* __restrict__ zp,
                                                              T* __restrict__ grad, double* __restrict__ klrow) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t row = (int64_t)blockIdx.x * (blockDim.x / kWave) + (threadIdx.x / kWave);
  if (row >= m) return;
  const double Z = zp[0];
  double yi[D], a[D], kl = 0.0;
#pragma unroll
  for (int c = 0; c < D; ++c) {
    yi[c] = (double)y[row * ldy + c];
    a[c] = 0.0;
  }
  const int64_t lo = ptr[row], hi = ptr[row + 1];
  for (int64_t e = lo + lane; e < hi; e += kWave) {
    const int32_t j = idx[e];
    if (j < 0 || (int64_t)j >= m) continue;   // (a caller's CSR: nothing outside the panel is read)
    const double P = (double)val[e];
    double d[D], d2 = 1.0;
#pragma unroll
    for (int c = 0; c < D; ++c) {
      d[c] = yi[c] - (double)y[(int64_t)j * ldy + c];
      d2 += d[c] * d[c];
    }
    const double q = 1.0 / d2;
#pragma unroll
    for (int c = 0; c < D; ++c) a[c] += P * q * d[c];
    if (P > 0.0 && Z > 0.0) kl += P * log(P * Z / q);
  }
#pragma unroll
  for (int c = 0; c < D; ++c) a[c] = wave_sum(a[c]);
  kl = wave_sum(kl);
  if (lane == 0) {
#pragma unroll
    for (int c = 0; c < D; ++c) grad[row * D + c] = (T)(exaggeration * a[c] - (Z > 0.0 ? rep[row * (D + 1) + c] / Z : 0.0));
    klrow[row] = kl;
  }
}

// ---- stage 5: the update --------------------------------------------------------------------------------------------------
__device__ inline int sgn(double x) { return (x > 0.0) - (x < 0.0); }

// a lane per row; colpart[b * D + c] = the block's column sums of the new y (f64, tree order)
template <typename T, int D>
__global__ void __launch_bounds__(256) tsne_update_kernel(T* __restrict__ y, T* __restrict__ v, T* __restrict__ gain, const T* __restrict__ grad,
                                                          int64_t m, double momentum, double rate, double* __restrict__ colpart) {
  __shared__ double sh[256];
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  double yn[D];
#pragma unroll
  for (int c = 0; c < D; ++c) yn[c] = 0.0;
  if (i < m) {
#pragma unroll
    for (int c = 0; c < D; ++c) {
      const int64_t e = i * D + c;
      const T g = grad[e], vel = v[e];
      T gn = gain[e];
      gn = (sgn((double)g) != sgn((double)vel)) ? gn + (T)0.2 : gn * (T)0.8;
      gn = gn < (T)0.01 ? (T)0.01 : gn;
      const T vn = (T)momentum * vel - (T)rate * gn * g;
      const T yy = y[e] + vn;
      gain[e] = gn;
      v[e] = vn;
      y[e] = yy;
      yn[c] = (double)yy;
    }
  }
#pragma unroll
  for (int c = 0; c < D; ++c) {
    const double r = block_tree_sum(yn[c], sh);
    if (threadIdx.x == 0) colpart[(int64_t)blockIdx.x * D + c] = r;
  }
}

// colpart of y as it stands (the initial embedding): the same layout as the update's
template <typename T, int D>
__global__ void __launch_bounds__(256) tsne_colsum_kernel(const T* __restrict__ y, int64_t m, double* __restrict__ colpart) {
  __shared__ double sh[256];
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
#pragma unroll
  for (int c = 0; c < D; ++c) {
    const double r = block_tree_sum(i < m ? (double)y[i * D + c] : 0.0, sh);
    if (threadIdx.x == 0) colpart[(int64_t)blockIdx.x * D + c] = r;
  }
}

// y[i][c] = T(y[i][c] - mean[c])
template <typename T, int D>
__global__ void tsne_center_kernel(T* __restrict__ y, int64_t m, const double* __restrict__ mean) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= m * D) return;
  y[e] = (T)((double)y[e] - mean[e % D]);
}

template <typename T>
__global__ void tsne_fill_kernel(T* __restrict__ p, int64_t n, T value) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < n) p[e] = value;
}
template <typename T>
__global__ void tsne_scale_inplace_kernel(T* __restrict__ p, int64_t n, T f) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < n) p[e] = p[e] * f;
}

inline unsigned blocks_of(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

}  // namespace

template <typename T>
void tsne_perplexity(const int32_t* idx, const T* dist, int64_t m, int K, double perplexity, double* p, double* beta, hipStream_t s) {
  if (m == 0) return;
  hipLaunchKernelGGL((tsne_perplexity_kernel<T>), dim3(blocks_of(m, 4)), dim3(256), 0, s, idx, dist, m, K, std::log(perplexity), p, beta);
  SAPCA_HIP(hipGetLastError());
}

void tsne_count(const int32_t* idx, int64_t m, int K, int64_t* len, int32_t* nvalid, hipStream_t s) {
  SAPCA_HIP(hipMemsetAsync(len, 0, (size_t)(m + 1) * sizeof(int64_t), s));
  if (m == 0) return;
  hipLaunchKernelGGL(tsne_count_kernel, dim3(blocks_of(m, 4)), dim3(256), 0, s, idx, m, K, len, nvalid);
  SAPCA_HIP(hipGetLastError());
}

void tsne_emit(const int32_t* idx, const double* p, int64_t m, int K, const int64_t* ptr, const int32_t* nvalid, int32_t* cursor,
               int32_t* out_idx, double* out_val, hipStream_t s) {
  if (m == 0) return;
  SAPCA_HIP(hipMemsetAsync(cursor, 0, (size_t)m * sizeof(int32_t), s));
  hipLaunchKernelGGL(tsne_emit_kernel, dim3(blocks_of(m, 4)), dim3(256), 0, s, idx, p, m, K, ptr, nvalid, cursor, out_idx, out_val);
  SAPCA_HIP(hipGetLastError());
}

template <typename T>
void tsne_scale(const double* in, int64_t nnz, double inv, T* out, hipStream_t s) {
  if (nnz == 0) return;
  unsigned g = blocks_of(nnz, 256);
  if (g > 8192) g = 8192;
  hipLaunchKernelGGL((tsne_scale_kernel<T>), dim3(g), dim3(256), 0, s, in, nnz, inv, out);
  SAPCA_HIP(hipGetLastError());
}

TsnePlan tsne_plan(int64_t m, int n_cus) {
  TsnePlan p;
  const int64_t ntiles = (m + kRepTile - 1) / kRepTile;
  p.nchunk = (int)(ntiles < 8 ? (ntiles < 1 ? 1 : ntiles) : 8);
  p.tiles_per_chunk = (int)((ntiles + p.nchunk - 1) / p.nchunk);
  if (p.tiles_per_chunk < 1) p.tiles_per_chunk = 1;
  p.split = p.nchunk > 1 && (m + kRepBlock - 1) / kRepBlock < (int64_t)n_cus;
  if (const char* f = dbg_env("SAPCA_TSNE_SPLIT")) p.split = p.nchunk > 1 && f[0] != '0';
  return p;
}

template <typename T, int D>
static void repulsion_d(const T* y, int64_t ldy, int64_t m, const TsnePlan& plan, double* part, double* rep, hipStream_t s) {
  const unsigned nib = blocks_of(m, kRepBlock);
  if (plan.split) {
    hipLaunchKernelGGL((tsne_repulsion_kernel<T, D, true>), dim3(nib, (unsigned)plan.nchunk), dim3(kRepBlock), 0, s, y, ldy, m, plan.nchunk,
                       plan.tiles_per_chunk, part);
    SAPCA_HIP(hipGetLastError());
    hipLaunchKernelGGL(tsne_rep_merge_kernel, dim3(blocks_of(m * (D + 1), 256)), dim3(256), 0, s, part, m, D + 1, plan.nchunk, rep);
  } else {
    hipLaunchKernelGGL((tsne_repulsion_kernel<T, D, false>), dim3(nib), dim3(kRepBlock), 0, s, y, ldy, m, plan.nchunk, plan.tiles_per_chunk, rep);
  }
  SAPCA_HIP(hipGetLastError());
}

size_t tsne_sum_parts(int64_t n) { return (size_t)((n + kSumSpan - 1) / kSumSpan); }

template <typename T>
void tsne_repulsion(const T* y, int64_t ldy, int64_t m, int D, const TsnePlan& plan, double* part, double* rep, double* sum_part, double* z,
                    hipStream_t s) {
  switch (D) {
    case 1: repulsion_d<T, 1>(y, ldy, m, plan, part, rep, s); break;
    case 2: repulsion_d<T, 2>(y, ldy, m, plan, part, rep, s); break;
    case 3: repulsion_d<T, 3>(y, ldy, m, plan, part, rep, s); break;
    default: throw Error(SAPCA_ERR_ARG, "tsne_repulsion: output_dim outside 1..3");
  }
  const int64_t nb = (int64_t)tsne_sum_parts(m);
  hipLaunchKernelGGL(tsne_sum1_kernel, dim3((unsigned)nb), dim3(256), 0, s, rep, m, D + 1, D, 1, sum_part);
  hipLaunchKernelGGL(tsne_sum2_kernel, dim3(1), dim3(256), 0, s, sum_part, nb, 1, 1.0, z);
  SAPCA_HIP(hipGetLastError());
}

template <typename T>
void tsne_attraction(const CsrView<T>& P, const T* y, int64_t ldy, int D, double exaggeration, const double* rep, const double* z, T* grad,
                     double* klrow, hipStream_t s) {
  const int64_t m = P.rows;
  const dim3 g(blocks_of(m, 4)), b(256);
  switch (D) {
    case 1: hipLaunchKernelGGL((tsne_attraction_kernel<T, 1>), g, b, 0, s, P.ptr, P.idx, P.val, y, ldy, m, exaggeration, rep, z, grad, klrow); break;
    case 2: hipLaunchKernelGGL((tsne_attraction_kernel<T, 2>), g, b, 0, s, P.ptr, P.idx, P.val, y, ldy, m, exaggeration, rep, z, grad, klrow); break;
    case 3: hipLaunchKernelGGL((tsne_attraction_kernel<T, 3>), g, b, 0, s, P.ptr, P.idx, P.val, y, ldy, m, exaggeration, rep, z, grad, klrow); break;
    default: throw Error(SAPCA_ERR_ARG, "tsne_attraction: output_dim outside 1..3");
  }
  SAPCA_HIP(hipGetLastError());
}

void tsne_sum(const double* in, int64_t n, double* sum_part, double* out, hipStream_t s) {
  const int64_t nb = (int64_t)tsne_sum_parts(n);
  hipLaunchKernelGGL(tsne_sum1_kernel, dim3((unsigned)nb), dim3(256), 0, s, in, n, 1, 0, 1, sum_part);
  hipLaunchKernelGGL(tsne_sum2_kernel, dim3(1), dim3(256), 0, s, sum_part, nb, 1, 1.0, out);
  SAPCA_HIP(hipGetLastError());
}

template <typename T>
void tsne_update(T* y, T* v, T* gain, const T* grad, int64_t m, int D, double momentum, double rate, double* colpart, double* mean,
                 hipStream_t s) {
  const unsigned nb = blocks_of(m, 256);
  switch (D) {
    case 1: hipLaunchKernelGGL((tsne_update_kernel<T, 1>), dim3(nb), dim3(256), 0, s, y, v, gain, grad, m, momentum, rate, colpart); break;
    case 2: hipLaunchKernelGGL((tsne_update_kernel<T, 2>), dim3(nb), dim3(256), 0, s, y, v, gain, grad, m, momentum, rate, colpart); break;
    case 3: hipLaunchKernelGGL((tsne_update_kernel<T, 3>), dim3(nb), dim3(256), 0, s, y, v, gain, grad, m, momentum, rate, colpart); break;
    default: throw Error(SAPCA_ERR_ARG, "tsne_update: output_dim outside 1..3");
  }
  SAPCA_HIP(hipGetLastError());
  tsne_center<T>(y, m, D, colpart, mean, false, s);
}

template <typename T>
void tsne_center(T* y, int64_t m, int D, double* colpart, double* mean, bool sum_first, hipStream_t s) {
  const unsigned nb = blocks_of(m, 256);
  if (sum_first) {
    switch (D) {
      case 1: hipLaunchKernelGGL((tsne_colsum_kernel<T, 1>), dim3(nb), dim3(256), 0, s, y, m, colpart); break;
      case 2: hipLaunchKernelGGL((tsne_colsum_kernel<T, 2>), dim3(nb), dim3(256), 0, s, y, m, colpart); break;
      default: hipLaunchKernelGGL((tsne_colsum_kernel<T, 3>), dim3(nb), dim3(256), 0, s, y, m, colpart); break;
    }
  }
  hipLaunchKernelGGL(tsne_sum2_kernel, dim3(1), dim3(256), 0, s, colpart, (int64_t)nb, D, 1.0 / (double)m, mean);
  const dim3 g(blocks_of(m * D, 256)), b(256);
  switch (D) {
    case 1: hipLaunchKernelGGL((tsne_center_kernel<T, 1>), g, b, 0, s, y, m, mean); break;
    case 2: hipLaunchKernelGGL((tsne_center_kernel<T, 2>), g, b, 0, s, y, m, mean); break;
    default: hipLaunchKernelGGL((tsne_center_kernel<T, 3>), g, b, 0, s, y, m, mean); break;
  }
  SAPCA_HIP(hipGetLastError());
}

template <typename T>
void tsne_init_state(T* y_or_null, T* v, T* gain, int64_t m, int D, uint32_t seed, hipStream_t s) {
  const int64_t n = m * D;
  if (n == 0) return;
  SAPCA_HIP(hipMemsetAsync(v, 0, (size_t)n * sizeof(T), s));
  hipLaunchKernelGGL((tsne_fill_kernel<T>), dim3(blocks_of(n, 256)), dim3(256), 0, s, gain, n, (T)1);
  if (y_or_null) {
    gaussian_panel<T>(y_or_null, m, D, D, seed, s);
    hipLaunchKernelGGL((tsne_scale_inplace_kernel<T>), dim3(blocks_of(n, 256)), dim3(256), 0, s, y_or_null, n, (T)1e-4);
  }
  SAPCA_HIP(hipGetLastError());
}

#define SAPCA_INSTANTIATE_TSNE(T)                                                                                                       \
  template void tsne_perplexity<T>(const int32_t*, const T*, int64_t, int, double, double*, double*, hipStream_t);                       \
  template void tsne_scale<T>(const double*, int64_t, double, T*, hipStream_t);                                                          \
  template void tsne_repulsion<T>(const T*, int64_t, int64_t, int, const TsnePlan&, double*, double*, double*, double*, hipStream_t);   \
  template void tsne_attraction<T>(const CsrView<T>&, const T*, int64_t, int, double, const double*, const double*, T*, double*, hipStream_t); \
  template void tsne_update<T>(T*, T*, T*, const T*, int64_t, int, double, double, double*, double*, hipStream_t);                       \
  template void tsne_center<T>(T*, int64_t, int, double*, double*, bool, hipStream_t);                                                   \
  template void tsne_init_state<T>(T*, T*, T*, int64_t, int, uint32_t, hipStream_t);
SAPCA_INSTANTIATE_TSNE(float)
SAPCA_INSTANTIATE_TSNE(double)
#undef SAPCA_INSTANTIATE_TSNE

}  // namespace k
}  // namespace sapca
