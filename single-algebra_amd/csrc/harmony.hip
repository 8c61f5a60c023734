// Harmony on dense row panels (sapca_harmony_*): unit rows -> (sums -> centroids -> order -> (fold -> block)* -> fold -> objective)*
// -> sums -> beta -> apply.
//
// block: the soft assignment is kmeans.hip's ranking problem with a softmax behind it.  A workgroup owns 64 rows of a block's list
// (16 per wave) and streams 64-centroid tiles of Y through LDS onto v_mfma_f32_16x16x4_f32 / v_mfma_f64_16x16x4_f64.  It sweeps Y
// three times -- the row's largest inner product; the f64 sum of exp(-(dist - min) / sigma) x the penalty of the row's batch; the
// normalised values, rounded once -- and every sweep recomputes the same k-ordered FMA chains, so the K scores of a row never
// leave the chip and K is not limited by registers or LDS.  fold: O / rs are f64 tables that one kernel per block moves: it adds
// the block before (from R as the block kernel left it), takes out the block to come and writes that block's penalty table.  A
// workgroup of 1024 threads owns 4 clusters for every batch, so no sum crosses a workgroup; the rows of a (block, batch) segment are summed in
// 256 interleaved lanes that are added pairwise in a fixed tree.  sums: R^T Zc and the ridge sums t are f64 sums over fixed slices of the rows
// (of every batch's list), folded in order by the kernels that consume them.  Integer atomics count rows; no floating-point
// atomic and no order reaches a value.
#include <algorithm>
#include <cmath>
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "hash_u01.h"
#include "kernels.h"
#include "rank_tile.h"

namespace sapca {
namespace k {

namespace {

constexpr uint64_t kOrderStream = 61;
constexpr int kSumCols = 64, kSumLanes = 4, kSumClusters = 16;   // harmony_sums: columns x row lanes per workgroup, clusters per thread
constexpr int kFoldClusters = 4, kFoldLanes = 256, kFoldThreads = kFoldClusters * kFoldLanes;               // harmony_fold: clusters x row lanes per workgroup

unsigned blocks_for(int64_t n, int per) { return (unsigned)std::min<int64_t>((n + per - 1) / per, 0x7FFFFFFF); }

// ---- unit rows: a wave per row -------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void hm_unit_kernel(const T* x, int64_t ldx, int64_t rows, int d, T* unit, int64_t ldu) {
  // (x and unit may be the same panel: a lane reads an element before it writes it, and no other lane touches it)
  const int lane = (int)threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * 4 + ((int)threadIdx.x >> 6);
  if (i >= rows) return;
  double s = 0.0;
  for (int t = lane; t < d; t += 64) {
    const double v = (double)x[i * ldx + t];
    s = fma(v, v, s);
  }
  for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off);
  const double nrm = sqrt(s);
  for (int t = lane; t < d; t += 64) unit[i * ldu + t] = nrm > 0.0 ? (T)((double)x[i * ldx + t] / nrm) : (T)0;
}

// ---- batches: counts, the first label out of range, the (batch, row) order -------------------------------------------------
// a workgroup counts kCountRows rows in an LDS histogram and adds every batch it met to the global counts once
constexpr int kCountRows = 4096;
__global__ __launch_bounds__(256) void hm_count_kernel(const int32_t* __restrict__ batch, int64_t m, int B, unsigned long long* __restrict__ cnt) {
  __shared__ unsigned hist[SAPCA_HARMONY_MAX_BATCHES];
  for (int b = (int)threadIdx.x; b < B; b += 256) hist[b] = 0u;
  __syncthreads();
  const int64_t lo = (int64_t)blockIdx.x * kCountRows, hi = lo + kCountRows < m ? lo + kCountRows : m;
  unsigned long long bad = ~0ull;
  for (int64_t i = lo + threadIdx.x; i < hi; i += 256) {
    const int b = batch[i];
    if (b >= 0 && b < B) atomicAdd(&hist[b], 1u);
    else if ((unsigned long long)i < bad) bad = (unsigned long long)i;
  }
  if (bad != ~0ull) atomicMin(cnt + B, bad);
  __syncthreads();
  for (int b = (int)threadIdx.x; b < B; b += 256)
    if (hist[b] != 0u) atomicAdd(cnt + b, (unsigned long long)hist[b]);
}

__global__ __launch_bounds__(256) void hm_batch_key_kernel(const int32_t* __restrict__ batch, int64_t m, int B, uint32_t* __restrict__ key,
                                                           uint32_t* __restrict__ val) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= m) return;
  const int b = batch[i];
  key[i] = b >= 0 && b < B ? (uint32_t)b : (uint32_t)B;   // (refused before this runs; kept inside the key space all the same)
  val[i] = (uint32_t)i;
}

// ---- the update order ------------------------------------------------------------------------------------------------------
// the 53 bits of hash_u01's uniform order as the uniform does
__global__ __launch_bounds__(256) void hm_hash_key_kernel(int64_t m, uint64_t seed, uint64_t pass, uint64_t* __restrict__ hkey,
                                                          uint32_t* __restrict__ iota) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= m) return;
  const double u = hash_u01(seed, kOrderStream, pass * (uint64_t)m + (uint64_t)i);
  hkey[i] = (uint64_t)(u * 9007199254740992.0);
  iota[i] = (uint32_t)i;
}

// the numpy.array_split piece of position p among nb pieces of m: the first m % nb pieces hold m / nb + 1
__host__ __device__ inline int64_t hm_block_of(int64_t p, int64_t m, int64_t nb) {
  const int64_t q = m / nb, r = m % nb, head = r * (q + 1);
  return p < head ? p / (q + 1) : r + (p - head) / q;   // (p >= head implies q >= 1: head == m when q == 0)
}
__host__ __device__ inline int64_t hm_block_begin(int64_t j, int64_t m, int64_t nb) {
  const int64_t q = m / nb, r = m % nb;
  return j < r ? j * (q + 1) : r * (q + 1) + (j - r) * q;
}

__global__ __launch_bounds__(256) void hm_block_key_kernel(const int32_t* __restrict__ batch, const uint32_t* __restrict__ perm, int64_t m,
                                                           int B, int64_t nb, uint64_t* __restrict__ key2) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= m) return;
  const uint32_t row = perm[p];
  int b = row < (uint64_t)m ? batch[row] : 0;
  if (b < 0 || b >= B) b = 0;
  key2[p] = (uint64_t)hm_block_of(p, m, nb) * (uint64_t)B + (uint64_t)b;
}

// ---- grouped weighted sums -------------------------------------------------------------------------------------------------
// grid (slices * column tiles, cluster tiles, batches); thread (tc, tr) adds the rows tr, tr + 4, .. of its slice for column
// t0 + tc and 16 clusters, then the four row lanes are added in order
template <typename T>
__global__ __launch_bounds__(256) void hm_sums_kernel(const T* __restrict__ x, int64_t ldx, int64_t m, int d, int D, const T* __restrict__ R,
                                                      int K, const uint32_t* __restrict__ order, const int64_t* __restrict__ seg, int slices,
                                                      double* __restrict__ partial) {
  __shared__ double buf[kSumLanes - 1][kSumCols][kSumClusters + 1];
  const int tid = (int)threadIdx.x, tc = tid % kSumCols, tr = tid / kSumCols;
  const int sl = (int)blockIdx.x % slices, t = ((int)blockIdx.x / slices) * kSumCols + tc;
  const int k0 = (int)blockIdx.y * kSumClusters, b = (int)blockIdx.z;
  const int64_t o0 = seg ? seg[b] : 0, o1 = seg ? seg[b + 1] : m;
  const int64_t n = o1 - o0, len = (n + slices - 1) / slices;
  const int64_t p0 = o0 + sl * len, p1 = p0 + len < o1 ? p0 + len : o1;
  double acc[kSumClusters];
#pragma unroll
  for (int j = 0; j < kSumClusters; ++j) acc[j] = 0.0;
  int64_t p = p0 + tr;
  for (; p + 3 * kSumLanes < p1; p += 4 * kSumLanes) {   // four rows' loads in flight; added in the same order as one by one
    int64_t row[4];
    T v[4], w[4][kSumClusters];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      row[u] = order ? (int64_t)order[p + u * kSumLanes] : p + u * kSumLanes;
      if (row[u] < 0 || row[u] >= m) row[u] = -1;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      v[u] = row[u] < 0 ? (T)0 : (t < d ? x[row[u] * ldx + t] : (t == d ? (T)1 : (T)0));
#pragma unroll
      for (int j = 0; j < kSumClusters; ++j) w[u][j] = row[u] >= 0 && k0 + j < K ? R[row[u] * K + k0 + j] : (T)0;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int j = 0; j < kSumClusters; ++j) acc[j] = fma((double)w[u][j], (double)v[u], acc[j]);
  }
  for (; p < p1; p += kSumLanes) {
    const int64_t row = order ? (int64_t)order[p] : p;
    if (row < 0 || row >= m) continue;
    const double v = t < d ? (double)x[row * ldx + t] : (t == d ? 1.0 : 0.0);
    const T* rr = R + row * K + k0;
#pragma unroll
    for (int j = 0; j < kSumClusters; ++j)
      if (k0 + j < K) acc[j] = fma((double)rr[j], v, acc[j]);
  }
  if (tr > 0) {
#pragma unroll
    for (int j = 0; j < kSumClusters; ++j) buf[tr - 1][tc][j] = acc[j];
  }
  __syncthreads();
  if (tr != 0 || t >= D) return;
#pragma unroll
  for (int j = 0; j < kSumClusters; ++j) {
    if (k0 + j >= K) continue;
    double sum = acc[j];
    for (int r = 0; r < kSumLanes - 1; ++r) sum += buf[r][tc][j];
    partial[(((int64_t)b * K + k0 + j) * slices + sl) * D + t] = sum;
  }
}

// sum of one value per thread of a 256-thread workgroup in an order fixed by the thread index, on every thread
__device__ inline double hm_block_sum(double v, double* sh) {
  __syncthreads();
  sh[threadIdx.x] = v;
  __syncthreads();
  for (int w = 128; w >= 1; w >>= 1) {
    if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
    __syncthreads();
  }
  return sh[0];
}

// a workgroup per cluster
template <typename T>
__global__ __launch_bounds__(256) void hm_centroids_kernel(const double* __restrict__ partial, int d, int slices, T* __restrict__ Y) {
  __shared__ double sh[256];
  __shared__ double col[1024];
  const int c = (int)blockIdx.x;
  double sq = 0.0;
  for (int t = (int)threadIdx.x; t < d; t += 256) {
    double sum = 0.0;
    for (int sl = 0; sl < slices; ++sl) sum += partial[((int64_t)c * slices + sl) * d + t];
    col[t] = sum;
    sq = fma(sum, sum, sq);
  }
  const double nrm = sqrt(hm_block_sum(sq, sh));
  for (int t = (int)threadIdx.x; t < d; t += 256) Y[(int64_t)c * d + t] = nrm > 0.0 ? (T)(col[t] / nrm) : (T)0;
}

// a workgroup per cluster: o_b, then a and beta_b column by column
__global__ __launch_bounds__(256) void hm_beta_kernel(const double* __restrict__ partial, int K, int B, int d, int slices, double lambda,
                                                      double* __restrict__ beta) {
  __shared__ double o[SAPCA_HARMONY_MAX_BATCHES];
  __shared__ double s_den;
  const int c = (int)blockIdx.x, D = d + 1;
  for (int b = (int)threadIdx.x; b < B; b += 256) {
    double sum = 0.0;
    for (int sl = 0; sl < slices; ++sl) sum += partial[(((int64_t)b * K + c) * slices + sl) * D + d];
    o[b] = sum;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double den = 0.0;
    for (int b = 0; b < B; ++b) den += lambda / (o[b] + lambda) * o[b];   // (1 - c_b = lambda / (o_b + lambda), without the cancellation)
    s_den = den;
  }
  __syncthreads();
  const double den = s_den;
  for (int t = (int)threadIdx.x; t < d; t += 256) {
    double num = 0.0;
    for (int b = 0; b < B; ++b) {
      double tb = 0.0;
      for (int sl = 0; sl < slices; ++sl) tb += partial[(((int64_t)b * K + c) * slices + sl) * D + t];
      num += lambda / (o[b] + lambda) * tb;
    }
    const double a = den > 0.0 ? num / den : 0.0;
    for (int b = 0; b < B; ++b) {
      double tb = 0.0;
      for (int sl = 0; sl < slices; ++sl) tb += partial[(((int64_t)b * K + c) * slices + sl) * D + t];
      beta[((int64_t)c * B + b) * d + t] = den > 0.0 ? (tb - o[b] * a) / (o[b] + lambda) : 0.0;
    }
  }
}

template <typename T>
__global__ __launch_bounds__(256) void hm_apply_kernel(const T* __restrict__ z, int64_t ldz, int64_t m, int d, const T* __restrict__ R, int K,
                                                       const int32_t* __restrict__ batch, int B, const double* __restrict__ beta,
                                                       T* __restrict__ out, int64_t ldc) {
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < m * d; e += (int64_t)gridDim.x * 256) {
  const int64_t i = e / d;
  const int t = (int)(e % d);
  const int b = batch[i];
  double v = (double)z[i * ldz + t];
  if (b >= 0 && b < B) {
    const T* rr = R + i * K;
    const double* bt = beta + (int64_t)b * d + t;
    double corr = 0.0;
    for (int c = 0; c < K; ++c) corr = fma((double)rr[c], bt[(int64_t)c * B * d], corr);
    v -= corr;
  }
  out[i * ldc + t] = (T)v;
  }
}

// O / rs from the slices' column sums of R: a thread per cluster, batches in order
__global__ __launch_bounds__(256) void hm_totals_kernel(const double* __restrict__ colsum, int K, int B, int slices, double* __restrict__ O,
                                                        double* __restrict__ rs) {
  const int c = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (c >= K) return;
  double tot = 0.0;
  for (int b = 0; b < B; ++b) {
    double sum = 0.0;
    for (int sl = 0; sl < slices; ++sl) sum += colsum[((int64_t)b * slices + sl) * K + c];
    O[(int64_t)b * K + c] = sum;
    tot += sum;
  }
  rs[c] = tot;
}

// colsum[(b * slices + sl) * K + c] = the f64 sum of R[row][c] over slice sl of batch b's list: four row lanes, added in order
template <typename T>
__global__ __launch_bounds__(256) void hm_colsum_kernel(const T* __restrict__ R, int64_t m, int K, const uint32_t* __restrict__ order,
                                                        const int64_t* __restrict__ seg, int slices, double* __restrict__ colsum) {
  __shared__ double buf[kSumLanes - 1][kSumCols];
  const int tid = (int)threadIdx.x, tc = tid % kSumCols, tr = tid / kSumCols;
  const int sl = (int)blockIdx.x, c = (int)blockIdx.y * kSumCols + tc, b = (int)blockIdx.z;
  const int64_t o0 = seg ? seg[b] : 0, o1 = seg ? seg[b + 1] : m;
  const int64_t n = o1 - o0, len = (n + slices - 1) / slices;
  const int64_t p0 = o0 + sl * len, p1 = p0 + len < o1 ? p0 + len : o1;
  double acc = 0.0;
  if (c < K)
    for (int64_t p = p0 + tr; p < p1; p += kSumLanes) {
      const int64_t row = order ? (int64_t)order[p] : p;
      if (row >= 0 && row < m) acc += (double)R[row * K + c];
    }
  if (tr > 0) buf[tr - 1][tc] = acc;
  __syncthreads();
  if (tr != 0 || c >= K) return;
  for (int r = 0; r < kSumLanes - 1; ++r) acc += buf[r][tc];
  colsum[((int64_t)b * slices + sl) * K + c] = acc;
}

// ---- the fold around a block -----------------------------------------------------------------------------------------------
// the first position of [lo, hi) whose key is not below `key`
__device__ inline int64_t hm_lower_bound(const uint64_t* keys, int64_t lo, int64_t hi, uint64_t key) {
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (keys[mid] < key) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// sums[b] for every batch of one block, this workgroup's 4 clusters: thread (kc, rl) adds the rows rl, rl + 256, .. of the
// block's segment of batch b; the lanes are halved onto each other in a fixed tree and lane rl == 0 and applies sign * sum to O and to its rs
template <typename T>
__device__ inline void hm_fold_block(const T* __restrict__ R, int64_t m, int K, int B, int64_t nb, int64_t j, double sign,
                                     const uint64_t* __restrict__ keys, const uint32_t* __restrict__ list, double* __restrict__ O,
                                     double& rsk, int64_t* bound, double (*red)[kFoldClusters]) {
  const int tid = (int)threadIdx.x, kc = tid % kFoldClusters, rl = tid / kFoldClusters;
  const int c = (int)blockIdx.x * kFoldClusters + kc;
  const int64_t q0 = hm_block_begin(j, m, nb), q1 = hm_block_begin(j + 1, m, nb);
  __syncthreads();   // (bound and red may still be read from the block before)
  for (int b = tid; b <= B; b += kFoldThreads) bound[b] = b == B ? q1 : hm_lower_bound(keys, q0, q1, (uint64_t)j * (uint64_t)B + (uint64_t)b);
  __syncthreads();
  for (int b = 0; b < B; ++b) {
    const int64_t lo = bound[b], hi = bound[b + 1];
    if (hi <= lo) continue;   // (uniform over the workgroup)
    double acc = 0.0;
    if (c < K) {
      int64_t p = lo + rl;
      for (; p + 7 * kFoldLanes < hi; p += 8 * kFoldLanes) {   // eight rows' loads in flight; added in the same order as one by one
        uint32_t row[8];
        double v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) row[u] = list[p + u * kFoldLanes];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = (int64_t)row[u] < m ? (double)R[(int64_t)row[u] * K + c] : 0.0;
#pragma unroll
        for (int u = 0; u < 8; ++u) acc += v[u];
      }
      for (; p < hi; p += kFoldLanes) {
        const uint32_t row = list[p];
        if ((int64_t)row < m) acc += (double)R[(int64_t)row * K + c];
      }
    }
    __syncthreads();
    red[rl][kc] = acc;
    __syncthreads();
    for (int w = kFoldLanes / 2; w >= 1; w >>= 1) {
      if (rl < w) red[rl][kc] += red[rl + w][kc];
      __syncthreads();
    }
    if (rl == 0 && c < K) {
      const double sum = red[0][kc];
      O[(int64_t)b * K + c] += sign * sum;
      rsk += sign * sum;
    }
  }
}

template <typename T>
__global__ __launch_bounds__(kFoldThreads) void hm_fold_kernel(const T* __restrict__ R, int64_t m, int K, int B, int64_t nb, int64_t add, int64_t remove,
                                                      const uint64_t* __restrict__ keys, const uint32_t* __restrict__ list,
                                                      const double* __restrict__ Pr, double theta, double* __restrict__ O,
                                                      double* __restrict__ rs, double* __restrict__ pen) {
  __shared__ int64_t bound[SAPCA_HARMONY_MAX_BATCHES + 1];
  __shared__ double red[kFoldLanes][kFoldClusters];
  __shared__ double s_rs[kFoldClusters];
  const int tid = (int)threadIdx.x, kc = tid % kFoldClusters, rl = tid / kFoldClusters;
  const int c = (int)blockIdx.x * kFoldClusters + kc;
  double rsk = rl == 0 && c < K ? rs[c] : 0.0;
  if (add >= 0) hm_fold_block<T>(R, m, K, B, nb, add, 1.0, keys, list, O, rsk, bound, red);
  if (remove >= 0) hm_fold_block<T>(R, m, K, B, nb, remove, -1.0, keys, list, O, rsk, bound, red);
  if (rl == 0) {
    s_rs[kc] = rsk;
    if (c < K) rs[c] = rsk;
  }
  __syncthreads();   // (and the O of this workgroup's clusters, written by its own lanes rl == 0 above, is read below by all)
  if (remove < 0 || c >= K) return;
  const double r = s_rs[kc];
  for (int b = rl; b < B; b += kFoldLanes) pen[(int64_t)b * K + c] = pow((Pr[b] * r + 1.0) / (O[(int64_t)b * K + c] + 1.0), theta);
}

// ---- the fused block update ------------------------------------------------------------------------------------------------
// 64 gathered rows x KC columns of the panel into registers (zero beyond d and for an empty slot), as knn_chunk_load lays them out
template <typename T, int KC>
__device__ inline void hm_gather_load(const T* base, int64_t ld, const int* s_row, int k0, int d, T* regs) {
  constexpr int RPI = kKnnThreads / KC;
  const int tr = (int)threadIdx.x / KC, tc = (int)threadIdx.x % KC;
#pragma unroll
  for (int i = 0; i < 64 / RPI; ++i) {
    const int row = s_row[tr + i * RPI];
    regs[i] = row >= 0 && k0 + tc < d ? base[(int64_t)row * ld + k0 + tc] : (T)0;
  }
}

template <typename T>
__global__ __launch_bounds__(kKnnThreads) void hm_block_kernel(const T* __restrict__ zc, int64_t ldz, int64_t m, int d, const T* __restrict__ Y,
                                                                int K, const int32_t* __restrict__ batch, int B,
                                                                const uint32_t* __restrict__ list, int64_t p0, int64_t n,
                                                                const double* __restrict__ pen, double sigma, T* __restrict__ R,
                                                                T* __restrict__ dist) {
  constexpr int KC = KnnChunk<T>::value, LD = KC + 4, QB = 64;
  using Acc = typename KnnAcc<T>::type;
  __shared__ __align__(16) T Qs[QB * LD];
  __shared__ __align__(16) T Cs[kKnnTile * LD];
  __shared__ int s_row[QB], s_bat[QB];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t q0 = (int64_t)blockIdx.x * QB;
  if (tid < QB) {
    int64_t row = -1;
    if (q0 + tid < n) {
      row = list ? (int64_t)list[p0 + q0 + tid] : p0 + q0 + tid;
      if (row >= m) row = -1;
    }
    int b = 0;
    if (row >= 0 && batch != nullptr) {
      b = batch[row];
      if (b < 0 || b >= B) b = 0;
    }
    s_row[tid] = (int)row;
    s_bat[tid] = b;
  }
  __syncthreads();

  const int ntiles = (K + kKnnTile - 1) / kKnnTile;
  const int nchunks = (d + KC - 1) / KC;
  const bool single = nchunks == 1;   // the rows' only chunk stays in LDS for all three sweeps
  const int steps = ntiles * nchunks;
  T qr[QB * KC / kKnnThreads], cr[kKnnTile * KC / kKnnThreads];
  if (single) {
    hm_gather_load<T, KC>(zc, ldz, s_row, 0, d, qr);
    knn_chunk_store<T, QB, KC>(qr, Qs);
  }
  knn_chunk_load<T, kKnnTile, KC>(Y, d, 0, K, 0, d, cr);
  if (!single) hm_gather_load<T, KC>(zc, ldz, s_row, 0, d, qr);

  int rowi[4], rowb[4];
  T best[4];
  double sum[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int q = wave * 16 + acc_row<T>(lane, r);
    rowi[r] = s_row[q];
    rowb[r] = s_bat[q];
    best[r] = -INFINITY;
    sum[r] = 0.0;
  }
  Acc acc[4];
  for (int gs = 0; gs < 3 * steps; ++gs) {
    const int phase = gs / steps, step = gs % steps;
    const int t = step / nchunks, ch = step % nchunks;
    __syncthreads();   // every wave is done with the previous chunk
    knn_chunk_store<T, kKnnTile, KC>(cr, Cs);
    if (!single) knn_chunk_store<T, QB, KC>(qr, Qs);
    __syncthreads();
    if (gs + 1 < 3 * steps) {   // the next chunk travels while this one is multiplied
      const int sn = (step + 1) % steps;
      const int tn = sn / nchunks, kn = (sn % nchunks) * KC;
      knn_chunk_load<T, kKnnTile, KC>(Y, d, (int64_t)tn * kKnnTile, K, kn, d, cr);
      if (!single) hm_gather_load<T, KC>(zc, ldz, s_row, kn, d, qr);
    }
    if (ch == 0) {
#pragma unroll
      for (int ct = 0; ct < 4; ++ct)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[ct][r] = (T)0;
    }
    const int left = d - ch * KC;
    const int ksteps = ((left < KC ? left : KC) + 3) / 4;   // d is padded to a multiple of 4 by the zeros in LDS
    const T* qa = Qs + (wave * 16 + (lane & 15)) * LD + (lane >> 4);
    const T* cb = Cs + (lane & 15) * LD + (lane >> 4);
    for (int ks = 0; ks < ksteps; ++ks) {
      const T a = qa[ks * 4];
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) acc[ct] = knn_mfma(a, cb[ct * 16 * LD + ks * 4], acc[ct]);
    }
    if (ch == nchunks - 1) {
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) {
        const int j = t * kKnnTile + ct * 16 + (lane & 15);
        if (j >= K) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const T dot = acc[ct][r];
          if (phase == 0) {
            if (dot > best[r]) best[r] = dot;
            continue;
          }
          if (rowi[r] < 0) continue;
          const double dk = 2.0 * (1.0 - (double)dot), dmin = 2.0 * (1.0 - (double)best[r]);
          double e = exp(-(dk - dmin) / sigma);
          if (pen != nullptr) e *= pen[(int64_t)rowb[r] * K + j];
          if (phase == 1) {
            sum[r] += e;
          } else {
            const int64_t at = (int64_t)rowi[r] * K + j;
            R[at] = sum[r] > 0.0 ? (T)(e / sum[r]) : (T)0;
            if (dist != nullptr) dist[at] = (T)dk;
          }
        }
      }
    }
    if (step != steps - 1 || phase == 2) continue;
    // the 16 lanes that hold a row's columns: the largest inner product after the first sweep, the sum after the second
#pragma unroll
    for (int off = 1; off < 16; off <<= 1)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (phase == 0) {
          const T ob = __shfl_xor(best[r], off);
          if (ob > best[r]) best[r] = ob;
        } else {
          sum[r] += __shfl_xor(sum[r], off);
        }
      }
  }
}

// ---- the objective: a wave per row -----------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void hm_objective_kernel(const T* __restrict__ R, const T* __restrict__ dist, const int32_t* __restrict__ batch,
                                                           int64_t m, int K, int B, const double* __restrict__ O, const double* __restrict__ rs,
                                                           const double* __restrict__ Pr, double sigma, double theta,
                                                           double* __restrict__ rowd) {
  const int lane = (int)threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * 4 + ((int)threadIdx.x >> 6);
  if (i >= m) return;
  int b = batch[i];
  if (b < 0 || b >= B) b = 0;
  const double pr = Pr[b];
  double t1 = 0.0, t2 = 0.0, t3 = 0.0;
  for (int c = lane; c < K; c += 64) {
    const double r = (double)R[i * K + c];
    t1 = fma(r, (double)dist[i * K + c], t1);
    if (r > 0.0) t2 = fma(r, log(r), t2);
    t3 = fma(r, log((O[(int64_t)b * K + c] + 1.0) / (pr * rs[c] + 1.0)), t3);
  }
  for (int off = 32; off >= 1; off >>= 1) {
    t1 += __shfl_xor(t1, off);
    t2 += __shfl_xor(t2, off);
    t3 += __shfl_xor(t3, off);
  }
  if (lane == 0) {
    rowd[i] = t1;
    rowd[m + i] = sigma * t2;
    rowd[2 * m + i] = sigma * theta * t3;
  }
}

template <typename K_, typename V_>
void sort_pairs(const K_* kin, K_* kout, const V_* vin, V_* vout, int64_t n, unsigned bits, DevBuf& tmp, hipStream_t s) {
  size_t bytes = 0;
  SAPCA_HIP(rocprim::radix_sort_pairs(nullptr, bytes, (const K_*)nullptr, (K_*)nullptr, (const V_*)nullptr, (V_*)nullptr, (size_t)n, 0u, bits, s));
  void* t = tmp.ensure(std::max<size_t>(bytes, 16));
  SAPCA_HIP(rocprim::radix_sort_pairs(t, bytes, kin, kout, vin, vout, (size_t)n, 0u, bits, s));
}

unsigned bits_for(uint64_t max_value) {
  unsigned b = 1;
  while (b < 64 && (max_value >> b) != 0) ++b;
  return b;
}

}  // namespace

template <typename T>
void harmony_unit_rows(const T* x, int64_t ldx, int64_t rows, int d, T* unit, int64_t ldu, hipStream_t s) {
  if (rows <= 0) return;
  hipLaunchKernelGGL((hm_unit_kernel<T>), dim3(blocks_for(rows, 4)), dim3(256), 0, s, x, ldx, rows, d, unit, ldu);
  SAPCA_HIP(hipGetLastError());
}

void harmony_count(const int32_t* batch, int64_t m, int B, unsigned long long* cnt, hipStream_t s) {
  SAPCA_HIP(hipMemsetAsync(cnt, 0, (size_t)B * sizeof(unsigned long long), s));
  const unsigned long long none = (unsigned long long)m;
  SAPCA_HIP(hipMemcpyAsync(cnt + B, &none, sizeof(none), hipMemcpyHostToDevice, s));
  SAPCA_HIP(hipStreamSynchronize(s));   // (`none` lives on this stack)
  if (m <= 0) return;
  hipLaunchKernelGGL(hm_count_kernel, dim3(blocks_for(m, kCountRows)), dim3(256), 0, s, batch, m, B, cnt);
  SAPCA_HIP(hipGetLastError());
}

void harmony_sort_batches(const int32_t* batch, int64_t m, int B, uint32_t* key, uint32_t* key_out, uint32_t* val, uint32_t* by_batch,
                          DevBuf& sort_tmp, hipStream_t s) {
  if (m <= 0) return;
  hipLaunchKernelGGL(hm_batch_key_kernel, dim3(blocks_for(m, 256)), dim3(256), 0, s, batch, m, B, key, val);
  SAPCA_HIP(hipGetLastError());
  sort_pairs(key, key_out, val, by_batch, m, bits_for((uint64_t)B), sort_tmp, s);   // (stable: rows ascend inside a batch)
}

void harmony_order(const int32_t* batch, int64_t m, int B, int64_t nb, uint64_t seed, uint64_t pass, uint64_t* hkey, uint64_t* hkey_out,
                   uint32_t* iota, uint32_t* perm, uint64_t* key2, uint64_t* keys, uint32_t* list, DevBuf& sort_tmp, hipStream_t s) {
  if (m <= 0) return;
  const dim3 grid(blocks_for(m, 256)), block(256);
  hipLaunchKernelGGL(hm_hash_key_kernel, grid, block, 0, s, m, seed, pass, hkey, iota);
  SAPCA_HIP(hipGetLastError());
  sort_pairs(hkey, hkey_out, iota, perm, m, 53u, sort_tmp, s);   // (stable: equal uniforms keep the row order)
  hipLaunchKernelGGL(hm_block_key_kernel, grid, block, 0, s, batch, perm, m, B, nb, key2);
  SAPCA_HIP(hipGetLastError());
  sort_pairs(key2, keys, perm, list, m, bits_for((uint64_t)nb * (uint64_t)B), sort_tmp, s);
}

int harmony_slices(int64_t rows) { return (int)std::min<int64_t>(128, std::max<int64_t>(1, rows / 256)); }

template <typename T>
void harmony_sums(const T* x, int64_t ldx, int64_t m, int d, bool ones, const T* R, int K, const uint32_t* order, const int64_t* seg, int B,
                  int slices, double* partial, hipStream_t s) {
  const int D = d + (ones ? 1 : 0);
  const dim3 grid((unsigned)slices * blocks_for(D, kSumCols), blocks_for(K, kSumClusters), (unsigned)B);
  hipLaunchKernelGGL((hm_sums_kernel<T>), grid, dim3(256), 0, s, x, ldx, m, d, D, R, K, order, seg, slices, partial);
  SAPCA_HIP(hipGetLastError());
}

template <typename T>
void harmony_centroids(const double* partial, int K, int d, int slices, T* Y, hipStream_t s) {
  hipLaunchKernelGGL((hm_centroids_kernel<T>), dim3((unsigned)K), dim3(256), 0, s, partial, d, slices, Y);
  SAPCA_HIP(hipGetLastError());
}

void harmony_beta(const double* partial, int K, int B, int d, int slices, double lambda, double* beta, hipStream_t s) {
  hipLaunchKernelGGL(hm_beta_kernel, dim3((unsigned)K), dim3(256), 0, s, partial, K, B, d, slices, lambda, beta);
  SAPCA_HIP(hipGetLastError());
}

template <typename T>
void harmony_apply(const T* z, int64_t ldz, int64_t m, int d, const T* R, int K, const int32_t* batch, int B, const double* beta, T* out,
                   int64_t ldc, hipStream_t s) {
  if (m <= 0) return;
  hipLaunchKernelGGL((hm_apply_kernel<T>), dim3(std::min(blocks_for(m * d, 256), 1u << 20)), dim3(256), 0, s, z, ldz, m, d, R, K, batch, B, beta, out, ldc);
  SAPCA_HIP(hipGetLastError());
}

template <typename T>
void harmony_totals(const T* R, int64_t m, int K, const uint32_t* by_batch, const int64_t* seg, int B, int slices, double* colsum, double* O,
                    double* rs, hipStream_t s) {
  hipLaunchKernelGGL((hm_colsum_kernel<T>), dim3((unsigned)slices, blocks_for(K, kSumCols), (unsigned)B), dim3(256), 0, s, R, m, K, by_batch, seg,
                     slices, colsum);
  SAPCA_HIP(hipGetLastError());
  hipLaunchKernelGGL(hm_totals_kernel, dim3(blocks_for(K, 256)), dim3(256), 0, s, colsum, K, B, slices, O, rs);
  SAPCA_HIP(hipGetLastError());
}

template <typename T>
void harmony_fold(const T* R, int64_t m, int K, int B, int64_t nb, int64_t add, int64_t remove, const uint64_t* keys, const uint32_t* list,
                  const double* Pr, double theta, double* O, double* rs, double* pen, hipStream_t s) {
  hipLaunchKernelGGL((hm_fold_kernel<T>), dim3(blocks_for(K, kFoldClusters)), dim3(kFoldThreads), 0, s, R, m, K, B, nb, add, remove, keys, list, Pr, theta,
                     O, rs, pen);
  SAPCA_HIP(hipGetLastError());
}

template <typename T>
void harmony_block(const T* zc, int64_t ldz, int64_t m, int d, const T* Y, int K, const int32_t* batch, int B, const uint32_t* list, int64_t p0,
                   int64_t n, const double* pen, double sigma, T* R, T* dist, hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL((hm_block_kernel<T>), dim3(blocks_for(n, 64)), dim3(kKnnThreads), 0, s, zc, ldz, m, d, Y, K, batch, B, list, p0, n, pen,
                     sigma, R, dist);
  SAPCA_HIP(hipGetLastError());
}

int64_t harmony_block_begin(int64_t j, int64_t m, int64_t nb) { return hm_block_begin(j, m, nb); }

template <typename T>
void harmony_objective(const T* R, const T* dist, const int32_t* batch, int64_t m, int K, int B, const double* O, const double* rs,
                       const double* Pr, double sigma, double theta, double* rowd, hipStream_t s) {
  if (m <= 0) return;
  hipLaunchKernelGGL((hm_objective_kernel<T>), dim3(blocks_for(m, 4)), dim3(256), 0, s, R, dist, batch, m, K, B, O, rs, Pr, sigma, theta, rowd);
  SAPCA_HIP(hipGetLastError());
}

#define SAPCA_INSTANTIATE_HARMONY(T)                                                                                                      \
  template void harmony_unit_rows<T>(const T*, int64_t, int64_t, int, T*, int64_t, hipStream_t);                                          \
  template void harmony_sums<T>(const T*, int64_t, int64_t, int, bool, const T*, int, const uint32_t*, const int64_t*, int, int, double*, \
                                hipStream_t);                                                                                             \
  template void harmony_centroids<T>(const double*, int, int, int, T*, hipStream_t);                                                      \
  template void harmony_apply<T>(const T*, int64_t, int64_t, int, const T*, int, const int32_t*, int, const double*, T*, int64_t,         \
                                 hipStream_t);                                                                                            \
  template void harmony_totals<T>(const T*, int64_t, int, const uint32_t*, const int64_t*, int, int, double*, double*, double*,           \
                                  hipStream_t);                                                                                           \
  template void harmony_fold<T>(const T*, int64_t, int, int, int64_t, int64_t, int64_t, const uint64_t*, const uint32_t*, const double*,  \
                                double, double*, double*, double*, hipStream_t);                                                          \
  template void harmony_block<T>(const T*, int64_t, int64_t, int, const T*, int, const int32_t*, int, const uint32_t*, int64_t, int64_t,  \
                                 const double*, double, T*, T*, hipStream_t);                                                             \
  template void harmony_objective<T>(const T*, const T*, const int32_t*, int64_t, int, int, const double*, const double*, const double*,  \
                                     double, double, double*, hipStream_t);
SAPCA_INSTANTIATE_HARMONY(float)
SAPCA_INSTANTIATE_HARMONY(double)
#undef SAPCA_INSTANTIATE_HARMONY

}  // namespace k
}  // namespace sapca
