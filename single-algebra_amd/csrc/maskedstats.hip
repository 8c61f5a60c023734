// Masked and stored-entry row statistics on a device-resident CSR, the ROW direction of
//   MatrixNonZero::nonzero_row_masked     src/sparse/csr.rs:188-252 of the reference
//   MatrixSum::sum_row_masked             csr.rs:490-556
//   MatrixVariance::var_row_masked        csr.rs:864-914  (and var_row_chunk, csr.rs:773-813: every column kept)
// and, on A^T with the row mask as the column mask, the COLUMN direction's fallback when the exact column accumulators
// (upstats.hip) cannot serve it.  One wave per row; no LDS, no atomics: the result depends only on the row's entries.
#include "kernels.h"

namespace sapca {
namespace k {

namespace {

constexpr int WAVE = 64;
constexpr int WAVES = 4;    // waves (rows in flight) per 256-thread workgroup
constexpr int TILE = 16;    // values per lane held in registers: rows of up to 1,024 entries are read once

// The column mask is a bitset read from global memory (L1 / L2 hold it: 2.5 KB at 20,000 columns), so any width works.
__device__ inline bool kept(const uint32_t* __restrict__ bits, int32_t c) { return (bits[c >> 5] >> (c & 31)) & 1u; }

__device__ inline double wave_sum(double x) {
#pragma unroll
  for (int off = WAVE / 2; off > 0; off >>= 1) x += __shfl_xor(x, off);
  return x;
}

// Row r: count, sum and sum of squares of the kept stored entries, then sum (x - mean)^2 over them (the reference's
// second pass, csr.rs:889-911) from the register tile, or from a re-read of the row (cache) when it is longer than
// the tile.  bits == nullptr keeps every entry and reads no column index.
template <typename T>
__global__ void __launch_bounds__(WAVE * WAVES) masked_row_stats_kernel(const int64_t* __restrict__ ptr, const int32_t* __restrict__ idx,
                                                                       const T* __restrict__ val, int64_t rows,
                                                                       const uint32_t* __restrict__ bits, double* __restrict__ out_sum,
                                                                       double* __restrict__ out_sumsq, double* __restrict__ out_m2,
                                                                       uint32_t* __restrict__ out_cnt) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int64_t r = (int64_t)blockIdx.x * WAVES + threadIdx.x / WAVE;
  if (r >= rows) return;   // (wave-uniform)
  const int64_t e0 = ptr[r];
  const int64_t len = ptr[r + 1] - e0;
  const T* v = val + e0;
  const int32_t* c = idx + e0;
  const bool in_regs = len <= (int64_t)TILE * WAVE;
  T tile[TILE];
  uint32_t keep = 0;   // bit j: tile[j] is a kept entry
  double s = 0.0, q = 0.0, n = 0.0;
  if (in_regs) {
#pragma unroll
    for (int j = 0; j < TILE; ++j) {
      const int64_t e = lane + (int64_t)j * WAVE;
      const bool k = e < len && (bits == nullptr || kept(bits, c[e]));
      tile[j] = k ? v[e] : (T)0;
      keep |= (uint32_t)k << j;
      const double x = (double)tile[j];
      s += k ? x : 0.0;
      q += k ? x * x : 0.0;
      n += k ? 1.0 : 0.0;
    }
  } else {
#pragma unroll
    for (int j = 0; j < TILE; ++j) tile[j] = (T)0;
    for (int64_t e = lane; e < len; e += WAVE) {
      if (bits != nullptr && !kept(bits, c[e])) continue;
      const double x = (double)v[e];
      s += x;
      q += x * x;
      n += 1.0;
    }
  }
  s = wave_sum(s);
  q = wave_sum(q);
  n = wave_sum(n);
  const double mean = n > 0.0 ? s / n : 0.0;
  double d2 = 0.0;
  if (in_regs) {
#pragma unroll
    for (int j = 0; j < TILE; ++j) {
      const double d = (double)tile[j] - mean;
      d2 += (keep >> j) & 1u ? d * d : 0.0;
    }
  } else {
    for (int64_t e = lane; e < len; e += WAVE) {
      if (bits != nullptr && !kept(bits, c[e])) continue;
      const double d = (double)v[e] - mean;
      d2 += d * d;
    }
  }
  d2 = wave_sum(d2);
  if (lane == 0) {
    if (out_sum) out_sum[r] = s;
    if (out_sumsq) out_sumsq[r] = q;
    if (out_m2) out_m2[r] = d2;
    if (out_cnt) out_cnt[r] = (uint32_t)n;
  }
}

}  // namespace

template <typename T>
void masked_row_stats(const CsrView<T>& A, const uint32_t* col_bits, double* sum, double* sumsq, double* m2, uint32_t* cnt,
                      hipStream_t s) {
  if (A.rows == 0) return;
  const int64_t blocks = (A.rows + WAVES - 1) / WAVES;
  SAPCA_CHECK(blocks < ((int64_t)1 << 31), SAPCA_ERR_ARG, "masked_row_stats: too many rows");
  hipLaunchKernelGGL((masked_row_stats_kernel<T>), dim3((unsigned)blocks), dim3(WAVE * WAVES), 0, s, A.ptr, A.idx, A.val, A.rows,
                     col_bits, sum, sumsq, m2, cnt);
  SAPCA_HIP(hipGetLastError());
}

#define INSTANTIATE(T) \
  template void masked_row_stats<T>(const CsrView<T>&, const uint32_t*, double*, double*, double*, uint32_t*, hipStream_t);
INSTANTIATE(float)
INSTANTIATE(double)
#undef INSTANTIATE

}  // namespace k
}  // namespace sapca
