// Per-batch statistics and top-n row sums on a device-resident CSR (the reference's last three CSR traits):
//   BatchMatrixVariance::var_batch_row / var_batch_col   src/sparse/csr.rs:1081-1245 of the reference
//   BatchMatrixMean::mean_batch_row / mean_batch_col     csr.rs:1248-1344
//   MatrixNTop::sum_row_n_top                            csr.rs:1347-1376
// Both kernels give one wave to a row of the operand R and keep everything the row needs in that wave's own LDS, so
// no workgroup barrier and no global atomic is involved; lanes of a wave meet only in LDS, ordered by wave fences.
#include "kernels.h"
#include "value_keys.h"

namespace sapca {
namespace k {

namespace {

constexpr int WAVE = 64;
constexpr int WAVES = 4;   // waves (rows in flight) per 256-thread workgroup

// Codes one launch of the labelled statistics holds: 20 bytes of LDS per code and wave (f64 sum, f64 sum of squared
// deviations, u32 count), 4 waves per workgroup -> 80 KiB per workgroup at 1,024 codes, so 2 workgroups (8 waves) share a
// CU's 160 KiB at the largest launch; a launch with fewer codes sizes its LDS to them (3 codes: 240 B per workgroup, the
// occupancy is then set by the registers: 30 / 32 VGPRs in f32 / f64, no scratch, 8 waves per SIMD).  More codes than
// this take ceil(n_batches / 1,024) launches over code ranges.
constexpr int kBatchCodesPerLaunch = 1024;

// orders this wave's LDS accesses before / after the point: every lane sees what the others wrote above it
__device__ inline void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
}

// ---- labelled row statistics -------------------------------------------------------------------------------------
// Row r of R, codes[idx[e]] in [lo, lo + nb): count, sum and sum of squared deviations from the row's per-code mean of
// the stored entries, the reference's two passes (csr.rs:1118-1160: the sum, then sum (x - mean)^2 over a second read of
// the row, which is in the cache by then).  Wave w of a workgroup owns the slots lds_sum[w][.], lds_m2[w][.],
// lds_cnt[w][.] (nb each: 20 bytes per code).  out_* are [nb][rows] (code-major, the layout of the host result).
template <typename T>
__global__ void __launch_bounds__(WAVE * WAVES) batch_row_stats_kernel(const int64_t* __restrict__ ptr, const int32_t* __restrict__ idx,
                                                                      const T* __restrict__ val, int64_t rows,
                                                                      const int32_t* __restrict__ codes, int lo, int nb,
                                                                      double* __restrict__ out_sum, double* __restrict__ out_m2,
                                                                      uint32_t* __restrict__ out_cnt) {
  extern __shared__ double lds_bs[];
  const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
  double* sum = lds_bs + (size_t)w * nb;
  double* m2 = lds_bs + (size_t)(WAVES + w) * nb;
  uint32_t* cnt = reinterpret_cast<uint32_t*>(lds_bs + (size_t)2 * WAVES * nb) + (size_t)w * nb;
  const int64_t r = (int64_t)blockIdx.x * WAVES + w;
  if (r >= rows) return;   // (wave-uniform)
  for (int b = lane; b < nb; b += WAVE) {
    sum[b] = 0.0;
    m2[b] = 0.0;
    cnt[b] = 0u;
  }
  wave_sync();
  const int64_t e0 = ptr[r], e1 = ptr[r + 1];
  for (int64_t e = e0 + lane; e < e1; e += WAVE) {
    const int b = codes[idx[e]] - lo;
    if ((unsigned)b < (unsigned)nb) {
      atomicAdd(&sum[b], (double)val[e]);
      atomicAdd(&cnt[b], 1u);
    }
  }
  wave_sync();
  for (int b = lane; b < nb; b += WAVE) {   // the slot's sum becomes its mean (csr.rs:1133-1138)
    const uint32_t c = cnt[b];
    const double s = sum[b];
    out_sum[(int64_t)b * rows + r] = s;
    out_cnt[(int64_t)b * rows + r] = c;
    sum[b] = c > 0 ? s / (double)c : 0.0;
  }
  wave_sync();
  for (int64_t e = e0 + lane; e < e1; e += WAVE) {
    const int b = codes[idx[e]] - lo;
    if ((unsigned)b < (unsigned)nb) {
      const double d = (double)val[e] - sum[b];
      atomicAdd(&m2[b], d * d);
    }
  }
  wave_sync();
  for (int b = lane; b < nb; b += WAVE) out_m2[(int64_t)b * rows + r] = m2[b];
}

// ---- top-n row sums --------------------------------------------------------------------------------------------------
// (the keys the select runs on: Keys<T> of value_keys.h, the order-preserving unsigned image of a value)
constexpr int DIGIT = 8, BINS = 1 << DIGIT;   // radix digits: 4 passes (f32) / 8 (f64), a 1 KiB histogram per wave
constexpr int TILE = 16;                        // values per lane held in registers: rows up to 1,024 entries are read once
// (row_top_n_kernel: 87 / 106 VGPRs in f32 / f64, no scratch, 4 KiB of LDS per workgroup: 5 / 4 waves per SIMD)

// out[i * rows + r] = sum of the min(ns[i], len) largest stored values of row r (csr.rs:1347-1376), f64 accumulation.
// For n < len a most-significant-digit radix select finds the key kt of the n-th largest value and k, how many of the n
// carry exactly kt; then sum = sum_{key > kt} x + k * value(kt).  Every n of the call shares the row's register tile and
// the row total; a row longer than the tile is re-read from global memory (L2) in every pass.
template <typename T>
__global__ void __launch_bounds__(WAVE * WAVES) row_top_n_kernel(const int64_t* __restrict__ ptr, const T* __restrict__ val, int64_t rows,
                                                                 const uint64_t* __restrict__ ns, int n_ns, double* __restrict__ out) {
  using KT = Keys<T>;
  using K = typename KT::K;
  __shared__ uint32_t hist_all[WAVES][BINS];
  const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
  uint32_t* hist = hist_all[w];
  const int64_t r = (int64_t)blockIdx.x * WAVES + w;
  if (r >= rows) return;   // (wave-uniform)
  const int64_t e0 = ptr[r];
  const int64_t len = ptr[r + 1] - e0;
  const T* v = val + e0;
  const bool in_regs = len <= (int64_t)TILE * WAVE;
  T tile[TILE];
  double total = 0.0;
  if (in_regs) {
#pragma unroll
    for (int j = 0; j < TILE; ++j) {
      const int64_t e = lane + (int64_t)j * WAVE;
      tile[j] = e < len ? v[e] : (T)0;
      total += e < len ? (double)tile[j] : 0.0;
    }
  } else {
#pragma unroll
    for (int j = 0; j < TILE; ++j) tile[j] = (T)0;
    for (int64_t e = lane; e < len; e += WAVE) total += (double)v[e];
  }
  // f(x) for every stored value of the row held by this lane
  auto each = [&](auto&& f) {
    if (in_regs) {
#pragma unroll
      for (int j = 0; j < TILE; ++j)
        if (lane + (int64_t)j * WAVE < len) f(tile[j]);
    } else {
      for (int64_t e = lane; e < len; e += WAVE) f(v[e]);
    }
  };
  bool row_total_reduced = false;
  for (int i = 0; i < n_ns; ++i) {
    const uint64_t n = ns[i];
    double res;
    if ((uint64_t)len <= n) {   // csr.rs:1364-1365: all of them
      if (!row_total_reduced) {
#pragma unroll
        for (int off = WAVE / 2; off > 0; off >>= 1) total += __shfl_xor(total, off);
        row_total_reduced = true;
      }
      res = total;
    } else if (n == 0) {
      res = 0.0;
    } else {
      K prefix = 0;                 // the digits of kt found so far
      uint32_t k = (uint32_t)n;     // rank still wanted among the keys that carry `prefix` (1-based, from the top)
#pragma unroll 1
      for (int shift = KT::BITS - DIGIT; shift >= 0; shift -= DIGIT) {
        for (int b = lane; b < BINS; b += WAVE) hist[b] = 0u;
        wave_sync();
        const K hi_mask = shift + DIGIT >= KT::BITS ? (K)0 : ~(K)0 << (shift + DIGIT);
        each([&](T x) {
          const K key = KT::key(x);
          if ((key & hi_mask) == prefix) atomicAdd(&hist[(uint32_t)(key >> shift) & (BINS - 1)], 1u);
        });
        wave_sync();
        // lane l holds bins 255 - 4l .. 252 - 4l (descending): a wave scan finds the bin the k-th key falls into
        uint32_t h[BINS / WAVE], own = 0;
#pragma unroll
        for (int j = 0; j < BINS / WAVE; ++j) {
          h[j] = hist[BINS - 1 - (BINS / WAVE) * lane - j];
          own += h[j];
        }
        uint32_t incl = own;
#pragma unroll
        for (int off = 1; off < WAVE; off <<= 1) {
          const uint32_t t = __shfl_up(incl, off);
          if (lane >= off) incl += t;
        }
        const uint32_t excl = incl - own;
        const unsigned long long hit = __ballot(excl < k && k <= incl);
        const int src = __ffsll((long long)hit) - 1;
        uint32_t digit = 0, k_left = 0, c = excl;
#pragma unroll
        for (int j = 0; j < BINS / WAVE; ++j) {
          if (k_left == 0 && c + h[j] >= k) {
            digit = BINS - 1 - (BINS / WAVE) * lane - j;
            k_left = k - c;
          }
          c += h[j];
        }
        digit = __shfl(digit, src);
        k = __shfl(k_left, src);
        prefix |= (K)digit << shift;
        wave_sync();   // (the histogram is cleared for the next digit only after every lane has read it)
      }
      // prefix = kt; k of the n selected values equal value(kt), the other n - k are the keys above it
      const T t = KT::value(prefix);
      double above = 0.0;
      each([&](T x) {
        if (KT::key(x) > prefix) above += (double)x;
      });
#pragma unroll
      for (int off = WAVE / 2; off > 0; off >>= 1) above += __shfl_xor(above, off);
      res = above + (double)k * (double)t;
    }
    if (lane == 0) out[(int64_t)i * rows + r] = res;
  }
}

}  // namespace

int batch_codes_per_launch() { return kBatchCodesPerLaunch; }

template <typename T>
void batch_row_stats(const CsrView<T>& R, const int32_t* codes, int lo, int nb, double* sum, double* m2, uint32_t* cnt, hipStream_t s) {
  if (R.rows == 0 || nb == 0) return;
  SAPCA_CHECK(nb <= kBatchCodesPerLaunch, SAPCA_ERR_ARG, "batch_row_stats: more codes than one launch holds");
  const size_t lds = (size_t)WAVES * nb * (2 * sizeof(double) + sizeof(uint32_t));
  static LdsAttrState attr;
  ensure_dynamic_lds(reinterpret_cast<const void*>(&batch_row_stats_kernel<T>), lds, attr);
  const int64_t blocks = (R.rows + WAVES - 1) / WAVES;
  SAPCA_CHECK(blocks < ((int64_t)1 << 31), SAPCA_ERR_ARG, "batch_row_stats: too many rows");
  hipLaunchKernelGGL((batch_row_stats_kernel<T>), dim3((unsigned)blocks), dim3(WAVE * WAVES), lds, s, R.ptr, R.idx, R.val, R.rows, codes,
                     lo, nb, sum, m2, cnt);
  SAPCA_HIP(hipGetLastError());
}

template <typename T>
void row_top_n(const CsrView<T>& A, const uint64_t* ns, int n_ns, double* out, hipStream_t s) {
  if (A.rows == 0 || n_ns == 0) return;
  const int64_t blocks = (A.rows + WAVES - 1) / WAVES;
  SAPCA_CHECK(blocks < ((int64_t)1 << 31), SAPCA_ERR_ARG, "row_top_n: too many rows");
  hipLaunchKernelGGL((row_top_n_kernel<T>), dim3((unsigned)blocks), dim3(WAVE * WAVES), 0, s, A.ptr, A.val, A.rows, ns, n_ns, out);
  SAPCA_HIP(hipGetLastError());
}

#define INSTANTIATE(T)                                                                                                        \
  template void batch_row_stats<T>(const CsrView<T>&, const int32_t*, int, int, double*, double*, uint32_t*, hipStream_t);  \
  template void row_top_n<T>(const CsrView<T>&, const uint64_t*, int, double*, hipStream_t);
INSTANTIATE(float)
INSTANTIATE(double)
#undef INSTANTIATE

}  // namespace k
}  // namespace sapca
