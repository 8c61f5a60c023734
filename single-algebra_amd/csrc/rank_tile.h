// The pieces of the matrix-core ranking kernels (knn.hip's selection, kmeans.hip's assignment): the tile geometry, the
// v_mfma_f32_16x16x4_f32 / v_mfma_f64_16x16x4_f64 wrappers with their result layouts, the ranking key, the loads of a
// panel chunk into registers / LDS, and the compensated f64 sums of the passes that recompute values from the rows.  Device code; include from a .hip file.
#pragma once
#include <climits>

#include "kernels.h"

namespace sapca {
namespace k {

constexpr int kKnnThreads = 256;   // 4 waves
constexpr int kKnnTile = 64;       // corpus rows per tile
constexpr int kKnnEmpty = INT_MAX; // index of a list slot that was never filled

template <typename T> struct KnnChunk;   // columns of d per LDS chunk
template <> struct KnnChunk<float> { static constexpr int value = 64; };
template <> struct KnnChunk<double> { static constexpr int value = 32; };

using f32x4 = __attribute__((ext_vector_type(4))) float;
using f64x4 = __attribute__((ext_vector_type(4))) double;
template <typename T> struct KnnAcc;
template <> struct KnnAcc<float> { using type = f32x4; };
template <> struct KnnAcc<double> { using type = f64x4; };

__device__ inline f32x4 knn_mfma(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
__device__ inline f64x4 knn_mfma(double a, double b, f64x4 c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }
// row of the 16 x 16 result that register `reg` of lane `lane` holds (its column is lane & 15 in both forms)
template <typename T>
__device__ inline int acc_row(int lane, int reg) {
  if (sizeof(T) == 4) return (lane >> 4) * 4 + reg;
  return (lane >> 4) + 4 * reg;
}

// (s1, i1) ranks before (s2, i2): the higher score, then the lower index.  A NaN score ranks before nothing.
template <typename T>
__device__ inline bool knn_better(T s1, int i1, T s2, int i2) {
  return s1 > s2 || (s1 == s2 && i1 < i2);
}

// rows x KC elements of a panel chunk (columns k0 .. k0 + KC, zero beyond d and beyond the last row) into registers / LDS.
// Thread t takes column t % KC of rows t / KC + i * (256 / KC): one 32-bit lane offset (ld < 2^28, checked by the caller)
// on a base that is uniform per i, so the addresses cost scalar arithmetic and no registers across the sweep.
template <typename T, int ROWS, int KC>
__device__ inline void knn_chunk_load(const T* base, int64_t ld, int64_t row0, int64_t nrows, int k0, int d, T* regs) {
  constexpr int RPI = kKnnThreads / KC;   // rows per pass
  const int tr = (int)threadIdx.x / KC, tc = (int)threadIdx.x % KC;
  const unsigned voff = (unsigned)tr * (unsigned)ld + (unsigned)tc;
  const int64_t left = nrows - row0 - tr;   // rows tr + i * RPI below this exist
  const int rlim = k0 + tc < d ? (int)(left < ROWS ? (left > 0 ? left : 0) : ROWS) : 0;
#pragma unroll
  for (int i = 0; i < ROWS / RPI; ++i) {
    const T* rb = base + (row0 + i * RPI) * ld + k0;
    regs[i] = i * RPI < rlim ? rb[voff] : (T)0;
  }
}
template <typename T, int ROWS, int KC>
__device__ inline void knn_chunk_store(const T* regs, T* lds) {
#pragma unroll
  for (int i = 0; i < ROWS * KC / kKnnThreads; ++i) {
    const int e = (int)threadIdx.x + kKnnThreads * i;
    lds[(e / KC) * (KC + 4) + e % KC] = regs[i];
  }
}

// s + c <- s + c + x * y, the product and the sum without their rounding errors (Dekker / Knuth); contraction is off in these:
// fusing s + x * y would take the error term away from under the two-sum
__device__ inline void knn_acc_prod(double& s, double& c, double x, double y) {
#pragma clang fp contract(off)
  const double p = x * y;
  const double pe = fma(x, y, -p);
  const double t = s + p;
  const double bb = t - s;
  const double se = (s - (t - bb)) + (p - bb);
  s = t;
  c += se + pe;
}
__device__ inline void knn_acc_add(double& s, double& c, double x) {
#pragma clang fp contract(off)
  const double t = s + x;
  const double bb = t - s;
  c += (s - (t - bb)) + (x - bb);
  s = t;
}

}  // namespace k
}  // namespace sapca
