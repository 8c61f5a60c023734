// What the dense tall-skinny panel units share: gram.hip, chol.hip, panel_gemm.hip, sym_eig.hip, panel_ops.hip.
//
// They are the normaliser (R10) and the small-SVD step (R11) of the randomized SVD
// (single_svdlib::randomized::randomized_svd, call sites: the reference's src/dimred/pca/sparse/mod.rs:170-180).  The
// reference's dependency does a serial Householder QR of every m x l panel; any orthonormal basis of the same span gives
// the same final result, so the panel step here is CholeskyQR2:
//     G = P^T P   (gram.hip: MFMA, f64 accumulate)  ->  R = chol(G), R^-1  (chol.hip: one workgroup, f64)
//     P <- P R^-1 (panel_gemm.hip: MFMA panel GEMM) ... twice.
// MFMA is used only in these three: they are the path's only dense contractions.
//
// v_mfma_f64_16x16x4_f64 lane maps (gfx950): A[i = lane&15][k = lane>>4], B[k = lane>>4][j = lane&15],
// D: col = lane&15, row = (lane>>4) + 4*reg.
#pragma once
#include "kernels.h"

#include <type_traits>

namespace sapca {
namespace k {

namespace {

constexpr int WAVE = 64;
typedef double d4 __attribute__((ext_vector_type(4)));

__device__ inline d4 mfma_f64(double a, double b, d4 c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }

// 16-byte loads of four consecutive panel elements: Four keeps the panel's type (and stores), Quad widens to f64
template <typename T> struct Four;
template <> struct Four<float> {
  __device__ static inline void load(const float* p, float out[4]) {
    const float4 v = *reinterpret_cast<const float4*>(p);
    out[0] = v.x; out[1] = v.y; out[2] = v.z; out[3] = v.w;
  }
  __device__ static inline void store(float* p, const float v[4]) { *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]); }
};
template <> struct Four<double> {
  __device__ static inline void load(const double* p, double out[4]) {
    const double2 a = *reinterpret_cast<const double2*>(p);
    const double2 b = *reinterpret_cast<const double2*>(p + 2);
    out[0] = a.x; out[1] = a.y; out[2] = b.x; out[3] = b.y;
  }
  __device__ static inline void store(double* p, const double v[4]) {
    *reinterpret_cast<double2*>(p) = make_double2(v[0], v[1]);
    *reinterpret_cast<double2*>(p + 2) = make_double2(v[2], v[3]);
  }
};

template <typename T> struct Quad;
template <> struct Quad<float> {
  __device__ static inline void load(const float* p, double out[4]) {
    const float4 v = *reinterpret_cast<const float4*>(p);
    out[0] = v.x; out[1] = v.y; out[2] = v.z; out[3] = v.w;
  }
};
template <> struct Quad<double> {
  __device__ static inline void load(const double* p, double out[4]) {
    const double2 a = *reinterpret_cast<const double2*>(p);
    const double2 b = *reinterpret_cast<const double2*>(p + 2);
    out[0] = a.x; out[1] = a.y; out[2] = b.x; out[3] = b.y;
  }
};

inline int grid_for(int64_t work_items, int block, int cap = 4096) {
  int64_t g = (work_items + block - 1) / block;
  if (g < 1) g = 1;
  if (g > cap) g = cap;
  return (int)g;
}

// A runtime count of 16-column tiles -> a compile-time one: f(std::integral_constant<int, N>) for the N of the list that
// equals n (the last of the list where none does: the callers have checked the width).  Instantiates f for the listed N only.
template <int N, int... Rest, typename F>
void with_tile_count(int n, F&& f) {
  if constexpr (sizeof...(Rest) == 0) f(std::integral_constant<int, N>{});
  else if (n == N) f(std::integral_constant<int, N>{});
  else with_tile_count<Rest...>(n, f);
}

}  // namespace

}  // namespace k
}  // namespace sapca
