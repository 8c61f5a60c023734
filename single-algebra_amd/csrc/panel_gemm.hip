// out = P M for a tall-skinny panel P and a small f64 factor M kept in LDS (step three of the CholeskyQR2 normaliser, where
// M = R^-1, and the projections; dense_common.h has the scheme and the MFMA lane maps).
#include "dense_common.h"

#include <algorithm>

namespace sapca {
namespace k {

namespace {

// out[16-row tile] = P[tile] * M.  Lane (i = lane&15, g = lane>>4) loads the 16-byte segments
// P[r0+i][16j+4g .. +3]; k-slot g of MFMA step (j, e) is panel column 16j+4g+e on both operands.
template <typename T, int NTO, int THREADS = 256>
__global__ void __launch_bounds__(THREADS, THREADS == 512 ? 4 : 1)   // (512 threads: four waves per SIMD, 128 registers)
panel_gemm_kernel(const T* P, int64_t rows, int ld, const double* __restrict__ M, int ldo, T* out, int ldp_stride, int ldm_stride,
                  int ldo_stride, int accumulate, int upper, int ncols_out) {
  // P: rows x ld at row stride ldp_stride; M: ld x ldo at row stride ldm_stride; out: rows x ldo at row stride ldo_stride
  // (only the first ncols_out columns are written: the projection's m x k output has row stride k, not a multiple of 16)
  // (the wide-panel driver below walks 128-column blocks of a bigger product with these; accumulate: out += P M;
  //  upper > 0: M is (a block column of) an upper triangular matrix -- the normaliser's R^-1 -- whose 16 x 16 blocks below the
  //  diagonal are skipped: output tile tb stands upper - 1 tiles to the right of K tile 0's diagonal block.  10 of 16
  //  block products at 64 columns, 36 of 64 at 128, where this kernel is bound by the f64 MFMA rate)
  extern __shared__ double Ms[];  // ld x ldo
  {
    // eight loads of the factor in flight per thread (two round trips at 64 columns, not sixteen), no division where M is dense
    const int nel = ld * ldo, step = blockDim.x;
    const bool dense = ldm_stride == ldo;
    auto at = [&](int i) { return dense ? i : (i / ldo) * ldm_stride + (i % ldo); };
    int i = threadIdx.x;
    for (; i + 7 * step < nel; i += 8 * step) {
      double v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = M[at(i + u * step)];
#pragma unroll
      for (int u = 0; u < 8; ++u) Ms[i + u * step] = v[u];
    }
    for (; i < nel; i += step) Ms[i] = M[at(i)];
  }
  __syncthreads();
  const int lane = threadIdx.x & (WAVE - 1);
  const int wave = threadIdx.x / WAVE;
  const int i = lane & 15, g = lane >> 4;
  const int nt = ld / 16;
  const int64_t ntiles = (rows + 15) / 16;
  constexpr int WPB = THREADS / WAVE;   // waves (= 16-row tiles in flight) per workgroup
  for (int64_t tile = (int64_t)blockIdx.x * WPB + wave; tile < ntiles; tile += (int64_t)gridDim.x * WPB) {
    const int64_t r0 = tile * 16;
    const bool row_ok = r0 + i < rows;
    const T* prow = P + (row_ok ? (r0 + i) : 0) * ldp_stride + 4 * g;
    d4 acc[NTO];
#pragma unroll
    for (int tb = 0; tb < NTO; ++tb) acc[tb] = d4{0, 0, 0, 0};
    for (int j = 0; j < nt; ++j) {
      double a4[4] = {0, 0, 0, 0};
      if (row_ok) Quad<T>::load(prow + 16 * j, a4);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const double* brow = Ms + (16 * j + 4 * g + e) * ldo + i;
#pragma unroll
        for (int tb = 0; tb < NTO; ++tb)
          if (!upper || tb + upper - 1 >= j) acc[tb] = mfma_f64(a4[e], brow[16 * tb], acc[tb]);
      }
    }
#pragma unroll
    for (int tb = 0; tb < NTO; ++tb)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int64_t r = r0 + g + 4 * reg;
        if (r < rows && 16 * tb + i < ncols_out) {
          T* o = out + r * ldo_stride + 16 * tb + i;
          *o = accumulate ? (T)((double)*o + acc[tb][reg]) : (T)acc[tb][reg];
        }
      }
  }
}

template <typename T, int NTO>
void launch_panel_gemm(const T* P, int64_t rows, int ld, const double* M, int ldo, T* out, hipStream_t s, int ldp_stride = 0,
                       int ldm_stride = 0, int ldo_stride = 0, int accumulate = 0, int upper = 0, int ncols_out = 0) {
  if (ncols_out <= 0 || ncols_out > ldo) ncols_out = ldo;
  if (!ldp_stride) ldp_stride = ld;
  if (!ldm_stride) ldm_stride = ldo;
  if (!ldo_stride) ldo_stride = ldo;
  const size_t lds = (size_t)ld * ldo * sizeof(double);
  const int64_t ntiles = (rows + 15) / 16;
  // THREADS / 64 tiles per workgroup, at least one workgroup, at most max_blocks
  auto launch = [&](auto threads, int max_blocks) {
    constexpr int THREADS = decltype(threads)::value, WPB = THREADS / WAVE;
    static LdsAttrState attr;
    if (lds > 48 * 1024) ensure_dynamic_lds(reinterpret_cast<const void*>(&panel_gemm_kernel<T, NTO, THREADS>), lds, attr);
    const int blocks = (int)std::min<int64_t>(std::max<int64_t>((ntiles + WPB - 1) / WPB, 1), max_blocks);
    hipLaunchKernelGGL((panel_gemm_kernel<T, NTO, THREADS>), dim3(blocks), dim3(THREADS), lds, s, P, rows, ld, M, ldo, out, ldp_stride, ldm_stride,
                       ldo_stride, accumulate, upper, ncols_out);
  };
  if constexpr (NTO >= 7) {
    // M above 80 KiB of LDS leaves one workgroup per CU: twelve waves then instead of four (three per SIMD at 160 VGPRs),
    // or the kernel sits on one tile's HBM round trip per SIMD at a time (1.7 ms on C5's 2M x 128 panel)
    if (lds > 80 * 1024) return launch(std::integral_constant<int, 768>{}, 256);
  }
  if constexpr (NTO == 4) {
    // the 64-column panels of the headline configurations: eight waves per workgroup under a 128-register bound (the
    // 256-thread build takes 228 VGPRs: two waves per SIMD, and the kernel waits on one tile's round trip after another)
    // From 1024 tiles on (below, a grid of eight-tile workgroups covers less than half of the CUs).  The n-side panel of the
    // headline (1250 tiles) takes 8 us here against 17 us on the 256-thread build; the m-side one (12500 tiles) is no
    // faster with 512 workgroups that loop longer than with these 1024.
    if (ntiles >= 1024) return launch(std::integral_constant<int, 512>{}, 1024);
  }
  launch(std::integral_constant<int, 256>{}, 1024);
}

}  // namespace

template <typename T>
void panel_gemm(const T* P, int64_t rows, int ld, const double* M, int ldo, T* out, hipStream_t s, bool upper, int out_stride, int out_cols) {
  if (out_stride <= 0) out_stride = ldo;
  if (out_cols <= 0 || out_cols > ldo) out_cols = ldo;
  SAPCA_CHECK(ld % 16 == 0 && ldo % 16 == 0 && ldo >= 16 && ld <= kMaxPanelWidth && ldo <= kMaxPanelWidth, SAPCA_ERR_ARG,
              "panel_gemm: unsupported panel width");
  if (rows == 0) return;
  if (ld > 128 || ldo > 128) {
    // wide: out[:, J] = sum_I P[:, I] M[I, J] over blocks of at most 128 columns, one launch per (I, J), accumulating over I
    // (`upper`: M is upper triangular, the blocks below its diagonal are skipped).  Never in place.
    SAPCA_CHECK(out != P, SAPCA_ERR_ARG, "panel_gemm: wide panels are not multiplied in place");
    for (int j0 = 0; j0 < ldo; j0 += 128) {
      const int nd = std::min(128, ldo - j0);
      if (out_cols <= j0) break;
      bool first = true;
      for (int i0 = 0; i0 < ld; i0 += 128) {
        const int kd = std::min(128, ld - i0);
        if (upper && i0 >= j0 + nd) break;
        const int nco = std::min(nd, out_cols - j0);
        const int acc = first ? 0 : 1;
        const int diag = (upper && i0 == j0) ? 1 : 0;   // (a diagonal block of an upper triangular M is upper triangular itself)
        first = false;
        const T* Pb = P + i0;
        const double* Mb = M + (size_t)i0 * ldo + j0;
        T* ob = out + j0;
        with_tile_count<1, 2, 3, 4, 5, 6, 7, 8>(nd / 16, [&](auto nto) {
          launch_panel_gemm<T, decltype(nto)::value>(Pb, rows, kd, Mb, nd, ob, s, ld, ldo, out_stride, acc, diag, nco);
        });
      }
    }
    SAPCA_HIP(hipGetLastError());
    return;
  }
  SAPCA_CHECK(out != P || (ldo == ld && out_stride == ldo), SAPCA_ERR_ARG, "panel_gemm: in-place needs ldo == ld");
  with_tile_count<1, 2, 3, 4, 5, 6, 7, 8>(ldo / 16, [&](auto nto) {
    launch_panel_gemm<T, decltype(nto)::value>(P, rows, ld, M, ldo, out, s, 0, 0, out_stride, 0, upper ? 1 : 0, out_cols);
  });
  SAPCA_HIP(hipGetLastError());
}

template void panel_gemm<float>(const float*, int64_t, int, const double*, int, float*, hipStream_t, bool, int, int);
template void panel_gemm<double>(const double*, int64_t, int, const double*, int, double*, hipStream_t, bool, int, int);

}  // namespace k
}  // namespace sapca
