// Cholesky factor and its inverse of the l x l Gram matrix (step two of the CholeskyQR2 normaliser: dense_common.h has the
// scheme and the MFMA lane maps): three one-workgroup kernels, a host fallback for l > 128, and chol_inv() that picks.
#include "dense_common.h"

#include <algorithm>
#include <cmath>
#include <vector>

namespace sapca {
namespace k {

namespace {

// ---------------------------------------------------------------- Cholesky + inverse
// One workgroup of 256 threads, everything in LDS (f64).
//   Cholesky (upper, G = R^T R), right-looking: per pivot k one thread takes the square root, the
//   row is scaled, and all 256 threads apply the rank-1 update to the trailing upper triangle on a
//   16 x 16 thread grid (no integer division in the loop).
//   R^-1 by back substitution: column j is owned by 4 consecutive lanes that split the inner dot
//   product and combine with two DPP-class shuffles; the inverse is parked in the unused strict
//   lower triangle (Rinv[t][j], t < j, lives at a[j][t]) and its diagonal in dinv[].
// A pivot that falls below 1e-13 of the panel's scale (rank-deficient panel) is replaced by that
// floor and counted in *info; the direction it produces carries a ~zero singular value downstream.
__global__ void __launch_bounds__(256)
chol_inv_kernel(const double* __restrict__ G, int l, int ld, double* __restrict__ R, double* __restrict__ Rinv,
                int* __restrict__ info) {
  extern __shared__ double a[];  // l x (l+1) working copy + l diagonal inverses
  const int st = l + 1;
  double* dinv = a + (size_t)l * st;
  __shared__ int bad;
  __shared__ double floor_s;
  const int tid = threadIdx.x;
  const int ti = tid >> 4, tj = tid & 15;
  if (tid == 0) bad = 0;
  for (int i = tid; i < l * l; i += blockDim.x) a[(i / l) * st + (i % l)] = G[(i / l) * ld + (i % l)];
  __syncthreads();
  if (tid == 0) {
    double scale = 0;
    for (int i = 0; i < l; ++i) scale = fmax(scale, fabs(a[i * st + i]));
    floor_s = scale * 1e-13 + 1e-300;
  }
  __syncthreads();
  for (int kk = 0; kk < l; ++kk) {
    if (tid == 0) {
      double v = a[kk * st + kk];
      if (!(v > floor_s)) { v = floor_s; bad += 1; }
      v = sqrt(v);
      a[kk * st + kk] = v;
      dinv[kk] = 1.0 / v;
    }
    __syncthreads();
    const double inv = dinv[kk];
    for (int j = kk + 1 + tid; j < l; j += blockDim.x) a[kk * st + j] *= inv;
    __syncthreads();
    for (int i = kk + 1 + ti; i < l; i += 16) {
      const double ri = a[kk * st + i];
      for (int j = kk + 1 + tj; j < l; j += 16)
        if (j >= i) a[i * st + j] -= ri * a[kk * st + j];
    }
    __syncthreads();
  }
  // x = column j of R^-1: x_j = 1/R_jj, x_i = -(sum_{i<t<=j} R[i][t] x_t) / R_ii; 4 lanes per column
  for (int j0 = 0; j0 < l; j0 += 64) {
    const int j = j0 + (tid >> 2), part = tid & 3;
    const bool live = j < l;
    const int jj = live ? j : 0;
    for (int i = l - 1; i >= 0; --i) {   // uniform trip count so that the shuffles stay converged
      double s = 0;
      if (live && i < jj) {
        for (int t = i + 1 + part; t < jj; t += 4) s += a[i * st + t] * a[jj * st + t];
        if (part == 0) s += a[i * st + jj] * dinv[jj];
      }
      s += __shfl_xor(s, 1);
      s += __shfl_xor(s, 2);
      if (live && i < jj && part == 0) a[jj * st + i] = -s * dinv[i];
      // lanes of one column are in the same wave: the write above is visible to their next iteration
      __builtin_amdgcn_wave_barrier();
    }
  }
  __syncthreads();
  for (int i = tid; i < ld * ld; i += blockDim.x) {
    const int r = i / ld, c2 = i % ld;
    const bool in = r < l && c2 < l;
    R[i] = (in && c2 >= r) ? a[r * st + c2] : 0.0;
    Rinv[i] = !in ? 0.0 : (c2 > r ? a[c2 * st + r] : (c2 == r ? dinv[r] : 0.0));
  }
  if (tid == 0 && bad) atomicAdd(info, bad);
}

// The same factorisation for l <= 64 on one workgroup of four waves, blocked.  The matrix sits in LDS
// (row-major, pitch 65) padded to a multiple of 16 with a harmless diagonal.  Per 16-column block:
// wave 0 takes the block's columns into registers, lane = matrix row, and runs the right-looking
// elimination on them -- the pivot and the multipliers come from the lanes of the diagonal block through
// v_readlane, so the diagonal factorisation and the triangular solve of the rows below are the same 16
// unrolled steps (1/sqrt by Goldschmidt from v_rsq_f64: the divide would double the dependent chain) --
// while wave 1 inverts the previous diagonal block in registers; then the four waves apply the rank-16
// update to the trailing lower triangle as 16 x 16 block products on the matrix cores.
// L^-1, block row by block row:  X_ij = -X_ii (sum_k L_ik X_kj), one wave per block; the inner sum leaves
// the accumulator in exactly the lane layout the second product wants as its B operand.
// 24 us for l = 60 (tools/ubench/chol_phases.hip: 32k of the 54k cycles are the 64 pivots at ~80 instructions
// each, one wave's issue rate); a one-wave left-looking version with everything in LDS took 85 us.
__device__ __forceinline__ double readlane_f64(double x, int lane) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(x), lane);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(x), lane);
  return __hiloint2double(hi, lo);
}

// s = sqrt(x), r = 1/sqrt(x) for a positive normal x
__device__ __forceinline__ void sqrt_rsqrt(double x, double& s, double& r) {
  const double y = __builtin_amdgcn_rsq(x);
  double g = x * y, h = 0.5 * y;
#pragma unroll
  for (int it = 0; it < 3; ++it) {
    const double e = fma(-h, g, 0.5);
    g = fma(g, e, g);
    h = fma(h, e, h);
  }
  g = fma(fma(-g, g, x), h, g);
  s = g;
  r = h + h;
}

// acc += A B for 16 x 16 blocks in LDS: A[i][k] = pa[i * sai + k * sak], B[k][j] = pb[k * sbk + j * sbj]
__device__ __forceinline__ d4 block_mma(const double* pa, int sai, int sak, const double* pb, int sbk, int sbj, d4 acc,
                                        int lane) {
  const int i = lane & 15, g = lane >> 4;
  double a[4], b[4];
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) {
    a[ks] = pa[i * sai + (4 * ks + g) * sak];
    b[ks] = pb[(4 * ks + g) * sbk + i * sbj];
  }
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) acc = mfma_f64(a[ks], b[ks], acc);
  return acc;
}

constexpr int CHB = 16, CHN = 64, CHP = 65;
constexpr int kCholBlockedLds = (2 * CHN * CHP + 2 * CHN) * (int)sizeof(double);
#ifdef SAPCA_CHOL_TIMING   // tools/ubench/chol_phases.hip: shader-clock stamps at the phase boundaries
__device__ unsigned long long sapca_chol_stamps[32];
#define CHOL_STAMP(k) if (threadIdx.x == 0) sapca_chol_stamps[k] = __builtin_readcyclecounter();
#else
#define CHOL_STAMP(k)
#endif

// lanes 0..15 of the calling wave: row r of the diagonal block at c0 in, column r of its inverse out
__device__ __forceinline__ void invert_diag_block(const double* Lm, double* Xm, const double* dinvs, int c0, int lane) {
  const int r = lane & (CHB - 1);
  double a[CHB], x[CHB];
#pragma unroll
  for (int k = 0; k < CHB; ++k) a[k] = Lm[(c0 + r) * CHP + c0 + k];
  const double dmine = dinvs[c0 + r];
#pragma unroll
  for (int i = 0; i < CHB; ++i) {
    double s0 = 0.0, s1 = 0.0;
#pragma unroll
    for (int k = 0; k + 1 < i; k += 2) {
      s0 += readlane_f64(a[k], i) * x[k];
      s1 += readlane_f64(a[k + 1], i) * x[k + 1];
    }
    if (i & 1) s0 += readlane_f64(a[i - 1], i) * x[i - 1];
    const double di = readlane_f64(dmine, i);
    x[i] = i == r ? di : (i > r ? -(s0 + s1) * di : 0.0);
  }
  if (lane < CHB) {
#pragma unroll
    for (int i = 0; i < CHB; ++i) Xm[(c0 + i) * CHP + c0 + r] = x[i];
  }
}

// Factor + invert the (16 nb) x (16 nb) matrix in Lm (lower triangle, upper part zero) -> L in Lm, L^-1 in Xm
// (Xm zeroed by the caller).  All 256 threads call it; it ends with a workgroup barrier.
template <bool STAMPS>
__device__ __forceinline__ void chol_inv_core(double* Lm, double* Xm, double* dinvs, int nb, double floor_s, int& bad) {
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
  const int i16 = lane & 15, g4 = lane >> 4;
  for (int b = 0; b < nb; ++b) {
    const int c0 = b * CHB;
    if (wave == 0) {
      double a[CHB];
#pragma unroll
      for (int c = 0; c < CHB; ++c) a[c] = Lm[lane * CHP + c0 + c];
#pragma unroll
      for (int j = 0; j < CHB; ++j) {
        double piv = readlane_f64(a[j], c0 + j);
        if (!(piv > floor_s)) { piv = floor_s; bad += 1; }
        double d, dinv;
        sqrt_rsqrt(piv, d, dinv);
        a[j] = lane == c0 + j ? d : a[j] * dinv;
        if (lane == 0) dinvs[c0 + j] = dinv;
#pragma unroll
        for (int c = j + 1; c < CHB; ++c) a[c] -= a[j] * readlane_f64(a[j], c0 + c);
      }
#pragma unroll
      for (int c = 0; c < CHB; ++c)
        if (lane >= c0 + c) Lm[lane * CHP + c0 + c] = a[c];
    } else if (wave == 1 && b > 0) {
      invert_diag_block(Lm, Xm, dinvs, c0 - CHB, lane);
    }
    __syncthreads();
    if (STAMPS) { CHOL_STAMP(2 + 2 * b) }
    // trailing blocks (I, J), b < J <= I < nb:  G_IJ -= P_I P_J^T with P = the block column just finished
    const int ntb = nb - b - 1, npairs = ntb * (ntb + 1) / 2;
    for (int p = wave; p < npairs; p += 4) {
      const int ii = p >= 3 ? 2 : (p >= 1 ? 1 : 0), jj = p - ii * (ii + 1) / 2;
      const int rI = (b + 1 + ii) * CHB, rJ = (b + 1 + jj) * CHB;
      d4 acc = d4{0, 0, 0, 0};
      acc = block_mma(Lm + rI * CHP + c0, CHP, 1, Lm + rJ * CHP + c0, 1, CHP, acc, lane);
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int row = rI + g4 + 4 * reg, col = rJ + i16;
        if (col <= row) Lm[row * CHP + col] -= acc[reg];
      }
    }
    __syncthreads();
    if (STAMPS) { CHOL_STAMP(3 + 2 * b) }
  }
  // the last diagonal block is inverted by wave 1 beside the block rows that do not need it yet
  if (wave == 1) invert_diag_block(Lm, Xm, dinvs, (nb - 1) * CHB, lane);
  if (STAMPS) { CHOL_STAMP(10) }
  for (int bi = 1; bi < nb; ++bi) {
    if (bi == nb - 1) __syncthreads();   // X of the last diagonal block
    const int bj = wave == 0 ? 0 : wave - 1;   // waves 0, 2, 3 take block columns 0, 1, 2
    if (wave != 1 && bj < bi) {
      d4 tacc = d4{0, 0, 0, 0};
      for (int kb = bj; kb < bi; ++kb)
        tacc = block_mma(Lm + bi * CHB * CHP + kb * CHB, CHP, 1, Xm + kb * CHB * CHP + bj * CHB, CHP, 1, tacc, lane);
      // D layout: tacc[ks] = T[g + 4 ks][j] -- the B operand of MFMA step ks
      d4 xacc = d4{0, 0, 0, 0};
      double a[4];
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) a[ks] = Xm[(bi * CHB + i16) * CHP + bi * CHB + 4 * ks + g4];
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) xacc = mfma_f64(a[ks], tacc[ks], xacc);
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) Xm[(bi * CHB + g4 + 4 * reg) * CHP + bj * CHB + i16] = -xacc[reg];
      // a block column stays with its wave: the next block row reads what this wave wrote, nothing else's
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
    }
    if (STAMPS) { CHOL_STAMP(10 + bi) }
  }
  __syncthreads();
  if (STAMPS) {
    for (int bi = nb; bi < 4; ++bi) { CHOL_STAMP(10 + bi) }
  }
}

__global__ void __launch_bounds__(256)
chol_inv_blocked_kernel(const double* __restrict__ G, int l, int ld, double* __restrict__ R, double* __restrict__ Rinv,
                        int* __restrict__ info, const double* __restrict__ wsum, float* __restrict__ vec32, double* __restrict__ vec64) {
  extern __shared__ double cb_lds[];
  double* Lm = cb_lds;              // Lm[i * CHP + c] = L[i][c] (lower), in place over G
  double* Xm = Lm + CHN * CHP;      // Xm[i * CHP + c] = (L^-1)[i][c]
  double* dinvs = Xm + CHN * CHP;
  double* ws = dinvs + CHN;         // the (weighted) column sums of the panel being normalised
  if (wsum && threadIdx.x < CHN) ws[threadIdx.x] = (int)threadIdx.x < l ? wsum[threadIdx.x] : 0.0;
  const int t = threadIdx.x, lane = t & 63;
  const int nb = (l + CHB - 1) / CHB;
  CHOL_STAMP(0)
  // every load in flight before the first use: one HBM latency for the whole matrix
  double v[16];
#pragma unroll
  for (int u = 0; u < 16; ++u) {
    const int e = t + u * 256, i = e >> 6, c = e & 63;
    v[u] = (i < l && c <= i) ? G[(size_t)i * ld + c] : 0.0;
  }
  double dg = lane < l ? fabs(G[(size_t)lane * ld + lane]) : 0.0;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) dg = fmax(dg, __shfl_xor(dg, off));
  const double floor_s = dg * 1e-13 + 1e-300;
  const double pad = dg > 0.0 ? dg : 1.0;
#pragma unroll
  for (int u = 0; u < 16; ++u) {
    const int e = t + u * 256, i = e >> 6, c = e & 63;
    Lm[i * CHP + c] = (i >= l && i == c) ? pad : v[u];
    Xm[i * CHP + c] = 0.0;
  }
  __syncthreads();
  CHOL_STAMP(1)
  int bad = 0;
  chol_inv_core<true>(Lm, Xm, dinvs, nb, floor_s, bad);
  // R = L^T (upper): R[r][c] = L[c][r];  R^-1 = (L^-1)^T
  if (ld == CHN) {
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const int e = t + u * 256, r = e >> 6, c = e & 63;
      const bool in = r < l && c < l && c >= r;
      R[e] = in ? Lm[c * CHP + r] : 0.0;
      Rinv[e] = in ? Xm[c * CHP + r] : 0.0;
    }
  } else {
    for (int e = t; e < ld * ld; e += 256) {
      const int r = e / ld, c = e % ld;
      const bool in = r < l && c < l && c >= r;
      R[e] = in ? Lm[c * CHP + r] : 0.0;
      Rinv[e] = in ? Xm[c * CHP + r] : 0.0;
    }
  }
  CHOL_STAMP(14)
  if (wsum && t < ld) {
    // vec[j] = sum_{i <= j} Rinv[i][j] ws[i] = row j of L^-1 times ws: the column sums of P R^-1 (the centring vector of
    // the next sweep) without another pass over the normalised panel
    double acc = 0;
    if (t < l)
      for (int i2 = 0; i2 <= t; ++i2) acc += Xm[t * CHP + i2] * ws[i2];
    if (vec32) vec32[t] = (float)acc;
    if (vec64) vec64[t] = acc;
  }
  if (t == 0 && bad) atomicAdd(info, bad);
}

// 64 < l <= 128 (ld = 128): the same core on the two 64 x 64 diagonal halves of G = [G11 . ; G21 G22],
//   L11 = chol(G11),  L21 = G21 L11^-T,  L22 = chol(G22 - L21 L21^T),  X21 = -X22 (L21 X11),
// with the 64 x 64 products as 16 x 16 blocks on the matrix cores; four 64 x 65 LDS buffers (133 KiB).
// sum over kb < nk of A_blk(kb) B_blk(kb) for one 16 x 16 output block
__device__ __forceinline__ d4 mm_block(const double* pa, int sai, int sak, const double* pb, int sbk, int sbj, int nk, int lane) {
  d4 acc = d4{0, 0, 0, 0};
  for (int kb = 0; kb < nk; ++kb) acc = block_mma(pa + kb * CHB * sak, sai, sak, pb + kb * CHB * sbk, sbk, sbj, acc, lane);
  return acc;
}

constexpr int kChol128Lds = (4 * CHN * CHP + CHN) * (int)sizeof(double);

__global__ void __launch_bounds__(256)
chol_inv_blocked128_kernel(const double* __restrict__ G, int l, double* __restrict__ R, double* __restrict__ Rinv,
                           int* __restrict__ info) {
  constexpr int LD = 128;
  extern __shared__ double cb_lds[];
  double* B0 = cb_lds;
  double* B1 = B0 + CHN * CHP;
  double* B2 = B1 + CHN * CHP;
  double* B3 = B2 + CHN * CHP;
  double* dinvs = B3 + CHN * CHP;
  const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
  const int i16 = lane & 15, g4 = lane >> 4;
  const int l2 = l - CHN, nb2 = (l2 + CHB - 1) / CHB;
  double dg = fabs(G[(size_t)lane * LD + lane]);
  if (lane + CHN < l) dg = fmax(dg, fabs(G[(size_t)(lane + CHN) * LD + lane + CHN]));
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) dg = fmax(dg, __shfl_xor(dg, off));
  const double floor_s = dg * 1e-13 + 1e-300;
  const double pad = dg > 0.0 ? dg : 1.0;
  int bad = 0;
  // ---- G11 -> L11 (B0), X11 (B1); G21 -> B2 meanwhile
  {
    double v[16], w[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const int e = t + u * 256, i = e >> 6, c = e & 63;
      v[u] = c <= i ? G[(size_t)i * LD + c] : 0.0;
      w[u] = i < l2 ? G[(size_t)(CHN + i) * LD + c] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const int e = t + u * 256, i = e >> 6, c = e & 63;
      B0[i * CHP + c] = v[u];
      B1[i * CHP + c] = 0.0;
      B2[i * CHP + c] = w[u];
    }
  }
  __syncthreads();
  chol_inv_core<false>(B0, B1, dinvs, 4, floor_s, bad);
  // outputs of the first half: R[0:64][0:64] = L11^T, Rinv likewise, and the zero block below them
#pragma unroll
  for (int u = 0; u < 16; ++u) {
    const int e = t + u * 256, r = e >> 6, c = e & 63;
    const bool in = c >= r;
    R[(size_t)r * LD + c] = in ? B0[c * CHP + r] : 0.0;
    Rinv[(size_t)r * LD + c] = in ? B1[c * CHP + r] : 0.0;
    R[(size_t)(CHN + r) * LD + c] = 0.0;
    Rinv[(size_t)(CHN + r) * LD + c] = 0.0;
  }
  // ---- L21 = G21 X11^T -> B3   (L21[i][j] = sum_k G21[i][k] X11[j][k], k <= j)
  for (int blk = wave; blk < 16; blk += 4) {
    const int I = blk >> 2, J = blk & 3;
    const d4 acc = mm_block(B2 + I * CHB * CHP, CHP, 1, B1 + J * CHB * CHP, 1, CHP, J + 1, lane);
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) B3[(I * CHB + g4 + 4 * reg) * CHP + J * CHB + i16] = acc[reg];
  }
  __syncthreads();
  // ---- S = G22 - L21 L21^T -> B0 (lower), R[0:64][64:128] = L21^T; B2 becomes the zeroed X22
  {
    double v[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const int e = t + u * 256, i = e >> 6, c = e & 63;
      v[u] = (i < l2 && c <= i) ? G[(size_t)(CHN + i) * LD + CHN + c] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const int e = t + u * 256, i = e >> 6, c = e & 63;
      B0[i * CHP + c] = (i >= l2 && i == c) ? pad : v[u];
      B2[i * CHP + c] = 0.0;
      R[(size_t)i * LD + CHN + c] = c < l2 ? B3[c * CHP + i] : 0.0;   // (r = i, column 64 + c)
    }
  }
  __syncthreads();
  for (int p = wave; p < 10; p += 4) {   // lower block pairs (I, J), J <= I < 4
    const int I = p >= 6 ? 3 : (p >= 3 ? 2 : (p >= 1 ? 1 : 0)), J = p - I * (I + 1) / 2;
    const d4 acc = mm_block(B3 + I * CHB * CHP, CHP, 1, B3 + J * CHB * CHP, 1, CHP, 4, lane);
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int row = I * CHB + g4 + 4 * reg, col = J * CHB + i16;
      if (col <= row) B0[row * CHP + col] -= acc[reg];
    }
  }
  __syncthreads();
  chol_inv_core<false>(B0, B2, dinvs, nb2, floor_s, bad);   // L22 in B0, X22 in B2
#pragma unroll
  for (int u = 0; u < 16; ++u) {
    const int e = t + u * 256, r = e >> 6, c = e & 63;
    const bool in = r < l2 && c < l2 && c >= r;
    R[(size_t)(CHN + r) * LD + CHN + c] = in ? B0[c * CHP + r] : 0.0;
    Rinv[(size_t)(CHN + r) * LD + CHN + c] = in ? B2[c * CHP + r] : 0.0;
  }
  __syncthreads();
  // ---- W = L21 X11 -> B0;  X21 = -X22 W -> B3;  Rinv[0:64][64:128] = X21^T
  for (int blk = wave; blk < 16; blk += 4) {
    const int I = blk >> 2, J = blk & 3;
    // X11 is lower triangular: block row kb of its block column J is zero for kb < J
    const d4 acc = mm_block(B3 + I * CHB * CHP + J * CHB, CHP, 1, B1 + J * CHB * CHP + J * CHB, CHP, 1, 4 - J, lane);
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) B0[(I * CHB + g4 + 4 * reg) * CHP + J * CHB + i16] = acc[reg];
  }
  __syncthreads();
  for (int blk = wave; blk < 16; blk += 4) {
    const int I = blk >> 2, J = blk & 3;
    // X22 is lower triangular: block column kb of its block row I is zero for kb > I
    const d4 acc = mm_block(B2 + I * CHB * CHP, CHP, 1, B0 + J * CHB, CHP, 1, I + 1, lane);
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) B3[(I * CHB + g4 + 4 * reg) * CHP + J * CHB + i16] = -acc[reg];
  }
  __syncthreads();
#pragma unroll
  for (int u = 0; u < 16; ++u) {
    const int e = t + u * 256, r = e >> 6, c = e & 63;
    Rinv[(size_t)r * LD + CHN + c] = c < l2 ? B3[c * CHP + r] : 0.0;
  }
  if (t == 0 && bad) atomicAdd(info, bad);
}

// vec[j] = sum_{i <= j} Rinv[i][j] wsum[i]: the column sums of P R^-1 from those of P (the normaliser's output is never re-read)
template <typename T>
__global__ void rinv_tvec_kernel(const double* __restrict__ Rinv, int l, int ld, const double* __restrict__ wsum, T* __restrict__ vec) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= ld) return;
  double s = 0;
  if (j < l)
    for (int i = 0; i <= j; ++i) s += Rinv[(size_t)i * ld + j] * wsum[i];
  vec[j] = (T)s;
}

}  // namespace

// l > 128: the factorisation runs on the host (the one-workgroup kernels keep the matrix in LDS); same pivot floor, same
// outputs.  A wide panel is not the path this library is tuned for: it is here so that no (n_components, n_oversamples)
// the reference accepts is refused.
static void chol_inv_host(const double* G, int l, int ld, double* R, double* Rinv, int* info, hipStream_t s) {
  std::vector<double> g((size_t)ld * ld);
  SAPCA_HIP(hipMemcpyAsync(g.data(), G, g.size() * sizeof(double), hipMemcpyDeviceToHost, s));
  SAPCA_HIP(hipStreamSynchronize(s));
  std::vector<double> a((size_t)l * l), r((size_t)ld * ld, 0.0), ri((size_t)ld * ld, 0.0), dinv((size_t)l);
  for (int i = 0; i < l; ++i)
    for (int j = 0; j < l; ++j) a[(size_t)i * l + j] = g[(size_t)i * ld + j];
  double scale = 0;
  for (int i = 0; i < l; ++i) scale = std::max(scale, std::fabs(a[(size_t)i * l + i]));
  const double floor_v = scale * 1e-13 + 1e-300;
  int bad = 0;
  for (int kk = 0; kk < l; ++kk) {   // upper factor, right-looking: G = R^T R
    double v = a[(size_t)kk * l + kk];
    if (!(v > floor_v)) { v = floor_v; ++bad; }
    v = std::sqrt(v);
    a[(size_t)kk * l + kk] = v;
    dinv[kk] = 1.0 / v;
    double* rk = &a[(size_t)kk * l];
    for (int j = kk + 1; j < l; ++j) rk[j] *= dinv[kk];
    for (int i = kk + 1; i < l; ++i) {
      const double rki = rk[i];
      double* ai = &a[(size_t)i * l];
      for (int j = i; j < l; ++j) ai[j] -= rki * rk[j];
    }
  }
  // R^-1 (upper) by back substitution, row by row from the bottom: X[i][j] = -(sum_{i<t<=j} R[i][t] X[t][j]) / R[i][i]
  for (int i = l - 1; i >= 0; --i) {
    double* xi = &ri[(size_t)i * ld];
    xi[i] = dinv[i];
    for (int t = i + 1; t < l; ++t) {
      const double rit = a[(size_t)i * l + t];
      const double* xt = &ri[(size_t)t * ld];
      for (int j = t; j < l; ++j) xi[j] -= rit * xt[j];
    }
    for (int j = i + 1; j < l; ++j) xi[j] *= dinv[i];
    // (xi[j] accumulated -sum R[i][t] X[t][j]; the division by R[i][i] completes the row)
  }
  for (int i = 0; i < l; ++i)
    for (int j = i; j < l; ++j) r[(size_t)i * ld + j] = a[(size_t)i * l + j];
  SAPCA_HIP(hipMemcpyAsync(R, r.data(), r.size() * sizeof(double), hipMemcpyHostToDevice, s));
  SAPCA_HIP(hipMemcpyAsync(Rinv, ri.data(), ri.size() * sizeof(double), hipMemcpyHostToDevice, s));
  if (bad) {
    int have = 0;
    SAPCA_HIP(hipMemcpyAsync(&have, info, sizeof(int), hipMemcpyDeviceToHost, s));
    SAPCA_HIP(hipStreamSynchronize(s));
    have += bad;
    SAPCA_HIP(hipMemcpyAsync(info, &have, sizeof(int), hipMemcpyHostToDevice, s));
  }
  SAPCA_HIP(hipStreamSynchronize(s));   // (the host vectors go out of scope)
}

// Which of the four takes an l x l matrix of row stride ld.  The callers (engine.cpp) pad ld to a multiple of 16 up to 128 and
// to a multiple of 64 beyond, so the shapes that arrive are
//   route      | code                        | l              | ld                        | vec = Rinv^T wsum by
//   Blocked    | chol_inv_blocked_kernel     | l <= 64        | 16 .. 64, 128             | its own epilogue
//   Blocked128 | chol_inv_blocked128_kernel  | 64 < l <= 128  | 128                       | rinv_tvec_kernel
//   General    | chol_inv_kernel             | 64 < l <= 112  | round_up(l, 16) < 128     | rinv_tvec_kernel
//   Host       | chol_inv_host               | l > 128        | round_up(l, 64)           | rinv_tvec_kernel
// and, in the debug variant under SAPCA_CHOL_GENERAL, General for every l <= 128.
enum class CholRoute { Blocked, Blocked128, General, Host };

static CholRoute chol_route(int l, int ld, bool general_only) {
  if (l > 128) return CholRoute::Host;
  if (general_only) return CholRoute::General;
  if (l <= 64 && ld >= l && ld <= 256) return CholRoute::Blocked;
  if (l > 64 && ld == 128) return CholRoute::Blocked128;
  return CholRoute::General;
}

void chol_inv(const double* G, int l, int ld, double* R, double* Rinv, int* info, hipStream_t s, const double* wsum, float* vec32, double* vec64) {
  static const bool general_only = dbg_env("SAPCA_CHOL_GENERAL") != nullptr;
  if (!vec32 && !vec64) wsum = nullptr;
  switch (chol_route(l, ld, general_only)) {
    case CholRoute::Blocked: {
      static LdsAttrState attr;
      ensure_dynamic_lds(reinterpret_cast<const void*>(&chol_inv_blocked_kernel), kCholBlockedLds, attr);
      hipLaunchKernelGGL(chol_inv_blocked_kernel, dim3(1), dim3(256), kCholBlockedLds, s, G, l, ld, R, Rinv, info, wsum, vec32, vec64);
      SAPCA_HIP(hipGetLastError());
      return;   // (the product rode in the epilogue)
    }
    case CholRoute::Blocked128: {
      static LdsAttrState attr;
      ensure_dynamic_lds(reinterpret_cast<const void*>(&chol_inv_blocked128_kernel), kChol128Lds, attr);
      hipLaunchKernelGGL(chol_inv_blocked128_kernel, dim3(1), dim3(256), kChol128Lds, s, G, l, R, Rinv, info);
      SAPCA_HIP(hipGetLastError());
      break;
    }
    case CholRoute::General: {
      const size_t lds = ((size_t)l * (l + 1) + l) * sizeof(double);
      static LdsAttrState attr;
      if (lds > 48 * 1024) ensure_dynamic_lds(reinterpret_cast<const void*>(&chol_inv_kernel), lds, attr);
      hipLaunchKernelGGL(chol_inv_kernel, dim3(1), dim3(256), lds, s, G, l, ld, R, Rinv, info);
      SAPCA_HIP(hipGetLastError());
      break;
    }
    case CholRoute::Host:
      chol_inv_host(G, l, ld, R, Rinv, info, s);
      break;
  }
  // the routes that do not carry the product in their own epilogue
  if (!wsum) return;
  if (vec32) hipLaunchKernelGGL((rinv_tvec_kernel<float>), dim3((ld + 63) / 64), dim3(64), 0, s, Rinv, l, ld, wsum, vec32);
  if (vec64) hipLaunchKernelGGL((rinv_tvec_kernel<double>), dim3((ld + 63) / 64), dim3(64), 0, s, Rinv, l, ld, wsum, vec64);
  SAPCA_HIP(hipGetLastError());
}

}  // namespace k
}  // namespace sapca
