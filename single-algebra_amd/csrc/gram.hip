// The Gram matrix G = P^T P of a tall-skinny panel (step one of the CholeskyQR2 normaliser: dense_common.h has the
// scheme and the MFMA lane maps), the panel fix-up that rides in its read pass, and the (weighted) column sums.
#include "dense_common.h"

#include <algorithm>

namespace sapca {
namespace k {

namespace {

// ---------------------------------------------------------------- Gram
// Upper-triangular tile pairs (ta <= tb) of G = P^T P.  Each wave streams 4-row chunks; the
// four waves of a block are summed through LDS in a fixed order and the block writes one slab
// of raw accumulator fragments; gram_reduce_kernel adds the slabs in block order (bitwise
// reproducible) and unpacks the fragment layout into the full symmetric matrix.
template <typename T, int NT>
__global__ void __launch_bounds__(256)
gram_kernel(const T* __restrict__ P, int64_t rows, int ld, double* __restrict__ slabs) {
  constexpr int NPAIR = NT * (NT + 1) / 2;
  extern __shared__ double lds[];  // NPAIR * 4 * 64
  const int lane = threadIdx.x & (WAVE - 1);
  const int wave = threadIdx.x / WAVE;
  const int g = lane >> 4, c = lane & 15;
  d4 acc[NPAIR];
#pragma unroll
  for (int p = 0; p < NPAIR; ++p) acc[p] = d4{0, 0, 0, 0};
  const int64_t stride = (int64_t)gridDim.x * 4 * 4;
  int64_t r0 = ((int64_t)blockIdx.x * 4 + wave) * 4;
  // D chunks of 4 rows in flight per wave: with one or two waves per SIMD the loop is otherwise bound by
  // the HBM latency of a single 1 KiB chunk (0.6 TB/s measured with D = 1)
  constexpr int D = 4;
  T buf[D][NT];
#pragma unroll
  for (int d = 0; d < D; ++d) {
    const int64_t r = r0 + d * stride + g;
#pragma unroll
    for (int t = 0; t < NT; ++t) buf[d][t] = (r < rows) ? P[r * ld + 16 * t + c] : (T)0;
  }
  for (; r0 < rows; r0 += D * stride) {
#pragma unroll
    for (int d = 0; d < D; ++d) {
      double v[NT];
#pragma unroll
      for (int t = 0; t < NT; ++t) v[t] = (double)buf[d][t];
      const int64_t rn = r0 + (d + D) * stride + g;
#pragma unroll
      for (int t = 0; t < NT; ++t) buf[d][t] = (rn < rows) ? P[rn * ld + 16 * t + c] : (T)0;
      int p = 0;
#pragma unroll
      for (int ta = 0; ta < NT; ++ta)
#pragma unroll
        for (int tb = ta; tb < NT; ++tb) {
          acc[p] = mfma_f64(v[ta], v[tb], acc[p]);
          ++p;
        }
    }
  }
  for (int w = 0; w < 4; ++w) {
    if (wave == w) {
#pragma unroll
      for (int p = 0; p < NPAIR; ++p)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          double* dst = lds + (p * 4 + reg) * WAVE + lane;
          if (w == 0) *dst = acc[p][reg]; else *dst += acc[p][reg];
        }
    }
    __syncthreads();
  }
  double* slab = slabs + (int64_t)blockIdx.x * NPAIR * 256;
  for (int i = threadIdx.x; i < NPAIR * 256; i += blockDim.x) slab[i] = lds[i];
}

// The same Gram for NT >= 7 tile columns (panels of 112 / 128 columns): 28 / 36 tile pairs of four f64 accumulators each do
// not fit one wave's registers (the kernel above spills 245 VGPRs at NT = 8 and runs one wave per SIMD: 2.5 ms on C5's
// 2M x 128 panel, against 0.25 ms of HBM time and 0.5 ms of MFMA time).  Here the four waves of a workgroup stream the
// SAME 4-row chunks and split the tile pairs among them (pair p belongs to wave p mod 4: nine pairs = 36 accumulator
// registers each); a chunk is fetched from HBM once and found in L1 by the other three waves.  No LDS, no barrier: every
// wave writes its own pairs' fragments of the slab.
template <typename T, int NT, int W>
__device__ __forceinline__ void gram_split_wave(const T* __restrict__ P, const T* __restrict__ Pb, int64_t rows, int ld, double* __restrict__ slab,
                                                int lane) {
  constexpr int NPAIR = NT * (NT + 1) / 2;
  constexpr int MINE = (NPAIR - W + 3) / 4;   // pairs p = W, W + 4, ...
  const int g = lane >> 4, c = lane & 15;
  d4 acc[MINE];
#pragma unroll
  for (int p = 0; p < MINE; ++p) acc[p] = d4{0, 0, 0, 0};
  const int64_t stride = (int64_t)gridDim.x * 4;
  int64_t r0 = (int64_t)blockIdx.x * 4;
  constexpr int D = 4;   // chunks in flight
  T buf[D][NT];
  auto fetch = [&](int64_t r, int t) -> T {
    return (r < rows) ? ((Pb && t >= 4) ? Pb[r * ld + 16 * (t - 4) + c] : P[r * ld + 16 * t + c]) : (T)0;
  };
#pragma unroll
  for (int d = 0; d < D; ++d)
#pragma unroll
    for (int t = 0; t < NT; ++t) buf[d][t] = fetch(r0 + d * stride + g, t);
  for (; r0 < rows; r0 += D * stride) {
#pragma unroll
    for (int d = 0; d < D; ++d) {
      double v[NT];
#pragma unroll
      for (int t = 0; t < NT; ++t) v[t] = (double)buf[d][t];
#pragma unroll
      for (int t = 0; t < NT; ++t) buf[d][t] = fetch(r0 + (d + D) * stride + g, t);
      int p = 0, mine = 0;
#pragma unroll
      for (int ta = 0; ta < NT; ++ta)
#pragma unroll
        for (int tb = ta; tb < NT; ++tb) {
          if (p % 4 == W) {
            acc[mine] = mfma_f64(v[ta], v[tb], acc[mine]);
            ++mine;
          }
          ++p;
        }
    }
  }
#pragma unroll
  for (int q = 0; q < MINE; ++q)
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) slab[((W + 4 * q) * 4 + reg) * WAVE + lane] = acc[q][reg];
}

template <typename T, int NT>
__global__ void __launch_bounds__(256)
gram_split_kernel(const T* __restrict__ P, int64_t rows, int ld, double* __restrict__ slabs, const T* __restrict__ Pb) {
  constexpr int NPAIR = NT * (NT + 1) / 2;
  const int lane = threadIdx.x & (WAVE - 1);
  double* slab = slabs + (int64_t)blockIdx.x * NPAIR * 256;
  switch (threadIdx.x / WAVE) {   // (a wave's pair list is static: its accumulators stay in registers)
    case 0: gram_split_wave<T, NT, 0>(P, Pb, rows, ld, slab, lane); break;
    case 1: gram_split_wave<T, NT, 1>(P, Pb, rows, ld, slab, lane); break;
    case 2: gram_split_wave<T, NT, 2>(P, Pb, rows, ld, slab, lane); break;
    default: gram_split_wave<T, NT, 3>(P, Pb, rows, ld, slab, lane); break;
  }
}


// ---------------------------------------------------------------- Gram with the producer's fix-up folded into its read pass
// Panels of 64 / 128 columns (NT = 4 / 8: every headline configuration).  A lane reads 16 bytes: lane (g, c) of a 4-row chunk
// holds columns 4c .. 4c+3 (and 64 + 4c .. for the second half) of row g, so MFMA tile t is the column set
// vcol(t, i) = 64 (t >> 2) + 4 i + (t & 3) -- a fixed permutation of the panel's columns that gram_reduce_kernel undoes.
// SRC: the panel is still in the state its producer left it in (PanelSource: the slabs of a sweep whose tile range was split
// over workgroups, minus the centring term mu sv^T).  Every element passes through exactly one lane here: it is summed,
// centred, written back to P and used -- split_reduce, rank1_subtract and one read of the panel are gone.
// want_sum: sum_r w[r] P[r][:] (w null: ones) rides along in f64 (the centring vector of the next sweep follows from it and
// R^-1: chol_inv).  NT = 8: the four waves stream the same rows and split the 36 tile pairs (see gram_split_kernel); wave 0
// does the write-back and the column sums.
__device__ __forceinline__ int vcol(int t, int i) { return 64 * (t >> 2) + 4 * i + (t & 3); }

template <typename T, int NT, bool SRC, int W>
__device__ __forceinline__ void gramv_wave(T* P, int64_t rows, int ld, double* __restrict__ slab, double* lds,
                                           const PanelSource<T>& src, const T* __restrict__ wgt, int want_sum, int lane, int wave) {
  constexpr int NPAIR = NT * (NT + 1) / 2;
  constexpr bool SPLIT = NT > 6;
  constexpr int MINE = SPLIT ? (NPAIR - W + 3) / 4 : NPAIR;
  constexpr int NH = NT / 4;
  const int g = lane >> 4, c = lane & 15;
  const bool owner = !SPLIT || W == 0;   // writes the panel back, sums the columns
  d4 acc[MINE];
#pragma unroll
  for (int p = 0; p < MINE; ++p) acc[p] = d4{0, 0, 0, 0};
  double cs[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) cs[t] = 0;
  const int64_t stride = SPLIT ? (int64_t)gridDim.x * 4 : (int64_t)gridDim.x * 16;
  int64_t r0 = SPLIT ? (int64_t)blockIdx.x * 4 : ((int64_t)blockIdx.x * 4 + wave) * 4;
  auto mma = [&](const T (&x)[NT], double wr) {
    double v[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) v[t] = (double)x[t];
    if (want_sum && owner) {
#pragma unroll
      for (int t = 0; t < NT; ++t) cs[t] += wr * v[t];
    }
    int p = 0, mine = 0;
#pragma unroll
    for (int ta = 0; ta < NT; ++ta)
#pragma unroll
      for (int tb = ta; tb < NT; ++tb) {
        if (!SPLIT || p % 4 == W) {
          acc[mine] = mfma_f64(v[ta], v[tb], acc[mine]);
          ++mine;
        }
        ++p;
      }
  };
  if constexpr (SRC) {
    T sv[NT];
    if (src.mu) {
#pragma unroll
      for (int hh = 0; hh < NH; ++hh) Four<T>::load(src.sv + 64 * hh + 4 * c, &sv[4 * hh]);
    }
    // A wave runs only a few chunks (2048 waves share a panel's rows), so what it waits for is the slabs of ONE chunk: U of
    // them are loaded into registers of their own before the first is added (a round trip per U slabs, not per slab), and
    // the head of the next chunk -- slab 0, the first U further slabs, mu and the weight -- is in flight while this chunk's
    // MFMAs run.  The adds keep their order: slab 1 .. nsplit - 1 onto slab 0, then - mu sv.
    constexpr int U = NT * sizeof(T) <= 16 ? 4 : NT * sizeof(T) <= 32 ? 2 : 1;   // (64 bytes of slabs per lane at a time: registers)
    const int nsplit = src.nsplit;
    const int64_t ss = src.slab_stride;
    auto load_slab = [&](const T* p, int sp, T (&y)[NT]) {
#pragma unroll
      for (int hh = 0; hh < NH; ++hh) Four<T>::load(p + sp * ss + 64 * hh, &y[4 * hh]);
    };
    T hx[NT], hy[U][NT], hm = (T)0;
    double hw = 0;
    auto head = [&](int64_t r) {
      if (r < rows) {
        const T* p = src.parts + r * ld + 4 * c;
        load_slab(p, 0, hx);
#pragma unroll
        for (int u = 0; u < U; ++u)
          if (1 + u < nsplit) load_slab(p, 1 + u, hy[u]);
        if (src.mu) hm = src.mu[r];
        hw = wgt ? (double)wgt[r] : 1.0;
      }
    };
    head(r0 + g);
    for (; r0 < rows; r0 += stride) {
      const int64_t r = r0 + g;
      const bool live = r < rows;
      T x[NT];
#pragma unroll
      for (int t = 0; t < NT; ++t) x[t] = (T)0;
      double wr = 0;
      T m = (T)0;
      if (live) {
        const T* p = src.parts + r * ld + 4 * c;
#pragma unroll
        for (int t = 0; t < NT; ++t) x[t] = hx[t];
#pragma unroll
        for (int u = 0; u < U; ++u)
          if (1 + u < nsplit) {
#pragma unroll
            for (int t = 0; t < NT; ++t) x[t] += hy[u][t];
          }
        m = hm;
        wr = hw;
        int sp = 1 + U;
        for (; sp + U <= nsplit; sp += U) {
          T y[U][NT];
#pragma unroll
          for (int u = 0; u < U; ++u) load_slab(p, sp + u, y[u]);
#pragma unroll
          for (int u = 0; u < U; ++u)
#pragma unroll
            for (int t = 0; t < NT; ++t) x[t] += y[u][t];
        }
        if constexpr (U > 1) if (sp < nsplit) {   // the remainder: up to U - 1 slabs, loaded together as well
          T y[U > 1 ? U - 1 : 1][NT];
#pragma unroll
          for (int u = 0; u < U - 1; ++u)
            if (sp + u < nsplit) load_slab(p, sp + u, y[u]);
#pragma unroll
          for (int u = 0; u < U - 1; ++u)
            if (sp + u < nsplit) {
#pragma unroll
              for (int t = 0; t < NT; ++t) x[t] += y[u][t];
            }
        }
      }
      head(r0 + stride + g);   // (another row: in place, too, it is not the one stored below)
      if (live) {
        if (src.mu) {
#pragma unroll
          for (int t = 0; t < NT; ++t) x[t] -= m * sv[t];
        }
        if (owner) {
#pragma unroll
          for (int hh = 0; hh < NH; ++hh) Four<T>::store(P + r * ld + 64 * hh + 4 * c, &x[4 * hh]);
        }
      }
      mma(x, wr);
    }
  } else {
    constexpr int D = NT == 4 ? 4 : 2;   // chunks in flight
    T buf[D][NT];
    double wb[D];
    auto fetch = [&](int64_t r, T (&out)[NT], double& wr) {
      if (r < rows) {
#pragma unroll
        for (int hh = 0; hh < NH; ++hh) Four<T>::load(P + r * ld + 64 * hh + 4 * c, &out[4 * hh]);
        wr = (want_sum && wgt) ? (double)wgt[r] : 1.0;
      } else {
#pragma unroll
        for (int t = 0; t < NT; ++t) out[t] = (T)0;
        wr = 0;
      }
    };
#pragma unroll
    for (int d = 0; d < D; ++d) fetch(r0 + d * stride + g, buf[d], wb[d]);
    for (; r0 < rows; r0 += D * stride) {
#pragma unroll
      for (int d = 0; d < D; ++d) {
        T x[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) x[t] = buf[d][t];
        const double wr = wb[d];
        fetch(r0 + (d + D) * stride + g, buf[d], wb[d]);
        mma(x, wr);
      }
    }
  }
  // column sums: over the four row groups of the wave by shuffles; over the waves in order through LDS
  if (want_sum && owner) {
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      cs[t] += __shfl_xor(cs[t], 16);
      cs[t] += __shfl_xor(cs[t], 32);
    }
  }
  if constexpr (SPLIT) {
#pragma unroll
    for (int q = 0; q < MINE; ++q)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) slab[((W + 4 * q) * 4 + reg) * WAVE + lane] = acc[q][reg];
    if (owner && g == 0) {
#pragma unroll
      for (int t = 0; t < NT; ++t) slab[NPAIR * 256 + 16 * t + c] = want_sum ? cs[t] : 0.0;
    }
  } else {
    double* lsum = lds + NPAIR * 256;   // [wave][16 NT]
    for (int w = 0; w < 4; ++w) {
      if (wave == w) {
#pragma unroll
        for (int p = 0; p < NPAIR; ++p)
#pragma unroll
          for (int reg = 0; reg < 4; ++reg) {
            double* dst = lds + (p * 4 + reg) * WAVE + lane;
            if (w == 0) *dst = acc[p][reg]; else *dst += acc[p][reg];
          }
        if (g == 0) {
#pragma unroll
          for (int t = 0; t < NT; ++t) {
            double* dst = lsum + 16 * t + c;
            if (w == 0) *dst = cs[t]; else *dst += cs[t];
          }
        }
      }
      __syncthreads();
    }
    for (int i = threadIdx.x; i < NPAIR * 256 + 16 * NT; i += blockDim.x) slab[i] = lds[i];
  }
}

template <typename T, int NT, bool SRC>
__global__ void __launch_bounds__(256, 2)   // (two workgroups per CU: 256 registers a lane, accumulators included)
gramv_kernel(T* P, int64_t rows, int ld, double* __restrict__ slabs, PanelSource<T> src, const T* __restrict__ wgt, int want_sum) {
  constexpr int NPAIR = NT * (NT + 1) / 2;
  extern __shared__ double lds[];   // NT <= 6: NPAIR * 256 + 16 NT doubles
  const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
  double* slab = slabs + (int64_t)blockIdx.x * (NPAIR * 256 + 16 * NT);
  if constexpr (NT > 6) {
    switch (wave) {   // (a wave's pair list is static: its accumulators stay in registers)
      case 0: gramv_wave<T, NT, SRC, 0>(P, rows, ld, slab, lds, src, wgt, want_sum, lane, wave); break;
      case 1: gramv_wave<T, NT, SRC, 1>(P, rows, ld, slab, lds, src, wgt, want_sum, lane, wave); break;
      case 2: gramv_wave<T, NT, SRC, 2>(P, rows, ld, slab, lds, src, wgt, want_sum, lane, wave); break;
      default: gramv_wave<T, NT, SRC, 3>(P, rows, ld, slab, lds, src, wgt, want_sum, lane, wave); break;
    }
  } else {
    gramv_wave<T, NT, SRC, 0>(P, rows, ld, slab, lds, src, wgt, want_sum, lane, wave);
  }
}

// P = sum_s parts[s] - mu sv^T, written out: the same fix-up for panels the kernel above does not take
template <typename T>
__global__ void materialize_kernel(T* P, int64_t rows, int ld, PanelSource<T> src) {
  const int64_t total = rows * ld;
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < total; i += stride) {
    T x = src.parts[i];
    for (int sp = 1; sp < src.nsplit; ++sp) x += src.parts[(int64_t)sp * src.slab_stride + i];
    if (src.mu) x -= src.mu[i / ld] * src.sv[i % ld];
    P[i] = x;
  }
}

// 16 elements x 16 slab-groups per block; each group sums its slabs in order, the 16 group sums
// are added in order: a fixed reduction tree, bitwise reproducible.
__global__ void __launch_bounds__(256)
gram_reduce_kernel(const double* __restrict__ slabs, int nslabs, int nt, int ld, double* __restrict__ G, int vtiles = 0,
                   double* __restrict__ wsum = nullptr) {
  // vtiles: the slabs come from gramv_kernel -- tile t is the column set vcol(t, .), and 16 nt (weighted) column sums
  // follow the fragments of every slab (wsum, nullable, receives their total)
  __shared__ double part[16][17];
  const int npair = nt * (nt + 1) / 2;
  const int slab_len = npair * 256 + (vtiles ? 16 * nt : 0);
  const int e = threadIdx.x & 15, grp = threadIdx.x >> 4;
  const int i = blockIdx.x * 16 + e;
  double sum = 0;
  if (i < slab_len) {
    // eight of the group's slabs are loaded before the first is added: a round trip per eight slabs, the order of the adds kept
    int b = grp;
    for (; b + 16 * 7 < nslabs; b += 16 * 8) {
      double v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = slabs[(int64_t)(b + 16 * u) * slab_len + i];
#pragma unroll
      for (int u = 0; u < 8; ++u) sum += v[u];
    }
    for (; b < nslabs; b += 16) sum += slabs[(int64_t)b * slab_len + i];
  }
  part[grp][e] = sum;
  __syncthreads();
  if (grp != 0 || i >= slab_len) return;
  sum = 0;
#pragma unroll
  for (int g2 = 0; g2 < 16; ++g2) sum += part[g2][e];
  if (i >= npair * 256) {
    const int t = (i - npair * 256) / 16, c = (i - npair * 256) % 16;
    if (wsum) wsum[vcol(t, c)] = sum;
    return;
  }
  int p = i / 256, rem = i % 256, reg = rem / 64, lane = rem % 64;
  int ta = 0;
  while (p >= nt - ta) { p -= nt - ta; ++ta; }
  const int tb = ta + p;
  const int row = vtiles ? vcol(ta, (lane >> 4) + 4 * reg) : 16 * ta + (lane >> 4) + 4 * reg;
  const int col = vtiles ? vcol(tb, lane & 15) : 16 * tb + (lane & 15);
  G[row * ld + col] = sum;
  G[col * ld + row] = sum;
}

template <typename T>
__global__ void colsum_partial_kernel(const T* __restrict__ P, int64_t rows, int ld, const T* __restrict__ w,
                                      double* __restrict__ partial) {
  extern __shared__ double red[];  // blockDim.y * ld
  const int j = threadIdx.x;
  double s = 0;
  const int64_t step = (int64_t)gridDim.x * blockDim.y;
  int64_t r = (int64_t)blockIdx.x * blockDim.y + threadIdx.y;
  for (; r + 3 * step < rows; r += 4 * step) {   // four loads in flight; the sum keeps its order
    const double a0 = (w ? (double)w[r] : 1.0) * (double)P[r * ld + j];
    const double a1 = (w ? (double)w[r + step] : 1.0) * (double)P[(r + step) * ld + j];
    const double a2 = (w ? (double)w[r + 2 * step] : 1.0) * (double)P[(r + 2 * step) * ld + j];
    const double a3 = (w ? (double)w[r + 3 * step] : 1.0) * (double)P[(r + 3 * step) * ld + j];
    s += a0;
    s += a1;
    s += a2;
    s += a3;
  }
  for (; r < rows; r += step) s += (w ? (double)w[r] : 1.0) * (double)P[r * ld + j];
  red[threadIdx.y * ld + j] = s;
  __syncthreads();
  if (threadIdx.y == 0) {
    for (int y = 1; y < (int)blockDim.y; ++y) s += red[y * ld + j];
    partial[(int64_t)blockIdx.x * ld + j] = s;
  }
}

template <typename T>
__global__ void __launch_bounds__(64)
colsum_final_kernel(const double* __restrict__ partial, int nblocks, int ld, T* __restrict__ out) {
  const int j = blockIdx.x;
  double s = 0;
  for (int b = threadIdx.x; b < nblocks; b += WAVE) s += partial[(int64_t)b * ld + j];
#pragma unroll
  for (int off = WAVE / 2; off > 0; off >>= 1) s += __shfl_xor(s, off);
  if (threadIdx.x == 0) out[j] = (T)s;
}

// out[j] = sum_r w[r] P[r][j] in f64 (w null: ones); partial: at least 1024 * ld doubles of scratch
template <typename T>
static void colsum_f64(const T* P, int64_t rows, int ld, const T* w, double* out, double* partial, hipStream_t s) {
  int by = 256 / ld;
  if (by < 1) by = 1;
  int nblocks = (int)((rows + by * 8 - 1) / (by * 8));
  if (nblocks > 1024) nblocks = 1024;
  if (nblocks < 1) nblocks = 1;
  hipLaunchKernelGGL((colsum_partial_kernel<T>), dim3(nblocks), dim3(ld, by), (size_t)by * ld * sizeof(double), s, P, rows, ld, w, partial);
  hipLaunchKernelGGL((colsum_final_kernel<double>), dim3(ld), dim3(64), 0, s, partial, nblocks, ld, out);
}

template <typename T, int NT>
void launch_gram(const T* P, int64_t rows, int ld, double* slabs, int nblocks, hipStream_t s) {
  constexpr int NPAIR = NT * (NT + 1) / 2;
  if constexpr (NT >= 7) {
    hipLaunchKernelGGL((gram_split_kernel<T, NT>), dim3(nblocks), dim3(256), 0, s, P, rows, ld, slabs, (const T*)nullptr);
    return;
  }
  const size_t lds = (size_t)NPAIR * 256 * sizeof(double);
  static LdsAttrState attr;
  if (lds > 48 * 1024) ensure_dynamic_lds(reinterpret_cast<const void*>(&gram_kernel<T, NT>), lds, attr);
  hipLaunchKernelGGL((gram_kernel<T, NT>), dim3(nblocks), dim3(256), lds, s, P, rows, ld, slabs);
}

}  // namespace

// [G_II G_IJ; . G_JJ] of a 128 x 128 pair Gram -> the 64 x 64 blocks (I, I), (I, J), (J, I), (J, J) of the ld x ld matrix
__global__ void gram_place_pair_kernel(const double* __restrict__ G2, int bi, int bj, int ld, double* __restrict__ G) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 128 * 128) return;
  const int r = i / 128, c = i % 128;
  const int gr = (r < 64 ? 64 * bi : 64 * bj - 64) + r, gc = (c < 64 ? 64 * bi : 64 * bj - 64) + c;
  G[(int64_t)gr * ld + gc] = G2[i];
}

template <typename T, int NT>
static void launch_gramv(T* P, int64_t rows, int ld, double* slabs, int nblocks, const PanelSource<T>* src, const T* w, bool want_sum,
                         hipStream_t s) {
  constexpr int NPAIR = NT * (NT + 1) / 2;
  const size_t lds = NT > 6 ? 0 : (size_t)(NPAIR * 256 + 16 * NT) * sizeof(double);
  if (src) {
    hipLaunchKernelGGL((gramv_kernel<T, NT, true>), dim3(nblocks), dim3(256), lds, s, P, rows, ld, slabs, *src, w, want_sum ? 1 : 0);
  } else {
    hipLaunchKernelGGL((gramv_kernel<T, NT, false>), dim3(nblocks), dim3(256), lds, s, P, rows, ld, slabs, PanelSource<T>{}, w, want_sum ? 1 : 0);
  }
}

template <typename T>
void materialize(T* P, int64_t rows, int ld, const PanelSource<T>& src, hipStream_t s) {
  if (rows == 0 || (src.parts == P && src.nsplit <= 1 && !src.mu)) return;
  hipLaunchKernelGGL((materialize_kernel<T>), dim3(grid_for(rows * ld, 256)), dim3(256), 0, s, P, rows, ld, src);
  SAPCA_HIP(hipGetLastError());
}

// Slabs (= workgroups) of a Gram pass over `rows` rows: one per 16 rows, at least one, at most 512
static int slab_blocks(int64_t rows) { return (int)std::min<int64_t>(std::max<int64_t>((rows + 15) / 16, 1), 512); }

// 64 / 128 columns, the panels of the staged sweeps: the producer's fix-up and the column sums ride in the read pass
template <typename T>
static void gram_fused(T* P, int64_t rows, int ld, double* G, DevBuf& scratch, hipStream_t s, const PanelSource<T>* src, const T* w, double* wsum) {
  const int nt = ld / 16;
  if (src && nt == 8 && src->parts == P) {   // (four waves read a row there: not in place)
    materialize(P, rows, ld, *src, s);
    src = nullptr;
  }
  const int npair = nt * (nt + 1) / 2, slab_len = npair * 256 + 16 * nt;
  const int nblocks = slab_blocks(rows);
  double* slabs = scratch.as<double>((size_t)nblocks * slab_len);
  if (nt == 4) launch_gramv<T, 4>(P, rows, ld, slabs, nblocks, src, w, wsum != nullptr, s);
  else launch_gramv<T, 8>(P, rows, ld, slabs, nblocks, src, w, wsum != nullptr, s);
  hipLaunchKernelGGL(gram_reduce_kernel, dim3((slab_len + 15) / 16), dim3(256), 0, s, slabs, nblocks, nt, ld, G, 1, wsum);
  SAPCA_HIP(hipGetLastError());
}

// More than 128 columns (P materialised): every pair (I < J) of 64-column blocks goes through the 128-wide kernel as the panel
// [P_I P_J] (a lone block pairs with itself); the diagonal blocks are written by several pairs, with the same bits each time
template <typename T>
static void gram_wide_pairs(const T* P, int64_t rows, int ld, double* G, DevBuf& scratch, hipStream_t s, const T* w, double* wsum) {
  const int nb = ld / 64, npair = 36;
  const int nblocks = slab_blocks(rows);
  double* slabs = scratch.as<double>((size_t)nblocks * npair * 256 + 128 * 128 + (wsum ? (size_t)1024 * ld : 0));
  double* G2 = slabs + (size_t)nblocks * npair * 256;
  for (int bi = 0; bi < nb; ++bi)
    for (int bj = bi + 1; bj < nb; ++bj) {
      hipLaunchKernelGGL((gram_split_kernel<T, 8>), dim3(nblocks), dim3(256), 0, s, P + 64 * bi, rows, ld, slabs, P + 64 * bj);
      hipLaunchKernelGGL(gram_reduce_kernel, dim3((npair * 256 + 15) / 16), dim3(256), 0, s, slabs, nblocks, 8, 128, G2, 0, (double*)nullptr);
      hipLaunchKernelGGL(gram_place_pair_kernel, dim3(64), dim3(256), 0, s, G2, bi, bj, ld, G);
    }
  SAPCA_HIP(hipGetLastError());
  if (wsum) colsum_f64(P, rows, ld, w, wsum, G2 + 128 * 128, s);
}

// 16 .. 112 columns but 64 (P materialised): the tile pairs in one kernel, the column sums in a pass of their own
template <typename T>
static void gram_plain(const T* P, int64_t rows, int ld, double* G, DevBuf& scratch, hipStream_t s, const T* w, double* wsum) {
  const int nt = ld / 16, npair = nt * (nt + 1) / 2;
  const int nblocks = slab_blocks(rows);
  double* slabs = scratch.as<double>((size_t)nblocks * npair * 256 + (wsum ? (size_t)1024 * ld : 0));
  with_tile_count<1, 2, 3, 5, 6, 7>(nt, [&](auto ntc) { launch_gram<T, decltype(ntc)::value>(P, rows, ld, slabs, nblocks, s); });
  hipLaunchKernelGGL(gram_reduce_kernel, dim3((npair * 256 + 15) / 16), dim3(256), 0, s, slabs, nblocks, nt, ld, G, 0, (double*)nullptr);
  SAPCA_HIP(hipGetLastError());
  if (wsum) colsum_f64(P, rows, ld, w, wsum, slabs + (size_t)nblocks * npair * 256, s);
}

template <typename T>
void gram(T* P, int64_t rows, int ld, double* G, DevBuf& scratch, hipStream_t s, const PanelSource<T>* src, const T* w, double* wsum) {
  SAPCA_CHECK(ld % 16 == 0 && ld >= 16 && (ld <= 128 || (ld % 64 == 0 && ld <= kMaxPanelWidth)), SAPCA_ERR_ARG,
              "gram: panel width must be a multiple of 16 up to 128, or of 64 up to 1024");
  if (ld == 64 || ld == 128) return gram_fused(P, rows, ld, G, scratch, s, src, w, wsum);
  if (src) materialize(P, rows, ld, *src, s);
  if (ld > 128) return gram_wide_pairs(P, rows, ld, G, scratch, s, w, wsum);
  gram_plain(P, rows, ld, G, scratch, s, w, wsum);
}

template <typename T>
void weighted_colsum(const T* P, int64_t rows, int ld, const T* w, T* out, DevBuf& scratch, hipStream_t s) {
  int by = 256 / ld;
  if (by < 1) by = 1;
  int nblocks = (int)((rows + by * 8 - 1) / (by * 8));
  if (nblocks > 1024) nblocks = 1024;
  if (nblocks < 1) nblocks = 1;
  double* partial = scratch.as<double>((size_t)nblocks * ld);
  hipLaunchKernelGGL((colsum_partial_kernel<T>), dim3(nblocks), dim3(ld, by), (size_t)by * ld * sizeof(double), s, P,
                     rows, ld, w, partial);
  hipLaunchKernelGGL((colsum_final_kernel<T>), dim3(ld), dim3(64), 0, s, partial, nblocks, ld, out);
  SAPCA_HIP(hipGetLastError());
}

#define INSTANTIATE(T)                                                                            \
  template void gram<T>(T*, int64_t, int, double*, DevBuf&, hipStream_t, const PanelSource<T>*, const T*, double*); \
  template void materialize<T>(T*, int64_t, int, const PanelSource<T>&, hipStream_t);             \
  template void weighted_colsum<T>(const T*, int64_t, int, const T*, T*, DevBuf&, hipStream_t);
INSTANTIATE(float)
INSTANTIATE(double)
#undef INSTANTIATE

}  // namespace k
}  // namespace sapca
