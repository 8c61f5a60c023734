// K-means on dense row panels (sapca_kmeans_*): seed -> (rank -> refine -> sort -> sums -> finalize -> step)* -> distances.
//
// rank: the assignment is knn.hip's ranking problem with the centroids as the corpus, maximise 2 <x_i, c> - |c|^2.  A workgroup
// owns 64 rows (16 per wave) and streams 64-centroid tiles through LDS onto v_mfma_f32_16x16x4_f32 / v_mfma_f64_16x16x4_f64;
// every lane keeps the best and the second-best score of its four rows over the columns it sees, and the 16 lanes of a row
// merge at the end.  A pair's score is the same k-ordered FMA chain wherever it falls, so the labels do not depend on the
// launch geometry.  refine: a row whose runner-up lies within the rounding of the scores is listed (an integer atomic hands
// out the list's slots) and decided by the k direct distances in f64 under (distance, index).
// update: a counting sort of the rows by (label, row) -- every wave counts a fixed run of rows, the table is scanned in
// (cluster, wave) order, every wave places its rows behind its own offsets in row order -- then f64 sums over fixed slices of
// each cluster's list, folded in order.  Integer atomics count; no floating-point atomic and no order reaches a value.
// Every kernel of the loop returns at once when the control block says the run has converged, so the host enqueues
// iterations without reading anything back.
#include <algorithm>
#include <cmath>
#include <limits>

#include "hash_u01.h"
#include "kernels.h"
#include "rank_tile.h"

namespace sapca {
namespace k {

namespace {

constexpr int kKmMaxClusters = SAPCA_KMEANS_MAX_CLUSTERS;
constexpr int kSeedBlock = 1024;   // rows per block of the seeding's prefix sums
constexpr uint64_t kSeedStream = 21;

__device__ inline bool km_skipped(const unsigned long long* skip) { return skip != nullptr && *skip != 0; }

// ---- assignment ----------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kKnnThreads) void km_rank_kernel(const unsigned long long* skip, const T* __restrict__ x, int64_t ldx, int64_t m,
                                                               const T* __restrict__ cen, int k, const T* __restrict__ bias,
                                                               const T* __restrict__ xb, int d, int32_t* __restrict__ labels,
                                                               int32_t* __restrict__ amb_list, unsigned long long* __restrict__ ctl) {
  if (km_skipped(skip)) return;
  constexpr int KC = KnnChunk<T>::value, LD = KC + 4, QB = 64;
  using Acc = typename KnnAcc<T>::type;
  __shared__ __align__(16) T Qs[QB * LD];
  __shared__ __align__(16) T Cs[kKnnTile * LD];
  __shared__ double s_max[kKnnThreads / 64];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t q0 = (int64_t)blockIdx.x * QB;

  double mx = 0.0;   // max |c|^2
  for (int c = tid; c < k; c += kKnnThreads) mx = fmax(mx, -(double)bias[c]);
  for (int off = 32; off >= 1; off >>= 1) mx = fmax(mx, __shfl_xor(mx, off));
  if (lane == 0) s_max[wave] = mx;   // (read behind the sweep's barriers: k >= 1 and d >= 1 give at least one step)

  const int ntiles = (k + kKnnTile - 1) / kKnnTile;
  const int nchunks = (d + KC - 1) / KC;
  const bool single = nchunks == 1;   // the rows' only chunk stays in LDS for the whole sweep
  const int steps = ntiles * nchunks;
  T qr[QB * KC / kKnnThreads], cr[kKnnTile * KC / kKnnThreads];
  if (single) {
    knn_chunk_load<T, QB, KC>(x, ldx, q0, m, 0, d, qr);
    knn_chunk_store<T, QB, KC>(qr, Qs);
  }
  knn_chunk_load<T, kKnnTile, KC>(cen, d, 0, k, 0, d, cr);
  if (!single) knn_chunk_load<T, QB, KC>(x, ldx, q0, m, 0, d, qr);

  T best[4], second[4];
  int besti[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    best[r] = -INFINITY;
    second[r] = -INFINITY;
    besti[r] = kKnnEmpty;
  }
  Acc acc[4];
  for (int step = 0; step < steps; ++step) {
    const int t = step / nchunks, ch = step % nchunks;
    __syncthreads();   // every wave is done with the previous chunk
    knn_chunk_store<T, kKnnTile, KC>(cr, Cs);
    if (!single) knn_chunk_store<T, QB, KC>(qr, Qs);
    __syncthreads();
    if (step + 1 < steps) {   // the next chunk travels while this one is multiplied
      const int tn = (step + 1) / nchunks, kn = ((step + 1) % nchunks) * KC;
      knn_chunk_load<T, kKnnTile, KC>(cen, d, (int64_t)tn * kKnnTile, k, kn, d, cr);
      if (!single) knn_chunk_load<T, QB, KC>(x, ldx, q0, m, kn, d, qr);
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
    if (ch != nchunks - 1) continue;
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
      const int j = t * kKnnTile + ct * 16 + (lane & 15);
      if (j >= k) continue;
      const T bj = bias[j];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const T sc = (T)2 * acc[ct][r] + bj;
        if (knn_better(sc, j, best[r], besti[r])) {
          second[r] = best[r];
          best[r] = sc;
          besti[r] = j;
        } else if (sc > second[r]) {
          second[r] = sc;
        }
      }
    }
  }
  // the 16 lanes that hold a row's columns
#pragma unroll
  for (int off = 1; off < 16; off <<= 1)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const T ob = __shfl_xor(best[r], off), os = __shfl_xor(second[r], off);
      const int oi = __shfl_xor(besti[r], off);
      if (knn_better(ob, oi, best[r], besti[r])) {
        second[r] = best[r] > os ? best[r] : os;
        best[r] = ob;
        besti[r] = oi;
      } else if (ob > second[r]) {
        second[r] = ob;
      }
    }
  if ((lane & 15) != 0) return;
  const double maxc = sqrt(fmax(fmax(s_max[0], s_max[1]), fmax(s_max[2], s_max[3])));
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int64_t gi = q0 + wave * 16 + acc_row<T>(lane, r);
    if (gi >= m) continue;
    int lab = besti[r];
    bool a = true;   // no score compared at all (NaN everywhere): the refine pass settles it inside [0, k)
    if (lab == kKnnEmpty) {
      lab = 0;
    } else {
      const double sum = sqrt(fmax(-(double)xb[gi], 0.0)) + maxc;
      const double bound = 4.0 * (double)d * (double)std::numeric_limits<T>::epsilon() * sum * sum;
      a = !((double)best[r] - (double)second[r] > bound);
    }
    labels[gi] = lab;
    if (a) {   // (the list's order varies from run to run; every entry is decided on its own, so no result does)
      const unsigned long long pos = atomicAdd(ctl + kKmAmbiguous, 1ull);
      if (pos < (unsigned long long)m) amb_list[pos] = (int32_t)gi;
    }
  }
}

// |a - b|^2 by the direct formula in f64, one lane, columns in order
template <typename T>
__device__ inline double km_dist2(const T* a, const T* b, int d) {
  double s = 0.0;
  for (int t = 0; t < d; ++t) {
    const double df = (double)a[t] - (double)b[t];
    s = fma(df, df, s);
  }
  return s;
}

// a wave per listed row, the waves striding over the list
template <typename T>
__global__ __launch_bounds__(kKnnThreads) void km_refine_kernel(const unsigned long long* skip, const T* __restrict__ x, int64_t ldx, int64_t m,
                                                                 const T* __restrict__ cen, int k, int d, int32_t* __restrict__ labels,
                                                                 const int32_t* __restrict__ amb_list,
                                                                 const unsigned long long* __restrict__ ctl) {
  if (km_skipped(skip)) return;
  const int lane = (int)threadIdx.x & 63;
  const unsigned long long listed = ctl[kKmAmbiguous];
  const int64_t n = listed < (unsigned long long)m ? (int64_t)listed : m;
  const int64_t nwaves = (int64_t)gridDim.x * (kKnnThreads / 64);
  for (int64_t e = (int64_t)blockIdx.x * (kKnnThreads / 64) + ((int)threadIdx.x >> 6); e < n; e += nwaves) {
    const int64_t i = amb_list[e];
    if (i < 0 || i >= m) continue;
    double bd = INFINITY;
    int bi = kKnnEmpty;
    for (int c = lane; c < k; c += 64) {
      const double dd = km_dist2(x + i * ldx, cen + (int64_t)c * d, d);
      if (dd < bd || (dd == bd && c < bi)) { bd = dd; bi = c; }
    }
    for (int off = 32; off >= 1; off >>= 1) {
      const double od = __shfl_xor(bd, off);
      const int oi = __shfl_xor(bi, off);
      if (od < bd || (od == bd && oi < bi)) { bd = od; bi = oi; }
    }
    if (lane == 0) labels[i] = bi == kKnnEmpty ? 0 : bi;   // (every distance NaN: inside [0, k) all the same)
  }
}

// s + c <- s + c + (a - b)^2 with the difference as an exact pair (hi, lo): hi^2 by knn_acc_prod, 2 hi lo into the correction
__device__ inline void km_acc_sqdiff(double& s, double& c, double a, double b) {
#pragma clang fp contract(off)
  const double hi = a - b;
  const double bb = hi - a;
  const double lo = (a - (hi - bb)) + (-b - bb);
  knn_acc_prod(s, c, hi, hi);
  c += 2.0 * hi * lo;
}

// a wave per row; compensated sums, so that the value is the direct formula's to within an ulp of f64 before its one rounding
template <typename T>
__global__ __launch_bounds__(kKnnThreads) void km_distances_kernel(const T* __restrict__ x, int64_t ldx, int64_t m, const T* __restrict__ cen, int k,
                                                                    int d, const int32_t* __restrict__ labels, T* __restrict__ dist2,
                                                                    double* __restrict__ rowd) {
  const int lane = (int)threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * (kKnnThreads / 64) + ((int)threadIdx.x >> 6);
  if (i >= m) return;
  const int lab = labels[i];
  double s = 0.0, c = 0.0;
  if (lab >= 0 && lab < k) {
    const T* a = x + i * ldx;
    const T* b = cen + (int64_t)lab * d;
    for (int t = lane; t < d; t += 64) km_acc_sqdiff(s, c, (double)a[t], (double)b[t]);
    for (int off = 32; off >= 1; off >>= 1) {
      const double os = __shfl_xor(s, off), oc = __shfl_xor(c, off);
      knn_acc_add(s, c, os);
      c += oc;
    }
  }
  if (lane == 0) {
    rowd[i] = s + c;
    if (dist2 != nullptr) dist2[i] = (T)(s + c);
  }
}

// ---- update: the counting sort ---------------------------------------------------------------------------------------------
// wave w owns the rows [w * rpw, (w + 1) * rpw); tab[c * nwaves + w] = its rows of cluster c, tab[k * nwaves] = 0.
// prev non-null: the rows whose label differs from prev[i] are counted into ctl[kKmChanged] on the way.
__global__ __launch_bounds__(256) void km_count_kernel(const unsigned long long* skip, const int32_t* __restrict__ labels, int64_t m, int k,
                                                       int64_t rpw, int64_t nwaves, int64_t* __restrict__ tab,
                                                       const int32_t* __restrict__ prev, unsigned long long* __restrict__ ctl) {
  if (km_skipped(skip)) return;
  __shared__ int hist[4][kKmMaxClusters];
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  const int64_t w = (int64_t)blockIdx.x * 4 + wave;
  for (int c = lane; c < k; c += 64) hist[wave][c] = 0;
  __syncthreads();
  if (w < nwaves) {
    const int64_t lo = w * rpw, hi = lo + rpw < m ? lo + rpw : m;
    int changed = 0;
    for (int64_t i = lo + lane; i < hi; i += 64) {
      const int lab = labels[i];
      if (lab >= 0 && lab < k) atomicAdd(&hist[wave][lab], 1);
      if (prev != nullptr && prev[i] != lab) ++changed;
    }
    for (int off = 32; off >= 1; off >>= 1) changed += __shfl_xor(changed, off);
    if (lane == 0 && changed > 0) atomicAdd(ctl + kKmChanged, (unsigned long long)changed);
  }
  __syncthreads();
  if (w < nwaves)
    for (int c = lane; c < k; c += 64) tab[(int64_t)c * nwaves + w] = hist[wave][c];
  if (blockIdx.x == 0 && threadIdx.x == 0) tab[(int64_t)k * nwaves] = 0;
}

// after the scan of tab: wave w writes its rows of cluster c at tab[c * nwaves + w] onwards, in row order
__global__ __launch_bounds__(256) void km_place_kernel(const unsigned long long* skip, const int32_t* __restrict__ labels, int64_t m, int k,
                                                       int64_t rpw, int64_t nwaves, const int64_t* __restrict__ tab,
                                                       int32_t* __restrict__ order) {
  if (km_skipped(skip)) return;
  __shared__ int cursor[4][kKmMaxClusters];
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  const int64_t w = (int64_t)blockIdx.x * 4 + wave;
  if (w >= nwaves) return;   // (no workgroup barrier below: a wave works alone on its own LDS row)
  for (int c = lane; c < k; c += 64) cursor[wave][c] = (int)tab[(int64_t)c * nwaves + w];
  __builtin_amdgcn_wave_barrier();
  const int64_t lo = w * rpw, hi = lo + rpw < m ? lo + rpw : m;
  const unsigned long long below = (1ull << lane) - 1ull;
  for (int64_t i0 = lo; i0 < hi; i0 += 64) {
    const int64_t i = i0 + lane;
    const int lab = i < hi ? labels[i] : -1;
    const bool valid = lab >= 0 && lab < k;
    unsigned long long todo = __ballot(valid);
    while (todo) {   // one cluster of this step's rows at a time; the LDS operations of one wave complete in program order
      const int src = __ffsll((long long)todo) - 1;
      const int cl = __shfl(lab, src);
      const unsigned long long same = __ballot(valid && lab == cl);
      if (valid && lab == cl) {
        const int64_t pos = (int64_t)cursor[wave][cl] + __popcll(same & below);
        if (pos >= 0 && pos < m) order[pos] = (int32_t)i;   // (always, unless the labels changed under the two passes)
      }
      __builtin_amdgcn_wave_barrier();
      if (lane == src) cursor[wave][cl] += __popcll(same);
      __builtin_amdgcn_wave_barrier();
      todo &= ~same;
    }
  }
}

// ---- update: the sums ------------------------------------------------------------------------------------------------------
// grid (slices, clusters).  The 256 threads are 256 / DT row lanes of DT columns (DT = 64, 128 or 256 by d): row lane r adds
// the rows r, r + 256 / DT, .. of the slice in list order, then the row lanes are added in order.
template <typename T>
__global__ __launch_bounds__(256) void km_sums_kernel(const unsigned long long* skip, const T* __restrict__ x, int64_t ldx, int64_t m, int d,
                                                      const int32_t* __restrict__ order, const int64_t* __restrict__ tab, int64_t nwaves,
                                                      int slices, const double* __restrict__ center, double* __restrict__ partial) {
  if (km_skipped(skip)) return;
  __shared__ double buf[4][256];
  const int tid = (int)threadIdx.x, c = (int)blockIdx.y, sl = (int)blockIdx.x;
  const int64_t o0 = tab ? tab[(int64_t)c * nwaves] : 0, o1 = tab ? tab[(int64_t)(c + 1) * nwaves] : m;
  const int64_t n = o1 - o0, len = (n + slices - 1) / slices;
  const int64_t p0 = o0 + sl * len, p1 = p0 + len < o1 ? p0 + len : o1;
  const int DT = d <= 64 ? 64 : (d <= 128 ? 128 : 256), RL = 256 / DT;
  const int tc = tid % DT, tr = tid / DT;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (int64_t p = p0 + tr; p < p1; p += RL) {
    const int64_t row = order ? (int64_t)order[p] : p;
    if (row < 0 || row >= m) continue;
    const T* xr = x + row * ldx;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int t = tc + j * 256;
      if (t >= d || (j > 0 && DT < 256)) continue;
      double v = (double)xr[t];
      if (center) {
        v -= center[t];
        acc[j] = fma(v, v, acc[j]);
      } else {
        acc[j] += v;
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) buf[j][tid] = acc[j];
  __syncthreads();
  if (tr != 0) return;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int t = tc + j * 256;
    if (t >= d || (j > 0 && DT < 256)) continue;
    double sum = buf[j][tc];
    for (int r = 1; r < RL; ++r) sum += buf[j][r * DT + tc];
    partial[((int64_t)c * slices + sl) * d + t] = sum;
  }
}

// sum of one value per thread of a 256-thread workgroup in an order fixed by the thread index, on every thread
__device__ inline double km_block_sum(double v, double* sh) {
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
__global__ __launch_bounds__(256) void km_finalize_kernel(const unsigned long long* skip, const double* __restrict__ partial,
                                                          const int64_t* __restrict__ tab, int64_t nwaves, int d, int slices,
                                                          T* __restrict__ cen, int64_t* __restrict__ counts, double* __restrict__ shiftpart) {
  if (km_skipped(skip)) return;
  __shared__ double sh[256];
  const int c = (int)blockIdx.x;
  const int64_t n = tab[(int64_t)(c + 1) * nwaves] - tab[(int64_t)c * nwaves];
  double shift = 0.0;
  if (n > 0) {
    for (int t = (int)threadIdx.x; t < d; t += 256) {
      double sum = 0.0;
      for (int sl = 0; sl < slices; ++sl) sum += partial[((int64_t)c * slices + sl) * d + t];
      const T fresh = (T)(sum / (double)n);
      const double df = (double)fresh - (double)cen[(int64_t)c * d + t];
      shift = fma(df, df, shift);
      cen[(int64_t)c * d + t] = fresh;
    }
  }
  shift = km_block_sum(shift, sh);
  if (threadIdx.x == 0) {
    shiftpart[c] = shift;
    if (counts != nullptr) counts[c] = n;
  }
}

__global__ __launch_bounds__(64) void km_step_kernel(unsigned long long* __restrict__ ctl, const double* __restrict__ shiftpart, int k,
                                                     const double* __restrict__ tol_abs, unsigned long long iter) {
  if (ctl[kKmDone]) return;
  const int lane = (int)threadIdx.x;
  double shift = 0.0;
  for (int c = lane; c < k; c += 64) shift += shiftpart[c];
  for (int off = 32; off >= 1; off >>= 1) shift += __shfl_xor(shift, off);
  if (lane != 0) return;
  ctl[kKmIter] = iter + 1;
  if (iter > 0 && ctl[kKmChanged] == 0) {
    ctl[kKmStrict] = 1;
    ctl[kKmDone] = 1;
  } else if (shift <= *tol_abs) {
    ctl[kKmDone] = 1;
  }
  ctl[kKmChanged] = 0;
  ctl[kKmAmbiguous] = 0;   // the next assignment lists its own
}

__global__ __launch_bounds__(256) void km_fold_columns_kernel(const double* __restrict__ partial, int slices, int d, int64_t m,
                                                              double* __restrict__ cols, double scale, double* __restrict__ scalar) {
  for (int t = (int)threadIdx.x; t < d; t += 256) {
    double sum = 0.0;
    for (int sl = 0; sl < slices; ++sl) sum += partial[(int64_t)sl * d + t];
    cols[t] = sum / (double)m;
  }
  __syncthreads();
  if (threadIdx.x == 0 && scalar != nullptr) {
    double sum = 0.0;
    for (int t = 0; t < d; ++t) sum += cols[t];
    *scalar = scale * (sum / (double)d);
  }
}

__global__ __launch_bounds__(256) void km_take_labels_kernel(const unsigned long long* __restrict__ ctl, const int32_t* __restrict__ lab0,
                                                             const int32_t* __restrict__ lab1, int32_t* __restrict__ out, int64_t m) {
  if (!ctl[kKmStrict]) return;
  const int32_t* from = ((ctl[kKmIter] - 1) & 1) ? lab1 : lab0;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < m) out[i] = from[i];
}

// ---- seeding ---------------------------------------------------------------------------------------------------------------
// inclusive prefix sums of one value per thread of a 1024-thread workgroup, associated by the thread index alone: inside a
// wave by doubling strides, then behind the totals of the waves before it, added in order.  sh: 16 doubles.
__device__ inline double km_block_scan(double v, double* sh) {
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  for (int off = 1; off < 64; off <<= 1) {
    const double o = __shfl_up(v, off);
    if (lane >= off) v += o;
  }
  __syncthreads();   // (sh may still be read from the call before)
  if (lane == 63) sh[wave] = v;
  __syncthreads();
  double base = 0.0;
  for (int w = 0; w < wave; ++w) base += sh[w];
  return wave ? base + v : v;
}

// dist[i] = min(dist[i], |x_i - x_rows[t - 1]|^2) (t == 1: the distance itself); bsum[b] = the sum of block b's 1024 values,
// as the last element of km_block_scan gives it
template <typename T>
__global__ __launch_bounds__(kSeedBlock) void km_seed_dist_kernel(const T* __restrict__ x, int64_t ldx, int64_t m, int d,
                                                                  const int32_t* __restrict__ rows, int t, double* __restrict__ dist,
                                                                  double* __restrict__ bsum) {
  __shared__ double sh[16];
  const int64_t i = (int64_t)blockIdx.x * kSeedBlock + threadIdx.x;
  double v = 0.0;
  if (i < m) {
    v = km_dist2(x + i * ldx, x + (int64_t)rows[t - 1] * ldx, d);
    if (t > 1) v = fmin(dist[i], v);
    dist[i] = v;
  }
  const double s = km_block_scan(v, sh);
  if (threadIdx.x == kSeedBlock - 1) bsum[blockIdx.x] = s;
}

// One chunk of up to 1024 block sums behind `carry`: excl = the sum in front of this thread's block, incl = excl + its own;
// the carry becomes the incl of the chunk's last block (`last`).  buf: 1024 doubles.
__device__ inline void km_chunk_prefix(double v, int last, double& carry, double* sh, double* buf, double& excl, double& incl) {
  const int tid = (int)threadIdx.x;
  const double sc = km_block_scan(v, sh);
  __syncthreads();   // (buf may still be read from the chunk before)
  buf[tid] = sc;
  __syncthreads();
  excl = carry + (tid ? buf[tid - 1] : 0.0);
  incl = excl + v;
  __syncthreads();
  buf[tid] = incl;
  __syncthreads();
  carry = buf[last];
}

// One workgroup picks centre t: the total S and the block prefixes from bsum, the first block whose end lies above u_t S,
// that block's own prefix sums (the same km_block_scan on the same values: its last element is the block sum that put the
// block's end above the threshold, so a row is always found), the first row above it, and the row's copy into cen[t].
template <typename T>
__global__ __launch_bounds__(kSeedBlock) void km_seed_pick_kernel(const T* __restrict__ x, int64_t ldx, int64_t m, int d, uint64_t seed, int t,
                                                                  const double* __restrict__ dist, const double* __restrict__ bsum,
                                                                  int64_t nb, int32_t* __restrict__ rows, T* __restrict__ cen) {
  __shared__ double sh[16];
  __shared__ double buf[kSeedBlock];
  __shared__ double s_excl;
  __shared__ unsigned s_first;
  constexpr unsigned kNone = 0xFFFFFFFFu;
  const int tid = (int)threadIdx.x;
  const double u = hash_u01(seed, kSeedStream, (uint64_t)t);
  int64_t pick = (int64_t)floor(u * (double)m);   // centre 0, and the fallback when every row coincides with a chosen centre
  if (pick > m - 1) pick = m - 1;
  if (t > 0) {
    double carry = 0.0, excl, incl;
    for (int64_t c0 = 0; c0 < nb; c0 += kSeedBlock) {
      const int last = (int)(nb - 1 - c0 < kSeedBlock - 1 ? nb - 1 - c0 : kSeedBlock - 1);
      km_chunk_prefix(c0 + tid < nb ? bsum[c0 + tid] : 0.0, last, carry, sh, buf, excl, incl);
    }
    const double total = carry;
    if (total > 0.0) {
      const double thr = u * total;
      if (tid == 0) s_first = kNone;   // (the barriers of the scan order this before the atomics)
      carry = 0.0;
      int64_t blk = -1;
      for (int64_t c0 = 0; c0 < nb && blk < 0; c0 += kSeedBlock) {
        const int last = (int)(nb - 1 - c0 < kSeedBlock - 1 ? nb - 1 - c0 : kSeedBlock - 1);
        km_chunk_prefix(c0 + tid < nb ? bsum[c0 + tid] : 0.0, last, carry, sh, buf, excl, incl);
        if (c0 + tid < nb && incl > thr) atomicMin(&s_first, (unsigned)tid);
        __syncthreads();
        if (s_first != kNone) {
          blk = c0 + s_first;
          if (tid == (int)s_first) s_excl = excl;
        }
        __syncthreads();
      }
      double before = 0.0;
      if (blk < 0) blk = nb - 1;   // (a NaN among the sums: unspecified, but inside the arrays)
      else before = s_excl;
      __syncthreads();
      if (tid == 0) s_first = kNone;
      const int64_t i = blk * kSeedBlock + tid;
      const double sc = km_block_scan(i < m ? dist[i] : 0.0, sh);
      if (i < m && before + sc > thr) atomicMin(&s_first, (unsigned)tid);
      __syncthreads();
      pick = blk * kSeedBlock + (s_first != kNone ? (int64_t)s_first : kSeedBlock - 1);
      if (pick > m - 1) pick = m - 1;
    }
  }
  if (tid == 0) rows[t] = (int32_t)pick;
  if (tid < d) cen[(int64_t)t * d + tid] = x[pick * ldx + tid];
}

unsigned blocks_for(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

}  // namespace

KmeansPlan kmeans_plan(int64_t m, int k) {
  KmeansPlan p;
  p.rows_per_wave = std::max<int64_t>(256, round_up((m + 8191) / 8192, 64));   // at most 8192 waves
  p.nwaves = std::max<int64_t>((m + p.rows_per_wave - 1) / p.rows_per_wave, 1);
  p.slices = (int)std::min<int64_t>(64, std::max<int64_t>(1, m / (64 * (int64_t)std::max(k, 1))));   // about 64 rows or more per slice
  return p;
}

int kmeans_column_slices(int64_t m) { return (int)std::min<int64_t>(1024, std::max<int64_t>(1, m / 256)); }

template <typename T>
void kmeans_seed(const T* x, int64_t ldx, int64_t m, int d, int k, uint32_t seed, T* cen, int32_t* rows, double* dist, double* bsum,
                 hipStream_t s) {
  if (m <= 0) return;
  const int64_t nb = (m + kSeedBlock - 1) / kSeedBlock;
  for (int t = 0; t < k; ++t) {
    if (t > 0)
      hipLaunchKernelGGL((km_seed_dist_kernel<T>), dim3((unsigned)nb), dim3(kSeedBlock), 0, s, x, ldx, m, d, rows, t, dist, bsum);
    hipLaunchKernelGGL((km_seed_pick_kernel<T>), dim3(1), dim3(kSeedBlock), 0, s, x, ldx, m, d, (uint64_t)seed, t, dist, bsum, nb, rows, cen);
  }
  SAPCA_HIP(hipGetLastError());
}

template <typename T>
void kmeans_rank(const unsigned long long* skip, const T* x, int64_t ldx, int64_t m, const T* cen, int k, const T* bias, const T* xb, int d,
                 int32_t* labels, int32_t* amb_list, unsigned long long* ctl, hipStream_t s) {
  if (m <= 0) return;
  hipLaunchKernelGGL((km_rank_kernel<T>), dim3(blocks_for(m, 64)), dim3(kKnnThreads), 0, s, skip, x, ldx, m, cen, k, bias, xb, d, labels,
                     amb_list, ctl);
  SAPCA_HIP(hipGetLastError());
}

template <typename T>
void kmeans_refine(const unsigned long long* skip, const T* x, int64_t ldx, int64_t m, const T* cen, int k, int d, int32_t* labels,
                   const int32_t* amb_list, const unsigned long long* ctl, hipStream_t s) {
  if (m <= 0) return;
  const unsigned blocks = std::min(blocks_for(m, kKnnThreads / 64), 1024u);
  hipLaunchKernelGGL((km_refine_kernel<T>), dim3(blocks), dim3(kKnnThreads), 0, s, skip, x, ldx, m, cen, k, d, labels, amb_list, ctl);
  SAPCA_HIP(hipGetLastError());
}

template <typename T>
void kmeans_distances(const T* x, int64_t ldx, int64_t m, const T* cen, int k, int d, const int32_t* labels, T* dist2, double* rowd,
                      hipStream_t s) {
  if (m <= 0) return;
  hipLaunchKernelGGL((km_distances_kernel<T>), dim3(blocks_for(m, kKnnThreads / 64)), dim3(kKnnThreads), 0, s, x, ldx, m, cen, k, d, labels,
                     dist2, rowd);
  SAPCA_HIP(hipGetLastError());
}

void kmeans_sort(const unsigned long long* skip, const int32_t* labels, int64_t m, int k, const KmeansPlan& plan, int64_t* cnt,
                 int64_t* tab, int32_t* order, DevBuf& scan, const int32_t* prev, unsigned long long* ctl, hipStream_t s) {
  const unsigned blocks = blocks_for(plan.nwaves, 4);
  hipLaunchKernelGGL(km_count_kernel, dim3(blocks), dim3(256), 0, s, skip, labels, m, k, plan.rows_per_wave, plan.nwaves, cnt, prev, ctl);
  exclusive_scan_i64(cnt, (int64_t)k * plan.nwaves + 1, scan, 0, s, tab);   // (never skipped: the same counts give the same offsets)
  hipLaunchKernelGGL(km_place_kernel, dim3(blocks), dim3(256), 0, s, skip, labels, m, k, plan.rows_per_wave, plan.nwaves, tab, order);
  SAPCA_HIP(hipGetLastError());
}

template <typename T>
void kmeans_sums(const unsigned long long* skip, const T* x, int64_t ldx, int64_t m, int d, const int32_t* order, const int64_t* tab,
                 int64_t nwaves, int k, int slices, const double* center, double* partial, hipStream_t s) {
  hipLaunchKernelGGL((km_sums_kernel<T>), dim3((unsigned)slices, (unsigned)k), dim3(256), 0, s, skip, x, ldx, m, d, order, tab, nwaves, slices,
                     center, partial);
  SAPCA_HIP(hipGetLastError());
}

template <typename T>
void kmeans_finalize(const unsigned long long* skip, const double* partial, const int64_t* tab, int64_t nwaves, int k, int d, int slices,
                     T* cen, int64_t* counts, double* shiftpart, hipStream_t s) {
  hipLaunchKernelGGL((km_finalize_kernel<T>), dim3((unsigned)k), dim3(256), 0, s, skip, partial, tab, nwaves, d, slices, cen, counts, shiftpart);
  SAPCA_HIP(hipGetLastError());
}

void kmeans_step(unsigned long long* ctl, const double* shiftpart, int k, const double* tol_abs, unsigned long long iter, hipStream_t s) {
  hipLaunchKernelGGL(km_step_kernel, dim3(1), dim3(64), 0, s, ctl, shiftpart, k, tol_abs, iter);
  SAPCA_HIP(hipGetLastError());
}

void kmeans_fold_columns(const double* partial, int slices, int d, int64_t m, double* cols, double scale, double* scalar, hipStream_t s) {
  hipLaunchKernelGGL(km_fold_columns_kernel, dim3(1), dim3(256), 0, s, partial, slices, d, m, cols, scale, scalar);
  SAPCA_HIP(hipGetLastError());
}

void kmeans_take_labels(const unsigned long long* ctl, const int32_t* lab0, const int32_t* lab1, int32_t* out, int64_t m, hipStream_t s) {
  if (m <= 0) return;
  hipLaunchKernelGGL(km_take_labels_kernel, dim3(blocks_for(m, 256)), dim3(256), 0, s, ctl, lab0, lab1, out, m);
  SAPCA_HIP(hipGetLastError());
}

#define SAPCA_INSTANTIATE_KMEANS(T)                                                                                                    \
  template void kmeans_seed<T>(const T*, int64_t, int64_t, int, int, uint32_t, T*, int32_t*, double*, double*, hipStream_t);           \
  template void kmeans_rank<T>(const unsigned long long*, const T*, int64_t, int64_t, const T*, int, const T*, const T*, int, int32_t*, \
                               int32_t*, unsigned long long*, hipStream_t);                                                            \
  template void kmeans_refine<T>(const unsigned long long*, const T*, int64_t, int64_t, const T*, int, int, int32_t*, const int32_t*,  \
                                 const unsigned long long*, hipStream_t);                                                              \
  template void kmeans_distances<T>(const T*, int64_t, int64_t, const T*, int, int, const int32_t*, T*, double*, hipStream_t);         \
  template void kmeans_sums<T>(const unsigned long long*, const T*, int64_t, int64_t, int, const int32_t*, const int64_t*, int64_t,    \
                               int, int, const double*, double*, hipStream_t);                                                         \
  template void kmeans_finalize<T>(const unsigned long long*, const double*, const int64_t*, int64_t, int, int, int, T*, int64_t*,     \
                                   double*, hipStream_t);
SAPCA_INSTANTIATE_KMEANS(float)
SAPCA_INSTANTIATE_KMEANS(double)
#undef SAPCA_INSTANTIATE_KMEANS

}  // namespace k
}  // namespace sapca
