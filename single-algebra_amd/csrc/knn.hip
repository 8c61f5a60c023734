// Exact k-nearest neighbours of dense row panels (sapca_knn_device_*): prepare -> select -> (merge) -> refine.
//
// All three metrics are one ranking problem, maximise s(i, j) = alpha <a_i, b_j> + bias_j:
//   EUCLIDEAN  alpha = 2, bias_j = -|b_j|^2 on the rows as they are (|a_i|^2 is constant per query and ranks nothing);
//   COSINE     alpha = 1, bias = 0 on rows scaled to unit norm;  PEARSON the same on rows centred first.
// select: a workgroup owns 64 * MT query rows (16 * MT per wave) and streams 64-row corpus tiles through LDS; the inner
// products run on v_mfma_f32_16x16x4_f32 / v_mfma_f64_16x16x4_f64 (one operand element per lane in both; the C/D row maps
// differ, acc_row below), MT * 4 independent accumulators per wave.  Every score is compared with the worst entry of its
// query's list (sorted, in LDS, private to the wave that owns the row); the few survivors are inserted one at a time by the
// whole wave.  The key is (score, -index), so ties go to the lower corpus index inside the kernel.  The score of a pair is
// the same k-ordered FMA chain wherever the pair falls in a tile, a block or a corpus split, so the selected SET does not
// depend on the launch geometry.  No atomics; every output word has one writer.
// refine: the inner-product form cancels for close neighbours, so the values are recomputed for the selected pairs only,
// from the original rows in f64 (compensated sums), rounded once to T, and each list is re-sorted by (value, index).
#include <algorithm>
#include <climits>
#include <cmath>
#include <limits>
#include <type_traits>

#include "kernels.h"
#include "rank_tile.h"

namespace sapca {
namespace k {

namespace {

// One candidate into a sorted list of k <= 128 entries by the whole wave: lane l owns positions l and l + 64; an entry the
// candidate ranks before moves one place down (the last one leaves).  Every lane reads before any lane writes (LDS
// operations of one wave complete in program order).  A candidate that ranks behind the whole list changes nothing.
template <typename T>
__device__ inline void knn_insert(T* sc, int32_t* ix, int k, T s, int j, int lane) {
  const int p0 = lane, p1 = lane + 64;
  const bool in0 = p0 < k, in1 = p1 < k;
  T e0s = 0, e1s = 0, q0s = 0, q1s = 0;
  int e0i = 0, e1i = 0, q0i = 0, q1i = 0;
  if (in0) {
    e0s = sc[p0]; e0i = ix[p0];
    if (p0 > 0) { q0s = sc[p0 - 1]; q0i = ix[p0 - 1]; }
  }
  if (in1) {
    e1s = sc[p1]; e1i = ix[p1];
    q1s = sc[p1 - 1]; q1i = ix[p1 - 1];
  }
  __builtin_amdgcn_wave_barrier();
  if (in0 && !knn_better(e0s, e0i, s, j)) {
    const bool here = p0 == 0 || knn_better(q0s, q0i, s, j);
    sc[p0] = here ? s : q0s;
    ix[p0] = here ? j : q0i;
  }
  if (in1 && !knn_better(e1s, e1i, s, j)) {
    const bool here = knn_better(q1s, q1i, s, j);
    sc[p1] = here ? s : q1s;
    ix[p1] = here ? j : q1i;
  }
  __builtin_amdgcn_wave_barrier();
}

// grid (query blocks, corpus splits).  part_sc / part_ix: [query][split][k], each list sorted best first
template <typename T, int MT>
__global__ __launch_bounds__(kKnnThreads, 2) void knn_select_kernel(const T* __restrict__ q, int64_t ldq, int64_t mq,
                                                                 const T* __restrict__ c, int64_t ldc, int64_t mc,
                                                                 const T* __restrict__ bias, int d, T alpha, int k, int exclude_self,
                                                                 int tiles_per_split, T* __restrict__ part_sc,
                                                                 int32_t* __restrict__ part_ix) {
  constexpr int KC = KnnChunk<T>::value, LD = KC + 4, QB = 64 * MT, RW = 16 * MT;
  using Acc = typename KnnAcc<T>::type;
  extern __shared__ __align__(16) unsigned char knn_smem[];
  T* Qs = reinterpret_cast<T*>(knn_smem);            // QB x LD
  T* Cs = Qs + QB * LD;                              // kKnnTile x LD
  T* Lsc = Cs + kKnnTile * LD;                       // QB x k scores
  int32_t* Lix = reinterpret_cast<int32_t*>(Lsc + QB * k);   // QB x k corpus rows

  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t q0 = (int64_t)blockIdx.x * QB;
  const int nsplit = (int)gridDim.y, split = (int)blockIdx.y;
  const int64_t ntiles = (mc + kKnnTile - 1) / kKnnTile;
  const int64_t t0 = (int64_t)split * tiles_per_split;
  const int64_t t1 = t0 + tiles_per_split < ntiles ? t0 + tiles_per_split : ntiles;
  const int nchunks = (d + KC - 1) / KC;
  const bool single = nchunks == 1;   // the queries' only chunk stays in LDS for the whole sweep

  for (int e = tid; e < QB * k; e += kKnnThreads) {
    Lsc[e] = -INFINITY;
    Lix[e] = kKnnEmpty;
  }
  T qr[QB * KC / kKnnThreads], cr[kKnnTile * KC / kKnnThreads];
  const int64_t steps = t1 > t0 ? (t1 - t0) * nchunks : 0;
  if (single) {
    knn_chunk_load<T, QB, KC>(q, ldq, q0, mq, 0, d, qr);
    knn_chunk_store<T, QB, KC>(qr, Qs);
  }
  if (steps > 0) {
    knn_chunk_load<T, kKnnTile, KC>(c, ldc, t0 * kKnnTile, mc, 0, d, cr);
    if (!single) knn_chunk_load<T, QB, KC>(q, ldq, q0, mq, 0, d, qr);
  }
  Acc acc[MT][4];
  for (int64_t step = 0; step < steps; ++step) {
    const int64_t t = t0 + step / nchunks;
    const int ch = (int)(step % nchunks);
    __syncthreads();   // every wave is done with the previous chunk (and, first, the lists are initialised)
    knn_chunk_store<T, kKnnTile, KC>(cr, Cs);
    if (!single) knn_chunk_store<T, QB, KC>(qr, Qs);
    __syncthreads();
    if (step + 1 < steps) {   // the next chunk travels while this one is multiplied
      const int64_t tn = t0 + (step + 1) / nchunks;
      const int kn = (int)((step + 1) % nchunks) * KC;
      knn_chunk_load<T, kKnnTile, KC>(c, ldc, tn * kKnnTile, mc, kn, d, cr);
      if (!single) knn_chunk_load<T, QB, KC>(q, ldq, q0, mq, kn, d, qr);
    }
    if (ch == 0) {
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int ct = 0; ct < 4; ++ct)
#pragma unroll
          for (int r = 0; r < 4; ++r) acc[mt][ct][r] = (T)0;
    }
    const bool last = ch == nchunks - 1;
    T bj[4];
    if (last) {
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) {
        const int64_t j = t * kKnnTile + ct * 16 + (lane & 15);
        bj[ct] = (bias != nullptr && j < mc) ? bias[j] : (T)0;
      }
    }
    const int left = d - ch * KC;
    const int ksteps = ((left < KC ? left : KC) + 3) / 4;   // d is padded to a multiple of 4 by the zeros in LDS
    const T* qa = Qs + (wave * RW + (lane & 15)) * LD + (lane >> 4);
    const T* cb = Cs + (lane & 15) * LD + (lane >> 4);
    for (int ks = 0; ks < ksteps; ++ks) {
      T a[MT];
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) a[mt] = qa[mt * 16 * LD + ks * 4];
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) {
        const T b = cb[ct * 16 * LD + ks * 4];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) acc[mt][ct] = knn_mfma(a[mt], b, acc[mt][ct]);
      }
    }
    if (!last) continue;
    // scores against the lists' worst entries; what survives goes in, one candidate at a time
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int ct = 0; ct < 4; ++ct)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[mt][ct][r] = alpha * acc[mt][ct][r] + bj[ct];
    // a tile that lies inside the corpus, under a block that lies inside the queries, away from the block's own rows when
    // they are excluded, needs one comparison per score to be dismissed (>=: no survivor of the exact test below is lost)
    const bool plain = (t + 1) * kKnnTile <= mc && q0 + QB <= mq &&
                       !(exclude_self && t * kKnnTile < q0 + QB && (t + 1) * kKnnTile > q0);
    if (plain) {
      bool any = false;
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const T ts = Lsc[(wave * RW + mt * 16 + acc_row<T>(lane, r)) * k + k - 1];
#pragma unroll
          for (int ct = 0; ct < 4; ++ct) any |= acc[mt][ct][r] >= ts;
        }
      if (__ballot(any) == 0) continue;
    }
    uint32_t cand = 0;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int rl = wave * RW + mt * 16 + acc_row<T>(lane, r);
        const int64_t gi = q0 + rl;
        const T ts = Lsc[rl * k + k - 1];
        const int ti = Lix[rl * k + k - 1];
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) {
          const int64_t j = t * kKnnTile + ct * 16 + (lane & 15);
          const bool ok = j < mc && gi < mq && !(exclude_self && j == gi) && knn_better(acc[mt][ct][r], (int)j, ts, ti);
          cand |= (ok ? 1u : 0u) << ((mt * 4 + ct) * 4 + r);
        }
      }
    if (__ballot(cand != 0) == 0) continue;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int ct = 0; ct < 4; ++ct)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          unsigned long long todo = __ballot((cand >> ((mt * 4 + ct) * 4 + r)) & 1u);
          while (todo) {
            const int src = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            const T s = __shfl(acc[mt][ct][r], src);
            const int rl = wave * RW + mt * 16 + acc_row<T>(src, r);
            const int j = (int)(t * kKnnTile + ct * 16 + (src & 15));
            knn_insert(Lsc + rl * k, Lix + rl * k, k, s, j, lane);
          }
        }
  }
  __syncthreads();   // (no tile at all: the lists' initialisation)
  for (int r = 0; r < RW; ++r) {
    const int rl = wave * RW + r;
    const int64_t gi = q0 + rl;
    if (gi >= mq) break;
    const int64_t o = (gi * nsplit + split) * k;
    for (int p = lane; p < k; p += 64) {
      part_sc[o + p] = Lsc[rl * k + p];
      part_ix[o + p] = Lix[rl * k + p];
    }
  }
}

// The best k of a query's nsplit <= 64 sorted lists, by the same key: lane l walks list l; a wave per query.
template <typename T>
__global__ __launch_bounds__(kKnnThreads) void knn_merge_kernel(const T* __restrict__ part_sc, const int32_t* __restrict__ part_ix,
                                                                int64_t mq, int nsplit, int k, int32_t* __restrict__ out_ix) {
  const int lane = (int)threadIdx.x & 63;
  const int64_t qi = (int64_t)blockIdx.x * (kKnnThreads / 64) + ((int)threadIdx.x >> 6);
  if (qi >= mq) return;
  const int64_t base = (qi * nsplit + lane) * k;
  const bool mine = lane < nsplit;
  int h = 0;
  T s = mine ? part_sc[base] : (T)-INFINITY;
  int i = mine ? part_ix[base] : kKnnEmpty;
  for (int p = 0; p < k; ++p) {
    T bs = s;
    int bi = i;
    for (int off = 32; off >= 1; off >>= 1) {
      const T os = __shfl_xor(bs, off);
      const int oi = __shfl_xor(bi, off);
      if (knn_better(os, oi, bs, bi)) { bs = os; bi = oi; }
    }
    if (lane == 0) out_ix[qi * k + p] = bi;
    if (mine && i == bi && bi != kKnnEmpty) {   // the splits' index ranges are disjoint: one lane advances
      ++h;
      s = h < k ? part_sc[base + h] : (T)-INFINITY;
      i = h < k ? part_ix[base + h] : kKnnEmpty;
    }
  }
}

// (hi, lo) = (s + c) / n to twice the working precision
__device__ inline void knn_mean(double s, double c, double n, double& hi, double& lo) {
#pragma clang fp contract(off)
  hi = s / n;
  lo = (fma(-hi, n, s) + c) / n;
}

// sqrt(s + c) and (s + c) / (r + rl) to twice the working precision, rounded once at the end: with the sums above this keeps
// the whole formula within an ulp of f64 (each plain f64 operation of it would cost up to one)
__device__ inline void knn_sqrt2(double s, double c, double& r, double& rl) {
#pragma clang fp contract(off)
  const double hi = s + c, lo = c - (hi - s);
  r = sqrt(hi);
  rl = r > 0 ? (fma(-r, r, hi) + lo) / (2.0 * r) : 0.0;
}
__device__ inline double knn_div2(double s, double c, double r, double rl) {
#pragma clang fp contract(off)
  const double hi = s + c, lo = c - (hi - s);
  const double q = hi / r;
  const double rem = (fma(-q, r, hi) - q * rl) + lo;
  return q + rem / r;
}

// The value of the pair (a, b) by the direct formula in f64: |a - b| (EUCLIDEAN), <a, b> / sqrt(|a|^2 |b|^2) (COSINE), the
// same on the centred rows (PEARSON: the reference's raw-moment expression, evaluated without its cancellation).  A row
// whose norm is <= zero_norm is the zero vector: similarity 0.
template <typename T>
__device__ inline double knn_pair_value(const T* a, const T* b, int d, int metric, double zero_norm) {
#pragma clang fp contract(off)
  double s = 0, sc = 0;
  if (metric == SAPCA_KNN_EUCLIDEAN) {
    for (int t = 0; t < d; ++t) {
      const double df = (double)a[t] - (double)b[t];
      knn_acc_prod(s, sc, df, df);
    }
    double r, rl;
    knn_sqrt2(s, sc, r, rl);
    return r + rl;
  }
  double mah = 0, mal = 0, mbh = 0, mbl = 0;
  if (metric == SAPCA_KNN_PEARSON) {
    double sa = 0, sac = 0, sb = 0, sbc = 0;
    for (int t = 0; t < d; ++t) {
      knn_acc_add(sa, sac, (double)a[t]);
      knn_acc_add(sb, sbc, (double)b[t]);
    }
    knn_mean(sa, sac, (double)d, mah, mal);
    knn_mean(sb, sbc, (double)d, mbh, mbl);
  }
  double na = 0, nac = 0, nb = 0, nbc = 0;
  for (int t = 0; t < d; ++t) {
    const double x = ((double)a[t] - mah) - mal, y = ((double)b[t] - mbh) - mbl;
    knn_acc_prod(s, sc, x, y);
    knn_acc_prod(na, nac, x, x);
    knn_acc_prod(nb, nbc, y, y);
  }
  if (!(sqrt(na + nac) > zero_norm) || !(sqrt(nb + nbc) > zero_norm)) return 0.0;
  // |a|^2 |b|^2 as a pair: the product of the two pairs, then its root and the quotient
  const double ah = na + nac, al = nac - (ah - na), bh = nb + nbc, bl = nbc - (bh - nb);
  const double p = ah * bh;
  const double pl = fma(ah, bh, -p) + (ah * bl + al * bh);
  double r, rl;
  knn_sqrt2(p, pl, r, rl);
  return knn_div2(s, sc, r, rl);
}

// A wave per query: the values of its k selected pairs, then the list sorted by (value, index) through each entry's rank.
// sel: [query][sel_stride] corpus rows (kKnnEmpty: never filled -> index -1, NaN, behind everything else).
template <typename T>
__global__ __launch_bounds__(kKnnThreads) void knn_refine_kernel(const T* __restrict__ q, int64_t ldq, int64_t mq,
                                                                 const T* __restrict__ c, int64_t ldc, int64_t mc, int d, int metric,
                                                                 double zero_norm, const int32_t* __restrict__ sel, int64_t sel_stride,
                                                                 int k, int32_t* __restrict__ out_ix, T* __restrict__ out_val) {
  __shared__ double s_key[kKnnThreads / 64][SAPCA_KNN_MAX_NEIGHBORS];
  __shared__ int32_t s_idx[kKnnThreads / 64][SAPCA_KNN_MAX_NEIGHBORS];
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  const int64_t qi = (int64_t)blockIdx.x * (kKnnThreads / 64) + wave;
  if (qi >= mq) return;
  const bool similarity = metric != SAPCA_KNN_EUCLIDEAN;
  T val[2];
  int idx[2];
  double key[2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int slot = lane + 64 * u;
    if (slot >= k) continue;
    int j = sel[qi * sel_stride + slot];
    if (j < 0 || (int64_t)j >= mc) {
      j = kKnnEmpty;
      val[u] = (T)NAN;
      key[u] = INFINITY;
    } else {
      val[u] = (T)knn_pair_value(q + qi * ldq, c + (int64_t)j * ldc, d, metric, zero_norm);
      const double v = (double)val[u];
      key[u] = v != v ? (double)INFINITY : (similarity ? -v : v);
    }
    idx[u] = j;
    s_key[wave][slot] = key[u];
    s_idx[wave][slot] = j;
  }
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int slot = lane + 64 * u;
    if (slot >= k) continue;
    int rank = 0;
    for (int e = 0; e < k; ++e) {
      const double ek = s_key[wave][e];
      const int ei = s_idx[wave][e];
      rank += (ek < key[u] || (ek == key[u] && (ei < idx[u] || (ei == idx[u] && e < slot)))) ? 1 : 0;
    }
    out_ix[qi * k + rank] = idx[u] == kKnnEmpty ? -1 : idx[u];
    out_val[qi * k + rank] = val[u];
  }
}

// A wave per row: the corpus bias -|b|^2 (EUCLIDEAN), or the row scaled to unit norm, centred first for PEARSON (f64
// arithmetic, sums in a fixed order, one rounding to T).  A row whose norm is <= zero_norm becomes the zero vector.
template <typename T>
__global__ __launch_bounds__(kKnnThreads) void knn_prepare_kernel(const T* __restrict__ x, int64_t ld, int64_t rows, int d, int metric,
                                                                  double zero_norm, T* __restrict__ unit, T* __restrict__ bias) {
  const int lane = (int)threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * (kKnnThreads / 64) + ((int)threadIdx.x >> 6);
  if (r >= rows) return;
  const T* row = x + r * ld;
  auto wave_sum = [](double v) {
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
  };
  double mean = 0;
  if (metric == SAPCA_KNN_PEARSON) {
    double s = 0;
    for (int t = lane; t < d; t += 64) s += (double)row[t];
    mean = wave_sum(s) / (double)d;
  }
  double s2 = 0;
  for (int t = lane; t < d; t += 64) {
    const double v = (double)row[t] - mean;
    s2 = fma(v, v, s2);
  }
  s2 = wave_sum(s2);
  if (metric == SAPCA_KNN_EUCLIDEAN) {
    if (lane == 0) bias[r] = (T)(-s2);
    return;
  }
  const double nrm = sqrt(s2);
  const bool zero = !(nrm > zero_norm);
  for (int t = lane; t < d; t += 64) unit[r * (int64_t)d + t] = zero ? (T)0 : (T)(((double)row[t] - mean) / nrm);
}

template <typename T>
size_t knn_lds_bytes(int mt, int k) {
  const size_t ld = (size_t)KnnChunk<T>::value + 4, qb = (size_t)64 * mt;
  return (qb + kKnnTile) * ld * sizeof(T) + qb * (size_t)k * (sizeof(T) + sizeof(int32_t));
}

template <typename T, int MT>
void knn_launch_select(const T* q, int64_t ldq, int64_t mq, const T* c, int64_t ldc, int64_t mc, const T* bias, int d, T alpha, int k,
                       bool exclude_self, const KnnPlan& plan, T* part_sc, int32_t* part_ix, hipStream_t s) {
  static LdsAttrState lds_state;
  ensure_dynamic_lds(reinterpret_cast<const void*>(&knn_select_kernel<T, MT>), plan.lds_bytes, lds_state);
  const int64_t blocks = (mq + 64 * MT - 1) / (64 * MT);
  hipLaunchKernelGGL((knn_select_kernel<T, MT>), dim3((unsigned)blocks, (unsigned)plan.nsplit), dim3(kKnnThreads), plan.lds_bytes, s, q,
                     ldq, mq, c, ldc, mc, bias, d, alpha, k, (int)exclude_self, plan.tiles_per_split, part_sc, part_ix);
  SAPCA_HIP(hipGetLastError());
}

}  // namespace

// Two query rows of 16 per wave (128 per workgroup) when that still fills the chip twice over and two workgroups fit a CU's
// LDS; otherwise one.  Fewer workgroups than that: the corpus tiles are dealt to up to 64 splits per query block.
template <typename T>
KnnPlan knn_plan(int64_t mq, int64_t mc, int k, int n_cus) {
  KnnPlan p;
  const int64_t want = 2 * (int64_t)(n_cus > 0 ? n_cus : 1);
  p.mt = ((mq + 127) / 128 >= want && knn_lds_bytes<T>(2, k) <= (size_t)80 * 1024) ? 2 : 1;
  p.lds_bytes = knn_lds_bytes<T>(p.mt, k);
  const int64_t blocks = (mq + 64 * p.mt - 1) / (64 * p.mt);
  const int64_t ntiles = (mc + kKnnTile - 1) / kKnnTile;
  int64_t nsplit = 1;
  if (blocks > 0 && blocks < want) nsplit = std::min<int64_t>(std::min<int64_t>((want + blocks - 1) / blocks, 64), ntiles);
  if (nsplit < 1) nsplit = 1;
  p.tiles_per_split = (int)((ntiles + nsplit - 1) / nsplit);
  if (p.tiles_per_split < 1) p.tiles_per_split = 1;
  p.nsplit = (int)std::max<int64_t>((ntiles + p.tiles_per_split - 1) / p.tiles_per_split, 1);
  return p;
}

template <typename T>
double knn_zero_norm() {
  return std::sqrt((double)std::numeric_limits<T>::epsilon());
}

template <typename T>
void knn_prepare(const T* x, int64_t ld, int64_t rows, int d, int metric, T* unit, T* bias, hipStream_t s) {
  if (rows <= 0) return;
  const int64_t blocks = (rows + kKnnThreads / 64 - 1) / (kKnnThreads / 64);
  hipLaunchKernelGGL((knn_prepare_kernel<T>), dim3((unsigned)blocks), dim3(kKnnThreads), 0, s, x, ld, rows, d, metric, knn_zero_norm<T>(),
                     unit, bias);
  SAPCA_HIP(hipGetLastError());
}

template <typename T>
void knn_select(const T* q, int64_t ldq, int64_t mq, const T* c, int64_t ldc, int64_t mc, const T* bias, int d, int metric, int k,
                bool exclude_self, const KnnPlan& plan, T* part_sc, int32_t* part_ix, hipStream_t s) {
  if (mq <= 0) return;
  const T alpha = metric == SAPCA_KNN_EUCLIDEAN ? (T)2 : (T)1;
  if (plan.mt == 2) knn_launch_select<T, 2>(q, ldq, mq, c, ldc, mc, bias, d, alpha, k, exclude_self, plan, part_sc, part_ix, s);
  else knn_launch_select<T, 1>(q, ldq, mq, c, ldc, mc, bias, d, alpha, k, exclude_self, plan, part_sc, part_ix, s);
}

template <typename T>
void knn_merge(const T* part_sc, const int32_t* part_ix, int64_t mq, int nsplit, int k, int32_t* merged, hipStream_t s) {
  if (mq <= 0) return;
  const int64_t blocks = (mq + kKnnThreads / 64 - 1) / (kKnnThreads / 64);
  hipLaunchKernelGGL((knn_merge_kernel<T>), dim3((unsigned)blocks), dim3(kKnnThreads), 0, s, part_sc, part_ix, mq, nsplit, k, merged);
  SAPCA_HIP(hipGetLastError());
}

template <typename T>
void knn_refine(const T* q, int64_t ldq, int64_t mq, const T* c, int64_t ldc, int64_t mc, int d, int metric, const int32_t* sel,
                int64_t sel_stride, int k, int32_t* out_ix, T* out_val, hipStream_t s) {
  if (mq <= 0) return;
  const int64_t blocks = (mq + kKnnThreads / 64 - 1) / (kKnnThreads / 64);
  hipLaunchKernelGGL((knn_refine_kernel<T>), dim3((unsigned)blocks), dim3(kKnnThreads), 0, s, q, ldq, mq, c, ldc, mc, d, metric,
                     knn_zero_norm<T>(), sel, sel_stride, k, out_ix, out_val);
  SAPCA_HIP(hipGetLastError());
}

#define SAPCA_INSTANTIATE_KNN(T)                                                                                                     \
  template KnnPlan knn_plan<T>(int64_t, int64_t, int, int);                                                                          \
  template void knn_prepare<T>(const T*, int64_t, int64_t, int, int, T*, T*, hipStream_t);                                           \
  template void knn_select<T>(const T*, int64_t, int64_t, const T*, int64_t, int64_t, const T*, int, int, int, bool, const KnnPlan&, \
                              T*, int32_t*, hipStream_t);                                                                            \
  template void knn_merge<T>(const T*, const int32_t*, int64_t, int, int, int32_t*, hipStream_t);                                    \
  template void knn_refine<T>(const T*, int64_t, int64_t, const T*, int64_t, int64_t, int, int, const int32_t*, int64_t, int,        \
                              int32_t*, T*, hipStream_t);
SAPCA_INSTANTIATE_KNN(float)
SAPCA_INSTANTIATE_KNN(double)
#undef SAPCA_INSTANTIATE_KNN

}  // namespace k
}  // namespace sapca
