// Louvain clustering of a symmetric CSR graph (sapca_louvain_*): hashed half-active synchronous sweeps with anchored targets;
// include/sapca.h states the algorithm in full.  Kernels:
//   row sums     one wave per row: k_i, and s_i (the weight a row sends into its own community) for the modularity
//   anchor       which communities hold an inactive vertex in this sweep
//   rows         THE hot kernel, one row per workgroup: the row's entries keyed (community << 32 | position), sorted (the key
//                is unique, so any sort gives one order), every run of equal community added left to right in f64.  Three
//                length classes: a wave with 64 keys in LDS, a workgroup of 256 with up to 4096 keys in LDS, a workgroup of
//                1024 with its keys in global scratch.  The sweep ranks the runs' gains; the aggregation counts / emits them.
//   totals       the vertices sorted by (community, vertex) by a bitonic network over global memory (tiles of 4096 in LDS),
//                then every community's k added in ascending vertex order by the thread that finds its first member
//   decide       keep or undo on the device: which label generation is current is a word of the control block
// No floating-point atomics.  Integer atomics count the moved vertices and hand out list slots whose order reaches no value.
#include <climits>

#include "hash_u01.h"
#include "kernels.h"

// products and sums as written: r_i = (gamma k_i) / S and w - r_i tot round every step, as the restatement does
#pragma clang fp contract(off)

namespace sapca {
namespace k {

namespace {

constexpr int kWave = 64;
constexpr unsigned long long kPad = ~0ull;   // sorts behind every key (a community is below 2^31)
constexpr int kSortTile = 4096;

inline unsigned blocks_of(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

__device__ inline bool lv_skip(const LouvainCtl* c, bool need_moved) { return c != nullptr && (c->done != 0 || (need_moved && c->moved == 0)); }
__device__ inline int lv_gen(const LouvainState& st, int flip) { return st.ctl ? (int)((st.ctl->cur ^ (unsigned long long)flip) & 1ull) : flip; }
__device__ inline bool lv_active(uint64_t seed, uint64_t stream_hi, int64_t i) { return hash_u01(seed, 41, (stream_hi << 32) + (uint64_t)i) < 0.5; }

__device__ inline double wave_sum(double v) {   // the same value in every lane, one order
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
  return v;
}

__device__ inline int64_t pow2_ceil(int64_t v) {
  int64_t p = 2;
  while (p < v) p <<= 1;
  return p;
}

// the n2 (a power of two) keys of a workgroup's row, ascending; ends on a barrier
template <int NT>
__device__ inline void bitonic_sort(unsigned long long* key, int64_t n2) {
  for (int64_t size = 2; size <= n2; size <<= 1)
    for (int64_t stride = size >> 1; stride > 0; stride >>= 1) {
      __syncthreads();
      for (int64_t t = threadIdx.x; t < (n2 >> 1); t += NT) {
        const int64_t lo = 2 * t - (t & (stride - 1));
        const int64_t hi = lo + stride;
        const bool up = (lo & size) == 0;
        const unsigned long long a = key[lo], b = key[hi];
        if ((a > b) == up) {
          key[lo] = b;
          key[hi] = a;
        }
      }
    }
  __syncthreads();
}

// ---- lists, labels ------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) lv_list_kernel(const int64_t* __restrict__ ptr, int64_t n, uint32_t* __restrict__ rows,
                                                      unsigned long long* __restrict__ long_off, unsigned long long* __restrict__ ctr) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int64_t len = ptr[i + 1] - ptr[i];
  const int c = len <= kLvWaveCap ? kLvListWave : (len <= kLvLdsCap ? kLvListLds : kLvListLong);
  const unsigned long long slot = atomicAdd(&ctr[c], 1ull);
  rows[(int64_t)c * n + (int64_t)slot] = (uint32_t)i;
  if (c == kLvListLong) long_off[slot] = atomicAdd(&ctr[kLvLongKeys], (unsigned long long)pow2_ceil(len));
}

__global__ void __launch_bounds__(256) lv_iota_kernel(int32_t* __restrict__ lab, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) lab[i] = (int32_t)i;
}

// ---- row sums -----------------------------------------------------------------------------------------------------------
template <typename TV>
__global__ void __launch_bounds__(256) lv_row_sums_kernel(const int64_t* __restrict__ ptr, const int32_t* __restrict__ idx,
                                                          const TV* __restrict__ val, int64_t n, LouvainState st, int flip, int internal,
                                                          double* __restrict__ out) {
  if (internal && lv_skip(st.ctl, flip != 0)) return;
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t row = (int64_t)blockIdx.x * (256 / kWave) + (threadIdx.x / kWave);
  if (row >= n) return;   // (whole waves leave together)
  const int32_t* lab = internal ? st.lab[lv_gen(st, flip)] : nullptr;
  const int64_t C = lab ? (int64_t)lab[row] : 0;
  double v = 0.0;
  if (!lab || (C >= 0 && C < n)) {
    const int64_t end = ptr[row + 1];
    for (int64_t e = ptr[row] + lane; e < end; e += kWave) {
      const int64_t j = idx[e];
      if (j < 0 || j >= n) continue;
      if (lab && (int64_t)lab[j] != C) continue;
      v += (double)val[e];
    }
  }
  v = wave_sum(v);
  if (lane == 0) out[row] = v;
}

// ---- anchors ------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) lv_anchor_kernel(LouvainState st, int64_t n, uint64_t seed, uint64_t stream_hi,
                                                        uint8_t* __restrict__ anchored) {
  if (lv_skip(st.ctl, false)) return;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int64_t C = st.lab[lv_gen(st, 0)][i];
  if (C < 0 || C >= n) return;
  if (!lv_active(seed, stream_hi, i)) anchored[C] = 1;   // (every writer stores the same byte)
}

// ---- the rows kernel ----------------------------------------------------------------------------------------------------
enum { kModeSweep = 0, kModeCount = 1, kModeEmit = 2 };

template <typename TV>
struct RowArgs {
  const int64_t* ptr;
  const int32_t* idx;
  const TV* val;
  int64_t n;   // rows, and the bound of columns and labels
  const uint32_t* list;
  int64_t count;
  const unsigned long long* long_off;
  unsigned long long* keyspace;
  LouvainState st;
  // the sweep
  const double* k;
  const uint8_t* anchored;
  uint64_t seed, stream_hi;
  // the aggregation
  const int32_t* renum;
  int64_t* cnt;
  const int64_t* out_off;
  const int32_t* pos;
  int32_t* out_idx;
  double* out_val;
};

template <typename TV, int NT, int STORE, int MODE>
__global__ void __launch_bounds__(NT) lv_rows_kernel(RowArgs<TV> a) {
  constexpr int kLds = STORE == 0 ? kLvWaveCap : (STORE == 1 ? kLvLdsCap : 1);
  __shared__ unsigned long long sk[kLds];
  __shared__ int sc[NT];
  __shared__ double sg[MODE == kModeSweep ? NT : 1];
  __shared__ double s_wc;
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x;
  if (b >= a.count) return;
  if (MODE == kModeSweep && lv_skip(a.st.ctl, false)) return;
  const int64_t i = a.list[b];
  const int32_t* lab = a.st.lab[lv_gen(a.st, 0)];   // null: every vertex its own community
  const int64_t C = lab ? (int64_t)lab[i] : i;
  const bool own_ok = C >= 0 && C < a.n;
  if (MODE == kModeSweep) {
    if (!own_ok || !lv_active(a.seed, a.stream_hi, i)) {   // inactive: the label is copied through
      if (tid == 0) a.st.lab[lv_gen(a.st, 1)][i] = (int32_t)C;
      return;
    }
  } else if (!own_ok) {
    if (MODE == kModeCount && tid == 0) a.cnt[i] = 0;
    return;
  }
  const int64_t start = a.ptr[i];
  const int64_t len = a.ptr[i + 1] - start;
  const int64_t n2 = STORE == 0 ? kLvWaveCap : pow2_ceil(len);
  unsigned long long* key = STORE == 2 ? a.keyspace + a.long_off[b] : sk;
  for (int64_t t = tid; t < n2; t += NT) {
    unsigned long long kk = kPad;
    if (t < len) {
      const int64_t j = a.idx[start + t];
      if (j >= 0 && j < a.n && !(MODE == kModeSweep && j == i)) {
        const int64_t cj = lab ? (int64_t)lab[j] : j;
        if (cj >= 0 && cj < a.n) kk = ((unsigned long long)cj << 32) | (unsigned long long)t;
      }
    }
    key[t] = kk;
  }
  if (tid == 0) s_wc = 0.0;
  bitonic_sort<NT>(key, n2);

  // every thread owns a stretch of the sorted keys; a run belongs to the thread that owns its first key
  const int64_t per = (n2 + NT - 1) / NT;
  const int64_t p0 = (int64_t)tid * per;
  const int64_t p1 = p0 + per < n2 ? p0 + per : n2;
  int64_t rank = 0;
  if (MODE != kModeSweep) {
    int heads = 0;
    for (int64_t p = p0; p < p1; ++p) {
      const unsigned long long kk = key[p];
      if (kk != kPad && (p == 0 || (key[p - 1] >> 32) != (kk >> 32))) ++heads;
    }
    sc[tid] = heads;
    __syncthreads();
    for (int o = 1; o < NT; o <<= 1) {   // inclusive scan
      const int add = tid >= o ? sc[tid - o] : 0;
      __syncthreads();
      sc[tid] += add;
      __syncthreads();
    }
    if (MODE == kModeCount) {
      if (tid == 0) a.cnt[i] = sc[NT - 1];
      return;
    }
    rank = sc[tid] - heads;
  }
  const double ki = MODE == kModeSweep ? a.k[i] : 0.0;
  const double S = MODE == kModeSweep ? a.st.ctl->S : 1.0;
  const double r = MODE == kModeSweep ? (a.st.ctl->gamma * ki) / S : 0.0;
  const double* tot = MODE == kModeSweep ? a.st.tot[lv_gen(a.st, 0)] : nullptr;
  const int64_t base = MODE == kModeEmit ? a.out_off[a.pos ? (int64_t)a.pos[i] : i] : 0;
  double best = 0.0;
  int best_d = INT_MAX;
  for (int64_t p = p0; p < p1; ++p) {
    const unsigned long long kk = key[p];
    if (kk == kPad) break;
    const unsigned long long D = kk >> 32;
    if (p != 0 && (key[p - 1] >> 32) == D) continue;
    double w = 0.0;
    for (int64_t q = p; q < n2; ++q) {
      const unsigned long long kq = key[q];
      if ((kq >> 32) != D) break;
      w += (double)a.val[start + (int64_t)(kq & 0xffffffffull)];
    }
    if (MODE == kModeSweep) {
      if ((int64_t)D == C) {
        s_wc = w;   // (one run at most carries the row's own community)
      } else if (a.anchored[D]) {
        const double g = w - r * tot[D];
        if (best_d == INT_MAX || g > best) {   // (runs ascend in D: a tie keeps the lower label)
          best = g;
          best_d = (int)D;
        }
      }
    } else {
      a.out_idx[base + rank] = a.renum ? a.renum[D] : (int32_t)D;
      a.out_val[base + rank] = w;
      ++rank;
    }
  }
  if (MODE == kModeSweep) {
    sg[tid] = best;
    sc[tid] = best_d;
    __syncthreads();
    for (int o = NT / 2; o > 0; o >>= 1) {
      if (tid < o) {
        const int od = sc[tid + o];
        const double og = sg[tid + o];
        const int md = sc[tid];
        const double mg = sg[tid];
        if (od != INT_MAX && (md == INT_MAX || og > mg || (og == mg && od < md))) {
          sg[tid] = og;
          sc[tid] = od;
        }
      }
      __syncthreads();
    }
    if (tid == 0) {
      const double gc = s_wc - r * (tot[C] - ki);
      const bool move = sc[0] != INT_MAX && sg[0] > gc;
      a.st.lab[lv_gen(a.st, 1)][i] = move ? sc[0] : (int32_t)C;
      if (move) atomicAdd(&a.st.ctl->moved, 1ull);
    }
  }
}

template <typename TV, int MODE>
void launch_rows(RowArgs<TV> a, const LouvainLists& L, hipStream_t s) {
  a.keyspace = L.keys;
  a.long_off = L.long_off;
  if (L.counts[0] > 0) {
    a.list = L.rows;
    a.count = L.counts[0];
    hipLaunchKernelGGL((lv_rows_kernel<TV, 64, 0, MODE>), dim3((unsigned)a.count), dim3(64), 0, s, a);
  }
  if (L.counts[1] > 0) {
    a.list = L.rows + L.n;
    a.count = L.counts[1];
    hipLaunchKernelGGL((lv_rows_kernel<TV, 256, 1, MODE>), dim3((unsigned)a.count), dim3(256), 0, s, a);
  }
  if (L.counts[2] > 0) {
    a.list = L.rows + 2 * L.n;
    a.count = L.counts[2];
    hipLaunchKernelGGL((lv_rows_kernel<TV, 1024, 2, MODE>), dim3((unsigned)a.count), dim3(1024), 0, s, a);
  }
  SAPCA_HIP(hipGetLastError());
}

// ---- the vertex sort and the community totals ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) lv_keys_kernel(LouvainState st, int flip, int need_moved, int64_t n, int64_t n2,
                                                      unsigned long long* __restrict__ keys) {
  if (lv_skip(st.ctl, need_moved != 0)) return;
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= n2) return;
  const int g = lv_gen(st, flip);
  unsigned long long kk = kPad;
  if (p < n) {
    const int64_t c = st.lab[g][p];
    if (c >= 0 && c < n) kk = ((unsigned long long)c << 32) | (unsigned long long)p;
    if (st.tot[g]) st.tot[g][p] = 0.0;
  }
  keys[p] = kk;
}

// the steps of the network with stride < tile, for sizes size_lo .. size_hi, on the workgroup's tile in LDS
__global__ void __launch_bounds__(256) lv_sort_tile_kernel(LouvainState st, int need_moved, unsigned long long* __restrict__ keys, int tile,
                                                           int64_t size_lo, int64_t size_hi) {
  __shared__ unsigned long long sh[kSortTile];
  if (lv_skip(st.ctl, need_moved != 0)) return;
  const int64_t base = (int64_t)blockIdx.x * tile;
  for (int t = threadIdx.x; t < tile; t += 256) sh[t] = keys[base + t];
  for (int64_t size = size_lo; size <= size_hi; size <<= 1) {
    for (int stride = (int)(size / 2 < tile / 2 ? size / 2 : tile / 2); stride > 0; stride >>= 1) {
      __syncthreads();
      for (int t = threadIdx.x; t < tile / 2; t += 256) {
        const int lo = 2 * t - (t & (stride - 1));
        const int hi = lo + stride;
        const bool up = ((base + lo) & size) == 0;
        const unsigned long long a = sh[lo], b = sh[hi];
        if ((a > b) == up) {
          sh[lo] = b;
          sh[hi] = a;
        }
      }
    }
  }
  __syncthreads();
  for (int t = threadIdx.x; t < tile; t += 256) keys[base + t] = sh[t];
}

__global__ void __launch_bounds__(256) lv_sort_step_kernel(LouvainState st, int need_moved, unsigned long long* __restrict__ keys, int64_t n2,
                                                           int64_t size, int64_t stride) {
  if (lv_skip(st.ctl, need_moved != 0)) return;
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (n2 >> 1)) return;
  const int64_t lo = 2 * t - (t & (stride - 1));
  const int64_t hi = lo + stride;
  const bool up = (lo & size) == 0;
  const unsigned long long a = keys[lo], b = keys[hi];
  if ((a > b) == up) {
    keys[lo] = b;
    keys[hi] = a;
  }
}

__global__ void __launch_bounds__(256) lv_tot_kernel(LouvainState st, int flip, int need_moved, int64_t n, const double* __restrict__ k,
                                                     const unsigned long long* __restrict__ keys) {
  if (lv_skip(st.ctl, need_moved != 0)) return;
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  const unsigned long long kk = keys[p];
  if (kk == kPad) return;
  const unsigned long long C = kk >> 32;
  if (p != 0 && (keys[p - 1] >> 32) == C) return;
  double sum = 0.0;
  for (int64_t q = p; q < n; ++q) {
    const unsigned long long kq = keys[q];
    if ((kq >> 32) != C) break;
    sum += k[kq & 0xffffffffull];
  }
  st.tot[lv_gen(st, flip)][C] = sum;
}

__global__ void __launch_bounds__(256) lv_sq_kernel(LouvainState st, int flip, int need_moved, int64_t n, const double* __restrict__ S,
                                                    double* __restrict__ sq) {
  if (lv_skip(st.ctl, need_moved != 0)) return;
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= n) return;
  const double t = S[0] > 0.0 ? st.tot[lv_gen(st, flip)][c] / S[0] : 0.0;
  sq[c] = t * t;
}

__global__ void lv_decide_kernel(LouvainCtl* c, int init) {
  if (c->done) return;
  const double q = c->S > 0.0 ? c->sum_s / c->S - c->gamma * c->sum_sq : 0.0;
  if (init) {
    c->Q = q;
    return;
  }
  if (c->moved != 0 && q > c->Q + c->tol) {
    c->cur ^= 1ull;
    c->Q = q;
    c->misses = 0;
    c->kept += 1;
  } else {
    c->misses += 1;
  }
  if (c->misses >= 4) c->done = 1;
  c->moved = 0;
  c->sweeps += 1;
}

// ---- aggregation ----------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) lv_flag_kernel(const int32_t* __restrict__ labels, int64_t n, int64_t* __restrict__ flag) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int64_t c = labels[i];
  if (c >= 0 && c < n) flag[c] = 1;
}

__global__ void __launch_bounds__(256) lv_renumber_kernel(const int32_t* __restrict__ labels, int64_t n, const int64_t* __restrict__ scan,
                                                          int32_t* __restrict__ renum, int32_t* __restrict__ renumbered) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  renum[i] = (int32_t)scan[i];
  if (renumbered) {
    const int64_t c = labels[i];
    renumbered[i] = (c >= 0 && c < n) ? (int32_t)scan[c] : (int32_t)c;
  }
}

__global__ void __launch_bounds__(256) lv_positions_kernel(const unsigned long long* __restrict__ keys, int64_t n, const int64_t* __restrict__ cnt,
                                                           int32_t* __restrict__ pos, int64_t* __restrict__ rawcnt) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p > n) return;
  int64_t c = 0;
  if (p < n) {
    const unsigned long long kk = keys[p];
    if (kk != kPad) {
      const int64_t v = (int64_t)(kk & 0xffffffffull);
      pos[v] = (int32_t)p;
      c = cnt[v];
    }
  }
  rawcnt[p] = c;
}

__global__ void __launch_bounds__(256) lv_coarse_offsets_kernel(const unsigned long long* __restrict__ keys, int64_t n,
                                                                const int64_t* __restrict__ rawoff, const int32_t* __restrict__ renum,
                                                                const int64_t* __restrict__ scan, int64_t* __restrict__ rawptr) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  if (p == 0) rawptr[scan[n]] = rawoff[n];
  const unsigned long long kk = keys[p];
  if (kk == kPad) return;
  const unsigned long long C = kk >> 32;
  if (p != 0 && (keys[p - 1] >> 32) == C) return;
  rawptr[renum[C]] = rawoff[p];
}

__global__ void __launch_bounds__(256) lv_compose_kernel(int32_t* __restrict__ final_labels, int64_t m, const int32_t* __restrict__ labels,
                                                         const int32_t* __restrict__ renum, int first) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= m) return;
  const int32_t f = first ? (int32_t)v : final_labels[v];
  final_labels[v] = renum[labels[f]];
}

template <typename TV>
RowArgs<TV> row_args(const CsrView<TV>& A) {
  RowArgs<TV> a = {};
  a.ptr = A.ptr;
  a.idx = A.idx;
  a.val = A.val;
  a.n = A.rows;
  return a;
}

}  // namespace

void louvain_list_rows(const int64_t* ptr, int64_t n, uint32_t* rows, unsigned long long* long_off, unsigned long long* ctr, hipStream_t s) {
  SAPCA_HIP(hipMemsetAsync(ctr, 0, kLvCtrWords * sizeof(unsigned long long), s));
  if (n == 0) return;
  hipLaunchKernelGGL(lv_list_kernel, dim3(blocks_of(n, 256)), dim3(256), 0, s, ptr, n, rows, long_off, ctr);
  SAPCA_HIP(hipGetLastError());
}

void louvain_iota(int32_t* lab, int64_t n, hipStream_t s) {
  hipLaunchKernelGGL(lv_iota_kernel, dim3(blocks_of(n, 256)), dim3(256), 0, s, lab, n);
  SAPCA_HIP(hipGetLastError());
}

template <typename TV>
void louvain_row_sums(const CsrView<TV>& A, const LouvainState& st, int flip, bool internal, double* out, hipStream_t s) {
  hipLaunchKernelGGL((lv_row_sums_kernel<TV>), dim3(blocks_of(A.rows, 256 / kWave)), dim3(256), 0, s, A.ptr, A.idx, A.val, A.rows, st, flip,
                     internal ? 1 : 0, out);
  SAPCA_HIP(hipGetLastError());
}

void louvain_anchor(const LouvainState& st, int64_t n, uint64_t seed, uint64_t level, uint64_t sweep, uint8_t* anchored, hipStream_t s) {
  SAPCA_HIP(hipMemsetAsync(anchored, 0, (size_t)n, s));
  hipLaunchKernelGGL(lv_anchor_kernel, dim3(blocks_of(n, 256)), dim3(256), 0, s, st, n, seed, level * 4096 + sweep, anchored);
  SAPCA_HIP(hipGetLastError());
}

template <typename TV>
void louvain_sweep(const CsrView<TV>& A, const LouvainLists& L, const LouvainState& st, const double* k, const uint8_t* anchored,
                   uint64_t seed, uint64_t level, uint64_t sweep, hipStream_t s) {
  RowArgs<TV> a = row_args(A);
  a.st = st;
  a.k = k;
  a.anchored = anchored;
  a.seed = seed;
  a.stream_hi = level * 4096 + sweep;
  launch_rows<TV, kModeSweep>(a, L, s);
}

int64_t louvain_sort_len(int64_t n) {
  int64_t p = 64;
  while (p < n) p <<= 1;
  return p;
}

void louvain_totals(const LouvainState& st, int flip, bool need_moved, int64_t n, const double* k, unsigned long long* keys, const double* S,
                    double* sq, hipStream_t s) {
  const int64_t n2 = louvain_sort_len(n);
  const int nm = need_moved ? 1 : 0;
  const int tile = (int)(n2 < kSortTile ? n2 : kSortTile);
  hipLaunchKernelGGL(lv_keys_kernel, dim3(blocks_of(n2, 256)), dim3(256), 0, s, st, flip, nm, n, n2, keys);
  hipLaunchKernelGGL(lv_sort_tile_kernel, dim3((unsigned)(n2 / tile)), dim3(256), 0, s, st, nm, keys, tile, (int64_t)2, (int64_t)tile);
  for (int64_t size = 2 * (int64_t)tile; size <= n2; size <<= 1) {
    for (int64_t stride = size >> 1; stride >= tile; stride >>= 1)
      hipLaunchKernelGGL(lv_sort_step_kernel, dim3(blocks_of(n2 >> 1, 256)), dim3(256), 0, s, st, nm, keys, n2, size, stride);
    hipLaunchKernelGGL(lv_sort_tile_kernel, dim3((unsigned)(n2 / tile)), dim3(256), 0, s, st, nm, keys, tile, size, size);
  }
  if (k) hipLaunchKernelGGL(lv_tot_kernel, dim3(blocks_of(n, 256)), dim3(256), 0, s, st, flip, nm, n, k, keys);
  if (sq) hipLaunchKernelGGL(lv_sq_kernel, dim3(blocks_of(n, 256)), dim3(256), 0, s, st, flip, nm, n, S, sq);
  SAPCA_HIP(hipGetLastError());
}

void louvain_decide(const LouvainState& st, bool init, hipStream_t s) {
  hipLaunchKernelGGL(lv_decide_kernel, dim3(1), dim3(1), 0, s, st.ctl, init ? 1 : 0);
  SAPCA_HIP(hipGetLastError());
}

void louvain_flag(const int32_t* labels, int64_t n, int64_t* flag, hipStream_t s) {
  SAPCA_HIP(hipMemsetAsync(flag, 0, (size_t)(n + 1) * sizeof(int64_t), s));
  hipLaunchKernelGGL(lv_flag_kernel, dim3(blocks_of(n, 256)), dim3(256), 0, s, labels, n, flag);
  SAPCA_HIP(hipGetLastError());
}

void louvain_renumber(const int32_t* labels, int64_t n, const int64_t* scan, int32_t* renum, int32_t* renumbered, hipStream_t s) {
  hipLaunchKernelGGL(lv_renumber_kernel, dim3(blocks_of(n, 256)), dim3(256), 0, s, labels, n, scan, renum, renumbered);
  SAPCA_HIP(hipGetLastError());
}

template <typename TV>
void louvain_group_count(const CsrView<TV>& A, const LouvainLists& L, const int32_t* labels, int64_t* cnt, hipStream_t s) {
  RowArgs<TV> a = row_args(A);
  a.st.lab[0] = const_cast<int32_t*>(labels);
  a.cnt = cnt;
  launch_rows<TV, kModeCount>(a, L, s);
}

void louvain_positions(const unsigned long long* keys, int64_t n, const int64_t* cnt, int32_t* pos, int64_t* rawcnt, hipStream_t s) {
  hipLaunchKernelGGL(lv_positions_kernel, dim3(blocks_of(n + 1, 256)), dim3(256), 0, s, keys, n, cnt, pos, rawcnt);
  SAPCA_HIP(hipGetLastError());
}

void louvain_coarse_offsets(const unsigned long long* keys, int64_t n, const int64_t* rawoff, const int32_t* renum, const int64_t* scan,
                            int64_t* rawptr, hipStream_t s) {
  hipLaunchKernelGGL(lv_coarse_offsets_kernel, dim3(blocks_of(n, 256)), dim3(256), 0, s, keys, n, rawoff, renum, scan, rawptr);
  SAPCA_HIP(hipGetLastError());
}

template <typename TV>
void louvain_group_emit(const CsrView<TV>& A, const LouvainLists& L, const int32_t* labels, const int32_t* renum, const int64_t* out_off,
                        const int32_t* pos, int32_t* out_idx, double* out_val, hipStream_t s) {
  RowArgs<TV> a = row_args(A);
  a.st.lab[0] = const_cast<int32_t*>(labels);
  a.renum = renum;
  a.out_off = out_off;
  a.pos = pos;
  a.out_idx = out_idx;
  a.out_val = out_val;
  launch_rows<TV, kModeEmit>(a, L, s);
}

void louvain_compose(int32_t* final_labels, int64_t m, const int32_t* labels, const int32_t* renum, bool first, hipStream_t s) {
  hipLaunchKernelGGL(lv_compose_kernel, dim3(blocks_of(m, 256)), dim3(256), 0, s, final_labels, m, labels, renum, first ? 1 : 0);
  SAPCA_HIP(hipGetLastError());
}

#define SAPCA_INSTANTIATE_LOUVAIN(TV)                                                                                              \
  template void louvain_row_sums<TV>(const CsrView<TV>&, const LouvainState&, int, bool, double*, hipStream_t);                    \
  template void louvain_sweep<TV>(const CsrView<TV>&, const LouvainLists&, const LouvainState&, const double*, const uint8_t*,     \
                                  uint64_t, uint64_t, uint64_t, hipStream_t);                                                      \
  template void louvain_group_count<TV>(const CsrView<TV>&, const LouvainLists&, const int32_t*, int64_t*, hipStream_t);           \
  template void louvain_group_emit<TV>(const CsrView<TV>&, const LouvainLists&, const int32_t*, const int32_t*, const int64_t*,    \
                                       const int32_t*, int32_t*, double*, hipStream_t);
SAPCA_INSTANTIATE_LOUVAIN(float)
SAPCA_INSTANTIATE_LOUVAIN(double)
#undef SAPCA_INSTANTIATE_LOUVAIN

}  // namespace k
}  // namespace sapca
