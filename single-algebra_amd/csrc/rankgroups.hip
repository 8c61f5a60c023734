// The rank pass behind sapca_rank_sums_csr_device_* / sapca_rank_groups_csr_device_* (include/sapca.h, "Rank groups"): per
// column of A -- a row of the operand At = A^T -- the ranks of the stored non-zero values of the included rows among all M
// included rows, the zeros (stored or implicit) as one tie block, summed per group.
// A column keeps its entries as (key, label): the key is the order-preserving unsigned image of the value (value_keys.h), an
// excluded row's entry or a stored zero gets the largest key and the label kDropped, so it sorts behind the L kept ones.
// After the sort by key, position p (0-based) of the kept entries stands at rank p + 1 when p < a (a: the negative ones) and
// at p + 1 + Z behind the Z zeros otherwise.  An entry whose neighbours differ is a run of its own; otherwise the ends p0, p1
// of its tie run are found by bisection in the sorted keys, so nothing is carried from one step of a walk to the next.  Each
// entry adds (rank of p0) + (rank of p1) -- twice its average rank -- to its group's 64-bit counter in LDS and one to its
// group's count; the first entry of a run adds t^3 - t to its lane's tie sum.  Integer LDS atomics only: no order reaches a
// value, and the lanes' tie sums meet in a fixed tree (exact integers while below 2^53).
// Three length classes (rankgroups.h); all three end in rank_finish.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>

#include <rocprim/rocprim.hpp>


#include "kernels.h"
#include "rankgroups.h"
#include "value_keys.h"

namespace sapca {
namespace k {

namespace {

constexpr int WAVE = 64;
constexpr int BLOCK = 256;
constexpr uint16_t kDropped = 0xffff;   // (a label is below SAPCA_RANK_MAX_GROUPS = 1,024)

template <int G>
__device__ inline void group_sync() {
  if constexpr (G == WAVE) {   // the lanes of a wave meet in their own LDS only
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  } else {
    __syncthreads();
  }
}

__host__ __device__ constexpr size_t up16(size_t b) { return (b + 15) / 16 * 16; }

// The LDS of one column in flight, every part 16-byte aligned: rs[nk] (u64) | keys[cap] | red[G] (f64) | cnt[nk] (u32) |
// misc[4] (u32: kept, negative) | labs[cap] (u16)
template <typename K>
struct RankLds {
  unsigned long long* rs;
  K* keys;
  double* red;
  uint32_t* cnt;
  uint32_t* misc;
  uint16_t* labs;
  __host__ __device__ static constexpr size_t bytes(int cap, int nk, int G) {
    return up16((size_t)nk * 8) + up16((size_t)cap * sizeof(K)) + up16((size_t)G * 8) + up16((size_t)nk * 4) + 16 + up16((size_t)cap * 2);
  }
  __device__ RankLds(char* b, int cap, int nk, int G) {
    rs = reinterpret_cast<unsigned long long*>(b);
    b += up16((size_t)nk * 8);
    keys = reinterpret_cast<K*>(b);
    b += up16((size_t)cap * sizeof(K));
    red = reinterpret_cast<double*>(b);
    b += up16((size_t)G * 8);
    cnt = reinterpret_cast<uint32_t*>(b);
    b += up16((size_t)nk * 4);
    misc = reinterpret_cast<uint32_t*>(b);
    b += 16;
    labs = reinterpret_cast<uint16_t*>(b);
  }
};

// (key, label) of the entry (row i of A, value x): dropped unless the row is included and x != 0; kept / neg count the kept ones
template <typename T>
__device__ inline void rank_entry(T x, int32_t code, int nk, typename Keys<T>::K& key, uint16_t& lab, uint32_t& kept, uint32_t& neg) {
  key = ~(typename Keys<T>::K)0;
  lab = kDropped;
  if ((unsigned)code < (unsigned)nk && x != (T)0) {
    key = Keys<T>::key(x);
    lab = (uint16_t)code;
    ++kept;
    neg += x < (T)0 ? 1u : 0u;
  }
}

// The run-and-accumulate step over the sorted (key, label) of one column: positions tid, tid + G, .. below L.
template <typename K>
__device__ inline void rank_accumulate(const K* keys, const uint16_t* labs, int64_t L, int64_t a, int64_t Z, int tid, int G, int nk,
                                       unsigned long long* rs, uint32_t* cnt, double& tie) {
  for (int64_t p = tid; p < L; p += G) {
    const unsigned lab = labs[p];
    if (lab >= (unsigned)nk) continue;   // (only a NaN can stand behind a dropped entry: the column is unspecified, the slot is not touched)
    const K key = keys[p];
    int64_t p0 = p, p1 = p;
    if (p > 0 && keys[p - 1] == key) {   // the first position that holds `key`
      int64_t lo = 0, hi = p - 1;
      while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (keys[mid] < key) lo = mid + 1;
        else hi = mid;
      }
      p0 = lo;
    }
    if (p + 1 < L && keys[p + 1] == key) {   // the last one
      int64_t lo = p + 1, hi = L - 1;
      while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (keys[mid] > key) hi = mid - 1;
        else lo = mid;
      }
      p1 = lo;
    }
    const int64_t off = p < a ? 0 : Z;
    atomicAdd(&rs[lab], (unsigned long long)(p0 + p1 + 2 + 2 * off));
    atomicAdd(&cnt[lab], 1u);
    if (p == p0) {
      const double t = (double)(p1 - p0 + 1);
      tie += t * t * t - t;
    }
  }
}

// The zero block and the K results of column j: rank_sum2[g][j] = the counter + (n_g - c_gj) ((a + 1) + (a + Z)).
template <int G, typename K>
__device__ inline void rank_finish(const RankLds<K>& s, int tid, int nk, int64_t a, int64_t Z, double tie, const unsigned long long* group,
                                   int64_t j, int64_t cols, long long* out_rs, uint32_t* out_cnt, double* out_tie) {
  if (tid == 0) {
    const double z = (double)Z;
    tie += z * z * z - z;
  }
  s.red[tid] = tie;
  group_sync<G>();   // (also: every atomic of the accumulation has landed)
  for (int off = G / 2; off > 0; off >>= 1) {
    if (tid < off) s.red[tid] += s.red[tid + off];
    group_sync<G>();
  }
  if (tid == 0) out_tie[j] = s.red[0];
  const long long zero2 = (long long)((a + 1) + (a + Z));
  for (int b = tid; b < nk; b += G) {
    const uint32_t c = s.cnt[b];
    out_rs[(int64_t)b * cols + j] = (long long)s.rs[b] + ((long long)group[b] - (long long)c) * zero2;
    out_cnt[(int64_t)b * cols + j] = c;
  }
}

// ---- the two LDS classes: G threads per column (a wave, or the workgroup), columns of stored length in (lo_len, hi_len] ----
template <typename T, int G, int CAP>
__global__ void __launch_bounds__(BLOCK) rank_lds_kernel(const int64_t* __restrict__ ptr, const int32_t* __restrict__ idx,
                                                         const T* __restrict__ val, int64_t cols, const int32_t* __restrict__ labels,
                                                         int nk, const unsigned long long* __restrict__ group, int64_t M, int lo_len,
                                                         int hi_len, long long* __restrict__ out_rs, uint32_t* __restrict__ out_cnt,
                                                         double* __restrict__ out_tie) {
  using KT = Keys<T>;
  using K = typename KT::K;
  extern __shared__ __attribute__((aligned(16))) char lds_rank[];
  const int tid = threadIdx.x % G, grp = threadIdx.x / G;
  const int64_t j = (int64_t)blockIdx.x * (BLOCK / G) + grp;
  if (j >= cols) return;   // (uniform over the G threads of a column, like every return and loop bound below)
  const int64_t e0 = ptr[j];
  const int64_t len = ptr[j + 1] - e0;
  if (len <= lo_len || len > hi_len) return;
  const RankLds<K> s(lds_rank + (size_t)grp * RankLds<K>::bytes(CAP, nk, G), CAP, nk, G);
  for (int b = tid; b < nk; b += G) {
    s.rs[b] = 0ull;
    s.cnt[b] = 0u;
  }
  if (tid < 2) s.misc[tid] = 0u;
  int n2 = WAVE;   // the sorted length: a power of two, len <= n2 <= CAP
  while (n2 < len) n2 <<= 1;
  group_sync<G>();
  uint32_t kept = 0, neg = 0;
  for (int p = tid; p < n2; p += G) {
    K key = ~(K)0;
    uint16_t lab = kDropped;
    if (p < len) rank_entry<T>(val[e0 + p], labels[idx[e0 + p]], nk, key, lab, kept, neg);
    s.keys[p] = key;
    s.labs[p] = lab;
  }
  atomicAdd(&s.misc[0], kept);
  atomicAdd(&s.misc[1], neg);
  group_sync<G>();
  // bitonic sort by key, ascending; the labels travel with their keys (the order inside a tie run reaches no result)
  for (int k = 2; k <= n2; k <<= 1) {
    for (int jj = k >> 1; jj > 0; jj >>= 1) {
      for (int t = tid; t < n2 / 2; t += G) {
        const int i = ((t & ~(jj - 1)) << 1) | (t & (jj - 1));
        const int l = i | jj;
        const K ki = s.keys[i], kl = s.keys[l];
        if ((ki > kl) == ((i & k) == 0)) {
          s.keys[i] = kl;
          s.keys[l] = ki;
          const uint16_t li = s.labs[i];
          s.labs[i] = s.labs[l];
          s.labs[l] = li;
        }
      }
      group_sync<G>();
    }
  }
  const int64_t L = s.misc[0], a = s.misc[1], Z = M - L;
  double tie = 0.0;
  rank_accumulate<K>(s.keys, s.labs, L, a, Z, tid, G, nk, s.rs, s.cnt, tie);
  rank_finish<G, K>(s, tid, nk, a, Z, tie, group, j, cols, out_rs, out_cnt, out_tie);
}

// ---- the long class: column cols_list[slot], its entries at seg[slot] .. seg[slot + 1] of the batch's scratch ----
template <typename T>
__global__ void __launch_bounds__(BLOCK) rank_long_build_kernel(const int64_t* __restrict__ ptr, const int32_t* __restrict__ idx,
                                                                const T* __restrict__ val, const int32_t* __restrict__ labels, int nk,
                                                                const int32_t* __restrict__ cols_list, const uint32_t* __restrict__ seg,
                                                                typename Keys<T>::K* __restrict__ keys, uint16_t* __restrict__ labs,
                                                                uint32_t* __restrict__ meta) {
  using K = typename Keys<T>::K;
  __shared__ uint32_t counts[4];
  const int slot = blockIdx.x, tid = threadIdx.x;
  const int64_t e0 = ptr[cols_list[slot]];
  const uint32_t base = seg[slot], len = seg[slot + 1] - base;
  if (tid < 2) counts[tid] = 0u;
  __syncthreads();
  uint32_t kept = 0, neg = 0;
  for (uint32_t p = tid; p < len; p += BLOCK) {
    K key;
    uint16_t lab;
    rank_entry<T>(val[e0 + p], labels[idx[e0 + p]], nk, key, lab, kept, neg);
    keys[base + p] = key;
    labs[base + p] = lab;
  }
  atomicAdd(&counts[0], kept);
  atomicAdd(&counts[1], neg);
  __syncthreads();
  if (tid < 2) meta[2 * slot + tid] = counts[tid];
}

template <typename T>
__global__ void __launch_bounds__(BLOCK) rank_long_walk_kernel(const typename Keys<T>::K* __restrict__ keys, const uint16_t* __restrict__ labs,
                                                               const int32_t* __restrict__ cols_list, const uint32_t* __restrict__ seg,
                                                               const uint32_t* __restrict__ meta, int64_t cols, int nk,
                                                               const unsigned long long* __restrict__ group, int64_t M,
                                                               long long* __restrict__ out_rs, uint32_t* __restrict__ out_cnt,
                                                               double* __restrict__ out_tie) {
  using K = typename Keys<T>::K;
  static_assert(kRankWalkChunk == BLOCK, "a step of the walk is one position per thread");
  extern __shared__ __attribute__((aligned(16))) char lds_rank[];
  const int slot = blockIdx.x, tid = threadIdx.x;
  const RankLds<K> s(lds_rank, 0, nk, BLOCK);
  for (int b = tid; b < nk; b += BLOCK) {
    s.rs[b] = 0ull;
    s.cnt[b] = 0u;
  }
  __syncthreads();
  const int64_t L = meta[2 * slot], a = meta[2 * slot + 1], Z = M - L;
  double tie = 0.0;
  rank_accumulate<K>(keys + seg[slot], labs + seg[slot], L, a, Z, tid, BLOCK, nk, s.rs, s.cnt, tie);
  rank_finish<BLOCK, K>(s, tid, nk, a, Z, tie, group, (int64_t)cols_list[slot], cols, out_rs, out_cnt, out_tie);
}

// ---- the counts alone (no ranks asked for): a wave per column of any length, cnt[g][j] = kept entries of group g ----
template <typename T>
__global__ void __launch_bounds__(BLOCK) rank_count_kernel(const int64_t* __restrict__ ptr, const int32_t* __restrict__ idx,
                                                           const T* __restrict__ val, int64_t cols, const int32_t* __restrict__ labels,
                                                           int nk, uint32_t* __restrict__ out_cnt) {
  extern __shared__ __attribute__((aligned(16))) char lds_rank[];
  const int lane = threadIdx.x % WAVE, w = threadIdx.x / WAVE;
  uint32_t* cnt = reinterpret_cast<uint32_t*>(lds_rank) + (size_t)w * nk;
  const int64_t j = (int64_t)blockIdx.x * (BLOCK / WAVE) + w;
  if (j >= cols) return;   // (wave-uniform)
  for (int b = lane; b < nk; b += WAVE) cnt[b] = 0u;
  group_sync<WAVE>();
  const int64_t e1 = ptr[j + 1];
  for (int64_t e = ptr[j] + lane; e < e1; e += WAVE) {
    const int32_t code = labels[idx[e]];
    if ((unsigned)code < (unsigned)nk && val[e] != (T)0) atomicAdd(&cnt[code], 1u);
  }
  group_sync<WAVE>();
  for (int b = lane; b < nk; b += WAVE) out_cnt[(int64_t)b * cols + j] = cnt[b];
}

// ---- group sizes: a histogram of the labels in [0, nk) per workgroup in LDS, flushed with integer atomics ----
__global__ void __launch_bounds__(BLOCK) rank_group_sizes_kernel(const int32_t* __restrict__ labels, int64_t m, int nk,
                                                                 unsigned long long* __restrict__ group) {
  extern __shared__ __attribute__((aligned(16))) char lds_rank[];
  uint32_t* hist = reinterpret_cast<uint32_t*>(lds_rank);
  for (int b = threadIdx.x; b < nk; b += BLOCK) hist[b] = 0u;
  __syncthreads();
  for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < m; i += (int64_t)gridDim.x * BLOCK) {
    const int32_t code = labels[i];
    if ((unsigned)code < (unsigned)nk) atomicAdd(&hist[code], 1u);
  }
  __syncthreads();
  for (int b = threadIdx.x; b < nk; b += BLOCK)
    if (hist[b]) atomicAdd(&group[b], (unsigned long long)hist[b]);
}

template <typename F>
void launch_with_lds(F kernel, size_t lds, LdsAttrState& attr) {
  ensure_dynamic_lds(reinterpret_cast<const void*>(kernel), lds, attr);
}

unsigned blocks_for(int64_t items, int per_block, const char* who) {
  const int64_t blocks = (items + per_block - 1) / per_block;
  SAPCA_CHECK(blocks < ((int64_t)1 << 31), SAPCA_ERR_ARG, std::string(who) + ": too many columns");
  return (unsigned)blocks;
}

}  // namespace

void rank_group_sizes(const int32_t* labels, int64_t m, int nk, unsigned long long* group, hipStream_t s) {
  SAPCA_HIP(hipMemsetAsync(group, 0, (size_t)nk * sizeof(unsigned long long), s));
  if (m == 0) return;
  const unsigned blocks = (unsigned)std::min<int64_t>((m + BLOCK - 1) / BLOCK, 1024);
  hipLaunchKernelGGL(rank_group_sizes_kernel, dim3(blocks), dim3(BLOCK), (size_t)nk * sizeof(uint32_t), s, labels, m, nk, group);
  SAPCA_HIP(hipGetLastError());
}

template <typename T>
void rank_count_nonzero(const CsrView<T>& At, const int32_t* labels, int nk, uint32_t* cnt, hipStream_t s) {
  if (At.rows == 0) return;
  hipLaunchKernelGGL((rank_count_kernel<T>), dim3(blocks_for(At.rows, BLOCK / WAVE, "rank_count_nonzero")), dim3(BLOCK),
                     (size_t)(BLOCK / WAVE) * nk * sizeof(uint32_t), s, At.ptr, At.idx, At.val, At.rows, labels, nk, cnt);
  SAPCA_HIP(hipGetLastError());
}

template <typename T>
void rank_sums_lds(const CsrView<T>& At, const int32_t* labels, int nk, const unsigned long long* group, int64_t M, long long* rs,
                   uint32_t* cnt, double* tie, hipStream_t s) {
  using K = typename Keys<T>::K;
  if (At.rows == 0) return;
  {
    constexpr int PER = BLOCK / WAVE;
    const size_t lds = PER * RankLds<K>::bytes(kRankWaveMax, nk, WAVE);
    static LdsAttrState attr;
    launch_with_lds(&rank_lds_kernel<T, WAVE, kRankWaveMax>, lds, attr);
    hipLaunchKernelGGL((rank_lds_kernel<T, WAVE, kRankWaveMax>), dim3(blocks_for(At.rows, PER, "rank_sums_lds")), dim3(BLOCK), lds, s,
                       At.ptr, At.idx, At.val, At.rows, labels, nk, group, M, -1, kRankWaveMax, rs, cnt, tie);
    SAPCA_HIP(hipGetLastError());
  }
  {
    const size_t lds = RankLds<K>::bytes(kRankLdsMax, nk, BLOCK);
    static LdsAttrState attr;
    launch_with_lds(&rank_lds_kernel<T, BLOCK, kRankLdsMax>, lds, attr);
    hipLaunchKernelGGL((rank_lds_kernel<T, BLOCK, kRankLdsMax>), dim3(blocks_for(At.rows, 1, "rank_sums_lds")), dim3(BLOCK), lds, s,
                       At.ptr, At.idx, At.val, At.rows, labels, nk, group, M, kRankWaveMax, kRankLdsMax, rs, cnt, tie);
    SAPCA_HIP(hipGetLastError());
  }
}

template <typename T>
void rank_sums_long(const CsrView<T>& At, const int32_t* labels, int nk, const unsigned long long* group, int64_t M,
                    const int32_t* cols_list, const uint32_t* seg, int nseg, uint32_t total, DevBuf& scratch, long long* rs, uint32_t* cnt,
                    double* tie, hipStream_t s) {
  using K = typename Keys<T>::K;
  if (nseg == 0) return;
  const auto up256 = [](size_t b) { return (b + 255) / 256 * 256; };
  size_t sort_bytes = 0;
  SAPCA_HIP(rocprim::segmented_radix_sort_pairs(nullptr, sort_bytes, (const K*)nullptr, (K*)nullptr, (const uint16_t*)nullptr,
                                                (uint16_t*)nullptr, total, (unsigned)nseg, seg, seg + 1, 0u, (unsigned)(8 * sizeof(K)), s));
  const size_t kb = up256((size_t)total * sizeof(K)), lb = up256((size_t)total * sizeof(uint16_t)), mb = up256((size_t)nseg * 2 * sizeof(uint32_t));
  char* base = scratch.as<char>(2 * kb + 2 * lb + mb + sort_bytes + 256);
  K* keys_in = reinterpret_cast<K*>(base);
  K* keys_out = reinterpret_cast<K*>(base + kb);
  uint16_t* labs_in = reinterpret_cast<uint16_t*>(base + 2 * kb);
  uint16_t* labs_out = reinterpret_cast<uint16_t*>(base + 2 * kb + lb);
  uint32_t* meta = reinterpret_cast<uint32_t*>(base + 2 * kb + 2 * lb);
  void* tmp = base + 2 * kb + 2 * lb + mb;
  hipLaunchKernelGGL((rank_long_build_kernel<T>), dim3((unsigned)nseg), dim3(BLOCK), 0, s, At.ptr, At.idx, At.val, labels, nk, cols_list, seg,
                     keys_in, labs_in, meta);
  SAPCA_HIP(hipGetLastError());
  SAPCA_HIP(rocprim::segmented_radix_sort_pairs(tmp, sort_bytes, keys_in, keys_out, labs_in, labs_out, total, (unsigned)nseg, seg, seg + 1, 0u,
                                                (unsigned)(8 * sizeof(K)), s));
  const size_t lds = RankLds<K>::bytes(0, nk, BLOCK);
  hipLaunchKernelGGL((rank_long_walk_kernel<T>), dim3((unsigned)nseg), dim3(BLOCK), lds, s, keys_out, labs_out, cols_list, seg, meta, At.rows,
                     nk, group, M, rs, cnt, tie);
  SAPCA_HIP(hipGetLastError());
}

#define INSTANTIATE(T)                                                                                                                  \
  template void rank_count_nonzero<T>(const CsrView<T>&, const int32_t*, int, uint32_t*, hipStream_t);                                 \
  template void rank_sums_lds<T>(const CsrView<T>&, const int32_t*, int, const unsigned long long*, int64_t, long long*, uint32_t*,    \
                                 double*, hipStream_t);                                                                                 \
  template void rank_sums_long<T>(const CsrView<T>&, const int32_t*, int, const unsigned long long*, int64_t, const int32_t*,          \
                                  const uint32_t*, int, uint32_t, DevBuf&, long long*, uint32_t*, double*, hipStream_t);
INSTANTIATE(float)
INSTANTIATE(double)
#undef INSTANTIATE

}  // namespace k
}  // namespace sapca
