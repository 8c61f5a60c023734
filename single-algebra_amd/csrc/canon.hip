// The gate in front of the device entry points (sapca_check_csr_device_*, sapca_canonicalize_csr_device_*): is a resident
// CSR safe (offsets, column range) and canonical (columns ascending and unique inside a row), and if it is not canonical,
// the same matrix with every row sorted and equal columns summed.
//
// CHECK, two kernels.  canon_offsets_kernel reads ptr[0 .. m] only; its verdict crosses to the host before anything
// touches an entry, so the entry pass never leaves [0, nnz).  canon_entries_kernel reads idx and val once.  Its work is cut
// over ENTRIES, select.hip's cut (a workgroup owns kCheckSpan consecutive positions, finds its rows by binary search in
// the offsets and stages them in LDS), not over rows as count_kept_kernel does: the pass is a pure stream with no per-row
// result, a wave per row would idle 61 lanes on a 3-entry row and leave a 60,000-entry row to one wave, and the entry cut
// gives 16-byte loads at any row length.  A predecessor is compared inside a row only (position > the row's offset); the
// column tests are unsigned, so a negative index is out of range.  Counts are sums of per-thread counts (integer atomics,
// one per workgroup and counter), first rows are 64-bit atomicMin: exact and independent of the launch geometry.  Per
// row, "has a descent" / "has an adjacent duplicate" are OR-ed into LDS and from there once per (row, span) into a
// per-row word; the workgroup that sets a row's descent bit first counts the row, so unsorted_rows is exact too.
//
// CANONICALIZE: the three arrays are copied with stream_copy16; rows whose word is set are listed by length class (the
// order of a list varies from run to run, the result does not) and sorted from the SOURCE into the copy -- the source is
// resident and untouched, so the values are gathered from it and no second value buffer is needed.  The sort key is
// (column << 32 | position in the row): unique, so any network is stable and the output deterministic.  The network is
// the bitonic sorter in its one-direction form (a "flip" step i <-> i ^ (k - 1), then halving steps i <-> i + j; the
// smaller key always goes to the lower position).  Keys beyond the row's length would be +infinity and never move, so
// pairs that reach past the length are skipped and a row needs no padding to a power of two:
//   <= 64 entries   one wave, keys and values in registers, exchanges by __shfl_xor;
//   <= kLdsCap      one workgroup, keys in 32 KiB of LDS (static, four workgroups per CU: chosen for occupancy; C2's rows of
//                   about 600 entries sort 1,024 slots), values gathered through the positions in the sorted keys;
//   longer          one workgroup of 1,024 threads, keys in global work space (8 bytes per entry of such rows): slow,
//                   rare, correct.
// Each sorted row counts its distinct columns.  If nothing merged anywhere the copy is the result.  Otherwise the distinct
// counts are scanned into new offsets and one fill pass (a wave per row) writes every run of equal columns as one entry
// whose value is the run's sum, added left to right in T by the lane that owns the run's head; an entry that does not
// merge moves as its bit pattern.  Only the duplicate case pays this second pass, and it is cut over rows: it is bound by
// the rows that merge, not built for skew.
// Limit: a row has fewer than 2^32 entries (the position half of the key).
#include <algorithm>
#include <string>
#include <type_traits>

#include "kernels.h"

namespace sapca {
namespace k {

namespace {

constexpr int kCheckSpan = 4096;     // entry positions per workgroup (a multiple of 4)
constexpr int kCheckRows = 2048;     // rows staged in LDS at a time (offsets 16 KiB + flags 8 KiB); a span over more takes turns
constexpr int kCheckThreads = 256;
constexpr int kWaveCap = 64;         // rows up to this length sort in one wave
constexpr int kLdsCap = 4096;        // .. up to this length in one workgroup's LDS
constexpr int kLdsThreads = 256;
constexpr int kLongThreads = 1024;
constexpr unsigned long long kNone = ~0ull;

typedef unsigned long long u64;

// the last index i in [0, count) with off[i] <= p; the caller guarantees off[0] <= p (of a run of equal offsets the last)
template <typename P>
__device__ inline int64_t last_not_above(P off, int64_t count, int64_t p) {
  int64_t lo = 0, hi = count;
  while (hi - lo > 1) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (off[mid] <= p) lo = mid;
    else hi = mid;
  }
  return lo;
}

__global__ void canon_offsets_kernel(const int64_t* __restrict__ ptr, int64_t m, int64_t nnz, u64* __restrict__ ctr) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r > m) return;
  bool bad = false;
  if (r == 0) bad = ptr[0] != 0;
  if (r < m) bad = bad || ptr[r + 1] < ptr[r];
  else bad = bad || ptr[m] != nnz;
  if (bad) atomicMin(&ctr[kCtrFirstBadOffset], (u64)r);
}

struct alignas(16) Words4 { uint32_t w[4]; };

__device__ inline void load4(uint32_t (&x)[4], const uint32_t* src) {   // (src aligned to a word only)
  Words4 v;
  __builtin_memcpy(&v, src, sizeof(v));
  x[0] = v.w[0]; x[1] = v.w[1]; x[2] = v.w[2]; x[3] = v.w[3];
}
__device__ inline void load4(uint64_t (&x)[4], const uint64_t* src) {
  Words4 a, b;
  __builtin_memcpy(&a, src, sizeof(a));
  __builtin_memcpy(&b, src + 2, sizeof(b));
  x[0] = (uint64_t)a.w[0] | (uint64_t)a.w[1] << 32; x[1] = (uint64_t)a.w[2] | (uint64_t)a.w[3] << 32;
  x[2] = (uint64_t)b.w[0] | (uint64_t)b.w[1] << 32; x[3] = (uint64_t)b.w[2] | (uint64_t)b.w[3] << 32;
}
__device__ inline bool nonfinite_bits(uint32_t b) { return (b & 0x7f800000u) == 0x7f800000u; }
__device__ inline bool nonfinite_bits(uint64_t b) { return (b & 0x7ff0000000000000ull) == 0x7ff0000000000000ull; }
__device__ inline bool zero_bits(uint32_t b) { return (b << 1) == 0u; }
__device__ inline bool zero_bits(uint64_t b) { return (b << 1) == 0ull; }

__device__ inline u64 wave_sum(u64 x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off);
  return x;
}
__device__ inline u64 wave_min(u64 x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const u64 y = __shfl_xor(x, off);
    x = y < x ? y : x;
  }
  return x;
}

// V: the value's bit pattern.  ptr is sound (canon_offsets_kernel passed), nnz > 0.  row_bits[r] |= 1 (a descent) | 2 (an
// adjacent duplicate).
template <typename V>
__global__ void __launch_bounds__(kCheckThreads)
canon_entries_kernel(const int64_t* __restrict__ ptr, const uint32_t* __restrict__ idx, const V* __restrict__ val, int64_t m,
                     uint32_t n, int64_t nnz, uint32_t* __restrict__ row_bits, u64* __restrict__ ctr) {
  __shared__ int64_t s_off[kCheckRows + 1];
  __shared__ uint32_t s_bits[kCheckRows];
  __shared__ int64_t s_range[2];
  __shared__ u64 s_sum[5], s_min[4];
  const int64_t p0 = (int64_t)blockIdx.x * kCheckSpan;
  const int64_t p1 = min(nnz, p0 + kCheckSpan);
  if (p0 >= p1) return;
  if (threadIdx.x < 2) s_range[threadIdx.x] = last_not_above(ptr, m + 1, threadIdx.x == 0 ? p0 : p1 - 1);
  if (threadIdx.x < 5) s_sum[threadIdx.x] = 0;
  if (threadIdx.x < 4) s_min[threadIdx.x] = kNone;
  __syncthreads();
  const int64_t r_first = s_range[0], r_last = s_range[1];
  u64 n_range = 0, n_dup = 0, n_nonfinite = 0, n_zero = 0, n_unsorted_rows = 0;
  u64 f_range = kNone, f_dup = kNone, f_nonfinite = kNone, f_unsorted = kNone;
  for (int64_t rc = r_first; rc <= r_last; rc += kCheckRows) {
    const int cnt = (int)min((int64_t)kCheckRows, r_last + 1 - rc);   // rows rc .. rc + cnt - 1, all < m
    if (rc != r_first) __syncthreads();
    for (int i = threadIdx.x; i <= cnt; i += kCheckThreads) {
      s_off[i] = ptr[rc + i];
      if (i < cnt) s_bits[i] = 0u;
    }
    __syncthreads();
    const int64_t q0 = max(p0, s_off[0]), q1 = min(p1, s_off[cnt]);
    for (int64_t g = (q0 >> 2) + threadIdx.x; 4 * g < q1; g += kCheckThreads) {
      const int64_t lo = max(4 * g, q0), hi = min(4 * g + 4, q1);
      int i = (int)last_not_above(s_off, cnt, lo);
      uint32_t c[4];
      V v[4];
      if (hi - lo == 4) {
        load4(c, idx + lo);
        load4(v, val + lo);
      } else {
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (lo + u < hi) {
            c[u] = idx[lo + u];
            v[u] = val[lo + u];
          }
      }
      uint32_t prev = lo > s_off[i] ? idx[lo - 1] : 0u;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int64_t q = lo + u;
        if (q < hi) {
          while (s_off[i + 1] <= q) ++i;   // (skips empty rows; ends below cnt because s_off[cnt] >= q1 > q)
          const u64 row = (u64)(rc + i);
          if (c[u] >= n) {
            ++n_range;
            f_range = row < f_range ? row : f_range;
          }
          if (q > s_off[i]) {
            if (c[u] < prev) {
              atomicOr(&s_bits[i], 1u);
            } else if (c[u] == prev) {
              atomicOr(&s_bits[i], 2u);
              ++n_dup;
              f_dup = row < f_dup ? row : f_dup;
            }
          }
          if (nonfinite_bits(v[u])) {
            ++n_nonfinite;
            f_nonfinite = row < f_nonfinite ? row : f_nonfinite;
          }
          n_zero += zero_bits(v[u]) ? 1u : 0u;
          prev = c[u];
        }
      }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < cnt; i += kCheckThreads) {
      const uint32_t b = s_bits[i];
      if (b) {
        const uint32_t old = atomicOr(&row_bits[rc + i], b);
        if ((b & ~old) & 1u) {   // this workgroup is the first to see a descent in the row
          ++n_unsorted_rows;
          const u64 row = (u64)(rc + i);
          f_unsorted = row < f_unsorted ? row : f_unsorted;
        }
      }
    }
  }
  u64 sums[5] = {n_range, n_unsorted_rows, n_dup, n_nonfinite, n_zero};
  u64 mins[4] = {f_range, f_unsorted, f_dup, f_nonfinite};
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int j = 0; j < 5; ++j) {
    const u64 x = wave_sum(sums[j]);
    if (lane == 0 && x) atomicAdd(&s_sum[j], x);
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const u64 x = wave_min(mins[j]);
    if (lane == 0 && x != kNone) atomicMin(&s_min[j], x);
  }
  __syncthreads();
  // (the slots of kernels.h are in this order: out of range, unsorted, duplicate, non-finite, stored zeros)
  if (threadIdx.x < 5 && s_sum[threadIdx.x]) atomicAdd(&ctr[kCtrColsOutOfRange + threadIdx.x], s_sum[threadIdx.x]);
  if (threadIdx.x >= 64 && threadIdx.x < 68 && s_min[threadIdx.x - 64] != kNone)
    atomicMin(&ctr[kCtrFirstOutOfRange + (threadIdx.x - 64)], s_min[threadIdx.x - 64]);
}

// rows with a set word -> lists[class * m + ..] (class by length); a long row also takes its share of the key work space
__global__ void canon_list_kernel(const int64_t* __restrict__ ptr, const uint32_t* __restrict__ row_bits, int64_t m,
                                  uint32_t* __restrict__ lists, u64* __restrict__ long_off, u64* __restrict__ ctr) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= m || row_bits[r] == 0u) return;
  const int64_t len = ptr[r + 1] - ptr[r];
  const int cls = len <= kWaveCap ? 0 : len <= kLdsCap ? 1 : 2;
  const u64 pos = atomicAdd(&ctr[kCtrListWave + cls], 1ull);
  lists[(int64_t)cls * m + (int64_t)pos] = (uint32_t)r;
  if (cls == 2) long_off[pos] = atomicAdd(&ctr[kCtrLongEntries], (u64)len);
}

template <typename V>
__device__ inline V shfl_bits(V x, int src) {
  if constexpr (sizeof(V) == 4) return (V)__shfl((unsigned)x, src);
  else return (V)__shfl((u64)x, src);
}

// one wave per listed row of at most 64 entries
template <typename V>
__global__ void __launch_bounds__(256)
canon_sort_wave_kernel(const int64_t* __restrict__ ptr, const uint32_t* __restrict__ idx, const V* __restrict__ val,
                       const uint32_t* __restrict__ list, int64_t count, uint32_t* __restrict__ out_idx, V* __restrict__ out_val,
                       uint32_t* __restrict__ distinct, u64* __restrict__ ctr) {
  const int lane = threadIdx.x & 63;
  const int64_t w = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (w >= count) return;
  const int64_t r = list[w];
  const int64_t e0 = ptr[r];
  const int len = (int)(ptr[r + 1] - e0);
  u64 key = lane < len ? ((u64)idx[e0 + lane] << 32 | (u64)lane) : kNone;
  const V v = lane < len ? val[e0 + lane] : (V)0;
#pragma unroll
  for (int k = 2; k <= 64; k <<= 1) {
    {
      const u64 other = __shfl_xor(key, k - 1);
      const bool lower = (lane & (k >> 1)) == 0;   // lane < lane ^ (k - 1)
      key = lower == (key < other) ? key : other;
    }
#pragma unroll
    for (int j = k >> 2; j >= 1; j >>= 1) {
      const u64 other = __shfl_xor(key, j);
      const bool lower = (lane & j) == 0;
      key = lower == (key < other) ? key : other;
    }
  }
  const uint32_t c = (uint32_t)(key >> 32);
  const V sv = shfl_bits(v, (int)(key & 63ull));
  const uint32_t pc = __shfl_up(c, 1);
  const bool head = lane < len && (lane == 0 || c != pc);
  const int heads = __popcll(__ballot(head));
  if (lane < len) {
    out_idx[e0 + lane] = c;
    out_val[e0 + lane] = sv;
  }
  if (lane == 0) {
    distinct[r] = (uint32_t)heads;
    if (len > heads) atomicAdd(&ctr[kCtrMerged], (u64)(len - heads));
  }
}

__device__ inline void order_pair(u64* keys, int64_t i, int64_t l) {
  const u64 a = keys[i], b = keys[l];
  if (b < a) {
    keys[i] = b;
    keys[l] = a;
  }
}

// keys[0 .. len) ascending, by every thread of the workgroup (keys: LDS or global).  Ends behind a barrier.
__device__ inline void sort_keys(u64* keys, int64_t len, int tid, int nthreads) {
  int lg = 0;
  while (((int64_t)1 << lg) < len) ++lg;
  const int64_t pairs = lg ? (int64_t)1 << (lg - 1) : 0;
  for (int s = 1; s <= lg; ++s) {   // blocks of k = 2^s
    const int64_t k = (int64_t)1 << s, half = k >> 1;
    for (int64_t t = tid; t < pairs; t += nthreads) {
      const int64_t base = (t >> (s - 1)) << s, off = t & (half - 1);
      const int64_t l = base + k - 1 - off;
      if (l < len) order_pair(keys, base + off, l);
    }
    __syncthreads();
    for (int js = s - 2; js >= 0; --js) {
      const int64_t j = (int64_t)1 << js;
      for (int64_t t = tid; t < pairs; t += nthreads) {
        const int64_t i = ((t >> js) << (js + 1)) + (t & (j - 1));
        if (i + j < len) order_pair(keys, i, i + j);
      }
      __syncthreads();
    }
  }
}

// sorted keys -> the row's output (values gathered from the source), the row's distinct columns and merged entries
template <typename V>
__device__ inline void write_sorted_row(const u64* keys, int64_t e0, int64_t len, const V* __restrict__ val, int64_t r,
                                        uint32_t* __restrict__ out_idx, V* __restrict__ out_val, uint32_t* __restrict__ distinct,
                                        u64* __restrict__ ctr, unsigned* s_heads, int tid, int nthreads) {
  unsigned heads = 0;
  for (int64_t i = tid; i < len; i += nthreads) {
    const u64 key = keys[i];
    const uint32_t c = (uint32_t)(key >> 32);
    heads += (i == 0 || (uint32_t)(keys[i - 1] >> 32) != c) ? 1u : 0u;
    out_idx[e0 + i] = c;
    out_val[e0 + i] = val[e0 + (int64_t)(key & 0xffffffffull)];
  }
  if (heads) atomicAdd(s_heads, heads);
  __syncthreads();
  if (tid == 0) {
    const unsigned h = *s_heads;
    distinct[r] = h;
    if ((u64)len > h) atomicAdd(&ctr[kCtrMerged], (u64)len - h);
  }
}

// one workgroup per listed row of 65 .. kLdsCap entries
template <typename V>
__global__ void __launch_bounds__(kLdsThreads)
canon_sort_lds_kernel(const int64_t* __restrict__ ptr, const uint32_t* __restrict__ idx, const V* __restrict__ val,
                      const uint32_t* __restrict__ list, uint32_t* __restrict__ out_idx, V* __restrict__ out_val,
                      uint32_t* __restrict__ distinct, u64* __restrict__ ctr) {
  __shared__ u64 keys[kLdsCap];
  __shared__ unsigned s_heads;
  const int64_t r = list[blockIdx.x];
  const int64_t e0 = ptr[r];
  const int64_t len = min(ptr[r + 1] - e0, (int64_t)kLdsCap);   // (the list holds no longer row; the bound keeps LDS safe)
  if (threadIdx.x == 0) s_heads = 0u;
  for (int64_t i = threadIdx.x; i < len; i += kLdsThreads) keys[i] = (u64)idx[e0 + i] << 32 | (u64)i;
  __syncthreads();
  sort_keys(keys, len, threadIdx.x, kLdsThreads);
  write_sorted_row(keys, e0, len, val, r, out_idx, out_val, distinct, ctr, &s_heads, threadIdx.x, kLdsThreads);
}

// one workgroup per listed row of more than kLdsCap entries; its keys at key_space + long_off[position in the list]
template <typename V>
__global__ void __launch_bounds__(kLongThreads)
canon_sort_long_kernel(const int64_t* __restrict__ ptr, const uint32_t* __restrict__ idx, const V* __restrict__ val,
                       const uint32_t* __restrict__ list, const u64* __restrict__ long_off, u64* key_space,
                       uint32_t* __restrict__ out_idx, V* __restrict__ out_val, uint32_t* __restrict__ distinct,
                       u64* __restrict__ ctr) {
  __shared__ unsigned s_heads;
  const int64_t r = list[blockIdx.x];
  const int64_t e0 = ptr[r];
  const int64_t len = ptr[r + 1] - e0;
  u64* keys = key_space + long_off[blockIdx.x];
  if (threadIdx.x == 0) s_heads = 0u;
  for (int64_t i = threadIdx.x; i < len; i += kLongThreads) keys[i] = (u64)idx[e0 + i] << 32 | (u64)i;
  __syncthreads();
  sort_keys(keys, len, threadIdx.x, kLongThreads);
  write_sorted_row(keys, e0, len, val, r, out_idx, out_val, distinct, ctr, &s_heads, threadIdx.x, kLongThreads);
}

// new_ptr[r] = entries row r keeps (its distinct columns if it was sorted, else its length); new_ptr[m] = 0 for the scan
__global__ void canon_lengths_kernel(const int64_t* __restrict__ ptr, const uint32_t* __restrict__ row_bits,
                                     const uint32_t* __restrict__ distinct, int64_t m, int64_t* __restrict__ new_ptr) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r < m) new_ptr[r] = row_bits[r] ? (int64_t)distinct[r] : ptr[r + 1] - ptr[r];
  else if (r == m) new_ptr[r] = 0;
}

template <typename T, typename V>
__device__ inline T from_bits(V b) {
  T x;
  __builtin_memcpy(&x, &b, sizeof(T));
  return x;
}
template <typename T, typename V>
__device__ inline V to_bits(T x) {
  V b;
  __builtin_memcpy(&b, &x, sizeof(T));
  return b;
}

// (idx, val at the OLD offsets ptr: every row sorted) -> (out_idx, out_val at new_ptr): one entry per run of equal columns
template <typename T, typename V>
__global__ void __launch_bounds__(256)
canon_merge_kernel(const int64_t* __restrict__ ptr, const uint32_t* __restrict__ idx, const V* __restrict__ val, int64_t m,
                   const int64_t* __restrict__ new_ptr, uint32_t* __restrict__ out_idx, V* __restrict__ out_val) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t r = wave; r < m; r += nwaves) {
    const int64_t e0 = ptr[r], e1 = ptr[r + 1];
    int64_t out = new_ptr[r];
    if (new_ptr[r + 1] - out == e1 - e0) {   // nothing merges in this row
      for (int64_t e = e0 + lane; e < e1; e += 64) {
        out_idx[out + (e - e0)] = idx[e];
        out_val[out + (e - e0)] = val[e];
      }
      continue;
    }
    for (int64_t base = e0; base < e1; base += 64) {
      const int64_t e = base + lane;
      const uint32_t c = e < e1 ? idx[e] : 0u;
      const bool head = e < e1 && (e == e0 || idx[e - 1] != c);
      const u64 mask = __ballot(head);
      if (head) {
        V b = val[e];
        int64_t j = e + 1;
        if (j < e1 && idx[j] == c) {
          T sum = from_bits<T, V>(b);
          for (; j < e1 && idx[j] == c; ++j) sum = sum + from_bits<T, V>(val[j]);   // left to right, in T
          b = to_bits<T, V>(sum);
        }
        const int64_t pos = out + __popcll(mask & ((1ull << lane) - 1ull));
        out_idx[pos] = c;
        out_val[pos] = b;
      }
      out += __popcll(mask);
    }
  }
}

template <typename T>
using bits_of = typename std::conditional<sizeof(T) == 4, uint32_t, uint64_t>::type;

unsigned blocks_for(int64_t items, int per_block, const char* what) {
  const int64_t b = (items + per_block - 1) / per_block;
  SAPCA_CHECK(b < ((int64_t)1 << 31), SAPCA_ERR_ARG, std::string(what) + ": the matrix is too large for one launch");
  return (unsigned)std::max<int64_t>(b, 1);
}

}  // namespace

void canon_check_offsets(const int64_t* ptr, int64_t m, int64_t nnz, unsigned long long* ctr, hipStream_t s) {
  // first rows start at "none" (all bits set), counts at zero
  SAPCA_HIP(hipMemsetAsync(ctr, 0xff, kCtrFirstCount * sizeof(u64), s));
  SAPCA_HIP(hipMemsetAsync(ctr + kCtrFirstCount, 0, (kCtrSlots - kCtrFirstCount) * sizeof(u64), s));
  hipLaunchKernelGGL(canon_offsets_kernel, dim3(blocks_for(m + 1, 256, "check_csr")), dim3(256), 0, s, ptr, m, nnz, ctr);
  SAPCA_HIP(hipGetLastError());
}

template <typename T>
void canon_check_entries(const CsrView<T>& A, uint32_t* row_bits, unsigned long long* ctr, hipStream_t s) {
  if (A.rows > 0) SAPCA_HIP(hipMemsetAsync(row_bits, 0, (size_t)A.rows * sizeof(uint32_t), s));
  if (A.nnz <= 0 || A.rows <= 0) return;
  using V = bits_of<T>;
  hipLaunchKernelGGL((canon_entries_kernel<V>), dim3(blocks_for(A.nnz, kCheckSpan, "check_csr")), dim3(kCheckThreads), 0, s, A.ptr,
                     reinterpret_cast<const uint32_t*>(A.idx), reinterpret_cast<const V*>(A.val), A.rows, (uint32_t)A.cols, A.nnz,
                     row_bits, ctr);
  SAPCA_HIP(hipGetLastError());
}

void canon_list_rows(const int64_t* ptr, const uint32_t* row_bits, int64_t m, uint32_t* lists, unsigned long long* long_off,
                     unsigned long long* ctr, hipStream_t s) {
  if (m <= 0) return;
  hipLaunchKernelGGL(canon_list_kernel, dim3(blocks_for(m, 256, "canonicalize")), dim3(256), 0, s, ptr, row_bits, m, lists, long_off,
                     ctr);
  SAPCA_HIP(hipGetLastError());
}

int64_t canon_lds_cap() { return kLdsCap; }

template <typename T>
void canon_sort_rows(const CsrView<T>& A, const uint32_t* lists, const unsigned long long* long_off, const int64_t counts[3],
                     unsigned long long* key_space, int32_t* out_idx, T* out_val, uint32_t* distinct, unsigned long long* ctr,
                     hipStream_t s) {
  using V = bits_of<T>;
  const uint32_t* idx = reinterpret_cast<const uint32_t*>(A.idx);
  const V* val = reinterpret_cast<const V*>(A.val);
  uint32_t* o_idx = reinterpret_cast<uint32_t*>(out_idx);
  V* o_val = reinterpret_cast<V*>(out_val);
  if (counts[0] > 0)
    hipLaunchKernelGGL((canon_sort_wave_kernel<V>), dim3(blocks_for(counts[0], 4, "canonicalize")), dim3(256), 0, s, A.ptr, idx, val,
                       lists, counts[0], o_idx, o_val, distinct, ctr);
  if (counts[1] > 0)
    hipLaunchKernelGGL((canon_sort_lds_kernel<V>), dim3(blocks_for(counts[1], 1, "canonicalize")), dim3(kLdsThreads), 0, s, A.ptr, idx,
                       val, lists + A.rows, o_idx, o_val, distinct, ctr);
  if (counts[2] > 0)
    hipLaunchKernelGGL((canon_sort_long_kernel<V>), dim3(blocks_for(counts[2], 1, "canonicalize")), dim3(kLongThreads), 0, s, A.ptr,
                       idx, val, lists + 2 * A.rows, long_off, key_space, o_idx, o_val, distinct, ctr);
  SAPCA_HIP(hipGetLastError());
}

void canon_new_lengths(const int64_t* ptr, const uint32_t* row_bits, const uint32_t* distinct, int64_t m, int64_t* new_ptr,
                       hipStream_t s) {
  hipLaunchKernelGGL(canon_lengths_kernel, dim3(blocks_for(m + 1, 256, "canonicalize")), dim3(256), 0, s, ptr, row_bits, distinct, m,
                     new_ptr);
  SAPCA_HIP(hipGetLastError());
}

template <typename T>
void canon_merge_fill(const int64_t* ptr, const int32_t* idx, const T* val, int64_t m, const int64_t* new_ptr, int32_t* out_idx,
                      T* out_val, hipStream_t s) {
  if (m <= 0) return;
  using V = bits_of<T>;
  const unsigned blocks = (unsigned)std::min<int64_t>((m + 3) / 4, 16384);
  hipLaunchKernelGGL((canon_merge_kernel<T, V>), dim3(blocks), dim3(256), 0, s, ptr, reinterpret_cast<const uint32_t*>(idx),
                     reinterpret_cast<const V*>(val), m, new_ptr, reinterpret_cast<uint32_t*>(out_idx), reinterpret_cast<V*>(out_val));
  SAPCA_HIP(hipGetLastError());
}

template void canon_check_entries<float>(const CsrView<float>&, uint32_t*, unsigned long long*, hipStream_t);
template void canon_check_entries<double>(const CsrView<double>&, uint32_t*, unsigned long long*, hipStream_t);
template void canon_sort_rows<float>(const CsrView<float>&, const uint32_t*, const unsigned long long*, const int64_t[3],
                                     unsigned long long*, int32_t*, float*, uint32_t*, unsigned long long*, hipStream_t);
template void canon_sort_rows<double>(const CsrView<double>&, const uint32_t*, const unsigned long long*, const int64_t[3],
                                      unsigned long long*, int32_t*, double*, uint32_t*, unsigned long long*, hipStream_t);
template void canon_merge_fill<float>(const int64_t*, const int32_t*, const float*, int64_t, const int64_t*, int32_t*, float*,
                                      hipStream_t);
template void canon_merge_fill<double>(const int64_t*, const int32_t*, const double*, int64_t, const int64_t*, int32_t*, double*,
                                       hipStream_t);

}  // namespace k
}  // namespace sapca
