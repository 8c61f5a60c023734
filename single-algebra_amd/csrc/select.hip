// Row selection of a device-resident CSR (sapca_select_rows_csr_device_*): output row i = source row rows[i], in any
// order and with repeats, as an ordinary CSR.  Two stages on one stream:
//   1. offsets: len[i] = ptr[rows[i] + 1] - ptr[rows[i]] into the new offset array, then the exclusive scan of prep.hip;
//   2. fill: the work is cut over OUTPUT ENTRIES, not rows -- a matrix of 3 entries per row would idle a wave per row, and
//      one row of tens of thousands of entries must not run on one wave.  Each workgroup owns kSelectSpan consecutive
//      output positions, finds the rows that intersect them by binary search in the new offsets, stages their offsets and
//      source bases ptr[rows[r]] in LDS and copies index and value position by position.  Source reads are contiguous
//      inside a row; output writes are contiguous throughout and 16 bytes wide.
// Values travel as their bit patterns (uint32_t / uint64_t): NaN payloads, -0.0 and stored zeros arrive as they are.
// No atomics: every output position is written once, by the workgroup that owns it.
// Further down: the same selection with a column mask and / or without stored zeros (sapca_select_submatrix_csr_device_*).
#include <type_traits>

#include "kernels.h"

namespace sapca {
namespace k {

namespace {

constexpr int kSelectSpan = 4096;    // output positions per workgroup (a multiple of 4: every span starts 16-byte aligned)
constexpr int kSelectRows = 2048;    // rows staged in LDS at a time (offsets + bases: 32 KiB); a span over more rows takes turns
constexpr int kSelectThreads = 256;
static_assert(kSelectSpan <= 8192 && kSelectSpan % 4 == 0, "span: at most 8192 positions, whole 16-byte groups");

__global__ void select_lengths_kernel(const int64_t* __restrict__ ptr, const uint64_t* __restrict__ rows, int64_t n_rows,
                                      int64_t* __restrict__ out_ptr) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_rows) {
    const int64_t r = (int64_t)rows[i];
    out_ptr[i] = ptr[r + 1] - ptr[r];
  } else if (i == n_rows) {
    out_ptr[i] = 0;   // (the scan leaves the total here)
  }
}

// the last index i in [0, count) with off[i] <= p; the caller guarantees off[0] <= p.  Upper-bound semantics: of a run of
// equal offsets (empty rows) the LAST is taken, the row that holds position p when p < off[count]
template <typename P>
__device__ inline int64_t last_not_above(P off, int64_t count, int64_t p) {
  int64_t lo = 0, hi = count;   // invariant: off[lo] <= p, (hi == count or off[hi] > p)
  while (hi - lo > 1) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (off[mid] <= p) lo = mid;
    else hi = mid;
  }
  return lo;
}

struct alignas(16) Words4 { uint32_t w[4]; };
struct alignas(16) Long2 { uint64_t w[2]; };

// dst (16-byte aligned) <- four consecutive words from src (aligned to a word only: a row starts anywhere)
__device__ inline void copy4(uint32_t* __restrict__ dst, const uint32_t* __restrict__ src) {
  Words4 v;
  __builtin_memcpy(&v, src, sizeof(v));
  *reinterpret_cast<Words4*>(dst) = v;
}
__device__ inline void copy4(uint64_t* __restrict__ dst, const uint64_t* __restrict__ src) {
  Long2 a, b;
  __builtin_memcpy(&a, src, sizeof(a));
  __builtin_memcpy(&b, src + 2, sizeof(b));
  reinterpret_cast<Long2*>(dst)[0] = a;
  reinterpret_cast<Long2*>(dst)[1] = b;
}
__device__ inline void store4(uint32_t* __restrict__ dst, const uint32_t (&x)[4]) {
  *reinterpret_cast<Words4*>(dst) = Words4{{x[0], x[1], x[2], x[3]}};
}
__device__ inline void store4(uint64_t* __restrict__ dst, const uint64_t (&x)[4]) {
  reinterpret_cast<Long2*>(dst)[0] = Long2{{x[0], x[1]}};
  reinterpret_cast<Long2*>(dst)[1] = Long2{{x[2], x[3]}};
}

// V: the value's bit pattern (uint32_t for f32, uint64_t for f64).  off: the NEW offsets (n_rows + 1), total = off[n_rows] > 0.
template <typename V>
__global__ void __launch_bounds__(kSelectThreads)
select_fill_kernel(const int64_t* __restrict__ ptr, const uint32_t* __restrict__ idx, const V* __restrict__ val,
                   const uint64_t* __restrict__ rows, int64_t n_rows, const int64_t* __restrict__ off, int64_t total,
                   uint32_t* __restrict__ out_idx, V* __restrict__ out_val) {
  __shared__ int64_t s_off[kSelectRows + 1];
  __shared__ int64_t s_base[kSelectRows];
  __shared__ int64_t s_range[2];
  const int64_t p0 = (int64_t)blockIdx.x * kSelectSpan;
  const int64_t p1 = min(total, p0 + kSelectSpan);
  if (p0 >= p1) return;
  // the rows that hold the span's first and last position (off[0] = 0 <= p, off[n_rows] = total > p: both exist)
  if (threadIdx.x < 2) s_range[threadIdx.x] = last_not_above(off, n_rows + 1, threadIdx.x == 0 ? p0 : p1 - 1);
  __syncthreads();
  const int64_t r_first = s_range[0], r_last = s_range[1];
  for (int64_t rc = r_first; rc <= r_last; rc += kSelectRows) {
    const int cnt = (int)min((int64_t)kSelectRows, r_last + 1 - rc);   // rows rc .. rc + cnt - 1, all < n_rows
    if (rc != r_first) __syncthreads();                                // the previous turn's readers are done
    for (int i = threadIdx.x; i <= cnt; i += kSelectThreads) {
      s_off[i] = off[rc + i];
      if (i < cnt) s_base[i] = ptr[rows[rc + i]];
    }
    __syncthreads();
    // this turn's positions: s_off[0] <= q0 and q1 <= s_off[cnt], so every q in [q0, q1) lies in one of the staged rows
    const int64_t q0 = max(p0, s_off[0]), q1 = min(p1, s_off[cnt]);
    for (int64_t g = (q0 >> 2) + threadIdx.x; 4 * g < q1; g += kSelectThreads) {   // groups of four positions, 16-byte aligned
      const int64_t lo = max(4 * g, q0), hi = min(4 * g + 4, q1);
      int i = (int)last_not_above(s_off, cnt, lo);
      if (hi - lo == 4 && s_off[i + 1] >= hi) {   // one row holds all four: 16-byte copies
        const int64_t src = s_base[i] + (lo - s_off[i]);
        copy4(out_idx + lo, idx + src);
        copy4(out_val + lo, val + src);
      } else {
        uint32_t c[4];
        V v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int64_t q = lo + u;
          if (q < hi) {
            while (s_off[i + 1] <= q) ++i;   // (skips empty rows; ends below cnt because s_off[cnt] >= q1 > q)
            const int64_t src = s_base[i] + (q - s_off[i]);
            c[u] = idx[src];
            v[u] = val[src];
          }
        }
        if (hi - lo == 4) {
          store4(out_idx + lo, c);
          store4(out_val + lo, v);
        } else {
#pragma unroll
          for (int u = 0; u < 4; ++u)
            if (lo + u < hi) {
              out_idx[lo + u] = c[u];
              out_val[lo + u] = v[u];
            }
        }
      }
    }
  }
}


// ---- rows and columns in one pass pair (sapca_select_submatrix_csr_device_*) ---------------------------------------------
// The gathered rows (the offsets `goff` of the row selection, never materialised) filtered by a column mask and / or the
// "drop stored zeros" flag.  The work is cut like the fill above: a workgroup per span of kSelectSpan GATHERED positions.
//   count: keep flag of every position of the span -> one count per span; a scan over the spans gives every span's output
//          base and the total;
//   fill:  the same flags into an LDS bit vector with a prefix per word, so the rank of a position in its span is
//          before[w] + popc(bits[w] below it); each kept entry goes to base + rank, its column renumbered through the map,
//          and the workgroup whose span holds goff[i] writes out_ptr[i] = base + rank(goff[i]).
// The column map: one bit per source column (kept) and per 32 columns the number of kept columns before them, built on the
// host (bits[words] | before[words], words = ceil(n / 32)); in LDS up to kSubMapWords words, read from memory above that.
// No atomics; every output word has one writer; the bytes do not depend on how the workgroups are scheduled.
constexpr int kSubRows = 1024;                  // rows staged at a time by these two kernels (16 KiB: the map needs room beside them)
constexpr int kSubWords = kSelectSpan / 32;     // keep flags of a span
constexpr int kSubMapWords = 3072;              // widest LDS-resident map: 98,304 columns, 24 KiB
static_assert(kSelectThreads % 64 == 0 && kSelectSpan % 32 == 0 && kSubWords <= 2 * 64, "one wave scans the span's words, two each");

template <bool kLds>
struct ColumnMap {
  const uint32_t* bits;     // null: every column is kept as it is
  const uint32_t* before;
  uint32_t n;
  __device__ inline bool kept(uint32_t c) const { return bits == nullptr || (c < n && ((bits[c >> 5] >> (c & 31u)) & 1u)); }
  __device__ inline uint32_t renumbered(uint32_t c) const {
    return bits == nullptr ? c : before[c >> 5] + (uint32_t)__popc(bits[c >> 5] & ((1u << (c & 31u)) - 1u));
  }
};

// the map of a kernel: staged in `lds` (2 * words words; visible after the next barrier) or left where it is
template <bool kLds>
__device__ inline ColumnMap<kLds> column_map(const uint32_t* __restrict__ cmap, int words, uint32_t n, uint32_t* lds) {
  if (cmap == nullptr) return ColumnMap<kLds>{nullptr, nullptr, n};
  if (!kLds) return ColumnMap<kLds>{cmap, cmap + words, n};
  for (int w = threadIdx.x; w < 2 * words; w += kSelectThreads) lds[w] = cmap[w];
  return ColumnMap<kLds>{lds, lds + words, n};
}

template <typename V>
__device__ inline bool stored_zero(V v) { return (V)(v << 1) == 0; }   // +0.0 and -0.0; a NaN is not

// the first index i in [0, count) with off[i] >= p, count if there is none
__device__ inline int64_t first_not_below(const int64_t* __restrict__ off, int64_t count, int64_t p) {
  int64_t lo = 0, hi = count;
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (off[mid] < p) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// Walks the gathered positions [p0, p1) of a span in groups of four (group g = positions 4g .. 4g + 3): f(g, src, one_row)
// with src[u] = the source entry of position 4g + u, or -1 where that position is outside this turn of the span; one_row:
// the four are consecutive entries of one source row.  The rows are found and staged as in select_fill_kernel.  Every
// thread of the workgroup makes the same calls in the same order (f may use wave-wide operations), and thread t takes the
// groups congruent to t modulo the workgroup's size, starting from a multiple of eight: eight neighbouring lanes hold one
// 32-position word.  rows == nullptr: source row i is row i.
template <typename F>
__device__ inline void walk_span(const int64_t* __restrict__ ptr, const uint64_t* __restrict__ rows, int64_t n_rows,
                                 const int64_t* __restrict__ off, int64_t p0, int64_t p1, int64_t* s_off, int64_t* s_base,
                                 int64_t* s_range, F&& f) {
  if (threadIdx.x < 2) s_range[threadIdx.x] = last_not_above(off, n_rows + 1, threadIdx.x == 0 ? p0 : p1 - 1);
  __syncthreads();
  const int64_t r_first = s_range[0], r_last = s_range[1];
  for (int64_t rc = r_first; rc <= r_last; rc += kSubRows) {
    const int cnt = (int)min((int64_t)kSubRows, r_last + 1 - rc);
    if (rc != r_first) __syncthreads();
    for (int i = threadIdx.x; i <= cnt; i += kSelectThreads) {
      s_off[i] = off[rc + i];
      if (i < cnt) s_base[i] = ptr[rows ? (int64_t)rows[rc + i] : rc + i];
    }
    __syncthreads();
    const int64_t q0 = max(p0, s_off[0]), q1 = min(p1, s_off[cnt]);
    for (int64_t gb = (q0 >> 5) << 3; 4 * gb < q1; gb += kSelectThreads) {
      const int64_t g = gb + threadIdx.x;
      const int64_t lo = max(4 * g, q0), hi = min(4 * g + 4, q1);
      int64_t src[4] = {-1, -1, -1, -1};
      bool one_row = false;
      if (lo < hi) {
        int i = (int)last_not_above(s_off, cnt, lo);
        one_row = hi - lo == 4 && s_off[i + 1] >= hi;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int64_t q = 4 * g + u;
          if (q >= lo && q < hi) {
            while (s_off[i + 1] <= q) ++i;   // (skips empty rows; ends below cnt because s_off[cnt] >= q1 > q)
            src[u] = s_base[i] + (q - s_off[i]);
          }
        }
      }
      f(g, src, one_row);
    }
  }
}

// bit u: position u of the group is kept
template <bool kLds, typename V>
__device__ inline uint32_t keep_flags(const uint32_t* __restrict__ idx, const V* __restrict__ val, const int64_t (&src)[4], bool one_row,
                                      const ColumnMap<kLds>& map, bool drop_zeros) {
  uint32_t c[4] = {0u, 0u, 0u, 0u};
  V v[4] = {1, 1, 1, 1};
  if (one_row) {
    Words4 w;
    __builtin_memcpy(&w, idx + src[0], sizeof(w));
#pragma unroll
    for (int u = 0; u < 4; ++u) c[u] = w.w[u];
    if (drop_zeros) __builtin_memcpy(v, val + src[0], sizeof(v));
  } else {
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (src[u] >= 0) {
        c[u] = idx[src[u]];
        if (drop_zeros) v[u] = val[src[u]];
      }
  }
  uint32_t nib = 0u;
#pragma unroll
  for (int u = 0; u < 4; ++u)
    if (src[u] >= 0 && map.kept(c[u]) && !(drop_zeros && stored_zero(v[u]))) nib |= 1u << u;
  return nib;
}

template <typename V, bool kLds>
__global__ void __launch_bounds__(kSelectThreads)
submatrix_count_kernel(const int64_t* __restrict__ ptr, const uint32_t* __restrict__ idx, const V* __restrict__ val,
                       const uint64_t* __restrict__ rows, int64_t n_rows, const int64_t* __restrict__ off, int64_t total,
                       const uint32_t* __restrict__ cmap, int words, uint32_t n, int drop_zeros, int64_t* __restrict__ span_cnt) {
  extern __shared__ uint32_t s_map[];
  __shared__ int64_t s_off[kSubRows + 1];
  __shared__ int64_t s_base[kSubRows];
  __shared__ int64_t s_range[2];
  __shared__ int s_wave[kSelectThreads / 64];
  const int64_t p0 = (int64_t)blockIdx.x * kSelectSpan;
  const int64_t p1 = min(total, p0 + kSelectSpan);
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) span_cnt[gridDim.x] = 0;   // (the scan leaves the total here)
  const ColumnMap<kLds> map = column_map<kLds>(cmap, words, n, s_map);            // (walk_span's first barrier publishes it)
  int kept = 0;   // of the wave, the same in every lane
  walk_span(ptr, rows, n_rows, off, p0, p1, s_off, s_base, s_range, [&](int64_t, const int64_t (&src)[4], bool one_row) {
    const uint32_t nib = keep_flags<kLds, V>(idx, val, src, one_row, map, drop_zeros != 0);
#pragma unroll
    for (int u = 0; u < 4; ++u) kept += __popcll(__ballot((nib >> u) & 1u));
  });
  if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = kept;
  __syncthreads();
  if (threadIdx.x == 0) {
    int64_t c = 0;
    for (int w = 0; w < kSelectThreads / 64; ++w) c += s_wave[w];
    span_cnt[blockIdx.x] = c;
  }
}

// span_base: the exclusive scan of the counts (gridDim.x + 1 entries, the last the output's total)
template <typename V, bool kLds>
__global__ void __launch_bounds__(kSelectThreads)
submatrix_fill_kernel(const int64_t* __restrict__ ptr, const uint32_t* __restrict__ idx, const V* __restrict__ val,
                      const uint64_t* __restrict__ rows, int64_t n_rows, const int64_t* __restrict__ off, int64_t total,
                      const uint32_t* __restrict__ cmap, int words, uint32_t n, int drop_zeros,
                      const int64_t* __restrict__ span_base, int64_t* __restrict__ out_ptr, uint32_t* __restrict__ out_idx,
                      V* __restrict__ out_val) {
  extern __shared__ uint32_t s_map[];
  __shared__ int64_t s_off[kSubRows + 1];
  __shared__ int64_t s_base[kSubRows];
  __shared__ int64_t s_range[2];
  __shared__ uint32_t s_bits[kSubWords + 1];     // keep flag of position p0 + 32 w + b: bit b of word w; the last word stays 0
  __shared__ uint32_t s_before[kSubWords + 1];   // kept positions of the span before word w; the last: all of them
  const int64_t p0 = (int64_t)blockIdx.x * kSelectSpan;
  const int64_t p1 = min(total, p0 + kSelectSpan);
  const int64_t base = span_base[blockIdx.x];
  const ColumnMap<kLds> map = column_map<kLds>(cmap, words, n, s_map);
  for (int w = threadIdx.x; w <= kSubWords; w += kSelectThreads) s_bits[w] = 0u;
  // (walk_span's barriers order the clearing, each turn's writes and the next turn's: a word has one writer per turn)
  walk_span(ptr, rows, n_rows, off, p0, p1, s_off, s_base, s_range, [&](int64_t g, const int64_t (&src)[4], bool one_row) {
    uint32_t word = keep_flags<kLds, V>(idx, val, src, one_row, map, drop_zeros != 0) << (4 * (threadIdx.x & 7));
    word |= __shfl_xor(word, 1);
    word |= __shfl_xor(word, 2);
    word |= __shfl_xor(word, 4);
    if ((threadIdx.x & 7) == 0 && word != 0u) s_bits[(4 * g - p0) >> 5] |= word;   // (word != 0: a position below p1)
  });
  __syncthreads();
  if (threadIdx.x < 64) {   // one wave: the exclusive prefix of the words' counts, two words a lane
    const int w = 2 * threadIdx.x;
    const uint32_t a = w < kSubWords ? (uint32_t)__popc(s_bits[w]) : 0u, b = w + 1 < kSubWords ? (uint32_t)__popc(s_bits[w + 1]) : 0u;
    uint32_t incl = a + b;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t up = __shfl_up(incl, d);
      if ((int)threadIdx.x >= d) incl += up;
    }
    if (w < kSubWords) s_before[w] = incl - a - b;
    if (w + 1 < kSubWords) s_before[w + 1] = incl - b;
    if (threadIdx.x == 63) s_before[kSubWords] = incl;
  }
  __syncthreads();
  walk_span(ptr, rows, n_rows, off, p0, p1, s_off, s_base, s_range, [&](int64_t g, const int64_t (&src)[4], bool one_row) {
    const int x = (int)(4 * g - p0);
    if (x < 0 || x >= kSelectSpan) return;
    const uint32_t b = s_bits[x >> 5];
    const uint32_t group = (b >> (x & 31)) & 15u;   // the kept positions of the group; `nib`: those of this turn
    uint32_t nib = group;
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (src[u] < 0) nib &= ~(1u << u);
    if (nib == 0u) return;
    uint32_t c[4];
    V v[4];
    if (one_row) {
      Words4 w;
      __builtin_memcpy(&w, idx + src[0], sizeof(w));
#pragma unroll
      for (int u = 0; u < 4; ++u) c[u] = w.w[u];
      __builtin_memcpy(v, val + src[0], sizeof(v));
    } else {
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if ((nib >> u) & 1u) {
          c[u] = idx[src[u]];
          v[u] = val[src[u]];
        }
    }
    int64_t o = base + s_before[x >> 5] + (uint32_t)__popc(b & ((1u << (x & 31)) - 1u));
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if ((group >> u) & 1u) {
        if ((nib >> u) & 1u) {
          out_idx[o] = map.renumbered(c[u]);
          out_val[o] = v[u];
        }
        ++o;   // (a kept position of another turn still takes its place)
      }
  });
  // the offsets: every i with goff[i] in this span (the last span: and those equal to the total, out_ptr[n_rows] among them)
  const bool last = p1 == total;
  const int64_t i_lo = first_not_below(off, n_rows + 1, p0);
  const int64_t i_hi = last ? n_rows + 1 : first_not_below(off, n_rows + 1, p1);
  for (int64_t i = i_lo + threadIdx.x; i < i_hi; i += kSelectThreads) {
    const int x = (int)(off[i] - p0);   // 0 .. kSelectSpan
    out_ptr[i] = base + s_before[x >> 5] + (uint32_t)__popc(s_bits[x >> 5] & ((1u << (x & 31)) - 1u));
  }
}

}  // namespace

void select_rows_offsets(const int64_t* ptr, const uint64_t* rows, int64_t n_rows, int64_t* out_ptr, int64_t* total_host,
                         DevBuf& scratch, hipStream_t s) {
  const int64_t blocks = (n_rows + 1 + 255) / 256;
  hipLaunchKernelGGL(select_lengths_kernel, dim3((unsigned)blocks), dim3(256), 0, s, ptr, rows, n_rows, out_ptr);
  SAPCA_HIP(hipGetLastError());
  exclusive_scan_i64(out_ptr, n_rows + 1, scratch, 0, s);
  SAPCA_HIP(hipMemcpyAsync(total_host, out_ptr + n_rows, sizeof(int64_t), hipMemcpyDeviceToHost, s));
  SAPCA_HIP(hipStreamSynchronize(s));
}

template <typename T>
void select_rows_fill(const CsrView<T>& A, const uint64_t* rows, int64_t n_rows, const int64_t* out_ptr, int64_t total,
                      int32_t* out_idx, T* out_val, hipStream_t s) {
  if (total <= 0 || n_rows <= 0) return;
  using V = typename std::conditional<sizeof(T) == 4, uint32_t, uint64_t>::type;
  const int64_t blocks = (total + kSelectSpan - 1) / kSelectSpan;
  SAPCA_CHECK(blocks < ((int64_t)1 << 31), SAPCA_ERR_ARG, "select_rows: the selection is too large for one launch");
  hipLaunchKernelGGL((select_fill_kernel<V>), dim3((unsigned)blocks), dim3(kSelectThreads), 0, s, A.ptr,
                     reinterpret_cast<const uint32_t*>(A.idx), reinterpret_cast<const V*>(A.val), rows, n_rows, out_ptr, total,
                     reinterpret_cast<uint32_t*>(out_idx), reinterpret_cast<V*>(out_val));
  SAPCA_HIP(hipGetLastError());
}

template void select_rows_fill<float>(const CsrView<float>&, const uint64_t*, int64_t, const int64_t*, int64_t, int32_t*, float*,
                                      hipStream_t);
template void select_rows_fill<double>(const CsrView<double>&, const uint64_t*, int64_t, const int64_t*, int64_t, int32_t*, double*,
                                       hipStream_t);

namespace {

// kernel<V, the map in LDS> for a matrix of A.cols columns; the dynamic LDS it needs
template <typename T, typename Launch>
void with_column_map(const CsrView<T>& A, const uint32_t* cmap, Launch&& launch) {
  const int words = (int)((A.cols + 31) / 32);
  if (cmap != nullptr && words > kSubMapWords) launch(std::false_type(), words, (size_t)0);
  else launch(std::true_type(), words, cmap ? (size_t)2 * words * sizeof(uint32_t) : (size_t)0);
}

}  // namespace

int64_t select_submatrix_spans(int64_t gtotal) {
  const int64_t spans = (gtotal + kSelectSpan - 1) / kSelectSpan;
  SAPCA_CHECK(spans < ((int64_t)1 << 31), SAPCA_ERR_ARG, "select_submatrix: the selection is too large for one launch");
  return spans;
}

template <typename T>
void select_submatrix_count(const CsrView<T>& A, const uint64_t* rows, int64_t n_rows, const int64_t* goff, int64_t gtotal,
                            const uint32_t* cmap, bool drop_zeros, int64_t* span_cnt, hipStream_t s) {
  if (gtotal <= 0 || n_rows <= 0) return;
  using V = typename std::conditional<sizeof(T) == 4, uint32_t, uint64_t>::type;
  const unsigned spans = (unsigned)select_submatrix_spans(gtotal);
  with_column_map(A, cmap, [&](auto lds, int words, size_t bytes) {
    hipLaunchKernelGGL((submatrix_count_kernel<V, decltype(lds)::value>), dim3(spans), dim3(kSelectThreads), bytes, s, A.ptr,
                       reinterpret_cast<const uint32_t*>(A.idx), reinterpret_cast<const V*>(A.val), rows, n_rows, goff, gtotal, cmap,
                       words, (uint32_t)A.cols, (int)drop_zeros, span_cnt);
  });
  SAPCA_HIP(hipGetLastError());
}

template <typename T>
void select_submatrix_fill(const CsrView<T>& A, const uint64_t* rows, int64_t n_rows, const int64_t* goff, int64_t gtotal,
                           const uint32_t* cmap, bool drop_zeros, const int64_t* span_base, int64_t* out_ptr, int32_t* out_idx,
                           T* out_val, hipStream_t s) {
  if (gtotal <= 0 || n_rows <= 0) return;
  using V = typename std::conditional<sizeof(T) == 4, uint32_t, uint64_t>::type;
  const unsigned spans = (unsigned)select_submatrix_spans(gtotal);
  with_column_map(A, cmap, [&](auto lds, int words, size_t bytes) {
    hipLaunchKernelGGL((submatrix_fill_kernel<V, decltype(lds)::value>), dim3(spans), dim3(kSelectThreads), bytes, s, A.ptr,
                       reinterpret_cast<const uint32_t*>(A.idx), reinterpret_cast<const V*>(A.val), rows, n_rows, goff, gtotal, cmap,
                       words, (uint32_t)A.cols, (int)drop_zeros, span_base, out_ptr, reinterpret_cast<uint32_t*>(out_idx),
                       reinterpret_cast<V*>(out_val));
  });
  SAPCA_HIP(hipGetLastError());
}

#define SAPCA_INSTANTIATE_SUBMATRIX(T)                                                                                              \
  template void select_submatrix_count<T>(const CsrView<T>&, const uint64_t*, int64_t, const int64_t*, int64_t, const uint32_t*, bool, \
                                          int64_t*, hipStream_t);                                                                    \
  template void select_submatrix_fill<T>(const CsrView<T>&, const uint64_t*, int64_t, const int64_t*, int64_t, const uint32_t*, bool,  \
                                         const int64_t*, int64_t*, int32_t*, T*, hipStream_t);
SAPCA_INSTANTIATE_SUBMATRIX(float)
SAPCA_INSTANTIATE_SUBMATRIX(double)
#undef SAPCA_INSTANTIATE_SUBMATRIX


}  // namespace k
}  // namespace sapca
