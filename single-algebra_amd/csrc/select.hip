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

}  // namespace k
}  // namespace sapca
