// extern "C" surface of libsapca.so (include/sapca.h).  Every function: set device, try,
// translate exceptions into a status + per-handle message.  No compute lives here.
#include <algorithm>
#include <atomic>
#include <thread>
#include <chrono>
#include <cmath>
#include <cstring>
#include <new>

#include "engine.h"

using sapca::CsrView;
using sapca::Engine;
using sapca::Error;

namespace {

thread_local std::string g_create_error;

template <typename F>
sapca_status guarded(sapca_handle h, F&& f) {
  if (!h) return SAPCA_ERR_ARG;
  try {
    hipError_t e = hipSetDevice(h->device);
    if (e != hipSuccess) throw Error(SAPCA_ERR_HIP, std::string("hipSetDevice: ") + hipGetErrorString(e));
    f();
    h->err.clear();
    return SAPCA_OK;
  } catch (const Error& e) {
    h->err = e.what();
    return e.code;
  } catch (const std::bad_alloc&) {
    h->err = "out of host memory";
    return SAPCA_ERR_NOMEM;
  } catch (const std::exception& e) {
    h->err = e.what();
    return SAPCA_ERR_ARG;
  }
}

// Host CSR (nalgebra layout, usize indices) -> device CSR in the handle's upload buffers.
// PCIe is the bound of this path, so the usize column indices are narrowed to int32 on the HOST, chunk by
// chunk into a page-locked ring by a few threads, while the previous chunk's DMA (and, first, the values')
// is in flight: 8 bytes per stored entry cross the bus instead of 12.
namespace {
constexpr size_t kUpChunk = (size_t)16 << 20;   // indices per chunk (64 MiB of int32)

// out[i] = (int32) in[i]; returns true if any in[i] >= n
bool narrow_chunk(const uint64_t* in, int32_t* out, size_t count, uint64_t n, unsigned nthreads) {
  std::atomic<bool> bad{false};
  auto work = [&](size_t lo, size_t hi) {
    bool b = false;
    for (size_t i = lo; i < hi; ++i) {
      const uint64_t c = in[i];
      b |= c >= n;
      out[i] = (int32_t)c;
    }
    if (b) bad.store(true, std::memory_order_relaxed);
  };
  if (nthreads <= 1 || count < (size_t)1 << 16) {
    work(0, count);
  } else {
    std::vector<std::thread> th;
    const size_t per = (count + nthreads - 1) / nthreads;
    for (unsigned t = 1; t < nthreads; ++t) {
      const size_t lo = std::min(count, t * per), hi = std::min(count, lo + per);
      if (lo < hi) th.emplace_back(work, lo, hi);
    }
    work(0, std::min(count, per));
    for (auto& x : th) x.join();
  }
  return bad.load();
}
}  // namespace

// side stream shared by prepare() (A's format beside the transposition) and upload() (statistics beside the DMA)
void ensure_side_stream(sapca_handle h) {
  if (h->stream2) return;
  SAPCA_HIP(hipStreamCreateWithFlags(&h->stream2, hipStreamNonBlocking));
  SAPCA_HIP(hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming));
  SAPCA_HIP(hipEventCreateWithFlags(&h->ev_join, hipEventDisableTiming));
}

// with_stats: the matrix is about to be fitted -- accumulate its column statistics (R1/R2 and the per-column counts)
// on the side stream, chunk by chunk behind the DMA, so prepare() finds them ready
template <typename T>
CsrView<T> upload(sapca_handle h, uint64_t m, uint64_t n, uint64_t nnz, const uint64_t* row_offsets,
                  const uint64_t* col_indices, const T* values, bool with_stats = false) {
  SAPCA_CHECK(row_offsets != nullptr && (nnz == 0 || (col_indices && values)), SAPCA_ERR_ARG, "null CSR array");
  SAPCA_CHECK(row_offsets[0] == 0 && row_offsets[m] == nnz, SAPCA_ERR_ARG, "row_offsets do not span [0, nnz]");
  {   // with monotone offsets and in-range columns (checked below) no kernel can leave the arrays
    bool monotone = true;
    for (uint64_t i = 0; i < m; ++i) monotone &= row_offsets[i] <= row_offsets[i + 1];
    SAPCA_CHECK(monotone, SAPCA_ERR_ARG, "row_offsets must be non-decreasing");
  }
  SAPCA_CHECK(n < (1ull << 31) && m < (1ull << 31), SAPCA_ERR_ARG, "more than 2^31-1 rows or columns is not supported");
  hipStream_t s = h->stream;
  h->prep_key.valid = false;  // the upload buffers are about to hold a different matrix
  h->up_stats.valid = false;
  auto t0 = std::chrono::steady_clock::now();
  int64_t* d_ptr = h->in_ptr.as<int64_t>(m + 1);
  int32_t* d_idx = h->in_idx.as<int32_t>(std::max<uint64_t>(nnz, 1));
  T* d_val = h->in_val.as<T>(std::max<uint64_t>(nnz, 1));
  uint64_t* d64 = h->up64.as<uint64_t>(m + 1 + 8);
  int* flag = reinterpret_cast<int*>(d64 + m + 1);
  SAPCA_HIP(hipMemsetAsync(flag, 0, sizeof(int), s));
  SAPCA_HIP(hipMemcpyAsync(d64, row_offsets, (m + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, s));
  bool bad_host = false, stats_here = false;
  void* stats_work = nullptr;
  sapca::k::narrow_indices(d64, d64, (int64_t)m, 0, (int64_t)n, d_ptr, d_idx, flag, s);   // row offsets only
  if (nnz) {
    SAPCA_HIP(hipMemcpyAsync(d_val, values, nnz * sizeof(T), hipMemcpyHostToDevice, s));
    const unsigned nthreads = std::max(1u, std::min(8u, std::thread::hardware_concurrency()));
    const size_t chunk = std::min<size_t>(kUpChunk, nnz);
    for (int b = 0; b < 2; ++b) {
      h->up_stage[b].ensure(chunk * sizeof(int32_t));
      if (!h->up_done[b]) SAPCA_HIP(hipEventCreateWithFlags(&h->up_done[b], hipEventDisableTiming));
    }
    static const bool stats_off = sapca::dbg_env("SAPCA_UPLOAD_STATS_OFF") != nullptr;
    stats_here = with_stats && !stats_off && n > 0 && sapca::k::exact_colstats_bytes<T>((int64_t)n) <= ((size_t)1 << 30);
    if (stats_here) {
      ensure_side_stream(h);
      stats_work = h->up_stats.work.ensure(sapca::k::exact_colstats_bytes<T>((int64_t)n));
      sapca::k::exact_colstats_reset<T>(stats_work, (int64_t)n, h->stream2);
      SAPCA_HIP(hipEventRecord(h->ev_fork, s));                        // row offsets and values are on the device
      SAPCA_HIP(hipStreamWaitEvent(h->stream2, h->ev_fork, 0));
      sapca::k::exact_colstats_scan_values<T>(d_val, (int64_t)nnz, (int64_t)n, stats_work, h->stream2);
    }
    bool used[2] = {false, false};
    int b = 0;
    for (size_t off = 0; off < nnz; off += chunk, b ^= 1) {
      const size_t cnt = std::min<size_t>(chunk, nnz - off);
      if (used[b]) SAPCA_HIP(hipEventSynchronize(h->up_done[b]));   // its DMA has drained
      int32_t* stage = static_cast<int32_t*>(h->up_stage[b].p);
      bad_host |= narrow_chunk(col_indices + off, stage, cnt, n, nthreads);
      SAPCA_HIP(hipMemcpyAsync(d_idx + off, stage, cnt * sizeof(int32_t), hipMemcpyHostToDevice, s));
      SAPCA_HIP(hipEventRecord(h->up_done[b], s));
      used[b] = true;
      if (stats_here) {   // this chunk's entries (the values all went first) feed the accumulators while the next chunk crosses
        SAPCA_HIP(hipStreamWaitEvent(h->stream2, h->up_done[b], 0));
        const uint64_t* ro_end = row_offsets + m + 1;
        const int64_t r_lo = (int64_t)(std::upper_bound(row_offsets, ro_end, (uint64_t)off) - row_offsets) - 1;
        const int64_t r_hi = (int64_t)(std::lower_bound(row_offsets, ro_end, (uint64_t)(off + cnt)) - row_offsets);
        sapca::k::exact_colstats_add<T>(d_ptr, d_idx, d_val, r_lo, std::min<int64_t>(r_hi, (int64_t)m), (int64_t)off,
                                        (int64_t)(off + cnt), (int64_t)n, stats_work, h->stream2);
      }
    }
  }
  int bad = 0;
  if (stats_here) {
    // the last chunk's share and the final rounding stay in flight behind this call: their consumer (prepare(), the column
    // statistics helper) waits for `up_stats_done` and reads the "a value was inf/nan" flag then
    double* out = h->up_stats.out.as<double>(3 * n);
    int* nonfinite = static_cast<int*>(h->up_stats.flag.ensure(sizeof(int)));
    sapca::k::exact_colstats_finish<T>(stats_work, (int64_t)n, out, nonfinite, h->stream2);
    if (!h->up_stats_done) SAPCA_HIP(hipEventCreateWithFlags(&h->up_stats_done, hipEventDisableTiming));
    SAPCA_HIP(hipEventRecord(h->up_stats_done, h->stream2));
  }
  SAPCA_HIP(hipMemcpyAsync(&bad, flag, sizeof(int), hipMemcpyDeviceToHost, s));
  SAPCA_HIP(hipStreamSynchronize(s));
  SAPCA_CHECK(bad == 0 && !bad_host, SAPCA_ERR_ARG, "column index out of range");
  if (stats_here) {
    h->up_stats.m = m; h->up_stats.n = n; h->up_stats.nnz = nnz; h->up_stats.dtype = sizeof(T) == 4 ? 0 : 1;
    h->up_stats.valid = true;
  }
  h->timings.upload_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  CsrView<T> v;
  v.rows = (int64_t)m; v.cols = (int64_t)n; v.nnz = (int64_t)nnz;
  v.ptr = d_ptr; v.idx = d_idx; v.val = d_val;
  return v;
}

template <typename T>
CsrView<T> device_view(uint64_t m, uint64_t n, uint64_t nnz, const int64_t* p, const int32_t* i, const T* v) {
  SAPCA_CHECK(p != nullptr && (nnz == 0 || (i && v)), SAPCA_ERR_ARG, "null CSR array");
  SAPCA_CHECK(n < (1ull << 31) && m < (1ull << 31), SAPCA_ERR_ARG, "more than 2^31-1 rows or columns is not supported");
  CsrView<T> a;
  a.rows = (int64_t)m; a.cols = (int64_t)n; a.nnz = (int64_t)nnz; a.ptr = p; a.idx = i; a.val = v;
  return a;
}

// dst <- src on a few host threads (a pageable destination at DRAM speed instead of one core's)
void parallel_copy(void* dst, const void* src, size_t bytes, unsigned nthreads) {
  if (nthreads <= 1 || bytes < ((size_t)1 << 20)) {
    std::memcpy(dst, src, bytes);
    return;
  }
  std::vector<std::thread> th;
  const size_t per = ((bytes + nthreads - 1) / nthreads + 63) & ~(size_t)63;
  for (unsigned t = 1; t < nthreads; ++t) {
    const size_t lo = std::min(bytes, t * per), hi = std::min(bytes, lo + per);
    if (lo < hi) th.emplace_back([=] { std::memcpy(static_cast<char*>(dst) + lo, static_cast<const char*>(src) + lo, hi - lo); });
  }
  std::memcpy(dst, src, std::min(bytes, per));
  for (auto& x : th) x.join();
}

// Device -> caller's (pageable) host array.  A direct copy to pageable memory runs at about 10 GB/s; results of more than a
// few MB (the m x k projection) go through the page-locked ring of the upload instead: DMA into one half while a few
// threads copy the other half out.
template <typename T>
void download_out(sapca_handle h, const T* d, T* out, size_t count) {
  hipStream_t s = h->stream;
  const size_t bytes = count * sizeof(T);
  constexpr size_t kPiece = (size_t)8 << 20;
  if (bytes < 2 * kPiece) {
    SAPCA_HIP(hipMemcpyAsync(out, d, bytes, hipMemcpyDeviceToHost, s));
    SAPCA_HIP(hipStreamSynchronize(s));
    return;
  }
  const unsigned nthreads = std::max(1u, std::min(8u, std::thread::hardware_concurrency()));
  for (int b = 0; b < 2; ++b) {
    h->up_stage[b].ensure(kPiece);
    if (!h->up_done[b]) SAPCA_HIP(hipEventCreateWithFlags(&h->up_done[b], hipEventDisableTiming));
  }
  const char* src = reinterpret_cast<const char*>(d);
  char* dst = reinterpret_cast<char*>(out);
  size_t pending_off[2] = {0, 0}, pending_len[2] = {0, 0};
  int b = 0;
  for (size_t off = 0; off < bytes; off += kPiece, b ^= 1) {
    if (pending_len[b]) {   // the piece that used this half: drained, copy it out
      SAPCA_HIP(hipEventSynchronize(h->up_done[b]));
      parallel_copy(dst + pending_off[b], h->up_stage[b].p, pending_len[b], nthreads);
    }
    const size_t len = std::min(kPiece, bytes - off);
    SAPCA_HIP(hipMemcpyAsync(h->up_stage[b].p, src + off, len, hipMemcpyDeviceToHost, s));
    SAPCA_HIP(hipEventRecord(h->up_done[b], s));
    pending_off[b] = off;
    pending_len[b] = len;
  }
  for (int i = 0; i < 2; ++i, b ^= 1)   // oldest first
    if (pending_len[b]) {
      SAPCA_HIP(hipEventSynchronize(h->up_done[b]));
      parallel_copy(dst + pending_off[b], h->up_stage[b].p, pending_len[b], nthreads);
      pending_len[b] = 0;
    }
  SAPCA_HIP(hipStreamSynchronize(s));
}

template <typename T>
sapca_status fit_host(sapca_handle h, uint64_t m, uint64_t n, uint64_t nnz, const uint64_t* ro, const uint64_t* ci,
                      const T* v) {
  return guarded(h, [&] { Engine<T>::fit(*h, upload<T>(h, m, n, nnz, ro, ci, v, true)); });
}

template <typename T>
sapca_status transform_host(sapca_handle h, uint64_t m, uint64_t n, uint64_t nnz, const uint64_t* ro,
                            const uint64_t* ci, const T* v, T* out, bool fit_first) {
  return guarded(h, [&] {
    SAPCA_CHECK(out != nullptr || m == 0, SAPCA_ERR_ARG, "null output buffer");
    if (!fit_first) {
      if (!h->mask.empty() && h->mask.size() != n)
        throw Error(SAPCA_ERR_MASK_LEN, "The mask vector length and the number of features (columns) have to be the same!");
      if (!h->fitted) throw Error(SAPCA_ERR_NOT_FITTED, "Must be fitted before transform!");
    }
    CsrView<T> A = upload<T>(h, m, n, nnz, ro, ci, v, fit_first);
    if (fit_first) Engine<T>::fit(*h, A, true);   // (its host-side tail runs once the projection is queued)
    try {
      T* d_out = h->out_tmp.as<T>(std::max<uint64_t>(m * h->k, 1));
      Engine<T>::transform(*h, A, d_out);
      download_out(h, d_out, out, (size_t)(m * h->k));
    } catch (...) {
      Engine<T>::finish_fit(*h);
      throw;
    }
  });
}

template <typename T>
sapca_status fit_device(sapca_handle h, uint64_t m, uint64_t n, uint64_t nnz, const int64_t* p, const int32_t* i,
                        const T* v) {
  return guarded(h, [&] { Engine<T>::fit(*h, device_view<T>(m, n, nnz, p, i, v)); });
}

template <typename T>
sapca_status transform_device(sapca_handle h, uint64_t m, uint64_t n, uint64_t nnz, const int64_t* p,
                              const int32_t* i, const T* v, T* d_out, bool fit_first, bool out_on_host = false) {
  return guarded(h, [&] {
    SAPCA_CHECK(d_out != nullptr || m == 0, SAPCA_ERR_ARG, "null output buffer");
    CsrView<T> A = device_view<T>(m, n, nnz, p, i, v);
    T* host_out = out_on_host ? d_out : nullptr;
    // (the staging holds what transform() writes and download_out() copies: m x k of the model that projects -- the one
    // being fitted here has at most n_components, a fitted one has h->k)
    if (out_on_host) d_out = h->out_tmp.as<T>(std::max<uint64_t>(m * std::max<uint64_t>(h->opt.n_components, fit_first ? 0 : h->k), 1));
    if (fit_first) {
      Engine<T>::fit(*h, A, true);
    } else if (static_cast<const void*>(v) != h->in_val.p) {
      // A separate transform call on caller-owned device arrays: pointer identity does not prove the matrix is the fitted
      // one (values edited in place, an allocator handing the same addresses to another matrix), so the preparation kept
      // from fit() -- tile-major copy of the values, per-column counts -- is not reused.  It is reused inside
      // fit_transform (one call, the matrix is borrowed unmodified) and for the library-owned arrays of sapca_upload_csr_*,
      // which only the library's own entry points modify (each of them drops the preparation).
      h->prep_key.valid = false;
    }
    try {
      Engine<T>::transform(*h, A, d_out);
      if (host_out) download_out(h, d_out, host_out, (size_t)(m * h->k));
    } catch (...) {
      Engine<T>::finish_fit(*h);   // (a fit whose tail was held back for the projection still completes)
      throw;
    }
  });
}

template <typename T>
void copy_out(const std::vector<double>& src, T* out, size_t cap) {
  SAPCA_CHECK(out != nullptr && cap >= src.size(), SAPCA_ERR_ARG, "output buffer too small");
  for (size_t i = 0; i < src.size(); ++i) out[i] = (T)src[i];
}

void need_fitted(sapca_handle h) {
  if (!h->fitted) throw Error(SAPCA_ERR_NOT_FITTED, "Model must be fitted first!");  // sparse/mod.rs:299,316
}

// components live on the device in the fitted dtype; fetched (and converted) on demand
template <typename T>
void get_components(sapca_handle h, T* out, size_t cap, bool squared) {
  need_fitted(h);
  const size_t count = (size_t)(h->k * h->n_used);
  SAPCA_CHECK(out != nullptr && cap >= count, SAPCA_ERR_ARG, "output buffer too small");
  if (h->dtype == 0) {
    std::vector<float> tmp(count);
    download_out(h, h->components_dev.ptr<float>(), tmp.data(), count);
    for (size_t i = 0; i < count; ++i) out[i] = squared ? (T)(tmp[i] * tmp[i]) : (T)tmp[i];
  } else {
    std::vector<double> tmp(count);
    download_out(h, h->components_dev.ptr<double>(), tmp.data(), count);
    for (size_t i = 0; i < count; ++i) out[i] = squared ? (T)(tmp[i] * tmp[i]) : (T)tmp[i];
  }
}

template <typename T>
void get_ratio(sapca_handle h, T* out, size_t cap, bool cumulative) {
  need_fitted(h);
  SAPCA_CHECK(out != nullptr && cap >= h->k, SAPCA_ERR_ARG, "output buffer too small");
  // sparse/mod.rs:318-319: ratio_i = ev_i / sum over the k computed components, in T
  T total = 0;
  for (uint64_t i = 0; i < h->k; ++i) total += (T)h->expl_var[i];
  T run = 0;
  for (uint64_t i = 0; i < h->k; ++i) {
    const T r = (T)h->expl_var[i] / total;
    run += r;  // sparse/mod.rs:336-340
    out[i] = cumulative ? run : r;
  }
}

// stage-level helpers -------------------------------------------------------------------
template <typename T>
sapca_status colstats_host(sapca_handle h, uint64_t m, uint64_t n, uint64_t nnz, const uint64_t* ro,
                           const uint64_t* ci, const T* v, T* sum_col, T* sum_sq, uint64_t* cnt) {
  return guarded(h, [&] {
    CsrView<T> A = upload<T>(h, m, n, nnz, ro, ci, v, true);
    hipStream_t s = h->stream;
    std::vector<double> host(3 * n);
    if (h->up_stats.valid) SAPCA_HIP(hipEventSynchronize(h->up_stats_done));
    if (h->up_stats.valid && *static_cast<const int*>(h->up_stats.flag.p) == 0) {   // gathered behind the DMA (exact sums, rounded once)
      download_out(h, h->up_stats.out.ptr<double>(), host.data(), 3 * n);
    } else {                   // row sums of A^T: what prepare() runs on device-resident input
      int64_t* at_ptr = h->at_ptr.as<int64_t>(n + 1);
      int32_t* at_idx = h->at_idx.as<int32_t>(std::max<uint64_t>(nnz, 1));
      T* at_val = h->at_val.as<T>(std::max<uint64_t>(nnz, 1));
      sapca::k::transpose_csr(A, at_ptr, at_idx, at_val, h->scratch, s);
      CsrView<T> At;
      At.rows = (int64_t)n; At.cols = (int64_t)m; At.nnz = (int64_t)nnz; At.ptr = at_ptr; At.idx = at_idx; At.val = at_val;
      double* d = h->stats.as<double>(3 * n + 1);
      sapca::k::row_sums(At, d, d + n, s);
      sapca::k::row_lengths_f64(at_ptr, (int64_t)n, d + 2 * n, s);
      download_out(h, d, host.data(), 3 * n);
    }
    for (uint64_t j = 0; j < n; ++j) {
      if (sum_col) sum_col[j] = (T)host[j];
      if (sum_sq) sum_sq[j] = (T)host[n + j];
      if (cnt) cnt[j] = (uint64_t)host[2 * n + j];
    }
  });
}

// ---- device-resident workflow: upload once, preprocess and analyse in HBM -------------
template <typename T>
sapca_status upload_host(sapca_handle h, uint64_t m, uint64_t n, uint64_t nnz, const uint64_t* ro, const uint64_t* ci,
                         const T* v, const int64_t** d_ptr, const int32_t** d_idx, T** d_val) {
  return guarded(h, [&] {
    SAPCA_CHECK(d_ptr && d_idx && d_val, SAPCA_ERR_ARG, "null output pointer");
    CsrView<T> A = upload<T>(h, m, n, nnz, ro, ci, v, true);   // (a later fit of the untouched arrays finds its statistics ready)
    *d_ptr = A.ptr;
    *d_idx = A.idx;
    *d_val = const_cast<T*>(A.val);
  });
}

template <typename T>
sapca_status normalize_device(sapca_handle h, uint64_t m, uint64_t n, uint64_t nnz, const int64_t* p, const int32_t* i, T* v,
                              const double* sums, uint64_t sums_len, double target, int32_t direction) {
  return guarded(h, [&] {
    SAPCA_CHECK(direction == 0 || direction == 1, SAPCA_ERR_ARG, "direction must be 0 (ROW) or 1 (COLUMN)");
    const uint64_t want = direction == 1 ? n : m;
    SAPCA_CHECK(sums != nullptr || want == 0, SAPCA_ERR_ARG, "null sums");
    SAPCA_CHECK(sums_len == want, SAPCA_ERR_ARG,
                direction == 1 ? "Length of sums must match number of columns" : "Length of sums must match number of rows");
    CsrView<T> A = device_view<T>(m, n, nnz, p, i, v);
    if (want == 0 || nnz == 0) return;
    h->prep_key.valid = false;   // the values change under any cached preparation
    h->up_stats.valid = false;   // .. and under the statistics gathered at upload
    double* d = h->stats.as<double>(2 * want);
    SAPCA_HIP(hipMemcpyAsync(d, sums, want * sizeof(double), hipMemcpyHostToDevice, h->stream));
    sapca::k::normalize_csr(A, v, d, target, direction == 1, d + want, h->stream);
    SAPCA_HIP(hipStreamSynchronize(h->stream));   // `sums` may go out of scope
  });
}

template <typename T>
sapca_status log1p_device(sapca_handle h, uint64_t nnz, T* v) {
  return guarded(h, [&] {
    SAPCA_CHECK(v != nullptr || nnz == 0, SAPCA_ERR_ARG, "null values");
    h->prep_key.valid = false;
    h->up_stats.valid = false;
    sapca::k::log1p_values(v, (int64_t)nnz, h->stream);
    SAPCA_HIP(hipStreamSynchronize(h->stream));
  });
}

// direction 0: per row (sum_row, sum_row_squared, nonzero_row, min_max_row); 1: per column (the same on A^T)
template <typename T>
sapca_status stats_device(sapca_handle h, uint64_t m, uint64_t n, uint64_t nnz, const int64_t* p, const int32_t* i, const T* v,
                          int32_t direction, double* sum, double* sumsq, uint64_t* nonzero, T* minv, T* maxv) {
  return guarded(h, [&] {
    SAPCA_CHECK(direction == 0 || direction == 1, SAPCA_ERR_ARG, "direction must be 0 (ROW) or 1 (COLUMN)");
    CsrView<T> A = device_view<T>(m, n, nnz, p, i, v);
    hipStream_t s = h->stream;
    const uint64_t len = direction == 1 ? n : m;
    if (len == 0) return;
    h->prep_key.valid = false;   // the statistics and transposition buffers are shared with prepare()
    CsrView<T> R = A;
    if (direction == 1) {
      // (the transposition buffers are shared with prepare())
      int64_t* at_ptr = h->at_ptr.as<int64_t>(n + 1);
      int32_t* at_idx = h->at_idx.as<int32_t>(std::max<uint64_t>(nnz, 1));
      T* at_val = h->at_val.as<T>(std::max<uint64_t>(nnz, 1));
      sapca::k::transpose_csr(A, at_ptr, at_idx, at_val, h->scratch, s);
      R.rows = (int64_t)n; R.cols = (int64_t)m; R.ptr = at_ptr; R.idx = at_idx; R.val = at_val;
    }
    double* d = h->stats.as<double>(3 * len + 1);
    T* dmm = h->out_tmp.as<T>(2 * len);
    sapca::k::row_stats(R, d, d + len, dmm, dmm + len, s);
    sapca::k::row_lengths_f64(R.ptr, (int64_t)len, d + 2 * len, s);
    std::vector<double> host(3 * len);
    std::vector<T> mm(2 * len);
    SAPCA_HIP(hipMemcpyAsync(host.data(), d, host.size() * sizeof(double), hipMemcpyDeviceToHost, s));
    SAPCA_HIP(hipMemcpyAsync(mm.data(), dmm, mm.size() * sizeof(T), hipMemcpyDeviceToHost, s));
    SAPCA_HIP(hipStreamSynchronize(s));
    for (uint64_t j = 0; j < len; ++j) {
      if (sum) sum[j] = host[j];
      if (sumsq) sumsq[j] = host[len + j];
      if (nonzero) nonzero[j] = (uint64_t)host[2 * len + j];
      if (minv) minv[j] = mm[j];
      if (maxv) maxv[j] = mm[len + j];
    }
  });
}

// BatchMatrixVariance / BatchMatrixMean (csr.rs:1081-1344) through one pass pair per code range.  grouped_axis 0: codes
// label the rows of A (length m), results per column, computed on the rows of A^T; 1: codes label the columns (length n),
// results per row of A.  The host counts the group sizes (the denominators of the means) and finishes mean / var.
template <typename T>
sapca_status batch_stats_device(sapca_handle h, uint64_t m, uint64_t n, uint64_t nnz, const int64_t* p, const int32_t* i, const T* v,
                                int32_t grouped_axis, const int32_t* codes, uint64_t codes_len, uint32_t n_batches, double* mean,
                                double* var, uint64_t* count) {
  return guarded(h, [&] {
    SAPCA_CHECK(grouped_axis == 0 || grouped_axis == 1, SAPCA_ERR_ARG, "grouped_axis must be 0 (codes label rows) or 1 (columns)");
    CsrView<T> A = device_view<T>(m, n, nnz, p, i, v);
    const uint64_t want = grouped_axis == 0 ? m : n, len = grouped_axis == 0 ? n : m;
    if (codes_len != want) {   // the message of the reference method this call serves (var_* when var is asked for)
      const std::string got = std::to_string(codes_len), have = std::to_string(want);
      if (var)
        throw Error(SAPCA_ERR_ARG, "Batch vector length (" + got + ") doesn't match matrix " + (grouped_axis == 0 ? "row" : "column") +
                                       " count (" + have + ")");
      throw Error(SAPCA_ERR_ARG, "Number of batch identifiers (" + got + ") must match number of " +
                                     (grouped_axis == 0 ? "rows" : "columns") + " (" + have + ")");
    }
    SAPCA_CHECK(codes != nullptr || codes_len == 0, SAPCA_ERR_ARG, "null codes");
    std::vector<uint64_t> group(n_batches, 0);
    for (uint64_t j = 0; j < codes_len; ++j) {
      SAPCA_CHECK(codes[j] >= 0 && (uint32_t)codes[j] < n_batches, SAPCA_ERR_ARG,
                  "batch code " + std::to_string(codes[j]) + " at " + std::to_string(j) + " is outside [0, n_batches)");
      ++group[codes[j]];
    }
    if (n_batches == 0 || len == 0) return;
    hipStream_t s = h->stream;
    int32_t* d_codes = h->batch_in.as<int32_t>(std::max<uint64_t>(codes_len, 1));
    if (codes_len) SAPCA_HIP(hipMemcpyAsync(d_codes, codes, codes_len * sizeof(int32_t), hipMemcpyHostToDevice, s));
    CsrView<T> R = A;
    if (grouped_axis == 0) {
      h->prep_key.valid = false;   // the transposition buffers are shared with prepare()
      int64_t* at_ptr = h->at_ptr.as<int64_t>(n + 1);
      int32_t* at_idx = h->at_idx.as<int32_t>(std::max<uint64_t>(nnz, 1));
      T* at_val = h->at_val.as<T>(std::max<uint64_t>(nnz, 1));
      sapca::k::transpose_csr(A, at_ptr, at_idx, at_val, h->scratch, s);
      R.rows = (int64_t)n; R.cols = (int64_t)m; R.ptr = at_ptr; R.idx = at_idx; R.val = at_val;
    }
    const int per = sapca::k::batch_codes_per_launch();
    const int nb_max = (int)std::min<uint32_t>(n_batches, (uint32_t)per);
    double* d_sum = h->batch_out.as<double>((size_t)nb_max * len * 5 / 2 + 1);   // sum, m2 (f64) and count (u32) per slot
    double* d_m2 = d_sum + (size_t)nb_max * len;
    uint32_t* d_cnt = reinterpret_cast<uint32_t*>(d_m2 + (size_t)nb_max * len);
    std::vector<double> hs, hm;
    std::vector<uint32_t> hc;
    for (uint32_t lo = 0; lo < n_batches; lo += (uint32_t)per) {
      const int nb = (int)std::min<uint32_t>(n_batches - lo, (uint32_t)per);
      const size_t cells = (size_t)nb * len;
      sapca::k::batch_row_stats(R, d_codes, (int)lo, nb, d_sum, d_m2, d_cnt, s);
      hs.resize(cells); hm.resize(cells); hc.resize(cells);
      SAPCA_HIP(hipMemcpyAsync(hs.data(), d_sum, cells * sizeof(double), hipMemcpyDeviceToHost, s));
      SAPCA_HIP(hipMemcpyAsync(hm.data(), d_m2, cells * sizeof(double), hipMemcpyDeviceToHost, s));
      SAPCA_HIP(hipMemcpyAsync(hc.data(), d_cnt, cells * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
      SAPCA_HIP(hipStreamSynchronize(s));
      for (int b = 0; b < nb; ++b) {
        const uint64_t g = group[lo + b];
        const size_t base = ((size_t)lo + b) * len;
        for (uint64_t r = 0; r < len; ++r) {
          const size_t c = (size_t)b * len + r;
          if (mean) mean[base + r] = g ? hs[c] / (double)g : 0.0;                        // csr.rs:1290-1293, 1337-1340
          if (var) var[base + r] = hc[c] > 1 ? hm[c] / (double)(hc[c] - 1) : 0.0;       // csr.rs:1151-1160
          if (count) count[base + r] = hc[c];
        }
      }
    }
  });
}

// MatrixNonZero / MatrixSum / MatrixVariance *_masked (csr.rs:153-252, 418-556, 815-914) and the stored-entry variance of
// var_*_chunk (csr.rs:728-813, mask == nullptr).  direction 0 (ROW): per row of A, `mask` over the columns (two passes in
// the wave of a row, maskedstats.hip); 1 (COLUMN): per column, `mask` over the rows, in the exact long accumulators of
// upstats.hip without a transposition (rows whose bit is clear are not read).  A kept inf / nan raises their flag; the
// columns it touched then take the ROW kernel's f64 sums on A^T, so it propagates as an f64 sum does.  So does a
// matrix too wide for the accumulators' 1 GiB.  The host finishes the variance: Σ(x − mean)² / count (ROW) or
// sumsq / count − mean² (COLUMN), 0 where count is 0.
template <typename T>
sapca_status masked_stats_device(sapca_handle h, uint64_t m, uint64_t n, uint64_t nnz, const int64_t* p, const int32_t* i, const T* v,
                                 int32_t direction, const uint8_t* mask, uint64_t mask_len, double* sum, double* sumsq,
                                 uint64_t* count, double* var) {
  return guarded(h, [&] {
    SAPCA_CHECK(direction == 0 || direction == 1, SAPCA_ERR_ARG, "direction must be 0 (ROW) or 1 (COLUMN)");
    CsrView<T> A = device_view<T>(m, n, nnz, p, i, v);
    const uint64_t masked = direction == 1 ? m : n, len = direction == 1 ? n : m;
    if (mask != nullptr && mask_len < masked)   // the reference's message; a longer mask's tail is ignored
      throw Error(SAPCA_ERR_ARG, "Mask length (" + std::to_string(mask_len) + ") is less than number of " +
                                     (direction == 1 ? "rows" : "columns") + " (" + std::to_string(masked) + ")");
    if (len == 0) return;
    hipStream_t s = h->stream;
    const uint64_t words = (masked + 31) / 32;
    uint32_t* d_bits = nullptr;
    std::vector<uint32_t> bits;   // (lives until the results are on the host: its copy is asynchronous)
    if (mask != nullptr) {        // (no mask: no bitset, and the kernels read no mask)
      bits.assign(std::max<uint64_t>(words, 1), 0u);
      for (uint64_t j = 0; j < masked; ++j)
        if (mask[j]) bits[j >> 5] |= 1u << (j & 31);
      d_bits = h->batch_in.as<uint32_t>(bits.size());
      SAPCA_HIP(hipMemcpyAsync(d_bits, bits.data(), bits.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    }
    std::vector<double> hs(len), hq(len), hm2;
    std::vector<uint32_t> hc(len);
    // the ROW kernel on R (A, or A^T for the column direction) into hs / hq / hm2 / hc
    auto row_pass = [&](const CsrView<T>& R) {
      double* d = h->batch_out.as<double>(3 * len + (len + 1) / 2);
      uint32_t* dc = reinterpret_cast<uint32_t*>(d + 3 * len);
      sapca::k::masked_row_stats(R, d_bits, d, d + len, d + 2 * len, dc, s);
      hm2.resize(len);
      SAPCA_HIP(hipMemcpyAsync(hs.data(), d, len * sizeof(double), hipMemcpyDeviceToHost, s));
      SAPCA_HIP(hipMemcpyAsync(hq.data(), d + len, len * sizeof(double), hipMemcpyDeviceToHost, s));
      SAPCA_HIP(hipMemcpyAsync(hm2.data(), d + 2 * len, len * sizeof(double), hipMemcpyDeviceToHost, s));
      SAPCA_HIP(hipMemcpyAsync(hc.data(), dc, len * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
      SAPCA_HIP(hipStreamSynchronize(s));
    };
    auto transposed = [&] {
      h->prep_key.valid = false;   // the transposition buffers are shared with prepare()
      int64_t* at_ptr = h->at_ptr.as<int64_t>(n + 1);
      int32_t* at_idx = h->at_idx.as<int32_t>(std::max<uint64_t>(nnz, 1));
      T* at_val = h->at_val.as<T>(std::max<uint64_t>(nnz, 1));
      sapca::k::transpose_csr(A, at_ptr, at_idx, at_val, h->scratch, s);
      CsrView<T> R = A;
      R.rows = (int64_t)n; R.cols = (int64_t)m; R.ptr = at_ptr; R.idx = at_idx; R.val = at_val;
      return R;
    };
    if (direction == 0) {
      row_pass(A);
    } else if (sapca::k::exact_colstats_bytes<T>((int64_t)n) > ((size_t)1 << 30)) {
      row_pass(transposed());
    } else {
      const size_t work_bytes = (sapca::k::exact_colstats_bytes<T>((int64_t)n) + 255) / 256 * 256;
      char* base = h->batch_out.as<char>(work_bytes + 3 * n * sizeof(double));
      double* d_out = reinterpret_cast<double*>(base + work_bytes);
      sapca::k::exact_colstats_reset<T>(base, (int64_t)n, s);
      if (d_bits) sapca::k::exact_colstats_scan_rows<T>(A.ptr, A.val, (int64_t)m, d_bits, (int64_t)n, base, s);
      else sapca::k::exact_colstats_scan_values<T>(A.val, (int64_t)nnz, (int64_t)n, base, s);
      sapca::k::exact_colstats_add<T>(A.ptr, A.idx, A.val, 0, (int64_t)m, 0, (int64_t)nnz, (int64_t)n, base, s, d_bits);
      int nonfinite = 0;
      sapca::k::exact_colstats_finish<T>(base, (int64_t)n, d_out, &nonfinite, s);
      std::vector<double> host(3 * n);
      SAPCA_HIP(hipMemcpyAsync(host.data(), d_out, host.size() * sizeof(double), hipMemcpyDeviceToHost, s));
      SAPCA_HIP(hipStreamSynchronize(s));
      for (uint64_t j = 0; j < n; ++j) {
        hs[j] = host[j];
        hq[j] = host[n + j];
        hc[j] = (uint32_t)host[2 * n + j];
      }
      if (nonfinite) {   // the columns whose kept entries hold an inf / nan take the f64 sums of the row pass on A^T
        const std::vector<double> es = hs, eq = hq;
        row_pass(transposed());
        for (uint64_t j = 0; j < n; ++j)
          if (std::isfinite(hs[j])) {
            hs[j] = es[j];
            hq[j] = eq[j];
          }
      }
    }
    for (uint64_t r = 0; r < len; ++r) {
      const double c = (double)hc[r];
      if (sum) sum[r] = hs[r];
      if (sumsq) sumsq[r] = hq[r];
      if (count) count[r] = hc[r];
      if (var) {
        if (hc[r] == 0) var[r] = 0.0;
        else if (direction == 0) var[r] = hm2[r] / c;                        // csr.rs:889-911
        else var[r] = hq[r] / c - (hs[r] / c) * (hs[r] / c);               // csr.rs:852-859
      }
    }
  });
}

// Rows `rows[0 .. n_rows)` of a device CSR (any order, repeats allowed) as a CSR in the handle's selection buffers: the
// offsets through a scan (one synchronisation: the total sizes the output), then a fill balanced over output entries
// (select.hip).  Everything that can be refused is refused before anything is enqueued or a buffer is touched.
template <typename T>
sapca_status select_rows_device(sapca_handle h, uint64_t m, uint64_t n, uint64_t nnz, const int64_t* p, const int32_t* i, const T* v,
                                const uint64_t* rows, uint64_t n_rows, uint64_t* nnz_out, const int64_t** d_ptr,
                                const int32_t** d_idx, T** d_val) {
  return guarded(h, [&] {
    SAPCA_CHECK(nnz_out && d_ptr && d_idx && d_val, SAPCA_ERR_ARG, "select_rows: null output pointer");
    SAPCA_CHECK(rows != nullptr || n_rows == 0, SAPCA_ERR_ARG, "select_rows: rows is NULL with n_rows > 0");
    CsrView<T> A = device_view<T>(m, n, nnz, p, i, v);
    SAPCA_CHECK(n_rows < (1ull << 31), SAPCA_ERR_ARG, "more than 2^31-1 rows or columns is not supported");
    auto inside = [](const void* q, const sapca::DevBuf& b) {
      const char* c = static_cast<const char*>(q);
      return b.p != nullptr && c >= static_cast<const char*>(b.p) && c < static_cast<const char*>(b.p) + b.cap;
    };
    SAPCA_CHECK(!inside(p, h->sub_ptr) && !inside(i, h->sub_idx) && !inside(v, h->sub_val), SAPCA_ERR_ARG,
                "select_rows: the source is this handle's own selection, which the call overwrites (select from the uploaded matrix)");
    for (uint64_t j = 0; j < n_rows; ++j)
      if (rows[j] >= m)
        throw Error(SAPCA_ERR_ARG, "select_rows: row index " + std::to_string(rows[j]) + " at position " + std::to_string(j) +
                                       " is out of range (m = " + std::to_string(m) + ")");
    hipStream_t s = h->stream;
    // a preparation cached for the previous selection describes arrays that are about to change; any other stays
    if (h->prep_key.valid && (inside(h->prep_key.ptr, h->sub_ptr) || inside(h->prep_key.idx, h->sub_idx) || inside(h->prep_key.val, h->sub_val)))
      h->prep_key.valid = false;
    int64_t* o_ptr = h->sub_ptr.as<int64_t>(n_rows + 1);
    int64_t total = 0;
    const uint64_t* d_rows = nullptr;
    if (n_rows == 0) {
      SAPCA_HIP(hipMemsetAsync(o_ptr, 0, sizeof(int64_t), s));
    } else {
      uint64_t* dr = h->sub_rows.as<uint64_t>(n_rows);
      SAPCA_HIP(hipMemcpyAsync(dr, rows, n_rows * sizeof(uint64_t), hipMemcpyHostToDevice, s));
      d_rows = dr;
      sapca::k::select_rows_offsets(A.ptr, d_rows, (int64_t)n_rows, o_ptr, &total, h->sub_scan, s);
    }
    int32_t* o_idx = h->sub_idx.as<int32_t>(std::max<int64_t>(total, 1));
    T* o_val = h->sub_val.as<T>(std::max<int64_t>(total, 1));
    sapca::k::select_rows_fill(A, d_rows, (int64_t)n_rows, o_ptr, total, o_idx, o_val, s);
    SAPCA_HIP(hipStreamSynchronize(s));   // the arrays are complete when the call returns, whatever stream reads them next
    *nnz_out = (uint64_t)total;
    *d_ptr = o_ptr;
    *d_idx = o_idx;
    *d_val = o_val;
  });
}

// ---- the gate in front of the device entry points (canon.hip) ----------------------------------------------------------
bool inside_buf(const void* q, const sapca::DevBuf& b) {
  const char* c = static_cast<const char*>(q);
  return b.p != nullptr && c >= static_cast<const char*>(b.p) && c < static_cast<const char*>(b.p) + b.cap;
}

// The check of a device CSR: the offsets first (one synchronisation: nothing reads an entry before they are known to be
// sound), then one pass over the entries; with_lists: the rows that need sorting are listed behind it for canonicalize.
// ctr_host receives the counter block; the per-row words stay in h->canon_rows.
template <typename T>
void run_check(sapca_handle h, const CsrView<T>& A, sapca_csr_report* rep, unsigned long long* ctr_host, bool with_lists) {
  namespace K = sapca::k;
  hipStream_t s = h->stream;
  const int64_t m = A.rows;
  unsigned long long* ctr = h->canon_ctr.as<unsigned long long>(K::kCtrSlots);
  // per row: defect bits, and for canonicalize behind them distinct columns | three lists (uint32 each)
  uint32_t* rows = h->canon_rows.as<uint32_t>((size_t)std::max<int64_t>(with_lists ? 5 * m : m, 1));
  unsigned long long* long_off = with_lists ? h->canon_long.as<unsigned long long>((size_t)std::max<int64_t>(m, 1)) : nullptr;
  K::canon_check_offsets(A.ptr, m, A.nnz, ctr, s);
  SAPCA_HIP(hipMemcpyAsync(ctr_host, ctr, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
  SAPCA_HIP(hipStreamSynchronize(s));
  const uint64_t none = UINT64_MAX;
  sapca_csr_report r{};
  r.struct_size = (uint32_t)sizeof(sapca_csr_report);
  r.first_bad_offset_row = ctr_host[K::kCtrFirstBadOffset];
  r.first_out_of_range_row = r.first_unsorted_row = r.first_duplicate_row = r.first_nonfinite_row = none;
  if (r.first_bad_offset_row != none) {
    r.flags = SAPCA_CSR_BAD_OFFSETS;
  } else {
    K::canon_check_entries(A, rows, ctr, s);
    if (with_lists) K::canon_list_rows(A.ptr, rows, m, rows + 2 * m, long_off, ctr, s);
    SAPCA_HIP(hipMemcpyAsync(ctr_host, ctr, K::kCtrSlots * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    SAPCA_HIP(hipStreamSynchronize(s));
    r.cols_out_of_range = ctr_host[K::kCtrColsOutOfRange];
    r.first_out_of_range_row = ctr_host[K::kCtrFirstOutOfRange];
    r.unsorted_rows = ctr_host[K::kCtrUnsortedRows];
    r.first_unsorted_row = ctr_host[K::kCtrFirstUnsorted];
    r.duplicate_entries = ctr_host[K::kCtrDuplicates];
    r.first_duplicate_row = ctr_host[K::kCtrFirstDuplicate];
    r.nonfinite_values = ctr_host[K::kCtrNonfinite];
    r.first_nonfinite_row = ctr_host[K::kCtrFirstNonfinite];
    r.stored_zeros = ctr_host[K::kCtrStoredZeros];
    r.flags = (r.cols_out_of_range ? SAPCA_CSR_COL_RANGE : 0u) | (r.unsorted_rows ? SAPCA_CSR_UNSORTED : 0u) |
              (r.duplicate_entries ? SAPCA_CSR_DUPLICATES : 0u) | (r.nonfinite_values ? SAPCA_CSR_NONFINITE : 0u);
  }
  *rep = r;
}

void check_report_arg(const sapca_csr_report* report, const char* who) {
  SAPCA_CHECK(report->struct_size == sizeof(sapca_csr_report), SAPCA_ERR_ARG,
              std::string(who) + ": report->struct_size is " + std::to_string(report->struct_size) + ", this library's sapca_csr_report has " +
                  std::to_string(sizeof(sapca_csr_report)) + " bytes");
}

template <typename T>
sapca_status check_device(sapca_handle h, uint64_t m, uint64_t n, uint64_t nnz, const int64_t* p, const int32_t* i, const T* v,
                          sapca_csr_report* report) {
  return guarded(h, [&] {
    SAPCA_CHECK(report != nullptr, SAPCA_ERR_ARG, "check_csr: null report");
    check_report_arg(report, "check_csr");
    CsrView<T> A = device_view<T>(m, n, nnz, p, i, v);
    unsigned long long ctr_host[sapca::k::kCtrSlots] = {};
    sapca_csr_report r;
    run_check(h, A, &r, ctr_host, false);
    *report = r;
  });
}

// dst <- src, `bytes` of device memory on the stream: the 16-byte streaming copy where both ends allow it, the tail (and an
// unaligned source) through the runtime's copy
void device_copy(const void* src, void* dst, size_t bytes, hipStream_t s) {
  if (bytes == 0) return;
  size_t body = 0;
  if ((reinterpret_cast<uintptr_t>(src) & 15) == 0 && (reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
    body = bytes & ~(size_t)15;
    sapca::k::stream_copy16(src, dst, (int64_t)body, s);
  }
  if (body < bytes)
    SAPCA_HIP(hipMemcpyAsync(static_cast<char*>(dst) + body, static_cast<const char*>(src) + body, bytes - body, hipMemcpyDeviceToDevice, s));
}

// Rows sorted by column, equal columns summed (canon.hip).  Everything that can be refused is refused before a canonical
// buffer is touched; a canonical input is handed back as it is.
template <typename T>
sapca_status canonicalize_device(sapca_handle h, uint64_t m, uint64_t n, uint64_t nnz, const int64_t* p, const int32_t* i, const T* v,
                                 uint64_t* nnz_out, const int64_t** d_ptr, const int32_t** d_idx, T** d_val, sapca_csr_report* report) {
  return guarded(h, [&] {
    namespace K = sapca::k;
    SAPCA_CHECK(nnz_out && d_ptr && d_idx && d_val, SAPCA_ERR_ARG, "canonicalize: null output pointer");
    if (report) check_report_arg(report, "canonicalize");
    CsrView<T> A = device_view<T>(m, n, nnz, p, i, v);
    auto own = [&](const void* q) {
      return inside_buf(q, h->canon_ptr) || inside_buf(q, h->canon_idx) || inside_buf(q, h->canon_val) || inside_buf(q, h->canon_idx2) ||
             inside_buf(q, h->canon_val2);
    };
    SAPCA_CHECK(!own(p) && !own(i) && !own(v), SAPCA_ERR_ARG,
                "canonicalize: the source is this handle's own canonical result, which the call overwrites (it is canonical already)");
    unsigned long long ctr_host[K::kCtrSlots] = {};
    sapca_csr_report r;
    run_check(h, A, &r, ctr_host, true);
    if (r.flags & SAPCA_CSR_BAD_OFFSETS)
      throw Error(SAPCA_ERR_ARG, "canonicalize: the row offsets are broken at row " + std::to_string(r.first_bad_offset_row) +
                                     " (ptr[0] != 0, a decreasing offset, or ptr[m] != nnz): this cannot be repaired");
    if (r.flags & SAPCA_CSR_COL_RANGE)
      throw Error(SAPCA_ERR_ARG, "canonicalize: " + std::to_string(r.cols_out_of_range) + " column indices are out of range (n = " +
                                     std::to_string(n) + "), the first in row " + std::to_string(r.first_out_of_range_row) +
                                     ": this cannot be repaired");
    if ((r.flags & (SAPCA_CSR_UNSORTED | SAPCA_CSR_DUPLICATES)) == 0) {   // the common case: the check's one pass is all it costs
      *nnz_out = nnz;
      *d_ptr = p;
      *d_idx = i;
      *d_val = const_cast<T*>(v);
      if (report) *report = r;
      return;
    }
    hipStream_t s = h->stream;
    // a preparation cached for the previous canonical result describes arrays that are about to change; any other stays
    if (h->prep_key.valid && (own(h->prep_key.ptr) || own(h->prep_key.idx) || own(h->prep_key.val))) h->prep_key.valid = false;
    const int64_t rows = A.rows;
    int64_t* o_ptr = h->canon_ptr.as<int64_t>(m + 1);
    int32_t* o_idx = h->canon_idx.as<int32_t>(nnz);
    T* o_val = h->canon_val.as<T>(nnz);
    device_copy(A.idx, o_idx, nnz * sizeof(int32_t), s);
    device_copy(A.val, o_val, nnz * sizeof(T), s);
    uint32_t* row_bits = h->canon_rows.ptr<uint32_t>();
    const int64_t counts[3] = {(int64_t)ctr_host[K::kCtrListWave], (int64_t)ctr_host[K::kCtrListLds], (int64_t)ctr_host[K::kCtrListLong]};
    unsigned long long* keys = counts[2] ? h->canon_keys.as<unsigned long long>(ctr_host[K::kCtrLongEntries]) : nullptr;
    unsigned long long* ctr = h->canon_ctr.ptr<unsigned long long>();
    K::canon_sort_rows(A, row_bits + 2 * rows, h->canon_long.ptr<unsigned long long>(), counts, keys, o_idx, o_val, row_bits + rows, ctr, s);
    unsigned long long merged = 0;
    SAPCA_HIP(hipMemcpyAsync(&merged, ctr + K::kCtrMerged, sizeof(merged), hipMemcpyDeviceToHost, s));
    SAPCA_HIP(hipStreamSynchronize(s));
    if (merged == 0) {   // the rows did not move: the offsets are the input's
      device_copy(A.ptr, o_ptr, (m + 1) * sizeof(int64_t), s);
    } else {
      K::canon_new_lengths(A.ptr, row_bits, row_bits + rows, rows, o_ptr, s);
      K::exclusive_scan_i64(o_ptr, rows + 1, h->canon_scan, 0, s);
      int32_t* f_idx = h->canon_idx2.as<int32_t>(nnz - merged + 1);
      T* f_val = h->canon_val2.as<T>(nnz - merged + 1);
      K::canon_merge_fill(A.ptr, o_idx, o_val, rows, o_ptr, f_idx, f_val, s);
      o_idx = f_idx;
      o_val = f_val;
    }
    SAPCA_HIP(hipStreamSynchronize(s));   // the arrays are complete when the call returns, whatever stream reads them next
    r.duplicate_entries = merged;         // exact here: adjacent or not, every entry that merged
    if (merged) r.flags |= SAPCA_CSR_DUPLICATES;
    *nnz_out = nnz - merged;
    *d_ptr = o_ptr;
    *d_idx = o_idx;
    *d_val = o_val;
    if (report) *report = r;
  });
}

// MatrixNTop::sum_row_n_top (csr.rs:1347-1376) for several n in one pass over the rows: out[i * m + r]
template <typename T>
sapca_status top_n_device(sapca_handle h, uint64_t m, uint64_t n, uint64_t nnz, const int64_t* p, const int32_t* i, const T* v,
                          const uint64_t* ns, uint32_t n_ns, double* out) {
  return guarded(h, [&] {
    SAPCA_CHECK(n_ns > 0 && ns != nullptr, SAPCA_ERR_ARG, "sum_row_n_top: at least one n is needed");
    SAPCA_CHECK(out != nullptr || m == 0, SAPCA_ERR_ARG, "null output");
    CsrView<T> A = device_view<T>(m, n, nnz, p, i, v);
    if (m == 0) return;
    hipStream_t s = h->stream;
    uint64_t* d_ns = h->batch_in.as<uint64_t>(n_ns);
    double* d_out = h->batch_out.as<double>((size_t)n_ns * m);
    SAPCA_HIP(hipMemcpyAsync(d_ns, ns, n_ns * sizeof(uint64_t), hipMemcpyHostToDevice, s));
    sapca::k::row_top_n(A, d_ns, (int)n_ns, d_out, s);
    SAPCA_HIP(hipMemcpyAsync(out, d_out, (size_t)n_ns * m * sizeof(double), hipMemcpyDeviceToHost, s));
    SAPCA_HIP(hipStreamSynchronize(s));
  });
}

template <typename T>
sapca_status spmm_host(sapca_handle h, uint64_t m, uint64_t n, uint64_t nnz, const uint64_t* ro, const uint64_t* ci,
                       const T* v, const T* mu, uint64_t l, const T* In, T* Out, bool transposed) {
  return guarded(h, [&] {
    SAPCA_CHECK(l >= 1 && l <= (uint64_t)sapca::k::kMaxPanelWidth && In && Out, SAPCA_ERR_ARG, "spmm: panel width must be in [1, 1024]");
    CsrView<T> A = upload<T>(h, m, n, nnz, ro, ci, v);
    hipStream_t s = h->stream;
    // spmm_variant == 2 exercises the LDS-staged sweep on its own (f32 only): panels padded to 64/128
    const bool want_tiled = h->opt.spmm_variant == 2;
    const int ld = l > 128 ? (int)sapca::round_up((int64_t)l, 64) : want_tiled ? (l <= 64 ? 64 : 128) : (int)sapca::round_up((int64_t)l, 16);
    const uint64_t in_rows = transposed ? m : n, out_rows = transposed ? n : m;
    T* stage = h->scratch2.as<T>(std::max<uint64_t>(in_rows * l, out_rows * l) + n + 2 * (uint64_t)std::max(ld, 128));
    T* X = h->panel_x.as<T>(std::max<uint64_t>(in_rows, 1) * ld);
    T* Y = h->panel_y.as<T>(std::max<uint64_t>(out_rows, 1) * ld);
    SAPCA_HIP(hipMemcpyAsync(stage, In, in_rows * l * sizeof(T), hipMemcpyHostToDevice, s));
    sapca::k::add_padding(stage, (int64_t)in_rows, (int)l, X, ld, s);
    T* d_mu = nullptr;
    if (mu) {
      d_mu = h->mean_used_dev.as<T>(n);
      SAPCA_HIP(hipMemcpyAsync(d_mu, mu, n * sizeof(T), hipMemcpyHostToDevice, s));
    }
    const sapca::SmallLayout lay(h->small, ld);
    T* cvec = lay.c<T>();
    T* svec = lay.s<T>();
    SAPCA_HIP(hipStreamSynchronize(s));
    if (!transposed) {
      if (mu) sapca::k::weighted_colsum(X, (int64_t)n, ld, d_mu, cvec, h->scratch, s);
      const sapca::TiledOp* top = nullptr;
      if (want_tiled && sapca::k::build_tiled(A, 64, h->tiled_a, h->tb_a, s)) top = &h->tiled_a;   // else: row kernel
      sapca::k::spmm(A, top, X, ld, Y, ld, ld, mu ? cvec : nullptr, h->opt.spmm_variant, h->split_scratch, s);
    } else {
      int64_t* at_ptr = h->at_ptr.as<int64_t>(n + 1);
      int32_t* at_idx = h->at_idx.as<int32_t>(std::max<uint64_t>(nnz, 1));
      T* at_val = h->at_val.as<T>(std::max<uint64_t>(nnz, 1));
      sapca::k::transpose_csr(A, at_ptr, at_idx, at_val, h->scratch, s);
      CsrView<T> At;
      At.rows = (int64_t)n; At.cols = (int64_t)m; At.nnz = (int64_t)nnz; At.ptr = at_ptr; At.idx = at_idx; At.val = at_val;
      const sapca::TiledOp* top = nullptr;
      if (want_tiled && sapca::k::build_tiled(At, 64, h->tiled_at, h->tb_at, s)) top = &h->tiled_at;
      sapca::k::spmm(At, top, X, ld, Y, ld, ld, (const T*)nullptr, h->opt.spmm_variant, h->split_scratch, s);
      if (mu) {
        sapca::k::weighted_colsum(X, (int64_t)m, ld, (const T*)nullptr, svec, h->scratch, s);
        sapca::k::rank1_subtract(Y, (int64_t)n, ld, d_mu, svec, s);
      }
    }
    sapca::k::strip_padding(Y, (int64_t)out_rows, ld, (int)l, stage, s);
    download_out(h, stage, Out, (size_t)(out_rows * l));
  });
}

template <typename T>
sapca_status normalize_host(sapca_handle h, int32_t normalizer, uint64_t rows, uint64_t l, T* panel) {
  return guarded(h, [&] {
    SAPCA_CHECK(l >= 1 && l <= (uint64_t)sapca::k::kMaxPanelWidth && panel && rows >= 1, SAPCA_ERR_ARG, "normalize: panel width must be in [1, 1024]");
    SAPCA_CHECK(normalizer >= 0 && normalizer <= 2, SAPCA_ERR_ARG, "unknown normalizer");
    hipStream_t s = h->stream;
    const int ld = (int)sapca::round_up((int64_t)l, l > 128 ? 64 : 16);
    T* stage = h->scratch.as<T>(rows * l);
    T* P = h->panel_y.as<T>(rows * ld);
    SAPCA_HIP(hipMemcpyAsync(stage, panel, rows * l * sizeof(T), hipMemcpyHostToDevice, s));
    sapca::k::add_padding(stage, (int64_t)rows, (int)l, P, ld, s);
    Engine<T>::normalize(*h, P, (int64_t)rows, (int)l, ld, normalizer, false, {});
    sapca::k::strip_padding(P, (int64_t)rows, ld, (int)l, stage, s);
    download_out(h, stage, panel, (size_t)(rows * l));
  });
}

template <typename T>
sapca_status omega_host(sapca_handle h, uint64_t rows, uint64_t l, T* out) {
  return guarded(h, [&] {
    SAPCA_CHECK(l >= 1 && l <= (uint64_t)sapca::k::kMaxPanelWidth && out, SAPCA_ERR_ARG, "omega: panel width must be in [1, 1024]");
    const int ld = (int)sapca::round_up((int64_t)l, 16);
    T* P = h->panel_x.as<T>(std::max<uint64_t>(rows, 1) * ld);
    T* stage = h->scratch.as<T>(std::max<uint64_t>(rows * l, 1));
    sapca::k::gaussian_panel(P, (int64_t)rows, (int)l, ld, h->opt.random_seed, h->stream);
    sapca::k::strip_padding(P, (int64_t)rows, ld, (int)l, stage, h->stream);
    download_out(h, stage, out, (size_t)(rows * l));
  });
}

}  // namespace

extern "C" {

int sapca_abi_version(void) { return SAPCA_ABI_VERSION; }

void sapca_options_default(sapca_options* o) {
  if (!o) return;
  std::memset(o, 0, sizeof(*o));
  o->struct_size = (uint32_t)sizeof(sapca_options);
  o->random_seed = 42;        // sparse/mod.rs:397
  o->n_components = 50;       // :394
  o->alpha = 1.0;             // :395
  o->tolerance = 1e-6;        // :396
  o->center = 1;              // :398
  o->verbose = 0;             // :399
  o->lanczos_center = 0;      // (no reference counterpart: the reference's Lanczos fit runs on the raw matrix, quirk Q1)
  o->method = SAPCA_LANCZOS;  // pca/mod.rs:64-68
  o->n_oversamples = 10;
  o->n_power_iterations = 4;
  o->normalizer = SAPCA_NORM_QR;
  o->transform_semantics = SAPCA_TRANSFORM_REFERENCE;
  o->device_id = -1;
  o->spmm_variant = 0;
  o->stream = nullptr;
}

sapca_status sapca_create(const sapca_options* opts, sapca_handle* out) {
  if (!out) return SAPCA_ERR_ARG;
  *out = nullptr;
  try {
    sapca_options o;
    sapca_options_default(&o);
    if (opts) {
      SAPCA_CHECK(opts->struct_size == sizeof(sapca_options), SAPCA_ERR_ARG, "sapca_options.struct_size mismatch (ABI)");
      o = *opts;
    }
    SAPCA_CHECK(o.method == SAPCA_LANCZOS || o.method == SAPCA_RANDOM, SAPCA_ERR_ARG, "unknown SVD method");
    SAPCA_CHECK(o.normalizer >= 0 && o.normalizer <= 2, SAPCA_ERR_ARG, "unknown normalizer");
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev == 0)
      throw Error(SAPCA_ERR_HIP, "no HIP device available: libsapca has no CPU path");
    sapca_handle h = new sapca_handle_s();
    h->opt = o;
    if (o.device_id >= 0) h->device = o.device_id;
    else SAPCA_HIP(hipGetDevice(&h->device));
    SAPCA_HIP(hipSetDevice(h->device));
    if (o.stream) {
      h->stream = static_cast<hipStream_t>(o.stream);
    } else {
      SAPCA_HIP(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
      h->own_stream = true;
    }
    *out = h;
    return SAPCA_OK;
  } catch (const Error& e) {
    g_create_error = e.what();
    return e.code;
  } catch (const std::exception& e) {
    g_create_error = e.what();
    return SAPCA_ERR_NOMEM;
  }
}

void sapca_destroy(sapca_handle h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  (void)hipStreamSynchronize(h->stream);
  h->comm.destroy();
  for (int b = 0; b < 2; ++b)
    if (h->up_done[b]) (void)hipEventDestroy(h->up_done[b]);
  if (h->stream2) {
    (void)hipStreamSynchronize(h->stream2);
    (void)hipStreamDestroy(h->stream2);
  }
  if (h->stream_comm) {
    (void)hipStreamSynchronize(h->stream_comm);
    (void)hipStreamDestroy(h->stream_comm);
    if (h->ev_piece) (void)hipEventDestroy(h->ev_piece);
    if (h->ev_comm) (void)hipEventDestroy(h->ev_comm);
  }
  if (h->stream3) {
    (void)hipStreamSynchronize(h->stream3);
    (void)hipStreamDestroy(h->stream3);
  }
  if (h->held_small.ev) (void)hipEventDestroy(h->held_small.ev);
  if (h->ev_kept) (void)hipEventDestroy(h->ev_kept);
  if (h->ev_stats) (void)hipEventDestroy(h->ev_stats);
  if (h->ev_fork) (void)hipEventDestroy(h->ev_fork);
  if (h->ev_join) (void)hipEventDestroy(h->ev_join);
  if (h->ev_drop) (void)hipEventDestroy(h->ev_drop);
  if (h->up_stats_done) (void)hipEventDestroy(h->up_stats_done);
  if (h->own_stream) (void)hipStreamDestroy(h->stream);
  delete h;
}

const char* sapca_last_error(sapca_handle h) { return h ? h->err.c_str() : g_create_error.c_str(); }

sapca_status sapca_set_mask(sapca_handle h, const uint8_t* mask, size_t len) {
  if (!h) return SAPCA_ERR_ARG;
  if (len && !mask) return SAPCA_ERR_ARG;
  h->mask.assign(mask, mask + len);
  for (auto& b : h->mask) b = b ? 1 : 0;
  h->mask_version++;
  h->prep_key.valid = false;
  return SAPCA_OK;
}

sapca_status sapca_set_omega_f32(sapca_handle h, const float* omega, size_t rows, size_t cols) {
  if (!h || ((rows * cols) && !omega)) return SAPCA_ERR_ARG;
  h->omega.assign(omega, omega + rows * cols);
  h->omega_rows = rows;
  h->omega_cols = cols;
  return SAPCA_OK;
}
sapca_status sapca_set_omega_f64(sapca_handle h, const double* omega, size_t rows, size_t cols) {
  if (!h || ((rows * cols) && !omega)) return SAPCA_ERR_ARG;
  h->omega.assign(omega, omega + rows * cols);
  h->omega_rows = rows;
  h->omega_cols = cols;
  return SAPCA_OK;
}

#define SAPCA_DEFINE_TYPED(SUF, T)                                                                                       \
  sapca_status sapca_fit_csr_##SUF(sapca_handle h, uint64_t m, uint64_t n, uint64_t nnz, const uint64_t* ro,             \
                                   const uint64_t* ci, const T* v) {                                                     \
    return fit_host<T>(h, m, n, nnz, ro, ci, v);                                                                         \
  }                                                                                                                      \
  sapca_status sapca_transform_csr_##SUF(sapca_handle h, uint64_t m, uint64_t n, uint64_t nnz, const uint64_t* ro,       \
                                         const uint64_t* ci, const T* v, T* out) {                                       \
    return transform_host<T>(h, m, n, nnz, ro, ci, v, out, false);                                                       \
  }                                                                                                                      \
  sapca_status sapca_fit_transform_csr_##SUF(sapca_handle h, uint64_t m, uint64_t n, uint64_t nnz, const uint64_t* ro,   \
                                             const uint64_t* ci, const T* v, T* out) {                                   \
    return transform_host<T>(h, m, n, nnz, ro, ci, v, out, true);                                                        \
  }                                                                                                                      \
  sapca_status sapca_fit_csr_device_##SUF(sapca_handle h, uint64_t m, uint64_t n, uint64_t nnz, const int64_t* p,        \
                                          const int32_t* i, const T* v) {                                                \
    return fit_device<T>(h, m, n, nnz, p, i, v);                                                                         \
  }                                                                                                                      \
  sapca_status sapca_transform_csr_device_##SUF(sapca_handle h, uint64_t m, uint64_t n, uint64_t nnz, const int64_t* p,  \
                                                const int32_t* i, const T* v, T* out) {                                  \
    return transform_device<T>(h, m, n, nnz, p, i, v, out, false);                                                       \
  }                                                                                                                      \
  sapca_status sapca_fit_transform_csr_device_##SUF(sapca_handle h, uint64_t m, uint64_t n, uint64_t nnz,                \
                                                    const int64_t* p, const int32_t* i, const T* v, T* out) {            \
    return transform_device<T>(h, m, n, nnz, p, i, v, out, true);                                                        \
  }                                                                                                                      \
  sapca_status sapca_transform_csr_device_to_host_##SUF(sapca_handle h, uint64_t m, uint64_t n, uint64_t nnz,            \
                                                        const int64_t* p, const int32_t* i, const T* v, T* out) {        \
    return transform_device<T>(h, m, n, nnz, p, i, v, out, false, true);                                                 \
  }                                                                                                                      \
  sapca_status sapca_fit_transform_csr_device_to_host_##SUF(sapca_handle h, uint64_t m, uint64_t n, uint64_t nnz,        \
                                                            const int64_t* p, const int32_t* i, const T* v, T* out) {    \
    return transform_device<T>(h, m, n, nnz, p, i, v, out, true, true);                                                  \
  }                                                                                                                      \
  sapca_status sapca_get_components_##SUF(sapca_handle h, T* out, size_t cap) {                                          \
    return guarded(h, [&] { get_components<T>(h, out, cap, false); });                                                   \
  }                                                                                                                      \
  sapca_status sapca_get_feature_importances_##SUF(sapca_handle h, T* out, size_t cap) {                                 \
    return guarded(h, [&] { get_components<T>(h, out, cap, true); });                                                    \
  }                                                                                                                      \
  sapca_status sapca_get_singular_values_##SUF(sapca_handle h, T* out, size_t cap) {                                     \
    return guarded(h, [&] { need_fitted(h); copy_out<T>(h->sing, out, cap); });                                          \
  }                                                                                                                      \
  sapca_status sapca_get_explained_variance_##SUF(sapca_handle h, T* out, size_t cap) {                                  \
    return guarded(h, [&] { need_fitted(h); copy_out<T>(h->expl_var, out, cap); });                                      \
  }                                                                                                                      \
  sapca_status sapca_get_mean_##SUF(sapca_handle h, T* out, size_t cap) {                                                \
    return guarded(h, [&] { need_fitted(h); copy_out<T>(h->mean, out, cap); });                                          \
  }                                                                                                                      \
  sapca_status sapca_get_explained_variance_ratio_##SUF(sapca_handle h, T* out, size_t cap) {                            \
    return guarded(h, [&] { get_ratio<T>(h, out, cap, false); });                                                        \
  }                                                                                                                      \
  sapca_status sapca_get_cumulative_explained_variance_ratio_##SUF(sapca_handle h, T* out, size_t cap) {                 \
    return guarded(h, [&] { get_ratio<T>(h, out, cap, true); });                                                         \
  }                                                                                                                      \
  sapca_status sapca_colstats_csr_##SUF(sapca_handle h, uint64_t m, uint64_t n, uint64_t nnz, const uint64_t* ro,        \
                                        const uint64_t* ci, const T* v, T* sc, T* ssq, uint64_t* cnt) {                  \
    return colstats_host<T>(h, m, n, nnz, ro, ci, v, sc, ssq, cnt);                                                      \
  }                                                                                                                      \
  sapca_status sapca_upload_csr_##SUF(sapca_handle h, uint64_t m, uint64_t n, uint64_t nnz, const uint64_t* ro,          \
                                      const uint64_t* ci, const T* v, const int64_t** dp, const int32_t** di, T** dv) {  \
    return upload_host<T>(h, m, n, nnz, ro, ci, v, dp, di, dv);                                                          \
  }                                                                                                                      \
  sapca_status sapca_normalize_csr_device_##SUF(sapca_handle h, uint64_t m, uint64_t n, uint64_t nnz, const int64_t* p,  \
                                                const int32_t* i, T* v, const double* sums, uint64_t sums_len,            \
                                                double target, int32_t direction) {                                      \
    return normalize_device<T>(h, m, n, nnz, p, i, v, sums, sums_len, target, direction);                                \
  }                                                                                                                      \
  sapca_status sapca_log1p_csr_device_##SUF(sapca_handle h, uint64_t nnz, T* v) { return log1p_device<T>(h, nnz, v); }    \
  sapca_status sapca_stats_csr_device_##SUF(sapca_handle h, uint64_t m, uint64_t n, uint64_t nnz, const int64_t* p,      \
                                            const int32_t* i, const T* v, int32_t direction, double* sum, double* sumsq, \
                                            uint64_t* nonzero, T* minv, T* maxv) {                                       \
    return stats_device<T>(h, m, n, nnz, p, i, v, direction, sum, sumsq, nonzero, minv, maxv);                           \
  }                                                                                                                      \
  sapca_status sapca_batch_stats_csr_device_##SUF(sapca_handle h, uint64_t m, uint64_t n, uint64_t nnz, const int64_t* p, \
                                                  const int32_t* i, const T* v, int32_t grouped_axis, const int32_t* codes, \
                                                  uint64_t codes_len, uint32_t n_batches, double* mean, double* var,        \
                                                  uint64_t* count) {                                                        \
    return batch_stats_device<T>(h, m, n, nnz, p, i, v, grouped_axis, codes, codes_len, n_batches, mean, var, count);     \
  }                                                                                                                      \
  sapca_status sapca_masked_stats_csr_device_##SUF(sapca_handle h, uint64_t m, uint64_t n, uint64_t nnz, const int64_t* p, \
                                                   const int32_t* i, const T* v, int32_t direction, const uint8_t* mask,    \
                                                   uint64_t mask_len, double* sum, double* sum_squared, uint64_t* count,    \
                                                   double* var) {                                                           \
    return masked_stats_device<T>(h, m, n, nnz, p, i, v, direction, mask, mask_len, sum, sum_squared, count, var);        \
  }                                                                                                                      \
  sapca_status sapca_select_rows_csr_device_##SUF(sapca_handle h, uint64_t m, uint64_t n, uint64_t nnz, const int64_t* p,  \
                                                  const int32_t* i, const T* v, const uint64_t* rows, uint64_t n_rows,     \
                                                  uint64_t* nnz_out, const int64_t** dp, const int32_t** di, T** dv) {     \
    return select_rows_device<T>(h, m, n, nnz, p, i, v, rows, n_rows, nnz_out, dp, di, dv);                               \
  }                                                                                                                      \
  sapca_status sapca_check_csr_device_##SUF(sapca_handle h, uint64_t m, uint64_t n, uint64_t nnz, const int64_t* p,        \
                                            const int32_t* i, const T* v, sapca_csr_report* report) {                      \
    return check_device<T>(h, m, n, nnz, p, i, v, report);                                                                \
  }                                                                                                                      \
  sapca_status sapca_canonicalize_csr_device_##SUF(sapca_handle h, uint64_t m, uint64_t n, uint64_t nnz, const int64_t* p, \
                                                   const int32_t* i, const T* v, uint64_t* nnz_out, const int64_t** dp,    \
                                                   const int32_t** di, T** dv, sapca_csr_report* report) {                 \
    return canonicalize_device<T>(h, m, n, nnz, p, i, v, nnz_out, dp, di, dv, report);                                    \
  }                                                                                                                      \
  sapca_status sapca_sum_row_n_top_csr_device_##SUF(sapca_handle h, uint64_t m, uint64_t n, uint64_t nnz, const int64_t* p, \
                                                    const int32_t* i, const T* v, const uint64_t* ns, uint32_t n_ns,        \
                                                    double* out) {                                                          \
    return top_n_device<T>(h, m, n, nnz, p, i, v, ns, n_ns, out);                                                         \
  }                                                                                                                      \
  sapca_status sapca_spmm_csr_##SUF(sapca_handle h, uint64_t m, uint64_t n, uint64_t nnz, const uint64_t* ro,            \
                                    const uint64_t* ci, const T* v, const T* mu, uint64_t l, const T* X, T* Y) {         \
    return spmm_host<T>(h, m, n, nnz, ro, ci, v, mu, l, X, Y, false);                                                    \
  }                                                                                                                      \
  sapca_status sapca_spmmt_csr_##SUF(sapca_handle h, uint64_t m, uint64_t n, uint64_t nnz, const uint64_t* ro,           \
                                     const uint64_t* ci, const T* v, const T* mu, uint64_t l, const T* Y, T* Z) {        \
    return spmm_host<T>(h, m, n, nnz, ro, ci, v, mu, l, Y, Z, true);                                                     \
  }                                                                                                                      \
  sapca_status sapca_normalize_panel_##SUF(sapca_handle h, int32_t normalizer, uint64_t rows, uint64_t l, T* panel) {    \
    return normalize_host<T>(h, normalizer, rows, l, panel);                                                             \
  }                                                                                                                      \
  sapca_status sapca_generate_omega_##SUF(sapca_handle h, uint64_t rows, uint64_t l, T* out) {                           \
    return omega_host<T>(h, rows, l, out);                                                                               \
  }

SAPCA_DEFINE_TYPED(f32, float)
SAPCA_DEFINE_TYPED(f64, double)
#undef SAPCA_DEFINE_TYPED

sapca_status sapca_get_dims(sapca_handle h, uint64_t* k, uint64_t* n_used, uint64_t* n_cols) {
  return guarded(h, [&] {
    need_fitted(h);
    if (k) *k = h->k;
    if (n_used) *n_used = h->n_used;
    if (n_cols) *n_cols = h->n_cols;
  });
}

sapca_status sapca_get_total_variance(sapca_handle h, double* out) {
  return guarded(h, [&] {
    need_fitted(h);
    SAPCA_CHECK(out != nullptr, SAPCA_ERR_ARG, "null output");
    *out = h->total_var;
  });
}

sapca_status sapca_get_mask_index_maps(sapca_handle h, uint64_t* cols_to_use, size_t cap_cols, int64_t* orig_to_masked,
                                       size_t cap_map) {
  return guarded(h, [&] {
    // maps follow the mask currently set (sparse_masked/mod.rs:264-271, :455-466); no fit needed
    std::vector<uint64_t> cols;
    std::vector<int64_t> o2m(h->mask.size(), -1);
    for (size_t j = 0; j < h->mask.size(); ++j)
      if (h->mask[j]) {
        o2m[j] = (int64_t)cols.size();
        cols.push_back((uint64_t)j);
      }
    if (cols_to_use) {
      SAPCA_CHECK(cap_cols >= cols.size(), SAPCA_ERR_ARG, "cols_to_use buffer too small");
      std::copy(cols.begin(), cols.end(), cols_to_use);
    }
    if (orig_to_masked) {
      SAPCA_CHECK(cap_map >= o2m.size(), SAPCA_ERR_ARG, "orig_to_masked buffer too small");
      std::copy(o2m.begin(), o2m.end(), orig_to_masked);
    }
  });
}

sapca_status sapca_get_timings(sapca_handle h, sapca_timings* out) {
  if (!h || !out) return SAPCA_ERR_ARG;
  *out = h->timings;
  return SAPCA_OK;
}

sapca_status sapca_partition_rows(uint64_t m, const uint64_t* row_offsets, uint32_t nparts, uint64_t* bounds) {
  if (!row_offsets || !bounds || nparts == 0) return SAPCA_ERR_ARG;
  // contiguous ranges balanced by stored entries: boundary p is the first row whose
  // prefix reaches p/nparts of nnz, kept monotone.
  const uint64_t nnz = row_offsets[m] - row_offsets[0];
  bounds[0] = 0;
  for (uint32_t p = 1; p < nparts; ++p) {
    const uint64_t target = row_offsets[0] + (uint64_t)((long double)nnz * p / nparts);
    const uint64_t* it = std::lower_bound(row_offsets, row_offsets + m + 1, target);
    uint64_t r = (uint64_t)(it - row_offsets);
    if (r > 0 && r <= m && target - row_offsets[r - 1] < row_offsets[r] - target) r -= 1;  // nearer boundary
    if (nnz == 0) r = m * p / nparts;
    if (r > m) r = m;
    if (r < bounds[p - 1]) r = bounds[p - 1];
    bounds[p] = r;
  }
  bounds[nparts] = m;
  return SAPCA_OK;
}

sapca_status sapca_upload_values_changed(sapca_handle h) {
  return guarded(h, [&] {
    h->prep_key.valid = false;
    h->up_stats.valid = false;
  });
}

sapca_status sapca_measure_copy_gbs(sapca_handle h, uint64_t bytes, uint32_t reps, double* gbs) {
  return guarded(h, [&] {
    SAPCA_CHECK(gbs != nullptr && bytes >= 4096 && reps >= 1, SAPCA_ERR_ARG, "measure_copy_gbs: bytes >= 4096, reps >= 1");
    bytes &= ~(uint64_t)15;
    void *src = nullptr, *dst = nullptr;
    hipEvent_t a = nullptr, b = nullptr;
    auto cleanup = [&] {
      if (a) (void)hipEventDestroy(a);
      if (b) (void)hipEventDestroy(b);
      if (src) (void)hipFree(src);
      if (dst) (void)hipFree(dst);
    };
    try {
      SAPCA_HIP(hipMalloc(&src, bytes));
      SAPCA_HIP(hipMalloc(&dst, bytes));
      SAPCA_HIP(hipMemsetAsync(src, 1, bytes, h->stream));
      SAPCA_HIP(hipEventCreate(&a));
      SAPCA_HIP(hipEventCreate(&b));
      float best = 0;
      for (uint32_t r = 0; r <= reps; ++r) {   // (the first pass also faults the pages in)
        SAPCA_HIP(hipEventRecord(a, h->stream));
        sapca::k::stream_copy16(src, dst, (int64_t)bytes, h->stream);
        SAPCA_HIP(hipEventRecord(b, h->stream));
        SAPCA_HIP(hipEventSynchronize(b));
        float ms = 0;
        SAPCA_HIP(hipEventElapsedTime(&ms, a, b));
        if (r > 0 && (best == 0 || ms < best)) best = ms;
      }
      *gbs = 2.0 * (double)bytes / ((double)best * 1e-3) / 1e9;
    } catch (...) {
      cleanup();
      throw;
    }
    cleanup();
  });
}

int sapca_comm_rccl_available(void) { return sapca::Comm::rccl_available() ? 1 : 0; }

sapca_status sapca_comm_unique_id(uint8_t id[128]) {
  if (!id) return SAPCA_ERR_ARG;
  try {
    sapca::Comm::unique_id(id);
    return SAPCA_OK;
  } catch (const Error& e) {
    g_create_error = e.what();
    return e.code;
  }
}

sapca_status sapca_comm_init_rank(sapca_handle h, uint32_t nranks, uint32_t rank, const uint8_t id[128]) {
  return guarded(h, [&] {
    SAPCA_CHECK(id != nullptr, SAPCA_ERR_ARG, "null unique id");
    h->comm.init_rccl(nranks, rank, id);
  });
}

sapca_status sapca_comm_set_callback(sapca_handle h, uint32_t nranks, uint32_t rank, sapca_allreduce_fn fn, void* ctx) {
  return guarded(h, [&] { h->comm.set_callback(nranks, rank, fn, ctx); });
}

sapca_status sapca_comm_abort(sapca_handle h) {
  if (!h) return SAPCA_ERR_ARG;
  try {   // (not `guarded`: callable from another thread while a fit of this handle is blocked behind a collective)
    h->comm.abort();
    return SAPCA_OK;
  } catch (...) {
    return SAPCA_ERR_COMM;
  }
}

sapca_status sapca_comm_async_error(sapca_handle h, int32_t* state) {
  if (!h || !state) return SAPCA_ERR_ARG;
  try {
    *state = h->comm.async_error();
    return SAPCA_OK;
  } catch (...) {
    return SAPCA_ERR_COMM;
  }
}

int sapca_comm_has_side_lane(sapca_handle h) { return (h && h->comm.has_side_lane()) ? 1 : 0; }

sapca_status sapca_comm_allreduce(sapca_handle h, void* buf, uint64_t count, int32_t dtype) {
  return guarded(h, [&] {
    h->comm.allreduce(buf, count, dtype, h->stream);
    SAPCA_HIP(hipStreamSynchronize(h->stream));
  });
}

}  // extern "C"
