// The row sort's host stage (rowsort.h; the kernels are canon.hip's).
#include "rowsort.h"

#include <algorithm>

namespace sapca {
namespace resident {

namespace K = sapca::k;
using u64 = unsigned long long;

template <typename T>
bool RowSort::survey(const CsrView<T>& A, bool with_lists, bool untrusted, hipStream_t s) {
  const int64_t m = A.rows;
  u64* c = ctr.as<u64>(K::kCtrSlots);
  uint32_t* bits = rows.as<uint32_t>((size_t)std::max<int64_t>(with_lists ? 5 * m : m, 1));
  u64* off = with_lists ? long_off.as<u64>((size_t)std::max<int64_t>(m, 1)) : nullptr;
  K::canon_check_offsets(A.ptr, m, A.nnz, c, s);
  if (untrusted) {
    SAPCA_HIP(hipMemcpyAsync(counters, c, sizeof(u64), hipMemcpyDeviceToHost, s));
    SAPCA_HIP(hipStreamSynchronize(s));
    if (counters[K::kCtrFirstBadOffset] != UINT64_MAX) return false;
  }
  K::canon_check_entries(A, bits, c, s);
  if (with_lists) K::canon_list_rows(A.ptr, bits, m, bits + 2 * m, off, c, s);
  SAPCA_HIP(hipMemcpyAsync(counters, c, sizeof(counters), hipMemcpyDeviceToHost, s));
  SAPCA_HIP(hipStreamSynchronize(s));
  return true;
}

template <typename T>
uint64_t RowSort::sort(const CsrView<T>& A, int32_t* idx, T* val, hipStream_t s) {
  const int64_t m = A.rows;
  uint32_t* bits = rows.ptr<uint32_t>();
  u64* c = ctr.ptr<u64>();
  const int64_t counts[3] = {(int64_t)counters[K::kCtrListWave], (int64_t)counters[K::kCtrListLds], (int64_t)counters[K::kCtrListLong]};
  u64* key_space = counts[2] ? keys.as<u64>(counters[K::kCtrLongEntries]) : nullptr;
  K::canon_sort_rows(A, bits + 2 * m, long_off.ptr<u64>(), counts, key_space, idx, val, bits + m, c, s);
  u64 merged = 0;
  SAPCA_HIP(hipMemcpyAsync(&merged, c + K::kCtrMerged, sizeof(merged), hipMemcpyDeviceToHost, s));
  SAPCA_HIP(hipStreamSynchronize(s));
  return merged;
}

void RowSort::merged_offsets(const int64_t* ptr, int64_t m, int64_t* new_ptr, hipStream_t s) {
  const uint32_t* bits = rows.ptr<uint32_t>();
  K::canon_new_lengths(ptr, bits, bits + m, m, new_ptr, s);
  K::exclusive_scan_i64(new_ptr, m + 1, scan, 0, s);
}

#define SAPCA_INSTANTIATE_ROWSORT(T)                                                  \
  template bool RowSort::survey<T>(const CsrView<T>&, bool, bool, hipStream_t);       \
  template uint64_t RowSort::sort<T>(const CsrView<T>&, int32_t*, T*, hipStream_t);
SAPCA_INSTANTIATE_ROWSORT(float)
SAPCA_INSTANTIATE_ROWSORT(double)
#undef SAPCA_INSTANTIATE_ROWSORT

}  // namespace resident
}  // namespace sapca
