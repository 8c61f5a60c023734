// The row sort of canon.hip as one host stage: the work space, the survey of a CSR (check, row lists, counter block), the sort
// of the listed rows and the offsets of the merged rows.  canonicalize / check (resident.cpp) and the two neighbour-graph
// builders (tsne.cpp) drive it; the layout of the per-row words and the sizing of the key space are known here and nowhere
// else.  The value-typed finishes (canon_merge_fill, umap_union_fill) stay with the callers.
#pragma once
#include "kernels.h"

namespace sapca {
namespace resident {

struct RowSort {
  // the counter block, per row {defect bits | distinct columns | three row lists} (uint32 each), the long rows' key offsets,
  // their keys, the scan's work space
  DevBuf ctr, rows, long_off, keys, scan;
  unsigned long long counters[k::kCtrSlots] = {};   // the counter block as the last survey read it back

  // canon_check_offsets, canon_check_entries and, with_lists, canon_list_rows on A, then the read-back of the counter block.
  // untrusted: A's offsets are the caller's: the call synchronises behind their check and, where they are broken, returns
  // false before an entry is read (counters[kCtrFirstBadOffset] says where).  Otherwise the offsets are this library's own:
  // one synchronisation, at the end.  Without lists `rows` holds the defect bits alone and sort() must not follow.
  template <typename T>
  bool survey(const CsrView<T>& A, bool with_lists, bool untrusted, hipStream_t s);
  bool needs_sort() const { return counters[k::kCtrUnsortedRows] || counters[k::kCtrDuplicates]; }
  // the rows the survey listed, sorted by (column, stored position) into idx / val: the caller's copies of A.idx / A.val, which
  // the values are gathered from.  Returns the entries that merge (synchronises).
  template <typename T>
  uint64_t sort(const CsrView<T>& A, int32_t* idx, T* val, hipStream_t s);
  // new_ptr[0 .. m] = the offsets of the surveyed and sorted rows with every run of equal columns as one entry
  void merged_offsets(const int64_t* ptr, int64_t m, int64_t* new_ptr, hipStream_t s);
};

}  // namespace resident
}  // namespace sapca
