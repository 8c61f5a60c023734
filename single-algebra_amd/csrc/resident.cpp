// The operations on a device-resident CSR (resident.h): upload once, preprocess and analyse in HBM.
#include "resident.h"

#include <cmath>

namespace sapca {
namespace resident {

namespace {

void check_direction(int32_t direction) {
  SAPCA_CHECK(direction == 0 || direction == 1, SAPCA_ERR_ARG, "direction must be 0 (ROW) or 1 (COLUMN)");
}

}  // namespace

template <typename T>
void normalize(H& h, const CsrView<T>& A, T* v, const double* sums, uint64_t sums_len, double target, int32_t direction) {
  check_direction(direction);
  const uint64_t want = direction == 1 ? (uint64_t)A.cols : (uint64_t)A.rows;
  SAPCA_CHECK(sums != nullptr || want == 0, SAPCA_ERR_ARG, "null sums");
  SAPCA_CHECK(sums_len == want, SAPCA_ERR_ARG,
              direction == 1 ? "Length of sums must match number of columns" : "Length of sums must match number of rows");
  check_view(A);
  if (want == 0 || A.nnz == 0) return;
  h.values_changed();
  double* d = h.stats.as<double>(2 * want);
  SAPCA_HIP(hipMemcpyAsync(d, sums, want * sizeof(double), hipMemcpyHostToDevice, h.stream));
  k::normalize_csr(A, v, d, target, direction == 1, d + want, h.stream);
  SAPCA_HIP(hipStreamSynchronize(h.stream));   // `sums` may go out of scope
}

template <typename T>
void log1p(H& h, uint64_t nnz, T* v) {
  SAPCA_CHECK(v != nullptr || nnz == 0, SAPCA_ERR_ARG, "null values");
  h.values_changed();
  k::log1p_values(v, (int64_t)nnz, h.stream);
  SAPCA_HIP(hipStreamSynchronize(h.stream));
}

template <typename T>
void stats(H& h, const CsrView<T>& A, int32_t direction, double* sum, double* sumsq, uint64_t* nonzero, T* minv, T* maxv) {
  check_direction(direction);
  check_view(A);
  hipStream_t s = h.stream;
  const uint64_t len = direction == 1 ? (uint64_t)A.cols : (uint64_t)A.rows;
  if (len == 0) return;
  // h.stats and out_tmp are shared with prepare(), and transform() reads the prepared matrix's column counts from h.stats:
  // this line is what covers the ROW direction (COLUMN drops the preparation again in transpose_into_at, for at_*)
  h.prep_key.valid = false;
  const CsrView<T> R = direction == 1 ? transpose_into_at(h, A) : A;
  double* d = h.stats.as<double>(3 * len + 1);
  T* dmm = h.out_tmp.as<T>(2 * len);
  k::row_stats(R, direction == 0, d, d + len, dmm, dmm + len, s);   // ROW: min / max from the first stored value
  k::row_lengths_f64(R.ptr, (int64_t)len, d + 2 * len, s);
  std::vector<double> host(3 * len);
  std::vector<T> mm(2 * len);
  fetch(host, d, s);
  fetch(mm, dmm, s);
  SAPCA_HIP(hipStreamSynchronize(s));
  for (uint64_t j = 0; j < len; ++j) {
    if (sum) sum[j] = host[j];
    if (sumsq) sumsq[j] = host[len + j];
    if (nonzero) nonzero[j] = (uint64_t)host[2 * len + j];
    if (minv) minv[j] = mm[j];
    if (maxv) maxv[j] = mm[len + j];
  }
}

// BatchMatrixVariance / BatchMatrixMean (csr.rs:1081-1344) through one pass pair per code range.  grouped_axis 0: codes
// label the rows of A (length m), results per column, computed on the rows of A^T; 1: codes label the columns (length n),
// results per row of A.  The host counts the group sizes (the denominators of the means) and finishes mean / var.
template <typename T>
void batch_stats(H& h, const CsrView<T>& A, int32_t grouped_axis, const int32_t* codes, uint64_t codes_len, uint32_t n_batches,
                 double* mean, double* var, uint64_t* count) {
  SAPCA_CHECK(grouped_axis == 0 || grouped_axis == 1, SAPCA_ERR_ARG, "grouped_axis must be 0 (codes label rows) or 1 (columns)");
  check_view(A);
  const uint64_t m = (uint64_t)A.rows, n = (uint64_t)A.cols;
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
  hipStream_t s = h.stream;
  int32_t* d_codes = h.batch_in.as<int32_t>(std::max<uint64_t>(codes_len, 1));
  if (codes_len) SAPCA_HIP(hipMemcpyAsync(d_codes, codes, codes_len * sizeof(int32_t), hipMemcpyHostToDevice, s));
  const CsrView<T> R = grouped_axis == 0 ? transpose_into_at(h, A) : A;
  for_each_code_slice(h, R, d_codes, n_batches, [&](uint32_t lo, int nb, const std::vector<double>& hs, const std::vector<double>& hm,
                                                    const std::vector<uint32_t>& hc) {
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
void masked_stats(H& h, const CsrView<T>& A, int32_t direction, const uint8_t* mask, uint64_t mask_len, double* sum, double* sumsq,
                  uint64_t* count, double* var) {
  check_direction(direction);
  check_view(A);
  const uint64_t m = (uint64_t)A.rows, n = (uint64_t)A.cols, nnz = (uint64_t)A.nnz;
  const uint64_t masked = direction == 1 ? m : n, len = direction == 1 ? n : m;
  if (mask != nullptr && mask_len < masked)   // the reference's message; a longer mask's tail is ignored
    throw Error(SAPCA_ERR_ARG, "Mask length (" + std::to_string(mask_len) + ") is less than number of " +
                                   (direction == 1 ? "rows" : "columns") + " (" + std::to_string(masked) + ")");
  if (len == 0) return;
  hipStream_t s = h.stream;
  const uint64_t words = (masked + 31) / 32;
  uint32_t* d_bits = nullptr;
  std::vector<uint32_t> bits;   // (lives until the results are on the host: its copy is asynchronous)
  if (mask != nullptr) {        // (no mask: no bitset, and the kernels read no mask)
    bits.assign(std::max<uint64_t>(words, 1), 0u);
    for (uint64_t j = 0; j < masked; ++j)
      if (mask[j]) bits[j >> 5] |= 1u << (j & 31);
    d_bits = h.batch_in.as<uint32_t>(bits.size());
    SAPCA_HIP(hipMemcpyAsync(d_bits, bits.data(), bits.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s));
  }
  std::vector<double> hs(len), hq(len), hm2;
  std::vector<uint32_t> hc(len);
  // the ROW kernel on R (A, or A^T for the column direction) into hs / hq / hm2 / hc
  auto row_pass = [&](const CsrView<T>& R) {
    double* d = h.batch_out.as<double>(3 * len + (len + 1) / 2);
    uint32_t* dc = reinterpret_cast<uint32_t*>(d + 3 * len);
    k::masked_row_stats(R, d_bits, d, d + len, d + 2 * len, dc, s);
    hm2.resize(len);
    fetch(hs, d, s);
    fetch(hq, d + len, s);
    fetch(hm2, d + 2 * len, s);
    fetch(hc, dc, s);
    SAPCA_HIP(hipStreamSynchronize(s));
  };
  if (direction == 0) {
    row_pass(A);
  } else if (k::exact_colstats_bytes<T>((int64_t)n) > ((size_t)1 << 30)) {
    row_pass(transpose_into_at(h, A));
  } else {
    const size_t work_bytes = (k::exact_colstats_bytes<T>((int64_t)n) + 255) / 256 * 256;
    char* base = h.batch_out.as<char>(work_bytes + 3 * n * sizeof(double));
    double* d_out = reinterpret_cast<double*>(base + work_bytes);
    k::exact_colstats_reset<T>(base, (int64_t)n, s);
    if (d_bits) k::exact_colstats_scan_rows<T>(A.ptr, A.val, (int64_t)m, d_bits, (int64_t)n, base, s);
    else k::exact_colstats_scan_values<T>(A.val, (int64_t)nnz, (int64_t)n, base, s);
    k::exact_colstats_add<T>(A.ptr, A.idx, A.val, 0, (int64_t)m, 0, (int64_t)nnz, (int64_t)n, base, s, d_bits);
    int nonfinite = 0;
    k::exact_colstats_finish<T>(base, (int64_t)n, d_out, &nonfinite, s);
    std::vector<double> host(3 * n);
    fetch(host, d_out, s);
    SAPCA_HIP(hipStreamSynchronize(s));
    for (uint64_t j = 0; j < n; ++j) {
      hs[j] = host[j];
      hq[j] = host[n + j];
      hc[j] = (uint32_t)host[2 * n + j];
    }
    if (nonfinite) {   // the columns whose kept entries hold an inf / nan take the f64 sums of the row pass on A^T
      const std::vector<double> es = hs, eq = hq;
      row_pass(transpose_into_at(h, A));
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
}

template <typename T>
void top_n(H& h, const CsrView<T>& A, const uint64_t* ns, uint32_t n_ns, double* out) {
  SAPCA_CHECK(n_ns > 0 && ns != nullptr, SAPCA_ERR_ARG, "sum_row_n_top: at least one n is needed");
  SAPCA_CHECK(out != nullptr || A.rows == 0, SAPCA_ERR_ARG, "null output");
  check_view(A);
  const uint64_t m = (uint64_t)A.rows;
  if (m == 0) return;
  hipStream_t s = h.stream;
  uint64_t* d_ns = h.batch_in.as<uint64_t>(n_ns);
  double* d_out = h.batch_out.as<double>((size_t)n_ns * m);
  SAPCA_HIP(hipMemcpyAsync(d_ns, ns, n_ns * sizeof(uint64_t), hipMemcpyHostToDevice, s));
  k::row_top_n(A, d_ns, (int)n_ns, d_out, s);
  SAPCA_HIP(hipMemcpyAsync(out, d_out, (size_t)n_ns * m * sizeof(double), hipMemcpyDeviceToHost, s));
  SAPCA_HIP(hipStreamSynchronize(s));
}

namespace {

// rows[0 .. n_rows) (host, every entry below A.rows) of A into the selection's buffers: the offsets through a scan (one
// synchronisation: the total sizes the output), then a fill balanced over output entries (select.hip)
template <typename T>
void gather_rows(H& h, const CsrView<T>& A, const uint64_t* rows, uint64_t n_rows, uint64_t* nnz_out, const int64_t** d_ptr,
                 const int32_t** d_idx, T** d_val) {
  H::Selection& sel = h.selection;
  hipStream_t s = h.stream;
  h.drop_preparation_of(sel);
  int64_t* o_ptr = sel.ptr.as<int64_t>(n_rows + 1);
  int64_t total = 0;
  const uint64_t* d_rows = nullptr;
  if (n_rows == 0) {
    SAPCA_HIP(hipMemsetAsync(o_ptr, 0, sizeof(int64_t), s));
  } else {
    uint64_t* dr = sel.rows.as<uint64_t>(n_rows);
    SAPCA_HIP(hipMemcpyAsync(dr, rows, n_rows * sizeof(uint64_t), hipMemcpyHostToDevice, s));
    d_rows = dr;
    k::select_rows_offsets(A.ptr, d_rows, (int64_t)n_rows, o_ptr, &total, sel.scan, s);
  }
  int32_t* o_idx = sel.idx.as<int32_t>(std::max<int64_t>(total, 1));
  T* o_val = sel.val.as<T>(std::max<int64_t>(total, 1));
  k::select_rows_fill(A, d_rows, (int64_t)n_rows, o_ptr, total, o_idx, o_val, s);
  SAPCA_HIP(hipStreamSynchronize(s));   // the arrays are complete when the call returns, whatever stream reads them next
  *nnz_out = (uint64_t)total;
  *d_ptr = o_ptr;
  *d_idx = o_idx;
  *d_val = o_val;
}

void check_row_list(const char* who, const uint64_t* rows, uint64_t n_rows, uint64_t m) {
  for (uint64_t j = 0; j < n_rows; ++j)
    if (rows[j] >= m)
      throw Error(SAPCA_ERR_ARG, std::string(who) + ": row index " + std::to_string(rows[j]) + " at position " + std::to_string(j) +
                                     " is out of range (m = " + std::to_string(m) + ")");
}

}  // namespace

// Rows `rows[0 .. n_rows)` of a device CSR (any order, repeats allowed) as a CSR in the handle's selection buffers.
// Everything that can be refused is refused before anything is enqueued or a buffer is touched.
template <typename T>
void select_rows(H& h, const CsrView<T>& A, const uint64_t* rows, uint64_t n_rows, uint64_t* nnz_out, const int64_t** d_ptr,
                 const int32_t** d_idx, T** d_val) {
  SAPCA_CHECK(nnz_out && d_ptr && d_idx && d_val, SAPCA_ERR_ARG, "select_rows: null output pointer");
  SAPCA_CHECK(rows != nullptr || n_rows == 0, SAPCA_ERR_ARG, "select_rows: rows is NULL with n_rows > 0");
  check_view(A);
  SAPCA_CHECK(n_rows < (1ull << 31), SAPCA_ERR_ARG, "more than 2^31-1 rows or columns is not supported");
  const H::Selection& sel = h.selection;
  SAPCA_CHECK(!sel.owns(A.ptr) && !sel.owns(A.idx) && !sel.owns(A.val), SAPCA_ERR_ARG,
              "select_rows: the source is this handle's own selection, which the call overwrites (select from the uploaded matrix)");
  check_row_list("select_rows", rows, n_rows, (uint64_t)A.rows);
  gather_rows(h, A, rows, n_rows, nnz_out, d_ptr, d_idx, d_val);
}

// A[rows][:, col_mask], optionally without stored zeros, in the same buffers (MaskedCSRMatrix::new's column compaction,
// sparse_masked/mod.rs:264-271, 455-466, fused with the row selection).  Without a mask that drops a column and without the
// flag it IS the row selection: the same launches, the same bytes.  Otherwise the gathered rows are never materialised:
// their offsets, a count per span of gathered positions, a scan (the one synchronisation: the total sizes the output) and
// the fill (select.hip).  Refusals come first, as above.
template <typename T>
void select_submatrix(H& h, const CsrView<T>& A, const uint64_t* rows, uint64_t n_rows, const uint8_t* col_mask, uint64_t mask_len,
                      uint32_t flags, uint64_t* n_cols_out, uint64_t* nnz_out, const int64_t** d_ptr, const int32_t** d_idx, T** d_val) {
  SAPCA_CHECK(n_cols_out && nnz_out && d_ptr && d_idx && d_val, SAPCA_ERR_ARG, "select_submatrix: null output pointer");
  SAPCA_CHECK((flags & ~(uint32_t)SAPCA_SELECT_DROP_STORED_ZEROS) == 0, SAPCA_ERR_ARG,
              "select_submatrix: unknown flag bits " + std::to_string(flags & ~(uint32_t)SAPCA_SELECT_DROP_STORED_ZEROS));
  check_view(A);
  SAPCA_CHECK(n_rows < (1ull << 31), SAPCA_ERR_ARG, "more than 2^31-1 rows or columns is not supported");
  H::Selection& sel = h.selection;
  SAPCA_CHECK(!sel.owns(A.ptr) && !sel.owns(A.idx) && !sel.owns(A.val), SAPCA_ERR_ARG,
              "select_submatrix: the source is this handle's own selection, which the call overwrites (select from the uploaded matrix)");
  const uint64_t m = (uint64_t)A.rows, n = (uint64_t)A.cols;
  if (rows == nullptr)
    SAPCA_CHECK(n_rows <= m, SAPCA_ERR_ARG,
                "select_submatrix: rows is NULL with n_rows = " + std::to_string(n_rows) + " > m = " + std::to_string(m));
  else
    check_row_list("select_submatrix", rows, n_rows, m);
  if (col_mask != nullptr && mask_len != n)
    throw Error(SAPCA_ERR_ARG, "select_submatrix: the column mask has " + std::to_string(mask_len) + " entries, the matrix " +
                                   std::to_string(n) + " columns");
  const bool drop_zeros = (flags & SAPCA_SELECT_DROP_STORED_ZEROS) != 0;
  // the column map of select.hip: a bit per column, and per 32 columns the kept ones before them
  const uint64_t words = (n + 31) / 32;
  std::vector<uint32_t> cmap;
  uint64_t kept = n;
  if (col_mask != nullptr) {
    cmap.assign(2 * words, 0u);
    kept = 0;
    for (uint64_t c = 0; c < n; ++c) {
      if ((c & 31) == 0) cmap[words + (c >> 5)] = (uint32_t)kept;
      if (col_mask[c]) {
        cmap[c >> 5] |= 1u << (c & 31);
        ++kept;
      }
    }
  }
  *n_cols_out = kept;
  if (kept == n && !drop_zeros) {   // nothing to filter: the row selection itself
    std::vector<uint64_t> all;
    if (rows == nullptr) {
      all.resize(n_rows);
      for (uint64_t j = 0; j < n_rows; ++j) all[j] = j;
      rows = all.data();
    }
    gather_rows(h, A, rows, n_rows, nnz_out, d_ptr, d_idx, d_val);   // (synchronises: `all` may go)
    return;
  }
  hipStream_t s = h.stream;
  h.drop_preparation_of(sel);
  int64_t* o_ptr = sel.ptr.as<int64_t>(n_rows + 1);
  const uint32_t* d_cmap = nullptr;
  if (kept < n) {
    uint32_t* dc = sel.cmap.as<uint32_t>(cmap.size());
    SAPCA_HIP(hipMemcpyAsync(dc, cmap.data(), cmap.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    d_cmap = dc;
  }
  // the gathered offsets: the source's own for rows 0 .. n_rows - 1
  const uint64_t* d_rows = nullptr;
  const int64_t* goff = A.ptr;
  int64_t gtotal = 0, total = 0;
  if (rows != nullptr && n_rows > 0) {
    uint64_t* dr = sel.rows.as<uint64_t>(n_rows);
    SAPCA_HIP(hipMemcpyAsync(dr, rows, n_rows * sizeof(uint64_t), hipMemcpyHostToDevice, s));
    d_rows = dr;
    int64_t* g = sel.gather.as<int64_t>(n_rows + 1);
    k::select_rows_offsets(A.ptr, d_rows, (int64_t)n_rows, g, &gtotal, sel.scan, s);
    goff = g;
  } else if (n_rows == m) {
    gtotal = A.nnz;
  } else if (n_rows > 0) {
    SAPCA_HIP(hipMemcpyAsync(&gtotal, A.ptr + n_rows, sizeof(int64_t), hipMemcpyDeviceToHost, s));
    SAPCA_HIP(hipStreamSynchronize(s));
  }
  int32_t* o_idx = nullptr;
  T* o_val = nullptr;
  if (n_rows == 0 || gtotal <= 0) {   // no entry to look at: every offset is 0
    SAPCA_HIP(hipMemsetAsync(o_ptr, 0, (n_rows + 1) * sizeof(int64_t), s));
    o_idx = sel.idx.as<int32_t>(1);
    o_val = sel.val.as<T>(1);
  } else {
    const int64_t spans = k::select_submatrix_spans(gtotal);
    int64_t* span = sel.spans.as<int64_t>(spans + 1);
    k::select_submatrix_count(A, d_rows, (int64_t)n_rows, goff, gtotal, d_cmap, drop_zeros, span, s);
    k::exclusive_scan_i64(span, spans + 1, sel.scan, 0, s);
    SAPCA_HIP(hipMemcpyAsync(&total, span + spans, sizeof(int64_t), hipMemcpyDeviceToHost, s));
    SAPCA_HIP(hipStreamSynchronize(s));
    o_idx = sel.idx.as<int32_t>(std::max<int64_t>(total, 1));
    o_val = sel.val.as<T>(std::max<int64_t>(total, 1));
    k::select_submatrix_fill(A, d_rows, (int64_t)n_rows, goff, gtotal, d_cmap, drop_zeros, span, o_ptr, o_idx, o_val, s);
  }
  SAPCA_HIP(hipStreamSynchronize(s));   // complete when the call returns; cmap may go
  *nnz_out = (uint64_t)total;
  *d_ptr = o_ptr;
  *d_idx = o_idx;
  *d_val = o_val;
}

// ---- the gate in front of the device entry points (canon.hip) ----------------------------------------------------------
namespace {

// The survey of an untrusted device CSR (rowsort.h) as a report; with_lists: the rows that need sorting are listed behind the
// check for canonicalize.  The counter block stays in h.canonical.sort.counters.
template <typename T>
sapca_csr_report run_check(H& h, const CsrView<T>& A, bool with_lists) {
  namespace K = sapca::k;
  const bool sound = h.canonical.sort.survey(A, with_lists, true, h.stream);
  const unsigned long long* c = h.canonical.sort.counters;
  const uint64_t none = UINT64_MAX;
  sapca_csr_report r{};
  r.struct_size = (uint32_t)sizeof(sapca_csr_report);
  r.first_bad_offset_row = c[K::kCtrFirstBadOffset];
  r.first_out_of_range_row = r.first_unsorted_row = r.first_duplicate_row = r.first_nonfinite_row = none;
  if (!sound) {
    r.flags = SAPCA_CSR_BAD_OFFSETS;
    return r;
  }
  r.cols_out_of_range = c[K::kCtrColsOutOfRange];
  r.first_out_of_range_row = c[K::kCtrFirstOutOfRange];
  r.unsorted_rows = c[K::kCtrUnsortedRows];
  r.first_unsorted_row = c[K::kCtrFirstUnsorted];
  r.duplicate_entries = c[K::kCtrDuplicates];
  r.first_duplicate_row = c[K::kCtrFirstDuplicate];
  r.nonfinite_values = c[K::kCtrNonfinite];
  r.first_nonfinite_row = c[K::kCtrFirstNonfinite];
  r.stored_zeros = c[K::kCtrStoredZeros];
  r.flags = (r.cols_out_of_range ? SAPCA_CSR_COL_RANGE : 0u) | (r.unsorted_rows ? SAPCA_CSR_UNSORTED : 0u) |
            (r.duplicate_entries ? SAPCA_CSR_DUPLICATES : 0u) | (r.nonfinite_values ? SAPCA_CSR_NONFINITE : 0u);
  return r;
}

// dst <- src, `bytes` of device memory on the stream: the 16-byte streaming copy where both ends allow it, the tail (and an
// unaligned source) through the runtime's copy
void device_copy(const void* src, void* dst, size_t bytes, hipStream_t s) {
  if (bytes == 0) return;
  size_t body = 0;
  if ((reinterpret_cast<uintptr_t>(src) & 15) == 0 && (reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
    body = bytes & ~(size_t)15;
    k::stream_copy16(src, dst, (int64_t)body, s);
  }
  if (body < bytes)
    SAPCA_HIP(hipMemcpyAsync(static_cast<char*>(dst) + body, static_cast<const char*>(src) + body, bytes - body, hipMemcpyDeviceToDevice, s));
}

}  // namespace

template <typename T>
void check(H& h, const CsrView<T>& A, sapca_csr_report* report) {
  SAPCA_CHECK(report != nullptr, SAPCA_ERR_ARG, "check_csr: null report");
  check_struct_size(report, "report", "sapca_csr_report", "check_csr");
  check_view(A);
  *report = run_check(h, A, false);
}

// Rows sorted by column, equal columns summed (canon.hip).  Everything that can be refused is refused before a canonical
// buffer is touched; a canonical input is handed back as it is.
template <typename T>
void canonicalize(H& h, const CsrView<T>& A, uint64_t* nnz_out, const int64_t** d_ptr, const int32_t** d_idx, T** d_val,
                  sapca_csr_report* report) {
  namespace K = sapca::k;
  SAPCA_CHECK(nnz_out && d_ptr && d_idx && d_val, SAPCA_ERR_ARG, "canonicalize: null output pointer");
  if (report) check_struct_size(report, "report", "sapca_csr_report", "canonicalize");
  check_view(A);
  const uint64_t m = (uint64_t)A.rows, n = (uint64_t)A.cols, nnz = (uint64_t)A.nnz;
  H::Canonical& can = h.canonical;
  SAPCA_CHECK(!can.owns(A.ptr) && !can.owns(A.idx) && !can.owns(A.val), SAPCA_ERR_ARG,
              "canonicalize: the source is this handle's own canonical result, which the call overwrites (it is canonical already)");
  sapca_csr_report r = run_check(h, A, true);
  if (r.flags & SAPCA_CSR_BAD_OFFSETS)
    throw Error(SAPCA_ERR_ARG, "canonicalize: the row offsets are broken at row " + std::to_string(r.first_bad_offset_row) +
                                   " (ptr[0] != 0, a decreasing offset, or ptr[m] != nnz): this cannot be repaired");
  if (r.flags & SAPCA_CSR_COL_RANGE)
    throw Error(SAPCA_ERR_ARG, "canonicalize: " + std::to_string(r.cols_out_of_range) + " column indices are out of range (n = " +
                                   std::to_string(n) + "), the first in row " + std::to_string(r.first_out_of_range_row) +
                                   ": this cannot be repaired");
  if ((r.flags & (SAPCA_CSR_UNSORTED | SAPCA_CSR_DUPLICATES)) == 0) {   // the common case: the check's one pass is all it costs
    *nnz_out = nnz;
    *d_ptr = A.ptr;
    *d_idx = A.idx;
    *d_val = const_cast<T*>(A.val);
    if (report) *report = r;
    return;
  }
  hipStream_t s = h.stream;
  h.drop_preparation_of(can);
  const int64_t rows = A.rows;
  int64_t* o_ptr = can.ptr.as<int64_t>(m + 1);
  int32_t* o_idx = can.idx.as<int32_t>(nnz);
  T* o_val = can.val.as<T>(nnz);
  device_copy(A.idx, o_idx, nnz * sizeof(int32_t), s);
  device_copy(A.val, o_val, nnz * sizeof(T), s);
  const uint64_t merged = can.sort.sort(A, o_idx, o_val, s);
  if (merged == 0) {   // the rows did not move: the offsets are the input's
    device_copy(A.ptr, o_ptr, (m + 1) * sizeof(int64_t), s);
  } else {
    can.sort.merged_offsets(A.ptr, rows, o_ptr, s);
    int32_t* f_idx = can.idx2.as<int32_t>(nnz - merged + 1);
    T* f_val = can.val2.as<T>(nnz - merged + 1);
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
}

#define SAPCA_INSTANTIATE_RESIDENT(T)                                                                                              \
  template void normalize<T>(H&, const CsrView<T>&, T*, const double*, uint64_t, double, int32_t);                                \
  template void log1p<T>(H&, uint64_t, T*);                                                                                        \
  template void stats<T>(H&, const CsrView<T>&, int32_t, double*, double*, uint64_t*, T*, T*);                                    \
  template void batch_stats<T>(H&, const CsrView<T>&, int32_t, const int32_t*, uint64_t, uint32_t, double*, double*, uint64_t*);  \
  template void masked_stats<T>(H&, const CsrView<T>&, int32_t, const uint8_t*, uint64_t, double*, double*, uint64_t*, double*);  \
  template void top_n<T>(H&, const CsrView<T>&, const uint64_t*, uint32_t, double*);                                               \
  template void select_rows<T>(H&, const CsrView<T>&, const uint64_t*, uint64_t, uint64_t*, const int64_t**, const int32_t**, T**); \
  template void select_submatrix<T>(H&, const CsrView<T>&, const uint64_t*, uint64_t, const uint8_t*, uint64_t, uint32_t, uint64_t*, \
                                    uint64_t*, const int64_t**, const int32_t**, T**);                                             \
  template void check<T>(H&, const CsrView<T>&, sapca_csr_report*);                                                                \
  template void canonicalize<T>(H&, const CsrView<T>&, uint64_t*, const int64_t**, const int32_t**, T**, sapca_csr_report*);
SAPCA_INSTANTIATE_RESIDENT(float)
SAPCA_INSTANTIATE_RESIDENT(double)
#undef SAPCA_INSTANTIATE_RESIDENT

// ---- sapca_knn_device_*: the exact k-nearest neighbours of device-resident score rows (the kernels are knn.hip's) --------
// Everything that can be refused is refused before anything is enqueued or a buffer is touched.
template <typename T>
void knn(H& h, uint64_t mq, const T* dq, uint64_t ldq, uint64_t mc, const T* dc, uint64_t ldc, uint64_t d, int32_t metric,
         uint32_t n_neighbors, uint32_t flags, int32_t* d_indices, T* d_values) {
  SAPCA_CHECK(metric == SAPCA_KNN_EUCLIDEAN || metric == SAPCA_KNN_COSINE || metric == SAPCA_KNN_PEARSON, SAPCA_ERR_ARG,
              "knn: unknown metric " + std::to_string(metric) + " (0 EUCLIDEAN, 1 COSINE, 2 PEARSON)");
  SAPCA_CHECK((flags & ~(uint32_t)SAPCA_KNN_EXCLUDE_SELF) == 0, SAPCA_ERR_ARG,
              "knn: unknown flag bits " + num(flags & ~(uint32_t)SAPCA_KNN_EXCLUDE_SELF));
  const bool exclude_self = (flags & SAPCA_KNN_EXCLUDE_SELF) != 0;
  SAPCA_CHECK(n_neighbors != 0, SAPCA_ERR_ARG, "knn: n_neighbors is 0");
  SAPCA_CHECK(n_neighbors <= SAPCA_KNN_MAX_NEIGHBORS, SAPCA_ERR_ARG,
              "knn: n_neighbors = " + num(n_neighbors) + " exceeds SAPCA_KNN_MAX_NEIGHBORS = " + num(SAPCA_KNN_MAX_NEIGHBORS));
  check_panel_width(d, "knn");
  check_stride_covers(d, ldq, "ldq", "knn");
  check_stride_covers(d, ldc, "ldc", "knn");
  check_stride_limit(ldq < (1ull << 28) ? ldc : ldq, "knn");   // (the first of the two that is too long)
  SAPCA_CHECK(mc < (1ull << 31), SAPCA_ERR_ARG, "knn: mc = " + num(mc) + " corpus rows; 2^31 or more are not supported");
  SAPCA_CHECK(mq < (1ull << 31), SAPCA_ERR_ARG, "knn: mq = " + num(mq) + " query rows; 2^31 or more are not supported");
  if ((uint64_t)n_neighbors + (exclude_self ? 1 : 0) > mc)
    throw Error(SAPCA_ERR_ARG, "knn: n_neighbors = " + num(n_neighbors) + " exceeds the " + num(mc - (exclude_self && mc ? 1 : 0)) +
                                   " corpus rows a query can have (mc = " + num(mc) + (exclude_self ? ", itself excluded)" : ")"));
  if (mq == 0) return;   // valid, nothing is read or written: no pointer is looked at
  SAPCA_CHECK(dc != nullptr, SAPCA_ERR_ARG, "knn: d_corpus is NULL with mc = " + num(mc));
  SAPCA_CHECK(dq != nullptr, SAPCA_ERR_ARG, "knn: d_queries is NULL with mq = " + num(mq));
  SAPCA_CHECK(d_indices != nullptr && d_values != nullptr, SAPCA_ERR_ARG, "knn: a NULL output with mq = " + num(mq));

  hipStream_t s = h.stream;
  const int nn = (int)n_neighbors, dd = (int)d;
  const k::KnnPlan plan = k::knn_plan<T>((int64_t)mq, (int64_t)mc, nn, cu_count(h));
  H::Knn& w = h.knn;
  // prepare: what the ranking s(i, j) = alpha <a_i, b_j> + bias_j runs on
  const T *sq = dq, *sc = dc, *bias = nullptr;
  int64_t sldq = (int64_t)ldq, sldc = (int64_t)ldc;
  if (metric == SAPCA_KNN_EUCLIDEAN) {
    T* b = w.bias.as<T>(mc);
    k::knn_prepare<T>(dc, (int64_t)ldc, (int64_t)mc, dd, metric, nullptr, b, s);
    bias = b;
  } else {
    T* uc = w.unit_c.as<T>(mc * d);
    k::knn_prepare<T>(dc, (int64_t)ldc, (int64_t)mc, dd, metric, uc, nullptr, s);
    sc = uc;
    sldc = dd;
    if (dq == dc && ldq == ldc && mq == mc) {   // neighbours within one panel: one set of unit rows
      sq = uc;
    } else {
      T* uq = w.unit_q.as<T>(mq * d);
      k::knn_prepare<T>(dq, (int64_t)ldq, (int64_t)mq, dd, metric, uq, nullptr, s);
      sq = uq;
    }
    sldq = dd;
  }
  const size_t lists = (size_t)mq * plan.nsplit * nn;
  T* part_sc = w.part_sc.as<T>(lists);
  int32_t* part_ix = w.part_ix.as<int32_t>(lists);
  k::knn_select<T>(sq, sldq, (int64_t)mq, sc, sldc, (int64_t)mc, bias, dd, metric, nn, exclude_self, plan, part_sc, part_ix, s);
  const int32_t* sel = part_ix;
  if (plan.nsplit > 1) {
    int32_t* merged = w.merged.as<int32_t>((size_t)mq * nn);
    k::knn_merge<T>(part_sc, part_ix, (int64_t)mq, plan.nsplit, nn, merged, s);
    sel = merged;
  }
  // refine: the values from the rows as the caller gave them
  k::knn_refine<T>(dq, (int64_t)ldq, (int64_t)mq, dc, (int64_t)ldc, (int64_t)mc, dd, metric, sel, nn, nn, d_indices, d_values, s);
  SAPCA_HIP(hipStreamSynchronize(s));   // the outputs are complete when the call returns, whatever stream reads them next
}

template void knn<float>(H&, uint64_t, const float*, uint64_t, uint64_t, const float*, uint64_t, uint64_t, int32_t, uint32_t, uint32_t,
                         int32_t*, float*);
template void knn<double>(H&, uint64_t, const double*, uint64_t, uint64_t, const double*, uint64_t, uint64_t, int32_t, uint32_t, uint32_t,
                          int32_t*, double*);

}  // namespace resident
}  // namespace sapca
