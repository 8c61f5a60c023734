// Launchers of the hand-written gfx950 kernels.  Everything takes device pointers and a
// stream; nothing here allocates except through the DevBuf scratch arguments.
#pragma once
#include <vector>
#include "common.h"

namespace sapca {
namespace k {

// How the producer of a panel left it: P = sum of nsplit slabs (slab sp at parts + sp * slab_stride, row stride = the panel's)
// minus the centring term mu sv^T (mu per row, sv per column; null: none).  gram() applies it on its way through the panel
// and writes P; materialize() only writes P.  parts may be P itself (nsplit = 1).
template <typename T>
struct PanelSource {
  const T* parts = nullptr;
  int nsplit = 0;
  int64_t slab_stride = 0;
  const T* mu = nullptr;
  const T* sv = nullptr;
};

// ---- prep.hip --------------------------------------------------------------------------
// nalgebra's usize indices -> int64 row offsets + int32 column indices; *flag |= 1 on col >= n.
void narrow_indices(const uint64_t* ptr64, const uint64_t* idx64, int64_t m, int64_t nnz, int64_t n,
                    int64_t* ptr, int32_t* idx, int* flag, hipStream_t s);
// CSR(A) -> CSR(A^T), entries of each A^T row in ascending A-row order (stable, deterministic).
template <typename T>
void transpose_csr(const CsrView<T>& A, int64_t* t_ptr, int32_t* t_idx, T* t_val, DevBuf& scratch, hipStream_t s,
                   int tile_major_nct = 0,   // f32, > 1: entries of a transposed row ordered by (row mod nct, row / nct)
                   const uint64_t** packed_rows_out = nullptr);   // with tile_major_nct: leave the rows packed as
                                                                   // (row << 32 | value bits) in `scratch`, skip t_idx / t_val
void unpack_transposed(const uint64_t* packed, int64_t nnz, int32_t* t_idx, float* t_val, hipStream_t s);
// Row sums of a CSR (applied to A^T: the reference's sum_col / sum_col_squared), f64 accumulation.
template <typename T>
void row_sums(const CsrView<T>& At, double* sum, double* sumsq, hipStream_t s);
// Mask compaction of A: keep entries with o2m[col] >= 0, renumbered.  Two passes around a scan.
template <typename T>
void compact_columns(const CsrView<T>& A, const int32_t* o2m, int64_t* new_ptr, int32_t* new_idx, T* new_val,
                     int64_t* new_nnz_host, DevBuf& scratch, hipStream_t s, int32_t* drop_col = nullptr, T* drop_val = nullptr,
                     unsigned long long* amax_bits = nullptr);
// (amax_bits: receives the bit pattern of max |value| over ALL stored entries of A as a double, a quiet nan's if one is not finite)
// (drop_col / drop_val, A.nnz each, receive the entries that were NOT kept as (original column, value) pairs, row after row)
// sum[c], sumsq[c] (c < n) over (column, value) pairs through a stable sort by column; seg (n + 1), keys_out, vals_out: work arrays
template <typename T>
void sums_by_column(const int32_t* cols, const T* vals, int64_t count, int64_t n, int64_t* seg, int32_t* keys_out, T* vals_out,
                    double* sum, double* sumsq, DevBuf& scratch, hipStream_t s);
// Exact, order-independent column statistics of a CSR whose entries land chunk by chunk (upstats.hip).  `work` holds the
// long accumulators.  scan_values (once all values are on the device) fixes the limb window kept in LDS; add takes the
// entries [e_lo, e_hi) of rows [r_lo, r_hi); finish writes out[0..n) = sum, out[n..2n) = sum of squares, out[2n..3n) =
// stored-entry count, each the correctly rounded exact value, and copies the "a value was inf/nan" flag to the host
// asynchronously.  row_bits (device bitset over the rows, may be null): add takes only the rows whose bit is set, and reads
// nothing of the others.
template <typename T> size_t exact_colstats_bytes(int64_t n);
template <typename T> void exact_colstats_reset(void* work, int64_t n, hipStream_t s);
template <typename T> void exact_colstats_scan_values(const T* val, int64_t count, int64_t n, void* work, hipStream_t s);
// (scan_values restricted to the stored values of the rows whose bit is set in row_bits: the window of a row-masked add)
template <typename T>
void exact_colstats_scan_rows(const int64_t* ptr, const T* val, int64_t rows, const uint32_t* row_bits, int64_t n, void* work,
                              hipStream_t s);
template <typename T>
void exact_colstats_add(const int64_t* ptr, const int32_t* idx, const T* val, int64_t r_lo, int64_t r_hi, int64_t e_lo, int64_t e_hi,
                        int64_t n, void* work, hipStream_t s, const uint32_t* row_bits = nullptr);
template <typename T> void exact_colstats_finish(void* work, int64_t n, double* out, int* nonfinite_host, hipStream_t s);
// out_a[where[j]] = a[where[j]], out_b[where[j]] = b[where[j]]   (the selected positions of two full-width arrays)
void copy_selected(const double* a, const double* b, const int32_t* where, int64_t count, double* out_a, double* out_b, hipStream_t s);
// out_a[where[j]] = a[j], out_b[where[j]] = b[j]   (column statistics from a compacted numbering back to the full width)
void scatter_pairs(const double* a, const double* b, const int32_t* where, int64_t count, double* out_a, double* out_b, hipStream_t s);
// mu[j] = T(sum[sel ? sel[j] : j] / count): the column means the sweeps centre with, from the device-side column sums
template <typename T>
void mean_from_sums(const double* sum, double count, const int32_t* sel, int64_t n_used, T* mu, hipStream_t s);
// out[r] = ptr[r+1] - ptr[r] as f64 (column counts when applied to A^T's row offsets)
void row_lengths_f64(const int64_t* ptr, int64_t rows, double* out, hipStream_t s);
// out[j] = number of stored entries with column j (integer atomics; transform of a matrix that
// was not the fitted one)
void column_counts_f64(const int32_t* idx, int64_t nnz, int64_t n, double* out, DevBuf& scratch, hipStream_t s);

// ---- preproc.hip (preprocessing and statistics on a device-resident CSR) ----------
// Normalize<T> for CsrMatrix (csr.rs:1012-1066): values *= target / sums[row or column] where the sum is > 0.
// d_sums: device, length rows or cols; d_scale: device scratch of the same length.
template <typename T>
void normalize_csr(const CsrView<T>& A, T* values, const double* d_sums, double target, bool by_column, double* d_scale,
                   hipStream_t s);
// Log1P (csr.rs:1069-1078): values = ln(1 + values): the sum in T, the logarithm in f64 and rounded once to T.
template <typename T>
void log1p_values(T* values, int64_t nnz, hipStream_t s);
// sum_row, sum_row_squared, min_max_row of a CSR (applied to A^T: the column versions); any output may be null.
// from_first_value: a row's min and max start from its first stored value (min_max_row_chunk); otherwise from
// (MAX, -MAX) (min_max_col_chunk, for the rows of A^T).  A NaN never wins a comparison in either.
template <typename T>
void row_stats(const CsrView<T>& A, bool from_first_value, double* sum, double* sumsq, T* minv, T* maxv, hipStream_t s);

// ---- batchstats.hip: per-batch statistics and top-n row sums (BatchMatrixVariance / BatchMatrixMean / MatrixNTop) ------
// the most codes one batch_row_stats launch takes (its LDS budget)
int batch_codes_per_launch();
// Per row r of R and code b in [lo, lo + nb), over the stored entries e of row r with codes[R.idx[e]] == lo + b:
// cnt[b * R.rows + r] = their count, sum[..] = their sum, m2[..] = sum (x - sum / count)^2 (two passes, f64).
template <typename T>
void batch_row_stats(const CsrView<T>& R, const int32_t* codes, int lo, int nb, double* sum, double* m2, uint32_t* cnt, hipStream_t s);
// out[i * A.rows + r] = sum of the min(ns[i], length of row r) largest stored values of row r (f64); ns: device, n_ns
template <typename T>
void row_top_n(const CsrView<T>& A, const uint64_t* ns, int n_ns, double* out, hipStream_t s);

// ---- rankgroups.hip: the rank pass of sapca_rank_sums_csr_device_* / sapca_rank_groups_csr_device_* (classes: rankgroups.h) ----
// group[b] = the labels equal to b, b < nk (device, zeroed here; labels outside [0, nk) are skipped)
void rank_group_sizes(const int32_t* labels, int64_t m, int nk, unsigned long long* group, hipStream_t s);
// cnt[b * At.rows + j] = the stored non-zero entries of row j of At whose row of A carries label b (no sort: the counts alone)
template <typename T>
void rank_count_nonzero(const CsrView<T>& At, const int32_t* labels, int nk, uint32_t* cnt, hipStream_t s);
// Per row j of At (a column of A) of stored length <= kRankLdsMax: rs[b * At.rows + j] = twice the rank sum of group b among the
// M included rows (M = sum of group[]), cnt[..] as above, tie[j] = sum over tie runs of t^3 - t, the zero block included.
template <typename T>
void rank_sums_lds(const CsrView<T>& At, const int32_t* labels, int nk, const unsigned long long* group, int64_t M, long long* rs,
                   uint32_t* cnt, double* tie, hipStream_t s);
// The same for the nseg longer rows cols_list[0 .. nseg) (device), row cols_list[i] at seg[i] .. seg[i + 1] (device, nseg + 1,
// seg[0] = 0, seg[nseg] = total) of the key scratch: build, segmented radix sort, walk.  `scratch` grows to what `total` needs.
template <typename T>
void rank_sums_long(const CsrView<T>& At, const int32_t* labels, int nk, const unsigned long long* group, int64_t M,
                    const int32_t* cols_list, const uint32_t* seg, int nseg, uint32_t total, DevBuf& scratch, long long* rs, uint32_t* cnt,
                    double* tie, hipStream_t s);

// ---- hvg.hip: variable genes (sapca_hvg_moments_csr_device_*, sapca_loess_f64, sapca_hvg_csr_device_*) ----
constexpr int kHvgPlain = -1;   // the untransformed moments of the chain's first pass (beside SAPCA_HVG_CLIP / SAPCA_HVG_EXPM1)
// Per row j of At (a column of A), over its stored entries whose row of A is included: sum[j] / sumsq[j] of f(x) in f64 and
// n_clipped[j] (may be null) = the entries with x > d_clip[j] (CLIP only; d_clip: device, At.rows).  labels null: every row;
// batch >= 0: the rows with labels[r] == batch; batch < 0: the rows with a label in [0, nk).  A column's entries are summed
// in stored order by a fixed lane assignment and butterfly: deterministic, no atomic.
template <typename T>
void hvg_moments(const CsrView<T>& At, const int32_t* labels, int32_t batch, int nk, int transform, const double* d_clip, double* sum,
                 double* sumsq, uint32_t* n_clipped, hipStream_t s);
// Local quadratic regression (the header's definition) of y on x over the nv smallest of the n abscissae x (the others must be
// +inf), window q <= nv: fit[j] is written for those nv points and left alone for the rest.  xs, ys (f64, n), iota, perm (u32, n):
// work arrays; sort_tmp grows to what the sort needs.
void hvg_loess(const double* x, const double* y, int64_t n, int64_t nv, int64_t q, double* xs, double* ys, uint32_t* iota, uint32_t* perm,
               double* fit, DevBuf& sort_tmp, hipStream_t s);
// The n-sized steps of the seurat_v3 chain, N the batch's rows: mean and ddof-1 variance from s / ss with the loess
// coordinates (lx = +inf where var <= 0) and *n_valid = the columns with var > 0; reg_std and clip from the estimate;
// norm_var from the clipped moments.
void hvg_mean_var(const double* s_, const double* ss, double N, int64_t n, double* mean, double* var, double* lx, double* ly,
                  uint32_t* n_valid, hipStream_t s);
void hvg_clip(const double* est, const double* mean, double N, int64_t n, double* reg_std, double* clip, hipStream_t s);
void hvg_norm_var(const double* s_, const double* ss, const double* mean, const double* reg_std, double N, int64_t n, double* norm_var,
                  hipStream_t s);

// ---- maskedstats.hip: masked and stored-entry statistics (MatrixSum / MatrixNonZero / MatrixVariance *_masked, *_chunk) ----
// Per row r of A, over its stored entries e whose column's bit (col_bits[c / 32] >> c % 32) & 1 is set (all of them when
// col_bits is null): cnt[r] = their count, sum[r] / sumsq[r] = their sum / sum of squares, m2[r] = sum (x - sum / cnt)^2
// (two passes, f64).  Any output may be null.
template <typename T>
void masked_row_stats(const CsrView<T>& A, const uint32_t* col_bits, double* sum, double* sumsq, double* m2, uint32_t* cnt,
                      hipStream_t s);

// ---- select.hip: rows of a CSR, in any order and with repeats, as a new CSR (sapca_select_rows_csr_device_*) ----------
// data[0 .. count) <- its exclusive prefix sums, in place (prep.hip); work space from `scratch` at scratch_offset
void exclusive_scan_i64(int64_t* data, int64_t count, DevBuf& scratch, size_t scratch_offset, hipStream_t s,
                        int64_t* out = nullptr);   // (out: the offsets go there and data stays; null: in place)
// out_ptr[0 .. n_rows] = the offsets of the selection (row i = source row rows[i]; rows: device, every entry below the source's
// row count); *total_host = out_ptr[n_rows], on the host when the call returns (one synchronisation, like compact_columns)
void select_rows_offsets(const int64_t* ptr, const uint64_t* rows, int64_t n_rows, int64_t* out_ptr, int64_t* total_host,
                         DevBuf& scratch, hipStream_t s);
// out_idx / out_val[out_ptr[i] ..) = the entries of row rows[i] of A in stored order, values bit for bit; out_idx and out_val
// are 16-byte aligned and do not overlap A.  A workgroup per span of output positions (kSelectSpan), no atomics.
template <typename T>
void select_rows_fill(const CsrView<T>& A, const uint64_t* rows, int64_t n_rows, const int64_t* out_ptr, int64_t total,
                      int32_t* out_idx, T* out_val, hipStream_t s);

// Rows AND columns (sapca_select_submatrix_csr_device_*): the gathered rows -- goff (n_rows + 1) their offsets, gtotal =
// goff[n_rows]; rows null: source rows 0 .. n_rows - 1, goff = A.ptr -- filtered by a column map and / or without stored zeros.
// cmap (device, null: every column): bits[words] | before[words], words = ceil(A.cols / 32): bit c % 32 of bits[c / 32] is
// set where column c is kept, before[w] = the kept columns below 32 w.  A workgroup per span of gathered positions:
// select_submatrix_spans(gtotal) of them.  count: span_cnt[0 .. spans) = the kept entries of each span, span_cnt[spans] = 0;
// after exclusive_scan_i64 over all spans + 1 the same array is the fill's span_base.  fill: out_ptr[0 .. n_rows], and the
// kept entries in gathered order at out_idx / out_val, columns renumbered by rank, values bit for bit.  No atomics.
int64_t select_submatrix_spans(int64_t gtotal);
template <typename T>
void select_submatrix_count(const CsrView<T>& A, const uint64_t* rows, int64_t n_rows, const int64_t* goff, int64_t gtotal,
                            const uint32_t* cmap, bool drop_zeros, int64_t* span_cnt, hipStream_t s);
template <typename T>
void select_submatrix_fill(const CsrView<T>& A, const uint64_t* rows, int64_t n_rows, const int64_t* goff, int64_t gtotal,
                           const uint32_t* cmap, bool drop_zeros, const int64_t* span_base, int64_t* out_ptr, int32_t* out_idx,
                           T* out_val, hipStream_t s);

// ---- canon.hip: check and canonicalise a device CSR (sapca_check_csr_device_*, sapca_canonicalize_csr_device_*) ----------
// slots of the 64-bit counter block `ctr` (device, kCtrSlots words): first rows (start at all bits set), then counts
enum CanonCtr {
  kCtrFirstBadOffset = 0, kCtrFirstOutOfRange, kCtrFirstUnsorted, kCtrFirstDuplicate, kCtrFirstNonfinite, kCtrFirstCount,
  kCtrColsOutOfRange = kCtrFirstCount, kCtrUnsortedRows, kCtrDuplicates, kCtrNonfinite, kCtrStoredZeros,
  kCtrListWave, kCtrListLds, kCtrListLong,   // rows listed per length class (canon_list_rows)
  kCtrLongEntries,                           // entries of the rows of the last class: the key work space they need
  kCtrMerged,                                // entries that merged into a predecessor of equal column (canon_sort_rows)
  kCtrSlots = 16
};
// resets ctr and checks ptr[0] == 0, ptr[r + 1] >= ptr[r], ptr[m] == nnz: ctr[kCtrFirstBadOffset] = the first r that fails
// (m for the last test).  Reads ptr[0 .. m] and nothing else.
void canon_check_offsets(const int64_t* ptr, int64_t m, int64_t nnz, unsigned long long* ctr, hipStream_t s);
// one pass over the entries of A (offsets sound): the counters above, and row_bits[r] (A.rows words, cleared here) |= 1 where
// row r has an entry whose column is below its predecessor's, |= 2 where one equals its predecessor's
template <typename T>
void canon_check_entries(const CsrView<T>& A, uint32_t* row_bits, unsigned long long* ctr, hipStream_t s);
// rows with row_bits != 0 -> lists[c * m ..) for length class c (0: <= 64 entries, 1: <= canon_lds_cap(), 2: longer),
// counted in ctr[kCtrListWave + c]; long_off[j] = where the j-th row of class 2 keeps its keys (ctr[kCtrLongEntries] in all)
void canon_list_rows(const int64_t* ptr, const uint32_t* row_bits, int64_t m, uint32_t* lists, unsigned long long* long_off,
                     unsigned long long* ctr, hipStream_t s);
int64_t canon_lds_cap();
// the listed rows of A, sorted by (column, stored position), into out_idx / out_val at A's offsets (values gathered from A,
// which the outputs must not overlap); distinct[r] = the row's distinct columns; ctr[kCtrMerged] += length - distinct
template <typename T>
void canon_sort_rows(const CsrView<T>& A, const uint32_t* lists, const unsigned long long* long_off, const int64_t counts[3],
                     unsigned long long* key_space, int32_t* out_idx, T* out_val, uint32_t* distinct, unsigned long long* ctr,
                     hipStream_t s);
// new_ptr[r] = row_bits[r] ? distinct[r] : ptr[r + 1] - ptr[r], new_ptr[m] = 0 (exclusive_scan_i64 makes offsets of them)
void canon_new_lengths(const int64_t* ptr, const uint32_t* row_bits, const uint32_t* distinct, int64_t m, int64_t* new_ptr,
                       hipStream_t s);
// (idx, val) at offsets ptr, every row sorted -> (out_idx, out_val) at new_ptr: a run of equal columns becomes one entry, its
// value the run's sum added left to right in T; an entry that does not merge keeps its bit pattern
template <typename T>
void canon_merge_fill(const int64_t* ptr, const int32_t* idx, const T* val, int64_t m, const int64_t* new_ptr, int32_t* out_idx,
                      T* out_val, hipStream_t s);

// dst[0 .. bytes) = src[0 .. bytes) by a 16-byte-per-lane streaming kernel (the attainable-HBM-rate probe of sapca_measure_copy_gbs)
void stream_copy16(const void* src, void* dst, int64_t bytes, hipStream_t s);

// ---- spmm.hip --------------------------------------------------------------------------
// Y[r][j] = sum_e val_e X[col_e][j] - cvec[j]   for j < ncols; X has leading dimension ldx
// (multiple of 16/sizeof(T)... see spmm.hip), Y leading dimension ldy.  cvec may be null.
// keep (nullable): a staged sweep whose tile range is split over workgroups may leave its partial slabs unsummed and describe
// them there (nsplit > 1; the caller's next pass over Y -- gram() -- sums them); otherwise keep = {Y, 1, 0}.  Only with cvec null.
template <typename T>
void spmm(const CsrView<T>& A, const TiledOp* tiled, const T* X, int ldx, T* Y, int ldy, int ncols,
          const T* cvec, int variant, DevBuf& scratch, hipStream_t s, PanelSource<T>* keep = nullptr);

// Y[r][j] = sum over the stored entries of row r of (value - shift[column]) X[column][j]   (quirk Q3 through the row kernel)
template <typename T>
void spmm_rows_shifted(const CsrView<T>& A, const T* X, int ldx, T* Y, int ldy, int ncols, const T* shift, hipStream_t s);

// ---- scatter.hip: column-wise reductions of a CSR without its transpose (fixed-point sums in LDS) ----------
bool scatter_fits(int64_t cols);   // one output vector of `cols` 64-bit words fits a workgroup's LDS
// *out_bits = bit pattern of max |v| as a double (a quiet NaN's pattern if any value is inf / nan)
template <typename T>
void absmax(const T* v, int64_t count, unsigned long long* out_bits, hipStream_t s);
// *out_bits = max(*out_bits, max |y|): the slot must have been cleared
void vecmax(const double* y, int64_t len, unsigned long long* out_bits, hipStream_t s);
// z = A^T y  (A: rows x cols, cols fitting LDS).  amax_bits / ymax_bits: max |a|, max |y| (the fixed-point scale follows from
// them); clear_bits (nullable): a slot to reset to 0 for the next product.  idx16 (nullable): 2-byte copy of A.idx.
template <typename T>
void spmvt_scatter(const CsrView<T>& A, const uint16_t* idx16, const double* y, const unsigned long long* amax_bits,
                   const unsigned long long* ymax_bits, unsigned long long* clear_bits, double* z, DevBuf& scratch, hipStream_t s);
// sum[c], sumsq[c], cnt[c] (nullable) of every column of A in ceil(cols / 7680) passes over the matrix
template <typename T>
void colstats_scatter(const CsrView<T>& A, const unsigned long long* amax_bits, double* sum, double* sumsq, double* cnt, DevBuf& scratch,
                      hipStream_t s);

// ---- tiled_build.hip: builders of the tile-major "quad" format the staged sweeps read ---------------------------
// Where the rows of the operator come from, which decides the builder's route.
struct AtDirectSrc;   // (tiled_build.hip: what build_tiled_at_direct hands the builder)
struct QuadSource {
  enum Kind {
    Csr,               // S is a CSR with ascending columns
    TileMajorCsr,      // S's rows were produced by transpose_csr(..., tile_major_nct = tiled_tile_count(S.cols, ldp))
    TileMajorPacked,   // ... and left packed: S.idx / S.val are not filled, `packed` holds (row << 32 | value bits); f32 only
    FromA              // A^T straight from A: build_tiled_at_direct's own
  };
  Kind kind = Csr;
  const uint64_t* packed = nullptr;
  bool seg_ready = false;                // TileMajorPacked: buf.seg already holds the per-row tile index (at_stats_index)
  const AtDirectSrc* from_a = nullptr;   // FromA
  static QuadSource csr() { return QuadSource(); }
  static QuadSource tile_major() {
    QuadSource q;
    q.kind = TileMajorCsr;
    return q;
  }
  static QuadSource tile_major_packed(const uint64_t* packed, bool seg_ready) {
    QuadSource q;
    q.kind = TileMajorPacked;
    q.packed = packed;
    q.seg_ready = seg_ready;
    return q;
  }
};
// Builds the tile-major format of an f32 operator for panels of leading dimension ldp (64).
// Returns false (op.valid == false) when the operator is outside the route's limits or does not fit the LDS staging;
// callers then stay on the row kernel.  Synchronises with the host (the entry counts come back).
bool build_tiled(const CsrView<float>& S, int ldp, TiledOp& op, TiledBuffers& buf, hipStream_t s, const QuadSource& src);
// The same format with f64 values for panels of 64 f64 columns (512-byte rows: the tile geometry of the
// 128-float panels); from a CSR (LDS-staged fill, direct scatter as the fallback) or a tile-major CSR (streaming fill).
bool build_tiled(const CsrView<double>& S, int ldp, TiledOp& op, TiledBuffers& buf, hipStream_t s, const QuadSource& src);
// The format of A^T (op: A.cols x A.rows) straight from A, without a transposed CSR: a histogram per (tile of A rows,
// column), a scatter of A's entries into per-chunk buckets, one workgroup per chunk for the format.  Byte-identical to
// build_tiled on the tile-major transposition.  at_ptr (A.cols + 1) receives A^T's row offsets, stats (2 * A.cols, may
// be null) the column sums and sums of squares of A, added per tile and then in tile order.  Returns false (nothing
// usable built) when the operator is outside this route's limits: the caller transposes instead.
bool build_tiled_at_direct(const CsrView<float>& A, int ldp, TiledOp& op, TiledBuffers& buf, int64_t* at_ptr, double* stats,
                           DevBuf& scratch, hipStream_t s);
// Column statistics of A (row sums / sums of squares of the packed tile-major A^T rows, same summation order as
// row_sums) and, in the same pass, the per-row tile index build_tiled(..., QuadSource::tile_major_packed(packed, true)) needs.
void at_stats_index(const int64_t* ptr, const uint64_t* packed, int64_t rows, int64_t cols, int ldp, TiledBuffers& buf,
                    double* sum, double* sumsq, hipStream_t s);
// number of interleaved column tiles the format uses for an operator with `cols` columns
int tiled_tile_count(int64_t cols, int ldp);

// ---- spmm_tiled.hip: the staged-entry sweep over that format, and the dispatch to the DPP-fed one (spmm_dq.hip) ----
void spmm_tiled(const TiledOp& op, const float* X, int ldx, float* Y, int ldy, int ncols, const float* cvec, DevBuf& scratch,
                hipStream_t s, PanelSource<float>* keep = nullptr);
// the DPP-fed sweep in pieces of its output rows (spmm_tiled.hip): can the operator be swept so, the pieces' row bounds, one piece
bool spmm_tiled_pieces_ok(const TiledOp& op, int npieces, int ldx);
void spmm_tiled_piece_bounds(const TiledOp& op, int npieces, std::vector<int64_t>& bounds, hipStream_t s);
void spmm_tiled_piece(const TiledOp& op, int piece, int npieces, int wgs, int64_t first_row, int64_t row_count, const float* X, int ldx, float* Y,
                      int ldy, int ncols, DevBuf& scratch, hipStream_t s);
void spmm_tiled(const TiledOp& op, const double* X, int ldx, double* Y, int ldy, int ncols, const double* cvec, DevBuf& scratch,
                hipStream_t s, PanelSource<double>* keep = nullptr);

// ---- the dense panel units (dense_common.h: what they share) ---------------------------
// widest panel (n_components + n_oversamples, padded) the dense kernels take: up to 128 columns in one launch, beyond that in
// blocks of 64 / 128 columns (correct, not tuned)
constexpr int kMaxPanelWidth = 1024;

// ---- gram.hip ----
// G = P^T P (ld x ld, f64, full symmetric) for a rows x ld panel with ld % 16 == 0 (ld <= 128) or ld % 64 == 0 (ld <= 1024).
template <typename T>
void materialize(T* P, int64_t rows, int ld, const PanelSource<T>& src, hipStream_t s);
// wsum (nullable, ld doubles): sum_r w[r] P[r][:] of the same pass (w null: ones)
template <typename T>
void gram(T* P, int64_t rows, int ld, double* G, DevBuf& scratch, hipStream_t s, const PanelSource<T>* src = nullptr, const T* w = nullptr,
          double* wsum = nullptr);
// ---- chol.hip ----
// Upper Cholesky G = R^T R on the leading l x l block, Rinv = R^{-1}; both ld x ld, zero padded.
// *info += number of pivots that had to be regularised.
// wsum / vec32 / vec64 (nullable): vec[j] = sum_i Rinv[i][j] wsum[i] -- the column sums of P R^-1 from those of P
void chol_inv(const double* G, int l, int ld, double* R, double* Rinv, int* info, hipStream_t s, const double* wsum = nullptr,
              float* vec32 = nullptr, double* vec64 = nullptr);

// ---- sym_eig.hip ----
// Eigen-decomposition of the symmetric l x l matrix G (row stride ld) on the device, one workgroup (parallel Jacobi in LDS,
// l <= 112): M (ld x ldk, zero padded) = leading k eigenvectors in columns, each divided by sigma_j = sqrt(lambda_j), in
// descending order; sigma[0..l) = all of them; status[0] = 0 / 1 (not converged) | 2 (non-finite), status[1] = sweeps.
bool sym_eig_device_ok(int l);
void sym_eig_device(const double* G, int l, int ld, int k, int ldk, double* M, double* sigma, int* status, hipStream_t s);
// ---- panel_gemm.hip ----
// out[rows x ldo] = P[rows x ld] * M[ld x ldo]  (M f64, row-major, ldo % 16 == 0); out may alias P
// when ldo == ld.
// out_stride (0: ldo) is the row stride of `out`, out_cols (0: ldo) the number of leading columns written.
template <typename T>
void panel_gemm(const T* P, int64_t rows, int ld, const double* M, int ldo, T* out, hipStream_t s, bool upper = false, int out_stride = 0,
                int out_cols = 0);
// ---- gram.hip (the column sums) ----
// out[j] = sum_r w[r] P[r][j]  (w null => ones), j < ld, f64 accumulation.
template <typename T>
void weighted_colsum(const T* P, int64_t rows, int ld, const T* w, T* out, DevBuf& scratch, hipStream_t s);
// ---- panel_ops.hip ----
// Z[r][j] -= mu[r] * svec[j]
template <typename T>
void rank1_subtract(T* Z, int64_t rows, int ld, const T* mu, const T* svec, hipStream_t s);
// components[r][j] = sign_r * VtT[j][r] for r < k, with sign_r making the largest-|.| entry of
// row r positive (first index on ties): single_svdlib::randomized::svd_flip, v-based.
// sign_out (nullable): receives the device address of the k signs (in `scratch`)
template <typename T>
void flip_transpose(const T* VtT, int64_t n, int ld, int k, T* components, DevBuf& scratch, hipStream_t s, const double** sign_out = nullptr);
// out[j][c] = scale[j] * P[j][c] (scale null: copy); M[i][j] *= sign[j] for j < k
template <typename T>
void scale_rows(const T* P, int64_t rows, int ld, const double* scale, T* out, hipStream_t s);
void scale_columns(double* M, int rows, int ld, int k, const double* sign, hipStream_t s);
// W[j][r] = scale[j] * comps[r][j]  (r < k; zero for k <= r < ld); scale may be null.
template <typename T>
void scaled_transpose(const T* comps, int64_t n, int k, const double* scale, T* W, int ld, hipStream_t s);
template <typename T>
void fill_zero(T* p, int64_t count, hipStream_t s);
template <typename T>
void convert_from_f64(const double* in, T* out, int64_t count, hipStream_t s);
template <typename T>
void strip_padding(const T* in, int64_t rows, int ld, int ncols, T* out, hipStream_t s);
template <typename T>
void add_padding(const T* in, int64_t rows, int ncols, T* out, int ld, hipStream_t s);

// ---- covar.hip: implicit row-side correction by an orthonormal covariate basis (sapca_set_covariates) --------------------
// columns of the basis panel Q (rows x kCovarCols of T, zero beyond the basis' rank) = SAPCA_MAX_DESIGN_COLUMNS
constexpr int kCovarCols = 16;
// S (kCovarCols x ld, f64) = Q^T Y for a rows x ld panel Y, ld % 16 == 0 (ld <= 128) or ld % 64 == 0 (ld <= 1024).  Per-workgroup
// partial sums (in `scratch`) added in block order by a second kernel: no atomics, the same bits from run to run.
template <typename T>
void panel_qt_y(const T* Y, const T* Q, int64_t rows, int ld, double* S, DevBuf& scratch, hipStream_t s);
// Y[i][c] = T(Y[i][c] - sum_j Q[i][j] S[j * lds + c]) for c < ncols (f64 arithmetic, one rounding).  Y has row stride ld; a full
// panel (ncols == ld, a width panel_qt_y takes) moves in 16-byte vectors, anything else -- the m x k projection -- by elements.
template <typename T>
void panel_sub_qs(T* Y, const T* Q, int64_t rows, int ld, int ncols, const double* S, int lds, hipStream_t s);

// ---- colscale.hip: implicit column scaling S = (A - 1 mu^T) diag(d) of a randomized fit (sapca_set_column_scaling) ------------
// The factors of the n_used columns a fit uses (column j sits at sel[j] of the full-width sums; sel null: at j), from the f64
// column sums: weights (full width, f64) null: d = 1 / sqrt(var) about the mean, 0 where ss = sumsq - sum^2 / m <= 4 m eps_f64 sumsq;
// else d = weights.  d64 / dt: d in f64 and rounded once to T; w = T(d * sum / m); *total = sum_j d_j^2 var_j, added in a fixed
// order through part (column_scale_partials(n_used) doubles).  No atomics.
size_t column_scale_partials(int64_t n_used);
template <typename T>
void column_scale_factors(const double* sum, const double* sumsq, double m, const int32_t* sel, const double* weights, int64_t n_used,
                          double* d64, T* dt, T* w, double* part, double* total, hipStream_t s);
// P[r][c] = P[r][c] * d[r] in place for a rows x ld panel whose rows are 16-byte vectors (ld % (16 / sizeof(T)) == 0, P aligned)
template <typename T>
void scale_panel_rows(T* P, int64_t rows, int ld, const T* d, hipStream_t s);
// P[r][c] = d[r] * (sum of src's slabs - src.mu[r] src.sv[c]): what materialize() writes, times d, in one pass (P may be src.parts)
template <typename T>
void finish_scaled_panel(T* P, int64_t rows, int ld, const PanelSource<T>& src, const T* d, hipStream_t s);

// ---- knn.hip: exact k-nearest neighbours of dense row panels (sapca_knn_device_*) ----------------------------------------
// The launch geometry of the selection: query rows per workgroup (64 * mt), corpus splits per query block, LDS per workgroup.
struct KnnPlan {
  int mt = 1, nsplit = 1, tiles_per_split = 1;
  size_t lds_bytes = 0;
};
template <typename T>
KnnPlan knn_plan(int64_t mq, int64_t mc, int k, int n_cus);
// EUCLIDEAN: bias[r] = -|x_r|^2 (unit unused).  COSINE / PEARSON: unit (rows x d, row stride d) = the rows (centred for
// PEARSON) scaled to unit norm, a row of norm <= sqrt(eps_T) as zeros (bias unused).  Reads x[r * ld + t] for t < d only.
template <typename T>
void knn_prepare(const T* x, int64_t ld, int64_t rows, int d, int metric, T* unit, T* bias, hipStream_t s);
// per (query, split) the k best corpus rows of the split's range by (alpha <a, b> + bias, -index), sorted:
// part_sc / part_ix [mq][plan.nsplit][k]; an unfilled slot holds (-inf, INT_MAX).  bias null: 0.
template <typename T>
void knn_select(const T* q, int64_t ldq, int64_t mq, const T* c, int64_t ldc, int64_t mc, const T* bias, int d, int metric, int k,
                bool exclude_self, const KnnPlan& plan, T* part_sc, int32_t* part_ix, hipStream_t s);
// merged [mq][k] = the corpus rows of the k best entries of a query's nsplit (<= 64) lists, by the same key
template <typename T>
void knn_merge(const T* part_sc, const int32_t* part_ix, int64_t mq, int nsplit, int k, int32_t* merged, hipStream_t s);
// the values of the selected pairs (sel[query * sel_stride + slot]) from the original rows in f64, rounded once to T, each
// list sorted by (value ascending for EUCLIDEAN / descending otherwise, index); an unfilled slot gives (-1, NaN), last
template <typename T>
void knn_refine(const T* q, int64_t ldq, int64_t mq, const T* c, int64_t ldc, int64_t mc, int d, int metric, const int32_t* sel,
                int64_t sel_stride, int k, int32_t* out_ix, T* out_val, hipStream_t s);

// ---- tsne.hip: t-SNE on dense row panels (sapca_tsne_*); include/sapca.h states the algorithm ------------------------------
// p[i * K + slot] = p_{slot|i} (f64) and beta[i] (nullable) from the K neighbour distances of row i (dist, NOT squared); a slot
// whose index is outside [0, m) contributes nothing and gets 0.  One wave per row, K <= 128.
template <typename T>
void tsne_perplexity(const int32_t* idx, const T* dist, int64_t m, int K, double perplexity, double* p, double* beta, hipStream_t s);
// len[0 .. m] (zeroed here) = per row its valid slots + the rows that list it, len[m] = 0; nvalid[i] = the former
void tsne_count(const int32_t* idx, int64_t m, int K, int64_t* len, int32_t* nvalid, hipStream_t s);
// the unsorted CSR of the 2 m K emitted entries at offsets ptr (the scan of len): row i's own (j, p_j|i) first, in slot order,
// then (j, p_i|j) of the rows j that list i in the order an integer cursor (m words, zeroed here) hands out
void tsne_emit(const int32_t* idx, const double* p, int64_t m, int K, const int64_t* ptr, const int32_t* nvalid, int32_t* cursor,
               int32_t* out_idx, double* out_val, hipStream_t s);
// out[e] = T(in[e] * inv)
template <typename T>
void tsne_scale(const double* in, int64_t nnz, double inv, T* out, hipStream_t s);
// The repulsion's geometry: the j tiles are dealt into nchunk chunks by m alone, and every chunk's sums are formed from zero
// and added in chunk order whether one workgroup walks them all or (split) one workgroup takes each: the same bits.
struct TsnePlan {
  int nchunk = 1, tiles_per_chunk = 1;
  bool split = false;   // by default where the i blocks alone leave CUs idle (debug builds: SAPCA_TSNE_SPLIT=0|1)
};
TsnePlan tsne_plan(int64_t m, int n_cus);
size_t tsne_sum_parts(int64_t n);   // doubles of work space tsne_sum / tsne_repulsion need for n addends
// rep[i * (D + 1) + c] = sum_{j != i} q_ij^2 (y_i - y_j)[c] (c < D), [.. + D] = sum_{j != i} q_ij; *z = the sum of the latter
// over i.  part: plan.nchunk * m * (D + 1) doubles when plan.split.  y: m rows of D values, row stride ldy.  D in 1..3.
template <typename T>
void tsne_repulsion(const T* y, int64_t ldy, int64_t m, int D, const TsnePlan& plan, double* part, double* rep, double* sum_part, double* z,
                    hipStream_t s);
// grad (m x D, packed) = T(exaggeration * sum_j P_ij q_ij (y_i - y_j) - rep_i / *z); klrow[i] = sum_j P_ij ln(P_ij *z / q_ij)
template <typename T>
void tsne_attraction(const CsrView<T>& P, const T* y, int64_t ldy, int D, double exaggeration, const double* rep, const double* z, T* grad,
                     double* klrow, hipStream_t s);
// *out = in[0] + .. + in[n - 1] in an order fixed by n
void tsne_sum(const double* in, int64_t n, double* sum_part, double* out, hipStream_t s);
// gains, velocity and step of one epoch on packed m x D arrays, then every column of y re-centred (tsne_center)
template <typename T>
void tsne_update(T* y, T* v, T* gain, const T* grad, int64_t m, int D, double momentum, double rate, double* colpart, double* mean,
                 hipStream_t s);
// y[:, c] -= its mean (f64, per-block sums in colpart -- ceil(m / 256) * D doubles -- then one workgroup; sum_first: form them here)
template <typename T>
void tsne_center(T* y, int64_t m, int D, double* colpart, double* mean, bool sum_first, hipStream_t s);
// v = 0, gain = 1, and, y non-null, y = 1e-4 N(0, 1) from gaussian_panel under `seed`
template <typename T>
void tsne_init_state(T* y_or_null, T* v, T* gain, int64_t m, int D, uint32_t seed, hipStream_t s);

// ---- umap.hip: UMAP on dense row panels (sapca_umap_*); include/sapca.h states the algorithm -------------------------------
// rowsum[i] = the sum of row i's distances over the slots whose index is inside [0, m) (f64, one order).  One wave per row, K <= 128.
template <typename T>
void umap_row_sums(const int32_t* idx, const T* dist, int64_t m, int K, double* rowsum, hipStream_t s);
// a[i * K + slot] = the membership of the slot (0 where its index is outside [0, m)), sigma[i], rho[i] (both nullable);
// *total = the sum of every valid distance of the panel (the floor of sigma where rho is 0)
template <typename T>
void umap_smooth(const int32_t* idx, const T* dist, int64_t m, int K, int n_neighbors, const double* total, double* a, double* sigma,
                 double* rho, hipStream_t s);
// (idx, val) at offsets ptr, every row sorted -> (out_idx, out_val) at new_ptr (which may be ptr): a run of equal columns becomes
// one entry, folded by (a + b) - a b in f64; every value rounded once to T
template <typename T>
void umap_union_fill(const int64_t* ptr, const int32_t* idx, const double* val, int64_t m, const int64_t* new_ptr, int32_t* out_idx,
                     T* out_val, hipStream_t s);
// *wmax = the largest positive value (0: none); next[e] = *wmax / val[e], nextn[e] = next[e] / rate
template <typename T>
void umap_schedule(const T* val, int64_t nnz, int rate, double* wmax, double* next, double* nextn, hipStream_t s);
// y (m x D packed) = 10 (x[:, c] - min_c) / (max_c - min_c), 0 for a constant column; minmax: 2 D doubles of work space
template <typename T>
void umap_init_panel(const T* x, int64_t ldx, int64_t m, int D, double* minmax, T* y, hipStream_t s);
// y[i * D + c] = T(10 hash_u01(seed, 31, i D + c))
template <typename T>
void umap_init_random(T* y, int64_t m, int D, uint32_t seed, hipStream_t s);
struct UmapEpoch {
  uint64_t epoch = 0, seed = 0;
  double n_epochs = 1, alpha = 0, a = 1, b = 1, gamma = 1, rate = 0;
};
// one epoch of the layout: y_out from y_in (distinct, m x D packed), the schedule advanced in place.  One launch.
template <typename T>
void umap_epoch(const CsrView<T>& G, const T* y_in, T* y_out, int D, const UmapEpoch& p, const double* wmax, double* next, double* nextn,
                hipStream_t s);

// ---- kmeans.hip: k-means on dense row panels (sapca_kmeans_*); include/sapca.h states the algorithm ------------------------
// The control block of a run (device, unsigned 64-bit words).  Every kernel below that takes `skip` returns at once when
// *skip != 0 (null: never): the loop's kernels watch kKmDone, the closing assignment watches kKmStrict.
enum { kKmDone = 0, kKmStrict = 1, kKmIter = 2, kKmChanged = 3, kKmAmbiguous = 4, kKmCtlWords = 8 };
// The geometry of the update, fixed by (m, k): a wave counts and places rows_per_wave consecutive rows (nwaves of them), and
// every cluster's sorted list is summed in `slices` consecutive pieces that are then added in order.
struct KmeansPlan {
  int64_t rows_per_wave = 256, nwaves = 1;
  int slices = 1;
};
KmeansPlan kmeans_plan(int64_t m, int k);
int kmeans_column_slices(int64_t m);   // pieces of the rows in the column sums behind tol_abs
// k-means++ from the uniforms hash_u01(seed, 21, t): cen (k x d, packed) = the chosen rows, rows[t] their numbers (k words).
// dist: m doubles, bsum: ceil(m / 1024) doubles of work space.  Nothing is read back.
template <typename T>
void kmeans_seed(const T* x, int64_t ldx, int64_t m, int d, int k, uint32_t seed, T* cen, int32_t* rows, double* dist, double* bsum,
                 hipStream_t s);
// labels[i] = argmax_c 2 <x_i, c> + bias[c] on the matrix cores (bias = -|c|^2 and xb[i] = -|x_i|^2 from knn_prepare), ties to
// the lower c; a row whose runner-up lies within 4 d eps_T (|x_i| + max |c|)^2 of the best is appended to amb_list (m words,
// in no particular order) and counted in ctl[kKmAmbiguous], which the caller (or kmeans_step) has set to 0
template <typename T>
void kmeans_rank(const unsigned long long* skip, const T* x, int64_t ldx, int64_t m, const T* cen, int k, const T* bias, const T* xb, int d,
                 int32_t* labels, int32_t* amb_list, unsigned long long* ctl, hipStream_t s);
// the ctl[kKmAmbiguous] listed rows decided by the k direct distances in f64 under (distance, index)
template <typename T>
void kmeans_refine(const unsigned long long* skip, const T* x, int64_t ldx, int64_t m, const T* cen, int k, int d, int32_t* labels,
                   const int32_t* amb_list, const unsigned long long* ctl, hipStream_t s);
// rowd[i] = |x_i - cen[labels[i]]|^2 by the direct formula in f64 (0 for a label outside [0, k)), dist2[i] (nullable) = T(rowd[i])
template <typename T>
void kmeans_distances(const T* x, int64_t ldx, int64_t m, const T* cen, int k, int d, const int32_t* labels, T* dist2, double* rowd,
                      hipStream_t s);
// the rows sorted by (label, row): cnt (k * plan.nwaves + 1 words) = the rows of every (cluster, wave) run, tab (as many) =
// their offsets, so cluster c's list is order[tab[c * nwaves] .. tab[(c + 1) * nwaves]); a label outside [0, k) is left out.
// The scan between the two passes cannot be skipped; it reads cnt and writes tab, so behind a skipped count it writes the
// same offsets again.  prev non-null: the rows whose
// label differs from prev[i] are counted into ctl[kKmChanged] by the counting pass.
void kmeans_sort(const unsigned long long* skip, const int32_t* labels, int64_t m, int k, const KmeansPlan& plan, int64_t* cnt,
                 int64_t* tab, int32_t* order, DevBuf& scan, const int32_t* prev, unsigned long long* ctl, hipStream_t s);
// partial[(c * slices + s) * d + t] = the f64 sum over slice s of cluster c's list of x[row][t] (center null) or of
// (x[row][t] - center[t])^2.  order / tab null: one cluster, the rows 0 .. m - 1 in order (k == 1).
template <typename T>
void kmeans_sums(const unsigned long long* skip, const T* x, int64_t ldx, int64_t m, int d, const int32_t* order, const int64_t* tab,
                 int64_t nwaves, int k, int slices, const double* center, double* partial, hipStream_t s);
// cen[c] = T(sum of its slices / n_c) where n_c > 0 (kept otherwise); counts[c] (nullable) = n_c; shiftpart[c] = |new - old|^2
template <typename T>
void kmeans_finalize(const unsigned long long* skip, const double* partial, const int64_t* tab, int64_t nwaves, int k, int d, int slices,
                     T* cen, int64_t* counts, double* shiftpart, hipStream_t s);
// the end of iteration `iter` of the loop: n_iter, the strict test (no label changed, iter > 0), shift <= *tol_abs; the counts
// of changed and of ambiguous rows go back to 0
void kmeans_step(unsigned long long* ctl, const double* shiftpart, int k, const double* tol_abs, unsigned long long iter, hipStream_t s);
// cols[t] = sum_s partial[s * d + t] / m; scalar (nullable): *scalar = scale * mean_t cols[t]
void kmeans_fold_columns(const double* partial, int slices, int d, int64_t m, double* cols, double scale, double* scalar, hipStream_t s);
// a strict run's labels are those of its last iteration: out = (ctl[kKmIter] - 1) & 1 ? lab1 : lab0 when ctl[kKmStrict]
void kmeans_take_labels(const unsigned long long* ctl, const int32_t* lab0, const int32_t* lab1, int32_t* out, int64_t m, hipStream_t s);

// ---- harmony.hip: Harmony on dense row panels (sapca_harmony_*); include/sapca.h states the algorithm -----------------------
// unit (rows x d, row stride ldu) = the rows of x scaled to unit L2 norm (the norm in f64; a row of norm 0 stays 0)
template <typename T>
void harmony_unit_rows(const T* x, int64_t ldx, int64_t rows, int d, T* unit, int64_t ldu, hipStream_t s);
// cnt[b] (B + 1 words, zeroed here) = the rows of batch b, cnt[B] = the first row whose label lies outside [0, B) (m: none)
void harmony_count(const int32_t* batch, int64_t m, int B, unsigned long long* cnt, hipStream_t s);
// by_batch (m words) = the rows sorted by (batch, row), a stable radix sort of the labels; key / key_out / val: m words of work
// space each
void harmony_sort_batches(const int32_t* batch, int64_t m, int B, uint32_t* key, uint32_t* key_out, uint32_t* val, uint32_t* by_batch,
                          DevBuf& sort_tmp, hipStream_t s);
// The update order of pass c: list (m words) = the rows sorted by (block, batch, order), where order is the rank under
// (hash_u01(seed, 61, c m + i), i) and block the numpy.array_split piece of that rank among nb pieces; keys (m words) = block *
// B + batch of every list entry, ascending.  hkey / hkey_out / key2 (u64) and perm / iota (u32): m words of work space each.
void harmony_order(const int32_t* batch, int64_t m, int B, int64_t nb, uint64_t seed, uint64_t pass, uint64_t* hkey, uint64_t* hkey_out,
                   uint32_t* iota, uint32_t* perm, uint64_t* key2, uint64_t* keys, uint32_t* list, DevBuf& sort_tmp, hipStream_t s);
int harmony_slices(int64_t rows);   // pieces of a list in harmony_sums, by the list's length alone
// partial[((b * K + k) * slices + sl) * D + t] = the f64 sum over slice sl of batch b's list (order[seg[b] .. seg[b + 1]); order
// and seg null: B == 1, the rows 0 .. m - 1) of R[row][k] x[row][t]; D = d + 1 with `ones` (column d of x counts as 1), else d
template <typename T>
void harmony_sums(const T* x, int64_t ldx, int64_t m, int d, bool ones, const T* R, int K, const uint32_t* order, const int64_t* seg, int B,
                  int slices, double* partial, hipStream_t s);
// Y[k] (K x d, packed) = the slices' sums of cluster k (B == 1, no ones column) added in order, scaled to unit norm in f64
template <typename T>
void harmony_centroids(const double* partial, int K, int d, int slices, T* Y, hipStream_t s);
// beta[(k * B + b) * d + t] from the slices' sums with the ones column (item 5's closed form; a cluster without weight: zeros)
void harmony_beta(const double* partial, int K, int B, int d, int slices, double lambda, double* beta, hipStream_t s);
// out[i] = T(z_i - sum_k R_ik beta[k][batch_i]) in f64
template <typename T>
void harmony_apply(const T* z, int64_t ldz, int64_t m, int d, const T* R, int K, const int32_t* batch, int B, const double* beta, T* out,
                   int64_t ldc, hipStream_t s);
// O (B x K) and rs (K) = the sums of R over every batch's list, formed from zero: the f64 column sums of R over fixed slices of
// each list, folded in order.  colsum: B * slices * K doubles of work space.
template <typename T>
void harmony_totals(const T* R, int64_t m, int K, const uint32_t* by_batch, const int64_t* seg, int B, int slices, double* colsum, double* O,
                    double* rs, hipStream_t s);
// The fold around block `remove` of a pass (nb blocks, -1: none): the rows of block `add` (-1: none) are added to O / rs from R
// as it stands, the rows of block `remove` taken out, and pen[b * K + k] = ((Pr_b rs_k + 1) / (O_bk + 1))^theta set for it.
// Every (batch, k) sum runs over the block's list segment of that batch in 256 interleaved lanes added pairwise in a fixed tree.
template <typename T>
void harmony_fold(const T* R, int64_t m, int K, int B, int64_t nb, int64_t add, int64_t remove, const uint64_t* keys, const uint32_t* list,
                  const double* Pr, double theta, double* O, double* rs, double* pen, hipStream_t s);
// The fused block update on the matrix cores: for the rows list[p0 .. p0 + n) (list null: the rows p0 .. p0 + n - 1),
// R[row][k] = T(e_k pen[batch_row][k] / their sum) with e_k = exp(-(dist_k - min dist) / sigma), dist_k = 2 (1 - <zc_row, Y_k>)
// (pen null: 1); dist (nullable, m x K) receives T(dist_k).  Three sweeps over Y recompute the same FMA chains: the row's
// scores never leave the chip.
template <typename T>
void harmony_block(const T* zc, int64_t ldz, int64_t m, int d, const T* Y, int K, const int32_t* batch, int B, const uint32_t* list, int64_t p0,
                   int64_t n, const double* pen, double sigma, T* R, T* dist, hipStream_t s);
int64_t harmony_block_begin(int64_t j, int64_t m, int64_t nb);   // the first list position of block j of a pass (j == nb: m)
// rowd[c * m + i] (c < 3) = row i's share of the three terms of the objective
template <typename T>
void harmony_objective(const T* R, const T* dist, const int32_t* batch, int64_t m, int K, int B, const double* O, const double* rs,
                       const double* Pr, double sigma, double theta, double* rowd, hipStream_t s);

// ---- louvain.hip: Louvain clustering of a symmetric CSR graph (sapca_louvain_*); include/sapca.h states the algorithm ------
// The control block of a level (device).  A kernel that takes a LouvainState returns at once when ctl->done is set (and, where
// it works on the candidate assignment, when ctl->moved is 0); ctl null: never.  `cur` says which of the two label / total
// generations holds the kept assignment; flip = 1 addresses the other, the candidate.
struct LouvainCtl {
  unsigned long long done, cur, sweeps, misses, kept, moved;
  double Q, S, sum_s, sum_sq, tol, gamma;
};
struct LouvainState {
  LouvainCtl* ctl = nullptr;
  int32_t* lab[2] = {nullptr, nullptr};   // (lab[0] null with ctl null: every vertex its own community, the coarse rows' merge)
  double* tot[2] = {nullptr, nullptr};
};
// rows per length class: <= kLvWaveCap entries (a wave, keys in 512 bytes of LDS), <= kLvLdsCap (a workgroup, keys in LDS),
// longer (a workgroup, keys in global scratch: ctr[kLvLongKeys] of them in all, row j of the class at long_off[j])
constexpr int kLvWaveCap = 64, kLvLdsCap = 4096;
enum { kLvListWave = 0, kLvListLds = 1, kLvListLong = 2, kLvLongKeys = 3, kLvCtrWords = 4 };
struct LouvainLists {
  const uint32_t* rows = nullptr;   // 3 n words: class c at rows + c n, in no particular order
  const unsigned long long* long_off = nullptr;
  int64_t n = 0, counts[3] = {0, 0, 0};
  unsigned long long* keys = nullptr;
};
void louvain_list_rows(const int64_t* ptr, int64_t n, uint32_t* rows, unsigned long long* long_off, unsigned long long* ctr, hipStream_t s);
void louvain_iota(int32_t* lab, int64_t n, hipStream_t s);
// internal false: out[i] = k_i, the sum of row i over its columns inside [0, n).  true: s_i under the labels (st, flip): the
// entries whose column carries the row's label, 0 for a row whose label is outside [0, n).  One wave per row: lane l adds the
// entries l, l + 64, .. in order and the lanes meet in a fixed butterfly.
template <typename TV>
void louvain_row_sums(const CsrView<TV>& A, const LouvainState& st, int flip, bool internal, double* out, hipStream_t s);
// anchored[C] = 1 where an inactive vertex carries label C (cleared here); active: hash_u01(seed, 41, ((level 4096 + sweep) << 32) + i) < 0.5
void louvain_anchor(const LouvainState& st, int64_t n, uint64_t seed, uint64_t level, uint64_t sweep, uint8_t* anchored, hipStream_t s);
// one local-moving sweep from the kept assignment into the candidate generation; ctl->moved += the vertices that moved
template <typename TV>
void louvain_sweep(const CsrView<TV>& A, const LouvainLists& L, const LouvainState& st, const double* k, const uint8_t* anchored,
                   uint64_t seed, uint64_t level, uint64_t sweep, hipStream_t s);
int64_t louvain_sort_len(int64_t n);   // keys the vertex sort needs
// the vertices sorted by (label, vertex) into keys (label << 32 | vertex, a label outside [0, n) left out), tot[C] = the sum of
// k over C's members in ascending vertex order (0 for an empty C), sq[C] = (tot[C] / *S)^2 (sq, S nullable)
void louvain_totals(const LouvainState& st, int flip, bool need_moved, int64_t n, const double* k, unsigned long long* keys, const double* S,
                    double* sq, hipStream_t s);
// the end of a sweep: keep or undo, misses, done (init: Q = Q of the generation just summed, nothing else)
void louvain_decide(const LouvainState& st, bool init, hipStream_t s);
// aggregation: flag[C] = 1 for every label in use (flag: n + 1 words, cleared here; its exclusive scan renumbers)
void louvain_flag(const int32_t* labels, int64_t n, int64_t* flag, hipStream_t s);
// renum[C] = int32 of the scan; renumbered[i] (nullable) = renum[labels[i]], a label outside [0, n) copied through
void louvain_renumber(const int32_t* labels, int64_t n, const int64_t* scan, int32_t* renum, int32_t* renumbered, hipStream_t s);
// cnt[i] = the distinct labels among the entries of row i (diagonal included; 0 for a row whose own label is out of range)
template <typename TV>
void louvain_group_count(const CsrView<TV>& A, const LouvainLists& L, const int32_t* labels, int64_t* cnt, hipStream_t s);
// pos[vertex] = its place p in the sorted keys, rawcnt[p] = cnt[vertex] (0 behind the last vertex; n + 1 words)
void louvain_positions(const unsigned long long* keys, int64_t n, const int64_t* cnt, int32_t* pos, int64_t* rawcnt, hipStream_t s);
// rawptr[renum[C]] = rawoff[first member of C], rawptr[n'] = rawoff[n] (n' = scan[n], on the device)
void louvain_coarse_offsets(const unsigned long long* keys, int64_t n, const int64_t* rawoff, const int32_t* renum, const int64_t* scan,
                            int64_t* rawptr, hipStream_t s);
// row i's entries grouped by label, each group's f64 sum added in stored order, written at out_off[pos ? pos[i] : i] in
// ascending label order as (renum ? renum[label] : label, sum)
template <typename TV>
void louvain_group_emit(const CsrView<TV>& A, const LouvainLists& L, const int32_t* labels, const int32_t* renum, const int64_t* out_off,
                        const int32_t* pos, int32_t* out_idx, double* out_val, hipStream_t s);
// final[v] = renum[labels[first ? v : final[v]]]
void louvain_compose(int32_t* final_labels, int64_t m, const int32_t* labels, const int32_t* renum, bool first, hipStream_t s);

// ---- spectral.hip: components, scale and operator of a symmetric graph (sapca_spectral_*); include/sapca.h states the algorithm ----
// parent[i] = i, *changed = 0
void components_init(int32_t* parent, int64_t m, unsigned long long* changed, hipStream_t s);
// one round: every stored (i, j) with j inside [0, m) hooks the larger root onto the smaller (atomicMin) and sets *changed,
// then every chain is shortened to its root
void components_round(const int64_t* ptr, const int32_t* idx, int64_t m, int32_t* parent, unsigned long long* changed, hipStream_t s);
// flag[i] = parent[i] == i (flag: m + 1 words, flag[m] = 0; its exclusive scan numbers the roots)
void components_flag(const int32_t* parent, int64_t m, int64_t* flag, hipStream_t s);
// labels[i] = scan[parent[i]]
void components_label(const int32_t* parent, int64_t m, const int64_t* scan, int32_t* labels, hipStream_t s);
// the lanes a row gets (8, 16, 32 or 64) from the mean row length; forced > 0: that one (debug switch SAPCA_SPECTRAL_GROUP)
int spectral_group(int64_t m, int64_t nnz, int forced);
// out[i] = sum_j W_ij / div_j over the columns inside [0, m) (div null: ones), by lane groups of g
template <typename T>
void spectral_row_sums(const CsrView<T>& W, const double* div, int g, double* out, hipStream_t s);
// s[i] = 1 / sqrt(d[i]) (q null) or 1 / (q[i] sqrt(z[i] / q[i])), z = d; 0 where a sum is not finite and positive
void spectral_scale_finish(const double* d, const double* q, int64_t m, double* s_out, hipStream_t s);
// wt[e] = W_e (s_i s_j), 0 for a column outside [0, m); safe_idx (nnz int32, nullable) = the columns with one outside [0, m)
// replaced by the row's own number: what a product that does not look at its columns (k::spmv) may read
template <typename T>
void spectral_scaled_copy(const CsrView<T>& W, const double* sc, double* wt, int32_t* safe_idx, hipStream_t s);
// y = Wt x by lane groups of g (the short-row product)
void spectral_spmv(const CsrView<double>& Wt, const double* x, double* y, int g, hipStream_t s);
// U[l][i] = lock_of[labels[i]] == l && t[i] > 0 ? t[i] inv_norm[l] : 0 for l < nlock (U: nlock x m, f64)
void spectral_locked(const int32_t* labels, const int32_t* lock_of, const double* inv_norm, const double* t, int64_t m, int nlock,
                     double* U, hipStream_t s);
// out[i * ldo + col0 + l] = T(sign_l src[l * lds_row + i * lds_col]), l < nvec; fix_sign: sign_l makes the entry of largest
// magnitude (lowest index on a tie) positive, else + (signs: nvec ints of work space)
template <typename T>
void spectral_store(const double* src, int64_t lds_row, int64_t lds_col, int64_t m, int nvec, bool fix_sign, int* signs, T* out,
                    int64_t ldo, int col0, hipStream_t s);
// the spectral start of UMAP; mx: one word of work space
template <typename T>
void umap_spectral_init(const T* E, int64_t ld, int64_t m, int od, uint32_t seed, unsigned long long* mx, T* y, hipStream_t s);

// ---- rng.hip ---------------------------------------------------------------------------
// Omega[r][j] ~ N(0,1) for j < l (zero for l <= j < ld), a pure function of (seed, r*l+j).
template <typename T>
void gaussian_panel(T* out, int64_t rows, int l, int ld, uint32_t seed, hipStream_t s);

// ---- lanczos.hip (BLAS-1/2 helpers on f64 vectors) ---------------------------------------
template <typename T>
void spmv(const CsrView<T>& A, const double* x, double* y, hipStream_t s);

}  // namespace k
}  // namespace sapca
