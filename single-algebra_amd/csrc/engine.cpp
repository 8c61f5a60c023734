// Host orchestration of the sparse-PCA hot path on one GPU (one rank of a row-sharded job).
// Mirrors, step by step:
//   SparsePCA::fit            /root/reference/src/dimred/pca/sparse/mod.rs:102-242
//   MaskedSparsePCA::fit      /root/reference/src/dimred/pca/sparse_masked/mod.rs:255-419
//   SparsePCA::transform      sparse/mod.rs:255-285   (quirk Q2)
//   MaskedSparsePCA::transform sparse_masked/mod.rs:438-546 (quirk Q3)
// with the single-svdlib calls (randomized_svd, svd_las2, svd_flip, MaskedCSRMatrix) realised
// by the kernels in this directory.
#include "engine.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <exception>
#include <memory>
#include <thread>

#include "lanczos.h"
#include "small_svd.h"
#include "spmm_dq.h"

namespace sapca {

namespace {

// Does the LDS-staged sweep pay on an operator of `rows` x `cols` with `entries` stored entries and panels of l columns?  It
// refills an 80 KiB panel tile per (row block, column tile) chunk and only beats the row-gather kernel when a chunk carries
// enough entries to amortise that fill (measured: 64 tile bytes per entry or less -> clearly faster; 164 -> no gain, 4x the
// preparation), and small operators stay on the row kernel whatever their density: their panels sit in L2 / Infinity Cache
// (tools/crossover.py, k = 50: f32 ties at 1e7 entries and the staged path wins by 18 % at 1.6e7; f64 wins by 27 % at 1e7).
// Returns the panel leading dimension of the tile geometry, 0 for the row kernel.
template <typename T>
int staged_sweep_ldp(int64_t rows, int64_t cols, double entries, int64_t l, int spmm_variant) {
  if (spmm_variant == 1 || rows <= 0 || cols <= 0 || l < 1 || l > k::kMaxPanelWidth) return 0;
  const int ldp = 64;
  const double row_bytes = (double)ldp * sizeof(T);
  const double tile_bytes = 80.0 * 1024.0, block_rows = row_bytes == 256.0 ? 512.0 : 256.0;
  const double chunks = std::ceil((double)rows / block_rows) * std::ceil((double)cols * row_bytes / tile_bytes);
  double floor_entries = sizeof(T) == 4 ? 1e7 : 5e6;
  if (const char* e = dbg_env("SAPCA_TILED_MIN_ENTRIES")) floor_entries = atof(e);   // tests: shards either side of the floor
  const bool dense_enough = entries * (sizeof(T) == 4 ? 64.0 : 96.0) >= chunks * tile_bytes && entries >= floor_entries;
  return (spmm_variant == 2 || dense_enough) ? ldp : 0;
}

enum Cat { C_PREPARE, C_STATS, C_SPMM, C_SPMMT, C_ORTHO, C_SMALL, C_LANCZOS, C_TRANSFORM, C_COMM, C_COUNT };

struct Scope {
  sapca_handle_s& h;
  int ev;
  // behind_last: the caller has queued nothing on the stream since the Scope before this one closed -- the two share that
  // point of the stream, and one event (two records back to back leave the GPU idle for about 10 us between the kernels
  // either side of them; a fit step has two such boundaries per sweep)
  Scope(sapca_handle_s& h_, int cat, bool behind_last = false) : h(h_), ev(behind_last ? h_.timer.start_behind_last() : h_.timer.start()) {
    if (ev >= 0) h.spans.emplace_back(cat, ev);
  }
  ~Scope() {
    try { h.timer.stop(ev); } catch (...) {}
  }
};

void collect_timings(sapca_handle_s& h, bool is_fit) {
  if (!h.timer.enabled) return;
  sapca_timings& t = h.timings;
  if (is_fit) {
    const double keep_upload = t.upload_ms;
    const uint64_t keep_steps = t.lanczos_steps;
    std::memset(&t, 0, sizeof(t));
    t.upload_ms = keep_upload;
    t.lanczos_steps = keep_steps;
  } else {
    t.transform_ms = 0;
    for (int ev : h.held_small.in_transform) t.transform_ms -= h.timer.ms(ev);   // the held-back small SVD counts as small_svd_ms only
  }
  double comm_dev_ms = 0;
  for (auto& sp : h.spans) {
    if (is_fit == (sp.first == C_TRANSFORM)) continue;  // fit spans on fit, transform spans on transform
    const double ms = h.timer.ms(sp.second);
    switch (sp.first) {
      case C_PREPARE: t.prepare_ms += ms; break;
      case C_STATS: t.stats_ms += ms; break;
      case C_SPMM:
        t.spmm_ms += ms;
        if (t.n_spmm < 32) t.spmm_sweep_ms[t.n_spmm] = ms;
        t.n_spmm++;
        break;
      case C_SPMMT:
        t.spmmt_ms += ms;
        if (t.n_spmmt < 32) t.spmmt_sweep_ms[t.n_spmmt] = ms;
        t.n_spmmt++;
        break;
      case C_ORTHO: t.ortho_ms += ms; break;
      case C_SMALL: t.small_svd_ms += ms; break;
      case C_LANCZOS: t.lanczos_ms += ms; break;
      case C_TRANSFORM: t.transform_ms += ms; break;
      case C_COMM: comm_dev_ms += ms; break;
      default: break;
    }
  }
  // collectives: device time between events around every all-reduce on the library stream (what the GPU waited);
  // the host-observed time is what remains when timings are not collected
  if (is_fit) t.comm_ms = comm_dev_ms > 0 ? comm_dev_ms : h.comm.host_ms;
}

// ------------------------------------------------------------------------------------------
// prepare: A^T, column statistics, mask compaction (and the few helpers it shares with fit_randomized and transform()).
// ------------------------------------------------------------------------------------------
using H = sapca_handle_s;

// A stream beside the main one and its two events, created on first use.
void lazy_stream(hipStream_t& st, hipEvent_t& a, hipEvent_t& b) {
  if (st) return;
  SAPCA_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
  SAPCA_HIP(hipEventCreateWithFlags(&a, hipEventDisableTiming));
  SAPCA_HIP(hipEventCreateWithFlags(&b, hipEventDisableTiming));
}
hipStream_t side_stream(H& h) { lazy_stream(h.stream2, h.ev_fork, h.ev_join); return h.stream2; }    // A's format beside A^T
hipStream_t stats_stream(H& h) { lazy_stream(h.stream3, h.ev_kept, h.ev_stats); return h.stream3; }  // statistics beside the fit
// what is queued on `later` from here on runs behind everything queued on `earlier` so far
void order_after(hipStream_t later, hipEvent_t ev, hipStream_t earlier) {
  SAPCA_HIP(hipEventRecord(ev, earlier));
  SAPCA_HIP(hipStreamWaitEvent(later, ev, 0));
}
// the device statistics: sum | sumsq | count (n each), then what rides behind them in a multi-rank all-reduce
double* stats_dev(H& h, int64_t n) { return h.stats.as<double>((size_t)3 * n + 1 + H::kStatsTail); }
// leading dimension of a k-column panel swept through a tile-major format built for ldp columns (0: none)
// (above 128 columns every panel is a multiple of 64 wide: column passes of the sweeps, 64 / 128-column blocks of the dense kernels)
int panel_ld(int k, int ldp) { return k > 128 ? (int)round_up(k, 64) : std::max(ldp, k <= 64 ? 64 : 128); }

// The key of the preparation the handle would hold of A under its present mask.
template <typename T>
H::PrepKey prep_key_of(const H& h, const CsrView<T>& A) {
  H::PrepKey key;
  key.ptr = A.ptr; key.idx = A.idx; key.val = A.val;
  key.m = (uint64_t)A.rows; key.n = (uint64_t)A.cols; key.nnz = (uint64_t)A.nnz;
  key.mask_version = h.mask_version; key.dtype = Engine<T>::kDtype; key.valid = true;
  return key;
}

// The original -> compacted column map of the handle's mask on the device.  Main stream, no wait: `o2m32` is pageable
// memory the copy reads, so it has to outlive the stream's next synchronisation.
int32_t* upload_o2m(H& h, std::vector<int32_t>& o2m32) {
  const size_t n = h.orig_to_masked.size();
  o2m32.resize(n);
  for (size_t j = 0; j < n; ++j) o2m32[j] = (int32_t)h.orig_to_masked[j];
  int32_t* d_o2m = h.o2m_dev.as<int32_t>(std::max<size_t>(n, 1));
  SAPCA_HIP(hipMemcpyAsync(d_o2m, o2m32.data(), n * sizeof(int32_t), hipMemcpyHostToDevice, h.stream));
  return d_o2m;
}
// MaskedCSRMatrix::new (sparse_masked/mod.rs:313): A without the masked-out columns, in ca_*.  Main stream; synchronises
// with the host (the entry count comes back).  drop_* / amax_bits: see k::compact_columns.
template <typename T>
H::RawCsr compact_a(H& h, const CsrView<T>& A, const int32_t* d_o2m, int64_t n_used, int32_t* drop_col = nullptr,
                    T* drop_val = nullptr, unsigned long long* amax_bits = nullptr) {
  const CsrBuf<T> ca = csr_buffers<T>(h.ca_ptr, h.ca_idx, h.ca_val, A.rows, A.nnz);
  int64_t nnz_used = 0;
  k::compact_columns(A, d_o2m, ca.ptr, ca.idx, ca.val, &nnz_used, h.scratch, h.stream, drop_col, drop_val, amax_bits);
  return ca.raw(A.rows, n_used, nnz_used);
}

// The route of a preparation: what prepare() knows before it enqueues its first kernel, as three choices.
//  A^T                 | taken by                                   | what happens
//  Nothing             | Lanczos, n_used <= m, m >= 4096, nnz > 0,  | no transposed operator: the second product of a step scatters into LDS (scatter.hip,
//                      | k::scatter_fits (~19k columns: C3 has 18k) | fixed-point sums: reproducible); masked fits still compact A
//  FormatFromA         | f32, staged sweep, unmasked                | A^T's tile-major format straight from A (tiled_build.hip, "bucket route"): no sort, no
//                      |                                            | transposed CSR; outside its limits (more than 65536 columns, ...) refused: Transposed
//  FormatFromCompacted | f32, staged sweep, masked, n_used <= 65536 | compaction, then the same builder on its result; refused: CompactedTransposed
//  CompactedTransposed | every other masked fit                     | compaction, then its transposition into cat_*
//  Transposed          | every other unmasked fit                   | transposition of A into at_* (tile-major and packed, tile-major, or natural rows)
//  statistics from     |                                            |
//  Upload              | a host matrix that came through upload()   | the exact sums gathered behind the DMA (not if a value was inf / nan)
//  Scatter             | A^T Nothing                                | k::colstats_scatter: the same kind of pass over A as the products
//  FormatBuild         | A^T FormatFromA                            | by-product of the builder + k::row_lengths_f64; Transposed where it refused
//  KeptAndDropped      | masked                                     | the kept columns' sums (the builder's, or row sums of the compacted A^T) scattered
//                      |                                            | over the sums of the (column, value) pairs the compaction dropped
//  Transposed          | the rest                                   | k::at_stats_index on packed rows, else k::row_sums; k::row_lengths_f64
//  statistics to host  |                                            |
//  AllReduce           | more than one rank                         | all-reduce with the tail (row count, piece votes), wait, finish_statistics now
//  MainCopy            | one rank; unmasked, or statistics Upload   | async copy on the main stream, read at the end of fit() (or SAPCA_MASK_STATS_INLINE)
//  SideChain           | one rank, statistics KeptAndDropped        | a chain on stream3 queued at the end of prepare(); a Lanczos fit queues the dropped
//                      |                                            | pairs' sort at once and only the rest of the chain at the end
//  ScatterSide         | one rank, statistics Scatter               | colstats_scatter and the host copy on stream3, queued at once: an uncentred Lanczos
//                      |                                            | fit reads them when fit() ends.  A centred one (sapca_options.lanczos_center) needs the
//                      |                                            | means before its first step: fit() makes the main stream wait for ev_stats in front of
//                      |                                            | the iterations and gives the overlap up
enum class AtFrom { Nothing, FormatFromA, FormatFromCompacted, CompactedTransposed, Transposed };
enum class StatsFrom { Upload, Scatter, FormatBuild, KeptAndDropped, Transposed };
enum class StatsTo { AllReduce, MainCopy, SideChain, ScatterSide };

struct PrepPlan {
  int64_t m = 0, n = 0, nnz = 0, n_used = 0;   // A's shape; the columns the mask keeps (no mask: n)
  bool masked = false;
  int tiled_ldp = 0;   // panel leading dimension of the LDS-staged sweep's formats; 0: row kernel, no formats
  int at_nct = 0;      // > 0: transposed rows come out grouped by the interleaved tile of the A row they came from
  AtFrom at = AtFrom::Transposed;
  StatsFrom stats = StatsFrom::Transposed;
  StatsTo deliver = StatsTo::MainCopy;
};

// What only a builder's return value settles; the stages fill it in.
template <typename T>
struct PrepOutcome {
  int64_t nnz_used = 0;                  // entries the compaction kept
  bool at_direct = false;                // build_tiled_at_direct took the operator (A, or the compacted matrix)
  bool a_aside = false, ok_a = false;    // A's format: queued on the side stream; came out
  CsrView<T> At;                         // unmasked fits: the transposed CSR (FormatFromA: its row offsets only)
  const uint64_t* at_packed = nullptr;   // the transposition left its rows packed (row << 32 | value bits)
  bool at_seg_ready = false;             // ... and the statistics pass left the format builder's per-row tile index
};

// The mask's index maps as the device wants them.  Pageable memory read by async copies: alive until prepare() has synchronised.
struct MaskMaps {
  std::vector<int32_t> o2m32, sel;
  int32_t *d_o2m = nullptr, *d_sel = nullptr;
};

// The thread that drives A's format build.  Joined on every exit of prepare(), exceptions included: it must not run into freed state.
struct Aside {
  std::thread t;
  std::exception_ptr err;
  ~Aside() { if (t.joinable()) t.join(); }
  void join() { if (t.joinable()) t.join(); if (err) std::rethrow_exception(err); }
};

// Enqueues nothing; waits on the host for the upload's accumulator flag where a host matrix brought its statistics along.
template <typename T>
PrepPlan plan_preparation(H& h, const CsrView<T>& A) {
  PrepPlan p;
  const int64_t m = p.m = A.rows, n = p.n = A.cols, nnz = p.nnz = A.nnz;
  p.masked = !h.mask.empty();
  const int64_t n_used = p.n_used = p.masked ? (int64_t)std::count_if(h.mask.begin(), h.mask.end(), [](uint8_t b) { return b != 0; }) : n;
  // LDS-staged sweep (randomized fits; staged_sweep_ldp has the break-even): it fixes the order the transposed rows are produced in
  if (h.opt.method == SAPCA_RANDOM && m > 0 && n > 0 && n_used > 0) {
    const int64_t l = std::min<int64_t>((int64_t)(h.opt.n_components + h.opt.n_oversamples), std::min<int64_t>(m, n_used));
    p.tiled_ldp = staged_sweep_ldp<T>(m, n_used, (double)nnz * ((double)n_used / (double)n), l, h.opt.spmm_variant);
  }
  // (SAPCA_TRANSPOSE_GATHER: transpose_csr's permutation + gather route for f64 only knows the natural row order)
  const bool at_tile_major = p.tiled_ldp != 0 && dbg_env("SAPCA_AT_NATURAL") == nullptr &&
                             !(sizeof(T) == 8 && dbg_env("SAPCA_TRANSPOSE_GATHER") != nullptr);
  p.at_nct = at_tile_major ? k::tiled_tile_count(m, p.tiled_ldp * (int)sizeof(T) / 4) : 0;   // (a panel row in 4-byte words)

  bool from_upload = h.up_stats.valid && A.ptr == h.in_ptr.p && A.idx == h.in_idx.p && A.val == h.in_val.p &&
                     h.up_stats.m == (uint64_t)m && h.up_stats.n == (uint64_t)n && h.up_stats.nnz == (uint64_t)nnz &&
                     h.up_stats.dtype == Engine<T>::kDtype && n > 0 && !h.comm.active();   // (ranks must not differ in their collectives)
  if (from_upload) {
    // the last chunk's share of those statistics may still be in flight; the accumulators refuse inf/nan (the flag is
    // final once the side stream has passed up_stats_done): the sums of the transposed matrix take over then
    SAPCA_HIP(hipEventSynchronize(h.up_stats_done));
    if (*static_cast<const int*>(h.up_stats.flag.p) != 0) h.up_stats.valid = from_upload = false;
  }
  // (SAPCA_LANCZOS_TRANSPOSE=1 brings the transposed operator of a Lanczos fit, a radix sort, back)
  const bool lz_scatter = h.opt.method == SAPCA_LANCZOS && n_used > 0 && n_used <= m && m >= 4096 && nnz > 0 &&
                          k::scatter_fits(n_used) && dbg_env("SAPCA_LANCZOS_TRANSPOSE") == nullptr;
  const bool bucket_route = sizeof(T) == 4 && at_tile_major;
  if (lz_scatter) p.at = AtFrom::Nothing;
  else if (!p.masked) p.at = bucket_route ? AtFrom::FormatFromA : AtFrom::Transposed;
  else p.at = bucket_route && n_used <= 65536 && dbg_env("SAPCA_AT_SORT") == nullptr ? AtFrom::FormatFromCompacted : AtFrom::CompactedTransposed;

  p.stats = from_upload ? StatsFrom::Upload : lz_scatter ? StatsFrom::Scatter : p.masked ? StatsFrom::KeptAndDropped
            : p.at == AtFrom::FormatFromA ? StatsFrom::FormatBuild : StatsFrom::Transposed;
  if (h.comm.active()) p.deliver = StatsTo::AllReduce;
  else if (p.stats == StatsFrom::Scatter) p.deliver = StatsTo::ScatterSide;
  else if (p.stats == StatsFrom::KeptAndDropped && dbg_env("SAPCA_MASK_STATS_INLINE") == nullptr) p.deliver = StatsTo::SideChain;
  return p;
}

// Mask index maps (sparse_masked/mod.rs:264-271, the HashMap of :462-466): host, then two copies on the main stream.  No wait.
void mask_maps(H& h, const PrepPlan& p, MaskMaps& maps) {
  h.cols_to_use.clear();
  h.orig_to_masked.clear();
  h.has_mask_maps = p.masked;
  if (!p.masked) return;
  h.orig_to_masked.assign((size_t)p.n, -1);
  for (int64_t j = 0; j < p.n; ++j)
    if (h.mask[(size_t)j]) {
      h.orig_to_masked[(size_t)j] = (int64_t)h.cols_to_use.size();
      h.cols_to_use.push_back((uint64_t)j);
    }
  // (sapca_get_mask_index_maps answers from here on; every rank of a sharded fit fails here, before its first collective)
  if (p.n_used == 0) throw Error(SAPCA_ERR_SVD, "SVD computation failed: the mask selects no feature");
  maps.sel.assign(h.cols_to_use.begin(), h.cols_to_use.end());
  maps.d_o2m = upload_o2m(h, maps.o2m32);
  maps.d_sel = h.sel_rows_dev.as<int32_t>((size_t)p.n_used);
  SAPCA_HIP(hipMemcpyAsync(maps.d_sel, maps.sel.data(), (size_t)p.n_used * sizeof(int32_t), hipMemcpyHostToDevice, h.stream));
}

// The sums of the masked-out columns (sum | sumsq of every column, zero where one is kept: mean_ is full width, sparse_masked/
// mod.rs:279-286) from the pairs the compaction dropped, sorted by column in at_*: to dst | dst + n.  stream3 only.
template <typename T>
void drop_sums(H& h, const PrepPlan& p, int64_t nnz_used, double* dst) {
  const CsrBuf<T> work = csr_buffers<T>(h.at_ptr, h.at_idx, h.at_val, p.n, p.nnz);
  k::sums_by_column(h.drop_col.ptr<int32_t>(), h.drop_val.ptr<T>(), p.nnz - nnz_used, p.n, work.ptr, work.idx, work.val, dst,
                    dst + p.n, h.drop_tmp, h.stream3);
}

// Masked fits compact first and transpose only what the mask keeps.  Main stream, synchronises with the host (the count);
// the dropped pairs' sums on stream3, beside the transposition / the bucket route of the kept part and A's format build.
template <typename T>
void compact_and_drop_sums(H& h, const CsrView<T>& A, const PrepPlan& p, const MaskMaps& maps, PrepOutcome<T>& out) {
  hipStream_t s = h.stream;
  Scope sc(h, C_PREPARE);
  const bool pairs = p.stats == StatsFrom::KeptAndDropped;
  const size_t cap = (size_t)std::max<int64_t>(p.nnz, 1);
  // (Lanczos scatter: the compaction gathers max |a| for the fixed-point scales on its way through the values)
  h.a_used = compact_a(h, A, maps.d_o2m, p.n_used, pairs ? h.drop_col.as<int32_t>(cap) : nullptr, pairs ? h.drop_val.as<T>(cap) : nullptr,
                       p.at == AtFrom::Nothing ? h.lz_scalars.as<unsigned long long>(4) : nullptr);
  out.nnz_used = h.a_used.nnz;
  if (!pairs) return;
  hipStream_t s3 = stats_stream(h);
  if (!h.ev_drop) SAPCA_HIP(hipEventCreateWithFlags(&h.ev_drop, hipEventDisableTiming));
  double* d_stats = stats_dev(h, p.n);
  SAPCA_HIP(hipMemsetAsync(d_stats + 2 * p.n, 0, (size_t)p.n * sizeof(double), s));
  if (p.deliver != StatsTo::SideChain) {
    // into the statistics themselves: the main stream waits for ev_drop before it puts the kept columns' sums on top
    order_after(s3, h.ev_drop, s);   // (the compaction synchronised: this only orders the side stream after it)
    drop_sums<T>(h, p, out.nnz_used, d_stats);
    SAPCA_HIP(hipEventRecord(h.ev_drop, s3));
  } else if (h.opt.method != SAPCA_RANDOM) {
    // SideChain keeps them in their own arrays and never waits for them on the main stream.  Randomized fits: queued at the
    // end of prepare(), behind the format builds -- they are the ones the first sweep waits for and the sort shares HBM
    // badly with them, while the sweeps leave most of the HBM rate unused.  Lanczos fits (HBM-bound steps, no formats):
    // now, beside the transposition.
    double* d_drop = h.drop_stats.as<double>((size_t)2 * p.n);
    order_after(s3, h.ev_drop, s);
    drop_sums<T>(h, p, out.nnz_used, d_drop);
  }
}

// A's format runs beside the main stream.  build_tiled synchronises with the host (entry counts come back), so where the main
// thread has such work of its own ahead a helper thread drives it: ev_fork on the main stream, the thread enqueues on stream2.
template <typename T>
void start_a_format_aside(H& h, const CsrView<T>& A, const PrepPlan& p, PrepOutcome<T>& out, Aside& aside) {
  side_stream(h);
  SAPCA_HIP(hipEventRecord(h.ev_fork, h.stream));   // A (and the index maps) are on the device
  h.tiled_a = TiledOp();                            // (while the thread that writes it does not exist yet)
  out.a_aside = true;
  const CsrView<T> src = p.masked ? Engine<T>::view(h.a_used) : A;
  aside.t = std::thread([&h, &p, &out, &aside, src] {
    try {
      SAPCA_HIP(hipSetDevice(h.device));
      SAPCA_HIP(hipStreamWaitEvent(h.stream2, h.ev_fork, 0));
      if (p.tiled_ldp != 0) out.ok_a = k::build_tiled(src, p.tiled_ldp, h.tiled_a, h.tb_a, h.stream2, k::QuadSource::csr());
      SAPCA_HIP(hipEventRecord(h.ev_join, h.stream2));
    } catch (...) {
      aside.err = std::current_exception();
    }
  });
}

// The kept columns' sums (compact numbering) over the dropped pairs' (the per-column counts are only read by the unmasked
// projection).  Main stream; waits for stream3's ev_drop unless the side chain merges the two at the end of prepare().
void scatter_kept_sums(H& h, const PrepPlan& p, const double* d_part, const int32_t* d_sel) {
  double* d_stats = stats_dev(h, p.n);
  if (p.deliver != StatsTo::SideChain) SAPCA_HIP(hipStreamWaitEvent(h.stream, h.ev_drop, 0));   // (the dropped pairs' sums)
  k::scatter_pairs(d_part, d_part + p.n_used, d_sel, p.n_used, d_stats, d_stats + p.n, h.stream);
}

// FormatFromA / FormatFromCompacted: the column sums of the operator it reads come out of the same pass.  Main stream, synchronises with the host.
template <typename T>
void at_format_direct(H& h, const CsrView<T>& A, const PrepPlan& p, const MaskMaps& maps, PrepOutcome<T>& out) {
  if constexpr (sizeof(T) == 4) {
    if (p.masked && out.nnz_used <= 0) return;
    Scope sc(h, C_PREPARE);
    const CsrView<T> src = p.masked ? Engine<T>::view(h.a_used) : A;
    int64_t* t_ptr = (p.masked ? h.cat_ptr : h.at_ptr).template as<int64_t>((size_t)src.cols + 1);
    // A's sums are the statistics; the compacted matrix's are the kept columns' (sums | sums of squares, compact numbering)
    double* d_sums = p.masked ? h.scratch2.as<double>((size_t)2 * p.n_used + 2) : stats_dev(h, p.n);
    h.tiled_at = TiledOp();
    out.at_direct = k::build_tiled_at_direct(src, p.tiled_ldp, h.tiled_at, h.tb_at, t_ptr,
                                             p.stats == StatsFrom::Upload ? nullptr : d_sums, h.scratch, h.stream);
    if (!out.at_direct) return;
    if (!p.masked) out.At = CsrView<T>{p.n, p.m, p.nnz, t_ptr, nullptr, nullptr};
    else h.at_used = {p.n_used, p.m, out.nnz_used, t_ptr, nullptr, nullptr};
    if (p.stats == StatsFrom::KeptAndDropped) scatter_kept_sums(h, p, d_sums, maps.d_sel);
  }
}

// The transposed CSR: of the compacted matrix into cat_* (the kept columns' sums: its row sums), of A into at_*.  Main stream, no wait.
template <typename T>
void at_transpose(H& h, const CsrView<T>& A, const PrepPlan& p, const MaskMaps& maps, PrepOutcome<T>& out) {
  Scope sc(h, C_PREPARE);
  // p.at_nct: rows of A^T grouped by the interleaved tile of the A row they came from -- its format fill streams
  if (p.masked) {
    const CsrBuf<T> cat = csr_buffers<T>(h.cat_ptr, h.cat_idx, h.cat_val, p.n_used, p.nnz);
    k::transpose_csr(Engine<T>::view(h.a_used), cat.ptr, cat.idx, cat.val, h.scratch, h.stream, p.at_nct, nullptr);
    h.at_used = cat.raw(p.n_used, p.m, out.nnz_used);
    if (p.stats != StatsFrom::KeptAndDropped) return;
    double* d_part = h.scratch2.as<double>((size_t)2 * p.n_used + 2);
    k::row_sums(Engine<T>::view(h.at_used), d_part, d_part + p.n_used, h.stream);
    scatter_kept_sums(h, p, d_part, maps.d_sel);
  } else {
    const CsrBuf<T> at = csr_buffers<T>(h.at_ptr, h.at_idx, h.at_val, p.n, p.nnz);
    // the statistics and the format builder read the sort's packed rows directly and the unpack pass into (at_idx, at_val)
    // is skipped (done lazily in build_formats if the row kernel has to take over)
    k::transpose_csr(A, at.ptr, at.idx, at.val, h.scratch, h.stream, p.at_nct,
                     (p.at_nct != 0 && dbg_env("SAPCA_AT_UNPACK") == nullptr) ? &out.at_packed : nullptr);
    out.At = CsrView<T>{p.n, p.m, p.nnz, at.ptr, at.idx, at.val};
  }
}

// R1/R2 (csr.rs:259-312, 558-608) as row sums of A^T, plus the per-column stored-entry count, and their way to the host.
// Main stream (ScatterSide: stream3); AllReduce: the collective, then a wait for the main stream and finish_statistics.
template <typename T>
void column_statistics(H& h, const CsrView<T>& A, const PrepPlan& p, PrepOutcome<T>& out) {
  hipStream_t s = h.stream;
  const int64_t m = p.m, n = p.n;
  double* sums = static_cast<double*>(h.stats_host.ensure(((size_t)2 * n + 1) * sizeof(double)));
  {
    Scope sc(h, C_STATS);
    double* d_stats = stats_dev(h, n);
    switch (p.stats == StatsFrom::FormatBuild && !out.at_direct ? StatsFrom::Transposed : p.stats) {
      case StatsFrom::Upload:
        SAPCA_HIP(hipMemcpyAsync(d_stats, h.up_stats.out.p, (size_t)3 * n * sizeof(double), hipMemcpyDeviceToDevice, s));
        break;
      case StatsFrom::Scatter: {   // every column of A, masked-out ones included, straight from A
        const bool side = p.deliver == StatsTo::ScatterSide;   // on stream3, with the copy to the host behind it: fit() waits for ev_stats at its end
        hipStream_t st = side ? stats_stream(h) : s;
        if (side) order_after(st, h.ev_kept, s);   // (A and max |a| are in place on the main stream)
        k::colstats_scatter(A, h.lz_scalars.ptr<unsigned long long>(), d_stats, d_stats + n, d_stats + 2 * n, side ? h.drop_tmp : h.scratch, st);
        if (side) {
          SAPCA_HIP(hipMemcpyAsync(sums, d_stats, (size_t)2 * n * sizeof(double), hipMemcpyDeviceToHost, st));
          SAPCA_HIP(hipEventRecord(h.ev_stats, st));
        }
        break;
      }
      case StatsFrom::FormatBuild:
        k::row_lengths_f64(out.At.ptr, n, d_stats + 2 * n, s);   // (the sums came out of the format build)
        break;
      case StatsFrom::KeptAndDropped: break;   // (sums in place; the per-column counts are only read by the unmasked projection)
      case StatsFrom::Transposed:
        if constexpr (sizeof(T) == 4) {
          // packed tile-major rows: the statistics pass also leaves the A^T builder's per-row tile index behind
          if (out.at_packed) {
            k::at_stats_index(out.At.ptr, out.at_packed, n, m, p.tiled_ldp, h.tb_at, d_stats, d_stats + n, s);
            out.at_seg_ready = true;
          }
        }
        if (!out.at_seg_ready) k::row_sums(out.At, d_stats, d_stats + n, s);
        k::row_lengths_f64(out.At.ptr, n, d_stats + 2 * n, s);
        break;
    }
    // one rank: the count is m -- no 8-byte copies in either direction in front of the first sweep (each a ~15 us hole)
    sums[(size_t)2 * n] = (double)m;
    // SideChain: the main stream holds the kept columns' sums (all the sweeps' centring reads); stream3 puts them over the dropped
    // columns' arrays and copies the lot to the host (queue_side_statistics) -- the main stream never waits for the dropped pairs' sort
    h.stats_on_side = p.deliver == StatsTo::SideChain || p.deliver == StatsTo::ScatterSide;
    if (p.deliver == StatsTo::MainCopy) {
      SAPCA_HIP(hipMemcpyAsync(sums, d_stats, (size_t)2 * n * sizeof(double), hipMemcpyDeviceToHost, s));
    } else if (p.deliver == StatsTo::AllReduce) {
      // the global row count rides along in the statistics' all-reduce, and so does this rank's vote on where the two-piece A^T sweep cuts
      // the panel (fit_randomized) when its A^T format exists by now (the bucket route builds it first): tail = {rows, ranks that voted, votes}
      double* tail = h.stats_tail;   // (a member: the copy may still be reading it when this function has returned)
      const uint32_t nr = h.comm.nranks;
      const bool ride = Engine<T>::vote_rides(h);
      const size_t ntail = 1 + (ride ? (size_t)nr + 1 : 0);
      std::fill(tail, tail + ntail, 0.0);
      tail[0] = (double)m;
      if (ride && h.tiled_at.valid) {
        // (the vote is for the panel the fit will sweep: above 64 columns it is wider than the format and the sweep stays whole.
        //  m_global is not known yet; where it cuts l to 64 or less every rank has still voted 0 alike)
        const int64_t l_vote = std::min<int64_t>((int64_t)h.opt.n_components + (int64_t)h.opt.n_oversamples, p.n_used);
        tail[1] = 1.0;
        tail[2 + h.comm.rank] = l_vote <= 64 ? (double)Engine<T>::piece_vote(h, h.tiled_at.ldp) : 0.0;
      }
      SAPCA_HIP(hipMemcpyAsync(d_stats + 3 * n, tail, ntail * sizeof(double), hipMemcpyHostToDevice, s));
      { Scope cs(h, C_COMM); h.comm.allreduce(d_stats, (uint64_t)3 * n + ntail, 1, s); }
      SAPCA_HIP(hipMemcpyAsync(sums, d_stats, (size_t)2 * n * sizeof(double), hipMemcpyDeviceToHost, s));
      SAPCA_HIP(hipMemcpyAsync(tail, d_stats + 3 * n, ntail * sizeof(double), hipMemcpyDeviceToHost, s));
    }
  }
  h.stats_cols = n;
  h.vote_ready = false;
  if (p.deliver == StatsTo::AllReduce) {   // the global row count is the sum over the ranks: needed on the host now
    SAPCA_HIP(hipStreamSynchronize(s));
    sums[(size_t)2 * n] = h.stats_tail[0];
    if (Engine<T>::vote_rides(h) && (uint32_t)std::llround(h.stats_tail[1]) == h.comm.nranks) {
      h.vote_cut = (int64_t)*std::min_element(h.stats_tail + 2, h.stats_tail + 2 + h.comm.nranks);
      h.vote_ready = true;
    }
    h.m_global = (uint64_t)std::llround(sums[(size_t)2 * n]);
    h.stats_pending = false;
    Engine<T>::finish_statistics(h);
  } else {   // one rank: the sums reach the host by the time fit() ends (the sweeps centre with means computed on the device)
    h.m_global = (uint64_t)m;
    h.stats_pending = true;
  }
}

// Tile-major companions for the LDS-staged sweep: A^T's on the main stream (build_tiled synchronises with the host), then
// the helper thread that built A's is joined.  Both or neither: a fit sweeps through the formats or through the CSRs.
template <typename T>
void build_formats(H& h, const PrepPlan& p, PrepOutcome<T>& out, Aside& aside) {
  hipStream_t s = h.stream;
  if (!out.a_aside) h.tiled_a = TiledOp();
  if (!out.at_direct) h.tiled_at = TiledOp();
  if (p.tiled_ldp == 0) return;
  Scope sc(h, C_PREPARE);
  const CsrView<T> at = Engine<T>::view(h.at_used);
  bool ok_at = out.at_direct;
  const k::QuadSource at_rows = p.at_nct != 0 ? k::QuadSource::tile_major() : k::QuadSource::csr();   // (how at_transpose ordered them)
  if constexpr (sizeof(T) == 4) {
    if (!ok_at)
      ok_at = k::build_tiled(at, p.tiled_ldp, h.tiled_at, h.tb_at, s,
                             out.at_packed ? k::QuadSource::tile_major_packed(out.at_packed, out.at_seg_ready) : at_rows);
    if (out.at_packed && !ok_at) {   // someone needs the transposed CSR after all
      k::unpack_transposed(out.at_packed, p.nnz, const_cast<int32_t*>(out.At.idx), const_cast<float*>(out.At.val), s);
      out.at_packed = nullptr;
      ok_at = k::build_tiled(at, p.tiled_ldp, h.tiled_at, h.tb_at, s, at_rows);
    }
  } else {
    ok_at = k::build_tiled(at, p.tiled_ldp, h.tiled_at, h.tb_at, s, at_rows);
  }
  aside.join();
  const bool ok_a = out.ok_a;
  ok_at = ok_at && ok_a;
  if (h.opt.verbose)
    fprintf(stderr, "sapca: tile-major formats%s: A %s (nrb %d, nct %d, split %d, %lld entries), A^T %s (nrb %d, nct %d, split %d, %lld entries)\n",
            sizeof(T) == 8 ? " (f64)" : "", ok_a ? "ok" : "no", h.tiled_a.nrb, h.tiled_a.nct, h.tiled_a.nsplit,
            (long long)h.tiled_a.total_entries, ok_at ? "ok" : "no", h.tiled_at.nrb, h.tiled_at.nct, h.tiled_at.nsplit,
            (long long)h.tiled_at.total_entries);
  if (ok_a && ok_at) return;
  h.tiled_a = TiledOp();
  h.tiled_at = TiledOp();
  if (out.at_direct) {   // the row kernel reads a transposed CSR, which the bucket route never made
    const CsrView<T> src = Engine<T>::view(h.a_used);   // (the compacted matrix on the masked route)
    const CsrBuf<T> t = p.masked ? csr_buffers<T>(h.cat_ptr, h.cat_idx, h.cat_val, src.cols, p.nnz)
                                 : csr_buffers<T>(h.at_ptr, h.at_idx, h.at_val, src.cols, p.nnz);
    k::transpose_csr(src, t.ptr, t.idx, t.val, h.scratch, s, 0, nullptr);
    h.at_used = t.raw(src.cols, src.rows, src.nnz);
  }
}

// SideChain: everything the first sweep needs is queued; now the masked-out columns' sums (randomized fits), the kept columns'
// over them, the copy of all statistics to the host (read at the end of fit()).  stream3, behind the main stream; no wait.
template <typename T>
void queue_side_statistics(H& h, const PrepPlan& p, const PrepOutcome<T>& out, const MaskMaps& maps) {
  const int64_t n = p.n;
  double* d_stats = stats_dev(h, n);
  double* d_drop = h.drop_stats.as<double>((size_t)2 * n);
  order_after(h.stream3, h.ev_kept, h.stream);
  if (h.opt.method == SAPCA_RANDOM) drop_sums<T>(h, p, out.nnz_used, d_drop);
  k::copy_selected(d_stats, d_stats + n, maps.d_sel, p.n_used, d_drop, d_drop + n, h.stream3);
  SAPCA_HIP(hipMemcpyAsync(h.stats_host.p, d_drop, (size_t)2 * n * sizeof(double), hipMemcpyDeviceToHost, h.stream3));
  SAPCA_HIP(hipEventRecord(h.ev_stats, h.stream3));
}

}  // namespace

template <typename T>
void Engine<T>::prepare(H& h, const CsrView<T>& A) {
  hipStream_t s = h.stream;
  if (!h.mask.empty() && (int64_t)h.mask.size() != A.cols)  // sparse_masked/mod.rs:258-262
    throw Error(SAPCA_ERR_MASK_LEN, "The mask vector length and the number of features (columns) have to be the same!");
  h.prep_key.valid = false;
  // A masked fit that failed after its prepare() (n_components check, SVD failure, no Lanczos convergence) leaves its
  // statistics chain queued on the third stream: that chain sorts in at_* and copies into the pinned statistics, which
  // every kind of fit reuses from here on.  Idle in the normal case.
  if (h.stream3) SAPCA_HIP(hipStreamSynchronize(h.stream3));
  h.stats_pending = false;
  h.stats_on_side = false;
  h.lz_scatter = false;

  const PrepPlan p = plan_preparation(h, A);
  const bool lz_scatter = p.at == AtFrom::Nothing;
  PrepOutcome<T> out;
  MaskMaps maps;
  Aside aside;   // (declared last: joined before anything above dies)
  mask_maps(h, p, maps);
  if (lz_scatter && !p.masked) {
    // max |a| for the fixed-point scales (masked fits: the compaction gathers it).  Values that are not finite turn the scale, and
    // with it every product and sum, into nan: the fit then fails to converge, as it does on the floating-point route.
    k::absmax(A.val, p.nnz, h.lz_scalars.as<unsigned long long>(4), s);
  }
  h.lz_scatter = lz_scatter;
  if (p.masked) compact_and_drop_sums(h, A, p, maps, out);
  if (p.masked || p.at == AtFrom::FormatFromA) start_a_format_aside(h, A, p, out, aside);
  if (p.at == AtFrom::FormatFromA || p.at == AtFrom::FormatFromCompacted) at_format_direct(h, A, p, maps, out);
  // (unmasked f64, or f32 off the bucket route: A's format is built on the side stream from this thread once the
  // transposition is queued; the side stream forks HERE, so the two run side by side on the GPU)
  const bool a_aside_late = p.tiled_ldp != 0 && !out.a_aside;
  if (a_aside_late) order_after(side_stream(h), h.ev_fork, s);   // A is ready on the main stream at this point
  if (!lz_scatter && !out.at_direct) at_transpose(h, A, p, maps, out);
  if (a_aside_late) {
    h.tiled_a = TiledOp();
    out.ok_a = k::build_tiled(A, p.tiled_ldp, h.tiled_a, h.tb_a, h.stream2, k::QuadSource::csr());
    SAPCA_HIP(hipEventRecord(h.ev_join, h.stream2));   // ...and the main stream waits for it at the end of prepare()
    out.a_aside = true;
  }

  column_statistics(h, A, p, out);
  // operator seen by the SVD engines (masked fits: the compacted pair, set above; Lanczos scatter: at_used is only a shape)
  if (!p.masked) {
    h.a_used = {p.m, p.n, p.nnz, A.ptr, A.idx, A.val};
    h.at_used = {p.n, p.m, p.nnz, out.At.ptr, out.At.idx, out.At.val};
  } else if (lz_scatter) {
    h.at_used = {p.n_used, p.m, out.nnz_used, nullptr, nullptr, nullptr};
  }

  build_formats(h, p, out, aside);
  aside.join();   // (fits without tile-major formats)
  if (out.a_aside) SAPCA_HIP(hipStreamWaitEvent(s, h.ev_join, 0));
  if (p.deliver == StatsTo::SideChain) queue_side_statistics(h, p, out, maps);

  h.prep_key = prep_key_of(h, A);
}

// R3: mean and total variance (sparse/mod.rs:106-131; masked :273-311, over cols_to_use only) from the column sums on the host
template <typename T>
void Engine<T>::finish_statistics(H& h) {
  const int64_t n = h.stats_cols;
  const double* sums = static_cast<const double*>(h.stats_host.p);
  const double mg = (double)h.m_global;
  const bool masked = h.has_mask_maps;
  h.prep_mean.assign((size_t)n, 0.0);
  h.prep_total_var = 0;
  if (h.opt.center) {
    for (int64_t j = 0; j < n; ++j) h.prep_mean[(size_t)j] = (double)(T)(sums[(size_t)j] / mg);
    auto var_of = [&](int64_t j) {
      const double mean = sums[(size_t)j] / mg;
      return (sums[(size_t)n + j] - mean * sums[(size_t)j]) / (mg - 1.0);
    };
    if (masked) for (uint64_t j : h.cols_to_use) h.prep_total_var += var_of((int64_t)j);
    else for (int64_t j = 0; j < n; ++j) h.prep_total_var += var_of(j);
  }
  // Q3 through two sweeps (A'W - P diag(mu) W, transform()) subtracts two f32 sums that cancel where stored values sit
  // close to their column's mean, i.e. in a well-filled column of small spread: (sum a)^2 / (m sum a^2) -> 1.  The
  // reference subtracts entry by entry (sparse_masked/mod.rs:488-494) and keeps those digits; above 1/4 the projection
  // takes the row kernel, which does the same.
  h.q3_cancels = false;
  if (h.opt.center && masked)
    for (uint64_t j : h.cols_to_use) {
      const double sj = sums[(size_t)j], qj = sums[(size_t)n + j];
      if (qj > 0 && sj * sj > 0.25 * mg * qj) { h.q3_cancels = true; break; }
    }
  h.stats_pending = false;
}

// ------------------------------------------------------------------------------------------
// R10: PowerIterationNormalizer on a rows x ld panel (CholeskyQR, f64 Gram on MFMA).
// ------------------------------------------------------------------------------------------
template <typename T>
void Engine<T>::normalize(H& h, T* P, int64_t rows, int l, int ld, int normalizer, bool sharded, const NormalizeExtras<T>& x) {
  // x.src: the panel is still as its producer left it (slabs of a split sweep, the centring term not yet subtracted): the
  // first Gram applies that on its way through.  x.vec_out: sum_r w[r] Q[r][:] of the normalised panel Q = P R^-1 -- the
  // centring vector of the sweep that reads Q next -- computed as R^-T (P^T w) from sums gathered in the Gram's read pass,
  // not from another pass over Q.
  hipStream_t s = h.stream;
  if (normalizer == SAPCA_NORM_NONE) {
    if (x.src) k::materialize(P, rows, ld, *x.src, s);
    if (x.vec_out) k::weighted_colsum(P, rows, ld, x.w, x.vec_out, h.scratch2, s);
    return;
  }
  Scope sc(h, C_ORTHO, x.behind_sweep);
  const SmallLayout lay(h.small, ld);
  double *G = lay.gram(), *wsum = x.vec_out ? lay.wsum() : nullptr;
  // QR -> CholeskyQR2 (orthonormal to working precision); LU -> one pass: a well-conditioned
  // basis of the same span, which is all the reference's LU normaliser provides.  Between power
  // iterations only the span matters (the next sweep re-mixes the basis), so the intermediate QR
  // normalisations run the single pass too (`passes` = 1); the final range basis Q and the
  // factorisation of B^T always get both passes.
  const int passes = x.passes > 0 ? x.passes : (normalizer == SAPCA_NORM_QR ? 2 : 1);
  for (int pass = 0; pass < passes; ++pass) {
    k::gram(P, rows, ld, G, h.scratch2, s, pass == 0 ? x.src : nullptr, x.w, wsum);
    if (sharded && h.comm.active()) { Scope cs(h, C_COMM); h.comm.allreduce(G, (uint64_t)ld * ld, 1, s); }
    double* Rout = pass == 0 ? x.R1 : x.R2;
    k::chol_inv(G, l, ld, Rout ? Rout : lay.r_scratch(), lay.r_inv(), lay.info(), s, wsum,
                sizeof(T) == 4 ? reinterpret_cast<float*>(x.vec_out) : nullptr, sizeof(T) == 8 ? reinterpret_cast<double*>(x.vec_out) : nullptr);
    // (R^-1 is upper triangular: its zero blocks are skipped; wide panels: block by block into a second panel, then back)
    T* Q = ld <= 128 ? P : h.panel_wide.as<T>((size_t)std::max<int64_t>(rows, 1) * ld);
    k::panel_gemm(P, rows, ld, lay.r_inv(), ld, Q, s, true);
    if (Q != P) SAPCA_HIP(hipMemcpyAsync(P, Q, (size_t)rows * ld * sizeof(T), hipMemcpyDeviceToDevice, s));
  }
}

template <typename T>
bool Engine<T>::vote_rides(const H& h) {
  return sizeof(T) == 4 && h.comm.active() && h.opt.method == SAPCA_RANDOM && h.opt.spmm_variant != 1 &&
         (size_t)h.comm.nranks + 2 <= H::kStatsTail;
}

template <typename T>
int64_t Engine<T>::piece_vote(H& h, int ld) {
  const char* ov = getenv("SAPCA_AT_OVERLAP");   // (read per fit: the tests switch it)
  const bool enabled = ov != nullptr ? atoi(ov) != 0 : h.comm.mode != Comm::RCCL;
  if (!enabled || !h.comm.has_side_lane() || !k::spmm_tiled_pieces_ok(h.tiled_at, 2, ld)) return 0;
  std::vector<int64_t> b;
  k::spmm_tiled_piece_bounds(h.tiled_at, 2, b, h.stream);
  return b[1];
}

// ------------------------------------------------------------------------------------------
// R7-R11, R13: randomized SVD of the (implicitly centred) prepared operator.
// ------------------------------------------------------------------------------------------
namespace {

// The route of a randomized fit: what fit_randomized() knows before it enqueues its first kernel -- all but the piece plan of
// the A^T sweep, which is agreed where its collective has always been queued (agree_on_at_pieces, behind the load of Omega).
//  panel ld          | taken by                                  | why
//  round_up(l, 16)   | one rank, l <= 128, row kernel            | the row kernel takes any multiple of 16
//  panel_ld(l, ldp)  | staged sweep, l > 128, or several ranks   | the tile geometry (64 / 128, above that multiples of 64).  ld enters the element
//                    |                                           | counts of the all-reduces, so with several ranks it must not depend on what a rank
//                    |                                           | decides locally (its entry count against the staged-sweep floor, whether its format
//                    |                                           | build succeeded): sharded fits always take this geometry, whichever kernel sweeps
//  A^T sweep         |                                           |
//  OnePiece          | one rank, f64, spmm_variant 1, or a vote  | one sweep, then one all-reduce of the panel (and the l column sums of Y behind it)
//                    | of 0 from any rank                        |
//  TwoPieces         | f32, several ranks, every rank voted > 0  | rows [0, cut) are all-reduced on stream_comm behind the first piece while the second
//                    |                                           | runs.  A rank votes > 0 (piece_vote) where the side stream has a lane of its own and
//                    |                                           | the path has run with several ranks: the callback / in-process transports.  Under
//                    |                                           | RCCL (the duplicate communicator made at init: two streams never issue on one
//                    |                                           | communicator) it is opt-in, SAPCA_AT_OVERLAP=1, until it has run on more than one
//                    |                                           | GPU; SAPCA_AT_OVERLAP=0 switches it off everywhere.  Whether a rank takes part is ITS
//                    |                                           | decision, so every rank votes and nobody waits in a collective a peer never joins.
//                    |                                           | The pieces are whole row blocks of a rank's operator and ranks cut their blocks
//                    |                                           | differently (the block count follows the shard's tile count): they agree on the
//                    |                                           | smallest first piece, so that every rank's collectives have the same sizes
//  small SVD         |                                           |
//  GramHost          | f32                                       | R11 through the l x l Gram of B^T: G = B B^T = Uh S^2 Uh^T (f64, MFMA + the host
//                    |                                           | eigensolver), vt = (B^T Uh S^-1)^T.  The Gram squares the condition number, so
//                    |                                           | sigma_i is good to eps_f64 (sigma_1/sigma_i)^2 relative: 1e-8 even for a 1e4 decay,
//                    |                                           | below what the f32 panels carry.  Saves two CholeskyQR passes over the n x l panel
//                    |                                           | and 0.4 ms of host time per fit against QrJacobi
//  GramHostHeldBack  | f32 fit_transform, unmasked, several      | the same, but fit() returns in front of the eigensolver and transform() runs it once
//                    | ranks or m * lw^2 <= 400e3 * 64^2         | the projection sweep is queued.  Where that pays: the rotation is one more m x l by
//                    | (lw = 64 for l_req <= 64, else 128)       | l x k panel product (0.2 ms per million rows at l <= 64, four times that at 128
//                    |                                           | columns) against a host stall of 0.25 ms (l = 60) to 1 ms (l = 110) -- C2 and the
//                    |                                           | shards of a strong-scaled fit gain 0.2 ms of a 9.5 ms step, a million rows on one GPU
//                    |                                           | would lose as much (measured, round 4).  Decided in fit() from what every rank sees
//                    |                                           | alike (m_global is not known there: a shard is about 1 / nranks of it)
//  GramDevice        | f32 under SAPCA_EIG_DEVICE=1              | opt-in experiment, slower (k::sym_eig_device_ok): one workgroup solves the
//                    |                                           | eigenproblem and writes M itself -- no wait for the host anywhere in the small SVD
//  QrJacobi          | f64                                       | R11 through a QR of B^T: B^T = Qz Rz, Rz = Ur S Vr^T  =>  vt = (Qz Ur)^T
//  covariates        |                                           |
//  cov               | sapca_set_covariates, basis of rank > 0   | the fit of R = (I - Q Q^T) A without forming it.  center is off for the sweeps (no c,
//                    | (one rank, SAPCA_RANDOM)                  | mu, 1^T Y): the intercept is a column of the design.  Before the iterations one A^T
//                    |                                           | sweep of the basis gives G = A^T Q; every A sweep is followed by Y -= Q (Q^T Y)
//                    |                                           | (covar.hip), every A^T sweep by X -= G (Q^T Y): with it X = A^T (I - Q Q^T) Y whatever
//                    |                                           | rounding left of Q in the normalised Y -- A^T amplifies that direction by |A^T Q| /
//                    |                                           | sigma_k, two orders of magnitude where a few columns carry a large offset.  The
//                    |                                           | A^T sweep sums its slabs itself (the correction needs X), and the small SVD is never
//                    |                                           | held back: the fit's host tail computes C = G^T V^T, which the projection reads
//  column scaling    |                                           |
//  scale             | sapca_set_column_scaling, SAPCA_RANDOM    | the fit of S = (A - 1 mu^T) D, D = diag(d), without forming it or touching A, the
//                    | (any rank count, masks, covariates with   | sweeps or the formats: only the n_used-row panels meet d (colscale.hip).  X <- D X in
//                    | explicit weights)                         | front of every A sweep (Omega included), its centring vector c = (D X)^T mu = X^T (D mu)
//                    |                                           | still from the Gram pass of X's normalisation (w = D mu in mu's place); behind every
//                    |                                           | A^T sweep -- and its all-reduce -- one finishing pass writes Z = D (sum of slabs -
//                    |                                           | mu sv^T) and the panel's next reader finds it plain.  A kernel of its own rather than
//                    |                                           | a row factor in PanelSource: gram() and materialize() stay byte for byte what an
//                    |                                           | unscaled fit runs.  With covariates G = A^T Q is scaled once to D G.  The small SVD is
//                    |                                           | never held back (the un-rotated projection would need D as well)
enum class AtSweep { OnePiece, TwoPieces };
enum class SmallSvd { GramHost, GramHostHeldBack, GramDevice, QrJacobi };

struct AtPieces {
  AtSweep sweep = AtSweep::OnePiece;
  int64_t cut = 0, r1 = 0;   // rows [0, cut) are all-reduced behind the first piece; this rank's second piece starts at r1 >= cut
  int wgs = 240;             // workgroups of a piece
};
struct RandomizedPlan {
  int64_t m = 0, n_used = 0;
  int l = 0, ld = 0, k = 0, ldk = 0, q = 0;
  int norm = 0, variant = 0;
  bool center = false, tiled = false;
  bool cov = false;          // the covariate route: uncentred sweeps around the projection by the basis Q (see "covariates" above)
  bool scale = false;        // the fit of (A - 1 mu^T) D (see "column scaling" above)
  SmallSvd small = SmallSvd::GramHost;
  AtPieces at;
};

// The panels of a fit and what its sweeps hand one another.
template <typename T>
struct FitPanels {
  T *X, *Y;                 // (n_used + 1) x ld (B^T; + one row: the column sums ride along in the all-reduce), m x ld
  SmallLayout lay;
  const T* mu;              // column means (null: no centring)
  T *cvec, *sv;             // c = X^T mu of sweep_a; the column sums 1^T Y of the A^T sweep
  bool cvec_current = false;   // the normaliser of X delivered c
  k::PanelSource<T> src;    // what the next pass over X still has to apply
  const T *d = nullptr, *dmu = nullptr;   // column scaling: the factors d and d mu in T (null: none)
};

// Enqueues nothing.
template <typename T>
RandomizedPlan plan_randomized(H& h) {
  RandomizedPlan p;
  p.m = h.a_used.rows; p.n_used = h.a_used.cols;
  p.k = (int)h.opt.n_components; p.ldk = (int)round_up(p.k, 16);
  const int64_t l_req = (int64_t)h.opt.n_components + (int64_t)h.opt.n_oversamples;
  p.l = (int)std::min<int64_t>(l_req, std::min<int64_t>((int64_t)h.m_global, p.n_used));
  SAPCA_CHECK(p.l <= k::kMaxPanelWidth, SAPCA_ERR_ARG, "n_components + n_oversamples above 1024 is not supported");
  p.tiled = h.tiled_a.valid && h.tiled_at.valid;
  p.ld = (p.l > 128 || p.tiled || h.comm.active()) ? panel_ld(p.l, p.tiled ? h.tiled_a.ldp : 0) : (int)round_up(p.l, 16);
  p.q = (int)h.opt.n_power_iterations; p.norm = h.opt.normalizer;
  p.cov = h.covar.active();
  p.scale = h.scale_fit != 0;
  p.center = h.opt.center != 0 && !p.cov;   // (covariates: the intercept of the design is the centring, the sweeps run uncentred)
  p.variant = h.opt.spmm_variant;
  p.small = sizeof(T) == 8 ? SmallSvd::QrJacobi : k::sym_eig_device_ok(p.l) ? SmallSvd::GramDevice
            : h.held_small.defer ? SmallSvd::GramHostHeldBack : SmallSvd::GramHost;
  return p;
}

// The piece plan of the A^T sweep.  The votes came with the column statistics when every rank had its A^T format by then (no
// extra collective, no host round trip here); otherwise one small all-reduce on the main stream and a wait for it.
template <typename T>
AtPieces agree_on_at_pieces(H& h, const RandomizedPlan& p) {
  AtPieces at;
  h.at_sweep_pieces = 1u;
  if (sizeof(T) != 4 || !h.comm.active() || p.variant == 1) return at;
  hipStream_t s = h.stream;
  // (only A^T's format matters for the pieces -- the vote may have been cast before A's own format was known to be built)
  const bool mine = h.tiled_at.valid && k::spmm_tiled_pieces_ok(h.tiled_at, 2, p.ld);
  if (h.vote_ready) {
    at.cut = h.vote_cut;
    SAPCA_CHECK(at.cut == 0 || mine, SAPCA_ERR_COMM, "internal: the ranks agreed on a two-piece A^T sweep this rank cannot run");
  } else {
    const uint32_t nr = h.comm.nranks;
    std::vector<double> votes((size_t)nr, 0.0);
    votes[h.comm.rank] = mine ? (double)Engine<T>::piece_vote(h, p.ld) : 0.0;
    double* d_votes = h.votes.as<double>(nr);
    SAPCA_HIP(hipMemcpyAsync(d_votes, votes.data(), nr * sizeof(double), hipMemcpyHostToDevice, s));
    h.comm.allreduce(d_votes, nr, 1, s);
    SAPCA_HIP(hipMemcpyAsync(votes.data(), d_votes, nr * sizeof(double), hipMemcpyDeviceToHost, s));
    SAPCA_HIP(hipStreamSynchronize(s));
    at.cut = (int64_t)*std::min_element(votes.begin(), votes.end());
  }
  if (!mine || at.cut <= 0 || at.cut >= p.n_used) return at;
  std::vector<int64_t> piece_rows;
  k::spmm_tiled_piece_bounds(h.tiled_at, 2, piece_rows, s);
  at.sweep = AtSweep::TwoPieces;
  at.r1 = piece_rows[1];
  h.at_sweep_pieces = 2u;
  hipDeviceProp_t pr;
  if (hipGetDeviceProperties(&pr, h.device) == hipSuccess) at.wgs = std::max(16, pr.multiProcessorCount - 16);   // (the collective keeps the rest)
  lazy_stream(h.stream_comm, h.ev_piece, h.ev_comm);
  return at;
}

// Omega into X: injected (parity tests; waits for the stream) or generated from the seed.
template <typename T>
void load_omega(H& h, const RandomizedPlan& p, FitPanels<T>& f) {
  hipStream_t s = h.stream;
  if (h.omega.empty()) {
    k::gaussian_panel(f.X, p.n_used, p.l, p.ld, h.opt.random_seed, s);
    return;
  }
  SAPCA_CHECK((int64_t)h.omega_rows == p.n_used && (int64_t)h.omega_cols >= p.l, SAPCA_ERR_ARG,
              "injected Omega must be (features seen by the SVD) x (n_components + n_oversamples)");
  std::vector<T> tmp((size_t)p.n_used * p.l);
  for (int64_t r = 0; r < p.n_used; ++r)
    for (int j = 0; j < p.l; ++j) tmp[(size_t)r * p.l + j] = (T)h.omega[(size_t)r * h.omega_cols + j];
  T* stage = h.scratch2.as<T>(tmp.size());
  SAPCA_HIP(hipMemcpyAsync(stage, tmp.data(), tmp.size() * sizeof(T), hipMemcpyHostToDevice, s));
  k::add_padding(stage, p.n_used, p.l, f.X, p.ld, s);
  SAPCA_HIP(hipStreamSynchronize(s));  // tmp goes out of scope
}

// Y = Ac X   (R8).  The centring vectors -- c = X^T mu here, the column sums 1^T Y of the A^T sweep -- belong to a panel that
// has just been normalised: normalize() delivers them from sums gathered in its Gram pass (vec_out), so no kernel re-reads
// the normalised panel for them; only the very first c (of Omega) is summed here.
// behind_normalize: the Scope of X's normalisation was the last thing on the stream (timings: see Scope).
template <typename T>
void sweep_a(H& h, const RandomizedPlan& p, FitPanels<T>& f, bool behind_normalize) {
  hipStream_t s = h.stream;
  if (p.scale) {   // X <- D X (a normalised X brought c = X^T (D mu) along: the same vector)
    Scope sc(h, C_ORTHO, behind_normalize);
    k::scale_panel_rows(f.X, p.n_used, p.ld, f.d, s);
  }
  if (p.center && !f.cvec_current) {
    k::weighted_colsum(f.X, p.n_used, p.ld, f.mu, f.cvec, h.scratch2, s);
    behind_normalize = false;
  }
  f.cvec_current = false;
  Scope sc(h, C_SPMM, behind_normalize);
  k::spmm(Engine<T>::view(h.a_used), &h.tiled_a, f.X, p.ld, f.Y, p.ld, p.ld, p.center ? f.cvec : nullptr, p.variant, h.split_scratch, s);
}

// ---- covariates: the three steps the route adds to a fit (RandomizedPlan's table) ----
template <typename T>
double* covar_s(H& h, int ld) { return h.covar_s.as<double>((size_t)k::kCovarCols * (size_t)std::max(ld, 16)); }

// Q on the device (m x 16, T) and G = A^T Q (n_used x 16, T).  Y carries the basis through the sweep as a panel of the fit's
// own width -- it is free until the first A sweep -- so the sweep is the one every iteration runs, tile-major formats included.
template <typename T>
void covar_basis_sweep(H& h, const RandomizedPlan& p, FitPanels<T>& f) {
  hipStream_t s = h.stream;
  constexpr int kq = k::kCovarCols;
  T* Q = h.covar_q.as<T>((size_t)p.m * kq);
  SAPCA_HIP(hipMemcpyAsync(Q, h.covar.q_t.data(), (size_t)p.m * kq * sizeof(T), hipMemcpyHostToDevice, s));   // (q_t: a member, alive)
  T* Gp = h.panel_xs.as<T>(((size_t)std::max<int64_t>(p.n_used, 1) + 1) * p.ld);
  T* G = h.covar_g.as<T>((size_t)p.n_used * kq);
  k::add_padding(Q, p.m, kq, f.Y, p.ld, s);
  {
    Scope sc(h, C_SPMMT);
    k::spmm(Engine<T>::view(h.at_used), &h.tiled_at, f.Y, p.ld, Gp, p.ld, p.ld, (const T*)nullptr, p.variant, h.split_scratch, s);
  }
  k::strip_padding(Gp, p.n_used, p.ld, kq, G, s);
  if (p.scale) k::scale_panel_rows(G, p.n_used, kq, f.d, s);   // D G: the A^T-side correction, C and trace(G^T G) are those of A D
}

// What the fitted model keeps of G once the components exist: C = G^T V^T (16 x ldc, f64, stays on the device for the
// projections) and G^T G (16 x 16, to the host: its trace is what the regression takes out of the total variance).  Both are
// panel_qt_y with G in the basis' place; V^T as the n_used x ldc panel project_with_components builds, too.
template <typename T>
void covar_model_products(H& h, const RandomizedPlan& p) {
  hipStream_t s = h.stream;
  constexpr int kq = k::kCovarCols;
  Scope sc(h, C_ORTHO);
  const int ldc = (int)round_up(p.k, p.k > 128 ? 64 : 16);
  h.covar.ldc = ldc;
  T* W = h.panel_w.as<T>((size_t)std::max<int64_t>(p.n_used, 1) * ldc);
  double* C = h.covar_c.as<double>((size_t)kq * ldc);
  double* GG = covar_s<T>(h, kq);
  const T* G = h.covar_g.ptr<T>();
  k::scaled_transpose(h.components_dev.ptr<T>(), p.n_used, p.k, nullptr, W, ldc, s);
  k::panel_qt_y(W, G, p.n_used, ldc, C, h.scratch2, s);
  k::panel_qt_y(G, G, p.n_used, kq, GG, h.scratch2, s);
  void* host = h.covar_host.ensure((size_t)kq * kq * sizeof(double));
  SAPCA_HIP(hipMemcpyAsync(host, GG, (size_t)kq * kq * sizeof(double), hipMemcpyDeviceToHost, s));
}

// P -= B (Q^T Y) for the m x ld panel Y: B = Q, P = Y behind an A sweep; B = G, P = X behind an A^T sweep.
template <typename T>
void covar_project(H& h, const RandomizedPlan& p, FitPanels<T>& f, bool behind_at) {
  Scope sc(h, C_ORTHO);
  double* S = covar_s<T>(h, p.ld);
  k::panel_qt_y(f.Y, h.covar_q.ptr<T>(), p.m, p.ld, S, h.scratch2, h.stream);
  if (behind_at) k::panel_sub_qs(f.X, h.covar_g.ptr<T>(), p.n_used, p.ld, p.ld, S, p.ld, h.stream);
  else k::panel_sub_qs(f.Y, h.covar_q.ptr<T>(), p.m, p.ld, p.ld, S, p.ld, h.stream);
}

// X = Ac^T Y   (R9); partial products are summed over ranks.  The panel is left as the sweep produced it: f.src says what the
// next pass over X -- the Gram of its normalisation, or of the small SVD -- still has to apply (slabs of a sweep whose tile
// range was split over workgroups, the centring term mu (1^T Y)^T; the normaliser of Y delivered 1^T Y into f.sv).
template <typename T>
void sweep_at_one_piece(H& h, const RandomizedPlan& p, FitPanels<T>& f, bool behind_normalize) {
  hipStream_t s = h.stream;
  f.src = k::PanelSource<T>();
  {
    Scope sc(h, C_SPMMT, behind_normalize);
    // (one rank: the slabs may stay unsummed; several: the collective needs the sum)
    k::spmm(Engine<T>::view(h.at_used), &h.tiled_at, f.Y, p.ld, f.X, p.ld, p.ld, (const T*)nullptr, p.variant, h.split_scratch, s,
            h.comm.active() || p.cov ? nullptr : &f.src);
  }
  if (!f.src.parts) { f.src.parts = f.X; f.src.nsplit = 1; }
  if (h.comm.active()) {
    Scope cs(h, C_COMM);
    h.comm.allreduce(f.X, (uint64_t)p.n_used * p.ld + (p.center ? (uint64_t)p.ld : 0), Engine<T>::kDtype, s);
  }
  if (p.center) { f.src.mu = f.mu; f.src.sv = f.sv; }
}

// ... in two pieces (f32, several ranks): the first piece's rows are all-reduced on stream_comm while the second piece runs.
template <typename T>
void sweep_at_two_pieces(H& h, const RandomizedPlan& p, FitPanels<T>& f) {
  if constexpr (sizeof(T) == 4) {
    hipStream_t s = h.stream;
    const int64_t cut = p.at.cut, r1 = p.at.r1;
    f.src = k::PanelSource<T>();
    {
      Scope sc(h, C_SPMMT);
      k::spmm_tiled_piece(h.tiled_at, 0, 2, p.at.wgs, 0, r1, f.Y, p.ld, f.X, p.ld, p.ld, h.split_scratch, s);
      SAPCA_HIP(hipEventRecord(h.ev_piece, s));
      k::spmm_tiled_piece(h.tiled_at, 1, 2, p.at.wgs, r1, p.n_used - r1, f.Y, p.ld, f.X, p.ld, p.ld, h.split_scratch2, s);
    }
    Scope cs(h, C_COMM);   // (device time from the first piece's collective being possible to the last one's end)
    SAPCA_HIP(hipStreamWaitEvent(h.stream_comm, h.ev_piece, 0));
    h.comm.allreduce(f.X, (uint64_t)cut * p.ld, Engine<T>::kDtype, h.stream_comm, 1);   // (cut <= r1: rows this rank has finished)
    SAPCA_HIP(hipEventRecord(h.ev_comm, h.stream_comm));
    h.comm.allreduce(f.X + (size_t)cut * p.ld, (uint64_t)(p.n_used - cut) * p.ld + (p.center ? (uint64_t)p.ld : 0), Engine<T>::kDtype, s);
    SAPCA_HIP(hipStreamWaitEvent(s, h.ev_comm, 0));
    f.src.parts = f.X; f.src.nsplit = 1;
    if (p.center) { f.src.mu = f.mu; f.src.sv = f.sv; }
  }
}

// behind_normalize: the Scope of Y's normalisation was the last thing on the stream (timings: see Scope).
template <typename T>
void sweep_at(H& h, const RandomizedPlan& p, FitPanels<T>& f, bool behind_normalize) {
  p.at.sweep == AtSweep::TwoPieces ? sweep_at_two_pieces(h, p, f) : sweep_at_one_piece(h, p, f, behind_normalize);
  if (p.scale) {   // Z = D (sum of slabs - mu sv^T), behind the all-reduce: the panel is plain from here on
    Scope sc(h, C_ORTHO);
    k::finish_scaled_panel(f.X, p.n_used, p.ld, f.src, f.d, h.stream);
    f.src = k::PanelSource<T>();
    f.src.parts = f.X; f.src.nsplit = 1;
  }
  if (p.cov) covar_project(h, p, f, true);
}

// R8-R10: q power iterations, then Q = qr(Ac X) and X = B^T = Ac^T Q (n_used x l), completed by the small SVD's first pass.
template <typename T>
void power_iterations(H& h, const RandomizedPlan& p, FitPanels<T>& f) {
  using Extras = NormalizeExtras<T>;
  T* const sv_out = p.center ? f.sv : nullptr;
  // Timings: sweep -> normalise -> sweep, each Scope opening at the event that closed the one before wherever nothing is
  // queued between the two.  (A normaliser of NONE opens no Scope; covariates, column scaling and collectives queue work of
  // their own behind a sweep.)
  const bool y_behind = !p.cov, x_behind = !p.cov && !p.scale && !h.comm.active() && p.at.sweep != AtSweep::TwoPieces;
  const bool normalises = p.norm != SAPCA_NORM_NONE;
  for (int it = 0; it < p.q; ++it) {
    sweep_a(h, p, f, it > 0 && normalises);
    if (p.cov) covar_project(h, p, f, false);
    Engine<T>::normalize(h, f.Y, p.m, p.l, p.ld, p.norm, true, Extras{.passes = 1, .vec_out = sv_out, .behind_sweep = y_behind});
    sweep_at(h, p, f, normalises);
    Engine<T>::normalize(h, f.X, p.n_used, p.l, p.ld, p.norm, false,
                         Extras{.passes = 1, .src = &f.src, .w = p.scale ? f.dmu : f.mu, .vec_out = p.center ? f.cvec : nullptr,
                                .behind_sweep = x_behind});
    f.cvec_current = p.center;
  }
  sweep_a(h, p, f, p.q > 0 && normalises);
  if (p.cov) covar_project(h, p, f, false);
  Engine<T>::normalize(h, f.Y, p.m, p.l, p.ld, SAPCA_NORM_QR, true, Extras{.vec_out = sv_out, .behind_sweep = y_behind});   // Q = qr(Y): always orthonormal
  sweep_at(h, p, f, true);
}

}  // namespace

// vt = (B^T M)^T with the sign convention of svd_flip (R13): the components, from an un-rotated panel X = B^T (n x ld) and
// the small factor M (ld x ldk, ldk = round_up(k, 16)) of whichever small SVD produced it.  A fit passes panel_x and its
// n_used rows; sapca_rotate_panel_* a caller's panel.  sign_out: the device address of the k flip signs.
template <typename T>
void Engine<T>::rotate_into_components(H& h, const T* X, int64_t n, int ld, int k, const double* Mdev, const double** sign_out) {
  const int ldk = (int)round_up(k, 16);
  T* VtT = h.panel_w.as<T>((size_t)std::max<int64_t>(n, 1) * ldk);
  k::panel_gemm(X, n, ld, Mdev, ldk, VtT, h.stream);
  T* comps = h.components_dev.as<T>((size_t)k * std::max<int64_t>(n, 1));
  k::flip_transpose(VtT, n, ldk, k, comps, h.scratch2, h.stream, sign_out);
}

namespace {

// GramDevice: the eigenproblem stays on the device (one workgroup, parallel Jacobi: sym_eig.hip).  The singular values (and the
// solver's status) cross in page-locked memory behind everything else; finish_fit() reads them after the fit's last wait.
template <typename T>
void small_svd_gram_device(H& h, const RandomizedPlan& p, FitPanels<T>& f) {
  hipStream_t s = h.stream;
  Scope sc(h, C_SMALL);
  k::gram(f.X, p.n_used, p.ld, f.lay.gram(), h.scratch2, s, &f.src);
  double* d_sigma = f.lay.r_inv();   // (the normaliser's R^-1 slot: free here)
  int* d_status = reinterpret_cast<int*>(d_sigma + p.ld);
  k::sym_eig_device(f.lay.gram(), p.l, p.ld, p.k, p.ldk, f.lay.m(), d_sigma, d_status, s);
  double* host = static_cast<double*>(h.small_host.ensure(((size_t)p.l + 4) * sizeof(double)));
  int* host_i = reinterpret_cast<int*>(host + p.l);
  SAPCA_HIP(hipMemcpyAsync(host, d_sigma, (size_t)p.l * sizeof(double), hipMemcpyDeviceToHost, s));
  SAPCA_HIP(hipMemcpyAsync(host_i, d_status, 2 * sizeof(int), hipMemcpyDeviceToHost, s));
  SAPCA_HIP(hipMemcpyAsync(host_i + 2, f.lay.info(), sizeof(int), hipMemcpyDeviceToHost, s));
  Engine<T>::rotate_into_components(h, f.X, p.n_used, p.ld, p.k, f.lay.m());
  h.held_tail.sing_l = p.l;
}

// GramHost / GramHostHeldBack: the Gram to the host in page-locked staging owned by the handle -- G comes back and M goes
// out without the runtime's bounce buffers, and M outlives this call: nothing waits for the device after the eigensolver.
template <typename T>
void small_svd_gram_host(H& h, const RandomizedPlan& p, FitPanels<T>& f) {
  hipStream_t s = h.stream;
  Scope sc(h, C_SMALL);
  k::gram(f.X, p.n_used, p.ld, f.lay.gram(), h.scratch2, s, &f.src);
  const size_t g_len = (size_t)p.ld * p.ld, m_len = (size_t)p.ld * p.ldk;
  double* g = static_cast<double*>(h.small_host.ensure((g_len + m_len + 2) * sizeof(double)));
  int* info_pinned = reinterpret_cast<int*>(g + g_len + m_len);
  SAPCA_HIP(hipMemcpyAsync(g, f.lay.gram(), g_len * sizeof(double), hipMemcpyDeviceToHost, s));
  SAPCA_HIP(hipMemcpyAsync(info_pinned, f.lay.info(), sizeof(int), hipMemcpyDeviceToHost, s));
  h.held_small.l = p.l;
  h.held_small.ld = p.ld;
  if (p.small == SmallSvd::GramHostHeldBack) {
    if (!h.held_small.ev) SAPCA_HIP(hipEventCreateWithFlags(&h.held_small.ev, hipEventDisableTiming));
    SAPCA_HIP(hipEventRecord(h.held_small.ev, s));
    h.held_small.pending = true;
    return;
  }
  Engine<T>::finish_small_svd(h, nullptr);
}

// QrJacobi: two CholeskyQR passes over X, the product of their factors to the host, Jacobi there.  Waits for the stream twice.
template <typename T>
void small_svd_qr_jacobi(H& h, const RandomizedPlan& p, FitPanels<T>& f) {
  hipStream_t s = h.stream;
  const int l = p.l, ld = p.ld;
  int info_host = 0;
  std::vector<double> r1((size_t)ld * ld), r2((size_t)ld * ld);
  {
    Scope sc(h, C_SMALL);
    Engine<T>::normalize(h, f.X, p.n_used, l, ld, SAPCA_NORM_QR, false, NormalizeExtras<T>{.R1 = f.lay.r1(), .R2 = f.lay.r2(), .src = &f.src});
    SAPCA_HIP(hipMemcpyAsync(r1.data(), f.lay.r1(), r1.size() * sizeof(double), hipMemcpyDeviceToHost, s));
    SAPCA_HIP(hipMemcpyAsync(r2.data(), f.lay.r2(), r2.size() * sizeof(double), hipMemcpyDeviceToHost, s));
    SAPCA_HIP(hipMemcpyAsync(&info_host, f.lay.info(), sizeof(int), hipMemcpyDeviceToHost, s));
    SAPCA_HIP(hipStreamSynchronize(s));
    std::vector<double> Rz((size_t)l * l, 0.0), Ur, sv;
    for (int i = 0; i < l; ++i)
      for (int j = i; j < l; ++j) {
        double acc = 0;
        for (int t = i; t <= j; ++t) acc += r2[(size_t)i * ld + t] * r1[(size_t)t * ld + j];
        Rz[(size_t)i * l + j] = acc;
      }
    const auto tj0 = std::chrono::steady_clock::now();
    jacobi_svd(Rz, l, Ur, sv);
    if (h.opt.verbose)
      fprintf(stderr, "sapca: host Jacobi SVD of the %d x %d factor: %.3f ms\n", l, l,
              std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tj0).count());
    for (int i = 0; i < l; ++i)
      SAPCA_CHECK(std::isfinite(sv[i]), SAPCA_ERR_SVD, "Randomized SVD computation failed: non-finite singular value");
    std::vector<double> M((size_t)ld * p.ldk, 0.0);
    for (int i = 0; i < l; ++i)
      for (int j = 0; j < p.k; ++j) M[(size_t)i * p.ldk + j] = Ur[(size_t)i * l + j];
    SAPCA_HIP(hipMemcpyAsync(f.lay.m(), M.data(), M.size() * sizeof(double), hipMemcpyHostToDevice, s));
    Engine<T>::rotate_into_components(h, f.X, p.n_used, ld, p.k, f.lay.m());
    SAPCA_HIP(hipStreamSynchronize(s));   // M goes out of scope
    h.sing.assign(sv.begin(), sv.begin() + p.k);
  }
  h.chol_regularised = info_host;
}

}  // namespace

template <typename T>
void Engine<T>::fit_randomized(H& h) {
  RandomizedPlan p = plan_randomized<T>(h);
  T* X = h.panel_x.as<T>(((size_t)std::max<int64_t>(p.n_used, 1) + 1) * p.ld);
  T* Y = h.panel_y.as<T>((size_t)std::max<int64_t>(p.m, 1) * p.ld);
  const SmallLayout lay(h.small, p.ld);
  // one collective carries the l column sums of this rank's Y too: they live in the row behind the panel then
  T* sv = h.comm.active() ? X + (size_t)p.n_used * p.ld : lay.s<T>();
  FitPanels<T> f{X, Y, lay, p.center ? h.mean_used_dev.ptr<T>() : nullptr, lay.c<T>(), sv};
  if (p.scale) { f.d = h.scale_dt.ptr<T>(); f.dmu = h.scale_w.ptr<T>(); }
  SAPCA_HIP(hipMemsetAsync(lay.info(), 0, sizeof(int), h.stream));
  load_omega(h, p, f);
  p.at = agree_on_at_pieces<T>(h, p);   // (several ranks: a collective and a host wait, at this point of the stream)
  if (p.cov) covar_basis_sweep(h, p, f);
  power_iterations(h, p, f);
  switch (p.small) {
    case SmallSvd::GramDevice: small_svd_gram_device(h, p, f); break;
    case SmallSvd::QrJacobi: small_svd_qr_jacobi(h, p, f); break;
    default: small_svd_gram_host(h, p, f); break;
  }
  if (p.cov) covar_model_products<T>(h, p);   // (the components exist: with covariates no small SVD is held back)
}

// R11 (f32), host half: eigen-decomposition of the l x l Gram staged in small_host by small_svd_gram_host, the factor
// M = Uh S^-1 back to the device, then the components.  Called at the end of the fit, or -- fit_transform,
// `held_small.pending` -- from transform() once the projection sweep is queued.  sign_out: see rotate_into_components.
template <typename T>
void Engine<T>::finish_small_svd(H& h, const double** sign_out) {
  hipStream_t s = h.stream;
  const bool deferred = h.held_small.pending;
  h.held_small.pending = false;
  const int l = h.held_small.l, ld = h.held_small.ld, k = (int)h.opt.n_components;
  const int ldk = (int)round_up(k, 16);
  const SmallLayout lay(h.small, ld);
  try {
    std::unique_ptr<Scope> sc(deferred ? new Scope(h, C_SMALL) : nullptr);   // (not deferred: inside the fit's own span)
    if (sc && sc->ev >= 0) h.held_small.in_transform.push_back(sc->ev);       // (it lies inside the projection's span: taken out of transform_ms)
    double* g = static_cast<double*>(h.small_host.p);
    double* M = g + (size_t)ld * ld;
    const int* info_pinned = reinterpret_cast<const int*>(M + (size_t)ld * ldk);
    if (deferred) SAPCA_HIP(hipEventSynchronize(h.held_small.ev));
    else SAPCA_HIP(hipStreamSynchronize(s));
    const int info_host = *info_pinned;
    std::vector<double> Gl((size_t)l * l), w, Vt;
    for (int i = 0; i < l; ++i)
      for (int j = 0; j < l; ++j) Gl[(size_t)i * l + j] = g[(size_t)i * ld + j];
    const auto tj0 = std::chrono::steady_clock::now();
    SAPCA_CHECK(sym_eigh_desc(Gl, l, w, Vt), SAPCA_ERR_SVD, "Randomized SVD computation failed: eigensolver did not converge");
    if (h.opt.verbose)
      fprintf(stderr, "sapca: host eigensolver of the %d x %d Gram: %.3f ms\n", l, l,
              std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tj0).count());
    std::vector<double> sv((size_t)l);
    for (int i = 0; i < l; ++i) {
      SAPCA_CHECK(std::isfinite(w[i]), SAPCA_ERR_SVD, "Randomized SVD computation failed: non-finite singular value");
      sv[i] = std::sqrt(std::max(w[i], 0.0));
    }
    std::fill(M, M + (size_t)ld * ldk, 0.0);
    const double tiny = sv[0] * 1e-12;
    for (int j = 0; j < k; ++j) {
      if (!(sv[j] > tiny)) continue;   // numerically rank-deficient direction: a zero component, sigma ~ 0
      const double inv = 1.0 / sv[j];
      for (int i = 0; i < l; ++i) M[(size_t)i * ldk + j] = Vt[(size_t)j * l + i] * inv;
    }
    SAPCA_HIP(hipMemcpyAsync(lay.m(), M, (size_t)ld * ldk * sizeof(double), hipMemcpyHostToDevice, s));
    rotate_into_components(h, h.panel_x.ptr<T>(), h.a_used.cols, ld, k, lay.m(), sign_out);
    h.sing.assign(sv.begin(), sv.begin() + k);
    h.chol_regularised = info_host;
  } catch (...) {
    if (deferred) {   // the fit had been reported as done: take that back
      h.fitted = false;
      h.held_tail.pending = false;
    }
    throw;
  }
}

// ------------------------------------------------------------------------------------------
// R12: Lanczos on the raw operator (no centring: quirk Q1); centred: on A - 1 mu^T, mu in h.lz_mu (opt-in, lanczos.hip).
// ------------------------------------------------------------------------------------------
template <typename T>
void Engine<T>::fit_lanczos(H& h, bool centred) {
  Scope sc(h, C_LANCZOS);
  lanczos_fit<T>(h, centred);
}

// ------------------------------------------------------------------------------------------
// covariates (sapca_set_covariates): what a fit or a transform settles on the host before it enqueues anything
// ------------------------------------------------------------------------------------------
void covar_check(H& h, uint64_t m, bool fit, bool then_transform) {
  const bool set = !h.covar_z.empty();
  const bool model = h.covar.model.design > 0;
  if (!fit) {
    if (!h.fitted || (!set && !model)) return;   // (not fitted: the reference's own error follows; neither: nothing to do)
    SAPCA_CHECK(model, SAPCA_ERR_ARG, "transform: covariates are set, but the model was fitted without covariates");
    SAPCA_CHECK(set, SAPCA_ERR_ARG, "transform: the model was fitted with covariates, but none are set");
    SAPCA_CHECK(h.covar_cols == h.covar.model.cols, SAPCA_ERR_ARG,
                "transform: covariates have " + std::to_string(h.covar_cols) + " columns, the fitted model's " + std::to_string(h.covar.model.cols));
  }
  if (!set) return;
  SAPCA_CHECK(!h.comm.active(), SAPCA_ERR_ARG, "covariates are not supported on a handle that belongs to a communicator");
  SAPCA_CHECK(h.opt.method == SAPCA_RANDOM, SAPCA_ERR_ARG, "covariates need SVDMethod::Random");
  SAPCA_CHECK(!(then_transform || !fit) || h.opt.transform_semantics == SAPCA_TRANSFORM_CENTERED, SAPCA_ERR_ARG,
              "covariates need SAPCA_TRANSFORM_CENTERED: the reference's transform semantics have no meaning on residuals");
  SAPCA_CHECK(h.covar_rows == m, SAPCA_ERR_ARG,
              "covariates have " + std::to_string(h.covar_rows) + " rows, the matrix " + std::to_string(m));
}

// ------------------------------------------------------------------------------------------
// column scaling (sapca_set_column_scaling): what a fit or a transform settles on the host before it enqueues anything
// ------------------------------------------------------------------------------------------
void scale_check(H& h, uint64_t m, uint64_t n, bool fit, bool then_transform) {
  const int mode = fit ? h.scale_mode : (h.fitted ? h.scale_model : 0);
  if (mode == SAPCA_SCALE_NONE) return;
  if (fit) {
    SAPCA_CHECK(h.opt.method == SAPCA_RANDOM, SAPCA_ERR_ARG, "column scaling needs SVDMethod::Random");
    if (mode == SAPCA_SCALE_WEIGHTS)
      SAPCA_CHECK(h.scale_weights.size() == n, SAPCA_ERR_ARG,
                  "column scaling has " + std::to_string(h.scale_weights.size()) + " weights, the matrix " + std::to_string(n) + " columns");
    if (mode == SAPCA_SCALE_UNIT_VARIANCE) {
      SAPCA_CHECK(m >= 2 || h.comm.active(), SAPCA_ERR_ARG,
                  "column scaling: unit variance needs at least two rows, the matrix has " + std::to_string(m));
      SAPCA_CHECK(h.covar_z.empty(), SAPCA_ERR_ARG,
                  "column scaling: unit variance of covariate residuals is not supported (" + std::to_string(h.covar_cols) +
                      " covariate columns are set): pass explicit weights");
    }
  }
  SAPCA_CHECK(!(then_transform || !fit) || h.opt.transform_semantics == SAPCA_TRANSFORM_CENTERED, SAPCA_ERR_ARG,
              "column scaling needs SAPCA_TRANSFORM_CENTERED: the reference's transform semantics have no meaning on scaled columns");
}

namespace {

// The factors of this fit on the device, from the column sums prepare() left there (all-reduced on a communicator, so every
// rank derives the same d): d in f64 and T, d mu in T, and sum_j d_j^2 var_j on its way to the host tail.  Main stream, no wait.
template <typename T>
void column_scale_factors(H& h, int64_t n_used) {
  hipStream_t s = h.stream;
  const int64_t n = h.stats_cols;
  const double* weights = nullptr;
  if (h.scale_fit == SAPCA_SCALE_WEIGHTS) {   // (scale_weights: a member, alive while the copy reads it)
    double* w = h.scale_in.as<double>((size_t)std::max<int64_t>(n, 1));
    SAPCA_HIP(hipMemcpyAsync(w, h.scale_weights.data(), (size_t)n * sizeof(double), hipMemcpyHostToDevice, s));
    weights = w;
  }
  const size_t cap = (size_t)std::max<int64_t>(n_used, 1), parts = k::column_scale_partials(n_used);
  double* red = h.scale_red.as<double>(parts + 1);
  const double* stats = h.stats.ptr<double>();
  k::column_scale_factors<T>(stats, stats + n, (double)h.m_global, h.has_mask_maps ? h.sel_rows_dev.ptr<int32_t>() : nullptr, weights, n_used,
                             h.scale_d64.as<double>(cap), h.scale_dt.as<T>(cap), h.scale_w.as<T>(cap), red, red + parts, s);
  void* host = h.scale_host.ensure(sizeof(double));
  SAPCA_HIP(hipMemcpyAsync(host, red + parts, sizeof(double), hipMemcpyDeviceToHost, s));
}

// the orthonormal basis Q of this fit's design and the map W (Q = D W), on the host; Q rounded to T for the device
template <typename T>
void covar_fit_basis(H& h) {
  constexpr size_t kq = k::kCovarCols;
  H::Covar& c = h.covar;
  c.fit = {};
  if (h.covar_z.empty()) return;
  const size_t m = (size_t)h.covar_rows, design = (size_t)h.covar_cols + (h.opt.center ? 1 : 0);
  c.q.resize(m * kq);
  c.w.resize(design * kq);
  uint64_t rank = 0;
  SAPCA_CHECK(sapca_covariate_basis(h.covar_z.data(), h.covar_rows, h.covar_cols, h.opt.center ? 1 : 0, c.q.data(), c.w.data(), &rank) == SAPCA_OK,
              SAPCA_ERR_ARG, "covariates: the design matrix was refused");
  c.fit = {h.covar_cols, (uint64_t)design, rank};
  c.q_t.resize(m * kq * sizeof(T));
  T* qt = reinterpret_cast<T*>(c.q_t.data());
  for (size_t i = 0; i < m * kq; ++i) qt[i] = (T)c.q[i];
}

// Q_rows = D_rows W of the fitted model for the rows of the covariates set now, rounded to T (transform)
template <typename T>
void covar_rows_basis(H& h) {
  constexpr size_t kq = k::kCovarCols;
  H::Covar& c = h.covar;
  const size_t m = (size_t)h.covar_rows, cols = (size_t)h.covar_cols, off = h.opt.center ? 1 : 0;
  c.q_t.resize(m * kq * sizeof(T));
  T* qt = reinterpret_cast<T*>(c.q_t.data());
  for (size_t i = 0; i < m; ++i)
    for (size_t j = 0; j < kq; ++j) {
      double acc = off ? c.w_model[j] : 0.0;
      for (size_t t = 0; t < cols; ++t) acc += h.covar_z[i * cols + t] * c.w_model[(off + t) * kq + j];
      qt[i * kq + j] = (T)acc;
    }
}

// The host tail of a fit with covariates: W for the projections to come and, for center = 1, the total variance of the
// residual, sum_j (sumsq_j - |G_j|^2) / (m - 1) over the columns the fit used; sum_j |G_j|^2 = trace(G^T G), which
// covar_model_products sent to covar_host.  The caller has waited for the stream.
void covar_finish_fit(H& h) {
  constexpr size_t kq = k::kCovarCols;
  H::Covar& c = h.covar;
  if (c.fit.design == 0) return;
  c.w_model = c.w;
  if (!c.active() || !h.opt.center) return;
  const double* GG = static_cast<const double*>(h.covar_host.p);
  const double* sums = static_cast<const double*>(h.stats_host.p);
  const size_t n = (size_t)h.stats_cols;
  double raw = 0, taken = 0;
  // (column scaling, explicit weights only on this route: the raw second moment of A D; G is D G already)
  const bool scaled = h.scale_model == SAPCA_SCALE_WEIGHTS && h.scale_weights.size() == n;
  auto moment = [&](size_t j) { return scaled ? h.scale_weights[j] * h.scale_weights[j] * sums[n + j] : sums[n + j]; };
  if (h.has_mask_maps) for (uint64_t j : h.cols_to_use) raw += moment((size_t)j);
  else for (size_t j = 0; j < n; ++j) raw += moment(j);
  for (size_t i = 0; i < kq; ++i) taken += GG[i * kq + i];
  h.total_var = (raw - taken) / (double)(h.m_fit - 1);
}

}  // namespace

// ------------------------------------------------------------------------------------------
// fit
// ------------------------------------------------------------------------------------------
template <typename T>
void Engine<T>::fit(H& h, const CsrView<T>& A, bool defer_finish) {
  hipStream_t s = h.stream;
  covar_check(h, (uint64_t)A.rows, true, false);   // (first: a refused fit leaves the handle as it was)
  scale_check(h, (uint64_t)A.rows, (uint64_t)A.cols, true, false);
  h.scale_fit = h.scale_mode;
  h.held_tail.reset();
  h.held_small.reset();
  covar_fit_basis<T>(h);
  {
    // GramHostHeldBack (RandomizedPlan's route table has the break-even)
    const double lw = (double)(h.opt.n_components + h.opt.n_oversamples) <= 64 ? 64.0 : 128.0;
    h.held_small.defer = defer_finish && h.mask.empty() && h.opt.method == SAPCA_RANDOM && sizeof(T) == 4 &&
                         (h.comm.active() || (double)A.rows * lw * lw <= 400e3 * 64.0 * 64.0) && !h.covar.active() && h.scale_fit == 0;
  }
  h.spans.clear();
  h.comm.host_ms = 0;
  h.timer.begin_collect(s, h.opt.collect_timings != 0);
  const int total_ev = h.timer.start();
  h.fitted = false;
  h.timings.lanczos_steps = 0;
  SAPCA_CHECK(h.opt.n_components > 0, SAPCA_ERR_ARG, "n_components must be positive");
  SAPCA_CHECK(A.rows > 0 && A.cols > 0, SAPCA_ERR_ARG, "empty matrix");
  prepare(h, A);   // (throws where the mask selects no feature)
  const int64_t n_used = h.a_used.cols;
  if ((int64_t)h.opt.n_components > std::min<int64_t>((int64_t)h.m_global - (int64_t)h.covar.fit.rank, n_used))
    throw Error(SAPCA_ERR_SVD, std::string(h.opt.method == SAPCA_RANDOM ? "Randomized SVD" : "SVD") +
                                   " computation failed: n_components exceeds the matrix dimensions");
  SAPCA_CHECK(h.m_global >= 2, SAPCA_ERR_ARG, "need at least two samples");

  // column means of the features the SVD sees, in T (the centring vector of the sweeps and of transform)
  auto device_means = [&] {
    T* d_mu = h.mean_used_dev.as<T>((size_t)n_used);
    if (h.opt.center)
      k::mean_from_sums(h.stats.ptr<double>(), (double)h.m_global, h.has_mask_maps ? h.sel_rows_dev.ptr<int32_t>() : nullptr, n_used, d_mu, s);
    else
      SAPCA_HIP(hipMemsetAsync(d_mu, 0, (size_t)n_used * sizeof(T), s));
  };

  if (h.opt.method == SAPCA_RANDOM) {
    device_means();
    if (h.scale_fit) column_scale_factors<T>(h, n_used);
    fit_randomized(h);
  } else {
    // the Lanczos branch does not centre (Q1) unless asked to: only transform reads the means.  On the scatter route the
    // column sums arrive from the third stream, beside the iterations: the main stream meets them here, behind the last step
    // -- or, for a centred fit (lanczos_center, opt-in), in front of the first one: its operator is A - 1 mu^T.  That mu is
    // f64 straight from the f64 column sums (all n-sized Lanczos data is f64; the T-rounded means of the sweeps would leave
    // an operator that is not symmetric to working precision where the mean term dwarfs sigma_k)
    const bool centred = h.opt.lanczos_center != 0 && h.opt.center != 0;
    const bool sums_on_side = h.lz_scatter && h.stats_on_side;
    const bool means_first = !sums_on_side || centred;
    if (sums_on_side && centred) SAPCA_HIP(hipStreamWaitEvent(s, h.ev_stats, 0));
    if (means_first) device_means();
    if (centred)
      k::mean_from_sums(h.stats.ptr<double>(), (double)h.m_global, h.has_mask_maps ? h.sel_rows_dev.ptr<int32_t>() : nullptr, n_used,
                        h.lz_mu.as<double>((size_t)n_used), s);
    fit_lanczos(h, centred);
    if (!means_first) {
      SAPCA_HIP(hipStreamWaitEvent(s, h.ev_stats, 0));
      device_means();
    }
  }

  h.k = h.opt.n_components;
  h.n_used = (uint64_t)n_used;
  h.n_cols = (uint64_t)A.cols;
  h.m_fit = h.m_global;
  h.dtype = kDtype;
  h.fitted = true;
  h.scale_model = h.scale_fit;
  h.covar.model = h.covar.fit;   // (now, not in the tail: a held-back tail runs behind the projection, whose checks read this)
  h.timer.stop(total_ev);
  h.held_tail.total_ev = total_ev;
  h.held_tail.pending = true;
  // fit_transform: the host-side tail (statistics, timings: two waits for the device) runs once the projection is queued --
  // the model the projection reads is all on the device by now
  // (masked fits finish first: their projection asks the finished statistics whether its two sweeps would cancel, Q3)
  // (covariates: the projection reads C = G^T V^T, which the tail computes)
  if (!defer_finish || !h.mask.empty() || h.covar.fit.design > 0) finish_fit(h);
}

namespace {

// What swept, for sapca_timings: ALGORITHMIC bytes of one sparse x dense sweep, the kernel, the pieces, the formats' slots.
template <typename T>
void describe_sweeps(H& h) {
  const int64_t n_used = (int64_t)h.n_used;
  const double l = (double)std::min<uint64_t>(h.opt.n_components + h.opt.n_oversamples, std::min<uint64_t>(h.m_global, (uint64_t)n_used));
  h.timings.bytes_per_sweep = (double)h.a_used.nnz * (sizeof(T) + 4) + ((double)h.a_used.rows + 1) * 8 +
                              (double)n_used * l * sizeof(T) + (double)h.a_used.rows * l * sizeof(T);
  const bool tiled = h.opt.method == SAPCA_RANDOM && h.tiled_a.valid && h.tiled_at.valid;
  h.timings.sweep_kernel = !tiled ? 0u : (k::dq_usable(h.tiled_a, 64) && k::dq_usable(h.tiled_at, 64) && h.opt.spmm_variant != 1 ? 2u : 1u);
  h.timings.at_sweep_pieces = h.opt.method == SAPCA_RANDOM ? h.at_sweep_pieces : 0u;
  h.timings.sweep_slots_a = tiled ? (uint64_t)h.tiled_a.total_entries : 0;
  h.timings.sweep_slots_at = tiled ? (uint64_t)h.tiled_at.total_entries : 0;
}

}  // namespace

template <typename T>
void Engine<T>::finish_fit(H& h) {
  if (!h.held_tail.pending) return;
  if (h.held_small.pending) finish_small_svd(h, nullptr);   // (a projection that failed before it reached the held-back half)
  h.held_tail.pending = false;
  hipStream_t s = h.stream;
  const int total_ev = h.held_tail.total_ev;
  if (h.held_tail.sing_l) {   // the device eigensolver's singular values and status (small_svd_gram_device)
    const int l = h.held_tail.sing_l;
    h.held_tail.sing_l = 0;
    SAPCA_HIP(hipStreamSynchronize(s));
    const double* host = static_cast<const double*>(h.small_host.p);
    const int* host_i = reinterpret_cast<const int*>(host + l);
    bool finite = true;
    for (int i = 0; i < l; ++i) finite = finite && std::isfinite(host[i]);
    if ((host_i[0] & 1) || (host_i[0] & 2) || !finite) {
      h.fitted = false;
      throw Error(SAPCA_ERR_SVD, (host_i[0] & 1) ? "Randomized SVD computation failed: eigensolver did not converge"
                                                 : "Randomized SVD computation failed: non-finite singular value");
    }
    if (h.opt.verbose) fprintf(stderr, "sapca: device eigensolver of the %d x %d Gram: %d sweeps\n", l, l, host_i[1]);
    h.sing.assign(host, host + h.k);
    h.chol_regularised = host_i[2];
  }
  // sparse/mod.rs:106-117: mean_ = col_sums / n when centring, zeros otherwise (the reference
  // allocates zeros(n_samples) there -- a length bug that is never read; n_cols zeros here).
  if (h.stats_pending) {   // (the copy was queued in prepare(); every path through the SVD engines has synchronised since)
    SAPCA_HIP(hipStreamSynchronize(s));
    if (h.stats_on_side) SAPCA_HIP(hipEventSynchronize(h.ev_stats));   // (masked fits: the copy came from the third stream)
    finish_statistics(h);
  }
  h.mean = h.prep_mean;
  const double nm1 = (double)(h.m_fit - 1);
  h.expl_var.resize(h.k);
  for (uint64_t i = 0; i < h.k; ++i) {  // sparse/mod.rs:210-216
    const T sv = (T)h.sing[i];
    h.expl_var[i] = (double)(T)((T)(sv * sv) / (T)nm1);
  }
  if (h.opt.center) {
    h.total_var = h.prep_total_var;
  } else {  // sparse/mod.rs:218-223
    h.total_var = 0;
    for (uint64_t i = 0; i < h.k; ++i) h.total_var += h.expl_var[i];
  }
  SAPCA_HIP(hipStreamSynchronize(s));
  // column scaling: the total variance of (A - 1 mu^T) D is sum_j d_j^2 var_j, reduced on the device beside the factors
  if (h.scale_model && h.opt.center) h.total_var = *static_cast<const double*>(h.scale_host.p);
  covar_finish_fit(h);
  collect_timings(h, true);
  if (total_ev >= 0) h.timings.fit_total_ms = h.timer.ms(total_ev);
  describe_sweeps<T>(h);
}

// ------------------------------------------------------------------------------------------
// transform
// ------------------------------------------------------------------------------------------
namespace {

// The operator a projection sweeps and what the handle holds of it.
template <typename T>
struct Projection {
  CsrView<T> Au;                 // the matrix without the masked-out columns
  const TiledOp* top = nullptr;  // its tile-major format (null: row kernel)
  int ldk = 0;                   // leading dimension of the k-column panel swept through it
  double* d_cnt = nullptr;       // stored entries per column (Q2's weights); null where nothing reads them
  bool prepared = false;         // A is the matrix the handle's preparation was made from
};

// The only place in transform() that invalidates the preparation's key or rebuilds tiled_a.  Main stream; a masked matrix
// other than the prepared one synchronises with the host (its compaction).
template <typename T>
Projection<T> select_projection_operator(H& h, const CsrView<T>& A) {
  hipStream_t s = h.stream;
  const int k = (int)h.k;
  const bool masked = !h.mask.empty(), ref_sem = h.opt.transform_semantics == SAPCA_TRANSFORM_REFERENCE;
  Projection<T> pr;
  pr.ldk = (int)round_up(k, 16);
  pr.prepared = h.prep_key == prep_key_of(h, A);
  if (pr.prepared) {
    // the fitted matrix's tile-major format serves the projection sweep too (one row block per workgroup)
    // (operators with few row blocks -- a shard of a strong-scaled fit -- split their tile range over workgroups: the sweep sums
    //  the slabs itself; only the masked Q3 projection insists on an unsplit operator and checks that on its own)
    if (h.tiled_a.valid && k <= k::kMaxPanelWidth) pr.top = &h.tiled_a;
    pr.Au = Engine<T>::view(h.a_used);
    pr.d_cnt = h.stats.ptr<double>() + 2 * A.cols;
  } else if (masked) {
    h.prep_key.valid = false;  // the compaction buffers are about to be reused
    std::vector<int32_t> o2m32;   // (the compaction synchronises before it goes out of scope)
    pr.Au = Engine<T>::view(compact_a(h, A, upload_o2m(h, o2m32), (int64_t)h.n_used));
  } else {
    pr.Au = A;
    if (ref_sem) {
      h.prep_key.valid = false;
      pr.d_cnt = stats_dev(h, A.cols) + 2 * A.cols;
      k::column_counts_f64(A.idx, A.nnz, A.cols, pr.d_cnt, h.scratch, s);
      if (h.comm.active()) h.comm.allreduce(pr.d_cnt, (uint64_t)A.cols, 1, s);
    }
  }
  // A matrix the handle holds no preparation of (a separate transform of new rows, or of caller-owned arrays): above the
  // staged sweep's break-even its tile-major format is built for this one sweep -- 0.9 ms + a 0.55 ms sweep at C2's size
  // against 5 ms through the row kernel.  (The masked Q3 projection checks on its own whether it can use it.)
  if (!pr.prepared && k <= k::kMaxPanelWidth && pr.Au.nnz > 0) {
    const int ldp_t = staged_sweep_ldp<T>(pr.Au.rows, pr.Au.cols, (double)pr.Au.nnz, k, h.opt.spmm_variant);
    if (ldp_t != 0) {
      h.prep_key.valid = false;   // (tiled_a no longer belongs to the fitted matrix)
      h.tiled_at = TiledOp();
      h.tiled_a = TiledOp();
      if (k::build_tiled(pr.Au, ldp_t, h.tiled_a, h.tb_a, s, k::QuadSource::csr()) && h.tiled_a.valid) pr.top = &h.tiled_a;
      else h.tiled_a = TiledOp();
    }
  }
  if (pr.top) pr.ldk = panel_ld(k, pr.top->ldp);
  return pr;
}

// fit_transform, f32 randomized: the fit stopped in front of the host eigensolver.  The projection is linear in the
// components: with vt^T = B^T M (M = Uh S^-1 diag(sign), l x k) the reference's t = Ac diag(cnt) vt^T (Q2; cnt = 1 for the
// centred semantics) is [Ac diag(cnt) B^T] M -- the sweep runs on the un-rotated n x l panel while the host solves the
// l x l eigenproblem, and one m x l by l x k panel product rotates its result.  (B^T = panel_x; Q = panel_y is free.)
template <typename T>
void project_unrotated(H& h, const Projection<T>& pr, T* d_out) {
  hipStream_t s = h.stream;
  const int ld = h.held_small.ld, k = (int)h.k;
  const int64_t m = pr.Au.rows, n_used = (int64_t)h.n_used;
  const bool center = h.opt.center != 0, ref_sem = h.opt.transform_semantics == SAPCA_TRANSFORM_REFERENCE;
  const SmallLayout lay(h.small, ld);
  T* cvec = lay.c<T>();
  T* Xs = h.panel_xs.as<T>((size_t)n_used * ld);
  T* Tp = h.panel_y.as<T>((size_t)m * ld);
  k::scale_rows(h.panel_x.ptr<T>(), n_used, ld, ref_sem ? pr.d_cnt : nullptr, Xs, s);
  if (center) k::weighted_colsum(Xs, n_used, ld, h.mean_used_dev.ptr<T>(), cvec, h.scratch2, s);
  k::spmm(pr.Au, h.tiled_a.valid ? &h.tiled_a : nullptr, Xs, ld, Tp, ld, ld, center ? cvec : nullptr, h.opt.spmm_variant, h.split_scratch, s);
  const double* sign = nullptr;
  Engine<T>::finish_small_svd(h, &sign);   // (waits for the Gram's copy only; the sweep above is running)
  const int ldm = (int)round_up(k, 16);
  k::scale_columns(lay.m(), ld, ldm, k, sign, s);
  k::panel_gemm(Tp, m, ld, lay.m(), ldm, d_out, s, false, k, k);
}

// The projection with the fitted components (a separate transform, masked fits, f64, Lanczos, large m), in one of three semantics:
//  Q2 (sparse/mod.rs:268-282), unmasked:            t_ik = sum_j cnt_j (x_ij - [center] mu_j) V_kj
//  Q3 (sparse_masked/mod.rs:488-529), masked:       the mean is subtracted at stored, kept entries only
//  centred (opt-in, SAPCA_TRANSFORM_CENTERED):      the mathematically centred projection (A - 1 mu^T) V^T
//  uncentred (a model fitted with covariates):      A V^T through the centred semantics' one sweep; project_residual_scores finishes it
template <typename T>
void project_with_components(H& h, const Projection<T>& pr, T* d_out, bool uncentred = false) {
  hipStream_t s = h.stream;
  const int k = (int)h.k, ldk = pr.ldk, variant = h.opt.spmm_variant;
  const int64_t m = pr.Au.rows, n_used = (int64_t)h.n_used;
  const bool center = h.opt.center != 0 && !uncentred, masked = !h.mask.empty(), ref_sem = h.opt.transform_semantics == SAPCA_TRANSFORM_REFERENCE;
  const T* mu = h.mean_used_dev.ptr<T>();
  T* cvec = SmallLayout(h.small, ldk).c<T>();
  T* W = h.panel_w.as<T>((size_t)n_used * ldk);
  k::scaled_transpose(h.components_dev.ptr<T>(), n_used, k, ref_sem && !masked ? pr.d_cnt : nullptr, W, ldk, s);
  if (h.scale_model) k::scale_panel_rows(W, n_used, ldk, h.scale_dt.ptr<T>(), s);   // W = D V^T, with the d (and mu) of the fit
  if (!(ref_sem && masked)) {   // Q2, centred: one sweep, centred through c = W^T mu
    if (center) k::weighted_colsum(W, n_used, ldk, mu, cvec, h.scratch2, s);
    k::spmm(pr.Au, pr.top, W, ldk, d_out, k, k, center ? cvec : nullptr, variant, h.split_scratch, s);
    return;
  }
  // Q3.  TwoSweeps: A'W - P diag(mu) W through the fitted matrix's tile-major format (spmm_dq.hip) -- only for the fitted
  // matrix: `q3_cancels` was decided from ITS column statistics.  ShiftedRows: the row kernel subtracts mu_j entry by entry,
  // like the reference; it also takes over where the two sweeps refuse the operator.  Plain: nothing to subtract.
  enum class Q3 { TwoSweeps, ShiftedRows, Plain };
  const bool dq = sizeof(T) == 4 && pr.top && pr.prepared && variant != 1 && !h.q3_cancels && dbg_env("SAPCA_Q3_ROWKERNEL") == nullptr;
  Q3 route = !center ? Q3::Plain : dq ? Q3::TwoSweeps : Q3::ShiftedRows;
  if constexpr (sizeof(T) == 4) {
    if (route == Q3::TwoSweeps) {
      float* W2 = h.scratch2.as<float>((size_t)n_used * ldk);
      float* tmp = h.panel_y.as<float>((size_t)m * std::max(k, 1));
      if (!k::q3_projection_dq(pr.Au, *pr.top, W, ldk, mu, W2, tmp, d_out, k, s)) route = Q3::ShiftedRows;
    }
  }
  if (route == Q3::ShiftedRows) k::spmm_rows_shifted(pr.Au, W, ldk, d_out, k, k, mu, s);
  if (route == Q3::Plain) k::spmm(pr.Au, pr.top, W, ldk, d_out, k, k, (const T*)nullptr, variant, h.split_scratch, s);
}

// A model fitted with covariates: scores = A V^T - Q_rows C, with Q_rows = D_rows W from the covariates set now (the fitted
// matrix's, or a new matrix's own rows) and C = Q^T A V^T from the fit (covar_c, on the device).  The host array the copy reads is a member.
template <typename T>
void project_residual_scores(H& h, const Projection<T>& pr, T* d_out) {
  hipStream_t s = h.stream;
  constexpr int kq = k::kCovarCols;
  const int k = (int)h.k;
  const int64_t m = pr.Au.rows;
  project_with_components(h, pr, d_out, true);
  covar_rows_basis<T>(h);
  T* Q = h.covar_q.as<T>((size_t)m * kq);
  SAPCA_HIP(hipMemcpyAsync(Q, h.covar.q_t.data(), (size_t)m * kq * sizeof(T), hipMemcpyHostToDevice, s));
  k::panel_sub_qs(d_out, Q, m, k, k, h.covar_c.ptr<double>(), h.covar.ldc, s);
}

}  // namespace

template <typename T>
void Engine<T>::transform(H& h, const CsrView<T>& A, T* d_out) {
  hipStream_t s = h.stream;
  const bool masked = !h.mask.empty();
  if (masked && (int64_t)h.mask.size() != A.cols)  // sparse_masked/mod.rs:440-444
    throw Error(SAPCA_ERR_MASK_LEN, "The mask vector length and the number of features (columns) have to be the same!");
  if (!h.fitted) throw Error(SAPCA_ERR_NOT_FITTED, "Must be fitted before transform!");  // sparse/mod.rs:259,263
  SAPCA_CHECK(h.dtype == kDtype, SAPCA_ERR_ARG, "transform dtype differs from the fitted model's");
  SAPCA_CHECK((uint64_t)A.cols == h.n_cols, SAPCA_ERR_ARG, "transform: column count differs from the fitted matrix");
  SAPCA_CHECK(masked == h.has_mask_maps, SAPCA_ERR_ARG, "transform: mask changed since fit");
  covar_check(h, (uint64_t)A.rows, false, false);
  scale_check(h, (uint64_t)A.rows, (uint64_t)A.cols, false, false);
  // keep the fit's spans (their events stay valid); drop those of an earlier transform
  h.spans.erase(std::remove_if(h.spans.begin(), h.spans.end(), [](const std::pair<int, int>& p) { return p.first == C_TRANSFORM; }),
                h.spans.end());
  if (h.spans.empty()) h.timer.begin_collect(s, h.opt.collect_timings != 0);
  if (A.rows == 0) {   // (a rank with an empty shard still completes a fit whose tail was held back)
    finish_fit(h);
    return;
  }
  {
    Scope sc(h, C_TRANSFORM);
    const Projection<T> pr = select_projection_operator(h, A);
    if (h.held_small.pending && pr.prepared && !masked) {
      project_unrotated(h, pr, d_out);
    } else {
      if (h.held_small.pending) finish_small_svd(h, nullptr);   // (a held-back small SVD whose projection cannot take the un-rotated route)
      if (h.covar.model.rank > 0) project_residual_scores(h, pr, d_out);
      else project_with_components(h, pr, d_out);
    }
  }
  SAPCA_HIP(hipStreamSynchronize(s));
  finish_fit(h);   // (fit_transform: the fit's host-side tail, held back until the projection was queued)
  collect_timings(h, false);
}

template struct Engine<float>;
template struct Engine<double>;

}  // namespace sapca
