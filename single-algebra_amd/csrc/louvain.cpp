// Host staging of sapca_louvain_* (the kernels are louvain.hip's, the ordered sums tsne.hip's, the scan prep.hip's): argument
// checks, buffer layouts, launches.  Everything that can be refused is refused before anything is enqueued or a buffer is
// touched.  All work space lives in h.louvain: a fitted model, a cached preparation, the upload's statistics, the selection, the
// canonical, the t-SNE, the k-means and the UMAP buffers are not touched.
#include "resident.h"

namespace sapca {
namespace resident {

namespace {

namespace KK = sapca::k;

template <typename T>
void check_graph(const CsrView<T>& G, const std::string& w) {
  check_rows((uint64_t)G.rows, w);
  SAPCA_CHECK(G.rows == G.cols, SAPCA_ERR_ARG, w + ": the graph must be square");
  SAPCA_CHECK(G.rows == 0 || G.ptr != nullptr, SAPCA_ERR_ARG, w + ": NULL row offsets with m = " + num((uint64_t)G.rows));
  SAPCA_CHECK(G.nnz == 0 || (G.idx != nullptr && G.val != nullptr), SAPCA_ERR_ARG,
              w + ": a NULL column or value array with nnz = " + num((uint64_t)G.nnz));
}

void check_options(const sapca_louvain_options* o, const std::string& w) {
  check_options_header(o, "sapca_louvain_options", w);
  check_constant(o->resolution, "resolution", w);
  check_constant(o->tol, "tol", w);
  SAPCA_CHECK(o->max_sweeps >= 1 && o->max_sweeps <= 4096, SAPCA_ERR_ARG, w + ": max_sweeps = " + num(o->max_sweeps) + " is outside 1 .. 4096");
  SAPCA_CHECK(o->max_levels <= 64, SAPCA_ERR_ARG, w + ": max_levels = " + num(o->max_levels) + " exceeds 64");
}

// the rows of a CSR per length class (one read-back: the class counts size the launches and the long rows' key space)
KK::LouvainLists make_lists(H& h, const int64_t* ptr, int64_t n, DevBuf& rows, DevBuf& long_off, DevBuf& keys) {
  hipStream_t s = h.stream;
  KK::LouvainLists L;
  L.n = n;
  uint32_t* r = rows.as<uint32_t>((size_t)std::max<int64_t>(3 * n, 1));
  unsigned long long* off = long_off.as<unsigned long long>((size_t)std::max<int64_t>(n, 1));
  unsigned long long* ctr = h.louvain.ctr.as<unsigned long long>(KK::kLvCtrWords);
  KK::louvain_list_rows(ptr, n, r, off, ctr, s);
  unsigned long long host[KK::kLvCtrWords] = {};
  SAPCA_HIP(hipMemcpyAsync(host, ctr, sizeof(host), hipMemcpyDeviceToHost, s));
  SAPCA_HIP(hipStreamSynchronize(s));
  L.rows = r;
  L.long_off = off;
  for (int c = 0; c < 3; ++c) L.counts[c] = (int64_t)host[c];
  L.keys = host[KK::kLvLongKeys] ? keys.as<unsigned long long>((size_t)host[KK::kLvLongKeys]) : nullptr;
  return L;
}

// the control block with (gamma, tol) and the two generations of a graph of n vertices; lab0 / lab1 null: the handle's
KK::LouvainState make_state(H& h, int64_t n, double gamma, double tol, int32_t* lab0, int32_t* lab1) {
  H::Louvain& w = h.louvain;
  const size_t rows = (size_t)std::max<int64_t>(n, 1);
  KK::LouvainState st;
  st.ctl = w.ctl.as<KK::LouvainCtl>(1);
  st.lab[0] = lab0 ? lab0 : w.lab0.as<int32_t>(rows);
  st.lab[1] = lab1 ? lab1 : w.lab1.as<int32_t>(rows);
  st.tot[0] = w.tot0.as<double>(rows);
  st.tot[1] = w.tot1.as<double>(rows);
  KK::LouvainCtl c = {};
  c.gamma = gamma;
  c.tol = tol;
  SAPCA_HIP(hipMemcpyAsync(st.ctl, &c, sizeof(c), hipMemcpyHostToDevice, h.stream));
  SAPCA_HIP(hipStreamSynchronize(h.stream));   // (c leaves scope)
  return st;
}

// k and ctl->S of the graph
template <typename TV>
double* enqueue_degrees(H& h, const CsrView<TV>& A, const KK::LouvainState& st) {
  H::Louvain& w = h.louvain;
  double* k = w.k.as<double>((size_t)A.rows);
  double* sum_part = w.sum_part.as<double>(KK::tsne_sum_parts(A.rows) + 1);
  KK::louvain_row_sums<TV>(A, st, 0, false, k, h.stream);
  KK::tsne_sum(k, A.rows, sum_part, &st.ctl->S, h.stream);
  return k;
}

// tot, ctl->sum_s and ctl->sum_sq of the generation (st, flip): what Q needs
template <typename TV>
void enqueue_quality(H& h, const CsrView<TV>& A, const KK::LouvainState& st, int flip, bool need_moved, const double* k) {
  H::Louvain& w = h.louvain;
  hipStream_t s = h.stream;
  const int64_t n = A.rows;
  unsigned long long* skeys = w.skeys.as<unsigned long long>((size_t)KK::louvain_sort_len(n));
  double* srow = w.srow.as<double>((size_t)n);
  double* sq = w.sq.as<double>((size_t)n);
  double* sum_part = w.sum_part.as<double>(KK::tsne_sum_parts(n) + 1);
  KK::louvain_totals(st, flip, need_moved, n, k, skeys, &st.ctl->S, sq, s);
  KK::louvain_row_sums<TV>(A, st, flip, true, srow, s);
  KK::tsne_sum(srow, n, sum_part, &st.ctl->sum_s, s);
  KK::tsne_sum(sq, n, sum_part, &st.ctl->sum_sq, s);
}

KK::LouvainCtl read_ctl(H& h, const KK::LouvainState& st) {
  KK::LouvainCtl c = {};
  SAPCA_HIP(hipMemcpyAsync(&c, st.ctl, sizeof(c), hipMemcpyDeviceToHost, h.stream));
  SAPCA_HIP(hipStreamSynchronize(h.stream));
  return c;
}

// one level on A from singletons; the kept labels are st.lab[result.cur]
template <typename TV>
KK::LouvainCtl run_level(H& h, const CsrView<TV>& A, const KK::LouvainLists& L, uint64_t level, const sapca_louvain_options* o,
                         KK::LouvainState& st) {
  H::Louvain& w = h.louvain;
  hipStream_t s = h.stream;
  const int64_t n = A.rows;
  st = make_state(h, n, o->resolution, o->tol, nullptr, nullptr);
  uint8_t* anchored = w.anchored.as<uint8_t>((size_t)n);
  KK::louvain_iota(st.lab[0], n, s);
  const double* k = enqueue_degrees<TV>(h, A, st);
  enqueue_quality<TV>(h, A, st, 0, false, k);
  KK::louvain_decide(st, true, s);
  KK::LouvainCtl c = read_ctl(h, st);
  if (!(c.S > 0.0)) return c;   // (no weight at all: nothing to move)
  for (uint64_t t = 0; t < o->max_sweeps; ++t) {   // kernels only
    KK::louvain_anchor(st, n, o->random_seed, level, t, anchored, s);
    KK::louvain_sweep<TV>(A, L, st, k, anchored, o->random_seed, level, t, s);
    enqueue_quality<TV>(h, A, st, 1, true, k);
    KK::louvain_decide(st, false, s);
    if ((t & 7) == 7 && t + 1 < o->max_sweeps) {   // stop enqueueing behind a finished level (what is enqueued already does nothing)
      unsigned long long flag = 0;
      SAPCA_HIP(hipMemcpyAsync(&flag, &st.ctl->done, sizeof(flag), hipMemcpyDeviceToHost, s));
      SAPCA_HIP(hipStreamSynchronize(s));
      if (flag) break;
    }
  }
  return read_ctl(h, st);
}

// the coarse graph of `labels` on A into the handle's set `set`; renum (n int32, of this call) stays in w.renum
template <typename TV>
CsrView<double> aggregate(H& h, const CsrView<TV>& A, const KK::LouvainLists& L, const int32_t* labels, int set, int32_t* d_renumbered) {
  H::Louvain& w = h.louvain;
  hipStream_t s = h.stream;
  const int64_t n = A.rows;
  KK::LouvainState byl;   // (no control block: labels as given, nothing skipped)
  byl.lab[0] = const_cast<int32_t*>(labels);
  unsigned long long* skeys = w.skeys.as<unsigned long long>((size_t)KK::louvain_sort_len(n));
  KK::louvain_totals(byl, 0, false, n, nullptr, skeys, nullptr, nullptr, s);
  int64_t* scan = w.flag.as<int64_t>((size_t)n + 1);
  KK::louvain_flag(labels, n, scan, s);
  KK::exclusive_scan_i64(scan, n + 1, w.scan, 0, s);
  int32_t* renum = w.renum.as<int32_t>((size_t)n);
  KK::louvain_renumber(labels, n, scan, renum, d_renumbered, s);
  int64_t* cnt = w.cnt.as<int64_t>((size_t)n);
  KK::louvain_group_count<TV>(A, L, labels, cnt, s);
  int32_t* pos = w.pos.as<int32_t>((size_t)n);
  int64_t* rawoff = w.rawcnt.as<int64_t>((size_t)n + 1);
  KK::louvain_positions(skeys, n, cnt, pos, rawoff, s);
  KK::exclusive_scan_i64(rawoff, n + 1, w.scan, 0, s);
  int64_t n1 = 0, nnz_raw = 0;
  SAPCA_HIP(hipMemcpyAsync(&n1, scan + n, sizeof(int64_t), hipMemcpyDeviceToHost, s));
  SAPCA_HIP(hipMemcpyAsync(&nnz_raw, rawoff + n, sizeof(int64_t), hipMemcpyDeviceToHost, s));
  SAPCA_HIP(hipStreamSynchronize(s));
  CsrView<double> out;
  out.rows = out.cols = n1;
  if (n1 == 0) {   // (every label out of range)
    int64_t* p0 = w.agg_ptr[set].as<int64_t>(1);
    SAPCA_HIP(hipMemsetAsync(p0, 0, sizeof(int64_t), s));
    out.ptr = p0;
    out.idx = w.agg_idx[set].as<int32_t>(1);
    out.val = w.agg_val[set].as<double>(1);
    return out;
  }
  // the rows of the members side by side, in ascending vertex order: the coarse rows before their merge
  int64_t* rawptr = w.raw_ptr.as<int64_t>((size_t)n1 + 1);
  int32_t* raw_idx = w.raw_idx.as<int32_t>((size_t)std::max<int64_t>(nnz_raw, 1));
  double* raw_val = w.raw_val.as<double>((size_t)std::max<int64_t>(nnz_raw, 1));
  KK::louvain_coarse_offsets(skeys, n, rawoff, renum, scan, rawptr, s);
  KK::louvain_group_emit<TV>(A, L, labels, renum, rawoff, pos, raw_idx, raw_val, s);
  CsrView<double> R;
  R.rows = R.cols = n1; R.nnz = nnz_raw; R.ptr = rawptr; R.idx = raw_idx; R.val = raw_val;
  const KK::LouvainLists L2 = make_lists(h, rawptr, n1, w.lists2, w.long_off2, w.keys2);
  int64_t* cnt2 = w.cnt2.as<int64_t>((size_t)n1 + 1);
  int64_t* optr = w.agg_ptr[set].as<int64_t>((size_t)n1 + 1);
  SAPCA_HIP(hipMemsetAsync(cnt2, 0, ((size_t)n1 + 1) * sizeof(int64_t), s));
  KK::louvain_group_count<double>(R, L2, nullptr, cnt2, s);
  KK::exclusive_scan_i64(cnt2, n1 + 1, w.scan, 0, s, optr);
  int64_t nnz1 = 0;
  SAPCA_HIP(hipMemcpyAsync(&nnz1, optr + n1, sizeof(int64_t), hipMemcpyDeviceToHost, s));
  SAPCA_HIP(hipStreamSynchronize(s));
  int32_t* oidx = w.agg_idx[set].as<int32_t>((size_t)std::max<int64_t>(nnz1, 1));
  double* oval = w.agg_val[set].as<double>((size_t)std::max<int64_t>(nnz1, 1));
  KK::louvain_group_emit<double>(R, L2, nullptr, nullptr, optr, nullptr, oidx, oval, s);
  out.nnz = nnz1;
  out.ptr = optr;
  out.idx = oidx;
  out.val = oval;
  return out;
}

}  // namespace

template <typename T>
void louvain_modularity(H& h, const CsrView<T>& G, const int32_t* d_labels, double resolution, double* modularity) {
  const std::string who("louvain_modularity");
  check_constant(resolution, "resolution", who);
  check_graph(G, who);
  SAPCA_CHECK(modularity != nullptr, SAPCA_ERR_ARG, who + ": null output pointer");
  if (G.rows == 0) {
    *modularity = 0.0;
    return;
  }
  SAPCA_CHECK(d_labels != nullptr, SAPCA_ERR_ARG, who + ": d_labels is NULL with m = " + num((uint64_t)G.rows));
  KK::LouvainState st = make_state(h, G.rows, resolution, 0.0, const_cast<int32_t*>(d_labels), nullptr);
  const double* k = enqueue_degrees<T>(h, G, st);
  enqueue_quality<T>(h, G, st, 0, false, k);
  KK::louvain_decide(st, true, h.stream);
  *modularity = read_ctl(h, st).Q;
}

template <typename T>
void louvain_sweep(H& h, const CsrView<T>& G, const int32_t* d_labels_in, uint32_t seed, uint32_t level, uint32_t sweep, double resolution,
                   int32_t* d_labels_out, uint64_t* n_moved) {
  const std::string who("louvain_sweep");
  check_constant(resolution, "resolution", who);
  SAPCA_CHECK(level < (1u << 20), SAPCA_ERR_ARG, who + ": level = " + num(level) + "; 2^20 or more are not supported");
  SAPCA_CHECK(sweep < 4096, SAPCA_ERR_ARG, who + ": sweep = " + num(sweep) + " is outside 0 .. 4095");
  check_graph(G, who);
  if (n_moved) *n_moved = 0;
  if (G.rows == 0) return;
  SAPCA_CHECK(d_labels_in != nullptr && d_labels_out != nullptr, SAPCA_ERR_ARG, who + ": a NULL label array with m = " + num((uint64_t)G.rows));
  SAPCA_CHECK(d_labels_in != d_labels_out, SAPCA_ERR_ARG, who + ": d_labels_in and d_labels_out are the same array");
  H::Louvain& w = h.louvain;
  hipStream_t s = h.stream;
  const int64_t n = G.rows;
  const KK::LouvainLists L = make_lists(h, G.ptr, n, w.lists, w.long_off, w.keys);
  KK::LouvainState st = make_state(h, n, resolution, 0.0, const_cast<int32_t*>(d_labels_in), d_labels_out);
  uint8_t* anchored = w.anchored.as<uint8_t>((size_t)n);
  unsigned long long* skeys = w.skeys.as<unsigned long long>((size_t)KK::louvain_sort_len(n));
  const double* k = enqueue_degrees<T>(h, G, st);
  KK::louvain_totals(st, 0, false, n, k, skeys, nullptr, nullptr, s);
  KK::louvain_anchor(st, n, seed, level, sweep, anchored, s);
  KK::louvain_sweep<T>(G, L, st, k, anchored, seed, level, sweep, s);
  const KK::LouvainCtl c = read_ctl(h, st);
  if (n_moved) *n_moved = c.moved;
}

template <typename T>
void louvain_aggregate(H& h, const CsrView<T>& G, const int32_t* d_labels, uint64_t* n_out, uint64_t* nnz_out, const int64_t** d_ptr,
                       const int32_t** d_idx, double** d_val, int32_t* d_renumbered) {
  const std::string who("louvain_aggregate");
  SAPCA_CHECK(n_out && nnz_out && d_ptr && d_idx && d_val, SAPCA_ERR_ARG, who + ": null output pointer");
  check_graph(G, who);
  H::Louvain& w = h.louvain;
  h.drop_preparation_of(w);
  if (G.rows == 0) {
    int64_t* p0 = w.agg_ptr[0].as<int64_t>(1);
    SAPCA_HIP(hipMemsetAsync(p0, 0, sizeof(int64_t), h.stream));
    SAPCA_HIP(hipStreamSynchronize(h.stream));
    *n_out = 0;
    *nnz_out = 0;
    *d_ptr = p0;
    *d_idx = w.agg_idx[0].as<int32_t>(1);
    *d_val = w.agg_val[0].as<double>(1);
    return;
  }
  SAPCA_CHECK(d_labels != nullptr, SAPCA_ERR_ARG, who + ": d_labels is NULL with m = " + num((uint64_t)G.rows));
  const KK::LouvainLists L = make_lists(h, G.ptr, G.rows, w.lists, w.long_off, w.keys);
  const CsrView<double> C = aggregate<T>(h, G, L, d_labels, 0, d_renumbered);
  SAPCA_HIP(hipStreamSynchronize(h.stream));   // complete when the call returns
  *n_out = (uint64_t)C.rows;
  *nnz_out = (uint64_t)C.nnz;
  *d_ptr = C.ptr;
  *d_idx = C.idx;
  *d_val = const_cast<double*>(C.val);
}

template <typename T>
void louvain_device(H& h, const CsrView<T>& G, const sapca_louvain_options* opts, int32_t* d_labels, uint64_t* n_communities,
                    double* modularity, uint32_t* n_levels) {
  const std::string who("louvain");
  check_options(opts, who);
  check_graph(G, who);
  if (n_communities) *n_communities = 0;
  if (modularity) *modularity = 0.0;
  if (n_levels) *n_levels = 0;
  if (G.rows == 0) return;
  SAPCA_CHECK(d_labels != nullptr, SAPCA_ERR_ARG, who + ": d_labels is NULL with m = " + num((uint64_t)G.rows));
  H::Louvain& w = h.louvain;
  hipStream_t s = h.stream;
  h.drop_preparation_of(w);
  const int64_t m = G.rows;
  const uint32_t max_levels = opts->max_levels ? opts->max_levels : 32;
  KK::LouvainState st;
  KK::LouvainLists L = make_lists(h, G.ptr, m, w.lists, w.long_off, w.keys);
  KK::LouvainCtl c = run_level<T>(h, G, L, 0, opts, st);
  double Q = c.S > 0.0 ? c.Q : 0.0;
  uint64_t ncomm = (uint64_t)m;
  uint32_t levels = 0;
  if (!(c.S > 0.0) || c.kept == 0) {
    KK::louvain_iota(d_labels, m, s);
  } else {
    int set = 0;
    CsrView<double> A = aggregate<T>(h, G, L, st.lab[c.cur & 1], set, nullptr);
    KK::louvain_compose(d_labels, m, st.lab[c.cur & 1], w.renum.ptr<int32_t>(), true, s);
    for (;;) {
      ++levels;
      Q = c.Q;
      ncomm = (uint64_t)A.rows;
      if (A.rows <= 1 || levels >= max_levels) break;
      L = make_lists(h, A.ptr, A.rows, w.lists, w.long_off, w.keys);
      c = run_level<double>(h, A, L, levels, opts, st);
      if (!(c.S > 0.0) || c.kept == 0) break;
      set ^= 1;
      const CsrView<double> B = aggregate<double>(h, A, L, st.lab[c.cur & 1], set, nullptr);
      KK::louvain_compose(d_labels, m, st.lab[c.cur & 1], w.renum.ptr<int32_t>(), false, s);
      A = B;
    }
  }
  SAPCA_HIP(hipStreamSynchronize(s));   // complete when the call returns
  if (n_communities) *n_communities = ncomm;
  if (modularity) *modularity = Q;
  if (n_levels) *n_levels = levels;
}

template <typename T>
void louvain_host(H& h, uint64_t m, uint64_t nnz, const int64_t* ptr, const int32_t* idx, const T* val, const sapca_louvain_options* opts,
                  int32_t* labels, uint64_t* n_communities, double* modularity, uint32_t* n_levels) {
  const std::string who("louvain");
  check_options(opts, who);
  CsrView<T> G = unchecked_view<T>(m, m, nnz, ptr, idx, val);
  check_graph(G, who);
  if (n_communities) *n_communities = 0;
  if (modularity) *modularity = 0.0;
  if (n_levels) *n_levels = 0;
  if (m == 0) return;
  SAPCA_CHECK(labels != nullptr, SAPCA_ERR_ARG, who + ": labels is NULL with m = " + num(m));
  H::Louvain& w = h.louvain;
  hipStream_t s = h.stream;
  int64_t* dp = w.in_ptr.as<int64_t>(m + 1);
  int32_t* di = w.in_idx.as<int32_t>(std::max<size_t>(nnz, 1));
  T* dv = w.in_val.as<T>(std::max<size_t>(nnz, 1));
  int32_t* dl = w.labels.as<int32_t>(m);
  SAPCA_HIP(hipMemcpyAsync(dp, ptr, (m + 1) * sizeof(int64_t), hipMemcpyHostToDevice, s));
  if (nnz) {
    SAPCA_HIP(hipMemcpyAsync(di, idx, nnz * sizeof(int32_t), hipMemcpyHostToDevice, s));
    SAPCA_HIP(hipMemcpyAsync(dv, val, nnz * sizeof(T), hipMemcpyHostToDevice, s));
  }
  louvain_device<T>(h, unchecked_view<T>(m, m, nnz, dp, di, dv), opts, dl, n_communities, modularity, n_levels);
  SAPCA_HIP(hipMemcpyAsync(labels, dl, m * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  SAPCA_HIP(hipStreamSynchronize(s));
}

#define SAPCA_INSTANTIATE_LOUVAIN(T)                                                                                                \
  template void louvain_modularity<T>(H&, const CsrView<T>&, const int32_t*, double, double*);                                      \
  template void louvain_sweep<T>(H&, const CsrView<T>&, const int32_t*, uint32_t, uint32_t, uint32_t, double, int32_t*, uint64_t*); \
  template void louvain_aggregate<T>(H&, const CsrView<T>&, const int32_t*, uint64_t*, uint64_t*, const int64_t**, const int32_t**, \
                                     double**, int32_t*);                                                                           \
  template void louvain_device<T>(H&, const CsrView<T>&, const sapca_louvain_options*, int32_t*, uint64_t*, double*, uint32_t*);    \
  template void louvain_host<T>(H&, uint64_t, uint64_t, const int64_t*, const int32_t*, const T*, const sapca_louvain_options*,     \
                                int32_t*, uint64_t*, double*, uint32_t*);
SAPCA_INSTANTIATE_LOUVAIN(float)
SAPCA_INSTANTIATE_LOUVAIN(double)
#undef SAPCA_INSTANTIATE_LOUVAIN

}  // namespace resident
}  // namespace sapca
