// sapca_hvg_moments_csr_device_* / sapca_loess_f64 / sapca_hvg_csr_device_*: variable genes on the resident CSR (include/sapca.h,
// "Variable genes").  Host side: the refusals, the batch sizes, the transposition, the passes and the n-sized device steps of
// hvg.hip, and the finishing arithmetic on n values per batch: ranks, medians, bins and the final sorts, in f64.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <functional>
#include <limits>
#include <numeric>

#include "resident.h"

namespace sapca {
namespace resident {

namespace {

constexpr double kNaN = std::numeric_limits<double>::quiet_NaN();

void check_span(const std::string& w, double span) {
  SAPCA_CHECK(span > 0.0 && span <= 1.0, SAPCA_ERR_ARG, w + ": span = " + numd(span) + " is outside (0, 1]");
}

// q = min(n, max(3, floor(span n + 1e-5)))
int64_t loess_window(double span, int64_t n) {
  const int64_t q = std::max<int64_t>(3, (int64_t)std::floor(span * (double)n + 1e-5));
  return std::min<int64_t>(n, q);
}

// The work arrays of a call in h.hvg.vec: `nd` f64 arrays of n, then two u32 arrays of n and a counter.
struct HvgWork {
  double* d;
  uint32_t *iota, *perm, *counter;
  size_t n;
  HvgWork(H& h, size_t n_, size_t nd) : n(std::max<size_t>(n_, 1)) {
    d = h.hvg.vec.as<double>(nd * n + n + 2);
    iota = reinterpret_cast<uint32_t*>(d + nd * n);
    perm = iota + n;
    counter = perm + n;
  }
  double* f64(size_t i) const { return d + i * n; }
};

// The rows of every batch (K values), from integer counts made on the device; no labels: the one batch of m rows.
std::vector<uint64_t> batch_rows(H& h, const int32_t* d_batch, uint64_t m, uint32_t K) {
  std::vector<uint64_t> rows(K, 0);
  if (d_batch == nullptr) {
    rows[0] = m;
    return rows;
  }
  unsigned long long* d_group = h.hvg.group.as<unsigned long long>(K);
  k::rank_group_sizes(d_batch, (int64_t)m, (int)K, d_group, h.stream);
  static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "batch sizes are fetched as they are");
  fetch(rows, reinterpret_cast<const uint64_t*>(d_group), h.stream);
  SAPCA_HIP(hipStreamSynchronize(h.stream));
  return rows;
}

// the median of the values (sorted here); NaN when there is none
double median_of(std::vector<double>& v) {
  if (v.empty()) return kNaN;
  std::sort(v.begin(), v.end());
  const size_t k = v.size();
  return k % 2 ? v[k / 2] : 0.5 * (v[k / 2 - 1] + v[k / 2]);
}

// order[r] = the column at position r of a stable descending sort of v, NaN last, ties by column index
std::vector<uint32_t> order_desc(const double* v, size_t n) {
  std::vector<uint32_t> order(n);
  std::iota(order.begin(), order.end(), 0u);
  std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
    const bool na = std::isnan(v[a]), nb = std::isnan(v[b]);
    if (na || nb) return !na && nb;
    return v[a] > v[b];
  });
  return order;
}

double nan_to_num(double v) {
  if (std::isnan(v)) return 0.0;
  if (std::isinf(v)) return v > 0 ? DBL_MAX : -DBL_MAX;
  return v;
}

// What the seurat flavour makes of one batch's EXPM1 moments: mean (log1p'd), var (of expm1 x), disp (ln), disp_norm, selected.
struct SeuratBatch {
  std::vector<double> mean, var, disp, norm;
  std::vector<uint8_t> hv;
};

bool within_cutoffs(const sapca_hvg_options& o, double mean, double norm) {
  const double d = std::isnan(norm) ? 0.0 : norm;
  return mean > o.min_mean && mean < o.max_mean && d > o.min_disp && d < o.max_disp;
}

void seurat_finish(const sapca_hvg_options& o, const std::vector<double>& s, const std::vector<double>& ss, double N, SeuratBatch& b) {
  const size_t n = s.size();
  b.mean.resize(n); b.var.resize(n); b.disp.resize(n); b.norm.resize(n); b.hv.assign(n, 0);
  for (size_t j = 0; j < n; ++j) {
    double mu = s[j] / N;
    const double msq = ss[j] / N;
    const double mu2 = mu * mu;
    const double v = (msq - mu2) * (N / (N - 1.0));
    b.var[j] = v;
    if (mu == 0.0) mu = 1e-12;
    double d = v / mu;
    if (d == 0.0) d = kNaN;
    b.disp[j] = std::log(d);
    b.mean[j] = std::log1p(mu);
  }
  // pandas.cut(mean, bins = n_bins)
  const uint32_t nb = o.n_bins;
  double mn = b.mean[0], mx = b.mean[0];
  for (size_t j = 1; j < n; ++j) {
    mn = std::min(mn, b.mean[j]);
    mx = std::max(mx, b.mean[j]);
  }
  std::vector<double> edge(nb + 1);
  const bool flat = mn == mx;
  if (flat) {
    mn -= mn != 0.0 ? 0.001 * std::fabs(mn) : 0.001;
    mx += mx != 0.0 ? 0.001 * std::fabs(mx) : 0.001;
  }
  const double step = (mx - mn) / (double)nb;
  for (uint32_t i = 0; i <= nb; ++i) {
    const double off = (double)i * step;
    edge[i] = off + mn;
  }
  edge[nb] = mx;
  if (!flat) edge[0] -= (mx - mn) * 0.001;
  std::vector<int32_t> bin(n);
  std::vector<double> bsum(nb, 0.0), bmean(nb, 0.0), bdev(nb, 0.0), bstd(nb, 0.0);
  std::vector<uint64_t> bcnt(nb, 0);
  for (size_t j = 0; j < n; ++j) {   // right-closed: edge[i] < mean <= edge[i + 1]
    const int32_t i = (int32_t)(std::lower_bound(edge.begin(), edge.end(), b.mean[j]) - edge.begin()) - 1;
    bin[j] = i;
    if (i < 0 || i >= (int32_t)nb || std::isnan(b.disp[j])) continue;
    bsum[i] += b.disp[j];
    ++bcnt[i];
  }
  for (uint32_t i = 0; i < nb; ++i) bmean[i] = bcnt[i] ? bsum[i] / (double)bcnt[i] : kNaN;
  for (size_t j = 0; j < n; ++j) {
    const int32_t i = bin[j];
    if (i < 0 || i >= (int32_t)nb || std::isnan(b.disp[j])) continue;
    const double d = b.disp[j] - bmean[i];
    bdev[i] += d * d;
  }
  for (uint32_t i = 0; i < nb; ++i) {
    if (bcnt[i] >= 2) {
      bstd[i] = std::sqrt(bdev[i] / (double)(bcnt[i] - 1));
    } else {   // a one-gene bin
      bstd[i] = bmean[i];
      bmean[i] = 0.0;
    }
  }
  for (size_t j = 0; j < n; ++j) {
    const int32_t i = bin[j];
    b.norm[j] = (i < 0 || i >= (int32_t)nb) ? kNaN : (b.disp[j] - bmean[i]) / bstd[i];
  }
  if (o.n_top) {
    std::vector<double> valid;
    for (size_t j = 0; j < n; ++j)
      if (!std::isnan(b.norm[j])) valid.push_back(b.norm[j]);
    if (!valid.empty()) {
      std::sort(valid.begin(), valid.end(), std::greater<double>());
      const double cutoff = valid[std::min<size_t>((size_t)o.n_top, valid.size()) - 1];
      for (size_t j = 0; j < n; ++j) b.hv[j] = nan_to_num(b.norm[j]) >= cutoff ? 1 : 0;
    }
  } else {
    for (size_t j = 0; j < n; ++j) b.hv[j] = within_cutoffs(o, b.mean[j], b.norm[j]) ? 1 : 0;
  }
}

template <typename U>
void fill(U* out, size_t n, U v) {
  if (out) std::fill(out, out + n, v);
}
template <typename U>
void copy_to(U* out, const std::vector<U>& v) {
  if (out) std::copy(v.begin(), v.end(), out);
}

}  // namespace

template <typename T>
void hvg_moments(H& h, const CsrView<T>& A, const int32_t* d_batch, int32_t batch, int32_t transform, const double* clip, double* sum,
                 double* sumsq, uint64_t* n_clipped) {
  const std::string w("hvg_moments");
  SAPCA_CHECK(transform == SAPCA_HVG_CLIP || transform == SAPCA_HVG_EXPM1, SAPCA_ERR_ARG,
              w + ": transform = " + std::to_string(transform) + " is neither SAPCA_HVG_CLIP (0) nor SAPCA_HVG_EXPM1 (1)");
  check_rows((uint64_t)A.rows, w);
  SAPCA_CHECK(transform != SAPCA_HVG_CLIP || clip != nullptr || A.cols == 0, SAPCA_ERR_ARG,
              w + ": clip is NULL with transform SAPCA_HVG_CLIP and n = " + num((uint64_t)A.cols));
  SAPCA_CHECK(d_batch == nullptr || batch >= 0, SAPCA_ERR_ARG, w + ": batch = " + std::to_string(batch) + " is negative");
  check_view(A);
  const size_t n = (size_t)A.cols;
  if (n == 0) return;
  hipStream_t s = h.stream;
  HvgWork wk(h, n, 3);
  double *d_sum = wk.f64(0), *d_sq = wk.f64(1), *d_clip = wk.f64(2);
  if (transform == SAPCA_HVG_CLIP) SAPCA_HIP(hipMemcpyAsync(d_clip, clip, n * sizeof(double), hipMemcpyHostToDevice, s));
  const CsrView<T> At = transpose_into_at(h, A);
  k::hvg_moments(At, A.rows ? d_batch : nullptr, batch, 0, transform, d_clip, d_sum, d_sq, wk.iota, s);
  std::vector<double> hs(sum ? n : 0), hq(sumsq ? n : 0);
  std::vector<uint32_t> hc(n_clipped ? n : 0);
  fetch(hs, d_sum, s);
  fetch(hq, d_sq, s);
  fetch(hc, wk.iota, s);
  SAPCA_HIP(hipStreamSynchronize(s));   // (`clip` may go out of scope)
  copy_to(sum, hs);
  copy_to(sumsq, hq);
  if (n_clipped) std::copy(hc.begin(), hc.end(), n_clipped);
}

void loess(H& h, uint64_t n, const double* x, const double* y, double span, double* fitted) {
  const std::string w("loess");
  check_span(w, span);
  SAPCA_CHECK(n < (1ull << 31), SAPCA_ERR_ARG, w + ": n = " + num(n) + " points; 2^31 or more are not supported");
  SAPCA_CHECK(n == 0 || (x && y && fitted), SAPCA_ERR_ARG, w + ": a NULL array with n = " + num(n));
  if (n == 0) return;
  hipStream_t s = h.stream;
  HvgWork wk(h, n, 5);
  double *dx = wk.f64(0), *dy = wk.f64(1), *dfit = wk.f64(2);
  SAPCA_HIP(hipMemcpyAsync(dx, x, n * sizeof(double), hipMemcpyHostToDevice, s));
  SAPCA_HIP(hipMemcpyAsync(dy, y, n * sizeof(double), hipMemcpyHostToDevice, s));
  k::hvg_loess(dx, dy, (int64_t)n, (int64_t)n, loess_window(span, (int64_t)n), wk.f64(3), wk.f64(4), wk.iota, wk.perm, dfit, h.hvg.sort, s);
  SAPCA_HIP(hipMemcpyAsync(fitted, dfit, n * sizeof(double), hipMemcpyDeviceToHost, s));
  SAPCA_HIP(hipStreamSynchronize(s));
}

template <typename T>
void hvg(H& h, const CsrView<T>& A, const int32_t* d_batch, uint32_t n_batches, const sapca_hvg_options* o, double* means,
         double* variances, double* variances_norm, double* dispersions, double* dispersions_norm, double* rank, uint32_t* n_batches_hv,
         uint8_t* highly_variable) {
  const std::string w("hvg");
  check_options_header(o, "sapca_hvg_options", w);
  SAPCA_CHECK(o->flavor == SAPCA_HVG_SEURAT_V3 || o->flavor == SAPCA_HVG_SEURAT, SAPCA_ERR_ARG,
              w + ": flavor = " + std::to_string(o->flavor) + " is neither SAPCA_HVG_SEURAT_V3 (0) nor SAPCA_HVG_SEURAT (1)");
  const bool v3 = o->flavor == SAPCA_HVG_SEURAT_V3;
  SAPCA_CHECK(!v3 || o->n_top != 0, SAPCA_ERR_ARG, w + ": n_top = 0 with flavor SAPCA_HVG_SEURAT_V3, which ranks and needs a count");
  check_span(w, o->span);
  SAPCA_CHECK(o->n_bins != 0, SAPCA_ERR_ARG, w + ": n_bins = 0");
  SAPCA_CHECK(n_batches != 0, SAPCA_ERR_ARG, w + ": n_batches = 0");
  SAPCA_CHECK(d_batch == nullptr || n_batches <= SAPCA_HVG_MAX_BATCHES, SAPCA_ERR_ARG,
              w + ": n_batches = " + num(n_batches) + " exceeds SAPCA_HVG_MAX_BATCHES = " + num(SAPCA_HVG_MAX_BATCHES));
  check_rows((uint64_t)A.rows, w);
  check_view(A);
  const size_t n = (size_t)A.cols;
  const uint64_t m = (uint64_t)A.rows;
  if (n == 0) return;
  SAPCA_CHECK(o->n_top <= n, SAPCA_ERR_ARG, w + ": n_top = " + num(o->n_top) + " exceeds n = " + num(n) + " columns");
  if (m == 0) {
    fill(means, n, 0.0); fill(variances, n, 0.0);
    fill(variances_norm, n, v3 ? 0.0 : kNaN);
    fill(dispersions, n, v3 ? kNaN : 0.0); fill(dispersions_norm, n, v3 ? kNaN : 0.0);
    fill(rank, n, kNaN); fill(n_batches_hv, n, 0u); fill(highly_variable, n, (uint8_t)0);
    return;
  }
  const uint32_t K = d_batch ? n_batches : 1u;
  const std::vector<uint64_t> rows = batch_rows(h, d_batch, m, K);
  uint64_t included = 0;
  for (uint32_t b = 0; b < K; ++b) {
    SAPCA_CHECK(rows[b] >= 2, SAPCA_ERR_ARG, w + ": batch " + num(b) + " has " + num(rows[b]) + " rows; a variance needs 2");
    included += rows[b];
  }
  hipStream_t s = h.stream;
  const size_t top = (size_t)o->n_top;
  const CsrView<T> At = transpose_into_at(h, A);

  if (!v3) {
    HvgWork wk(h, n, 2);
    std::vector<SeuratBatch> bs(K);
    std::vector<double> hs(n), hq(n);
    for (uint32_t b = 0; b < K; ++b) {
      k::hvg_moments(At, d_batch, (int32_t)b, (int)K, SAPCA_HVG_EXPM1, nullptr, wk.f64(0), wk.f64(1), nullptr, s);
      fetch(hs, wk.f64(0), s);
      fetch(hq, wk.f64(1), s);
      SAPCA_HIP(hipStreamSynchronize(s));
      seurat_finish(*o, hs, hq, (double)rows[b], bs[b]);
    }
    std::vector<double> mean(n), var(n), disp(n), norm(n);
    std::vector<uint32_t> nhv(n, 0);
    std::vector<uint8_t> hv(n, 0);
    const auto nanmean = [&](size_t j, const std::vector<double> SeuratBatch::*f) {
      double acc = 0.0;
      uint32_t c = 0;
      for (uint32_t b = 0; b < K; ++b) {
        const double v = (bs[b].*f)[j];
        if (std::isnan(v)) continue;
        acc += v;
        ++c;
      }
      return c ? acc / (double)c : kNaN;
    };
    for (size_t j = 0; j < n; ++j) {
      if (K == 1) {
        mean[j] = bs[0].mean[j]; var[j] = bs[0].var[j]; disp[j] = bs[0].disp[j]; norm[j] = bs[0].norm[j];
      } else {
        mean[j] = nanmean(j, &SeuratBatch::mean); var[j] = nanmean(j, &SeuratBatch::var);
        disp[j] = nanmean(j, &SeuratBatch::disp); norm[j] = nanmean(j, &SeuratBatch::norm);
      }
      for (uint32_t b = 0; b < K; ++b) nhv[j] += bs[b].hv[j];
    }
    if (K == 1) {
      hv = bs[0].hv;
    } else if (top) {
      std::vector<uint32_t> order(n);
      std::iota(order.begin(), order.end(), 0u);
      std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
        if (nhv[a] != nhv[b]) return nhv[a] > nhv[b];
        const bool na = std::isnan(norm[a]), nb = std::isnan(norm[b]);
        if (na || nb) return !na && nb;
        return norm[a] > norm[b];
      });
      for (size_t r = 0; r < top; ++r) hv[order[r]] = 1;
    } else {
      for (size_t j = 0; j < n; ++j) hv[j] = within_cutoffs(*o, mean[j], norm[j]) ? 1 : 0;
    }
    copy_to(means, mean); copy_to(variances, var); copy_to(dispersions, disp); copy_to(dispersions_norm, norm);
    fill(variances_norm, n, kNaN); fill(rank, n, kNaN);
    copy_to(n_batches_hv, nhv); copy_to(highly_variable, hv);
    return;
  }

  // seurat_v3: s | ss | mean | var | lx | ly | est | reg_std | clip | cs | css | norm_var | xs | ys
  HvgWork wk(h, n, 14);
  double *d_s = wk.f64(0), *d_ss = wk.f64(1), *d_mean = wk.f64(2), *d_var = wk.f64(3), *d_lx = wk.f64(4), *d_ly = wk.f64(5),
         *d_est = wk.f64(6), *d_reg = wk.f64(7), *d_clip = wk.f64(8), *d_cs = wk.f64(9), *d_css = wk.f64(10), *d_nv = wk.f64(11);
  std::vector<std::vector<double>> nv(K, std::vector<double>(n));
  std::vector<double> mean(n), var(n);
  for (uint32_t b = 0; b < K; ++b) {
    const double N = (double)rows[b];
    k::hvg_moments(At, d_batch, (int32_t)b, (int)K, k::kHvgPlain, nullptr, d_s, d_ss, nullptr, s);
    k::hvg_mean_var(d_s, d_ss, N, (int64_t)n, d_mean, d_var, d_lx, d_ly, wk.counter, s);
    uint32_t valid = 0;
    SAPCA_HIP(hipMemcpyAsync(&valid, wk.counter, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    if (K == 1) {   // one batch: its moments are the overall ones
      fetch(mean, d_mean, s);
      fetch(var, d_var, s);
    }
    SAPCA_HIP(hipStreamSynchronize(s));   // (the window's length needs the count)
    SAPCA_HIP(hipMemsetAsync(d_est, 0, n * sizeof(double), s));
    k::hvg_loess(d_lx, d_ly, (int64_t)n, (int64_t)valid, loess_window(o->span, (int64_t)valid), wk.f64(12), wk.f64(13), wk.iota, wk.perm,
                 d_est, h.hvg.sort, s);
    k::hvg_clip(d_est, d_mean, N, (int64_t)n, d_reg, d_clip, s);
    k::hvg_moments(At, d_batch, (int32_t)b, (int)K, SAPCA_HVG_CLIP, d_clip, d_cs, d_css, nullptr, s);
    k::hvg_norm_var(d_cs, d_css, d_mean, d_reg, N, (int64_t)n, d_nv, s);
    fetch(nv[b], d_nv, s);
  }
  if (K > 1) {   // means and variances over all included rows
    k::hvg_moments(At, d_batch, -1, (int)K, k::kHvgPlain, nullptr, d_s, d_ss, nullptr, s);
    k::hvg_mean_var(d_s, d_ss, (double)included, (int64_t)n, d_mean, d_var, d_lx, d_ly, wk.counter, s);
    fetch(mean, d_mean, s);
    fetch(var, d_var, s);
  }
  SAPCA_HIP(hipStreamSynchronize(s));
  std::vector<double> rk(n), vnorm(n, 0.0);
  std::vector<uint32_t> nhv(n, 0);
  std::vector<std::vector<double>> ranks(n);
  for (uint32_t b = 0; b < K; ++b) {
    const std::vector<uint32_t> order = order_desc(nv[b].data(), n);
    for (size_t r = 0; r < top; ++r) ranks[order[r]].push_back((double)r);
    for (size_t j = 0; j < n; ++j) vnorm[j] += nv[b][j];
  }
  for (size_t j = 0; j < n; ++j) {
    nhv[j] = (uint32_t)ranks[j].size();
    rk[j] = median_of(ranks[j]);
    vnorm[j] /= (double)K;
  }
  std::vector<uint32_t> order(n);
  std::iota(order.begin(), order.end(), 0u);
  std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
    const bool na = std::isnan(rk[a]), nb = std::isnan(rk[b]);
    if (na != nb) return nb;
    if (!na && rk[a] != rk[b]) return rk[a] < rk[b];
    return nhv[a] > nhv[b];
  });
  std::vector<uint8_t> hv(n, 0);
  for (size_t r = 0; r < top; ++r) hv[order[r]] = 1;
  copy_to(means, mean); copy_to(variances, var); copy_to(variances_norm, vnorm);
  fill(dispersions, n, kNaN); fill(dispersions_norm, n, kNaN);
  copy_to(rank, rk); copy_to(n_batches_hv, nhv); copy_to(highly_variable, hv);
}

#define SAPCA_INSTANTIATE_HVG(T)                                                                                                      \
  template void hvg_moments<T>(H&, const CsrView<T>&, const int32_t*, int32_t, int32_t, const double*, double*, double*, uint64_t*); \
  template void hvg<T>(H&, const CsrView<T>&, const int32_t*, uint32_t, const sapca_hvg_options*, double*, double*, double*, double*, \
                       double*, double*, uint32_t*, uint8_t*);
SAPCA_INSTANTIATE_HVG(float)
SAPCA_INSTANTIATE_HVG(double)
#undef SAPCA_INSTANTIATE_HVG

}  // namespace resident
}  // namespace sapca
