// sapca_rank_sums_csr_device_* / sapca_rank_groups_csr_device_*: marker genes of a labelled resident CSR (include/sapca.h, "Rank
// groups").  Host side: the refusals, the group sizes, the transposition, the rank pass by length class (rankgroups.hip), the
// moments through the labelled statistics of batchstats.hip, and the f64 finish on K x n values.
#include <cmath>

#include "rankgroups.h"
#include "resident.h"

namespace sapca {
namespace resident {

namespace {

// What the device passes leave on the host, code-major K x n where per group and column.
struct RankParts {
  uint64_t M = 0;                  // included rows
  std::vector<uint64_t> group;     // n_g (K)
  std::vector<int64_t> rs2;        // twice the rank sums (ranks)
  std::vector<uint32_t> cnt;       // stored non-zero entries (ranks or counts)
  std::vector<double> tie;         // per column (ranks)
  std::vector<double> s, q;        // sum and sum of squares of the stored entries (moments)
};

// Everything that can be refused is refused here, before anything is enqueued or a buffer is touched.
template <typename T>
void check_rank_args(const char* who, const CsrView<T>& A, const int32_t* d_labels, uint32_t n_groups, int32_t tie_correct) {
  const std::string w(who);
  SAPCA_CHECK(n_groups != 0, SAPCA_ERR_ARG, w + ": n_groups is 0");
  SAPCA_CHECK(n_groups <= SAPCA_RANK_MAX_GROUPS, SAPCA_ERR_ARG,
              w + ": n_groups = " + std::to_string(n_groups) + " exceeds SAPCA_RANK_MAX_GROUPS = " + std::to_string(SAPCA_RANK_MAX_GROUPS));
  SAPCA_CHECK((uint64_t)A.rows < (1ull << 31), SAPCA_ERR_ARG,
              w + ": m = " + std::to_string((uint64_t)A.rows) + " rows; 2^31 or more are not supported");
  SAPCA_CHECK(tie_correct == 0 || tie_correct == 1, SAPCA_ERR_ARG, w + ": tie_correct = " + std::to_string(tie_correct) + " is neither 0 nor 1");
  SAPCA_CHECK(d_labels != nullptr || A.rows == 0, SAPCA_ERR_ARG, w + ": d_labels is NULL with m = " + std::to_string((uint64_t)A.rows));
  check_view(A);
}

// The device passes: group sizes always; ranks: the rank pass (rank sums, counts, tie sums); counts: the counts without a sort
// (ignored with ranks); moments: sum and sum of squares per group and column.
template <typename T>
void run_passes(H& h, const CsrView<T>& A, const int32_t* d_labels, uint32_t K, bool ranks, bool counts, bool moments, RankParts& out) {
  hipStream_t s = h.stream;
  const uint64_t m = (uint64_t)A.rows, n = (uint64_t)A.cols;
  out.group.assign(K, 0);
  unsigned long long* d_group = h.rank.group.as<unsigned long long>(K);
  k::rank_group_sizes(d_labels, (int64_t)m, (int)K, d_group, s);   // (m == 0: zeroes them, reads no label)
  static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "group sizes are fetched as they are");
  fetch(out.group, reinterpret_cast<const uint64_t*>(d_group), s);
  counts = counts && !ranks;
  const bool matrix = n > 0 && (ranks || counts || moments);
  CsrView<T> At;
  std::vector<int64_t> at_ptr;
  if (matrix) {
    At = transpose_into_at(h, A);   // (an empty matrix: n empty rows)
    if (ranks) {
      at_ptr.resize(n + 1);
      fetch(at_ptr, At.ptr, s);
    }
  }
  SAPCA_HIP(hipStreamSynchronize(s));
  out.M = 0;
  for (uint64_t g : out.group) out.M += g;
  if (!matrix) return;
  const size_t cells = (size_t)K * n;
  if (ranks || counts) {
    // rank sums (i64, cells) | tie sums (f64, n) | counts (u32, cells)
    char* base = h.rank.out.as<char>(cells * 12 + n * 8 + 16);
    long long* d_rs = reinterpret_cast<long long*>(base);
    double* d_tie = reinterpret_cast<double*>(base + cells * 8);
    uint32_t* d_cnt = reinterpret_cast<uint32_t*>(base + cells * 8 + n * 8);
    std::vector<int32_t> cols;    // the long columns, batch after batch
    std::vector<uint32_t> segs;   // per batch: its columns' offsets in the key scratch, from 0, and the batch's total
    struct Batch { size_t first, nseg, seg_at; };
    std::vector<Batch> batches;
    if (ranks) {
      k::rank_sums_lds(At, d_labels, (int)K, d_group, (int64_t)out.M, d_rs, d_cnt, d_tie, s);
      int64_t total = 0;
      for (uint64_t j = 0; j < n; ++j) {
        const int64_t len = at_ptr[j + 1] - at_ptr[j];
        if (len <= k::kRankLdsMax) continue;
        if (batches.empty() || total + len > k::kRankLongBatch) {
          batches.push_back({cols.size(), 0, segs.size()});
          segs.push_back(0u);
          total = 0;
        }
        total += len;
        cols.push_back((int32_t)j);
        segs.push_back((uint32_t)total);
        ++batches.back().nseg;
      }
      if (!batches.empty()) {
        char* lb = h.rank.list.as<char>((cols.size() + segs.size()) * 4);
        int32_t* d_cols = reinterpret_cast<int32_t*>(lb);
        uint32_t* d_segs = reinterpret_cast<uint32_t*>(lb + cols.size() * 4);
        SAPCA_HIP(hipMemcpyAsync(d_cols, cols.data(), cols.size() * 4, hipMemcpyHostToDevice, s));
        SAPCA_HIP(hipMemcpyAsync(d_segs, segs.data(), segs.size() * 4, hipMemcpyHostToDevice, s));
        for (const Batch& b : batches)   // (one after the other on the stream: they share the scratch)
          k::rank_sums_long(At, d_labels, (int)K, d_group, (int64_t)out.M, d_cols + b.first, d_segs + b.seg_at, (int)b.nseg,
                            segs[b.seg_at + b.nseg], h.rank.scratch, d_rs, d_cnt, d_tie, s);
      }
      out.rs2.resize(cells);
      out.tie.resize(n);
      static_assert(sizeof(long long) == sizeof(int64_t), "rank sums are fetched as they are");
      fetch(out.rs2, reinterpret_cast<const int64_t*>(d_rs), s);
      fetch(out.tie, d_tie, s);
    } else {
      k::rank_count_nonzero(At, d_labels, (int)K, d_cnt, s);
    }
    out.cnt.resize(cells);
    fetch(out.cnt, d_cnt, s);
    SAPCA_HIP(hipStreamSynchronize(s));   // (cols / segs may go)
  }
  if (moments) {
    out.s.resize(cells);
    out.q.resize(cells);
    for_each_code_slice(h, At, d_labels, K, [&](uint32_t lo, int nb, const std::vector<double>& hs, const std::vector<double>& hm,
                                                const std::vector<uint32_t>& hc) {
      for (size_t c = 0; c < (size_t)nb * n; ++c) {
        const size_t o = (size_t)lo * n + c;
        out.s[o] = hs[c];
        out.q[o] = hc[c] ? hm[c] + hs[c] * hs[c] / (double)hc[c] : 0.0;   // q = m2 + s^2 / c over the stored entries
      }
    });
  }
}

// max(0, (q - s^2 / k) / (k - 1)), 0 when k < 2
double sample_var(double s, double q, uint64_t k) {
  if (k < 2) return 0.0;
  const double v = (q - s * s / (double)k) / (double)(k - 1);
  return v > 0.0 ? v : 0.0;
}

}  // namespace

template <typename T>
void rank_sums(H& h, const CsrView<T>& A, const int32_t* d_labels, uint32_t n_groups, uint64_t* group_rows, int64_t* rank_sum2,
               uint64_t* nonzero, double* tie_sum) {
  check_rank_args("rank_sums", A, d_labels, n_groups, 0);
  RankParts p;
  run_passes(h, A, d_labels, n_groups, rank_sum2 != nullptr || tie_sum != nullptr, nonzero != nullptr, false, p);
  const size_t n = (size_t)A.cols, cells = (size_t)n_groups * n;
  if (group_rows) std::copy(p.group.begin(), p.group.end(), group_rows);
  if (rank_sum2 && cells) std::copy(p.rs2.begin(), p.rs2.end(), rank_sum2);
  if (tie_sum && n) std::copy(p.tie.begin(), p.tie.end(), tie_sum);
  if (nonzero)
    for (size_t c = 0; c < cells; ++c) nonzero[c] = p.cnt[c];
}

template <typename T>
void rank_groups(H& h, const CsrView<T>& A, const int32_t* d_labels, uint32_t n_groups, int32_t tie_correct, uint64_t* group_rows,
                 double* mean, double* var, uint64_t* nonzero, double* t_score, double* t_df, double* z_score, double* z_pvalue) {
  check_rank_args("rank_groups", A, d_labels, n_groups, tie_correct);
  const bool ranks = z_score != nullptr || z_pvalue != nullptr;
  const bool moments = mean != nullptr || var != nullptr || t_score != nullptr || t_df != nullptr;
  RankParts p;
  run_passes(h, A, d_labels, n_groups, ranks, nonzero != nullptr, moments, p);
  const size_t n = (size_t)A.cols, K = n_groups;
  const uint64_t M = p.M;
  if (group_rows) std::copy(p.group.begin(), p.group.end(), group_rows);
  if (nonzero)
    for (size_t c = 0; c < K * n; ++c) nonzero[c] = p.cnt[c];
  if (ranks) {
    const double m3 = (double)M * (double)M * (double)M - (double)M;
    for (size_t g = 0; g < K; ++g) {
      const uint64_t ng = p.group[g], nr = M - ng;
      for (size_t j = 0; j < n; ++j) {
        const size_t c = g * n + j;
        double z = 0.0, pv = 1.0;
        if (ng != 0 && nr != 0) {
          const double tcorr = tie_correct ? 1.0 - p.tie[j] / m3 : 1.0;
          const double sd = std::sqrt((double)ng * (double)nr * (double)(M + 1) / 12.0 * tcorr);
          if (sd > 0.0) {
            z = 0.5 * (double)(p.rs2[c] - (int64_t)(ng * (M + 1))) / sd;   // R_g - n_g (M + 1) / 2, the difference exact
            pv = std::erfc(std::fabs(z) / std::sqrt(2.0));
          }
        }
        if (z_score) z_score[c] = z;
        if (z_pvalue) z_pvalue[c] = pv;
      }
    }
  }
  if (moments) {
    std::vector<double> s_tot(n, 0.0), q_tot(n, 0.0);
    for (size_t g = 0; g < K; ++g)   // the totals: over g = 0 .. K - 1 in that order
      for (size_t j = 0; j < n; ++j) {
        s_tot[j] += p.s[g * n + j];
        q_tot[j] += p.q[g * n + j];
      }
    for (size_t g = 0; g < K; ++g) {
      const uint64_t ng = p.group[g], nr = M - ng;
      for (size_t j = 0; j < n; ++j) {
        const size_t c = g * n + j;
        const double s = p.s[c], q = p.q[c], sr = s_tot[j] - s, qr = q_tot[j] - q;
        const double mean_g = ng ? s / (double)ng : 0.0, var_g = sample_var(s, q, ng);
        if (mean) mean[c] = mean_g;
        if (var) var[c] = var_g;
        double t = 0.0, df = 0.0;
        if (ng != 0 && nr != 0) {
          const double mean_r = sr / (double)nr, var_r = sample_var(sr, qr, nr);
          const double vg = var_g / (double)ng, vr = var_r / (double)nr;
          const double sd = std::sqrt(vg + vr);
          if (sd > 0.0) {
            t = (mean_g - mean_r) / sd;
            if (ng >= 2 && nr >= 2) df = (vg + vr) * (vg + vr) / (vg * vg / (double)(ng - 1) + vr * vr / (double)(nr - 1));
          }
        }
        if (t_score) t_score[c] = t;
        if (t_df) t_df[c] = df;
      }
    }
  }
}

#define SAPCA_INSTANTIATE_RANK(T)                                                                                                    \
  template void rank_sums<T>(H&, const CsrView<T>&, const int32_t*, uint32_t, uint64_t*, int64_t*, uint64_t*, double*);             \
  template void rank_groups<T>(H&, const CsrView<T>&, const int32_t*, uint32_t, int32_t, uint64_t*, double*, double*, uint64_t*,    \
                               double*, double*, double*, double*);
SAPCA_INSTANTIATE_RANK(float)
SAPCA_INSTANTIATE_RANK(double)
#undef SAPCA_INSTANTIATE_RANK

}  // namespace resident
}  // namespace sapca
