// The symmetric eigenproblem of the l x l Gram matrix on the device (the small-SVD step, R11): opt-in under SAPCA_EIG_DEVICE,
// the host solver (small_svd.cpp) is the default.
#include "dense_common.h"

namespace sapca {
namespace k {

namespace {

// ---------------------------------------------------------------- symmetric eigenproblem of the l x l Gram (R11)
// One workgroup, everything in LDS (f64): parallel two-sided Jacobi.  A round pairs the l indices off (round-robin
// tournament, l - 1 rounds visit every pair once: a sweep); each pair (p, q) gets the rotation that annihilates a_pq, and
// since the pairs of a round are disjoint all of them are applied at once: the 2 x 2 block of A between pair a and pair b
// becomes Ja^T B Jb, touched by one thread and by nobody else, in place.  A is kept as its packed upper triangle, the
// eigenvector matrix V (rotated along with it) in full: l <= 112 fits the 160 KiB.  Converged when a whole sweep applied
// no rotation (|a_pq| <= 2^-53 sqrt(|a_pp a_qq|) for every pair): eigenvalues of a Gram matrix to high relative accuracy.
// Output: what the small-SVD step needs on the device -- M[i][j] = v_j[i] / sigma_j for the k leading eigenpairs in
// descending order (sigma_j = sqrt(lambda_j); a direction below 1e-12 sigma_0 stays zero), and sigma for the host.
constexpr int EIG_THREADS = 1024;
constexpr int EIG_MAX_L = 112;
constexpr int EIG_MAX_SWEEPS = 40;

__device__ __forceinline__ int eig_tri(int i, int j, int l) {   // packed upper triangle, i <= j
  return i * l - (i * (i - 1)) / 2 + (j - i);
}

__global__ void __launch_bounds__(EIG_THREADS)
sym_eig_jacobi_kernel(const double* __restrict__ G, int l, int ld, int k, int ldk, double* __restrict__ M, double* __restrict__ sigma_out,
                      int* __restrict__ status) {
  extern __shared__ double eig_lds[];
  const int L = (l + 1) & ~1;            // an odd l gets a dummy index (its pair idles)
  const int np = L / 2;
  const int vs = l | 1;                  // odd row stride of V
  double* A = eig_lds;                                   // l (l + 1) / 2
  double* V = A + (size_t)l * (l + 1) / 2;               // l x vs
  double* cs = V + (size_t)l * vs;                       // np x 2: cosine, sine of every pair
  int* pq = reinterpret_cast<int*>(cs + 2 * np);         // np x 2: the pair's indices, p < q (q = -1: idle)
  __shared__ int rotated, sweeps_done;
  const int tid = threadIdx.x;
  for (int e = tid; e < l * l; e += EIG_THREADS) {
    const int i = e / l, j = e % l;
    if (i <= j) A[eig_tri(i, j, l)] = 0.5 * (G[(size_t)i * ld + j] + G[(size_t)j * ld + i]);
    V[i * vs + j] = i == j ? 1.0 : 0.0;
  }
  if (tid == 0) { rotated = 0; sweeps_done = 0; }
  __syncthreads();
  // (elements below 1e-30 of the largest diagonal entry are left alone: a rank-deficient Gram would otherwise keep
  //  rotating rounding noise against its zero eigenvalues; directions below 1e-12 sigma_0 are dropped downstream anyway)
  __shared__ double floor_abs;
  if (tid == 0) {
    double mx = 0.0;
    for (int i = 0; i < l; ++i) mx = fmax(mx, fabs(A[eig_tri(i, i, l)]));
    floor_abs = mx * 1e-30;
  }
  __syncthreads();
  int sweep = 0;
  for (; sweep < EIG_MAX_SWEEPS; ++sweep) {
    for (int r = 0; r < L - 1; ++r) {
      // ---- the round's pairs and their rotations
      if (tid < np) {
        int a, b;
        if (tid == 0) { a = L - 1; b = r; }
        else { a = (r + tid) % (L - 1); b = (r - tid + (L - 1)) % (L - 1); }
        int p = min(a, b), q = max(a, b);
        double c = 1.0, sn = 0.0;
        if (q >= l) {
          q = -1;                                        // the dummy's partner sits this round out
        } else {
          const double app = A[eig_tri(p, p, l)], aqq = A[eig_tri(q, q, l)], apq = A[eig_tri(p, q, l)];
          if (fabs(apq) > 1.1102230246251565e-16 * sqrt(fabs(app * aqq)) && fabs(apq) > floor_abs) {
            const double tau = (aqq - app) / (2.0 * apq);
            const double t = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
            c = 1.0 / sqrt(1.0 + t * t);
            sn = t * c;
            atomicAdd(&rotated, 1);
          }
        }
        pq[2 * tid] = p;
        pq[2 * tid + 1] = q;
        cs[2 * tid] = c;
        cs[2 * tid + 1] = sn;
      }
      __syncthreads();
      // ---- blocks (pair a <= pair b) of A: B <- Ja^T B Jb with J = [c s; -s c]
      for (int e = tid; e < np * np; e += EIG_THREADS) {
        const int pa = e / np, pb = e % np;
        if (pb < pa) continue;
        const int p = pq[2 * pa], q = pq[2 * pa + 1];
        const double ca = cs[2 * pa], sa = cs[2 * pa + 1];
        if (pa == pb) {
          if (q < 0 || sa == 0.0) continue;
          const int ipp = eig_tri(p, p, l), iqq = eig_tri(q, q, l), ipq = eig_tri(p, q, l);
          const double app = A[ipp], aqq = A[iqq], apq = A[ipq];
          const double t = sa / ca;
          A[ipp] = app - t * apq;
          A[iqq] = aqq + t * apq;
          A[ipq] = 0.0;
          continue;
        }
        const int rr = pq[2 * pb], ss = pq[2 * pb + 1];
        const double cb = cs[2 * pb], sb = cs[2 * pb + 1];
        if (sa == 0.0 && sb == 0.0) continue;
        // the four elements between {p, q} and {rr, ss} (those that exist), each at its place in the upper triangle
        auto at = [&](int i, int j) { return i <= j ? eig_tri(i, j, l) : eig_tri(j, i, l); };
        const bool hq = q >= 0, hs = ss >= 0;
        const int i_pr = at(p, rr), i_ps = hs ? at(p, ss) : 0, i_qr = hq ? at(q, rr) : 0, i_qs = (hq && hs) ? at(q, ss) : 0;
        const double b_pr = A[i_pr], b_ps = hs ? A[i_ps] : 0.0, b_qr = hq ? A[i_qr] : 0.0, b_qs = (hq && hs) ? A[i_qs] : 0.0;
        // rows: (p, q) <- Ja^T
        const double r_pr = ca * b_pr - sa * b_qr, r_qr = sa * b_pr + ca * b_qr;
        const double r_ps = ca * b_ps - sa * b_qs, r_qs = sa * b_ps + ca * b_qs;
        // columns: (rr, ss) <- Jb
        A[i_pr] = cb * r_pr - sb * r_ps;
        if (hs) A[i_ps] = sb * r_pr + cb * r_ps;
        if (hq) A[i_qr] = cb * r_qr - sb * r_qs;
        if (hq && hs) A[i_qs] = sb * r_qr + cb * r_qs;
      }
      // ---- V <- V J
      for (int e = tid; e < l * np; e += EIG_THREADS) {
        const int i = e / np, pa = e % np;
        const int p = pq[2 * pa], q = pq[2 * pa + 1];
        const double sa = cs[2 * pa + 1];
        if (q < 0 || sa == 0.0) continue;
        const double ca = cs[2 * pa];
        const double vp = V[i * vs + p], vq = V[i * vs + q];
        V[i * vs + p] = ca * vp - sa * vq;
        V[i * vs + q] = sa * vp + ca * vq;
      }
      __syncthreads();
    }
    const int done = rotated == 0;
    __syncthreads();
    if (tid == 0) { rotated = 0; sweeps_done = sweep + 1; }
    __syncthreads();
    if (done) break;
  }
  // ---- eigenvalues in descending order (ties by index), M = V_sorted[:, :k] diag(1 / sigma)
  double* lam = cs;                                      // (the pair table is free now: l <= 2 np doubles)
  int* rank = pq;
  if (tid < l) lam[tid] = A[eig_tri(tid, tid, l)];
  __syncthreads();
  if (tid < l) {
    const double mine = lam[tid];
    int rk = 0;
    for (int j = 0; j < l; ++j) {
      const double o = lam[j];
      rk += (o > mine || (o == mine && j < tid)) ? 1 : 0;
    }
    rank[tid] = rk;
  }
  __syncthreads();
  __shared__ double sigma0;
  if (tid < l && rank[tid] == 0) sigma0 = sqrt(fmax(lam[tid], 0.0));
  __syncthreads();
  for (int e = tid; e < ld * ldk; e += EIG_THREADS) M[e] = 0.0;
  __syncthreads();
  const double tiny = sigma0 * 1e-12;
  int bad = 0;
  if (tid < l) {
    const double w = lam[tid];
    const double sg = sqrt(fmax(w, 0.0));
    sigma_out[rank[tid]] = isfinite(w) ? sg : w;   // (a non-finite eigenvalue reaches the host as it is: the fit then fails there)
    if (!isfinite(w)) bad = 1;
  }
  for (int e = tid; e < l * l; e += EIG_THREADS) {
    const int i = e / l, t = e % l;                    // component i of eigenvector t
    const int j = rank[t];
    const double sg = sqrt(fmax(lam[t], 0.0));
    if (j < k && sg > tiny) M[(size_t)i * ldk + j] = V[i * vs + t] / sg;
  }
  if (bad) atomicOr(status, 2);
  if (tid == 0 && sweep >= EIG_MAX_SWEEPS) atomicOr(status, 1);
  if (tid == 0) status[1] = sweeps_done;
}

}  // namespace

bool sym_eig_device_ok(int l) {
  // Opt-in (SAPCA_EIG_DEVICE=1; read per fit, the tests switch it).  Measured on MI355X: 1.03 ms at l = 60 and 5 ms at l = 110
  // (nine sweeps, 1.9 us per round: two workgroup barriers and a chain of f64 divisions and square roots per round) against
  // 0.27 ms / 1.0 ms for the host's Householder + QL including both crossings -- one workgroup is the wrong machine for
  // this problem, so the host solver stays the default and this kernel documents the attempt.
  const bool on = dbg_env("SAPCA_EIG_DEVICE") != nullptr;
  return on && l >= 1 && l <= EIG_MAX_L;
}

void sym_eig_device(const double* G, int l, int ld, int k, int ldk, double* M, double* sigma, int* status, hipStream_t s) {
  SAPCA_CHECK(sym_eig_device_ok(l) && k <= l && k <= ldk && l <= ld, SAPCA_ERR_ARG, "sym_eig_device: unsupported size");
  const int L = (l + 1) & ~1, np = L / 2, vs = l | 1;
  const size_t lds = ((size_t)l * (l + 1) / 2 + (size_t)l * vs + 2 * (size_t)np) * sizeof(double) + 2 * (size_t)np * sizeof(int) + 64;
  static LdsAttrState attr;
  ensure_dynamic_lds(reinterpret_cast<const void*>(&sym_eig_jacobi_kernel), lds, attr);
  SAPCA_HIP(hipMemsetAsync(status, 0, 2 * sizeof(int), s));
  hipLaunchKernelGGL(sym_eig_jacobi_kernel, dim3(1), dim3(EIG_THREADS), lds, s, G, l, ld, k, ldk, M, sigma, status);
  SAPCA_HIP(hipGetLastError());
}

}  // namespace k
}  // namespace sapca
