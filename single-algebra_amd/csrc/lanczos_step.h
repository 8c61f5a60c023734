// The fixed-order f64 step kernels of lanczos.hip (classical Gram-Schmidt by two skinny GEMVs, norm, scale, Ritz combination)
// as launches another driver can share: spectral.cpp runs its Lanczos iteration with them.  The kernels are lanczos.hip's,
// unchanged; these are the launches lanczos_fit issues for an uncentred fit, with its grids.
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

namespace sapca {
namespace k {

constexpr int kLanczosPartialSlots = 1024;   // doubles of `partial` a pass may write
// h[i] = V[i] . w, i < nvec (V: nvec x len row-major)
void lanczos_gemv_t(const double* V, int64_t len, int nvec, const double* w, double* h, hipStream_t s);
// w -= sum_i h[i] V[i]
void lanczos_gemv_n_sub(const double* V, int64_t len, int nvec, const double* h, double* w, hipStream_t s);
// w -= sum_i h2[i] V[i], partial <- the blocks' shares of |w|^2, alpha[j] = h1[j] + h2[j]; returns the partial sums written
int lanczos_gemv_n_sub_norm(const double* V, int64_t len, int nvec, const double* h1, const double* h2, double* w, double* partial,
                            int j, double* alpha, hipStream_t s);
// partial <- the blocks' shares of |w|^2; returns the partial sums written
int lanczos_norm2(const double* w, int64_t len, double* partial, hipStream_t s);
// *beta_out = |w| from the partial sums, vnext = w / |w| (zeros for |w| = 0)
void lanczos_scale(const double* w, int64_t len, const double* partial, int nparts, double* beta_out, double* vnext, hipStream_t s);
// out[r * ldo + i] = sum_j V[j][r] S[j * k + i], i < k
template <typename T>
void lanczos_combine(const double* V, int64_t len, int nvec, const double* S, int k, int ldo, T* out, hipStream_t s);

}  // namespace k
}  // namespace sapca
