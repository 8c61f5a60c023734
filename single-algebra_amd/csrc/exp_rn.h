// exp(x) for x <= 0 in double-double arithmetic, for host and device (tsne.hip uses it once per neighbour slot, after the
// search for beta has ended; tests/test_tsne_cpu.py compiles it for the host and holds it to 50-digit arithmetic).
// x = k ln 2 + r; the Taylor series of expm1 on r / 256 (|r / 256| < 1.4e-3: ten terms, truncation below 1e-35); eight
// squarings in the expm1 form (1 + e)^2 - 1 = 2 e + e^2; then 2^k.  The Taylor coefficients 1/3!, 1/4!, .. are plain doubles,
// each good to 2^-53 relative: the term r^3 / 6 is at most 3e-7 of expm1(r / 256), so the value before the final rounding is
// good to about 3e-7 * 2^-53 * 256 (the squarings double a relative error of e eight times) ~ 1e-20 relative, 1e-4 ulp: the
// result is the correctly rounded one unless exp(x) lies within about 1e-4 ulp of the midpoint of two doubles.
// The library exp is good to 1 ulp, and two such values added leave the 2 ulp that P is held to.
// Contraction is off in these functions: once inlined, a fused multiply-add takes a product unrounded into the sum that
// follows it, which counts a rounding error twice in the error-free sums (measured on gfx950: 7 % of P's f64 entries 1 to
// 3 ulp off) -- they must be evaluated as written.
#pragma once
#include <cmath>
#if !defined(__HIPCC__) && !defined(__host__)
#define __host__
#define __device__
#endif

namespace sapca {
namespace k {

struct dd {
  double hi, lo;
};
__host__ __device__ inline dd dd_renorm(double a, double b) {   // |a| >= |b|
#pragma clang fp contract(off)
  const double s = a + b;
  return dd{s, b - (s - a)};
}
__host__ __device__ inline dd dd_add(dd a, dd b) {
#pragma clang fp contract(off)
  const double s = a.hi + b.hi;
  const double bb = s - a.hi;
  const double e = (a.hi - (s - bb)) + (b.hi - bb);
  return dd_renorm(s, e + (a.lo + b.lo));
}
__host__ __device__ inline dd dd_mul(dd a, dd b) {
#pragma clang fp contract(off)
  const double p = a.hi * b.hi;
  const double e = fma(a.hi, b.hi, -p);
  return dd_renorm(p, e + (a.hi * b.lo + a.lo * b.hi));
}
__host__ __device__ inline double exp_rn(double x) {
#pragma clang fp contract(off)
  if (!(x > -745.2)) return x == x ? 0.0 : x;
  if (x > 0.0) x = 0.0;   // (not reached: the argument is -beta D)
  const double kf = rint(x * 1.44269504088896338700e+00);
  const double ln2_hi = 6.93147180369123816490e-01, ln2_lo = 1.90821492927058770002e-10;   // ln2_hi: 32 bits, k ln2_hi is exact
  const double r0 = x - kf * ln2_hi;
  const double pl = kf * ln2_lo;
  const double pe = fma(kf, ln2_lo, -pl);
  dd r = dd_add(dd{r0, 0.0}, dd{-pl, -pe});
  r.hi *= 0.00390625;
  r.lo *= 0.00390625;
  const double inv_fact[9] = {1.0 / 3628800.0, 1.0 / 362880.0, 1.0 / 40320.0, 1.0 / 5040.0, 1.0 / 720.0, 1.0 / 120.0, 1.0 / 24.0,
                              1.0 / 6.0, 0.5};
  dd s{inv_fact[0], 0.0};
#pragma unroll
  for (int i = 1; i < 9; ++i) s = dd_add(dd_mul(s, r), dd{inv_fact[i], 0.0});
  s = dd_add(dd_mul(s, r), dd{1.0, 0.0});
  dd e = dd_mul(s, r);   // expm1(r / 256)
#pragma unroll
  for (int i = 0; i < 8; ++i) e = dd_add(dd{2.0 * e.hi, 2.0 * e.lo}, dd_mul(e, e));
  const dd one_plus = dd_add(dd{1.0, 0.0}, e);
  return ldexp(one_plus.hi + one_plus.lo, (int)kf);
}

}  // namespace k
}  // namespace sapca
