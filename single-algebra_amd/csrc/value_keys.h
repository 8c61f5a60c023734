// The order-preserving unsigned image of a value: larger value <=> larger key (-0 just below +0; NaN unspecified).
// Shared by the radix select of batchstats.hip and the rank pass of rankgroups.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace sapca {
namespace k {

template <typename T> struct Keys;
template <> struct Keys<float> {
  using K = uint32_t;
  static constexpr int BITS = 32;
  __device__ static K key(float x) {
    const uint32_t u = __float_as_uint(x);
    return u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
  }
  __device__ static float value(K k) { return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xffffffffu)); }
};
template <> struct Keys<double> {
  using K = uint64_t;
  static constexpr int BITS = 64;
  __device__ static K key(double x) {
    const uint64_t u = (uint64_t)__double_as_longlong(x);
    return u ^ ((u >> 63) ? ~0ull : 0x8000000000000000ull);
  }
  __device__ static double value(K k) { return __longlong_as_double((long long)(k ^ ((k >> 63) ? 0x8000000000000000ull : ~0ull))); }
};

}  // namespace k
}  // namespace sapca
