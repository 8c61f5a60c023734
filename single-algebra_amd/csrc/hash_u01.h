// The counter generator of rng.hip (the same function as sapca.synth.hash_u01): a uniform in [0, 1) as a pure function of
// (seed, stream, index).  Device code; include from a .hip file.
#pragma once
#include <cstdint>

namespace sapca {
namespace k {

__device__ inline uint64_t mix64(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

__device__ inline double hash_u01(uint64_t seed, uint64_t stream, uint64_t idx) {
  const uint64_t key = seed * 0xD1342543DE82EF95ull + stream * 0x2545F4914F6CDD1Dull + 0x1234567ull;
  uint64_t z = mix64(idx ^ key);
  z = mix64(z + key);
  return (double)(z >> 11) * (1.0 / 9007199254740992.0);
}

}  // namespace k
}  // namespace sapca
