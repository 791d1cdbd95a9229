// The counter-based generator of the device samplers (sampling.hip, word2vec.hip): every draw is a pure function of
// (seed, position), so there is no generator state and no dependence on the order of evaluation.
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

namespace lr {

__host__ __device__ inline uint64_t mix64(uint64_t z) {   // splitmix64 finaliser
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

}  // namespace lr
