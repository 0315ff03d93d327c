// lde_philox.h — the counter-based generator of the library, device side: Philox4x32-10 [Salmon, Moraes, Dror, Shaw: "Parallel random numbers:
// as easy as 1, 2, 3", SC'11] — what torch and Julia's Random123 use — and the Box–Muller map of a pair of its words. Shared by lde_randn
// (csrc/lde_loss.hip: the ε of the variational sample) and the stochastic pendulum's stepper (csrc/lde_pend_sde.hip: the ΔW of a substep);
// tests/philox_ref.py restates both on the CPU, tests/test_philox.py pins the words by the generator's published known-answer vectors.
#pragma once
#include <hip/hip_runtime.h>

namespace lde {

__device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1, unsigned (&o)[4]) {
#pragma unroll
  for (int r = 0; r < 10; r++) {
    const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
    const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n1 = (unsigned)p1, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1, n3 = (unsigned)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  o[0] = c0; o[1] = c1; o[2] = c2; o[3] = c3;
}

// two words → two independent N(0, 1): u = ((w >> 8) + ½)/2²⁴ ∈ (0, 1) (24 bits, never 0), (√(−2 ln u₁)·cos 2πu₂, √(−2 ln u₁)·sin 2πu₂)
__device__ __forceinline__ void box_muller_pair(unsigned w1, unsigned w2, float& za, float& zb) {
  const float u1 = ((float)(w1 >> 8) + 0.5f) * (1.0f / 16777216.0f);
  const float u2 = ((float)(w2 >> 8) + 0.5f) * (1.0f / 16777216.0f);
  const float rad = sqrtf(-2.0f * logf(u1));
  float sn, cs;
  sincospif(2.0f * u2, &sn, &cs);
  za = rad * cs;
  zb = rad * sn;
}

}  // namespace lde
