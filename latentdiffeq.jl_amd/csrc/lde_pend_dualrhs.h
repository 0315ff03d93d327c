// lde_pend_dualrhs.h — the pendulum as a system of the dual-number solve: what the kernels that carry ∂(x, v)/∂(x₀, v₀, L) through a solve
// share — k_forward_dual (csrc/lde_dual.hip: LDE_SENSE_FORWARD_DUAL on the deterministic pendulums) and k_pend_forward_sde
// (csrc/lde_pend_sde.hip: the stochastic pendulum's drift; its additive noise has zero partials).
#pragma once
#include "lde_device.h"
#include "lde_dual.h"

namespace lde {

// du = [v, −(G/L) sin x (− (b/m) v)] on duals: ∂f/∂u = [[0, 1], [−(G/L) cos x, (−b/m)]], ∂f/∂L = [0, (G/L²) sin x]
template <int KIND>
struct PendDual {
  static constexpr int NP = 3;            // partials per component: x₀, v₀, L
  static constexpr int DN = 2 + 2 * NP;   // [x, v, ∂x/∂x₀, ∂x/∂v₀, ∂x/∂L, ∂v/∂x₀, ∂v/∂v₀, ∂v/∂L]
  float ngl, gl2;   // −G/L, G/L²
  float noff;       // −(whole turns of the step's start angle): turn_anchor (lde_device.h)
  __device__ __forceinline__ explicit PendDual(float L) : ngl(-10.0f / L), gl2(10.0f / (L * L)), noff(0.f) {}
  // θ of trajectory b: its length L
  static __device__ __forceinline__ PendDual load(const float* __restrict__ theta, int b) { return PendDual(theta[b]); }
  // seeds: ∂y₀/∂x₀ = e₀, ∂y₀/∂v₀ = e₁, ∂y₀/∂L = 0
  static __device__ __forceinline__ void seed(float u0, float u1, float (&y)[DN]) {
    const float s[DN] = {u0, u1, 1.f, 0.f, 0.f, 0.f, 1.f, 0.f};
#pragma unroll
    for (int c = 0; c < DN; c++) y[c] = s[c];
  }
  __device__ __forceinline__ void anchor(float x0) { noff = turn_anchor(x0); }
  __device__ __forceinline__ void operator()(const float (&y)[DN], float (&dy)[DN]) const {
    float s, c;
    hw_sincos(y[0], s, c, noff);
    dy[0] = y[1];
    float acc = ngl * s;
    if (KIND == 1) acc -= 0.7f * y[1];
    dy[1] = acc;
    const float ngc = ngl * c;
#pragma unroll
    for (int q = 0; q < 3; q++) {
      dy[2 + q] = y[5 + q];
      float a = ngc * y[2 + q];
      if (KIND == 1) a -= 0.7f * y[5 + q];
      dy[5 + q] = a;
    }
    dy[7] += gl2 * s;
  }
};

}  // namespace lde
