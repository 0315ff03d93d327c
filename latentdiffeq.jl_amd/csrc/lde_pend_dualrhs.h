// lde_pend_dualrhs.h — the pendulum's right-hand side on dual numbers: what the two kernels that carry ∂(x, v)/∂(x₀, v₀, L) through a solve
// share — k_pend_forward_dual (csrc/lde_pend_dual.hip: LDE_SENSE_FORWARD_DUAL on the deterministic pendulums) and k_pend_forward_sde
// (csrc/lde_pend_sde.hip: the stochastic pendulum's drift; its additive noise has zero partials).
#pragma once
#include "lde_device.h"
#include "lde_dual.h"   // DUAL_TS_LDS_MAX

namespace lde {

constexpr int DN = 8;                 // [x, v, ∂x/∂x₀, ∂x/∂v₀, ∂x/∂L, ∂v/∂x₀, ∂v/∂v₀, ∂v/∂L]

// du = [v, −(G/L) sin x (− (b/m) v)] on duals: ∂f/∂u = [[0, 1], [−(G/L) cos x, (−b/m)]], ∂f/∂L = [0, (G/L²) sin x]
template <int KIND>
struct PendDual {
  float ngl, gl2;   // −G/L, G/L²
  float noff;       // −(whole turns of the step's start angle): turn_anchor (lde_device.h)
  __device__ __forceinline__ explicit PendDual(float L) : ngl(-10.0f / L), gl2(10.0f / (L * L)), noff(0.f) {}
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
