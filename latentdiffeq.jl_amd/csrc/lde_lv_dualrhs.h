// lde_lv_dualrhs.h — the Lotka–Volterra system (LDE_RHS_LOTKA_VOLTERRA: dx = αx − βxy, dy = −γy + δxy) on dual numbers: values and
// NP = 6 partials per component, ∂(x, y)/∂(x₀, y₀, α, β, γ, δ). Polynomial — plain f32 arithmetic, no anchor, no transcendental. What a
// further two-state system needs in order to run on k_forward_dual (csrc/lde_dual.hip) is a struct of this shape: NP, load, seed, anchor
// and the right-hand side.
#pragma once
#include "lde_device.h"

namespace lde {

// ∂f/∂u = [[α − βy, −βx], [δy, −γ + δx]], ∂f/∂θ = [[x, −xy, 0, 0], [0, 0, −y, xy]]
struct LvDual {
  static constexpr int NP = 6;            // partials per component: x₀, y₀, α, β, γ, δ
  static constexpr int DN = 2 + 2 * NP;   // [x, y, ∂x/∂q (6), ∂y/∂q (6)]
  float al, be, ga, de;
  __device__ __forceinline__ LvDual(float a, float b, float g, float d) : al(a), be(b), ga(g), de(d) {}
  // θ of trajectory b: (α, β, γ, δ)
  static __device__ __forceinline__ LvDual load(const float* __restrict__ theta, int b) {
    const float* th4 = theta + (size_t)4 * b;
    return LvDual(th4[0], th4[1], th4[2], th4[3]);
  }
  // seeds: ∂(x, y)/∂(x₀, y₀) = I, ∂/∂θ = 0
  static __device__ __forceinline__ void seed(float u0, float u1, float (&y)[DN]) {
#pragma unroll
    for (int c = 0; c < DN; c++) y[c] = 0.f;
    y[0] = u0;
    y[1] = u1;
    y[2] = 1.f;
    y[2 + NP + 1] = 1.f;
  }
  __device__ __forceinline__ void anchor(float) {}
  __device__ __forceinline__ void operator()(const float (&u)[DN], float (&du)[DN]) const {
    const float x = u[0], y = u[1], xy = x * y;
    du[0] = al * x - be * xy;
    du[1] = de * xy - ga * y;
    const float a00 = al - be * y, a01 = -be * x, a10 = de * y, a11 = de * x - ga;
#pragma unroll
    for (int q = 0; q < NP; q++) {
      const float px = u[2 + q], py = u[2 + NP + q];
      du[2 + q] = a00 * px + a01 * py;
      du[2 + NP + q] = a10 * px + a11 * py;
    }
    du[2 + 2] += x;          // ∂f₀/∂α
    du[2 + 3] -= xy;         // ∂f₀/∂β
    du[2 + NP + 4] -= y;     // ∂f₁/∂γ
    du[2 + NP + 5] += xy;    // ∂f₁/∂δ
  }
};

}  // namespace lde
