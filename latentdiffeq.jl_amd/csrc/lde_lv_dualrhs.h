// lde_lv_dualrhs.h — the Lotka–Volterra right-hand side (LDE_RHS_LOTKA_VOLTERRA: dx = αx − βxy, dy = −γy + δxy) on dual numbers: values and
// NP = 6 partials per component, ∂(x, y)/∂(x₀, y₀, α, β, γ, δ). Polynomial — plain f32 arithmetic, no anchor, no transcendental. What a
// further two-state system needs in order to run on k_lv_forward_dual's scheme is a struct of this shape.
#pragma once
#include "lde_device.h"

namespace lde {

constexpr int LV_NP = 6;                // partials per component: x₀, y₀, α, β, γ, δ
constexpr int LV_DN = 2 + 2 * LV_NP;    // [x, y, ∂x/∂q (6), ∂y/∂q (6)]

// ∂f/∂u = [[α − βy, −βx], [δy, −γ + δx]], ∂f/∂θ = [[x, −xy, 0, 0], [0, 0, −y, xy]]
struct LvDual {
  float al, be, ga, de;
  __device__ __forceinline__ LvDual(float a, float b, float g, float d) : al(a), be(b), ga(g), de(d) {}
  __device__ __forceinline__ void operator()(const float (&u)[LV_DN], float (&du)[LV_DN]) const {
    const float x = u[0], y = u[1], xy = x * y;
    du[0] = al * x - be * xy;
    du[1] = de * xy - ga * y;
    const float a00 = al - be * y, a01 = -be * x, a10 = de * y, a11 = de * x - ga;
#pragma unroll
    for (int q = 0; q < LV_NP; q++) {
      const float px = u[2 + q], py = u[2 + LV_NP + q];
      du[2 + q] = a00 * px + a01 * py;
      du[2 + LV_NP + q] = a10 * px + a11 * py;
    }
    du[2 + 2] += x;             // ∂f₀/∂α
    du[2 + 3] -= xy;            // ∂f₀/∂β
    du[2 + LV_NP + 4] -= y;     // ∂f₁/∂γ
    du[2 + LV_NP + 5] += xy;    // ∂f₁/∂δ
  }
};

}  // namespace lde
