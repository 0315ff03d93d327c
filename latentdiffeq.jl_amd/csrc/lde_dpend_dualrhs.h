// lde_dpend_dualrhs.h — the double pendulum (LDE_RHS_DOUBLE_PENDULUM: z = (θ₁, θ₂, ω₁, ω₂), θ = (L₁, L₂, m₁, m₂), g = 10; include/lde.h: "the
// double pendulum") as ONE LANE of the lane-per-direction dual solve sees it (csrc/lde_dual_dir.hip): D = 4 components, NP = 8 directions —
// q = 0 … 3: ẑ₀, seed e_q; q = 4 … 7: L₁, L₂, m₁, m₂, zero seed and a parameter tangent on their own lane — exactly one 8-lane group with no
// pad lane. A lane carries u = [z (4), v (4)] with v = ∂z/∂q_q and evaluates f ONCE, on numbers with one partial (Dual1): the value parts
// are the same instructions on the same inputs on every lane of a group, hence the same bits; the tangent parts differ by what the lane
// carries in v and in its parameters' tangents, which are per-lane constants — no lane branches.
//
// With Δ = θ₁ − θ₂ the right-hand side is homogeneous of degree 0 in (m₁, m₂), and it is evaluated in the mass ratio μ = m₂/m₁ (numerators
// and denominator of include/lde.h's form divided by m₁):
//   den = 2 + μ − μ cos 2Δ
//   ω₁' = [ −g(2 + μ) sin θ₁ − μ g sin(θ₁ − 2θ₂) − 2 sinΔ · μ (ω₂² L₂ + ω₁² L₁ cosΔ) ] / (L₁ · den)
//   ω₂' = [ 2 sinΔ ( (1 + μ)(ω₁² L₁ + g cos θ₁) + ω₂² L₂ μ cosΔ ) ] / (L₂ · den)
// The two mass directions are then ∂μ/∂m₁ = −m₂/m₁² and ∂μ/∂m₂ = 1/m₁ on lanes 6 and 7: m₁ ∂ẑ/∂m₁ + m₂ ∂ẑ/∂m₂ vanishes to rounding, and at
// m₂ = 0 — where (θ₁, ω₁) is the pendulum of length L₁ — the columns ∂(θ₁, ω₁)/∂L₂ and ∂/∂m₁ are exact zeros, not rounding residue.
// Two hw_sincos per evaluation, on θ₁ and θ₂, each against its own turn_anchor taken once per step attempt; sin Δ, cos Δ, cos 2Δ and
// sin(θ₁ − 2θ₂) = sin(Δ − θ₂) come from those four numbers by the angle-sum identities: an angle past 256 turns keeps its dynamics. One
// division per evaluation (1/den); 1/L₁ and 1/L₂ are formed once per trajectory.
#pragma once
#include "lde_device.h"

namespace lde {

// a value and ONE partial
struct Dual1 {
  float v, d;
};
__device__ __forceinline__ Dual1 operator+(Dual1 a, Dual1 b) { return {a.v + b.v, a.d + b.d}; }
__device__ __forceinline__ Dual1 operator-(Dual1 a, Dual1 b) { return {a.v - b.v, a.d - b.d}; }
__device__ __forceinline__ Dual1 operator*(Dual1 a, Dual1 b) { return {a.v * b.v, a.d * b.v + a.v * b.d}; }
__device__ __forceinline__ Dual1 operator*(Dual1 a, float c) { return {a.v * c, a.d * c}; }
__device__ __forceinline__ Dual1 operator+(Dual1 a, float c) { return {a.v + c, a.d}; }
__device__ __forceinline__ Dual1 dual_rcp(Dual1 a) {
  const float r = 1.0f / a.v;
  return {r, -a.d * r * r};
}

struct DoublePendDir {
  static constexpr int D = 4;        // components: θ₁, θ₂, ω₁, ω₂
  static constexpr int NP = 8;       // partial directions: ẑ₀ (4), L₁, L₂, m₁, m₂
  static constexpr int G = 8;        // lanes of a trajectory: no pad lane
  static constexpr int DN = 2 * D;   // floats of a lane's state: the four values and its one tangent column
  static constexpr float GRAV = 10.0f;
  Dual1 l1, l2;      // L₁, L₂: tangent 1 on lanes 4 and 5
  Dual1 il1, il2;    // 1/L₁, 1/L₂: tangent −1/L² on those lanes
  Dual1 mu;          // m₂/m₁: tangent −m₂/m₁² on lane 6, 1/m₁ on lane 7
  float noff[2];     // −(whole turns of θ₁, θ₂ at the step's start): turn_anchor (lde_device.h)

  // θ of trajectory b: (L₁, L₂, m₁, m₂); q: the lane's direction
  static __device__ __forceinline__ DoublePendDir load(const float* __restrict__ theta, long long b, int q) {
    DoublePendDir f;
    const float* th = theta + (size_t)4 * b;
    const float L1 = th[0], L2 = th[1], m1 = th[2], m2 = th[3];
    const float i1 = 1.0f / L1, i2 = 1.0f / L2, im = 1.0f / m1;
    f.l1 = {L1, q == 4 ? 1.f : 0.f};
    f.l2 = {L2, q == 5 ? 1.f : 0.f};
    f.il1 = {i1, q == 4 ? -i1 * i1 : 0.f};
    f.il2 = {i2, q == 5 ? -i2 * i2 : 0.f};
    f.mu = {m2 * im, q == 6 ? -(m2 * im) * im : q == 7 ? im : 0.f};
    f.noff[0] = f.noff[1] = 0.f;
    return f;
  }
  // seeds: ∂z(t₀)/∂ẑ₀ = I — lane q < 4 starts with e_q — and ∂/∂θ = 0
  static __device__ __forceinline__ void seed(const float* __restrict__ z0, long long b, int q, float (&y)[DN]) {
#pragma unroll
    for (int i = 0; i < D; i++) {
      y[i] = z0[(size_t)D * b + i];
      y[D + i] = q == i ? 1.f : 0.f;
    }
  }
  __device__ __forceinline__ void anchor(const float (&y)[DN]) {
    noff[0] = turn_anchor(y[0]);
    noff[1] = turn_anchor(y[1]);
  }
  __device__ __forceinline__ void operator()(const float (&u)[DN], float (&du)[DN]) const {
    float s1, c1, s2, c2;
    hw_sincos(u[0], s1, c1, noff[0]);
    hw_sincos(u[1], s2, c2, noff[1]);
    const Dual1 S1{s1, c1 * u[4]}, C1{c1, -s1 * u[4]}, S2{s2, c2 * u[5]}, C2{c2, -s2 * u[5]};
    const Dual1 W1{u[2], u[6]}, W2{u[3], u[7]};
    const Dual1 sd = S1 * C2 - C1 * S2, cd = C1 * C2 + S1 * S2;   // sin Δ, cos Δ
    const Dual1 c2d = cd * cd - sd * sd;                          // cos 2Δ
    const Dual1 s12 = sd * C2 - cd * S2;                          // sin(θ₁ − 2θ₂) = sin(Δ − θ₂)
    const Dual1 rden = dual_rcp((mu + 2.0f) - mu * c2d);
    const Dual1 a = W1 * W1 * l1, b = W2 * W2 * l2;               // ω₁² L₁, ω₂² L₂
    const Dual1 num1 = ((mu + 2.0f) * S1 + mu * s12) * (-GRAV) - sd * mu * (b + a * cd) * 2.0f;
    const Dual1 num2 = sd * ((mu + 1.0f) * (a + C1 * GRAV) + b * mu * cd) * 2.0f;
    const Dual1 r1 = num1 * il1 * rden, r2 = num2 * il2 * rden;
    du[0] = u[2];
    du[1] = u[3];
    du[2] = r1.v;
    du[3] = r2.v;
    du[4] = u[6];
    du[5] = u[7];
    du[6] = r1.d;
    du[7] = r2.d;
  }
};

}  // namespace lde
