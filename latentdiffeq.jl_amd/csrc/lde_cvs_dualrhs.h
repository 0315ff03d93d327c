// lde_cvs_dualrhs.h — the cardiovascular system (LDE_RHS_CVS: z = (p_a/100, p_v/10, s, sv/100), θ = (i_ext, r_mod); include/lde.h: "the
// cardiovascular system" — the GOKU-net paper's third benchmark, its form AS RECALLED from the authors' data generator, unpinned: neither
// the paper nor its code was at hand) as ONE LANE of the lane-per-direction dual solve sees it (csrc/lde_dual_dir.hip): D = 4 components,
// NP = 6 directions — q = 0 … 3: ẑ₀, seed e_q; q = 4: i_ext, q = 5: r_mod, zero seed and a parameter tangent on their own lane — in an
// 8-lane group whose lanes 6 and 7 are pad lanes: zero seed, zero parameter tangents, so their column starts at 0 and stays there. A lane
// carries u = [z (4), v (4)] with v = ∂z/∂q_q and evaluates f ONCE, on numbers with one partial (Dual1, csrc/lde_dpend_dualrhs.h): the value
// parts are the same instructions on the same inputs on every lane of a group, hence the same bits; the tangent parts differ by what the
// lane carries in v and in its parameters' tangents, which are per-lane constants — no lane branches.
//
// In the scaled state, with the constants folded at compile time:
//   f_hr  = s·(F_MAX − F_MIN) + F_MIN
//   r_tpr = s·(R_MAX − R_MIN) + (R_MIN − r_mod)
//   dva   = 100·z₃·f_hr − (100·z₀ − 10·z₁)/r_tpr
//   z₀' = dva/400,   z₁' = (i_ext − dva)/1110,   z₂' = (w − s)/TAU,   z₃' = i_ext·SV_MOD
// where w = 1 − σ(K_W·(p_a − P_SET)) is evaluated as 1/(1 + eˣ), x = K_W·(100·z₀ − P_SET), with the partial −K_W·w·(1 − w)·∂p_a written out
// (not taken through the reciprocal's rule): a pressure far from the set point gives eˣ = inf or 0, w = 0 or 1 and w·(1 − w) = 0 — no
// inf/inf and no inf·0 in a value or a tangent. eˣ is the hardware's exp2 behind the folded factor K_W·log₂e: at the pressures of the
// system |x| is a few units, the argument's rounding is 6e-8·|x·log₂e| and the instruction's own error ≈ 1 ulp — far inside the parity
// bounds, which the CPU reference alone sets (tests/cvs_ref.py). One exponential and two reciprocals (1/r_tpr, 1/(1 + eˣ)) per evaluation.
// z₃' depends on i_ext alone: its tangent is the constant SV_MOD on lane 4 and an exact 0 on every other lane. Nothing is anchored.
#pragma once
#include "lde_device.h"
#include "lde_dpend_dualrhs.h"   // Dual1 and its arithmetic

namespace lde {

struct CvsDir {
  static constexpr int D = 4;        // components: p_a/100, p_v/10, s, sv/100
  static constexpr int NP = 6;       // partial directions: ẑ₀ (4), i_ext, r_mod
  static constexpr int G = 8;        // lanes of a trajectory: lanes 6 and 7 are pad lanes
  static constexpr int DN = 2 * D;   // floats of a lane's state: the four values and its one tangent column
  static constexpr float F_MAX = 3.0f, F_MIN = 2.0f / 3.0f, R_MAX = 2.134f, R_MIN = 0.5335f, C_A = 4.0f, C_V = 111.0f;
  static constexpr float K_W = 0.1838f, P_SET = 70.0f, TAU = 20.0f, SV_MOD = 0.001f;
  static constexpr float LOG2E = 1.4426950408889634f;
  Dual1 iext;    // i_ext: tangent 1 on lane 4
  Dual1 rbase;   // R_MIN − r_mod: tangent −1 on lane 5
  Dual1 dz3;     // i_ext·SV_MOD: tangent SV_MOD on lane 4 — the whole fourth row

  // θ of trajectory b: (i_ext, r_mod); q: the lane's direction
  static __device__ __forceinline__ CvsDir load(const float* __restrict__ theta, long long b, int q) {
    CvsDir f;
    const float* th = theta + (size_t)2 * b;
    const float ie = th[0], rm = th[1];
    f.iext = {ie, q == 4 ? 1.f : 0.f};
    f.rbase = {R_MIN - rm, q == 5 ? -1.f : 0.f};
    f.dz3 = {ie * SV_MOD, q == 4 ? SV_MOD : 0.f};
    return f;
  }
  // seeds: ∂z(t₀)/∂ẑ₀ = I — lane q < 4 starts with e_q — and ∂/∂θ = 0; a pad lane starts (and stays) at zero
  static __device__ __forceinline__ void seed(const float* __restrict__ z0, long long b, int q, float (&y)[DN]) {
#pragma unroll
    for (int i = 0; i < D; i++) {
      y[i] = z0[(size_t)D * b + i];
      y[D + i] = q == i ? 1.f : 0.f;
    }
  }
  __device__ __forceinline__ void anchor(const float (&)[DN]) {}   // no angle: nothing to anchor
  __device__ __forceinline__ void operator()(const float (&u)[DN], float (&du)[DN]) const {
    const Dual1 Z0{u[0], u[4]}, Z1{u[1], u[5]}, S{u[2], u[6]}, Z3{u[3], u[7]};
    const Dual1 fhr = S * (F_MAX - F_MIN) + F_MIN;
    const Dual1 rr = dual_rcp(S * (R_MAX - R_MIN) + rbase);                      // 1/r_tpr
    const Dual1 dva = Z3 * 100.0f * fhr - (Z0 * 100.0f - Z1 * 10.0f) * rr;
    const Dual1 r0 = dva * (1.0f / (C_A * 100.0f)), r1 = (iext - dva) * (1.0f / (C_V * 10.0f));
    // w = 1/(1 + eˣ) and its partial −K_W·100·w·(1 − w)·v₀, written out: finite at eˣ = inf and at eˣ = 0
    const float e = __builtin_amdgcn_exp2f(fmaf(u[0], K_W * 100.0f * LOG2E, -K_W * P_SET * LOG2E));
    const float w = 1.0f / (1.0f + e);
    const Dual1 W{w, (-K_W * 100.0f) * (w * (1.0f - w)) * u[4]};
    const Dual1 r2 = (W - S) * (1.0f / TAU);
    du[0] = r0.v;
    du[1] = r1.v;
    du[2] = r2.v;
    du[3] = dz3.v;
    du[4] = r0.d;
    du[5] = r1.d;
    du[6] = r2.d;
    du[7] = dz3.d;
  }
};

}  // namespace lde
