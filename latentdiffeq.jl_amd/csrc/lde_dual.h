// lde_dual.h — the step control of a solve on dual numbers (LDE_SENSE_FORWARD_DUAL), over "a two-state system with NP partials per
// component": what decides the steps of k_pend_forward_dual (csrc/lde_pend_dual.hip, NP = 3: x₀, v₀, L) and k_lv_forward_dual
// (csrc/lde_lv_dual.hip, NP = 6: x₀, y₀, α, β, γ, δ) — the dual norms, their squares, the RMS (accumulated in f64 as the checkers do) and the
// Hairer initial step, in the checkers' order of operations (oracle/: dual_solve; tests/lv_ref.py). A dual state is 2 + 2·NP floats:
// [u₀, u₁, ∂u₀/∂q (NP), ∂u₁/∂q (NP)].
#pragma once
#include "lde_device.h"

namespace lde {

constexpr int DUAL_TS_LDS_MAX = 6000;   // doubles of the save-time grid kept in LDS (48 KB)

// ‖u_i‖ of component i as ODE_DEFAULT_NORM takes it on a dual: sqrt(v² + Σ_q p_q²), the squares added in the checker's order, unfused
template <int NP>
__device__ __forceinline__ float dual_abs(const float (&u)[2 + 2 * NP], int i) {
#pragma clang fp contract(off)
  float s2 = u[i] * u[i];
#pragma unroll
  for (int q = 0; q < NP; q++) s2 += u[2 + NP * i + q] * u[2 + NP * i + q];
  return sqrtf(s2);
}

// RMS over the two components of ‖e_i‖ / sk_i: each ratio and its square in f32, the sum of squares and the root in f64 (oracle: dual_rms)
template <int NP>
__device__ __forceinline__ double dual_rms(const float (&e)[2 + 2 * NP], const float (&sk)[2]) {
#pragma clang fp contract(off)
  double s2 = 0.0;
#pragma unroll
  for (int i = 0; i < 2; i++) {
    const float r = dual_abs<NP>(e, i) / sk[i];
    s2 += (double)(r * r);
  }
  return sqrt(s2 / 2.0);
}

// Hairer–Nørsett–Wanner initial step with every norm the dual norm; f0 = f(y0) given (oracle: dual_solve's initial step)
template <int NP, class F>
__device__ __forceinline__ double dual_init_dt(F& f, const float (&y)[2 + 2 * NP], const float (&f0)[2 + 2 * NP], double dtmax, const KOpts& o) {
  constexpr int DN = 2 + 2 * NP;
  float sk[2];
  {
#pragma clang fp contract(off)
#pragma unroll
    for (int i = 0; i < 2; i++) sk[i] = o.abstol + dual_abs<NP>(y, i) * o.reltol;
  }
  const double d0 = dual_rms<NP>(y, sk), d1 = dual_rms<NP>(f0, sk);
  double dt0 = (d0 < 1e-5 || d1 < 1e-5) ? 1e-6 : 0.01 * d0 / d1;
  if (dt0 > dtmax) dt0 = dtmax;
  const float h = (float)dt0;
  float tmp[DN], f1[DN];
#pragma unroll
  for (int c = 0; c < DN; c++) tmp[c] = y[c] + h * f0[c];
  f(tmp, f1);
#pragma unroll
  for (int c = 0; c < DN; c++) f1[c] -= f0[c];
  const double d2 = dual_rms<NP>(f1, sk) / dt0, dm = d1 > d2 ? d1 : d2;
  const double dt1 = (dm <= 1e-15) ? fmax(1e-6, dt0 * 1e-3) : pow(10.0, -(2.0 + log10(dm)) / 5.0);
  const double dt = fmin(100.0 * dt0, dt1);
  return dt > dtmax ? dtmax : dt;
}

// EEst of a Tsit5 attempt on duals: e = h·Σ_j b̃_j k_j per component, scale abstol + reltol·max(‖y_i‖, ‖y_new,i‖), RMS of ‖e_i‖ / scale
template <int NP>
__device__ __forceinline__ float dual_eest(float h, const float (&y)[2 + 2 * NP], const float (&yn)[2 + 2 * NP], const float (&k)[7][2 + 2 * NP],
                                           const KOpts& o) {
  constexpr int DN = 2 + 2 * NP;
  float e[DN];
#pragma unroll
  for (int c = 0; c < DN; c++) {
    float a = ts5::BT[0] * k[0][c];
#pragma unroll
    for (int j = 1; j < 7; j++) a += ts5::BT[j] * k[j][c];
    e[c] = a * h;
  }
  float sk[2];
  {
#pragma clang fp contract(off)
#pragma unroll
    for (int i = 0; i < 2; i++) sk[i] = o.abstol + fmaxf(dual_abs<NP>(y, i), dual_abs<NP>(yn, i)) * o.reltol;
  }
  return (float)dual_rms<NP>(e, sk);
}

}  // namespace lde
