// lde_sl_dualrhs.h — the Stuart–Landau network (LDE_RHS_STUART_LANDAU: N Hopf normal-form oscillators with uniform all-to-all diffusive
// coupling, z = (x₁ … x_N, y₁ … y_N), θ = (a₁ … a_N, ω₁ … ω_N, G); include/lde.h: "the Stuart–Landau network" — GOKU-UI's latent system, its
// form AS RECALLED from the literature, unpinned) as ONE LANE of the lane-per-direction solves sees it (csrc/lde_dual_dir.hip): D = 2N
// components, NP = 4N + 1 directions — q = 0 … 2N−1: ẑ₀, seed e_q; 2N … 3N−1: a; 3N … 4N−1: ω; 4N: G; beyond: a pad lane — in a group of 8
// (N = 1) or 16 (N = 2, 3) lanes. A lane carries u = [x (N), y (N), vx (N), vy (N)] with v = ∂z/∂q_q, and the right-hand side on it is
//   dz = f(z),   dv = J(z)·v + ∂f/∂q_q.
// Mean-field form, like the Kuramoto system's: with c_j = a_j − r_j², r_j² = x_j² + y_j², x̄ = (1/N) Σ x_i, ȳ = (1/N) Σ y_i
//   dx_j = c_j x_j − ω_j y_j + G (x̄ − x_j),   dy_j = c_j y_j + ω_j x_j + G (ȳ − y_j),
// and J·v without forming J: with s_j = x_j vx_j + y_j vy_j (∂(r_j²)/2 along v) and v̄x, v̄y the means of the tangent,
//   dvx_j = c_j vx_j − 2 x_j s_j − ω_j vy_j + G (v̄x − vx_j),   dvy_j = c_j vy_j − 2 y_j s_j + ω_j vx_j + G (v̄y − vy_j)
// (the diagonal's a_j − r_j² − 2x_j² − G(1 − 1/N) and the G/N off it are in there). The forcing column — ∂f/∂a_j = (x_j, y_j) and
// ∂f/∂ω_j = (−y_j, x_j) on oscillator j, ∂f/∂G = (x̄ − x, ȳ − y) — enters through per-lane constants: wa[j] is 1 on the lane of a_j, wo[j] on
// the lane of ω_j, wg on the lane of G, 0 elsewhere; a ẑ₀-lane and a pad lane have all of them 0, so no lane branches. Polynomial: no
// transcendental function, no angle — anchor is empty. Plain f32, as KuramotoDir.
#pragma once
#include "lde_device.h"
#include "lde_host.h"

namespace lde {

template <int N>
struct StuartLandauDir {
  static_assert(N >= lde_host::SL_MIN_N && N <= lde_host::SL_MAX_N, "one to three oscillators");
  static constexpr int D = 2 * N;        // components: x₁ … x_N, y₁ … y_N
  static constexpr int NP = 4 * N + 1;   // partial directions: ẑ₀ (2N), a (N), ω (N), G
  static constexpr int G = lde_host::dir_group_width(LDE_RHS_STUART_LANDAU, D);   // lanes of a trajectory: 8 for N = 1, 16 for N = 2, 3
  static constexpr int DN = 2 * D;       // floats of a lane's state: the 2N values and its one tangent column
  float a[N], om[N];   // a_j, ω_j
  float g;             // G
  float wa[N], wo[N];  // 1 on the lane of a_j / of ω_j, 0 elsewhere
  float wg;            // 1 on the lane of G, 0 elsewhere

  // θ of trajectory b: (a₁ … a_N, ω₁ … ω_N, G); q: the lane's direction
  static __device__ __forceinline__ StuartLandauDir load(const float* __restrict__ theta, long long b, int q) {
    StuartLandauDir f;
    const float* th = theta + (size_t)(2 * N + 1) * b;
#pragma unroll
    for (int j = 0; j < N; j++) {
      f.a[j] = th[j];
      f.om[j] = th[N + j];
      f.wa[j] = q == 2 * N + j ? 1.f : 0.f;
      f.wo[j] = q == 3 * N + j ? 1.f : 0.f;
    }
    f.g = th[2 * N];
    f.wg = q == 4 * N ? 1.f : 0.f;
    return f;
  }
  // seeds: ∂z(t₀)/∂ẑ₀ = I — lane q < 2N starts with e_q — and ∂/∂θ = 0; a pad lane starts (and stays) at zero
  static __device__ __forceinline__ void seed(const float* __restrict__ z0, long long b, int q, float (&y)[DN]) {
#pragma unroll
    for (int i = 0; i < D; i++) {
      y[i] = z0[(size_t)D * b + i];
      y[D + i] = q == i ? 1.f : 0.f;
    }
  }
  __device__ __forceinline__ void anchor(const float (&)[DN]) {}   // no angle: nothing to anchor
  __device__ __forceinline__ void operator()(const float (&u)[DN], float (&du)[DN]) const {
    float xs = 0.f, ys = 0.f, vxs = 0.f, vys = 0.f;
#pragma unroll
    for (int j = 0; j < N; j++) {
      xs += u[j];
      ys += u[N + j];
      vxs += u[D + j];
      vys += u[D + N + j];
    }
    const float xm = xs * (1.0f / N), ym = ys * (1.0f / N), vxm = vxs * (1.0f / N), vym = vys * (1.0f / N);
#pragma unroll
    for (int j = 0; j < N; j++) {
      const float x = u[j], y = u[N + j], vx = u[D + j], vy = u[D + N + j];
      const float c = a[j] - (x * x + y * y);
      const float dxm = xm - x, dym = ym - y;
      du[j] = c * x - om[j] * y + g * dxm;
      du[N + j] = c * y + om[j] * x + g * dym;
      const float s2 = 2.0f * (x * vx + y * vy);
      du[D + j] = c * vx - s2 * x - om[j] * vy + g * (vxm - vx) + (wa[j] * x - wo[j] * y + wg * dxm);
      du[D + N + j] = c * vy - s2 * y + om[j] * vx + g * (vym - vy) + (wa[j] * y + wo[j] * x + wg * dym);
    }
  }
};

}  // namespace lde
