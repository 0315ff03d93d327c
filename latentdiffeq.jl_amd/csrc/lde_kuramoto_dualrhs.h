// lde_kuramoto_dualrhs.h — the Kuramoto system (LDE_RHS_KURAMOTO: dφ_i = ω_i + (K/N) Σ_j sin(φ_j − φ_i), N phase oscillators, θ = (ω₁ … ω_N, K))
// as ONE LANE of the lane-per-direction dual solve sees it (csrc/lde_dual_dir.hip): the lane of partial direction q — q = 0 … N−1: φ₀,
// N … 2N−1: ω, 2N: K, beyond: a pad lane — carries u = [φ (N), v (N)] with v = ∂φ/∂q_q, and the right-hand side on it is
//   dφ = f(φ),   dv = J(φ)·v + ∂f/∂q_q.
// Mean-field form: s_i = sin φ_i, c_i = cos φ_i, S = Σ s_j, C = Σ c_j give f_i = ω_i + (K/N)(c_i S − s_i C) with N sine / cosine pairs, not
// N². The Jacobian in the same terms — ∂f_i/∂φ_j = (K/N)(c_i c_j + s_i s_j) for j ≠ i, ∂f_i/∂φ_i = −(K/N)(c_i C + s_i S − 1) — applied to v
// without forming it: with A = Σ c_j v_j and D = Σ s_j v_j, (J·v)_i = (K/N)(c_i A + s_i D − (c_i C + s_i S) v_i) (the j = i term of the
// sums, (c_i² + s_i²) v_i, is the "− 1" of the diagonal). The forcing column: δ_i,q−N on an ω-lane, (c_i S − s_i C)/N on the K-lane, nothing
// on a φ₀-lane or a pad lane — as two per-lane constants, so that no lane branches.
#pragma once
#include "lde_device.h"
#include "lde_host.h"

namespace lde {

template <int N>
struct KuramotoDir {
  static constexpr int D = N;            // components
  static constexpr int NP = 2 * N + 1;   // partial directions: φ₀ (N), ω (N), K
  static constexpr int G = lde_host::dir_group_width(N);   // lanes of a trajectory: 8 for N ≤ 3, 16 for N ≤ 7
  static constexpr int DN = 2 * N;       // floats of a lane's state: the N values and its one tangent column
  float om[N];     // ω
  float kn;        // K/N
  float wk;        // 1/N on the K-lane (q = 2N), 0 elsewhere: the weight of the K-column in this lane's forcing
  int qom;         // q − N: the oscillator whose ω this lane differentiates by (outside 0 … N−1: none)
  float noff[N];   // −(whole turns of each oscillator's phase at the step's start): turn_anchor (lde_device.h)

  // θ of trajectory b: (ω₁ … ω_N, K); q: the lane's direction
  static __device__ __forceinline__ KuramotoDir load(const float* __restrict__ theta, long long b, int q) {
    KuramotoDir f;
    const float* th = theta + (size_t)(N + 1) * b;
#pragma unroll
    for (int i = 0; i < N; i++) {
      f.om[i] = th[i];
      f.noff[i] = 0.f;
    }
    f.kn = th[N] * (1.0f / N);
    f.wk = q == 2 * N ? 1.0f / N : 0.f;
    f.qom = q - N;
    return f;
  }
  // seeds: ∂φ(t₀)/∂φ₀ = I — lane q < N starts with e_q — and ∂/∂θ = 0; a pad lane starts (and stays) at zero
  static __device__ __forceinline__ void seed(const float* __restrict__ z0, long long b, int q, float (&y)[DN]) {
#pragma unroll
    for (int i = 0; i < N; i++) {
      y[i] = z0[(size_t)N * b + i];
      y[N + i] = q == i ? 1.f : 0.f;
    }
  }
  // The hardware sine is defined up to 256 turns (lde_device.h): every oscillator's whole turns are anchored once per step attempt, as the
  // pendulum anchors its one angle — a phase that has run past 256 turns keeps its coupling.
  __device__ __forceinline__ void anchor(const float (&y)[DN]) {
#pragma unroll
    for (int i = 0; i < N; i++) noff[i] = turn_anchor(y[i]);
  }
  __device__ __forceinline__ void operator()(const float (&u)[DN], float (&du)[DN]) const {
    float s[N], c[N];
    float S = 0.f, C = 0.f, A = 0.f, D = 0.f;
#pragma unroll
    for (int i = 0; i < N; i++) {
      hw_sincos(u[i], s[i], c[i], noff[i]);
      S += s[i];
      C += c[i];
      A += c[i] * u[N + i];
      D += s[i] * u[N + i];
    }
#pragma unroll
    for (int i = 0; i < N; i++) {
      const float g = c[i] * S - s[i] * C;   // Σ_j sin(φ_j − φ_i)
      du[i] = om[i] + kn * g;
      const float jv = c[i] * A + s[i] * D - (c[i] * C + s[i] * S) * u[N + i];
      du[N + i] = kn * jv + wk * g + (qom == i ? 1.f : 0.f);
    }
  }
};

}  // namespace lde
