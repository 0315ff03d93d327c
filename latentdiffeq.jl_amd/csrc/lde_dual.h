// lde_dual.h — what the kernels that carry a dual state through a solve (LDE_SENSE_FORWARD_DUAL) share, over "a two-state system with NP
// partials per component": k_forward_dual (csrc/lde_dual.hip; the pendulums at NP = 3: x₀, v₀, L; Lotka–Volterra at NP = 6: x₀, y₀, α, β,
// γ, δ) and k_pend_forward_sde (csrc/lde_pend_sde.hip, NP = 3). A dual state is 2 + 2·NP floats: [u₀, u₁, ∂u₀/∂q (NP), ∂u₁/∂q (NP)].
//   * the step control — the dual norms, their squares, the RMS (accumulated in f64 as the checkers do) and the Hairer initial step, in the
//     checkers' order of operations (oracle/: dual_solve; tests/lv_ref.py);
//   * a lane's pieces around its stepper — the save grid in LDS, one (ẑ_j, J_j) row of the dual record (lde_types.h: DualRec), the failed
//     solve's fill, the closing statistics — and the workgroup size of a batch.
#pragma once
#include "lde_device.h"
#include "lde_host.h"

namespace lde {

constexpr int DUAL_TS_LDS_MAX = 6000;   // doubles of the save-time grid kept in LDS (48 KB)

// Workgroups by the dual solve's batch rule (lde_host::pend_dual_mapping): a wave each up to 4 096 trajectories, four waves beyond.
static int dual_block(int B) { return lde_host::pend_dual_mapping(B) == lde_host::PEND_DUAL_LANE64 ? 64 : 256; }

// The save grid of a launch: staged in LDS by the whole workgroup where it fits (TS_LDS: the launch brings T doubles of dynamic LDS), read
// from global memory otherwise. dual_stage_ts is called by every lane, before the lanes past the batch leave.
extern __shared__ __attribute__((aligned(16))) double s_ts_dual[];
template <bool TS_LDS>
__device__ __forceinline__ void dual_stage_ts(const double* ts_g, int T) {
  if (TS_LDS)
    for (int i = threadIdx.x; i < T; i += blockDim.x) s_ts_dual[i] = ts_g[i];
  __syncthreads();
}
template <bool TS_LDS>
__device__ __forceinline__ double dual_ts(const double* ts_g, int i) { return TS_LDS ? s_ts_dual[i] : ts_g[i]; }

// ẑ_j and J_j of trajectory b: ẑ to z_out [T×B×2], the 2·NP partials to the dual record, a row of B floats each (trajectory fastest)
template <int NP>
__device__ __forceinline__ void dual_save(float2* z_out, const DualRec& rec, int j, int B, int b, const float (&u)[2 + 2 * NP]) {
  z_out[(size_t)j * B + b] = make_float2(u[0], u[1]);
  float* Jj = rec.J + (size_t)j * (2 * NP) * B + b;
#pragma unroll
  for (int c = 0; c < 2 * NP; c++) Jj[(size_t)c * B] = u[2 + c];
}

// failed solve ⇒ NaN block and zero Jacobians (zero gradient) [REF GOKU.jl:114]
template <int NP>
__device__ __forceinline__ void dual_fill_failed(float2* z_out, const DualRec& rec, int T, int B, int b) {
  const float qn = __int_as_float(0x7fc00000);
  for (int j = 0; j < T; j++) {
    z_out[(size_t)j * B + b] = make_float2(qn, qn);
    float* Jj = rec.J + (size_t)j * (2 * NP) * B + b;
#pragma unroll
    for (int c = 0; c < 2 * NP; c++) Jj[(size_t)c * B] = 0.f;
  }
}

// a trajectory's return code, its statistics and its entry of the dual record: the accepted steps, or −retcode for the pullback to see
__device__ __forceinline__ void dual_finish(int b, int ret, int nfe, int nacc, int nrej, const DualRec& rec, int32_t* retcode, int32_t* st_nfe,
                                            int32_t* st_nacc, int32_t* st_nrej, int32_t* st_ret) {
  if (retcode) retcode[b] = ret;
  st_ret[b] = ret;
  st_nfe[b] = nfe;
  st_nacc[b] = nacc;
  st_nrej[b] = nrej;
  rec.n[b] = ret == LDE_RET_SUCCESS ? nacc : -ret;
}

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
