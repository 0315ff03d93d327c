// lde_pend_sde.hip — LDE_RHS_SPENDULUM: the reference's `SPendulum` plug-in [REF examples/pendulum_friction-less/pendulum.jl:93-140] on the
// GOKU path, dx = v dt + σ dW₁, dv = −(G/L) sin x dt + σ dW₂ with σ = 0.01 on both components (additive: Itô = Stratonovich).
//
// Two fixed-step schemes of StochasticDiffEq — EM() and EulerHeun() — in f32; the reference's default SOSRI() (adaptive, rejection sampling
// with memory) is NOT reproduced (include/lde.h: "the stochastic pendulum" states the deviation and the substep rule). The noise of
// (trajectory, substep) is ONE Philox4x32-10 block keyed by the caller's seed (csrc/lde_philox.h: lde_randn's device code) — a pure function
// of its counter, so the launch geometry, a shard's place in the batch and a graph replay do not enter it.
//
// k_pend_forward_sde: a lane per trajectory, its own stepper inside the dual solve's frame — the state and its six partials ∂(x, v)/∂(x₀, v₀, L)
// in registers (the noise has zero partials: the gradient is the exact derivative of the scheme along the drawn path, the reference's
// ForwardDiffSensitivity() at a fixed step), one hw_sincos on the step's turn anchor per evaluation, one Philox block and one Box–Muller pair
// per substep; per save interval n_j, h_j and σ·√h are formed once. What surrounds the stepper is csrc/lde_dual.h's, as in k_forward_dual:
// `ts` in LDS where it fits, the (ẑ_j, J_j) rows trajectory fastest (a wave stores whole lines), the failed solve's fill, the closing
// statistics, the workgroup size; the system is csrc/lde_pend_dualrhs.h's PendDual. The pullback is k_adjoint_dual<3> (csrc/lde_dual.hip) on
// the dual record this kernel leaves. Per trajectory: 12 B read, 8·T + 24·T B written.
#include "lde_device.h"
#include "lde_host.h"
#include "lde_pend_dualrhs.h"
#include "lde_philox.h"

namespace lde {

// `over`: the host's substep plan (lde_host::sde_plan) is longer than maxiters — every trajectory fails with LDE_RET_MAXITERS, nothing is stepped
template <int SOLVER, bool TS_LDS>
__global__ void __launch_bounds__(256) k_pend_forward_sde(const float2* __restrict__ z0, const float* __restrict__ theta,
                                                          const double* __restrict__ ts_g, KOpts o, DualRec rec, SdeNoise nz, int over,
                                                          float2* __restrict__ z_out, int32_t* __restrict__ retcode,
                                                          int32_t* __restrict__ st_nfe, int32_t* __restrict__ st_nacc,
                                                          int32_t* __restrict__ st_nrej, int32_t* __restrict__ st_ret) {
  using SYS = PendDual<LDE_RHS_PENDULUM>;
  constexpr int NP = SYS::NP, DN = SYS::DN;
  const int T = o.T, B = o.B;
  dual_stage_ts<TS_LDS>(ts_g, T);
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;

  SYS f = SYS::load(theta, b);
  float y[DN];
  const float2 zi = z0[b];
  SYS::seed(zi.x, zi.y, y);
  dual_save<NP>(z_out, rec, 0, B, b, y);   // ẑ(ts[0]) = ẑ₀
  int ret = over ? LDE_RET_MAXITERS : LDE_RET_SUCCESS;
  long long nsub = 0;

  if (!over && T > 1) {
    // the counter's words that do not change along the solve
    const unsigned long long off = nz.offset + (nz.epoch_dev ? (unsigned long long)*nz.epoch_dev : 0ull);
    const unsigned c_traj = (unsigned)(nz.first_trajectory + (unsigned long long)b), c_lo = (unsigned)off, c_hi = (unsigned)(off >> 32);
    const unsigned k_lo = (unsigned)nz.seed, k_hi = (unsigned)(nz.seed >> 32);
    unsigned s = 0;   // the substep index of the whole solve: the counter's second word
    double tprev = o.t_first;
    for (int j = 1; j < T; j++) {
      const double tj = dual_ts<TS_LDS>(ts_g, j), D = tj - tprev;
      const int n = sde_substeps(D, o.dt_fixed);
      const double hd = D / (double)n;
      const float h = (float)hd, hh = 0.5f * h, sw = 0.01f * sqrtf(h);
      for (int i = 0; i < n; i++, s++) {
        unsigned w[4];
        philox4x32_10(c_traj, s, c_lo, c_hi, k_lo, k_hi, w);
        float xi_x, xi_v;
        box_muller_pair(w[0], w[1], xi_x, xi_v);
        const float dwx = sw * xi_x, dwv = sw * xi_v;
        float k0[DN];
        f.anchor(y[0]);
        f(y, k0);
        if (SOLVER == LDE_SOLVER_EM) {
#pragma unroll
          for (int c = 0; c < DN; c++) y[c] += h * k0[c];
        } else {
          float yb[DN], k1[DN];
#pragma unroll
          for (int c = 0; c < DN; c++) yb[c] = y[c] + h * k0[c];
          yb[0] += dwx;
          yb[1] += dwv;
          f(yb, k1);
#pragma unroll
          for (int c = 0; c < DN; c++) y[c] += hh * (k0[c] + k1[c]);
        }
        y[0] += dwx;
        y[1] += dwv;
        if (rec.t && nsub + i < rec.cap) {   // option "step_trace": the substep's start time and size
          rec.t[(size_t)(nsub + i) * B + b] = tprev + (double)i * hd;
          rec.dt[(size_t)(nsub + i) * B + b] = hd;
        }
      }
      nsub += n;
      // (a non-finite value never becomes finite again under y ← y + …: one look per save interval sees it)
      if (!all_finite<DN>(y)) { ret = LDE_RET_NONFINITE; break; }
      dual_save<NP>(z_out, rec, j, B, b, y);
      tprev = tj;
    }
  }
  if (ret != LDE_RET_SUCCESS) dual_fill_failed<NP>(z_out, rec, T, B, b);
  constexpr int NFE = SOLVER == LDE_SOLVER_EM ? 1 : 2;
  const int nacc = (int)(nsub < 0x3fffffffLL ? nsub : 0x3fffffffLL);   // (int32 statistics: a longer solve saturates)
  dual_finish(b, ret, NFE * nacc, nacc, 0, rec, retcode, st_nfe, st_nacc, st_nrej, st_ret);
}

// ---- host-side launcher (called from lde_api.hip) ------------------------------------------------------------------------------------
// The stochastic right-hand side has a dispatch of its own (lde_host::pend_dispatch serves the deterministic pendulums' six combinations and
// nothing else): the two solvers lde_host::validate admits for it.
int launch_pend_forward_sde(int solver, const float* z0, const float* theta, const double* ts_dev, const KOpts& o, const DualRec& rec,
                            const SdeNoise& nz, bool over, float* z_out, int32_t* retcode, int32_t* nfe, int32_t* nacc, int32_t* nrej,
                            int32_t* ret, hipStream_t stream) {
  const int block = dual_block(o.B), grid = (o.B + block - 1) / block;
  const size_t shm = o.T <= DUAL_TS_LDS_MAX ? (size_t)o.T * sizeof(double) : 0;
  auto launch = [&](auto S) -> int {
    if (shm)
      hipLaunchKernelGGL((k_pend_forward_sde<S, true>), dim3(grid), dim3(block), shm, stream, (const float2*)z0, theta, ts_dev, o, rec, nz,
                         (int)over, (float2*)z_out, retcode, nfe, nacc, nrej, ret);
    else
      hipLaunchKernelGGL((k_pend_forward_sde<S, false>), dim3(grid), dim3(block), 0, stream, (const float2*)z0, theta, ts_dev, o, rec, nz,
                         (int)over, (float2*)z_out, retcode, nfe, nacc, nrej, ret);
    return hipGetLastError() == hipSuccess ? LDE_OK : LDE_ERR_HIP;
  };
  if (solver == LDE_SOLVER_EM) return launch(std::integral_constant<int, LDE_SOLVER_EM>{});
  if (solver == LDE_SOLVER_EULER_HEUN) return launch(std::integral_constant<int, LDE_SOLVER_EULER_HEUN>{});
  return LDE_ERR_UNSUPPORTED;
}

}  // namespace lde
