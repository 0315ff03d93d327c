// lde_dual.hip — LDE_SENSE_FORWARD_DUAL: ForwardDiffSensitivity as the reference executes it during training, on the GOKU path.
//
// `Pendulum()` carries ForwardDiffSensitivity() [REF examples/pendulum_friction-less/pendulum.jl:8-11], splatted into solve() at
// [REF src/models/GOKU.jl:107, :121]: upstream seeds (u0, p) with dual partials and runs the SAME OrdinaryDiffEq solve on Dual numbers, and
// its error norm (ODE_DEFAULT_NORM on a Dual = sqrt(value² + Σ partials²)) sees the partials — the accepted steps of a training solve are not
// the primal solve's. LDE_SENSE_DISCRETE differentiates the primal sequence; this mode reproduces the dual one. The specification is the
// checkers' dual solve, step for step: oracle/ (dual_solve with dual_norm = 1) for the pendulums, tests/lv_ref.py for Lotka–Volterra.
//
// k_forward_dual<SYS>: ONE kernel for every deterministic two-state system — a lane per trajectory, the dual state [u₀, u₁, ∂u₀/∂q (NP),
// ∂u₁/∂q (NP)] and Tsit5's seven slopes of it in registers. The system is a struct (csrc/lde_pend_dualrhs.h: the pendulums, NP = 3,
// q = (x₀, v₀, L), every stage's sin x and cos x from ONE hw_sincos on the step's turn anchor; csrc/lde_lv_dualrhs.h: Lotka–Volterra, NP = 6,
// q = (x₀, y₀, α, β, γ, δ), polynomial, no anchor) that gives NP, its θ of a trajectory, the seeded state, the anchor and the right-hand side.
// The stage sums, the solution weights and the interpolant are lde_device.h's (tsit5_attempt / rk4_step / tsit5_dense_* on a DN-vector); what
// decides the steps and what a lane does around its stepper is csrc/lde_dual.h's, shared with the stochastic pendulum's kernel.
// ẑ goes to z_out [T×B×2] as lde_forward's other kernels write it; J_j = ∂ẑ(t_j)/∂q to the dual record, trajectory fastest (lde_types.h:
// DualRec), so that a wave's 64 lanes write — and the pullback's read — 256 consecutive bytes.
// k_adjoint_dual<NP>: dz0 = Σ_j J_j[:, 0:2]ᵀ dz_out_j, dθ = Σ_j J_j[:, 2:NP]ᵀ dz_out_j, summed j outer, i inner in f32 (the checkers' order).
#include "lde_device.h"
#include "lde_dual.h"
#include "lde_host.h"
#include "lde_lv_dualrhs.h"
#include "lde_pend_dualrhs.h"

namespace lde {

template <class SYS, int SOLVER, bool TS_LDS>
__global__ void __launch_bounds__(256) k_forward_dual(const float2* __restrict__ z0, const float* __restrict__ theta,
                                                      const double* __restrict__ ts_g, KOpts o, DualRec rec,
                                                      float2* __restrict__ z_out, int32_t* __restrict__ retcode,
                                                      int32_t* __restrict__ st_nfe, int32_t* __restrict__ st_nacc,
                                                      int32_t* __restrict__ st_nrej, int32_t* __restrict__ st_ret) {
  constexpr int NP = SYS::NP, DN = 2 + 2 * NP;
  const int T = o.T, B = o.B;
  dual_stage_ts<TS_LDS>(ts_g, T);
  auto s_ts = [&](int i) -> double { return dual_ts<TS_LDS>(ts_g, i); };
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;

  const float2 zi = z0[b];
  SYS f = SYS::load(theta, b);
  float y[DN];
  SYS::seed(zi.x, zi.y, y);
  float k[7][DN], yn[DN];
  dual_save<NP>(z_out, rec, 0, B, b, y);   // ts[0] is saved as ẑ₀ itself
  int ret = LDE_RET_SUCCESS, nfe = 0, nacc = 0, nrej = 0;

  if (T > 1) {
    double t = o.t_first;
    const double tend = o.t_last, dtmax = tend - t;
    f.anchor(y[0]);
    f(y, k[0]);
    nfe = 1;
    double dt;
    if (!o.adaptive) dt = o.dt_fixed;
    else if (o.dt_fixed > 0) dt = fmin(o.dt_fixed, dtmax);
    else {
      dt = dual_init_dt<NP>(f, y, k[0], dtmax, o);
      nfe++;
    }
    float qold = 1e-4f;
    long long iters = 0;
    int j = 1;
    double tj = s_ts(1), tjn = s_ts(min(2, T - 1));
    while (t < tend) {
      if (iters++ >= o.maxiters) { ret = LDE_RET_MAXITERS; break; }
      double dtp = dt;
      bool last = false;
      if (t + dt >= tend - 1e-12 * fmax(fabs(tend), dtmax)) { dt = tend - t; last = true; }
      const float h = (float)dt;
      float EEst = 0.f;
      f.anchor(y[0]);
      if (SOLVER == LDE_SOLVER_TSIT5) {
        tsit5_attempt<DN, SYS, false, 0>(f, h, y, k, yn, o);
        if (o.adaptive) EEst = dual_eest<NP>(h, y, yn, k, o);
        nfe += 6;
      } else {
        rk4_step<DN>(f, h, y, k, yn);
        nfe += 4;
      }
      if (!all_finite<DN>(yn) || !(EEst == EEst)) {
        if (o.adaptive && dt > o.dtmin) { nrej++; dt = dt * (double)o.qmin; continue; }
        ret = LDE_RET_NONFINITE;
        break;
      }
      if (o.adaptive) {
        float q11;
        const float q = pi_q(EEst, qold, o, q11);
        if (EEst > 1.0f) {
          nrej++;
          dt = dt * (double)fast_rcp(fminf(o.q_hi, q11 * o.inv_gamma));
          if (dt < o.dtmin) { ret = LDE_RET_DTMIN; break; }
          continue;
        }
        qold = fmaxf(EEst, 1e-4f);
        dtp = dt * (double)fast_rcp(q);
        if (dtp > dtmax) dtp = dtmax;
      }
      if (rec.t && nacc < rec.cap) {   // option "step_trace": the accepted step's start time and size
        rec.t[(size_t)nacc * B + b] = t;
        rec.dt[(size_t)nacc * B + b] = dt;
      }
      nacc++;
      const double tnew = last ? tend : t + dt;
      if (j < T && tj <= tnew) {   // at least one save time in (t, tnew]
        float P[3][DN];
        if (SOLVER == LDE_SOLVER_TSIT5) tsit5_dense_coeffs<DN>(k, P);
        do {
          float u[DN];
          if (tj >= tnew || (j == T - 1 && last)) {
#pragma unroll
            for (int c = 0; c < DN; c++) u[c] = yn[c];
          } else {
            const double thd = (tj - t) / dt;
            if (SOLVER == LDE_SOLVER_TSIT5) {
              const float th = (float)thd;
#pragma unroll
              for (int c = 0; c < DN; c++) u[c] = tsit5_dense_eval<DN>(th, h, y[c], k[0][c], P[0][c], P[1][c], P[2][c]);
            } else {   // cubic Hermite between (y, k₁) and (y_new, f(y_new)), coefficients in f64 as the checkers form them
              const double om = 1.0 - thd;
              const float h00 = (float)((1.0 + 2.0 * thd) * om * om), h10 = (float)(thd * om * om * dt);
              const float h01 = (float)(thd * thd * (3.0 - 2.0 * thd)), h11 = (float)(thd * thd * (thd - 1.0) * dt);
#pragma unroll
              for (int c = 0; c < DN; c++) u[c] = h00 * y[c] + h10 * k[0][c] + h01 * yn[c] + h11 * k[4][c];
            }
          }
          dual_save<NP>(z_out, rec, j, B, b, u);
          j++;
          tj = tjn;
          tjn = s_ts(min(j + 1, T - 1));
        } while (j < T && tj <= tnew);
      }
#pragma unroll
      for (int c = 0; c < DN; c++) y[c] = yn[c];
      constexpr int FS = (SOLVER == LDE_SOLVER_TSIT5) ? 6 : 4;   // FSAL slope
#pragma unroll
      for (int c = 0; c < DN; c++) k[0][c] = k[FS][c];
      t = tnew;
      dt = o.adaptive ? dtp : o.dt_fixed;
    }
  }
  if (ret != LDE_RET_SUCCESS) dual_fill_failed<NP>(z_out, rec, T, B, b);
  dual_finish(b, ret, nfe, nacc, nrej, rec, retcode, st_nfe, st_nacc, st_nrej, st_ret);
}

// g_q = Σ_j (J_j[0][q]·dz_out_j.x + J_j[1][q]·dz_out_j.y): per accumulator first the d.x term, then the d.y term, of each j
template <int NP>
__global__ void __launch_bounds__(256) k_adjoint_dual(DualRec rec, const float2* __restrict__ dz_out, int T, int B,
                                                      float2* __restrict__ dz0, float* __restrict__ dtheta,
                                                      int32_t* __restrict__ st_nfe, int32_t* __restrict__ st_nacc,
                                                      int32_t* __restrict__ st_nrej, int32_t* __restrict__ st_ret) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const int n = rec.n[b];
  float g[NP];
#pragma unroll
  for (int q = 0; q < NP; q++) g[q] = 0.f;
  if (n >= 0) {   // (a failed trajectory's gradient is zero whatever its cotangent holds: a NaN ẑ block usually brings a NaN one)
    const float* Jb = rec.J + b;
    for (int j = 0; j < T; j++) {
      const float2 d = dz_out[(size_t)j * B + b];
      const float* Jj = Jb + (size_t)j * (2 * NP) * B;
#pragma unroll
      for (int q = 0; q < NP; q++) g[q] += Jj[(size_t)q * B] * d.x;
#pragma unroll
      for (int q = 0; q < NP; q++) g[q] += Jj[(size_t)(NP + q) * B] * d.y;
    }
  }
  dz0[b] = make_float2(g[0], g[1]);
#pragma unroll
  for (int p = 0; p < NP - 2; p++) dtheta[(size_t)(NP - 2) * b + p] = g[2 + p];
  st_nfe[b] = 0;
  st_nacc[b] = 0;
  st_nrej[b] = 0;
  st_ret[b] = n < 0 ? -n : LDE_RET_SUCCESS;
}

// ---- host-side launchers (called from lde_api.hip) -------------------------------------------------------------------------------
template <class SYS>
struct sys_of {   // a system's type as a value: what the two dispatches hand to the one launch lambda
  using type = SYS;
};

int launch_forward_dual(int kind, int solver, const float* z0, const float* theta, const double* ts_dev, const KOpts& o, const DualRec& rec,
                        float* z_out, int32_t* retcode, int32_t* nfe, int32_t* nacc, int32_t* nrej, int32_t* ret, hipStream_t stream) {
  const int block = dual_block(o.B), grid = (o.B + block - 1) / block;
  const size_t shm = o.T <= DUAL_TS_LDS_MAX ? (size_t)o.T * sizeof(double) : 0;
  auto launch = [&](auto sys, auto S) -> int {
    using SYS = typename decltype(sys)::type;
    if (shm)
      hipLaunchKernelGGL((k_forward_dual<SYS, S, true>), dim3(grid), dim3(block), shm, stream, (const float2*)z0, theta, ts_dev, o, rec,
                         (float2*)z_out, retcode, nfe, nacc, nrej, ret);
    else
      hipLaunchKernelGGL((k_forward_dual<SYS, S, false>), dim3(grid), dim3(block), 0, stream, (const float2*)z0, theta, ts_dev, o, rec,
                         (float2*)z_out, retcode, nfe, nacc, nrej, ret);
    return LDE_OK;
  };
  const int rc = kind == LDE_RHS_LOTKA_VOLTERRA
                     ? lde_host::lv_dispatch(solver, o.adaptive != 0, [&](auto S) -> int { return launch(sys_of<LvDual>{}, S); })
                     : lde_host::pend_dispatch(kind, solver, o.adaptive != 0,
                                               [&](auto K, auto S, auto) -> int { return launch(sys_of<PendDual<K>>{}, S); });
  return rc != LDE_OK ? rc : hipGetLastError() == hipSuccess ? LDE_OK : LDE_ERR_HIP;
}

int launch_adjoint_dual(int kind, const DualRec& rec, const float* dz_out, int T, int B, float* dz0, float* dtheta, int32_t* nfe,
                        int32_t* nacc, int32_t* nrej, int32_t* ret, hipStream_t stream) {
  const int block = dual_block(B), grid = (B + block - 1) / block;
  auto launch = [&](auto NP) -> int {
    hipLaunchKernelGGL(k_adjoint_dual<NP>, dim3(grid), dim3(block), 0, stream, rec, (const float2*)dz_out, T, B, (float2*)dz0, dtheta, nfe,
                       nacc, nrej, ret);
    return hipGetLastError() == hipSuccess ? LDE_OK : LDE_ERR_HIP;
  };
  // (the stochastic pendulum's record is a pendulum's: csrc/lde_pend_sde.hip)
  return kind == LDE_RHS_LOTKA_VOLTERRA ? launch(std::integral_constant<int, LvDual::NP>{}) : launch(std::integral_constant<int, PendDual<0>::NP>{});
}

}  // namespace lde
