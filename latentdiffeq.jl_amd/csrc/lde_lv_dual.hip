// lde_lv_dual.hip — LDE_RHS_LOTKA_VOLTERRA on the GOKU path: dx = αx − βxy, dy = −γy + δxy with θ = (α, β, γ, δ) per trajectory, served by
// LDE_SENSE_FORWARD_DUAL — the solve on dual numbers, as the reference executes ForwardDiffSensitivity() during training
// [REF src/models/GOKU.jl:107, :121] — and by nothing else (include/lde.h: "the Lotka–Volterra system").
//
// k_lv_forward_dual: k_pend_forward_dual (csrc/lde_pend_dual.hip) line for line with NP = 6 partials per component instead of 3 — a lane per
// trajectory, the dual state [x, y, ∂x/∂q (6), ∂y/∂q (6)], q ∈ (x₀, y₀, α, β, γ, δ), and Tsit5's seven slopes of it in registers; the stage
// sums, the solution weights and the interpolant are lde_device.h's on a 14-vector, the step control is csrc/lde_dual.h's with all six
// partials in every norm; the right-hand side is polynomial (csrc/lde_lv_dualrhs.h). ẑ goes to z_out [T×B×2], J_j = ∂ẑ(t_j)/∂q to the dual
// record as J [T][2][6][B], trajectory fastest: a wave stores whole lines.
// k_lv_adjoint_dual: dz0 = Σ_j J_j[:, 0:2]ᵀ dz_out_j, dθ = Σ_j J_j[:, 2:6]ᵀ dz_out_j, summed j outer, i inner in f32 (tests/lv_ref.py's order).
// The checker is tests/lv_ref.py (numpy, f64 and f32), compared in tests/test_gpu_lv.py.
#include "lde_device.h"
#include "lde_dual.h"
#include "lde_host.h"
#include "lde_lv_dualrhs.h"

namespace lde {

template <int SOLVER, bool TS_LDS>
__global__ void __launch_bounds__(256) k_lv_forward_dual(const float2* __restrict__ z0, const float* __restrict__ theta,
                                                         const double* __restrict__ ts_g, KOpts o, DualRec rec,
                                                         float2* __restrict__ z_out, int32_t* __restrict__ retcode,
                                                         int32_t* __restrict__ st_nfe, int32_t* __restrict__ st_nacc,
                                                         int32_t* __restrict__ st_nrej, int32_t* __restrict__ st_ret) {
  constexpr int NP = LV_NP, DN = LV_DN;
  extern __shared__ __attribute__((aligned(16))) double s_ts_lv[];
  const int T = o.T, B = o.B;
  if (TS_LDS)
    for (int i = threadIdx.x; i < T; i += blockDim.x) s_ts_lv[i] = ts_g[i];
  __syncthreads();
  auto s_ts = [&](int i) -> double { return TS_LDS ? s_ts_lv[i] : ts_g[i]; };
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;

  // J_j of this trajectory: 2·NP rows of B floats per save time
  auto save = [&](int j, const float (&u)[DN]) {
    z_out[(size_t)j * B + b] = make_float2(u[0], u[1]);
    float* Jj = rec.J + (size_t)j * (2 * NP) * B + b;
#pragma unroll
    for (int c = 0; c < 2 * NP; c++) Jj[(size_t)c * B] = u[2 + c];
  };

  const float2 zi = z0[b];
  const float* th4 = theta + (size_t)4 * b;   // (α, β, γ, δ) of this trajectory
  LvDual f(th4[0], th4[1], th4[2], th4[3]);
  float y[DN];   // seeds: ∂(x, y)/∂(x₀, y₀) = I, ∂/∂θ = 0
#pragma unroll
  for (int c = 0; c < DN; c++) y[c] = 0.f;
  y[0] = zi.x;
  y[1] = zi.y;
  y[2] = 1.f;
  y[2 + NP + 1] = 1.f;
  float k[7][DN], yn[DN];
  save(0, y);   // ts[0] is saved as ẑ₀ itself
  int ret = LDE_RET_SUCCESS, nfe = 0, nacc = 0, nrej = 0;

  if (T > 1) {
    double t = o.t_first;
    const double tend = o.t_last, dtmax = tend - t;
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
      if (t + dt >= tend - 1e-12 * fabs(tend)) { dt = tend - t; last = true; }
      const float h = (float)dt;
      float EEst = 0.f;
      if (SOLVER == LDE_SOLVER_TSIT5) {
        tsit5_attempt<DN, LvDual, false, 0>(f, h, y, k, yn, o);
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
            } else {   // cubic Hermite between (y, k₁) and (y_new, f(y_new)), coefficients in f64 as the checker forms them
              const double om = 1.0 - thd;
              const float h00 = (float)((1.0 + 2.0 * thd) * om * om), h10 = (float)(thd * om * om * dt);
              const float h01 = (float)(thd * thd * (3.0 - 2.0 * thd)), h11 = (float)(thd * thd * (thd - 1.0) * dt);
#pragma unroll
              for (int c = 0; c < DN; c++) u[c] = h00 * y[c] + h10 * k[0][c] + h01 * yn[c] + h11 * k[4][c];
            }
          }
          save(j, u);
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
  if (ret != LDE_RET_SUCCESS) {   // failed solve ⇒ NaN block and zero Jacobians (zero gradient) [REF GOKU.jl:114]
    const float qn = __int_as_float(0x7fc00000);
    for (int j = 0; j < T; j++) {
      z_out[(size_t)j * B + b] = make_float2(qn, qn);
      float* Jj = rec.J + (size_t)j * (2 * NP) * B + b;
#pragma unroll
      for (int c = 0; c < 2 * NP; c++) Jj[(size_t)c * B] = 0.f;
    }
  }
  if (retcode) retcode[b] = ret;
  st_ret[b] = ret;
  st_nfe[b] = nfe;
  st_nacc[b] = nacc;
  st_nrej[b] = nrej;
  rec.n[b] = ret == LDE_RET_SUCCESS ? nacc : -ret;
}

__global__ void __launch_bounds__(256) k_lv_adjoint_dual(DualRec rec, const float2* __restrict__ dz_out, int T, int B,
                                                         float2* __restrict__ dz0, float* __restrict__ dtheta,
                                                         int32_t* __restrict__ st_nfe, int32_t* __restrict__ st_nacc,
                                                         int32_t* __restrict__ st_nrej, int32_t* __restrict__ st_ret) {
  constexpr int NP = LV_NP;
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
  for (int p = 0; p < 4; p++) dtheta[(size_t)4 * b + p] = g[2 + p];
  st_nfe[b] = 0;
  st_nacc[b] = 0;
  st_nrej[b] = 0;
  st_ret[b] = n < 0 ? -n : LDE_RET_SUCCESS;
}

// ---- host-side launchers (called from lde_api.hip) -------------------------------------------------------------------------------
// Workgroups by the pendulum dual solve's batch rule (lde_host::pend_dual_mapping): a wave each up to 4 096 trajectories, four waves beyond.
static int lv_block(int B) { return lde_host::pend_dual_mapping(B) == lde_host::PEND_DUAL_LANE64 ? 64 : 256; }

int launch_lv_forward_dual(int solver, const float* z0, const float* theta, const double* ts_dev, const KOpts& o, const DualRec& rec,
                           float* z_out, int32_t* retcode, int32_t* nfe, int32_t* nacc, int32_t* nrej, int32_t* ret, hipStream_t stream) {
  const int block = lv_block(o.B), grid = (o.B + block - 1) / block;
  const size_t shm = o.T <= DUAL_TS_LDS_MAX ? (size_t)o.T * sizeof(double) : 0;
  const int rc = lde_host::lv_dispatch(solver, o.adaptive != 0, [&](auto S) -> int {
    if (shm)
      hipLaunchKernelGGL((k_lv_forward_dual<S, true>), dim3(grid), dim3(block), shm, stream, (const float2*)z0, theta, ts_dev, o,
                         rec, (float2*)z_out, retcode, nfe, nacc, nrej, ret);
    else
      hipLaunchKernelGGL((k_lv_forward_dual<S, false>), dim3(grid), dim3(block), 0, stream, (const float2*)z0, theta, ts_dev, o,
                         rec, (float2*)z_out, retcode, nfe, nacc, nrej, ret);
    return LDE_OK;
  });
  return rc != LDE_OK ? rc : hipGetLastError() == hipSuccess ? LDE_OK : LDE_ERR_HIP;
}

int launch_lv_adjoint_dual(const DualRec& rec, const float* dz_out, int T, int B, float* dz0, float* dtheta, int32_t* nfe, int32_t* nacc,
                           int32_t* nrej, int32_t* ret, hipStream_t stream) {
  const int block = lv_block(B), grid = (B + block - 1) / block;
  hipLaunchKernelGGL(k_lv_adjoint_dual, dim3(grid), dim3(block), 0, stream, rec, (const float2*)dz_out, T, B, (float2*)dz0, dtheta,
                     nfe, nacc, nrej, ret);
  return hipGetLastError() == hipSuccess ? LDE_OK : LDE_ERR_HIP;
}

}  // namespace lde
