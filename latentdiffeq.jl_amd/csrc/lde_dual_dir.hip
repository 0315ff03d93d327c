// lde_dual_dir.hip — LDE_SENSE_FORWARD_DUAL with ONE LANE PER (TRAJECTORY, PARTIAL DIRECTION): the dual-number solve for systems of more than
// two states (LDE_RHS_KURAMOTO, N = 2 … 7 phase oscillators: csrc/lde_kuramoto_dualrhs.h).
//
// k_forward_dual (csrc/lde_dual.hip) keeps a trajectory's whole dual state, D·(1 + D + P) floats, and Tsit5's seven slopes of it in one lane:
// 14 floats per vector for Lotka–Volterra, 112 for seven oscillators — it cannot grow in D. Here a trajectory is a GROUP of G consecutive
// lanes (lde_host::dir_group_width: 8 for N ≤ 3, 16 for N ≤ 7 — a group never leaves a 16-lane row) and lane q of the group carries
//   * the N values φ — redundant: every lane of the group computes the same bits from the same inputs by the same instructions —
//   * and ONE tangent column v = ∂φ/∂q_q, q = (φ₀ (N), ω (N), K),
// 2N floats per vector, ≈ 12 vectors live. Lanes q ≥ NP = 2N + 1 are pad lanes: zero seed, zero forcing, so their tangent stays 0, adds 0
// to every norm, and they need no branch. The stage sums, the solution weights and the interpolant are lde_device.h's on the 2N-vector
// (tsit5_attempt / rk4_step / tsit5_dense_*), as k_forward_dual uses them on its DN-vector; the loop around them is k_forward_dual's.
//
// Step control is csrc/lde_dual.h's, from 2 to N components: ‖u_i‖ = sqrt(v_i² + Σ_q p_iq²), scale abstol + reltol·max(‖y_i‖, ‖y_new,i‖),
// EEst the RMS over i of ‖e_i‖ / scale_i — ratios and squares in f32, the sum over i and the root in f64 — and the Hairer initial step on
// the same norms. Σ_q runs ACROSS the lanes of a group, and every lane of a group must hold the same bits of it: EEst, the accept decision
// and dt follow from it, and lanes that disagreed would walk different step sequences. The sum is a BUTTERFLY over the group (group_sum):
// at every level a lane adds its partner's value to its own, the partner adds this lane's to its — a + b and b + a are the same bits (IEEE
// addition is commutative), so after log₂ G levels all G lanes hold one value. A rotate-and-add all-reduce would associate the sum
// differently on every lane. (No fused multiply-add may slip into a level — fma(p, p, partner) would round one lane's own square
// differently from the partner's view of it: contraction is off in these functions.) Control flow in the stepping loop is then uniform over
// a group, so a lane's partners are always active; a group whose trajectory is past the batch leaves as a whole, after dual_stage_ts's
// barrier. Groups of one wave do take different numbers of steps: that is divergence between groups, never inside one.
//
// The dual record of this kind (lde_types.h: DualRec; include/lde.h: "the Kuramoto system") is n [B] | J [T][N][B][G]: element (j, i, b, q)
// = ∂ẑ_i(t_j)/∂q_q at ((j·N + i)·B + b)·G + q — a wave's 64 lanes write 64 consecutive floats per (save time, component), and the pullback
// reads them the same way (the trajectory-fastest layout of the two-state kernels would put neighbouring lanes B floats apart). Pad lanes
// write their zeros. ẑ goes to z_out [T×B×N] from the group's first lane, which also writes the step trace, the return code and the
// statistics (dual_finish). Failed solve: NaN block in ẑ, zero J, rec.n[b] = −retcode [REF GOKU.jl:114].
// k_adjoint_dual_dir<N>: lane (b, q) forms g_q = Σ_j Σ_i J_j[i][q]·dz_out_j[i], j outer, i inner, in f32 (the checkers' order); lanes q < N
// write dz0 [B×N], lanes N ≤ q < NP write dθ [B×(N+1)], pad lanes nothing.
#include "lde_device.h"
#include "lde_dual.h"
#include "lde_host.h"
#include "lde_kuramoto_dualrhs.h"

namespace lde {

// x of this lane + x of lane (lane ^ m), m = 1, 2 by quad permutes; the two halves of 8 and of 16 lanes meet through the mirrors (lane i with
// 7 − i, then with 15 − i: partners in the other half, which is all a level needs once the halves are uniform)
template <int CTRL>
__device__ __forceinline__ float dpp_pair_add(float x) {
#pragma clang fp contract(off)
  return x + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, 0xf, 0xf, false));
}
template <int G>
__device__ __forceinline__ float group_sum(float x) {
  static_assert(G == 8 || G == 16, "a group is 8 or 16 lanes of one row");
  x = dpp_pair_add<0xB1>(x);    // quad_perm [1, 0, 3, 2]
  x = dpp_pair_add<0x4E>(x);    // quad_perm [2, 3, 0, 1]
  x = dpp_pair_add<0x141>(x);   // row_half_mirror
  if (G == 16) x = dpp_pair_add<0x140>(x);   // row_mirror
  return x;
}

// ‖u_i‖ of every component, the same bits on every lane of the group: sqrt(v_i² + Σ_q p_iq²), this lane's p_i = u[N + i]
template <int N, int G>
__device__ __forceinline__ void dir_abs(const float (&u)[2 * N], float (&nrm)[N]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int i = 0; i < N; i++) {
    const float p2 = group_sum<G>(u[N + i] * u[N + i]);
    nrm[i] = sqrtf(u[i] * u[i] + p2);
  }
}

// RMS over the N components of ‖e_i‖ / sk_i: each ratio and its square in f32, the sum of squares and the root in f64 (lde_dual.h: dual_rms)
template <int N>
__device__ __forceinline__ double dir_rms(const float (&ne)[N], const float (&sk)[N]) {
#pragma clang fp contract(off)
  double s2 = 0.0;
#pragma unroll
  for (int i = 0; i < N; i++) {
    const float r = ne[i] / sk[i];
    s2 += (double)(r * r);
  }
  return sqrt(s2 / (double)N);
}

// Hairer–Nørsett–Wanner initial step with every norm the dual norm; f0 = f(y0) given (lde_dual.h: dual_init_dt)
template <int N, int G, class F>
__device__ __forceinline__ double dir_init_dt(F& f, const float (&y)[2 * N], const float (&f0)[2 * N], double dtmax, const KOpts& o) {
  constexpr int DN = 2 * N;
  float sk[N], nn[N];
  dir_abs<N, G>(y, nn);
  {
#pragma clang fp contract(off)
#pragma unroll
    for (int i = 0; i < N; i++) sk[i] = o.abstol + nn[i] * o.reltol;
  }
  const double d0 = dir_rms<N>(nn, sk);
  dir_abs<N, G>(f0, nn);
  const double d1 = dir_rms<N>(nn, sk);
  double dt0 = (d0 < 1e-5 || d1 < 1e-5) ? 1e-6 : 0.01 * d0 / d1;
  if (dt0 > dtmax) dt0 = dtmax;
  const float h = (float)dt0;
  float tmp[DN], f1[DN];
#pragma unroll
  for (int c = 0; c < DN; c++) tmp[c] = y[c] + h * f0[c];
  f(tmp, f1);
#pragma unroll
  for (int c = 0; c < DN; c++) f1[c] -= f0[c];
  dir_abs<N, G>(f1, nn);
  const double d2 = dir_rms<N>(nn, sk) / dt0, dm = d1 > d2 ? d1 : d2;
  const double dt1 = (dm <= 1e-15) ? fmax(1e-6, dt0 * 1e-3) : pow(10.0, -(2.0 + log10(dm)) / 5.0);
  const double dt = fmin(100.0 * dt0, dt1);
  return dt > dtmax ? dtmax : dt;
}

// EEst of a Tsit5 attempt: e = h·Σ_j b̃_j k_j per entry, scale abstol + reltol·max(‖y_i‖, ‖y_new,i‖), RMS of ‖e_i‖ / scale (lde_dual.h: dual_eest)
template <int N, int G>
__device__ __forceinline__ float dir_eest(float h, const float (&y)[2 * N], const float (&yn)[2 * N], const float (&k)[7][2 * N], const KOpts& o) {
  constexpr int DN = 2 * N;
  float e[DN];
#pragma unroll
  for (int c = 0; c < DN; c++) {
    float a = ts5::BT[0] * k[0][c];
#pragma unroll
    for (int j = 1; j < 7; j++) a += ts5::BT[j] * k[j][c];
    e[c] = a * h;
  }
  float sk[N], na[N], nb[N];
  dir_abs<N, G>(y, na);
  dir_abs<N, G>(yn, nb);
  {
#pragma clang fp contract(off)
#pragma unroll
    for (int i = 0; i < N; i++) sk[i] = o.abstol + fmaxf(na[i], nb[i]) * o.reltol;
  }
  dir_abs<N, G>(e, na);
  return (float)dir_rms<N>(na, sk);
}

// ẑ_j from the group's first lane, this lane's column of J_j: J [T][N][B][G]
template <int N, int G>
__device__ __forceinline__ void dir_save(float* z_out, const DualRec& rec, int j, int B, long long b, int q, const float (&u)[2 * N]) {
  if (q == 0) {
    float* zj = z_out + ((size_t)j * B + b) * N;
#pragma unroll
    for (int i = 0; i < N; i++) zj[i] = u[i];
  }
  float* Jj = rec.J + ((size_t)j * N * B + b) * G + q;
#pragma unroll
  for (int i = 0; i < N; i++) Jj[(size_t)i * B * G] = u[N + i];
}

template <int N, int SOLVER, bool TS_LDS>
__global__ void __launch_bounds__(256) k_forward_dual_dir(const float* __restrict__ z0, const float* __restrict__ theta,
                                                          const double* __restrict__ ts_g, KOpts o, DualRec rec, float* __restrict__ z_out,
                                                          int32_t* __restrict__ retcode, int32_t* __restrict__ st_nfe,
                                                          int32_t* __restrict__ st_nacc, int32_t* __restrict__ st_nrej,
                                                          int32_t* __restrict__ st_ret) {
  using SYS = KuramotoDir<N>;
  constexpr int DN = 2 * N, G = lde_host::dir_group_width(N);
  static_assert(SYS::NP <= G && 64 % G == 0, "a trajectory's directions fit its group, and groups tile a wave");
  const int T = o.T, B = o.B;
  dual_stage_ts<TS_LDS>(ts_g, T);
  auto s_ts = [&](int i) -> double { return dual_ts<TS_LDS>(ts_g, i); };
  const long long lane = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long b = lane / G;
  const int q = (int)(lane % G);
  if (b >= B) return;   // (the whole group: its G lanes share b)

  SYS f = SYS::load(theta, b, q);
  float y[DN];
  SYS::seed(z0, b, q, y);
  float k[7][DN], yn[DN];
  dir_save<N, G>(z_out, rec, 0, B, b, q, y);   // ts[0] is saved as ẑ₀ itself
  int ret = LDE_RET_SUCCESS, nfe = 0, nacc = 0, nrej = 0;

  if (T > 1) {
    double t = o.t_first;
    const double tend = o.t_last, dtmax = tend - t;
    f.anchor(y);
    f(y, k[0]);
    nfe = 1;
    double dt;
    if (!o.adaptive) dt = o.dt_fixed;
    else if (o.dt_fixed > 0) dt = fmin(o.dt_fixed, dtmax);
    else {
      dt = dir_init_dt<N, G>(f, y, k[0], dtmax, o);
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
      f.anchor(y);
      if (SOLVER == LDE_SOLVER_TSIT5) {
        tsit5_attempt<DN, SYS, false, 0>(f, h, y, k, yn, o);
        if (o.adaptive) EEst = dir_eest<N, G>(h, y, yn, k, o);
        nfe += 6;
      } else {
        rk4_step<DN>(f, h, y, k, yn);
        nfe += 4;
      }
      // one lane's tangent may overflow where its neighbours' do not: the group decides together (a count of the lanes that are not finite)
      const float nbad = group_sum<G>(all_finite<DN>(yn) ? 0.f : 1.f);
      if (nbad != 0.f || !(EEst == EEst)) {
        if (o.adaptive && dt > o.dtmin) { nrej++; dt = dt * (double)o.qmin; continue; }
        ret = LDE_RET_NONFINITE;
        break;
      }
      if (o.adaptive) {
        float q11;
        const float qq = pi_q(EEst, qold, o, q11);
        if (EEst > 1.0f) {
          nrej++;
          dt = dt * (double)fast_rcp(fminf(o.q_hi, q11 * o.inv_gamma));
          if (dt < o.dtmin) { ret = LDE_RET_DTMIN; break; }
          continue;
        }
        qold = fmaxf(EEst, 1e-4f);
        dtp = dt * (double)fast_rcp(qq);
        if (dtp > dtmax) dtp = dtmax;
      }
      if (q == 0 && rec.t && nacc < rec.cap) {   // option "step_trace": the accepted step's start time and size
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
          dir_save<N, G>(z_out, rec, j, B, b, q, u);
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
    float u[DN];
#pragma unroll
    for (int c = 0; c < DN; c++) u[c] = c < N ? __int_as_float(0x7fc00000) : 0.f;
    for (int jj = 0; jj < T; jj++) dir_save<N, G>(z_out, rec, jj, B, b, q, u);
  }
  if (q == 0) dual_finish((int)b, ret, nfe, nacc, nrej, rec, retcode, st_nfe, st_nacc, st_nrej, st_ret);
}

// g_q = Σ_j Σ_i J_j[i][q]·dz_out_j[i]: j outer, i inner
template <int N>
__global__ void __launch_bounds__(256) k_adjoint_dual_dir(DualRec rec, const float* __restrict__ dz_out, int T, int B, float* __restrict__ dz0,
                                                          float* __restrict__ dtheta, int32_t* __restrict__ st_nfe,
                                                          int32_t* __restrict__ st_nacc, int32_t* __restrict__ st_nrej,
                                                          int32_t* __restrict__ st_ret) {
  constexpr int G = lde_host::dir_group_width(N), NP = 2 * N + 1;
  const long long lane = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long b = lane / G;
  const int q = (int)(lane % G);
  if (b >= B) return;
  const int n = rec.n[b];
  float g = 0.f;
  if (n >= 0) {   // (a failed trajectory's gradient is zero whatever its cotangent holds: a NaN ẑ block usually brings a NaN one)
    const float* Jb = rec.J + (size_t)b * G + q;
    for (int j = 0; j < T; j++) {
      const float* d = dz_out + ((size_t)j * B + b) * N;
      const float* Jj = Jb + (size_t)j * N * B * G;
#pragma unroll
      for (int i = 0; i < N; i++) g += Jj[(size_t)i * B * G] * d[i];
    }
  }
  if (q < N) dz0[(size_t)N * b + q] = g;
  else if (q < NP) dtheta[(size_t)(N + 1) * b + (q - N)] = g;
  if (q == 0) {
    st_nfe[b] = 0;
    st_nacc[b] = 0;
    st_nrej[b] = 0;
    st_ret[b] = n < 0 ? -n : LDE_RET_SUCCESS;
  }
}

// ---- host-side launchers (called from lde_api.hip) -------------------------------------------------------------------------------
int launch_forward_dual_dir(int N, int solver, const float* z0, const float* theta, const double* ts_dev, const KOpts& o, const DualRec& rec,
                            float* z_out, int32_t* retcode, int32_t* nfe, int32_t* nacc, int32_t* nrej, int32_t* ret, hipStream_t stream) {
  const int block = lde_host::dir_block(N, o.B);
  const int64_t grid = lde_host::dir_grid(N, o.B);
  if (grid < 1 || grid > 0x7fffffff) return LDE_ERR_INVALID_ARG;
  const size_t shm = o.T <= DUAL_TS_LDS_MAX ? (size_t)o.T * sizeof(double) : 0;
  const int rc = lde_host::dir_dispatch(N, solver, o.adaptive != 0, [&](auto n, auto S) -> int {
    if (shm)
      hipLaunchKernelGGL((k_forward_dual_dir<n, S, true>), dim3((unsigned)grid), dim3(block), shm, stream, z0, theta, ts_dev, o, rec, z_out,
                         retcode, nfe, nacc, nrej, ret);
    else
      hipLaunchKernelGGL((k_forward_dual_dir<n, S, false>), dim3((unsigned)grid), dim3(block), 0, stream, z0, theta, ts_dev, o, rec, z_out,
                         retcode, nfe, nacc, nrej, ret);
    return LDE_OK;
  });
  return rc != LDE_OK ? rc : hipGetLastError() == hipSuccess ? LDE_OK : LDE_ERR_HIP;
}

int launch_adjoint_dual_dir(int N, const DualRec& rec, const float* dz_out, int T, int B, float* dz0, float* dtheta, int32_t* nfe,
                            int32_t* nacc, int32_t* nrej, int32_t* ret, hipStream_t stream) {
  const int block = lde_host::dir_block(N, B);
  const int64_t grid = lde_host::dir_grid(N, B);
  if (grid < 1 || grid > 0x7fffffff) return LDE_ERR_INVALID_ARG;
  const int rc = lde_host::dir_dispatch_n(N, [&](auto n) -> int {
    hipLaunchKernelGGL(k_adjoint_dual_dir<n>, dim3((unsigned)grid), dim3(block), 0, stream, rec, dz_out, T, B, dz0, dtheta, nfe, nacc, nrej, ret);
    return LDE_OK;
  });
  return rc != LDE_OK ? rc : hipGetLastError() == hipSuccess ? LDE_OK : LDE_ERR_HIP;
}

}  // namespace lde
