// lde_dual_dir.hip — LDE_SENSE_FORWARD_DUAL with ONE LANE PER (TRAJECTORY, PARTIAL DIRECTION): the dual-number solve for systems of more than
// two states, as kernels over a system: LDE_RHS_KURAMOTO (N = 2 … 7 phase oscillators: csrc/lde_kuramoto_dualrhs.h, KuramotoDir<N>),
// LDE_RHS_DOUBLE_PENDULUM (four states, four parameters: csrc/lde_dpend_dualrhs.h, DoublePendDir), LDE_RHS_CVS (the cardiovascular
// system, four states, two parameters: csrc/lde_cvs_dualrhs.h, CvsDir) and LDE_RHS_STUART_LANDAU (N = 1 … 3 Hopf oscillators, 2N states,
// 2N + 1 parameters: csrc/lde_sl_dualrhs.h, StuartLandauDir<N>) — the last one also under additive noise, by k_forward_sde_dir below.
//
// k_forward_dual (csrc/lde_dual.hip) keeps a trajectory's whole dual state, D·(1 + D + P) floats, and Tsit5's seven slopes of it in one lane:
// 14 floats per vector for Lotka–Volterra, 112 for seven oscillators — it cannot grow in D. Here a trajectory is a GROUP of G consecutive
// lanes (SYS::G: 8 or 16 — a group never leaves a 16-lane row; lde_host::dir_group_width is the host's copy of the rule) and lane q of the
// group carries
//   * the D values z — redundant: every lane of the group computes the same bits from the same inputs by the same instructions —
//   * and ONE tangent column v = ∂z/∂q_q, q = (ẑ₀ (D), θ (NP − D)),
// 2D floats per vector, ≈ 12 vectors live. Lanes q ≥ NP are pad lanes (Kuramoto: G − 2N − 1 of them; the double pendulum: none; CVS: two): zero seed,
// zero forcing, so their tangent stays 0, adds 0 to every norm, and they need no branch. The stage sums, the solution weights and the
// interpolant are lde_device.h's on the 2D-vector (tsit5_attempt / rk4_step / tsit5_dense_*), as k_forward_dual uses them on its DN-vector;
// the loop around them is k_forward_dual's. What a system supplies: D, NP ≤ G, G, DN = 2·D, load(theta, b, q), seed(z0, b, q, y),
// anchor(y) (once per step attempt: the whole turns of its angles) and operator()(u, du).
//
// Step control is csrc/lde_dual.h's, from 2 to D components: ‖u_i‖ = sqrt(v_i² + Σ_q p_iq²), scale abstol + reltol·max(‖y_i‖, ‖y_new,i‖),
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
// The dual record of this kind (lde_types.h: DualRec; include/lde.h: "the Kuramoto system", "the double pendulum", "the cardiovascular system") is n [B] | J [T][D][B][G]:
// element (j, i, b, q) = ∂ẑ_i(t_j)/∂q_q at ((j·D + i)·B + b)·G + q — a wave's 64 lanes write 64 consecutive floats per (save time,
// component), and the pullback reads them the same way (the trajectory-fastest layout of the two-state kernels would put neighbouring lanes
// B floats apart). Pad lanes write their zeros. ẑ goes to z_out [T×B×D] from the group's first lane, which also writes the step trace, the
// return code and the statistics (dual_finish). Failed solve: NaN block in ẑ, zero J, rec.n[b] = −retcode [REF GOKU.jl:114].
// k_adjoint_dual_dir<D, NP, G>: lane (b, q) forms g_q = Σ_j Σ_i J_j[i][q]·dz_out_j[i], j outer, i inner, in f32 (the checkers' order); lanes
// q < D write dz0 [B×D], lanes D ≤ q < NP write dθ [B×(NP−D)], pad lanes nothing.
#include "lde_device.h"
#include "lde_dual.h"
#include "lde_host.h"
#include "lde_kuramoto_dualrhs.h"
#include "lde_dpend_dualrhs.h"
#include "lde_cvs_dualrhs.h"
#include "lde_sl_dualrhs.h"
#include "lde_philox.h"

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

// ‖u_i‖ of every component, the same bits on every lane of the group: sqrt(v_i² + Σ_q p_iq²), this lane's p_i = u[D + i]
template <int D, int G>
__device__ __forceinline__ void dir_abs(const float (&u)[2 * D], float (&nrm)[D]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int i = 0; i < D; i++) {
    const float p2 = group_sum<G>(u[D + i] * u[D + i]);
    nrm[i] = sqrtf(u[i] * u[i] + p2);
  }
}

// RMS over the D components of ‖e_i‖ / sk_i: each ratio and its square in f32, the sum of squares and the root in f64 (lde_dual.h: dual_rms)
template <int D>
__device__ __forceinline__ double dir_rms(const float (&ne)[D], const float (&sk)[D]) {
#pragma clang fp contract(off)
  double s2 = 0.0;
#pragma unroll
  for (int i = 0; i < D; i++) {
    const float r = ne[i] / sk[i];
    s2 += (double)(r * r);
  }
  return sqrt(s2 / (double)D);
}

// Hairer–Nørsett–Wanner initial step with every norm the dual norm; f0 = f(y0) given (lde_dual.h: dual_init_dt)
template <int D, int G, class F>
__device__ __forceinline__ double dir_init_dt(F& f, const float (&y)[2 * D], const float (&f0)[2 * D], double dtmax, const KOpts& o) {
  constexpr int DN = 2 * D;
  float sk[D], nn[D];
  dir_abs<D, G>(y, nn);
  {
#pragma clang fp contract(off)
#pragma unroll
    for (int i = 0; i < D; i++) sk[i] = o.abstol + nn[i] * o.reltol;
  }
  const double d0 = dir_rms<D>(nn, sk);
  dir_abs<D, G>(f0, nn);
  const double d1 = dir_rms<D>(nn, sk);
  double dt0 = (d0 < 1e-5 || d1 < 1e-5) ? 1e-6 : 0.01 * d0 / d1;
  if (dt0 > dtmax) dt0 = dtmax;
  const float h = (float)dt0;
  float tmp[DN], f1[DN];
#pragma unroll
  for (int c = 0; c < DN; c++) tmp[c] = y[c] + h * f0[c];
  f(tmp, f1);
#pragma unroll
  for (int c = 0; c < DN; c++) f1[c] -= f0[c];
  dir_abs<D, G>(f1, nn);
  const double d2 = dir_rms<D>(nn, sk) / dt0, dm = d1 > d2 ? d1 : d2;
  const double dt1 = (dm <= 1e-15) ? fmax(1e-6, dt0 * 1e-3) : pow(10.0, -(2.0 + log10(dm)) / 5.0);
  const double dt = fmin(100.0 * dt0, dt1);
  return dt > dtmax ? dtmax : dt;
}

// EEst of a Tsit5 attempt: e = h·Σ_j b̃_j k_j per entry, scale abstol + reltol·max(‖y_i‖, ‖y_new,i‖), RMS of ‖e_i‖ / scale (lde_dual.h: dual_eest)
template <int D, int G>
__device__ __forceinline__ float dir_eest(float h, const float (&y)[2 * D], const float (&yn)[2 * D], const float (&k)[7][2 * D], const KOpts& o) {
  constexpr int DN = 2 * D;
  float e[DN];
#pragma unroll
  for (int c = 0; c < DN; c++) {
    float a = ts5::BT[0] * k[0][c];
#pragma unroll
    for (int j = 1; j < 7; j++) a += ts5::BT[j] * k[j][c];
    e[c] = a * h;
  }
  float sk[D], na[D], nb[D];
  dir_abs<D, G>(y, na);
  dir_abs<D, G>(yn, nb);
  {
#pragma clang fp contract(off)
#pragma unroll
    for (int i = 0; i < D; i++) sk[i] = o.abstol + fmaxf(na[i], nb[i]) * o.reltol;
  }
  dir_abs<D, G>(e, na);
  return (float)dir_rms<D>(na, sk);
}

// ẑ_j from the group's first lane, this lane's column of J_j: J [T][D][B][G]
template <int D, int G>
__device__ __forceinline__ void dir_save(float* z_out, const DualRec& rec, int j, int B, long long b, int q, const float (&u)[2 * D]) {
  if (q == 0) {
    float* zj = z_out + ((size_t)j * B + b) * D;
#pragma unroll
    for (int i = 0; i < D; i++) zj[i] = u[i];
  }
  float* Jj = rec.J + ((size_t)j * D * B + b) * G + q;
#pragma unroll
  for (int i = 0; i < D; i++) Jj[(size_t)i * B * G] = u[D + i];
}

// SYS (csrc/lde_kuramoto_dualrhs.h: KuramotoDir<N>; csrc/lde_dpend_dualrhs.h: DoublePendDir; csrc/lde_cvs_dualrhs.h: CvsDir; csrc/lde_sl_dualrhs.h: StuartLandauDir<N>) supplies D components, NP ≤ G directions, the
// group width G (8 or 16), DN = 2·D, load(theta, b, q), seed(z0, b, q, y), anchor(y) and operator()(u, du).
template <class SYS, int SOLVER, bool TS_LDS>
__global__ void __launch_bounds__(256) k_forward_dual_dir(const float* __restrict__ z0, const float* __restrict__ theta,
                                                          const double* __restrict__ ts_g, KOpts o, DualRec rec, float* __restrict__ z_out,
                                                          int32_t* __restrict__ retcode, int32_t* __restrict__ st_nfe,
                                                          int32_t* __restrict__ st_nacc, int32_t* __restrict__ st_nrej,
                                                          int32_t* __restrict__ st_ret) {
  constexpr int D = SYS::D, DN = SYS::DN, G = SYS::G;
  static_assert(DN == 2 * D && SYS::NP <= G && (G == 8 || G == 16), "a trajectory's directions fit its group, and groups tile a 16-lane row");
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
  dir_save<D, G>(z_out, rec, 0, B, b, q, y);   // ts[0] is saved as ẑ₀ itself
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
      dt = dir_init_dt<D, G>(f, y, k[0], dtmax, o);
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
      f.anchor(y);
      if (SOLVER == LDE_SOLVER_TSIT5) {
        tsit5_attempt<DN, SYS, false, 0>(f, h, y, k, yn, o);
        if (o.adaptive) EEst = dir_eest<D, G>(h, y, yn, k, o);
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
          dir_save<D, G>(z_out, rec, j, B, b, q, u);
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
    for (int c = 0; c < DN; c++) u[c] = c < D ? __int_as_float(0x7fc00000) : 0.f;
    for (int jj = 0; jj < T; jj++) dir_save<D, G>(z_out, rec, jj, B, b, q, u);
  }
  if (q == 0) dual_finish((int)b, ret, nfe, nacc, nrej, rec, retcode, st_nfe, st_nacc, st_nrej, st_ret);
}

// g_q = Σ_j Σ_i J_j[i][q]·dz_out_j[i]: j outer, i inner
template <int D, int NP, int G>
__global__ void __launch_bounds__(256) k_adjoint_dual_dir(DualRec rec, const float* __restrict__ dz_out, int T, int B, float* __restrict__ dz0,
                                                          float* __restrict__ dtheta, int32_t* __restrict__ st_nfe,
                                                          int32_t* __restrict__ st_nacc, int32_t* __restrict__ st_nrej,
                                                          int32_t* __restrict__ st_ret) {
  static_assert(D <= NP && NP <= G && (G == 8 || G == 16), "directions: the D of ẑ₀ first, then θ's");
  const long long lane = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long b = lane / G;
  const int q = (int)(lane % G);
  if (b >= B) return;
  const int n = rec.n[b];
  float g = 0.f;
  if (n >= 0) {   // (a failed trajectory's gradient is zero whatever its cotangent holds: a NaN ẑ block usually brings a NaN one)
    const float* Jb = rec.J + (size_t)b * G + q;
    for (int j = 0; j < T; j++) {
      const float* d = dz_out + ((size_t)j * B + b) * D;
      const float* Jj = Jb + (size_t)j * D * B * G;
#pragma unroll
      for (int i = 0; i < D; i++) g += Jj[(size_t)i * B * G] * d[i];
    }
  }
  if (q < D) dz0[(size_t)D * b + q] = g;
  else if (q < NP) dtheta[(size_t)(NP - D) * b + (q - D)] = g;
  if (q == 0) {
    st_nfe[b] = 0;
    st_nacc[b] = 0;
    st_nrej[b] = 0;
    st_ret[b] = n < 0 ? -n : LDE_RET_SUCCESS;
  }
}

// ---- the stochastic solve in the same frame: dz = f(z) dt + σ dW, diagonal additive noise with one σ (include/lde.h: "the Stuart–Landau
// network") — k_pend_forward_sde's stepper (csrc/lde_pend_sde.hip) over a system SYS, a group of G lanes per trajectory. Fixed-step EM() or
// EulerHeun() on the substeps of lde::sde_substeps, save times hit exactly, one draw per substep shared by both lines of EulerHeun. Lane q
// carries the D values and its one tangent column; the tangents get no noise — the gradient is the exact derivative of the scheme along the
// drawn path, and the pullback is k_adjoint_dual_dir on the record this kernel leaves.
// EVERY lane of a group computes the draw itself, from the same counter by the same instructions: the G copies of z receive the same bits
// of ΔW and stay the same bits; no lane reads another's. Component c takes word c mod 4 of Philox block ⌊c/4⌋ of (trajectory, substep);
// words (0, 1) and (2, 3) are Box–Muller pairs. Block 0 has the stochastic pendulum's counter and key; block 1 (D > 4) the same counter and
// the key with the top bit of its high word flipped. One look per save interval for a non-finite state — a count over the group, so the
// group decides together. `over`: the host's substep plan is longer than maxiters (lde_host::sde_plan): LDE_RET_MAXITERS, nothing stepped.
template <class SYS, int SOLVER, bool TS_LDS>
__global__ void __launch_bounds__(256) k_forward_sde_dir(const float* __restrict__ z0, const float* __restrict__ theta,
                                                         const double* __restrict__ ts_g, KOpts o, DualRec rec, SdeNoise nz, float sigma, int over,
                                                         float* __restrict__ z_out, int32_t* __restrict__ retcode, int32_t* __restrict__ st_nfe,
                                                         int32_t* __restrict__ st_nacc, int32_t* __restrict__ st_nrej,
                                                         int32_t* __restrict__ st_ret) {
  constexpr int D = SYS::D, DN = SYS::DN, G = SYS::G;
  static_assert(DN == 2 * D && SYS::NP <= G && (G == 8 || G == 16) && D % 2 == 0 && D <= 8, "whole Box–Muller pairs, at most two Philox blocks");
  static_assert(SOLVER == LDE_SOLVER_EM || SOLVER == LDE_SOLVER_EULER_HEUN, "the two stochastic steppers");
  const int T = o.T, B = o.B;
  dual_stage_ts<TS_LDS>(ts_g, T);
  const long long lane = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long b = lane / G;
  const int q = (int)(lane % G);
  if (b >= B) return;   // (the whole group: its G lanes share b)

  SYS f = SYS::load(theta, b, q);
  float y[DN];
  SYS::seed(z0, b, q, y);
  dir_save<D, G>(z_out, rec, 0, B, b, q, y);   // ẑ(ts[0]) = ẑ₀
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
      const double tj = dual_ts<TS_LDS>(ts_g, j), Dt = tj - tprev;
      const int n = sde_substeps(Dt, o.dt_fixed);
      const double hd = Dt / (double)n;
      const float h = (float)hd, hh = 0.5f * h, sw = sigma * sqrtf(h);
      for (int i = 0; i < n; i++, s++) {
        float dw[D];
#pragma unroll
        for (int m = 0; m < (D + 3) / 4; m++) {
          unsigned w[4];
          philox4x32_10(c_traj, s, c_lo, c_hi, k_lo, m ? k_hi ^ 0x80000000u : k_hi, w);
#pragma unroll
          for (int p = 0; p < 2; p++)
            if (4 * m + 2 * p < D) {
              float xa, xb;
              box_muller_pair(w[2 * p], w[2 * p + 1], xa, xb);
              dw[4 * m + 2 * p] = sw * xa;
              dw[4 * m + 2 * p + 1] = sw * xb;
            }
        }
        float k0[DN];
        f.anchor(y);
        f(y, k0);
        if (SOLVER == LDE_SOLVER_EM) {
#pragma unroll
          for (int c = 0; c < DN; c++) y[c] += h * k0[c];
        } else {
          float yb[DN], k1[DN];
#pragma unroll
          for (int c = 0; c < DN; c++) yb[c] = y[c] + h * k0[c];
#pragma unroll
          for (int c = 0; c < D; c++) yb[c] += dw[c];
          f(yb, k1);
#pragma unroll
          for (int c = 0; c < DN; c++) y[c] += hh * (k0[c] + k1[c]);
        }
#pragma unroll
        for (int c = 0; c < D; c++) y[c] += dw[c];
        if (q == 0 && rec.t && nsub + i < rec.cap) {   // option "step_trace": the substep's start time and size
          rec.t[(size_t)(nsub + i) * B + b] = tprev + (double)i * hd;
          rec.dt[(size_t)(nsub + i) * B + b] = hd;
        }
      }
      nsub += n;
      // (a non-finite value never becomes finite again under y ← y + …: one look per save interval sees it; one lane's tangent may overflow
      // where its neighbours' do not, so the group counts)
      const float nbad = group_sum<G>(all_finite<DN>(y) ? 0.f : 1.f);
      if (nbad != 0.f) { ret = LDE_RET_NONFINITE; break; }
      dir_save<D, G>(z_out, rec, j, B, b, q, y);
      tprev = tj;
    }
  }
  if (ret != LDE_RET_SUCCESS) {   // failed solve ⇒ NaN block and zero Jacobians (zero gradient) [REF GOKU.jl:114]
    float u[DN];
#pragma unroll
    for (int c = 0; c < DN; c++) u[c] = c < D ? __int_as_float(0x7fc00000) : 0.f;
    for (int jj = 0; jj < T; jj++) dir_save<D, G>(z_out, rec, jj, B, b, q, u);
  }
  constexpr int NFE = SOLVER == LDE_SOLVER_EM ? 1 : 2;
  const int nacc = (int)(nsub < 0x3fffffffLL ? nsub : 0x3fffffffLL);   // (int32 statistics: a longer solve saturates)
  if (q == 0) dual_finish((int)b, ret, NFE * nacc, nacc, 0, rec, retcode, st_nfe, st_nacc, st_nrej, st_ret);
}

// ---- host-side launchers (called from lde_api.hip) -------------------------------------------------------------------------------
// lde_host::dir_all_dispatch hands out (rhs_kind, state_dim) as constants; this is the system they name
template <int KIND, int N>
struct DirSystem;
template <int N>
struct DirSystem<LDE_RHS_KURAMOTO, N> { using type = KuramotoDir<N>; };
template <>
struct DirSystem<LDE_RHS_DOUBLE_PENDULUM, 4> { using type = DoublePendDir; };
template <>
struct DirSystem<LDE_RHS_CVS, 4> { using type = CvsDir; };
template <int D>
struct DirSystem<LDE_RHS_STUART_LANDAU, D> { using type = StuartLandauDir<D / 2>; };

int launch_forward_dual_dir(const lde_problem_desc& d, const float* z0, const float* theta, const double* ts_dev, const KOpts& o,
                            const DualRec& rec, float* z_out, int32_t* retcode, int32_t* nfe, int32_t* nacc, int32_t* nrej, int32_t* ret,
                            hipStream_t stream) {
  const int block = lde_host::dir_block(d, o.B);
  const int64_t grid = lde_host::dir_grid(d, o.B);
  if (grid < 1 || grid > 0x7fffffff) return LDE_ERR_INVALID_ARG;
  const size_t shm = o.T <= DUAL_TS_LDS_MAX ? (size_t)o.T * sizeof(double) : 0;
  const int rc = lde_host::dir_all_dispatch(d, [&](auto kind, auto n, auto S) -> int {
    using SYS = typename DirSystem<kind, n>::type;
    static_assert(SYS::D == n && SYS::G == lde_host::dir_group_width(kind, n) && SYS::NP == lde_host::dir_partials(kind, n), "the host's shape of the launch is the system's");
    if (shm)
      hipLaunchKernelGGL((k_forward_dual_dir<SYS, S, true>), dim3((unsigned)grid), dim3(block), shm, stream, z0, theta, ts_dev, o, rec, z_out,
                         retcode, nfe, nacc, nrej, ret);
    else
      hipLaunchKernelGGL((k_forward_dual_dir<SYS, S, false>), dim3((unsigned)grid), dim3(block), 0, stream, z0, theta, ts_dev, o, rec, z_out,
                         retcode, nfe, nacc, nrej, ret);
    return LDE_OK;
  });
  return rc != LDE_OK ? rc : hipGetLastError() == hipSuccess ? LDE_OK : LDE_ERR_HIP;
}

int launch_adjoint_dual_dir(const lde_problem_desc& d, const DualRec& rec, const float* dz_out, int T, int B, float* dz0, float* dtheta,
                            int32_t* nfe, int32_t* nacc, int32_t* nrej, int32_t* ret, hipStream_t stream) {
  const int block = lde_host::dir_block(d, B);
  const int64_t grid = lde_host::dir_grid(d, B);
  if (grid < 1 || grid > 0x7fffffff) return LDE_ERR_INVALID_ARG;
  const int rc = lde_host::dir_all_dispatch_n(d, [&](auto kind, auto n) -> int {
    constexpr int NP = lde_host::dir_partials(kind, n), G = lde_host::dir_group_width(kind, n);
    hipLaunchKernelGGL((k_adjoint_dual_dir<n, NP, G>), dim3((unsigned)grid), dim3(block), 0, stream, rec, dz_out, T, B, dz0, dtheta, nfe, nacc,
                       nrej, ret);
    return LDE_OK;
  });
  return rc != LDE_OK ? rc : hipGetLastError() == hipSuccess ? LDE_OK : LDE_ERR_HIP;
}

// the stochastic solve: lde_host::dir_sde_dispatch hands out the Stuart–Landau network's D and the two solvers validate() admits for it
int launch_forward_sde_dir(const lde_problem_desc& d, const float* z0, const float* theta, const double* ts_dev, const KOpts& o,
                           const DualRec& rec, const SdeNoise& nz, float sigma, bool over, float* z_out, int32_t* retcode, int32_t* nfe,
                           int32_t* nacc, int32_t* nrej, int32_t* ret, hipStream_t stream) {
  const int block = lde_host::dir_block(d, o.B);
  const int64_t grid = lde_host::dir_grid(d, o.B);
  if (grid < 1 || grid > 0x7fffffff) return LDE_ERR_INVALID_ARG;
  const size_t shm = o.T <= DUAL_TS_LDS_MAX ? (size_t)o.T * sizeof(double) : 0;
  const int rc = lde_host::dir_sde_dispatch(d, [&](auto n, auto S) -> int {
    using SYS = typename DirSystem<LDE_RHS_STUART_LANDAU, n>::type;
    static_assert(SYS::D == n && SYS::G == lde_host::dir_group_width(LDE_RHS_STUART_LANDAU, n) && SYS::NP == lde_host::dir_partials(LDE_RHS_STUART_LANDAU, n), "the host's shape of the launch is the system's");
    if (shm)
      hipLaunchKernelGGL((k_forward_sde_dir<SYS, S, true>), dim3((unsigned)grid), dim3(block), shm, stream, z0, theta, ts_dev, o, rec, nz, sigma,
                         (int)over, z_out, retcode, nfe, nacc, nrej, ret);
    else
      hipLaunchKernelGGL((k_forward_sde_dir<SYS, S, false>), dim3((unsigned)grid), dim3(block), 0, stream, z0, theta, ts_dev, o, rec, nz, sigma,
                         (int)over, z_out, retcode, nfe, nacc, nrej, ret);
    return LDE_OK;
  });
  return rc != LDE_OK ? rc : hipGetLastError() == hipSuccess ? LDE_OK : LDE_ERR_HIP;
}

}  // namespace lde
