// lde_host.h — the host-side LOGIC of the C ABI that touches no device: validation of a problem description, the flat weight count,
// the layout arithmetic of a step record, the option block handed to the kernels, the step count of a fixed-step solve, the checks on a
// save-time grid. lde_api.hip is these functions plus HIP calls; kept apart so that an ordinary host compiler can build them under
// AddressSanitizer + UndefinedBehaviorSanitizer (tests/host_logic_driver.cpp, tests/test_sanitizers.py: GPU sanitizers are not available
// on this pool) and drive them with hostile inputs: a C ABI's arguments come from another language's runtime.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <limits>
#include <string>
#include <type_traits>

#include "lde_types.h"

namespace lde_host {
using lde::KOpts;
using lde::StepRec;
using lde::DualRec;

// ---- the lane-per-direction dual solve (csrc/lde_dual_dir.hip: k_forward_dual_dir / k_adjoint_dual_dir over a system): a trajectory of D
// states and NP partial directions is a group of G consecutive lanes, lane q of it carries the D values and the ONE tangent column ∂z/∂q_q.
// G = 8 holds NP ≤ 8, G = 16 holds NP ≤ 16: a group never leaves a 16-lane row, which is what its cross-lane sums (DPP within a row) need.
// Three systems: LDE_RHS_KURAMOTO, D = N and NP = 2N + 1 directions q = (φ₀ (N), ω (N), K), N ≤ 3 in 8 lanes and N ≤ 7 in 16 (the forms that
// take N alone are this system's; 0: N is not served), and LDE_RHS_DOUBLE_PENDULUM, D = 4 and NP = 8 = (ẑ₀ (4), L₁, L₂, m₁, m₂): one 8-lane
// group with no pad lane; and LDE_RHS_CVS, D = 4 and NP = 6 = (ẑ₀ (4), i_ext, r_mod): one 8-lane group whose lanes 6 and 7 are pad lanes. The
// forms that take (rhs_kind, state_dim) or a description serve all three, and the fourth system below (LDE_RHS_STUART_LANDAU).
constexpr int KURAMOTO_MIN_N = 2, KURAMOTO_MAX_N = 7;
static constexpr bool dir_state_ok(int N) { return N >= KURAMOTO_MIN_N && N <= KURAMOTO_MAX_N; }
static constexpr int dir_partials(int N) { return dir_state_ok(N) ? 2 * N + 1 : 0; }
static constexpr int dir_group_width(int N) { return !dir_state_ok(N) ? 0 : N <= 3 ? 8 : 16; }
// lanes of a launch over B trajectories (0: none — B < 1 or N not served) and its workgroups, by the dual solve's batch rule
// (pend_dual_mapping) applied to the LANES: a wave per workgroup up to 4 096 lanes, four waves beyond. A workgroup holds whole groups.
static int64_t dir_lanes(int N, int B) { return B < 1 ? 0 : (int64_t)B * dir_group_width(N); }
static int dir_block(int N, int B) { return dir_lanes(N, B) <= 4096 ? 64 : 256; }
static int64_t dir_grid(int N, int B) { return (dir_lanes(N, B) + dir_block(N, B) - 1) / dir_block(N, B); }
// … of either system: D = state_dim of a right-hand side of `kind` (0: not a system of these kernels, or a D it does not serve)
constexpr int DPEND_D = 4, DPEND_P = 4;
constexpr int CVS_D = 4, CVS_P = 2;
// LDE_RHS_STUART_LANDAU, the fourth system: N = 1 … 3 oscillators, D = 2N components (x₁ … x_N, y₁ … y_N), NP = 4N + 1 directions
// q = (ẑ₀ (2N), a (N), ω (N), G) — 5 in 8 lanes (N = 1), 9 and 13 in 16 (N = 2, 3). D = 6 is the first D that is no Kuramoto N and not 4.
constexpr int SL_MIN_N = 1, SL_MAX_N = 3;
static constexpr bool sl_state_ok(int D) { return D == 2 || D == 4 || D == 6; }
static constexpr bool dir_state_ok(int kind, int D) {
  return kind == LDE_RHS_KURAMOTO ? dir_state_ok(D)
                                  : (kind == LDE_RHS_DOUBLE_PENDULUM && D == DPEND_D) || (kind == LDE_RHS_CVS && D == CVS_D) ||
                                        (kind == LDE_RHS_STUART_LANDAU && sl_state_ok(D));
}
static constexpr int dir_partials(int kind, int D) {
  return kind == LDE_RHS_KURAMOTO ? dir_partials(D)
         : !dir_state_ok(kind, D) ? 0
         : kind == LDE_RHS_STUART_LANDAU ? 2 * D + 1
         : kind == LDE_RHS_CVS ? CVS_D + CVS_P
                               : DPEND_D + DPEND_P;
}
static constexpr int dir_group_width(int kind, int D) {
  return kind == LDE_RHS_KURAMOTO ? dir_group_width(D) : !dir_state_ok(kind, D) ? 0 : (kind == LDE_RHS_STUART_LANDAU && D > 2) ? 16 : 8;
}
static int dir_group_width(const lde_problem_desc& d) { return dir_group_width(d.rhs_kind, d.state_dim); }
static int64_t dir_lanes(const lde_problem_desc& d, int B) { return B < 1 ? 0 : (int64_t)B * dir_group_width(d); }
static int dir_block(const lde_problem_desc& d, int B) { return dir_lanes(d, B) <= 4096 ? 64 : 256; }
static int64_t dir_grid(const lde_problem_desc& d, int B) { return (dir_lanes(d, B) + dir_block(d, B) - 1) / dir_block(d, B); }

static bool has_mlp(const lde_problem_desc& d) {
  return d.rhs_kind == LDE_RHS_MLP || d.rhs_kind == LDE_RHS_PENDULUM_PLUS_MLP;
}
static bool is_lv(const lde_problem_desc& d) { return d.rhs_kind == LDE_RHS_LOTKA_VOLTERRA; }
static bool is_kuramoto(const lde_problem_desc& d) { return d.rhs_kind == LDE_RHS_KURAMOTO; }
static bool is_dpend(const lde_problem_desc& d) { return d.rhs_kind == LDE_RHS_DOUBLE_PENDULUM; }
static bool is_cvs(const lde_problem_desc& d) { return d.rhs_kind == LDE_RHS_CVS; }
static bool is_sl(const lde_problem_desc& d) { return d.rhs_kind == LDE_RHS_STUART_LANDAU; }
static bool is_dir(const lde_problem_desc& d) { return is_kuramoto(d) || is_dpend(d) || is_cvs(d) || is_sl(d); }   // the systems of the lane-per-direction kernels
static bool has_pend(const lde_problem_desc& d) { return d.rhs_kind != LDE_RHS_MLP && !is_lv(d) && !is_dir(d); }
static bool is_sde(const lde_problem_desc& d) { return d.rhs_kind == LDE_RHS_SPENDULUM; }
static bool sde_solver(int solver) { return solver == LDE_SOLVER_EM || solver == LDE_SOLVER_EULER_HEUN; }
// the stochastic solve of the lane-per-direction frame (csrc/lde_dual_dir.hip: k_forward_sde_dir): the Stuart–Landau network under a stochastic stepper
static bool is_dir_sde(const lde_problem_desc& d) { return is_sl(d) && sde_solver(d.solver); }

static int validate(const lde_problem_desc* d, std::string* why) {
  auto bad = [&](const char* m) {
    if (why) *why = m;
    return (int)LDE_ERR_INVALID_ARG;
  };
  if (!d) return bad("desc is NULL");
  if (d->abi_version != LDE_ABI_VERSION) return bad("abi_version mismatch");
  // 6 and 8 are no right-hand sides and stay refused: tests/lv_host_driver.cpp and tests/kuramoto_host_driver.cpp pin them as "unknown
  // rhs_kind", so the Kuramoto system took 7 and the double pendulum 9; tests/dpend_host_driver.cpp pins 10 likewise, so CVS took 11, and
  // tests/cvs_host_driver.cpp pins 12, so the Stuart–Landau network took 13 (nothing pins 14: the next kind takes it)
  if (d->rhs_kind < 0 || d->rhs_kind > LDE_RHS_STUART_LANDAU || d->rhs_kind == 6 || d->rhs_kind == 8 || d->rhs_kind == 10 || d->rhs_kind == 12)
    return bad("unknown rhs_kind");
  if (d->state_dim < 1 || d->param_dim < 0 || d->augment_dim < 0) return bad("bad dims");
  if (has_pend(*d) && (d->state_dim != 2 || d->param_dim != 1 || d->augment_dim != 0))
    return bad("pendulum RHS needs state_dim=2, param_dim=1, augment_dim=0");
  if (is_lv(*d) && (d->state_dim != 2 || d->param_dim != 4 || d->augment_dim != 0))
    return bad("LDE_RHS_LOTKA_VOLTERRA needs state_dim=2, param_dim=4, augment_dim=0");
  if (is_kuramoto(*d) && (d->state_dim < KURAMOTO_MIN_N || d->state_dim > KURAMOTO_MAX_N || d->param_dim != d->state_dim + 1 || d->augment_dim != 0))
    return bad("LDE_RHS_KURAMOTO needs state_dim=N with 2 <= N <= 7, param_dim=N+1, augment_dim=0");
  if (is_dpend(*d) && (d->state_dim != DPEND_D || d->param_dim != DPEND_P || d->augment_dim != 0))
    return bad("LDE_RHS_DOUBLE_PENDULUM needs state_dim=4, param_dim=4, augment_dim=0");
  if (is_cvs(*d) && (d->state_dim != CVS_D || d->param_dim != CVS_P || d->augment_dim != 0))
    return bad("LDE_RHS_CVS needs state_dim=4, param_dim=2, augment_dim=0");
  if (is_sl(*d) && (!sl_state_ok(d->state_dim) || d->param_dim != d->state_dim + 1 || d->augment_dim != 0))
    return bad("LDE_RHS_STUART_LANDAU needs state_dim=2N with 1 <= N <= 3, param_dim=2N+1, augment_dim=0");
  if (d->rhs_kind == LDE_RHS_MLP && d->param_dim != 0) return bad("MLP RHS takes no per-trajectory parameters");
  if (has_mlp(*d)) {
    if (d->n_layers < 1 || d->n_layers > LDE_MAX_LAYERS) return bad("n_layers out of range");
    const int Dp = d->state_dim + d->augment_dim;
    if (d->layer_sizes[0] != Dp || d->layer_sizes[d->n_layers] != Dp) return bad("MLP in/out must equal D+augment_dim");
    for (int l = 0; l <= d->n_layers; l++)
      if (d->layer_sizes[l] < 1) return bad("layer size < 1");
    if (d->activation != LDE_ACT_RELU && d->activation != LDE_ACT_TANH) return bad("unknown activation");
  }
  if (is_sde(*d) && d->n_layers != 0) return bad("LDE_RHS_SPENDULUM is analytic: n_layers must be 0");
  if (is_lv(*d) && d->n_layers != 0) return bad("LDE_RHS_LOTKA_VOLTERRA is analytic: n_layers must be 0");
  if (is_kuramoto(*d) && d->n_layers != 0) return bad("LDE_RHS_KURAMOTO is analytic: n_layers must be 0");
  if (is_dpend(*d) && d->n_layers != 0) return bad("LDE_RHS_DOUBLE_PENDULUM is analytic: n_layers must be 0");
  if (is_cvs(*d) && d->n_layers != 0) return bad("LDE_RHS_CVS is analytic: n_layers must be 0");
  if (is_sl(*d) && d->n_layers != 0) return bad("LDE_RHS_STUART_LANDAU is analytic: n_layers must be 0");
  if (d->solver != LDE_SOLVER_TSIT5 && d->solver != LDE_SOLVER_RK4 && !sde_solver(d->solver)) return bad("unknown solver");
  if (d->batching != LDE_BATCH_PER_TRAJECTORY && d->batching != LDE_BATCH_COUPLED && d->batching != LDE_BATCH_COUPLED_GLOBAL)
    return bad("unknown batching");
  if (d->batching == LDE_BATCH_COUPLED_GLOBAL && !has_mlp(*d)) return bad("LDE_BATCH_COUPLED_GLOBAL needs an MLP right-hand side");
  if (d->sensealg < LDE_SENSE_BACKSOLVE_CHECKPOINTED || d->sensealg > LDE_SENSE_FORWARD_DUAL) return bad("unknown sensealg");
  // (LDE_SENSE_DISCRETE with LDE_BATCH_COUPLED_GLOBAL: every rank records the common step sequence and ITS columns' states; the sweep
  //  has no step control, hence no sum to exchange)

  auto unsupported = [&](const char* m) {
    if (why) *why = m;
    return (int)LDE_ERR_UNSUPPORTED;
  };
  // the stochastic pendulum is served by its own two fixed-step schemes on the dual-number path; besides it they serve the Stuart–Landau
  // network (below) and nothing else (include/lde.h)
  if (sde_solver(d->solver) && !is_sde(*d) && !is_sl(*d))
    return unsupported("LDE_SOLVER_EM / LDE_SOLVER_EULER_HEUN are stochastic steppers: LDE_RHS_SPENDULUM only");
  if (is_sde(*d)) {
    if (!sde_solver(d->solver)) return unsupported("LDE_RHS_SPENDULUM: no deterministic solver; use LDE_SOLVER_EM or LDE_SOLVER_EULER_HEUN");
    if (d->batching != LDE_BATCH_PER_TRAJECTORY) return unsupported("LDE_RHS_SPENDULUM: no coupled solve; LDE_BATCH_PER_TRAJECTORY only");
    if (d->adaptive) return unsupported("LDE_RHS_SPENDULUM: no adaptive stepping (the reference's SOSRI is not reproduced); pass adaptive=0, dt=h");
    if (!(d->dt > 0) || !std::isfinite(d->dt)) return unsupported("LDE_RHS_SPENDULUM: fixed step only; pass a finite dt > 0");
    if (d->sensealg != LDE_SENSE_FORWARD_DUAL)
      return unsupported("LDE_RHS_SPENDULUM: the gradient is the scheme's exact derivative along the drawn path; use LDE_SENSE_FORWARD_DUAL");
  }
  // Lotka–Volterra is served on the dual-number path and nowhere else: the Nyström forward kernel, the discrete sweep and the continuous
  // adjoints are written for the pendulum (include/lde.h: "the Lotka–Volterra system")
  if (is_lv(*d)) {
    if (d->batching != LDE_BATCH_PER_TRAJECTORY) return unsupported("LDE_RHS_LOTKA_VOLTERRA: no coupled solve; LDE_BATCH_PER_TRAJECTORY only");
    if (d->sensealg != LDE_SENSE_FORWARD_DUAL)
      return unsupported("LDE_RHS_LOTKA_VOLTERRA: only the solve on dual numbers exists for this system (no discrete sweep, no continuous adjoint); use LDE_SENSE_FORWARD_DUAL");
  }
  // the Kuramoto system likewise: its kernels (csrc/lde_dual_dir.hip) are the dual-number solve with a lane per partial direction
  if (is_kuramoto(*d)) {
    if (d->batching != LDE_BATCH_PER_TRAJECTORY) return unsupported("LDE_RHS_KURAMOTO: no coupled solve; LDE_BATCH_PER_TRAJECTORY only");
    if (d->sensealg != LDE_SENSE_FORWARD_DUAL)
      return unsupported("LDE_RHS_KURAMOTO: only the solve on dual numbers exists for this system (no discrete sweep, no continuous adjoint); use LDE_SENSE_FORWARD_DUAL");
  }
  if (is_dpend(*d)) {   // … and the double pendulum, their second system
    if (d->batching != LDE_BATCH_PER_TRAJECTORY) return unsupported("LDE_RHS_DOUBLE_PENDULUM: no coupled solve; LDE_BATCH_PER_TRAJECTORY only");
    if (d->sensealg != LDE_SENSE_FORWARD_DUAL)
      return unsupported("LDE_RHS_DOUBLE_PENDULUM: only the solve on dual numbers exists for this system (no discrete sweep, no continuous adjoint); use LDE_SENSE_FORWARD_DUAL");
  }
  if (is_cvs(*d)) {   // … and the cardiovascular system, their third
    if (d->batching != LDE_BATCH_PER_TRAJECTORY) return unsupported("LDE_RHS_CVS: no coupled solve; LDE_BATCH_PER_TRAJECTORY only");
    if (d->sensealg != LDE_SENSE_FORWARD_DUAL)
      return unsupported("LDE_RHS_CVS: only the solve on dual numbers exists for this system (no discrete sweep, no continuous adjoint); use LDE_SENSE_FORWARD_DUAL");
  }
  if (is_sl(*d)) {   // … and the Stuart–Landau network, their fourth — and the first with a stochastic solve (k_forward_sde_dir)
    if (d->batching != LDE_BATCH_PER_TRAJECTORY) return unsupported("LDE_RHS_STUART_LANDAU: no coupled solve; LDE_BATCH_PER_TRAJECTORY only");
    if (d->sensealg != LDE_SENSE_FORWARD_DUAL)
      return unsupported("LDE_RHS_STUART_LANDAU: only the solve on dual numbers exists for this system (no discrete sweep, no continuous adjoint); use LDE_SENSE_FORWARD_DUAL");
    if (sde_solver(d->solver)) {   // the conditions of LDE_RHS_SPENDULUM
      if (d->adaptive) return unsupported("LDE_RHS_STUART_LANDAU: no adaptive stochastic stepping; pass adaptive=0, dt=h with LDE_SOLVER_EM / LDE_SOLVER_EULER_HEUN");
      if (!(d->dt > 0) || !std::isfinite(d->dt)) return unsupported("LDE_RHS_STUART_LANDAU: the stochastic steppers are fixed-step; pass a finite dt > 0");
    }
  }
  if (d->solver == LDE_SOLVER_RK4 && d->adaptive) {
    if (why) *why = "RK4 is fixed-step only here: pass adaptive=0, dt=h";
    return LDE_ERR_UNSUPPORTED;
  }
  if (!d->adaptive && !(d->dt > 0)) return bad("adaptive=0 needs dt>0");
  if (d->adaptive && (!(d->abstol > 0) || !(d->reltol > 0))) return bad("tolerances must be > 0");
  if (d->maxiters < 1) return bad("maxiters < 1");
  if (!(d->qmin > 0) || !(d->qmax > 0) || !(d->gamma > 0)) return bad("controller constants must be > 0");
  if (d->sensealg == LDE_SENSE_FORWARD_DUAL) {   // the dual-number solve is served for the GOKU path only (include/lde.h)
    if (has_mlp(*d)) {
      if (why) *why = "LDE_SENSE_FORWARD_DUAL: no MLP right-hand side (the weights would be thousands of partials); analytic right-hand sides only";
      return LDE_ERR_UNSUPPORTED;
    }
    if (d->batching != LDE_BATCH_PER_TRAJECTORY) {
      if (why) *why = "LDE_SENSE_FORWARD_DUAL: no coupled solve; LDE_BATCH_PER_TRAJECTORY only";
      return LDE_ERR_UNSUPPORTED;
    }
  }
  return LDE_OK;
}


static int rec_nseq(const lde_problem_desc& d, int B) { return d.batching == LDE_BATCH_PER_TRAJECTORY ? B : 1; }
// accepted steps a record holds per sequence: the "record_capacity" option, else max(64, 4T) (forward) / max(256, 16T) (reverse-time trace), never more than maxiters
static int rec_capacity(const lde_problem_desc& d, int opt_record_capacity, int T, int which) {
  if (opt_record_capacity > 0) return opt_record_capacity;
  const int64_t c = which == 0 ? std::max<int64_t>(64, 4 * (int64_t)T) : std::max<int64_t>(256, 16 * (int64_t)T);
  return (int)std::min<int64_t>(c, std::max<int64_t>(1, d.maxiters));
}
static size_t align256(size_t x) { return (x + 255) & ~size_t(255); }
// layout: n [nseq] | t [cap][nseq] | dt [cap][nseq] | y [cap][B][D'] (forward records only)
static size_t rec_bytes(const lde_problem_desc& d, int B, int cap, bool with_y) {
  const size_t nseq = (size_t)rec_nseq(d, B), Dp = (size_t)(d.state_dim + d.augment_dim);
  return align256(nseq * 4) + 2 * align256((size_t)cap * nseq * 8) + (with_y ? align256((size_t)cap * B * Dp * 4) : 0);
}
static StepRec rec_view(const lde_problem_desc& d, void* base, int B, int cap, bool with_y) {
  StepRec r{};
  const size_t nseq = (size_t)rec_nseq(d, B);
  unsigned char* p = (unsigned char*)base;
  r.n = (int32_t*)p; p += align256(nseq * 4);
  r.t = (double*)p; p += align256((size_t)cap * nseq * 8);
  r.dt = (double*)p; p += align256((size_t)cap * nseq * 8);
  r.y = with_y ? (float*)p : nullptr;
  r.cap = cap;
  r.nseq = (int)nseq;
  return r;
}

// LDE_SENSE_FORWARD_DUAL's record (include/lde.h: "the dual record"): n [B] | J [T][2][NP][B] f32 | with the step trace t, dt [cap][B] f64;
// `np` = NP = D + P partials per component — 3 for the pendulums (the four-argument forms), 6 for Lotka–Volterra (dual_partials).
// J first: its place depends on B alone, so the pullback (which reads n and J) finds it whether or not the forward traced its steps.
// The record of the lane-per-direction kernels' systems is its own (include/lde.h: "the Kuramoto system", "the double pendulum", "the cardiovascular system"): n [B] |
// J [T][D][B][G] f32 | t, dt — a trajectory's G lanes (dir_group_width) fastest, so D·G floats per (save time, trajectory) where the
// two-state systems have 2·NP; `np` is then D·G/2 (G is even; 16 for the double pendulum and for CVS), and every size and offset below serves these
// kinds unchanged.
static int dual_partials(const lde_problem_desc& d) {
  if (is_dir(d)) return d.state_dim * dir_group_width(d) / 2;   // (0 where the kind does not serve state_dim)
  return is_lv(d) ? 6 : 3;
}
static size_t dual_rec_bytes(int B, int T, int cap, bool trace, int np) {
  return align256((size_t)B * 4) + align256((size_t)T * 2 * np * B * 4) + (trace ? 2 * align256((size_t)cap * B * 8) : 0);
}
static DualRec dual_rec_view(void* base, int B, int T, int cap, bool trace, int np) {
  DualRec r{};
  unsigned char* p = (unsigned char*)base;
  r.n = (int32_t*)p; p += align256((size_t)B * 4);
  r.J = (float*)p; p += align256((size_t)T * 2 * np * B * 4);
  r.t = trace ? (double*)p : nullptr; p += trace ? align256((size_t)cap * B * 8) : 0;
  r.dt = trace ? (double*)p : nullptr;
  r.cap = trace ? cap : 0;
  return r;
}
static size_t dual_rec_bytes(int B, int T, int cap, bool trace) { return dual_rec_bytes(B, T, cap, trace, 3); }
static DualRec dual_rec_view(void* base, int B, int T, int cap, bool trace) { return dual_rec_view(base, B, T, cap, trace, 3); }

// Number of floats in the flat weight vector implied by desc (0 for analytic right-hand sides; n_layers clamped to the struct's capacity)
static int64_t num_weights(const lde_problem_desc* d) {
  if (!d || !has_mlp(*d)) return 0;
  int64_t n = 0;
  for (int l = 0; l < d->n_layers && l < LDE_MAX_LAYERS; l++)
    n += (int64_t)d->layer_sizes[l + 1] * d->layer_sizes[l] + d->layer_sizes[l + 1];
  return n;
}

// ts must be finite and strictly increasing
static bool grid_ok(const double* ts, int T) {
  for (int j = 0; j < T; j++)
    if (!std::isfinite(ts[j]) || (j && !(ts[j] > ts[j - 1]))) return false;
  return true;
}

// a fixed-step solve's number of step attempts over the grid (0: adaptive — unknown here)
static int64_t fixed_step_count(const lde_problem_desc& d, const double* ts, int T) {
  if (d.adaptive || !(d.dt > 0)) return 0;
  int64_t steps = 0;
  for (int j = 0; j + 1 < T; j++) {
    const double n = std::ceil((ts[j + 1] - ts[j]) / d.dt * (1.0 - 1e-12));
    steps += n < 1 ? 1 : (n > 1e9 ? (int64_t)1e9 : (int64_t)n);
    if (steps > d.maxiters) return d.maxiters;
  }
  return steps > d.maxiters ? d.maxiters : steps;
}

// The substep plan of the stochastic pendulum's solve over a save grid (include/lde.h: "the substep rule"): N = Σ_j n_j with n_j =
// lde::sde_substeps(ts[j] − ts[j−1], dt) — the function the kernel's loop calls — capped at maxiters. `over`: the plan is longer than
// maxiters, every trajectory ends with LDE_RET_MAXITERS (the grid is shared). No sum can overflow: n_j ≤ 1e9 and the loop ends at the cap.
struct SdePlan {
  int64_t N;
  bool over;
};
static SdePlan sde_plan(const lde_problem_desc& d, const double* ts, int T) {
  const int64_t cap = std::max<int64_t>(d.maxiters, 0);
  int64_t N = 0;
  for (int j = 1; j < T; j++) {
    N += lde::sde_substeps(ts[j] - ts[j - 1], d.dt);
    if (N > cap) return {cap, true};
  }
  return {N, false};
}

// Which forward mapping of the analytic right-hand sides serves a solve (csrc/lde_pendulum.hip's launch code switches on this; DESIGN.md §4.1;
// the thresholds are measurements: abl/lp_midB.py, abl/pend_B.py, abl/pend_LB.py). `ts_lds_max`: the longest save grid the kernels stage in LDS.
enum PendFwdMap {
  PEND_FWD_LP4 = 0,   // k_pend_forward_lp<REC, 4>: a trajectory per workgroup, lane pairs / Nyström form, four dense-output waves
  PEND_FWD_LP3,       // … three (more than two workgroups per CU)
  PEND_FWD_SH,        // k_pend_forward_sh: a trajectory per workgroup, every other solve (friction, RK4, fixed steps; option "pend_lp" = 0)
  PEND_FWD_TL,        // k_pend_forward_tl<…, 1>: lanes = save times (writes no step record)
  PEND_FWD_WS,        // k_pend_forward_ws: a stepping wave + dense-output waves per 64 trajectories
  PEND_FWD_RING,      // k_pend_forward_tl<…, 64, RING>: a lane per trajectory, ẑ rows through an LDS ring (large batches)
  PEND_FWD_LANE       // k_pend_forward: a lane per trajectory, direct stores
};
static PendFwdMap pend_forward_mapping(int kind, int solver, bool adaptive, bool recording, int B, int T, const lde::PendTune& tn, int ts_lds_max) {
  const bool lp_shape = kind == LDE_RHS_PENDULUM && solver == LDE_SOLVER_TSIT5 && adaptive && tn.lp;
  // option "pend_sh_max_b" ≥ 0: ONE threshold for both mappings with a trajectory per workgroup (what the tests force a mapping with); −1: the measured ones
  const int sh_max_b = tn.sh_max_b >= 0 ? tn.sh_max_b : lp_shape ? 1024 : recording ? 768 : 256;
  if (T > 1 && B <= sh_max_b) return lp_shape ? (B <= 512 ? PEND_FWD_LP4 : PEND_FWD_LP3) : PEND_FWD_SH;
  if (!recording && T > 1 && B <= tn.tl_max_b) return PEND_FWD_TL;
  if (tn.ws != 0 && T <= ts_lds_max && T > 2 && B <= 16384) return PEND_FWD_WS;   // (21.6 against 31.2 µs at 16 384, 36.8 against 32.6 at 32 768)
  if (tn.lb_ring > 0 && T > 1 && T <= 2048 && B >= tn.lb_min_b) return PEND_FWD_RING;
  return PEND_FWD_LANE;
}

// PEND_FWD_TL with at most 64 save intervals: a lane serves exactly one save time (the variant without a load in the stepping loop)
static bool pend_tl_one_save_per_lane(int T) { return T - 1 <= 64; }

// The row ring of PEND_FWD_RING (options "pend_lb" = rows: 8 / 16 / 32, "pend_lb_hold" = the hold margin, −1: half the ring); a recording
// forward has the 16-row ring. A lane sits out while j ≥ jc + rows − hold; the slowest lane has j = jc, so hold ≤ rows − 1 keeps it (and
// with it jc) moving — hold ≥ rows would hold EVERY lane on every iteration and the solve loop would never end.
struct PendRing {
  int rows, hold;
};
static PendRing pend_ring_shape(bool recording, const lde::PendTune& tn) {
  const int rows = recording ? 16 : tn.lb_ring >= 32 ? 32 : tn.lb_ring >= 16 ? 16 : 8;
  return {rows, std::max(0, std::min(tn.lb_hold >= 0 ? tn.lb_hold : rows / 2, rows - 1))};
}

// Which pullback of the analytic right-hand sides serves an lde_adjoint (csrc/lde_pendulum.hip's launch code switches on this; DESIGN.md
// §4.2). LDE_SENSE_FORWARD_DUAL has a pullback of its own (csrc/lde_dual.hip).
enum PendAdjMap {
  PEND_ADJ_SEQ = 0,   // k_pend_adjoint: a lane per trajectory, the reverse-time solve (LDE_SENSE_BACKSOLVE[_CHECKPOINTED])
  PEND_ADJ_FUSED,     // k_pend_adjoint_fused: a workgroup per trajectory, a lane per save interval, the interval operators composed in a tree
  PEND_ADJ_STREAM,    // k_pend_adjoint_stream: a lane per trajectory, interval by interval (large batches, long save grids)
  PEND_ADJ_DISC_TP,   // k_pend_adjoint_disc_tp: LDE_SENSE_DISCRETE, a wave per trajectory, the recorded steps side by side
  PEND_ADJ_DISC       // k_pend_adjoint_disc: LDE_SENSE_DISCRETE, a lane per trajectory
};
static PendAdjMap pend_adjoint_mapping(int sensealg, int B, int T, const lde::PendTune& tn) {
  // a wave per trajectory while the chip has waves to spare (option "pend_disc_tp_max_b"); 16·T + 3 168 bytes of LDS: within the 64 KB a
  // launch gets without asking
  if (sensealg == LDE_SENSE_DISCRETE) return T > 1 && T <= 3840 && B <= tn.disc_tp_max_b ? PEND_ADJ_DISC_TP : PEND_ADJ_DISC;
  // measured (abl/adj_B.py): fused 9.5 µs vs stream 39 µs at 4096, 48 vs 41 µs at 32768
  if (sensealg == LDE_SENSE_PARALLEL_CHECKPOINTED) return T > 1 && T - 1 <= 1024 && B <= 24576 ? PEND_ADJ_FUSED : PEND_ADJ_STREAM;
  return PEND_ADJ_SEQ;
}

// The template arguments of the analytic right-hand sides' kernels: calls f(KIND, SOLVER, ADAPT) with std::integral_constants for exactly
// the six combinations validate() admits — two right-hand sides × {Tsit5 adaptive, Tsit5 fixed-step, RK4 fixed-step} — and returns what f
// returns; anything else is LDE_ERR_UNSUPPORTED. Kernels without an ADAPT parameter ignore the third argument.
template <int KIND, class F>
static int pend_dispatch_solver(int solver, bool adaptive, F& f) {
  using K = std::integral_constant<int, KIND>;
  using TSIT5 = std::integral_constant<int, LDE_SOLVER_TSIT5>;
  if (solver == LDE_SOLVER_TSIT5) return adaptive ? f(K{}, TSIT5{}, std::true_type{}) : f(K{}, TSIT5{}, std::false_type{});
  if (solver == LDE_SOLVER_RK4 && !adaptive) return f(K{}, std::integral_constant<int, LDE_SOLVER_RK4>{}, std::false_type{});
  return LDE_ERR_UNSUPPORTED;
}
template <class F>
static int pend_dispatch(int kind, int solver, bool adaptive, F&& f) {
  if (kind == LDE_RHS_PENDULUM) return pend_dispatch_solver<LDE_RHS_PENDULUM>(solver, adaptive, f);
  if (kind == LDE_RHS_PENDULUM_FRICTION) return pend_dispatch_solver<LDE_RHS_PENDULUM_FRICTION>(solver, adaptive, f);
  return LDE_ERR_UNSUPPORTED;
}

// The template arguments of k_forward_dual (csrc/lde_dual.hip) for Lotka–Volterra: calls f(SOLVER) with a std::integral_constant for exactly
// the three (solver, adaptive) combinations validate() admits for LDE_RHS_LOTKA_VOLTERRA — Tsit5 adaptive, Tsit5 fixed-step, RK4 fixed-step
// (the kernel reads `adaptive` at run time) — and returns what f returns; anything else is LDE_ERR_UNSUPPORTED. A dispatch of its own:
// pend_dispatch serves the pendulums' six combinations and nothing else; the two meet in launch_forward_dual's one launch lambda.
template <class F>
static int lv_dispatch(int solver, bool adaptive, F&& f) {
  if (solver == LDE_SOLVER_TSIT5) return f(std::integral_constant<int, LDE_SOLVER_TSIT5>{});
  if (solver == LDE_SOLVER_RK4 && !adaptive) return f(std::integral_constant<int, LDE_SOLVER_RK4>{});
  return LDE_ERR_UNSUPPORTED;
}

// The template arguments of k_forward_dual_dir (csrc/lde_dual_dir.hip): calls f(N, SOLVER) with std::integral_constants for N = 2 … 7 and
// the three (solver, adaptive) combinations of lv_dispatch — what validate() admits for LDE_RHS_KURAMOTO — and returns what f returns;
// anything else is LDE_ERR_UNSUPPORTED. dir_dispatch_n alone serves the pullback, which has no solver.
template <class F>
static int dir_dispatch_n(int N, F&& f) {
  switch (N) {
    case 2: return f(std::integral_constant<int, 2>{});
    case 3: return f(std::integral_constant<int, 3>{});
    case 4: return f(std::integral_constant<int, 4>{});
    case 5: return f(std::integral_constant<int, 5>{});
    case 6: return f(std::integral_constant<int, 6>{});
    case 7: return f(std::integral_constant<int, 7>{});
    default: return LDE_ERR_UNSUPPORTED;
  }
}
template <class F>
static int dir_dispatch(int N, int solver, bool adaptive, F&& f) {
  return dir_dispatch_n(N, [&](auto n) -> int { return lv_dispatch(solver, adaptive, [&](auto S) -> int { return f(n, S); }); });
}
// … over the system: f(KIND, D) / f(KIND, D, SOLVER) with (LDE_RHS_KURAMOTO, N = 2 … 7) or (LDE_RHS_DOUBLE_PENDULUM, 4) — the one dispatch
// behind the one forward and the one pullback launcher; any other kind or state_dim is LDE_ERR_UNSUPPORTED.
template <class F>
static int dir_dispatch_n(const lde_problem_desc& d, F&& f) {
  if (is_kuramoto(d)) return dir_dispatch_n(d.state_dim, [&](auto n) -> int { return f(std::integral_constant<int, LDE_RHS_KURAMOTO>{}, n); });
  if (is_dpend(d) && d.state_dim == DPEND_D) return f(std::integral_constant<int, LDE_RHS_DOUBLE_PENDULUM>{}, std::integral_constant<int, DPEND_D>{});
  return LDE_ERR_UNSUPPORTED;
}
template <class F>
static int dir_dispatch(const lde_problem_desc& d, F&& f) {
  return dir_dispatch_n(d, [&](auto kind, auto n) -> int {
    return lv_dispatch(d.solver, d.adaptive != 0, [&](auto S) -> int { return f(kind, n, S); });
  });
}
// … and with (LDE_RHS_CVS, 4), the third system: what the launchers call. A layer of its own and not one more branch above, because
// tests/dpend_host_driver.cpp hands the two-system forms a functor that static_asserts the pairs it may be instantiated with — a third
// pair there would stop that driver from compiling, and it stays as it is.
template <class F>
static int dir_system_dispatch_n(const lde_problem_desc& d, F&& f) {
  if (is_cvs(d)) return d.state_dim == CVS_D ? f(std::integral_constant<int, LDE_RHS_CVS>{}, std::integral_constant<int, CVS_D>{}) : (int)LDE_ERR_UNSUPPORTED;
  return dir_dispatch_n(d, f);
}
template <class F>
static int dir_system_dispatch(const lde_problem_desc& d, F&& f) {
  return dir_system_dispatch_n(d, [&](auto kind, auto n) -> int {
    return lv_dispatch(d.solver, d.adaptive != 0, [&](auto S) -> int { return f(kind, n, S); });
  });
}
// … and with (LDE_RHS_STUART_LANDAU, D = 2, 4, 6), the fourth system: what the launchers call now. Once more a layer of its own:
// tests/cvs_host_driver.cpp hands dir_system_dispatch(_n) a functor that static_asserts the three systems' pairs. dir_all_dispatch serves the
// deterministic solves (Tsit5 adaptive, Tsit5 fixed-step, RK4 fixed-step: lv_dispatch); a stochastic solver is LDE_ERR_UNSUPPORTED here.
template <class F>
static int dir_all_dispatch_n(const lde_problem_desc& d, F&& f) {
  if (is_sl(d)) {
    using K = std::integral_constant<int, LDE_RHS_STUART_LANDAU>;
    switch (d.state_dim) {
      case 2: return f(K{}, std::integral_constant<int, 2>{});
      case 4: return f(K{}, std::integral_constant<int, 4>{});
      case 6: return f(K{}, std::integral_constant<int, 6>{});
      default: return LDE_ERR_UNSUPPORTED;
    }
  }
  return dir_system_dispatch_n(d, f);
}
template <class F>
static int dir_all_dispatch(const lde_problem_desc& d, F&& f) {
  return dir_all_dispatch_n(d, [&](auto kind, auto n) -> int {
    return lv_dispatch(d.solver, d.adaptive != 0, [&](auto S) -> int { return f(kind, n, S); });
  });
}
// The template arguments of k_forward_sde_dir (csrc/lde_dual_dir.hip): f(D, SOLVER) for the Stuart–Landau network's D = 2, 4, 6 × {LDE_SOLVER_EM,
// LDE_SOLVER_EULER_HEUN} with adaptive = 0 — what validate() admits for the stochastic solve — and nothing else.
template <class F>
static int dir_sde_dispatch(const lde_problem_desc& d, F&& f) {
  if (!is_dir_sde(d) || d.adaptive) return LDE_ERR_UNSUPPORTED;
  auto with_solver = [&](auto n) -> int {
    if (d.solver == LDE_SOLVER_EM) return f(n, std::integral_constant<int, LDE_SOLVER_EM>{});
    return f(n, std::integral_constant<int, LDE_SOLVER_EULER_HEUN>{});
  };
  switch (d.state_dim) {
    case 2: return with_solver(std::integral_constant<int, 2>{});
    case 4: return with_solver(std::integral_constant<int, 4>{});
    case 6: return with_solver(std::integral_constant<int, 6>{});
    default: return LDE_ERR_UNSUPPORTED;
  }
}

// Which mapping serves a solve under LDE_SENSE_FORWARD_DUAL (csrc/lde_dual.h: dual_block switches on this, for every system and for the
// stochastic pendulum). Kept apart from pend_forward_mapping, whose seven results tests/host_logic_driver.cpp pins: the dual solve has ONE
// mapping, a lane per trajectory (two values and their partials in registers), and the batch only sizes its workgroups — a wave each up to
// 4 096 trajectories (one wave per CU as long as there are CUs to spare), four waves beyond.
enum PendDualMap {
  PEND_DUAL_LANE64 = 0,   // k_forward_dual / k_pend_forward_sde, 64-lane workgroups
  PEND_DUAL_LANE256       // … 256-lane workgroups
};
static PendDualMap pend_dual_mapping(int B) { return B <= 4096 ? PEND_DUAL_LANE64 : PEND_DUAL_LANE256; }

// ---- the MLP right-hand sides: which kernel family serves a solve / an lde_adjoint (csrc/lde_mlp.hip's launch code switches on this;
// DESIGN.md §4.3 – §4.5). The values are what option "adjoint_family" and lde_last_kernel report. Every threshold is a measurement on the
// MI355X (abl/, profiles/) or a residency limit of the 256 CUs; the LDS bytes arrive as numbers (lde::MlpLds).
enum MlpFamily {
  MLP_TILES = 0,     // k_mlp_forward / k_mlp_adjoint / k_mlp_adjoint_disc: 16 trajectories per workgroup on MFMA tiles, the weight gradient from the
                     // staged panels (k_mlp_dw). Serves whatever nothing below takes.
  MLP_64 = 1,        // k_mlp64: a wave per trajectory, everything in registers (three layers ≤ 64 wide, D′ ≤ 4, per-trajectory control)
  MLP_B = 2,         // k_mlpb: four waves per trajectory, W₂ as register blocks, the weight gradient folded on the CU (H ≤ 200, D′ ≤ 16)
  MLP_C = 3,         // k_mlpc: two trajectories per workgroup on one register copy of the weights (H ≤ 128, D′ ≤ 32, coupled control)
  MLP_W = 4,         // k_mlpw: 2 / 4 waves per trajectory, weights and state in registers, the weight gradient staged (H ≤ 200, D′ ≤ 32)
  MLP_V = 5,         // k_mlpv: a trajectory per workgroup, lanes = hidden units (every width ≤ 256), staged
  MLP_4 = 6,         // k_mlp4_adjoint: four columns per wave, the weights in LDS (adjoint only; layers up to "mlp4_maxw" wide), staged
  MLP_NOT_SERVED = 7 // LDE_ERR_UNSUPPORTED: *why says which of the two refusals
};
using lde::MlpLds;
using lde::MlpShape;
using lde::MlpTune;

// The shape summary of a validated MLP problem: what the mappings below read, and which families the network fits at all (their register
// and LDS layouts: csrc/lde_mlpv.h, lde_mlpw.h, lde_mlpb.h, lde_mlpc.h).
static MlpShape mlp_shape(const lde_problem_desc& d) {
  MlpShape s;
  s.nL = d.n_layers;
  s.Dp = d.state_dim + d.augment_dim;
  s.P = d.param_dim;
  for (int l = 0; l <= s.nL && l <= LDE_MAX_LAYERS; l++) s.maxw = std::max(s.maxw, d.layer_sizes[l]);
  s.hm = s.nL == 3 ? std::max(d.layer_sizes[1], d.layer_sizes[2]) : 0;
  s.coupled = d.batching == LDE_BATCH_COUPLED || d.batching == LDE_BATCH_COUPLED_GLOBAL;
  s.global = d.batching == LDE_BATCH_COUPLED_GLOBAL;
  s.disc = d.sensealg == LDE_SENSE_DISCRETE;
  // the register families: three Dense layers, no analytic part, no per-trajectory parameters
  const bool reg = s.nL == 3 && d.rhs_kind != LDE_RHS_PENDULUM_PLUS_MLP && s.P == 0 && s.hm >= 1;
  s.w_ok = reg && s.Dp <= 32 && s.hm <= 200;
  s.b_ok = reg && s.Dp <= 16 && s.hm <= 200;
  s.c_ok = reg && s.Dp <= 32 && s.hm <= 128 && s.coupled;
  s.w_waves = s.hm <= 128 ? 2 : 4;
  // k_mlpv: every width ≤ 256; lanes = the widest layer rounded up to a power of two — or, with three layers and a hidden×hidden product
  // of 17 … 128 units that stays in registers, 64 lanes (≤ 64 units) / 256 lanes (two lane groups split K) where that is no fewer
  s.vec_ok = s.maxw <= 256;
  int nt = 64;
  while (nt < s.maxw && nt < 256) nt *= 2;
  const int want = s.hm <= 64 ? 64 : 256;
  s.v_reg = s.nL == 3 && s.hm > 16 && s.hm <= 128 && nt <= want;
  s.v_nt = s.v_reg ? want : nt;
  return s;
}

// one wave per trajectory: measured on the c3 shape — 0.28 + 3.9 ms against 0.61 + 5.8 for the tiles at B = 4096, 0.77 + 10.4 against 2.2 + 12.0 at 16 384
static bool mlp64_serves(const MlpShape& s, const MlpTune& tn, int B) {
  return tn.mlp64 && s.nL == 3 && s.hm <= 64 && s.Dp <= 4 && s.P <= 1 && !s.coupled && B <= 65536;
}
// k_mlp64's adjoint: workgroups of four waves (one per SIMD: the kernel takes more than 256 registers), at most 256 of them; a wave walks
// trajectories b, b + 4·workgroups, … with ONE set of gradient sums, the four waves' sums meet in LDS, so the row workspace has one row per
// workgroup whatever the batch
constexpr int MLP64_NWV = 4;
static int mlp64_adj_waves(int B) {   // = workgroups = rows
  return (int)std::min<int64_t>(((int64_t)B + MLP64_NWV - 1) / MLP64_NWV, 256);
}
// k_mlpb. Option "mlpb": 0 = off (k_mlpw instead: this kernel's parity reference), 2 = also the networks of at most 128 units that k_mlpw's
// two-wave form serves by default; "mlpw" = 0 switches BOTH register families and k_mlpc off (the tests' "tiles" / "mlpv" legs). One
// workgroup per CU (512 registers per lane): 256 trajectories are resident at once; a solve whose workgroups may queue takes a second round.
static bool mlpb_serves(const MlpShape& s, const MlpTune& tn, size_t lds, size_t cap, int B, bool resident) {
  if (!s.b_ok || tn.mlpb == 0 || !tn.mlpw) return false;
  if (s.hm <= 128 && tn.mlpb != 2) return false;
  return lds <= cap && B <= (resident ? 256 : 512);
}
// k_mlpc (k_mlpb's switches). One workgroup = two trajectories per CU: 512 are resident at once.
static bool mlpc_serves(const MlpShape& s, const MlpTune& tn, size_t lds, size_t cap, int B, bool resident) {
  if (!s.c_ok || tn.mlpb == 0 || !tn.mlpw) return false;
  return lds <= cap && B <= (resident ? 512 : 1024);
}
// k_mlpw. 4 / W workgroups share a CU's LDS (one wave per SIMD: the weights take most of the 512 registers), 1024 waves are resident at
// once; an uncoupled solve may queue a second round.
static bool mlpw_serves(const MlpShape& s, const MlpTune& tn, const MlpLds& l, int B, bool resident) {
  if (!s.w_ok || !tn.mlpw || s.w_waves < 1) return false;
  return l.w <= l.cap * (size_t)s.w_waves / 4 && (int64_t)B * s.w_waves <= (resident ? 1024 : 2048);
}
// k_mlpv's LDS per workgroup: everything when a CU gets one workgroup, a share otherwise (the launch code sizes the weight cache with it)
static size_t mlpv_lds_budget(size_t cap, int B) {
  const size_t per_cu = (size_t)std::max<int64_t>(1, ((int64_t)B + 255) / 256);
  const size_t share = cap / per_cu;
  return per_cu > 1 ? share - std::min<size_t>(share, 256) : share;
}
// k_mlpv. Measured (c2 / c3 / c4 shapes): the one-trajectory workgroups win while the chip has a SIMD per wave — B·NT/64 ≤ 1024: c2 0.88 +
// 1.97 ms against 1.77 + 3.44 at B = 256, c3 0.36 + 4.28 against 0.63 + 5.0 at 1024, c4 0.46 + 3.77 against 0.45 + 4.3 at 512 — and lose
// beyond (c2 at B = 1024: 1.94 + 4.5 against 1.78 + 3.9); with the register-resident layer two waves per SIMD still win. Coupled adaptive
// control needs all B workgroups resident: their fixed part must fit the CU's share.
static bool mlpv_serves(const MlpShape& s, const MlpTune& tn, const MlpLds& l, int B, bool resident) {
  if (!s.vec_ok || !tn.mlpv || s.v_nt < 1) return false;
  if (B > (s.v_reg ? 2048 : 1024) * 64 / s.v_nt || l.v_fixed > l.cap / 2) return false;
  return !resident || mlpv_lds_budget(l.cap, B) >= l.v_fixed;
}
// k_mlp4_adjoint. Measured: one wave has ONE SIMD's matrix pipe and v_mfma_f32_4x4x1 costs 11 cycles per 256 MACs (the 16x16x4 form: 8), so
// the kernel only wins while the layers are small enough for the tiles' fixed ≈ 2 000 cycles per layer to dominate: c3 (64 wide) 7.3 → 5.3 ms,
// c4 (128 wide) 4.4 → 5.5 ms — hence "mlp4_maxw" = 64. Grid-wide sums need every workgroup resident.
static bool mlp4_serves(const MlpShape& s, const MlpTune& tn, const MlpLds& l, bool coupled_adaptive) {
  if (!tn.mlp4 || s.Dp > 64 || s.P > 1 || s.maxw > tn.mlp4_maxw || s.maxw > 256) return false;
  return !(coupled_adaptive && l.mlp4_blocks > 256) && l.mlp4 <= l.cap;
}
static MlpFamily mlp_refuse(const char** why, const char* text) {
  if (why) *why = text;
  return MLP_NOT_SERVED;
}
static MlpFamily mlp_refuse_global(const char** why) {
  return mlp_refuse(why, "LDE_BATCH_COUPLED_GLOBAL: this shape / batch is not served by the register kernels (three Dense layers, 2·D' ≤ 64, H ≤ 200, B·W ≤ 1024 waves)");
}
// the coupled adaptive tiles: 256 workgroups of 16 trajectories, one resident per CU, meet in the grid-wide sum
static MlpFamily mlp_refuse_tiles(const char** why) {
  return mlp_refuse(why, "coupled adaptive solve: batch per GPU limited to 4096 trajectories (one resident workgroup per CU)");
}

// The forward solve of B trajectories; `l`: the forward kernels' LDS for this save grid; `recording`: a step record is being written
// (k_mlpw and k_mlpv write none; k_mlp64, k_mlpb, k_mlpc and the tiles do). Precedence as listed. A coupled ADAPTIVE solve of more than one
// trajectory needs every workgroup resident (the grid-wide sum of the step control): that — not "coupled" — halves the limits here.
static MlpFamily mlp_forward_mapping(const MlpShape& s, const MlpTune& tn, const MlpLds& l, int B, bool adaptive, bool recording, const char** why = nullptr) {
  if (mlp64_serves(s, tn, B)) return MLP_64;
  const bool ca = s.coupled && adaptive && B > 1;
  if (mlpb_serves(s, tn, l.b, l.cap, B, ca)) return MLP_B;
  if (mlpc_serves(s, tn, l.c, l.cap, B, ca)) return MLP_C;
  if (!recording && mlpw_serves(s, tn, l, B, ca)) return MLP_W;
  if (s.global) return mlp_refuse_global(why);   // only the register kernels exchange their sums across ranks
  if (!recording && mlpv_serves(s, tn, l, B, ca)) return MLP_V;
  if (s.coupled && adaptive && B > 4096) return mlp_refuse_tiles(why);
  return MLP_TILES;
}

// lde_adjoint on B trajectories; `l`: the adjoint kernels' LDS for this save grid. Precedence as listed. Three different readings of
// "coupled", each as measured / as the kernel needs it:
//  · the continuous adjoint of k_mlpb / k_mlpc takes the resident limits (256 / 512) for EVERY coupled solve, fixed-step ones included —
//    where the forward (above) takes them for adaptive ones only: a coupled fixed-step 8-200-200-8 solve at B = 300 runs forward on k_mlpb
//    and backward on k_mlpw;
//  · k_mlpw, k_mlpv: coupled && adaptive && B > 1, as in the forward; k_mlp4_adjoint: coupled && adaptive;
//  · LDE_SENSE_DISCRETE sweeps a record without step control, hence without a grid-wide sum: workgroups may queue, and the register
//    kernels take the shapes of the continuous adjoint (its LDS test at a batch within the limit) up to what a row of the workspace per
//    workgroup costs in memory — B ≤ 1024 (k_mlpb) / 2048 (k_mlpc) — and what their sweeps' LDS allows; everything else runs on the tiles,
//    and nothing is refused.
static MlpFamily mlp_adjoint_mapping(const MlpShape& s, const MlpTune& tn, const MlpLds& l, int B, bool adaptive, const char** why = nullptr) {
  if (mlp64_serves(s, tn, B)) return MLP_64;
  if (s.disc) {
    if (mlpb_serves(s, tn, l.b, l.cap, std::min(B, 256), false) && B <= 1024 && l.b_disc <= l.cap) return MLP_B;
    if (mlpc_serves(s, tn, l.c, l.cap, std::min(B, 512), false) && B <= 2048 && l.c_disc <= l.cap) return MLP_C;
    return MLP_TILES;
  }
  if (mlpb_serves(s, tn, l.b, l.cap, B, s.coupled)) return MLP_B;
  if (mlpc_serves(s, tn, l.c, l.cap, B, s.coupled)) return MLP_C;
  if (s.coupled && adaptive && B > 4096) return mlp_refuse_tiles(why);   // (the tile kernel runs behind the three staged families below)
  const bool ca = s.coupled && adaptive && B > 1;
  if (mlpw_serves(s, tn, l, B, ca)) return MLP_W;
  if (s.global) return mlp_refuse_global(why);
  if (mlpv_serves(s, tn, l, B, ca)) return MLP_V;
  if (mlp4_serves(s, tn, l, s.coupled && adaptive)) return MLP_4;
  return MLP_TILES;
}

// The adjoint's workspace follows from its family: k_mlp64, k_mlpb and k_mlpc fold the weight gradient in the solve kernel and leave rows
// of it for k_sum_rows; every other family stages panels for k_mlp_dw. Rows the family WRITES for a batch (0: the staging area) …
static int mlp_adjoint_rows(MlpFamily f, int B) {
  return f == MLP_64 ? mlp64_adj_waves(B) : f == MLP_B ? B : f == MLP_C ? (int)(((int64_t)B + 1) / 2) : 0;
}
// … and rows lde_reserve sizes for it (k_mlpc: per trajectory). lde_reserve knows the batch and the grid but not the call: it asks the
// mapping with adaptive = false — the three row families do not depend on `adaptive`
static int mlp_reserved_rows(MlpFamily f, int B) {
  return f == MLP_64 ? mlp64_adj_waves(B) : (f == MLP_B || f == MLP_C) ? B : 0;
}

// The template argument of the MLP kernels: calls f(SOLVER) with a std::integral_constant for the two solvers validate() admits and
// returns what f returns; anything else is LDE_ERR_UNSUPPORTED.
template <class F>
static int mlp_dispatch(int solver, F&& f) {
  if (solver == LDE_SOLVER_TSIT5) return f(std::integral_constant<int, LDE_SOLVER_TSIT5>{});
  if (solver == LDE_SOLVER_RK4) return f(std::integral_constant<int, LDE_SOLVER_RK4>{});
  return LDE_ERR_UNSUPPORTED;
}

// ---- the dense chains (csrc/lde_chain.hip's launch code asks these): tile widths, the layout of a call, the split of the
// weight-gradient product. A tile is 16·cg columns (cg column groups); the thresholds are measurements on the MI355X.
using lde::ChainLdsDims;

// LDS bytes of a tile kernel: f32 — the input panel, 2 (forward) / 3 (pullback) hidden panels and the biases; bf16 forward — two bf16
// panels (the input panel shares the second one's space), a third with skip layers, the biases, the chunk buffers of a wide input read
// in place; bf16 pullback — two bf16 panels and the f32 skip-gradient panel.
static size_t chain_lds_bytes(const ChainLdsDims& q, bool bf16, bool bwd, int cg) {
  const size_t NC = 16 * (size_t)cg, bias = ((size_t)q.nbias + 3) & ~size_t(3);
  if (!bf16) return (NC * q.ld0 + (bwd ? 3 : 2) * NC * q.ldh + bias) * sizeof(float);
  if (bwd) return NC * q.ldb * 2 * 2 + NC * q.ldg * 4;
  return (2 + (q.fpanel ? 1 : 0)) * NC * q.ldb * 2 + bias * 4 + (size_t)cg * q.xs_per_cg;
}

// Column groups per workgroup, chosen once per handle: the widest tile that still lets TWO workgroups share a CU (half the LDS each) —
// one tile's barrier / prologue latencies are then covered by the other's MFMAs. Measured on the reconstructor (N = 12800): f32 forward
// 64 columns 110 µs, 32 columns 107 µs; pullback 32 columns 331 µs, 16 columns 313 µs. Falls back to the widest tile that fits at all;
// 0: none does. Candidates: 4, 2, 1 for the f32 forward; 2, 1 for the f32 pullback and for bf16 (≤ 128 registers: csrc/lde_chain_bf16.h —
// a 64-column bf16 forward instantiation exists and is never picked here).
static int chain_tile_pick(const ChainLdsDims& q, bool bf16, bool bwd, size_t lds_max) {
  for (size_t lim : {lds_max / 2, lds_max})
    for (int cg = (bf16 || bwd) ? 2 : 4; cg >= 1; cg /= 2)
      if (chain_lds_bytes(q, bf16, bwd, cg) <= lim) return cg;
  return 0;
}

// workgroups of a tile kernel = its grid (0 only for N < 1, which every entry point refuses)
static int64_t chain_tiles(int64_t N, int cg) { return N < 1 ? 0 : (N - 1) / (16 * (int64_t)std::max(cg, 1)) + 1; }

// Mid-size batches (a training step's N = B·T ≈ 3 200 columns): the widest tile leaves most CUs without a workgroup — 50–100 tiles on
// 256 CUs — and a tile's time barely depends on its width (the weight fragments stream through the workgroup either way). Narrow the tile
// until the grid has ≈ 200 workgroups (measured, GOKU training step at B = 64: 1.70 → 1.32 ms and 2.17 → 1.84 ms in two back-to-back
// pairs; at B = 256 the grids are full and nothing changes).
static int chain_narrow(int64_t N, int cg0) {
  int g = std::max(cg0, 1);
  while (g > 1 && chain_tiles(N, g) < 192) g /= 2;
  return g;
}

// Which layout a call uses: the panel-free one (x[in×N] itself is the first layer's B operand; `cgx` column groups, 0: the chain has
// none) when N fills one of its tiles and x is 16-byte aligned, else the one with an input panel (`cg`, 0: its panels do not fit) — and
// the call's tile width.
enum ChainLayout { CHAIN_NONE = 0, CHAIN_PANEL, CHAIN_GX };
struct ChainChoice {
  ChainLayout layout;
  int cg;
};
static ChainChoice chain_call_choice(int cgx, int cg, int64_t N, bool x_aligned) {
  if (cgx > 0 && N >= 16 * (int64_t)cgx && x_aligned) return {CHAIN_GX, chain_narrow(N, cgx)};
  if (cg > 0) return {CHAIN_PANEL, chain_narrow(N, cg)};
  return {CHAIN_NONE, 0};
}

// The f32 weight gradient: k_mlp_dw sees the pullback's staged 16-column slots (`total`: every tile brings cg of them) as `nvt` virtual
// tiles of `cap` slots; (virtual tiles × jobs) ≈ one workgroup per CU — the kernel's register footprint allows one resident workgroup per
// CU, so 256 equal shares beat 384 (a second, half-empty round).
struct ChainDwSplit {
  int nvt, cap;
  int64_t total;
};
static ChainDwSplit chain_dw_split(int jobs, int cg, int64_t N) {
  ChainDwSplit s;
  s.total = chain_tiles(N, cg) * std::max(cg, 1);
  const int64_t v = std::max<int64_t>(1, std::min<int64_t>(std::max(256 / std::max(jobs, 1), 1), s.total));
  s.nvt = (int)v;
  s.cap = (int)std::min<int64_t>(std::max<int64_t>((s.total + v - 1) / v, 1), std::numeric_limits<int>::max());
  return s;
}
// … and the bf16 one: k_chain_dw_b splits the N rows of its operands into `parts` K-ranges of whole `chunk`-row chunks, by the same rule
static int chain_dw_parts_bf16(int jobs, int64_t N, int chunk) {
  const int64_t nchunks = N < 1 ? 1 : (N - 1) / std::max(chunk, 1) + 1;
  return (int)std::min<int64_t>(std::max(256 / std::max(jobs, 1), 1), nchunks);
}

// ---- the GRU cell of the recurrent pattern extractor (LDE_CELL_GRU; csrc/lde_rnn_gru.h): the pure part of its plan.
// The kernels run a cell of h units as P = 4h PSEUDO-ROWS of [Wi | Wh] over K = in + h columns — (r, z, n_x, n_h), h rows each: n_x is
// [Wi₃ | 0] with the bias, n_h is [0 | Wh₃] without one — and the weight-gradient product leaves vec of that [P × K] matrix, column-major,
// then its P bias sums. The flat (Flux.destructure) order of the cell is vec(Wi) [3h × in], vec(Wh) [3h × h], b [3h], state0 [h].
constexpr int GRU_MAX_H = 64, GRU_MAX_IN = 256;   // the limits lde_rnn_create states for every cell kind
static bool gru_dims_ok(int64_t in, int64_t h) { return in >= 1 && h >= 1 && in <= GRU_MAX_IN && h <= GRU_MAX_H; }
static int gru_rows(int h) { return h >= 1 && h <= GRU_MAX_H ? 4 * h : 0; }
// lanes per trajectory: one per pseudo-row of the widest cell, a power of two, at most a wave (a trajectory never leaves its wave) …
static int gru_lanes(int hmax) {
  int Hp = 1;
  while (Hp < gru_rows(hmax) && Hp < 64) Hp <<= 1;
  return Hp;
}
// … and the pseudo-rows a lane owns then: rows u, u + lanes, … (1 up to h = 16; 4 at h = 64)
static int gru_rows_per_lane(int h, int lanes) { return lanes >= 1 ? (gru_rows(h) + lanes - 1) / lanes : 0; }
// floats of one cell in the flat weight vector (−1: sizes outside the limits), and of one (step, trajectory) training record per unit
// row: r, z, n, Wh₃·h, h′
static int64_t gru_cell_weights(int64_t in, int64_t h) { return gru_dims_ok(in, h) ? 3 * h * in + 3 * h * h + 3 * h + h : -1; }
constexpr int GRU_REC_ROWS = 5;
// offsets of vec(Wh), b and state0 from the cell's start in the flat order
struct GruFlat {
  int64_t wh, b, s0, end;
};
static GruFlat gru_flat_offsets(int64_t in, int64_t h) {
  if (!gru_dims_ok(in, h)) return {-1, -1, -1, -1};
  return {3 * h * in, 3 * h * in + 3 * h * h, 3 * h * in + 3 * h * h + 3 * h, 3 * h * in + 3 * h * h + 3 * h + h};
}
// floats the staged product leaves for one cell: [4h × K] + [4h]
// (0 for sizes outside the limits, here and below: no arithmetic is done on them)
LDE_HD inline bool gru_sizes_ok(int in, int h) { return in >= 1 && h >= 1 && in <= 256 && h <= 64; }
LDE_HD inline long long gru_staged_floats(int in, int h) { return gru_sizes_ok(in, h) ? 4LL * h * (in + h) + 4LL * h : 0; }
// flat entries that come out of the staged product (everything but state0)
LDE_HD inline long long gru_staged_count(int in, int h) { return gru_sizes_ok(in, h) ? 3LL * h * (in + h) + 3LL * h : 0; }
// where flat entry e ∈ [0, gru_staged_count) of the cell sits in the staged result (−1: e or the sizes out of range). One-to-one, and
// never a structural zero of the pseudo-rows (n_x × h columns, n_h × x columns, the bias of n_h).
LDE_HD inline long long gru_staged_index(int in, int h, long long e) {
  if (!gru_sizes_ok(in, h) || e < 0) return -1;
  const long long R = 3LL * h, P = 4LL * h;
  if (e < R * in) {
    const long long k = e / R, r = e - k * R;   // Wi: rows r, z, n → pseudo-rows r, z, n_x
    return k * P + r;
  }
  e -= R * in;
  if (e < R * h) {
    const long long k = e / R, r = e - k * R;   // Wh: rows r, z, n → pseudo-rows r, z, n_h
    return (in + k) * P + (r < 2LL * h ? r : r + h);
  }
  e -= R * h;
  return e < R ? P * (in + h) + e : -1;         // b: pseudo-rows r, z, n_x
}

// ---- the recurrent stacks (csrc/lde_rnn.hip's launch code asks these): weight counts, the LDS / flat-weight layout of a
// stack, which of the four kernel forms serves a call and with what launch shape, the k-split of the weight gradient. Every threshold is a
// measurement on the MI355X.
using lde::RnnDims;
static bool rnn_desc_ok(const lde_rnn_desc* d) {
  if (!d || d->abi_version != LDE_ABI_VERSION || d->n_layers < 1 || d->n_layers > LDE_RNN_MAX_LAYERS) return false;
  if (d->cell < 0 || d->cell > LDE_CELL_GRU) return false;
  for (int l = 0; l <= d->n_layers; l++)
    if (d->sizes[l] < 1) return false;
  return true;
}
// per cell kind: gate rows per unit as the kernels run them (GRU: its four pseudo-rows), gate rows per unit in the flat order, state vectors
static int rnn_gate_rows(int cell) { return cell == LDE_CELL_LSTM || cell == LDE_CELL_GRU ? 4 : 1; }
static int rnn_flat_rows(int cell) { return cell == LDE_CELL_LSTM ? 4 : cell == LDE_CELL_GRU ? 3 : 1; }
static int rnn_state_vectors(int cell) { return cell == LDE_CELL_LSTM ? 2 : 1; }
// floats of one cell in the flat weight vector: vec(Wi) [F·h × in], vec(Wh) [F·h × h], b [F·h], state0 [S·h] (−1: a size < 1, or a count
// beyond int64) …
static int64_t rnn_cell_weights(int cell, int64_t in, int64_t h) {
  if (in < 1 || h < 1 || in > std::numeric_limits<int32_t>::max() || h > std::numeric_limits<int32_t>::max()) return -1;
  const int64_t R = rnn_flat_rows(cell) * h;   // ≤ 2³³
  int64_t n = 0;
  if (__builtin_mul_overflow(R, in + h + 1, &n) || __builtin_add_overflow(n, rnn_state_vectors(cell) * h, &n)) return -1;
  return n;
}
// … and of the stack (−1: not a description)
static int64_t rnn_num_weights(const lde_rnn_desc* d) {
  if (!rnn_desc_ok(d)) return -1;
  int64_t n = 0;
  for (int l = 0; l < d->n_layers; l++) {
    const int64_t c = rnn_cell_weights(d->cell, d->sizes[l], d->sizes[l + 1]);
    if (c < 0 || __builtin_add_overflow(n, c, &n)) return -1;
  }
  return n;
}

// The four kernel forms: the run-time-shaped kernel (any stack), and for the default stacks the compile-time-shaped kernel with its weight
// rows in LDS (any workgroup size) or in registers (one wave per workgroup), and the two-wave pipeline (one wave per cell).
enum RnnForm { RNN_FORM_GENERIC = 0, RNN_FORM_ROWS_LDS, RNN_FORM_ROWS_REG, RNN_FORM_PIPE };
// LDS bytes of a launch with tpw trajectories per workgroup: the weight area, then per trajectory [x; h], the gate deltas and h, c, dh, dc
// of every cell; the pipeline: per (cell, trajectory) the two vectors and 4·16 floats, the two rings of PIPE_R steps, the four counters
static size_t rnn_lds_bytes(const RnnDims& rd, RnnForm form, int tpw) {
  const int64_t t = std::min(std::max(tpw, 0), 64), nL = std::min(std::max(rd.nL, 0), lde::RNN_ML), w = rd.lds_w, v = (int64_t)rd.vmax + rd.rmax;   // (clamped: any RnnDims, no overflow)
  const int64_t fl = form == RNN_FORM_PIPE ? w + 2 * t * (v + 4 * 16) + 2 * lde::PIPE_R * t * 16 + 16 : w + t * (v + 4 * nL * rd.hmax);
  return fl > 0 ? (size_t)fl * sizeof(float) : 0;
}

// The layout of a stack: what the kernels index LDS and the flat weight vector with (lde::RnnDims), floats per trajectory of the initial
// states' gradient (*g0w) and the weight count (*nW). Any description: LDE_ERR_INVALID_ARG for what is none, LDE_ERR_UNSUPPORTED with *why
// for the three limits — checked before any arithmetic on the sizes (beyond them every product below fits an int many times over).
static int rnn_layout(const lde_rnn_desc* d, size_t lds_max, RnnDims* out, int* g0w, int64_t* nW, const char** why = nullptr) {
  auto refuse = [&](const char* m) {
    if (why) *why = m;
    return (int)LDE_ERR_UNSUPPORTED;
  };
  if (!out || !g0w || !nW || !rnn_desc_ok(d)) return LDE_ERR_INVALID_ARG;
  RnnDims& rd = *out;
  rd = RnnDims{};
  *g0w = 0;
  *nW = 0;
  rd.cell = d->cell; rd.nL = d->n_layers; rd.reverse = d->reverse ? 1 : 0; rd.G = rnn_gate_rows(d->cell);
  const bool gru = d->cell == LDE_CELL_GRU;
  int hmax = 0, kmax = 0, rmax = 0;
  for (int l = 0; l <= rd.nL; l++) rd.sizes[l] = d->sizes[l];
  for (int l = 1; l <= rd.nL; l++) hmax = std::max(hmax, d->sizes[l]);
  if (hmax > GRU_MAX_H || d->sizes[0] > GRU_MAX_IN)
    return refuse("recurrent stack: hidden width ≤ 64 and input width ≤ 256 supported (every cell kind, LDE_CELL_GRU included)");
  int Hp = 1;   // lanes per trajectory: one per gate row of the widest cell (≤ 64 ⇒ a trajectory never leaves its wave)
  while (Hp < rd.G * hmax && Hp < 64) Hp <<= 1;
  if (gru) Hp = gru_lanes(hmax);   // (the same rule; above 64 pseudo-rows a lane owns several: gru_rows_per_lane)
  if (!gru && Hp < rd.G * hmax) return refuse("recurrent stack: G·h ≤ 64 gate rows per cell supported (LSTM: h ≤ 16, RNN: h ≤ 64)");
  rd.Hp = Hp;
  rd.hmax = hmax;
  int off = 0;
  int64_t foff = 0;
  for (int l = 0; l < rd.nL; l++) {
    const int in = rd.sizes[l], h = rd.sizes[l + 1], R = rd.G * h, K = in + h;
    rd.K[l] = K;
    rd.ldk[l] = lde::rnn_ldk(K);
    rd.w_off[l] = off; off += R * rd.ldk[l];
    rd.b_off[l] = off; off += (R + 3) & ~3;
    rd.s_off[l] = off; off += (2 * h + 3) & ~3;
    rd.f_off[l] = (int)foff;
    foff += rnn_cell_weights(rd.cell, in, h);
    kmax = std::max(kmax, K);
    rmax = std::max(rmax, R);
    *g0w += rnn_state_vectors(rd.cell) * h;
  }
  rd.vmax = ((kmax + 3) & ~3) + 4;
  rd.rmax = (rmax + 3) & ~3;
  rd.recw = (gru ? GRU_REC_ROWS : rd.G + 2) * hmax;
  rd.lds_w = off;
  for (int l = 0; l < rd.nL; l++) {   // transposed copies for the pullback, when they fit beside everything else at 16 trajectories per workgroup
    rd.ldr[l] = lde::rnn_ldk(rd.G * rd.sizes[l + 1]);
    rd.wt_off[l] = rd.lds_w;
    rd.lds_w += rd.K[l] * rd.ldr[l];
  }
  rd.wt = rnn_lds_bytes(rd, RNN_FORM_GENERIC, 16) <= lds_max ? 1 : 0;
  if (!rd.wt) rd.lds_w = off;
  *nW = foff;
  if (rnn_lds_bytes(rd, RNN_FORM_GENERIC, 16) > lds_max) return refuse("recurrent stack: weights do not fit the 160 KiB LDS");
  return LDE_OK;
}

// the reference's default pattern extractors (32 → 16 → 16, two cells) [REF src/models/GOKU.jl:229-238]: the shape the compile-time forms exist for
static bool rnn_default_shape(const RnnDims& rd) { return rd.wt && rd.nL == 2 && rd.sizes[0] == 32 && rd.sizes[1] == 16 && rd.sizes[2] == 16; }

// One call on B trajectories. Trajectories per workgroup: the sweep is sequential in time and every trajectory re-reads the cell's weights
// from LDS at every step, so a small batch is spread over as many CUs as it has waves (one wave per workgroup: the LDS of a CU then serves
// one wave instead of sixteen); only a batch that would exceed ~4 workgroups per CU (1024) packs more trajectories behind one LDS copy of
// the weights. One wave per workgroup (tpw·Hp = 64) of a default stack runs the register-row form (option "regw"), and by default the
// pipeline, one wave per CELL (option "pipe"; not in an LDE_PROF build). Whole staging tiles of 16 trajectories are covered: rows past B
// write zero panels.
struct RnnPlan {
  RnnForm form;
  int tpw;
  unsigned block, grid;
  size_t lds_bytes;
};
static RnnPlan rnn_launch_plan(const RnnDims& rd, int B, int opt_generic, int opt_regw, int opt_pipe, bool prof) {
  const int Hp = std::min(std::max(rd.Hp, 1), 64);
  const int64_t b = std::max(B, 0);
  RnnPlan p;
  p.tpw = std::max(1, 64 / Hp);
  while (p.tpw < 16 && (b + p.tpw - 1) / p.tpw > 1024) p.tpw *= 2;
  const bool one_wave = p.tpw * Hp == 64 && opt_regw != 0;
  const bool shaped = rnn_default_shape(rd) && opt_generic == 0;
  p.form = !shaped ? RNN_FORM_GENERIC : !one_wave ? RNN_FORM_ROWS_LDS : (!prof && opt_pipe != 0) ? RNN_FORM_PIPE : RNN_FORM_ROWS_REG;
  p.block = p.form == RNN_FORM_PIPE ? 128u : (unsigned)(p.tpw * Hp);
  p.grid = (unsigned)((b + 15) / 16 * (16 / p.tpw));
  p.lds_bytes = rnn_lds_bytes(rd, p.form, p.tpw);
  return p;
}
// a grouped call runs several stacks in one launch of k_rnn_group, which switches between the RNN / LSTM bodies of the two single-wave forms
static bool rnn_groupable(const RnnDims& rd, RnnForm form) {
  return (form == RNN_FORM_ROWS_REG || form == RNN_FORM_PIPE) && rnn_default_shape(rd) && rd.cell != LDE_CELL_GRU;
}
// K-split parts of a cell's weight-gradient product: (staging tiles × jobs × parts) ≈ 512 workgroups, 1 … 8 parts
static int rnn_dw_ksplit(int ntile, int jobs) {
  const int64_t wg = (int64_t)ntile * jobs;
  return wg < 1 ? 8 : (int)std::min<int64_t>(std::max<int64_t>((512 + wg - 1) / wg, 1), 8);
}
// The template arguments of the shaped recurrent kernels: calls f(CELL, MODE) with std::integral_constants for the four cell kinds × the
// four modes (0 forward, 1 pullback, 2 training forward, 3 pullback from kept records) and returns what f returns; anything else is
// LDE_ERR_UNSUPPORTED. rnn_dispatch_mode: the mode alone (k_rnn_group).
template <class F>
static int rnn_dispatch_mode(int mode, F&& f) {
  switch (mode) {
    case 0: return f(std::integral_constant<int, 0>{});
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 3: return f(std::integral_constant<int, 3>{});
  }
  return LDE_ERR_UNSUPPORTED;
}
template <class F>
static int rnn_dispatch(int cell, int mode, F&& f) {
  auto with = [&](auto C) { return rnn_dispatch_mode(mode, [&](auto M) { return f(C, M); }); };
  switch (cell) {
    case LDE_CELL_RNN_RELU: return with(std::integral_constant<int, LDE_CELL_RNN_RELU>{});
    case LDE_CELL_RNN_TANH: return with(std::integral_constant<int, LDE_CELL_RNN_TANH>{});
    case LDE_CELL_LSTM: return with(std::integral_constant<int, LDE_CELL_LSTM>{});
    case LDE_CELL_GRU: return with(std::integral_constant<int, LDE_CELL_GRU>{});
  }
  return LDE_ERR_UNSUPPORTED;
}

// ---- the parameter update (csrc/lde_optim.hip's launch code asks this): which arrays of the caller's t[] travel in which
// launch. A launch carries at most OPT_MAXT NON-EMPTY arrays (its kernel-argument table) and at most 2³⁰ − 1 workgroups; a workgroup owns
// `per_wg` consecutive elements of one array. The update (OPT_PER_WG) and the gradient scan of the guarded step (GUARD_PER_WG: it moves
// 4 bytes per element where the update moves 28) both walk t[] with this function, each with its own slice.
constexpr int OPT_WG = 256;
constexpr int OPT_PER_WG = 8 * OPT_WG;      // the update: two 16-byte accesses per lane and array
constexpr int GUARD_PER_WG = 32 * OPT_WG;   // the scan: eight 16-byte loads per lane, 32 KiB per workgroup — the default GOKU model (2 MB of
                                            // gradients) is 70 workgroups where the update has 252. Measured (abl/guard_time.py):
                                            // at that size a larger slice only lengthens the one workgroup everything waits for — the scan adds
                                            // 3.4 µs at 8 192, 3.7 at 16 384, 4.2 at 32 768, 5.2 at 65 536; at 2²⁶ floats the slice does not matter
constexpr int OPT_MAXT = 48;                // arrays per launch (kernel-argument table: 48 × 40 B)
constexpr int OPT_MAX_BLOCKS = 0x3fffffff;
struct OptLaunch {
  int n;                     // non-empty arrays in this launch (0: nothing left to launch)
  int idx[OPT_MAXT];         // their indices in the caller's t[]
  int blk0[OPT_MAXT + 1];    // first workgroup of each; blk0[n] = the grid
  int next;                  // where the following launch starts in t[]
  bool last;                 // no array after `next` has elements: the step's last launch
  bool too_large;            // n == 0 because t[next] alone needs more than OPT_MAX_BLOCKS workgroups (the caller refuses the call)
};
static OptLaunch opt_next_launch(int n, const lde_adam_tensor* t, int first, int per_wg) {
  OptLaunch L{};
  int blk = 0;
  while (first < n && L.n < OPT_MAXT) {
    if (t[first].n > 0) {
      const int64_t nb = (t[first].n - 1) / per_wg + 1;
      if (nb > OPT_MAX_BLOCKS - blk) break;   // next launch
      L.idx[L.n] = first;
      L.blk0[L.n] = blk;
      blk += (int)nb;
      L.n++;
    }
    first++;
  }
  L.blk0[L.n] = blk;
  L.next = first;
  L.too_large = L.n == 0 && first < n;
  bool more = false;   // another launch follows? (only the step's last one advances the count)
  for (int j = first; j < n; j++) more = more || t[j].n > 0;
  L.last = !more;
  return L;
}

// ---- the workspace of the clipped step (lde_adamw_flux_step_clipped, include/lde.h: "the clipped step"): what the norm scan leaves for
// the finalising kernel and the finalising kernel for the update. The scan walks t[] with opt_next_launch at GUARD_PER_WG, so its workgroups
// — launch after launch, workgroup after workgroup — meet the non-empty arrays in the caller's order, each array's slices side by side.
// One f64 partial per scan workgroup in THAT order: array L.idx[i] of a launch with slot base s owns slots [s + L.blk0[i], s + L.blk0[i+1]).
// The non-empty arrays are numbered 0 … nne − 1 in the caller's order ("ordinals": the update's launches, whose packing may differ from the
// scan's, meet them in the same order); per ordinal the workspace holds the array's Σg² (f64, the finalising kernel's), its descriptor
// (written by the scan workgroup that owns the array's first slice: the table of a launch travels in kernel arguments, the finalising
// kernel sees every launch's arrays) and its scale (f32).
//     [0, 8·slots) partials | [off_sums, +8·nne) | [off_desc, +16·nne) | [off_scale, +4·nne)              (ws_dev: 8-byte aligned)
// `on_launch(L, slot0, ord0)` is called once per scan launch; lde_clip_ws_bytes passes one that does nothing.
struct ClipDesc {
  int64_t slot0;    // the array's first partial
  int32_t nslots;   // its scan workgroups
  int32_t idx;      // its index in the caller's t[]
};
struct ClipWs {
  int64_t slots;    // scan workgroups of the whole call = f64 partials
  int64_t nne;      // non-empty arrays
  size_t off_sums, off_desc, off_scale, bytes;
};
template <class F>
static ClipWs clip_plan(int n, const lde_adam_tensor* t, F&& on_launch) {
  ClipWs w{};
  for (int first = 0; first < n;) {
    const OptLaunch L = opt_next_launch(n, t, first, GUARD_PER_WG);
    if (L.n == 0) break;   // nothing left (or an array no launch holds: the update's plan, with the smaller slice, has refused the call)
    on_launch(L, w.slots, w.nne);
    first = L.next;
    w.slots += L.blk0[L.n];
    w.nne += L.n;
  }
  w.off_sums = sizeof(double) * (size_t)w.slots;
  w.off_desc = w.off_sums + sizeof(double) * (size_t)w.nne;
  w.off_scale = w.off_desc + sizeof(ClipDesc) * (size_t)w.nne;
  w.bytes = w.off_scale + sizeof(float) * (size_t)w.nne;
  return w;
}
// what every form of the update refuses, and what the clipped step refuses on top of it — all of it before any device call
static bool opt_args_ok(int n, const lde_adam_tensor* t, float beta1, float beta2, int64_t step, const void* step_dev) {
  if (n < 0 || (n > 0 && !t) || (!step_dev && step < 1) || !(beta1 >= 0.f && beta1 < 1.f) || !(beta2 >= 0.f && beta2 < 1.f)) return false;
  for (int i = 0; i < n; i++)
    if (t[i].n < 0 || (t[i].n > 0 && (!t[i].p || !t[i].g || !t[i].m || !t[i].v))) return false;
  return true;
}
static bool clip_args_ok(int n, const lde_adam_tensor* t, float beta1, float beta2, float clip_norm, int clip_mode, const void* step_dev,
                         const void* guard_dev, const void* ws_dev, const void* norms_dev) {
  if (!step_dev || !guard_dev || !norms_dev || !(clip_norm > 0.f) || !std::isfinite(clip_norm)) return false;
  if (clip_mode != LDE_CLIP_GLOBAL && clip_mode != LDE_CLIP_PER_ARRAY) return false;
  if (!opt_args_ok(n, t, beta1, beta2, 0, step_dev)) return false;
  for (int first = 0; first < n;) {   // the update's plan: an array no launch holds
    const OptLaunch L = opt_next_launch(n, t, first, OPT_PER_WG);
    if (L.too_large) return false;
    if (L.n == 0) break;
    first = L.next;
  }
  bool any = false;
  for (int i = 0; i < n; i++) any = any || t[i].n > 0;
  return !any || (ws_dev && (reinterpret_cast<uintptr_t>(ws_dev) & 7) == 0);
}
// what the AdaBelief step (lde_adabelief_flux_step*, include/lde.h: "the AdaBelief step") refuses on top of its ADAMW twin: an ε that is
// negative or not finite (0 is allowed: the rule without the term)
static bool belief_eps_ok(float eps_var, float eps_den) {
  return eps_var >= 0.f && eps_den >= 0.f && std::isfinite(eps_var) && std::isfinite(eps_den);
}

static KOpts make_opts(const lde_problem_desc& d, const double* ts, int T, int B) {
  KOpts o;
  o.abstol = (float)d.abstol;
  o.reltol = (float)d.reltol;
  o.beta1 = (float)d.beta1;
  o.beta2 = (float)d.beta2;
  o.inv_gamma = (float)(1.0 / d.gamma);
  o.q_lo = (float)(1.0 / d.qmax);
  o.q_hi = (float)(1.0 / d.qmin);
  o.qmin = (float)d.qmin;
  o.dtmin = d.dtmin > 0 ? d.dtmin : 1e-12 * std::fabs(ts[T - 1] - ts[0]);
  o.dt_fixed = d.dt;
  o.maxiters = d.maxiters;
  o.adaptive = d.adaptive;
  o.checkpoint = d.sensealg != LDE_SENSE_BACKSOLVE;
  o.T = T;
  o.B = B;
  o.lb_hold = 0;
  o.dw_overwrite = 0;
  o.t_first = ts[0];
  o.t_last = ts[T - 1];
  o.rec = StepRec{};
  return o;
}

}  // namespace lde_host
