// sde_host_driver.cpp — the stochastic pendulum's substep plan (csrc/lde_host.h: sde_plan; csrc/lde_types.h: sde_substeps — the function
// the kernel's loop calls) and the description rules that go with it, compiled with an ordinary host compiler under AddressSanitizer +
// UndefinedBehaviorSanitizer and run as a program by tests/test_sde_host.py.
#undef NDEBUG
#include <cassert>
#include <cstdio>
#include <limits>
#include <vector>

#include "../latentdiffeq.jl_amd/csrc/lde_host.h"

using namespace lde_host;

static lde_problem_desc sde_desc(double dt, int64_t maxiters = 100000) {
  lde_problem_desc d{};
  d.abi_version = LDE_ABI_VERSION;
  d.rhs_kind = LDE_RHS_SPENDULUM;
  d.state_dim = 2;
  d.param_dim = 1;
  d.solver = LDE_SOLVER_EULER_HEUN;
  d.batching = LDE_BATCH_PER_TRAJECTORY;
  d.sensealg = LDE_SENSE_FORWARD_DUAL;
  d.adaptive = 0;
  d.dt = dt;
  d.maxiters = maxiters;
  d.abstol = 1e-6; d.reltol = 1e-3; d.qmin = 0.2; d.qmax = 10.0; d.gamma = 0.9; d.beta1 = 0.14; d.beta2 = 0.08;
  return d;
}

int main() {
  std::string why;
  // the rule itself: max(1, ceil(D/dt − 1e-9)), at most 1e9
  assert(lde::sde_substeps(0.05, 0.05) == 1 && lde::sde_substeps(0.05, 0.0125) == 4 && lde::sde_substeps(0.051, 0.05) == 2);
  assert(lde::sde_substeps(0.01, 0.05) == 1 && lde::sde_substeps(0.13, 0.05) == 3 && lde::sde_substeps(0.1, 0.05) == 2);
  assert(lde::sde_substeps(0.05 * 7 - 0.05 * 6, 0.05) == 1);   // a grid 0.05·j in f64: the 1e-9 absorbs the quotient's last bits
  assert(lde::sde_substeps(1.0, 1e-30) == 1000000000 && lde::sde_substeps(std::numeric_limits<double>::max(), 1e-300) == 1000000000);
  assert(lde::sde_substeps(std::numeric_limits<double>::quiet_NaN(), 0.05) == 1);

  // the uniform grid of the tests: 49 intervals of one / four substeps
  {
    std::vector<double> ts(50);
    for (int j = 0; j < 50; j++) ts[j] = 0.05 * j;
    lde_problem_desc d = sde_desc(0.05);
    assert(validate(&d, &why) == LDE_OK);
    SdePlan p = sde_plan(d, ts.data(), 50);
    assert(p.N == 49 && !p.over);
    d.dt = 0.0125;
    p = sde_plan(d, ts.data(), 50);
    assert(p.N == 196 && !p.over);
    d.dt = 0.05;
    d.maxiters = 10;   // 49 substeps against maxiters = 10: capped, every trajectory fails
    p = sde_plan(d, ts.data(), 50);
    assert(p.N == 10 && p.over);
    d.maxiters = 49;   // exactly maxiters substeps are allowed
    p = sde_plan(d, ts.data(), 50);
    assert(p.N == 49 && !p.over);
    // the helpers the C ABI calls for any accepted description stay defined for this one
    KOpts o = make_opts(d, ts.data(), 50, 7);
    assert(o.T == 50 && o.B == 7 && o.dt_fixed == 0.05 && !o.adaptive);
    assert(fixed_step_count(d, ts.data(), 50) == 49);
    const int cap = rec_capacity(d, 0, 50, 0);
    assert(cap >= 1 && rec_nseq(d, 7) == 7 && rec_bytes(d, 7, cap, true) >= 28);
    assert(dual_rec_bytes(7, 50, cap, false) >= 256 + 24 * 50 * 7);
  }
  // a ragged grid: 1, 3, 2, 1, 3 substeps
  {
    const double ts[6] = {0.0, 0.01, 0.14, 0.22, 0.27, 0.3701};
    lde_problem_desc d = sde_desc(0.05);
    const SdePlan p = sde_plan(d, ts, 6);
    assert(p.N == 1 + 3 + 2 + 1 + 3 && !p.over);
  }
  // dt larger than every interval: one substep each
  {
    const double ts[4] = {-1.0, -0.9, 0.0, 0.02};
    lde_problem_desc d = sde_desc(5.0);
    const SdePlan p = sde_plan(d, ts, 4);
    assert(p.N == 3 && !p.over);
  }
  // dt = 1e-30: 1e9 substeps per interval, capped at maxiters — also at the largest maxiters — without overflow
  {
    std::vector<double> ts(4096);
    for (int j = 0; j < 4096; j++) ts[j] = 1e3 * j;
    lde_problem_desc d = sde_desc(1e-30);
    assert(validate(&d, &why) == LDE_OK);
    SdePlan p = sde_plan(d, ts.data(), 4096);
    assert(p.N == 100000 && p.over);
    d.maxiters = std::numeric_limits<int64_t>::max();
    p = sde_plan(d, ts.data(), 4096);
    assert(p.N == (int64_t)4095 * 1000000000 && !p.over);
    d.maxiters = 0;   // (validate refuses it; the plan still answers)
    p = sde_plan(d, ts.data(), 4096);
    assert(p.N == 0 && p.over);
  }
  // T = 1: nothing to step
  {
    const double ts[1] = {3.0};
    lde_problem_desc d = sde_desc(0.05);
    const SdePlan p = sde_plan(d, ts, 1);
    assert(p.N == 0 && !p.over);
    KOpts o = make_opts(d, ts, 1, 1);
    assert(o.t_first == 3.0 && o.t_last == 3.0);
  }
  // what validate() serves of the new kind, and what it refuses with LDE_ERR_UNSUPPORTED
  {
    lde_problem_desc d = sde_desc(0.05);
    for (int s : {LDE_SOLVER_EM, LDE_SOLVER_EULER_HEUN}) { d.solver = s; assert(validate(&d, &why) == LDE_OK); }
    auto refused = [&](lde_problem_desc x, const char* needle) {
      std::string w;
      return validate(&x, &w) == LDE_ERR_UNSUPPORTED && w.find(needle) != std::string::npos;
    };
    lde_problem_desc x = d; x.adaptive = 1; assert(refused(x, "adaptive"));
    x = d; x.dt = 0; assert(refused(x, "dt"));
    x = d; x.dt = std::numeric_limits<double>::infinity(); assert(refused(x, "dt"));
    x = d; x.batching = LDE_BATCH_COUPLED; assert(refused(x, "LDE_BATCH_PER_TRAJECTORY"));
    x = d; x.sensealg = LDE_SENSE_DISCRETE; assert(refused(x, "use LDE_SENSE_FORWARD_DUAL"));
    x = d; x.solver = LDE_SOLVER_TSIT5; assert(refused(x, "LDE_SOLVER_EM"));
    x = d; x.rhs_kind = LDE_RHS_PENDULUM; x.solver = LDE_SOLVER_EM; assert(refused(x, "LDE_RHS_SPENDULUM"));
    x = d; x.state_dim = 3; assert(validate(&x, &why) == LDE_ERR_INVALID_ARG);
    x = d; x.n_layers = 1; assert(validate(&x, &why) == LDE_ERR_INVALID_ARG);
    x = d; x.rhs_kind = 5; assert(validate(&x, &why) == LDE_ERR_INVALID_ARG);
    x = d; x.solver = 4; assert(validate(&x, &why) == LDE_ERR_INVALID_ARG);
    assert(num_weights(&d) == 0 && has_pend(d) && !has_mlp(d));
  }
  std::printf("sde substep plan under ASan + UBSan: rule, ragged grids, dt beyond an interval, the maxiters cap and T = 1 checked\n");
  return 0;
}
