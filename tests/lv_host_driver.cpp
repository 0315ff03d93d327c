// lv_host_driver.cpp — what csrc/lde_host.h decides about the Lotka–Volterra right-hand side (LDE_RHS_LOTKA_VOLTERRA): which descriptions
// validate() serves and refuses and with what text, the dual record generalised over NP partials per component (the pendulum's offsets
// unchanged), the dispatch of its kernels' template arguments — compiled with an ordinary host compiler under AddressSanitizer +
// UndefinedBehaviorSanitizer and run as a program by tests/test_lv_host.py.
#undef NDEBUG
#include <cassert>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../latentdiffeq.jl_amd/csrc/lde_host.h"

using namespace lde_host;

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {   // xorshift64*
  g_state ^= g_state >> 12; g_state ^= g_state << 25; g_state ^= g_state >> 27;
  return g_state * 0x2545F4914F6CDD1Dull;
}
static int hostile_int() {
  static const int v[] = {0, 1, -1, 2, 3, 4, 5, 6, 7, 64, 255, 256, 65536, std::numeric_limits<int>::max(), std::numeric_limits<int>::min(), -7, 1 << 30};
  return (rnd() & 3) ? v[rnd() % (sizeof(v) / sizeof(v[0]))] : (int)(uint32_t)rnd();
}
static double hostile_double() {
  static const double v[] = {0.0, -0.0, 1.0, -1.0, 1e-300, 1e300, -1e300, 0.05, 1e-6, std::numeric_limits<double>::infinity(),
                             -std::numeric_limits<double>::infinity(), std::numeric_limits<double>::quiet_NaN(), std::numeric_limits<double>::denorm_min()};
  return v[rnd() % (sizeof(v) / sizeof(v[0]))];
}

static lde_problem_desc lv_desc() {
  lde_problem_desc d{};
  d.abi_version = LDE_ABI_VERSION;
  d.rhs_kind = LDE_RHS_LOTKA_VOLTERRA;
  d.state_dim = 2;
  d.param_dim = 4;
  d.solver = LDE_SOLVER_TSIT5;
  d.batching = LDE_BATCH_PER_TRAJECTORY;
  d.sensealg = LDE_SENSE_FORWARD_DUAL;
  d.adaptive = 1;
  d.maxiters = 100000;
  d.abstol = 1e-6; d.reltol = 1e-3; d.qmin = 0.2; d.qmax = 10.0; d.gamma = 0.9; d.beta1 = 0.14; d.beta2 = 0.08;
  return d;
}

static size_t a256(size_t x) { return (x + 255) & ~size_t(255); }

int main() {
  std::string why;
  static_assert(LDE_RHS_LOTKA_VOLTERRA == 5 && LDE_RHS_SPENDULUM == 4 && LDE_SOLVER_EULER_HEUN == 3, "enum values");

  // 1. what validate() serves: Tsit5 adaptive, Tsit5 fixed-step, RK4 fixed-step — and nothing of the kind's helpers changes for the others
  {
    lde_problem_desc d = lv_desc();
    assert(validate(&d, &why) == LDE_OK);
    d.adaptive = 0; d.dt = 0.05;
    assert(validate(&d, &why) == LDE_OK);
    d.solver = LDE_SOLVER_RK4;
    assert(validate(&d, &why) == LDE_OK);
    d = lv_desc();
    d.dt = 0.01;   // adaptive with a first step given
    assert(validate(&d, &why) == LDE_OK);
    assert(num_weights(&d) == 0 && is_lv(d) && !has_pend(d) && !has_mlp(d) && !is_sde(d) && dual_partials(d) == 6);
    lde_problem_desc p = d;
    p.rhs_kind = LDE_RHS_PENDULUM; p.param_dim = 1;
    assert(validate(&p, &why) == LDE_OK && has_pend(p) && !is_lv(p) && dual_partials(p) == 3);
    p.rhs_kind = LDE_RHS_SPENDULUM;
    assert(has_pend(p) && is_sde(p) && dual_partials(p) == 3);
    // the helpers the C ABI calls for any accepted description
    std::vector<double> ts(50);
    for (int j = 0; j < 50; j++) ts[j] = 0.05 * j;
    KOpts o = make_opts(d, ts.data(), 50, 7);
    assert(o.T == 50 && o.B == 7 && o.adaptive == 1 && o.t_last == ts[49]);
    assert(rec_capacity(d, 0, 50, 0) == 200 && rec_nseq(d, 7) == 7);
  }
  // 2. what it refuses, with which status and text
  {
    const lde_problem_desc d = lv_desc();
    auto refused = [&](lde_problem_desc x, int status, const char* needle) {
      std::string w;
      return validate(&x, &w) == status && w.find(needle) != std::string::npos;
    };
    const int INV = LDE_ERR_INVALID_ARG, UNS = LDE_ERR_UNSUPPORTED;
    lde_problem_desc x = d;
    x.state_dim = 3; assert(refused(x, INV, "state_dim=2, param_dim=4"));
    x = d; x.param_dim = 1; assert(refused(x, INV, "LDE_RHS_LOTKA_VOLTERRA needs state_dim=2, param_dim=4, augment_dim=0"));
    x = d; x.param_dim = 3; assert(refused(x, INV, "param_dim=4"));
    x = d; x.augment_dim = 1; assert(refused(x, INV, "augment_dim=0"));
    x = d; x.n_layers = 1; assert(refused(x, INV, "n_layers must be 0"));
    // the dimension check comes before any solver check: a wrong-dims description with an unserved solver is an argument error
    x = d; x.param_dim = 1; x.solver = LDE_SOLVER_EM; assert(refused(x, INV, "param_dim=4"));
    x = d; x.param_dim = 1; x.solver = 4; assert(refused(x, INV, "param_dim=4"));
    x = d; x.solver = 4; assert(refused(x, INV, "unknown solver"));
    x = d; x.rhs_kind = 6; assert(refused(x, INV, "unknown rhs_kind"));
    for (int s : {LDE_SENSE_BACKSOLVE_CHECKPOINTED, LDE_SENSE_BACKSOLVE, LDE_SENSE_PARALLEL_CHECKPOINTED, LDE_SENSE_DISCRETE}) {
      x = d; x.sensealg = s; assert(refused(x, UNS, "use LDE_SENSE_FORWARD_DUAL"));
    }
    x = d; x.batching = LDE_BATCH_COUPLED; assert(refused(x, UNS, "LDE_BATCH_PER_TRAJECTORY only"));
    x = d; x.batching = LDE_BATCH_COUPLED_GLOBAL; assert(refused(x, INV, "LDE_BATCH_COUPLED_GLOBAL needs an MLP"));
    for (int s : {LDE_SOLVER_EM, LDE_SOLVER_EULER_HEUN}) {   // the stochastic steppers keep their refusal
      x = d; x.solver = s; x.adaptive = 0; x.dt = 0.05; assert(refused(x, UNS, "LDE_RHS_SPENDULUM only"));
    }
    x = d; x.solver = LDE_SOLVER_RK4; assert(refused(x, UNS, "RK4 is fixed-step only"));   // adaptive RK4 keeps its refusal
    x = d; x.adaptive = 0; x.dt = 0; assert(refused(x, INV, "dt>0"));
    x = d; x.maxiters = 0; assert(refused(x, INV, "maxiters"));
    // the pendulum description with the new kind's number (tests/sde_host_driver.cpp pins this outcome): an argument error, by the dims
    x = d; x.param_dim = 1; x.solver = LDE_SOLVER_EULER_HEUN; x.adaptive = 0; x.dt = 0.05;
    assert(refused(x, INV, "param_dim=4"));
  }
  // 3. the dual record over NP partials per component: consecutive, aligned, inside dual_rec_bytes; the last element of every array touched
  //    (an overrun is an ASan report) — and the pendulum's offsets are what they were
  for (int np : {3, 6})
    for (int B : {1, 3, 37, 64, 257, 4097})
      for (int T : {1, 2, 9, 50})
        for (int cap : {1, 64, 200})
          for (int trace = 0; trace < 2; trace++) {
            const size_t bytes = dual_rec_bytes(B, T, cap, trace != 0, np);
            const size_t nJ = (size_t)T * 2 * np * B;
            assert(bytes == a256((size_t)4 * B) + a256(4 * nJ) + (trace ? 2 * a256((size_t)8 * cap * B) : 0));
            std::vector<unsigned char> buf(bytes + 256);
            unsigned char* base = (unsigned char*)(((uintptr_t)buf.data() + 255) & ~(uintptr_t)255);
            DualRec r = dual_rec_view(base, B, T, cap, trace != 0, np);
            assert((unsigned char*)r.n == base && (unsigned char*)r.J == base + a256((size_t)4 * B));
            r.n[B - 1] = 1;
            r.J[nJ - 1] = 1.f;
            assert((unsigned char*)(r.J + nJ) <= base + bytes);
            if (trace) {
              assert((unsigned char*)r.t == base + a256((size_t)4 * B) + a256(4 * nJ) && (unsigned char*)r.dt == (unsigned char*)r.t + a256((size_t)8 * cap * B));
              assert(r.cap == cap && ((uintptr_t)r.t & 255) == 0 && ((uintptr_t)r.dt & 255) == 0);
              r.t[(size_t)cap * B - 1] = 1.0;
              r.dt[(size_t)cap * B - 1] = 1.0;
              assert((unsigned char*)(r.dt + (size_t)cap * B) <= base + bytes);
            } else {
              assert(!r.t && !r.dt && r.cap == 0);
            }
            if (np == 3) {   // the four-argument forms are the pendulum's: every size and offset as before (24·T·B bytes of J)
              assert(dual_rec_bytes(B, T, cap, trace != 0) == bytes && bytes == a256((size_t)4 * B) + a256((size_t)24 * T * B) + (trace ? 2 * a256((size_t)8 * cap * B) : 0));
              DualRec q = dual_rec_view(base, B, T, cap, trace != 0);
              assert(q.n == r.n && q.J == r.J && q.t == r.t && q.dt == r.dt && q.cap == r.cap);
            }
          }
  assert(dual_rec_bytes(7, 50, 200, false, 6) >= 256 + 48 * 50 * 7);
  // 4. the kernels' template arguments: exactly (Tsit5 adaptive, Tsit5 fixed-step, RK4 fixed-step) reach the kernels
  {
    int seen[2] = {};
    auto rec = [&](auto S) -> int {
      static_assert(decltype(S)::value == LDE_SOLVER_TSIT5 || decltype(S)::value == LDE_SOLVER_RK4, "SOLVER");
      seen[S]++;
      return 10 + S;
    };
    const int TS = LDE_SOLVER_TSIT5, RK = LDE_SOLVER_RK4;
    assert(lv_dispatch(TS, true, rec) == 10 && lv_dispatch(TS, false, rec) == 10 && lv_dispatch(RK, false, rec) == 11);
    assert(lv_dispatch(RK, true, rec) == LDE_ERR_UNSUPPORTED);   // adaptive RK4
    assert(lv_dispatch(LDE_SOLVER_EM, false, rec) == LDE_ERR_UNSUPPORTED && lv_dispatch(LDE_SOLVER_EULER_HEUN, false, rec) == LDE_ERR_UNSUPPORTED);
    assert(lv_dispatch(-1, true, rec) == LDE_ERR_UNSUPPORTED && lv_dispatch(4, false, rec) == LDE_ERR_UNSUPPORTED);
    assert(seen[0] == 2 && seen[1] == 1);
    // the pendulums' dispatch does not know the kind
    assert(pend_dispatch(LDE_RHS_LOTKA_VOLTERRA, TS, true, [&](auto, auto, auto) -> int { return LDE_OK; }) == LDE_ERR_UNSUPPORTED);
    // any arguments: f is called for a combination validate() admits for this kind, or not at all
    for (int it = 0; it < 20000; it++) {
      lde_problem_desc d = lv_desc();
      d.solver = (rnd() & 1) ? hostile_int() : (int)(rnd() % 4);
      d.adaptive = (int)(rnd() % 2);
      d.dt = 0.05;
      int called = 0;
      const int rc = lv_dispatch(d.solver, d.adaptive != 0, [&](auto) -> int { called++; return LDE_OK; });
      assert(called == (rc == LDE_OK) && (rc == LDE_OK || rc == LDE_ERR_UNSUPPORTED));
      assert(called == (validate(&d, &why) == LDE_OK));
    }
  }
  // 5. hostile descriptions of the new kind: never a crash, always a status; an accepted one is one of the three served combinations
  int accepted = 0;
  for (int it = 0; it < 20000; it++) {
    lde_problem_desc d = lv_desc();
    const int nmut = 1 + (int)(rnd() % 4);
    for (int m = 0; m < nmut; m++) {
      switch (rnd() % 22) {
        case 0: d.abi_version = hostile_int(); break;
        case 1: d.rhs_kind = (rnd() & 1) ? hostile_int() : (int)(rnd() % 7); break;
        case 2: d.state_dim = hostile_int(); break;
        case 3: d.param_dim = hostile_int(); break;
        case 4: d.augment_dim = hostile_int(); break;
        case 5: d.n_layers = hostile_int(); break;
        case 6: d.layer_sizes[rnd() % (LDE_MAX_LAYERS + 1)] = hostile_int(); break;
        case 7: d.activation = hostile_int(); break;
        case 8: d.solver = (rnd() & 1) ? hostile_int() : (int)(rnd() % 5); break;
        case 9: d.batching = hostile_int(); break;
        case 10: d.sensealg = (rnd() & 1) ? hostile_int() : (int)(rnd() % 6); break;
        case 11: d.adaptive = hostile_int(); break;
        case 12: d.maxiters = (int64_t)rnd() * ((rnd() & 1) ? 1 : -1); break;
        case 13: d.dt = hostile_double(); break;
        case 14: d.abstol = hostile_double(); break;
        case 15: d.reltol = hostile_double(); break;
        case 16: d.dtmin = hostile_double(); break;
        case 17: d.qmin = hostile_double(); break;
        case 18: d.qmax = hostile_double(); break;
        case 19: d.gamma = hostile_double(); break;
        case 20: d.beta1 = hostile_double(); break;
        default: d.beta2 = hostile_double(); break;
      }
    }
    why.clear();
    const int rc = validate(&d, &why);
    assert(rc == LDE_OK || rc == LDE_ERR_INVALID_ARG || rc == LDE_ERR_UNSUPPORTED);
    assert((rc == LDE_OK) == why.empty());
    (void)num_weights(&d);
    (void)dual_partials(d);
    if (rc == LDE_OK && is_lv(d)) {
      accepted++;
      assert(d.state_dim == 2 && d.param_dim == 4 && d.augment_dim == 0 && d.n_layers == 0 && d.batching == LDE_BATCH_PER_TRAJECTORY);
      assert(d.sensealg == LDE_SENSE_FORWARD_DUAL && num_weights(&d) == 0);
      assert(lv_dispatch(d.solver, d.adaptive != 0, [&](auto) -> int { return LDE_OK; }) == LDE_OK);
      const double ts[3] = {0.0, 0.5, 1.0};
      const KOpts o = make_opts(d, ts, 3, 5);
      assert(o.T == 3 && o.B == 5);
      const int cap = rec_capacity(d, 0, 3, 0);
      assert(cap >= 1 && dual_rec_bytes(5, 3, cap, true, dual_partials(d)) >= 256 + 48 * 3 * 5);
    }
  }
  assert(accepted > 100);
  std::printf("lotka-volterra host logic under ASan + UBSan: validate, the dual record over NP, the dispatch and %d accepted of 20000 hostile descriptions checked\n", accepted);
  return 0;
}
