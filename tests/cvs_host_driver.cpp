// cvs_host_driver.cpp — what csrc/lde_host.h decides about the cardiovascular system (LDE_RHS_CVS) on the lane-per-direction kernels
// (csrc/lde_dual_dir.hip): validate(), the group width (G = 8 for NP = 6: two pad lanes), lanes / block / grid at the 4 096-lane threshold
// (B = 512 and 513), dual_partials, the dual record (sizes, offsets, the last element of every array touched) and the dispatch of the
// kernels' template arguments for all three systems — compiled with an ordinary host compiler under AddressSanitizer +
// UndefinedBehaviorSanitizer and run as a program by tests/test_cvs_host.py.
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
  static const int v[] = {0, 1, -1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 15, 16, 64, 255, 256, 65536, std::numeric_limits<int>::max(), std::numeric_limits<int>::min(), -7, 1 << 30};
  return (rnd() & 3) ? v[rnd() % (sizeof(v) / sizeof(v[0]))] : (int)(uint32_t)rnd();
}

static lde_problem_desc base_desc(int kind, int D, int P) {
  lde_problem_desc d{};
  d.abi_version = LDE_ABI_VERSION;
  d.rhs_kind = kind;
  d.state_dim = D;
  d.param_dim = P;
  d.solver = LDE_SOLVER_TSIT5;
  d.batching = LDE_BATCH_PER_TRAJECTORY;
  d.sensealg = LDE_SENSE_FORWARD_DUAL;
  d.adaptive = 1;
  d.maxiters = 100000;
  d.abstol = 1e-6; d.reltol = 1e-3; d.qmin = 0.2; d.qmax = 10.0; d.gamma = 0.9; d.beta1 = 0.14; d.beta2 = 0.08;
  return d;
}
static lde_problem_desc cvs_desc() { return base_desc(LDE_RHS_CVS, 4, 2); }
static lde_problem_desc dpend_desc() { return base_desc(LDE_RHS_DOUBLE_PENDULUM, 4, 4); }
static lde_problem_desc kuramoto_desc(int N) { return base_desc(LDE_RHS_KURAMOTO, N, N + 1); }

static size_t a256(size_t x) { return (x + 255) & ~size_t(255); }

int main() {
  std::string why;
  static_assert(LDE_RHS_CVS == 11 && LDE_RHS_DOUBLE_PENDULUM == 9 && LDE_RHS_KURAMOTO == 7 && LDE_RHS_LOTKA_VOLTERRA == 5 && LDE_ABI_VERSION == 1, "enum values; the ABI version did not move");
  const int CV = LDE_RHS_CVS, DP = LDE_RHS_DOUBLE_PENDULUM, KU = LDE_RHS_KURAMOTO;

  // 1. the group: D = 4 with NP = 6 sits in one 8-lane group, lanes 6 and 7 pad; the other systems' rules are what they were
  static_assert(dir_group_width(CV, 4) == 8 && dir_partials(CV, 4) == 6 && dir_state_ok(CV, 4), "CVS: six directions in eight lanes");
  static_assert(dir_group_width(DP, 4) == 8 && dir_partials(DP, 4) == 8 && dir_state_ok(DP, 4), "the double pendulum fills its group");
  for (int D = -3; D <= 20; D++) {
    if (D != 4) assert(dir_group_width(CV, D) == 0 && dir_partials(CV, D) == 0 && !dir_state_ok(CV, D));
    if (D != 4) assert(dir_group_width(DP, D) == 0 && dir_partials(DP, D) == 0 && !dir_state_ok(DP, D));
    assert(dir_group_width(KU, D) == dir_group_width(D) && dir_partials(KU, D) == dir_partials(D) && dir_state_ok(KU, D) == dir_state_ok(D));
    for (int kind : {-1, 0, 1, 2, 3, 4, 5, 6, 8, 10, 12}) assert(dir_group_width(kind, D) == 0 && dir_partials(kind, D) == 0 && !dir_state_ok(kind, D));
  }
  {
    const lde_problem_desc d = cvs_desc();
    assert(dir_group_width(d) == 8 && dual_partials(d) == 16 && dual_partials(d) * 2 == d.state_dim * dir_group_width(d));
    assert(is_cvs(d) && is_dir(d) && !is_dpend(d) && !is_kuramoto(d) && !is_lv(d) && !has_pend(d) && !has_mlp(d) && !is_sde(d) && num_weights(&d) == 0);
    const lde_problem_desc p = dpend_desc();
    assert(dual_partials(p) == 16 && !is_cvs(p) && is_dir(p));
  }

  // 2. the launch over B·8 lanes: whole groups per workgroup, every lane covered, 64-lane workgroups up to 4 096 lanes (B = 512), 256 beyond
  {
    const lde_problem_desc d = cvs_desc();
    for (int B : {1, 2, 7, 8, 37, 255, 256, 257, 511, 512, 513, 4097, 65536, std::numeric_limits<int>::max()}) {
      const int block = dir_block(d, B);
      const int64_t lanes = dir_lanes(d, B), grid = dir_grid(d, B);
      assert(lanes == (int64_t)B * 8 && (block == 64 || block == 256) && block % 8 == 0);
      assert((block == 64) == (lanes <= 4096));
      assert(grid >= 1 && grid * block >= lanes && (grid - 1) * block < lanes);
    }
    assert(dir_lanes(d, 0) == 0 && dir_lanes(d, -5) == 0 && dir_grid(d, 0) == 0 && dir_block(d, 0) == 64);
    assert(dir_lanes(d, 1) == 8 && dir_block(d, 1) == 64 && dir_grid(d, 1) == 1);
    assert(dir_lanes(d, 512) == 4096 && dir_block(d, 512) == 64 && dir_grid(d, 512) == 64);
    assert(dir_lanes(d, 513) == 4104 && dir_block(d, 513) == 256 && dir_grid(d, 513) == 17);
  }

  // 3. what validate() serves …
  {
    lde_problem_desc d = cvs_desc();
    assert(validate(&d, &why) == LDE_OK);
    d.dt = 0.01;   // adaptive with a first step given
    assert(validate(&d, &why) == LDE_OK);
    d.adaptive = 0; d.dt = 0.05;
    assert(validate(&d, &why) == LDE_OK);
    d.solver = LDE_SOLVER_RK4;
    assert(validate(&d, &why) == LDE_OK);
    std::vector<double> ts(50);
    for (int j = 0; j < 50; j++) ts[j] = 1.0 * j;
    KOpts o = make_opts(d, ts.data(), 50, 7);
    assert(o.T == 50 && o.B == 7 && o.adaptive == 0 && o.t_last == ts[49]);
    assert(rec_capacity(d, 0, 50, 0) == 200 && rec_nseq(d, 7) == 7);
  }
  // 4. … and what it refuses, with which status and text
  {
    const lde_problem_desc d = cvs_desc();
    auto refused = [&](lde_problem_desc x, int status, const char* needle) {
      std::string w;
      return validate(&x, &w) == status && w.find(needle) != std::string::npos;
    };
    const int INV = LDE_ERR_INVALID_ARG, UNS = LDE_ERR_UNSUPPORTED;
    const char* dims = "LDE_RHS_CVS needs state_dim=4, param_dim=2, augment_dim=0";
    lde_problem_desc x = d;
    x.state_dim = 2; assert(refused(x, INV, dims));
    x = d; x.state_dim = 5; x.param_dim = 3; assert(refused(x, INV, dims));
    x = d; x.state_dim = 0; assert(refused(x, INV, "bad dims"));
    x = d; x.param_dim = 1; assert(refused(x, INV, dims));
    x = d; x.param_dim = 4; assert(refused(x, INV, dims));
    x = d; x.augment_dim = 1; assert(refused(x, INV, dims));
    x = d; x.n_layers = 1; assert(refused(x, INV, "LDE_RHS_CVS is analytic: n_layers must be 0"));
    for (int kind : {6, 8, 10, 12, -1}) {   // still no right-hand sides
      x = d; x.rhs_kind = kind; assert(refused(x, INV, "unknown rhs_kind"));
    }
    x = d; x.param_dim = 1; x.solver = LDE_SOLVER_EM; assert(refused(x, INV, dims));   // the dimension check comes before any solver check
    x = d; x.solver = 4; assert(refused(x, INV, "unknown solver"));
    for (int s : {LDE_SENSE_BACKSOLVE_CHECKPOINTED, LDE_SENSE_BACKSOLVE, LDE_SENSE_PARALLEL_CHECKPOINTED, LDE_SENSE_DISCRETE}) {
      x = d; x.sensealg = s; assert(refused(x, UNS, "LDE_RHS_CVS: only the solve on dual numbers exists") && refused(x, UNS, "use LDE_SENSE_FORWARD_DUAL"));
    }
    x = d; x.batching = LDE_BATCH_COUPLED; assert(refused(x, UNS, "LDE_RHS_CVS: no coupled solve; LDE_BATCH_PER_TRAJECTORY only"));
    x = d; x.batching = LDE_BATCH_COUPLED_GLOBAL; assert(refused(x, INV, "LDE_BATCH_COUPLED_GLOBAL needs an MLP"));
    for (int s : {LDE_SOLVER_EM, LDE_SOLVER_EULER_HEUN}) {
      x = d; x.solver = s; x.adaptive = 0; x.dt = 0.05; assert(refused(x, UNS, "LDE_RHS_SPENDULUM only"));
    }
    x = d; x.solver = LDE_SOLVER_RK4; assert(refused(x, UNS, "RK4 is fixed-step only"));
    x = d; x.adaptive = 0; x.dt = 0; assert(refused(x, INV, "dt>0"));
    x = d; x.maxiters = 0; assert(refused(x, INV, "maxiters"));
    // the double pendulum's description is still served, and still refuses CVS's dimensions
    x = dpend_desc(); assert(validate(&x, &why) == LDE_OK);
    x.param_dim = 2; assert(refused(x, INV, "LDE_RHS_DOUBLE_PENDULUM needs"));
  }
  // 5. the dual record — n [B] | J [T][4][B][8] | t, dt [cap][B]: consecutive, 256-byte aligned, inside the bytes, no overlap; the last element
  //    of every array — and the last element a lane of the kernels indexes, a pad lane's — touched (an overrun is an ASan report)
  {
    const lde_problem_desc d = cvs_desc();
    const int D = 4, G = dir_group_width(d), np = dual_partials(d);
    for (int B : {1, 3, 37, 64, 257, 513, 1025})
      for (int T : {1, 2, 9, 50})
        for (int cap : {1, 64, 200})
          for (int trace = 0; trace < 2; trace++) {
            const size_t nJ = (size_t)T * D * B * G;
            const size_t bytes = dual_rec_bytes(B, T, cap, trace != 0, np);
            assert(bytes == a256((size_t)4 * B) + a256(4 * nJ) + (trace ? 2 * a256((size_t)8 * cap * B) : 0));
            assert(a256(4 * nJ) == a256((size_t)128 * T * B));
            std::vector<unsigned char> buf(bytes + 256);
            unsigned char* base = (unsigned char*)(((uintptr_t)buf.data() + 255) & ~(uintptr_t)255);
            DualRec r = dual_rec_view(base, B, T, cap, trace != 0, np);
            assert((unsigned char*)r.n == base && (unsigned char*)r.J == base + a256((size_t)4 * B) && ((uintptr_t)r.J & 255) == 0);
            assert((unsigned char*)(r.n + B) <= (unsigned char*)r.J);
            r.n[B - 1] = 1;
            const size_t last = (((size_t)(T - 1) * D + (D - 1)) * B + (B - 1)) * G + (G - 1);   // the kernels' index of the last (j, i, b, q)
            assert(last == nJ - 1);
            r.J[last] = 1.f;
            r.J[0] = 1.f;
            assert((unsigned char*)(r.J + nJ) <= base + bytes);
            if (trace) {
              assert((unsigned char*)r.t == (unsigned char*)r.J + a256(4 * nJ) && (unsigned char*)r.dt == (unsigned char*)r.t + a256((size_t)8 * cap * B));
              assert(r.cap == cap && ((uintptr_t)r.t & 255) == 0 && ((uintptr_t)r.dt & 255) == 0);
              r.t[(size_t)cap * B - 1] = 1.0;
              r.dt[(size_t)cap * B - 1] = 1.0;
              assert((unsigned char*)(r.dt + (size_t)cap * B) <= base + bytes);
            } else {
              assert(!r.t && !r.dt && r.cap == 0);
            }
          }
  }
  // 6. the launchers' dispatch over all three systems: (LDE_RHS_KURAMOTO, N = 2 … 7), (LDE_RHS_DOUBLE_PENDULUM, 4) and (LDE_RHS_CVS, 4) × exactly
  //    (Tsit5 adaptive, Tsit5 fixed-step, RK4 fixed-step) reach the kernels; nothing else does. The two-system forms do not know CVS.
  {
    int seen[12][8][2] = {};
    auto rec = [&](auto kind, auto n, auto S) -> int {
      static_assert((decltype(kind)::value == LDE_RHS_KURAMOTO && decltype(n)::value >= 2 && decltype(n)::value <= 7) ||
                        ((decltype(kind)::value == LDE_RHS_DOUBLE_PENDULUM || decltype(kind)::value == LDE_RHS_CVS) && decltype(n)::value == 4), "the system");
      static_assert(decltype(S)::value == LDE_SOLVER_TSIT5 || decltype(S)::value == LDE_SOLVER_RK4, "SOLVER");
      static_assert(dir_group_width(decltype(kind)::value, decltype(n)::value) >= dir_partials(decltype(kind)::value, decltype(n)::value), "NP <= G");
      seen[kind][n][S]++;
      return 1000 * kind + 10 * n + S;
    };
    auto with = [](lde_problem_desc d, int solver, int adaptive) { d.solver = solver; d.adaptive = adaptive; d.dt = 0.05; return d; };
    const int TS = LDE_SOLVER_TSIT5, RK = LDE_SOLVER_RK4;
    {
      const lde_problem_desc d = cvs_desc();
      assert(dir_system_dispatch(with(d, TS, 1), rec) == 11040 && dir_system_dispatch(with(d, TS, 0), rec) == 11040 && dir_system_dispatch(with(d, RK, 0), rec) == 11041);
      assert(dir_system_dispatch(with(d, RK, 1), rec) == LDE_ERR_UNSUPPORTED);
      assert(dir_system_dispatch(with(d, LDE_SOLVER_EM, 0), rec) == LDE_ERR_UNSUPPORTED && dir_system_dispatch(with(d, LDE_SOLVER_EULER_HEUN, 0), rec) == LDE_ERR_UNSUPPORTED);
      assert(seen[CV][4][0] == 2 && seen[CV][4][1] == 1);
      assert(dir_system_dispatch_n(d, [&](auto kind, auto n) -> int { return 100 * kind + n; }) == 1104);
      lde_problem_desc x = d;
      x.state_dim = 3; assert(dir_system_dispatch(x, rec) == LDE_ERR_UNSUPPORTED && dir_system_dispatch_n(x, [&](auto, auto) -> int { return LDE_OK; }) == LDE_ERR_UNSUPPORTED);
      assert(dir_dispatch_n(d, [&](auto, auto) -> int { return LDE_OK; }) == LDE_ERR_UNSUPPORTED);
    }
    {
      const lde_problem_desc d = dpend_desc();
      assert(dir_system_dispatch(with(d, TS, 1), rec) == 9040 && dir_system_dispatch(with(d, RK, 0), rec) == 9041 && dir_system_dispatch(with(d, RK, 1), rec) == LDE_ERR_UNSUPPORTED);
      assert(dir_system_dispatch_n(d, [&](auto kind, auto n) -> int { return 100 * kind + n; }) == 904);
    }
    for (int N = 2; N <= 7; N++) {
      const lde_problem_desc d = kuramoto_desc(N);
      assert(dir_system_dispatch(with(d, TS, 1), rec) == 7000 + 10 * N && dir_system_dispatch(with(d, RK, 0), rec) == 7001 + 10 * N);
      assert(dir_system_dispatch_n(d, [&](auto kind, auto n) -> int { return 100 * kind + n; }) == 700 + N);
    }
    for (int kind : {0, 1, 2, 3, 4, 5, 6, 8, 10, 12, -1}) {
      lde_problem_desc d = cvs_desc();
      d.rhs_kind = kind;
      assert(dir_system_dispatch(d, rec) == LDE_ERR_UNSUPPORTED && dir_system_dispatch_n(d, [&](auto, auto) -> int { return LDE_OK; }) == LDE_ERR_UNSUPPORTED);
    }
    assert(pend_dispatch(CV, TS, true, [&](auto, auto, auto) -> int { return LDE_OK; }) == LDE_ERR_UNSUPPORTED);   // the pendulums' dispatch does not know the kind
    // any arguments: f is called for a combination validate() admits for one of the three kinds, or not at all
    for (int it = 0; it < 20000; it++) {
      const int pick = (int)(rnd() % 3);
      lde_problem_desc d = pick == 0 ? cvs_desc() : pick == 1 ? dpend_desc() : kuramoto_desc(2 + (int)(rnd() % 6));
      if (!(rnd() & 3)) d.state_dim = hostile_int();
      if (!(rnd() & 3)) d.rhs_kind = (rnd() & 1) ? hostile_int() : (int)(rnd() % 13);
      if (is_kuramoto(d)) d.param_dim = d.state_dim < std::numeric_limits<int>::max() ? d.state_dim + 1 : 1;
      if (is_dpend(d)) d.param_dim = 4;
      if (is_cvs(d)) d.param_dim = 2;
      d.solver = (rnd() & 1) ? hostile_int() : (int)(rnd() % 4);
      d.adaptive = (int)(rnd() % 2);
      d.dt = 0.05;
      int called = 0;
      const int rc = dir_system_dispatch(d, [&](auto, auto, auto) -> int { called++; return LDE_OK; });
      assert(called == (rc == LDE_OK) && (rc == LDE_OK || rc == LDE_ERR_UNSUPPORTED));
      if (is_dir(d)) assert(called == (validate(&d, &why) == LDE_OK));
      else assert(!called);
    }
  }
  // 7. hostile descriptions of the new kind: never a crash, always a status; an accepted one is one of the served combinations
  int accepted = 0;
  for (int it = 0; it < 20000; it++) {
    lde_problem_desc d = cvs_desc();
    const int nmut = 1 + (int)(rnd() % 3);
    for (int m = 0; m < nmut; m++) {
      switch (rnd() % 12) {
        case 0: d.abi_version = hostile_int(); break;
        case 1: d.rhs_kind = (rnd() & 1) ? hostile_int() : (int)(rnd() % 13); break;
        case 2: d.state_dim = hostile_int(); break;
        case 3: d.param_dim = hostile_int(); break;
        case 4: d.augment_dim = hostile_int(); break;
        case 5: d.n_layers = hostile_int(); break;
        case 6: d.solver = (rnd() & 1) ? hostile_int() : (int)(rnd() % 5); break;
        case 7: d.batching = hostile_int(); break;
        case 8: d.sensealg = (rnd() & 1) ? hostile_int() : (int)(rnd() % 6); break;
        case 9: d.adaptive = hostile_int(); break;
        case 10: d.maxiters = (int64_t)rnd() * ((rnd() & 1) ? 1 : -1); break;
        default: d.dt = (rnd() & 1) ? 0.05 : -1.0; break;
      }
    }
    why.clear();
    const int rc = validate(&d, &why);
    assert(rc == LDE_OK || rc == LDE_ERR_INVALID_ARG || rc == LDE_ERR_UNSUPPORTED);
    assert((rc == LDE_OK) == why.empty());
    assert((d.rhs_kind != 6 && d.rhs_kind != 8 && d.rhs_kind != 10 && d.rhs_kind != 12) || rc == LDE_ERR_INVALID_ARG);
    (void)num_weights(&d);
    (void)dual_partials(d);
    (void)dir_grid(d, hostile_int());
    if (rc == LDE_OK && is_cvs(d)) {
      accepted++;
      assert(d.state_dim == 4 && d.param_dim == 2 && d.augment_dim == 0 && d.n_layers == 0);
      assert(d.batching == LDE_BATCH_PER_TRAJECTORY && d.sensealg == LDE_SENSE_FORWARD_DUAL && num_weights(&d) == 0);
      assert(dir_system_dispatch(d, [&](auto, auto, auto) -> int { return LDE_OK; }) == LDE_OK);
      const int cap = rec_capacity(d, 0, 3, 0);
      assert(cap >= 1 && dual_rec_bytes(5, 3, cap, true, dual_partials(d)) >= 256 + 4 * 3 * (size_t)4 * 5 * 8);
    }
  }
  assert(accepted > 100);
  std::printf("cardiovascular system host logic under ASan + UBSan: validate, the group width, the launch shape, the dual record, the dispatch of all three systems and %d accepted of 20000 hostile descriptions checked\n", accepted);
  return 0;
}
