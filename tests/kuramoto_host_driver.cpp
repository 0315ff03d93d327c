// kuramoto_host_driver.cpp — what csrc/lde_host.h decides about the Kuramoto right-hand side (LDE_RHS_KURAMOTO) and its lane-per-direction
// kernels (csrc/lde_dual_dir.hip): the group-width rule, the launch shape over B·G lanes, the dual record of every N (sizes, offsets,
// alignment, no overlap, the last element of every array touched), the dispatch of the kernels' template arguments, and which descriptions
// validate() serves and refuses with what text — compiled with an ordinary host compiler under AddressSanitizer +
// UndefinedBehaviorSanitizer and run as a program by tests/test_kuramoto_host.py.
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
  static const int v[] = {0, 1, -1, 2, 3, 4, 5, 6, 7, 8, 9, 15, 16, 64, 255, 256, 65536, std::numeric_limits<int>::max(), std::numeric_limits<int>::min(), -7, 1 << 30};
  return (rnd() & 3) ? v[rnd() % (sizeof(v) / sizeof(v[0]))] : (int)(uint32_t)rnd();
}
static double hostile_double() {
  static const double v[] = {0.0, -0.0, 1.0, -1.0, 1e-300, 1e300, -1e300, 0.05, 1e-6, std::numeric_limits<double>::infinity(),
                             -std::numeric_limits<double>::infinity(), std::numeric_limits<double>::quiet_NaN(), std::numeric_limits<double>::denorm_min()};
  return v[rnd() % (sizeof(v) / sizeof(v[0]))];
}

static lde_problem_desc kuramoto_desc(int N) {
  lde_problem_desc d{};
  d.abi_version = LDE_ABI_VERSION;
  d.rhs_kind = LDE_RHS_KURAMOTO;
  d.state_dim = N;
  d.param_dim = N + 1;
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
  static_assert(LDE_RHS_KURAMOTO == 7 && LDE_RHS_LOTKA_VOLTERRA == 5 && LDE_ABI_VERSION == 1, "enum values; the ABI version did not move");

  // 1. the group-width rule: NP = 2N + 1 directions fit G lanes, G divides a 16-lane row, N outside 2 … 7 has no group
  for (int N = -3; N <= 20; N++) {
    const int G = dir_group_width(N), NP = dir_partials(N);
    if (N < 2 || N > 7) {
      assert(G == 0 && NP == 0 && !dir_state_ok(N));
      continue;
    }
    assert(dir_state_ok(N) && NP == 2 * N + 1 && G == (N <= 3 ? 8 : 16) && NP <= G && 16 % G == 0 && 64 % G == 0);
    assert(G - NP == (N == 2 ? 3 : N == 3 ? 1 : 15 - 2 * N));   // pad lanes: 3, 1 | 7, 5, 3, 1
  }
  assert(dir_group_width(std::numeric_limits<int>::max()) == 0 && dir_group_width(std::numeric_limits<int>::min()) == 0);

  // 2. the launch over B·G lanes: whole groups per workgroup, every lane of the batch covered, the 64- / 256-lane threshold at 4 096 lanes,
  //    no overflow at the largest batch an int holds
  for (int N = 2; N <= 7; N++) {
    const int G = dir_group_width(N);
    for (int B : {1, 2, 7, 8, 37, 255, 256, 257, 4096 / G - 1, 4096 / G, 4096 / G + 1, 4097, 65536, std::numeric_limits<int>::max()}) {
      const int block = dir_block(N, B);
      const int64_t lanes = dir_lanes(N, B), grid = dir_grid(N, B);
      assert(lanes == (int64_t)B * G && (block == 64 || block == 256) && block % G == 0);
      assert((block == 64) == (lanes <= 4096));
      assert(grid >= 1 && grid * block >= lanes && (grid - 1) * block < lanes);
    }
    assert(dir_lanes(N, 0) == 0 && dir_lanes(N, -5) == 0 && dir_grid(N, 0) == 0);
    assert(dir_block(N, 4096 / G) == 64 && dir_block(N, 4096 / G + 1) == 256);
  }

  // 3. what validate() serves: every N of 2 … 7 × {Tsit5 adaptive, Tsit5 fixed-step, RK4 fixed-step}
  for (int N = 2; N <= 7; N++) {
    lde_problem_desc d = kuramoto_desc(N);
    assert(validate(&d, &why) == LDE_OK);
    d.dt = 0.01;   // adaptive with a first step given
    assert(validate(&d, &why) == LDE_OK);
    d.adaptive = 0; d.dt = 0.05;
    assert(validate(&d, &why) == LDE_OK);
    d.solver = LDE_SOLVER_RK4;
    assert(validate(&d, &why) == LDE_OK);
    assert(num_weights(&d) == 0 && is_kuramoto(d) && !is_lv(d) && !has_pend(d) && !has_mlp(d) && !is_sde(d));
    assert(dual_partials(d) * 2 == N * dir_group_width(N));
    std::vector<double> ts(50);
    for (int j = 0; j < 50; j++) ts[j] = 0.05 * j;
    KOpts o = make_opts(d, ts.data(), 50, 7);
    assert(o.T == 50 && o.B == 7 && o.adaptive == 0 && o.t_last == ts[49]);
    assert(rec_capacity(d, 0, 50, 0) == 200 && rec_nseq(d, 7) == 7);
  }
  // … and the other kinds are what they were: the new kind is no pendulum
  {
    lde_problem_desc p = kuramoto_desc(2);
    p.rhs_kind = LDE_RHS_PENDULUM; p.param_dim = 1;
    assert(validate(&p, &why) == LDE_OK && has_pend(p) && !is_kuramoto(p) && dual_partials(p) == 3);
    p.rhs_kind = LDE_RHS_LOTKA_VOLTERRA; p.param_dim = 4;
    assert(validate(&p, &why) == LDE_OK && !has_pend(p) && is_lv(p) && dual_partials(p) == 6);
  }
  // 4. what it refuses, with which status and text
  {
    const lde_problem_desc d = kuramoto_desc(3);
    auto refused = [&](lde_problem_desc x, int status, const char* needle) {
      std::string w;
      return validate(&x, &w) == status && w.find(needle) != std::string::npos;
    };
    const int INV = LDE_ERR_INVALID_ARG, UNS = LDE_ERR_UNSUPPORTED;
    const char* dims = "LDE_RHS_KURAMOTO needs state_dim=N with 2 <= N <= 7, param_dim=N+1, augment_dim=0";
    lde_problem_desc x = d;
    x.state_dim = 1; x.param_dim = 2; assert(refused(x, INV, dims));
    x = d; x.state_dim = 8; x.param_dim = 9; assert(refused(x, INV, dims));
    x = d; x.state_dim = 0; x.param_dim = 1; assert(refused(x, INV, "bad dims"));
    x = d; x.param_dim = 3; assert(refused(x, INV, dims));
    x = d; x.param_dim = 5; assert(refused(x, INV, dims));
    x = d; x.augment_dim = 1; assert(refused(x, INV, dims));
    x = d; x.n_layers = 1; assert(refused(x, INV, "LDE_RHS_KURAMOTO is analytic: n_layers must be 0"));
    x = d; x.rhs_kind = 6; assert(refused(x, INV, "unknown rhs_kind"));   // 6 is still no right-hand side
    x = d; x.rhs_kind = 8; assert(refused(x, INV, "unknown rhs_kind"));
    x = d; x.rhs_kind = -1; assert(refused(x, INV, "unknown rhs_kind"));
    // the dimension check comes before any solver check
    x = d; x.param_dim = 1; x.solver = LDE_SOLVER_EM; assert(refused(x, INV, dims));
    x = d; x.solver = 4; assert(refused(x, INV, "unknown solver"));
    for (int s : {LDE_SENSE_BACKSOLVE_CHECKPOINTED, LDE_SENSE_BACKSOLVE, LDE_SENSE_PARALLEL_CHECKPOINTED, LDE_SENSE_DISCRETE}) {
      x = d; x.sensealg = s; assert(refused(x, UNS, "LDE_RHS_KURAMOTO") && refused(x, UNS, "use LDE_SENSE_FORWARD_DUAL"));
    }
    x = d; x.batching = LDE_BATCH_COUPLED; assert(refused(x, UNS, "LDE_RHS_KURAMOTO: no coupled solve; LDE_BATCH_PER_TRAJECTORY only"));
    x = d; x.batching = LDE_BATCH_COUPLED_GLOBAL; assert(refused(x, INV, "LDE_BATCH_COUPLED_GLOBAL needs an MLP"));
    for (int s : {LDE_SOLVER_EM, LDE_SOLVER_EULER_HEUN}) {   // the stochastic steppers keep their refusal
      x = d; x.solver = s; x.adaptive = 0; x.dt = 0.05; assert(refused(x, UNS, "LDE_RHS_SPENDULUM only"));
    }
    x = d; x.solver = LDE_SOLVER_RK4; assert(refused(x, UNS, "RK4 is fixed-step only"));   // adaptive RK4 keeps its refusal
    x = d; x.adaptive = 0; x.dt = 0; assert(refused(x, INV, "dt>0"));
    x = d; x.maxiters = 0; assert(refused(x, INV, "maxiters"));
  }
  // 5. the dual record of every N — n [B] | J [T][N][B][G] | t, dt [cap][B]: consecutive, 256-byte aligned, inside the bytes, no overlap;
  //    the last element of every array — and the last element a lane of the kernels indexes — touched (an overrun is an ASan report)
  for (int N = 2; N <= 7; N++) {
    const lde_problem_desc d = kuramoto_desc(N);
    const int G = dir_group_width(N), np = dual_partials(d);
    for (int B : {1, 3, 37, 64, 257, 1025})
      for (int T : {1, 2, 9, 50})
        for (int cap : {1, 64, 200})
          for (int trace = 0; trace < 2; trace++) {
            const size_t nJ = (size_t)T * N * B * G;
            const size_t bytes = dual_rec_bytes(B, T, cap, trace != 0, np);
            assert(bytes == a256((size_t)4 * B) + a256(4 * nJ) + (trace ? 2 * a256((size_t)8 * cap * B) : 0));
            std::vector<unsigned char> buf(bytes + 256);
            unsigned char* base = (unsigned char*)(((uintptr_t)buf.data() + 255) & ~(uintptr_t)255);
            DualRec r = dual_rec_view(base, B, T, cap, trace != 0, np);
            assert((unsigned char*)r.n == base && (unsigned char*)r.J == base + a256((size_t)4 * B) && ((uintptr_t)r.J & 255) == 0);
            assert((unsigned char*)(r.n + B) <= (unsigned char*)r.J);
            r.n[B - 1] = 1;
            // the kernels' index of (j, i, b, q) = (T − 1, N − 1, B − 1, G − 1): the last float of J
            const size_t last = (((size_t)(T - 1) * N + (N - 1)) * B + (B - 1)) * G + (G - 1);
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
  // 6. the kernels' template arguments: N = 2 … 7 × exactly (Tsit5 adaptive, Tsit5 fixed-step, RK4 fixed-step) reach the kernels
  {
    int seen[8][2] = {};
    auto rec = [&](auto n, auto S) -> int {
      static_assert(decltype(n)::value >= 2 && decltype(n)::value <= 7, "N");
      static_assert(decltype(S)::value == LDE_SOLVER_TSIT5 || decltype(S)::value == LDE_SOLVER_RK4, "SOLVER");
      seen[n][S]++;
      return 100 * n + S;
    };
    const int TS = LDE_SOLVER_TSIT5, RK = LDE_SOLVER_RK4;
    for (int N = 2; N <= 7; N++) {
      assert(dir_dispatch(N, TS, true, rec) == 100 * N && dir_dispatch(N, TS, false, rec) == 100 * N && dir_dispatch(N, RK, false, rec) == 100 * N + 1);
      assert(dir_dispatch(N, RK, true, rec) == LDE_ERR_UNSUPPORTED);   // adaptive RK4
      assert(dir_dispatch(N, LDE_SOLVER_EM, false, rec) == LDE_ERR_UNSUPPORTED && dir_dispatch(N, LDE_SOLVER_EULER_HEUN, false, rec) == LDE_ERR_UNSUPPORTED);
      assert(seen[N][0] == 2 && seen[N][1] == 1);
      assert(dir_dispatch_n(N, [&](auto n) -> int { return n; }) == N);
    }
    for (int N : {-1, 0, 1, 8, 16, std::numeric_limits<int>::max()}) {
      assert(dir_dispatch(N, TS, true, rec) == LDE_ERR_UNSUPPORTED);
      assert(dir_dispatch_n(N, [&](auto) -> int { return LDE_OK; }) == LDE_ERR_UNSUPPORTED);
    }
    // the pendulums' dispatch does not know the kind
    assert(pend_dispatch(LDE_RHS_KURAMOTO, TS, true, [&](auto, auto, auto) -> int { return LDE_OK; }) == LDE_ERR_UNSUPPORTED);
    // any arguments: f is called for a combination validate() admits for this kind, or not at all
    for (int it = 0; it < 20000; it++) {
      const int N = (rnd() & 3) ? 2 + (int)(rnd() % 6) : hostile_int();
      lde_problem_desc d = kuramoto_desc(3);
      d.state_dim = N;
      d.param_dim = N < std::numeric_limits<int>::max() ? N + 1 : 1;   // (N + 1 must not overflow in THIS program)
      d.solver = (rnd() & 1) ? hostile_int() : (int)(rnd() % 4);
      d.adaptive = (int)(rnd() % 2);
      d.dt = 0.05;
      int called = 0;
      const int rc = dir_dispatch(d.state_dim, d.solver, d.adaptive != 0, [&](auto, auto) -> int { called++; return LDE_OK; });
      assert(called == (rc == LDE_OK) && (rc == LDE_OK || rc == LDE_ERR_UNSUPPORTED));
      assert(called == (validate(&d, &why) == LDE_OK));
    }
  }
  // 7. hostile descriptions of the new kind: never a crash, always a status; an accepted one is one of the served combinations
  int accepted = 0;
  for (int it = 0; it < 20000; it++) {
    lde_problem_desc d = kuramoto_desc(2 + (int)(rnd() % 6));
    const int nmut = 1 + (int)(rnd() % 4);
    for (int m = 0; m < nmut; m++) {
      switch (rnd() % 22) {
        case 0: d.abi_version = hostile_int(); break;
        case 1: d.rhs_kind = (rnd() & 1) ? hostile_int() : (int)(rnd() % 9); break;
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
    assert(d.rhs_kind != 6 || rc == LDE_ERR_INVALID_ARG);
    (void)num_weights(&d);
    (void)dual_partials(d);
    if (rc == LDE_OK && is_kuramoto(d)) {
      accepted++;
      assert(d.state_dim >= 2 && d.state_dim <= 7 && d.param_dim == d.state_dim + 1 && d.augment_dim == 0 && d.n_layers == 0);
      assert(d.batching == LDE_BATCH_PER_TRAJECTORY && d.sensealg == LDE_SENSE_FORWARD_DUAL && num_weights(&d) == 0);
      assert(dir_dispatch(d.state_dim, d.solver, d.adaptive != 0, [&](auto, auto) -> int { return LDE_OK; }) == LDE_OK);
      const double ts[3] = {0.0, 0.5, 1.0};
      const KOpts o = make_opts(d, ts, 3, 5);
      assert(o.T == 3 && o.B == 5);
      const int cap = rec_capacity(d, 0, 3, 0);
      const size_t G = (size_t)dir_group_width(d.state_dim);
      assert(cap >= 1 && dual_rec_bytes(5, 3, cap, true, dual_partials(d)) >= 256 + 4 * 3 * (size_t)d.state_dim * 5 * G);
    }
  }
  assert(accepted > 100);
  std::printf("kuramoto host logic under ASan + UBSan: the group width, the launch shape, the dual record of every N, the dispatch, validate and %d accepted of 20000 hostile descriptions checked\n", accepted);
  return 0;
}
