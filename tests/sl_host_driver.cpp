// sl_host_driver.cpp — what csrc/lde_host.h decides about the Stuart–Landau network (LDE_RHS_STUART_LANDAU) on the lane-per-direction
// kernels (csrc/lde_dual_dir.hip): validate() for the deterministic and the stochastic solves, the group width (G = 8 for N = 1, 16 for
// N = 2, 3), lanes / block / grid at the 4 096-lane threshold, dual_partials, the dual record for D = 2, 4, 6 (sizes, offsets, the last
// element of every array touched), the new dispatch layer (dir_all_dispatch(_n), dir_sde_dispatch) reaching exactly the served
// (N, solver, adaptive) combinations, and sde_plan — compiled with an ordinary host compiler under AddressSanitizer +
// UndefinedBehaviorSanitizer and run as a program by tests/test_sl_host.py.
#undef NDEBUG
#include <cassert>
#include <cmath>
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
  static const int v[] = {0, 1, -1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 15, 16, 64, 255, 256, 65536, std::numeric_limits<int>::max(), std::numeric_limits<int>::min(), -7, 1 << 30};
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
static lde_problem_desc sl_desc(int N) { return base_desc(LDE_RHS_STUART_LANDAU, 2 * N, 2 * N + 1); }
static lde_problem_desc sl_sde_desc(int N, int solver) {
  lde_problem_desc d = sl_desc(N);
  d.solver = solver; d.adaptive = 0; d.dt = 0.05;
  return d;
}
static lde_problem_desc cvs_desc() { return base_desc(LDE_RHS_CVS, 4, 2); }
static lde_problem_desc dpend_desc() { return base_desc(LDE_RHS_DOUBLE_PENDULUM, 4, 4); }
static lde_problem_desc kuramoto_desc(int N) { return base_desc(LDE_RHS_KURAMOTO, N, N + 1); }
static lde_problem_desc spend_desc() {
  lde_problem_desc d = base_desc(LDE_RHS_SPENDULUM, 2, 1);
  d.solver = LDE_SOLVER_EULER_HEUN; d.adaptive = 0; d.dt = 0.05;
  return d;
}

static size_t a256(size_t x) { return (x + 255) & ~size_t(255); }

int main() {
  std::string why;
  static_assert(LDE_RHS_STUART_LANDAU == 13 && LDE_RHS_CVS == 11 && LDE_RHS_DOUBLE_PENDULUM == 9 && LDE_RHS_KURAMOTO == 7 && LDE_ABI_VERSION == 1, "enum values; the ABI version did not move");
  const int SL = LDE_RHS_STUART_LANDAU, CV = LDE_RHS_CVS, DP = LDE_RHS_DOUBLE_PENDULUM, KU = LDE_RHS_KURAMOTO;
  const int TS = LDE_SOLVER_TSIT5, RK = LDE_SOLVER_RK4, EM = LDE_SOLVER_EM, EH = LDE_SOLVER_EULER_HEUN;

  // 1. the group: D = 2, 4, 6 with NP = 5, 9, 13 in 8, 16, 16 lanes; np = D·G/2 = 8, 32, 48; the other systems' rules are what they were
  static_assert(dir_group_width(SL, 2) == 8 && dir_partials(SL, 2) == 5 && dir_state_ok(SL, 2), "N = 1: five directions in eight lanes");
  static_assert(dir_group_width(SL, 4) == 16 && dir_partials(SL, 4) == 9 && dir_state_ok(SL, 4), "N = 2: nine directions in sixteen lanes");
  static_assert(dir_group_width(SL, 6) == 16 && dir_partials(SL, 6) == 13 && dir_state_ok(SL, 6), "N = 3: thirteen directions in sixteen lanes");
  static_assert(dir_group_width(CV, 4) == 8 && dir_partials(CV, 4) == 6 && dir_group_width(DP, 4) == 8 && dir_partials(DP, 4) == 8, "CVS and the double pendulum");
  for (int D = -3; D <= 20; D++) {
    if (D != 2 && D != 4 && D != 6) assert(dir_group_width(SL, D) == 0 && dir_partials(SL, D) == 0 && !dir_state_ok(SL, D));
    if (D != 4) assert(dir_group_width(CV, D) == 0 && dir_partials(CV, D) == 0 && !dir_state_ok(CV, D));
    if (D != 4) assert(dir_group_width(DP, D) == 0 && dir_partials(DP, D) == 0 && !dir_state_ok(DP, D));
    assert(dir_group_width(KU, D) == dir_group_width(D) && dir_partials(KU, D) == dir_partials(D) && dir_state_ok(KU, D) == dir_state_ok(D));
    for (int kind : {-1, 0, 1, 2, 3, 4, 5, 6, 8, 10, 12}) assert(dir_group_width(kind, D) == 0 && dir_partials(kind, D) == 0 && !dir_state_ok(kind, D));
  }
  for (int N = 1; N <= 3; N++) {
    const lde_problem_desc d = sl_desc(N);
    const int G = N == 1 ? 8 : 16, np = N == 1 ? 8 : N == 2 ? 32 : 48;
    assert(dir_group_width(d) == G && dual_partials(d) == np && dual_partials(d) * 2 == d.state_dim * dir_group_width(d));
    assert(is_sl(d) && is_dir(d) && !is_dir_sde(d) && !is_cvs(d) && !is_dpend(d) && !is_kuramoto(d) && !is_lv(d) && !has_pend(d) && !has_mlp(d) && !is_sde(d) && num_weights(&d) == 0);
    const lde_problem_desc s = sl_sde_desc(N, EH);
    assert(is_sl(s) && is_dir(s) && is_dir_sde(s) && !is_sde(s) && dual_partials(s) == np);
  }
  {
    const lde_problem_desc c = cvs_desc(), p = spend_desc();
    assert(is_dir(c) && !is_sl(c) && !is_dir_sde(c) && dual_partials(c) == 16);
    assert(is_sde(p) && !is_dir(p) && !is_dir_sde(p) && !is_sl(p) && has_pend(p));
  }

  // 2. the launch over B·G lanes: whole groups per workgroup, every lane covered, 64-lane workgroups up to 4 096 lanes, 256 beyond
  for (int N = 1; N <= 3; N++) {
    const lde_problem_desc d = sl_desc(N);
    const int G = dir_group_width(d);
    for (int B : {1, 2, 7, 8, 37, 255, 256, 257, 511, 512, 513, 4097, 65536, std::numeric_limits<int>::max()}) {
      const int block = dir_block(d, B);
      const int64_t lanes = dir_lanes(d, B), grid = dir_grid(d, B);
      assert(lanes == (int64_t)B * G && (block == 64 || block == 256) && block % G == 0);
      assert((block == 64) == (lanes <= 4096));
      assert(grid >= 1 && grid * block >= lanes && (grid - 1) * block < lanes);
    }
    assert(dir_lanes(d, 0) == 0 && dir_lanes(d, -5) == 0 && dir_grid(d, 0) == 0 && dir_block(d, 0) == 64);
    const int Bt = 4096 / G;   // 512 or 256 trajectories fill 4 096 lanes
    assert(dir_lanes(d, Bt) == 4096 && dir_block(d, Bt) == 64 && dir_grid(d, Bt) == 64);
    assert(dir_lanes(d, Bt + 1) == 4096 + G && dir_block(d, Bt + 1) == 256 && dir_grid(d, Bt + 1) == 17);
  }

  auto refused = [&](lde_problem_desc x, int status, const char* needle) {
    std::string w;
    return validate(&x, &w) == status && w.find(needle) != std::string::npos;
  };
  const int INV = LDE_ERR_INVALID_ARG, UNS = LDE_ERR_UNSUPPORTED;

  // 3. what validate() serves: the three deterministic combinations and the two stochastic solvers, for N = 1, 2, 3 …
  for (int N = 1; N <= 3; N++) {
    lde_problem_desc d = sl_desc(N);
    assert(validate(&d, &why) == LDE_OK);
    d.dt = 0.01;   // adaptive with a first step given
    assert(validate(&d, &why) == LDE_OK);
    d.adaptive = 0; d.dt = 0.05;
    assert(validate(&d, &why) == LDE_OK);
    d.solver = RK;
    assert(validate(&d, &why) == LDE_OK);
    for (int s : {EM, EH}) {
      d = sl_sde_desc(N, s);
      assert(validate(&d, &why) == LDE_OK);
    }
    std::vector<double> ts(50);
    for (int j = 0; j < 50; j++) ts[j] = 0.05 * j;
    KOpts o = make_opts(d, ts.data(), 50, 7);
    assert(o.T == 50 && o.B == 7 && o.adaptive == 0 && o.t_last == ts[49] && o.dt_fixed == 0.05);
    assert(rec_capacity(d, 0, 50, 0) == 200 && rec_nseq(d, 7) == 7);
  }
  // 4. … and what it refuses, with which status and text
  for (int N = 1; N <= 3; N++) {
    const lde_problem_desc d = sl_desc(N);
    const char* dims = "LDE_RHS_STUART_LANDAU needs state_dim=2N with 1 <= N <= 3, param_dim=2N+1, augment_dim=0";
    lde_problem_desc x = d;
    x.state_dim = 3; x.param_dim = 4; assert(refused(x, INV, dims));
    x = d; x.state_dim = 8; x.param_dim = 9; assert(refused(x, INV, dims));
    x = d; x.state_dim = 0; assert(refused(x, INV, "bad dims"));
    x = d; x.param_dim = 2 * N; assert(refused(x, INV, dims));
    x = d; x.param_dim = 2 * N + 2; assert(refused(x, INV, dims));
    x = d; x.augment_dim = 1; assert(refused(x, INV, dims));
    x = d; x.n_layers = 1; assert(refused(x, INV, "LDE_RHS_STUART_LANDAU is analytic: n_layers must be 0"));
    for (int kind : {6, 8, 10, 12, -1}) {   // still no right-hand sides (14 is not pinned: the next kind takes it)
      x = d; x.rhs_kind = kind; assert(refused(x, INV, "unknown rhs_kind"));
    }
    x = d; x.param_dim = 1; x.solver = EM; x.adaptive = 0; x.dt = 0.05; assert(refused(x, INV, dims));   // the dimension check comes before any solver check
    x = d; x.solver = 4; assert(refused(x, INV, "unknown solver"));
    for (int s : {LDE_SENSE_BACKSOLVE_CHECKPOINTED, LDE_SENSE_BACKSOLVE, LDE_SENSE_PARALLEL_CHECKPOINTED, LDE_SENSE_DISCRETE}) {
      x = d; x.sensealg = s; assert(refused(x, UNS, "LDE_RHS_STUART_LANDAU: only the solve on dual numbers exists") && refused(x, UNS, "use LDE_SENSE_FORWARD_DUAL"));
      x = sl_sde_desc(N, EH); x.sensealg = s; assert(refused(x, UNS, "use LDE_SENSE_FORWARD_DUAL"));
    }
    x = d; x.batching = LDE_BATCH_COUPLED; assert(refused(x, UNS, "LDE_RHS_STUART_LANDAU: no coupled solve; LDE_BATCH_PER_TRAJECTORY only"));
    x = sl_sde_desc(N, EM); x.batching = LDE_BATCH_COUPLED; assert(refused(x, UNS, "LDE_RHS_STUART_LANDAU: no coupled solve"));
    x = d; x.batching = LDE_BATCH_COUPLED_GLOBAL; assert(refused(x, INV, "LDE_BATCH_COUPLED_GLOBAL needs an MLP"));
    x = d; x.solver = RK; assert(refused(x, UNS, "RK4 is fixed-step only"));
    for (int s : {EM, EH}) {   // the stochastic solvers under the stochastic pendulum's conditions
      x = sl_sde_desc(N, s); x.adaptive = 1; assert(refused(x, UNS, "LDE_RHS_STUART_LANDAU: no adaptive stochastic stepping"));
      x = sl_sde_desc(N, s); x.dt = 0; assert(refused(x, UNS, "pass a finite dt > 0"));
      x = sl_sde_desc(N, s); x.dt = -1; assert(refused(x, UNS, "pass a finite dt > 0"));
      x = sl_sde_desc(N, s); x.dt = std::numeric_limits<double>::infinity(); assert(refused(x, UNS, "pass a finite dt > 0"));
      x = sl_sde_desc(N, s); x.dt = std::nan(""); assert(refused(x, UNS, "pass a finite dt > 0"));
    }
    x = d; x.adaptive = 0; x.dt = 0; assert(refused(x, INV, "dt>0"));
    x = d; x.maxiters = 0; assert(refused(x, INV, "maxiters"));
  }
  // every other kind still refuses the stochastic steppers with its old text (the stochastic pendulum is still served)
  for (int s : {EM, EH}) {
    auto with = [&](lde_problem_desc x) { x.solver = s; x.adaptive = 0; x.dt = 0.05; return x; };
    assert(refused(with(cvs_desc()), UNS, "LDE_SOLVER_EM / LDE_SOLVER_EULER_HEUN are stochastic steppers: LDE_RHS_SPENDULUM only"));
    assert(refused(with(dpend_desc()), UNS, "LDE_SOLVER_EM / LDE_SOLVER_EULER_HEUN are stochastic steppers: LDE_RHS_SPENDULUM only"));
    assert(refused(with(kuramoto_desc(3)), UNS, "LDE_SOLVER_EM / LDE_SOLVER_EULER_HEUN are stochastic steppers: LDE_RHS_SPENDULUM only"));
    assert(refused(with(base_desc(LDE_RHS_LOTKA_VOLTERRA, 2, 4)), UNS, "LDE_SOLVER_EM / LDE_SOLVER_EULER_HEUN are stochastic steppers: LDE_RHS_SPENDULUM only"));
    assert(refused(with(base_desc(LDE_RHS_PENDULUM, 2, 1)), UNS, "LDE_SOLVER_EM / LDE_SOLVER_EULER_HEUN are stochastic steppers: LDE_RHS_SPENDULUM only"));
    assert(refused(with(base_desc(LDE_RHS_PENDULUM_FRICTION, 2, 1)), UNS, "LDE_SOLVER_EM / LDE_SOLVER_EULER_HEUN are stochastic steppers: LDE_RHS_SPENDULUM only"));
    lde_problem_desc p = with(spend_desc());
    assert(validate(&p, &why) == LDE_OK);
  }
  {
    lde_problem_desc p = spend_desc();
    p.solver = TS; assert(refused(p, UNS, "LDE_RHS_SPENDULUM: no deterministic solver"));
  }

  // 5. the dual record — n [B] | J [T][D][B][G] | t, dt [cap][B] for D = 2, 4, 6: consecutive, 256-byte aligned, inside the bytes, no overlap; the
  //    last element of every array — and the last element a lane of the kernels indexes, a pad lane's — touched (an overrun is an ASan report)
  for (int N = 1; N <= 3; N++) {
    const lde_problem_desc d = sl_desc(N);
    const int D = 2 * N, G = dir_group_width(d), np = dual_partials(d);
    for (int B : {1, 3, 37, 64, 257, 513})
      for (int T : {1, 2, 9, 50})
        for (int cap : {1, 64, 200})
          for (int trace = 0; trace < 2; trace++) {
            const size_t nJ = (size_t)T * D * B * G;
            const size_t bytes = dual_rec_bytes(B, T, cap, trace != 0, np);
            assert(bytes == a256((size_t)4 * B) + a256(4 * nJ) + (trace ? 2 * a256((size_t)8 * cap * B) : 0));
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

  // 6. the new dispatch layer. Deterministic: all four systems × exactly (Tsit5 adaptive, Tsit5 fixed-step, RK4 fixed-step) reach the kernels
  //    through dir_all_dispatch; the three-system forms do not know the Stuart–Landau network. Stochastic: dir_sde_dispatch reaches exactly
  //    (D = 2, 4, 6) × (EM, EulerHeun) with adaptive = 0, and nothing else.
  {
    int seen[14][8][2] = {};
    auto rec = [&](auto kind, auto n, auto S) -> int {
      static_assert((decltype(kind)::value == LDE_RHS_KURAMOTO && decltype(n)::value >= 2 && decltype(n)::value <= 7) ||
                        ((decltype(kind)::value == LDE_RHS_DOUBLE_PENDULUM || decltype(kind)::value == LDE_RHS_CVS) && decltype(n)::value == 4) ||
                        (decltype(kind)::value == LDE_RHS_STUART_LANDAU && (decltype(n)::value == 2 || decltype(n)::value == 4 || decltype(n)::value == 6)), "the system");
      static_assert(decltype(S)::value == LDE_SOLVER_TSIT5 || decltype(S)::value == LDE_SOLVER_RK4, "SOLVER");
      static_assert(dir_group_width(decltype(kind)::value, decltype(n)::value) >= dir_partials(decltype(kind)::value, decltype(n)::value), "NP <= G");
      seen[kind][n][S]++;
      return 1000 * kind + 10 * n + S;
    };
    auto with = [](lde_problem_desc d, int solver, int adaptive) { d.solver = solver; d.adaptive = adaptive; d.dt = 0.05; return d; };
    for (int N = 1; N <= 3; N++) {
      const lde_problem_desc d = sl_desc(N);
      const int D = 2 * N;
      assert(dir_all_dispatch(with(d, TS, 1), rec) == 13000 + 10 * D && dir_all_dispatch(with(d, TS, 0), rec) == 13000 + 10 * D && dir_all_dispatch(with(d, RK, 0), rec) == 13001 + 10 * D);
      assert(dir_all_dispatch(with(d, RK, 1), rec) == UNS);
      assert(dir_all_dispatch(with(d, EM, 0), rec) == UNS && dir_all_dispatch(with(d, EH, 0), rec) == UNS);   // the stochastic solvers have a dispatch of their own
      assert(seen[SL][D][0] == 2 && seen[SL][D][1] == 1);
      assert(dir_all_dispatch_n(d, [&](auto kind, auto n) -> int { return 100 * kind + n; }) == 1300 + D);
      lde_problem_desc x = d;
      x.state_dim = 3; assert(dir_all_dispatch(x, rec) == UNS && dir_all_dispatch_n(x, [&](auto, auto) -> int { return LDE_OK; }) == UNS);
      x.state_dim = 8; assert(dir_all_dispatch(x, rec) == UNS);
      assert(dir_system_dispatch_n(d, [&](auto, auto) -> int { return LDE_OK; }) == UNS && dir_dispatch_n(d, [&](auto, auto) -> int { return LDE_OK; }) == UNS);
    }
    {
      const lde_problem_desc c = cvs_desc(), p = dpend_desc();
      assert(dir_all_dispatch(with(c, TS, 1), rec) == 11040 && dir_all_dispatch(with(c, RK, 0), rec) == 11041 && dir_all_dispatch(with(c, RK, 1), rec) == UNS);
      assert(dir_all_dispatch(with(p, TS, 1), rec) == 9040 && dir_all_dispatch(with(p, RK, 0), rec) == 9041);
      assert(dir_all_dispatch_n(c, [&](auto kind, auto n) -> int { return 100 * kind + n; }) == 1104);
    }
    for (int N = 2; N <= 7; N++) {
      const lde_problem_desc d = kuramoto_desc(N);
      assert(dir_all_dispatch(with(d, TS, 1), rec) == 7000 + 10 * N && dir_all_dispatch(with(d, RK, 0), rec) == 7001 + 10 * N);
      assert(dir_all_dispatch_n(d, [&](auto kind, auto n) -> int { return 100 * kind + n; }) == 700 + N);
    }
    for (int kind : {0, 1, 2, 3, 4, 5, 6, 8, 10, 12, 14, -1}) {
      lde_problem_desc d = sl_desc(2);
      d.rhs_kind = kind;
      assert(dir_all_dispatch(d, rec) == UNS && dir_all_dispatch_n(d, [&](auto, auto) -> int { return LDE_OK; }) == UNS);
    }
    // the stochastic dispatch
    int sseen[8][4] = {};
    auto srec = [&](auto n, auto S) -> int {
      static_assert(decltype(n)::value == 2 || decltype(n)::value == 4 || decltype(n)::value == 6, "D");
      static_assert(decltype(S)::value == LDE_SOLVER_EM || decltype(S)::value == LDE_SOLVER_EULER_HEUN, "SOLVER");
      sseen[n][S]++;
      return 10 * n + S;
    };
    for (int N = 1; N <= 3; N++) {
      const int D = 2 * N;
      assert(dir_sde_dispatch(sl_sde_desc(N, EM), srec) == 10 * D + EM && dir_sde_dispatch(sl_sde_desc(N, EH), srec) == 10 * D + EH);
      assert(sseen[D][EM] == 1 && sseen[D][EH] == 1);
      lde_problem_desc x = sl_sde_desc(N, EM);
      x.adaptive = 1; assert(dir_sde_dispatch(x, srec) == UNS);
      x = sl_sde_desc(N, EH); x.state_dim = 3; assert(dir_sde_dispatch(x, srec) == UNS);
      x.state_dim = 8; assert(dir_sde_dispatch(x, srec) == UNS);
      assert(dir_sde_dispatch(with(sl_desc(N), TS, 0), srec) == UNS && dir_sde_dispatch(with(sl_desc(N), RK, 0), srec) == UNS);
    }
    assert(dir_sde_dispatch(spend_desc(), srec) == UNS && dir_sde_dispatch(with(cvs_desc(), EM, 0), srec) == UNS && dir_sde_dispatch(with(kuramoto_desc(2), EH, 0), srec) == UNS);
    assert(pend_dispatch(SL, TS, true, [&](auto, auto, auto) -> int { return LDE_OK; }) == UNS);   // the pendulums' dispatch does not know the kind
    // any arguments: f is called for a combination validate() admits, or not at all
    for (int it = 0; it < 20000; it++) {
      const int pick = (int)(rnd() % 4);
      lde_problem_desc d = pick == 0 ? cvs_desc() : pick == 1 ? dpend_desc() : pick == 2 ? kuramoto_desc(2 + (int)(rnd() % 6)) : sl_desc(1 + (int)(rnd() % 3));
      if (!(rnd() & 3)) d.state_dim = hostile_int();
      if (!(rnd() & 3)) d.rhs_kind = (rnd() & 1) ? hostile_int() : (int)(rnd() % 15);
      if (is_kuramoto(d) || is_sl(d)) d.param_dim = d.state_dim < std::numeric_limits<int>::max() ? d.state_dim + 1 : 1;
      if (is_dpend(d)) d.param_dim = 4;
      if (is_cvs(d)) d.param_dim = 2;
      d.solver = (rnd() & 1) ? hostile_int() : (int)(rnd() % 4);
      d.adaptive = (int)(rnd() % 2);
      d.dt = 0.05;
      int called = 0, scalled = 0;
      const int rc = dir_all_dispatch(d, [&](auto, auto, auto) -> int { called++; return LDE_OK; });
      const int src = dir_sde_dispatch(d, [&](auto, auto) -> int { scalled++; return LDE_OK; });
      assert(called == (rc == LDE_OK) && (rc == LDE_OK || rc == UNS) && scalled == (src == LDE_OK) && (src == LDE_OK || src == UNS));
      assert(called + scalled <= 1);
      if (is_dir(d)) assert(called + scalled == (validate(&d, &why) == LDE_OK));
      else assert(!called && !scalled);
      if (scalled) assert(is_dir_sde(d) && !d.adaptive);
    }
  }

  // 7. sde_plan on a description of this kind: the stochastic pendulum's substep rule — n_j = max(1, ceil(D_j/dt − 1e-9)), capped at maxiters
  {
    lde_problem_desc d = sl_sde_desc(3, EH);
    std::vector<double> ts(50);
    for (int j = 0; j < 50; j++) ts[j] = 0.05 * j;
    SdePlan p = sde_plan(d, ts.data(), 50);
    assert(p.N == 49 && !p.over);
    d.dt = 0.0125; p = sde_plan(d, ts.data(), 50); assert(p.N == 196 && !p.over);
    d.dt = 0.05; d.maxiters = 49; p = sde_plan(d, ts.data(), 50); assert(p.N == 49 && !p.over);
    d.maxiters = 48; p = sde_plan(d, ts.data(), 50); assert(p.N == 48 && p.over);
    d.maxiters = 100000;
    const double rg[4] = {0.0, 0.01, 0.13, 0.19};   // 1, 3 and 2 unequal substeps
    p = sde_plan(d, rg, 4); assert(p.N == 6 && !p.over);
    assert(lde::sde_substeps(0.01, 0.05) == 1 && lde::sde_substeps(0.12, 0.05) == 3 && lde::sde_substeps(0.1, 0.05) == 2 && lde::sde_substeps(1e30, 0.05) == 1000000000);
    p = sde_plan(d, ts.data(), 1); assert(p.N == 0 && !p.over);
    const double huge[3] = {0.0, 1e30, 2e30};
    p = sde_plan(d, huge, 3); assert(p.over && p.N == 100000);
  }

  // 8. hostile descriptions of the new kind: never a crash, always a status; an accepted one is one of the served combinations
  int accepted = 0, accepted_sde = 0;
  for (int it = 0; it < 20000; it++) {
    lde_problem_desc d = (rnd() & 1) ? sl_desc(1 + (int)(rnd() % 3)) : sl_sde_desc(1 + (int)(rnd() % 3), (rnd() & 1) ? EM : EH);
    const int nmut = 1 + (int)(rnd() % 3);
    for (int m = 0; m < nmut; m++) {
      switch (rnd() % 12) {
        case 0: d.abi_version = hostile_int(); break;
        case 1: d.rhs_kind = (rnd() & 1) ? hostile_int() : (int)(rnd() % 15); break;
        case 2: d.state_dim = hostile_int(); break;
        case 3: d.param_dim = hostile_int(); break;
        case 4: d.augment_dim = hostile_int(); break;
        case 5: d.n_layers = hostile_int(); break;
        case 6: d.solver = (rnd() & 1) ? hostile_int() : (int)(rnd() % 5); break;
        case 7: d.batching = hostile_int(); break;
        case 8: d.sensealg = (rnd() & 1) ? hostile_int() : (int)(rnd() % 6); break;
        case 9: d.adaptive = hostile_int(); break;
        case 10: d.maxiters = (int64_t)rnd() * ((rnd() & 1) ? 1 : -1); break;
        default: d.dt = (rnd() & 1) ? 0.05 : (rnd() & 1) ? -1.0 : std::numeric_limits<double>::infinity(); break;
      }
    }
    why.clear();
    const int rc = validate(&d, &why);
    assert(rc == LDE_OK || rc == INV || rc == UNS);
    assert((rc == LDE_OK) == why.empty());
    assert((d.rhs_kind != 6 && d.rhs_kind != 8 && d.rhs_kind != 10 && d.rhs_kind != 12) || rc == INV);
    (void)num_weights(&d);
    (void)dual_partials(d);
    (void)dir_grid(d, hostile_int());
    if (rc == LDE_OK && is_sl(d)) {
      assert((d.state_dim == 2 || d.state_dim == 4 || d.state_dim == 6) && d.param_dim == d.state_dim + 1 && d.augment_dim == 0 && d.n_layers == 0);
      assert(d.batching == LDE_BATCH_PER_TRAJECTORY && d.sensealg == LDE_SENSE_FORWARD_DUAL && num_weights(&d) == 0);
      const int det = dir_all_dispatch(d, [&](auto, auto, auto) -> int { return LDE_OK; }), sde = dir_sde_dispatch(d, [&](auto, auto) -> int { return LDE_OK; });
      if (is_dir_sde(d)) {
        accepted_sde++;
        assert(sde == LDE_OK && det == UNS && !d.adaptive && d.dt > 0 && std::isfinite(d.dt));
        const double ts[3] = {0.0, 0.05, 0.1};
        const SdePlan p = sde_plan(d, ts, 3);
        assert(p.N >= 1 && p.N <= std::max<int64_t>(d.maxiters, 0));
      } else {
        accepted++;
        assert(det == LDE_OK && sde == UNS);
      }
      const int cap = rec_capacity(d, 0, 3, 0);
      assert(cap >= 1 && dual_rec_bytes(5, 3, cap, true, dual_partials(d)) >= 256 + 4 * 3 * (size_t)d.state_dim * 5 * dir_group_width(d));
    }
  }
  assert(accepted > 100 && accepted_sde > 100);
  std::printf("Stuart-Landau host logic under ASan + UBSan: validate, the group width, the launch shape, the dual record for D = 2, 4, 6, the dispatch of all four systems, the stochastic dispatch, sde_plan and %d + %d accepted of 20000 hostile descriptions checked\n", accepted, accepted_sde);
  return 0;
}
