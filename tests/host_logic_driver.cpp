// host_logic_driver.cpp — the C ABI's host-side logic (latentdiffeq.jl_amd/csrc/lde_host.h: what lde_api.hip does BEFORE it touches the
// device) under AddressSanitizer + UndefinedBehaviorSanitizer, driven with well-formed and hostile inputs. Built and run by
// tests/test_sanitizers.py (g++; no HIP, no GPU). A C ABI's arguments come from another language's runtime: every field of a problem
// description is an int or a double somebody else filled in.
#include <cassert>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../latentdiffeq.jl_amd/csrc/lde_host.h"

using namespace lde_host;

static unsigned long long rs = 0x9E3779B97F4A7C15ULL;
static unsigned long long rnd() { rs ^= rs << 13; rs ^= rs >> 7; rs ^= rs << 17; return rs; }
static int hostile_int() {
  static const int v[] = {0, 1, -1, 2, 6, 7, 8, 64, 255, 256, 1024, 1025, 1 << 20, std::numeric_limits<int>::max(), std::numeric_limits<int>::min(), -7};
  return (rnd() & 3) ? v[rnd() % (sizeof(v) / sizeof(v[0]))] : (int)rnd();
}
static double hostile_double() {
  static const double v[] = {0.0, -0.0, 1e-6, 1e-3, 1.0, -1.0, 1e300, -1e300, 1e-320, std::numeric_limits<double>::infinity(),
                             -std::numeric_limits<double>::infinity(), std::numeric_limits<double>::quiet_NaN(), 0.05, 0.2, 10.0, 0.9};
  return v[rnd() % (sizeof(v) / sizeof(v[0]))];
}

static lde_problem_desc good() {
  lde_problem_desc d;
  std::memset(&d, 0, sizeof(d));
  d.abi_version = LDE_ABI_VERSION; d.rhs_kind = LDE_RHS_PENDULUM; d.state_dim = 2; d.param_dim = 1; d.solver = LDE_SOLVER_TSIT5;
  d.sensealg = LDE_SENSE_DISCRETE; d.adaptive = 1; d.maxiters = 100000; d.abstol = 1e-6; d.reltol = 1e-3; d.qmin = 0.2; d.qmax = 10; d.gamma = 0.9;
  d.beta1 = 0.14; d.beta2 = 0.08;
  return d;
}

int main() {
  int n_ok = 0, n_bad = 0;
  std::string why;
  // 1. well-formed descriptions of every family validate; their derived quantities are what include/lde.h says
  {
    lde_problem_desc d = good();
    assert(validate(&d, &why) == LDE_OK && num_weights(&d) == 0);
    d.rhs_kind = LDE_RHS_MLP; d.state_dim = 16; d.param_dim = 0; d.n_layers = 3; d.batching = LDE_BATCH_COUPLED;
    const int s[4] = {16, 200, 200, 16};
    for (int i = 0; i < 4; i++) d.layer_sizes[i] = s[i];
    assert(validate(&d, &why) == LDE_OK && num_weights(&d) == 46816);            // the reference's default NODE [REF nODE.jl:11-14]
    assert(rec_nseq(d, 64) == 1 && rec_capacity(d, 0, 50, 0) == 200 && rec_capacity(d, 0, 50, 1) == 800 && rec_capacity(d, 7, 50, 0) == 7);
    d.maxiters = 5;
    assert(rec_capacity(d, 0, 50, 0) == 5);
    d.maxiters = 100000; d.solver = LDE_SOLVER_RK4;
    assert(validate(&d, &why) == LDE_ERR_UNSUPPORTED);                           // adaptive RK4: declared out of scope
    d.adaptive = 0; d.dt = 0.05;
    assert(validate(&d, &why) == LDE_OK);
    std::vector<double> ts(50);
    for (int j = 0; j < 50; j++) ts[j] = 0.05 * j;
    assert(grid_ok(ts.data(), 50) && fixed_step_count(d, ts.data(), 50) == 49);
    d.dt = 1e-30;
    assert(fixed_step_count(d, ts.data(), 50) == d.maxiters);                    // capped, no overflow
    KOpts o = make_opts(d, ts.data(), 50, 64);
    assert(o.T == 50 && o.B == 64 && o.t_first == 0.0 && o.t_last == ts[49] && o.checkpoint == 1 && o.dtmin > 0);
    // the record layout: consecutive, aligned, inside rec_bytes
    d = good();
    for (int B : {1, 3, 64, 257}) for (int cap : {1, 7, 64, 200}) {
      const size_t bytes = rec_bytes(d, B, cap, true);
      std::vector<unsigned char> buf(bytes + 256);
      unsigned char* base = (unsigned char*)(((uintptr_t)buf.data() + 255) & ~(uintptr_t)255);
      StepRec r = rec_view(d, base, B, cap, true);
      assert((unsigned char*)r.n == base && ((uintptr_t)r.t & 255) == 0 && ((uintptr_t)r.dt & 255) == 0 && ((uintptr_t)r.y & 255) == 0);
      assert((unsigned char*)(r.y + (size_t)cap * B * 2) <= base + bytes && r.cap == cap && r.nseq == B);
      // touch the last element of every array: an overrun is an ASan report
      r.n[B - 1] = 1; r.t[(size_t)cap * B - 1] = 1.0; r.dt[(size_t)cap * B - 1] = 1.0; r.y[(size_t)cap * B * 2 - 1] = 1.f;
    }
  }
  // 2. hostile descriptions: never a crash, never an out-of-bounds index, always a status
  for (int it = 0; it < 200000; it++) {
    lde_problem_desc d = good();
    const int nmut = 1 + (int)(rnd() % 5);
    for (int m = 0; m < nmut; m++) {
      switch (rnd() % 22) {
        case 0: d.abi_version = hostile_int(); break;
        case 1: d.rhs_kind = hostile_int(); break;
        case 2: d.state_dim = hostile_int(); break;
        case 3: d.param_dim = hostile_int(); break;
        case 4: d.augment_dim = hostile_int(); break;
        case 5: d.n_layers = hostile_int(); break;
        case 6: d.layer_sizes[rnd() % (LDE_MAX_LAYERS + 1)] = hostile_int(); break;
        case 7: d.activation = hostile_int(); break;
        case 8: d.solver = hostile_int(); break;
        case 9: d.batching = hostile_int(); break;
        case 10: d.sensealg = hostile_int(); break;
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
    {   // the dense chains' choices with hostile numbers: no division by zero, no signed overflow, never an empty grid for N ≥ 1
      const int64_t N = (rnd() & 1) ? (int64_t)hostile_int() : (rnd() & 1) ? std::numeric_limits<int64_t>::max() - (int64_t)(rnd() % 64) : (int64_t)(rnd() % 100000);
      const int cg = hostile_int(), jobs = hostile_int();
      const int g = chain_narrow(N, cg);
      assert(g >= 1 && (cg < 1 || g <= cg) && (N < 1) == (chain_tiles(N, cg) == 0) && chain_tiles(N, g) >= chain_tiles(N, cg));
      const ChainChoice ch = chain_call_choice(hostile_int(), cg, N, rnd() & 1);
      assert(ch.layout == CHAIN_NONE ? ch.cg == 0 : ch.cg >= 1);
      if (ch.layout != CHAIN_NONE && N >= 1) assert(chain_tiles(N, ch.cg) >= 1);
      const ChainDwSplit sp = chain_dw_split(jobs, cg, N);
      assert(sp.nvt >= 1 && sp.nvt <= 256 && sp.cap >= 1 && (N >= 1 ? sp.total >= 1 : sp.total == 0));
      if (sp.total < (int64_t)1 << 40) assert((int64_t)sp.nvt * sp.cap >= sp.total && sp.nvt <= std::max<int64_t>(sp.total, 1));   // every slot in a virtual tile
      const int parts = chain_dw_parts_bf16(jobs, N, (rnd() & 1) ? 64 : hostile_int());
      assert(parts >= 1 && parts <= 256);
      lde::ChainLdsDims q;
      q.ld0 = hostile_int(); q.ldh = hostile_int(); q.nbias = hostile_int(); q.ldb = hostile_int(); q.ldg = hostile_int(); q.fpanel = (int)(rnd() & 1); q.xs_per_cg = (size_t)rnd();
      const int t = chain_tile_pick(q, rnd() & 1, rnd() & 1, (rnd() & 1) ? (size_t)160 * 1024 : (size_t)rnd());
      assert(t == 0 || t == 1 || t == 2 || t == 4);
    }
    const int rc = validate(&d, &why);
    (void)num_weights(&d);                                       // (defined for ANY description: n_layers is clamped to the struct's capacity)
    if (rc == LDE_OK) {
      n_ok++;
      const int T = 1 + (int)(rnd() % 300), B = 1 + (int)(rnd() % 5000);
      std::vector<double> ts(T);
      double t = hostile_double();
      if (!std::isfinite(t) || std::fabs(t) > 1e6) t = 0;   // (a grid that stays strictly increasing in f64)
      for (int j = 0; j < T; j++) { ts[j] = t; t += 1e-3 + (double)(rnd() % 1000) * 1e-4; }
      assert(grid_ok(ts.data(), T));
      KOpts o = make_opts(d, ts.data(), T, B);
      assert(o.T == T && o.B == B);
      (void)fixed_step_count(d, ts.data(), T);
      const int cap = rec_capacity(d, (int)(rnd() % 3) ? 0 : 1 + (int)(rnd() % 4096), T, (int)(rnd() & 1));
      assert(cap >= 1);
      assert(rec_bytes(d, B, cap, true) >= (size_t)rec_nseq(d, B) * 4);
    } else {
      n_bad++;
      assert(rc == LDE_ERR_INVALID_ARG || rc == LDE_ERR_UNSUPPORTED);
    }
  }
  assert(validate(nullptr, &why) == LDE_ERR_INVALID_ARG && num_weights(nullptr) == 0);
  // 3. save-time grids
  {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const double a[3] = {0, 1, 1}, b[3] = {0, nan, 2}, c[2] = {0, inf}, e[1] = {5};
    assert(!grid_ok(a, 3) && !grid_ok(b, 3) && !grid_ok(c, 2) && grid_ok(e, 1));
  }
  // 4. which forward mapping serves a solve of the analytic right-hand sides (csrc/lde_pendulum.hip's launch code switches on this)
  {
    const lde::PendTune def;   // the measured thresholds
    const int P = LDE_RHS_PENDULUM, F = LDE_RHS_PENDULUM_FRICTION, TS = LDE_SOLVER_TSIT5, RK = LDE_SOLVER_RK4, LMAX = 6000;
    auto m = [&](int kind, int solver, bool ad, bool rec, int B, int T, const lde::PendTune& tn) { return pend_forward_mapping(kind, solver, ad, rec, B, T, tn, LMAX); };
    // the metric's shape (frictionless, Tsit5, adaptive): lane pairs up to 1 024, four dense-output waves up to 512 — recording or not
    for (int rec = 0; rec < 2; rec++) {
      assert(m(P, TS, true, rec, 1, 50, def) == PEND_FWD_LP4 && m(P, TS, true, rec, 256, 50, def) == PEND_FWD_LP4 && m(P, TS, true, rec, 512, 50, def) == PEND_FWD_LP4);
      assert(m(P, TS, true, rec, 513, 50, def) == PEND_FWD_LP3 && m(P, TS, true, rec, 1024, 50, def) == PEND_FWD_LP3);
    }
    assert(m(P, TS, true, false, 1025, 50, def) == PEND_FWD_TL && m(P, TS, true, false, 2048, 50, def) == PEND_FWD_TL && m(P, TS, true, false, 2049, 50, def) == PEND_FWD_WS);
    assert(m(P, TS, true, true, 1025, 50, def) == PEND_FWD_WS && m(P, TS, true, true, 16384, 50, def) == PEND_FWD_WS);
    // every other solve of a trajectory per workgroup: B ≤ 768 when it writes step records, ≤ 256 when it does not
    assert(m(F, TS, true, true, 768, 50, def) == PEND_FWD_SH && m(F, TS, true, true, 769, 50, def) == PEND_FWD_WS);
    assert(m(F, TS, true, false, 256, 50, def) == PEND_FWD_SH && m(F, TS, true, false, 257, 50, def) == PEND_FWD_TL);
    assert(m(P, RK, false, false, 256, 50, def) == PEND_FWD_SH && m(P, TS, false, true, 700, 50, def) == PEND_FWD_SH);
    // beyond: a lane per trajectory, through the row ring from 2^17 on (save grids that fit beside it)
    assert(m(P, TS, true, false, 16385, 50, def) == PEND_FWD_LANE && m(P, TS, true, true, (1 << 17) - 1, 50, def) == PEND_FWD_LANE);
    assert(m(P, TS, true, false, 1 << 17, 50, def) == PEND_FWD_RING && m(P, TS, true, true, 1 << 20, 50, def) == PEND_FWD_RING && m(P, TS, true, false, 1 << 20, 2049, def) == PEND_FWD_LANE);
    // degenerate grids: T = 1 solves nothing (a lane per trajectory writes ẑ₀); T = 2 has no interior for k_pend_forward_ws
    assert(m(P, TS, true, false, 256, 1, def) == PEND_FWD_LANE && m(P, TS, true, true, 5000, 2, def) == PEND_FWD_LANE && m(P, TS, true, true, 5000, 6001, def) == PEND_FWD_LANE);
    // the options the tests force a mapping with: "pend_sh_max_b" ≥ 0 is ONE threshold for lp and sh; "pend_lp" = 0 sends the metric's shape to sh
    lde::PendTune t = def;
    t.sh_max_b = 0;
    assert(m(P, TS, true, false, 1, 50, t) == PEND_FWD_TL && m(P, TS, true, true, 1, 50, t) == PEND_FWD_WS);
    t.sh_max_b = 1 << 20;
    assert(m(P, TS, true, true, 5000, 50, t) == PEND_FWD_LP3 && m(F, TS, true, false, 5000, 50, t) == PEND_FWD_SH);
    t.lp = 0;
    assert(m(P, TS, true, true, 100, 50, t) == PEND_FWD_SH);
    t = def; t.ws = 0; t.tl_max_b = 0; t.sh_max_b = 0; t.lb_min_b = 0;
    assert(m(P, TS, true, false, 1000, 50, t) == PEND_FWD_RING);
    t.lb_ring = 0;
    assert(m(P, TS, true, false, 1000, 50, t) == PEND_FWD_LANE);
    // … and for ANY arguments one of the seven
    for (int it = 0; it < 20000; it++) {
      lde::PendTune h;
      h.ws = (int)(rnd() % 3); h.tl_max_b = (int)(rnd() % 5000); h.sh_max_b = (int)(rnd() % 3000) - 1; h.lp = (int)(rnd() & 1);
      h.lb_ring = (int)(rnd() % 40); h.lb_min_b = (int)(rnd() % 300000);
      const PendFwdMap r = m((int)(rnd() % 2), (int)(rnd() % 2), rnd() & 1, rnd() & 1, 1 + (int)(rnd() % (1 << 21)), 1 + (int)(rnd() % 7000), h);
      assert(r >= PEND_FWD_LP4 && r <= PEND_FWD_LANE);
    }
    // the lanes-as-save-times form: one save time per lane up to 64 save intervals
    assert(pend_tl_one_save_per_lane(2) && pend_tl_one_save_per_lane(65) && !pend_tl_one_save_per_lane(66));
  }
  // 5. the large-batch forward's row ring: 16 rows when recording, else 32 / 16 / 8 from "pend_lb"; the hold clamped to [0, rows − 1]
  {
    lde::PendTune t;
    auto ring = [&](bool rec, int lb, int hold) { t.lb_ring = lb; t.lb_hold = hold; return pend_ring_shape(rec, t); };
    assert(ring(false, 16, -1).rows == 16 && ring(false, 16, -1).hold == 8);                            // the defaults: 16 rows, half held
    assert(ring(true, 8, -1).rows == 16 && ring(true, 32, -1).rows == 16 && ring(true, 32, 3).hold == 3);
    assert(ring(false, 32, -1).rows == 32 && ring(false, 33, -1).rows == 32 && ring(false, 32, -1).hold == 16);
    assert(ring(false, 31, -1).rows == 16 && ring(false, 15, -1).rows == 8 && ring(false, 1, -1).rows == 8 && ring(false, 8, -1).hold == 4);
    // tests/test_gpu_pendulum.py's "lb8": 8 rows, a requested hold of 8 — clamped to 7, or no lane would ever move
    assert(ring(false, 8, 8).rows == 8 && ring(false, 8, 8).hold == 7);
    assert(ring(false, 8, 7).hold == 7 && ring(false, 8, 0).hold == 0 && ring(false, 32, 1 << 30).hold == 31 && ring(true, 8, 16).hold == 15);
    for (int it = 0; it < 20000; it++) {
      const PendRing r = ring(rnd() & 1, hostile_int(), hostile_int());
      assert((r.rows == 8 || r.rows == 16 || r.rows == 32) && r.hold >= 0 && r.hold < r.rows);
    }
  }
  // 6. which pullback serves an lde_adjoint of the analytic right-hand sides (csrc/lde_pendulum.hip's launch code switches on this)
  {
    const lde::PendTune def;
    const int DI = LDE_SENSE_DISCRETE, PA = LDE_SENSE_PARALLEL_CHECKPOINTED;
    // the time-parallel continuous pullback: fused for B ≤ 24 576 and 1 ≤ T − 1 ≤ 1024, streamed per trajectory otherwise
    assert(pend_adjoint_mapping(PA, 256, 50, def) == PEND_ADJ_FUSED && pend_adjoint_mapping(PA, 24576, 50, def) == PEND_ADJ_FUSED);
    assert(pend_adjoint_mapping(PA, 24577, 50, def) == PEND_ADJ_STREAM && pend_adjoint_mapping(PA, 1 << 20, 50, def) == PEND_ADJ_STREAM);
    assert(pend_adjoint_mapping(PA, 1, 2, def) == PEND_ADJ_FUSED && pend_adjoint_mapping(PA, 64, 1025, def) == PEND_ADJ_FUSED);
    assert(pend_adjoint_mapping(PA, 64, 1026, def) == PEND_ADJ_STREAM && pend_adjoint_mapping(PA, 1, 1, def) == PEND_ADJ_STREAM);
    // the discrete pullback: a wave per trajectory for 1 < T ≤ 3840 and B ≤ "pend_disc_tp_max_b" (16 384), a lane per trajectory otherwise
    assert(pend_adjoint_mapping(DI, 256, 50, def) == PEND_ADJ_DISC_TP && pend_adjoint_mapping(DI, 16384, 50, def) == PEND_ADJ_DISC_TP);
    assert(pend_adjoint_mapping(DI, 16385, 50, def) == PEND_ADJ_DISC && pend_adjoint_mapping(DI, 1, 2, def) == PEND_ADJ_DISC_TP);
    assert(pend_adjoint_mapping(DI, 1, 1, def) == PEND_ADJ_DISC && pend_adjoint_mapping(DI, 64, 3840, def) == PEND_ADJ_DISC_TP);
    assert(pend_adjoint_mapping(DI, 64, 3841, def) == PEND_ADJ_DISC);
    lde::PendTune t = def;
    t.disc_tp_max_b = 0;
    assert(pend_adjoint_mapping(DI, 1, 50, t) == PEND_ADJ_DISC);
    t.disc_tp_max_b = 1 << 30;
    assert(pend_adjoint_mapping(DI, 1 << 20, 50, t) == PEND_ADJ_DISC_TP && pend_adjoint_mapping(PA, 1 << 20, 50, t) == PEND_ADJ_STREAM);
    // the reverse-time solve: a lane per trajectory, whatever the shape
    for (int s : {LDE_SENSE_BACKSOLVE_CHECKPOINTED, LDE_SENSE_BACKSOLVE})
      for (int B : {1, 256, 24577, 1 << 20}) assert(pend_adjoint_mapping(s, B, 50, def) == PEND_ADJ_SEQ && pend_adjoint_mapping(s, B, 5000, def) == PEND_ADJ_SEQ);
    for (int it = 0; it < 20000; it++) {
      lde::PendTune h;
      h.disc_tp_max_b = hostile_int();
      const PendAdjMap r = pend_adjoint_mapping((int)(rnd() % 5), hostile_int(), hostile_int(), h);
      assert(r >= PEND_ADJ_SEQ && r <= PEND_ADJ_DISC);
    }
  }
  // 7. the kernels' template arguments: exactly validate()'s six (rhs_kind, solver, adaptive) combinations reach the kernels
  {
    int seen[2][2][2] = {};
    auto rec = [&](auto K, auto S, auto A) -> int {
      static_assert(decltype(K)::value == 0 || decltype(K)::value == 1, "KIND");
      seen[K][S][A]++;
      return 100 * K + 10 * S + A;
    };
    const int P = LDE_RHS_PENDULUM, F = LDE_RHS_PENDULUM_FRICTION, TS = LDE_SOLVER_TSIT5, RK = LDE_SOLVER_RK4;
    assert(pend_dispatch(P, TS, true, rec) == 1 && pend_dispatch(P, TS, false, rec) == 0 && pend_dispatch(P, RK, false, rec) == 10);
    assert(pend_dispatch(F, TS, true, rec) == 101 && pend_dispatch(F, TS, false, rec) == 100 && pend_dispatch(F, RK, false, rec) == 110);
    assert(pend_dispatch(P, RK, true, rec) == LDE_ERR_UNSUPPORTED && pend_dispatch(F, RK, true, rec) == LDE_ERR_UNSUPPORTED);   // adaptive RK4
    assert(pend_dispatch(LDE_RHS_MLP, TS, true, rec) == LDE_ERR_UNSUPPORTED && pend_dispatch(LDE_RHS_PENDULUM_PLUS_MLP, TS, false, rec) == LDE_ERR_UNSUPPORTED);
    assert(pend_dispatch(P, 2, false, rec) == LDE_ERR_UNSUPPORTED && pend_dispatch(-1, TS, true, rec) == LDE_ERR_UNSUPPORTED);
    for (int k = 0; k < 2; k++)
      for (int s = 0; s < 2; s++)
        for (int a = 0; a < 2; a++) assert(seen[k][s][a] == (s == 1 && a == 1 ? 0 : 1));
    // any arguments: f is called for a combination validate() admits, or not at all
    for (int it = 0; it < 20000; it++) {
      lde_problem_desc d = good();
      d.rhs_kind = (rnd() & 1) ? hostile_int() : (int)(rnd() % 4);
      d.solver = (rnd() & 1) ? hostile_int() : (int)(rnd() % 2);
      d.adaptive = (int)(rnd() % 2);
      d.dt = 0.05;
      int called = 0;
      const int rc = pend_dispatch(d.rhs_kind, d.solver, d.adaptive != 0, [&](auto, auto, auto) -> int { called++; return LDE_OK; });
      assert(called == (rc == LDE_OK) && (rc == LDE_OK || rc == LDE_ERR_UNSUPPORTED));
      assert(!called || (validate(&d, &why) == LDE_OK && has_pend(d) && !has_mlp(d)));
    }
  }
  // 8. which kernel family serves the MLP right-hand sides (csrc/lde_mlp.hip's launch code switches on this). Expected values: the constants
  //    of the predicates this mapping replaced (mlp64_applicable, vec_applicable, w_applicable, b_applicable, c_applicable, disc_family,
  //    mlp4_layout), in their order of precedence.
  {
    const int RK = LDE_SOLVER_RK4, PT = LDE_BATCH_PER_TRAJECTORY, CO = LDE_BATCH_COUPLED, GL = LDE_BATCH_COUPLED_GLOBAL;
    const int CONT = LDE_SENSE_BACKSOLVE_CHECKPOINTED, DISC = LDE_SENSE_DISCRETE;
    auto net = [&](std::vector<int> layers, int batching, int sense, int kind = LDE_RHS_MLP, int solver = LDE_SOLVER_TSIT5) {
      lde_problem_desc d = good();
      d.rhs_kind = kind; d.batching = batching; d.sensealg = sense; d.solver = solver;
      if (solver == LDE_SOLVER_RK4) { d.adaptive = 0; d.dt = 0.05; }
      if (kind == LDE_RHS_MLP) { d.state_dim = layers[0]; d.param_dim = 0; }
      d.n_layers = (int)layers.size() - 1;
      for (size_t i = 0; i < layers.size(); i++) d.layer_sizes[i] = layers[i];
      assert(validate(&d, &why) == LDE_OK);
      return mlp_shape(d);
    };
    const size_t CAP = 160 * 1024;
    auto roomy = [&](int B) {   // LDS that never binds; k_mlp4_adjoint's workgroups as its layout counts them
      lde::MlpLds l;
      l.cap = CAP;
      l.v_fixed = l.w = l.b = l.c = l.b_disc = l.c_disc = l.mlp4 = 4096;
      const int nwaves = (B + 3) / 4, wpb = std::max(1, std::min(4, (nwaves + 255) / 256));
      l.mlp4_blocks = (nwaves + wpb - 1) / wpb;
      return l;
    };
    const lde::MlpTune def;
    auto fwd = [&](const lde::MlpShape& s, const lde::MlpTune& tn, int B, bool ad, bool rec = false) { return mlp_forward_mapping(s, tn, roomy(B), B, ad, rec); };
    auto adj = [&](const lde::MlpShape& s, const lde::MlpTune& tn, int B, bool ad) { return mlp_adjoint_mapping(s, tn, roomy(B), B, ad); };
    // the values option "adjoint_family" reports
    static_assert(MLP_TILES == 0 && MLP_64 == 1 && MLP_B == 2 && MLP_C == 3 && MLP_W == 4 && MLP_V == 5 && MLP_4 == 6 && MLP_NOT_SERVED == 7, "adjoint_family");

    // the shapes' summaries
    const lde::MlpShape c2 = net({8, 200, 200, 8}, CO, CONT, LDE_RHS_MLP, RK), c3 = net({2, 64, 64, 2}, PT, CONT, LDE_RHS_PENDULUM_PLUS_MLP);
    const lde::MlpShape c4 = net({32, 128, 128, 32}, CO, CONT), ref = net({16, 200, 200, 16}, CO, CONT), c4pt = net({32, 128, 128, 32}, PT, CONT);
    assert(c2.b_ok && c2.w_ok && !c2.c_ok && c2.vec_ok && c2.v_nt == 256 && !c2.v_reg && c2.w_waves == 4 && c2.hm == 200 && c2.maxw == 200);
    assert(!c3.b_ok && !c3.w_ok && !c3.c_ok && c3.vec_ok && c3.v_nt == 64 && c3.v_reg && c3.P == 1 && c3.Dp == 2);
    assert(!c4.b_ok && c4.w_ok && c4.c_ok && c4.v_nt == 256 && c4.v_reg && c4.w_waves == 2 && !c4pt.c_ok && c4pt.w_ok);
    assert(ref.b_ok && ref.w_ok && !ref.c_ok && ref.v_nt == 256 && !ref.v_reg);
    assert(net({6, 40, 24, 40, 6}, PT, CONT).v_nt == 64 && !net({6, 40, 24, 40, 6}, PT, CONT).v_reg && !net({6, 40, 24, 40, 6}, PT, CONT).w_ok);
    assert(net({6, 100, 24, 100, 6}, PT, CONT).v_nt == 128 && net({8, 16, 16, 8}, PT, CONT).v_nt == 64 && !net({8, 16, 16, 8}, PT, CONT).v_reg);
    assert(net({8, 17, 16, 8}, PT, CONT).v_reg && net({8, 129, 16, 8}, PT, CONT).v_nt == 256 && !net({8, 129, 16, 8}, PT, CONT).v_reg);
    assert(!net({8, 300, 16, 8}, PT, CONT).vec_ok && !net({8, 201, 16, 8}, PT, CONT).w_ok && net({33, 64, 64, 33}, CO, CONT).vec_ok && !net({33, 64, 64, 33}, CO, CONT).c_ok);
    assert(net({17, 64, 64, 17}, CO, CONT).c_ok && !net({17, 64, 64, 17}, CO, CONT).b_ok && !net({8, 129, 128, 8}, CO, CONT).c_ok && net({8, 128, 128, 8}, CO, CONT).c_ok);

    // the five bench shapes: c2 B = 256, c3 B = 1024, c4 B = 512 and 4096, the reference NODE B = 64 — forward and adjoint
    assert(fwd(c2, def, 256, false) == MLP_B && adj(c2, def, 256, false) == MLP_B);
    assert(fwd(c3, def, 1024, true) == MLP_64 && adj(c3, def, 1024, true) == MLP_64);
    assert(fwd(c4, def, 512, true) == MLP_C && adj(c4, def, 512, true) == MLP_C);
    assert(fwd(c4, def, 4096, true) == MLP_TILES && adj(c4, def, 4096, true) == MLP_TILES);
    assert(fwd(ref, def, 64, true) == MLP_B && adj(ref, def, 64, true) == MLP_B);

    // k_mlp64: B ≤ 65 536, per-trajectory control only, hidden layers ≤ 64, D′ ≤ 4; beyond, c3 falls to the tiles (forward) / k_mlp4_adjoint
    assert(fwd(c3, def, 65536, true) == MLP_64 && fwd(c3, def, 65537, true) == MLP_TILES && adj(c3, def, 65536, true) == MLP_64 && adj(c3, def, 65537, true) == MLP_4);
    assert(fwd(net({4, 64, 64, 4}, PT, CONT), def, 100, true) == MLP_64 && fwd(net({5, 64, 64, 5}, PT, CONT), def, 100, true) != MLP_64);
    assert(fwd(net({4, 65, 64, 4}, PT, CONT), def, 100, true) != MLP_64 && fwd(net({4, 64, 64, 4}, CO, CONT), def, 100, true) != MLP_64);
    assert(fwd(net({4, 64, 64, 64, 4}, PT, CONT), def, 100, true) != MLP_64);
    lde::MlpTune t = def;
    t.mlp64 = 0;
    // k_mlpv: B·NT/64 ≤ 1024, twice that with the register-resident hidden layer (c3: NT = 64 → 2048; c4: 256 → 512; deep: 64, plain → 1024)
    assert(fwd(c3, t, 2048, true) == MLP_V && fwd(c3, t, 2049, true) == MLP_TILES && adj(c3, t, 2048, true) == MLP_V && adj(c3, t, 2049, true) == MLP_4);
    const lde::MlpShape deep = net({6, 40, 24, 40, 6}, PT, CONT), deep128 = net({6, 100, 24, 100, 6}, PT, CONT);
    assert(adj(deep, def, 1024, true) == MLP_V && adj(deep, def, 1025, true) == MLP_4 && fwd(deep, def, 1024, true) == MLP_V && fwd(deep, def, 1025, true) == MLP_TILES);
    assert(adj(deep128, def, 512, true) == MLP_V && adj(deep128, def, 513, true) == MLP_TILES);
    t = def; t.mlpv = 0;
    assert(adj(deep, t, 100, true) == MLP_4 && fwd(deep, t, 100, true) == MLP_TILES);

    // k_mlpb: 512 trajectories, 256 when they must all be resident — the forward: coupled AND adaptive AND B > 1; the continuous adjoint: coupled
    assert(fwd(c2, def, 512, false) == MLP_B && fwd(c2, def, 513, false) == MLP_TILES);                  // (fixed step: the forward may queue)
    assert(adj(c2, def, 257, false) == MLP_W && adj(c2, def, 512, false) == MLP_W && adj(c2, def, 513, false) == MLP_TILES);
    assert(fwd(c2, def, 300, false) == MLP_B && adj(c2, def, 300, false) == MLP_W);                      // the split at B = 300: forward k_mlpb, adjoint k_mlpw
    assert(fwd(ref, def, 256, true) == MLP_B && fwd(ref, def, 257, true) == MLP_TILES && adj(ref, def, 256, true) == MLP_B && adj(ref, def, 257, true) == MLP_TILES);
    const lde::MlpShape c2pt = net({8, 200, 200, 8}, PT, CONT);
    assert(fwd(c2pt, def, 512, true) == MLP_B && adj(c2pt, def, 512, true) == MLP_B && adj(c2pt, def, 513, true) == MLP_TILES);
    // "mlpb": 0 = k_mlpw instead, 1 = networks wider than 128 only, 2 = the narrower ones too
    const lde::MlpShape h70 = net({8, 70, 65, 8}, PT, CONT);
    assert(adj(h70, def, 26, true) == MLP_W && fwd(h70, def, 26, true) == MLP_W);
    t = def; t.mlpb = 2;
    assert(adj(h70, t, 26, true) == MLP_B && adj(h70, t, 512, true) == MLP_B && adj(h70, t, 513, true) == MLP_W);
    t.mlpb = 0;
    assert(adj(h70, t, 26, true) == MLP_W && adj(c2, t, 256, false) == MLP_W && fwd(c2, t, 256, false) == MLP_W && adj(c4, t, 512, true) == MLP_W);
    // "mlpw" = 0 switches k_mlpw, k_mlpb AND k_mlpc off
    t = def; t.mlpw = 0;
    assert(adj(c2, t, 256, false) == MLP_V && fwd(c2, t, 256, false) == MLP_V && adj(c2, t, 257, false) == MLP_TILES && adj(c4, t, 512, true) == MLP_V && adj(ref, t, 64, true) == MLP_V);
    assert(adj(c4, t, 513, true) == MLP_TILES && fwd(c4, t, 512, true) == MLP_V && fwd(c4, t, 513, true) == MLP_TILES);   // (register-resident layer at NT = 256: 2048·64/256)
    t.mlpv = 0; t.mlp64 = 0;   // the tests' "tiles" leg
    assert(adj(c2, t, 48, false) == MLP_TILES && adj(c3, t, 80, true) == MLP_4 && adj(c4, t, 40, true) == MLP_TILES && fwd(c3, t, 80, true) == MLP_TILES);

    // k_mlpc: 1024 trajectories, 512 resident (the same two readings of "coupled")
    assert(fwd(c4, def, 513, true) == MLP_TILES && adj(c4, def, 513, true) == MLP_TILES && fwd(c4, def, 1, true) == MLP_C);
    assert(fwd(c4, def, 1024, false) == MLP_C && fwd(c4, def, 1025, false) == MLP_TILES);                // (coupled, fixed step)
    assert(adj(c4, def, 512, false) == MLP_C && adj(c4, def, 513, false) == MLP_W && adj(c4, def, 1024, false) == MLP_W && adj(c4, def, 1025, false) == MLP_TILES);
    // k_mlpw: 2048 waves, 1024 resident (W = 2 up to 128 units, 4 beyond)
    assert(adj(c4pt, def, 1024, true) == MLP_W && adj(c4pt, def, 1025, true) == MLP_TILES && fwd(c4pt, def, 1024, true) == MLP_W);
    t = def; t.mlpb = 0;
    assert(fwd(c4, t, 512, true) == MLP_W && fwd(c4, t, 513, true) == MLP_TILES && fwd(ref, t, 256, true) == MLP_W && fwd(ref, t, 257, true) == MLP_TILES);
    assert(fwd(c2, t, 512, false) == MLP_W && fwd(c2, t, 513, false) == MLP_TILES);

    // a forward that writes a step record: never k_mlpw / k_mlpv; k_mlp64, k_mlpb, k_mlpc and the tiles write it
    assert(fwd(c4pt, def, 512, true, true) == MLP_TILES && fwd(deep, def, 100, true, true) == MLP_TILES && fwd(h70, def, 26, true, true) == MLP_TILES);
    assert(fwd(c3, def, 1024, true, true) == MLP_64 && fwd(c2, def, 256, false, true) == MLP_B && fwd(c4, def, 512, true, true) == MLP_C);

    // k_mlp4_adjoint: layers up to "mlp4_maxw" (64) and 256 wide, D′ ≤ 64, P ≤ 1; coupled adaptive: at most 256 workgroups
    const lde::MlpShape n48 = net({4, 48, 33, 4}, PT, CONT);
    t = def; t.mlp64 = 0; t.mlpv = 0; t.mlpw = 0;
    assert(adj(n48, t, 37, true) == MLP_4);
    t.mlp4_maxw = 47;
    assert(adj(n48, t, 37, true) == MLP_TILES);
    t.mlp4_maxw = 48;
    assert(adj(n48, t, 37, true) == MLP_4);
    t.mlp4 = 0;
    assert(adj(n48, t, 37, true) == MLP_TILES);
    t.mlp4 = 1; t.mlp4_maxw = 1 << 20;
    assert(adj(c2, t, 48, false) == MLP_4 && adj(net({8, 257, 16, 8}, PT, CONT), t, 48, true) == MLP_TILES && adj(net({65, 70, 16, 65}, PT, CONT), t, 48, true) == MLP_TILES);
    {
      lde::MlpShape p2 = n48;
      p2.P = 2;
      assert(adj(p2, t, 37, true) == MLP_TILES);
      lde::MlpLds l = roomy(64);
      const lde::MlpShape co48 = net({4, 48, 33, 4}, CO, CONT);
      l.mlp4_blocks = 256;
      assert(mlp_adjoint_mapping(co48, t, l, 64, true) == MLP_4);
      l.mlp4_blocks = 257;
      assert(mlp_adjoint_mapping(co48, t, l, 64, true) == MLP_TILES && mlp_adjoint_mapping(co48, t, l, 64, false) == MLP_4 && mlp_adjoint_mapping(n48, t, l, 64, true) == MLP_4);
      l.mlp4 = CAP + 1;
      assert(mlp_adjoint_mapping(n48, t, l, 64, true) == MLP_TILES);
    }

    // LDE_SENSE_DISCRETE: k_mlp64 first, then k_mlpb up to 1024 and k_mlpc up to 2048 trajectories (coupled or not, adaptive or not), else the tiles
    const lde::MlpShape c2d = net({8, 200, 200, 8}, CO, DISC, LDE_RHS_MLP, RK), c3d = net({2, 64, 64, 2}, PT, DISC, LDE_RHS_PENDULUM_PLUS_MLP), c4d = net({32, 128, 128, 32}, CO, DISC);
    assert(c2d.disc && adj(c3d, def, 1024, true) == MLP_64 && adj(c3d, def, 65537, true) == MLP_TILES);
    assert(adj(c2d, def, 256, false) == MLP_B && adj(c2d, def, 1024, false) == MLP_B && adj(c2d, def, 1025, false) == MLP_TILES);
    assert(adj(c4d, def, 512, true) == MLP_C && adj(c4d, def, 2048, true) == MLP_C && adj(c4d, def, 2049, true) == MLP_TILES && adj(c4d, def, 5000, true) == MLP_TILES);
    assert(adj(net({8, 200, 200, 8}, PT, DISC), def, 1024, true) == MLP_B && adj(net({16, 200, 200, 16}, CO, DISC), def, 64, true) == MLP_B);
    t = def; t.mlpb = 0;
    assert(adj(c2d, t, 256, false) == MLP_TILES && adj(c4d, t, 512, true) == MLP_TILES);
    t = def; t.mlpw = 0;
    assert(adj(c2d, t, 256, false) == MLP_TILES && adj(c4d, t, 512, true) == MLP_TILES);

    // the two refusals, and which comes first
    const char* msg = nullptr;
    assert(fwd(c4, def, 4096, true) == MLP_TILES && mlp_forward_mapping(c4, def, roomy(4097), 4097, true, false, &msg) == MLP_NOT_SERVED && std::strstr(msg, "4096 trajectories"));
    msg = nullptr;
    assert(mlp_adjoint_mapping(c4, def, roomy(4097), 4097, true, &msg) == MLP_NOT_SERVED && std::strstr(msg, "4096 trajectories") && adj(c4, def, 4097, false) == MLP_TILES);
    const lde::MlpShape c4g = net({32, 128, 128, 32}, GL, CONT), c4gd = net({32, 128, 128, 32}, GL, DISC);
    assert(c4g.global && c4g.coupled && fwd(c4g, def, 512, true) == MLP_C && adj(c4g, def, 512, true) == MLP_C);
    msg = nullptr;
    assert(mlp_forward_mapping(c4g, def, roomy(513), 513, true, false, &msg) == MLP_NOT_SERVED && std::strstr(msg, "LDE_BATCH_COUPLED_GLOBAL"));
    msg = nullptr;
    assert(mlp_adjoint_mapping(c4g, def, roomy(513), 513, true, &msg) == MLP_NOT_SERVED && std::strstr(msg, "LDE_BATCH_COUPLED_GLOBAL"));
    assert(mlp_forward_mapping(c4g, def, roomy(5000), 5000, true, false, &msg) == MLP_NOT_SERVED && std::strstr(msg, "LDE_BATCH_COUPLED_GLOBAL"));
    assert(mlp_adjoint_mapping(c4g, def, roomy(5000), 5000, true, &msg) == MLP_NOT_SERVED && std::strstr(msg, "4096 trajectories"));
    assert(adj(c4gd, def, 2049, true) == MLP_TILES);   // the discrete sweep exchanges nothing: nothing to refuse

    // the LDS comparisons: k_mlpw shares a CU's LDS between 4 / W workgroups, k_mlpv takes at most half of it and — resident — its CU's share
    {
      lde::MlpLds l = roomy(512);
      l.c = CAP + 1;
      assert(mlp_forward_mapping(c4, def, l, 512, true, false) == MLP_W);
      l.w = CAP * 2 / 4;
      assert(mlp_forward_mapping(c4, def, l, 512, true, false) == MLP_W);
      l.w += 1;
      assert(mlp_forward_mapping(c4, def, l, 512, true, false) == MLP_V);
      l.v_fixed = CAP / 2 - 256;   // two workgroups per CU: half the LDS less 256 bytes each
      assert(mlpv_lds_budget(CAP, 512) == CAP / 2 - 256 && mlpv_lds_budget(CAP, 256) == CAP && mlp_forward_mapping(c4, def, l, 512, true, false) == MLP_V);
      l.v_fixed += 1;
      assert(mlp_forward_mapping(c4, def, l, 512, true, false) == MLP_TILES && mlp_forward_mapping(c4, def, l, 512, false, false) == MLP_V);
      l.v_fixed = CAP / 2 + 1;
      assert(mlp_forward_mapping(c4, def, l, 512, false, false) == MLP_TILES);
      l = roomy(256);
      l.b = CAP + 1;
      assert(mlp_adjoint_mapping(c2, def, l, 256, false) == MLP_W && mlp_adjoint_mapping(c2d, def, l, 256, false) == MLP_TILES);
      l = roomy(256);
      l.b_disc = CAP + 1;
      assert(mlp_adjoint_mapping(c2d, def, l, 256, false) == MLP_TILES && mlp_adjoint_mapping(c2, def, l, 256, false) == MLP_B);
      l = roomy(512);
      l.c_disc = CAP + 1;
      assert(mlp_adjoint_mapping(c4d, def, l, 512, true) == MLP_TILES && mlp_adjoint_mapping(c4, def, l, 512, true) == MLP_C);
    }

    // the adjoint's workspace: rows of the weight gradient for k_mlp64 (a row per workgroup of four waves, at most 256), k_mlpb (a row per
    // trajectory) and k_mlpc (a row per pair; sized per trajectory), the staging area (0 rows) for everything else
    assert(mlp64_adj_waves(1) == 1 && mlp64_adj_waves(4) == 1 && mlp64_adj_waves(5) == 2 && mlp64_adj_waves(1024) == 256 && mlp64_adj_waves(1 << 20) == 256);
    auto reserve = [&](const lde::MlpShape& s, int B) { return mlp_reserved_rows(adj(s, def, B, false), B); };   // as lde_reserve asks
    assert(reserve(c3, 1024) == 256 && mlp_adjoint_rows(MLP_64, 100) == 25 && reserve(c3d, 100) == 25);
    assert(reserve(c2, 256) == 256 && mlp_adjoint_rows(MLP_B, 256) == 256 && reserve(c2, 300) == 0);
    assert(reserve(c4, 511) == 511 && mlp_adjoint_rows(MLP_C, 511) == 256 && reserve(c4d, 2048) == 2048);
    assert(mlp_reserved_rows(MLP_TILES, 64) == 0 && mlp_reserved_rows(MLP_W, 64) == 0 && mlp_reserved_rows(MLP_V, 64) == 0 && mlp_reserved_rows(MLP_4, 64) == 0 && mlp_reserved_rows(MLP_NOT_SERVED, 64) == 0);
    assert(mlp_adjoint_rows(MLP_TILES, 64) == 0 && mlp_adjoint_rows(MLP_W, 64) == 0 && mlp_adjoint_rows(MLP_V, 64) == 0 && mlp_adjoint_rows(MLP_4, 64) == 0);

    // ANY shape, knobs, LDS numbers and batch: one of the enum's values (the forward never k_mlp4_adjoint), and lde_reserve — which does not
    // know whether the call will be adaptive — sizes at least the rows the adjoint's family writes
    for (int it = 0; it < 100000; it++) {
      lde::MlpShape s;
      lde::MlpTune h;
      lde::MlpLds l;
      s.nL = (rnd() & 1) ? 3 : hostile_int(); s.Dp = hostile_int(); s.P = hostile_int(); s.hm = hostile_int(); s.maxw = hostile_int();
      s.coupled = rnd() & 1; s.global = rnd() & 1; s.disc = rnd() & 1; s.vec_ok = rnd() & 1; s.w_ok = rnd() & 1; s.b_ok = rnd() & 1; s.c_ok = rnd() & 1;
      s.v_nt = (rnd() & 1) ? 64 << (rnd() % 3) : hostile_int(); s.v_reg = rnd() & 1; s.w_waves = (rnd() & 1) ? 2 + 2 * (int)(rnd() & 1) : hostile_int();
      h.mlp64 = (int)(rnd() % 2); h.mlpv = (int)(rnd() % 2); h.mlpw = (int)(rnd() % 2); h.mlp4 = (int)(rnd() % 2); h.mlpb = (int)(rnd() % 3); h.mlp4_maxw = hostile_int();
      auto bytes = [&]() { return (rnd() & 1) ? (size_t)(rnd() % (2 * CAP)) : (size_t)rnd(); };
      l.cap = (rnd() & 3) ? CAP : bytes();
      l.v_fixed = bytes(); l.w = bytes(); l.b = bytes(); l.c = bytes(); l.b_disc = bytes(); l.c_disc = bytes(); l.mlp4 = bytes(); l.mlp4_blocks = hostile_int();
      const int B = (rnd() & 1) ? 1 + (int)(rnd() % 5000) : hostile_int();
      const MlpFamily f = mlp_forward_mapping(s, h, l, B, rnd() & 1, rnd() & 1);
      assert(f >= MLP_TILES && f <= MLP_NOT_SERVED && f != MLP_4);
      for (int ad = 0; ad < 2; ad++) {
        const MlpFamily a = mlp_adjoint_mapping(s, h, l, B, ad != 0);
        assert(a >= MLP_TILES && a <= MLP_NOT_SERVED);
        const int rows = mlp_adjoint_rows(a, B);   // the call's family writes them; lde_reserve asked with adaptive = false
        if (rows > 0) assert(mlp_reserved_rows(mlp_adjoint_mapping(s, h, l, B, false), B) >= rows);
      }
    }
  }
  // 9. the MLP kernels' template argument: the two solvers validate() admits reach the kernels, nothing else
  {
    int seen[2] = {0, 0};
    auto rec = [&](auto S) -> int { seen[decltype(S)::value]++; return 10 + decltype(S)::value; };
    static_assert(LDE_SOLVER_TSIT5 == 0 && LDE_SOLVER_RK4 == 1, "solver codes");
    assert(mlp_dispatch(LDE_SOLVER_TSIT5, rec) == 10 && mlp_dispatch(LDE_SOLVER_RK4, rec) == 11 && seen[0] == 1 && seen[1] == 1);
    assert(mlp_dispatch(2, rec) == LDE_ERR_UNSUPPORTED && mlp_dispatch(-1, rec) == LDE_ERR_UNSUPPORTED && seen[0] == 1 && seen[1] == 1);
    for (int it = 0; it < 20000; it++) {
      const int solver = hostile_int();
      int called = 0;
      const int rc = mlp_dispatch(solver, [&](auto) -> int { called++; return LDE_OK; });
      assert(called == (solver == LDE_SOLVER_TSIT5 || solver == LDE_SOLVER_RK4) && rc == (called ? LDE_OK : LDE_ERR_UNSUPPORTED));
    }
  }
  // 10. the dense chains (csrc/lde_chain.hip's launch code asks these): LDS bytes, tile widths, the layout of a call, the weight-gradient split
  {
    const size_t CAP = 160 * 1024;
    // the reconstructor 2-200-200-200-784: input panel stride 40, hidden panels 232, 3·200 + 784 biases
    lde::ChainLdsDims rec;
    rec.ld0 = 40; rec.ldh = 232; rec.nbias = 1384;
    assert(chain_lds_bytes(rec, false, false, 4) == 134560 && chain_lds_bytes(rec, false, false, 2) == 70048 && chain_lds_bytes(rec, false, false, 1) == 37792);
    assert(chain_lds_bytes(rec, false, true, 2) == 99744 && chain_lds_bytes(rec, false, true, 1) == 52640);
    assert(chain_tile_pick(rec, false, false, CAP) == 2 && chain_tile_pick(rec, false, true, CAP) == 1);   // two workgroups per CU: the instances the profiles show
    // its bf16 form: panels of stride 272 elements (skip layers: a third forward panel), the f32 gradient panel 232 floats
    rec.ldb = 272; rec.ldg = 232; rec.fpanel = 1;
    assert(chain_lds_bytes(rec, true, false, 2) == 3 * 32 * 272 * 2 + 1384 * 4 && chain_lds_bytes(rec, true, true, 2) == 32 * 272 * 4 + 32 * 232 * 4);
    assert(chain_tile_pick(rec, true, false, CAP) == 2 && chain_tile_pick(rec, true, true, CAP) == 2);
    rec.xs_per_cg = 9216;   // a wide input read in place: the chunk buffers grow with the column groups
    assert(chain_lds_bytes(rec, true, false, 2) == 3 * 32 * 272 * 2 + 1384 * 4 + 2 * 9216 && chain_lds_bytes(rec, true, true, 2) == 32 * 272 * 4 + 32 * 232 * 4);
    // half the LDS first, then all of it, then nothing: 512-wide hidden panels (stride 520) with a 32-wide input (stride 40)
    lde::ChainLdsDims wide;
    wide.ld0 = 40; wide.ldh = 520; wide.nbias = 1064;
    assert(chain_lds_bytes(wide, false, false, 1) == 73376 && chain_lds_bytes(wide, false, false, 2) == 142496 && chain_lds_bytes(wide, false, true, 1) == 106656);
    assert(chain_tile_pick(wide, false, false, CAP) == 1 && chain_tile_pick(wide, false, true, CAP) == 1);   // 16 columns fit half; the pullback only the whole
    assert(chain_tile_pick(wide, false, false, 2 * 73376 - 1) == 2 && chain_tile_pick(wide, false, true, 106655) == 0);
    wide.nbias = 5; wide.ld0 = 0;
    assert(chain_lds_bytes(wide, false, false, 1) == (2 * 16 * 520 + 8) * 4);                                // biases rounded up to 4 floats
    // the narrowing rule: halve the tile until the grid has 192 workgroups
    assert(chain_narrow(3200, 4) == 1 && chain_narrow(12800, 2) == 2 && chain_narrow(12288, 4) == 4 && chain_narrow(12224, 4) == 2);
    assert(chain_narrow(6144, 2) == 2 && chain_narrow(6112, 2) == 1 && chain_narrow(1, 4) == 1 && chain_narrow(3072, 1) == 1 && chain_narrow(1 << 20, 4) == 4);
    assert(chain_tiles(1, 4) == 1 && chain_tiles(64, 4) == 1 && chain_tiles(65, 4) == 2 && chain_tiles(37, 1) == 3 && chain_tiles(0, 1) == 0);
    // the layout of a call: x in place when the chain has that layout, N fills a tile of it and x is 16-byte aligned; else the input panel; else none
    auto is = [](ChainChoice c, ChainLayout l, int cg) { return c.layout == l && c.cg == cg; };
    assert(is(chain_call_choice(2, 2, 12800, true), CHAIN_GX, 2) && is(chain_call_choice(2, 1, 12800, false), CHAIN_PANEL, 1));
    assert(is(chain_call_choice(4, 2, 64, true), CHAIN_GX, 1) && is(chain_call_choice(4, 2, 63, true), CHAIN_PANEL, 1) && is(chain_call_choice(0, 4, 12288, true), CHAIN_PANEL, 4));
    assert(is(chain_call_choice(2, 0, 31, true), CHAIN_NONE, 0) && is(chain_call_choice(2, 0, 32, false), CHAIN_NONE, 0) && is(chain_call_choice(2, 0, 32, true), CHAIN_GX, 1));
    assert(is(chain_call_choice(0, 0, 1000, true), CHAIN_NONE, 0) && is(chain_call_choice(2, 2, 6144, true), CHAIN_GX, 2) && is(chain_call_choice(2, 2, 6112, true), CHAIN_GX, 1));
    // the weight-gradient split: (virtual tiles × jobs) ≈ 256 workgroups, never more virtual tiles than slots
    auto split = [](int jobs, int cg, int64_t N, int nvt, int cap, int64_t total) { const ChainDwSplit s = chain_dw_split(jobs, cg, N); return s.nvt == nvt && s.cap == cap && s.total == total; };
    assert(split(8, 2, 12800, 32, 25, 800) && split(300, 1, 37, 1, 3, 3) && split(4, 1, 16, 1, 1, 1) && split(8, 2, 37, 4, 1, 4) && split(8, 1, 3200, 32, 7, 200));
    assert(split(8, 2, 300000, 32, 586, 18750) && split(1, 1, 1 << 20, 256, 256, 65536));
    assert(chain_dw_parts_bf16(8, 12800, 64) == 32 && chain_dw_parts_bf16(8, 100, 64) == 2 && chain_dw_parts_bf16(300, 12800, 64) == 1);
    assert(chain_dw_parts_bf16(8, 64, 64) == 1 && chain_dw_parts_bf16(8, 65, 64) == 2 && chain_dw_parts_bf16(1, 1 << 20, 64) == 256);
  }
  // 11. the recurrent stacks (csrc/lde_rnn.hip's launch code asks these): weight counts, the LDS / flat-weight layout, the kernel form and
  //     launch shape of a call, groupability, the k-split of the weight gradient. Pins: the formulas lde_rnn_create / rnn_launch had inline.
  int n_rnn_ok = 0, n_rnn_bad = 0;
  {
    const size_t CAP = 160 * 1024;
    auto desc = [](int cell, std::vector<int> sizes, int reverse = 0) {
      lde_rnn_desc d;
      std::memset(&d, 0, sizeof(d));
      d.abi_version = LDE_ABI_VERSION; d.cell = cell; d.n_layers = (int)sizes.size() - 1; d.reverse = reverse;
      for (size_t i = 0; i < sizes.size(); i++) d.sizes[i] = sizes[i];
      return d;
    };
    struct Laid { int rc; lde::RnnDims rd; int g0w; int64_t nW; const char* why; };
    auto lay = [&](int cell, std::vector<int> sizes, size_t cap = 160 * 1024) {
      Laid r;
      r.why = "";
      const lde_rnn_desc d = desc(cell, sizes, 1);
      r.rc = rnn_layout(&d, cap, &r.rd, &r.g0w, &r.nW, &r.why);
      assert(r.rc != LDE_OK || r.nW == rnn_num_weights(&d));
      return r;
    };
    auto two = [](const int* a, int x, int y) { return a[0] == x && a[1] == y; };
    // per-cell constants and counts
    assert(rnn_gate_rows(LDE_CELL_RNN_RELU) == 1 && rnn_gate_rows(LDE_CELL_RNN_TANH) == 1 && rnn_gate_rows(LDE_CELL_LSTM) == 4 && rnn_gate_rows(LDE_CELL_GRU) == 4);
    assert(rnn_flat_rows(LDE_CELL_RNN_RELU) == 1 && rnn_flat_rows(LDE_CELL_LSTM) == 4 && rnn_flat_rows(LDE_CELL_GRU) == 3);
    assert(rnn_state_vectors(LDE_CELL_RNN_TANH) == 1 && rnn_state_vectors(LDE_CELL_LSTM) == 2 && rnn_state_vectors(LDE_CELL_GRU) == 1);
    assert(rnn_cell_weights(LDE_CELL_LSTM, 32, 16) == 3168 && rnn_cell_weights(LDE_CELL_RNN_RELU, 32, 16) == 800 && rnn_cell_weights(LDE_CELL_RNN_TANH, 3, 2) == 14);
    assert(rnn_cell_weights(LDE_CELL_RNN_RELU, 8, 100) == 100 * 8 + 100 * 100 + 100 + 100);   // (the count is defined beyond what lde_rnn_create serves)
    for (int in : {1, 5, 32, 256}) for (int h : {1, 7, 16, 64}) assert(rnn_cell_weights(LDE_CELL_GRU, in, h) == gru_cell_weights(in, h));
    assert(rnn_cell_weights(LDE_CELL_LSTM, 0, 16) == -1 && rnn_cell_weights(LDE_CELL_LSTM, 16, -3) == -1);
    assert(rnn_cell_weights(LDE_CELL_LSTM, std::numeric_limits<int>::max(), std::numeric_limits<int>::max()) == -1);   // 4·2⁶² does not fit
    assert(rnn_cell_weights(LDE_CELL_RNN_RELU, std::numeric_limits<int>::max(), 1) == (int64_t)std::numeric_limits<int>::max() + 3);
    assert(rnn_cell_weights(LDE_CELL_RNN_RELU, std::numeric_limits<int64_t>::max(), 1) == -1);
    {
      lde_rnn_desc d = desc(LDE_CELL_LSTM, {32, 16, 16});
      assert(rnn_num_weights(&d) == 5312 && rnn_num_weights(nullptr) == -1);
      d.abi_version++;
      assert(rnn_num_weights(&d) == -1 && !rnn_desc_ok(&d));
      d = desc(LDE_CELL_RNN_RELU, {8, 100});
      assert(rnn_num_weights(&d) == 11000);
      d = desc(LDE_CELL_LSTM, {std::numeric_limits<int>::max(), std::numeric_limits<int>::max()});
      assert(rnn_desc_ok(&d) && rnn_num_weights(&d) == -1);
    }
    // the layout of the default LSTM stack 32 → 16 → 16
    const Laid lstm = lay(LDE_CELL_LSTM, {32, 16, 16});
    {
      const lde::RnnDims& r = lstm.rd;
      assert(lstm.rc == LDE_OK && r.cell == LDE_CELL_LSTM && r.nL == 2 && r.reverse == 1 && r.G == 4 && r.Hp == 64 && r.hmax == 16);
      assert(two(r.K, 48, 32) && two(r.ldk, 52, 36) && two(r.w_off, 0, 3424) && two(r.b_off, 3328, 5728) && two(r.s_off, 3392, 5792) && two(r.f_off, 0, 3168));
      assert(lstm.nW == 5312 && two(r.ldr, 68, 68) && two(r.wt_off, 5824, 9088) && r.wt == 1 && r.lds_w == 11264);
      assert(r.vmax == 52 && r.rmax == 64 && r.recw == 96 && lstm.g0w == 64 && r.sizes[0] == 32 && r.sizes[1] == 16 && r.sizes[2] == 16);
    }
    // … of the default RNN stack …
    const Laid relu = lay(LDE_CELL_RNN_RELU, {32, 16, 16});
    {
      const lde::RnnDims& r = relu.rd;
      assert(relu.rc == LDE_OK && r.G == 1 && r.Hp == 16 && r.hmax == 16 && two(r.K, 48, 32) && two(r.ldk, 52, 36));
      assert(two(r.w_off, 0, 880) && two(r.b_off, 832, 1456) && two(r.s_off, 848, 1472) && two(r.f_off, 0, 800) && relu.nW == 1344);
      assert(two(r.ldr, 20, 20) && two(r.wt_off, 1504, 2464) && r.wt == 1 && r.lds_w == 3104 && r.vmax == 52 && r.rmax == 16 && r.recw == 48 && relu.g0w == 32);
    }
    // … and of the default GRU stack: the LSTM's LDS layout (four pseudo-rows), three gate rows in the flat order, records of five rows
    const Laid gru = lay(LDE_CELL_GRU, {32, 16, 16});
    {
      const lde::RnnDims& r = gru.rd;
      assert(gru.rc == LDE_OK && r.G == 4 && r.Hp == 64 && two(r.ldk, 52, 36) && two(r.w_off, 0, 3424) && two(r.b_off, 3328, 5728) && two(r.s_off, 3392, 5792));
      assert(two(r.f_off, 0, 2368) && gru.nW == 3968 && gru.nW == gru_cell_weights(32, 16) + gru_cell_weights(16, 16) && r.f_off[1] == gru_cell_weights(32, 16));
      assert(two(r.ldr, 68, 68) && two(r.wt_off, 5824, 9088) && r.wt == 1 && r.lds_w == 11264 && r.vmax == 52 && r.rmax == 64 && r.recw == 80 && gru.g0w == 32);
    }
    // a run-time shape with three cells, and a one-layer RNN 256 → 64: served, but the transposed copy does not fit beside 16 trajectories
    const Laid nd = lay(LDE_CELL_RNN_TANH, {5, 7, 3, 9}), wide = lay(LDE_CELL_RNN_TANH, {256, 64});
    {
      const lde::RnnDims& r = nd.rd;
      assert(nd.rc == LDE_OK && r.Hp == 16 && r.hmax == 9 && r.ldk[0] == 12 && r.ldk[1] == 12 && r.ldk[2] == 12 && r.w_off[2] == 156 && r.s_off[2] == 276);
      assert(r.f_off[1] == 98 && r.f_off[2] == 134 && nd.nW == 260 && r.ldr[1] == 4 && r.wt_off[0] == 296 && r.wt_off[2] == 480 && r.wt == 1 && r.lds_w == 624);
      assert(r.vmax == 16 && r.rmax == 12 && r.recw == 27 && nd.g0w == 19);
      const lde::RnnDims& w = wide.rd;
      assert(wide.rc == LDE_OK && w.wt == 0 && w.Hp == 64 && w.ldk[0] == 324 && w.b_off[0] == 20736 && w.s_off[0] == 20800 && w.lds_w == 20928 && w.wt_off[0] == 20928);
      assert(w.ldr[0] == 68 && w.vmax == 324 && w.rmax == 64 && w.recw == 192 && wide.nW == 20608 && wide.g0w == 64);
      assert(rnn_lds_bytes(w, RNN_FORM_GENERIC, 16) == 124928 && rnn_lds_bytes(w, RNN_FORM_GENERIC, 1) == 86288);
      assert(lay(LDE_CELL_RNN_TANH, {256, 64}, 124927).rc == LDE_ERR_UNSUPPORTED && lay(LDE_CELL_RNN_TANH, {256, 64}, 124928).rc == LDE_OK);
      // with room for (20928 + 320·68 + 16·644)·4 bytes the copy is there
      assert(lay(LDE_CELL_RNN_TANH, {256, 64}, 211967).rd.wt == 0 && lay(LDE_CELL_RNN_TANH, {256, 64}, 211968).rd.wt == 1 && lay(LDE_CELL_RNN_TANH, {256, 64}, 211968).rd.lds_w == 42688);
    }
    // the three refusals, each with its text; what is no description at all
    {
      Laid r = lay(LDE_CELL_RNN_RELU, {8, 65});
      assert(r.rc == LDE_ERR_UNSUPPORTED && !std::strcmp(r.why, "recurrent stack: hidden width ≤ 64 and input width ≤ 256 supported (every cell kind, LDE_CELL_GRU included)"));
      r = lay(LDE_CELL_GRU, {257, 8});
      assert(r.rc == LDE_ERR_UNSUPPORTED && std::strstr(r.why, "input width ≤ 256"));
      assert(lay(LDE_CELL_RNN_RELU, {256, 64}).rc == LDE_OK && lay(LDE_CELL_GRU, {256, 16}).rc == LDE_OK && lay(LDE_CELL_GRU, {8, 64}).rc == LDE_OK);
      r = lay(LDE_CELL_LSTM, {8, 17});
      assert(r.rc == LDE_ERR_UNSUPPORTED && !std::strcmp(r.why, "recurrent stack: G·h ≤ 64 gate rows per cell supported (LSTM: h ≤ 16, RNN: h ≤ 64)"));
      assert(lay(LDE_CELL_LSTM, {8, 16}).rc == LDE_OK && lay(LDE_CELL_GRU, {8, 17}).rc == LDE_OK && lay(LDE_CELL_LSTM, {20, 24, 8}).rc == LDE_ERR_UNSUPPORTED);
      r = lay(LDE_CELL_RNN_RELU, {256, 64, 64, 64, 64});
      assert(r.rc == LDE_ERR_UNSUPPORTED && !std::strcmp(r.why, "recurrent stack: weights do not fit the 160 KiB LDS"));
      assert(lay(LDE_CELL_GRU, {256, 64, 64, 64, 64}).rc == LDE_ERR_UNSUPPORTED);
      lde_rnn_desc d = desc(LDE_CELL_LSTM, {32, 16, 16});
      lde::RnnDims rd;
      int g0w;
      int64_t nW;
      assert(rnn_layout(nullptr, CAP, &rd, &g0w, &nW) == LDE_ERR_INVALID_ARG && rnn_layout(&d, CAP, nullptr, &g0w, &nW) == LDE_ERR_INVALID_ARG);
      d.cell = -1;
      assert(rnn_layout(&d, CAP, &rd, &g0w, &nW) == LDE_ERR_INVALID_ARG);
      d.cell = LDE_CELL_GRU + 1;
      assert(rnn_layout(&d, CAP, &rd, &g0w, &nW) == LDE_ERR_INVALID_ARG);
      d.cell = LDE_CELL_LSTM; d.n_layers = LDE_RNN_MAX_LAYERS + 1;
      assert(rnn_layout(&d, CAP, &rd, &g0w, &nW) == LDE_ERR_INVALID_ARG);
      d.n_layers = 2; d.sizes[1] = 0;
      assert(rnn_layout(&d, CAP, &rd, &g0w, &nW) == LDE_ERR_INVALID_ARG);
    }
    // the default shape: two cells 32 → 16 → 16 WITH the transposed copies
    {
      assert(rnn_default_shape(lstm.rd) && rnn_default_shape(relu.rd) && rnn_default_shape(gru.rd) && !rnn_default_shape(nd.rd) && !rnn_default_shape(wide.rd));
      lde::RnnDims r = lstm.rd;
      r.wt = 0;
      assert(!rnn_default_shape(r));
      assert(!rnn_default_shape(lay(LDE_CELL_LSTM, {32, 16}).rd) && !rnn_default_shape(lay(LDE_CELL_LSTM, {32, 16, 16, 16}).rd));
      assert(!rnn_default_shape(lay(LDE_CELL_LSTM, {31, 16, 16}).rd) && !rnn_default_shape(lay(LDE_CELL_LSTM, {32, 15, 16}).rd) && !rnn_default_shape(lay(LDE_CELL_LSTM, {32, 16, 12}).rd));
    }
    // the per-call plan on both sides of every threshold; LDS bytes as the two expressions rnn_launch had
    auto plan_is = [](const RnnPlan& p, RnnForm f, int tpw, unsigned block, unsigned grid, size_t lds) {
      return p.form == f && p.tpw == tpw && p.block == block && p.grid == grid && p.lds_bytes == lds;
    };
    auto plan = [](const Laid& s, int B, int generic = 0, int regw = 1, int pipe = 1, bool prof = false) { return rnn_launch_plan(s.rd, B, generic, regw, pipe, prof); };
    auto old_lds = [](const lde::RnnDims& r, bool pipe, int tpw) {
      return pipe ? ((size_t)r.lds_w + 2 * tpw * (r.vmax + r.rmax + 4 * 16) + 2 * 8 * tpw * 16 + 16) * sizeof(float)
                  : ((size_t)r.lds_w + tpw * ((size_t)r.vmax + r.rmax + 4 * r.nL * r.hmax)) * sizeof(float);
    };
    for (const Laid* s : {&lstm, &gru}) {   // 64 lanes per trajectory: one trajectory per workgroup up to B = 1024, then 2, 4, 8, 16
      assert(plan_is(plan(*s, 1), RNN_FORM_PIPE, 1, 128, 16, 47584) && plan_is(plan(*s, 5), RNN_FORM_PIPE, 1, 128, 16, 47584));
      assert(plan_is(plan(*s, 1024), RNN_FORM_PIPE, 1, 128, 1024, 47584) && plan_is(plan(*s, 1025), RNN_FORM_ROWS_LDS, 2, 128, 520, 47008));
      assert(plan_is(plan(*s, 2048), RNN_FORM_ROWS_LDS, 2, 128, 1024, 47008) && plan_is(plan(*s, 2049), RNN_FORM_ROWS_LDS, 4, 256, 516, 48960));
      assert(plan_is(plan(*s, 4096), RNN_FORM_ROWS_LDS, 4, 256, 1024, 48960) && plan_is(plan(*s, 4097), RNN_FORM_ROWS_LDS, 8, 512, 514, 52864));
      assert(plan_is(plan(*s, 8192), RNN_FORM_ROWS_LDS, 8, 512, 1024, 52864) && plan_is(plan(*s, 8193), RNN_FORM_ROWS_LDS, 16, 1024, 513, 60672));
      assert(plan_is(plan(*s, 16385), RNN_FORM_ROWS_LDS, 16, 1024, 1025, 60672) && plan_is(plan(*s, 100000), RNN_FORM_ROWS_LDS, 16, 1024, 6250, 60672));
      // the options: "pipe" = 0 and an LDE_PROF build keep the single wave, "regw" = 0 the LDS rows, "generic" the run-time-shaped kernel
      assert(plan_is(plan(*s, 1024, 0, 1, 0), RNN_FORM_ROWS_REG, 1, 64, 1024, 46032) && plan_is(plan(*s, 1024, 0, 1, 1, true), RNN_FORM_ROWS_REG, 1, 64, 1024, 46032));
      assert(plan_is(plan(*s, 1024, 0, 0, 1), RNN_FORM_ROWS_LDS, 1, 64, 1024, 46032) && plan_is(plan(*s, 1024, 1, 1, 1), RNN_FORM_GENERIC, 1, 64, 1024, 46032));
      assert(plan(*s, 1025, 0, 1, 0).form == RNN_FORM_ROWS_LDS && plan(*s, 1025, 0, 1, 1, true).form == RNN_FORM_ROWS_LDS && plan(*s, 1025, 1).form == RNN_FORM_GENERIC);
      assert(plan(*s, 5, 0, 7, 3).form == RNN_FORM_PIPE && plan(*s, 5, 2).form == RNN_FORM_GENERIC);   // any non-zero value switches
    }
    // 16 lanes per trajectory: four trajectories fill the wave up to B = 4096
    assert(plan_is(plan(relu, 1), RNN_FORM_PIPE, 4, 128, 4, 20800) && plan_is(plan(relu, 4096), RNN_FORM_PIPE, 4, 128, 1024, 20800));
    assert(plan_is(plan(relu, 4097), RNN_FORM_ROWS_LDS, 8, 128, 514, 18688) && plan_is(plan(relu, 8192), RNN_FORM_ROWS_LDS, 8, 128, 1024, 18688));
    assert(plan_is(plan(relu, 8193), RNN_FORM_ROWS_LDS, 16, 256, 513, 24960) && plan_is(plan(relu, 100000), RNN_FORM_ROWS_LDS, 16, 256, 6250, 24960));
    assert(plan_is(plan(relu, 4096, 0, 1, 0), RNN_FORM_ROWS_REG, 4, 64, 1024, 15552) && plan_is(plan(relu, 4096, 0, 0), RNN_FORM_ROWS_LDS, 4, 64, 1024, 15552));
    assert(plan(relu, 4096, 0, 1, 1, true).form == RNN_FORM_ROWS_REG && plan(relu, 4096, 1).form == RNN_FORM_GENERIC && plan(relu, 4097, 0, 1, 0).form == RNN_FORM_ROWS_LDS);
    assert(plan(lay(LDE_CELL_RNN_TANH, {8, 4}), 5).tpw == 16 && plan(lay(LDE_CELL_RNN_TANH, {8, 4}), 5).grid == 1 && plan(lay(LDE_CELL_RNN_TANH, {8, 2}), 5).tpw == 32 && plan(lay(LDE_CELL_RNN_TANH, {8, 2}), 5).grid == 0);
    // a shape without instantiation: always the run-time-shaped kernel, the same workgroup rule
    for (int B : {1, 5, 1024, 4096, 4097, 8193, 100000})
      for (int o = 0; o < 16; o++) assert(plan(nd, B, o & 1, (o >> 1) & 1, (o >> 2) & 1, (o >> 3) & 1).form == RNN_FORM_GENERIC && plan(wide, B, o & 1, (o >> 1) & 1, (o >> 2) & 1, (o >> 3) & 1).form == RNN_FORM_GENERIC);
    assert(plan_is(plan(nd, 4096), RNN_FORM_GENERIC, 4, 64, 1024, 4672) && plan_is(plan(nd, 4097), RNN_FORM_GENERIC, 8, 128, 514, 6848) && plan_is(plan(nd, 8193), RNN_FORM_GENERIC, 16, 256, 513, 11200));
    assert(plan_is(plan(wide, 1024), RNN_FORM_GENERIC, 1, 64, 1024, 86288) && plan_is(plan(wide, 1025), RNN_FORM_GENERIC, 2, 128, 520, 88864) && plan_is(plan(wide, 8193), RNN_FORM_GENERIC, 16, 1024, 513, 124928));
    for (const Laid* s : {&lstm, &relu, &gru, &nd, &wide})
      for (int tpw : {1, 2, 4, 8, 16}) {
        for (RnnForm f : {RNN_FORM_GENERIC, RNN_FORM_ROWS_LDS, RNN_FORM_ROWS_REG}) assert(rnn_lds_bytes(s->rd, f, tpw) == old_lds(s->rd, false, tpw));
        assert(rnn_lds_bytes(s->rd, RNN_FORM_PIPE, tpw) == old_lds(s->rd, true, tpw));
      }
    // groupable: the two single-wave forms of a default RNN / LSTM stack
    assert(rnn_groupable(lstm.rd, RNN_FORM_PIPE) && rnn_groupable(lstm.rd, RNN_FORM_ROWS_REG) && rnn_groupable(relu.rd, RNN_FORM_PIPE) && rnn_groupable(relu.rd, RNN_FORM_ROWS_REG));
    assert(!rnn_groupable(lstm.rd, RNN_FORM_ROWS_LDS) && !rnn_groupable(lstm.rd, RNN_FORM_GENERIC) && !rnn_groupable(relu.rd, RNN_FORM_GENERIC));
    for (RnnForm f : {RNN_FORM_GENERIC, RNN_FORM_ROWS_LDS, RNN_FORM_ROWS_REG, RNN_FORM_PIPE}) assert(!rnn_groupable(gru.rd, f) && !rnn_groupable(nd.rd, f) && !rnn_groupable(wide.rd, f));
    // the k-split of the weight gradient: ⌈512 / (tiles × jobs)⌉ clamped to 1 … 8
    assert(rnn_dw_ksplit(1, 1) == 8 && rnn_dw_ksplit(16, 4) == 8 && rnn_dw_ksplit(64, 1) == 8 && rnn_dw_ksplit(65, 1) == 8 && rnn_dw_ksplit(73, 1) == 8 && rnn_dw_ksplit(74, 1) == 7);
    assert(rnn_dw_ksplit(16, 8) == 4 && rnn_dw_ksplit(256, 1) == 2 && rnn_dw_ksplit(511, 1) == 2 && rnn_dw_ksplit(512, 1) == 1 && rnn_dw_ksplit(513, 1) == 1 && rnn_dw_ksplit(6250, 4) == 1);
    assert(rnn_dw_ksplit(0, 4) == 8 && rnn_dw_ksplit(-3, 4) == 8 && rnn_dw_ksplit(std::numeric_limits<int>::max(), std::numeric_limits<int>::max()) == 1);
    // the shaped kernels' template arguments: four cell kinds × four modes, nothing else
    {
      int seen[4][4] = {};
      auto rec = [&](auto C, auto M) -> int { seen[decltype(C)::value][decltype(M)::value]++; return 10 * decltype(C)::value + decltype(M)::value; };
      static_assert(LDE_CELL_RNN_RELU == 0 && LDE_CELL_RNN_TANH == 1 && LDE_CELL_LSTM == 2 && LDE_CELL_GRU == 3, "cell codes");
      for (int c = 0; c < 4; c++)
        for (int m = 0; m < 4; m++) assert(rnn_dispatch(c, m, rec) == 10 * c + m && seen[c][m] == 1);
      assert(rnn_dispatch(-1, 0, rec) == LDE_ERR_UNSUPPORTED && rnn_dispatch(4, 0, rec) == LDE_ERR_UNSUPPORTED && rnn_dispatch(2, 4, rec) == LDE_ERR_UNSUPPORTED && rnn_dispatch(2, -1, rec) == LDE_ERR_UNSUPPORTED);
      int modes = 0;
      for (int m = -2; m < 7; m++) assert(rnn_dispatch_mode(m, [&](auto M) -> int { modes++; return decltype(M)::value; }) == (m >= 0 && m < 4 ? m : (int)LDE_ERR_UNSUPPORTED));
      assert(modes == 4);
      for (int it = 0; it < 20000; it++) {
        const int c = hostile_int(), m = hostile_int();
        int called = 0;
        const int rc = rnn_dispatch(c, m, [&](auto, auto) -> int { called++; return LDE_OK; });
        assert(called == (c >= 0 && c < 4 && m >= 0 && m < 4) && rc == (called ? LDE_OK : LDE_ERR_UNSUPPORTED));
      }
    }
    // hostile descriptions: a status for every one, no arithmetic on what is refused; an accepted layout has its areas in ascending order
    // and inside the weight area, the weight area with 16 trajectories' buffers inside the LDS, the cells in order in the flat vector
    for (int it = 0; it < 200000; it++) {
      lde_rnn_desc d = desc((int)(rnd() % 4), {32, 16, 16}, (int)(rnd() & 1));
      d.n_layers = 1 + (int)(rnd() % LDE_RNN_MAX_LAYERS);
      for (int l = 0; l <= LDE_RNN_MAX_LAYERS; l++) d.sizes[l] = (rnd() % 3) ? 1 + (int)(rnd() % (l == 0 ? 300 : 70)) : 1 + (int)(rnd() % 20);
      const int nmut = (int)(rnd() % 3);
      for (int m = 0; m < nmut; m++) {
        switch (rnd() % 5) {
          case 0: d.abi_version = hostile_int(); break;
          case 1: d.cell = hostile_int(); break;
          case 2: d.n_layers = hostile_int(); break;
          case 3: d.reverse = hostile_int(); break;
          default: d.sizes[rnd() % (LDE_RNN_MAX_LAYERS + 1)] = hostile_int(); break;
        }
      }
      const size_t cap = (rnd() & 3) ? CAP : (rnd() & 1) ? (size_t)(rnd() % (2 * CAP)) : (size_t)rnd();
      lde::RnnDims rd;
      int g0w = -1;
      int64_t nW = -1;
      const char* why = nullptr;
      const int rc = rnn_layout(&d, cap, &rd, &g0w, &nW, &why);
      const int64_t cnt = rnn_num_weights(&d);
      assert((cnt >= 0) == rnn_desc_ok(&d) || cnt == -1);
      if (rc != LDE_OK) {
        n_rnn_bad++;
        assert(rc == LDE_ERR_INVALID_ARG ? !rnn_desc_ok(&d) : (rc == LDE_ERR_UNSUPPORTED && why && std::strstr(why, "recurrent stack: ")));
        continue;
      }
      n_rnn_ok++;
      assert(nW == cnt && nW > 0 && g0w > 0 && rd.Hp >= 1 && rd.Hp <= 64 && (rd.Hp & (rd.Hp - 1)) == 0 && rd.nL == d.n_layers && rd.reverse == (d.reverse ? 1 : 0));
      assert(rd.cell == LDE_CELL_GRU ? rd.Hp == gru_lanes(rd.hmax) : rd.Hp >= rd.G * rd.hmax);
      int end = 0;
      int64_t fend = 0;
      for (int l = 0; l < rd.nL; l++) {
        const int h = rd.sizes[l + 1], R = rd.G * h;
        assert(rd.K[l] == rd.sizes[l] + h && rd.ldk[l] >= rd.K[l] && rd.ldk[l] % 4 == 0 && ((rd.ldk[l] / 4) & 1) && rd.ldk[l] <= rd.vmax && R <= rd.rmax);
        assert(rd.w_off[l] == end && rd.b_off[l] == rd.w_off[l] + R * rd.ldk[l] && rd.s_off[l] >= rd.b_off[l] + R && rd.s_off[l] % 4 == 0);
        end = rd.s_off[l] + ((2 * h + 3) & ~3);
        assert(rd.f_off[l] == fend);
        fend += rnn_cell_weights(rd.cell, rd.sizes[l], h);
      }
      assert(fend == nW);
      for (int l = 0; l < rd.nL; l++) {
        assert(rd.wt_off[l] == end && rd.ldr[l] >= rd.G * rd.sizes[l + 1] && ((rd.ldr[l] / 4) & 1) && rd.ldr[l] % 4 == 0);
        end += rd.K[l] * rd.ldr[l];
      }
      assert(rd.lds_w == (rd.wt ? end : rd.wt_off[0]) && rnn_lds_bytes(rd, RNN_FORM_GENERIC, 16) <= cap);
      // … and its plan for any batch and options: a form the stack has, a grid that covers whole staging tiles, LDS within the 16-trajectory bound
      const int B = (rnd() & 1) ? 1 + (int)(rnd() % 20000) : hostile_int();
      const RnnPlan p = rnn_launch_plan(rd, B, (int)(rnd() & 1), (int)(rnd() & 1), (int)(rnd() & 1), rnd() & 1);
      // (a stack no wider than two gate rows — Hp ≤ 2 — starts at 32 / 64 trajectories per workgroup, more than a staging tile: grid 0, a
      //  launch the runtime refuses. As the launch code always had it; pinned, not served.)
      assert(p.tpw >= 1 && p.tpw <= 64 && (p.tpw & (p.tpw - 1)) == 0 && p.tpw * rd.Hp >= 64 && p.block >= 64 && p.block <= 1024 && (p.tpw <= 16) == (rd.Hp >= 4));
      assert(rnn_default_shape(rd) || p.form == RNN_FORM_GENERIC);
      if (p.form == RNN_FORM_PIPE || p.form == RNN_FORM_ROWS_REG) assert(p.tpw * rd.Hp == 64);
      if (p.form != RNN_FORM_PIPE && p.tpw <= 16) assert(p.lds_bytes <= cap);
      if (p.tpw > 16) assert(p.grid == 0);
      else if (B >= 1) assert((int64_t)p.grid * p.tpw >= B && (int64_t)p.grid * p.tpw % 16 == 0 && (int64_t)p.grid * p.tpw < (int64_t)B + 16);
      else assert(p.grid == 0);
      (void)rnn_dw_ksplit(hostile_int(), hostile_int());
    }
    assert(n_rnn_ok > 1000 && n_rnn_bad > 1000);
    {   // a plan never divides by what a layout did not produce
      lde::RnnDims z{};
      const RnnPlan p = rnn_launch_plan(z, std::numeric_limits<int>::max(), 0, 1, 1, false);
      assert(p.form == RNN_FORM_GENERIC && p.tpw == 64 && p.block == 64 && p.grid == 0);
      z.Hp = 4;
      assert(rnn_launch_plan(z, std::numeric_limits<int>::max(), 0, 1, 1, false).grid == 134217728u);
      z.Hp = std::numeric_limits<int>::max(); z.lds_w = z.vmax = z.rmax = z.hmax = z.nL = std::numeric_limits<int>::max();
      (void)rnn_launch_plan(z, std::numeric_limits<int>::min(), 1, 1, 1, true);
      (void)rnn_lds_bytes(z, RNN_FORM_PIPE, std::numeric_limits<int>::max());
    }
  }
  std::printf("host logic under ASan + UBSan: %d accepted, %d refused hostile descriptions; forward mappings as measured; "
              "pullback mappings, ring shapes and kernel dispatch checked; MLP family mappings as measured, reserve rows and solver dispatch checked\n", n_ok, n_bad);
  std::printf("dense chains: LDS bytes, tile picks, call layouts, tile narrowing and weight-gradient splits as measured; hostile sizes checked\n");
  std::printf("recurrent stacks: weight counts, layouts, refusals, launch plans, groupability, k-split and kernel dispatch as in the launch code; "
              "%d accepted, %d refused hostile descriptions\n", n_rnn_ok, n_rnn_bad);
  return 0;
}
