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
  std::printf("host logic under ASan + UBSan: %d accepted, %d refused hostile descriptions; forward mappings as measured; "
              "pullback mappings, ring shapes and kernel dispatch checked; MLP family mappings as measured, reserve rows and solver dispatch checked\n", n_ok, n_bad);
  std::printf("dense chains: LDS bytes, tile picks, call layouts, tile narrowing and weight-gradient splits as measured; hostile sizes checked\n");
  return 0;
}
