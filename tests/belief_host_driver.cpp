// belief_host_driver.cpp — what csrc/lde_host.h decides about the AdaBelief step (lde_adabelief_flux_step*, include/lde.h: "the AdaBelief
// step") without a device: the ε refusal it adds (belief_eps_ok) on top of what its ADAMW twin refuses (opt_args_ok, clip_args_ok), and the
// launch plan its update walks (opt_next_launch at OPT_PER_WG: every non-empty array in exactly one launch, every element in exactly one
// workgroup's slice, ONE launch flagged as the step's last — the one whose last workgroup advances the count). Compiled with an ordinary
// host compiler under AddressSanitizer + UndefinedBehaviorSanitizer and run as a program by tests/test_belief_host.py.
#undef NDEBUG
#include <cassert>
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "../latentdiffeq.jl_amd/csrc/lde_host.h"

using namespace lde_host;

static std::vector<lde_adam_tensor> arrays(const std::vector<int64_t>& sizes, float* where) {
  std::vector<lde_adam_tensor> t(sizes.size());
  for (size_t i = 0; i < sizes.size(); i++) {
    t[i] = lde_adam_tensor{};
    t[i].n = sizes[i];
    if (sizes[i] > 0) t[i].p = t[i].m = t[i].v = where, t[i].g = where;   // never dereferenced
  }
  return t;
}

// the update's plan, walked the way the launcher and k_adabelief_flux walk it; returns the number of launches
static int check_update_plan(const std::vector<int64_t>& sizes) {
  float dummy[4];
  std::vector<lde_adam_tensor> t = arrays(sizes, dummy);
  const int n = (int)t.size();
  std::vector<int64_t> covered(sizes.size(), 0);
  int launches = 0, lasts = 0, prev = -1;
  for (int first = 0; first < n;) {
    const OptLaunch L = opt_next_launch(n, t.data(), first, OPT_PER_WG);
    assert(!L.too_large);
    first = L.next;
    if (L.n == 0) break;
    launches++;
    lasts += L.last ? 1 : 0;
    assert(L.n <= OPT_MAXT && L.blk0[0] == 0);
    for (int b = 0; b < L.blk0[L.n]; b++) {   // every workgroup: its array and its slice
      int i = 0;
      while (i + 1 < L.n && b >= L.blk0[i + 1]) i++;
      const lde_adam_tensor& a = t[(size_t)L.idx[i]];
      const int64_t lo = (int64_t)(b - L.blk0[i]) * OPT_PER_WG;
      const int64_t hi = lo + OPT_PER_WG < a.n ? lo + OPT_PER_WG : a.n;
      assert(lo < hi && hi <= a.n);           // no workgroup without an element, none past the end
      covered[(size_t)L.idx[i]] += hi - lo;
    }
    for (int i = 0; i < L.n; i++) {
      assert(L.idx[i] > prev && t[(size_t)L.idx[i]].n > 0);
      prev = L.idx[i];
    }
    bool more = false;
    for (int j = first; j < n; j++) more = more || t[(size_t)j].n > 0;
    assert(L.last == !more);
  }
  for (size_t i = 0; i < sizes.size(); i++) assert(covered[i] == sizes[i]);
  assert(lasts == (launches ? 1 : 0));        // the count is bumped once per step
  return launches;
}

int main() {
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  int checks = 0;
  // 1. the ε refusal
  assert(belief_eps_ok(1e-16f, 1e-16f) && belief_eps_ok(1e-8f, 1e-8f) && belief_eps_ok(0.f, 0.f) && belief_eps_ok(0.f, 1e-3f) && belief_eps_ok(-0.f, 0.f));
  assert(belief_eps_ok(std::numeric_limits<float>::denorm_min(), std::numeric_limits<float>::max()));
  for (float bad : {-1.0f, -1e-30f, nan, -nan, inf, -inf}) {
    assert(!belief_eps_ok(bad, 1e-8f));
    assert(!belief_eps_ok(1e-8f, bad));
    assert(!belief_eps_ok(bad, bad));
    checks += 3;
  }
  // 2. what the ADAMW twin refuses holds for this rule's table too (v holds s): the same functions, called the way belief_impl calls them
  {
    float dummy[4];
    std::vector<lde_adam_tensor> t = arrays({4, 0, 9}, dummy);
    alignas(8) char ws[64];
    const void* P = ws;
    assert(opt_args_ok(3, t.data(), 0.9f, 0.999f, 1, nullptr) && opt_args_ok(3, t.data(), 0.9f, 0.999f, 0, P));
    assert(!opt_args_ok(3, t.data(), 0.9f, 0.999f, 0, nullptr));                                     // host-counted: t ≥ 1
    assert(!opt_args_ok(-1, t.data(), 0.9f, 0.999f, 1, nullptr) && !opt_args_ok(3, nullptr, 0.9f, 0.999f, 1, nullptr));
    for (float b : {1.0f, -0.1f, nan, inf}) assert(!opt_args_ok(3, t.data(), b, 0.999f, 1, nullptr) && !opt_args_ok(3, t.data(), 0.9f, b, 1, nullptr));
    t[2].v = nullptr;                                                                                // the array that holds s
    assert(!opt_args_ok(3, t.data(), 0.9f, 0.999f, 1, nullptr));
    assert(!clip_args_ok(3, t.data(), 0.9f, 0.999f, 1.0f, LDE_CLIP_GLOBAL, P, P, P, P));
    t[2].v = dummy;
    assert(clip_args_ok(3, t.data(), 0.9f, 0.999f, 1.0f, LDE_CLIP_PER_ARRAY, P, P, P, P));
    t[0].n = (int64_t)OPT_MAX_BLOCKS * OPT_PER_WG + 1;                                              // an array no update launch holds
    assert(!clip_args_ok(3, t.data(), 0.9f, 0.999f, 1.0f, LDE_CLIP_GLOBAL, P, P, P, P));
    assert(opt_next_launch(3, t.data(), 0, OPT_PER_WG).too_large);
    checks += 12;
  }
  // 3. the update's plan on the sizes of tests/test_gpu_belief.py and around the table size
  static_assert(OPT_PER_WG == 2048 && OPT_MAXT == 48, "the sizes of tests/test_gpu_belief.py are chosen around these");
  assert(check_update_plan({1, 0, 5, 2047, 2048, 2049, 8193, 3 * 2048 + 7}) == 1);
  assert(check_update_plan({}) == 0 && check_update_plan({0, 0}) == 0);
  for (int count : {1, 47, 48, 49, 96, 97}) {
    for (int empties = 0; empties < 3; empties++) {
      std::vector<int64_t> sizes;
      for (int i = 0; i < count; i++) {
        if (empties == 1 && i % 3 == 1) sizes.push_back(0);
        if (empties == 2) { sizes.push_back(0); sizes.push_back(0); }
        sizes.push_back(1 + (int64_t)(i * 977) % 5000);
      }
      if (empties) sizes.push_back(0);
      assert(check_update_plan(sizes) == (count + OPT_MAXT - 1) / OPT_MAXT);
      checks++;
    }
  }
  std::printf("AdaBelief step host logic under ASan + UBSan: %d checks (the eps refusal, the twin's refusals, the update's plan: one slice per workgroup, the count bumped once)\n", checks);
  return 0;
}
