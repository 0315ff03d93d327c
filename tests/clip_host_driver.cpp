// clip_host_driver.cpp — what csrc/lde_host.h decides about the clipped step (lde_adamw_flux_step_clipped, include/lde.h: "the clipped
// step"): the workspace plan (clip_plan: the slot base of every scan launch, every array's range of partials, where the sums, the
// descriptors and the scales lie) and the refusals that need no device (clip_args_ok) — compiled with an ordinary host compiler under
// AddressSanitizer + UndefinedBehaviorSanitizer and run as a program by tests/test_clip_host.py. The "device" side is played here on a
// byte buffer of exactly clip_plan(...).bytes bytes: every write the kernels make is made into it, so a slot outside it is an ASan report.
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

static std::vector<lde_adam_tensor> arrays(const std::vector<int64_t>& sizes) {
  std::vector<lde_adam_tensor> t(sizes.size());
  for (size_t i = 0; i < sizes.size(); i++) {
    t[i] = lde_adam_tensor{};
    t[i].n = sizes[i];
  }
  return t;
}

struct Seen {
  int launches = 0;
  int64_t slots = 0, nne = 0;
};

// The plan of one table, walked the way the launcher and the kernels walk it.
static Seen check_plan(int n, const lde_adam_tensor* t) {
  const ClipWs w = clip_plan(n, t, [](const OptLaunch&, int64_t, int64_t) {});
  int64_t want_slots = 0, want_nne = 0;
  for (int i = 0; i < n; i++)
    if (t[i].n > 0) {
      want_slots += (t[i].n - 1) / GUARD_PER_WG + 1;
      want_nne++;
    }
  assert(w.slots == want_slots && w.nne == want_nne);
  // the four regions in order, disjoint, aligned for what they hold, and the total is the last one's end
  assert(w.off_sums == 8 * (size_t)w.slots && w.off_desc == w.off_sums + 8 * (size_t)w.nne && w.off_scale == w.off_desc + sizeof(ClipDesc) * (size_t)w.nne);
  assert(w.bytes == w.off_scale + 4 * (size_t)w.nne && w.off_sums % 8 == 0 && w.off_desc % 8 == 0 && w.off_scale % 4 == 0);
  static_assert(sizeof(ClipDesc) == 16 && alignof(ClipDesc) == 8, "the descriptor's layout");
  assert((w.bytes == 0) == (w.nne == 0));

  std::vector<unsigned char> ws(w.bytes);   // exactly the bytes the caller was told to bring
  std::vector<int> hits((size_t)w.slots, 0);
  std::vector<int> desc_hits((size_t)w.nne, 0);
  Seen seen;
  int prev = -1;
  const ClipWs again = clip_plan(n, t, [&](const OptLaunch& L, int64_t slot0, int64_t ord0) {
    assert(slot0 == seen.slots && ord0 == seen.nne);   // a launch starts where the one before it ended
    assert(L.n > 0 && L.blk0[0] == 0);
    // every workgroup of the launch: exactly one slot, found the way k_grad_norm_guard finds it (part + slot0)[blockIdx.x]
    for (int b = 0; b < L.blk0[L.n]; b++) {
      int i = 0;
      while (i + 1 < L.n && b >= L.blk0[i + 1]) i++;
      const int64_t slot = slot0 + b;
      assert(slot >= 0 && slot < w.slots);
      hits[(size_t)slot]++;
      const double one = 1.0;
      std::memcpy(ws.data() + 8 * (size_t)slot, &one, 8);   // inside the buffer, or ASan says so
      if (b == L.blk0[i]) {                                   // the workgroup that owns the array's first slice leaves the descriptor
        ClipDesc d;
        d.slot0 = slot0 + L.blk0[i];
        d.nslots = L.blk0[i + 1] - L.blk0[i];
        d.idx = L.idx[i];
        assert(ord0 + i < w.nne);
        desc_hits[(size_t)(ord0 + i)]++;
        std::memcpy(ws.data() + w.off_desc + sizeof(ClipDesc) * (size_t)(ord0 + i), &d, sizeof d);
      }
    }
    for (int i = 0; i < L.n; i++) {
      assert(L.idx[i] > prev);   // ordinals follow the caller's order
      prev = L.idx[i];
    }
    seen.launches++;
    seen.slots += L.blk0[L.n];
    seen.nne += L.n;
  });
  assert(again.bytes == w.bytes && seen.slots == w.slots && seen.nne == w.nne);
  for (int h : hits) assert(h == 1);        // disjoint, none unwritten — the last slot included
  for (int h : desc_hits) assert(h == 1);
  if (w.slots > 0) assert(hits[(size_t)w.slots - 1] == 1);
  // the finalising kernel's view: per ordinal a range of partials; the ranges tile [0, slots) in order; the array is the right one
  int64_t next = 0, ord = 0;
  for (int i = 0; i < n; i++) {
    if (t[i].n <= 0) continue;
    ClipDesc d;
    std::memcpy(&d, ws.data() + w.off_desc + sizeof(ClipDesc) * (size_t)ord, sizeof d);
    assert(d.idx == i && d.slot0 == next && d.nslots == (t[i].n - 1) / GUARD_PER_WG + 1);
    for (int j = 0; j < d.nslots; j++) {
      double v;
      std::memcpy(&v, ws.data() + 8 * (size_t)(d.slot0 + j), 8);
      assert(v == 1.0);
    }
    const double s = (double)d.nslots;
    std::memcpy(ws.data() + w.off_sums + 8 * (size_t)ord, &s, 8);
    const float sc = 1.0f;
    std::memcpy(ws.data() + w.off_scale + 4 * (size_t)ord, &sc, 4);   // the last scale ends at w.bytes
    next += d.nslots;
    ord++;
  }
  assert(next == w.slots && ord == w.nne);
  // the update's launches (another slice, possibly another packing) take the scales launch by launch in the same order
  int64_t uord = 0;
  int uprev = -1;
  for (int first = 0; first < n;) {
    const OptLaunch L = opt_next_launch(n, t, first, OPT_PER_WG);
    first = L.next;
    if (L.n == 0) break;
    for (int i = 0; i < L.n; i++) {
      ClipDesc d;
      std::memcpy(&d, ws.data() + w.off_desc + sizeof(ClipDesc) * (size_t)(uord + i), sizeof d);
      assert(d.idx == L.idx[i] && L.idx[i] > uprev);   // scale[uord + i] is array L.idx[i]'s
      uprev = L.idx[i];
    }
    uord += L.n;
  }
  assert(uord == w.nne);
  return seen;
}

int main() {
  const int64_t S = GUARD_PER_WG;
  static_assert(GUARD_PER_WG == 8192 && GUARD_PER_WG / OPT_WG == 32, "a lane of the scan sees at most 32 elements: the bound of tests/test_gpu_clip.py");
  const int64_t around[] = {1, 2, 3, 5, S - 1, S, S + 1, 2 * S - 1, 2 * S, 2 * S + 7, 3 * S + 1, 2047, 2048, 2049};
  const int NA = (int)(sizeof(around) / sizeof(around[0]));
  int plans = 0;
  // 1. the array counts around the table size, sizes around the slice, with and without empty arrays in between
  for (int count : {0, 1, 47, 48, 49, 97}) {
    for (int empties = 0; empties < 3; empties++) {
      for (int shift = 0; shift < 5; shift++) {
        std::vector<int64_t> sizes;
        for (int i = 0; i < count; i++) {
          if (empties == 1 && i % 3 == 1) sizes.push_back(0);
          if (empties == 2) { sizes.push_back(0); sizes.push_back(0); }
          sizes.push_back(around[(i * 5 + shift * 3) % NA]);
        }
        if (empties) sizes.push_back(0);
        std::vector<lde_adam_tensor> t = arrays(sizes);
        const Seen s = check_plan((int)t.size(), t.data());
        assert(s.launches == (count + OPT_MAXT - 1) / OPT_MAXT && s.nne == count);
        plans++;
      }
    }
  }
  // nothing to plan
  {
    const ClipWs z = clip_plan(0, nullptr, [](const OptLaunch&, int64_t, int64_t) { assert(false); });
    assert(z.bytes == 0 && z.slots == 0 && z.nne == 0);
    std::vector<lde_adam_tensor> t = arrays({0, 0, 0});
    assert(check_plan(3, t.data()).launches == 0);
  }
  // one large array: 2²⁶ floats are 8 192 slots, one launch
  {
    std::vector<lde_adam_tensor> t = arrays({(int64_t)1 << 26});
    const ClipWs w = clip_plan(1, t.data(), [](const OptLaunch&, int64_t, int64_t) {});
    assert(w.slots == 8192 && w.nne == 1 && w.bytes == 8 * 8192 + 8 + 16 + 4);
  }
  // 2. any table
  for (int it = 0; it < 20000; it++) {
    const int n = (int)(rnd() % 120);
    std::vector<int64_t> sizes(n);
    for (int i = 0; i < n; i++) {
      const uint64_t r = rnd() % 10;
      sizes[i] = r < 2 ? 0 : r < 6 ? (int64_t)(rnd() % 5000) : r < 9 ? around[rnd() % NA] : (int64_t)(rnd() % (3 * S));
    }
    std::vector<lde_adam_tensor> t = arrays(sizes);
    check_plan(n, t.data());
    plans++;
  }
  // 3. the refusals that need no device
  {
    std::vector<lde_adam_tensor> t = arrays({4, 0, 9});
    float dummy[4];
    for (auto& a : t)
      if (a.n > 0) a.p = a.m = a.v = dummy, a.g = dummy;
    alignas(8) char ws[64];
    const void* P = ws;   // a non-NULL pointer; nothing is dereferenced
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    assert(clip_args_ok(3, t.data(), 0.9f, 0.999f, 1.0f, LDE_CLIP_GLOBAL, P, P, P, P));
    assert(clip_args_ok(3, t.data(), 0.9f, 0.999f, 1e-30f, LDE_CLIP_PER_ARRAY, P, P, P, P));
    assert(!clip_args_ok(3, t.data(), 0.9f, 0.999f, 1.0f, LDE_CLIP_GLOBAL, nullptr, P, P, P));   // step_dev
    assert(!clip_args_ok(3, t.data(), 0.9f, 0.999f, 1.0f, LDE_CLIP_GLOBAL, P, nullptr, P, P));   // guard_dev
    assert(!clip_args_ok(3, t.data(), 0.9f, 0.999f, 1.0f, LDE_CLIP_GLOBAL, P, P, nullptr, P));   // ws_dev with non-empty arrays
    assert(!clip_args_ok(3, t.data(), 0.9f, 0.999f, 1.0f, LDE_CLIP_GLOBAL, P, P, ws + 4, P));    // … or one that cannot hold an f64
    assert(!clip_args_ok(3, t.data(), 0.9f, 0.999f, 1.0f, LDE_CLIP_GLOBAL, P, P, P, nullptr));   // norms_dev
    for (float c : {0.0f, -1.0f, nan, inf, -inf}) assert(!clip_args_ok(3, t.data(), 0.9f, 0.999f, c, LDE_CLIP_GLOBAL, P, P, P, P));
    for (int mode : {-1, 2, 7}) assert(!clip_args_ok(3, t.data(), 0.9f, 0.999f, 1.0f, mode, P, P, P, P));
    // what lde_adamw_flux_step_dev refuses
    assert(!clip_args_ok(-1, t.data(), 0.9f, 0.999f, 1.0f, LDE_CLIP_GLOBAL, P, P, P, P));
    assert(!clip_args_ok(3, nullptr, 0.9f, 0.999f, 1.0f, LDE_CLIP_GLOBAL, P, P, P, P));
    assert(!clip_args_ok(3, t.data(), 1.0f, 0.999f, 1.0f, LDE_CLIP_GLOBAL, P, P, P, P));
    assert(!clip_args_ok(3, t.data(), 0.9f, nan, 1.0f, LDE_CLIP_GLOBAL, P, P, P, P));
    t[2].g = nullptr;
    assert(!clip_args_ok(3, t.data(), 0.9f, 0.999f, 1.0f, LDE_CLIP_GLOBAL, P, P, P, P));
    t[2].g = dummy;
    t[2].n = -3;
    assert(!clip_args_ok(3, t.data(), 0.9f, 0.999f, 1.0f, LDE_CLIP_GLOBAL, P, P, P, P));
    t[2].n = (int64_t)OPT_MAX_BLOCKS * OPT_PER_WG + 1;   // an array no update launch holds
    assert(!clip_args_ok(3, t.data(), 0.9f, 0.999f, 1.0f, LDE_CLIP_GLOBAL, P, P, P, P));
    // only empty arrays, or none: no workspace needed
    std::vector<lde_adam_tensor> e = arrays({0, 0});
    assert(clip_args_ok(2, e.data(), 0.9f, 0.999f, 1.0f, LDE_CLIP_GLOBAL, P, P, nullptr, P));
    assert(clip_args_ok(0, nullptr, 0.9f, 0.999f, 1.0f, LDE_CLIP_PER_ARRAY, P, P, nullptr, P));
    assert(!clip_args_ok(0, nullptr, 0.9f, 0.999f, 1.0f, LDE_CLIP_PER_ARRAY, P, P, nullptr, nullptr));
  }
  std::printf("clipped step host logic under ASan + UBSan: %d workspace plans checked (one slot per scan workgroup, disjoint, inside the workspace, the last one written)\n", plans);
  return 0;
}
