// guard_host_driver.cpp — what csrc/lde_host.h decides about the parameter update's launches (opt_next_launch: which arrays of the caller's
// t[] travel in which launch, each array's first workgroup, which launch is the step's last), for the update's slice (OPT_PER_WG) and for
// the gradient scan of the guarded step (GUARD_PER_WG) — compiled with an ordinary host compiler under AddressSanitizer +
// UndefinedBehaviorSanitizer and run as a program by tests/test_guard_host.py. No pointer of a table is ever dereferenced here.
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

// The plan as csrc/lde_optim.hip's launch loop computed it before the packing moved here, written out by hand: per launch the indices of
// its arrays, blk0[] and the `bump` flag.
struct OldLaunch {
  std::vector<int> idx, blk0;
  bool bump;
};
static bool old_plan(int n, const lde_adam_tensor* t, std::vector<OldLaunch>* out) {   // false: LDE_ERR_INVALID_ARG
  const int PER = 2048, MAXT = 48;
  for (int first = 0; first < n;) {
    OldLaunch L;
    int blk = 0, tn = 0;
    while (first < n && tn < MAXT) {
      if (t[first].n > 0) {
        const int64_t nb = (t[first].n + PER - 1) / PER;
        if (nb > 0x3fffffff - blk) break;
        L.idx.push_back(first);
        L.blk0.push_back(blk);
        blk += (int)nb;
        tn++;
      }
      first++;
    }
    if (tn == 0) return !(first < n);
    L.blk0.push_back(blk);
    bool more = false;
    for (int j = first; j < n; j++) more = more || t[j].n > 0;
    L.bump = !more;
    out->push_back(L);
  }
  return true;
}

static std::vector<OptLaunch> plan(int n, const lde_adam_tensor* t, int per, bool* refused) {
  std::vector<OptLaunch> v;
  *refused = false;
  for (int first = 0; first < n;) {
    const OptLaunch L = opt_next_launch(n, t, first, per);
    assert(L.next >= first && L.next <= n && L.n >= 0 && L.n <= OPT_MAXT);
    assert(L.n > 0 || L.next == first || L.too_large || L.next == n);
    first = L.next;
    if (L.n == 0) {
      *refused = L.too_large;
      break;
    }
    assert(!L.too_large);
    v.push_back(L);
  }
  return v;
}

// every element of every array in exactly one workgroup's range, found the way the kernels find it; ranges of an array contiguous and in
// workgroup order; exactly one launch marked last — the final one
static void check_plan(int n, const lde_adam_tensor* t, int per, bool count_elements) {
  bool refused = false;
  const std::vector<OptLaunch> v = plan(n, t, per, &refused);
  assert(!refused);
  std::vector<int> seen(n > 0 ? n : 1, 0);
  int nlast = 0, prev = -1;
  bool any = false;
  for (int i = 0; i < n; i++) any = any || t[i].n > 0;
  assert(any == !v.empty());
  for (size_t l = 0; l < v.size(); l++) {
    const OptLaunch& L = v[l];
    nlast += L.last ? 1 : 0;
    assert(L.last == (l + 1 == v.size()));
    assert(L.blk0[0] == 0 && L.blk0[L.n] > 0 && L.blk0[L.n] <= OPT_MAX_BLOCKS);
    for (int i = 0; i < L.n; i++) {
      const int a = L.idx[i];
      assert(a > prev && a < n && t[a].n > 0);   // the caller's order, every non-empty array once
      for (int k = prev + 1; k < a; k++) assert(t[k].n == 0);
      prev = a;
      seen[a]++;
      const int64_t wgs = (int64_t)L.blk0[i + 1] - L.blk0[i];
      assert(wgs >= 1 && (wgs - 1) * per < t[a].n && wgs * per >= t[a].n);   // contiguous slices cover [0, n) and none is empty
    }
    if (!count_elements) continue;
    std::vector<std::vector<unsigned char>> cover(L.n);
    for (int i = 0; i < L.n; i++) cover[i].assign((size_t)t[L.idx[i]].n, 0);
    int64_t expect_lo = 0;
    int cur = -1;
    for (int b = 0; b < L.blk0[L.n]; b++) {
      int i = 0;
      while (i + 1 < L.n && b >= L.blk0[i + 1]) i++;   // the kernels' search
      const int64_t nn = t[L.idx[i]].n;
      const int64_t lo = (int64_t)(b - L.blk0[i]) * per;
      const int64_t hi = lo + per < nn ? lo + per : nn;
      if (i != cur) {
        assert(i == cur + 1 && (cur < 0 || expect_lo == t[L.idx[cur]].n));
        cur = i;
        expect_lo = 0;
      }
      assert(lo == expect_lo && hi > lo && hi <= nn);
      expect_lo = hi;
      for (int64_t e = lo; e < hi; e++) cover[i][(size_t)e]++;
    }
    assert(cur == L.n - 1 && expect_lo == t[L.idx[cur]].n);
    for (int i = 0; i < L.n; i++)
      for (unsigned char c : cover[i]) assert(c == 1);
  }
  for (int i = 0; i < n; i++) assert(seen[i] == (t[i].n > 0 ? 1 : 0));
  assert(nlast == (any ? 1 : 0));
}

// the update's plan is the plan of the code it was moved from
static void check_against_old(int n, const lde_adam_tensor* t) {
  std::vector<OldLaunch> o;
  const bool ok = old_plan(n, t, &o);
  bool refused = false;
  const std::vector<OptLaunch> v = plan(n, t, OPT_PER_WG, &refused);
  assert(ok == !refused);
  assert(v.size() == o.size());   // (a refused call too: the launches in front of the refusal, which the unguarded call has issued by then)
  for (size_t l = 0; l < v.size(); l++) {
    assert((size_t)v[l].n == o[l].idx.size());
    for (int i = 0; i < v[l].n; i++) assert(v[l].idx[i] == o[l].idx[i] && v[l].blk0[i] == o[l].blk0[i]);
    assert(v[l].blk0[v[l].n] == o[l].blk0[v[l].n] && v[l].last == o[l].bump);
  }
}

static std::vector<lde_adam_tensor> arrays(const std::vector<int64_t>& sizes) {
  std::vector<lde_adam_tensor> t(sizes.size());
  for (size_t i = 0; i < sizes.size(); i++) {
    t[i] = lde_adam_tensor{};
    t[i].n = sizes[i];
  }
  return t;
}

int main() {
  static_assert(OPT_WG == 256 && OPT_PER_WG == 2048 && OPT_MAXT == 48 && OPT_MAX_BLOCKS == 0x3fffffff, "the update's constants are what they were");
  static_assert(GUARD_PER_WG % (4 * OPT_WG) == 0 && GUARD_PER_WG > OPT_PER_WG, "the scan's slice: whole rounds of 16-byte loads, larger than the update's");
  const int64_t U = OPT_PER_WG, S = GUARD_PER_WG;
  const int64_t around[] = {1, 2, 3, 4, 5, U - 1, U, U + 1, 2 * U - 1, 2 * U, 2 * U + 3, S - 1, S, S + 1, 2 * S - 1, 2 * S, 2 * S + 3, 3 * S + U + 1};
  const int NA = (int)(sizeof(around) / sizeof(around[0]));
  int plans = 0;
  // 1. 0, 1, 48, 49 and 97 arrays, sizes around both slices, with and without empty arrays in between
  for (int count : {0, 1, 2, 47, 48, 49, 96, 97}) {
    for (int empties = 0; empties < 3; empties++) {
      for (int shift = 0; shift < 4; shift++) {
        std::vector<int64_t> sizes;
        for (int i = 0; i < count; i++) {
          if (empties == 1 && i % 3 == 1) sizes.push_back(0);
          if (empties == 2) { sizes.push_back(0); sizes.push_back(0); }
          sizes.push_back(around[(i * 5 + shift * 7) % NA]);
        }
        if (empties) sizes.push_back(0);
        std::vector<lde_adam_tensor> t = arrays(sizes);
        for (int per : {OPT_PER_WG, GUARD_PER_WG}) {
          check_plan((int)t.size(), t.data(), per, true);
          plans++;
        }
        check_against_old((int)t.size(), t.data());
      }
    }
  }
  // 48 non-empty arrays fill one table exactly; the 49th opens a second launch — and array 48 is its first
  {
    std::vector<lde_adam_tensor> t = arrays(std::vector<int64_t>(50, 7));
    for (int i = 0; i < 50; i++) t[i].n = i + 1;
    for (int per : {OPT_PER_WG, GUARD_PER_WG}) {
      bool refused;
      const std::vector<OptLaunch> v = plan(50, t.data(), per, &refused);
      assert(v.size() == 2 && v[0].n == 48 && v[1].n == 2 && v[1].idx[0] == 48 && v[1].idx[1] == 49 && !v[0].last && v[1].last);
      assert(v[0].blk0[48] == 48 && v[1].blk0[2] == 2);
    }
    t.resize(48);
    bool refused;
    assert(plan(48, t.data(), OPT_PER_WG, &refused).size() == 1);
  }
  // only empty arrays, a NULL table of none: nothing to launch, nothing refused
  {
    std::vector<lde_adam_tensor> t = arrays({0, 0, 0});
    const OptLaunch L = opt_next_launch(3, t.data(), 0, OPT_PER_WG);
    assert(L.n == 0 && L.next == 3 && L.last && !L.too_large && L.blk0[0] == 0);
    const OptLaunch Z = opt_next_launch(0, nullptr, 0, GUARD_PER_WG);
    assert(Z.n == 0 && Z.next == 0 && Z.last && !Z.too_large);
  }
  // 2. the workgroup limit of a launch: arrays that do not fit beside each other take a launch each; one that fits none is refused by the
  //    update's slice — as before — and not by the scan's
  {
    const int64_t big = (int64_t)0x20000000 * U;   // 2²⁹ workgroups of the update
    std::vector<lde_adam_tensor> t = arrays({big, 5, big, 0, big - U, U + 1, 1});
    check_plan((int)t.size(), t.data(), OPT_PER_WG, false);
    check_plan((int)t.size(), t.data(), GUARD_PER_WG, false);
    check_against_old((int)t.size(), t.data());
    bool refused;
    assert(plan((int)t.size(), t.data(), OPT_PER_WG, &refused).size() == 3 && plan((int)t.size(), t.data(), GUARD_PER_WG, &refused).size() == 1);
    const int64_t most = (int64_t)OPT_MAX_BLOCKS * U;
    for (int64_t n : {most - 1, most, most + 1, 2 * most, std::numeric_limits<int64_t>::max()}) {
      std::vector<lde_adam_tensor> w = arrays({3, n, 4});
      const std::vector<OptLaunch> v = plan(3, w.data(), OPT_PER_WG, &refused);
      assert(refused == (n > most));
      if (n <= most + 1 && n < std::numeric_limits<int64_t>::max() - U) check_against_old(3, w.data());   // (the old sum n + 2047 must not overflow)
      if (!refused) {   // a launch of its own for the array that fills one: 3 | n | 4
        check_plan(3, w.data(), OPT_PER_WG, false);
        assert(v.size() == 3 && v[0].n == 1 && v[1].n == 1 && v[1].blk0[1] == OPT_MAX_BLOCKS && v[2].idx[0] == 2);
      } else {
        assert(v.size() == 1 && v[0].n == 1 && !v[0].last);
      }
      plan(3, w.data(), GUARD_PER_WG, &refused);
      assert(refused == (n > (int64_t)OPT_MAX_BLOCKS * S));   // the scan's slice never refuses what the update's takes
    }
  }
  // 3. any table: the invariants hold and the update's plan is the old one
  for (int it = 0; it < 3000; it++) {
    const int n = (int)(rnd() % 120);
    std::vector<int64_t> sizes(n);
    for (int i = 0; i < n; i++) {
      const uint64_t r = rnd() % 10;
      sizes[i] = r < 2 ? 0 : r < 6 ? (int64_t)(rnd() % 5000) : r < 9 ? around[rnd() % NA] : (int64_t)(rnd() % (3 * S));
    }
    std::vector<lde_adam_tensor> t = arrays(sizes);
    check_plan(n, t.data(), OPT_PER_WG, it < 40);
    check_plan(n, t.data(), GUARD_PER_WG, it < 40);
    check_against_old(n, t.data());
    plans += 2;
  }
  std::printf("guarded step host logic under ASan + UBSan: %d launch plans checked (coverage, contiguity, one last launch, the update's plan unchanged)\n", plans);
  return 0;
}
