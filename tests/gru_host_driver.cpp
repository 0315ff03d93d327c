// gru_host_driver.cpp — the pure part of the GRU plan (csrc/lde_host.h: pseudo-row count, lanes and rows per lane, flat offsets, the map
// from the staged weight-gradient product to the cell's flat order), compiled with an ordinary host compiler under AddressSanitizer +
// UndefinedBehaviorSanitizer and run as a program by tests/test_gru_host.py, with hostile sizes.
#undef NDEBUG
#include <cassert>
#include <cstdio>
#include <limits>
#include <vector>

#include "../latentdiffeq.jl_amd/csrc/lde_host.h"

using namespace lde_host;

int main() {
  const int IMAX = std::numeric_limits<int>::max(), IMIN = std::numeric_limits<int>::min();
  // rows, lanes, rows per lane
  assert(gru_rows(16) == 64 && gru_rows(1) == 4 && gru_rows(64) == 256);
  for (int h : {0, -1, 65, IMAX, IMIN}) assert(gru_rows(h) == 0);
  assert(gru_lanes(1) == 4 && gru_lanes(3) == 16 && gru_lanes(9) == 64 && gru_lanes(16) == 64 && gru_lanes(17) == 64 && gru_lanes(64) == 64);
  for (int h : {0, -5, 65, IMAX, IMIN}) assert(gru_lanes(h) == 1);
  assert(gru_rows_per_lane(16, 64) == 1 && gru_rows_per_lane(17, 64) == 2 && gru_rows_per_lane(32, 64) == 2 && gru_rows_per_lane(64, 64) == 4);
  assert(gru_rows_per_lane(3, 16) == 1 && gru_rows_per_lane(16, 0) == 0 && gru_rows_per_lane(16, -64) == 0 && gru_rows_per_lane(IMAX, 64) == 0);
  for (int h = 1; h <= GRU_MAX_H; h++) {
    const int Hp = gru_lanes(h);
    assert(Hp >= 1 && Hp <= 64 && (Hp & (Hp - 1)) == 0);
    assert(gru_rows_per_lane(h, Hp) * Hp >= gru_rows(h) && (gru_rows_per_lane(h, Hp) - 1) * Hp < gru_rows(h));
  }
  // flat counts and offsets
  assert(gru_cell_weights(32, 16) == 3 * 16 * 32 + 3 * 16 * 16 + 3 * 16 + 16);
  assert(gru_cell_weights(256, 64) == 3 * 64 * 256 + 3 * 64 * 64 + 3 * 64 + 64);
  assert(gru_cell_weights(0, 16) == -1 && gru_cell_weights(32, 0) == -1 && gru_cell_weights(257, 16) == -1 && gru_cell_weights(32, 65) == -1);
  assert(gru_cell_weights(std::numeric_limits<int64_t>::max(), 16) == -1 && gru_cell_weights(32, std::numeric_limits<int64_t>::min()) == -1);
  {
    const GruFlat f = gru_flat_offsets(5, 7);
    assert(f.wh == 105 && f.b == 105 + 147 && f.s0 == 105 + 147 + 21 && f.end == gru_cell_weights(5, 7));
    const GruFlat g = gru_flat_offsets(-1, 7);
    assert(g.wh == -1 && g.end == -1);
  }
  // the map: one-to-one into the staged result, never onto a structural zero, and it is the pseudo-row layout the kernels load
  const int shapes[][2] = {{1, 1}, {32, 16}, {16, 16}, {5, 7}, {7, 3}, {3, 9}, {3, 10}, {40, 21}, {21, 11}, {40, 22}, {32, 32}, {16, 64}, {256, 64}, {256, 1}, {1, 64}};
  for (const auto& sh : shapes) {
    const int in = sh[0], h = sh[1], K = in + h, P = 4 * h;
    const long long n = gru_staged_count(in, h), m = gru_staged_floats(in, h);
    assert(n == gru_cell_weights(in, h) - h && m == (long long)P * K + P);
    std::vector<unsigned char> hit((size_t)m, 0);
    const GruFlat f = gru_flat_offsets(in, h);
    for (long long e = 0; e < n; e++) {
      const long long j = gru_staged_index(in, h, e);
      assert(j >= 0 && j < m && !hit[(size_t)j]);
      hit[(size_t)j] = 1;
      if (j < (long long)P * K) {
        const long long k = j / P, p = j % P;
        assert(!(p >= 2 * h && p < 3 * h && k >= in));   // n_x has no h columns
        assert(!(p >= 3 * h && k < in));                  // n_h has no x columns
        // flat (row r of Wi / Wh, column k) ↔ pseudo-row p
        if (e < f.wh) assert(k == e / (3 * h) && p == e % (3 * h));
        else { const long long r = (e - f.wh) % (3 * h); assert(e < f.b && k == in + (e - f.wh) / (3 * h) && p == (r < 2 * h ? r : r + h)); }
      } else {
        assert(e >= f.b && j - (long long)P * K == e - f.b && j - (long long)P * K < 3 * h);   // no bias on n_h
      }
    }
    long long used = 0;
    for (unsigned char c : hit) used += c;
    assert(used == n);
    // out of range on either side
    assert(gru_staged_index(in, h, -1) == -1 && gru_staged_index(in, h, n) == -1 && gru_staged_index(in, h, n + h) == -1);
    assert(gru_staged_index(in, h, std::numeric_limits<long long>::max()) == -1 && gru_staged_index(in, h, std::numeric_limits<long long>::min()) == -1);
  }
  // hostile sizes: refused, no overflow
  for (int v : {0, -1, IMIN, IMAX, 257, 65536}) {
    assert(gru_staged_index(v, 16, 0) == -1 || (v >= 1 && v <= 256));
    assert(gru_staged_index(32, v, 0) == -1 || (v >= 1 && v <= 64));
    assert(gru_staged_index(v, v, 0) == -1);
    (void)gru_staged_count(v, v);   // 64-bit arithmetic on 32-bit sizes: defined for every input
    (void)gru_staged_floats(v, v);
  }
  std::printf("gru host plan under ASan + UBSan: rows, lanes, flat offsets and the staged-gradient map checked\n");
  return 0;
}
