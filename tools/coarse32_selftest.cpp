// CPU self-test of pass A's coarse walk on scaled 32-bit state (csrc/dmf_brick.hpp Coarse32,
// coarse_walk32) against the 64-bit coarse walk (Coarse / coarse_next), over whole rays:
//   1. coarse_init32's gamma is (E - 1) >> 14 of coarse_init's E for every pair of two moving
//      axes, and stays so after every step (so every step's axis from coarse_next32 equals
//      coarse_next's); a pair with a non-moving axis keeps its sign;
//   2. |gamma| stays within the header's bound max(|dq_a|, |dq_b|) + 1 (coarse_gamma_ok);
//   3. coarse_walk32's brick index, moved by the per-axis steps st * nb1 * nb2, st * nb2, st,
//      equals the index of the brick coordinates at every brick, and the coordinates stay
//      inside the grid;
//   4. the path it returns (two 32-bit words, path_word_put) equals path_put's over the same
//      axes, and path_axis2 reads from its words what path_axis reads from the uint64.
// Rays: random ones on grids up to 1024 cells per axis; end points on exact multiples of
// 256 * 32 (two- and three-way ties at brick corners); axis-aligned and planar rays (the
// sentinels), also with sub-cell motion along the non-moving axes; the largest |dq| on a
// 1024-cell axis; starts on a brick face; long diagonals (more than 32 boundaries).  The run
// asserts that every sign octant, ties and rays of more than kPathSteps boundaries occurred.
// run: <exe> [random rays] [seed]
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "dmf_brick.hpp"

using namespace dmf::brick;

static long long g_fail = 0, g_rays = 0, g_steps = 0, g_long = 0, g_ties = 0;
static int32_t g_maxg = 0;
static bool g_signs[27];

static void fail(const char* what, const int32_t qs[3], const int32_t qe[3], int t) {
  if (++g_fail <= 20)
    std::printf("FAIL %s: qs %d %d %d  qe %d %d %d  step %d\n", what, qs[0], qs[1], qs[2], qe[0], qe[1], qe[2], t);
}

static int64_t gamma_of(int64_t E) { return (E - 1) >> kCoarseShift; }

// one ray on a grid of ng cells per axis (its end points inside the grid)
static void check_ray(const int32_t qs[3], const int32_t qe[3], const int32_t ng[3]) {
  QRay r;
  qray_from(qs, qe, true, r);
  ++g_rays;
  g_signs[(r.st[0] + 1) * 9 + (r.st[1] + 1) * 3 + (r.st[2] + 1)] = true;
  const int32_t nb[3] = {(ng[0] + kB - 1) / kB, (ng[1] + kB - 1) / kB, (ng[2] + kB - 1) / kB};
  Coarse c64;
  Coarse32 c32;
  coarse_init(r, c64);
  coarse_init32(r, c32);
  if (c32.total != c64.total) fail("total", qs, qe, -1);
  int32_t bc[3] = {r.cs[0] >> kLog, r.cs[1] >> kLog, r.cs[2] >> kLog};
  auto index = [&]() { return (bc[0] * nb[1] + bc[1]) * nb[2] + bc[2]; };
  std::vector<int32_t> want;
  want.push_back(index());
  uint64_t path = 0;
  auto state_ok = [&](int t) {
    // exact where both axes move; the sign (all that is used) where one does not
    auto one = [&](int a, int b, int64_t E, int32_t g) {
      if (r.st[a] && r.st[b]) {
        if (gamma_of(E) != (int64_t)g) fail("gamma", qs, qe, t);
        const int32_t ag = g < 0 ? -g : g;
        if (ag > g_maxg) g_maxg = ag;
        if (E == 0) ++g_ties;
      } else if ((E > 0) != (g >= 0)) {
        fail("sentinel sign", qs, qe, t);
      }
    };
    one(0, 1, c64.E01, c32.g01);
    one(0, 2, c64.E02, c32.g02);
    one(1, 2, c64.E12, c32.g12);
    if (!coarse_gamma_ok(r, c32)) fail("gamma bound", qs, qe, t);
  };
  state_ok(-1);
  for (int t = 0; t < c64.total; ++t) {
    const int a = coarse_next(c64), a32 = coarse_next32(c32);
    if (a != a32) {
      fail("axis", qs, qe, t);
      return;
    }
    state_ok(t);
    bc[a] += r.st[a];
    if (bc[a] < 0 || bc[a] >= nb[a]) fail("brick outside the grid", qs, qe, t);
    want.push_back(index());
    path = path_put(path, t, a);
  }
  g_steps += c64.total;
  if (c64.total > kPathSteps) ++g_long;
  // pass A's walk itself
  const int32_t b0 = ((r.cs[0] >> kLog) * nb[1] + (r.cs[1] >> kLog)) * nb[2] + (r.cs[2] >> kLog);
  const int32_t D0 = r.st[0] * nb[1] * nb[2], D1 = r.st[1] * nb[2], D2 = r.st[2];
  std::vector<int32_t> got;
  const uint64_t p32 = coarse_walk32(r, b0, D0, D1, D2, [&](int32_t b) { got.push_back(b); });
  if (got != want) fail("brick index", qs, qe, -1);
  if (p32 != path) fail("path", qs, qe, -1);
  const uint32_t lo = (uint32_t)p32, hi = (uint32_t)(p32 >> 32);
  for (int t = 0; t < kPathSteps && t < c64.total; ++t)
    if (path_axis2(t < kPathSteps / 2 ? lo : hi, t) != path_axis(path, t)) fail("path_axis2", qs, qe, t);
}

int main(int argc, char** argv) {
  const long long nrand = argc > 1 ? std::atoll(argv[1]) : 3000000;
  const unsigned seed = argc > 2 ? (unsigned)std::atoi(argv[2]) : 1;
  std::mt19937_64 rng(seed);
  auto uni = [&](int32_t lo, int32_t hi) { return (int32_t)(lo + (int64_t)(rng() % (uint64_t)(hi - lo + 1))); };
  const int32_t Q = (int32_t)kQ, BQ = kB * Q;  // 256 * 32: a brick edge in fixed-point units

  // random rays on random grids (every third one 1024^3, where |dq| and the walks are largest)
  for (long long i = 0; i < nrand; ++i) {
    int32_t ng[3], qs[3], qe[3];
    for (int a = 0; a < 3; ++a) {
      ng[a] = i % 3 == 0 ? 1024 : uni(1, 1024);
      qs[a] = uni(0, ng[a] * Q - 1);
      qe[a] = uni(0, ng[a] * Q - 1);
    }
    check_ray(qs, qe, ng);
  }
  const long long n_random = g_rays;

  // end points on brick corners (multiples of 256 * 32): two- and three-way ties at every
  // corner the ray passes; also from cell centres and from the fixed-point unit before a corner
  for (int i = 0; i < 60000; ++i) {
    const int32_t ng[3] = {1024, 1024, 1024};
    int32_t qs[3], qe[3];
    const int kind = i % 4;
    const int32_t len = uni(1, 31);
    for (int a = 0; a < 3; ++a) {
      const int32_t c0 = uni(0, 31), dir = uni(-1, 1);
      int32_t c1 = c0 + dir * (kind == 3 ? uni(0, 31) : len);  // kind 3: unequal spans (two-way ties)
      c1 = c1 < 0 ? 0 : (c1 > 31 ? 31 : c1);
      qs[a] = c0 * BQ + (kind == 1 ? Q / 2 : 0) - (kind == 2 && c0 > 0 ? 1 : 0);
      qe[a] = c1 * BQ + (kind == 1 ? Q / 2 : 0);
    }
    check_ray(qs, qe, ng);
  }

  // axis-aligned and planar rays: one or two axes do not move (exactly, or inside one cell)
  for (int i = 0; i < 60000; ++i) {
    const int32_t ng[3] = {uni(1, 1024), uni(1, 1024), uni(1, 1024)};
    int32_t qs[3], qe[3];
    const int still = 1 + i % 6;  // bit a: axis a does not move (1..6: one or two axes)
    for (int a = 0; a < 3; ++a) {
      qs[a] = uni(0, ng[a] * Q - 1);
      qe[a] = uni(0, ng[a] * Q - 1);
      if (still >> a & 1) qe[a] = (i / 6) % 2 ? qs[a] : (qs[a] / Q) * Q + uni(0, Q - 1);
    }
    check_ray(qs, qe, ng);
  }

  // the largest |dq| on a 1024-cell axis, every sign octant, the other axes random or extreme too
  for (int i = 0; i < 40000; ++i) {
    const int32_t ng[3] = {1024, 1024, 1024};
    const int32_t top = 1024 * Q - 1;
    int32_t qs[3], qe[3];
    for (int a = 0; a < 3; ++a) {
      const bool ext = a == i % 3 || (i / 3) % 4 == 3, down = (i / 12) >> a & 1;
      const int32_t lo = ext ? 0 : uni(0, top), hi = ext ? top : uni(0, top);
      qs[a] = down ? (lo > hi ? lo : hi) : (lo < hi ? lo : hi);
      qe[a] = down ? (lo < hi ? lo : hi) : (lo > hi ? lo : hi);
    }
    check_ray(qs, qe, ng);
  }

  // starts on a brick face: the first or the last fixed-point unit of a brick along one axis
  for (int i = 0; i < 60000; ++i) {
    const int32_t ng[3] = {uni(33, 1024), uni(33, 1024), uni(33, 1024)};
    int32_t qs[3], qe[3];
    for (int a = 0; a < 3; ++a) {
      qs[a] = uni(0, ng[a] * Q - 1);
      qe[a] = uni(0, ng[a] * Q - 1);
    }
    const int a = i % 3;
    const int32_t face = uni(1, (ng[a] - 1) / kB) * BQ;  // a brick boundary inside the grid
    qs[a] = face - ((i / 3) % 2);
    check_ray(qs, qe, ng);
  }

  // long diagonals of a 1024^3 grid: up to 93 boundaries, far past the recorded path
  for (int i = 0; i < 40000; ++i) {
    const int32_t ng[3] = {1024, 1024, 1024};
    int32_t qs[3], qe[3];
    for (int a = 0; a < 3; ++a) {
      const bool down = i >> a & 1;
      const int32_t lo = uni(0, 64 * Q), hi = 1024 * Q - 1 - uni(0, 64 * Q);
      qs[a] = down ? hi : lo;
      qe[a] = down ? lo : hi;
    }
    check_ray(qs, qe, ng);
  }

  // the run must have met what it is meant to exercise
  int octs = 0;
  for (int s = 0; s < 27; ++s) octs += g_signs[s] ? 1 : 0;
  if (octs != 27) { ++g_fail; std::printf("FAIL coverage: %d of 27 sign patterns\n", octs); }
  if (g_long == 0) { ++g_fail; std::printf("FAIL coverage: no ray of more than %d boundaries\n", kPathSteps); }
  if (g_ties == 0) { ++g_fail; std::printf("FAIL coverage: no tie (E = 0)\n"); }
  if (g_maxg > (1 << 18) + 1) { ++g_fail; std::printf("FAIL |gamma| %d over 2^18 + 1\n", g_maxg); }
  std::printf("coarse32 self-test: %lld rays (%lld random), %lld boundary steps, %lld rays over %d boundaries, "
              "%lld tied states, max |gamma| %d (bound 2^18 + 1 = %d), %d/27 sign patterns: %lld failures\n",
              g_rays, n_random, g_steps, g_long, kPathSteps, g_ties, g_maxg, (1 << 18) + 1, octs, g_fail);
  return g_fail ? 1 : 0;
}
