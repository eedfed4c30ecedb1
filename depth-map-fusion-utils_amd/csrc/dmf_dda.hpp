// dmf_dda.hpp — the exact integer 3D-DDA of a probe ray and the tiled counter
// layout, shared by the fusion kernels (dmf_fuse.hip), the log-odds ray-cast (dmf_raycast.hip)
// and the segment clearance (dmf_distance.hip): clip and quantise origin -> endpoint (dmf_quant.hpp,
// host-compilable), the int32 walk state, one selection step, the walk in scalars, the per-pixel
// ray of a depth frame, and the exact jump out of an aligned cube of cells (rc_jump: the
// ray-cast's and the view gain's).
#pragma once
#include "dmf_internal.hpp"
#include "dmf_quant.hpp"

namespace dmf {

// (kQ, grid_coord, the endpoint acceptance and the clip / quantisation:
// dmf_quant.hpp, which the CPU self-test compiles too)

__device__ inline void atomic_add_dev(int32_t* p, int32_t v) {
  __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Tiled counter layout: 2x2x4-cell tiles (x, y, z), 16 int32 = one 64-B line, tiles
// x-major over the padded grid; inside a tile ((x&1)*2 + (y&1))*4 + (z&3).
struct Tiles {
  uint32_t ny, nz;  // tiles along y and z
};
__host__ __device__ inline Tiles tiles_of(const int n[3]) {
  return Tiles{(uint32_t)(n[1] + 1) >> 1, (uint32_t)(n[2] + 3) >> 2};
}
__host__ __device__ inline uint32_t tile_base(const Tiles& t, int tx, int ty, int tz) {
  return (((uint32_t)tx * t.ny + (uint32_t)ty) * t.nz + (uint32_t)tz) << 4;
}
__host__ __device__ inline uint32_t tiled_index(const Tiles& t, int x, int y, int z) {
  return tile_base(t, x >> 1, y >> 1, z >> 2) | (uint32_t)(((x & 1) << 3) | ((y & 1) << 2) | (z & 3));
}
inline size_t tiled_cells(const int n[3]) {
  return (size_t)((n[0] + 1) >> 1) * (size_t)((n[1] + 1) >> 1) * (size_t)((n[2] + 3) >> 2) * 16;
}

// Per-ray DDA state after setup (exact integer walk).
//
// The oracle compares next-crossing times T_a = h_a * prod_{b != a} |dq_b| in 64 bits.
// For a pair of moving axes, sign(T_a - T_b) = sign(E_ab) with
// E_ab = h_a |dq_b| - h_b |dq_a| (T_a - T_b divided by the third axis' |dq|), and
// because both next crossings lie within one cell interval of the current time,
// |E_ab| < (2Q + 1) max|dq| <= 2^29 for grids up to 2048 cells per axis: the walk
// runs on three int32 differences.  A step along axis a adds 2Q|dq_b| to E_ab (and
// subtracts 2Q|dq_a| from E_ba).  A pair with a non-moving axis holds a constant that
// never lets that axis win.
struct Ray {
  int c[3];        // current cell
  int st[3];       // step direction per axis (-1, 0, +1)
  int32_t E01, E02, E12;  // crossing-time differences (see above)
  int32_t K[3];    // 2Q |dq_a|
  int left;        // remaining cell updates (misses + final), 0 = inactive
  bool end_inside;
};
constexpr int32_t kNever = 1 << 30;  // |E| of a pair with a non-moving axis

// One DDA selection (earliest crossing; ties x before y before z): s2 = z, s1 = y, else x.
__device__ inline void dda_select(int32_t& E01, int32_t& E02, int32_t& E12, int32_t K0, int32_t K1, int32_t K2,
                                  bool& s0, bool& s1, bool& s2) {
  const bool b10 = E01 > 0;             // T1 < T0
  s2 = (b10 ? E12 : E02) > 0;            // T2 < min(T0, T1)
  s1 = !s2 && b10;
  s0 = !s2 && !b10;
  E01 += s0 ? K1 : (s1 ? -K0 : 0);
  E02 += s0 ? K2 : (s2 ? -K0 : 0);
  E12 += s1 ? K2 : (s2 ? -K1 : 0);
}

// A Ray's walk in scalars: a lane keeps it in registers (members, never arrays indexed by an axis:
// a dynamically indexed private array once made phase F 15x slower).  left counts the cells still
// to visit, the current one included; the caller owns its decrement.
struct Walk {
  int c0, c1, c2, st0, st1, st2;
  int32_t E01, E02, E12, K0, K1, K2;
  int left;
  __device__ explicit Walk(const Ray& R)
      : c0(R.c[0]), c1(R.c[1]), c2(R.c[2]), st0(R.st[0]), st1(R.st[1]), st2(R.st[2]), E01(R.E01), E02(R.E02),
        E12(R.E12), K0(R.K[0]), K1(R.K[1]), K2(R.K[2]), left(R.left) {}
  __device__ void step() {  // to the next cell of the sequence
    bool s0, s1, s2;
    dda_select(E01, E02, E12, K0, K1, K2, s0, s1, s2);
    c0 += s0 ? st0 : 0;
    c1 += s1 ? st1 : 0;
    c2 += s2 ? st2 : 0;
  }
};

// Clip/quantise (dmf_quant.hpp), then set up the walk state (oracle.cpp dda_ray lines 781-806).
// end_inside = endpoint_inside(g, E).
__device__ inline bool dda_setup(const Geom& g, const float O[3], const float E[3], bool end_inside, Ray& R) {
  double go[3], ge[3];
  grid_origin(g, O, go);
  grid_origin(g, E, ge);
  int32_t qs32[3], qe32[3];
  if (!dda_quantize_ge(g, go, ge, end_inside, qs32, qe32)) return false;
  const int64_t qs[3] = {qs32[0], qs32[1], qs32[2]}, qe[3] = {qe32[0], qe32[1], qe32[2]};
  int64_t cs[3], ce[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    cs[a] = qs[a] / kQ;  // qs, qe >= 0 and clamped into their cells
    ce[a] = qe[a] / kQ;
  }
  int64_t adq[3], h[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const int64_t dq = qe[a] - qs[a];
    adq[a] = dq < 0 ? -dq : dq;
    R.st[a] = ce[a] > cs[a] ? 1 : (ce[a] < cs[a] ? -1 : 0);
    // next crossing numerator in half fixed-point units (oracle.cpp dda_ray)
    h[a] = R.st[a] > 0 ? 2 * ((cs[a] + 1) * kQ - qs[a]) : 2 * (qs[a] - cs[a] * kQ) + 1;
    R.K[a] = (int32_t)(2 * kQ * adq[a]);
  }
  auto pair = [&](int a, int b) -> int32_t {
    if (R.st[a] && R.st[b]) return (int32_t)(h[a] * adq[b] - h[b] * adq[a]);
    return R.st[a] ? -kNever : (R.st[b] ? kNever : 0);
  };
  R.E01 = pair(0, 1);
  R.E02 = pair(0, 2);
  R.E12 = pair(1, 2);
  const int nsteps = (int)((ce[0] > cs[0] ? ce[0] - cs[0] : cs[0] - ce[0]) + (ce[1] > cs[1] ? ce[1] - cs[1] : cs[1] - ce[1]) +
                           (ce[2] > cs[2] ? ce[2] - cs[2] : cs[2] - ce[2]));
  R.c[0] = (int)cs[0];
  R.c[1] = (int)cs[1];
  R.c[2] = (int)cs[2];
  R.left = nsteps + 1;
  R.end_inside = end_inside;
  return true;
}

// Per-pixel ray: back-projection (Camera.hpp:24-45) + binning of the endpoint
// (Volume.hpp:150-156, 199-228) + DDA setup.  Returns the update count (0 = no ray).
__device__ inline int pixel_ray(const Geom& g, const CamP& cam, const uint16_t* __restrict__ depth,
                                const PoseX* __restrict__ poses, int p, int r, int c, int dmin, int dmax, Ray& R,
                                bool& valid) {
  R.left = 0;
  valid = false;
  if (r >= cam.H || c >= cam.W) return 0;
  const int d = depth[((int64_t)p * cam.H + r) * cam.W + c];
  if (!(d >= dmin && d < dmax)) return 0;
  valid = true;
  const PoseX& T = poses[p];
  float pc[3], E[3];
  project(cam, r, c, d, pc);
  xform(T.f, pc[0], pc[1], pc[2], E);
  const bool inside = endpoint_inside(g, E);
  const float O[3] = {T.f[3], T.f[7], T.f[11]};
  if (!dda_setup(g, O, E, inside, R)) { R.left = 0; return 0; }
  return R.left;
}

// The brick path's ray record: pixel_ray up to the quantised endpoints, with the pose's grid
// origin already computed (go = grid_origin of poses[p]'s translation; d < 0: outside the frame).
__device__ inline bool pixel_quant_go(const Geom& g, const CamP& cam, int d, const float Tf[12], const double go[3],
                                      int r, int c, int dmin, int dmax, int32_t qs[3], int32_t qe[3], bool& inside,
                                      bool& valid) {
  valid = false;
  inside = false;
  if (d < 0 || !(d >= dmin && d < dmax)) return false;
  valid = true;
  float pc[3], E[3];
  project(cam, r, c, d, pc);
  xform(Tf, pc[0], pc[1], pc[2], E);
  return dda_quantize_go(g, go, E, &inside, qs, qe);
}

__device__ inline int pixel_depth(const CamP& cam, const uint16_t* __restrict__ depth, int p, int r, int c) {
  return (r >= cam.H || c >= cam.W) ? -1 : (int)depth[((int64_t)p * cam.H + r) * cam.W + c];
}

// floor(x / k) for 0 <= x < 2^35, 1 <= k < 2^29 with quotient < 2^12: a float estimate (within 1 of
// the quotient: three roundings of 2^-24 relative each) and exact integer correction.
__device__ inline int32_t rc_div(int64_t x, int32_t k) {
  int32_t q = (int32_t)((float)x * __builtin_amdgcn_rcpf((float)k));
  int64_t r = x - (int64_t)q * k;
  if (r < 0) { --q; r += k; }
  if (r < 0) { --q; r += k; }
  if (r >= k) { ++q; r -= k; }
  if (r >= k) { ++q; }
  return q;
}

// Exact jump out of the aligned cube of (m + 1)^3 cells (m = 7 or 31) that holds the current cell:
// the walk state after the crossing that leaves the cube, and the number of steps that takes.
// In the cube, axis a can still make r_a crossings; its (r_a + 1)-th leaves.  The earliest of the
// three leaving events in the walk's own order (crossing time, ties x < y < z) is found as
// dda_select finds the next crossing, from F_ab = E_ab + r_a K_b - r_b K_a (the crossing-time
// difference of the two leaving events); every crossing of another axis b that
// precedes that event (a*, r*) in the same order is taken with it: #{k >= 0 : k K_a* < X} for
// b > a*, <= X for b < a*, X = (h_a* + 2Q r*) |dq_b| - h_b |dq_a*| = +-E + r* K_b.  A step along a
// adds K_b to E_ab and takes K_a from E_ba, so n_a steps per axis move E_ab by n_a K_b - n_b K_a.
// A non-moving axis has K = 0, r = 0 and |E| = kNever against a moving one: it neither leaves
// nor steps.  Returns the steps; more than the ray has left means the ray ends in the cube.
__device__ inline int rc_jump(int m, Walk& W) {
  const int r0 = W.st0 > 0 ? m - (W.c0 & m) : (W.st0 < 0 ? (W.c0 & m) : 0);
  const int r1 = W.st1 > 0 ? m - (W.c1 & m) : (W.st1 < 0 ? (W.c1 & m) : 0);
  const int r2 = W.st2 > 0 ? m - (W.c2 & m) : (W.st2 < 0 ? (W.c2 & m) : 0);
  const int64_t F01 = (int64_t)W.E01 + (int64_t)r0 * W.K1 - (int64_t)r1 * W.K0;
  const int64_t F02 = (int64_t)W.E02 + (int64_t)r0 * W.K2 - (int64_t)r2 * W.K0;
  const int64_t F12 = (int64_t)W.E12 + (int64_t)r1 * W.K2 - (int64_t)r2 * W.K1;
  const bool b10 = F01 > 0;
  const bool s2 = (b10 ? F12 : F02) > 0, s1 = !s2 && b10;
  // crossings of axis b before the leaving event of a*: d = h_a* |dq_b| - h_b |dq_a*|
  auto before = [](int64_t d, int rs, int32_t kb, int32_t ka, bool b_after) -> int {
    const int64_t x = d + (int64_t)rs * kb;
    if (x < 0 || ka == 0) return 0;
    const int32_t q = rc_div(x, ka);
    return b_after ? (int)(q + ((int64_t)q * ka < x ? 1 : 0)) : (int)q + 1;
  };
  int n0, n1, n2;
  if (s2) {
    n2 = r2 + 1;
    n0 = before(-(int64_t)W.E02, r2, W.K0, W.K2, false);
    n1 = before(-(int64_t)W.E12, r2, W.K1, W.K2, false);
  } else if (s1) {
    n1 = r1 + 1;
    n0 = before(-(int64_t)W.E01, r1, W.K0, W.K1, false);
    n2 = before((int64_t)W.E12, r1, W.K2, W.K1, true);
  } else {
    n0 = r0 + 1;
    n1 = before((int64_t)W.E01, r0, W.K1, W.K0, true);
    n2 = before((int64_t)W.E02, r0, W.K2, W.K0, true);
  }
  W.c0 += W.st0 * n0;
  W.c1 += W.st1 * n1;
  W.c2 += W.st2 * n2;
  W.E01 = (int32_t)((uint32_t)W.E01 + (uint32_t)n0 * (uint32_t)W.K1 - (uint32_t)n1 * (uint32_t)W.K0);
  W.E02 = (int32_t)((uint32_t)W.E02 + (uint32_t)n0 * (uint32_t)W.K2 - (uint32_t)n2 * (uint32_t)W.K0);
  W.E12 = (int32_t)((uint32_t)W.E12 + (uint32_t)n1 * (uint32_t)W.K2 - (uint32_t)n2 * (uint32_t)W.K1);
  return n0 + n1 + n2;
}

}  // namespace dmf
