// dmf_quant.hpp — clip and quantisation of a probe ray: the grid coordinate of
// a world coordinate, the endpoint's acceptance from it, and the clipped endpoints in 1/256 cell.
// Shared by every kernel that sets up the exact DDA (dmf_dda.hpp).  No HIP dependency: the CPU
// self-test tools/quant_selftest.cpp compiles this same code with g++ and checks it, field for
// field, against an operation-for-operation copy of the code it replaced.
#pragma once
#include <cmath>
#include <cstdint>

#include "dmf_geom.hpp"

namespace dmf {

constexpr int64_t kQ = 256;  // fixed-point sub-cell resolution (1/256 cell)

__host__ __device__ inline int32_t imin32(int32_t a, int32_t b) { return a < b ? a : b; }
__host__ __device__ inline int32_t imax32(int32_t a, int32_t b) { return a > b ? a : b; }

// (int32_t) x, truncated, saturated to the int32 range, 0 for a NaN: what v_cvt_i32_f64 does, in
// that one instruction (C++'s conversion is undefined out of range, and the compiler's saturating
// conversion wraps the instruction in the compares and selects that restate what it does anyway).
__host__ __device__ inline int32_t trunc_sat32(double x) {
#if defined(__HIP_DEVICE_COMPILE__)
  int32_t r;
  asm("v_cvt_i32_f64 %0, %1" : "=v"(r) : "v"(x));
  return r;
#else
  if (!(x == x)) return 0;
  if (x <= -2147483648.0) return INT32_MIN;
  if (x >= 2147483647.0) return INT32_MAX;
  return (int32_t)x;
#endif
}

// Kept from being speculated: the arm of a branch that holds it stays a branch (a wave whose lanes
// all take the other arm skips it) instead of being computed by every lane and selected.
__host__ __device__ inline void keep_branch() {
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("");
#endif
}

// (x - min) / delta in double (oracle.cpp dda_ray); a power-of-two delta divides exactly
// as a multiplication by its (exact) reciprocal, as in bin_axis
__host__ __device__ inline double grid_coord(const Geom& g, int a, float x) {
  const double t = (double)x - g.mn[a];
  return g.pow2 ? t * g.inv[a] : t / g.dl[a];
}

// Grid coordinates of a point (the ray origin: one per pose, callers hoist it).
__host__ __device__ inline void grid_origin(const Geom& g, const float O[3], double go[3]) {
#pragma unroll
  for (int a = 0; a < 3; ++a) go[a] = grid_coord(g, a, O[a]);
}

// The acceptance of integratePointCloud(cloud, normals) (Volume.hpp:199-228):
// validPoints(E) && validCoords(getVoxel(E)), from ge = the grid coordinates of E.  validPoints as
// float compares (vlo / vhi, dmf_geom.hpp; a NaN endpoint, from a non-finite pose, is outside: the
// reference's getVoxel gives INT_MIN for it, which validCoords rejects).  getVoxel's bin is
// floor(ge) (bin_axis is grid_coord's expression), and 0 <= floor(ge) < n <=> 0 <= ge < n for an
// integer n (floor(-0.0) = -0.0 bins to 0, and -0.0 >= 0), so no floor is taken.
__host__ __device__ inline bool endpoint_inside_ge(const Geom& g, const float E[3], const double ge[3]) {
  const bool in = (E[0] >= g.vlo[0]) & (E[0] <= g.vhi[0]) & (E[1] >= g.vlo[1]) & (E[1] <= g.vhi[1]) &
                  (E[2] >= g.vlo[2]) & (E[2] <= g.vhi[2]);
  return in & (ge[0] >= 0.0) & (ge[0] < (double)g.n[0]) & (ge[1] >= 0.0) & (ge[1] < (double)g.n[1]) &
         (ge[2] >= 0.0) & (ge[2] < (double)g.n[2]);
}
__host__ __device__ inline bool endpoint_inside(const Geom& g, const float E[3]) {
  double ge[3];
  grid_origin(g, E, ge);
  return endpoint_inside_ge(g, E, ge);
}

// One quantised coordinate: the oracle (oracle.cpp dda_ray() lines 772-780) takes the cell
// c = clamp(floor(x), 0, n - 1) and then q = clamp(floor(256 x), 256 c, 256 c + 255), both floors
// as its x86 conversion gives them (NaN and |.| >= 2^63: INT64_MIN).  y = 256 x is exact, and
// floor(floor(y) / 256) = floor(x), so while floor(y) converts, c = clamp(floor(y) >> 8, 0, n - 1)
// and the two clamps are one:
//   q = clamp(floor(y), 0, top),  top = 256 n - 1,   c = q >> 8   (what qray_from takes)
// (floor(y) >> 8 below 0: both give q = 0; above n - 1: both give top; else q = floor(y), inside its
// cell).  Truncation serves as the floor: they differ only below 0, which clamps to 0; a NaN
// gives 0 either way (the oracle: c = 0, q = clamp(INT64_MIN)), and so does everything below
// -2^31.  Two floors and one clamp per axis instead of four and four.
// A value that saturates the 32-bit conversion (y >= 2^31 - 1, far outside any grid) takes
// quant_far: up to 2^63 both of the oracle's conversions still succeed (c = n - 1, q = top); from
// 2^63 to 2^71 floor(y) fails while floor(x) converts (c = n - 1, q = 256 c = top - 255); from
// 2^71 on, +inf included, both fail (c = 0, q = 0).
__host__ __device__ inline int32_t quant_far(double y, int32_t top) {
  return y < 9223372036854775808.0 ? top : (y < 2361183241434822606848.0 ? top - ((int32_t)kQ - 1) : 0);
}
__host__ __device__ inline int32_t quant_coord(double x, int32_t top) {
  const double y = x * (double)kQ;
  const int32_t i = trunc_sat32(y);
  int32_t q = imin32(imax32(i, 0), top);  // (top >= 0: the clamp in two instructions)
  if (i == INT32_MAX) {
    keep_branch();
    q = quant_far(y, top);
  }
  return q;
}

// Clip O->E to the grid and quantise the clipped endpoints to 1/256 cell (clamped
// into their cells).  Mirrors oracle.cpp dda_ray() lines 752-780; go = grid_origin(O), ge =
// grid_origin(E), end_inside = endpoint_inside_ge(g, E, ge) (so 0 <= ge < n where it is set).
// Returns false when the ray misses the grid.
// A ray that ends inside the grid has t1 overwritten by 1, so of each axis' two slab
// quotients only the entry one, min(ta, tb), matters, and only when it can exceed t0 >= 0:
// (0 - go) / D for D > 0, which is <= 0 unless go < 0, and (n - go) / D for D < 0, which is
// <= 0 unless go > n (division is monotone and keeps the sign) -- so the other divisions
// are skipped with identical t0 and t1.
// The quantised values: quant_coord above.
__host__ __device__ inline bool dda_quantize_ge(const Geom& g, const double go[3], const double ge[3], bool end_inside,
                                                int32_t qs[3], int32_t qe[3]) {
  double D[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) D[a] = ge[a] - go[a];
  double t0 = 0.0, t1 = 1.0;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    if (D[a] == 0.0) {
      if (go[a] < 0.0 || go[a] >= (double)g.n[a]) return false;
    } else if (end_inside) {
      if (D[a] > 0.0 ? go[a] < 0.0 : go[a] > (double)g.n[a]) {
        const double lo = (D[a] > 0.0 ? 0.0 - go[a] : (double)g.n[a] - go[a]) / D[a];
        if (lo > t0) t0 = lo;
      }
    } else {
      double ta = (0.0 - go[a]) / D[a];
      double tb = ((double)g.n[a] - go[a]) / D[a];
      if (ta > tb) { const double tt = ta; ta = tb; tb = tt; }
      if (ta > t0) t0 = ta;
      if (tb < t1) t1 = tb;
    }
  }
  if (end_inside) { t1 = 1.0; if (t0 > 1.0) t0 = 1.0; }
  if (t0 > t1) return false;
  double gs[3], gx[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    gs[a] = go[a] + t0 * D[a];
    gx[a] = ge[a];
  }
  if (!end_inside) {  // (the headline's rays end inside the grid)
    keep_branch();
#pragma unroll
    for (int a = 0; a < 3; ++a) gx[a] = go[a] + t1 * D[a];
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const int32_t top = (int32_t)g.n[a] * (int32_t)kQ - 1;
    qs[a] = quant_coord(gs[a], top);
    qe[a] = quant_coord(gx[a], top);
  }
  return true;
}

// dda_quantize_ge from the endpoint itself: its grid coordinates, taken once, give the acceptance
// (*inside) and the clip.
__host__ __device__ inline bool dda_quantize_go(const Geom& g, const double go[3], const float E[3], bool* inside,
                                                int32_t qs[3], int32_t qe[3]) {
  double ge[3];
  grid_origin(g, E, ge);
  *inside = endpoint_inside_ge(g, E, ge);
  return dda_quantize_ge(g, go, ge, *inside, qs, qe);
}

}  // namespace dmf
