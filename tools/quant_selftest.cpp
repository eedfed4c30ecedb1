// CPU self-test of the per-ray setup of the fusion DDA (csrc/dmf_quant.hpp: endpoint_inside_ge,
// dda_quantize_go / dda_quantize_ge, quant_coord; csrc/dmf_brick.hpp: qray_from, coarse_total,
// coarse_init32, pack_ray32) against an operation-for-operation copy of the code they replaced
// (namespace old_ below: four saturating floors and four clamps per axis, the endpoint binned by
// its own floor, the direction of an axis tested once per use, 64-bit record fields).  Every
// output is compared field for field: the acceptance, the miss / hit of the clip, qs, qe, every
// QRay field, the coarse walk's initial state and count, and the record's four dwords.
// Rays: random ones over four geometries (256^3 power-of-two cells; 1000^3 and 256 x 1000 x 2048
// with cells that are no power of two; 2048^3), plus the edge sets: origins on a grid face and one
// ulp either side (go == 0, go == n); D == 0 on one and on two axes; endpoints on cell boundaries
// and one fixed-point unit either side (...255 | ...256); rays that miss the grid and rays that end
// outside it; and grid coordinates given directly, so that +-0, denormals, 2^22, 2^23, 2^31,
// 2^55, 2^63, 2^71, +-inf and NaN (and their neighbours) reach every position of the clip and of
// the quantisation.  Exits non-zero on the first difference.
// run: <exe> [random rays per geometry] [seed]
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "dmf_brick.hpp"
#include "dmf_quant.hpp"

using dmf::Geom;
namespace bk = dmf::brick;

// ---- the replaced code, operation for operation ----
namespace old_ {
constexpr int64_t kQ = 256;
inline int32_t clamp32(int32_t v, int32_t lo, int32_t hi) { return v < lo ? lo : (v > hi ? hi : v); }
inline int32_t floor_sat32(double x) {
  const double f = floor(x);
  return fabs(f) < 9223372036854775808.0 ? (int32_t)fmin(fmax(f, -1073741824.0), 1073741824.0) : -(1 << 30);
}
inline double grid_coord(const Geom& g, int a, float x) {
  const double t = (double)x - g.mn[a];
  return g.pow2 ? t * g.inv[a] : t / g.dl[a];
}
inline bool valid_coords(const Geom& g, int x, int y, int z) {
  return x < g.n[0] && y < g.n[1] && z < g.n[2] && x >= 0 && y >= 0 && z >= 0;
}
inline bool endpoint_inside(const Geom& g, const float E[3]) {
  const bool in = (E[0] >= g.vlo[0]) & (E[0] <= g.vhi[0]) & (E[1] >= g.vlo[1]) & (E[1] <= g.vhi[1]) &
                  (E[2] >= g.vlo[2]) & (E[2] <= g.vhi[2]);
  if (!in) return false;
  return old_::valid_coords(g, dmf::bin_axis(g, 0, E[0]), dmf::bin_axis(g, 1, E[1]), dmf::bin_axis(g, 2, E[2]));
}
// dda_quantize_go after its first loop (ge[a] = grid_coord(g, a, E[a])): the body, unchanged
inline bool quantize_tail(const Geom& g, const double go[3], const double ge[3], bool end_inside, int64_t qs[3],
                          int64_t qe[3]) {
  double D[3];
  for (int a = 0; a < 3; ++a) D[a] = ge[a] - go[a];
  double t0 = 0.0, t1 = 1.0;
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
  for (int a = 0; a < 3; ++a) {
    const double gs = go[a] + t0 * D[a];
    const double gx = end_inside ? ge[a] : go[a] + t1 * D[a];
    const int32_t n = (int32_t)g.n[a], Q = (int32_t)kQ;
    const int32_t cs = clamp32(floor_sat32(gs), 0, n - 1);
    const int32_t ce = end_inside ? floor_sat32(ge[a]) : clamp32(floor_sat32(gx), 0, n - 1);
    qs[a] = clamp32(floor_sat32(gs * (double)kQ), cs * Q, cs * Q + Q - 1);
    qe[a] = clamp32(floor_sat32(gx * (double)kQ), ce * Q, ce * Q + Q - 1);
  }
  return true;
}
inline bool dda_quantize_go(const Geom& g, const double go[3], const float E[3], bool end_inside, int64_t qs[3],
                            int64_t qe[3]) {
  double ge[3];
  for (int a = 0; a < 3; ++a) ge[a] = old_::grid_coord(g, a, E[a]);
  return quantize_tail(g, go, ge, end_inside, qs, qe);
}
inline void pack_ray(const int64_t qs[3], const int64_t qe[3], bool end_inside, uint64_t& A, uint64_t& B) {
  A = (uint64_t)qs[0] | ((uint64_t)qs[1] << 19) | ((uint64_t)qs[2] << 38) | ((uint64_t)(end_inside ? 1 : 0) << 63);
  B = (uint64_t)qe[0] | ((uint64_t)qe[1] << 19) | ((uint64_t)qe[2] << 38) | ((uint64_t)1 << 63);
}
inline void qray_from(const int32_t qs[3], const int32_t qe[3], bool end_inside, bk::QRay& r) {
  r.end_inside = end_inside;
  r.nsteps = 0;
  for (int a = 0; a < 3; ++a) {
    r.cs[a] = qs[a] >> 8;
    r.ce[a] = qe[a] >> 8;
    const int32_t dq = qe[a] - qs[a];
    r.adq[a] = dq < 0 ? -dq : dq;
    r.st[a] = r.ce[a] > r.cs[a] ? 1 : (r.ce[a] < r.cs[a] ? -1 : 0);
    r.n[a] = r.ce[a] > r.cs[a] ? r.ce[a] - r.cs[a] : r.cs[a] - r.ce[a];
    r.h0[a] = r.st[a] > 0 ? 2 * ((r.cs[a] + 1) * (int32_t)kQ - qs[a]) : 2 * (qs[a] - r.cs[a] * (int32_t)kQ) + 1;
    r.nsteps += r.n[a];
  }
}
inline int32_t coarse_total(const bk::QRay& r) {
  int32_t total = 0;
  for (int a = 0; a < 3; ++a) {
    const int32_t off = r.cs[a] & (bk::kB - 1);
    const int32_t k0 = r.st[a] > 0 ? bk::kB - 1 - off : off;
    if (r.st[a] != 0 && r.n[a] > k0) total += (r.n[a] - 1 - k0) / bk::kB + 1;
  }
  return total;
}
inline void coarse_init32(const bk::QRay& r, bk::Coarse32& w) {
  int32_t H[3];
  w.total = old_::coarse_total(r);
  for (int a = 0; a < 3; ++a) {
    const int32_t off = r.cs[a] & (bk::kB - 1);
    const int32_t k0 = r.st[a] > 0 ? bk::kB - 1 - off : off;
    H[a] = r.h0[a] + (int32_t)(2 * kQ) * k0;
  }
  auto pr = [&](int a, int b) -> int32_t {
    if (r.st[a] && r.st[b]) {
      auto mul = [](int32_t x, int32_t y) {
        return (int64_t)((uint64_t)((uint32_t)x & 0xffffffu) * ((uint32_t)y & 0xffffffu));
      };
      const int64_t E = mul(H[a], r.adq[b]) - mul(H[b], r.adq[a]);
      return (int32_t)((E - 1) >> bk::kCoarseShift);
    }
    return r.st[a] ? -bk::kNever32 : (r.st[b] ? bk::kNever32 : -1);
  };
  w.g01 = pr(0, 1);
  w.g02 = pr(0, 2);
  w.g12 = pr(1, 2);
  w.d0 = r.adq[0];
  w.d1 = r.adq[1];
  w.d2 = r.adq[2];
}
}  // namespace old_

// ---- the comparison ----
static long long g_rays = 0, g_hit = 0, g_inside = 0, g_miss = 0, g_far = 0, g_outside_end = 0;

static void fail(const char* what, const Geom& g, const double go[3], const double ge[3]) {
  std::printf("FAIL %s: n %d %d %d pow2 %d  go %a %a %a  ge %a %a %a\n", what, g.n[0], g.n[1], g.n[2], g.pow2, go[0],
              go[1], go[2], ge[0], ge[1], ge[2]);
  std::exit(1);
}

// everything after the quantisation: QRay, coarse walk start, record
static void check_after(const Geom& g, const double go[3], const double ge[3], const int64_t qs64[3],
                        const int64_t qe64[3], const int32_t qs[3], const int32_t qe[3], bool inside) {
  for (int a = 0; a < 3; ++a)
    if (qs64[a] != qs[a] || qe64[a] != qe[a]) fail("qs / qe", g, go, ge);
  bk::QRay ro, rn;
  std::memset(&ro, 0, sizeof ro);
  std::memset(&rn, 0, sizeof rn);
  old_::qray_from(qs, qe, inside, ro);
  bk::qray_from(qs, qe, inside, rn);
  for (int a = 0; a < 3; ++a)
    if (ro.cs[a] != rn.cs[a] || ro.ce[a] != rn.ce[a] || ro.st[a] != rn.st[a] || ro.n[a] != rn.n[a] ||
        ro.adq[a] != rn.adq[a] || ro.h0[a] != rn.h0[a])
      fail("qray_from", g, go, ge);
  if (ro.nsteps != rn.nsteps || ro.end_inside != rn.end_inside) fail("qray_from nsteps", g, go, ge);
  if (old_::coarse_total(ro) != bk::coarse_total(rn)) fail("coarse_total", g, go, ge);
  bk::Coarse32 co, cn;
  old_::coarse_init32(ro, co);
  bk::coarse_init32(rn, cn);
  if (co.g01 != cn.g01 || co.g02 != cn.g02 || co.g12 != cn.g12 || co.d0 != cn.d0 || co.d1 != cn.d1 ||
      co.d2 != cn.d2 || co.total != cn.total)
    fail("coarse_init32", g, go, ge);
  uint64_t A, B;
  old_::pack_ray(qs64, qe64, inside, A, B);
  uint32_t ra[2], rb[2];
  bk::pack_ray32(qs, qe, inside, ra, rb);
  if (A != ((uint64_t)ra[0] | (uint64_t)ra[1] << 32) || B != ((uint64_t)rb[0] | (uint64_t)rb[1] << 32))
    fail("pack_ray32", g, go, ge);
  bk::QRay rd;
  bk::decode_ray(A, B, rd);
  if (rd.nsteps != rn.nsteps || rd.cs[0] != rn.cs[0] || rd.ce[2] != rn.ce[2]) fail("decode_ray", g, go, ge);
}

// a ray as the kernels see it: float origin and endpoint
static void check_ray(const Geom& g, const float O[3], const float E[3]) {
  ++g_rays;
  double go[3], go_o[3], ge[3];
  dmf::grid_origin(g, O, go);
  for (int a = 0; a < 3; ++a) {
    go_o[a] = old_::grid_coord(g, a, O[a]);
    ge[a] = old_::grid_coord(g, a, E[a]);
    if (std::memcmp(&go[a], &go_o[a], sizeof(double)) != 0) fail("grid_origin", g, go, ge);
  }
  const bool in_o = old_::endpoint_inside(g, E);
  if (in_o != dmf::endpoint_inside(g, E)) fail("endpoint_inside", g, go, ge);
  int64_t qs64[3], qe64[3];
  const bool ok_o = old_::dda_quantize_go(g, go, E, in_o, qs64, qe64);
  int32_t qs[3], qe[3];
  bool in_n = !in_o;
  const bool ok_n = dmf::dda_quantize_go(g, go, E, &in_n, qs, qe);
  if (in_n != in_o) fail("inside", g, go, ge);
  if (ok_n != ok_o) fail("hit / miss", g, go, ge);
  g_inside += in_o ? 1 : 0;
  if (!ok_o) { ++g_miss; return; }
  ++g_hit;
  if (!in_o) ++g_outside_end;
  check_after(g, go, ge, qs64, qe64, qs, qe, in_o);
}

// grid coordinates given directly (the clip and the quantisation on any double)
static void check_coords(const Geom& g, const double go[3], const double ge[3]) {
  ++g_rays;
  bool inside = true;  // the precondition of end_inside: 0 <= ge < n
  for (int a = 0; a < 3; ++a) inside = inside && ge[a] >= 0.0 && ge[a] < (double)g.n[a];
  for (int pass = 0; pass < 2; ++pass) {
    const bool ei = pass == 0 ? inside : false;  // (an accepted endpoint may also be treated as outside)
    int64_t qs64[3], qe64[3];
    int32_t qs[3], qe[3];
    const bool ok_o = old_::quantize_tail(g, go, ge, ei, qs64, qe64);
    const bool ok_n = dmf::dda_quantize_ge(g, go, ge, ei, qs, qe);
    if (ok_o != ok_n) fail("hit / miss (coords)", g, go, ge);
    if (!ok_o) { ++g_miss; continue; }
    ++g_hit;
    check_after(g, go, ge, qs64, qe64, qs, qe, ei);
  }
}

static Geom make_geom(const double mn[3], const double dl[3], const int n[3]) {
  Geom g;
  std::memset(&g, 0, sizeof g);
  g.pow2 = 1;
  for (int a = 0; a < 3; ++a) {
    g.mn[a] = mn[a];
    g.dl[a] = dl[a];
    g.n[a] = n[a];
    g.mx[a] = mn[a] + dl[a] * n[a];
    g.hdl[a] = dl[a] / 2.0;
    int e;
    const bool p2 = std::frexp(dl[a], &e) == 0.5;
    g.inv[a] = p2 ? 1.0 / dl[a] : 0.0;
    if (!p2) g.pow2 = 0;
    float lo = (float)g.mn[a];
    while (!((double)lo > g.mn[a])) lo = std::nextafterf(lo, INFINITY);
    while ((double)std::nextafterf(lo, -INFINITY) > g.mn[a]) lo = std::nextafterf(lo, -INFINITY);
    float hi = (float)g.mx[a];
    while (!((double)hi < g.mx[a])) hi = std::nextafterf(hi, -INFINITY);
    while ((double)std::nextafterf(hi, INFINITY) < g.mx[a]) hi = std::nextafterf(hi, INFINITY);
    g.vlo[a] = lo;
    g.vhi[a] = hi;
  }
  return g;
}

int main(int argc, char** argv) {
  const long long nrand = argc > 1 ? std::atoll(argv[1]) : 2500000;
  const unsigned seed = argc > 2 ? (unsigned)std::atoi(argv[2]) : 1;
  std::mt19937_64 rng(seed);
  auto u01 = [&]() { return (double)(rng() >> 11) * 0x1p-53; };

  std::vector<Geom> geoms;
  {
    const double mn[3] = {-0.5, -0.5, -0.5}, dl[3] = {0x1p-8, 0x1p-8, 0x1p-8};
    const int n[3] = {256, 256, 256};
    geoms.push_back(make_geom(mn, dl, n));  // power-of-two cells
  }
  {
    const double mn[3] = {-1.3, 0.2, -0.7}, dl[3] = {0.0037, 0.0037, 0.0037};
    const int n[3] = {1000, 1000, 1000};
    geoms.push_back(make_geom(mn, dl, n));  // no power of two
  }
  {
    const double mn[3] = {-1.0, -1.0, -1.0}, dl[3] = {0x1p-10, 0x1p-10, 0x1p-10};
    const int n[3] = {2048, 2048, 2048};
    geoms.push_back(make_geom(mn, dl, n));  // the largest grid of a 19-bit record
  }
  {
    const double mn[3] = {-0.128, -0.5, -1.024}, dl[3] = {0.001, 0.001, 0.001};
    const int n[3] = {256, 1000, 2048};
    geoms.push_back(make_geom(mn, dl, n));  // unequal dims, no power of two
  }

  for (const Geom& g : geoms) {
    auto world = [&](int a, double gc) { return (float)(g.mn[a] + gc * g.dl[a]); };  // ~ grid coordinate gc
    // random rays: origins inside and up to two grid lengths outside, endpoints mostly inside
    for (long long i = 0; i < nrand; ++i) {
      float O[3], E[3];
      const int ko = (int)(rng() % 4), ke = (int)(rng() % 8);
      for (int a = 0; a < 3; ++a) {
        const double n = g.n[a];
        const double o = ko == 0 ? u01() * n : (u01() * 5.0 - 2.0) * n;
        const double e = ke == 0 ? (u01() * 3.0 - 1.0) * n : u01() * n;
        O[a] = world(a, o);
        E[a] = world(a, e);
      }
      check_ray(g, O, E);
    }
    // origins on a grid face and one ulp either side (go == 0, go == n), D == 0 on one and two
    // axes, endpoints on cell boundaries and one fixed-point unit either side
    for (int i = 0; i < 400000; ++i) {
      float O[3], E[3];
      for (int a = 0; a < 3; ++a) {
        const double n = g.n[a];
        O[a] = world(a, (u01() * 3.0 - 1.0) * n);
        E[a] = world(a, u01() * n);
      }
      const int a = i % 3, kind = (i / 3) % 8;
      const float face = world(a, (i / 24) % 2 ? (double)g.n[a] : 0.0);
      if (kind == 0) O[a] = face;
      if (kind == 1) O[a] = std::nextafterf(face, INFINITY);
      if (kind == 2) O[a] = std::nextafterf(face, -INFINITY);
      if (kind == 3) E[a] = O[a];                                   // D == 0 on one axis
      if (kind == 4) { E[a] = O[a]; E[(a + 1) % 3] = O[(a + 1) % 3]; }  // on two
      if (kind >= 5) {
        const double cell = (double)(rng() % (uint64_t)(g.n[a] + 1));
        const double fine = kind == 5 ? 0.0 : (kind == 6 ? -1.0 / 256 : 1.0 / 256);
        E[a] = world(a, cell + fine);
        if (i % 5 == 0) { E[a] = std::nextafterf(E[a], i % 2 ? INFINITY : -INFINITY); }
      }
      check_ray(g, O, E);
      // the same ray from an origin on a face plane, with the endpoint beyond the far face
      if (kind < 3) {
        E[a] = world(a, (i % 2 ? 2.5 : -1.5) * g.n[a]);
        check_ray(g, O, E);
      }
    }
    // special values as floats: every position of O and E
    const float fs[] = {0.0f, -0.0f, FLT_MIN, -FLT_MIN, 1e-45f, -1e-45f, 4194304.0f, 8388608.0f, 2147483648.0f,
                        -2147483648.0f, 9223372036854775808.0f, -9223372036854775808.0f, 1e30f, -1e30f, FLT_MAX,
                        -FLT_MAX, INFINITY, -INFINITY, NAN};
    const int nfs = (int)(sizeof fs / sizeof fs[0]);
    for (int i = 0; i < nfs; ++i)
      for (int j = 0; j < nfs; ++j)
        for (int a = 0; a < 3; ++a)
          for (int rep = 0; rep < 8; ++rep) {
            float O[3], E[3];
            for (int b = 0; b < 3; ++b) {
              O[b] = world(b, (u01() * 3.0 - 1.0) * g.n[b]);
              E[b] = world(b, u01() * g.n[b]);
            }
            O[a] = fs[i];
            E[rep % 2 ? a : (a + 1) % 3] = fs[j];
            check_ray(g, O, E);
          }
    // special values as grid coordinates: the clip and the quantisation on any double
    const double two63 = 9223372036854775808.0;
    const double base[] = {0.0, -0.0, DBL_MIN, -DBL_MIN, 4.9e-324, -4.9e-324, 0x1p22, 0x1p23, 0x1p31, 0x1p31 - 1.0,
                           0x1p23 - 0x1p-8, -0x1p31, 0x1p55, 0x1p55 - 8.0, two63, two63 - 1024.0, -two63, 0x1p71,
                           0x1p71 - 0x1p19, 0x1p1016, 1e300, -1e300, DBL_MAX, -DBL_MAX, INFINITY, -INFINITY, NAN};
    std::vector<double> ds(base, base + sizeof base / sizeof base[0]);
    for (int a = 0; a < 3; ++a) {
      const double n = g.n[a];
      const double more[] = {n, std::nextafter(n, 0.0), std::nextafter(n, 1e9), n - 1.0 / 256, n + 1.0 / 256,
                             std::nextafter(0.0, 1.0), 1.0 - 0x1p-53, 255.0 / 256, 1.0, n / 2};
      ds.insert(ds.end(), more, more + sizeof more / sizeof more[0]);
    }
    const int nds = (int)ds.size();
    for (int i = 0; i < nds; ++i)
      for (int j = 0; j < nds; ++j)
        for (int a = 0; a < 3; ++a)
          for (int rep = 0; rep < 6; ++rep) {
            double go[3], ge[3];
            for (int b = 0; b < 3; ++b) {
              go[b] = rep < 2 ? u01() * g.n[b] : (u01() * 3.0 - 1.0) * g.n[b];
              ge[b] = u01() * g.n[b];
            }
            go[a] = ds[i];
            ge[rep % 2 ? a : (a + 1) % 3] = ds[j];
            if (rep == 5) go[(a + 2) % 3] = ds[(i + j) % nds];
            for (int b = 0; b < 3; ++b)
              if (fabs(go[b]) >= 0x1p31 || fabs(ge[b]) >= 0x1p31) { ++g_far; break; }
            check_coords(g, go, ge);
          }
  }
  // quant_coord alone against the oracle's two floors and two clamps, densely around every bound
  long long nq = 0;
  for (int n : {1, 256, 1000, 2048}) {
    const int32_t top = n * 256 - 1;
    auto one = [&](double x) {
      const int32_t c = old_::clamp32(old_::floor_sat32(x), 0, n - 1);
      const int32_t q = old_::clamp32(old_::floor_sat32(x * 256.0), c * 256, c * 256 + 255);
      if (dmf::quant_coord(x, top) != q) {
        std::printf("FAIL quant_coord: n %d x %a: %d, oracle %d\n", n, x, dmf::quant_coord(x, top), q);
        std::exit(1);
      }
      ++nq;
    };
    const double pts[] = {0.0, 1.0 / 256, 1.0, (double)n, n - 1.0 / 256, 0x1p22, 0x1p23, 0x1p23 - 0x1p-8, 0x1p31, 0x1p55,
                          0x1p63, 0x1p71, 0x1p1016, DBL_MAX, DBL_MIN, 4.9e-324, INFINITY, NAN};
    for (double p : pts)
      for (int sgn = 0; sgn < 2; ++sgn) {
        double x = sgn ? -p : p, lo = x, hi = x;
        one(x);
        for (int k = 0; k < 64; ++k) {
          lo = std::nextafter(lo, -INFINITY);
          hi = std::nextafter(hi, INFINITY);
          one(lo);
          one(hi);
        }
      }
    for (int k = -600; k <= n * 256 + 600; ++k) {  // every fixed-point unit of the axis and beyond
      one(k / 256.0);
      one(std::nextafter(k / 256.0, -INFINITY));
      one(k / 256.0 + u01() / 256.0);
    }
  }

  // the run must have met what it is meant to exercise
  if (g_hit == 0 || g_miss == 0 || g_inside == 0 || g_outside_end == 0 || g_far == 0) {
    std::printf("FAIL coverage: hit %lld miss %lld inside %lld ending outside %lld far %lld\n", g_hit, g_miss, g_inside,
                g_outside_end, g_far);
    return 1;
  }
  std::printf("quant self-test: %lld rays (%lld hit the grid, %lld miss, %lld accepted endpoints, %lld end outside, "
              "%lld with a coordinate >= 2^31), %lld single coordinates: 0 failures\n",
              g_rays, g_hit, g_miss, g_inside, g_outside_end, g_far, nq);
  return 0;
}
