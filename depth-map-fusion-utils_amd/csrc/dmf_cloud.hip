// dmf_cloud.hip — exact nearest neighbour of every query point in a reference cloud, and the
// cloud-error summary built on it (include/dmf.h dmf_cloud_nearest*): what
// the reference's tests/ErrorCalc.cpp:71-97 asks of PCL's k-d tree, one point at a time.
//
// A uniform index of cubic cells over the valid reference points, built and queried on the device
// (the device form never waits for the host): bounds -> sizing -> histogram, scan, scatter into
// cell-sorted 16-byte records -> per query, shells of cells outwards from its home cell until a
// lower bound on everything not yet scanned exceeds the best.  The result is the lexicographic
// minimum of (d2, index), which does not depend on the order in which candidates are met.
#include <algorithm>
#include <cfloat>

#include "dmf_host.hpp"

namespace dmf {

constexpr int kClThreads = 256;
constexpr unsigned kClMaxWgs = 4096;      // grid-stride beyond
constexpr int kClAxisCap = 1024;          // cells per axis ...
constexpr uint32_t kClCellCap = 1u << 22; // ... and in all: 32 MiB of counts and offsets at the most
constexpr int kClCellBits = 22;
// dmf_cloud_nearest_set_variant(0, 0), measured: a target mean of 4 points per cell
// of the box, and the queries sorted by home cell first
constexpr int kClDefaultOcc = 4;
constexpr int kClDefaultOrder = 2;
constexpr int32_t kClNone = 0x7fffffff;   // "no candidate yet": above every index (m <= 2^31 - 1)
constexpr int kClMaxThr = 8;

// The call's control block in device scratch: the bounds reduction, the index parameters that
// k_cl_size derives from it, and the summary accumulators.
struct ClCtl {
  uint32_t kmin[3], kmax[3];  // per axis: ordered keys (cl_key) of the least / largest valid coordinate
  uint32_t kabs;              // bits of the largest |coordinate|
  uint32_t maxbits;           // bits of the largest sqrtf(dist2) (non-negative floats order as their bits)
  unsigned long long nvalid;  // valid reference points
  float lo[3], hi[3];         // the box
  float inv;                  // cells per unit length (one for all axes: cubic cells)
  int32_t n[3];               // cells per axis
  double h, slop;             // 1 / inv and the binning's rounding allowance (k_cl_size)
  unsigned long long cnt[1 + kClMaxThr];  // queries with a neighbour; of those, over threshold k
  double sum;
  unsigned long long stats[2];  // DMF_EXP_STATS: candidates examined, shells scanned
};

struct ClThr {
  double t[kClMaxThr];
  int32_t T;
};

__device__ inline uint32_t cl_key(float f) {
  const uint32_t b = __float_as_uint(f);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ inline float cl_unkey(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }
__device__ inline bool cl_finite(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }
__device__ inline bool cl_valid(float x, float y, float z) { return cl_finite(x) && cl_finite(y) && cl_finite(z); }

// The cell of coordinate r on an axis of n cells: monotone in r, since each float operation is.
__device__ inline int cl_cell(float r, float lo, float inv, int n) {
  const float u = (r - lo) * inv;
  return (int)floorf(fminf(fmaxf(u, 0.0f), (float)(n - 1)));
}

__global__ void k_cl_init(ClCtl* ctl) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    for (int a = 0; a < 3; ++a) {
      ctl->kmin[a] = 0xffffffffu;
      ctl->kmax[a] = 0;
    }
    ctl->kabs = 0;
    ctl->maxbits = 0;
    ctl->nvalid = 0;
    for (int k = 0; k <= kClMaxThr; ++k) ctl->cnt[k] = 0;
    ctl->sum = 0.0;
    ctl->stats[0] = ctl->stats[1] = 0;
  }
}

// 1. Bounds: min / max per axis, the largest magnitude and the count of the valid reference points.
__global__ __launch_bounds__(kClThreads) void k_cl_bounds(const float* __restrict__ ref, int64_t m, ClCtl* ctl) {
  float mn0 = INFINITY, mn1 = INFINITY, mn2 = INFINITY, mx0 = -INFINITY, mx1 = -INFINITY, mx2 = -INFINITY, ab = 0.0f;
  unsigned long long c = 0;
  const int64_t stride = (int64_t)gridDim.x * kClThreads;
  for (int64_t j = (int64_t)blockIdx.x * kClThreads + threadIdx.x; j < m; j += stride) {
    const float x = ref[3 * j], y = ref[3 * j + 1], z = ref[3 * j + 2];
    if (!cl_valid(x, y, z)) continue;
    mn0 = fminf(mn0, x); mx0 = fmaxf(mx0, x);
    mn1 = fminf(mn1, y); mx1 = fmaxf(mx1, y);
    mn2 = fminf(mn2, z); mx2 = fmaxf(mx2, z);
    ab = fmaxf(ab, fmaxf(fabsf(x), fmaxf(fabsf(y), fabsf(z))));
    ++c;
  }
  for (int o = 32; o > 0; o >>= 1) {
    mn0 = fminf(mn0, __shfl_xor(mn0, o)); mx0 = fmaxf(mx0, __shfl_xor(mx0, o));
    mn1 = fminf(mn1, __shfl_xor(mn1, o)); mx1 = fmaxf(mx1, __shfl_xor(mx1, o));
    mn2 = fminf(mn2, __shfl_xor(mn2, o)); mx2 = fmaxf(mx2, __shfl_xor(mx2, o));
    ab = fmaxf(ab, __shfl_xor(ab, o));
    c += __shfl_xor(c, o);
  }
  if ((threadIdx.x & (kWave - 1)) == 0 && c) {
    atomicMin(&ctl->kmin[0], cl_key(mn0)); atomicMax(&ctl->kmax[0], cl_key(mx0));
    atomicMin(&ctl->kmin[1], cl_key(mn1)); atomicMax(&ctl->kmax[1], cl_key(mx1));
    atomicMin(&ctl->kmin[2], cl_key(mn2)); atomicMax(&ctl->kmax[2], cl_key(mx2));
    atomicMax(&ctl->kabs, __float_as_uint(ab));
    atomicAdd(&ctl->nvalid, c);
  }
}

// 2. Sizing, one lane: cubic cells of edge h for a mean of `occ` points per cell of the box, at
// most kClAxisCap per axis and `limit` in all (the caller's scratch); an axis of zero extent gets
// one cell; h is at least 2^-16 of the largest magnitude, so that a float's spacing there is
// 1/256 cell at the most.  A box that no cell edge fits (no extent at all, or an extent whose
// differences overflow a float) is one cell: the query then is brute force, and still exact.
// slop bounds what the binning's two roundings can hide: with e = 2^-24,
// u = fl(fl(r - lo) * inv) = (r - lo) * inv * (1 + d), |d| <= 2e + e^2, for both points of a pair,
// each within E = the largest extent of lo; a product that underflows adds 2^-150.
__global__ void k_cl_size(ClCtl* ctl, int occ, uint32_t limit) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const unsigned long long nv = ctl->nvalid;
  float lo[3] = {0.0f, 0.0f, 0.0f}, hi[3] = {0.0f, 0.0f, 0.0f};
  double e[3] = {0.0, 0.0, 0.0}, E = 0.0;
  if (nv) {
    for (int a = 0; a < 3; ++a) {
      lo[a] = cl_unkey(ctl->kmin[a]);
      hi[a] = cl_unkey(ctl->kmax[a]);
      e[a] = (double)hi[a] - (double)lo[a];
      E = fmax(E, e[a]);
    }
  }
  int n[3] = {1, 1, 1};
  double h = 1.0;
  if (E > 0.0 && E < 0x1p127) {
    const double target = fmin(fmax(1.0, (double)nv / (double)occ), (double)limit);
    int d = 0;
    double vol = 1.0;
    for (int a = 0; a < 3; ++a)
      if (e[a] > 0.0) {
        vol *= e[a];
        ++d;
      }
    h = d == 1 ? vol / target : d == 2 ? sqrt(vol / target) : cbrt(vol / target);
    h = fmax(h, E / (double)kClAxisCap * (1.0 + 0x1p-20));
    h = fmax(h, (double)__uint_as_float(ctl->kabs) * 0x1p-16);
    h = fmax(h, 0x1p-100);
    for (;;) {
      double total = 1.0;
      for (int a = 0; a < 3; ++a) {
        n[a] = e[a] > 0.0 ? (int)fmin((double)kClAxisCap, floor(e[a] / h) + 1.0) : 1;
        total *= (double)n[a];
      }
      if (total <= (double)limit) break;
      h *= 1.25;
    }
  }
  const float inv = (float)(1.0 / h);
  for (int a = 0; a < 3; ++a) {
    ctl->lo[a] = lo[a];
    ctl->hi[a] = hi[a];
    ctl->n[a] = n[a];
  }
  ctl->inv = inv;
  ctl->h = (1.0 / (double)inv) * (1.0 - 0x1p-40);  // never above the real 1 / inv
  ctl->slop = E * 0x1p-21 * (1.0 + 0x1p-30) + (1.0 / (double)inv) * 0x1p-100;
}

// 3. Binning: the histogram by cell ...
__global__ __launch_bounds__(kClThreads) void k_cl_hist(const float* __restrict__ ref, int64_t m,
                                                         const ClCtl* __restrict__ ctl, uint32_t* __restrict__ cnt) {
  const float l0 = ctl->lo[0], l1 = ctl->lo[1], l2 = ctl->lo[2], inv = ctl->inv;
  const int n0 = ctl->n[0], n1 = ctl->n[1], n2 = ctl->n[2];
  const int64_t stride = (int64_t)gridDim.x * kClThreads;
  for (int64_t j = (int64_t)blockIdx.x * kClThreads + threadIdx.x; j < m; j += stride) {
    const float x = ref[3 * j], y = ref[3 * j + 1], z = ref[3 * j + 2];
    if (!cl_valid(x, y, z)) continue;
    const uint32_t cell = ((uint32_t)cl_cell(x, l0, inv, n0) * n1 + cl_cell(y, l1, inv, n1)) * n2 + cl_cell(z, l2, inv, n2);
    atomicAdd(&cnt[cell], 1u);
  }
}

// ... and, after the exclusive scan of the counts, the scatter into cell-sorted records {x, y, z,
// index}.  The counts run back down to zero as the slots are handed out; the order within a cell
// depends on the atomics, the query's result does not.
__global__ __launch_bounds__(kClThreads) void k_cl_scatter(const float* __restrict__ ref, int64_t m,
                                                            const ClCtl* __restrict__ ctl, const uint32_t* __restrict__ off,
                                                            uint32_t* __restrict__ cnt, float4* __restrict__ rec) {
  const float l0 = ctl->lo[0], l1 = ctl->lo[1], l2 = ctl->lo[2], inv = ctl->inv;
  const int n0 = ctl->n[0], n1 = ctl->n[1], n2 = ctl->n[2];
  const int64_t stride = (int64_t)gridDim.x * kClThreads;
  for (int64_t j = (int64_t)blockIdx.x * kClThreads + threadIdx.x; j < m; j += stride) {
    const float x = ref[3 * j], y = ref[3 * j + 1], z = ref[3 * j + 2];
    if (!cl_valid(x, y, z)) continue;
    const uint32_t cell = ((uint32_t)cl_cell(x, l0, inv, n0) * n1 + cl_cell(y, l1, inv, n1)) * n2 + cl_cell(z, l2, inv, n2);
    const uint32_t pos = off[cell] + atomicSub(&cnt[cell], 1u) - 1u;
    rec[pos] = make_float4(x, y, z, __int_as_float((int32_t)j));
  }
}

// The sorted variant's keys: the home cell of every query (0 for an invalid one) with its index.
__global__ __launch_bounds__(kClThreads) void k_cl_home(const float* __restrict__ q, int64_t n,
                                                         const ClCtl* __restrict__ ctl, uint32_t* __restrict__ keys,
                                                         uint32_t* __restrict__ vals) {
  const int n0 = ctl->n[0], n1 = ctl->n[1], n2 = ctl->n[2];
  const float inv = ctl->inv;
  const int64_t stride = (int64_t)gridDim.x * kClThreads;
  for (int64_t i = (int64_t)blockIdx.x * kClThreads + threadIdx.x; i < n; i += stride) {
    const float x = q[3 * i], y = q[3 * i + 1], z = q[3 * i + 2];
    uint32_t cell = 0;
    if (cl_valid(x, y, z)) {
      const int cx = cl_cell(fminf(fmaxf(x, ctl->lo[0]), ctl->hi[0]), ctl->lo[0], inv, n0);
      const int cy = cl_cell(fminf(fmaxf(y, ctl->lo[1]), ctl->hi[1]), ctl->lo[1], inv, n1);
      const int cz = cl_cell(fminf(fmaxf(z, ctl->lo[2]), ctl->hi[2]), ctl->lo[2], inv, n2);
      cell = ((uint32_t)cx * n1 + cy) * n2 + cz;
    }
    keys[i] = cell;
    vals[i] = (uint32_t)i;
  }
}

// The records of cells [ca, cb] (one run: z is the fastest cell index) against the best so far.
template <bool kStats>
__device__ inline void cl_scan(const uint32_t* __restrict__ off, const float4* __restrict__ rec, uint32_t ca, uint32_t cb,
                               float x, float y, float z, float& best, int32_t& bi, unsigned long long& cand) {
  const uint32_t p1 = off[cb + 1];
  for (uint32_t p = off[ca]; p < p1; ++p) {
    const float4 r = rec[p];
    const float dx = x - r.x, dy = y - r.y, dz = z - r.z;
    const float d = (dx * dx + dy * dy) + dz * dz;
    const int32_t j = __float_as_int(r.w);
    if (d < best || (d == best && j < bi)) {
      best = d;
      bi = j;
    }
  }
  if (kStats) cand += p1 - off[ca];
}

// 4 + 5. One lane per query: shells of cells outwards from the home cell of the query clamped into
// the box.  After shell s every unscanned point lies s + 1 or more cells away on some axis, so its
// coordinate differs from the clamped query's by more than s * h - slop there (k_cl_size), and from
// the query's by that plus the query's distance to the box on that axis (the home cell of a query
// outside lies on the face it is nearest to, so the gap opens away from it); on every axis it differs
// by at least the query's distance to the box.
// d2 is monotone in each |difference|, rounding included, so d2 at those lower bounds (the least
// over the axis that carries the gap) bounds the d2 of everything unscanned from below; the scan
// stops once that is strictly greater than the best (an equal one may hold a lower index).
template <bool kStats>
__global__ __launch_bounds__(kClThreads) void k_cl_query(const float* __restrict__ q, int64_t n,
                                                          const uint32_t* __restrict__ order, ClCtl* ctl,
                                                          const uint32_t* __restrict__ off, const float4* __restrict__ rec,
                                                          float* __restrict__ dist2, int32_t* __restrict__ index,
                                                          ClThr thr, int summary) {
  const float l0 = ctl->lo[0], l1 = ctl->lo[1], l2 = ctl->lo[2], h0 = ctl->hi[0], h1 = ctl->hi[1], h2 = ctl->hi[2];
  const float inv = ctl->inv;
  const int n0 = ctl->n[0], n1 = ctl->n[1], n2 = ctl->n[2];
  const double h = ctl->h, slop = ctl->slop;
  const bool any = ctl->nvalid != 0;
  unsigned long long c0 = 0, cand = 0, shells = 0;
  unsigned long long ov0 = 0, ov1 = 0, ov2 = 0, ov3 = 0, ov4 = 0, ov5 = 0, ov6 = 0, ov7 = 0;
  float emax = 0.0f;
  double esum = 0.0;
  const int64_t stride = (int64_t)gridDim.x * kClThreads;
  for (int64_t k = (int64_t)blockIdx.x * kClThreads + threadIdx.x; k < n; k += stride) {
    const int64_t i = order ? (int64_t)order[k] : k;
    const float x = q[3 * i], y = q[3 * i + 1], z = q[3 * i + 2];
    float best = INFINITY;
    int32_t bi = kClNone;
    if (any && cl_valid(x, y, z)) {
      const int cx = cl_cell(fminf(fmaxf(x, l0), h0), l0, inv, n0);
      const int cy = cl_cell(fminf(fmaxf(y, l1), h1), l1, inv, n1);
      const int cz = cl_cell(fminf(fmaxf(z, l2), h2), l2, inv, n2);
      // the query's distance to the box per axis, as d2 would form it against a point on the face
      const float ox = x < l0 ? l0 - x : x > h0 ? x - h0 : 0.0f;
      const float oy = y < l1 ? l1 - y : y > h1 ? y - h1 : 0.0f;
      const float oz = z < l2 ? l2 - z : z > h2 ? z - h2 : 0.0f;
      // ... and in reals (the doubles' own rounding is covered by the factor on the bound below)
      const double dox = x < l0 ? (double)l0 - (double)x : x > h0 ? (double)x - (double)h0 : 0.0;
      const double doy = y < l1 ? (double)l1 - (double)y : y > h1 ? (double)y - (double)h1 : 0.0;
      const double doz = z < l2 ? (double)l2 - (double)z : z > h2 ? (double)z - (double)h2 : 0.0;
      const int smax = max(max(max(cx, n0 - 1 - cx), max(cy, n1 - 1 - cy)), max(cz, n2 - 1 - cz));
      for (int s = 0;; ++s) {
        const int x0 = max(cx - s, 0), x1 = min(cx + s, n0 - 1), y0 = max(cy - s, 0), y1 = min(cy + s, n1 - 1);
        const int z0 = max(cz - s, 0), z1 = min(cz + s, n2 - 1);
        for (int xi = x0; xi <= x1; ++xi)
          for (int yi = y0; yi <= y1; ++yi) {
            const uint32_t base = ((uint32_t)xi * n1 + yi) * n2;
            if (xi - cx == s || cx - xi == s || yi - cy == s || cy - yi == s) {
              cl_scan<kStats>(off, rec, base + z0, base + z1, x, y, z, best, bi, cand);
            } else {  // (s > 0 here) the two caps of the shell, where they lie inside the grid
              if (cz - s >= 0) cl_scan<kStats>(off, rec, base + cz - s, base + cz - s, x, y, z, best, bi, cand);
              if (cz + s < n2) cl_scan<kStats>(off, rec, base + cz + s, base + cz + s, x, y, z, best, bi, cand);
            }
          }
        if (kStats) ++shells;
        if (s >= smax) break;
        // floats not above the real bounds: the gap L alone is worth nothing until it is positive
        const double L = (double)s * h - slop;
        float gx = ox, gy = oy, gz = oz;
        if (L > 0x1p-60) {
          gx = fmaxf(ox, (float)((L + dox) * (1.0 - 0x1p-23)));
          gy = fmaxf(oy, (float)((L + doy) * (1.0 - 0x1p-23)));
          gz = fmaxf(oz, (float)((L + doz) * (1.0 - 0x1p-23)));
        }
        const float bx = (gx * gx + oy * oy) + oz * oz, by = (ox * ox + gy * gy) + oz * oz,
                    bz = (ox * ox + oy * oy) + gz * gz;
        if (fminf(bx, fminf(by, bz)) > best) break;
      }
    }
    if (dist2) dist2[i] = best;
    if (index) index[i] = bi == kClNone ? DMF_NO_POINT : bi;
    if (summary && bi != kClNone) {
      const float e = sqrtf(best);
      const double ed = (double)e;
      ++c0;
      emax = fmaxf(emax, e);
      esum += ed;
      ov0 += thr.T > 0 && ed > thr.t[0];
      ov1 += thr.T > 1 && ed > thr.t[1];
      ov2 += thr.T > 2 && ed > thr.t[2];
      ov3 += thr.T > 3 && ed > thr.t[3];
      ov4 += thr.T > 4 && ed > thr.t[4];
      ov5 += thr.T > 5 && ed > thr.t[5];
      ov6 += thr.T > 6 && ed > thr.t[6];
      ov7 += thr.T > 7 && ed > thr.t[7];
    }
  }
  if (summary) {
    for (int o = 32; o > 0; o >>= 1) {
      c0 += __shfl_xor(c0, o);
      emax = fmaxf(emax, __shfl_xor(emax, o));
      esum += __shfl_xor(esum, o);
      ov0 += __shfl_xor(ov0, o); ov1 += __shfl_xor(ov1, o); ov2 += __shfl_xor(ov2, o); ov3 += __shfl_xor(ov3, o);
      ov4 += __shfl_xor(ov4, o); ov5 += __shfl_xor(ov5, o); ov6 += __shfl_xor(ov6, o); ov7 += __shfl_xor(ov7, o);
    }
    if ((threadIdx.x & (kWave - 1)) == 0 && c0) {
      atomicAdd(&ctl->cnt[0], c0);
      atomicMax(&ctl->maxbits, __float_as_uint(emax));
      atomicAdd(&ctl->sum, esum);
      if (ov0) atomicAdd(&ctl->cnt[1], ov0);
      if (ov1) atomicAdd(&ctl->cnt[2], ov1);
      if (ov2) atomicAdd(&ctl->cnt[3], ov2);
      if (ov3) atomicAdd(&ctl->cnt[4], ov3);
      if (ov4) atomicAdd(&ctl->cnt[5], ov4);
      if (ov5) atomicAdd(&ctl->cnt[6], ov5);
      if (ov6) atomicAdd(&ctl->cnt[7], ov6);
      if (ov7) atomicAdd(&ctl->cnt[8], ov7);
    }
  }
  if (kStats) {
    for (int o = 32; o > 0; o >>= 1) {
      cand += __shfl_xor(cand, o);
      shells += __shfl_xor(shells, o);
    }
    if ((threadIdx.x & (kWave - 1)) == 0 && shells) {
      atomicAdd(&ctl->stats[0], cand);
      atomicAdd(&ctl->stats[1], shells);
    }
  }
}

// The summaries as the caller reads them: counts[2 + T], sums[2].
__global__ void k_cl_finish(const ClCtl* ctl, int T, unsigned long long* counts, double* sums) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  if (counts) {
    counts[0] = ctl->cnt[0];
    counts[1] = ctl->nvalid;
    for (int k = 0; k < T; ++k) counts[2 + k] = ctl->cnt[1 + k];
  }
  if (sums) {
    sums[0] = ctl->cnt[0] ? (double)__uint_as_float(ctl->maxbits) : -1.0;
    sums[1] = ctl->sum;
  }
}

static unsigned cl_wgs(int64_t items) {
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>((items + kClThreads - 1) / kClThreads, kClMaxWgs));
}

// The plain arguments (no access to the volume: they are rejected without a device).
static int check_cloud_args(const dmf_volume* v, const void* query, int64_t n, const void* ref, int64_t m,
                            const void* dist2, const void* index, const double* thresholds, int32_t T,
                            const void* counts, const void* sums) {
  if (!v) return fail(DMF_ERR_INVALID, "null volume");
  if (n < 0 || m < 0) return fail(DMF_ERR_INVALID, "negative point count (n %lld, m %lld)", (long long)n, (long long)m);
  if ((n > 0 && !query) || (m > 0 && !ref)) return fail(DMF_ERR_INVALID, "null cloud with points");
  if (!dist2 && !index && !counts && !sums) return fail(DMF_ERR_INVALID, "no output");
  if (T < 0 || T > kClMaxThr) return fail(DMF_ERR_INVALID, "%d thresholds, at most %d", T, kClMaxThr);
  if (T > 0 && !thresholds) return fail(DMF_ERR_INVALID, "null thresholds with T = %d", T);
  if (m > 0x7fffffffll) return fail(DMF_ERR_RANGE, "the reference cloud is limited to 2^31 - 1 points");
  return DMF_OK;
}

static int cloud_device(dmf_volume* v, const float* d_query, int64_t n, const float* d_ref, int64_t m, float* d_dist2,
                        int32_t* d_index, const double* thresholds, int32_t T, uint64_t* d_counts, double* d_sums) {
  // dmf_cloud_nearest_set_variant (dmf_diag.h): the A/B of DESIGN.md §5.17
  const int occ = v->cloud_occ > 0 ? v->cloud_occ : kClDefaultOcc;
  int order = v->cloud_order > 0 ? v->cloud_order : kClDefaultOrder;
  if (n > 0xffffffffll) order = 1;  // the sort's values are 32-bit query indices
  const uint32_t ncell = (uint32_t)std::min<int64_t>(kClCellCap, m / occ + 1);
  void *ctlp, *cells, *recp;
  DMF_TRY(scratch(v, kScClCtl, sizeof(ClCtl), &ctlp));
  DMF_TRY(scratch(v, kScClCells, sizeof(uint32_t) * 2 * ((size_t)ncell + 1), &cells));
  DMF_TRY(scratch(v, kScClRec, sizeof(float4) * (size_t)std::max<int64_t>(m, 1), &recp));
  ClCtl* const ctl = (ClCtl*)ctlp;
  uint32_t* const cnt = (uint32_t*)cells;
  uint32_t* const off = cnt + ncell + 1;
  hipLaunchKernelGGL(k_cl_init, dim3(1), dim3(64), 0, v->stream, ctl);
  DMF_LAUNCH_CHECK();
  if (m > 0) {
    hipLaunchKernelGGL(k_cl_bounds, dim3(cl_wgs(m)), dim3(kClThreads), 0, v->stream, d_ref, m, ctl);
    DMF_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(k_cl_size, dim3(1), dim3(64), 0, v->stream, ctl, occ, ncell);
  DMF_LAUNCH_CHECK();
  if (n > 0) {
    DMF_HIP(hipMemsetAsync(cells, 0, sizeof(uint32_t) * 2 * ((size_t)ncell + 1), v->stream));
    if (m > 0) {
      hipLaunchKernelGGL(k_cl_hist, dim3(cl_wgs(m)), dim3(kClThreads), 0, v->stream, d_ref, m, (const ClCtl*)ctl, cnt);
      DMF_LAUNCH_CHECK();
      DMF_TRY(exclusive_scan_i32(v, (const int32_t*)cnt, (int32_t*)off, (size_t)ncell + 1));
      hipLaunchKernelGGL(k_cl_scatter, dim3(cl_wgs(m)), dim3(kClThreads), 0, v->stream, d_ref, m, (const ClCtl*)ctl,
                         (const uint32_t*)off, cnt, (float4*)recp);
      DMF_LAUNCH_CHECK();
    }
    const uint32_t* d_order = nullptr;
    if (order == 2) {
      void* keys;
      DMF_TRY(scratch(v, kScClKeys, sizeof(uint32_t) * 2 * (size_t)n, &keys));
      uint32_t* const vals = (uint32_t*)keys + n;
      hipLaunchKernelGGL(k_cl_home, dim3(cl_wgs(n)), dim3(kClThreads), 0, v->stream, d_query, n, (const ClCtl*)ctl,
                         (uint32_t*)keys, vals);
      DMF_LAUNCH_CHECK();
      DMF_TRY(sort_pairs_u32(v, (uint32_t*)keys, vals, (size_t)n, kClCellBits));
      d_order = vals;
    }
    ClThr thr = {};
    thr.T = T;
    for (int k = 0; k < T; ++k) thr.t[k] = thresholds[k];
#if defined(DMF_EXP_STATS)
    constexpr bool stats = true;
#else
    constexpr bool stats = false;
#endif
    hipLaunchKernelGGL(k_cl_query<stats>, dim3(cl_wgs(n)), dim3(kClThreads), 0, v->stream, d_query, n, d_order, ctl,
                       (const uint32_t*)off, (const float4*)recp, d_dist2, d_index, thr, (d_counts || d_sums) ? 1 : 0);
    DMF_LAUNCH_CHECK();
  }
  if (d_counts || d_sums) {
    hipLaunchKernelGGL(k_cl_finish, dim3(1), dim3(64), 0, v->stream, (const ClCtl*)ctl, (int)T,
                       (unsigned long long*)d_counts, d_sums);
    DMF_LAUNCH_CHECK();
  }
  return DMF_OK;
}

}  // namespace dmf

using namespace dmf;

extern "C" {

int dmf_cloud_nearest_device(dmf_volume* v, const float* d_query, int64_t n, const float* d_ref, int64_t m,
                             float* d_dist2, int32_t* d_index, const double* thresholds, int32_t T, uint64_t* d_counts,
                             double* d_sums) {
  DMF_API_BEGIN
  DMF_TRY(check_cloud_args(v, d_query, n, d_ref, m, d_dist2, d_index, thresholds, T, d_counts, d_sums));
  DMF_TRY(activate(v));
  return cloud_device(v, d_query, n, d_ref, m, d_dist2, d_index, thresholds, T, d_counts, d_sums);
  DMF_API_END
}

int dmf_cloud_nearest(dmf_volume* v, const float* query, int64_t n, const float* ref, int64_t m, float* dist2,
                      int32_t* index, const double* thresholds, int32_t T, uint64_t* counts, double* sums) {
  DMF_API_BEGIN
  DMF_TRY(check_cloud_args(v, query, n, ref, m, dist2, index, thresholds, T, counts, sums));
  DMF_TRY(activate(v));
  void *dq = nullptr, *dr = nullptr, *dd = nullptr, *di = nullptr, *ds = nullptr;
  if (n > 0) {
    DMF_TRY(scratch(v, kScClQuery, sizeof(float) * 3 * (size_t)n, &dq));
    DMF_HIP(hipMemcpyAsync(dq, query, sizeof(float) * 3 * (size_t)n, hipMemcpyHostToDevice, v->stream));
    if (dist2) DMF_TRY(scratch(v, kScClDist, sizeof(float) * (size_t)n, &dd));
    if (index) DMF_TRY(scratch(v, kScClIndex, sizeof(int32_t) * (size_t)n, &di));
  }
  if (m > 0) {
    DMF_TRY(scratch(v, kScClRef, sizeof(float) * 3 * (size_t)m, &dr));
    DMF_HIP(hipMemcpyAsync(dr, ref, sizeof(float) * 3 * (size_t)m, hipMemcpyHostToDevice, v->stream));
  }
  // counts[2 + 8] | sums[2]
  DMF_TRY(scratch(v, kScClSums, sizeof(uint64_t) * (2 + kClMaxThr) + sizeof(double) * 2, &ds));
  uint64_t* const dc = (uint64_t*)ds;
  double* const dsum = (double*)(dc + 2 + kClMaxThr);
  DMF_TRY(cloud_device(v, (const float*)dq, n, (const float*)dr, m, n > 0 ? (float*)dd : nullptr,
                       n > 0 ? (int32_t*)di : nullptr, thresholds, T, counts ? dc : nullptr, sums ? dsum : nullptr));
  if (n > 0 && dist2) DMF_HIP(hipMemcpyAsync(dist2, dd, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost, v->stream));
  if (n > 0 && index) DMF_HIP(hipMemcpyAsync(index, di, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, v->stream));
  if (counts) DMF_HIP(hipMemcpyAsync(counts, dc, sizeof(uint64_t) * (2 + T), hipMemcpyDeviceToHost, v->stream));
  if (sums) DMF_HIP(hipMemcpyAsync(sums, dsum, sizeof(double) * 2, hipMemcpyDeviceToHost, v->stream));
  DMF_HIP(hipStreamSynchronize(v->stream));
  return DMF_OK;
  DMF_API_END
}

int dmf_cloud_nearest_set_variant(dmf_volume* v, int32_t occ, int32_t order) {
  DMF_API_BEGIN
  if (!v) return fail(DMF_ERR_INVALID, "null volume");
  if (occ < 0 || occ > 1024 || order < 0 || order > 2)
    return fail(DMF_ERR_INVALID, "cloud variant (occ %d, order %d) outside 0..1024, 0..2", occ, order);
  v->cloud_occ = occ;
  v->cloud_order = order;
  return DMF_OK;
  DMF_API_END
}

int dmf_cloud_nearest_stats(const dmf_volume* v, uint64_t* stats4) {
  DMF_API_BEGIN
  if (!v || !stats4) return fail(DMF_ERR_INVALID, "null argument");
  for (int k = 0; k < 4; ++k) stats4[k] = 0;
  if ((int)v->scratch.size() <= kScClCtl || !v->scratch[kScClCtl].first) return DMF_OK;  // no call yet
  DMF_TRY(activate(v));
  ClCtl h;
  DMF_HIP(hipMemcpyAsync(&h, v->scratch[kScClCtl].first, sizeof(h), hipMemcpyDeviceToHost, v->stream));
  DMF_HIP(hipStreamSynchronize(v->stream));
  stats4[0] = h.stats[0];
  stats4[1] = h.stats[1];
  stats4[2] = (uint64_t)h.n[0] * (uint64_t)h.n[1] * (uint64_t)h.n[2];
  stats4[3] = h.nvalid;
  return DMF_OK;
  DMF_API_END
}

}  // extern "C"
