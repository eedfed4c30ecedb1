// dmf_views.hip — candidate views from an oriented cloud: the voxel-grid
// downsample every planner of the reference runs over its cloud (PointCloudProcessing::downsample,
// PCL's VoxelGrid as compat/shims/pcl/filters/voxel_grid.h restates it) and the camera placement
// that follows it (Algorithms::positionCameras), bit for bit, and the chain surface -> downsample
// -> placement over a fused grid.
//  k_vw_bounds  — per-axis min / max of the points with three finite coordinates, and their number;
//  k_vw_setup   — one thread: the leaf box (min_b, div) in float32 as the host forms it, or "refused";
//  k_vw_keys    — a point's leaf key i0 + i1 div0 + i2 div0 div1, all ones for a skipped point;
//  (rocPRIM)    — stable sort of (key, index): a leaf's points in ascending index;
//  k_vw_flags / (rocPRIM scan) / k_vw_starts — the segment heads and each leaf's first position;
//  k_vw_maxpop, k_vw_totals — the largest population and the three counts;
//  k_vw_means   — one walker per leaf over its sorted run: the float32 adds in ascending index are
//                 the contract, so a leaf's sum is never split across lanes;
//  k_vw_place   — positionCamera(s) per location.
#include "dmf_host.hpp"

namespace dmf {

constexpr int kVwThreads = 256;
constexpr uint32_t kVwSkip = 0xFFFFFFFFu;  // no leaf has this key: a grid has at most 2^31 - 1 leaves

struct VwCtl {
  uint32_t mn[3], mx[3];  // ordered encodings (vw_enc) of the finite points' per-axis min and max
  uint32_t refused;       // the grid has more than 2^31 - 1 leaves, or a leaf coordinate leaves int32
  uint32_t maxpop;
  unsigned long long nfinite, leaves;
  int32_t min_b[3];
  uint32_t div0, div01;
};
struct VwInv {
  float a[3];
};

// float bits <-> an unsigned key of the same order (-0 below +0; only finite values are encoded)
__device__ inline uint32_t vw_enc(uint32_t u) { return u ^ ((uint32_t)((int32_t)u >> 31) | 0x80000000u); }
__device__ inline float vw_dec(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? k ^ 0x80000000u : ~k); }
__device__ inline bool vw_finite(uint32_t u) { return (u & 0x7f800000u) != 0x7f800000u; }

__global__ void k_vw_init(VwCtl* __restrict__ ctl) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    for (int a = 0; a < 3; ++a) {
      ctl->mn[a] = 0xFFFFFFFFu;
      ctl->mx[a] = 0u;
      ctl->min_b[a] = 0;
    }
    ctl->refused = 0u;
    ctl->maxpop = 0u;
    ctl->nfinite = 0ull;
    ctl->leaves = 0ull;
    ctl->div0 = 1u;
    ctl->div01 = 1u;
  }
}

__global__ __launch_bounds__(kVwThreads) void k_vw_bounds(const uint32_t* __restrict__ xyz, int64_t n,
                                                          VwCtl* __restrict__ ctl) {
  uint32_t mn[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, mx[3] = {0u, 0u, 0u}, cnt = 0u;
  const int64_t stride = (int64_t)gridDim.x * kVwThreads;
  for (int64_t i = (int64_t)blockIdx.x * kVwThreads + threadIdx.x; i < n; i += stride) {
    const uint32_t p[3] = {xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]};
    if (!(vw_finite(p[0]) && vw_finite(p[1]) && vw_finite(p[2]))) continue;
    ++cnt;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const uint32_t k = vw_enc(p[a]);
      mn[a] = min(mn[a], k);
      mx[a] = max(mx[a], k);
    }
  }
  for (int o = 32; o > 0; o >>= 1) {
    cnt += __shfl_down(cnt, o, 64);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      mn[a] = min(mn[a], (uint32_t)__shfl_down(mn[a], o, 64));
      mx[a] = max(mx[a], (uint32_t)__shfl_down(mx[a], o, 64));
    }
  }
  if ((threadIdx.x & 63) == 0 && cnt) {
    atomicAdd(&ctl->nfinite, (unsigned long long)cnt);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      atomicMin(&ctl->mn[a], mn[a]);
      atomicMax(&ctl->mx[a], mx[a]);
    }
  }
}

// min_b = (int)floorf(min * inv), max_b likewise, div = max_b - min_b + 1 (voxel_grid.h).  Refused:
// a bound's leaf coordinate at or beyond 2^31 in magnitude (or NaN, from an infinite inverse), or
// more than 2^31 - 1 leaves.
__global__ void k_vw_setup(VwCtl* __restrict__ ctl, VwInv inv) {
  if (threadIdx.x != 0 || blockIdx.x != 0 || ctl->nfinite == 0ull) return;
  long long div[3];
  bool bad = false;
  for (int a = 0; a < 3; ++a) {
    const float lo = floorf(vw_dec(ctl->mn[a]) * inv.a[a]), hi = floorf(vw_dec(ctl->mx[a]) * inv.a[a]);
    if (!(fabsf(lo) < 2147483648.0f) || !(fabsf(hi) < 2147483648.0f)) {
      bad = true;
      div[a] = 1;
      continue;
    }
    ctl->min_b[a] = (int)lo;
    div[a] = (long long)(int)hi - (long long)(int)lo + 1;
  }
  // (each div is at most 2^32, so the products are formed only below 2^31 * 2^32)
  if (!bad) bad = div[0] > 2147483647ll || div[1] > 2147483647ll || div[2] > 2147483647ll;
  if (!bad) bad = div[0] * div[1] > 2147483647ll;
  if (!bad) bad = div[0] * div[1] * div[2] > 2147483647ll;
  if (bad) {
    ctl->refused = 1u;
    return;
  }
  ctl->div0 = (uint32_t)div[0];
  ctl->div01 = (uint32_t)(div[0] * div[1]);
}

__global__ __launch_bounds__(kVwThreads) void k_vw_keys(const uint32_t* __restrict__ xyz, int64_t n,
                                                        const VwCtl* __restrict__ ctl, VwInv inv,
                                                        uint32_t* __restrict__ keys, uint32_t* __restrict__ vals) {
  const int64_t i = (int64_t)blockIdx.x * kVwThreads + threadIdx.x;
  if (i >= n) return;
  const uint32_t p[3] = {xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]};
  uint32_t key = kVwSkip;
  if (!ctl->refused && vw_finite(p[0]) && vw_finite(p[1]) && vw_finite(p[2])) {
    const uint32_t i0 = (uint32_t)((int)floorf(__uint_as_float(p[0]) * inv.a[0]) - ctl->min_b[0]);
    const uint32_t i1 = (uint32_t)((int)floorf(__uint_as_float(p[1]) * inv.a[1]) - ctl->min_b[1]);
    const uint32_t i2 = (uint32_t)((int)floorf(__uint_as_float(p[2]) * inv.a[2]) - ctl->min_b[2]);
    key = i0 + i1 * ctl->div0 + i2 * ctl->div01;
  }
  keys[i] = key;
  vals[i] = (uint32_t)i;
}

// flags[i] = sorted position i opens a leaf; flags[n] = 0, so that the scan's entry n is the number of leaves
__global__ __launch_bounds__(kVwThreads) void k_vw_flags(const uint32_t* __restrict__ keys, int64_t n,
                                                         int32_t* __restrict__ flags) {
  const int64_t i = (int64_t)blockIdx.x * kVwThreads + threadIdx.x;
  if (i > n) return;
  int32_t f = 0;
  if (i < n) {
    const uint32_t k = keys[i];
    f = k != kVwSkip && (i == 0 || keys[i - 1] != k);
  }
  flags[i] = f;
}

// start[j] = the first sorted position of leaf j; start[leaves] = the finite points (skipped
// points sort behind every leaf)
__global__ __launch_bounds__(kVwThreads) void k_vw_starts(const int32_t* __restrict__ flags,
                                                          const int32_t* __restrict__ pos, int64_t n,
                                                          VwCtl* __restrict__ ctl, uint32_t* __restrict__ start) {
  const int64_t i = (int64_t)blockIdx.x * kVwThreads + threadIdx.x;
  if (i > n) return;
  if (i == n) {
    const uint32_t m = (uint32_t)pos[n];
    start[m] = ctl->refused ? 0u : (uint32_t)ctl->nfinite;
    ctl->leaves = m;
  } else if (flags[i]) {
    start[pos[i]] = (uint32_t)i;
  }
}

__global__ __launch_bounds__(kVwThreads) void k_vw_maxpop(const int32_t* __restrict__ pos, int64_t n,
                                                          const uint32_t* __restrict__ start, VwCtl* __restrict__ ctl) {
  const int64_t j = (int64_t)blockIdx.x * kVwThreads + threadIdx.x;
  uint32_t c = 0u;
  if (j < (int64_t)pos[n]) c = start[j + 1] - start[j];
  for (int o = 32; o > 0; o >>= 1) c = max(c, (uint32_t)__shfl_down(c, o, 64));
  if ((threadIdx.x & 63) == 0 && c) atomicMax(&ctl->maxpop, c);
}

__global__ void k_vw_totals(const VwCtl* __restrict__ ctl, unsigned long long* __restrict__ count) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    count[0] = ctl->refused ? 0xFFFFFFFFFFFFFFFFull : ctl->leaves;
    count[1] = ctl->nfinite;
    count[2] = ctl->maxpop;
  }
}

// Leaf j: acc = 0.0f, then its points in ascending input index, one float32 add at a time;
// mean = acc / (float)count (dmf_compat::mean_point).  unit: the mean normal over
// sqrtf(x*x + (y*y + z*z)), a zero mean normal kept.
__global__ __launch_bounds__(kVwThreads) void k_vw_means(const float* __restrict__ xyz, const float* __restrict__ nrm,
                                                         const uint32_t* __restrict__ vals,
                                                         const uint32_t* __restrict__ start,
                                                         const VwCtl* __restrict__ ctl, int64_t cap, int unit,
                                                         float* __restrict__ out_xyz, float* __restrict__ out_nrm,
                                                         int32_t* __restrict__ out_pts) {
  const int64_t j = (int64_t)blockIdx.x * kVwThreads + threadIdx.x;
  if (j >= cap || j >= (int64_t)ctl->leaves) return;
  const uint32_t s = start[j], e = start[j + 1];
  const float cnt = (float)(e - s);
  if (out_pts) out_pts[j] = (int32_t)(e - s);
  if (out_xyz) {
    float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f;
    for (uint32_t k = s; k < e; ++k) {
      const int64_t i = vals[k];
      a0 += xyz[3 * i];
      a1 += xyz[3 * i + 1];
      a2 += xyz[3 * i + 2];
    }
    out_xyz[3 * j] = a0 / cnt;
    out_xyz[3 * j + 1] = a1 / cnt;
    out_xyz[3 * j + 2] = a2 / cnt;
  }
  if (out_nrm) {
    float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f;
    for (uint32_t k = s; k < e; ++k) {
      const int64_t i = vals[k];
      a0 += nrm[3 * i];
      a1 += nrm[3 * i + 1];
      a2 += nrm[3 * i + 2];
    }
    a0 = a0 / cnt;
    a1 = a1 / cnt;
    a2 = a2 / cnt;
    if (unit && !(a0 == 0.0f && a1 == 0.0f && a2 == 0.0f)) {
      const float q = sqrtf(sum3(a0 * a0, a1 * a1, a2 * a2));
      a0 = a0 / q;
      a1 = a1 / q;
      a2 = a2 / q;
    }
    out_nrm[3 * j] = a0;
    out_nrm[3 * j + 1] = a1;
    out_nrm[3 * j + 2] = a2;
  }
}

// positionCameras / positionCamera (compat/Algorithms.hpp).  m entries, or min(*d_m, m) when d_m is
// given (the chain: the leaves of the downsample before it; a refused grid places nothing).
__global__ __launch_bounds__(kVwThreads) void k_vw_place(const float* __restrict__ xyz, float* __restrict__ nrm,
                                                         int64_t m, const unsigned long long* __restrict__ d_m,
                                                         float dist, int keep, float* __restrict__ poses) {
  const int64_t i = (int64_t)blockIdx.x * kVwThreads + threadIdx.x;
  if (i >= m) return;
  if (d_m) {
    const unsigned long long lim = *d_m;
    if (lim == 0xFFFFFFFFFFFFFFFFull || (unsigned long long)i >= lim) return;
  }
  float nv[3] = {nrm[3 * i], nrm[3 * i + 1], nrm[3 * i + 2]};
  if (!keep && nv[2] <= 0.0f) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      nv[a] = -nv[a];
      nrm[3 * i + a] = nv[a];
    }
  }
  float* const q = poses + 12 * i;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    q[4 * a] = a == 1 ? -1.0f : 0.0f;
    q[4 * a + 1] = a == 0 ? 1.0f : 0.0f;
    q[4 * a + 2] = -nv[a];
    q[4 * a + 3] = (float)((double)(dist * nv[a]) + (double)xyz[3 * i + a]);
  }
}

static inline unsigned vw_wgs(int64_t n) { return (unsigned)((n + kVwThreads - 1) / kVwThreads); }

static int check_leaf(const float* leaf) {
  if (!leaf) return fail(DMF_ERR_INVALID, "null leaf");
  for (int a = 0; a < 3; ++a)
    if (!(leaf[a] > 0.0f) || !std::isfinite(leaf[a]))
      return fail(DMF_ERR_INVALID, "leaf[%d] = %g must be finite and > 0", a, (double)leaf[a]);
  return DMF_OK;
}

static int check_downsample_args(const dmf_volume* v, const void* xyz, const void* normals, int64_t n,
                                 const float* leaf, uint32_t flags, const void* out_normals, int64_t cap) {
  if (!v) return fail(DMF_ERR_INVALID, "null volume");
  if (n < 0) return fail(DMF_ERR_INVALID, "negative point count %lld", (long long)n);
  if (n > 0 && !xyz) return fail(DMF_ERR_INVALID, "null cloud with points");
  if (cap < 0) return fail(DMF_ERR_INVALID, "negative capacity %lld", (long long)cap);
  if (flags & ~(uint32_t)DMF_DOWNSAMPLE_UNIT_NORMALS) return fail(DMF_ERR_INVALID, "unknown downsample flags %u", flags);
  if (out_normals && !normals && n > 0) return fail(DMF_ERR_INVALID, "normals asked of a cloud without normals");
  DMF_TRY(check_leaf(leaf));
  if (n > 0x7fffffffll) return fail(DMF_ERR_RANGE, "the cloud is limited to 2^31 - 1 points");
  return DMF_OK;
}

// Bounds, keys, order and segment heads, left in the volume's scratch for downsample_emit;
// d_count[3] = {leaves or DMF_LEAVES_REFUSED, finite points, largest leaf population}.
static int downsample_count(dmf_volume* v, const float* d_xyz, int64_t n, const float* leaf, uint64_t* d_count) {
  void* ctlp;
  DMF_TRY(scratch(v, kScVwCtl, sizeof(VwCtl), &ctlp));
  VwCtl* const ctl = (VwCtl*)ctlp;
  hipLaunchKernelGGL(k_vw_init, dim3(1), dim3(64), 0, v->stream, ctl);
  DMF_LAUNCH_CHECK();
  if (n > 0) {
    const VwInv inv = {{1.0f / leaf[0], 1.0f / leaf[1], 1.0f / leaf[2]}};
    void *keys, *flags, *start;
    DMF_TRY(scratch(v, kScVwKeys, sizeof(uint32_t) * 2 * (size_t)n, &keys));
    DMF_TRY(scratch(v, kScVwFlags, sizeof(int32_t) * 2 * ((size_t)n + 1), &flags));
    DMF_TRY(scratch(v, kScVwStart, sizeof(uint32_t) * ((size_t)n + 1), &start));
    uint32_t* const vals = (uint32_t*)keys + n;
    int32_t* const pos = (int32_t*)flags + n + 1;
    hipLaunchKernelGGL(k_vw_bounds, dim3(std::min(vw_wgs(n), 1024u)), dim3(kVwThreads), 0, v->stream,
                       (const uint32_t*)d_xyz, n, ctl);
    DMF_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_vw_setup, dim3(1), dim3(64), 0, v->stream, ctl, inv);
    DMF_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_vw_keys, dim3(vw_wgs(n)), dim3(kVwThreads), 0, v->stream, (const uint32_t*)d_xyz, n,
                       (const VwCtl*)ctl, inv, (uint32_t*)keys, vals);
    DMF_LAUNCH_CHECK();
    DMF_TRY(sort_pairs_u32(v, (uint32_t*)keys, vals, (size_t)n, 32));
    hipLaunchKernelGGL(k_vw_flags, dim3(vw_wgs(n + 1)), dim3(kVwThreads), 0, v->stream, (const uint32_t*)keys, n,
                       (int32_t*)flags);
    DMF_LAUNCH_CHECK();
    DMF_TRY(exclusive_scan_i32(v, (const int32_t*)flags, pos, (size_t)n + 1));
    hipLaunchKernelGGL(k_vw_starts, dim3(vw_wgs(n + 1)), dim3(kVwThreads), 0, v->stream, (const int32_t*)flags,
                       (const int32_t*)pos, n, ctl, (uint32_t*)start);
    DMF_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_vw_maxpop, dim3(vw_wgs(n)), dim3(kVwThreads), 0, v->stream, (const int32_t*)pos, n,
                       (const uint32_t*)start, ctl);
    DMF_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(k_vw_totals, dim3(1), dim3(64), 0, v->stream, (const VwCtl*)ctl, (unsigned long long*)d_count);
  DMF_LAUNCH_CHECK();
  return DMF_OK;
}

// After downsample_count on the same cloud: the first min(leaves, cap) entries of the given outputs.
static int downsample_emit(dmf_volume* v, const float* d_xyz, const float* d_nrm, int64_t n, uint32_t flags,
                           float* d_out_xyz, float* d_out_nrm, int32_t* d_out_pts, int64_t cap) {
  if (n <= 0 || cap <= 0 || (!d_out_xyz && !d_out_nrm && !d_out_pts)) return DMF_OK;
  void *ctlp, *keys, *start;
  DMF_TRY(scratch(v, kScVwCtl, 0, &ctlp));
  DMF_TRY(scratch(v, kScVwKeys, 0, &keys));
  DMF_TRY(scratch(v, kScVwStart, 0, &start));
  hipLaunchKernelGGL(k_vw_means, dim3(vw_wgs(std::min(n, cap))), dim3(kVwThreads), 0, v->stream, d_xyz, d_nrm,
                     (const uint32_t*)keys + n, (const uint32_t*)start, (const VwCtl*)ctlp, cap,
                     (int)(flags & DMF_DOWNSAMPLE_UNIT_NORMALS), d_out_xyz, d_out_nrm, d_out_pts);
  DMF_LAUNCH_CHECK();
  return DMF_OK;
}

static int check_place_args(const dmf_volume* v, const void* xyz, const void* normals, int64_t m, uint32_t flags,
                            const void* poses) {
  if (!v) return fail(DMF_ERR_INVALID, "null volume");
  if (m < 0) return fail(DMF_ERR_INVALID, "negative location count %lld", (long long)m);
  if (m > 0 && (!xyz || !normals || !poses)) return fail(DMF_ERR_INVALID, "null argument with locations");
  if (flags & ~(uint32_t)DMF_PLACE_KEEP_NORMALS) return fail(DMF_ERR_INVALID, "unknown placement flags %u", flags);
  return DMF_OK;
}

static int place(dmf_volume* v, const float* d_xyz, float* d_nrm, int64_t m, const uint64_t* d_m, uint32_t distance_mm,
                 uint32_t flags, float* d_poses) {
  if (m <= 0) return DMF_OK;
  // movePointAway's scale: the double distance in metres, narrowed to the vector's float scalar
  const float dist = (float)((double)distance_mm / 1000.0);
  hipLaunchKernelGGL(k_vw_place, dim3(vw_wgs(m)), dim3(kVwThreads), 0, v->stream, d_xyz, d_nrm, m,
                     (const unsigned long long*)d_m, dist, (int)(flags & DMF_PLACE_KEEP_NORMALS), d_poses);
  DMF_LAUNCH_CHECK();
  return DMF_OK;
}

static int check_views_args(const dmf_volume* v, const void* logodds, const float* leaf, uint32_t ds_flags,
                            uint32_t place_flags, int64_t cap) {
  if (!v || !logodds) return fail(DMF_ERR_INVALID, "null argument");
  if (cap < 0) return fail(DMF_ERR_INVALID, "negative capacity %lld", (long long)cap);
  if (ds_flags & ~(uint32_t)DMF_DOWNSAMPLE_UNIT_NORMALS)
    return fail(DMF_ERR_INVALID, "unknown downsample flags %u", ds_flags);
  if (place_flags & ~(uint32_t)DMF_PLACE_KEEP_NORMALS)
    return fail(DMF_ERR_INVALID, "unknown placement flags %u", place_flags);
  return check_leaf(leaf);
}
static const char kVwGridLimit[] = "surface views are limited to 2048 cells per axis";

// The surface cloud of a counted grid (ns cells) into kScSfXyz / kScSfNrm, and its leaves counted.
static int views_count(dmf_volume* v, const int16_t* d_logodds, int64_t ns, const float* leaf, float** sx, float** sn,
                       uint64_t* d_leafcount) {
  void *dx = nullptr, *dn = nullptr;
  if (ns > 0) {
    DMF_TRY(scratch(v, kScSfXyz, sizeof(float) * 3 * (size_t)ns, &dx));
    DMF_TRY(scratch(v, kScSfNrm, sizeof(float) * 3 * (size_t)ns, &dn));
    DMF_TRY(surface_emit(v, d_logodds, nullptr, (float*)dx, (float*)dn, ns));
  }
  *sx = (float*)dx;
  *sn = (float*)dn;
  return downsample_count(v, (const float*)dx, ns, leaf, d_leafcount);
}

__global__ void k_vw_view_counts(const unsigned long long* __restrict__ leafcount,
                                 const unsigned long long* __restrict__ surfcount,
                                 unsigned long long* __restrict__ count) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    count[0] = leafcount[0];
    count[1] = surfcount[0];
    count[2] = surfcount[1];
  }
}

}  // namespace dmf

using namespace dmf;

extern "C" {

int dmf_cloud_downsample_device(dmf_volume* v, const float* d_xyz, const float* d_normals, int64_t n,
                                const float* leaf, uint32_t flags, float* d_out_xyz, float* d_out_normals,
                                int32_t* d_out_points, int64_t cap, uint64_t* d_count) {
  DMF_API_BEGIN
  DMF_TRY(check_downsample_args(v, d_xyz, d_normals, n, leaf, flags, d_out_normals, cap));
  if (!d_count) return fail(DMF_ERR_INVALID, "null d_count");
  DMF_TRY(activate(v));
  DMF_TRY(downsample_count(v, d_xyz, n, leaf, d_count));
  return downsample_emit(v, d_xyz, d_normals, n, flags, d_out_xyz, d_out_normals, d_out_points, cap);
  DMF_API_END
}

int dmf_cloud_downsample(dmf_volume* v, const float* xyz, const float* normals, int64_t n, const float* leaf,
                         uint32_t flags, float* out_xyz, float* out_normals, int32_t* out_points, int64_t cap,
                         uint64_t* count) {
  DMF_API_BEGIN
  DMF_TRY(check_downsample_args(v, xyz, normals, n, leaf, flags, out_normals, cap));
  DMF_TRY(activate(v));
  void *dx = nullptr, *dn = nullptr, *dc;
  const bool want_nrm = out_normals && normals;
  if (n > 0) {
    DMF_TRY(scratch(v, kScVwInXyz, sizeof(float) * 3 * (size_t)n, &dx));
    DMF_HIP(hipMemcpyAsync(dx, xyz, sizeof(float) * 3 * (size_t)n, hipMemcpyHostToDevice, v->stream));
  }
  DMF_TRY(scratch(v, kScVwCount, sizeof(uint64_t) * 3, &dc));
  DMF_TRY(downsample_count(v, (const float*)dx, n, leaf, (uint64_t*)dc));
  uint64_t cnt[3] = {0, 0, 0};
  DMF_HIP(hipMemcpyAsync(cnt, dc, sizeof(cnt), hipMemcpyDeviceToHost, v->stream));
  DMF_HIP(hipStreamSynchronize(v->stream));
  if (count)
    for (int k = 0; k < 3; ++k) count[k] = cnt[k];
  if (cnt[0] == DMF_LEAVES_REFUSED)
    return fail(DMF_ERR_RANGE, "leaf size is too small: the grid has more than 2^31 - 1 leaves");
  const int64_t m = (int64_t)cnt[0];
  const bool outputs = out_xyz || out_normals || out_points;
  if (cap < m) {
    if (cap == 0 && !outputs) return DMF_OK;  // the size query
    return fail(DMF_ERR_CAPACITY, "need %lld entries", (long long)m);
  }
  if (m == 0 || !outputs) return DMF_OK;
  void *ox = nullptr, *on = nullptr, *op = nullptr;
  if (want_nrm) {
    DMF_TRY(scratch(v, kScVwInNrm, sizeof(float) * 3 * (size_t)n, &dn));
    DMF_HIP(hipMemcpyAsync(dn, normals, sizeof(float) * 3 * (size_t)n, hipMemcpyHostToDevice, v->stream));
    DMF_TRY(scratch(v, kScVwOutNrm, sizeof(float) * 3 * (size_t)m, &on));
  }
  if (out_xyz) DMF_TRY(scratch(v, kScVwOutXyz, sizeof(float) * 3 * (size_t)m, &ox));
  if (out_points) DMF_TRY(scratch(v, kScVwOutPts, sizeof(int32_t) * (size_t)m, &op));
  DMF_TRY(downsample_emit(v, (const float*)dx, (const float*)dn, n, flags, (float*)ox, (float*)on, (int32_t*)op, m));
  if (ox) DMF_HIP(hipMemcpyAsync(out_xyz, ox, sizeof(float) * 3 * (size_t)m, hipMemcpyDeviceToHost, v->stream));
  if (on) DMF_HIP(hipMemcpyAsync(out_normals, on, sizeof(float) * 3 * (size_t)m, hipMemcpyDeviceToHost, v->stream));
  if (op) DMF_HIP(hipMemcpyAsync(out_points, op, sizeof(int32_t) * (size_t)m, hipMemcpyDeviceToHost, v->stream));
  DMF_HIP(hipStreamSynchronize(v->stream));
  return DMF_OK;
  DMF_API_END
}

int dmf_position_cameras_device(dmf_volume* v, const float* d_xyz, float* d_normals, int64_t m, uint32_t distance_mm,
                                uint32_t flags, float* d_poses) {
  DMF_API_BEGIN
  DMF_TRY(check_place_args(v, d_xyz, d_normals, m, flags, d_poses));
  DMF_TRY(activate(v));
  return place(v, d_xyz, d_normals, m, nullptr, distance_mm, flags, d_poses);
  DMF_API_END
}

int dmf_position_cameras(dmf_volume* v, const float* xyz, float* normals, int64_t m, uint32_t distance_mm,
                         uint32_t flags, float* poses) {
  DMF_API_BEGIN
  DMF_TRY(check_place_args(v, xyz, normals, m, flags, poses));
  DMF_TRY(activate(v));
  if (m == 0) return DMF_OK;
  void *dx, *dn, *dp;
  DMF_TRY(scratch(v, kScVwOutXyz, sizeof(float) * 3 * (size_t)m, &dx));
  DMF_TRY(scratch(v, kScVwOutNrm, sizeof(float) * 3 * (size_t)m, &dn));
  DMF_TRY(scratch(v, kScVwPoses, sizeof(float) * 12 * (size_t)m, &dp));
  DMF_HIP(hipMemcpyAsync(dx, xyz, sizeof(float) * 3 * (size_t)m, hipMemcpyHostToDevice, v->stream));
  DMF_HIP(hipMemcpyAsync(dn, normals, sizeof(float) * 3 * (size_t)m, hipMemcpyHostToDevice, v->stream));
  DMF_TRY(place(v, (const float*)dx, (float*)dn, m, nullptr, distance_mm, flags, (float*)dp));
  DMF_HIP(hipMemcpyAsync(poses, dp, sizeof(float) * 12 * (size_t)m, hipMemcpyDeviceToHost, v->stream));
  DMF_HIP(hipMemcpyAsync(normals, dn, sizeof(float) * 3 * (size_t)m, hipMemcpyDeviceToHost, v->stream));
  DMF_HIP(hipStreamSynchronize(v->stream));
  return DMF_OK;
  DMF_API_END
}

int dmf_grid_surface_views_device(dmf_volume* v, const int16_t* d_logodds, int32_t occ_threshold,
                                  int32_t free_threshold, const float* leaf, uint32_t downsample_flags,
                                  uint32_t distance_mm, uint32_t placement_flags, float* d_poses, float* d_xyz,
                                  float* d_normals, int64_t cap, uint64_t* d_count) {
  DMF_API_BEGIN
  DMF_TRY(check_views_args(v, d_logodds, leaf, downsample_flags, placement_flags, cap));
  if (!d_count) return fail(DMF_ERR_INVALID, "null d_count");
  if (!d_poses && !d_xyz && !d_normals) return fail(DMF_ERR_INVALID, "every output is null");
  DMF_TRY(require_grid_2048(v, kVwGridLimit));
  // the surface count sizes the cloud's scratch: 16 bytes come back before the rest is enqueued
  void *sc, *lc;
  DMF_TRY(scratch(v, kScOut3, sizeof(uint64_t) * 2, &sc));
  DMF_TRY(scratch(v, kScVwCount, sizeof(uint64_t) * 3, &lc));
  DMF_TRY(surface_count(v, d_logodds, occ_threshold, free_threshold, (uint64_t*)sc));
  uint64_t scnt[2] = {0, 0};
  DMF_HIP(hipMemcpyAsync(scnt, sc, sizeof(scnt), hipMemcpyDeviceToHost, v->stream));
  DMF_HIP(hipStreamSynchronize(v->stream));
  const int64_t ns = (int64_t)scnt[0];
  float *sx, *sn;
  DMF_TRY(views_count(v, d_logodds, ns, leaf, &sx, &sn, (uint64_t*)lc));
  hipLaunchKernelGGL(k_vw_view_counts, dim3(1), dim3(64), 0, v->stream, (const unsigned long long*)lc,
                     (const unsigned long long*)sc, (unsigned long long*)d_count);
  DMF_LAUNCH_CHECK();
  const int64_t lim = std::min(cap, ns);  // (no more leaves than points)
  if (lim <= 0) return DMF_OK;
  void *ox = d_xyz, *on = d_normals;
  if (!ox && d_poses) DMF_TRY(scratch(v, kScVwOutXyz, sizeof(float) * 3 * (size_t)lim, &ox));
  if (!on && d_poses) DMF_TRY(scratch(v, kScVwOutNrm, sizeof(float) * 3 * (size_t)lim, &on));
  DMF_TRY(downsample_emit(v, sx, sn, ns, downsample_flags, (float*)ox, (float*)on, nullptr, lim));
  if (!d_poses && (placement_flags & DMF_PLACE_KEEP_NORMALS)) return DMF_OK;
  // (without poses the placement still flips the returned normals, into a scratch pose table)
  void* dp = d_poses;
  if (!dp) {
    if (!on) return DMF_OK;
    DMF_TRY(scratch(v, kScVwPoses, sizeof(float) * 12 * (size_t)lim, &dp));
    if (!ox) DMF_TRY(scratch(v, kScVwOutXyz, sizeof(float) * 3 * (size_t)lim, &ox));
  }
  return place(v, (const float*)ox, (float*)on, lim, (const uint64_t*)lc, distance_mm, placement_flags, (float*)dp);
  DMF_API_END
}

int dmf_grid_surface_views(dmf_volume* v, const int16_t* logodds, int32_t occ_threshold, int32_t free_threshold,
                           const float* leaf, uint32_t downsample_flags, uint32_t distance_mm, uint32_t placement_flags,
                           float* poses, float* xyz, float* normals, int64_t cap, uint64_t* count) {
  DMF_API_BEGIN
  DMF_TRY(check_views_args(v, logodds, leaf, downsample_flags, placement_flags, cap));
  DMF_TRY(require_grid_2048(v, kVwGridLimit));
  void *dl, *lc;
  uint64_t scnt[2] = {0, 0}, lcnt[3] = {0, 0, 0};
  DMF_TRY(surface_count_host(v, logodds, occ_threshold, free_threshold, &dl, scnt));
  const int64_t ns = (int64_t)scnt[0];
  DMF_TRY(scratch(v, kScVwCount, sizeof(uint64_t) * 3, &lc));
  float *sx, *sn;
  DMF_TRY(views_count(v, (const int16_t*)dl, ns, leaf, &sx, &sn, (uint64_t*)lc));
  DMF_HIP(hipMemcpyAsync(lcnt, lc, sizeof(lcnt), hipMemcpyDeviceToHost, v->stream));
  DMF_HIP(hipStreamSynchronize(v->stream));
  if (count) {
    count[0] = lcnt[0];
    count[1] = scnt[0];
    count[2] = scnt[1];
  }
  if (lcnt[0] == DMF_LEAVES_REFUSED)
    return fail(DMF_ERR_RANGE, "leaf size is too small: the grid has more than 2^31 - 1 leaves");
  const int64_t m = (int64_t)lcnt[0];
  const bool outputs = poses || xyz || normals;
  if (cap < m) {
    if (cap == 0 && !outputs) return DMF_OK;  // the size query
    return fail(DMF_ERR_CAPACITY, "need %lld entries", (long long)m);
  }
  if (m == 0 || !outputs) return DMF_OK;
  void *ox, *on, *dp;
  DMF_TRY(scratch(v, kScVwOutXyz, sizeof(float) * 3 * (size_t)m, &ox));
  DMF_TRY(scratch(v, kScVwOutNrm, sizeof(float) * 3 * (size_t)m, &on));
  DMF_TRY(scratch(v, kScVwPoses, sizeof(float) * 12 * (size_t)m, &dp));
  DMF_TRY(downsample_emit(v, sx, sn, ns, downsample_flags, (float*)ox, (float*)on, nullptr, m));
  DMF_TRY(place(v, (const float*)ox, (float*)on, m, nullptr, distance_mm, placement_flags, (float*)dp));
  if (poses) DMF_HIP(hipMemcpyAsync(poses, dp, sizeof(float) * 12 * (size_t)m, hipMemcpyDeviceToHost, v->stream));
  if (xyz) DMF_HIP(hipMemcpyAsync(xyz, ox, sizeof(float) * 3 * (size_t)m, hipMemcpyDeviceToHost, v->stream));
  if (normals) DMF_HIP(hipMemcpyAsync(normals, on, sizeof(float) * 3 * (size_t)m, hipMemcpyDeviceToHost, v->stream));
  DMF_HIP(hipStreamSynchronize(v->stream));
  return DMF_OK;
  DMF_API_END
}

}  // extern "C"
