// ErrorCalc.hpp — the cloud-error loop of the reference's tests/ErrorCalc.cpp:74-97 over the MI355X
// engine.  The reference builds a pcl::search::KdTree over cloud_ref (:71-72) and asks it for the
// nearest neighbour of one point at a time (:81); here ONE call finds every point's exact nearest
// neighbour on the GPU (dmf_cloud_nearest), and the loop over its distances forms
// max_error and avg_error exactly as :74-97 does.  The reference program itself is not a drop-in:
// compiled unchanged it would make one launch per point.
#pragma once
#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <vector>

#include "Volume.hpp"

namespace ErrorCalc {

struct CloudError {
  double max_error = -1.0;      // ErrorCalc.cpp:74
  double avg_error = 0.0;       // :75, divided by the points counted (:97 divides by cloud->points.size())
  std::vector<float> distance;  // per point of `cloud`: sqrt(dist[0]) of :82; +inf where there is no neighbour
  long long counted = 0;        // points with finite coordinates (PCL's search asserts on any other) and a neighbour
};

struct SurfaceError {
  long long n_surface = 0, n_valid = 0;
  double max_error = -1.0, avg_error = 0.0;
  std::vector<unsigned long long> over;  // per threshold: surface points farther than it from the model
  std::vector<float> dist2;              // per surface point, when asked for
};

inline std::vector<float> packXYZ(const pcl::PointCloud<pcl::PointXYZ>& c) {
  std::vector<float> p(3 * c.points.size());
  for (size_t i = 0; i < c.points.size(); ++i) {
    p[3 * i] = c.points[i].x;
    p[3 * i + 1] = c.points[i].y;
    p[3 * i + 2] = c.points[i].z;
  }
  return p;
}

// ErrorCalc.cpp:74-97 with `v` lending its device, stream and scratch (it need not be constructed).
inline CloudError cloudError(VoxelVolume& v, const pcl::PointCloud<pcl::PointXYZ>& cloud,
                             const pcl::PointCloud<pcl::PointXYZ>& cloud_ref) {
  const std::vector<float> q = packXYZ(cloud), r = packXYZ(cloud_ref);
  const size_t n = cloud.points.size();
  std::vector<float> dist2(n);
  std::vector<int32_t> index(n);
  CloudError e;
  e.distance.resize(n);
  if (n)
    dmf_check(dmf_cloud_nearest(v.handle(), q.data(), (int64_t)n, r.empty() ? nullptr : r.data(),
                                (int64_t)cloud_ref.points.size(), dist2.data(), index.data(), nullptr, 0, nullptr,
                                nullptr));
  for (size_t i = 0; i < n; i++) {
    const float distance = std::sqrt(dist2[i]);  // :82 (dist is a vector<float>: the float sqrt)
    e.distance[i] = distance;
    if (index[i] == DMF_NO_POINT) continue;
    if (e.max_error < distance) e.max_error = distance;  // :83-84
    e.avg_error += distance;                             // :93
    ++e.counted;
  }
  if (e.counted) e.avg_error /= (double)e.counted;  // :97
  return e;
}

inline CloudError cloudError(const pcl::PointCloud<pcl::PointXYZ>& cloud, const pcl::PointCloud<pcl::PointXYZ>& cloud_ref) {
  VoxelVolume v;
  return cloudError(v, cloud, cloud_ref);
}

// The error of the fused grid's surface (VoxelVolume::extractSurface's voxel centres) against the
// model cloud, without the surface leaving the device: dmf_grid_surface_device, then
// dmf_cloud_nearest_device; the surface count and the summaries come back, and dist2 per surface
// point when per_point is set.  thresholds: at most 8, in metres (ErrorCalc.cpp:89-91 marks 3 and 5 mm).
inline SurfaceError surfaceError(VoxelVolume& v, const std::vector<int16_t>& logodds,
                                 const pcl::PointCloud<pcl::PointXYZ>& cloud_ref, int occ_threshold = 1,
                                 int free_threshold = -1, const std::vector<double>& thresholds = {0.003, 0.005},
                                 bool per_point = false) {
  if (logodds.size() != (size_t)v.xdim_ * v.ydim_ * v.zdim_) throw std::invalid_argument("surfaceError: grid size");
  if (thresholds.size() > 8) throw std::invalid_argument("surfaceError: at most 8 thresholds");
  const std::vector<float> r = packXYZ(cloud_ref);
  const int T = (int)thresholds.size();
  dmf_volume* h = v.handle();
  std::vector<void*> bufs;
  auto alloc = [&](size_t bytes) {
    void* p = nullptr;
    dmf_check(dmf_device_malloc(h, &p, bytes ? bytes : 8));
    bufs.push_back(p);
    return p;
  };
  SurfaceError e;
  try {
    void* d_grid = alloc(logodds.size() * sizeof(int16_t));
    uint64_t* d_count = (uint64_t*)alloc(16);
    float* d_ref = (float*)alloc(r.size() * sizeof(float));
    dmf_check(dmf_memcpy_h2d(h, d_grid, logodds.data(), logodds.size() * sizeof(int16_t)));
    if (!r.empty()) dmf_check(dmf_memcpy_h2d(h, d_ref, r.data(), r.size() * sizeof(float)));
    // the count first (capacity 0: nothing is written), then the centres into a buffer of that size
    uint64_t count[2] = {0, 0};
    dmf_check(dmf_grid_surface_device(h, (const int16_t*)d_grid, occ_threshold, free_threshold, nullptr,
                                      (float*)alloc(8), nullptr, 0, d_count));
    dmf_check(dmf_memcpy_d2h(h, count, d_count, sizeof(count)));
    const int64_t n = (int64_t)count[0];
    float* d_xyz = (float*)alloc(12 * (size_t)n);
    if (n)
      dmf_check(dmf_grid_surface_device(h, (const int16_t*)d_grid, occ_threshold, free_threshold, nullptr, d_xyz,
                                        nullptr, n, d_count));
    float* d_d2 = per_point && n ? (float*)alloc(4 * (size_t)n) : nullptr;
    uint64_t* d_cnt = (uint64_t*)alloc(8 * (2 + (size_t)T));
    double* d_sums = (double*)alloc(16);
    dmf_check(dmf_cloud_nearest_device(h, n ? d_xyz : nullptr, n, r.empty() ? nullptr : d_ref,
                                       (int64_t)cloud_ref.points.size(), d_d2, nullptr, T ? thresholds.data() : nullptr,
                                       T, d_cnt, d_sums));
    std::vector<uint64_t> cnt(2 + (size_t)T);
    double sums[2];
    dmf_check(dmf_memcpy_d2h(h, cnt.data(), d_cnt, cnt.size() * sizeof(uint64_t)));
    dmf_check(dmf_memcpy_d2h(h, sums, d_sums, sizeof(sums)));
    if (d_d2) {
      e.dist2.resize((size_t)n);
      dmf_check(dmf_memcpy_d2h(h, e.dist2.data(), d_d2, 4 * (size_t)n));
    }
    e.n_surface = n;
    e.n_valid = (long long)cnt[0];
    e.max_error = sums[0];
    e.avg_error = cnt[0] ? sums[1] / (double)cnt[0] : 0.0;
    e.over.assign(cnt.begin() + 2, cnt.end());
  } catch (...) {
    for (void* p : bufs) dmf_device_free(h, p);
    throw;
  }
  for (void* p : bufs) dmf_device_free(h, p);
  return e;
}

}  // namespace ErrorCalc
