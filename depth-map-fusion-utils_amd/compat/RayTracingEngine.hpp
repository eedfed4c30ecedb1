// RayTracingEngine.hpp — drop-in for the reference include/RayTracingEngine.hpp:27-564:
// same class, same eight methods, same default arguments; every trace runs on the
// MI355X through include/dmf.h.  Cheap to copy (holds only the camera), as the
// reference's callers pass it by value (Algorithms.hpp:364, tests/SetCover.cpp:218).
#pragma once
#include <cstdint>
#include <stdexcept>
#include <utility>
#include <vector>

#include "Camera.hpp"
#include "CommonUtilities.hpp"
#include "Volume.hpp"
#include "dmf.h"

constexpr double k_AngleMin = 0;
constexpr double k_AngleMax = 90;
constexpr double k_ZMin = 0.20;
constexpr double k_ZMax = 1.0;

class RayTracingEngine {
 public:
  Camera cam_;
  explicit RayTracingEngine(Camera& cam) : cam_(cam) {}

  // RayTracingEngine.hpp:45-134
  std::pair<bool, std::vector<unsigned long long int>> reverseRayTrace(VoxelVolume& volume, Eigen::Affine3f T,
                                                                       bool viz, int zdelta = 1) {
    return reverse(volume, T, viz, false);
  }
  // RayTracingEngine.hpp:136-226
  std::pair<bool, std::vector<unsigned long long int>> reverseRayTraceFast(VoxelVolume& volume, Eigen::Affine3f T,
                                                                           bool viz, int zdelta = 1) {
    return reverse(volume, T, viz, true);
  }
  // Batched extension: P poses in one launch (the set-cover loop of tests/SetCover.cpp:218-240).
  std::vector<std::pair<bool, std::vector<unsigned long long int>>> reverseRayTraceFastBatch(
      VoxelVolume& volume, const std::vector<Eigen::Affine3f>& poses, bool viz) {
    std::vector<float> p(12 * poses.size());
    for (size_t i = 0; i < poses.size(); ++i) dmf_compat::pose12(poses[i], &p[12 * i]);
    const int P = (int)poses.size();
    std::vector<uint8_t> found(P);
    std::vector<int64_t> counts(P);
    std::vector<uint64_t> out(volume.occupied_cells_.size() * (size_t)P / 2 + 64);
    const dmf_camera c = cam_.abi();
    int st = dmf_reverse_ray_trace_fast(volume.handle(), &c, p.data(), P, viz, found.data(), counts.data(),
                                        out.data(), (int64_t)out.size());
    if (st == DMF_ERR_CAPACITY) {
      int64_t tot = 0;
      for (auto n : counts) tot += n;
      out.resize((size_t)tot);
      st = dmf_reverse_ray_trace_fast(volume.handle(), &c, p.data(), P, viz, found.data(), counts.data(), out.data(),
                                      tot);
    }
    dmf_check(st);
    if (viz) volume.touch();
    std::vector<std::pair<bool, std::vector<unsigned long long int>>> res(P);
    size_t o = 0;
    for (int i = 0; i < P; ++i) {
      res[i].first = found[i] != 0;
      res[i].second.assign(out.begin() + o, out.begin() + o + counts[i]);
      o += counts[i];
    }
    return res;
  }
  // Extension (BASELINE.json north_star; no reference counterpart): 3D-DDA
  // log-odds fusion of P depth frames -- the per-frame back-project + integrate loop of
  // tests/Raytracing.cpp:70-76 / Volume.hpp:199-228 as one GPU call.  depth: P frames of
  // cam_ height x width uint16 millimetres (row-major), poses: the frames' camera -> world
  // transforms; hit / miss counts accumulate into `acc` (x-major over the volume's grid,
  // sized on first use).  dmf_fuse_depth in include/dmf.h.
  struct FusionCounts {
    std::vector<int32_t> hits, misses;  // per voxel, x-major (the reference's voxel order)
    int64_t updates = 0, rays = 0, hit_rays = 0;
  };
  FusionCounts& fuseDepth(VoxelVolume& volume, const std::vector<uint16_t>& depth,
                          const std::vector<Eigen::Affine3f>& poses, FusionCounts& acc,
                          const dmf_fuse_params* params = nullptr) {
    const size_t P = poses.size(), HW = (size_t)cam_.getHeight() * (size_t)cam_.getWidth();
    if (depth.size() != P * HW) throw std::invalid_argument("fuseDepth: depth must hold P frames of height x width");
    const size_t n = (size_t)volume.xdim_ * volume.ydim_ * volume.zdim_;
    if (acc.hits.size() != n) acc.hits.assign(n, 0);
    if (acc.misses.size() != n) acc.misses.assign(n, 0);
    std::vector<float> p(12 * P);
    for (size_t i = 0; i < P; ++i) dmf_compat::pose12(poses[i], &p[12 * i]);
    dmf_fuse_params prm;
    dmf_fuse_params_default(&prm);
    if (params) prm = *params;
    const dmf_camera c = cam_.abi();
    int64_t st[3] = {0, 0, 0};
    dmf_check(dmf_fuse_depth(volume.handle(), &c, depth.data(), p.data(), (int32_t)P, &prm, acc.hits.data(),
                             acc.misses.data(), st));
    acc.updates += st[0];
    acc.rays += st[1];
    acc.hit_rays += st[2];
    return acc;
  }
  // Extension: the same fusion of point clouds with sensor origins, the
  // insertPointCloud(scan, origin) call.  xyz: S scans of N world-frame endpoints each (packed
  // x, y, z), origins: the S world-frame sensor positions (S = origins.size() / 3).  Point i of
  // scan s is the ray origins[s] -> xyz[s][i], traced exactly as fuseDepth traces a pixel's.  A
  // point with a non-finite coordinate is no ray (pad scans of unequal length with NaN); there is
  // no range gate (params' dmin_mm / dmax_mm are not applied).  dmf_fuse_points in include/dmf.h.
  FusionCounts& fusePoints(VoxelVolume& volume, const std::vector<float>& xyz, const std::vector<float>& origins,
                           FusionCounts& acc, const dmf_fuse_params* params = nullptr) {
    const size_t S = origins.size() / 3;
    if (S == 0 || origins.size() != 3 * S || xyz.size() % (3 * S) != 0)
      throw std::invalid_argument("fusePoints: origins must hold S x 3 floats and xyz S scans of N x 3 floats");
    const size_t N = xyz.size() / (3 * S);
    const size_t n = (size_t)volume.xdim_ * volume.ydim_ * volume.zdim_;
    if (acc.hits.size() != n) acc.hits.assign(n, 0);
    if (acc.misses.size() != n) acc.misses.assign(n, 0);
    dmf_fuse_params prm;
    dmf_fuse_params_default(&prm);
    if (params) prm = *params;
    int64_t st[3] = {0, 0, 0};
    dmf_check(dmf_fuse_points(volume.handle(), xyz.data(), origins.data(), (int32_t)S, (int64_t)N, &prm,
                              acc.hits.data(), acc.misses.data(), st));
    acc.updates += st[0];
    acc.rays += st[1];
    acc.hit_rays += st[2];
    return acc;
  }
  // One cloud as readPointCloud yields it (FileRoutines.hpp), seen from one sensor position.
  FusionCounts& fusePoints(VoxelVolume& volume, const pcl::PointCloud<pcl::PointXYZRGBNormal>::Ptr& cloud,
                           const Eigen::Vector3f& origin, FusionCounts& acc, const dmf_fuse_params* params = nullptr) {
    std::vector<float> xyz;
    xyz.reserve(3 * cloud->points.size());
    for (const auto& p : cloud->points) {
      xyz.push_back(p.x);
      xyz.push_back(p.y);
      xyz.push_back(p.z);
    }
    return fusePoints(volume, xyz, std::vector<float>{origin(0), origin(1), origin(2)}, acc, params);
  }
  // The clamped int16 log-odds grid of fused counts (x-major): clamp(hits * l_hit + misses *
  // l_miss, l_min, l_max) milli-logit (dmf_fuse_finalize).
  std::vector<int16_t> logOdds(VoxelVolume& volume, const FusionCounts& acc, const dmf_fuse_params* params = nullptr) {
    dmf_fuse_params prm;
    dmf_fuse_params_default(&prm);
    if (params) prm = *params;
    std::vector<int16_t> out(acc.hits.size());
    dmf_check(dmf_fuse_finalize(volume.handle(), acc.hits.data(), acc.misses.data(), &prm, out.data()));
    return out;
  }
  // Extension: ray-cast of a fused log-odds grid (x-major int16, as logOdds
  // returns it) from P poses -- per pixel the first cell with log-odds >= threshold along the
  // fusion's probe ray of depth range_mm.  depth / cells are resized to P * height * width
  // (row-major per pose): cells = getHashId of the surface cell or DMF_NO_CELL, depth =
  // rayTraceVolume's value of that voxel or -1.  dmf_raycast_logodds in include/dmf.h.
  void rayCastLogOdds(VoxelVolume& volume, const std::vector<int16_t>& logodds,
                      const std::vector<Eigen::Affine3f>& poses, int threshold, int range_mm,
                      std::vector<int32_t>& depth, std::vector<unsigned long long int>& cells) {
    const size_t P = poses.size(), HW = (size_t)cam_.getHeight() * (size_t)cam_.getWidth();
    const size_t n = (size_t)volume.xdim_ * volume.ydim_ * volume.zdim_;
    if (logodds.size() != n) throw std::invalid_argument("rayCastLogOdds: logodds must hold xdim*ydim*zdim cells");
    std::vector<float> p(12 * P);
    for (size_t i = 0; i < P; ++i) dmf_compat::pose12(poses[i], &p[12 * i]);
    depth.assign(P * HW, -1);
    std::vector<uint64_t> h(P * HW, DMF_NO_CELL);
    const dmf_camera c = cam_.abi();
    dmf_check(dmf_raycast_logodds(volume.handle(), &c, logodds.data(), p.data(), (int32_t)P, threshold, range_mm,
                                  depth.data(), h.data()));
    cells.assign(h.begin(), h.end());
  }
  // Extension: view gain over a fused log-odds grid -- per candidate pose the
  // number of unknown cells (neither L >= occ nor L <= free) that its pixels' probe rays of depth
  // range_mm reach before their first solid cell.  gain is resized to P; seen (may be null) to
  // P * words uint64 in the mask layout of include/dmf.h (dmf_view_gain_words, dmf_view_mask_index).
  // dmf_view_gain in include/dmf.h.
  void viewGain(VoxelVolume& volume, const std::vector<int16_t>& logodds, const std::vector<Eigen::Affine3f>& poses,
                int occ, int free, int range_mm, std::vector<unsigned long long int>& gain,
                std::vector<unsigned long long int>* seen = nullptr) {
    const size_t P = poses.size();
    const size_t n = (size_t)volume.xdim_ * volume.ydim_ * volume.zdim_;
    if (logodds.size() != n) throw std::invalid_argument("viewGain: logodds must hold xdim*ydim*zdim cells");
    std::vector<float> p(12 * P);
    for (size_t i = 0; i < P; ++i) dmf_compat::pose12(poses[i], &p[12 * i]);
    int64_t words = 0;
    dmf_check(dmf_view_gain_words(volume.handle(), &words));
    std::vector<uint64_t> g(P, 0), m(seen ? P * (size_t)words : 0, 0);
    const dmf_camera c = cam_.abi();
    dmf_check(dmf_view_gain(volume.handle(), &c, logodds.data(), p.data(), (int32_t)P, occ, free, range_mm,
                            seen ? m.data() : nullptr, g.data()));
    gain.assign(g.begin(), g.end());
    if (seen) seen->assign(m.begin(), m.end());
  }
  // Extension: greedySetCover (Algorithms.hpp:38-86) over those sets -- the
  // indices of the poses to take next, in selection order.  dmf_next_best_views in include/dmf.h.
  std::vector<int> nextBestViews(VoxelVolume& volume, const std::vector<int16_t>& logodds,
                                 const std::vector<Eigen::Affine3f>& poses, int occ, int free, int range_mm,
                                 int min_gain = 5) {
    const size_t P = poses.size();
    const size_t n = (size_t)volume.xdim_ * volume.ydim_ * volume.zdim_;
    if (logodds.size() != n) throw std::invalid_argument("nextBestViews: logodds must hold xdim*ydim*zdim cells");
    std::vector<float> p(12 * P);
    for (size_t i = 0; i < P; ++i) dmf_compat::pose12(poses[i], &p[12 * i]);
    std::vector<int32_t> sel(P ? P : 1, -1);
    int32_t nsel = 0;
    const dmf_camera c = cam_.abi();
    dmf_check(dmf_next_best_views(volume.handle(), &c, logodds.data(), p.data(), (int32_t)P, occ, free, range_mm,
                                  min_gain, sel.data(), &nsel, nullptr));
    return std::vector<int>(sel.begin(), sel.begin() + nsel);
  }

  // RayTracingEngine.hpp:229-264
  int rayTraceAndGetMinimum(VoxelVolume& volume, Eigen::Affine3f& T, int zdelta = 1, bool sparse = true) {
    float p[12];
    dmf_compat::pose12(T, p);
    const dmf_camera c = cam_.abi();
    int32_t m = -1;
    dmf_check(dmf_ray_trace_and_get_minimum(volume.handle(), &c, p, zdelta, sparse, &m));
    return m;
  }
  // RayTracingEngine.hpp:268-309
  void rayTrace(VoxelVolume& volume, Eigen::Affine3f& T, int zdelta = 10, bool sparse = true) {
    float p[12];
    dmf_compat::pose12(T, p);
    const dmf_camera c = cam_.abi();
    dmf_check(dmf_ray_trace(volume.handle(), &c, p, zdelta, sparse));
    volume.touch();
  }
  // RayTracingEngine.hpp:311-375
  void rayTraceAndClassify(VoxelVolume& volume, Eigen::Affine3f& T, int zdelta = 10, int view = 1,
                           bool sparse = true) {
    float p[12];
    dmf_compat::pose12(T, p);
    const dmf_camera c = cam_.abi();
    dmf_check(dmf_ray_trace_and_classify(volume.handle(), &c, p, zdelta, view, sparse));
    volume.touch();
  }
  // RayTracingEngine.hpp:377-445
  std::pair<bool, std::vector<unsigned long long int>> rayTraceAndGetGoodPoints(VoxelVolume& volume,
                                                                                Eigen::Affine3f& T, int zdelta = 10,
                                                                                bool sparse = true) {
    return fwd_list(volume, T, zdelta, sparse, true);
  }
  // RayTracingEngine.hpp:447-494
  std::pair<bool, std::vector<unsigned long long int>> rayTraceAndGetPoints(VoxelVolume& volume, Eigen::Affine3f& T,
                                                                            int zdelta = 10, bool sparse = true) {
    return fwd_list(volume, T, zdelta, sparse, false);
  }
  // RayTracingEngine.hpp:498-564
  void rayTraceVolume(VoxelVolume& volume, Eigen::Affine3f& T) {
    float p[12];
    dmf_compat::pose12(T, p);
    const dmf_camera c = cam_.abi();
    dmf_check(dmf_ray_trace_volume(volume.handle(), &c, p, nullptr));
    volume.touch();
  }

 private:
  std::pair<bool, std::vector<unsigned long long int>> reverse(VoxelVolume& volume, const Eigen::Affine3f& T, bool viz,
                                                               bool fast) {
    float p[12];
    dmf_compat::pose12(T, p);
    const dmf_camera c = cam_.abi();
    uint8_t found = 0;
    int64_t count = 0;
    std::vector<uint64_t> out(volume.occupied_cells_.size() + 64);
    auto call = [&](int64_t cap) {
      return fast ? dmf_reverse_ray_trace_fast(volume.handle(), &c, p, 1, viz, &found, &count, out.data(), cap)
                  : dmf_reverse_ray_trace(volume.handle(), &c, p, 1, viz, &found, &count, out.data(), cap);
    };
    int st = call((int64_t)out.size());
    if (st == DMF_ERR_CAPACITY) {
      out.resize((size_t)count);
      st = call(count);
    }
    dmf_check(st);
    if (viz) volume.touch();
    return {found != 0, std::vector<unsigned long long int>(out.begin(), out.begin() + count)};
  }
  std::pair<bool, std::vector<unsigned long long int>> fwd_list(VoxelVolume& volume, Eigen::Affine3f& T, int zdelta,
                                                                bool sparse, bool good) {
    float p[12];
    dmf_compat::pose12(T, p);
    const dmf_camera c = cam_.abi();
    uint8_t found = 0;
    int64_t n = 0;
    std::vector<uint64_t> out(1 << 16);
    auto call = [&](int64_t cap) {
      return good ? dmf_ray_trace_and_get_good_points(volume.handle(), &c, p, zdelta, sparse, &found, out.data(), cap, &n)
                  : dmf_ray_trace_and_get_points(volume.handle(), &c, p, zdelta, sparse, &found, out.data(), cap, &n);
    };
    int st = call((int64_t)out.size());
    if (st == DMF_ERR_CAPACITY) {
      out.resize((size_t)n);
      st = call(n);
    }
    dmf_check(st);
    return {found != 0, std::vector<unsigned long long int>(out.begin(), out.begin() + n)};
  }
};
