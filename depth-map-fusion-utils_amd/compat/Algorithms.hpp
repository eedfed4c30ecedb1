// Algorithms.hpp — drop-in for the set-cover consumer of the reference hot path:
// Algorithms::greedySetCover (include/Algorithms.hpp:38-86; the driver loop of
// tests/SetCover.cpp:218-240 batched as dmf_compat::setCoverBatched), and the camera
// placement the reference drivers call (positionCameras, :114-122, 189-298).  The greedy runs on the MI355X over bitmask
// sets (popcount of good & ~covered per candidate); the host only maps set elements
// to bit positions.  Same selection rule as the reference: remaining ids scanned in
// increasing order, strictly largest new-element count wins, stop when nothing is
// new or the best adds fewer than 5.  (The reference's console prints are dropped.)
#pragma once
#include <algorithm>
#include <cassert>
#include <memory>
#include <numeric>
#include <unordered_map>
#include <vector>

#include "RayTracingEngine.hpp"
#include "Volume.hpp"
#include "dmf.h"

namespace dmf_compat {
// A constructed 1-cell volume on device 0 for engine calls that the reference makes
// without a volume (greedySetCover): it only supplies the device and stream.
inline dmf_volume* service_volume() {
  static std::unique_ptr<dmf_volume, int (*)(dmf_volume*)> h(
      [] {
        dmf_volume* v = nullptr;
        dmf_check(dmf_volume_create(&v, 0));
        dmf_check(dmf_volume_set_dimensions(v, 0, 1, 0, 1, 0, 1));
        dmf_check(dmf_volume_set_volume_size(v, 1, 1, 1));
        dmf_check(dmf_volume_construct(v));
        return v;
      }(),
      dmf_volume_destroy);
  return h.get();
}
}  // namespace dmf_compat

namespace Algorithms {

// greedySetCover over arbitrary host sets on the device of `v`.
inline std::vector<unsigned long long int> greedySetCoverOn(dmf_volume* v,
                                                            std::vector<std::vector<unsigned long long int>>& candidate_sets) {
  std::unordered_map<unsigned long long int, int64_t> bit;
  for (auto& s : candidate_sets)
    for (auto h : s) bit.emplace(h, (int64_t)bit.size());
  const int32_t P = (int32_t)candidate_sets.size();
  const int64_t words = ((int64_t)bit.size() + 63) / 64;
  std::vector<uint64_t> masks((size_t)P * std::max<int64_t>(words, 1), 0);
  for (int32_t p = 0; p < P; ++p)
    for (auto h : candidate_sets[p]) {
      const int64_t i = bit[h];
      masks[(size_t)p * words + i / 64] |= 1ull << (i % 64);
    }
  void* d = nullptr;
  dmf_check(dmf_device_malloc(v, &d, sizeof(uint64_t) * masks.size()));
  std::vector<int32_t> sel(std::max(P, 1));
  int32_t n = 0;
  int st = dmf_memcpy_h2d(v, d, masks.data(), sizeof(uint64_t) * masks.size());
  if (st == DMF_OK) st = dmf_greedy_set_cover_masks_device(v, (const uint64_t*)d, P, words, 5, sel.data(), &n);
  dmf_device_free(v, d);
  dmf_check(st);
  return std::vector<unsigned long long int>(sel.begin(), sel.begin() + n);
}

// Algorithms.hpp:38-86, the reference signature (device 0)
inline std::vector<unsigned long long int> greedySetCover(std::vector<std::vector<unsigned long long int>>& candidate_sets,
                                                          double resolution = 0.000008) {
  (void)resolution;  // only feeds the reference's commented-out volume threshold
  return greedySetCoverOn(dmf_compat::service_volume(), candidate_sets);
}

// Extension: the same on `volume`'s device and stream.
inline std::vector<unsigned long long int> greedySetCover(VoxelVolume& volume,
                                                          std::vector<std::vector<unsigned long long int>>& candidate_sets,
                                                          double resolution = 0.000008) {
  (void)resolution;
  return greedySetCoverOn(volume.handle(), candidate_sets);
}

// ---- camera placement used by the reference drivers (Algorithms.hpp:114-122, 189-298) ----
// Not on the hot path; restated so tests/Raytracing.cpp:80-81 builds and runs unchanged.

// :114-122 movePointAway: pi + (float)distance * nor, summed in double
inline std::vector<double> movePointAway(std::vector<double> pi, std::vector<double> nor, double distance) {
  Eigen::Vector3f n(3);
  n << nor[0], nor[1], nor[2];
  n = n * distance;
  return {n(0) + pi[0], n(1) + pi[1], n(2) + pi[2]};
}

// :189-234 positionCamera(locations, id, distance): the camera `distance` mm out along the
// location's normal, looking back along it (z = -normal), with the reference's fixed
// x = (0, -1, 0), y = (1, 0, 0) columns (its computed orthogonal x, y are overwritten).
inline Eigen::Affine3f positionCamera(pcl::PointCloud<pcl::PointXYZRGBNormal>::Ptr locations, int id,
                                      unsigned int distance = 300) {
  const pcl::PointXYZRGBNormal pt = locations->points[id];
  Eigen::Vector3f nor(3);
  nor << pt.normal[0], pt.normal[1], pt.normal[2];
  const std::vector<double> normals = {nor(0), nor(1), nor(2)};
  nor = nor * -1;
  const std::vector<double> np = movePointAway({pt.x, pt.y, pt.z}, normals, double(distance) / 1000.0);
  const Eigen::Vector3f x(0, -1, 0), y(1, 0, 0);
  Eigen::Affine3f Q = Eigen::Affine3f::Identity();
  for (int i = 0; i < 3; i++) {
    Q(i, 0) = x(i);
    Q(i, 1) = y(i);
    Q(i, 2) = nor(i);
    Q(i, 3) = (float)np[i];
  }
  return Q;
}

// :236-279 positionCamera(location): camera AT the location, z = -normal, x orthogonal to
// it from the first non-zero normal component, y = z x x
inline Eigen::Affine3f positionCamera(pcl::PointXYZRGBNormal location) {
  Eigen::Vector3f nor(3);
  nor << location.normal[0], location.normal[1], location.normal[2];
  nor = nor * -1;
  Eigen::Vector3f x(3);
  if (nor(2) != 0.0) {
    x << 1, 1, 0;
    x(2) = -(nor(0) + nor(1)) / nor(2);
  } else if (nor(1) != 0) {
    x << 1, 0, 1;
    x(1) = -(nor(0) + nor(2)) / nor(1);
  } else if (nor(0) != 0) {
    x << 0, 1, 1;
    x(0) = -(nor(1) + nor(2)) / nor(0);
  }
  x = x.normalized();
  const Eigen::Vector3f y = nor.cross(x);
  Eigen::Affine3f Q = Eigen::Affine3f::Identity();
  for (int i = 0; i < 3; i++) {
    Q(i, 0) = x(i);
    Q(i, 1) = y(i);
    Q(i, 2) = nor(i);
  }
  Q(0, 3) = location.x;
  Q(1, 3) = location.y;
  Q(2, 3) = location.z;
  return Q;
}

// :281-298 positionCameras: normals with z <= 0 are flipped IN the locations cloud first
inline std::vector<Eigen::Affine3f> positionCameras(pcl::PointCloud<pcl::PointXYZRGBNormal>::Ptr locations,
                                                    unsigned int distance = 300) {
  std::vector<Eigen::Affine3f> cameras;
  for (size_t i = 0; i < locations->points.size(); i++) {
    if (locations->points[i].normal[2] <= 0)
      for (int a = 0; a < 3; ++a) locations->points[i].normal[a] *= -1;
    cameras.push_back(positionCamera(locations, (int)i, distance));
  }
  return cameras;
}
}  // namespace Algorithms

// The loop of tests/SetCover.cpp:218-240 (reverseRayTraceFast good sets of every
// candidate pose, then greedySetCover) as ONE batched visibility launch plus the GPU
// greedy.  (The reference defines setCover in its driver, so the drop-in does not.)
namespace dmf_compat {
inline std::vector<unsigned long long int> setCoverBatched(RayTracingEngine engine, VoxelVolume& volume,
                                                    std::vector<Eigen::Affine3f> camera_locations,
                                                    int resolution_single_dimension = 0, bool sparse = true) {
  (void)resolution_single_dimension;
  (void)sparse;
  std::vector<float> poses(12 * camera_locations.size());
  for (size_t i = 0; i < camera_locations.size(); ++i) dmf_compat::pose12(camera_locations[i], &poses[12 * i]);
  const dmf_camera c = engine.cam_.abi();
  std::vector<int32_t> sel(std::max<size_t>(camera_locations.size(), 1));
  int32_t n = 0;
  dmf_check(dmf_greedy_set_cover(volume.handle(), &c, poses.data(), (int32_t)camera_locations.size(), 5, sel.data(),
                                 &n));
  volume.touch();
  return std::vector<unsigned long long int>(sel.begin(), sel.begin() + n);
}

// ---- candidate views on the device (include/dmf.h: dmf_cloud_downsample, dmf_position_cameras,
// dmf_grid_surface_views).  The host code above and in <pcl/filters/voxel_grid.h> stays the truth:
// these give the same bits for xyz, the normals and the poses.  Colour and curvature are not
// carried: the filtered points hold 0 there.
using LocationCloud = pcl::PointCloud<pcl::PointXYZRGBNormal>;

inline std::vector<Eigen::Affine3f> poses_from12(const std::vector<float>& poses, size_t m) {
  std::vector<Eigen::Affine3f> cameras(m, Eigen::Affine3f::Identity());
  for (size_t i = 0; i < m; ++i)
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 4; ++c) cameras[i](r, c) = poses[12 * i + 4 * r + c];
  return cameras;
}
inline void locations_from(const std::vector<float>& xyz, const std::vector<float>& nrm, size_t m, LocationCloud& out) {
  out.points.assign(m, pcl::PointXYZRGBNormal());
  for (size_t i = 0; i < m; ++i) {
    pcl::PointXYZRGBNormal& p = out.points[i];
    p.x = xyz[3 * i]; p.y = xyz[3 * i + 1]; p.z = xyz[3 * i + 2];
    for (int a = 0; a < 3; ++a) p.normal[a] = nrm[3 * i + a];
  }
  out.width = (uint32_t)m;
  out.height = 1;
}

// PointCloudProcessing::downsample<pcl::PointXYZRGBNormal>(cloud, cloud_filtered, leaf) on the
// device of `volume` (which need not be constructed)
inline void downsampleOnDevice(VoxelVolume& volume, LocationCloud::Ptr cloud, LocationCloud::Ptr cloud_filtered,
                               double leaf) {
  const size_t n = cloud->points.size();
  std::vector<float> xyz(3 * n), nrm(3 * n);
  for (size_t i = 0; i < n; ++i) {
    const pcl::PointXYZRGBNormal& p = cloud->points[i];
    xyz[3 * i] = p.x; xyz[3 * i + 1] = p.y; xyz[3 * i + 2] = p.z;
    for (int a = 0; a < 3; ++a) nrm[3 * i + a] = p.normal[a];
  }
  const float l[3] = {(float)leaf, (float)leaf, (float)leaf};
  uint64_t cnt[3] = {0, 0, 0};
  dmf_check(dmf_cloud_downsample(volume.handle(), xyz.data(), nrm.data(), (int64_t)n, l, 0, nullptr, nullptr, nullptr, 0,
                                 cnt));
  const size_t m = (size_t)cnt[0];
  std::vector<float> oxyz(3 * m), onrm(3 * m);
  if (m)
    dmf_check(dmf_cloud_downsample(volume.handle(), xyz.data(), nrm.data(), (int64_t)n, l, 0, oxyz.data(), onrm.data(),
                                   nullptr, (int64_t)m, cnt));
  locations_from(oxyz, onrm, m, *cloud_filtered);
}

// Algorithms::positionCameras(locations, distance) on the device of `volume`; the flipped normals
// come back in `locations`, as the host code leaves them.  flip = false: the plain
// positionCamera(locations, i, distance) loop.
inline std::vector<Eigen::Affine3f> positionCamerasOnDevice(VoxelVolume& volume, LocationCloud::Ptr locations,
                                                            unsigned int distance = 300, bool flip = true) {
  const size_t m = locations->points.size();
  std::vector<float> xyz(3 * m), nrm(3 * m), poses(12 * m);
  for (size_t i = 0; i < m; ++i) {
    const pcl::PointXYZRGBNormal& p = locations->points[i];
    xyz[3 * i] = p.x; xyz[3 * i + 1] = p.y; xyz[3 * i + 2] = p.z;
    for (int a = 0; a < 3; ++a) nrm[3 * i + a] = p.normal[a];
  }
  dmf_check(dmf_position_cameras(volume.handle(), xyz.data(), nrm.data(), (int64_t)m, distance,
                                 flip ? 0u : DMF_PLACE_KEEP_NORMALS, poses.data()));
  for (size_t i = 0; i < m; ++i)
    for (int a = 0; a < 3; ++a) locations->points[i].normal[a] = nrm[3 * i + a];
  return poses_from12(poses, m);
}

// The fused grid's surface -> downsample(leaf) -> positionCameras(distance) in one call, the
// surface never leaving the device: the candidate locations into `locations`, the poses returned.
// `logodds` is the int16 grid of the constructed `volume` (x-major, as dmf_fuse_finalize writes it).
inline std::vector<Eigen::Affine3f> surfaceViews(VoxelVolume& volume, const std::vector<int16_t>& logodds,
                                                 LocationCloud::Ptr locations, double leaf, unsigned int distance = 300,
                                                 int occ_threshold = 1, int free_threshold = -1, bool flip = true) {
  const float l[3] = {(float)leaf, (float)leaf, (float)leaf};
  const uint32_t pf = flip ? 0u : DMF_PLACE_KEEP_NORMALS;
  uint64_t cnt[3] = {0, 0, 0};
  dmf_check(dmf_grid_surface_views(volume.handle(), logodds.data(), occ_threshold, free_threshold, l, 0, distance, pf,
                                   nullptr, nullptr, nullptr, 0, cnt));
  const size_t m = (size_t)cnt[0];
  std::vector<float> poses(12 * m), xyz(3 * m), nrm(3 * m);
  if (m)
    dmf_check(dmf_grid_surface_views(volume.handle(), logodds.data(), occ_threshold, free_threshold, l, 0, distance, pf,
                                     poses.data(), xyz.data(), nrm.data(), (int64_t)m, cnt));
  locations_from(xyz, nrm, m, *locations);
  return poses_from12(poses, m);
}
}  // namespace dmf_compat
