// Headless PCD pipelines over the drop-in headers in compat/, self-contained counterparts of the
// two reference drivers tests/Raytracing.cpp and tests/SetCover.cpp: the same library calls in
// the same order (readPointCloud, pcl::getMinMax3D, VoxelVolume setup + integratePointCloud,
// downsample + positionCameras, reverseRayTraceFast, greedySetCover, writeCameraLocations, the
// viewer wrapper), so that the -m gpu suite exercises that whole surface on a checkout that has
// no reference tree beside it.
//   pcd_pipeline_headless visibility cloud.pcd
//       volume at 125 voxels per metre, camera 0 of positionCameras(downsample(cloud, 0.3)),
//       reverseRayTraceFast(camera 0, viz = true), addVolumeWithVoxelsClassified (its dump goes
//       to $DMF_COMPAT_VIZ_DUMP)
//   pcd_pipeline_headless setcover cloud.pcd selected.txt
//       on a VizThread's input thread: volume at 63 voxels per metre, the cameras of
//       positionCameras(downsample(cloud, 0.1), 500) with z >= 0, each camera's sorted good set,
//       greedySetCover, writeCameraLocations of the selected cameras
#include <algorithm>
#include <cmath>
#include <iostream>
#include <string>
#include <tuple>
#include <vector>

#include <pcl/common/common.h>

#include "Algorithms.hpp"
#include "Camera.hpp"
#include "FileRoutines.hpp"
#include "PointCloudProcessing.hpp"
#include "RayTracingEngine.hpp"
#include "VisualizationUtilities.hpp"
#include "Volume.hpp"

using Cloud = pcl::PointCloud<pcl::PointXYZRGBNormal>;

// (not const: Camera takes it by non-const reference)
static std::vector<float> kIntrinsics = {602.39306640625, 0.0, 314.6370849609375, 0.0, 602.39306640625,
                                         245.04962158203125, 0.0, 0.0, 1.0};

struct Scene {
  Cloud::Ptr cloud_normal{new Cloud};
  pcl::PointCloud<pcl::PointXYZRGB>::Ptr cloud{new pcl::PointCloud<pcl::PointXYZRGB>};
  pcl::PointCloud<pcl::Normal>::Ptr normals{new pcl::PointCloud<pcl::Normal>};
};

// the cloud's bounding box as the volume, `per_metre` voxels per metre on each axis
static void integrate(Scene& s, VoxelVolume& volume, const std::string& pcd, double per_metre) {
  readPointCloud(pcd, s.cloud_normal, s.cloud, s.normals);
  pcl::PointXYZRGB lo, hi;
  pcl::getMinMax3D<pcl::PointXYZRGB>(*s.cloud, lo, hi);
  volume.setDimensions(lo.x, hi.x, lo.y, hi.y, lo.z, hi.z);
  const double nx = (hi.x - lo.x) * per_metre, ny = (hi.y - lo.y) * per_metre, nz = (hi.z - lo.z) * per_metre;
  volume.setVolumeSize(int(nx), int(ny), int(nz));
  volume.constructVolume();
  volume.integratePointCloud(s.cloud, s.normals);
  std::cout << "integrated " << volume.occupied_cells_.size() << " voxels of " << volume.xdim_ << " x " << volume.ydim_
            << " x " << volume.zdim_ << std::endl;
}

static std::vector<Eigen::Affine3f> cameras(Scene& s, double leaf, int distance_mm) {
  Cloud::Ptr locations(new Cloud);
  PointCloudProcessing::downsample<pcl::PointXYZRGBNormal>(s.cloud_normal, locations, leaf);
  return Algorithms::positionCameras(locations, distance_mm);
}

static int visibility(const std::string& pcd) {
  Scene s;
  VoxelVolume volume;
  integrate(s, volume, pcd, 125);
  auto poses = cameras(s, 0.3, 300);
  Camera cam(kIntrinsics);
  const int side = int(std::round(std::cbrt(volume.voxel_size_ * 1e9)));
  VisualizationUtilities::PCLVisualizerWrapper viz;
  viz.addCoordinateSystem();
  viz.addCamera(cam, poses[0], "camera", 2000);
  RayTracingEngine engine(cam);
  auto res = engine.reverseRayTraceFast(volume, poses[0], true, side);
  std::cout << "camera 0 of " << poses.size() << ": " << res.second.size() << " good voxels" << std::endl;
  viz.addVolumeWithVoxelsClassified(volume);
  viz.spinViewer();
  return 0;
}

class SetCoverRun : public VizThread {
  std::string pcd_, out_;
  VoxelVolume volume_;

  void input() override {
    Scene s;
    integrate(s, volume_, pcd_, 63);
    std::vector<Eigen::Affine3f> poses;
    for (const auto& T : cameras(s, 0.1, 500))
      if (!(T(2, 3) < 0)) poses.push_back(T);
    Camera cam(kIntrinsics);
    RayTracingEngine engine(cam);
    std::vector<std::vector<unsigned long long int>> covered;
    for (auto& T : poses) {
      bool found;
      std::vector<unsigned long long int> good;
      std::tie(found, good) = engine.reverseRayTraceFast(volume_, T, false);
      std::sort(good.begin(), good.end());
      covered.push_back(good);
    }
    auto selected = Algorithms::greedySetCover(covered);
    std::cout << "Total Cameras: " << poses.size() << std::endl;
    std::cout << "Cameras found: " << selected.size() << std::endl;
    std::vector<Eigen::Affine3f> keep;
    for (auto i : selected) keep.push_back(poses[i]);
    writeCameraLocations(out_, keep);
    updateViewer();
  }

 public:
  SetCoverRun(std::string pcd, std::string out) : pcd_(std::move(pcd)), out_(std::move(out)) {}
};

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "visibility" && argc == 3) return visibility(argv[2]);
  if (mode == "setcover" && argc == 4) {
    SetCoverRun run(argv[2], argv[3]);
    run.makeThreads();
    return 0;
  }
  std::cerr << "usage: " << argv[0] << " visibility cloud.pcd | setcover cloud.pcd selected.txt\n";
  return 2;
}
