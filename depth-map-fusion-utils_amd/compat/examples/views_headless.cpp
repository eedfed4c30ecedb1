// views_headless — the candidate poses of the reference's planners by two routes over the drop-in
// headers: the host route every driver takes (PointCloudProcessing::downsample, PCL's VoxelGrid,
// then Algorithms::positionCameras: tests/SetCover.cpp:280, CameraPathGen.cpp:85-92) and the device
// route (dmf_compat::downsampleOnDevice, dmf_compat::positionCamerasOnDevice).  Prints whether
// the locations, their normals and the poses agree bit for bit, a digest (FNV-1a over those words
// of the device route), the leaf statistics and both times.
// usage: views_headless [cloud.pcd | --synthetic N SEED] [leaf = 0.1] [distance_mm = 300]
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include <pcl/io/pcd_io.h>
#include <pcl/point_cloud.h>
#include <pcl/point_types.h>

#include "Algorithms.hpp"
#include "PointCloudProcessing.hpp"

using Cloud = pcl::PointCloud<pcl::PointXYZRGBNormal>;

// An oriented cloud on a unit sphere's upper and lower halves around (0.3, -0.2, 0.5), from a
// 64-bit LCG: outward normals, so that about half of them face down.
static void synthetic(Cloud& c, size_t n, uint64_t seed) {
  uint64_t s = seed * 6364136223846793005ull + 1442695040888963407ull;
  auto u = [&] {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(s >> 11) / 9007199254740992.0;
  };
  c.points.resize(n);
  for (auto& p : c.points) {
    double d[3], q;
    do {
      for (double& e : d) e = 2.0 * u() - 1.0;
      q = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
    } while (q < 1e-3 || q > 1.0);
    q = std::sqrt(q);
    p.x = (float)(0.3 + d[0] / q);
    p.y = (float)(-0.2 + d[1] / q);
    p.z = (float)(0.5 + d[2] / q);
    for (int a = 0; a < 3; ++a) p.normal[a] = (float)(d[a] / q);
  }
  c.width = (uint32_t)n;
  c.height = 1;
}

static void words(const Cloud& loc, const std::vector<Eigen::Affine3f>& cams, std::vector<uint32_t>& w) {
  auto put = [&](float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    w.push_back(u);
  };
  for (const auto& p : loc.points) {
    put(p.x); put(p.y); put(p.z);
    for (int a = 0; a < 3; ++a) put(p.normal[a]);
  }
  for (const auto& q : cams)
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 4; ++c) put(q(r, c));
}

int main(int argc, char** argv) {
  Cloud::Ptr cloud(new Cloud);
  int k = 1;
  if (argc > 1 && std::string(argv[1]) == "--synthetic") {
    if (argc < 4) {
      std::fprintf(stderr, "usage: %s [cloud.pcd | --synthetic N SEED] [leaf] [distance_mm]\n", argv[0]);
      return 2;
    }
    synthetic(*cloud, (size_t)std::atoll(argv[2]), (uint64_t)std::atoll(argv[3]));
    k = 4;
  } else if (argc > 1) {
    if (pcl::io::loadPCDFile<pcl::PointXYZRGBNormal>(std::string(argv[1]), *cloud) == -1) {
      std::fprintf(stderr, "cannot read %s\n", argv[1]);
      return 3;
    }
    k = 2;
  } else {
    synthetic(*cloud, 20000, 1);
  }
  const double leaf = argc > k ? std::atof(argv[k]) : 0.1;
  const unsigned distance = argc > k + 1 ? (unsigned)std::atoi(argv[k + 1]) : 300u;
  using clk = std::chrono::steady_clock;
  auto ms = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
  try {
    VoxelVolume volume;  // only its device and stream are used: no geometry
    Cloud::Ptr warm(new Cloud), host(new Cloud), dev(new Cloud);
    dmf_compat::downsampleOnDevice(volume, cloud, warm, leaf);  // (the first call creates the scratch)

    const auto t0 = clk::now();
    PointCloudProcessing::downsample<pcl::PointXYZRGBNormal>(cloud, host, leaf);
    const std::vector<Eigen::Affine3f> hc = Algorithms::positionCameras(host, distance);
    const auto t1 = clk::now();
    dmf_compat::downsampleOnDevice(volume, cloud, dev, leaf);
    const std::vector<Eigen::Affine3f> dc = dmf_compat::positionCamerasOnDevice(volume, dev, distance);
    const auto t2 = clk::now();

    std::vector<uint32_t> hw, dw;
    words(*host, hc, hw);
    words(*dev, dc, dw);
    uint64_t h = 1469598103934665603ull;
    for (uint32_t u : dw)
      for (int b = 0; b < 4; ++b) h = (h ^ ((u >> (8 * b)) & 0xffu)) * 1099511628211ull;
    const float l[3] = {(float)leaf, (float)leaf, (float)leaf};
    uint64_t cnt[3] = {0, 0, 0};
    std::vector<float> xyz(3 * cloud->points.size());
    for (size_t i = 0; i < cloud->points.size(); ++i) {
      xyz[3 * i] = cloud->points[i].x; xyz[3 * i + 1] = cloud->points[i].y; xyz[3 * i + 2] = cloud->points[i].z;
    }
    dmf_check(dmf_cloud_downsample(volume.handle(), xyz.data(), nullptr, (int64_t)cloud->points.size(), l, 0, nullptr,
                                   nullptr, nullptr, 0, cnt));
    std::printf("points %zu leaf %g distance_mm %u\n", cloud->points.size(), leaf, distance);
    std::printf("views host %zu device %zu\n", hc.size(), dc.size());
    std::printf("bitwise %s\n", hw == dw ? "equal" : "DIFFERENT");
    std::printf("digest %016llx\n", (unsigned long long)h);
    std::printf("leaves %llu finite %llu mean_population %.3f max_population %llu\n", (unsigned long long)cnt[0],
                (unsigned long long)cnt[1], cnt[0] ? (double)cnt[1] / (double)cnt[0] : 0.0, (unsigned long long)cnt[2]);
    std::printf("host_ms %.3f device_ms %.3f\n", ms(t0, t1), ms(t1, t2));
    return hw == dw ? 0 : 1;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "views_headless: %s\n", e.what());
    return 4;
  }
}
