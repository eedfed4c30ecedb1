// Headless driver of the OccupancyGrid drop-in (compat/OccupancyGrid.hpp), written against it
// as reference code is written against include/OccupancyGrid.hpp: setDimensions, setResolution,
// setK, construct, updateStates, then the four downloads.  All I/O is raw float32:
//   cloud.bin    x y z per point            (the PointXYZRGB cloud)
//   normals.bin  x y z nx ny nz per point   (the PointNormal cloud)
//   PREFIX.cloud / .hq / .reorg / .clean    x y z nx ny nz per downloaded point (downloadCloud,
//                downloadHQCloud, downloadReorganizedCloud(false), downloadReorganizedCloud(true))
// usage: ogrid_headless cloud.bin normals.bin xmin xmax ymin ymax zmin zmax xres yres zres K PREFIX
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <memory>
#include <string>
#include <vector>

#include "OccupancyGrid.hpp"

using namespace std;

static vector<float> readFloats(const string& path) {
  ifstream f(path, ios::binary | ios::ate);
  if (!f) {
    cerr << "cannot read " << path << "\n";
    exit(3);
  }
  const streamsize bytes = f.tellg();
  vector<float> v((size_t)bytes / sizeof(float));
  f.seekg(0);
  f.read(reinterpret_cast<char*>(v.data()), (streamsize)(v.size() * sizeof(float)));
  return v;
}

static void writeCloud(const string& path, const pcl::PointCloud<pcl::PointXYZRGBNormal>& c) {
  vector<float> v;
  v.reserve(6 * c.points.size());
  for (const auto& p : c.points) {
    v.push_back(p.x); v.push_back(p.y); v.push_back(p.z);
    v.push_back(p.normal[0]); v.push_back(p.normal[1]); v.push_back(p.normal[2]);
  }
  ofstream o(path, ios::binary);
  o.write(reinterpret_cast<const char*>(v.data()), (streamsize)(v.size() * sizeof(float)));
}

int main(int argc, char** argv) {
  if (argc != 14) {
    cerr << "usage: " << argv[0] << " cloud.bin normals.bin xmin xmax ymin ymax zmin zmax xres yres zres K PREFIX\n";
    return 2;
  }
  const vector<float> c = readFloats(argv[1]), n = readFloats(argv[2]);
  pcl::PointCloud<pcl::PointXYZRGB>::Ptr cloud(new pcl::PointCloud<pcl::PointXYZRGB>);
  pcl::PointCloud<pcl::PointNormal>::Ptr normals(new pcl::PointCloud<pcl::PointNormal>);
  for (size_t i = 0; i + 3 <= c.size(); i += 3) {
    pcl::PointXYZRGB p;
    p.x = c[i]; p.y = c[i + 1]; p.z = c[i + 2];
    cloud->points.push_back(p);
  }
  for (size_t i = 0; i + 6 <= n.size(); i += 6) {
    pcl::PointNormal p;
    p.x = n[i]; p.y = n[i + 1]; p.z = n[i + 2];
    p.normal[0] = n[i + 3]; p.normal[1] = n[i + 4]; p.normal[2] = n[i + 5];
    normals->points.push_back(p);
  }
  OccupancyGrid grid;
  grid.setDimensions(strtod(argv[3], nullptr), strtod(argv[4], nullptr), strtod(argv[5], nullptr),
                     strtod(argv[6], nullptr), strtod(argv[7], nullptr), strtod(argv[8], nullptr));
  grid.setResolution(strtof(argv[9], nullptr), strtof(argv[10], nullptr), strtof(argv[11], nullptr));
  grid.setK(atoi(argv[12]));
  grid.construct();
  cout << "dims " << grid.xdim_ << " " << grid.ydim_ << " " << grid.zdim_ << "\n";
  grid.updateStates(cloud, normals);
  const string prefix = argv[13];
  const char* names[4] = {".cloud", ".hq", ".reorg", ".clean"};
  for (int m = 0; m < 4; ++m) {
    pcl::PointCloud<pcl::PointXYZRGBNormal>::Ptr out(new pcl::PointCloud<pcl::PointXYZRGBNormal>);
    if (m == 0) grid.downloadCloud(out);
    else if (m == 1) grid.downloadHQCloud(out);
    else grid.downloadReorganizedCloud(out, m == 3);
    cout << (names[m] + 1) << " " << out->points.size() << "\n";
    writeCloud(prefix + names[m], *out);
  }
  return 0;
}
