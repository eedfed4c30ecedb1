// Headless driver of the cloud error (compat/ErrorCalc.hpp): the reference's tests/ErrorCalc.cpp
// without its viewer types -- load two PCD files (:63-70), find every point's nearest neighbour in
// the second cloud, print the reference's two lines (:96-97) in its formatting, and write the
// per-point distances (sqrt(dist[0]) of :82) as raw float32 in place of the coloured cloud (:101).
// usage: cloud_error_headless cloud.pcd cloud_ref.pcd distances.bin
#include <fstream>
#include <iostream>
#include <string>

#include <pcl/io/pcd_io.h>
#include <pcl/point_cloud.h>
#include <pcl/point_types.h>

#include "ErrorCalc.hpp"

using namespace std;

int main(int argc, char** argv) {
  if (argc != 4) {
    cerr << "usage: " << argv[0] << " cloud.pcd cloud_ref.pcd distances.bin\n";
    return 2;
  }
  pcl::PointCloud<pcl::PointXYZ> cloud, cloud_ref;
  for (int k = 0; k < 2; ++k)
    if (pcl::io::loadPCDFile<pcl::PointXYZ>(string(argv[1 + k]), k ? cloud_ref : cloud) == -1) {
      cerr << "cannot read " << argv[1 + k] << "\n";
      return 3;
    }
  const ErrorCalc::CloudError e = ErrorCalc::cloudError(cloud, cloud_ref);
  std::cout << "The max error is : " << e.max_error << std::endl;
  std::cout << "The avg error is : " << e.avg_error << std::endl;
  ofstream o(argv[3], ios::binary);
  o.write(reinterpret_cast<const char*>(e.distance.data()), (streamsize)(e.distance.size() * sizeof(float)));
  return o ? 0 : 4;
}
