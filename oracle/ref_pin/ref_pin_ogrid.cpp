// ref_pin_ogrid — runs the reference's OccupancyGrid on one scene file and writes its dense
// state and its four downloads to a result file (formats: tests/ref_pin.py).  Built only
// against a checkout of the reference (oracle/Makefile ref_pin), in a translation unit of its
// own because OccupancyGrid.hpp defines another struct Voxel than Volume.hpp, and without
// OpenMP, so that the loops the reference races over run in their sequential order.
// The header is included by name; nothing of it is restated here.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <OccupancyGrid.hpp>

namespace {

template <class T>
std::vector<T> many(FILE* f, size_t n) {
  std::vector<T> v(n);
  if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "ref_pin: short scene file\n"); exit(2); }
  return v;
}

template <class T>
void put(FILE* f, const std::string& name, uint32_t code, const std::vector<T>& a) {
  const uint32_t len = (uint32_t)name.size();
  const uint64_t bytes = (uint64_t)a.size() * sizeof(T);
  fwrite(&len, 4, 1, f);
  fwrite(name.data(), 1, len, f);
  fwrite(&code, 4, 1, f);
  fwrite(&bytes, 8, 1, f);
  if (bytes) fwrite(a.data(), 1, bytes, f);
}

std::vector<float> rows(const pcl::PointCloud<pcl::PointXYZRGBNormal>::Ptr& c) {
  std::vector<float> a;
  for (const auto& p : c->points) {
    a.push_back(p.x); a.push_back(p.y); a.push_back(p.z);
    a.push_back(p.normal[0]); a.push_back(p.normal[1]); a.push_back(p.normal[2]);
  }
  return a;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: %s scene.bin result.bin\n", argv[0]); return 2; }
  FILE* fi = fopen(argv[1], "rb");
  if (!fi) { perror(argv[1]); return 2; }
  if (std::memcmp(many<char>(fi, 8).data(), "DMFPIN02", 8) != 0) { fprintf(stderr, "ref_pin: bad magic\n"); return 2; }
  const std::vector<double> b = many<double>(fi, 6);
  const std::vector<float> res = many<float>(fi, 3);
  const int32_t k = many<int32_t>(fi, 1)[0];
  const int32_t n = many<int32_t>(fi, 1)[0];
  const std::vector<float> cloud = many<float>(fi, 3 * (size_t)n);
  const int32_t m = many<int32_t>(fi, 1)[0];
  const std::vector<float> nrm = many<float>(fi, 6 * (size_t)m);
  const int32_t n_first = many<int32_t>(fi, 1)[0];  // the first updateStates call takes this many of each
  fclose(fi);

  OccupancyGrid g;
  g.setDimensions(b[0], b[1], b[2], b[3], b[4], b[5]);
  g.setResolution(res[0], res[1], res[2]);
  g.setK(k);
  g.construct();
  for (int part = 0; part < 2; ++part) {  // two calls: the state persists
    pcl::PointCloud<pcl::PointXYZRGB>::Ptr c(new pcl::PointCloud<pcl::PointXYZRGB>());
    pcl::PointCloud<pcl::PointNormal>::Ptr pn(new pcl::PointCloud<pcl::PointNormal>());
    for (int i = part ? n_first : 0; i < (part ? n : (n_first < n ? n_first : n)); ++i) {
      pcl::PointXYZRGB p;
      p.x = cloud[3 * i]; p.y = cloud[3 * i + 1]; p.z = cloud[3 * i + 2];
      c->points.push_back(p);
    }
    for (int i = part ? n_first : 0; i < (part ? m : (n_first < m ? n_first : m)); ++i) {
      pcl::PointNormal p;
      p.x = nrm[6 * i]; p.y = nrm[6 * i + 1]; p.z = nrm[6 * i + 2];
      for (int a = 0; a < 3; ++a) p.normal[a] = nrm[6 * i + 3 + a];
      pn->points.push_back(p);
    }
    g.updateStates(c, pn);
  }

  FILE* fo = fopen(argv[2], "wb");
  if (!fo) { perror(argv[2]); return 2; }
  put(fo, "og_dims", 1, std::vector<int32_t>{g.xdim_, g.ydim_, g.zdim_});
  std::vector<float> sn, sc;
  std::vector<int32_t> cnt;
  std::vector<uint8_t> fl;
  for (int x = 0; x < g.xdim_; ++x)
    for (int y = 0; y < g.ydim_; ++y)
      for (int z = 0; z < g.zdim_; ++z) {
        const Voxel& v = g.voxels_[x][y][z];
        for (int a = 0; a < 3; ++a) { sn.push_back(v.normal(a)); sc.push_back(v.centroid(a)); }
        cnt.push_back(v.count);
        fl.push_back((uint8_t)((v.occupied ? 1 : 0) | (v.normal_found ? 2 : 0)));
      }
  put(fo, "og_normal", 4, sn);
  put(fo, "og_centroid", 4, sc);
  put(fo, "og_count", 1, cnt);
  put(fo, "og_flags", 0, fl);
  const char* names[4] = {"og_cloud", "og_hq", "og_reorg", "og_reorg_clean"};
  for (int mode = 0; mode < 4; ++mode) {
    pcl::PointCloud<pcl::PointXYZRGBNormal>::Ptr out(new pcl::PointCloud<pcl::PointXYZRGBNormal>());
    if (mode == 0) g.downloadCloud(out);
    else if (mode == 1) g.downloadHQCloud(out);
    else g.downloadReorganizedCloud(out, mode == 3);
    put(fo, names[mode], 4, rows(out));
  }
  if (fclose(fo) != 0) { perror(argv[2]); return 2; }
  return 0;
}
