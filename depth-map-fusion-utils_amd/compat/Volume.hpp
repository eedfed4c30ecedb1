// Volume.hpp — drop-in for the reference include/Volume.hpp:29-255 over the MI355X
// engine.  Same struct Voxel, same VoxelVolume member functions and public fields.
//
// The grid lives on the GPU (flat occupancy bitmask + slot map + CSR points/normals,
// DESIGN.md §6).  The public fields the reference's callers read directly are kept in
// sync: the geometry fields after every setup call, occupied_cells_ after every
// integration, and voxels_[x][y][z] (Voxel*) through a host mirror that is rebuilt
// lazily from the device whenever the device state changed (engine calls with viz
// flags, integration).  Copying is disabled, as a copy of the reference double-frees.
#pragma once
#include <array>
#include <cmath>
#include <cstdint>
#include <memory>
#include <stdexcept>
#include <string>
#include <tuple>
#include <vector>

#include "dmf.h"
#include "dmf_types.hpp"

// Volume.hpp:29-48
struct Voxel {
  std::vector<pcl::PointXYZRGB> pts;
  std::vector<pcl::Normal> normals;
  int view = 0;
  bool good = false;
  Voxel() = default;
  explicit Voxel(pcl::PointXYZRGB pt) { pts.push_back(pt); }
  Voxel(pcl::PointXYZRGB pt, pcl::Normal n) { pts.push_back(pt); normals.push_back(n); }
};

inline void dmf_check(int status) {
  if (status != DMF_OK) throw std::runtime_error(std::string("dmf: ") + dmf_status_string(status) + ": " + dmf_last_error());
}

class VoxelVolume {
 public:
  // Volume.hpp:54-61 public fields
  std::vector<unsigned long long int> occupied_cells_;
  double xmin_ = 0, xmax_ = 0, ymin_ = 0, ymax_ = 0, zmin_ = 0, zmax_ = 0;
  double xcenter_ = 0, ycenter_ = 0, zcenter_ = 0;
  double xdelta_ = 0, ydelta_ = 0, zdelta_ = 0;
  double voxel_size_ = 0;
  int xdim_ = 0, ydim_ = 0, zdim_ = 0;
  unsigned long long int hsize_ = 0;

  // voxels_[x][y][z] -> Voxel* (nullptr if empty), served from the lazily rebuilt mirror
  struct ZRow {
    VoxelVolume* v;
    int x, y;
    Voxel* operator[](int z) const { return v->mirror_at(x, y, z); }
  };
  struct YRow {
    VoxelVolume* v;
    int x;
    ZRow operator[](int y) const { return ZRow{v, x, y}; }
  };
  struct Grid {
    VoxelVolume* v;
    YRow operator[](int x) const { return YRow{v, x}; }
  } voxels_{this};

  explicit VoxelVolume(int device = 0) { dmf_check(dmf_volume_create(&h_, device)); }
  ~VoxelVolume() { dmf_volume_destroy(h_); }
  VoxelVolume(const VoxelVolume&) = delete;
  VoxelVolume& operator=(const VoxelVolume&) = delete;

  // Volume.hpp:89-128
  void setDimensions(double xmin, double xmax, double ymin, double ymax, double zmin, double zmax) {
    dmf_check(dmf_volume_set_dimensions(h_, xmin, xmax, ymin, ymax, zmin, zmax));
    pull_info();
  }
  void setResolution(double xdelta, double ydelta, double zdelta) {
    dmf_check(dmf_volume_set_resolution(h_, xdelta, ydelta, zdelta));
    pull_info();
  }
  void setVolumeSize(int xdim, int ydim, int zdim) {
    dmf_check(dmf_volume_set_volume_size(h_, xdim, ydim, zdim));
    pull_info();
  }
  bool constructVolume() {
    dmf_check(dmf_volume_construct(h_));
    pull_info();
    occupied_cells_.clear();
    touch();
    return true;
  }
  template <typename PointT>
  bool addPointCloud(typename pcl::PointCloud<PointT>::Ptr) { return true; }  // Volume.hpp:130-133 stub

  // Volume.hpp:135-170 helpers (host formulas)
  unsigned long long int getHash(float x, float y, float z) {
    int a, b, c;
    std::tie(a, b, c) = getVoxel(x, y, z);
    return getHashId(a, b, c);
  }
  unsigned long long int getHashId(int x, int y, int z) {
    unsigned long long int hash = x;
    return (hash << 40) ^ (unsigned long long int)(long long)(y << 20) ^ (unsigned long long int)(long long)z;
  }
  std::tuple<int, int, int> getVoxel(float x, float y, float z) {
    return std::make_tuple((int)std::floor((x - xmin_) / xdelta_), (int)std::floor((y - ymin_) / ydelta_),
                           (int)std::floor((z - zmin_) / zdelta_));
  }
  std::tuple<int, int, int> getVoxelCoords(unsigned long long int id) {
    const unsigned long long int mask = (1 << 20) - 1;
    return std::make_tuple((int)(id >> 40), (int)(id >> 20 & mask), (int)(id & mask));
  }
  bool validCoords(int x, int y, int z) { return x < xdim_ && y < ydim_ && z < zdim_ && x >= 0 && y >= 0 && z >= 0; }
  bool validPoints(float x, float y, float z) {
    return !(x >= xmax_ || y >= ymax_ || z >= zmax_ || x <= xmin_ || y <= ymin_ || z <= zmin_);
  }

  // Volume.hpp:172-197 / 199-228 — binning on the GPU
  bool integratePointCloud(pcl::PointCloud<pcl::PointXYZRGB>::Ptr cloud) { return integrate(cloud, nullptr); }
  bool integratePointCloud(pcl::PointCloud<pcl::PointXYZRGB>::Ptr cloud, pcl::PointCloud<pcl::Normal>::Ptr normals) {
    return integrate(cloud, normals.get());
  }

  // Surface of a fused log-odds grid (dmf_grid_surface; not in the reference): the
  // cells with L >= occ that have a face neighbour with L <= free, in ascending getHashId, as
  // voxel centres with normals towards free space.  The volume's occupancy is not touched.
  void extractSurface(const std::vector<int16_t>& L, int occ, int free, std::vector<unsigned long long int>& cells,
                      pcl::PointCloud<pcl::PointNormal>& out) {
    if (L.size() != (size_t)xdim_ * ydim_ * zdim_) throw std::invalid_argument("extractSurface: grid size");
    int64_t n = 0;
    dmf_check(dmf_grid_surface(h_, L.data(), occ, free, nullptr, nullptr, nullptr, 0, &n, nullptr));
    cells.assign((size_t)n, 0);
    std::vector<float> xyz(3 * (size_t)n), nrm(3 * (size_t)n);
    if (n)
      dmf_check(dmf_grid_surface(h_, L.data(), occ, free, reinterpret_cast<uint64_t*>(cells.data()), xyz.data(),
                                 nrm.data(), n, &n, nullptr));
    out.points.resize((size_t)n);
    for (size_t i = 0; i < (size_t)n; ++i) {
      pcl::PointNormal& p = out.points[i];
      p.x = xyz[3 * i]; p.y = xyz[3 * i + 1]; p.z = xyz[3 * i + 2];
      for (int k = 0; k < 3; ++k) p.normal[k] = nrm[3 * i + k];
    }
  }
  // extractSurface's cloud into integratePointCloud(cloud, normals) without leaving the device:
  // the number of surface cells.
  long long integrateSurface(const std::vector<int16_t>& L, int occ, int free) {
    if (L.size() != (size_t)xdim_ * ydim_ * zdim_) throw std::invalid_argument("integrateSurface: grid size");
    int64_t n = 0;
    dmf_check(dmf_volume_integrate_surface(h_, L.data(), occ, free, &n));
    pull_occupied();
    return (long long)n;
  }

  // Distance field of a fused log-odds grid (dmf_grid_distance; not in the
  // reference): out[(x * ydim_ + y) * zdim_ + z] = the squared distance, in cells, to the nearest
  // cell with L >= threshold; DMF_NO_DIST everywhere when there is none.
  void distanceField(const std::vector<int16_t>& L, int threshold, std::vector<uint32_t>& out) {
    if (L.size() != (size_t)xdim_ * ydim_ * zdim_) throw std::invalid_argument("distanceField: grid size");
    out.assign(L.size(), 0);
    dmf_check(dmf_grid_distance(h_, L.data(), threshold, out.data(), nullptr));
  }
  // The least dist2 over the cells of each segment a[i] -> b[i] (the cells the ray origin a[i],
  // point b[i] updates in the point fusion); DMF_NO_DIST for a segment that visits no cell.
  std::vector<uint32_t> segmentClearance(const std::vector<uint32_t>& dist2, const std::vector<Eigen::Vector3f>& a,
                                         const std::vector<Eigen::Vector3f>& b) {
    if (dist2.size() != (size_t)xdim_ * ydim_ * zdim_) throw std::invalid_argument("segmentClearance: field size");
    if (a.size() != b.size()) throw std::invalid_argument("segmentClearance: a and b differ in length");
    std::vector<float> pa(3 * a.size()), pb(3 * b.size());
    for (size_t i = 0; i < a.size(); ++i)
      for (int k = 0; k < 3; ++k) {
        pa[3 * i + k] = a[i](k);
        pb[3 * i + k] = b[i](k);
      }
    std::vector<uint32_t> out(a.size(), 0);
    if (!a.empty())
      dmf_check(dmf_grid_clearance(h_, dist2.data(), pa.data(), pb.data(), (int64_t)a.size(), out.data()));
    return out;
  }

  // Travel field over a distance field (dmf_grid_travel; not in the reference):
  // out[(x * ydim_ + y) * zdim_ + z] = the least number of face-to-face steps from any seed cell
  // {x, y, z} through cells with dist2 >= radius2; DMF_NO_PATH where a cell is blocked or not
  // reachable.  Returns {traversable cells, reached cells, largest finite hop count}.
  std::array<uint64_t, 3> travelField(const std::vector<uint32_t>& dist2, uint32_t radius2,
                                      const std::vector<std::array<int32_t, 3>>& seeds, std::vector<uint32_t>& out) {
    if (dist2.size() != (size_t)xdim_ * ydim_ * zdim_) throw std::invalid_argument("travelField: field size");
    out.assign(dist2.size(), 0);
    std::array<uint64_t, 3> info{{0, 0, 0}};
    dmf_check(dmf_grid_travel(h_, dist2.data(), radius2, seeds.empty() ? nullptr : seeds[0].data(),
                              (int64_t)seeds.size(), out.data(), info.data()));
    return info;
  }
  // The path target, ..., seed in a field of travelField (hops[target] + 1 cells, ties to the
  // first of -x +x -y +y -z +z); empty for a target outside the grid or with DMF_NO_PATH.
  std::vector<std::array<int32_t, 3>> pathTo(const std::vector<uint32_t>& hops, const std::array<int32_t, 3>& target) {
    if (hops.size() != (size_t)xdim_ * ydim_ * zdim_) throw std::invalid_argument("pathTo: field size");
    int64_t n = 0;
    dmf_check(dmf_grid_path(h_, hops.data(), target.data(), nullptr, 0, &n));
    std::vector<std::array<int32_t, 3>> cells((size_t)n);
    if (n) dmf_check(dmf_grid_path(h_, hops.data(), target.data(), cells[0].data(), n, &n));
    return cells;
  }

  // Volume.hpp:235-255 (with the reference's `i==j==k==0` test)
  std::vector<unsigned long long int> getNeighborHashes(unsigned long long int hash, int K = 1) {
    int x, y, z;
    std::tie(x, y, z) = getVoxelCoords(hash);
    std::vector<unsigned long long int> out;
    for (int i = -K; i <= K; i++)
      for (int j = -K; j <= K; j++)
        for (int k = -K; k <= K; k++) {
          if (((i == j) == k) == 0) continue;
          if (validCoords(x + i, y + j, z + k) && voxels_[x + i][y + j][z + k] != nullptr)
            out.push_back(getHashId(x + i, y + j, z + k));
        }
    return out;
  }

  dmf_volume* handle() { return h_; }
  // Called by the engine after GPU calls that may change per-voxel flags.
  void touch() { ++version_; }

 private:
  dmf_volume* h_ = nullptr;
  uint64_t version_ = 1, mirror_version_ = 0;
  std::vector<std::unique_ptr<Voxel>> store_;
  std::vector<int32_t> slot_of_;  // dense x-major -> slot index or -1

  void pull_info() {
    dmf_volume_info i;
    dmf_check(dmf_volume_get_info(h_, &i));
    xmin_ = i.xmin; xmax_ = i.xmax; ymin_ = i.ymin; ymax_ = i.ymax; zmin_ = i.zmin; zmax_ = i.zmax;
    xcenter_ = i.xcenter; ycenter_ = i.ycenter; zcenter_ = i.zcenter;
    xdelta_ = i.xdelta; ydelta_ = i.ydelta; zdelta_ = i.zdelta;
    voxel_size_ = i.voxel_size;
    xdim_ = i.xdim; ydim_ = i.ydim; zdim_ = i.zdim;
    hsize_ = i.hsize;
  }

  bool integrate(const pcl::PointCloud<pcl::PointXYZRGB>::Ptr& cloud, const pcl::PointCloud<pcl::Normal>* normals) {
    const size_t n = cloud->points.size();
    std::vector<float> xyz(3 * n), nrm(normals ? 3 * n : 0);
    for (size_t i = 0; i < n; ++i) {
      xyz[3 * i] = cloud->points[i].x;
      xyz[3 * i + 1] = cloud->points[i].y;
      xyz[3 * i + 2] = cloud->points[i].z;
      if (normals)
        for (int k = 0; k < 3; ++k) nrm[3 * i + k] = normals->points[i].normal[k];
    }
    int64_t binned = 0, hazard = 0;
    dmf_check(dmf_volume_integrate(h_, xyz.data(), normals ? nrm.data() : nullptr, (int64_t)n, &binned, &hazard));
    pull_occupied();
    return true;
  }

  void pull_occupied() {
    int64_t V = 0;
    dmf_check(dmf_volume_occupied(h_, nullptr, 0, &V));
    occupied_cells_.resize((size_t)V);
    if (V) dmf_check(dmf_volume_occupied(h_, reinterpret_cast<uint64_t*>(occupied_cells_.data()), V, &V));
    touch();
  }

  void rebuild_mirror() {
    const size_t V = occupied_cells_.size();
    dmf_volume_info info;
    dmf_check(dmf_volume_get_info(h_, &info));
    const int64_t np = info.num_points;
    std::vector<int32_t> view(V), off(V + 1);
    std::vector<uint8_t> good(V);
    std::vector<float> pts(3 * (size_t)np), nrm4(4 * (size_t)np);
    if (V) {
      dmf_check(dmf_volume_voxel_flags(h_, view.data(), good.data(), (int64_t)V));
      dmf_check(dmf_volume_export(h_, off.data(), pts.data(), nrm4.data(), np));
    }
    store_.clear();
    store_.reserve(V);
    slot_of_.assign((size_t)xdim_ * ydim_ * zdim_, -1);
    for (size_t s = 0; s < V; ++s) {
      std::unique_ptr<Voxel> vx(new Voxel());
      for (int32_t i = off[s]; i < off[s + 1]; ++i) {
        pcl::PointXYZRGB pt;
        pt.x = pts[3 * (size_t)i]; pt.y = pts[3 * (size_t)i + 1]; pt.z = pts[3 * (size_t)i + 2];
        vx->pts.push_back(pt);
        if (nrm4[4 * (size_t)i + 3] != 0.f) {  // only points integrated with a normal carry one
          pcl::Normal nm;
          for (int k = 0; k < 3; ++k) nm.normal[k] = nrm4[4 * (size_t)i + k];
          vx->normals.push_back(nm);
        }
      }
      vx->view = view[s];
      vx->good = good[s] != 0;
      store_.push_back(std::move(vx));
      int x, y, z;
      std::tie(x, y, z) = getVoxelCoords(occupied_cells_[s]);
      slot_of_[((size_t)x * ydim_ + y) * zdim_ + z] = (int32_t)s;
    }
    mirror_version_ = version_;
  }

  Voxel* mirror_at(int x, int y, int z) {
    if (mirror_version_ != version_) rebuild_mirror();
    if (!validCoords(x, y, z)) return nullptr;
    const int32_t s = slot_of_[((size_t)x * ydim_ + y) * zdim_ + z];
    return s < 0 ? nullptr : store_[(size_t)s].get();
  }
};
