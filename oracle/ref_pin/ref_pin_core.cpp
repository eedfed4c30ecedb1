// ref_pin_core — runs Camera / VoxelVolume / RayTracingEngine on one scene file and writes
// every observable to a result file (formats: tests/ref_pin.py, which writes the one and
// reads the other).
//
// One source, two builds:
//  * against a checkout of the reference (its include/ directory on the include path, with
//    compat/shims for the Eigen / PCL vocabulary): the reference's own control flow, on the
//    CPU.  The results are the fixtures tests/golden/ref_pin_*.npz (oracle/Makefile ref_pin).
//  * against compat/ and libdmf.so (the drop-in headers over the GPU engine): the same
//    calls must give the same file.
// Nothing here restates the reference: the headers are included by name.
//
// The reference cannot reset a voxel's view / good, and the drop-in's voxels_ is a read-only
// mirror, so the flags are reset the one way both allow: a new volume, integrated again,
// after every call that may have written them.
//
// Left out, because the reference leaves them undefined: z = 0 in deProjectPoint, acos
// arguments outside [-1, 1] (int(NaN)), points that bin to xdim in the no-normals
// integratePointCloud (no validCoords check), and -- on a grid whose dims truncate -- every
// function that indexes voxels_ without validCoords (the forward family, reverseRayTrace,
// rayTraceVolume); a scene switches those off with bit 1 of its flags.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <tuple>
#include <utility>
#include <vector>

#include <Volume.hpp>
#include <RayTracingEngine.hpp>

namespace {

struct Reader {
  FILE* f;
  template <class T>
  T one() {
    T v;
    if (fread(&v, sizeof(T), 1, f) != 1) { fprintf(stderr, "ref_pin: short scene file\n"); exit(2); }
    return v;
  }
  template <class T>
  std::vector<T> many(size_t n) {
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "ref_pin: short scene file\n"); exit(2); }
    return v;
  }
};

template <class T> struct Code;
template <> struct Code<uint8_t> { static const uint32_t v = 0; };
template <> struct Code<int32_t> { static const uint32_t v = 1; };
template <> struct Code<int64_t> { static const uint32_t v = 2; };
template <> struct Code<uint64_t> { static const uint32_t v = 3; };
template <> struct Code<float> { static const uint32_t v = 4; };
template <> struct Code<double> { static const uint32_t v = 5; };

struct Writer {
  FILE* f;
  template <class T>
  void put(const std::string& name, const std::vector<T>& a) {
    const uint32_t len = (uint32_t)name.size(), code = Code<T>::v;
    const uint64_t bytes = (uint64_t)a.size() * sizeof(T);
    fwrite(&len, 4, 1, f);
    fwrite(name.data(), 1, len, f);
    fwrite(&code, 4, 1, f);
    fwrite(&bytes, 8, 1, f);
    if (bytes) fwrite(a.data(), 1, bytes, f);
  }
};

struct Scene {
  int32_t H, W;
  std::vector<float> K;
  std::vector<double> bounds;
  int32_t mode;
  std::vector<int32_t> dims;
  std::vector<double> res;
  int32_t flags;
  std::vector<float> xyz, nrm;
  std::vector<float> poses;
};

std::unique_ptr<VoxelVolume> make_volume(const Scene& s, bool normals) {
  std::unique_ptr<VoxelVolume> v(new VoxelVolume());
  v->setDimensions(s.bounds[0], s.bounds[1], s.bounds[2], s.bounds[3], s.bounds[4], s.bounds[5]);
  if (s.mode == 0) v->setVolumeSize(s.dims[0], s.dims[1], s.dims[2]);
  else v->setResolution(s.res[0], s.res[1], s.res[2]);
  v->constructVolume();
  pcl::PointCloud<pcl::PointXYZRGB>::Ptr cloud(new pcl::PointCloud<pcl::PointXYZRGB>());
  pcl::PointCloud<pcl::Normal>::Ptr nn(new pcl::PointCloud<pcl::Normal>());
  for (size_t i = 0; i < s.xyz.size() / 3; ++i) {
    pcl::PointXYZRGB p;
    p.x = s.xyz[3 * i]; p.y = s.xyz[3 * i + 1]; p.z = s.xyz[3 * i + 2];
    cloud->points.push_back(p);
    pcl::Normal n;
    for (int k = 0; k < 3; ++k) n.normal[k] = s.nrm[3 * i + k];
    nn->points.push_back(n);
  }
  if (normals) v->integratePointCloud(cloud, nn);
  else v->integratePointCloud(cloud);
  return v;
}

Eigen::Affine3f pose_of(const Scene& s, int p) {
  Eigen::Affine3f T = Eigen::Affine3f::Identity();
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 4; ++j) T(i, j) = s.poses[12 * p + 4 * i + j];
  return T;
}

// view / good (and, with counts, pts.size() / normals.size()) of every occupied voxel, appended
void read_flags(VoxelVolume& v, std::vector<int32_t>& view, std::vector<uint8_t>& good,
                std::vector<int32_t>* npts = nullptr, std::vector<int32_t>* nnrm = nullptr) {
  for (auto h : v.occupied_cells_) {
    int x, y, z;
    std::tie(x, y, z) = v.getVoxelCoords(h);
    Voxel* vx = v.voxels_[x][y][z];
    view.push_back(vx->view);
    good.push_back(vx->good ? 1 : 0);
    if (npts) npts->push_back((int32_t)vx->pts.size());
    if (nnrm) nnrm->push_back((int32_t)vx->normals.size());
  }
}

struct Calls {
  std::vector<uint8_t> found, good;
  std::vector<int32_t> ret, view;
  std::vector<int64_t> count;
  std::vector<uint64_t> list;
  void add(VoxelVolume& v, bool f, int32_t r, const std::vector<unsigned long long int>* l) {
    found.push_back(f ? 1 : 0);
    ret.push_back(r);
    count.push_back(l ? (int64_t)l->size() : 0);
    if (l) for (auto h : *l) list.push_back((uint64_t)h);
    read_flags(v, view, good);
  }
  void write(Writer& w, const std::string& pre) {
    w.put(pre + "_found", found);
    w.put(pre + "_ret", ret);
    w.put(pre + "_count", count);
    w.put(pre + "_list", list);
    w.put(pre + "_view", view);
    w.put(pre + "_good", good);
  }
};

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: %s scene.bin result.bin\n", argv[0]); return 2; }
  FILE* fi = fopen(argv[1], "rb");
  if (!fi) { perror(argv[1]); return 2; }
  Reader in{fi};
  const std::vector<char> magic = in.many<char>(8);
  if (std::memcmp(magic.data(), "DMFPIN01", 8) != 0) { fprintf(stderr, "ref_pin: bad magic\n"); return 2; }
  Scene s;
  s.H = in.one<int32_t>(); s.W = in.one<int32_t>();
  s.K = in.many<float>(9);
  s.bounds = in.many<double>(6);
  s.mode = in.one<int32_t>();
  s.dims = in.many<int32_t>(3);
  s.res = in.many<double>(3);
  s.flags = in.one<int32_t>();
  const int32_t n = in.one<int32_t>();
  s.xyz = in.many<float>(3 * (size_t)n);
  s.nrm = in.many<float>(3 * (size_t)n);
  const int32_t P = in.one<int32_t>();
  s.poses = in.many<float>(12 * (size_t)P);
  const int32_t n_proj = in.one<int32_t>();
  const std::vector<int32_t> proj = in.many<int32_t>(3 * (size_t)n_proj);
  const int32_t n_tr = in.one<int32_t>();
  const std::vector<double> tr = in.many<double>(3 * (size_t)n_tr);
  const std::vector<int32_t> tr_pose = in.many<int32_t>((size_t)n_tr);
  const int32_t n_dep = in.one<int32_t>();
  const std::vector<double> dep = in.many<double>(3 * (size_t)n_dep);
  const int32_t n_vp = in.one<int32_t>();
  const std::vector<int32_t> vp = in.many<int32_t>(2 * (size_t)n_vp);
  const int32_t n_deg = in.one<int32_t>();
  const std::vector<double> deg = in.many<double>((size_t)n_deg);
  const int32_t n_vpt = in.one<int32_t>();
  const std::vector<float> vpt = in.many<float>(3 * (size_t)n_vpt);
  fclose(fi);
  const bool no_normals = s.flags & 1, unguarded = s.flags & 2;

  FILE* fo = fopen(argv[2], "wb");
  if (!fo) { perror(argv[2]); return 2; }
  Writer out{fo};

  // ---- volume
  {
    std::unique_ptr<VoxelVolume> v = make_volume(s, true);
    out.put("vol_dims", std::vector<int32_t>{v->xdim_, v->ydim_, v->zdim_});
    out.put("vol_deltas", std::vector<double>{v->xdelta_, v->ydelta_, v->zdelta_, v->voxel_size_});
    out.put("vol_hsize", std::vector<uint64_t>{(uint64_t)v->hsize_});
    out.put("occ", std::vector<uint64_t>(v->occupied_cells_.begin(), v->occupied_cells_.end()));
    std::vector<int32_t> view, npts, nnrm;
    std::vector<uint8_t> good;
    read_flags(*v, view, good, &npts, &nnrm);
    out.put("occ_npts", npts);
    out.put("occ_nnrm", nnrm);
  }
  if (no_normals) {
    std::unique_ptr<VoxelVolume> v = make_volume(s, false);
    out.put("nn_occ", std::vector<uint64_t>(v->occupied_cells_.begin(), v->occupied_cells_.end()));
    std::vector<int32_t> view, npts, nnrm;
    std::vector<uint8_t> good;
    read_flags(*v, view, good, &npts, &nnrm);
    out.put("nn_npts", npts);
    out.put("nn_nnrm", nnrm);
  }

  // ---- camera and utilities
  Camera cam(s.K, s.H, s.W);
  {
    std::vector<float> a;
    for (int i = 0; i < n_proj; ++i) {
      float x, y, z;
      std::tie(x, y, z) = cam.projectPoint(proj[3 * i], proj[3 * i + 1], proj[3 * i + 2]);
      a.push_back(x); a.push_back(y); a.push_back(z);
    }
    out.put("probe_project", a);
    std::vector<float> b;
    for (int i = 0; i < n_tr; ++i) {
      Eigen::Affine3f T = pose_of(s, tr_pose[i]);
      float x, y, z;
      std::tie(x, y, z) = cam.transformPoints(tr[3 * i], tr[3 * i + 1], tr[3 * i + 2], T);
      b.push_back(x); b.push_back(y); b.push_back(z);
    }
    out.put("probe_transform", b);
    std::vector<int32_t> c;
    for (int i = 0; i < n_dep; ++i) {
      int r, col;
      std::tie(r, col) = cam.deProjectPoint(dep[3 * i], dep[3 * i + 1], dep[3 * i + 2]);
      c.push_back(r); c.push_back(col);
    }
    out.put("probe_deproject", c);
    std::vector<uint8_t> d;
    for (int i = 0; i < n_vp; ++i) d.push_back(cam.validPixel(vp[2 * i], vp[2 * i + 1]) ? 1 : 0);
    out.put("probe_validpixel", d);
    std::vector<int32_t> e;
    for (int i = 0; i < n_deg; ++i) e.push_back(degree(deg[i]));
    out.put("probe_degree", e);
  }

  // ---- the engine
  RayTracingEngine engine(cam);
  std::unique_ptr<VoxelVolume> vol = make_volume(s, true);
  {
    // validPoints and getVoxel themselves: behind validCoords, integratePointCloud and the
    // marches cannot tell `>=` from `>` at an upper bound
    std::vector<uint8_t> a;
    std::vector<int32_t> b;
    for (int i = 0; i < n_vpt; ++i) {
      a.push_back(vol->validPoints(vpt[3 * i], vpt[3 * i + 1], vpt[3 * i + 2]) ? 1 : 0);
      int x, y, z;
      std::tie(x, y, z) = vol->getVoxel(vpt[3 * i], vpt[3 * i + 1], vpt[3 * i + 2]);
      b.push_back(x); b.push_back(y); b.push_back(z);
    }
    out.put("probe_validpoints", a);
    out.put("probe_getvoxel", b);
  }
  bool dirty = false;
  auto fresh = [&]() -> VoxelVolume& {
    if (dirty) { vol = make_volume(s, true); dirty = false; }
    return *vol;
  };

  Calls rev;  // pose, {fast, full}, viz {1, 0}, zdelta {1, 3}
  for (int p = 0; p < P; ++p)
    for (int full = 0; full < (unguarded ? 2 : 1); ++full)
      for (int viz = 1; viz >= 0; --viz)
        for (int zd : {1, 3}) {
          VoxelVolume& v = fresh();
          std::pair<bool, std::vector<unsigned long long int>> r =
              full ? engine.reverseRayTrace(v, pose_of(s, p), viz != 0, zd)
                   : engine.reverseRayTraceFast(v, pose_of(s, p), viz != 0, zd);
          rev.add(v, r.first, 0, &r.second);
          dirty = viz != 0;
        }
  rev.write(out, "rev");

  if (unguarded) {
    Calls fwd;  // pose, function, sparse {1, 0}, zdelta {10, 7, 1}
    for (int p = 0; p < P; ++p)
      for (int fn = 0; fn < 5; ++fn)
        for (int sparse = 1; sparse >= 0; --sparse)
          for (int zd : {10, 7, 1}) {
            VoxelVolume& v = fresh();
            Eigen::Affine3f T = pose_of(s, p);
            if (fn == 0) {
              engine.rayTrace(v, T, zd, sparse != 0);
              fwd.add(v, false, 0, nullptr);
              dirty = true;
            } else if (fn == 1) {
              engine.rayTraceAndClassify(v, T, zd, p + 1, sparse != 0);
              fwd.add(v, false, 0, nullptr);
              dirty = true;
            } else if (fn == 2) {
              auto r = engine.rayTraceAndGetGoodPoints(v, T, zd, sparse != 0);
              fwd.add(v, r.first, 0, &r.second);
            } else if (fn == 3) {
              auto r = engine.rayTraceAndGetPoints(v, T, zd, sparse != 0);
              fwd.add(v, r.first, 0, &r.second);
            } else {
              const int m = engine.rayTraceAndGetMinimum(v, T, zd, sparse != 0);
              fwd.add(v, false, m, nullptr);
            }
          }
    fwd.write(out, "fwd");

    Calls rtv;  // rayTraceVolume of every pose
    for (int p = 0; p < P; ++p) {
      VoxelVolume& v = fresh();
      Eigen::Affine3f T = pose_of(s, p);
      engine.rayTraceVolume(v, T);
      rtv.add(v, false, 0, nullptr);
      dirty = true;
    }
    rtv.write(out, "rtv");

    // flags that survive from call to call: rayTraceAndClassify keeps a view that is set and a
    // good that is true; reverseRayTraceFast(viz) then writes over both
    Calls chain;
    if (P >= 2) {
      VoxelVolume& v = fresh();
      Eigen::Affine3f T0 = pose_of(s, 0), T1 = pose_of(s, 1);
      engine.rayTraceAndClassify(v, T0, 10, 2, false);
      chain.add(v, false, 0, nullptr);
      engine.rayTraceAndClassify(v, T1, 7, 3, false);
      chain.add(v, false, 0, nullptr);
      auto r = engine.reverseRayTraceFast(v, T1, true, 1);
      chain.add(v, r.first, 0, &r.second);
      dirty = true;
    }
    chain.write(out, "chain");
  }
  if (fclose(fo) != 0) { perror(argv[2]); return 2; }
  return 0;
}
