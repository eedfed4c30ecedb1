"""CPU: the candidate views' restatement tests/views_ref.py pinned bit for bit to the
tree's host code -- pcl::VoxelGrid<PointXYZRGBNormal> of compat/shims and Algorithms::positionCameras /
positionCamera of compat/Algorithms.hpp, compiled here with g++ -- on every named case; that the named
cases are adversarial where they claim to be; the Python argument checks; and that the new compat
functions and the example compile."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import views_ref as VR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "depth-map-fusion-utils_amd")
COMPAT = os.path.join(PKG, "compat")
INCLUDES = ["-I", COMPAT, "-I", os.path.join(COMPAT, "shims"), "-I", os.path.join(ROOT, "include")]
DISTANCES = (0, 100, 300, 600)

# Reads cases (int32 n, float leaf[3], n x 3 xyz, n x 3 normals), runs the host VoxelGrid on each (leaf > 0) and
# writes int32 m, m x 3 xyz, m x 3 mean normals; then for each distance the plain positionCamera loop
# (12 floats per pose), positionCameras (12 floats per pose) and the normals it leaves behind.
HOST_PIN = r'''
#include <cmath>
#include <cstdio>
#include <vector>
#include <pcl/filters/voxel_grid.h>
#include <pcl/point_cloud.h>
#include <pcl/point_types.h>
#include "Algorithms.hpp"
#include "PointCloudProcessing.hpp"
using Cloud = pcl::PointCloud<pcl::PointXYZRGBNormal>;
static void poses_out(const std::vector<Eigen::Affine3f>& cams, FILE* o) {
  for (const auto& q : cams) {
    float p[12];
    dmf_compat::pose12(q, p);
    fwrite(p, 4, 12, o);
  }
}
int main(int argc, char** argv) {
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  int ncases = 0, nd = 0;
  unsigned dist[8];
  if (fread(&ncases, 4, 1, in) != 1 || fread(&nd, 4, 1, in) != 1 || fread(dist, 4, nd, in) != (size_t)nd) return 2;
  for (int c = 0; c < ncases; ++c) {
    int n = 0;
    float leaf[3];
    if (fread(&n, 4, 1, in) != 1 || fread(leaf, 4, 3, in) != 3) return 2;
    std::vector<float> xyz(3 * (size_t)n), nrm(3 * (size_t)n);
    if (fread(xyz.data(), 4, xyz.size(), in) != xyz.size() || fread(nrm.data(), 4, nrm.size(), in) != nrm.size()) return 2;
    Cloud::Ptr cloud(new Cloud), small(new Cloud);
    cloud->points.resize(n);
    for (int i = 0; i < n; ++i) {
      pcl::PointXYZRGBNormal& p = cloud->points[i];
      p.x = xyz[3 * i]; p.y = xyz[3 * i + 1]; p.z = xyz[3 * i + 2];
      for (int a = 0; a < 3; ++a) p.normal[a] = nrm[3 * i + a];
      // (as the PCD reader marks a cloud with a non-finite point)
      if (!(std::isfinite(p.x) && std::isfinite(p.y) && std::isfinite(p.z))) cloud->is_dense = false;
    }
    cloud->width = n;
    if (leaf[0] <= 0) {
      *small = *cloud;  // the placement's own case: no VoxelGrid in front
    } else if (leaf[0] == leaf[1] && leaf[1] == leaf[2]) {
      PointCloudProcessing::downsample<pcl::PointXYZRGBNormal>(cloud, small, (double)leaf[0]);
    } else {
      pcl::VoxelGrid<pcl::PointXYZRGBNormal> sor;
      sor.setLeafSize(leaf[0], leaf[1], leaf[2]);
      sor.setInputCloud(cloud);
      sor.filter(*small);
    }
    const int m = (int)small->points.size();
    fwrite(&m, 4, 1, out);
    for (const auto& p : small->points) { const float v[3] = {p.x, p.y, p.z}; fwrite(v, 4, 3, out); }
    for (const auto& p : small->points) fwrite(p.normal, 4, 3, out);
    for (int d = 0; d < nd; ++d) {
      Cloud::Ptr loc(new Cloud(*small));
      std::vector<Eigen::Affine3f> plain;
      for (int i = 0; i < m; ++i) plain.push_back(Algorithms::positionCamera(loc, i, dist[d]));
      poses_out(plain, out);
      poses_out(Algorithms::positionCameras(loc, dist[d]), out);
      for (const auto& p : loc->points) fwrite(p.normal, 4, 3, out);
    }
  }
  fclose(out);
  return 0;
}
'''

# every named case the host code can run (it has no refusal: the refused case is the GPU's), and the
# placement's own inputs as one more case that skips the VoxelGrid (leaf <= 0 in the pin's input)
PIN_CASES = tuple(n for n in VR.CASES if n not in ("refused", "unit_normals", "unit_zero_mean"))


def _gxx():
    g = shutil.which("g++")
    assert g, "g++ not found"
    return g


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """{case: (xyz, normals, {distance: (plain poses, poses, normals left behind)})} of the host code."""
    d = tmp_path_factory.mktemp("views_pin")
    src, exe, fin, fout = d / "pin.cpp", d / "pin", d / "in.bin", d / "out.bin"
    src.write_text(HOST_PIN)
    r = subprocess.run([_gxx(), "-O2", "-std=c++17", "-Wall", *INCLUDES, "-o", str(exe), str(src)], capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stderr
    names = PIN_CASES + ("placement",)
    with open(fin, "wb") as f:
        f.write(struct.pack("<ii", len(names), len(DISTANCES)) + np.asarray(DISTANCES, np.uint32).tobytes())
        for name in names:
            if name == "placement":
                xyz, nn = VR.placement_inputs()
                leaf = VR.leaf3(-1.0)
            else:
                xyz, nn, leaf, _, _ = VR.case(name)
            if nn is None:
                nn = np.zeros_like(xyz)
            f.write(struct.pack("<i", xyz.shape[0]) + leaf.tobytes() + xyz.tobytes() + nn.tobytes())
    r = subprocess.run([str(exe), str(fin), str(fout)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    raw = np.fromfile(fout, np.uint32)
    out, at = {}, 0

    def take(k):
        nonlocal at
        a = raw[at:at + k]
        at += k
        return a
    for name in names:
        m = int(take(1)[0])
        xyz, nn = take(3 * m).reshape(m, 3), take(3 * m).reshape(m, 3)
        place = {}
        for dist in DISTANCES:
            place[dist] = (take(12 * m).reshape(m, 3, 4), take(12 * m).reshape(m, 3, 4), take(3 * m).reshape(m, 3))
        out[name] = (xyz, nn, place)
    assert at == raw.size
    return out


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("name", PIN_CASES)
def test_restatement_equals_the_host_voxel_grid(host, name):
    """views_ref.downsample == pcl::VoxelGrid of compat/shims on the named case, as bit patterns."""
    xyz, nn, leaf, unit, want = VR.case(name)
    hx, hn, _ = host[name]
    assert hx.shape[0] == want[3][0]
    assert np.array_equal(hx, _bits(want[0]))
    if nn is not None:
        assert np.array_equal(hn, _bits(want[1]))


@pytest.mark.parametrize("name", ("placement", "uniform", "nonfinite_rows", "far"))
def test_restatement_equals_the_host_placement(host, name):
    """views_ref.position_cameras == Algorithms::positionCameras (poses and the normals it flips in its
    cloud) and, with flip=False, the plain positionCamera loop, for every distance; signs of zero
    and NaN words included."""
    hx, hn, place = host[name]
    xyz, nn = hx.view(np.float32), hn.view(np.float32)
    for dist, (plain, poses, left) in place.items():
        wp, wn = VR.position_cameras(xyz, nn, dist, flip=True)
        assert np.array_equal(_bits(wp), poses), dist
        assert np.array_equal(_bits(wn), left), dist
        kp, kn = VR.position_cameras(xyz, nn, dist, flip=False)
        assert np.array_equal(_bits(kp), plain), dist
        assert np.array_equal(_bits(kn), hn), dist


def test_placement_case_keeps_every_point(host):
    """(the pin's placement case reaches the host placement as it is: zeros of both signs, NaN words)"""
    xyz, nn = VR.placement_inputs()
    assert np.array_equal(host["placement"][0], _bits(xyz)) and np.array_equal(host["placement"][1], _bits(nn))


def test_crowded_leaf_depends_on_the_order_of_its_adds():
    """About 4094 points in one 0.1 leaf near x = 1000: summing the leaf in descending index gives
    other bits, so a reduction tree or a reordered walk cannot pass."""
    for name in ("crowded", "crowded_interleaved"):
        xyz, nn, leaf, unit, want = VR.case(name)
        j = int(np.argmax(want[2]))
        assert want[2][j] >= 4094
        rev = VR.downsample(xyz, leaf, nn, unit, reverse=True)
        assert np.array_equal(rev[2], want[2])
        assert (_bits(rev[0][j]) != _bits(want[0][j])).any() or (_bits(rev[1][j]) != _bits(want[1][j])).any()


def test_crowded_interleaved_needs_a_stable_order():
    """The crowded leaf's members sit at the even indices of the whole range, other leaves' between."""
    xyz, _, leaf, _, want = VR.case("crowded_interleaved")
    idx, key = VR.leaf_keys(xyz, leaf)
    big = np.bincount(key - key.min()).argmax() + key.min()
    members = idx[key == big]
    assert members.size >= 4094 and members.min() < 4 and members.max() > xyz.shape[0] - 4


def test_boundary_lattice_falls_into_the_leaf_below():
    """Of the float lattice k * 0.1f some points land in leaf k - 1 under the float32 product p * inv
    (none would in double); with leaf 0.125 = 2^-3 the product is exact and none does."""
    k = np.arange(-40, 81)
    px = k.astype(np.float32) * np.float32(0.1)
    got = np.floor(px * (np.float32(1) / np.float32(0.1))).astype(np.int64)
    assert ((got == k) | (got == k - 1)).all() and 0 < int((got == k - 1).sum()) < 20
    assert (np.floor(px.astype(np.float64) * (1.0 / 0.1)).astype(np.int64) != got).any()
    k = np.arange(-20, 21)
    px = k.astype(np.float32) * np.float32(0.125)
    assert np.array_equal(np.floor(px * (np.float32(1) / np.float32(0.125))).astype(np.int64), k)
    xyz = VR.case("lattice_01")[0]
    assert (xyz < 0).any() and (xyz > 0).any()


def test_large_key_and_refused_cases():
    xyz, _, leaf, _, want = VR.case("large_key")
    _, key = VR.leaf_keys(xyz, leaf)
    _, _, _, div = VR.leaf_box(xyz, leaf)
    assert int(np.prod(div.astype(object))) == 1201 ** 3 == 1732323601 and int(key.max()) > 2 ** 30
    assert want[3] == (3, 3, 1)
    xyz, _, leaf, _, want = VR.case("refused")
    assert want is None
    inv = np.float32(1) / leaf
    div = np.floor(xyz.max(axis=0) * inv).astype(np.int64) - np.floor(xyz.min(axis=0) * inv).astype(np.int64) + 1
    assert int(np.prod(div.astype(object))) == 2197000000 > VR.INT_MAX
    with pytest.raises(VR.Refused):
        VR.downsample(np.array([[0, 0, 0], [3e9, 0, 0]], np.float32), 1.0)


def test_unit_normals_restatement():
    xyz, nn, leaf, unit, want = VR.case("unit_zero_mean")
    assert unit and (_bits(want[1][0]) == 0).all() and want[2][0] == 2
    lens = np.linalg.norm(want[1][1:].astype(np.float64), axis=1)
    assert np.abs(lens - 1).max() < 1e-6


def test_python_argument_checks():
    """Checked before any device call: the volume handle is never touched."""
    import dmf_amd

    class NoDevice(dmf_amd.VoxelVolume):
        def __init__(self):                      # no dmf_volume_create: any call into the library would fail
            self._L, self._h = None, None

        def __del__(self):
            pass

        dims = (4, 4, 4)

    v = NoDevice()
    xyz, nn = np.zeros((5, 3), np.float32), np.zeros((5, 3), np.float32)
    lo = np.zeros(64, np.int16)
    bad_calls = [
        lambda: v.cloud_downsample(np.zeros((5, 2), np.float32), 0.1),
        lambda: v.cloud_downsample(xyz.astype(np.float64), 0.1),
        lambda: v.cloud_downsample(xyz, 0.0),
        lambda: v.cloud_downsample(xyz, -0.1),
        lambda: v.cloud_downsample(xyz, float("nan")),
        lambda: v.cloud_downsample(xyz, float("inf")),
        lambda: v.cloud_downsample(xyz, (0.1, 0.1)),
        lambda: v.cloud_downsample(xyz, 1e-60),            # underflows to 0 in float32
        lambda: v.cloud_downsample(xyz, "0.1"),
        lambda: v.cloud_downsample(xyz, 0.1, normals=np.zeros((4, 3), np.float32)),
        lambda: dmf_amd.position_cameras(v, xyz, nn[:4]),
        lambda: dmf_amd.position_cameras(v, xyz[:, :2], nn),
        lambda: dmf_amd.position_cameras(v, xyz, nn, distance_mm=-1),
        lambda: dmf_amd.position_cameras(v, xyz, nn, distance_mm=2 ** 32),
        lambda: v.surface_views(lo.astype(np.int32), 0.1),
        lambda: v.surface_views(lo[:63], 0.1),
        lambda: v.surface_views(lo, 0.0),
        lambda: v.surface_views(lo, (0.1, 0.2, float("nan"))),
        lambda: v.surface_views(lo, 0.1, distance_mm=-5),
    ]
    for k, call in enumerate(bad_calls):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"call {k} was accepted")


def test_abi_declares_the_six_calls():
    from dmf_amd import _lib
    names = {"dmf_cloud_downsample", "dmf_cloud_downsample_device", "dmf_position_cameras",
             "dmf_position_cameras_device", "dmf_grid_surface_views", "dmf_grid_surface_views_device"}
    assert names <= set(_lib.declared_symbols()) and names <= set(_lib.SIGNATURES)
    hdr = open(_lib.HEADER_PATH).read()
    assert "DMF_LEAVES_REFUSED" in hdr


def test_compat_functions_and_example_compile(tmp_path):
    """dmf_compat::downsampleOnDevice / positionCamerasOnDevice / surfaceViews in the reference's
    vocabulary, and compat/examples/views_headless.cpp (g++ -fsyntax-only against the headless shims)."""
    src = tmp_path / "views.cpp"
    src.write_text('''
#include "Algorithms.hpp"
#include "PointCloudProcessing.hpp"
int main() {
  VoxelVolume volume;
  pcl::PointCloud<pcl::PointXYZRGBNormal>::Ptr cloud(new pcl::PointCloud<pcl::PointXYZRGBNormal>),
      locations(new pcl::PointCloud<pcl::PointXYZRGBNormal>);
  dmf_compat::downsampleOnDevice(volume, cloud, locations, 0.1);
  std::vector<Eigen::Affine3f> a = dmf_compat::positionCamerasOnDevice(volume, locations, 300);
  std::vector<Eigen::Affine3f> b = dmf_compat::positionCamerasOnDevice(volume, locations, 300, false);
  std::vector<int16_t> logodds(1);
  std::vector<Eigen::Affine3f> c = dmf_compat::surfaceViews(volume, logodds, locations, 0.1, 300, 1, -1, false);
  return (int)(a.size() + b.size() + c.size());
}
''')
    example = os.path.join(COMPAT, "examples", "views_headless.cpp")
    for f in (str(src), example):
        r = subprocess.run([_gxx(), "-std=c++17", "-fsyntax-only", "-Wall", *INCLUDES, f], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
