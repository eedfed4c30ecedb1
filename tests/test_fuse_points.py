"""CPU: point-cloud fusion's ABI surface and the self-check of its pure-Python
restatement (tests/fuse_points_ref.py).  No GPU: the entry points are only asked to refuse bad
plain arguments, which they do before they touch the volume."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np

import fuse_points_ref as FR
import helpers as Hh

NAMES = ("dmf_fuse_points", "dmf_fuse_points_device", "dmf_fuse_points_reserve")


def test_symbols_declared_and_exported():
    from dmf_amd import _lib
    L = _lib.load()
    syms = _lib.declared_symbols()
    for n in NAMES:
        assert n in syms and n in _lib.SIGNATURES and hasattr(L, n), n
    import dmf_amd
    assert callable(dmf_amd.RayTracingEngine.fuse_points)
    assert "fuse_points" not in dmf_amd.__all__
    assert L.dmf_abi_version() == 1


def test_plain_arguments_rejected_without_gpu():
    """Null volume / params / buffers, N = 0, S = 0 and S = 65536 are DMF_ERR_INVALID; these
    checks precede any access to the volume, so a zeroed stand-in buffer serves as the non-null
    handle.  With plain arguments in order that handle is read, and its `constructed` = 0 gives
    DMF_ERR_STATE.  The counters stay as they were."""
    from dmf_amd import _lib
    L = _lib.load()
    fake = C.create_string_buffer(1 << 16)
    v = C.addressof(fake)
    prm = _lib.default_fuse_params()
    pp = C.addressof(prm)
    xyz, org = np.zeros(12, np.float32), np.zeros(3, np.float32)
    hits, misses = np.full(8, 5, np.int32), np.full(8, -7, np.int32)
    st = np.full(8, 3, np.int64)
    x, o, h, m, s = (a.ctypes.data for a in (xyz, org, hits, misses, st))
    INV = _lib.DMF_ERR_INVALID
    for call in (L.dmf_fuse_points, L.dmf_fuse_points_device):
        assert call(None, x, o, 1, 4, pp, h, m, s) == INV
        assert call(v, None, o, 1, 4, pp, h, m, s) == INV
        assert call(v, x, None, 1, 4, pp, h, m, s) == INV
        assert call(v, x, o, 1, 4, None, h, m, s) == INV
        assert call(v, x, o, 1, 4, pp, None, m, s) == INV
        assert call(v, x, o, 1, 4, pp, h, None, s) == INV
        for S, N in ((1, 0), (1, -1), (0, 4), (-1, 4), (65536, 4)):
            assert call(v, x, o, S, N, pp, h, m, s) == INV, (S, N)
        assert b"" != L.dmf_last_error()
        assert call(v, x, o, 1, 4, pp, h, m, s) == _lib.DMF_ERR_STATE
        assert call(v, x, o, 1, 4, pp, h, m, None) == _lib.DMF_ERR_STATE   # the statistics are optional
    res = L.dmf_fuse_points_reserve
    assert res(None, 1, 4, 0) == INV
    for S, N in ((1, 0), (0, 4), (65536, 4)):
        assert res(v, S, N, 0) == INV, (S, N)
    assert res(v, 1, 4, 0) == _lib.DMF_ERR_STATE
    assert (hits == 5).all() and (misses == -7).all() and (st == 3).all()


def test_compat_fuse_points_compiles(tmp_path):
    """Both fusePoints overloads beside fuseDepth in compat/RayTracingEngine.hpp (g++ -fsyntax-only
    against the headless shims)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    compat = os.path.join(root, "depth-map-fusion-utils_amd", "compat")
    src = tmp_path / "points.cpp"
    src.write_text('''
#include "Camera.hpp"
#include "RayTracingEngine.hpp"
#include "Volume.hpp"
int main() {
  VoxelVolume v;
  std::vector<float> K = {600, 0, 320, 0, 600, 240, 0, 0, 1};
  Camera cam(K);
  RayTracingEngine eng(cam);
  RayTracingEngine::FusionCounts acc;
  const std::vector<float> xyz = {0.1f, 0.2f, 0.3f, 0.0f, 0.1f, -0.2f}, origins = {0.0f, 0.0f, 0.9f};
  eng.fusePoints(v, xyz, origins, acc);
  dmf_fuse_params prm;
  dmf_fuse_params_default(&prm);
  eng.fusePoints(v, xyz, origins, acc, &prm);
  pcl::PointCloud<pcl::PointXYZRGBNormal>::Ptr cloud(new pcl::PointCloud<pcl::PointXYZRGBNormal>);
  pcl::PointXYZRGBNormal p;
  p.x = 0.1f;
  cloud->points.push_back(p);
  Eigen::Vector3f origin;
  origin(0) = 0.f; origin(1) = 0.f; origin(2) = 0.9f;
  RayTracingEngine::FusionCounts& r = eng.fusePoints(v, cloud, origin, acc);
  return (int)(r.rays + (long long)eng.logOdds(v, acc).size());
}
''')
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    r = subprocess.run([gxx, "-std=c++17", "-fsyntax-only", "-Wall", "-I", compat, "-I", os.path.join(compat, "shims"),
                        "-I", os.path.join(root, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_segment_case_holds_its_forced_cases():
    """The arbitrary-segment case of the GPU test (fuse_points_ref.segment_case) really holds what
    it names: the diagonals from the inside origin tie exactly at every crossing (origin on a cell
    corner, equal quantised extents on the moving axes), the skipped points are skipped, rays that
    miss the grid make no update, and E == O inside the grid is one hit."""
    xyz, origins, h0, m0 = FR.segment_case()
    assert xyz.shape == (3, FR.SEG_N, 3) and origins.shape == (3, 3) and h0.any() and m0.any()
    qo = FR.quantised(FR.SEG_BOUNDS, FR.SEG_DIMS, FR.SEG_INSIDE)
    assert all(q % 256 == 0 for q in qo), qo
    for E in FR.SEG_DIAGONALS:
        d = [abs(a - b) for a, b in zip(FR.quantised(FR.SEG_BOUNDS, FR.SEG_DIMS, E), qo)]
        moving = [x for x in d if x]
        assert len(moving) >= 2 and len(set(moving)) == 1 and moving[0] % 256 == 0, (E, d)
    one = lambda O, E: FR.fuse_points(FR.SEG_BOUNDS, FR.SEG_DIMS, np.array([E], np.float32), np.array(O, np.float32))
    nan = np.nan
    for O, E in ((FR.SEG_INSIDE, (nan, 0.1, 0.1)), (FR.SEG_INSIDE, (0.1, np.inf, 0.1)), ((0.0, nan, 0.9), (0.1, 0.1, 0.1))):
        h, m, st = one(O, E)
        assert not h.any() and not m.any() and not st.any()
    h, m, st = one(FR.SEG_OUTSIDE, (0.9, 0.0, 0.9))         # a ray, but it misses the grid
    assert not h.any() and not m.any() and list(st) == [0, 1, 0]
    h, m, st = one(FR.SEG_INSIDE, FR.SEG_INSIDE)            # E == O
    assert h.sum() == 1 and not m.any() and list(st) == [1, 1, 1]
    h, m, st = one(FR.SEG_INSIDE, FR.SEG_DIAGONALS[0])      # 15 steps on each axis, ties x < y < z
    assert list(st) == [46, 1, 1] and m.sum() == 45
    cells = np.argwhere(m.reshape(FR.SEG_DIMS) > 0)
    assert [tuple(c) for c in cells[:4]] == [(24, 24, 20), (25, 24, 20), (25, 25, 20), (25, 25, 21)]
    h, m, st = one(FR.SEG_OUTSIDE, (0.0, 0.0, -0.8))        # through the whole grid: misses only
    assert not h.any() and list(st) == [40, 1, 0]


def test_restatement_equals_oracle_on_frames(oracle):
    """Two 61x37 frames turned into points on the host with the oracle's own back-projection
    (pixels outside the depth gate NaN, origin = the pose's translation): the restatement's
    counters and statistics equal oracle.fuse_depth's on the frames."""
    from dmf_amd import scene
    W, H = Hh.KA_WH
    poses = np.ascontiguousarray(scene.fibonacci_poses(2, seed=5), np.float32)
    depth = scene.render_frames(Hh.KA, W, H, poses)
    dmin, dmax = 300, 800
    gated = (depth >= dmin) & (depth < dmax)
    assert gated.any() and ((depth > 0) & ~gated).any()   # the gate rejects pixels that hold a depth
    ho, mo, so = oracle.fuse_depth(Hh.oracle_grid(oracle, Hh.ODD_DIMS, Hh.ODD_BOUNDS), Hh.KA, depth, poses,
                                   dmin=dmin, dmax=dmax)
    xyz = np.stack([oracle.backproject(Hh.KA, depth[i], poses[i]) for i in range(2)])
    pts, origins = FR.frame_points(xyz, depth, poses, dmin, dmax)
    assert pts.shape == (2, W * H, 3) and np.isnan(pts).any()
    hr, mr, sr = FR.fuse_points(Hh.ODD_BOUNDS, Hh.ODD_DIMS, pts, origins)
    assert so[0] > 10 ** 4 and so[2] > 0
    assert np.array_equal(np.asarray(so)[:3], sr)
    assert np.array_equal(ho, hr) and np.array_equal(mo, mr)
