"""Pass A's per-ray setup (csrc/dmf_quant.hpp, dmf_brick.hpp qray_from / coarse_init32 / pack_ray32,
the scalar packet arithmetic of dmf_fuse.hip bk_rays_wg) against the CPU oracle on the inputs its
clip and quantisation are most likely to get wrong: hit and miss counters cell for cell, and the
statistics.  64x48 frames, at most four poses per case, the oracle's result computed once per case.

Pose sets (the intrinsics have a whole-pixel principal point and a power-of-two focal length):
  "out": cameras outside the grid beyond one face, beyond two faces and exactly on the plane of a
         third (go == n on that axis), beyond three faces, and the first pose again with a NaN
         rotation entry (NaN endpoint coordinates: counted as rays, the clip keeps or drops them
         as the oracle does).
  "in":  a camera on a brick corner inside the grid; an exact axis permutation on cell boundaries
         (axis-aligned centre ray, planar centre row and column); a camera inside looking out
         through the far face with depths that put most endpoints beyond it (the exit divisions);
         a camera outside looking past the grid's edge (some rays miss the grid entirely).
Geometries: 256^3 (power-of-two cells, the smallest grid the default dispatch sends to the brick
path) and 256 x 230 x 195 over odd bounds (cells that are no power of two, partial bricks).
Each case runs the brick pipeline with pass A's direct histogram, with its hashed histogram forced
to 16 words (the hashed kernel and, after its overflow, the recovery kernel) and the LDS-box kernel
(dda_setup over the same quantisation); the frames' finite poses also run as point scans."""
import functools

import numpy as np
import pytest

import helpers as Hh

pytestmark = pytest.mark.gpu

HH, WW = 48, 64
KK = np.array([32, 0, 32, 0, 32, 24, 0, 0, 1], np.float32)
DMIN, DMAX = 200, 1000
GEOMS = {"pow2": ((256, 256, 256), Hh.BOUNDS), "odd": ((256, 230, 195), Hh.ODD_BOUNDS)}


def _pose(R, eye):
    """Camera->world [R|t], R's columns x right, y down, z forward."""
    M = np.concatenate([np.asarray(R, np.float64), np.asarray(eye, np.float64)[:, None]], axis=1)
    return M.astype(np.float32).reshape(12)


def _look(eye, target=(0.0, 0.0, 0.0)):
    from dmf_amd import scene
    return _pose(scene.look_at(eye, target), eye)


def _depth(P, lo, hi, seed):
    """Depth in [lo, hi) mm with holes and values outside the gate; a constant centre block."""
    rng = np.random.default_rng(seed)
    d = rng.integers(lo, hi, (P, HH, WW)).astype(np.uint16)
    d[:, 20:29, 28:37] = (lo + hi) // 2
    d[:, ::7, ::5] = 0
    d[:, 3::11, 2::9] = DMAX + 5
    return d


def _poses(name):
    ax = np.eye(3)
    if name == "out":
        p = np.stack([
            _look((0.9, 0.1, 0.05)),                       # beyond one face
            _look((0.8, -0.75, 0.5), (0.0, 0.0, 0.1)),     # beyond two, exactly on the z = 0.5 plane
            _look((0.8, 0.75, -0.7)),                      # beyond three
            _look((0.9, 0.1, 0.05)),                       # non-finite below
        ])
        p[3, 0] = np.nan
        return p, _depth(4, 250, 1400, 11)
    p = np.stack([
        _look((0.125, 0.125, 0.125), (-0.3, -0.2, 0.1)),                       # a brick corner inside
        _pose(np.stack([ax[1], -ax[2], -ax[0]], axis=1), (0.625, 0.0, 0.0)),   # along -x, on cell boundaries
        _look((0.3, 0.2, -0.1), (1.5, 0.4, 0.0)),                              # inside, out through x = 0.5
        _look((0.9, 0.1, 0.05), (0.3, 1.2, 0.05)),                             # past the grid's edge
    ])
    return p, _depth(4, 250, 990, 12)


@functools.lru_cache(maxsize=None)
def _case(name, geom):
    from oracle import oracle as O
    O.lib()
    dims, bounds = GEOMS[geom]
    poses, depth = _poses(name)
    ov = Hh.oracle_grid(O, dims, bounds)
    ho, mo, so = O.fuse_depth(ov, KK, depth, poses, dmin=DMIN, dmax=DMAX)
    for a in (ho, mo, so):
        a.setflags(write=False)
    return dims, bounds, poses, depth, (ho, mo, so)


@functools.lru_cache(maxsize=None)
def _case_points(name, geom):
    """The case's finite poses as point scans (the oracle's own back-projection, gated-out pixels
    NaN) and the oracle's fusion of those frames."""
    import fuse_points_ref as FR
    from oracle import oracle as O
    O.lib()
    dims, bounds, poses, depth, _ = _case(name, geom)
    keep = np.isfinite(poses).all(axis=1)
    poses, depth = np.ascontiguousarray(poses[keep]), np.ascontiguousarray(depth[keep])
    xyz = np.stack([O.backproject(KK, depth[i], poses[i]).reshape(HH, WW, 3) for i in range(len(poses))])
    pts, origins = FR.frame_points(xyz, depth, poses, DMIN, DMAX)
    ov = Hh.oracle_grid(O, dims, bounds)
    ho, mo, so = O.fuse_depth(ov, KK, depth, poses, dmin=DMIN, dmax=DMAX)
    return pts, origins, (ho, mo, so)


def _grid(dims, bounds, variant, a_hash):
    from dmf_amd import _lib
    gv = Hh.gpu_grid(dims, bounds)
    _lib.set_variant(gv, variant)
    if a_hash:
        _lib.set_knob(gv, "a_hash", a_hash)
    return gv


def _engine():
    import dmf_amd
    return dmf_amd.RayTracingEngine(dmf_amd.Camera(KK, HH, WW)), dmf_amd.FuseParams(dmin_mm=DMIN, dmax_mm=DMAX)


VARIANTS = {"direct": (57, 0, "dmf::k_bk_fuse_s<"), "hash16": (57, 16, "dmf::k_bk_fuse_s<"),
            "lds_box": (31, 0, "dmf::k_fuse_l<")}


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("geom", list(GEOMS))
@pytest.mark.parametrize("name", ["out", "in"])
def test_frames(name, geom, variant):
    from dmf_amd import _lib
    dims, bounds, poses, depth, (ho, mo, so) = _case(name, geom)
    var, a_hash, kernel = VARIANTS[variant]
    gv = _grid(dims, bounds, var, a_hash)
    eng, prm = _engine()
    hg, mg, sg = eng.fuse_depth(gv, depth, poses, prm)
    assert _lib.kernel_name(gv).startswith(kernel)
    assert _lib.fuse_status(gv) == 0
    gv.close()
    assert np.array_equal(so, sg), (so, sg)
    assert np.array_equal(ho, hg) and np.array_equal(mo, mg)
    # the case is what it says: rays were fused, some endpoints lie outside the grid (the "in"
    # set's third pose looks out through the far face), and every gated pixel is counted
    gated = int(((depth >= DMIN) & (depth < DMAX)).sum())
    assert so[1] == gated and 0 < so[2] < gated and ho.sum() == so[2] and mo.any()


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("geom", list(GEOMS))
@pytest.mark.parametrize("name", ["out", "in"])
def test_frames_as_points(name, geom, variant):
    from dmf_amd import _lib
    dims, bounds = GEOMS[geom]
    pts, origins, (ho, mo, so) = _case_points(name, geom)
    var, a_hash, kernel = VARIANTS[variant]
    gv = _grid(dims, bounds, var, a_hash)
    eng, prm = _engine()
    hg, mg, sg = eng.fuse_points(gv, pts, origins, prm)
    assert _lib.kernel_name(gv).startswith(kernel)
    assert _lib.fuse_status(gv) == 0
    gv.close()
    assert np.array_equal(so[:3], sg[:3]), (so, sg)
    assert np.array_equal(ho, hg) and np.array_equal(mo, mg)
