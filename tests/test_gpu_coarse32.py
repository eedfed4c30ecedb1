"""Brick-pipeline fusion against the CPU oracle on the inputs pass A's 32-bit coarse walk
(dmf_brick.hpp Coarse32 / coarse_walk32) is most likely to get wrong: hit and miss counters cell
for cell, and the statistics.

(a) 256^3, 3 frames of 64x48: a camera outside the grid (every ray starts on a grid face), a
    camera on a brick corner inside the grid, and a camera whose optical axis is a grid axis.
    The intrinsics have a whole-pixel principal point and a power-of-two focal length, and the
    third pose is an exact axis permutation placed on cell boundaries, so its centre ray is
    axis-aligned, its centre row and column are planar (the +-never pairs of a non-moving axis)
    and rays run along brick edges and through brick corners (two- and three-way ties).
(b) 1024 x 256 x 256, 2 frames of 64x48 looking along x from either end: the largest |dq| the
    brick path admits and rays of more than 32 brick boundaries (past the recorded path).

Each case also runs with pass A's hashed histogram forced to 16 words, so that the hashed kernel
and, after its overflow, the recovery kernel walk the same rays.  The oracle's result is computed
once per case."""
import functools

import numpy as np
import pytest

import helpers as Hh

pytestmark = pytest.mark.gpu

HH, WW = 48, 64
KK = np.array([32, 0, 32, 0, 32, 24, 0, 0, 1], np.float32)


def _pose(xr, yd, f, eye):
    """Camera->world [R|t] with columns x right, y down, z forward."""
    M = np.concatenate([np.stack([xr, yd, f], axis=1), np.asarray(eye, np.float64)[:, None]], axis=1)
    return M.astype(np.float32).reshape(12)


def _depth(P, lo, hi, seed):
    """Depth in [lo, hi) mm with a few holes; a constant frame-centre block (equal ray lengths)."""
    rng = np.random.default_rng(seed)
    d = rng.integers(lo, hi, (P, HH, WW)).astype(np.uint16)
    d[:, 20:29, 28:37] = (lo + hi) // 2
    d[:, ::7, ::5] = 0
    return d


@functools.lru_cache(maxsize=None)
def _case(name):
    from dmf_amd import scene
    if name == "a":
        dims, bounds = (256, 256, 256), Hh.BOUNDS
        ax = np.eye(3)
        poses = np.stack([
            np.concatenate([scene.look_at((0.9, 0.1, 0.05)), np.array([[0.9], [0.1], [0.05]])], axis=1)
            .astype(np.float32).reshape(12),                 # outside: rays clipped to the x = 0.5 face
            _pose(*scene.look_at((0.125, 0.125, 0.125), (-0.3, -0.2, 0.1)).T, (0.125, 0.125, 0.125)),  # a brick corner
            _pose(ax[1], -ax[2], -ax[0], (0.625, 0.0, 0.0)),  # looking along -x from a cell boundary
        ])
        depth = _depth(3, 250, 990, 5)
    else:
        dims, bounds = (1024, 256, 256), (-0.5, 0.5, -0.5, 0.5, -0.5, 0.5)
        ax = np.eye(3)
        poses = np.stack([
            _pose(ax[1], -ax[2], ax[0], (-0.4990234375, 0.0107421875, -0.0068359375)),   # along +x, exact
            _pose(*scene.look_at((0.497, 0.21, -0.17), (-0.5, -0.3, 0.25)).T, (0.497, 0.21, -0.17)),  # along -x, oblique
        ])
        depth = _depth(2, 700, 1000, 6)
    from oracle import oracle as O
    O.lib()
    ov = Hh.oracle_grid(O, dims, bounds)
    ho, mo, so = O.fuse_depth(ov, KK, depth, poses, dmin=200, dmax=1000)
    for a in (ho, mo, so):
        a.setflags(write=False)
    return dims, bounds, poses, depth, (ho, mo, so)


def _run(name, a_hash):
    import dmf_amd
    from dmf_amd import _lib
    dims, bounds, poses, depth, (ho, mo, so) = _case(name)
    gv = Hh.gpu_grid(dims, bounds)
    _lib.set_variant(gv, _lib.FUSE_SLAB)
    _lib.set_knob(gv, "a_hash", a_hash)
    eng = dmf_amd.RayTracingEngine(dmf_amd.Camera(KK, HH, WW))
    hg, mg, sg = eng.fuse_depth(gv, depth, poses, dmf_amd.FuseParams(dmin_mm=200, dmax_mm=1000))
    assert _lib.kernel_name(gv).startswith("dmf::k_bk_fuse_s<")
    assert _lib.fuse_status(gv) == 0
    assert np.array_equal(so, sg), (so, sg)
    assert np.array_equal(ho, hg) and np.array_equal(mo, mg)
    return ho, mo, so


@pytest.mark.parametrize("a_hash", [0, 16])
def test_ties_and_sentinels_256(a_hash):
    """Case (a): every frame fuses rays (valid pixels, hits inside the grid, misses along them)."""
    ho, mo, so = _run("a", a_hash)
    valid = int((_case("a")[3] > 0).sum())
    assert so[1] == valid and so[2] > valid // 2 and ho.sum() == so[2] and mo.any()
    # the rays are not short: over 150 cell updates per valid pixel (several bricks each)
    assert so[0] > 150 * valid


@pytest.mark.parametrize("a_hash", [0, 16])
def test_long_rays_1024x256x256(a_hash):
    """Case (b): rays of ~1000 cells along x: more than 32 brick boundaries per ray."""
    ho, mo, so = _run("b", a_hash)
    valid = int((_case("b")[3] > 0).sum())
    assert so[1] == valid and so[2] > 0
    # updates per ray: the mean walk is several hundred cells long (x spans up to 1024 cells)
    assert so[0] > 400 * valid
