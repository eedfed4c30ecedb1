"""Point fusion restated over oracle/py_oracle.py (TEST INFRASTRUCTURE ONLY).

Point i of scan s is the ray origins[s] -> xyz[s, i]: end_inside from the volume's valid_points /
get_voxel / valid_coords, the cells from dda_cells (the §4 walk for an arbitrary segment).  A point
with a non-finite coordinate is no ray, and neither is any point of a scan whose origin has one.
Pure Python: a few thousand rays per case."""
import functools
import math

import numpy as np

from oracle import py_oracle as PO


def _finite3(p):
    return all(math.isfinite(float(v)) for v in p)


def fuse_points(bounds, dims, xyz, origins, hits=None, misses=None):
    """-> (hits, misses, stats) as RayTracingEngine.fuse_points returns them: int64 counters,
    x-major over the volume's (truncated) dims, accumulated onto `hits` / `misses` when given;
    stats = [cell updates, rays, hit rays]."""
    vol = PO.Vol(bounds, dims)
    nx, ny, nz = vol.n
    xyz = np.asarray(xyz, np.float32)
    origins = np.asarray(origins, np.float32)
    if xyz.ndim == 2:
        xyz = xyz[None]
    if origins.ndim == 1:
        origins = origins[None]
    assert xyz.shape[2] == 3 and origins.shape == (xyz.shape[0], 3)
    h = np.zeros(nx * ny * nz, np.int64) if hits is None else np.array(hits, np.int64).reshape(-1)
    m = np.zeros(nx * ny * nz, np.int64) if misses is None else np.array(misses, np.int64).reshape(-1)
    assert h.size == nx * ny * nz and m.size == nx * ny * nz
    updates = rays = hit_rays = 0
    for s in range(xyz.shape[0]):
        O = origins[s]
        if not _finite3(O):
            continue
        for E in xyz[s]:
            if not _finite3(E):
                continue
            rays += 1
            inside = vol.valid_points(E) and vol.valid_coords(vol.get_voxel(E))
            missed, hit = PO.dda_cells(vol, O, E, inside)
            for c in missed:
                m[(c[0] * ny + c[1]) * nz + c[2]] += 1
            updates += len(missed)
            if hit is not None:
                h[(hit[0] * ny + hit[1]) * nz + hit[2]] += 1
                updates += 1
                hit_rays += 1
    return h, m, np.array([updates, rays, hit_rays], np.int64)


# ---------------------------------------------------------------- arbitrary segments
# 64 x 48 x 40 cells over the unit cube: no cubic cells, and only the x delta is a power of two.
# Cell corner (i, 3a, 5b) has float-exact world coordinates (j / 48 = (j / 3) / 16, k / 40 =
# (k / 5) / 8), so rays between such corners keep exact ties in the 1/256 quantisation.
SEG_DIMS = (64, 48, 40)
SEG_BOUNDS = (-0.5, 0.5, -0.5, 0.5, -0.5, 0.5)
SEG_N = 700
SEG_OUTSIDE = (0.0, 0.0, 0.9)          # scan 0: a sensor above the grid
SEG_INSIDE = (-0.125, 0.0, 0.0)        # scan 1: cell corner (24, 24, 20), inside the grid


def _corner(i, j, k):
    return (-0.5 + i / 64.0, -0.5 + j / 48.0, -0.5 + k / 40.0)


# from SEG_INSIDE: exactly diagonal through cell corners (all three axes tie at every crossing)
# (15 cells along each moving axis, in every combination of directions, and along two axes only)
SEG_DIAGONALS = (_corner(39, 39, 35), _corner(9, 9, 5), _corner(39, 9, 35), _corner(9, 39, 5), _corner(39, 39, 20),
                 _corner(24, 9, 5), _corner(9, 24, 35))


@functools.lru_cache(maxsize=None)
def segment_case():
    """-> (xyz (3, SEG_N, 3), origins (3, 3), hits0, misses0): two scans of random unordered points
    with the forced cases first, and scan 0's points again under a NaN origin; non-zero starting
    counters (int32, x-major)."""
    rng = np.random.default_rng(20)
    xyz = rng.uniform(-0.7, 0.7, (2, SEG_N, 3)).astype(np.float32)   # inside and outside the grid
    origins = np.array([SEG_OUTSIDE, SEG_INSIDE], np.float32)
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    for s in range(2):
        O = origins[s]
        forced = [(nan, 0.1, 0.1), (0.1, inf, 0.1), (0.1, 0.1, -inf), (nan, nan, nan), (-inf, inf, nan),
                  (0.8, 0.0, 0.0), (-0.8, 0.0, 0.0), (0.0, 0.8, 0.0), (0.0, -0.8, 0.0), (0.0, 0.0, 0.8), (0.0, 0.0, -0.8),
                  tuple(O),                                         # E == O
                  (O[0] + 0.001, O[1] + 0.001, O[2] + 0.001),       # E in the origin's cell
                  (0.4, O[1], O[2]), (O[0], 0.4, O[2]), (O[0], O[1], 0.3), (-0.45, O[1], O[2]),   # axis-parallel
                  (O[0], O[1], -0.45), (0.9, O[1], O[2]),
                  (0.9, 0.0, 0.9), (0.9, 0.9, 0.9),                 # from above the grid: misses it
                  (0.5, 0.1, 0.1), (0.1, -0.5, 0.1), (0.49999997, 0.1, 0.1)]   # on / next to the bounds
        forced += list(SEG_DIAGONALS)
        xyz[s, :len(forced)] = np.array(forced, np.float32)
    xyz = np.concatenate([xyz, xyz[:1]])
    origins = np.concatenate([origins, np.array([[0.0, nan, 0.9]], np.float32)])
    n = int(np.prod(SEG_DIMS))
    return (np.ascontiguousarray(xyz), np.ascontiguousarray(origins), rng.integers(0, 5, n).astype(np.int32),
            rng.integers(0, 9, n).astype(np.int32))


@functools.lru_cache(maxsize=None)
def segment_reference():
    """The restatement's counters and statistics of segment_case(), onto its starting counters."""
    xyz, origins, h0, m0 = segment_case()
    return fuse_points(SEG_BOUNDS, SEG_DIMS, xyz, origins, h0, m0)


def quantised(bounds, dims, p):
    """floor(256 x grid coordinate) of a float32 point, per axis, as dda_cells computes it for a
    point inside the grid."""
    vol = PO.Vol(bounds, dims)
    return [int(math.floor((PO.f64(np.float32(p[a])) - vol.mn[a]) / vol.dl[a] * 256)) for a in range(3)]


def frame_points(xyz, depth, poses, dmin, dmax):
    """The point form of depth frames: xyz (P, H, W, 3) their back-projection, pixels outside the
    depth gate [dmin, dmax) set to NaN -> (points (P, H*W, 3) float32, origins (P, 3) = the poses'
    translation columns)."""
    depth = np.asarray(depth)
    pts = np.array(xyz, np.float32).reshape(depth.shape[0], -1, 3)
    gate = ((depth >= dmin) & (depth < dmax)).reshape(depth.shape[0], -1)
    pts[~gate] = np.nan
    origins = np.ascontiguousarray(np.asarray(poses, np.float32).reshape(-1, 12)[:, 3::4])
    return np.ascontiguousarray(pts), origins
