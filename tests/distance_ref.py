"""Numpy restatement of the distance field's definition and of the segment clearance
over oracle/py_oracle.dda_cells -- TEST INFRASTRUCTURE ONLY.  The field twice: a separable min-plus
over each axis in int64 (every site against every cell of its line, no envelope), and the brute
force over the list of solid cells.  It shares no code with csrc/dmf_distance.hip.  The named cases
of tests/test_gpu_distance.py live here with their pinned totals."""
import functools
import math

import numpy as np

import fuse_points_ref as FP
from oracle import py_oracle as PO

NO_DIST = 0xFFFFFFFF
_INF = 1 << 40          # above every finite value (3 * 2047^2 < 2^24), far from int64 overflow


def solid_mask(L, dims, threshold):
    return np.asarray(L, np.int16).reshape(dims).astype(np.int64) >= int(threshold)


def edt2(L, dims, threshold):
    """-> uint32 dims: the squared distance, in cells, to the nearest cell with L >= threshold;
    NO_DIST everywhere when there is none.  out[i] = min_j f[j] + (i - j)^2 along z, y, x in turn."""
    f = np.where(solid_mask(L, dims, threshold), 0, _INF).astype(np.int64)
    for axis in (2, 1, 0):
        n = dims[axis]
        src = np.moveaxis(f, axis, 0)
        out = np.full(src.shape, _INF, np.int64)
        i = np.arange(n, dtype=np.int64).reshape((n,) + (1,) * (src.ndim - 1))
        for j in range(n):
            if (src[j] < _INF).any():
                np.minimum(out, src[j][None] + (i - j) ** 2, out=out)
        f = np.moveaxis(out, 0, axis)
    return np.where(f >= _INF, NO_DIST, f).astype(np.uint32)


def edt2_brute(L, dims, threshold):
    """The definition itself: the minimum over the list of solid cells."""
    solid = np.argwhere(solid_mask(L, dims, threshold))
    x, y, z = np.meshgrid(*(np.arange(d, dtype=np.int64) for d in dims), indexing="ij")
    best = np.full(dims, _INF, np.int64)
    for c in solid:
        np.minimum(best, (x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2, out=best)
    return np.where(best >= _INF, NO_DIST, best).astype(np.uint32)


def totals(d2, L, dims, threshold):
    """(sum of dist2, max of dist2, solid cells)."""
    return int(d2.astype(np.uint64).sum()), int(d2.max()), int(solid_mask(L, dims, threshold).sum())


def clearance(bounds, dims, dist2, a, b):
    """-> uint32 (n,): the minimum of dist2 over the cells that the ray a[i] -> b[i] updates in
    fuse_points_ref.fuse_points (the misses and the hit); NO_DIST where it updates none."""
    vol = PO.Vol(bounds, dims)
    assert tuple(vol.n) == tuple(dims)
    d = np.asarray(dist2, np.uint32).reshape(dims)
    a = np.asarray(a, np.float32).reshape(-1, 3)
    b = np.asarray(b, np.float32).reshape(-1, 3)
    out = np.full(a.shape[0], NO_DIST, np.uint32)
    for i, (O, E) in enumerate(zip(a, b)):
        if not (FP._finite3(O) and FP._finite3(E)):
            continue
        inside = vol.valid_points(E) and vol.valid_coords(vol.get_voxel(E))
        cells, hit = PO.dda_cells(vol, O, E, inside)
        if hit is not None:
            cells = cells + [hit]
        if cells:
            out[i] = min(int(d[c]) for c in cells)
    return out


# ---------------------------------------------------------------- the named cases
def _sparse(seed, dims, share=0.01):
    rng = np.random.default_rng(seed)
    return np.where(rng.random(dims) < share, 5, -3).astype(np.int16)


def _cells(dims, cells):
    L = np.full(dims, -4, np.int16)
    for c in cells:
        L[c] = 9
    return L


def _plane_x0(dims):
    L = np.full(dims, -4, np.int16)
    L[0] = np.where(np.random.default_rng(44).random(dims[1:]) < 0.05, 9, -4)
    return L


def _grid1():
    import raycast_cases as RC
    return np.asarray(RC.grid1(), np.int16).reshape(RC.DIMS1)


# name -> (dims, grid builder, threshold)
CASES = {
    "grid1_t1": ((72, 40, 44), _grid1, 1),
    "grid1_t3511": ((72, 40, 44), _grid1, 3511),
    "grid1_none": ((72, 40, 44), _grid1, 32768),
    "grid1_all": ((72, 40, 44), _grid1, -32768),
    # (seeds at which the small grids are not empty: 3, 354, 1 and 3 solid cells)
    "sparse_9_8_7": ((9, 8, 7), lambda: _sparse(102, (9, 8, 7)), 1),
    "sparse_33_17_65": ((33, 17, 65), lambda: _sparse(102, (33, 17, 65)), 1),
    "sparse_1_1_1": ((1, 1, 1), lambda: _sparse(126, (1, 1, 1)), 1),
    "sparse_2_40_3": ((2, 40, 3), lambda: _sparse(109, (2, 40, 3)), 1),
    "long_x": ((300, 3, 5), lambda: _sparse(105, (300, 3, 5)), 1),
    "long_y": ((3, 300, 5), lambda: _sparse(106, (3, 300, 5)), 1),
    "long_z": ((5, 3, 300), lambda: _sparse(107, (5, 3, 300)), 1),
    "corner_lo": ((70, 66, 130), lambda: _cells((70, 66, 130), [(0, 0, 0)]), 1),
    "corner_hi": ((70, 66, 130), lambda: _cells((70, 66, 130), [(69, 65, 129)]), 1),
    "plane_x0": ((40, 33, 70), lambda: _plane_x0((40, 33, 70)), 1),
    "column_ends": ((64, 5, 9), lambda: _cells((64, 5, 9), [(0, 2, 4), (63, 2, 4)]), 1),
    "axis_2048": ((2048, 2, 2), lambda: _cells((2048, 2, 2), [(0, 0, 0)]), 1),
    # a line of sites 30 cells away along 40 cells of x, then one site on the x column itself: in
    # the column (y, z) = (0, 0) the envelope grows 40 entries deep and the last site pops 29 of
    # them in one step
    "deep_pops": ((48, 33, 2), lambda: _cells((48, 33, 2), [(x, 30, 0) for x in range(40)] + [(40, 0, 0)]), 1),
}
# (sum of dist2, max of dist2, solid cells) of each case, by edt2_brute
TOTALS = {
    "grid1_t1": (18322881, 949, 1799),
    "grid1_t3511": (26484251, 1249, 195),
    "grid1_none": (126720 * NO_DIST, NO_DIST, 0),
    "grid1_all": (0, 0, 126720),
    "sparse_9_8_7": (6624, 59, 3),
    "sparse_33_17_65": (304996, 59, 354),
    "sparse_1_1_1": (0, 0, 1),
    "sparse_2_40_3": (14245, 329, 3),
    "long_x": (84390, 242, 48),
    "long_y": (134961, 216, 36),
    "long_z": (121314, 242, 46),
    "corner_lo": (5156851700, 25627, 1),
    "corner_hi": (5156851700, 25627, 1),
    "plane_x0": (48013880, 1570, 117),
    "column_ends": (962400, 981, 2),
    "axis_2048": (11444867072, 4190211, 1),
    "deep_pops": (578896, 901, 41),
}
# the self-check runs both forms where the brute force is quick: at most about 10^5 cells, and at
# most BRUTE_WORK cell-solid pairs (grid1_all, every cell solid and every distance 0, is left to
# its pinned totals: 1.6e10 pairs)
BRUTE_CELLS, BRUTE_WORK = 130000, 3 * 10 ** 8


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (dims, L int16 dims, threshold, dist2 uint32 dims by edt2), computed once and shared."""
    dims, build, threshold = CASES[name]
    L = np.ascontiguousarray(build(), np.int16).reshape(dims)
    d2 = edt2(L, dims, threshold)
    d2.setflags(write=False)
    L.setflags(write=False)
    return dims, L, threshold, d2


# ---------------------------------------------------------------- the clearance case
SEG_GRID_SEED = 77


@functools.lru_cache(maxsize=None)
def segment_grid():
    """int16 log-odds over fuse_points_ref.SEG_DIMS, about 2 % solid at threshold 1."""
    return _sparse(SEG_GRID_SEED, FP.SEG_DIMS, 0.02)


@functools.lru_cache(maxsize=None)
def segments():
    """-> (a (n, 3), b (n, 3)) float32 from fuse_points_ref.segment_case(): a = the scan's origin,
    b = the point (the third scan has a NaN origin)."""
    xyz, origins, _, _ = FP.segment_case()
    a = np.ascontiguousarray(np.repeat(origins[:, None, :], xyz.shape[1], axis=1).reshape(-1, 3), np.float32)
    return a, np.ascontiguousarray(xyz.reshape(-1, 3), np.float32)


@functools.lru_cache(maxsize=None)
def segment_reference():
    """-> (dist2 by edt2, clear2 by clearance) of segment_grid() and segments()."""
    d2 = edt2(segment_grid(), FP.SEG_DIMS, 1)
    a, b = segments()
    return d2, clearance(FP.SEG_BOUNDS, FP.SEG_DIMS, d2, a, b)
