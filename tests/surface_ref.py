"""Numpy restatement of the surface extraction's definition over the geometry of
oracle/py_oracle.Vol -- TEST INFRASTRUCTURE ONLY.  Integer neighbourhoods on a grid padded with 0
(unobserved), float32 arithmetic exactly as the definition orders it; it shares no code with
csrc/dmf_surface.hip."""
import functools

import numpy as np

import helpers as Hh
from oracle import py_oracle as PO

f32, f64 = np.float32, np.float64

THRESHOLDS1 = ((1, -1), (847, -405), (3511, -2000), (1, 0))     # raycast_cases.grid1()
COUNTS1 = {(1, -1): (1650, 1799), (847, -405): (1240, 1411), (3511, -2000): (177, 195), (1, 0): (1799, 1799)}
RANDOM_DIMS = ((9, 8, 7), (33, 17, 65), (1, 1, 1), (8, 8, 8), (2, 40, 3))
RANDOM_COUNTS = (201, 14956, 0, 208, 97)
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1


def vol(bounds, dims):
    v = PO.Vol(bounds, dims)
    assert tuple(v.n) == tuple(dims), (v.n, dims)
    return v


def surface(bounds, dims, L, occ_threshold, free_threshold):
    """-> dict(hash uint64 (n,), xyz float32 (n, 3), normals float32 (n, 3), cells int (n, 3),
    count (surface cells, solid cells)), the surface cells in ascending x-major cell index."""
    v = vol(bounds, dims)
    L = np.asarray(L, np.int16).reshape(dims)
    pad = np.zeros(tuple(d + 2 for d in dims), np.int32)           # a neighbour outside the grid reads as 0 ...
    pad[1:-1, 1:-1, 1:-1] = L
    free = np.zeros(pad.shape, bool)                                # ... and is never free
    free[1:-1, 1:-1, 1:-1] = L.astype(np.int64) <= int(free_threshold)
    solid = L.astype(np.int64) >= int(occ_threshold)
    inner = (slice(1, -1),) * 3

    def shifted(a, axis, d):
        s = list(inner)
        s[axis] = slice(1 + d, a.shape[axis] - 1 + d)
        return a[tuple(s)]
    near = np.zeros(dims, bool)
    for a in range(3):
        near |= shifted(free, a, -1) | shifted(free, a, 1)
    cells = np.argwhere(solid & near)                               # C order = ascending x-major index
    n = cells.shape[0]
    x, y, z = (cells[:, a].astype(np.uint64) for a in range(3))
    hashes = (x << np.uint64(40)) ^ (y << np.uint64(20)) ^ z
    xyz = np.zeros((n, 3), f32)
    for a in range(3):
        lo = (cells[:, a].astype(f64) * v.dl[a] + v.mn[a]).astype(f32)
        xyz[:, a] = (lo.astype(f64) + v.dl[a] / 2.0).astype(f32)
    g = np.stack([shifted(pad, a, -1)[tuple(cells.T)] - shifted(pad, a, 1)[tuple(cells.T)] for a in range(3)],
                 axis=1).astype(np.int32).reshape(n, 3)
    gf = g.astype(f32)
    sq = gf * gf
    s = sq[:, 0] + (sq[:, 1] + sq[:, 2])                            # Eigen's a0 + (a1 + a2), float32
    normals = np.zeros((n, 3), f32)
    nz = (g != 0).any(axis=1)
    normals[nz] = gf[nz] / np.sqrt(s[nz])[:, None]
    assert s.dtype == f32 and normals.dtype == f32
    return {"hash": hashes, "xyz": xyz, "normals": normals, "cells": cells, "g": g,
            "count": (n, int(solid.sum()))}


def random_grid(k):
    """The k-th random grid: values in -3..3 over RANDOM_DIMS[k] (one generator, drawn in order)."""
    return random_grids()[k]


@functools.lru_cache(maxsize=None)
def random_grids():
    rng = np.random.default_rng(3)
    return tuple(rng.integers(-3, 4, d).astype(np.int16) for d in RANDOM_DIMS)


@functools.lru_cache(maxsize=None)
def ref1(thresholds):
    import raycast_cases as RC
    return surface(RC.BOUNDS1, RC.DIMS1, RC.grid1(), *thresholds)


@functools.lru_cache(maxsize=None)
def ref_random(k):
    return surface(Hh.ODD_BOUNDS, RANDOM_DIMS[k], random_grid(k), 1, -1)


def round_trip_failures(bounds, dims, ref):
    """Centres that fail validPoints or do not bin back to their own cell."""
    v = vol(bounds, dims)
    bad = 0
    for p, c in zip(ref["xyz"], ref["cells"]):
        if not v.valid_points(p) or v.get_voxel(p) != tuple(int(q) for q in c):
            bad += 1
    return bad


def in_order(ref, dims):
    c = ref["cells"].astype(np.int64)
    lin = (c[:, 0] * dims[1] + c[:, 1]) * dims[2] + c[:, 2]
    return bool((np.diff(lin) > 0).all()) and bool((np.diff(ref["hash"].astype(np.int64)) > 0).all())
