#!/usr/bin/env python3
"""Timing of VoxelVolume.travel_cost_map (dmf_grid_travel_cost_map) at the
size of tests/test_gpu_travel.py::test_travel_cost_map (the percolation case, 70 x 37 x 41, its 6
cells) and with 64 random cells of the same grid, against the form it replaced: one
dmf_grid_travel_device per row and V^2 device-to-host copies of 4 bytes, restated here (`old`) over
the SAME library -- so the two differ in how the entries are fetched and in nothing else; the
parent commit's library is not involved.  Host wall clock around each call, alternating, after one
warm call of each; the maps are compared.  Prints one JSON line."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "depth-map-fusion-utils_amd"), os.path.join(ROOT, "tests")]
import torch  # noqa: F401,E402
import helpers as Hh  # noqa: E402
import travel_ref as TR  # noqa: E402
from dmf_amd import NO_PATH  # noqa: E402
from dmf_amd._lib import check, ptr  # noqa: E402

dims, d2, radius2, _, _ = TR.case("percolation")
cells = TR.cost_cells()
gv = Hh.gpu_grid(dims, Hh.ODD_BOUNDS)


def old(self, dist2, radius2, cells):
    d2 = self._field(dist2, "dist2")
    c = self._cells(cells, "cells")
    V = c.shape[0]
    nx, ny, nz = self.dims
    out = np.full((V, V), 2147483647, np.int32)
    inside = ((c >= 0) & (c < np.array([nx, ny, nz]))).all(axis=1)
    flat = (c[:, 0].astype(np.int64) * ny + c[:, 1]) * nz + c[:, 2]
    bufs = []

    def alloc(nbytes):
        p = C.c_void_p()
        check(self._L.dmf_device_malloc(self._h, C.addressof(p), max(int(nbytes), 8)))
        bufs.append(p.value)
        return p.value

    try:
        d_d2, d_hops, d_seeds = alloc(d2.nbytes), alloc(d2.nbytes), alloc(c.nbytes)
        check(self._L.dmf_memcpy_h2d(self._h, d_d2, ptr(d2), d2.nbytes))
        check(self._L.dmf_memcpy_h2d(self._h, d_seeds, ptr(c), c.nbytes))
        one = np.zeros(1, np.uint32)
        for i in range(V):
            check(self._L.dmf_grid_travel_device(self._h, d_d2, int(radius2), d_seeds + 12 * i, 1, d_hops, None))
            for j in np.flatnonzero(inside):
                check(self._L.dmf_memcpy_d2h(self._h, ptr(one), d_hops + 4 * int(flat[j]), 4))
                if one[0] != NO_PATH:
                    out[i, j] = int(one[0])
    finally:
        for p in bufs:
            self._L.dmf_device_free(self._h, p)
    return out


res = {"dims": list(dims), "V": int(cells.shape[0]), "old_ms": [], "new_ms": []}
a, b = old(gv, d2, radius2, cells), gv.travel_cost_map(d2, radius2, cells)
res["equal"] = bool(np.array_equal(a, b))
for _ in range(7):
    t = time.perf_counter()
    old(gv, d2, radius2, cells)
    res["old_ms"].append(round((time.perf_counter() - t) * 1e3, 3))
    t = time.perf_counter()
    gv.travel_cost_map(d2, radius2, cells)
    res["new_ms"].append(round((time.perf_counter() - t) * 1e3, 3))
# a larger V on the same grid: 64 random cells
rng = np.random.default_rng(3)
many = np.stack([rng.integers(0, n, 64) for n in dims], axis=1).astype(np.int32)
a, b = old(gv, d2, radius2, many), gv.travel_cost_map(d2, radius2, many)
res["equal_64"] = bool(np.array_equal(a, b))
res["old_64_ms"], res["new_64_ms"] = [], []
for _ in range(5):
    t = time.perf_counter()
    old(gv, d2, radius2, many)
    res["old_64_ms"].append(round((time.perf_counter() - t) * 1e3, 3))
    t = time.perf_counter()
    gv.travel_cost_map(d2, radius2, many)
    res["new_64_ms"].append(round((time.perf_counter() - t) * 1e3, 3))
print(json.dumps(res), flush=True)
