"""Pure-Python restatement of the log-odds ray-cast -- TEST INFRASTRUCTURE ONLY.

Built only from what exists: py_oracle.Vol (geometry, binning, hash), py_oracle.dda_cells (the
exact DDA of DESIGN.md §4), oracle.project_point / transform_point / inverse_pose (the C++
oracle's camera arithmetic) and the voxel-centre and depth formulas of reverseRayTraceFast /
rayTraceVolume.  About 1 s per 61x37 pose on a CPU: walk() a case once and share it; surface()
over a walk is cheap.
"""
import math

import numpy as np

from oracle import py_oracle as PY

NO_CELL = np.uint64(0xFFFFFFFFFFFFFFFF)
f32, f64 = np.float32, np.float64


def sequence(vol, K, T, r, c, range_mm):
    """The probe ray's cells in walk order: the ray the fusion traces for pixel (r, c) with depth
    range_mm (missed cells in order, then the end cell when the endpoint is inside)."""
    from oracle import oracle as ORC
    p = ORC.project_point(K, r, c, range_mm)
    E = ORC.transform_point(T, p[0], p[1], p[2])
    inside = vol.valid_points(E) and vol.valid_coords(vol.get_voxel(E))
    cam = (f32(T[3]), f32(T[7]), f32(T[11]))
    missed, hit = PY.dda_cells(vol, cam, E, inside)
    return missed + ([hit] if hit is not None else [])


def cell_depth(vol, inv, cell):
    """rayTraceVolume's depth of a voxel (RayTracingEngine.hpp:519-528): int(round(zz * 1000)) with
    zz the float camera-frame z of the centre, the centre formed from the cell index as
    reverseRayTraceFast does (py_oracle.reverse_ray_trace_fast)."""
    from oracle import oracle as ORC
    x = [f32(f64(cell[a]) * vol.dl[a] + vol.mn[a]) for a in range(3)]
    cen = [f32(f64(x[a]) + vol.dl[a] / 2.0) for a in range(3)]
    zz = f32(ORC.transform_point(inv, cen[0], cen[1], cen[2])[2])
    v = float(f32(zz * f32(1000.0)))
    return int(math.floor(v + 0.5) if v >= 0 else -math.floor(-v + 0.5))


class Walk:
    """Every pixel's cell sequence for P poses of one camera over one grid."""

    def __init__(self, bounds, dims, K, H, W, poses, range_mm):
        from oracle import oracle as ORC
        self.vol = PY.Vol(bounds, dims)
        assert tuple(self.vol.n) == tuple(dims), (self.vol.n, dims)
        self.dims, self.H, self.W = tuple(dims), H, W
        self.poses = np.ascontiguousarray(poses, np.float32).reshape(-1, 12)
        self.P = self.poses.shape[0]
        K = np.asarray(K, np.float32).reshape(9)
        self.inv = [ORC.inverse_pose(T) for T in self.poses]
        self.seq = [[[sequence(self.vol, K, T, r, c, range_mm) for c in range(W)] for r in range(H)]
                    for T in self.poses]

    def cells(self):
        """The union of all walked cells."""
        return {q for sp in self.seq for sr in sp for s in sr for q in s}

    def surface(self, L, threshold):
        """-> dict(depth (P,H,W) int32, cell (P,H,W) uint64, index (P,H,W) int32: the surface
        cell's position in its ray's sequence or -1, length (P,H,W) int32: cells of the sequence,
        stats uint64[2] = {rays with a non-empty sequence, rays with a surface cell})."""
        L = np.asarray(L, np.int16).reshape(self.dims)
        shape = (self.P, self.H, self.W)
        depth = np.full(shape, -1, np.int32)
        cell = np.full(shape, NO_CELL, np.uint64)
        index = np.full(shape, -1, np.int32)
        length = np.zeros(shape, np.int32)
        for p in range(self.P):
            for r in range(self.H):
                for c in range(self.W):
                    s = self.seq[p][r][c]
                    length[p, r, c] = len(s)
                    for k, q in enumerate(s):
                        if int(L[q]) >= threshold:
                            index[p, r, c] = k
                            cell[p, r, c] = np.uint64(self.vol.hash_id(q))
                            depth[p, r, c] = cell_depth(self.vol, self.inv[p], q)
                            break
        return {"depth": depth, "cell": cell, "index": index, "length": length,
                "stats": np.array([(length > 0).sum(), (index >= 0).sum()], np.uint64)}


def unhash(h):
    """getHashId's (x, y, z) of in-grid cells (20 bits per axis)."""
    h = np.asarray(h, np.uint64)
    m = np.uint64((1 << 20) - 1)
    return ((h >> np.uint64(40)) & m).astype(np.int64), ((h >> np.uint64(20)) & m).astype(np.int64), \
        (h & m).astype(np.int64)
