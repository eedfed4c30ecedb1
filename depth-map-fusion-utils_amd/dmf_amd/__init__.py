"""dmf_amd — Python mirror of the reference Camera / VoxelVolume / RayTracingEngine
API (include/Camera.hpp, include/Volume.hpp, include/RayTracingEngine.hpp of
REXJJ/depth-map-fusion-utils) over the MI355X C ABI in libdmf.so.

Same class and method names, argument meaning and defaults as the reference, so
code written against the reference reads the same:

    cam = Camera(K)                                  # Camera.hpp:23
    volume = VoxelVolume()
    volume.setDimensions(xmin, xmax, ymin, ymax, zmin, zmax)
    volume.setVolumeSize(nx, ny, nz); volume.constructVolume()
    volume.integratePointCloud(xyz, normals)         # Volume.hpp:199-228
    engine = RayTracingEngine(cam)
    found, good = engine.reverseRayTraceFast(volume, pose, True)   # :136-226

Batched extensions (reverseRayTraceFastBatch, fuse_depth, ...) expose the GPU's
pose-parallelism.  Every compute call runs on the GPU through libdmf.so; there
is no CPU fallback.
"""
from __future__ import annotations

import collections
import ctypes as C

import numpy as np

from . import _lib
from ._lib import DmfError, check, load, ptr

__all__ = ["Camera", "VoxelVolume", "RayTracingEngine", "OccupancyGrid", "DmfError", "degree", "FuseParams"]

# RayTracingEngine.raycast_logodds: the cell value of a pixel whose ray finds no solid cell
# (DMF_NO_CELL, include/dmf.h; no getHashId is all ones)
NO_CELL = np.uint64(0xFFFFFFFFFFFFFFFF)
# VoxelVolume.distance_field / segment_clearance: no solid cell in the grid / no cell on the segment
# (DMF_NO_DIST, include/dmf.h; no squared distance in a grid of at most 2048 cells per axis is all ones)
NO_DIST = np.uint32(0xFFFFFFFF)
# VoxelVolume.travel_field: a cell that is not traversable or not reachable (DMF_NO_PATH, include/dmf.h;
# a grid of at most 2^31 cells has no hop count of all ones)
NO_PATH = np.uint32(0xFFFFFFFF)
# VoxelVolume.cloud_nearest: the index of a query that has no neighbour (DMF_NO_POINT, include/dmf.h)
NO_POINT = -1

CloudError = collections.namedtuple("CloudError", "n_valid max_error avg_error over dist2")
SurfaceError = collections.namedtuple("SurfaceError", "n_surface n_valid max_error avg_error over dist2")


def degree(radian):
    """CommonUtilities.hpp:17 degree(): int((radian*180)/3.14159)."""
    v = (float(radian) * 180) / 3.14159
    return int(v) if -2147483648.0 <= v < 2147483648.0 else -2147483648


class Camera:
    """Camera.hpp:17-86.  Scalar helpers are the reference formulas on the host;
    the per-pixel hot path (back-projection of whole frames) runs on the GPU."""

    def __init__(self, K, height=480, width=640):
        self.K_ = np.asarray(K, np.float32).reshape(9).copy()
        self.height_ = int(height)
        self.width_ = int(width)
        self._c = _lib.make_camera(self.K_, self.height_, self.width_)

    def getHeight(self):
        return self.height_

    def getWidth(self):
        return self.width_

    def validPixel(self, r, c):
        return 0 <= r < self.height_ and 0 <= c < self.width_

    def projectPoint(self, r, c, depth_mm):
        """Camera.hpp:24-31 (double math, float result)."""
        fx, cx, fy, cy = (float(self.K_[i]) for i in (0, 2, 4, 5))
        z = depth_mm * 0.001
        x = z * (float(c) - cx) / fx
        y = z * (float(r) - cy) / fy
        return np.float32(x), np.float32(y), np.float32(z)

    getPoint = projectPoint

    def deProjectPoint(self, x, y, z):
        """Camera.hpp:32-38: int(round((x*fx)/z + cx)) in double (C round: half away from 0)."""
        fx, cx, fy, cy = (float(self.K_[i]) for i in (0, 2, 4, 5))

        def cround_int(v):
            if not np.isfinite(v):
                return -2147483648
            v = float(np.sign(v) * np.floor(abs(v) + 0.5))
            return int(v) if -2147483648.0 <= v < 2147483648.0 else -2147483648

        with np.errstate(all="ignore"):
            c = cround_int(np.float64(x) * fx / np.float64(z) + cx)
            r = cround_int(np.float64(y) * fy / np.float64(z) + cy)
        return r, c

    def transformPoints(self, x, y, z, transformation):
        """Camera.hpp:39-45 (Eigen float affine, sum order a0+(a1+a2))."""
        m = np.asarray(transformation, np.float32).reshape(12)
        p = np.array([x, y, z], np.float32)
        out = []
        for i in range(3):
            s = m[4 * i + 0] * p[0] + (m[4 * i + 1] * p[1] + m[4 * i + 2] * p[2])
            out.append(np.float32(m[4 * i + 3] + s))
        return tuple(out)

    def getPixel(self, x, y, z, transformation=None):
        if transformation is None:
            transformation = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32)
        x, y, z = self.transformPoints(x, y, z, transformation)
        return self.deProjectPoint(x, y, z)

    def getAreaCovered(self, depth_mm):
        x1, y1, _ = (float(v) for v in self.getPoint(0, 0, depth_mm))
        x2, y2, _ = (float(v) for v in self.getPoint(0, self.height_, depth_mm))
        x3, y3, _ = (float(v) for v in self.getPoint(self.width_, 0, depth_mm))
        d = lambda a, b, c, e: np.sqrt((a - c) ** 2 + (b - e) ** 2)
        return np.float32(d(x1, y1, x2, y2) * d(x1, y1, x3, y3))

    def getDistance(self, depth_mm):
        x1, y1, _ = (float(v) for v in self.getPoint(100, 100, depth_mm))
        x2, y2, _ = (float(v) for v in self.getPoint(101, 101, depth_mm))
        return np.float32(np.sqrt((x1 - x2) ** 2 + (y1 - y2) ** 2))


def _unpack_view_mask(mask, dims):
    """VoxelVolume.view_mask_dense over explicit grid dimensions (numpy only)."""
    nx, ny, nz = (int(d) for d in dims)
    tx, ty, tz = (nx + 7) // 8, (ny + 7) // 8, (nz + 7) // 8
    m = np.ascontiguousarray(mask, np.uint64).reshape(-1)
    if m.size != 8 * tx * ty * tz:
        raise ValueError(f"mask must hold {8 * tx * ty * tz} uint64 words, got {m.size}")
    bits = np.unpackbits(m.astype("<u8").view(np.uint8), bitorder="little").astype(bool)
    # (tile x, tile y, tile z, x & 7, y & 7, z & 7) -> (x, y, z)
    cells = bits.reshape(tx, ty, tz, 8, 8, 8).transpose(0, 3, 1, 4, 2, 5).reshape(tx * 8, ty * 8, tz * 8)
    return np.ascontiguousarray(cells[:nx, :ny, :nz])


class VoxelVolume:
    """Volume.hpp:50-255 VoxelVolume, device-resident (flat occupancy bitmask,
    dense slot map, occupied_cells_ list, CSR per-voxel points/normals)."""

    def __init__(self, device=0):
        self._L = load()
        h = C.c_void_p()
        check(self._L.dmf_volume_create(C.addressof(h), int(device)))
        self._h = h
        self._fields = {}

    def close(self):
        if getattr(self, "_h", None):
            self._L.dmf_volume_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- setup (Volume.hpp:89-128)
    def setDimensions(self, xmin, xmax, ymin, ymax, zmin, zmax):
        check(self._L.dmf_volume_set_dimensions(self._h, xmin, xmax, ymin, ymax, zmin, zmax))

    def setResolution(self, xdelta, ydelta, zdelta):
        check(self._L.dmf_volume_set_resolution(self._h, xdelta, ydelta, zdelta))

    def setVolumeSize(self, xdim, ydim, zdim):
        check(self._L.dmf_volume_set_volume_size(self._h, int(xdim), int(ydim), int(zdim)))

    def constructVolume(self):
        check(self._L.dmf_volume_construct(self._h))
        return True

    def set_stream(self, stream_ptr):
        check(self._L.dmf_volume_set_stream(self._h, stream_ptr))

    def set_fuse_input_stream(self, stream_ptr):
        """Pipelined fusion (dmf_fuse_set_input_stream): the device inputs of later fusion
        calls are ordered on stream_ptr; None restores the serial order."""
        check(self._L.dmf_fuse_set_input_stream(self._h, stream_ptr))

    def synchronize(self):
        check(self._L.dmf_volume_synchronize(self._h))

    def info(self):
        i = _lib.dmf_volume_info()
        check(self._L.dmf_volume_get_info(self._h, C.addressof(i)))
        return {f: getattr(i, f) for f, _ in i._fields_}

    def __getattr__(self, name):
        # public fields of the reference: xmin_, xdelta_, xdim_, hsize_, voxel_size_ ...
        if name.endswith("_") and not name.startswith("_"):
            key = name[:-1]
            inf = self.info()
            if key in inf:
                return inf[key]
        raise AttributeError(name)

    @property
    def dims(self):
        i = self.info()
        return i["xdim"], i["ydim"], i["zdim"]

    # -- view-gain masks
    def view_gain_words(self):
        """uint64 words of one pose's view mask (dmf_view_gain_words)."""
        w = C.c_int64(0)
        check(self._L.dmf_view_gain_words(self._h, C.addressof(w)))
        return w.value

    def view_mask_dense(self, mask):
        """One pose's view mask (words uint64, RayTracingEngine.view_gain(masks=True)) -> bool
        (xdim, ydim, zdim).  Layout: cell (x, y, z) is bit i & 63 of word i >> 6 with
        i = tile << 9 | (x & 7) << 6 | (y & 7) << 3 | (z & 7), 8x8x8-cell tiles x-major over the
        grid padded to whole tiles."""
        return _unpack_view_mask(mask, self.dims)

    # -- hashing helpers (Volume.hpp:135-170, 230-233): host formulas
    def getHashId(self, x, y, z):
        return ((int(x) << 40) ^ ((int(y) << 20) & 0xFFFFFFFFFFFFFFFF) ^ int(z)) & 0xFFFFFFFFFFFFFFFF

    def getVoxel(self, x, y, z):
        i = self.info()
        f = lambda v, lo, d: int(np.floor((np.float64(np.float32(v)) - lo) / d))
        return f(x, i["xmin"], i["xdelta"]), f(y, i["ymin"], i["ydelta"]), f(z, i["zmin"], i["zdelta"])

    def getHash(self, x, y, z):
        return self.getHashId(*self.getVoxel(x, y, z))

    @staticmethod
    def getVoxelCoords(h):
        h = int(h)
        return h >> 40, (h >> 20) & ((1 << 20) - 1), h & ((1 << 20) - 1)

    def validCoords(self, x, y, z):
        nx, ny, nz = self.dims
        return 0 <= x < nx and 0 <= y < ny and 0 <= z < nz

    def validPoints(self, x, y, z):
        i = self.info()
        x, y, z = (np.float64(np.float32(v)) for v in (x, y, z))
        return not (x >= i["xmax"] or y >= i["ymax"] or z >= i["zmax"] or x <= i["xmin"] or y <= i["ymin"]
                    or z <= i["zmin"])

    # -- fusion of a point cloud (Volume.hpp:172-228), on the GPU
    def integratePointCloud(self, cloud, normals=None):
        xyz = np.ascontiguousarray(cloud, np.float32).reshape(-1, 3)
        nrm = None
        if normals is not None:
            nrm = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
            if nrm.shape != xyz.shape:
                raise ValueError("normals must match the cloud")
        nb = C.c_int64(0)
        hz = C.c_int64(0)
        check(self._L.dmf_volume_integrate(self._h, ptr(xyz), ptr(nrm), xyz.shape[0], C.addressof(nb),
                                           C.addressof(hz)))
        return True

    def integrate_device(self, d_xyz, d_normals, n):
        check(self._L.dmf_volume_integrate_device(self._h, d_xyz, d_normals, int(n)))

    # -- surface of a fused log-odds grid, on the GPU
    def _logodds(self, logodds):
        n = int(np.prod(self.dims))
        lo = np.asarray(logodds)
        if lo.dtype != np.int16 or lo.size != n:
            raise ValueError(f"logodds must be int16 with {n} cells (x-major over dims {tuple(self.dims)}), "
                             f"got {lo.dtype} with {lo.size}")
        return np.ascontiguousarray(lo).reshape(-1)

    def extract_surface(self, logodds, occ_threshold=1, free_threshold=-1):
        """The surface cells of the int16 log-odds grid `logodds` (xdim*ydim*zdim cells, x-major, as
        fuse_finalize returns it) -> (hash uint64 (n,), xyz float32 (n, 3), normals float32 (n, 3)),
        in ascending getHashId: the cells with log-odds >= occ_threshold that have a face neighbour
        with log-odds <= free_threshold, their voxel centres and normals towards free space.  The
        volume's point-cloud occupancy is not touched."""
        lo = self._logodds(logodds)
        n = C.c_int64(0)
        args = (self._h, ptr(lo), int(occ_threshold), int(free_threshold))
        check(self._L.dmf_grid_surface(*args, None, None, None, 0, C.addressof(n), None))
        m = n.value
        h, xyz, nrm = np.zeros(m, np.uint64), np.zeros((m, 3), np.float32), np.zeros((m, 3), np.float32)
        if m:
            check(self._L.dmf_grid_surface(*args, ptr(h), ptr(xyz), ptr(nrm), m, C.addressof(n), None))
        return h, xyz, nrm

    def integrate_surface(self, logodds, occ_threshold=1, free_threshold=-1):
        """integratePointCloud(cloud, normals) of extract_surface's cloud without leaving the
        device -> the number of surface cells."""
        lo = self._logodds(logodds)
        n = C.c_int64(0)
        check(self._L.dmf_volume_integrate_surface(self._h, ptr(lo), int(occ_threshold), int(free_threshold),
                                                   C.addressof(n)))
        return n.value

    # -- distance field of a fused log-odds grid and segment clearance, on the GPU
    def distance_field(self, logodds, threshold=1):
        """The exact squared Euclidean distance field of the int16 log-odds grid `logodds`
        (xdim*ydim*zdim cells, x-major, as fuse_finalize returns it) -> uint32 (xdim, ydim, zdim):
        per cell the least (x-x')^2 + (y-y')^2 + (z-z')^2 over the solid cells (log-odds >=
        threshold), 0 on solid cells, NO_DIST everywhere when no cell is solid.  Threshold 1 makes
        the observed-occupied cells the obstacles; 0 also counts unobserved cells (conservative).
        The unit is the cell index, so the field is exact for every volume: with cubic voxels the
        distance in metres is sqrt(d2) * delta, with anisotropic ones sqrt(d2) * min(delta) is a
        lower bound.  The volume's point-cloud occupancy is not touched."""
        lo = self._logodds(logodds)
        out = np.empty(tuple(self.dims), np.uint32)
        check(self._L.dmf_grid_distance(self._h, ptr(lo), int(threshold), ptr(out), None))
        return out

    def segment_clearance(self, dist2, a, b):
        """The clearance of the segments a[i] -> b[i] (float32 world-frame points, (n, 3) or (3,)) in
        the field `dist2` of distance_field (uint32, xdim*ydim*zdim cells) -> uint32 (n,): the
        minimum of dist2 over the cells the ray with origin a[i] and endpoint b[i] updates in
        fuse_points (only the part inside the grid); NO_DIST for a segment that visits no cell (a
        non-finite coordinate, or it misses the grid).  A body of radius r cells collides on
        segment i iff the result is < r * r."""
        n = int(np.prod(self.dims))
        d2 = np.asarray(dist2)
        if d2.dtype != np.uint32 or d2.size != n:
            raise ValueError(f"dist2 must be uint32 with {n} cells (x-major over dims {tuple(self.dims)}), "
                             f"got {d2.dtype} with {d2.size}")
        d2 = np.ascontiguousarray(d2).reshape(-1)
        pa, pb = (np.ascontiguousarray(p, np.float32) for p in (a, b))
        if pa.shape != pb.shape or pa.ndim not in (1, 2) or pa.shape[-1] != 3:
            raise ValueError(f"a and b must both be (n, 3) or (3,), got {pa.shape} and {pb.shape}")
        pa, pb = pa.reshape(-1, 3), pb.reshape(-1, 3)
        out = np.empty(pa.shape[0], np.uint32)
        check(self._L.dmf_grid_clearance(self._h, ptr(d2), ptr(pa), ptr(pb), pa.shape[0], ptr(out)))
        return out

    # -- travel field over a distance field, the path back and the travel cost map, on the GPU
    def _field(self, a, name):
        n = int(np.prod(self.dims))
        f = np.asarray(a)
        if f.dtype != np.uint32 or f.size != n:
            raise ValueError(f"{name} must be uint32 with {n} cells (x-major over dims {tuple(self.dims)}), "
                             f"got {f.dtype} with {f.size}")
        return np.ascontiguousarray(f).reshape(-1)

    @staticmethod
    def _cells(a, name):
        c = np.asarray(a)
        if c.dtype.kind not in "iu" or c.ndim != 2 or c.shape[1] != 3:
            raise ValueError(f"{name} must be integer cell indices of shape (n, 3), got {c.dtype} {c.shape}")
        return np.ascontiguousarray(c, np.int32)

    def travel_field(self, dist2, radius2, seeds, info=False):
        """The travel field of the seed cells `seeds` (integers, (n, 3)) over the field `dist2` of
        distance_field -> uint32 (xdim, ydim, zdim): per cell the least number of face-to-face steps
        from any valid seed through cells with dist2 >= radius2 (both ends included), 0 on a valid
        seed, NO_PATH where a cell is not traversable or not reachable.  Seeds outside the grid or
        on blocked cells are ignored.  Steps cross faces only: a hop count over-estimates the
        Euclidean length, in cells, by up to sqrt(3).  info=True also returns (traversable cells,
        reached cells, largest finite hop count)."""
        d2 = self._field(dist2, "dist2")
        s = self._cells(seeds, "seeds")
        if not 0 <= int(radius2) <= 0xFFFFFFFF:
            raise ValueError(f"radius2 must fit uint32, got {radius2}")
        out = np.empty(tuple(self.dims), np.uint32)
        cnt = np.zeros(3, np.uint64)
        check(self._L.dmf_grid_travel(self._h, ptr(d2), int(radius2), ptr(s) if s.shape[0] else None, s.shape[0],
                                      ptr(out), ptr(cnt)))
        return (out, tuple(int(c) for c in cnt)) if info else out

    def path_to(self, hops, target):
        """The path from the cell `target` back to a seed in the field `hops` of travel_field ->
        int32 (n, 3), target first: n = hops[target] + 1 cells, each step to the first face
        neighbour in the order -x +x -y +y -z +z that holds one hop less; (0, 3) for a target
        outside the grid or with NO_PATH."""
        h = self._field(hops, "hops")
        t = np.asarray(target)
        if t.dtype.kind not in "iu" or t.shape != (3,):
            raise ValueError(f"target must be one integer cell index (3,), got {t.dtype} {t.shape}")
        t = np.ascontiguousarray(t, np.int32)
        nx, ny, nz = self.dims
        if not (0 <= t[0] < nx and 0 <= t[1] < ny and 0 <= t[2] < nz):
            return np.zeros((0, 3), np.int32)
        k = int(h[(int(t[0]) * ny + int(t[1])) * nz + int(t[2])])
        if k == int(NO_PATH):
            return np.zeros((0, 3), np.int32)
        out = np.zeros((min(k + 1, h.size), 3), np.int32)
        n = C.c_int64(0)
        check(self._L.dmf_grid_path(self._h, ptr(h), ptr(t), ptr(out), out.shape[0], C.addressof(n)))
        return out[:n.value]

    def travel_cost_map(self, dist2, radius2, cells):
        """The V x V travel cost map of the cells `cells` (integers, (V, 3)) -> int32 (V, V):
        entry [i][j] = the hop count from cells[i] to cells[j] through cells with dist2 >= radius2,
        INT_MAX where there is no path -- the fused grid's counterpart of collisionCostMap, with
        detours.  One travel field per row, made on the device into one reused buffer, and a gather
        of the row's V entries; the map comes back in one copy."""
        d2 = self._field(dist2, "dist2")
        c = self._cells(cells, "cells")
        if not 0 <= int(radius2) <= 0xFFFFFFFF:
            raise ValueError(f"radius2 must fit uint32, got {radius2}")
        V = c.shape[0]
        out = np.full((V, V), 2147483647, np.int32)
        if V:
            check(self._L.dmf_grid_travel_cost_map(self._h, ptr(d2), int(radius2), ptr(c), V, ptr(out)))
        return out

    # -- exact nearest neighbour between clouds and the cloud error, on the GPU
    @staticmethod
    def _cloud(a, name):
        p = np.asarray(a)
        if p.dtype != np.float32 and not (p.dtype.kind in "fiu" and np.can_cast(p.dtype, np.float32, "safe")):
            raise ValueError(f"{name} must be float32 (or a type that float32 holds exactly), got {p.dtype}")
        if p.ndim != 2 or p.shape[1] != 3:
            raise ValueError(f"{name} must have shape (n, 3), got {p.shape}")
        return np.ascontiguousarray(p, np.float32)

    @staticmethod
    def _thresholds(thresholds):
        t = np.asarray(list(thresholds), np.float64).reshape(-1)
        if t.size > 8:
            raise ValueError(f"at most 8 thresholds, got {t.size}")
        if not (t >= 0).all():
            raise ValueError(f"thresholds must be non-negative, got {t.tolist()}")
        return t

    def cloud_nearest(self, query, ref):
        """For every point of `query` (float32 (n, 3)) its exact nearest neighbour in `ref` (float32
        (m, 3)) -> (dist2 float32 (n,), index int32 (n,)): the least d2 = (dx*dx + dy*dy) + dz*dz in
        float32 over the reference points with finite coordinates and the lowest index that attains
        it; +inf and NO_POINT for a query with a non-finite coordinate, and for every query when the
        reference has no valid point.  What ErrorCalc.cpp asks of PCL's k-d tree, for all points in
        one call.  The volume only lends its device, stream and scratch: it need not be constructed."""
        q, r = self._cloud(query, "query"), self._cloud(ref, "ref")
        n = q.shape[0]
        d2, idx = np.empty(n, np.float32), np.empty(n, np.int32)
        if n:
            check(self._L.dmf_cloud_nearest(self._h, ptr(q), n, ptr(r) if r.shape[0] else None, r.shape[0], ptr(d2),
                                            ptr(idx), None, 0, None, None))
        return d2, idx

    def cloud_error(self, query, ref, thresholds=(0.003, 0.005)):
        """The error of the cloud `query` against the model cloud `ref` as tests/ErrorCalc.cpp:74-97
        reports it -> CloudError(n_valid, max_error, avg_error, over, dist2): the queries that have a
        neighbour, the largest and the mean of their distances sqrtf(dist2), how many of them lie
        beyond each threshold (metres; the reference marks 3 mm and 5 mm), and dist2 (float32 (n,))
        of cloud_nearest.  avg_error is formed as the reference's loop forms it: sqrtf in float,
        accumulated in a double in index order, divided by n_valid (nan when that is 0); max_error is
        -1.0 when n_valid is 0, the reference's initial value."""
        q, r = self._cloud(query, "query"), self._cloud(ref, "ref")
        t = self._thresholds(thresholds)
        n = q.shape[0]
        d2 = np.empty(n, np.float32)
        cnt, sums = np.zeros(2 + t.size, np.uint64), np.zeros(2, np.float64)
        check(self._L.dmf_cloud_nearest(self._h, ptr(q) if n else None, n, ptr(r) if r.shape[0] else None, r.shape[0],
                                        ptr(d2) if n else None, None, ptr(t) if t.size else None, t.size, ptr(cnt),
                                        ptr(sums)))
        # a query has a neighbour iff it is valid and the reference has a valid point
        has = np.isfinite(q).all(axis=1) if int(cnt[1]) else np.zeros(n, bool)
        nv = int(cnt[0])
        dist = np.sqrt(d2[has]).astype(np.float64)
        avg = float(np.cumsum(dist)[-1] / nv) if nv else float("nan")
        return CloudError(nv, float(sums[0]), avg, tuple(int(c) for c in cnt[2:]), d2)

    def surface_error(self, logodds, ref, occ_threshold=1, free_threshold=-1, thresholds=(0.003, 0.005),
                      per_point=False):
        """The error of the fused grid's surface (extract_surface's voxel centres, in its order)
        against the model cloud `ref`, without the surface leaving the device ->
        SurfaceError(n_surface, n_valid, max_error, avg_error, over, dist2): only the surface count
        and the summaries come back, and dist2 (float32 (n_surface,)) with per_point=True (else
        None).  avg_error is the device's sum of the distances over n_valid (its order of additions
        is unspecified; nan when n_valid is 0)."""
        lo = self._logodds(logodds)
        r = self._cloud(ref, "ref")
        t = self._thresholds(thresholds)
        args = (int(occ_threshold), int(free_threshold))
        bufs = []

        def alloc(nbytes):
            p = C.c_void_p()
            check(self._L.dmf_device_malloc(self._h, C.addressof(p), max(int(nbytes), 8)))
            bufs.append(p.value)
            return p.value

        try:
            d_grid, d_count, d_ref = alloc(lo.nbytes), alloc(16), alloc(r.nbytes)
            check(self._L.dmf_memcpy_h2d(self._h, d_grid, ptr(lo), lo.nbytes))
            if r.nbytes:
                check(self._L.dmf_memcpy_h2d(self._h, d_ref, ptr(r), r.nbytes))
            # the count first (capacity 0: nothing is written), then the centres into a buffer of that size
            count = np.zeros(2, np.uint64)
            check(self._L.dmf_grid_surface_device(self._h, d_grid, *args, None, alloc(8), None, 0, d_count))
            check(self._L.dmf_memcpy_d2h(self._h, ptr(count), d_count, 16))
            n = int(count[0])
            d_xyz = alloc(12 * n)
            if n:
                check(self._L.dmf_grid_surface_device(self._h, d_grid, *args, None, d_xyz, None, n, d_count))
            d_d2 = alloc(4 * n) if per_point and n else None
            d_cnt, d_sums = alloc(8 * (2 + t.size)), alloc(16)
            check(self._L.dmf_cloud_nearest_device(self._h, d_xyz if n else None, n, d_ref if r.shape[0] else None,
                                                   r.shape[0], d_d2, None, ptr(t) if t.size else None, t.size, d_cnt,
                                                   d_sums))
            cnt, sums = np.zeros(2 + t.size, np.uint64), np.zeros(2, np.float64)
            check(self._L.dmf_memcpy_d2h(self._h, ptr(cnt), d_cnt, cnt.nbytes))
            check(self._L.dmf_memcpy_d2h(self._h, ptr(sums), d_sums, sums.nbytes))
            d2 = None
            if per_point:
                d2 = np.empty(n, np.float32)
                if n:
                    check(self._L.dmf_memcpy_d2h(self._h, ptr(d2), d_d2, d2.nbytes))
        finally:
            for p in bufs:
                self._L.dmf_device_free(self._h, p)
        nv = int(cnt[0])
        return SurfaceError(n, nv, float(sums[0]), float(sums[1]) / nv if nv else float("nan"),
                            tuple(int(c) for c in cnt[2:]), d2)

    # -- candidate views: voxel-grid downsample, camera placement and the chain over a fused grid
    #    (DESIGN.md §4.9), on the GPU
    @staticmethod
    def _leaf(leaf):
        l = np.asarray(leaf)
        if l.dtype.kind not in "fiu" or l.shape not in ((), (3,)):
            raise ValueError(f"leaf must be one number or three, got {l.dtype} {l.shape}")
        l = np.ascontiguousarray(np.broadcast_to(l.astype(np.float32), (3,)))
        if not (np.isfinite(l).all() and (l > 0).all()):
            raise ValueError(f"leaf must be finite and > 0 in float32, got {l.tolist()}")
        return l

    def cloud_downsample(self, xyz, leaf, normals=None, unit_normals=False):
        """PCL's VoxelGrid over the cloud `xyz` (float32 (n, 3)) with `normals` (float32 (n, 3) or
        None), as PointCloudProcessing::downsample runs it -> (xyz float32 (m, 3), normals float32
        (m, 3) or None, points int32 (m,)): one entry per non-empty leaf of size `leaf` (one number or
        three), in ascending leaf index, holding the float32 mean of the leaf's points (summed in
        input order) and their number; bit for bit the drop-in's host VoxelGrid.  Points with a
        non-finite coordinate are skipped.  unit_normals=True renormalises the mean normals (PCL >=
        1.8).  A grid of more than 2^31 - 1 leaves raises DmfError (DMF_ERR_RANGE).  The volume only
        lends its device, stream and scratch: it need not be constructed."""
        p = self._cloud(xyz, "xyz")
        l = self._leaf(leaf)
        nn = None
        if normals is not None:
            nn = self._cloud(normals, "normals")
            if nn.shape != p.shape:
                raise ValueError(f"normals must have xyz's shape {p.shape}, got {nn.shape}")
        n = p.shape[0]
        flags = 1 if unit_normals else 0
        cnt = np.zeros(3, np.uint64)
        args = (self._h, ptr(p) if n else None, ptr(nn) if n and nn is not None else None, n, ptr(l), flags)
        check(self._L.dmf_cloud_downsample(*args, None, None, None, 0, ptr(cnt)))
        m = int(cnt[0])
        ox, on, op = np.zeros((m, 3), np.float32), np.zeros((m, 3), np.float32), np.zeros(m, np.int32)
        if m:
            check(self._L.dmf_cloud_downsample(*args, ptr(ox), ptr(on) if nn is not None else None, ptr(op), m,
                                               ptr(cnt)))
        return ox, (on if nn is not None else None), op

    def surface_views(self, logodds, leaf, distance_mm=300, occ_threshold=1, free_threshold=-1, unit_normals=False,
                      flip=True):
        """Candidate camera poses for the fused grid `logodds` without the surface leaving the
        device: extract_surface -> cloud_downsample(leaf) -> position_cameras(distance_mm, flip) ->
        (poses float32 (m, 3, 4), xyz float32 (m, 3), normals float32 (m, 3)): the poses, the
        candidate locations and their normals as the placement left them.  The poses can go
        straight into RayTracingEngine.view_gain / next_best_views on the same grid.  flip=False
        keeps normals that face down (a fused grid has such surfaces; the reference's table-top
        scans do not)."""
        lo = self._logodds(logodds)
        l = self._leaf(leaf)
        if not 0 <= int(distance_mm) <= 0xFFFFFFFF:
            raise ValueError(f"distance_mm must fit uint32, got {distance_mm}")
        cnt = np.zeros(3, np.uint64)
        args = (self._h, ptr(lo), int(occ_threshold), int(free_threshold), ptr(l), 1 if unit_normals else 0,
                int(distance_mm), 0 if flip else 1)
        check(self._L.dmf_grid_surface_views(*args, None, None, None, 0, ptr(cnt)))
        m = int(cnt[0])
        poses, xyz, nrm = np.zeros((m, 3, 4), np.float32), np.zeros((m, 3), np.float32), np.zeros((m, 3), np.float32)
        if m:
            check(self._L.dmf_grid_surface_views(*args, ptr(poses), ptr(xyz), ptr(nrm), m, ptr(cnt)))
        return poses, xyz, nrm

    @property
    def occupied_cells_(self):
        n = C.c_int64(0)
        check(self._L.dmf_volume_occupied(self._h, None, 0, C.addressof(n)))
        out = np.zeros(max(n.value, 1), np.uint64)
        check(self._L.dmf_volume_occupied(self._h, ptr(out), out.size, C.addressof(n)))
        return out[:n.value]

    def voxel_flags(self):
        """(view int32, good uint8) per occupied voxel in occupied_cells_ order."""
        V = self.info()["num_occupied"]
        view = np.zeros(max(V, 1), np.int32)
        good = np.zeros(max(V, 1), np.uint8)
        check(self._L.dmf_volume_voxel_flags(self._h, ptr(view), ptr(good), view.size))
        return view[:V], good[:V]

    def reset_flags(self):
        check(self._L.dmf_volume_reset_flags(self._h))

    def voxel_counts(self):
        V = self.info()["num_occupied"]
        a = np.zeros(max(V, 1), np.int64)
        b = np.zeros(max(V, 1), np.int64)
        check(self._L.dmf_volume_voxel_counts(self._h, ptr(a), ptr(b), a.size))
        return a[:V], b[:V]

    def voxel_points(self, hash_):
        n = C.c_int64(0)
        check(self._L.dmf_volume_voxel_points(self._h, int(hash_), None, None, 0, C.addressof(n)))
        if n.value < 0:
            return None, None
        p = np.zeros((max(n.value, 1), 3), np.float32)
        q = np.zeros((max(n.value, 1), 3), np.float32)
        check(self._L.dmf_volume_voxel_points(self._h, int(hash_), ptr(p), ptr(q), n.value, C.addressof(n)))
        return p[:n.value], q[:n.value]

    def export(self):
        """dmf_volume_export: every voxel's points in one call -> (offsets int32 (V + 1,), pts
        float32 (n, 3), normals4 float32 (n, 4)); the points of slot s (occupied_cells_ order) are
        rows offsets[s]:offsets[s + 1] in insertion order, normals4[:, 3] = 1 where the point
        carried a normal."""
        i = self.info()
        V, n = int(i["num_occupied"]), int(i["num_points"])
        off = np.zeros(V + 1, np.int32)
        pts = np.zeros((max(n, 1), 3), np.float32)
        nrm = np.zeros((max(n, 1), 4), np.float32)
        check(self._L.dmf_volume_export(self._h, ptr(off), ptr(pts), ptr(nrm), n))
        return off, pts[:n], nrm[:n]

    def occupancy_dense(self):
        nx, ny, nz = self.dims
        out = np.zeros(nx * ny * nz, np.uint8)
        check(self._L.dmf_volume_occupancy(self._h, ptr(out)))
        return out.reshape(nx, ny, nz)

    def getNeighborHashes(self, hash_, K=1):
        """Volume.hpp:235-255 (kept with the reference's `i==j==k==0` test)."""
        occ = self.occupancy_dense()
        x, y, z = self.getVoxelCoords(hash_)
        out = []
        for i in range(-K, K + 1):
            for j in range(-K, K + 1):
                for k in range(-K, K + 1):
                    if int(int(i == j) == k) == 0:
                        continue
                    a, b, c = x + i, y + j, z + k
                    if self.validCoords(a, b, c) and occ[a, b, c]:
                        out.append(self.getHashId(a, b, c))
        return out


def _pose(T):
    a = np.ascontiguousarray(T, np.float32).reshape(-1)
    if a.size == 16:
        a = np.ascontiguousarray(a.reshape(4, 4)[:3].reshape(12))
    if a.size != 12:
        raise ValueError("pose must be 3x4 (or 4x4) floats")
    return a


def _poses(T):
    """A stack of poses -> (P, 12) float32: each pose 3x4 or 4x4 (Eigen::Affine3f rows),
    a single pose, or already flattened rows of 12; anything else is rejected."""
    a = np.asarray(T, np.float32)
    if a.ndim == 2 and a.shape in ((3, 4), (4, 4)):
        a = a[None]
    if a.ndim == 3 and a.shape[1:] in ((3, 4), (4, 4)):
        return np.ascontiguousarray(a[:, :3, :].reshape(-1, 12))
    if a.ndim == 2 and a.shape[1] == 12:
        return np.ascontiguousarray(a)
    if a.ndim == 1 and a.size in (12, 16):
        return _pose(a)[None]
    raise ValueError(f"poses must be (P, 3, 4), (P, 4, 4) or (P, 12) floats, got shape {a.shape}")


class FuseParams:
    def __new__(cls, **kw):
        return _lib.default_fuse_params(**kw)


class RayTracingEngine:
    """RayTracingEngine.hpp:27-564 over the GPU.  Cheap to copy (holds only the camera)."""

    def __init__(self, cam):
        self.cam_ = cam

    def _c(self):
        return C.addressof(self.cam_._c)

    # reverseRayTraceFast  RayTracingEngine.hpp:136-226
    def reverseRayTraceFast(self, volume, transformation, viz, zdelta=1):
        found, lists = self.reverseRayTraceFastBatch(volume, _pose(transformation)[None], viz)
        return bool(found[0]), lists[0]

    def reverseRayTraceFastBatch(self, volume, poses, viz=False):
        return self._reverse(volume, poses, viz, volume._L.dmf_reverse_ray_trace_fast)

    # Set-cover consumer (Algorithms.hpp:38-86 greedySetCover over the
    # reverseRayTraceFast good sets, tests/SetCover.cpp:218-240): selected pose indices.
    def setCover(self, volume, poses, min_gain=5):
        poses = np.ascontiguousarray(np.asarray(poses, np.float32).reshape(-1, 12))
        P = poses.shape[0]
        sel = np.zeros(max(P, 1), np.int32)
        n = C.c_int32()
        check(volume._L.dmf_greedy_set_cover(volume._h, self._c(), ptr(poses), P, int(min_gain), ptr(sel),
                                             C.addressof(n)))
        return sel[:n.value]

    # reverseRayTrace  RayTracingEngine.hpp:45-134
    def reverseRayTrace(self, volume, transformation, viz, zdelta=1):
        found, lists = self._reverse(volume, _pose(transformation)[None], viz, volume._L.dmf_reverse_ray_trace)
        return bool(found[0]), lists[0]

    def _reverse(self, volume, poses, viz, fn):
        poses = np.ascontiguousarray(np.asarray(poses, np.float32).reshape(-1, 12))
        P = poses.shape[0]
        found = np.zeros(P, np.uint8)
        counts = np.zeros(P, np.int64)
        cap = max(int(volume.info()["num_occupied"]) * 2, 1024)
        while True:
            out = np.zeros(cap, np.uint64)
            st = fn(volume._h, self._c(), ptr(poses), P, int(bool(viz)), ptr(found), ptr(counts), ptr(out), cap)
            if st == _lib.DMF_ERR_CAPACITY:
                cap = int(counts.sum())
                continue
            check(st)
            break
        offs = np.concatenate([[0], np.cumsum(counts)])
        return found.astype(bool), [out[offs[i]:offs[i + 1]] for i in range(P)]

    # rayTrace  RayTracingEngine.hpp:268-309
    def rayTrace(self, volume, transformation, zdelta=10, sparse=True):
        check(volume._L.dmf_ray_trace(volume._h, self._c(), ptr(_pose(transformation)), int(zdelta), int(bool(sparse))))

    # rayTraceAndClassify  RayTracingEngine.hpp:311-375
    def rayTraceAndClassify(self, volume, transformation, zdelta=10, view=1, sparse=True):
        check(volume._L.dmf_ray_trace_and_classify(volume._h, self._c(), ptr(_pose(transformation)), int(zdelta),
                                                   int(view), int(bool(sparse))))

    # rayTraceAndGetMinimum  RayTracingEngine.hpp:229-264
    def rayTraceAndGetMinimum(self, volume, transformation, zdelta=1, sparse=True):
        m = C.c_int32(0)
        check(volume._L.dmf_ray_trace_and_get_minimum(volume._h, self._c(), ptr(_pose(transformation)), int(zdelta),
                                                      int(bool(sparse)), C.addressof(m)))
        return m.value

    def _fwd_list(self, fn, volume, transformation, zdelta, sparse):
        T = _pose(transformation)
        found = np.zeros(1, np.uint8)
        n = C.c_int64(0)
        cap = 1 << 16
        while True:
            out = np.zeros(cap, np.uint64)
            st = fn(volume._h, self._c(), ptr(T), int(zdelta), int(bool(sparse)), ptr(found), ptr(out), cap,
                    C.addressof(n))
            if st == _lib.DMF_ERR_CAPACITY:
                cap = n.value
                continue
            check(st)
            return bool(found[0]), out[:n.value]

    # rayTraceAndGetGoodPoints  RayTracingEngine.hpp:377-445
    def rayTraceAndGetGoodPoints(self, volume, transformation, zdelta=10, sparse=True):
        return self._fwd_list(volume._L.dmf_ray_trace_and_get_good_points, volume, transformation, zdelta, sparse)

    # rayTraceAndGetPoints  RayTracingEngine.hpp:447-494
    def rayTraceAndGetPoints(self, volume, transformation, zdelta=10, sparse=True):
        return self._fwd_list(volume._L.dmf_ray_trace_and_get_points, volume, transformation, zdelta, sparse)

    def forward_first_hits(self, volume, transformation, zstart, zdelta, rdelta, cdelta):
        H, W = self.cam_.height_, self.cam_.width_
        R, Cc = (H + rdelta - 1) // rdelta, (W + cdelta - 1) // cdelta
        k = np.zeros(R * Cc, np.int32)
        h = np.zeros(R * Cc, np.uint64)
        check(volume._L.dmf_forward_first_hits(volume._h, self._c(), ptr(_pose(transformation)), zstart, zdelta,
                                               rdelta, cdelta, ptr(k), ptr(h)))
        return k.reshape(R, Cc), h.reshape(R, Cc)

    # rayTraceVolume  RayTracingEngine.hpp:498-564
    def rayTraceVolume(self, volume, transformation):
        d = np.zeros(self.cam_.height_ * self.cam_.width_, np.int32)
        check(volume._L.dmf_ray_trace_volume(volume._h, self._c(), ptr(_pose(transformation)), ptr(d)))
        return d.reshape(self.cam_.height_, self.cam_.width_)

    # back-projection of whole frames (Camera.hpp:24-45), on the GPU
    def backproject(self, volume, depth, transformation):
        depth = np.ascontiguousarray(depth, np.uint16)
        out = np.zeros(depth.shape + (3,), np.float32)
        check(volume._L.dmf_backproject(volume._h, self._c(), ptr(depth), ptr(_pose(transformation)), ptr(out)))
        return out

    # 3D-DDA log-odds fusion
    def fuse_depth(self, volume, depth, poses, params=None, hits=None, misses=None):
        depth = np.ascontiguousarray(depth, np.uint16)
        if depth.ndim == 2:
            depth = depth[None]
        poses = _poses(poses)
        H, W = self.cam_.height_, self.cam_.width_
        if depth.shape != (poses.shape[0], H, W):
            raise ValueError(f"depth must be (P, H, W) = ({poses.shape[0]}, {H}, {W}) uint16, got {depth.shape}")
        n = int(np.prod(volume.dims))
        for name, a in (("hits", hits), ("misses", misses)):
            if a is not None and not (isinstance(a, np.ndarray) and a.dtype == np.int32 and a.size == n
                                      and a.flags.c_contiguous):
                raise ValueError(f"{name} must be a contiguous int32 array of {n} cells (accumulated in place)")
        hits = np.zeros(n, np.int32) if hits is None else hits
        misses = np.zeros(n, np.int32) if misses is None else misses
        stats = np.zeros(3, np.int64)
        params = params or _lib.default_fuse_params()
        check(volume._L.dmf_fuse_depth(volume._h, self._c(), ptr(depth), ptr(poses), poses.shape[0],
                                       C.addressof(params), ptr(hits), ptr(misses), ptr(stats)))
        return hits, misses, stats

    # the same fusion of point clouds with sensor origins
    def fuse_points(self, volume, xyz, origins, params=None, hits=None, misses=None):
        """insertPointCloud(scan, origin): xyz (S, N, 3) or (N, 3) float32 world-frame endpoints,
        origins (S, 3) or (3,) world-frame sensor positions -> what fuse_depth returns.  Point i of
        scan s is the ray origins[s] -> xyz[s, i], traced exactly as fuse_depth traces a pixel's.  A
        point with a non-finite coordinate is no ray (pad unequal scans with NaN); there is no range
        gate (params.dmin_mm / dmax_mm are not applied: filter by range, or mark rejected points NaN)."""
        xyz = np.ascontiguousarray(xyz, np.float32)
        origins = np.ascontiguousarray(origins, np.float32)
        if xyz.ndim == 2:
            xyz = xyz[None]
        if origins.ndim == 1:
            origins = origins[None]
        if xyz.ndim != 3 or xyz.shape[2] != 3 or origins.shape != (xyz.shape[0], 3):
            raise ValueError(f"xyz must be (S, N, 3) or (N, 3) and origins (S, 3) or (3,), got {xyz.shape} and "
                             f"{origins.shape}")
        n = int(np.prod(volume.dims))
        for name, a in (("hits", hits), ("misses", misses)):
            if a is not None and not (isinstance(a, np.ndarray) and a.dtype == np.int32 and a.size == n
                                      and a.flags.c_contiguous):
                raise ValueError(f"{name} must be a contiguous int32 array of {n} cells (accumulated in place)")
        hits = np.zeros(n, np.int32) if hits is None else hits
        misses = np.zeros(n, np.int32) if misses is None else misses
        stats = np.zeros(3, np.int64)
        params = params or _lib.default_fuse_params()
        check(volume._L.dmf_fuse_points(volume._h, ptr(xyz), ptr(origins), xyz.shape[0], xyz.shape[1],
                                        C.addressof(params), ptr(hits), ptr(misses), ptr(stats)))
        return hits, misses, stats

    def fuse_finalize(self, volume, hits, misses, params=None):
        params = params or _lib.default_fuse_params()
        out = np.zeros(hits.size, np.int16)
        check(volume._L.dmf_fuse_finalize(volume._h, ptr(np.ascontiguousarray(hits, np.int32)),
                                          ptr(np.ascontiguousarray(misses, np.int32)), C.addressof(params), ptr(out)))
        return out

    # ray-cast of a fused log-odds grid: predicted depth and first solid cell
    def raycast_logodds(self, volume, logodds, poses, threshold=0, range_mm=1000):
        """What a camera at each pose sees in the int16 log-odds grid `logodds` (xdim*ydim*zdim
        cells, x-major, as fuse_finalize returns it): -> (depth (P, H, W) int32, cell (P, H, W)
        uint64).  cell is the getHashId of the first cell with log-odds >= threshold along the
        pixel's probe ray (the fusion's ray for depth range_mm), NO_CELL when there is none; depth
        is rayTraceVolume's value of that voxel, -1 without one."""
        poses = _poses(poses)
        n = int(np.prod(volume.dims))
        lo = np.asarray(logodds)
        if lo.dtype != np.int16 or lo.size != n:
            raise ValueError(f"logodds must be int16 with {n} cells (x-major over dims {tuple(volume.dims)}), "
                             f"got {lo.dtype} with {lo.size}")
        lo = np.ascontiguousarray(lo).reshape(-1)
        P, H, W = poses.shape[0], self.cam_.height_, self.cam_.width_
        depth = np.zeros((P, H, W), np.int32)
        cell = np.zeros((P, H, W), np.uint64)
        check(volume._L.dmf_raycast_logodds(volume._h, self._c(), ptr(lo), ptr(poses), P, int(threshold),
                                            int(range_mm), ptr(depth), ptr(cell)))
        return depth, cell

    # view gain over a fused log-odds grid and next-best-view selection
    @staticmethod
    def _grid_and_poses(volume, logodds, poses):
        poses = _poses(poses)
        n = int(np.prod(volume.dims))
        lo = np.asarray(logodds)
        if lo.dtype != np.int16 or lo.size != n:
            raise ValueError(f"logodds must be int16 with {n} cells (x-major over dims {tuple(volume.dims)}), "
                             f"got {lo.dtype} with {lo.size}")
        return np.ascontiguousarray(lo).reshape(-1), poses

    def view_gain(self, volume, logodds, poses, occ_threshold=1, free_threshold=-1, range_mm=1000, masks=False):
        """How many unobserved cells each candidate pose would see in the int16 log-odds grid
        `logodds` (as fuse_finalize returns it): -> gain (P,) uint64, and with masks=True also
        seen (P, words) uint64 (VoxelVolume.view_mask_dense unpacks one row).  A cell is solid iff
        L >= occ_threshold, free iff not solid and L <= free_threshold, unknown otherwise; a
        pixel sees the cells of its probe ray (depth range_mm) before the first solid one."""
        lo, poses = self._grid_and_poses(volume, logodds, poses)
        P = poses.shape[0]
        gain = np.zeros(P, np.uint64)
        seen = np.zeros((P, volume.view_gain_words()), np.uint64) if masks else None
        check(volume._L.dmf_view_gain(volume._h, self._c(), ptr(lo), ptr(poses), P, int(occ_threshold),
                                      int(free_threshold), int(range_mm), ptr(seen) if masks else None, ptr(gain)))
        return (gain, seen) if masks else gain

    def next_best_views(self, volume, logodds, poses, occ_threshold=1, free_threshold=-1, range_mm=1000, min_gain=5):
        """greedySetCover over the poses' sets of unobserved visible cells (view_gain's masks):
        -> (selected pose indices in selection order (int32), gain (P,) uint64: each pose's own
        gain).  The selection stops when the best pose adds nothing or fewer than min_gain cells."""
        lo, poses = self._grid_and_poses(volume, logodds, poses)
        P = poses.shape[0]
        sel, nsel, gain = np.zeros(max(P, 1), np.int32), C.c_int32(0), np.zeros(P, np.uint64)
        check(volume._L.dmf_next_best_views(volume._h, self._c(), ptr(lo), ptr(poses), P, int(occ_threshold),
                                            int(free_threshold), int(range_mm), int(min_gain), ptr(sel),
                                            C.addressof(nsel), ptr(gain)))
        return sel[:nsel.value].copy(), gain


def will_collide(volume, a, b):
    """tests/CameraPathGen.cpp:128-156 willCollide, batched over segment pairs."""
    a = np.ascontiguousarray(a, np.float32).reshape(-1, 3)
    b = np.ascontiguousarray(b, np.float32).reshape(-1, 3)
    out = np.zeros(a.shape[0], np.uint8)
    check(volume._L.dmf_will_collide(volume._h, ptr(a), ptr(b), a.shape[0], ptr(out)))
    return out.astype(bool)


def collision_cost_map(volume, poses):
    """Planner::run_tsp cost map (tests/CameraPathGen.cpp:310-331): (V, V) int32 over the
    camera centres of `poses` (V x 3x4), INT_MAX where willCollide, else int(dist * 1000)."""
    poses = np.ascontiguousarray(poses, np.float32).reshape(-1, 12)
    V = poses.shape[0]
    out = np.zeros((V, V), np.int32)
    check(volume._L.dmf_collision_cost_map(volume._h, ptr(poses), V, ptr(out)))
    return out


def position_cameras(volume, xyz, normals, distance_mm=300, flip=True):
    """Algorithms::positionCameras over the locations `xyz` (float32 (m, 3)) with `normals` (float32
    (m, 3)) -> (poses float32 (m, 3, 4), normals float32 (m, 3)); on the GPU.  With
    flip=True a normal with z <= 0 is negated first (the returned normals; the argument is not
    changed), as the reference does in its cloud; then each camera stands distance_mm out along the
    normal and looks back along it: columns x = (0, -1, 0), y = (1, 0, 0), z = -normal.  flip=False
    is the plain positionCamera loop.  `volume` supplies the device and stream."""
    p = VoxelVolume._cloud(xyz, "xyz")
    nn = np.array(VoxelVolume._cloud(normals, "normals"), np.float32)
    if nn.shape != p.shape:
        raise ValueError(f"normals must have xyz's shape {p.shape}, got {nn.shape}")
    if not 0 <= int(distance_mm) <= 0xFFFFFFFF:
        raise ValueError(f"distance_mm must fit uint32, got {distance_mm}")
    m = p.shape[0]
    poses = np.zeros((m, 3, 4), np.float32)
    if m:
        check(volume._L.dmf_position_cameras(volume._h, ptr(p), ptr(nn), m, int(distance_mm), 0 if flip else 1,
                                             ptr(poses)))
    return poses, nn


def _tour_map(cost_map):
    m = np.asarray(cost_map)
    if m.dtype != np.int32 or m.ndim != 2 or m.shape[0] != m.shape[1]:
        raise ValueError(f"cost_map must be int32 of shape (V, V), got {m.dtype} {m.shape}")
    return np.ascontiguousarray(m)


def _tour_result(path, cnt, info):
    # (the edge sum is an int64 in its uint64 word: entries may be negative)
    return (path, tuple(int(c) for c in cnt[:3]) + (int(cnt.view(np.int64)[3]), int(cnt[4]))) if info else path


def tour_nearest_neighbour(volume, cost_map, info=False):
    """TSP::NearestNeighborSearch (TSPSolver.hpp:76-98) over `cost_map` (int32 (V, V), [a][b] = the
    cost from a to b, INT_MAX = no edge) -> the int32 path (V,), from node 0; on the GPU
    (DESIGN.md §4.8).  Where every unvisited entry of a row is INT_MAX the lowest unvisited index
    is taken (the reference aborts).  info=True also returns (forced picks, 0, 0, the sum of the
    path's edges below INT_MAX, its INT_MAX edges).  `volume` supplies the device and stream."""
    m = _tour_map(cost_map)
    V = m.shape[0]
    path, cnt = np.zeros(V, np.int32), np.zeros(5, np.uint64)
    check(volume._L.dmf_tour_nearest_neighbour(volume._h, ptr(m) if V else None, V, ptr(path) if V else None, ptr(cnt)))
    return _tour_result(path, cnt, info)


def tour_two_opt(volume, cost_map, path, max_rounds=0, info=False):
    """TSP::TwoOptSearch (TSPSolver.hpp:136-156) from `path` (a permutation of 0..V-1; position 0
    stays) -> the improved int32 path: the first candidate (i, k) in lexicographic order whose
    reversal of positions i..k makes the path strictly shorter is applied and the scan restarts,
    until none is left or `max_rounds` > 0 reversals are applied.  info=True also returns (0,
    reversals, converged 0/1, the sum of the edges below INT_MAX, the INT_MAX edges)."""
    m = _tour_map(cost_map)
    V = m.shape[0]
    p = np.asarray(path)
    if p.dtype.kind not in "iu" or p.shape != (V,):
        raise ValueError(f"path must be integer indices of shape ({V},), got {p.dtype} {p.shape}")
    if V and (int(p.min()) < -2 ** 31 or int(p.max()) >= 2 ** 31):
        raise ValueError("path holds an index that int32 does not hold")   # (it would wrap in the cast below)
    if int(max_rounds) < 0:
        raise ValueError(f"max_rounds must be >= 0, got {max_rounds}")
    out, cnt = np.array(p, np.int32), np.zeros(5, np.uint64)
    check(volume._L.dmf_tour_two_opt(volume._h, ptr(m) if V else None, V, ptr(out) if V else None, int(max_rounds),
                                     ptr(cnt)))
    return _tour_result(out, cnt, info)


def tour(volume, cost_map, max_rounds=0, info=False):
    """tour_nearest_neighbour, then tour_two_opt from its path: what every planner of the reference
    runs over its cost map (run_tsp).  info=True also returns (forced picks, reversals, converged
    0/1, the sum of the edges below INT_MAX, the INT_MAX edges)."""
    m = _tour_map(cost_map)
    V = m.shape[0]
    if int(max_rounds) < 0:
        raise ValueError(f"max_rounds must be >= 0, got {max_rounds}")
    path, cnt = np.zeros(V, np.int32), np.zeros(5, np.uint64)
    check(volume._L.dmf_tour(volume._h, ptr(m) if V else None, V, ptr(path) if V else None, int(max_rounds), ptr(cnt)))
    return _tour_result(path, cnt, info)


class OccupancyGrid:
    """OccupancyGrid.hpp:50-318 on the GPU (dmf_ogrid_*): same setup sequence
    (setDimensions, setResolution, setK, construct), updateStates(cloud, normals) and the
    download calls.  updateStates gives the deterministic single-threaded result."""

    def __init__(self, device=0):
        self._L = load()
        h = C.c_void_p()
        check(self._L.dmf_ogrid_create(C.addressof(h), int(device)))
        self._h = h
        self._b = None
        self._r = None
        self.k_ = 0

    def close(self):
        if getattr(self, "_h", None):
            self._L.dmf_ogrid_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def setDimensions(self, xmin, xmax, ymin, ymax, zmin, zmax):
        self._b = np.array([xmin, xmax, ymin, ymax, zmin, zmax], np.float64)

    def setResolution(self, x, y, z):
        self._r = (float(np.float32(x)), float(np.float32(y)), float(np.float32(z)))

    def setK(self, k):
        self.k_ = int(k)

    def construct(self):
        check(self._L.dmf_ogrid_setup(self._h, ptr(self._b), *self._r, self.k_))
        return True

    @property
    def dims(self):
        d = np.zeros(3, np.int32)
        check(self._L.dmf_ogrid_get_dims(self._h, ptr(d)))
        return tuple(int(x) for x in d)

    def updateStates(self, cloud, normals):
        """cloud (n,3) xyz; normals (m,6) x y z nx ny nz (PointNormal)."""
        cloud = np.ascontiguousarray(cloud, np.float32).reshape(-1, 3)
        normals = np.ascontiguousarray(normals, np.float32).reshape(-1, 6)
        check(self._L.dmf_ogrid_update_states(self._h, ptr(cloud), cloud.shape[0], ptr(normals), normals.shape[0]))
        return True

    def state(self):
        n = int(np.prod(self.dims))
        nrm, cen = np.zeros(3 * n, np.float32), np.zeros(3 * n, np.float32)
        cnt, fl = np.zeros(n, np.int32), np.zeros(n, np.uint8)
        check(self._L.dmf_ogrid_state(self._h, ptr(nrm), ptr(cen), ptr(cnt), ptr(fl)))
        return nrm.reshape(-1, 3), cen.reshape(-1, 3), cnt, fl

    def _download(self, mode):
        n = C.c_int64()
        st = self._L.dmf_ogrid_download(self._h, mode, None, 0, C.addressof(n))
        if st not in (0, _lib.DMF_ERR_CAPACITY):
            check(st)
        out = np.zeros(6 * max(n.value, 1), np.float32)
        check(self._L.dmf_ogrid_download(self._h, mode, ptr(out), n.value, C.addressof(n)))
        return out[:6 * n.value].reshape(-1, 6)

    def downloadCloud(self):
        """(n, 6) centroid xyz + normal of occupied voxels, x-major (:166-193)."""
        return self._download(0)

    def downloadHQCloud(self):
        """as downloadCloud for voxels with count > 100 (:283-318)."""
        return self._download(1)

    def downloadReorganizedCloud(self, clean=False):
        """(n, 6) of the reorganized grid (:200-286): every occupied voxel (with clean,
        count >= 100) merges into the voxel holding its centroid, in the single-threaded
        x-major order; occupied reorganized voxels, x-major."""
        return self._download(3 if clean else 2)

    @property
    def reorg_rounds(self):
        """dmf_ogrid_reorg_rounds (include/dmf_diag.h): rounds of the latest
        downloadReorganizedCloud's fixed point, -1 = the serial fallback, 0 = none yet."""
        r = C.c_int32()
        check(self._L.dmf_ogrid_reorg_rounds(self._h, C.addressof(r)))
        return r.value

    def set_reorg_round_cap(self, cap):
        """dmf_ogrid_set_reorg_round_cap: 0 = the default (64), else 1..65536; never changes a result."""
        check(self._L.dmf_ogrid_set_reorg_round_cap(self._h, int(cap)))

    def set_state(self, normal, centroid, count, flags):
        """Write the dense voxels_ fields (normal, centroid (n, 3) float; count int32;
        flags occupied | normal_found << 1) — the reference's public state."""
        n = int(np.prod(self.dims))
        nrm = np.ascontiguousarray(normal, np.float32).reshape(3 * n)
        cen = np.ascontiguousarray(centroid, np.float32).reshape(3 * n)
        cnt = np.ascontiguousarray(count, np.int32).reshape(n)
        fl = np.ascontiguousarray(flags, np.uint8).reshape(n)
        check(self._L.dmf_ogrid_set_state(self._h, ptr(nrm), ptr(cen), ptr(cnt), ptr(fl)))
