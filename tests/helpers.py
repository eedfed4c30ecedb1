"""Shared synthetic scenes for the parity tests (SURVEY.md §8d inputs, small sizes)."""
import functools

import numpy as np

from dmf_amd import scene

K = scene.K_640x480
H, W = 480, 640
BOUNDS = (-0.5, 0.5, -0.5, 0.5, -0.5, 0.5)


@functools.lru_cache(maxsize=None)
def frames(P=6, seed=1234, width=W, height=H):
    Kx = scene.intrinsics(width, height)
    poses = scene.fibonacci_poses(P, seed=seed)
    depth, nrm = scene.render_frames(Kx, width, height, poses, normals=True)
    return poses, depth, nrm


@functools.lru_cache(maxsize=None)
def cloud(n_frames=3, P=6):
    """Back-projected depth frames (oracle back-projection) + analytic normals."""
    from oracle import oracle as O
    poses, depth, nrm = frames(P)
    pts, nn = [], []
    for i in range(n_frames):
        xyz = O.backproject(K, depth[i], poses[i])
        m = depth[i] > 0
        pts.append(xyz[m])
        nn.append(nrm[i][m])
    return np.concatenate(pts).astype(np.float32), np.concatenate(nn).astype(np.float32)


@functools.lru_cache(maxsize=None)
def ref_style_poses(n=6, seed=7):
    pts, nn = cloud()
    rng = np.random.default_rng(seed)
    idx = rng.choice(pts.shape[0], n, replace=False)
    return scene.reference_style_poses(pts[idx], nn[idx], 300)


def all_poses():
    return np.concatenate([frames()[0], ref_style_poses()])


def oracle_volume(O, n=128, bounds=BOUNDS, with_normals=True, clouds=None):
    v = O.Volume()
    v.setDimensions(*bounds)
    v.setVolumeSize(n, n, n)
    v.constructVolume()
    for pts, nn in (clouds if clouds is not None else [cloud()]):
        v.integratePointCloud(pts, nn if with_normals else None)
    return v


def gpu_volume(n=128, bounds=BOUNDS, with_normals=True, clouds=None):
    import dmf_amd
    v = dmf_amd.VoxelVolume()
    v.setDimensions(*bounds)
    v.setVolumeSize(n, n, n)
    v.constructVolume()
    for pts, nn in (clouds if clouds is not None else [cloud()]):
        v.integratePointCloud(pts, nn if with_normals else None)
    return v


# ----------------------------------------------------------------------------- shapes / lifecycle scenes
# Volume offsets of the off-origin tests: the first is float-exact, the second is not (so the
# bounds, and with them the voxel deltas, are no powers of two).
OFFSETS = ((100.25, -7.5, 3.0), (1000.0, -2000.5, 333.3))
# Cameras with fx != fy and a fractional principal point; (K, width, height).
KA = np.array([60, 0, 30.3, 0, 47.5, 18.7, 0, 0, 1], np.float32)
KA_WH = (61, 37)
KB = np.array([190.25, 0, 99.6, 0, 201.5, 77.2, 0, 0, 1], np.float32)
KB_WH = (203, 149)
ODD_BOUNDS = (-0.45, 0.52, -0.4, 0.47, -0.33, 0.41)  # test_reverse_sparse_partial_bricks
ODD_DIMS = (91, 77, 61)


def shifted_bounds(o, half=0.5):
    return tuple(float(s * half + o[a]) for a in range(3) for s in (-1, 1))


def shift_points(pts, o):
    """Points moved by o in float64, rounded to float32."""
    return (np.asarray(pts, np.float64) + np.asarray(o, np.float64)).astype(np.float32)


def shift_poses(poses, o):
    """(P, 12) poses whose translation is moved by o in float64, rounded to float32."""
    p = np.asarray(poses, np.float64).reshape(-1, 12).copy()
    p[:, 3::4] += np.asarray(o, np.float64)
    return np.ascontiguousarray(p.astype(np.float32))


@functools.lru_cache(maxsize=None)
def five_poses():
    """3 Fibonacci-sphere poses (seed 11) + 2 reference-style (non-orthonormal) poses."""
    return np.concatenate([scene.fibonacci_poses(3, seed=11), ref_style_poses()[:2]]).astype(np.float32)


def _fill(v, dims, bounds, clouds):
    if isinstance(dims, int):
        dims = (dims, dims, dims)
    v.setDimensions(*bounds)
    v.setVolumeSize(*dims)
    v.constructVolume()
    for pts, nn in clouds:
        v.integratePointCloud(pts, nn)
    return v


def oracle_grid(O, dims, bounds=BOUNDS, clouds=()):
    """An oracle volume of dims (an int: a cube) cells over bounds with the (points, normals or
    None) clouds integrated."""
    return _fill(O.Volume(), dims, bounds, clouds)


def gpu_grid(dims, bounds=BOUNDS, clouds=()):
    import dmf_amd
    return _fill(dmf_amd.VoxelVolume(), dims, bounds, clouds)


def volume_pair(O, dims, bounds=BOUNDS, clouds=()):
    """(oracle volume, GPU volume) of the same geometry with the same clouds integrated."""
    return oracle_grid(O, dims, bounds, clouds), gpu_grid(dims, bounds, clouds)


def cell_cloud(V, n=40, bounds=BOUNDS, seed=3):
    """One point at the centre of each of V distinct cells of an n^3 grid (cells drawn with
    default_rng(seed).integers(8, 32, 3), repeats skipped), each with the outward normal (from
    the volume's centre)."""
    rng = np.random.default_rng(seed)
    cells, seen = [], set()
    while len(cells) < V:
        c = tuple(int(x) for x in rng.integers(8, 32, 3))
        if c not in seen:
            seen.add(c)
            cells.append(c)
    cells = np.asarray(cells, np.float64).reshape(-1, 3)
    lo, hi = np.array(bounds[0::2]), np.array(bounds[1::2])
    pts = lo + (cells + 0.5) * ((hi - lo) / n)
    nn = pts - (lo + hi) / 2
    nn /= np.maximum(np.linalg.norm(nn, axis=1, keepdims=True), 1e-12)
    return pts.astype(np.float32), nn.astype(np.float32)


def flags_equal(ov, gv):
    """view / good flags of every occupied voxel: oracle == GPU."""
    oview, ogood, _, _ = ov.voxel_table()
    gview, ggood = gv.voxel_flags()
    return np.array_equal(oview, gview) and np.array_equal(ogood, ggood)


def mask_bits(words, V):
    """A row of uint64 mask words -> (bool[V] of the slots' bits, True if a bit past V - 1 is set)."""
    bits = np.unpackbits(np.ascontiguousarray(words, np.uint64).view(np.uint8), bitorder="little")
    return bits[:V].astype(bool), bool(bits[V:].any())


class DeviceCalls:
    """The *_device entry points of one GPU volume over buffers of dmf_device_malloc (freed by
    close()); every call synchronises and returns host arrays."""

    def __init__(self, gv):
        from dmf_amd import _lib
        self._lib, self.gv, self.L, self.h = _lib, gv, gv._L, gv._h
        self._bufs = []

    def alloc(self, nbytes):
        import ctypes as C
        p = C.c_void_p()
        self._lib.check(self.L.dmf_device_malloc(self.h, C.addressof(p), max(int(nbytes), 8)))
        self._bufs.append(p.value)
        return p.value

    def upload(self, a):
        a = np.ascontiguousarray(a)
        d = self.alloc(a.nbytes)
        if a.nbytes:
            self._lib.check(self.L.dmf_memcpy_h2d(self.h, d, a.ctypes.data, a.nbytes))
        return d

    def zeros(self, nbytes):
        return self.upload(np.zeros(max(int(nbytes), 8), np.uint8))

    def download(self, d, shape, dtype):
        out = np.zeros(shape, dtype)
        if out.nbytes:
            self._lib.check(self.L.dmf_memcpy_d2h(self.h, out.ctypes.data, d, out.nbytes))
        return out

    def close(self):
        for p in self._bufs:
            self.L.dmf_device_free(self.h, p)
        self._bufs = []

    def reverse(self, K, height, width, poses, viz=False):
        """dmf_reverse_visibility_device -> (visible (P, words) uint64, good, stats[2])."""
        import ctypes as C
        poses = np.ascontiguousarray(poses, np.float32).reshape(-1, 12)
        P, V = poses.shape[0], int(self.gv.info()["num_occupied"])
        words = (V + 63) // 64
        cam = self._lib.make_camera(K, height, width)
        dp, dv, dg, ds = self.upload(poses), self.zeros(8 * P * words), self.zeros(8 * P * words), self.zeros(16)
        self._lib.check(self.L.dmf_reverse_visibility_device(self.h, C.addressof(cam), dp, P, int(bool(viz)), dv, dg, ds))
        return (self.download(dv, (P, words), np.uint64), self.download(dg, (P, words), np.uint64),
                self.download(ds, 2, np.uint64))

    def forward(self, K, height, width, poses, zstart, zdelta, rdelta, cdelta):
        """dmf_forward_first_hits_device -> (k (P, R, C) int32, slot (P, R, C) int32, march samples)."""
        import ctypes as C
        poses = np.ascontiguousarray(poses, np.float32).reshape(-1, 12)
        P = poses.shape[0]
        R, Cc = (height + rdelta - 1) // rdelta, (width + cdelta - 1) // cdelta
        cam = self._lib.make_camera(K, height, width)
        # -2 never is an output: a pixel the kernel left unwritten shows
        dp, ds = self.upload(poses), self.zeros(8)
        dk, dl = self.upload(np.full(P * R * Cc, -2, np.int32)), self.upload(np.full(P * R * Cc, -2, np.int32))
        self._lib.check(self.L.dmf_forward_first_hits_device(self.h, C.addressof(cam), dp, P, zstart, zdelta, rdelta,
                                                             cdelta, dk, dl, ds))
        return (self.download(dk, (P, R, Cc), np.int32), self.download(dl, (P, R, Cc), np.int32),
                int(self.download(ds, 1, np.uint64)[0]))

    def cover_masks(self, masks, min_gain):
        """dmf_greedy_set_cover_masks_device over host masks (P, words) uint64 -> selected."""
        import ctypes as C
        masks = np.ascontiguousarray(masks, np.uint64)
        P, words = masks.shape
        sel = np.zeros(max(P, 1), np.int32)
        n = C.c_int32()
        self._lib.check(self.L.dmf_greedy_set_cover_masks_device(self.h, self.upload(masks), P, words, int(min_gain),
                                                                 sel.ctypes.data, C.addressof(n)))
        return sel[:n.value]

    def cover_masks_guarded(self, d_masks, P, words, min_gain, fill=-7, guard=5):
        """dmf_greedy_set_cover_masks_device over device masks with selected (P + guard entries) and
        nselected pre-filled with `fill`, which never is an output -> (status, nselected, the whole
        of selected): an entry the call left unwritten, or wrote past the end, shows."""
        import ctypes as C
        sel = np.full(max(int(P), 0) + guard, fill, np.int32)
        n = C.c_int32(fill)
        st = self.L.dmf_greedy_set_cover_masks_device(self.h, d_masks, int(P), int(words), int(min_gain),
                                                      sel.ctypes.data, C.addressof(n))
        return st, n.value, sel
