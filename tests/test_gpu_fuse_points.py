"""GPU: point-cloud fusion (dmf_fuse_points*): a second ray source for the exact
log-odds fusion.  Exact equality everywhere.

* The points dmf_backproject gives for a frame (pixels outside the depth gate NaN), fused from the
  pose's translation, make the counters and statistics of fuse_depth on that frame: every variant
  on an odd grid, and the production route at 256^3.
* The order of the points changes nothing.
* Arbitrary segments, packet edges: against the pure-Python restatement (fuse_points_ref).
* The brick pipeline's own branches (several pass-A workgroups per scan, the hashed histogram's
  overflow, device-cut batches, super-batches), pipelined calls mixed with depth calls, and the
  device form against the host form.
* The C++ drop-in's fusePoints overloads, from the headless driver.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import fuse_points_ref as FR
import helpers as Hh

pytestmark = pytest.mark.gpu

LDS_BOX, CELL_WALK, SLAB = 31, 40, 57
WA, HA = Hh.KA_WH
N1 = WA * HA                 # 2257 points per scan: 36 packets, the last one of 17 points
DMIN, DMAX = 40, 800         # the depth gate of the frames (rejects the far pixels)


# ---------------------------------------------------------------- the scans of depth frames
@functools.lru_cache(maxsize=None)
def _frames1():
    """5 poses and their rendered frames (every depth kept by the renderer: the fusion's gate does
    the rejecting).  Poses 0-2 look at the scene from outside the grid, pose 3 from below the
    ground plane (rays that all end before the grid: counted, no update), pose 4 has its eye
    inside the odd grid."""
    from dmf_amd import scene
    poses = np.ascontiguousarray(np.concatenate([scene.fibonacci_poses(4, seed=5),
                                                 scene.fibonacci_poses(1, radius=0.3, seed=3)]), np.float32)
    eye = poses[4, 3::4]
    lo, hi = np.array(Hh.ODD_BOUNDS[0::2]), np.array(Hh.ODD_BOUNDS[1::2])
    assert ((eye > lo) & (eye < hi)).all()
    depth = np.ascontiguousarray(scene.render_frames(Hh.KA, WA, HA, poses, dmin=1, dmax=65535), np.uint16)
    gated = (depth >= DMIN) & (depth < DMAX)
    assert gated.reshape(5, -1).any(1).all() and ((depth > 0) & ~gated).any()
    return poses, depth


def _grid(dims, bounds, variant=0, knobs=None):
    from dmf_amd import _lib
    gv = Hh.gpu_grid(dims, bounds)
    _lib.set_variant(gv, variant)
    for k, v in (knobs or {}).items():
        _lib.set_knob(gv, k, v)
    return gv


def _engine():
    import dmf_amd
    return dmf_amd.RayTracingEngine(dmf_amd.Camera(Hh.KA, HA, WA))


def _params():
    import dmf_amd
    return dmf_amd.FuseParams(dmin_mm=DMIN, dmax_mm=DMAX)


@functools.lru_cache(maxsize=None)
def _scans1():
    """The frames as scans: dmf_backproject's points with the gated-out pixels NaN, and the
    poses' translation columns."""
    poses, depth = _frames1()
    gv = Hh.gpu_grid(Hh.ODD_DIMS, Hh.ODD_BOUNDS)
    eng = _engine()
    xyz = np.stack([eng.backproject(gv, depth[i], poses[i]) for i in range(poses.shape[0])])
    gv.close()
    pts, origins = FR.frame_points(xyz, depth, poses, DMIN, DMAX)
    assert pts.shape == (5, N1, 3) and N1 % 64 == 17
    return pts, origins


@functools.lru_cache(maxsize=None)
def _depth_result(dims, bounds, variant):
    """fuse_depth of the frames with `variant` (read-only: shared by the tests)."""
    poses, depth = _frames1()
    gv = _grid(dims, bounds, variant)
    h, m, s = _engine().fuse_depth(gv, depth, poses, _params())
    gv.close()
    assert s[0] > 10 ** 5 and s[2] > 0
    for a in (h, m, s):
        a.setflags(write=False)
    return h, m, s


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2][:3], b[2][:3])


# ---------------------------------------------------------------- 1. same rays, same counters
@pytest.mark.parametrize("variant", [LDS_BOX, CELL_WALK, SLAB])
def test_points_of_frames_equal_fuse_depth(variant):
    """Odd grid (truncating dims, partial bricks), camera KA (tail packet of 17 points), 5 poses
    (one eye inside the grid), a gate that rejects pixels: hits, misses and stats[0..2]."""
    from dmf_amd import _lib
    pts, origins = _scans1()
    gv = _grid(Hh.ODD_DIMS, Hh.ODD_BOUNDS, variant)
    got = _engine().fuse_points(gv, pts, origins, _params())
    name = _lib.kernel_name(gv)
    assert _lib.fuse_status(gv) == 0
    gv.close()
    assert name.startswith({SLAB: "dmf::k_bk_fuse_s<", CELL_WALK: "dmf::k_bk_fuse<", LDS_BOX: "dmf::k_fuse_l<"}[variant])
    assert _same(got, _depth_result(Hh.ODD_DIMS, Hh.ODD_BOUNDS, variant))


def test_points_of_frames_equal_fuse_depth_256_default():
    """The production route: the default dispatch at 256^3 (the slab-walk brick pipeline)."""
    from dmf_amd import _lib
    pts, origins = _scans1()
    gv = _grid(256, Hh.BOUNDS)
    got = _engine().fuse_points(gv, pts, origins, _params())
    assert _lib.kernel_name(gv) == "dmf::k_bk_fuse_s<16, 32, 8>"
    gv.close()
    assert _same(got, _depth_result(256, Hh.BOUNDS, 0))


# ---------------------------------------------------------------- 2. order never matters
@pytest.mark.parametrize("variant", [SLAB, LDS_BOX])
def test_point_order_never_matters(variant):
    pts, origins = _scans1()
    rng = np.random.default_rng(8)
    shuffled = np.stack([pts[s][rng.permutation(N1)] for s in range(pts.shape[0])])
    assert not np.array_equal(shuffled.view(np.uint32), pts.view(np.uint32))
    gv = _grid(Hh.ODD_DIMS, Hh.ODD_BOUNDS, variant)
    got = _engine().fuse_points(gv, shuffled, origins, _params())
    gv.close()
    assert _same(got, _depth_result(Hh.ODD_DIMS, Hh.ODD_BOUNDS, variant))


# ---------------------------------------------------------------- 3. arbitrary segments
@pytest.mark.parametrize("variant", [LDS_BOX, CELL_WALK, SLAB])
def test_arbitrary_segments_equal_restatement(variant):
    """Random unordered points and the forced cases of fuse_points_ref.segment_case (non-finite
    coordinates, endpoints outside on each side, origins outside and inside, E == O, E in the
    origin's cell, axis-parallel and exactly diagonal rays, a ray that misses the grid, a scan
    with a NaN origin), accumulated onto non-zero counters."""
    xyz, origins, h0, m0 = FR.segment_case()
    href, mref, sref = FR.segment_reference()
    gv = _grid(FR.SEG_DIMS, FR.SEG_BOUNDS, variant)
    h, m = h0.copy(), m0.copy()
    h2, m2, s = _engine().fuse_points(gv, xyz, origins, None, h, m)
    gv.close()
    assert h2 is h and m2 is m
    assert sref[0] > 10 ** 4 and 0 < sref[2] < sref[1] < 2 * FR.SEG_N
    assert np.array_equal(s, sref)
    assert np.array_equal(h, href) and np.array_equal(m, mref)


# ---------------------------------------------------------------- 4. packet edges
@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 129])
def test_packet_edges_equal_restatement(N, S):
    """Scans of N points around the 64-ray packet size, through k_fuse_l and the brick pipeline."""
    xyz, origins, _, _ = FR.segment_case()
    xyz = np.ascontiguousarray(np.stack([xyz[s % 2, 40 + 7 * s:40 + 7 * s + N] for s in range(S)]))
    origins = np.ascontiguousarray(origins[[s % 2 for s in range(S)]])
    href, mref, sref = FR.fuse_points(FR.SEG_BOUNDS, FR.SEG_DIMS, xyz, origins)
    assert sref[1] == S * N
    for variant in (LDS_BOX, SLAB):
        gv = _grid(FR.SEG_DIMS, FR.SEG_BOUNDS, variant)
        h, m, s = _engine().fuse_points(gv, xyz, origins)
        gv.close()
        assert np.array_equal(s, sref), variant
        assert np.array_equal(h, href) and np.array_equal(m, mref), variant


# ---------------------------------------------------------------- 5. the pipeline's own branches
@pytest.mark.parametrize("knobs", [{"span": 4}, {"a_hash": 16}, {"batch_poses": 1}, {"super_poses": 2}],
                         ids=["span4", "hash16", "batch1", "super2"])
def test_pipeline_branches_with_point_source(knobs):
    """Slab-walk brick pipeline on the odd grid, the scans of the frames: several pass-A
    workgroups per scan; the hashed histogram with 16 words (overflowing workgroups are redone by
    k_bk_rays_recover); one device-cut batch per scan; super-batches of 2 scans and a remainder of
    1.  Each equals the unknobbed result, and the layout check reports no fault."""
    from dmf_amd import _lib
    pts, origins = _scans1()
    gv = _grid(Hh.ODD_DIMS, Hh.ODD_BOUNDS, SLAB, knobs)
    got = _engine().fuse_points(gv, pts, origins, _params())
    if "batch_poses" in knobs:
        assert _lib.fuse_batches_used(gv) == 5
    assert _lib.fuse_status(gv) == 0
    gv.close()
    assert _same(got, _depth_result(Hh.ODD_DIMS, Hh.ODD_BOUNDS, SLAB))


def test_hashed_histogram_overflow_with_point_source():
    """k_bk_rays_recover with a point source for certain: the odd grid has 18 bricks and a pass-A
    workgroup of these scans touches at most 10 of them, so 16 hash words never fill there; at
    256^3 (512 bricks, 0.125 m each) a workgroup's 2048 rays cross far more than 16."""
    from dmf_amd import _lib
    pts, origins = _scans1()
    gv = _grid(256, Hh.BOUNDS, 0, {"a_hash": 16})
    got = _engine().fuse_points(gv, pts, origins, _params())
    assert _lib.fuse_status(gv) == 0
    gv.close()
    assert _same(got, _depth_result(256, Hh.BOUNDS, 0))


# ---------------------------------------------------------------- 8. the C++ drop-in
def test_compat_fuse_points_driver(tmp_path, oracle):
    """compat RayTracingEngine::fusePoints from the headless driver (tests/test_gpu_compat.py's
    mechanism): 3 frames of 640x480 as scans (the oracle's back-projection, gated-out pixels NaN)
    fused into the driver's own volume give oracle.fuse_depth's counters of the frames; scan 0
    through the PointXYZRGBNormal overload gives frame 0's statistics."""
    import os
    import subprocess
    from dmf_amd import scene
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    driver = os.path.join(root, "depth-map-fusion-utils_amd", "build", "raytracing_headless")
    assert os.path.exists(driver), "build the driver: make -C depth-map-fusion-utils_amd"
    cpts, nrm = Hh.cloud()
    fposes, fdepth, _ = Hh.frames()
    poses = np.concatenate([fposes[:3], Hh.ref_style_poses()[:2]])
    np.concatenate([cpts, nrm], axis=1).astype(np.float32).tofile(tmp_path / "cloud.bin")
    scene.write_pose_file(tmp_path / "poses.txt", poses)
    depth = np.ascontiguousarray(fdepth[:3], np.uint16)
    depth.tofile(tmp_path / "depth.bin")
    xyz = np.stack([oracle.backproject(Hh.K, depth[i], poses[i]) for i in range(3)])
    pts, _ = FR.frame_points(xyz, depth, poses[:3], 200, 1000)
    pts.tofile(tmp_path / "points.bin")
    out = subprocess.run([driver, str(tmp_path / "cloud.bin"), str(tmp_path / "poses.txt"), str(tmp_path / "depth.bin"),
                          "3", str(tmp_path / "fused.bin"), str(tmp_path / "points.bin"), "3", str(pts.shape[1]),
                          str(tmp_path / "pfused.bin")], check=True, capture_output=True, text=True, timeout=600).stdout
    line = {ln.split()[0]: [int(x) for x in ln.split()[1:]] for ln in out.splitlines()
            if ln.startswith(("points ", "points_scan0 "))}
    lo, hi = cpts.min(0), cpts.max(0)
    ov = oracle.Volume()
    ov.setDimensions(float(lo[0]), float(hi[0]), float(lo[1]), float(hi[1]), float(lo[2]), float(hi[2]))
    ov.setVolumeSize(*[int(np.float32(hi[i] - lo[i]) * np.float32(125)) for i in range(3)])
    ov.constructVolume()
    ho, mo, so = oracle.fuse_depth(ov, Hh.K, depth, poses[:3], dmin=200, dmax=1000)
    _, _, s0 = oracle.fuse_depth(ov, Hh.K, depth[:1], poses[:1], dmin=200, dmax=1000)
    n = int(np.prod(ov.dims))
    raw = np.fromfile(tmp_path / "pfused.bin", np.int32)
    assert raw.size == 2 * n
    assert line["points"] == [int(x) for x in so] and so[0] > 0
    assert line["points_scan0"] == [int(x) for x in s0] and s0[0] > 0
    assert np.array_equal(raw[:n], ho) and np.array_equal(raw[n:], mo)


# ---------------------------------------------------------------- device forms
class _Dev:
    """The device forms on one volume (slab-walk brick pipeline on the odd grid) with its own
    main / input streams and torch buffers."""

    def __init__(self, variant=SLAB):
        import torch
        from dmf_amd import _lib
        self.torch, self._lib, self.L = torch, _lib, _lib.load()
        self.dev = torch.device("cuda", 0)
        self.vol = _grid(Hh.ODD_DIMS, Hh.ODD_BOUNDS, variant)
        self.main, self.inp = torch.cuda.Stream(self.dev), torch.cuda.Stream(self.dev)
        self.vol.set_stream(self.main.cuda_stream)
        self.cam = _lib.make_camera(Hh.KA, HA, WA)
        self.prm = _lib.default_fuse_params(dmin_mm=DMIN, dmax_mm=DMAX)
        nct = C.c_int64()
        _lib.check(self.L.dmf_fuse_counter_cells(self.vol._h, C.addressof(nct)))
        self.nt = nct.value
        self.counters = torch.zeros(2 * self.nt, dtype=torch.int32, device=self.dev)
        self.stats = torch.zeros(8, dtype=torch.int64, device=self.dev)
        poses, depth = _frames1()
        pts, origins = _scans1()
        self.d_depth = torch.from_numpy(depth.view(np.int16)).to(self.dev)
        self.d_poses = torch.from_numpy(poses).to(self.dev)
        self.d_pts = torch.from_numpy(pts).to(self.dev)
        self.d_org = torch.from_numpy(origins).to(self.dev)
        torch.cuda.synchronize(self.dev)

    def pipelined(self, on):
        self._lib.check(self.L.dmf_fuse_set_input_stream(self.vol._h, self.inp.cuda_stream if on else None))

    def depth(self, a, b):
        self._lib.check(self.L.dmf_fuse_depth_device(
            self.vol._h, C.addressof(self.cam), self.d_depth[a:b].data_ptr(), self.d_poses[a:b].data_ptr(), b - a,
            C.addressof(self.prm), self.counters.data_ptr(), self.counters.data_ptr() + 4 * self.nt,
            self.stats.data_ptr()))

    def points(self, a, b):
        self._lib.check(self.L.dmf_fuse_points_device(
            self.vol._h, self.d_pts[a:b].data_ptr(), self.d_org[a:b].data_ptr(), b - a, N1, C.addressof(self.prm),
            self.counters.data_ptr(), self.counters.data_ptr() + 4 * self.nt, self.stats.data_ptr()))

    def linear(self):
        torch = self.torch
        torch.cuda.synchronize(self.dev)
        lin = torch.empty(int(np.prod(self.vol.dims)), dtype=torch.int32, device=self.dev)
        out = []
        for half in range(2):
            self._lib.check(self.L.dmf_fuse_counters_to_linear_device(
                self.vol._h, self.counters.data_ptr() + 4 * self.nt * half, lin.data_ptr()))
            self.vol.synchronize()
            out.append(lin.cpu().numpy())
        return out[0], out[1], self.stats.cpu().numpy()

    def close(self):
        self.pipelined(False)
        self.vol.close()


def _sequence(pipelined):
    """depth call, point call, point call, depth call on one volume, no synchronisation between."""
    v = _Dev()
    try:
        if pipelined:
            v.pipelined(True)
        v.depth(0, 2)
        v.points(0, 3)
        v.points(3, 5)
        v.depth(2, 5)
        out = v.linear()
        assert v._lib.fuse_status(v.vol) == 0
        return out
    finally:
        v.close()


# ---------------------------------------------------------------- 6. pipelined equals serial
def test_pipelined_point_calls_equal_serial():
    """With an input stream set, point calls mixed with depth calls give the serial sequence's
    counters: every frame was fused twice, once from its pixels and once from its points."""
    hs, ms, ss = _sequence(False)
    hp, mp, sp = _sequence(True)
    assert ss[3] == 0 and sp[3] == 0
    assert np.array_equal(ss[:5], sp[:5])
    assert np.array_equal(hs, hp) and np.array_equal(ms, mp)
    h, m, s = _depth_result(Hh.ODD_DIMS, Hh.ODD_BOUNDS, SLAB)
    assert np.array_equal(hs, 2 * h) and np.array_equal(ms, 2 * m) and np.array_equal(ss[:3], 2 * s[:3])


# ---------------------------------------------------------------- 7. host and device forms
@pytest.mark.parametrize("variant", [SLAB, LDS_BOX])
def test_device_form_equals_host_form(variant):
    """Tiled counters of the device form through dmf_fuse_counters_to_linear_device against the
    host form's linear ones; after dmf_fuse_points_reserve(S, N) a device call of that size
    succeeds."""
    v = _Dev(variant)
    try:
        v._lib.check(v.L.dmf_fuse_points_reserve(v.vol._h, 5, N1, 0))
        v.points(0, 5)
        hd, md, sd = v.linear()
        assert v._lib.fuse_status(v.vol) == 0
    finally:
        v.close()
    pts, origins = _scans1()
    gv = _grid(Hh.ODD_DIMS, Hh.ODD_BOUNDS, variant)
    hh, mh, sh = _engine().fuse_points(gv, pts, origins, _params())
    gv.close()
    assert sd[3] == 0 and np.array_equal(sd[:3], sh)
    assert np.array_equal(hd, hh) and np.array_equal(md, mh)
    assert _same((hh, mh, sh), _depth_result(Hh.ODD_DIMS, Hh.ODD_BOUNDS, variant))
