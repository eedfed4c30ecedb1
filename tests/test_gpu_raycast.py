"""GPU: the log-odds ray-cast (k_rc_mask, k_rc_cast) against the pure-Python
reference tests/raycast_ref.py -- exact equality of cell, depth and statistics, through the host
form and the device form, in P > 1 batches, with outputs pre-filled by values that can never be
outputs (an unwritten pixel shows)."""
import ctypes as C

import numpy as np
import pytest

import helpers as Hh
import raycast_cases as RC
import raycast_ref as RR

pytestmark = pytest.mark.gpu

FILL_DEPTH = np.int32(-2)            # depth is -1 or rayTraceVolume's value of a voxel in range
FILL_CELL = np.uint64(1 << 63)       # a hash has 60 bits, "none" is all ones


@pytest.fixture(scope="module")
def dmf():
    import dmf_amd
    return dmf_amd


def _host(gv, K, H, W, L, poses, threshold, range_mm):
    """dmf_raycast_logodds into pre-filled outputs -> (depth, cell)."""
    from dmf_amd import _lib
    poses = np.ascontiguousarray(poses, np.float32).reshape(-1, 12)
    P = poses.shape[0]
    cam = _lib.make_camera(K, H, W)
    lo = np.ascontiguousarray(L, np.int16).reshape(-1)
    depth, cell = np.full((P, H, W), FILL_DEPTH, np.int32), np.full((P, H, W), FILL_CELL, np.uint64)
    _lib.check(gv._L.dmf_raycast_logodds(gv._h, C.addressof(cam), lo.ctypes.data, poses.ctypes.data, P, int(threshold),
                                         int(range_mm), depth.ctypes.data, cell.ctypes.data))
    return depth, cell


def _device(dc, K, H, W, d_L, poses, threshold, range_mm):
    """dmf_raycast_logodds_device on the device grid d_L -> (depth, cell, stats[2])."""
    from dmf_amd import _lib
    poses = np.ascontiguousarray(poses, np.float32).reshape(-1, 12)
    P = poses.shape[0]
    cam = _lib.make_camera(K, H, W)
    dd, dcell = dc.upload(np.full(P * H * W, FILL_DEPTH, np.int32)), dc.upload(np.full(P * H * W, FILL_CELL, np.uint64))
    dp, ds = dc.upload(poses), dc.zeros(16)
    _lib.check(dc.L.dmf_raycast_logodds_device(dc.h, C.addressof(cam), d_L, dp, P, int(threshold), int(range_mm), dd,
                                               dcell, ds))
    return (dc.download(dd, (P, H, W), np.int32), dc.download(dcell, (P, H, W), np.uint64),
            dc.download(ds, 2, np.uint64))


WALKS = (1, 2)  # DMF_KNOB_RAYCAST_WALK: the cell-by-cell walk, the walk that jumps empty bricks and tiles


def _check_both(gv, K, H, W, L, poses, threshold, range_mm, ref):
    """Host form and device form with either walk, and the Python method (the default walk), ==
    the reference."""
    import dmf_amd
    from dmf_amd import _lib
    dc = Hh.DeviceCalls(gv)
    try:
        d_L = dc.upload(np.ascontiguousarray(L, np.int16).reshape(-1))
        for walk in WALKS:
            _lib.set_knob(gv, "raycast_walk", walk)
            depth, cell = _host(gv, K, H, W, L, poses, threshold, range_mm)
            assert np.array_equal(cell, ref["cell"]), (walk, "host cell", int((cell != ref["cell"]).sum()))
            assert np.array_equal(depth, ref["depth"]), (walk, "host depth", int((depth != ref["depth"]).sum()))
            depth, cell, stats = _device(dc, K, H, W, d_L, poses, threshold, range_mm)
            assert np.array_equal(cell, ref["cell"]), (walk, "device cell", int((cell != ref["cell"]).sum()))
            assert np.array_equal(depth, ref["depth"]), (walk, "device depth", int((depth != ref["depth"]).sum()))
            assert np.array_equal(stats, ref["stats"]), (walk, stats, ref["stats"])
    finally:
        dc.close()
        _lib.set_knob(gv, "raycast_walk", 0)
    eng = dmf_amd.RayTracingEngine(dmf_amd.Camera(K, H, W))
    d2, c2 = eng.raycast_logodds(gv, np.asarray(L, np.int16).reshape(gv.dims), np.asarray(poses).reshape(-1, 3, 4),
                                 threshold, range_mm)
    assert d2.dtype == np.int32 and c2.dtype == np.uint64
    assert np.array_equal(d2, ref["depth"]) and np.array_equal(c2, ref["cell"])
    assert np.array_equal(c2 == dmf_amd.NO_CELL, ref["index"] < 0)


# surface-cell fractions of the reference: threshold -> (pose 0, pose 1, inside pose, looking away)
FRACTIONS1 = {1: (0.78, 0.65, 1.00, 0.0), 3511: (0.25, 0.19, 0.83, 0.0)}


@pytest.mark.parametrize("threshold", RC.THRESHOLDS1)
def test_fused_scene_odd_grid(dmf, threshold):
    """Four fused frames in a (72, 40, 44) grid (no power-of-two delta; tiles and mask words
    partial on every axis), cast from a fusion pose, an unrelated pose, a camera inside the grid
    and a camera that looks away."""
    ref = RC.ref1(threshold)
    frac = (ref["index"] >= 0).reshape(4, -1).mean(axis=1)
    entered = ref["length"] > 0
    assert entered[:3].all() and not entered[3].any()      # the last pose looks away: every pixel none
    if threshold in FRACTIONS1:
        # (the stated fractions are two-decimal figures of the reference: 552 / 2257 = 0.2446 is "0.25")
        assert np.allclose(frac, FRACTIONS1[threshold], atol=0.01), frac
        assert (ref["index"][:3] > 0).any()
    else:                                                   # at the clamp floor every cell is solid
        assert np.array_equal(ref["index"] == 0, entered) and np.array_equal(frac, [1, 1, 1, 0])
    assert (ref["cell"][3] == RR.NO_CELL).all() and (ref["depth"][3] == -1).all()
    _check_both(Hh.gpu_grid(RC.DIMS1, RC.BOUNDS1), RC.KA, RC.HA, RC.WA, RC.grid1(), RC.poses1(), threshold, RC.RANGE1,
                ref)


def test_sparse_grid_empty_bricks_off_origin(dmf):
    """403 solid cells in a (96, 72, 80) grid far from the origin: most rays cross wholly empty
    32^3 blocks (and so empty mask tiles of any size up to that) before a solid cell, or run off the
    grid without one."""
    L, wk, ref = RC.grid2(), RC.walk2(), RC.ref2()
    assert int((~RC.empty_blocks(L, RC.THRESHOLD2)).sum()) == 11
    hits = (ref["index"] >= 0).reshape(5, -1).sum(axis=1)
    after_empty = RC.hits_after_empty_block(wk, ref, L, RC.THRESHOLD2)
    assert hits.tolist() == [288, 171, 140, 8, 167] and after_empty.tolist() == [1, 171, 140, 3, 167]
    n = RC.HA * RC.WA
    assert n == 2257 and (n - hits >= 0.87 * n).all()
    assert (after_empty >= 1).all() and (hits < n).all()
    for q in RC.CORNERS2:                                    # brick corners and the last cell are solid
        assert L[q] == 7
    _check_both(Hh.gpu_grid(RC.DIMS2, RC.BOUNDS2), RC.KA, RC.HA, RC.WA, L, RC.poses2(), RC.THRESHOLD2, RC.RANGE2, ref)


@pytest.mark.parametrize("size", [1, 3])
@pytest.mark.parametrize("range_mm", [1, 65535])
def test_axis_aligned_and_degenerate_rays(dmf, size, range_mm):
    """Principal point on a pixel centre and identity rotation: the centre ray moves along z only
    (two axes with step 0).  One pose inside the sparse grid of case 2 and one outside it, in one
    batch; range_mm = 1 is a ray within one cell, 65535 leaves through the far face.  Threshold 0
    (sparse) and -5 (every cell solid: the first cell is the answer)."""
    K = np.array([50, 0, size // 2, 0, 50, size // 2, 0, 0, 1], np.float32)
    o = np.asarray(Hh.OFFSETS[1], np.float64)
    eye = np.eye(3, 4)
    poses = np.stack([eye, eye]).reshape(2, 12)
    inside = o + [0.1700, -0.2300, -0.3100]
    outside = o + [0.1700, -0.2300, -0.8000]
    poses[0, 3::4], poses[1, 3::4] = inside, outside
    poses = np.ascontiguousarray(poses, np.float32)
    wk = RR.Walk(RC.BOUNDS2, RC.DIMS2, K, size, size, poses, range_mm)
    centre = wk.seq[0][size // 2][size // 2]
    assert len(centre) >= 1 and len({q[:2] for q in centre}) == 1          # x and y never step
    if range_mm == 1:
        assert all(len(s) <= 2 for sr in wk.seq[0] for s in sr)
        assert all(len(s) == 0 for sr in wk.seq[1] for s in sr)              # 1 mm from outside: never enters
    else:
        assert len(centre) > 40 and len(wk.seq[1][size // 2][size // 2]) == RC.DIMS2[2]
    gv = Hh.gpu_grid(RC.DIMS2, RC.BOUNDS2)
    for threshold in (0, -5):
        _check_both(gv, K, size, size, RC.grid2(), poses, threshold, range_mm, wk.surface(RC.grid2(), threshold))


def test_device_chain_and_statelessness(dmf, oracle):
    """GPU fuse_depth -> dmf_fuse_finalize_device -> dmf_raycast_logodds_device on the same device
    buffer: equal to the host form on the downloaded grid and to the reference; a second call with
    another threshold gives that threshold's result (the mask is rebuilt); the volume's point-cloud
    queries are unchanged by a ray-cast."""
    from dmf_amd import _lib
    fposes, frames = RC.fusion_frames()
    poses = RC.poses1()[:2]
    gv = Hh.gpu_grid(RC.DIMS1, RC.BOUNDS1, clouds=[Hh.cloud()])
    eng640 = dmf.RayTracingEngine(dmf.Camera(Hh.K))
    before = [eng640.reverseRayTraceFast(gv, T, False) for T in Hh.five_poses()[:2]]
    assert any(len(g) for _, g in before)
    occupied = np.array(gv.occupied_cells_)
    L, h = gv._L, gv._h
    ncell = int(np.prod(RC.DIMS1))
    nt = C.c_int64()
    _lib.check(L.dmf_fuse_counter_cells(h, C.addressof(nt)))
    cam = _lib.make_camera(RC.KA, RC.HA, RC.WA)
    prm = dmf.FuseParams(dmin_mm=200, dmax_mm=1000)
    dc = Hh.DeviceCalls(gv)
    try:
        d_h, d_m, d_lo = dc.zeros(4 * nt.value), dc.zeros(4 * nt.value), dc.alloc(2 * ncell + 64)
        d_f, d_p = dc.upload(np.ascontiguousarray(frames, np.uint16)), dc.upload(np.ascontiguousarray(fposes, np.float32))
        _lib.check(L.dmf_fuse_depth_device(h, C.addressof(cam), d_f, d_p, len(fposes), C.addressof(prm), d_h, d_m, None))
        _lib.check(L.dmf_fuse_finalize_device(h, d_h, d_m, C.addressof(prm), d_lo))
        first = _device(dc, RC.KA, RC.HA, RC.WA, d_lo, poses, 1, RC.RANGE1)
        second = _device(dc, RC.KA, RC.HA, RC.WA, d_lo, poses, 3511, RC.RANGE1)
        _lib.set_knob(gv, "raycast_walk", 1)  # the other walk over the same scratch
        again = _device(dc, RC.KA, RC.HA, RC.WA, d_lo, poses, 1, RC.RANGE1)
        _lib.set_knob(gv, "raycast_walk", 0)
        grid = dc.download(d_lo, ncell, np.int16)
    finally:
        dc.close()
    assert _lib.fuse_status(gv) == 0
    assert np.array_equal(grid, RC.grid1())
    for got, threshold in ((first, 1), (second, 3511), (again, 1)):
        ref = RC.ref1(threshold)
        hd, hc = _host(gv, RC.KA, RC.HA, RC.WA, grid, poses, threshold, RC.RANGE1)
        assert np.array_equal(got[0], hd) and np.array_equal(got[1], hc)
        assert np.array_equal(got[0], ref["depth"][:2]) and np.array_equal(got[1], ref["cell"][:2])
        assert np.array_equal(got[2], [(ref["length"][:2] > 0).sum(), (ref["index"][:2] >= 0).sum()])
    assert not np.array_equal(first[1], second[1])
    after = [eng640.reverseRayTraceFast(gv, T, False) for T in Hh.five_poses()[:2]]
    for (f0, g0), (f1, g1) in zip(before, after):
        assert f0 == f1 and np.array_equal(g0, g1)
    assert np.array_equal(occupied, np.array(gv.occupied_cells_))


def test_status_rules_on_a_volume(dmf):
    """P = 0 and P > 65535 as the fusion refuses them (DMF_ERR_INVALID); an unconstructed volume is
    DMF_ERR_STATE; a wrong grid size or dtype is refused by the Python method; outputs may be NULL."""
    from dmf_amd import _lib
    gv = Hh.gpu_grid((8, 8, 8))
    cam = _lib.make_camera(Hh.KA, RC.HA, RC.WA)
    lo, poses = np.zeros(512, np.int16), np.ascontiguousarray(RC.poses1()[:1])
    call = lambda v, P: v._L.dmf_raycast_logodds(v._h, C.addressof(cam), lo.ctypes.data, poses.ctypes.data, P, 0, 1000,
                                                 None, None)
    assert call(gv, 0) == _lib.DMF_ERR_INVALID and call(gv, 65536) == _lib.DMF_ERR_INVALID
    assert call(gv, 1) == _lib.DMF_OK
    raw = dmf.VoxelVolume()
    assert call(raw, 1) == _lib.DMF_ERR_STATE
    eng = dmf.RayTracingEngine(dmf.Camera(Hh.KA, RC.HA, RC.WA))
    with pytest.raises(ValueError):
        eng.raycast_logodds(gv, np.zeros(511, np.int16), poses)
    with pytest.raises(ValueError):
        eng.raycast_logodds(gv, np.zeros(512, np.int32), poses)
    with pytest.raises(ValueError):
        eng.raycast_logodds(gv, lo, np.zeros((2, 5), np.float32))
