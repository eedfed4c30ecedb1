"""GPU: view gain over a fused grid and next-best-view selection (k_vg_mask,
k_vg_cast, k_vg_count) against the pure-Python reference tests/viewgain_ref.py -- exact equality
of masks, gains, statistics and selections, with every walk, through the host form, the device
form and the Python methods, with outputs pre-filled so that untouched memory shows."""
import ctypes as C
import functools

import numpy as np
import pytest

import helpers as Hh
import raycast_cases as RC
import raycast_ref as RR
import viewgain_ref as VR

pytestmark = pytest.mark.gpu

FILL = np.uint64(0xA5A5A5A5A5A5A5A5)     # masks are zeroed by the call; no gain of these grids is this
WALKS = (1, 2, 3)  # DMF_KNOB_VIEWGAIN_WALK: plain; jumps + one atomic per word; the same with a read first


@pytest.fixture(scope="module")
def dmf():
    import dmf_amd
    return dmf_amd


def _ref(walk, L, occ, free):
    """-> dict(seen bool (P,)+dims, masks (P, words) uint64, gain (P,), stats (P, 3))."""
    s, st = VR.seen(walk, L, occ, free)
    return {"seen": s, "masks": np.stack([VR.pack(m, walk.dims) for m in s]),
            "gain": s.reshape(walk.P, -1).sum(axis=1).astype(np.uint64), "stats": st}


@functools.lru_cache(maxsize=None)
def ref1(occ, free):
    return _ref(RC.walk1(), RC.grid1(), occ, free)


@functools.lru_cache(maxsize=None)
def grid3():
    """Case 3: the sparse grid of case 2 with the negative cells of L[40:64, :, 8:72] unknown."""
    L = RC.grid2().copy()
    sub = L[40:64, :, 8:72]
    sub[sub < 0] = 0
    L.setflags(write=False)
    return L


@functools.lru_cache(maxsize=None)
def ref3():
    return _ref(RC.walk2(), grid3(), 1, -1)


@functools.lru_cache(maxsize=None)
def ref_dominated():
    return _ref(RC.walk2(), RC.grid2(), 0, -6)


def _host(gv, K, H, W, L, poses, occ, free, range_mm):
    """dmf_view_gain into pre-filled outputs -> (seen, gain)."""
    from dmf_amd import _lib
    poses = np.ascontiguousarray(poses, np.float32).reshape(-1, 12)
    P, words = poses.shape[0], gv.view_gain_words()
    cam = _lib.make_camera(K, H, W)
    lo = np.ascontiguousarray(L, np.int16).reshape(-1)
    seen, gain = np.full((P, words), FILL, np.uint64), np.full(P, FILL, np.uint64)
    _lib.check(gv._L.dmf_view_gain(gv._h, C.addressof(cam), lo.ctypes.data, poses.ctypes.data, P, int(occ), int(free),
                                   int(range_mm), seen.ctypes.data, gain.ctypes.data))
    return seen, gain


def _device(dc, K, H, W, d_L, poses, occ, free, range_mm, masks=True, d_seen=None):
    """dmf_view_gain_device on the device grid d_L -> (seen or None, gain, stats[3], d_seen)."""
    from dmf_amd import _lib
    poses = np.ascontiguousarray(poses, np.float32).reshape(-1, 12)
    P, words = poses.shape[0], dc.gv.view_gain_words()
    cam = _lib.make_camera(K, H, W)
    if masks and d_seen is None:
        d_seen = dc.upload(np.full(P * words, FILL, np.uint64))
    dg, dp, ds = dc.upload(np.full(P, FILL, np.uint64)), dc.upload(poses), dc.zeros(24)
    _lib.check(dc.L.dmf_view_gain_device(dc.h, C.addressof(cam), d_L, dp, P, int(occ), int(free), int(range_mm),
                                         d_seen if masks else None, dg, ds))
    return (dc.download(d_seen, (P, words), np.uint64) if masks else None, dc.download(dg, P, np.uint64),
            dc.download(ds, 3, np.uint64), d_seen)


def _check_all(gv, K, H, W, L, poses, occ, free, range_mm, ref):
    """Host form and device form with every walk, and the Python method (the default walk), ==
    the reference."""
    import dmf_amd
    from dmf_amd import _lib
    dc = Hh.DeviceCalls(gv)
    stats = ref["stats"].sum(axis=0)
    try:
        d_L = dc.upload(np.ascontiguousarray(L, np.int16).reshape(-1))
        for walk in WALKS:
            _lib.set_knob(gv, "viewgain_walk", walk)
            seen, gain = _host(gv, K, H, W, L, poses, occ, free, range_mm)
            assert np.array_equal(gain, ref["gain"]), (walk, "host gain", gain, ref["gain"])
            assert np.array_equal(seen, ref["masks"]), (walk, "host masks", int((seen != ref["masks"]).sum()))
            seen, gain, st, _ = _device(dc, K, H, W, d_L, poses, occ, free, range_mm)
            assert np.array_equal(gain, ref["gain"]), (walk, "device gain", gain, ref["gain"])
            assert np.array_equal(seen, ref["masks"]), (walk, "device masks", int((seen != ref["masks"]).sum()))
            assert np.array_equal(st, stats), (walk, st, stats)
            none, gain, st, _ = _device(dc, K, H, W, d_L, poses, occ, free, range_mm, masks=False)
            assert none is None and np.array_equal(gain, ref["gain"]) and np.array_equal(st, stats), (walk, gain, st)
    finally:
        dc.close()
        _lib.set_knob(gv, "viewgain_walk", 0)
    eng = dmf_amd.RayTracingEngine(dmf_amd.Camera(K, H, W))
    lo, p34 = np.asarray(L, np.int16).reshape(gv.dims), np.asarray(poses).reshape(-1, 3, 4)
    g2 = eng.view_gain(gv, lo, p34, occ, free, range_mm)
    assert g2.dtype == np.uint64 and np.array_equal(g2, ref["gain"])
    g3, m3 = eng.view_gain(gv, lo, p34, occ, free, range_mm, masks=True)
    assert m3.dtype == np.uint64 and np.array_equal(g3, ref["gain"]) and np.array_equal(m3, ref["masks"])
    for p in range(len(p34)):
        assert np.array_equal(gv.view_mask_dense(m3[p]), ref["seen"][p]), p


# (occ, free) -> per pose (gain, rays stopped, unknown visits), greedy order at min_gain 5
CASE1 = {
    (1, -1): ([7106, 11841, 0, 0], [1757, 1468, 2257, 0], [34751, 87223, 0, 0], [1, 0]),
    (3511, -1): ([19908, 22043, 6514, 0], None, None, [1, 0, 2]),
    (-2000, -1): ([0, 0, 0, 0], None, None, []),
    (1, 3510): ([0, 0, 0, 0], None, None, []),
}


@pytest.mark.parametrize("thresholds", sorted(CASE1))
def test_fused_scene_mixed_tiles(dmf, thresholds):
    """Four fused frames in a (72, 40, 44) grid: all three classes in most tiles and no wholly
    free 8^3 tile, so every tile is walked cell by cell.  Solid wins where the thresholds cross
    ((1, 3510): nothing is unknown)."""
    occ, free = thresholds
    gain, stopped, visits, order = CASE1[thresholds]
    ref = ref1(occ, free)
    assert ref["gain"].tolist() == gain
    if stopped is not None:
        assert ref["stats"][:, 1].tolist() == stopped and ref["stats"][:, 2].tolist() == visits
    got, marginal = VR.greedy(ref["seen"], 5)
    assert got == order
    if thresholds == (1, -1):
        assert marginal == [11841, 4637]
        solid, unknown = VR.classes(np.asarray(RC.grid1()).reshape(RC.DIMS1), 1, -1)
        nf = solid | unknown
        assert all(nf[x:x + 8, y:y + 8, z:z + 8].any() for x in range(0, 72, 8) for y in range(0, 40, 8)
                   for z in range(0, 44, 8))                          # no wholly free tile: the mixed-tile path
    _check_all(Hh.gpu_grid(RC.DIMS1, RC.BOUNDS1), RC.KA, RC.HA, RC.WA, RC.grid1(), RC.poses1(), occ, free, RC.RANGE1, ref)


def _free_blocks(L, occ, free, B):
    solid, unknown = VR.classes(L, occ, free)
    nf = solid | unknown
    n = L.shape
    return sum(1 for x in range(0, n[0], B) for y in range(0, n[1], B) for z in range(0, n[2], B)
               if not nf[x:x + B, y:y + B, z:z + B].any())


def test_jumps_over_free_tiles_and_bricks(dmf):
    """Case 3: an unknown slab in the sparse off-origin grid.  620 of 1080 tiles and 8 of 27 bricks
    are wholly free, and rays mark unknown cells after crossing them -- the reference itself shows
    that the tile jump and the brick jump are both followed by marks."""
    L, wk, ref = grid3(), RC.walk2(), ref3()
    solid, unknown = VR.classes(L, 1, -1)
    assert int(unknown.sum()) == 110592 and int(solid.sum()) == 403
    assert _free_blocks(L, 1, -1, 8) == 620 and _free_blocks(L, 1, -1, 32) == 8
    assert VR.marks_after(wk, L, 1, -1, 8).tolist() == [1971, 2067, 2257, 1158, 2257]
    assert VR.marks_after(wk, L, 1, -1, 32).tolist() == [0, 2067, 0, 0, 2257]
    assert ref["gain"].tolist() == [55104, 56358, 53778, 10342, 31446]
    assert ref["stats"][:, 2].tolist() == [89049, 80636, 144324, 92249, 121578]
    assert ref["stats"][:, 1].tolist() == [288, 171, 140, 8, 167]
    assert VR.greedy(ref["seen"], 5)[0] == [1, 2, 0, 4, 3]
    assert VR.greedy(ref["seen"], 20000)[0] == [1] and VR.greedy(ref["seen"], 60000)[0] == []
    _check_all(Hh.gpu_grid(RC.DIMS2, RC.BOUNDS2), RC.KA, RC.HA, RC.WA, L, RC.poses2(), 1, -1, RC.RANGE2, ref)


def test_unknown_dominated_grid(dmf):
    """Thresholds (0, -6) on the sparse grid: every cell that is not solid is unknown, nothing can
    be jumped and every step marks."""
    ref = ref_dominated()
    assert _free_blocks(RC.grid2(), 0, -6, 8) == 0
    assert ref["gain"].tolist() == [168713, 164805, 173220, 88781, 86861]
    _check_all(Hh.gpu_grid(RC.DIMS2, RC.BOUNDS2), RC.KA, RC.HA, RC.WA, RC.grid2(), RC.poses2(), 0, -6, RC.RANGE2, ref)


def test_pose_batches_in_scratch(dmf):
    """d_seen = NULL with P = 5 and at most 2 poses per internal batch (3 batches, the last of one
    pose): gains and statistics equal the unbatched call's and the reference's."""
    from dmf_amd import _lib
    ref = ref3()
    gv = Hh.gpu_grid(RC.DIMS2, RC.BOUNDS2)
    dc = Hh.DeviceCalls(gv)
    try:
        d_L = dc.upload(np.ascontiguousarray(grid3()).reshape(-1))
        args = (dc, RC.KA, RC.HA, RC.WA, d_L, RC.poses2(), 1, -1, RC.RANGE2)
        _, whole, st_whole, _ = _device(*args, masks=False)
        for cap in (2, 1, 5, 7):
            _lib.set_knob(gv, "viewgain_batch", cap)
            _, gain, st, _ = _device(*args, masks=False)
            assert np.array_equal(gain, whole) and np.array_equal(st, st_whole), (cap, gain, st)
        assert np.array_equal(whole, ref["gain"]) and np.array_equal(st_whole, ref["stats"].sum(axis=0))
    finally:
        dc.close()
        _lib.set_knob(gv, "viewgain_batch", 0)


@pytest.mark.parametrize("size", [1, 3])
@pytest.mark.parametrize("range_mm", [1, 65535])
def test_axis_aligned_and_degenerate_rays(dmf, size, range_mm):
    """The cameras of the ray-cast's test of the same name: one pose inside the grid and one
    outside it.  A 1-mm ray from inside marks at most two cells; one from outside that never
    enters marks none.  Thresholds (1, -1) on case 3's grid and (0, -6) (everything unknown)."""
    K = np.array([50, 0, size // 2, 0, 50, size // 2, 0, 0, 1], np.float32)
    o = np.asarray(Hh.OFFSETS[1], np.float64)
    eye = np.eye(3, 4)
    poses = np.stack([eye, eye]).reshape(2, 12)
    poses[0, 3::4], poses[1, 3::4] = o + [0.1700, -0.2300, -0.3100], o + [0.1700, -0.2300, -0.8000]
    poses = np.ascontiguousarray(poses, np.float32)
    wk = RR.Walk(RC.BOUNDS2, RC.DIMS2, K, size, size, poses, range_mm)
    gv = Hh.gpu_grid(RC.DIMS2, RC.BOUNDS2)
    for L, occ, free in ((grid3(), 1, -1), (RC.grid2(), 0, -6)):
        ref = _ref(wk, L, occ, free)
        if range_mm == 1:
            assert all(len(s) <= 2 for sr in wk.seq[0] for s in sr) and ref["gain"][0] <= 2 * size * size
            assert all(len(s) == 0 for sr in wk.seq[1] for s in sr) and ref["gain"][1] == 0
            assert ref["stats"][1].tolist() == [0, 0, 0]
        elif free == -6:
            assert ref["gain"][0] > 40 and ref["gain"][1] > 0      # (the outside pose's centre ray meets a solid cell)
        _check_all(gv, K, size, size, L, poses, occ, free, range_mm, ref)


def test_unaligned_grid(dmf):
    """d_logodds at a base + 2 bytes between cells of 32767 (solid at every threshold): no 16-B
    load may be taken, and a neighbour read as a cell changes the masks."""
    from dmf_amd import _lib
    gv = Hh.gpu_grid(RC.DIMS1, RC.BOUNDS1)
    dc = Hh.DeviceCalls(gv)
    try:
        flat = np.ascontiguousarray(RC.grid1(), np.int16).reshape(-1)
        base = dc.upload(np.concatenate([[32767], flat, np.full(8, 32767)]).astype(np.int16))
        assert base % 16 == 0
        for walk in WALKS:
            _lib.set_knob(gv, "viewgain_walk", walk)
            for occ, free in ((1, -1), (3511, -1)):
                ref = ref1(occ, free)
                seen, gain, st, _ = _device(dc, RC.KA, RC.HA, RC.WA, base + 2, RC.poses1(), occ, free, RC.RANGE1)
                assert np.array_equal(gain, ref["gain"]) and np.array_equal(seen, ref["masks"]), (walk, occ, gain)
                assert np.array_equal(st, ref["stats"].sum(axis=0)), (walk, occ, st)
    finally:
        dc.close()
        _lib.set_knob(gv, "viewgain_walk", 0)


def test_device_chain_and_statelessness(dmf, oracle):
    """GPU fuse_depth -> dmf_fuse_finalize_device -> dmf_view_gain_device on the same device
    buffer.  A second call with other thresholds gives that pair's result; masks of a previous call
    are overwritten, not OR-ed into; a ray-cast between two view-gain calls on the same volume
    still gives its own reference, and the view gain after it its own; the volume's point-cloud
    queries are unchanged."""
    import test_gpu_raycast as TR
    from dmf_amd import _lib
    fposes, frames = RC.fusion_frames()
    poses = RC.poses1()
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
        args = (dc, RC.KA, RC.HA, RC.WA, d_lo, poses)
        first = _device(*args, 3511, -1, RC.RANGE1)                       # the larger sets first ...
        second = _device(*args, 1, -1, RC.RANGE1, d_seen=first[3])         # ... then the smaller into the same masks
        cast = TR._device(dc, RC.KA, RC.HA, RC.WA, d_lo, poses, 1, RC.RANGE1)
        _lib.set_knob(gv, "viewgain_walk", 1)
        third = _device(*args, 3511, -1, RC.RANGE1, d_seen=first[3])
        _lib.set_knob(gv, "viewgain_walk", 0)
        grid = dc.download(d_lo, ncell, np.int16)
    finally:
        dc.close()
        _lib.set_knob(gv, "viewgain_walk", 0)
    assert _lib.fuse_status(gv) == 0
    assert np.array_equal(grid, RC.grid1())
    for got, occ in ((first, 3511), (second, 1), (third, 3511)):
        ref = ref1(occ, -1)
        assert np.array_equal(got[0], ref["masks"]) and np.array_equal(got[1], ref["gain"]), occ
        assert np.array_equal(got[2], ref["stats"].sum(axis=0)), occ
    assert (ref1(3511, -1)["masks"] & ~ref1(1, -1)["masks"]).any()        # OR-ing into the old masks would show
    rc = RC.ref1(1)
    assert np.array_equal(cast[0], rc["depth"]) and np.array_equal(cast[1], rc["cell"])
    assert np.array_equal(cast[2], rc["stats"])
    after = [eng640.reverseRayTraceFast(gv, T, False) for T in Hh.five_poses()[:2]]
    for (f0, g0), (f1, g1) in zip(before, after):
        assert f0 == f1 and np.array_equal(g0, g1)
    assert np.array_equal(occupied, np.array(gv.occupied_cells_))


def _nbv(gv, dc, K, H, W, L, d_L, poses, occ, free, range_mm, min_gain):
    """-> the selections of dmf_next_best_views, dmf_next_best_views_device (with its gains) and
    dmf_greedy_set_cover_masks_device over the masks dmf_view_gain_device wrote."""
    from dmf_amd import _lib
    poses = np.ascontiguousarray(poses, np.float32).reshape(-1, 12)
    P = poses.shape[0]
    cam = _lib.make_camera(K, H, W)
    lo = np.ascontiguousarray(L, np.int16).reshape(-1)
    out = []
    for form in ("host", "device", "masks"):
        sel, nsel, gain = np.full(P, -7, np.int32), C.c_int32(-7), np.full(P, FILL, np.uint64)
        if form == "host":
            _lib.check(gv._L.dmf_next_best_views(gv._h, C.addressof(cam), lo.ctypes.data, poses.ctypes.data, P, occ, free,
                                                 range_mm, min_gain, sel.ctypes.data, C.addressof(nsel), gain.ctypes.data))
        elif form == "device":
            _lib.check(gv._L.dmf_next_best_views_device(gv._h, C.addressof(cam), d_L, dc.upload(poses), P, occ, free,
                                                        range_mm, min_gain, sel.ctypes.data, C.addressof(nsel),
                                                        gain.ctypes.data))
        else:
            _, g, _, d_seen = _device(dc, K, H, W, d_L, poses, occ, free, range_mm)
            gain[:] = g
            _lib.check(gv._L.dmf_greedy_set_cover_masks_device(gv._h, d_seen, P, gv.view_gain_words(), min_gain,
                                                               sel.ctypes.data, C.addressof(nsel)))
        assert 0 <= nsel.value <= P and (sel[nsel.value:] == -7).all(), (form, sel, nsel.value)
        out.append((form, sel[:nsel.value].tolist(), gain))
    return out


def test_next_best_views(dmf):
    """The selection of next_best_views (host and device form), of the set cover over the masks
    of dmf_view_gain_device, and of the Python method == viewgain_ref.greedy."""
    eng = dmf.RayTracingEngine(dmf.Camera(RC.KA, RC.HA, RC.WA))
    cases = [(RC.DIMS2, RC.BOUNDS2, grid3(), RC.poses2(), 1, -1, RC.RANGE2, mg, ref3()) for mg in (5, 20000, 60000)]
    cases += [(RC.DIMS1, RC.BOUNDS1, RC.grid1(), RC.poses1(), occ, -1, RC.RANGE1, 5, ref1(occ, -1))
              for occ in (1, 3511, -2000)]
    volumes = {}
    for dims, bounds, L, poses, occ, free, rng, min_gain, ref in cases:
        gv = volumes.setdefault(dims, Hh.gpu_grid(dims, bounds))
        want = VR.greedy(ref["seen"], min_gain)[0]
        dc = Hh.DeviceCalls(gv)
        try:
            d_L = dc.upload(np.ascontiguousarray(L, np.int16).reshape(-1))
            for form, sel, gain in _nbv(gv, dc, RC.KA, RC.HA, RC.WA, L, d_L, poses, occ, free, rng, min_gain):
                assert sel == want, (form, occ, min_gain, sel, want)
                assert np.array_equal(gain, ref["gain"]), (form, occ, gain)
        finally:
            dc.close()
        sel, gain = eng.next_best_views(gv, np.asarray(L, np.int16).reshape(dims), poses.reshape(-1, 3, 4), occ, free, rng,
                                        min_gain)
        assert sel.dtype == np.int32 and sel.tolist() == want and np.array_equal(gain, ref["gain"])
    assert VR.greedy(ref3()["seen"], 5)[0] == [1, 2, 0, 4, 3]


@pytest.mark.parametrize("dims", [(72, 40, 44), (8, 8, 8)])
def test_words_and_mask_index_equal_the_layout(dmf, dims):
    """dmf_view_gain_words and dmf_view_mask_index (host arithmetic over a constructed volume)
    against viewgain_ref.pack: every cell's bit is the one pack sets; outside the grid is
    DMF_ERR_INVALID with the output untouched."""
    from dmf_amd import _lib
    gv = Hh.gpu_grid(dims)
    assert gv.view_gain_words() == VR.words(dims)
    bit = np.zeros(1, np.uint64)
    rng = np.random.default_rng(3)
    cells = [(0, 0, 0), tuple(n - 1 for n in dims), (7, 7, 7)] + [tuple(int(rng.integers(0, n)) for n in dims)
                                                                  for _ in range(60)]
    for x, y, z in cells:
        _lib.check(gv._L.dmf_view_mask_index(gv._h, x, y, z, bit.ctypes.data))
        one = np.zeros(dims, bool)
        one[x, y, z] = True
        w = VR.pack(one, dims)
        i = int(bit[0])
        assert int(w[i >> 6]) == 1 << (i & 63) and int(np.count_nonzero(w)) == 1, (x, y, z, i)
    bit[0] = 77
    for x, y, z in ((-1, 0, 0), (dims[0], 0, 0), (0, dims[1], 0), (0, 0, dims[2]), (0, -1, 0), (0, 0, -1)):
        assert gv._L.dmf_view_mask_index(gv._h, x, y, z, bit.ctypes.data) == _lib.DMF_ERR_INVALID
    assert bit[0] == 77


def test_status_rules_on_a_volume(dmf):
    """P = 0 and P > 65535 as the fusion refuses them (DMF_ERR_INVALID); an unconstructed volume is
    DMF_ERR_STATE; a wrong grid size, dtype or pose shape is refused by the Python methods."""
    from dmf_amd import _lib
    gv = Hh.gpu_grid((8, 8, 8))
    cam = _lib.make_camera(Hh.KA, RC.HA, RC.WA)
    lo, poses = np.zeros(512, np.int16), np.ascontiguousarray(RC.poses1()[:1])
    gain, sel, nsel = np.full(1, FILL, np.uint64), np.full(1, -7, np.int32), C.c_int32(-7)
    gains = lambda v, P: v._L.dmf_view_gain(v._h, C.addressof(cam), lo.ctypes.data, poses.ctypes.data, P, 1, -1, 1000,
                                            None, gain.ctypes.data)
    nbv = lambda v, P: v._L.dmf_next_best_views(v._h, C.addressof(cam), lo.ctypes.data, poses.ctypes.data, P, 1, -1, 1000,
                                                5, sel.ctypes.data, C.addressof(nsel), None)
    raw = dmf.VoxelVolume()
    words = C.c_int64(-3)
    assert raw._L.dmf_view_gain_words(raw._h, C.addressof(words)) == _lib.DMF_ERR_STATE and words.value == -3
    for call in (gains, nbv):
        assert call(gv, 0) == _lib.DMF_ERR_INVALID and call(gv, 65536) == _lib.DMF_ERR_INVALID
        assert call(raw, 1) == _lib.DMF_ERR_STATE
    assert gain[0] == FILL and sel[0] == -7 and nsel.value == -7
    assert gains(gv, 1) == _lib.DMF_OK and nbv(gv, 1) == _lib.DMF_OK
    assert gain[0] > 0 and nsel.value == 1 and sel[0] == 0               # an all-zero grid is all unknown
    eng = dmf.RayTracingEngine(dmf.Camera(Hh.KA, RC.HA, RC.WA))
    for method in (eng.view_gain, eng.next_best_views):
        with pytest.raises(ValueError):
            method(gv, np.zeros(511, np.int16), poses)
        with pytest.raises(ValueError):
            method(gv, np.zeros(512, np.int32), poses)
        with pytest.raises(ValueError):
            method(gv, lo, np.zeros((2, 5), np.float32))
