"""GPU parity away from the shapes the rest of the suite uses: volumes far from the origin,
cameras with fx != fy whose lattices end in partial 8x8 tiles, and occupied counts of 0, 1 and
around a 64-bit mask word and a 256-item workgroup unit.

The unchecked jumps of the reverse march (Geom::jmarg), the forward march's unverified entry and
brick jumps (eA = 2^-21 |t_a|), the float-accumulated enumeration axes, the certified binning and
the fusion's per-brick restart all scale with the coordinate magnitude; a wrong jump does not
fault, it changes a list.  Every comparison is exact equality with the CPU oracle, whose results
are computed once per module and asserted non-empty.
"""
import functools

import numpy as np
import pytest

import helpers as Hh
from helpers import H, K, W

pytestmark = pytest.mark.gpu

REVERSE_KERNELS = [0, 4, 5, 3, 1, 2]
INT_MAX = np.iinfo(np.int32).max


def _O():
    from oracle import oracle as O
    O.lib()
    return O


def _dmf():
    import dmf_amd
    return dmf_amd


def _set_knob(gv, name, value):
    from dmf_amd import _lib
    _lib.set_knob(gv, name, value)


def _gpu_volume(dims, bounds, clouds):
    return Hh.gpu_grid(dims, bounds, clouds)


def _oracle_volume(dims, bounds, clouds):
    return Hh.oracle_grid(_O(), dims, bounds, clouds)


def _reverse_fast_expected(ov, oeng, poses):
    """viz=False lists of every pose (the flags stay as they are)."""
    return [oeng.reverseRayTraceFast(ov, T, False) for T in poses]


def _check_reverse_fast(gv, engine, poses, exp):
    found, lists = engine.reverseRayTraceFastBatch(gv, poses, viz=False)
    for i, (f, g) in enumerate(exp):
        assert f == bool(found[i]), f"pose {i}"
        assert np.array_equal(g, lists[i]), f"pose {i}: {len(g)} vs {len(lists[i])}"


def _check_forward_device(dc, occ, cam, poses, args, exp):
    """dmf_forward_first_hits_device == the oracle's (k, hash) of every pose; returns the march
    samples the call counted."""
    Kc, Hc, Wc = cam
    k, slot, samples = dc.forward(Kc, Hc, Wc, poses, *args)
    for p, (ko, ho) in enumerate(exp):
        assert np.array_equal(k[p], ko), f"pose {p}"
        hit = ko >= 0
        assert (slot[p][~hit] == -1).all(), f"pose {p}"
        assert np.array_equal(occ[slot[p][hit]], ho[hit]), f"pose {p}"
    return samples


# =============================================================================== A. off-origin
OFF_CASES = [(oi, n) for oi in range(len(Hh.OFFSETS)) for n in (64, 100)]
FWD_ARGS = (10, 10, 5, 5)


def _off_inputs(oi):
    o = Hh.OFFSETS[oi]
    pts, nn = Hh.cloud()
    return Hh.shifted_bounds(o), (Hh.shift_points(pts, o), nn), Hh.shift_poses(Hh.five_poses(), o)


@functools.lru_cache(maxsize=None)
def _off_oracle(oi, n):
    """The oracle's volume and every expected result of offset oi at n^3, computed once."""
    O = _O()
    bounds, cl, poses = _off_inputs(oi)
    ov = _oracle_volume(n, bounds, [cl])
    oeng = O.Engine(K, H, W)
    e = {"ov": ov, "occ": ov.occupied_cells_.copy(), "dense": ov.occupancy_dense(), "counts": ov.voxel_table()[2:]}
    e["fast"] = _reverse_fast_expected(ov, oeng, poses)
    e["fwd"] = [oeng.forward_first_hits(ov, T, *FWD_ARGS) for T in poses]
    e["min"] = [oeng.rayTraceAndGetMinimum(ov, T, 1, True) for T in poses]
    e["points"] = [oeng.rayTraceAndGetPoints(ov, T, 10, True) for T in poses]
    ov.reset_flags()
    e["good_points"] = [oeng.rayTraceAndGetGoodPoints(ov, T, 10, True) for T in poses]
    # one viz=True round on reset flags: reverseRayTrace on two poses, then rayTraceVolume
    ov.reset_flags()
    e["full"] = [oeng.reverseRayTrace(ov, T, True) for T in poses[:2]]
    e["zbuf"] = oeng.rayTraceVolume(ov, poses[2])
    e["flags"] = tuple(a.copy() for a in ov.voxel_table()[:2])
    ov.reset_flags()
    return e


def _off_costmap_poses(oi):
    bounds, _, poses = _off_inputs(oi)
    rng = np.random.default_rng(7)
    inner = np.tile(poses[:1], (6, 1))
    lo, hi = np.array(bounds[0::2]), np.array(bounds[1::2])
    inner[:, 3::4] = (lo + (hi - lo) * rng.uniform(0.2, 0.8, (6, 3))).astype(np.float32)
    return np.concatenate([poses, inner])


@pytest.mark.parametrize("oi,n", OFF_CASES)
def test_offorigin_integrate(oi, n):
    """integratePointCloud of a cloud around OFFSETS[oi]: occupied list (order included), dense
    occupancy and per-voxel counts (the certified binning at |x| up to 2000 m)."""
    e = _off_oracle(oi, n)
    bounds, cl, _ = _off_inputs(oi)
    gv = _gpu_volume(n, bounds, [cl])
    assert len(e["occ"]) > 1000 and e["counts"][0].sum() > 0
    assert np.array_equal(e["occ"], gv.occupied_cells_)
    assert np.array_equal(e["dense"], gv.occupancy_dense())
    gnp, gnn = gv.voxel_counts()
    assert np.array_equal(e["counts"][0], gnp) and np.array_equal(e["counts"][1], gnn)


@pytest.mark.parametrize("kernel", REVERSE_KERNELS)
@pytest.mark.parametrize("oi,n", OFF_CASES)
def test_offorigin_reverse_fast(oi, n, kernel):
    """reverseRayTraceFast off-origin, every march kernel, with the brick distance field saturated
    at the default and at 1 brick: the unchecked jumps' margin (Geom::jmarg, 32 ulp of the largest
    |bound|) must keep every list exact."""
    e = _off_oracle(oi, n)
    bounds, cl, poses = _off_inputs(oi)
    gv = _gpu_volume(n, bounds, [cl])
    engine = _dmf().RayTracingEngine(_dmf().Camera(K, H, W))
    assert sum(len(g) for _, g in e["fast"]) > 0 and sum(len(g) > 0 for _, g in e["fast"]) >= 3
    _set_knob(gv, "reverse_kernel", kernel)
    for cap in (0, 1):
        _set_knob(gv, "bdist_cap", cap)
        _check_reverse_fast(gv, engine, poses, e["fast"])


@pytest.mark.parametrize("oi,n", OFF_CASES)
def test_offorigin_reverse_full_and_volume(oi, n):
    """One viz=True round off-origin: reverseRayTrace (the float-accumulated axes, k_float_axes) on
    two poses, rayTraceVolume's z-buffer, then the view / good flags of every voxel."""
    e = _off_oracle(oi, n)
    bounds, cl, poses = _off_inputs(oi)
    gv = _gpu_volume(n, bounds, [cl])
    engine = _dmf().RayTracingEngine(_dmf().Camera(K, H, W))
    assert all(len(g) > 0 for _, g in e["full"]) and (e["zbuf"] >= 0).any()
    assert e["flags"][0].any() and e["flags"][1].any()
    for T, (f, g) in zip(poses[:2], e["full"]):
        f2, g2 = engine.reverseRayTrace(gv, T, True)
        assert f == f2 and np.array_equal(g, g2)
    assert np.array_equal(e["zbuf"], engine.rayTraceVolume(gv, poses[2]))
    gview, ggood = gv.voxel_flags()
    assert np.array_equal(e["flags"][0], gview) and np.array_equal(e["flags"][1], ggood)


@pytest.mark.parametrize("oi,n", OFF_CASES)
def test_offorigin_forward_first_hits(oi, n):
    """Forward first hits off-origin: the host form with empty-space skipping on and off, the
    batched device form with every kernel (the entry jump's and the brick jumps' margins grow with
    |t_a|)."""
    e = _off_oracle(oi, n)
    bounds, cl, poses = _off_inputs(oi)
    gv = _gpu_volume(n, bounds, [cl])
    engine = _dmf().RayTracingEngine(_dmf().Camera(K, H, W))
    for ko, _ in e["fwd"]:
        assert (ko >= 0).sum() > 1000 and (ko < 0).any()
    for skip in (0, -1):
        _set_knob(gv, "fwd_skip", skip)
        for T, (ko, ho) in zip(poses, e["fwd"]):
            kg, hg = engine.forward_first_hits(gv, T, *FWD_ARGS)
            assert np.array_equal(ko, kg) and np.array_equal(ho[ko >= 0], hg[kg >= 0])
    _set_knob(gv, "fwd_skip", 0)
    dc = Hh.DeviceCalls(gv)
    try:
        for fk in (0, 1, 2):
            _set_knob(gv, "fwd_kernel", fk)
            _check_forward_device(dc, e["occ"], (K, H, W), poses, FWD_ARGS, e["fwd"])
    finally:
        dc.close()


@pytest.mark.parametrize("oi,n", OFF_CASES)
def test_offorigin_forward_family(oi, n):
    e = _off_oracle(oi, n)
    bounds, cl, poses = _off_inputs(oi)
    gv = _gpu_volume(n, bounds, [cl])
    engine = _dmf().RayTracingEngine(_dmf().Camera(K, H, W))
    assert max(e["min"]) > 0 and all(len(g) > 0 for _, g in e["points"])
    assert sum(len(g) for _, g in e["good_points"]) > 0
    for i, T in enumerate(poses):
        assert e["min"][i] == engine.rayTraceAndGetMinimum(gv, T, 1, True)
        f, g = engine.rayTraceAndGetPoints(gv, T, 10, True)
        assert e["points"][i][0] == f and np.array_equal(e["points"][i][1], g)
    gv.reset_flags()
    for i, T in enumerate(poses):
        f, g = engine.rayTraceAndGetGoodPoints(gv, T, 10, True)
        assert e["good_points"][i][0] == f and np.array_equal(e["good_points"][i][1], g)


@pytest.mark.parametrize("oi,n", OFF_CASES)
def test_offorigin_collision_cost_map(oi, n):
    e = _off_oracle(oi, n)
    bounds, cl, _ = _off_inputs(oi)
    gv = _gpu_volume(n, bounds, [cl])
    centres = _off_costmap_poses(oi)
    exp = _O().collision_cost_map(e["ov"], centres)
    coll = exp == INT_MAX
    assert coll.any() and not coll.all()
    assert np.array_equal(exp, _dmf().collision_cost_map(gv, centres))


def _off_frames(oi):
    poses, depth, _ = Hh.frames()
    return Hh.shift_poses(poses[:3], Hh.OFFSETS[oi]), depth[:3]


@functools.lru_cache(maxsize=None)
def _off_fuse_oracle(oi, n):
    O = _O()
    poses, depth = _off_frames(oi)
    ov = _oracle_volume(n, Hh.shifted_bounds(Hh.OFFSETS[oi]), [])
    return O.fuse_depth(ov, K, depth, poses, dmin=200, dmax=1000)


def _check_fuse(oi, n, variant):
    from dmf_amd import _lib
    dmf = _dmf()
    ho, mo, so = _off_fuse_oracle(oi, n)
    assert so[0] > 1_000_000 and so[2] > 0 and ho.any() and mo.any()
    poses, depth = _off_frames(oi)
    gv = _gpu_volume(n, Hh.shifted_bounds(Hh.OFFSETS[oi]), [])
    _lib.set_variant(gv, variant)
    engine = dmf.RayTracingEngine(dmf.Camera(K, H, W))
    hg, mg, sg = engine.fuse_depth(gv, depth, poses, dmf.FuseParams(dmin_mm=200, dmax_mm=1000))
    assert np.array_equal(so, sg)
    assert np.array_equal(ho, hg) and np.array_equal(mo, mg)
    return _lib.kernel_name(gv)


@pytest.mark.parametrize("variant", [57, 40, 31])
@pytest.mark.parametrize("oi,n", OFF_CASES)
def test_offorigin_fuse(oi, n, variant):
    """3D-DDA fusion of 3 frames into an off-origin grid, every implementation: counters and
    statistics (the brick pipeline restarts the walk per brick from coordinates of this size)."""
    name = _check_fuse(oi, n, variant)
    assert name.startswith({57: "dmf::k_bk_fuse_s<", 40: "dmf::k_bk_fuse<", 31: "dmf::k_fuse_l<"}[variant])


def test_offorigin_fuse_default_256():
    """The default dispatch at 256^3 (the brick pipeline's production kernel) around OFFSETS[0]."""
    assert _check_fuse(0, 256, 0).startswith("dmf::k_bk_fuse_s<")


# =============================================================================== B. camera shapes
CAMS = {"Ka": (Hh.KA, Hh.KA_WH[1], Hh.KA_WH[0]), "Kb": (Hh.KB, Hh.KB_WH[1], Hh.KB_WH[0])}  # (K, H, W)
# (camera, rdelta, cdelta) -> lattice R x C and its 8x8 tiles: every lattice ends in partial tiles
LATTICES = [("Ka", 1, 1, (37, 61), 40), ("Ka", 2, 3, (19, 21), 9), ("Ka", 5, 5, (8, 13), 2),
            ("Ka", 37, 61, (1, 1), 1), ("Kb", 1, 1, (149, 203), 494), ("Kb", 2, 3, (75, 68), 90),
            ("Kb", 5, 5, (30, 41), 24)]
ZSTART, ZDELTA = 10, 7
LAST_K = (1000 - 1 - ZSTART) // ZDELTA  # the march samples k = 0 .. LAST_K (zd < k_ZMax mm)


@functools.lru_cache(maxsize=None)
def _cam_volume():
    return Hh.oracle_volume(_O(), n=64)


@functools.lru_cache(maxsize=None)
def _cam_forward_oracle(cam, rd, cd):
    Kc, Hc, Wc = CAMS[cam]
    oeng = _O().Engine(Kc, Hc, Wc)
    return [oeng.forward_first_hits(_cam_volume(), T, ZSTART, ZDELTA, rd, cd) for T in Hh.five_poses()]


@pytest.mark.parametrize("cam,rd,cd,shape,tiles", LATTICES)
def test_camera_forward_lattices(cam, rd, cd, shape, tiles):
    """Forward first hits with fx != fy and a fractional principal point on lattices that are no
    multiple of the 8x8 tile (the `ri < R && ci < C` guards, k_forward_q's nitems tail and refill
    over out-of-lattice lanes, k_forward_x's tile tail and its bands when there are fewer than 8
    units): the host form and the batched device form of every kernel, with skipping on and off.
    d_slot is compared through occupied_cells_; d_stats[0] with skipping off is the sum over
    pixels of the samples fwd_ray evaluates (k + 1 up to a hit, else LAST_K + 1), and skipping
    never evaluates more."""
    Kc, Hc, Wc = CAMS[cam]
    exp = _cam_forward_oracle(cam, rd, cd)
    R, Cc = exp[0][0].shape
    assert (R, Cc) == shape and ((R + 7) // 8) * ((Cc + 7) // 8) == tiles
    assert (R % 8 or Cc % 8) and ZSTART + LAST_K * ZDELTA < 1000 <= ZSTART + (LAST_K + 1) * ZDELTA
    allk = np.stack([ko for ko, _ in exp])
    assert (allk >= 0).any()
    if R * Cc > 1:
        assert all((ko >= 0).any() and (ko < 0).any() for ko, _ in exp)
    want_samples = int(np.where(allk >= 0, allk + 1, LAST_K + 1).sum())
    poses = Hh.five_poses()
    gv = Hh.gpu_volume(n=64)
    occ = np.asarray(gv.occupied_cells_)
    engine = _dmf().RayTracingEngine(_dmf().Camera(Kc, Hc, Wc))
    dc = Hh.DeviceCalls(gv)
    try:
        for skip in (0, -1):
            _set_knob(gv, "fwd_skip", skip)
            for T, (ko, ho) in zip(poses, exp):
                kg, hg = engine.forward_first_hits(gv, T, ZSTART, ZDELTA, rd, cd)
                assert np.array_equal(ko, kg) and np.array_equal(ho[ko >= 0], hg[kg >= 0])
            for fk in (0, 1, 2):
                _set_knob(gv, "fwd_kernel", fk)
                samples = _check_forward_device(dc, occ, (Kc, Hc, Wc), poses, (ZSTART, ZDELTA, rd, cd), exp)
                if skip == -1:
                    assert samples == want_samples, (fk, samples, want_samples)
                else:
                    assert 0 < samples <= want_samples, (fk, samples, want_samples)
    finally:
        dc.close()


@pytest.mark.parametrize("cam", ["Ka", "Kb"])
def test_camera_marches(cam):
    """project() / deproject_valid() take fx, fy (and their reciprocals) separately: reverse fast
    (kernels 0, 5, 1), reverse full, rayTraceVolume, the forward family and the back-projection
    with a camera whose fx != fy, whose principal point is fractional and whose image is no
    multiple of anything."""
    from dmf_amd import scene
    O = _O()
    Kc, Hc, Wc = CAMS[cam]
    ov = _cam_volume()
    oeng = O.Engine(Kc, Hc, Wc)
    poses = Hh.five_poses()
    gv = Hh.gpu_volume(n=64)
    engine = _dmf().RayTracingEngine(_dmf().Camera(Kc, Hc, Wc))
    fast = _reverse_fast_expected(ov, oeng, poses)
    assert sum(len(g) for _, g in fast) > 0
    for kernel in (0, 5, 1):
        _set_knob(gv, "reverse_kernel", kernel)
        _check_reverse_fast(gv, engine, poses, fast)
    ov.reset_flags()
    try:
        n_full = 0
        for T in poses[:2]:
            f, g = oeng.reverseRayTrace(ov, T, True)
            f2, g2 = engine.reverseRayTrace(gv, T, True)
            assert f == f2 and np.array_equal(g, g2)
            n_full += len(g)
        zo = oeng.rayTraceVolume(ov, poses[2])
        assert n_full > 0 and (zo >= 0).any() and (zo < 0).any()
        assert np.array_equal(zo, engine.rayTraceVolume(gv, poses[2]))
        assert ov.voxel_table()[0].any() and Hh.flags_equal(ov, gv)
        ov.reset_flags()
        gv.reset_flags()
        n_pts = n_good = 0
        mins = []
        for T in poses:
            mins.append(oeng.rayTraceAndGetMinimum(ov, T, 1, True))
            assert mins[-1] == engine.rayTraceAndGetMinimum(gv, T, 1, True)
            for sparse in (True, False):
                f, g = oeng.rayTraceAndGetPoints(ov, T, 10, sparse)
                f2, g2 = engine.rayTraceAndGetPoints(gv, T, 10, sparse)
                assert f == f2 and np.array_equal(g, g2)
                n_pts += len(g)
                f, g = oeng.rayTraceAndGetGoodPoints(ov, T, 10, sparse)
                f2, g2 = engine.rayTraceAndGetGoodPoints(gv, T, 10, sparse)
                assert f == f2 and np.array_equal(g, g2)
                n_good += len(g)
        assert max(mins) > 0 and n_pts > 0 and n_good > 0
        assert Hh.flags_equal(ov, gv)
    finally:
        ov.reset_flags()
    holes = 0
    for T in poses:
        depth = scene.render(Kc, Wc, Hc, T)[0]
        assert (depth > 0).sum() > 500 and len(np.unique(depth)) > 40
        holes += int((depth == 0).sum())
        xo = O.backproject(Kc, depth, T)
        xg = engine.backproject(gv, depth, T)
        assert np.array_equal(xo.view(np.uint32), xg.view(np.uint32))
    assert holes > 0  # pixels without depth (back-projected to the camera centre) are covered too


# =============================================================================== C. occupied counts
COUNTS = [0, 1, 63, 64, 65, 255, 256, 257]
CN = 40  # grid cells per axis


def _count_cloud(V):
    if V == 0:
        return []
    return [Hh.cell_cloud(V, CN)]


@functools.lru_cache(maxsize=None)
def _count_poses():
    from dmf_amd import scene
    return scene.fibonacci_poses(3, seed=11)


@functools.lru_cache(maxsize=None)
def _count_oracle(V):
    O = _O()
    ov = _oracle_volume(CN, Hh.BOUNDS, _count_cloud(V))
    oeng = O.Engine(K, H, W)
    poses = _count_poses()
    e = {"ov": ov, "occ": ov.occupied_cells_.copy()}
    assert len(e["occ"]) == V
    e["fast"] = _reverse_fast_expected(ov, oeng, poses)
    # per pose, on reset flags: the view / good flags one viz=True call sets
    e["viz"] = []
    for T in poses:
        ov.reset_flags()
        f, g = oeng.reverseRayTraceFast(ov, T, True)
        view, good = (a.copy() for a in ov.voxel_table()[:2])
        e["viz"].append((f, g, view, good))
    ov.reset_flags()
    if V >= 63:  # the inputs are not vacuous: 12 .. 58 good voxels per pose
        assert all(12 <= len(g) <= 58 for _, g in e["fast"]), [len(g) for _, g in e["fast"]]
        assert all(view.any() for _, _, view, _ in e["viz"])
    return e


@pytest.mark.parametrize("kernel", REVERSE_KERNELS)
@pytest.mark.parametrize("V", COUNTS)
def test_count_edges_reverse(V, kernel):
    """Every reverse kernel, k_mask_to_slots and the compaction at V = 0, 1, 64 +- 1 and 256 +- 1
    occupied cells: found, the lists and the viz flags of each pose."""
    e = _count_oracle(V)
    gv = _gpu_volume(CN, Hh.BOUNDS, _count_cloud(V))
    assert np.array_equal(e["occ"], gv.occupied_cells_)
    engine = _dmf().RayTracingEngine(_dmf().Camera(K, H, W))
    _set_knob(gv, "reverse_kernel", kernel)
    poses = _count_poses()
    _check_reverse_fast(gv, engine, poses, e["fast"])
    for T, (f, g, view, good) in zip(poses, e["viz"]):
        gv.reset_flags()
        f2, g2 = engine.reverseRayTraceFast(gv, T, True)
        assert f == f2 and np.array_equal(g, g2)
        gview, ggood = gv.voxel_flags()
        assert np.array_equal(view, gview) and np.array_equal(good, ggood)


@pytest.mark.parametrize("kernel", REVERSE_KERNELS)
@pytest.mark.parametrize("V", COUNTS)
def test_count_edges_device_masks(V, kernel):
    """dmf_reverse_visibility_device at the count edges: d_good's bits are the oracle's lists,
    d_visible's bits are the voxels whose `view` one viz=True call of that pose sets (the mask is
    filled with viz = 0 too: every kernel writes it unconditionally), no bit lies past slot V - 1,
    and d_stats[1] counts one voxel ray per (voxel, pose)."""
    e = _count_oracle(V)
    gv = _gpu_volume(CN, Hh.BOUNDS, _count_cloud(V))
    _set_knob(gv, "reverse_kernel", kernel)
    poses = _count_poses()
    dc = Hh.DeviceCalls(gv)
    try:
        vis, good, stats = dc.reverse(K, H, W, poses, viz=False)
    finally:
        dc.close()
    assert vis.shape == good.shape == (len(poses), (V + 63) // 64)
    slot = {int(h): i for i, h in enumerate(e["occ"])}
    for p, (_, g, view, _) in enumerate(e["viz"]):
        gbits, gpast = Hh.mask_bits(good[p], V)
        vbits, vpast = Hh.mask_bits(vis[p], V)
        assert not gpast and not vpast
        want = np.zeros(V, bool)
        want[np.array([slot[int(h)] for h in g], np.int64)] = True
        assert np.array_equal(gbits, want), p
        assert np.array_equal(vbits, view != 0), p
    assert int(stats[1]) == V * len(poses)
    if any(view.any() for _, _, view, _ in e["viz"]):  # a visible voxel's march took samples
        assert int(stats[0]) > 0
    assert not gv.voxel_flags()[0].any()  # viz = 0 leaves the flags alone


@pytest.mark.parametrize("V", COUNTS)
def test_count_edges_set_cover(V):
    """Greedy set cover over 3 poses at the count edges (min_gain 1), from the poses and from caller
    masks of 1 (V <= 64), 2 (V = 65), 4 and 5 (V = 257) words."""
    O = _O()
    e = _count_oracle(V)
    gv = _gpu_volume(CN, Hh.BOUNDS, _count_cloud(V))
    engine = _dmf().RayTracingEngine(_dmf().Camera(K, H, W))
    poses = _count_poses()
    sets = [g for _, g in e["fast"]]
    exp = O.greedy_set_cover(sets, 1)
    if V >= 63:
        assert len(exp) >= 2
    assert np.array_equal(exp, engine.setCover(gv, poses, 1))
    words = (V + 63) // 64
    assert words == {0: 0, 1: 1, 63: 1, 64: 1, 65: 2, 255: 4, 256: 4, 257: 5}[V]
    slot = {int(h): i for i, h in enumerate(e["occ"])}
    masks = np.zeros((len(poses), words), np.uint64)
    for p, st in enumerate(sets):
        for h in st:
            i = slot[int(h)]
            masks[p, i // 64] |= np.uint64(1) << np.uint64(i % 64)
    dc = Hh.DeviceCalls(gv)
    try:
        assert np.array_equal(exp, dc.cover_masks(masks, 1))
    finally:
        dc.close()


def test_empty_volume_queries():
    """A constructed volume with nothing integrated: every query returns what the oracle returns
    (no list, minimum -1, k = -1 and z-buffer -1 everywhere, no collision) and no call fails."""
    O = _O()
    dmf = _dmf()
    ov, gv = Hh.volume_pair(O, CN)
    oeng = O.Engine(K, H, W)
    engine = dmf.RayTracingEngine(dmf.Camera(K, H, W))
    poses = _count_poses()
    assert len(gv.occupied_cells_) == 0 and gv.info()["num_points"] == 0
    assert not gv.occupancy_dense().any() and len(gv.voxel_counts()[0]) == 0 and len(gv.voxel_flags()[0]) == 0
    off, pts, nrm = gv.export()
    assert off.tolist() == [0] and len(pts) == 0 and len(nrm) == 0
    T = poses[0]
    for fn in ("reverseRayTraceFast", "reverseRayTrace"):
        for viz in (False, True):
            assert getattr(oeng, fn)(ov, T, viz)[0] is False
            f, g = getattr(engine, fn)(gv, T, viz)
            assert f is False and len(g) == 0
    for fn in ("rayTraceAndGetPoints", "rayTraceAndGetGoodPoints"):
        fo, go = getattr(oeng, fn)(ov, T, 10, True)
        f, g = getattr(engine, fn)(gv, T, 10, True)
        assert (fo, len(go)) == (False, 0) and (f, len(g)) == (False, 0)
    assert oeng.rayTraceAndGetMinimum(ov, T, 1, True) == -1 == engine.rayTraceAndGetMinimum(gv, T, 1, True)
    engine.rayTrace(gv, T)
    engine.rayTraceAndClassify(gv, T)
    ko, _ = oeng.forward_first_hits(ov, T, 10, 10, 5, 5)
    kg, hg = engine.forward_first_hits(gv, T, 10, 10, 5, 5)
    assert (ko == -1).all() and np.array_equal(ko, kg) and not hg.any()
    zo = oeng.rayTraceVolume(ov, T)
    assert (zo == -1).all() and np.array_equal(zo, engine.rayTraceVolume(gv, T))
    cm = O.collision_cost_map(ov, poses)
    assert not (cm == INT_MAX).any() and np.array_equal(cm, dmf.collision_cost_map(gv, poses))
    c = poses[:, 3::4]
    assert not dmf.will_collide(gv, c, c[::-1]).any()
    assert len(engine.setCover(gv, poses, 1)) == 0 == len(O.greedy_set_cover([[], [], []], 1))
    dc = Hh.DeviceCalls(gv)
    try:
        for fk in (0, 1, 2):
            _set_knob(gv, "fwd_kernel", fk)
            k, slot, _ = dc.forward(K, H, W, poses, 10, 10, 5, 5)
            assert (k == -1).all() and (slot == -1).all()
        vis, good, stats = dc.reverse(K, H, W, poses)
        assert vis.size == 0 and good.size == 0 and not stats.any()
    finally:
        dc.close()
