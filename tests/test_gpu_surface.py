"""GPU: the surface extraction (csrc/dmf_surface.hip) against the numpy restatement
tests/surface_ref.py -- exact equality of the hashes, of the bit patterns of centres and normals and
of both counts, through the host form, the device form and the Python method, with outputs
pre-filled by values that can never be results (an unwritten or overwritten entry shows)."""
import ctypes as C

import numpy as np
import pytest

import helpers as Hh
import raycast_cases as RC
import surface_ref as SR

pytestmark = pytest.mark.gpu

FILL_HASH = np.uint64(1 << 63)            # a hash has 60 bits
FILL_F32 = np.uint32(0x7FC00123)          # a NaN with a payload: no centre, no normal component
GUARD = 3                                  # entries kept after cap


def _filled(cap):
    n = cap + GUARD
    return (np.full(n, FILL_HASH, np.uint64), np.full(3 * n, FILL_F32, np.uint32).view(np.float32),
            np.full(3 * n, FILL_F32, np.uint32).view(np.float32))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32)


def _host(gv, L, occ, free, cap, use=(True, True, True)):
    """dmf_grid_surface into pre-filled outputs of cap + GUARD entries -> (status, n, n_solid, hash, xyz, normals)."""
    lo = np.ascontiguousarray(L, np.int16).reshape(-1)
    h, xyz, nrm = _filled(cap)
    n, ns = C.c_int64(-1), C.c_int64(-1)
    p = [a.ctypes.data if u else None for a, u in zip((h, xyz, nrm), use)]
    st = gv._L.dmf_grid_surface(gv._h, lo.ctypes.data, int(occ), int(free), *p, int(cap), C.addressof(n), C.addressof(ns))
    return st, n.value, ns.value, h, xyz, nrm


def _device(dc, d_L, occ, free, cap, use=(True, True, True)):
    """dmf_grid_surface_device into pre-filled device outputs of cap + GUARD entries -> (count[2], hash, xyz, normals)."""
    from dmf_amd import _lib
    h, xyz, nrm = _filled(cap)
    dh, dx, dn = dc.upload(h), dc.upload(xyz), dc.upload(nrm)
    dcnt = dc.upload(np.full(2, FILL_HASH, np.uint64))
    p = [d if u else None for d, u in zip((dh, dx, dn), use)]
    _lib.check(dc.L.dmf_grid_surface_device(dc.h, d_L, int(occ), int(free), *p, int(cap), dcnt))
    return (dc.download(dcnt, 2, np.uint64), dc.download(dh, h.shape, np.uint64), dc.download(dx, xyz.shape, np.float32),
            dc.download(dn, nrm.shape, np.float32))


def _assert_prefix(ref, m, h, xyz, nrm, use=(True, True, True), what=""):
    """The first m entries equal the reference's; everything after them is still the fill."""
    if use[0]:
        assert np.array_equal(h[:m], ref["hash"][:m]), (what, "hash")
        assert (h[m:] == FILL_HASH).all(), (what, "hash guard")
    else:
        assert (h == FILL_HASH).all(), (what, "unused hash")
    for name, a, on in (("xyz", xyz, use[1]), ("normals", nrm, use[2])):
        b = _bits(a)
        if on:
            bad = int((b[:3 * m] != _bits(ref[name][:m])).sum())
            assert bad == 0, (what, name, bad)
            assert (b[3 * m:] == FILL_F32).all(), (what, name, "guard")
        else:
            assert (b == FILL_F32).all(), (what, "unused", name)


def _check_all(gv, bounds, dims, L, occ, free, ref=None):
    """Host form, device form and the Python method == the reference (exactly, bit patterns)."""
    from dmf_amd import _lib
    ref = ref or SR.surface(bounds, dims, L, occ, free)
    m, solid = ref["count"]
    st, n, ns, h, xyz, nrm = _host(gv, L, occ, free, m)
    assert st == _lib.DMF_OK and (n, ns) == (m, solid), (st, n, ns, m, solid)
    _assert_prefix(ref, m, h, xyz, nrm, what="host")
    dc = Hh.DeviceCalls(gv)
    try:
        d_L = dc.upload(np.ascontiguousarray(L, np.int16).reshape(-1))
        cnt, h, xyz, nrm = _device(dc, d_L, occ, free, m + 2)       # more room than needed: nothing past count
        assert cnt.tolist() == [m, solid], (cnt, m, solid)
        _assert_prefix(ref, m, h, xyz, nrm, what="device")
    finally:
        dc.close()
    h2, x2, n2 = gv.extract_surface(np.asarray(L, np.int16).reshape(dims), occ, free)
    assert h2.dtype == np.uint64 and x2.dtype == np.float32 and n2.dtype == np.float32
    assert h2.shape == (m,) and x2.shape == (m, 3) and n2.shape == (m, 3)
    assert np.array_equal(h2, ref["hash"]) and np.array_equal(_bits(x2), _bits(ref["xyz"]))
    assert np.array_equal(_bits(n2), _bits(ref["normals"]))
    return ref


@pytest.mark.parametrize("thresholds", SR.THRESHOLDS1)
def test_fused_scene_odd_grid(thresholds):
    """Four fused frames in a (72, 40, 44) grid: tiles and mask words partial on every axis."""
    ref = SR.ref1(thresholds)
    assert ref["count"] == SR.COUNTS1[thresholds]
    _check_all(Hh.gpu_grid(RC.DIMS1, RC.BOUNDS1), RC.BOUNDS1, RC.DIMS1, RC.grid1(), *thresholds, ref=ref)


@pytest.mark.parametrize("k", range(len(SR.RANDOM_DIMS)))
def test_random_grids(k):
    """Dense random values: surface cells on every face of the grid, in every word and byte
    position; a 1-cell grid; grids thinner than a tile."""
    dims, ref = SR.RANDOM_DIMS[k], SR.ref_random(k)
    assert ref["count"][0] == SR.RANDOM_COUNTS[k]
    _check_all(Hh.gpu_grid(dims, Hh.ODD_BOUNDS), Hh.ODD_BOUNDS, dims, SR.random_grid(k), 1, -1, ref=ref)


@pytest.mark.parametrize("dims", [(9, 5, 129), (3, 10, 300)])
def test_long_rows_several_chunks(dims):
    """Rows of more than 128 cells: the emit pass ranks a row's cells over several chunks of 16
    tiles (129: the second chunk holds one partial tile; 300: three chunks, every wave of each)."""
    L = np.random.default_rng(11).integers(-3, 4, dims).astype(np.int16)
    ref = _check_all(Hh.gpu_grid(dims, Hh.ODD_BOUNDS), Hh.ODD_BOUNDS, dims, L, 1, -1)
    per_row = np.bincount(ref["cells"][:, 0] * dims[1] + ref["cells"][:, 1], minlength=dims[0] * dims[1])
    assert per_row.min() > 16 and (ref["cells"][:, 2] >= 128).any()


def test_sparse_grid_off_origin_and_no_free_cell():
    """403 solid cells in a (96, 72, 80) grid far from the origin, every other cell -5: mostly empty
    tiles.  With free_threshold = -6 no cell is free: {0, solid}."""
    L = RC.grid2()
    gv = Hh.gpu_grid(RC.DIMS2, RC.BOUNDS2)
    ref = _check_all(gv, RC.BOUNDS2, RC.DIMS2, L, 0, -5)
    solid = int((L >= 0).sum())
    assert ref["count"][1] == solid == 403 and 0 < ref["count"][0] <= solid
    none = _check_all(gv, RC.BOUNDS2, RC.DIMS2, L, 0, -6)
    assert none["count"] == (0, solid)


def test_int16_extremes_and_int32_thresholds():
    """-32768 beside 32767 (|g| = 65535) and thresholds at INT32_MIN / INT32_MAX in both roles."""
    dims = (5, 9, 11)
    L = np.zeros(dims, np.int16)
    L[::2, :, :] = 32767
    L[1::2, :, :] = -32768
    L[:, 4, 3:7] = [-32768, 32767, -32768, 32767]
    L[2, 5, :] = np.where(np.arange(11) % 2 == 0, 32767, -32768)
    gv = Hh.gpu_grid(dims, Hh.ODD_BOUNDS)
    ref = _check_all(gv, Hh.ODD_BOUNDS, dims, L, 32767, -32768)
    assert ref["count"][0] > 0 and int(np.abs(ref["g"]).max()) == 65535
    lo, hi = SR.INT32_MIN, SR.INT32_MAX
    n = int(np.prod(dims))
    got = {}
    for occ, free in ((lo, lo), (lo, hi), (hi, lo), (hi, hi), (lo, -32768), (32767, hi)):
        got[occ, free] = _check_all(gv, Hh.ODD_BOUNDS, dims, L, occ, free)["count"]
    assert got[lo, lo] == (0, n) and got[lo, hi] == (n, n) and got[hi, lo] == (0, 0) and got[hi, hi] == (0, 0)
    assert 0 < got[lo, -32768][0] <= n and got[lo, -32768][1] == n
    assert 0 < got[32767, hi][0] == got[32767, hi][1] == int((L == 32767).sum())


def test_capacity_and_null_outputs():
    from dmf_amd import _lib
    thresholds = (1, -1)
    ref = SR.ref1(thresholds)
    m, solid = ref["count"]
    L = RC.grid1()
    gv = Hh.gpu_grid(RC.DIMS1, RC.BOUNDS1)
    dc = Hh.DeviceCalls(gv)
    try:
        d_L = dc.upload(np.ascontiguousarray(L, np.int16).reshape(-1))
        for cap in (m - 1, 0):                       # the prefix, nothing at or past cap, the full count
            cnt, h, xyz, nrm = _device(dc, d_L, *thresholds, cap)
            assert cnt.tolist() == [m, solid]
            _assert_prefix(ref, cap, h, xyz, nrm, what=f"device cap {cap}")
        for k in range(3):                           # each output NULL in turn
            use = tuple(j != k for j in range(3))
            cnt, h, xyz, nrm = _device(dc, d_L, *thresholds, m, use)
            assert cnt.tolist() == [m, solid]
            _assert_prefix(ref, m, h, xyz, nrm, use, what=f"device without output {k}")
            st, n, ns, h, xyz, nrm = _host(gv, L, *thresholds, m, use)
            assert st == _lib.DMF_OK and (n, ns) == (m, solid)
            _assert_prefix(ref, m, h, xyz, nrm, use, what=f"host without output {k}")
    finally:
        dc.close()
    for cap in (m - 1, 0, 1):
        st, n, ns, h, xyz, nrm = _host(gv, L, *thresholds, cap)
        assert st == _lib.DMF_ERR_CAPACITY and (n, ns) == (m, solid), (cap, st, n, ns)
        _assert_prefix(ref, 0, h, xyz, nrm, what=f"host cap {cap}")
    st, n, ns, h, xyz, nrm = _host(gv, L, *thresholds, 0, (False, False, False))   # the size query
    assert st == _lib.DMF_OK and (n, ns) == (m, solid)
    st, n, ns, h, xyz, nrm = _host(gv, L, *thresholds, m - 1, (False, False, False))
    assert st == _lib.DMF_ERR_CAPACITY and n == m
    lo = np.ascontiguousarray(L, np.int16).reshape(-1)
    assert gv._L.dmf_grid_surface(gv._h, lo.ctypes.data, 1, -1, None, None, None, 0, None, None) == _lib.DMF_OK


def test_back_to_back_grids_and_status_rules():
    """Two different grids and threshold pairs through one volume, with a ray-cast of the same
    volume between them: masks, counts and staging buffers are rebuilt by every call."""
    import dmf_amd
    from dmf_amd import _lib
    gv = Hh.gpu_grid(RC.DIMS1, RC.BOUNDS1)
    A = np.asarray(RC.grid1()).reshape(RC.DIMS1)
    B =np.ascontiguousarray(-np.roll(A.astype(np.int32), (5, 3, 7), axis=(0, 1, 2))).astype(np.int16)
    _check_all(gv, RC.BOUNDS1, RC.DIMS1, A, 1, -1, ref=SR.ref1((1, -1)))
    refB = _check_all(gv, RC.BOUNDS1, RC.DIMS1, B, 405, -847)
    assert refB["count"][0] > 1000 and refB["count"] != SR.ref1((1, -1))["count"]
    eng = dmf_amd.RayTracingEngine(dmf_amd.Camera(RC.KA, RC.HA, RC.WA))
    depth, cell = eng.raycast_logodds(gv, A, RC.poses1()[:1], 1, RC.RANGE1)
    assert (cell != dmf_amd.NO_CELL).any() and (depth[cell != dmf_amd.NO_CELL] > 0).all()
    _check_all(gv, RC.BOUNDS1, RC.DIMS1, A, 3511, -2000, ref=SR.ref1((3511, -2000)))
    _check_all(gv, RC.BOUNDS1, RC.DIMS1, A, 1, -1, ref=SR.ref1((1, -1)))
    assert gv.info()["num_occupied"] == 0            # the point-cloud occupancy is not touched
    raw = dmf_amd.VoxelVolume()
    lo = np.zeros(8, np.int16)
    n = C.c_int64()
    assert raw._L.dmf_grid_surface(raw._h, lo.ctypes.data, 1, -1, None, None, None, 0, C.addressof(n),
                                   None) == _lib.DMF_ERR_STATE
    assert raw._L.dmf_volume_integrate_surface(raw._h, lo.ctypes.data, 1, -1, C.addressof(n)) == _lib.DMF_ERR_STATE
    with pytest.raises(ValueError):
        gv.extract_surface(np.zeros(7, np.int16))
    with pytest.raises(ValueError):
        gv.integrate_surface(A.astype(np.int32))


GOOD1 = (372, 285, 0, 0)   # reverseRayTraceFast good lists of raycast_cases.poses1() on the surface of grid1


def _loop_queries(ov, gv, oracle):
    import dmf_amd
    oeng = oracle.Engine(RC.KA, RC.HA, RC.WA)
    eng = dmf_amd.RayTracingEngine(dmf_amd.Camera(RC.KA, RC.HA, RC.WA))
    sizes = []
    for T in RC.poses1():
        f, g = oeng.reverseRayTraceFast(ov, T, True)
        f2, g2 = eng.reverseRayTraceFast(gv, T, True)
        assert f == f2 and np.array_equal(g, g2)
        sizes.append(len(g))
    assert tuple(sizes) == GOOD1
    assert ov.voxel_table()[0].any() and ov.voxel_table()[1].any() and Hh.flags_equal(ov, gv)


def test_the_loop_fused_grid_to_visibility(oracle):
    """integrate_surface on a GPU volume: occupied_cells_ = the reference hashes in order, and
    reverseRayTraceFast gives what the oracle gives on the reference cloud -- found, the good
    lists and every view / good flag.  Then the same through the device composition."""
    from dmf_amd import _lib
    ref = SR.ref1((1, -1))
    m = ref["count"][0]
    L = RC.grid1()
    ov = Hh.oracle_grid(oracle, RC.DIMS1, RC.BOUNDS1, clouds=[(ref["xyz"], ref["normals"])])
    gv = Hh.gpu_grid(RC.DIMS1, RC.BOUNDS1)
    assert gv.integrate_surface(L, 1, -1) == m
    assert np.array_equal(gv.occupied_cells_, ref["hash"])
    assert gv.info()["num_points"] == m
    _loop_queries(ov, gv, oracle)

    ov.reset_flags()
    gd = Hh.gpu_grid(RC.DIMS1, RC.BOUNDS1)
    dc = Hh.DeviceCalls(gd)
    try:
        d_L = dc.upload(np.ascontiguousarray(L, np.int16).reshape(-1))
        cap = m + 5
        dx, dn, dcnt = dc.alloc(12 * cap), dc.alloc(12 * cap), dc.zeros(16)
        _lib.check(dc.L.dmf_grid_surface_device(dc.h, d_L, 1, -1, None, dx, dn, cap, dcnt))
        cnt = dc.download(dcnt, 2, np.uint64)
        assert cnt.tolist() == list(ref["count"]) and cnt[0] <= cap
        _lib.check(dc.L.dmf_volume_integrate_device(dc.h, dx, dn, int(cnt[0])))
    finally:
        dc.close()
    assert np.array_equal(gd.occupied_cells_, ref["hash"])
    _loop_queries(ov, gd, oracle)
