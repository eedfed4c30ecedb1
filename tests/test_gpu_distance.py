"""GPU: the distance field and the segment clearance (csrc/dmf_distance.hip) against
the numpy restatement tests/distance_ref.py -- exact equality on every cell and every segment, through
the host form, the device form and the Python method.  Device outputs are pre-filled with a value
that is never a result and carry guard entries after the end (an unwritten or overwritten entry
shows)."""
import ctypes as C

import numpy as np
import pytest

import distance_ref as DR
import fuse_points_ref as FP
import helpers as Hh

pytestmark = pytest.mark.gpu

FILL = np.uint32(0xFFFFFFFE)              # neither a squared distance (< 2^24) nor DMF_NO_DIST
FILL_COUNT = np.uint64(1 << 63)
GUARD = 5                                  # entries kept after the end


def _host(gv, L, threshold):
    """dmf_grid_distance -> (status, n_solid, dist2 flat)."""
    lo = np.ascontiguousarray(L, np.int16).reshape(-1)
    out = np.full(lo.size, FILL, np.uint32)
    ns = C.c_int64(-1)
    st = gv._L.dmf_grid_distance(gv._h, lo.ctypes.data, int(threshold), out.ctypes.data, C.addressof(ns))
    return st, ns.value, out


def _device(dc, d_L, ncell, threshold, count=True):
    """dmf_grid_distance_device into a pre-filled output of ncell + GUARD entries -> (count, dist2 with guard)."""
    from dmf_amd import _lib
    d_out = dc.upload(np.full(ncell + GUARD, FILL, np.uint32))
    d_cnt = dc.upload(np.full(2, FILL_COUNT, np.uint64))
    _lib.check(dc.L.dmf_grid_distance_device(dc.h, d_L, int(threshold), d_out, d_cnt if count else None))
    return dc.download(d_cnt, 2, np.uint64), dc.download(d_out, ncell + GUARD, np.uint32), d_out


def _check_all(gv, dims, L, threshold, ref):
    """Host form, device form and the Python method == the reference, on every cell."""
    from dmf_amd import _lib
    n = int(np.prod(dims))
    want, solid = ref.reshape(-1), int((ref == 0).sum())
    st, ns, out = _host(gv, L, threshold)
    assert st == _lib.DMF_OK and ns == solid, (st, ns, solid)
    assert int((out != want).sum()) == 0, "host"
    dc = Hh.DeviceCalls(gv)
    try:
        d_L = dc.upload(np.ascontiguousarray(L, np.int16).reshape(-1))
        cnt, out, _ = _device(dc, d_L, n, threshold)
        assert cnt.tolist() == [solid, int(FILL_COUNT)], (cnt, solid)     # one counter, not two
        assert int((out[:n] != want).sum()) == 0 and (out[n:] == FILL).all(), "device"
        cnt, out, _ = _device(dc, d_L, n, threshold, count=False)
        assert (cnt == FILL_COUNT).all() and np.array_equal(out[:n], want) and (out[n:] == FILL).all()
    finally:
        dc.close()
    got = gv.distance_field(np.asarray(L, np.int16).reshape(dims), threshold)
    assert got.dtype == np.uint32 and got.shape == tuple(dims) and np.array_equal(got, ref)


@pytest.mark.parametrize("name", sorted(DR.CASES))
def test_named_cases(name):
    """The fused scene on an odd grid at four thresholds (none solid: all DMF_NO_DIST; all solid: all
    0), random sparse grids down to one cell and with one long axis, a single site in either far
    corner (distances across the whole diagonal), sites only in the plane x = 0 (every z and y
    column beyond it infinite until the last pass), two sites at the ends of one x column, the
    ABI's longest axis (d^2 up to 2047^2), and an x column whose envelope grows 40 entries deep
    before one site pops 29 of them (entries read back from the stack, far below its top)."""
    dims, L, threshold, ref = DR.case(name)
    assert DR.totals(ref, L, dims, threshold) == DR.TOTALS[name]
    _check_all(Hh.gpu_grid(dims, Hh.ODD_BOUNDS), dims, L, threshold, ref)


def test_status_rules_and_python_validation():
    import dmf_amd
    from dmf_amd import _lib
    big = Hh.gpu_grid((2049, 1, 1), Hh.ODD_BOUNDS)
    lo, out = np.zeros(2049, np.int16), np.full(2049, FILL, np.uint32)
    a = np.zeros((1, 3), np.float32)
    cl = np.full(1, FILL, np.uint32)
    assert big._L.dmf_grid_distance(big._h, lo.ctypes.data, 1, out.ctypes.data, None) == _lib.DMF_ERR_RANGE
    assert big._L.dmf_grid_clearance(big._h, out.ctypes.data, a.ctypes.data, a.ctypes.data, 1,
                                     cl.ctypes.data) == _lib.DMF_ERR_RANGE
    raw = dmf_amd.VoxelVolume()
    assert raw._L.dmf_grid_distance(raw._h, lo.ctypes.data, 1, out.ctypes.data, None) == _lib.DMF_ERR_STATE
    assert raw._L.dmf_grid_distance_device(raw._h, lo.ctypes.data, 1, out.ctypes.data, None) == _lib.DMF_ERR_STATE
    assert raw._L.dmf_grid_clearance(raw._h, out.ctypes.data, a.ctypes.data, a.ctypes.data, 1,
                                     cl.ctypes.data) == _lib.DMF_ERR_STATE
    assert raw._L.dmf_grid_clearance(raw._h, out.ctypes.data, a.ctypes.data, a.ctypes.data, 0,
                                     cl.ctypes.data) == _lib.DMF_OK
    assert (out == FILL).all() and (cl == FILL).all()
    gv = Hh.gpu_grid((9, 8, 7), Hh.ODD_BOUNDS)
    d2 = gv.distance_field(np.zeros((9, 8, 7), np.int16), 0)
    assert (d2 == 0).all()
    with pytest.raises(ValueError):
        gv.distance_field(np.zeros(7, np.int16))
    with pytest.raises(ValueError):
        gv.distance_field(np.zeros((9, 8, 7), np.int32))
    with pytest.raises(ValueError):
        gv.segment_clearance(d2.astype(np.int32), a, a)
    with pytest.raises(ValueError):
        gv.segment_clearance(d2.reshape(-1)[:-1], a, a)
    with pytest.raises(ValueError):
        gv.segment_clearance(d2, np.zeros((2, 3), np.float32), np.zeros((3, 3), np.float32))
    with pytest.raises(ValueError):
        gv.segment_clearance(d2, np.zeros((2, 2), np.float32), np.zeros((2, 2), np.float32))
    one = gv.segment_clearance(d2, np.zeros(3, np.float32), np.full(3, 0.1, np.float32))
    assert one.shape == (1,) and one.dtype == np.uint32 and one[0] == 0
    assert gv.segment_clearance(d2, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32)).shape == (0,)


def test_two_device_calls_dense_then_sparse():
    """One volume, one output buffer: every cell solid (threshold -32768), then 195 solid cells
    (3511), then none.  The envelope stacks and the counter of the first call must not leak into
    the later ones, and the point-cloud occupancy stays untouched."""
    from dmf_amd import _lib
    dims, L, _, _ = DR.case("grid1_t1")
    n = int(np.prod(dims))
    gv = Hh.gpu_grid(dims, Hh.ODD_BOUNDS)
    dc = Hh.DeviceCalls(gv)
    try:
        d_L = dc.upload(np.ascontiguousarray(L, np.int16).reshape(-1))
        d_out = dc.upload(np.full(n + GUARD, FILL, np.uint32))
        d_cnt = dc.upload(np.full(2, FILL_COUNT, np.uint64))
        for name in ("grid1_all", "grid1_t3511", "grid1_none", "grid1_t1"):
            _, _, threshold, ref = DR.case(name)
            _lib.check(dc.L.dmf_grid_distance_device(dc.h, d_L, threshold, d_out, d_cnt))
            out, cnt = dc.download(d_out, n + GUARD, np.uint32), dc.download(d_cnt, 2, np.uint64)
            assert cnt.tolist() == [DR.TOTALS[name][2], int(FILL_COUNT)], name
            assert np.array_equal(out[:n], ref.reshape(-1)) and (out[n:] == FILL).all(), name
    finally:
        dc.close()
    assert gv.info()["num_occupied"] == 0


# ---------------------------------------------------------------- clearance
def _seg_volume():
    return Hh.gpu_grid(FP.SEG_DIMS, FP.SEG_BOUNDS)


def test_clearance_segments_host_device_python():
    """Every segment of fuse_points_ref.segment_case() (anisotropic cells; NaN, inf, a == b,
    axis-parallel, exactly diagonal and off-grid segments) over the GPU's own distance field of a
    2 % solid grid: clear2 == the restatement, DMF_NO_DIST exactly where it has no cell."""
    from dmf_amd import _lib
    ref_d2, ref_c2 = DR.segment_reference()
    a, b = DR.segments()
    m, n = a.shape[0], int(np.prod(FP.SEG_DIMS))
    gv = _seg_volume()
    d2 = gv.distance_field(DR.segment_grid(), 1)
    assert np.array_equal(d2, ref_d2)
    got = gv.segment_clearance(d2, a, b)
    assert got.dtype == np.uint32 and got.shape == (m,)
    assert int((got != ref_c2).sum()) == 0
    assert np.array_equal(got == DR.NO_DIST, ref_c2 == DR.NO_DIST) and 0 < int((got == DR.NO_DIST).sum()) < m
    out = np.full(m + GUARD, FILL, np.uint32)
    flat = np.ascontiguousarray(d2).reshape(-1)
    _lib.check(gv._L.dmf_grid_clearance(gv._h, flat.ctypes.data, a.ctypes.data, b.ctypes.data, m, out.ctypes.data))
    assert np.array_equal(out[:m], ref_c2) and (out[m:] == FILL).all()
    dc = Hh.DeviceCalls(gv)
    try:
        d_L = dc.upload(DR.segment_grid().reshape(-1))
        d_d2 = dc.upload(np.full(n, FILL, np.uint32))
        _lib.check(dc.L.dmf_grid_distance_device(dc.h, d_L, 1, d_d2, None))
        d_a, d_b, d_c = dc.upload(a), dc.upload(b), dc.upload(np.full(m + GUARD, FILL, np.uint32))
        _lib.check(dc.L.dmf_grid_clearance_device(dc.h, d_d2, d_a, d_b, m, d_c))
        out = dc.download(d_c, m + GUARD, np.uint32)
        assert np.array_equal(out[:m], ref_c2) and (out[m:] == FILL).all()
        _lib.check(dc.L.dmf_grid_clearance_device(dc.h, d_d2, d_a, d_b, 0, d_c))      # n = 0: nothing written
        assert np.array_equal(dc.download(d_c, m + GUARD, np.uint32), out)
    finally:
        dc.close()


def test_clearance_is_the_fusions_own_walk():
    """32 of the segments, each fused alone with fuse_points (S = 1, N = 1): the cells whose hit or
    miss counter changed are the walk, and the minimum of dist2 over them is clear2."""
    import dmf_amd
    ref_d2, ref_c2 = DR.segment_reference()
    a, b = DR.segments()
    with_cells = np.flatnonzero(ref_c2 != DR.NO_DIST)
    none = np.flatnonzero(ref_c2 == DR.NO_DIST)
    # the forced cases of both scans that have cells, segments without one, and a spread of the rest
    forced = [i for s in range(2) for i in range(s * FP.SEG_N, s * FP.SEG_N + 31) if ref_c2[i] != DR.NO_DIST]
    pick = []
    for i in forced[::3] + none[:4].tolist() + with_cells[40::45].tolist():
        if int(i) not in pick:
            pick.append(int(i))
    pick = pick[:32]
    assert len(pick) == 32 and len(forced) >= 16
    gv = _seg_volume()
    got = gv.segment_clearance(ref_d2, a[pick], b[pick])
    eng = dmf_amd.RayTracingEngine(dmf_amd.Camera(Hh.KA, *Hh.KA_WH[::-1]))
    flat = ref_d2.reshape(-1)
    for k, i in enumerate(pick):
        h, m, _ = eng.fuse_points(gv, b[i].reshape(1, 1, 3), a[i].reshape(1, 3))
        walk = np.flatnonzero((np.asarray(h).reshape(-1) != 0) | (np.asarray(m).reshape(-1) != 0))
        want = int(flat[walk].min()) if walk.size else DR.NO_DIST
        assert int(got[k]) == want == int(ref_c2[i]), (i, int(got[k]), want, int(ref_c2[i]))
