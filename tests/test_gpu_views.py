"""GPU: candidate views (csrc/dmf_views.hip) -- the voxel-grid downsample, the camera
placement and the chain surface -> downsample -> placement -- against tests/views_ref.py, which
tests/test_views.py pins to the tree's host code.  EXACT equality of bit patterns everywhere, through
the host forms, the device forms and the Python methods.  Device outputs are pre-filled with a NaN
pattern that is never a result and carry guard entries after the end; one run has every input and
output shifted by 4 bytes.  The references are computed once per case and shared (views_ref.case)."""
import os
import subprocess

import numpy as np
import pytest

import helpers as Hh
import raycast_cases as RC
import surface_ref as SR
import views_ref as VR

pytestmark = pytest.mark.gpu

FILL = np.uint32(0x7FC00321)               # a NaN no arithmetic makes: no mean, normal or pose word is this
FILL_PTS = np.int32(-77)
FILL_COUNT = np.uint64(0x5A5A5A5A5A5A5A5A)
GUARD = 5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXAMPLE = os.path.join(ROOT, "depth-map-fusion-utils_amd", "build", "views_headless")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _p(a):
    return a.ctypes.data if a is not None and a.size else None


@pytest.fixture(scope="module")
def gv():
    """An UNCONSTRUCTED volume: the downsample and the placement take only its device, stream and scratch."""
    import dmf_amd
    return dmf_amd.VoxelVolume()


def _host_downsample(gv, xyz, nn, leaf, flags, cap, outputs=(True, True, True)):
    n = xyz.shape[0]
    ox = np.full((cap + GUARD) * 3, FILL, np.uint32)
    on = np.full((cap + GUARD) * 3, FILL, np.uint32)
    op = np.full(cap + GUARD, FILL_PTS, np.int32)
    oc = np.full(4, FILL_COUNT, np.uint64)
    st = gv._L.dmf_cloud_downsample(gv._h, _p(xyz), _p(nn), n, leaf.ctypes.data, flags,
                                    ox.ctypes.data if outputs[0] else None,
                                    on.ctypes.data if outputs[1] and nn is not None else None,
                                    op.ctypes.data if outputs[2] else None, cap, oc.ctypes.data)
    return st, ox, on, op, oc


def _device_downsample(dc, xyz, nn, leaf, flags, cap, shift=0):
    from dmf_amd import _lib
    n, k = xyz.shape[0], shift // 4
    pad = np.zeros(k, np.uint32)
    up = lambda a: dc.upload(np.concatenate([pad, _bits(a).reshape(-1)])) + shift      # noqa: E731
    d_x = up(xyz)
    d_n = up(nn) if nn is not None else None
    d_ox = dc.upload(np.full(k + (cap + GUARD) * 3, FILL, np.uint32))
    d_on = dc.upload(np.full(k + (cap + GUARD) * 3, FILL, np.uint32))
    d_op = dc.upload(np.full(k + cap + GUARD, FILL_PTS, np.int32))
    d_c = dc.upload(np.full(4, FILL_COUNT, np.uint64))
    st = dc.L.dmf_cloud_downsample_device(dc.h, d_x if n else None, d_n if n and nn is not None else None, n,
                                          leaf.ctypes.data, flags, d_ox + shift, d_on + shift if nn is not None else None,
                                          d_op + shift, cap, d_c)
    _lib.check(dc.L.dmf_volume_synchronize(dc.h))
    ox = dc.download(d_ox, k + (cap + GUARD) * 3, np.uint32)
    on = dc.download(d_on, k + (cap + GUARD) * 3, np.uint32)
    op = dc.download(d_op, k + cap + GUARD, np.int32)
    assert (ox[:k] == FILL).all() and (on[:k] == FILL).all() and (op[:k] == FILL_PTS).all(), "written before the start"
    return st, ox[k:], on[k:], op[k:], dc.download(d_c, 4, np.uint64)


def _check_outputs(tag, got, want, has_normals, cap):
    """The first min(M, cap) entries equal the reference's, everything after them is untouched, and
    the counts are the whole cloud's."""
    st, ox, on, op, oc = got
    wx, wn, wp, counts = want
    w = min(counts[0], cap)
    assert oc.tolist() == list(counts) + [int(FILL_COUNT)], (tag, oc, counts)
    assert np.array_equal(ox[:3 * w], _bits(wx[:w]).reshape(-1)) and (ox[3 * w:] == FILL).all(), tag + " xyz"
    assert np.array_equal(op[:w], wp[:w]) and (op[w:] == FILL_PTS).all(), tag + " points"
    if has_normals:
        assert np.array_equal(on[:3 * w], _bits(wn[:w]).reshape(-1)) and (on[3 * w:] == FILL).all(), tag + " normals"
    else:
        assert (on == FILL).all(), tag + " normals written without input normals"


def _check_case(gv, name, shift=0, host=True, python=True):
    from dmf_amd import _lib
    xyz, nn, leaf, unit, want = VR.case(name)
    flags = 1 if unit else 0
    m = want[3][0]
    if host:
        got = _host_downsample(gv, xyz, nn, leaf, flags, m)
        assert got[0] == _lib.DMF_OK
        _check_outputs("host", got, want, nn is not None, m)
    dc = Hh.DeviceCalls(gv)
    try:
        got = _device_downsample(dc, xyz, nn, leaf, flags, m, shift)
        assert got[0] == _lib.DMF_OK
        _check_outputs("device", got, want, nn is not None, m)
    finally:
        dc.close()
    if python:
        px, pn, pp = gv.cloud_downsample(xyz, leaf, nn, unit_normals=unit)
        assert px.dtype == np.float32 and px.shape == (m, 3) and pp.dtype == np.int32 and pp.shape == (m,)
        assert np.array_equal(_bits(px), _bits(want[0])) and np.array_equal(pp, want[2])
        assert (pn is None) == (nn is None)
        if nn is not None:
            assert np.array_equal(_bits(pn), _bits(want[1]))


@pytest.mark.parametrize("name", [n for n in VR.CASES if n != "refused"])
def test_named_cases(gv, name):
    """Uniform random points, about 8 per leaf; the boundary lattices k * 0.125f and k * 0.1f with the
    floats on both sides and negative coordinates (floor, not truncation; 4 lattice points of the
    second fall into leaf k - 1 under the float32 product); an anisotropic leaf; 4094 points in one
    leaf near x = 1000, where the order of the float32 adds decides 3 of 6 words, in index order and
    with the members interleaved with other leaves' across the whole index range (stability); a cloud
    near (1000, 2000, 0); rows with NaN / inf coordinates and a NaN normal on a finite point; every
    row non-finite; no point; one point; coincident points; keys above 2^30; no normals; unit normals,
    and a mean normal of exactly zero under them."""
    _check_case(gv, name)


def test_shifted_by_four_bytes(gv):
    """Every input and output 4 bytes off its allocation: no alignment beyond a float's is owed."""
    for name in ("nonfinite_rows", "anisotropic"):
        _check_case(gv, name, shift=4, host=False, python=False)


def test_refused_grid(gv):
    """(0, 0, 0), (0.65, ...), (1.3, ...) with leaf 0.001 would be 2 197 000 000 leaves: the host form
    returns DMF_ERR_RANGE, the device form reports DMF_LEAVES_REFUSED; neither touches an output.  The
    call after it on the same volume is not disturbed."""
    from dmf_amd import _lib
    xyz, nn, leaf, unit, want = VR.case("refused")
    assert want is None
    st, ox, on, op, oc = _host_downsample(gv, xyz, nn, leaf, 0, 3)
    assert st == _lib.DMF_ERR_RANGE
    assert (ox == FILL).all() and (on == FILL).all() and (op == FILL_PTS).all()
    dc = Hh.DeviceCalls(gv)
    try:
        st, ox, on, op, oc = _device_downsample(dc, xyz, nn, leaf, 0, 3)
        assert st == _lib.DMF_OK
        assert oc.tolist() == [VR.REFUSED, 3, 0, int(FILL_COUNT)]
        assert (ox == FILL).all() and (on == FILL).all() and (op == FILL_PTS).all()
    finally:
        dc.close()
    with pytest.raises(_lib.DmfError) as e:
        gv.cloud_downsample(xyz, leaf, nn)
    assert e.value.status == _lib.DMF_ERR_RANGE
    # a bound whose leaf coordinate leaves int32
    far = np.array([[0, 0, 0], [3e9, 0, 0]], np.float32)
    st, ox, on, op, oc = _host_downsample(gv, far, None, VR.leaf3(1.0), 0, 2)
    assert st == _lib.DMF_ERR_RANGE and (ox == FILL).all()
    _check_case(gv, "large_key", python=False)


def test_capacity_and_size_query(gv):
    """cap < M: the device form writes the first cap entries, leaves the guards and reports the true
    count; the host form is DMF_ERR_CAPACITY with the need and untouched outputs; cap = 0 with NULL
    outputs is the size query."""
    from dmf_amd import _lib
    xyz, nn, leaf, unit, want = VR.case("anisotropic")
    m = want[3][0]
    dc = Hh.DeviceCalls(gv)
    try:
        for cap in (m - 1, 257, 1, 0, m + 3):
            got = _device_downsample(dc, xyz, nn, leaf, 0, cap)
            assert got[0] == _lib.DMF_OK
            _check_outputs(f"device cap {cap}", got, want, True, cap)
    finally:
        dc.close()
    st, ox, on, op, oc = _host_downsample(gv, xyz, nn, leaf, 0, m - 1)
    assert st == _lib.DMF_ERR_CAPACITY and int(oc[0]) == m
    assert (ox == FILL).all() and (on == FILL).all() and (op == FILL_PTS).all()
    st, ox, on, op, oc = _host_downsample(gv, xyz, nn, leaf, 0, 0, outputs=(False, False, False))
    assert st == _lib.DMF_OK and oc.tolist() == list(want[3]) + [int(FILL_COUNT)]
    got = _host_downsample(gv, xyz, nn, leaf, 0, m + 3)
    assert got[0] == _lib.DMF_OK
    _check_outputs("host cap m + 3", got, want, True, m + 3)
    # each output alone
    for outs in ((True, False, False), (False, True, False), (False, False, True)):
        st, ox, on, op, oc = _host_downsample(gv, xyz, nn, leaf, 0, m, outputs=outs)
        assert st == _lib.DMF_OK
        assert np.array_equal(ox[:3 * m], _bits(want[0]).reshape(-1)) if outs[0] else (ox == FILL).all()
        assert np.array_equal(on[:3 * m], _bits(want[1]).reshape(-1)) if outs[1] else (on == FILL).all()
        assert np.array_equal(op[:m], want[2]) if outs[2] else (op == FILL_PTS).all()


def test_status_rules(gv):
    from dmf_amd import _lib
    INV, RNG = _lib.DMF_ERR_INVALID, _lib.DMF_ERR_RANGE
    xyz, nn = np.zeros((4, 3), np.float32), np.zeros((4, 3), np.float32)
    leaf = VR.leaf3(0.1)
    ox, on, op = np.full(12, FILL, np.uint32), np.full(12, FILL, np.uint32), np.full(4, FILL_PTS, np.int32)
    oc = np.full(3, FILL_COUNT, np.uint64)
    P = lambda a: a.ctypes.data                                                     # noqa: E731
    outs = (P(ox), P(on), P(op))
    bad_leaves = [np.array(v, np.float32) for v in ((0.1, 0.0, 0.1), (0.1, -0.1, 0.1), (np.nan, 0.1, 0.1), (0.1, 0.1, np.inf))]
    rejected = [
        ((None, P(xyz), P(nn), 4, P(leaf), 0, *outs, 4, P(oc)), INV),
        (("v", None, P(nn), 4, P(leaf), 0, *outs, 4, P(oc)), INV),
        (("v", P(xyz), P(nn), -1, P(leaf), 0, *outs, 4, P(oc)), INV),
        (("v", P(xyz), P(nn), 4, None, 0, *outs, 4, P(oc)), INV),
        (("v", P(xyz), P(nn), 4, P(leaf), 2, *outs, 4, P(oc)), INV),
        (("v", P(xyz), P(nn), 4, P(leaf), 0, *outs, -1, P(oc)), INV),
        (("v", P(xyz), None, 4, P(leaf), 0, *outs, 4, P(oc)), INV),                 # normals asked, none given
        (("v", P(xyz), P(nn), 1 << 31, P(leaf), 0, *outs, 4, P(oc)), RNG),
    ] + [(("v", P(xyz), P(nn), 4, P(b), 0, *outs, 4, P(oc)), INV) for b in bad_leaves]
    for fn in (gv._L.dmf_cloud_downsample, gv._L.dmf_cloud_downsample_device):
        for args, want in rejected:
            args = tuple(gv._h if isinstance(a, str) else a for a in args)
            assert fn(*args) == want, (args, want)
            assert (ox == FILL).all() and (on == FILL).all() and (op == FILL_PTS).all() and (oc == FILL_COUNT).all()
    assert gv._L.dmf_cloud_downsample_device(gv._h, P(xyz), P(nn), 4, P(leaf), 0, *outs, 4, None) == INV
    poses = np.full(48, FILL, np.uint32)
    for fn in (gv._L.dmf_position_cameras, gv._L.dmf_position_cameras_device):
        assert fn(None, P(xyz), P(nn), 4, 300, 0, P(poses)) == INV
        assert fn(gv._h, None, P(nn), 4, 300, 0, P(poses)) == INV
        assert fn(gv._h, P(xyz), None, 4, 300, 0, P(poses)) == INV
        assert fn(gv._h, P(xyz), P(nn), 4, 300, 0, None) == INV
        assert fn(gv._h, P(xyz), P(nn), -1, 300, 0, P(poses)) == INV
        assert fn(gv._h, P(xyz), P(nn), 4, 300, 2, P(poses)) == INV
        assert fn(gv._h, None, None, 0, 300, 0, None) == _lib.DMF_OK
        assert (poses == FILL).all() and not nn.any()
    L = np.zeros(8, np.int16)
    for fn in (gv._L.dmf_grid_surface_views, gv._L.dmf_grid_surface_views_device):
        assert fn(gv._h, None, 1, -1, P(leaf), 0, 300, 0, P(poses), None, None, 4, P(oc)) == INV
        assert fn(gv._h, P(L), 1, -1, P(bad_leaves[0]), 0, 300, 0, P(poses), None, None, 4, P(oc)) == INV
        assert fn(gv._h, P(L), 1, -1, P(leaf), 0, 300, 0, P(poses), None, None, -1, P(oc)) == INV
        assert fn(gv._h, P(L), 1, -1, P(leaf), 2, 300, 0, P(poses), None, None, 4, P(oc)) == INV
        assert fn(gv._h, P(L), 1, -1, P(leaf), 0, 300, 2, P(poses), None, None, 4, P(oc)) == INV
        assert fn(gv._h, P(L), 1, -1, P(leaf), 0, 300, 0, P(poses), None, None, 4, P(oc)) == _lib.DMF_ERR_STATE   # unconstructed
        assert (poses == FILL).all() and (oc == FILL_COUNT).all()


# ---------------------------------------------------------------- placement
def _device_place(dc, xyz, nn, dist, flags, shift=0):
    from dmf_amd import _lib
    m, k = xyz.shape[0], shift // 4
    pad = np.zeros(k, np.uint32)
    d_x = dc.upload(np.concatenate([pad, _bits(xyz).reshape(-1)])) + shift
    d_n = dc.upload(np.concatenate([pad, _bits(nn).reshape(-1), np.full(GUARD * 3, FILL, np.uint32)]))
    d_p = dc.upload(np.full(k + (m + GUARD) * 12, FILL, np.uint32))
    st = dc.L.dmf_position_cameras_device(dc.h, d_x, d_n + shift, m, dist, flags, d_p + shift)
    _lib.check(dc.L.dmf_volume_synchronize(dc.h))
    return st, dc.download(d_p, k + (m + GUARD) * 12, np.uint32)[k:], dc.download(d_n, k + (m + GUARD) * 3, np.uint32)[k:]


@pytest.mark.parametrize("flip", (True, False))
@pytest.mark.parametrize("dist", (0, 100, 300, 600))
def test_placement(gv, dist, flip):
    """Normals with z > 0, z < 0, +0.0, -0.0 and NaN, NaN in x, zero normals of both signs and random
    ones; the poses and the in/out normals, through the host form, the device form (also 4 bytes off)
    and the Python function."""
    import dmf_amd
    from dmf_amd import _lib
    xyz, nn = VR.placement_inputs()
    m = xyz.shape[0]
    wp, wn = VR.position_cameras(xyz, nn, dist, flip)
    flags = 0 if flip else 1
    hn = np.array(nn)
    hp = np.full((m + GUARD) * 12, FILL, np.uint32)
    assert gv._L.dmf_position_cameras(gv._h, xyz.ctypes.data, hn.ctypes.data, m, dist, flags, hp.ctypes.data) == _lib.DMF_OK
    assert np.array_equal(hp[:12 * m], _bits(wp).reshape(-1)) and (hp[12 * m:] == FILL).all()
    assert np.array_equal(_bits(hn), _bits(wn))
    dc = Hh.DeviceCalls(gv)
    try:
        for shift in (0, 4):
            st, dp, dn = _device_place(dc, xyz, nn, dist, flags, shift)
            assert st == _lib.DMF_OK
            assert np.array_equal(dp[:12 * m], _bits(wp).reshape(-1)) and (dp[12 * m:] == FILL).all()
            assert np.array_equal(dn[:3 * m], _bits(wn).reshape(-1)) and (dn[3 * m:] == FILL).all()
    finally:
        dc.close()
    pp, pn = dmf_amd.position_cameras(gv, xyz, nn, dist, flip)
    assert pp.shape == (m, 3, 4) and np.array_equal(_bits(pp), _bits(wp)) and np.array_equal(_bits(pn), _bits(wn))
    if flip:
        with np.errstate(invalid="ignore"):
            assert not (wn[:, 2] < 0).any()
        # a zero z flips with the rest, whatever its sign: +0.0 -> -0.0 and -0.0 -> +0.0
        assert _bits(wn[2:4, 2]).tolist() == [0x80000000, 0]
    else:
        assert np.array_equal(_bits(wn), _bits(nn))


# ---------------------------------------------------------------- the chain
CH_DIMS, CH_BOUNDS = (24, 20, 18), Hh.ODD_BOUNDS


def _ball_on_slab():
    """A synthetic fused grid: free space (-3), a solid slab (4) at the bottom and a solid ball on it,
    with an unobserved (0) corner -- surfaces facing up, sideways and (the ball's underside) down."""
    x, y, z = np.meshgrid(*(np.arange(d) for d in CH_DIMS), indexing="ij")
    L = np.full(CH_DIMS, -3, np.int16)
    L[z < 3] = 4
    L[(x - 11.5) ** 2 + (y - 9.5) ** 2 + (z - 9.0) ** 2 <= 5.2 ** 2] = 6
    L[18:, 15:, 12:] = 0
    return L


@pytest.fixture(scope="module")
def chain():
    gvc = Hh.gpu_grid(CH_DIMS, CH_BOUNDS)
    L = _ball_on_slab()
    h, sx, sn = gvc.extract_surface(L)
    ref = SR.surface(CH_BOUNDS, CH_DIMS, L, 1, -1)
    assert np.array_equal(_bits(sx), _bits(ref["xyz"])) and np.array_equal(_bits(sn), _bits(ref["normals"]))
    d = [(CH_BOUNDS[2 * a + 1] - CH_BOUNDS[2 * a]) / CH_DIMS[a] for a in range(3)]
    leaf = VR.leaf3([3.3 * d[0], 3.3 * d[1], 3.3 * d[2]])       # 3.3 cells: off the cell lattice
    return gvc, L, sx, sn, leaf, ref["count"]


@pytest.mark.parametrize("unit", (False, True))
@pytest.mark.parametrize("flip", (True, False))
def test_chain(chain, flip, unit):
    """surface_views == extract_surface -> views_ref.downsample -> views_ref.position_cameras, through
    the host form (the Python method) and the device form with a capacity below the count; the
    counts; and the poses are accepted by view_gain on the same grid."""
    import dmf_amd
    from dmf_amd import _lib
    gvc, L, sx, sn, leaf, scount = chain
    assert (sn[:, 2] < 0).any() and (sn[:, 2] > 0).any()
    lx, ln, _, counts = VR.downsample(sx, leaf, sn, unit)
    wp, wn = VR.position_cameras(lx, ln, 250, flip)
    m = counts[0]
    assert 10 < m < sx.shape[0]
    poses, xyz, nrm = gvc.surface_views(L, leaf, distance_mm=250, unit_normals=unit, flip=flip)
    assert poses.shape == (m, 3, 4)
    assert np.array_equal(_bits(xyz), _bits(lx)) and np.array_equal(_bits(nrm), _bits(wn)) and np.array_equal(_bits(poses), _bits(wp))
    dc = Hh.DeviceCalls(gvc)
    try:
        d_L = dc.upload(L.reshape(-1))
        for cap in (m + 2, m - 3):
            w = min(m, cap)
            d_p = dc.upload(np.full((cap + GUARD) * 12, FILL, np.uint32))
            d_x = dc.upload(np.full((cap + GUARD) * 3, FILL, np.uint32))
            d_n = dc.upload(np.full((cap + GUARD) * 3, FILL, np.uint32))
            d_c = dc.upload(np.full(4, FILL_COUNT, np.uint64))
            st = dc.L.dmf_grid_surface_views_device(dc.h, d_L, 1, -1, leaf.ctypes.data, 1 if unit else 0, 250, 0 if flip else 1,
                                                    d_p, d_x, d_n, cap, d_c)
            assert st == _lib.DMF_OK
            _lib.check(dc.L.dmf_volume_synchronize(dc.h))
            gp, gx, gn = (dc.download(d, (cap + GUARD) * k, np.uint32) for d, k in ((d_p, 12), (d_x, 3), (d_n, 3)))
            assert dc.download(d_c, 4, np.uint64).tolist() == [m, scount[0], scount[1], int(FILL_COUNT)]
            assert np.array_equal(gp[:12 * w], _bits(wp[:w]).reshape(-1)) and (gp[12 * w:] == FILL).all()
            assert np.array_equal(gx[:3 * w], _bits(lx[:w]).reshape(-1)) and (gx[3 * w:] == FILL).all()
            assert np.array_equal(gn[:3 * w], _bits(wn[:w]).reshape(-1)) and (gn[3 * w:] == FILL).all()
        # poses alone: the locations stay in scratch
        d_p = dc.upload(np.full((m + GUARD) * 12, FILL, np.uint32))
        d_c = dc.upload(np.full(4, FILL_COUNT, np.uint64))
        assert dc.L.dmf_grid_surface_views_device(dc.h, d_L, 1, -1, leaf.ctypes.data, 1 if unit else 0, 250, 0 if flip else 1,
                                                  d_p, None, None, m, d_c) == _lib.DMF_OK
        _lib.check(dc.L.dmf_volume_synchronize(dc.h))
        gp = dc.download(d_p, (m + GUARD) * 12, np.uint32)
        assert np.array_equal(gp[:12 * m], _bits(wp).reshape(-1)) and (gp[12 * m:] == FILL).all()
    finally:
        dc.close()
    # host form: capacity and size query
    oc = np.full(4, FILL_COUNT, np.uint64)
    hp = np.full(12 * m, FILL, np.uint32)
    args = (gvc._h, L.ctypes.data, 1, -1, leaf.ctypes.data, 1 if unit else 0, 250, 0 if flip else 1)
    assert gvc._L.dmf_grid_surface_views(*args, hp.ctypes.data, None, None, m - 1, oc.ctypes.data) == _lib.DMF_ERR_CAPACITY
    assert int(oc[0]) == m and (hp == FILL).all()
    assert gvc._L.dmf_grid_surface_views(*args, None, None, None, 0, oc.ctypes.data) == _lib.DMF_OK
    assert oc.tolist() == [m, scount[0], scount[1], int(FILL_COUNT)]
    if flip and not unit:
        eng = dmf_amd.RayTracingEngine(dmf_amd.Camera(RC.KA, RC.HA, RC.WA))
        gain = eng.view_gain(gvc, L, poses)
        assert gain.shape == (m,) and gain.dtype == np.uint64


def test_chain_empty_and_refused(chain):
    """A grid with no surface gives no view; a leaf too small for the surface's box is refused."""
    from dmf_amd import _lib
    gvc, L, sx, sn, leaf, scount = chain
    poses, xyz, nrm = gvc.surface_views(np.zeros(CH_DIMS, np.int16), leaf)
    assert poses.shape == (0, 3, 4) and xyz.shape == (0, 3) and nrm.shape == (0, 3)
    with pytest.raises(_lib.DmfError) as e:
        gvc.surface_views(L, 1e-4)
    assert e.value.status == _lib.DMF_ERR_RANGE
    dc = Hh.DeviceCalls(gvc)
    try:
        d_L = dc.upload(L.reshape(-1))
        d_p = dc.upload(np.full(120, FILL, np.uint32))
        d_c = dc.upload(np.full(4, FILL_COUNT, np.uint64))
        tiny = VR.leaf3(1e-4)
        assert dc.L.dmf_grid_surface_views_device(dc.h, d_L, 1, -1, tiny.ctypes.data, 0, 300, 0, d_p, None, None, 10,
                                                  d_c) == _lib.DMF_OK
        _lib.check(dc.L.dmf_volume_synchronize(dc.h))
        assert dc.download(d_c, 4, np.uint64).tolist() == [VR.REFUSED, scount[0], scount[1], int(FILL_COUNT)]
        assert (dc.download(d_p, 120, np.uint32) == FILL).all()
    finally:
        dc.close()


def test_example_binary():
    """build/views_headless on its synthetic cloud: the host route and the device route agree bit for bit."""
    res = subprocess.run([EXAMPLE, "--synthetic", "6000", "5", "0.1", "300"], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout + res.stderr
    lines = res.stdout.splitlines()
    assert "bitwise equal" in lines, res.stdout
    views = [ln for ln in lines if ln.startswith("views ")][0].split()
    assert views[2] == views[4] and int(views[2]) > 100
