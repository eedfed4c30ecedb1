"""GPU: the exact cloud nearest neighbour and the cloud error (csrc/dmf_cloud.hip) against
the brute-force restatement tests/cloud_ref.py -- EXACT equality of dist2 (as bit patterns) and of index
on every query, through the host form, the device form and the Python method.  Device outputs are
pre-filled with values that are never results and carry guard entries after the end (an unwritten or
overwritten entry shows).  The references are computed once per case and shared (cloud_ref.case)."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import cloud_ref as CR
import helpers as Hh

pytestmark = pytest.mark.gpu

FILL_D2 = np.uint32(0x7FC00123)            # a NaN: no dist2 is one
FILL_IDX = np.int32(-77)
FILL_COUNT = np.uint64(1 << 63)
FILL_SUM = -12345.5
GUARD = 5
THR = (0.003, 0.005)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXAMPLE = os.path.join(ROOT, "depth-map-fusion-utils_amd", "build", "cloud_error_headless")


def _p(a):
    return a.ctypes.data if a is not None and a.size else None


def _host(gv, q, r, thr=THR, d2=True, idx=True, counts=True, sums=True):
    """dmf_cloud_nearest into pre-filled outputs with guards -> (status, dist2 bits, index, counts, sums)."""
    n, T = q.shape[0], len(thr)
    od = np.full(n + GUARD, FILL_D2, np.uint32)
    oi = np.full(n + GUARD, FILL_IDX, np.int32)
    oc = np.full(2 + T + 1, FILL_COUNT, np.uint64)
    os_ = np.full(3, FILL_SUM, np.float64)
    t = np.asarray(thr, np.float64)
    st = gv._L.dmf_cloud_nearest(gv._h, _p(q), n, _p(r), r.shape[0], od.ctypes.data if d2 else None,
                                 oi.ctypes.data if idx else None, _p(t), T, oc.ctypes.data if counts else None,
                                 os_.ctypes.data if sums else None)
    return st, od, oi, oc, os_


def _device(dc, q, r, thr=THR, d2=True, idx=True, counts=True, sums=True, bufs=None, shift=0):
    """dmf_cloud_nearest_device likewise; `shift` bytes are put in front of both inputs and both
    per-point outputs; `bufs` reuses (d_d2, d_idx, d_counts, d_sums, entries) of an earlier call."""
    from dmf_amd import _lib
    n, T = q.shape[0], len(thr)
    pad = np.zeros(shift // 4, np.float32)
    d_q = dc.upload(np.concatenate([pad, q.reshape(-1)])) + shift
    d_r = dc.upload(np.concatenate([pad, r.reshape(-1)])) + shift
    k = shift // 4
    if bufs is None:
        cap = n
        bufs = (dc.upload(np.full(k + cap + GUARD, FILL_D2, np.uint32)), dc.upload(np.full(k + cap + GUARD, FILL_IDX, np.int32)),
                dc.upload(np.full(2 + T + 1, FILL_COUNT, np.uint64)), dc.upload(np.full(3, FILL_SUM, np.float64)), cap)
    d_d2, d_idx, d_c, d_s, cap = bufs
    t = np.asarray(thr, np.float64)
    st = dc.L.dmf_cloud_nearest_device(dc.h, d_q if n else None, n, d_r if r.shape[0] else None, r.shape[0],
                                       d_d2 + shift if d2 else None, d_idx + shift if idx else None, _p(t), T,
                                       d_c if counts else None, d_s if sums else None)
    _lib.check(dc.L.dmf_volume_synchronize(dc.h))
    return (st, dc.download(d_d2, k + cap + GUARD, np.uint32), dc.download(d_idx, k + cap + GUARD, np.int32),
            dc.download(d_c, 2 + T + 1, np.uint64), dc.download(d_s, 3, np.float64), bufs)


def _want_summary(d2, idx, r, thr=THR):
    counts, mx, total, avg = CR.summaries(d2, idx, r, thr)
    return counts, mx, total, avg


def _check_summary(oc, os_, want, n, thr=THR):
    """counts and the max exact; the sum against fsum with relative tolerance n * 2^-53 (each of the
    n - 1 additions of non-negative doubles errs by at most half an ulp of a partial sum that never
    exceeds the total)."""
    counts, mx, total, _ = want
    assert oc.tolist() == counts + [int(FILL_COUNT)], (oc, counts)
    assert os_[0] == mx and os_[2] == FILL_SUM, (os_, mx)
    assert abs(os_[1] - total) <= max(n, 1) * 2.0 ** -53 * total, (os_[1], total)


def _check_all(gv, q, r, wd, wi, thr=THR):
    from dmf_amd import _lib
    n = q.shape[0]
    want = _want_summary(wd, wi, r, thr)
    wb = wd.view(np.uint32)
    st, od, oi, oc, os_ = _host(gv, q, r, thr)
    assert st == _lib.DMF_OK
    assert int((od[:n] != wb).sum()) == 0 and (od[n:] == FILL_D2).all(), "host dist2"
    assert int((oi[:n] != wi).sum()) == 0 and (oi[n:] == FILL_IDX).all(), "host index"
    _check_summary(oc, os_, want, n, thr)
    dc = Hh.DeviceCalls(gv)
    try:
        st, od, oi, oc, os_, _ = _device(dc, q, r, thr)
        assert st == _lib.DMF_OK
        assert int((od[:n] != wb).sum()) == 0 and (od[n:] == FILL_D2).all(), "device dist2"
        assert int((oi[:n] != wi).sum()) == 0 and (oi[n:] == FILL_IDX).all(), "device index"
        _check_summary(oc, os_, want, n, thr)
    finally:
        dc.close()
    gd, gi = gv.cloud_nearest(q, r)
    assert gd.dtype == np.float32 and gi.dtype == np.int32 and gd.shape == gi.shape == (n,)
    assert np.array_equal(gd.view(np.uint32), wb) and np.array_equal(gi, wi)
    e = gv.cloud_error(q, r, thr)
    assert e.n_valid == want[0][0] and e.max_error == want[1] and e.over == tuple(want[0][2:])
    assert e.avg_error == want[3] or (math.isnan(e.avg_error) and math.isnan(want[3]))     # bit for bit
    assert np.array_equal(e.dist2.view(np.uint32), wb)


@pytest.fixture(scope="module")
def gv():
    return Hh.gpu_grid((9, 8, 7), Hh.ODD_BOUNDS)


@pytest.mark.parametrize("name", sorted(CR.CASES))
def test_named_cases(gv, name):
    """Uniform random points; a lattice followed by itself reversed with queries at the centres of its
    cubes (4 to 16 tied minimisers: the lowest index wins); a cloud against itself with duplicates;
    the random and lattice cases far from the origin, where a float's spacing reaches 1e-4; points and
    queries on, one float below and one float above lattice coordinates that cell boundaries fall on;
    planar, linear, one-point and coincident references and a blob with an outlier 10 m away; queries
    ten box lengths outside on every face, edge and corner; NaN and +-inf rows on both sides, an
    all-invalid and an empty reference, no query; and sizes around the wave."""
    q, r, wd, wi = CR.case(name)
    _check_all(gv, q, r, wd, wi)
    if name == "outside":
        assert np.array_equal(gv.cloud_nearest(q, r)[1], CR.outside_closed_form(q))
    if name in CR.TIE_CASES:
        assert (gv.cloud_nearest(q, r)[1] < 4913).all()


@pytest.mark.parametrize("variant", [(8, 1), (16, 2), (4, 1), (1, 2), (0, 1)])
@pytest.mark.parametrize("name", ["ties", "far_uniform_1", "outlier", "invalid_rows", "outside"])
def test_every_index_shape_and_query_order_gives_the_same_bytes(name, variant):
    """The A/B controls of DESIGN.md §5.17 (the target occupancy of a cell; the queries in the order
    given or sorted by home cell first) change the work, never a result."""
    from dmf_amd import _lib
    v = Hh.gpu_grid((9, 8, 7), Hh.ODD_BOUNDS)
    _lib.cloud_variant(v, *variant)
    q, r, wd, wi = CR.case(name)
    _check_all(v, q, r, wd, wi)


@pytest.mark.parametrize("name", ["uniform", "small_65_65", "invalid_rows"])
def test_unaligned_pointers(gv, name):
    """Both inputs and both per-point outputs at a base + 4 bytes: no caller owes more than 4-byte
    alignment; the entry before each output and the guards after stay as they were."""
    from dmf_amd import _lib
    q, r, wd, wi = CR.case(name)
    n = q.shape[0]
    dc = Hh.DeviceCalls(gv)
    try:
        st, od, oi, oc, os_, _ = _device(dc, q, r, shift=4)
        assert st == _lib.DMF_OK
        assert od[0] == FILL_D2 and np.array_equal(od[1:1 + n], wd.view(np.uint32)) and (od[1 + n:] == FILL_D2).all()
        assert oi[0] == FILL_IDX and np.array_equal(oi[1:1 + n], wi) and (oi[1 + n:] == FILL_IDX).all()
        _check_summary(oc, os_, _want_summary(wd, wi, r), n)
    finally:
        dc.close()
    # the host form from odd host addresses
    qb, rb = np.zeros(q.size + 1, np.float32), np.zeros(r.size + 1, np.float32)
    qb[1:], rb[1:] = q.reshape(-1), r.reshape(-1)
    od, oi = np.full(n + 2, FILL_D2, np.uint32), np.full(n + 2, FILL_IDX, np.int32)
    st = gv._L.dmf_cloud_nearest(gv._h, qb.ctypes.data + 4, n, rb.ctypes.data + 4, r.shape[0], od.ctypes.data + 4,
                                 oi.ctypes.data + 4, None, 0, None, None)
    assert st == _lib.DMF_OK and od[0] == FILL_D2 and od[-1] == FILL_D2 and oi[0] == FILL_IDX and oi[-1] == FILL_IDX
    assert np.array_equal(od[1:-1], wd.view(np.uint32)) and np.array_equal(oi[1:-1], wi)


def test_each_optional_output_null_in_turn(gv):
    from dmf_amd import _lib
    q, r, wd, wi = CR.case("invalid_rows")
    n = q.shape[0]
    want = _want_summary(wd, wi, r)
    dc = Hh.DeviceCalls(gv)
    try:
        for drop in ("d2", "idx", "counts", "sums", ("d2", "idx"), ("counts", "sums"), ("d2", "idx", "counts"),
                     ("d2", "idx", "sums")):
            keep = {k: k not in (drop if isinstance(drop, tuple) else (drop,)) for k in ("d2", "idx", "counts", "sums")}
            for form in ("host", "device"):
                if form == "host":
                    st, od, oi, oc, os_ = _host(gv, q, r, **keep)
                else:
                    st, od, oi, oc, os_, _ = _device(dc, q, r, **keep)
                assert st == _lib.DMF_OK, (drop, form)
                assert np.array_equal(od[:n], wd.view(np.uint32)) if keep["d2"] else (od == FILL_D2).all(), (drop, form)
                assert np.array_equal(oi[:n], wi) if keep["idx"] else (oi == FILL_IDX).all(), (drop, form)
                assert (od[n:] == FILL_D2).all() and (oi[n:] == FILL_IDX).all()
                assert oc.tolist() == want[0] + [int(FILL_COUNT)] if keep["counts"] else (oc == FILL_COUNT).all(), (drop, form)
                if keep["sums"]:
                    assert os_[0] == want[1] and abs(os_[1] - want[2]) <= n * 2.0 ** -53 * want[2] and os_[2] == FILL_SUM
                else:
                    assert (os_ == FILL_SUM).all()
    finally:
        dc.close()


def test_thresholds_zero_to_eight(gv):
    q, r, wd, wi = CR.case("uniform")
    dist = np.sqrt(wd).astype(np.float64)
    for thr in ((), (0.0,), tuple(float(np.quantile(dist, k / 9)) for k in range(1, 9)), (float(dist.max()), float(dist[5]), 1e30)):
        st, od, oi, oc, os_ = _host(gv, q, r, thr)
        assert st == 0
        _check_summary(oc, os_, _want_summary(wd, wi, r, thr), q.shape[0], thr)
        assert gv.cloud_error(q, r, thr).over == tuple(int((dist > t).sum()) for t in thr)


def test_calls_share_one_volume_and_one_set_of_outputs():
    """One volume, one set of output buffers: a large call, a small one, an empty reference, the large
    one again.  Nothing of an earlier call's index, records or sums may show, the first and the last
    call give the same bytes, the point-cloud occupancy stays untouched, and a raw, unconstructed
    VoxelVolume gives the same results."""
    import dmf_amd
    from dmf_amd import _lib
    order = ("uniform", "small_65_2", "empty_ref", "self", "uniform")
    cap = max(CR.case(name)[0].shape[0] for name in order)
    seen = {}
    for vol in (Hh.gpu_grid((9, 8, 7), Hh.ODD_BOUNDS), dmf_amd.VoxelVolume()):
        dc = Hh.DeviceCalls(vol)
        try:
            bufs = (dc.upload(np.full(cap + GUARD, FILL_D2, np.uint32)), dc.upload(np.full(cap + GUARD, FILL_IDX, np.int32)),
                    dc.upload(np.full(5, FILL_COUNT, np.uint64)), dc.upload(np.full(3, FILL_SUM, np.float64)), cap)
            first = None
            for name in order:
                q, r, wd, wi = CR.case(name)
                n = q.shape[0]
                st, od, oi, oc, os_, _ = _device(dc, q, r, bufs=bufs)
                assert st == _lib.DMF_OK, name
                assert np.array_equal(od[:n], wd.view(np.uint32)) and np.array_equal(oi[:n], wi), name
                assert (od[cap:] == FILL_D2).all() and (oi[cap:] == FILL_IDX).all(), name
                _check_summary(oc, os_, _want_summary(wd, wi, r), n)
                if name == "uniform":
                    got = od[:n].tobytes() + oi[:n].tobytes() + oc.tobytes() + os_[:1].tobytes()
                    assert first is None or first == got
                    first = got
                seen.setdefault(name, (od[:n].tobytes(), oi[:n].tobytes()))
                assert seen[name] == (od[:n].tobytes(), oi[:n].tobytes()), name
        finally:
            dc.close()
        info = vol.info()
        assert info["num_occupied"] == 0 and info["num_points"] == 0
    assert vol.info()["constructed"] == 0
    gd, gi = vol.cloud_nearest(*CR.case("ties")[:2])                      # the raw volume, through Python
    assert np.array_equal(gd.view(np.uint32), CR.case("ties")[2].view(np.uint32)) and np.array_equal(gi, CR.case("ties")[3])


@pytest.fixture(scope="module")
def fused():
    """The smoke scene: two frames fused into 64^3 cells, finalized."""
    import dmf_amd
    poses, depth, _ = Hh.frames(P=2)
    v = Hh.gpu_grid(64, Hh.BOUNDS)
    eng = dmf_amd.RayTracingEngine(dmf_amd.Camera(Hh.K))
    prm = dmf_amd.FuseParams(dmin_mm=200, dmax_mm=1000)
    h, m, _ = eng.fuse_depth(v, depth, poses, prm)
    ref = eng.backproject(v, depth[0], poses[0]).reshape(-1, 3)
    return v, eng.fuse_finalize(v, h, m, prm), np.ascontiguousarray(ref[::7])


def test_surface_error_equals_extract_then_nearest(fused):
    v, L, ref = fused
    _, xyz, _ = v.extract_surface(L, 1, -1)
    assert xyz.shape[0] > 1000 and ref.shape[0] > 10000
    wd, wi = CR.nearest(xyz, ref)
    gd, gi = v.cloud_nearest(xyz, ref)
    assert np.array_equal(gd.view(np.uint32), wd.view(np.uint32)) and np.array_equal(gi, wi)
    thr = (0.003, 0.005, 0.02)
    counts, mx, total, _ = CR.summaries(wd, wi, ref, thr)
    e = v.surface_error(L, ref, thresholds=thr, per_point=True)
    assert (e.n_surface, e.n_valid, e.max_error, e.over) == (xyz.shape[0], counts[0], mx, tuple(counts[2:]))
    assert abs(e.avg_error * counts[0] - total) <= 2 * xyz.shape[0] * 2.0 ** -53 * total
    assert e.dist2.dtype == np.float32 and np.array_equal(e.dist2.view(np.uint32), wd.view(np.uint32))
    s = v.surface_error(L, ref, thresholds=thr)
    # only summaries; the device's sum has no fixed order, so the mean may differ in its last bits
    assert s.dist2 is None and s[:3] == e[:3] and s.over == e.over
    assert abs(s.avg_error - e.avg_error) <= 2 * xyz.shape[0] * 2.0 ** -53 * e.avg_error
    # other thresholds of the surface, an empty model, and no surface at all
    e2 = v.surface_error(L, ref, occ_threshold=2, free_threshold=-2, per_point=True)
    x2 = v.extract_surface(L, 2, -2)[1]
    assert e2.n_surface == x2.shape[0] and np.array_equal(e2.dist2.view(np.uint32), CR.nearest(x2, ref)[0].view(np.uint32))
    none = v.surface_error(L, np.zeros((0, 3), np.float32), per_point=True)
    assert none.n_valid == 0 and none.max_error == -1.0 and math.isnan(none.avg_error) and np.isposinf(none.dist2).all()
    flat = v.surface_error(np.zeros_like(L), ref, per_point=True)
    assert (flat.n_surface, flat.n_valid, flat.max_error, flat.over) == (0, 0, -1.0, (0, 0)) and flat.dist2.size == 0
    assert v.info()["num_occupied"] == 0


def _write_pcd(path, pts, binary):
    head = (f"# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z\nSIZE 4 4 4\nTYPE F F F\nCOUNT 1 1 1\n"
            f"WIDTH {pts.shape[0]}\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS {pts.shape[0]}\nDATA {'binary' if binary else 'ascii'}\n")
    with open(path, "wb") as f:
        f.write(head.encode())
        if binary:
            f.write(np.ascontiguousarray(pts, np.float32).tobytes())
        else:
            f.write("".join(f"{float(p[0])!r} {float(p[1])!r} {float(p[2])!r}\n" for p in pts).encode())


def _cout_double(v):
    """A double as std::cout prints it by default (%g)."""
    return "%g" % v


def test_example_binary(tmp_path):
    """compat/examples/cloud_error_headless over two small PCD files written here: its two lines in the
    reference's formatting (ErrorCalc.cpp:96-97: operator<< of a double) of the restatement's numbers,
    and its raw file equal to the per-point distances."""
    q, r, wd, wi = CR.case("small_257_63")
    _write_pcd(tmp_path / "cloud.pcd", q, True)
    _write_pcd(tmp_path / "ref.pcd", r, False)
    res = subprocess.run([EXAMPLE, str(tmp_path / "cloud.pcd"), str(tmp_path / "ref.pcd"), str(tmp_path / "dist.bin")],
                         capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr
    _, mx, _, avg = CR.summaries(wd, wi, r)
    assert res.stdout.splitlines() == [f"The max error is : {_cout_double(mx)}", f"The avg error is : {_cout_double(avg)}"]
    got = np.fromfile(tmp_path / "dist.bin", np.float32)
    assert np.array_equal(got.view(np.uint32), np.sqrt(wd).view(np.uint32))


def test_status_rules(gv):
    """Item by item; a rejected call leaves every output as it was."""
    from dmf_amd import _lib
    INV, RNG = _lib.DMF_ERR_INVALID, _lib.DMF_ERR_RANGE
    q, r = np.zeros((4, 3), np.float32), np.ones((6, 3), np.float32)
    od, oi = np.full(8, FILL_D2, np.uint32), np.full(8, FILL_IDX, np.int32)
    oc, os_ = np.full(11, FILL_COUNT, np.uint64), np.full(3, FILL_SUM, np.float64)
    t = np.array([0.003, 0.005])
    P = lambda a: a.ctypes.data                                                     # noqa: E731
    outs = (P(od), P(oi))
    rejected = [
        ((None, P(q), 4, P(r), 6, *outs, P(t), 2, P(oc), P(os_)), INV),                 # null v
        (("v", None, 4, P(r), 6, *outs, P(t), 2, P(oc), P(os_)), INV),                  # null query, n > 0
        (("v", P(q), 4, None, 6, *outs, P(t), 2, P(oc), P(os_)), INV),                  # null ref, m > 0
        (("v", P(q), 4, P(r), 6, None, None, P(t), 2, None, None), INV),                # no output at all
        (("v", P(q), -1, P(r), 6, *outs, P(t), 2, P(oc), P(os_)), INV),                 # negative n
        (("v", P(q), 4, P(r), -1, *outs, P(t), 2, P(oc), P(os_)), INV),                 # negative m
        (("v", P(q), 4, P(r), 6, *outs, P(t), -1, P(oc), P(os_)), INV),                 # T < 0
        (("v", P(q), 4, P(r), 6, *outs, P(t), 9, P(oc), P(os_)), INV),                  # T > 8
        (("v", P(q), 4, P(r), 6, *outs, None, 2, P(oc), P(os_)), INV),                  # thresholds missing
        (("v", P(q), 4, P(r), 1 << 31, *outs, P(t), 2, P(oc), P(os_)), RNG),            # m >= 2^31
        (("v", P(q), 4, P(r), 1 << 40, *outs, P(t), 2, P(oc), P(os_)), RNG),
        (("v", None, 4, P(r), 1 << 31, *outs, P(t), 2, P(oc), P(os_)), INV),            # INVALID is checked first
    ]
    for fn in (gv._L.dmf_cloud_nearest, gv._L.dmf_cloud_nearest_device):
        for args, want in rejected:
            args = tuple(gv._h if a == "v" else a for a in args)
            assert fn(*args) == want, (args, want)
            assert (od == FILL_D2).all() and (oi == FILL_IDX).all() and (oc == FILL_COUNT).all() and (os_ == FILL_SUM).all()
    # n = 0 is DMF_OK and writes only the summaries; null clouds go with zero counts
    st = gv._L.dmf_cloud_nearest(gv._h, None, 0, P(r), 6, *outs, P(t), 2, P(oc), P(os_))
    assert st == _lib.DMF_OK and (od == FILL_D2).all() and (oi == FILL_IDX).all()
    assert oc.tolist() == [0, 6, 0, 0] + [int(FILL_COUNT)] * 7 and os_.tolist() == [-1.0, 0.0, FILL_SUM]
    oc[:], os_[:] = FILL_COUNT, FILL_SUM
    st = gv._L.dmf_cloud_nearest(gv._h, None, 0, None, 0, None, None, None, 0, P(oc), None)
    assert st == _lib.DMF_OK and oc.tolist() == [0, 0] + [int(FILL_COUNT)] * 9 and (os_ == FILL_SUM).all()
    st = gv._L.dmf_cloud_nearest(gv._h, P(q), 4, None, 0, *outs, None, 0, None, None)
    assert st == _lib.DMF_OK and (od[:4] == 0x7F800000).all() and (oi[:4] == -1).all() and (od[4:] == FILL_D2).all()
    stats = np.full(5, FILL_COUNT, np.uint64)
    assert gv._L.dmf_cloud_nearest_stats(gv._h, P(stats)) == _lib.DMF_OK and stats[4] == FILL_COUNT and stats[3] == 0
    for occ, order in ((-1, 0), (1025, 0), (0, -1), (0, 3)):
        assert gv._L.dmf_cloud_nearest_set_variant(gv._h, occ, order) == INV
    assert gv._L.dmf_cloud_nearest_set_variant(None, 0, 0) == INV and gv._L.dmf_cloud_nearest_set_variant(gv._h, 0, 0) == _lib.DMF_OK


def test_python_validation(gv):
    import dmf_amd
    assert dmf_amd.NO_POINT == -1
    q, r = CR.case("small_65_65")[:2]
    d2, idx = gv.cloud_nearest(q.astype(np.float16), r)                 # a type that float32 holds exactly
    assert np.array_equal(idx, CR.nearest(q.astype(np.float16).astype(np.float32), r)[1])
    d2, idx = gv.cloud_nearest(np.zeros((0, 3), np.float32), r)
    assert d2.shape == idx.shape == (0,) and d2.dtype == np.float32 and idx.dtype == np.int32
    e = gv.cloud_error(np.zeros((0, 3), np.float32), r, ())
    assert (e.n_valid, e.max_error, e.over) == (0, -1.0, ()) and math.isnan(e.avg_error) and e.dist2.size == 0
    L = np.zeros(9 * 8 * 7, np.int16)
    for bad in (lambda: gv.cloud_nearest(q.astype(np.float64), r),
                lambda: gv.cloud_nearest(q, r.astype(np.float64)),
                lambda: gv.cloud_nearest(q.astype(np.int32), r),
                lambda: gv.cloud_nearest(q[0], r),
                lambda: gv.cloud_nearest(q, r[:, :2]),
                lambda: gv.cloud_nearest(q.reshape(5, 13, 3), r),
                lambda: gv.cloud_nearest(np.zeros((4, 4), np.float32), r),
                lambda: gv.cloud_error(q, r.astype(np.float64)),
                lambda: gv.cloud_error(q, r, thresholds=tuple(range(9))),
                lambda: gv.cloud_error(q, r, thresholds=(0.003, -0.005)),
                lambda: gv.surface_error(L, r, thresholds=tuple(range(9))),
                lambda: gv.surface_error(L, r, thresholds=(-1.0,)),
                lambda: gv.surface_error(L, r.astype(np.float64)),
                lambda: gv.surface_error(L[:-1], r),
                lambda: gv.surface_error(L.astype(np.int32), r)):
        with pytest.raises(ValueError):
            bad()
