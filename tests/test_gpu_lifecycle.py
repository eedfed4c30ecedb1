"""GPU parity across a volume's life: query, change the volume or a control, query again.

integratePointCloud drops the enumeration, the brick distance field and the spatial order; a new
distance-field cap drops the field; constructVolume on a used handle frees everything.  A cache
kept by mistake does not fault, it answers for the volume as it was -- so each step below is
compared with the CPU oracle, and the oracle's answers are asserted to change between steps.
Also here: the entry points that had no parity test at test size (dmf_volume_export, a volume
with and without normals, dmf_volume_integrate_device).
"""
import numpy as np
import pytest

import helpers as Hh
from helpers import H, K, W

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dmf():
    import dmf_amd
    return dmf_amd


@pytest.fixture(scope="module")
def engine(dmf):
    return dmf.RayTracingEngine(dmf.Camera(K, H, W))


@pytest.fixture(scope="module")
def oeng(oracle):
    return oracle.Engine(K, H, W)


def _knob(gv, name, value):
    from dmf_amd import _lib
    _lib.set_knob(gv, name, value)


def _halves():
    pts, nn = Hh.cloud()
    half = pts.shape[0] // 2
    return (pts[:half], nn[:half]), (pts[half:], nn[half:])


def _sparse_cloud():
    """The scatter of test_reverse_sparse_partial_bricks (for ODD_BOUNDS / ODD_DIMS)."""
    rng = np.random.default_rng(21)
    pts = rng.uniform([-0.44, -0.39, -0.32], [0.51, 0.46, 0.40], (400, 3)).astype(np.float32)
    nn = rng.normal(size=(400, 3)).astype(np.float32)
    nn /= np.linalg.norm(nn, axis=1, keepdims=True)
    return pts, nn


def _query_round(ov, gv, oeng, engine, poses, fwd=(10, 10, 5, 5)):
    """Reverse fast (all poses), reverse full, rayTraceVolume and forward first hits (pose 0):
    oracle == GPU; returns the oracle's answers."""
    fast = [oeng.reverseRayTraceFast(ov, T, False) for T in poses]
    found, lists = engine.reverseRayTraceFastBatch(gv, poses, viz=False)
    for i, (f, g) in enumerate(fast):
        assert f == bool(found[i]) and np.array_equal(g, lists[i]), f"pose {i}: {len(g)} vs {len(lists[i])}"
    fo, go = oeng.reverseRayTrace(ov, poses[0], False)
    fg, gg = engine.reverseRayTrace(gv, poses[0], False)
    assert fo == fg and np.array_equal(go, gg)
    zo = oeng.rayTraceVolume(ov, poses[0])
    assert np.array_equal(zo, engine.rayTraceVolume(gv, poses[0]))
    ko, ho = oeng.forward_first_hits(ov, poses[0], *fwd)
    kg, hg = engine.forward_first_hits(gv, poses[0], *fwd)
    assert np.array_equal(ko, kg) and np.array_equal(ho[ko >= 0], hg[kg >= 0])
    assert len(go) > 0 and (zo >= 0).any() and (ko >= 0).any()
    return [len(g) for _, g in fast], go, zo, ko


def test_query_mutate_query(oracle, dmf, engine, oeng):
    """One GPU volume through its life against one oracle volume: integrate half a cloud, query
    (the default reverse kernel builds the spatial order and the distance field, reverseRayTrace
    and rayTraceVolume the enumeration), integrate the rest, query again; then new distance-field
    caps, reverse kernels and forward skipping between marches, reset_flags, and a new geometry
    constructed on the same handle."""
    from dmf_amd import scene
    first, second = _halves()
    poses = scene.fibonacci_poses(3, seed=11)
    ov, gv = Hh.volume_pair(oracle, 64, clouds=[first])
    n1, full1, z1, k1 = _query_round(ov, gv, oeng, engine, poses)
    for v in (ov, gv):
        v.integratePointCloud(*second)
    assert np.array_equal(ov.occupied_cells_, gv.occupied_cells_)
    n2, full2, z2, k2 = _query_round(ov, gv, oeng, engine, poses)
    # the second cloud changed every answer: a cache kept across integratePointCloud fails above
    assert n1 != n2 and sum(n2) > sum(n1) > 0
    assert not np.array_equal(full1, full2) and not np.array_equal(z1, z2) and not np.array_equal(k1, k2)
    # controls switched between marches of one volume
    for cap in (0, 1, 255, 0):
        _knob(gv, "bdist_cap", cap)
        _query_round(ov, gv, oeng, engine, poses)
    for kernel in (1, 0, 5, 3, 4, 2, 0):
        _knob(gv, "reverse_kernel", kernel)
        _query_round(ov, gv, oeng, engine, poses)
    for skip in (-1, 0, -1, 0):
        _knob(gv, "fwd_skip", skip)
        _query_round(ov, gv, oeng, engine, poses, fwd=(10, 7, 3, 4))
    # flags: set by a viz round, cleared by reset_flags, set again
    for rnd in range(2):
        for T in poses[:2]:
            f, g = oeng.reverseRayTraceFast(ov, T, True)
            f2, g2 = engine.reverseRayTraceFast(gv, T, True)
            assert f == f2 and np.array_equal(g, g2)
        assert ov.voxel_table()[0].any() and ov.voxel_table()[1].any() and Hh.flags_equal(ov, gv)
        ov.reset_flags()
        gv.reset_flags()
        assert not gv.voxel_flags()[0].any() and not gv.voxel_flags()[1].any() and Hh.flags_equal(ov, gv)
    # a new geometry on the same handle
    gv.setDimensions(*Hh.ODD_BOUNDS)
    gv.setVolumeSize(*Hh.ODD_DIMS)
    gv.constructVolume()
    assert tuple(gv.dims) == Hh.ODD_DIMS and len(gv.occupied_cells_) == 0 and gv.info()["num_points"] == 0
    ov2 = oracle.Volume()
    ov2.setDimensions(*Hh.ODD_BOUNDS)
    ov2.setVolumeSize(*Hh.ODD_DIMS)
    ov2.constructVolume()
    pts, nn = _sparse_cloud()
    ov2.integratePointCloud(pts, nn)
    gv.integratePointCloud(pts, nn)
    assert np.array_equal(ov2.occupied_cells_, gv.occupied_cells_) and len(gv.occupied_cells_) > 300
    poses2 = np.concatenate([scene.fibonacci_poses(4, seed=5), scene.reference_style_poses(pts[:2], nn[:2], 150)])
    n3, _, _, _ = _query_round(ov2, gv, oeng, engine, poses2)
    assert sum(n3) > 0
    for T in poses2[:3]:
        f, g = oeng.reverseRayTraceFast(ov2, T, True)
        f2, g2 = engine.reverseRayTraceFast(gv, T, True)
        assert f == f2 and np.array_equal(g, g2)
    assert ov2.voxel_table()[0].any() and Hh.flags_equal(ov2, gv)


def test_fuse_replans_across_cameras_and_variants(oracle, dmf):
    """Fusion calls of different image sizes and pose counts on one volume (3 frames of 61x37, 2 of
    640x480, 1 of 61x37), with each implementation in turn, all accumulated into the same host
    counters: the scratch is re-planned between the calls and the sum equals the oracle's."""
    from dmf_amd import _lib, scene
    Ka, (Wa, Ha) = Hh.KA, Hh.KA_WH
    big_poses, big_depth, _ = Hh.frames()
    pa = Hh.five_poses()
    da = np.stack([scene.render(Ka, Wa, Ha, T)[0] for T in pa[:4]])
    assert all((d > 0).any() for d in da)
    calls = [(Ka, Ha, Wa, da[:3], pa[:3]), (K, H, W, big_depth[:2], big_poses[:2]), (Ka, Ha, Wa, da[3:4], pa[3:4])]
    ov, gv = Hh.volume_pair(oracle, 64)
    n = 64 ** 3
    ho, mo, so = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(3, np.int64)
    hg, mg, sg = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(3, np.int64)
    prm = dmf.FuseParams(dmin_mm=200, dmax_mm=1000)
    for variant in (57, 40, 31):
        _lib.set_variant(gv, variant)
        for Kc, Hc, Wc, depth, poses in calls:
            before = int(so[0])
            so += oracle.fuse_depth(ov, Kc, depth, poses, dmin=200, dmax=1000, hits=ho, misses=mo)[2]
            assert int(so[0]) > before  # each call adds updates
            eng = dmf.RayTracingEngine(dmf.Camera(Kc, Hc, Wc))
            sg += eng.fuse_depth(gv, depth, poses, prm, hits=hg, misses=mg)[2]
            assert np.array_equal(so, sg), (variant, Hc, Wc)
            assert np.array_equal(ho, hg) and np.array_equal(mo, mg), (variant, Hc, Wc)
    assert ho.any() and mo.any()


def test_construct_forgets_the_last_fusion(oracle, dmf, engine):
    """constructVolume frees the fusion scratch, and with it the batch table the latest
    brick-pipeline call left for dmf_fuse_batches_used: the count is 0 again (it used to be copied
    from the freed table), and the handle fuses like a new one."""
    from dmf_amd import _lib
    poses, depth, _ = Hh.frames()
    ov, gv = Hh.volume_pair(oracle, 64)
    _lib.set_variant(gv, 57)
    prm = dmf.FuseParams(dmin_mm=200, dmax_mm=1000)
    engine.fuse_depth(gv, depth[:2], poses[:2], prm)
    assert _lib.kernel_name(gv).startswith("dmf::k_bk_fuse_s<") and _lib.fuse_batches_used(gv) >= 1
    gv.constructVolume()
    assert _lib.fuse_batches_used(gv) == 0
    ho, mo, so = oracle.fuse_depth(ov, K, depth[:2], poses[:2], dmin=200, dmax=1000)
    hg, mg, sg = engine.fuse_depth(gv, depth[:2], poses[:2], prm)
    assert so[0] > 0 and np.array_equal(so, sg) and np.array_equal(ho, hg) and np.array_equal(mo, mg)
    assert _lib.fuse_batches_used(gv) >= 1


def _check_export(ov, gv):
    """dmf_volume_export == the oracle's per-voxel points / normals, every slot."""
    off, pts, nrm4 = gv.export()
    occ = ov.occupied_cells_
    _, _, onp, onn = ov.voxel_table()
    assert len(occ) > 0 and off.shape == (len(occ) + 1,) and off[0] == 0
    assert np.array_equal(np.diff(off), onp) and off[-1] == gv.info()["num_points"] == onp.sum()
    assert set(np.unique(nrm4[:, 3]).tolist()) <= {0.0, 1.0}
    for s, h in enumerate(occ):
        x, y, z = int(h) >> 40, (int(h) >> 20) & 0xFFFFF, int(h) & 0xFFFFF
        op, on = ov.voxel_points(x, y, z)
        a, b = off[s], off[s + 1]
        assert np.array_equal(op.view(np.uint32), pts[a:b].view(np.uint32)), s
        has = nrm4[a:b, 3] == 1.0
        assert int(has.sum()) == onn[s], s
        assert np.array_equal(on[:onn[s]].view(np.uint32), nrm4[a:b][has][:, :3].copy().view(np.uint32)), s
    return off, pts, nrm4


def test_volume_export(oracle):
    first, second = _halves()
    ov, gv = Hh.volume_pair(oracle, 64, clouds=[first, second])
    _, _, nrm4 = _check_export(ov, gv)
    assert (nrm4[:, 3] == 1.0).all()


def test_mixed_normals(oracle, engine, oeng):
    """One integration with normals and one without into the same volume: normals counts, the
    points / normals of every voxel and a reverseRayTraceFast query (its normal test skips the
    points that carried none)."""
    first, second = _halves()
    from dmf_amd import scene
    ov, gv = Hh.volume_pair(oracle, 64, clouds=[first, (second[0], None)])
    assert np.array_equal(ov.occupied_cells_, gv.occupied_cells_)
    _, _, onp, onn = ov.voxel_table()
    gnp, gnn = gv.voxel_counts()
    assert np.array_equal(onp, gnp) and np.array_equal(onn, gnn)
    assert (onn == 0).any() and (onn == onp).any() and ((onn > 0) & (onn < onp)).any()  # every kind of voxel
    occ = ov.occupied_cells_
    for h in occ[:: max(1, len(occ) // 200)]:
        x, y, z = int(h) >> 40, (int(h) >> 20) & 0xFFFFF, int(h) & 0xFFFFF
        op, on = ov.voxel_points(x, y, z)
        gp, gn = gv.voxel_points(h)
        assert np.array_equal(op, gp) and np.array_equal(on, gn)
    _, _, nrm4 = _check_export(ov, gv)
    assert (nrm4[:, 3] == 1.0).any() and (nrm4[:, 3] == 0.0).any()
    poses = scene.fibonacci_poses(3, seed=11)
    found, lists = engine.reverseRayTraceFastBatch(gv, poses, viz=False)
    total = 0
    for i, T in enumerate(poses):
        f, g = oeng.reverseRayTraceFast(ov, T, False)
        assert f == bool(found[i]) and np.array_equal(g, lists[i])
        total += len(g)
    assert total > 0


@pytest.mark.parametrize("with_normals", [True, False])
def test_integrate_device_equals_host(oracle, dmf, with_normals):
    """dmf_volume_integrate_device over device tensors == integratePointCloud from the host, in
    two calls each: occupied list, per-voxel counts and the whole export (and the oracle's list)."""
    import torch
    clouds = [(p, n if with_normals else None) for p, n in _halves()]
    ov, host = Hh.volume_pair(oracle, 64, clouds=clouds)
    dev = dmf.VoxelVolume()
    dev.setDimensions(*Hh.BOUNDS)
    dev.setVolumeSize(64, 64, 64)
    dev.constructVolume()
    for p, n in clouds:
        dp = torch.from_numpy(p).cuda()
        dn = torch.from_numpy(n).cuda() if n is not None else None
        torch.cuda.synchronize()
        dev.integrate_device(dp.data_ptr(), dn.data_ptr() if dn is not None else None, p.shape[0])
        dev.synchronize()
    occ = ov.occupied_cells_
    assert len(occ) > 1000
    assert np.array_equal(occ, host.occupied_cells_) and np.array_equal(occ, dev.occupied_cells_)
    for a, b in zip(host.voxel_counts(), dev.voxel_counts()):
        assert np.array_equal(a, b)
    assert dev.voxel_counts()[1].any() == with_normals
    for a, b in zip(host.export(), dev.export()):
        assert a.size > 0 and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert dev.info()["num_points"] == host.info()["num_points"] == int(ov.voxel_table()[2].sum())
