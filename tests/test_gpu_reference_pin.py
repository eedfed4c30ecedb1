"""The HIP engine against what the reference's own code computed.

Every other GPU parity test compares libdmf.so with oracle/oracle.cpp; these compare it with
tests/golden/ref_pin_<scene>.npz, the recorded results of the reference's headers themselves
(tests/golden/gen_ref_pin.py describes the scenes, tests/ref_pin.py the plan of calls).  Exact
equality throughout, and nothing but tests/golden/ is read.

The shapes: a 64x48 and a 61x37 camera (partial 8x8 tiles), grids of 64^3 and 60x50x56 (partial
bricks, off-origin, non-cubic, truncating), 0, 1 and 3000-4000 occupied voxels, cameras outside
and inside the grid (empty-space jumps from the first sample on).

* integratePointCloud, both overloads, through the host and the device entry point, with
  validPoints / getVoxel of the resulting volume;
* reverseRayTraceFast / reverseRayTrace under every kernel of REVERSE_KERNELS;
* the forward family and rayTraceVolume through their host entry points (k_forward), with and
  without empty-space skipping;
* the batched forward kernels (dmf_forward_first_hits_device under fwd_kernel 0, 1, 2: k_forward,
  k_forward_x, k_forward_q), with and without skipping: their first hits must explain what the
  reference's rayTrace marked, what rayTraceAndGetPoints listed, in its order, and what
  rayTraceAndGetMinimum returned, for every pose, lattice and zdelta of the fixture;
* OccupancyGrid::updateStates and its four downloads;
* the drop-in claim: oracle/ref_pin/ref_pin_core.cpp -- the very source that produced the fixtures
  when compiled against the reference -- compiled against compat/ and libdmf.so must write the
  same result file.
"""
import functools
import hashlib
import os

import numpy as np
import pytest

import helpers as Hh
import ref_pin as RP

pytestmark = pytest.mark.gpu

REVERSE_KERNELS = [0, 4, 5, 3, 1, 2]
FORWARD_KERNELS = [0, 1, 2]  # DMF_KNOB_FWD_KERNEL of dmf_forward_first_hits_device
UNGUARDED = [s for s in RP.SCENES if int(RP.load(s)["in_flags"]) & 2]
DROPIN = os.path.join(RP.ROOT, "depth-map-fusion-utils_amd", "build", "ref_pin_core_dmf")


@functools.lru_cache(maxsize=None)
def _fx(scene):
    return RP.load(scene)


def _records(fx, prefixes):
    return {k: v for k, v in RP.expected(fx).items() if k.startswith(prefixes)}


def _knobs(**kw):
    from dmf_amd import _lib

    def setup(v):
        for k, val in kw.items():
            _lib.set_knob(v, k, val)
    return setup


def _integrate_device(v, xyz, nrm):
    """dmf_volume_integrate_device over torch tensors in place of the host integratePointCloud."""
    import torch
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    if xyz.shape[0] == 0:
        return type(v).integratePointCloud(v, xyz, nrm)
    dp = torch.from_numpy(xyz).cuda()
    dn = torch.from_numpy(np.ascontiguousarray(nrm, np.float32)).cuda() if nrm is not None else None
    torch.cuda.synchronize()
    v.integrate_device(dp.data_ptr(), dn.data_ptr() if dn is not None else None, xyz.shape[0])
    v.synchronize()
    return True


@pytest.mark.parametrize("entry", ["host", "device"])
@pytest.mark.parametrize("scene", RP.SCENES)
def test_volume(scene, entry):
    """Dims, deltas, hsize_, occupied_cells_ in order and the per-voxel counts, with normals and
    (exact scene) without; validPoints and getVoxel around every bound of that volume."""
    import dmf_amd
    fx = _fx(scene)
    exp = _records(fx, ("vol_", "occ", "nn_", "probe_validpoints", "probe_getvoxel"))
    assert len(exp) == (11 if int(fx["in_flags"]) & 1 else 8) and exp["probe_validpoints"].size > 50
    B = RP.GpuBackend(dmf_amd, integrate=_integrate_device if entry == "device" else None)
    assert RP.differences({**RP.run_volume(B, fx), **RP.run_volume_probes(B, fx)}, exp) == []


@pytest.mark.parametrize("kernel", REVERSE_KERNELS)
@pytest.mark.parametrize("scene", RP.SCENES)
def test_reverse(scene, kernel):
    """found, good_points in order and every voxel's view / good after reverseRayTraceFast and
    (where the reference defines it) reverseRayTrace, viz on and off."""
    import dmf_amd
    fx = _fx(scene)
    exp = _records(fx, ("rev_",))
    assert len(exp) == 6 and exp["rev_found"].size >= 16
    B = RP.GpuBackend(dmf_amd, setup=_knobs(reverse_kernel=kernel))
    assert RP.differences(RP.run_reverse(B, fx), exp) == []


@pytest.mark.parametrize("skip", [0, -1])
@pytest.mark.parametrize("scene", UNGUARDED)
def test_forward_family_and_volume(scene, skip):
    """rayTrace, rayTraceAndClassify, rayTraceAndGetGoodPoints, rayTraceAndGetPoints,
    rayTraceAndGetMinimum (sparse and dense, zdelta 10 / 7 / 1, every pose), rayTraceVolume, and
    the flags that survive from one call into the next."""
    import dmf_amd
    fx = _fx(scene)
    exp = _records(fx, ("fwd_", "rtv_", "chain_"))
    P = fx["in_poses"].reshape(-1, 12).shape[0]
    assert len(exp) == 18 and exp["fwd_found"].size == 30 * P
    B = RP.GpuBackend(dmf_amd, setup=_knobs(fwd_skip=skip))
    assert RP.differences(RP.run_forward(B, fx), exp) == []


@pytest.mark.parametrize("kernel", FORWARD_KERNELS)
@pytest.mark.parametrize("skip", [0, -1])
@pytest.mark.parametrize("scene", UNGUARDED)
def test_forward_device_kernels(scene, skip, kernel):
    """Each batched forward kernel against the reference.  A pixel's first hit (plane k, voxel) is
    all the reference's marches act on: rayTrace sets view = 1 on exactly the first-hit voxels of
    its lattice; rayTraceAndGetPoints lists them in (plane, row, column) order of first sight;
    rayTraceAndGetMinimum returns the nearest plane of its own lattice (stride 10, from 5 mm)."""
    import dmf_amd
    fx = _fx(scene)
    exp = RP.expected(fx)
    K, H, W = fx["in_K"], int(fx["in_H"]), int(fx["in_W"])
    poses = fx["in_poses"].reshape(-1, 12)
    P, occ, V = poses.shape[0], exp["occ"], exp["occ"].size
    calls = {c: i for i, c in enumerate(RP.forward_calls(P))}
    off = np.concatenate([[0], np.cumsum(exp["fwd_count"])])
    gv = RP.make_volume(RP.GpuBackend(dmf_amd, setup=_knobs(fwd_skip=skip, fwd_kernel=kernel)), fx)
    dc = Hh.DeviceCalls(gv)
    hits = 0
    try:
        for sparse in (True, False):
            for zd in (10, 7, 1):
                s = 5 if sparse else 1
                k, slot, _ = dc.forward(K, H, W, poses, 10, zd, s, s)
                sm = 10 if sparse else 1
                km, slotm, _ = dc.forward(K, H, W, poses, 5, zd, sm, sm)
                for p in range(P):
                    hit = k[p] >= 0
                    assert (slot[p][~hit] == -1).all() and (k[p][~hit] == -1).all()
                    assert ((slot[p][hit] >= 0) & (slot[p][hit] < V)).all()
                    hits += int(hit.sum())
                    # rayTrace: view = 1 on the first-hit voxels, nowhere else
                    view = np.zeros(V, np.int32)
                    view[slot[p][hit]] = 1
                    i = calls[p, 0, sparse, zd]
                    assert np.array_equal(view, exp["fwd_view"][i * V:(i + 1) * V]), (p, sparse, zd)
                    # rayTraceAndGetPoints: the voxels in order of first sight
                    r, c = np.nonzero(hit)
                    order = np.lexsort((c, r, k[p][r, c]))
                    seq = slot[p][r, c][order]
                    _, first = np.unique(seq, return_index=True)
                    lst = occ[seq[np.sort(first)]] if seq.size else np.zeros(0, np.uint64)
                    i = calls[p, 3, sparse, zd]
                    assert exp["fwd_found"][i] == int(hit.any())
                    assert np.array_equal(lst, exp["fwd_list"][off[i]:off[i + 1]]), (p, sparse, zd)
                    # rayTraceAndGetMinimum: the nearest plane of the stride-10 (or dense) lattice
                    hm = km[p] >= 0
                    ret = 5 + zd * int(km[p][hm].min()) if hm.any() else -1
                    assert ret == exp["fwd_ret"][calls[p, 4, sparse, zd]], (p, sparse, zd)
    finally:
        dc.close()
    assert (hits > 0) == (V > 0)


@pytest.mark.parametrize("scene", [s for s in RP.SCENES if RP.has_ogrid(RP.load(s))])
def test_occupancy_grid(scene):
    import dmf_amd
    fx = _fx(scene)
    exp = _records(fx, ("og_",))
    assert len(exp) == 9 and exp["og_hq"].size and exp["og_reorg_clean"].size
    assert RP.differences(RP.run_ogrid(RP.GpuBackend(dmf_amd), fx), exp) == []


@pytest.mark.parametrize("scene", RP.SCENES)
def test_dropin_driver_writes_the_reference_file(scene, tmp_path):
    """One source, two builds: against the reference it wrote the fixture, against compat/ and
    libdmf.so it must write the same bytes."""
    assert os.path.exists(DROPIN), "build it: python -c 'import __graft_entry__ as g; g.build()'"
    fx = _fx(scene)
    raw = RP.start_binary(DROPIN, RP.core_scene_bytes(fx), str(tmp_path), scene)()
    exp = {k: v for k, v in RP.expected(fx).items() if not k.startswith("og_")}
    assert RP.differences(RP.parse_result(raw), exp) == []
    assert hashlib.sha256(raw).hexdigest() == fx["meta"]["sha256_core"]
