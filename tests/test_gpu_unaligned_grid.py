"""GPU: the device forms of the fused grid's three consumers (ray-cast, surface extraction, distance
field) on a grid pointer that is NOT 16-B aligned.  The shared 8-cell loader (csrc/dmf_gridbits.hpp)
then takes its cell-by-cell path for every group instead of the 16-B load; every other device test
passes dmf_device_malloc bases.  The grid sits at base + 2 bytes between int16 cells of 32767, solid
at every threshold used: a neighbour read as a cell changes the result.  Exact equality with the
restatements, element by element and on both counters, as the neighbouring tests compare them."""
import functools

import numpy as np
import pytest

import distance_ref as DR
import helpers as Hh
import raycast_cases as RC
import raycast_ref as RR
import surface_ref as SR
import test_gpu_distance as TD
import test_gpu_raycast as TR
import test_gpu_surface as TS
from dmf_amd import scene

pytestmark = pytest.mark.gpu

PAD = 32767
TRAIL = 8                                  # int16 cells of PAD after the grid (one before it)

# every z-row a whole number of 16-B groups: with an aligned base every group takes the wide load,
# with the moved base none may
SMALL_DIMS = (9, 8, 16)
SMALL_K, SMALL_H, SMALL_W = np.array([20, 0, 7.3, 0, 20, 5.7, 0, 0, 1], np.float32), 12, 16
SMALL_RANGE = 2000


@functools.lru_cache(maxsize=None)
def small_grid():
    L = np.where(np.random.default_rng(102).random(SMALL_DIMS) < 0.05, 5, -3).astype(np.int16)
    assert int((L >= 1).sum()) == 43
    L.setflags(write=False)
    return L


@functools.lru_cache(maxsize=None)
def small_poses():
    return np.ascontiguousarray(scene.fibonacci_poses(2, seed=5), np.float32)


@functools.lru_cache(maxsize=None)
def small_raycast_ref():
    wk = RR.Walk(Hh.ODD_BOUNDS, SMALL_DIMS, SMALL_K, SMALL_H, SMALL_W, small_poses(), SMALL_RANGE)
    return wk.surface(small_grid(), 1)


def _moved(dc, L):
    """The grid on the device at a base + 2 bytes, PAD before and after it -> its device pointer."""
    flat = np.ascontiguousarray(L, np.int16).reshape(-1)
    base = dc.upload(np.concatenate([[PAD], flat, np.full(TRAIL, PAD)]).astype(np.int16))
    assert base % 16 == 0
    return base + 2


# (volume dims, bounds, grid) of the two cases
def _small():
    return SMALL_DIMS, Hh.ODD_BOUNDS, small_grid()


def _odd():
    return RC.DIMS1, RC.BOUNDS1, np.asarray(RC.grid1(), np.int16).reshape(RC.DIMS1)


def test_raycast_small_grid_reference_has_both_outcomes():
    ref = small_raycast_ref()
    found = ref["index"] >= 0
    assert found.any() and (~found).any() and (ref["length"] > 0).all()


@pytest.mark.parametrize("case", ["small", "odd"])
def test_raycast(case):
    from dmf_amd import _lib
    if case == "small":
        (dims, bounds, L), cam, poses, rng = _small(), (SMALL_K, SMALL_H, SMALL_W), small_poses(), SMALL_RANGE
        refs = {1: small_raycast_ref()}
    else:
        (dims, bounds, L), cam, poses, rng = _odd(), (RC.KA, RC.HA, RC.WA), RC.poses1(), RC.RANGE1
        refs = {t: RC.ref1(t) for t in RC.THRESHOLDS1}
    gv = Hh.gpu_grid(dims, bounds)
    dc = Hh.DeviceCalls(gv)
    try:
        d_L = _moved(dc, L)
        for walk in TR.WALKS:
            _lib.set_knob(gv, "raycast_walk", walk)
            for threshold, ref in refs.items():
                depth, cell, stats = TR._device(dc, *cam, d_L, poses, threshold, rng)
                assert np.array_equal(cell, ref["cell"]), (walk, threshold, int((cell != ref["cell"]).sum()))
                assert np.array_equal(depth, ref["depth"]), (walk, threshold, int((depth != ref["depth"]).sum()))
                assert np.array_equal(stats, ref["stats"]), (walk, threshold, stats, ref["stats"])
    finally:
        dc.close()
        _lib.set_knob(gv, "raycast_walk", 0)


@pytest.mark.parametrize("case", ["small", "odd"])
def test_surface(case):
    if case == "small":
        dims, bounds, L = _small()
        refs = {(1, -1): SR.surface(bounds, dims, L, 1, -1)}
        assert refs[1, -1]["count"][1] == 43 and refs[1, -1]["count"][0] > 0
    else:
        dims, bounds, L = _odd()
        refs = {t: SR.ref1(t) for t in SR.THRESHOLDS1}
    gv = Hh.gpu_grid(dims, bounds)
    dc = Hh.DeviceCalls(gv)
    try:
        d_L = _moved(dc, L)
        for (occ, free), ref in refs.items():
            m, solid = ref["count"]
            cnt, h, xyz, nrm = TS._device(dc, d_L, occ, free, m + 2)
            assert cnt.tolist() == [m, solid], (occ, free, cnt, m, solid)
            TS._assert_prefix(ref, m, h, xyz, nrm, what=f"device {occ} {free}")
    finally:
        dc.close()


@pytest.mark.parametrize("case", ["small", "odd"])
def test_distance_into_an_unaligned_field(case):
    """... and d_dist2 = base + 4 bytes: no 16-B store either; the entry before the field and the
    guard after it keep their fill."""
    from dmf_amd import _lib
    if case == "small":
        dims, bounds, L = _small()
        refs = {1: DR.edt2(L, dims, 1)}
    else:
        dims, bounds, L = _odd()
        refs = {DR.case(n)[2]: DR.case(n)[3] for n in ("grid1_t1", "grid1_t3511", "grid1_all")}
    n = int(np.prod(dims))
    gv = Hh.gpu_grid(dims, bounds)
    dc = Hh.DeviceCalls(gv)
    try:
        d_L = _moved(dc, L)
        for threshold, ref in refs.items():
            d_out = dc.upload(np.full(1 + n + TD.GUARD, TD.FILL, np.uint32))
            d_cnt = dc.upload(np.full(2, TD.FILL_COUNT, np.uint64))
            assert d_out % 16 == 0
            _lib.check(dc.L.dmf_grid_distance_device(dc.h, d_L, int(threshold), d_out + 4, d_cnt))
            out, cnt = dc.download(d_out, 1 + n + TD.GUARD, np.uint32), dc.download(d_cnt, 2, np.uint64)
            assert cnt.tolist() == [int((ref == 0).sum()), int(TD.FILL_COUNT)], (threshold, cnt)
            assert int((out[1:n + 1] != ref.reshape(-1)).sum()) == 0, threshold
            assert out[0] == TD.FILL and (out[n + 1:] == TD.FILL).all(), threshold
    finally:
        dc.close()
