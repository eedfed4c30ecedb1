"""OccupancyGrid beyond the shallow inputs of test_ogrid.py: the single-lane fallback of
downloadReorganizedCloud, fixed points tens of rounds deep and at the round cap, voxels with
hundreds of points (the HQ / clean threshold on real updateStates data, event runs longer than a
block), the input edges, the device entry point, the download capacity contract and the C++
drop-in.  The CPU tests first show on the oracle side that each input does what its GPU test
relies on (tests/ogrid_ref.py: the round emulator and the generators)."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import ogrid_ref as R
from test_ogrid import _REORG_GRIDS, _adversarial_state, _inputs, _setup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "depth-map-fusion-utils_amd", "build", "ogrid_headless")

# ---- chain states (grid of R.CHAIN_GRIDS, seed, emulated rounds) found by scanning seeds 0..399
# with R.fixed_point_rounds; test_chain_rounds pins every figure.
DEEP = [(0, 0, 49), (0, 6, 36), (2, 1, 44)]    # settle under the default cap of 64
AT_64 = (2, 6, 64)                             # the last round the default cap allows
AT_65 = (2, 38, 65)                            # one more
OVER = (1, 1, 75)                              # 12 x 10 x 9: past the cap, settles under cap 200
OVER_SMALL = (0, 2, 73)                        # 9 x 8 x 7 and past the cap (test_one_grid_across_paths)
CHAINS = DEEP + [AT_64, AT_65, OVER, OVER_SMALL]
CLEAN_COUNTS = (100, 150, 250)                 # every voxel passes the clean gate: the same merges


@functools.lru_cache(maxsize=None)
def _chain(gi, seed, clean):
    bounds, res = R.CHAIN_GRIDS[gi]
    return R.chain_state(R.grid_dims(bounds, res), bounds, res, seed,
                         counts=CLEAN_COUNTS if clean else (1, 7, 250))


@functools.lru_cache(maxsize=None)
def _emulated(gi, seed, clean):
    bounds, res = R.CHAIN_GRIDS[gi]
    return R.fixed_point_rounds(R.grid_dims(bounds, res), bounds[0::2], np.float32(res), *_chain(gi, seed, clean), clean,
                                return_cloud=True)


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(got, exp):
    return got.shape == exp.shape and np.array_equal(_u32(got), _u32(exp))


# ---- dense updateStates input on the 8 mm grid of test_ogrid._setup ------------------------
DENSE_BOUNDS = (-0.45, 0.47, -0.43, 0.44, -0.41, 0.4)
DENSE_RES = (0.008, 0.008, 0.008)
SMALL_RES = (0.02, 0.02, 0.02)  # at most 48 cells per axis: the grid of the fallback after updateStates


@functools.lru_cache(maxsize=None)
def _dense_input(res=DENSE_RES, seed=5):
    """3000 points of test_ogrid._inputs + 24 dense voxels (R.dense_cloud), shuffled: one voxel at
    index 0 and one at dims - 1 of an axis (clipped K-neighbourhoods), two face neighbours, one
    with 800 points (an event run over more than two 256-thread blocks), the others 90..260."""
    dims = R.grid_dims(DENSE_BOUNDS, res)
    rng = np.random.default_rng(seed)
    vox = [(0, dims[1] // 3, dims[2] // 2), (dims[0] // 2, dims[1] - 1, dims[2] // 3),
           (dims[0] // 4, dims[1] // 4, dims[2] // 4), (dims[0] // 4 + 1, dims[1] // 4, dims[2] // 4),
           (dims[0] // 5, dims[1] // 2, dims[2] - 1)]
    while len(vox) < 24:
        v = tuple(int(rng.integers(2, dims[a] - 2)) for a in range(3))
        if all(max(abs(v[a] - w[a]) for a in range(3)) > 5 for w in vox):  # apart: K = 2 neighbourhoods disjoint
            vox.append(v)
    counts = [int(c) for c in rng.integers(90, 261, len(vox))]
    counts[5] = 800
    dc, dn = R.dense_cloud(dims, DENSE_BOUNDS[0::2], res, rng, vox, counts)
    c0, n0 = _inputs(seed=31, n=3000)
    cloud, normals = np.concatenate([c0, dc]), np.concatenate([n0, dn])
    if res == SMALL_RES:
        # a bridge: 120 + 240 points on the x-parallel line through the centres of two x-neighbours
        # (the first pair with no other point within 3 voxels), normals +x.  With K = 1 both voxels
        # fold all 360 points, and both centroids (the points' mean) lie in the second: the first
        # merges into a voxel after it, a dependency that takes the reorganization a second round
        # -- with clean as well
        r = float(np.float32(res[0]))
        mins = np.array(DENSE_BOUNDS[0::2])
        taken = np.zeros(dims, bool)
        ijk = np.floor((cloud.astype(np.float64) - mins) / r).astype(int)
        ijk = ijk[np.all((ijk >= 0) & (ijk < np.array(dims)), axis=1)]
        taken[tuple(ijk.T)] = True
        a = next(v for v in np.ndindex(*dims) if min(v) >= 4 and all(v[i] < dims[i] - 5 for i in range(3))
                 and not taken[v[0] - 3:v[0] + 5, v[1] - 3:v[1] + 4, v[2] - 3:v[2] + 4].any())
        c = mins + (np.array(a) + 0.5) * r
        x = np.concatenate([rng.uniform(-0.4 * r, 0.4 * r, 120), rng.uniform(0.6 * r, 1.4 * r, 240)])
        bp = c + np.stack([x, rng.normal(0, 0.0003, 360), rng.normal(0, 0.0003, 360)], 1)
        bn = np.concatenate([bp, np.tile([[1.0, 0.0, 0.0]], (360, 1))], 1)
        cloud, normals = np.concatenate([cloud, bp.astype(np.float32)]), np.concatenate([normals, bn.astype(np.float32)])
    perm = rng.permutation(cloud.shape[0])
    return np.ascontiguousarray(cloud[perm]), np.ascontiguousarray(normals[perm])


def _split():
    """The dense input in two updateStates calls: every dense voxel gets half of its points in
    each, so that those of 101..200 points cross the threshold of 100 only in the second."""
    cloud, normals = _dense_input()
    h = cloud.shape[0] // 2
    return [(cloud[:h], normals[:h]), (cloud[h:], normals[h:])]


@functools.lru_cache(maxsize=None)
def _dense_oracle(k, res=DENSE_RES):
    """Oracle run of the dense input: (state, [downloadCloud, HQ, reorganized, reorganized clean])."""
    from oracle import oracle as O
    cloud, normals = _dense_input(res)
    og = _setup(O.OccupancyGrid(), k, res, DENSE_BOUNDS)
    og.updateStates(cloud, normals)
    return og.state(), [og.download(0), og.download(1), og.downloadReorganizedCloud(False),
                        og.downloadReorganizedCloud(True)]


def _gpu_downloads(gg):
    return [gg.downloadCloud(), gg.downloadHQCloud(), gg.downloadReorganizedCloud(False),
            gg.downloadReorganizedCloud(True)]


def _states_equal(og, gg):
    return all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(og.state(), gg.state()))


# ============================================================================ CPU: the inputs do what the GPU tests need

@pytest.mark.parametrize("case", CHAINS)
@pytest.mark.parametrize("clean", [False, True])
def test_chain_oracle_vs_python(oracle, case, clean):
    """oracle.cpp == py_oracle on the chain states, bit for bit, and so is the emulator's fixed point."""
    from oracle import py_oracle as P
    gi, seed, _ = case
    bounds, res = R.CHAIN_GRIDS[gi]
    st = _chain(gi, seed, clean)
    og = _setup(oracle.OccupancyGrid(), 0, res, bounds)
    assert og.dims == R.grid_dims(bounds, res)
    og.set_state(*st)
    got = og.downloadReorganizedCloud(clean)
    exp = P.reorganized_cloud(og.dims, bounds[0::2], np.float32(res), *st, clean)
    assert got.shape[0] > 100 and _same(got, exp)
    assert _same(_emulated(gi, seed, clean)[1], exp)


@pytest.mark.parametrize("clean", [False, True])
def test_chain_rounds(clean):
    """The emulated rounds of every chain state are the recorded ones: the deep states settle in
    30..60 rounds (two grids), one state in exactly 64, one in exactly 65, one needs >= 70."""
    for gi, seed, rounds in CHAINS:
        assert _emulated(gi, seed, clean)[0] == rounds, (gi, seed)
    assert all(30 <= r <= 60 for _, _, r in DEEP) and len({g for g, _, _ in DEEP}) >= 2
    assert AT_64[2] == 64 and AT_65[2] == 65 and OVER[2] >= 70


def test_chain_unclean_counts_gate():
    """With counts from {1, 7, 250} the clean gate cuts the chains short (a different, shallow
    problem): the clean runs of the deep tests therefore draw counts from CLEAN_COUNTS."""
    gi, seed, rounds = DEEP[0]
    bounds, res = R.CHAIN_GRIDS[gi]
    r = R.fixed_point_rounds(R.grid_dims(bounds, res), bounds[0::2], np.float32(res), *_chain(gi, seed, False), True)
    assert 2 <= r < rounds


@pytest.mark.parametrize("grid", range(len(_REORG_GRIDS)))
def test_adversarial_states_need_two_rounds(grid):
    """Every adversarial state of the forced-fallback test needs 2..4 rounds: a cap of 1 cannot settle it."""
    bounds, res = _REORG_GRIDS[grid]
    dims = R.grid_dims(bounds, res)
    for seed in range(4):
        st = _adversarial_state(dims, bounds, np.float32(res), 100 + seed)
        for clean in (False, True):
            assert 2 <= R.fixed_point_rounds(dims, bounds[0::2], np.float32(res), *st, clean) <= 4


@pytest.mark.parametrize("k", [0, 1, 2])
def test_dense_input_nontrivial(k):
    (nrm, cen, cnt, fl), dl = _dense_oracle(k)
    cloud, normals = _dense_input()
    dims = R.grid_dims(DENSE_BOUNDS, DENSE_RES)
    print(f"k={k}: largest count {cnt.max()}, voxels > 100: {(cnt > 100).sum()}, rows {[len(d) for d in dl]}, "
          f"longest run {R.longest_event_run(dims, DENSE_BOUNDS[0::2], DENSE_RES, cloud, k)}")
    assert cnt.max() >= 150
    assert len(dl[1]) >= 10 and len(dl[3]) >= 10 and len(dl[0]) > 1000 and len(dl[2]) > 100
    assert R.longest_event_run(dims, DENSE_BOUNDS[0::2], DENSE_RES, cloud, k) >= 600
    assert R.longest_event_run(dims, DENSE_BOUNDS[0::2], DENSE_RES, normals, k) >= 600


def test_dense_small_grid_nontrivial():
    """The state after updateStates (K = 1) on the small grid needs a second round, clean or not:
    a cap of 1 forces the fallback."""
    st, dl = _dense_oracle(1, SMALL_RES)
    cnt = st[2]
    dims = R.grid_dims(DENSE_BOUNDS, SMALL_RES)
    rounds = [R.fixed_point_rounds(dims, DENSE_BOUNDS[0::2], np.float32(SMALL_RES), *st, clean) for clean in (False, True)]
    print(f"small grid: largest count {cnt.max()}, rows {[len(d) for d in dl]}, rounds {rounds}")
    assert max(dims) <= 48 and min(rounds) >= 2
    assert cnt.max() >= 150 and len(dl[3]) >= 10 and len(dl[2]) >= 10


def test_split_input_crosses_threshold(oracle):
    og = _setup(oracle.OccupancyGrid(), 0, DENSE_RES, DENSE_BOUNDS)
    parts = _split()
    og.updateStates(*parts[0])
    c1 = og.state()[2].copy()
    og.updateStates(*parts[1])
    c2 = og.state()[2]
    crossing = int(((c1 <= 100) & (c1 > 0) & (c2 > 100)).sum())
    print(f"voxels crossing 100 in the second call: {crossing}; above 100 after the first: {(c1 > 100).sum()}")
    assert crossing >= 5


def test_oracle_skips_nan_points(oracle):
    """What the oracle does with a NaN coordinate (its int conversion gives INT_MIN: no voxel):
    the NaN points and the normals at NaN positions leave no trace in the state."""
    cloud, normals = _edge_inputs()["nan_points"]
    ok_c, ok_n = ~np.isnan(cloud).any(1), ~np.isnan(normals[:, :3]).any(1)
    assert (~ok_c).sum() == 4 and (~ok_n).sum() == 4
    a = _setup(oracle.OccupancyGrid(), 1, DENSE_RES, DENSE_BOUNDS)
    b = _setup(oracle.OccupancyGrid(), 1, DENSE_RES, DENSE_BOUNDS)
    a.updateStates(cloud, normals)
    b.updateStates(cloud[ok_c], normals[ok_n])
    assert _states_equal(a, b) and (a.state()[3] & 1).sum() > 100


# ============================================================================ GPU

def _pair(oracle, bounds, res, k=0):
    import dmf_amd
    return _setup(oracle.OccupancyGrid(), k, res, bounds), _setup(dmf_amd.OccupancyGrid(), k, res, bounds)


@pytest.mark.gpu
@pytest.mark.parametrize("grid", range(len(_REORG_GRIDS)))
@pytest.mark.parametrize("clean", [False, True])
def test_forced_fallback_adversarial(oracle, grid, clean):
    """Round cap 1: k_og_reorg_serial produces the download (reorg_rounds == -1), bit for bit."""
    bounds, res = _REORG_GRIDS[grid]
    og, gg = _pair(oracle, bounds, res)
    assert gg.reorg_rounds == 0
    gg.set_reorg_round_cap(1)
    for seed in range(4):
        st = _adversarial_state(og.dims, bounds, np.float32(res), 100 + seed)
        og.set_state(*st)
        gg.set_state(*st)
        exp = og.downloadReorganizedCloud(clean)
        assert exp.shape[0] > 10 and _same(gg.downloadReorganizedCloud(clean), exp)
        assert gg.reorg_rounds == -1


@pytest.mark.gpu
@pytest.mark.parametrize("case", CHAINS)
@pytest.mark.parametrize("clean", [False, True])
def test_forced_fallback_chain(oracle, case, clean):
    gi, seed, _ = case
    bounds, res = R.CHAIN_GRIDS[gi]
    og, gg = _pair(oracle, bounds, res)
    gg.set_reorg_round_cap(1)
    st = _chain(gi, seed, clean)
    og.set_state(*st)
    gg.set_state(*st)
    exp = og.downloadReorganizedCloud(clean)
    assert exp.shape[0] > 100 and _same(gg.downloadReorganizedCloud(clean), exp)
    assert gg.reorg_rounds == -1


@pytest.mark.gpu
@pytest.mark.parametrize("case", DEEP)
@pytest.mark.parametrize("clean", [False, True])
def test_deep_fixed_point(oracle, case, clean):
    """Default cap, 36..49 rounds: the fixed point itself, never the fallback."""
    gi, seed, rounds = case
    bounds, res = R.CHAIN_GRIDS[gi]
    og, gg = _pair(oracle, bounds, res)
    st = _chain(gi, seed, clean)
    og.set_state(*st)
    gg.set_state(*st)
    exp = og.downloadReorganizedCloud(clean)
    assert exp.shape[0] > 100 and _same(gg.downloadReorganizedCloud(clean), exp)
    print(f"grid {gi} seed {seed} clean {clean}: reorg_rounds {gg.reorg_rounds}, emulated {rounds}")
    assert gg.reorg_rounds >= 2
    assert 30 <= gg.reorg_rounds <= 60


@pytest.mark.gpu
@pytest.mark.parametrize("clean", [False, True])
def test_round_cap_boundary(oracle, clean):
    """States of exactly 64 and 65 rounds and one of 75 under the default cap of 64; the last under cap 200."""
    for case in (AT_64, AT_65, OVER):
        gi, seed, rounds = case
        bounds, res = R.CHAIN_GRIDS[gi]
        og, gg = _pair(oracle, bounds, res)
        st = _chain(gi, seed, clean)
        og.set_state(*st)
        gg.set_state(*st)
        exp = og.downloadReorganizedCloud(clean)
        assert _same(gg.downloadReorganizedCloud(clean), exp)
        print(f"{rounds}-round state, clean {clean}: reorg_rounds {gg.reorg_rounds}")
        if case is OVER:
            assert gg.reorg_rounds == -1
            gg.set_reorg_round_cap(200)
            assert _same(gg.downloadReorganizedCloud(clean), exp)
            print(f"  cap 200: reorg_rounds {gg.reorg_rounds}")
            assert gg.reorg_rounds != -1 and gg.reorg_rounds > 64
            gg.set_reorg_round_cap(0)  # back to the default
            assert _same(gg.downloadReorganizedCloud(clean), exp) and gg.reorg_rounds == -1
        else:
            assert gg.reorg_rounds in (rounds, -1)


@pytest.mark.gpu
def test_round_cap_range_and_setup(oracle):
    import dmf_amd
    from dmf_amd import _lib
    bounds, res = R.CHAIN_GRIDS[0]
    gg = _setup(dmf_amd.OccupancyGrid(), 0, res, bounds)
    for bad in (-1, 65537, 1 << 20):
        assert gg._L.dmf_ogrid_set_reorg_round_cap(gg._h, bad) == _lib.DMF_ERR_RANGE
    for ok in (1, 65536, 0, 1):
        gg.set_reorg_round_cap(ok)
    _setup(gg, 0, res, bounds)  # the cap (1) survives dmf_ogrid_setup
    st = _chain(*DEEP[0][:2], False)
    gg.set_state(*st)
    og = _setup(oracle.OccupancyGrid(), 0, res, bounds)
    og.set_state(*st)
    assert _same(gg.downloadReorganizedCloud(False), og.downloadReorganizedCloud(False)) and gg.reorg_rounds == -1


@pytest.mark.gpu
@pytest.mark.parametrize("clean", [False, True])
def test_one_grid_across_paths(oracle, clean):
    """Fallback, then a shallow state through the fixed point, then the fallback again on ONE grid
    object: stale scratch (P0 / P1, keys) or occ left by the other path would show."""
    bounds, res = R.CHAIN_GRIDS[0]
    og, gg = _pair(oracle, bounds, res)
    deep = _chain(*OVER_SMALL[:2], clean)  # 73 rounds: over the default cap
    shallow = _adversarial_state(og.dims, bounds, np.float32(res), 100)
    seen = []
    for st in (deep, shallow, deep, shallow):
        og.set_state(*st)
        gg.set_state(*st)
        exp = og.downloadReorganizedCloud(clean)
        assert exp.shape[0] > 10 and _same(gg.downloadReorganizedCloud(clean), exp)
        seen.append(gg.reorg_rounds)
    assert seen[0] == -1 and seen[2] == -1 and 2 <= seen[1] <= 4 and seen[3] == seen[1]


@pytest.mark.gpu
@pytest.mark.parametrize("k", [0, 1, 2])
def test_dense_update_states(oracle, k):
    """Counts past 100 on real updateStates data: HQ, clean reorganization, long event runs."""
    import dmf_amd
    cloud, normals = _dense_input()
    state, dl = _dense_oracle(k)
    gg = _setup(dmf_amd.OccupancyGrid(), k, DENSE_RES, DENSE_BOUNDS)
    gg.updateStates(cloud, normals)
    for a, b in zip(state, gg.state()):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    got = _gpu_downloads(gg)
    assert len(got[1]) >= 10 and len(got[3]) >= 10
    for g, e in zip(got, dl):
        assert _same(g, e)


@pytest.mark.gpu
def test_dense_split_calls(oracle):
    og, gg = _pair(oracle, DENSE_BOUNDS, DENSE_RES)
    for part in _split():
        og.updateStates(*part)
        gg.updateStates(*part)
        assert _states_equal(og, gg)
        assert _same(gg.downloadHQCloud(), og.download(1))
    assert len(gg.downloadHQCloud()) >= 10
    assert _same(gg.downloadReorganizedCloud(True), og.downloadReorganizedCloud(True))


@pytest.mark.gpu
@pytest.mark.parametrize("clean", [False, True])
def test_dense_forced_fallback_after_update_states(oracle, clean):
    import dmf_amd
    cloud, normals = _dense_input(SMALL_RES)
    state, dl = _dense_oracle(1, SMALL_RES)
    gg = _setup(dmf_amd.OccupancyGrid(), 1, SMALL_RES, DENSE_BOUNDS)
    assert max(gg.dims) <= 48
    gg.updateStates(cloud, normals)
    for a, b in zip(state, gg.state()):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    gg.set_reorg_round_cap(1)
    exp = dl[3 if clean else 2]
    assert len(exp) >= 10 and _same(gg.downloadReorganizedCloud(clean), exp)
    assert gg.reorg_rounds == -1


def _edge_inputs():
    """name -> (cloud, normals) of the input edges, on the 8 mm grid (K = 1)."""
    cloud, normals = _inputs(seed=41, n=1500)
    lo, hi = np.array(DENSE_BOUNDS[0::2]), np.array(DENSE_BOUNDS[1::2])
    nan = np.float32(np.nan)
    lo32 = lo.astype(np.float32)  # the float nearest to min: on it or one step outside
    on_min = np.where(lo32.astype(np.float64) < lo, np.nextafter(lo32, np.float32(1)), lo32)
    below = np.nextafter(hi.astype(np.float32), np.float32(-1))
    end = lo + np.array(R.grid_dims(DENSE_BOUNDS, DENSE_RES)) * np.float64(np.float32(DENSE_RES[0]))  # the last cell's end
    last = np.nextafter(end.astype(np.float32), np.float32(-1))
    edge_pts = np.array([lo32, on_min, below, last, [on_min[0], 0.0, last[2]], [5.0, 5.0, 5.0], [-1e30, 0.0, 0.0],
                         [0.0, 3e38, 0.0], hi, end, [0.1, 0.1, np.inf]], np.float32)
    edge_nrm = np.concatenate([edge_pts, np.tile(np.array([[0, 0, 1]], np.float32), (len(edge_pts), 1))], axis=1)
    nan_pts = np.array([[nan, 0.1, 0.1], [0.1, nan, 0.1], [0.1, 0.1, nan], [nan, nan, nan]], np.float32)
    nan_pn = np.concatenate([nan_pts, np.tile(np.array([[1, 0, 0]], np.float32), (4, 1))], axis=1)
    nan_normals = normals[:6].copy()
    nan_normals[0, 3] = nan
    nan_normals[1, 3:] = nan
    dup = np.repeat(cloud[:3], 300, axis=0)
    dupn = np.repeat(normals[:3], 300, axis=0)
    return {
        "more_points_than_normals": (cloud, normals[:700]),
        "more_normals_than_points": (cloud[:700], normals),
        "no_points": (cloud[:0], normals),
        "no_normals": (cloud, normals[:0]),
        "nothing": (cloud[:0], normals[:0]),
        "nan_points": (np.concatenate([cloud[:500], nan_pts, cloud[500:]]),
                       np.concatenate([normals[:200], nan_pn, normals[200:]])),
        "nan_normals": (cloud, np.concatenate([nan_normals, normals])),
        "on_min_below_max_outside": (np.concatenate([edge_pts, cloud]), np.concatenate([edge_nrm, normals])),
        "duplicates": (np.concatenate([cloud[:200], dup]), np.concatenate([normals[:200], dupn])),
    }


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["more_points_than_normals", "more_normals_than_points", "no_points", "no_normals",
                                  "nothing", "nan_points", "nan_normals", "on_min_below_max_outside", "duplicates"])
def test_update_states_input_edges(oracle, name):
    cloud, normals = _edge_inputs()[name]
    og, gg = _pair(oracle, DENSE_BOUNDS, DENSE_RES, 1)
    base = _inputs(seed=42, n=500)  # a first call, so that the edge input meets existing state
    for c, n in (base, (cloud, normals)):
        og.updateStates(c, n)
        gg.updateStates(c, n)
    assert _states_equal(og, gg)
    assert (og.state()[3] & 1).sum() > 100
    assert _same(gg.downloadCloud(), og.download(0))
    assert _same(gg.downloadReorganizedCloud(False), og.downloadReorganizedCloud(False))


@pytest.mark.gpu
def test_update_states_device_on_torch_stream(oracle):
    """dmf_ogrid_update_states_device over torch tensors on a non-default torch stream given to
    dmf_ogrid_set_stream; dmf_ogrid_state follows with no synchronisation in between."""
    import torch
    import dmf_amd
    from dmf_amd import _lib
    cloud, normals = _dense_input()
    parts = [(cloud[:4000], normals[:3500]), (cloud[4000:], normals[3500:])]
    host = _setup(dmf_amd.OccupancyGrid(), 1, DENSE_RES, DENSE_BOUNDS)
    for c, n in parts:
        host.updateStates(c, n)
    og = _setup(oracle.OccupancyGrid(), 1, DENSE_RES, DENSE_BOUNDS)
    for c, n in parts:
        og.updateStates(c, n)
    gg = _setup(dmf_amd.OccupancyGrid(), 1, DENSE_RES, DENSE_BOUNDS)
    s = torch.cuda.Stream()
    try:
        _lib.check(gg._L.dmf_ogrid_set_stream(gg._h, C.c_void_p(s.cuda_stream)))
        with torch.cuda.stream(s):
            for c, n in parts:
                dc = torch.from_numpy(c).pin_memory().to("cuda", non_blocking=True)
                dn = torch.from_numpy(n).pin_memory().to("cuda", non_blocking=True)
                _lib.check(gg._L.dmf_ogrid_update_states_device(gg._h, dc.data_ptr(), c.shape[0], dn.data_ptr(),
                                                                n.shape[0]))
        got = gg.state()
        dl = gg.downloadHQCloud()
    finally:
        s.synchronize()
        gg._L.dmf_ogrid_set_stream(gg._h, None)
    for a, b, c in zip(got, host.state(), og.state()):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)) and np.array_equal(a.view(np.uint8), c.view(np.uint8))
    assert len(dl) >= 10 and _same(dl, og.download(1))
    gg.close()


@pytest.mark.gpu
def test_download_capacity_contract(oracle):
    import dmf_amd
    from dmf_amd import _lib
    bounds, res = _REORG_GRIDS[0]
    og, gg = _pair(oracle, bounds, res)
    st = _adversarial_state(og.dims, bounds, np.float32(res), 100)
    og.set_state(*st)
    gg.set_state(*st)
    L, h = gg._L, gg._h
    for mode, exp in ((0, og.download(0)), (1, og.download(1)), (2, og.downloadReorganizedCloud(False)),
                      (3, og.downloadReorganizedCloud(True))):
        full = exp.shape[0]
        assert full > 5
        guard = np.float32(-77.0)
        for cap, with_buf in ((0, False), (0, True), (full - 1, True)):
            buf = np.full(6 * full + 6, guard, np.float32)
            n = C.c_int64(-1)
            assert L.dmf_ogrid_download(h, mode, buf.ctypes.data if with_buf else None, cap,
                                        C.addressof(n)) == _lib.DMF_ERR_CAPACITY
            assert n.value == full and np.all(buf == guard)
        buf = np.full(6 * full + 6, guard, np.float32)
        n = C.c_int64(-1)
        assert L.dmf_ogrid_download(h, mode, buf.ctypes.data, full, C.addressof(n)) == 0 and n.value == full
        assert _same(buf[:6 * full].reshape(-1, 6), exp) and np.all(buf[6 * full:] == guard)
    n = C.c_int64(-1)
    buf = np.zeros(6, np.float32)
    for mode in (4, -1):
        assert L.dmf_ogrid_download(h, mode, buf.ctypes.data, 1, C.addressof(n)) == _lib.DMF_ERR_INVALID
    assert L.dmf_ogrid_download(h, 0, buf.ctypes.data, 1, None) == _lib.DMF_ERR_INVALID
    fresh = dmf_amd.OccupancyGrid()  # never set up
    assert L.dmf_ogrid_download(fresh._h, 0, buf.ctypes.data, 1, C.addressof(n)) == _lib.DMF_ERR_STATE
    r = C.c_int32(-5)
    assert L.dmf_ogrid_reorg_rounds(fresh._h, C.addressof(r)) == 0 and r.value == 0


@pytest.mark.gpu
def test_cpp_dropin_downloads(tmp_path, oracle):
    """compat/OccupancyGrid.hpp executed (compat/examples/ogrid_headless.cpp): updateStates of the
    dense input and the four downloads equal the oracle's."""
    assert os.path.exists(DRIVER), "build the driver: make -C depth-map-fusion-utils_amd"
    cloud, normals = _dense_input()
    k = 1
    _, dl = _dense_oracle(k)
    cloud.tofile(tmp_path / "cloud.bin")
    normals.tofile(tmp_path / "normals.bin")
    args = [repr(float(b)) for b in DENSE_BOUNDS] + [repr(float(np.float32(r))) for r in DENSE_RES]
    out = subprocess.run([DRIVER, str(tmp_path / "cloud.bin"), str(tmp_path / "normals.bin")] + args +
                         [str(k), str(tmp_path / "out")], check=True, capture_output=True, text=True, timeout=300).stdout
    dims = R.grid_dims(DENSE_BOUNDS, DENSE_RES)
    assert out.splitlines()[0].split() == ["dims"] + [str(d) for d in dims]
    for ext, exp in zip(("cloud", "hq", "reorg", "clean"), dl):
        got = np.fromfile(tmp_path / f"out.{ext}", np.float32).reshape(-1, 6)
        assert len(exp) >= 10 and _same(got, exp), ext
