"""GPU: the travel field, the path back and the travel cost map (csrc/dmf_travel.hip)
against the numpy restatement tests/travel_ref.py -- exact equality on every cell, every path cell,
every cost-map entry and the three counters, through the host form, the device form and the Python
method.  Device outputs are pre-filled with a value that is never a result and carry guard entries
after the end (an unwritten or overwritten entry shows).  The distance fields of the named cases are
built in numpy, so a failure points at the travel field and not at distance_field."""
import ctypes as C

import numpy as np
import pytest

import distance_ref as DR
import helpers as Hh
import travel_ref as TR

pytestmark = pytest.mark.gpu

FILL = np.uint32(0xFFFFFFFE)              # neither a hop count (< 2^31) nor DMF_NO_PATH
FILL_COUNT = np.uint64(1 << 63)
FILL_CELL = np.int32(-77)
GUARD = 5                                  # entries kept after the end


def _seed_ptr(seeds):
    return seeds.ctypes.data if seeds.shape[0] else None


def _host(gv, d2, radius2, seeds):
    """dmf_grid_travel -> (status, info[4] (the last a guard), hops flat)."""
    flat = np.ascontiguousarray(d2, np.uint32).reshape(-1)
    seeds = np.ascontiguousarray(seeds, np.int32).reshape(-1, 3)
    out = np.full(flat.size, FILL, np.uint32)
    info = np.full(4, FILL_COUNT, np.uint64)
    st = gv._L.dmf_grid_travel(gv._h, flat.ctypes.data, int(radius2), _seed_ptr(seeds), seeds.shape[0], out.ctypes.data,
                               info.ctypes.data)
    return st, info, out


def _device(dc, d2, radius2, seeds, d_out=None, d_info=None, info=True):
    """dmf_grid_travel_device into a pre-filled output of ncell + GUARD entries -> (info[4], hops with guard)."""
    from dmf_amd import _lib
    flat = np.ascontiguousarray(d2, np.uint32).reshape(-1)
    seeds = np.ascontiguousarray(seeds, np.int32).reshape(-1, 3)
    n = flat.size
    d_d2 = dc.upload(flat)
    d_seeds = dc.upload(seeds) if seeds.shape[0] else None
    if d_out is None:
        d_out = dc.upload(np.full(n + GUARD, FILL, np.uint32))
    if d_info is None:
        d_info = dc.upload(np.full(4, FILL_COUNT, np.uint64))
    _lib.check(dc.L.dmf_grid_travel_device(dc.h, d_d2, int(radius2), d_seeds, seeds.shape[0], d_out,
                                           d_info if info else None))
    return dc.download(d_info, 4, np.uint64), dc.download(d_out, n + GUARD, np.uint32)


def _check_all(gv, name):
    """Host form, device form and the Python method == the reference, on every cell and counter."""
    from dmf_amd import _lib
    dims, d2, radius2, seeds, ref = TR.case(name)
    n = int(np.prod(dims))
    want, tot = ref.reshape(-1), TR.TOTALS[name]
    counters = [tot[0], tot[1], tot[2], int(FILL_COUNT)]                   # three counters, not four
    st, info, out = _host(gv, d2, radius2, seeds)
    assert st == _lib.DMF_OK and info.tolist() == counters, (st, info, counters)
    assert int((out != want).sum()) == 0, "host"
    dc = Hh.DeviceCalls(gv)
    try:
        info, out = _device(dc, d2, radius2, seeds)
        assert info.tolist() == counters, (info, counters)
        assert int((out[:n] != want).sum()) == 0 and (out[n:] == FILL).all(), "device"
        info, out = _device(dc, d2, radius2, seeds, info=False)
        assert (info == FILL_COUNT).all() and np.array_equal(out[:n], want) and (out[n:] == FILL).all()
    finally:
        dc.close()
    got, cnt = gv.travel_field(d2, radius2, seeds, info=True)
    assert got.dtype == np.uint32 and got.shape == tuple(dims) and np.array_equal(got, ref)
    assert cnt == tot[:3]
    assert int(got[got != TR.NO_PATH].astype(np.int64).sum()) == tot[3]


@pytest.mark.parametrize("name", sorted(TR.CASES))
def test_named_cases(name):
    """Over (70, 37, 41) cells, 3 x 2 x 2 bricks with partial tiles on every axis: the open grid from
    either corner (hops = the Manhattan distance, 145 at most); the serpentine along x, y and z (721
    hops through 81,098 cells along x: the path re-enters every tile row many times, so a tile that
    went idle must wake again, across each face direction in turn); the percolation field (islands,
    dead ends, detours: 183 hops over a Manhattan span of 136); the sealed chamber from outside, from
    inside and from both; the corridor of a real dist2 at radius2 = 4 (its centre line only), 5
    (closed: the seed is blocked) and 0 (walls traversable); many seeds with duplicates, seeds outside
    and on blocked cells; only invalid seeds; no seed; the degenerate dims (1, 1, 1), (300, 1, 1)
    with a block in the middle, (1, 40, 33) and (33, 33, 33), whose seed is alone in its tile; and two
    grids with zdim a multiple of 4, where full rows take the 16-byte accesses."""
    dims, d2, radius2, seeds, ref = TR.case(name)
    assert TR.totals(d2, radius2, ref) == TR.TOTALS[name]
    _check_all(Hh.gpu_grid(dims, Hh.ODD_BOUNDS), name)


def test_distance_field_then_travel_field():
    """End to end on the device's own distance field: 2 % of the cells solid, a body of radius^2 = 3
    cells (every cell within sqrt(2) of a solid cell is closed) and the point body of radius^2 = 1."""
    dims = TR.DIMS
    L = np.where(np.random.default_rng(21).random(dims) < 0.02, 5, -3).astype(np.int16)
    L[:3, :3, :3] = -3
    gv = Hh.gpu_grid(dims, Hh.ODD_BOUNDS)
    d2 = gv.distance_field(L, 1)
    assert np.array_equal(d2, DR.edt2(L, dims, 1))
    seeds = np.array([[0, 0, 0]], np.int32)
    for radius2 in (1, 3):
        ref = TR.bfs(d2, radius2, seeds)
        got, cnt = gv.travel_field(d2, radius2, seeds, info=True)
        assert np.array_equal(got, ref)
        assert cnt == TR.totals(d2, radius2, ref)[:3] and 1000 < cnt[1] <= cnt[0] < L.size


@pytest.mark.parametrize("name", ["dims_24_17_40", "percolation"])
def test_unaligned_device_fields(name):
    """d_dist2 and d_hops at a base + 4 bytes (no caller owes the library 16-byte alignment): no
    16-byte access fits, the cell-by-cell loaders and stores take over; the entries before the
    fields and the guard after d_hops stay as they were, and the path walk reads the same field."""
    from dmf_amd import _lib
    dims, d2, radius2, seeds, ref = TR.case(name)
    n = int(np.prod(dims))
    gv = Hh.gpu_grid(dims, Hh.ODD_BOUNDS)
    dc = Hh.DeviceCalls(gv)
    try:
        d_d2 = dc.upload(np.concatenate([[np.uint32(0)], d2.reshape(-1)]).astype(np.uint32))   # a blocked cell before
        d_out = dc.upload(np.full(1 + n + GUARD, FILL, np.uint32))
        d_info = dc.upload(np.full(4, FILL_COUNT, np.uint64))
        d_seeds = dc.upload(seeds)
        _lib.check(dc.L.dmf_grid_travel_device(dc.h, d_d2 + 4, int(radius2), d_seeds, seeds.shape[0], d_out + 4, d_info))
        out = dc.download(d_out, 1 + n + GUARD, np.uint32)
        assert out[0] == FILL and np.array_equal(out[1:1 + n], ref.reshape(-1)) and (out[1 + n:] == FILL).all()
        assert dc.download(d_info, 4, np.uint64).tolist() == list(TR.TOTALS[name][:3]) + [int(FILL_COUNT)]
        far = TR.farthest(ref)
        want = TR.path(ref, far)
        d_cells = dc.upload(np.full((want.shape[0] + GUARD, 3), FILL_CELL, np.int32))
        d_n = dc.upload(np.full(2, FILL_COUNT, np.uint64))
        _lib.check(dc.L.dmf_grid_path_device(dc.h, d_out + 4, dc.upload(np.asarray(far, np.int32)), d_cells,
                                             want.shape[0], d_n))
        got = dc.download(d_cells, (want.shape[0] + GUARD, 3), np.int32)
        assert np.array_equal(got[:want.shape[0]], want) and (got[want.shape[0]:] == FILL_CELL).all()
        assert dc.download(d_n, 2, np.uint64).tolist() == [want.shape[0], int(FILL_COUNT)]
    finally:
        dc.close()


def test_calls_share_one_volume_and_one_output():
    """One volume, one output buffer, one counter buffer: every cell reached, then the chamber's
    inside only, then no seed at all, then the first again.  Nothing of an earlier call's field,
    lists, queued bits or counters may show; the same call twice gives the same bytes; and the
    point-cloud occupancy stays untouched."""
    n = int(np.prod(TR.DIMS))
    gv = Hh.gpu_grid(TR.DIMS, Hh.ODD_BOUNDS)
    dc = Hh.DeviceCalls(gv)
    try:
        d_out = dc.upload(np.full(n + GUARD, FILL, np.uint32))
        d_info = dc.upload(np.full(4, FILL_COUNT, np.uint64))
        first = None
        for name in ("open_lo", "sealed_in", "seeds_none", "percolation", "open_lo"):
            _, d2, radius2, seeds, ref = TR.case(name)
            info, out = _device(dc, d2, radius2, seeds, d_out, d_info)
            assert info.tolist() == list(TR.TOTALS[name][:3]) + [int(FILL_COUNT)], name
            assert np.array_equal(out[:n], ref.reshape(-1)) and (out[n:] == FILL).all(), name
            if name == "open_lo":
                assert first is None or first == out.tobytes()
                first = out.tobytes()
    finally:
        dc.close()
    assert gv.info()["num_occupied"] == 0


def _targets(name):
    """The farthest cell, a seed, a blocked or unreached cell, two cells outside the grid, and a few more."""
    _, d2, radius2, seeds, hops = TR.case(name)
    reach = np.argwhere(hops != TR.NO_PATH)
    extra = reach[np.random.default_rng(3).integers(0, len(reach), 4)]
    seed = tuple(TR.valid_seeds(TR.traversable(d2, radius2), seeds)[0])
    none = tuple(np.argwhere(hops == TR.NO_PATH)[7])
    return [TR.farthest(hops), seed, none, (-1, 3, 3), (3, 3, hops.shape[2])] + [tuple(c) for c in extra]


@pytest.mark.parametrize("name", ["serpentine_x", "percolation"])
def test_paths_host_device_python(name):
    """Equality with the reference's path, tie order included; 1 cell at a seed, 0 cells (DMF_OK) at
    an unreachable cell and outside the grid; the size query; and a capacity smaller than the path:
    DMF_ERR_CAPACITY with the need and untouched cells in the host form, the first cap cells and
    nothing past them in the device form."""
    from dmf_amd import _lib
    dims, _, _, _, hops = TR.case(name)
    flat = np.ascontiguousarray(hops).reshape(-1)
    gv = Hh.gpu_grid(dims, Hh.ODD_BOUNDS)
    dc = Hh.DeviceCalls(gv)
    try:
        d_hops = dc.upload(flat)
        for t in _targets(name):
            want = TR.path(hops, t)
            m = want.shape[0]
            tgt = np.asarray(t, np.int32)
            got = gv.path_to(hops, t)
            assert got.dtype == np.int32 and got.shape == (m, 3) and np.array_equal(got, want), t
            n = C.c_int64(-1)
            assert gv._L.dmf_grid_path(gv._h, flat.ctypes.data, tgt.ctypes.data, None, 0, C.addressof(n)) == _lib.DMF_OK
            assert n.value == m, t
            cells = np.full((m + GUARD, 3), FILL_CELL, np.int32)
            st = gv._L.dmf_grid_path(gv._h, flat.ctypes.data, tgt.ctypes.data, cells.ctypes.data, m + 2, C.addressof(n))
            assert st == _lib.DMF_OK and n.value == m and np.array_equal(cells[:m], want) and (cells[m:] == FILL_CELL).all()
            for cap in sorted({0, 1, m // 2, m - 1} - {m, -1}):          # smaller than the path
                if m == 0:
                    continue
                cells[:] = FILL_CELL
                st = gv._L.dmf_grid_path(gv._h, flat.ctypes.data, tgt.ctypes.data, cells.ctypes.data, cap, C.addressof(n))
                assert st == _lib.DMF_ERR_CAPACITY and n.value == m and (cells == FILL_CELL).all(), (t, cap)
            d_t = dc.upload(tgt)
            for cap in sorted({m + 2, m, m // 2, 1, 0}):
                d_cells = dc.upload(np.full((cap + GUARD, 3), FILL_CELL, np.int32))
                d_n = dc.upload(np.full(2, FILL_COUNT, np.uint64))
                _lib.check(dc.L.dmf_grid_path_device(dc.h, d_hops, d_t, d_cells, cap, d_n))
                out = dc.download(d_cells, (cap + GUARD, 3), np.int32)
                k = min(cap, m)
                assert dc.download(d_n, 2, np.uint64).tolist() == [m, int(FILL_COUNT)], (t, cap)
                assert np.array_equal(out[:k], want[:k]) and (out[k:] == FILL_CELL).all(), (t, cap)
    finally:
        dc.close()


def test_path_walk_ends_on_a_field_no_travel_call_made():
    """All cells 9 but a short descending chain: the walk follows it and stops where no neighbour
    holds k - 1; a constant field gives the target alone."""
    dims = (9, 8, 7)
    gv = Hh.gpu_grid(dims, Hh.ODD_BOUNDS)
    odd = np.full(dims, 9, np.uint32)
    odd[1, 1, 1], odd[1, 1, 2] = 8, 7
    assert np.array_equal(gv.path_to(odd, (2, 1, 1)), TR.path(odd, (2, 1, 1)))
    assert gv.path_to(odd, (2, 1, 1)).tolist() == [[2, 1, 1], [1, 1, 1], [1, 1, 2]]
    flat = np.full(dims, 5, np.uint32)
    assert gv.path_to(flat, (4, 4, 4)).tolist() == [[4, 4, 4]]


def test_travel_cost_map():
    """Six cells of the percolation field, one on an island and one blocked: the map equals the
    reference, is symmetric, has a zero diagonal on traversable cells and INT_MAX where there is
    no path."""
    dims, d2, radius2, _, _ = TR.case("percolation")
    cells = TR.cost_cells()
    want = TR.cost_map(d2, radius2, cells)
    gv = Hh.gpu_grid(dims, Hh.ODD_BOUNDS)
    got = gv.travel_cost_map(d2, radius2, cells)
    assert got.dtype == np.int32 and got.shape == (6, 6) and np.array_equal(got, want)
    assert np.array_equal(got, got.T) and np.diag(got).tolist() == [0, 0, 0, 0, 0, TR.INT_MAX]
    assert (got[4, :4] == TR.INT_MAX).all() and (got[5] == TR.INT_MAX).all() and (got[:4, :4] < TR.INT_MAX).all()
    outside = np.concatenate([cells[:2], [[70, 0, 0]]]).astype(np.int32)
    assert np.array_equal(gv.travel_cost_map(d2, radius2, outside), TR.cost_map(d2, radius2, outside))
    assert gv.travel_cost_map(d2, radius2, np.zeros((0, 3), np.int32)).shape == (0, 0)
    assert gv.info()["num_occupied"] == 0


def test_status_rules_and_python_validation():
    import dmf_amd
    from dmf_amd import _lib
    big = Hh.gpu_grid((2049, 1, 1), Hh.ODD_BOUNDS)
    d2, out = np.full(2049, 1, np.uint32), np.full(2049, FILL, np.uint32)
    seeds, tgt = np.zeros((1, 3), np.int32), np.zeros(3, np.int32)
    cells, n = np.full((4, 3), FILL_CELL, np.int32), C.c_int64(-3)
    travel_args = (d2.ctypes.data, 1, seeds.ctypes.data, 1, out.ctypes.data, None)
    path_args = (out.ctypes.data, tgt.ctypes.data, cells.ctypes.data, 4, C.addressof(n))
    assert big._L.dmf_grid_travel(big._h, *travel_args) == _lib.DMF_ERR_RANGE
    assert big._L.dmf_grid_travel_device(big._h, *travel_args) == _lib.DMF_ERR_RANGE
    assert big._L.dmf_grid_path(big._h, *path_args) == _lib.DMF_ERR_RANGE
    assert big._L.dmf_grid_path_device(big._h, *path_args) == _lib.DMF_ERR_RANGE
    raw = dmf_amd.VoxelVolume()
    assert raw._L.dmf_grid_travel(raw._h, *travel_args) == _lib.DMF_ERR_STATE
    assert raw._L.dmf_grid_travel_device(raw._h, *travel_args) == _lib.DMF_ERR_STATE
    assert raw._L.dmf_grid_path(raw._h, *path_args) == _lib.DMF_ERR_STATE
    assert raw._L.dmf_grid_path_device(raw._h, *path_args) == _lib.DMF_ERR_STATE
    assert (out == FILL).all() and (cells == FILL_CELL).all() and n.value == -3
    gv = Hh.gpu_grid((9, 8, 7), Hh.ODD_BOUNDS)
    assert gv._L.dmf_grid_travel(gv._h, d2.ctypes.data, 1, None, 1, out.ctypes.data, None) == _lib.DMF_ERR_INVALID
    assert gv._L.dmf_grid_travel(gv._h, d2.ctypes.data, 1, seeds.ctypes.data, -1, out.ctypes.data, None) == _lib.DMF_ERR_INVALID
    assert gv._L.dmf_grid_path(gv._h, out.ctypes.data, tgt.ctypes.data, cells.ctypes.data, -1,
                               C.addressof(n)) == _lib.DMF_ERR_INVALID
    assert (out == FILL).all()
    free = np.full((9, 8, 7), TR.NO_DIST, np.uint32)
    hops = gv.travel_field(free, 1, [(0, 0, 0)])
    x, y, z = np.meshgrid(np.arange(9), np.arange(8), np.arange(7), indexing="ij")
    assert hops.dtype == np.uint32 and np.array_equal(hops, (x + y + z).astype(np.uint32))
    st = np.zeros(4, np.uint64)
    _lib.check(gv._L.dmf_grid_travel_stats(gv._h, st.ctypes.data))
    # two tiles: the seed's, its neighbour, and the seed's once more; launched in batches, plus three passes
    assert 2 <= st[0] <= 3 and st[0] + 3 <= st[1] <= 64 + 3
    assert (gv.travel_field(free, 1, np.zeros((0, 3), np.int32)) == dmf_amd.NO_PATH).all()
    assert gv.travel_field(free.reshape(-1), 1, np.array([[8, 7, 6]], np.int64))[0, 0, 0] == 21
    for bad in (lambda: gv.travel_field(free.astype(np.int32), 1, seeds),
                lambda: gv.travel_field(free.reshape(-1)[:-1], 1, seeds),
                lambda: gv.travel_field(free, 1, np.zeros(3, np.int32)),
                lambda: gv.travel_field(free, 1, np.zeros((2, 2), np.int32)),
                lambda: gv.travel_field(free, 1, np.zeros((1, 3), np.float32)),
                lambda: gv.travel_field(free, -1, seeds),
                lambda: gv.path_to(hops.astype(np.int64), (0, 0, 0)),
                lambda: gv.path_to(hops.reshape(-1)[:-1], (0, 0, 0)),
                lambda: gv.path_to(hops, (0, 0)),
                lambda: gv.path_to(hops, np.zeros((1, 3), np.int32)),
                lambda: gv.travel_cost_map(free.astype(np.int32), 1, seeds),
                lambda: gv.travel_cost_map(free, 1, np.zeros(3, np.int32)),
                lambda: gv.travel_cost_map(free, 1, np.zeros((2, 3), np.float32))):
        with pytest.raises(ValueError):
            bad()
    p = gv.path_to(hops, (2, 1, 0))
    assert p.dtype == np.int32 and p.tolist() == [[2, 1, 0], [1, 1, 0], [0, 1, 0], [0, 0, 0]]
    assert gv.path_to(hops, (9, 0, 0)).shape == (0, 3)
