"""CPU: the travel field's ABI surface and self-checks of its numpy restatement
(tests/travel_ref.py).  No GPU: the entry points are only asked to refuse bad plain arguments, which
they do before they touch the volume."""
import collections
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import travel_ref as TR

NAMES = ("dmf_grid_travel", "dmf_grid_travel_device", "dmf_grid_path", "dmf_grid_path_device")
# the cases on which the plain queue search runs (a Python loop over every reached cell)
QUEUE_CASES = ("percolation", "serpentine_y", "sealed_both", "seeds_many", "seeds_invalid", "radius_4", "radius_0",
               "dims_1_1_1", "dims_300_1_1", "dims_1_40_33", "dims_33_33_33")


def test_symbols_declared_and_exported():
    from dmf_amd import _lib
    L = _lib.load()
    syms = _lib.declared_symbols()
    for n in NAMES + ("dmf_grid_travel_stats",):
        assert n in syms and n in _lib.SIGNATURES and hasattr(L, n), n
    import dmf_amd
    for m in ("travel_field", "path_to", "travel_cost_map"):
        assert callable(getattr(dmf_amd.VoxelVolume, m)), m
    assert dmf_amd.NO_PATH == TR.NO_PATH == 2 ** 32 - 1 and dmf_amd.NO_PATH.dtype == np.uint32
    assert "#define DMF_NO_PATH UINT32_MAX" in open(_lib.HEADER_PATH).read()
    assert L.dmf_abi_version() == 1


def test_plain_arguments_rejected_without_gpu():
    """Null pointers, a negative seed count, null seeds with a positive count, a negative capacity
    and null cells with a positive capacity are DMF_ERR_INVALID.  These checks precede any access
    to the volume, so a zeroed stand-in buffer serves as the non-null handle; once they pass, the
    stand-in's `constructed` = 0 gives DMF_ERR_STATE.  Pre-filled outputs stay as they were."""
    from dmf_amd import _lib
    L = _lib.load()
    fake = C.create_string_buffer(1 << 16)
    v = C.addressof(fake)
    d2, hops, info = np.full(8, 1, np.uint32), np.full(8, 77, np.uint32), np.full(3, 9, np.uint64)
    seeds, cells, tgt = np.zeros((2, 3), np.int32), np.full((4, 3), 55, np.int32), np.zeros(3, np.int32)
    n = np.full(1, 33, np.uint64)
    pd, ph, pi, ps, pc, pt, pn = (a.ctypes.data for a in (d2, hops, info, seeds, cells, tgt, n))
    INV, STATE = _lib.DMF_ERR_INVALID, _lib.DMF_ERR_STATE
    for travel in (L.dmf_grid_travel, L.dmf_grid_travel_device):
        assert travel(None, pd, 1, ps, 2, ph, pi) == INV
        assert travel(v, None, 1, ps, 2, ph, pi) == INV
        assert travel(v, pd, 1, ps, 2, None, pi) == INV
        assert travel(v, pd, 1, None, 2, ph, pi) == INV
        assert travel(v, pd, 1, ps, -1, ph, pi) == INV
        assert travel(v, pd, 1, None, -2 ** 63, ph, None) == INV
        assert travel(v, pd, 1, ps, 2, ph, None) == STATE
        assert travel(v, pd, 1, None, 0, ph, None) == STATE       # no seeds is a call like any other
    assert b"" != L.dmf_last_error()
    for path in (L.dmf_grid_path, L.dmf_grid_path_device):
        assert path(None, ph, pt, pc, 4, pn) == INV
        assert path(v, None, pt, pc, 4, pn) == INV
        assert path(v, ph, None, pc, 4, pn) == INV
        assert path(v, ph, pt, pc, 4, None) == INV
        assert path(v, ph, pt, None, 4, pn) == INV
        assert path(v, ph, pt, pc, -1, pn) == INV
        assert path(v, ph, pt, pc, 4, pn) == STATE
        assert path(v, ph, pt, None, 0, pn) == STATE
    assert (hops == 77).all() and (info == 9).all() and (cells == 55).all() and n[0] == 33


def test_compat_travel_compiles(tmp_path):
    """travelField / pathTo in compat/Volume.hpp and travelCostMap in compat/PathPlanning.hpp (g++
    -fsyntax-only against the headless shims)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    compat = os.path.join(root, "depth-map-fusion-utils_amd", "compat")
    src = tmp_path / "travel.cpp"
    src.write_text('''
#include "Camera.hpp"
#include "PathPlanning.hpp"
#include "RayTracingEngine.hpp"
#include "Volume.hpp"
int main() {
  VoxelVolume v;
  v.setDimensions(-0.5, 0.5, -0.5, 0.5, -0.5, 0.5);
  v.setVolumeSize(8, 8, 8);
  v.constructVolume();
  const std::vector<uint32_t> d2(512, DMF_NO_DIST);
  std::vector<uint32_t> hops;
  const std::vector<std::array<int32_t, 3>> seeds = {{{0, 0, 0}}, {{7, 7, 7}}};
  const std::array<uint64_t, 3> info = v.travelField(d2, 4, seeds, hops);
  const std::vector<std::array<int32_t, 3>> path = v.pathTo(hops, {{3, 3, 3}});
  const std::vector<std::vector<int>> map = PathPlanning::travelCostMap(v, d2, 4, seeds);
  return (int)(info[1] + path.size() + map.size()) + (hops[0] == DMF_NO_PATH);
}
''')
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    r = subprocess.run([gxx, "-std=c++17", "-fsyntax-only", "-Wall", "-I", compat, "-I", os.path.join(compat, "shims"),
                        "-I", os.path.join(root, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


# ---------------------------------------------------------------- the restatement's self-checks
def _queue_bfs(trav, seeds):
    """The textbook search: a queue of cells, no arrays shifted."""
    nx, ny, nz = trav.shape
    hops = np.full(trav.shape, TR.NO_PATH, np.uint32)
    q = collections.deque()
    for s in seeds:
        c = tuple(int(v) for v in s)
        if 0 <= c[0] < nx and 0 <= c[1] < ny and 0 <= c[2] < nz and trav[c] and hops[c] == TR.NO_PATH:
            hops[c] = 0
            q.append(c)
    while q:
        x, y, z = q.popleft()
        k = int(hops[x, y, z]) + 1
        for c in ((x + 1, y, z), (x - 1, y, z), (x, y + 1, z), (x, y - 1, z), (x, y, z + 1), (x, y, z - 1)):
            if 0 <= c[0] < nx and 0 <= c[1] < ny and 0 <= c[2] < nz and trav[c] and hops[c] == TR.NO_PATH:
                hops[c] = k
                q.append(c)
    return hops


def test_cases_and_totals_are_one_list():
    assert set(TR.CASES) == set(TR.TOTALS) and set(QUEUE_CASES) <= set(TR.CASES)


@pytest.mark.parametrize("name", sorted(TR.CASES))
def test_reference_pinned_totals(name):
    dims, d2, radius2, seeds, hops = TR.case(name)
    assert hops.shape == tuple(dims) and hops.dtype == np.uint32
    assert TR.totals(d2, radius2, hops) == TR.TOTALS[name]
    trav = TR.traversable(d2, radius2)
    assert (hops[~trav] == TR.NO_PATH).all()
    valid = TR.valid_seeds(trav, seeds)
    assert np.array_equal(np.argwhere(hops == 0), np.unique(valid, axis=0).reshape(-1, 3))
    # every reached cell but a seed has a face neighbour one hop nearer, and none two hops nearer
    h = np.where(hops == TR.NO_PATH, 1 << 40, hops.astype(np.int64))
    best = np.full(dims, 1 << 40, np.int64)
    for axis in range(3):
        for sh in (1, -1):
            r = np.roll(h, sh, axis)
            edge = [slice(None)] * 3
            edge[axis] = 0 if sh == 1 else -1
            r[tuple(edge)] = 1 << 40
            np.minimum(best, r, out=best)
    reached = (hops != TR.NO_PATH) & (hops != 0)
    assert (best[reached] == h[reached] - 1).all()
    assert not (trav & (hops == TR.NO_PATH) & (best < (1 << 40))).any()      # no reachable cell left out


def test_reference_analytic_and_issue_figures():
    _, _, _, _, h = TR.case("open_lo")
    x, y, z = np.meshgrid(*(np.arange(d) for d in TR.DIMS), indexing="ij")
    assert np.array_equal(h, (x + y + z).astype(np.uint32)) and int(h.max()) == 145
    _, _, _, _, h = TR.case("open_hi")
    assert np.array_equal(h, ((69 - x) + (36 - y) + (40 - z)).astype(np.uint32))
    assert TR.TOTALS["serpentine_x"][1:3] == (81098, 721)
    assert TR.TOTALS["percolation"][:3] == (40445, 33460, 183) and 183 > 136
    # the chamber: outside and inside are two components that together are all traversable cells
    out, ins, both = (TR.TOTALS[n] for n in ("sealed_out", "sealed_in", "sealed_both"))
    assert out[1] + ins[1] == both[1] == both[0]
    inside = TR.case("sealed_in")[4] != TR.NO_PATH
    lo, hi = TR.CHAMBER_LO, TR.CHAMBER_HI
    assert inside[lo[0] + 1:hi[0], lo[1] + 1:hi[1], lo[2] + 1:hi[2]].all() and int(inside.sum()) == ins[1]
    assert not (inside & (TR.case("sealed_out")[4] != TR.NO_PATH)).any()
    # the corridor: radius2 = 4 leaves the centre line of the corridor, 5 closes it, 0 opens the walls
    d2 = TR.case("radius_4")[1]
    assert d2[0, 18, 0] == 4 and d2[0, 17, 0] == d2[0, 19, 0] == 1 and d2[0, 16, 0] == d2[0, 20, 0] == 0
    r4 = TR.case("radius_4")[4] != TR.NO_PATH
    assert r4[:, 18, :].all() and int(r4.sum()) == 70 * 41
    assert TR.TOTALS["radius_5"][1] == 0 and TR.TOTALS["radius_0"][:2] == (106190, 106190)


@pytest.mark.parametrize("name", QUEUE_CASES)
def test_reference_shift_search_equals_queue_search(name):
    _, d2, radius2, seeds, hops = TR.case(name)
    assert np.array_equal(_queue_bfs(TR.traversable(d2, radius2), seeds), hops)


@pytest.mark.parametrize("name", ["serpentine_x", "percolation", "seeds_many", "dims_300_1_1"])
def test_reference_path_properties(name):
    _, d2, radius2, seeds, hops = TR.case(name)
    far = TR.farthest(hops)
    rng = np.random.default_rng(12)
    reach = np.argwhere(hops != TR.NO_PATH)
    for t in [far] + [tuple(c) for c in reach[rng.integers(0, len(reach), 8)]]:
        p = TR.path(hops, t)
        k = int(hops[t])
        assert p.shape == (k + 1, 3) and tuple(p[0]) == tuple(t)
        assert (np.abs(np.diff(p.astype(np.int64), axis=0)).sum(axis=1) == 1).all()          # one face per step
        assert np.array_equal(hops[p[:, 0], p[:, 1], p[:, 2]], np.arange(k, -1, -1, dtype=np.uint32))
        assert hops[tuple(p[-1])] == 0 and (seeds == p[-1]).all(axis=1).any()               # ends on a seed
    s = tuple(TR.valid_seeds(TR.traversable(d2, radius2), seeds)[0])
    assert TR.path(hops, s).tolist() == [list(s)]
    assert TR.path(hops, (-1, 0, 0)).shape == (0, 3) and TR.path(hops, hops.shape).shape == (0, 3)
    blocked = np.argwhere(hops == TR.NO_PATH)
    if len(blocked):
        assert TR.path(hops, tuple(blocked[0])).shape == (0, 3)


def test_reference_path_tie_order_and_foreign_fields():
    """In the open grid from (0, 0, 0) every cell has up to three neighbours one hop nearer: the
    path takes -x while x > 0, then -y, then -z.  From the far seed it takes +x first.  A field
    that no search made ends the walk where no neighbour holds k - 1."""
    h = TR.case("open_lo")[4]
    p = TR.path(h, (5, 4, 3))
    want = [(x, 4, 3) for x in range(5, -1, -1)] + [(0, y, 3) for y in range(3, -1, -1)] + [(0, 0, z) for z in range(2, -1, -1)]
    assert p.tolist() == [list(c) for c in want]
    p = TR.path(TR.case("open_hi")[4], (66, 35, 39))
    assert p[:4].tolist() == [[66, 35, 39], [67, 35, 39], [68, 35, 39], [69, 35, 39]] and p[4].tolist() == [69, 36, 39]
    odd = np.full((4, 4, 4), 9, np.uint32)
    odd[1, 1, 1], odd[1, 1, 2] = 8, 7
    assert TR.path(odd, (2, 1, 1)).tolist() == [[2, 1, 1], [1, 1, 1], [1, 1, 2]]
    assert TR.path(np.full((3, 3, 3), 5, np.uint32), (1, 1, 1)).tolist() == [[1, 1, 1]]


def test_reference_cost_map():
    _, d2, radius2, _, hops = TR.case("percolation")
    cells = TR.cost_cells()
    m = TR.cost_map(d2, radius2, cells)
    assert m.dtype == np.int32 and m.shape == (6, 6) and np.array_equal(m, m.T)
    assert np.diag(m).tolist() == [0, 0, 0, 0, 0, TR.INT_MAX]          # the last cell is blocked
    assert (m[4, :4] == TR.INT_MAX).all() and (m[5] == TR.INT_MAX).all()  # an island, a blocked cell
    assert m[0].tolist() == [int(hops[tuple(c)]) if hops[tuple(c)] != TR.NO_PATH else TR.INT_MAX for c in cells]
    assert m[0, 3] == 183 and (m[:4, :4] < TR.INT_MAX).all()
