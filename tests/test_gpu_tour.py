"""GPU: the open tour over a cost map (csrc/dmf_tour.hip) -- nearest neighbour and
first-improvement 2-opt -- against the paths recorded from the reference's own TSPSolver.hpp
(tests/golden/tour_ref_cases.npz) and against the Python restatement tests/tour_ref.py: exact
equality of every path and every info word, through the host forms, the device forms, the Python
functions and the drop-in header's example.  Device outputs are pre-filled and carry guard entries
after the end.  Also the device form of the travel cost map, which feeds the tour."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import helpers as Hh
import tour_ref as TO

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL_PATH = np.int32(-77)
FILL_INFO = np.uint64(1 << 63)
GUARD = 5


@functools.lru_cache(maxsize=None)
def _gv():
    return Hh.gpu_grid((4, 4, 4))


def _map(kind, V):
    return TO.euclid_map(V, 1) if kind == "euclid" else TO.random_map(kind, V, 1)


@functools.lru_cache(maxsize=None)
def _ref(kind, V, start, max_rounds):
    """tour_ref on the shared map -> (nn path, forced, 2-opt path from `start`, info5); computed once."""
    m = _map(kind, V)
    nn, forced = TO.nearest_neighbour(m)
    first = {"nn": nn, "identity": list(range(V)), "perm": _perm(V)}[start]
    path, n, conv = TO.two_opt(m, first, max_rounds)
    return nn, forced, path, (forced if start == "nn" else 0, n, conv) + TO.edge_sums(m, path)


def _perm(V):
    return [0] + (1 + np.random.default_rng(V).permutation(V - 1)).tolist() if V else []


def _info(words):
    """The five uint64 info words as ints; word 3, the edge sum, is an int64 (entries may be negative)."""
    w = np.ascontiguousarray(words, np.uint64)
    return tuple(int(x) for x in w[:3]) + (int(w.view(np.int64)[3]), int(w[4]))


def _stats(gv):
    s = np.zeros(4, np.uint64)
    assert gv._L.dmf_tour_stats(gv._h, s.ctypes.data) == 0
    return [int(x) for x in s]


class Dev:
    """The device forms over one uploaded map: pre-filled path and info with guards."""

    def __init__(self, gv, m):
        self.dc, self.V = Hh.DeviceCalls(gv), m.shape[0]
        self.d_map = self.dc.upload(np.ascontiguousarray(m, np.int32)) if m.size else None

    def run(self, name, path=None, max_rounds=None, status=0):
        V, dc = self.V, self.dc
        first = np.full(V + GUARD, FILL_PATH, np.int32)
        if path is not None:
            first[:V] = path
        d_path, d_info = dc.upload(first), dc.upload(np.full(5 + GUARD, FILL_INFO, np.uint64))
        args = (dc.h, self.d_map, V, d_path if V else None) + (() if max_rounds is None else (max_rounds,)) + (d_info,)
        assert getattr(dc.L, name)(*args) == status
        got, info = dc.download(d_path, V + GUARD, np.int32), dc.download(d_info, 5 + GUARD, np.uint64)
        assert (got[V:] == FILL_PATH).all() and (info[5:] == FILL_INFO).all(), "guard"
        return got[:V].tolist(), _info(info[:5])

    def close(self):
        self.dc.close()


def test_fixture_cases_host_and_device():
    """The engine's nearest-neighbour path and 2-opt path == the reference's recorded ones."""
    import dmf_amd
    gv = _gv()
    for kind, m, nn, opt in TO.fixture_cases():
        V = m.shape[0]
        assert dmf_amd.tour_nearest_neighbour(gv, m).tolist() == nn, (kind, V, "host nn")
        assert dmf_amd.tour_two_opt(gv, m, nn).tolist() == opt, (kind, V, "host 2-opt")
        assert dmf_amd.tour(gv, m).tolist() == opt, (kind, V, "host tour")
        d = Dev(gv, m)
        try:
            assert d.run("dmf_tour_nearest_neighbour_device")[0] == nn, (kind, V, "device nn")
            assert d.run("dmf_tour_two_opt_device", nn, 0)[0] == opt, (kind, V, "device 2-opt")
            assert d.run("dmf_tour_device", None, 0)[0] == opt, (kind, V, "device tour")
        finally:
            d.close()


@pytest.mark.parametrize("V", [0, 1, 2, 3])
def test_smallest_sizes(V):
    import dmf_amd
    gv = _gv()
    for kind in ("asym", "all_nopath"):
        m = TO.random_map(kind, V, 1)
        want, winfo = TO.tour(m)
        path, info = dmf_amd.tour(gv, m, info=True)
        assert path.dtype == np.int32 and path.tolist() == want and info == winfo, (kind, info, winfo)
        nn, forced = TO.nearest_neighbour(m)
        path, info = dmf_amd.tour_nearest_neighbour(gv, m, info=True)
        assert path.tolist() == nn and info == (forced, 0, 0) + TO.edge_sums(m, nn)
        path, info = dmf_amd.tour_two_opt(gv, m, np.arange(V), info=True)
        ref = TO.two_opt(m, list(range(V)))
        assert path.tolist() == ref[0] and info == (0, ref[1], 1) + TO.edge_sums(m, ref[0])
        d = Dev(gv, m)
        try:
            assert d.run("dmf_tour_device", None, 0) == (want, winfo)
            assert d.run("dmf_tour_nearest_neighbour_device") == (nn, (forced, 0, 0) + TO.edge_sums(m, nn))
            assert d.run("dmf_tour_two_opt_device", list(range(V)), 0)[0] == ref[0]
        finally:
            d.close()


@pytest.mark.parametrize("V", [65, 257])
@pytest.mark.parametrize("kind", ["euclid", "asym", "binary", "asym_nopath", "asym_gap", "all_nopath", "minus"])
def test_against_tour_ref(kind, V):
    """V = 65 and 257 (no multiple of a wave or a workgroup): nearest neighbour, the whole tour, and
    2-opt from the identity (the reference's default path_), each with its info, host and device.
    asym_nopath: 15 % INT_MAX; the identity path holds several INT_MAX edges, more than one
    reversal mends, and stays as it is; asym_gap: the same map with one INT_MAX edge on the identity
    path, so the first candidate without any wins, whatever its sum; all_nopath: forced picks everywhere and no change; minus: entries of -1."""
    import dmf_amd
    gv, m = _gv(), _map(kind, V)
    nn, forced, opt, winfo = _ref(kind, V, "nn", 0)
    _, _, iopt, iinfo = _ref(kind, V, "identity", 0)
    if kind == "asym_nopath":
        assert TO.edge_sums(m, list(range(V)))[1] > 1 and iinfo[1] == 0 and iopt == list(range(V))
    if kind == "asym_gap":
        assert TO.edge_sums(m, list(range(V)))[1] == 1 and iinfo[4] == 0 and iinfo[1] > 1
        one = TO.two_opt(m, list(range(V)), 1)[0]                     # the first reversal: finite, and not shorter in sum
        assert TO.edge_sums(m, one)[1] == 0
    if kind == "all_nopath":
        assert forced == V - 1 and winfo[1] == 0 and opt == nn == list(range(V)) and winfo[4] == V - 1
    if kind == "minus":
        assert (m == -1).any()
    path, info = dmf_amd.tour_nearest_neighbour(gv, m, info=True)
    assert path.tolist() == nn and info == (forced, 0, 0) + TO.edge_sums(m, nn), info
    path, info = dmf_amd.tour(gv, m, info=True)
    assert path.tolist() == opt and info == winfo, (info, winfo)
    assert info[3:] == TO.edge_sums(m, path.tolist())          # a host recomputation over the returned path
    path, info = dmf_amd.tour_two_opt(gv, m, np.arange(V), info=True)
    assert path.tolist() == iopt and info == iinfo, (info, iinfo)
    d = Dev(gv, m)
    try:
        assert d.run("dmf_tour_nearest_neighbour_device") == (nn, (forced, 0, 0) + TO.edge_sums(m, nn))
        assert d.run("dmf_tour_device", None, 0) == (opt, winfo)
        assert d.run("dmf_tour_two_opt_device", list(range(V)), 0) == (iopt, iinfo)
    finally:
        d.close()


@pytest.mark.parametrize("kind", ["euclid", "asym_gap", "asym_nopath"])
def test_above_one_position_per_thread(kind):
    """V = 1025: the first size at which a thread of the one-workgroup kernels owns two positions of
    the prefix arrays (1024 threads) and the nearest-neighbour search strides twice over a row.
    Nearest neighbour, 2-opt from the identity and the whole tour, cut at 40 rounds, more than a batch (each applies
    a reversal and rebuilds the arrays), with every info word, host and device."""
    import dmf_amd
    V, cut = 1025, 40
    gv, m = _gv(), _map(kind, V)
    nn, forced, opt, winfo = _ref(kind, V, "nn", cut)
    _, _, iopt, iinfo = _ref(kind, V, "identity", cut)
    if kind == "euclid":
        assert winfo[1] == iinfo[1] == cut
    if kind == "asym_gap":
        assert iinfo[1] == cut and iinfo[4] == 0 and TO.edge_sums(m, list(range(V)))[1] == 1
    if kind == "asym_nopath":
        assert TO.edge_sums(m, list(range(V)))[1] > 1 and iinfo[1:3] == (0, 1)
    path, info = dmf_amd.tour_nearest_neighbour(gv, m, info=True)
    assert path.tolist() == nn and info == (forced, 0, 0) + TO.edge_sums(m, nn), info
    path, info = dmf_amd.tour_two_opt(gv, m, np.arange(V), max_rounds=cut, info=True)
    assert path.tolist() == iopt and info == iinfo, (info, iinfo)
    d = Dev(gv, m)
    try:
        assert d.run("dmf_tour_nearest_neighbour_device") == (nn, (forced, 0, 0) + TO.edge_sums(m, nn))
        assert d.run("dmf_tour_device", None, cut) == (opt, winfo)
        assert d.run("dmf_tour_two_opt_device", list(range(V)), cut) == (iopt, iinfo)
    finally:
        d.close()


@pytest.mark.parametrize("kind", ["euclid", "asym_gap", "binary"])
def test_from_a_random_permutation(kind):
    import dmf_amd
    V = 65
    gv, m = _gv(), _map(kind, V)
    _, _, want, winfo = _ref(kind, V, "perm", 0)
    path, info = dmf_amd.tour_two_opt(gv, m, _perm(V), info=True)
    assert path.tolist() == want and info == winfo, (info, winfo)
    d = Dev(gv, m)
    try:
        assert d.run("dmf_tour_two_opt_device", _perm(V), 0) == (want, winfo)
    finally:
        d.close()


@pytest.mark.parametrize("V", [65, 257])
@pytest.mark.parametrize("where", ["first", "last"])
def test_the_one_improving_candidate(where, V):
    """A map whose only improving candidate from the identity is the first one, (1, 2), or the
    last one, (V - 2, V - 1): one round applies exactly it; the full solve equals tour_ref's."""
    import dmf_amd
    i, k = (1, 2) if where == "first" else (V - 2, V - 1)
    gv, m = _gv(), TO.only_candidate_map(V, i, k)
    ident = list(range(V))
    path, info = dmf_amd.tour_two_opt(gv, m, ident, max_rounds=1, info=True)
    assert path.tolist() == ident[:i] + [k, i] + ident[k + 1:] and info[1:3] == (1, 0)
    total = (V - 1) * (V - 2) // 2
    assert _stats(gv)[3] == (0 if where == "first" else total - 1)     # the candidates ahead of it
    ref = TO.two_opt(m, ident)
    path, info = dmf_amd.tour_two_opt(gv, m, ident, info=True)
    assert path.tolist() == ref[0] and info == (0, ref[1], 1) + TO.edge_sums(m, ref[0])


def test_more_improvements_than_a_batch():
    """V = 257 Euclidean from the nearest-neighbour path: more improvements than the host enqueues
    between two reads of the "done" word, so the solve crosses a batch boundary."""
    import dmf_amd
    V = 257
    gv, m = _gv(), _map("euclid", V)
    _, _, opt, winfo = _ref("euclid", V, "nn", 0)
    path, info = dmf_amd.tour(gv, m, info=True)
    rounds, batches, applied, _ = _stats(gv)
    assert path.tolist() == opt and info == winfo
    assert batches >= 2 and rounds % batches == 0
    batch = rounds // batches                                         # the rounds between two reads of the "done" word
    assert info[1] > batch and info[2] == 1
    assert batches == info[1] // batch + 1 and applied == info[1]     # (the last round with work is the scan that finds nothing)


@pytest.mark.parametrize("cut", [1, 5])
@pytest.mark.parametrize("kind", ["euclid", "asym_gap"])
def test_max_rounds(kind, cut):
    import dmf_amd
    V = 65
    gv, m = _gv(), _map(kind, V)
    _, _, want, winfo = _ref(kind, V, "identity", cut)
    assert winfo[1] == cut and winfo[2] == 0                          # (the full solve needs more)
    path, info = dmf_amd.tour_two_opt(gv, m, np.arange(V), max_rounds=cut, info=True)
    assert path.tolist() == want and info == winfo and info[2] == 0, (info, winfo)
    _, _, want, winfo = _ref(kind, V, "nn", cut)
    path, info = dmf_amd.tour(gv, m, max_rounds=cut, info=True)
    assert path.tolist() == want and info == winfo, (info, winfo)
    d = Dev(gv, m)
    try:
        assert d.run("dmf_tour_device", None, cut) == (want, winfo)
    finally:
        d.close()


def test_errors():
    """A path that repeats an index or holds one out of range is DMF_ERR_INVALID in both forms and
    stays as it was; V > 46340 is DMF_ERR_RANGE, with a null map."""
    from dmf_amd import _lib
    V = 65
    gv, m = _gv(), _map("asym", V)
    L, info = gv._L, np.full(5, FILL_INFO, np.uint64)
    twice, outside, negative = np.arange(V, dtype=np.int32), np.arange(V, dtype=np.int32), np.arange(V, dtype=np.int32)
    twice[40] = 3
    outside[64] = V
    negative[1] = -1
    d = Dev(gv, m)
    try:
        for bad in (twice, outside, negative):
            p = bad.copy()
            assert L.dmf_tour_two_opt(gv._h, m.ctypes.data, V, p.ctypes.data, 0, info.ctypes.data) == _lib.DMF_ERR_INVALID
            assert np.array_equal(p, bad) and (info == FILL_INFO).all()
            got, dinfo = d.run("dmf_tour_two_opt_device", bad, 0, status=_lib.DMF_ERR_INVALID)
            assert got == bad.tolist() and dinfo == _info(np.full(5, FILL_INFO, np.uint64))
    finally:
        d.close()
    for f in (L.dmf_tour, L.dmf_tour_device, L.dmf_tour_two_opt, L.dmf_tour_two_opt_device):
        assert f(gv._h, None, 46341, None, 0, None) == _lib.DMF_ERR_RANGE
    for f in (L.dmf_tour_nearest_neighbour, L.dmf_tour_nearest_neighbour_device):
        assert f(gv._h, None, 46341, None, None) == _lib.DMF_ERR_RANGE
    assert L.dmf_tour(gv._h, None, 4, None, 0, None) == _lib.DMF_ERR_INVALID


def test_pipeline_collision_cost_map():
    """dmf_collision_cost_map_device on a small scene, V = 40 centres on a sphere around it, then
    dmf_tour_device on the device map == tour_ref on the downloaded map."""
    from dmf_amd import _lib, scene
    V = 40
    gv = Hh.gpu_volume()
    dc = Hh.DeviceCalls(gv)
    try:
        d_cp = dc.upload(scene.sphere_centres(V))
        d_map = dc.upload(np.full(V * V + GUARD, -5, np.int32))
        _lib.check(dc.L.dmf_collision_cost_map_device(dc.h, d_cp, V, d_map))
        d_path, d_info = dc.upload(np.full(V + GUARD, FILL_PATH, np.int32)), dc.upload(np.full(5, FILL_INFO, np.uint64))
        _lib.check(dc.L.dmf_tour_device(dc.h, d_map, V, d_path, 0, d_info))
        m = dc.download(d_map, V * V + GUARD, np.int32)
        path, info = dc.download(d_path, V + GUARD, np.int32), dc.download(d_info, 5, np.uint64)
    finally:
        dc.close()
    assert (m[V * V:] == -5).all() and (path[V:] == FILL_PATH).all()
    m = m[:V * V].reshape(V, V)
    assert (m == TO.INT_MAX).any() and not (m == TO.INT_MAX).all()
    want, winfo = TO.tour(m)
    assert path[:V].tolist() == want and _info(info) == winfo


def test_pipeline_travel_cost_map():
    """A 32^3 grid cut by a wall with one door, a sealed box behind it: the device form of the travel
    cost map == the existing travel_cost_map entry for entry (some pairs unreachable), and
    dmf_tour_device over it == tour_ref on the downloaded map."""
    from dmf_amd import _lib
    n, V = 32, 24
    gv = Hh.gpu_grid((n, n, n))
    d2 = np.full((n, n, n), 9, np.uint32)
    d2[15, :, :] = 0                       # the wall ...
    d2[15, 4, 5] = 9                       # ... and its door
    d2[24:29, 24:29, 24:29] = 0            # a sealed box
    d2[25:28, 25:28, 25:28] = 9
    rng = np.random.default_rng(5)
    cells = rng.integers(0, n, (V, 3)).astype(np.int32)
    cells[3] = (26, 26, 26)                # inside the box: unreachable from the rest
    cells[7] = (15, 9, 9)                  # in the wall: blocked
    cells[11] = (40, 2, 2)                 # outside the grid
    want = gv.travel_cost_map(d2, 4, cells)
    assert (want == TO.INT_MAX).any() and (want[0] != TO.INT_MAX).sum() > V // 2
    dc = Hh.DeviceCalls(gv)
    try:
        d_d2, d_cells = dc.upload(d2), dc.upload(cells)
        d_map = dc.upload(np.full(V * V + GUARD, -5, np.int32))
        _lib.check(dc.L.dmf_grid_travel_cost_map_device(dc.h, d_d2, 4, d_cells, V, d_map))
        d_path, d_info = dc.upload(np.full(V + GUARD, FILL_PATH, np.int32)), dc.upload(np.full(5, FILL_INFO, np.uint64))
        _lib.check(dc.L.dmf_tour_device(dc.h, d_map, V, d_path, 0, d_info))
        m = dc.download(d_map, V * V + GUARD, np.int32)
        path, info = dc.download(d_path, V + GUARD, np.int32), dc.download(d_info, 5, np.uint64)
    finally:
        dc.close()
    assert (m[V * V:] == -5).all() and np.array_equal(m[:V * V].reshape(V, V), want)
    wpath, winfo = TO.tour(want)
    assert path[:V].tolist() == wpath and (path[V:] == FILL_PATH).all() and _info(info) == winfo
    assert winfo[0] > 0                    # the lost cells are forced picks


def test_compat_example_prints_the_recorded_paths(tmp_path):
    """build/tour_headless (compat/TSPSolver.hpp) on three fixture matrices."""
    exe = os.path.join(ROOT, "depth-map-fusion-utils_amd", "build", "tour_headless")
    cases = TO.fixture_cases()
    picked = [next(c for c in cases if c[0] == kind and c[1].shape[0] == V)
              for kind, V in (("ties", 13), ("asym_nopath", 32), ("sym", 64))]
    for kind, m, nn, opt in picked:
        V = m.shape[0]
        f = tmp_path / f"{kind}_{V}.txt"
        f.write_text(f"{V}\n" + "\n".join(" ".join(str(int(x)) for x in row) for row in m) + "\n")
        r = subprocess.run([exe, str(f)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        lines = r.stdout.strip().splitlines()
        assert len(lines) == 4, r.stdout
        assert [int(x) for x in lines[0].split()] == nn and [int(x) for x in lines[2].split()] == opt
        assert int(lines[1]) == TO.path_length(m, nn) and int(lines[3]) == TO.path_length(m, opt)
