"""CPU: the tour's Python restatement (tests/tour_ref.py) against paths recorded from the reference's
own TSPSolver.hpp (tests/golden/tour_ref_cases.npz, made by tools/record_tour_ref.py), its two forms
against each other, and what the engine's tour entry points reject before they touch a device."""
import ctypes as C
import os

import numpy as np
import pytest

import tour_ref as TO

NAMES = ("dmf_tour_nearest_neighbour", "dmf_tour_nearest_neighbour_device", "dmf_tour_two_opt",
         "dmf_tour_two_opt_device", "dmf_tour", "dmf_tour_device", "dmf_tour_stats", "dmf_grid_travel_cost_map",
         "dmf_grid_travel_cost_map_device")


def test_fixture_covers_what_it_should():
    cases = TO.fixture_cases()
    assert len(cases) >= 40
    sizes = {m.shape[0] for _, m, _, _ in cases}
    assert set(range(2, 14)) <= sizes and {32, 64} <= sizes
    assert {k for k, _, _, _ in cases} == {"ties", "asym", "sym", "ties_nopath", "asym_nopath", "sym_nopath"}
    for kind, m, nn, opt in cases:
        V = m.shape[0]
        assert m.dtype == np.int32 and m.shape == (V, V)
        assert sorted(nn) == sorted(opt) == list(range(V)) and nn[0] == opt[0] == 0
        assert kind.endswith("_nopath") or not (m == TO.INT_MAX).any()
    assert sum((m == TO.INT_MAX).any() for kind, m, _, _ in cases if kind.endswith("_nopath")) >= 20


def test_both_forms_equal_the_recorded_paths():
    for kind, m, nn, opt in TO.fixture_cases():
        V = m.shape[0]
        got, forced = TO.nearest_neighbour(m)
        assert got == nn and forced == 0, (kind, V)      # (the reference aborts at a forced pick)
        assert TO.two_opt(m, nn)[0] == opt, (kind, V)
        assert TO.two_opt_literal(m, nn)[0] == opt, (kind, V)


@pytest.mark.parametrize("kind", TO.KINDS)
def test_forms_equal_each_other(kind):
    """Random maps of every kind, the dead-end ones included, up to V = 24: from the nearest-
    neighbour path, the identity and a random permutation, to the end and cut by max_rounds."""
    for V in (0, 1, 2, 3, 4, 5, 7, 11, 16, 24):
        m = TO.random_map(kind, V, 1)
        nn, forced = TO.nearest_neighbour(m)
        assert sorted(nn) == list(range(V))
        if kind == "all_nopath":
            assert nn == list(range(V)) and forced == max(V - 1, 0)
        perm = [0] + (1 + np.random.default_rng(V).permutation(max(V - 1, 0))).tolist() if V else []
        for start in (nn, list(range(V)), perm):
            full = TO.two_opt_literal(m, start)
            assert TO.two_opt(m, start) == full and full[2] == 1
            if kind == "all_nopath":
                assert full[0] == start and full[1] == 0
            for cut in (1, 2, 5):
                a, b = TO.two_opt_literal(m, start, cut), TO.two_opt(m, start, cut)
                assert a == b and a[1] == min(cut, full[1]) and a[2] == (full[1] < cut)
                assert TO.path_length(m, a[0]) <= TO.path_length(m, start)


def test_constructed_single_candidate_maps():
    for V, (i, k) in ((9, (1, 2)), (9, (7, 8)), (65, (63, 64)), (65, (1, 2))):
        m = TO.only_candidate_map(V, i, k)
        ident = list(range(V))
        base = TO.path_length(m, ident)
        better = [(a, b) for a in range(1, V) for b in range(a + 1, V)
                  if TO.path_length(m, ident[:a] + ident[a:b + 1][::-1] + ident[b + 1:]) < base] if V < 10 else None
        assert better in (None, [(i, k)])
        path, n, conv = TO.two_opt(m, ident, 1)
        assert n == 1 and path == ident[:i] + [ident[k], ident[i]] + ident[k + 1:]


def test_symbols_declared_and_exported():
    import dmf_amd
    from dmf_amd import _lib
    L = _lib.load()
    syms = _lib.declared_symbols()
    for n in NAMES:
        assert n in syms and n in _lib.SIGNATURES and hasattr(L, n), n
    for f in ("tour_nearest_neighbour", "tour_two_opt", "tour"):
        assert callable(getattr(dmf_amd, f)), f


def test_plain_arguments_rejected_without_gpu():
    """A null volume, a negative V or max_rounds and null pointers with V > 0 are DMF_ERR_INVALID;
    V > 46340 is DMF_ERR_RANGE and comes before the pointers.  These checks precede any access to
    the volume, so a zeroed stand-in serves as the handle.  Pre-filled outputs stay as they were."""
    from dmf_amd import _lib
    L = _lib.load()
    fake = C.create_string_buffer(1 << 16)
    v = C.addressof(fake)
    m, p, info = np.zeros((4, 4), np.int32), np.full(4, 77, np.int32), np.full(5, 9, np.uint64)
    pm, pp, pi = m.ctypes.data, p.ctypes.data, info.ctypes.data
    INV, RANGE = _lib.DMF_ERR_INVALID, _lib.DMF_ERR_RANGE
    for nn in (L.dmf_tour_nearest_neighbour, L.dmf_tour_nearest_neighbour_device):
        assert nn(None, pm, 4, pp, pi) == INV
        assert nn(v, None, 4, pp, pi) == INV
        assert nn(v, pm, 4, None, pi) == INV
        assert nn(v, pm, -1, pp, pi) == INV
        assert nn(v, None, 46341, None, None) == RANGE
    for f in (L.dmf_tour_two_opt, L.dmf_tour_two_opt_device, L.dmf_tour, L.dmf_tour_device):
        assert f(None, pm, 4, pp, 0, pi) == INV
        assert f(v, None, 4, pp, 0, pi) == INV
        assert f(v, pm, 4, None, 0, pi) == INV
        assert f(v, pm, -1, pp, 0, pi) == INV
        assert f(v, pm, 4, pp, -1, pi) == INV
        assert f(v, None, 46341, None, 0, None) == RANGE
        assert f(v, None, 2 ** 31 - 1, None, 0, None) == RANGE
    assert L.dmf_tour_stats(None, pi) == INV and L.dmf_tour_stats(v, None) == INV
    d2, cells = np.full(8, 1, np.uint32), np.zeros((4, 3), np.int32)
    pd, pc = d2.ctypes.data, cells.ctypes.data
    for f in (L.dmf_grid_travel_cost_map, L.dmf_grid_travel_cost_map_device):
        assert f(None, pd, 1, pc, 4, pm) == INV
        assert f(v, None, 1, pc, 4, pm) == INV
        assert f(v, pd, 1, None, 4, pm) == INV
        assert f(v, pd, 1, pc, 4, None) == INV
        assert f(v, pd, 1, pc, -1, pm) == INV
        assert f(v, pd, 1, None, 46341, None) == RANGE
        assert f(v, pd, 1, pc, 4, pm) == _lib.DMF_ERR_STATE
    assert (p == 77).all() and (info == 9).all() and (m == 0).all()


def test_python_validation():
    import dmf_amd

    class NoVolume:
        pass

    m = np.zeros((3, 3), np.int32)
    for bad in (m.astype(np.int64), np.zeros((3, 4), np.int32), np.zeros(9, np.int32)):
        for call in (lambda: dmf_amd.tour_nearest_neighbour(NoVolume(), bad), lambda: dmf_amd.tour(NoVolume(), bad),
                     lambda: dmf_amd.tour_two_opt(NoVolume(), bad, [0, 1, 2])):
            with pytest.raises(ValueError):
                call()
    for call in (lambda: dmf_amd.tour_two_opt(NoVolume(), m, [0, 1]), lambda: dmf_amd.tour_two_opt(NoVolume(), m, [0., 1., 2.]),
                 lambda: dmf_amd.tour_two_opt(NoVolume(), m, np.array([0, 1, 2 ** 32 + 2], np.int64)),   # (would wrap to 2)
                 lambda: dmf_amd.tour_two_opt(NoVolume(), m, np.array([0, 1, 2 ** 32 + 2], np.uint64)),
                 lambda: dmf_amd.tour_two_opt(NoVolume(), m, [0, 1, -2 ** 32 + 2]),
                 lambda: dmf_amd.tour_two_opt(NoVolume(), m, [0, 1, 2], max_rounds=-1),
                 lambda: dmf_amd.tour(NoVolume(), m, max_rounds=-1)):
        with pytest.raises(ValueError):
            call()


def test_compat_header_compiles(tmp_path):
    """compat/TSPSolver.hpp with the reference's names and members (g++ -fsyntax-only against the
    headless shims), and without <nlopt.hpp> anywhere on the include path."""
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    compat = os.path.join(root, "depth-map-fusion-utils_amd", "compat")
    src = tmp_path / "tsp.cpp"
    src.write_text('''
#include "TSPSolver.hpp"
int main() {
  std::vector<std::vector<int>> map = {{0, 3, 1}, {3, 0, 2}, {1, 2, 0}};
  TSP::NearestNeighborSearch nn(map);
  nn.solve();
  std::vector<int> path = nn.getPath();
  TSP::TwoOptSearch opt(map);
  opt.setPath(path);
  opt.solve();
  opt.printPath();
  std::vector<int> swapped = opt.twoOptSwap(opt.path_, 1, 2);
  TSP::GreedySolver g(map);
  return opt.getPathLength() + opt.getPathLength(swapped) + (int)g.map_.size() + g.path_[0];
}
''')
    r = subprocess.run([shutil.which("g++"), "-std=c++17", "-fsyntax-only", "-Wall", "-I", compat, "-I",
                        os.path.join(compat, "shims"), "-I", os.path.join(root, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
