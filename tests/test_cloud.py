"""CPU: the brute-force restatement of the cloud nearest neighbour (tests/cloud_ref.py) against a float64
computation, the properties that make its named cases adversarial, the summaries' arithmetic, the
Python argument checks that need no device, and the new drop-in header and example under g++."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import cloud_ref as CR
import helpers as Hh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMPAT = os.path.join(ROOT, "depth-map-fusion-utils_amd", "compat")


@pytest.mark.parametrize("name", ["uniform", "far_uniform_0", "far_uniform_1", "outlier", "planar", "invalid_rows"])
def test_float32_minimum_against_float64(name):
    """The float32 minimiser's float64 distance lies within rounding of the float64 minimum.  Each of
    dx, dx*dx, the two sums errs by at most 2^-24 relative, so a computed d2 is within (1 +- 6 * 2^-24)
    of the exact one of the same float32 points, and the float32 minimiser's exact d2 is at most
    (1 + 6e) / (1 - 6e) < 1 + 16 * 2^-24 times the least exact d2."""
    q, r, d2, idx = CR.case(name)
    rows = np.flatnonzero(idx != CR.NO_POINT)[:300]
    r64 = r.astype(np.float64)
    ok = np.isfinite(r64).all(axis=1)
    for i in rows:
        d = ((q[i].astype(np.float64) - r64[ok]) ** 2).sum(axis=1)
        mine = ((q[i].astype(np.float64) - r64[idx[i]]) ** 2).sum()
        assert mine <= d.min() * (1 + 16 * 2.0 ** -24), (name, i)
        assert abs(float(d2[i]) - mine) <= mine * 8 * 2.0 ** -24


@pytest.mark.parametrize("name", CR.TIE_CASES)
def test_tie_cases_have_4_to_16_minimisers(name):
    q, r, d2, idx = CR.case(name)
    assert r.shape[0] == 9826 and q.shape[0] == 4000
    ties = CR.count_ties(q, r, d2)
    assert ties.min() >= 4 and ties.max() == 16 and set(np.unique(ties)) == {4, 8, 16}
    # the winner is in the first copy of the lattice: its twin in the reversed copy has a higher index
    assert (idx < 4913).all()
    # ... and it is the lowest of the tied ones
    for i in range(0, 4000, 97):
        dx, dy, dz = q[i, 0] - r[:, 0], q[i, 1] - r[:, 1], q[i, 2] - r[:, 2]
        assert idx[i] == np.flatnonzero(((dx * dx + dy * dy) + dz * dz) == d2[i])[0]


def test_self_case_returns_the_first_duplicate():
    q, r, d2, idx = CR.case("self")
    assert (d2 == 0).all() and (idx < 2500).all() and (idx[2500:] != np.arange(2500, 3200)).all()
    assert np.array_equal(r[idx], q)


def test_far_cases_sit_where_floats_are_coarse():
    q, r, _, _ = CR.case("far_uniform_1")
    gap = np.spacing(np.abs(r).max(axis=0))
    assert 6e-5 <= gap[0] <= 1.3e-4 and 1.2e-4 <= gap[1] <= 2.5e-4     # x near 1000, y near 2000
    # the cloud still is a unit cube there: many distinct values per axis
    assert all(np.unique(r[:, a]).size > 3000 for a in range(3))


@pytest.mark.parametrize("name", ["boundaries_pow2", "boundaries_5_64"])
def test_boundary_queries_straddle_lattice_coordinates(name):
    q, r, d2, idx = CR.case(name)
    vals = np.unique(r[:, 0])
    assert vals.size == 16 and r.shape[0] == 4096
    near = vals[np.abs(q[:, :, None] - vals[None, None, :]).argmin(axis=2)]
    below, on, above = (q < near), (q == near), (q > near)
    assert below.sum() > 4000 and on.sum() > 4000 and above.sum() > 4000
    assert np.array_equal(np.where(below, np.nextafter(q, np.float32(np.inf)), np.where(above, np.nextafter(q, np.float32(-np.inf)), q)), near)


def test_degenerate_cases_are_degenerate():
    assert np.ptp(CR.case("planar")[1], axis=0).tolist()[2] == 0
    assert np.ptp(CR.case("linear")[1], axis=0).tolist()[1:] == [0, 0]
    assert CR.case("single")[1].shape[0] == 1 and (CR.case("single")[3] == 0).all()
    assert np.ptp(CR.case("coincident")[1], axis=0).tolist() == [0, 0, 0] and (CR.case("coincident")[3] == 0).all()
    r = CR.case("outlier")[1]
    assert r.shape[0] == 5001 and (r[:5000].max(axis=0) <= 0.01).all() and r[5000].tolist() == [10, 10, 10]


def test_outside_queries_match_the_closed_form():
    q, r, d2, idx = CR.case("outside")
    assert q.shape[0] == 208 and (np.abs(q - 0.5).max(axis=1) > 9).all()
    assert np.array_equal(idx, CR.outside_closed_form(q))


def test_invalid_cases():
    q, r, d2, idx = CR.case("invalid_rows")
    badq = ~np.isfinite(q).all(axis=1)
    assert badq.sum() == 60 and (~np.isfinite(r).all(axis=1)).sum() == 401
    assert (idx[badq] == CR.NO_POINT).all() and np.isposinf(d2[badq]).all()
    assert (idx[~badq] > 0).all() and np.isfinite(r[idx[~badq]]).all()
    for name in ("invalid_ref", "empty_ref"):
        _, _, d2, idx = CR.case(name)
        assert (idx == CR.NO_POINT).all() and np.isposinf(d2).all() and idx.size == 200
    assert CR.case("empty_query")[2].size == 0


def test_summaries_arithmetic():
    q, r, d2, idx = CR.case("invalid_rows")
    counts, mx, total, avg = CR.summaries(d2, idx, r, (0.0, 0.05, 1e9))
    dist = np.sqrt(d2[idx >= 0]).astype(np.float64)
    assert counts == [540, 2599, int((dist > 0).sum()), int((dist > 0.05).sum()), 0]
    assert mx == dist.max() and abs(avg * 540 - total) <= 540 * 2.0 ** -53 * total
    assert CR.summaries(*CR.case("empty_ref")[2:], CR.case("empty_ref")[1])[:3] == ([0, 0, 0, 0], -1.0, 0.0)
    assert math.isnan(CR.summaries(*CR.case("empty_ref")[2:], CR.case("empty_ref")[1])[3])


def test_python_argument_checks_need_no_device():
    import dmf_amd
    V = dmf_amd.VoxelVolume
    assert dmf_amd.NO_POINT == -1
    assert V._cloud(np.zeros((4, 3), np.float16), "q").dtype == np.float32
    assert V._cloud(np.zeros((4, 3), np.int16), "q").dtype == np.float32
    for bad in (np.zeros((4, 3), np.float64), np.zeros((4, 3), np.int32), np.zeros((4, 3), np.complex64),
                np.zeros((4, 3), object), np.zeros(3, np.float32), np.zeros((4, 4), np.float32),
                np.zeros((2, 4, 3), np.float32)):
        with pytest.raises(ValueError):
            V._cloud(bad, "q")
    assert V._thresholds(()).size == 0 and V._thresholds(range(8)).size == 8
    for bad in (range(9), (-0.001,), (0.003, float("nan"))):
        with pytest.raises(ValueError):
            V._thresholds(bad)


def test_null_volume_is_rejected_without_a_device():
    from dmf_amd import _lib
    L = _lib.load()
    out = np.zeros(4, np.float32)
    for fn in (L.dmf_cloud_nearest, L.dmf_cloud_nearest_device):
        assert fn(None, None, 0, None, 0, out.ctypes.data, None, None, 0, None, None) == _lib.DMF_ERR_INVALID
    assert L.dmf_cloud_nearest_stats(None, out.ctypes.data) == _lib.DMF_ERR_INVALID


def test_compat_header_and_example_compile(tmp_path):
    """compat/ErrorCalc.hpp and compat/examples/cloud_error_headless.cpp against the headless shims
    (g++ -fsyntax-only; no GPU needed), as tests/test_abi.py does for the other drop-in headers."""
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    src = tmp_path / "use.cpp"
    src.write_text('''
#include <pcl/point_cloud.h>
#include <pcl/point_types.h>
#include "ErrorCalc.hpp"
int main() {
  pcl::PointCloud<pcl::PointXYZ> a, b;
  VoxelVolume v;
  ErrorCalc::CloudError e = ErrorCalc::cloudError(a, b);
  e = ErrorCalc::cloudError(v, a, b);
  std::vector<int16_t> grid;
  ErrorCalc::SurfaceError s = ErrorCalc::surfaceError(v, grid, b);
  s = ErrorCalc::surfaceError(v, grid, b, 1, -1, {0.003, 0.005}, true);
  return (int)(e.distance.size() + s.over.size() + s.dist2.size());
}
''')
    inc = ["-I", COMPAT, "-I", os.path.join(COMPAT, "shims"), "-I", os.path.join(ROOT, "include")]
    for f in (str(src), os.path.join(COMPAT, "examples", "cloud_error_headless.cpp")):
        subprocess.run([gxx, "-std=c++17", "-fsyntax-only", "-Wall", "-Werror"] + inc + [f], check=True,
                       capture_output=True, text=True)
