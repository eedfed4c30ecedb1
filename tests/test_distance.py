"""CPU: the distance field's and the segment clearance's ABI surface and
self-checks of their numpy restatement (tests/distance_ref.py).  No GPU: the entry points are only
asked to refuse bad plain arguments, which they do before they touch the volume."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import distance_ref as DR
import fuse_points_ref as FP

NAMES = ("dmf_grid_distance", "dmf_grid_distance_device", "dmf_grid_clearance", "dmf_grid_clearance_device")


def test_symbols_declared_and_exported():
    from dmf_amd import _lib
    L = _lib.load()
    syms = _lib.declared_symbols()
    for n in NAMES:
        assert n in syms and n in _lib.SIGNATURES and hasattr(L, n), n
    import dmf_amd
    assert callable(dmf_amd.VoxelVolume.distance_field) and callable(dmf_amd.VoxelVolume.segment_clearance)
    assert dmf_amd.NO_DIST == DR.NO_DIST == 2 ** 32 - 1 and dmf_amd.NO_DIST.dtype == np.uint32
    assert "NO_DIST" not in dmf_amd.__all__
    assert L.dmf_abi_version() == 1


def test_plain_arguments_rejected_without_gpu():
    """Null pointers and a negative segment count are DMF_ERR_INVALID, and n = 0 is DMF_OK.  These
    checks precede any access to the volume, so a zeroed stand-in buffer serves as the non-null
    handle (were it read, `constructed` = 0 would give DMF_ERR_STATE).  Pre-filled outputs stay as
    they were."""
    from dmf_amd import _lib
    L = _lib.load()
    fake = C.create_string_buffer(1 << 16)
    v = C.addressof(fake)
    lo = np.zeros(8, np.int16)
    d2, cl, cnt = np.full(8, 77, np.uint32), np.full(4, 55, np.uint32), np.full(1, 9, np.uint64)
    a, b = np.full(12, 0.25, np.float32), np.full(12, -0.25, np.float32)
    ns = C.c_int64(-4)
    g, pd, pc, pk, pa, pb, pn = (lo.ctypes.data, d2.ctypes.data, cl.ctypes.data, cnt.ctypes.data, a.ctypes.data,
                                 b.ctypes.data, C.addressof(ns))
    INV, OK = _lib.DMF_ERR_INVALID, _lib.DMF_OK
    for dist, last in ((L.dmf_grid_distance, pn), (L.dmf_grid_distance_device, pk)):
        assert dist(None, g, 1, pd, last) == INV
        assert dist(v, None, 1, pd, last) == INV
        assert dist(v, g, 1, None, last) == INV
        assert dist(None, g, 1, pd, None) == INV
    assert b"" != L.dmf_last_error()
    for clear in (L.dmf_grid_clearance, L.dmf_grid_clearance_device):
        assert clear(None, pd, pa, pb, 4, pc) == INV
        assert clear(v, None, pa, pb, 4, pc) == INV
        assert clear(v, pd, None, pb, 4, pc) == INV
        assert clear(v, pd, pa, None, 4, pc) == INV
        assert clear(v, pd, pa, pb, 4, None) == INV
        assert clear(v, pd, pa, pb, -1, pc) == INV
        assert clear(v, pd, pa, pb, -2 ** 63, pc) == INV
        assert clear(None, pd, pa, pb, 0, pc) == INV
        assert clear(v, pd, pa, pb, 0, pc) == OK          # touches nothing, the volume included
    assert (d2 == 77).all() and (cl == 55).all() and (cnt == 9).all() and ns.value == -4


def test_compat_distance_compiles(tmp_path):
    """distanceField / segmentClearance beside extractSurface in compat/Volume.hpp (g++
    -fsyntax-only against the headless shims)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    compat = os.path.join(root, "depth-map-fusion-utils_amd", "compat")
    src = tmp_path / "distance.cpp"
    src.write_text('''
#include "Camera.hpp"
#include "RayTracingEngine.hpp"
#include "Volume.hpp"
int main() {
  VoxelVolume v;
  v.setDimensions(-0.5, 0.5, -0.5, 0.5, -0.5, 0.5);
  v.setVolumeSize(8, 8, 8);
  v.constructVolume();
  const std::vector<int16_t> L(512, 0);
  std::vector<uint32_t> d2;
  v.distanceField(L, 1, d2);
  std::vector<Eigen::Vector3f> a(2, Eigen::Vector3f(0.f, 0.f, 0.9f)), b(2, Eigen::Vector3f(0.1f, 0.1f, 0.1f));
  const std::vector<uint32_t> c2 = v.segmentClearance(d2, a, b);
  return (int)(d2.size() + c2.size()) + (c2[0] == DMF_NO_DIST);
}
''')
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    r = subprocess.run([gxx, "-std=c++17", "-fsyntax-only", "-Wall", "-I", compat, "-I", os.path.join(compat, "shims"),
                        "-I", os.path.join(root, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


@pytest.mark.timeout(900)
def test_distance_kernels_no_scratch_no_spills(tmp_path):
    """Stricter than tests/test_kernel_resources.py's check of every source, for
    csrc/dmf_distance.hip: the three kernels exist and spill no SGPR either (the envelope stack of
    the y / x pass is in global memory with its newest entries in LDS, never a private array), and
    all stay light enough in registers for 8 waves per SIMD."""
    import test_kernel_resources as KR
    if not os.path.exists(KR.HIPCC):
        pytest.skip("hipcc not installed")
    ks = {n: v for n, v in KR._kernels("dmf_distance", tmp_path).items() if n.startswith("_ZN3dmf")}
    for name in ("k_df_z", "k_df_axis", "k_df_clear"):
        assert any(name in n for n in ks), (name, sorted(ks))
    bad = {n: v for n, v in ks.items() if v.get("private_segment_fixed_size", 0) or v.get("vgpr_spill_count", 0)
           or v.get("sgpr_spill_count", 0)}
    assert not bad, f"kernels with scratch or spills: {bad}"
    assert all(v["vgpr_count"] <= 64 for v in ks.values()), ks   # 8 waves per SIMD


# ---------------------------------------------------------------- the restatement's self-checks
def _brute_ok(name):
    dims, _, _ = DR.CASES[name]
    return int(np.prod(dims)) <= DR.BRUTE_CELLS and int(np.prod(dims)) * DR.TOTALS[name][2] <= DR.BRUTE_WORK


def test_cases_and_totals_are_one_list():
    assert set(DR.CASES) == set(DR.TOTALS)
    assert sum(_brute_ok(n) for n in DR.CASES) >= 12


@pytest.mark.parametrize("name", sorted(DR.CASES))
def test_reference_pinned_totals(name):
    dims, L, threshold, d2 = DR.case(name)
    assert d2.shape == tuple(dims) and d2.dtype == np.uint32
    assert DR.totals(d2, L, dims, threshold) == DR.TOTALS[name]
    solid = DR.solid_mask(L, dims, threshold)
    assert np.array_equal(d2 == 0, solid)
    assert bool((d2 == DR.NO_DIST).all()) == (not solid.any()) and bool((d2 == DR.NO_DIST).any()) == (not solid.any())


@pytest.mark.parametrize("name", [n for n in sorted(DR.CASES) if _brute_ok(n)])
def test_reference_separable_equals_brute_force(name):
    dims, L, threshold, d2 = DR.case(name)
    assert np.array_equal(DR.edt2_brute(L, dims, threshold), d2)


@pytest.mark.parametrize("dims,site", [((7, 5, 9), (3, 0, 8)), ((1, 1, 33), (0, 0, 16)),
                                       ((70, 66, 130), (69, 65, 129))])
def test_reference_single_site_is_analytic(dims, site):
    L = np.full(dims, -2, np.int16)
    L[site] = 4
    x, y, z = np.meshgrid(*(np.arange(d, dtype=np.int64) for d in dims), indexing="ij")
    want = ((x - site[0]) ** 2 + (y - site[1]) ** 2 + (z - site[2]) ** 2).astype(np.uint32)
    assert np.array_equal(DR.edt2(L, dims, 1), want)
    assert np.array_equal(DR.edt2(L, dims, 4), want) and (DR.edt2(L, dims, 5) == DR.NO_DIST).all()


def test_reference_clearance_case():
    """The segments of fuse_points_ref.segment_case() over a 2 % solid grid: NO_DIST exactly on the
    segments without a cell (the non-finite ones, those that miss the grid, the whole NaN-origin
    scan), 0 on segments through a solid cell, and the end cell of an accepted endpoint counts."""
    d2, c2 = DR.segment_reference()
    a, b = DR.segments()
    assert c2.shape == (3 * FP.SEG_N,) and c2.dtype == np.uint32
    assert (c2[2 * FP.SEG_N:] == DR.NO_DIST).all()                 # the NaN origin
    assert (c2[:5] == DR.NO_DIST).all()                             # the non-finite points come first
    finite = np.isfinite(a).all(axis=1) & np.isfinite(b).all(axis=1)
    assert (c2[~finite] == DR.NO_DIST).all()
    some = c2[c2 != DR.NO_DIST]
    assert 1000 < some.size < 2 * FP.SEG_N and (some == 0).any() and (some > 0).any()
    assert int(some.max()) <= int(d2.max())
    # a == b inside the grid: one cell, its own value
    i = FP.SEG_N + 11
    assert tuple(a[i]) == tuple(b[i]) == tuple(np.float32(v) for v in FP.SEG_INSIDE)
    assert c2[i] == d2[24, 24, 20]
