"""CPU: the surface extraction's ABI surface and self-checks of its numpy
restatement (tests/surface_ref.py).  No GPU: the entry points are only asked to refuse bad plain
arguments, which they do before they touch the volume."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import helpers as Hh
import raycast_cases as RC
import surface_ref as SR

NAMES = ("dmf_grid_surface_device", "dmf_grid_surface", "dmf_volume_integrate_surface")


def test_symbols_declared_and_exported():
    from dmf_amd import _lib
    L = _lib.load()
    syms = _lib.declared_symbols()
    for n in NAMES:
        assert n in syms and n in _lib.SIGNATURES and hasattr(L, n), n
    import dmf_amd
    assert callable(dmf_amd.VoxelVolume.extract_surface) and callable(dmf_amd.VoxelVolume.integrate_surface)
    assert L.dmf_abi_version() == 1


def test_plain_arguments_rejected_without_gpu():
    """A null volume or grid, a negative cap and, in the device form, a null d_count or three null
    outputs are DMF_ERR_INVALID.  These checks precede any access to the volume, so a zeroed
    stand-in buffer serves as the non-null handle (were it read, `constructed` = 0 would give
    DMF_ERR_STATE).  Pre-filled outputs stay as they were."""
    from dmf_amd import _lib
    L = _lib.load()
    fake = C.create_string_buffer(1 << 16)
    v = C.addressof(fake)
    lo = np.zeros(8, np.int16)
    h, xyz, nrm = np.full(4, 5, np.uint64), np.full(12, -7.5, np.float32), np.full(12, 3.25, np.float32)
    cnt, n, ns = np.full(2, 9, np.uint64), C.c_int64(-3), C.c_int64(-4)
    g, ph, px, pn, pc = lo.ctypes.data, h.ctypes.data, xyz.ctypes.data, nrm.ctypes.data, cnt.ctypes.data
    dev, host, integ = L.dmf_grid_surface_device, L.dmf_grid_surface, L.dmf_volume_integrate_surface
    INV = _lib.DMF_ERR_INVALID
    assert dev(None, g, 1, -1, ph, px, pn, 4, pc) == INV
    assert dev(v, None, 1, -1, ph, px, pn, 4, pc) == INV
    assert dev(v, g, 1, -1, ph, px, pn, -1, pc) == INV
    assert dev(v, g, 1, -1, ph, px, pn, 4, None) == INV
    assert dev(v, g, 1, -1, None, None, None, 4, pc) == INV
    assert dev(v, g, 1, -1, None, None, None, 0, pc) == INV
    assert b"" != L.dmf_last_error()
    pn_, pns = C.addressof(n), C.addressof(ns)
    assert host(None, g, 1, -1, ph, px, pn, 4, pn_, pns) == INV
    assert host(v, None, 1, -1, ph, px, pn, 4, pn_, pns) == INV
    assert host(v, g, 1, -1, ph, px, pn, -1, pn_, pns) == INV
    assert host(v, g, 1, -1, None, None, None, -2 ** 63, pn_, pns) == INV
    assert integ(None, g, 1, -1, pn_) == INV
    assert integ(v, None, 1, -1, pn_) == INV
    assert (h == 5).all() and (xyz == -7.5).all() and (nrm == 3.25).all() and (cnt == 9).all()
    assert n.value == -3 and ns.value == -4


def test_compat_surface_compiles(tmp_path):
    """extractSurface / integrateSurface beside the drop-in methods of compat/Volume.hpp (g++
    -fsyntax-only against the headless shims)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    compat = os.path.join(root, "depth-map-fusion-utils_amd", "compat")
    src = tmp_path / "surface.cpp"
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
  std::vector<unsigned long long int> cells;
  pcl::PointCloud<pcl::PointNormal> cloud;
  v.extractSurface(L, 1, -1, cells, cloud);
  const long long n = v.integrateSurface(L, 1, -1);
  float s = 0;
  for (const auto& p : cloud.points) s += p.x + p.normal[2];
  return (int)(n + (long long)cells.size() + (long long)v.occupied_cells_.size() + (long long)s);
}
''')
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    r = subprocess.run([gxx, "-std=c++17", "-fsyntax-only", "-Wall", "-I", compat, "-I", os.path.join(compat, "shims"),
                        "-I", os.path.join(root, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


@pytest.mark.timeout(900)
def test_surface_kernels_no_scratch_no_spills(tmp_path):
    """Stricter than tests/test_kernel_resources.py's check of every source, for csrc/dmf_surface.hip:
    the four kernels exist, spill no SGPR either, and the streaming and bit passes stay light enough
    for full occupancy."""
    import test_kernel_resources as KR
    if not os.path.exists(KR.HIPCC):
        pytest.skip("hipcc not installed")
    ks = {n: v for n, v in KR._kernels("dmf_surface", tmp_path).items() if n.startswith("_ZN3dmf")}
    for name in ("k_sf_mask", "k_sf_surface", "k_sf_totals", "k_sf_emit"):
        assert any(name in n for n in ks), (name, sorted(ks))
    bad = {n: v for n, v in ks.items() if v.get("private_segment_fixed_size", 0) or v.get("vgpr_spill_count", 0)
           or v.get("sgpr_spill_count", 0)}
    assert not bad, f"kernels with scratch or spills: {bad}"
    assert all(v["vgpr_count"] <= 64 for v in ks.values()), ks   # 8 waves per SIMD


# ---------------------------------------------------------------- the restatement's self-checks
@pytest.mark.parametrize("thresholds", SR.THRESHOLDS1)
def test_reference_counts_fused_scene(thresholds):
    ref = SR.ref1(thresholds)
    assert ref["count"] == SR.COUNTS1[thresholds]
    assert ref["hash"].shape == (ref["count"][0],) and SR.in_order(ref, RC.DIMS1)
    if thresholds[1] == 0:      # every unobserved cell is free too: a solid cell without one is enclosed
        assert ref["count"][0] == ref["count"][1]


def _ulps_from_one(a):
    """|a - 1| in units of ulp(1.0f) = 2^-23."""
    return np.abs(a.astype(np.float64) - 1.0) / 2.0 ** -23


def test_reference_normals_fused_scene():
    """At (1, -1): one symmetric neighbourhood (zero normal); every other normal has unit float32
    norm within 2 ulp; the normals point towards free space, that is, towards a fusion camera."""
    ref = SR.ref1((1, -1))
    n = ref["normals"]
    zero = ~(n != 0).any(axis=1)
    assert int(zero.sum()) == 1 and not (ref["g"][zero] != 0).any()
    assert not np.signbit(n[zero]).any()
    sq = n * n
    norm = np.sqrt(sq[:, 0] + (sq[:, 1] + sq[:, 2]))
    assert norm.dtype == np.float32 and (_ulps_from_one(norm[~zero]) <= 2).all()
    assert (np.abs(ref["g"]) <= 65535).all()
    centres = np.asarray(RC.fusion_frames()[0], np.float64).reshape(-1, 3, 4)[:, :, 3]
    to_cam = centres[None, :, :] - ref["xyz"].astype(np.float64)[:, None, :]
    facing = ((to_cam * n.astype(np.float64)[:, None, :]).sum(axis=2) > 0).any(axis=1)
    assert facing.mean() > 0.95, facing.mean()


def test_reference_centres_round_trip_and_integrate_in_order(oracle):
    """Every centre passes validPoints and bins back to its own cell; integrating the cloud into an
    oracle volume gives occupied_cells_ = the hashes, in order."""
    ref = SR.ref1((1, -1))
    assert SR.round_trip_failures(RC.BOUNDS1, RC.DIMS1, ref) == 0
    v = SR.vol(RC.BOUNDS1, RC.DIMS1)
    assert [v.hash_id(tuple(int(q) for q in c)) for c in ref["cells"]] == [int(h) for h in ref["hash"]]
    ov = Hh.oracle_grid(oracle, RC.DIMS1, RC.BOUNDS1, clouds=[(ref["xyz"], ref["normals"])])
    assert np.array_equal(ov.occupied_cells_, ref["hash"])
    _, _, npts, nn = ov.voxel_table()
    assert (npts == 1).all() and (nn == 1).all()


@pytest.mark.parametrize("k", range(len(SR.RANDOM_DIMS)))
def test_reference_random_grids(k):
    """Partial tiles and words on every axis, a 1-cell grid, surface cells on every face."""
    dims, ref = SR.RANDOM_DIMS[k], SR.ref_random(k)
    assert ref["count"][0] == SR.RANDOM_COUNTS[k]
    assert ref["count"][1] == int((SR.random_grid(k) >= 1).sum())
    assert SR.round_trip_failures(Hh.ODD_BOUNDS, dims, ref) == 0 and SR.in_order(ref, dims)
    if k == 1:
        c = ref["cells"]
        for a in range(3):
            assert (c[:, a] == 0).any() and (c[:, a] == dims[a] - 1).any()
