"""CPU: the view gain's ABI surface, its mask layout and self-checks of its
pure-Python reference (tests/viewgain_ref.py).  No GPU: the entry points are only asked to refuse
bad plain arguments, which they do before they touch the volume."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np

import helpers as Hh
import raycast_ref as RR
import viewgain_ref as VR

NAMES = ("dmf_view_gain_words", "dmf_view_mask_index", "dmf_view_gain", "dmf_view_gain_device",
         "dmf_next_best_views", "dmf_next_best_views_device")


def test_symbols_declared_and_exported():
    from dmf_amd import _lib
    L = _lib.load()
    syms = _lib.declared_symbols()
    for n in NAMES:
        assert n in syms and n in _lib.SIGNATURES and hasattr(L, n), n
    assert _lib.KNOBS["viewgain_walk"] == 14 and _lib.KNOBS["viewgain_batch"] == 15
    diag = open(_lib.DIAG_HEADER_PATH).read()
    for text in ("DMF_KNOB_VIEWGAIN_WALK = 14", "DMF_KNOB_VIEWGAIN_BATCH = 15", "DMF_KNOB_COUNT = 16"):
        assert text in diag, text
    assert "#define DMF_ABI_VERSION 1\n" in open(_lib.HEADER_PATH).read()
    import dmf_amd
    for m in ("view_gain", "next_best_views"):
        assert callable(getattr(dmf_amd.RayTracingEngine, m)), m
    assert callable(dmf_amd.VoxelVolume.view_mask_dense)


def test_plain_arguments_rejected_without_gpu():
    """Null volume / camera / grid / poses, range_mm outside 1..65535, a negative P and all
    outputs NULL are DMF_ERR_INVALID and leave the outputs untouched.  These checks precede any
    access to the volume, so a zeroed stand-in buffer serves as the non-null handle (were it read,
    `constructed` = 0 would give DMF_ERR_STATE)."""
    from dmf_amd import _lib
    L = _lib.load()
    fake = C.create_string_buffer(1 << 16)
    v = C.addressof(fake)
    cam = _lib.make_camera(Hh.KA, Hh.KA_WH[1], Hh.KA_WH[0])
    pc = C.addressof(cam)
    lo = np.zeros(8, np.int16)
    poses = np.zeros(12, np.float32)
    seen, gain, stats = np.full(4, 5, np.uint64), np.full(4, 6, np.uint64), np.full(3, 7, np.uint64)
    sel, nsel = np.full(4, -7, np.int32), np.full(1, -8, np.int32)
    s, gn, st, se, ns = (a.ctypes.data for a in (seen, gain, stats, sel, nsel))
    calls = {
        "host": lambda *a: L.dmf_view_gain(*a, s, gn),
        "device": lambda *a: L.dmf_view_gain_device(*a, s, gn, st),
        "nbv": lambda *a: L.dmf_next_best_views(*a, 5, se, ns, gn),
        "nbv device": lambda *a: L.dmf_next_best_views_device(*a, 5, se, ns, gn),
    }
    g, p = lo.ctypes.data, poses.ctypes.data
    for name, call in calls.items():
        assert call(None, pc, g, p, 1, 1, -1, 1000) == _lib.DMF_ERR_INVALID, name
        assert call(v, None, g, p, 1, 1, -1, 1000) == _lib.DMF_ERR_INVALID, name
        assert call(v, pc, None, p, 1, 1, -1, 1000) == _lib.DMF_ERR_INVALID, name
        assert call(v, pc, g, None, 1, 1, -1, 1000) == _lib.DMF_ERR_INVALID, name
        for rng in (0, -1, 65536, 2 ** 31 - 1, -2 ** 31):
            assert call(v, pc, g, p, 1, 1, -1, rng) == _lib.DMF_ERR_INVALID, (name, rng)
        assert call(v, pc, g, p, -1, 1, -1, 1000) == _lib.DMF_ERR_INVALID, name
        assert b"" != L.dmf_last_error()
    # all outputs NULL (the statistics are no output of their own)
    assert L.dmf_view_gain(v, pc, g, p, 1, 1, -1, 1000, None, None) == _lib.DMF_ERR_INVALID
    assert L.dmf_view_gain_device(v, pc, g, p, 1, 1, -1, 1000, None, None, st) == _lib.DMF_ERR_INVALID
    for f in (L.dmf_next_best_views, L.dmf_next_best_views_device):
        assert f(v, pc, g, p, 1, 1, -1, 1000, 5, None, ns, gn) == _lib.DMF_ERR_INVALID
        assert f(v, pc, g, p, 1, 1, -1, 1000, 5, se, None, gn) == _lib.DMF_ERR_INVALID
    # the two layout queries: null arguments; an unconstructed (zeroed) volume is DMF_ERR_STATE
    words, bit = np.full(1, -9, np.int64), np.full(1, 9, np.uint64)
    assert L.dmf_view_gain_words(None, words.ctypes.data) == _lib.DMF_ERR_INVALID
    assert L.dmf_view_gain_words(v, None) == _lib.DMF_ERR_INVALID
    assert L.dmf_view_mask_index(None, 0, 0, 0, bit.ctypes.data) == _lib.DMF_ERR_INVALID
    assert L.dmf_view_mask_index(v, 0, 0, 0, None) == _lib.DMF_ERR_INVALID
    assert (seen == 5).all() and (gain == 6).all() and (stats == 7).all() and (sel == -7).all() and nsel[0] == -8
    assert words[0] == -9 and bit[0] == 9


def test_mask_layout_pack_and_unpack():
    """The documented layout on grids (72, 40, 44) (partial tiles on two axes) and (8, 8, 8):
    viewgain_ref.pack, written from the formula, against the library's Python unpacking and
    against an independent cell-by-cell statement; padding bits stay 0.  (dmf_view_gain_words and
    dmf_view_mask_index need a constructed volume: tests/test_gpu_viewgain.py checks them against
    the same pack on the same grids.)"""
    import dmf_amd
    for dims in ((72, 40, 44), (8, 8, 8)):
        rng = np.random.default_rng(sum(dims))
        mask = rng.random(dims) < 0.3
        mask[0, 0, 0] = mask[-1, -1, -1] = True
        w = VR.pack(mask, dims)
        nt = [(n + 7) // 8 for n in dims]
        assert w.dtype == np.uint64 and w.size == 8 * nt[0] * nt[1] * nt[2] == VR.words(dims)
        assert sum(bin(int(x)).count("1") for x in w) == int(mask.sum())     # padding cells: no bit
        for x, y, z in ((0, 0, 0), (7, 7, 7), tuple(n - 1 for n in dims), (dims[0] // 2, 3, dims[2] - 2)):
            tile = ((x // 8) * nt[1] + y // 8) * nt[2] + z // 8
            i = tile * 512 + (x % 8) * 64 + (y % 8) * 8 + z % 8
            assert i == VR.bit_index(dims, x, y, z)
            assert bool((int(w[i // 64]) >> (i % 64)) & 1) == bool(mask[x, y, z])
        assert np.array_equal(dmf_amd._unpack_view_mask(w, dims), mask)
        all_set = VR.pack(np.ones(dims, bool), dims)
        assert np.array_equal(dmf_amd._unpack_view_mask(all_set, dims), np.ones(dims, bool))
    try:
        dmf_amd._unpack_view_mask(np.zeros(7, np.uint64), (8, 8, 8))
    except ValueError:
        pass
    else:
        raise AssertionError("a mask of the wrong size must be refused")


def test_compat_viewgain_compiles(tmp_path):
    """viewGain / nextBestViews next to rayCastLogOdds in compat/RayTracingEngine.hpp (g++
    -fsyntax-only against the headless shims)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    compat = os.path.join(root, "depth-map-fusion-utils_amd", "compat")
    src = tmp_path / "gain.cpp"
    src.write_text('''
#include "Camera.hpp"
#include "RayTracingEngine.hpp"
#include "Volume.hpp"
int main() {
  VoxelVolume v;
  std::vector<float> K = {600, 0, 320, 0, 600, 240, 0, 0, 1};
  Camera cam(K);
  RayTracingEngine eng(cam);
  std::vector<Eigen::Affine3f> poses{Eigen::Affine3f::Identity()};
  RayTracingEngine::FusionCounts acc;
  std::vector<uint16_t> frame(640 * 480);
  eng.fuseDepth(v, frame, poses, acc);
  const std::vector<int16_t> L = eng.logOdds(v, acc);
  std::vector<unsigned long long int> gain, seen;
  eng.viewGain(v, L, poses, 1, -1, 1000, gain);
  eng.viewGain(v, L, poses, 1, -1, 1000, gain, &seen);
  const std::vector<int> next = eng.nextBestViews(v, L, poses, 1, -1, 1000, 5);
  return (int)(gain.size() + seen.size() + next.size() + eng.nextBestViews(v, L, poses, 1, -1, 1000).size());
}
''')
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    r = subprocess.run([gxx, "-std=c++17", "-fsyntax-only", "-Wall", "-I", compat, "-I", os.path.join(compat, "shims"),
                        "-I", os.path.join(root, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


# ---------------------------------------------------------------- reference self-checks
DIMS = (24, 20, 16)
W, H = Hh.KA_WH


def test_reference_threshold_extremes_and_monotony(oracle):
    """On the (24, 20, 16) walk of test_raycast.py.  occ_threshold at or below every value: every
    cell is solid, the gain is 0 and every entering ray is stopped.  occ_threshold above and
    free_threshold below every value: every cell is unknown and seen = the union of the walked
    cells.  seen grows as free_threshold falls."""
    from dmf_amd import scene
    wk = RR.Walk(Hh.BOUNDS, DIMS, Hh.KA, H, W, scene.fibonacci_poses(1, seed=2), 1000)
    L = np.random.default_rng(4).integers(-100, 101, DIMS).astype(np.int16)
    entered = sum(1 for sr in wk.seq[0] for s in sr if s)
    assert 0 < entered <= H * W
    for occ in (int(L.min()), int(L.min()) - 5):
        s, st = VR.seen(wk, L, occ, -1)
        assert not s.any() and st.tolist() == [[entered, entered, 0]]
    s, st = VR.seen(wk, L, int(L.max()) + 1, int(L.min()) - 1)
    union = np.zeros(DIMS, bool)
    for q in wk.cells():
        union[q] = True
    assert union.any() and np.array_equal(s[0], union)
    assert st[0, 0] == entered and st[0, 1] == 0 and st[0, 2] == sum(len(x) for sr in wk.seq[0] for x in sr)
    prev = None
    for free in (60, 20, 0, -20, -60, -101):
        s, st = VR.seen(wk, L, 61, free)
        assert not (s[0] & ((L >= 61) | (L <= free))).any()              # only unknown cells are marked
        if prev is not None:
            assert (s[0] | ~prev[0]).all() and st[0, 2] >= prev[1] and st[0, 1] == prev[2]
        prev = (s[0], st[0, 2], st[0, 1])
    assert prev[0].any()
    # crossed thresholds: solid wins
    s, st = VR.seen(wk, L, -200, 200)
    assert not s.any() and st[0, 1] == entered


def test_reference_greedy():
    """greedy on hand-made sets: ties to the lowest index, a set that adds nothing is never
    taken, min_gain stops the selection."""
    a = np.zeros((4, 16), bool)
    a[0, :6] = True
    a[1, 4:10] = True
    a[2, :6] = True                                # equal to set 0: the tie goes to 0, then 2 adds nothing
    a[3, 12:14] = True
    assert VR.greedy(a, 1) == ([0, 1, 3], [6, 4, 2])
    assert VR.greedy(a, 3) == ([0, 1], [6, 4])
    assert VR.greedy(a, 7) == ([], [])
    assert VR.greedy(np.zeros((3, 8), bool), 0) == ([], [])
