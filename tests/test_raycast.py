"""CPU: the log-odds ray-cast's ABI surface and self-checks of its pure-Python
reference (tests/raycast_ref.py).  No GPU: the entry points are only asked to refuse bad plain
arguments, which they do before they touch the volume."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np

import helpers as Hh
import raycast_ref as RR

NAMES = ("dmf_raycast_logodds", "dmf_raycast_logodds_device")


def test_symbols_declared_and_exported():
    from dmf_amd import _lib
    L = _lib.load()
    syms = _lib.declared_symbols()
    for n in NAMES:
        assert n in syms and n in _lib.SIGNATURES and hasattr(L, n), n
    import dmf_amd
    assert dmf_amd.NO_CELL == np.uint64(2 ** 64 - 1) and dmf_amd.NO_CELL == RR.NO_CELL
    assert "NO_CELL" not in dmf_amd.__all__
    assert callable(dmf_amd.RayTracingEngine.raycast_logodds)


def test_plain_arguments_rejected_without_gpu():
    """Null volume / camera / grid / poses, range_mm outside 1..65535 and a negative P are
    DMF_ERR_INVALID.  These checks precede any access to the volume, so a zeroed stand-in buffer
    serves as the non-null handle (were it read, `constructed` = 0 would give DMF_ERR_STATE)."""
    from dmf_amd import _lib
    L = _lib.load()
    fake = C.create_string_buffer(1 << 16)
    v = C.addressof(fake)
    cam = _lib.make_camera(Hh.KA, Hh.KA_WH[1], Hh.KA_WH[0])
    pc = C.addressof(cam)
    lo = np.zeros(8, np.int16)
    poses = np.zeros(12, np.float32)
    out_d, out_c = np.full(4, -7, np.int32), np.full(4, 5, np.uint64)
    host = lambda *a: L.dmf_raycast_logodds(*a, out_d.ctypes.data, out_c.ctypes.data)
    dev = lambda *a: L.dmf_raycast_logodds_device(*a, out_d.ctypes.data, out_c.ctypes.data, None)
    g, p = lo.ctypes.data, poses.ctypes.data
    for call in (host, dev):
        assert call(None, pc, g, p, 1, 0, 1000) == _lib.DMF_ERR_INVALID
        assert call(v, None, g, p, 1, 0, 1000) == _lib.DMF_ERR_INVALID
        assert call(v, pc, None, p, 1, 0, 1000) == _lib.DMF_ERR_INVALID
        assert call(v, pc, g, None, 1, 0, 1000) == _lib.DMF_ERR_INVALID
        for rng in (0, -1, 65536, 2 ** 31 - 1, -2 ** 31):
            assert call(v, pc, g, p, 1, 0, rng) == _lib.DMF_ERR_INVALID, rng
        assert call(v, pc, g, p, -1, 0, 1000) == _lib.DMF_ERR_INVALID
        assert b"" != L.dmf_last_error()
    assert (out_d == -7).all() and (out_c == 5).all()


def test_compat_raycast_compiles(tmp_path):
    """rayCastLogOdds next to fuseDepth / logOdds in compat/RayTracingEngine.hpp (g++ -fsyntax-only
    against the headless shims)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    compat = os.path.join(root, "depth-map-fusion-utils_amd", "compat")
    src = tmp_path / "cast.cpp"
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
  std::vector<int32_t> depth;
  std::vector<unsigned long long int> cells;
  eng.rayCastLogOdds(v, L, poses, 0, 1000, depth, cells);
  size_t none = 0;
  for (auto h : cells) none += h == DMF_NO_CELL;
  return (int)(none + depth.size());
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


def _walk(range_mm):
    from dmf_amd import scene
    return RR.Walk(Hh.BOUNDS, DIMS, Hh.KA, H, W, scene.fibonacci_poses(1, seed=2), range_mm)


def test_reference_threshold_extremes(oracle):
    """Above every value: no cell anywhere (depth -1).  At or below every value: every ray that
    enters the grid stops at the first cell of its sequence, with that cell's hash and depth."""
    wk = _walk(1000)
    L = np.random.default_rng(4).integers(-100, 101, DIMS).astype(np.int16)
    hi = wk.surface(L, int(L.max()) + 1)
    assert (hi["cell"] == RR.NO_CELL).all() and (hi["depth"] == -1).all() and (hi["index"] == -1).all()
    assert hi["stats"][1] == 0 and 0 < hi["stats"][0] <= H * W
    lo = wk.surface(L, int(L.min()))
    entered = lo["length"] > 0
    assert entered.any() and np.array_equal(lo["index"] == 0, entered) and (lo["index"][~entered] == -1).all()
    assert np.array_equal(lo["cell"] == RR.NO_CELL, ~entered)
    assert np.array_equal(lo["stats"], [entered.sum(), entered.sum()]) and np.array_equal(hi["stats"][0], entered.sum())
    for r, c in ((0, 0), (H // 2, W // 2), (H - 1, W - 1)):
        if entered[0, r, c]:
            q = wk.seq[0][r][c][0]
            assert lo["cell"][0, r, c] == np.uint64(wk.vol.hash_id(q))
            assert lo["depth"][0, r, c] == RR.cell_depth(wk.vol, wk.inv[0], q)
            x, y, z = RR.unhash(lo["cell"][0, r, c])
            assert (int(x), int(y), int(z)) == q
    # one value in between: the reported cell is the first at or above it, nothing before it is
    mid = wk.surface(L, 60)
    for r in range(0, H, 5):
        for c in range(0, W, 7):
            k, s = mid["index"][0, r, c], wk.seq[0][r][c]
            assert all(L[q] < 60 for q in (s if k < 0 else s[:k])) and (k < 0 or L[s[k]] >= 60)


def test_reference_walks_the_fusion_cells(oracle):
    """The probe ray is the fusion's ray: for a constant-depth frame the union of the walked cells
    equals the cells with a non-zero hit or miss counter of oracle.fuse_depth."""
    for depth_mm in (700, 1500):
        wk = _walk(depth_mm)
        frame = np.full((1, H, W), depth_mm, np.uint16)
        h, m, st = oracle.fuse_depth(Hh.oracle_grid(oracle, DIMS), Hh.KA, frame, wk.poses, dmin=1, dmax=65535)
        touched = np.zeros(DIMS, bool)
        for q in wk.cells():
            touched[q] = True
        assert touched.any() and np.array_equal(touched.reshape(-1), (h != 0) | (m != 0))
        assert st[0] == sum(len(s) for sr in wk.seq[0] for s in sr)


# ---------------------------------------------------------------- the exact jump's arithmetic
def _jump_setup(n, rnd):
    """dda_setup's walk state (csrc/dmf_dda.hpp) for random quantised endpoints in an n grid."""
    Q, never = 256, 1 << 30
    qs = [rnd.randrange(0, n[a] * Q) for a in range(3)]
    qe = [rnd.randrange(0, n[a] * Q) for a in range(3)]
    if rnd.random() < 0.3:  # short and axis-aligned rays
        for a in range(3):
            if rnd.random() < 0.5:
                qe[a] = qs[a] + rnd.randrange(-300, 300)
            qe[a] = min(max(qe[a], 0), n[a] * Q - 1)
    cs, ce = [q // Q for q in qs], [q // Q for q in qe]
    adq = [abs(qe[a] - qs[a]) for a in range(3)]
    st = [(ce[a] > cs[a]) - (ce[a] < cs[a]) for a in range(3)]
    h = [2 * ((cs[a] + 1) * Q - qs[a]) if st[a] > 0 else 2 * (qs[a] - cs[a] * Q) + 1 for a in range(3)]
    K = [2 * Q * adq[a] for a in range(3)]

    def pair(a, b):
        if st[a] and st[b]:
            return h[a] * adq[b] - h[b] * adq[a]
        return -never if st[a] else (never if st[b] else 0)
    return cs, st, [pair(0, 1), pair(0, 2), pair(1, 2)], K, sum(abs(ce[a] - cs[a]) for a in range(3)) + 1


def _select(E, K):
    """dda_select: the stepped axis; E updated in place."""
    b10 = E[0] > 0
    s2 = (E[2] if b10 else E[1]) > 0
    s1, s0 = (not s2) and b10, (not s2) and (not b10)
    E[0] += K[1] if s0 else (-K[0] if s1 else 0)
    E[1] += K[2] if s0 else (-K[0] if s2 else 0)
    E[2] += K[2] if s1 else (-K[1] if s2 else 0)
    return 2 if s2 else (1 if s1 else 0)


def _jump(m, c, st, E, K):
    """rc_jump (csrc/dmf_raycast.hip) restated: -> (steps, cell after, E after)."""
    def before(d, rs, kb, ka, after):
        x = d + rs * kb
        if x < 0 or ka == 0:
            return 0
        q = x // ka
        return q + (1 if q * ka < x else 0) if after else q + 1
    r = [m - (c[a] & m) if st[a] > 0 else ((c[a] & m) if st[a] < 0 else 0) for a in range(3)]
    F01 = E[0] + r[0] * K[1] - r[1] * K[0]
    F02 = E[1] + r[0] * K[2] - r[2] * K[0]
    F12 = E[2] + r[1] * K[2] - r[2] * K[1]
    b10 = F01 > 0
    s2 = (F12 if b10 else F02) > 0
    s1 = (not s2) and b10
    if s2:
        n = [before(-E[1], r[2], K[0], K[2], False), before(-E[2], r[2], K[1], K[2], False), r[2] + 1]
    elif s1:
        n = [before(-E[0], r[1], K[0], K[1], False), r[1] + 1, before(E[2], r[1], K[2], K[1], True)]
    else:
        n = [r[0] + 1, before(E[0], r[0], K[1], K[0], True), before(E[1], r[0], K[2], K[0], True)]
    return (sum(n), [c[a] + st[a] * n[a] for a in range(3)],
            [E[0] + n[0] * K[1] - n[1] * K[0], E[1] + n[0] * K[2] - n[2] * K[0], E[2] + n[1] * K[2] - n[2] * K[1]])


def test_jump_arithmetic_equals_the_stepped_walk():
    """The cast kernel leaves an empty aligned cube of 8 or 32 cells in one jump.
    A restatement of that arithmetic against dda_select stepped cell by cell, from random
    positions of random rays: every skipped cell lies in the cube, the landing cell is the first
    outside it, the walk state after the jump is the stepped walk's, and a jump longer than the
    ray means the ray ends inside the cube.  (The HIP code itself is checked on the GPU against
    the reference, with both walks: tests/test_gpu_raycast.py.)"""
    import random
    rnd = random.Random(7)
    jumped = ended = 0
    for it in range(6000):
        n = rnd.choice([(2048, 2048, 2048), (72, 40, 44), (96, 72, 80), (512, 512, 512), (33, 1, 2047)])
        c, st, E, K, left = _jump_setup(n, rnd)
        states, cc, EE = [(list(c), list(E))], list(c), list(E)
        for _ in range(left - 1):
            a = _select(EE, K)
            cc[a] += st[a]
            states.append((list(cc), list(EE)))
        for _ in range(4):
            i, m = rnd.randrange(left), rnd.choice([7, 31])
            ci, Ei = states[i]
            nj, c2, E2 = _jump(m, ci, st, Ei, K)
            cube = [x & ~m for x in ci]
            if nj >= left - i:
                assert all([x & ~m for x in s[0]] == cube for s in states[i:]), (it, i, m)
                ended += 1
            else:
                assert all([x & ~m for x in s[0]] == cube for s in states[i:i + nj]), (it, i, m)
                assert (c2, E2) == states[i + nj] and [x & ~m for x in c2] != cube, (it, i, m, nj)
                jumped += 1
    assert jumped > 10000 and ended > 2000
