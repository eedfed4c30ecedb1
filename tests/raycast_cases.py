"""The grids, cameras and poses of the log-odds ray-cast tests, with their reference walks
(raycast_ref.Walk), each built once per process and shared (TEST INFRASTRUCTURE ONLY)."""
import functools

import numpy as np

import helpers as Hh
import raycast_ref as RR
from dmf_amd import scene

KA = Hh.KA
WA, HA = Hh.KA_WH

# ---------------------------------------------------------------- case 1: fused scene, odd grid
DIMS1 = (72, 40, 44)      # deltas are no powers of two; tiles and mask words are partial on every axis
BOUNDS1 = Hh.BOUNDS
RANGE1 = 1000
THRESHOLDS1 = (1, 3511, -2000)


@functools.lru_cache(maxsize=None)
def fusion_frames():
    poses = scene.fibonacci_poses(4, seed=5)
    return poses, scene.render_frames(KA, WA, HA, poses)


@functools.lru_cache(maxsize=None)
def grid1():
    """The oracle's fusion of four rendered frames, finalized with the default parameters."""
    from oracle import oracle as O
    poses, depth = fusion_frames()
    h, m, _ = O.fuse_depth(Hh.oracle_grid(O, DIMS1, BOUNDS1), KA, depth, poses, dmin=200, dmax=1000)
    return O.fuse_finalize(h, m)


@functools.lru_cache(maxsize=None)
def poses1():
    """fusion pose 0; an unrelated pose; a camera inside the grid; fusion pose 1 looking away."""
    fp = fusion_frames()[0]
    away = np.array(fp[1], np.float32).reshape(3, 4).copy()
    away[:, :3] = -away[:, :3]
    return np.ascontiguousarray(np.stack([fp[0], scene.fibonacci_poses(3, seed=9)[1],
                                          scene.fibonacci_poses(2, radius=0.4, seed=3)[0], away.reshape(12)]),
                                np.float32)


@functools.lru_cache(maxsize=None)
def walk1():
    return RR.Walk(BOUNDS1, DIMS1, KA, HA, WA, poses1(), RANGE1)


@functools.lru_cache(maxsize=None)
def ref1(threshold):
    return walk1().surface(grid1(), threshold)


# ---------------------------------------------------------------- case 2: sparse grid, off-origin
DIMS2 = (96, 72, 80)
BOUNDS2 = Hh.shifted_bounds(Hh.OFFSETS[1])
RANGE2 = 1500
THRESHOLD2 = 0
CORNERS2 = ((31, 31, 31), (32, 32, 32), (95, 71, 79))  # brick corners and the last cell


@functools.lru_cache(maxsize=None)
def grid2():
    L = np.full(DIMS2, -5, np.int16)
    c = np.random.default_rng(21).integers([64, 0, 0], [96, 72, 80], (400, 3))
    L[c[:, 0], c[:, 1], c[:, 2]] = 7
    for q in CORNERS2:
        L[q] = 7
    return L


@functools.lru_cache(maxsize=None)
def poses2():
    p = np.concatenate([scene.fibonacci_poses(3, seed=5), scene.fibonacci_poses(2, radius=0.3, seed=8)])
    return Hh.shift_poses(p, Hh.OFFSETS[1])


@functools.lru_cache(maxsize=None)
def walk2():
    return RR.Walk(BOUNDS2, DIMS2, KA, HA, WA, poses2(), RANGE2)


@functools.lru_cache(maxsize=None)
def ref2():
    return walk2().surface(grid2(), THRESHOLD2)


def empty_blocks(L, threshold, B=32):
    """bool[ceil(n / B)...]: the aligned B^3 blocks of L without a cell >= threshold."""
    n = L.shape
    nb = [(n[a] + B - 1) // B for a in range(3)]
    out = np.ones(nb, bool)
    xs, ys, zs = np.nonzero(np.asarray(L) >= threshold)
    out[xs // B, ys // B, zs // B] = False
    return out


def hits_after_empty_block(walk, ref, L, threshold, B=32):
    """Per pose: the rays with a surface cell whose sequence crossed a wholly empty B^3 block
    before reaching it."""
    empty = empty_blocks(L, threshold, B)
    out = np.zeros(walk.P, np.int64)
    for p in range(walk.P):
        for r in range(walk.H):
            for c in range(walk.W):
                k = ref["index"][p, r, c]
                if k > 0 and any(empty[q[0] // B, q[1] // B, q[2] // B] for q in walk.seq[p][r][c][:k]):
                    out[p] += 1
    return out
