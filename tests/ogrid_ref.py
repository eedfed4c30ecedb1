"""Inputs and a round emulator for the OccupancyGrid tests (tests/test_ogrid_paths.py).

chain_state      dense states whose reorganization (OccupancyGrid.hpp:200-286) has long
                 dependency chains: the fixed-point rounds of the GPU form run deep, or past
                 their cap into the single-lane fallback.
fixed_point_rounds  float32 emulation of those rounds in plain Python (the scalar helpers of
                 oracle/py_oracle.py; no code shared with oracle.cpp or the kernels): how many
                 rounds a state needs, so that a test knows which path a download must take.
dense_cloud      updateStates inputs with hundreds of points per voxel: counts past the HQ /
                 clean threshold (100) and per-voxel event runs longer than a 256-thread block.
"""
import numpy as np

from oracle.py_oracle import f32, s3

# ---------------------------------------------------------------------------- chain states


def grid_dims(bounds, res):
    """OccupancyGrid::construct (:345-352): int((max - min) / double(float res))."""
    return tuple(int((bounds[2 * a + 1] - bounds[2 * a]) / float(np.float32(res[a]))) for a in range(3))


def chain_state(dims, bounds, res, seed, lo=0.55, hi=0.95, counts=(1, 7, 250)):
    """(normal, centroid, count, flags): every voxel occupied; voxel s's centroid lies in voxel
    s + 1 (linear x-major index; the last voxel's in its own) at a relative offset uniform in
    (lo, hi) per axis; counts drawn from `counts` (with (100, 150, 250) every voxel passes the
    clean gate, and the merges are those of clean = False); random unit normals.  A merge halves the target's
    centroid towards the source's, which may or may not move the target's own target: the chains
    break at random, and the longest one sets the rounds."""
    rng = np.random.default_rng(seed)
    n = int(np.prod(dims))
    mins = np.array(bounds[0::2], np.float64)
    res = np.asarray(np.float32(res), np.float64)
    nxt = np.minimum(np.arange(n) + 1, n - 1)
    idx = np.stack(np.unravel_index(nxt, dims), 1).astype(np.float64)
    cen = (mins + (idx + rng.uniform(lo, hi, (n, 3))) * res).astype(np.float32)
    cnt = rng.choice(list(counts), n).astype(np.int32)
    nrm = rng.normal(size=(n, 3)).astype(np.float32)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True).astype(np.float32)
    fl = np.full(n, 3, np.uint8)
    return nrm, cen, cnt, fl


# Grids of the chain states: (bounds, res).  CHAIN_GRIDS[0] is test_ogrid's first reorganization
# grid (9 x 8 x 7), [1] the 12 x 10 x 9 one, [2] 8 x 8 x 6.
CHAIN_GRIDS = [((-0.05, 0.04, -0.035, 0.045, -0.04, 0.03), (0.01, 0.01, 0.01)),
               ((-0.06, 0.06, -0.05, 0.05, -0.045, 0.045), (0.01, 0.01, 0.01)),
               ((-0.04, 0.04, -0.04, 0.04, -0.03, 0.03), (0.01, 0.01, 0.01))]


# ---------------------------------------------------------------------------- round emulator

def _target(c, mins, res, dims):
    """getVoxelCoords (:373-379) of a centroid + validCoords; linear index or -1."""
    t = []
    for a in range(3):
        q = np.floor((np.float64(c[a]) - np.float64(mins[a])) / np.float64(res[a]))
        t.append(int(q) if (np.isfinite(q) and -2147483648.0 <= q < 2147483648.0) else -2147483648)
    if not all(0 <= t[a] < dims[a] for a in range(3)):
        return -1
    return (t[0] * dims[1] + t[1]) * dims[2] + t[2]


def _merge(d, s):
    """:242-255: state d (normal, centroid, count) after voxel state s merged into it."""
    dn, dc, dk = d
    sn, sc, _ = s
    sm = [dn[a] + sn[a] for a in range(3)]
    q2 = s3(sm[0] * sm[0], sm[1] * sm[1], sm[2] * sm[2])
    if q2 > f32(0):
        rt = f32(np.sqrt(q2))
        sm = [sm[a] / rt for a in range(3)]
    if dk == 0:
        return sm, list(sc), dk
    return sm, [(dc[a] + sc[a]) / f32(2) for a in range(3)], dk + 1


def _bits(st):
    return np.array(st[0] + st[1], np.float32).tobytes() + int(st[2]).to_bytes(4, "little", signed=True)


def fixed_point_rounds(dims, mins, res, normal, centroid, count, flags, clean, return_cloud=False):
    """Rounds of the parallel form of downloadReorganizedCloud: P_0 = the initial state; targets
    t_r(s) from P_r (occupied s, with clean: P_r(s).count >= 100); P_{r+1}(T) = init(T) folded with
    [P_r(s) : s < T, t_r(s) = T] in index order; stop when P_{r+1} == P_r bit for bit.  Returns the
    rounds run, the confirming one counted.  With return_cloud also the cloud of the final fold
    (every source of a target in order, a source equal to its target reading P(T)).

    A target whose source list and source states are those of the round before is not folded
    again (its fold would repeat): the work is about the sum of the voxels' chain depths."""
    n = int(np.prod(dims))
    with np.errstate(all="ignore"):
        init = [([f32(v) for v in normal[i]], [f32(v) for v in centroid[i]], int(count[i])) for i in range(n)]
        ibits = [_bits(st) for st in init]
        occ = [bool(int(flags[i]) & 1) for i in range(n)]
        P, pbits = list(init), list(ibits)
        tcache = {}   # state bits -> target
        memo = {}     # T -> (signature of its sources, folded state, its bits)
        rounds = 0
        while True:
            src = {}
            for s in range(n):
                if not occ[s] or (clean and P[s][2] < 100):
                    continue
                key = pbits[s][12:24]
                T = tcache.get(key)
                if T is None:
                    T = tcache[key] = _target(P[s][1], mins, res, dims)
                if T >= 0:
                    src.setdefault(T, []).append(s)
            Pn, nbits = list(init), list(ibits)
            for T, ss in src.items():
                before = [s for s in ss if s < T]
                if not before:
                    continue
                sig = tuple((s, pbits[s]) for s in before)
                hit = memo.get(T)
                if hit is None or hit[0] != sig:
                    d = init[T]
                    for s in before:
                        d = _merge(d, P[s])
                    hit = memo[T] = (sig, d, _bits(d))
                Pn[T], nbits[T] = hit[1], hit[2]
            rounds += 1
            same = nbits == pbits
            P, pbits = Pn, nbits
            if same:
                break
        if not return_cloud:
            return rounds
        out = []
        for T in sorted(src):
            d = init[T]
            for s in src[T]:
                d = _merge(d, P[s])
            out.append(d[1] + d[0])
        return rounds, np.array(out, np.float32).reshape(-1, 6)


# ---------------------------------------------------------------------------- dense updateStates input

def dense_cloud(dims, mins, res, rng, voxels, counts, half_len=0.0035, sigma=0.0003):
    """Points along a line through each chosen voxel's centre: for voxel i (x, y, z indices) a
    random unit direction d and counts[i] points centre + t d + N(0, sigma), |t| <= half_len; the
    normal of every one of the voxel's points is d.  Returns (cloud (n, 3), normals (n, 6) =
    x y z nx ny nz), voxel after voxel (shuffle before use).  With K = 0 the voxel's normal
    becomes d and most of its points lie within the 1 mm cylinder around the line: its count
    approaches counts[i]."""
    mins = np.asarray(mins, np.float64)
    res = np.asarray(np.float32(res), np.float64)
    pts, nrm = [], []
    for v, m in zip(voxels, counts):
        assert all(0 <= v[a] < dims[a] for a in range(3))
        c = mins + (np.asarray(v, np.float64) + 0.5) * res
        d = rng.normal(size=3)
        d /= np.linalg.norm(d)
        t = rng.uniform(-half_len, half_len, (m, 1))
        pts.append(c + t * d + rng.normal(0, sigma, (m, 3)))
        nrm.append(np.broadcast_to(d, (m, 3)))
    cloud = np.concatenate(pts).astype(np.float32)
    normals = np.concatenate([cloud, np.concatenate(nrm).astype(np.float32)], axis=1)
    return cloud, np.ascontiguousarray(normals, np.float32)


def longest_event_run(dims, mins, res, pts, k):
    """The largest number of (voxel, point) events of one voxel that updateStates builds from the
    points pts (n, >= 3) with neighbourhood K = k: points whose own voxel lies within k of it."""
    mins = np.asarray(mins, np.float64)
    res = np.asarray(np.float32(res), np.float64)
    ijk = np.floor((np.asarray(pts, np.float32)[:, :3].astype(np.float64) - mins) / res).astype(np.int64)
    runs = np.zeros(dims, np.int64)
    for o in np.ndindex(2 * k + 1, 2 * k + 1, 2 * k + 1):
        q = ijk + (np.asarray(o) - k)
        ok = np.all((q >= 0) & (q < np.asarray(dims)), axis=1)
        np.add.at(runs, tuple(q[ok].T), 1)
    return int(runs.max())
