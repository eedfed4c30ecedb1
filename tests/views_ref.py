"""numpy restatement of the candidate views: PCL's VoxelGrid as
compat/shims/pcl/filters/voxel_grid.h states it, then Algorithms::positionCameras of
compat/Algorithms.hpp.  float32 throughout; a leaf's sum is formed one float32 add at a time in
ascending input index, starting from 0.0f.  tests/test_views.py pins this file to the tree's host code
(compiled with g++) bit for bit; tests/test_gpu_views.py compares the GPU with it.  The named cases are
computed once and shared (case())."""
import functools

import numpy as np

F = np.float32
INT_MAX = 2 ** 31 - 1
REFUSED = 0xFFFFFFFFFFFFFFFF


class Refused(Exception):
    """More than 2^31 - 1 leaves, or a bound's leaf coordinate at or beyond 2^31 in magnitude."""


def leaf3(leaf):
    return np.ascontiguousarray(np.broadcast_to(np.asarray(leaf, F), (3,)))


def leaf_box(xyz, leaf):
    """(indices of the participating points, inv, min_b, div) or None when no point takes part."""
    xyz = np.asarray(xyz, F).reshape(-1, 3)
    inv = F(1.0) / leaf3(leaf)
    idx = np.flatnonzero(np.isfinite(xyz).all(axis=1))
    if idx.size == 0:
        return None
    p = xyz[idx]
    with np.errstate(over="ignore", invalid="ignore"):
        lo, hi = np.floor(p.min(axis=0) * inv), np.floor(p.max(axis=0) * inv)
    if not ((np.abs(lo) < F(2.0 ** 31)).all() and (np.abs(hi) < F(2.0 ** 31)).all()):
        raise Refused()
    min_b = lo.astype(np.int64)
    div = hi.astype(np.int64) - min_b + 1
    if int(div[0]) * int(div[1]) * int(div[2]) > INT_MAX:
        raise Refused()
    return idx, inv, min_b, div


def leaf_keys(xyz, leaf):
    """(indices of the participating points, their leaf keys) -- ([], []) when none takes part."""
    box = leaf_box(xyz, leaf)
    if box is None:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    idx, inv, min_b, div = box
    ijk = np.floor(np.asarray(xyz, F).reshape(-1, 3)[idx] * inv).astype(np.int64) - min_b
    return idx, ijk[:, 0] + ijk[:, 1] * div[0] + ijk[:, 2] * div[0] * div[1]


def _sequential_sums(rows, starts, pops, reverse=False):
    """Per segment: 0.0f + rows[s] + rows[s + 1] + ... one float32 add at a time (reverse: from the
    segment's last row down)."""
    acc = np.zeros((starts.size, rows.shape[1]), F)
    for r in range(int(pops.max()) if pops.size else 0):
        live = np.flatnonzero(pops > r)
        at = starts[live] + (pops[live] - 1 - r if reverse else r)
        with np.errstate(invalid="ignore", over="ignore"):
            acc[live] = acc[live] + rows[at]
    return acc


def downsample(xyz, leaf, normals=None, unit_normals=False, reverse=False):
    """-> (xyz (m, 3), normals (m, 3) or None, points int32 (m,), counts (leaves, finite, largest));
    raises Refused.  reverse=True sums every leaf in descending index (what the result must NOT be)."""
    xyz = np.asarray(xyz, F).reshape(-1, 3)
    idx, key = leaf_keys(xyz, leaf)
    order = np.argsort(key, kind="stable")
    ks, src = key[order], idx[order]
    starts = np.flatnonzero(np.r_[True, ks[1:] != ks[:-1]]) if ks.size else np.zeros(0, np.int64)
    pops = np.diff(np.r_[starts, ks.size]).astype(np.int64)
    cnt = pops.astype(F)[:, None]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        oxyz = _sequential_sums(xyz[src], starts, pops, reverse) / cnt
        onrm = None
        if normals is not None:
            nn = np.asarray(normals, F).reshape(-1, 3)
            onrm = _sequential_sums(nn[src], starts, pops, reverse) / cnt
            if unit_normals:
                x, y, z = onrm[:, 0], onrm[:, 1], onrm[:, 2]
                q = np.sqrt(x * x + (y * y + z * z))
                nz = ~((x == 0) & (y == 0) & (z == 0))
                onrm[nz] = onrm[nz] / q[nz, None]
    counts = (int(starts.size), int(idx.size), int(pops.max()) if pops.size else 0)
    return oxyz.astype(F), onrm, pops.astype(np.int32), counts


def position_cameras(xyz, normals, distance_mm=300, flip=True):
    """-> (poses float32 (m, 3, 4), normals float32 (m, 3) as positionCameras leaves them)."""
    p = np.asarray(xyz, F).reshape(-1, 3)
    nn = np.array(normals, F).reshape(-1, 3)
    if flip:
        with np.errstate(invalid="ignore"):
            m = nn[:, 2] <= 0
        nn[m] = -nn[m]
    dist = F(float(distance_mm) / 1000.0)
    poses = np.zeros((p.shape[0], 3, 4), F)
    poses[:, 1, 0] = -1.0
    poses[:, 0, 1] = 1.0
    with np.errstate(invalid="ignore", over="ignore"):
        poses[:, :, 2] = -nn
        poses[:, :, 3] = ((dist * nn).astype(np.float64) + p.astype(np.float64)).astype(F)
    return poses, nn


# ---------------------------------------------------------------- named cases
def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F)


def _lattice(step, ks, js):
    """(k * step, j * step, step / 2) in float32 products, each also one float below and one above in
    x and y."""
    st = F(step)
    k, j = np.meshgrid(np.asarray(ks, F), np.asarray(js, F), indexing="ij")
    base = np.stack([(k * st).ravel(), (j * st).ravel(), np.full(k.size, F(0.5) * st, F)], axis=1).astype(F)
    out = [base]
    for d in (-np.inf, np.inf):
        q = base.copy()
        q[:, :2] = np.nextafter(base[:, :2], F(d))
        out.append(q)
    return np.concatenate(out)


def _crowded(rng):
    """4094 points in one 0.1 leaf near x = 1000 (float spacing 6e-5: the order of the adds shows),
    and 300 in the leaves around it."""
    a = np.stack([rng.uniform(1000.02, 1000.08, 4094), rng.uniform(0.02, 0.08, 4094), rng.uniform(0.02, 0.08, 4094)], 1)
    b = np.stack([rng.uniform(999.7, 1000.4, 300), rng.uniform(-0.2, 0.3, 300), rng.uniform(-0.2, 0.3, 300)], 1)
    return a.astype(F), b.astype(F)


def _build(name):
    rng = np.random.default_rng(sum(map(ord, name)))
    leaf, nn, unit = 0.1, "unit", False
    if name == "uniform":
        xyz = rng.uniform(-0.6, 0.66, (16000, 3)).astype(F)
    elif name == "lattice_0125":
        xyz, leaf = _lattice(0.125, range(-20, 21), range(-3, 4)), 0.125
    elif name == "lattice_01":
        xyz = _lattice(0.1, range(-40, 81), range(-2, 3))
    elif name == "anisotropic":
        xyz, leaf = rng.uniform(-0.5, 0.55, (9000, 3)).astype(F), (0.1, 0.05, 0.2)
    elif name == "crowded":
        a, b = _crowded(rng)
        xyz = np.concatenate([a, b])
    elif name == "crowded_interleaved":
        a, b = _crowded(rng)
        b = np.concatenate([b, np.stack([rng.uniform(999.0, 1001.0, 3794), rng.uniform(-1, 1, 3794),
                                         rng.uniform(-1, 1, 3794)], 1).astype(F)])
        xyz = np.empty((8188, 3), F)
        xyz[0::2], xyz[1::2] = a, b
    elif name == "far":
        xyz = (rng.uniform(0, 1.0, (8000, 3)) + np.array([1000.0, 2000.0, 0.0])).astype(F)
    elif name == "nonfinite_rows":
        xyz = rng.uniform(-0.4, 0.4, (3000, 3)).astype(F)
        bad = rng.choice(3000, 90, replace=False)
        for t, i in enumerate(bad):
            xyz[i, t % 3] = (np.nan, np.inf, -np.inf)[(t // 3) % 3]
        xyz[0, 0], xyz[2999, 2] = np.inf, np.nan     # the first and the last row too
    elif name == "all_nonfinite":
        xyz = rng.uniform(-1, 1, (50, 3)).astype(F)
        xyz[np.arange(50), np.arange(50) % 3] = np.tile(np.array([np.nan, np.inf, -np.inf], F), 17)[:50]
    elif name == "empty":
        xyz = np.zeros((0, 3), F)
    elif name == "single":
        xyz = np.array([[-0.3, 0.25, 7.0]], F)
    elif name == "coincident":
        xyz = np.tile(np.array([[0.123, -4.56, 0.789]], F), (100, 1))
    elif name in ("large_key", "refused"):
        e = 1.2 if name == "large_key" else 1.3
        xyz, leaf = np.array([[0, 0, 0], [e / 2, e / 2, e / 2], [e, e, e]], F), 0.001
    elif name == "no_normals":
        xyz, nn = rng.uniform(-0.3, 0.35, (2000, 3)).astype(F), None
    elif name == "unit_normals":
        xyz, unit = rng.uniform(-0.3, 0.35, (3000, 3)).astype(F), True
    elif name == "unit_zero_mean":
        # the first leaf holds n, -n: its mean normal is exactly zero and stays zero
        xyz, unit = rng.uniform(0.0, 0.5, (400, 3)).astype(F), True
        xyz[:2] = [[0.01, 0.01, 0.01], [0.02, 0.02, 0.02]]
        xyz[2:, 0] += F(0.1)
    else:
        raise KeyError(name)
    normals = None
    if nn == "unit":
        normals = _unit(rng, xyz.shape[0])
        if name == "nonfinite_rows":
            ok = np.flatnonzero(np.isfinite(xyz).all(axis=1))
            normals[ok[7], 1] = np.nan      # a NaN normal on a finite point propagates into its leaf
            normals[~np.isfinite(xyz).all(axis=1)] = np.nan   # the skipped rows' normals are never read
        if name == "unit_zero_mean":
            normals[1] = -normals[0]
    return xyz, normals, leaf3(leaf), unit


CASES = ("uniform", "lattice_0125", "lattice_01", "anisotropic", "crowded", "crowded_interleaved", "far",
         "nonfinite_rows", "all_nonfinite", "empty", "single", "coincident", "large_key", "refused", "no_normals",
         "unit_normals", "unit_zero_mean")


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (xyz, normals or None, leaf (3,), unit_normals, want): want = (xyz, normals or None, points,
    counts) of downsample(), or None for the refused case.  Shared: do not modify."""
    xyz, normals, leaf, unit = _build(name)
    try:
        want = downsample(xyz, leaf, normals, unit)
    except Refused:
        want = None
    for a in (xyz, normals, leaf) + (want[:3] if want else ()):
        if a is not None:
            a.setflags(write=False)
    return xyz, normals, leaf, unit, want


@functools.lru_cache(maxsize=None)
def placement_inputs():
    """Locations and normals for the placement: z > 0, z < 0, +0.0, -0.0 and NaN in z, NaN elsewhere,
    zero normals of both signs, and random ones; shared, read-only."""
    rng = np.random.default_rng(99)
    nn = np.concatenate([np.array([[0.1, 0.2, 0.97], [0.1, 0.2, -0.97], [0.6, -0.8, 0.0], [0.6, -0.8, -0.0],
                                   [0.3, 0.4, np.nan], [np.nan, 0.5, -0.5], [np.nan, 0.5, 0.5], [0.0, 0.0, 0.0],
                                   [-0.0, -0.0, -0.0], [0.0, -0.0, 1.0], [-0.0, 0.0, -1.0]], F), _unit(rng, 500)])
    xyz = rng.uniform(-2, 2, nn.shape).astype(F)
    xyz[7] = 0.0
    xyz[8] = -0.0
    xyz.setflags(write=False)
    nn.setflags(write=False)
    return xyz, nn
