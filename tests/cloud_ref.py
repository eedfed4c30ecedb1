"""Brute-force restatement of the cloud nearest neighbour (include/dmf.h dmf_cloud_nearest*, DESIGN.md
§4.7) in chunked numpy float32, the named cases of tests/test_cloud.py and tests/test_gpu_cloud.py, and
the summaries as the reference's tests/ErrorCalc.cpp:74-97 forms them.

d2(q, r) = (dx*dx + dy*dy) + dz*dz in float32, one rounding per operation (numpy contracts nothing);
dist2 = the minimum over the reference points with finite coordinates, index = the lowest that attains
it (argmin returns the first minimum); +inf and -1 for a query with a non-finite coordinate and for
every query when no reference point is valid."""
import functools
import math

import numpy as np

import helpers as Hh

NO_POINT = -1
CHUNK = 1 << 22                       # distances held at once


def _f32(a):
    return np.ascontiguousarray(a, np.float32).reshape(-1, 3)


def nearest(query, ref):
    """-> (dist2 float32 (n,), index int32 (n,))."""
    q, r = _f32(query), _f32(ref)
    n = q.shape[0]
    d2, idx = np.full(n, np.inf, np.float32), np.full(n, NO_POINT, np.int32)
    rj = np.flatnonzero(np.isfinite(r).all(axis=1))
    rv = r[rj]
    qi = np.flatnonzero(np.isfinite(q).all(axis=1))
    if rv.shape[0] == 0 or qi.size == 0:
        return d2, idx
    rows = max(1, CHUNK // rv.shape[0])
    with np.errstate(over="ignore"):
        for a in range(0, qi.size, rows):
            sel = qi[a:a + rows]
            qc = q[sel]
            dx = qc[:, None, 0] - rv[None, :, 0]
            d = dx * dx
            dy = qc[:, None, 1] - rv[None, :, 1]
            d += dy * dy
            dz = qc[:, None, 2] - rv[None, :, 2]
            d += dz * dz
            assert d.dtype == np.float32
            j = np.argmin(d, axis=1)
            d2[sel] = d[np.arange(sel.size), j]
            idx[sel] = rj[j]
    return d2, idx


def summaries(d2, idx, ref, thresholds=(0.003, 0.005)):
    """-> (counts list[2 + T], max_error, fsum of the distances, avg_error in the reference's order):
    counts = {queries with a neighbour, valid reference points, per threshold the queries with
    (double)sqrtf(dist2) > t}; max_error -1.0 when no query is counted (ErrorCalc.cpp:74); avg_error =
    the double accumulated in index order over the count (nan when that is 0)."""
    has = idx != NO_POINT
    dist = np.sqrt(d2[has]).astype(np.float64)                  # sqrtf in float, promoted
    assert np.sqrt(d2[has]).dtype == np.float32
    nv = int(has.sum())
    counts = [nv, int(np.isfinite(_f32(ref)).all(axis=1).sum())] + [int((dist > float(t)).sum()) for t in thresholds]
    acc = 0.0
    for v in dist.tolist():
        acc += v
    return counts, (float(dist.max()) if nv else -1.0), math.fsum(dist.tolist()), (acc / nv if nv else float("nan"))


def count_ties(query, ref, d2):
    """Per query the number of valid reference points at exactly dist2."""
    q, r = _f32(query), _f32(ref)
    out = np.zeros(q.shape[0], np.int64)
    for i in range(q.shape[0]):
        dx, dy, dz = q[i, 0] - r[:, 0], q[i, 1] - r[:, 1], q[i, 2] - r[:, 2]
        out[i] = int((((dx * dx + dy * dy) + dz * dz) == d2[i]).sum())
    return out


# ----------------------------------------------------------------------------- the named cases
def lattice(k, step, origin=(0.0, 0.0, 0.0)):
    """k^3 points origin + step * (i, j, l), x slowest, in float64."""
    a = np.arange(k, dtype=np.float64) * step
    g = np.stack(np.meshgrid(a, a, a, indexing="ij"), axis=-1).reshape(-1, 3)
    return g + np.asarray(origin, np.float64)


def _uniform(n=2048, m=20000, seed=5):
    rng = np.random.default_rng(seed)
    return rng.random((n, 3)), rng.random((m, 3))


def _ties(step, n=4000, seed=6):
    """The 17^3 lattice followed by itself reversed (m = 9826); the queries are lattice points moved
    half a step on every axis -- all but the far corner, whose query would see 2 minimisers only: a
    query with j axes on the far face has 2 * 2^(3 - j) tied minimisers, 4 to 16."""
    g = lattice(17, step)
    ref = np.concatenate([g, g[::-1]])
    far = (np.rint(g / step) == 16).all(axis=1)
    pick = np.random.default_rng(seed).choice(np.flatnonzero(~far), n, replace=False)
    return g[pick] + step / 2, ref


def _self(seed=7):
    rng = np.random.default_rng(seed)
    base = rng.random((2500, 3))
    ref = np.concatenate([base, base[rng.permutation(2500)[:700]]])
    return ref, ref


def _boundaries(step, seed=8):
    """Reference points on a lattice of 16 values per axis over [0, 16 * step] (the value 15 * step
    left out, so 4096 points span a box of 16 steps: at 8 points per cell the plain cell edge is two
    steps); the queries are lattice points with, per axis, the coordinate itself, the float below or
    the float above."""
    a = np.array([k for k in range(17) if k != 15], np.float64) * step
    ref = np.stack(np.meshgrid(a, a, a, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float32)
    rng = np.random.default_rng(seed)
    q = ref[rng.integers(0, ref.shape[0], 6000)].copy()
    move = rng.integers(-1, 2, q.shape)
    q = np.where(move < 0, np.nextafter(q, np.float32(-np.inf)), np.where(move > 0, np.nextafter(q, np.float32(np.inf)), q))
    return q.astype(np.float32), ref


def _around(ref, n, seed, spread=0.3):
    """n queries: reference points moved by a normal step of `spread` box lengths."""
    rng = np.random.default_rng(seed)
    r = np.asarray(ref, np.float64)
    size = max(float((r.max(axis=0) - r.min(axis=0)).max()), 1e-3)
    return r[rng.integers(0, r.shape[0], n)] + rng.normal(0, spread * size, (n, 3))


def _planar(seed=9):
    ref = np.random.default_rng(seed).random((3000, 3))
    ref[:, 2] = 0.3
    return _around(ref, 500, seed + 1), ref


def _linear(seed=11):
    ref = np.random.default_rng(seed).random((3000, 3))
    ref[:, 1:] = (-0.2, 0.7)
    return _around(ref, 500, seed + 1), ref


def _single():
    ref = np.array([[0.25, -1.5, 3.0]])
    return _around(ref, 300, 13, spread=2000.0), ref


def _coincident():
    ref = np.tile(np.array([[0.1, 0.2, 0.3]], np.float32), (1000, 1))
    return _around(ref, 300, 14, spread=1000.0), ref


def _outlier(seed=15):
    """A blob of 5000 points within 1 cm and one point 10 m away: the box is the outlier's."""
    rng = np.random.default_rng(seed)
    ref = np.concatenate([rng.random((5000, 3)) * 0.01, [[10.0, 10.0, 10.0]]])
    q = np.concatenate([rng.random((300, 3)) * 0.012 - 0.001, rng.random((50, 3)) * 12 - 1, [[10.0, 10.0, 10.0]]])
    return q, ref


OUTSIDE_STEP = 0.125


def _outside(seed=16):
    """The 9^3 lattice over [0, 1]^3; 8 queries ten box lengths out on each face, edge and corner,
    off the lattice's bisectors (no ties)."""
    rng = np.random.default_rng(seed)
    dirs = np.array([(a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1) if (a, b, c) != (0, 0, 0)])
    q = np.repeat(dirs, 8, axis=0) * 10.0 + 0.5 + (rng.random((26 * 8, 3)) - 0.5) * 0.9
    q = (np.floor(q / OUTSIDE_STEP) + 0.13 + 0.25 * rng.random(q.shape)) * OUTSIDE_STEP
    return q, lattice(9, OUTSIDE_STEP)


def outside_closed_form(q):
    """The nearest point of the 9^3 lattice to each query, as its index: per axis the nearest of the 9
    coordinates."""
    k = np.clip(np.rint(np.asarray(q, np.float64) / OUTSIDE_STEP), 0, 8).astype(np.int64)
    return ((k[:, 0] * 9 + k[:, 1]) * 9 + k[:, 2]).astype(np.int32)


def _invalid(seed=17):
    """NaN and +-inf rows in both clouds (each with one, two or three bad coordinates)."""
    rng = np.random.default_rng(seed)
    q, r = rng.random((600, 3)).astype(np.float32), rng.random((3000, 3)).astype(np.float32)
    bad = (np.nan, np.inf, -np.inf)
    for a, rows in ((q, rng.choice(600, 60, replace=False)), (r, rng.choice(3000, 400, replace=False))):
        for t, i in enumerate(rows):
            a[i, rng.choice(3, 1 + t % 3, replace=False)] = bad[t % 3]
    r[0] = np.nan                                            # the lowest index is not a candidate
    return q, r


def _shifted(make, o):
    def f():
        q, r = make()
        return Hh.shift_points(q, o), Hh.shift_points(r, o)
    return f


def _small(n, m):
    def f():
        rng = np.random.default_rng(100 * n + m)
        return rng.random((n, 3)), rng.random((m, 3))
    return f


SMALL = ((1, 1), (63, 2), (64, 63), (65, 65), (257, 1), (1, 65), (257, 63), (64, 2), (63, 65), (65, 2))

CASES = {
    "uniform": _uniform,
    "ties": functools.partial(_ties, 2.0 ** -4),
    "self": _self,
    "far_uniform_0": _shifted(_uniform, Hh.OFFSETS[0]),
    "far_ties_0": _shifted(functools.partial(_ties, 2.0 ** -7), Hh.OFFSETS[0]),
    "far_uniform_1": _shifted(_uniform, Hh.OFFSETS[1]),
    "boundaries_pow2": functools.partial(_boundaries, 2.0 ** -4),
    "boundaries_5_64": functools.partial(_boundaries, 5.0 / 64),
    "planar": _planar,
    "linear": _linear,
    "single": _single,
    "coincident": _coincident,
    "outlier": _outlier,
    "outside": _outside,
    "invalid_rows": _invalid,
    "invalid_ref": lambda: (_uniform(200, 50)[0], np.full((50, 3), np.nan, np.float32)),
    "empty_ref": lambda: (_uniform(200, 50)[0], np.zeros((0, 3), np.float32)),
    "empty_query": lambda: (np.zeros((0, 3), np.float32), _uniform(200, 500)[1]),
}
CASES.update({f"small_{n}_{m}": _small(n, m) for n, m in SMALL})
TIE_CASES = ("ties", "far_ties_0")


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (query float32 (n, 3), ref float32 (m, 3), dist2, index), computed once and shared: read-only."""
    q, r = CASES[name]()
    q, r = _f32(q), _f32(r)
    d2, idx = nearest(q, r)
    for a in (q, r, d2, idx):
        a.setflags(write=False)
    return q, r, d2, idx
