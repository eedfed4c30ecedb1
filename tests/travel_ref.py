"""Numpy restatement of the travel field's definition, of the path rule and of the
travel cost map -- TEST INFRASTRUCTURE ONLY.  The field is a level-synchronous breadth-first search
by array shifts: level k + 1 = the traversable, unreached cells with a face neighbour in level k.
It shares no code with csrc/dmf_travel.hip.  The named cases of tests/test_gpu_travel.py live here
with their pinned totals; their distance fields are built in numpy, not by the distance kernels."""
import functools

import numpy as np

NO_DIST = 0xFFFFFFFF
NO_PATH = 0xFFFFFFFF
INT_MAX = 2147483647
DIMS = (70, 37, 41)          # 3 x 2 x 2 bricks, partial tiles and partial bricks on every axis
# the order in which the path rule looks at the face neighbours
NEIGHBOURS = ((-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1))


def traversable(dist2, radius2):
    return np.asarray(dist2, np.uint32) >= np.uint32(radius2)


def valid_seeds(trav, seeds):
    """The seeds inside the grid on traversable cells, (n, 3) int64."""
    s = np.asarray(seeds, np.int64).reshape(-1, 3)
    inside = ((s >= 0) & (s < np.array(trav.shape))).all(axis=1)
    s = s[inside]
    return s[trav[s[:, 0], s[:, 1], s[:, 2]]]


def bfs(dist2, radius2, seeds):
    """-> uint32 field: hops from any valid seed through cells with dist2 >= radius2; NO_PATH elsewhere."""
    trav = traversable(dist2, radius2)
    hops = np.full(trav.shape, NO_PATH, np.uint32)
    s = valid_seeds(trav, seeds)
    front = np.zeros(trav.shape, bool)
    front[s[:, 0], s[:, 1], s[:, 2]] = True
    free = trav & ~front
    k = 0
    while front.any():
        hops[front] = k
        grow = np.zeros_like(front)
        grow[1:] |= front[:-1]
        grow[:-1] |= front[1:]
        grow[:, 1:] |= front[:, :-1]
        grow[:, :-1] |= front[:, 1:]
        grow[:, :, 1:] |= front[:, :, :-1]
        grow[:, :, :-1] |= front[:, :, 1:]
        front = grow & free
        free &= ~front
        k += 1
    return hops


def totals(dist2, radius2, hops):
    """(traversable cells, reached cells, largest finite hop count, sum of the finite hop counts)."""
    fin = hops[hops != NO_PATH].astype(np.int64)
    return (int(traversable(dist2, radius2).sum()), int(fin.size), int(fin.max()) if fin.size else 0, int(fin.sum()))


def path(hops, target):
    """-> int32 (n, 3): target, ..., seed by the path rule; (0, 3) for a target outside or with NO_PATH.
    Stops where no neighbour holds k - 1 (a field that no travel call made)."""
    hops = np.asarray(hops)
    c = tuple(int(v) for v in target)
    if not all(0 <= c[a] < hops.shape[a] for a in range(3)) or int(hops[c]) == NO_PATH:
        return np.zeros((0, 3), np.int32)
    out = [c]
    k = int(hops[c])
    while k > 0:
        for d in NEIGHBOURS:
            q = (c[0] + d[0], c[1] + d[1], c[2] + d[2])
            if all(0 <= q[a] < hops.shape[a] for a in range(3)) and int(hops[q]) == k - 1:
                break
        else:
            break
        c = q
        out.append(c)
        k -= 1
    return np.asarray(out, np.int32).reshape(-1, 3)


def cost_map(dist2, radius2, cells):
    """-> int32 (V, V): [i][j] = hops from cells[i] to cells[j], INT_MAX where there is no path."""
    cells = np.asarray(cells, np.int64).reshape(-1, 3)
    V = cells.shape[0]
    out = np.full((V, V), INT_MAX, np.int32)
    shape = np.asarray(dist2).shape
    inside = ((cells >= 0) & (cells < np.array(shape))).all(axis=1)
    for i in range(V):
        h = bfs(dist2, radius2, cells[i:i + 1])
        for j in np.flatnonzero(inside):
            v = int(h[tuple(cells[j])])
            if v != NO_PATH:
                out[i, j] = v
    return out


# ---------------------------------------------------------------- the named cases
def _from_trav(trav):
    """A field whose cells are traversable at radius2 = 1 exactly where trav is set."""
    return np.where(trav, 1, 0).astype(np.uint32)


def _open(dims=DIMS):
    return np.full(dims, NO_DIST, np.uint32)


def _serpentine(axis, dims=DIMS):
    """Solid planes at 2, 6, 10, ... along `axis`, each with one open row: at the low and the high
    end of the next axis in turn, running along the third."""
    gap_axis = (axis + 1) % 3
    trav = np.ones(dims, bool)
    for n, p in enumerate(range(2, dims[axis], 4)):
        plane = [slice(None)] * 3
        plane[axis] = p
        trav[tuple(plane)] = False
        plane[gap_axis] = 0 if n % 2 == 0 else dims[gap_axis] - 1
        trav[tuple(plane)] = True
    return _from_trav(trav)


def _percolation(dims=DIMS, seed=5, cell=(3, 3, 3), blocked=0.62):
    trav = np.random.default_rng(seed).random(dims) >= blocked
    trav[cell] = True
    return _from_trav(trav)


CHAMBER_LO, CHAMBER_HI = (20, 10, 10), (50, 28, 30)   # the box's wall cells, both inclusive
SEED_OUT, SEED_IN = (0, 0, 0), (35, 20, 20)


def _chamber(dims=DIMS):
    trav = np.ones(dims, bool)
    lo, hi = CHAMBER_LO, CHAMBER_HI
    trav[lo[0]:hi[0] + 1, lo[1]:hi[1] + 1, lo[2]:hi[2] + 1] = False
    trav[lo[0] + 1:hi[0], lo[1] + 1:hi[1], lo[2] + 1:hi[2]] = True
    return _from_trav(trav)


def _corridor(dims=DIMS):
    """The exact dist2 of two solid planes y = 16 and y = 20: a 3-cell corridor whose centre line
    y = 18 has d^2 = 4."""
    y = np.arange(dims[1], dtype=np.int64)
    d = np.minimum(np.abs(y - 16), np.abs(y - 20)) ** 2
    return np.ascontiguousarray(np.broadcast_to(d[None, :, None], dims)).astype(np.uint32)


def _row300():
    trav = np.ones((300, 1, 1), bool)
    trav[150] = False
    return _from_trav(trav)


def _many_seeds():
    """48 seeds of default_rng(9) over a box larger than the grid (some outside, some on blocked
    cells), the first six repeated, and (3, 3, 3)."""
    s = np.random.default_rng(9).integers(-4, 74, (48, 3))
    s[:, 1] %= 45
    s[:, 2] %= 45
    return np.concatenate([s, s[:6], [[3, 3, 3]], [[-1, 0, 0]], [[70, 36, 40]], [[3, 3, 41]]]).astype(np.int32)


def _invalid_seeds():
    """Outside the grid on every side, and blocked cells of the percolation field."""
    blocked = np.argwhere(_percolation() == 0)[:5]
    return np.concatenate([[[-1, 3, 3], [70, 3, 3], [3, -1, 3], [3, 37, 3], [3, 3, -1], [3, 3, 41]], blocked]).astype(np.int32)


def _seeds(*cells):
    return np.asarray(cells, np.int32).reshape(-1, 3)


# name -> (field builder, radius2, seeds builder)
CASES = {
    "open_lo": (_open, 1, lambda: _seeds((0, 0, 0))),
    "open_hi": (_open, 7, lambda: _seeds((69, 36, 40))),
    "serpentine_x": (lambda: _serpentine(0), 1, lambda: _seeds((0, 0, 0))),
    "serpentine_y": (lambda: _serpentine(1), 1, lambda: _seeds((0, 0, 0))),
    "serpentine_z": (lambda: _serpentine(2), 1, lambda: _seeds((0, 0, 0))),
    "percolation": (_percolation, 1, lambda: _seeds((3, 3, 3))),
    "sealed_out": (_chamber, 1, lambda: _seeds(SEED_OUT)),
    "sealed_in": (_chamber, 1, lambda: _seeds(SEED_IN)),
    "sealed_both": (_chamber, 1, lambda: _seeds(SEED_OUT, SEED_IN)),
    "radius_4": (_corridor, 4, lambda: _seeds((0, 18, 0))),
    "radius_5": (_corridor, 5, lambda: _seeds((0, 18, 0))),
    "radius_0": (_corridor, 0, lambda: _seeds((0, 18, 0))),
    "seeds_many": (_percolation, 1, _many_seeds),
    "seeds_invalid": (_percolation, 1, _invalid_seeds),
    "seeds_none": (_percolation, 1, lambda: np.zeros((0, 3), np.int32)),
    "dims_1_1_1": (lambda: _open((1, 1, 1)), 1, lambda: _seeds((0, 0, 0))),
    "dims_300_1_1": (_row300, 1, lambda: _seeds((0, 0, 0))),
    "dims_1_40_33": (lambda: _percolation((1, 40, 33), 6, (0, 3, 3), 0.3), 1, lambda: _seeds((0, 3, 3))),
    "dims_33_33_33": (lambda: _percolation((33, 33, 33), 7, (32, 32, 32)), 1, lambda: _seeds((32, 32, 32))),
    # zdim a multiple of 4: every full row of 8 traversable cells starts on 16 bytes (the kernels' wide accesses)
    "dims_24_17_40": (lambda: _percolation((24, 17, 40), 8, (1, 1, 1), 0.3), 1, lambda: _seeds((1, 1, 1))),
    "dims_16_16_16": (lambda: _open((16, 16, 16)), 1, lambda: _seeds((5, 9, 2))),
}
# (traversable, reached, max hops, sum of finite hops) of each case, by bfs()
TOTALS = {
    "open_lo": (106190, 106190, 145, 7698775),
    "open_hi": (106190, 106190, 145, 7698775),
    "serpentine_x": (81098, 81098, 721, 28362037),
    "serpentine_y": (80990, 80990, 465, 17439975),
    "serpentine_z": (80660, 80660, 766, 28467430),
    "percolation": (40445, 33460, 183, 3153184),
    "sealed_out": (103188, 93821, 145, 6783469),
    "sealed_in": (103188, 9367, 32, 152423),
    "sealed_both": (103188, 103188, 145, 6935892),
    "radius_4": (88970, 2870, 109, 156415),
    "radius_5": (80360, 0, 0, 0),
    "radius_0": (106190, 106190, 127, 6768895),
    "seeds_many": (40445, 33460, 86, 1196074),
    "seeds_invalid": (40445, 0, 0, 0),
    "seeds_none": (40445, 0, 0, 0),
    "dims_1_1_1": (1, 1, 0, 0),
    "dims_300_1_1": (299, 150, 149, 11175),
    "dims_1_40_33": (956, 944, 64, 32986),
    "dims_33_33_33": (13882, 11479, 126, 849008),
    "dims_24_17_40": (11546, 11539, 75, 429396),
    "dims_16_16_16": (4096, 4096, 32, 58880),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (dims, dist2 uint32 dims, radius2, seeds int32 (n, 3), hops uint32 dims by bfs), computed
    once and shared, read-only."""
    build, radius2, seeds = CASES[name]
    d2 = np.ascontiguousarray(build(), np.uint32)
    s = np.ascontiguousarray(seeds(), np.int32).reshape(-1, 3)
    hops = bfs(d2, radius2, s)
    for a in (d2, s, hops):
        a.setflags(write=False)
    return d2.shape, d2, radius2, s, hops


def farthest(hops):
    """The first cell, in x-major order, with the largest finite hop count."""
    h = np.where(hops == NO_PATH, -1, hops.astype(np.int64))
    return tuple(int(v) for v in np.unravel_index(int(np.argmax(h)), hops.shape))


# the cost map's cells on the percolation field: the seed, three reachable cells far apart, one
# traversable cell that (3, 3, 3) does not reach, and one blocked cell
@functools.lru_cache(maxsize=None)
def cost_cells():
    _, d2, _, _, hops = case("percolation")
    reach = np.argwhere(hops != NO_PATH)
    island = np.argwhere((d2 >= 1) & (hops == NO_PATH))
    blocked = np.argwhere(d2 == 0)
    cells = [(3, 3, 3), tuple(reach[len(reach) // 3]), tuple(reach[2 * len(reach) // 3]), farthest(hops),
             tuple(island[len(island) // 2]), tuple(blocked[len(blocked) // 2])]
    return np.asarray(cells, np.int32)
