"""The open tour over a cost map restated in Python: the nearest-neighbour
construction and the first-improvement 2-opt of the reference's TSPSolver.hpp, in two forms that
tests/test_tour.py holds against each other and against paths recorded from the reference
(tests/golden/tour_ref_cases.npz):
  * the literal form (nearest_neighbour, two_opt_literal): the path is rebuilt for every candidate
    and summed again, leaving with INT_MAX at the first INT_MAX edge;
  * the prefix-sum form (two_opt): four prefix arrays over the current path give every
    candidate's length at once, the first improving one is the least i * V + k.
Python ints do not overflow, like the engine's int64 sums.  Where every unvisited entry of a row is
INT_MAX the reference aborts; both forms take the lowest unvisited index and count it."""
import os

import numpy as np

INT_MAX = 2 ** 31 - 1
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tour_ref_cases.npz")


def fixture_cases():
    """[(kind, map, nearest-neighbour path, 2-opt path from it)] as the reference's own code gave them."""
    z = np.load(GOLDEN)
    return [(str(kind), z[f"m_{k}"], z[f"nn_{k}"].tolist(), z[f"opt_{k}"].tolist()) for k, kind in enumerate(z["kinds"])]


def path_length(m, path):
    """The reference's getPathLength(path): INT_MAX at the first INT_MAX edge, else the sum."""
    total = 0
    for a, b in zip(path[:-1], path[1:]):
        e = int(m[a][b])
        if e == INT_MAX:
            return INT_MAX
        total += e
    return total


def edge_sums(m, path):
    """(the sum of the path's edges below INT_MAX, the number of its INT_MAX edges): info[3], info[4]."""
    e = [int(m[a][b]) for a, b in zip(path[:-1], path[1:])]
    return sum(x for x in e if x != INT_MAX), sum(x == INT_MAX for x in e)


def nearest_neighbour(m):
    """-> (path, forced picks)."""
    V = len(m)
    if V == 0:
        return [], 0
    path, left, forced = [0], set(range(1, V)), 0
    while left:
        row, best, pick = m[path[-1]], INT_MAX, -1
        for j in sorted(left):
            if int(row[j]) < best:
                best, pick = int(row[j]), j
        if pick < 0:
            pick = min(left)
            forced += 1
        path.append(pick)
        left.remove(pick)
    return path, forced


def two_opt_literal(m, path, max_rounds=0):
    """-> (path, improvements, converged)."""
    path, V, n = [int(x) for x in path], len(path), 0
    while True:
        best, found = path_length(m, path), False
        for i in range(1, V):
            for k in range(i + 1, V):
                new = path[:i] + path[i:k + 1][::-1] + path[k + 1:]
                if path_length(m, new) < best:
                    path, found = new, True
                    break
            if found:
                break
        if not found:
            return path, n, 1
        n += 1
        if max_rounds and n >= max_rounds:
            return path, n, 0


def two_opt(m, path, max_rounds=0):
    """The prefix-sum form -> (path, improvements, converged)."""
    m = np.asarray(m, np.int64)
    p = np.array(path, np.int64)
    V, n = len(p), 0
    if V < 3:
        return [int(x) for x in p], 0, 1
    ii, kk = np.triu_indices(V, 1)
    keep = ii >= 1
    ii, kk = ii[keep], kk[keep]                     # lexicographic already
    kn = np.minimum(kk + 1, V - 1)
    tail = kk + 1 < V
    while True:
        ef, eb = m[p[:-1], p[1:]], m[p[1:], p[:-1]]
        fs = np.concatenate([[0], np.cumsum(np.where(ef == INT_MAX, 0, ef))])
        bs = np.concatenate([[0], np.cumsum(np.where(eb == INT_MAX, 0, eb))])
        fc = np.concatenate([[0], np.cumsum(ef == INT_MAX)])
        bc = np.concatenate([[0], np.cumsum(eb == INT_MAX)])
        cur = INT_MAX if fc[-1] else fs[-1]
        e1, e2 = m[p[ii - 1], p[kk]], m[p[ii], p[kn]]
        s = fs[ii - 1] + np.where(e1 == INT_MAX, 0, e1) + bs[kk] - bs[ii]
        c = fc[ii - 1] + (e1 == INT_MAX) + bc[kk] - bc[ii]
        s = s + np.where(tail, np.where(e2 == INT_MAX, 0, e2) + fs[-1] - fs[kn], 0)
        c = c + np.where(tail, (e2 == INT_MAX) + fc[-1] - fc[kn], 0)
        hit = np.flatnonzero(np.where(c > 0, INT_MAX, s) < cur)
        if hit.size == 0:
            return [int(x) for x in p], n, 1
        i, k = int(ii[hit[0]]), int(kk[hit[0]])
        p[i:k + 1] = p[i:k + 1][::-1].copy()
        n += 1
        if max_rounds and n >= max_rounds:
            return [int(x) for x in p], n, 0


def tour(m, max_rounds=0):
    """-> (path, (forced, improvements, converged, edge sum, INT_MAX edges)): the engine's info."""
    nn, forced = nearest_neighbour(m)
    path, n, conv = two_opt(m, nn, max_rounds)
    return path, (forced, n, conv) + edge_sums(m, path)


# ---------------------------------------------------------------- cost maps the tests share
KINDS = ("ties", "asym", "sym", "binary", "minus", "ties_nopath", "asym_nopath", "sym_nopath", "all_nopath", "one_lost", "asym_gap")


def random_map(kind, V, seed):
    """An int32 (V, V) cost map: entries in 0..5 / asymmetric in 0..999 / symmetric / in {0, 1} /
    in -1..3 (the device cost map writes -1); *_nopath: 15 % INT_MAX off the diagonal; all_nopath:
    INT_MAX everywhere; one_lost: no edge into or out of one node; asym_gap: asym_nopath, but the
    path 0, 1, 2, ... holds exactly one INT_MAX edge, into node V // 2, so one reversal can mend it."""
    rng = np.random.default_rng([V, KINDS.index(kind), seed])
    base = kind.split("_")[0]
    if base == "ties":
        m = rng.integers(0, 6, (V, V))
    elif base == "binary":
        m = rng.integers(0, 2, (V, V))
    elif base == "minus":
        m = rng.integers(-1, 4, (V, V))
    elif base == "sym":
        m = np.triu(rng.integers(0, 1000, (V, V)), 1)
        m = m + m.T
    else:
        m = rng.integers(0, 1000, (V, V))
    if (kind.endswith("_nopath") and base != "all") or kind == "asym_gap":
        m[(rng.random((V, V)) < 0.15) & ~np.eye(V, dtype=bool)] = INT_MAX
    if kind == "all_nopath":
        m[:] = INT_MAX
    if kind == "asym_gap" and V > 1:
        j = np.arange(1, V)
        m[j - 1, j] = np.where(m[j - 1, j] == INT_MAX, 500, m[j - 1, j])
        m[V // 2 - 1, V // 2] = INT_MAX
    if kind == "one_lost" and V > 1:
        lost = int(rng.integers(1, V))
        m[lost, :] = INT_MAX
        m[:, lost] = INT_MAX
    return m.astype(np.int32)


def euclid_map(V, seed):
    """int(dist * 1000) between V random points of the unit cube: the planners' cost, symmetric."""
    pts = np.random.default_rng([V, 99, seed]).random((V, 3))
    d = np.sqrt(((pts[:, None, :] - pts[None, :, :]) ** 2).sum(-1))
    return (d * 1000).astype(np.int32)


def only_candidate_map(V, i, k):
    """A map on which, from the path 0, 1, ..., V - 1, reversing positions i..k is the ONE improving
    candidate: every entry 10 but the identity path's forward edges (1) -- the path costs V - 1,
    any new edge costs 10 -- except that the edges the reversal brings are cheap enough to win by
    1.  (k = i + 1 only: the reversed stretch is one edge.)"""
    assert k == i + 1 and 1 <= i and k <= V - 1
    m = np.full((V, V), 10, np.int32)
    for j in range(1, V):
        m[j - 1, j] = 1
    # reversal of (i, i+1): edges (i-1 -> i+1), (i+1 -> i), (i -> i+2 if any) replace three (or two) edges of cost 1
    m[i - 1, k] = 0
    m[k, i] = 0
    if k + 1 < V:
        m[i, k + 1] = 1
    return m
