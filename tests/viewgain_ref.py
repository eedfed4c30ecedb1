"""Pure-Python restatement of the view gain over a fused grid and of next-best-view selection
 -- TEST INFRASTRUCTURE ONLY.

Built over raycast_ref.Walk.seq (the ray-cast's cell sequences, §4.1), so that one walk per case
is shared with the ray-cast tests.  Nothing here calls the library: pack() states the mask layout
from the specification's formula alone.
"""
import numpy as np


def classes(L, occ, free):
    """-> (solid, unknown) bool grids: solid iff L >= occ; unknown iff not solid and L > free."""
    L = np.asarray(L, np.int16).astype(np.int64)
    solid = L >= occ
    return solid, ~solid & (L > free)


def seen(walk, L, occ, free):
    """-> (seen bool (P,) + dims: the unknown cells strictly before the first solid cell of at
    least one pixel's sequence; stats int64 (P, 3): per pose {rays with a non-empty sequence, rays
    stopped by a solid cell, unknown visible cells summed over rays})."""
    L = np.asarray(L, np.int16).reshape(walk.dims)
    solid, unknown = classes(L, occ, free)
    out = np.zeros((walk.P,) + tuple(walk.dims), bool)
    stats = np.zeros((walk.P, 3), np.int64)
    for p in range(walk.P):
        for sr in walk.seq[p]:
            for s in sr:
                if not s:
                    continue
                stats[p, 0] += 1
                for q in s:
                    if solid[q]:
                        stats[p, 1] += 1
                        break
                    if unknown[q]:
                        stats[p, 2] += 1
                        out[p][q] = True
    return out, stats


def words(dims):
    """uint64 words per pose: 8 per 8x8x8-cell tile of the grid padded to whole tiles."""
    return 8 * int(np.prod([(n + 7) // 8 for n in dims]))


def bit_index(dims, x, y, z):
    """tile << 9 | (x & 7) << 6 | (y & 7) << 3 | (z & 7), tiles x-major over the padded grid."""
    nty, ntz = (dims[1] + 7) // 8, (dims[2] + 7) // 8
    tile = ((x >> 3) * nty + (y >> 3)) * ntz + (z >> 3)
    return (tile << 9) | ((x & 7) << 6) | ((y & 7) << 3) | (z & 7)


def pack(mask, dims):
    """A bool grid of `dims` -> its uint64 words: bit i & 63 of word i >> 6 for every set cell."""
    mask = np.asarray(mask, bool).reshape(dims)
    out = np.zeros(words(dims), np.uint64)
    x, y, z = np.nonzero(mask)
    i = bit_index(dims, x.astype(np.int64), y.astype(np.int64), z.astype(np.int64))
    np.bitwise_or.at(out, i >> 6, np.uint64(1) << (i & 63).astype(np.uint64))
    return out


def greedy(masks, min_gain):
    """greedySetCover (Algorithms.hpp:38-86) over bool sets masks[p]: gain = |set & ~covered|,
    argmax with ties to the lowest index, stop when the best gain is 0 or below min_gain.
    -> (selection order, the marginal gain of each selected set)."""
    sets = [np.asarray(m, bool).reshape(-1) for m in masks]
    covered = np.zeros_like(sets[0]) if sets else None
    order, gains = [], []
    left = set(range(len(sets)))
    while left:
        g = [int((sets[p] & ~covered).sum()) if p in left else -1 for p in range(len(sets))]
        best = int(np.argmax(g))          # the first maximum: ties to the lowest index
        if g[best] <= 0 or g[best] < min_gain:
            break
        order.append(best)
        gains.append(g[best])
        covered |= sets[best]
        left.discard(best)
    return order, gains


def marks_after(walk, L, occ, free, B):
    """Per pose: the rays that mark an unknown visible cell after their sequence crossed an
    aligned B^3 block without a solid or an unknown cell (wholly free)."""
    L = np.asarray(L, np.int16).reshape(walk.dims)
    solid, unknown = classes(L, occ, free)
    n = L.shape
    nb = [(n[a] + B - 1) // B for a in range(3)]
    free_block = np.ones(nb, bool)
    xs, ys, zs = np.nonzero(solid | unknown)
    free_block[xs // B, ys // B, zs // B] = False
    out = np.zeros(walk.P, np.int64)
    for p in range(walk.P):
        for sr in walk.seq[p]:
            for s in sr:
                crossed = False
                for q in s:
                    if solid[q]:
                        break
                    if free_block[q[0] // B, q[1] // B, q[2] // B]:
                        crossed = True
                    elif crossed and unknown[q]:
                        out[p] += 1
                        break
    return out
