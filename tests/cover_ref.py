"""Packed-mask restatement of the greedy set cover (Algorithms.hpp:38-86; DESIGN.md §4.5;
csrc/dmf_cover.hip: k_cover_gain, k_cover_pick, k_cover_merge) and the synthetic cases that reach
the kernels' data-independent regimes -- TEST INFRASTRUCTURE ONLY.

Nothing here calls the library.  cover() is vectorised numpy over (P, words) uint64 masks, so that
65535 sets cost a fraction of a second; tests/test_cover.py holds it against the oracle's C++
std::set_difference restatement and against viewgain_ref.greedy, and pins every selection in
EXPECTED below.

CASES maps a name to (masks, [min_gain, ...]); DOC maps the same name to one line that says which
kernel mistake the case is there to catch.  Every case is built from default_rng(SEED + its family's
number) and from nothing else, so the literals of EXPECTED hold on every machine.
"""
import numpy as np

SEED = 20261020
INT32_MIN, INT32_MAX = -2147483648, 2147483647

_POP8 = np.array([bin(i).count("1") for i in range(256)], np.int64)


def _bytes(a):
    """(P, words) uint64 -> its (P, 8 * words) bytes (the shape spelt out: P or words may be 0)."""
    a = np.ascontiguousarray(a, np.uint64)
    return a.view(np.uint8).reshape(a.shape[0], 8 * a.shape[1])


def popcount(a):
    """Bits set per row of a (P, words) uint64 array -> int64 (P,)."""
    return _POP8[_bytes(a)].sum(axis=1)


def cover(masks, min_gain):
    """Greedy set cover over (P, words) uint64 masks: gain = popcount(masks & ~covered) of the sets
    not yet taken, the first maximum (ties to the lowest index), stop when the best gain is 0 or
    below the SIGNED min_gain.  -> (selection order, the marginal gain of each selected set)."""
    masks = np.ascontiguousarray(masks, np.uint64)
    P, words = masks.shape
    covered = np.zeros(words, np.uint64)
    left = np.ones(P, bool)
    order, gains = [], []
    for _ in range(P):
        g = popcount(masks & ~covered)
        g[~left] = -1
        best = int(np.argmax(g))          # the first maximum
        if g[best] <= 0 or g[best] < int(min_gain):
            break
        order.append(best)
        gains.append(int(g[best]))
        covered |= masks[best]
        left[best] = False
    return order, gains


def index_lists(masks):
    """(P, words) uint64 -> P sorted arrays of the set bits' indices (64 * word + bit)."""
    return [np.nonzero(r)[0].astype(np.uint64) for r in unpack(masks)]


def unpack(masks):
    """(P, words) uint64 -> bool (P, 64 * words): bit i & 63 of word i >> 6 is element i."""
    return np.unpackbits(_bytes(masks), axis=1, bitorder="little").astype(bool)


def from_bits(P, words, sets):
    """{set index: iterable of bit indices} -> (P, words) uint64."""
    out = np.zeros((P, words), np.uint64)
    for p, bits in sets.items():
        b = np.asarray(list(bits), np.int64)
        np.bitwise_or.at(out[p], b >> 6, np.uint64(1) << (b & 63).astype(np.uint64))
    return out


def random_masks(rng, P, words, density):
    """(P, words) uint64 with each bit set with probability `density`."""
    bits = rng.random((P, 64 * words)) < density
    return np.packbits(bits, axis=1, bitorder="little").view(np.uint64).reshape(P, words)


# ---------------------------------------------------------------- the cases
CASES, DOC = {}, {}
TIES_FIRST = (5, 63, 64, 69)                 # ties_first_round's equal largest sets
TIES_STRIDE = (261, 5 + 256 * 2, 599)        # ties_across_stride's
WORD_TAILS = (1, 255, 256, 257, 1025)
BATCHES = ((8, 8), (9, 9), (16, 16), (17, 17), (20, 7), (20, 8), (20, 9), (12, 1))   # (P, k)
BOUNDARY_GAINS = [9, 5, 5, 4, 1]             # min_gain_boundary's marginal gains, in selection order
BOUNDARY_MIN_GAINS = [INT32_MIN, -1, 0, 1, 4, 5, 6, 10, INT32_MAX]


def _add(name, masks, min_gains, doc):
    CASES[name] = (np.ascontiguousarray(masks, np.uint64), [int(m) for m in min_gains])
    DOC[name] = doc


def _ties_first_round():
    rng = np.random.default_rng(SEED + 1)
    m = random_masks(rng, 70, 2, 0.3)
    big = random_masks(rng, 1, 2, 0.8)[0]
    for p in TIES_FIRST:
        m[p] = big
    _add("ties_first_round", m, [1, 5],
         "ties going to the highest index (or to any but the first), and a wave-boundary error in "
         "the pick's shuffle reduction at sets 63 / 64")


def _ties_across_stride():
    rng = np.random.default_rng(SEED + 2)
    m = random_masks(rng, 600, 1, 0.25)
    big = from_bits(1, 1, {0: range(3, 47)})[0]
    for p in TIES_STRIDE:
        m[p] = big
    _add("ties_across_stride", m, [1],
         "a pick whose strided thread loop keeps the later of two equal sets of one thread (261 and "
         "517 are thread 5's), or whose last thread's set (599) wins the reduction")


def _ties_in_marginal_gain():
    sets = {0: range(0, 30),                                    # 30: the first pick
            1: list(range(0, 25)) + [40, 41],                   # raw 27, adds 2 after set 0
            2: list(range(10, 13)) + list(range(30, 36)),       # raw 9, adds 6
            3: list(range(0, 5)) + list(range(34, 40))}         # raw 11, adds 6: ties with set 2
    _add("ties_in_marginal_gain", from_bits(5, 1, sets), [1, 5],
         "a pick that ranks by the sets' raw sizes, or a gain that forgets `& ~covered`, and ties "
         "of the marginal gain going to the higher index")


def _many_sets():
    p = np.arange(65535, dtype=np.int64)
    one = np.uint64(1)
    m = (one << ((7 * p) % 64).astype(np.uint64)) | (one << ((p // 64) % 64).astype(np.uint64))
    m[40000] = m[40001] = np.uint64((1 << 10) - 1)
    _add("many_sets", m.reshape(-1, 1), [1, 2],
         "a pick that reads only its first 256 sets or truncates the index to 16 bits, and a gain "
         "grid that stops short of the API's 65535 sets")


def _word_tails():
    for i, words in enumerate(WORD_TAILS):
        rng = np.random.default_rng(SEED + 50 + i)
        m = random_masks(rng, 9, words, 0.02)
        last = 64 * (words - 1)
        m[1] = from_bits(1, words, {0: [last + int(b) for b in rng.choice(63, 20, replace=False)]})[0]
        m[4] = from_bits(1, words, {0: [last + 63]})[0]
        m[2] = random_masks(rng, 1, words, 0.5)[0]
        m[6] = np.uint64(0xFFFFFFFFFFFFFFFF)
        full = 64 * words
        _add(f"word_tails_{words}", m, [1, full, full + 1],
             "a merge grid that drops the words past the last whole 256 (a set with bits only in the "
             "last word would be taken after the full set), and a gain loop that counts words "
             "short or twice (the full set's gain is exactly min_gain; above 2^16 at 1025 words)")


def _batch_boundaries():
    for i, (P, k) in enumerate(BATCHES):
        rng = np.random.default_rng(SEED + 100 + i)
        where = rng.permutation(P)            # where[j]: the index of the j-th largest disjoint set
        sets, at = {}, 0
        for j in range(k):
            sets[int(where[j])] = range(at, at + k - j)
            at += k - j
        for j in range(k, P):                 # never selectable: inside the largest set
            sets[int(where[j])] = range(0, k - 1)
        _add(f"batch_boundaries_{P}_{k}", from_bits(P, (at + 63) // 64, sets), [1],
             "a host loop that loses or repeats an iteration where the selection ends on one of its "
             "batches of 8, at P not a multiple of 8, or where all P sets are taken and the stop "
             "flag is never set")


def _min_gain_boundary():
    sizes = {2: 9, 0: 5, 4: 5, 3: 4, 1: 1}   # disjoint: selection order 2, 0, 4, 3, 1
    sets, at = {}, 0
    for p, n in sizes.items():
        sets[p] = range(at, at + n)
        at += n
    _add("min_gain_boundary", from_bits(6, 1, sets), BOUNDARY_MIN_GAINS,
         "`<=` in place of `<` at the min_gain test, and a min_gain compared unsigned (a negative "
         "one then stops the selection at once)")


def _nothing_to_select():
    doc = ("a call that selects a set of gain 0, reads masks it does not have (no words, no sets) "
           "or leaves the previous call's count")
    _add("nothing_to_select_zero_masks", np.zeros((4, 3), np.uint64), [-1, 1], doc)
    _add("nothing_to_select_no_words", np.zeros((3, 0), np.uint64), [-1, 1], doc)
    _add("nothing_to_select_no_sets", np.zeros((0, 2), np.uint64), [-1, 1], doc)


def _saturated():
    rng = np.random.default_rng(SEED + 9)
    m = random_masks(rng, 12, 4, 0.5)
    m[1:] &= m[0]
    m[7] = m[10] = m[0]
    size = int(popcount(m[:1])[0])
    _add("saturated", m, [1, size - 1, size, size + 1],
         "a removed or wholly covered set selected again (two later sets equal the first pick), "
         "and a stop that comes a round late")


def _random_medium():
    rng = np.random.default_rng(SEED + 10)
    m = random_masks(rng, 300, 11, 0.05)
    m[7] = m[3]
    _add("random_medium", m, [1, 5],
         "anything the named cases miss at more than 256 sets over several words, with one "
         "duplicated row")


for _build in (_ties_first_round, _ties_across_stride, _ties_in_marginal_gain, _many_sets, _word_tails,
               _batch_boundaries, _min_gain_boundary, _nothing_to_select, _saturated, _random_medium):
    _build()


# ---------------------------------------------------------------- the pinned selections
# name -> {min_gain: selection order}; literals, so that a change of cover() or of a case shows
_MANY = [40000, 642, 707, 772, 837, 966, 1031, 1096, 1161, 1228, 1421, 1486, 1551, 1616, 1681, 1874, 1943,
         2008, 2073, 2330, 2395, 2465, 2786, 2851, 2916, 3244, 3309, 3702]
_MEDIUM = [77, 44, 200, 56, 6, 14, 95, 23, 92, 142, 275, 277, 256, 139, 279, 278, 174, 147, 188, 220, 297, 4,
           57, 66, 51, 121, 69, 73, 187, 20, 36, 236, 24, 156, 123, 222, 67, 102, 246, 3, 8, 221, 34, 40, 48, 97]
EXPECTED = {
    "ties_first_round": {1: [5, 3, 51, 54], 5: [5, 3, 51]},
    "ties_across_stride": {1: [261, 19, 200, 9]},
    "ties_in_marginal_gain": {1: [0, 2, 3, 1], 5: [0, 2]},
    "many_sets": {1: _MANY, 2: _MANY},                       # every gain after the first is 2
    "word_tails_1": {1: [6], 64: [6], 65: []},
    "word_tails_255": {1: [6], 16320: [6], 16321: []},
    "word_tails_256": {1: [6], 16384: [6], 16385: []},
    "word_tails_257": {1: [6], 16448: [6], 16449: []},
    "word_tails_1025": {1: [6], 65600: [6], 65601: []},
    "batch_boundaries_8_8": {1: [5, 2, 3, 0, 7, 4, 6, 1]},
    "batch_boundaries_9_9": {1: [7, 2, 3, 4, 8, 5, 6, 0, 1]},
    "batch_boundaries_16_16": {1: [0, 6, 15, 10, 4, 9, 13, 3, 11, 12, 8, 2, 1, 5, 7, 14]},
    "batch_boundaries_17_17": {1: [14, 6, 3, 1, 9, 15, 13, 11, 5, 12, 16, 2, 8, 4, 10, 0, 7]},
    "batch_boundaries_20_7": {1: [11, 17, 0, 14, 19, 18, 10]},
    "batch_boundaries_20_8": {1: [14, 5, 4, 17, 12, 0, 16, 6]},
    "batch_boundaries_20_9": {1: [5, 19, 14, 12, 13, 3, 18, 1, 6]},
    "batch_boundaries_12_1": {1: [3]},
    "min_gain_boundary": {INT32_MIN: [2, 0, 4, 3, 1], -1: [2, 0, 4, 3, 1], 0: [2, 0, 4, 3, 1], 1: [2, 0, 4, 3, 1],
                          4: [2, 0, 4, 3], 5: [2, 0, 4], 6: [2], 10: [], INT32_MAX: []},
    "nothing_to_select_zero_masks": {-1: [], 1: []},
    "nothing_to_select_no_words": {-1: [], 1: []},
    "nothing_to_select_no_sets": {-1: [], 1: []},
    "saturated": {1: [0], 138: [0], 139: [0], 140: []},
    "random_medium": {1: _MEDIUM, 5: _MEDIUM[:34]},
}
