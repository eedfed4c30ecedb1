"""CPU: tests/cover_ref.py, the packed-mask restatement of the greedy set cover that
tests/test_gpu_cover.py holds the kernels against.  For every named case and every min_gain its
selection equals the pinned literal, the oracle's C++ std::set_difference restatement over sorted
index lists and, up to 600 sets, viewgain_ref.greedy over the unpacked masks; and each case is
what its name claims (the ties are ties, the batches end where they say, the boundary gains are
the listed ones)."""
import numpy as np
import pytest

import cover_ref as CR
import viewgain_ref as VG

PAIRS = [(name, mg) for name in CR.CASES for mg in CR.CASES[name][1]]


def test_cases_expected_and_docs_are_one_list():
    assert set(CR.CASES) == set(CR.EXPECTED) == set(CR.DOC)
    for name, (masks, min_gains) in CR.CASES.items():
        assert masks.dtype == np.uint64 and masks.ndim == 2 and masks.shape[0] <= 65535, name
        assert list(CR.EXPECTED[name]) == min_gains, name
        assert len(CR.DOC[name]) > 20, name
    assert {f"word_tails_{w}" for w in CR.WORD_TAILS} | {f"batch_boundaries_{P}_{k}" for P, k in CR.BATCHES} \
        <= set(CR.CASES)


@pytest.mark.parametrize("name,min_gain", PAIRS, ids=[f"{n}-{m}" for n, m in PAIRS])
def test_reference_equals_pinned_oracle_and_python(name, min_gain, oracle):
    masks, _ = CR.CASES[name]
    order, gains = CR.cover(masks, min_gain)
    print(name, min_gain, order, gains)
    assert order == CR.EXPECTED[name][min_gain]
    assert len(set(order)) == len(order) and len(gains) == len(order)
    assert all(g > 0 and g >= min_gain for g in gains) and gains == sorted(gains, reverse=True)
    covered = np.bitwise_or.reduce(masks[order], axis=0) if order else np.zeros(masks.shape[1], np.uint64)
    assert sum(gains) == int(CR.popcount(covered[None])[0])
    assert [int(x) for x in oracle.greedy_set_cover(CR.index_lists(masks), min_gain)] == order
    if masks.shape[0] <= 600:
        assert VG.greedy(CR.unpack(masks), min_gain) == (order, gains)


def test_unpack_states_the_bit_layout():
    m = CR.from_bits(2, 3, {0: [0, 63, 64, 191], 1: [130]})
    assert m.tolist() == [[(1 << 63) | 1, 1, 1 << 63], [0, 0, 4]]
    assert [x.tolist() for x in CR.index_lists(m)] == [[0, 63, 64, 191], [130]]
    assert CR.popcount(m).tolist() == [4, 1] and CR.unpack(m).sum(axis=1).tolist() == [4, 1]


def test_ties_are_ties():
    for name, tied in (("ties_first_round", CR.TIES_FIRST), ("ties_across_stride", CR.TIES_STRIDE)):
        masks, _ = CR.CASES[name]
        size = CR.popcount(masks)
        assert all(np.array_equal(masks[p], masks[tied[0]]) for p in tied), name
        others = np.delete(size, tied)
        assert others.max() < size[tied[0]], name            # strictly the largest, all equal
        assert CR.EXPECTED[name][1][0] == min(tied), name
    assert CR.TIES_FIRST[1] == 63 and CR.TIES_FIRST[2] == 64               # either side of a wave's end
    a, b, c = CR.TIES_STRIDE
    assert a % 256 == b % 256 == 5 and a // 256 != b // 256                # one thread's, two strides
    assert c == CR.CASES["ties_across_stride"][0].shape[0] - 1             # the last set
    # marginal ties: the raw sizes differ, the gains after the first pick tie, the raw-larger set loses
    masks, _ = CR.CASES["ties_in_marginal_gain"]
    raw = CR.popcount(masks).tolist()
    after = CR.popcount(masks & ~masks[0]).tolist()
    assert raw == [30, 27, 9, 11, 0] and after == [0, 2, 6, 6, 0]
    assert CR.cover(masks, 1) == ([0, 2, 3, 1], [30, 6, 4, 2])


@pytest.mark.parametrize("P,k", CR.BATCHES)
def test_batch_boundaries_select_k(P, k):
    masks, _ = CR.CASES[f"batch_boundaries_{P}_{k}"]
    order, gains = CR.cover(masks, 1)
    assert masks.shape[0] == P and len(order) == k and gains == list(range(k, 0, -1))
    covered = np.bitwise_or.reduce(masks[order], axis=0)
    assert not (masks & ~covered).any()                      # then the best gain is 0


def test_min_gain_boundary_gains():
    masks, min_gains = CR.CASES["min_gain_boundary"]
    assert CR.cover(masks, 0)[1] == CR.BOUNDARY_GAINS == [9, 5, 5, 4, 1]
    assert min_gains == [-2147483648, -1, 0, 1, 4, 5, 6, 10, 2147483647]
    assert [len(CR.EXPECTED["min_gain_boundary"][m]) for m in min_gains] == [5, 5, 5, 5, 4, 3, 1, 0, 0]


def test_word_tails_sets():
    for words in CR.WORD_TAILS:
        masks, min_gains = CR.CASES[f"word_tails_{words}"]
        assert masks.shape == (9, words) and min_gains == [1, 64 * words, 64 * words + 1]
        assert not masks[1, :-1].any() and CR.popcount(masks[1:2])[0] == 20          # the last word only
        assert not masks[4, :-1].any() and int(masks[4, -1]) == 1 << 63              # its bit 63 only
        assert abs(int(CR.popcount(masks[2:3])[0]) - 32 * words) <= 4 * np.sqrt(16 * words)   # dense
        assert int(CR.popcount(masks[6:7])[0]) == 64 * words                         # every bit
    assert 64 * 1025 > 1 << 16


def test_saturated_and_many_sets_shapes():
    masks, min_gains = CR.CASES["saturated"]
    assert not (masks & ~masks[0]).any() and np.array_equal(masks[7], masks[0]) and np.array_equal(masks[10], masks[0])
    size = int(CR.popcount(masks[:1])[0])
    assert min_gains == [1, size - 1, size, size + 1]
    masks, _ = CR.CASES["many_sets"]
    assert masks.shape == (65535, 1) and int(masks[40000, 0]) == int(masks[40001, 0]) == 1023
    assert int(CR.popcount(masks).max()) == 10 and int((CR.popcount(masks) == 10).sum()) == 2
    masks, _ = CR.CASES["random_medium"]
    assert masks.shape == (300, 11) and np.array_equal(masks[3], masks[7])
    assert 3 in CR.EXPECTED["random_medium"][1] and 7 not in CR.EXPECTED["random_medium"][1]
