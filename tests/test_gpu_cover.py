"""GPU: the greedy set cover (csrc/dmf_cover.hip: k_cover_gain, k_cover_pick,
k_cover_merge) on the synthetic masks of tests/cover_ref.py, through
dmf_greedy_set_cover_masks_device.  The rendered scenes of the other GPU tests never tie, never pass
30 sets and a few hundred words, and never stop at min_gain itself; the named cases do (each one's
line in cover_ref.DOC says which mistake it catches).  The volume only supplies the device and the
stream.  selected carries guard entries after the end and, with nselected, is pre-filled with a value
that is never an output: the selection must equal cover_ref.EXPECTED, exactly, and nothing else may
be written."""
import time

import numpy as np
import pytest

import cover_ref as CR
import helpers as Hh

pytestmark = pytest.mark.gpu

FILL = -7


@pytest.fixture(scope="module")
def gv():
    return Hh.gpu_grid((8, 8, 8))


def _check(dc, d_masks, masks, name):
    """Every min_gain of the case over the uploaded masks == EXPECTED, the rest of selected untouched."""
    from dmf_amd import _lib
    P, words = masks.shape
    for min_gain in CR.CASES[name][1]:
        exp = CR.EXPECTED[name][min_gain]
        st, n, sel = dc.cover_masks_guarded(d_masks, P, words, min_gain, fill=FILL)
        print(name, min_gain, st, n, sel[:max(n, 0)].tolist())
        assert st == _lib.DMF_OK, (name, min_gain, st)
        assert n == len(exp) and sel[:n].tolist() == exp, (name, min_gain, n, sel[:max(n, 0)].tolist(), exp)
        assert (sel[n:] == FILL).all(), (name, min_gain)


@pytest.mark.parametrize("name", list(CR.CASES))
def test_named_cases(name, gv):
    masks, _ = CR.CASES[name]
    dc = Hh.DeviceCalls(gv)
    try:
        _check(dc, dc.upload(masks), masks, name)
    finally:
        dc.close()


def test_calls_do_not_leak(gv):
    """One volume, one scratch: a call after a larger one (more sets, more words, more selected) must
    not see its `removed` flags, its control block or its `covered` words."""
    names = ("random_medium", "batch_boundaries_9_9", "nothing_to_select_zero_masks", "nothing_to_select_no_words",
             "nothing_to_select_no_sets", "random_medium", "many_sets", "ties_first_round")
    dc = Hh.DeviceCalls(gv)
    try:
        d = {name: dc.upload(CR.CASES[name][0]) for name in set(names)}
        for name in names:
            _check(dc, d[name], CR.CASES[name][0], name)
    finally:
        dc.close()


def test_gain_of_two_to_the_32(gv):
    """2 sets over 2^26 words (1 GiB of masks): set 0 holds one bit, set 1 every bit, a gain of
    exactly 2^32.  A key that keeps the gain in 32 bits reads it as "adds nothing" and takes set 0
    first."""
    from dmf_amd import _lib
    t0 = time.perf_counter()
    words = 1 << 26
    masks = np.full((2, words), 0xFFFFFFFFFFFFFFFF, np.uint64)
    masks[0] = 0
    masks[0, 12345] = 1 << 17
    dc = Hh.DeviceCalls(gv)
    try:
        d_masks = dc.upload(masks)
        t1 = time.perf_counter()
        st, n, sel = dc.cover_masks_guarded(d_masks, 2, words, 1, fill=FILL)
        t2 = time.perf_counter()
    finally:
        dc.close()                                           # the only large allocation of the file
    print(f"2^32: fill + upload {t1 - t0:.2f} s, call {t2 - t1:.2f} s -> status {st}, n {n}, selected {sel.tolist()}")
    assert st == _lib.DMF_OK
    assert n == 1 and sel.tolist() == [1] + [FILL] * (len(sel) - 1)


def test_status_rules(gv):
    import ctypes as C

    import dmf_amd
    from dmf_amd import _lib
    masks, _ = CR.CASES["min_gain_boundary"]
    P, words = masks.shape
    dc = Hh.DeviceCalls(gv)
    try:
        d_masks = dc.upload(masks)
        for bad_P, bad_words in ((-1, words), (65536, words), (P, -1)):
            st, n, sel = dc.cover_masks_guarded(d_masks, bad_P, bad_words, 1, fill=FILL)
            assert st == _lib.DMF_ERR_INVALID and n == FILL and (sel == FILL).all(), (bad_P, bad_words)
        sel, n = np.full(P + 5, FILL, np.int32), C.c_int32(FILL)
        call = dc.L.dmf_greedy_set_cover_masks_device
        assert call(dc.h, d_masks, P, words, 1, None, C.addressof(n)) == _lib.DMF_ERR_INVALID and n.value == FILL
        assert call(dc.h, d_masks, P, words, 1, sel.ctypes.data, None) == _lib.DMF_ERR_INVALID
        assert call(dc.h, None, P, words, 1, sel.ctypes.data, C.addressof(n)) == _lib.DMF_ERR_INVALID
        raw = dmf_amd.VoxelVolume()
        assert raw._L.dmf_greedy_set_cover_masks_device(raw._h, d_masks, P, words, 1, sel.ctypes.data,
                                                        C.addressof(n)) == _lib.DMF_ERR_STATE
        assert (sel == FILL).all() and n.value == FILL
        _check(dc, d_masks, masks, "min_gain_boundary")      # and the volume still serves
    finally:
        dc.close()
