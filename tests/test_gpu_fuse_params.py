"""GPU: fusion across its parameter space -- the counter plane, the depth gate, degenerate rays.

The other GPU modules run fusion at one point of dmf_fuse_params (the default log-odds, a gate
of 200 mm and up, counters in the low thousands).  Here:

A. finalize (k_finalize, k_counter_layout, finalize_tiles on a slab) against int64 numpy
   arithmetic, with counters at the 2^23 / 2^24 / 2^31 edges and on either side of the counts at
   which hits * 847 and misses * 405 leave int32, clamps at the int16 edges and degenerate,
   garbage in every padding element of the tiled layout, sentinels behind the int16 output;
B. the clamps every finalize entry point rejects, output and counters untouched;
C. the depth gate ([dmin, dmax) over any int32 pair) and the rays it lets in that a 200 mm gate
   never does: d = 0 (start = end, dq = 0 on every axis), one-cell rays, 65 m rays clipped at the
   far face, a whole frame into one cell (phase F's 16-bit LDS fields at kBkPartMax pairs),
   grids one or two cells thin, and accumulation onto counters that are not small.

Every comparison is exact equality.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import helpers as Hh

pytestmark = pytest.mark.gpu

I32_MIN, I32_MAX = -(2 ** 31), 2 ** 31 - 1


@pytest.fixture(scope="module")
def dmf():
    import dmf_amd
    return dmf_amd


@pytest.fixture(scope="module")
def engine(dmf):
    """The 64x48 camera Ka of the gate / thin-grid cases."""
    return dmf.RayTracingEngine(dmf.Camera(KA, HA, WA))


# ============================================================================ A. finalize
GRIDS = [(1, 1, 1), (1, 1, 5), (2, 2, 4), (3, 5, 7), (5, 3, 2), (33, 2, 9), (61, 61, 61)]
# (l_hit, l_miss, l_min, l_max)
PARAMS = [(847, -405, -2000, 3511), (32767, -32768, -32768, 32767), (1, -1, -1, 1), (-3, 5, 0, 0), (7, 7, -7, -7),
          (I32_MAX, -I32_MAX, -32768, 32767), (0, 0, -5, 5)]
# 2 535 000 / 2 536 000: hits * 847 passes 2^31 between them; 5 302 000 / 5 303 000: misses * 405
EDGE_COUNTS = [0, 1, -1, 2 ** 23 - 1, 2 ** 23, 2 ** 24 + 1, 2535000, 2536000, 5302000, 5303000, I32_MAX, I32_MIN]
SENTINEL = 12345  # int16 fill of outputs: an element the kernel left alone shows


@functools.lru_cache(maxsize=None)
def _counters(dims):
    """[(hits, misses), ...] linear int32 counters of a grid: every cell is an EDGE_COUNTS value
    or a random int32 (seeded).  Over the rounds of a grid every EDGE_COUNTS value and a random
    one appears in hits and in misses (one round for grids of >= 26 cells; grids of fewer cells
    take several rounds), and hits and misses pair the values differently."""
    n = int(np.prod(dims))
    rng = np.random.default_rng(1000 + n)
    nv = len(EDGE_COUNTS) + 1  # index nv - 1: a random int32
    rounds = max(1, -(-2 * nv // n))
    rand = rng.integers(I32_MIN, I32_MAX, (2, rounds * n), endpoint=True)
    pick = rng.integers(0, nv, (2, rounds * n))
    pick[0, : 2 * nv] = np.arange(2 * nv) % nv           # every value twice in hits ...
    pick[1, : 2 * nv] = (np.arange(2 * nv) * 5 + 3) % nv  # ... and in misses, against other partners
    if n >= 2 * nv:  # one round: the forced head is spread over the grid
        perm = rng.permutation(n)
        pick, rand = pick[:, perm], rand[:, perm]
    vals = np.array(EDGE_COUNTS + [0], np.int64)
    out = np.where(pick == nv - 1, rand, vals[pick]).astype(np.int32)
    res = [(np.ascontiguousarray(out[0, r * n:(r + 1) * n]), np.ascontiguousarray(out[1, r * n:(r + 1) * n]))
           for r in range(rounds)]
    for k in (0, 1):
        allv = np.concatenate([r[k] for r in res])
        assert all((allv == v).any() for v in EDGE_COUNTS) and not np.isin(allv, EDGE_COUNTS).all()
    for a in res:
        for b in a:
            b.setflags(write=False)
    return res


def _exact(h, m, prm):
    """The reference: clip(h*l_hit + m*l_miss, l_min, l_max) in int64 (it fits: |counter| <= 2^31
    and |l_hit| + |l_miss| <= 2^32 - 2 bound the sum by 2^63 - 2^32)."""
    l_hit, l_miss, l_min, l_max = prm
    assert abs(l_hit) + abs(l_miss) <= 2 ** 32 - 2
    return np.clip(h.astype(np.int64) * l_hit + m.astype(np.int64) * l_miss, l_min, l_max).astype(np.int16)


def _prm(p, **kw):
    from dmf_amd import _lib
    return _lib.default_fuse_params(l_hit=p[0], l_miss=p[1], l_min=p[2], l_max=p[3], **kw)


def _empty_volume(dims):
    return Hh.gpu_grid(dims)


def _poisoned_tiled(lin, dims, n_pad, seed):
    """dist.to_tiled(lin) with every padding element (of partial tiles and past the tiled cells up
    to n_pad) overwritten: 0x7fffffff and random non-zero values alternate.  Returns (tiled,
    mask of the real cells)."""
    from dmf_amd import dist
    t = dist.to_tiled(lin, dims, n_pad)
    real = dist.to_tiled(np.ones(int(np.prod(dims)), np.int32), dims, n_pad).astype(bool)
    rng = np.random.default_rng(seed)
    junk = rng.integers(1, I32_MAX, n_pad, endpoint=True).astype(np.int32)
    junk[::2] = I32_MAX
    junk[rng.random(n_pad) < 0.25] *= -1
    assert (junk != 0).all()
    return np.where(real, t, junk), real


@pytest.mark.parametrize("dims", GRIDS, ids=lambda d: "x".join(map(str, d)))
def test_finalize_exact(oracle, dmf, dims):
    """dmf_fuse_finalize (host, through k_counter_layout<false>), dmf_fuse_finalize_device on tiled
    counters with poisoned padding and a guarded output, and dmf_fuse_counters_to_linear_device
    on the same arrays, for every parameter set: equal to int64 numpy arithmetic, as is the
    oracle's finalize."""
    from dmf_amd import _lib
    gv = _empty_volume(dims)
    L, h = gv._L, gv._h
    eng = dmf.RayTracingEngine(dmf.Camera(KA, HA, WA))
    ncell = int(np.prod(dims))
    n_pad = _lib.merge_plan(gv, 8, -1)["n_padded"]  # padded for 8 ranks: elements past the tiled cells
    nt = C.c_int64()
    _lib.check(L.dmf_fuse_counter_cells(h, C.addressof(nt)))
    assert ncell <= nt.value <= n_pad
    dc = Hh.DeviceCalls(gv)
    try:
        for rnd, (hl, ml) in enumerate(_counters(dims)):
            (ht, real), (mt, _) = _poisoned_tiled(hl, dims, n_pad, 7 + rnd), _poisoned_tiled(ml, dims, n_pad, 70 + rnd)
            assert int(real.sum()) == ncell and (n_pad == ncell or not real.all())
            d_h, d_m, d_lin = dc.upload(ht), dc.upload(mt), dc.alloc(4 * ncell)
            for src, exp in ((d_h, hl), (d_m, ml)):
                _lib.check(L.dmf_memset_device(h, d_lin, 0x5a, 4 * ncell))
                _lib.check(L.dmf_fuse_counters_to_linear_device(h, src, d_lin))
                assert np.array_equal(dc.download(d_lin, ncell, np.int32), exp)
            for p in PARAMS:
                ref = _exact(hl, ml, p)
                assert np.array_equal(oracle.fuse_finalize(hl, ml, *p), ref), p
                assert np.array_equal(eng.fuse_finalize(gv, hl, ml, _prm(p)), ref), p
                guard = np.full(ncell + 64, SENTINEL, np.int16)
                d_out = dc.upload(guard)
                prm = _prm(p)
                _lib.check(L.dmf_fuse_finalize_device(h, d_h, d_m, C.addressof(prm), d_out))
                got = dc.download(d_out, ncell + 64, np.int16)
                assert np.array_equal(got[:ncell], ref), p
                assert (got[ncell:] == SENTINEL).all(), p
            # the counters were only read
            assert np.array_equal(dc.download(d_h, n_pad, np.int32), ht)
            assert np.array_equal(dc.download(d_m, n_pad, np.int32), mt)
    finally:
        dc.close()


@pytest.mark.parametrize("G", [2, 3, 8])
@pytest.mark.parametrize("dims", [(3, 5, 7), (33, 2, 9), (61, 61, 61)], ids=lambda d: "x".join(map(str, d)))
def test_finalize_slab_exact(dmf, dims, G):
    """dmf_fuse_finalize_slab_device for every rank r of G emulated ranks (the pattern of
    test_merge_slabs_emulated_ranks) against int64 numpy arithmetic: rank r's buffer holds the
    counters only in its own chunk (dmf_fuse_merge_plan) and garbage everywhere else, padding
    included; its slab of the sentinel-filled output equals the reference and nothing else is
    written; the slabs tile the padded grid."""
    from dmf_amd import _lib
    gv = _empty_volume(dims)
    L, h = gv._L, gv._h
    ncell = int(np.prod(dims))
    whole = _lib.merge_plan(gv, G, -1)
    n_pad, nlo = whole["n_padded"], whole["logodds_padded"]
    assert whole == _lib.merge_plan_dims(dims, G, -1)
    hl, ml = _counters(dims)[0]
    ht, mt = _poisoned_tiled(hl, dims, n_pad, 11)[0], _poisoned_tiled(ml, dims, n_pad, 12)[0]
    dc = Hh.DeviceCalls(gv)
    try:
        for p in (PARAMS[1], PARAMS[3]):
            ref = _exact(hl, ml, p)
            prm = _prm(p)
            gathered = np.full(nlo, -7, np.int16)
            covered = 0
            for r in range(G):
                pl = _lib.merge_plan(gv, G, r)
                assert pl == _lib.merge_plan_dims(dims, G, r)
                a, n = pl["chunk_offset"], pl["chunk"]
                rng = np.random.default_rng(100 * G + r)
                buf = rng.integers(I32_MIN, I32_MAX, 2 * n_pad, endpoint=True).astype(np.int32)
                buf[a:a + n] = ht[a:a + n]
                buf[n_pad + a:n_pad + a + n] = mt[a:a + n]
                d_buf, d_lo = dc.upload(buf), dc.upload(np.full(nlo, SENTINEL, np.int16))
                _lib.check(L.dmf_fuse_finalize_slab_device(h, d_buf, C.addressof(prm), d_lo, G, r, None))
                lo = dc.download(d_lo, nlo, np.int16)
                s0, sb = pl["slab_offset"] // 2, pl["slab_bytes"] // 2
                expect = np.full(nlo, SENTINEL, np.int16)
                s1 = min(s0 + sb, ncell)
                if s1 > s0:
                    expect[s0:s1] = ref[s0:s1]
                assert np.array_equal(lo, expect), (p, r)
                assert np.array_equal(dc.download(d_buf, 2 * n_pad, np.int32), buf), (p, r)
                gathered[s0:s0 + sb] = lo[s0:s0 + sb]
                covered += sb
                dc.close()
            assert covered == nlo
            assert np.array_equal(gathered[:ncell], ref), p
    finally:
        dc.close()


# ============================================================================ B. validation
BAD_CLAMPS = [(1, 0), (3511, -2000), (-32769, 0), (0, 32768), (-32769, 32768), (I32_MIN, I32_MAX), (32768, 32768),
              (-32769, -32769)]


@pytest.mark.parametrize("l_min,l_max", BAD_CLAMPS)
def test_finalize_rejects_invalid_clamp(dmf, l_min, l_max):
    """l_min > l_max, l_min < -32768 or l_max > 32767 through the four finalize entry points at
    world size 1: DMF_ERR_INVALID with a message, the output and the counters untouched."""
    from dmf_amd import _lib
    dims = (5, 3, 2)
    gv = _empty_volume(dims)
    L, h = gv._L, gv._h
    ncell = int(np.prod(dims))
    hl, ml = _counters(dims)[0]
    prm = _prm((847, -405, l_min, l_max))
    pa = C.addressof(prm)
    n_pad, nlo = _lib.merge_plan(gv, 1, -1)["n_padded"], _lib.merge_plan(gv, 1, -1)["logodds_padded"]
    ht, mt = _poisoned_tiled(hl, dims, n_pad, 1)[0], _poisoned_tiled(ml, dims, n_pad, 2)[0]
    both = np.concatenate([ht, mt])

    def rejected(status):
        assert status == _lib.DMF_ERR_INVALID, status
        msg = L.dmf_last_error().decode()
        assert "l_min" in msg and str(l_min) in msg and str(l_max) in msg, msg

    out = np.full(ncell, SENTINEL, np.int16)
    h0, m0 = hl.copy(), ml.copy()
    rejected(L.dmf_fuse_finalize(h, h0.ctypes.data, m0.ctypes.data, pa, out.ctypes.data))
    assert (out == SENTINEL).all() and np.array_equal(h0, hl) and np.array_equal(m0, ml)
    with pytest.raises(dmf.DmfError):
        dmf.RayTracingEngine(dmf.Camera(KA, HA, WA)).fuse_finalize(gv, hl, ml, prm)
    dc = Hh.DeviceCalls(gv)
    try:
        d_c, d_lo = dc.upload(both), dc.upload(np.full(nlo + 64, SENTINEL, np.int16))
        for call in (lambda: L.dmf_fuse_finalize_device(h, d_c, d_c + 4 * n_pad, pa, d_lo),
                     lambda: L.dmf_fuse_finalize_slab_device(h, d_c, pa, d_lo, 1, 0, None),
                     lambda: L.dmf_fuse_finalize_slab_device(h, d_c, pa, d_lo, 1, -1, None),
                     lambda: L.dmf_fuse_merge_finalize_device(h, d_c, pa, d_lo, None, None)):
            rejected(call())
            assert (dc.download(d_lo, nlo + 64, np.int16) == SENTINEL).all()
            assert np.array_equal(dc.download(d_c, 2 * n_pad, np.int32), both)
        # the same buffers with the clamp at the int16 edges are accepted
        ok = _prm((847, -405, -32768, 32767))
        _lib.check(L.dmf_fuse_merge_finalize_device(h, d_c, C.addressof(ok), d_lo, None, None))
        got = dc.download(d_lo, nlo + 64, np.int16)
        assert np.array_equal(got[:ncell], _exact(hl, ml, (847, -405, -32768, 32767)))
    finally:
        dc.close()


# ============================================================================ C. gate, degenerate rays
KA = np.array([50.0, 0.0, 32.0, 0.0, 50.0, 24.0, 0.0, 0.0, 1.0], np.float32)
HA, WA = 48, 64
PERM = [[0, 0, 1], [1, 0, 0], [0, 1, 0]]  # camera z along world x
DISPATCHES = [(256, 0), (96, 57), (96, 40), (96, 31)]
SLAB_KERNEL = "dmf::k_bk_fuse_s<16, 32, 8>"


def _pose(R, t):
    return np.concatenate([np.asarray(R, np.float32), np.asarray(t, np.float32)[:, None]], 1).reshape(12)


@functools.lru_cache(maxsize=None)
def _gate_poses():
    """Two cameras inside the grid, one 0.3 mm outside the z = -0.5 face looking in, one 0.4 m outside."""
    return np.stack([_pose(np.eye(3), [0.013, -0.02, 0.1]), _pose(PERM, [-0.3, 0.2, 0.0]),
                     _pose(np.eye(3), [0.0, 0.0, -0.5003]), _pose(np.eye(3), [0.0, 0.0, -0.9])])


@functools.lru_cache(maxsize=None)
def _gate_cases():
    """[(name, depth (4, 48, 64) uint16, dmin, dmax)]."""
    rng = np.random.default_rng(2024)
    shape = (4, HA, WA)
    zeros = np.zeros(shape, np.uint16)
    short = rng.integers(0, 40, shape).astype(np.uint16)
    far = rng.integers(60000, 65536, shape).astype(np.uint16)
    far[:, 5, 7] = 65535  # rejected by d < 65535
    mid = rng.integers(0, 2000, shape).astype(np.uint16)
    cases = [("zeros", zeros, 0, 65535), ("zeros_negative_dmin", zeros, -5, 65535), ("zeros_default_gate", zeros, 1, 65535),
             ("short", short, 1, 65535), ("far", far, 1, 65535),
             ("far_65536", np.full(shape, 65535, np.uint16), 1, 65536),
             ("empty_gate", mid, 1000, 1000), ("inverted_gate", mid, 1000, 200),
             ("gate_int32_all", short, I32_MIN, I32_MAX), ("gate_int32_inverted", short, I32_MAX, I32_MIN)]
    for dmin, dmax in ((1, 2), (999, 1000), (65534, 65535)):
        row = np.array([dmin - 1, dmin, dmax - 1, dmax], np.uint16)[np.arange(WA) % 4]
        cases.append((f"gate_edges_{dmin}_{dmax}", np.broadcast_to(row, shape).copy(), dmin, dmax))
    for _, d, _, _ in cases:
        d.setflags(write=False)
    return cases


def _sparse(a):
    i = np.flatnonzero(a)
    return i, a[i].copy()


def _same(sp, a):
    i = np.flatnonzero(a)
    return np.array_equal(i, sp[0]) and np.array_equal(a[i], sp[1])


_GATE_ORACLE = {}


def _gate_oracle(O, n):
    """{name: (hits, misses as (index, value) of the non-zero cells, stats)} of the gate cases on
    an n^3 grid, computed once and shared by the dispatches."""
    if n not in _GATE_ORACLE:
        ov = Hh.oracle_grid(O, n)
        res = {}
        for name, D, dmin, dmax in _gate_cases():
            ho, mo, so = O.fuse_depth(ov, KA, D, _gate_poses(), dmin=dmin, dmax=dmax)
            res[name] = (_sparse(ho), _sparse(mo), so)
        _GATE_ORACLE[n] = res
    return _GATE_ORACLE[n]


def _one_cell_rays(O, n, D, poses, dmin, dmax):
    """Rays of the oracle with exactly one update (start cell = end cell), counted per pixel: each
    valid pixel is fused alone (the counters are scratch, only the update count is read)."""
    ov = Hh.oracle_grid(O, n)
    hb, mb = np.zeros(n ** 3, np.int32), np.zeros(n ** 3, np.int32)
    frame = np.zeros((1, HA, WA), np.uint16)
    count = 0
    for p in range(len(poses)):
        for r, c in zip(*np.nonzero((D[p] >= dmin) & (D[p] < dmax))):
            frame[0, r, c] = D[p, r, c]
            count += int(O.fuse_depth(ov, KA, frame, poses[p:p + 1], dmin=dmin, dmax=dmax, hits=hb, misses=mb)[2][0] == 1)
            frame[0, r, c] = 0
    return count


def test_gate_cases_are_not_vacuous(oracle):
    """The oracle's numbers of the gate cases at n = 96: what each case is there for happens."""
    res = _gate_oracle(oracle, 96)
    cases = {c[0]: c for c in _gate_cases()}
    npix = 4 * HA * WA
    (hz, mz, sz) = res["zeros"]
    assert list(sz) == [6144, 12288, 6144] and len(hz[0]) == 2 and list(hz[1]) == [3072, 3072] and len(mz[0]) == 0
    hn, mn, sn = res["zeros_negative_dmin"]
    assert np.array_equal(sn, sz) and np.array_equal(hn[0], hz[0]) and np.array_equal(hn[1], hz[1]) and len(mn[0]) == 0
    assert list(res["zeros_default_gate"][2]) == [0, 0, 0]
    ss = res["short"][2]
    assert 0 < ss[0] < 4 * ss[1], ss
    _, D, dmin, dmax = cases["short"]
    assert _one_cell_rays(oracle, 96, D, _gate_poses(), dmin, dmax) > 1000
    hf, mf, sf = res["far"]
    assert sf[2] == 0 and len(hf[0]) == 0 and 1.0e6 < sf[0] < 1.6e6, sf
    assert sf[1] == int((cases["far"][1] < 65535).sum()) < npix
    assert res["far_65536"][2][1] == npix and res["far_65536"][2][0] > 0
    for name in ("empty_gate", "inverted_gate", "gate_int32_inverted"):
        h, m, s = res[name]
        assert list(s) == [0, 0, 0] and len(h[0]) == 0 and len(m[0]) == 0
    sa = res["gate_int32_all"][2]
    assert sa[1] == npix and sa[0] > ss[0]  # d = 0 is admitted as well
    for name, (_, D, dmin, dmax) in cases.items():
        if name.startswith("gate_edges"):
            assert res[name][2][1] == int((D == dmin).sum()) == npix // 2, name


@pytest.mark.parametrize("n,variant", DISPATCHES)
def test_gate_cases(oracle, dmf, engine, n, variant):
    """Every gate case through the default dispatch at 256^3 (the production slab-walk brick
    pipeline) and variants 57, 40 and 31 at 96^3: counters and stats[0:3] equal the oracle's."""
    from dmf_amd import _lib
    res = _gate_oracle(oracle, n)
    gv = _empty_volume(n)
    _lib.set_variant(gv, variant)
    for name, D, dmin, dmax in _gate_cases():
        ho, mo, so = res[name]
        hg, mg, sg = engine.fuse_depth(gv, D, _gate_poses(), dmf.FuseParams(dmin_mm=dmin, dmax_mm=dmax))
        if n == 256 and so[0] > 0:
            assert _lib.kernel_name(gv) == SLAB_KERNEL, name
        assert np.array_equal(so, sg), (name, so, sg)
        assert _same(ho, hg) and _same(mo, mg), name
        assert _lib.fuse_status(gv) == 0


@functools.lru_cache(maxsize=None)
def _one_cell_poses(n):
    """Two cameras at the centre of cell n/2, identity and permuted rotation."""
    t = [0.5 / n] * 3
    return np.stack([_pose(np.eye(3), t), _pose(PERM, t)])


def _one_cell_cases(n):
    """[(name, depth, poses, dmin, dmax, rays)]: 640x480 frames of constant depth 1 (every hit in
    the camera's cell) or 600 (every ray's first miss there).  `whole`: two full frames, 614 400
    rays.  65535 / 65536: one frame whose first that many pixels are valid and the rest 0."""
    poses = _one_cell_poses(n)
    cases = [("hits_whole", np.full((2, 480, 640), 1, np.uint16), poses, 0, 65535, 614400),
             ("misses_whole", np.full((2, 480, 640), 600, np.uint16), poses, 200, 1000, 614400)]
    for k, N in enumerate((65535, 65536)):
        for name, d, dmin, dmax in (("hits", 1, 1, 65535), ("misses", 600, 200, 1000)):
            D = np.zeros(480 * 640, np.uint16)
            D[:N] = d
            cases.append((f"{name}_{N}", D.reshape(1, 480, 640), poses[k:k + 1], dmin, dmax, N))
    return cases


_ONE_CELL_ORACLE = {}


def _one_cell_oracle(O, n):
    from dmf_amd import scene
    if n not in _ONE_CELL_ORACLE:
        ov = Hh.oracle_grid(O, n)
        out = []
        for name, D, poses, dmin, dmax, rays in _one_cell_cases(n):
            ho, mo, so = O.fuse_depth(ov, scene.intrinsics(640, 480), D, poses, dmin=dmin, dmax=dmax, threads=8)
            out.append((name, D, poses, dmin, dmax, rays, _sparse(ho), _sparse(mo), so))
        _ONE_CELL_ORACLE[n] = out
    return _ONE_CELL_ORACLE[n]


@pytest.mark.parametrize("n,variant", DISPATCHES)
def test_one_cell_takes_every_ray(oracle, dmf, n, variant):
    """Every ray of a call adds to one counter of one cell: its hit (depth 1 mm from the centre of
    a cell) or its first miss (depth 600, gate (200, 1000)).  At 256^3 that cell's brick takes
    one pair per ray, and phase F adds each part's pairs into one 16-bit field of one LDS word
    (misses low, hits high).  A brick's pairs are cut evenly into ceil(pairs / kBkPartMax) parts,
    kBkPartMax = 65 535, so that no field carries:
      * 614 400 rays (two whole frames): 10 parts of 61 440;
      * 65 535 rays: one part, the field ends at 0xffff -- the exact edge of 'never carries';
      * 65 536 rays: two parts of 32 768 (one part of 65 536 would wrap the hits field to 0, or
        carry the misses field into the hits)."""
    from dmf_amd import _lib, scene
    cell = ((n // 2) * n + n // 2) * n + n // 2
    gv = _empty_volume(n)
    _lib.set_variant(gv, variant)
    eng = dmf.RayTracingEngine(dmf.Camera(scene.intrinsics(640, 480), 480, 640))
    for name, D, poses, dmin, dmax, rays, ho, mo, so in _one_cell_oracle(oracle, n):
        if name.startswith("hits"):
            assert list(so) == [rays, rays, rays] and list(ho[0]) == [cell] and list(ho[1]) == [rays], name
            assert len(mo[0]) == 0, name
        else:
            k = int(np.searchsorted(mo[0], cell))
            assert so[1] == rays and mo[0][k] == cell and mo[1][k] == rays == mo[1].max(), name
        hg, mg, sg = eng.fuse_depth(gv, D, poses, dmf.FuseParams(dmin_mm=dmin, dmax_mm=dmax))
        if n == 256:
            assert _lib.kernel_name(gv) == SLAB_KERNEL
        assert np.array_equal(so, sg), (name, so, sg)
        assert _same(ho, hg) and _same(mo, mg), (name, int(hg[cell]), int(mg[cell]))
        assert (hg[cell] if name.startswith("hits") else mg[cell]) == rays, name
        assert _lib.fuse_status(gv) == 0


# dims -> the oracle's updates (3 frames of scene.render under the default gate)
THIN = {(1, 1, 1): 4387, (1, 37, 5): 49245, (96, 96, 1): 240721, (2, 256, 64): 356947, (256, 3, 2): 364863,
        (33, 2, 9): 59888, (2048, 2, 2): 2878780}


@functools.lru_cache(maxsize=None)
def _thin_inputs():
    from dmf_amd import scene
    poses = scene.fibonacci_poses(3, seed=5)
    depth = np.stack([scene.render(KA, WA, HA, T)[0] for T in poses]).astype(np.uint16)
    depth.setflags(write=False)
    return poses, depth


@pytest.mark.parametrize("dims", list(THIN), ids=lambda d: "x".join(map(str, d)))
def test_thin_grids(oracle, dmf, engine, dims):
    """Grids one or two cells thin under the library's default gate (1 <= d < 65535): the default
    dispatch, and variants 57 and 40 wherever dmf_fuse_plan says the brick pipeline applies."""
    from dmf_amd import _lib
    poses, depth = _thin_inputs()
    ov = Hh.oracle_grid(oracle, dims)
    ho, mo, so = oracle.fuse_depth(ov, KA, depth, poses)
    assert list(so) == [THIN[dims], 4387, 4263]
    cam = _lib.make_camera(KA, HA, WA)
    ran = []
    for variant in (0, 57, 40):
        gv = _empty_volume(dims)
        _lib.set_variant(gv, variant)
        if variant and not _lib.fuse_plan(gv, cam, len(poses))["brick"]:
            continue
        hg, mg, sg = engine.fuse_depth(gv, depth, poses, dmf.FuseParams())
        assert np.array_equal(so, sg), (variant, so, sg)
        assert np.array_equal(ho, hg) and np.array_equal(mo, mg), variant
        assert _lib.fuse_status(gv) == 0
        ran.append(variant)
    assert ran == ([0] if max(dims) > 1024 else [0, 57, 40])


@pytest.mark.parametrize("n,variant", DISPATCHES)
def test_fusion_accumulates_onto_large_counters(oracle, dmf, engine, n, variant):
    """'hits / misses are ACCUMULATED (the caller zeroes)': counters preloaded with seeded random
    int32 in [-2^30, 2^30], host form and device form (tiled, padding poisoned), take the `short`
    gate case and an edge case of test_fuse_edge_cases; the result is the preload plus the
    oracle's counters from zero, and a second call into the same buffers adds them again."""
    from dmf_amd import _lib, dist
    from test_gpu_parity import _edge_fusion_cases
    short = next(c for c in _gate_cases() if c[0] == "short")
    edge = next(c for c in _edge_fusion_cases() if c[0] == "axis_ramp")
    runs = [(KA, HA, WA, _gate_poses(), short[1], short[2], short[3]),
            (edge[1], edge[2], edge[3], np.ascontiguousarray(edge[4], np.float32), edge[5], 200, 1000)]
    ncell = n ** 3
    rng = np.random.default_rng(77)
    pre_h = rng.integers(-(2 ** 30), 2 ** 30, ncell, endpoint=True).astype(np.int32)
    pre_m = rng.integers(-(2 ** 30), 2 ** 30, ncell, endpoint=True).astype(np.int32)
    gv = _empty_volume(n)
    _lib.set_variant(gv, variant)
    L, h = gv._L, gv._h
    ov = Hh.oracle_grid(oracle, n)
    nt = C.c_int64()
    _lib.check(L.dmf_fuse_counter_cells(h, C.addressof(nt)))
    nt = nt.value
    # host form
    hh, mh = pre_h.copy(), pre_m.copy()
    exp_h, exp_m = pre_h.copy(), pre_m.copy()
    dc = Hh.DeviceCalls(gv)
    try:
        # device form: tiled, padding poisoned (16 spare elements behind the tiled cells)
        ht, real = _poisoned_tiled(pre_h, (n, n, n), nt + 16, 5)
        mt, _ = _poisoned_tiled(pre_m, (n, n, n), nt + 16, 6)
        d_h, d_m, d_lin = dc.upload(ht), dc.upload(mt), dc.alloc(4 * ncell)
        for Kc, Hc, Wc, P, D, dmin, dmax in runs:
            ho, mo, so = oracle.fuse_depth(ov, Kc, D, P, dmin=dmin, dmax=dmax)
            assert so[0] > 0
            eng = dmf.RayTracingEngine(dmf.Camera(Kc, Hc, Wc))
            prm = dmf.FuseParams(dmin_mm=dmin, dmax_mm=dmax)
            cam = _lib.make_camera(Kc, Hc, Wc)
            d_d, d_p = dc.upload(np.ascontiguousarray(D, np.uint16)), dc.upload(P)
            for _ in range(2):  # the second call adds the same counts again
                exp_h += ho
                exp_m += mo
                _, _, sg = eng.fuse_depth(gv, D, P, prm, hits=hh, misses=mh)
                assert np.array_equal(sg, so)
                assert np.array_equal(hh, exp_h) and np.array_equal(mh, exp_m)
                d_st = dc.zeros(8 * 32)
                _lib.check(L.dmf_fuse_depth_device(h, C.addressof(cam), d_d, d_p, len(P), C.addressof(prm), d_h, d_m, d_st))
                assert np.array_equal(dc.download(d_st, 3, np.uint64).astype(np.int64), so)
                for src, exp in ((d_h, exp_h), (d_m, exp_m)):
                    _lib.check(L.dmf_fuse_counters_to_linear_device(h, src, d_lin))
                    assert np.array_equal(dc.download(d_lin, ncell, np.int32), exp)
                assert _lib.fuse_status(gv) == 0
        # the padding elements are as they were
        for src, t0 in ((d_h, ht), (d_m, mt)):
            got = dc.download(src, nt + 16, np.int32)
            assert np.array_equal(got[~real], t0[~real])
        assert np.array_equal(dist.to_tiled(exp_h, (n, n, n), nt + 16)[real], dc.download(d_h, nt + 16, np.int32)[real])
    finally:
        dc.close()
