"""GPU: pipelined fusion (dmf_fuse_set_input_stream).

With an input stream declared, each call's pose table, pass A, batch layout and pass B run
on the volume's staging stream into one of two slots and overlap the previous call's
phase F.  The counters and statistics must equal the serial order's exactly, also when
* the inputs are rewritten on the input stream before every call (the call must have made
  the input stream wait for its pass A),
* a call spans several super-batches (DMF_KNOB_SUPER_POSES: the slots alternate inside the
  call, slot reuse waits for the super-batch two back),
* the device cuts a super-batch into several pose batches (DMF_KNOB_BATCH_POSES: batch j+1's
  pass B after batch j's phase F),
* serial and pipelined calls are mixed on one volume with no synchronisation between them
  (a pipelined call must wait for the serial calls that used its slot),
and at 128^3 the sum over the calls equals the oracle's counters.  At the bench's own shape
(512^3, 128 frames of 640x480 per call: the timed mode of bench.py) several pipelined calls
equal the serial calls and the committed oracle digest (tests/golden/fusion_digests.json).
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

import helpers as Hh

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fusion_digests.json")


def _frames(P, seed=77):
    from dmf_amd import scene
    poses = np.ascontiguousarray(scene.fibonacci_poses(P, seed=seed), np.float32)
    depth = np.ascontiguousarray(scene.render_frames(scene.intrinsics(640, 480), 640, 480, poses), np.uint16)
    return poses, depth


class _Vol:
    """A device-API fusion volume with its own main / input streams."""

    def __init__(self, n, per_call, knobs=None, variant=0):
        import torch
        import dmf_amd
        from dmf_amd import _lib, scene
        self.torch, self._lib, self.L = torch, _lib, _lib.load()
        self.dev = torch.device("cuda", 0)
        self.vol = dmf_amd.VoxelVolume()
        self.vol.setDimensions(*Hh.BOUNDS)
        self.vol.setVolumeSize(n, n, n)
        self.vol.constructVolume()
        self.n = n
        self.main = torch.cuda.Stream(self.dev)
        self.inp = torch.cuda.Stream(self.dev)
        self.vol.set_stream(self.main.cuda_stream)
        self.cam = _lib.make_camera(scene.intrinsics(640, 480), 480, 640)
        self.prm = _lib.default_fuse_params(dmin_mm=scene.DEPTH_MIN_MM, dmax_mm=scene.DEPTH_MAX_MM)
        nct = C.c_int64()
        _lib.check(self.L.dmf_fuse_counter_cells(self.vol._h, C.addressof(nct)))
        self.nt = nct.value
        self.per_call = per_call
        _lib.set_variant(self.vol, variant)
        for k, v in (knobs or {}).items():
            _lib.set_knob(self.vol, k, v)
        self.counters = torch.zeros(2 * self.nt, dtype=torch.int32, device=self.dev)
        self.stats = torch.zeros(8, dtype=torch.int64, device=self.dev)

    def pipelined(self, on):
        self._lib.check(self.L.dmf_fuse_set_input_stream(self.vol._h, self.inp.cuda_stream if on else None))

    def reserve(self):
        self._lib.check(self.L.dmf_fuse_reserve(self.vol._h, C.addressof(self.cam), self.per_call, 0))

    def call(self, d_depth, d_poses):
        self._lib.check(self.L.dmf_fuse_depth_device(
            self.vol._h, C.addressof(self.cam), d_depth.data_ptr(), d_poses.data_ptr(), self.per_call,
            C.addressof(self.prm), self.counters.data_ptr(), self.counters.data_ptr() + 4 * self.nt,
            self.stats.data_ptr()))

    def linear(self):
        torch = self.torch
        torch.cuda.synchronize(self.dev)
        lin = torch.empty(self.n ** 3, dtype=torch.int32, device=self.dev)
        out = []
        for half in range(2):
            self._lib.check(self.L.dmf_fuse_counters_to_linear_device(
                self.vol._h, self.counters.data_ptr() + 4 * self.nt * half, lin.data_ptr()))
            self.vol.synchronize()
            out.append(lin.cpu().numpy())
        return out[0], out[1], self.stats.cpu().numpy()

    def logodds_digest(self):
        """sha256[:16] of the finalized int16 grid (bench.py logodds_digest)."""
        import hashlib
        torch = self.torch
        torch.cuda.synchronize(self.dev)
        lo = torch.empty(self.n ** 3, dtype=torch.int16, device=self.dev)
        self._lib.check(self.L.dmf_fuse_finalize_device(self.vol._h, self.counters.data_ptr(),
                                                        self.counters.data_ptr() + 4 * self.nt,
                                                        C.addressof(self.prm), lo.data_ptr()))
        self.vol.synchronize()
        return hashlib.sha256(lo.cpu().numpy().tobytes()).hexdigest()[:16]

    def close(self):
        self.pipelined(False)
        self.vol.close()


def _run(n, poses, depth, per_call, pipelined, variant=0, knobs=None):
    """Calls of per_call frames through ONE input buffer rewritten before every call (on the
    input stream when pipelined)."""
    v = _Vol(n, per_call, knobs, variant)
    torch = v.torch
    all_depth = torch.from_numpy(depth.view(np.int16)).to(v.dev)
    all_poses = torch.from_numpy(poses).to(v.dev)
    d_depth = torch.empty_like(all_depth[:per_call])
    d_poses = torch.empty_like(all_poses[:per_call])
    torch.cuda.synchronize(v.dev)
    try:
        if pipelined:
            v.pipelined(True)
        v.reserve()
        for c0 in range(0, poses.shape[0], per_call):
            with torch.cuda.stream(v.inp if pipelined else v.main):
                d_depth.copy_(all_depth[c0:c0 + per_call])
                d_poses.copy_(all_poses[c0:c0 + per_call])
            v.call(d_depth, d_poses)
        return v.linear()
    finally:
        v.close()


@pytest.mark.parametrize("case", ["calls", "super2", "super1_batches", "hash_overflow_batches"])
def test_pipelined_equals_serial_256(case):
    """256^3 (the default brick pipeline), 4 calls of 3 frames.  hash_overflow_batches: pass
    A's hashed histogram forced with 64 words (most workgroups overflow and are redone by
    k_bk_rays_recover) and three device batches per super-batch (batches j > 0 on the
    volume's stream)."""
    poses, depth = _frames(12)
    knobs = {"calls": {}, "super2": {"super_poses": 2},  # 3 frames -> super-batches of 2 + 1
             "super1_batches": {"super_poses": 3, "batch_poses": 1},  # three device batches each
             "hash_overflow_batches": {"super_poses": 3, "batch_poses": 1, "a_hash": 64}}[case]
    hs, ms, ss = _run(256, poses, depth, 3, pipelined=False, knobs=knobs)
    hp, mp, sp = _run(256, poses, depth, 3, pipelined=True, knobs=knobs)
    assert ss[0] > 10 ** 7 and ss[3] == 0
    # stats[5] (parts) differs by design: serial calls cut the part queue's tail (k_bk_scan),
    # pipelined ones do not; stats[6] (flushed cells) depends on which pairs share a part, i.e.
    # on the order of pass B's slot atomics, and varies run to run in either mode
    assert np.array_equal(ss[:5], sp[:5])
    assert np.array_equal(hs, hp) and np.array_equal(ms, mp)


def test_pipelined_oracle_128(oracle):
    """128^3 through the brick pipeline (DMF_FUSE_SLAB), 3 pipelined calls of 2 frames, vs
    the oracle."""
    poses, depth = _frames(6)
    hp, mp, sp = _run(128, poses, depth, 2, pipelined=True, variant=57)
    ov = oracle.Volume()
    ov.setDimensions(*Hh.BOUNDS)
    ov.setVolumeSize(128, 128, 128)
    ov.constructVolume()
    from dmf_amd import scene
    ho, mo, so = oracle.fuse_depth(ov, scene.intrinsics(640, 480), depth, poses,
                                   dmin=scene.DEPTH_MIN_MM, dmax=scene.DEPTH_MAX_MM)
    assert np.array_equal(np.asarray(so)[:3], sp[:3])
    assert np.array_equal(ho, hp) and np.array_equal(mo, mp)


def test_serial_then_pipelined_without_sync():
    """a serial call on the volume's stream, then dmf_fuse_set_input_stream
    and pipelined calls with NO synchronisation by the caller.  The first pipelined call's pass
    A reuses slot 0's buffers, which the serial call's pass B and phase F may still be reading
    (the serial call is held back by a ~0.5 s spin kernel queued ahead of it, so an unordered
    pass A would overwrite its records).  The mode switch orders it: it frees and re-plans the
    fusion scratch after the volume's streams drain, and staged calls wait for the serial
    slot's last reader (slots[0].free).  Counters equal an all-serial volume's."""
    poses, depth = _frames(9, seed=5)
    hs, ms, ss = _run(256, poses, depth, 3, pipelined=False)
    v = _Vol(256, 3)
    torch = v.torch
    d_depth = torch.from_numpy(depth.view(np.int16)).to(v.dev)
    d_poses = torch.from_numpy(poses).to(v.dev)
    torch.cuda.synchronize(v.dev)
    try:
        v.reserve()
        with torch.cuda.stream(v.main):
            torch.cuda._sleep(1_000_000_000)
        v.call(d_depth[0:3], d_poses[0:3])        # serial, slot 0, behind the spin
        v.pipelined(True)                         # the mode switch
        v.call(d_depth[3:6], d_poses[3:6])        # staged: slot 0 again
        v.call(d_depth[6:9], d_poses[6:9])        # staged: slot 1
        v.pipelined(False)
        hp, mp, sp = v.linear()
    finally:
        v.close()
    assert np.array_equal(ss[:5], sp[:5])
    assert np.array_equal(hs, hp) and np.array_equal(ms, mp)


def test_pipelined_then_serial_mixed():
    """Pipelined calls, then serial calls on the same volume (input stream cleared) with no
    synchronisation, then pipelined again: equal to all-serial."""
    poses, depth = _frames(12, seed=6)
    hs, ms, ss = _run(256, poses, depth, 3, pipelined=False)
    v = _Vol(256, 3)
    torch = v.torch
    d_depth = torch.from_numpy(depth.view(np.int16)).to(v.dev)
    d_poses = torch.from_numpy(poses).to(v.dev)
    torch.cuda.synchronize(v.dev)
    try:
        v.pipelined(True)
        v.reserve()
        v.call(d_depth[0:3], d_poses[0:3])
        v.pipelined(False)
        v.call(d_depth[3:6], d_poses[3:6])
        v.pipelined(True)
        v.call(d_depth[6:9], d_poses[6:9])
        v.call(d_depth[9:12], d_poses[9:12])
        hp, mp, sp = v.linear()
    finally:
        v.close()
    assert np.array_equal(ss[:5], sp[:5])
    assert np.array_equal(hs, hp) and np.array_equal(ms, mp)


def test_pipelined_with_phase_event():
    """dmf_fuse_set_phase_event on a pipelined volume (what bench.py does): the caller's event
    is recorded before every phase F and also marks the end of pass B for the next call's pass
    A.  Pipelined calls with the event set, then with it replaced by a
    second event and the first destroyed (the next pass A must not wait on it), then with none
    equal the serial counters, and the events were recorded."""
    poses, depth = _frames(12, seed=8)
    hs, ms, ss = _run(256, poses, depth, 3, pipelined=False)
    v = _Vol(256, 3)
    torch = v.torch
    d_depth = torch.from_numpy(depth.view(np.int16)).to(v.dev)
    d_poses = torch.from_numpy(poses).to(v.dev)
    torch.cuda.synchronize(v.dev)
    ev1, ev2 = torch.cuda.Event(), torch.cuda.Event()
    ev1.record(v.main)
    ev2.record(v.main)
    try:
        v.pipelined(True)
        v.reserve()
        v._lib.check(v.L.dmf_fuse_set_phase_event(v.vol._h, C.c_void_p(ev1.cuda_event)))
        v.call(d_depth[0:3], d_poses[0:3])
        v.call(d_depth[3:6], d_poses[3:6])
        v.inp.wait_event(ev1)  # what a caller does with it: its next work after phase F began
        v._lib.check(v.L.dmf_fuse_set_phase_event(v.vol._h, C.c_void_p(ev2.cuda_event)))
        ev1.synchronize()  # the second call's phase F has begun: the replaced event may go
        del ev1            # (the next pass A no longer waits on it)
        import gc
        gc.collect()
        v.call(d_depth[6:9], d_poses[6:9])
        v._lib.check(v.L.dmf_fuse_set_phase_event(v.vol._h, None))
        v.call(d_depth[9:12], d_poses[9:12])
        hp, mp, sp = v.linear()
        assert ev2.query()
    finally:
        v.close()
    assert np.array_equal(ss[:5], sp[:5])
    assert np.array_equal(hs, hp) and np.array_equal(ms, mp)


def test_timed_mode_config4_shape():
    """The bench's timed mode at its own shape: 512^3, calls of the 128 frames of config 4's
    per-GPU shard (bench.py at N = 1), pipelined through an idle input stream exactly as
    bench.py does (three calls back to back, no synchronisation), equal counter for counter to
    three serial calls, and the finalized grid of ONE pipelined call equals the committed
    oracle digest of the same 128 frames (tests/golden/fusion_digests.json, generated by the
    oracle in tests/golden/gen_fusion_digests.py)."""
    from dmf_amd import scene
    golden = json.load(open(GOLDEN))["config4_shard_N1"]
    poses = np.ascontiguousarray(scene.fibonacci_poses(128, seed=1234), np.float32)
    depth = np.ascontiguousarray(scene.render_frames(scene.intrinsics(640, 480), 640, 480, poses), np.uint16)
    results = {}
    for mode in ("serial", "pipelined"):
        v = _Vol(512, 128)
        torch = v.torch
        d_depth = torch.from_numpy(depth.view(np.int16)).to(v.dev)
        d_poses = torch.from_numpy(poses).to(v.dev)
        torch.cuda.synchronize(v.dev)
        try:
            v.pipelined(mode == "pipelined")
            v.reserve()
            v.call(d_depth, d_poses)
            if mode == "pipelined":
                assert v.logodds_digest() == golden["logodds_digest"]
                assert int(v.stats.cpu()[0]) == golden["updates"]
            for _ in range(2):
                v.call(d_depth, d_poses)
            torch.cuda.synchronize(v.dev)
            results[mode] = (v.counters.clone(), v.stats.cpu().numpy())
        finally:
            v.close()
    (cs, ss), (cp, sp) = results["serial"], results["pipelined"]
    assert np.array_equal(ss[:5], sp[:5]) and int(ss[0]) == 3 * golden["updates"]
    assert results["serial"][0].equal(cp)


@pytest.mark.parametrize("extra", [1, 1 << 20])
def test_pass_b_layout_guard(extra):
    """Pass B's record stores are guarded: with DMF_KNOB_FAULT_INJECT the
    first pair of thread 0 of each pass-B workgroup of the first pose takes `extra` slots more
    than pass A counted.  The call must neither fault
    nor store outside the pair records: the layout check reports the disagreement in
    d_stats[3] and through dmf_fuse_status (DMF_ERR_DEVICE_CHECK), the host form returns that
    status, and the volume is clean again afterwards (same counters as before, status ok).
    extra = 1 shifts one workgroup's slots into its neighbour's range; 2^20 sends that lane's
    later slots in the brick past the call's records (dropped stores)."""
    from test_gpu_configs import Fusion
    import dmf_amd
    from dmf_amd import _lib
    f = Fusion(256, 640, 480, 8)
    c0, st0, name = f.run(0)
    assert name.startswith("dmf::k_bk_fuse_s") and int(st0[3]) == 0
    assert _lib.fuse_status(f.vol) == 0
    for pipelined in (False, True):
        inp = f.torch.cuda.Stream(f.dev)
        if pipelined:
            _lib.check(f.L.dmf_fuse_set_input_stream(f.vol._h, inp.cuda_stream))
        _lib.set_knob(f.vol, "fault_inject", extra)
        c1, st1, _ = f.run(0)
        assert int(st1[3]) > 0
        with pytest.raises(_lib.DmfError) as e:
            _lib.fuse_status(f.vol)
        assert e.value.status == _lib.DMF_ERR_DEVICE_CHECK
        _lib.set_knob(f.vol, "fault_inject", 0)
        c2, st2, _ = f.run(0)
        assert int(st2[3]) == 0 and _lib.fuse_status(f.vol) == 0
        assert f.torch.equal(c2, c0)
        if pipelined:
            _lib.check(f.L.dmf_fuse_set_input_stream(f.vol._h, None))
    # the host form returns the status itself
    eng = dmf_amd.RayTracingEngine(dmf_amd.Camera(f.K))
    prm = dmf_amd.FuseParams(dmin_mm=200, dmax_mm=1000)
    _lib.set_knob(f.vol, "fault_inject", extra)
    with pytest.raises(_lib.DmfError) as e:
        eng.fuse_depth(f.vol, f.depth, f.poses, prm)
    assert e.value.status == _lib.DMF_ERR_DEVICE_CHECK
    _lib.set_knob(f.vol, "fault_inject", 0)
    eng.fuse_depth(f.vol, f.depth, f.poses, prm)
    assert _lib.fuse_status(f.vol) == 0
