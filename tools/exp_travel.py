#!/usr/bin/env python3
"""Timing of the travel field (dmf_grid_travel_device) on bench.py's fused
scene: a 512^3 grid fused from 128 rendered 640x480 frames (fibonacci_poses seed 1234, the default
fusion parameters with the scene's depth gate), finalized on the device (setup as
tools/exp_distance.py); the distance field at threshold 1, then a travel field from the cell of the
first camera's position (clamped into the grid) at radius2 = 1 and at radius2 = 16 (a body of 4
cells).  Two yardsticks measured in the same run, alternating with the calls: a device-to-device
copy of 1 GiB (the box's stream rate; the byte floor, one read of dist2 plus one write of hops = 8 B
per cell, is taken at it) and dmf_grid_distance_device on the same grid.  Prints one JSON line: ms
per call of each repeat (device events on the volume's stream around CALLS back-to-back calls, after
a warm-up call; the travel call waits for its own rounds, so this is what a caller sees), min /
median / max, both ratios, and per travel field the counters, the rounds that had work, the
launches, and -- from a library built with -DDMF_EXP_STATS (tools/build_exp.sh stats
-DDMF_EXP_STATS, run with DMF_LIB=...; 0 otherwise, and the timings of such a library are not the
product's) -- the tile activations and the cell updates per reached cell.
argv: [repeats >= 5] [calls per repeat]."""
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "depth-map-fusion-utils_amd")]
import dmf_amd  # noqa: E402
from dmf_amd import _lib, scene  # noqa: E402

W, H, P, N = 640, 480, 128, 512
THRESHOLD, RADII2 = 1, (1, 16)
REPEATS = max(5, int(sys.argv[1])) if len(sys.argv) > 1 else 7
CALLS = max(1, int(sys.argv[2])) if len(sys.argv) > 2 else 2
dev = torch.device("cuda", 0)
K = scene.intrinsics(W, H)
poses = np.ascontiguousarray(scene.fibonacci_poses(P, seed=1234), np.float32)
depth = np.ascontiguousarray(scene.render_frames(K, W, H, poses), np.uint16)
L = _lib.load()
vol = dmf_amd.VoxelVolume(0)
s = torch.cuda.current_stream(dev)
vol.set_stream(s.cuda_stream)
vol.setDimensions(-0.5, 0.5, -0.5, 0.5, -0.5, 0.5)
vol.setVolumeSize(N, N, N)
vol.constructVolume()
cam = _lib.make_camera(K, H, W)
prm = _lib.default_fuse_params(dmin_mm=scene.DEPTH_MIN_MM, dmax_mm=scene.DEPTH_MAX_MM)
d_depth = torch.from_numpy(depth.view(np.int16)).to(dev)
d_poses = torch.from_numpy(poses).to(dev)
nt = C.c_int64()
_lib.check(L.dmf_fuse_counter_cells(vol._h, C.addressof(nt)))
hits = torch.zeros(nt.value, dtype=torch.int32, device=dev)
misses = torch.zeros(nt.value, dtype=torch.int32, device=dev)
logodds = torch.empty(N ** 3 + 32, dtype=torch.int16, device=dev)
_lib.check(L.dmf_fuse_depth_device(vol._h, C.addressof(cam), d_depth.data_ptr(), d_poses.data_ptr(), P,
                                   C.addressof(prm), hits.data_ptr(), misses.data_ptr(), None))
_lib.check(L.dmf_fuse_finalize_device(vol._h, hits.data_ptr(), misses.data_ptr(), C.addressof(prm), logodds.data_ptr()))
torch.cuda.synchronize(dev)
_lib.fuse_status(vol)
del hits, misses, d_depth

dist2 = torch.empty(N ** 3, dtype=torch.int32, device=dev)
hops = torch.empty(N ** 3, dtype=torch.int32, device=dev)
count = torch.zeros(1, dtype=torch.int64, device=dev)
info = torch.zeros(3, dtype=torch.int64, device=dev)
seed = np.clip(np.floor((poses[0].reshape(3, 4)[:, 3].astype(np.float64) + 0.5) * N), 0, N - 1).astype(np.int32)
d_seed = torch.from_numpy(seed.reshape(1, 3)).to(dev)


def distance():
    _lib.check(L.dmf_grid_distance_device(vol._h, logodds.data_ptr(), THRESHOLD, dist2.data_ptr(), count.data_ptr()))


def travel(radius2):
    def call():
        _lib.check(L.dmf_grid_travel_device(vol._h, dist2.data_ptr(), radius2, d_seed.data_ptr(), 1, hops.data_ptr(),
                                            info.data_ptr()))
    return call


COPY_BYTES = 1 << 30
src = torch.empty(COPY_BYTES, dtype=torch.uint8, device=dev)
dst = torch.empty(COPY_BYTES, dtype=torch.uint8, device=dev)


def copy():
    dst.copy_(src)


def timed(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    for _ in range(calls):
        fn()
    e1.record(s)
    torch.cuda.synchronize(dev)
    return e0.elapsed_time(e1) / calls


fns = {"distance": distance, "copy_1GiB": copy}
for r2 in RADII2:
    fns[f"travel_r2_{r2}"] = travel(r2)
fields = {}
for k, fn in fns.items():  # warm-up (code objects, scratch growth), and each travel field's own figures
    fn()
    torch.cuda.synchronize(dev)
    if k.startswith("travel"):
        st = np.zeros(4, np.uint64)
        _lib.check(L.dmf_grid_travel_stats(vol._h, st.ctypes.data))
        trav, reached, mx = (int(x) for x in info.cpu().numpy())
        fields[k] = {"traversable": trav, "reached": reached, "max_hops": mx, "rounds_with_work": int(st[0]),
                     "kernel_launches": int(st[1]), "tile_activations": int(st[2]),
                     "activations_per_512_reached_cells": round(int(st[2]) / max(reached / 512, 1), 2),
                     "cell_updates_per_reached_cell": round(int(st[3]) / max(reached, 1), 3)}
ms = {k: [] for k in fns}
for _ in range(REPEATS):  # the measurements alternate
    for k, fn in fns.items():
        ms[k].append(timed(fn, CALLS))
med = {k: float(np.median(v)) for k, v in ms.items()}
rate = 2 * COPY_BYTES / (med["copy_1GiB"] * 1e-3)            # bytes read + written per second
floor = 8 * N ** 3 / rate * 1e3
out = {"grid": N, "poses_fused": P, "threshold": THRESHOLD, "calls_per_repeat": CALLS, "seed": seed.tolist(),
       "solid_cells": int(count.cpu().numpy()[0]), "fields": fields,
       "ms_per_call": {k: [round(x, 4) for x in v] for k, v in ms.items()},
       "ms": {k: {"min": round(min(v), 4), "median": round(med[k], 4), "max": round(max(v), 4)} for k, v in ms.items()},
       "stream_bytes_per_s": round(rate, 1), "travel_floor_ms_8B_per_cell": round(floor, 4),
       "travel_over_floor": {k: round(med[k] / floor, 2) for k in med if k.startswith("travel")},
       "travel_over_distance": {k: round(med[k] / med["distance"], 2) for k in med if k.startswith("travel")}}
print(json.dumps(out), flush=True)
