#!/usr/bin/env python3
"""Timing of the log-odds ray-cast (dmf_raycast_logodds_device) on bench.py's
fused scene: a 512^3 grid fused from 128 rendered 640x480 frames (fibonacci_poses seed 1234, the
default fusion parameters with the scene's depth gate), finalized on the device, then cast from the
same 128 poses with threshold 1 and range 1000 mm -- 39.3 M rays per call.  (Setup as
tools/exp_forward.py.)  A/B of the two walks (DMF_KNOB_RAYCAST_WALK 1 = cell by cell, 2 = empty
bricks and tiles jumped), alternated; their outputs and statistics are compared.  Prints one JSON
line: per walk the ms per call of each repeat (device events around CALLS back-to-back calls, after
a warm-up call), min / median / max and Mrays/s at the median; the mask passes' share from a proxy
(a call with P = 1 of an 8x6 camera); the fractions of rays that enter the grid and that find a
surface cell.
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
THRESHOLD, RANGE_MM = 1, 1000
REPEATS = max(5, int(sys.argv[1])) if len(sys.argv) > 1 else 7
CALLS = max(1, int(sys.argv[2])) if len(sys.argv) > 2 else 5
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
pcam = C.addressof(cam)
prm = _lib.default_fuse_params(dmin_mm=scene.DEPTH_MIN_MM, dmax_mm=scene.DEPTH_MAX_MM)
d_depth = torch.from_numpy(depth.view(np.int16)).to(dev)
d_poses = torch.from_numpy(poses).to(dev)
nt = C.c_int64()
_lib.check(L.dmf_fuse_counter_cells(vol._h, C.addressof(nt)))
hits = torch.zeros(nt.value, dtype=torch.int32, device=dev)
misses = torch.zeros(nt.value, dtype=torch.int32, device=dev)
logodds = torch.empty(N ** 3 + 32, dtype=torch.int16, device=dev)
_lib.check(L.dmf_fuse_depth_device(vol._h, pcam, d_depth.data_ptr(), d_poses.data_ptr(), P, C.addressof(prm),
                                   hits.data_ptr(), misses.data_ptr(), None))
_lib.check(L.dmf_fuse_finalize_device(vol._h, hits.data_ptr(), misses.data_ptr(), C.addressof(prm), logodds.data_ptr()))
torch.cuda.synchronize(dev)
_lib.fuse_status(vol)
del hits, misses, d_depth
out_d = torch.empty(P * H * W, dtype=torch.int32, device=dev)
out_c = torch.empty(P * H * W, dtype=torch.int64, device=dev)
stats = torch.zeros(2, dtype=torch.int64, device=dev)


def cast(st=None):
    _lib.check(L.dmf_raycast_logodds_device(vol._h, pcam, logodds.data_ptr(), d_poses.data_ptr(), P, THRESHOLD, RANGE_MM,
                                            out_d.data_ptr(), out_c.data_ptr(), st))


# the mask passes alone, nearly: the same grid and threshold with one pose of an 8x6 camera (one workgroup of rays)
K8 = K.copy()
K8[[0, 2, 4, 5]] /= np.float32(80)
cam8 = _lib.make_camera(K8, 6, 8)
out8_d = torch.empty(48, dtype=torch.int32, device=dev)
out8_c = torch.empty(48, dtype=torch.int64, device=dev)


def mask_proxy():
    _lib.check(L.dmf_raycast_logodds_device(vol._h, C.addressof(cam8), logodds.data_ptr(), d_poses.data_ptr(), 1, THRESHOLD,
                                            RANGE_MM, out8_d.data_ptr(), out8_c.data_ptr(), None))


def timed(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    for _ in range(calls):
        fn()
    e1.record(s)
    torch.cuda.synchronize(dev)
    return e0.elapsed_time(e1) / calls


WALKS = {1: "cell", 2: "jump"}  # DMF_KNOB_RAYCAST_WALK
rays = P * H * W
res, st_of = {}, {}
for kw in WALKS:  # warm-up (code objects, scratch growth), the statistics and the outputs of one call each
    _lib.set_knob(vol, "raycast_walk", kw)
    stats.zero_()
    cast(stats.data_ptr())
    torch.cuda.synchronize(dev)
    st_of[kw] = [int(x) for x in stats.cpu().numpy()]
    res[kw] = (out_d.cpu().numpy().copy(), out_c.cpu().numpy().view(np.uint64).copy())
mask_proxy()
torch.cuda.synchronize(dev)
ms = {kw: [] for kw in WALKS}
ms_mask = []
for _ in range(REPEATS):  # the measurements alternate
    for kw in WALKS:
        _lib.set_knob(vol, "raycast_walk", kw)
        ms[kw].append(timed(cast, CALLS))
    ms_mask.append(timed(mask_proxy, CALLS))
_lib.set_knob(vol, "raycast_walk", 0)
depths, cells = res[1]
found = cells != np.uint64(0xFFFFFFFFFFFFFFFF)
out = {"grid": N, "poses": P, "rays": rays, "threshold": THRESHOLD, "range_mm": RANGE_MM, "calls_per_repeat": CALLS}
for kw, name in WALKS.items():
    med = float(np.median(ms[kw]))
    out[f"ms_per_call_{name}"] = [round(x, 4) for x in ms[kw]]
    out[f"ms_{name}"] = {"min": round(min(ms[kw]), 4), "median": round(med, 4), "max": round(max(ms[kw]), 4)}
    out[f"mrays_per_s_{name}"] = round(rays / med / 1e3, 1)
out.update({"ms_mask_proxy": [round(x, 4) for x in ms_mask],
            "outputs_equal": bool(np.array_equal(res[1][0], res[2][0]) and np.array_equal(res[1][1], res[2][1])
                                  and st_of[1] == st_of[2]),
            "entered_fraction": round(st_of[1][0] / rays, 4), "surface_fraction": round(st_of[1][1] / rays, 4),
            "surface_matches_cells": bool(int(found.sum()) == st_of[1][1]),
            "median_depth_mm": int(np.median(depths[found])) if found.any() else None})
print(json.dumps(out), flush=True)
