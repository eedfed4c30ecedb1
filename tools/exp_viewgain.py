#!/usr/bin/env python3
"""Timing of the view gain (dmf_view_gain_device) on bench.py's fused scene:
a 512^3 grid fused from 128 rendered 640x480 frames (setup as tools/exp_raycast.py), finalized on the
device, then the view gain of the same 128 poses with thresholds (1, -1) and range 1000 mm -- 39.3 M
rays per call, caller-allocated masks of 16 MiB per pose (2 GiB).  A/B of the walks
(DMF_KNOB_VIEWGAIN_WALK 1 = plain, 2 = jumps and one atomic per mask word, 3 = 2 with a read before
the atomic), alternated in one process; the masks, gains and statistics of every walk are compared
on the whole workload.  The yardstick is dmf_raycast_logodds_device on the same workload in the
same process.  Prints one JSON line: per walk the ms per call of each repeat (device events around
CALLS back-to-back calls, after a warm-up call), min / median / max; the same for the ray-cast, for
the gain-only call (d_seen NULL: masks in scratch, 16 poses per batch) and for the mask passes'
proxy (a call with P = 1 of an 8x6 camera and range 1 mm: the mask and brick passes, one pose's
memset and count);
the three statistics, the duplication ratio visits / sum of gains, and the gain distribution.
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
OCC, FREE, RANGE_MM = 1, -1, 1000
REPEATS = max(5, int(sys.argv[1])) if len(sys.argv) > 1 else 5
CALLS = max(1, int(sys.argv[2])) if len(sys.argv) > 2 else 3
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
grid = logodds[:N ** 3]
classes = {"solid": int((grid >= OCC).sum()), "unknown": int(((grid < OCC) & (grid > FREE)).sum()), "cells": N ** 3}
words = vol.view_gain_words()
seen = torch.empty(P * words, dtype=torch.int64, device=dev)
gain = torch.empty(P, dtype=torch.int64, device=dev)
stats = torch.zeros(3, dtype=torch.int64, device=dev)
out_d = torch.empty(P * H * W, dtype=torch.int32, device=dev)
out_c = torch.empty(P * H * W, dtype=torch.int64, device=dev)


def view_gain(st=None, masks=True):
    _lib.check(L.dmf_view_gain_device(vol._h, pcam, logodds.data_ptr(), d_poses.data_ptr(), P, OCC, FREE, RANGE_MM,
                                      seen.data_ptr() if masks else None, gain.data_ptr(), st))


def raycast():
    _lib.check(L.dmf_raycast_logodds_device(vol._h, pcam, logodds.data_ptr(), d_poses.data_ptr(), P, OCC, RANGE_MM,
                                            out_d.data_ptr(), out_c.data_ptr(), None))


# the mask passes alone, nearly: the same grid and thresholds with one pose of an 8x6 camera and rays of 1 mm (one
# workgroup of rays of one or two cells; at range 1000 that one wave's walk through unknown space took 2.2 ms)
K8 = K.copy()
K8[[0, 2, 4, 5]] /= np.float32(80)
cam8 = _lib.make_camera(K8, 6, 8)


def mask_proxy():
    _lib.check(L.dmf_view_gain_device(vol._h, C.addressof(cam8), logodds.data_ptr(), d_poses.data_ptr(), 1, OCC, FREE,
                                      1, seen.data_ptr(), gain.data_ptr(), None))


def timed(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    for _ in range(calls):
        fn()
    e1.record(s)
    torch.cuda.synchronize(dev)
    return e0.elapsed_time(e1) / calls


WALKS = {1: "plain", 2: "word", 3: "word_read"}  # DMF_KNOB_VIEWGAIN_WALK
rays = P * H * W
st_of, gain_of, equal = {}, {}, {}
first = None
for kw in WALKS:  # warm-up (code objects, scratch growth); the masks, gains and statistics of one call each
    _lib.set_knob(vol, "viewgain_walk", kw)
    seen.fill_(-1)
    stats.zero_()
    view_gain(stats.data_ptr())
    torch.cuda.synchronize(dev)
    st_of[kw] = [int(x) for x in stats.cpu().numpy()]
    gain_of[kw] = gain.cpu().numpy().astype(np.uint64)
    if first is None:
        first = seen.clone()
    equal[kw] = bool(torch.equal(seen, first))
popcount = int(np.unpackbits(first[first != 0].cpu().numpy().view(np.uint8)).sum(dtype=np.int64))
del first
_lib.set_knob(vol, "viewgain_walk", 0)
_lib.set_knob(vol, "viewgain_batch", 16)
view_gain(masks=False)
torch.cuda.synchronize(dev)
gain_batched = gain.cpu().numpy().astype(np.uint64)
raycast()
mask_proxy()
torch.cuda.synchronize(dev)
ms = {name: [] for name in list(WALKS.values()) + ["gain_only", "raycast", "mask_proxy"]}
for _ in range(REPEATS):  # the measurements alternate
    for kw, name in WALKS.items():
        _lib.set_knob(vol, "viewgain_walk", kw)
        ms[name].append(timed(view_gain, CALLS))
    _lib.set_knob(vol, "viewgain_walk", 0)
    ms["gain_only"].append(timed(lambda: view_gain(masks=False), CALLS))
    ms["raycast"].append(timed(raycast, CALLS))
    ms["mask_proxy"].append(timed(mask_proxy, CALLS))
_lib.set_knob(vol, "viewgain_batch", 0)
g = gain_of[1]
out = {"grid": N, "poses": P, "rays": rays, "thresholds": [OCC, FREE], "range_mm": RANGE_MM, "calls_per_repeat": CALLS,
       "mask_bytes_per_pose": 8 * words, "classes": classes}
for name, v in ms.items():
    out[f"ms_per_call_{name}"] = [round(x, 4) for x in v]
    out[f"ms_{name}"] = {"min": round(min(v), 4), "median": round(float(np.median(v)), 4), "max": round(max(v), 4)}
rc = float(np.median(ms["raycast"]))
out.update({
    "multiple_of_raycast": {name: round(float(np.median(ms[name])) / rc, 2) for name in WALKS.values()},
    "masks_equal": equal, "stats_equal": all(st_of[kw] == st_of[1] for kw in WALKS),
    "gains_equal": bool(all(np.array_equal(gain_of[kw], g) for kw in WALKS) and np.array_equal(gain_batched, g)),
    "gain_equals_popcount": bool(int(g.sum()) == popcount),
    "stats": {"entered": st_of[1][0], "stopped": st_of[1][1], "visits": st_of[1][2]},
    "entered_fraction": round(st_of[1][0] / rays, 4), "stopped_fraction": round(st_of[1][1] / rays, 4),
    "visits_per_ray": round(st_of[1][2] / rays, 2),
    "duplication_ratio": round(st_of[1][2] / max(int(g.sum()), 1), 2),
    "gain": {"min": int(g.min()), "median": int(np.median(g)), "max": int(g.max()), "sum": int(g.sum())}})
print(json.dumps(out), flush=True)
