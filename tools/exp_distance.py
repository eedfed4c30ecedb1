#!/usr/bin/env python3
"""Timing of the distance field and of the segment clearance (dmf_grid_distance_device,
dmf_grid_clearance_device) on bench.py's fused scene: a 512^3 grid fused from
128 rendered 640x480 frames (fibonacci_poses seed 1234, the default fusion parameters with the
scene's depth gate), finalized on the device (setup as tools/exp_surface.py); the field at threshold
1, then the clearance of the 1024^2 ordered pairs of the cost-map workload's 1024 sphere centres.
Two yardsticks measured in the same run, alternating with the calls: a device-to-device copy of
1 GiB (the box's stream rate; the byte floors below are taken at it) and dmf_grid_surface_device on
the same grid (a streaming pass over the same int16 bytes).  Prints one JSON line: ms per call of
each repeat (device events on the volume's stream around CALLS back-to-back calls, after a warm-up
call), min / median / max, both ratios, and the byte floors: the call's own bytes (2 B read + 4 B
written per cell) and the chosen passes' (z: 2 + 4, y and x: 4 + 4 each = 22 B per cell; the
envelope stacks' traffic depends on the scene and is not counted).
argv: [repeats >= 5] [calls per repeat].

Per pass: run the same command under `rocprofv3 --kernel-trace --output-format csv -d DIR -o run`
(a run of its own: tracing slows the host), then `exp_distance.py --passes DIR` prints the median
duration of k_df_z, of k_df_axis along y and along x (its dispatches alternate, y first), of
k_df_clear and of the surface kernels from the trace."""
import csv
import ctypes as C
import glob
import json
import os
import sys

import numpy as np


def passes(d):
    files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        sys.exit("no kernel_trace.csv under " + d)
    rows = sorted(csv.DictReader(open(files[0])), key=lambda r: int(r["Start_Timestamp"]))
    ms, axis = {}, 0
    for r in rows:
        name = r["Kernel_Name"]
        key = next((k for k in ("k_df_z", "k_df_axis", "k_df_clear", "k_sf_mask", "k_sf_surface", "k_sf_emit")
                    if k in name), None)
        if key is None:
            continue
        if key == "k_df_axis":
            key += "_y" if axis % 2 == 0 else "_x"
            axis += 1
        ms.setdefault(key, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6)
    print(json.dumps({k: {"dispatches": len(v), "median_ms": round(float(np.median(v)), 4),
                          "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)} for k, v in ms.items()}))


if len(sys.argv) > 2 and sys.argv[1] == "--passes":
    passes(sys.argv[2])
    sys.exit(0)

import torch  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "depth-map-fusion-utils_amd")]
import dmf_amd  # noqa: E402
from dmf_amd import _lib, scene  # noqa: E402

W, H, P, N, VC = 640, 480, 128, 512, 1024
THRESHOLD, OCC, FREE = 1, 1, -1
REPEATS = max(5, int(sys.argv[1])) if len(sys.argv) > 1 else 7
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
count = torch.zeros(1, dtype=torch.int64, device=dev)


def distance():
    _lib.check(L.dmf_grid_distance_device(vol._h, logodds.data_ptr(), THRESHOLD, dist2.data_ptr(), count.data_ptr()))


cp = np.ascontiguousarray(scene.sphere_centres(VC)[:, 3::4], np.float32)   # the poses' translation columns
assert cp.shape == (VC, 3)
ii, jj = np.meshgrid(np.arange(VC), np.arange(VC), indexing="ij")
d_a = torch.from_numpy(np.ascontiguousarray(cp[ii.reshape(-1)])).to(dev)
d_b = torch.from_numpy(np.ascontiguousarray(cp[jj.reshape(-1)])).to(dev)
clear2 = torch.empty(VC * VC, dtype=torch.int32, device=dev)


def clearance():
    _lib.check(L.dmf_grid_clearance_device(vol._h, dist2.data_ptr(), d_a.data_ptr(), d_b.data_ptr(), VC * VC,
                                           clear2.data_ptr()))


# the surface yardstick, sized by a first call
scount = torch.zeros(2, dtype=torch.int64, device=dev)
one = torch.zeros(1, dtype=torch.int64, device=dev)
_lib.check(L.dmf_grid_surface_device(vol._h, logodds.data_ptr(), OCC, FREE, one.data_ptr(), None, None, 1,
                                     scount.data_ptr()))
torch.cuda.synchronize(dev)
cap = max(int(scount.cpu().numpy()[0]), 1)
out_h = torch.empty(cap, dtype=torch.int64, device=dev)
out_x = torch.empty(3 * cap, dtype=torch.float32, device=dev)
out_n = torch.empty(3 * cap, dtype=torch.float32, device=dev)


def surface():
    _lib.check(L.dmf_grid_surface_device(vol._h, logodds.data_ptr(), OCC, FREE, out_h.data_ptr(), out_x.data_ptr(),
                                         out_n.data_ptr(), cap, scount.data_ptr()))


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


fns = {"distance": distance, "clearance": clearance, "surface": surface, "copy_1GiB": copy}
for fn in fns.values():  # warm-up (code objects, scratch growth)
    fn()
torch.cuda.synchronize(dev)
n_solid = int(count.cpu().numpy()[0])
d2 = dist2.cpu().numpy().view(np.uint32)
c2 = clear2.cpu().numpy().view(np.uint32)
ms = {k: [] for k in fns}
for _ in range(REPEATS):  # the measurements alternate
    for k, fn in fns.items():
        ms[k].append(timed(fn, CALLS))
med = {k: float(np.median(v)) for k, v in ms.items()}
rate = 2 * COPY_BYTES / (med["copy_1GiB"] * 1e-3)            # bytes read + written per second
floor_call = 6 * N ** 3 / rate * 1e3
floor_passes = 22 * N ** 3 / rate * 1e3
floor_clear = (24 + 4) * VC * VC / rate * 1e3
out = {"grid": N, "poses_fused": P, "threshold": THRESHOLD, "calls_per_repeat": CALLS, "solid_cells": n_solid,
       "zero_cells_equal_solid": int((d2 == 0).sum()) == n_solid, "dist2_max": int(d2.max()),
       "segments": VC * VC, "segments_without_cell": int((c2 == 0xFFFFFFFF).sum()),
       "segments_through_solid": int((c2 == 0).sum()),
       "ms_per_call": {k: [round(x, 4) for x in v] for k, v in ms.items()},
       "ms": {k: {"min": round(min(v), 4), "median": round(med[k], 4), "max": round(max(v), 4)} for k, v in ms.items()},
       "stream_bytes_per_s": round(rate, 1),
       "distance_floor_ms": {"call_6B_per_cell": round(floor_call, 4), "passes_22B_per_cell": round(floor_passes, 4)},
       "distance_over_floor": {"call": round(med["distance"] / floor_call, 2),
                               "passes": round(med["distance"] / floor_passes, 2)},
       "distance_over_surface": round(med["distance"] / med["surface"], 2),
       "clearance_floor_ms_28B_per_segment": round(floor_clear, 5),
       "clearance_over_floor": round(med["clearance"] / floor_clear, 1),
       "clearance_over_surface": round(med["clearance"] / med["surface"], 3)}
print(json.dumps(out), flush=True)
