#!/usr/bin/env python3
"""Timing of the surface extraction (dmf_grid_surface_device) on bench.py's
fused scene: a 512^3 grid fused from 128 rendered 640x480 frames (fibonacci_poses seed 1234, the
default fusion parameters with the scene's depth gate), finalized on the device, then extracted with
thresholds (1, -1) into device buffers sized by a first call.  (Setup as tools/exp_raycast.py.)
Alternating with it in the same process: a ray-cast call with P = 1 of an 8x6 camera, the existing
proxy for the mask passes, which stream the same grid.  Prints one JSON line: ms per call of each
repeat (device events around CALLS back-to-back calls, after a warm-up call), min / median / max
of both, the surface and solid counts, and the achieved bytes/s by algorithmic bytes (2 B per cell
+ 32 B per surface cell) as a fraction of 8.0 TB/s.
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
PEAK_BYTES_PER_S = 8.0e12
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

# the size: one call with a one-entry hash output (cap = 1), the count read back
count = torch.zeros(2, dtype=torch.int64, device=dev)
one = torch.zeros(1, dtype=torch.int64, device=dev)
_lib.check(L.dmf_grid_surface_device(vol._h, logodds.data_ptr(), OCC, FREE, one.data_ptr(), None, None, 1,
                                     count.data_ptr()))
torch.cuda.synchronize(dev)
n_surface, n_solid = (int(x) for x in count.cpu().numpy())
cap = max(n_surface, 1)
out_h = torch.empty(cap, dtype=torch.int64, device=dev)
out_x = torch.empty(3 * cap, dtype=torch.float32, device=dev)
out_n = torch.empty(3 * cap, dtype=torch.float32, device=dev)


def extract():
    _lib.check(L.dmf_grid_surface_device(vol._h, logodds.data_ptr(), OCC, FREE, out_h.data_ptr(), out_x.data_ptr(),
                                         out_n.data_ptr(), cap, count.data_ptr()))


# the mask passes alone, nearly: the same grid with one pose of an 8x6 camera (one workgroup of rays)
K8 = K.copy()
K8[[0, 2, 4, 5]] /= np.float32(80)
cam8 = _lib.make_camera(K8, 6, 8)
out8_d = torch.empty(48, dtype=torch.int32, device=dev)
out8_c = torch.empty(48, dtype=torch.int64, device=dev)


def mask_proxy():
    _lib.check(L.dmf_raycast_logodds_device(vol._h, C.addressof(cam8), logodds.data_ptr(), d_poses.data_ptr(), 1, OCC,
                                            RANGE_MM, out8_d.data_ptr(), out8_c.data_ptr(), None))


def timed(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    for _ in range(calls):
        fn()
    e1.record(s)
    torch.cuda.synchronize(dev)
    return e0.elapsed_time(e1) / calls


extract()  # warm-up (code objects, scratch growth)
mask_proxy()
torch.cuda.synchronize(dev)
counts_again = [int(x) for x in count.cpu().numpy()]
h = out_h.cpu().numpy().view(np.uint64)[:n_surface]
ordered = bool((np.diff(h.astype(np.int64)) > 0).all())
nrm = out_n.cpu().numpy().reshape(-1, 3)[:n_surface]
zero_normals = int((~(nrm != 0).any(axis=1)).sum())
ms, ms_mask = [], []
for _ in range(REPEATS):  # the measurements alternate
    ms.append(timed(extract, CALLS))
    ms_mask.append(timed(mask_proxy, CALLS))
med, med_mask = float(np.median(ms)), float(np.median(ms_mask))
alg_bytes = 2 * N ** 3 + 32 * n_surface
out = {"grid": N, "poses_fused": P, "thresholds": [OCC, FREE], "calls_per_repeat": CALLS,
       "surface_cells": n_surface, "solid_cells": n_solid, "counts_stable": counts_again == [n_surface, n_solid],
       "hashes_ascending": ordered, "zero_normals": zero_normals,
       "ms_per_call": [round(x, 4) for x in ms],
       "ms": {"min": round(min(ms), 4), "median": round(med, 4), "max": round(max(ms), 4)},
       "ms_mask_proxy_per_call": [round(x, 4) for x in ms_mask],
       "ms_mask_proxy": {"min": round(min(ms_mask), 4), "median": round(med_mask, 4), "max": round(max(ms_mask), 4)},
       "ratio_to_mask_proxy": round(med / med_mask, 3),
       "algorithmic_bytes": alg_bytes, "bytes_per_s": round(alg_bytes / (med * 1e-3), 1),
       "fraction_of_8TBps": round(alg_bytes / (med * 1e-3) / PEAK_BYTES_PER_S, 4)}
print(json.dumps(out), flush=True)
