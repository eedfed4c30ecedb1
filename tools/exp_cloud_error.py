#!/usr/bin/env python3
"""Timing of the cloud error (dmf_cloud_nearest_device) on bench.py's fused
scene: a 512^3 grid fused from 128 rendered 640x480 frames (fibonacci_poses seed 1234, the default
fusion parameters with the scene's depth gate), finalized on the device (setup as
tools/exp_travel.py).  The queries are the grid's extracted surface (dmf_grid_surface_device at
thresholds 1 / -1, about 419 k voxel centres, on the device); the reference cloud is the
back-projected points of the first 8 frames (about 2.4 M).  Every variant of the call -- the target
occupancy of a cell 4, 8, 16 times the queries in the order given or sorted by home cell
(dmf_cloud_nearest_set_variant) -- is timed in the same run, alternating, with the library's
default, with the index build alone (the same call with one query) and with a device-to-device copy
of 1 GiB (the box's stream rate; the byte floor, both clouds read once and dist2, index written once,
is taken at it).  Every variant's outputs are compared with the default's: they must be the same bytes.
Prints one JSON line and writes it to argv[3] (default profiles/cloud_error/result.json): ms per call
of each repeat (device events on the volume's stream around CALLS back-to-back calls, after a warm-up
call), min / median / max, the default call over the byte floor, the summaries, and -- from a library
built with -DDMF_EXP_STATS (tools/build_exp.sh stats -DDMF_EXP_STATS, run with DMF_LIB=...; 0
otherwise, and the timings of such a library are not the product's) -- the reference points examined
and the shells scanned per query.
argv: [repeats >= 5] [calls per repeat] [output path]."""
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

W, H, P, N, REF_FRAMES = 640, 480, 128, 512, 8
THR = np.array([0.003, 0.005])
REPEATS = max(5, int(sys.argv[1])) if len(sys.argv) > 1 else 7
CALLS = max(1, int(sys.argv[2])) if len(sys.argv) > 2 else 3
OUT = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "cloud_error", "result.json")
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

# the queries: the surface's voxel centres, extracted on the device (the count first, capacity 0)
count = torch.zeros(2, dtype=torch.int64, device=dev)
tiny = torch.zeros(4, dtype=torch.float32, device=dev)
_lib.check(L.dmf_grid_surface_device(vol._h, logodds.data_ptr(), 1, -1, None, tiny.data_ptr(), None, 0, count.data_ptr()))
n = int(count.cpu().numpy()[0])
xyz = torch.empty(3 * n, dtype=torch.float32, device=dev)
_lib.check(L.dmf_grid_surface_device(vol._h, logodds.data_ptr(), 1, -1, None, xyz.data_ptr(), None, n, count.data_ptr()))
# the reference: the back-projected points of the first frames with a depth
eng = dmf_amd.RayTracingEngine(dmf_amd.Camera(K, H, W))
ref = np.concatenate([eng.backproject(vol, depth[i], poses[i]).reshape(-1, 3)[depth[i].reshape(-1) > 0]
                      for i in range(REF_FRAMES)]).astype(np.float32)
m = ref.shape[0]
d_ref = torch.from_numpy(ref).to(dev)
del logodds

d2 = torch.empty(n, dtype=torch.float32, device=dev)
idx = torch.empty(n, dtype=torch.int32, device=dev)
cnt = torch.zeros(2 + THR.size, dtype=torch.int64, device=dev)
sums = torch.zeros(2, dtype=torch.float64, device=dev)


def call(occ, order, nq=None):
    def f():
        _lib.cloud_variant(vol, occ, order)
        _lib.check(L.dmf_cloud_nearest_device(vol._h, xyz.data_ptr(), n if nq is None else nq, d_ref.data_ptr(), m,
                                              d2.data_ptr(), idx.data_ptr(), THR.ctypes.data, THR.size, cnt.data_ptr(),
                                              sums.data_ptr()))
    return f


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


fns = {"default": call(0, 0), "copy_1GiB": copy, "build_default_one_query": call(0, 0, 1)}
for occ in (4, 8, 16):
    for order, tag in ((1, "given"), (2, "sorted")):
        fns[f"occ{occ}_{tag}"] = call(occ, order)
    fns[f"build_occ{occ}_one_query"] = call(occ, 1, 1)
variants, first = {}, None
for k, fn in fns.items():  # warm-up (code objects, scratch growth), each variant's counters and its bytes
    fn()
    torch.cuda.synchronize(dev)
    if k == "copy_1GiB" or k.startswith("build"):
        continue
    st = np.zeros(4, np.uint64)
    _lib.check(L.dmf_cloud_nearest_stats(vol._h, st.ctypes.data))
    got = (d2.cpu().numpy().tobytes(), idx.cpu().numpy().tobytes(), cnt.cpu().numpy().tolist(), float(sums.cpu().numpy()[0]))
    if first is None:  # the default's own figures
        first = got
        summary = {"counts": got[2], "max_error": got[3],
                   "avg_error": float(sums.cpu().numpy()[1]) / max(int(got[2][0]), 1)}
    variants[k] = {"same_bytes_as_default": got == first, "index_cells": int(st[2]), "valid_reference_points": int(st[3]),
                   "candidates_per_query": round(int(st[0]) / max(n, 1), 2), "shells_per_query": round(int(st[1]) / max(n, 1), 3)}
ms = {k: [] for k in fns}
for _ in range(REPEATS):  # the measurements alternate
    for k, fn in fns.items():
        ms[k].append(timed(fn, CALLS))
med = {k: float(np.median(v)) for k, v in ms.items()}
rate = 2 * COPY_BYTES / (med["copy_1GiB"] * 1e-3)            # bytes read + written per second
floor = (12 * (n + m) + 8 * n) / rate * 1e3
out = {"grid": N, "poses_fused": P, "queries": n, "reference_points": m, "reference_frames": REF_FRAMES,
       "thresholds": THR.tolist(), "calls_per_repeat": CALLS, "summary": summary, "variants": variants,
       "all_variants_same_bytes": all(v["same_bytes_as_default"] for v in variants.values()),
       "ms_per_call": {k: [round(x, 4) for x in v] for k, v in ms.items()},
       "ms": {k: {"min": round(min(v), 4), "median": round(med[k], 4), "max": round(max(v), 4)} for k, v in ms.items()},
       "stream_bytes_per_s": round(rate, 1), "byte_floor_ms": round(floor, 4),
       "default_over_floor": round(med["default"] / floor, 1), "library": os.path.basename(os.path.dirname(os.environ["DMF_LIB"])) if os.environ.get("DMF_LIB") else "product"}
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as f:
    f.write(json.dumps(out, indent=1) + "\n")
print(json.dumps(out), flush=True)
