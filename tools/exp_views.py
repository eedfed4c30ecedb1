#!/usr/bin/env python3
"""Timing of the candidate views (dmf_cloud_downsample_device, dmf_position_cameras_device,
dmf_grid_surface_views_device) on bench.py's fused scene: a 512^3 grid fused
from 128 rendered 640x480 frames (setup as tools/exp_surface.py), its extracted surface (about 419 k
oriented points) downsampled with leaves 0.1, 0.05 and 0.02 and cameras placed 300 mm out.
Per leaf, device events around warmed calls: the downsample without outputs (bounds, keys, sort and
heads), the whole downsample (the difference is the leaf walk), the placement, and the whole
dmf_grid_surface_views_device from the grid (it synchronises once for the surface count).  Alternating
with it in the same process, the host route the device calls replace: download of the surface, the
drop-in's pcl::VoxelGrid and Algorithms::positionCameras (compiled here with g++ into a small shared
object), upload of the poses; its poses are compared with the device's bit for bit.  Prints one JSON
line.  argv: [repeats >= 5].

Per stage: run `exp_views.py --trace` under `rocprofv3 --kernel-trace --output-format csv -d DIR -o run`
(a run of its own: TRACE_CALLS downsample + placement calls per leaf after a warm-up call), then
`exp_views.py --stages DIR` prints the median microseconds per call of each stage's kernels."""
import csv
import ctypes as C
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "depth-map-fusion-utils_amd")
LEAVES = (0.1, 0.05, 0.02)
DIST_MM = 300
TRACE_CALLS = 5
STAGES = (("bounds_keys", ("k_vw_init", "k_vw_bounds", "k_vw_setup", "k_vw_keys")),
          ("sort", ("radix", "sort", "onesweep", "histogram")),
          ("heads", ("k_vw_flags", "scan", "lookback", "k_vw_starts", "k_vw_maxpop", "k_vw_totals")),
          ("means", ("k_vw_means",)), ("placement", ("k_vw_place",)))


def stages(d):
    files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        sys.exit("no kernel_trace.csv under " + d)
    rows = sorted(csv.DictReader(open(files[0])), key=lambda r: int(r["Start_Timestamp"]))
    calls, cur = [], None       # one dict of stage -> ns per downsample + placement call
    for r in rows:
        name = r["Kernel_Name"]
        if "k_vw_init" in name:
            cur = dict.fromkeys([s for s, _ in STAGES], 0)
            calls.append(cur)
        if cur is None:
            continue
        for s, keys in STAGES:
            if any(k in name for k in keys):
                cur[s] += int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
                break
    per = 1 + TRACE_CALLS
    out = {}
    for i, leaf in enumerate(LEAVES):
        mine = calls[i * per + 1:(i + 1) * per]
        out[str(leaf)] = {s: round(float(np.median([c[s] for c in mine])) / 1e3, 1) for s, _ in STAGES} if mine else None
    print(json.dumps({"stage_us_per_call": out, "calls_seen": len(calls)}))


if len(sys.argv) > 2 and sys.argv[1] == "--stages":
    stages(sys.argv[2])
    sys.exit(0)

import torch  # noqa: E402

sys.path[:0] = [ROOT, PKG]
import dmf_amd  # noqa: E402
from dmf_amd import _lib, scene  # noqa: E402

HOST_SRC = r'''
#include <pcl/point_cloud.h>
#include <pcl/point_types.h>
#include "Algorithms.hpp"
#include "PointCloudProcessing.hpp"
// the host route of the reference's planners over n oriented points -> the number of poses (<= cap written)
extern "C" long long host_views(const float* xyz, const float* nrm, long long n, double leaf, unsigned dist,
                                float* poses, long long cap) {
  using Cloud = pcl::PointCloud<pcl::PointXYZRGBNormal>;
  Cloud::Ptr cloud(new Cloud), loc(new Cloud);
  cloud->points.resize(n);
  for (long long i = 0; i < n; ++i) {
    pcl::PointXYZRGBNormal& p = cloud->points[i];
    p.x = xyz[3 * i]; p.y = xyz[3 * i + 1]; p.z = xyz[3 * i + 2];
    for (int a = 0; a < 3; ++a) p.normal[a] = nrm[3 * i + a];
  }
  PointCloudProcessing::downsample<pcl::PointXYZRGBNormal>(cloud, loc, leaf);
  const std::vector<Eigen::Affine3f> cams = Algorithms::positionCameras(loc, dist);
  for (size_t i = 0; i < cams.size() && (long long)i < cap; ++i) dmf_compat::pose12(cams[i], poses + 12 * i);
  return (long long)cams.size();
}
'''

TRACE = len(sys.argv) > 1 and sys.argv[1] == "--trace"
REPEATS = max(5, int(sys.argv[1])) if len(sys.argv) > 1 and not TRACE else 7
W, H, P, N = 640, 480, 128, 512
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
_lib.check(L.dmf_fuse_depth_device(vol._h, C.addressof(cam), d_depth.data_ptr(), d_poses.data_ptr(), P, C.addressof(prm),
                                   hits.data_ptr(), misses.data_ptr(), None))
_lib.check(L.dmf_fuse_finalize_device(vol._h, hits.data_ptr(), misses.data_ptr(), C.addressof(prm), logodds.data_ptr()))
torch.cuda.synchronize(dev)
_lib.fuse_status(vol)
del hits, misses, d_depth

count = torch.zeros(3, dtype=torch.int64, device=dev)
one = torch.zeros(3, dtype=torch.float32, device=dev)
_lib.check(L.dmf_grid_surface_device(vol._h, logodds.data_ptr(), 1, -1, None, one.data_ptr(), None, 1, count.data_ptr()))
torch.cuda.synchronize(dev)
n_surface = int(count[0].item())
sx = torch.empty(3 * max(n_surface, 1), dtype=torch.float32, device=dev)
sn = torch.empty(3 * max(n_surface, 1), dtype=torch.float32, device=dev)
_lib.check(L.dmf_grid_surface_device(vol._h, logodds.data_ptr(), 1, -1, None, sx.data_ptr(), sn.data_ptr(), n_surface,
                                     count.data_ptr()))
torch.cuda.synchronize(dev)


def leaf_arr(leaf):
    return np.full(3, leaf, np.float32)


def downsample(leaf, ox, on, cap):
    _lib.check(L.dmf_cloud_downsample_device(vol._h, sx.data_ptr(), sn.data_ptr(), n_surface, leaf_arr(leaf).ctypes.data, 0,
                                             ox.data_ptr() if ox is not None else None,
                                             on.data_ptr() if on is not None else None, None, cap, count.data_ptr()))


def place(ox, on, m, dp):
    _lib.check(L.dmf_position_cameras_device(vol._h, ox.data_ptr(), on.data_ptr(), m, DIST_MM, 0, dp.data_ptr()))


def sized(leaf):
    downsample(leaf, None, None, 0)
    torch.cuda.synchronize(dev)
    m, finite, largest = (int(x) for x in count.cpu().numpy())
    return m, finite, largest, [torch.empty(k * max(m, 1), dtype=torch.float32, device=dev) for k in (3, 3, 12)]


if TRACE:
    for leaf in LEAVES:
        m, _, _, (ox, on, dp) = sized(leaf)          # (the sizing call is the leaf's warm-up call in the trace)
        for _ in range(TRACE_CALLS):
            downsample(leaf, ox, on, m)
            place(ox, on, m, dp)
        torch.cuda.synchronize(dev)
    sys.exit(0)

tmp = tempfile.mkdtemp(prefix="exp_views_")
src, so = os.path.join(tmp, "host_views.cpp"), os.path.join(tmp, "host_views.so")
open(src, "w").write(HOST_SRC)
subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I", os.path.join(PKG, "compat"), "-I",
                os.path.join(PKG, "compat", "shims"), "-I", os.path.join(ROOT, "include"), "-o", so, src], check=True)
HL = C.CDLL(so)
HL.host_views.restype = C.c_longlong
HL.host_views.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_double, C.c_uint, C.c_void_p, C.c_longlong]


def timed(fn, calls=3):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    for _ in range(calls):
        fn()
    e1.record(s)
    torch.cuda.synchronize(dev)
    return e0.elapsed_time(e1) / calls


def stat(v):
    return {"min": round(min(v), 4), "median": round(float(np.median(v)), 4), "max": round(max(v), 4)}


result = {"grid": N, "surface_points": n_surface, "distance_mm": DIST_MM, "repeats": REPEATS, "leaves": {}}
for leaf in LEAVES:
    m, finite, largest, (ox, on, dp) = sized(leaf)
    cp, cx, cn = (torch.empty_like(t) for t in (dp, ox, on))
    host_poses = np.empty((max(m, 1), 12), np.float32)

    def chain():
        _lib.check(L.dmf_grid_surface_views_device(vol._h, logodds.data_ptr(), 1, -1, leaf_arr(leaf).ctypes.data, 0,
                                                   DIST_MM, 0, cp.data_ptr(), cx.data_ptr(), cn.data_ptr(), m,
                                                   count.data_ptr()))

    def host_route():
        t0 = time.perf_counter()
        hx, hn = sx.cpu().numpy(), sn.cpu().numpy()
        t1 = time.perf_counter()
        got = HL.host_views(hx.ctypes.data, hn.ctypes.data, n_surface, float(np.float32(leaf)), DIST_MM,
                            host_poses.ctypes.data, m)
        t2 = time.perf_counter()
        d = torch.from_numpy(host_poses).to(dev)
        torch.cuda.synchronize(dev)
        t3 = time.perf_counter()
        return got, d, [(t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3, (t3 - t0) * 1e3]

    downsample(leaf, ox, on, m)
    place(ox, on, m, dp)
    chain()
    got, d_host, _ = host_route()       # warm-up of every route
    torch.cuda.synchronize(dev)
    equal = bool(got == m and torch.equal(d_host.view(torch.int32).reshape(-1)[:12 * m], dp.view(torch.int32)[:12 * m])
                 and torch.equal(cp.view(torch.int32), dp.view(torch.int32)))
    t = {k: [] for k in ("count", "downsample", "placement", "chain", "chain_wall", "host", "host_download", "host_compute",
                         "host_upload")}
    for _ in range(REPEATS):            # the measurements alternate
        t["count"].append(timed(lambda: downsample(leaf, None, None, 0)))
        t["downsample"].append(timed(lambda: downsample(leaf, ox, on, m)))
        t["placement"].append(timed(lambda: place(ox, on, m, dp)))
        t["chain"].append(timed(chain))
        torch.cuda.synchronize(dev)
        w0 = time.perf_counter()
        chain()
        torch.cuda.synchronize(dev)
        t["chain_wall"].append((time.perf_counter() - w0) * 1e3)
        _, _, h = host_route()
        for k, v in zip(("host_download", "host_compute", "host_upload", "host"), h):
            t[k].append(v)
    r = {k: stat(v) for k, v in t.items()}
    r.update({"views": m, "finite_points": finite, "mean_population": round(finite / max(m, 1), 2),
              "largest_population": largest, "host_and_device_poses_equal": equal,
              "means_ms_by_difference": round(r["downsample"]["median"] - r["count"]["median"], 4),
              "host_over_chain_wall": round(r["host"]["median"] / r["chain_wall"]["median"], 1)})
    result["leaves"][str(leaf)] = r
print(json.dumps(result), flush=True)
