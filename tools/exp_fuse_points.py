#!/usr/bin/env python3
"""What the order of a point cloud costs the fusion (run on the GPU box).

The bench's scene (config 4 shard: 128 frames of 640x480 into 512^3, or --grid / --poses /
--image) is fused from its depth frames (dmf_fuse_depth_device) and, in the same process, from
the same rays as points (dmf_fuse_points_device): the frames back-projected on the device, the
pixels outside the depth gate set to NaN, one scan per frame with the pose's translation as its
origin, in three orders:

  packet   each frame's points permuted into 8x8-packet order: every 64-ray packet holds the
           rays of the depth call's packet
  rows     row-major image order
  random   one fixed random permutation per frame

Per case: ms per serial call (HIP events, warm-up, the median of --reps blocks of --calls
calls), whether the counters and stats[0..2] equal the depth call's, and pass A's own ms from a
kernel trace: unless --no-trace, each case is run again in a child process under rocprofv3
--kernel-trace --stats, into --profile-dir.  Prints one JSON line."""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "depth-map-fusion-utils_amd")]
import dmf_amd  # noqa: E402
from dmf_amd import _lib, scene  # noqa: E402

CASES = ("depth", "packet", "rows", "random")

ap = argparse.ArgumentParser()
ap.add_argument("--grid", type=int, default=512)
ap.add_argument("--poses", type=int, default=128)
ap.add_argument("--image", default="640x480")
ap.add_argument("--calls", type=int, default=10)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--profile-dir", default=os.path.join(ROOT, "profiles", "fuse_points"))
ap.add_argument("--no-trace", action="store_true")
ap.add_argument("--trace-case", choices=CASES, help="(child run) only this case, --calls calls, no timing")
a = ap.parse_args()
W, H = (int(x) for x in a.image.split("x"))
P = a.poses
dev = torch.device("cuda", 0)
K = scene.intrinsics(W, H)
cache = f"/tmp/exp_depth_{W}x{H}_{P}.npy"
poses = np.ascontiguousarray(scene.fibonacci_poses(P, seed=1234), np.float32)
if os.path.exists(cache):
    depth = np.load(cache)
else:
    print(f"[exp_fuse_points] rendering {P} frames", file=sys.stderr, flush=True)
    depth = np.ascontiguousarray(scene.render_frames(K, W, H, poses), np.uint16)
    np.save(cache, depth)
L = _lib.load()
vol = dmf_amd.VoxelVolume(0)
main = torch.cuda.Stream(dev)
vol.set_stream(main.cuda_stream)
vol.setDimensions(-0.5, 0.5, -0.5, 0.5, -0.5, 0.5)
vol.setVolumeSize(a.grid, a.grid, a.grid)
vol.constructVolume()
cam = _lib.make_camera(K, H, W)
prm = _lib.default_fuse_params(dmin_mm=scene.DEPTH_MIN_MM, dmax_mm=scene.DEPTH_MAX_MM)
nct = C.c_int64()
_lib.check(L.dmf_fuse_counter_cells(vol._h, C.addressof(nct)))
nt = nct.value
d_depth = torch.from_numpy(depth.view(np.int16)).to(dev)
d_poses = torch.from_numpy(poses).to(dev)
cnt = torch.zeros(2 * nt, dtype=torch.int32, device=dev)
st = torch.zeros(8, dtype=torch.int64, device=dev)

# the frames as points (dmf_backproject_device: bit-exact endpoints), gated-out pixels NaN
xyz = torch.empty((P, H * W, 3), dtype=torch.float32, device=dev)
with torch.cuda.stream(main):
    _lib.check(L.dmf_backproject_device(vol._h, C.addressof(cam), d_depth.data_ptr(), d_poses.data_ptr(), P,
                                        xyz.data_ptr()))
    dmm = d_depth.view(P, H * W).to(torch.int32) & 0xffff
    xyz[(dmm < prm.dmin_mm) | (dmm >= prm.dmax_mm)] = float("nan")
    origins = d_poses.view(P, 3, 4)[:, :, 3].contiguous()
torch.cuda.synchronize(dev)


def ordered(case):
    """(P, N, 3) points of the frames in the case's order (N >= H * W: the 8x8 packets of a frame
    whose sides are no multiples of 8 are padded with NaN)."""
    if case == "rows":
        return xyz
    if case == "random":
        g = torch.Generator(device="cpu").manual_seed(4321)
        out = torch.empty_like(xyz)
        for p in range(P):
            out[p] = xyz[p][torch.randperm(H * W, generator=g).to(dev)]
        return out
    pkx, pky = (W + 7) // 8, (H + 7) // 8
    q = torch.arange(pkx * pky).view(-1, 1)
    lane = torch.arange(64).view(1, -1)
    r, c = (q // pkx) * 8 + (lane >> 3), (q % pkx) * 8 + (lane & 7)
    inside = ((r < H) & (c < W)).reshape(-1).to(dev)
    idx = (torch.clamp(r, max=H - 1) * W + torch.clamp(c, max=W - 1)).reshape(-1).to(dev)
    out = xyz[:, idx].contiguous()
    out[:, ~inside] = float("nan")
    return out


def caller(case):
    if case == "depth":
        _lib.check(L.dmf_fuse_reserve(vol._h, C.addressof(cam), P, 0))
        return (lambda: _lib.check(L.dmf_fuse_depth_device(
            vol._h, C.addressof(cam), d_depth.data_ptr(), d_poses.data_ptr(), P, C.addressof(prm), cnt.data_ptr(),
            cnt.data_ptr() + 4 * nt, st.data_ptr()))), None
    pts = ordered(case)
    N = pts.shape[1]
    _lib.check(L.dmf_fuse_points_reserve(vol._h, P, N, 0))
    return (lambda: _lib.check(L.dmf_fuse_points_device(
        vol._h, pts.data_ptr(), origins.data_ptr(), P, N, C.addressof(prm), cnt.data_ptr(), cnt.data_ptr() + 4 * nt,
        st.data_ptr()))), pts


def kernel_ms(case):
    """The case again in a child process under rocprofv3 --kernel-trace --stats -> average ms per
    launch of every dmf:: kernel."""
    prof = shutil.which("rocprofv3")
    if prof is None:
        return None
    d = os.path.join(a.profile_dir, case)
    cmd = [prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "run", "--", sys.executable,
           os.path.abspath(__file__), "--grid", str(a.grid), "--poses", str(P), "--image", a.image, "--calls", "5",
           "--trace-case", case]
    r = subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=400)
    if r.returncode != 0:
        print(f"[exp_fuse_points] trace of {case} failed ({r.returncode}): {r.stderr.decode(errors='replace')[-400:]}",
              file=sys.stderr, flush=True)
        return None
    kt = {}
    for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(f)):
            k = row["Name"].split("(")[0].replace("void ", "").strip()
            if k.startswith("dmf::k_bk_") or k.startswith("dmf::k_fuse_l"):
                kt[k] = {"avg_ms": float(row["AverageNs"]) * 1e-6, "calls": int(row["Calls"])}
    return kt


if a.trace_case:
    call, _keep = caller(a.trace_case)
    torch.cuda.synchronize(dev)
    with torch.cuda.stream(main):
        for _ in range(1 + a.calls):
            call()
    torch.cuda.synchronize(dev)
    sys.exit(0)

out = {"grid": a.grid, "poses": P, "image": a.image, "calls": a.calls, "reps": a.reps, "cases": {}}
ref = None
for case in CASES:
    print(f"[exp_fuse_points] case {case}", file=sys.stderr, flush=True)
    call, _keep = caller(case)
    cnt.zero_()
    st.zero_()
    torch.cuda.synchronize(dev)
    with torch.cuda.stream(main):
        call()
    torch.cuda.synchronize(dev)
    res = {"updates": int(st[0].item()), "rays": int(st[1].item()), "hits": int(st[2].item()),
           "layout_faults": int(st[3].item()), "pairs": int(st[4].item())}
    if ref is None:
        ref = (cnt.clone(), st[:3].clone())
    else:
        res["equals_depth"] = bool(torch.equal(cnt, ref[0]) and torch.equal(st[:3], ref[1]))
    for _ in range(3):
        call()
    torch.cuda.synchronize(dev)
    blocks = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(main)
        for _ in range(a.calls):
            call()
        e1.record(main)
        torch.cuda.synchronize(dev)
        blocks.append(e0.elapsed_time(e1) / a.calls)
    res["ms"] = statistics.median(blocks)
    res["ms_min"], res["ms_max"] = min(blocks), max(blocks)
    out["cases"][case] = res
    del call, _keep
out["kernel"] = _lib.kernel_name(vol)
for case in CASES[1:]:
    out["cases"][case]["ms_over_depth"] = out["cases"][case]["ms"] / out["cases"]["depth"]["ms"]
if not a.no_trace:
    # the traced runs are processes of their own: this one gives its device memory back first
    vol.close()
    del cnt, xyz, d_depth, ref
    torch.cuda.empty_cache()
    out["profile_dir"] = os.path.relpath(a.profile_dir, ROOT)
    for case in CASES:
        kt = kernel_ms(case)
        out["cases"][case]["kernel_avg_ms"] = kt
        if kt:
            out["cases"][case]["pass_a_ms"] = sum(v["avg_ms"] for k, v in kt.items() if k.startswith("dmf::k_bk_rays"))
print(json.dumps(out), flush=True)
