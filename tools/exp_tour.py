#!/usr/bin/env python3
"""Timing of the tour (dmf_tour*_device) on device-resident cost maps:
Euclidean maps (int(dist * 1000) between V random points of the unit cube, tests/tour_ref.py
euclid_map) at V = 256, 1024 and 4096, and -- unless --no-scene -- bench.py's collision cost map:
1024 centres on a 0.45 m sphere in the 512^3 volume integrated from 16 back-projected 640x480 frames
(setup as tools/exp_costmap.py), made on the device by dmf_collision_cost_map_device.
Per map: nearest neighbour alone, 2-opt alone from the nearest-neighbour path, and the whole
dmf_tour_device; each is warmed once and then timed REPEATS times with device events on the
volume's stream around one call (the calls wait for their own rounds, so this is what a caller
sees): min / median / max ms.  From dmf_tour_stats and info: the improvements, the rounds launched,
the batches, the share of a scan's candidates that stood ahead of the first improving one (mean over
the improving scans), and microseconds per round (2-opt's median over the rounds that had work:
improvements + 1).
Baseline: the SAME prefix-sum first-improvement algorithm on the host, tests/tour_ref.py two_opt
(numpy, one vectorised pass over all candidates per round), from the same nearest-neighbour path:
run to the end for V <= 1024 and for --baseline-rounds rounds (default 10) above, where only its
time per round is reported.  The result paths are compared: the final ones for V <= 1024; above,
the engine's path cut at the baseline's round count against the baseline's, plus a host scan of the
engine's final path (it must find nothing to improve) and a recomputation of its length; the
nearest-neighbour path against tour_ref's at every size.  With --literal the reference's own
O(V^3)-per-improvement loop (tour_ref.two_opt_literal) is also timed at V = 256, for the record.
Prints one JSON line.  argv: [--repeats N >= 3] [--no-scene] [--literal] [--baseline-rounds N]
[--sizes 256,1024,4096]."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "depth-map-fusion-utils_amd"), os.path.join(ROOT, "tests")]
import dmf_amd  # noqa: E402
import tour_ref as TO  # noqa: E402
from dmf_amd import _lib, scene  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--no-scene", action="store_true")
ap.add_argument("--literal", action="store_true")
ap.add_argument("--baseline-rounds", type=int, default=10)
ap.add_argument("--sizes", default="256,1024,4096")
args = ap.parse_args()
REPEATS = max(3, args.repeats)

dev = torch.device("cuda", 0)
L = _lib.load()
s = torch.cuda.current_stream(dev)


def scene_map():
    """bench.py's collision cost map, left on the device."""
    W, H, NI, Vc = 640, 480, 16, 1024
    K = scene.intrinsics(W, H)
    poses = np.ascontiguousarray(scene.fibonacci_poses(128, seed=1234)[:NI], np.float32)
    rendered = [scene.render(K, W, H, p) for p in poses]
    depth = np.ascontiguousarray(np.stack([r[0] for r in rendered]), np.uint16)
    nrm = np.concatenate([r[1].reshape(-1, 3) for r in rendered])
    vol = dmf_amd.VoxelVolume(0)
    vol.set_stream(s.cuda_stream)
    vol.setDimensions(-0.5, 0.5, -0.5, 0.5, -0.5, 0.5)
    vol.setVolumeSize(512, 512, 512)
    vol.constructVolume()
    cam = _lib.make_camera(K, H, W)
    d_depth = torch.from_numpy(depth.view(np.int16)).to(dev)
    d_poses = torch.from_numpy(poses).to(dev)
    xyz = torch.empty((NI, H, W, 3), dtype=torch.float32, device=dev)
    _lib.check(L.dmf_backproject_device(vol._h, C.addressof(cam), d_depth.data_ptr(), d_poses.data_ptr(), NI,
                                        xyz.data_ptr()))
    valid = (d_depth > 0).reshape(-1)
    pts = xyz.reshape(-1, 3)[valid].contiguous()
    d_nrm = torch.from_numpy(nrm).to(dev).reshape(-1, 3)[valid].contiguous()
    vol.integrate_device(pts.data_ptr(), d_nrm.data_ptr(), pts.shape[0])
    d_cp = torch.from_numpy(scene.sphere_centres(Vc)).to(dev)
    cmap = torch.empty((Vc, Vc), dtype=torch.int32, device=dev)
    _lib.check(L.dmf_collision_cost_map_device(vol._h, d_cp.data_ptr(), Vc, cmap.data_ptr()))
    torch.cuda.synchronize(dev)
    return vol, cmap


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    fn()
    e1.record(s)
    torch.cuda.synchronize(dev)
    return e0.elapsed_time(e1)


def summary(v):
    return {"min": round(min(v), 4), "median": round(float(np.median(v)), 4), "max": round(max(v), 4)}


def measure(vol, cmap):
    V = cmap.shape[0]
    path = torch.empty(V, dtype=torch.int32, device=dev)
    nn_path = torch.empty(V, dtype=torch.int32, device=dev)
    info = torch.zeros(5, dtype=torch.int64, device=dev)
    _lib.check(L.dmf_tour_nearest_neighbour_device(vol._h, cmap.data_ptr(), V, nn_path.data_ptr(), info.data_ptr()))
    torch.cuda.synchronize(dev)

    def nn():
        _lib.check(L.dmf_tour_nearest_neighbour_device(vol._h, cmap.data_ptr(), V, path.data_ptr(), info.data_ptr()))

    def two_opt():
        path.copy_(nn_path)
        _lib.check(L.dmf_tour_two_opt_device(vol._h, cmap.data_ptr(), V, path.data_ptr(), 0, info.data_ptr()))

    def whole():
        _lib.check(L.dmf_tour_device(vol._h, cmap.data_ptr(), V, path.data_ptr(), 0, info.data_ptr()))

    out = {"V": V}
    for name, fn in (("nearest_neighbour", nn), ("two_opt", two_opt), ("tour", whole)):
        fn()
        torch.cuda.synchronize(dev)
        out[name + "_ms"] = summary([timed(fn) for _ in range(REPEATS)])
    st = np.zeros(4, np.uint64)
    _lib.check(L.dmf_tour_stats(vol._h, st.ctypes.data))
    forced, applied, conv, length, nopath = (int(x) for x in info.cpu().numpy())
    cand = (V - 1) * (V - 2) // 2
    out.update({"forced_picks": forced, "improvements": applied, "converged": conv, "length": length,
                "int_max_edges": nopath, "rounds_launched": int(st[0]), "batches": int(st[1]),
                "candidates_per_scan": cand,
                "share_ahead_of_first_improving": round(int(st[3]) / max(applied * cand, 1), 4),
                "us_per_round_two_opt": round(out["two_opt_ms"]["median"] * 1e3 / (applied + 1), 3)})
    m = cmap.cpu().numpy()
    start = nn_path.cpu().numpy().tolist()
    full = V <= 1024
    t0 = time.perf_counter()
    ref, n, _ = TO.two_opt(m, start, 0 if full else args.baseline_rounds)
    dt = time.perf_counter() - t0
    out["baseline"] = {"what": "tests/tour_ref.py two_opt (numpy prefix sums, host)", "rounds": n + (1 if full else 0),
                       "ms": round(dt * 1e3, 2) if full else None,
                       "us_per_round": round(dt * 1e6 / (n + (1 if full else 0)), 1)}
    if full:
        out["baseline"]["same_path"] = bool(ref == path.cpu().numpy().tolist())
    else:
        # above 1024 views the baseline stops after a few rounds: the engine cut at the same round must
        # hold the same path, and its final path must be one in which a host scan finds nothing to improve
        final = path.cpu().numpy().tolist()
        path.copy_(nn_path)
        _lib.check(L.dmf_tour_two_opt_device(vol._h, cmap.data_ptr(), V, path.data_ptr(), args.baseline_rounds,
                                             info.data_ptr()))
        torch.cuda.synchronize(dev)
        out["baseline"]["same_path_after_its_rounds"] = bool(ref == path.cpu().numpy().tolist())
        out["final_path_host_scan_finds_nothing"] = bool(TO.two_opt(m, final, 1)[1] == 0)
        out["final_length_recomputed_equal"] = bool(TO.edge_sums(m, final) == (length, nopath))
    out["nearest_neighbour_same_as_host"] = bool(TO.nearest_neighbour(m)[0] == start)
    if args.literal and V == 256:
        t0 = time.perf_counter()
        lit = TO.two_opt_literal(m, start)
        out["reference_loop_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        out["reference_loop_same_path"] = bool(lit[0] == path.cpu().numpy().tolist())
    return out


results = []
vol = None
if not args.no_scene:
    vol, cmap = scene_map()
    r = measure(vol, cmap)
    r["map"] = "collision cost map, 1024 sphere centres, 512^3 volume"
    results.append(r)
if vol is None:
    vol = dmf_amd.VoxelVolume(0)
    vol.set_stream(s.cuda_stream)
for V in (int(x) for x in args.sizes.split(",") if x):
    r = measure(vol, torch.from_numpy(TO.euclid_map(V, 1)).to(dev))
    r["map"] = "euclid"
    results.append(r)
print(json.dumps({"repeats": REPEATS, "results": results}), flush=True)
