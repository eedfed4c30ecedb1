#!/usr/bin/env python3
"""Record tests/golden/fuse_plan_parent.json: what dmf_fuse_reserve + dmf_fuse_plan answer for
the cases below (tests/test_gpu_fuse_plan.py compares the library under test with it).

The plan (bk_plan, dmf_fuse.hip) decides how every large fusion call is cut into batches, so
the fixture is recorded from a build of the commit BEFORE a change to the planning code, never
from the code under test:

    DMF_LIB=<parent checkout>/depth-map-fusion-utils_amd/build/libdmf.so \\
        python tests/golden/gen_fuse_plan.py <parent commit hash>

Every budget is explicit, so the figures do not depend on the card's memory.  The script
refuses to write a fixture in which a case other than the deliberately starved budgets fails,
or in which the three budgets of the batch-count cases do not give three outcomes.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "depth-map-fusion-utils_amd")]

OUT = os.path.join(HERE, "fuse_plan_parent.json")
MIB = 1 << 20
SLAB, CELL_WALK, DEFAULT = 57, 40, 0
# 64^3 = 2 x 2 x 2 bricks of 32^3 cells; a 64x48 camera = 48 packets = 3072 rays per pose,
# <= 4 pairs per ray: one pose makes at most 12288 pairs and takes 73940 bytes of per-pose tables
BASE = {"grid": [64, 64, 64], "camera": [64, 48], "P": 8, "variant": SLAB, "pipelined": False, "knobs": {},
        "budget": 16 * MIB}
# budgets: every pose in one batch | several batches | not one pose's pairs (starved: an error)
BUDGETS = {"16m": 16 * MIB, "1m": 1 * MIB, "256k": 256 << 10}
STARVED = "256k"


def cases():
    out = {}
    for pipelined in (False, True):  # pipelined: two staging slots of half the budget each
        for tag, budget in BUDGETS.items():
            out[("staged_" if pipelined else "serial_") + tag] = dict(BASE, budget=budget, pipelined=pipelined)
    out["cell_walk"] = dict(BASE, variant=CELL_WALK)  # 24-byte pair records
    out["default_small"] = dict(BASE, variant=DEFAULT)  # k_fuse_l below 256 cells: brick = 0
    out["knob_super_poses"] = dict(BASE, knobs={"super_poses": 3})
    out["knob_batch_poses"] = dict(BASE, knobs={"batch_poses": 2})
    out["knob_pair_cap"] = dict(BASE, knobs={"pair_cap": 12300})  # just above one pose's 12288
    out["knob_span"] = dict(BASE, knobs={"span": 4})
    # (the hashed histogram's size is not in dmf_fuse_plan_info and moves no byte count: this case
    # pins only that the knob leaves the plan as it is)
    out["knob_a_hash"] = dict(BASE, knobs={"a_hash": 64})
    out["partial_bricks"] = dict(BASE, grid=[72, 40, 24])  # 3 x 2 x 1 bricks, the last ones partial
    out["odd_camera"] = dict(BASE, camera=[70, 50])  # sides no multiples of the 8x8 packet
    # 32 x 32 x 9 = 9216 bricks > kBkBigHist (8192): the hashed pass A (hash_log 11, span 128) is
    # planned.  Bricks are 32^3 cells and an axis holds at most 32 of them, so no grid that is
    # long along one axis only gets there.  The plan shows the branch through its span alone: a
    # 64x136 camera has 136 packets per pose, two pass-A workgroups at span 128 against one at
    # the direct table's 256, and the per-workgroup tables in scratch_bytes double with them.
    out["hashed_default"] = dict(BASE, grid=[1000, 1000, 260], camera=[64, 136], P=2, budget=64 * MIB)
    return out


def run_case(case):
    """(reserve status, plan status, the eight dmf_fuse_plan_info fields) of one case, through the
    library dmf_amd._lib loads."""
    import ctypes as C

    import torch

    import dmf_amd
    from dmf_amd import _lib
    L = _lib.load()
    vol = dmf_amd.VoxelVolume(0)
    nx, ny, nz = case["grid"]
    vol.setDimensions(0.0, nx * 0.01, 0.0, ny * 0.01, 0.0, nz * 0.01)
    vol.setVolumeSize(nx, ny, nz)
    vol.constructVolume()
    _lib.set_variant(vol, case["variant"])
    inp = torch.cuda.Stream(torch.device("cuda", 0)) if case["pipelined"] else None
    if inp is not None:
        vol.set_fuse_input_stream(inp.cuda_stream)
    for k, val in case["knobs"].items():
        _lib.set_knob(vol, k, val)
    W, H = case["camera"]
    cam = _lib.make_camera([[W, 0, W / 2], [0, W, H / 2], [0, 0, 1]], H, W)
    info = _lib.dmf_fuse_plan_info()
    rs = L.dmf_fuse_reserve(vol._h, C.addressof(cam), case["P"], case["budget"])
    ps = L.dmf_fuse_plan(vol._h, C.addressof(cam), case["P"], C.addressof(info))
    if inp is not None:
        vol.set_fuse_input_stream(None)
    vol.close()
    return int(rs), int(ps), {k: int(getattr(info, k)) for k, _ in _lib.dmf_fuse_plan_info._fields_}


def main():
    parent = sys.argv[1]
    rec = {}
    for name, case in cases().items():
        rs, ps, plan = run_case(case)
        rec[name] = dict(case, reserve_status=rs, plan_status=ps, plan=plan)
        print(name, rs, ps, plan, flush=True)
        assert (rs, ps) == (0, 0) or name.endswith(STARVED), f"{name}: fix the case, not the expectation"
    for mode in ("serial_", "staged_"):
        one, many, starved = (rec[mode + t] for t in BUDGETS)
        assert one["plan"]["max_batches"] == 1 and many["plan"]["max_batches"] > 1 and starved["plan_status"] != 0, mode
    with open(OUT, "w") as f:
        f.write(json.dumps({"parent": parent, "cases": rec}, indent=1, sort_keys=True) + "\n")
    print("wrote", OUT)


if __name__ == "__main__":
    main()
