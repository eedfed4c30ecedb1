"""CPU: the gfx950 kernels' register budgets (hipcc cross-compiles here).  Every kernel of the
product keeps its state in registers: no scratch (private segment) and no spilled VGPRs.  A
select between struct fields or a per-axis constant indexed by a lane's axis can silently become
a dynamically indexed private array (one such change made pass B 15x slower in round 5), so the
code objects' metadata is checked at every CPU run.  The hot kernels' VGPR counts are pinned to
their occupancy bands.

The assembly comes from the Makefile's own rule (`$(OUT)/%.s`: the object rule's flags, per-file
ones included) and the sources from its SRCS: what is checked is what ships, and a new source is
covered without an edit here."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "depth-map-fusion-utils_amd")
HIPCC = "/opt/rocm/bin/hipcc"


def _srcs():
    """The Makefile's SRCS, as stems ("dmf_fuse")."""
    text = open(os.path.join(PKG, "Makefile")).read().replace("\\\n", " ")
    words = re.search(r"^SRCS\s*:=(.*)$", text, re.M).group(1).split()
    return [os.path.splitext(os.path.basename(w))[0] for w in words]


def _kernels(stem, tmp_path, extra=""):
    """{kernel symbol: metadata figures} of csrc/<stem>.hip as the Makefile compiles it (+ extra)."""
    out = tmp_path / "asm"
    asm = out / (stem + ".s")
    subprocess.run(["make", "-s", "-C", PKG, f"OUT={out}", f"EXTRA={extra}", str(asm)], check=True,
                   capture_output=True, timeout=600)
    meta = asm.read_text().split(".end_amdgpu_metadata")[0].split("amdhsa.kernels:")[-1]
    kernels = {}
    for block in re.split(r"\n  - ", meta)[1:]:
        name = re.search(r"\.name:\s+(\S+)", block)
        if not name:
            continue
        val = {k: int(m.group(1)) for k in ("private_segment_fixed_size", "vgpr_count", "vgpr_spill_count",
                                            "sgpr_spill_count")
               if (m := re.search(r"\." + k + r":\s+(\d+)", block))}
        kernels[name.group(1)] = val
    return kernels


def _has_kernels(stem):
    return "__global__" in open(os.path.join(PKG, "csrc", stem + ".hip")).read()


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
@pytest.mark.timeout(900)
@pytest.mark.parametrize("src", [s + ".hip" for s in _srcs()])
def test_no_scratch_no_spills(src, tmp_path):
    stem = src[:-len(".hip")]
    # the engine's own kernels (namespace dmf; rocPRIM's library kernels are not ours)
    ks = {n: v for n, v in _kernels(stem, tmp_path).items() if n.startswith("_ZN3dmf")}
    assert ks or not _has_kernels(stem), "no kernels parsed"
    bad = {n: v for n, v in ks.items() if v.get("private_segment_fixed_size", 0) or v.get("vgpr_spill_count", 0)}
    assert not bad, f"kernels with scratch or VGPR spills: {bad}"
    if src == "dmf_fuse.hip":
        f = [v for n, v in ks.items() if "k_bk_fuse_s" in n]
        b = [v for n, v in ks.items() if "k_bk_pairsILb1" in n]
        assert f and all(v["vgpr_count"] <= 64 for v in f)   # phase F: LDS bounds it to 4 waves/SIMD anyway
        assert b and all(v["vgpr_count"] <= 128 for v in b)  # pass B: 4 waves per SIMD
    if src == "dmf_trace.hip":
        r = [v for n, v in ks.items() if "k_reverse_x" in n]
        assert r and all(v["vgpr_count"] <= 80 for v in r)   # reverseRayTraceFast: 6 waves per SIMD


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
@pytest.mark.timeout(900)
@pytest.mark.parametrize("src", ["dmf_fuse", "dmf_trace"])
def test_stats_build_compiles(src, tmp_path):
    """DMF_EXP_STATS, the one diagnostic build the sources keep (bench.py and tools/exp_*.py read
    its counters), still compiles; its register figures are its own and are not pinned."""
    ks = {n for n in _kernels(src, tmp_path, extra="-DDMF_EXP_STATS") if n.startswith("_ZN3dmf")}
    assert ks, "no kernels parsed"
