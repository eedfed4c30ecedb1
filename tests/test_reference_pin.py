"""The oracle pinned to the reference's own code.

tests/golden/ref_pin_<scene>.npz hold scenes and what the reference's headers (Camera.hpp,
Volume.hpp, CommonUtilities.hpp, RayTracingEngine.hpp, OccupancyGrid.hpp, compiled unchanged
into oracle/_ref/ by `make -C oracle` and driven by oracle/ref_pin/*.cpp) computed on them;
tests/golden/gen_ref_pin.py describes the scenes, tests/ref_pin.py the formats and the plan.

(a) the oracle, on every fixture's inputs, gives every recorded output: exact equality, no
    reference needed, never skipped; so do the host formulas of dmf_amd.Camera / degree;
(b) where a reference checkout exists, the binaries built from it reproduce the fixtures;
(c) the binaries that sum three terms in the other order, (a0 + a1) + a2, give the same on the
    exact tier; on the general tier the number of entries that differ is reported (and kept
    in the fixture's meta): it says how much of that tier rests on the stand-in's Eigen order.
"""
import functools
import hashlib
import os
import subprocess

import pytest

import ref_pin as RP

HAVE_REF = os.path.isfile(os.path.join(RP.REFERENCE, "include", "RayTracingEngine.hpp"))
needs_ref = pytest.mark.skipif(not HAVE_REF, reason="reference checkout absent")
EXES = ("ref_pin_core", "ref_pin_core_left", "ref_pin_ogrid", "ref_pin_ogrid_left")


@functools.lru_cache(maxsize=None)
def _fx(scene):
    return RP.load(scene)


@functools.lru_cache(maxsize=None)
def _oracle_core(scene):
    from oracle import oracle as O
    O.lib()
    return RP.run_core(RP.OracleBackend(O), _fx(scene))


def _records(fx, prefixes):
    return {k: v for k, v in RP.expected(fx).items() if k.startswith(prefixes)}


# ------------------------------------------------------------------------------------- (a)
PARTS = {"volume": ("vol_", "occ", "nn_"), "probes": ("probe_",), "reverse": ("rev_",),
         "forward": ("fwd_", "rtv_", "chain_")}


@pytest.mark.parametrize("part", sorted(PARTS))
@pytest.mark.parametrize("scene", RP.SCENES)
def test_oracle_reproduces_reference(scene, part):
    fx = _fx(scene)
    exp = _records(fx, PARTS[part])
    if part == "forward" and not int(fx["in_flags"]) & 2:
        assert not exp  # undefined in the reference on a truncating grid: nothing recorded
        return
    assert exp, (scene, part)
    got = {k: v for k, v in _oracle_core(scene).items() if k.startswith(PARTS[part])}
    assert RP.differences(got, exp) == []


@pytest.mark.parametrize("scene", [s for s in RP.SCENES if RP.has_ogrid(RP.load(s))])
def test_oracle_reproduces_reference_ogrid(scene, oracle):
    fx = _fx(scene)
    exp = _records(fx, ("og_",))
    assert len(exp) == 9
    assert RP.differences(RP.run_ogrid(RP.OracleBackend(oracle), fx), exp) == []


@pytest.mark.parametrize("scene", ["exact", "general"])
def test_python_camera_mirror_reproduces_reference(scene):
    """dmf_amd.Camera's helpers and dmf_amd.degree are host formulas in Python (no kernel, no GPU):
    projectPoint, transformPoints, deProjectPoint, validPixel, degree against the probes."""
    import dmf_amd
    fx = _fx(scene)
    exp = {k: v for k, v in _records(fx, ("probe_",)).items() if k in RP.PROBE_TYPES}
    assert len(exp) == 5 and all(v.size for v in exp.values())
    assert RP.differences(RP.run_camera_probes(RP.GpuBackend(dmf_amd), fx), exp) == []


def test_fixtures_cover_what_they_claim():
    """Sizes and shape of the committed fixtures (the generator asserts the rest when it runs)."""
    for scene in RP.SCENES:
        fx = _fx(scene)
        assert os.path.getsize(RP.fixture_path(scene)) <= 256 * 1024
        V = fx["out_occ"].size
        assert {"exact": 3000 <= V <= 5000, "general": 3000 <= V <= 5000, "general_trunc": 3000 <= V <= 5000,
                "one": V == 1, "empty": V == 0}[scene], V
    assert _fx("exact")["meta"]["order_sensitive"][0] == 0
    assert "nn_occ" in RP.expected(_fx("exact")) and "nn_occ" not in RP.expected(_fx("general"))


# ------------------------------------------------------------------------------- (b), (c)
@pytest.fixture(scope="module")
def ref_runs(tmp_path_factory):
    """Every reference binary on every scene, all started at once: {(exe, scene): raw result}."""
    subprocess.run(["make", "-s", "-C", os.path.join(RP.ROOT, "oracle"), "ref_pin"], check=True)
    tmp = str(tmp_path_factory.mktemp("ref_pin"))
    started = {}
    for scene in RP.SCENES:
        fx = _fx(scene)
        for exe in EXES:
            if "ogrid" in exe and not RP.has_ogrid(fx):
                continue
            path = os.path.join(RP.REF_BIN, exe)
            assert os.path.isfile(path), path
            data = RP.ogrid_scene_bytes(fx) if "ogrid" in exe else RP.core_scene_bytes(fx)
            started[exe, scene] = RP.start_binary(path, data, tmp, f"{exe}_{scene}")
    return {k: f() for k, f in started.items()}


def _which(fx, exe):
    return _records(fx, ("og_",)) if "ogrid" in exe else \
        {k: v for k, v in RP.expected(fx).items() if not k.startswith("og_")}


@needs_ref
@pytest.mark.parametrize("scene", RP.SCENES)
def test_reference_binaries_reproduce_fixtures(ref_runs, scene):
    fx = _fx(scene)
    for exe in ("ref_pin_core", "ref_pin_ogrid"):
        if (exe, scene) not in ref_runs:
            continue
        raw = ref_runs[exe, scene]
        assert RP.differences(RP.parse_result(raw), _which(fx, exe)) == []
        assert hashlib.sha256(raw).hexdigest() == fx["meta"]["sha256_" + exe.split("_")[-1]]


@needs_ref
@pytest.mark.parametrize("scene", RP.SCENES)
def test_other_sum_order(ref_runs, scene, record_property):
    fx = _fx(scene)
    nd = nt = 0
    for exe in ("ref_pin_core_left", "ref_pin_ogrid_left"):
        if (exe, scene) in ref_runs:
            d, t = RP.count_differing(RP.parse_result(ref_runs[exe, scene]), _which(fx, exe))
            nd, nt = nd + d, nt + t
    record_property("order_sensitive_entries", nd)
    print(f"{scene}: {nd} of {nt} entries differ under (a0 + a1) + a2")
    if fx["meta"]["tier"] == "exact":
        assert nd == 0
