"""GPU: the fusion plan is pinned.  dmf_fuse_plan's figures (poses per super-batch and per batch,
pair capacity, batch count, scratch bytes, slots) decide how every large call is cut into
batches; a slip in the byte arithmetic of bk_plan (dmf_fuse.hip) would change them silently.

Each case of tests/golden/fuse_plan_parent.json creates a volume, sets the variant, optionally
an input stream (pipelined) and knobs, reserves under an explicit budget and asks for the plan:
the two status codes and all eight fields of dmf_fuse_plan_info equal the recorded ones.

The fixture was recorded by tests/golden/gen_fuse_plan.py from a build of the parent commit
62b542335df033f18d5fcfa675a628ad7a0acf7b (the last one before the fusion host code moved its
buffer sizes into one table), never from the code under test.  The cases are the smallest
shapes that reach each branch of bk_plan: one batch / several / a starved budget, serial and
staged; 24-byte records; the k_fuse_l route (brick = 0); the knobs that change the per-pose bytes
or the cut; partial bricks; a camera of odd sides; past 8192 bricks, the span of 128 packets that
the hashed pass A is planned with (its table size is not in dmf_fuse_plan_info, so neither that
case nor the a_hash knob's pins it).
"""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE = json.load(open(os.path.join(GOLDEN, "fuse_plan_parent.json")))
CASE_KEYS = ("grid", "camera", "P", "variant", "pipelined", "knobs", "budget")


def _gen():
    spec = importlib.util.spec_from_file_location("gen_fuse_plan", os.path.join(GOLDEN, "gen_fuse_plan.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_fixture_covers_the_generator_cases():
    """The fixture holds every case the generator defines, as it defines them; only the starved
    budgets recorded an error."""
    cases = _gen().cases()
    assert sorted(cases) == sorted(FIXTURE["cases"])
    for name, rec in FIXTURE["cases"].items():
        assert {k: rec[k] for k in CASE_KEYS} == cases[name], name
        assert len(rec["plan"]) == 8
        if not name.endswith("256k"):
            assert (rec["reserve_status"], rec["plan_status"]) == (0, 0), name


@pytest.mark.parametrize("name", sorted(FIXTURE["cases"]))
def test_plan_equals_parent(name):
    rec = FIXTURE["cases"][name]
    rs, ps, plan = _gen().run_case({k: rec[k] for k in CASE_KEYS})
    print(name, rs, ps, plan)
    assert (rs, ps) == (rec["reserve_status"], rec["plan_status"])
    assert plan == rec["plan"]
