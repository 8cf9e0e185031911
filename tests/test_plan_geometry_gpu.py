"""What plans come out as on the real device, pinned to tests/golden/plan_geometry_mi355x.json.gz: every field of
plan.geometry(), plan.describe() and workspace_bytes() of the plans of tests/plan_geometry_cases.py, as
tools/record_plan_geometry.py recorded them at the commit the file names.  Planning code may be rearranged; what it
decides on this device may not change unnoticed."""
import gzip
import json
import time

import pytest

from tests import plan_geometry_cases as pc
from tests.conftest import GOLDEN_DIR

pytestmark = pytest.mark.gpu
GOLDEN = json.loads(gzip.decompress((GOLDEN_DIR / "plan_geometry_mi355x.json.gz").read_bytes()))


def test_case_list_is_the_recorded_one():
    keys = [pc.key(c) for c in pc.cases()]
    assert len(set(keys)) == len(keys)
    assert sorted(keys) == sorted(GOLDEN["plans"]), "the case list and the recorded file differ: record again at " \
        "the commit whose planning is the reference"
    assert 200 <= len(keys) <= 300


def test_plans_equal_the_recorded_geometry(hip):
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert cus == GOLDEN["compute_units"], \
        f"this device has {cus} compute units, the geometry was recorded on {GOLDEN['compute_units']}"
    t0 = time.perf_counter()
    differ = []
    for case in pc.cases():
        w, h, d, s, border, pairs, opt = case
        plan = hip.StereoPlan(w, h, d, s, border, max_pairs=pairs, options=opt or None)
        try:
            got = {"geometry": plan.geometry(), "describe": plan.describe(), "workspace_bytes": plan.workspace_bytes()}
        finally:
            plan.close()
        want = GOLDEN["plans"][pc.key(case)]
        for name in want["geometry"]:
            if got["geometry"].get(name) != want["geometry"][name]:
                differ.append(f"{pc.key(case)}: {name} = {got['geometry'].get(name)}, recorded {want['geometry'][name]}")
        assert sorted(got["geometry"]) == sorted(want["geometry"])
        for name in ("describe", "workspace_bytes"):
            if got[name] != want[name]:
                differ.append(f"{pc.key(case)}: {name} = {got[name]!r}, recorded {want[name]!r}")
    dt = time.perf_counter() - t0
    print(f"{len(pc.cases())} plans in {dt:.2f} s ({1e3 * dt / len(pc.cases()):.1f} ms a plan)")
    assert not differ, f"{len(differ)} differences from commit {GOLDEN['commit'][:12]}:\n" + "\n".join(differ[:20])
