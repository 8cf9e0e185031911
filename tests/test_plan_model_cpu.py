"""Launch planning on the CPU (csrc/sm_plan_model.h, plain C++17), built for the host with
tests/helpers/plan_model_check.cpp and run against the stand-in device of tests/helpers/plan_cases.h.

tests/golden/plan_model_parent.json.gz holds what the planners of the commit it names returned for the ~1500 match and
~1500 cost cases of plan_cases.h on that device, recorded from that commit's own functions (sm_match_configure with the
runtime's queries redirected, sm_sad_pc_configure, sm_sad_qs_configure, sm_ssd_mfma_configure): every field of the
geometry, the kernel, and the describe string (as a 32-bit hash).  The model must return the same, field for field.
The file is the reference: it is never written from the code under test.  (Compact JSON, stored gzipped: `zcat` reads it.)

A sweep of 20 000 further seeded shapes asserts what every consumer of a geometry relies on (LDS within the limit,
tiles that cover the image, staged words inside the packed image, lane counts, merge buffers inside the LDS request,
explicit options honoured or clamped), once more as a stand-alone binary under the address and undefined-behaviour
sanitizers."""
import gzip
import json
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "helpers" / "plan_model_check.cpp"
GOLDEN = ROOT / "tests" / "golden" / "plan_model_parent.json.gz"
INCLUDES = [f"-I{ROOT / 'stereomatching_amd' / 'csrc'}", f"-I{ROOT / 'include'}", f"-I{ROOT / 'tests' / 'helpers'}"]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("plan_model") / "plan_model_check"
    # (-ffp-contract=off: the cost models' doubles as the library's own build computes them)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", *INCLUDES,
                           str(SRC), "-o", str(exe)])
    return exe


def first_difference(names, want, got):
    if (want == 0) != (got == 0):
        return f"kernel: {'not built' if got == 0 else got[0]}, recorded {'not built' if want == 0 else want[0]}"
    if want == 0:
        return None
    assert len(names) == len(want) == len(got)
    # (the describe string last: it differs whenever a field it prints does, and the field says more)
    for name, w, g in sorted(zip(names, want, got), key=lambda t: t[0] == "describe"):
        if w != g:
            return f"{name} = {g}, recorded {w}"
    return None


def test_model_equals_the_recorded_planners(program):
    text = gzip.decompress(GOLDEN.read_bytes())
    want = json.loads(text)
    got = json.loads(subprocess.run([str(program), "dump"], capture_output=True, text=True, check=True).stdout)
    assert len(want["commit"]) == 40
    assert len(text) < 300 * 1024
    for key in ("match_fields", "cost_fields"):
        assert got[key] == want[key]
    assert len(got["match"]) == len(want["match"]) >= 1400
    assert len(got["cost"]) == len(want["cost"]) >= 1400

    def inputs(kind, i):
        return subprocess.run([str(program), "case", str(kind), str(i)], capture_output=True, text=True).stdout.strip()
    for i, (w, g) in enumerate(zip(want["match"], got["match"])):
        diff = first_difference(want["match_fields"], w, g)
        assert diff is None, f"match case {i} ({inputs(0, i)}): {diff}"
    for i, (w, g) in enumerate(zip(want["cost"], got["cost"])):
        assert len(w) == len(g) == 3
        for planner, wk, gk in zip(("sad_pc", "sad_qs", "ssd_mfma"), w, g):
            diff = first_difference(want["cost_fields"], wk, gk)
            assert diff is None, f"cost case {i} ({inputs(1, i)}), {planner}: {diff}"


def test_cases_reach_every_branch(program):
    """the stand-in device must take the recorded cases through the planner's branches, or equality proves little"""
    out = subprocess.run([str(program), "stats"], capture_output=True, text=True, check=True).stdout
    n = {k: int(v) for k, v in (kv.split("=") for kv in out.split())}
    print(out)
    for key in ("bit_sliced", "tiled", "generic", "multi_round", "two_wave_variant", "lds_pad", "two_wave_workgroups",
                "lane_merge_lds", "ds16", "ds8", "ds4"):
        assert n[key] >= 50, (key, n)
    want = json.loads(gzip.decompress(GOLDEN.read_bytes()))
    for planner in range(3):
        assert sum(1 for c in want["cost"] if c[planner] != 0) >= 150, planner


def test_property_sweep(program):
    p = subprocess.run([str(program), "sweep"], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-2000:]
    assert "cases=20000 failures=0" in p.stdout


def test_property_sweep_under_address_and_undefined_sanitizers(tmp_path):
    """the same program as a stand-alone host binary with -fsanitize=address,undefined"""
    exe = tmp_path / "plan_model_check_san"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-ffp-contract=off", *INCLUDES, str(SRC), "-o", str(exe)])
    p = subprocess.run([str(exe), "sweep"], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert "cases=20000 failures=0" in p.stdout
