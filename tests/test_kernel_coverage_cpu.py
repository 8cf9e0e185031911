"""Is every kernel that the library ships launched by a GPU test?

tools/kernel_inventory.py lists the kernels of the built libstereo_hip.so from its symbol tables;
tests/golden/kernel_dispatches_mi355x.json.gz records, from kernel traces of the GPU test files on an MI355X
(tools/record_dispatches.py), which test file launched which kernel; tests/golden/kernel_waivers.json names the kernels
that no accepted plan can select.  The three have to agree: a new instantiation needs a test that launches it (and a
fresh trace of that test file merged into the record), a removed one leaves the record."""
import json
import math
import subprocess
from pathlib import Path

import numpy as np
import pytest

from stereomatching_amd import build
from tools import kernel_inventory as ki
from tools import record_dispatches as rd

ROOT = Path(__file__).resolve().parent.parent
ADMISSIBLE = "no plan selects it"


def test_normalise_reads_both_spellings():
    want = "k_census_wta<2, true, false>"
    # the demangler's: the kernel descriptor's symbol, with and without the suffix llvm-cxxfilt gives it
    assert ki.normalise("void k_census_wta<2, true, false>(unsigned long const*, int*, int*, CensusGeom) [clone .kd]") == want
    assert ki.normalise("void k_census_wta<2, true, false>(unsigned long const*, int*, int*, CensusGeom)") == want
    # the profiler's: a CSV field, quoted, sometimes with the descriptor's suffix left on
    assert ki.normalise('"void k_census_wta<2, true, false>(unsigned long const*, int*, int*, CensusGeom)"') == want
    assert ki.normalise("k_census_wta<2, true, false>(unsigned long const*, int*, int*, CensusGeom).kd") == want
    assert ki.normalise("void k_census_wta<2,true,false>(unsigned long const*, int*)") == want
    # no template arguments, no parameters, a kernel that is not void-prefixed
    assert ki.normalise("k_edge_thresholds(double, unsigned int*, int*)") == "k_edge_thresholds"
    assert ki.normalise("k_edge_thresholds.kd") == "k_edge_thresholds"
    # a cast among the template arguments is not the parameter list; nested templates keep their brackets
    assert ki.normalise("void k_x<(Cost)1, 4>(int)") == "k_x<(Cost)1, 4>"
    assert ki.normalise("void k_reproject<short, 4>(short const*, RpjQ, float, float) [clone .kd]") == "k_reproject<short, 4>"
    assert ki.normalise("void k_y<Pair<int, 2>, true>(Pair<int, 2> const*)") == "k_y<Pair<int, 2>, true>"
    assert ki.family("k_census_wta<2, true, false>") == "k_census_wta" and ki.family("k_edge_table") == "k_edge_table"


def test_merge_replaces_the_entries_of_the_files_it_is_given():
    known = {"k_a", "k_b<1>", "k_c"}
    rec = {"head": "x", "kernels": {"k_a": ["tests/t1.py", "tests/t2.py"], "k_b<1>": ["tests/t1.py"], "k_gone": ["tests/t2.py"]}}
    got = rd.merge(rec, {"tests/t1.py": {"k_c", "k_a", "torch_kernel"}}, known, "y")
    assert got == {"head": "y", "kernels": {"k_a": ["tests/t1.py", "tests/t2.py"], "k_c": ["tests/t1.py"]}}
    assert rd.missing(got, known) == ["k_b<1>"] and rd.missing(got, known, {"k_b<1>": ADMISSIBLE}) == []


@pytest.fixture(scope="module")
def inventory():
    return set(ki.inventory(build.LIB))


@pytest.fixture(scope="module")
def record():
    return rd.load()["kernels"]


@pytest.fixture(scope="module")
def waivers():
    return json.loads(rd.WAIVERS.read_text())


def test_every_compiled_kernel_has_a_launching_test_or_a_waiver(inventory, record, waivers):
    assert len(inventory) > 500, "the inventory of the built library looks empty"
    untested = sorted(inventory - set(record) - set(waivers))
    assert not untested, (f"{len(untested)} compiled kernels that no GPU test file is recorded to launch (add a test that "
                          f"selects them, trace it and merge the trace: tools/record_dispatches.py)", untested[:20])


def test_the_record_and_the_waivers_name_only_compiled_kernels(inventory, record, waivers):
    gone = sorted((set(record) | set(waivers)) - inventory)
    assert not gone, ("entries for kernels that the library no longer holds", gone[:20])


def test_every_recorded_kernel_names_a_gpu_test_file(record):
    files = {t for tests in record.values() for t in tests}
    assert all(tests for tests in record.values())
    for t in sorted(files):
        path = ROOT / t
        assert t.startswith("tests/") and path.is_file(), t
        assert "pytest.mark.gpu" in path.read_text(), f"{t} has no gpu-marked test"


def test_waivers_are_of_the_one_admissible_kind(inventory, record, waivers):
    for name, reason in waivers.items():
        assert name in inventory and name not in record, name
        assert reason.startswith(ADMISSIBLE + ":") and len(reason) > len(ADMISSIBLE) + 20, (name, reason)


# ---------------------------------------------------------------------------
# the searches that the waivers name
# ---------------------------------------------------------------------------

def test_strip_kernels_no_cost_launch_reaches(tmp_path, inventory, waivers):
    """plan_model_check strips: the cost planners over every window and shift count.  The strip kernels of two shifts a
    thread (more than 256 shifts) that it does not print -- SSD, whose matrix-core kernel stops at 256 shifts, and the SAD
    windows 17 .. 21, whose kernel stops at 240 -- are the waived ones, and the only ones"""
    from tests.test_plan_model_cpu import INCLUDES, SRC
    exe = tmp_path / "plan_model_check"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", *INCLUDES,
                           str(SRC), "-o", str(exe)])
    reached = set(subprocess.run([str(exe), "strips"], capture_output=True, text=True, check=True).stdout.split("\n")) - {""}
    built = {k for k in inventory if ki.family(k) == "k_cost_strip"}
    assert reached <= built and len(reached) > 20
    assert built - reached == {k for k in waivers if ki.family(k) == "k_cost_strip"}


def thresholds():
    rng = np.random.default_rng(766)
    fixed = [0.0, 5e-324, 2.3e-308, 1e-17, 2.0 ** -52, 1e-9, 1e-4, 0.01, 0.1, 0.15, 0.25, 1 / 3, 0.5, 2 / 3, 0.75, 0.9, 0.99,
             math.nextafter(1.0, 0.0), 1.0]
    return fixed + rng.random(24).tolist() + (10.0 ** -rng.uniform(0, 12, 12)).tolist()


def test_every_accepted_threshold_gives_tables_of_threshold_form(inventory, waivers):
    """The edge kernels without decision tables (TABLES = false) run only where k_edge_thresholds finds a row of the
    766 x 766 decision table that is not "true up to lo, false, true from hi on".  sm_check_threshold accepts 0 .. 1, and
    there a step of the right sum moves |ma - mb| by 1/768 and the limit by at most 1/1536: every row has the form.  The
    same test as the kernel's, on the reference's own table (oracle.edge_table), over the range's ends and 55 values in it."""
    from tests import oracle
    sa, sb = np.arange(766)[:, None], np.arange(766)[None, :]
    for t in thresholds():
        table = oracle.edge_table(t) != 0
        below, above = table & (sb <= sa), table & (sb >= sa)
        lo = np.where(below.any(axis=1), 765 - np.argmax(below[:, ::-1], axis=1), -1)
        hi = np.where(above.any(axis=1), np.argmax(above, axis=1), 766)
        assert np.array_equal(below.sum(axis=1), lo + 1) and np.array_equal(above.sum(axis=1), 766 - hi), t
    without = {k for k in inventory if ki.family(k) in ("k_edges_ext", "k_edges_ext4") and k.split(", ")[1].startswith("false")}
    assert without == {k for k in waivers if ki.family(k).startswith("k_edges_ext")} and len(without) == 6
