"""The mutation audit's data stays usable (tools/mutants.py, profiles/mutants/README.md): every mutant of
tests/mutants/manifest.json is complete, its patch still fits the sources and touches the one file it names, its groups
are GPU test files, and the recorded run (profiles/mutants/results.json) has a verdict for exactly the mutants that may
run, with every survivor accounted for in the record.  Nothing is built here."""
import json
import re
from pathlib import Path

import pytest

from tools import mutants as mt

ROOT = Path(__file__).resolve().parent.parent
RESULTS = ROOT / "profiles" / "mutants" / "results.json"
README = ROOT / "profiles" / "mutants" / "README.md"
MANIFEST = mt.manifest()
IDS = [m["id"] for m in MANIFEST]
VERDICTS = ("killed", "survived")
# the nine mutants of the two earlier records, and the least the newest kernels get
RECORDED = {"census_a", "census_b", "census_b2", "census_c", "poison_a", "poison_b", "poison_c", "poison_d", "poison_e"}
NEWEST = {"B1", "B2", "B3", "B4", "N1", "N2", "N3", "N4", "C1", "C2", "U1", "U2", "U3", "U4", "W1", "W2"}
# the second audit: the stages around the matchers (smoother, interpolation, post-filters, pyramid, rectification,
# subpixel refinement), each against its unit's own GPU module
AROUND = ({f"G{i}" for i in range(1, 9)} | {f"I{i}" for i in range(1, 7)} | {f"F{i}" for i in range(1, 7)}
          | {f"P{i}" for i in range(1, 8)} | {f"R{i}" for i in range(1, 8)} | {f"X{i}" for i in range(1, 6)})
AROUND_OWN = {"G": "tests/test_wls_gpu.py", "I": "tests/test_interp_gpu.py", "F": "tests/test_filter_gpu.py",
              "P": "tests/test_pyramid_gpu.py", "R": "tests/test_rectify_gpu.py", "X": "tests/test_subpix_gpu.py"}
# the two newer mutants with a second group: the row scan's carry needs more than 64 chunks, which only the module of
# the loops' second turns has; and C1 mutates the one text of two kernels (sm_near_tile_body.h), each with its module
SECOND_GROUP = {"I2": {"turns": ["tests/test_second_turns_gpu.py"]}, "C1": {"near": ["tests/test_near_gpu.py"]}}
# the third audit: the matchers of the cost modes (general / strip, prefix-chain, quad-SAD, matrix-core), census, SGM, the
# left-right check, the reprojection and step 3 -- the least each unit gets, and the GPU files its groups may name.  A
# group of these is a list of pytest node ids (single tests of a long module), which tools/mutants.py passes on as they are
MATCHERS = ({f"K{i}" for i in range(1, 11)} | {f"S{i}" for i in range(1, 9)} | {f"Q{i}" for i in range(1, 5)}
            | {f"M{i}" for i in range(1, 11)} | {f"T{i}" for i in range(1, 11)} | {f"H{i}" for i in range(1, 11)}
            | {f"L{i}" for i in range(1, 9)} | {f"J{i}" for i in range(1, 11)} | {f"Z{i}" for i in range(1, 7)})
COST_FILES = {"tests/test_extremes_gpu.py", "tests/test_hip_gpu.py"}
MATCHERS_FILES = {"K": COST_FILES, "S": COST_FILES, "Q": COST_FILES, "M": COST_FILES,
                  "T": {"tests/test_census_gpu.py", "tests/test_census_extremes_gpu.py"},
                  "H": {"tests/test_sgm_gpu.py", "tests/test_census_extremes_gpu.py"},
                  "L": {"tests/test_lr_gpu.py", "tests/test_lr_sweep_gpu.py", "tests/test_cost_lr_gpu.py"},
                  "J": {"tests/test_reproject_gpu.py"}, "Z": {"tests/test_step3_gpu.py", "tests/test_hip_gpu.py"}}
# the fourth audit: the cross-based matcher (sm_cross.hip) -- the least each of its three kernels gets (A: k_cross_arms,
# E: k_cross_wta, Y: k_cross_refine), and the GPU files its groups may name, as whole modules or as node ids
CROSS = {f"A{i}" for i in range(1, 8)} | {f"E{i}" for i in range(1, 15)} | {f"Y{i}" for i in range(1, 6)}
CROSS_KERNEL = {"A": "k_cross_arms", "E": "k_cross_wta", "Y": "k_cross_refine"}
CROSS_FILES = {"tests/test_cross_gpu.py", "tests/test_cross_shapes_gpu.py"}
# full-size tests no group may name (and so no group may name their whole module)
TOO_LONG = {"tests/test_hip_gpu.py", "tests/test_extremes_gpu.py", "tests/test_step3_gpu.py"}


def third(m):
    return re.fullmatch(r"[KSQMTHLJZ]\d+", m["id"]) is not None


def fourth(m):
    return re.fullmatch(r"[AEY]\d+", m["id"]) is not None


@pytest.fixture(scope="module")
def results():
    return json.loads(RESULTS.read_text())


@pytest.fixture(scope="module")
def survivors_recorded():
    """{(id, group): (kind, test id or None)} of the README's lines `- ID (group): equivalent, because ...` and
    `- ID (group): closed by tests/file.py::test_name`"""
    out = {}
    for m in re.finditer(r"^- `?(\w+)`? \((\w+)\): (equivalent, because \S.*|closed by (tests/\S+?\.py)::(\w+).*)$",
                         README.read_text(), re.M):
        out[(m.group(1), m.group(2))] = ("closed", (m.group(4), m.group(5))) if m.group(4) else ("equivalent", None)
    return out


def test_the_manifest_names_each_mutant_once_and_the_ones_asked_for():
    assert len(IDS) == len(set(IDS))
    assert RECORDED | NEWEST | AROUND | MATCHERS | CROSS <= set(IDS)
    assert len(AROUND) == 39 and len(MATCHERS) == 76 and len(CROSS) == 26
    assert sum(1 for m in MANIFEST if third(m) and m["run"]) >= 60, "the third audit runs at least 60 mutants"
    assert sum(1 for m in MANIFEST if fourth(m)) >= 28, "the fourth audit has at least 28 mutants"
    assert sum(1 for m in MANIFEST if fourth(m) and m["run"]) >= 24, "the fourth audit runs at least 24 mutants"
    patches = {p.stem for p in mt.MUTDIR.glob("*.patch")}
    assert patches == set(IDS), "a patch without an entry, or an entry without a patch"


@pytest.mark.parametrize("m", MANIFEST, ids=IDS)
def test_every_entry_is_complete(m):
    for f in mt.FIELDS:
        assert f in m, f
    assert isinstance(m["run"], bool)
    assert re.match(r"(k|sm)_\w+", m["kernel"])
    for f in ("what", "reach"):
        assert isinstance(m[f], str) and len(m[f]) > 10, f
    assert "\n" not in m["what"], "one sentence"
    assert (mt.B.CSRC / m["file"]).is_file()
    assert m["groups"] and set(m["predicted"]) == set(m["groups"])
    for name, p in m["predicted"].items():
        assert p["verdict"] in VERDICTS, name
        assert p["test"] if p["verdict"] == "killed" else p.get("why"), name
    # the two earlier records keep their "new" and "old" groups; a newer mutant has one group, its unit's own modules
    # (and I2 the one second group named above)
    extra = SECOND_GROUP.get(m["id"], {})
    assert set(m["groups"]) == ({"new", "old"} if m["id"] in RECORDED else {"own"} | set(extra))
    for name, files in extra.items():
        assert m["groups"][name] == files
    if m["id"] in AROUND:
        assert m["groups"]["own"] == [AROUND_OWN[m["id"][0]]], "a mutant of the second audit runs against its unit's module"
    if third(m):
        files = {f.split("::")[0] for f in m["groups"]["own"]}
        assert files <= MATCHERS_FILES[m["id"][0]], "a mutant of the third audit runs against its unit's modules"
        for f in m["groups"]["own"]:
            assert "::" in f or f.split("::")[0] not in TOO_LONG, f"{f}: name single tests of this module"
            assert not f.endswith("test_cost_mode_4k_full_image_vs_own_oracle"), "the 4K test is no part of a group"
    if fourth(m):
        assert m["file"] == "sm_cross.hip" and m["kernel"] == CROSS_KERNEL[m["id"][0]]
        files = {f.split("::")[0] for f in m["groups"]["own"]}
        assert files and files <= CROSS_FILES, "a mutant of the fourth audit runs against the cross matcher's modules"


def test_a_value_that_can_reach_an_address_is_never_run():
    by_id = {m["id"]: m for m in MANIFEST}
    assert by_id["poison_c"]["run"] is False and by_id["poison_c"]["reach"].startswith("YES")
    for m in MANIFEST:
        assert m["run"] or re.match(r"YES|STOPPED", m["reach"]), m["id"]


@pytest.mark.parametrize("m", MANIFEST, ids=IDS)
def test_every_patch_fits_the_sources_and_touches_the_file_it_names(m):
    """(a refactoring that moves a mutated line fails here, not in the audit)"""
    text = (mt.MUTDIR / f"{m['id']}.patch").read_text()
    assert mt.patch_files(text) == [mt.CSRC_REL + m["file"]]
    assert re.findall(r"^--- (\S+)", text, re.M) == ["a/" + mt.CSRC_REL + m["file"]]
    source = (mt.B.CSRC / m["file"]).read_text()
    mutated = mt.check_patch(m)
    changed = sum(1 for ln in text.splitlines() if re.match(r"[+-](?![+-]{2} )", ln))
    assert mutated != source and 1 <= changed <= 12, "a mutant is a handful of lines"
    assert mt.units_of(m["file"]), "no translation unit would be rebuilt"


def test_the_patch_check_refuses_a_patch_that_does_not_fit():
    m = dict(MANIFEST[0])
    text = (mt.MUTDIR / f"{m['id']}.patch").read_text()
    source = (mt.B.CSRC / m["file"]).read_text()
    with pytest.raises(ValueError):
        mt.apply_patch(text, "// a line more\n" + source, "moved")
    with pytest.raises(ValueError):
        mt.apply_patch(text, source.replace("0x8000", "0x8001"), "edited")
    assert mt.apply_patch(text, source, "fits") != source


@pytest.mark.parametrize("m", MANIFEST, ids=IDS)
def test_every_group_is_gpu_test_files(m):
    for files in m["groups"].values():
        assert files
        for f in files:
            # a GPU test file, or one test of it as a pytest node id (third and fourth audit)
            name, _, test = f.partition("::")
            path = ROOT / name
            assert re.fullmatch(r"tests/test_\w+_gpu\.py", name) and path.is_file(), f
            assert re.search(r"^pytestmark = pytest\.mark\.gpu|^@pytest\.mark\.gpu", path.read_text(), re.M), f
            if "::" in f:
                assert (third(m) or fourth(m)) and re.fullmatch(r"test_\w+", test), f
                assert re.search(rf"^def {test}\(", path.read_text(), re.M), f"{f}: no such test"


def test_the_recorded_run_has_a_verdict_for_exactly_the_mutants_that_may_run(results):
    assert "stopped" not in results, "the recorded run was ended by a child"
    assert "tools/mutants.py" in results["command"]
    want = {m["id"] for m in MANIFEST if m["run"]}
    assert set(results["mutants"]) == want
    for m in MANIFEST:
        if not m["run"]:
            continue
        got = results["mutants"][m["id"]]
        assert set(got) == set(m["groups"]), m["id"]
        for name, files in m["groups"].items():
            key = mt.group_key(files)
            base = results["unmodified"][key]
            assert base["verdict"] == "passed" and base["limit"] >= max(mt.MIN_LIMIT, 2 * base["seconds"])
            v = got[name]
            assert v["verdict"] in VERDICTS and v["files"] == key, (m["id"], name)
            assert v["limit"] >= mt.MIN_LIMIT and v["seconds"] <= v["limit"]
            assert (v["verdict"] == "killed") == bool(v.get("first_failure")), (m["id"], name)


def test_every_survivor_is_equivalent_or_closed_in_the_record(results, survivors_recorded):
    by_id = {m["id"]: m for m in MANIFEST}
    for mid, groups in results["mutants"].items():
        alive = [g for g, v in groups.items() if v["verdict"] == "survived"]
        for g in alive:
            assert (mid, g) in survivors_recorded, f"{mid} survived {g}: the record names it neither equivalent nor closed"
            kind, test = survivors_recorded[(mid, g)]
            if kind == "closed":
                path = ROOT / test[0]
                assert path.is_file() and re.search(rf"^def {test[1]}\(", path.read_text(), re.M), test
                # what closes it killed it: another group of the same mutant holds that file and died
                assert any(v["verdict"] == "killed" and test[0] in by_id[mid]["groups"][h]
                           for h, v in groups.items()), (mid, g)
        if alive and len(alive) == len(groups):
            # killed by nothing: only an equivalent mutant may end so
            assert all(survivors_recorded[(mid, g)][0] == "equivalent" for g in alive), mid
