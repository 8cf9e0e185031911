#!/usr/bin/env python3
"""Which GPU test file launches which kernel: merge kernel traces into
tests/golden/kernel_dispatches_mi355x.json.gz

    {"head": <commit>, "kernels": {normalised kernel name: [test files that launched it]}}

Only kernels of the library's inventory (tools/kernel_inventory.py) are kept, so the kernels of
torch and of the runtime drop out.  tests/test_kernel_coverage_cpu.py holds the record against the
built library: every compiled kernel has a launching test file here or a waiver.

Recipe (on an MI355X, one process per GPU test file, one after another, each under its own time
limit, the chain ending at the first fault, abort or time-out; no counters and no other tracing):

    for f in tests/test_*_gpu.py; do
        n=$(basename $f .py)
        timeout -k 10 600 rocprofv3 --kernel-trace --output-format csv -d $PWD/traces/$n -- \\
            python -m pytest -m gpu $f -q -p no:cacheprovider > $PWD/traces/$n.log 2>&1
        rc=$?; [ $rc -le 1 ] || exit $rc
        python tools/record_dispatches.py names traces/$n > names/$n.txt && rm -r traces/$n
    done
    python tools/record_dispatches.py merge names/*.txt

`names` reduces a trace directory (every *kernel_trace.csv below it, the children of the test
process included) to the sorted set of normalised kernel names, so that only a few kilobytes per
test file have to be kept.  The trace directory is absolute because the programs that
tests/test_cli_gpu.py starts are traced too and run elsewhere; that file takes minutes under the
tracer (every child loads it), and its one test that reads a child's stderr fails there, on the
tracer's own lines: the kernels are recorded all the same, and a failed test does not end the job.  `merge` takes name lists, trace CSVs or trace directories, each as
FILE or as tests/test_x_gpu.py=FILE (without the prefix the test file is tests/<stem of FILE>.py),
and REPLACES the entries of the test files it is given; entries of other test files stay.  A test
file killed at its limit only because tracing slows it gets a longer limit or is split with -k; it
is not retried in a loop.  A stage added later keeps the
traces of its own GPU test files in a record of its own beside the first one, tests/golden/
kernel_dispatches_mi355x.<stage>.json.gz (`merge --record THAT_FILE tests/test_<stage>_gpu.py=FILE`): load() adds
every such supplement to the record it returns, so the coverage test sees them, and the first record's bytes change
only when the test files recorded in it are traced again.  `missing` prints the inventory's kernels that no test file launches,
by family (profiles/coverage/never_launched.txt is its output at the commit named there).
"""
from __future__ import annotations

import csv
import gzip
import json
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from tools.kernel_inventory import by_family, inventory, normalise     # noqa: E402

RECORD = ROOT / "tests" / "golden" / "kernel_dispatches_mi355x.json.gz"
WAIVERS = ROOT / "tests" / "golden" / "kernel_waivers.json"


def names_of(path: Path) -> set[str]:
    """normalised kernel names of a name list, a kernel-trace CSV or a directory of them"""
    path = Path(path)
    if path.is_dir():
        files = sorted(path.rglob("*kernel_trace.csv"))
        if not files:
            raise FileNotFoundError(f"{path}: no *kernel_trace.csv below it")
        return set().union(*(names_of(f) for f in files))
    if path.suffix == ".csv":
        csv.field_size_limit(1 << 24)
        with open(path, newline="") as f:
            return {normalise(r["Kernel_Name"]) for r in csv.DictReader(f)}
    return {normalise(line) for line in path.read_text().splitlines() if line.strip()}


def supplements(path: Path = RECORD) -> list[Path]:
    """the records beside `path` that add to it: kernel_dispatches_mi355x.<stage>.json.gz for ...mi355x.json.gz"""
    stem = path.name[:-len(".json.gz")]
    return sorted(p for p in path.parent.glob(stem + ".*.json.gz") if p != path)


def _load_one(path: Path) -> dict:
    if not path.exists():
        return {"head": "", "kernels": {}}
    with gzip.open(path, "rt") as f:
        return json.load(f)


def load(path: Path = RECORD, with_supplements: bool = True) -> dict:
    """the record at `path`, by default with the test files of its supplements added to each kernel's list"""
    rec = _load_one(path)
    if with_supplements:
        for extra in supplements(path):
            for k, tests in _load_one(extra)["kernels"].items():
                rec["kernels"][k] = sorted(set(rec["kernels"].get(k, [])) | set(tests))
    return rec


def save(rec: dict, path: Path = RECORD) -> None:
    text = json.dumps(rec, indent=0, sort_keys=True) + "\n"
    with open(path, "wb") as raw, gzip.GzipFile(fileobj=raw, mode="wb", mtime=0, filename="") as f:
        f.write(text.encode())         # (mtime 0: the same record gives the same bytes)


def merge(rec: dict, traced: dict[str, set[str]], known: set[str], head: str) -> dict:
    """`traced`: test file -> kernel names it launched; the entries of those files are replaced"""
    kernels = {k: [t for t in v if t not in traced] for k, v in rec["kernels"].items() if k in known}
    for test, names in traced.items():
        for k in names & known:
            kernels.setdefault(k, []).append(test)
    return {"head": head, "kernels": {k: sorted(set(v)) for k, v in sorted(kernels.items()) if v}}


def missing(rec: dict, known: set[str], waived=()) -> list[str]:
    return sorted(known - set(rec["kernels"]) - set(waived))


def report(names: list[str], known: set[str], head: str) -> str:
    fam_all, fam = by_family(known), by_family(names)
    out = [f"# kernels of libstereo_hip.so that no GPU test file launches, at {head}",
           f"# {len(names)} of {len(known)} kernels, in {len(fam)} of {len(fam_all)} families", ""]
    for f, ks in sorted(fam.items(), key=lambda kv: (-len(kv[1]), kv[0])):
        out.append(f"{f}: {len(ks)} of {len(fam_all[f])}")
        out += [f"    {k}" for k in ks]
    return "\n".join(out) + "\n"


def _head() -> str:
    try:
        return subprocess.check_output(["git", "-C", str(ROOT), "describe", "--always", "--dirty", "--abbrev=12"],
                                       text=True, stderr=subprocess.DEVNULL).strip()
    except (OSError, subprocess.CalledProcessError):
        return "unknown"


def main(argv) -> int:
    if len(argv) < 1 or argv[0] not in ("names", "merge", "missing"):
        print(__doc__)
        return 2
    cmd, args = argv[0], argv[1:]
    opts = {}
    while args and args[0].startswith("--"):
        opts[args[0]] = args[1]
        args = args[2:]
    if cmd == "names":
        print("\n".join(sorted(set().union(*(names_of(Path(a)) for a in args)))))
        return 0
    known = set(inventory(Path(opts["--lib"]) if "--lib" in opts else None))
    record = Path(opts.get("--record", RECORD))
    # merge rewrites one file: what its supplements hold stays in them
    rec = load(record, with_supplements=cmd != "merge")
    if cmd == "merge":
        traced = {}
        for a in args:
            test, _, path = a.rpartition("=")
            test = test or f"tests/{Path(path).stem}.py"
            if not (ROOT / test).exists():
                raise FileNotFoundError(f"{test}: no such test file")
            traced.setdefault(test, set()).update(names_of(Path(path)))
        rec = merge(rec, traced, known, opts.get("--head", _head()))
        save(rec, record)
        print(f"{record}: {len(rec['kernels'])} of {len(known)} kernels launched by "
              f"{len({t for v in rec['kernels'].values() for t in v})} test files")
        return 0
    waived = json.loads(WAIVERS.read_text()) if WAIVERS.exists() else {}
    print(report(missing(rec, known, waived), known, rec["head"]), end="")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
