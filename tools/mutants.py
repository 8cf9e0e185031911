#!/usr/bin/env python3
"""The mutation audit: do the GPU tests notice a kernel that is subtly wrong?  (profiles/mutants/README.md)

    python tools/mutants.py check                       # every patch applies and touches the file it names (no build)
    python tools/mutants.py build [ids...]              # no GPU needed: stereomatching_amd/mutants/<id>.so
    python tools/mutants.py run [ids...] --out profiles/mutants/results.json      # on the GPU, one process at a time

tests/mutants/manifest.json lists the mutants, tests/mutants/<id>.patch is each one's change to
stereomatching_amd/csrc/.  A mutant changes a stored or compared VALUE only; one whose value can reach an address has
`run: false` and is never run.  Nothing built here is committed, and neither csrc/ nor the product library is touched:
a mutant is compiled from a patched COPY of the sources and reaches the tests through SM_HIP_LIB (capi.py).
"""
from __future__ import annotations

import argparse
import concurrent.futures as cf
import json
import os
import re
import shutil
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from stereomatching_amd import build as B          # noqa: E402

MUTDIR = ROOT / "tests" / "mutants"
MANIFEST = MUTDIR / "manifest.json"
LIBDIR = B.PKG / "mutants"
SCRATCH = B.OBJDIR / "mutants"
CSRC_REL = "stereomatching_amd/csrc/"
FIELDS = ("id", "file", "kernel", "what", "reach", "run", "groups", "predicted")
MIN_LIMIT = 60                                      # seconds: the least time limit of a child
# an exit status other than 0 (survived) and 1 (killed), or this text, ends the whole run
FAULT_TEXT = "illegal memory access"


def manifest() -> list[dict]:
    return json.loads(MANIFEST.read_text())["mutants"]


def chosen(ids) -> list[dict]:
    ms = manifest()
    if ids:
        known = {m["id"] for m in ms}
        unknown = [i for i in ids if i not in known]
        if unknown:
            sys.exit(f"no such mutant: {', '.join(unknown)}")
        ms = [m for m in ms if m["id"] in ids]
    return ms


def group_key(files) -> str:
    return " ".join(files)


# ---------------------------------------------------------------------------
# patches
# ---------------------------------------------------------------------------

def patch_files(text: str) -> list[str]:
    """the files a unified diff changes (its +++ lines, without the b/ prefix)"""
    return [re.sub(r"^b/", "", m.group(1)) for m in re.finditer(r"^\+\+\+ (\S+)", text, re.M)]


def apply_patch(text: str, source: str, name: str) -> str:
    """`source` with the unified diff `text` applied.  Every hunk must match its line numbers and every context and
    removed line exactly: a patch that would need fuzz or an offset fails."""
    lines = source.splitlines(True)
    out, at = [], 0
    hunks = list(re.finditer(r"^@@ -(\d+)(?:,(\d+))? \+(\d+)(?:,(\d+))? @@.*\n((?:[ +\-\\].*\n?)*)", text, re.M))
    if not hunks:
        raise ValueError(f"{name}: no hunk")
    for h in hunks:
        start = int(h.group(1)) - 1
        if start < at:
            raise ValueError(f"{name}: hunks overlap")
        out += lines[at:start]
        at = start
        for ln in h.group(5).splitlines(True):
            tag, body = ln[0], ln[1:]
            if tag == "\\":
                continue
            if tag in " -":
                if at >= len(lines) or lines[at] != body:
                    raise ValueError(f"{name}: line {at + 1} of the source is not what the patch expects")
                if tag == " ":
                    out.append(body)
                at += 1
            else:
                out.append(body)
    return "".join(out + lines[at:])


def check_patch(m: dict) -> str:
    """the mutated text of m's file; raises where the patch does not fit the current tree"""
    text = (MUTDIR / f"{m['id']}.patch").read_text()
    files = patch_files(text)
    if files != [CSRC_REL + m["file"]]:
        raise ValueError(f"{m['id']}: the patch touches {files}, the manifest names {CSRC_REL + m['file']}")
    source = (B.CSRC / m["file"]).read_text()
    mutated = apply_patch(text, source, m["id"])
    if mutated == source:
        raise ValueError(f"{m['id']}: the patch changes nothing")
    return mutated


# ---------------------------------------------------------------------------
# build
# ---------------------------------------------------------------------------

def includes(path: Path) -> set[str]:
    return set(re.findall(r'^\s*#\s*include\s+"([^"]+)"', path.read_text(), re.M))


def units_of(changed: str) -> list[str]:
    """the translation units that include `changed` (a file of csrc/), directly or through headers"""
    reach: dict[str, set[str]] = {}

    def closure(name: str) -> set[str]:
        if name not in reach:
            reach[name] = set()
            for inc in includes(B.CSRC / name):
                if (B.CSRC / inc).exists():
                    reach[name] |= {inc} | closure(inc)
        return reach[name]
    return [s for s in B.SOURCES if s == changed or changed in closure(s)]


def build_one(m: dict, jobs: int) -> Path:
    mutated = check_patch(m)
    work = SCRATCH / m["id"]
    if work.exists():
        shutil.rmtree(work)
    try:
        return build_in(m, mutated, work, jobs)
    finally:
        # no copy of the sources stays inside the package (tests walk it), whether the build went through or not
        shutil.rmtree(work, ignore_errors=True)


def build_in(m: dict, mutated: str, work: Path, jobs: int) -> Path:
    shutil.copytree(B.CSRC, work / "csrc")
    shutil.copytree(B.ROOT / "include", work / "include")
    (work / "csrc" / m["file"]).write_text(mutated)
    units = units_of(m["file"])
    if not units:
        raise RuntimeError(f"{m['id']}: no translation unit includes {m['file']}")

    def one(src: str) -> Path:
        obj = work / (Path(src).stem + ".o")
        subprocess.check_call([B._hipcc(), *B.HIPCC_FLAGS, f"-I{work / 'include'}", f"-I{work / 'csrc'}", "-c",
                               str(work / "csrc" / src), "-o", str(obj)])
        return obj
    with cf.ThreadPoolExecutor(max_workers=max(1, jobs)) as ex:
        own = {Path(o).name: o for o in ex.map(one, units)}
    objs = [own.get(Path(s).stem + ".o", B.OBJDIR / "product" / (Path(s).stem + ".o")) for s in B.SOURCES]
    missing = [str(o) for o in objs if not Path(o).exists()]
    if missing:
        raise RuntimeError(f"{m['id']}: product objects missing: {missing}")
    LIBDIR.mkdir(exist_ok=True)
    out = LIBDIR / f"{m['id']}.so"
    subprocess.check_call([B._hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", *map(str, objs), "-o", str(out)])
    return out


def cmd_build(ids) -> None:
    B.build_hip()                                   # the product library and obj/product/*.o, if stale
    product = B.OBJDIR / "product"
    if any(not (product / (Path(s).stem + ".o")).exists() for s in B.SOURCES):
        B.build_hip(force=True)                     # the library came without its objects
    ms = chosen(ids)
    total = B._jobs()                               # at most 16 compilers side by side
    side = max(1, min(len(ms), total))
    with cf.ThreadPoolExecutor(max_workers=side) as ex:
        for m, out in zip(ms, ex.map(lambda m: build_one(m, max(1, total // side)), ms)):
            print(f"{m['id']:10s} {out.relative_to(ROOT)}", flush=True)


# ---------------------------------------------------------------------------
# run
# ---------------------------------------------------------------------------

def first_failure(output: str) -> str | None:
    m = re.search(r"^(?:FAILED|ERROR) (.+?)(?: - .*)?$", output, re.M)       # (a parametrised id may hold spaces)
    return m.group(1) if m else None


def child(files, limit: int, lib: Path | None) -> tuple[int, str, float]:
    """one fresh pytest process over `files`, under `timeout -k 10 limit`; SM_HIP_LIB names `lib` (None: unset)"""
    env = dict(os.environ)
    env.pop("SM_HIP_LIB", None)
    if lib is not None:
        env["SM_HIP_LIB"] = str(lib)
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", *files]
    t0 = time.monotonic()
    p = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    return p.returncode, p.stdout, time.monotonic() - t0


def cmd_run(ids, out_path: Path, baseline_limit: int) -> int:
    ms = [m for m in chosen(ids) if m["run"]]
    for m in ms:
        if not (LIBDIR / f"{m['id']}.so").exists():
            sys.exit(f"{m['id']}: {LIBDIR / (m['id'] + '.so')} is missing: run `build` first")
    results = json.loads(out_path.read_text()) if ids and out_path.exists() else {}
    results.setdefault("command", "python tools/mutants.py build && python tools/mutants.py run "
                                  "--out profiles/mutants/results.json   (a run of named ids replaces their entries)")
    results.setdefault("unmodified", {})
    results.setdefault("mutants", {})
    results.pop("stopped", None)
    out_path.parent.mkdir(parents=True, exist_ok=True)

    def save() -> None:
        out_path.write_text(json.dumps(results, indent=1) + "\n")

    def stop(what: str, rc: int, output: str, pending) -> int:
        results["stopped"] = {"at": what, "exit": rc, "tail": output[-2000:]}
        for mid, name in pending:
            results["mutants"].setdefault(mid, {}).setdefault(name, {"verdict": "not run"})
        save()
        print(f"STOPPED at {what}: exit {rc}\n{output[-2000:]}", flush=True)
        return 2

    groups = {}
    for m in ms:
        for name, files in m["groups"].items():
            groups.setdefault(group_key(files), files)
    todo = [(m["id"], name) for m in ms for name in m["groups"]]
    for m in ms:
        results["mutants"][m["id"]] = {}

    # 1. every group once against the unmodified library
    for key, files in groups.items():
        rc, output, secs = child(files, baseline_limit, None)
        print(f"unmodified  {key}: exit {rc}, {secs:.1f} s", flush=True)
        if rc != 0 or FAULT_TEXT in output:
            return stop(f"unmodified {key}", rc, output, todo)
        results["unmodified"][key] = {"verdict": "passed", "seconds": round(secs, 1),
                                      "limit": max(MIN_LIMIT, int(2 * secs + 1))}
        save()

    # 2. every mutant against each of its groups
    for m in ms:
        for name, files in m["groups"].items():
            key = group_key(files)
            limit = results["unmodified"][key]["limit"]
            rc, output, secs = child(files, limit, LIBDIR / f"{m['id']}.so")
            todo.remove((m["id"], name))
            if rc not in (0, 1) or FAULT_TEXT in output:
                results["mutants"][m["id"]][name] = {"verdict": "stopped the run", "exit": rc}
                return stop(f"{m['id']} {name}", rc, output, todo)
            entry = {"verdict": "survived" if rc == 0 else "killed", "seconds": round(secs, 1), "limit": limit,
                     "files": key}
            if rc == 1:
                entry["first_failure"] = first_failure(output)
            results["mutants"][m["id"]][name] = entry
            print(f"{m['id']:10s} {name:4s} {entry['verdict']:9s} {secs:6.1f} s  {entry.get('first_failure') or ''}",
                  flush=True)
            save()
    save()
    return 0


def cmd_check() -> None:
    for m in manifest():
        check_patch(m)
    print(len(manifest()), "patches apply")


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    sub = ap.add_subparsers(dest="cmd", required=True)
    sub.add_parser("check")
    b = sub.add_parser("build")
    b.add_argument("ids", nargs="*")
    r = sub.add_parser("run")
    r.add_argument("ids", nargs="*")
    r.add_argument("--out", type=Path, default=ROOT / "profiles" / "mutants" / "results.json")
    r.add_argument("--baseline-limit", type=int, default=600,
                   help="time limit in seconds of a group's run against the unmodified library")
    a = ap.parse_args()
    if a.cmd == "check":
        cmd_check()
    elif a.cmd == "build":
        cmd_build(a.ids)
    else:
        return cmd_run(a.ids, a.out if a.out.is_absolute() else ROOT / a.out, a.baseline_limit)
    return 0


if __name__ == "__main__":
    sys.exit(main())
