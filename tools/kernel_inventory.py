#!/usr/bin/env python3
"""Print the GPU kernels that libstereo_hip.so holds, one normalised name per line, sorted.

    python tools/kernel_inventory.py [path/to/libstereo_hip.so]

The device code objects are taken out of the library with `llvm-objdump --offloading`
(into a temporary directory), their `*.kd` kernel-descriptor symbols are read with
`llvm-readelf --symbols --wide` and demangled with llvm-cxxfilt or c++filt.  Only symbol
tables are read: nothing is disassembled.

normalise() is the one place that turns a demangled or a profiler-reported kernel name into
the name used by the inventory, by tools/record_dispatches.py and by
tests/test_kernel_coverage_cpu.py:  `k_census_wta<2, true, false>`.
"""
from __future__ import annotations

import os
import re
import shutil
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
LLVM_DIRS = ("/opt/rocm/llvm/bin", "/opt/rocm/lib/llvm/bin")


def normalise(name: str) -> str:
    """`void k_x<1, (Cost)1>(int const*, Geom) [clone .kd]` -> `k_x<1, (Cost)1>`.

    Drops a leading `void `, a trailing `.kd`, any `[clone ...]` suffix and the parameter
    list; keeps the template arguments.  The parameter list starts at the first `(` outside
    every `<...>`, so a cast such as `(Cost)1` among the template arguments stays."""
    s = name.strip().strip('"').strip()
    s = re.sub(r"\s*\[clone [^\]]*\]", "", s).strip()
    if s.endswith(".kd"):
        s = s[:-3]
    if s.startswith("void "):
        s = s[5:]
    depth = 0
    for i, c in enumerate(s):
        if c == "<":
            depth += 1
        elif c == ">":
            depth -= 1
        elif c == "(" and depth == 0:
            s = s[:i]
            break
    s = re.sub(r"\s*,\s*", ", ", s.strip())
    return re.sub(r"<\s+|\s+>", lambda m: m.group(0).strip(), s)


def family(name: str) -> str:
    """`k_census_wta<2, true, false>` -> `k_census_wta`"""
    return name.split("<", 1)[0]


def _tool(*names: str) -> str:
    for n in names:
        p = shutil.which(n)
        if p:
            return p
        for d in LLVM_DIRS:
            if (Path(d) / n).exists():
                return str(Path(d) / n)
    raise RuntimeError(f"none of {', '.join(names)} found on PATH or under {', '.join(LLVM_DIRS)}")


def kernel_symbols(lib: Path) -> list[str]:
    """The mangled names of every kernel descriptor (`<kernel>.kd`) in the library's code objects."""
    objdump, readelf = _tool("llvm-objdump"), _tool("llvm-readelf")
    names = set()
    with tempfile.TemporaryDirectory(prefix="kernel_inventory_") as tmp:
        # llvm-objdump writes <input file name>.<index>.<triple> next to the current directory
        local = Path(tmp) / lib.name
        os.symlink(lib.resolve(), local)
        subprocess.check_call([objdump, "--offloading", local.name], cwd=tmp, stdout=subprocess.DEVNULL)
        objs = [p for p in Path(tmp).iterdir() if p != local and p.is_file()]
        if not objs:
            raise RuntimeError(f"llvm-objdump --offloading found no device code object in {lib}")
        for obj in objs:
            if obj.read_bytes()[:4] != b"\x7fELF":      # the host entry of a fat binary is empty
                continue
            out = subprocess.check_output([readelf, "--symbols", "--wide", str(obj)], text=True)
            for line in out.splitlines():
                f = line.split()
                if len(f) >= 8 and f[3] == "OBJECT" and f[7].endswith(".kd"):
                    names.add(f[7][:-3])
    return sorted(names)


def demangle(names: list[str]) -> list[str]:
    if not names:
        return []
    out = subprocess.run([_tool("llvm-cxxfilt", "c++filt")], input="\n".join(names) + "\n",
                         text=True, capture_output=True, check=True).stdout
    res = out.splitlines()
    assert len(res) == len(names), "the demangler dropped or added lines"
    return res


def inventory(lib: Path | None = None) -> list[str]:
    """Sorted normalised names of every kernel in `lib` (default: the built library)."""
    if lib is None:
        sys.path.insert(0, str(ROOT))
        from stereomatching_amd import build
        lib = build.LIB
    lib = Path(lib)
    if not lib.exists():
        raise FileNotFoundError(f"{lib}: build the library first (python -m stereomatching_amd.build)")
    return sorted({normalise(n) for n in demangle(kernel_symbols(lib))})


def by_family(names) -> dict[str, list[str]]:
    fam: dict[str, list[str]] = {}
    for n in sorted(names):
        fam.setdefault(family(n), []).append(n)
    return fam


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("-")]
    names = inventory(Path(args[0]) if args else None)
    if "--families" in sys.argv:
        for f, ks in sorted(by_family(names).items(), key=lambda kv: (-len(kv[1]), kv[0])):
            print(f"{len(ks):4d}  {f}")
        print(f"{len(names):4d}  kernels in {len(by_family(names))} families")
    else:
        print("\n".join(names))
