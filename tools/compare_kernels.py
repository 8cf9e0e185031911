#!/usr/bin/env python3
"""Compare the gfx950 kernels and the exported C symbols of two builds of libstereo_hip.so.

    python tools/compare_kernels.py [--allow-added] OLD.so NEW.so

--allow-added: for a change that adds kernels and entry points beside the existing ones: only OLD's symbols are compared
(what NEW has besides them is not a difference, and the counts of NEW in the summary line are of those symbols).
For a change that must not touch any kernel (a refactor, a new stage beside the existing ones).  Kernels are compared
per SYMBOL, not per file, so a kernel may move to another translation unit (another code object): every gfx950 code
object of each library is extracted from its .hip_fatbin section and disassembled, the listing is split at function
symbols, addresses / encodings / the padding after s_endpgm are stripped, and the text is compared.  The resource
use of every kernel (.vgpr_count, .sgpr_count, .group_segment_fixed_size, .private_segment_fixed_size,
.kernarg_segment_size of the code object's notes) and the unmangled sm_* symbols of the dynamic symbol table are
compared too.  Prints what differs; the exit status is 0 iff nothing does.  Needs no GPU: llvm-objdump, llvm-readelf
and llvm-objcopy of the ROCm tree ($ROCM_PATH, default /opt/rocm) do the work.
"""
from __future__ import annotations

import os
import re
import struct
import subprocess
import sys
import tempfile
from pathlib import Path

LLVM = Path(os.environ.get("ROCM_PATH", "/opt/rocm")) / "lib" / "llvm" / "bin"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
NOTES = (".vgpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size",
         ".kernarg_segment_size")


def tool(name: str, *args: str) -> str:
    return subprocess.run([str(LLVM / name), *args], check=True, capture_output=True, text=True).stdout


def code_objects(lib: Path, tmp: Path) -> list[Path]:
    """the gfx950 ELF of every bundle (one per translation unit) of the library's .hip_fatbin"""
    fat = tmp / (lib.name + ".fatbin")
    tool("llvm-objcopy", f"--dump-section=.hip_fatbin={fat}", str(lib), str(tmp / "unused"))
    data = fat.read_bytes()
    out = []
    for n, m in enumerate(re.finditer(re.escape(MAGIC), data)):
        base = m.start()
        pos = base + len(MAGIC)
        (entries,) = struct.unpack_from("<Q", data, pos)
        pos += 8
        for _ in range(entries):
            off, size, tlen = struct.unpack_from("<QQQ", data, pos)
            pos += 24
            triple = data[pos:pos + tlen].decode()
            pos += tlen
            if "gfx950" in triple and size:
                out.append(tmp / f"{lib.stem}_{n}.co")
                out[-1].write_bytes(data[base + off:base + off + size])
    return out


def functions(co: Path) -> dict[str, str]:
    """symbol -> its instructions, one per line, without addresses and encodings"""
    funcs: dict[str, list[str]] = {}
    cur = None
    for line in tool("llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", str(co)).splitlines():
        m = re.match(r"^(?:[0-9a-f]+ )?<([^>]+)>:$", line)
        if m:
            cur = funcs.setdefault(m.group(1), [])
        elif cur is not None and line.strip():
            text = re.sub(r"\s*//.*$", "", line).strip()
            if text:
                cur.append(text)
    res = {}
    for name, ins in funcs.items():
        while ins and ins[-1].split()[0] in ("s_code_end", "s_nop", "..."):     # the padding behind the last s_endpgm
            ins.pop()
        res[name] = "\n".join(ins)
    return res


def resources(co: Path) -> dict[str, tuple]:
    """kernel symbol -> the NOTES values of its entry in the code object's metadata"""
    res, name, vals = {}, None, {}
    text = tool("llvm-readelf", "--notes", str(co))
    for line in text.splitlines() + ["  - .end:"]:
        m = re.match(r"^\s+(- )?(\.[a-z_]+):\s*(.*)$", line)
        if not m:
            continue
        if m.group(1) and (name or vals):               # a new list item: the previous kernel is complete
            if name and all(k in vals for k in NOTES):
                res[name] = tuple(vals[k] for k in NOTES)
            name, vals = None, {}
        if m.group(2) == ".symbol":
            name = m.group(3).strip("'\"")
        elif m.group(2) in NOTES:
            vals[m.group(2)] = m.group(3)
    return res


def exported(lib: Path) -> set[str]:
    names = set()
    for line in tool("llvm-readelf", "--dyn-syms", "-W", str(lib)).splitlines():
        f = line.split()
        if len(f) == 8 and f[6] != "UND" and f[7].startswith("sm_"):
            names.add(f[7])
    return names


def survey(lib: Path, tmp: Path):
    funcs, res = {}, {}
    cos = code_objects(lib, tmp)
    for co in cos:
        for name, text in functions(co).items():
            if name in funcs and funcs[name] != text:
                print(f"{lib}: {name} is defined twice, differently")
            funcs[name] = text
        res.update(resources(co))
    return len(cos), funcs, res, exported(lib)


def main() -> int:
    added_ok = "--allow-added" in sys.argv
    args = [a for a in sys.argv[1:] if a != "--allow-added"]
    if len(args) != 2:
        print(__doc__)
        return 2
    old, new = Path(args[0]), Path(args[1])
    with tempfile.TemporaryDirectory() as t:
        n_old, f_old, r_old, e_old = survey(old, Path(t))
        n_new, f_new, r_new, e_new = survey(new, Path(t))
    if added_ok:                                        # a new stage: only OLD's symbols are compared
        f_new = {k: v for k, v in f_new.items() if k in f_old}
        r_new = {k: v for k, v in r_new.items() if k in r_old}
        e_new &= e_old
    bad = 0
    for name in sorted(set(f_old) | set(f_new)):
        if name not in f_new:
            print(f"missing in {new.name}: {name}")
        elif name not in f_old:
            print(f"extra in {new.name}: {name}")
        elif f_old[name] != f_new[name]:
            print(f"instructions differ: {name}")
        else:
            continue
        bad += 1
    for name in sorted(set(r_old) | set(r_new)):
        if r_old.get(name) != r_new.get(name):
            print(f"resources differ: {name}: {dict(zip(NOTES, r_old.get(name, ())))} -> {dict(zip(NOTES, r_new.get(name, ())))}")
            bad += 1
    for name in sorted(e_old ^ e_new):
        print(f"exported symbol {'missing' if name in e_old else 'extra'}: {name}")
        bad += 1
    print(f"{len(f_old)} symbols in {n_old} code objects against {len(f_new)} in {n_new}; {len(r_old)} kernels with notes "
          f"against {len(r_new)}; {len(e_old)} exported sm_* symbols against {len(e_new)}; {bad} differences")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
