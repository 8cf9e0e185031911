"""The signed carry-save network of the bit-sliced match kernel's row step (csrc/sm_bs_network.h), built for the
host -- bop<IMM> in plain C++ -- and run against integer arithmetic by tests/helpers/bs_network_check.cpp.

S' = S + (entering bits) - (leaving bits) for every window the library instantiates: all 2^18 combinations of
entering and leaving bits for 9 x 9 (and all of 3 x 3, 5 x 5 and 7 x 7), each with S in {0, 1, the value that makes S' = 0,
N^2 - 1, N^2} and 64 random values; 10^6 random cases for each larger window; everything entering an empty window,
everything leaving a full one, and ties.  Legal cases only (0 <= S, S' <= N^2): a candidate S outside the legal
range of its bits is moved to the nearest legal value, none is skipped.

The same program prints the number of operations the wiring generator emits next to the forms it replaces (two
count_lockstep trees and addsub_lockstep); DESIGN.md 5.1 quotes these."""
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "helpers" / "bs_network_check.cpp"
WINDOWS = (3, 5, 7, 9, 11, 13, 15, 17, 19, 21)
# N: (operations of the network, of the separate forms), per shift and row, mismatch bits not counted
OPS = {3: (13, 15), 5: (23, 27), 7: (31, 33), 9: (43, 49), 11: (49, 53), 13: (59, 63), 15: (65, 67), 17: (79, 87),
       19: (85, 91), 21: (93, 99)}


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = tmp_path_factory.mktemp("bs_network") / "bs_network_check"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", f"-I{ROOT / 'stereomatching_amd' / 'csrc'}",
                           str(SRC), "-o", str(exe)])
    return exe


def bits_for(v):
    return v.bit_length()


def separate_ops(n):
    """operations of count_lockstep x 2 + addsub_lockstep, counted here from their loops, not by the header.
    (The row step no longer runs those forms, and this follows the same description of their loops as
    net_ops_separate does: it guards against a slip in either, no more.  The literal OPS table is the pin.)"""
    hb, sb = bits_for(n), bits_for(n * n)
    tree, m = 0, n
    for _ in range(hb):
        full, rest = (m - 1) // 2 if m >= 3 else 0, 0
        left = m - 2 * full
        if left == 2:
            rest = 1
        tree += 2 * (full + rest)
        m = full + rest
    diff = 2 + 2 * (hb - 1)
    add = 2 + sum(2 if k + 1 < sb else 1 for k in range(1, sb))
    return 2 * tree + diff + add


def test_operation_counts(program):
    out = subprocess.run([str(program), "counts"], capture_output=True, text=True, check=True).stdout
    rows = {int(f[0]): tuple(map(int, f[1:])) for f in (line.split() for line in out.splitlines())}
    assert sorted(rows) == list(WINDOWS)
    for n in WINDOWS:
        sb, net, sep, cells = rows[n]
        assert sb == bits_for(n * n)
        assert sep == separate_ops(n), n
        assert (net, sep) == OPS[n], n
        assert net < sep, n
    assert OPS[9][1] - OPS[9][0] >= 2          # the issue's bar for going on


def test_network_equals_integer_arithmetic(program):
    p = subprocess.run([str(program), "check"], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    seen = {}
    for line in p.stdout.splitlines():
        f = dict(kv.split("=") for kv in line.split()[:3])
        seen[int(f["N"])] = int(f["cases"])
    assert sorted(seen) == list(WINDOWS), p.stdout
    assert seen[9] >= (1 << 18) * 69
    assert seen[3] >= (1 << 6) * 69
    assert all(seen[n] >= 1000000 for n in WINDOWS if n > 9), seen


def test_network_under_address_and_undefined_sanitizers(tmp_path):
    """the same program as a stand-alone host binary with -fsanitize=address,undefined"""
    exe = tmp_path / "bs_network_check_san"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           f"-I{ROOT / 'stereomatching_amd' / 'csrc'}", str(SRC), "-o", str(exe)])
    p = subprocess.run([str(exe), "check"], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
