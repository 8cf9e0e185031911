"""The row network of the bit-sliced match kernel with GROUPED inputs (csrc/sm_bs_network.h: of every three window
columns of a row side, two mismatch bits and the parity of the three), built for the host and run against integer
arithmetic S + (entering bits) - (leaving bits) by tests/helpers/bs_groups_check.cpp:

  * all 2^18 combinations of entering and leaving bits at 9 x 9, each with EVERY admissible S (0 <= S, S' <= N^2);
    the same for 3 x 3, 5 x 5 and 7 x 7;
  * 10^6 sampled combinations for each of 11 x 11 ... 21 x 21 (xorshift64, seed 0x9E3779B97F4A7C15, printed by the
    program), each with a random S and both ends of its admissible range, plus full / empty rows and groups;
  * the operation count: one fewer per group, net_ops(grouped) == net_ops(per bit) - 2 * (N // 3) for every window
    (also a static_assert of the program, next to the one on the dependency distance of the grouped plan)."""
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "helpers" / "bs_groups_check.cpp"
WINDOWS = (3, 5, 7, 9, 11, 13, 15, 17, 19, 21)
# operations of the per-bit network per shift and row (tests/test_bs_network_cpu.py pins the same figures)
PER_BIT = {3: 13, 5: 23, 7: 31, 9: 43, 11: 49, 13: 59, 15: 65, 17: 79, 19: 85, 21: 93}
SEED = 0x9E3779B97F4A7C15


def compile_program(exe, *flags):
    subprocess.check_call(["g++", "-std=c++17", *flags, "-Wall", "-Wextra", f"-I{ROOT / 'stereomatching_amd' / 'csrc'}",
                           str(SRC), "-o", str(exe)])
    return exe


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return compile_program(tmp_path_factory.mktemp("bs_groups") / "bs_groups_check", "-O2")


def admissible_cases(n):
    """number of (e, l, S) with 0 <= S <= n^2 and 0 <= S + #e - #l <= n^2 over all n-bit e, l"""
    from math import comb
    return sum(comb(n, a) * comb(n, b) * (n * n + 1 - abs(a - b)) for a in range(n + 1) for b in range(n + 1))


def check_output(p, sampled=False):
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    seen = {}
    for line in p.stdout.splitlines():
        f = dict(kv.split("=") for kv in line.split()[:4])
        assert int(f["seed"], 16) == SEED
        seen[int(f["N"])] = int(f["cases"])
    assert sorted(seen) == list(WINDOWS), p.stdout
    exhaustive = (3, 5, 7) if sampled else (3, 5, 7, 9)
    for n in exhaustive:
        assert seen[n] == admissible_cases(n), (n, seen[n])
    assert all(seen[n] >= (300000 if sampled else 3000000) for n in WINDOWS if n not in exhaustive), seen


def test_grouped_operation_counts(program):
    out = subprocess.run([str(program), "counts"], capture_output=True, text=True, check=True).stdout
    rows = {int(f[0]): tuple(map(int, f[1:])) for f in (line.split() for line in out.splitlines())}
    assert sorted(rows) == list(WINDOWS)
    for n in WINDOWS:
        sb, grouped, per_bit, groups, cells = rows[n]
        assert sb == (n * n).bit_length()
        assert per_bit == PER_BIT[n], n
        assert groups == n // 3, n
        assert grouped == per_bit - 2 * (n // 3), n
    assert rows[9][1] == 37


def test_grouped_network_equals_integer_arithmetic(program):
    check_output(subprocess.run([str(program), "check"], capture_output=True, text=True))


def test_grouped_network_under_address_and_undefined_sanitizers(tmp_path):
    """the same program as a stand-alone host binary with -fsanitize=address,undefined.  Its `sampled` mode: every
    window, all combinations up to 7 x 7, 10^5 sampled ones from 9 x 9 on -- the instrumented network is some 50 times
    slower, and which memory it touches does not depend on the bits (every index is a compile-time constant)"""
    exe = compile_program(tmp_path / "bs_groups_check_san", "-O1", "-g1", "-fsanitize=address,undefined",
                          "-fno-sanitize-recover=all")
    check_output(subprocess.run([str(exe), "sampled"], capture_output=True, text=True), sampled=True)
