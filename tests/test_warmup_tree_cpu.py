"""The counter of a two-wave workgroup's shared warm-up rows (count_chain_lockstep of csrc/sm_bs_network.h: the
HALF * N mismatch bits of one shift to their count on bits_for(HALF * N) planes), built for the host and run against
integer popcounts by tests/helpers/warmup_tree_check.cpp, 32 cases per word, four items side by side as in the kernel and two in a second pass,
for every window whose two-wave builds take the counter (warm_tree_taken of csrc/sm_match_bs_kernel.h):

  * every input pattern where HALF * N <= 21 (5 x 5, 7 x 7);
  * at 9 x 9, 11 x 11 and 13 x 13 every pattern of weight <= 2 and >= HALF * N - 2, all-zero and all-one among them, and 10^6
    random patterns (xorshift64, seed 0x9E3779B97F4A7C15, printed by the program);
  * the operation count per shift, mismatch bits included: 104 at 9 x 9 against 144 row by row (also a static_assert
    of the program and of the kernel), and fewer than row by row at every window."""
import subprocess
from math import comb
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "helpers" / "warmup_tree_check.cpp"
WINDOWS = (5, 7, 9, 11, 13)
SEED = 0x9E3779B97F4A7C15


def compile_program(exe, *flags):
    subprocess.check_call(["g++", "-std=c++17", *flags, "-Wall", "-Wextra", f"-I{ROOT / 'stereomatching_amd' / 'csrc'}",
                           str(SRC), "-o", str(exe)])
    return exe


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return compile_program(tmp_path_factory.mktemp("warmup_tree") / "warmup_tree_check", "-O2")


def check_output(p, sampled=False):
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    seen = {}
    for line in p.stdout.splitlines():
        f = dict(kv.split("=") for kv in line.split()[:5])
        assert int(f["seed"], 16) == SEED
        n = int(f["N"])
        assert int(f["NI"]) == n // 2 * n and int(f["TB"]) == (n // 2 * n).bit_length()
        seen[n] = int(f["cases"])
    assert sorted(seen) == list(WINDOWS), p.stdout
    for n in WINDOWS:
        ni = n // 2 * n
        if ni <= (10 if sampled else 21):
            assert seen[n] == 2 ** ni, (n, seen[n])
        else:
            assert seen[n] == 2 * (1 + ni + comb(ni, 2)) + (100000 if sampled else 1000000), (n, seen[n])


def test_operation_counts(program):
    out = subprocess.run([str(program), "counts"], capture_output=True, text=True, check=True).stdout
    rows = {int(f[0]): tuple(map(int, f[1:])) for f in (line.split() for line in out.splitlines())}
    assert sorted(rows) == list(WINDOWS)
    for n in WINDOWS:
        ni, tb, tree, by_rows, cells = rows[n]
        assert ni == n // 2 * n and tb == ni.bit_length()
        # row by row: per row n bits, a tree n -> HB planes (two operations per adder) and a ripple add into SB planes
        assert tree < by_rows, n
        # every cell but those of the top plane is two operations
        assert ni + cells <= tree <= ni + 2 * cells, n
    assert rows[9][2:4] == (104, 144)


def test_counter_equals_integer_popcount(program):
    check_output(subprocess.run([str(program), "check"], capture_output=True, text=True))


def test_counter_under_address_and_undefined_sanitizers(tmp_path):
    """the same program as a stand-alone host binary with -fsanitize=address,undefined.  Its `sampled` mode: every
    window, all patterns up to 10 inputs, the light and heavy patterns and 10^5 random ones above -- the instrumented
    counter is some 50 times slower, and which memory it touches does not depend on the bits (every index is a
    compile-time constant)"""
    exe = compile_program(tmp_path / "warmup_tree_check_san", "-O1", "-g1", "-fsanitize=address,undefined",
                          "-fno-sanitize-recover=all")
    check_output(subprocess.run([str(exe), "sampled"], capture_output=True, text=True), sampled=True)
