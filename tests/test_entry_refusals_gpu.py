"""What the eleven left / right / checked entry points of the cost modes refuse, and with which words: every bad call of
tests/refusal_cases.py against the record of the build before the entries shared a driver
(tests/golden/entry_refusals_parent.json, written by tools/record_refusals.py).  The first failing check decides the
message, so equal messages on the calls that break two rules mean an equal order of checks.  No kernel is launched."""
import json
from pathlib import Path

import pytest

from tests import refusal_cases as rc

GOLDEN = Path(__file__).parent / "golden" / "entry_refusals_parent.json"


def test_the_table_is_well_formed_and_matches_the_record():
    """on the CPU: unique names, at least three two-rule calls per entry, and the record holds exactly these cases"""
    names = [name for name, _, _ in rc.CASES]
    assert len(names) == len(set(names))
    for entry, params in rc.ENTRIES.items():
        mine = [(n, a) for n, e, a in rc.CASES if e == entry]
        assert all(len(a) == len(params) + 1 for _, a in mine), entry
        assert sum(" + " in n for n, _ in mine) >= 3, entry
    golden = json.loads(GOLDEN.read_text())
    assert set(golden) == set(names)
    assert all(r != 0 and n.split(":")[0] + ": " in m for n, (r, m) in golden.items())


@pytest.mark.gpu
def test_every_refusal_is_the_parents(hip):
    golden = json.loads(GOLDEN.read_text())
    got = rc.replay(hip)
    assert set(got) == set(golden)
    wrong = {n: (got[n][:2], golden[n]) for n in golden if got[n][:2] != golden[n]}
    assert not wrong, wrong
    grew = {n: v[2:] for n, v in got.items() if v[2] != v[3]}
    assert not grew, grew
