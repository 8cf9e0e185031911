"""CPU tests of bench.py's --dump-outputs writer and of its --steps check."""
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import bench  # noqa: E402


def test_outputs_are_written_in_a_float_type_that_holds_them_exactly(tmp_path):
    rng = np.random.default_rng(3)
    small = rng.integers(-(1 << 24), 1 << 24, (2, 5, 7), dtype=np.int32)
    large = small.astype(np.int64) * 4 + 1                      # beyond float32's exact integers
    rec = bench.dump_outputs(str(tmp_path / "out"), {"web": small, "best": large}, 1 << 20)
    web, best = np.load(tmp_path / "out" / "web.npy"), np.load(tmp_path / "out" / "best.npy")
    assert web.dtype == np.float32 and np.array_equal(web, small)
    assert best.dtype == np.float64 and np.array_equal(best, large)
    assert rec["web"] == {"shape": [2, 5, 7], "dtype": "float32", "sampled": False}
    assert rec["best"]["dtype"] == "float64" and rec["best"]["sampled"] is False


def test_outputs_beyond_the_limit_are_the_same_seeded_sample_every_time(tmp_path):
    web = np.arange(3 * 40 * 50, dtype=np.int32).reshape(3, 40, 50)
    best = (web % 97).astype(np.int32)
    limit = web.nbytes // 2                                     # float32: both come to 2 x the limit
    rec = bench.dump_outputs(str(tmp_path / "a"), {"web": web, "best": best}, limit)
    bench.dump_outputs(str(tmp_path / "b"), {"web": web, "best": best}, limit)
    total = 0
    for name, full in (("web", web), ("best", best)):
        a, b = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert np.array_equal(a, b) and a.dtype == np.float32
        assert rec[name]["sampled"] is True and rec[name]["elements"] == a.size == full.size // 4
        # the documented draw: sorted flat indices from the generator seeded with [0, size]
        idx = np.sort(np.random.default_rng([0, full.size]).choice(full.size, a.size, replace=False))
        assert np.array_equal(a, full.reshape(-1)[idx].astype(np.float32))
        total += a.nbytes
    assert total <= limit


@pytest.mark.parametrize("steps", ["0", "-3"])
def test_steps_below_one_are_refused(steps):
    with pytest.raises(SystemExit):
        bench.parse(["--steps", steps])
    assert bench.parse(["--steps", "1"]).steps == 1
