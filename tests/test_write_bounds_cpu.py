"""tests/guarded.py catches what it exists to catch: fake writers on CPU tensors, each with one store fault, and a
correct one that must pass.  The GPU module (test_write_bounds_gpu.py) relies on exactly these reports."""
import numpy as np
import pytest
import torch

from tests.guarded import guarded, guarded_input

PAIRS, MAX_PAIRS, H, W = 2, 3, 5, 7


def value(p, y, x):
    return 1 + (p * 31 + y * 7 + x) % 50


def writer(out, skip=None, extra=None):
    """writes value() into out (pairs, H, W); skip(p, y, x) -> True leaves an element alone; extra(flat) may store
    outside the view, through the flat storage the view lives in"""
    pairs, h, w = out.shape
    for p in range(pairs):
        for y in range(h):
            for x in range(w):
                if not (skip and skip(p, y, x)):
                    out[p, y, x] = value(p, y, x)


def run_twice(buf, write):
    """fill, write, collect problems -- once per poison"""
    probs = []
    for run in (0, 1):
        buf.fill(run)
        write(run)
        probs += buf.problems()
    return probs


def make(dtype=torch.int32, offset=0):
    return guarded((PAIRS, H, W), dtype, "cpu", offset=offset, max_pairs=MAX_PAIRS, name="web")


@pytest.mark.parametrize("dtype,offset", [(torch.int32, 0), (torch.int32, 4), (torch.uint8, 1), (torch.uint8, 3),
                                          (torch.uint16, 2), (torch.int16, 2)])
def test_correct_writer_is_accepted_and_offsets_give_the_alignment(dtype, offset):
    buf = make(dtype, offset)
    ptr = buf.t.data_ptr()
    assert ptr % 256 == offset
    if offset:
        assert ptr % buf.itemsize == 0
    assert run_twice(buf, lambda run: writer(buf.t)) == []
    want = np.array([[[value(p, y, x) for x in range(W)] for y in range(H)] for p in range(PAIRS)])
    assert np.array_equal(buf.value().astype(np.int64), want)
    # the guards are as large as promised
    assert buf.start >= buf.pair_bytes + 4096
    assert buf.raw.numel() - buf.end >= (MAX_PAIRS - PAIRS + 1) * buf.pair_bytes + 4096


def stray(buf, elem_offset, v=9):
    """store v at element elem_offset relative to the first owned element (may be outside the view)"""
    flat = buf.raw.view(torch.uint8)
    b = buf.start + elem_offset * buf.itemsize
    flat[b:b + buf.itemsize] = torch.tensor([v], dtype=buf.dtype).view(torch.uint8)


def test_one_element_past_the_end():
    buf = make()
    probs = run_twice(buf, lambda run: (writer(buf.t), stray(buf, PAIRS * H * W)))
    assert any("after the map" in p and "+0..+3" in p and "pair slot 2" in p for p in probs), probs


def test_one_element_before_the_start():
    buf = make(torch.uint16, 2)
    probs = run_twice(buf, lambda run: (writer(buf.t), stray(buf, -1)))
    assert any("before the map" in p and "-2..-1" in p for p in probs), probs


def test_write_into_the_first_unused_pair_slot():
    buf = make()
    probs = run_twice(buf, lambda run: (writer(buf.t), stray(buf, PAIRS * H * W + 2 * W + 3)))
    assert any("pair slot 2" in p for p in probs), probs


def test_write_past_every_pair_slot():
    buf = make()
    probs = run_twice(buf, lambda run: (writer(buf.t), stray(buf, MAX_PAIRS * H * W)))
    assert any("past the map" in p for p in probs), probs


def test_skipped_last_column():
    buf = make()
    probs = run_twice(buf, lambda run: writer(buf.t, skip=lambda p, y, x: x == W - 1))
    assert any(f"{PAIRS * H} of {PAIRS * H * W} elements not written" in p and f"(0, 0, {W - 1})" in p
               for p in probs), probs


def test_skipped_last_row():
    buf = make(torch.uint8, 3)
    probs = run_twice(buf, lambda run: writer(buf.t, skip=lambda p, y, x: p == PAIRS - 1 and y == H - 1))
    assert any(f"{W} of" in p and f"({PAIRS - 1}, {H - 1}, 0)" in p for p in probs), probs


def test_pixel_written_in_one_run_only():
    buf = make()
    probs = run_twice(buf, lambda run: writer(buf.t, skip=lambda p, y, x: run == 1 and (p, y, x) == (1, 2, 3)))
    assert any("1 of" in p and "(1, 2, 3)" in p for p in probs), probs


def test_writer_of_the_poison_value_is_not_mistaken_for_a_skip():
    """a pixel whose correct value happens to equal one run's poison is written in both runs: no report"""
    buf = make()

    def write(run):
        writer(buf.t)
        buf.t[0, 0, 0] = 0              # poison of run 0, written all the same
    assert run_twice(buf, write) == []


@pytest.mark.parametrize("offset", [0, 1, 3])
def test_input_modified_in_place(offset):
    data = np.arange(PAIRS * H * W, dtype=np.uint8).reshape(PAIRS, H, W)
    inp = guarded_input(data, "cpu", offset=offset, name="left")
    assert inp.t.data_ptr() % 256 == offset
    assert np.array_equal(inp.value(), data)
    assert inp.problems() == []
    inp.t[1, 4, 6] += 1
    probs = inp.problems()
    assert any("left: 1 bytes of the input changed" in p for p in probs), probs


def test_input_guard_overwritten():
    inp = guarded_input(np.ones((1, H, W), np.int32), "cpu", name="web")
    inp.raw[inp.end + 5] ^= 1
    probs = inp.problems()
    assert any("after the input changed" in p for p in probs), probs
