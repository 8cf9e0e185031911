"""The plans whose geometry on the real device is pinned by tests/golden/plan_geometry_mi355x.json.gz: shared by
tools/record_plan_geometry.py (which wrote that file at the commit it names) and tests/test_plan_geometry_gpu.py.

A case is (width, height, num_shifts, square_width, border, max_pairs, options); its key is its text."""
from stereomatching_amd.synth import CONFIGS

WINDOWS = list(range(1, 28, 2))
SHIFTS = [1, 15, 16, 17, 64, 100, 128, 256, 512, 513, 1024, 1025]
# every option of sm_plan_options that planning reads, at each of its values
OPTIONS = [{"kernel_family": 1}, {"tile_h": 1}, {"tile_h": 7}, {"tile_h": 300},
           {"shifts_per_lane": 4}, {"shifts_per_lane": 8}, {"shifts_per_lane": 16},
           {"workgroup_waves": 1}, {"workgroup_waves": 2}, {"no_two_wave_cap": 1},
           {"lane_merge": 1}, {"lane_merge": 2}, {"no_four_shift_lanes": 1}]
OPTION_SHAPES = [(640, 480, 64, 7, "toroidal", 1), (640, 480, 128, 11, "ghost", 1), (1920, 1080, 64, 7, "toroidal", 1)]


def cases():
    out = []
    for name, (w, h, d, s, border) in CONFIGS.items():
        for pairs in (1, 8, 64) if name == "C4" else (1, 8):
            out.append((w, h, d, s, border, pairs, {}))
    for s in WINDOWS:
        for d in SHIFTS:
            out.append((640, 480, d, s, "toroidal", 1, {}))
        for d in (64, 256):
            out.append((640, 480, d, s, "ghost", 1, {}))
    for shape in OPTION_SHAPES:
        for opt in OPTIONS:
            out.append((*shape, dict(opt)))
    # (C4 is C2's shape: each plan once)
    return list({key(c): c for c in out}.values())


def key(case) -> str:
    w, h, d, s, border, pairs, opt = case
    return f"{w}x{h} D={d} S={s} {border} x{pairs}" + "".join(f" {k}={v}" for k, v in sorted(opt.items()))
