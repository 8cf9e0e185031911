"""Rectification at 4K: time per sm_rectify call (one 3840 x 2160 pair, both sides) with device events after a warm-up,
for {ABS32, REL16} x {bilinear, nearest} x {validity on, off} x three maps: "identity"; "smooth", the calibration of
tests/rectify_patterns.smooth_calibration (k1 = -0.12, a 0.02 rad rotation; built by sm_rectify_map_build); "random", a
permutation of the pixels with random fractions (the locality worst case; ABS32 only, its displacements do not fit
REL16).  Beside them, in the same run and on the same shape, the yardsticks sm_lr_check and sm_median_filter(k = 3),
and sm_rectify_map_build and sm_valid_mask.  One JSON line per row with the compulsory bytes (map entry + one source
byte + output + validity per pixel, both sides), the bandwidth they imply and the multiple of the floor at 6.3 TB/s;
the per-kernel times come from a kernel trace of the same tool:

    python tools/rectify_timing.py [--steps N] [--warmup N] [--out FILE]
    rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/rectify_timing.py --steps 3 --warmup 1
    python tools/rectify_timing.py --summarise DIR --out profiles/rectify/kernel_stats.json"""
import argparse
import ctypes
import json
import re
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

W, H = 3840, 2160
HBM_TBS = 6.3


def per_step_us(fn, steps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return round(e0.elapsed_time(e1) / steps * 1e3, 2)


def row(name, us, nbytes, **more):
    floor_us = nbytes / (HBM_TBS * 1e12) * 1e6
    return dict(call=name, **more, us=us, compulsory_bytes=nbytes, tb_per_s=round(nbytes / us / 1e6, 3),
                floor_us=round(floor_us, 2), times_floor=round(us / floor_us, 2))


def measure(steps, warmup):
    import numpy as np
    import torch

    from stereomatching_amd import capi, pipeline
    from tests import rectify_patterns as rp
    lib, ptr, check = pipeline.lib, pipeline._ptr, pipeline.check
    plan = pipeline.StereoPlan(W, H, 64, 1, "toroidal")
    npx = W * H
    rng = np.random.default_rng(1)
    raw_l = torch.from_numpy(rng.integers(0, 256, (1, H, W), dtype=np.uint8)).cuda()
    raw_r = torch.from_numpy(rng.integers(0, 256, (1, H, W), dtype=np.uint8)).cuda()
    xs = torch.arange(W, device="cuda", dtype=torch.int32)[None, :].expand(H, W)
    ys = torch.arange(H, device="cuda", dtype=torch.int32)[:, None].expand(H, W)
    perm = torch.from_numpy(rng.permutation(npx).astype(np.int32).reshape(H, W)).cuda()
    frac = torch.from_numpy(rng.integers(0, 32, (H, W, 2), dtype=np.int32)).cuda()
    maps = {
        ("identity", "abs32"): (torch.stack([32 * xs, 32 * ys], dim=-1).contiguous(),) * 2,
        ("identity", "rel16"): (torch.zeros((H, W, 2), dtype=torch.int16, device="cuda"),) * 2,
        ("random", "abs32"): ((torch.stack([32 * (perm % W), 32 * (perm // W)], dim=-1) + frac).contiguous(),) * 2,
    }
    build = {}
    for fmt in ("abs32", "rel16"):
        calibs = [capi.RectifyCalib.make(**rp.smooth_calibration(W, H, side)) for side in (0, 1)]
        maps[("smooth", fmt)] = tuple(plan.rectify_map(c, fmt) for c in calibs)
        out = maps[("smooth", fmt)][0]
        build[fmt] = per_step_us(lambda: check(lib.sm_rectify_map_build(plan._h, ctypes.byref(calibs[0]), capi.RMAP_FORMATS[fmt],
                                                                        ptr(out), plan._stream())), steps, warmup)
    left = torch.empty((1, H, W), dtype=torch.uint8, device="cuda")
    right, vl, vr = torch.empty_like(left), torch.empty_like(left), torch.empty_like(left)
    h_, st = plan._h, plan._stream()
    lines = []
    for (name, fmt), (ml, mr) in maps.items():
        for interp in ("bilinear", "nearest"):
            for valid in (True, False):
                fn = lambda: check(lib.sm_rectify(h_, ptr(raw_l), ptr(raw_r), W, H, ptr(ml), ptr(mr), capi.RMAP_FORMATS[fmt],
                                                  capi.INTERPS[interp], 0, 1, ptr(left), ptr(right),
                                                  ptr(vl if valid else None), ptr(vr if valid else None), st))
                per_px = (8 if fmt == "abs32" else 4) + 1 + 1 + (1 if valid else 0)
                lines.append(row("sm_rectify", per_step_us(fn, steps, warmup), 2 * npx * per_px, map=name, format=fmt,
                                 interp=interp, validity=valid))
                print(json.dumps(lines[-1]), flush=True)
    # the yardsticks, on maps of the same pixel count
    web = torch.from_numpy(rng.integers(1, 65, (1, H, W), dtype=np.int32)).cuda()
    web_right = torch.from_numpy(rng.integers(1, 65, (1, H, W), dtype=np.int32)).cuda()
    out32 = torch.empty_like(web)
    count = torch.empty(1, dtype=torch.int32, device="cuda")
    yard = {
        "sm_lr_check": (lambda: check(lib.sm_lr_check(h_, ptr(web), ptr(web_right), 1, 1, ptr(out32), ptr(count), st)),
                        12 * npx),
        "sm_median_filter k=3 int32": (lambda: check(lib.sm_median_filter(h_, ptr(web), capi.SM_MAP_I32, 3, 1, ptr(out32),
                                                                          st)), 8 * npx),
        "sm_valid_mask int32": (lambda: check(lib.sm_valid_mask(h_, ptr(out32), capi.SM_MAP_I32, ptr(vl), 1, st)), npx),
    }
    for name, (fn, nbytes) in yard.items():
        lines.append(row(name, per_step_us(fn, steps, warmup), nbytes))
        print(json.dumps(lines[-1]), flush=True)
    for fmt, us in build.items():
        lines.append(row("sm_rectify_map_build", us, npx * (8 if fmt == "abs32" else 4), format=fmt))
        print(json.dumps(lines[-1]), flush=True)
    plan.close()
    return lines


def summarise(root, out):
    """the rocprofv3 database under ROOT -> per-kernel dispatch durations of the stage's and the yardsticks' kernels"""
    import sqlite3
    dbs = sorted(Path(root).rglob("*.db"))
    res = {"source": "rocprofv3 --kernel-trace --stats -d ROOT -- python tools/rectify_timing.py --steps 3 --warmup 1",
           "kernels": {}}
    if dbs:
        c = sqlite3.connect(str(dbs[-1]))
        tables = [r[0] for r in c.execute("select name from sqlite_master where type in ('table', 'view')")]
        table = "kernels" if "kernels" in tables else next((t for t in tables if t.startswith("kernels")), None)
        if table:
            for name, calls, mean, lo, hi in c.execute(f"select name, count(*), avg(duration), min(duration), max(duration) "
                                                       f"from {table} group by name"):
                short = re.sub(r"^void ", "", name).split("(")[0]
                if re.search(r"k_rectify|k_rmap|k_valid_mask|k_median|k_lr_check|k_lr_zero", short):
                    res["kernels"][short] = {"calls": calls, "mean_us": round(mean / 1e3, 2), "min_us": round(lo / 1e3, 2),
                                             "max_us": round(hi / 1e3, 2)}
    Path(out).parent.mkdir(parents=True, exist_ok=True)
    Path(out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res, indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--summarise", default=None, metavar="ROOT")
    a = ap.parse_args()
    if a.summarise:
        summarise(a.summarise, a.out or "profiles/rectify/kernel_stats.json")
        return
    lines = measure(a.steps, a.warmup)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("".join(json.dumps(r) + "\n" for r in lines))


if __name__ == "__main__":
    main()
