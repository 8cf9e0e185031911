"""Reprojection at 4K: time per call (one 3840 x 2160 pair) with device events after a warm-up, for sm_reproject on
{I32, I16} maps x {depth, XYZ, both} (every pixel kept, no gate), for sm_point_cloud on an int32 map with 1 %, 50 % and
99 % of the pixels kept (records, indices and the gray image), and for the dense XYZ call on the same three maps.
Beside them, in the same run and on the same shape, the yardsticks sm_valid_mask and sm_median_filter(k = 3).  One JSON
line per row with the compulsory bytes (the map element plus 4 / 12 / 16 output bytes per pixel; for the cloud the map
element per pixel plus 16 record, 4 index and 1 gray byte per KEPT pixel), the bandwidth they imply and the multiple
of the floor at 6.3 TB/s; the per-kernel times come from a kernel trace of the same tool:

    python tools/reproject_timing.py [--steps N] [--warmup N] [--out FILE]
    rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/reproject_timing.py --steps 3 --warmup 1
    python tools/reproject_timing.py --summarise DIR --out profiles/reproject/kernel_stats.json"""
import argparse
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
    lib, ptr, check = pipeline.lib, pipeline._ptr, pipeline.check
    plan = pipeline.StereoPlan(W, H, 64, 1, "toroidal")
    plan.reserve_cloud()
    npx = W * H
    inf = float("inf")
    rng = np.random.default_rng(1)
    first = dict(fx=1.0, fy=1.0, cx=0.0, cy=0.0, new_fx=3500.0, new_fy=3501.5, new_cx=1919.25, new_cy=1080.5)
    q = capi.q16(pipeline.reprojection_matrix(first, dict(first, new_cx=1918.75), 0.12))      # Z = f t / (d + 0.5)
    web = torch.from_numpy(rng.integers(1, 65, (1, H, W), dtype=np.int32)).cuda()
    maps = {"int32": (web, capi.SM_MAP_I32, 4), "int16": ((web * 16).to(torch.int16), capi.SM_MAP_I16, 2)}
    depth = torch.empty((1, H, W), dtype=torch.float32, device="cuda")
    xyz = torch.empty((1, H, W, 3), dtype=torch.float32, device="cuda")
    count = torch.empty(1, dtype=torch.int32, device="cuda")
    h_, st = plan._h, plan._stream()
    lines = []

    def emit(r):
        lines.append(r)
        print(json.dumps(r), flush=True)
    for name, (m, mt, elem) in maps.items():
        for outs, (d_, x_, per_px) in {"depth": (depth, None, 4), "xyz": (None, xyz, 12), "both": (depth, xyz, 16)}.items():
            for counted in (False, True):
                fn = lambda: check(lib.sm_reproject(h_, ptr(m), mt, q, -inf, inf, 0.0, 1, ptr(d_), ptr(x_),
                                                    ptr(count if counted else None), st))
                emit(row("sm_reproject", per_step_us(fn, steps, warmup), npx * (elem + per_px), map=name, outputs=outs,
                         count=counted))
    # the cloud against the dense XYZ call at the same kept share
    gray = torch.from_numpy(rng.integers(0, 256, (1, H, W), dtype=np.uint8)).cuda()
    points = torch.empty((1, npx, 4), dtype=torch.float32, device="cuda")
    index = torch.empty((1, npx), dtype=torch.int32, device="cuda")
    for share in (0.01, 0.5, 0.99):
        m = torch.where(torch.from_numpy(rng.random((1, H, W)) < share).cuda(), web, torch.zeros_like(web))
        kept = int((m != 0).sum())
        fn = lambda: check(lib.sm_point_cloud(h_, ptr(m), capi.SM_MAP_I32, q, -inf, inf, ptr(gray), 1, npx, ptr(points),
                                              ptr(index), ptr(count), st))
        us = per_step_us(fn, steps, warmup)
        assert int(count[0]) == kept, (int(count[0]), kept)
        emit(row("sm_point_cloud", us, 4 * npx + 21 * kept, map="int32", kept_share=share, kept=kept))
        fn = lambda: check(lib.sm_point_cloud(h_, ptr(m), capi.SM_MAP_I32, q, -inf, inf, None, 1, 0, None, None, ptr(count), st))
        emit(row("sm_point_cloud count only", per_step_us(fn, steps, warmup), 4 * npx, map="int32", kept_share=share, kept=kept))
        fn = lambda: check(lib.sm_reproject(h_, ptr(m), capi.SM_MAP_I32, q, -inf, inf, 0.0, 1, None, ptr(xyz), ptr(count), st))
        emit(row("sm_reproject", per_step_us(fn, steps, warmup), npx * 16, map="int32", outputs="xyz", count=True,
                 kept_share=share))
    # the yardsticks, on maps of the same pixel count
    out32 = torch.empty_like(web)
    valid = torch.from_numpy((rng.random((1, H, W)) < 0.9).astype(np.uint8)).cuda()
    yard = {
        "sm_median_filter k=3 int32": (lambda: check(lib.sm_median_filter(h_, ptr(web), capi.SM_MAP_I32, 3, 1, ptr(out32), st)),
                                       8 * npx),
        "sm_valid_mask int32": (lambda: check(lib.sm_valid_mask(h_, ptr(out32), capi.SM_MAP_I32, ptr(valid), 1, st)), npx),
    }
    for name, (fn, nbytes) in yard.items():
        emit(row(name, per_step_us(fn, steps, warmup), nbytes))
    plan.close()
    return lines


def summarise(root, out):
    """the rocprofv3 database under ROOT -> per-kernel dispatch durations of the stage's and the yardsticks' kernels"""
    import sqlite3
    dbs = sorted(Path(root).rglob("*.db"))
    res = {"source": "rocprofv3 --kernel-trace --stats -d ROOT -- python tools/reproject_timing.py --steps 3 --warmup 1",
           "kernels": {}}
    if dbs:
        c = sqlite3.connect(str(dbs[-1]))
        tables = [r[0] for r in c.execute("select name from sqlite_master where type in ('table', 'view')")]
        table = "kernels" if "kernels" in tables else next((t for t in tables if t.startswith("kernels")), None)
        if table:
            for name, calls, mean, lo, hi in c.execute(f"select name, count(*), avg(duration), min(duration), max(duration) "
                                                       f"from {table} group by name"):
                short = re.sub(r"^void ", "", name).split("(")[0]
                if re.search(r"k_reproject|k_cloud|k_valid_mask|k_median|k_lr_zero", short):
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
        summarise(a.summarise, a.out or "profiles/reproject/kernel_stats.json")
        return
    lines = measure(a.steps, a.warmup)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("".join(json.dumps(r) + "\n" for r in lines))


if __name__ == "__main__":
    main()
