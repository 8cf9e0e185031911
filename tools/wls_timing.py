"""The edge-aware smoother at 4K: time per call of sm_wls_filter with device events after a warm-up, beside
sm_weighted_median (r = 5) and sm_median_filter (k = 5) in the same run as the yardsticks.  One JSON line per case: T
(1, 3) x map type (int16 / int32, the output of the same type) x confidence (NULL / given), on a scene map (a tilted
plane with raised blocks, noise of +-1 step, 30 % of the pixels invalid) with guide_weights(8).  Each line carries its
ratio to the yardsticks and to the byte floor: per pass pair (rows and columns, forward and backward) 81 bytes a pixel --
forward reads N, M and the guide byte and writes cp, N, M (41), backward reads cp, N, M and writes N, M (40) -- plus
init (map and confidence in, N and M out) and finish (map, N, M in, map out), at 6.3 TB/s.
The per-kernel times come from a kernel trace of the same tool, in a run of its own:

    python tools/wls_timing.py [--steps N] [--warmup N] [--out FILE]
    rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/wls_timing.py --steps 2 --warmup 1
    python tools/wls_timing.py --summarise DIR --out profiles/wls/kernel_stats.json"""
import argparse
import json
import re
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

W, H, D = 3840, 2160, 64
ITERATIONS = (1, 3)
INVALID = 0.3
LAMBDA = 64 / 1024                  # a smoothing strength of 64 with guide_weights(8)'s peak of 1024
FLOOR_BYTES_PER_S = 6.3e12


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


def make_inputs(torch, gen):
    """-> map in shifts (int64 [1][H][W], INVALID of it 0), guide uint8 [1][H][W], confidence uint8 [1][H][W]"""
    yy, xx = torch.meshgrid(torch.arange(H, device="cuda"), torch.arange(W, device="cuda"), indexing="ij")
    blocks = ((xx // 240 + yy // 135) % 3 == 0)                      # raised blocks of 240 x 135 pixels
    guide = (60 + 60 * blocks + (xx * 40) // W + torch.randint(-3, 4, (H, W), generator=gen, device="cuda")).clamp(0, 255)
    hole = torch.rand((H, W), generator=gen, device="cuda") < INVALID
    plane = 1 + (xx * (D // 2 - 4)) // W + blocks * (D // 2) + torch.randint(0, 3, (H, W), generator=gen, device="cuda")
    conf = torch.randint(0, 256, (H, W), generator=gen, device="cuda")
    return (torch.where(hole, 0, plane.clamp(1, D))[None].contiguous(), guide.to(torch.uint8)[None].contiguous(),
            conf.to(torch.uint8)[None].contiguous())


def floor_bytes(iterations, elem, with_conf):
    npx = W * H
    return npx * (81 * iterations + (elem + with_conf + 16) + (elem + 16 + elem))


def measure(steps, warmup):
    import torch

    from stereomatching_amd import capi, pipeline
    lib, ptr, check = pipeline.lib, pipeline._ptr, pipeline.check
    plan = pipeline.StereoPlan(W, H, D, 1, "toroidal")
    plan.reserve_wls()
    gen = torch.Generator(device="cuda").manual_seed(5)
    m64, guide, conf = make_inputs(torch, gen)
    table = pipeline.guide_weights(8)
    weights = capi.w256(table)
    count = torch.empty(1, dtype=torch.int32, device="cuda")
    h_, st = plan._h, plan._stream()
    lines = []
    for dtype, ty, name in ((torch.int16, capi.SM_MAP_I16, "int16"), (torch.int32, capi.SM_MAP_I32, "int32")):
        m = (m64 * 16 if dtype == torch.int16 else m64).to(dtype)
        o = torch.empty_like(m)
        med5 = per_step_us(lambda: check(lib.sm_median_filter(h_, ptr(m), ty, 5, 1, ptr(o), st)), steps, warmup)
        wmed5 = per_step_us(lambda: check(lib.sm_weighted_median(h_, ptr(m), ty, ptr(guide), 5, weights, 0, 1, 1, ptr(o),
                                                                 ptr(count), st)), steps, warmup)
        for iterations in ITERATIONS:
            for cf in (None, conf):
                us = per_step_us(lambda: check(lib.sm_wls_filter(h_, ptr(m), ty, ptr(cf), ptr(guide), weights, LAMBDA,
                                                                 iterations, 0, 1, ptr(o), ty, None, ptr(count), st)),
                                 steps, warmup)
                torch.cuda.synchronize()
                floor = floor_bytes(iterations, m.element_size(), cf is not None)
                res = {"width": W, "height": H, "steps": steps, "warmup": warmup, "map": name, "iterations": iterations,
                       "confidence": cf is not None, "invalid": INVALID, "lambda": LAMBDA, "filled": int(count[0]),
                       "dense": bool((o != 0).all()), "wls_us": us, "weighted_median5_us": wmed5, "median5_us": med5,
                       "over_weighted_median5": round(us / wmed5, 2), "over_median5": round(us / med5, 2),
                       "floor_bytes": floor, "over_byte_floor": round(us / (floor / FLOOR_BYTES_PER_S * 1e6), 1)}
                lines.append(res)
                print(json.dumps(res), flush=True)
    plan.close()
    return lines


def summarise(root, out):
    """the rocprofv3 database under ROOT -> per-kernel dispatch durations of the smoother's and the yardsticks' kernels"""
    import sqlite3
    dbs = sorted(Path(root).rglob("*.db"))
    res = {"source": "rocprofv3 --kernel-trace --stats -d ROOT -- python tools/wls_timing.py --steps 2 --warmup 1",
           "kernels": {}}
    if dbs:
        c = sqlite3.connect(str(dbs[-1]))
        tables = [r[0] for r in c.execute("select name from sqlite_master where type in ('table', 'view')")]
        table = "kernels" if "kernels" in tables else next(t for t in tables if t.startswith("kernels"))
        for name, calls, mean, lo, hi in c.execute(f"select name, count(*), avg(duration), min(duration), max(duration) "
                                                   f"from {table} group by name"):
            short = re.sub(r"^void ", "", name).split("(")[0]
            if re.search(r"k_wls|k_wmedian|k_median|k_lr_zero", short):
                res["kernels"][short] = {"calls": calls, "mean_us": round(mean / 1e3, 2), "min_us": round(lo / 1e3, 2),
                                         "max_us": round(hi / 1e3, 2)}
    Path(out).parent.mkdir(parents=True, exist_ok=True)
    Path(out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res, indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--summarise", default=None, metavar="ROOT")
    a = ap.parse_args()
    if a.summarise:
        summarise(a.summarise, a.out or "profiles/wls/kernel_stats.json")
        return
    lines = measure(a.steps, a.warmup)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("".join(json.dumps(r) + "\n" for r in lines))


if __name__ == "__main__":
    main()
