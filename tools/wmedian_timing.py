"""The guided weighted median at 4K: time per call of sm_weighted_median with device events after a warm-up, beside
sm_median_filter (k = 5) and sm_lr_check (with its zeroing kernel) in the same run as the yardsticks.  One JSON line
per case: map type (int32 / int16) x radius (1, 2, 3, 5, 7) x fill (off / on; 30 % of the pixels invalid in both) x value
range (128 shifts / 2048 subpixel steps) x content.  The bisection's passes follow the range of the values in a
window, so the content decides the time: "noise" is uniform over the whole range in every window (the worst case),
"scene" is a tilted plane with raised blocks and noise of +-1 (a window spans a few values, or one step).  Each line
carries its ratio to the k = 5 median of the same run and to the byte floor (map in + guide in + map out at 6.3 TB/s).
The per-kernel times come from a kernel trace of the same tool:

    python tools/wmedian_timing.py [--steps N] [--warmup N] [--out FILE]
    rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/wmedian_timing.py --steps 2 --warmup 1
    python tools/wmedian_timing.py --summarise DIR --out profiles/wmedian/kernel_stats.json"""
import argparse
import json
import re
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

W, H, D = 3840, 2160, 64
RADII = (1, 2, 3, 5, 7)
RANGES = {"128 shifts": 128, "2048 subpixel steps": 2048}
INVALID = 0.3
FLOOR_BYTES_PER_S = 6.3e12
FILL_MIN = 2048                     # two taps of the centre's own gray value (guide_weights(8): 1024 each)


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
    """-> {(content, range name): int64 map [1][H][W] with INVALID of it 0}, guide uint8 [1][H][W]"""
    yy, xx = torch.meshgrid(torch.arange(H, device="cuda"), torch.arange(W, device="cuda"), indexing="ij")
    blocks = ((xx // 240 + yy // 135) % 3 == 0)                      # raised blocks of 240 x 135 pixels
    guide = (60 + 60 * blocks + (xx * 40) // W + torch.randint(-3, 4, (H, W), generator=gen, device="cuda")).clamp(0, 255)
    hole = torch.rand((H, W), generator=gen, device="cuda") < INVALID
    maps = {}
    for name, n in RANGES.items():
        noise = torch.randint(1, n + 1, (H, W), generator=gen, device="cuda")
        plane = 1 + (xx * (n // 2 - 4)) // W + blocks * (n // 2) + torch.randint(0, 3, (H, W), generator=gen, device="cuda")
        for content, m in (("noise", noise), ("scene", plane.clamp(1, n))):
            maps[(content, name)] = torch.where(hole, 0, m)[None].contiguous()
    return maps, guide.to(torch.uint8)[None].contiguous()


def measure(steps, warmup):
    import torch

    from stereomatching_amd import capi, pipeline
    lib, ptr, check = pipeline.lib, pipeline._ptr, pipeline.check
    plan = pipeline.StereoPlan(W, H, D, 1, "toroidal")
    gen = torch.Generator(device="cuda").manual_seed(5)
    maps, guide = make_inputs(torch, gen)
    weights = capi.w256(pipeline.guide_weights(8))
    out = {torch.int32: torch.empty((1, H, W), dtype=torch.int32, device="cuda"),
           torch.int16: torch.empty((1, H, W), dtype=torch.int16, device="cuda")}
    count = torch.empty(1, dtype=torch.int32, device="cuda")
    h_, st = plan._h, plan._stream()
    npx = W * H
    lines = []
    for (content, rng), m64 in maps.items():
        for dtype, ty, name in ((torch.int32, capi.SM_MAP_I32, "int32"), (torch.int16, capi.SM_MAP_I16, "int16")):
            m, o = m64.to(dtype), out[dtype]
            med5 = per_step_us(lambda: check(lib.sm_median_filter(h_, ptr(m), ty, 5, 1, ptr(o), st)), steps, warmup)
            w32 = m64.to(torch.int32)
            lrc = per_step_us(lambda: check(lib.sm_lr_check(h_, ptr(w32), ptr(w32), 1, 1, ptr(out[torch.int32]), ptr(count),
                                                            st)), steps, warmup)
            floor_us = npx * (2 * m.element_size() + 1) / FLOOR_BYTES_PER_S * 1e6
            for radius in RADII:
                for fill in (False, True):
                    flags = capi.SM_WMED_FILL if fill else 0
                    us = per_step_us(lambda: check(lib.sm_weighted_median(h_, ptr(m), ty, ptr(guide), radius, weights, flags,
                                                                          FILL_MIN, 1, ptr(o), ptr(count), st)), steps, warmup)
                    torch.cuda.synchronize()
                    res = {"width": W, "height": H, "steps": steps, "warmup": warmup, "map": name, "range": rng,
                           "content": content, "invalid": INVALID, "radius": radius, "fill": fill,
                           "fill_min_weight": FILL_MIN if fill else None, "filled": int(count[0]), "wmedian_us": us,
                           "median5_us": med5, "sm_lr_check_us": lrc, "over_median5": round(us / med5, 2),
                           "floor_bytes": npx * (2 * m.element_size() + 1), "over_byte_floor": round(us / floor_us, 1)}
                    lines.append(res)
                    print(json.dumps(res), flush=True)
    plan.close()
    return lines


def summarise(root, out):
    """the rocprofv3 database under ROOT -> per-kernel dispatch durations of the filter's and the yardsticks' kernels"""
    import sqlite3
    dbs = sorted(Path(root).rglob("*.db"))
    res = {"source": "rocprofv3 --kernel-trace --stats -d ROOT -- python tools/wmedian_timing.py --steps 2 --warmup 1",
           "kernels": {}}
    if dbs:
        c = sqlite3.connect(str(dbs[-1]))
        tables = [r[0] for r in c.execute("select name from sqlite_master where type in ('table', 'view')")]
        table = "kernels" if "kernels" in tables else next(t for t in tables if t.startswith("kernels"))
        for name, calls, mean, lo, hi in c.execute(f"select name, count(*), avg(duration), min(duration), max(duration) "
                                                   f"from {table} group by name"):
            short = re.sub(r"^void ", "", name).split("(")[0]
            if re.search(r"k_wmedian|k_median|k_lr_check|k_lr_zero", short):
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
        summarise(a.summarise, a.out or "profiles/wmedian/kernel_stats.json")
        return
    lines = measure(a.steps, a.warmup)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("".join(json.dumps(r) + "\n" for r in lines))


if __name__ == "__main__":
    main()
