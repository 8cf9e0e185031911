"""Occlusion-aware interpolation at 4K: time per call of sm_occlusion_classify and sm_interpolate (int32 and int16) with
device events after a warm-up, beside sm_median_filter 5 x 5 and sm_lr_check (with its zeroing kernel) on the same
shape in the same run as the yardsticks.  Three inputs: "scene", the checked web, sub and right maps of a real
sm_sgm_lr run on a make_pair scene (64 shifts, 1 x 1 window, 4 paths) after sm_speckle_filter(max_size 100); "band",
valid everywhere except a vertical band a quarter of the width wide; "lone", a single valid pixel in one corner (every
other pixel walks to the edge in seven directions).  One JSON line per input; the per-kernel times come from a kernel
trace of the same tool:

    python tools/interp_timing.py [--steps N] [--warmup N] [--out FILE]
    rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/interp_timing.py --steps 3 --warmup 1
    python tools/interp_timing.py --summarise DIR --out profiles/interp/kernel_stats.json"""
import argparse
import json
import re
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

W, H, D = 3840, 2160, 64
MAX_SIZE, MAX_DIFF = 100, 1


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


def measure(steps, warmup):
    import torch

    from stereomatching_amd import capi, pipeline
    from stereomatching_amd.synth import make_pair
    lib, ptr, check = pipeline.lib, pipeline._ptr, pipeline.check
    left, right = make_pair(W, H, D, seed=1)
    plan = pipeline.StereoPlan(W, H, D, 1, "toroidal")
    plan.reserve_sgm()
    plan.reserve_filter()
    plan.reserve_interp()
    scene = plan.sgm_lr(torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda(), 7, 10, 120, 4, max_diff=1,
                        want_right=True, want_sub=True)
    raw, _, _ = plan.sgm_wta(torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda(), 7, 10, 120, 4)
    web = plan.speckle_filter(scene.web, MAX_SIZE, MAX_DIFF)
    sub = plan.sub_mask(web, scene.sub.clone())
    xs = torch.arange(W, device="cuda", dtype=torch.int32)[None, None, :]
    ys = torch.arange(H, device="cuda", dtype=torch.int32)[None, :, None]
    band = (1 + (3 * xs + 7 * ys) % 23).to(torch.int32).contiguous()
    band[:, :, W // 3:W // 3 + W // 4] = 0
    lone = torch.zeros((1, H, W), dtype=torch.int32, device="cuda")
    lone[0, 0, 0] = 7
    flat = torch.full((1, H, W), 3, dtype=torch.int32, device="cuda")
    inputs = {"scene": (web, sub, raw, scene.web_right),
              "band": (band, (16 * band).to(torch.int16), band.clamp(min=1), flat),
              "lone": (lone, (16 * lone).to(torch.int16), lone.clamp(min=1), flat)}
    out32 = torch.empty((1, H, W), dtype=torch.int32, device="cuda")
    out16 = torch.empty((1, H, W), dtype=torch.int16, device="cuda")
    cls = torch.empty((1, H, W), dtype=torch.uint8, device="cuda")
    count = torch.empty(1, dtype=torch.int32, device="cuda")
    h_, st = plan._h, plan._stream()
    I32, I16 = capi.SM_MAP_I32, capi.SM_MAP_I16
    lines = []
    for name, (web, sub, unchecked, web_right) in inputs.items():
        calls = {
            "sm_lr_check_us": lambda: check(lib.sm_lr_check(h_, ptr(unchecked), ptr(web_right), 1, 1, ptr(out32),
                                                            ptr(count), st)),
            "median5_i32_us": lambda: check(lib.sm_median_filter(h_, ptr(web), I32, 5, 1, ptr(out32), st)),
            "median5_i16_us": lambda: check(lib.sm_median_filter(h_, ptr(sub), I16, 5, 1, ptr(out16), st)),
            "classify_us": lambda: check(lib.sm_occlusion_classify(h_, ptr(web), ptr(web_right), 1, ptr(cls), st)),
            "interpolate_i32_us": lambda: check(lib.sm_interpolate(h_, ptr(web), I32, ptr(cls), 1, ptr(out32),
                                                                   ptr(count), st)),
            "interpolate_i16_us": lambda: check(lib.sm_interpolate(h_, ptr(sub), I16, ptr(cls), 1, ptr(out16),
                                                                   ptr(count), st)),
        }
        calls["classify_us"]()
        torch.cuda.synchronize()
        npx = W * H
        res = {"input": name, "width": W, "height": H, "shifts": D, "steps": steps, "warmup": warmup,
               "invalid_share": round(int((web == 0).sum()) / npx, 4),
               "occluded_share": round(int((cls == 1).sum()) / npx, 4),
               "mismatched_share": round(int((cls == 2).sum()) / npx, 4)}
        for key, fn in calls.items():
            res[key] = per_step_us(fn, steps, warmup)
        calls["interpolate_i32_us"]()
        torch.cuda.synchronize()
        res["interpolate_i32_filled"] = int(count[0])
        res["interpolate_i32_over_median5_i32"] = round(res["interpolate_i32_us"] / res["median5_i32_us"], 2)
        res["interpolate_i16_over_median5_i16"] = round(res["interpolate_i16_us"] / res["median5_i16_us"], 2)
        lines.append(res)
        print(json.dumps(res), flush=True)
    plan.close()
    return lines


def summarise(root, out):
    """the rocprofv3 database under ROOT -> per-kernel dispatch durations of the interpolation's and the yardsticks'
    kernels"""
    import sqlite3
    dbs = sorted(Path(root).rglob("*.db"))
    res = {"source": "rocprofv3 --kernel-trace --stats -d ROOT -- python tools/interp_timing.py --steps 3 --warmup 1",
           "kernels": {}}
    if dbs:
        c = sqlite3.connect(str(dbs[-1]))
        for name, calls, mean, lo, hi in c.execute("select name, count(*), avg(duration), min(duration), max(duration) "
                                                   "from kernels group by name"):
            short = re.sub(r"^void ", "", name).split("(")[0]
            if re.search(r"k_itp|k_median|k_lr_check|k_lr_zero", short):
                res["kernels"][short] = {"calls": calls, "mean_us": round(mean / 1e3, 2), "min_us": round(lo / 1e3, 2),
                                         "max_us": round(hi / 1e3, 2)}
    Path(out).parent.mkdir(parents=True, exist_ok=True)
    Path(out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res, indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--summarise", default=None, metavar="ROOT")
    a = ap.parse_args()
    if a.summarise:
        summarise(a.summarise, a.out or "profiles/interp/kernel_stats.json")
        return
    lines = measure(a.steps, a.warmup)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("".join(json.dumps(r) + "\n" for r in lines))


if __name__ == "__main__":
    main()
