"""The disparity post-filters at 4K: time per call of sm_median_filter and sm_speckle_filter with device events after a
warm-up, beside sm_lr_check (with its zeroing kernel) on the same maps in the same run as the yardstick.  Two inputs:
the checked web map and the sub map of a real sm_sgm_lr run on a make_pair scene, and a map of uniform noise (every
pixel valid, values 1 .. 64: the worst case for the merge of the speckle filter).  One JSON line per input; the
per-kernel times come from a kernel trace of the same tool:

    python tools/filter_timing.py [--steps N] [--warmup N] [--out FILE]
    rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/filter_timing.py --steps 3 --warmup 1
    python tools/filter_timing.py --summarise DIR --out profiles/filter/kernel_stats.json"""
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
    scene = plan.sgm_lr(torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda(), 7, 10, 120, 4, max_diff=1,
                        want_right=True, want_sub=True)
    raw, _, _ = plan.sgm_wta(torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda(), 7, 10, 120, 4)
    g = torch.Generator(device="cuda").manual_seed(5)
    noise = torch.randint(1, 65, (1, H, W), generator=g, device="cuda", dtype=torch.int32)
    inputs = {"sgm_lr scene": (scene.web, scene.sub, raw, scene.web_right),
              "uniform noise": (noise, (16 * noise).to(torch.int16), noise, noise.flip(2).contiguous())}
    out32 = torch.empty((1, H, W), dtype=torch.int32, device="cuda")
    out16 = torch.empty((1, H, W), dtype=torch.int16, device="cuda")
    count = torch.empty(1, dtype=torch.int32, device="cuda")
    h_, st = plan._h, plan._stream()
    I32, I16 = capi.SM_MAP_I32, capi.SM_MAP_I16
    lines = []
    for name, (web, sub, unchecked, web_right) in inputs.items():
        calls = {
            "sm_lr_check_us": lambda: check(lib.sm_lr_check(h_, ptr(unchecked), ptr(web_right), 1, 1, ptr(out32),
                                                            ptr(count), st)),
            "median3_i16_us": lambda: check(lib.sm_median_filter(h_, ptr(sub), I16, 3, 1, ptr(out16), st)),
            "median5_i16_us": lambda: check(lib.sm_median_filter(h_, ptr(sub), I16, 5, 1, ptr(out16), st)),
            "median3_i32_us": lambda: check(lib.sm_median_filter(h_, ptr(web), I32, 3, 1, ptr(out32), st)),
            "median5_i32_us": lambda: check(lib.sm_median_filter(h_, ptr(web), I32, 5, 1, ptr(out32), st)),
            "speckle_i32_us": lambda: check(lib.sm_speckle_filter(h_, ptr(web), I32, MAX_SIZE, MAX_DIFF, 1, ptr(out32),
                                                                  ptr(count), st)),
            "speckle_i16_us": lambda: check(lib.sm_speckle_filter(h_, ptr(sub), I16, MAX_SIZE, 16 * MAX_DIFF, 1,
                                                                  ptr(out16), ptr(count), st)),
        }
        res = {"input": name, "width": W, "height": H, "steps": steps, "warmup": warmup, "max_size": MAX_SIZE,
               "max_diff": MAX_DIFF, "valid_pixels": int((web != 0).sum())}
        for key, fn in calls.items():
            res[key] = per_step_us(fn, steps, warmup)
        calls["speckle_i32_us"]()
        torch.cuda.synchronize()
        res["speckle_i32_removed"] = int(count[0])
        res["median3_i16_over_lr_check"] = round(res["median3_i16_us"] / res["sm_lr_check_us"], 2)
        res["speckle_i32_over_lr_check"] = round(res["speckle_i32_us"] / res["sm_lr_check_us"], 2)
        lines.append(res)
        print(json.dumps(res), flush=True)
    plan.close()
    return lines


def summarise(root, out):
    """the rocprofv3 database under ROOT -> per-kernel dispatch durations of the filters' and the check's kernels"""
    import sqlite3
    dbs = sorted(Path(root).rglob("*.db"))
    res = {"source": "rocprofv3 --kernel-trace --stats -d ROOT -- python tools/filter_timing.py --steps 3 --warmup 1",
           "kernels": {}}
    if dbs:
        c = sqlite3.connect(str(dbs[-1]))
        for name, calls, mean, lo, hi in c.execute("select name, count(*), avg(duration), min(duration), max(duration) "
                                                   "from kernels group by name"):
            short = re.sub(r"^void ", "", name).split("(")[0]
            if re.search(r"k_median|k_spk|k_lr_check|k_lr_zero", short):
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
        summarise(a.summarise, a.out or "profiles/filter/kernel_stats.json")
        return
    lines = measure(a.steps, a.warmup)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("".join(json.dumps(r) + "\n" for r in lines))


if __name__ == "__main__":
    main()
