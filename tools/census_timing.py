"""Census cost mode: time per call of sm_census_transform (one pair: both images), sm_census_wta (transform included),
sm_census_lr and sm_census_refine on one plan, with device events after a warm-up, beside C3 SAD (sm_cost_wta) on the
same plan for scale.  One JSON line per configuration; the per-kernel times come from a kernel trace of the same tool,
one rocprofv3 run per configuration:

    python tools/census_timing.py [C3:7 C3:5 C3:3 C5:7 ...] [--steps N] [--warmup N] [--out FILE]
    rocprofv3 --kernel-trace --stats -d DIR/C3-7 -o run -- python tools/census_timing.py C3:7 ...
    python tools/census_timing.py --summarise DIR --out profiles/census/kernel_stats.json

A configuration is <CONFIGS name of stereomatching_amd/synth.py>:<census width>."""
import argparse
import csv
import json
import re
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

DEFAULT = ["C3:7", "C3:5", "C3:3", "C5:7"]


def per_step_ms(fn, steps, warmup):
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
    return e0.elapsed_time(e1) / steps


def measure(spec, steps, warmup):
    import torch

    from stereomatching_amd import pipeline
    from stereomatching_amd.synth import CONFIGS, make_pair
    cfg, c = spec.split(":")
    c = int(c)
    w, h, d, sw, mode = CONFIGS[cfg]
    left, right = make_pair(w, h, d, seed=1)
    L, R = torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda()
    LR = torch.stack([L, R])
    plan = pipeline.StereoPlan(w, h, d, sw, mode)
    plan.reserve_census()
    web = torch.empty((1, h, w), dtype=torch.int32, device="cuda")
    sub = torch.empty((1, h, w), dtype=torch.int16, device="cuda")
    desc = torch.empty((2, h, w), dtype=torch.int64, device="cuda")
    rejected = torch.empty(1, dtype=torch.int32, device="cuda")
    lib, h_, ptr = pipeline.lib, plan._h, pipeline._ptr

    def transform():
        pipeline.check(lib.sm_census_transform(h_, ptr(LR), c, 2, ptr(desc), plan._stream()))

    def census_wta():
        pipeline.check(lib.sm_census_wta(h_, ptr(L), ptr(R), c, 1, ptr(web), None, plan._stream()))

    def census_lr():
        pipeline.check(lib.sm_census_lr(h_, ptr(L), ptr(R), c, 1, 0, ptr(web), None, None, ptr(rejected),
                                        plan._stream()))

    def census_refine():
        pipeline.check(lib.sm_census_refine(h_, ptr(L), ptr(R), c, 1, ptr(web), ptr(sub), None, plan._stream()))

    def sad_wta():
        pipeline.check(lib.sm_cost_wta(h_, ptr(L), ptr(R), 1, 1, ptr(web), None, plan._stream()))

    census_lr()
    torch.cuda.synchronize()
    res = {"config": cfg, "census": c, "width": w, "height": h, "num_shifts": d, "square_width": sw, "border": mode,
           "steps": steps, "warmup": warmup}
    for name, fn in (("sm_census_transform_ms", transform), ("sm_census_wta_ms", census_wta),
                     ("sm_census_lr_ms", census_lr), ("sm_census_refine_ms", census_refine),
                     ("sm_cost_wta_sad_ms", sad_wta)):
        res[name] = round(per_step_ms(fn, steps, warmup), 4)
    res["targets_ms"] = {"sm_census_transform": 0.040, "sm_census_wta": 0.75,
                         "sm_census_lr": round(2 * res["sm_census_wta_ms"] + 0.060, 4)}
    res["rejected_pixels"] = int(rejected[0])
    res["pixel_shifts"] = w * h * d
    # the public transform reads the two images and writes 8 bytes per pixel of each
    res["transform_compulsory_bytes"] = 2 * w * h * (1 + 8)
    plan.close()
    return res


def summarise(root, out):
    """kernel_stats.csv of one rocprofv3 run per configuration (ROOT/<config>-<census>/...) -> one JSON file"""
    res = {"source": "rocprofv3 --kernel-trace --stats -d ROOT/<config>-<census> -- python tools/census_timing.py "
                     "<config>:<census> (one run per configuration); per-kernel dispatch durations",
           "configs": {}}
    for d in sorted(p for p in Path(root).iterdir() if p.is_dir()):
        stats = sorted(d.rglob("*kernel_stats.csv"))
        if not stats:
            continue
        kernels = {}
        with open(stats[-1]) as f:
            for row in csv.DictReader(f):
                name = re.sub(r"^void ", "", row["Name"]).split("(")[0]
                kernels[name] = {"calls": int(row["Calls"]), "mean_us": round(float(row["AverageNs"]) / 1e3, 2),
                                 "min_us": round(float(row["MinNs"]) / 1e3, 2)}
        res["configs"][d.name] = kernels
    Path(out).parent.mkdir(parents=True, exist_ok=True)
    Path(out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res, indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("configs", nargs="*", default=DEFAULT)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--summarise", default=None, metavar="ROOT")
    a = ap.parse_args()
    if a.summarise:
        summarise(a.summarise, a.out or "profiles/census/kernel_stats.json")
        return
    lines = []
    for spec in a.configs:
        res = measure(spec, a.steps, a.warmup)
        print(json.dumps(res), flush=True)
        lines.append(res)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("".join(json.dumps(r) + "\n" for r in lines))


if __name__ == "__main__":
    main()
