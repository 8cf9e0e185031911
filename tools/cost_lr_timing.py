"""Left-right consistency check of the cost mode: time per step of sm_cost_wta and of sm_cost_lr on one plan, with
device events after a warm-up, at the configurations of DESIGN.md section 12 (C3 SAD, C3 SSD, C5 SSD with the ghost
border).  One JSON line per configuration; the per-kernel times come from a kernel trace of the same tool, one
rocprofv3 run per configuration:

    python tools/cost_lr_timing.py [C3:sad C3:ssd C5:ssd ...] [--steps N] [--warmup N] [--out FILE]
    rocprofv3 --kernel-trace --stats -d DIR/C3-sad -o run -- python tools/cost_lr_timing.py C3:sad ...
    python tools/cost_lr_timing.py --summarise DIR --out profiles/cost_lr/kernel_stats.json"""
import argparse
import csv
import json
import re
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

DEFAULT = ["C3:sad", "C3:ssd", "C5:ssd"]


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
    cfg, cost = spec.split(":")
    w, h, d, sw, mode = CONFIGS[cfg]
    left, right = make_pair(w, h, d, seed=1)
    L, R = torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda()
    plan = pipeline.StereoPlan(w, h, d, sw, mode)
    plan.reserve_cost_lr()
    c = {"sad": 1, "ssd": 2}[cost]
    web = torch.empty((1, h, w), dtype=torch.int32, device="cuda")
    web_right = torch.empty_like(web)
    rejected = torch.empty(1, dtype=torch.int32, device="cuda")
    lib, h_, ptr = pipeline.lib, plan._h, pipeline._ptr

    def cost_wta():
        pipeline.check(lib.sm_cost_wta(h_, ptr(L), ptr(R), c, 1, ptr(web), None, plan._stream()))

    def cost_wta_right():
        pipeline.check(lib.sm_cost_wta_right(h_, ptr(L), ptr(R), c, 1, ptr(web_right), None, plan._stream()))

    def cost_lr():
        pipeline.check(lib.sm_cost_lr(h_, ptr(L), ptr(R), c, 1, 0, ptr(web), None, None, ptr(rejected),
                                      plan._stream()))

    def cost_lr_right():
        pipeline.check(lib.sm_cost_lr(h_, ptr(L), ptr(R), c, 1, 0, ptr(web), None, ptr(web_right), ptr(rejected),
                                      plan._stream()))

    cost_lr()
    torch.cuda.synchronize()
    res = {"config": cfg, "cost": cost, "width": w, "height": h, "num_shifts": d, "square_width": sw, "border": mode,
           "steps": steps, "warmup": warmup}
    for name, fn in (("sm_cost_wta_ms", cost_wta), ("sm_cost_lr_ms", cost_lr),
                     ("sm_cost_lr_with_right_map_ms", cost_lr_right), ("sm_cost_wta_right_ms", cost_wta_right)):
        res[name] = round(per_step_ms(fn, steps, warmup), 4)
    res["target_ms"] = round(2 * res["sm_cost_wta_ms"] + 0.060, 4)       # cost_lr <= 2 cost_wta + 60 us per pair
    res["rejected_pixels"] = int(rejected[0])
    # k_mirror_gray reads both images and writes both mirrored ones
    res["mirror_compulsory_bytes"] = 4 * w * h
    plan.close()
    return res


def summarise(root, out):
    """kernel_stats.csv of one rocprofv3 run per configuration (ROOT/<config>-<cost>/...) -> one JSON file"""
    res = {"source": "rocprofv3 --kernel-trace --stats -d ROOT/<config>-<cost> -- python tools/cost_lr_timing.py "
                     "<config>:<cost> (one run per configuration); per-kernel dispatch durations",
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
        summarise(a.summarise, a.out or "profiles/cost_lr/kernel_stats.json")
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
