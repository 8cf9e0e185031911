"""Cross-based matcher: time per call of sm_cross_wta at arm 4, 8 and 15 (descriptors and arms included), of
sm_cross_wta with the subpixel map, of sm_cross_lr and of sm_cross_arms (one pair: both images), with device events
after a warm-up -- and, in the same process and on the same pair, of the two matchers it stands between: sm_census_wta
at the configuration's window and sm_sgm_wta with 4 paths.  One JSON line per configuration; the counters come from a
run of their own of the same tool:

    python tools/cross_timing.py [C3:7 ...] [--steps N] [--warmup N] [--out profiles/cross/cross_timing.jsonl]
    rocprofv3 --pmc SQ_INSTS_VALU SQ_WAVE_CYCLES SQ_WAIT_INST_LDS -d DIR/pmc -- python tools/cross_timing.py C3:7 \\
        --steps 1 --warmup 0 --only-cross                                       (no tracing beside the counters)
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR/trace -- python tools/cross_timing.py C3:7 --steps 2 \\
        --warmup 0 --only-cross                                                 (a run of its own as well)
    python tools/cross_timing.py --summarise DIR --out profiles/cross/cross_pmc.json

A configuration is <CONFIGS name of stereomatching_amd/synth.py>:<census width>."""
import argparse
import csv
import json
import re
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

DEFAULT = ["C3:7"]
ARMS = (4, 8, 15)
TAU = 20


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


def measure(spec, steps, warmup, only_cross=False):
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
    plan.reserve_cross()
    if not only_cross:
        plan.reserve_sgm()
    web = torch.empty((1, h, w), dtype=torch.int32, device="cuda")
    sub = torch.empty((1, h, w), dtype=torch.int16, device="cuda")
    arms = torch.empty((2, h, w), dtype=torch.uint16, device="cuda")
    support = torch.empty((2, h, w), dtype=torch.int32, device="cuda")
    rejected = torch.empty(1, dtype=torch.int32, device="cuda")
    lib, h_, ptr = pipeline.lib, plan._h, pipeline._ptr
    p1 = 10 * sw * sw // 9 + 10
    p2 = 12 * p1

    def cross_wta(arm, s=None):
        return lambda: pipeline.check(lib.sm_cross_wta(h_, ptr(L), ptr(R), c, TAU, arm, 1, ptr(web), None, ptr(s),
                                                       plan._stream()))

    def cross_lr():
        pipeline.check(lib.sm_cross_lr(h_, ptr(L), ptr(R), c, TAU, 8, 1, 0, ptr(web), None, None, ptr(rejected), None,
                                       plan._stream()))

    def cross_arms():
        pipeline.check(lib.sm_cross_arms(h_, ptr(LR), TAU, 15, 2, ptr(arms), None, plan._stream()))

    def census_wta():
        pipeline.check(lib.sm_census_wta(h_, ptr(L), ptr(R), c, 1, ptr(web), None, plan._stream()))

    def sgm_wta():
        pipeline.check(lib.sm_sgm_wta(h_, ptr(L), ptr(R), c, p1, p2, 4, 1, ptr(web), None, None, plan._stream()))

    cross_lr()
    torch.cuda.synchronize()
    res = {"config": cfg, "census": c, "tau": TAU, "width": w, "height": h, "num_shifts": d, "square_width": sw,
           "border": mode, "steps": steps, "warmup": warmup, "rejected_pixels_arm8": int(rejected[0])}
    todo = [(f"sm_cross_wta_arm{a}_ms", cross_wta(a)) for a in ARMS]
    todo += [("sm_cross_wta_arm8_sub_ms", cross_wta(8, sub)), ("sm_cross_lr_arm8_ms", cross_lr),
             ("sm_cross_arms_ms", cross_arms)]
    if not only_cross:
        todo += [("sm_census_wta_ms", census_wta), ("sm_sgm_wta_4_paths_ms", sgm_wta)]
    for name, fn in todo:
        res[name] = round(per_step_ms(fn, steps, warmup), 4)
    # how large the supports of this pair are: the work of the refinement, and what tau lets through
    pipeline.check(lib.sm_cross_arms(h_, ptr(LR), TAU, 15, 2, ptr(arms), ptr(support), plan._stream()))
    torch.cuda.synchronize()
    res["mean_support_arm15"] = round(float(support[0].double().mean()), 1)
    res["pixel_shifts"] = w * h * d
    res["workspace_bytes"] = plan.workspace_bytes()
    plan.close()
    return res


def _name(full):
    return re.sub(r"^void ", "", full).split("(")[0]


def summarise(root, out):
    """the rocprofv3 database of the counter run under ROOT -> one JSON file: per-dispatch counters of the cross kernels,
    averaged per kernel and grid (the grid tells the arms of one run apart: 64 - 2 arm columns a workgroup)"""
    import sqlite3
    res = {"source": "rocprofv3 --pmc SQ_INSTS_VALU SQ_WAVE_CYCLES SQ_WAIT_INST_LDS -d ROOT/pmc -- python "
                     "tools/cross_timing.py C3:7 --steps 1 --warmup 0 --only-cross (a run of its own, no tracing); "
                     "per-dispatch counters averaged per kernel and grid",
           "trace_source": "rocprofv3 --kernel-trace --stats --output-format csv -d ROOT/trace -- python "
                           "tools/cross_timing.py C3:7 --steps 2 --warmup 0 --only-cross; per-kernel dispatch durations "
                           "(all arms and calls of the run together)",
           "counters": {}, "trace": {}}
    for stats in sorted(Path(root).rglob("*kernel_stats.csv")):
        with open(stats) as f:
            for row in csv.DictReader(f):
                if "cross" in row["Name"] or "census" in row["Name"]:
                    res["trace"][_name(row["Name"])] = {"calls": int(row["Calls"]),
                                                        "mean_us": round(float(row["AverageNs"]) / 1e3, 2),
                                                        "min_us": round(float(row["MinNs"]) / 1e3, 2),
                                                        "max_us": round(float(row["MaxNs"]) / 1e3, 2)}
    for db in sorted((Path(root) / "pmc").rglob("*.db")):
        con = sqlite3.connect(str(db))
        acc = {}
        for name, grid, ctr, disp, val in con.execute("select kernel_name, grid_size, counter_name, dispatch_id, "
                                                      "sum(value) from counters_collection group by kernel_name, "
                                                      "grid_size, counter_name, dispatch_id"):
            if "cross" not in name:
                continue
            acc.setdefault(f"{_name(name)} grid {grid}", {}).setdefault(ctr, []).append(val)
        for k, ctrs in acc.items():
            row = res["counters"].setdefault(k, {})
            for ctr, vals in ctrs.items():
                row[ctr] = int(sum(vals) / len(vals))
                row["dispatches"] = max(row.get("dispatches", 0), len(vals))
    Path(out).parent.mkdir(parents=True, exist_ok=True)
    Path(out).write_text(json.dumps(res, indent=1, sort_keys=True) + "\n")
    print(json.dumps(res, indent=1, sort_keys=True))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("configs", nargs="*", default=DEFAULT)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only-cross", action="store_true", help="without the census and SGM calls (the counter run)")
    ap.add_argument("--summarise", default=None, metavar="ROOT")
    a = ap.parse_args()
    if a.summarise:
        summarise(a.summarise, a.out or "profiles/cross/cross_pmc.json")
        return
    lines = []
    for spec in a.configs:
        res = measure(spec, a.steps, a.warmup, a.only_cross)
        print(json.dumps(res), flush=True)
        lines.append(res)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("".join(json.dumps(r) + "\n" for r in lines))


if __name__ == "__main__":
    main()
