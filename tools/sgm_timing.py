"""SGM over the census data term: time per call of sm_sgm_wta (web only, and with best and sub) and sm_sgm_lr on one
plan, with device events after a warm-up, beside sm_census_wta on the same plan for scale.  One JSON line per
configuration; the per-kernel times come from a kernel trace of the same tool, one rocprofv3 run per configuration:

    python tools/sgm_timing.py [C2:8 C3:4 C3:8 C3n1:8 C5:8] [--steps N] [--warmup N] [--out FILE]
    rocprofv3 --kernel-trace --stats -d DIR/C3-8 -o run -- python tools/sgm_timing.py C3:8 ...
    python tools/sgm_timing.py --summarise DIR --out profiles/sgm/kernel_stats.json     (DIR/trace/*, DIR/pmc_*)

A configuration is <CONFIGS name of stereomatching_amd/synth.py, or C3n1 = C3 with a 1 x 1 window>:<paths>.  Census
width 7; penalties scaled with the window: p1 = 10 n^2 // 9 + 10, p2 = 12 p1 (10 and 120 at n = 1)."""
import argparse
import json
import re
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

DEFAULT = ["C2:8", "C3:4", "C3:8", "C3n1:8", "C5:8"]
BYTES_PER_PD = {4: 34, 8: 74}           # HBM bytes per (pixel, shift) of the suggested design
HBM_TBPS = 6.3


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


def config(spec):
    from stereomatching_amd.synth import CONFIGS
    name, paths = spec.split(":")
    if name.endswith("n1"):
        w, h, d, _, mode = CONFIGS[name[:-2]]
        return name, w, h, d, 1, mode, int(paths)
    w, h, d, sw, mode = CONFIGS[name]
    return name, w, h, d, sw, mode, int(paths)


def measure(spec, steps, warmup):
    import torch

    from stereomatching_amd import pipeline
    from stereomatching_amd.synth import make_pair
    cfg, w, h, d, sw, mode, paths = config(spec)
    c = 7
    p1 = 10 * sw * sw // 9 + 10
    p2 = 12 * p1
    left, right = make_pair(w, h, d, seed=1)
    L, R = torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda()
    plan = pipeline.StereoPlan(w, h, d, sw, mode)
    plan.reserve_sgm()
    web = torch.empty((1, h, w), dtype=torch.int32, device="cuda")
    best = torch.empty_like(web)
    sub = torch.empty((1, h, w), dtype=torch.int16, device="cuda")
    rejected = torch.empty(1, dtype=torch.int32, device="cuda")
    lib, h_, ptr = pipeline.lib, plan._h, pipeline._ptr

    def sgm_wta():
        pipeline.check(lib.sm_sgm_wta(h_, ptr(L), ptr(R), c, p1, p2, paths, 1, ptr(web), None, None, plan._stream()))

    def sgm_wta_all():
        pipeline.check(lib.sm_sgm_wta(h_, ptr(L), ptr(R), c, p1, p2, paths, 1, ptr(web), ptr(best), ptr(sub),
                                      plan._stream()))

    def sgm_lr():
        pipeline.check(lib.sm_sgm_lr(h_, ptr(L), ptr(R), c, p1, p2, paths, 1, 0, ptr(web), None, None, ptr(rejected),
                                     ptr(sub), plan._stream()))

    def census_wta():
        pipeline.check(lib.sm_census_wta(h_, ptr(L), ptr(R), c, 1, ptr(web), None, plan._stream()))

    sgm_lr()
    torch.cuda.synchronize()
    res = {"config": cfg, "paths": paths, "census": c, "p1": p1, "p2": p2, "width": w, "height": h, "num_shifts": d,
           "square_width": sw, "border": mode, "steps": steps, "warmup": warmup}
    for name, fn in (("sm_sgm_wta_ms", sgm_wta), ("sm_sgm_wta_best_sub_ms", sgm_wta_all), ("sm_sgm_lr_ms", sgm_lr),
                     ("sm_census_wta_ms", census_wta)):
        res[name] = round(per_step_ms(fn, steps, warmup), 3)
    floor = BYTES_PER_PD[paths] * w * h * d / (HBM_TBPS * 1e12) * 1e3
    res["floor_ms"] = round(floor, 3)
    res["target_ms"] = round(1.5 * floor, 3)
    res["sm_sgm_wta_over_floor"] = round(res["sm_sgm_wta_ms"] / floor, 2)
    res["rejected_pixels"] = int(rejected[0])
    res["pixel_shifts"] = w * h * d
    res["workspace_bytes"] = plan.workspace_bytes()
    plan.close()
    return res


def _db(d):
    import sqlite3
    dbs = sorted(Path(d).rglob("*.db"))
    return sqlite3.connect(str(dbs[-1])) if dbs else None


def _name(full):
    return re.sub(r"^void ", "", full).split("(")[0]


def summarise(root, out):
    """The rocprofv3 databases under ROOT -> one JSON file: per-kernel dispatch durations of the kernel trace of each
    configuration (ROOT/trace/<config>-<paths>/), and the per-dispatch counters of the counter runs (ROOT/pmc_*/),
    averaged per kernel and grid (the grid tells the configurations of one run apart)"""
    res = {"source": "rocprofv3 --kernel-trace --stats -d ROOT/trace/<config>-<paths> -- python tools/sgm_timing.py "
                     "<config>:<paths> --steps 2 --warmup 0 (one run per configuration); rocprofv3 --pmc <counters> "
                     "-d ROOT/pmc_<set> -- python tools/sgm_timing.py <configs> --steps 1 --warmup 0 (runs of their "
                     "own, no tracing)",
           "traces": {}, "counters": {}}
    for d in sorted(p for p in (Path(root) / "trace").iterdir() if p.is_dir()):
        c = _db(d)
        if c is None:
            continue
        kernels = {}
        for name, calls, mean, lo, tot in c.execute("select name, count(*), avg(duration), min(duration), "
                                                    "sum(duration) from kernels group by name"):
            kernels[_name(name)] = {"calls": calls, "mean_us": round(mean / 1e3, 2), "min_us": round(lo / 1e3, 2),
                                    "total_ms": round(tot / 1e6, 3)}
        res["traces"][d.name] = kernels
    for d in sorted(Path(root).glob("pmc_*")):
        c = _db(d)
        if c is None:
            continue
        acc = {}
        for name, grid, ctr, disp, val in c.execute("select kernel_name, grid_size, counter_name, dispatch_id, "
                                                    "sum(value) from counters_collection group by kernel_name, "
                                                    "grid_size, counter_name, dispatch_id"):
            if "sgm" not in name and "census" not in name:
                continue
            e = acc.setdefault(f"{_name(name)} grid {grid}", {}).setdefault(ctr, [])
            e.append(val)
        for k, ctrs in acc.items():
            row = res["counters"].setdefault(k, {})
            for ctr, vals in ctrs.items():
                row[ctr] = int(sum(vals) / len(vals))
                row["dispatches"] = max(row.get("dispatches", 0), len(vals))
    Path(out).parent.mkdir(parents=True, exist_ok=True)
    Path(out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res, indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("configs", nargs="*", default=DEFAULT)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--summarise", default=None, metavar="ROOT")
    a = ap.parse_args()
    if a.summarise:
        summarise(a.summarise, a.out or "profiles/sgm/kernel_stats.json")
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
