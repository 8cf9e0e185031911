"""SGM's left-right check from one aggregated volume: time per call of sm_sgm_wta, sm_sgm_lr,
sm_sgm_wta_both and sm_sgm_lr_single on one plan IN ONE PROCESS, the four calls alternating round by round, with device
events after a warm-up round.  The configurations and penalties are tools/sgm_timing.py's.  One JSON line per
configuration, with (for reading only) the share of pixels where the single-volume right map differs from
sm_sgm_wta_right's and the rejection counts of the two checked maps.  The per-kernel times come from kernel traces of the
same tool, each in a run of its own:

    python tools/sgm_single_timing.py [C2:8 C3:4 C3:8 C5:8] [--steps N] [--warmup N] [--out FILE]
    rocprofv3 --kernel-trace --stats -d ROOT/<label> -- python tools/sgm_single_timing.py C3:8 --steps 2 --warmup 1
    python tools/sgm_single_timing.py --summarise ROOT --out profiles/sgm_single/kernel_stats.json

The sweep of the kernel's segment length (SGB_X = SGB_XK * K of sm_sgm_both.hip; profiles/sgm_single/x_sweep.json) is
the same trace taken with builds of the library that differ in that length only (-DSGB_XK=N), loaded through
SM_HIP_LIB, one label per build."""
import argparse
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from tools.sgm_timing import HBM_TBPS, _db, _name, config  # noqa: E402

DEFAULT = ["C2:8", "C3:4", "C3:8", "C5:8"]


def segment(d):
    """SGB_X of sm_sgm_both.hip, the right pixels a wave owns: 4 Dp (for the byte floor only)"""
    return 4 * (64 if d <= 64 else 128 if d <= 128 else 256)


def alternating_ms(fns, steps, warmup):
    """{name: mean ms per call}, the calls taken in turn within each round"""
    import torch
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    marks = []
    for _ in range(steps):
        for name, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            marks.append((name, e0, e1))
    torch.cuda.synchronize()
    total = dict.fromkeys(fns, 0.0)
    for name, e0, e1 in marks:
        total[name] += e0.elapsed_time(e1)
    return {name: round(t / steps, 3) for name, t in total.items()}


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
    new = lambda: torch.empty((1, h, w), dtype=torch.int32, device="cuda")      # noqa: E731
    web, web_right, web_single, right_single = new(), new(), new(), new()
    sub = torch.empty((1, h, w), dtype=torch.int16, device="cuda")
    rejected, rejected_single = (torch.empty(1, dtype=torch.int32, device="cuda") for _ in range(2))
    lib, h_, ptr, st = pipeline.lib, plan._h, pipeline._ptr, plan._stream()
    fns = {
        "sm_sgm_wta_ms": lambda: pipeline.check(lib.sm_sgm_wta(h_, ptr(L), ptr(R), c, p1, p2, paths, 1, ptr(web), None,
                                                               None, st)),
        "sm_sgm_lr_ms": lambda: pipeline.check(lib.sm_sgm_lr(h_, ptr(L), ptr(R), c, p1, p2, paths, 1, 0, ptr(web), None,
                                                             ptr(web_right), ptr(rejected), ptr(sub), st)),
        "sm_sgm_wta_both_ms": lambda: pipeline.check(lib.sm_sgm_wta_both(h_, ptr(L), ptr(R), c, p1, p2, paths, 1,
                                                                         ptr(web_single), None, None, ptr(right_single),
                                                                         None, st)),
        "sm_sgm_lr_single_ms": lambda: pipeline.check(lib.sm_sgm_lr_single(h_, ptr(L), ptr(R), c, p1, p2, paths, 1, 0,
                                                                           ptr(web_single), None, ptr(right_single),
                                                                           ptr(rejected_single), ptr(sub), st)),
    }
    res = {"config": cfg, "paths": paths, "census": c, "p1": p1, "p2": p2, "width": w, "height": h, "num_shifts": d,
           "square_width": sw, "border": mode, "steps": steps, "warmup": warmup}
    res.update(alternating_ms(fns, steps, warmup))
    res["lr_single_over_lr"] = round(res["sm_sgm_lr_single_ms"] / res["sm_sgm_lr_ms"], 3)
    res["wta_both_minus_wta_ms"] = round(res["sm_sgm_wta_both_ms"] - res["sm_sgm_wta_ms"], 3)
    # k_sgm_both reads S once plus the warm-up columns; the last direction stores S where SGM_LAST does not (+ 4 B)
    read_floor = 4 * (1 + (d - 1) / segment(d)) * w * h * d / (HBM_TBPS * 1e12) * 1e3
    res["k_sgm_both_floor_ms"] = round(read_floor, 3)
    res["k_sgm_both_target_ms"] = round(1.5 * read_floor, 3)
    res["added_floor_ms"] = round(read_floor + 4 * w * h * d / (HBM_TBPS * 1e12) * 1e3, 3)
    # for reading only: the two right maps are different definitions
    fns["sm_sgm_lr_ms"]()
    fns["sm_sgm_lr_single_ms"]()
    torch.cuda.synchronize()
    res["right_maps_differ_share"] = round(float((web_right != right_single).float().mean()), 4)
    res["checked_maps_differ_share"] = round(float((web != web_single).float().mean()), 4)
    res["rejected_pixels_lr"] = int(rejected[0])
    res["rejected_pixels_lr_single"] = int(rejected_single[0])
    res["workspace_bytes"] = plan.workspace_bytes()
    plan.close()
    return res


def summarise(root, out):
    """the rocprofv3 databases under ROOT/<label>/ -> one JSON file: per label, the dispatch durations of the SGM kernels"""
    res = {"source": "rocprofv3 --kernel-trace --stats -d ROOT/<label> -- python tools/sgm_single_timing.py <config> "
                     "--steps 2 --warmup 1 (one run per label, no counters)",
           "traces": {}}
    for d in sorted(p for p in Path(root).iterdir() if p.is_dir()):
        c = _db(d)
        if c is None:
            continue
        kernels = {}
        # (C2, C3 and C5 differ in the shifts a lane holds and in the border: the kernels' names tell them apart)
        for name, calls, mean, lo in c.execute("select name, count(*), avg(duration), min(duration) from kernels "
                                               "group by name"):
            if "sgm" in name:
                kernels[_name(name)] = {"calls": calls, "mean_us": round(mean / 1e3, 2), "min_us": round(lo / 1e3, 2)}
        # the last direction as SGM_MID: the dispatch in front of each k_sgm_both (beside k_sgm_path<K, 2>, SGM_LAST)
        try:
            rows = list(c.execute("select name, duration from kernels order by start"))
        except Exception:                                         # a trace database without start times
            rows = []
        for (prev, dur), (name, _) in zip(rows, rows[1:]):
            if "k_sgm_both" in name and "k_sgm_path" in prev:
                e = kernels.setdefault(_name(prev) + " as the last direction", {"calls": 0, "mean_us": 0.0})
                e["mean_us"] = round((e["mean_us"] * e["calls"] + dur / 1e3) / (e["calls"] + 1), 2)
                e["calls"] += 1
        res["traces"][d.name] = kernels
    Path(out).parent.mkdir(parents=True, exist_ok=True)
    Path(out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res, indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("configs", nargs="*", default=DEFAULT)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    ap.add_argument("--summarise", default=None, metavar="ROOT")
    a = ap.parse_args()
    if a.summarise:
        summarise(a.summarise, a.out or "profiles/sgm_single/kernel_stats.json")
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
