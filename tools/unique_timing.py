"""Match uniqueness at 4K: time per call, with device events after a warm-up, of
  sm_census_wta beside sm_census_second (against census_wta's own map),
  sm_sgm_wta beside sm_sgm_wta2,
  sm_uniqueness_filter (ratio 15, with the count) and sm_confidence,
on one 3840 x 2160 pair (make_pair) in two configurations: C3 (census width 7, a 9 x 9 window, 128 shifts, toroidal) and
C5 (256 shifts, 11 x 11, ghost).  The yardstick and the new call alternate, `--repeats` times each in the same run, so
that the yardstick's own run-to-run spread stands beside the difference.  One JSON line per configuration and stage.

    python tools/unique_timing.py [--steps N] [--sgm-steps N] [--warmup N] [--repeats N] [--out FILE]"""
import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from tools.pyramid_timing import per_step_us, sgm_args  # noqa: E402

W, H, CENSUS = 3840, 2160, 7
CONFIGS = {"C3": dict(shifts=128, square_width=9, border="toroidal"), "C5": dict(shifts=256, square_width=11, border="ghost")}


def beside(old, new, steps, warmup, repeats):
    """old and new alternating -> their times per call, the medians and the yardstick's spread"""
    a, b = [], []
    for _ in range(repeats):
        a.append(per_step_us(old, steps, warmup))
        b.append(per_step_us(new, steps, warmup))
    ma, mb = statistics.median(a), statistics.median(b)
    return {"old_us": a, "new_us": b, "old_median_us": ma, "new_median_us": mb, "new_over_old": round(mb / ma, 4),
            "old_spread": round((max(a) - min(a)) / ma, 4)}


def measure(steps, sgm_steps, warmup, repeats):
    import torch

    from stereomatching_amd import pipeline
    from stereomatching_amd.synth import make_pair
    lines = []

    def emit(res):
        lines.append(res)
        print(json.dumps(res), flush=True)

    for name, cfg in CONFIGS.items():
        D, sw = cfg["shifts"], cfg["square_width"]
        plan = pipeline.StereoPlan(W, H, D, sw, cfg["border"])
        plan.reserve_sgm()
        left, right = (torch.from_numpy(a).cuda()[None].contiguous() for a in make_pair(W, H, D, seed=5))
        new = lambda: torch.empty((1, H, W), dtype=torch.int32, device="cuda")      # noqa: E731
        web, best, web2, best2, kept, web_s, best_s = (new() for _ in range(7))
        conf = torch.empty((1, H, W), dtype=torch.uint8, device="cuda")
        common = {"config": name, "width": W, "height": H, "census": CENSUS, **cfg, "warmup": warmup, "repeats": repeats}
        plan.census_wta(left, right, CENSUS, web=web, best=best)
        res = beside(lambda: plan.census_wta(left, right, CENSUS, web=web_s, best=best_s),
                     lambda: plan.census_second(left, right, web, CENSUS, web2=web2, best2=best2), steps, warmup, repeats)
        emit({**common, "stage": "census", "old": "sm_census_wta", "new": "sm_census_second", "steps": steps, **res})
        f_us = per_step_us(lambda: plan.uniqueness_filter(web, best, best2, 15, out=kept, want_rejected=True), steps, warmup)
        c_us = per_step_us(lambda: plan.confidence(web, best, best2, out=conf), steps, warmup)
        _, rej = plan.uniqueness_filter(web, best, best2, 15, out=kept, want_rejected=True)
        emit({**common, "stage": "element-wise", "steps": steps, "uniqueness_filter_us": f_us, "confidence_us": c_us,
              "ratio": 15, "rejected_share": round(int(rej[0]) / (W * H), 4),
              "mean_confidence": round(float(conf.float().mean()), 2)})
        args = sgm_args(sw)
        res = beside(lambda: plan.sgm_wta(left, right, web=web_s, best=best_s, **args),
                     lambda: plan.sgm_wta2(left, right, web=web_s, best=best_s, web2=web2, best2=best2, **args),
                     sgm_steps, 1, repeats)
        emit({**common, "stage": "sgm", "old": "sm_sgm_wta", "new": "sm_sgm_wta2", "steps": sgm_steps, **args, **res})
        plan.close()
        del left, right, web, best, web2, best2, kept, web_s, best_s, conf
        torch.cuda.empty_cache()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--sgm-steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default="profiles/unique/unique_timing.jsonl")
    a = ap.parse_args()
    lines = measure(a.steps, a.sgm_steps, a.warmup, a.repeats)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("".join(json.dumps(r) + "\n" for r in lines))


if __name__ == "__main__":
    main()
