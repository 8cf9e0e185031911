"""Banded SGM at 4K: time per call of sm_sgm_wta_near and sm_sgm_near_lr at 3840 x 2160, 128 shifts, a
9 x 9 window, census width 7, toroidal (C3), radius 1 and 2, with the three priors of tools/near_timing.py -- (a) the
upsampled maps of the half path (census_lr on the half plan, from make_pair), (b) a constant, (c) white noise over
0 .. D -- beside sm_sgm_wta and sm_sgm_lr of the same plan IN THE SAME RUN (the yardstick: full-size SGM), with device
events after a warm-up.  Then the whole chain -- reduce, sm_sgm_lr at 1920 x 1080, upsample of both maps,
sm_sgm_near_lr(radius = 1) -- beside sm_sgm_lr at full size and beside the same chain ending in sm_census_near_lr
(section 21): the time of each, the share of valid pixels and the agreement with the full-size map within 0, 1 and 2
shifts.  One JSON line per case.

    python tools/sgm_near_timing.py [--steps N] [--warmup N] [--out FILE]
    rocprofv3 --kernel-trace --stats -d ROOT -- python tools/sgm_near_timing.py --trace --steps 3 --warmup 1
    python tools/sgm_near_timing.py --summarise ROOT --out profiles/sgm_near/kernel_stats.json"""
import argparse
import json
import re
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from tools.near_timing import CENSUS, agreement, wanted_per_tile  # noqa: E402
from tools.pyramid_timing import D, H, SW_COARSE, SW_FINE, W, per_step_us, sgm_args  # noqa: E402


def setup():
    import torch

    from stereomatching_amd import pipeline
    from stereomatching_amd.synth import make_pair
    fine = pipeline.StereoPlan(W, H, D, SW_FINE, "toroidal")
    cw, ch = fine.half_shape()
    coarse = pipeline.StereoPlan(cw, ch, D // 2, SW_COARSE, "toroidal")
    fine.reserve_sgm_near()
    coarse.reserve_sgm()
    left, right = (torch.from_numpy(a).cuda()[None].contiguous() for a in make_pair(W, H, D, seed=5))
    return torch, pipeline, fine, coarse, left, right


def measure(steps, warmup, trace=False):
    torch, pipeline, fine, coarse, left, right = setup()
    cw, ch = fine.half_shape()
    both = torch.cat([left, right]).contiguous()
    weights = pipeline.guide_weights(8)
    new = lambda: torch.empty((1, H, W), dtype=torch.int32, device="cuda")      # noqa: E731
    web, best, web_right, up, up_right = new(), new(), new(), new(), new()
    sub = torch.empty((1, H, W), dtype=torch.int16, device="cuda")
    web_c = torch.empty((1, ch, cw), dtype=torch.int32, device="cuda")
    web_c_right = torch.empty_like(web_c)
    small = torch.empty((2, ch, cw), dtype=torch.uint8, device="cuda")
    args = sgm_args(SW_FINE)
    common = {"width": W, "height": H, "shifts": D, "square_width": SW_FINE, "border": "toroidal", **args,
              "steps": steps, "warmup": warmup}
    lines = []

    def emit(res):
        lines.append(res)
        print(json.dumps(res), flush=True)

    def upsample_both():
        fine.upsample_double(web_c, left, small[0:1], weights, fill=False, out=up)
        fine.upsample_double(web_c_right, right, small[1:2], weights, fill=False, out=up_right)

    # ---- the priors
    fine.reduce_half(both, "binomial", out=small)
    coarse.census_lr(small[0:1], small[1:2], CENSUS, max_diff=1, want_right=True, web=web_c, web_right=web_c_right)
    upsample_both()
    gen = torch.Generator(device="cuda").manual_seed(5)
    priors = {"upsampled": (up.clone(), up_right.clone()),
              "constant": (torch.full_like(up, D // 2), torch.full_like(up, D // 2)),
              "noise": tuple(torch.randint(0, D + 1, (1, H, W), generator=gen, device="cuda", dtype=torch.int32)
                             for _ in range(2))}
    if trace:
        # the kernel trace's run: one prior, one radius, the left pass only
        p = priors["upsampled"][0]
        per_step_us(lambda: fine.sgm_wta_near(left, right, p, radius=1, web=web, best=best, want_sub=True, sub=sub, **args),
                    steps, warmup)
        fine.close()
        coarse.close()
        return lines

    # ---- full-size SGM of the same plan (the parent's kernels), then the banded passes
    fine.reserve_sgm()
    wta_us = per_step_us(lambda: fine.sgm_wta(left, right, web=web, best=best, want_sub=True, sub=sub, **args), steps, warmup)
    lr_us = per_step_us(lambda: fine.sgm_lr(left, right, max_diff=1, want_right=True, want_best=True, want_sub=True, web=web,
                                            web_right=web_right, best=best, sub=sub, **args), steps, warmup)
    emit({**common, "stage": "full size", "sgm_wta_us": wta_us, "sgm_lr_us": lr_us})
    for name, (p, p_right) in priors.items():
        for radius in (1, 2):
            near_us = per_step_us(lambda: fine.sgm_wta_near(left, right, p, radius=radius, web=web, best=best, want_sub=True,
                                                            sub=sub, **args), steps, warmup)
            near_lr_us = per_step_us(lambda: fine.sgm_near_lr(left, right, p, p_right, radius=radius, max_diff=1,
                                                              want_right=True, want_best=True, want_sub=True, web=web,
                                                              web_right=web_right, best=best, sub=sub, **args),
                                     steps, warmup)
            emit({**common, "stage": "near", "prior": name, "radius": radius,
                  "wanted_shifts_per_tile": wanted_per_tile(p, radius), "sgm_wta_near_us": near_us,
                  "sgm_near_lr_us": near_lr_us, "near_over_sgm_wta": round(near_us / wta_us, 3),
                  "near_lr_over_sgm_lr": round(near_lr_us / lr_us, 3)})

    # ---- the whole chain beside full-size SGM, and beside the chain that ends in the census re-search
    web_f, web_n = new(), new()

    def half_path():
        fine.reduce_half(both, "binomial", out=small)
        coarse.sgm_lr(small[0:1], small[1:2], want_right=True, web=web_c, web_right=web_c_right, **sgm_args(SW_COARSE))
        upsample_both()

    def chain():
        half_path()
        fine.sgm_near_lr(left, right, up, up_right, radius=1, max_diff=1, web=web, **args)

    def chain_census():
        half_path()
        fine.census_near_lr(left, right, up, up_right, CENSUS, 1, max_diff=1, web=web_n)

    full_us = per_step_us(lambda: fine.sgm_lr(left, right, max_diff=1, web=web_f, **args), steps, warmup)
    half_us = per_step_us(half_path, steps, warmup)
    chain_us = per_step_us(chain, steps, warmup)
    chain_census_us = per_step_us(chain_census, steps, warmup)
    torch.cuda.synchronize()
    emit({**common, "stage": "half path then sgm near", "sgm_lr_full_us": full_us, "half_path_us": half_us,
          "chain_us": chain_us, "chain_with_census_near_us": chain_census_us,
          "full_over_chain": round(full_us / chain_us, 2), "valid_full": round(float((web_f != 0).float().mean()), 4),
          "upsampled_alone": agreement(up, web_f), "census_near": agreement(web_n, web_f),
          "sgm_near": agreement(web, web_f)})
    fine.close()
    coarse.close()
    return lines


def summarise(root, out):
    """the rocprofv3 database under ROOT -> per-kernel dispatch durations of the banded pass's kernels"""
    import sqlite3
    dbs = sorted(Path(root).rglob("*.db"))
    res = {"source": "rocprofv3 --kernel-trace --stats -d ROOT -- python tools/sgm_near_timing.py --trace --steps 3 "
                     "--warmup 1 (a run of its own: 4 calls of sgm_wta_near, prior (a), radius 1, C3; the banded "
                     "pass's kernels only: the descriptor kernel also runs on the half plan while the prior is made)",
           "kernels": {}}
    if dbs:
        c = sqlite3.connect(str(dbs[-1]))
        for name, calls, mean, lo, hi in c.execute("select name, count(*), avg(duration), min(duration), max(duration) "
                                                   "from kernels group by name"):
            short = re.sub(r"^void ", "", name).split("(")[0]
            if re.search(r"k_sgm_near", short):
                res["kernels"][short] = {"calls": calls, "mean_us": round(mean / 1e3, 2), "min_us": round(lo / 1e3, 2),
                                         "max_us": round(hi / 1e3, 2)}
    Path(out).parent.mkdir(parents=True, exist_ok=True)
    Path(out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res, indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="profiles/sgm_near/sgm_near_timing.jsonl")
    ap.add_argument("--trace", action="store_true", help="only sgm_wta_near on prior (a), radius 1: for a kernel trace")
    ap.add_argument("--summarise", default=None, metavar="ROOT")
    a = ap.parse_args()
    if a.summarise:
        summarise(a.summarise, a.out if a.out.endswith(".json") else "profiles/sgm_near/kernel_stats.json")
        return
    lines = measure(a.steps, a.warmup, a.trace)
    if not a.trace:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("".join(json.dumps(r) + "\n" for r in lines))


if __name__ == "__main__":
    main()
