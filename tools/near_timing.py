"""The guided census re-search at 4K: time per call of sm_census_wta_near, sm_census_wta_near_right and
sm_census_near_lr at 3840 x 2160, 128 shifts, a 9 x 9 window, census width 7, toroidal (C3), radius 1 and 2, with three
priors -- (a) the upsampled maps of the half path (census_lr on the half plan, from make_pair), (b) a constant, (c)
white noise over 0 .. D -- beside sm_census_wta and sm_census_lr of the same plan IN THE SAME RUN, with device events
after a warm-up.  Then the half SGM path of section 20 (reduce, sm_sgm_lr at 1920 x 1080, upsample of both maps)
followed by census_near_lr(radius = 1), beside sm_sgm_lr at full size: the time of each, the share of valid pixels and
the agreement with the full-size map within 0, 1 and 2 shifts, for the upsampled map alone and for the re-searched one.
One JSON line per case.

    python tools/near_timing.py [--steps N] [--warmup N] [--out FILE]"""
import argparse
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from tools.pyramid_timing import D, H, SW_COARSE, SW_FINE, W, per_step_us, sgm_args  # noqa: E402

CENSUS = 7
SECTION_20 = {"valid_half": 0.858, "within_2_where_both_valid": 0.978}     # DESIGN.md 20, the upsampled map alone


def wanted_per_tile(prior, radius):
    """mean number of distinct shifts a 64 x 16 tile of the kernel wants (what its work is proportional to)"""
    import torch
    p = prior[0, :H // 16 * 16, :W // 64 * 64].long()
    total = torch.zeros((), dtype=torch.long, device=p.device)
    for d in range(D):
        m = (p != 0) & ((p - 1 - d).abs() <= radius)
        total += m.view(H // 16, 16, W // 64, 64).any(3).any(1).sum()
    return round(float(total) / ((H // 16) * (W // 64)), 2)


def agreement(m, full):
    both = (m != 0) & (full != 0)
    n = both.sum().clamp(min=1)
    diff = (m - full).abs()
    return {"valid": round(float((m != 0).float().mean()), 4),
            **{f"within_{k}_where_both_valid": round(float(((diff <= k) & both).sum() / n), 4) for k in (0, 1, 2)}}


def measure(steps, warmup):
    import torch

    from stereomatching_amd import pipeline
    from stereomatching_amd.synth import make_pair
    fine = pipeline.StereoPlan(W, H, D, SW_FINE, "toroidal")
    cw, ch = fine.half_shape()
    coarse = pipeline.StereoPlan(cw, ch, D // 2, SW_COARSE, "toroidal")
    fine.reserve_sgm()
    coarse.reserve_sgm()
    left, right = (torch.from_numpy(a).cuda()[None].contiguous() for a in make_pair(W, H, D, seed=5))
    both = torch.cat([left, right]).contiguous()
    weights = pipeline.guide_weights(8)
    new = lambda: torch.empty((1, H, W), dtype=torch.int32, device="cuda")      # noqa: E731
    web, best, web_right, up, up_right = new(), new(), new(), new(), new()
    web_c = torch.empty((1, ch, cw), dtype=torch.int32, device="cuda")
    web_c_right = torch.empty_like(web_c)
    small = torch.empty((2, ch, cw), dtype=torch.uint8, device="cuda")
    common = {"width": W, "height": H, "shifts": D, "square_width": SW_FINE, "census": CENSUS, "border": "toroidal",
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

    # ---- the full search of the same plan, then the re-search
    wta_us = per_step_us(lambda: fine.census_wta(left, right, CENSUS, web=web, best=best), steps, warmup)
    lr_us = per_step_us(lambda: fine.census_lr(left, right, CENSUS, max_diff=1, want_right=True, want_best=True, web=web,
                                               web_right=web_right, best=best), steps, warmup)
    emit({**common, "stage": "full search", "census_wta_us": wta_us, "census_lr_us": lr_us})
    for name, (p, p_right) in priors.items():
        for radius in (1, 2):
            near_us = per_step_us(lambda: fine.census_wta_near(left, right, p, CENSUS, radius, web=web, best=best),
                                  steps, warmup)
            right_us = per_step_us(lambda: fine.census_wta_near_right(left, right, p_right, CENSUS, radius,
                                                                      web_right=web_right, best_right=best), steps, warmup)
            near_lr_us = per_step_us(lambda: fine.census_near_lr(left, right, p, p_right, CENSUS, radius, max_diff=1,
                                                                 want_right=True, want_best=True, web=web,
                                                                 web_right=web_right, best=best), steps, warmup)
            emit({**common, "stage": "near", "prior": name, "radius": radius,
                  "wanted_shifts_per_tile": wanted_per_tile(p, radius), "near_us": near_us, "near_right_us": right_us,
                  "near_lr_us": near_lr_us, "near_over_census_wta": round(near_us / wta_us, 3),
                  "near_lr_over_census_lr": round(near_lr_us / lr_us, 3)})

    # ---- the half SGM path of section 20, then the re-search, beside the full-size SGM
    web_f = new()

    def half_path():
        fine.reduce_half(both, "binomial", out=small)
        coarse.sgm_lr(small[0:1], small[1:2], want_right=True, web=web_c, web_right=web_c_right, **sgm_args(SW_COARSE))
        upsample_both()

    def half_path_near():
        half_path()
        fine.census_near_lr(left, right, up, up_right, CENSUS, 1, max_diff=1, web=web)

    full_us = per_step_us(lambda: fine.sgm_lr(left, right, web=web_f, **sgm_args(SW_FINE)), steps, warmup)
    half_us = per_step_us(half_path, steps, warmup)
    half_near_us = per_step_us(half_path_near, steps, warmup)
    torch.cuda.synchronize()
    emit({**common, "stage": "half path then near", "sgm_lr_full_us": full_us, "half_path_us": half_us,
          "half_path_then_near_lr_us": half_near_us, "full_over_half_then_near": round(full_us / half_near_us, 2),
          "valid_full": round(float((web_f != 0).float().mean()), 4), "upsampled_alone": agreement(up, web_f),
          "re_searched": agreement(web, web_f), "section_20_upsampled_alone": SECTION_20})
    fine.close()
    coarse.close()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="profiles/near/near_timing.jsonl")
    a = ap.parse_args()
    lines = measure(a.steps, a.warmup)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("".join(json.dumps(r) + "\n" for r in lines))


if __name__ == "__main__":
    main()
