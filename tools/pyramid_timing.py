"""The half-resolution path at 4K: time per call of sm_reduce_half (both filters) and sm_upsample_double (both map
types, fill off / on) at 3840 x 2160 with device events after a warm-up, each with its ratio to the byte floor at
6.3 TB/s (reduce: source + destination; upsample: coarse map + both guides + fine map); then the half path end to end
(reduce both sides, sm_sgm_lr at 1920 x 1080 with 64 shifts and a 7 x 7 window, upsample) beside sm_sgm_lr at
3840 x 2160 with 128 shifts and a 9 x 9 window (DESIGN.md 14's C2 and C3; penalties scaled with the window as
tools/sgm_timing.py scales them), in the same run.  One JSON line per case.

    python tools/pyramid_timing.py [--steps N] [--warmup N] [--out FILE]"""
import argparse
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

W, H, D = 3840, 2160, 128
INVALID = 0.3
FLOOR_BYTES_PER_S = 6.3e12
SW_FINE, SW_COARSE = 9, 7


def sgm_args(sw):
    p1 = 10 * sw * sw // 9 + 10
    return dict(census=7, p1=p1, p2=12 * p1, paths=8)


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
    fine = pipeline.StereoPlan(W, H, D, SW_FINE, "toroidal")
    cw, ch = fine.half_shape()
    coarse = pipeline.StereoPlan(cw, ch, D // 2, SW_COARSE, "toroidal")
    left, right = (torch.from_numpy(a).cuda() for a in make_pair(W, H, D, seed=5))
    both = torch.stack([left, right]).contiguous()
    small = torch.empty((2, ch, cw), dtype=torch.uint8, device="cuda")
    weights = capi.w256(pipeline.guide_weights(8))
    h_, st = fine._h, fine._stream()
    npx, cpx = W * H, cw * ch
    common = {"width": W, "height": H, "steps": steps, "warmup": warmup}
    lines = []

    def emit(res):
        lines.append(res)
        print(json.dumps(res), flush=True)

    for name, code in pipeline.REDUCE_FILTERS.items():
        for images in (1, 2):
            us = per_step_us(lambda: check(lib.sm_reduce_half(h_, ptr(both), code, images, ptr(small), st)), steps, warmup)
            floor = images * (npx + cpx)
            emit({**common, "stage": "reduce_half", "filter": name, "images": images, "us": us, "floor_bytes": floor,
                  "over_byte_floor": round(us / (floor / FLOOR_BYTES_PER_S * 1e6), 1)})
    check(lib.sm_reduce_half(h_, ptr(both), capi.SM_REDUCE_BINOMIAL, 2, ptr(small), st))
    gen = torch.Generator(device="cuda").manual_seed(5)
    yy, xx = torch.meshgrid(torch.arange(ch, device="cuda"), torch.arange(cw, device="cuda"), indexing="ij")
    scene = 1 + (xx * (D // 4 - 4)) // cw + ((xx // 120 + yy // 68) % 3 == 0) * (D // 4) + torch.randint(0, 3, (ch, cw), generator=gen, device="cuda")
    hole = torch.rand((ch, cw), generator=gen, device="cuda") < INVALID
    for dtype, ty, name, unit in ((torch.int32, capi.SM_MAP_I32, "int32", 1), (torch.int16, capi.SM_MAP_I16, "int16", 16)):
        m = torch.where(hole, 0, scene * unit)[None].to(dtype).contiguous()
        o = torch.empty((1, H, W), dtype=dtype, device="cuda")
        for fill in (False, True):
            flags = capi.SM_UP_FILL if fill else 0
            us = per_step_us(lambda: check(lib.sm_upsample_double(h_, ptr(m), ty, ptr(left), ptr(small), weights, flags, 1,
                                                                  ptr(o), st)), steps, warmup)
            floor = cpx * m.element_size() + npx + cpx + npx * m.element_size()
            emit({**common, "stage": "upsample_double", "map": name, "fill": fill, "invalid": INVALID, "us": us,
                  "floor_bytes": floor, "over_byte_floor": round(us / (floor / FLOOR_BYTES_PER_S * 1e6), 1)})

    # the half path end to end beside the full-resolution matcher
    fine.reserve_sgm()
    coarse.reserve_sgm()
    l1, r1 = left[None].contiguous(), right[None].contiguous()
    web_f = torch.empty((1, H, W), dtype=torch.int32, device="cuda")
    web_c = torch.empty((1, ch, cw), dtype=torch.int32, device="cuda")
    up = torch.empty((1, H, W), dtype=torch.int32, device="cuda")

    def half_path():
        fine.reduce_half(both, "binomial", out=small)
        coarse.sgm_lr(small[0:1], small[1:2], web=web_c, **sgm_args(SW_COARSE))
        fine.upsample_double(web_c, l1, small[0:1], weights, fill=False, out=up)

    full_us = per_step_us(lambda: fine.sgm_lr(l1, r1, web=web_f, **sgm_args(SW_FINE)), steps, warmup)
    half_us = per_step_us(half_path, steps, warmup)
    coarse_us = per_step_us(lambda: coarse.sgm_lr(small[0:1], small[1:2], web=web_c, **sgm_args(SW_COARSE)), steps, warmup)
    torch.cuda.synchronize()
    agree = (up - web_f).abs() <= 2
    both_valid = (up != 0) & (web_f != 0)
    emit({**common, "stage": "half path", "full": {"size": [W, H], "shifts": D, "square_width": SW_FINE, **sgm_args(SW_FINE), "sgm_lr_us": full_us},
          "half": {"size": [cw, ch], "shifts": D // 2, "square_width": SW_COARSE, **sgm_args(SW_COARSE), "reduce_sgm_lr_upsample_us": half_us, "sgm_lr_alone_us": coarse_us},
          "full_over_half": round(full_us / half_us, 2),
          "valid_full": round(float((web_f != 0).float().mean()), 4), "valid_half": round(float((up != 0).float().mean()), 4),
          "within_2_where_both_valid": round(float((agree & both_valid).sum() / both_valid.sum().clamp(min=1)), 4)})
    fine.close()
    coarse.close()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="profiles/pyramid/pyramid_timing.jsonl")
    a = ap.parse_args()
    lines = measure(a.steps, a.warmup)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text("".join(json.dumps(r) + "\n" for r in lines))


if __name__ == "__main__":
    main()
