"""Subpixel refinement of the cost mode: time per call of cost_wta alone, of cost_wta + cost_refine, and of
cost_refine alone (with and without the three cost planes), on one plan, with device events after a warm-up, at
the configurations of DESIGN.md section 11 (C3 SAD, C3 SSD, C5 SSD).  One JSON line per configuration; the
per-kernel times come from a kernel trace of the same tool (rocprofv3 --kernel-trace --stats).

    python tools/subpix_timing.py [C3:sad C3:ssd C5:ssd ...] [--steps N] [--warmup N] [--out FILE]"""
import argparse
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch  # noqa: E402

from stereomatching_amd import pipeline  # noqa: E402
from stereomatching_amd.synth import CONFIGS, make_pair  # noqa: E402


def per_step_ms(fn, steps, warmup):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("configs", nargs="*", default=["C3:sad", "C3:ssd", "C5:ssd"])
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []
    for spec in a.configs:
        cfg, cost = spec.split(":")
        w, h, d, sw, mode = CONFIGS[cfg]
        left, right = make_pair(w, h, d, seed=1)
        L, R = torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda()
        plan = pipeline.StereoPlan(w, h, d, sw, mode)
        web = torch.empty((1, h, w), dtype=torch.int32, device="cuda")
        best = torch.empty_like(web)
        sub = torch.empty((1, h, w), dtype=torch.int16, device="cuda")
        costs = torch.empty((1, 3, h, w), dtype=torch.int32, device="cuda")
        lib, h_, ptr = pipeline.lib, plan._h, pipeline._ptr
        c = {"sad": 1, "ssd": 2}[cost]

        def wta():
            pipeline.check(lib.sm_cost_wta(h_, ptr(L), ptr(R), c, 1, ptr(web), ptr(best), plan._stream()))

        def refine():
            pipeline.check(lib.sm_cost_refine(h_, ptr(L), ptr(R), c, 1, ptr(web), ptr(sub), None, plan._stream()))

        def refine_costs():
            pipeline.check(lib.sm_cost_refine(h_, ptr(L), ptr(R), c, 1, ptr(web), ptr(sub), ptr(costs),
                                              plan._stream()))

        def both():
            wta()
            refine()

        wta()
        torch.cuda.synchronize()
        inner = ((web >= 2) & (web <= d - 1)).float().mean().item()
        res = {"config": cfg, "cost": cost, "width": w, "height": h, "num_shifts": d, "square_width": sw,
               "border": mode, "steps": a.steps, "warmup": a.warmup, "plan": plan.describe()}
        for name, fn in (("cost_wta_ms", wta), ("cost_wta_plus_refine_ms", both), ("cost_refine_ms", refine),
                         ("cost_refine_with_costs_ms", refine_costs)):
            res[name] = round(per_step_ms(fn, a.steps, a.warmup), 4)
        res["pixels_with_both_neighbours"] = round(inner, 4)
        # gray pair 2 B, web 4 B and sub 2 B per pixel (+ 12 B with the cost planes)
        res["refine_compulsory_bytes"] = {"cost_refine": 8 * w * h, "cost_refine_with_costs": 20 * w * h}
        print(json.dumps(res), flush=True)
        lines.append(res)
        plan.close()
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("".join(json.dumps(r) + "\n" for r in lines))


if __name__ == "__main__":
    main()
