"""Left-right consistency check: time per step of sm_run and of sm_run_lr on one plan, with device events after a
warm-up, at the configurations of DESIGN.md section 10 (C3, C2, the reference's defaults at 4K).  One JSON line
per configuration; the per-kernel times come from a kernel trace of the same tool (rocprofv3 --kernel-trace).

    python tools/lr_timing.py [C3 C2 REF4K ...] [--steps N] [--warmup N] [--out FILE]"""
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
    ap.add_argument("configs", nargs="*", default=["C3", "C2", "REF4K"])
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []
    for cfg in a.configs:
        w, h, d, sw, mode = CONFIGS[cfg]
        left, right = make_pair(w, h, d, seed=1)
        L, R = torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda()
        plan = pipeline.StereoPlan(w, h, d, sw, mode)
        plan.prepare_threshold(0.15)
        plan.reserve_lr()
        web = torch.empty((1, h, w), dtype=torch.int32, device="cuda")
        web_right = torch.empty_like(web)
        checked = torch.empty_like(web)
        rejected = torch.empty(1, dtype=torch.int32, device="cuda")
        lib, h_, ptr = pipeline.lib, plan._h, pipeline._ptr

        def stream():
            return plan._stream()

        def run():
            pipeline.check(lib.sm_run(h_, ptr(L), ptr(R), 0.15, 1, ptr(web), None, stream()))

        def run_lr():
            pipeline.check(lib.sm_run_lr(h_, ptr(L), ptr(R), 0.15, 1, 0, ptr(web), None, None, ptr(rejected), stream()))

        def run_lr_right():
            pipeline.check(lib.sm_run_lr(h_, ptr(L), ptr(R), 0.15, 1, 0, ptr(web), None, ptr(web_right), ptr(rejected),
                                         stream()))

        def match_right():
            pipeline.check(lib.sm_match_wta_right(h_, 1, ptr(web_right), None, stream()))

        def lr_check():
            pipeline.check(lib.sm_lr_check(h_, ptr(web), ptr(web_right), 0, 1, ptr(checked), ptr(rejected), stream()))

        def lr_check_no_count():
            pipeline.check(lib.sm_lr_check(h_, ptr(web), ptr(web_right), 0, 1, ptr(checked), None, stream()))

        run()
        match_right()
        torch.cuda.synchronize()
        res = {"config": cfg, "width": w, "height": h, "num_shifts": d, "square_width": sw, "border": mode,
               "steps": a.steps, "warmup": a.warmup, "plan": plan.describe()}
        for name, fn in (("sm_run_ms", run), ("sm_run_lr_ms", run_lr), ("sm_run_lr_with_right_map_ms", run_lr_right),
                         ("sm_match_wta_right_ms", match_right), ("sm_lr_check_ms", lr_check),
                         ("sm_lr_check_without_count_ms", lr_check_no_count)):
            res[name] = round(per_step_ms(fn, a.steps, a.warmup), 4)
        res["rejected_pixels"] = int(rejected[0])
        res["check_compulsory_bytes"] = {"sm_run_lr": 12 * w * h, "sm_run_lr_with_right_map": 16 * w * h,
                                         "sm_lr_check": 12 * w * h}
        g = plan.geometry()
        res["mirror_compulsory_bytes"] = 2 * 2 * g["ext_words"] * g["ext_rows"] * 4
        print(json.dumps(res), flush=True)
        lines.append(res)
        plan.close()
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("".join(json.dumps(r) + "\n" for r in lines))


if __name__ == "__main__":
    main()
