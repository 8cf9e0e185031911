"""Record what the plans of tests/plan_geometry_cases.py come out as on this device:

    python tools/record_plan_geometry.py --commit <id> [--out tests/golden/plan_geometry_mi355x.json.gz]

Every field of plan.geometry(), plan.describe() and workspace_bytes(), with the device's CU count and the commit
that was built.  Public API only, so it runs on any commit; tests/test_plan_geometry_gpu.py compares later commits
with the file.  The file is a reference: record it BEFORE touching planning code, never from the code under test."""
import argparse
import gzip
import json
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def snapshot(case):
    from stereomatching_amd import pipeline
    w, h, d, s, border, pairs, opt = case
    plan = pipeline.StereoPlan(w, h, d, s, border, max_pairs=pairs, options=opt or None)
    try:
        return {"geometry": plan.geometry(), "describe": plan.describe(), "workspace_bytes": plan.workspace_bytes()}
    finally:
        plan.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", default=None, help="id of the commit that is built (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=str(ROOT / "tests" / "golden" / "plan_geometry_mi355x.json.gz"))
    args = ap.parse_args()
    import torch
    from tests import plan_geometry_cases as pc
    commit = args.commit or subprocess.check_output(["git", "-C", str(ROOT), "rev-parse", "HEAD"], text=True).strip()
    prop = torch.cuda.get_device_properties(0)
    plans = {pc.key(c): snapshot(c) for c in pc.cases()}
    doc = {"commit": commit, "device": prop.name, "compute_units": prop.multi_processor_count, "plans": plans}
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    text = (json.dumps(doc, separators=(",", ":"), sort_keys=True) + "\n").encode()
    with open(args.out, "wb") as f, gzip.GzipFile(filename="", mode="wb", fileobj=f, compresslevel=9, mtime=0) as z:
        z.write(text)             # (compact JSON, gzipped without a time stamp: the same plans give the same file)
    print(f"recorded {len(plans)} plans at {commit} on {prop.name} ({prop.multi_processor_count} CUs) -> {args.out}")


if __name__ == "__main__":
    main()
