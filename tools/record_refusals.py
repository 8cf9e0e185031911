"""Record what the cost modes' entry points refuse: every bad call of tests/refusal_cases.py against the loaded
library (SM_HIP_LIB selects the build), as {case: [rc, message]} in JSON.  Needs a device; launches no kernel.

    SM_HIP_LIB=/path/to/libstereo_hip.so python tools/record_refusals.py [--out FILE]"""
import argparse
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="tests/golden/entry_refusals_parent.json")
    a = ap.parse_args()
    from stereomatching_amd import pipeline
    from tests import refusal_cases
    res = refusal_cases.replay(pipeline)
    accepted = [n for n, v in res.items() if v[0] == 0]
    grew = [n for n, v in res.items() if v[2] != v[3]]
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps({n: v[:2] for n, v in res.items()}, indent=0, sort_keys=True) + "\n")
    print(f"{len(res)} cases from {pipeline.capi.LIB_PATH}; accepted: {accepted}; workspace grew: {grew}")
    return 1 if accepted or grew else 0


if __name__ == "__main__":
    sys.exit(main())
