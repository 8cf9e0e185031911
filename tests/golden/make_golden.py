#!/usr/bin/env python3
"""Generate tests/golden/*.npz from the UNMODIFIED compiled reference.

Run in the build container only (needs oracle/_ref, i.e. /root/reference):

    make -C oracle ref && python tests/golden/make_golden.py

Each fixture holds the uint8 input pair and the exact arrays the reference
produced for it (captured as raw u8 / i32 through oracle/capture_image.c, not
through the lossy PPM view): both edge images, score_best, web-1, web-2,
output, and the match / score_all / scores planes of a few shifts.  The
reference's NUM_SHIFTS is compile-time 30 (src/stereo.c:6), so every fixture
is at D = 30.  Fixtures are data only; no reference source is stored.
"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))

from stereomatching_amd.synth import make_pair  # noqa: E402
from tests import oracle  # noqa: E402

# name: (w, h, kind, seed, threshold, square_width, times, lines, mode)
CASES = {
    "tor_64x48_s5":    (64, 48, "scene", 11, 0.15, 5, 32, 10, "toroidal"),
    "tor_80x60_s21":   (80, 60, "scene", 12, 0.15, 21, 32, 10, "toroidal"),
    "tor_50x37_s8":    (50, 37, "scene", 13, 0.10, 8, 5, 3, "toroidal"),
    "tor_96x40_noise": (96, 40, "noise", 14, 0.30, 9, 32, 7, "toroidal"),
    "gh_64x48_s5":     (64, 48, "scene", 15, 0.15, 5, 32, 10, "ghost"),
    "gh_80x60_s21":    (80, 60, "scene", 16, 0.15, 21, 32, 10, "ghost"),
    "gh_50x37_s8":     (50, 37, "scene", 17, 0.10, 8, 5, 3, "ghost"),
    "gh_33x70_s13":    (33, 70, "scene", 18, 0.05, 13, 32, 4, "ghost"),
    "tor_40x33_s33":   (40, 33, "scene", 19, 0.15, 33, 32, 5, "toroidal"),
}
PLANE_SHIFTS = (0, 1, 7, 29)

# the reference's own smallest test pair (test/imgs/1-240x135/{a,b}.png, what test/diff.sh
# runs on) at its default parameters (src/stereo.c:7-10): the fixture stores the DECODED
# uint8 pixels (data of the reference's tests, not source) and the compiled reference's arrays
REF_PAIR = Path("/root/reference/test/imgs/1-240x135")
REF_CASES = {
    "ref_240x135_tor": (0.15, 21, 32, 10, "toroidal"),
    "ref_240x135_gh":  (0.15, 21, 32, 10, "ghost"),
}


def decode_gray_png(path):
    from PIL import Image
    im = Image.open(path)
    assert im.mode == "L", im.mode              # 8-bit gray, as read_image requires
    return np.asarray(im, np.uint8).copy()


def main():
    if not oracle.ref_available():
        sys.exit("oracle/_ref is missing: run `make -C oracle ref` where /root/reference exists")
    out_dir = Path(__file__).resolve().parent
    jobs = []
    for name, (w, h, kind, seed, thr, sw, times, lines, mode) in CASES.items():
        left, right = make_pair(w, h, oracle.REF_NUM_SHIFTS, seed=seed, kind=kind)
        jobs.append((name, left, right, thr, sw, times, lines, mode))
    if REF_PAIR.is_dir():
        left, right = decode_gray_png(REF_PAIR / "a.png"), decode_gray_png(REF_PAIR / "b.png")
        for name, (thr, sw, times, lines, mode) in REF_CASES.items():
            jobs.append((name, left, right, thr, sw, times, lines, mode))
    for name, left, right, thr, sw, times, lines, mode in jobs:
        ref = oracle.run_reference(left, right, thr, sw, times, lines, mode)
        keep = {"left": left, "right": right,
                "params": np.array([thr, sw, times, lines, oracle.MODES[mode]], np.float64)}
        for k in ("edges-1", "edges-2", "score_best-0", "web-1", "web-2", "output-0"):
            keep[k] = ref[k]
        for d in PLANE_SHIFTS:
            for k in ("matches", "score_all", "scores"):
                keep[f"{k}-{d}"] = ref[f"{k}-{d}"]
        np.savez_compressed(out_dir / f"{name}.npz", **keep)
        print(name, {k: v.shape for k, v in keep.items() if k in ("left", "web-1")})


if __name__ == "__main__" and not {"--big", "--pinned", "--step3"} & set(sys.argv):
    main()


# ---------------------------------------------------------------------------
# the reference's LARGE test pairs (test/time.sh:6-9 runs all of test/imgs): the decoded pixels
# of a pair are stored once, and of the arrays the compiled reference produces for it at its
# defaults only SHA-256 digests -- enough to pin the 4K tiling of the HIP path at D = 30 /
# S = 21 to the reference itself, bit for bit, without shipping gigabytes.
#     python tests/golden/make_golden.py --big       (minutes: the serial program at 4K)
# ---------------------------------------------------------------------------
BIG_PAIRS = {"ref_1920x1080": Path("/root/reference/test/imgs/4-1920x1080"),
             "ref_3840x2160": Path("/root/reference/test/imgs/5-3840x2160")}
BIG_KEYS = ("edges-1", "edges-2", "score_best-0", "web-1", "web-2", "output-0")


def main_big():
    import hashlib
    import json
    if not oracle.ref_available():
        sys.exit("oracle/_ref is missing: run `make -C oracle ref` where /root/reference exists")
    out_dir = Path(__file__).resolve().parent
    digests = {}
    for name, d in BIG_PAIRS.items():
        left, right = decode_gray_png(d / "a.png"), decode_gray_png(d / "b.png")
        np.savez_compressed(out_dir / f"{name}_pair.npz", left=left, right=right)
        for mode in ("toroidal", "ghost"):
            ref = oracle.run_reference(left, right, 0.15, 21, 32, 10, mode, keep=lambda k: k in BIG_KEYS)
            digests[f"{name}:{mode}"] = {
                "params": {"threshold": 0.15, "square_width": 21, "times": 32, "lines": 10, "num_shifts": 30},
                "sha256": {k: hashlib.sha256(np.ascontiguousarray(ref[k]).tobytes()).hexdigest() for k in BIG_KEYS},
                "dtype": {k: str(ref[k].dtype) for k in BIG_KEYS},
                "shape": list(ref["web-1"].shape)}
            print(name, mode, digests[f"{name}:{mode}"]["sha256"]["web-1"][:16], flush=True)
            (out_dir / "ref_big_digests.json").write_text(json.dumps(digests, indent=1) + "\n")


if __name__ == "__main__" and "--big" in sys.argv:
    main_big()


# ---------------------------------------------------------------------------
# what the compiled reference made of the cases tests/test_oracle.py and tests/test_cli_cpu.py pin
# the checker and the command-line programs to, so that those tests need no reference at run time:
#     python tests/golden/make_golden.py --pinned
#   ref_pinned_cases.json    per case of test_oracle: SHA-256 / dtype / shape of every array the
#                            reference dumps (all 30 shifts), or its exit status where it traps
#   ref_240x135_{a,b}.png    the reference's own smallest test pair, the files as they are (data)
#   ref_240x135_dumps.json   per debug program: the SHA-256 of each of the 96 PPMs its debug build
#                            writes for that pair at (0.15, 7, 32, 10), and its stdout line
# ---------------------------------------------------------------------------
# (mode, w, h, square_width, kind, threshold): the parameters of test_oracle_matches_compiled_reference
PINNED_CASES = [(mode, *c) for mode in ("toroidal", "ghost") for c in (
    (72, 41, 7, "scene", 0.15), (41, 72, 11, "noise", 0.5), (30, 30, 30, "scene", 0.0),
    (64, 32, 0, "scene", 1.0), (45, 52, 1, "scene", 0.15))]
CLI_ARGS = ("a.png", "b.png", "0.15", "7", "32", "10")


def pinned_key(mode, w, h, sw, kind, thr):
    return f"{mode}:{w}x{h}:sw{sw}:{kind}:thr{thr}"


def array_record(a):
    import hashlib
    a = np.ascontiguousarray(a)
    return {"sha256": hashlib.sha256(a.tobytes()).hexdigest(), "dtype": str(a.dtype), "shape": list(a.shape)}


# near-tie edge images (tests/edge_tie_patterns.py): the first image pair of each batch, at thresholds whose
# decisions sit on the f32 prefilter's band; only the two edge images are pinned (the contour stage may trap)
EDGE_TIE_PINNED = [(mode, 40, 31, t) for mode in ("toroidal", "ghost") for t in (0.15, 2.0 / 3.0, 1.0)]


def edge_tie_key(mode, w, h, t):
    return f"edge_ties:{mode}:{w}x{h}:thr{t!r}"


def edge_tie_images(mode, w, h, t):
    from tests import edge_tie_patterns as et
    lefts, rights = et.batch(w, h, mode, t, variants=1)
    return lefts[0], rights[0]


def edge_tie_cases():
    cases = {}
    for mode, w, h, t in EDGE_TIE_PINNED:
        left, right = edge_tie_images(mode, w, h, t)
        # repr(float) round-trips: the reference parses exactly this threshold
        ref = oracle.run_reference(left, right, t, 5, 0, 10, mode, keep=lambda s: s in ("edges-1", "edges-2"),
                                   allow_sigfpe=True)
        cases[edge_tie_key(mode, w, h, t)] = {"returncode": ref["returncode"],
                                              "arrays": {k: array_record(ref[k]) for k in ("edges-1", "edges-2")}}
    return cases


def main_pinned():
    import hashlib
    import json
    import os
    import shutil
    import subprocess
    import tempfile
    if not oracle.ref_available():
        sys.exit("oracle/_ref is missing: run `make -C oracle ref` where /root/reference exists")
    out_dir = Path(__file__).resolve().parent
    cases = {}
    for mode, w, h, sw, kind, thr in PINNED_CASES:
        left, right = make_pair(w, h, 30, seed=w * 131 + h, kind=kind)
        ref = oracle.run_reference(left, right, thr, sw, 6, 3, mode, allow_sigfpe=True)
        arrays = {k: array_record(v) for k, v in ref.items() if isinstance(v, np.ndarray)} if ref["returncode"] == 0 else {}
        cases[pinned_key(mode, w, h, sw, kind, thr)] = {"returncode": ref["returncode"], "arrays": arrays}
    # all scores equal: the reference traps on the zero contour interval after writing web and score_best
    left, right = make_pair(40, 30, 30, kind="constant")
    ref = oracle.run_reference(left, right, 0.15, 5, 0, 10, "toroidal",
                               keep=lambda s: s in ("web-1", "score_best-0"), allow_sigfpe=True)
    cases["constant:40x30:sw5"] = {"returncode": ref["returncode"],
                                   "arrays": {k: array_record(ref[k]) for k in ("web-1", "score_best-0")}}
    cases.update(edge_tie_cases())
    (out_dir / "ref_pinned_cases.json").write_text(json.dumps(cases, indent=1, sort_keys=True) + "\n")

    dumps = {}
    for side in ("a", "b"):
        shutil.copyfile(REF_PAIR / f"{side}.png", out_dir / f"ref_240x135_{side}.png")
    for variant, subdir in (("stereomatch", "ser"), ("stereomatch-ghost", "sergh")):
        with tempfile.TemporaryDirectory() as td:
            for side in ("a", "b"):
                shutil.copyfile(REF_PAIR / f"{side}.png", f"{td}/{side}.png")
            os.mkdir(f"{td}/{subdir}")
            p = subprocess.run([str(oracle.REF_DIR / f"{variant}-debug"), *CLI_ARGS], cwd=td,
                               capture_output=True, text=True, check=True)
            files = {f.name: hashlib.sha256(f.read_bytes()).hexdigest() for f in sorted(Path(td, subdir).iterdir())}
        dumps[variant] = {"subdir": subdir, "args": list(CLI_ARGS), "stdout": p.stdout, "sha256": files}
        print(variant, len(files), "files")
    (out_dir / "ref_240x135_dumps.json").write_text(json.dumps(dumps, indent=1, sort_keys=True) + "\n")


if __name__ == "__main__" and "--pinned" in sys.argv:
    main_pinned()


# ---------------------------------------------------------------------------
# step 3 on maps WITH holes, pinned to the reference's own fill_web_holes and draw_contour_map (both
# source files; oracle/ref_step3_driver.c runs them on a map of ours):
#     make -C oracle ref && python tests/golden/make_golden.py --step3
# writes tests/golden/step3/<case>.npz for every case of tests/step3_patterns.py.CASES: the input map,
# [times, lines], and per source file the map fill_web_holes returned, the contour image and the exit
# status (-8: the zero contour interval trapped; the contour is then all 0 and not compared).  The
# AddressSanitizer / UBSan build of the driver runs every case as well and must be clean: no fixture
# reads outside its map.  (A subdirectory: the *.npz of tests/golden/ itself are pipeline fixtures.)
# The files are written byte for byte the same on every run (fixed zip time stamps).
# ---------------------------------------------------------------------------
STEP3_DIR = Path(__file__).resolve().parent / "step3"
STEP3_SOURCES = {"stereo": "tor", "stereo-ghost": "gh"}      # source file -> key suffix


def save_npz_stable(path, **arrays):
    """np.savez_compressed with fixed member time stamps, so that a rerun writes identical bytes"""
    import io
    import zipfile
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for k, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(f"{k}.npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue(), compresslevel=9)


def step3_reference(web, times, lines):
    """the fixture arrays of one map: both source files, each also run under ASan / UBSan"""
    keep = {"web": web, "params": np.array([times, lines], np.int32)}
    for source, sfx in STEP3_SOURCES.items():
        r = oracle.run_step3_reference(web, times, lines, source)
        if r["returncode"] not in (0, -8) or r["filled"] is None:
            raise RuntimeError(f"{source}: driver exited {r['returncode']}: {r['stderr']}")
        s = oracle.run_step3_reference(web, times, lines, source, asan=True)
        if s["returncode"] != r["returncode"] or s["stderr"] or not np.array_equal(s["filled"], r["filled"]):
            raise RuntimeError(f"{source}: sanitizer run differs (exit {s['returncode']}):\n{s['stderr']}")
        keep[f"filled_{sfx}"] = r["filled"]
        keep[f"contour_{sfx}"] = r["contour"] if r["contour"] is not None else np.zeros(web.shape, np.uint8)
        keep[f"rc_{sfx}"] = np.array(r["returncode"], np.int32)
    return keep


def main_step3():
    from tests import step3_patterns as sp
    if not (oracle.step3_ref_available() and oracle.step3_ref_available(asan=True)):
        sys.exit("oracle/_ref/step3-ref* is missing: run `make -C oracle ref` where /root/reference exists")
    STEP3_DIR.mkdir(exist_ok=True)
    for old in STEP3_DIR.glob("*.npz"):
        if old.stem not in sp.CASES:
            old.unlink()
    for name in sp.CASES:
        web, times, lines = sp.case(name)
        keep = step3_reference(web, times, lines)
        save_npz_stable(STEP3_DIR / f"{name}.npz", **keep)
        print(name, web.shape, "holes", int((web == 0).sum()), "exit", int(keep["rc_tor"]), flush=True)


if __name__ == "__main__" and "--step3" in sys.argv:
    main_step3()
