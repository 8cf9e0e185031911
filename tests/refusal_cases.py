"""Bad calls of the eleven left / right / checked entry points of the cost modes (csrc/sm_entry.h), as a table: what
each is refused with is recorded once from the build before the entries shared a driver
(tests/golden/entry_refusals_parent.json, by tools/record_refusals.py) and replayed by tests/test_entry_refusals_gpu.py.
The first failing check decides the message, so the cases that break two rules at once pin the ORDER of the checks.

A case is (name, entry, arguments); an argument is an int or the name of a pointer: a plan ("plan": 64 x 32, 16 shifts,
window 5, toroidal, max_pairs 2; "plan27" / "plan513": a 27 x 27 window / 513 shifts, beyond every mode's reach), "st"
(the stream), "NULL", or a buffer, optionally "+ bytes" into it.  All buffers lie 32 KiB apart in one arena of 1 MiB, so
a map of two pairs (16 KiB) written from any of them would stay inside it -- though no case gets as far as a launch."""

SLOT = 32 * 1024
ARENA_BYTES = 1024 * 1024
BUFFERS = ("left", "right", "prior", "prior_right", "web", "best", "web_right", "sub", "rejected")
PLANS = {"plan": (64, 32, 16, 5, 2), "plan27": (64, 32, 16, 27, 1), "plan513": (64, 32, 513, 5, 1)}   # w, h, d, sw, max_pairs

# entry -> its parameters in order (without the stream, which is last everywhere)
_IMG = ("plan", "left", "right")
ENTRIES = {
    "sm_census_wta": _IMG + ("census", "pairs", "web", "best"),
    "sm_census_wta_right": _IMG + ("census", "pairs", "web", "best"),
    "sm_census_lr": _IMG + ("census", "pairs", "max_diff", "web", "best", "web_right", "rejected"),
    "sm_census_wta_near": _IMG + ("census", "pairs", "prior", "radius", "web", "best"),
    "sm_census_wta_near_right": _IMG + ("census", "pairs", "prior", "radius", "web", "best"),
    "sm_census_near_lr": _IMG + ("census", "pairs", "prior", "prior_right", "radius", "max_diff", "web", "best",
                                 "web_right", "rejected"),
    "sm_sgm_wta": _IMG + ("census", "p1", "p2", "paths", "pairs", "web", "best", "sub"),
    "sm_sgm_wta_right": _IMG + ("census", "p1", "p2", "paths", "pairs", "web", "best"),
    "sm_sgm_lr": _IMG + ("census", "p1", "p2", "paths", "pairs", "max_diff", "web", "best", "web_right", "rejected", "sub"),
    "sm_cost_wta_right": _IMG + ("cost", "pairs", "web", "best"),
    "sm_cost_lr": _IMG + ("cost", "pairs", "max_diff", "web", "best", "web_right", "rejected"),
}
GOOD = {"plan": "plan", "census": 5, "cost": 1, "p1": 10, "p2": 120, "paths": 8, "pairs": 2, "radius": 1, "max_diff": 0,
        **{b: b for b in BUFFERS}}
REQUIRED = ("plan", "left", "right", "prior", "prior_right", "web")      # NULL is refused; the other pointers may be NULL
OUTPUTS = ("web", "best", "web_right", "sub", "rejected")
# what makes one parameter bad, by the rule it breaks
BAD = {"pairs 0": {"pairs": 0}, "pairs 3": {"pairs": 3}, "census 4": {"census": 4}, "cost 3": {"cost": 3},
       "paths 5": {"paths": 5}, "p1 -1": {"p1": -1}, "p2 below p1": {"p2": 5}, "p2 40000": {"p2": 40000},
       "radius 0": {"radius": 0}, "radius 5": {"radius": 5}, "max_diff -1": {"max_diff": -1},
       "window 27": {"plan": "plan27", "pairs": 1}, "513 shifts": {"plan": "plan513", "pairs": 1}}


def _inside(a, b):
    """parameter b placed a few bytes into buffer a (2 for the int16 map: it stays aligned for its type)"""
    return {b: f"{a}+{8 if 'rejected' in (a, b) else 2 if 'sub' in (a, b) else 4}"}


def _double(params):
    """calls that break two rules: (name, overrides), the rules in the order the entries check them"""
    scalar = "cost 3" if "cost" in params else "census 4"
    yield "left NULL + pairs 3", {"left": "NULL", "pairs": 3}
    yield "web NULL + plan NULL", {"web": "NULL", "plan": "NULL"}
    yield f"web NULL + {scalar}", {"web": "NULL", **BAD[scalar]}
    yield f"{scalar} + plan NULL", {**BAD[scalar], "plan": "NULL"}
    yield "pairs 3 + best in web", {"pairs": 3, **_inside("web", "best")}
    yield "best in web + window 27", {**_inside("web", "best"), **BAD["window 27"]}
    yield f"{scalar} + 513 shifts", {**BAD[scalar], **BAD["513 shifts"]}
    if "max_diff" in params:
        yield f"max_diff -1 + {scalar}", {"max_diff": -1, **BAD[scalar]}
        yield "web NULL + max_diff -1", {"web": "NULL", "max_diff": -1}
        yield "best in web + rejected in web", {**_inside("web", "best"), **_inside("web", "rejected")}
        yield "rejected in web_right + window 27", {**_inside("web_right", "rejected"), **BAD["window 27"]}
    if "paths" in params:
        yield "census 4 + paths 5", {"census": 4, "paths": 5}
        yield "paths 5 + p1 -1", {"paths": 5, "p1": -1}
        yield "p2 40000 + pairs 3", {"p2": 40000, "pairs": 3}
    if "radius" in params:
        yield "radius 0 + census 4", {"radius": 0, "census": 4}
        yield "radius 5 + plan NULL", {"radius": 5, "plan": "NULL"}
        yield "prior NULL + web NULL", {"prior": "NULL", "web": "NULL"}
        yield "left NULL + prior NULL", {"left": "NULL", "prior": "NULL"}
        yield "best in web + web over left", {"web": "left", "best": "left+4"}
        yield "web over left + best over prior", {"web": "left", "best": "prior"}
        yield "web over prior + window 27", {"web": "prior", **BAD["window 27"]}
    if "prior_right" in params:
        yield "web_right over prior + rejected over right", {"web_right": "prior", "rejected": "right"}
        yield "max_diff -1 + radius 0", {"max_diff": -1, "radius": 0}


def _cases():
    for entry, params in ENTRIES.items():
        single = {}
        for p in params:
            if p in REQUIRED:
                single[f"{p} NULL"] = {p: "NULL"}
        for rule, over in BAD.items():
            if all(k in params for k in over):
                single[rule] = over
        outs = [p for p in OUTPUTS if p in params]
        for i, a in enumerate(outs):
            for b in outs[i + 1:]:
                single[f"{b} in {a}"] = _inside(a, b)
        if "prior" in params:
            for o in outs:
                for src in ("left", "right", "prior", "prior_right"):
                    if src in params:
                        single[f"{o} over {src}"] = {o: src}
        for name, over in list(single.items()) + list(_double(params)):
            yield f"{entry}: {name}", entry, tuple({**GOOD, **over}[p] for p in params) + ("st",)


CASES = list(_cases())


def replay(pipeline):
    """every case on the loaded library -> {name: [rc, message, workspace bytes before, after]}; needs a device"""
    import ctypes as C

    import torch
    lib = pipeline.lib
    arena = torch.zeros(ARENA_BYTES, dtype=torch.uint8, device="cuda")
    plans = {k: pipeline.StereoPlan(w, h, d, sw, "toroidal", max_pairs=mp) for k, (w, h, d, sw, mp) in PLANS.items()}
    st = torch.cuda.current_stream().cuda_stream

    def value(a):
        if isinstance(a, int):
            return a
        if a in plans:
            return plans[a]._h
        if a in ("NULL", "st"):
            return C.c_void_p(st) if a == "st" else None
        buf, _, off = a.partition("+")
        return C.c_void_p(arena.data_ptr() + SLOT * BUFFERS.index(buf) + int(off or 0))
    res = {}
    for name, entry, args in CASES:
        plan = plans.get(args[0])
        before = plan.workspace_bytes() if plan else 0
        rc = getattr(lib, entry)(*map(value, args))
        msg = lib.sm_last_error().decode(errors="replace") if rc else ""
        res[name] = [rc, msg, before, plan.workspace_bytes() if plan else 0]
    torch.cuda.synchronize()
    for p in plans.values():
        p.close()
    return res
