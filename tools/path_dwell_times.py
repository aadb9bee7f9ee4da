#!/usr/bin/env python3
"""Event-timed dwell schedule (ppp_get_path_dwell, Hertzian profile, uniform target, 8 rounds, bounds [0.25, 4]): the first call
after a pass on a cloud just set, which also builds what ppp_get_path_removal's first call builds (slab index and normal field
behind a window pass, the sample table, the lengths, the unit-feed map) -- per-kernel HIP-event times summed over the call's
launches, the launches of each kernel and the wall time of the call (statistics only), best of the repeats.  Beside it, in the
same run: the first call of ppp_get_path_removal on a cloud just set, the call the schedule is measured against.  Workloads:
  cfg2_window   cfg 2 (1 M points, 256 slices), kd pairing, window path (walk 1, no adjustment)
  cfg2_dyn      cfg 2, walk 1 with the dynamic adjustment (the pass leaves index and normals behind)
Appends one JSON line per workload to profiles/path_dwell_times.jsonl.
usage: python tools/path_dwell_times.py [--reps N] [workload ...]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from polishpathplanning_amd import engine, synth  # noqa: E402

WORKLOADS = {
    "cfg2_window": ("cfg2_1m_s256", dict(walk=1)),
    "cfg2_dyn": ("cfg2_1m_s256", dict(walk=1, dynamic_adjustment=1)),
}
ROUNDS, BOUNDS = 8, (0.25, 4.0)

args = sys.argv[1:]
reps = 5
if args and args[0] == "--reps":
    reps = int(args[1])
    args = args[2:]
for name in args or list(WORKLOADS):
    cfg_name, kw = WORKLOADS[name]
    pts, cfg = synth.make_config(cfg_name)
    kw = dict(kw, tool_radius=cfg["tool_radius"])
    h = engine.Engine(0, **kw)
    h.set_cloud(pts)
    S = h.gen_path()
    h.path_dwell(engine.REMOVAL_HERTZ, None, ROUNDS, *BOUNDS, maps=False)   # first call of the process: code objects, buffers
    h.enable_timing(True)
    best, best_rem, launches, walls, walls_rem, stats = {}, {}, {}, [], [], None
    for rep in range(reps):
        h.set_cloud(pts)                      # the cloud anew: the call builds the slab index (and the normals) again
        h.gen_path()
        h.kernel_times()
        t = time.perf_counter()
        st = h.path_dwell(engine.REMOVAL_HERTZ, None, ROUNDS, *BOUNDS, maps=False)[2]
        walls.append(time.perf_counter() - t)
        kt, launches = h.kernel_times(with_launches=True)
        h.set_cloud(pts)                      # and once more for the call it is measured against
        h.gen_path()
        h.kernel_times()
        t = time.perf_counter()
        h.path_removal(engine.REMOVAL_HERTZ, maps=False)
        walls_rem.append(time.perf_counter() - t)
        for acc, k_ms in ((best, kt), (best_rem, h.kernel_times())):
            for k, v in k_ms.items():
                acc[k] = min(acc.get(k, 1e30), v)
        key = (st["at_min"], st["at_max"], st["min_dwell"], st["max_dwell"], st["residual_after"], st["time_factor"])
        assert stats is None or stats == key      # the same bits in every repeat
        stats = key
    line = json.dumps({"tool": "path_dwell_times.py", "workload": name, "config": cfg_name, "n": int(len(pts)), "S": S,
                       "window_path": bool(h.fast_path()), "profile": "hertz", "rounds": ROUNDS, "bounds": BOUNDS, "rows": st["rows"],
                       "touched": st["touched"], "at_min": st["at_min"], "at_max": st["at_max"],
                       "min_dwell": round(st["min_dwell"], 4), "max_dwell": round(st["max_dwell"], 4),
                       "residual_before": round(st["residual_before"], 4), "residual_after": round(st["residual_after"], 4),
                       "time_factor": round(st["time_factor"], 4),
                       "kernel_us": {k: round(v * 1e3, 1) for k, v in sorted(best.items())},
                       "kernel_launches": {k: int(v) for k, v in sorted(launches.items())},
                       "first_call_ms": round(min(walls) * 1e3, 3),
                       "removal_kernel_us": {k: round(v * 1e3, 1) for k, v in sorted(best_rem.items())},
                       "removal_first_call_ms": round(min(walls_rem) * 1e3, 3), "reps": reps})
    print(line)
    with open(os.path.join(ROOT, "profiles", "path_dwell_times.jsonl"), "a") as f:
        f.write(line + "\n")
    h.close()
