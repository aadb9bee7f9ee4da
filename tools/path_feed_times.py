#!/usr/bin/env python3
"""Event-timed feed schedule (ppp_get_path_feed, Hertzian profile, uniform target, 8 rounds, bounds [0.25, 4], the default feed
parameters 20 / 30 / 100 / 0 / 100): the first call after a pass and its getPath on a cloud just set, which also builds what
ppp_get_path_dwell's first call builds -- per-kernel HIP-event times summed over the call's launches, the launches of each
kernel and the wall time of the call (statistics only), best of the repeats; then the same call with another accel on the same
pass, which finds the dwell rows kept and launches the feed kernels alone.  Beside it, in the same run: the first call of
ppp_get_path_dwell on a cloud just set, the call the schedule is measured against.  Workloads:
  cfg2_window   cfg 2 (1 M points, 256 slices), kd pairing, window path (walk 1, no adjustment)
  cfg2_dyn      cfg 2, walk 1 with the dynamic adjustment (the pass leaves index and normals behind)
Appends one JSON line per workload to profiles/path_feed_times.jsonl.
usage: python tools/path_feed_times.py [--reps N] [workload ...]"""
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
FEED = dict(feed=20.0, feed_max=30.0, accel=100.0, end_feed=0.0, link_feed=100.0)

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

    def fresh_pass():
        h.set_cloud(pts)                      # the cloud anew: the call builds the slab index (and the normals) again
        S = h.gen_path()
        h.get_path()
        h.kernel_times()
        return S

    S = fresh_pass()
    h.path_feed(engine.REMOVAL_HERTZ, None, ROUNDS, *BOUNDS, maps=False, **FEED)   # first call of the process: code objects, buffers
    h.enable_timing(True)
    best, best_again, best_dwell, launches, walls, walls_again, walls_dwell, stats = {}, {}, {}, {}, [], [], [], None
    for rep in range(reps):
        fresh_pass()
        t = time.perf_counter()
        st = h.path_feed(engine.REMOVAL_HERTZ, None, ROUNDS, *BOUNDS, maps=False, **FEED)[1]
        walls.append(time.perf_counter() - t)
        kt, launches = h.kernel_times(with_launches=True)
        t = time.perf_counter()
        h.path_feed(engine.REMOVAL_HERTZ, None, ROUNDS, *BOUNDS, maps=False, **dict(FEED, accel=50.0))
        walls_again.append(time.perf_counter() - t)
        kt_again = h.kernel_times()
        fresh_pass()                          # and once more for the call it is measured against
        t = time.perf_counter()
        h.path_dwell(engine.REMOVAL_HERTZ, None, ROUNDS, *BOUNDS, maps=False)
        walls_dwell.append(time.perf_counter() - t)
        for acc, k_ms in ((best, kt), (best_again, kt_again), (best_dwell, h.kernel_times())):
            for k, v in k_ms.items():
                acc[k] = min(acc.get(k, 1e30), v)
        key = tuple(st[k] for k in ("by_dwell", "by_feed_max", "by_end", "by_accel", "min_feed", "max_feed", "duration"))
        assert stats is None or stats == key      # the same bits in every repeat
        stats = key
    line = json.dumps({"tool": "path_feed_times.py", "workload": name, "config": cfg_name, "n": int(len(pts)), "S": S,
                       "window_path": bool(h.fast_path()), "profile": "hertz", "rounds": ROUNDS, "bounds": BOUNDS, "feed": FEED,
                       "W": st["W"], "slices": st["slices"], "by_dwell": st["by_dwell"], "by_feed_max": st["by_feed_max"],
                       "by_end": st["by_end"], "by_accel": st["by_accel"], "duration_s": round(st["duration"], 3),
                       "duration_nominal_s": round(st["duration_nominal"], 3), "path_length_mm": round(st["path_length"], 1),
                       "kernel_us": {k: round(v * 1e3, 1) for k, v in sorted(best.items())},
                       "kernel_launches": {k: int(v) for k, v in sorted(launches.items())},
                       "first_call_ms": round(min(walls) * 1e3, 3),
                       "other_accel_kernel_us": {k: round(v * 1e3, 1) for k, v in sorted(best_again.items())},
                       "other_accel_call_ms": round(min(walls_again) * 1e3, 3),
                       "dwell_kernel_us": {k: round(v * 1e3, 1) for k, v in sorted(best_dwell.items())},
                       "dwell_first_call_ms": round(min(walls_dwell) * 1e3, 3), "reps": reps})
    print(line)
    with open(os.path.join(ROOT, "profiles", "path_feed_times.jsonl"), "a") as f:
        f.write(line + "\n")
    h.close()
