#!/usr/bin/env python3
"""Event-timed coverage call (ppp_get_coverage) after a contact pass with the dynamic adjustment: per-kernel HIP-event times of
its two launches and the wall time of the call (counts only, and with the flags copied to the host), best of the repeats.
usage: python tools/coverage_times.py [--reps N] [config ...]      (default cfg2_1m_s256: walk 3, brute pairing, k = 10)"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from polishpathplanning_amd import engine, synth  # noqa: E402

args = sys.argv[1:]
reps = 5
if args and args[0] == "--reps":
    reps = int(args[1])
    args = args[2:]
for name in args or ["cfg2_1m_s256"]:
    pts, cfg = synth.make_config(name)
    e = engine.Engine(0, tool_radius=cfg["tool_radius"], walk=3, pairing=1, curvature_k=10, depth=0.005, dynamic_adjustment=1)
    e.set_cloud(pts)
    S = e.gen_path()
    e.coverage(flags=False)                       # first call of the process: code objects, buffers
    e.enable_timing(True)
    best = {}
    walls, walls_flags = [], []
    covered = None
    for rep in range(reps):
        e.gen_path()                               # a new pass: the next call computes again
        e.kernel_times()
        t = time.perf_counter()
        _, c = e.coverage(flags=False)
        walls.append(time.perf_counter() - t)
        kt = e.kernel_times()
        for k in ("k_cov_balls", "k_cov_count"):
            best[k] = min(best.get(k, 1e30), kt.get(k, 0.0))
        e.gen_path()
        t = time.perf_counter()
        flags, c2 = e.coverage()
        walls_flags.append(time.perf_counter() - t)
        e.kernel_times()
        assert c == c2 and (covered is None or c == covered)
        covered = c
    print(json.dumps({"config": name, "n": int(len(pts)), "S": S, "covered": covered, "rate": covered / len(pts),
                      "kernel_us": {k: round(v * 1e3, 1) for k, v in best.items()},
                      "call_ms_counts_only": round(min(walls) * 1e3, 3), "call_ms_with_flags": round(min(walls_flags) * 1e3, 3),
                      "reps": reps}))
    e.close()
