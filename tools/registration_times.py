#!/usr/bin/env python3
"""Event-timed registration (ppp_register): cfg 2 (1 M points) moved by a small known motion -- 0.2 degrees about every axis
through the cloud's centre and (0.3, -0.2, 0.25) mm -- as the scan against a second cfg 2 cloud of another seed as the reference,
max_dist 3 mm, the default iterations, min_step and lock_eps.  Per-kernel HIP-event times on the scan's handle divided by the
launches that did work (steps + 1 evaluations, the step kernels that wrote a row: a chain that has ended turns the rest of its
launches into returns, which the events time too and the division leaves in), the wall time of the call, best of the repeats,
both handles' slab indices and the reference's normal field built beforehand.  Beside it, in the same run: k_dev_nearest of
ppp_get_deviation over the same queries (the scan at the identity), the natural comparison for one evaluation.  Appends one JSON
line to profiles/registration_times.jsonl.  No pass/fail condition hangs on a time.
usage: python tools/registration_times.py [--reps N] [--config NAME]"""
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from polishpathplanning_amd import engine, synth  # noqa: E402

args = sys.argv[1:]
reps, cfg_name = 5, "cfg2_1m_s256"
while args:
    if args[0] == "--reps":
        reps = int(args[1])
    elif args[0] == "--config":
        cfg_name = args[1]
    else:
        raise SystemExit(__doc__)
    args = args[2:]

scan_pts, cfg = synth.make_config(cfg_name)
ref_pts, _ = synth.make_config(cfg_name, seed=97)
mm = scan_pts.astype(np.float64) * 1000.0
c = 0.5 * (mm.min(axis=0) + mm.max(axis=0))
a = math.radians(0.2)
ca, sa = math.cos(a), math.sin(a)
R = (np.array([[ca, -sa, 0], [sa, ca, 0], [0, 0, 1]]) @ np.array([[ca, 0, sa], [0, 1, 0], [-sa, 0, ca]])
     @ np.array([[1, 0, 0], [0, ca, -sa], [0, sa, ca]]))
moved = (((mm - c) @ R.T + c + np.array([0.3, -0.2, 0.25])) / 1000.0).astype(np.float32)
kw = dict(tool_radius=cfg["tool_radius"], walk=1)
ref, scan = engine.Engine(0, **kw), engine.Engine(0, **kw)
ref.set_cloud(ref_pts)
scan.set_cloud(moved)
RP = dict(max_dist=3.0)
ref.estimate_normals()                                       # first calls of the process: code objects, indices, buffers
scan.register(ref, **RP)
scan.deviation(ref, max_dist=3.0, maps=False)
scan.enable_timing(True)
scan.kernel_times()
best = {"register": {}, "deviation": {}}
walls = {k: [] for k in best}
launches, sig = {}, None


def keep(acc, k_ms):
    for k, v in k_ms.items():
        acc[k] = min(acc.get(k, 1e30), v)


for rep in range(reps):
    t = time.perf_counter()
    T, rows, st = scan.register(ref, **RP)
    walls["register"].append(time.perf_counter() - t)
    kt, launches["register"] = scan.kernel_times(with_launches=True)
    keep(best["register"], kt)
    s = (st["steps"], st["converged"], st["locked"], st["pairs_after"], st["rms_after"], T.tobytes())
    assert sig in (None, s)                                  # the same bits in every repeat
    sig = s
    t = time.perf_counter()
    dst = scan.deviation(ref, max_dist=3.0, maps=False)[5]
    walls["deviation"].append(time.perf_counter() - t)
    kt, launches["deviation"] = scan.kernel_times(with_launches=True)
    keep(best["deviation"], kt)

us = lambda d: {k: round(v * 1e3, 1) for k, v in sorted(d.items())}
evals, steps = st["steps"] + 1, max(st["steps"], 1)
line = json.dumps({"tool": "registration_times.py", "config": cfg_name, "n_scan": int(len(moved)), "n_ref": int(len(ref_pts)),
                   "params": dict(RP, iterations=30, min_step=1e-6, lock_eps=1e-9), "steps": st["steps"], "converged": st["converged"],
                   "locked": st["locked"], "pairs_before": st["pairs_before"], "pairs_after": st["pairs_after"],
                   "rms_before_mm": round(st["rms_before"], 5), "rms_after_mm": round(st["rms_after"], 5),
                   "kernel_us": us(best["register"]), "kernel_launches": {k: int(v) for k, v in sorted(launches["register"].items())},
                   "k_reg_terms_us_per_evaluation": round(best["register"].get("k_reg_terms", 0.0) * 1e3 / evals, 1),
                   "k_reg_step_us_per_step": round(best["register"].get("k_reg_step", 0.0) * 1e3 / steps, 1),
                   "call_ms": round(min(walls["register"]) * 1e3, 3),
                   "deviation_kernel_us": us(best["deviation"]), "deviation_matched": dst["matched"],
                   "deviation_call_ms": round(min(walls["deviation"]) * 1e3, 3), "reps": reps})
print(line)
with open(os.path.join(ROOT, "profiles", "registration_times.jsonl"), "a") as f:
    f.write(line + "\n")
ref.close(); scan.close()
