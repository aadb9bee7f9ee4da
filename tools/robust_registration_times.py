#!/usr/bin/env python3
"""Event-timed robust registration (ppp_register_robust) beside ppp_register_trimmed and ppp_register on the same inputs in the
same run: the scan of tools/trimmed_registration_times.py -- cfg 2 (1 M points) with one eighth of it, x in the first quarter
and y in the lower half of its box, raised by 1.5 mm and then moved by 0.2 degrees about every axis through the cloud's centre
and (0.3, -0.2, 0.25) mm -- against a second cfg 2 cloud of another seed as the reference; max_dist 3 mm, tune 4.685, sigma_min
1e-4 mm, keep 0.8 for the trimmed call, the default iterations, min_step and lock_eps.  Per-kernel HIP-event times on the scan's
handle, summed over a call's launches and divided by the evaluations that did work (steps + 1; a chain that has ended turns the
rest of its launches into returns, which the events time too and the division leaves in), the wall time of each call, best of
the repeats, both handles' slab indices and the reference's normal field built beforehand.  Appends one JSON line to
profiles/robust_registration_times.jsonl (--out: elsewhere).  No pass/fail condition hangs on a time.
usage: python tools/robust_registration_times.py [--reps N] [--config NAME] [--tune C] [--keep SHARE] [--out FILE]"""
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
reps, cfg_name, tune, share, out = 5, "cfg2_1m_s256", 4.685, 0.8, os.path.join(ROOT, "profiles", "robust_registration_times.jsonl")
while args:
    if args[0] == "--reps":
        reps = int(args[1])
    elif args[0] == "--config":
        cfg_name = args[1]
    elif args[0] == "--tune":
        tune = float(args[1])
    elif args[0] == "--keep":
        share = float(args[1])
    elif args[0] == "--out":
        out = args[1]
    else:
        raise SystemExit(__doc__)
    args = args[2:]

scan_pts, cfg = synth.make_config(cfg_name)
ref_pts, _ = synth.make_config(cfg_name, seed=97)
mm = scan_pts.astype(np.float64) * 1000.0
lo, hi = mm.min(axis=0), mm.max(axis=0)
raised = (mm[:, 0] < lo[0] + 0.25 * (hi[0] - lo[0])) & (mm[:, 1] < lo[1] + 0.5 * (hi[1] - lo[1]))
mm[raised, 2] += 1.5
c = 0.5 * (lo + hi)
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
calls = {"robust": lambda: scan.register_robust(ref, tune=tune, **RP),
         "trimmed": lambda: scan.register_trimmed(ref, keep=share, **RP),
         "register": lambda: scan.register(ref, **RP)}
ref.estimate_normals()                                       # first calls of the process: code objects, indices, buffers
for call in calls.values():
    call()
scan.enable_timing(True)
scan.kernel_times()
best = {k: {} for k in calls}
walls = {k: [] for k in calls}
launches, sigs, results = {}, {}, {}

for rep in range(reps):
    for name, call in calls.items():
        t = time.perf_counter()
        got = call()
        walls[name].append(time.perf_counter() - t)
        kt, launches[name] = scan.kernel_times(with_launches=True)
        for k, v in kt.items():
            best[name][k] = min(best[name].get(k, 1e30), v)
        st = got[-1]
        s = (st["steps"], st["converged"], st["locked"], st["pairs_after"], st["rms_after"], got[0].tobytes()) + tuple(m.tobytes() for m in got[2:-1])
        assert sigs.get(name) in (None, s)                   # the same bits in every repeat
        sigs[name], results[name] = s, got


def report(name):
    st = results[name][-1]
    n = st["steps"] + 1
    return {"steps": st["steps"], "converged": st["converged"], "locked": st["locked"], "pairs_before": st["pairs_before"],
            "pairs_after": st["pairs_after"], "rms_before_mm": round(st["rms_before"], 5), "rms_after_mm": round(st["rms_after"], 5),
            "kernel_us": {k: round(v * 1e3, 1) for k, v in sorted(best[name].items())},
            "kernel_launches": {k: int(v) for k, v in sorted(launches[name].items())},
            "kernel_us_per_evaluation": {k: round(v * 1e3 / n, 1) for k, v in sorted(best[name].items())},
            "call_ms": round(min(walls[name]) * 1e3, 3)}


T, rows, status, weight, residual, st = results["robust"]
robust = report("robust")
robust.update(used_before=rows[0]["used"], used_after=rows[-1]["used"], median_after_mm=rows[-1]["median_abs"], sigma_after_mm=rows[-1]["sigma"],
              weight_sum_after=round(math.ldexp(float(rows[-1]["weight_sum"]), -st["shift"]), 3),
              raised_used=int((status[raised] == engine.ROBUST_USED).sum()),
              status_used_rejected_unpaired_dropped=[int((status == v).sum()) for v in range(4)])
trimmed = report("trimmed")
trimmed.update(raised_kept=int((results["trimmed"][2][raised] == engine.TRIM_KEPT).sum()))
line = json.dumps({"tool": "robust_registration_times.py", "config": cfg_name, "n_scan": int(len(moved)), "n_ref": int(len(ref_pts)),
                   "raised": int(raised.sum()), "tune": tune, "sigma_min": 1e-4, "keep": share,
                   "params": dict(RP, iterations=30, min_step=1e-6, lock_eps=1e-9), "robust": robust, "trimmed": trimmed, "register": report("register"),
                   "translation_difference_to_trimmed_mm": [round(float(v), 5) for v in (T[:, 3] - results["trimmed"][0][:, 3])],
                   "translation_difference_to_register_mm": [round(float(v), 5) for v in (T[:, 3] - results["register"][0][:, 3])], "reps": reps})
print(line)
with open(out, "a") as f:
    f.write(line + "\n")
ref.close(); scan.close()
