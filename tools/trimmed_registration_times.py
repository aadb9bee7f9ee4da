#!/usr/bin/env python3
"""Event-timed trimmed registration (ppp_register_trimmed) beside ppp_register on the same inputs in the same run: cfg 2 (1 M
points) with one eighth of it -- x in the first quarter, y in the lower half of its box -- raised by 1.5 mm and then moved as
tools/registration_times.py moves it (0.2 degrees about every axis through the cloud's centre and (0.3, -0.2, 0.25) mm), as the
scan against a second cfg 2 cloud of another seed as the reference; max_dist 3 mm, keep 0.8, the default iterations, min_step
and lock_eps.  Per-kernel HIP-event times on the scan's handle, summed over a call's launches and divided by the evaluations
that did work (steps + 1; a chain that has ended turns the rest of its launches into returns, which the events time too and
the division leaves in), the wall time of each call, best of the repeats, both handles' slab indices and the reference's normal
field built beforehand.  Appends one JSON line to profiles/trimmed_registration_times.jsonl (--out: elsewhere).  No pass/fail
condition hangs on a time.
usage: python tools/trimmed_registration_times.py [--reps N] [--config NAME] [--keep SHARE] [--out FILE]"""
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
reps, cfg_name, share, out = 5, "cfg2_1m_s256", 0.8, os.path.join(ROOT, "profiles", "trimmed_registration_times.jsonl")
while args:
    if args[0] == "--reps":
        reps = int(args[1])
    elif args[0] == "--config":
        cfg_name = args[1]
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
ref.estimate_normals()                                       # first calls of the process: code objects, indices, buffers
scan.register(ref, **RP)
scan.register_trimmed(ref, keep=share, **RP)
scan.enable_timing(True)
scan.kernel_times()
best = {"trimmed": {}, "register": {}}
walls = {k: [] for k in best}
launches, sig = {}, None


def keep_best(acc, k_ms):
    for k, v in k_ms.items():
        acc[k] = min(acc.get(k, 1e30), v)


for rep in range(reps):
    t = time.perf_counter()
    T, rows, status, d2, st = scan.register_trimmed(ref, keep=share, **RP)
    walls["trimmed"].append(time.perf_counter() - t)
    kt, launches["trimmed"] = scan.kernel_times(with_launches=True)
    keep_best(best["trimmed"], kt)
    s = (st["steps"], st["converged"], st["locked"], st["pairs_after"], st["rms_after"], T.tobytes(), status.tobytes(), d2.tobytes())
    assert sig in (None, s)                                  # the same bits in every repeat
    sig = s
    t = time.perf_counter()
    T0, rows0, st0 = scan.register(ref, **RP)
    walls["register"].append(time.perf_counter() - t)
    kt, launches["register"] = scan.kernel_times(with_launches=True)
    keep_best(best["register"], kt)

us = lambda d: {k: round(v * 1e3, 1) for k, v in sorted(d.items())}
evals, evals0 = st["steps"] + 1, st0["steps"] + 1
per = lambda d, n: {k: round(v * 1e3 / n, 1) for k, v in sorted(d.items())}
status_counts = [int((status == v).sum()) for v in range(4)]
line = json.dumps({"tool": "trimmed_registration_times.py", "config": cfg_name, "n_scan": int(len(moved)), "n_ref": int(len(ref_pts)),
                   "raised": int(raised.sum()), "keep": share, "params": dict(RP, iterations=30, min_step=1e-6, lock_eps=1e-9),
                   "trimmed": {"steps": st["steps"], "converged": st["converged"], "locked": st["locked"],
                               "kept_before": st["pairs_before"], "kept_after": st["pairs_after"], "paired_after": rows[-1]["paired"],
                               "trim_d2_after": rows[-1]["trim_d2"], "rms_before_mm": round(st["rms_before"], 5),
                               "rms_after_mm": round(st["rms_after"], 5), "raised_kept": int((status[raised] == engine.TRIM_KEPT).sum()),
                               "status_kept_trimmed_unpaired_dropped": status_counts,
                               "kernel_us": us(best["trimmed"]), "kernel_launches": {k: int(v) for k, v in sorted(launches["trimmed"].items())},
                               "kernel_us_per_evaluation": per(best["trimmed"], evals), "call_ms": round(min(walls["trimmed"]) * 1e3, 3)},
                   "register": {"steps": st0["steps"], "converged": st0["converged"], "locked": st0["locked"],
                                "pairs_before": st0["pairs_before"], "pairs_after": st0["pairs_after"],
                                "rms_before_mm": round(st0["rms_before"], 5), "rms_after_mm": round(st0["rms_after"], 5),
                                "kernel_us": us(best["register"]), "kernel_launches": {k: int(v) for k, v in sorted(launches["register"].items())},
                                "kernel_us_per_evaluation": per(best["register"], evals0), "call_ms": round(min(walls["register"]) * 1e3, 3)},
                   "translation_difference_mm": [round(float(v), 5) for v in (T[:, 3] - T0[:, 3])], "reps": reps})
print(line)
with open(out, "a") as f:
    f.write(line + "\n")
ref.close(); scan.close()
