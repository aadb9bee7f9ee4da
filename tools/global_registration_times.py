#!/usr/bin/env python3
"""Event-timed global registration (ppp_register_global): cfg 2 (1 M points) moved by a large known motion -- (130, 25, -160)
degrees about x, y, z through the cloud's centre and (40, -25, 60) mm -- as the scan against a second cfg 2 cloud of another seed
as the reference, the default parameters (24 starts, coarse 10 mm / 8 iterations).  Per-kernel HIP-event times on the scan's
handle, best of the repeats, both handles' slab indices and the reference's normal field built beforehand:
  - the coarse stage as a whole (the compaction, k_reg_terms_multi, k_reg_step_multi) and per multi evaluation, at the default
    stride 16 and at stride 1;
  - the same K chains as K ppp_register calls one after the other from the same starts at stride 1 (k_reg_terms + k_reg_step
    summed over the calls, and the calls' wall time);
  - the fine chain (k_reg_terms, k_reg_step inside the global call) and the moments kernel (k_cloud_moments; the reference's runs
    on the reference's handle and is timed there).
Appends one JSON line to profiles/global_registration_times.jsonl.  No pass/fail condition hangs on a time.
usage: python tools/global_registration_times.py [--reps N] [--config NAME]"""
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


def rot(deg_x, deg_y, deg_z):
    ax, ay, az = (math.radians(v) for v in (deg_x, deg_y, deg_z))
    Rx = np.array([[1, 0, 0], [0, math.cos(ax), -math.sin(ax)], [0, math.sin(ax), math.cos(ax)]])
    Ry = np.array([[math.cos(ay), 0, math.sin(ay)], [0, 1, 0], [-math.sin(ay), 0, math.cos(ay)]])
    Rz = np.array([[math.cos(az), -math.sin(az), 0], [math.sin(az), math.cos(az), 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


scan_pts, cfg = synth.make_config(cfg_name)
ref_pts, _ = synth.make_config(cfg_name, seed=97)
mm = scan_pts.astype(np.float64) * 1000.0
c = 0.5 * (mm.min(axis=0) + mm.max(axis=0))
moved = (((mm - c) @ rot(130.0, 25.0, -160.0).T + c + np.array([40.0, -25.0, 60.0])) / 1000.0).astype(np.float32)
kw = dict(tool_radius=cfg["tool_radius"], walk=1)
ref, scan = engine.Engine(0, **kw), engine.Engine(0, **kw)
ref.set_cloud(ref_pts)
scan.set_cloud(moved)
COARSE = dict(max_dist=10.0, iterations=8, min_step=1e-3, lock_eps=1e-9)
ref.estimate_normals()                                       # first calls of the process: code objects, indices, buffers
T, cands, rows, st = scan.register_global(ref)
scan.register_global(ref, stride=1)
scan.register(ref, T0=cands[0]["T0"], **COARSE)
for e in (scan, ref):
    e.enable_timing(True)
    e.kernel_times()


def keep(acc, k_ms):
    for k, v in k_ms.items():
        acc[k] = min(acc.get(k, 1e30), v)


best = {"stride16": {}, "stride1": {}, "serial": {}, "ref": {}}
walls = {k: [] for k in best}
launches, sig = {}, {}
for rep in range(reps):
    for name, stride in (("stride16", 16), ("stride1", 1)):
        t = time.perf_counter()
        out = scan.register_global(ref, stride=stride)
        walls[name].append(time.perf_counter() - t)
        kt, launches[name] = scan.kernel_times(with_launches=True)
        keep(best[name], kt)
        keep(best["ref"], ref.kernel_times())
        s = (out[3]["winner"], out[3]["winner_cost"], out[3]["second_cost"], out[0].tobytes())
        assert sig.get(name) in (None, s)                    # the same bits in every repeat
        sig[name] = s
        if name == "stride16":
            g16 = out
        else:
            g1 = out
    t = time.perf_counter()
    serial = {}
    for cd in g1[1]:
        Tk, rk, sk = scan.register(ref, T0=cd["T0"], **COARSE)
        assert Tk.tobytes() == cd["T"].tobytes()             # stride 1: each coarse chain is ppp_register from that start
        for k, v in scan.kernel_times().items():
            serial[k] = serial.get(k, 0.0) + v
    walls["serial"].append(time.perf_counter() - t)
    keep(best["serial"], serial)

us = lambda d: {k: round(v * 1e3, 1) for k, v in sorted(d.items())}
evals = COARSE["iterations"] + 1
coarse_of = lambda d: sum(v for k, v in d.items() if k.startswith("k_compact") or k.endswith("_multi"))


def stage(name, g):
    d = best[name]
    return {"queries": g[3]["queries"], "shift": g[3]["shift"], "winner": g[3]["winner"], "winner_cost": g[3]["winner_cost"],
            "second_cost": g[3]["second_cost"], "coarse_steps": [cd["steps"] for cd in g[1]], "fine_steps": g[3]["fine"]["steps"],
            "fine_converged": g[3]["fine"]["converged"], "fine_rms_after_mm": g[3]["fine"]["rms_after"],
            "kernel_us": us(d), "kernel_launches": {k: int(v) for k, v in sorted(launches[name].items())},
            "coarse_stage_us": round(coarse_of(d) * 1e3, 1),
            "k_reg_terms_multi_us_per_evaluation": round(d.get("k_reg_terms_multi", 0.0) * 1e3 / evals, 1),
            "fine_chain_us": round((d.get("k_reg_terms", 0.0) + d.get("k_reg_step", 0.0)) * 1e3, 1),
            "k_cloud_moments_us": round(d.get("k_cloud_moments", 0.0) * 1e3, 1), "call_ms": round(min(walls[name]) * 1e3, 3)}


line = json.dumps({"tool": "global_registration_times.py", "config": cfg_name, "n_scan": int(len(moved)), "n_ref": int(len(ref_pts)),
                   "candidates": 24, "coarse": COARSE, "stride16": stage("stride16", g16), "stride1": stage("stride1", g1),
                   "one_after_the_other_stride1": {"kernel_us": us(best["serial"]),
                                                   "chains_us": round((best["serial"].get("k_reg_terms", 0.0) + best["serial"].get("k_reg_step", 0.0)) * 1e3, 1),
                                                   "calls_ms": round(min(walls["serial"]) * 1e3, 3)},
                   "reference_handle_kernel_us": us(best["ref"]), "reps": reps})
print(line)
with open(os.path.join(ROOT, "profiles", "global_registration_times.jsonl"), "a") as f:
    f.write(line + "\n")
ref.close(); scan.close()
