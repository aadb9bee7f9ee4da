#!/usr/bin/env python3
"""Event-timed contact field call (ppp_get_contact_field): the first call on a cloud just set (slab index and normal field
resident, no pass), per-kernel HIP-event times of its launches and the wall time of the call (statistics only, no maps), best of the repeats.  Beside it the comparator that exists
without the field -- the same values for all n points through ppp_area2cloud with key 0 and key 1 (k_area2cloud_api) -- and
ppp_estimate_normals on the same cloud as a scale (the closest existing whole-cloud gather).  One whole-cloud handle each:
  cfg2   cfg 2 (1 M points)
  cfg5   cfg 5 (10 M points)
A line per workload is printed and appended to profiles/contact_field_times.jsonl.
usage: python tools/contact_field_times.py [--reps N] [workload ...]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from polishpathplanning_amd import engine, synth  # noqa: E402

WORKLOADS = {"cfg2": "cfg2_1m_s256", "cfg5": "cfg5_10m_s1024"}
FIELD = ("k_field_batch", "k_field_stats")

args = sys.argv[1:]
reps = 5
if args and args[0] == "--reps":
    reps = int(args[1])
    args = args[2:]
for name in args or list(WORKLOADS):
    cfg_name = WORKLOADS[name]
    pts, cfg = synth.make_config(cfg_name)
    h = engine.Engine(0, tool_radius=cfg["tool_radius"], walk=1)
    h.set_cloud(pts)
    h.contact_field(maps=False)                   # first call of the process: code objects, buffers
    h.enable_timing(True)
    best, walls = {}, []
    for rep in range(reps):
        h.set_cloud(pts)                          # the cloud anew: the field is computed again
        h.estimate_normals()                      # index and normal-field code warm; the index is resident from here on
        h.kernel_times()
        t = time.perf_counter()
        st = h.contact_field(maps=False, min_width=float(int(2 * cfg["tool_radius"])))[2]
        walls.append(time.perf_counter() - t)
        for k, v in h.kernel_times().items():
            best[k] = min(best.get(k, 1e30), v)
    field_ms = sum(best.get(k, 0.0) for k in FIELD)
    # the comparator: every point through ppp_area2cloud, key 0 and key 1 (its normal field is excluded, as the field's is)
    P = h.cloud().astype(np.float64)
    a2c = []
    h.area2cloud(P[:4096], 0)
    for rep in range(reps):
        h.kernel_times()
        h.area2cloud(P, 0); h.area2cloud(P, 1)
        a2c.append(h.kernel_times().get("k_area2cloud_api", 0.0))
    nrm = []
    for rep in range(reps):
        h.kernel_times()
        h.estimate_normals()
        nrm.append(h.kernel_times().get("k_normals_all", 0.0))
    rec = {"workload": name, "config": cfg_name, "n": int(len(pts)), "curvature_k": 50, "valid": int(st["valid"]),
           "narrow": int(st["narrow"]), "mean_abs_r": round(st["mean_abs_r"], 6),
           "kernel_us": {k: round(v * 1e3, 1) for k, v in sorted(best.items())},
           "field_kernels_ms": round(field_ms, 3), "area2cloud_both_keys_ms": round(min(a2c), 3),
           "ratio": round(field_ms / max(min(a2c), 1e-9), 3), "estimate_normals_ms": round(min(nrm), 3),
           "first_call_ms": round(min(walls) * 1e3, 3), "reps": reps}
    line = json.dumps(rec)
    print(line)
    with open(os.path.join(ROOT, "profiles", "contact_field_times.jsonl"), "a") as f:
        f.write(line + "\n")
    h.close()
