#!/usr/bin/env python3
"""Event-timed deviation map (ppp_get_deviation): cfg 2 (1 M points) as the scan against a second cfg 2 cloud of another seed
as the reference, max_dist 3 mm, allowance 0.05, gain 1, without smoothing and with smooth_radius 4 mm -- per-kernel HIP-event
times on the scan's handle, the launches of each kernel and the wall time of the call (statistics only), best of the repeats,
both handles' slab indices built beforehand.  Beside it, in the same run: ppp_estimate_normals(ref) (k_normals_all on the
reference's handle, the field every call builds), and ppp_nearest over the same queries -- the scan's points in cloud order
through the existing thread-per-query kernel (k_nearest_api), which has no bound and does not enter the slabs through their
y-bucket rows.  Appends one JSON line to profiles/deviation_times.jsonl.  No pass/fail condition hangs on a time.
usage: python tools/deviation_times.py [--reps N] [--config NAME]"""
import json
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
kw = dict(tool_radius=cfg["tool_radius"], walk=1)
ref, scan = engine.Engine(0, **kw), engine.Engine(0, **kw)
ref.set_cloud(ref_pts)
scan.set_cloud(scan_pts)
DP = dict(max_dist=3.0, allowance=0.05, gain=1.0)
queries = scan.cloud()
ref.estimate_normals(); ref.nearest(queries[:64])        # first calls of the process: code objects, indices, buffers
for sr in (0.0, 4.0):
    scan.deviation(ref, smooth_radius=sr, maps=False, **DP)
ref.enable_timing(True); scan.enable_timing(True)
ref.kernel_times(); scan.kernel_times()
best = {"plain": {}, "smooth": {}, "normals": {}, "nearest": {}}
walls = {k: [] for k in best}
launches, stats = {}, {}


def keep(acc, k_ms):
    for k, v in k_ms.items():
        acc[k] = min(acc.get(k, 1e30), v)


for rep in range(reps):
    for key, sr in (("plain", 0.0), ("smooth", 4.0)):
        ref.kernel_times()
        t = time.perf_counter()
        st = scan.deviation(ref, smooth_radius=sr, maps=False, **DP)[5]
        walls[key].append(time.perf_counter() - t)
        kt, launches[key] = scan.kernel_times(with_launches=True)
        keep(best[key], kt)
        keep(best[key], {"ref:" + k: v for k, v in ref.kernel_times().items()})
        sig = tuple(st[k] for k in ("matched", "too_far", "no_normal", "dropped", "proud", "below", "min_dev", "max_dev", "mean_dev"))
        assert stats.get(key, sig) == sig                # the same bits in every repeat
        stats[key] = sig
        last = st
    t = time.perf_counter()
    ref.estimate_normals()
    walls["normals"].append(time.perf_counter() - t)
    keep(best["normals"], ref.kernel_times())
    t = time.perf_counter()
    idx = ref.nearest(queries)
    walls["nearest"].append(time.perf_counter() - t)
    keep(best["nearest"], ref.kernel_times())

us = lambda d: {k: round(v * 1e3, 1) for k, v in sorted(d.items())}
line = json.dumps({"tool": "deviation_times.py", "config": cfg_name, "n_scan": int(len(scan_pts)), "n_ref": int(len(ref_pts)),
                   "params": DP, "smooth_radius": 4.0, "matched": last["matched"], "too_far": last["too_far"],
                   "rms_dev_mm": round(last["rms_dev"], 4), "nearest_found": int((idx >= 0).sum()),
                   "kernel_us": us(best["plain"]), "kernel_launches": {k: int(v) for k, v in sorted(launches["plain"].items())},
                   "call_ms": round(min(walls["plain"]) * 1e3, 3),
                   "smooth_kernel_us": us(best["smooth"]), "smooth_call_ms": round(min(walls["smooth"]) * 1e3, 3),
                   "estimate_normals_kernel_us": us(best["normals"]), "estimate_normals_call_ms": round(min(walls["normals"]) * 1e3, 3),
                   "nearest_kernel_us": us(best["nearest"]), "nearest_call_ms": round(min(walls["nearest"]) * 1e3, 3), "reps": reps})
print(line)
with open(os.path.join(ROOT, "profiles", "deviation_times.jsonl"), "a") as f:
    f.write(line + "\n")
ref.close(); scan.close()
