#!/usr/bin/env python3
"""Event-timed deviation tiles (ppp_get_deviation_tile): cfg 5 (10 M points, 1024 slices) as 8 slice-range handles of the scan
against a second cfg 5 cloud of another seed as 8 slice-range handles of the reference, max_dist 3 mm, smooth_radius 4 mm,
allowance 0.05, gain 1, halo 7 mm -- per-kernel HIP-event times summed over the 8 tiles (one after the other on one device),
the wall time of the 8 calls (parts only) and of the host merge, best of the repeats, all slab indices built beforehand.
Beside it, in the same run: ppp_get_deviation of the same two clouds on one whole-cloud handle each.  The merged statistics
are asserted equal to the whole-cloud call's.  Appends one JSON line to profiles/deviation_tile_times.jsonl.  No pass/fail
condition hangs on a time.
usage: python tools/deviation_tile_times.py [--reps N] [--config NAME] [--tiles K]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from polishpathplanning_amd import engine, synth  # noqa: E402
from polishpathplanning_amd.robot_path import slice_ranges  # noqa: E402

args = sys.argv[1:]
reps, cfg_name, K = 3, "cfg5_10m_s1024", 8
while args:
    if args[0] == "--reps":
        reps = int(args[1])
    elif args[0] == "--config":
        cfg_name = args[1]
    elif args[0] == "--tiles":
        K = int(args[1])
    else:
        raise SystemExit(__doc__)
    args = args[2:]

def note(msg):
    print("[deviation_tile_times] " + msg, file=sys.stderr, flush=True)


scan_pts, cfg = synth.make_config(cfg_name)
ref_pts, _ = synth.make_config(cfg_name, seed=97)
kw = dict(tool_radius=cfg["tool_radius"], walk=1)
DP = dict(max_dist=3.0, smooth_radius=4.0, allowance=0.05, gain=1.0)
HALO = 7.0
ref, scan = engine.Engine(0, **kw), engine.Engine(0, **kw)
ref.set_cloud(ref_pts)
scan.set_cloud(scan_pts)
S, Sr = scan.gen_path(), ref.gen_path()
note("clouds set: %d and %d points, %d and %d slices" % (len(scan_pts), len(ref_pts), S, Sr))
whole = scan.deviation(ref, maps=False, **DP)[5]          # first call of the process: code objects, indices, buffers
tiles_h = []
for (b, e), (rb, re_) in zip(slice_ranges(S, K), slice_ranges(Sr, K)):
    h = engine.Engine(0, slice_begin=b, slice_end=e, **kw)
    h.set_cloud(scan_pts)
    r = engine.Engine(0, slice_begin=rb, slice_end=re_, **kw)
    r.set_cloud(ref_pts)
    h.deviation_tile(r, HALO, maps=False, **DP)
    h.enable_timing(True); r.enable_timing(True)
    h.kernel_times(); r.kernel_times()
    tiles_h.append((h, r))
    note("tile %d of %d ready" % (len(tiles_h), K))
scan.enable_timing(True); ref.enable_timing(True)
scan.kernel_times(); ref.kernel_times()


def keep(acc, k_ms):
    for k, v in k_ms.items():
        acc[k] = min(acc.get(k, 1e30), v)


best_t, best_w, wall_t, wall_w, wall_m = {}, {}, [], [], []
for rep in range(reps):
    ksum, t0 = {}, time.perf_counter()
    for h, r in tiles_h:
        h.deviation_tile(r, HALO, maps=False, **DP)
    wall_t.append(time.perf_counter() - t0)
    for h, r in tiles_h:
        for k, v in list(h.kernel_times().items()) + [("ref:" + k, v) for k, v in r.kernel_times().items()]:
            ksum[k] = ksum.get(k, 0.0) + v
    keep(best_t, ksum)
    t0 = time.perf_counter()
    st = scan.deviation(ref, maps=False, **DP)[5]
    wall_w.append(time.perf_counter() - t0)
    keep(best_w, scan.kernel_times())
    keep(best_w, {"ref:" + k: v for k, v in ref.kernel_times().items()})
    note("repeat %d of %d timed" % (rep + 1, reps))
    assert all(np.array([st[k]]).tobytes() == np.array([whole[k]]).tobytes() for k in st if k != "hist")
# the maps once, for the merge (not timed: eight times five maps of 10 M entries over the bus)
tiles = [h.deviation_tile(r, HALO, **DP) for h, r in tiles_h]
for rep in range(reps):
    t0 = time.perf_counter()
    merged = engine.merge_deviation_tiles(tiles)
    wall_m.append(time.perf_counter() - t0)
for k in whole:
    assert np.asarray(merged[k]).tobytes() == np.asarray(whole[k]).tobytes(), k

us = lambda d: {k: round(v * 1e3, 1) for k, v in sorted(d.items())}
line = json.dumps({"tool": "deviation_tile_times.py", "config": cfg_name, "n_scan": int(len(scan_pts)), "n_ref": int(len(ref_pts)),
                   "tiles": K, "halo": HALO, "params": DP, "matched": whole["matched"], "too_far": whole["too_far"],
                   "evaluated": [t[6]["evaluated"] for t in tiles], "owned": [t[6]["owned"] for t in tiles],
                   "tiles_kernel_us_sum": us(best_t), "tiles_calls_ms_sum": round(min(wall_t) * 1e3, 3),
                   "merge_host_ms": round(min(wall_m) * 1e3, 1),
                   "whole_kernel_us": us(best_w), "whole_call_ms": round(min(wall_w) * 1e3, 3), "reps": reps})
print(line)
with open(os.path.join(ROOT, "profiles", "deviation_tile_times.jsonl"), "a") as f:
    f.write(line + "\n")
for h, r in tiles_h:
    h.close(); r.close()
ref.close(); scan.close()
