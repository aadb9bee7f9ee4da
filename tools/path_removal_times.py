#!/usr/bin/env python3
"""Event-timed path removal call (ppp_get_path_removal, Hertzian profile): the first call after a pass on a cloud just set, which
also builds what that pass did not (slab index and normal field behind a window pass) and the sample table, per-kernel
HIP-event times of its launches and the wall time of the call (statistics only, no map), best of the repeats.  Beside it, in
the same run: the first call of ppp_get_path_contacts on a cloud just set (the call the removal is measured against), and the
removal of a second profile on the same pass (the sample table and the lengths are the handle's by then).  The workloads of
tools/path_contacts_times.py:
  cfg2_window   cfg 2 (1 M points, 256 slices), kd pairing, window path (walk 1, no adjustment)
  cfg2_dyn      cfg 2, walk 1 with the dynamic adjustment (the pass leaves index and normals behind)
  cfg5_ranged8  cfg 5 (10 M points, 1024 slices) as 8 slice-range handles, one after the other (the times are summed)
usage: python tools/path_removal_times.py [--reps N] [workload ...]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from polishpathplanning_amd import engine, synth  # noqa: E402
from polishpathplanning_amd.robot_path import slice_ranges  # noqa: E402

WORKLOADS = {
    "cfg2_window": ("cfg2_1m_s256", dict(walk=1), 1),
    "cfg2_dyn": ("cfg2_1m_s256", dict(walk=1, dynamic_adjustment=1), 1),
    "cfg5_ranged8": ("cfg5_10m_s1024", dict(walk=1), 8),
}

args = sys.argv[1:]
reps = 5
if args and args[0] == "--reps":
    reps = int(args[1])
    args = args[2:]
for name in args or list(WORKLOADS):
    cfg_name, kw, parts = WORKLOADS[name]
    pts, cfg = synth.make_config(cfg_name)
    kw = dict(kw, tool_radius=cfg["tool_radius"])
    probe = engine.Engine(0, **kw)
    probe.set_cloud(pts)
    S = probe.gen_path()
    probe.close()
    ranges = slice_ranges(S, parts) if parts > 1 else [(0, 0)]
    handles = []
    for b, e in ranges:
        h = engine.Engine(0, slice_begin=b, slice_end=e, **kw) if parts > 1 else engine.Engine(0, **kw)
        h.set_cloud(pts)
        h.gen_path()
        h.path_removal(engine.REMOVAL_HERTZ, maps=False)   # first calls of the process: code objects, buffers
        h.path_removal(engine.REMOVAL_FLAT, maps=False)
        h.path_contacts(maps=False)
        h.enable_timing(True)
        handles.append(h)
    best, best_con, walls, walls_second, walls_con, stats = {}, {}, [], [], [], None
    for rep in range(reps):
        kt_sum, kt_con, wall, wall2, wall_con = {}, {}, 0.0, 0.0, 0.0
        touched, length, total = 0, 0.0, 0.0
        for h in handles:
            h.set_cloud(pts)                      # the cloud anew: the call builds the slab index (and the normals) again
            h.gen_path()
            h.kernel_times()
            t = time.perf_counter()
            st = h.path_removal(engine.REMOVAL_HERTZ, maps=False)[1]
            wall += time.perf_counter() - t
            for k, v in h.kernel_times().items():
                kt_sum[k] = kt_sum.get(k, 0.0) + v
            t = time.perf_counter()
            h.path_removal(engine.REMOVAL_FLAT, maps=False)
            wall2 += time.perf_counter() - t
            touched += st["touched"]; length += st["path_length"]; total += st["sum"]
            h.set_cloud(pts)                      # and once more for the call it is measured against
            h.gen_path()
            h.kernel_times()
            t = time.perf_counter()
            h.path_contacts(maps=False)
            wall_con += time.perf_counter() - t
            for k, v in h.kernel_times().items():
                kt_con[k] = kt_con.get(k, 0.0) + v
        for acc, kt in ((best, kt_sum), (best_con, kt_con)):
            for k, v in kt.items():
                acc[k] = min(acc.get(k, 1e30), v)
        walls.append(wall); walls_second.append(wall2); walls_con.append(wall_con)
        assert stats is None or stats == (touched, length, total)   # the same bits in every repeat
        stats = (touched, length, total)
    window = all(h.fast_path() for h in handles)   # (asked after the calls: they leave the window path alone)
    whole = handles[0].path_removal(engine.REMOVAL_HERTZ, maps=False)[1] if parts == 1 else None
    print(json.dumps({"tool": "path_removal_times.py", "workload": name, "config": cfg_name, "n": int(len(pts)), "S": S,
                      "handles": len(handles), "window_path": window, "profile": "hertz", "touched": stats[0],
                      "path_length_mm": round(stats[1], 3), "mean_removal_mm": round(stats[2] / max(stats[0], 1), 4),
                      "cv": round(whole["cv"], 4) if whole else None,
                      "kernel_us": {k: round(v * 1e3, 1) for k, v in sorted(best.items())},
                      "first_call_ms": round(min(walls) * 1e3, 3), "second_profile_ms": round(min(walls_second) * 1e3, 3),
                      "contacts_kernel_us": {k: round(v * 1e3, 1) for k, v in sorted(best_con.items())},
                      "contacts_first_call_ms": round(min(walls_con) * 1e3, 3), "reps": reps}))
    for h in handles:
        h.close()
