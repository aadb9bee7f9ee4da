#!/usr/bin/env python3
"""Timed tiled registration (ppp_register_tiles): cfg 5 (10 M points, 1024 slices) moved by a small known motion -- 0.2 degrees
about every axis through the cloud's centre and (0.3, -0.2, 0.25) mm, as tools/registration_times.py moves its scan -- held as 8
slice-range handles, against a second cfg 5 cloud of another seed on ONE whole-cloud handle that stands in every slot, max_dist
3 mm, the default iterations, min_step and lock_eps.

What a tiled loop pays and the whole-cloud chain does not is one host round trip per evaluation: T to every tile, a launch and
a copy back per tile, the wait, the merge and the step.  Nobody had measured it.  Per evaluation this reports
  - the slowest tile's k_regt_terms (HIP events on every tile's handle, in repeats of their own: the events cost time),
  - the host's merge and step (ppp_merge_registration_terms and ppp_registration_step on the last evaluation's parts, timed
    alone), and
  - the rest of the evaluation's wall time: enqueueing, the copies and the wait beyond the slowest kernel,
and the whole call.  Beside it, in the same run, ppp_register on a whole-cloud handle of the same cloud: k_reg_terms per
evaluation and the whole call.  The tiled result is asserted equal to the whole-cloud call's, bit for bit.  Appends one JSON line
to profiles/registration_tile_times.jsonl.  No pass/fail condition hangs on a time.

Every step that uses the GPU is a process of its own under `timeout -k 10`, chained with &&: the driver (no --step) starts
`--step tiles`, then `--step whole`, and joins what they wrote; a step that fails or runs out of time ends the run.
usage: python tools/registration_tile_times.py [--reps N] [--config NAME] [--tiles K] [--limit SECONDS]"""
import json
import math
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

args = sys.argv[1:]
reps, cfg_name, K, step, out, limit = 3, "cfg5_10m_s1024", 8, None, None, 420
while args:
    if args[0] == "--reps":
        reps = int(args[1])
    elif args[0] == "--config":
        cfg_name = args[1]
    elif args[0] == "--tiles":
        K = int(args[1])
    elif args[0] == "--step":
        step = args[1]
    elif args[0] == "--out":
        out = args[1]
    elif args[0] == "--limit":
        limit = int(args[1])
    else:
        raise SystemExit(__doc__)
    args = args[2:]

RP = dict(max_dist=3.0)


def note(msg):
    print("[registration_tile_times] " + msg, file=sys.stderr, flush=True)


if step is None:
    with tempfile.TemporaryDirectory() as tmp:
        parts = [os.path.join(tmp, s + ".json") for s in ("tiles", "whole")]
        common = "--reps %d --config %s --tiles %d" % (reps, cfg_name, K)
        me = os.path.abspath(__file__)
        chain = " && ".join("timeout -k 10 %d %s %s %s --step %s --out %s" % (limit, sys.executable, me, common, s, p)
                            for s, p in zip(("tiles", "whole"), parts))
        rc = subprocess.call(chain, shell=True)
        if rc:
            raise SystemExit("a step failed or ran out of time (exit %d): nothing recorded" % rc)
        tiles, whole = (json.load(open(p)) for p in parts)
    assert tiles.pop("signature") == whole.pop("signature"), "the tiled loop and ppp_register disagree"
    line = json.dumps(dict({"tool": "registration_tile_times.py", "config": cfg_name, "tiles": K, "params": dict(RP, iterations=30, min_step=1e-6, lock_eps=1e-9),
                            "reps": reps}, **dict(tiles, **whole)))
    print(line)
    with open(os.path.join(ROOT, "profiles", "registration_tile_times.jsonl"), "a") as f:
        f.write(line + "\n")
    raise SystemExit(0)

from polishpathplanning_amd import engine, synth  # noqa: E402
from polishpathplanning_amd.robot_path import slice_ranges  # noqa: E402

scan_pts, cfg = synth.make_config(cfg_name)
ref_pts, _ = synth.make_config(cfg_name, seed=97)
mm = scan_pts.astype(np.float64) * 1000.0
c = 0.5 * (mm.min(axis=0) + mm.max(axis=0))
a = math.radians(0.2)
ca, sa = math.cos(a), math.sin(a)
R = (np.array([[ca, -sa, 0], [sa, ca, 0], [0, 0, 1]]) @ np.array([[ca, 0, sa], [0, 1, 0], [-sa, 0, ca]])
     @ np.array([[1, 0, 0], [0, ca, -sa], [0, sa, ca]]))
moved = (((mm - c) @ R.T + c + np.array([0.3, -0.2, 0.25])) / 1000.0).astype(np.float32)
del mm
kw = dict(tool_radius=cfg["tool_radius"], walk=1)
ref = engine.Engine(0, **kw)
ref.set_cloud(ref_pts)
ref.estimate_normals()                                       # first calls of the process: code objects, the index, the normal field
us = lambda ms: round(ms * 1e3, 1)


def signature(T, rows, st):
    return [st["steps"], st["converged"], st["locked"], st["pairs_before"], st["pairs_after"], T.tobytes().hex(),
            [int(r["E"]) for r in rows], [r["pairs"] for r in rows]]


if step == "whole":
    scan = engine.Engine(0, **kw)
    scan.set_cloud(moved)
    T, rows, st = scan.register(ref, **RP)
    note("whole-cloud handle ready: %d steps" % st["steps"])
    plain, timed = [], {}
    for rep in range(reps):
        t0 = time.perf_counter()
        got = scan.register(ref, **RP)
        plain.append(time.perf_counter() - t0)
        assert signature(*got) == signature(T, rows, st)
    scan.enable_timing(True)
    scan.kernel_times()
    for rep in range(reps):
        scan.register(ref, **RP)
        for k, v in scan.kernel_times().items():
            timed[k] = min(timed.get(k, 1e30), v)
    evals = st["steps"] + 1
    res = {"signature": signature(T, rows, st), "whole_call_ms": round(min(plain) * 1e3, 3),
           "whole_k_reg_terms_us_per_evaluation": us(timed.get("k_reg_terms", 0.0) / evals),
           "whole_k_reg_step_us_per_step": us(timed.get("k_reg_step", 0.0) / max(st["steps"], 1))}
    scan.close()
elif step == "tiles":
    first = engine.Engine(0, **kw)
    first.set_cloud(moved)
    S = first.gen_path()
    first.close()
    hs = []
    for b, e in slice_ranges(S, K):
        h = engine.Engine(0, slice_begin=b, slice_end=e, **kw)
        h.set_cloud(moved)
        hs.append(h)
        note("tile %d of %d set: slices [%d, %d)" % (len(hs), K, b, e))
    T, rows, st = engine.register_tiles(hs, ref, **RP)        # the indices, the buffers
    evals = st["steps"] + 1
    note("tiles ready: %d steps" % st["steps"])
    plain, slowest = [], 1e30
    for rep in range(reps):
        t0 = time.perf_counter()
        got = engine.register_tiles(hs, ref, **RP)
        plain.append(time.perf_counter() - t0)
        assert signature(*got) == signature(T, rows, st)
    for h in hs:
        h.enable_timing(True)
        h.kernel_times()
    timed_wall = []
    for rep in range(reps):
        t0 = time.perf_counter()
        engine.register_tiles(hs, ref, **RP)
        timed_wall.append(time.perf_counter() - t0)
        per_tile = [h.kernel_times().get("k_regt_terms", 0.0) / evals for h in hs]
        slowest = min(slowest, max(per_tile))
    for h in hs:
        h.enable_timing(False)
    # the host's merge and step, alone: the last evaluation's parts through the two host calls
    tiles = [h.registration_terms_tile(ref, T=T, **RP) for h in hs]
    n_host, t0 = 2000, time.perf_counter()
    for _ in range(n_host):
        row, part = engine.merge_registration_terms(tiles, T)
    merge_us = (time.perf_counter() - t0) / n_host * 1e6
    t0 = time.perf_counter()
    for _ in range(n_host):
        engine.registration_step(rows[0], part)
    step_us = (time.perf_counter() - t0) / n_host * 1e6
    per_eval_us = min(plain) * 1e6 / evals
    res = {"signature": signature(T, rows, st), "n_scan": int(len(moved)), "n_ref": int(len(ref_pts)), "steps": st["steps"],
           "converged": st["converged"], "pairs_after": st["pairs_after"], "rms_before_mm": round(st["rms_before"], 5),
           "rms_after_mm": round(st["rms_after"], 5), "owned": [t[1]["owned"] for t in tiles], "evaluated": [t[1]["evaluated"] for t in tiles],
           "tiles_call_ms": round(min(plain) * 1e3, 3), "tiles_call_ms_with_events": round(min(timed_wall) * 1e3, 3),
           "tiles_us_per_evaluation": round(per_eval_us, 1), "slowest_tile_k_regt_terms_us_per_evaluation": us(slowest),
           "host_merge_us_through_python": round(merge_us, 1), "host_step_us_through_python": round(step_us, 1),
           "round_trip_us_per_evaluation_beyond_the_slowest_kernel": round(per_eval_us - slowest * 1e3, 1)}
    for h in hs:
        h.close()
else:
    raise SystemExit(__doc__)
ref.close()
with open(out, "w") as f:
    json.dump(res, f)
