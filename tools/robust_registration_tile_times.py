#!/usr/bin/env python3
"""Timed tiled robust registration (ppp_register_robust_tiles): cfg 5 (10 M points, 1024 slices) with one eighth of it -- x in
the first quarter, y in the lower half of its box -- raised by 1.5 mm and then moved as tools/trimmed_registration_tile_times.py
moves its scan (0.2 degrees about every axis through the cloud's centre and (0.3, -0.2, 0.25) mm), held as 8 slice-range handles
on one device, against a second cfg 5 cloud of another seed on ONE whole-cloud handle that stands in every slot; max_dist 3 mm,
tune 4.685, sigma_min 1e-4, the default iterations, min_step and lock_eps.

A tiled robust evaluation pays the tiled trimmed one's four host waits -- three histogram merges and the sums.  Per evaluation
this reports
  - the slowest tile's kernels (HIP events on every tile's handle, in repeats of their own: the events cost time): k_robt_pair,
    k_trimt_narrow<1>, <2>, k_robt_terms, each the largest over the tiles, and their sum,
  - what the four waits cost: the evaluation's wall time beyond that sum -- enqueueing, the copies, the waits, the merges --,
and the whole call, without maps and with them.  Beside it, in the same run: ppp_register_trimmed_tiles (keep 0.8) on the same
tiles and ppp_register_robust on one whole-cloud handle of the same cloud.  The tiled robust result -- T, every row's words,
used, paired, weight_sum, median and sigma, the statistics and the merged maps -- is asserted equal to the whole-cloud call's,
bit for bit.  Appends one JSON line to profiles/robust_registration_tile_times.jsonl.  No pass/fail condition hangs on a time.

Every step that uses the GPU is a process of its own under `timeout -k 10`, chained with &&: the driver (no --step) starts
`--step tiles`, then `--step whole`, and joins what they wrote; a step that fails or runs out of time ends the run.
usage: python tools/robust_registration_tile_times.py [--reps N] [--config NAME] [--tiles K] [--keep SHARE] [--limit SECONDS]"""
import hashlib
import json
import math
import os
import struct
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

args = sys.argv[1:]
reps, cfg_name, K, share, step, out, limit = 3, "cfg5_10m_s1024", 8, 0.8, None, None, 480
while args:
    if args[0] == "--reps":
        reps = int(args[1])
    elif args[0] == "--config":
        cfg_name = args[1]
    elif args[0] == "--tiles":
        K = int(args[1])
    elif args[0] == "--keep":
        share = float(args[1])
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
BP = dict(tune=4.685, sigma_min=1e-4)
KERNELS = ("k_robt_pair", "k_trimt_narrow<1>", "k_trimt_narrow<2>", "k_robt_terms")


def note(msg):
    print("[robust_registration_tile_times] " + msg, file=sys.stderr, flush=True)


if step is None:
    with tempfile.TemporaryDirectory() as tmp:
        parts = [os.path.join(tmp, s + ".json") for s in ("tiles", "whole")]
        common = "--reps %d --config %s --tiles %d --keep %r" % (reps, cfg_name, K, share)
        me = os.path.abspath(__file__)
        chain = " && ".join("timeout -k 10 %d %s %s %s --step %s --out %s" % (limit, sys.executable, me, common, s, p)
                            for s, p in zip(("tiles", "whole"), parts))
        rc = subprocess.call(chain, shell=True)
        if rc:
            raise SystemExit("a step failed or ran out of time (exit %d): nothing recorded" % rc)
        tiles, whole = (json.load(open(p)) for p in parts)
    assert tiles.pop("signature") == whole.pop("signature"), "the tiled loop and ppp_register_robust disagree"
    line = json.dumps(dict({"tool": "robust_registration_tile_times.py", "config": cfg_name, "tiles": K,
                            "params": dict(RP, iterations=30, min_step=1e-6, lock_eps=1e-9, trimmed_keep=share, **BP), "reps": reps, "equal_bits": True},
                           **dict(tiles, **whole)))
    print(line)
    with open(os.path.join(ROOT, "profiles", "robust_registration_tile_times.jsonl"), "a") as f:
        f.write(line + "\n")
    raise SystemExit(0)

from polishpathplanning_amd import engine, synth  # noqa: E402
from polishpathplanning_amd.robot_path import slice_ranges  # noqa: E402

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
del mm
kw = dict(tool_radius=cfg["tool_radius"], walk=1)
ref = engine.Engine(0, **kw)
ref.set_cloud(ref_pts)
ref.estimate_normals()                                       # first calls of the process: code objects, the index, the normal field
us = lambda ms: round(ms * 1e3, 1)
sha = lambda m: hashlib.sha256(m.tobytes()).hexdigest()


def signature(T, rows, status, weight, residual, st):
    """what both calls must agree on, as JSON keeps it: the doubles by their bits"""
    bits = lambda v: struct.pack("<d", float(v)).hex()
    return [st["steps"], st["converged"], st["locked"], st["pairs_before"], st["pairs_after"], bits(st["rms_before"]), bits(st["rms_after"]),
            T.tobytes().hex(), [int(r["E"]) for r in rows], [r["pairs"] for r in rows], [r["used"] for r in rows], [r["weight_sum"] for r in rows],
            [r["median_bits"] for r in rows], [bits(r["sigma"]) for r in rows], [int(r["locked"]) for r in rows],
            [sha(r["A"]) + sha(r["b"]) for r in rows], sha(status), sha(weight.view(np.uint32)), sha(residual.view(np.uint64))]


if step == "whole":
    scan = engine.Engine(0, **kw)
    scan.set_cloud(moved)
    T, rows, status, weight, residual, st = scan.register_robust(ref, **RP, **BP)
    note("whole-cloud handle ready: %d steps" % st["steps"])
    plain, with_maps, timed = [], [], {}
    for rep in range(reps):
        t0 = time.perf_counter()
        scan.register_robust(ref, maps=False, **RP, **BP)
        plain.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        got = scan.register_robust(ref, **RP, **BP)
        with_maps.append(time.perf_counter() - t0)
        assert signature(*got) == signature(T, rows, status, weight, residual, st)
    scan.enable_timing(True)
    scan.kernel_times()
    for rep in range(reps):
        scan.register_robust(ref, maps=False, **RP, **BP)
        for k, v in scan.kernel_times().items():
            timed[k] = min(timed.get(k, 1e30), v)
    evals = st["steps"] + 1
    res = {"signature": signature(T, rows, status, weight, residual, st), "whole_robust_call_ms": round(min(plain) * 1e3, 3),
           "whole_robust_call_ms_with_maps": round(min(with_maps) * 1e3, 3), "whole_robust_us_per_evaluation": round(min(plain) * 1e6 / evals, 1),
           "whole_robust_kernels_us_per_evaluation": {k: us(timed.get(k, 0.0) / evals) for k in ("k_rob_pair", "k_trim_narrow<1>", "k_trim_narrow<2>", "k_rob_terms")}}
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
    T, rows, statuses, weights, residuals, owneds, st = engine.register_robust_tiles(hs, ref, **RP, **BP)       # the indices, the buffers
    owned = [int(o.sum()) for o in owneds]
    sig = signature(T, rows, *engine.merge_robust_maps(statuses, weights, residuals, owneds), st)
    del statuses, weights, residuals, owneds
    evals = st["steps"] + 1
    note("tiles ready: %d steps" % st["steps"])
    plain, with_maps, trimmed, slowest = [], [], [], {}
    tT, trows, _, _, _, tst = engine.register_trimmed_tiles(hs, ref, keep=share, maps=False, **RP)
    for rep in range(reps):
        t0 = time.perf_counter()
        got = engine.register_robust_tiles(hs, ref, maps=False, **RP, **BP)
        plain.append(time.perf_counter() - t0)
        assert got[0].tobytes() == T.tobytes() and [r["median_bits"] for r in got[1]] == [r["median_bits"] for r in rows]
        t0 = time.perf_counter()
        engine.register_trimmed_tiles(hs, ref, keep=share, maps=False, **RP)
        trimmed.append(time.perf_counter() - t0)
    t0 = time.perf_counter()
    got = engine.register_robust_tiles(hs, ref, **RP, **BP)
    with_maps.append(time.perf_counter() - t0)
    assert signature(got[0], got[1], *engine.merge_robust_maps(*got[2:6]), got[6]) == sig
    del got
    for h in hs:
        h.enable_timing(True)
        h.kernel_times()
    timed_wall = []
    for rep in range(reps):
        t0 = time.perf_counter()
        engine.register_robust_tiles(hs, ref, maps=False, **RP, **BP)
        timed_wall.append(time.perf_counter() - t0)
        per_tile = [h.kernel_times() for h in hs]
        for k in KERNELS:
            slowest[k] = min(slowest.get(k, 1e30), max(t.get(k, 0.0) for t in per_tile) / evals)
    for h in hs:
        h.enable_timing(False)
    per_eval_us = min(plain) * 1e6 / evals
    kernels_us = sum(slowest[k] for k in KERNELS) * 1e3
    res = {"signature": sig, "n_scan": int(len(moved)), "n_ref": int(len(ref_pts)), "raised": int(raised.sum()), "steps": st["steps"],
           "converged": st["converged"], "used_after": rows[-1]["used"], "paired_after": rows[-1]["pairs"], "sigma_after_mm": rows[-1]["sigma"],
           "rms_before_mm": round(st["rms_before"], 5), "rms_after_mm": round(st["rms_after"], 5), "owned": owned,
           "tiles_robust_call_ms": round(min(plain) * 1e3, 3), "tiles_robust_call_ms_with_maps": round(min(with_maps) * 1e3, 3),
           "tiles_robust_call_ms_with_events": round(min(timed_wall) * 1e3, 3), "tiles_robust_us_per_evaluation": round(per_eval_us, 1),
           "slowest_tile_kernels_us_per_evaluation": dict({k: us(slowest[k]) for k in KERNELS}, sum=round(kernels_us, 1)),
           "four_waits_us_per_evaluation_beyond_the_slowest_kernels": round(per_eval_us - kernels_us, 1),
           "per_wait_us": round((per_eval_us - kernels_us) / 4, 1),
           "tiles_trimmed_call_ms": round(min(trimmed) * 1e3, 3), "tiles_trimmed_steps": tst["steps"],
           "tiles_trimmed_us_per_evaluation": round(min(trimmed) * 1e6 / (tst["steps"] + 1), 1)}
    for h in hs:
        h.close()
else:
    raise SystemExit(__doc__)
ref.close()
with open(out, "w") as f:
    json.dump(res, f)
