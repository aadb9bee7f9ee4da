#!/usr/bin/env python3
"""Timed mesh calls over slice-range tiles (ppp_register_mesh_tiles, ppp_get_mesh_deviation_tile with
ppp_merge_mesh_deviation_tiles) on the workload of tools/mesh_registration_times.py: the 900 x 600 mm sheet as a coarse mesh
(1 200 triangles) and as a fine one (480 000), and the scan of about 1.03 M points of that sheet, turned by (0.3, -0.2, 1.0)
degrees and shifted by (0.3, -0.2, 0.25) mm -- held as 8 slice-range handles on ONE device, one mesh standing in every slot.

What the tiled loop pays and ppp_register_mesh does not is one host round trip per evaluation: T to every tile, two launches and
a copy back per tile, the wait, the merge and the step.  Per mesh, in one run on one box, best of the repeats, this reports
  - per evaluation the slowest tile's k_mesht_reg_search and k_mesht_reg_sum (HIP events on every tile's handle, in repeats of
    their own: the events cost time) and the rest of the evaluation's wall time beyond the slowest tile's kernels,
  - the whole call ppp_register_mesh_tiles, and beside it ppp_register_mesh on a whole-cloud handle of the same cloud:
    k_mesh_reg_search and k_mesh_reg_sum per evaluation and the whole call,
  - the eight ppp_get_mesh_deviation_tile calls (smooth_radius 1.5 mm) with their kernels, and the host's merge, beside
    ppp_get_mesh_deviation on the whole-cloud handle.
The tiled results are asserted equal to the whole-cloud calls', bit for bit: T, the rows' words, the statistics, every map over
the owned points.  Appends one JSON line per mesh to profiles/mesh_tile_times.jsonl.  No pass/fail condition hangs on a time.

Every step that uses the GPU is a process of its own under `timeout -k 10`, chained with &&: the driver (no --step) starts
`--step tiles`, then `--step whole`, per mesh, and joins what they wrote; a step that fails or runs out of time ends the run.
usage: python tools/mesh_tile_times.py [--reps N] [--tiles K] [--only coarse|fine] [--limit SECONDS]"""
import hashlib
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
reps, K, only, step, out, limit = 3, 8, None, None, None, 420
while args:
    if args[0] == "--reps":
        reps = int(args[1])
    elif args[0] == "--tiles":
        K = int(args[1])
    elif args[0] == "--only":
        only = args[1]
    elif args[0] == "--step":
        step = args[1]
    elif args[0] == "--out":
        out = args[1]
    elif args[0] == "--limit":
        limit = int(args[1])
    else:
        raise SystemExit(__doc__)
    args = args[2:]

NX, NY, PITCH = 601, 401, 0.735
RP = dict(max_dist=2.0, iterations=30, min_step=1e-6, lock_eps=1e-9)
DP = dict(max_dist=2.0, smooth_radius=1.5, allowance=0.05, gain=1.0)
DEG, SHIFT = (0.3, -0.2, 1.0), (0.3, -0.2, 0.25)
MESHES = {"coarse": 20, "fine": 1}


def note(msg):
    print("[mesh_tile_times] " + msg, file=sys.stderr, flush=True)


if step is None:
    lines = []
    for name in MESHES:
        if only not in (None, name):
            continue
        with tempfile.TemporaryDirectory() as tmp:
            parts = [os.path.join(tmp, s + ".json") for s in ("tiles", "whole")]
            common = "--reps %d --tiles %d --only %s" % (reps, K, name)
            me = os.path.abspath(__file__)
            chain = " && ".join("timeout -k 10 %d %s %s %s --step %s --out %s" % (limit, sys.executable, me, common, s, p)
                                for s, p in zip(("tiles", "whole"), parts))
            rc = subprocess.call(chain, shell=True)
            if rc:
                raise SystemExit("a step failed or ran out of time (exit %d): nothing recorded" % rc)
            tiles, whole = (json.load(open(p)) for p in parts)
        assert tiles.pop("register_signature") == whole.pop("register_signature"), "the tiled loop and ppp_register_mesh disagree"
        assert tiles.pop("deviation_signature") == whole.pop("deviation_signature"), "the tiles and ppp_get_mesh_deviation disagree"
        lines.append(json.dumps(dict({"tool": "mesh_tile_times.py", "mesh": name, "tiles": K, "pitch_mm": PITCH, "params": RP, "deviation_params": DP,
                                      "moved_deg": DEG, "moved_mm": SHIFT, "reps": reps, "equal_bits": True}, **dict(tiles, **whole))))
        print(lines[-1])
    with open(os.path.join(ROOT, "profiles", "mesh_tile_times.jsonl"), "a") as f:
        for line in lines:
            f.write(line + "\n")
    raise SystemExit(0)

from polishpathplanning_amd import engine, synth  # noqa: E402
from polishpathplanning_amd.robot_path import slice_ranges  # noqa: E402


def grid_mesh(nx, ny, every):                             # (tools/mesh_registration_times.py's meshes)
    pts = synth.make_plate(nx, ny, kind="wavy", amp=20.0, seed=4, permute=False)
    keep_i, keep_j = np.arange(0, nx, every), np.arange(0, ny, every)
    v = pts.reshape(nx, ny, 3)[np.ix_(keep_i, keep_j)].reshape(-1, 3)
    mx, my = len(keep_i), len(keep_j)
    i, j = np.meshgrid(np.arange(mx - 1), np.arange(my - 1), indexing="ij")
    p = (i * my + j).ravel()
    tris = np.concatenate([np.stack([p, p + my, p + 1], axis=1), np.stack([p + my, p + my + 1, p + 1], axis=1)]).astype(np.int32)
    return np.ascontiguousarray(v), tris


def rotation(deg):
    ax, ay, az = (math.radians(v) for v in deg)
    Rx = np.array([[1, 0, 0], [0, math.cos(ax), -math.sin(ax)], [0, math.sin(ax), math.cos(ax)]])
    Ry = np.array([[math.cos(ay), 0, math.sin(ay)], [0, 1, 0], [-math.sin(ay), 0, math.cos(ay)]])
    Rz = np.array([[math.cos(az), -math.sin(az), 0], [math.sin(az), math.cos(az), 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def register_signature(T, rows, st):
    return [st["steps"], st["converged"], st["locked"], st["pairs_before"], st["pairs_after"], T.tobytes().hex(),
            [int(r["E"]) for r in rows], [r["pairs"] for r in rows], [[int(w) for w in r["A"]] for r in rows[:1]]]


def deviation_signature(maps, stats):
    """the seven maps' bytes and every field of the statistics"""
    h = hashlib.sha256()
    for m in maps:
        h.update(np.ascontiguousarray(m).tobytes())
    flat = {k: (np.asarray(v).tobytes().hex() if k == "hist" else np.array([v]).tobytes().hex()) for k, v in sorted(stats.items())}
    return [h.hexdigest(), flat]


def keep(acc, k_ms):
    for k, v in k_ms.items():
        acc[k] = min(acc.get(k, 1e30), v)


us = lambda d: {k: round(v * 1e3, 1) for k, v in sorted(d.items())}
kw = dict(tool_radius=6.0, walk=1)
ref = engine.Engine(0, **kw)                              # takes the meshes in metres, as the files give them
ref.set_cloud_mesh(*grid_mesh(NX, NY, 20), pitch=PITCH)
rng = np.random.default_rng(31)
pts = ref.cloud().astype(np.float64)
pts[:, :2] += rng.uniform(-0.2, 0.2, (len(pts), 2))
pts[:, 2] += 0.1 + rng.uniform(-0.05, 0.05, len(pts))
c = 0.5 * (pts.min(axis=0) + pts.max(axis=0))
pts = ((pts - c) @ rotation(DEG).T + c + np.asarray(SHIFT)).astype(np.float32)
verts, tris = grid_mesh(NX, NY, MESHES[only])
mesh = ref.trimesh(verts, tris)
skw = dict(change_range=0, **kw)                          # the scan in resident millimetres

if step == "whole":
    scan = engine.Engine(0, **skw)
    scan.set_cloud(pts)
    T, rows, st = scan.register_mesh(mesh, **RP)          # first calls of the process: code objects, the index, the buffers
    whole_dev = scan.mesh_deviation(mesh, **DP)
    evals = st["steps"] + 1
    note("whole-cloud handle ready: %d steps" % st["steps"])
    walls, dwalls, timed, dtimed = [], [], {}, {}
    for rep in range(reps):
        t0 = time.perf_counter()
        got = scan.register_mesh(mesh, **RP)
        walls.append(time.perf_counter() - t0)
        assert register_signature(*got) == register_signature(T, rows, st)
        t0 = time.perf_counter()
        scan.mesh_deviation(mesh, maps=False, **DP)
        dwalls.append(time.perf_counter() - t0)
    scan.enable_timing(True)
    scan.kernel_times()
    for rep in range(reps):
        scan.register_mesh(mesh, **RP)
        keep(timed, scan.kernel_times())
        scan.mesh_deviation(mesh, maps=False, **DP)
        keep(dtimed, scan.kernel_times())
    res = {"register_signature": register_signature(T, rows, st), "deviation_signature": deviation_signature(whole_dev[:7], whole_dev[7]),
           "whole_register_mesh_call_ms": round(min(walls) * 1e3, 3),
           "whole_us_per_evaluation": {k: round(timed.get(k, 0.0) * 1e3 / evals, 1) for k in ("k_mesh_reg_search", "k_mesh_reg_sum")},
           "whole_mesh_deviation_call_ms_without_maps": round(min(dwalls) * 1e3, 3), "whole_mesh_deviation_kernel_us": us(dtimed)}
    scan.close()
elif step == "tiles":
    first = engine.Engine(0, **skw)
    _, _, S = first.range_interval(float(pts[:, 0].min()), float(pts[:, 0].max()))
    first.close()
    hs = []
    for b, e in slice_ranges(S, K):
        h = engine.Engine(0, slice_begin=b, slice_end=e, **skw)
        h.set_cloud(pts)
        hs.append(h)
        note("tile %d of %d set: slices [%d, %d) of %d" % (len(hs), K, b, e, S))
    T, rows, st = engine.register_mesh_tiles(hs, mesh, **RP)  # the indices, the buffers
    evals = st["steps"] + 1
    note("tiles ready: %d steps" % st["steps"])
    walls, timed_walls, slowest = [], [], {}
    for rep in range(reps):
        t0 = time.perf_counter()
        got = engine.register_mesh_tiles(hs, mesh, **RP)
        walls.append(time.perf_counter() - t0)
        assert register_signature(*got) == register_signature(T, rows, st)
    for h in hs:
        h.enable_timing(True)
        h.kernel_times()
    for rep in range(reps):
        t0 = time.perf_counter()
        engine.register_mesh_tiles(hs, mesh, **RP)
        timed_walls.append(time.perf_counter() - t0)
        per_tile = [h.kernel_times() for h in hs]
        keep(slowest, {k: max(t.get(k, 0.0) for t in per_tile) / evals for k in ("k_mesht_reg_search", "k_mesht_reg_sum")})
    for h in hs:
        h.enable_timing(False)
    parts = [h.mesh_registration_terms_tile(mesh, T=T, max_dist=RP["max_dist"])[1] for h in hs]
    # the deviation: eight tile calls with maps and the merge; then without maps, timed; then the kernels
    tiles = [h.mesh_deviation_tile(mesh, **DP) for h in hs]
    t0 = time.perf_counter()
    merged = engine.merge_mesh_deviation_tiles(tiles)
    merge_ms = (time.perf_counter() - t0) * 1e3
    n = len(pts)
    fill = (np.full(n, np.nan), np.full(n, np.nan), np.full(n, np.nan), np.full(n, -1, np.int32), np.full(n, 255, np.uint8), np.full(n, 3, np.uint8),
            np.zeros(n))
    owners = np.zeros(n, np.int32)
    for t in tiles:
        mine = t[7] == 1
        owners += mine
        for dst, src in zip(fill, t[:7]):
            dst[mine] = src[mine]
            assert src.dtype == dst.dtype
    assert owners.max() == 1 and owners.sum() == sum(t[8]["owned"] for t in tiles)
    dwalls, dtimed = [], {}
    for rep in range(reps):
        t0 = time.perf_counter()
        for h in hs:
            h.mesh_deviation_tile(mesh, maps=False, **DP)
        dwalls.append(time.perf_counter() - t0)
    for h in hs:
        h.enable_timing(True)
        h.kernel_times()
    for rep in range(reps):
        for h in hs:
            h.mesh_deviation_tile(mesh, maps=False, **DP)
        per_tile = [h.kernel_times() for h in hs]
        keep(dtimed, {k: max(t.get(k, 0.0) for t in per_tile) for k in per_tile[0]})
    per_eval_us = min(walls) * 1e6 / evals
    kernels_us = sum(slowest.values()) * 1e3
    res = {"register_signature": register_signature(T, rows, st), "deviation_signature": deviation_signature(fill, merged),
           "n_scan": int(n), "triangles": int(len(tris)), "slices": int(S), "steps": st["steps"], "converged": st["converged"],
           "pairs_after": st["pairs_after"], "rms_before_mm": round(st["rms_before"], 5), "rms_after_mm": round(st["rms_after"], 5),
           "owned": [p["owned"] for p in parts], "evaluated": [p["evaluated"] for p in parts],
           "tiles_register_mesh_call_ms": round(min(walls) * 1e3, 3), "tiles_register_mesh_call_ms_with_events": round(min(timed_walls) * 1e3, 3),
           "tiles_us_per_evaluation": round(per_eval_us, 1), "slowest_tile_us_per_evaluation": us(slowest),
           "round_trip_us_per_evaluation_beyond_the_slowest_tile_kernels": round(per_eval_us - kernels_us, 1),
           "deviation_evaluated": [t[8]["evaluated"] for t in tiles],
           "tiles_mesh_deviation_calls_ms_without_maps": round(min(dwalls) * 1e3, 3), "slowest_tile_mesh_deviation_kernel_us": us(dtimed),
           "host_merge_ms_through_python": round(merge_ms, 3)}
    for h in hs:
        h.close()
else:
    raise SystemExit(__doc__)
mesh.close(); ref.close()
with open(out, "w") as f:
    json.dump(res, f)
