#!/usr/bin/env python3
"""Event-timed global registration against the triangles (ppp_register_mesh_global) on the workload of
tools/mesh_registration_times.py: the 900 x 600 mm sheet as a coarse mesh (1 200 triangles) and as a fine one (480 000), and a scan
of about 1.03 M points of that sheet (the coarse mesh's samples at pitch 0.735 mm, jittered as there), moved by the motion of
tools/global_registration_times.py -- (130, 25, -160) degrees about the scan's centre and (40, -25, 60) mm --, the default
parameters (24 starts, stride 16, coarse 10 mm / 8 iterations).  Per mesh, in one run on one box, best of the repeats, per-kernel
HIP-event times on the scan's handle:
  - the call (wall time), the coarse stage as a whole (the compaction, k_mesh_reg_search_multi, k_mesh_reg_sum_multi,
    k_reg_step_multi) and per multi evaluation the search and the sum separately, at the default stride and at stride 1;
  - k_mesh_moments (inside the global call, on the scan's stream, under its event timers), TriMesh.moments() as a whole call (the
    same kernel on the mesh's own stream with its clear, its copy and its wait) and the fine chain (k_mesh_reg_search,
    k_mesh_reg_sum, k_reg_step inside the global call);
  - the same K chains as K ppp_register_mesh calls one after the other from the same starts at stride 1 with `coarse` -- the bits
    are asserted equal -- as kernel time beside the side-by-side stage's;
  - the old route in the same run: ppp_set_cloud_mesh of the mesh at pitch 0.735 on a second handle, ppp_register_global against
    those samples (with the samples' normal field, which every call rebuilds after the cloud was set), ppp_register_mesh from its
    result.
Appends one JSON line per mesh to profiles/mesh_global_registration_times.jsonl.  No pass/fail condition hangs on a time.
usage: python tools/mesh_global_registration_times.py [--reps N] [--only coarse|fine]"""
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
reps, only = 5, None
while args:
    if args[0] == "--reps":
        reps = int(args[1])
    elif args[0] == "--only":
        only = args[1]
    else:
        raise SystemExit(__doc__)
    args = args[2:]


def grid_mesh(nx, ny, step):                              # (tools/mesh_cloud_times.py's meshes)
    pts = synth.make_plate(nx, ny, kind="wavy", amp=20.0, seed=4, permute=False)
    keep_i, keep_j = np.arange(0, nx, step), np.arange(0, ny, step)
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


def keep(acc, k_ms):
    for k, v in k_ms.items():
        acc[k] = min(acc.get(k, 1e30), v)


def us(d):
    return {k: round(v * 1e3, 1) for k, v in sorted(d.items())}


NX, NY, PITCH = 601, 401, 0.735
COARSE = dict(max_dist=10.0, iterations=8, min_step=1e-3, lock_eps=1e-9)
DEG, SHIFT = (130.0, 25.0, -160.0), (40.0, -25.0, 60.0)
EVALS = COARSE["iterations"] + 1
kw = dict(tool_radius=6.0, walk=1)
ref = engine.Engine(0, **kw)                              # takes the meshes in metres, as the files give them
scan = engine.Engine(0, change_range=0, **kw)             # takes the scan in resident millimetres
ref.set_cloud_mesh(*grid_mesh(NX, NY, 20), pitch=PITCH)
rng = np.random.default_rng(31)
pts = ref.cloud().astype(np.float64)
pts[:, :2] += rng.uniform(-0.2, 0.2, (len(pts), 2))
pts[:, 2] += 0.1 + rng.uniform(-0.05, 0.05, len(pts))
c = 0.5 * (pts.min(axis=0) + pts.max(axis=0))
pts = (pts - c) @ rotation(DEG).T + c + np.asarray(SHIFT)
scan.set_cloud(pts.astype(np.float32))
coarse_of = lambda d: sum(v for k, v in d.items() if k.startswith("k_compact") or k.endswith("_multi"))
lines = []
for name, step in (("coarse", 20), ("fine", 1)):
    if only not in (None, name):
        continue
    verts, tris = grid_mesh(NX, NY, step)
    mesh = scan.trimesh(verts * np.float32(1000.0), tris)  # resident millimetres, as the scan's handle takes them
    g16 = scan.register_mesh_global(mesh)                 # first calls of the process: code objects, indices, buffers
    scan.register_mesh_global(mesh, stride=1)
    scan.register_mesh(mesh, T0=g16[1][0]["T0"], rows=False, **COARSE)
    ref.set_cloud_mesh(verts, tris, pitch=PITCH)
    scan.register_global(ref)
    mesh.moments()
    ref.enable_timing(True); scan.enable_timing(True)
    ref.kernel_times(); scan.kernel_times()
    best = {"stride16": {}, "stride1": {}, "serial": {}, "old_global": {}, "old_mesh": {}, "old_sample": {}}
    walls = {k: [] for k in ("stride16", "stride1", "serial", "moments", "old_sample", "old_global", "old_mesh")}
    launches, sig, got = {}, {}, {}
    for rep in range(reps):
        for key, stride in (("stride16", 16), ("stride1", 1)):
            t = time.perf_counter()
            out = scan.register_mesh_global(mesh, stride=stride)
            walls[key].append(time.perf_counter() - t)
            kt, launches[key] = scan.kernel_times(with_launches=True)
            keep(best[key], kt)
            s = (out[3]["winner"], out[3]["winner_cost"], out[3]["second_cost"], out[0].tobytes())
            assert sig.get(key) in (None, s)              # the same bits in every repeat
            sig[key], got[key] = s, out
        t = time.perf_counter()
        mesh.moments()
        walls["moments"].append(time.perf_counter() - t)
        t = time.perf_counter()
        serial = {}
        for cd in got["stride1"][1]:
            Tk, rk, sk = scan.register_mesh(mesh, T0=cd["T0"], **COARSE)
            # stride 1: each coarse chain is ppp_register_mesh from that start, bit for bit
            assert Tk.tobytes() == cd["T"].tobytes() and (sk["steps"], rk[-1]["pairs"], rk[-1]["E"]) == (cd["steps"], cd["pairs"], cd["E"])
            for k, v in scan.kernel_times().items():
                serial[k] = serial.get(k, 0.0) + v
        walls["serial"].append(time.perf_counter() - t)
        keep(best["serial"], serial)
        # the old route: sample the mesh onto a second handle, register globally against the samples, then against the facets
        ref.kernel_times()
        t = time.perf_counter()
        ref.set_cloud_mesh(verts, tris, pitch=PITCH)
        walls["old_sample"].append(time.perf_counter() - t)
        keep(best["old_sample"], ref.kernel_times())
        t = time.perf_counter()
        old = scan.register_global(ref)
        walls["old_global"].append(time.perf_counter() - t)
        keep(best["old_global"], scan.kernel_times())
        keep(best["old_global"], {"ref:" + k: v for k, v in ref.kernel_times().items()})
        t = time.perf_counter()
        Tm, _, sm = scan.register_mesh(mesh, T0=old[0], rows=False)
        walls["old_mesh"].append(time.perf_counter() - t)
        keep(best["old_mesh"], scan.kernel_times())
    ref.enable_timing(False); scan.enable_timing(False)

    def stage(key):
        d, g = best[key], got[key]
        return {"queries": g[3]["queries"], "shift": g[3]["shift"], "winner": g[3]["winner"], "winner_cost": g[3]["winner_cost"],
                "second_cost": g[3]["second_cost"], "coarse_steps": [cd["steps"] for cd in g[1]], "fine_steps": g[3]["fine"]["steps"],
                "fine_converged": g[3]["fine"]["converged"], "fine_rms_after_mm": g[3]["fine"]["rms_after"],
                "kernel_us": us(d), "kernel_launches": {k: int(v) for k, v in sorted(launches[key].items())},
                "coarse_stage_us": round(coarse_of(d) * 1e3, 1),
                "k_mesh_reg_search_multi_us_per_evaluation": round(d.get("k_mesh_reg_search_multi", 0.0) * 1e3 / EVALS, 1),
                "k_mesh_reg_sum_multi_us_per_evaluation": round(d.get("k_mesh_reg_sum_multi", 0.0) * 1e3 / EVALS, 1),
                "fine_chain_us": round(sum(d.get(k, 0.0) for k in ("k_mesh_reg_search", "k_mesh_reg_sum", "k_reg_step")) * 1e3, 1),
                "k_cloud_moments_us": round(d.get("k_cloud_moments", 0.0) * 1e3, 1),
                "k_mesh_moments_us": round(d.get("k_mesh_moments", 0.0) * 1e3, 1), "call_ms": round(min(walls[key]) * 1e3, 3)}

    ms = lambda k: round(min(walls[k]) * 1e3, 3)
    side = sum(best["stride1"].get(k, 0.0) for k in ("k_mesh_reg_search_multi", "k_mesh_reg_sum_multi", "k_reg_step_multi"))
    one = sum(best["serial"].get(k, 0.0) for k in ("k_mesh_reg_search", "k_mesh_reg_sum", "k_reg_step"))
    grid = {k: (list(v) if k == "cells" else v) for k, v in mesh.stats.items() if k not in ("mn", "mx")}
    out = {"tool": "mesh_global_registration_times.py", "mesh": name, "n_scan": int(len(pts)), "candidates": 24, "coarse": COARSE,
           "moved_deg": DEG, "moved_mm": SHIFT, "reps": reps, "grid": grid, "stride16": stage("stride16"), "stride1": stage("stride1"),
           "trimesh_moments_call_ms": ms("moments"),
           "one_after_the_other_stride1": {"kernel_us": us(best["serial"]), "chains_us": round(one * 1e3, 1), "calls_ms": ms("serial")},
           "side_by_side_stride1_chains_us": round(side * 1e3, 1), "side_by_side_over_one_after_the_other": round(side / one, 3) if one else None,
           "old_route": {"pitch_mm": PITCH, "samples": int(len(ref.cloud())), "set_cloud_mesh_call_ms": ms("old_sample"),
                         "register_global_call_ms": ms("old_global"), "register_mesh_call_ms": ms("old_mesh"),
                         "total_ms": round(ms("old_sample") + ms("old_global") + ms("old_mesh"), 3),
                         "register_global_kernel_us": us(best["old_global"]), "register_mesh_kernel_us": us(best["old_mesh"]),
                         "winner": old[3]["winner"], "fine_converged": sm["converged"], "rms_after_mm": sm["rms_after"]}}
    lines.append(json.dumps(out))
    print(lines[-1])
    mesh.close()
with open(os.path.join(ROOT, "profiles", "mesh_global_registration_times.jsonl"), "a") as f:
    for ln in lines:
        f.write(ln + "\n")
ref.close(); scan.close()
