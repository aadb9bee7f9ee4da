#!/usr/bin/env python3
"""Event-timed robust registration against the triangles (ppp_get_mesh_robust_registration_terms, ppp_register_mesh_robust) on
the workload of tools/mesh_registration_times.py -- the 900 x 600 mm sheet as a coarse mesh (1 200 triangles) and as a fine one
(480 000), a scan of about 1 M points of it, turned and shifted -- with the eighth of the scan at the low end of x raised by
1.5 mm: the clamp pad.  Per mesh, in one run on one box, best of the repeats: one evaluation at the identity per kernel
(k_mesh_rob_pair, k_mesh_rob_digit0 unless the build is MESH_ROB_DIGIT_PASS=0, k_trim_narrow<1>, <2>, k_mesh_rob_terms) beside
ppp_get_mesh_registration_terms' k_mesh_reg_search and k_mesh_reg_sum over the same queries; the whole call ppp_register_mesh_robust
(wall time, its kernels' sums and launches) beside ppp_register_mesh on the same inputs and ppp_register_robust against the same
mesh sampled at pitch 0.735.  The bytes of T are compared between the repeats.  Appends one JSON line per mesh to
profiles/mesh_robust_registration_times.jsonl.  No pass/fail condition hangs on a time.
usage: python tools/mesh_robust_registration_times.py [--reps N] [--lib libppp_hip_x.so] [--only coarse|fine] [--evals-only]
--lib: a tuning build (make variant NAME=x DEFS="-DMESH_ROB_DIGIT_PASS=0", "-DMESH_ROB_GRID_CUS=4"); --evals-only: no whole calls"""
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
reps, only, evals_only = 5, None, False
while args:
    if args[0] == "--reps":
        reps = int(args[1]); args = args[2:]
    elif args[0] == "--lib":
        engine.LIB_PATH = os.path.join(os.path.dirname(engine.LIB_PATH), args[1]); args = args[2:]
    elif args[0] == "--only":
        only = args[1]; args = args[2:]
    elif args[0] == "--evals-only":
        evals_only = True; args = args[1:]
    else:
        raise SystemExit(__doc__)


def grid_mesh(nx, ny, step):                              # (tools/mesh_registration_times.py's meshes)
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
RP = dict(max_dist=2.0, iterations=30, min_step=1e-6, lock_eps=1e-9)
BP = dict(RP, tune=4.685, sigma_min=1e-4)
DEG, SHIFT = (0.3, -0.2, 1.0), (0.3, -0.2, 0.25)
RAISED_SHARE, RAISE_MM = 0.125, 1.5
kw = dict(tool_radius=6.0, walk=1)
ref = engine.Engine(0, **kw)                              # takes the meshes in metres, as the files give them
scan = engine.Engine(0, change_range=0, **kw)             # takes the scan in resident millimetres
ref.set_cloud_mesh(*grid_mesh(NX, NY, 20), pitch=PITCH)
rng = np.random.default_rng(31)
pts = ref.cloud().astype(np.float64)
pts[:, :2] += rng.uniform(-0.2, 0.2, (len(pts), 2))
pts[:, 2] += 0.1 + rng.uniform(-0.05, 0.05, len(pts))
raised = pts[:, 0] < pts[:, 0].min() + RAISED_SHARE * (pts[:, 0].max() - pts[:, 0].min())
pts[raised, 2] += RAISE_MM
c = 0.5 * (pts.min(axis=0) + pts.max(axis=0))
R = rotation(DEG)
pts = (pts - c) @ R.T + c + np.asarray(SHIFT)
scan.set_cloud(pts.astype(np.float32))
sstat = lambda s: {k: s[k] for k in ("steps", "converged", "locked", "pairs_before", "pairs_after", "rms_before", "rms_after")}
lines = []
for name, step in (("coarse", 20), ("fine", 1)):
    if only not in (None, name):
        continue
    verts, tris = grid_mesh(NX, NY, step)
    sampled = ref.set_cloud_mesh(verts, tris, pitch=PITCH)
    mesh = ref.trimesh(verts, tris)                       # first calls of the process: code objects, indices, buffers
    scan.mesh_robust_registration_terms(mesh, maps=False, max_dist=RP["max_dist"])
    scan.mesh_registration_terms(mesh, max_dist=RP["max_dist"])
    if not evals_only:
        scan.register_mesh_robust(mesh, maps=False, **BP)
        scan.register_mesh(mesh, rows=False, **RP)
        scan.register_robust(ref, maps=False, **BP)
    ref.enable_timing(True); scan.enable_timing(True)
    ref.kernel_times(); scan.kernel_times()
    best = {"terms": {}, "plain_terms": {}, "chain": {}, "plain": {}, "sampled": {}}
    walls = {"chain": [], "plain": [], "sampled": []}
    launches, bits, row0, prow0, out_r, out_p, out_s = {}, {}, None, None, None, None, None
    for rep in range(reps):
        row0 = scan.mesh_robust_registration_terms(mesh, maps=False, max_dist=RP["max_dist"])[0]
        kt, launches["terms"] = scan.kernel_times(with_launches=True)
        keep(best["terms"], kt)
        prow0, _ = scan.mesh_registration_terms(mesh, max_dist=RP["max_dist"])
        kt, launches["plain_terms"] = scan.kernel_times(with_launches=True)
        keep(best["plain_terms"], kt)
        assert prow0["pairs"] == row0["pairs"]            # the same queries, the same bound
        if evals_only:
            continue
        for key, call in (("chain", lambda: scan.register_mesh_robust(mesh, maps=False, **BP)), ("plain", lambda: scan.register_mesh(mesh, rows=False, **RP)),
                          ("sampled", lambda: scan.register_robust(ref, maps=False, **BP))):
            ref.kernel_times()
            t = time.perf_counter()
            res = call()
            walls[key].append(time.perf_counter() - t)
            kt, launches[key] = scan.kernel_times(with_launches=True)
            keep(best[key], kt)
            if key == "sampled":
                keep(best[key], {"ref:" + k: v for k, v in ref.kernel_times().items()})
            assert bits.get(key) in (None, res[0].tobytes())  # the same bits in every repeat
            bits[key] = res[0].tobytes()
            if key == "chain":
                out_r = res
            elif key == "plain":
                out_p = res
            else:
                out_s = res
    ref.enable_timing(False); scan.enable_timing(False)
    grid = {k: (list(v) if k == "cells" else v) for k, v in mesh.stats.items() if k not in ("mn", "mx")}
    out = {"tool": "mesh_robust_registration_times.py", "lib": os.path.basename(engine.LIB_PATH), "mesh": name, "n_scan": int(len(pts)),
           "raised": int(raised.sum()), "raise_mm": RAISE_MM, "pitch_mm": PITCH, "params": BP, "moved_deg": DEG, "moved_mm": SHIFT, "reps": reps, "grid": grid,
           "pairs_at_identity": row0["pairs"], "used_at_identity": row0["used"],
           "terms_kernel_us": us(best["terms"]), "terms_launches": {k: int(v) for k, v in sorted(launches["terms"].items())},
           "mesh_registration_terms_kernel_us": us(best["plain_terms"])}
    if not evals_only:
        last = out_r[1][-1]
        out.update({"samples_at_pitch": sampled["samples"],
                    "register_mesh_robust_call_ms": round(min(walls["chain"]) * 1e3, 3), "register_mesh_robust_kernel_us": us(best["chain"]),
                    "register_mesh_robust_launches": {k: int(v) for k, v in sorted(launches["chain"].items())},
                    "register_mesh_robust": dict(sstat(out_r[5]), used=last["used"], median_abs=last["median_abs"], sigma=last["sigma"]),
                    "register_mesh_call_ms": round(min(walls["plain"]) * 1e3, 3), "register_mesh_kernel_us": us(best["plain"]),
                    "register_mesh": sstat(out_p[2]),
                    "register_robust_call_ms": round(min(walls["sampled"]) * 1e3, 3), "register_robust_kernel_us": us(best["sampled"]),
                    "register_robust": sstat(out_s[5])})
    mesh.close()
    lines.append(json.dumps(out))
    print(lines[-1])
with open(os.path.join(ROOT, "profiles", "mesh_robust_registration_times.jsonl"), "a") as f:
    for line in lines:
        f.write(line + "\n")
ref.close(); scan.close()
