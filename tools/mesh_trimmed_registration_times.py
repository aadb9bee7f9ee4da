#!/usr/bin/env python3
"""Event-timed trimmed registration against the triangles (ppp_get_mesh_trimmed_registration_terms, ppp_register_mesh_trimmed) on
the workload of tools/mesh_robust_registration_times.py -- the 900 x 600 mm sheet as a coarse mesh (1 200 triangles) and as a fine
one (480 000), a scan of about 1 M points of it, turned and shifted, the eighth of the scan at the low end of x raised by 1.5 mm.
Per mesh, in one run on one box: one evaluation at the identity per kernel under PPP_MESH_BORDER_PAIR and under _REJECT
(k_mesh_trim_pair<pair> / <reject>, k_mesh_trim_digit0, k_trim_narrow<1>, <2>, k_mesh_trim_terms, k_mesh_trim_scatter), best of the
repeats, beside ppp_get_mesh_robust_registration_terms' and ppp_get_mesh_registration_terms' kernels over the same queries; the
whole calls ppp_register_mesh_trimmed under either rule (wall time of every repeat, its kernels' sums and launches) beside
ppp_register_mesh_robust and ppp_register_mesh on the same inputs.  The topology is built before the timed repeats (its cost is
tools/mesh_signed_times.py's subject).  The bytes of T are compared between the repeats.  Appends one JSON line per mesh to
profiles/mesh_trimmed_registration_times.jsonl.  No pass/fail condition hangs on a time.
usage: python tools/mesh_trimmed_registration_times.py [--reps N] [--lib libppp_hip_x.so] [--only coarse|fine] [--evals-only]
--lib: a tuning build (make variant NAME=x DEFS="-DMESH_TRIM_GRID_CUS=4"); --evals-only: no whole calls"""
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


def keep_best(acc, k_ms):
    for k, v in k_ms.items():
        acc[k] = min(acc.get(k, 1e30), v)


def us(d):
    return {k: round(v * 1e3, 1) for k, v in sorted(d.items())}


NX, NY, PITCH = 601, 401, 0.735
RP = dict(max_dist=2.0, iterations=30, min_step=1e-6, lock_eps=1e-9)
BP = dict(RP, tune=4.685, sigma_min=1e-4)
KEEP = 0.8
PAIR, REJECT = engine.MESH_BORDER_PAIR, engine.MESH_BORDER_REJECT
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
spread = lambda w: {"best_ms": round(min(w) * 1e3, 3), "worst_ms": round(max(w) * 1e3, 3)}
lines = []
for name, step in (("coarse", 20), ("fine", 1)):
    if only not in (None, name):
        continue
    verts, tris = grid_mesh(NX, NY, step)
    mesh = ref.trimesh(verts, tris)                       # first calls of the process: code objects, indices, buffers, the topology
    topo = mesh.topology(maps=False)[0]
    evals = {"pair": lambda: scan.mesh_trimmed_registration_terms(mesh, keep=KEEP, border=PAIR, maps=False, max_dist=RP["max_dist"]),
             "reject": lambda: scan.mesh_trimmed_registration_terms(mesh, keep=KEEP, border=REJECT, maps=False, max_dist=RP["max_dist"]),
             "robust": lambda: scan.mesh_robust_registration_terms(mesh, maps=False, max_dist=RP["max_dist"]),
             "plain": lambda: scan.mesh_registration_terms(mesh, max_dist=RP["max_dist"])}
    calls = {"pair": lambda: scan.register_mesh_trimmed(mesh, keep=KEEP, border=PAIR, maps=False, **RP),
             "reject": lambda: scan.register_mesh_trimmed(mesh, keep=KEEP, border=REJECT, maps=False, **RP),
             "robust": lambda: scan.register_mesh_robust(mesh, maps=False, **BP),
             "plain": lambda: scan.register_mesh(mesh, rows=False, **RP)}
    for f in evals.values():
        f()
    if not evals_only:
        for f in calls.values():
            f()
    scan.enable_timing(True)
    scan.kernel_times()
    best_e, best_c = {k: {} for k in evals}, {k: {} for k in calls}
    walls = {k: [] for k in calls}
    launches_e, launches_c, bits, rows0, outs = {}, {}, {}, {}, {}
    for rep in range(reps):
        for key, f in evals.items():
            rows0[key] = f()[0]
            kt, launches_e[key] = scan.kernel_times(with_launches=True)
            keep_best(best_e[key], kt)
        assert rows0["pair"]["paired"] == rows0["plain"]["pairs"] == rows0["robust"]["pairs"]     # the same queries, the same bound
        assert rows0["reject"]["paired"] + rows0["reject"]["on_border"] == rows0["pair"]["paired"]
        if evals_only:
            continue
        for key, f in calls.items():
            t = time.perf_counter()
            res = f()
            walls[key].append(time.perf_counter() - t)
            kt, launches_c[key] = scan.kernel_times(with_launches=True)
            keep_best(best_c[key], kt)
            assert bits.get(key) in (None, res[0].tobytes())  # the same bits in every repeat
            bits[key] = res[0].tobytes()
            outs[key] = res
    scan.enable_timing(False)
    grid = {k: (list(v) if k == "cells" else v) for k, v in mesh.stats.items() if k not in ("mn", "mx")}
    out = {"tool": "mesh_trimmed_registration_times.py", "lib": os.path.basename(engine.LIB_PATH), "mesh": name, "n_scan": int(len(pts)),
           "raised": int(raised.sum()), "raise_mm": RAISE_MM, "keep": KEEP, "params": RP, "robust_params": BP, "moved_deg": DEG, "moved_mm": SHIFT, "reps": reps,
           "grid": grid, "border_edges": topo["border_edges"], "closed": topo["closed"],
           "at_identity": {k: {f: rows0[k][f] for f in ("pairs", "paired", "on_border")} for k in ("pair", "reject")},
           "terms_kernel_us": {k: us(best_e[k]) for k in evals}, "terms_kernel_sum_us": {k: round(sum(best_e[k].values()) * 1e3, 1) for k in evals},
           "terms_launches": {k: {n: int(v) for n, v in sorted(launches_e[k].items())} for k in evals}}
    if not evals_only:
        out["calls"] = {}
        for key in calls:
            res = outs[key]
            st = res[-1]
            d = dict(spread(walls[key]), kernel_us=us(best_c[key]), kernel_sum_us=round(sum(best_c[key].values()) * 1e3, 1),
                     launches={n: int(v) for n, v in sorted(launches_c[key].items())}, stats=sstat(st))
            if key in ("pair", "reject"):
                last = res[1][-1]
                d.update(kept=last["pairs"], paired=last["paired"], on_border=last["on_border"], trim_d2=last["trim_d2"])
            out["calls"][key] = d
    mesh.close()
    lines.append(json.dumps(out))
    print(lines[-1])
with open(os.path.join(ROOT, "profiles", "mesh_trimmed_registration_times.jsonl"), "a") as f:
    for line in lines:
        f.write(line + "\n")
ref.close(); scan.close()
