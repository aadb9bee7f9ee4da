#!/usr/bin/env python3
"""Event-timed exact deviation (ppp_trimesh_create, ppp_get_mesh_deviation): the 900 x 600 mm sheet of tools/mesh_cloud_times.py as
a coarse mesh (1 200 triangles) and as a fine one (480 000), and a scan of about 1 M points of that sheet (cfg 2's size: the coarse
mesh's samples at pitch 0.735 mm, moved by a seeded +-0.2 mm in x and y and lifted by 0.1 +- 0.05 mm) -- per-kernel HIP-event times
of the grid build (on the handle that lends its stream) and of the search and its tail (on the scan's handle), their launches,
and the wall times of ppp_trimesh_create and of ppp_get_mesh_deviation (statistics only), best of the repeats, with the maps'
bits compared between the repeats.  Beside it, in the same run on the same box: ppp_get_deviation of the same scan against the
ppp_set_cloud_mesh handle of the same mesh at pitch 0.735 (the sampled path: its search, the reference's normal field and the
same tail).  The grid's statistics (cells, pairs, the longest list of a cell) go into the line: they say what the search walks.
Appends one JSON line to profiles/mesh_deviation_times.jsonl.  No pass/fail condition hangs on a time.
usage: python tools/mesh_deviation_times.py [--reps N]"""
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from polishpathplanning_amd import engine, synth  # noqa: E402

args = sys.argv[1:]
reps = 5
while args:
    if args[0] == "--reps":
        reps = int(args[1])
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


def keep(acc, k_ms):
    for k, v in k_ms.items():
        acc[k] = min(acc.get(k, 1e30), v)


def us(d):
    return {k: round(v * 1e3, 1) for k, v in sorted(d.items())}


NX, NY, PITCH = 601, 401, 0.735
DP = dict(max_dist=3.0, allowance=0.05, gain=1.0)
kw = dict(tool_radius=6.0, walk=1)
ref = engine.Engine(0, **kw)                              # takes the meshes in metres, as the files give them
scan = engine.Engine(0, change_range=0, **kw)             # takes the scan in resident millimetres
ref.set_cloud_mesh(*grid_mesh(NX, NY, 20), pitch=PITCH)
rng = np.random.default_rng(31)
pts = ref.cloud().astype(np.float64)
pts[:, :2] += rng.uniform(-0.2, 0.2, (len(pts), 2))
pts[:, 2] += 0.1 + rng.uniform(-0.05, 0.05, len(pts))
scan.set_cloud(pts.astype(np.float32))
out = {"tool": "mesh_deviation_times.py", "n_scan": int(len(pts)), "pitch_mm": PITCH, "params": DP, "reps": reps, "meshes": {}}
for name, step in (("coarse", 20), ("fine", 1)):
    verts, tris = grid_mesh(NX, NY, step)
    sampled = ref.set_cloud_mesh(verts, tris, pitch=PITCH)
    mesh = ref.trimesh(verts, tris)                       # first calls of the process: code objects, indices, buffers
    scan.mesh_deviation(mesh, maps=False, **DP)
    scan.deviation(ref, maps=False, **DP)
    mesh.close()
    ref.enable_timing(True); scan.enable_timing(True)
    ref.kernel_times(); scan.kernel_times()
    best = {"build": {}, "exact": {}, "sampled": {}}
    walls = {k: [] for k in best}
    launches, bits, sampled_sig = {}, None, None
    for rep in range(reps):
        t = time.perf_counter()
        mesh = ref.trimesh(verts, tris)
        walls["build"].append(time.perf_counter() - t)
        kt, launches["build"] = ref.kernel_times(with_launches=True)
        keep(best["build"], kt)
        t = time.perf_counter()
        st = scan.mesh_deviation(mesh, maps=False, **DP)[7]
        walls["exact"].append(time.perf_counter() - t)
        kt, launches["exact"] = scan.kernel_times(with_launches=True)
        keep(best["exact"], kt)
        maps = scan.mesh_deviation(mesh, **DP)[:7]        # (untimed: the maps come down for the comparison)
        h = hashlib.sha256(b"".join(np.ascontiguousarray(m).tobytes() for m in maps)).hexdigest()
        assert bits in (None, h)                          # the same bits in every repeat, from a grid built again
        bits = h
        scan.kernel_times(); ref.kernel_times()
        t = time.perf_counter()
        ss = scan.deviation(ref, maps=False, **DP)[5]
        walls["sampled"].append(time.perf_counter() - t)
        kt, launches["sampled"] = scan.kernel_times(with_launches=True)
        keep(best["sampled"], kt)
        keep(best["sampled"], {"ref:" + k: v for k, v in ref.kernel_times().items()})
        sig = tuple(ss[k] for k in ("matched", "too_far", "no_normal", "min_dev", "max_dev", "mean_dev"))
        assert sampled_sig in (None, sig)
        sampled_sig = sig
        grid = {k: (list(v) if k == "cells" else v) for k, v in mesh.stats.items() if k not in ("mn", "mx")}
        mesh.close()
    ref.enable_timing(False); scan.enable_timing(False)
    out["meshes"][name] = {"grid": grid, "samples_at_pitch": sampled["samples"],
                           "build_kernel_us": us(best["build"]), "build_launches": {k: int(v) for k, v in sorted(launches["build"].items())},
                           "trimesh_create_call_ms": round(min(walls["build"]) * 1e3, 3),
                           "exact_kernel_us": us(best["exact"]), "exact_launches": {k: int(v) for k, v in sorted(launches["exact"].items())},
                           "mesh_deviation_call_ms": round(min(walls["exact"]) * 1e3, 3),
                           "exact": {k: st[k] for k in ("matched", "too_far", "on_face", "on_edge", "on_vertex", "mean_dev", "rms_dev", "max_distance")},
                           "sampled_kernel_us": us(best["sampled"]), "deviation_call_ms": round(min(walls["sampled"]) * 1e3, 3),
                           "sampled": {k: ss[k] for k in ("matched", "too_far", "no_normal", "mean_dev", "rms_dev")}}
line = json.dumps(out)
print(line)
with open(os.path.join(ROOT, "profiles", "mesh_deviation_times.jsonl"), "a") as f:
    f.write(line + "\n")
ref.close(); scan.close()
