#!/usr/bin/env python3
"""Event-timed signed distance to a triangle mesh (ppp_trimesh_topology, ppp_get_mesh_signed_deviation): the sheet of
tools/mesh_deviation_times.py as a coarse mesh (1 200 triangles) and a fine one (480 000), given as an STL-like soup so that the
weld has work to do, and that tool's scan of about 1 M points -- per-kernel HIP-event times of the grid build (on the handle that
lends its stream), of the topology build (timed on the scan's handle: the first signed call builds it) and of the search, the sign
launch and the tail of that same call; their launches; and the wall times of ppp_trimesh_create, of ppp_trimesh_topology on a
fresh mesh, of ppp_get_mesh_signed_deviation (topology there) and of ppp_get_mesh_deviation of the same run (statistics only),
best of the repeats, with the maps' and the topology's bits compared between the repeats.
Appends one JSON line to profiles/mesh_signed_times.jsonl.  No pass/fail condition hangs on a time.
usage: python tools/mesh_signed_times.py [--reps N]"""
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


def digest(arrays):
    return hashlib.sha256(b"".join(np.ascontiguousarray(a).tobytes() for a in arrays)).hexdigest()


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
out = {"tool": "mesh_signed_times.py", "n_scan": int(len(pts)), "params": DP, "reps": reps, "meshes": {}}
for name, step in (("coarse", 20), ("fine", 1)):
    verts, tris = grid_mesh(NX, NY, step)
    soup = np.ascontiguousarray(verts[tris.ravel()])      # three vertices per triangle, as an STL file holds them
    mesh = ref.trimesh(soup)                              # first calls of the process: code objects, indices, buffers
    scan.mesh_signed_deviation(mesh, maps=False, **DP)
    scan.mesh_deviation(mesh, maps=False, **DP)
    mesh.close()
    ref.enable_timing(True); scan.enable_timing(True)
    ref.kernel_times(); scan.kernel_times()
    best = {"build": {}, "signed_first": {}, "signed": {}, "plain": {}}
    walls = {k: [] for k in ("build", "topology", "signed_first", "signed", "plain")}
    launches, bits = {}, None
    for rep in range(reps):
        t = time.perf_counter()
        mesh = ref.trimesh(soup)
        walls["build"].append(time.perf_counter() - t)
        kt, launches["build"] = ref.kernel_times(with_launches=True)
        keep(best["build"], kt)
        t = time.perf_counter()
        st = scan.mesh_signed_deviation(mesh, maps=False, **DP)[9]   # builds the topology: its kernels are timed here
        walls["signed_first"].append(time.perf_counter() - t)
        kt, launches["signed_first"] = scan.kernel_times(with_launches=True)
        keep(best["signed_first"], kt)
        t = time.perf_counter()
        scan.mesh_signed_deviation(mesh, maps=False, **DP)
        walls["signed"].append(time.perf_counter() - t)
        kt, launches["signed"] = scan.kernel_times(with_launches=True)
        keep(best["signed"], kt)
        t = time.perf_counter()
        scan.mesh_deviation(mesh, maps=False, **DP)
        walls["plain"].append(time.perf_counter() - t)
        kt, launches["plain"] = scan.kernel_times(with_launches=True)
        keep(best["plain"], kt)
        maps = scan.mesh_signed_deviation(mesh, **DP)[:9]  # (untimed: the maps come down for the comparison)
        topo_stats, topo = mesh.topology()
        h = digest(list(maps) + [topo[k] for k in sorted(topo)])
        assert bits in (None, h)                          # the same bits in every repeat, from a mesh built again
        bits = h
        grid = {k: (list(v) if k == "cells" else v) for k, v in mesh.stats.items() if k not in ("mn", "mx")}
        mesh.close()
        fresh = ref.trimesh(soup)
        t = time.perf_counter()
        fresh.topology(maps=False)                        # the explicit build, alone
        walls["topology"].append(time.perf_counter() - t)
        fresh.close()
        scan.kernel_times(); ref.kernel_times()
    ref.enable_timing(False); scan.enable_timing(False)
    topo_k = {k: v for k, v in best["signed_first"].items() if k.startswith("k_tt_") or k.startswith("trimesh_topology")}
    out["meshes"][name] = {"grid": grid, "topology": topo_stats,
                           "build_kernel_us": us(best["build"]), "build_launches": {k: int(v) for k, v in sorted(launches["build"].items())},
                           "grid_build_kernels_total_us": round(sum(best["build"].values()) * 1e3, 1),
                           "topology_kernel_us": us(topo_k), "topology_kernels_total_us": round(sum(topo_k.values()) * 1e3, 1),
                           "topology_launches": {k: int(v) for k, v in sorted(launches["signed_first"].items()) if k in topo_k},
                           "signed_kernel_us": us(best["signed"]), "signed_launches": {k: int(v) for k, v in sorted(launches["signed"].items())},
                           "plain_kernel_us": us(best["plain"]),
                           "sign_over_search": round(best["signed"]["k_mesh_sign"] / best["signed"]["k_mesh_nearest"], 4),
                           "trimesh_create_call_ms": round(min(walls["build"]) * 1e3, 3), "trimesh_topology_call_ms": round(min(walls["topology"]) * 1e3, 3),
                           "mesh_signed_deviation_first_call_ms": round(min(walls["signed_first"]) * 1e3, 3),
                           "mesh_signed_deviation_call_ms": round(min(walls["signed"]) * 1e3, 3),
                           "mesh_deviation_call_ms": round(min(walls["plain"]) * 1e3, 3),
                           "signed": {k: st[k] for k in ("matched", "too_far", "on_face", "on_edge", "on_vertex", "on_border", "irregular", "fallback", "negative",
                                                         "positive", "mean_dev", "rms_dev", "max_distance")}}
line = json.dumps(out)
print(line)
with open(os.path.join(ROOT, "profiles", "mesh_signed_times.jsonl"), "a") as f:
    f.write(line + "\n")
ref.close(); scan.close()
