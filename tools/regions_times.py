#!/usr/bin/env python3
"""Event-timed region call (ppp_get_regions): per-kernel HIP-event times of its launches and the wall time of the first call
(the size query: no maps copied), best of the repeats, beside the two things a caller can compare it with on the same machine
in the same run:
  (a) the route without the call: the per-point map copied to the host (Engine.path_coverage() flags; for a mask nothing is
      copied) and clustered there with scipy (k-d tree pairs, the float32 link test, connected_components, the rows by numpy);
  (b) the first-call time of ppp_get_path_coverage for the same pass (UNCOVERED workloads only).
Workloads:
  cfg2_uncovered           cfg 2 (1 M points, 256 slices), walk 1, default depth: a few thousand uncovered points
  cfg2_uncovered_released  cfg 2, depth = 1e-7 (the clamp released)
  cfg2_mask30              cfg 2, a seeded 30 % Bernoulli mask
  cfg5_mask30              cfg 5 (10 M points), the same
usage: python tools/regions_times.py [--reps N] [--host-reps N] [--lib libppp_hip_x.so] [workload ...]
(--lib: a tuning build, make variant DEFS=-DPPP_TUNING, which reads PPP_REG_GROUP: the lanes per point of k_reg_link)"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from polishpathplanning_amd import engine, synth  # noqa: E402

WORKLOADS = {
    "cfg2_uncovered": ("cfg2_1m_s256", dict(walk=1), None),
    "cfg2_uncovered_released": ("cfg2_1m_s256", dict(walk=1, depth=1e-7), None),
    "cfg2_mask30": ("cfg2_1m_s256", dict(walk=1), 0.30),
    "cfg5_mask30": ("cfg5_10m_s1024", dict(walk=1), 0.30),
}
LINK = 2.5


def host_regions(P, selected, r):
    """the scipy route: (regions, largest)"""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    from scipy.spatial import cKDTree
    idx = np.nonzero(selected & np.isfinite(P).all(axis=1))[0]
    Q = P[idx]
    if not len(idx):
        return 0, 0
    pairs = cKDTree(Q.astype(np.float64)).query_pairs(r * 1.001, output_type="ndarray")
    d = Q[pairs[:, 0]] - Q[pairs[:, 1]]
    keep = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2] <= np.float32(r) * np.float32(r)
    g = coo_matrix((np.ones(int(keep.sum()), np.int8), (pairs[keep, 0], pairs[keep, 1])), shape=(len(idx), len(idx)))
    ncomp, comp = connected_components(g, directed=False)
    lab = np.full(ncomp, np.iinfo(np.int64).max, np.int64)
    np.minimum.at(lab, comp, idx)
    count = np.bincount(comp, minlength=ncomp)
    mn = np.full((ncomp, 3), np.inf, np.float32); mx = np.full((ncomp, 3), -np.inf, np.float32)
    np.minimum.at(mn, comp, Q); np.maximum.at(mx, comp, Q)
    sums = np.zeros((ncomp, 3), np.int64)
    np.add.at(sums, comp, np.rint(Q.astype(np.float64) * 1048576.0).astype(np.int64))
    labels = np.full(len(P), -1, np.int32)
    labels[idx] = lab[comp]
    return ncomp, int(count.max())


args = sys.argv[1:]
reps, host_reps = 5, 1
while args and args[0].startswith("--"):
    if args[0] == "--reps":
        reps = int(args[1])
    elif args[0] == "--host-reps":
        host_reps = int(args[1])
    elif args[0] == "--lib":
        engine.LIB_PATH = os.path.abspath(args[1])
    else:
        raise SystemExit(__doc__)
    args = args[2:]
L = engine.lib()
for name in args or list(WORKLOADS):
    cfg_name, kw, share = WORKLOADS[name]
    pts, cfg = synth.make_config(cfg_name)
    kw = dict(kw, tool_radius=cfg["tool_radius"])
    h = engine.Engine(0, **kw)
    h.set_cloud(pts)
    h.gen_path()
    mask = None if share is None else (np.random.default_rng(2).random(len(pts)) < share).astype(np.uint8)
    source = engine.REGIONS_UNCOVERED if mask is None else engine.REGIONS_MASK
    mp = None if mask is None else mask.ctypes.data_as(C.POINTER(C.c_ubyte))
    st = engine.RegionStats()

    def call():
        rc = L.ppp_get_regions(h.h, source, mp, 0.0, LINK, None, 0, None, 0, C.byref(st))
        if rc:
            raise engine.PPPError(rc, L.ppp_last_error(h.h).decode())

    call()                                            # first call of the process: code objects, buffers
    h.enable_timing(True)
    best, walls, cov_walls = {}, [], []
    for rep in range(reps):
        if mask is None:
            h.set_cloud(pts)                          # the cloud anew: the coverage call builds the slab index again
            h.gen_path()
            t = time.perf_counter()
            h.path_coverage(flags=False)
            cov_walls.append(time.perf_counter() - t)
        h.kernel_times()
        t = time.perf_counter()
        call()
        walls.append(time.perf_counter() - t)
        for k, v in h.kernel_times().items():
            best[k] = min(best.get(k, 1e30), v)
    P = h.cloud()
    host = []
    for rep in range(host_reps):
        t = time.perf_counter()
        selected = (h.path_coverage()[0] == 0) if mask is None else (mask != 0)
        got = host_regions(P, selected, LINK)
        host.append(time.perf_counter() - t)
    assert not host or got == (st.regions, st.largest), (got, st.regions, st.largest)
    out = {"workload": name, "config": cfg_name, "n": int(len(pts)), "link_mm": LINK, "selected": st.selected, "regions": st.regions,
           "singletons": st.singletons, "largest": st.largest, "window_path": h.fast_path(),
           "group": os.environ.get("PPP_REG_GROUP", "default"),
           "kernel_us": {k: round(v * 1e3, 1) for k, v in sorted(best.items())},
           "kernels_sum_us": round(sum(best.values()) * 1e3, 1),
           "first_call_ms": round(min(walls) * 1e3, 3), "host_scipy_ms": round(min(host) * 1e3, 1) if host else None, "reps": reps}
    if cov_walls:
        out["path_coverage_first_call_ms"] = round(min(cov_walls) * 1e3, 3)
    print(json.dumps(out), flush=True)
    h.close()
