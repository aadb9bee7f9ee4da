"""Child process of tests/test_scatter_forms.py: plans the test's clouds under ONE form of the window path's binning launch and leaves
the results in an .npz.  The form is forced by PPP_WIN_SCAT_T / PPP_WIN_PPT in the environment, which the tuning build of the engine
reads once per plan (libppp_hip_tune.so, -DPPP_TUNING); the process is fresh, so nothing has touched the GPU before the variables
are in place.  The test process imports this module for its clouds only: importing it changes nothing (the tuning library is chosen
in main()).  usage: scatter_forms_child.py out.npz case[,case...]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
from polishpathplanning_amd import engine, synth

EDGE_PLATES = {1: (2, 2), 700: (30, 24), 2047: (66, 32), 2048: (66, 32), 2049: (66, 32), 4099: (66, 64),
               8191: (130, 64), 8192: (130, 64), 8193: (130, 64), 16387: (130, 128)}


def edge_cloud(n):
    """a dense plate cut to exactly n points (the plate comes permuted: the cut leaves scattered holes, not a missing edge)"""
    nx, ny = EDGE_PLATES[n]
    return np.ascontiguousarray(synth.make_plate(nx, ny, kind="wavy", amp=8.0, seed=100 + n)[:n])


def piled_cloud():
    """tests/test_gpu_parity.py::test_plan_reuse_for_a_stream_of_clouds_of_one_size: 150 points of small_40k moved from between the
    windows into the x range of one window, which then overflows the capacities inherited from the plan of the unmoved cloud"""
    pts0, _ = synth.make_config("small_40k")
    probe = engine.Engine(0, tool_radius=6.0); probe.set_cloud(pts0)
    px = probe.slice_positions(); probe.close()
    piled = pts0.copy()
    x = piled[:, 0] * 1000.0
    far = np.nonzero((x > px[len(px) * 3 // 4]) & (x < x.max() - 20.0) & (np.abs(x[:, None] - px[None, :]).min(axis=1) > 4.6))[0][:150]
    rng = np.random.default_rng(5)
    donors = np.nonzero(np.abs(x - px[len(px) // 3]) < 3.5)[0]
    src = piled[rng.choice(donors, len(far))]
    piled[far, 0] = src[:, 0] + rng.uniform(-2e-4, 2e-4, len(far)).astype(np.float32)
    piled[far, 1] = rng.uniform(piled[:, 1].min(), piled[:, 1].max(), len(far)).astype(np.float32)
    piled[far, 2] = ((20.0 * np.sin(piled[far, 0].astype(np.float64) * 1000.0 / 600.0) * np.cos(piled[far, 1].astype(np.float64) * 1000.0 / 300.0) + 1500.0) / 1000.0).astype(np.float32)
    return pts0, piled


def plan(out, key, pts, batch=False, **kw):
    """list, counts, bounds, path taken and form of one fresh handle; batch: the same pass again as a batch of one
    (ppp_run_batch_async: the k_win_scatter_b kernels, whose form PPP_WIN_DEBUG's "window batch" line names)"""
    try:
        e = engine.Engine(0, **kw)
        e.set_cloud(pts)
        form = e.binning_form()
        S = e.gen_path(); W = e.get_path()
        out[key + ".SW"] = np.array([S, W])
        if kw.get("slice_begin") is None:
            out[key + ".wp"] = e.waypoints()
        else:   # a slice-range handle has no finished list of its own: its block of sampled waypoints and their nearest points
            out[key + ".wp"] = e.stage(engine.STAGE_WP_XYZ)
            out[key + ".nn"] = e.stage(engine.STAGE_WP_NN)
        out[key + ".counts"] = e.waypoint_counts()
        mn, mx = e.minmax()
        out[key + ".bounds"] = np.concatenate([mn, mx])
        out[key + ".form"] = np.array(list(form) + [1 if e.fast_path() else 0])
        if batch:
            for _ in range(2):          # capture, then a replay of the batch graph
                engine.run_batch_async([e]); engine.sync_batch([e])
            out[key + ".wp_batch"] = e.waypoints()
            out[key + ".counts_batch"] = e.waypoint_counts()
        e.close()
    except engine.PPPError as ex:
        out[key + ".error"] = np.array([ex.code])


def main():
    engine.LIB_PATH = os.path.join(os.path.dirname(engine.LIB_PATH), "libppp_hip_tune.so")
    out = {}
    for case in sys.argv[2].split(","):
        if case == "shapes":
            for name in ("tiny_5k", "cfg1_50k_s32"):
                pts, cfg = synth.make_config(name)
                plan(out, name, pts, batch=True, tool_radius=cfg["tool_radius"])
        elif case.startswith("edge"):
            for n in [int(v) for v in case[4:].split("+")]:
                plan(out, "edge%d" % n, edge_cloud(n), tool_radius=6.0)
        elif case == "nan":
            pts, cfg = synth.make_config("tiny_5k")
            pts = pts.copy(); pts[::97, 0] = np.nan; pts[5] = np.nan
            plan(out, "nan", pts, tool_radius=6.0)
        elif case == "range":
            pts, cfg = synth.make_config("small_40k")
            plan(out, "range", pts, tool_radius=6.0, slice_begin=5, slice_end=17)
        elif case == "piled":
            pts0, piled = piled_cloud()
            h = engine.Engine(0, tool_radius=6.0)
            h.set_cloud(pts0); h.gen_path(); h.get_path()
            out["piled.form0"] = np.array(list(h.binning_form()) + [1 if h.fast_path() else 0])
            h.set_cloud(piled)             # inherits the capacities of the unmoved cloud's plan: the piled window overflows them
            S = h.gen_path(); W = h.get_path()
            out["piled.SW"] = np.array([S, W]); out["piled.wp"] = h.waypoints(); out["piled.counts"] = h.waypoint_counts()
            out["piled.form"] = np.array(list(h.binning_form()) + [1 if h.fast_path() else 0])
            h.close()
        else:
            raise SystemExit("unknown case " + case)
    np.savez(sys.argv[1], **out)


if __name__ == "__main__":
    main()
