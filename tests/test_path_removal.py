"""Predicted material removal (ppp_get_path_removal): the balls of the path contacts, each
weighted by the path length its sample stands for and by the point's place inside the ball.

The restatement below rebuilds the three maps (flat, parabolic, Hertzian) from ONE oracle of the same walk and parameters,
through its public methods only (points, nodes, eval_spline, area2cloud, radius_search), ball by ball in ascending (slice,
sample) order -- every point's own ascending order, so the maps are expected bit for bit."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from polishpathplanning_amd import synth
from test_path_coverage import CASES, boundary_samples, case_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BINS = 64
FLAT, PARABOLIC, HERTZ = 0, 1, 2
EPS = 2.0 ** -52


def sample_lengths(q):
    """ds of one slice's samples q (float32[m, 3]): double differences of the float positions, ((dx*dx) + dy*dy) + dz*dz, a
    segment with a non-finite end 0, half a segment on either side of a sample"""
    m = len(q)
    if m < 2:
        return np.zeros(m)
    q = q.astype(np.float64)
    d = q[1:] - q[:-1]
    with np.errstate(invalid="ignore"):
        seg = np.sqrt(((d[:, 0] * d[:, 0]) + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    ok = np.isfinite(q).all(axis=1)
    seg[~(ok[1:] & ok[:-1])] = 0.0
    ds = np.empty(m)
    ds[0], ds[-1] = 0.5 * seg[0], 0.5 * seg[-1]
    ds[1:-1] = 0.5 * (seg[:-1] + seg[1:])
    return ds


def ordered_sum(v):
    """v[0] + v[1] + ... one after the other (np.sum adds pairwise)"""
    return float(np.cumsum(np.asarray(v, np.float64))[-1]) if len(v) else 0.0


def restate_path_removal(pts, kw, oracle_mod):
    """dict: maps (profile -> float64[n]), counts (the contact counts), lens (the ds of every slice, in slice order: an empty
    array where a slice has no sample), path_length, multi (counts > 0 on a slice of more than one sample), S"""
    R = kw["tool_radius"]
    o = oracle_mod.Oracle(pts, **kw)
    S = o.gen_path()
    cloud = o.points()
    n = len(cloud)
    maps = {p: np.zeros(n) for p in (FLAT, PARABOLIC, HERTZ)}
    counts = np.zeros(n, np.int64)
    multi = np.zeros(n, bool)
    lens = []
    for s in range(S):
        y, _, _ = o.nodes(s)
        dys = boundary_samples(y, R) if len(y) >= 3 else []
        if not dys:
            lens.append(np.zeros(0))                  # B.15: no sample, no ball, no length
            continue
        rc, P = o.eval_spline(s, dys)
        assert rc == 0
        Q = P.astype(np.float32)
        ds = sample_lengths(Q)
        lens.append(ds)
        for j, p in enumerate(P):
            lo, hi = o.area2cloud(p, 0), o.area2cloud(p, 1)
            r = (np.float32(lo[0]) - np.float32(hi[0])) / np.float32(2)
            if np.isnan(r):
                continue                              # B.16: the sample keeps its position and its ds, its ball holds nothing
            idx = np.asarray(o.radius_search(Q[j], float(r)), np.int64)
            if not len(idx):
                continue
            r2 = np.float32(r) * np.float32(r)
            c = cloud[idx]
            dx, dy, dz = Q[j, 0] - c[:, 0], Q[j, 1] - c[:, 1], Q[j, 2] - c[:, 2]      # dist2_flann's order, in float32
            d2 = dx * dx
            d2 = d2 + dy * dy
            d2 = d2 + dz * dz
            assert d2.dtype == np.float32 and np.all(d2 <= r2)
            u = d2.astype(np.float64) / np.float64(r2) if r2 != 0 else np.zeros(len(idx))
            counts[idx] += 1                          # (a search returns a point once)
            multi[idx] |= len(dys) > 1
            maps[FLAT][idx] += 1.0 * ds[j]
            maps[PARABOLIC][idx] += (1.0 - u) * ds[j]
            maps[HERTZ][idx] += np.sqrt(1.0 - u) * ds[j]
    o.close()
    path_length = ordered_sum([ordered_sum(d) for d in lens])
    return dict(maps=maps, counts=counts, lens=lens, path_length=path_length, multi=multi, S=S)


@functools.lru_cache(maxsize=None)
def _restated(ci):
    from oracle import ppo
    ppo.build()
    pts, kw = case_params(*CASES[ci])
    return restate_path_removal(pts, kw, ppo)


def restated(ci, oracle_mod):
    """the restatement of CASES[ci], computed once and shared; nobody writes to it"""
    return _restated(ci)


def same(x, y):
    """equal, arrays and floats by their bytes (so NaN equals NaN), through tuples and dicts"""
    if isinstance(x, (tuple, list)):
        return len(x) == len(y) and all(same(p, q) for p, q in zip(x, y))
    if isinstance(x, dict):
        return x.keys() == y.keys() and all(same(x[k], y[k]) for k in x)
    if isinstance(x, np.ndarray):
        return x.dtype == y.dtype and x.tobytes() == y.tobytes()
    return np.array([x]).tobytes() == np.array([y]).tobytes()


@functools.lru_cache(maxsize=None)
def compute_units():
    """multi_processor_count of device 0 as torch reports it, asked once, in a process of its own: torch finds no device in a
    process in which the engine's HIP runtime is already at work"""
    out = subprocess.check_output([sys.executable, "-c", "import torch; print(torch.cuda.get_device_properties(0).multi_processor_count)"])
    return int(out.split()[-1])


def past_the_grid_cap(n_sorted):
    """the precondition of every test beyond the grid cap: on this device the capped grids (two workgroups of 256 threads per
    CU) no longer hold n_sorted threads, so a second trip is taken; returns that cap"""
    cap = 2 * compute_units() * 256
    print("n_sorted %d, grid cap %d threads (%d workgroups)" % (n_sorted, cap, cap // 256))
    assert n_sorted > cap, "this device needs more than %d points to reach a second trip" % n_sorted
    return cap


def check_stats(removal, touched, st, path_length=None):
    """the statistics are those of the map, of the touched points and of the sample table's lengths (path_length None: the
    caller has no restated length)"""
    t = removal[touched]
    assert st["n"] == len(removal) and st["touched"] == int(touched.sum())
    if path_length is not None:
        assert st["path_length"] == path_length, (st["path_length"], path_length)
    assert st["hist"].shape == (BINS,) and int(st["hist"].sum()) == len(t)
    if not len(t):
        assert np.isnan(st["min_removal"]) and np.isnan(st["max_removal"]) and st["sum"] == 0 and st["sum_sq"] == 0
        assert np.isnan(st["mean"]) and np.isnan(st["cv"])
        return
    mx = float(t.max())
    assert st["min_removal"] == float(t.min()) and st["max_removal"] == mx
    bins = np.minimum(BINS - 1, np.floor(t / mx * (BINS - 1))).astype(np.int64) if mx > 0 else np.zeros(len(t), np.int64)
    assert np.array_equal(st["hist"], np.bincount(bins, minlength=BINS))
    for got, want in ((st["sum"], float(np.sum(t))), (st["sum_sq"], float(np.sum(t * t)))):
        print("sum: got %r numpy %r bound %r" % (got, want, len(t) * EPS * want))
        assert abs(got - want) <= len(t) * EPS * want
    mean = st["sum"] / len(t)
    assert st["mean"] == mean
    if mean > 0:
        assert st["cv"] == float(np.sqrt(max(0.0, st["sum_sq"] / len(t) - mean * mean))) / mean


def test_header_declares_and_engine_exports_path_removal(engine_mod):
    hdr = open(os.path.join(ROOT, "include", "ppp_hip.h")).read()
    assert "enum { PPP_REMOVAL_FLAT = 0, PPP_REMOVAL_PARABOLIC = 1, PPP_REMOVAL_HERTZ = 2 };" in hdr
    assert ("typedef struct {\n    size_t n, touched;\n    double min_removal, max_removal, sum, sum_sq, path_length;\n"
            "    size_t hist[PPP_CONTACT_BINS];\n} ppp_removal_stats;") in hdr
    assert "int ppp_get_path_removal(ppp_handle h, int profile, double *removal, size_t cap, ppp_removal_stats *stats);" in hdr
    assert "ppp_get_path_removal" in engine_mod.EXPORTS
    assert hasattr(engine_mod.Engine, "path_removal")
    assert (engine_mod.REMOVAL_FLAT, engine_mod.REMOVAL_PARABOLIC, engine_mod.REMOVAL_HERTZ) == (FLAT, PARABOLIC, HERTZ)
    for h in ("Path_Generate.h", "Path_Generate_Algorithm.h", "robot_path.h"):
        assert "void get_path_removal()" in open(os.path.join(ROOT, "include", h)).read(), h
    planner = open(os.path.join(ROOT, "include", "ppp_planner.hpp")).read()
    assert ("bool path_removal(ppp_removal_stats &st, int profile = PPP_REMOVAL_HERTZ, std::vector<double> *removal = nullptr)"
            in planner)
    assert "void print_path_removal()" in planner


def test_header_is_c99_clean_with_path_removal(tmp_path):
    src = tmp_path / "c99.c"
    src.write_text('#include "ppp_hip.h"\nint main(void) {\n'
                   '    int (*f)(ppp_handle, int, double *, size_t, ppp_removal_stats *) = ppp_get_path_removal;\n'
                   '    ppp_removal_stats st;\n    st.hist[PPP_CONTACT_BINS - 1] = 0; st.path_length = 0.0; st.touched = 0;\n'
                   '    return f == 0 || st.hist[63] != 0 || PPP_REMOVAL_HERTZ != 2;\n}\n')
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                           str(src)])


def test_removal_stats_layout_matches_the_header(engine_mod, tmp_path):
    """the ctypes mirror of ppp_removal_stats has the C struct's size and offsets"""
    src = tmp_path / "layout.c"
    fields = ("touched", "min_removal", "max_removal", "sum", "sum_sq", "path_length", "hist")
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ppp_hip.h"\nint main(void) {\n'
                   '    printf("%zu' + " %zu" * len(fields) + '\\n", sizeof(ppp_removal_stats)'
                   + "".join(", offsetof(ppp_removal_stats, %s)" % f for f in fields) + ');\n    return 0;\n}\n')
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)])
    got = [int(v) for v in subprocess.check_output([exe]).split()]
    S = engine_mod.RemovalStats
    assert got == [ctypes.sizeof(S)] + [getattr(S, f).offset for f in fields]


def test_examples_build_with_the_path_removal_switch(engine_mod):
    for ex in ("connect.cpp", "robot.cpp"):
        src = open(os.path.join(ROOT, "examples", ex)).read()
        assert 'getenv("PPP_PATH_REMOVAL")' in src and "get_path_removal()" in src, ex
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "examples"), "connect", "connect1", "robot", "main"])
    for exe in ("connect", "connect1", "robot", "main"):
        assert os.access(os.path.join(ROOT, "examples", exe), os.X_OK)


def test_restatement_weighs_the_contacts(oracle_mod):
    """the restatement on CPU, small_40k walk 1: three different maps ordered as the weights are, a removal wherever there
    is a contact, and a flat map that is NOT a multiple of the contact count -- the samples' lengths differ, which is what a
    count cannot say"""
    ci = CASES.index(("small_40k", 1, 0, 1, {}))
    w = restated(ci, oracle_mod)
    flat, par, hz, counts = w["maps"][FLAT], w["maps"][PARABOLIC], w["maps"][HERTZ], w["counts"]
    assert w["S"] > 2 and int(counts.max()) >= 2
    assert not np.array_equal(flat, par) and not np.array_equal(par, hz) and not np.array_equal(flat, hz)
    assert np.all(0 <= par) and np.all(par <= hz) and np.all(hz <= flat)
    assert np.all(flat[w["multi"]] > 0) and np.all(flat[counts == 0] == 0)
    ratio = flat[counts > 0] / counts[counts > 0]
    assert len(np.unique(ratio)) > 1 and float(ratio.max()) > 1.01 * float(ratio.min())
    assert w["path_length"] > 0


PARITY = [(ci, HERTZ) for ci in range(len(CASES))] + [(ci, p) for ci in (1, 5, 7) for p in (FLAT, PARABOLIC)]


@pytest.mark.gpu
@pytest.mark.parametrize("ci,profile", PARITY, ids=["%s-w%d-p%d" % (CASES[ci][0], CASES[ci][1], p) for ci, p in PARITY])
def test_path_removal_matches_the_restatement(engine_mod, oracle_mod, ci, profile):
    """Engine.path_removal(): every sum the restatement's bits, for every walk; touched is path_contacts()'s covered; the
    statistics are the map's and the table's"""
    pts, kw = case_params(*CASES[ci])
    w = restated(ci, oracle_mod)
    want = w["maps"][profile]
    e = engine_mod.Engine(0, **kw)
    e.set_cloud(pts)
    assert e.gen_path() == w["S"]
    removal, st = e.path_removal(profile)
    counts, _, _, cst = e.path_contacts()
    assert removal.dtype == np.float64 and removal.shape == (len(pts),)
    assert np.array_equal(counts, w["counts"])
    bad = np.nonzero(removal != want)[0]
    print("differing points %d of %d; largest relative difference %r" % (
        len(bad), len(want), float(np.max(np.abs(removal[bad] - want[bad]) / want[bad])) if len(bad) else 0.0))
    assert np.array_equal(removal, want), len(bad)
    assert st["touched"] == cst["covered"]
    assert not np.any((removal > 0) & (counts == 0))
    check_stats(removal, counts > 0, st, w["path_length"])
    none, st2 = e.path_removal(profile, maps=False)
    assert none is None and same(st2, st)
    e.close()


KERNELS = ("k_prem_ds", "k_prem_points", "k_prem_range", "k_prem_stats")
TABLE = ("k_pcon_offsets", "k_pcon_samples")


@pytest.mark.gpu
def test_path_removal_is_the_same_in_every_run_and_kept_per_pass_and_profile(engine_mod):
    """two fresh handles give the same bytes of map and statistics; a repeated call launches nothing, a second profile
    launches neither the sample table nor the lengths again, and path_contacts() behind it shares the table"""
    pts, cfg = synth.make_config("small_40k")
    kw = dict(tool_radius=cfg["tool_radius"], walk=1)
    a, b = engine_mod.Engine(0, **kw), engine_mod.Engine(0, **kw)
    for e in (a, b):
        e.set_cloud(pts)
        e.gen_path(); e.get_path()
    a.enable_timing(True)
    a.kernel_times()
    first = {}
    for i, p in enumerate((HERTZ, FLAT, PARABOLIC)):
        first[p] = a.path_removal(p)
        _, launches = a.kernel_times(with_launches=True)
        assert all(launches.get(k) == 1 for k in KERNELS[1:]), launches
        assert all((launches.get(k) or 0) == (1 if i == 0 else 0) for k in TABLE + KERNELS[:1]), launches
    for p in (FLAT, PARABOLIC, HERTZ):
        again = a.path_removal(p)
        _, launches = a.kernel_times(with_launches=True)
        assert not any(launches.get(k) for k in KERNELS + TABLE), launches
        other = b.path_removal(p)
        assert same(again, first[p]) and same(other, first[p])
    assert first[HERTZ][1]["touched"] > 0 and first[HERTZ][1]["cv"] > 0
    ca = a.path_contacts()
    _, launches = a.kernel_times(with_launches=True)
    assert not any(launches.get(k) for k in TABLE) and launches.get("k_pcon_points") == 1, launches
    cb = engine_mod.Engine(0, **kw)
    cb.set_cloud(pts)
    cb.gen_path()
    want = cb.path_contacts()
    assert all(np.array_equal(x, y) for x, y in zip(ca[:3], want[:3])) and ca[3]["total"] == want[3]["total"]
    a.close(); b.close(); cb.close()


@pytest.mark.gpu
def test_window_path_and_slab_path_give_the_same_removal(engine_mod):
    pts, cfg = synth.make_config("small_40k")
    kw = dict(tool_radius=cfg["tool_radius"], walk=1)
    a = engine_mod.Engine(0, **kw)
    b = engine_mod.Engine(0, fast_path=False, **kw)
    for e in (a, b):
        e.set_cloud(pts)
        e.gen_path(); e.get_path()
    assert a.fast_path() and not b.fast_path()
    ra, sa = a.path_removal()
    rb, sb = b.path_removal()
    assert ra.tobytes() == rb.tobytes()
    assert sa["sum"] == sb["sum"] and sa["path_length"] == sb["path_length"] and np.array_equal(sa["hist"], sb["hist"])
    assert sa["touched"] > 0 and sa["max_removal"] > sa["min_removal"]
    assert a.fast_path()
    a.close(); b.close()


@pytest.mark.gpu
def test_ranged_handles_tile_the_whole_cloud_removal(engine_mod):
    """4 slice ranges: the maps and the path lengths add up to the whole cloud's to within the rounding of another
    association; a range_margin too small for the balls is refused, a part handle has no whole-cloud map"""
    from polishpathplanning_amd.robot_path import slice_ranges
    pts, cfg = synth.make_config("small_40k")
    R = cfg["tool_radius"]
    kw = dict(tool_radius=R, walk=1)
    whole = engine_mod.Engine(0, **kw)
    whole.set_cloud(pts)
    S = whole.gen_path()
    want, ws = whole.path_removal()
    counts = whole.path_contacts()[0]
    n = len(pts)
    got, length, touched = np.zeros(n), 0.0, np.zeros(n, bool)
    ranges = slice_ranges(S, 4)
    assert len(ranges) == 4
    for b, e in ranges:
        h = engine_mod.Engine(0, slice_begin=b, slice_end=e, **kw)
        h.set_cloud(pts)
        h.gen_path()
        r, st = h.path_removal()
        c = h.path_contacts()[0]
        assert r.shape == (n,) and 0 < st["touched"] <= ws["touched"] and st["touched"] == int((c > 0).sum())
        got += r
        length += st["path_length"]
        touched |= c > 0
        h.close()
    assert np.array_equal(touched, counts > 0)
    err = np.abs(got - want)
    print("largest difference / bound: %r" % float(np.max(err[counts > 0] / (counts[counts > 0] * EPS * want[counts > 0] + 1e-300))))
    assert np.all(err <= counts * EPS * want)
    print("path length: parts %r whole %r" % (length, ws["path_length"]))
    assert abs(length - ws["path_length"]) <= S * EPS * ws["path_length"]
    b, e = ranges[1]
    h = engine_mod.Engine(0, slice_begin=b, slice_end=e, range_margin=5.0, **kw)
    h.set_cloud(pts)
    h.gen_path()
    with pytest.raises(engine_mod.PPPError) as ex:
        h.path_removal()
    assert ex.value.code == engine_mod.ERR_CAPACITY and "range_margin" in str(ex.value)
    h.close(); whole.close()
    scaled = (pts * np.float32(1000)).astype(np.float32)             # a part handle: its map would need the caller's index map
    mn, mx = scaled.min(axis=0), scaled.max(axis=0)
    g = engine_mod.Engine(0, tool_radius=R, slice_begin=2, slice_end=9)
    lo, hi, _ = g.range_interval(mn[0], mx[0])
    keep = np.nonzero((scaled[:, 0] >= lo) & (scaled[:, 0] <= hi))[0]
    g.set_cloud_part(pts[keep], keep, mn, mx, len(pts), lo, hi)
    g.gen_path()
    with pytest.raises(engine_mod.PPPError) as ex:
        g.path_removal()
    assert ex.value.code == engine_mod.ERR_UNSUPPORTED
    g.close()


@pytest.mark.gpu
def test_path_removal_leaves_the_other_results_alone(engine_mod):
    """path_coverage(), path_contacts() and a regions() result taken before and after the removal are identical, and are those
    of a handle that never asked for the removal"""
    pts, cfg = synth.make_config("small_40k")
    kw = dict(tool_radius=cfg["tool_radius"], walk=1)

    def results(e):
        f, c = e.path_coverage()
        con = e.path_contacts()
        reg = e.regions(engine_mod.REGIONS_OVERLAP)
        return f, c, con, reg

    e = engine_mod.Engine(0, **kw)
    e.set_cloud(pts)
    e.gen_path()
    before = results(e)
    for p in (HERTZ, FLAT, PARABOLIC):
        e.path_removal(p)
    assert same(before, results(e))
    f = engine_mod.Engine(0, **kw)                       # the removal first: the other calls build on its sample table
    f.set_cloud(pts)
    f.gen_path()
    f.path_removal()
    assert same(before, results(f))
    e.close(); f.close()


@pytest.mark.gpu
def test_path_removal_refusals(engine_mod):
    pts, cfg = synth.make_config("small_40k")
    e = engine_mod.Engine(0, tool_radius=cfg["tool_radius"])
    e.set_cloud(pts)
    with pytest.raises(engine_mod.PPPError) as ex:                   # before any pass
        e.path_removal()
    assert ex.value.code == engine_mod.ERR_ARG
    e.gen_path()
    for profile in (-1, 3):
        with pytest.raises(engine_mod.PPPError) as ex:
            e.path_removal(profile)
        assert ex.value.code == engine_mod.ERR_ARG and "profile" in str(ex.value)
    removal, st = e.path_removal(PARABOLIC)
    assert st["touched"] > 0 and removal.shape == (len(pts),)
    e.close()


@pytest.mark.gpu
def test_path_removal_beyond_the_grid_cap(engine_mod):
    """cfg3_250k_s128, walk 1: more points than two workgroups of 256 threads per CU, so k_prem_range takes a second trip of
    its capped grid and k_prem_stats's parts are longer than a workgroup.  The statistics against the downloaded map (the
    restated path length costs too much at this size), and the same bytes from two fresh handles"""
    pts, cfg = synth.make_config("cfg3_250k_s128")
    kw = dict(tool_radius=cfg["tool_radius"], walk=1)
    n = len(pts)
    cap = past_the_grid_cap(n)
    out = []
    for _ in range(2):
        e = engine_mod.Engine(0, **kw)
        e.set_cloud(pts)
        assert e.gen_path() == cfg["slices"]
        removal, st = e.path_removal(HERTZ)
        counts, _, _, cst = e.path_contacts()
        out.append((removal, st, counts))
        e.close()
    removal, st, counts = out[0]
    touched = counts > 0
    print("touched %d of %d: %d with a cloud index below %d, %d at or above" % (touched.sum(), n, touched[:cap].sum(), cap, touched[cap:].sum()))
    assert st["touched"] == cst["covered"] and touched[:cap].sum() > 1000 and touched[cap:].sum() > 1000
    assert not np.any((removal > 0) & ~touched) and st["path_length"] > 0
    check_stats(removal, touched, st)
    assert same(out[1], out[0])
