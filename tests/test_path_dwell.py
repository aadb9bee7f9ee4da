"""The dwell schedule (ppp_get_path_dwell): a factor per row of the sample table that steers the
predicted removal towards a target map.

The restatement below builds the held pairs (point, row, d2, r2) and the rows' ds from ONE oracle of the same walk and
parameters, through its public methods only, the way test_path_removal.restate_path_removal builds its maps, and then iterates
the definitions in numpy: the forward pass ball by ball in ascending (slice, sample) order, np.rint for llrint, int64 sums.
Integer sums have no order, so rows, map and the factors' statistics are expected bit for bit; the level L and the residuals
come from device reductions whose order numpy cannot restate and are checked within touched * 2^-52 (relative)."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

from polishpathplanning_amd import synth
from test_path_coverage import CASES, boundary_samples, case_params
from test_path_removal import past_the_grid_cap, sample_lengths

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAT, PARABOLIC, HERTZ = 0, 1, 2
EPS = 2.0 ** -52
FIXED = 2.0 ** 28
G_LO, G_HI = 2.0 ** -6, 2.0 ** 6

ROW_DECL = "typedef struct { int slice; float x, y, z, r; double ds, dwell; } ppp_dwell_row;"
STATS_DECL = ("typedef struct {\n"
              "    size_t n, touched, rows;        /* cloud->size(); points a ball holds; rows of the sample table */\n"
              "    size_t at_min, at_max;          /* rows whose factor ended on a bound */\n"
              "    int    iterations;\n"
              "    double level;                   /* L, see above */\n"
              "    double residual_before, residual_after;   /* sqrt(mean over touched of ((R_i - T_i) / L)^2), at t = 1 and at the result */\n"
              "    double min_dwell, max_dwell;    /* over rows with den > 0; NaN when there are none */\n"
              "    double path_length, time_factor;/* sum ds_j ; sum ds_j t_j / sum ds_j, both in (slice, sample) order */\n"
              "} ppp_dwell_stats;")
CALL_DECL = ("int ppp_get_path_dwell(ppp_handle h, int profile, const double *target, int iterations, double dwell_min, double dwell_max,\n"
             "                       ppp_dwell_row *rows, size_t row_cap, double *removal, size_t cap, ppp_dwell_stats *stats);")
ROW_FIELDS = ("slice", "x", "y", "z", "r", "ds", "dwell")
STATS_FIELDS = ("n", "touched", "rows", "at_min", "at_max", "iterations", "level", "residual_before", "residual_after", "min_dwell",
                "max_dwell", "path_length", "time_factor")


def ordered_sum(v):
    """v[0] + v[1] + ... one after the other (np.sum adds pairwise)"""
    return float(np.cumsum(np.asarray(v, np.float64))[-1]) if len(v) else 0.0


def restate_pairs(pts, kw, oracle_mod):
    """dict: n, S, cloud (float32[n, 3]), rows (structured: slice, x, y, z, r, ds; the sample table in (slice, sample) order),
    first (the first row of every slice that has rows, and the row count at the end), and the held pairs in ascending row
    order: pj (row), pi (cloud index), d2, r2 (float32)"""
    R = kw["tool_radius"]
    o = oracle_mod.Oracle(pts, **kw)
    S = o.gen_path()
    cloud = o.points()
    rows, first, pj, pi, pd2, pr2 = [], [], [], [], [], []
    for s in range(S):
        y, _, _ = o.nodes(s)
        dys = boundary_samples(y, R) if len(y) >= 3 else []
        if not dys:
            continue                                  # B.15: no sample, no row
        rc, P = o.eval_spline(s, dys)
        assert rc == 0
        Q = P.astype(np.float32)
        ds = sample_lengths(Q)
        first.append(len(rows))
        for j, p in enumerate(P):
            lo, hi = o.area2cloud(p, 0), o.area2cloud(p, 1)
            r = (np.float32(lo[0]) - np.float32(hi[0])) / np.float32(2)
            r2 = np.float32(r) * np.float32(r)
            row = len(rows)
            rows.append((s, Q[j, 0], Q[j, 1], Q[j, 2], np.sqrt(r2), ds[j]))      # r: the float root of r2 (NaN stays NaN)
            if np.isnan(r):
                continue                              # B.16: the row keeps its position and its ds, its ball holds nothing
            idx = np.asarray(o.radius_search(Q[j], float(r)), np.int64)
            if not len(idx):
                continue
            c = cloud[idx]
            dx, dy, dz = Q[j, 0] - c[:, 0], Q[j, 1] - c[:, 1], Q[j, 2] - c[:, 2]      # dist2_flann's order, in float32
            d2 = dx * dx
            d2 = d2 + dy * dy
            d2 = d2 + dz * dz
            assert d2.dtype == np.float32 and np.all(d2 <= r2)
            pj.append(np.full(len(idx), row, np.int64)); pi.append(idx); pd2.append(d2); pr2.append(np.full(len(idx), r2, np.float32))
    o.close()
    first.append(len(rows))
    dt = np.dtype([("slice", np.int32), ("x", np.float32), ("y", np.float32), ("z", np.float32), ("r", np.float32), ("ds", np.float64)])
    cat = lambda v, t: np.concatenate(v) if v else np.zeros(0, t)
    return dict(n=len(cloud), S=S, cloud=cloud, rows=np.array(rows, dt), first=np.array(first, np.int64), pj=cat(pj, np.int64),
                pi=cat(pi, np.int64), d2=cat(pd2, np.float32), r2=cat(pr2, np.float32))


@functools.lru_cache(maxsize=None)
def _pairs(ci):
    from oracle import ppo
    ppo.build()
    pts, kw = case_params(*CASES[ci])
    return restate_pairs(pts, kw, ppo)


def pairs_of(ci, oracle_mod):
    """the pairs of CASES[ci], computed once and shared; nobody writes to them"""
    return _pairs(ci)


def weights(w, profile):
    """a_ij of every held pair: prem_weight<profile>(d2, r2)"""
    if profile == FLAT:
        return np.ones(len(w["pj"]))
    with np.errstate(invalid="ignore", divide="ignore"):
        u = np.where(w["r2"] == 0, 0.0, w["d2"].astype(np.float64) / w["r2"].astype(np.float64))
    return 1.0 - u if profile == PARABOLIC else np.sqrt(1.0 - u)


class Solver:
    """the definitions of §7h on the pairs of one case and one profile"""

    def __init__(self, w, profile):
        self.w, self.a = w, weights(w, profile)
        self.n, self.nrow = w["n"], len(w["rows"])
        self.ds = w["rows"]["ds"]
        self.held = np.zeros(self.n, bool)
        self.held[w["pi"]] = True
        self.touched = int(self.held.sum())
        self.cut = np.searchsorted(w["pj"], np.arange(self.nrow + 1))       # the pairs of row j: [cut[j], cut[j + 1])
        self.den = np.zeros(self.nrow, np.int64)
        np.add.at(self.den, w["pj"], np.rint(self.a * FIXED).astype(np.int64))

    def forward(self, t):
        """R_i = sum_j a_ij (ds_j t_j): the rounded products, per ball in ascending row order"""
        dst = self.ds * t
        out = np.zeros(self.n)
        pi, cut, a = self.w["pi"], self.cut, self.a
        for j in range(self.nrow):
            k0, k1 = cut[j], cut[j + 1]
            if k1 > k0:
                out[pi[k0:k1]] += a[k0:k1] * dst[j]               # (a search returns a point once)
        return out

    def unit_level(self):
        """sum / touched of the unit-feed map by numpy: what the engine's level is compared with"""
        R = self.forward(np.ones(self.nrow))
        return float(np.sum(R[self.held])) / self.touched

    def residual(self, R, T, L):
        e = (R[self.held] - T[self.held]) / L
        return float(np.sqrt(np.sum(e * e) / self.touched))

    def solve(self, T, L, iterations, dmin, dmax, trace=None):
        """(t, R at the result, residual_before, residual_after); T: float64[n]; trace: a list that takes the residual after
        every round"""
        t = np.ones(self.nrow)
        pi, pj = self.w["pi"], self.w["pj"]
        R = self.forward(t)
        before = self.residual(R, T, L)
        for it in range(iterations):
            if it:
                R = self.forward(t)
            with np.errstate(divide="ignore", invalid="ignore"):
                g = np.where(R > 0, np.minimum(np.maximum(T / R, G_LO), G_HI), 1.0)
            num = np.zeros(self.nrow, np.int64)
            np.add.at(num, pj, np.rint((self.a * g[pi]) * FIXED).astype(np.int64))
            has = self.den > 0
            t[has] = np.minimum(np.maximum(t[has] * (num[has].astype(np.float64) / self.den[has].astype(np.float64)), dmin), dmax)
            if trace is not None:
                trace.append(self.residual(self.forward(t), T, L))
        R = self.forward(t)
        return t, R, before, self.residual(R, T, L)

    def factor_stats(self, t, dmin, dmax):
        has = self.den > 0
        first = self.w["first"]
        scaled = self.ds * t
        length = ordered_sum([ordered_sum(self.ds[a:b]) for a, b in zip(first[:-1], first[1:])])
        total = ordered_sum([ordered_sum(scaled[a:b]) for a, b in zip(first[:-1], first[1:])])
        return dict(at_min=int((t[has] == dmin).sum()), at_max=int((t[has] == dmax).sum()),
                    min_dwell=float(t[has].min()) if has.any() else float("nan"),
                    max_dwell=float(t[has].max()) if has.any() else float("nan"), path_length=length, time_factor=total / length)


def same(x, y):
    """equal, arrays and floats by their bytes (so NaN equals NaN), through tuples and dicts"""
    if isinstance(x, (tuple, list)):
        return len(x) == len(y) and all(same(p, q) for p, q in zip(x, y))
    if isinstance(x, dict):
        return x.keys() == y.keys() and all(same(x[k], y[k]) for k in x)
    if isinstance(x, np.ndarray):
        return x.dtype == y.dtype and x.tobytes() == y.tobytes()
    return np.array([x]).tobytes() == np.array([y]).tobytes()


# ---------------------------------------------------------------- CPU


def test_header_declares_and_engine_exports_path_dwell(engine_mod):
    hdr = open(os.path.join(ROOT, "include", "ppp_hip.h")).read()
    assert ROW_DECL in hdr and STATS_DECL in hdr and CALL_DECL in hdr
    assert hdr.index("int ppp_get_path_removal(") < hdr.index(ROW_DECL) < hdr.index("int ppp_get_contact_field(")
    assert "ppp_get_path_dwell" in engine_mod.EXPORTS
    assert hasattr(engine_mod.Engine, "path_dwell")
    for h in ("Path_Generate.h", "Path_Generate_Algorithm.h", "robot_path.h"):
        assert "void get_path_dwell()" in open(os.path.join(ROOT, "include", h)).read(), h
    planner = open(os.path.join(ROOT, "include", "ppp_planner.hpp")).read()
    assert "bool path_dwell(ppp_dwell_stats &st, " in planner and "void print_path_dwell()" in planner


def test_header_is_c99_clean_with_path_dwell(tmp_path):
    src = tmp_path / "c99.c"
    src.write_text('#include "ppp_hip.h"\nint main(void) {\n'
                   '    int (*f)(ppp_handle, int, const double *, int, double, double, ppp_dwell_row *, size_t, double *, size_t,\n'
                   '             ppp_dwell_stats *) = ppp_get_path_dwell;\n'
                   '    ppp_dwell_stats st;\n    ppp_dwell_row row;\n'
                   '    st.time_factor = 0.0; st.at_max = 0; st.iterations = 0; row.slice = 0; row.dwell = 1.0; row.r = 0.f;\n'
                   '    return f == 0 || st.at_max != 0 || row.slice != 0;\n}\n')
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                           str(src)])


def test_dwell_structs_layout_matches_the_header(engine_mod, tmp_path):
    """the ctypes mirrors of ppp_dwell_row and ppp_dwell_stats have the C structs' sizes and offsets"""
    src = tmp_path / "layout.c"
    args = (["sizeof(ppp_dwell_row)"] + ["offsetof(ppp_dwell_row, %s)" % f for f in ROW_FIELDS]
            + ["sizeof(ppp_dwell_stats)"] + ["offsetof(ppp_dwell_stats, %s)" % f for f in STATS_FIELDS])
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ppp_hip.h"\nint main(void) {\n'
                   '    printf("' + " ".join(["%zu"] * len(args)) + '\\n", ' + ", ".join(args) + ');\n    return 0;\n}\n')
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)])
    got = [int(v) for v in subprocess.check_output([exe]).split()]
    Rw, St = engine_mod.DwellRow, engine_mod.DwellStats
    assert got == ([ctypes.sizeof(Rw)] + [getattr(Rw, f).offset for f in ROW_FIELDS]
                   + [ctypes.sizeof(St)] + [getattr(St, f).offset for f in STATS_FIELDS])
    assert np.dtype(Rw).itemsize == ctypes.sizeof(Rw) and np.dtype(Rw).names == ROW_FIELDS


def test_examples_build_with_the_path_dwell_switch(engine_mod):
    for ex in ("connect.cpp", "robot.cpp"):
        src = open(os.path.join(ROOT, "examples", ex)).read()
        assert 'getenv("PPP_PATH_DWELL")' in src and "get_path_dwell()" in src, ex
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "examples"), "connect", "connect1", "robot", "main"])
    for exe in ("connect", "connect1", "robot", "main"):
        assert os.access(os.path.join(ROOT, "examples", exe), os.X_OK)


def test_restatement_lowers_the_residual(oracle_mod):
    """the restatement alone, small_40k walk 1, Hertz, uniform target, bounds [0.25, 4]: the residual strictly decreases over
    1, 2, 4 and 8 rounds, and the factors are not all equal"""
    ci = CASES.index(("small_40k", 1, 0, 1, {}))
    s = Solver(pairs_of(ci, oracle_mod), HERTZ)
    L = s.unit_level()
    trace = []
    t, R, before, after = s.solve(np.full(s.n, L), L, 8, 0.25, 4.0, trace)
    print("residual: before %r, after rounds 1..8 %r" % (before, trace))
    assert after == trace[7]
    assert before > trace[0] > trace[1] > trace[3] > trace[7] > 0
    assert len(np.unique(t)) > 1 and float(t.max()) > 1 > float(t.min())


BOUNDS = (0.85, 1.5)            # both are reached within 3 rounds on every case below (test_bounds_are_reached)


@pytest.mark.parametrize("ci", [1, 5, 7], ids=["%s-w%d" % CASES[ci][:2] for ci in (1, 5, 7)])
def test_bounds_are_reached(oracle_mod, ci):
    """bounds [0.85, 1.5], 3 rounds, Hertz, uniform target: rows end on either bound, so the parity below tests the clamp"""
    s = Solver(pairs_of(ci, oracle_mod), HERTZ)
    L = s.unit_level()
    t, _, _, _ = s.solve(np.full(s.n, L), L, 3, *BOUNDS)
    f = s.factor_stats(t, *BOUNDS)
    print("at_min %d at_max %d of %d rows" % (f["at_min"], f["at_max"], s.nrow))
    assert f["at_min"] > 0 and f["at_max"] > 0


# ---------------------------------------------------------------- GPU


def engine_for(engine_mod, ci, **more):
    pts, kw = case_params(*CASES[ci])
    e = engine_mod.Engine(0, **dict(kw, **more))
    e.set_cloud(pts)
    return e, pts


def sine_target(w, L):
    """L (1 + 0.5 sin(2 pi y / 40 mm)) on the cloud's y (planner units: millimetres)"""
    return L * (1.0 + 0.5 * np.sin(2.0 * np.pi * w["cloud"][:, 1].astype(np.float64) / 40.0))


def check_parity(e, w, profile, iterations, target_of=None):
    s = Solver(w, profile)
    unit, ust = e.path_removal(profile)
    if target_of is None:
        rows, removal, st = e.path_dwell(profile, None, iterations, *BOUNDS)
        want_L = s.unit_level()
        T = None
    else:
        T = target_of(w, ust["mean"])
        rows, removal, st = e.path_dwell(profile, T, iterations, *BOUNDS)
        want_L = float(np.sum(T[s.held])) / s.touched
    L = st["level"]
    print("level: got %r numpy %r bound %r" % (L, want_L, s.touched * EPS * want_L))
    assert abs(L - want_L) <= s.touched * EPS * want_L
    if T is None:
        assert L == ust["mean"]
        T = np.full(s.n, L)
    t, R, before, after = s.solve(T, L, iterations, *BOUNDS)
    assert (st["n"], st["touched"], st["rows"], st["iterations"]) == (s.n, s.touched, s.nrow, iterations)
    assert st["touched"] == ust["touched"] and rows.shape == (s.nrow,) and removal.shape == (s.n,)
    for f in ("slice", "x", "y", "z", "r", "ds"):
        assert same(np.ascontiguousarray(rows[f]), np.ascontiguousarray(w["rows"][f])), f
    bad = np.nonzero(rows["dwell"] != t)[0]
    print("differing factors %d of %d" % (len(bad), len(t)))
    assert same(np.ascontiguousarray(rows["dwell"]), t), len(bad)
    bad = np.nonzero(removal != R)[0]
    print("differing points %d of %d" % (len(bad), len(R)))
    assert same(removal, R), len(bad)
    f = s.factor_stats(t, *BOUNDS)
    assert same({k: st[k] for k in f}, f), (st, f)
    assert st["path_length"] == ust["path_length"]
    for got, want in ((st["residual_before"], before), (st["residual_after"], after)):
        print("residual: got %r numpy %r bound %r" % (got, want, s.n * EPS * want))
        assert abs(got - want) <= s.n * EPS * want
    return st


PARITY = [(ci, HERTZ, it) for ci in (1, 5, 7) for it in (1, 3)] + [(5, p, it) for p in (FLAT, PARABOLIC) for it in (1, 3)]


@pytest.mark.gpu
@pytest.mark.parametrize("ci,profile,iterations", PARITY,
                         ids=["%s-w%d-p%d-it%d" % (CASES[ci][0], CASES[ci][1], p, it) for ci, p, it in PARITY])
def test_path_dwell_matches_the_restatement(engine_mod, oracle_mod, ci, profile, iterations):
    """rows (every field), the predicted map and the factors' statistics bit for bit, the level and the residuals within the
    reduction bound; short_slices has slices without a sample"""
    w = pairs_of(ci, oracle_mod)
    e, _ = engine_for(engine_mod, ci)
    assert e.gen_path() == w["S"]
    st = check_parity(e, w, profile, iterations)
    if profile == HERTZ and iterations == 3:
        assert st["at_min"] > 0 and st["at_max"] > 0 and st["residual_after"] < st["residual_before"]
    if CASES[ci][0] == "short_slices":
        assert len(w["first"]) - 1 < w["S"]
    none = e.path_dwell(profile, None, iterations, *BOUNDS, maps=False)
    assert none[0] is None and none[1] is None and same(none[2], st)
    e.close()


@pytest.mark.gpu
def test_path_dwell_follows_a_target_map(engine_mod, oracle_mod):
    """a target that varies along the path, L (1 + 0.5 sin(2 pi y / 40 mm)), small_40k walk 1"""
    w = pairs_of(1, oracle_mod)
    e, _ = engine_for(engine_mod, 1)
    assert e.gen_path() == w["S"]
    st = check_parity(e, w, HERTZ, 3, sine_target)
    assert st["residual_after"] < st["residual_before"]
    e.close()


KERNELS = ("k_dwell_scale", "k_dwell_ratio", "k_dwell_back", "k_dwell_update", "k_dwell_resid", "k_dwell_stats", "k_prem_points")


@pytest.mark.gpu
def test_path_dwell_is_the_same_in_every_run_and_kept_without_a_target(engine_mod):
    """two fresh handles give the same bytes; a repeated call without a target launches nothing, other arguments and a call
    with a target launch again"""
    pts, cfg = synth.make_config("small_40k")
    kw = dict(tool_radius=cfg["tool_radius"], walk=1)
    a, b = engine_mod.Engine(0, **kw), engine_mod.Engine(0, **kw)
    for e in (a, b):
        e.set_cloud(pts)
        e.gen_path(); e.get_path()
    a.enable_timing(True)
    a.kernel_times()
    first = a.path_dwell(HERTZ, None, 3, *BOUNDS)
    _, launches = a.kernel_times(with_launches=True)
    assert launches.get("k_dwell_back") == 3 and launches.get("k_dwell_update") == 3 and launches.get("k_dwell_ratio") == 3, launches
    assert launches.get("k_dwell_scale") == 3 and launches.get("k_prem_points") == 4 and launches.get("k_dwell_resid") == 2, launches
    again = a.path_dwell(HERTZ, None, 3, *BOUNDS)
    _, launches = a.kernel_times(with_launches=True)
    assert not any(launches.get(k) for k in KERNELS), launches
    assert same(again, first) and same(b.path_dwell(HERTZ, None, 3, *BOUNDS), first)
    assert first[2]["touched"] > 0 and first[2]["max_dwell"] > first[2]["min_dwell"]
    other = a.path_dwell(HERTZ, None, 2, *BOUNDS)
    _, launches = a.kernel_times(with_launches=True)
    assert launches.get("k_dwell_back") == 2 and not same(other[0], first[0]), launches
    T = np.full(len(pts), first[2]["level"])
    for _ in range(2):
        got = a.path_dwell(HERTZ, T, 3, *BOUNDS, maps=False)
        _, launches = a.kernel_times(with_launches=True)
        assert launches.get("k_dwell_back") == 3, launches
    assert got[2]["at_min"] == first[2]["at_min"] and got[2]["min_dwell"] == first[2]["min_dwell"]
    a.close(); b.close()


@pytest.mark.gpu
def test_window_path_and_slab_path_give_the_same_dwell(engine_mod):
    pts, cfg = synth.make_config("small_40k")
    kw = dict(tool_radius=cfg["tool_radius"], walk=1)
    a = engine_mod.Engine(0, **kw)
    b = engine_mod.Engine(0, fast_path=False, **kw)
    for e in (a, b):
        e.set_cloud(pts)
        e.gen_path(); e.get_path()
    assert a.fast_path() and not b.fast_path()
    assert same(a.path_dwell(HERTZ, None, 3, *BOUNDS), b.path_dwell(HERTZ, None, 3, *BOUNDS))
    assert a.fast_path()
    a.close(); b.close()


@pytest.mark.gpu
def test_path_dwell_leaves_the_other_results_alone(engine_mod):
    """path_coverage(), path_contacts(), path_removal() of all three profiles and a regions() result taken before and after a
    dwell call are identical, and are those of a handle that never asked for one"""
    pts, cfg = synth.make_config("small_40k")
    kw = dict(tool_radius=cfg["tool_radius"], walk=1)

    def results(e):
        f, c = e.path_coverage()
        con = e.path_contacts()
        rem = [e.path_removal(p) for p in (FLAT, PARABOLIC, HERTZ)]
        reg = e.regions(engine_mod.REGIONS_OVERLAP)
        return f, c, con, rem, reg

    never = engine_mod.Engine(0, **kw)
    never.set_cloud(pts)
    never.gen_path()
    want = results(never)
    e = engine_mod.Engine(0, **kw)
    e.set_cloud(pts)
    e.gen_path()
    before = results(e)
    st = None
    for p in (HERTZ, FLAT, PARABOLIC):
        st = e.path_dwell(p, None, 2, *BOUNDS)[2]
        e.path_dwell(p, np.full(len(pts), st["level"] * 2), 1, *BOUNDS, maps=False)
    assert st["touched"] > 0 and st["rows"] > 0
    assert same(before, results(e)) and same(before, want)
    f = engine_mod.Engine(0, **kw)                       # the dwell first: the other calls build on what it left
    f.set_cloud(pts)
    f.gen_path()
    f.path_dwell(HERTZ, None, 2, *BOUNDS)
    assert same(want, results(f))
    never.close(); e.close(); f.close()


@pytest.mark.gpu
def test_path_dwell_refusals(engine_mod):
    from polishpathplanning_amd.robot_path import slice_ranges
    pts, cfg = synth.make_config("small_40k")
    R = cfg["tool_radius"]
    e = engine_mod.Engine(0, tool_radius=R, walk=1)
    e.set_cloud(pts)

    def refused(h, code, *a, **k):
        with pytest.raises(engine_mod.PPPError) as ex:
            h.path_dwell(*a, **k)
        assert ex.value.code == code, (a, k, ex.value)

    refused(e, engine_mod.ERR_ARG)                                   # before any pass
    S = e.gen_path()
    for it in (0, 65):
        refused(e, engine_mod.ERR_ARG, iterations=it)
    for lo, hi in ((0.0, 1.0), (1.5, 2.0), (float("nan"), 2.0), (0.5, float("nan")), (0.5, float("inf"))):
        refused(e, engine_mod.ERR_ARG, dwell_min=lo, dwell_max=hi)
    refused(e, engine_mod.ERR_ARG, 3)
    counts = e.path_contacts()[0]
    T = np.ones(len(pts))
    T[np.nonzero(counts > 0)[0][0]] = np.nan
    refused(e, engine_mod.ERR_ARG, HERTZ, T)
    T = np.ones(len(pts))
    if (counts == 0).any():
        T[np.nonzero(counts == 0)[0][0]] = np.nan                    # nobody reads the target of an untouched point
    rows, removal, st = e.path_dwell(HERTZ, T, 1, 1.0, 1.0)
    assert st["touched"] > 0 and np.all(rows["dwell"] == 1.0) and st["time_factor"] == 1.0
    assert removal.tobytes() == e.path_removal(HERTZ)[0].tobytes()
    e.close()
    b, en = slice_ranges(S, 4)[1]
    h = engine_mod.Engine(0, tool_radius=R, walk=1, slice_begin=b, slice_end=en)
    h.set_cloud(pts)
    h.gen_path()
    refused(h, engine_mod.ERR_UNSUPPORTED)
    h.close()
    scaled = (pts * np.float32(1000)).astype(np.float32)
    mn, mx = scaled.min(axis=0), scaled.max(axis=0)
    g = engine_mod.Engine(0, tool_radius=R, slice_begin=2, slice_end=9)
    lo, hi, _ = g.range_interval(mn[0], mx[0])
    keep = np.nonzero((scaled[:, 0] >= lo) & (scaled[:, 0] <= hi))[0]
    g.set_cloud_part(pts[keep], keep, mn, mx, len(pts), lo, hi)
    g.gen_path()
    refused(g, engine_mod.ERR_UNSUPPORTED)
    g.close()


@pytest.mark.gpu
def test_path_dwell_beyond_the_grid_cap(engine_mod):
    """cfg3_250k_s128, walk 1, 2 rounds: k_dwell_resid's parts are longer than a workgroup.  No restatement at this size: the
    same bytes from two fresh handles, the integer fields against path_removal() and path_contacts(), the level as
    check_parity has it, and the two residuals from the maps the engine returns -- Solver.residual's expression, within
    check_parity's bound"""
    pts, cfg = synth.make_config("cfg3_250k_s128")
    kw = dict(tool_radius=cfg["tool_radius"], walk=1)
    n = len(pts)
    past_the_grid_cap(n)
    out = []
    for _ in range(2):
        e = engine_mod.Engine(0, **kw)
        e.set_cloud(pts)
        assert e.gen_path() == cfg["slices"]
        out.append(e.path_dwell(HERTZ, None, 2, *BOUNDS))
        unit, ust = e.path_removal(HERTZ)
        held = e.path_contacts()[0] > 0
        e.close()
    rows, removal, st = out[0]
    assert same(out[1], out[0])
    touched = int(held.sum())
    assert (st["n"], st["touched"], st["rows"], st["iterations"]) == (n, touched, len(rows), 2) and touched == ust["touched"] and len(rows) > 0
    assert st["at_min"] + st["at_max"] <= len(rows) and removal.shape == (n,)
    L = st["level"]
    assert L == ust["mean"] and st["path_length"] == ust["path_length"]

    def residual(R):
        e = (R[held] - L) / L
        return float(np.sqrt(np.sum(e * e) / touched))

    for got, want in ((st["residual_before"], residual(unit)), (st["residual_after"], residual(removal))):
        print("residual: got %r numpy %r bound %r" % (got, want, n * EPS * want))
        assert abs(got - want) <= n * EPS * want
    assert st["residual_after"] < st["residual_before"]
