"""The contact model's values (wave_contact_tail, ppp_dynamic.h) on clouds that are not a gently waved sheet.

Every other cloud of the suite is a synth.make_plate sheet whose second principal curvature is about 1e-7: both ellipse axes
are clamped to Tool_Radius, the covariance of the projected normals has rank one, and most of the decision code of the tail
(the cubic's trigonometric path, the sort of its roots, the choice among the three cross products, a free or NaN axis, a zero
covariance, the place of the extremum window) is reached by a handful of queries or by none.  The clouds built here are curved,
creased or exactly flat:

PLANE      z exactly constant: zero covariance, every curvature and width NaN
BOWL, CAP  the R = 60 mm sphere, concave / convex towards the viewpoint (the normals flip: n0 x cv changes hand)
CYL_X, CYL_Y, CYL_30   the R = 30 mm cylinder, axis along x, along y, turned 30 degrees about z (points further than 26 mm from
           the axis are left out: the sheet would be steeper than the normal radius can follow)
SADDLE     (x^2 - y^2) / 80
CREASE     z = 0.7 |y|
TIGHT      an exactly flat plate with a half cylinder of R = 4 mm and a half sphere of R = 5 mm on it, sampled along their arcs:
           radii of curvature under Tool_Radius 6, and rows without a value right beside rows with one

Each is a seeded, permuted, jittered 1.5 mm grid in metres, 1 500 mm from the viewpoint as make_plate's, of 1 700 .. 2 600 points
and never a multiple of 16 (the field kernel takes 16 queries per wave: the last wave is not full).

The CPU tests restate the tail in numpy float32, operation by operation in the kernel's written order, from Oracle.knn and
Oracle.estimate_normals alone; the restated pc0 / pc1 and principal direction equal Oracle.principal_curvature bit for bit, and
the census counts which branch every query takes.  The GPU tests compare the engine with the oracle: equal bits, NaNs in the
same places."""
import math
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from polishpathplanning_amd import synth
from test_contact_field import bits, check_stats, flann_dist2, restate_field
from test_coverage import V1 as V1_CONTACT, restate_coverage
from test_density_adversaries import TOL_M, TOL_RAD, same_floats
from test_path_coverage import restate_path_coverage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
FLT_EPSILON = F(1.1920929e-07)
FLT_MIN = F(1.17549435e-38)
FIELD_Q = 16        # ppp_contact.h: #define FIELD_Q 16, the queries of one wave of k_field_batch
NX, NY = 61, 39
XC = 0.5 + 0.5 * (NX - 1) * synth.SPACING_MM     # the plate's middle in x, mm
R_TOOL = 6.0
TIE_CAP = 0.01      # of a cloud's queries may be left out for equal distances among their k + 1 nearest
MIN_CLASS = 20      # queries a census class needs in at least one cloud

CLOUDS = ("plane", "bowl", "cap", "cyl_x", "cyl_y", "cyl_30", "saddle", "crease", "tight")
SEEDS = {name: 100 + i for i, name in enumerate(CLOUDS)}

# the parameter sets of the sweep: one parameter off its default at a time, and the two clamps' parameters together
PARAM_SETS = [
    ("default", {}),
    ("depth1e-7", dict(depth=1e-7)),
    ("depth5", dict(depth=5.0)),
    ("k10", dict(curvature_k=10)),
    ("k3", dict(curvature_k=3)),
    ("k64", dict(curvature_k=64)),
    ("thick0.5", dict(toolthickness=0.5)),
    ("R15", dict(tool_radius=15.0)),
    ("R15-thick0.5", dict(tool_radius=15.0, toolthickness=0.5)),
    ("k10-R15-thick0.5", dict(curvature_k=10, tool_radius=15.0, toolthickness=0.5)),   # (the one set that reaches the toolthickness clamp)
]
DEFAULTS = dict(tool_radius=R_TOOL, depth=0.01, toolthickness=10.0, curvature_k=50)


def params_of(extra):
    return dict(DEFAULTS, **extra)


# ---------------------------------------------------------------- the clouds


def _grid(rng, nx=NX, ny=NY):
    gx = (np.arange(nx, dtype=np.float64) * synth.SPACING_MM + 0.5)[:, None]
    gy = ((np.arange(ny, dtype=np.float64) - 0.5 * (ny - 1)) * synth.SPACING_MM)[None, :]
    x = gx + rng.uniform(-synth.JITTER_MM, synth.JITTER_MM, (nx, ny))
    y = gy + rng.uniform(-synth.JITTER_MM, synth.JITTER_MM, (nx, ny))
    return x.ravel(), y.ravel()


def _tight(rng):
    """the flat plate; a ridge (half cylinder R = 4 along x at y = -14) and a bump (half sphere R = 5 at (XC, 12)), both towards
    the viewpoint and sampled on a jittered 1.5 mm grid of their arc lengths"""
    x, y = _grid(rng)
    yr, rr, xb, yb, rb = -14.0, 4.0, XC, 12.0, 5.0
    keep = (np.abs(y - yr) >= rr) & (np.hypot(x - xb, y - yb) >= rb)
    x, y, z = x[keep], y[keep], np.zeros(int(keep.sum()))
    rows = int(np.floor(np.pi * rr / synth.SPACING_MM))          # arc positions across the ridge, -90 .. 90 degrees
    sx = (np.arange(NX) * synth.SPACING_MM + 0.5)[:, None] + rng.uniform(-synth.JITTER_MM, synth.JITTER_MM, (NX, rows))
    ss = ((np.arange(rows) - 0.5 * (rows - 1)) * synth.SPACING_MM)[None, :] + rng.uniform(-synth.JITTER_MM, synth.JITTER_MM, (NX, rows))
    t = ss.ravel() / rr
    rx, ry, rz = sx.ravel(), yr + rr * np.sin(t), -rr * np.cos(t)
    m = int(np.floor(np.pi * rb / synth.SPACING_MM))
    u = ((np.arange(m) - 0.5 * (m - 1)) * synth.SPACING_MM)[:, None] + rng.uniform(-synth.JITTER_MM, synth.JITTER_MM, (m, m))
    v = ((np.arange(m) - 0.5 * (m - 1)) * synth.SPACING_MM)[None, :] + rng.uniform(-synth.JITTER_MM, synth.JITTER_MM, (m, m))
    s, phi = np.hypot(u, v).ravel(), np.arctan2(v, u).ravel()
    on = s < 0.5 * np.pi * rb
    s, phi = s[on], phi[on]
    bx, by, bz = xb + rb * np.sin(s / rb) * np.cos(phi), yb + rb * np.sin(s / rb) * np.sin(phi), -rb * np.cos(s / rb)
    return np.concatenate([x, rx, bx]), np.concatenate([y, ry, by]), np.concatenate([z, rz, bz])


def make_cloud(name):
    """float32 [n, 3] in metres, permuted"""
    rng = np.random.default_rng(SEEDS[name])
    if name == "tight":
        x, y, z = _tight(rng)
    else:
        x, y = _grid(rng, NX, 65 if name == "cyl_y" else NY)   # (CYL_Y keeps 35 of its 61 columns: more rows instead)
        xc = x - XC
        if name == "plane":
            z = np.zeros_like(x)
        elif name in ("bowl", "cap"):
            z = (60.0 - np.sqrt(60.0 ** 2 - xc ** 2 - y ** 2)) * (1.0 if name == "cap" else -1.0)
        elif name in ("cyl_x", "cyl_y", "cyl_30"):
            d = {"cyl_x": y, "cyl_y": xc, "cyl_30": -xc * np.sin(np.pi / 6) + y * np.cos(np.pi / 6)}[name]
            keep = np.abs(d) <= 26.0
            x, y, d = x[keep], y[keep], d[keep]
            z = 30.0 - np.sqrt(30.0 ** 2 - d ** 2)
        elif name == "saddle":
            z = (xc ** 2 - y ** 2) / 80.0
        elif name == "crease":
            z = 0.7 * np.abs(y)
        else:
            raise ValueError(name)
    pts = np.stack([x, y, z + synth.Z0_MM], axis=1)
    pts = pts[rng.permutation(len(pts))]
    if len(pts) % FIELD_Q == 0:
        pts = pts[:-1]
    return np.ascontiguousarray((pts / 1000.0).astype(np.float32))


_cache = {}


def shared(name, make):
    """a cloud or an expectation computed once and shared by the tests that need it (they leave it unchanged)"""
    if name not in _cache:
        _cache[name] = make()
    return _cache[name]


def cloud(name):
    return shared(("cloud", name), lambda: make_cloud(name))


def config_cloud(name):
    return synth.make_config(name)[0]


def points_of(name):
    return cloud(name) if name in CLOUDS else shared(("cloud", name), lambda: config_cloud(name))


def oracle_for(oracle_mod, name, extra=()):
    """an oracle per (cloud, parameters): kept open and shared"""
    extra = dict(extra)
    return shared(("oracle", name, tuple(sorted(extra.items()))), lambda: oracle_mod.Oracle(points_of(name), **params_of(extra)))


def tie_mask(P, Q, k):
    """queries with two equal float32 flann_dist2 among their k + 1 nearest (nearest_have_equal_distances of
    test_density_adversaries, for all of Q at once)"""
    out = np.zeros(len(Q), bool)
    for j, q in enumerate(Q):
        d2 = flann_dist2(q, P)
        s = np.partition(d2, k + 1)[: k + 2]
        s.sort()
        out[j] = bool((s[1:k + 1] == s[:k]).any() or s[k + 1] == s[k])
    return out


def ties(oracle_mod, name, k):
    P = oracle_for(oracle_mod, name).points()
    return shared(("ties", name, k), lambda: tie_mask(P, P, k))


def off_surface_queries(oracle_mod, name):
    """200 seeded points of the cloud displaced 0.5 .. 5 mm along their normal, 100 either way (resident unit, mm)"""
    def make():
        o = oracle_for(oracle_mod, name)
        P, N = o.points(), o.estimate_normals()[:, :3]
        rng = np.random.default_rng(SEEDS[name] + 1000)
        have = np.nonzero(np.isfinite(N).all(axis=1))[0]
        idx = rng.choice(have, 200, replace=False)
        t = rng.uniform(0.5, 5.0, 200) * np.where(np.arange(200) < 100, 1.0, -1.0)
        return np.ascontiguousarray((P[idx].astype(np.float64) + t[:, None] * N[idx].astype(np.float64)).astype(np.float32))
    return shared(("off", name), make)


# ---------------------------------------------------------------- the tail in numpy float32, in the kernel's written order


def _seq_sum(a):
    """a[:, 0] + a[:, 1] + ... one addition at a time from +0, as the rank-order loops do"""
    acc = np.zeros(a.shape[0], F)
    for j in range(a.shape[1]):
        acc = acc + a[:, j]
    return acc


def _roots2(b, c):
    d = ((b * b).astype(np.float64) - 4.0 * c.astype(np.float64)).astype(F)
    d = np.where(d < F(0), F(0), d)
    sd = np.sqrt(d)
    return np.zeros_like(b), F(0.5) * (b - sd), F(0.5) * (b + sd)


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def restate_frames(o, Q, k):
    """computePointPrincipalCurvatures at the queries Q (resident unit) for curvature_k = k, every float32 operation as
    wave_contact_tail writes it.  Returns a dict of per-query arrays: n0, cv, pc0, pc1 and the branch taken at every decision"""
    N = o.estimate_normals()[:, :3].astype(F)
    nb = np.stack([o.knn(q, k) for q in Q])
    assert nb.shape == (len(Q), k)
    with np.errstate(all="ignore"):
        nn = N[nb]                                            # [Q, k, 3]: the normal of the neighbour of rank r
        n0 = nn[:, 0, :]
        proj = np.empty_like(nn)
        for i in range(3):
            m = [F(1.0 if i == j else 0.0) - n0[:, i] * n0[:, j] for j in range(3)]
            proj[:, :, i] = (m[0][:, None] * nn[:, :, 0] + m[1][:, None] * nn[:, :, 1]) + m[2][:, None] * nn[:, :, 2]
        cen = np.stack([_seq_sum(proj[:, :, i]) / F(k) for i in range(3)], axis=1)
        d = proj - cen[:, None, :]
        cxx, cxy, cxz = _seq_sum(d[:, :, 0] * d[:, :, 0]), _seq_sum(d[:, :, 0] * d[:, :, 1]), _seq_sum(d[:, :, 0] * d[:, :, 2])
        cyy, cyz, czz = _seq_sum(d[:, :, 1] * d[:, :, 1]), _seq_sum(d[:, :, 1] * d[:, :, 2]), _seq_sum(d[:, :, 2] * d[:, :, 2])
        cov6 = np.stack([cxx, cxy, cxz, cyy, cyz, czz], axis=1)
        scale = np.fmax.reduce(np.abs(cov6), axis=1, initial=F(0))           # fmaxf / std::max from 0: a NaN never wins
        zero_cov = (cov6 == 0).all(axis=1)
        scale = np.where(scale <= FLT_MIN, F(1), scale).astype(F)
        m00, m01, m02, m11, m12, m22 = [(cov6[:, i] / scale).astype(F) for i in range(6)]
        c0 = m00 * m11 * m22 + F(2) * m01 * m02 * m12 - m00 * m12 * m12 - m11 * m02 * m02 - m22 * m01 * m01
        c1 = m00 * m11 - m01 * m01 + m00 * m22 - m02 * m02 + m11 * m22 - m12 * m12
        c2 = m00 + m11 + m22
        nan_frame = ~np.isfinite(c0)
        small = np.abs(c0) < FLT_EPSILON
        q0, q1, q2 = _roots2(c2, c1)
        s_inv3, s_sqrt3 = F(1.0 / 3.0), np.sqrt(F(3.0))
        c2_3 = c2 * s_inv3
        a_3 = (c1 - c2 * c2_3) * s_inv3
        a_3 = np.where(a_3 > F(0), F(0), a_3)
        half_b = F(0.5) * (c0 + c2_3 * (F(2) * c2_3 * c2_3 - c1))
        qq = half_b * half_b + a_3 * a_3 * a_3
        qq = np.where(qq > F(0), F(0), qq)
        rho = np.sqrt(-a_3)
        sq = np.sqrt(-qq)
        # atan2 / cos / sin in double through libm, rounded to float: the correctly rounded float results
        theta = np.array([math.atan2(float(a), float(b)) for a, b in zip(sq, half_b)], np.float64).astype(F) * s_inv3
        cos_t = np.array([math.cos(float(t)) if math.isfinite(t) else math.nan for t in theta], np.float64).astype(F)
        sin_t = np.array([math.sin(float(t)) if math.isfinite(t) else math.nan for t in theta], np.float64).astype(F)
        r0 = c2_3 + F(2) * rho * cos_t
        r1 = c2_3 - rho * (cos_t + s_sqrt3 * sin_t)
        r2 = c2_3 - rho * (cos_t - s_sqrt3 * sin_t)
        sw = r0 >= r1
        r0, r1 = np.where(sw, r1, r0), np.where(sw, r0, r1)
        sw = r1 >= r2
        r1, r2 = np.where(sw, r2, r1), np.where(sw, r1, r2)
        sw2 = sw & (r0 >= r1)
        r0, r1 = np.where(sw2, r1, r0), np.where(sw2, r0, r1)
        discard = ~small & (r0 <= F(0))
        use2 = small | discard
        e0, e1, e2 = [np.where(use2, a, b).astype(F) * scale for a, b in ((q0, r0), (q1, r1), (q2, r2))]
        shift = e2 / scale
        rows = [[m00 - shift, m01, m02], [m01, m11 - shift, m12], [m02, m12, m22 - shift]]
        cp = [_cross(rows[0], rows[1]), _cross(rows[0], rows[2]), _cross(rows[1], rows[2])]
        ln = [np.sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]) for c in cp]
        bi = np.zeros(len(Q), np.int64)
        bi = np.where(ln[1] > ln[0], 1, bi)
        lb = np.where(bi == 1, ln[1], ln[0])
        bi = np.where(ln[2] > lb, 2, bi)
        lb = np.where(bi == 2, ln[2], lb)
        cv = np.stack([np.choose(bi, [cp[0][i], cp[1][i], cp[2][i]]) / lb for i in range(3)], axis=1).astype(F)
        inv = F(1.0) / F(k)
        pc0, pc1 = (e2 * inv).astype(F), (e1 * inv).astype(F)
        # the closest calls of the two decisions that compare computed floats with each other
        gaps = np.sort(np.stack(ln, axis=1), axis=1)
    exit_ = np.where(nan_frame, "nan", np.where(small, "c0 small", np.where(discard, "trig discarded", "trig kept")))
    return dict(n0=n0, cv=cv, pc0=pc0, pc1=pc1, exit=exit_, winner=bi, zero_cov=zero_cov, nan_frame=nan_frame, sp=np.asarray(Q, F),
                len_equal=(gaps[:, 2] == gaps[:, 1]) & ~nan_frame & ~zero_cov,
                roots_equal=~use2 & ~nan_frame & ((r0 == r1) | (r1 == r2)))


def restate_axes(fr, P):
    """the ellipse axes (double, as std::pow / std::sqrt give), their branch and clamp states, and where the windowed fold
    looks: per-query arrays for the parameter set P"""
    R, depth, thick = float(P["tool_radius"]), float(P["depth"]), float(P["toolthickness"])
    pc0, pc1 = fr["pc0"], fr["pc1"]
    with np.errstate(all="ignore"):
        both = (pc0 >= 0) & (pc1 >= 0)
        out = {}
        for name, pc in (("long", pc1), ("short", pc0)):
            inv = (F(1) / pc).astype(F)
            i, a = inv.astype(np.float64), np.abs(inv).astype(np.float64)
            arg_a, arg_b = i * i - (a - depth) * (a - depth), i * i - R * R
            ax_a, ax_b = np.sqrt(arg_a), a - np.sqrt(arg_b)
            state_a = np.where(np.isnan(ax_a), "NaN", np.where(ax_a > R, "clamped to Tool_Radius", "free"))
            state_b = np.where(np.isnan(ax_b), "NaN", np.where(ax_b > thick, "clamped to toolthickness", "free"))
            out[name] = np.where(both, np.minimum(ax_a, R), np.minimum(ax_b, thick))
            out[name] = np.where(np.isnan(np.where(both, ax_a, ax_b)), np.nan, out[name])
            out[name + " state"] = np.where(both, state_a, state_b)
            out[name + " sqrt of a negative"] = np.where(both, arg_a < 0, arg_b < 0)
        out["both"] = both
        out["negative pc"] = ~both & ~(np.isnan(pc0) | np.isnan(pc1))
        n0, cv = fr["n0"], fr["cv"]
        cr = np.stack(_cross([n0[:, i] for i in range(3)], [cv[:, i] for i in range(3)]), axis=1).astype(F)
        A, B = cr[:, 0] * out["long"].astype(F), cv[:, 0] * out["short"].astype(F)
        Rr = np.sqrt(A * A + B * B)
        Cm = np.abs(fr["sp"][:, 0]) + Rr
        ok = (Rr > 0) & (Rr < F(1e30)) & (Cm < F(1e30)) & ~np.isnan(cr[:, 1]) & ~np.isnan(cr[:, 2]) & ~np.isnan(cv[:, 1]) & ~np.isnan(cv[:, 2])
        ulp = (np.ascontiguousarray(Cm, F).view(np.uint32) & np.uint32(0x7f800000)).view(F) * FLT_EPSILON
        E = F(4) * ulp + F(8) * Rr * FLT_EPSILON
        dl = F(0.008726646)
        K2 = (F(2) * E / (Rr * dl * dl) + F(0.125)) / F(0.49)
        windowed = ok & (K2 < F(27.0 * 27.0))
        for key in (0, 1):
            th = np.arctan2(B, A).astype(F)
            if key != 1:
                th = th + F(3.14159265)
            th = np.where(th < 0, th + F(6.2831853), th)
            a_star = np.where(windowed, np.floor(th / dl + F(0.5)), 0).astype(np.int64) % 720
            out["wrap key %d" % key] = windowed & ((a_star <= 31) | (a_star >= 689))
        out["windowed"] = windowed
        out["fold evaluated"] = ~np.isnan(out["long"]) & ~np.isnan(out["short"]) & ~fr["nan_frame"]
        out["small R"] = windowed & (Rr < F(0.05) * F(R))
    return out


CLASSES = (
    ["exit: " + s for s in ("c0 small", "trig kept", "trig discarded")]
    + ["winner: cross product %d" % i for i in range(3)]
    + ["zero covariance", "branch: both pc >= 0", "branch: a pc < 0 or NaN", "branch: a finite pc < 0"]
    + ["%s axis: %s" % (a, s) for a in ("long", "short") for s in ("clamped to Tool_Radius", "clamped to toolthickness", "free", "NaN")]
    + ["sqrt of a negative", "fold: windowed", "fold: all 721", "window holds 0/360, key 0", "window holds 0/360, key 1",
       "window holds 0/360 for neither key", "windowed with R under Tool_Radius / 20"]
)
# Classes behind a finite negative curvature (DESIGN.md 7zb says why): pc1 < 0 needs a covariance whose second eigenvalue is
# rounding noise, which a handful of queries of CREASE and TIGHT have and no more; the census asserts that these classes stay
# UNDER 20 queries, so that a cloud or a change that reaches one of them in numbers does not pass unnoticed
SPARSE = ("branch: a finite pc < 0", "long axis: clamped to toolthickness", "short axis: clamped to toolthickness", "sqrt of a negative")


def census_of(fr, ax, counted):
    """class -> number of the counted queries in it"""
    c = {}
    valid = counted & ~fr["nan_frame"]
    for s in ("c0 small", "trig kept", "trig discarded"):
        c["exit: " + s] = int((valid & (fr["exit"] == s) & ~fr["zero_cov"]).sum())
    for i in range(3):
        c["winner: cross product %d" % i] = int((valid & ~fr["zero_cov"] & (fr["winner"] == i)).sum())
    c["zero covariance"] = int((counted & fr["zero_cov"]).sum())
    c["branch: both pc >= 0"] = int((counted & ax["both"]).sum())
    c["branch: a pc < 0 or NaN"] = int((counted & ~ax["both"]).sum())
    c["branch: a finite pc < 0"] = int((counted & ax["negative pc"]).sum())
    for a in ("long", "short"):
        for s in ("clamped to Tool_Radius", "clamped to toolthickness", "free", "NaN"):
            c["%s axis: %s" % (a, s)] = int((valid & (ax[a + " state"] == s)).sum())
    c["sqrt of a negative"] = int((valid & (ax["long sqrt of a negative"] | ax["short sqrt of a negative"])).sum())
    ev = counted & ax["fold evaluated"]
    c["fold: windowed"] = int((ev & ax["windowed"]).sum())
    c["fold: all 721"] = int((ev & ~ax["windowed"]).sum())
    c["window holds 0/360, key 0"] = int((ev & ax["wrap key 0"]).sum())
    c["window holds 0/360, key 1"] = int((ev & ax["wrap key 1"]).sum())
    c["window holds 0/360 for neither key"] = int((ev & ax["windowed"] & ~ax["wrap key 0"] & ~ax["wrap key 1"]).sum())
    c["windowed with R under Tool_Radius / 20"] = int((ev & ax["small R"]).sum())
    return c


def frames(oracle_mod, name, k):
    """the restated frames at every point of a cloud, with the oracle's own rows beside them"""
    def make():
        o = oracle_for(oracle_mod, name, dict(curvature_k=k))
        P = o.points()
        fr = restate_frames(o, P, k)
        fr["oracle"] = np.stack([o.principal_curvature(p) for p in P])
        return fr
    return shared(("frames", name, k), make)


def print_table(title, columns, rows):
    print("\n" + title)
    w = max(len(r) for r in rows)
    print(" " * w + "".join("%9s" % c[:8] for c in columns))
    for r in rows:
        print(r.ljust(w) + "".join("%9d" % v for v in rows[r]))


# ---------------------------------------------------------------- CPU: the clouds, the restatement, the census


def test_clouds_are_what_they_claim(oracle_mod):
    for name in CLOUDS:
        pts = cloud(name)
        o = oracle_for(oracle_mod, name)
        P = o.points()
        assert 1500 < len(P) < 3000 and len(P) % FIELD_Q != 0, (name, len(P))
        assert bits(P).tobytes() == bits(pts * F(1000)).tobytes()
        assert np.array_equal(pts, make_cloud(name))                          # seeded
        assert 1400.0 < P[:, 2].min() and P[:, 2].max() < 1600.0
        N = o.estimate_normals()
        print("%-7s %d points, z %.2f .. %.2f mm, %d without a normal" % (name, len(P), P[:, 2].min(), P[:, 2].max(), int(np.isnan(N[:, 0]).sum())))
    P = oracle_for(oracle_mod, "plane").points()
    assert (P[:, 2] == F(1500.0)).all()
    N = oracle_for(oracle_mod, "plane").estimate_normals()
    assert (np.abs(N[:, 2]) == 1).all() and (N[:, 0] == 0).all() and (N[:, 1] == 0).all()
    nb, nc = oracle_for(oracle_mod, "bowl").estimate_normals(), oracle_for(oracle_mod, "cap").estimate_normals()
    ok = np.isfinite(nb[:, 0]) & np.isfinite(nc[:, 0])
    assert (nb[ok, 2] < 0).all() and (nc[ok, 2] < 0).all()                    # both face the viewpoint ...
    Pb = oracle_for(oracle_mod, "bowl").points()
    out = (Pb[:, 0] - F(XC)) * nb[:, 0] + Pb[:, 1] * nb[:, 1]
    far = ok & (np.hypot(Pb[:, 0] - XC, Pb[:, 1]) > 10)
    assert (out[far] < 0).mean() > 0.99                                         # ... the bowl's lean inwards, the cap's outwards
    Pc = oracle_for(oracle_mod, "cap").points()
    inw = (Pc[:, 0] - F(XC)) * nc[:, 0] + Pc[:, 1] * nc[:, 1]
    assert (inw[ok & (np.hypot(Pc[:, 0] - XC, Pc[:, 1]) > 10)] > 0).mean() > 0.99
    # a pass runs on CYL_X and SADDLE, with and without the dynamic adjustment
    for name in ("cyl_x", "saddle"):
        for dyn in (0, 1):
            o = oracle_mod.Oracle(cloud(name), tool_radius=R_TOOL, walk=1, dynamic_adjustment=dyn)
            S = o.gen_path()
            assert S > 4 and o.get_path() > 0, (name, dyn, S)
            o.close()


def test_equal_distances_are_rare(oracle_mod):
    """at most 1 % of a cloud's points, and of its off-surface queries, have two equal float32 distances among their k + 1
    nearest (they are left out of every bit comparison); counted for k = 64, which holds every smaller k's neighbours"""
    total = 0
    for name in CLOUDS:
        t = {k: int(ties(oracle_mod, name, k).sum()) for k in (50, 64, 10, 3)}
        P = oracle_for(oracle_mod, name).points()
        tq = int(tie_mask(P, off_surface_queries(oracle_mod, name), 64).sum())
        print("%-7s equal distances among the k + 1 nearest: %s of %d points; %d of 200 off-surface queries (k = 64)" % (name, t, len(P), tq))
        assert max(t.values()) <= TIE_CAP * len(P) and tq <= 2
        total += t[64]
    print("left out in all (k = 64): %d" % total)


@pytest.mark.parametrize("k", [50, 10, 3, 64])
def test_restatement_equals_the_oracle_bit_for_bit(oracle_mod, k):
    """pc0, pc1 and the principal direction of the numpy restatement against Oracle.principal_curvature at every point of
    every cloud: the census below describes the computation it claims to"""
    for name in CLOUDS:
        fr = frames(oracle_mod, name, k)
        counted = ~ties(oracle_mod, name, k)
        want = fr["oracle"]
        got = np.concatenate([fr["cv"], fr["pc0"][:, None], fr["pc1"][:, None]], axis=1)
        assert np.array_equal(np.isnan(got), np.isnan(want)), name
        bad = np.nonzero(((bits(got) != bits(want)) & ~np.isnan(want)).any(axis=1) & counted)[0]
        print("%-7s k=%d: %d of %d counted rows differ; %d rows are NaN" % (name, k, len(bad), int(counted.sum()), int(np.isnan(want[:, 3]).sum())))
        assert len(bad) == 0, (name, bad[:5], got[bad[:5]], want[bad[:5]])


def test_census_every_reachable_class_is_populated(oracle_mod):
    """the table per cloud and parameter set, and for tiny_5k and small_40k: every class is populated by at least 20 queries in
    at least one cloud of this file, or is listed as sparse and stays under 20"""
    best = {c: 0 for c in CLASSES}
    for label, extra in PARAM_SETS:
        P = params_of(extra)
        k = P["curvature_k"]
        rows = {c: [] for c in CLASSES}
        rows["(left out: equal distances)"] = []
        rows["(points)"] = []
        for name in CLOUDS:
            fr = frames(oracle_mod, name, k)
            counted = ~ties(oracle_mod, name, k)
            c = census_of(fr, restate_axes(fr, P), counted)
            for cl in CLASSES:
                rows[cl].append(c[cl])
                best[cl] = max(best[cl], c[cl])
            rows["(left out: equal distances)"].append(int((~counted).sum()))
            rows["(points)"].append(len(counted))
        print_table("census, parameters %s %s" % (label, extra), CLOUDS, rows)
    for cl in CLASSES:
        if cl in SPARSE:
            assert best[cl] < MIN_CLASS, (cl, best[cl])
        else:
            assert best[cl] >= MIN_CLASS, (cl, best[cl])
    assert best["branch: a finite pc < 0"] >= 5 and best["short axis: clamped to toolthickness"] >= 1
    assert best["long axis: clamped to toolthickness"] == 0 and best["sqrt of a negative"] == 0


def test_census_of_the_synthetic_sheets(oracle_mod):
    """the same table for tiny_5k (every point) and small_40k (4 000 seeded points): what the rest of the suite reaches"""
    rows = {c: [] for c in CLASSES}
    rows["(queries)"] = []
    for name in ("tiny_5k", "small_40k"):
        o = oracle_for(oracle_mod, name)
        P = o.points()
        idx = np.arange(len(P)) if len(P) <= 5000 else np.sort(np.random.default_rng(40).choice(len(P), 4000, replace=False))
        fr = restate_frames(o, P[idx], 50)
        want = np.stack([o.principal_curvature(p) for p in P[idx]])
        counted = ~tie_mask(P, P[idx], 50)
        got = np.stack([fr["pc0"], fr["pc1"]], axis=1)
        assert np.array_equal(np.isnan(got), np.isnan(want[:, 3:]))
        assert not ((bits(got) != bits(want[:, 3:])) & ~np.isnan(want[:, 3:]))[counted].any(), name
        c = census_of(fr, restate_axes(fr, DEFAULTS), counted)
        for cl in CLASSES:
            rows[cl].append(c[cl])
        rows["(queries)"].append(int(counted.sum()))
    print_table("census of the synthetic sheets, default parameters", ("tiny_5k", "small_40k"), rows)
    for cl in ("exit: trig kept", "long axis: free", "short axis: free", "long axis: NaN", "zero covariance", "fold: all 721"):
        assert max(rows[cl]) < MIN_CLASS, (cl, rows[cl])                        # the gap this file closes


# ---------------------------------------------------------------- GPU


def oracle_field(oracle_mod, name, extra):
    def make():
        return restate_field(oracle_for(oracle_mod, name, extra))
    return shared(("field", name, tuple(sorted(extra.items()))), make)


def same_where(got, want, counted, what):
    """same_floats on the counted rows: equal bits, NaNs in the same places.  A row left out for equal distances is left out
    whole: where the tie is between the k-th and the (k + 1)-th neighbour the oracle's neighbour SET is traversal-defined, and
    with it whether a neighbour without a normal is in it"""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    assert got.shape == want.shape, what
    assert np.array_equal(np.isnan(got[counted]), np.isnan(want[counted])), (what, int((np.isnan(got) != np.isnan(want)).sum()))
    same_floats(got[counted], want[counted], what)


@pytest.mark.gpu
@pytest.mark.parametrize("name", CLOUDS)
def test_contact_field_matches_the_oracle(engine_mod, oracle_mod, name):
    """Engine.contact_field() at every point, for every parameter set on one handle (ppp_set_params recomputes the field):
    curv5 and half_width bit-equal, NaNs in the same places; the statistics are the maps'; `narrow` for a threshold that the
    free widths straddle.  No cloud's size is a multiple of 16, so the last wave of k_field_batch holds fewer than 16 queries,
    and every cloud but SADDLE and CREASE has rows without a value among rows with one"""
    pts = cloud(name)
    e = engine_mod.Engine(0, **DEFAULTS)
    e.set_cloud(pts)
    assert len(pts) % FIELD_Q != 0
    for label, extra in PARAM_SETS:
        P = params_of(extra)
        want_c, want_h = oracle_field(oracle_mod, name, extra)
        counted = ~ties(oracle_mod, name, P["curvature_k"])
        e.set_params(**P)
        R = P["tool_radius"]
        a = np.abs(want_h[np.isfinite(want_h)])
        free = a[(a > 0) & (a < F(0.98 * R))]               # (a released depth cancels some axes to 0: not a width to straddle)
        min_width = float(F(2) * np.median(free)) if len(free) >= 40 else float(int(2 * R))
        curv, hw, st = e.contact_field(min_width=min_width)
        print("%s %s: NaN widths %d of %d, free widths %d, narrow below %g: %d" % (name, label, int(np.isnan(want_h).sum()), len(pts), len(free), min_width, st["narrow"]))
        same_where(hw, want_h, counted, "%s %s half_width" % (name, label))
        same_where(curv, want_c, counted, "%s %s curv5" % (name, label))
        check_stats(hw, st, R, min_width)
        if len(free) >= 40:
            assert 10 <= st["narrow"] <= st["valid"] - 10                      # the threshold separates
    if name == "plane":
        assert np.isnan(oracle_field(oracle_mod, name, {})[1]).all()
    elif name not in ("saddle", "crease"):
        nan = np.isnan(oracle_field(oracle_mod, name, {})[1])
        assert 0 < nan.sum() < 0.5 * len(pts)
    e.close()


@pytest.mark.gpu
def test_curvature_k_below_three_is_refused_as_before(engine_mod):
    """ppp_set_params takes curvature_k 1 and 2 when no dynamic adjustment is asked for; every contact query refuses them
    (curvature_k must be in [3, 64]); with the dynamic adjustment ppp_set_params itself refuses"""
    e = engine_mod.Engine(0, **DEFAULTS)
    e.set_cloud(cloud("cyl_x"))
    for k in (1, 2):
        e.set_params(curvature_k=k)
        for call in (lambda: e.contact_field(), lambda: e.principal_curvatures_at(e.cloud()[:4]),
                     lambda: e.area2cloud(e.cloud()[:4].astype(np.float64), 0)):
            with pytest.raises(engine_mod.PPPError) as ex:
                call()
            assert ex.value.code == engine_mod.ERR_ARG
        with pytest.raises(engine_mod.PPPError) as ex:
            e.set_params(walk=1, dynamic_adjustment=1)
        assert ex.value.code == engine_mod.ERR_ARG
        e.set_params(dynamic_adjustment=0)
    e.set_params(curvature_k=3)
    assert e.contact_field(maps=False)[2]["n"] == len(cloud("cyl_x"))
    e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", CLOUDS)
def test_per_query_forms_match_the_oracle_and_the_field(engine_mod, oracle_mod, name):
    """principal_curvatures_at (k_field_waves) and area2cloud with key 0 and key 1 (k_area2cloud_api) at every cloud point and
    at 200 queries 0.5 .. 5 mm off the surface, for curvature_k 50 and 10, a released depth and tool_radius 15 with toolthickness
    0.5: bit-equal to the oracle (on PLANE: NaN in every place); at the cloud points (area2cloud(key 0).x - area2cloud(key 1).x) / 2
    and the curvature rows are the field's rows"""
    pts = cloud(name)
    e = engine_mod.Engine(0, **DEFAULTS)
    e.set_cloud(pts)
    Pm = e.cloud()
    Q = np.ascontiguousarray(np.concatenate([Pm, off_surface_queries(oracle_mod, name)]), np.float32)
    q64 = Q.astype(np.float64)
    for extra in ({}, dict(curvature_k=10), dict(depth=1e-7), dict(tool_radius=15.0, toolthickness=0.5)):
        P = params_of(extra)
        o = oracle_for(oracle_mod, name, extra)
        e.set_params(**P)
        counted = np.concatenate([~ties(oracle_mod, name, P["curvature_k"]), ~tie_mask(Pm, Q[len(Pm):], P["curvature_k"])])
        assert (~counted[len(Pm):]).sum() <= 2
        key = ("per query", name, tuple(sorted(extra.items())))
        want_c, want_a = shared(key, lambda: (np.stack([o.principal_curvature(q) for q in Q]),
                                               [np.stack([o.area2cloud(p, kk) for p in q64]) for kk in (0, 1)]))
        got_c = e.principal_curvatures_at(Q)
        same_where(got_c, want_c, counted, "%s %s principal_curvatures_at" % (name, extra))
        got_a = [e.area2cloud(q64, kk) for kk in (0, 1)]
        for kk in (0, 1):
            same_where(got_a[kk], want_a[kk], counted, "%s %s area2cloud key %d" % (name, extra, kk))
        if name == "plane":
            assert np.isnan(want_c[:, :3]).all() and (want_c[:, 3:] == 0).all()   # pc0 == pc1 == 0, no direction, no width
            assert np.isnan(want_a[0]).all() and np.isnan(want_a[1]).all()
        else:                                                # a quarter of the off-surface queries at least have answers (TIGHT: 45 % of its points lie on the flat plate, where there is none)
            assert np.isfinite(want_a[0][len(Pm):, 0]).sum() >= 50
        curv, hw, _ = e.contact_field()
        n = len(Pm)
        with np.errstate(invalid="ignore"):
            hw_q = (got_a[0][:n, 0] - got_a[1][:n, 0]) / F(2)
        same_floats(hw, hw_q, "%s %s field against area2cloud" % (name, extra))
        same_floats(curv, got_c[:n], "%s %s field against principal_curvatures_at" % (name, extra))
    e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cyl_x", "saddle"])
def test_coverage_on_curved_clouds(engine_mod, oracle_mod, name):
    """get_coverage after the contact pass (walk 3, brute pairing, adjusted) and path_coverage after an adjusted walk-1 pass:
    every flag as the existing restatements set it -- the coverage balls take both extrema of one ellipse (BOTH_X)"""
    pts = cloud(name)
    kw = dict(V1_CONTACT, tool_radius=R_TOOL, dynamic_adjustment=1)
    e = engine_mod.Engine(0, **kw)
    e.set_cloud(pts)
    want = restate_coverage(pts, R_TOOL, oracle_mod)
    assert e.gen_path() > 4
    flags, covered = e.coverage()
    print("%s coverage: %d of %d" % (name, covered, len(pts)))
    assert np.array_equal(flags, want), (int(flags.sum()), int(want.sum()), int((flags != want).sum()))
    assert covered == int(want.sum()) and 0 < covered
    e.close()
    kw = dict(tool_radius=R_TOOL, walk=1, pairing=0, dynamic_adjustment=1)
    want, S = restate_path_coverage(pts, kw, oracle_mod)
    e = engine_mod.Engine(0, **kw)
    e.set_cloud(pts)
    assert e.gen_path() == S
    flags, covered = e.path_coverage()
    print("%s path coverage: %d of %d" % (name, covered, len(pts)))
    assert np.array_equal(flags, want), (int(flags.sum()), int(want.sum()), int((flags != want).sum()))
    assert covered == int(want.sum()) and 0 < covered < len(pts)
    e.close()


PASSES = [("adjusted", 1, True), ("adjusted-slab", 1, False), ("plain-window", 0, True), ("plain-slab", 0, False)]


@pytest.mark.gpu
@pytest.mark.parametrize("label,dynamic,fast", PASSES, ids=[p[0] for p in PASSES])
@pytest.mark.parametrize("name", ["cyl_x", "saddle"])
def test_whole_pass_matches_the_oracle(engine_mod, oracle_mod, name, label, dynamic, fast):
    """a whole walk-1 pass: S and W equal, the knots of every slice bit-equal, waypoints within 1e-4 m / 1e-4 rad, the tail
    index equal.  With the dynamic adjustment, on a handle that may take the window path and on one kept off it (a plan with
    the adjustment runs the slab index either way: asserted); without it, on the window path and on the slab path"""
    pts = cloud(name)
    kw = dict(tool_radius=R_TOOL, walk=1, dynamic_adjustment=dynamic)
    o = oracle_mod.Oracle(pts, **kw)
    e = engine_mod.Engine(0, fast_path=fast, **kw)
    e.set_cloud(pts)
    So, S = o.gen_path(), e.gen_path()
    assert S == So > 4
    assert e.fast_path() == (fast and not dynamic)
    for s in range(S):
        assert all(np.array_equal(a, b) for a, b in zip(e.nodes(s), o.nodes(s))), s
    Wo, W = o.get_path(), e.get_path()
    assert W == Wo > 0
    wp, owp = e.waypoints(), o.waypoints()
    assert np.array_equal(np.isnan(wp), np.isnan(owp))
    ok = ~np.isnan(owp).any(axis=1)
    assert ok.sum() > 0.9 * W
    assert np.linalg.norm(wp[ok, :3] - owp[ok, :3], axis=1).max() <= TOL_M
    d = np.abs(wp[ok, 3:] - owp[ok, 3:])
    assert np.minimum(d, np.abs(d - 2 * np.pi)).max() <= TOL_RAD
    assert np.array_equal(e.tail_index(), o.tail_index())
    print("%s %s: S %d W %d" % (name, label, S, W))
    e.close(); o.close()


ELLCHECK_PASSES = [(name, extra) for name in ("cyl_x", "cyl_30", "saddle", "crease", "tight") for extra in ({}, dict(depth=1e-7))]


@pytest.mark.gpu
def test_windowed_fold_equals_the_full_fold_on_these_surfaces(engine_mod):
    """the test build that evaluates all 721 samples beside the windowed fold, every time, and raises a device error on any
    difference (-DDYN_ELL_CHECK, built as test_gpu_parity builds it): the adjusted walk-1 passes on CYL_X, CYL_30, SADDLE, CREASE
    and TIGHT, with the default and with a released depth, end without an error -- gen_path maps the device's verdict, so a
    difference is PPP_ERR_DOMAIN -- and give the product build's knots and waypoints.  (Only a pass brings the verdict to the
    host: ppp_area2cloud does not read it back, so the per-query forms are not run here; their windowed folds are compared with
    the oracle's fold over all 721 samples in the tests above.)  In a process of its own: the engine library is chosen when it
    is loaded"""
    src = os.path.join(ROOT, "polishpathplanning_amd", "csrc")
    subprocess.check_call(["make", "-C", src, "variant", "NAME=ellcheck", "DEFS=-DDYN_ELL_CHECK"], stdout=subprocess.DEVNULL)
    code = textwrap.dedent("""
        import hashlib, os, sys
        sys.path.insert(0, %r); sys.path.insert(0, %r)
        from polishpathplanning_amd import engine
        import test_contact_adversaries as T
        base = os.path.dirname(engine.LIB_PATH)
        sums = []
        for libname in ("libppp_hip.so", "libppp_hip_ellcheck.so"):
            engine.LIB_PATH = os.path.join(base, libname)
            engine._lib = None
            h = hashlib.md5()
            for name, extra in T.ELLCHECK_PASSES:
                e = engine.Engine(0, walk=1, dynamic_adjustment=1, **T.params_of(extra))
                e.set_cloud(T.cloud(name))
                S = e.gen_path()                     # (raises PPPError on a device error)
                W = e.get_path()
                assert S > 4 and W > 0, (libname, name, extra, S, W)
                for s in range(S):
                    for a in e.nodes(s):
                        h.update(a.tobytes())
                h.update(e.waypoints().tobytes())
                e.close()
            sums.append(h.hexdigest())
            print(libname, sums[-1])
        assert sums[0] == sums[1]
        print("no difference")
    """ % (ROOT, os.path.join(ROOT, "tests")))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "no difference" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


@pytest.mark.gpu
def test_two_fresh_handles_give_the_same_bytes_on_crease(engine_mod):
    pts = cloud("crease")
    out = []
    for _ in range(2):
        e = engine_mod.Engine(0, **DEFAULTS)
        e.set_cloud(pts)
        curv, hw, st = e.contact_field(min_width=12.0)
        q = np.concatenate([e.cloud(), e.cloud() + F(0.75)])
        a = [e.area2cloud(q.astype(np.float64), kk) for kk in (0, 1)]
        out.append([bits(curv).tobytes(), bits(hw).tobytes(), {k: v for k, v in st.items() if k != "hist"}, st["hist"].tobytes(),
                    bits(e.principal_curvatures_at(q)).tobytes(), bits(a[0]).tobytes(), bits(a[1]).tobytes()])
        e.close()
    for i, (x, y) in enumerate(zip(*out)):
        assert x == y, i
