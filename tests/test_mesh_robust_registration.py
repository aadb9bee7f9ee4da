"""Robust registration of a scan to the triangle mesh itself (ppp_get_mesh_robust_registration_terms, ppp_register_mesh_robust;
DESIGN.md 7v): ppp_register_mesh's pairs on the facets under ppp_register_robust's weights.

The yardstick is restate_mesh_robust_terms(): the search and the frame of restate_mesh_terms() of tests/test_mesh_registration.py
-- the moved points in double, the brute force over ALL valid triangles with the first minimum, the box's frame -- with the winner's
closest point and normal kept, and on them biweight(), trim_rank() and f32_from_bits() of the robust and the trimmed modules: the key
of (float)|r|, the k-th smallest key, sigma, the weight, every term ((product) w) 2^shift rounded and summed in int64.  The search is
written out here because restate_mesh_terms() hands back neither the closest point nor the winner; test_infinite_tune_restates_the_
mesh_loop ties the two bit for bit.  Every comparison of the engine with the restatement is for equal bytes."""
import ctypes
import functools
import math
import os
import subprocess

import numpy as np
import pytest

from test_registration import ALL_LOCKED, IDENTITY, NAN, apply, frame, motion_about, restate_step, rows_equal, stats_equal
from test_path_dwell import same
from test_trimesh import EDGE, FACE, VERTEX, BRANCH_REGION, closest_on_triangles, sheet
from test_mesh_registration import (KW0, MOTION, flat_case, flat_restated, mesh_box, part_way, restate_mesh_terms, restate_register_mesh, scan_engine,
                                    surface, wavy_case, wavy_restated)
from test_robust_registration import (DROPPED, INF, REJECTED, SIGMA_MIN, TUNE, UNPAIRED, USED, biweight, bits32, brows_equal, maps_equal, median_scan,
                                      robust_rms, tied_scan)
from test_trimmed_registration import NAN32_BITS, digit_heights, f32_from_bits, part_handle, trim_rank

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- the restatement


def restate_mesh_robust_terms(P, rv, tris, max_dist, T, tune=TUNE, sigma_min=SIGMA_MIN, flip=False, chunk=256, search=None):
    """One evaluation as restate_robust_terms() of tests/test_robust_registration.py gives it -- T, pairs (= paired), the weighted A / b /
    E, weight_sum, used, k, median_bits, sigma, shift, centre, length, n, indexed, status uint8[n], weight float32[n], residual
    float64[n] by cloud index -- on restate_mesh_terms()'s pairs; region uint8[pairs] for the census.  flip: every facet turned over;
    search: restate_mesh_terms()'s"""
    P = np.ascontiguousarray(P, np.float32)
    T = np.asarray(T, np.float64).reshape(3, 4)
    n = len(P)
    mn, mx, (a, b, c, N, A2) = mesh_box(rv, tris)
    cen, Ln, shift, _ = frame(mn, mx, n, max_dist)
    md2 = float(np.float32(max_dist)) * float(np.float32(max_dist))
    scale = 2.0 ** shift
    finite = np.isfinite(P).all(axis=1)
    rows = np.nonzero(finite)[0]                                              # the indexed points of the scan
    p = P[rows].astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        m = np.stack([((T[r, 0] * p[:, 0] + T[r, 1] * p[:, 1]) + T[r, 2] * p[:, 2]) + T[r, 3] for r in range(3)], axis=1)
    ok = np.isfinite(m).all(axis=1)
    paired = np.zeros(len(rows), bool)
    win = np.zeros(len(rows), np.int64)
    X = np.zeros((len(rows), 3))
    branch = np.zeros(len(rows), np.int64)
    if search is not None:
        paired, win, X, _, branch = search(m, ok, (a, b, c), md2)
    for s in range(0, len(rows) if search is None else 0, chunk):
        sel = np.nonzero(ok[s:s + chunk])[0] + s
        if not len(sel) or not len(a):
            continue
        x, D2, br = closest_on_triangles(m[sel][:, None, :], a[None], b[None], c[None])
        j = D2.argmin(axis=1)                                                # the first minimum: the lowest f
        i = np.arange(len(sel))
        hit = D2[i, j] <= md2
        paired[sel[hit]] = True
        win[sel[hit]] = j[hit]
        X[sel[hit]] = x[i, j][hit]
        branch[sel[hit]] = br[i, j][hit]
    mm, xx, f = m[paired], X[paired], win[paired]
    nn = N[f] / A2[f][:, None]
    if flip:
        nn = -nn
    e = mm - xx
    r = ((e[:, 0] * nn[:, 0]) + e[:, 1] * nn[:, 1]) + e[:, 2] * nn[:, 2]
    npairs = int(paired.sum())
    keys = np.abs(r).astype(np.float32).view(np.uint32)
    k = trim_rank(0.5, npairs)
    if npairs:
        tau = int(np.sort(keys)[k - 1])
        sigma = max(1.4826 * float(f32_from_bits(tau)), float(sigma_min))
        cs = float(tune) * sigma
    else:
        tau, sigma, cs = NAN32_BITS, NAN, NAN
    w = biweight(r, cs, float(tune))
    u = (mm - cen[None, :]) / Ln
    J = [u[:, 1] * nn[:, 2] - u[:, 2] * nn[:, 1], u[:, 2] * nn[:, 0] - u[:, 0] * nn[:, 2], u[:, 0] * nn[:, 1] - u[:, 1] * nn[:, 0],
         nn[:, 0], nn[:, 1], nn[:, 2]]
    fix = lambda v: int(np.rint(v * scale).astype(np.int64).sum(dtype=np.int64))
    A = np.array([fix((J[i] * J[q]) * w) for i in range(6) for q in range(i, 6)], np.int64)
    bb = np.array([fix((J[i] * r) * w) for i in range(6)], np.int64)
    at = rows[paired]
    status = np.full(n, UNPAIRED, np.uint8)
    status[~finite] = DROPPED
    status[at] = np.where(w > 0.0, USED, REJECTED)
    weight = np.full(n, np.nan, np.float32)
    weight[at] = w.astype(np.float32)
    residual = np.full(n, np.nan, np.float64)
    residual[at] = r
    return dict(T=T.copy(), pairs=npairs, A=A, b=bb, E=fix((r * r) * w), weight_sum=fix(w), used=int((w > 0.0).sum()), k=k, median_bits=tau,
                sigma=sigma, shift=shift, centre=cen, length=Ln, n=n, indexed=len(rows), status=status, weight=weight, residual=residual,
                region=BRANCH_REGION[branch[paired]])


def restate_register_mesh_robust(P, rv, tris, tune=TUNE, sigma_min=SIGMA_MIN, max_dist=2.0, iterations=30, min_step=1e-6, lock_eps=1e-9, T0=None, flip=False,
                                 search=None):
    """(T, rows, status, weight, residual, stats) as Engine.register_mesh_robust gives them: restate_register_robust()'s loop of
    tests/test_robust_registration.py -- "fewer than 6 pairs" read as used < 6 -- over restate_mesh_robust_terms()"""
    T = IDENTITY.copy() if T0 is None else np.asarray(T0, np.float64).reshape(3, 4).copy()
    rows, converged, locked, stop = [], 0, 0, False
    while True:
        row = restate_mesh_robust_terms(P, rv, tris, max_dist, T, tune, sigma_min, flip, search=search)
        row.update(locked=ALL_LOCKED, step2=NAN)
        rows.append(row)
        if stop or len(rows) > iterations:
            break
        if row["used"] >= 6 and not np.any(row["b"]):
            converged = 1
            break
        step = restate_step(dict(row, pairs=row["used"]), row["centre"], row["length"], lock_eps)
        if step is None:
            break
        mask, _, T, step2 = step
        row.update(locked=mask, step2=step2)
        locked |= mask
        if step2 < min_step * min_step:
            converged, stop = 1, True
    first, last = rows[0], rows[-1]
    stats = dict(n=first["n"], indexed=first["indexed"], steps=len(rows) - 1, converged=converged, locked=locked, shift=first["shift"],
                 centre=first["centre"], length=first["length"], T=last["T"].copy(), pairs_before=first["pairs"], pairs_after=last["pairs"],
                 rms_before=robust_rms(first), rms_after=robust_rms(last))
    return last["T"].copy(), rows, last["status"], last["weight"], last["residual"], stats


# ---------------------------------------------------------------- the cases

N_DIRTY = 1500
# The contaminated case's loops are capped at DIRTY_ITERATIONS: the numpy brute force takes about half a second an evaluation, four
# loops are restated (plain and robust, 13.7 % and 35 %), and both loops use every iteration they are given on this case.  Both restatements and the engine run under the same cap.
DIRTY_ITERATIONS = 12
DIRTY = dict(max_dist=2.0, iterations=DIRTY_ITERATIONS)
# the worst coordinate error over the clean points, mm, by the bit-exact restatements under DIRTY (test_census_of_the_contaminated_
# case prints and pins them), measured 2026-10-21
PLAIN_CLEAN_MM = 0.5778656938384029
ROBUST_CLEAN_MM = 0.05833872723098921
ROBUST_CLEAN_BITS = 0x3FADDE92DB184000
PAIRS_AT_IDENTITY = 1463                                   # of 1 500: the motion carries 37 raised points beyond max_dist at first
BEYOND_X = 20.0


@functools.lru_cache(maxsize=None)
def dirty_case(raise_below=7.0):
    """(verts, tris, scan float64[1500, 3] before the motion, moved float32[1500, 3]: what the engine gets, raised bool[1500]): the
    wavy sheet of tests/test_mesh_registration.py (768 facets); a scan that overhangs it by 1 mm, noise +-0.05 mm, every point with
    x < raise_below lifted by 1.5 mm -- within max_dist, so it pairs -- and the whole scan moved by MOTION; nobody writes to them"""
    v, t = wavy_case()[:2]
    rng = np.random.default_rng(11)
    x, y = rng.uniform(-1.0, 61.0, N_DIRTY), rng.uniform(-1.0, 41.0, N_DIRTY)
    z = surface(np.clip(x, 0.0, 60.0), np.clip(y, 0.0, 40.0)) + rng.uniform(-0.05, 0.05, N_DIRTY)
    raised = x < raise_below
    z[raised] += 1.5
    scan = np.stack([x, y, z], axis=1)
    Tm = motion_about(MOTION["c"], MOTION["deg"], MOTION["shift"])
    R, tt = Tm[:, :3], Tm[:, 3]
    moved = ((scan - tt) @ R).astype(np.float32)
    for arr in (scan, moved, raised):
        arr.setflags(write=False)
    return v, t, scan, moved, raised


def clean_error(T, moved, scan, raised):
    return float(np.abs(apply(T, moved[~raised]) - scan[~raised]).max())


@functools.lru_cache(maxsize=None)
def dirty_robust_restated(raise_below=7.0):
    v, t, scan, moved, raised = dirty_case(raise_below)
    return restate_register_mesh_robust(moved, v, t, **DIRTY)


@functools.lru_cache(maxsize=None)
def dirty_plain_restated(raise_below=7.0):
    v, t, scan, moved, raised = dirty_case(raise_below)
    return restate_register_mesh(moved, v, t, **DIRTY)


def census(row):
    reg = row["region"]
    return int((reg == FACE).sum()), int((reg == EDGE).sum()), int((reg == VERTEX).sum())


def flat_points(z):
    """points strictly inside the exactly planar sheet(8, 8, 4.0) (0 .. 32 mm both ways, z = 0, every normal (0, 0, +1)) at the
    heights z float32[n]: a 0.75 mm lattice from (2, 2), coordinates exact in float, so the residual of a point is its height"""
    z = np.asarray(z, np.float32)
    i = np.arange(len(z))
    pts = np.stack([2.0 + 0.75 * (i % 36), 2.0 + 0.75 * (i // 36), z], axis=1).astype(np.float32)
    assert pts[:, :2].min() >= 2.0 and pts[:, :2].max() <= 30.0
    return pts


# ---------------------------------------------------------------- CPU


def test_header_declares_and_engine_exports_mesh_robust_registration(engine_mod, tmp_path):
    hdr = open(os.path.join(ROOT, "include", "ppp_hip.h")).read()
    decls = ("int  ppp_get_mesh_robust_registration_terms(ppp_handle h, ppp_trimesh m, const ppp_robust_registration_params *bp, const double *T12,\n"
             "                                            ppp_robust_registration_row *row,\n"
             "                                            unsigned char *status, float *weight, double *residual, size_t cap,\n"
             "                                            ppp_registration_stats *stats);",
             "int  ppp_register_mesh_robust(ppp_handle h, ppp_trimesh m, const ppp_robust_registration_params *bp, const double *T0_12,\n"
             "                              ppp_robust_registration_row *rows, size_t row_cap,\n"
             "                              unsigned char *status, float *weight, double *residual, size_t cap,\n"
             "                              ppp_registration_stats *stats);")
    for decl in decls:
        assert decl in hdr, decl
    assert "DESIGN.md 7v" in hdr and "it is negated where the facet is flipped" in hdr
    assert hdr.count("} ppp_robust_registration_params;") == 1 and hdr.count("} ppp_robust_registration_row;") == 1   # no new struct
    L = ctypes.CDLL(engine_mod.LIB_PATH)
    for sym in ("ppp_get_mesh_robust_registration_terms", "ppp_register_mesh_robust"):
        assert sym in engine_mod.EXPORTS and hasattr(L, sym)
    for m in ("mesh_robust_registration_terms", "register_mesh_robust"):
        assert hasattr(engine_mod.Engine, m)
    planner = open(os.path.join(ROOT, "include", "ppp_planner.hpp")).read()
    assert "register_mesh_robust(" in planner and "print_mesh_robust_registration(" in planner
    for h in ("Path_Generate.h", "Path_Generate_Algorithm.h", "robot_path.h"):
        assert "register_robust_to_mesh(" in open(os.path.join(ROOT, "include", h)).read(), h
    src = tmp_path / "c99.c"
    src.write_text('#include "ppp_hip.h"\nint main(void) {\n'
                   '    int (*f)(ppp_handle, ppp_trimesh, const ppp_robust_registration_params *, const double *, ppp_robust_registration_row *,\n'
                   '             unsigned char *, float *, double *, size_t, ppp_registration_stats *) = ppp_get_mesh_robust_registration_terms;\n'
                   '    int (*g)(ppp_handle, ppp_trimesh, const ppp_robust_registration_params *, const double *, ppp_robust_registration_row *, size_t,\n'
                   '             unsigned char *, float *, double *, size_t, ppp_registration_stats *) = ppp_register_mesh_robust;\n'
                   '    return f == 0 || g == 0;\n}\n')
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_examples_build_with_the_mesh_robust_switch(engine_mod):
    for ex in ("connect.cpp", "robot.cpp"):
        src = open(os.path.join(ROOT, "examples", ex)).read()
        assert '"mesh-robust"' in src and "register_robust_to_mesh(" in src and "register_to_mesh(" in src and "register_robust_to(" in src, ex
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "examples"), "connect", "connect1", "robot", "main", "api_check"])
    for exe in ("connect", "connect1", "robot", "main", "api_check"):
        assert os.access(os.path.join(ROOT, "examples", exe), os.X_OK)


def test_infinite_tune_restates_the_mesh_loop():
    """with w = 1 every product is exact in the written order: rows and T are restate_register_mesh()'s, bit for bit, on the wavy
    case (3 iterations: the identity holds per evaluation) and on the flat one to its end"""
    v, t, scan, moved, Tm = wavy_case()
    T, rows, status, weight, residual, st = restate_register_mesh_robust(moved, v, t, tune=INF, iterations=3)
    wT, wrows, wst = restate_register_mesh(moved, v, t, iterations=3)
    rows_equal(rows, wrows)
    stats_equal(st, wst)
    assert same(T, wT) and st["steps"] == 3
    for row, want in zip(rows, wrows):
        assert row["used"] == row["pairs"] and row["weight_sum"] == row["pairs"] << row["shift"]
        assert np.array_equal(row["region"], want["region"])
    assert not np.any(status == REJECTED) and np.all(weight[status == USED] == 1.0)
    v, t, scan, T0 = flat_case()
    T, rows, _, _, _, st = restate_register_mesh_robust(scan, v, t, tune=INF, T0=T0)
    wT, wrows, wst = flat_restated()
    rows_equal(rows, wrows)
    stats_equal(st, wst)
    assert same(T, wT)


def test_census_of_the_contaminated_case():
    """Seed 11, x < 7 raised by 1.5 mm: 205 of 1 500 points (13.7 %).  In the pose the scan was made in -- the start of the
    construction, before MOTION -- every point pairs: the raised strip and the 1 mm overhang lie within max_dist.  Moved, 1 463 pair
    at the identity (PAIRS_AT_IDENTITY) and all 1 500 at the end.  Under DIRTY (12 iterations, the cap
    explained at DIRTY_ITERATIONS) the restatements give, measured 2026-10-21: the plain loop 0.5779 mm off over the clean points,
    not converged; the robust loop 0.0583 mm off, 1 294 of 1 500 pairs used, sigma 0.0873 mm, not converged either (its steps stay
    near 1e-5, above min_step); pairs at the identity 1 316 face, 147 edge, 0 vertex, at the end 1 375, 124, 1.  The plain loop must
    end at least 5 times worse than the robust one -- half the ratio of ten measured -- so the case cannot quietly stop being a
    contaminated one; every raised point ends REJECTED."""
    v, t, scan, moved, raised = dirty_case()
    assert len(t) == 768 and int(raised.sum()) == 205 and len(scan) == N_DIRTY
    T, rows, status, weight, residual, st = dirty_robust_restated()
    pT, prows, pst = dirty_plain_restated()
    e, pe = clean_error(T, moved, scan, raised), clean_error(pT, moved, scan, raised)
    last = rows[-1]
    print("plain: steps %d converged %d clean error %r mm; robust: steps %d converged %d clean error %r mm (bits %#x), used %d of %d, sigma %r mm"
          % (pst["steps"], pst["converged"], pe, st["steps"], st["converged"], e, int(np.float64(e).view(np.uint64)), last["used"], last["pairs"], last["sigma"]))
    for k in (0, len(rows) - 1):
        print("row %d: pairs %d: face / edge / vertex %r; used %d" % (k, rows[k]["pairs"], census(rows[k]), rows[k]["used"]))
    made = restate_mesh_robust_terms(moved, v, t, 2.0, motion_about(MOTION["c"], MOTION["deg"], MOTION["shift"]))
    assert made["pairs"] == N_DIRTY                                          # every point pairs where the scan was made
    assert rows[0]["pairs"] == prows[0]["pairs"] == PAIRS_AT_IDENTITY and last["pairs"] == N_DIRTY
    assert census(rows[0]) == (1316, 147, 0) and census(last) == (1375, 124, 1)
    assert (st["steps"], st["converged"], pst["steps"], pst["converged"]) == (DIRTY_ITERATIONS, 0, DIRTY_ITERATIONS, 0)
    assert (last["used"], last["pairs"]) == (1294, 1500)
    assert pe >= 5.0 * e
    assert np.all(status[raised] == REJECTED) and np.all(weight[raised] == 0.0)
    assert same(pe, PLAIN_CLEAN_MM) and same(e, ROBUST_CLEAN_MM)            # the constants are the measurement
    assert int(np.float64(e).view(np.uint64)) == ROBUST_CLEAN_BITS
    for r in rows:
        assert r["k"] == trim_rank(0.5, r["pairs"]) and r["used"] <= r["pairs"] and r["sigma"] >= SIGMA_MIN


def test_more_than_a_third_raised_is_beyond_the_estimator():
    """the median's known limit: with x < 20 raised (about 35 %) the median residual belongs to neither part; the robust loop does
    NOT recover the motion: it ends nearer to the plain loop's error than to the 13.7 % case's robust error"""
    v, t, scan, moved, raised = dirty_case(BEYOND_X)
    share = raised.sum() / N_DIRTY
    T = dirty_robust_restated(BEYOND_X)[0]
    pT = dirty_plain_restated(BEYOND_X)[0]
    e, pe = clean_error(T, moved, scan, raised), clean_error(pT, moved, scan, raised)
    print("share %r: plain %r mm, robust %r mm; the 13.7 %% case's robust error %r mm" % (share, pe, e, ROBUST_CLEAN_MM))
    assert 0.3 < share < 0.4
    assert abs(e - pe) < abs(e - ROBUST_CLEAN_MM)


def test_orientation_negates_the_residual_map_alone():
    """every facet turned over: r and J change sign together, so the key, the weight and every product are the same doubles; the
    rows are equal and the residual map is negated, bit for bit"""
    v, t, scan, moved, raised = dirty_case()
    for T in (IDENTITY, part_way(2.0 / 3.0), part_way(1.0)):                # (at the whole motion the raised strip is rejected)
        a, b = restate_mesh_robust_terms(moved, v, t, 2.0, T), restate_mesh_robust_terms(moved, v, t, 2.0, T, flip=True)
        brows_equal([dict(a, locked=0, step2=0.0)], [dict(b, locked=0, step2=0.0)])
        assert a["status"].tobytes() == b["status"].tobytes() and a["weight"].tobytes() == b["weight"].tobytes()
        paired = a["status"] <= REJECTED
        assert same(b["residual"][paired], -a["residual"][paired]) and np.any(a["residual"][paired] != 0)
    assert np.any(a["status"] == REJECTED) and np.any(a["status"] == USED)


# ---------------------------------------------------------------- GPU


def terms_parity(s, mesh, v, t, T=None, max_dist=2.0, lock_eps=1e-9, want=None, **kw):
    """Engine.mesh_robust_registration_terms against restate_mesh_robust_terms on the engine's own cloud (want: that evaluation, made
    by the caller): the row, the maps, stats"""
    if want is None:
        want = restate_mesh_robust_terms(s.cloud(), v, t, max_dist, IDENTITY if T is None else T, **kw)
    want = dict(want, locked=ALL_LOCKED, step2=NAN)
    row, status, weight, residual, st = s.mesh_robust_registration_terms(mesh, T=T, max_dist=max_dist, lock_eps=lock_eps, **kw)
    brows_equal([row], [want])
    maps_equal((status, weight, residual), (want["status"], want["weight"], want["residual"]))
    assert st["steps"] == 0 and st["converged"] == 0 and st["pairs_before"] == st["pairs_after"] == row["pairs"] and st["shift"] == want["shift"]
    assert same(st["rms_before"], robust_rms(want)) and same(st["rms_after"], robust_rms(want)) and same(st["T"], want["T"])
    assert same(st["centre"], want["centre"]) and same(st["length"], want["length"]) and st["indexed"] == want["indexed"] and st["n"] == want["n"]
    return row, status, weight, residual, want


def chain_parity(s, mesh, v, t, want=None, **kw):
    got = s.register_mesh_robust(mesh, **kw)
    if want is None:
        want = restate_register_mesh_robust(s.cloud(), v, t, **kw)
    T, rows, status, weight, residual, st = got
    print("steps %d (want %d) converged %d (want %d) used %r paired %r sigma %r" % (st["steps"], want[5]["steps"], st["converged"], want[5]["converged"],
                                                                                 [w["used"] for w in rows], [w["pairs"] for w in rows], [w["sigma"] for w in rows]))
    brows_equal(rows, want[1])
    stats_equal(st, want[5])
    maps_equal((status, weight, residual), want[2:5])
    assert same(T, want[0]) and same(T, rows[-1]["T"]) and rows[-1]["locked"] == ALL_LOCKED and math.isnan(rows[-1]["step2"])
    return got, want


@pytest.mark.gpu
@pytest.mark.parametrize("cell", [0.0, 0.9, 25.0])
def test_terms_match_the_restatement(engine_mod, cell):
    v, t, scan, moved, raised = dirty_case()
    s = scan_engine(engine_mod, moved)
    mesh = s.trimesh(v, t, cell=cell)
    print("grid %r cell %r" % (mesh.stats["cells"], mesh.stats["cell"]))
    for T in (None, part_way(2.0 / 3.0), part_way(1.0)):                    # the identity, part-way, and the whole motion: the strip rejected
        row, status, weight, residual, want = terms_parity(s, mesh, v, t, T=T)
        print("pairs %d used %d median %r sigma %r" % (row["pairs"], row["used"], row["median_abs"], row["sigma"]))
        assert 6 <= row["used"] <= row["pairs"]
        again = s.mesh_robust_registration_terms(mesh, T=T)                   # the same bits in every run
        assert same(again[:4], (row, status, weight, residual))
    assert row["used"] < row["pairs"] and np.all(status[raised] == REJECTED)
    mesh.close(); s.close()


@pytest.mark.gpu
def test_chain_matches_the_restatement_on_the_contaminated_case(engine_mod):
    v, t, scan, moved, raised = dirty_case()
    s = scan_engine(engine_mod, moved)
    mesh = s.trimesh(v, t)
    got = s.register_mesh_robust(mesh, **DIRTY)
    want = dirty_robust_restated()
    T, rows, status, weight, residual, st = got
    print("steps %d converged %d used %r sigma %r" % (st["steps"], st["converged"], [w["used"] for w in rows], [w["sigma"] for w in rows]))
    brows_equal(rows, want[1])
    stats_equal(st, want[5])
    maps_equal((status, weight, residual), want[2:5])
    assert same(T, want[0])
    e = clean_error(T, moved, scan, raised)
    assert int(np.float64(e).view(np.uint64)) == ROBUST_CLEAN_BITS          # the census's error, reached by the engine's T
    assert np.all(status[raised] == REJECTED) and rows[-1]["used"] < rows[-1]["pairs"]
    mesh.close(); s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["wavy", "flat"])
def test_infinite_tune_is_register_mesh_bit_for_bit(engine_mod, case):
    if case == "wavy":
        v, t, _, pts, _ = wavy_case()
        T0 = None
    else:
        v, t, pts, T0 = flat_case()
    s = scan_engine(engine_mod, pts)
    mesh = s.trimesh(v, t)
    T, rows, st = s.register_mesh(mesh, T0=T0)
    bT, brows, status, weight, residual, bst = s.register_mesh_robust(mesh, tune=INF, T0=T0)
    assert st["steps"] >= 1
    rows_equal(brows, rows)
    stats_equal(bst, st)
    assert same(bT, T)
    for w in brows:
        assert w["used"] == w["pairs"] and w["weight_sum"] == w["pairs"] << st["shift"]
    assert not np.any(status == REJECTED) and int((status == USED).sum()) == brows[-1]["pairs"] and np.all(weight[status == USED] == 1.0)
    mesh.close(); s.close()


@pytest.mark.gpu
def test_median_on_ties_and_digit_edges(engine_mod):
    """the planar sheet: the residual of a point strictly inside it is its height, exactly.  The heights are median_scan()'s and
    tied_scan()'s of tests/test_robust_registration.py: the median inside a tied group, and on the first and the last rank of keys
    that differ in the low, the middle and the top digit, for an even and an odd number of pairs; then all keys equal"""
    v, t = sheet(8, 8, 4.0)
    s = engine_mod.Engine(0, **KW0)
    s.set_cloud(flat_points(tied_scan()[:, 2]))
    mesh = s.trimesh(v, t)
    kw = dict(max_dist=3.0, lock_eps=1e-3)
    row, _, _, _, want = terms_parity(s, mesh, v, t, **kw)
    assert row["median_bits"] == bits32(0.5) and row["pairs"] // 3 < want["k"] < 2 * row["pairs"] // 3
    for odd in (False, True):
        for zt in digit_heights():
            for where in ("first", "last"):
                z = median_scan(zt, where, odd)[:, 2]
                s.set_cloud(flat_points(z))
                row, _, _, residual, want = terms_parity(s, mesh, v, t, **kw)
                assert row["pairs"] == len(z) and row["pairs"] % 2 == (1 if odd else 0), (odd, zt, where)
                assert row["median_bits"] == bits32(zt), (odd, zt, where, row["median_abs"])
                assert np.array_equal(residual, z.astype(np.float64))
    s.set_cloud(flat_points(np.full(101, 0.375, np.float32)))
    row, status, weight, _, _ = terms_parity(s, mesh, v, t, **kw)
    assert row["median_bits"] == bits32(0.375) and row["used"] == row["pairs"] == 101 and np.all(status == USED)
    mesh.close(); s.close()


@pytest.mark.gpu
def test_sigma_floor(engine_mod):
    """a scan lying exactly on the flat mesh with sigma_min = 0: the median, sigma and cs are 0, every weight is 1, b = 0, E = 0 and
    the loop ends converged with no step.  Then sigma_min binds: a residual of exactly cs has weight 0, the float below it not"""
    v, t = sheet(8, 8, 4.0)
    s = engine_mod.Engine(0, **KW0)
    s.set_cloud(flat_points(np.zeros(400, np.float32)))
    mesh = s.trimesh(v, t)
    (T, rows, status, weight, residual, st), _ = chain_parity(s, mesh, v, t, sigma_min=0.0, max_dist=3.0, lock_eps=1e-3)
    row = rows[0]
    assert st["steps"] == 0 and st["converged"] == 1 and len(rows) == 1 and same(T, IDENTITY)
    assert row["pairs"] == row["used"] == 400 and row["median_bits"] == 0 and row["sigma"] == 0.0 and not np.any(row["b"]) and row["E"] == 0
    assert row["weight_sum"] == 400 << st["shift"] and st["rms_after"] == 0.0 and np.all(weight == 1.0) and np.all(residual == 0.0)
    tune, sigma_min = 4.0, 0.25
    z = np.zeros(400, np.float32)
    at, below = np.float32(tune * sigma_min), np.nextafter(np.float32(tune * sigma_min), np.float32(0))
    z[5:25:2] = at
    z[6:26:2] = below
    s.set_cloud(flat_points(z))
    row, status, weight, residual, want = terms_parity(s, mesh, v, t, max_dist=3.0, lock_eps=1e-3, tune=tune, sigma_min=sigma_min)
    assert row["median_bits"] == 0 and row["sigma"] == sigma_min and row["pairs"] == 400 and row["used"] == 390
    assert np.all(status[5:25:2] == REJECTED) and np.all(weight[5:25:2] == 0.0) and np.all(status[6:26:2] == USED) and np.all(weight[6:26:2] > 0.0)
    mesh.close(); s.close()


def few_used_scan(k):
    """k points of the contaminated case's clean part well inside the mesh, 20 more 50 mm above it"""
    v, t, scan, moved, raised = dirty_case()
    inside = np.nonzero((scan[:, 0] > 10) & (scan[:, 0] < 55) & (scan[:, 1] > 5) & (scan[:, 1] < 35))[0]
    far = scan[inside[40:60]] + np.array([0.0, 0.0, 50.0])
    return np.concatenate([scan[inside[:k]], far]).astype(np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [0, 5, 6, 7])
def test_few_pairs(engine_mod, k):
    """k pairs, every one of them used at tune = 1e6: no step below 6; without a pair the median is the float NaN, sigma the double
    one, and the maps hold no number"""
    v, t = dirty_case()[:2]
    s = scan_engine(engine_mod, few_used_scan(k))
    mesh = s.trimesh(v, t)
    (T, rows, status, weight, residual, st), _ = chain_parity(s, mesh, v, t, T0=part_way(0.1), iterations=3, tune=1e6)
    assert rows[0]["pairs"] == rows[0]["used"] == k and st["indexed"] == k + 20
    assert int((status == USED).sum()) == rows[-1]["used"] and int((status == UNPAIRED).sum()) == k + 20 - rows[-1]["pairs"]
    if k == 0:
        assert rows[0]["median_bits"] == NAN32_BITS and math.isnan(rows[0]["sigma"]) and rows[0]["weight_sum"] == 0
        assert math.isnan(st["rms_before"]) and np.all(np.isnan(weight)) and np.all(np.isnan(residual))
    if k < 6:
        assert st["steps"] == 0 and st["converged"] == 0 and len(rows) == 1 and same(T, part_way(0.1))
    else:
        assert st["steps"] >= 1
    mesh.close(); s.close()


@pytest.mark.gpu
def test_the_ends_of_a_chain(engine_mod):
    v, t, scan, moved, raised = dirty_case()
    s = scan_engine(engine_mod, moved)
    mesh = s.trimesh(v, t)
    # the iteration cap: the last row comes from the evaluation no step follows
    (T, rows, _, _, _, st), _ = chain_parity(s, mesh, v, t, iterations=2)
    assert st["steps"] == 2 and st["converged"] == 0 and len(rows) == 3
    # a min_step so large that the first step ends the loop: converged
    (T, rows, _, _, _, st), _ = chain_parity(s, mesh, v, t, min_step=10.0)
    assert st["steps"] == 1 and st["converged"] == 1 and len(rows) == 2
    mesh.close(); s.close()
    # b == 0: the scan lies on the flat mesh; every residual is 0 (sigma from the floor), a stationary point
    v, t = sheet(8, 8, 4.0)
    s = engine_mod.Engine(0, **KW0)
    s.set_cloud(flat_points(np.zeros(300, np.float32)))
    mesh = s.trimesh(v, t)
    (T, rows, _, _, _, st), _ = chain_parity(s, mesh, v, t, lock_eps=1e-3)
    assert st["steps"] == 0 and st["converged"] == 1 and not np.any(rows[0]["b"]) and rows[0]["used"] == 300
    mesh.close(); s.close()


@pytest.mark.gpu
def test_scatter_with_a_long_run_and_dropped_points(engine_mod):
    """more than 2 x 256 points, not a multiple of 64, every seventh not finite: DROPPED entries, the scatter by cloud index over
    more than two workgroups of the walk, and cap < n"""
    v, t, scan, moved, raised = dirty_case()
    pts = moved[:843].copy()
    pts[3::7, 1] = np.nan
    pts[5::49, 0] = np.inf
    s = scan_engine(engine_mod, pts)
    mesh = s.trimesh(v, t)
    assert len(pts) > 2 * 256 and len(pts) % 64 != 0
    (T, rows, status, weight, residual, st), want = chain_parity(s, mesh, v, t, iterations=3)
    bad = ~np.isfinite(pts).all(axis=1)
    assert st["n"] == 843 and st["indexed"] == 843 - int(bad.sum()) and np.all(status[bad] == DROPPED) and not np.any(status[~bad] == DROPPED)
    assert np.any(status == REJECTED) and np.any(status == USED)
    E = engine_mod
    bp = E.RobustRegistrationParams(E.RegistrationParams(2.0, 3, 1e-6, 1e-9), TUNE, SIGMA_MIN)
    raw = E.RegistrationStats()
    st8 = np.full(600, 0xA5, np.uint8); w8 = np.full(600, 7.0, np.float32); r8 = np.full(600, 7.0, np.float64)
    assert s.L.ppp_register_mesh_robust(s.h, mesh.m, ctypes.byref(bp), None, None, 0, st8.ctypes.data_as(ctypes.POINTER(ctypes.c_ubyte)),
                                        w8.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), r8.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), 517,
                                        ctypes.byref(raw)) == 0
    assert st8[:517].tobytes() == status[:517].tobytes() and w8[:517].tobytes() == weight[:517].tobytes() and r8[:517].tobytes() == residual[:517].tobytes()
    assert np.all(st8[517:] == 0xA5) and np.all(w8[517:] == 7.0) and np.all(r8[517:] == 7.0)
    stats_equal(E._registration_stats(raw), st)
    mesh.close(); s.close()


@pytest.mark.gpu
def test_flipped_winding_on_the_device(engine_mod):
    """The same mesh with every triangle's winding reversed.  On the planar sheet under flat_case()'s tilted start the identity of
    the header holds in every bit, whatever order a record keeps its vertices in: the closest point's z is 0 and the normal (0, 0,
    -+1) exactly, so r = -+ the moved point's z and J is negated with it -- the rows and T are equal, the residual map is negated.
    On the wavy sheet a reversed triangle is another record (its vertices in another order), so its closest point may differ in the
    last bit, and with it the winner between two facets that meet in an edge: there the turned mesh is held against the restatement
    of the turned triangles, bit for bit, and against the mesh as given only in what survives that: the typical pair's residual is
    negated to within rounding"""
    v, t, pts, T0 = flat_case()
    s = scan_engine(engine_mod, pts)
    mesh, turned = s.trimesh(v, t), s.trimesh(v, np.ascontiguousarray(t[:, ::-1]))
    kw = dict(tune=0.8, sigma_min=0.01, lock_eps=1e-3)                      # a cut just above the median: the tilt's high side is rejected
    a, b = s.mesh_robust_registration_terms(mesh, T=T0, **kw), s.mesh_robust_registration_terms(turned, T=T0, **kw)
    assert same((a[0], a[1], a[2], a[4]), (b[0], b[1], b[2], b[4])) and np.any(a[0]["b"]) and a[0]["used"] < a[0]["pairs"] == 400
    assert same(b[3], -a[3]) and np.all(a[3] > 0)
    a, b = s.register_mesh_robust(mesh, T0=T0, **kw), s.register_mesh_robust(turned, T0=T0, **kw)
    assert same((a[0], a[1], a[2], a[3], a[5]), (b[0], b[1], b[2], b[3], b[5])) and a[5]["steps"] >= 1
    assert same(b[4], -a[4]) and np.any(a[4] != 0)
    turned.close(); mesh.close(); s.close()
    v, t, scan, moved, raised = dirty_case()
    back = np.ascontiguousarray(t[:, ::-1])
    s = scan_engine(engine_mod, moved)
    mesh, turned = s.trimesh(v, t), s.trimesh(v, back)
    for T in (None, part_way(2.0 / 3.0)):
        b = terms_parity(s, turned, v, back, T=T)
        a = s.mesh_robust_registration_terms(mesh, T=T)
        paired = a[1] <= REJECTED
        both = paired & (b[1] <= REJECTED)
        assert int(both.sum()) >= 0.9 * a[0]["pairs"] and float(np.median(np.abs(b[3][both] + a[3][both]))) <= 1e-12 and np.any(a[3][both] != 0)
    turned.close(); mesh.close(); s.close()


@pytest.mark.gpu
def test_a_mesh_on_another_device_is_refused(engine_mod):
    from test_deviation_tiles import device_count
    if device_count() < 2:
        pytest.skip("needs two GPUs in one process: this machine shows %d" % device_count())
    E = engine_mod
    v, t, scan, moved, raised = dirty_case()
    s = scan_engine(engine_mod, moved)
    other = E.Engine(1, **KW0)
    far = other.trimesh(v, t)
    for call in (s.register_mesh_robust, s.mesh_robust_registration_terms):
        with pytest.raises(E.PPPError) as ex:
            call(far)
        assert ex.value.code == E.ERR_ARG
    far.close(); other.close(); s.close()


@pytest.mark.gpu
def test_same_bits_on_fresh_handles_and_nothing_stored_is_touched(engine_mod):
    from polishpathplanning_amd import synth
    v, t, scan, moved, raised = dirty_case()
    out = []
    for _ in range(2):
        s = scan_engine(engine_mod, moved)
        mesh = s.trimesh(v, t)
        dev0 = s.mesh_deviation(mesh)
        reg0 = s.register_mesh(mesh, iterations=4)
        cloud0 = s.cloud().copy()
        near0 = mesh.nearest(np.ascontiguousarray(moved[::7]), 2.0)
        out.append(s.register_mesh_robust(mesh, iterations=4))
        assert same(s.register_mesh_robust(mesh, iterations=4), out[-1])
        s.mesh_robust_registration_terms(mesh, T=part_way(0.5))
        assert same(s.mesh_deviation(mesh), dev0) and same(s.register_mesh(mesh, iterations=4), reg0) and same(s.cloud(), cloud0)
        assert same(mesh.nearest(np.ascontiguousarray(moved[::7]), 2.0), near0)
        assert same(s.register_mesh_robust(mesh, iterations=4), out[-1])
        mesh.close(); s.close()
    assert same(out[0], out[1]) and out[0][5]["steps"] >= 3
    # the plan of a handle that has one survives both calls
    pts, cfg = synth.make_config("tiny_5k")
    w = engine_mod.Engine(0, tool_radius=cfg["tool_radius"], walk=1)
    w.set_cloud(pts)
    S = w.gen_path(); W = w.get_path(); wp = w.waypoints().copy()
    mesh = w.trimesh(v, t)
    w.register_mesh_robust(mesh, iterations=2)
    w.mesh_robust_registration_terms(mesh)
    assert (w.gen_path(), w.get_path()) == (S, W) and same(w.waypoints(), wp)
    mesh.close(); w.close()


@pytest.mark.gpu
def test_refusals(engine_mod):
    from polishpathplanning_amd import synth
    from polishpathplanning_amd.robot_path import slice_ranges
    E = engine_mod
    v, t, scan, moved, raised = dirty_case()
    s = scan_engine(engine_mod, moved)
    mesh = s.trimesh(v, t)
    L = s.L
    dp = ctypes.POINTER(ctypes.c_double)
    good = dict(max_dist=2.0, iterations=3, min_step=1e-6, lock_eps=1e-9, tune=TUNE, sigma_min=SIGMA_MIN)

    def raw(h, m, T0=None, rows=None, cap=0, params=True, **k):
        p = dict(good, **k)
        bp = E.RobustRegistrationParams(E.RegistrationParams(p["max_dist"], p["iterations"], p["min_step"], p["lock_eps"]), p["tune"], p["sigma_min"])
        st, row = E.RegistrationStats(), E.RobustRegistrationRow()
        t12 = None if T0 is None else np.ascontiguousarray(np.asarray(T0, np.float64).reshape(12))
        tp = None if t12 is None else t12.ctypes.data_as(dp)
        a = L.ppp_register_mesh_robust(h.h, m, ctypes.byref(bp) if params else None, tp, rows, cap, None, None, None, 0, ctypes.byref(st))
        b = L.ppp_get_mesh_robust_registration_terms(h.h, m, ctypes.byref(bp) if params else None, tp, ctypes.byref(row), None, None, None, 0, ctypes.byref(st))
        return a, b

    def refused(code, h=None, m=mesh.m, loop_only=False, **k):
        h = h or s
        a, b = raw(h, m, **k)
        text = L.ppp_last_error(h.h).decode()
        assert a == code and (loop_only or b == code), (k, a, b, text)
        assert text, k                                                       # the last-error text is set
        assert raw(s, mesh.m) == (0, 0)                                      # and the handle still works

    refused(E.ERR_ARG, m=None)
    refused(E.ERR_ARG, params=False)
    for bad in (dict(tune=0.0), dict(tune=-1.0), dict(tune=NAN), dict(tune=-INF), dict(sigma_min=-1e-9), dict(sigma_min=NAN), dict(sigma_min=INF),
                dict(max_dist=0.0), dict(max_dist=INF), dict(max_dist=NAN), dict(lock_eps=0.0), dict(lock_eps=1.0), dict(min_step=-1.0)):
        refused(E.ERR_ARG, **bad)
    for bad in (dict(iterations=0), dict(iterations=65)):
        refused(E.ERR_ARG, loop_only=True, **bad)
    Tb = IDENTITY.copy(); Tb[1, 2] = NAN
    refused(E.ERR_ARG, T0=Tb)
    refused(E.ERR_ARG, loop_only=True, rows=None, cap=1)
    refused(E.ERR_ARG, max_dist=3.0e6)                                        # shift < 16: n max_dist^2 leaves too few fractional bits
    assert raw(s, mesh.m, tune=INF) == (0, 0)                                # +INFINITY is a tune
    empty = E.Engine(0, **KW0)                                               # a handle without a cloud
    a, b = raw(empty, mesh.m)
    assert a == b == E.ERR_ARG and L.ppp_last_error(empty.h).decode()
    empty.close()
    pts, cfg = synth.make_config("tiny_5k")
    w = E.Engine(0, tool_radius=cfg["tool_radius"], walk=1)
    w.set_cloud(pts)
    S = w.gen_path()
    lo, hi = slice_ranges(S, 2)[1]
    h = E.Engine(0, tool_radius=cfg["tool_radius"], walk=1, slice_begin=lo, slice_end=hi)
    h.set_cloud(pts)
    part = part_handle(engine_mod, w, pts, cfg)
    for bad in (h, part):
        a, b = raw(bad, mesh.m)
        assert a == b == E.ERR_UNSUPPORTED and L.ppp_last_error(bad.h).decode()
    assert raw(w, mesh.m) == (0, 0)                                          # the whole-cloud handle of the same cloud is served
    chain_parity(s, mesh, v, t, iterations=3)                                # every refusal leaves a later good call working
    for e in (part, w, h, s):
        e.close()
    mesh.close()


@pytest.mark.gpu
def test_connect_registers_robust_against_the_triangles(engine_mod, tmp_path):
    """PPP_REGISTER=mesh-robust PPP_DEVIATION=<part.stl> ./connect <scan.pcd>: exit status 0, the robust line with
    ppp_register_mesh_robust's numbers, ppp_register's lines behind it and the deviation taken behind them"""
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "examples"), "connect"])
    v, t, scan, moved, raised = dirty_case()
    soup = v[t]                                                              # float32[768, 3, 3]; millimetres, as the scan
    stl, scan_pcd = str(tmp_path / "part.stl"), str(tmp_path / "scan.pcd")
    engine_mod.save_stl(stl, soup)
    engine_mod.save_pcd(scan_pcd, moved, binary=True)
    conf = tmp_path / "config.txt"
    conf.write_text("Tool_Radius = 6\npathFile = %s\nPathResolution = 7\nRPYresolution = 7\nEnd effector length = 0.3\n"
                    "Smooth = false\nAlignment = false\nChangeRange = false\nRemoveOutlier = false\nDynamic_adjustment = false\n"
                    "Adjust_Threshold = 1\ntoolthickness = 10\ndepth = 0.01\n" % str(tmp_path / "wp.txt"))
    exe = os.path.join(ROOT, "examples", "connect")
    env = {k: val for k, val in os.environ.items() if not k.startswith("PPP_")}
    env.update(PPP_CONFIG=str(conf), PPP_DEVIATION=stl, PPP_REGISTER="mesh-robust", PPP_REGISTER_TUNE="4.0", PPP_REGISTER_SIGMA_MIN="0.001",
               PPP_DEVIATION_EXACT="1")
    run = subprocess.run([exe, scan_pcd], env=env, capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert run.returncode == 0, run.stderr
    out = run.stdout.splitlines()
    reg = [ln for ln in out if ln.startswith("registration: ")]
    print("\n".join(reg))
    s = scan_engine(engine_mod, moved)
    mesh = s.trimesh_stl(stl)
    T, rows, status, weight, residual, st = s.register_mesh_robust(mesh, tune=4.0, sigma_min=0.001)
    want = ("registration: robust, tune %f: %d of %d pairs used, median %f mm, sigma %f mm; after %d steps %d of %d, median %f mm, sigma %f mm"
            % (4.0, rows[0]["used"], rows[0]["pairs"], rows[0]["median_abs"], rows[0]["sigma"], st["steps"], rows[-1]["used"], rows[-1]["pairs"],
               rows[-1]["median_abs"], rows[-1]["sigma"]))
    assert reg[0] == want and len(reg) == 6 and st["steps"] >= 1 and rows[-1]["used"] < rows[-1]["pairs"]
    dev = [ln for ln in out if ln.startswith("deviation: ")]
    assert dev and " matched, " in dev[0] and out.index(dev[0]) > out.index(reg[-1])
    mesh.close(); s.close()
