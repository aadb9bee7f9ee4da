"""Registration of a scan to the triangle mesh itself (ppp_get_mesh_registration_terms, ppp_register_mesh).  The
yardstick is restate_mesh_terms(): the rule of include/ppp_hip.h in numpy float64 -- the moved points in double, the brute force of
tests/test_trimesh.py over ALL valid triangles with the first minimum (the lowest f), the terms rounded to 2^-shift and summed in
int64 -- and restate_step() of tests/test_registration.py for the solve and the composition.  It knows nothing of a grid, of a
cell or of the order the device sums in: a row that differs in one bit fails.  The CPU tests check the restatement itself and
that the GPU tests' input holds what they claim."""
import ctypes
import functools
import math
import os
import subprocess

import numpy as np
import pytest

from test_registration import ALL_LOCKED, IDENTITY, NAN, apply, clog2, frame, motion_about, restate_step, rms_of, rows_equal, stats_equal
from test_path_dwell import same
from test_trimesh import EDGE, FACE, VERTEX, BRANCH_REGION, closest_on_triangles, frames, sheet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KW0 = dict(change_range=0)                                                    # resident units are the inputs' float32, as given


# ---------------------------------------------------------------- the restatement


def mesh_box(rv, tris):
    """(mn, mx) float32[3]: the box over the valid triangles' vertices; (p0, p1, p2, N, A2) of the valid triangles, ascending f"""
    p0, p1, p2, N, A2, valid = frames(rv, tris)
    fi = np.nonzero(valid)[0]
    allv = np.concatenate([p0[fi], p1[fi], p2[fi]])
    mn, mx = allv.min(axis=0), allv.max(axis=0)
    for d in range(3):                                                        # the box orders -0 below +0, as ppp_trimesh_stats reports it
        zero = allv[allv[:, d] == 0.0, d]
        if mn[d] == 0.0:
            mn[d] = -0.0 if np.signbit(zero).any() else 0.0
        if mx[d] == 0.0:
            mx[d] = 0.0 if (~np.signbit(zero)).any() else -0.0
    return mn.astype(np.float32), mx.astype(np.float32), (p0[fi], p1[fi], p2[fi], N[fi], A2[fi])


def restate_mesh_terms(P, rv, tris, max_dist, T, flip=False, chunk=256, search=None):
    """One evaluation, as restate_terms() of tests/test_registration.py gives it: dict(T, pairs, A, b, E, shift, centre, length, n,
    indexed) and, for the census, moved float64[indexed, 3], paired bool[indexed], region uint8[pairs].  P float32[n, 3] the scan,
    rv / tris the mesh's resident vertices and indices, T float64[3, 4]; flip: every facet normal negated.  search: the brute force
    below made by the caller -- search(m, ok, (a, b, c), md2) gives (paired, win, X, D2, branch) of the moved points m float64[indexed, 3]
    as the loop leaves them, zeros without a pair --, so that evaluations at one T share it (tests/test_mesh_registration_adversaries.py)"""
    P = np.ascontiguousarray(P, np.float32)
    T = np.asarray(T, np.float64).reshape(3, 4)
    n = len(P)
    mn, mx, (a, b, c, N, A2) = mesh_box(rv, tris)
    cen, Ln, shift, _ = frame(mn, mx, n, max_dist)
    md2 = float(np.float32(max_dist)) * float(np.float32(max_dist))
    scale = 2.0 ** shift
    rows = np.nonzero(np.isfinite(P).all(axis=1))[0]                         # the indexed points of the scan
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
        r = np.arange(len(sel))
        hit = D2[r, j] <= md2
        paired[sel[hit]] = True
        win[sel[hit]] = j[hit]
        X[sel[hit]] = x[r, j][hit]
        branch[sel[hit]] = br[r, j][hit]
    mm, xx, f = m[paired], X[paired], win[paired]
    nn = N[f] / A2[f][:, None]
    if flip:
        nn = -nn
    e = mm - xx
    r = ((e[:, 0] * nn[:, 0]) + e[:, 1] * nn[:, 1]) + e[:, 2] * nn[:, 2]
    u = (mm - cen[None, :]) / Ln
    J = [u[:, 1] * nn[:, 2] - u[:, 2] * nn[:, 1], u[:, 2] * nn[:, 0] - u[:, 0] * nn[:, 2], u[:, 0] * nn[:, 1] - u[:, 1] * nn[:, 0],
         nn[:, 0], nn[:, 1], nn[:, 2]]
    fix = lambda v: int(np.rint(v * scale).astype(np.int64).sum(dtype=np.int64))
    A = np.array([fix(J[i] * J[k]) for i in range(6) for k in range(i, 6)], np.int64)
    bb = np.array([fix(J[i] * r) for i in range(6)], np.int64)
    return dict(T=T.copy(), pairs=int(paired.sum()), A=A, b=bb, E=fix(r * r), shift=shift, centre=cen, length=Ln, n=n, indexed=len(rows),
                moved=m, paired=paired, region=BRANCH_REGION[branch[paired]])


def restate_register_mesh(P, rv, tris, max_dist=2.0, iterations=30, min_step=1e-6, lock_eps=1e-9, T0=None, search=None):
    """(T, rows, stats) as Engine.register_mesh gives them: restate_register()'s loop of tests/test_registration.py over
    restate_mesh_terms()"""
    T = IDENTITY.copy() if T0 is None else np.asarray(T0, np.float64).reshape(3, 4).copy()
    rows, converged, locked, stop = [], 0, 0, False
    while True:
        row = restate_mesh_terms(P, rv, tris, max_dist, T, search=search)
        row.update(locked=ALL_LOCKED, step2=NAN)
        rows.append(row)
        if stop or len(rows) > iterations:
            break
        if row["pairs"] >= 6 and not np.any(row["b"]):
            converged = 1
            break
        step = restate_step(row, row["centre"], row["length"], lock_eps)
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
                 rms_before=rms_of(first, first["shift"]), rms_after=rms_of(last, first["shift"]))
    return last["T"].copy(), rows, stats


# ---------------------------------------------------------------- the cases


def surface(x, y):
    return 3.0 * np.sin(0.21 * x) * np.cos(0.17 * y) + 0.002 * x * y


MOTION = dict(c=[30.0, 20.0, 0.0], deg=(1.0, -0.8, 1.5), shift=(0.4, -0.3, 0.35))
N_SCAN, N_RAISED = 1500, 150


@functools.lru_cache(maxsize=None)
def wavy_case():
    """(verts float32[425, 3], tris int32[768, 3], scan float32[1500, 3] before the motion, moved float32[1500, 3]: what the
    engine gets, Tm: the motion that carries moved back onto scan); nobody writes to them"""
    v, t = sheet(24, 16, 2.5)
    v = v.copy()
    v[:, 2] = surface(v[:, 0].astype(np.float64), v[:, 1].astype(np.float64)).astype(np.float32)
    rng = np.random.default_rng(7)
    x, y = rng.uniform(-3.0, 63.0, N_SCAN), rng.uniform(-3.0, 43.0, N_SCAN)
    z = surface(np.clip(x, 0.0, 60.0), np.clip(y, 0.0, 40.0)) + rng.uniform(-0.05, 0.05, N_SCAN)
    z[:N_RAISED] += 4.0                                                       # the first tenth: beyond max_dist, never paired
    scan = np.stack([x, y, z], axis=1)
    Tm = motion_about(MOTION["c"], MOTION["deg"], MOTION["shift"])
    R, tt = Tm[:, :3], Tm[:, 3]
    moved = ((scan - tt) @ R).astype(np.float32)                             # the inverse motion: R^T (p - t)
    return v, t, scan, moved, Tm


def part_way(share):
    return motion_about(MOTION["c"], tuple(share * d for d in MOTION["deg"]), tuple(share * s for s in MOTION["shift"]))


def clean_error(T, moved, scan):
    """the worst coordinate error of the nine clean tenths moved by T, against the scan before the motion"""
    return float(np.abs(apply(T, moved[N_RAISED:]) - scan[N_RAISED:]).max())


@functools.lru_cache(maxsize=None)
def wavy_restated():
    v, t, scan, moved, Tm = wavy_case()
    return restate_register_mesh(moved, v, t)


@functools.lru_cache(maxsize=None)
def flat_case():
    """(verts, tris, scan float32[400, 3], T0): an exactly planar sheet, 400 points 0.3 above it strictly inside, a tilted start"""
    v, t = sheet(8, 8, 4.0)
    rng = np.random.default_rng(3)
    scan = np.stack([rng.uniform(2.0, 30.0, 400), rng.uniform(2.0, 30.0, 400), np.full(400, 0.3)], axis=1).astype(np.float32)
    return v, t, scan, motion_about([16.0, 16.0, 0.0], (0.5, -0.4, 0.0), (0.0, 0.0, 0.2))


@functools.lru_cache(maxsize=None)
def flat_restated():
    v, t, scan, T0 = flat_case()
    return restate_register_mesh(scan, v, t, T0=T0)


def census(row):
    reg = row["region"]
    return int((reg == FACE).sum()), int((reg == EDGE).sum()), int((reg == VERTEX).sum())


# ---------------------------------------------------------------- CPU


def test_header_declares_and_engine_exports_mesh_registration(engine_mod, tmp_path):
    hdr = open(os.path.join(ROOT, "include", "ppp_hip.h")).read()
    for decl in ("int  ppp_get_mesh_registration_terms(ppp_handle h, ppp_trimesh m, const ppp_registration_params *rp, const double *T12,\n"
                 "                                     ppp_registration_row *row, ppp_registration_stats *stats);",
                 "int  ppp_register_mesh(ppp_handle h, ppp_trimesh m, const ppp_registration_params *rp, const double *T0_12,\n"
                 "                       ppp_registration_row *rows, size_t row_cap, ppp_registration_stats *stats);"):
        assert decl in hdr, decl
    assert "DESIGN.md 7u" in hdr and "THE QUERY IS p' ITSELF" in hdr and "n -> -n" in hdr
    for sym in ("ppp_get_mesh_registration_terms", "ppp_register_mesh"):
        assert sym in engine_mod.EXPORTS
    for m in ("mesh_registration_terms", "register_mesh"):
        assert hasattr(engine_mod.Engine, m)
    assert "register_mesh(" in open(os.path.join(ROOT, "include", "ppp_planner.hpp")).read()
    src = tmp_path / "c99.c"
    src.write_text('#include "ppp_hip.h"\nint main(void) {\n'
                   '    int (*f)(ppp_handle, ppp_trimesh, const ppp_registration_params *, const double *, ppp_registration_row *,\n'
                   '             ppp_registration_stats *) = ppp_get_mesh_registration_terms;\n'
                   '    int (*g)(ppp_handle, ppp_trimesh, const ppp_registration_params *, const double *, ppp_registration_row *, size_t,\n'
                   '             ppp_registration_stats *) = ppp_register_mesh;\n'
                   '    return f == 0 || g == 0;\n}\n')
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_restatement_recovers_a_known_motion():
    """The wavy sheet of 768 facets and a noisy scan of 1500 points that overhangs it by 3 mm on every side, the first tenth raised
    out of reach, moved by a degree and a few tenths.  Converged in at most 10 steps; the nine clean tenths come back to within
    0.1 mm: the noise is 0.05 mm and the facets' chord error covers the rest.  The GPU equals this restatement bit for bit, so
    the bound is on the restatement (the rule), not on the kernel."""
    v, t, scan, moved, Tm = wavy_case()
    T, rows, st = wavy_restated()
    before, after = clean_error(IDENTITY, moved, scan), clean_error(T, moved, scan)
    print("steps %d converged %d locked %d pairs %d -> %d rms %r -> %r; face / edge / vertex at the start %r; clean error %r -> %r mm"
          % (st["steps"], st["converged"], st["locked"], st["pairs_before"], st["pairs_after"], st["rms_before"], st["rms_after"], census(rows[0]),
             before, after))
    assert len(t) == 768 and st["n"] == st["indexed"] == N_SCAN
    assert st["converged"] == 1 and 1 <= st["steps"] <= 10
    assert st["locked"] == 0 and rows[-1]["locked"] == ALL_LOCKED and math.isnan(rows[-1]["step2"])
    assert after < 0.1 < before


def test_census_of_the_wavy_case():
    """by restatement alone: the GPU tests' input holds what they claim, at the start and at the result"""
    T, rows, st = wavy_restated()
    for k in (0, len(rows) - 1):
        row = rows[k]
        face, edge, vertex = census(row)
        unpaired = row["indexed"] - row["pairs"]
        m = row["moved"]
        not_float = int((m != m.astype(np.float32).astype(np.float64)).any(axis=1).sum())
        print("row %d: %d pairs: %d face, %d edge, %d vertex; %d unpaired; %d moved points are no floats" % (k, row["pairs"], face, edge, vertex, unpaired, not_float))
        assert face + edge + vertex == row["pairs"]
        assert edge >= 0.1 * row["pairs"] and vertex >= 1
        assert unpaired >= 0.1 * N_SCAN
        # at the identity p' is the point's float widened, exactly; behind a step the query really is a double
        assert not_float == 0 if k == 0 else not_float >= 1
    # the part-way start of the GPU tests moves the query off the floats too
    v, t, scan, moved, Tm = wavy_case()
    row = restate_mesh_terms(moved, v, t, 2.0, part_way(2.0 / 3.0))
    assert (row["moved"] != row["moved"].astype(np.float32).astype(np.float64)).any() and row["pairs"] >= 0.5 * N_SCAN


def test_a_flat_mesh_locks_what_it_cannot_see():
    """an exactly planar sheet sees neither the rotation about z nor the translations in x and y: every step's mask is 28"""
    T, rows, st = flat_restated()
    print("steps %d converged %d masks %r rms %r -> %r" % (st["steps"], st["converged"], [r["locked"] for r in rows], st["rms_before"], st["rms_after"]))
    assert st["steps"] >= 1 and all(r["locked"] == 28 for r in rows[:-1]) and st["locked"] == 28
    assert rows[-1]["locked"] == ALL_LOCKED and st["converged"] == 1
    assert all(r["pairs"] == 400 for r in rows)


def test_orientation_does_not_enter_the_words():
    """n -> -n negates J and r together: every product, and with it every word, is the same integer"""
    v, t, scan, moved, Tm = wavy_case()
    for T in (IDENTITY, part_way(2.0 / 3.0)):
        a, b = restate_mesh_terms(moved, v, t, 2.0, T), restate_mesh_terms(moved, v, t, 2.0, T, flip=True)
        assert a["pairs"] == b["pairs"] > 0 and np.array_equal(a["A"], b["A"]) and np.array_equal(a["b"], b["b"]) and a["E"] == b["E"]
        assert np.any(a["b"])


# ---------------------------------------------------------------- GPU


def scan_engine(engine_mod, pts):
    s = engine_mod.Engine(0, **KW0)
    s.set_cloud(np.ascontiguousarray(pts, np.float32))
    return s


@pytest.mark.gpu
@pytest.mark.parametrize("cell", [0.0, 0.9, 25.0])
def test_terms_match_the_restatement(engine_mod, cell):
    v, t, scan, moved, Tm = wavy_case()
    s = scan_engine(engine_mod, moved)
    mesh = s.trimesh(v, t, cell=cell)
    print("grid %r cell %r" % (mesh.stats["cells"], mesh.stats["cell"]))
    for T in (None, part_way(2.0 / 3.0)):
        want = restate_mesh_terms(s.cloud(), v, t, 2.0, IDENTITY if T is None else T)
        want.update(locked=ALL_LOCKED, step2=NAN)
        row, st = s.mesh_registration_terms(mesh, T=T)
        print("pairs %d (want %d) E %d (want %d) shift %d" % (row["pairs"], want["pairs"], row["E"], want["E"], st["shift"]))
        rows_equal([row], [want])
        assert st["shift"] == want["shift"] == 40 and same(st["centre"], want["centre"]) and same(st["length"], want["length"])
        assert st["n"] == N_SCAN and st["indexed"] == want["indexed"] and st["steps"] == 0 and st["converged"] == 0 and st["locked"] == 0
        assert st["pairs_before"] == st["pairs_after"] == row["pairs"] and same(st["rms_before"], st["rms_after"])
        assert same(st["rms_before"], rms_of(want, want["shift"])) and same(st["T"], want["T"])
        again = s.mesh_registration_terms(mesh, T=T)
        assert same(again, (row, st))                                        # the same bits in every run
    mesh.close(); s.close()


@pytest.mark.gpu
def test_chain_matches_the_restatement(engine_mod):
    v, t, scan, moved, Tm = wavy_case()
    s = scan_engine(engine_mod, moved)
    mesh = s.trimesh(v, t)
    T, rows, st = s.register_mesh(mesh)
    wT, wrows, wst = wavy_restated()
    print("steps %d (want %d) converged %d locked %d rms %r -> %r" % (st["steps"], wst["steps"], st["converged"], st["locked"], st["rms_before"], st["rms_after"]))
    assert st["steps"] == wst["steps"]
    rows_equal(rows, wrows)
    stats_equal(st, wst)
    assert same(T, wT) and rows[-1]["locked"] == ALL_LOCKED and math.isnan(rows[-1]["step2"])
    # the fit, applied, brings the clean points closer to the triangles
    clean = np.arange(N_SCAN) >= N_RAISED
    before = s.mesh_deviation(mesh)[0]
    s.transform_cloud(T)
    after = s.mesh_deviation(mesh)[0]
    worst = lambda d: float(np.nanmax(np.abs(d[clean])))
    print("largest |deviation| of the clean points %r -> %r mm" % (worst(before), worst(after)))
    assert worst(after) < worst(before)
    mesh.close(); s.close()


@pytest.mark.gpu
def test_cross_check_against_the_exact_deviation(engine_mod):
    """without the restatement: at the identity the pairs are ppp_get_mesh_deviation's matched points and E is the fixed-point sum
    of their squared deviations; a mesh oriented by viewpoint gives the same row bytes as one oriented by winding"""
    v, t, scan, moved, Tm = wavy_case()
    s = scan_engine(engine_mod, moved)
    mesh = s.trimesh(v, t)
    row, st = s.mesh_registration_terms(mesh)
    dev, _, _, _, _, status, _, ds = s.mesh_deviation(mesh, max_dist=2.0)
    matched = status == 0
    assert row["pairs"] == ds["matched"] == int(matched.sum()) > 0
    d = dev[matched]
    E = int(np.rint((d * d) * 2.0 ** st["shift"]).astype(np.int64).sum(dtype=np.int64))
    print("pairs %d E %d (from the deviation map %d)" % (row["pairs"], row["E"], E))
    assert row["E"] == E
    below = s.trimesh(v, t, orient=engine_mod.TRIMESH_VIEWPOINT, viewpoint=(30.0, 20.0, -500.0))   # every facet turned over
    flipped = s.mesh_deviation(below, max_dist=2.0)[0]
    assert same(flipped[matched], -d) and np.any(d != 0)
    for T in (None, part_way(2.0 / 3.0)):
        assert same(s.mesh_registration_terms(below, T=T), s.mesh_registration_terms(mesh, T=T))
    assert same(s.register_mesh(below), s.register_mesh(mesh))
    below.close(); mesh.close(); s.close()


@pytest.mark.gpu
def test_a_flat_mesh_on_the_gpu(engine_mod):
    v, t, scan, T0 = flat_case()
    s = scan_engine(engine_mod, scan)
    mesh = s.trimesh(v, t)
    T, rows, st = s.register_mesh(mesh, T0=T0)
    wT, wrows, wst = flat_restated()
    print("masks %r steps %d converged %d" % ([r["locked"] for r in rows], st["steps"], st["converged"]))
    assert all(r["locked"] == 28 for r in rows[:-1]) and st["locked"] == 28 and st["converged"] == 1 and st["steps"] >= 1
    rows_equal(rows, wrows)
    stats_equal(st, wst)
    mesh.close(); s.close()


def few_pairs_scan(k):
    """k clean points of the wavy case within reach of the mesh (well inside it), 20 more 50 mm above it"""
    v, t, scan, moved, Tm = wavy_case()
    inside = np.nonzero((scan[:, 0] > 5) & (scan[:, 0] < 55) & (scan[:, 1] > 5) & (scan[:, 1] < 35) & (np.arange(N_SCAN) >= N_RAISED))[0]
    far = scan[inside[40:60]] + np.array([0.0, 0.0, 50.0])
    return np.concatenate([scan[inside[:k]], far]).astype(np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [0, 5, 6])
def test_few_pairs(engine_mod, k):
    """no step below 6 pairs; with 6 the solve decides, as the restatement's does"""
    v, t = wavy_case()[:2]
    pts = few_pairs_scan(k)
    s = scan_engine(engine_mod, pts)
    mesh = s.trimesh(v, t)
    T0 = part_way(0.1)
    T, rows, st = s.register_mesh(mesh, T0=T0, iterations=3)
    wT, wrows, wst = restate_register_mesh(s.cloud(), v, t, T0=T0, iterations=3)
    print("k %d: pairs %d steps %d converged %d locked %d" % (k, rows[0]["pairs"], st["steps"], st["converged"], st["locked"]))
    assert rows[0]["pairs"] == k and st["indexed"] == k + 20
    if k < 6:
        assert st["steps"] == 0 and st["converged"] == 0 and len(rows) == 1 and same(T, T0)
        assert math.isnan(st["rms_before"]) == (k == 0)
    rows_equal(rows, wrows)
    stats_equal(st, wst)
    mesh.close(); s.close()


@pytest.mark.gpu
def test_the_ends_of_a_chain(engine_mod):
    v, t, scan, moved, Tm = wavy_case()
    s = scan_engine(engine_mod, moved)
    mesh = s.trimesh(v, t)
    wT, wrows, wst = wavy_restated()
    assert wst["steps"] >= 3
    # a chain that uses up its iterations: the last row comes from the evaluation no step follows
    T, rows, st = s.register_mesh(mesh, iterations=2)
    assert st["steps"] == 2 and st["converged"] == 0 and len(rows) == 3
    want = restate_register_mesh(s.cloud(), v, t, iterations=2)
    rows_equal(rows, want[1]); stats_equal(st, want[2]); assert same(T, want[0])
    rows_equal(rows[:2], wrows[:2])
    # row_cap below the number of rows: the first rows, the whole statistics
    T, rows, st = s.register_mesh(mesh, rows=2)
    assert len(rows) == 2
    rows_equal(rows, wrows[:2]); stats_equal(st, wst)
    T, rows, st = s.register_mesh(mesh, rows=False)
    assert rows == [] and same(T, wT)
    stats_equal(st, wst)
    # a min_step so large that the first step ends the loop
    T, rows, st = s.register_mesh(mesh, min_step=10.0)
    assert st["steps"] == 1 and st["converged"] == 1 and len(rows) == 2 and rows[1]["locked"] == ALL_LOCKED
    want = restate_register_mesh(s.cloud(), v, t, min_step=10.0)
    rows_equal(rows, want[1]); stats_equal(st, want[2])
    s.close()
    # a scan wholly outside
    s = scan_engine(engine_mod, moved + np.float32([0.0, 0.0, 50.0]))
    T, rows, st = s.register_mesh(mesh)
    assert st["steps"] == 0 and st["converged"] == 0 and st["pairs_before"] == st["pairs_after"] == 0 and len(rows) == 1
    assert math.isnan(st["rms_before"]) and math.isnan(st["rms_after"]) and same(T, IDENTITY)
    assert rows[0]["pairs"] == 0 and rows[0]["E"] == 0 and not np.any(rows[0]["A"]) and rows[0]["locked"] == ALL_LOCKED
    row, st1 = s.mesh_registration_terms(mesh)
    assert row["pairs"] == 0 and math.isnan(st1["rms_before"])
    mesh.close(); s.close()


@pytest.mark.gpu
def test_nothing_else_moved(engine_mod):
    v, t, scan, moved, Tm = wavy_case()
    s = scan_engine(engine_mod, moved)
    mesh = s.trimesh(v, t)
    r = engine_mod.Engine(0, **KW0)
    r.set_cloud_mesh(v, t, pitch=0.8)                                        # the same mesh, sampled: ppp_register's reference
    q = np.ascontiguousarray(moved[::7])
    cloud0 = s.cloud().copy()
    near0 = mesh.nearest(q, 2.0)
    sampled0 = s.register(r, max_dist=2.0, iterations=6)
    assert sampled0[2]["steps"] >= 1
    s.mesh_registration_terms(mesh, T=part_way(0.5))
    T, rows, st = s.register_mesh(mesh)
    assert st["steps"] >= 3
    assert same(s.cloud(), cloud0)
    assert same(mesh.nearest(q, 2.0), near0)
    assert same(s.register(r, max_dist=2.0, iterations=6), sampled0)         # the two chains share the handle's buffers
    assert same(s.register_mesh(mesh), (T, rows, st))
    mesh.close(); r.close(); s.close()


@pytest.mark.gpu
def test_refusals(engine_mod):
    from polishpathplanning_amd import synth
    from polishpathplanning_amd.robot_path import slice_ranges
    E = engine_mod
    v, t, scan, moved, Tm = wavy_case()
    s = scan_engine(engine_mod, moved)
    mesh = s.trimesh(v, t)
    L = s.L
    dp = ctypes.POINTER(ctypes.c_double)
    good = dict(max_dist=2.0, iterations=30, min_step=1e-6, lock_eps=1e-9)
    inf = float("inf")

    def raw(h, m, T0=None, rows=None, cap=0, params=True, **k):
        p = dict(good, **k)
        rp = E.RegistrationParams(p["max_dist"], p["iterations"], p["min_step"], p["lock_eps"])
        st, row = E.RegistrationStats(), E.RegistrationRow()
        t12 = None if T0 is None else np.ascontiguousarray(np.asarray(T0, np.float64).reshape(12))
        tp = None if t12 is None else t12.ctypes.data_as(dp)
        a = L.ppp_register_mesh(h.h, m, ctypes.byref(rp) if params else None, tp, rows, cap, ctypes.byref(st))
        b = L.ppp_get_mesh_registration_terms(h.h, m, ctypes.byref(rp) if params else None, tp, ctypes.byref(row), ctypes.byref(st))
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
    for bad in (dict(max_dist=0.0), dict(max_dist=inf), dict(max_dist=NAN), dict(lock_eps=0.0), dict(lock_eps=1.0)):
        refused(E.ERR_ARG, **bad)
    for bad in (dict(iterations=0), dict(iterations=65)):
        refused(E.ERR_ARG, loop_only=True, **bad)
    Tb = IDENTITY.copy(); Tb[1, 2] = NAN
    refused(E.ERR_ARG, T0=Tb)
    refused(E.ERR_ARG, loop_only=True, rows=None, cap=1)
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
    a, b = raw(h, mesh.m)
    assert a == b == E.ERR_UNSUPPORTED and "slice-range" in L.ppp_last_error(h.h).decode()
    assert raw(w, mesh.m) == (0, 0)                                          # the whole-cloud handle of the same cloud is served
    wT, wrows, wst = wavy_restated()
    T, rows, st = s.register_mesh(mesh)
    rows_equal(rows, wrows)
    for e in (w, h, s):
        e.close()
    mesh.close()


@pytest.mark.gpu
def test_connect_registers_against_the_triangles(engine_mod, tmp_path):
    """PPP_REGISTER=mesh PPP_DEVIATION=<reference.stl> ./connect <scan.pcd>: exit status 0, ppp_register's lines with
    ppp_register_mesh's numbers, and the deviation taken behind them"""
    from test_registration import known_clouds, relief_mm
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "examples"), "connect"])
    ref, scan, moved, Tm = known_clouds()
    mn, mx = ref.min(axis=0).astype(np.float64), ref.max(axis=0).astype(np.float64)
    x, y = np.meshgrid(np.linspace(mn[0], mx[0], 48), np.linspace(mn[1], mx[1], 28), indexing="ij")
    g = np.stack([x, y, 1500.0 + relief_mm(x, y)], axis=2).astype(np.float32)   # the nominal relief (the plates stand 1.5 m off) as 2 538 facets
    a, b, c, d = g[:-1, :-1], g[1:, :-1], g[:-1, 1:], g[1:, 1:]
    soup = np.concatenate([np.stack([a, b, c], axis=2).reshape(-1, 3, 3), np.stack([c, b, d], axis=2).reshape(-1, 3, 3)])
    stl, scan_pcd = str(tmp_path / "reference.stl"), str(tmp_path / "scan.pcd")
    engine_mod.save_stl(stl, soup)
    engine_mod.save_pcd(scan_pcd, moved, binary=True)
    conf = tmp_path / "config.txt"
    conf.write_text("Tool_Radius = 6\npathFile = %s\nPathResolution = 7\nRPYresolution = 7\nEnd effector length = 0.3\n"
                    "Smooth = false\nAlignment = false\nChangeRange = false\nRemoveOutlier = false\nDynamic_adjustment = false\n"
                    "Adjust_Threshold = 1\ntoolthickness = 10\ndepth = 0.01\n" % str(tmp_path / "wp.txt"))
    exe = os.path.join(ROOT, "examples", "connect")
    env = {k: v for k, v in os.environ.items() if not k.startswith("PPP_")}
    env.update(PPP_CONFIG=str(conf), PPP_DEVIATION=stl, PPP_REGISTER="mesh", PPP_REGISTER_MAXDIST="3", PPP_REGISTER_MINSTEP="1e-4", PPP_DEVIATION_MAXDIST="3",
               PPP_DEVIATION_EXACT="1")
    run = subprocess.run([exe, scan_pcd], env=env, capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert run.returncode == 0, run.stderr
    out = run.stdout.splitlines()
    reg = [ln for ln in out if ln.startswith("registration: ")]
    print("\n".join(reg))
    s = scan_engine(engine_mod, moved)
    mesh = s.trimesh_stl(stl)
    T, rows, st = s.register_mesh(mesh, max_dist=3.0, min_step=1e-4)
    want = ("registration: %d of %d points paired, rms %f mm; after %d steps %d paired, rms %f mm"
            % (st["pairs_before"], st["indexed"], st["rms_before"], st["steps"], st["pairs_after"], st["rms_after"]))
    how = "converged" if st["converged"] else ("out of iterations" if st["steps"] == 30 else "no step possible")
    assert st["steps"] >= 1 and st["rms_after"] < st["rms_before"]
    assert len(reg) == 5 and reg[0] == want
    assert reg[1] == "registration: %s, locked unknowns 0x%02x (rotation x y z, translation x y z from bit 0)" % (how, st["locked"])
    dev = [ln for ln in out if ln.startswith("deviation: ")]
    assert dev and " matched, " in dev[0] and out.index(dev[0]) > out.index(reg[-1])
    mesh.close(); s.close()
