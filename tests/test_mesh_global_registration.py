"""Global registration of a scan to the triangle mesh itself: area moments of the surface and K coarse mesh chains side by side
(ppp_trimesh_get_moments, ppp_mesh_frame_from_moments, ppp_register_mesh_global).

restate_mesh_moments and restate_mesh_frame below are the rule of include/ppp_hip.h in numpy float64 and Python floats: the
rotated resident corners of tests/test_trimesh.py's frames(), every written operation once, np.rint and int64 for the ten words;
the eigen part is B.74's, operation for operation as tests/test_global_registration.py's restate_frame writes it.  The coarse
table is tests/test_mesh_registration.py's restate_register_mesh per start on the scan with every point that is no query made NaN,
Python integers for the cost.  They know nothing of a grid, of a cell or of the order the device sums in.

The numbers the tests pin were taken from this restatement, never from the engine."""
import ctypes
import functools
import math
import os
import subprocess

import numpy as np
import pytest

from test_deviation import KW0, plate_mm
from test_path_dwell import same
from test_path_removal import compute_units
from test_registration import ALL_LOCKED, IDENTITY, apply, box_centre, clog2, frame, motion_about, relief_mm, relief_plate, rows_equal, stats_equal, worst_error
from test_global_registration import (CAND_FIELDS, FRAME_FIELDS, GSTATS_FIELDS, MOTION_DEG, MOTION_SHIFT, SWEEPS, cands_equal, frames_equal, pick, queries_of,
                                      restate_frame, restate_moments, restate_starts)
from test_mesh_registration import mesh_box, restate_mesh_terms, restate_register_mesh
from test_trimesh import closest_on_triangles, frames, sheet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")
ENTRIES = ("ppp_trimesh_get_moments", "ppp_mesh_frame_from_moments", "ppp_register_mesh_global")


# ---------------------------------------------------------------- the restatement


def restate_mesh_moments(rv, tris):
    """(words int64[10], ms, c float64[3], L, indexed): B.135 from the mesh's resident vertices rv float32[nv, 3] and tris (None: a
    soup), over the valid triangles in their rotated frame"""
    n_tris = len(rv) // 3 if tris is None else len(tris)
    mn, mx, (p0, p1, p2, _, _) = mesh_box(rv, tris)
    mn, mx = mn.astype(np.float64), mx.astype(np.float64)
    c = (mn + mx) * 0.5
    e = mx - mn
    L = float(((e[0] + e[1]) + e[2]) * 0.5)
    ms = min(40, 54 - clog2(max(2, n_tris)))
    scale = 2.0 ** ms
    u0, u1, u2 = ((p - c[None, :]) / L for p in (p0, p1, p2))
    e1, e2 = u1 - u0, u2 - u0
    N = [e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2], e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]]
    a = np.sqrt((N[0] * N[0] + N[1] * N[1]) + N[2] * N[2]) * 0.5
    s = (u0 + u1) + u2
    fix = lambda v: int(np.rint(v * scale).astype(np.int64).sum(dtype=np.int64))
    q = lambda d, k: ((u0[:, d] * u0[:, k] + u1[:, d] * u1[:, k]) + u2[:, d] * u2[:, k]) + s[:, d] * s[:, k]
    words = [fix(a)] + [fix(a * s[:, d]) for d in range(3)] + [fix(a * q(d, k)) for d in range(3) for k in range(d, 3)]
    return np.array(words, np.int64), ms, c, L, len(p0)


def restate_mesh_frame(words, ms, c, L, count=0):
    """the frame dict of B.136 in Python floats: m = S1 / (3 W0), C = S2 / (12 W0) - m m, then B.74's sweeps, ordering and signs"""
    W0 = float(int(words[0]))
    m = [float(int(words[1 + d])) / (3.0 * W0) for d in range(3)]
    A = [[0.0] * 3 for _ in range(3)]
    w = 4
    for d in range(3):
        for k in range(d, 3):
            A[d][k] = A[k][d] = float(int(words[w])) / (12.0 * W0) - m[d] * m[k]
            w += 1
    V = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    for _ in range(SWEEPS):
        for p, q, r in ((0, 1, 2), (0, 2, 1), (1, 2, 0)):
            apq = A[p][q]
            if apq == 0.0:
                continue
            theta = (A[q][q] - A[p][p]) / (2.0 * apq)
            at = -theta if theta < 0.0 else theta
            den = at + math.sqrt(theta * theta + 1.0)
            t = -1.0 / den if theta < 0.0 else 1.0 / den
            cs = 1.0 / math.sqrt(t * t + 1.0)
            sn = t * cs
            A[p][p] = A[p][p] - t * apq
            A[q][q] = A[q][q] + t * apq
            A[p][q] = A[q][p] = 0.0
            arp, arq = A[r][p], A[r][q]
            A[r][p] = A[p][r] = cs * arp - sn * arq
            A[r][q] = A[q][r] = sn * arp + cs * arq
            for k in range(3):
                vp, vq = V[k][p], V[k][q]
                V[k][p] = cs * vp - sn * vq
                V[k][q] = sn * vp + cs * vq
    order = sorted(range(3), key=lambda k: -A[k][k])
    ax = []
    for k in range(2):
        col = [V[d][order[k]] for d in range(3)]
        big = 0
        for d in (1, 2):
            if abs(col[d]) > abs(col[big]):
                big = d
        ax.append([-v for v in col] if col[big] < 0.0 else col)
    a, b = ax
    ax.append([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])
    return dict(count=int(count), ms=ms, c=np.array(c, np.float64), L=L, words=np.array(words, np.int64),
                mean=np.array([float(c[d]) + L * m[d] for d in range(3)]), axes=np.array([[ax[k][d] for k in range(3)] for d in range(3)]),
                eigenvalues=np.array([(A[order[d]][order[d]] * L) * L for d in range(3)]))


def mesh_frame_of(rv, tris):
    words, ms, c, L, indexed = restate_mesh_moments(rv, tris)
    return restate_mesh_frame(words, ms, c, L, indexed)


def restate_mesh_coarse(P, rv, tris, candidates, stride, coarse):
    """(frames, cands, queries, shift): the coarse stage; every candidate dict also carries its restated rows"""
    mn_s, mx_s, _ = box_centre(P)
    fs = restate_frame(*restate_moments(P, mn_s, mx_s))
    fr = mesh_frame_of(rv, tris)
    T0s = restate_starts(fs, fr, candidates)
    Pq = queries_of(P, stride)
    nq = int(np.isfinite(Pq).all(axis=1).sum())
    mn, mx, _ = mesh_box(rv, tris)
    _, _, shift, md2 = frame(mn, mx, len(P), coarse["max_dist"])
    far = int(np.rint(np.float64(md2) * 2.0 ** shift))
    cands = []
    for g in range(candidates):
        T, rows, st = restate_register_mesh(Pq, rv, tris, T0=T0s[g], **coarse)
        assert st["indexed"] == nq and st["shift"] == shift
        cost = int(rows[-1]["E"]) + (nq - rows[-1]["pairs"]) * far
        assert -2 ** 63 <= cost < 2 ** 63
        cands.append(dict(index=g, T0=T0s[g].copy(), T=T, steps=st["steps"], converged=st["converged"], locked=st["locked"],
                          pairs0=rows[0]["pairs"], pairs=rows[-1]["pairs"], E0=int(rows[0]["E"]), E=int(rows[-1]["E"]), cost=cost, rows=rows))
    return (fs, fr), cands, nq, shift


def restate_mesh_fine(P, rv, tris, frames_, cands, nq, shift, fine):
    """(T, rows, stats) as Engine.register_mesh_global gives them (cands apart), from a coarse table"""
    win, second = pick(cands)
    T, rows, st = restate_register_mesh(P, rv, tris, T0=cands[win]["T"], **fine)
    stats = dict(fine=st, scan=frames_[0], ref=frames_[1], queries=nq, shift=shift, candidates=len(cands), winner=win,
                 winner_cost=cands[win]["cost"], second_cost=second)
    return T, rows, stats


# ---------------------------------------------------------------- the cases


LATTICE = (56, 30)                                      # cells over the 141 x 78 mm plate: 2.5 x 2.6 mm, 3360 triangles
COARSE = dict(max_dist=10.0, iterations=3, min_step=1e-3, lock_eps=1e-9)       # the restated table: short chains
FINE = dict(max_dist=2.0, iterations=30, min_step=1e-6, lock_eps=1e-9)
STRIDE = 8                                              # 611 queries of 4888
# Taken from the restatement (test_census_of_the_main_case prints them): see DESIGN.md 7x.  A lattice of 6 mm (624 triangles) gave
# a ratio of 5.9 between the winner and the cheapest other basin -- the facets' chord error of 0.16 mm rms is the winner's whole
# cost, and the relief 3 sin(x / 9) cos(y / 7) nearly maps onto itself under the half turns --, so the lattice is 2.5 mm: ratio 130
MAIN_WINNER = 2
MAIN_WORST_MM = 4.9e-3                                  # the largest coordinate error of the moved-back scan behind the fine chain
CAP_MM = min(4 * MAIN_WORST_MM, 0.05)
RATIO_GUARD = 100


@functools.lru_cache(maxsize=None)
def main_case():
    """(verts float32[1767, 3], tris int32[3360, 3], unmoved scan, moved scan float32[4888, 3], the motion float64[3, 4]): the relief
    of the 141 x 78 mm plate as triangles with shared vertices, the plate's scan moved by 7l's motion about the centre of the
    mesh's box; nobody writes to them"""
    plate = relief_plate(94, 52, 31, 20.0)
    mn, mx = plate.min(axis=0).astype(np.float64), plate.max(axis=0).astype(np.float64)
    nx, ny = LATTICE
    v, t = sheet(nx, ny, 1.0)
    x = mn[0] + (mx[0] - mn[0]) * v[:, 0].astype(np.float64) / nx
    y = mn[1] + (mx[1] - mn[1]) * v[:, 1].astype(np.float64) / ny
    z0 = float(plate_mm(2, 2, "flat", 0, 20.0)[0, 2])
    verts = np.stack([x, y, z0 + relief_mm(x, y)], axis=1).astype(np.float32)
    scan = relief_plate(94, 52, 32, 20.0)
    bmn, bmx, _ = mesh_box(verts, t)
    c = (bmn.astype(np.float64) + bmx.astype(np.float64)) * 0.5
    Tm = motion_about(c, MOTION_DEG, MOTION_SHIFT)
    moved = apply(Tm, scan).astype(np.float32)
    for a in (verts, t, scan, moved, Tm):
        a.setflags(write=False)
    return verts, t, scan, moved, Tm


@functools.lru_cache(maxsize=None)
def main_restated():
    """(T, cands, rows, stats) of the main case at candidates = 4, STRIDE, COARSE and FINE, by restatement alone"""
    v, t, scan, moved, Tm = main_case()
    frames_, cands, nq, shift = restate_mesh_coarse(moved, v, t, 4, STRIDE, COARSE)
    T, rows, st = restate_mesh_fine(moved, v, t, frames_, cands, nq, shift, FINE)
    return T, cands, rows, st


@functools.lru_cache(maxsize=None)
def uneven_sheet():
    """(verts, tris): the flat sheet [0, 64] x [0, 32] at z = 5, its left half in cells of 8 mm, its right half in cells of 1 mm:
    64 times as many vertices per area on the right.  The halves do not share vertices along x = 32; both cover it."""
    a, ta = sheet(4, 4, 8.0)
    b, tb = sheet(32, 32, 1.0)
    b = b + np.float32([32.0, 0.0, 0.0])
    v = np.concatenate([a, b]).astype(np.float32)
    v[:, 2] = np.float32(5.0)
    return v, np.concatenate([ta, tb + len(a)]).astype(np.int32)


def spoiled_mesh():
    """the main mesh with degenerate and non-finite triangles interleaved: (verts, tris, the clean mesh's (verts, tris))"""
    v, t = main_case()[:2]
    bad_v = np.float32([[NAN, 0.0, 0.0], [np.inf, 1.0, 2.0]])
    verts = np.concatenate([v, bad_v]).astype(np.float32)
    nv = len(v)
    bad = np.array([[0, 0, 1], [3, nv, 5], [7, 8, nv + 1], [2, 2, 2], [-1, 4, 5], [1, 2, nv + 7]], np.int32)
    tris = np.concatenate([np.concatenate([t[k::6], bad[k:k + 1]]) for k in range(6)]).astype(np.int32)
    return verts, tris, v, t


def fine_sheet(nx, ny):
    """a wavy sheet of 2 nx ny triangles over 200 x 100 mm"""
    v, t = sheet(nx, ny, 1.0)
    x, y = 200.0 * v[:, 0].astype(np.float64) / nx, 100.0 * v[:, 1].astype(np.float64) / ny
    return np.stack([x, y, 4.0 * np.sin(x / 23.0) * np.cos(y / 17.0)], axis=1).astype(np.float32), t


# ---------------------------------------------------------------- CPU


def test_header_declares_and_engine_exports_mesh_global_registration(engine_mod, tmp_path):
    hdr = open(os.path.join(ROOT, "include", "ppp_hip.h")).read()
    for decl in ("int  ppp_trimesh_get_moments(ppp_trimesh m, ppp_cloud_frame *frame);",
                 "int  ppp_mesh_frame_from_moments(const long long *words10, int ms, const double *c3, double L, ppp_cloud_frame *frame);",
                 "int  ppp_register_mesh_global(ppp_handle h, ppp_trimesh m, const ppp_global_registration_params *gp,\n"
                 "                              ppp_registration_candidate *cands, size_t cand_cap, ppp_registration_row *rows, size_t row_cap,\n"
                 "                              ppp_global_registration_stats *stats);"):
        assert decl in hdr, decl
    assert "DESIGN.md 7x" in hdr and "ppp_cloud_frame_from_moments is not the inverse" in hdr
    assert "global start from the mesh" not in hdr
    L = engine_mod.lib()
    for sym in ENTRIES:
        assert sym in engine_mod.EXPORTS and hasattr(L, sym), sym
    assert hasattr(engine_mod.Engine, "register_mesh_global") and hasattr(engine_mod.TriMesh, "moments") and callable(engine_mod.mesh_frame_from_moments)
    assert "register_mesh_global(" in open(os.path.join(ROOT, "include", "ppp_planner.hpp")).read()
    src = tmp_path / "c99.c"
    src.write_text('#include "ppp_hip.h"\nint main(void) {\n'
                   '    int (*m)(ppp_trimesh, ppp_cloud_frame *) = ppp_trimesh_get_moments;\n'
                   '    int (*f)(const long long *, int, const double *, double, ppp_cloud_frame *) = ppp_mesh_frame_from_moments;\n'
                   '    int (*g)(ppp_handle, ppp_trimesh, const ppp_global_registration_params *, ppp_registration_candidate *, size_t,\n'
                   '             ppp_registration_row *, size_t, ppp_global_registration_stats *) = ppp_register_mesh_global;\n'
                   '    return m == 0 || f == 0 || g == 0;\n}\n')
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_examples_build_with_the_mesh_global_switch(engine_mod):
    for ex in ("connect.cpp", "robot.cpp"):
        src = open(os.path.join(ROOT, "examples", ex)).read()
        assert '"mesh-global"' in src and "register_global_to_mesh(" in src, ex
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "examples"), "connect", "connect1", "robot", "main"])


@pytest.mark.parametrize("case", ["main", "uneven", "spoiled"])
def test_mesh_frame_from_moments_matches_the_restatement(engine_mod, case):
    """ppp_mesh_frame_from_moments through the library, no device: the restatement's bits; the points' rule gives another frame"""
    v, t = dict(main=lambda: main_case()[:2], uneven=uneven_sheet, spoiled=lambda: spoiled_mesh()[:2])[case]()
    words, ms, c, L, indexed = restate_mesh_moments(v, t)
    want = restate_mesh_frame(words, ms, c, L)
    got = engine_mod.mesh_frame_from_moments(words, ms, c, L)
    print("W0 %d ms %d indexed %d mean %r eigenvalues %r" % (words[0], ms, indexed, want["mean"], want["eigenvalues"]))
    frames_equal(got, want)
    assert got["count"] == 0 and ms == min(40, 54 - clog2(len(t))) and abs(np.abs(words).max()) < 2 ** (6 + 54)
    V = got["axes"]
    assert np.abs(V.T @ V - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(V) - 1.0) < 1e-12
    assert not same(engine_mod.cloud_frame_from_moments(words, ms, c, L)["mean"], got["mean"])
    for bad in (dict(words=[0] * 10), dict(words=[-5] + [1] * 9), dict(L=0.0), dict(L=NAN), dict(ms=63), dict(ms=-1)):
        a = dict(words=words, ms=ms, L=L); a.update(bad)
        with pytest.raises(engine_mod.PPPError) as ex:
            engine_mod.mesh_frame_from_moments(a["words"], a["ms"], c, a["L"])
        assert ex.value.code == engine_mod.ERR_ARG


def test_the_ordinary_frame_call_returns_the_bits_it_returned(engine_mod):
    """the eigen part is written once now: ppp_cloud_frame_from_moments against restate_frame on the scan, and the area rule on a
    mesh whose moments are known in closed form -- the unit square's centre and its second moments 1/12"""
    moved = main_case()[3]
    mn, mx, _ = box_centre(moved)
    words, ms, c, L = restate_moments(moved, mn, mx)
    frames_equal(engine_mod.cloud_frame_from_moments(words, ms, c, L), restate_frame(words, ms, c, L))
    v, t = sheet(1, 1, 1.0)
    f = mesh_frame_of(v, t)
    assert np.abs(f["mean"] - [0.5, 0.5, 0.0]).max() < 1e-12 and np.abs(f["eigenvalues"] - [1 / 12, 1 / 12, 0.0]).max() < 1e-12


def test_the_mean_on_an_unevenly_meshed_sheet():
    """one half in cells 8 times finer than the other: the area frame's mean is the sheet's centre, the vertex mean is far off.
    The bound: every word is off by at most half a unit per triangle, so |S1_d| is off by <= T / 2 and W0 by <= T / 2 units of
    2^-ms; m_d = S1_d / (3 W0) with |m_d| <= 1 moves by at most (T / 2 + T / 2) / (3 W0) (to first order, doubled for the
    roundings of the terms themselves in double, which are far below one unit), and the mean by L times that."""
    v, t = uneven_sheet()
    words, ms, c, L, indexed = restate_mesh_moments(v, t)
    f = restate_mesh_frame(words, ms, c, L, indexed)
    T = indexed
    bound = 2.0 * L * (T / 2 + T / 2) / (3.0 * float(words[0]))
    centre = np.array([32.0, 16.0, 5.0])
    off = np.abs(f["mean"] - centre).max()
    vertex_mean = v.astype(np.float64).mean(axis=0)
    print("triangles %d W0 %d bound %.3g mm; area mean off by %.3g mm; vertex mean %r" % (T, words[0], bound, off, vertex_mean))
    assert indexed == len(t) == 2 * 16 + 2 * 1024 and bound < 1e-6
    assert off <= bound
    assert abs(vertex_mean[0] - centre[0]) > 0.1 * 64.0


def test_census_of_the_main_case():
    """by restatement alone: the input of the GPU parity tests is what they claim (figures in DESIGN.md 7x)"""
    v, t, scan, moved, Tm = main_case()
    T, cands, rows, st = main_restated()
    win = st["winner"]
    errs = [worst_error(c["T"], moved, scan) for c in cands]
    for c, e in zip(cands, errs):
        print("start %2d steps %d converged %d locked %2d pairs %4d -> %4d cost %.4g error %.4g mm"
              % (c["index"], c["steps"], c["converged"], c["locked"], c["pairs0"], c["pairs"], c["cost"], e))
    wrong = [c["cost"] for c, e in zip(cands, errs) if e > 1.0]
    err = worst_error(T, moved, scan)
    print("triangles %d queries %d shift %d winner %d cost %d second %d lowest cost in another basin %d ratio %.4g; fine steps %d converged %d rms %r "
          "largest error %r mm" % (len(t), st["queries"], st["shift"], win, st["winner_cost"], st["second_cost"], min(wrong),
                                   min(wrong) / max(st["winner_cost"], 1), st["fine"]["steps"], st["fine"]["converged"], st["fine"]["rms_after"], err))
    assert len(t) == 3360 and len(v) == 1767 and len(moved) == 4888 and st["queries"] == 611 and st["shift"] >= 24
    assert win == MAIN_WINNER and errs[win] <= 1.0 and len(wrong) >= 1
    assert min(wrong) >= RATIO_GUARD * st["winner_cost"]
    assert st["fine"]["converged"] == 1 and err <= CAP_MM
    assert MAIN_WORST_MM / 1.5 <= err <= MAIN_WORST_MM                     # the pinned figure is this one, rounded up
    # ppp_register_mesh from the identity does not find the motion: that is what the global start is for
    Ti, rows_i, st_i = restate_register_mesh(moved, v, t, **FINE)
    lost = worst_error(Ti, moved, scan)
    print("from the identity: steps %d pairs %d largest error %r mm" % (st_i["steps"], st_i["pairs_after"], lost))
    assert lost > 1.0
    # ... and not for want of reach.  At 2 mm, and at the coarse stage's 10 mm, the moved scan has no pair at all and the chain
    # takes no step; at 80 mm it pairs 466 of the coarse stage's 611 queries and iterates -- 8 steps here, and 30 without
    # converging when it is let -- and stays 190 mm off: another basin
    Tw, rows_w, st_w = restate_register_mesh(queries_of(moved, STRIDE), v, t, **dict(FINE, max_dist=80.0, iterations=8))
    lost_wide = worst_error(Tw, moved, scan)
    print("from the identity at 80 mm: steps %d pairs %d -> %d largest error %r mm" % (st_w["steps"], st_w["pairs_before"], st_w["pairs_after"], lost_wide))
    assert st_w["steps"] == 8 and st_w["pairs_before"] >= 400 and lost_wide > 1.0


# ---------------------------------------------------------------- GPU


def scan_engine(engine_mod, pts):
    s = engine_mod.Engine(0, **KW0)
    s.set_cloud(np.ascontiguousarray(pts, np.float32))
    return s


def moments_parity(engine_mod, mesh, v, t):
    words, ms, c, L, indexed = restate_mesh_moments(v, t)
    want = restate_mesh_frame(words, ms, c, L, indexed)
    got = mesh.moments()
    print("indexed %d W0 %d (want %d) ms %d" % (got["count"], got["words"][0], words[0], got["ms"]))
    frames_equal(got, want)
    again = mesh.moments()
    frames_equal(again, got)
    host = engine_mod.mesh_frame_from_moments(got["words"], got["ms"], got["c"], got["L"])
    assert host["count"] == 0
    frames_equal(dict(host, count=got["count"]), got)
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["main", "uneven", "spoiled"])
def test_moments_match_the_restatement(engine_mod, case):
    e = engine_mod.Engine(0, **KW0)
    if case == "spoiled":
        v, t, cv, ct = spoiled_mesh()
        mesh = e.trimesh(v, t)
        assert mesh.stats["degenerate"] == 6 and mesh.stats["indexed"] == len(ct)
        got = moments_parity(engine_mod, mesh, v, t)
        clean = e.trimesh(cv, ct)
        want = clean.moments()
        # the spoiled triangles add nothing: the clean mesh's words; ms is the same here (3366 and 3360 triangles: clog2 = 12)
        assert same(got["words"], want["words"]) and got["count"] == want["count"] == len(ct) and got["ms"] == want["ms"]
        clean.close()
    else:
        v, t = main_case()[:2] if case == "main" else uneven_sheet()
        mesh = e.trimesh(v, t)
        got = moments_parity(engine_mod, mesh, v, t)
        # the caller's triangle order permuted, and another cell: the same words
        perm = np.random.default_rng(5).permutation(len(t))
        other = e.trimesh(v, t[perm], cell=3.7)
        frames_equal(other.moments(), got)
        other.close()
    mesh.close(); e.close()


@pytest.mark.gpu
def test_moments_grid_stride_loop(engine_mod):
    """more records than 2 * CUs * 256: every workgroup of k_mesh_moments strides over the records more than once"""
    cus = compute_units()
    nx = 300
    ny = max(240, (2 * cus * 256) // (2 * nx) + 8)
    v, t = fine_sheet(nx, ny)
    print("triangles %d, threads of the capped grid %d" % (len(t), 2 * cus * 256))
    assert len(t) > 2 * cus * 256
    e = engine_mod.Engine(0, **KW0)
    mesh = e.trimesh(v, t)
    assert mesh.stats["indexed"] == len(t)
    moments_parity(engine_mod, mesh, v, t)
    mesh.close(); e.close()


def global_parity(got, want):
    T, cands, rows, st = got
    wT, wcands, wrows, wst = want
    cands_equal(cands, [{k: c[k] for k in CAND_FIELDS} for c in wcands])
    rows_equal(rows, wrows)
    assert tuple(st) == GSTATS_FIELDS
    stats_equal(st["fine"], wst["fine"])
    frames_equal(st["scan"], wst["scan"]); frames_equal(st["ref"], wst["ref"])
    for f in GSTATS_FIELDS[3:]:
        assert st[f] == wst[f], (f, st[f], wst[f])
    assert same(T, wT) and same(T, rows[-1]["T"]) and rows[-1]["locked"] == ALL_LOCKED


@pytest.mark.gpu
@pytest.mark.parametrize("cell", [0.0, 17.0])
def test_coarse_table_and_fine_rows_match_the_restatement(engine_mod, cell):
    v, t, scan, moved, Tm = main_case()
    s = scan_engine(engine_mod, moved)
    assert same(s.cloud(), moved)                                            # resident units are the inputs' floats (KW0)
    mesh = s.trimesh(v, t, cell=cell)
    got = s.register_mesh_global(mesh, candidates=4, stride=STRIDE, coarse=COARSE, fine=FINE)
    st = got[3]
    print("grid %r: winner %d cost %d second %d queries %d shift %d fine steps %d" % (mesh.stats["cells"], st["winner"], st["winner_cost"], st["second_cost"],
                                                                                     st["queries"], st["shift"], st["fine"]["steps"]))
    global_parity(got, main_restated())
    assert st["winner"] == MAIN_WINNER and st["queries"] == 611 and len(got[1]) == 4
    mesh.close(); s.close()


def chains_are_register_mesh(s, mesh, got, coarse, fine):
    """stride 1: every coarse chain is Engine.register_mesh with `coarse` from its start, the fine rows are register_mesh with
    `fine` from the winner's end, on the same handle"""
    T, cands, rows, st = got
    assert st["queries"] == st["fine"]["indexed"]
    for c in cands:
        Tk, rk, sk = s.register_mesh(mesh, T0=c["T0"], **coarse)
        assert same(c["T"], Tk), c["index"]
        assert (c["steps"], c["converged"], c["locked"]) == (sk["steps"], sk["converged"], sk["locked"]), c["index"]
        assert (c["pairs0"], c["E0"], c["pairs"], c["E"]) == (rk[0]["pairs"], rk[0]["E"], rk[-1]["pairs"], rk[-1]["E"]), c["index"]
        assert st["shift"] == sk["shift"]
    win, second = pick(cands)
    assert (st["winner"], st["second_cost"], st["winner_cost"]) == (win, second, cands[win]["cost"])
    Tf, rf, sf = s.register_mesh(mesh, T0=cands[win]["T"], **fine)
    rows_equal(rows, rf)
    stats_equal(st["fine"], sf)
    assert same(T, Tf)


COARSE24 = dict(max_dist=10.0, iterations=6, min_step=1e-3, lock_eps=1e-9)


@pytest.mark.gpu
def test_twenty_four_starts_at_stride_one(engine_mod):
    v, t, scan, moved, Tm = main_case()
    s = scan_engine(engine_mod, moved)
    mesh = s.trimesh(v, t)
    got = s.register_mesh_global(mesh, candidates=24, stride=1, coarse=COARSE24, fine=FINE)
    cands = got[1]
    assert len(cands) == 24 and got[3]["queries"] == len(moved)
    chains_are_register_mesh(s, mesh, got, COARSE24, FINE)
    steps = sorted({c["steps"] for c in cands})
    early = [c["index"] for c in cands if c["steps"] < COARSE24["iterations"] and c["converged"] == 0]
    print("steps that occur: %r; ended early without converging: %r; pairs at the end %r" % (steps, early, [c["pairs"] for c in cands]))
    assert len(steps) >= 2 and early                                         # (two starts end at once, on an evaluation without a pair)
    assert all(cands[k]["pairs"] < 6 for k in early) and any(cands[k]["pairs"] == 0 for k in early)
    assert worst_error(got[0], moved, scan) <= CAP_MM
    # a start-poor variant: 49 points of the scan within 0.25 mm -- the wrong starts cross the mesh along a line and find fewer
    # than 6 pairs there, so their chains end on their first evaluation while the right one goes on
    few = scan_engine(engine_mod, moved[::100])
    poor = dict(COARSE24, max_dist=0.25)
    got = few.register_mesh_global(mesh, candidates=24, stride=1, coarse=poor, fine=FINE)
    chains_are_register_mesh(few, mesh, got, poor, FINE)
    ended = [c["index"] for c in got[1] if c["steps"] == 0 and c["converged"] == 0 and c["pairs"] < 6]
    print("start-poor variant: steps %r; ended on the first evaluation with fewer than 6 pairs: %r" % ([c["steps"] for c in got[1]], ended))
    assert ended and len({c["steps"] for c in got[1]}) >= 2
    few.close(); mesh.close(); s.close()


@pytest.mark.gpu
def test_the_stride_loop_of_the_summing_kernel(engine_mod):
    """more queries per start than 256 x its workgroup cap with 24 starts, so every workgroup of k_mesh_reg_sum_multi strides over
    the queries more than once; the identities of stride 1"""
    from test_global_registration import dense_relief
    v, t, _, _, Tm = main_case()
    per = max(1, 2 * compute_units() // 24)
    n = 256 * per + 2500
    side = int(math.ceil(math.sqrt(n / 2.0)))
    scan = apply(Tm, dense_relief(2 * side, side, 7)).astype(np.float32)
    print("queries %d, workgroups per start %d (%d threads)" % (len(scan), per, 256 * per))
    assert len(scan) > 256 * per
    s = scan_engine(engine_mod, scan)
    mesh = s.trimesh(v, t)
    coarse, fine = dict(COARSE24, iterations=2), dict(FINE, iterations=2)
    got = s.register_mesh_global(mesh, candidates=24, stride=1, coarse=coarse, fine=fine)
    assert max(c["pairs"] for c in got[1]) > 256 * per
    chains_are_register_mesh(s, mesh, got, coarse, fine)
    mesh.close(); s.close()


@pytest.mark.gpu
def test_end_to_end_and_repeatable(engine_mod):
    """the defaults but stride 4: the moved-back scan is within the census's cap, where ppp_register_mesh from the identity is
    lost; two runs on fresh handles give equal bytes"""
    v, t, scan, moved, Tm = main_case()
    out = []
    for _ in range(2):
        s = scan_engine(engine_mod, moved)
        mesh = s.trimesh(v, t)
        out.append(s.register_mesh_global(mesh, stride=4))
        if len(out) == 2:
            Ti = s.register_mesh(mesh)[0]
            Tw, _, sw = s.register_mesh(mesh, max_dist=80.0)                 # within reach of the facets: it iterates, elsewhere
        mesh.close(); s.close()
    T, cands, rows, st = out[0]
    err, lost = worst_error(T, moved, scan), worst_error(Ti, moved, scan)
    print("winner %d of %d, queries %d, fine steps %d converged %d: largest error %r mm (cap %r); from the identity %r mm"
          % (st["winner"], st["candidates"], st["queries"], st["fine"]["steps"], st["fine"]["converged"], err, CAP_MM, lost))
    assert st["candidates"] == 24 and st["queries"] == 1222 and st["fine"]["converged"] == 1
    print("from the identity at 80 mm: steps %d pairs %d -> %d, %r mm" % (sw["steps"], sw["pairs_before"], sw["pairs_after"], worst_error(Tw, moved, scan)))
    assert err <= CAP_MM and lost > 1.0 and sw["steps"] >= 8 and worst_error(Tw, moved, scan) > 1.0
    assert same(out[0], out[1])


@pytest.mark.gpu
def test_nothing_else_moved(engine_mod):
    from test_deviation import engines
    v, t, scan, moved, Tm = main_case()
    r, s = engines(engine_mod, relief_plate(94, 52, 31, 20.0), moved)
    mesh = s.trimesh(v, t)
    field = s.contact_field()                                                # a stored result of the handle, and its index with it
    cloud0, box0 = s.cloud().copy(), s.minmax()
    kw = dict(candidates=4, stride=4, coarse=COARSE24, fine=FINE)
    before = (s.register_global(r, **kw), s.register_mesh(mesh, T0=main_restated()[0]), s.mesh_deviation(mesh, max_dist=2.0), mesh.moments())
    got = s.register_mesh_global(mesh, **kw)
    assert got[3]["winner"] == MAIN_WINNER
    after = (s.register_global(r, **kw), s.register_mesh(mesh, T0=main_restated()[0]), s.mesh_deviation(mesh, max_dist=2.0), mesh.moments())
    assert same(before, after)
    assert same(s.cloud(), cloud0) and same(s.minmax(), box0) and same(s.contact_field(), field)
    assert same(s.register_mesh_global(mesh, **kw), got)
    # a handle with a plan and a pass behind it (the plate as scanned, lying along x): the plan and the list stay what they were,
    # and a second pass gives the same list
    p = engine_mod.Engine(0, tool_radius=6.0, walk=1, **KW0)
    p.set_cloud(scan)
    S, W = p.gen_path(), p.get_path()
    plan0, list0 = p.slice_positions().copy(), p.waypoints().copy()
    assert S >= 2 and W >= 2
    Tp = p.register_mesh_global(mesh, **kw)[0]
    assert worst_error(Tp, scan, scan) <= CAP_MM                             # (already in place: the identity's basin)
    assert p.num_slices() == S and p.num_waypoints() == W and same(p.slice_positions(), plan0) and same(p.waypoints(), list0)
    assert (p.gen_path(), p.get_path()) == (S, W) and same(p.slice_positions(), plan0) and same(p.waypoints(), list0)
    mesh.close(); r.close(); s.close(); p.close()


@pytest.mark.gpu
def test_refusals(engine_mod):
    from polishpathplanning_amd import synth
    from polishpathplanning_amd.robot_path import slice_ranges
    E = engine_mod
    v, t, scan, moved, Tm = main_case()
    s = scan_engine(engine_mod, moved)
    mesh = s.trimesh(v, t)
    good = dict(candidates=4, stride=STRIDE, coarse=COARSE, fine=FINE)

    def refused(h, m, code, **k):
        kw = dict(good); kw.update(k)
        with pytest.raises(E.PPPError) as ex:
            h.register_mesh_global(m, **kw)
        assert ex.value.code == code and str(ex.value), (k, ex.value)       # its code and a message
        assert s.register_mesh_global(mesh, **good)[3]["winner"] == MAIN_WINNER    # and the handle still works

    inf = float("inf")
    for c in (0, 3, 5, 12, 25, -24):
        refused(s, mesh, E.ERR_ARG, candidates=c)
    for st_ in (0, -1):
        refused(s, mesh, E.ERR_ARG, stride=st_)
    for stage in ("coarse", "fine"):
        base = COARSE if stage == "coarse" else FINE
        for bad in (dict(max_dist=0.0), dict(max_dist=NAN), dict(max_dist=inf), dict(max_dist=1e9), dict(iterations=0), dict(iterations=65),
                    dict(min_step=-1.0), dict(min_step=NAN), dict(lock_eps=0.0), dict(lock_eps=1.0)):
            refused(s, mesh, E.ERR_ARG, **{stage: dict(base, **bad)})
    gp = E.GlobalRegistrationParams()
    s.L.ppp_default_global_registration_params(ctypes.byref(gp))
    raw = E.GlobalRegistrationStats()
    call = s.L.ppp_register_mesh_global
    for args in ((s.h, None, ctypes.byref(gp), None, 0, None, 0), (s.h, mesh.m, None, None, 0, None, 0), (s.h, mesh.m, ctypes.byref(gp), None, 2, None, 0),
                 (s.h, mesh.m, ctypes.byref(gp), None, 0, None, 2)):
        assert call(*args, ctypes.byref(raw)) == E.ERR_ARG and s.L.ppp_last_error(s.h).decode()
    assert s.L.ppp_trimesh_get_moments(mesh.m, None) == E.ERR_ARG and s.L.ppp_trimesh_get_moments(None, ctypes.byref(E.CloudFrame())) == E.ERR_ARG
    empty = E.Engine(0, **KW0)                                               # no cloud on the handle
    refused(empty, mesh, E.ERR_ARG)
    empty.close()
    one = E.Engine(0, **KW0)                                                 # L == 0 on the scan: every point the same
    one.set_cloud(np.tile(np.float32([[5.0, 1.0, 2.0]]), (70, 1)))
    refused(one, mesh, E.ERR_ARG)
    one.close()
    gap = moved.copy()                                                       # no query left: every multiple of 7 is not finite
    gap[::7, 0] = np.float32(NAN)
    g = E.Engine(0, **KW0)
    g.set_cloud(gap)
    refused(g, mesh, E.ERR_ARG, stride=7)
    g.close()
    # W0 <= 0: two triangles 1.7 km apart, each a few float steps across: their areas over L^2 round to nothing at 2^-40
    step = np.float32(np.spacing(np.float32(1000.0)))
    far = np.float32(1000.0)
    dust = np.float32([[0, 0, 0], [1e-7, 0, 0], [0, 1e-7, 0], [far, far, far], [far + step, far, far], [far, far + step, far]])
    speck = s.trimesh(dust)
    assert speck.stats["indexed"] == 2
    with pytest.raises(E.PPPError) as ex:
        speck.moments()
    assert ex.value.code == E.ERR_ARG
    refused(s, speck, E.ERR_ARG)
    speck.close()
    pts, cfg = synth.make_config("tiny_5k")
    w = E.Engine(0, tool_radius=cfg["tool_radius"], walk=1)
    w.set_cloud(pts)
    S = w.gen_path()
    lo, hi = slice_ranges(S, 2)[1]
    h = E.Engine(0, tool_radius=cfg["tool_radius"], walk=1, slice_begin=lo, slice_end=hi)
    h.set_cloud(pts)
    with pytest.raises(E.PPPError) as ex:
        h.register_mesh_global(mesh, **good)
    assert ex.value.code == E.ERR_UNSUPPORTED and "slice-range" in str(ex.value)
    w.register_mesh_global(mesh, **good)                                     # the whole-cloud handle of the same cloud is served
    from test_trimmed_registration import part_handle
    part = part_handle(engine_mod, w, pts, cfg)                              # a handle that holds a part of the cloud (ppp_set_cloud_part)
    with pytest.raises(E.PPPError) as ex:
        part.register_mesh_global(mesh, **good)
    assert ex.value.code == E.ERR_UNSUPPORTED and "part" in str(ex.value) and s.L.ppp_last_error(part.h).decode()
    n_part = len(part.cloud())
    with pytest.raises(E.PPPError):                                          # the same refusal again: the handle took no harm
        part.register_mesh_global(mesh, **good)
    assert len(part.cloud()) == n_part and n_part > 0
    w.register_mesh_global(mesh, **good)
    assert s.register_mesh_global(mesh, **good)[3]["winner"] == MAIN_WINNER
    part.close()
    for e in (w, h, s):
        e.close()
    mesh.close()


@pytest.mark.gpu
def test_a_mesh_on_another_device_is_refused(engine_mod):
    from test_deviation_tiles import device_count
    if device_count() < 2:
        pytest.skip("needs two GPUs in one process: this machine shows %d" % device_count())
    v, t, scan, moved, Tm = main_case()
    s = scan_engine(engine_mod, moved)
    other = engine_mod.Engine(1, **KW0)
    far = other.trimesh(v, t)
    with pytest.raises(engine_mod.PPPError) as ex:
        s.register_mesh_global(far, candidates=4, stride=STRIDE, coarse=COARSE, fine=FINE)
    assert ex.value.code == engine_mod.ERR_ARG and "another device" in str(ex.value)
    near = s.trimesh(v, t)
    assert s.register_mesh_global(near, candidates=4, stride=STRIDE, coarse=COARSE, fine=FINE)[3]["winner"] == MAIN_WINNER
    frames_equal(far.moments(), near.moments())                              # the mesh's own call runs where the mesh lives
    near.close(); far.close(); other.close(); s.close()


@pytest.mark.gpu
def test_connect_registers_globally_against_the_triangles(engine_mod, tmp_path):
    """PPP_REGISTER=mesh-global PPP_DEVIATION=<part.stl> ./connect <scan.pcd>: exit status 0, the winner's line, and a result
    within the cap"""
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "examples"), "connect"])
    v, t, scan, moved, Tm = main_case()
    stl, scan_pcd = str(tmp_path / "part.stl"), str(tmp_path / "scan.pcd")
    engine_mod.save_stl(stl, v[t].reshape(-1, 3, 3))
    engine_mod.save_pcd(scan_pcd, moved, binary=True)
    conf = tmp_path / "config.txt"
    conf.write_text("Tool_Radius = 6\npathFile = %s\nPathResolution = 7\nRPYresolution = 7\nEnd effector length = 0.3\n"
                    "Smooth = false\nAlignment = false\nChangeRange = false\nRemoveOutlier = false\nDynamic_adjustment = false\n"
                    "Adjust_Threshold = 1\ntoolthickness = 10\ndepth = 0.01\n" % str(tmp_path / "wp.txt"))
    exe = os.path.join(ROOT, "examples", "connect")
    env = {k: v_ for k, v_ in os.environ.items() if not k.startswith("PPP_")}
    env.update(PPP_CONFIG=str(conf), PPP_DEVIATION=stl, PPP_REGISTER="mesh-global", PPP_REGISTER_STRIDE="4", PPP_DEVIATION_MAXDIST="3", PPP_DEVIATION_EXACT="1")
    run = subprocess.run([exe, scan_pcd], env=env, capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert run.returncode == 0, run.stderr
    out = run.stdout.splitlines()
    glob = [ln for ln in out if ln.startswith("global registration: ")]
    reg = [ln for ln in out if ln.startswith("registration: ")]
    print("\n".join(glob + reg))
    s = scan_engine(engine_mod, moved)
    mesh = s.trimesh_stl(stl)
    T, cands, rows, st = s.register_mesh_global(mesh, stride=4)
    assert len(glob) == 2 and glob[0].startswith("global registration: %d starts on %d queries; " % (st["candidates"], st["queries"]))
    assert glob[1] == "global registration: start %d wins at cost %d, the next other pose at %d" % (st["winner"], st["winner_cost"], st["second_cost"])
    fs = st["fine"]
    assert len(reg) == 5 and reg[0] == ("registration: %d of %d points paired, rms %f mm; after %d steps %d paired, rms %f mm"
                                        % (fs["pairs_before"], fs["indexed"], fs["rms_before"], fs["steps"], fs["pairs_after"], fs["rms_after"]))
    assert reg[1].startswith("registration: converged")
    got = np.array([[float(x) for x in ln.split()[2:6]] for ln in reg[2:]])
    assert np.abs(got - T).max() < 1e-5 * max(1.0, np.abs(T).max())         # (printed with six decimals)
    assert worst_error(T, moved, scan) <= CAP_MM
    dev = [ln for ln in out if ln.startswith("deviation: ")]
    assert dev and " matched, " in dev[0] and out.index(dev[0]) > out.index(reg[-1])
    mesh.close(); s.close()
