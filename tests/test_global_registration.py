"""Global registration: principal-frame starts and K coarse chains side by side (ppp_get_cloud_moments,
ppp_cloud_frame_from_moments, ppp_registration_starts, ppp_register_global).

restate_moments, restate_frame, restate_starts and restate_global below are the definitions in numpy and plain Python floats:
np.rint and int64 for the ten words, Python floats (one rounding per written operation, math.sqrt) for the Jacobi sweeps and the
starts, test_registration's restate_register per start on the scan with every point that is no query made NaN (so n stays the
whole cloud's and the queries are the indexed points), Python integers for the cost.  Everything the engine returns is expected
bit for bit.  The CPU inputs come from the oracle (estimate_normals() of the reference), the GPU inputs from the engine's own
getters.

The numbers the tests pin were taken from this restatement with the oracle's normals, never from the engine."""
import ctypes
import functools
import math
import os
import subprocess

import numpy as np
import pytest

from test_deviation import KW0, engines, plate_mm
from test_path_dwell import same
from test_path_removal import compute_units
from test_registration import (ALL_LOCKED, IDENTITY, apply, box_centre, clog2, frame, motion_about, oracle_normals, relief_mm, relief_plate,
                               restate_register, rows_equal, stats_equal, worst_error)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")
ENTRIES = ("ppp_get_cloud_moments", "ppp_cloud_frame_from_moments", "ppp_registration_starts", "ppp_default_global_registration_params",
           "ppp_register_global")
FRAME_FIELDS = ("count", "ms", "c", "L", "words", "mean", "axes", "eigenvalues")
GPARAMS_FIELDS = ("candidates", "stride", "coarse", "fine")
CAND_FIELDS = ("index", "T0", "T", "steps", "converged", "locked", "pairs0", "pairs", "E0", "E", "cost")
GSTATS_FIELDS = ("fine", "scan", "ref", "queries", "shift", "candidates", "winner", "winner_cost", "second_cost")
SWEEPS = 12


# ---------------------------------------------------------------- the restatement


def restate_moments(P, mn, mx):
    """(words int64[10], ms, c float64[3], L): B.73 from the cloud P float32[n, 3] and its ppp_minmax"""
    P = np.ascontiguousarray(P, np.float32)
    mn = np.asarray(mn, np.float32).astype(np.float64); mx = np.asarray(mx, np.float32).astype(np.float64)
    c = (mn + mx) * 0.5
    e = mx - mn
    L = float(((e[0] + e[1]) + e[2]) * 0.5)
    ms = min(40, 60 - clog2(max(2, len(P))))
    scale = 2.0 ** ms
    p = P[np.isfinite(P).all(axis=1)].astype(np.float64)
    u = (p - c[None, :]) / L
    fix = lambda v: int(np.rint(v * scale).astype(np.int64).sum(dtype=np.int64))
    words = [len(p)] + [fix(u[:, d]) for d in range(3)] + [fix(u[:, d] * u[:, k]) for d in range(3) for k in range(d, 3)]
    return np.array(words, np.int64), ms, c, L


def restate_frame(words, ms, c, L):
    """the frame dict of B.74 in Python floats, operation for operation"""
    cnt = float(int(words[0]))
    inv = 1.0
    for _ in range(ms):
        inv = inv * 0.5
    m = [(float(int(words[1 + d])) / cnt) * inv for d in range(3)]
    A = [[0.0] * 3 for _ in range(3)]
    w = 4
    for d in range(3):
        for k in range(d, 3):
            A[d][k] = A[k][d] = (float(int(words[w])) / cnt) * inv - m[d] * m[k]
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
    order = sorted(range(3), key=lambda k: -A[k][k])                        # stable: a tie keeps the lower original column first
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
    return dict(count=int(words[0]), ms=ms, c=np.array(c, np.float64), L=L, words=np.array(words, np.int64),
                mean=np.array([float(c[d]) + L * m[d] for d in range(3)]), axes=np.array([[ax[k][d] for k in range(3)] for d in range(3)]),
                eigenvalues=np.array([(A[order[d]][order[d]] * L) * L for d in range(3)]))


PERMS = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))
PARITY = (1, -1, -1, 1, 1, -1)


def start_table():
    """the 24 (perm, sgn) of B.75 in the header's order"""
    out = [((0, 1, 2), s) for s in ((1, 1, 1), (1, -1, -1), (-1, 1, -1), (-1, -1, 1))]
    for perm, par in zip(PERMS[1:], PARITY[1:]):
        for s in ((a, b, c) for a in (1, -1) for b in (1, -1) for c in (1, -1)):
            if par * s[0] * s[1] * s[2] == 1:
                out.append((perm, s))
    assert len(out) == 24 and len(set(out)) == 24
    return out


def restate_starts(fs, fr, candidates):
    Vs, Vr = fs["axes"].tolist(), fr["axes"].tolist()
    ms_, mr = fs["mean"].tolist(), fr["mean"].tolist()
    out = np.zeros((candidates, 3, 4))
    for g, (perm, sgn) in enumerate(start_table()[:candidates]):
        for r in range(3):
            a = [-Vr[r][perm[k]] if sgn[k] < 0 else Vr[r][perm[k]] for k in range(3)]
            row = [((a[0] * Vs[cc][0]) + a[1] * Vs[cc][1]) + a[2] * Vs[cc][2] for cc in range(3)]
            out[g, r, :3] = row
            out[g, r, 3] = mr[r] - (((row[0] * ms_[0]) + row[1] * ms_[1]) + row[2] * ms_[2])
    return out


def queries_of(P, stride):
    """the scan with every point that is no query of the coarse stage made NaN: n unchanged, the queries indexed"""
    Q = np.array(P, np.float32)
    Q[np.arange(len(Q)) % stride != 0] = np.float32(np.nan)
    return Q


def pick(cands):
    """(winner, second cost or -1) by B.76's rule"""
    win = min(range(len(cands)), key=lambda k: (cands[k]["cost"], k))
    others = [c["cost"] for c in cands if c["T"].tobytes() != cands[win]["T"].tobytes()]
    return win, (min(others) if others else -1)


def restate_coarse(P, Q, normals, mn_s, mx_s, mn_r, mx_r, candidates, stride, coarse):
    """(frames, cands, queries, shift): the coarse stage; every candidate dict also carries its restated rows"""
    fs = restate_frame(*restate_moments(P, mn_s, mx_s))
    fr = restate_frame(*restate_moments(Q, mn_r, mx_r))
    T0s = restate_starts(fs, fr, candidates)
    Pq = queries_of(P, stride)
    nq = int(np.isfinite(Pq).all(axis=1).sum())
    _, _, shift, md2 = frame(mn_r, mx_r, len(P), coarse["max_dist"])
    far = int(np.rint(np.float64(md2) * 2.0 ** shift))
    cands = []
    for g in range(candidates):
        T, rows, st = restate_register(Pq, Q, normals, mn_r, mx_r, T0=T0s[g], **coarse)
        assert st["indexed"] == nq and st["shift"] == shift
        cost = int(rows[-1]["E"]) + (nq - rows[-1]["pairs"]) * far
        assert -2 ** 63 <= cost < 2 ** 63
        cands.append(dict(index=g, T0=T0s[g].copy(), T=T, steps=st["steps"], converged=st["converged"], locked=st["locked"],
                          pairs0=rows[0]["pairs"], pairs=rows[-1]["pairs"], E0=int(rows[0]["E"]), E=int(rows[-1]["E"]), cost=cost, rows=rows))
    return (fs, fr), cands, nq, shift


def restate_fine(P, Q, normals, mn_r, mx_r, frames, cands, nq, shift, fine):
    """(T, rows, stats) as Engine.register_global gives them (cands apart), from a coarse table"""
    win, second = pick(cands)
    T, rows, st = restate_register(P, Q, normals, mn_r, mx_r, T0=cands[win]["T"], **fine)
    stats = dict(fine=st, scan=frames[0], ref=frames[1], queries=nq, shift=shift, candidates=len(cands), winner=win,
                 winner_cost=cands[win]["cost"], second_cost=second)
    return T, rows, stats


# ---------------------------------------------------------------- clouds


MOTION_DEG, MOTION_SHIFT = (130.0, 25.0, -160.0), (40.0, -25.0, 60.0)
COARSE = dict(max_dist=10.0, iterations=6, min_step=1e-3, lock_eps=1e-9)
FINE = dict(max_dist=2.0, iterations=30, min_step=1e-6, lock_eps=1e-9)
STRIDE = 4
LATTICE_MM = 1.5                                        # synth's lattice step
# Taken from the restatement with the oracle's normals (test_census_of_the_main_case prints them): see DESIGN.md §7l
MAIN_WINNER = 2                                         # the half turn about the second axis
MAIN_WORST_MM = 5.5e-4                                  # the largest coordinate error of the moved-back scan behind the fine chain
CAP_MM = min(4 * MAIN_WORST_MM, 0.05)
RATIO_GUARD = 100


@functools.lru_cache(maxsize=None)
def main_case():
    """(reference, unmoved scan, moved scan float32, the motion float64[3, 4]); nobody writes to them"""
    ref = relief_plate(94, 52, 31, 20.0)
    scan = relief_plate(94, 52, 32, 20.0)
    _, _, c = box_centre(ref)
    Tm = motion_about(c, MOTION_DEG, MOTION_SHIFT)
    moved = apply(Tm, scan).astype(np.float32)
    for a in (ref, scan, moved, Tm):
        a.setflags(write=False)
    return ref, scan, moved, Tm


@functools.lru_cache(maxsize=None)
def main_coarse_cpu():
    ref, scan, moved, _ = main_case()
    mn_r, mx_r, _ = box_centre(ref)
    mn_s, mx_s, _ = box_centre(moved)
    return restate_coarse(moved, ref, oracle_normals(ref), mn_s, mx_s, mn_r, mx_r, 24, STRIDE, COARSE)


def square_plate():
    """a flat square lattice, symmetric under x <-> y: two equal eigenvalues, exactly"""
    g = np.arange(-8, 9, dtype=np.float32) * np.float32(2.0)
    x, y = np.meshgrid(g, g, indexing="ij")
    return np.stack([x.ravel(), y.ravel(), np.full(x.size, 3.0, np.float32)], axis=1).astype(np.float32)


def line_of_points():
    t = np.arange(40, dtype=np.float32)
    return np.stack([t * np.float32(0.5), t * np.float32(-0.25) + np.float32(3.0), t * np.float32(0.125)], axis=1).astype(np.float32)


def frames_equal(got, want):
    assert tuple(got) == FRAME_FIELDS
    for f in FRAME_FIELDS:
        assert same(got[f], want[f]), (f, got[f], want[f])


def cands_equal(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert tuple(g) == CAND_FIELDS
        for f in CAND_FIELDS:
            assert same(g[f], w[f]), (w["index"], f, g[f], w[f])


def gstats_equal(got, want):
    assert tuple(got) == GSTATS_FIELDS
    stats_equal(got["fine"], want["fine"])
    frames_equal(got["scan"], want["scan"]); frames_equal(got["ref"], want["ref"])
    for f in GSTATS_FIELDS[3:]:
        assert got[f] == want[f], (f, got[f], want[f])


# ---------------------------------------------------------------- CPU


def test_header_declares_and_engine_exports_global_registration(engine_mod):
    hdr = open(os.path.join(ROOT, "include", "ppp_hip.h")).read()
    for decl in ("int  ppp_get_cloud_moments(ppp_handle h, ppp_cloud_frame *frame);",
                 "int  ppp_cloud_frame_from_moments(const long long *words10, int ms, const double *c3, double L, ppp_cloud_frame *frame);",
                 "int  ppp_registration_starts(const ppp_cloud_frame *scan, const ppp_cloud_frame *ref, int candidates, double *T12s);",
                 "void ppp_default_global_registration_params(ppp_global_registration_params *gp);",
                 "int  ppp_register_global(ppp_handle h, ppp_handle ref, const ppp_global_registration_params *gp,",
                 "} ppp_cloud_frame;", "} ppp_global_registration_params;", "} ppp_registration_candidate;", "} ppp_global_registration_stats;"):
        assert decl in hdr, decl
    assert "DESIGN.md 7l" in hdr and "a guess for parts of a few hundred millimetres" in hdr
    L = engine_mod.lib()
    for sym in ENTRIES:
        assert sym in engine_mod.EXPORTS and hasattr(L, sym), sym
    for m in ("cloud_moments", "register_global"):
        assert hasattr(engine_mod.Engine, m)
    for f in ("cloud_frame_from_moments", "registration_starts"):
        assert callable(getattr(engine_mod, f))


def test_header_is_c99_clean_with_global_registration(tmp_path):
    src = tmp_path / "c99.c"
    src.write_text('#include "ppp_hip.h"\nint main(void) {\n'
                   '    int (*m)(ppp_handle, ppp_cloud_frame *) = ppp_get_cloud_moments;\n'
                   '    int (*f)(const long long *, int, const double *, double, ppp_cloud_frame *) = ppp_cloud_frame_from_moments;\n'
                   '    int (*s)(const ppp_cloud_frame *, const ppp_cloud_frame *, int, double *) = ppp_registration_starts;\n'
                   '    void (*d)(ppp_global_registration_params *) = ppp_default_global_registration_params;\n'
                   '    int (*g)(ppp_handle, ppp_handle, const ppp_global_registration_params *, ppp_registration_candidate *, size_t,\n'
                   '             ppp_registration_row *, size_t, ppp_global_registration_stats *) = ppp_register_global;\n'
                   '    ppp_global_registration_stats st;\n    ppp_registration_candidate c;\n'
                   '    st.scan.words[9] = 0; st.ref.axes[8] = 0.0; st.fine.shift = 40; c.T0[11] = 0.0; c.cost = 0;\n'
                   '    return m == 0 || f == 0 || s == 0 || d == 0 || g == 0 || st.fine.shift != 40 || c.cost != 0;\n}\n')
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_global_registration_structs_layout_matches_the_header(engine_mod, tmp_path):
    src = tmp_path / "layout.c"
    structs = (("ppp_cloud_frame", FRAME_FIELDS, engine_mod.CloudFrame),
               ("ppp_global_registration_params", GPARAMS_FIELDS, engine_mod.GlobalRegistrationParams),
               ("ppp_registration_candidate", CAND_FIELDS, engine_mod.RegistrationCandidate),
               ("ppp_global_registration_stats", GSTATS_FIELDS, engine_mod.GlobalRegistrationStats))
    args, want = [], []
    for name, fields, T in structs:
        args += ["sizeof(%s)" % name] + ["offsetof(%s, %s)" % (name, f) for f in fields]
        want += [ctypes.sizeof(T)] + [getattr(T, f).offset for f in fields]
        assert tuple(f for f, _ in T._fields_) == fields
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ppp_hip.h"\nint main(void) {\n'
                   '    printf("' + " ".join(["%zu"] * len(args)) + '\\n", ' + ", ".join(args) + ');\n    return 0;\n}\n')
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)])
    assert [int(v) for v in subprocess.check_output([exe]).split()] == want
    gp = engine_mod.GlobalRegistrationParams()
    engine_mod.lib().ppp_default_global_registration_params(ctypes.byref(gp))
    assert (gp.candidates, gp.stride) == (24, 16)
    assert (gp.coarse.max_dist, gp.coarse.iterations, gp.coarse.min_step, gp.coarse.lock_eps) == (10.0, 8, 1e-3, 1e-9)
    assert (gp.fine.max_dist, gp.fine.iterations, gp.fine.min_step, gp.fine.lock_eps) == (2.0, 30, 1e-6, 1e-9)


def host_cases():
    ref, _, moved, _ = main_case()
    return dict(relief=moved, reference=ref, square=square_plate(), line=line_of_points())


@pytest.mark.parametrize("case", ["relief", "reference", "square", "line"])
def test_frame_from_moments_matches_the_restatement(engine_mod, case):
    """ppp_cloud_frame_from_moments through the library, no device: the restatement's bits"""
    P = host_cases()[case]
    mn, mx, _ = box_centre(P)
    words, ms, c, L = restate_moments(P, mn, mx)
    want = restate_frame(words, ms, c, L)
    got = engine_mod.cloud_frame_from_moments(words, ms, c, L)
    print("eigenvalues %r mean %r\naxes\n%r" % (want["eigenvalues"], want["mean"], want["axes"]))
    frames_equal(got, want)
    V = got["axes"]
    assert np.abs(V.T @ V - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(V) - 1.0) < 1e-12
    ev = got["eigenvalues"]
    assert ev[0] >= ev[1] >= ev[2]
    if case == "square":
        assert ev[0] == ev[1] > 0 and ev[2] == 0 and same(V, np.eye(3))      # the tie keeps the lower original column first
    if case == "line":
        assert ev[0] > 0 and abs(ev[1]) < 1e-9 * ev[0] and abs(ev[2]) < 1e-9 * ev[0]
    for bad in (dict(words=[0] * 10), dict(L=0.0), dict(L=NAN), dict(ms=63)):
        a = dict(words=words, ms=ms, L=L); a.update(bad)
        with pytest.raises(engine_mod.PPPError) as ex:
            engine_mod.cloud_frame_from_moments(a["words"], a["ms"], c, a["L"])
        assert ex.value.code == engine_mod.ERR_ARG


def test_starts_match_the_restatement_and_are_proper_rotations(engine_mod):
    cases = host_cases()
    frames = {k: restate_frame(*restate_moments(P, *box_centre(P)[:2])) for k, P in cases.items()}
    for a, b in (("relief", "reference"), ("square", "reference"), ("line", "square"), ("reference", "reference")):
        want = restate_starts(frames[a], frames[b], 24)
        got = engine_mod.registration_starts(frames[a], frames[b], 24)
        assert same(got, want), (a, b)
        four = engine_mod.registration_starts(frames[a], frames[b], 4)
        assert same(four, got[:4]) and same(four, restate_starts(frames[a], frames[b], 4))
        for T in got:
            R = T[:, :3]
            assert np.abs(R.T @ R - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(R) - 1.0) < 1e-12
            assert np.abs(R @ frames[a]["mean"] + T[:, 3] - frames[b]["mean"]).max() < 1e-9
        assert len({np.round(T[:, :3], 6).tobytes() for T in got}) == 24       # 24 different rotations
    for bad in (0, 3, 5, 23, 25, -4):
        with pytest.raises(engine_mod.PPPError) as ex:
            engine_mod.registration_starts(frames["relief"], frames["reference"], bad)
        assert ex.value.code == engine_mod.ERR_ARG


def test_census_of_the_main_case():
    """by restatement alone, with the oracle's normals: the input of the GPU parity tests is what they claim (figures in
    DESIGN.md §7l)"""
    ref, scan, moved, Tm = main_case()
    frames, cands, nq, shift = main_coarse_cpu()
    mn_r, mx_r, _ = box_centre(ref)
    T, rows, st = restate_fine(moved, ref, oracle_normals(ref), mn_r, mx_r, frames, cands, nq, shift, FINE)
    win = st["winner"]
    errs = [worst_error(c["T"], moved, scan) for c in cands]
    for c, e in zip(cands, errs):
        print("start %2d steps %d converged %d locked %2d pairs %4d -> %4d cost %.4g error %.4g mm"
              % (c["index"], c["steps"], c["converged"], c["locked"], c["pairs0"], c["pairs"], c["cost"], e))
    wrong = [c["cost"] for c, e in zip(cands, errs) if e > 1.0]
    err = worst_error(T, moved, scan)
    print("queries %d shift %d winner %d cost %d second %d lowest cost in another basin %d ratio %.4g; fine steps %d rms %r largest error %r mm"
          % (nq, shift, win, st["winner_cost"], st["second_cost"], min(wrong), min(wrong) / max(st["winner_cost"], 1), st["fine"]["steps"],
             st["fine"]["rms_after"], err))
    assert len(moved) == 4888 and nq == 1222 and shift >= 24                 # the shift floor is 16: room to spare
    assert win == MAIN_WINNER and errs[win] <= 1.0 and len(wrong) >= 1
    assert min(wrong) >= RATIO_GUARD * st["winner_cost"]
    assert cands[win]["pairs"] == nq
    ended_early = [c for c in cands if c["steps"] < COARSE["iterations"] and c["converged"] == 0]
    used_up = [c for c in cands if c["steps"] == COARSE["iterations"]]
    print("ended early without converging: %r; used up their iterations: %r" % ([c["index"] for c in ended_early], [c["index"] for c in used_up]))
    assert st["fine"]["converged"] == 1 and err <= CAP_MM
    # stride 4 by cloud index does not empty a region: the subsample's box is within one lattice step of the whole scan's, taken
    # on the unmoved scan (the same cloud indices), where the box's sides run along the lattice
    q = scan[::STRIDE]
    gap = max(np.abs(q.min(axis=0) - scan.min(axis=0)).max(), np.abs(q.max(axis=0) - scan.max(axis=0)).max())
    print("the subsample's box against the scan's: %r mm" % gap)
    assert gap <= LATTICE_MM


def test_examples_build_with_the_global_switch(engine_mod):
    for ex in ("connect.cpp", "robot.cpp"):
        src = open(os.path.join(ROOT, "examples", ex)).read()
        assert '"global"' in src and "register_global_to(" in src, ex
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "examples"), "connect", "connect1", "robot", "main"])
    for exe in ("connect", "connect1", "robot", "main"):
        assert os.access(os.path.join(ROOT, "examples", exe), os.X_OK)


# ---------------------------------------------------------------- GPU


def restated_from(s, r, candidates, stride, coarse, fine=None):
    """(T, cands, rows, stats) by restatement from the engine's own getters"""
    mn_r, mx_r = r.minmax()
    mn_s, mx_s = s.minmax()
    P, Q, N = s.cloud(), r.cloud(), r.estimate_normals()
    frames, cands, nq, shift = restate_coarse(P, Q, N, mn_s, mx_s, mn_r, mx_r, candidates, stride, coarse)
    if fine is None:
        return frames, cands, nq, shift
    T, rows, st = restate_fine(P, Q, N, mn_r, mx_r, frames, cands, nq, shift, fine)
    return T, cands, rows, st


def global_parity(got, want):
    T, cands, rows, st = got
    wT, wcands, wrows, wst = want
    cands_equal(cands, [{k: c[k] for k in CAND_FIELDS} for c in wcands])
    rows_equal(rows, wrows)
    gstats_equal(st, wst)
    assert same(T, wT) and same(T, rows[-1]["T"]) and rows[-1]["locked"] == ALL_LOCKED


@pytest.mark.gpu
@pytest.mark.parametrize("fast", [True, False])
def test_moments_match_the_restatement(engine_mod, fast):
    """4888 + 3 points, no multiple of 64, one of them not finite; the window path and the slab path give the same bits"""
    ref, _, moved, _ = main_case()
    P = np.concatenate([moved, moved[:3] + np.float32(0.25)]).astype(np.float32)
    P[17, 1] = np.float32("inf")
    assert len(P) % 64
    s = engine_mod.Engine(0, tool_radius=6.0, walk=1, fast_path=fast, **KW0)
    s.set_cloud(P)
    got = s.cloud_moments()
    assert s.fast_path() == fast
    mn, mx = s.minmax()
    words, ms, c, L = restate_moments(s.cloud(), mn, mx)
    assert words[0] == len(P) - 1 and ms == 40
    frames_equal(got, restate_frame(words, ms, c, L))
    frames_equal(s.cloud_moments(), got)
    s.close()


@functools.lru_cache(maxsize=None)
def main_gpu_run(engine_mod):
    """the main case at stride 4 with 24 and with 4 candidates, and its restatement from the engine's getters, once"""
    ref, _, moved, _ = main_case()
    r, s = engines(engine_mod, ref, moved)
    got24 = s.register_global(r, candidates=24, stride=STRIDE, coarse=COARSE, fine=FINE)
    got4 = s.register_global(r, candidates=4, stride=STRIDE, coarse=COARSE, fine=FINE)
    frames, cands, nq, shift = restated_from(s, r, 24, STRIDE, COARSE)
    mn_r, mx_r = r.minmax()
    args = (s.cloud(), r.cloud(), r.estimate_normals(), mn_r, mx_r, frames)
    want24 = restate_fine(*args, cands, nq, shift, FINE)
    want4 = restate_fine(*args, cands[:4], nq, shift, FINE)
    r.close(); s.close()
    return got24, got4, (want24[0], cands, want24[1], want24[2]), (want4[0], cands[:4], want4[1], want4[2])


@pytest.mark.gpu
@pytest.mark.parametrize("candidates", [24, 4])
def test_coarse_table_and_fine_rows_match_the_restatement(engine_mod, candidates):
    got24, got4, want24, want4 = main_gpu_run(engine_mod)
    got, want = (got24, want24) if candidates == 24 else (got4, want4)
    st = got[3]
    print("winner %d cost %d second %d queries %d shift %d fine steps %d" % (st["winner"], st["winner_cost"], st["second_cost"], st["queries"],
                                                                          st["shift"], st["fine"]["steps"]))
    global_parity(got, want)
    assert st["winner"] == MAIN_WINNER and st["queries"] == 1222 and len(got[1]) == candidates


@pytest.mark.gpu
def test_chains_end_at_different_times(engine_mod):
    """in the main case's table some starts end early without converging while others use up their iterations; parity is
    test_coarse_table_and_fine_rows_match_the_restatement's"""
    got24, _, want24, _ = main_gpu_run(engine_mod)
    cands = want24[1]
    early = [c["index"] for c in cands if c["steps"] < COARSE["iterations"] and c["converged"] == 0]
    used = [c["index"] for c in cands if c["steps"] == COARSE["iterations"]]
    print("ended early: %r, used up: %r" % (early, used))
    assert early and used
    for c in cands:
        if c["index"] in early:
            assert c["pairs"] < 6 or c["rows"][-1]["locked"] == ALL_LOCKED
    cands_equal(got24[1], [{k: c[k] for k in CAND_FIELDS} for c in cands])


@pytest.mark.gpu
def test_stride_one_chains_are_ppp_register(engine_mod):
    """stride 1, 4 candidates: every coarse chain equals Engine.register from that start on the same handles"""
    ref, _, moved, _ = main_case()
    r, s = engines(engine_mod, ref, moved)
    T, cands, rows, st = s.register_global(r, candidates=4, stride=1, coarse=COARSE, fine=FINE)
    assert st["queries"] == len(moved) and len(cands) == 4
    for c in cands:
        Tk, rk, sk = s.register(r, T0=c["T0"], **COARSE)
        assert same(c["T"], Tk) and (c["steps"], c["converged"], c["locked"]) == (sk["steps"], sk["converged"], sk["locked"])
        assert (c["pairs0"], c["E0"], c["pairs"], c["E"]) == (rk[0]["pairs"], rk[0]["E"], rk[-1]["pairs"], rk[-1]["E"])
        assert st["shift"] == sk["shift"]
    r.close(); s.close()


def dense_relief(nx, ny, seed):
    """the relief surface over the reference's box, on a jittered lattice of nx x ny points in a random order"""
    rng = np.random.Generator(np.random.PCG64(seed))
    ref = main_case()[0]
    mn, mx = ref.min(axis=0).astype(np.float64), ref.max(axis=0).astype(np.float64)
    hx, hy = (mx[0] - mn[0]) / (nx - 1), (mx[1] - mn[1]) / (ny - 1)
    x = mn[0] + hx * (np.arange(nx)[:, None] + rng.uniform(-0.3, 0.3, (nx, ny)))
    y = mn[1] + hy * (np.arange(ny)[None, :] + rng.uniform(-0.3, 0.3, (nx, ny)))
    z = float(plate_mm(2, 2, "flat", 0, 20.0)[0, 2]) + relief_mm(x, y)
    pts = np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1)
    return pts[rng.permutation(len(pts))].astype(np.float32)


@pytest.mark.gpu
def test_the_grid_stride_loop_of_the_multi_kernel(engine_mod):
    """a scan of 36 450 points at stride 1 with 4 candidates and 1 iteration: more queries per start than 256 x its workgroup
    cap, so every workgroup of k_reg_terms_multi strides over the queries more than once; the table against the restatement"""
    ref, _, _, Tm = main_case()
    scan = apply(Tm, dense_relief(270, 135, 7)).astype(np.float32)
    coarse = dict(COARSE, iterations=1)
    r, s = engines(engine_mod, ref, scan)
    per = max(1, 2 * compute_units() // 4)
    print("queries %d, workgroups per start %d (%d threads)" % (len(scan), per, 256 * per))
    assert len(scan) > 256 * per
    T, cands, rows, st = s.register_global(r, candidates=4, stride=1, coarse=coarse, fine=dict(FINE, iterations=1))
    frames, wcands, nq, shift = restated_from(s, r, 4, 1, coarse)
    assert nq == len(scan) == st["queries"] and st["shift"] == shift
    cands_equal(cands, [{k: c[k] for k in CAND_FIELDS} for c in wcands])
    assert st["winner"] == pick(wcands)[0] and max(c["pairs"] for c in cands) > 256 * per
    r.close(); s.close()


@pytest.mark.gpu
def test_global_registration_end_to_end(engine_mod):
    """from the moved scan alone: register_global, transform_cloud, and the deviation map matches what the unmoved scan's does"""
    ref, scan, moved, Tm = main_case()
    got24 = main_gpu_run(engine_mod)[0]
    T = got24[0]
    err = worst_error(T, moved, scan)
    print("largest error %r mm (cap %r)" % (err, CAP_MM))
    assert got24[3]["fine"]["converged"] == 1 and err <= CAP_MM
    r, s = engines(engine_mod, ref, moved)
    u = engine_mod.Engine(0, **KW0)
    u.set_cloud(scan)
    want = u.deviation(r, max_dist=2.0, maps=False)[5]
    s.transform_cloud(s.register_global(r, candidates=24, stride=STRIDE, coarse=COARSE, fine=FINE)[0])
    got = s.deviation(r, max_dist=2.0, maps=False)[5]
    print("matched %d of %d (unmoved scan: %d), rms_dev %r (unmoved %r)" % (got["matched"], got["n"], want["matched"], got["rms_dev"], want["rms_dev"]))
    assert got["matched"] == want["matched"] == len(scan) - want["no_normal"] and got["no_normal"] == want["no_normal"] and got["too_far"] == 0
    for e in (r, s, u):
        e.close()


@pytest.mark.gpu
def test_global_registration_refusals_and_a_cloud_against_itself(engine_mod):
    from polishpathplanning_amd import synth
    from polishpathplanning_amd.robot_path import slice_ranges
    ref, _, moved, _ = main_case()
    r, s = engines(engine_mod, ref, moved)
    # h == ref: the winner maps the cloud onto itself, at the identity start's cost
    T, cands, rows, st = r.register_global(r, candidates=24, stride=STRIDE, coarse=COARSE, fine=FINE)
    assert st["winner_cost"] == cands[0]["cost"] and worst_error(T, ref, ref) <= CAP_MM
    assert np.abs(cands[0]["T0"] - IDENTITY).max() < 1e-9
    # stored results stay byte-identical over a call
    field = s.contact_field()
    dev = s.deviation(r, max_dist=2.0)
    before = s.cloud().copy(), r.cloud().copy()
    s.register_global(r, candidates=4, stride=STRIDE, coarse=COARSE, fine=FINE)
    assert same(s.contact_field(), field) and same(s.deviation(r, max_dist=2.0), dev)
    assert same(s.cloud(), before[0]) and same(r.cloud(), before[1])

    def refused(h, other, code, **k):
        kw = dict(candidates=4, stride=STRIDE, coarse=COARSE, fine=FINE); kw.update(k)
        with pytest.raises(engine_mod.PPPError) as ex:
            h.register_global(other, **kw)
        assert ex.value.code == code, (k, ex.value)

    inf = float("inf")
    for c in (0, 3, 5, 12, 25, -24):
        refused(s, r, engine_mod.ERR_ARG, candidates=c)
    for st_ in (0, -1):
        refused(s, r, engine_mod.ERR_ARG, stride=st_)
    for stage in ("coarse", "fine"):
        base = COARSE if stage == "coarse" else FINE
        for bad in (dict(max_dist=0.0), dict(max_dist=NAN), dict(max_dist=inf), dict(max_dist=1e9), dict(iterations=0), dict(iterations=65),
                    dict(min_step=-1.0), dict(min_step=NAN), dict(lock_eps=0.0), dict(lock_eps=1.0)):
            refused(s, r, engine_mod.ERR_ARG, **{stage: dict(base, **bad)})
    gp = engine_mod.GlobalRegistrationParams()
    s.L.ppp_default_global_registration_params(ctypes.byref(gp))
    raw = engine_mod.GlobalRegistrationStats()
    assert s.L.ppp_register_global(s.h, None, ctypes.byref(gp), None, 0, None, 0, ctypes.byref(raw)) == engine_mod.ERR_ARG
    assert s.L.ppp_register_global(s.h, r.h, None, None, 0, None, 0, ctypes.byref(raw)) == engine_mod.ERR_ARG
    assert s.L.ppp_register_global(s.h, r.h, ctypes.byref(gp), None, 2, None, 0, ctypes.byref(raw)) == engine_mod.ERR_ARG
    assert s.L.ppp_register_global(s.h, r.h, ctypes.byref(gp), None, 0, None, 2, ctypes.byref(raw)) == engine_mod.ERR_ARG
    assert s.L.ppp_get_cloud_moments(s.h, None) == engine_mod.ERR_ARG
    empty = engine_mod.Engine(0, **KW0)                                      # no cloud on either handle
    refused(s, empty, engine_mod.ERR_ARG)
    refused(empty, r, engine_mod.ERR_ARG)
    with pytest.raises(engine_mod.PPPError) as ex:
        empty.cloud_moments()
    assert ex.value.code == engine_mod.ERR_ARG
    empty.close()
    one = engine_mod.Engine(0, **KW0)                                        # L == 0: every point the same
    one.set_cloud(np.tile(np.float32([[5.0, 1.0, 2.0]]), (70, 1)))
    with pytest.raises(engine_mod.PPPError) as ex:
        one.cloud_moments()
    assert ex.value.code == engine_mod.ERR_ARG
    refused(one, r, engine_mod.ERR_ARG)
    refused(s, one, engine_mod.ERR_ARG)
    one.close()
    gap = moved.copy()                                                       # no query left: every multiple of 7 is not finite
    gap[::7, 0] = np.float32(NAN)
    g = engine_mod.Engine(0, **KW0)
    g.set_cloud(gap)
    refused(g, r, engine_mod.ERR_ARG, stride=7)
    g.close()
    pts, cfg = synth.make_config("tiny_5k")
    w = engine_mod.Engine(0, tool_radius=cfg["tool_radius"], walk=1)
    w.set_cloud(pts)
    S = w.gen_path()
    lo, hi = slice_ranges(S, 2)[1]
    h = engine_mod.Engine(0, tool_radius=cfg["tool_radius"], walk=1, slice_begin=lo, slice_end=hi)
    h.set_cloud(pts)
    refused(h, w, engine_mod.ERR_UNSUPPORTED)
    refused(w, h, engine_mod.ERR_UNSUPPORTED)
    with pytest.raises(engine_mod.PPPError) as ex:
        h.cloud_moments()
    assert ex.value.code == engine_mod.ERR_UNSUPPORTED
    # every refusal leaves a later good call working
    T, cands, rows, st = s.register_global(r, candidates=4, stride=STRIDE, coarse=COARSE, fine=FINE)
    assert st["winner"] == MAIN_WINNER and st["fine"]["converged"] == 1
    for e in (r, s, w, h):
        e.close()


@pytest.mark.gpu
def test_global_registration_is_repeatable(engine_mod):
    """two runs on fresh handles: byte-identical tables, rows and stats; and equal to the shared run"""
    ref, _, moved, _ = main_case()
    out = []
    for _ in range(2):
        r, s = engines(engine_mod, ref, moved)
        out.append(s.register_global(r, candidates=24, stride=STRIDE, coarse=COARSE, fine=FINE))
        r.close(); s.close()
    assert same(out[0], out[1])
