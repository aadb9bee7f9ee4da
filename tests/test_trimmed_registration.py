"""Trimmed registration: ICP that keeps the share `keep` of an evaluation's pairs with the smallest pair distance
(ppp_register_trimmed).

The restatement is test_registration's plus the cut: restate_terms pairs the scan (brute force, float32 d2, the first minimum),
the pairs' float d2 -- dist2_flann's order on the float query, as d2_table writes it -- are read as uint32 keys, k =
ceil(keep * paired) clamped to [1, paired], tau the k-th smallest key, and restate_terms runs once more on the scan in which
every point that is not KEPT is NaN (a pair does not depend on the other points; n, and with it the fixed point, is the
cloud's).  restate_step takes the step.  Integer sums and a rank statistic have no order, so every word of the engine is
expected bit for bit.  CPU inputs: the oracle's normals; GPU inputs: the engine's own getters.

Digit split of the engine's selection: key bits 31..21, 20..10, 9..0 (TOP, MID, LOW below); the digit cases straddle those."""
import ctypes
import functools
import math
import os
import subprocess

import numpy as np
import pytest

import test_registration as tr
from test_deviation import engines, large_clouds, main_clouds, past_the_grid_cap
from test_path_dwell import same
from test_registration import (ALL_LOCKED, CENSUS, IDENTITY, KNOWN, LARGE, MOTION_DEG, MOTION_SHIFT, NAN, apply, box_centre, census_T0,
                               few_pairs_scan, known_clouds, large_T0, motion_about, oracle_normals, relief_plate, restate_register,
                               restate_step, restate_terms, rms_of)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEPT, TRIMMED, UNPAIRED, DROPPED = 0, 1, 2, 3
NAN32_BITS = 0x7FC00000
TOP, MID = 21, 10                                        # key >> TOP: the top digit; (key >> MID) & 0x7ff: the middle; key & 0x3ff: the low

TPARAMS_DECL = ("typedef struct {\n"
                "    ppp_registration_params icp;   /* ppp_register's four, with its ranges */\n"
                "    double keep;                   /* in (0, 1]: the share of an evaluation's pairs that enter its sums */\n"
                "} ppp_trimmed_registration_params;          /* defaults: ppp_default_registration_params, 0.8 */")
TROW_DECL = ("typedef struct {\n"
             "    ppp_registration_row row;      /* as ppp_register's, but pairs / A / b / E are over the KEPT pairs */\n"
             "    size_t paired;                 /* pairs found by the search at row.T (what ppp_register would sum) */\n"
             "    float  trim_d2;                /* the cut: the largest float d2 that is kept; NaN when paired == 0 */\n"
             "} ppp_trimmed_registration_row;")
TENUM_DECL = "enum { PPP_TRIM_KEPT = 0, PPP_TRIM_TRIMMED = 1, PPP_TRIM_UNPAIRED = 2, PPP_TRIM_DROPPED = 3 };"
TFUNC_DECLS = ("void ppp_default_trimmed_registration_params(ppp_trimmed_registration_params *tp);",
               "int  ppp_register_trimmed(ppp_handle h, ppp_handle ref, const ppp_trimmed_registration_params *tp, const double *T0_12,\n"
               "                          ppp_trimmed_registration_row *rows, size_t row_cap,\n"
               "                          unsigned char *status, float *d2, size_t cap,\n"
               "                          ppp_registration_stats *stats);")


# ---------------------------------------------------------------- the restatement


def trim_rank(keep, paired):
    """k of B.78: one double product, one ceil, clamped to [1, paired]; 0 without a pair"""
    if not paired:
        return 0
    return min(paired, max(1, int(math.ceil(float(keep) * float(paired)))))


def pair_d2(P, Q, T, partner):
    """float32 d2 of every pair (partner >= 0), by cloud index of the scan, NaN elsewhere: the float query against the float
    reference point in dist2_flann's order"""
    P = np.ascontiguousarray(P, np.float32); Q = np.ascontiguousarray(Q, np.float32)
    T = np.asarray(T, np.float64).reshape(3, 4)
    at = np.nonzero(partner >= 0)[0]
    p = P[at].astype(np.float64)
    m = np.stack([((T[r, 0] * p[:, 0] + T[r, 1] * p[:, 1]) + T[r, 2] * p[:, 2]) + T[r, 3] for r in range(3)], axis=1)
    q32 = m.astype(np.float32)
    B = Q[partner[at]]
    dx = q32[:, 0] - B[:, 0]
    d = dx * dx
    dy = q32[:, 1] - B[:, 1]
    d = d + dy * dy
    dz = q32[:, 2] - B[:, 2]
    d = d + dz * dz
    assert d.dtype == np.float32
    out = np.full(len(P), np.nan, np.float32)
    out[at] = d
    return out


def restate_trimmed_terms(P, Q, normals, mn, mx, max_dist, T, keep):
    """restate_terms's dict over the KEPT pairs (pairs = kept) with paired, k, trim_bits (tau; the float quiet NaN without a
    pair), status uint8[n] and d2 float32[n] by cloud index of the scan"""
    P = np.ascontiguousarray(P, np.float32)
    full = restate_terms(P, Q, normals, mn, mx, max_dist, T)
    d2 = pair_d2(P, Q, T, full["partner"])
    paired = full["pairs"]
    pair = full["partner"] >= 0
    assert int(pair.sum()) == paired and not np.isnan(d2[pair]).any() and not np.signbit(d2[pair]).any()
    keys = d2.view(np.uint32)
    k = trim_rank(keep, paired)
    status = np.full(len(P), UNPAIRED, np.uint8)
    status[~np.isfinite(P).all(axis=1)] = DROPPED
    if paired:
        tau = int(np.sort(keys[pair])[k - 1])
        kept = pair & (keys <= np.uint32(tau))
        status[pair] = TRIMMED
        status[kept] = KEPT
    else:
        tau, kept = NAN32_BITS, pair
    cut = P.copy()
    cut[~kept] = np.float32(np.nan)                                         # what is not kept is not indexed: no pair, no term
    row = restate_terms(cut, Q, normals, mn, mx, max_dist, T)
    assert row["pairs"] == int(kept.sum()) >= k and row["shift"] == full["shift"] and np.array_equal(row["partner"][kept], full["partner"][kept])
    row.update(n=full["n"], indexed=full["indexed"], paired=paired, k=k, trim_bits=tau, status=status, d2=d2, partner=full["partner"])
    return row


def restate_register_trimmed(P, Q, normals, mn, mx, keep=0.8, max_dist=2.0, iterations=30, min_step=1e-6, lock_eps=1e-9, T0=None):
    """(T, rows, status, d2, stats) as Engine.register_trimmed gives them: restate_register's loop on restate_trimmed_terms"""
    T = IDENTITY.copy() if T0 is None else np.asarray(T0, np.float64).reshape(3, 4).copy()
    rows, converged, locked, stop = [], 0, 0, False
    while True:
        row = restate_trimmed_terms(P, Q, normals, mn, mx, max_dist, T, keep)
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
    return last["T"].copy(), rows, last["status"], last["d2"], stats


# ---------------------------------------------------------------- the contaminated case

RAISE_MM = 1.5
DIRTY = dict(KNOWN)                                                          # max_dist 3 and the defaults otherwise, from the identity
# the largest coordinate error of the moved-back scan over the points that were not raised, measured by the restatement with
# the oracle's normals at keep 0.8 (test_census_of_the_contaminated_case prints it), and the cap the GPU test asserts: 4 times
# that, never above 0.05 mm -- test_registration's convention: the normal estimate sets the floor, the margin covers the engine's
# own normals and nothing else
TRIMMED_MEASURED_MM = 2.95e-3
TRIM_CAP_MM = min(4 * TRIMMED_MEASURED_MM, 0.05)


@functools.lru_cache(maxsize=None)
def dirty_clouds():
    """(reference, unmoved scan with one eighth raised, moved scan float32, raised bool[n], the motion); nobody writes to them"""
    ref = relief_plate(94, 52, 31, 20.0)
    scan = relief_plate(80, 44, 32, 30.0).copy()
    x, y = scan[:, 0], scan[:, 1]
    raised = (x < x.min() + 0.25 * (x.max() - x.min())) & (y < y.min() + 0.5 * (y.max() - y.min()))
    scan[raised, 2] += np.float32(RAISE_MM)
    _, _, c = box_centre(ref)
    Tm = motion_about(c, MOTION_DEG, MOTION_SHIFT)
    moved = apply(Tm, scan).astype(np.float32)
    for a in (ref, scan, moved, raised, Tm):
        a.setflags(write=False)
    return ref, scan, moved, raised, Tm


def clean_error(T, moved, scan, raised):
    return float(np.abs(apply(T, moved[~raised]) - scan[~raised].astype(np.float64)).max())


@functools.lru_cache(maxsize=None)
def dirty_restated_cpu(keep):
    ref, scan, moved, raised, Tm = dirty_clouds()
    mn, mx, _ = box_centre(ref)
    return restate_register_trimmed(moved, ref, oracle_normals(ref), mn, mx, keep=keep, **DIRTY)


# ---------------------------------------------------------------- the tie and digit cases: a flat lattice, the scan above it


@functools.lru_cache(maxsize=None)
def lattice():
    """a flat reference lattice at z = 0: 40 x 24 points, 1.5 mm apart, coordinates exact in float"""
    gx, gy = np.meshgrid(np.arange(40, dtype=np.float32) * np.float32(1.5) + np.float32(16.0), np.arange(24, dtype=np.float32) * np.float32(1.5) - np.float32(18.0))
    ref = np.stack([gx.ravel(), gy.ravel(), np.zeros(gx.size, np.float32)], axis=1).astype(np.float32)
    ref.setflags(write=False)
    return ref


def above_lattice(zs):
    """the scan: the interior lattice points (the rim's normals may be missing) at the heights zs, cycled; d2 = z * z exactly where
    the normal exists, as x and y agree"""
    ref = lattice()
    inner = (ref[:, 0] > ref[:, 0].min() + 4) & (ref[:, 0] < ref[:, 0].max() - 4) & (ref[:, 1] > ref[:, 1].min() + 4) & (ref[:, 1] < ref[:, 1].max() - 4)
    scan = ref[inner].copy()
    zs = np.asarray(zs, np.float32)
    scan[:, 2] = zs[np.arange(len(scan)) % len(zs)]
    return scan


TIES = dict(max_dist=3.0, iterations=1, min_step=1e-6, lock_eps=1e-3)


def tie_scan(moved=0):
    """half the points at z = 0.5, half at z = 1.0 (alternating); `moved` points of the 0.5 group lifted to 1.0"""
    scan = above_lattice([0.5, 1.0])
    low = np.nonzero(scan[:, 2] == np.float32(0.5))[0]
    scan[low[:moved], 2] = np.float32(1.0)
    return scan


def f32_from_bits(b):
    return np.array([b], np.uint32).view(np.float32)[0]


def digit_heights():
    """z values whose float squares -- d2 is the float product z * z, the other two differences being zero -- are keys of three
    kinds: g0, four keys that differ only in the low digit (z = 0.5 + 100 i 2^-24: the squares lie 200 ulps apart above
    0.25, whose low digits are zero); g1, keys that share the top digit with g0 and differ first in the middle digit (z = 0.5
    + j 2^-12: 8 192 ulps apart); g2, keys in other binades: another top digit"""
    zs = [0.5 + 100 * i * 2.0 ** -24 for i in range(1, 5)]
    zs += [0.5 + j * 2.0 ** -12 for j in range(1, 4)]
    zs += [1.25, 1.5, 0.125]
    return np.array(zs, np.float32)


# ---------------------------------------------------------------- CPU


def test_header_declares_and_engine_exports_trimmed_registration(engine_mod):
    hdr = open(os.path.join(ROOT, "include", "ppp_hip.h")).read()
    decls = (TPARAMS_DECL, TROW_DECL, TENUM_DECL) + TFUNC_DECLS
    for decl in decls:
        assert decl in hdr, decl
    at = [hdr.index("int  ppp_register(")] + [hdr.index(d) for d in decls] + [hdr.index("int  ppp_transform_cloud(")]
    assert at == sorted(at)
    assert "DESIGN.md 7m" in hdr and "0x7fc00000" in hdr
    L = ctypes.CDLL(engine_mod.LIB_PATH)
    for sym in ("ppp_default_trimmed_registration_params", "ppp_register_trimmed"):
        assert sym in engine_mod.EXPORTS and hasattr(L, sym)
    assert hasattr(engine_mod.Engine, "register_trimmed")
    assert (engine_mod.TRIM_KEPT, engine_mod.TRIM_TRIMMED, engine_mod.TRIM_UNPAIRED, engine_mod.TRIM_DROPPED) == (0, 1, 2, 3)
    for h in ("Path_Generate.h", "Path_Generate_Algorithm.h", "robot_path.h"):
        assert "register_trimmed_to(" in open(os.path.join(ROOT, "include", h)).read(), h
    planner = open(os.path.join(ROOT, "include", "ppp_planner.hpp")).read()
    for name in ("register_trimmed_to(", "trimmed_registration_params_env()", "PPP_REGISTER_KEEP", "ppp_register_trimmed("):
        assert name in planner, name


def test_header_is_c99_clean_with_trimmed_registration(tmp_path):
    src = tmp_path / "c99.c"
    src.write_text('#include "ppp_hip.h"\nint main(void) {\n'
                   '    int (*g)(ppp_handle, ppp_handle, const ppp_trimmed_registration_params *, const double *, ppp_trimmed_registration_row *,\n'
                   '             size_t, unsigned char *, float *, size_t, ppp_registration_stats *) = ppp_register_trimmed;\n'
                   '    void (*d)(ppp_trimmed_registration_params *) = ppp_default_trimmed_registration_params;\n'
                   '    ppp_trimmed_registration_row row;\n    ppp_trimmed_registration_params tp;\n'
                   '    row.row.A[20] = 0; row.paired = 0; row.trim_d2 = 0.f; tp.keep = 0.8; tp.icp.iterations = 1;\n'
                   '    return g == 0 || d == 0 || row.row.A[20] != 0 || tp.keep > 1.0 || PPP_TRIM_DROPPED != 3 || PPP_TRIM_KEPT != 0;\n}\n')
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_trimmed_registration_structs_layout_matches_the_header(engine_mod, tmp_path):
    """the ctypes mirrors have the C structs' sizes and offsets; the defaults are ((2, 30, 1e-6, 1e-9), 0.8)"""
    src = tmp_path / "layout.c"
    structs = (("ppp_trimmed_registration_params", ("icp", "keep"), engine_mod.TrimmedRegistrationParams),
               ("ppp_trimmed_registration_row", ("row", "paired", "trim_d2"), engine_mod.TrimmedRegistrationRow))
    args, want = [], []
    for name, fields, T in structs:
        args += ["sizeof(%s)" % name] + ["offsetof(%s, %s)" % (name, f) for f in fields]
        want += [ctypes.sizeof(T)] + [getattr(T, f).offset for f in fields]
        assert tuple(f for f, _ in T._fields_) == fields
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ppp_hip.h"\nint main(void) {\n'
                   '    printf("' + " ".join(["%zu"] * len(args)) + '\\n", ' + ", ".join(args) + ');\n    return 0;\n}\n')
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)])
    got = [int(v) for v in subprocess.check_output([exe]).split()]
    assert got == want
    tp = engine_mod.TrimmedRegistrationParams()
    engine_mod.lib().ppp_default_trimmed_registration_params(ctypes.byref(tp))
    assert [tp.icp.max_dist, tp.icp.iterations, tp.icp.min_step, tp.icp.lock_eps, tp.keep] == [2.0, 30, 1e-6, 1e-9, 0.8]


def test_examples_build_with_the_trimmed_switch(engine_mod):
    for ex in ("connect.cpp", "robot.cpp"):
        src = open(os.path.join(ROOT, "examples", ex)).read()
        assert "PPP_REGISTER_KEEP" in src and "register_trimmed_to(" in src and "register_to(" in src, ex
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "examples"), "connect", "connect1", "robot", "main"])
    for exe in ("connect", "connect1", "robot", "main"):
        assert os.access(os.path.join(ROOT, "examples", exe), os.X_OK)


def test_census_of_the_contaminated_case():
    """Reference 94 x 52, scan 80 x 44 of the relief surface; the scan's corner x < xmin + 0.25 (xmax - xmin), y < ymin + 0.5
    (ymax - ymin) -- one eighth of it -- raised by 1.5 mm, then the whole scan moved by MOTION_DEG / MOTION_SHIFT about the
    reference's box centre; max_dist 3, from the identity, the oracle's normals.  Measured with the restatement: untrimmed, 6
    steps to a fit that is 0.673 mm off over the clean points; keep 0.8 converges in 7 steps, keeps 2 816 of 3 520 pairs within
    0.810 mm^2 and is 2.95e-3 mm off (TRIMMED_MEASURED_MM), every raised point TRIMMED; keep 0.9 -- more than the clean share
    0.875 -- converges in 11 steps to a fit 0.896 mm off"""
    ref, scan, moved, raised, Tm = dirty_clouds()
    n = len(scan)
    share = raised.sum() / n
    print("n %d raised %d share %r" % (n, int(raised.sum()), share))
    assert n == 3520 and abs(share - 0.125) <= 0.01
    mn, mx, _ = box_centre(ref)
    T0, rows0, st0 = restate_register(moved, ref, oracle_normals(ref), mn, mx, **DIRTY)
    e0 = clean_error(T0, moved, scan, raised)
    print("untrimmed: steps %d converged %d error %r mm" % (st0["steps"], st0["converged"], e0))
    assert e0 >= 0.1
    T, rows, status, d2, st = dirty_restated_cpu(0.8)
    e = clean_error(T, moved, scan, raised)
    last = rows[-1]
    print("keep 0.8: steps %d converged %d kept %d of %d paired, cut %r mm^2, error %r mm (cap %r); raised: %d trimmed %d unpaired %d kept"
          % (st["steps"], st["converged"], last["pairs"], last["paired"], float(f32_from_bits(last["trim_bits"])), e, TRIM_CAP_MM,
             int((status[raised] == TRIMMED).sum()), int((status[raised] == UNPAIRED).sum()), int((status[raised] == KEPT).sum())))
    assert st["converged"] == 1 and st["steps"] <= 30
    assert np.all((status[raised] == TRIMMED) | (status[raised] == UNPAIRED))
    assert e <= TRIMMED_MEASURED_MM * 1.05 and e >= TRIMMED_MEASURED_MM / 1.05   # the constant is the measurement
    assert TRIM_CAP_MM <= 0.05
    for r in rows:
        assert r["pairs"] >= r["k"] == trim_rank(0.8, r["paired"]) and r["paired"] >= 0.7 * n
    T9, rows9, _, _, st9 = dirty_restated_cpu(0.9)
    e9 = clean_error(T9, moved, scan, raised)
    print("keep 0.9: steps %d converged %d error %r mm" % (st9["steps"], st9["converged"], e9))
    assert e9 > 0.1


def lattice_keys(scan, keep):
    ref = lattice()
    mn, mx, _ = box_centre(ref)
    N = oracle_normals(ref)
    row = restate_trimmed_terms(scan, ref, N, mn, mx, TIES["max_dist"], IDENTITY, keep)
    return row


def test_census_of_the_tie_and_digit_cases():
    """by restatement alone: every scan point above the lattice pairs with the lattice point below it at d2 = z * z; the tie case
    has two keys, each on half the pairs; the digit case's keys are of the three kinds, read from their bits"""
    scan = tie_scan()
    row = lattice_keys(scan, 0.5)
    n = len(scan)
    keys = row["d2"].view(np.uint32)
    assert row["paired"] == n and n % 2 == 0 and np.array_equal(row["d2"], scan[:, 2] * scan[:, 2])
    assert sorted(set(keys.tolist())) == [int(np.float32(0.25).view(np.uint32)), int(np.float32(1.0).view(np.uint32))]
    assert int((row["d2"] == np.float32(0.25)).sum()) == n // 2 == row["k"] == row["pairs"] and row["trim_bits"] == int(np.float32(0.25).view(np.uint32))
    one = lattice_keys(tie_scan(1), 0.5)
    assert one["k"] == n // 2 and one["pairs"] == n and one["trim_bits"] == int(np.float32(1.0).view(np.uint32))   # k lands among the ties
    quarter = lattice_keys(tie_scan(), 0.25)
    assert quarter["k"] == n // 4 and quarter["pairs"] == n // 2
    zs = digit_heights()
    scan = above_lattice(zs)
    row = lattice_keys(scan, 0.5)
    assert row["paired"] == len(scan) and np.array_equal(row["d2"], scan[:, 2] * scan[:, 2])
    kz = (zs * zs).view(np.uint32).astype(np.int64)
    assert len(set(kz.tolist())) == len(zs)
    g0, g1, g2 = kz[:4], kz[4:7], kz[7:]
    assert len(set((g0 >> MID).tolist())) == 1 and len(set((g0 & 0x3FF).tolist())) == 4               # the low digit alone differs
    assert len(set((np.concatenate([g0, g1]) >> TOP).tolist())) == 1                                   # one top digit ...
    assert len(set(((np.concatenate([g0[:1], g1]) >> MID) & 0x7FF).tolist())) == 4                     # ... four middle digits
    assert len(set((np.concatenate([g0[:1], g2]) >> TOP).tolist())) == 4                               # four top digits
    for keep, want in digit_sweep(len(scan), zs):
        assert lattice_keys(scan, keep)["trim_bits"] == want, keep


def digit_sweep(n, zs):
    """[(keep, the tau expected)]: for every distinct key, a share that puts k on it, and the shares at the group boundaries"""
    counts = np.bincount(np.arange(n) % len(zs), minlength=len(zs))          # points per height: above_lattice cycles the heights
    order = np.argsort((zs * zs).view(np.uint32))
    out, below = [], 0
    for i in order:
        c = int(counts[i])
        for k in (below + 1, below + c):                                     # the first and the last rank on this key
            keep = (k - 0.5) / n
            assert trim_rank(keep, n) == k
            out.append((keep, int((zs[i] * zs[i]).view(np.uint32))))
        below += c
    return out


# ---------------------------------------------------------------- GPU

TROW_EXACT = tr.ROW_EXACT + ("paired", "trim_bits")


def trows_equal(got, want):
    assert len(got) == len(want), (len(got), len(want))
    for k, (g, w) in enumerate(zip(got, want)):
        for f in TROW_EXACT:
            assert same(g[f], w[f]), (k, f, g[f], w[f])


def maps_equal(status, d2, wstatus, wd2):
    assert status.dtype == np.uint8 and d2.dtype == np.float32
    assert status.tobytes() == wstatus.tobytes()
    assert d2.tobytes() == wd2.tobytes()                                     # the NaNs too: 0x7fc00000 on either side


def trimmed_restated_from(s, r, **kw):
    mn, mx = r.minmax()
    return restate_register_trimmed(s.cloud(), r.cloud(), r.estimate_normals(), mn, mx, **kw)


def trimmed_parity(engine_mod, ref, scan, T0=None, **p):
    """Engine.register_trimmed on fresh handles against the restatement fed by the engine's getters: rows, maps, stats, T"""
    r, s = engines(engine_mod, ref, scan)
    got = s.register_trimmed(r, T0=T0, **p)
    want = trimmed_restated_from(s, r, T0=T0, **p)
    T, rows, status, d2, st = got
    print("steps %d (want %d) converged %d (want %d) kept %r paired %r cut %r rms %r -> %r"
          % (st["steps"], want[4]["steps"], st["converged"], want[4]["converged"], [w["pairs"] for w in rows], [w["paired"] for w in rows],
             [w["trim_d2"] for w in rows], st["rms_before"], st["rms_after"]))
    trows_equal(rows, want[1])
    tr.stats_equal(st, want[4])
    maps_equal(status, d2, want[2], want[3])
    assert same(T, want[0]) and same(T, rows[-1]["T"]) and rows[-1]["locked"] == ALL_LOCKED and math.isnan(rows[-1]["step2"])
    r.close(); s.close()
    return got, want


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["known", "census"])
def test_keep_one_is_register_bit_for_bit(engine_mod, case):
    if case == "known":
        ref, _, scan, _ = known_clouds()
        T0, p = None, KNOWN
    else:
        ref, scan, _ = main_clouds()
        T0, p = census_T0(), CENSUS
    r, s = engines(engine_mod, ref, scan)
    T, rows, st = s.register(r, T0=T0, **p)
    tT, trows, status, d2, tst = s.register_trimmed(r, keep=1.0, T0=T0, **p)
    print("steps %d pairs %r" % (st["steps"], [w["pairs"] for w in rows]))
    assert st["steps"] >= 3
    tr.rows_equal(trows, rows)
    tr.stats_equal(tst, st)
    assert same(tT, T)
    for w in trows:
        assert w["paired"] == w["pairs"]
    assert not np.any(status == TRIMMED) and int((status == KEPT).sum()) == trows[-1]["pairs"]
    assert trows[-1]["trim_bits"] == int(d2[status == KEPT].max().view(np.uint32))
    assert np.all(np.isnan(d2[status != KEPT])) and int((status == DROPPED).sum()) == st["n"] - st["indexed"]
    r.close(); s.close()


@pytest.mark.gpu
def test_chain_matches_the_restatement_on_the_contaminated_case(engine_mod):
    ref, scan, moved, raised, Tm = dirty_clouds()
    (T, rows, status, d2, st), _ = trimmed_parity(engine_mod, ref, moved, keep=0.8, **DIRTY)
    assert st["converged"] == 1 and st["steps"] >= 3
    assert all(w["pairs"] < w["paired"] for w in rows) and np.any(status == TRIMMED)


@pytest.mark.gpu
def test_contaminated_scan_end_to_end(engine_mod):
    """the engine's own normals: the trimmed fit stays under the cap over the clean points, every raised point is cut off,
    and ppp_register on the same handles stays above 0.1 mm"""
    ref, scan, moved, raised, Tm = dirty_clouds()
    r, s = engines(engine_mod, ref, moved)
    T, rows, status, d2, st = s.register_trimmed(r, keep=0.8, **DIRTY)
    e = clean_error(T, moved, scan, raised)
    T0, _, st0 = s.register(r, **DIRTY)
    e0 = clean_error(T0, moved, scan, raised)
    print("trimmed: steps %d converged %d error %r mm (cap %r); untrimmed: steps %d converged %d error %r mm"
          % (st["steps"], st["converged"], e, TRIM_CAP_MM, st0["steps"], st0["converged"], e0))
    assert st["converged"] == 1
    assert e <= TRIM_CAP_MM
    assert e0 > 0.1
    assert np.all((status[raised] == TRIMMED) | (status[raised] == UNPAIRED))
    r.close(); s.close()


def row0(engine_mod, r, s, keep, **p):
    T, rows, status, d2, st = s.register_trimmed(r, keep=keep, **p)
    return rows[0], status, d2, st


@pytest.mark.gpu
def test_ties_at_the_cut(engine_mod):
    ref = lattice()
    bits = lambda v: int(np.float32(v).view(np.uint32))
    for moved, keep, tau, kept_of in ((0, 0.5, 0.25, lambda n: n // 2), (1, 0.5, 1.0, lambda n: n), (0, 0.25, 0.25, lambda n: n // 2)):
        scan = tie_scan(moved)
        n = len(scan)
        r, s = engines(engine_mod, ref, scan)
        mn, mx = r.minmax()
        want = restate_trimmed_terms(s.cloud(), r.cloud(), r.estimate_normals(), mn, mx, TIES["max_dist"], IDENTITY, keep)
        got, status, d2, st = row0(engine_mod, r, s, keep, **TIES)
        k = trim_rank(keep, got["paired"])
        print("moved %d keep %r: paired %d k %d kept %d cut %r" % (moved, keep, got["paired"], k, got["pairs"], got["trim_d2"]))
        assert got["paired"] == n == want["paired"]                          # the engine's normals exist under every scan point
        assert got["trim_bits"] == bits(tau) and got["pairs"] == kept_of(n)
        if moved or keep == 0.25:
            assert got["pairs"] > k                                          # the whole tied group is kept
        else:
            assert got["pairs"] == k == n // 2
        for f in ("pairs", "A", "b", "E", "paired", "trim_bits"):
            assert same(got[f], want[f]), f
        if st["steps"] == 0:                                                 # row 0 is then the last evaluation: the maps are its
            maps_equal(status, d2, want["status"], want["d2"])
        r.close(); s.close()


@pytest.mark.gpu
def test_digit_boundaries(engine_mod):
    """the keys of test_census_of_the_tie_and_digit_cases: k on the first and on the last rank of every distinct key, so the
    selection ends in each of the three digits' bins and at their edges"""
    ref = lattice()
    zs = digit_heights()
    scan = above_lattice(zs)
    r, s = engines(engine_mod, ref, scan)
    mn, mx = r.minmax()
    Q, N, P = r.cloud(), r.estimate_normals(), s.cloud()
    for keep, tau in digit_sweep(len(scan), zs):
        want = restate_trimmed_terms(P, Q, N, mn, mx, TIES["max_dist"], IDENTITY, keep)
        got, status, d2, st = row0(engine_mod, r, s, keep, **TIES)
        assert got["paired"] == len(scan) and want["trim_bits"] == tau
        for f in ("pairs", "A", "b", "E", "paired", "trim_bits"):
            assert same(got[f], want[f]), (keep, f, got[f], want[f])
    r.close(); s.close()


FEW_SEVENTH = (65.0, 20.0)                                                   # a seventh (x, y) well inside the reference: tr.FEW_AT has six


def few_pairs(k):
    """test_registration.few_pairs_scan(k); for k = 7, which its six places do not reach, the same scan with a seventh place"""
    if k <= len(tr.FEW_AT):
        return few_pairs_scan(k)
    _, scan, _ = main_clouds()
    keep = []
    for x, y in (tr.FEW_AT + (FEW_SEVENTH,))[:k]:
        d = (scan[:, 0] - x) ** 2 + (scan[:, 1] - y) ** 2
        d[keep] = np.inf
        keep.append(int(np.nanargmin(d)))
    out = scan.copy()
    rest = np.ones(len(scan), bool)
    rest[keep] = False
    out[rest, 2] += np.float32(1000.0)
    return out, keep


@pytest.mark.gpu
@pytest.mark.parametrize("k", [0, 5, 6, 7])
def test_few_pairs(engine_mod, k):
    """keep 0.8 of k pairs: ceil(0.8 k) kept -- 0, 4, 5 and 6 -- so only k = 7 leaves the six a step needs"""
    ref, _, _ = main_clouds()
    scan, keep_at = few_pairs(k)
    assert len(keep_at) == len(set(keep_at)) == k
    (T, rows, status, d2, st), _ = trimmed_parity(engine_mod, ref, scan, keep=0.8, **dict(CENSUS))
    assert rows[0]["paired"] == k and rows[0]["pairs"] == trim_rank(0.8, k) == (0, 0, 0, 0, 0, 4, 5, 6)[k]
    assert int((status == KEPT).sum()) == rows[-1]["pairs"] and (st["steps"] > 0 or np.all(status[keep_at] <= TRIMMED))
    if k == 0:
        assert rows[0]["trim_bits"] == NAN32_BITS and math.isnan(rows[0]["trim_d2"]) and rows[0]["pairs"] == 0
        assert not np.any(status == KEPT) and not np.any(status == TRIMMED) and np.all(np.isnan(d2))
    if rows[0]["pairs"] < 6:
        assert st["steps"] == 0 and st["converged"] == 0 and len(rows) == 1 and same(T, IDENTITY)
    else:
        assert k == 7 and st["steps"] >= 1


@pytest.mark.gpu
def test_chain_beyond_the_grid_cap(engine_mod):
    """large_clouds() from large_T0(): the grid-stride loops of the four kernels take a second trip and every workgroup's
    histogram is flushed into the shared one; rows, maps, statistics and T bit for bit"""
    ref, scan, _ = large_clouds()
    (T, rows, status, d2, st), _ = trimmed_parity(engine_mod, ref, scan, T0=large_T0(), keep=0.8, **LARGE)
    past_the_grid_cap(st["indexed"])
    assert st["steps"] == 2 and rows[0]["paired"] >= 1500 and all(w["pairs"] < w["paired"] for w in rows)


@pytest.mark.gpu
def test_window_path_and_slab_path_register_alike(engine_mod):
    ref, scan, moved, raised, Tm = dirty_clouds()
    out = []
    for fast in (True, False):
        r, s = engines(engine_mod, ref, moved, tool_radius=6.0, walk=1, fast_path=fast)
        assert r.fast_path() == fast and s.fast_path() == fast
        out.append(s.register_trimmed(r, keep=0.8, **DIRTY))
        assert r.fast_path() == fast and s.fast_path() == fast
        r.close(); s.close()
    assert out[0][4]["steps"] >= 3 and same(out[0], out[1])


@pytest.mark.gpu
def test_same_bits_on_fresh_handles_and_nothing_stored_is_touched(engine_mod):
    ref, scan, moved, raised, Tm = dirty_clouds()
    out = []
    for _ in range(2):
        r, s = engines(engine_mod, ref, moved)
        dev0 = s.deviation(r, max_dist=3.0)
        reg0 = s.register(r, **DIRTY)
        clouds = s.cloud().copy(), r.cloud().copy()
        out.append(s.register_trimmed(r, keep=0.8, **DIRTY))
        again = s.register_trimmed(r, keep=0.8, **DIRTY)
        assert same(again, out[-1])
        assert same(s.deviation(r, max_dist=3.0), dev0) and same(s.register(r, **DIRTY), reg0)
        assert same(s.cloud(), clouds[0]) and same(r.cloud(), clouds[1])
        r.close(); s.close()
    assert same(out[0], out[1])


@pytest.mark.gpu
def test_refusals(engine_mod):
    from polishpathplanning_amd import synth
    from polishpathplanning_amd.robot_path import slice_ranges
    ref, scan, _ = main_clouds()
    r, s = engines(engine_mod, ref, scan)
    for keep in (0.0, -0.5, 1.000001, NAN):
        with pytest.raises(engine_mod.PPPError) as ex:
            s.register_trimmed(r, keep=keep, T0=census_T0(), **CENSUS)
        assert ex.value.code == engine_mod.ERR_ARG, keep
    for bad in (dict(max_dist=0.0), dict(iterations=0), dict(iterations=65), dict(min_step=-1.0), dict(lock_eps=1.0)):
        with pytest.raises(engine_mod.PPPError) as ex:
            s.register_trimmed(r, keep=0.8, **dict(CENSUS, **bad))
        assert ex.value.code == engine_mod.ERR_ARG, bad
    L = s.L
    tp = engine_mod.TrimmedRegistrationParams(engine_mod.RegistrationParams(CENSUS["max_dist"], CENSUS["iterations"], CENSUS["min_step"], CENSUS["lock_eps"]), 0.8)
    raw = engine_mod.RegistrationStats()
    t0 = np.ascontiguousarray(census_T0().reshape(12))
    pt0 = t0.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    assert L.ppp_register_trimmed(s.h, r.h, None, pt0, None, 0, None, None, 0, ctypes.byref(raw)) == engine_mod.ERR_ARG
    assert L.ppp_register_trimmed(s.h, None, ctypes.byref(tp), pt0, None, 0, None, None, 0, ctypes.byref(raw)) == engine_mod.ERR_ARG
    assert L.ppp_register_trimmed(s.h, r.h, ctypes.byref(tp), pt0, None, 3, None, None, 0, ctypes.byref(raw)) == engine_mod.ERR_ARG
    # cap 0 with NULL maps, and NULL maps with a cap: the statistics alone
    T, rows, status, d2, st = s.register_trimmed(r, keep=0.8, T0=census_T0(), **CENSUS)
    assert len(rows) >= 4
    for cap in (0, len(scan)):
        assert L.ppp_register_trimmed(s.h, r.h, ctypes.byref(tp), pt0, None, 0, None, None, cap, ctypes.byref(raw)) == 0
        tr.stats_equal(engine_mod._registration_stats(raw), st)
    none = s.register_trimmed(r, keep=0.8, T0=census_T0(), maps=False, **CENSUS)
    assert none[2] is None and none[3] is None and same((none[0], none[1], none[4]), (T, rows, st))
    # row_cap below steps + 1: the first rows only, nothing written behind them; cap below n: the first entries of the maps
    buf = (engine_mod.TrimmedRegistrationRow * 5)()
    size = ctypes.sizeof(engine_mod.TrimmedRegistrationRow)
    ctypes.memset(buf, 0xA5, 5 * size)
    st8 = np.full(16, 0xA5, np.uint8); d8 = np.full(16, 7.0, np.float32)
    assert L.ppp_register_trimmed(s.h, r.h, ctypes.byref(tp), pt0, buf, 2, st8.ctypes.data_as(ctypes.POINTER(ctypes.c_ubyte)),
                                  d8.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), 8, ctypes.byref(raw)) == 0
    trows_equal([engine_mod._trimmed_registration_row(buf[0]), engine_mod._trimmed_registration_row(buf[1])], rows[:2])
    assert ctypes.string_at(ctypes.addressof(buf) + 2 * size, 3 * size) == b"\xa5" * (3 * size)
    assert st8[:8].tobytes() == status[:8].tobytes() and d8[:8].tobytes() == d2[:8].tobytes()
    assert np.all(st8[8:] == 0xA5) and np.all(d8[8:] == 7.0)
    # a slice-range handle and a part handle
    pts, cfg = synth.make_config("tiny_5k")
    w = engine_mod.Engine(0, tool_radius=cfg["tool_radius"], walk=1)
    w.set_cloud(pts)
    S = w.gen_path()
    lo, hi = slice_ranges(S, 2)[1]
    h = engine_mod.Engine(0, tool_radius=cfg["tool_radius"], walk=1, slice_begin=lo, slice_end=hi)
    h.set_cloud(pts)
    for a, b in ((h, w), (w, h)):
        with pytest.raises(engine_mod.PPPError) as ex:
            a.register_trimmed(b, keep=0.8, max_dist=3.0)
        assert ex.value.code == engine_mod.ERR_UNSUPPORTED
    part = part_handle(engine_mod, w, pts, cfg)
    for a, b in ((part, w), (w, part)):
        with pytest.raises(engine_mod.PPPError) as ex:
            a.register_trimmed(b, keep=0.8, max_dist=3.0)
        assert ex.value.code == engine_mod.ERR_UNSUPPORTED
    part.close()
    # every refusal leaves a later good call working
    assert same(s.register_trimmed(r, keep=0.8, T0=census_T0(), **CENSUS), (T, rows, status, d2, st))
    for e in (r, s, w, h):
        e.close()


def part_handle(engine_mod, whole, pts, cfg):
    """a handle that holds a part of the cloud (ppp_set_cloud_part), as test_deviation makes it"""
    scaled = (pts * np.float32(1000)).astype(np.float32)
    mn, mx = scaled.min(axis=0), scaled.max(axis=0)
    p = engine_mod.Engine(0, tool_radius=cfg["tool_radius"], slice_begin=2, slice_end=9)
    lo, hi, _ = p.range_interval(mn[0], mx[0])
    keep = np.nonzero((scaled[:, 0] >= lo) & (scaled[:, 0] <= hi))[0]
    p.set_cloud_part(pts[keep], keep, mn, mx, len(pts), lo, hi)
    return p


@pytest.mark.gpu
def test_connect_registers_trimmed(engine_mod, tmp_path):
    """PPP_REGISTER=1 PPP_REGISTER_KEEP=0.8 PPP_DEVIATION=<ref.pcd> ./connect <scan.pcd> on the contaminated pair: the kept /
    paired line, then the deviation's lines; without PPP_REGISTER_KEEP -- and with a share that is not below 1 -- the output
    is ppp_register's, line for line"""
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "examples"), "connect"])
    ref, scan, moved, raised, Tm = dirty_clouds()
    ref_pcd, scan_pcd = str(tmp_path / "ref.pcd"), str(tmp_path / "scan.pcd")
    engine_mod.save_pcd(ref_pcd, ref, binary=True)
    engine_mod.save_pcd(scan_pcd, moved, binary=True)
    conf = tmp_path / "config.txt"
    conf.write_text("Tool_Radius = 6\npathFile = %s\nPathResolution = 7\nRPYresolution = 7\nEnd effector length = 0.3\n"
                    "Smooth = false\nAlignment = false\nChangeRange = false\nRemoveOutlier = false\nDynamic_adjustment = false\n"
                    "Adjust_Threshold = 1\ntoolthickness = 10\ndepth = 0.01\n" % str(tmp_path / "wp.txt"))
    exe = os.path.join(ROOT, "examples", "connect")

    def run(**extra):
        env = {k: v for k, v in os.environ.items() if not k.startswith("PPP_")}
        env.update(PPP_CONFIG=str(conf), PPP_DEVIATION=ref_pcd, PPP_REGISTER="1", PPP_REGISTER_MAXDIST="3", PPP_DEVIATION_MAXDIST="3", **extra)
        r = subprocess.run([exe, scan_pcd], env=env, capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
        assert r.returncode == 0, r.stderr
        return [ln for ln in r.stdout.splitlines() if not ln.startswith("Toal Using Time")]

    plain, one, trimmed = run(), run(PPP_REGISTER_KEEP="1"), run(PPP_REGISTER_KEEP="0.8")
    assert plain == one and not any("pairs kept" in ln for ln in plain)
    r, s = engines(engine_mod, ref, moved)
    T, rows, status, d2, st = s.register_trimmed(r, keep=0.8, **DIRTY)
    T0, rows0, st0 = s.register(r, **DIRTY)
    want = "registration: keep %f: %d of %d pairs kept within %f mm^2; after %d steps %d of %d within %f mm^2" % (
        0.8, rows[0]["pairs"], rows[0]["paired"], rows[0]["trim_d2"], st["steps"], rows[-1]["pairs"], rows[-1]["paired"], rows[-1]["trim_d2"])
    reg = [ln for ln in trimmed if ln.startswith("registration: ")]
    print("\n".join(reg))
    assert reg[0] == want and len(reg) == 6 and reg[2] == "registration: converged, locked unknowns 0x00 (rotation x y z, translation x y z from bit 0)"
    reg0 = [ln for ln in plain if ln.startswith("registration: ")]
    assert len(reg0) == 5 and ("after %d steps" % st0["steps"]) in reg0[0]
    dev = [ln for ln in trimmed if ln.startswith("deviation: ")]
    assert len(dev) == 3 and " matched, " in dev[0] and trimmed.index(dev[0]) > trimmed.index(reg[-1])
    s.transform_cloud(T)
    assert dev[0].startswith("deviation: %d points: %d matched, " % (len(moved), s.deviation(r, max_dist=3.0, maps=False)[5]["matched"]))
    r.close(); s.close()
