"""Robust registration of a scan held as slice-range tiles (ppp_robust_sigma, ppp_robust_weight, ppp_register_robust_tiles;
DESIGN.md 7r and B.106-B.110).

Every comparison is for equality.  A pair, its residual and its key are a point's own, the median is a rank statistic of the union
of the keys -- found on histograms that add bin by bin --, sigma and the cut follow from the merged median by one routine that the
host and the device compile alike, and the 30 words add as integers: for ranges that tile the walk the tiled loop must be
ppp_register_robust's T, rows (words, pairs, used, weight_sum, the median's bits, sigma, locked, step2), statistics and maps on
whole-cloud handles, bit for bit.  No tolerance appears anywhere in this file.

The clouds are the whole-cloud tests': dirty_clouds (5 slices, cut into [0, 1), [1, 3), [3, 5); the raised eighth lies below
x = 60, inside the two low tiles), the lattice with median_scan and tied_scan above it (3 slices, cut into [0, 2), [2, 3): the seam
at x = 57.125 runs through the scan), the main scan with all but a few points lifted out of reach, and large_clouds past the grid
cap."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

from test_deviation import KW0, large_clouds, main_clouds, past_the_grid_cap
from test_deviation_tiles import cuts_of, device_count, finite_rows, handle, ranges3
from test_path_dwell import same
from test_registration import ALL_LOCKED, CENSUS, IDENTITY, KNOWN, LARGE, NAN, box_centre, known_clouds, large_T0, oracle_normals, rows_equal, stats_equal
from test_registration_tiles import SHIFT_5MM, THIN_MARGIN, indexed_interval, moved_x, open_tiles, owned_rows, reach_of, refusing
from test_robust_registration import (DROPPED, LAT, NAN64_BITS, REJECTED, UNPAIRED, USED, biweight, bits32, brows_equal, dirty_restated_cpu, maps_equal,
                                      median_scan, restate_register_robust, restate_robust_terms, tied_scan)
from test_trimmed_registration import DIRTY, NAN32_BITS, above_lattice, digit_heights, dirty_clouds, f32_from_bits, few_pairs, lattice, trim_rank
from test_trimmed_registration_tiles import FEW_RANGES, few_scan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
FUNC_DECLS = ("double ppp_robust_sigma(unsigned int median_bits, int none, double sigma_min);",
              "double ppp_robust_weight(double r, double cs, double tune);",
              "int    ppp_register_robust_tiles(const ppp_handle *hs, const ppp_handle *refs, size_t count,\n"
              "                                 const ppp_robust_registration_params *bp, const double *T0_12,\n"
              "                                 ppp_robust_registration_row *rows, size_t row_cap,\n"
              "                                 unsigned char *const *status, float *const *weight, double *const *residual,\n"
              "                                 unsigned char *const *owned, size_t cap,\n"
              "                                 ppp_register_tiles_stats *stats);")
SYMBOLS = ("ppp_robust_sigma", "ppp_robust_weight", "ppp_register_robust_tiles")
DIRTY_RANGES = [(0, 1), (1, 3), (3, 5)]
LATTICE_RANGES = [(0, 2), (2, 3)]
SEAM = np.float32(57.125)                                                    # cut(2) of the lattice scans' walk
# a cut so wide that the six pairs of few_scan all keep a weight above zero: their largest |r| is below 0.2 mm and sigma is at
# least sigma_min = 1e-4, so cs = 1e6 sigma >= 100 mm
WIDE_TUNE = 1e6


def f64_bits(v):
    return int(np.array([v], np.float64).view(np.uint64)[0])


# ---------------------------------------------------------------- CPU: header, ABI, the two host calls


def test_header_declares_and_engine_exports_the_robust_tiles(engine_mod):
    hdr = open(os.path.join(ROOT, "include", "ppp_hip.h")).read()
    for decl in FUNC_DECLS:
        assert decl in hdr, decl
    at = [hdr.index("int    ppp_register_trimmed_tiles(")] + [hdr.index(d) for d in FUNC_DECLS] + [hdr.index("int ppp_eval_spline(")]
    assert at == sorted(at)
    between = hdr[hdr.index("int    ppp_register_trimmed_tiles("):hdr.index(FUNC_DECLS[0])]
    assert between.count("/*") == 1 and "DESIGN.md 7r, B.106-B.110" in between and "never a tile's own\n   count" in between
    for sym in SYMBOLS:
        assert sym in engine_mod.EXPORTS and hasattr(engine_mod.lib(), sym), sym
    assert callable(engine_mod.Engine.register_robust_tiles)
    for f in ("register_robust_tiles", "robust_sigma", "robust_weight", "merge_robust_maps"):
        assert callable(getattr(engine_mod, f)), f
    planner = open(os.path.join(ROOT, "include", "ppp_planner.hpp")).read()
    assert "inline bool register_robust_tiles(std::vector<Planner *> &tiles, std::vector<Planner *> &refs, ppp_register_tiles_stats &st," in planner
    mk = open(os.path.join(ROOT, "polishpathplanning_amd", "csrc", "Makefile")).read()
    assert "ppp_robust_tile.h" in [l for l in mk.splitlines() if l.startswith("SCAN_HDR")][0]
    assert '#include "ppp_robust_tile.h"' in open(os.path.join(ROOT, "polishpathplanning_amd", "csrc", "ppp_scan.hip")).read()


def test_header_is_c99_clean_with_the_robust_tiles(tmp_path):
    src = tmp_path / "c99.c"
    src.write_text('#include "ppp_hip.h"\nint main(void) {\n'
                   '    int (*g)(const ppp_handle *, const ppp_handle *, size_t, const ppp_robust_registration_params *, const double *,\n'
                   '             ppp_robust_registration_row *, size_t, unsigned char *const *, float *const *, double *const *,\n'
                   '             unsigned char *const *, size_t, ppp_register_tiles_stats *) = ppp_register_robust_tiles;\n'
                   '    double (*s)(unsigned int, int, double) = ppp_robust_sigma;\n'
                   '    double (*w)(double, double, double) = ppp_robust_weight;\n'
                   '    return g == 0 || s == 0 || w == 0;\n}\n')
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_robust_weight_against_biweight(engine_mod):
    """ppp_robust_weight against the restatement's biweight, bit for bit: tune = inf; cs = 0 with r = 0 and r != 0; |r| equal to cs
    and the doubles on either side of it; r negative; a seeded sweep"""
    E = engine_mod
    one = lambda r, cs, tune: f64_bits(biweight(np.array([r], np.float64), float(cs), float(tune))[0])
    cases = [(0.3, 1.0, INF), (-7.0, 0.0, INF), (1e300, 1e-300, INF),                                      # tune = inf: 1 whatever r and cs
             (0.0, 0.0, 4.685), (-0.0, 0.0, 4.685), (1e-300, 0.0, 4.685), (-2.0, 0.0, 4.685),             # cs = 0
             (0.5, 1.0, 4.0), (-0.5, 1.0, 4.0), (0.0, 1.0, 4.0), (-0.99, 1.0, 4.0), (3.0, 1.0, 4.0), (-3.0, 1.0, 4.0)]
    for cs in (1.0, 0.029, 4.685 * 1.4826 * 0.0062, 1e-4 * 4.685):
        for r in (cs, np.nextafter(cs, 0.0), np.nextafter(cs, INF)):
            cases += [(float(r), cs, 4.685), (-float(r), cs, 4.685)]
    for r, cs, tune in cases:
        assert f64_bits(E.robust_weight(r, cs, tune)) == one(r, cs, tune), (r, cs, tune)
    assert E.robust_weight(1.0, 1.0, 4.0) == 0.0 and E.robust_weight(-1.0, 1.0, 4.0) == 0.0 and E.robust_weight(np.nextafter(1.0, 0.0), 1.0, 4.0) > 0.0
    assert E.robust_weight(np.nextafter(1.0, INF), 1.0, 4.0) == 0.0 and E.robust_weight(0.5, 1.0, 4.0) == 0.5625
    assert (E.robust_weight(0.0, 0.0, 4.0), E.robust_weight(1e-300, 0.0, 4.0), E.robust_weight(5.0, 0.0, INF)) == (1.0, 0.0, 1.0)
    rs = np.random.RandomState(11)
    r = rs.randn(4000) * np.exp(rs.randn(4000) * 3.0)
    cs = np.abs(rs.randn(4000)) * np.exp(rs.randn(4000) * 3.0)
    L = E.lib()
    for a, b in zip(r, cs):
        assert f64_bits(L.ppp_robust_weight(float(a), float(b), 4.685)) == one(a, b, 4.685), (a, b)
    assert int((np.abs(r) < cs).sum()) > 500 and int((np.abs(r) >= cs).sum()) > 500


def test_robust_sigma_against_the_restatement(engine_mod):
    """ppp_robust_sigma against max(1.4826 * float(bits), sigma_min): none set, sigma_min binding and not, bits of 0, a denormal,
    a seeded sweep"""
    E = engine_mod
    want = lambda bits, smin: f64_bits(max(1.4826 * float(f32_from_bits(bits)), float(smin)))
    assert f64_bits(E.robust_sigma(0, True, 1e-4)) == NAN64_BITS and f64_bits(E.robust_sigma(bits32(0.5), 1, 0.0)) == NAN64_BITS
    assert f64_bits(E.lib().ppp_robust_sigma(0x3F000000, 7, 0.25)) == NAN64_BITS                       # any none != 0
    cases = [(0, 1e-4), (0, 0.0), (bits32(0.5), 1e-4), (bits32(1e-5), 1e-4), (bits32(0.25 / 1.4826), 0.25), (1, 0.0), (1, 1e-4), (0x007FFFFF, 0.0),
             (bits32(0.0062 / 1.4826), 1e-4), (0x7F7FFFFF, 1e-4)]
    for bits, smin in cases:
        assert f64_bits(E.robust_sigma(bits, False, smin)) == want(bits, smin), (hex(bits), smin)
    assert E.robust_sigma(0, False, 1e-4) == 1e-4 and E.robust_sigma(0, False, 0.0) == 0.0 and E.robust_sigma(bits32(1.0), False, 1e-4) == 1.4826
    assert E.robust_sigma(bits32(1e-5), False, 1e-4) == 1e-4 and E.robust_sigma(1, False, 0.0) == 1.4826 * float(f32_from_bits(1)) > 0.0
    rs = np.random.RandomState(5)
    for bits, smin in zip(rs.randint(0, 0x7F800000, 3000), np.abs(rs.randn(3000)) * np.exp(rs.randn(3000) * 4.0)):
        assert f64_bits(E.robust_sigma(int(bits), False, float(smin))) == want(int(bits), smin), (hex(int(bits)), smin)


def test_merge_robust_maps(engine_mod):
    E = engine_mod
    n32, n64 = np.float32(np.nan), np.nan
    s0, w0, r0, o0 = (np.array([USED, DROPPED, DROPPED, DROPPED], np.uint8), np.array([0.5, n32, n32, n32], np.float32), np.array([-0.25, n64, n64, n64]),
                      np.array([1, 0, 0, 0], np.uint8))
    s1, w1, r1, o1 = (np.array([DROPPED, REJECTED, UNPAIRED, DROPPED], np.uint8), np.array([n32, 0.0, n32, n32], np.float32),
                      np.array([n64, 2.0, n64, n64]), np.array([0, 1, 1, 0], np.uint8))
    status, weight, residual = E.merge_robust_maps([s0, s1], [w0, w1], [r0, r1], [o0, o1])
    assert status.dtype == np.uint8 and weight.dtype == np.float32 and residual.dtype == np.float64
    assert status.tolist() == [USED, REJECTED, UNPAIRED, DROPPED] and weight.view(np.uint32).tolist() == [0x3F000000, 0, NAN32_BITS, NAN32_BITS]
    assert residual.view(np.uint64).tolist() == [f64_bits(-0.25), f64_bits(2.0), NAN64_BITS, NAN64_BITS]
    assert same(E.merge_robust_maps([s1, s0], [w1, w0], [r1, r0], [o1, o0]), (status, weight, residual))     # any order of the tiles
    for bad in (([s0, s0], [w0, w0], [r0, r0], [o0, o0]), ([], [], [], []), ([s0, s1[:3]], [w0, w1[:3]], [r0, r1[:3]], [o0, o1[:3]]),
                ([s0, s1], [w0], [r0, r1], [o0, o1]), ([s0, s1], [w0, w1], [r0, r1[:3]], [o0, o1])):
        with pytest.raises(E.PPPError) as ex:
            E.merge_robust_maps(*bad)
        assert ex.value.code == E.ERR_ARG


# ---------------------------------------------------------------- CPU: the census of the GPU cases, by restatement


def words30(row):
    """the 30 words of a restated evaluation: used, A, b, E, weight_sum"""
    return [int(row["used"])] + [int(v) for v in row["A"]] + [int(v) for v in row["b"]] + [int(row["E"]), int(row["weight_sum"])]


def test_census_of_the_tiled_contaminated_case(engine_mod):
    """dirty_clouds in DIRTY_RANGES, the oracle's normals, no engine.  At the identity and at the chain's second transform every
    tile holds pairs and every tile's own median key differs from the merged tau, so a scale taken per tile would be caught (the raised eighth lies in the
    two low tiles; before the fit has tightened the motion's own residuals still decide the order of the tiles' medians, which
    the test prints); the tiles' restated 30 words, each
    tile weighing its pairs at the MERGED cut, add up to the whole restatement's; and for every transform of the chain every
    moved owned query's reach lies inside what the reference's matching default range handle indexes (B.89)"""
    E = engine_mod
    ref, scan, moved, raised, Tm = dirty_clouds()
    T, rows, status, weight, residual, st = dirty_restated_cpu()
    S, cuts = cuts_of(E, moved)
    Sr, rcuts = cuts_of(E, ref)
    assert S == Sr == 5 and ranges3(S) == ranges3(Sr) == DIRTY_RANGES and st["steps"] >= 3
    assert not owned_rows(moved, cuts, DIRTY_RANGES[2])[raised].any() and all(owned_rows(moved, cuts, r)[raised].any() for r in DIRTY_RANGES[:2])
    assert sum(int(owned_rows(moved, cuts, r).sum()) for r in DIRTY_RANGES) == st["indexed"] == len(moved)
    mn, mx, _ = box_centre(ref)
    N = oracle_normals(ref)
    for name, row in (("identity", rows[0]), ("second", rows[1])):
        assert name != "identity" or same(row["T"], IDENTITY)
        pair = row["partner"] >= 0
        keys = np.abs(row["residual"]).astype(np.float32).view(np.uint32)
        assert row["k"] == trim_rank(0.5, row["pairs"]) and row["median_bits"] == int(np.sort(keys[pair])[row["k"] - 1])
        own = []
        for r in DIRTY_RANGES:
            mine = np.sort(keys[owned_rows(moved, cuts, r) & pair])
            own.append(int(mine[trim_rank(0.5, len(mine)) - 1]))
            print("%s tile %r: %d pairs, own median %#x (%r mm), merged %#x (%r mm)" % (name, r, len(mine), own[-1], float(f32_from_bits(own[-1])),
                                                                                          row["median_bits"], float(f32_from_bits(row["median_bits"]))))
            assert len(mine) >= 6 and own[-1] != row["median_bits"]
        # B.108: a tile's words are its owned pairs' terms at the merged cut; they add up to the whole's in every word
        cs = float(row["sigma"]) * 4.685
        total = [0] * 30
        for r in DIRTY_RANGES:
            P = moved.copy()
            P[~owned_rows(moved, cuts, r)] = np.float32(NAN)                 # not indexed: the tile's scan with n unchanged
            tile = restate_robust_terms(P, ref, N, mn, mx, DIRTY["max_dist"], row["T"], tune=1.0, sigma_min=cs)
            # (tune 1 with the floor at the merged cs: the tile's own median is below it here, so its cut is the merged one)
            assert tile["sigma"] == cs and tile["shift"] == row["shift"] and 0 < tile["used"] <= tile["pairs"]
            total = [a + b for a, b in zip(total, words30(tile))]
        assert total == words30(row)
    reach = reach_of(DIRTY["max_dist"])
    for k, row in enumerate(rows):
        for r in DIRTY_RANGES:
            lo, hi = indexed_interval(E, ref, r)
            assert not refusing(moved_x(row["T"], moved[owned_rows(moved, cuts, r)]), lo, hi, mn[0], mx[0], reach).any(), (k, r)


def test_census_of_the_tiled_lattice_cases(engine_mod):
    """the lattice scans in LATTICE_RANGES, the seam through the scan: both tiles own points of every tied group of tied_scan, and
    of every key of median_scan's digit cases but the median's own, of which a scan holds two points only: they lie on either
    side of the seam in 30 of the 40 cases, and both below it in the ten cases (odd, "last") -- there the bin the selection ends in
    is fed by the low tile alone, and the high tile sends zeros for it; the rank that finds it is still the merged one"""
    E = engine_mod
    scan = tied_scan()
    S, cuts = cuts_of(E, scan)
    assert S == 3 and cuts_of(E, lattice())[0] == 3 and cuts[2] == SEAM
    keys = scan[:, 2].view(np.uint32)
    sides = [owned_rows(scan, cuts, r) for r in LATTICE_RANGES]
    assert sides[0].sum() + sides[1].sum() == len(scan) and all(int((keys[s] == key).sum()) >= 50 for s in sides for key in np.unique(keys))
    one_sided = []
    for odd in (False, True):
        for zt in digit_heights():
            for where in ("first", "last"):
                scan = median_scan(zt, where, odd)
                S, cuts = cuts_of(E, scan)
                assert S == 3 and cuts[2] == SEAM
                keys = scan[:, 2].view(np.uint32)
                sides = [owned_rows(scan, cuts, r) for r in LATTICE_RANGES]
                assert sides[0].sum() + sides[1].sum() == len(scan) and min(sides[0].sum(), sides[1].sum()) >= 100
                for key in np.unique(keys):
                    per = [int((keys[s] == key).sum()) for s in sides]
                    if key == bits32(zt):
                        assert sum(per) == 2
                        if min(per) == 0:
                            one_sided.append((odd, where))
                            assert per == [2, 0]
                    else:
                        assert min(per) >= 2, (odd, float(zt), where, hex(int(key)), per)
    assert one_sided == [(True, "last")] * len(digit_heights())


def test_census_of_the_few_pairs_cases(engine_mod):
    """few_scan's six pairs, three in each of two tiles, by restatement with the oracle's normals: at the defaults three of them
    keep a weight above zero (paired >= 6, used < 6: no step), at WIDE_TUNE all six do"""
    scan, six, cuts = few_scan(engine_mod)
    ref, _, _ = main_clouds()
    mn, mx, _ = box_centre(ref)
    N = oracle_normals(ref)
    row = restate_robust_terms(scan, ref, N, mn, mx, CENSUS["max_dist"], IDENTITY)
    wide = restate_robust_terms(scan, ref, N, mn, mx, CENSUS["max_dist"], IDENTITY, tune=WIDE_TUNE)
    print("six pairs: used %d at the defaults, %d at tune %r; |r| %r" % (row["used"], wide["used"], WIDE_TUNE, np.sort(np.abs(row["residual"][row["partner"] >= 0]))))
    assert row["pairs"] == wide["pairs"] == 6 and row["used"] < 6 and wide["used"] == 6
    assert np.abs(row["residual"][row["partner"] >= 0]).max() < 0.2


# ---------------------------------------------------------------- GPU


def whole_robust(E, ref, scan, **kw):
    r, s = handle(E, ref), handle(E, scan)
    out = s.register_robust(r, **kw)
    r.close(); s.close()
    return out


def tiled_equals_whole(E, ref, scan, ranges, ref_ranges=None, whole=None, **kw):
    """Engine.register_robust_tiles on `ranges` against Engine.register_robust on whole-cloud handles: T, rows, statistics, the
    merged maps; every tile's owned map is the cuts', the owned maps partition the finite points, and what a tile does not own
    keeps the fill.  Returns (the tiled answer, the whole one)"""
    want = whole_robust(E, ref, scan, **kw) if whole is None else whole
    hs, rs, everything = open_tiles(E, ref, scan, ranges, ref_ranges)
    got = E.register_robust_tiles(hs, rs, **kw)
    for e in everything:
        e.close()
    T, rows, statuses, weights, residuals, owneds, st = got
    wT, wrows, wstatus, wweight, wresidual, wst = want
    print("steps %d (whole %d) used %r paired %r median %r sigma %r" % (st["steps"], wst["steps"], [w["used"] for w in rows], [w["pairs"] for w in rows],
                                                                        [hex(w["median_bits"]) for w in rows], [w["sigma"] for w in rows]))
    brows_equal(rows, wrows); stats_equal(st, wst)
    assert same(T, wT) and same(T, rows[-1]["T"])
    _, cuts = cuts_of(E, scan)
    for r, status, weight, residual, owned in zip(ranges, statuses, weights, residuals, owneds):
        assert owned.dtype == np.uint8 and np.array_equal(owned == 1, owned_rows(scan, cuts, r)) and set(np.unique(owned)) <= {0, 1}
        out = owned == 0
        assert np.all(status[out] == DROPPED) and np.all(weight[out].view(np.uint32) == NAN32_BITS) and np.all(residual[out].view(np.uint64) == NAN64_BITS)
        maps_equal((status[~out], weight[~out], residual[~out]), (wstatus[~out], wweight[~out], wresidual[~out]))
    assert np.array_equal(np.sum(owneds, axis=0), finite_rows(scan).astype(np.int64))
    maps_equal(E.merge_robust_maps(statuses, weights, residuals, owneds), (wstatus, wweight, wresidual))
    return got, want


@pytest.mark.gpu
@pytest.mark.parametrize("ref_ranged", [False, True])
def test_tiled_robust_loop_equals_the_whole_loop(engine_mod, ref_ranged):
    """dirty_clouds at the defaults in three ranges, the reference whole or in its own three default ranges; fresh handles give the
    same bits; iterations used up; a row_cap below the number of rows; maps asked for some tiles only"""
    E = engine_mod
    ref, scan, moved, raised, Tm = dirty_clouds()
    ref_ranges = DIRTY_RANGES if ref_ranged else None
    got, want = tiled_equals_whole(E, ref, moved, DIRTY_RANGES, ref_ranges, **DIRTY)
    T, rows, statuses, weights, residuals, owneds, st = got
    assert st["converged"] == 1 and st["steps"] >= 3 and rows[-1]["used"] < rows[-1]["pairs"] and rows[-1]["sigma"] < rows[0]["sigma"]
    status, weight, _ = E.merge_robust_maps(statuses, weights, residuals, owneds)
    assert np.all(status[raised] == REJECTED) and np.all(weight[raised] == 0.0)
    again, _ = tiled_equals_whole(E, ref, moved, DIRTY_RANGES, ref_ranges, whole=want, **DIRTY)              # fresh handles
    assert same(again, got)
    two = dict(DIRTY, iterations=2)
    g2, w2 = tiled_equals_whole(E, ref, moved, DIRTY_RANGES, ref_ranges, **two)
    assert g2[6]["steps"] == 2 and g2[6]["converged"] == 0 and len(g2[1]) == 3
    # the C call: row_cap 2 of more rows, untouched memory behind them; some maps asked for, some not; everything optional
    hs, rs, everything = open_tiles(E, ref, moved, DIRTY_RANGES, ref_ranges)
    k, n = len(hs), len(moved)
    hv = (ctypes.c_void_p * k)(*[h.h for h in hs]); rv = (ctypes.c_void_p * k)(*[r.h for r in rs])
    bp = E.RobustRegistrationParams(E.RegistrationParams(DIRTY["max_dist"], DIRTY["iterations"], DIRTY["min_step"], DIRTY["lock_eps"]), 4.685, 1e-4)
    buf = (E.RobustRegistrationRow * 4)()
    size = ctypes.sizeof(E.RobustRegistrationRow)
    ctypes.memset(buf, 0xA5, 4 * size)
    raw = E.RegisterTilesStats()
    ub, fp, dp = ctypes.POINTER(ctypes.c_ubyte), ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_double)
    s1, o2, r0, w1 = np.full(n, 0xA5, np.uint8), np.full(n, 0xA5, np.uint8), np.full(n, 7.0, np.float64), np.full(n, 7.0, np.float32)
    sv = (ub * k)(None, s1.ctypes.data_as(ub), None); ov = (ub * k)(None, None, o2.ctypes.data_as(ub))
    rsv = (dp * k)(r0.ctypes.data_as(dp), None, None); wv = (fp * k)(None, w1.ctypes.data_as(fp), None)
    L = E.lib()
    half = n // 2
    assert L.ppp_register_robust_tiles(hv, rv, k, ctypes.byref(bp), None, buf, 2, sv, wv, rsv, ov, half, ctypes.byref(raw)) == 0 and raw.failed_tile == -1
    brows_equal([E._robust_registration_row(buf[0]), E._robust_registration_row(buf[1])], want[1][:2])
    stats_equal(E._registration_stats(raw.reg), want[5])
    assert ctypes.string_at(ctypes.addressof(buf) + 2 * size, 2 * size) == b"\xa5" * (2 * size)
    assert np.array_equal(s1[:half], statuses[1][:half]) and np.array_equal(o2[:half], owneds[2][:half])      # the first min(cap, n) entries
    assert r0[:half].tobytes() == residuals[0][:half].tobytes() and w1[:half].tobytes() == weights[1][:half].tobytes()
    assert np.all(s1[half:] == 0xA5) and np.all(o2[half:] == 0xA5) and np.all(r0[half:] == 7.0) and np.all(w1[half:] == 7.0)
    assert L.ppp_register_robust_tiles(hv, rv, k, ctypes.byref(bp), None, None, 0, None, None, None, None, 0, None) == 0
    none = E.register_robust_tiles(hs, rs, maps=False, **DIRTY)
    assert none[2:6] == (None, None, None, None) and same((none[0], none[1], none[6]), (T, rows, st))
    for e in everything:
        e.close()


def handle_register(E, ref, scan):
    r, s = handle(E, ref), handle(E, scan)
    out = s.register(r, **KNOWN)
    r.close(); s.close()
    return out


@pytest.mark.gpu
def test_infinite_tune_is_the_tiled_register(engine_mod):
    """tune = inf on the known motion: the rows' words, T and the statistics are ppp_register_tiles', and so ppp_register's"""
    E = engine_mod
    ref, scan, moved, Tm = known_clouds()
    S, _ = cuts_of(E, moved)
    hs, rs, everything = open_tiles(E, ref, moved, ranges3(S))
    T, rows, st = E.register_tiles(hs, rs, **KNOWN)
    bT, brows, statuses, weights, residuals, owneds, bst = E.register_robust_tiles(hs, rs, tune=INF, **KNOWN)
    wT, wrows, wst = handle_register(E, ref, moved)
    for e in everything:
        e.close()
    assert st["steps"] >= 3
    rows_equal(brows, rows); stats_equal(bst, st); assert same(bT, T)
    rows_equal(brows, wrows); stats_equal(bst, wst); assert same(bT, wT)
    status, weight, residual = E.merge_robust_maps(statuses, weights, residuals, owneds)
    for w in brows:
        assert w["used"] == w["pairs"] and w["weight_sum"] == w["pairs"] << st["shift"]
    assert not np.any(status == REJECTED) and int((status == USED).sum()) == brows[-1]["pairs"] and np.all(weight[status == USED] == 1.0)


@pytest.mark.gpu
@pytest.mark.parametrize("odd", [False, True])
def test_medians_across_the_seam(engine_mod, odd):
    """the lattice in two ranges: for each of median_scan's low-, middle- and top-digit keys the median on the first and on the
    last rank of the key, for an even and an odd number of pairs, and (with the even cases) tied_scan, whose median lies inside a
    tied group.  The rows against the whole-cloud call, row 0 against the restatement too"""
    E = engine_mod
    ref = lattice()
    p = dict(LAT, iterations=1)
    scans = [(median_scan(zt, where, odd), bits32(zt), True) for zt in digit_heights() for where in ("first", "last")]
    if not odd:
        scans.append((tied_scan(), bits32(0.5), False))
    r = handle(E, ref)
    rs = [r, r]
    mn, mx = r.minmax()
    Q, N = r.cloud(), r.estimate_normals()
    for scan, tau, parity in scans:
        s = handle(E, scan)
        hs = [handle(E, scan, rng) for rng in LATTICE_RANGES]
        wT, wrows, wstatus, wweight, wresidual, wst = s.register_robust(r, **p)
        T, rows, statuses, weights, residuals, owneds, st = E.register_robust_tiles(hs, rs, **p)
        restated = restate_robust_terms(s.cloud(), Q, N, mn, mx, LAT["max_dist"], IDENTITY)
        brows_equal(rows, wrows); stats_equal(st, wst); assert same(T, wT)
        maps_equal(E.merge_robust_maps(statuses, weights, residuals, owneds), (wstatus, wweight, wresidual))
        n = len(scan)
        assert rows[0]["pairs"] == n and (not parity or n % 2 == (1 if odd else 0)) and rows[0]["median_bits"] == tau
        assert all(0 < int(o.sum()) < n for o in owneds)
        for f in ("pairs", "A", "b", "E", "used", "weight_sum", "median_bits", "sigma"):
            assert same(rows[0][f], restated[f]), (f, rows[0][f], restated[f])
        for e in hs + [s]:
            e.close()
    r.close()


@pytest.mark.gpu
def test_sigma_min_binds_across_the_seam(engine_mod):
    """most of the scan lies on the lattice: the merged median is 0, sigma is sigma_min = 0.25 and cs = tune sigma = 1 exactly.  A
    point at height 1 in the low tile has weight 0, the float below 1 in the high tile a weight above 0; and a cloud against itself
    in three ranges with sigma_min = 0: every weight is 1 and the loop ends converged with no step"""
    E = engine_mod
    scan = above_lattice([0.0]).copy()
    low, high = np.nonzero(scan[:, 0] < SEAM)[0], np.nonzero(scan[:, 0] >= SEAM)[0]
    at, below = np.float32(1.0), np.nextafter(np.float32(1.0), np.float32(0))
    scan[low[3:13], 2] = at
    scan[high[3:13], 2] = below
    p = dict(LAT, iterations=1, tune=4.0, sigma_min=0.25)
    (T, rows, statuses, weights, residuals, owneds, st), want = tiled_equals_whole(E, lattice(), scan, LATTICE_RANGES, **p)
    assert rows[0]["median_bits"] == 0 and rows[0]["sigma"] == 0.25 and rows[0]["pairs"] == len(scan) and rows[0]["used"] == len(scan) - 10
    assert np.all(owneds[0][low[3:13]] == 1) and np.all(owneds[1][high[3:13]] == 1)     # (the maps are the last evaluation's, behind a step)
    ref, _, _ = main_clouds()
    S, _ = cuts_of(E, ref)
    (T, rows, statuses, weights, residuals, owneds, st), _ = tiled_equals_whole(E, ref, ref, ranges3(S), sigma_min=0.0, **CENSUS)
    row = rows[0]
    assert st["steps"] == 0 and st["converged"] == 1 and len(rows) == 1 and same(T, IDENTITY)
    assert row["pairs"] >= 1000 and row["used"] == row["pairs"] and row["weight_sum"] == row["pairs"] << st["shift"]
    assert row["median_bits"] == 0 and row["sigma"] == 0.0 and not np.any(row["b"]) and row["E"] == 0 and st["rms_after"] == 0.0
    status, weight, residual = E.merge_robust_maps(statuses, weights, residuals, owneds)
    assert int((status == USED).sum()) == row["pairs"] and np.all(weight[status == USED] == 1.0) and np.all(residual[status == USED] == 0.0)


@pytest.mark.gpu
def test_few_pairs_over_the_tiles(engine_mod):
    """six pairs, three in each of two tiles, beside a tile whose owned points all lack a pair and a tile that owns nothing: at
    WIDE_TUNE all six are used and the loop takes a step neither tile could take alone; at the defaults paired is 6 but fewer
    than 6 keep a weight above zero: no step; without any pair the median and sigma are the quiet NaNs and every indexed point
    is UNPAIRED"""
    E = engine_mod
    ref, _, _ = main_clouds()
    scan, six, cuts = few_scan(E)
    p = dict(CENSUS)
    (T, rows, statuses, weights, residuals, owneds, st), _ = tiled_equals_whole(E, ref, scan, FEW_RANGES, tune=WIDE_TUNE, **p)
    assert rows[0]["pairs"] == rows[0]["used"] == 6 and st["steps"] >= 1
    assert owneds[2].sum() == 0 and owneds[0].sum() > 6 and np.all(statuses[0][owneds[0] == 1] == UNPAIRED)
    (T, rows, statuses, weights, residuals, owneds, st), _ = tiled_equals_whole(E, ref, scan, FEW_RANGES, **p)
    assert rows[0]["pairs"] == 6 and rows[0]["used"] < 6 and st["steps"] == 0 and st["converged"] == 0 and len(rows) == 1 and same(T, IDENTITY)
    assert rows[0]["locked"] == ALL_LOCKED and math.isnan(rows[0]["step2"]) and st["pairs_before"] == st["pairs_after"] == 6
    assert [int((s <= REJECTED).sum()) for s in statuses] == [0, 3, 0, 3] and sum(int((s == USED).sum()) for s in statuses) == rows[0]["used"]
    none, _ = few_pairs(0)
    S, _ = cuts_of(E, none)
    (T, rows, statuses, weights, residuals, owneds, st), _ = tiled_equals_whole(E, ref, none, ranges3(S), **p)
    assert rows[0]["pairs"] == 0 and rows[0]["used"] == 0 and rows[0]["weight_sum"] == 0 and st["steps"] == 0 and len(rows) == 1
    assert rows[0]["median_bits"] == NAN32_BITS and math.isnan(rows[0]["median_abs"]) and f64_bits(rows[0]["sigma"]) == NAN64_BITS
    assert math.isnan(st["rms_before"]) and math.isnan(st["rms_after"])
    status, weight, residual = E.merge_robust_maps(statuses, weights, residuals, owneds)
    assert np.all(status[finite_rows(none)] == UNPAIRED) and np.all(weight.view(np.uint32) == NAN32_BITS) and np.all(residual.view(np.uint64) == NAN64_BITS)


@pytest.mark.gpu
def test_robust_tiles_beyond_the_grid_cap(engine_mod):
    """large_clouds in two ranges, the first all slices but the last: its tile visits more positions than the capped grid holds
    threads, so the grid-stride loops of the kernels take a second trip and many workgroups flush into one histogram"""
    E = engine_mod
    ref, scan, _ = large_clouds()
    S, _ = cuts_of(E, scan)
    (T, rows, statuses, weights, residuals, owneds, st), _ = tiled_equals_whole(E, ref, scan, [(0, S - 1), (S - 1, S)], T0=large_T0(), **LARGE)
    past_the_grid_cap(int(owneds[0].sum()))
    assert owneds[1].sum() > 0 and st["steps"] == 2 and rows[0]["pairs"] >= 1500 and all(0 < w["used"] <= w["pairs"] for w in rows)


@pytest.mark.gpu
def test_robust_tiles_refusals(engine_mod):
    E = engine_mod
    ref, scan, moved, Tm = known_clouds()
    S, _ = cuts_of(E, moved)
    rng = ranges3(S)
    h, r = handle(E, moved, rng[1]), handle(E, ref)
    thin = handle(E, ref, (1, 3), range_margin=THIN_MARGIN)

    def refused(hs, rs, code, text, T0=None, **k):
        with pytest.raises(E.PPPError) as ex:
            E.register_robust_tiles(hs, rs, T0=T0, **dict(KNOWN, **k))
        assert ex.value.code == code and text in str(ex.value), (k, ex.value)

    # 7o's case: margin 17 mm, T shifted by 5 mm; the same margin at the identity and the same shift against the whole reference answer
    ok0 = E.register_robust_tiles([h], [thin], **dict(KNOWN, iterations=1))
    assert ok0[1][0]["pairs"] >= 6 and E.register_robust_tiles([h], [r], T0=SHIFT_5MM, **dict(KNOWN, iterations=1))[1][0]["pairs"] >= 6
    refused([h], [thin], E.ERR_CAPACITY, "range_margin", T0=SHIFT_5MM)
    refused([h], [thin], E.ERR_CAPACITY, "tile 0", T0=SHIFT_5MM)
    low = handle(E, moved, rng[0])
    refused([low, h], [r, thin], E.ERR_CAPACITY, "tile 1", T0=SHIFT_5MM)         # failed_tile names the tile that refused
    L = E.lib()
    hv, tv, rv = (ctypes.c_void_p * 1)(h.h), (ctypes.c_void_p * 1)(thin.h), (ctypes.c_void_p * 1)(r.h)
    bp = E.RobustRegistrationParams(E.RegistrationParams(KNOWN["max_dist"], KNOWN["iterations"], KNOWN["min_step"], KNOWN["lock_eps"]), 4.685, 1e-4)
    t5 = np.ascontiguousarray(SHIFT_5MM.reshape(12))
    raw = E.RegisterTilesStats()
    call = lambda hs_, rs_, n, bp_, T_=None, rows=None, cap=0: L.ppp_register_robust_tiles(hs_, rs_, n, bp_, T_, rows, cap, None, None, None, None, 0,
                                                                                            ctypes.byref(raw))
    assert call(hv, tv, 1, ctypes.byref(bp), t5.ctypes.data_as(ctypes.POINTER(ctypes.c_double))) == E.ERR_CAPACITY and raw.failed_tile == 0
    assert "range_margin" in h.L.ppp_last_error(h.h).decode()
    # the PPP_ERR_ARGs: ppp_register_robust's own, ppp_register's, ppp_register_tiles'
    for tune in (0.0, -1.0, NAN, -INF):
        refused([h], [r], E.ERR_ARG, "tune must be > 0", tune=tune)
    for sigma_min in (-1e-9, NAN, INF, -INF):
        refused([h], [r], E.ERR_ARG, "sigma_min must be finite and >= 0", sigma_min=sigma_min)
    for bad in (dict(max_dist=0.0), dict(max_dist=NAN), dict(max_dist=INF), dict(max_dist=1e30), dict(lock_eps=0.0), dict(lock_eps=1.0),
                dict(iterations=0), dict(iterations=65), dict(min_step=-1.0), dict(min_step=NAN)):
        refused([h], [r], E.ERR_ARG, "registration", **bad)
    for v in (NAN, INF):
        Tb = IDENTITY.copy(); Tb[0, 3] = v
        refused([h], [r], E.ERR_ARG, "not finite", T0=Tb)
    empty = E.Engine(0, **KW0)
    refused([h], [empty], E.ERR_ARG, "holds no cloud")
    refused([empty], [r], E.ERR_ARG, "holds no cloud")
    assert call(hv, rv, 1, None) == E.ERR_ARG and "no parameters" in h.L.ppp_last_error(h.h).decode()                    # bp NULL
    assert call(None, rv, 1, ctypes.byref(bp)) == E.ERR_ARG and call(hv, None, 1, ctypes.byref(bp)) == E.ERR_ARG
    assert call(hv, rv, 0, ctypes.byref(bp)) == E.ERR_ARG
    assert call(hv, rv, 1, ctypes.byref(bp), None, None, 3) == E.ERR_ARG and "rows is NULL" in h.L.ppp_last_error(h.h).decode()
    assert call(hv, (ctypes.c_void_p * 1)(None), 1, ctypes.byref(bp)) == E.ERR_ARG and "a NULL handle" in h.L.ppp_last_error(h.h).decode()
    refused([h, h], [r, r], E.ERR_ARG, "stands in two slots")               # a handle given twice
    over = handle(E, moved, (0, 2))
    refused([over, h], [r, r], E.ERR_ARG, "overlap")                         # ranges that overlap: the merge refuses
    # a part handle on either side
    f = finite_rows(moved)
    mn, mx = moved[f].min(axis=0), moved[f].max(axis=0)
    p = E.Engine(0, slice_begin=rng[1][0], slice_end=rng[1][1], **KW0)
    lo, hi, _ = p.range_interval(mn[0], mx[0])
    at = np.nonzero(f & (moved[:, 0] >= lo) & (moved[:, 0] <= hi))[0]
    p.set_cloud_part(moved[at], at, mn, mx, int(f.sum()), lo, hi)
    refused([p], [r], E.ERR_UNSUPPORTED, "holds a part")
    refused([h], [p], E.ERR_UNSUPPORTED, "holds a part")
    # +INFINITY is a tune; every refusal left the handles usable and the answer unchanged
    E.register_robust_tiles([h], [r], tune=INF, **dict(KNOWN, iterations=1))
    assert same(E.register_robust_tiles([h], [thin], **dict(KNOWN, iterations=1)), ok0)
    for e in (h, r, thin, low, empty, over, p):
        e.close()


@pytest.mark.gpu
def test_nothing_stored_is_touched_by_the_robust_tiles(engine_mod):
    """a deviation tile taken before and after the tiled loop is byte-equal, ppp_register_robust on whole handles -- the tiles'
    reference among them -- gives its own bits afterwards, and the clouds are as they were"""
    E = engine_mod
    ref, scan, moved, raised, Tm = dirty_clouds()
    hs, rs, everything = open_tiles(E, ref, moved, DIRTY_RANGES)
    r, s = rs[0], handle(E, moved)
    dp = dict(max_dist=3.0, smooth_radius=4.0, allowance=0.05, gain=1.0)
    before = s.register_robust(r, **DIRTY)
    dev_before = [h.deviation_tile(r, 7.0, **dp) for h in hs]
    clouds = [h.cloud().copy() for h in hs] + [r.cloud().copy()]
    first = E.register_robust_tiles(hs, rs, **DIRTY)
    assert same(E.register_robust_tiles(hs, rs, **DIRTY), first)
    assert same([h.deviation_tile(r, 7.0, **dp) for h in hs], dev_before)
    assert same(s.register_robust(r, **DIRTY), before)
    assert same([h.cloud() for h in hs] + [r.cloud()], clouds)
    assert same(E.register_tiles(hs, rs, **DIRTY)[0], s.register(r, **DIRTY)[0])                             # the other tiled loops on the same handles
    assert same(E.register_trimmed_tiles(hs, rs, keep=0.8, **DIRTY)[0], s.register_trimmed(r, keep=0.8, **DIRTY)[0])
    assert same(E.register_robust_tiles(hs, rs, **DIRTY), first)
    brows_equal(first[1], before[1])
    for e in everything + [s]:
        e.close()


@pytest.mark.gpu
def test_robust_tiles_on_two_devices(engine_mod):
    """the low tile and its reference on device 0, the others on device 1 with a reference of their own: the whole loop's bits"""
    if device_count() < 2:
        pytest.skip("needs two GPUs in one process: this machine shows %d" % device_count())
    E = engine_mod
    ref, scan, moved, raised, Tm = dirty_clouds()
    want = whole_robust(E, ref, moved, **DIRTY)
    hs, refs = [], []
    for dev, rngs in ((0, DIRTY_RANGES[:1]), (1, DIRTY_RANGES[1:])):
        r = E.Engine(dev, **KW0)
        r.set_cloud(ref)
        for b, e in rngs:
            h = E.Engine(dev, **dict(KW0, slice_begin=b, slice_end=e))
            h.set_cloud(moved)
            hs.append(h); refs.append(r)
    T, rows, statuses, weights, residuals, owneds, st = E.register_robust_tiles(hs, refs, **DIRTY)
    brows_equal(rows, want[1]); stats_equal(st, want[5]); assert same(T, want[0])
    maps_equal(E.merge_robust_maps(statuses, weights, residuals, owneds), want[2:5])
    with pytest.raises(E.PPPError) as ex:                                    # a tile and its reference on different devices
        E.register_robust_tiles(hs, [refs[0]] * 3, **DIRTY)
    assert ex.value.code == E.ERR_ARG and "tile 1" in str(ex.value)
    for e in hs + [refs[0], refs[-1]]:
        e.close()
