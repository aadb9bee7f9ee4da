"""Trimmed registration of a scan held as slice-range tiles (ppp_trim_select, ppp_trim_rank, ppp_register_trimmed_tiles;
DESIGN.md 7p and B.95-B.100).

Every comparison is for equality.  Pairs and keys are a point's own, the cut is a rank statistic of the union of the keys --
found on histograms that add bin by bin -- and the 29 words add as integers: for ranges that tile the walk the tiled loop must
be ppp_register_trimmed's T, rows (words, kept, locked, step2, paired, trim_d2), statistics and maps on whole-cloud handles,
bit for bit.  No tolerance appears anywhere in this file.

The clouds are test_trimmed_registration's: dirty_clouds (5 slices, cut into [0, 1), [1, 3), [3, 5) as test_registration_tiles
cuts the known motion; the raised eighth lies below x = 60, inside the two low tiles), the lattice with tie_scan and
digit_heights above it (3 slices, cut into [0, 2), [2, 3): the seam at x = 57.125 runs through the scan), the main scan with
all but a few points lifted out of reach, and large_clouds past the grid cap."""
import ctypes
import math
import os

import numpy as np
import pytest

from test_deviation import KW0, large_clouds, main_clouds, past_the_grid_cap
from test_deviation_tiles import cuts_of, device_count, finite_rows, handle, ranges3
from test_path_dwell import same
from test_registration import ALL_LOCKED, CENSUS, IDENTITY, KNOWN, LARGE, NAN, box_centre, known_clouds, large_T0, oracle_normals, rows_equal, stats_equal
from test_registration_tiles import (SHIFT_5MM, THIN_MARGIN, indexed_interval, moved_x, open_tiles, owned_rows, reach_of, refusing)
from test_trimmed_registration import (DIRTY, DROPPED, KEPT, NAN32_BITS, TIES, TRIMMED, UNPAIRED, above_lattice, digit_heights, digit_sweep,
                                       dirty_clouds, dirty_restated_cpu, few_pairs, lattice, maps_equal, restate_trimmed_terms, tie_scan, trim_rank,
                                       trows_equal)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
FUNC_DECLS = ("int    ppp_trim_select(const unsigned int *hist, size_t bins, size_t rank, unsigned int *bin, size_t *rank_in_bin);",
              "size_t ppp_trim_rank(double keep, size_t paired);",
              "int    ppp_register_trimmed_tiles(const ppp_handle *hs, const ppp_handle *refs, size_t count,\n"
              "                                  const ppp_trimmed_registration_params *tp, const double *T0_12,\n"
              "                                  ppp_trimmed_registration_row *rows, size_t row_cap,\n"
              "                                  unsigned char *const *status, float *const *d2, unsigned char *const *owned, size_t cap,\n"
              "                                  ppp_register_tiles_stats *stats);")
SYMBOLS = ("ppp_trim_select", "ppp_trim_rank", "ppp_register_trimmed_tiles")
DIRTY_RANGES = [(0, 1), (1, 3), (3, 5)]
LATTICE_RANGES = [(0, 2), (2, 3)]
TIE_HEIGHTS = np.array([0.5, 1.0], np.float32)                               # tie_scan() is above_lattice(TIE_HEIGHTS)
KEEP = 0.8


# ---------------------------------------------------------------- CPU: header, ABI, the two host calls


def test_header_declares_and_engine_exports_the_trimmed_tiles(engine_mod):
    hdr = open(os.path.join(ROOT, "include", "ppp_hip.h")).read()
    for decl in FUNC_DECLS:
        assert decl in hdr, decl
    at = [hdr.index("int ppp_register_tiles(")] + [hdr.index(d) for d in FUNC_DECLS] + [hdr.index("int ppp_eval_spline(")]
    assert at == sorted(at)
    assert "DESIGN.md 7p, B.95-B.100" in hdr and "never a tile's own\n   count" in hdr
    for sym in SYMBOLS:
        assert sym in engine_mod.EXPORTS and hasattr(engine_mod.lib(), sym), sym
    assert callable(engine_mod.Engine.register_trimmed_tiles)
    for f in ("register_trimmed_tiles", "trim_select", "trim_rank", "merge_trimmed_maps"):
        assert callable(getattr(engine_mod, f)), f
    planner = open(os.path.join(ROOT, "include", "ppp_planner.hpp")).read()
    assert "inline bool register_trimmed_tiles(std::vector<Planner *> &tiles, std::vector<Planner *> &refs, ppp_register_tiles_stats &st," in planner
    mk = open(os.path.join(ROOT, "polishpathplanning_amd", "csrc", "Makefile")).read()
    assert "ppp_trimmed_tile.h" in [l for l in mk.splitlines() if l.startswith("SCAN_HDR")][0]


def select_restated(hist, rank):
    """the selection rule in numpy: the first bin whose running count reaches rank (1-based), and the rank inside it"""
    run = np.cumsum(np.asarray(hist, np.int64))
    if rank < 1 or not len(run) or rank > run[-1]:
        return 0, 0
    b = int(np.nonzero(run >= rank)[0][0])
    return b, int(rank - (run[b] - hist[b]))


def test_trim_select_against_the_restatement(engine_mod):
    E = engine_mod
    hist = np.zeros(2048, np.uint32)
    hist[[5, 6, 900, 2047]] = (3, 1, 40000, 7)                               # empty bins in front, between and a last bin in use
    total = int(hist.sum())
    want = {1: (5, 1), 3: (5, 3), 4: (6, 1), 5: (900, 1), 40004: (900, 40000), 40005: (2047, 1), total: (2047, 7), 0: (0, 0), total + 1: (0, 0),
            2 ** 40: (0, 0)}
    for rank, w in want.items():
        assert E.trim_select(hist, rank) == w == select_restated(hist, rank), rank
    rs = np.random.RandomState(7)
    for bins in (1, 10, 1024, 2048):
        h = (rs.randint(0, 5, bins) * (rs.rand(bins) < 0.3)).astype(np.uint32)
        for rank in range(0, int(h.sum()) + 2):
            assert E.trim_select(h, rank) == select_restated(h, rank), (bins, rank)
    big = np.array([0xFFFFFFFF, 0xFFFFFFFF, 5], np.uint32)                   # the running count is wider than a bin
    assert E.trim_select(big, 2 ** 32) == (1, 1) and E.trim_select(big, 2 ** 33 - 1) == (2, 1) and E.trim_select(big, 2 ** 33 + 4) == (0, 0)
    assert E.trim_select(np.zeros(0, np.uint32), 1) == (0, 0)
    L = E.lib()
    b, r = ctypes.c_uint(), ctypes.c_size_t()
    hp = hist.ctypes.data_as(ctypes.POINTER(ctypes.c_uint))
    assert L.ppp_trim_select(None, 2048, 1, ctypes.byref(b), ctypes.byref(r)) == E.ERR_ARG
    assert L.ppp_trim_select(hp, 2048, 1, None, ctypes.byref(r)) == E.ERR_ARG
    assert L.ppp_trim_select(hp, 2048, 1, ctypes.byref(b), None) == E.ERR_ARG


def test_trim_rank_against_the_restatement(engine_mod):
    E = engine_mod
    cases = [(0.5, 4), (0.25, 8), (0.8, 5), (0.75, 3520),                    # keep * paired an exact integer
             (1.0, 1), (1.0, 7), (1.0, 10 ** 7), (0.8, 0), (1.0, 0),         # keep = 1; paired = 0
             (0.8, 7), (0.8, 6), (1e-9, 4), (0.1, 3), (np.nextafter(1.0, 0.0), 10 ** 7), (0.8, 3520), (0.3, 10)]
    for keep, paired in cases:
        assert E.trim_rank(keep, paired) == trim_rank(keep, paired), (keep, paired)
    assert (E.trim_rank(0.5, 4), E.trim_rank(0.8, 5), E.trim_rank(1.0, 7), E.trim_rank(0.8, 0), E.trim_rank(1e-9, 4)) == (2, 4, 7, 0, 1)
    rs = np.random.RandomState(3)
    for keep, paired in zip(rs.rand(300), rs.randint(0, 10 ** 6, 300)):
        assert E.trim_rank(keep, int(paired)) == trim_rank(keep, int(paired))


def test_merge_trimmed_maps(engine_mod):
    E = engine_mod
    nan = np.float32(np.nan)
    s0, d0, o0 = np.array([KEPT, DROPPED, DROPPED, DROPPED], np.uint8), np.array([0.5, nan, nan, nan], np.float32), np.array([1, 0, 0, 0], np.uint8)
    s1, d1, o1 = np.array([DROPPED, TRIMMED, UNPAIRED, DROPPED], np.uint8), np.array([nan, 2.0, nan, nan], np.float32), np.array([0, 1, 1, 0], np.uint8)
    status, d2 = E.merge_trimmed_maps([s0, s1], [d0, d1], [o0, o1])
    assert status.tolist() == [KEPT, TRIMMED, UNPAIRED, DROPPED] and d2.view(np.uint32).tolist() == [0x3F000000, 0x40000000, NAN32_BITS, NAN32_BITS]
    for bad in (([s0, s0], [d0, d0], [o0, o0]), ([], [], []), ([s0, s1[:3]], [d0, d1[:3]], [o0, o1[:3]])):
        with pytest.raises(E.PPPError) as ex:
            E.merge_trimmed_maps(*bad)
        assert ex.value.code == E.ERR_ARG


# ---------------------------------------------------------------- CPU: the census of the GPU cases, by restatement


def test_census_of_the_tiled_contaminated_case(engine_mod):
    """(a) dirty_clouds in DIRTY_RANGES, the oracle's normals, at the identity and at the chain's second transform: every tile
    owns pairs, the raised eighth lies in the two low tiles only, and every tile's own k-th key differs from the merged tau -- a
    cut taken per tile would be caught; (c) for every transform of the chain every moved owned query's reach lies inside what
    the reference's matching default range handle indexes (B.89)"""
    E = engine_mod
    ref, scan, moved, raised, Tm = dirty_clouds()
    T, rows, status, d2, st = dirty_restated_cpu(KEEP)
    S, cuts = cuts_of(E, moved)
    Sr, rcuts = cuts_of(E, ref)
    assert S == Sr == 5 and ranges3(S) == ranges3(Sr) == DIRTY_RANGES and st["steps"] >= 3
    assert not owned_rows(moved, cuts, DIRTY_RANGES[2])[raised].any() and all(owned_rows(moved, cuts, r)[raised].any() for r in DIRTY_RANGES[:2])
    assert sum(int(owned_rows(moved, cuts, r).sum()) for r in DIRTY_RANGES) == st["indexed"] == len(moved)
    for name, row in (("identity", rows[0]), ("second", rows[1])):
        assert name != "identity" or same(row["T"], IDENTITY)
        keys, pair = row["d2"].view(np.uint32), row["partner"] >= 0
        assert row["k"] == trim_rank(KEEP, row["paired"]) and row["pairs"] < row["paired"]
        for r in DIRTY_RANGES:
            mine = np.sort(keys[owned_rows(moved, cuts, r) & pair])
            own_tau = int(mine[trim_rank(KEEP, len(mine)) - 1])
            print("%s tile %r: %d pairs, own cut %#x, merged cut %#x" % (name, r, len(mine), own_tau, row["trim_bits"]))
            assert len(mine) >= 6 and own_tau != row["trim_bits"]
    mn, mx, _ = box_centre(ref)
    reach = reach_of(DIRTY["max_dist"])
    for k, row in enumerate(rows):
        for r in DIRTY_RANGES:
            lo, hi = indexed_interval(E, ref, r)
            assert not refusing(moved_x(row["T"], moved[owned_rows(moved, cuts, r)]), lo, hi, mn[0], mx[0], reach).any(), (k, r)


def test_census_of_the_tiled_lattice_cases(engine_mod):
    """(b) the lattice scans in LATTICE_RANGES: both tiles own points of every tied key, and of every key of the digit case -- so
    the keys that share a top digit, and those that share the middle digit too, are counted by both tiles, and every bin the
    selection walks is fed from both sides of the seam"""
    E = engine_mod
    for zs in (TIE_HEIGHTS, digit_heights()):
        scan = above_lattice(zs)
        S, cuts = cuts_of(E, scan)
        assert S == 3 and cuts_of(E, lattice())[0] == 3 and cuts[2] == np.float32(57.125)
        keys = (scan[:, 2] * scan[:, 2]).view(np.uint32)
        sides = [owned_rows(scan, cuts, r) for r in LATTICE_RANGES]
        assert sides[0].sum() + sides[1].sum() == len(scan) and min(sides[0].sum(), sides[1].sum()) >= 100
        for key in np.unique(keys):
            assert all(int((keys[s] == key).sum()) >= 2 for s in sides), hex(int(key))
    assert np.array_equal(tie_scan(), above_lattice(TIE_HEIGHTS))
    one = tie_scan(1)                                                        # the lifted point: the tie at 1.0 gains a pair below the seam
    assert owned_rows(one, cuts_of(E, one)[1], LATTICE_RANGES[0])[np.nonzero(one[:, 2] != tie_scan()[:, 2])[0]].all()


def few_scan(E):
    """the main scan with six pairs, three on either side of cut(3); the rows of slice 3's owned interval taken out (the walk
    stays): in FEW_RANGES tile 0 owns points that all lack a pair, tiles 1 and 3 own three pairs each, tile 2 owns nothing"""
    scan, keep_at = few_pairs(6)
    S, cuts = cuts_of(E, scan)
    x = scan[:, 0]
    gap = (x >= cuts[3]) & (x < cuts[4])
    assert not gap[keep_at].any()
    out = scan[~gap]
    assert cuts_of(E, out)[1].tobytes() == cuts.tobytes()
    return out, scan[keep_at], cuts


FEW_RANGES = [(0, 1), (1, 3), (3, 4), (4, 7)]


def test_census_of_the_few_pairs_case(engine_mod):
    scan, six, cuts = few_scan(engine_mod)
    per = [int(((six[:, 0] >= cuts[b]) & (six[:, 0] < cuts[e])).sum()) for b, e in FEW_RANGES]
    owned = [int(owned_rows(scan, cuts, r).sum()) for r in FEW_RANGES]
    print("six pairs per tile %r, owned %r" % (per, owned))
    assert per == [0, 3, 0, 3] and owned[2] == 0 and min(owned[0], owned[1], owned[3]) > 6 and sum(owned) == len(scan)
    assert trim_rank(1.0, 6) == 6 and trim_rank(KEEP, 6) == 5


# ---------------------------------------------------------------- GPU


def whole_trimmed(E, ref, scan, **kw):
    r, s = handle(E, ref), handle(E, scan)
    out = s.register_trimmed(r, **kw)
    r.close(); s.close()
    return out


def tiled_equals_whole(E, ref, scan, ranges, ref_ranges=None, whole=None, **kw):
    """Engine.register_trimmed_tiles on `ranges` against Engine.register_trimmed on whole-cloud handles: T, rows, statistics, the
    merged maps; every tile's owned map is the cut's, the owned maps partition the finite points, and what a tile does not own
    keeps the fill.  Returns (the tiled answer, the whole one)"""
    want = whole_trimmed(E, ref, scan, **kw) if whole is None else whole
    hs, rs, everything = open_tiles(E, ref, scan, ranges, ref_ranges)
    got = E.register_trimmed_tiles(hs, rs, **kw)
    for e in everything:
        e.close()
    T, rows, statuses, d2s, owneds, st = got
    wT, wrows, wstatus, wd2, wst = want
    print("steps %d (whole %d) kept %r paired %r cut %r" % (st["steps"], wst["steps"], [w["pairs"] for w in rows], [w["paired"] for w in rows],
                                                              [hex(w["trim_bits"]) for w in rows]))
    trows_equal(rows, wrows); stats_equal(st, wst)
    assert same(T, wT) and same(T, rows[-1]["T"])
    _, cuts = cuts_of(E, scan)
    for r, status, d2, owned in zip(ranges, statuses, d2s, owneds):
        assert owned.dtype == np.uint8 and np.array_equal(owned == 1, owned_rows(scan, cuts, r)) and set(np.unique(owned)) <= {0, 1}
        assert np.all(status[owned == 0] == DROPPED) and np.all(d2[owned == 0].view(np.uint32) == NAN32_BITS)
        maps_equal(status[owned == 1], d2[owned == 1], wstatus[owned == 1], wd2[owned == 1])
    assert np.array_equal(np.sum(owneds, axis=0), finite_rows(scan).astype(np.int64))
    maps_equal(*E.merge_trimmed_maps(statuses, d2s, owneds), wstatus, wd2)
    return got, want


@pytest.mark.gpu
@pytest.mark.parametrize("ref_ranged", [False, True])
def test_tiled_trimmed_loop_equals_the_whole_loop(engine_mod, ref_ranged):
    """dirty_clouds at keep 0.8 in three ranges, the reference whole or in its own three default ranges; fresh handles give the
    same bits; iterations used up and a row_cap below the number of rows"""
    E = engine_mod
    ref, scan, moved, raised, Tm = dirty_clouds()
    ref_ranges = DIRTY_RANGES if ref_ranged else None
    got, want = tiled_equals_whole(E, ref, moved, DIRTY_RANGES, ref_ranges, keep=KEEP, **DIRTY)
    T, rows, statuses, d2s, owneds, st = got
    assert st["converged"] == 1 and st["steps"] >= 3 and all(w["pairs"] < w["paired"] for w in rows)
    status, _ = E.merge_trimmed_maps(statuses, d2s, owneds)
    assert np.all((status[raised] == TRIMMED) | (status[raised] == UNPAIRED)) and np.any(status == TRIMMED)
    again, _ = tiled_equals_whole(E, ref, moved, DIRTY_RANGES, ref_ranges, whole=want, keep=KEEP, **DIRTY)     # fresh handles
    assert same(again, got)
    two = dict(DIRTY, iterations=2)
    g2, w2 = tiled_equals_whole(E, ref, moved, DIRTY_RANGES, ref_ranges, keep=KEEP, **two)
    assert g2[5]["steps"] == 2 and g2[5]["converged"] == 0 and len(g2[1]) == 3
    # the C call: row_cap 2 of more rows, untouched memory behind them; some maps asked for, some not; everything optional
    hs, rs, everything = open_tiles(E, ref, moved, DIRTY_RANGES, ref_ranges)
    k, n = len(hs), len(moved)
    hv = (ctypes.c_void_p * k)(*[h.h for h in hs]); rv = (ctypes.c_void_p * k)(*[r.h for r in rs])
    tp = E.TrimmedRegistrationParams(E.RegistrationParams(DIRTY["max_dist"], DIRTY["iterations"], DIRTY["min_step"], DIRTY["lock_eps"]), KEEP)
    buf = (E.TrimmedRegistrationRow * 4)()
    size = ctypes.sizeof(E.TrimmedRegistrationRow)
    ctypes.memset(buf, 0xA5, 4 * size)
    raw = E.RegisterTilesStats()
    ub, fp = ctypes.POINTER(ctypes.c_ubyte), ctypes.POINTER(ctypes.c_float)
    s1, o2 = np.full(n, 0xA5, np.uint8), np.full(n, 0xA5, np.uint8)
    sv = (ub * k)(None, s1.ctypes.data_as(ub), None); ov = (ub * k)(None, None, o2.ctypes.data_as(ub))
    L = E.lib()
    half = n // 2
    assert L.ppp_register_trimmed_tiles(hv, rv, k, ctypes.byref(tp), None, buf, 2, sv, None, ov, half, ctypes.byref(raw)) == 0 and raw.failed_tile == -1
    trows_equal([E._trimmed_registration_row(buf[0]), E._trimmed_registration_row(buf[1])], want[1][:2])
    stats_equal(E._registration_stats(raw.reg), want[4])
    assert ctypes.string_at(ctypes.addressof(buf) + 2 * size, 2 * size) == b"\xa5" * (2 * size)
    assert np.array_equal(s1[:half], statuses[1][:half]) and np.array_equal(o2[:half], owneds[2][:half])      # the first min(cap, n) entries
    assert np.all(s1[half:] == 0xA5) and np.all(o2[half:] == 0xA5)
    assert L.ppp_register_trimmed_tiles(hv, rv, k, ctypes.byref(tp), None, None, 0, None, None, None, 0, None) == 0
    for e in everything:
        e.close()


@pytest.mark.gpu
def test_keep_one_is_the_tiled_register(engine_mod):
    """keep = 1 on the known motion: the rows' words, T and the statistics are ppp_register_tiles', and so ppp_register's"""
    E = engine_mod
    ref, scan, moved, Tm = known_clouds()
    S, _ = cuts_of(E, moved)
    hs, rs, everything = open_tiles(E, ref, moved, ranges3(S))
    T, rows, st = E.register_tiles(hs, rs, **KNOWN)
    tT, trows, statuses, d2s, owneds, tst = E.register_trimmed_tiles(hs, rs, keep=1.0, **KNOWN)
    wT, wrows, wst = handle_register(E, ref, moved)
    for e in everything:
        e.close()
    assert st["steps"] >= 3
    rows_equal(trows, rows); stats_equal(tst, st); assert same(tT, T)
    rows_equal(trows, wrows); stats_equal(tst, wst); assert same(tT, wT)
    status, d2 = E.merge_trimmed_maps(statuses, d2s, owneds)
    assert all(w["paired"] == w["pairs"] for w in trows) and not np.any(status == TRIMMED) and int((status == KEPT).sum()) == trows[-1]["pairs"]
    assert trows[-1]["trim_bits"] == int(d2[status == KEPT].max().view(np.uint32))


def handle_register(E, ref, scan):
    r, s = handle(E, ref), handle(E, scan)
    out = s.register(r, **KNOWN)
    r.close(); s.close()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["ties", "ties_one_lifted", "digits"])
def test_ties_and_digits_across_the_seam(engine_mod, case):
    """the lattice in two ranges.  For every distinct key a share that puts k on its first and one that puts k on its last pair:
    in the tie cases k lands on the first and on the last pair of a tie that spans the seam, in the digit case the k-th key sits
    in low-digit bins and in middle-digit bins that both tiles feed.  Row 0 against the whole-cloud call and the restatement"""
    E = engine_mod
    ref = lattice()
    zs = TIE_HEIGHTS if case != "digits" else digit_heights()
    scan = tie_scan(1) if case == "ties_one_lifted" else above_lattice(zs)
    n = len(scan)
    sweep = digit_sweep(n, zs) if case != "ties_one_lifted" else [((k - 0.5) / n, None) for k in (1, n // 2 - 1, n // 2, n)]
    assert [trim_rank(keep, n) for keep, _ in sweep][-1] == n and (case != "ties_one_lifted" or [trim_rank(keep, n) for keep, _ in sweep] == [1, n // 2 - 1, n // 2, n])
    hs, rs, everything = open_tiles(E, ref, scan, LATTICE_RANGES)
    r, s = handle(E, ref), handle(E, scan)
    mn, mx = r.minmax()
    Q, N, P = r.cloud(), r.estimate_normals(), s.cloud()
    seen = set()
    for keep, tau in sweep:
        wT, wrows, wstatus, wd2, wst = s.register_trimmed(r, keep=keep, **TIES)
        T, rows, statuses, d2s, owneds, st = E.register_trimmed_tiles(hs, rs, keep=keep, **TIES)
        restated = restate_trimmed_terms(P, Q, N, mn, mx, TIES["max_dist"], IDENTITY, keep)
        trows_equal(rows, wrows); stats_equal(st, wst); assert same(T, wT)
        maps_equal(*E.merge_trimmed_maps(statuses, d2s, owneds), wstatus, wd2)
        assert rows[0]["paired"] == n and (tau is None or rows[0]["trim_bits"] == tau)
        for f in ("pairs", "A", "b", "E", "paired", "trim_bits"):
            assert same(rows[0][f], restated[f]), (keep, f)
        seen.add((trim_rank(keep, n), rows[0]["trim_bits"], rows[0]["pairs"]))
    print(sorted(seen))
    if case == "ties":                                                       # k = 1, n / 2: the tie at 0.25; k = n / 2 + 1, n: the tie at 1.0
        lo, hi = int(np.float32(0.25).view(np.uint32)), int(np.float32(1.0).view(np.uint32))
        assert seen == {(1, lo, n // 2), (n // 2, lo, n // 2), (n // 2 + 1, hi, n), (n, hi, n)}
    if case == "ties_one_lifted":                                            # the tie at 1.0 begins one rank earlier
        lo, hi = int(np.float32(0.25).view(np.uint32)), int(np.float32(1.0).view(np.uint32))
        assert seen == {(1, lo, n // 2 - 1), (n // 2 - 1, lo, n // 2 - 1), (n // 2, hi, n), (n, hi, n)}
    for e in everything + [r, s]:
        e.close()


@pytest.mark.gpu
def test_few_pairs_over_the_tiles(engine_mod):
    """six pairs, three in each of two tiles, beside a tile whose owned points all lack a pair and a tile that owns nothing:
    keep 1 keeps six and takes a step neither tile could take alone; keep 0.8 keeps five: no step; without any pair trim_d2 is
    the quiet NaN and every indexed point UNPAIRED"""
    E = engine_mod
    ref, _, _ = main_clouds()
    scan, six, cuts = few_scan(E)
    p = dict(CENSUS)
    (T, rows, statuses, d2s, owneds, st), _ = tiled_equals_whole(E, ref, scan, FEW_RANGES, keep=1.0, **p)
    assert rows[0]["paired"] == rows[0]["pairs"] == 6 and st["steps"] >= 1
    assert owneds[2].sum() == 0 and owneds[0].sum() > 6 and np.all(statuses[0][owneds[0] == 1] == UNPAIRED)
    (T, rows, statuses, d2s, owneds, st), _ = tiled_equals_whole(E, ref, scan, FEW_RANGES, keep=KEEP, **p)
    assert rows[0]["paired"] == 6 and rows[0]["pairs"] == 5 and st["steps"] == 0 and st["converged"] == 0 and len(rows) == 1 and same(T, IDENTITY)
    assert rows[0]["locked"] == ALL_LOCKED and math.isnan(rows[0]["step2"])
    assert [int((s == KEPT).sum()) + int((s == TRIMMED).sum()) for s in statuses] == [0, 3, 0, 3]
    none, _ = few_pairs(0)
    S, _ = cuts_of(E, none)
    (T, rows, statuses, d2s, owneds, st), _ = tiled_equals_whole(E, ref, none, ranges3(S), keep=KEEP, **p)
    assert rows[0]["paired"] == 0 and rows[0]["pairs"] == 0 and rows[0]["trim_bits"] == NAN32_BITS and math.isnan(rows[0]["trim_d2"]) and st["steps"] == 0
    status, d2 = E.merge_trimmed_maps(statuses, d2s, owneds)
    assert np.all(status[finite_rows(none)] == UNPAIRED) and np.all(d2.view(np.uint32) == NAN32_BITS)


@pytest.mark.gpu
def test_trimmed_tiles_beyond_the_grid_cap(engine_mod):
    """large_clouds in two ranges, the first all slices but the last: its tile visits more positions than the capped grid holds
    threads, so the grid-stride loops of the four kernels take a second trip and many workgroups flush into one histogram"""
    E = engine_mod
    ref, scan, _ = large_clouds()
    S, _ = cuts_of(E, scan)
    (T, rows, statuses, d2s, owneds, st), _ = tiled_equals_whole(E, ref, scan, [(0, S - 1), (S - 1, S)], T0=large_T0(), keep=KEEP, **LARGE)
    past_the_grid_cap(int(owneds[0].sum()))
    assert owneds[1].sum() > 0 and st["steps"] == 2 and rows[0]["paired"] >= 1500 and all(w["pairs"] < w["paired"] for w in rows)


@pytest.mark.gpu
def test_trimmed_tiles_refusals(engine_mod):
    E = engine_mod
    ref, scan, moved, Tm = known_clouds()
    S, _ = cuts_of(E, moved)
    rng = ranges3(S)
    h, r = handle(E, moved, rng[1]), handle(E, ref)
    thin = handle(E, ref, (1, 3), range_margin=THIN_MARGIN)

    def refused(hs, rs, code, text, T0=None, keep=KEEP, **k):
        with pytest.raises(E.PPPError) as ex:
            E.register_trimmed_tiles(hs, rs, keep=keep, T0=T0, **dict(KNOWN, **k))
        assert ex.value.code == code and text in str(ex.value), (k, ex.value)

    # §7o's case: margin 17 mm, T shifted by 5 mm; the same margin at the identity and the same shift against the whole reference answer
    ok0 = E.register_trimmed_tiles([h], [thin], keep=KEEP, **dict(KNOWN, iterations=1))
    assert ok0[1][0]["paired"] >= 6 and E.register_trimmed_tiles([h], [r], keep=KEEP, T0=SHIFT_5MM, **dict(KNOWN, iterations=1))[1][0]["paired"] >= 6
    refused([h], [thin], E.ERR_CAPACITY, "range_margin", T0=SHIFT_5MM)
    refused([h], [thin], E.ERR_CAPACITY, "tile 0", T0=SHIFT_5MM)
    low = handle(E, moved, rng[0])
    refused([low, h], [r, thin], E.ERR_CAPACITY, "tile 1", T0=SHIFT_5MM)         # failed_tile names the tile that refused
    L = E.lib()
    hv, tv, rv = (ctypes.c_void_p * 1)(h.h), (ctypes.c_void_p * 1)(thin.h), (ctypes.c_void_p * 1)(r.h)
    tp = E.TrimmedRegistrationParams(E.RegistrationParams(KNOWN["max_dist"], KNOWN["iterations"], KNOWN["min_step"], KNOWN["lock_eps"]), KEEP)
    t5 = np.ascontiguousarray(SHIFT_5MM.reshape(12))
    raw = E.RegisterTilesStats()
    call = lambda hs_, rs_, n, tp_, T_=None, rows=None, cap=0: L.ppp_register_trimmed_tiles(hs_, rs_, n, tp_, T_, rows, cap, None, None, None, 0, ctypes.byref(raw))
    assert call(hv, tv, 1, ctypes.byref(tp), t5.ctypes.data_as(ctypes.POINTER(ctypes.c_double))) == E.ERR_CAPACITY and raw.failed_tile == 0
    # the PPP_ERR_ARGs: ppp_register_trimmed's own, ppp_register's, ppp_register_tiles'
    for keep in (0.0, -0.5, 1.0000001, NAN, INF):
        refused([h], [r], E.ERR_ARG, "keep must be in (0, 1]", keep=keep)
    for bad in (dict(max_dist=0.0), dict(max_dist=NAN), dict(max_dist=INF), dict(max_dist=1e30), dict(lock_eps=0.0), dict(lock_eps=1.0),
                dict(iterations=0), dict(iterations=65), dict(min_step=-1.0), dict(min_step=NAN)):
        refused([h], [r], E.ERR_ARG, "registration", **bad)
    for v in (NAN, INF):
        Tb = IDENTITY.copy(); Tb[0, 3] = v
        refused([h], [r], E.ERR_ARG, "not finite", T0=Tb)
    empty = E.Engine(0, **KW0)
    refused([h], [empty], E.ERR_ARG, "holds no cloud")
    refused([empty], [r], E.ERR_ARG, "holds no cloud")
    assert call(hv, rv, 1, None) == E.ERR_ARG and "no parameters" in h.L.ppp_last_error(h.h).decode()
    assert call(None, rv, 1, ctypes.byref(tp)) == E.ERR_ARG and call(hv, None, 1, ctypes.byref(tp)) == E.ERR_ARG
    assert call(hv, rv, 0, ctypes.byref(tp)) == E.ERR_ARG
    assert call(hv, rv, 1, ctypes.byref(tp), None, None, 3) == E.ERR_ARG and "rows is NULL" in h.L.ppp_last_error(h.h).decode()
    assert call(hv, (ctypes.c_void_p * 1)(None), 1, ctypes.byref(tp)) == E.ERR_ARG and "a NULL handle" in h.L.ppp_last_error(h.h).decode()
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
    # every refusal left the handles usable and the answer unchanged
    assert same(E.register_trimmed_tiles([h], [thin], keep=KEEP, **dict(KNOWN, iterations=1)), ok0)
    for e in (h, r, thin, low, empty, over, p):
        e.close()


@pytest.mark.gpu
def test_nothing_stored_is_touched_by_the_trimmed_tiles(engine_mod):
    """a deviation tile taken before and after the tiled loop is byte-equal, ppp_register_trimmed on whole handles -- the tiles'
    reference among them -- gives its own bits afterwards, and the clouds are as they were"""
    E = engine_mod
    ref, scan, moved, raised, Tm = dirty_clouds()
    hs, rs, everything = open_tiles(E, ref, moved, DIRTY_RANGES)
    r, s = rs[0], handle(E, moved)
    dp = dict(max_dist=3.0, smooth_radius=4.0, allowance=0.05, gain=1.0)
    before = s.register_trimmed(r, keep=KEEP, **DIRTY)
    dev_before = [h.deviation_tile(r, 7.0, **dp) for h in hs]
    clouds = [h.cloud().copy() for h in hs] + [r.cloud().copy()]
    first = E.register_trimmed_tiles(hs, rs, keep=KEEP, **DIRTY)
    assert same(E.register_trimmed_tiles(hs, rs, keep=KEEP, **DIRTY), first)
    assert same([h.deviation_tile(r, 7.0, **dp) for h in hs], dev_before)
    assert same(s.register_trimmed(r, keep=KEEP, **DIRTY), before)
    assert same([h.cloud() for h in hs] + [r.cloud()], clouds)
    assert same(E.register_tiles(hs, rs, **DIRTY)[0], s.register(r, **DIRTY)[0])                             # the untrimmed tiled loop on the same handles
    trows_equal(first[1], before[1])
    for e in everything + [s]:
        e.close()


@pytest.mark.gpu
def test_trimmed_tiles_on_two_devices(engine_mod):
    """the low tile and its reference on device 0, the others on device 1 with a reference of their own: the whole loop's bits"""
    if device_count() < 2:
        pytest.skip("needs two GPUs in one process: this machine shows %d" % device_count())
    E = engine_mod
    ref, scan, moved, raised, Tm = dirty_clouds()
    want = whole_trimmed(E, ref, moved, keep=KEEP, **DIRTY)
    hs, refs = [], []
    for dev, rngs in ((0, DIRTY_RANGES[:1]), (1, DIRTY_RANGES[1:])):
        r = E.Engine(dev, **KW0)
        r.set_cloud(ref)
        for b, e in rngs:
            h = E.Engine(dev, **dict(KW0, slice_begin=b, slice_end=e))
            h.set_cloud(moved)
            hs.append(h); refs.append(r)
    T, rows, statuses, d2s, owneds, st = E.register_trimmed_tiles(hs, refs, keep=KEEP, **DIRTY)
    trows_equal(rows, want[1]); stats_equal(st, want[4]); assert same(T, want[0])
    maps_equal(*E.merge_trimmed_maps(statuses, d2s, owneds), want[2], want[3])
    with pytest.raises(E.PPPError) as ex:                                    # a tile and its reference on different devices
        E.register_trimmed_tiles(hs, [refs[0]] * 3, keep=KEEP, **DIRTY)
    assert ex.value.code == E.ERR_ARG and "tile 1" in str(ex.value)
    for e in hs + [refs[0], refs[-1]]:
        e.close()
