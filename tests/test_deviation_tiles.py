"""The deviation map tiled over slice ranges (ppp_get_deviation_tile, ppp_merge_deviation_tiles).

Every comparison is for equality: a tile's five maps against ppp_get_deviation on whole-cloud handles by bytes over the owned
points, the merged statistics against the whole-cloud statistics field for field by bits -- rms_dev and target_sum included: the
merge adds them in the whole-cloud call's own fixed order (fixed_order_sum below restates that order in numpy).  The one bound is
test_deviation's n * 2^-52 (relative) of those two sums against math.fsum, in the CPU test that feeds the merge with the numpy
restatement, whose own rms_dev and target_sum come from fsum.

The clouds are test_deviation's main_clouds (7 slices of the default walk, cut into [0, 2), [2, 5), [5, 7): the middle tile is
interior, with a seam at x = 53 and one at x = 125) and seam_clouds below: the same two clouds with two exact ties and a pair at
exactly max_dist laid across the seam at 53.  range_margin is the default 24 mm: a range indexes from int(px[sb]) - 2 - 24, and
the cut lies half a step (12 mm) below px[sb], which leaves 14 mm of room for halo + normal_radius = 8.5 mm (asserted in the
census)."""
import ctypes
import functools
import math
import os
import subprocess

import numpy as np
import pytest

from polishpathplanning_amd import synth
from polishpathplanning_amd.robot_path import slice_ranges
from test_contact_tiles import RANGE_MARGIN, host_cuts
from test_deviation import (DROPPED, F24, INF, KW0, MAIN, MAPS, MATCHED, NO_NORMAL, SMOOTH, STATS_FIELDS, TOO_FAR, bumped, d2_table,
                            large_clouds, main_clouds, main_restated_cpu, past_the_grid_cap, restate_deviation, same)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NORMAL_RADIUS = 2.5                          # ppp_default_params
HALO = MAIN["max_dist"] + SMOOTH             # 6 mm: the least the call accepts with smoothing
NAN_BITS = np.array([0x7ff8000000000000], np.uint64).view(np.float64)[0]
TILE_FIELDS = ("n", "owned", "evaluated", "matched", "too_far", "no_normal", "proud", "below", "min_dev", "max_dev", "fix_sum",
               "max_dist2", "own_lo", "own_hi", "sum_parts")
TILE_DECL = ("typedef struct {\n"
             "    size_t n, owned, evaluated;\n"
             "    size_t matched, too_far, no_normal;  /* the owned points by status */\n"
             "    size_t proud, below;\n"
             "    double min_dev, max_dev;             /* over v of the owned matched points; NaN when matched == 0 */\n"
             "    long long fix_sum;                   /* the sum of llrint(v 2^24) over them */\n"
             "    float  max_dist2;                    /* NaN when matched == 0 */\n"
             "    float  own_lo, own_hi;               /* the owned interval [own_lo, own_hi) */\n"
             "    int    sum_parts;\n"
             "} ppp_deviation_tile_stats;")
CALL_DECL = ("int ppp_get_deviation_tile(ppp_handle h, ppp_handle ref, const ppp_deviation_params *dp, float halo,\n"
             "                           double *deviation, double *smoothed, int *ref_index, unsigned char *status,\n"
             "                           double *target, unsigned char *owned, size_t cap, ppp_deviation_tile_stats *part);")
MERGE_DECL = ("int ppp_merge_deviation_tiles(size_t tiles, const ppp_deviation_tile_stats *parts, const double *const *v,\n"
              "                              const unsigned char *const *status, const double *const *target,\n"
              "                              const unsigned char *const *owned, ppp_deviation_stats *stats);")


def ranges3(S):
    """[0, S) in three ranges, the middle one interior"""
    a, b = max(1, (2 * S) // 7), max(2, (5 * S) // 7)
    return [(0, a), (a, b), (b, S)]


def finite_rows(P):
    return np.isfinite(P).all(axis=1)


def cuts_of(E, P, **kw):
    f = finite_rows(P)
    return host_cuts(E, dict(KW0, **kw), P[f, 0].min(), P[f, 0].max())


# ---------------------------------------------------------------- the clouds with a tie and a limit pair across a seam

SEAM = np.float32(53.0)          # cut(2) of both clouds' walks (asserted in the census)
TIE_Y, LIMIT_Y = (-10.0, 10.0), 25.0


@functools.lru_cache(maxsize=None)
def seam_clouds():
    """(reference, scan, notes): main_clouds with, across the seam at x = 53,
    - two ties: reference points at (53 - 0.5, y, z) and (53 + 0.5, y, z) and a scan point at (53, y, z), d2 = 0.25 to either;
      at y near -10 the lower cloud index lies left of the seam, at y near +10 right of it
    - a reference point at (52, y, z), y near 25, left of the seam, with the reference lifted out of reach right of it
      (52.3 < x < 56.2, within 3.5 mm in y), and two scan points right of the seam: one at (54, y, z), d2 = 4 = max_dist^2 exactly, one a float further in x"""
    ref, scan, _ = main_clouds()
    ref, scan = ref.copy(), scan.copy()
    used_r, used_s = set(), set()

    def near(P, used, x, y):
        d = (P[:, 0] - np.float32(x)) ** 2 + (P[:, 1] - np.float32(y)) ** 2
        d[~np.isfinite(d)] = np.inf
        d[list(used)] = np.inf
        i = int(d.argmin())
        used.add(i)
        return i

    notes = dict(ties=[])
    for y, low_left in zip(TIE_Y, (True, False)):
        a, b = near(ref, used_r, SEAM - 0.75, y), near(ref, used_r, SEAM + 0.75, y)
        lo, hi = min(a, b), max(a, b)
        left, right = (lo, hi) if low_left else (hi, lo)
        yy, zz = ref[a, 1], np.float32(np.round(ref[a, 2] * 1024.0) / 1024.0)
        ref[left] = (SEAM - np.float32(0.5), yy, zz)
        ref[right] = (SEAM + np.float32(0.5), yy, zz)
        s = near(scan, used_s, SEAM, yy)
        scan[s] = (SEAM, yy, zz)
        notes["ties"].append(dict(scan=s, left=left, right=right, winner=lo))
    e = near(ref, used_r, SEAM - 1.0, LIMIT_Y)                         # the partner: left of the seam, its neighbours to the left kept
    ref[e] = (SEAM - np.float32(1.0), np.float32(np.round(ref[e, 1] * 1024.0) / 1024.0), np.float32(np.round(ref[e, 2] * 1024.0) / 1024.0))
    yy, zz = ref[e, 1], ref[e, 2]
    hole = (ref[:, 0] > SEAM - np.float32(0.7)) & (ref[:, 0] < SEAM + np.float32(3.2)) & (np.abs(ref[:, 1] - yy) < 3.5)
    ref[hole, 2] += np.float32(60.0)                                   # out of every search: 60 mm off the surface
    at, beyond = near(scan, used_s, SEAM + 1.0, yy), near(scan, used_s, SEAM + 1.0, yy + 1.5)
    scan[at] = (SEAM + np.float32(1.0), yy, zz)
    scan[beyond] = (np.nextafter(SEAM + np.float32(1.0), np.float32(INF)), yy, zz)
    notes.update(edge=e, at=at, beyond=beyond)
    ref.setflags(write=False); scan.setflags(write=False)
    return ref, scan, notes


@functools.lru_cache(maxsize=None)
def seam_restated_cpu():
    from oracle import ppo
    ppo.build()
    ref, scan, _ = seam_clouds()
    o = ppo.Oracle(ref, **KW0)
    Q, N = o.points(), o.estimate_normals()
    o.close()
    return restate_deviation(scan, Q, N, dict(MAIN, smooth_radius=SMOOTH))


# ---------------------------------------------------------------- the restatement of a tile and of the fixed-order sums


def fixed_order_sum(terms, parts):
    """the sum of float64 terms in ppp_get_deviation's order (B.46): `parts` contiguous parts of ceil(n / parts) entries, inside a
    part 256 strided shares each added in index order from +0, the fixed tree over the shares, the parts in order from +0"""
    n = len(terms)
    per = (n + parts - 1) // parts
    total = 0.0
    for g in range(parts):
        seg = terms[g * per:min(n, (g + 1) * per)]
        rows = (len(seg) + 255) // 256
        M = np.zeros((rows + 1, 256))
        M[1:].reshape(-1)[:len(seg)] = seg
        s = np.add.accumulate(M, axis=0)[-1].copy()                     # (accumulate adds in order; np.sum would add pairwise)
        o = 128
        while o:
            s[:o] = s[:o] + s[o:2 * o]
            o //= 2
        total = total + float(s[0])
    return total


def numpy_tile(E, scan, want, lo, hi, parts):
    """a hand-made ppp_get_deviation_tile result from the whole-cloud restatement `want`: the owned rows kept, the others dropped"""
    mine = finite_rows(scan) & (scan[:, 0] >= np.float32(lo)) & (scan[:, 0] < np.float32(hi))
    st = np.where(mine, want["status"], DROPPED).astype(np.uint8)
    m = st == MATCHED
    v = want["smoothed"][m]
    nan = float("nan")
    vlo, vhi = (float(v.min()), float(v.max())) if m.any() else (nan, nan)
    if m.any() and vlo == 0 and np.any(np.signbit(v) & (v == 0)):
        vlo = -0.0
    if m.any() and vhi == 0 and np.any(~np.signbit(v) & (v == 0)):
        vhi = 0.0
    part = dict(n=len(scan), owned=int(mine.sum()), evaluated=int(mine.sum()), matched=int(m.sum()), too_far=int((st == TOO_FAR).sum()),
                no_normal=int((st == NO_NORMAL).sum()), proud=int((v > MAIN["allowance"]).sum()), below=int((v < 0).sum()),
                min_dev=vlo, max_dev=vhi, fix_sum=int(np.rint(v * F24).astype(np.int64).sum(dtype=np.int64)),
                max_dist2=float(want["d2"][m].max()) if m.any() else nan, own_lo=float(lo), own_hi=float(hi), sum_parts=parts)
    return (np.where(m, want["deviation"], NAN_BITS), np.where(m, want["smoothed"], NAN_BITS), np.where(mine, want["ref_index"], -1).astype(np.int32),
            st, np.where(m, want["target"], 0.0), mine.astype(np.uint8), part)


# ---------------------------------------------------------------- CPU


def test_header_declares_and_engine_exports_the_deviation_tiles(engine_mod):
    hdr = open(os.path.join(ROOT, "include", "ppp_hip.h")).read()
    for decl in (TILE_DECL, CALL_DECL, MERGE_DECL):
        assert decl in hdr, decl
    assert hdr.index("int ppp_merge_region_tiles(") < hdr.index(TILE_DECL) < hdr.index(CALL_DECL) < hdr.index(MERGE_DECL)
    assert "DESIGN.md 7n, B.81-B.87" in hdr and "on the host, from the union of the owned entries" in hdr
    for sym in ("ppp_get_deviation_tile", "ppp_merge_deviation_tiles"):
        assert sym in engine_mod.EXPORTS and hasattr(engine_mod.lib(), sym), sym
    assert hasattr(engine_mod.Engine, "deviation_tile") and callable(engine_mod.merge_deviation_tiles)
    planner = open(os.path.join(ROOT, "include", "ppp_planner.hpp")).read()
    assert "bool deviation_tile(const Planner &ref, ppp_deviation_tile_stats &part, " in planner


def test_header_is_c99_clean_with_the_deviation_tiles(tmp_path):
    src = tmp_path / "c99.c"
    src.write_text('#include "ppp_hip.h"\nint main(void) {\n'
                   '    int (*f)(ppp_handle, ppp_handle, const ppp_deviation_params *, float, double *, double *, int *, unsigned char *, double *,\n'
                   '             unsigned char *, size_t, ppp_deviation_tile_stats *) = ppp_get_deviation_tile;\n'
                   '    int (*g)(size_t, const ppp_deviation_tile_stats *, const double *const *, const unsigned char *const *,\n'
                   '             const double *const *, const unsigned char *const *, ppp_deviation_stats *) = ppp_merge_deviation_tiles;\n'
                   '    ppp_deviation_tile_stats st;\n'
                   '    st.fix_sum = 0; st.sum_parts = 1; st.own_hi = 0.f; st.evaluated = 0;\n'
                   '    return f == 0 || g == 0 || st.fix_sum != 0 || st.sum_parts != 1 || st.evaluated != 0;\n}\n')
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                           str(src)])


def test_deviation_tile_stats_layout_matches_the_header(engine_mod, tmp_path):
    T = engine_mod.DeviationTileStats
    assert tuple(f for f, _ in T._fields_) == TILE_FIELDS
    args = ["sizeof(ppp_deviation_tile_stats)"] + ["offsetof(ppp_deviation_tile_stats, %s)" % f for f in TILE_FIELDS]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ppp_hip.h"\nint main(void) {\n'
                   '    printf("' + " ".join(["%zu"] * len(args)) + '\\n", ' + ", ".join(args) + ');\n    return 0;\n}\n')
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)])
    got = [int(v) for v in subprocess.check_output([exe]).split()]
    assert got == [ctypes.sizeof(T)] + [getattr(T, f).offset for f in TILE_FIELDS]


def census(E, ref, scan, want, label):
    """what the GPU tests' input must hold for the halo to be exercised, by restatement alone"""
    S, cuts = cuts_of(E, scan)
    Sr, rcuts = cuts_of(E, ref)
    assert S == Sr == 7 and cuts[2] == rcuts[2] == SEAM and cuts[5] == rcuts[5] == np.float32(125.0)
    # the room a default range handle leaves beyond its cut: int(px[sb]) - 2 - 24 against cut(sb) = px[sb] - 12
    assert 1.0001 * (HALO + NORMAL_RADIUS) < 2 + 24.0 - 12.0 - 1.0
    fin, x = finite_rows(scan), scan[:, 0]
    status, hood, sr2 = want["status"], want["hood"], np.float32(SMOOTH) * np.float32(SMOOTH)
    across_ref = across_smooth = 0
    for t, (b, e) in enumerate(ranges3(S)):
        mine = fin & (x >= cuts[b]) & (x < cuts[e])
        m = mine & (status == MATCHED)
        print("%s tile %d [%g, %g): %d owned, %d matched, %d too far, %d smoothed over more than themselves"
              % (label, t, cuts[b], cuts[e], mine.sum(), m.sum(), (mine & (status == TOO_FAR)).sum(), (m & (hood > 1)).sum()))
        assert m.any() and (mine & (status == TOO_FAR)).any() and (m & (hood > 1)).any()
        rx = ref[want["ref_index"][m], 0]
        out_ref = (rx < rcuts[b]) | (rx >= rcuts[e])                        # the partner lies outside the reference's matching tile
        near = np.nonzero(m & ((x - cuts[b] < SMOOTH) | (cuts[e] - x <= SMOOTH)))[0]
        halo_pts = np.nonzero(fin & ~mine & (status == MATCHED) & (x >= cuts[b] - np.float32(SMOOTH)) & (x <= cuts[e] + np.float32(SMOOTH)))[0]
        reach = (d2_table(scan[near], scan[halo_pts]) <= sr2).any(axis=1) if len(near) and len(halo_pts) else np.zeros(0, bool)
        print("    %d owned points with a partner outside the reference's tile, %d with a smoothing neighbour outside the tile"
              % (out_ref.sum(), reach.sum()))
        assert out_ref.any() and reach.any()
        across_ref += int(out_ref.sum()); across_smooth += int(reach.sum())
    return across_ref, across_smooth


def test_census_of_the_tiled_cases(engine_mod):
    """every tile owns a MATCHED, a TOO_FAR and a smoothed point; in every tile some owned point has a smoothing neighbour outside
    the tile and some owned point's partner lies outside the reference's matching tile; the seam clouds hold what they claim"""
    ref, scan, _ = main_clouds()
    census(engine_mod, ref, scan, main_restated_cpu(SMOOTH), "main")
    ref, scan, notes = seam_clouds()
    want = seam_restated_cpu()
    census(engine_mod, ref, scan, want, "seam")
    for tie in notes["ties"]:
        s = tie["scan"]
        assert want["ties"][s] == 2 and want["d2"][s] == np.float32(0.25) and want["ref_index"][s] == tie["winner"]
        assert ref[tie["left"], 0] < SEAM <= ref[tie["right"], 0] and scan[s, 0] == SEAM
    assert notes["ties"][0]["winner"] == notes["ties"][0]["left"] and notes["ties"][1]["winner"] == notes["ties"][1]["right"]
    md2 = want["md2"]
    assert want["d2"][notes["at"]] == md2 == np.float32(4.0) and want["status"][notes["at"]] == MATCHED
    assert want["ref_index"][notes["at"]] == notes["edge"] and ref[notes["edge"], 0] < SEAM <= scan[notes["at"], 0]
    assert want["d2"][notes["beyond"]] > md2 and want["status"][notes["beyond"]] == TOO_FAR and scan[notes["beyond"], 0] >= SEAM


@pytest.mark.parametrize("parts", [1, 7, 23])
def test_merge_of_hand_made_parts_equals_the_restatement(engine_mod, parts):
    """main_clouds cut into the three tiles in numpy; the C merge gives the restatement's whole-cloud statistics: every integer,
    min_dev, max_dev, mean_dev, max_dist2 and hist exactly, rms_dev and target_sum the bits of the fixed-order sum restated in
    numpy (and within n * 2^-52 of fsum); a doubly-owned point, a part that is not its maps' and tiles that disagree are refused"""
    E = engine_mod
    ref, scan, _ = main_clouds()
    want = main_restated_cpu(SMOOTH)
    S, cuts = cuts_of(E, scan)
    tiles = [numpy_tile(E, scan, want, cuts[b], cuts[e], parts) for b, e in ranges3(S)]
    assert sum(t[6]["owned"] for t in tiles) == int(finite_rows(scan).sum())
    got, ws = E.merge_deviation_tiles(tiles), want["stats"]
    print("got  %r\nwant %r" % ({k: v for k, v in got.items() if k != "hist"}, {k: v for k, v in ws.items() if k != "hist"}))
    assert list(got) == list(STATS_FIELDS)
    for f in STATS_FIELDS:
        if f not in ("rms_dev", "target_sum"):
            assert same(got[f], ws[f]), f
    m = want["status"] == MATCHED
    sq = fixed_order_sum(np.where(m, want["smoothed"] * want["smoothed"], 0.0), parts)
    tg = fixed_order_sum(np.where(m, want["target"], 0.0), parts)
    assert same(got["rms_dev"], math.sqrt(sq / ws["matched"])) and same(got["target_sum"], tg)
    n = len(scan)
    assert abs(got["target_sum"] - ws["target_sum"]) <= n * 2.0 ** -52 * ws["target_sum"]
    assert abs(got["rms_dev"] - ws["rms_dev"]) <= n * 2.0 ** -52 * ws["rms_dev"]
    twice = tiles[1][5].copy()
    twice[np.nonzero(tiles[0][5])[0][0]] = 1                                # a point of tile 0, owned again
    wrong = dict(tiles[1][6], matched=tiles[1][6]["matched"] - 1, too_far=tiles[1][6]["too_far"] + 1)
    other = dict(tiles[2][6], sum_parts=parts + 1)
    for bad in ([tiles[0], tiles[1][:5] + (twice, tiles[1][6]), tiles[2]], [tiles[0], tiles[1][:6] + (wrong,), tiles[2]],
                [tiles[0], tiles[1], tiles[2][:6] + (other,)]):
        with pytest.raises(E.PPPError) as ex:
            E.merge_deviation_tiles(bad)
        assert ex.value.code == E.ERR_ARG


def test_merge_bins_the_ends_of_the_span_the_zeros_and_a_zero_span(engine_mod):
    """the histogram's bin rule, through the merge of two hand-made parts, against the formula written out: bin min(63, max(0,
    floor((v / span + 1) 32))) for v at -span and +span (bins 0 and 63: the clamp), at -0.0 and +0.0 (bin 32), at the largest
    double below span and the smallest above -span, and at a few values between; with every value a zero span == 0 and all of
    them land in bin 32.  An owned point that is not matched is in no bin."""
    E = engine_mod

    def bins_of(x, span):
        if not span > 0.0:
            return np.full(len(x), 32)
        return np.minimum(63, np.maximum(0, np.floor((x / span + 1.0) * 32.0))).astype(np.int64)

    def hand_tile(v, st, mine):
        m = mine & (st == MATCHED)
        w = v[m]
        lo = -0.0 if (w.min() == 0 and np.signbit(w[w == 0]).any()) else float(w.min())
        hi = 0.0 if (w.max() == 0 and not np.signbit(w[w == 0]).all()) else float(w.max())
        part = dict(n=len(v), owned=int(mine.sum()), evaluated=int(mine.sum()), matched=int(m.sum()), too_far=int((mine & (st == TOO_FAR)).sum()),
                    no_normal=0, proud=0, below=int((w < 0).sum()), min_dev=lo, max_dev=hi,
                    fix_sum=int(np.rint(w * F24).astype(np.int64).sum(dtype=np.int64)), max_dist2=1.0, own_lo=0.0, own_hi=1.0, sum_parts=1)
        status = np.where(mine, st, DROPPED).astype(np.uint8)
        return (np.where(m, v, NAN_BITS), np.where(m, v, NAN_BITS), np.full(len(v), -1, np.int32), status, np.zeros(len(v)), mine.astype(np.uint8), part)

    cases = [(span, np.array([-span, span, -0.0, 0.0, np.nextafter(span, 0.0), np.nextafter(-span, 0.0), span / 3.0, -span / 64.0,
                              -span / 32.0, span * 0.984375, float("nan")])) for span in (0.3, 1.0, 2.0 ** -30)]
    cases.append((0.0, np.array([-0.0, 0.0, 0.0, -0.0, float("nan")])))
    for span, v in cases:
        st = np.where(np.isnan(v), TOO_FAR, MATCHED)
        first = np.arange(len(v)) % 2 == 0
        got = E.merge_deviation_tiles([hand_tile(v, st, first), hand_tile(v, st, ~first)])
        m = st == MATCHED
        want = np.bincount(bins_of(v[m], span), minlength=64)
        print("span %r: bins %r" % (span, bins_of(v[m], span).tolist()))
        assert max(abs(got["min_dev"]), abs(got["max_dev"])) == span and got["matched"] == m.sum() and got["too_far"] == 1
        assert np.array_equal(np.asarray(got["hist"]), want) and want.sum() == m.sum()
        if span > 0.0:
            assert want[0] >= 1 and want[63] >= 2 and want[32] == 2      # -span; +span and the double below it; the two zeros
        else:
            assert want[32] == m.sum()


# ---------------------------------------------------------------- GPU

_WHOLE = {}


def whole_of(E, key, ref, scan, **dp):
    """ppp_get_deviation of the two clouds on whole-cloud handles, once per (clouds, parameters)"""
    k = (key, tuple(sorted(dp.items())))
    if k not in _WHOLE:
        r = E.Engine(0, **KW0)
        r.set_cloud(ref)
        s = E.Engine(0, **KW0)
        s.set_cloud(scan)
        _WHOLE[k] = s.deviation(r, **dp)
        r.close(); s.close()
    return _WHOLE[k]


def handle(E, pts, rng=None, **kw):
    more = {} if rng is None else dict(slice_begin=rng[0], slice_end=rng[1])
    h = E.Engine(0, **dict(KW0, **dict(more, **kw)))
    h.set_cloud(pts)
    return h


def check_tile(E, tile, whole, scan, lo, hi, what):
    """one tile against the whole-cloud answer: the owned set by the cuts, the five maps by bytes over it, the fill elsewhere, the
    part's counts those of its maps"""
    dev, sm, idx, status, target, owned, part = tile
    mine = owned == 1
    assert np.array_equal(mine, finite_rows(scan) & (scan[:, 0] >= np.float32(lo)) & (scan[:, 0] < np.float32(hi))), what
    assert set(np.unique(owned)) <= {0, 1} and (part["own_lo"], part["own_hi"]) == (lo, hi)
    for f, got, want in zip(MAPS, tile[:5], whole[:5]):
        bad = np.nonzero((got.view(np.uint8).reshape(len(got), -1) != want.view(np.uint8).reshape(len(want), -1)).any(axis=1) & mine)[0]
        print("%s %s: %d of %d owned entries differ%s" % (what, f, len(bad), mine.sum(), "" if not len(bad) else
              " (first %d: got %r want %r)" % (bad[0], got[bad[0]], want[bad[0]])))
        assert got.dtype == want.dtype and len(bad) == 0, (what, f)
    out = ~mine
    assert np.all(status[out] == DROPPED) and np.all(idx[out] == -1) and np.all(target[out].view(np.uint64) == 0)
    assert np.all(dev[out].view(np.uint64) == 0x7ff8000000000000) and np.all(sm[out].view(np.uint64) == 0x7ff8000000000000)
    m = mine & (status == MATCHED)
    assert (part["n"], part["owned"], part["matched"]) == (len(scan), mine.sum(), m.sum()) and part["evaluated"] >= part["owned"]
    assert (part["too_far"], part["no_normal"]) == ((mine & (status == TOO_FAR)).sum(), (mine & (status == NO_NORMAL)).sum())
    if m.any():
        assert (part["min_dev"], part["max_dev"]) == (sm[m].min(), sm[m].max())
        assert part["fix_sum"] == int(np.rint(sm[m] * F24).astype(np.int64).sum(dtype=np.int64))
    return mine


def check_tiling(E, key, ref, scan, ranges, ref_ranges, halo, **dp):
    """every tile of `ranges` (ref_ranges: None = a whole-cloud reference handle, else the reference's range per tile) against
    the whole-cloud answer, the partition, the merge; returns the tiles"""
    whole = whole_of(E, key, ref, scan, **dp)
    S, cuts = cuts_of(E, scan)
    assert ranges[0][0] == 0 and ranges[-1][1] == S and all(a[1] == b[0] for a, b in zip(ranges, ranges[1:]))
    owners = np.zeros(len(scan), np.int32)
    r_whole = handle(E, ref) if ref_ranges is None else None
    tiles = []
    for t, (b, e) in enumerate(ranges):
        h = handle(E, scan, (b, e))
        r = r_whole if ref_ranges is None else handle(E, ref, ref_ranges[t])
        lo, hi = h.range_owned(float(scan[finite_rows(scan), 0].min()), float(scan[finite_rows(scan), 0].max()))
        assert (np.float32(lo), np.float32(hi)) == (cuts[b], cuts[e])
        tile = h.deviation_tile(r, halo, **dp)
        none = h.deviation_tile(r, halo, maps=False, **dp)
        assert all(x is None for x in none[:6]) and same(none[6], tile[6])
        owners += check_tile(E, tile, whole, scan, lo, hi, "tile %d [%d, %d)" % (t, b, e))
        tiles.append(tile)
        h.close()
        if r is not r_whole:
            r.close()
    if r_whole is not None:
        r_whole.close()
    assert np.array_equal(owners == 1, finite_rows(scan)) and owners.max() == 1          # the owned sets partition the indexed points
    merged, ws = E.merge_deviation_tiles(tiles), whole[5]
    print("merged %r\nwhole  %r" % ({k: v for k, v in merged.items() if k != "hist"}, {k: v for k, v in ws.items() if k != "hist"}))
    assert list(merged) == list(STATS_FIELDS)
    for f in STATS_FIELDS:
        assert same(merged[f], ws[f]), f
    return tiles, whole


@pytest.mark.gpu
@pytest.mark.parametrize("ref_ranged", [False, True])
@pytest.mark.parametrize("smooth", [0.0, SMOOTH])
def test_tiles_equal_the_whole_deviation(engine_mod, smooth, ref_ranged):
    """main_clouds in three slice ranges: for every tile and owned point the five maps are ppp_get_deviation's bytes, the owned
    sets partition the indexed points, the merge is the whole-cloud statistics field for field by bits; with the reference on a
    whole-cloud handle and on a range handle per tile, with smoothing and without"""
    E = engine_mod
    ref, scan, notes = main_clouds()
    S, _ = cuts_of(E, scan)
    Sr, _ = cuts_of(E, ref)
    tiles, whole = check_tiling(E, "main", ref, scan, ranges3(S), ranges3(Sr) if ref_ranged else None, MAIN["max_dist"] + smooth,
                                smooth_radius=smooth, **MAIN)
    st = whole[5]
    assert min(st["matched"], st["too_far"], st["no_normal"], st["dropped"]) > 0
    assert all(t[6]["matched"] > 0 and t[6]["too_far"] > 0 for t in tiles)
    if smooth:
        assert all(t[6]["evaluated"] > t[6]["owned"] for t in tiles)                     # every tile evaluated halo points


@pytest.mark.gpu
@pytest.mark.parametrize("smooth", [0.0, SMOOTH])
def test_a_whole_cloud_handle_is_one_tile_that_owns_everything(engine_mod, smooth):
    """main_clouds, scan and reference on whole-cloud handles (no slice range): the tile call owns exactly the finite rows, its
    five maps are ppp_get_deviation's bytes over all n entries, it evaluates what it owns, and the merge of that single part is
    the whole-cloud statistics field for field by bits"""
    E = engine_mod
    ref, scan, _ = main_clouds()
    dp = dict(MAIN, smooth_radius=smooth)
    whole = whole_of(E, "main", ref, scan, **dp)
    h, r = handle(E, scan), handle(E, ref)
    tile = h.deviation_tile(r, MAIN["max_dist"] + smooth, **dp)
    h.close(); r.close()
    mine = check_tile(E, tile, whole, scan, -INF, INF, "whole-cloud handle, smooth %r" % smooth)
    assert np.array_equal(mine, finite_rows(scan)) and tile[6]["evaluated"] == tile[6]["owned"] == mine.sum()
    for f, got, want in zip(MAPS, tile[:5], whole[:5]):
        assert got.dtype == want.dtype and got.tobytes() == want.tobytes(), f
    merged, ws = E.merge_deviation_tiles([tile]), whole[5]
    print("merged %r\nwhole  %r" % ({k: v for k, v in merged.items() if k != "hist"}, {k: v for k, v in ws.items() if k != "hist"}))
    assert list(merged) == list(STATS_FIELDS)
    for f in STATS_FIELDS:
        assert same(merged[f], ws[f]), f


@pytest.mark.gpu
@pytest.mark.parametrize("ref_ranged", [False, True])
def test_tie_and_limit_across_a_seam(engine_mod, ref_ranged):
    """seam_clouds: a scan point at equal float d2 from two reference points on either side of the reference's range boundary
    takes the lower cloud index, whichever side it lies on, in the tile as in the whole cloud; a scan point at exactly max_dist
    from a partner in the halo, across the seam, is matched, and the one a float further is TOO_FAR"""
    E = engine_mod
    ref, scan, notes = seam_clouds()
    S, _ = cuts_of(E, scan)
    Sr, _ = cuts_of(E, ref)
    tiles, whole = check_tiling(E, "seam", ref, scan, ranges3(S), ranges3(Sr) if ref_ranged else None, HALO, smooth_radius=SMOOTH, **MAIN)
    mid = tiles[1]                                                                       # [53, 125): owns the points at x = 53 and beyond
    for tie in notes["ties"]:
        s = tie["scan"]
        assert mid[5][s] == 1 and mid[2][s] == whole[2][s] == tie["winner"] and tiles[0][5][s] == 0
    assert mid[5][notes["at"]] == 1 and mid[3][notes["at"]] == MATCHED and mid[2][notes["at"]] == notes["edge"]
    assert mid[5][notes["beyond"]] == 1 and mid[3][notes["beyond"]] == TOO_FAR and mid[2][notes["beyond"]] == -1
    assert whole[5]["max_dist2"] == 4.0 and mid[6]["max_dist2"] == 4.0


@pytest.mark.gpu
def test_tiles_beyond_the_grid_cap(engine_mod):
    """large_clouds in two ranges, the first all slices but the last: its tile evaluates more points than the capped grid of
    k_devt_target holds threads, so the grid-stride loop takes a second lap (k_devt_fill's does in both tiles)"""
    E = engine_mod
    ref, scan, notes = large_clouds()
    S, _ = cuts_of(E, scan)
    tiles, whole = check_tiling(E, "large", ref, scan, [(0, S - 1), (S - 1, S)], None, 3.0, max_dist=3.0, smooth_radius=0.0, allowance=0.05,
                                gain=2.0)
    cap = past_the_grid_cap(tiles[0][6]["evaluated"])
    assert len(scan) > cap and tiles[1][6]["owned"] > 0 and whole[5]["dropped"] == 2
    first = np.nonzero((tiles[0][3] == MATCHED))[0]
    assert len(first) >= 100 and whole[5]["matched"] >= 200


@pytest.mark.gpu
def test_same_bits_on_fresh_handles_and_nothing_stored_is_touched(engine_mod):
    """small_40k walk 1 with a bump against itself: a range handle that ran a pass and answered contact queries gives the tile a
    fresh range handle gives; its path contacts, its path coverage and its path (window or slab) are as before; a whole-cloud handle
    on the window path owns everything, equals ppp_get_deviation and stays on the window path; the reference keeps its pass too"""
    E = engine_mod
    pts, cfg = synth.make_config("small_40k")
    scan, _ = bumped(pts)
    kw = dict(tool_radius=cfg["tool_radius"], walk=1)
    dp = dict(max_dist=3.0, smooth_radius=4.0, allowance=0.05, gain=1.0)
    r = E.Engine(0, **kw)
    r.set_cloud(pts)
    Sr = r.gen_path(); r.get_path()
    rwp = r.waypoints().copy()
    w = E.Engine(0, **kw)
    w.set_cloud(scan)
    S = w.gen_path(); w.get_path()
    assert w.fast_path()
    wwp = w.waypoints().copy()
    whole = w.deviation(r, **dp)
    all_of_it = w.deviation_tile(r, 7.0, **dp)
    assert same(all_of_it[:5], whole[:5]) and np.array_equal(all_of_it[5] == 1, whole[3] != DROPPED)
    assert same(E.merge_deviation_tiles([all_of_it]), whole[5])
    assert w.fast_path() and same(w.waypoints(), wwp) and r.fast_path() and same(r.waypoints(), rwp)
    b, e = slice_ranges(S, 4)[1]
    a = E.Engine(0, slice_begin=b, slice_end=e, range_margin=RANGE_MARGIN, **kw)
    a.set_cloud(scan)
    a.gen_path(); a.get_path()
    fast, slices, contacts, covered = a.fast_path(), a.num_slices(), a.path_contacts(), a.path_coverage()
    first = a.deviation_tile(r, 7.0, **dp)
    again = a.deviation_tile(r, 7.0, **dp)
    fresh = E.Engine(0, slice_begin=b, slice_end=e, range_margin=RANGE_MARGIN, **kw)
    fresh.set_cloud(scan)
    other = fresh.deviation_tile(r, 7.0, **dp)
    assert same(first, again) and same(first, other) and first[6]["owned"] > 0 and first[6]["evaluated"] > first[6]["owned"]
    mine = first[5] == 1
    for got, want in zip(first[:5], whole[:5]):
        assert got[mine].tobytes() == want[mine].tobytes()
    assert a.fast_path() == fast and a.num_slices() == slices and same(a.path_contacts(), contacts) and same(a.path_coverage(), covered)
    assert same(r.waypoints(), rwp) and (Sr, S) == (r.num_slices(), w.num_slices())
    for h in (r, w, a, fresh):
        h.close()


@pytest.mark.gpu
def test_deviation_tile_refusals(engine_mod):
    E = engine_mod
    ref, scan, _ = main_clouds()
    S, cuts = cuts_of(E, scan)
    rng = ranges3(S)
    r, h = handle(E, ref), handle(E, scan, rng[1])
    ok = dict(MAIN, smooth_radius=SMOOTH)

    def refused(h, other, code, halo=HALO, **k):
        """the code, and not one launch on either handle: no index build, no normal field, no kernel of the call"""
        for e in (h, other):
            e.enable_timing(True)
            e.kernel_times()
        for maps in (False, True):
            with pytest.raises(E.PPPError) as ex:
                h.deviation_tile(other, halo, maps=maps, **dict(ok, **k))
            assert ex.value.code == code, (k, maps, ex.value)
            for e in (h, other):
                launches = e.kernel_times(with_launches=True)[1]
                assert not any(launches.values()), (k, maps, launches)

    h.enable_timing(True)
    h.kernel_times()
    h.deviation_tile(r, HALO, maps=False, **ok)                               # the accepted call all refusals below differ from
    launches = h.kernel_times(with_launches=True)[1]                          # (and the counter does see this call's kernels)
    assert all(launches.get(k) == 1 for k in ("k_devt_fill", "k_devt_nearest", "k_devt_smooth", "k_devt_target")), launches
    refused(h, r, E.ERR_ARG, halo=np.nextafter(np.float32(HALO), np.float32(0)))         # halo too small
    refused(h, r, E.ERR_ARG, halo=INF)
    refused(h, r, E.ERR_ARG, halo=float("nan"))
    refused(h, r, E.ERR_ARG, halo=1e30, max_dist=INF, smooth_radius=0.0)      # a tile needs a finite max_dist
    for bad in (dict(max_dist=0.0), dict(max_dist=float("nan")), dict(smooth_radius=-1.0), dict(allowance=INF), dict(gain=-1.0)):
        refused(h, r, E.ERR_ARG, halo=1e30, **bad)                            # as ppp_get_deviation
    # a reference range that does not cover the halo: another tile's range, and the matching range with the least margin a
    # handle takes (twice the normal radius: it indexes from 58, the halo starts at 53 - 8.5)
    far = handle(E, ref, rng[2])
    refused(h, far, E.ERR_ARG)
    bare = handle(E, ref, rng[1], range_margin=5.0)
    refused(h, bare, E.ERR_ARG)
    # a scan margin that does not cover smooth_radius: the same range indexed from 58, the evaluated interval starts at 49
    thin = handle(E, scan, rng[1], range_margin=5.0)
    refused(thin, r, E.ERR_ARG)
    # a part handle on either side
    f = finite_rows(scan)
    mn, mx = scan[f].min(axis=0), scan[f].max(axis=0)
    p = E.Engine(0, slice_begin=rng[1][0], slice_end=rng[1][1], **KW0)
    lo, hi, _ = p.range_interval(mn[0], mx[0])
    keep = np.nonzero(f & (scan[:, 0] >= lo) & (scan[:, 0] <= hi))[0]
    p.set_cloud_part(scan[keep], keep, mn, mx, int(f.sum()), lo, hi)
    refused(p, r, E.ERR_UNSUPPORTED)
    refused(h, p, E.ERR_UNSUPPORTED)
    # NULL dp / ref, no cloud
    part = E.DeviationTileStats()
    dpar = E.DeviationParams(2.0, SMOOTH, 0.1, 3.0)
    L = h.L
    h.kernel_times(); r.kernel_times()
    assert L.ppp_get_deviation_tile(h.h, None, ctypes.byref(dpar), HALO, None, None, None, None, None, None, 0, ctypes.byref(part)) == E.ERR_ARG
    assert L.ppp_get_deviation_tile(h.h, r.h, None, HALO, None, None, None, None, None, None, 0, ctypes.byref(part)) == E.ERR_ARG
    assert not any(h.kernel_times(with_launches=True)[1].values()) and not any(r.kernel_times(with_launches=True)[1].values())
    empty = E.Engine(0, **KW0)
    refused(h, empty, E.ERR_ARG)
    refused(empty, r, E.ERR_ARG)
    # every refusal left the handle usable and the answer unchanged
    whole = whole_of(E, "main", ref, scan, smooth_radius=SMOOTH, **MAIN)
    tile = h.deviation_tile(r, HALO, **ok)
    check_tile(E, tile, whole, scan, float(cuts[rng[1][0]]), float(cuts[rng[1][1]]), "after the refusals")
    for e in (r, h, far, bare, thin, p, empty):
        e.close()


@functools.lru_cache(maxsize=None)
def device_count():
    """the devices torch sees, asked once in a process of its own (as test_path_removal.compute_units asks)"""
    import sys
    return int(subprocess.check_output([sys.executable, "-c", "import torch; print(torch.cuda.device_count())"]).split()[-1])


@pytest.mark.gpu
def test_handles_on_different_devices_are_refused(engine_mod):
    """the scan's range handle on device 0, the reference on device 1: PPP_ERR_ARG, and no launch on either"""
    if device_count() < 2:
        pytest.skip("needs two GPUs in one process: this machine shows %d" % device_count())
    E = engine_mod
    ref, scan, _ = main_clouds()
    S, _ = cuts_of(E, scan)
    h = handle(E, scan, ranges3(S)[1])
    d1 = E.Engine(1, **KW0)
    d1.set_cloud(ref)
    for e in (h, d1):
        e.enable_timing(True)
        e.kernel_times()
    for maps in (False, True):
        with pytest.raises(E.PPPError) as ex:
            h.deviation_tile(d1, HALO, maps=maps, smooth_radius=SMOOTH, **MAIN)
        assert ex.value.code == E.ERR_ARG
        assert not any(h.kernel_times(with_launches=True)[1].values()) and not any(d1.kernel_times(with_launches=True)[1].values())
    h.close(); d1.close()
