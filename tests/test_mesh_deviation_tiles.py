"""The exact deviation against a triangle mesh for the points a handle owns (ppp_get_mesh_deviation_tile,
ppp_get_mesh_signed_deviation_tile, ppp_merge_mesh_deviation_tiles, ppp_merge_mesh_signed_deviation_tiles; DESIGN.md 7za and
B.144-B.147).

Every comparison is for equality: a tile's maps against the whole-cloud call's by bytes over the owned points and against the numpy
restatements of tests/test_trimesh.py and tests/test_trimesh_topology.py, the fill everywhere else, the merged statistics against
the whole-cloud call's field for field by bits.  No tolerance appears anywhere in this file.

The case is the wavy sheet of tests/test_mesh_registration.py stretched in x: sheet(40, 16, 2.5) with surface() on z, 1 280
triangles over 100 x 40 mm, under 3 000 scan points with 0.05 mm of noise that go on 3 mm past the border (so closest points lie on
edges and vertices), the first tenth raised beyond max_dist, one point moved onto a cut's float.  The default walk cuts it into at
least 5 slices; the tiles are ranges3(S), the middle one interior with two seams."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from test_deviation import d2_table
from test_deviation_tiles import cuts_of, device_count, finite_rows, fixed_order_sum, handle, ranges3
from test_mesh_registration import surface
from test_path_dwell import same
from test_registration import motion_about
from test_trimesh import DROPPED, EDGE, FACE, MATCHED, TOO_FAR, VERTEX, nearest_on_mesh, restate_tail, sheet
from test_trimesh_topology import restate_signed, restate_topology

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN64 = 0x7ff8000000000000
F24 = 2.0 ** 24
N_SCAN, N_RAISED = 3000, 300
MAX_DIST, SMOOTH = 2.0, 3.0
DP = dict(max_dist=MAX_DIST, allowance=0.02, gain=3.0)
MOTION = dict(c=[50.0, 20.0, 0.0], deg=(1.0, -0.8, 1.5), shift=(0.4, -0.3, 0.35))
UNSIGNED_MAPS = ("deviation", "smoothed", "distance", "tri_index", "region", "status", "target")
SIGNED_MAPS = ("signed_distance", "smoothed", "distance", "tri_index", "region", "feature", "flags", "status", "target")
DEV_PART = ("n", "owned", "evaluated", "matched", "too_far", "no_normal", "proud", "below", "min_dev", "max_dev", "fix_sum", "max_dist2", "own_lo",
            "own_hi", "sum_parts")
MESH_PART = ("on_face", "on_edge", "on_vertex", "max_distance")
SIGNED_PART = ("on_border", "irregular", "fallback", "negative", "positive")
STRUCTS = ("typedef struct {\n"
           "    ppp_deviation_tile_stats dev;\n"
           "    size_t on_face, on_edge, on_vertex;  /* the owned matched points by region */\n"
           "    double max_distance;                 /* over them; NaN when dev.matched == 0 */\n"
           "} ppp_mesh_deviation_tile_stats;",
           "typedef struct {\n"
           "    ppp_mesh_deviation_tile_stats mesh;\n"
           "    size_t on_border, irregular, fallback, negative, positive;\n"
           "} ppp_mesh_signed_deviation_tile_stats;")
DECLS = ("int ppp_get_mesh_deviation_tile(ppp_handle h, ppp_trimesh m, const ppp_deviation_params *dp,\n"
         "                                double *deviation, double *smoothed, double *distance, int *tri_index,\n"
         "                                unsigned char *region, unsigned char *status, double *target, unsigned char *owned,\n"
         "                                size_t cap, ppp_mesh_deviation_tile_stats *part);",
         "int ppp_get_mesh_signed_deviation_tile(ppp_handle h, ppp_trimesh m, const ppp_deviation_params *dp,\n"
         "                                       double *signed_distance, double *smoothed, double *distance, int *tri_index,\n"
         "                                       unsigned char *region, unsigned char *feature, unsigned char *flags,\n"
         "                                       unsigned char *status, double *target, unsigned char *owned,\n"
         "                                       size_t cap, ppp_mesh_signed_deviation_tile_stats *part);",
         "int ppp_merge_mesh_deviation_tiles(size_t tiles, const ppp_mesh_deviation_tile_stats *parts, const double *const *v,\n"
         "                                   const unsigned char *const *status, const double *const *target,\n"
         "                                   const unsigned char *const *owned, ppp_mesh_deviation_stats *stats);",
         "int ppp_merge_mesh_signed_deviation_tiles(size_t tiles, const ppp_mesh_signed_deviation_tile_stats *parts,\n"
         "                                          const double *const *v, const unsigned char *const *status,\n"
         "                                          const double *const *target, const unsigned char *const *owned,\n"
         "                                          ppp_mesh_signed_deviation_stats *stats);")
SYMBOLS = ("ppp_get_mesh_deviation_tile", "ppp_get_mesh_signed_deviation_tile", "ppp_merge_mesh_deviation_tiles", "ppp_merge_mesh_signed_deviation_tiles")


# ---------------------------------------------------------------- the case


def long_mesh():
    v, t = sheet(40, 16, 2.5)
    v = v.copy()
    v[:, 2] = surface(v[:, 0].astype(np.float64), v[:, 1].astype(np.float64)).astype(np.float32)
    return v, t


_CASE = {}


def tile_case(E):
    """dict: verts float32[697, 3], tris int32[1280, 3]; scan float32[3000, 3], the scan on the mesh, with S and cuts of its walk
    and `planted`, the point whose x is cuts[ranges3(S)[0][1]] exactly; moved float32[3000, 3], the scan carried off by the inverse
    of Tm, with its own S and cuts.  Nobody writes to them"""
    if _CASE:
        return _CASE
    v, t = long_mesh()
    rng = np.random.default_rng(11)
    x, y = rng.uniform(-3.0, 103.0, N_SCAN), rng.uniform(-3.0, 43.0, N_SCAN)
    z = surface(np.clip(x, 0.0, 100.0), np.clip(y, 0.0, 40.0)) + rng.uniform(-0.05, 0.05, N_SCAN)
    z[:N_RAISED] += 4.0                                                       # the first tenth: beyond max_dist
    scan64 = np.stack([x, y, z], axis=1)
    scan = scan64.astype(np.float32)
    S, cuts = cuts_of(E, scan)
    seam = cuts[ranges3(S)[0][1]]
    planted = N_RAISED + int(np.abs(scan[N_RAISED:, 0] - seam).argmin())     # a clean point, the nearest to the seam: it moves by a hair
    assert planted not in (int(scan[:, 0].argmin()), int(scan[:, 0].argmax()))
    scan[planted, 0] = seam
    assert same(cuts_of(E, scan)[1], cuts)                                   # the bounds, and with them the cuts, stayed
    Tm = motion_about(MOTION["c"], MOTION["deg"], MOTION["shift"])
    moved = ((scan.astype(np.float64) - Tm[:, 3]) @ Tm[:, :3]).astype(np.float32)       # the inverse motion: R^T (p - t)
    mS, mcuts = cuts_of(E, moved)
    for a in (v, t, scan, moved, cuts, mcuts, Tm):
        a.setflags(write=False)
    _CASE.update(verts=v, tris=t, scan=scan, S=S, cuts=cuts, planted=planted, moved=moved, mS=mS, mcuts=mcuts, Tm=Tm)
    return _CASE


def owned_by(P, lo, hi):
    return finite_rows(P) & (P[:, 0] >= np.float32(lo)) & (P[:, 0] < np.float32(hi))


_RESTATED = {}


def restated(E, smooth, signed):
    """the whole-cloud answer by restatement: dict of the maps (UNSIGNED_MAPS or SIGNED_MAPS) and `stats` with the exact fields"""
    key = (smooth, signed)
    if key in _RESTATED:
        return _RESTATED[key]
    C = tile_case(E)
    P = C["scan"]
    if "first" not in _RESTATED:
        _RESTATED["first"] = nearest_on_mesh(C["verts"], C["tris"], P, max_dist=MAX_DIST)
        _RESTATED["sign"] = restate_signed(C["verts"], C["tris"], P, topo=restate_topology(C["verts"], C["tris"]), max_dist=MAX_DIST)
    first = dict(_RESTATED["sign"] if signed else _RESTATED["first"])
    if signed:
        first["deviation"] = first["signed_distance"]
    dp = dict(DP, smooth_radius=smooth)
    sm, target, stats = restate_tail(P, first, dp)
    m = first["status"] == MATCHED
    sm = np.where(m, sm, np.nan)
    reg = first["region"][m]
    stats.update(on_face=int((reg == FACE).sum()), on_edge=int((reg == EDGE).sum()), on_vertex=int((reg == VERTEX).sum()),
                 max_distance=float(first["distance"][m].max()))
    out = dict(first, smoothed=sm, target=target, stats=stats, d2f=first["D2"].astype(np.float32))
    if signed:
        fl, sd = first["flags"][m], first["signed_distance"][m]
        stats.update(on_border=int(((fl & 1) != 0).sum()), irregular=int(((fl & 2) != 0).sum()), fallback=int(((fl & 4) != 0).sum()),
                     negative=int((sd < 0).sum()), positive=int((sd > 0).sum()))
    _RESTATED[key] = out
    return out


def numpy_tile(E, want, signed, lo, hi, parts, allowance=DP["allowance"]):
    """a hand-made tile result from the whole-cloud restatement `want`: the owned rows kept, the others filled"""
    P = tile_case(E)["scan"]
    mine = owned_by(P, lo, hi)
    st = np.where(mine, want["status"], DROPPED).astype(np.uint8)
    m = st == MATCHED
    v = want["smoothed"][m]
    nan = float("nan")
    part = dict(n=len(P), owned=int(mine.sum()), evaluated=int(mine.sum()), matched=int(m.sum()), too_far=int((st == TOO_FAR).sum()), no_normal=0,
                proud=int((v > allowance).sum()), below=int((v < 0).sum()), min_dev=float(v.min()) if m.any() else nan,
                max_dev=float(v.max()) if m.any() else nan, fix_sum=int(np.rint(v * F24).astype(np.int64).sum(dtype=np.int64)),
                max_dist2=float(want["d2f"][m].max()) if m.any() else nan, own_lo=float(lo), own_hi=float(hi), sum_parts=parts)
    reg = want["region"][m]
    part.update(on_face=int((reg == FACE).sum()), on_edge=int((reg == EDGE).sum()), on_vertex=int((reg == VERTEX).sum()),
                max_distance=float(want["distance"][m].max()) if m.any() else nan)
    nanmap = lambda a: np.where(m, a, np.nan)
    maps = [nanmap(want["deviation"]), nanmap(want["smoothed"]), nanmap(want["distance"]), np.where(m, want["tri_index"], -1).astype(np.int32),
            np.where(m, want["region"], 255).astype(np.uint8)]
    if signed:
        fl, sd = want["flags"][m], want["signed_distance"][m]
        part.update(on_border=int(((fl & 1) != 0).sum()), irregular=int(((fl & 2) != 0).sum()), fallback=int(((fl & 4) != 0).sum()),
                    negative=int((sd < 0).sum()), positive=int((sd > 0).sum()))
        maps += [np.where(m, want["feature"], 255).astype(np.uint8), np.where(m, want["flags"], 0).astype(np.uint8)]
    return tuple(maps) + (st, np.where(m, want["target"], 0.0), mine.astype(np.uint8), part)


# ---------------------------------------------------------------- CPU


def test_header_declares_and_engine_exports_the_mesh_deviation_tiles(engine_mod):
    hdr = open(os.path.join(ROOT, "include", "ppp_hip.h")).read()
    for decl in STRUCTS + DECLS:
        assert decl in hdr, decl
    at = [hdr.index("int    ppp_register_robust_tiles(")] + [hdr.index(d) for d in STRUCTS + DECLS] + [hdr.index("int ppp_eval_spline(")]
    assert at == sorted(at)
    assert "DESIGN.md 7za, B.144-B.149" in hdr and "There is no halo argument" in hdr
    for sym in SYMBOLS:
        assert sym in engine_mod.EXPORTS and hasattr(engine_mod.lib(), sym), sym
    for m in ("mesh_deviation_tile", "mesh_signed_deviation_tile"):
        assert callable(getattr(engine_mod.Engine, m)), m
    assert callable(engine_mod.merge_mesh_deviation_tiles) and callable(engine_mod.merge_mesh_signed_deviation_tiles)
    planner = open(os.path.join(ROOT, "include", "ppp_planner.hpp")).read()
    assert "bool mesh_deviation_tile(const TriMesh &mesh, ppp_mesh_deviation_tile_stats &part, " in planner
    mk = open(os.path.join(ROOT, "polishpathplanning_amd", "csrc", "Makefile")).read()
    assert "ppp_mesh_tile.h" in [l for l in mk.splitlines() if l.startswith("SCAN_HDR")][0]
    assert '#include "ppp_mesh_tile.h"' in open(os.path.join(ROOT, "polishpathplanning_amd", "csrc", "ppp_scan.hip")).read()


def test_header_is_c99_clean_and_the_layouts_match(engine_mod, tmp_path):
    E = engine_mod
    U, Sg = E.MeshDeviationTileStats, E.MeshSignedDeviationTileStats
    assert tuple(f for f, _ in U._fields_) == ("dev",) + MESH_PART and tuple(f for f, _ in Sg._fields_) == ("mesh",) + SIGNED_PART
    args = (["sizeof(ppp_mesh_deviation_tile_stats)"] + ["offsetof(ppp_mesh_deviation_tile_stats, %s)" % f for f in ("dev",) + MESH_PART] +
            ["sizeof(ppp_mesh_signed_deviation_tile_stats)"] + ["offsetof(ppp_mesh_signed_deviation_tile_stats, %s)" % f for f in ("mesh",) + SIGNED_PART])
    src = tmp_path / "c99.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ppp_hip.h"\nint main(void) {\n'
                   '    int (*f)(ppp_handle, ppp_trimesh, const ppp_deviation_params *, double *, double *, double *, int *, unsigned char *,\n'
                   '             unsigned char *, double *, unsigned char *, size_t, ppp_mesh_deviation_tile_stats *) = ppp_get_mesh_deviation_tile;\n'
                   '    int (*g)(ppp_handle, ppp_trimesh, const ppp_deviation_params *, double *, double *, double *, int *, unsigned char *,\n'
                   '             unsigned char *, unsigned char *, unsigned char *, double *, unsigned char *, size_t,\n'
                   '             ppp_mesh_signed_deviation_tile_stats *) = ppp_get_mesh_signed_deviation_tile;\n'
                   '    int (*m)(size_t, const ppp_mesh_deviation_tile_stats *, const double *const *, const unsigned char *const *,\n'
                   '             const double *const *, const unsigned char *const *, ppp_mesh_deviation_stats *) = ppp_merge_mesh_deviation_tiles;\n'
                   '    int (*s)(size_t, const ppp_mesh_signed_deviation_tile_stats *, const double *const *, const unsigned char *const *,\n'
                   '             const double *const *, const unsigned char *const *, ppp_mesh_signed_deviation_stats *) =\n'
                   '        ppp_merge_mesh_signed_deviation_tiles;\n'
                   '    if (f == 0 || g == 0 || m == 0 || s == 0) return 1;\n'
                   '    printf("' + " ".join(["%lu"] * len(args)) + '\\n", ' + ", ".join("(unsigned long)" + a for a in args) + ');\n    return 0;\n}\n')
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src), os.path.join(ROOT, "polishpathplanning_amd", "libppp_hip.so"),
                           "-Wl,-rpath," + os.path.join(ROOT, "polishpathplanning_amd")])
    got = [int(x) for x in subprocess.check_output([exe]).split()]
    assert got == ([ctypes.sizeof(U)] + [getattr(U, f).offset for f in ("dev",) + MESH_PART] +
                   [ctypes.sizeof(Sg)] + [getattr(Sg, f).offset for f in ("mesh",) + SIGNED_PART])


def test_census_of_the_tiled_mesh_case(engine_mod):
    """by restatement alone: at least 5 slices; every tile owns matched and too-far points; on both sides of either seam a matched
    point lies within smooth_radius of it and has a matched neighbour across it within smooth_radius (a missing halo changes its
    smoothed value); face, edge and vertex regions all occur among the owned points of one tile; the point on the cut's float is
    the upper tile's alone"""
    E = engine_mod
    C = tile_case(E)
    P, S, cuts = C["scan"], C["S"], C["cuts"]
    want = restated(E, SMOOTH, True)
    status, region = want["status"], want["region"]
    rngs = ranges3(S)
    print("S %d, cuts %r, ranges %r; moved: S %d" % (S, cuts.tolist(), rngs, C["mS"]))
    assert S >= 5 and C["mS"] >= 5 and len(C["tris"]) == 1280 and len(P) == N_SCAN
    assert rngs[1][0] > 0 and rngs[1][1] < S                                 # the middle tile is interior: two seams
    m = status == MATCHED
    sr2 = np.float32(SMOOTH) * np.float32(SMOOTH)
    all_three = 0
    for t, (b, e) in enumerate(rngs):
        mine = owned_by(P, cuts[b], cuts[e])
        reg = region[mine & m]
        counts = tuple(int((reg == k).sum()) for k in (FACE, EDGE, VERTEX))
        print("tile %d [%g, %g): %d owned, %d matched (face / edge / vertex %r), %d too far" % (t, cuts[b], cuts[e], mine.sum(), (mine & m).sum(), counts,
                                                                                                (mine & (status == TOO_FAR)).sum()))
        assert (mine & m).any() and (mine & (status == TOO_FAR)).any()
        all_three += min(counts) > 0
    assert all_three >= 1
    for seam in (cuts[rngs[1][0]], cuts[rngs[1][1]]):
        x = P[:, 0]
        below = np.nonzero(m & (x < seam) & (seam - x <= SMOOTH))[0]
        above = np.nonzero(m & (x >= seam) & (x - seam < SMOOTH))[0]
        across = d2_table(P[below], P[above]) <= sr2
        print("seam %g: %d matched points within smooth_radius below it, %d above; %d / %d have a neighbour across it"
              % (seam, len(below), len(above), across.any(axis=1).sum(), across.any(axis=0).sum()))
        assert across.any(axis=1).sum() >= 3 and across.any(axis=0).sum() >= 3
    p, a = C["planted"], rngs[0][1]
    assert P[p, 0] == cuts[a] and status[p] == MATCHED
    assert not owned_by(P, cuts[0], cuts[a])[p] and owned_by(P, cuts[a], cuts[rngs[1][1]])[p]
    # the signed case has both signs, and border features under the overhang
    st = want["stats"]
    print("signed: %r" % {k: st[k] for k in SIGNED_PART})
    assert st["negative"] > 100 and st["positive"] > 100 and st["on_border"] > 0 and st["matched"] == st["on_face"] + st["on_edge"] + st["on_vertex"]
    assert st["dropped"] == 0 and st["too_far"] >= N_RAISED


@pytest.mark.parametrize("signed", [False, True])
def test_merges_of_hand_made_parts(engine_mod, signed):
    """the restatement cut into the three tiles in numpy: the C merges give the whole cloud's statistics -- every count the sum,
    max_distance the maximum, the deviation's fields as ppp_merge_deviation_tiles gives them (rms_dev and target_sum the bits of the
    fixed-order sum restated in numpy); max_distance is the NaN when nothing matched; two tiles that own one point, a part whose
    regions do not add up and a NULL map are refused"""
    E = engine_mod
    C = tile_case(E)
    P, S, cuts = C["scan"], C["S"], C["cuts"]
    want = restated(E, SMOOTH, signed)
    parts = 3
    tiles = [numpy_tile(E, want, signed, cuts[b], cuts[e], parts) for b, e in ranges3(S)]
    merge = E.merge_mesh_signed_deviation_tiles if signed else E.merge_mesh_deviation_tiles
    got, ws = merge(tiles), want["stats"]
    print("got  %r\nwant %r" % ({k: v for k, v in got.items() if k != "hist"}, {k: v for k, v in ws.items() if k != "hist"}))
    assert sum(t[-1]["owned"] for t in tiles) == int(finite_rows(P).sum())
    for f in got:
        if f not in ("rms_dev", "target_sum"):
            assert same(np.asarray(got[f]), np.asarray(ws[f]).astype(np.asarray(got[f]).dtype)), (f, got[f], ws[f])
    for f in MESH_PART[:3] + (SIGNED_PART if signed else ()):
        assert got[f] == sum(t[-1][f] for t in tiles), f
    assert got["max_distance"] == max(t[-1]["max_distance"] for t in tiles)
    m = want["status"] == MATCHED
    sq = fixed_order_sum(np.where(m, want["smoothed"] * want["smoothed"], 0.0), parts)
    tg = fixed_order_sum(np.where(m, want["target"], 0.0), parts)
    assert same(got["rms_dev"], float(np.sqrt(sq / ws["matched"]))) and same(got["target_sum"], tg)
    # nothing matched anywhere: the NaN
    nothing = dict(want, status=np.where(m, TOO_FAR, want["status"]).astype(np.uint8))
    none = merge([numpy_tile(E, nothing, signed, cuts[b], cuts[e], parts) for b, e in ranges3(S)])
    assert none["matched"] == 0 and np.array([none["max_distance"]]).view(np.uint64)[0] == NAN64 and none["on_face"] == none["on_edge"] == none["on_vertex"] == 0
    # one tile matched nothing: its NaN does not enter the maximum
    a, b = ranges3(S)[0]
    mixed = [numpy_tile(E, nothing, signed, cuts[a], cuts[b], parts)] + tiles[1:]
    assert merge(mixed)["max_distance"] == max(t[-1]["max_distance"] for t in tiles[1:])
    twice = tiles[1][-2].copy()
    twice[np.nonzero(tiles[0][-2])[0][0]] = 1                                # a point of tile 0, owned again
    lopsided = dict(tiles[1][-1], on_face=tiles[1][-1]["on_face"] + 1)
    for bad in ([tiles[0], tiles[1][:-2] + (twice, tiles[1][-1]), tiles[2]], [tiles[0], tiles[1][:-1] + (lopsided,), tiles[2]]):
        with pytest.raises(E.PPPError) as ex:
            merge(bad)
        assert ex.value.code == E.ERR_ARG
    L = E.lib()
    st = (E.MeshSignedDeviationStats if signed else E.MeshDeviationStats)()
    one = (E.MeshSignedDeviationTileStats if signed else E.MeshDeviationTileStats)()
    call = L.ppp_merge_mesh_signed_deviation_tiles if signed else L.ppp_merge_mesh_deviation_tiles
    assert call(1, ctypes.byref(one), None, None, None, None, ctypes.byref(st)) == E.ERR_ARG
    assert call(0, ctypes.byref(one), None, None, None, None, ctypes.byref(st)) == E.ERR_ARG
    assert call(1, None, None, None, None, None, ctypes.byref(st)) == E.ERR_ARG


# ---------------------------------------------------------------- GPU


_WHOLE = {}


def whole_of(E, smooth, signed):
    """the whole-cloud call on a whole-cloud handle with an automatic cell, once per (smooth, signed)"""
    key = (smooth, signed)
    if key not in _WHOLE:
        C = tile_case(E)
        s = handle(E, C["scan"])
        mesh = s.trimesh(C["verts"], C["tris"])
        call = s.mesh_signed_deviation if signed else s.mesh_deviation
        _WHOLE[key] = call(mesh, smooth_radius=smooth, **DP)
        mesh.close(); s.close()
    return _WHOLE[key]


def differing(got, want, rows):
    return np.nonzero((got.view(np.uint8).reshape(len(got), -1) != want.view(np.uint8).reshape(len(want), -1)).any(axis=1) & rows)[0]


def check_tile(E, tile, whole, signed, lo, hi, what, restatement=None):
    """one tile against the whole-cloud answer (and the restatement): the owned set by the cuts, every map by bytes over it, the
    fill elsewhere, the part's counts those of its maps"""
    P = tile_case(E)["scan"]
    names = SIGNED_MAPS if signed else UNSIGNED_MAPS
    maps, owned, part = dict(zip(names, tile)), tile[-2], tile[-1]
    mine = owned == 1
    assert np.array_equal(mine, owned_by(P, lo, hi)) and set(np.unique(owned)) <= {0, 1}, what
    assert (np.float32(part["own_lo"]), np.float32(part["own_hi"])) == (np.float32(lo), np.float32(hi))
    for k, (name, want) in enumerate(zip(names, whole)):
        got = maps[name]
        bad = differing(got, want, mine)
        print("%s %s: %d of %d owned entries differ from the whole-cloud call%s" % (what, name, len(bad), mine.sum(), "" if not len(bad) else
              " (first %d: got %r want %r)" % (bad[0], got[bad[0]], want[bad[0]])))
        assert got.dtype == want.dtype and len(bad) == 0, (what, name)
        if restatement is not None:
            w = np.ascontiguousarray(restatement["deviation" if name == "signed_distance" else name]).astype(got.dtype)
            assert len(differing(got, w, mine)) == 0, (what, name, "restatement")
    out = ~mine
    st = maps["status"]
    assert np.all(st[out] == DROPPED) and np.all(maps["tri_index"][out] == -1) and np.all(maps["region"][out] == 255)
    assert np.all(maps["target"][out].view(np.uint64) == 0)
    for name in (names[0], "smoothed", "distance"):
        assert np.all(maps[name][out].view(np.uint64) == NAN64), (what, name)
    if signed:
        assert np.all(maps["feature"][out] == 255) and np.all(maps["flags"][out] == 0)
    m = mine & (st == MATCHED)
    assert (part["n"], part["owned"], part["matched"], part["too_far"], part["no_normal"]) == (len(P), mine.sum(), m.sum(), (mine & (st == TOO_FAR)).sum(), 0)
    assert part["evaluated"] >= part["owned"]
    reg = maps["region"][m]
    assert (part["on_face"], part["on_edge"], part["on_vertex"]) == tuple(int((reg == k).sum()) for k in (FACE, EDGE, VERTEX))
    if m.any():
        sm = maps["smoothed"]
        assert (part["min_dev"], part["max_dev"], part["max_distance"]) == (sm[m].min(), sm[m].max(), maps["distance"][m].max())
        assert part["fix_sum"] == int(np.rint(sm[m] * F24).astype(np.int64).sum(dtype=np.int64))
    if signed:
        fl, sd = maps["flags"][m], maps["signed_distance"][m]
        assert (part["on_border"], part["irregular"], part["fallback"], part["negative"], part["positive"]) == (
            ((fl & 1) != 0).sum(), ((fl & 2) != 0).sum(), ((fl & 4) != 0).sum(), (sd < 0).sum(), (sd > 0).sum())
    return mine


def tiles_of(E, smooth, signed, cell=0.0, device_of=lambda t: 0, restatement=None):
    """every tile of ranges3(S) against the whole-cloud answer, the partition and the merge; returns the tiles"""
    C = tile_case(E)
    P, S, cuts = C["scan"], C["S"], C["cuts"]
    whole = whole_of(E, smooth, signed)
    owners = np.zeros(len(P), np.int32)
    tiles = []
    for t, (b, e) in enumerate(ranges3(S)):
        h = E.Engine(device_of(t), change_range=0, slice_begin=b, slice_end=e)
        h.set_cloud(P)
        mesh = h.trimesh(C["verts"], C["tris"], cell=cell)
        call = h.mesh_signed_deviation_tile if signed else h.mesh_deviation_tile
        tile = call(mesh, smooth_radius=smooth, **DP)
        none = call(mesh, smooth_radius=smooth, maps=False, **DP)
        assert all(x is None for x in none[:-1]) and same(none[-1], tile[-1])
        owners += check_tile(E, tile, whole[:-1], signed, cuts[b], cuts[e], "tile %d [%d, %d)" % (t, b, e), restatement)
        tiles.append(tile)
        mesh.close(); h.close()
    assert np.array_equal(owners == 1, finite_rows(P)) and owners.max() == 1            # the owned maps partition the indexed points
    merged = (E.merge_mesh_signed_deviation_tiles if signed else E.merge_mesh_deviation_tiles)(tiles)
    ws = whole[-1]
    print("merged %r\nwhole  %r" % ({k: v for k, v in merged.items() if k != "hist"}, {k: v for k, v in ws.items() if k != "hist"}))
    assert list(merged) == list(ws)
    for f in ws:
        assert same(merged[f], ws[f]), f
    return tiles


@pytest.mark.gpu
@pytest.mark.parametrize("signed", [False, True])
@pytest.mark.parametrize("smooth", [0.0, SMOOTH])
def test_tiles_equal_the_whole_mesh_deviation(engine_mod, smooth, signed):
    """three slice ranges: for every tile and owned point every map is the whole-cloud call's bytes and the restatement's, every
    other entry the fill, the owned maps partition the indexed points, the merge is the whole-cloud struct field for field by bits"""
    E = engine_mod
    tiles = tiles_of(E, smooth, signed, restatement=restated(E, smooth, signed))
    assert all(t[-1]["matched"] > 0 and t[-1]["too_far"] > 0 for t in tiles)
    n = len(tile_case(E)["scan"])
    assert tiles[1][-1]["evaluated"] < n                                      # a tile's launches cover its positions, not n
    if smooth:
        assert all(t[-1]["evaluated"] > t[-1]["owned"] for t in tiles)       # every tile evaluated halo points
    p = tile_case(E)["planted"]
    assert [int(t[-2][p]) for t in tiles] == [0, 1, 0]                        # x on the cut's float: the upper tile's alone


@pytest.mark.gpu
@pytest.mark.parametrize("cell", [0.9, 25.0])
def test_tiles_do_not_depend_on_the_grid(engine_mod, cell):
    """the tiles' meshes with a forced cell against the whole-cloud call's automatic one (the automatic cell on both sides is the
    test above): the answers do not depend on the grid"""
    for signed in (False, True):
        tiles_of(engine_mod, SMOOTH, signed, cell=cell)


@pytest.mark.gpu
def test_a_whole_cloud_handle_is_one_tile_that_owns_everything(engine_mod):
    E = engine_mod
    C = tile_case(E)
    P = C["scan"]
    h = handle(E, P)
    mesh = h.trimesh(C["verts"], C["tris"])
    for signed in (False, True):
        whole = whole_of(E, SMOOTH, signed)
        tile = (h.mesh_signed_deviation_tile if signed else h.mesh_deviation_tile)(mesh, smooth_radius=SMOOTH, **DP)
        mine = check_tile(E, tile, whole[:-1], signed, -np.inf, np.inf, "whole-cloud handle")
        assert np.array_equal(mine, finite_rows(P)) and tile[-1]["evaluated"] == tile[-1]["owned"] == mine.sum()
        for got, want in zip(tile[:-2], whole[:-1]):
            assert got.dtype == want.dtype and got.tobytes() == want.tobytes()
        merged = (E.merge_mesh_signed_deviation_tiles if signed else E.merge_mesh_deviation_tiles)([tile])
        assert same(merged, whole[-1])
    mesh.close(); h.close()


@pytest.mark.gpu
def test_mesh_deviation_tile_refusals_and_nothing_else_moved(engine_mod):
    E = engine_mod
    C = tile_case(E)
    P, S, cuts = C["scan"], C["S"], C["cuts"]
    rng = ranges3(S)[1]
    h, w = handle(E, P, rng), handle(E, P)
    mesh = w.trimesh(C["verts"], C["tris"])
    ok = dict(DP, smooth_radius=SMOOTH)

    def refused(e, m, code, **k):
        """the code, and not one launch on the handle: no index build, no kernel of the call"""
        e.enable_timing(True)
        e.kernel_times()
        for call in (e.mesh_deviation_tile, e.mesh_signed_deviation_tile):
            for maps in (False, True):
                with pytest.raises(E.PPPError) as ex:
                    call(m, maps=maps, **dict(ok, **k))
                assert ex.value.code == code, (k, maps, ex.value)
                launches = e.kernel_times(with_launches=True)[1]
                assert not any(launches.values()), (k, maps, launches)

    h.enable_timing(True)
    h.kernel_times()
    topo_before = mesh.topology(maps=False)
    first = h.mesh_signed_deviation_tile(mesh, **ok)                          # the accepted call all refusals below differ from
    launches = h.kernel_times(with_launches=True)[1]                          # (and the counter does see this call's kernels)
    assert all(launches.get(k) == 1 for k in ("k_mesht_fill", "k_mesht_nearest", "k_mesht_sign", "k_mesht_stats", "k_devt_smooth", "k_devt_target")), launches
    assert not any(launches.get(k) for k in ("k_mesh_nearest", "k_mesh_sign", "k_tm_region_stats", "k_dev_target"))
    for bad in (dict(max_dist=0.0), dict(max_dist=float("nan")), dict(smooth_radius=-1.0), dict(allowance=float("inf")), dict(gain=-1.0),
                dict(max_dist=float("inf"))):                                 # (smoothing needs a finite max_dist) as ppp_get_mesh_deviation
        refused(h, mesh, E.ERR_ARG, **bad)
    refused(h, None, E.ERR_ARG)
    # a margin that covers the owned interval and not smooth_radius beyond it: the index starts 2 mm below the lower
    # interior seam and ends 1 mm above the upper (a range indexes from int(px[sb]) - 2 - range_margin, the cut lies 12 mm below px[sb])
    thin = handle(E, P, rng, range_margin=12.0)
    lo, hi, _ = thin.range_interval(float(P[:, 0].min()), float(P[:, 0].max()))
    assert 0.0 < cuts[rng[0]] - lo < SMOOTH and 0.0 < hi - cuts[rng[1]] < SMOOTH
    refused(thin, mesh, E.ERR_ARG)
    bare = thin.mesh_deviation_tile(mesh, **dict(ok, smooth_radius=0.0))      # without smoothing the same handle answers
    check_tile(E, bare, whole_of(E, 0.0, False)[:-1], False, cuts[rng[0]], cuts[rng[1]], "thin margin, no smoothing")
    # a part handle
    f = finite_rows(P)
    mn, mx = P[f].min(axis=0), P[f].max(axis=0)
    p = E.Engine(0, slice_begin=rng[0], slice_end=rng[1], change_range=0)
    plo, phi, _ = p.range_interval(mn[0], mx[0])
    keep = np.nonzero(f & (P[:, 0] >= plo) & (P[:, 0] <= phi))[0]
    p.set_cloud_part(P[keep], keep, mn, mx, int(f.sum()), plo, phi)
    refused(p, mesh, E.ERR_UNSUPPORTED)
    empty = E.Engine(0, change_range=0)
    refused(empty, mesh, E.ERR_ARG)
    L = h.L
    part = E.MeshDeviationTileStats()
    assert L.ppp_get_mesh_deviation_tile(h.h, mesh.m, None, None, None, None, None, None, None, None, None, 0, ctypes.byref(part)) == E.ERR_ARG
    assert L.ppp_get_mesh_deviation_tile(None, mesh.m, None, None, None, None, None, None, None, None, None, 0, ctypes.byref(part)) == E.ERR_ARG
    # the whole-cloud calls still refuse a range handle
    for call in (h.mesh_deviation, h.mesh_signed_deviation):
        with pytest.raises(E.PPPError) as ex:
            call(mesh, **ok)
        assert ex.value.code == E.ERR_UNSUPPORTED
    # every refusal left the handle usable and the answer unchanged; the mesh's topology statistics are what they were
    again = h.mesh_signed_deviation_tile(mesh, **ok)
    assert same(again, first) and same(mesh.topology(maps=False), topo_before)
    check_tile(E, again, whole_of(E, SMOOTH, True)[:-1], True, cuts[rng[0]], cuts[rng[1]], "after the refusals")
    for e in (h, w, thin, p, empty):
        e.close()
    mesh.close()


@pytest.mark.gpu
def test_a_handle_that_ran_a_pass_keeps_its_results(engine_mod):
    """a range handle that planned a path and answered contact queries gives the tile a fresh range handle gives; its cloud, its
    plan and its stored contact results are as before"""
    from polishpathplanning_amd import synth
    from polishpathplanning_amd.robot_path import slice_ranges
    from test_contact_tiles import RANGE_MARGIN
    E = engine_mod
    pts, cfg = synth.make_config("small_40k")
    kw = dict(tool_radius=cfg["tool_radius"], walk=1)
    w = E.Engine(0, **kw)
    w.set_cloud(pts)
    S = w.gen_path()
    b, e = slice_ranges(S, 4)[1]
    a = E.Engine(0, slice_begin=b, slice_end=e, range_margin=RANGE_MARGIN, **kw)
    a.set_cloud(pts)
    a.gen_path(); a.get_path()
    cloud, fast, slices, contacts, covered = a.cloud().copy(), a.fast_path(), a.num_slices(), a.path_contacts(), a.path_coverage()
    f = finite_rows(pts)
    mn, mx = pts[f].min(axis=0), pts[f].max(axis=0)
    z = float(np.median(pts[f, 2]))                                           # a plate of two triangles through the cloud, in its file's units
    plate = np.array([[mn[0], mn[1], z], [mx[0], mn[1], z], [mx[0], mx[1], z], [mn[0], mx[1], z]], np.float32)
    mesh = a.trimesh(plate, np.array([[0, 1, 2], [0, 2, 3]], np.int32))
    dp = dict(max_dist=30.0, smooth_radius=4.0, allowance=0.05, gain=1.0)
    first = (a.mesh_deviation_tile(mesh, **dp), a.mesh_signed_deviation_tile(mesh, **dp), a.mesh_registration_terms_tile(mesh, max_dist=30.0))
    fresh = E.Engine(0, slice_begin=b, slice_end=e, range_margin=RANGE_MARGIN, **kw)
    fresh.set_cloud(pts)
    other = (fresh.mesh_deviation_tile(mesh, **dp), fresh.mesh_signed_deviation_tile(mesh, **dp), fresh.mesh_registration_terms_tile(mesh, max_dist=30.0))
    assert same(first, other) and first[0][-1]["matched"] > 0 and first[0][-1]["evaluated"] > first[0][-1]["owned"] and first[2][0]["pairs"] > 0
    assert same(a.cloud(), cloud) and a.fast_path() == fast and a.num_slices() == slices
    assert same(a.path_contacts(), contacts) and same(a.path_coverage(), covered)
    for x in (mesh, a, fresh, w):
        x.close()


@pytest.mark.gpu
def test_tiles_and_their_meshes_on_two_devices(engine_mod):
    """the tiles alternate between device 0 and device 1, each with a mesh of its own device: the one-device bits; a mesh on
    another device than its handle is refused"""
    if device_count() < 2:
        pytest.skip("needs two GPUs in one process: this machine shows %d" % device_count())
    E = engine_mod
    for signed in (False, True):
        tiles_of(E, SMOOTH, signed, device_of=lambda t: t % 2)
    C = tile_case(E)
    h = handle(E, C["scan"], ranges3(C["S"])[1])
    d1 = E.Engine(1, change_range=0)
    far = d1.trimesh(C["verts"], C["tris"])
    h.enable_timing(True)
    h.kernel_times()
    with pytest.raises(E.PPPError) as ex:
        h.mesh_deviation_tile(far, smooth_radius=SMOOTH, **DP)
    assert ex.value.code == E.ERR_ARG and not any(h.kernel_times(with_launches=True)[1].values())
    far.close(); d1.close(); h.close()
