"""Registration to a triangle mesh of a scan held as slice-range tiles (ppp_get_mesh_registration_terms_tile,
ppp_register_mesh_tiles).

Every comparison is for equality.  An evaluation is 29 integer sums over the scan's pairs, the owned sets of ranges that tile the
walk partition the indexed points and the mesh is whole on every device: the tiles' rows merged by ppp_merge_registration_terms must
be ppp_get_mesh_registration_terms' row on a whole-cloud handle in every word, and the tiled loop ppp_register_mesh's T, rows and
statistics, bit for bit -- and those of restate_mesh_terms() / restate_register_mesh() of tests/test_mesh_registration.py.  No
tolerance appears anywhere in this file.

The case is tests/test_mesh_deviation_tiles.py's: the long wavy sheet of 1 280 triangles and 3 000 scan points, carried off by a
degree and a few tenths of a millimetre; ownership goes by the resident, unmoved x of that moved cloud."""
import ctypes
import functools
import math
import os
import subprocess

import numpy as np
import pytest

from test_deviation_tiles import cuts_of, device_count, finite_rows, handle, ranges3
from test_mesh_deviation_tiles import MOTION, N_RAISED, N_SCAN, owned_by, tile_case
from test_mesh_registration import restate_mesh_terms, restate_register_mesh
from test_mesh_registration_adversaries import large_mesh_case
from test_path_dwell import same
from test_path_removal import past_the_grid_cap
from test_registration import ALL_LOCKED, IDENTITY, LARGE, NAN, motion_about, restate_step, rows_equal, stats_equal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECLS = ("int ppp_get_mesh_registration_terms_tile(ppp_handle h, ppp_trimesh m, const ppp_registration_params *rp,\n"
         "                                         const double *T12, ppp_registration_row *row, ppp_registration_part *part);",
         "int ppp_register_mesh_tiles(const ppp_handle *hs, const ppp_trimesh *ms, size_t count,\n"
         "                            const ppp_registration_params *rp, const double *T0_12, ppp_registration_row *rows,\n"
         "                            size_t row_cap, ppp_register_tiles_stats *stats);")
SYMBOLS = ("ppp_get_mesh_registration_terms_tile", "ppp_register_mesh_tiles")
SHORT = dict(max_dist=2.0, iterations=3, min_step=1e-6, lock_eps=1e-9)       # a chain that ends on `iterations`


def part_way(share):
    return motion_about(MOTION["c"], tuple(share * d for d in MOTION["deg"]), tuple(share * s for s in MOTION["shift"]))


@functools.lru_cache(maxsize=None)
def restated_chain(iterations):
    import polishpathplanning_amd.engine as E
    C = tile_case(E)
    return restate_register_mesh(C["moved"], C["verts"], C["tris"], iterations=iterations)


# ---------------------------------------------------------------- CPU


def test_header_declares_and_engine_exports_the_mesh_registration_tiles(engine_mod, tmp_path):
    hdr = open(os.path.join(ROOT, "include", "ppp_hip.h")).read()
    for decl in DECLS:
        assert decl in hdr, decl
    at = [hdr.index("int ppp_merge_mesh_signed_deviation_tiles(")] + [hdr.index(d) for d in DECLS] + [hdr.index("int ppp_eval_spline(")]
    assert at == sorted(at)
    assert "ppp_register_mesh_tiles (B.149)" in hdr and "one host round trip per evaluation, where ppp_register_mesh has\n   none" in hdr
    for sym in SYMBOLS:
        assert sym in engine_mod.EXPORTS and hasattr(engine_mod.lib(), sym), sym
    assert callable(engine_mod.Engine.mesh_registration_terms_tile) and callable(engine_mod.register_mesh_tiles)
    planner = open(os.path.join(ROOT, "include", "ppp_planner.hpp")).read()
    assert "inline bool register_mesh_tiles(std::vector<Planner *> &tiles, std::vector<TriMesh *> &meshes, ppp_register_tiles_stats &st," in planner
    assert "bool mesh_registration_terms_tile(const TriMesh &mesh, ppp_registration_row &row, ppp_registration_part &part, " in planner
    src = tmp_path / "c99.c"
    src.write_text('#include "ppp_hip.h"\nint main(void) {\n'
                   '    int (*f)(ppp_handle, ppp_trimesh, const ppp_registration_params *, const double *, ppp_registration_row *,\n'
                   '             ppp_registration_part *) = ppp_get_mesh_registration_terms_tile;\n'
                   '    int (*g)(const ppp_handle *, const ppp_trimesh *, size_t, const ppp_registration_params *, const double *,\n'
                   '             ppp_registration_row *, size_t, ppp_register_tiles_stats *) = ppp_register_mesh_tiles;\n'
                   '    return f == 0 || g == 0;\n}\n')
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_census_of_the_moved_case(engine_mod):
    """by restatement alone: the moved scan walks in at least 5 slices; at the identity and at the part-way transform every tile
    owns pairs and points without one, and the tiles' restated words add up to the whole cloud's; the chain from the identity
    converges, the short chain ends on its iterations"""
    E = engine_mod
    C = tile_case(E)
    P, S, cuts = C["moved"], C["mS"], C["mcuts"]
    assert S >= 5 and len(P) == N_SCAN
    for T in (IDENTITY, part_way(2.0 / 3.0)):
        whole = restate_mesh_terms(P, C["verts"], C["tris"], 2.0, T)
        paired = np.zeros(len(P), bool)
        paired[np.nonzero(finite_rows(P))[0][whole["paired"]]] = True
        total = 0
        for b, e in ranges3(S):
            mine = owned_by(P, cuts[b], cuts[e])
            print("tile [%g, %g): %d owned, %d paired" % (cuts[b], cuts[e], mine.sum(), (mine & paired).sum()))
            assert (mine & paired).sum() >= 100 and (mine & ~paired).any()
            total += int((mine & paired).sum())
        assert total == whole["pairs"] and np.any(whole["b"])
    T, rows, st = restated_chain(30)
    print("steps %d converged %d pairs %d -> %d rms %r -> %r" % (st["steps"], st["converged"], st["pairs_before"], st["pairs_after"], st["rms_before"], st["rms_after"]))
    assert st["converged"] == 1 and 2 <= st["steps"] < 30 and st["rms_after"] < st["rms_before"]
    clean = np.arange(N_SCAN) >= N_RAISED
    err = lambda T: float(np.abs((P[clean].astype(np.float64) @ T[:, :3].T + T[:, 3]) - C["scan"][clean]).max())
    assert err(T) < 0.1 < err(IDENTITY)
    T3, rows3, st3 = restated_chain(SHORT["iterations"])
    assert st3["steps"] == SHORT["iterations"] == len(rows3) - 1 and st3["converged"] == 0 and rows3[-1]["locked"] == ALL_LOCKED


# ---------------------------------------------------------------- GPU


def open_tiles(E, P, S, v, t, device_of=lambda i: 0, one_mesh=True, orient_of=lambda i: 0):
    """the range handles of ranges3(S) and their meshes: one mesh for all of them, or one per tile"""
    hs = []
    for i, (b, e) in enumerate(ranges3(S)):
        h = E.Engine(device_of(i), change_range=0, slice_begin=b, slice_end=e)
        h.set_cloud(P)
        hs.append(h)
    if one_mesh:
        ms = [hs[0].trimesh(v, t)] * len(hs)
    else:
        ms = [h.trimesh(v, t, orient=orient_of(i), viewpoint=(50.0, 20.0, 500.0) if orient_of(i) else None) for i, h in enumerate(hs)]
    return hs, ms


def close_all(hs, ms):
    for m in {id(m): m for m in ms}.values():
        m.close()
    for h in hs:
        h.close()


def check_terms(E, hs, ms, s, mesh, P, cuts, S, v, t, T, max_dist=2.0):
    """the tiles' rows at T: the merge is the whole-cloud call's row and the restatement's in every word; the parts' owned add up
    to the indexed count; every part carries the whole call's frame"""
    row, st = s.mesh_registration_terms(mesh, T=T, max_dist=max_dist)
    tiles = [h.mesh_registration_terms_tile(m, T=T, max_dist=max_dist) for h, m in zip(hs, ms)]
    merged, whole = E.merge_registration_terms(tiles, T=T)
    rows_equal([merged], [row])
    for (r, p), (b, e) in zip(tiles, ranges3(S)):
        mine = owned_by(P, cuts[b], cuts[e])
        print("tile [%g, %g): owned %d evaluated %d pairs %d" % (cuts[b], cuts[e], p["owned"], p["evaluated"], r["pairs"]))
        assert p["owned"] == mine.sum() and p["evaluated"] >= p["owned"] and (np.float32(p["own_lo"]), np.float32(p["own_hi"])) == (cuts[b], cuts[e])
        assert (p["n"], p["shift"]) == (st["n"], st["shift"]) and same(p["centre"], st["centre"]) and same(p["length"], st["length"])
        assert r["locked"] == ALL_LOCKED and math.isnan(r["step2"]) and same(r["T"], row["T"])
    assert whole["owned"] == st["indexed"] == sum(p["owned"] for _, p in tiles)
    return row, st, tiles


@pytest.mark.gpu
def test_merged_terms_equal_the_whole_call_and_the_restatement(engine_mod):
    E = engine_mod
    C = tile_case(E)
    P, S, cuts, v, t = C["moved"], C["mS"], C["mcuts"], C["verts"], C["tris"]
    s = handle(E, P)
    mesh = s.trimesh(v, t)
    hs, ms = open_tiles(E, P, S, v, t)
    for T in (None, part_way(2.0 / 3.0)):
        row, st, tiles = check_terms(E, hs, ms, s, mesh, P, cuts, S, v, t, T)
        want = restate_mesh_terms(s.cloud(), v, t, 2.0, IDENTITY if T is None else T)
        want.update(locked=ALL_LOCKED, step2=NAN)
        rows_equal([row], [want])
        assert all(r["pairs"] > 0 for r, _ in tiles) and tiles[1][1]["evaluated"] < len(P)      # the interior tile visits its positions, not n
        again = [h.mesh_registration_terms_tile(m, T=T) for h, m in zip(hs, ms)]
        assert same(again, tiles)                                            # the same bits in every run
        # the step the host takes from the merged row is the restatement's
        merged, whole = E.merge_registration_terms(tiles, T=T)
        step = restate_step(want, want["centre"], want["length"], 1e-9)
        code, Tn, locked, step2 = E.registration_step(merged, whole, 1e-9)
        assert code == E.STEP_TAKEN and step is not None and locked == step[0] and same(Tn, step[2]) and same(step2, step[3])
    # a whole-cloud handle as a tile owns every indexed point: its row is the whole call's
    r1, p1 = s.mesh_registration_terms_tile(mesh)
    rows_equal([r1], [s.mesh_registration_terms(mesh)[0]])
    assert p1["owned"] == p1["evaluated"] == int(finite_rows(P).sum())
    close_all(hs, ms)
    mesh.close(); s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kw", [dict(), SHORT], ids=["known-motion", "ends-on-iterations"])
def test_tiled_loop_equals_register_mesh(engine_mod, kw):
    """ppp_register_mesh_tiles against ppp_register_mesh on a whole-cloud handle and against the restatement: T, every row, every
    field of the statistics; with one mesh in every slot, with a mesh per tile of which one is oriented the other way, and with a
    single whole-cloud handle as the only tile"""
    E = engine_mod
    C = tile_case(E)
    P, S, v, t = C["moved"], C["mS"], C["verts"], C["tris"]
    s = handle(E, P)
    mesh = s.trimesh(v, t)
    T, rows, st = s.register_mesh(mesh, **kw)
    wT, wrows, wst = restated_chain(kw.get("iterations", 30))
    rows_equal(rows, wrows)
    stats_equal(st, wst)
    print("steps %d converged %d pairs %d -> %d" % (st["steps"], st["converged"], st["pairs_before"], st["pairs_after"]))
    assert (st["steps"] == SHORT["iterations"] and st["converged"] == 0) if kw else st["converged"] == 1
    for one_mesh in (True, False):
        hs, ms = open_tiles(E, P, S, v, t, one_mesh=one_mesh, orient_of=lambda i: int(i == 1))
        tT, trows, tst = E.register_mesh_tiles(hs, ms[0] if one_mesh else ms, **kw)
        assert same(tT, T) and len(trows) == len(rows)
        rows_equal(trows, rows)
        stats_equal(tst, st)
        close_all(hs, ms)
    oT, orows, ost = E.register_mesh_tiles([s], mesh, **kw)
    assert same(oT, T)
    rows_equal(orows, rows)
    stats_equal(ost, st)
    mesh.close(); s.close()


@pytest.mark.gpu
def test_a_tile_past_the_grid_cap(engine_mod):
    """the 141 877 points of tests/test_mesh_registration_adversaries.py, cut into all slices but the last and the last: the first
    tile alone holds more positions than k_mesht_reg_sum's capped grid has threads, so its grid-stride loop takes a second trip.
    The merged terms are the whole-cloud call's, which that file pins to the restatement"""
    E = engine_mod
    v, t, scan, raised, T0 = large_mesh_case()
    S, cuts = cuts_of(E, scan)
    s = handle(E, scan)
    mesh = s.trimesh(v, t)
    row, st = s.mesh_registration_terms(mesh, T=T0, max_dist=LARGE["max_dist"])
    tiles = []
    for b, e in ((0, S - 1), (S - 1, S)):
        h = handle(E, scan, (b, e))
        tiles.append(h.mesh_registration_terms_tile(mesh, T=T0, max_dist=LARGE["max_dist"]))
        h.close()
    past_the_grid_cap(tiles[0][1]["evaluated"])
    merged, whole = E.merge_registration_terms(tiles, T=T0)
    rows_equal([merged], [row])
    print("pairs %d + %d = %d" % (tiles[0][0]["pairs"], tiles[1][0]["pairs"], row["pairs"]))
    assert whole["owned"] == st["indexed"] == len(scan) - 2 and tiles[1][1]["owned"] > 0 and min(r["pairs"] for r, _ in tiles) > 0
    mesh.close(); s.close()


@pytest.mark.gpu
def test_mesh_registration_tile_refusals(engine_mod):
    E = engine_mod
    C = tile_case(E)
    P, S, v, t = C["moved"], C["mS"], C["verts"], C["tris"]
    hs, ms = open_tiles(E, P, S, v, t)
    mesh = ms[0]
    L = E.lib()

    def refused(code, call):
        with pytest.raises(E.PPPError) as ex:
            call()
        assert ex.value.code == code, ex.value

    # a part handle
    f = finite_rows(P)
    mn, mx = P[f].min(axis=0), P[f].max(axis=0)
    b, e = ranges3(S)[1]
    p = E.Engine(0, slice_begin=b, slice_end=e, change_range=0)
    lo, hi, _ = p.range_interval(mn[0], mx[0])
    keep = np.nonzero(f & (P[:, 0] >= lo) & (P[:, 0] <= hi))[0]
    p.set_cloud_part(P[keep], keep, mn, mx, int(f.sum()), lo, hi)
    refused(E.ERR_UNSUPPORTED, lambda: p.mesh_registration_terms_tile(mesh))
    refused(E.ERR_UNSUPPORTED, lambda: E.register_mesh_tiles([hs[0], p, hs[2]], mesh))
    # meshes that disagree: one triangle fewer, and the same triangles moved by a float
    fewer = hs[0].trimesh(v, t[:-1])
    v2 = v.copy()
    v2[:, 2] += np.float32(0.5)
    lifted = hs[0].trimesh(v2, t)
    for other in (fewer, lifted):
        refused(E.ERR_ARG, lambda: E.register_mesh_tiles(hs, [mesh, other, mesh]))
    # a handle twice, NULLs, bad parameters, rows NULL with a cap
    refused(E.ERR_ARG, lambda: E.register_mesh_tiles([hs[0], hs[1], hs[0]], mesh))
    refused(E.ERR_ARG, lambda: E.register_mesh_tiles(hs, [mesh, None, mesh]))
    refused(E.ERR_ARG, lambda: E.register_mesh_tiles(hs, [mesh, mesh]))
    refused(E.ERR_ARG, lambda: hs[1].mesh_registration_terms_tile(None))
    for bad in (dict(max_dist=0.0), dict(max_dist=float("inf")), dict(iterations=0), dict(iterations=65), dict(min_step=-1.0), dict(lock_eps=1.0)):
        refused(E.ERR_ARG, lambda: E.register_mesh_tiles(hs, mesh, **bad))
    bad_T = IDENTITY.copy()
    bad_T[1, 2] = float("nan")
    refused(E.ERR_ARG, lambda: E.register_mesh_tiles(hs, mesh, T0=bad_T))
    refused(E.ERR_ARG, lambda: hs[1].mesh_registration_terms_tile(mesh, T=bad_T))
    rp = E.RegistrationParams(2.0, 5, 1e-6, 1e-9)
    st = E.RegisterTilesStats()
    harr = (ctypes.c_void_p * 3)(*[h.h for h in hs])
    marr = (ctypes.c_void_p * 3)(*[m.m for m in ms])
    assert L.ppp_register_mesh_tiles(None, marr, 3, ctypes.byref(rp), None, None, 0, ctypes.byref(st)) == E.ERR_ARG
    assert L.ppp_register_mesh_tiles(harr, None, 3, ctypes.byref(rp), None, None, 0, ctypes.byref(st)) == E.ERR_ARG
    assert L.ppp_register_mesh_tiles(harr, marr, 0, ctypes.byref(rp), None, None, 0, ctypes.byref(st)) == E.ERR_ARG
    assert L.ppp_register_mesh_tiles(harr, marr, 3, None, None, None, 0, ctypes.byref(st)) == E.ERR_ARG
    assert L.ppp_register_mesh_tiles(harr, marr, 3, ctypes.byref(rp), None, None, 4, ctypes.byref(st)) == E.ERR_ARG
    assert L.ppp_register_mesh_tiles(harr, marr, 3, ctypes.byref(rp), None, None, 0, ctypes.byref(st)) == 0 and st.failed_tile == -1
    assert L.ppp_get_mesh_registration_terms_tile(None, mesh.m, ctypes.byref(rp), None, None, None) == E.ERR_ARG
    assert L.ppp_get_mesh_registration_terms_tile(hs[1].h, mesh.m, None, None, None, None) == E.ERR_ARG
    # the whole-cloud calls still refuse a range handle
    refused(E.ERR_UNSUPPORTED, lambda: hs[1].mesh_registration_terms(mesh))
    refused(E.ERR_UNSUPPORTED, lambda: hs[1].register_mesh(mesh))
    # every refusal left the handles usable
    T, rows, st2 = E.register_mesh_tiles(hs, mesh)
    wT, wrows, wst = restated_chain(30)
    rows_equal(rows, wrows)
    for x in (fewer, lifted, p):
        x.close()
    close_all(hs, ms)


@pytest.mark.gpu
def test_tiles_and_their_meshes_on_two_devices(engine_mod):
    """tiles on devices 0, 1, 0, each with a mesh on its own device: the one-device bits; a mesh on another device than its tile
    is refused with the tile's slot"""
    if device_count() < 2:
        pytest.skip("needs two GPUs in one process: this machine shows %d" % device_count())
    E = engine_mod
    C = tile_case(E)
    P, S, v, t = C["moved"], C["mS"], C["verts"], C["tris"]
    hs, ms = open_tiles(E, P, S, v, t, device_of=lambda i: i % 2, one_mesh=False)
    T, rows, st = E.register_mesh_tiles(hs, ms)
    wT, wrows, wst = restated_chain(30)
    rows_equal(rows, wrows)
    stats_equal(st, wst)
    assert same(T, wT)
    with pytest.raises(E.PPPError) as ex:
        E.register_mesh_tiles(hs, [ms[0], ms[0], ms[2]])
    assert ex.value.code == E.ERR_ARG and "tile 1" in str(ex.value)
    with pytest.raises(E.PPPError) as ex:
        hs[1].mesh_registration_terms_tile(ms[0])
    assert ex.value.code == E.ERR_ARG
    close_all(hs, ms)
