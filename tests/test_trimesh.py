"""The resident triangle mesh and the exact point-to-triangle search (ppp_trimesh_create, ppp_trimesh_nearest,
ppp_get_mesh_deviation).  The yardstick is nearest_on_mesh(): the rule of include/ppp_hip.h in numpy float64 as a
brute force over ALL triangles with the minimum over (D2, f).  It knows nothing of a grid, so a search that stops early, skips
a cell or clamps wrongly shows as unequal bits.  The CPU tests check the restatement itself against bounds that are derived,
not measured."""
import functools
import math
import os

import numpy as np
import pytest

from test_mesh_cloud import rand_triangles, resident, same_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MATCHED, TOO_FAR, NO_NORMAL, DROPPED = range(4)
FACE, EDGE, VERTEX, NONE = 0, 1, 2, 255
WINDING, VIEWPOINT = 0, 1
INF = float("inf")
MAPS = ("distance", "closest", "deviation", "tri_index", "region", "status")
# the seven branches of the walk, in the order the rule tests them, and the region each one reports
BRANCH_REGION = np.array([VERTEX, VERTEX, EDGE, VERTEX, EDGE, EDGE, FACE], np.uint8)


# ---------------------------------------------------------------- the restatement


def dot(u, v):
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def frames(rv, tris):
    """7s's frame of every triangle on the resident vertices rv float32[nv, 3] (tris int[nt, 3] or None for a soup):
    (p0, p1, p2 float64[nt, 3], N, A2, valid)"""
    rv = np.ascontiguousarray(rv, np.float32).reshape(-1, 3)
    idx = np.arange(len(rv) // 3 * 3).reshape(-1, 3) if tris is None else np.asarray(tris, np.int64).reshape(-1, 3)
    inside = ((idx >= 0) & (idx < len(rv))).all(axis=1)
    v = rv[np.where(inside[:, None], idx, 0)].astype(np.float64)
    finite = np.isfinite(v).all(axis=(1, 2))
    v = np.where(finite[:, None, None], v, 0.0)

    def len2(a, b):
        d = b - a
        return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]

    ab, bc, ca = len2(v[:, 0], v[:, 1]), len2(v[:, 1], v[:, 2]), len2(v[:, 2], v[:, 0])
    first = np.where((ab >= bc) & (ab >= ca), 0, np.where(bc >= ca, 1, 2))
    r = np.arange(len(v))
    p0, p1, p2 = v[r, first], v[r, (first + 1) % 3], v[r, (first + 2) % 3]
    e1, e2 = p1 - p0, p2 - p0
    N = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2], e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1)
    A2 = np.sqrt((N[:, 0] * N[:, 0] + N[:, 1] * N[:, 1]) + N[:, 2] * N[:, 2])
    valid = inside & finite & (A2 > 0) & np.isfinite(A2)
    return p0, p1, p2, N, A2, valid


def closest_on_triangles(p, a, b, c):
    """Ericson's region walk, every written operation once, on arrays that broadcast to [..., 3]: (x, D2, branch 0 .. 6)"""
    with np.errstate(all="ignore"):
        ab, ac, ap = b - a, c - a, p - a
        d1, d2 = dot(ab, ap), dot(ac, ap)
        bp = p - b
        d3, d4 = dot(ab, bp), dot(ac, bp)
        vc = d1 * d4 - d3 * d2
        cp = p - c
        d5, d6 = dot(ab, cp), dot(ac, cp)
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
                 (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & ((d4 - d3) >= 0) & ((d5 - d6) >= 0)]
        branch = np.full(conds[0].shape, 6, np.int64)
        for k in range(5, -1, -1):                                            # the first test that holds decides
            branch = np.where(conds[k], k, branch)
        v3 = d1 / (d1 - d3)
        w5 = d2 / (d2 - d6)
        w6 = (d4 - d3) / ((d4 - d3) + (d5 - d6))
        den = 1.0 / ((va + vb) + vc)
        v7, w7 = vb * den, vc * den
        full = np.broadcast_shapes(p.shape, a.shape)
        xs = [np.broadcast_to(a, full), np.broadcast_to(b, full), a + ab * v3[..., None], np.broadcast_to(c, full), a + ac * w5[..., None],
              b + (c - b) * w6[..., None], (a + ab * v7[..., None]) + ac * w7[..., None]]
        x = np.zeros(full)
        for k in range(7):
            x = np.where((branch == k)[..., None], xs[k], x)
        e = p - x
        D2 = (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]
    return x, D2, branch


def nearest_on_mesh(rv, tris, P, max_dist=INF, orient=WINDING, vp=(0.0, 0.0, 0.0), chunk=256):
    """dict of the six maps (and D2) for the queries P float32[n, 3] in resident units: brute force over all indexed triangles"""
    P = np.ascontiguousarray(P, np.float32).reshape(-1, 3)
    n = len(P)
    p0, p1, p2, N, A2, valid = frames(rv, tris)
    fi = np.nonzero(valid)[0]                                                # ascending f: the first minimum is the lowest index
    a, b, c = p0[fi][None], p1[fi][None], p2[fi][None]
    md2 = float(np.float32(max_dist)) * float(np.float32(max_dist))
    out = dict(distance=np.full(n, np.nan), closest=np.full((n, 3), np.nan), deviation=np.full(n, np.nan), tri_index=np.full(n, -1, np.int32),
               region=np.full(n, NONE, np.uint8), status=np.full(n, DROPPED, np.uint8), D2=np.full(n, np.nan), branch=np.full(n, -1, np.int64))
    ok = np.isfinite(P).all(axis=1)
    vpd = np.asarray(vp, np.float64)
    for s in range(0, n, chunk):
        rows = np.nonzero(ok[s:s + chunk])[0] + s
        if not len(rows):
            continue
        if not len(fi):
            out["status"][rows] = TOO_FAR
            continue
        p = P[rows].astype(np.float64)
        x, D2, branch = closest_on_triangles(p[:, None, :], a, b, c)
        j = D2.argmin(axis=1)
        r = np.arange(len(rows))
        best = D2[r, j]
        hit = best <= md2
        out["status"][rows] = np.where(hit, MATCHED, TOO_FAR)
        rows, j, r = rows[hit], j[hit], r[hit]
        f = fi[j]
        xx = x[r, j]
        e = p[r] - xx
        with np.errstate(all="ignore"):
            nn = N[f] / A2[f][:, None]
        if orient == VIEWPOINT:
            s_ = (N[f, 0] * (vpd[0] - p0[f, 0]) + N[f, 1] * (vpd[1] - p0[f, 1])) + N[f, 2] * (vpd[2] - p0[f, 2])
            nn = np.where((s_ < 0)[:, None], -nn, nn)
        out["tri_index"][rows] = f
        out["region"][rows] = BRANCH_REGION[branch[r, j]]
        out["branch"][rows] = branch[r, j]
        out["distance"][rows] = np.sqrt(best[hit])
        out["D2"][rows] = best[hit]
        out["closest"][rows] = xx
        out["deviation"][rows] = ((e[:, 0] * nn[:, 0]) + e[:, 1] * nn[:, 1]) + e[:, 2] * nn[:, 2]
    return out


def got_maps(mesh, P, max_dist=INF):
    return dict(zip(MAPS, mesh.nearest(P, max_dist)))


def assert_same_maps(got, want, what=""):
    for k in MAPS:
        g, w = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert g.shape == w.shape and g.dtype == w.dtype, (what, k, g.shape, w.shape, g.dtype, w.dtype)
        if g.tobytes() != w.tobytes():
            gb, wb = (np.frombuffer(z.tobytes(), np.uint8).reshape(len(z), -1) for z in (g, w))
            bad = np.nonzero((gb != wb).any(axis=1))[0]
            raise AssertionError("%s: map %s differs at %d of %d entries, first at %s: got %r, want %r" % (what, k, len(bad), len(g), bad[:5], g[bad[:3]], w[bad[:3]]))


# ---------------------------------------------------------------- CPU: the restatement itself


def cpu_case(seed=11, nt=40, nq=50):
    rng = np.random.default_rng(seed)
    tri = rand_triangles(rng, nt, 4.0, 10.0)                                  # coordinates within +-14
    q = rng.uniform(-16, 16, (nq, 3)).astype(np.float32)
    return tri, q


def test_header_declares_and_engine_exports_the_trimesh_calls(engine_mod):
    txt = open(os.path.join(ROOT, "include", "ppp_hip.h")).read()
    for name in ("ppp_default_trimesh_params", "ppp_trimesh_create", "ppp_trimesh_create_stl", "ppp_trimesh_destroy", "ppp_trimesh_nearest",
                 "ppp_get_mesh_deviation"):
        assert name + "(" in txt and name in engine_mod.EXPORTS, name
    for name in ("trimesh", "trimesh_stl", "mesh_deviation"):
        assert hasattr(engine_mod.Engine, name), name
    assert hasattr(engine_mod.TriMesh, "nearest") and hasattr(engine_mod.TriMesh, "close")
    assert "no call\n * measures a point against a triangle" not in txt


def test_walk_reaches_all_seven_branches_and_stays_inside():
    tri, q = cpu_case()
    a, b, c = (tri[:, k].astype(np.float64)[None] for k in range(3))
    x, D2, branch = closest_on_triangles(q.astype(np.float64)[:, None, :], a, b, c)
    counts = np.bincount(branch.ravel(), minlength=7)
    print("pairs by branch (a, b, ab, c, ac, bc, face):", counts)
    assert (counts > 0).all()
    # the barycentric weights of x as ratios of signed areas: wa = ((b - x) x (c - x)) . n / (n . n), n = ab x ac, and so on.
    # Slack: every coordinate is below B = 32, so a difference is below 2 B and a cross product's component below 8 B^2, with a
    # few eps of that as rounding; x itself is a sum of three products of coordinates with weights <= 1, so it sits within a few
    # eps B of its exact place, which moves a cross product by at most 2 (2 B) times that.  Together the numerator is off by
    # less than 256 eps B^2 |n|, and the weight by that over n . n: 256 eps B^2 / A2 per triangle, A2 = |n| twice its area
    def cross(u, v):
        return np.stack([u[..., 1] * v[..., 2] - u[..., 2] * v[..., 1], u[..., 2] * v[..., 0] - u[..., 0] * v[..., 2], u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]], axis=-1)

    assert np.abs(tri).max() < 32 and np.abs(q).max() < 32
    n = cross(b - a, c - a)
    nn = dot(n, n)
    eps, B = np.finfo(np.float64).eps, 32.0
    slack = 256 * eps * B * B / np.sqrt(nn)
    wa, wb, wc = dot(cross(b - x, c - x), n) / nn, dot(cross(c - x, a - x), n) / nn, dot(cross(a - x, b - x), n) / nn
    print("largest slack %.3e; weights in [%.17g, %.17g], their sum off 1 by %.3e" % (slack.max(), min(wa.min(), wb.min(), wc.min()),
                                                                                    max(wa.max(), wb.max(), wc.max()), np.abs(wa + wb + wc - 1).max()))
    for w in (wa, wb, wc):
        assert (w >= -slack).all() and (w <= 1 + slack).all()
    assert (np.abs(wa + wb + wc - 1) <= 3 * slack).all()                      # x lies in the triangle's plane


def test_walk_against_a_barycentric_lattice():
    """every point of a triangle is within L / N of a lattice point (a lattice cell is the triangle scaled by 1 / N: its diameter
    is L / N), the vertices belong to the lattice, and lattice points lie on the triangle: distance <= d_lattice (up to
    rounding, 1e-12 relative) and d_lattice <= distance + L / N"""
    tri, q = cpu_case(seed=12, nt=12, nq=40)
    Nsub = 48
    i, j = np.meshgrid(np.arange(Nsub + 1), np.arange(Nsub + 1), indexing="ij")
    keep = i + j <= Nsub
    s, t = i[keep] / Nsub, j[keep] / Nsub
    for f in range(len(tri)):
        a, b, c = (tri[f, k].astype(np.float64) for k in range(3))
        lattice = a[None] + (b - a)[None] * s[:, None] + (c - a)[None] * t[:, None]
        L = math.sqrt(max(dot(b - a, b - a), dot(c - a, c - a), dot(c - b, c - b)))
        x, D2, _ = closest_on_triangles(q.astype(np.float64), a[None], b[None], c[None])
        dist = np.sqrt(D2)
        d_lat = np.sqrt(((q.astype(np.float64)[:, None, :] - lattice[None]) ** 2).sum(axis=2)).min(axis=1)
        assert (dist <= d_lat * (1 + 1e-12)).all(), f
        assert (d_lat <= dist + L / Nsub).all(), f


def test_walk_on_the_triangle_itself_gives_zero():
    a, b, c = (np.array(v, np.float64) for v in ([0, 0, 0], [4, 0, 0], [0, 4, 0]))
    for q, branch in (([0, 0, 0], 0), ([4, 0, 0], 1), ([0, 4, 0], 3), ([2, 0, 0], 2), ([0, 2, 0], 4), ([2, 2, 0], 5), ([1, 1, 0], 6)):
        x, D2, br = closest_on_triangles(np.array(q, np.float64), a, b, c)
        assert D2 == 0 and br == branch and (x == np.array(q)).all(), (q, x, D2, br)
    assert list(BRANCH_REGION[[0, 1, 3]]) == [VERTEX] * 3 and list(BRANCH_REGION[[2, 4, 5]]) == [EDGE] * 3 and BRANCH_REGION[6] == FACE


def test_restatement_picks_the_lower_index_on_a_tie_and_skips_degenerates():
    v = np.array([[0, 0, 0], [2, 0, 0], [0, 2, 0], [2, 2, 0], [np.nan, 0, 0]], np.float32)
    tris = np.array([[1, 2, 3], [0, 1, 2], [0, 1, 4], [0, 0, 1], [0, 1, 7]], np.int32)  # two that share an edge, a NaN, zero area, out of range
    r = nearest_on_mesh(v, tris, np.array([[1, 1, 3], [np.inf, 0, 0], [50, 50, 0]], np.float32), max_dist=10.0)
    assert list(r["status"]) == [MATCHED, DROPPED, TOO_FAR] and list(r["tri_index"]) == [0, -1, -1]
    assert r["region"][0] == EDGE and r["distance"][0] == 3.0 and r["deviation"][0] in (3.0, -3.0)
    assert frames(v, tris)[5].tolist() == [True, True, False, False, False]


# ---------------------------------------------------------------- GPU


def file_units(rv_wanted, change_range):
    """vertices in the file's units whose conversion is wanted (change_range: metres)"""
    return (rv_wanted / np.float32(1000)).astype(np.float32) if change_range else rv_wanted


@functools.lru_cache(maxsize=None)
def soup_case(change_range):
    rng = np.random.default_rng(5)
    n = 200
    size = rng.uniform(0.5, 6.0, (n, 1, 1))
    tri = (rng.uniform(-50, 50, (n, 1, 3)) + rng.uniform(-1, 1, (n, 3, 3)) * size).astype(np.float32)
    return file_units(tri.reshape(-1, 3), change_range)


def soup_queries(rv, stats, rng):
    mn, mx = rv.min(axis=0).astype(np.float64), rv.max(axis=0).astype(np.float64)
    ext = mx - mn
    q = [rng.uniform(mn, mx, (1000, 3))]
    for d in range(3):                                                       # outside on every side, and 10 x outside
        for sign in (-1, 1):
            for far in (1.0, 10.0):
                p = rng.uniform(mn, mx, (50, 3))
                p[:, d] = (mx[d] if sign > 0 else mn[d]) + sign * rng.uniform(0.01, 1.0, 50) * far * ext[d]
                q.append(p)
    q.append(rng.uniform(mn - 10 * ext, mx + 10 * ext, (100, 3)))            # outside on several axes at once
    q.append(rv[rng.integers(0, len(rv), 150)].astype(np.float64))           # exactly on vertices
    cell, gm, cells = float(stats["cell"]), stats["mn"].astype(np.float64), stats["cells"]
    for d in range(3):                                                       # exactly on cell faces of the automatic grid
        p = rng.uniform(mn, mx, (60, 3))
        p[:, d] = gm[d] + rng.integers(0, cells[d] + 1, 60) * cell
        q.append(p)
    return np.concatenate(q).astype(np.float32)


@functools.lru_cache(maxsize=None)
def soup_reference(change_range, engine_mod):
    verts = soup_case(change_range)
    rv = resident(engine_mod, verts, change_range)
    e = engine_mod.Engine(0, change_range=change_range)
    m = e.trimesh(verts)
    q = soup_queries(rv, m.stats, np.random.default_rng(6))
    m.close()
    e.close()
    return rv, q, nearest_on_mesh(rv, None, q)


@pytest.mark.gpu
@pytest.mark.parametrize("change_range", [0, 1])
def test_random_soup_matches_the_brute_force_for_every_cell(engine_mod, change_range):
    verts = soup_case(change_range)
    rv, q, want = soup_reference(change_range, engine_mod)
    assert len(q) >= 2000 and (want["status"] == MATCHED).all()
    print("winners by region (face, edge, vertex):", np.bincount(want["region"], minlength=3)[:3])
    ext = float((rv.max(axis=0).astype(np.float64) - rv.min(axis=0)).max())
    e = engine_mod.Engine(0, change_range=change_range)
    for what, cell in (("automatic", 0.0), ("box / 64", ext / 64), ("one cell", 2 * ext), ("no divisor", ext / 7.3)):
        m = e.trimesh(verts, cell=cell)
        print("%s: %s" % (what, {k: v for k, v in m.stats.items() if k not in ("mn", "mx")}))
        assert m.stats["indexed"] == 200 and m.stats["degenerate"] == 0
        assert same_bits(m.stats["mn"], rv.min(axis=0)) and same_bits(m.stats["mx"], rv.max(axis=0))
        if what == "one cell":
            assert m.stats["cells"] == (1, 1, 1) and m.stats["pairs"] == 200 == m.stats["max_per_cell"]
        got = got_maps(m, q)
        assert_same_maps(got, want, what)
        again = got_maps(m, q)                                               # twice: the same bits
        assert_same_maps(again, got, what + ", second run")
        m.close()
    e.close()


def sheet(nx, ny, pitch, wave=0.0):
    """(verts float32[(nx + 1)(ny + 1), 3], tris int32[2 nx ny, 3]): a grid mesh with shared vertices"""
    x, y = np.meshgrid(np.arange(nx + 1) * pitch, np.arange(ny + 1) * pitch, indexing="ij")
    z = wave * np.sin(x * 0.3) * np.cos(y * 0.2)
    v = np.stack([x, y, z], axis=2).reshape(-1, 3).astype(np.float32)
    i, j = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    k = (i * (ny + 1) + j).ravel()
    t = np.concatenate([np.stack([k, k + ny + 1, k + 1], axis=1), np.stack([k + 1, k + ny + 1, k + ny + 2], axis=1)])
    return v, t.astype(np.int32)


@pytest.mark.gpu
def test_indexed_sheet_ties_go_to_the_lower_index(engine_mod):
    v, t = sheet(8, 8, 2.0)
    e = engine_mod.Engine(0, change_range=0)
    rv = resident(engine_mod, v, 0)
    mids = (rv[t[:, 0]] + rv[t[:, 1]]) * np.float32(0.5)                      # on edges (exact: the pitch is a power of two)
    q = np.concatenate([rv + np.float32([0, 0, 1.5]), mids + np.float32([0, 0, 0.75]), rv - np.float32([0, 0, 2.0])]).astype(np.float32)
    want = nearest_on_mesh(rv, t, q)
    # straight above a vertex or an edge every triangle around it is at the same D2: the brute force must have had ties to break
    a, b, c = (rv[t[:, k]].astype(np.float64)[None] for k in range(3))
    _, D2, _ = closest_on_triangles(q.astype(np.float64)[:, None, :], a, b, c)
    ties = (D2 == D2.min(axis=1, keepdims=True)).sum(axis=1)
    print("queries by number of tied triangles:", np.bincount(ties))
    assert (ties >= 2).sum() > len(q) // 2
    for cell in (0.0, 3.1):
        m = e.trimesh(v, t, cell=cell)
        assert_same_maps(got_maps(m, q), want, "cell %g" % cell)
        m.close()
    e.close()


@pytest.mark.gpu
def test_one_triangle_across_the_box_among_many_small_ones(engine_mod):
    rng = np.random.default_rng(8)
    small = rand_triangles(rng, 300, 1.0, 30.0)
    big = np.array([[[-31, -31, -31], [31, 31, 28], [-29, 31, 31]]], np.float32)
    verts = np.concatenate([small[:150], big, small[150:]]).reshape(-1, 3)
    rv = resident(engine_mod, verts, 0)
    q = rng.uniform(-35, 35, (1200, 3)).astype(np.float32)
    want = nearest_on_mesh(rv, None, q)
    assert (want["tri_index"] == 150).sum() > 50
    e = engine_mod.Engine(0, change_range=0)
    for cell in (0.0, 4.0):
        m = e.trimesh(verts, cell=cell)
        st = m.stats
        # the pairs: every triangle's box in cells, floor((x - mn) / cell) per corner in double
        tri = rv.reshape(-1, 3, 3).astype(np.float64)
        mn, c = st["mn"].astype(np.float64), float(np.float32(st["cell"]))
        lo = np.clip(np.floor((tri.min(axis=1) - mn) / c), 0, np.array(st["cells"]) - 1)
        hi = np.clip(np.floor((tri.max(axis=1) - mn) / c), 0, np.array(st["cells"]) - 1)
        per = (hi - lo + 1).prod(axis=1)
        print("cell %g: cells %s, pairs %d (the large triangle: %d), longest list %d" % (st["cell"], st["cells"], st["pairs"], per[150], st["max_per_cell"]))
        assert st["pairs"] == int(per.sum()) and per[150] > 100
        assert_same_maps(got_maps(m, q), want, "cell %g" % cell)
        m.close()
    e.close()


@pytest.mark.gpu
def test_skipped_triangles_are_counted_and_never_returned(engine_mod):
    v = np.array([[0, 0, 0], [2, 0, 0], [0, 2, 0], [2, 2, 0], [np.nan, 0, 0], [5, 5, 5]], np.float32)
    tris = np.array([[0, 1, 4], [0, 0, 1], [0, 1, 7], [1, 2, 3], [0, 1, 2], [-1, 1, 2], [0, 5, 5]], np.int32)
    e = engine_mod.Engine(0, change_range=0)
    m = e.trimesh(v, tris)
    assert (m.stats["triangles"], m.stats["indexed"], m.stats["degenerate"]) == (7, 2, 5)
    assert same_bits(m.stats["mn"], np.float32([0, 0, 0])) and same_bits(m.stats["mx"], np.float32([2, 2, 0]))  # the NaN and vertex 5 are in no indexed triangle
    q = np.random.default_rng(2).uniform(-3, 6, (300, 3)).astype(np.float32)
    want = nearest_on_mesh(v, tris, q)
    got = got_maps(m, q)
    assert_same_maps(got, want)
    assert set(got["tri_index"]) <= {3, 4}
    m.close()
    with pytest.raises(engine_mod.PPPError) as ei:
        e.trimesh(v, tris[[0, 1, 2, 5, 6]])
    assert ei.value.code == engine_mod.ERR_ARG and ei.value.handle is None
    assert (ei.value.stats["triangles"], ei.value.stats["indexed"], ei.value.stats["degenerate"]) == (5, 0, 5)
    e.close()


@pytest.mark.gpu
def test_max_dist_is_inclusive_and_infinity_is_no_limit(engine_mod):
    v = np.array([[0, 0, 0], [4, 0, 0], [0, 4, 0]], np.float32)               # powers of two: the face branch is exact here
    hgt = np.float32(1.7)                                                     # (a float's square is exact in double)
    below = np.nextafter(hgt, np.float32(0))
    q = np.array([[1, 1, hgt], [1, 1, -hgt], [np.nan, 1, 1], [4000, 4000, 4000], [1, np.inf, 1]], np.float32)
    e = engine_mod.Engine(0, change_range=0)
    m = e.trimesh(v)
    for md, status in ((hgt, [MATCHED, MATCHED, DROPPED, TOO_FAR, DROPPED]), (below, [TOO_FAR, TOO_FAR, DROPPED, TOO_FAR, DROPPED]),
                       (INF, [MATCHED, MATCHED, DROPPED, MATCHED, DROPPED])):
        want = nearest_on_mesh(v, None, q, max_dist=md)
        got = got_maps(m, q, md)
        assert list(want["status"]) == status, (md, want["status"])
        assert_same_maps(got, want, "max_dist %r" % md)
    got = got_maps(m, q, hgt)
    assert got["distance"][0] == float(hgt) and got["region"][0] == FACE and got["deviation"][0] == float(hgt) == -got["deviation"][1]
    assert same_bits(got["closest"][0], np.array([1.0, 1.0, 0.0]))
    m.close()
    e.close()


@pytest.mark.gpu
def test_orientation_by_winding_and_by_viewpoint(engine_mod):
    tri = np.array([[0, 0, 0], [4, 0, 0], [0, 4, 0]], np.float32)
    both = np.concatenate([tri + np.float32([0, 0, 0]), (tri + np.float32([10, 0, 0]))[::-1]])     # the copy is wound the other way
    q = np.array([[1, 1, 2], [11, 1, 2], [1, 1, -2], [11, 1, -2]], np.float32)
    e = engine_mod.Engine(0, change_range=0)
    m = e.trimesh(both)
    got = got_maps(m, q)
    assert_same_maps(got, nearest_on_mesh(both, None, q))
    assert list(got["tri_index"]) == [0, 1, 0, 1] and list(got["deviation"]) == [2.0, -2.0, -2.0, 2.0]
    m.close()
    for vp, sign in (((3.0, 1.0, 50.0), 1.0), ((3.0, 1.0, -50.0), -1.0)):
        m = e.trimesh(both, orient=VIEWPOINT, viewpoint=vp)
        got = got_maps(m, q)
        assert_same_maps(got, nearest_on_mesh(both, None, q, orient=VIEWPOINT, vp=vp))
        assert list(got["deviation"]) == [2.0 * sign, 2.0 * sign, -2.0 * sign, -2.0 * sign]
        m.close()
    e.close()


# ---- ppp_get_mesh_deviation: the first stage is the search, the tail is ppp_get_deviation's (restated from its header comment:
# tests/test_deviation.py's restate_deviation has no tail of its own to import, its d2_table and its list of exact fields are used)

F24 = 2.0 ** 24


def restate_tail(P, first, dp):
    from test_deviation import d2_table
    n = len(P)
    status, dev = first["status"], first["deviation"]
    mi = np.nonzero(status == MATCHED)[0]
    sr2 = np.float32(dp["smooth_radius"]) * np.float32(dp["smooth_radius"])
    sm = dev.copy()
    if dp["smooth_radius"] > 0:
        fix = np.rint(dev[mi] * F24).astype(np.int64)
        Pm = P[mi]
        for s in range(0, len(mi), 512):
            inside = d2_table(Pm[s:s + 512], Pm) <= sr2
            sm[mi[s:s + 512]] = (inside * fix[None, :]).sum(axis=1, dtype=np.int64).astype(np.float64) / inside.sum(axis=1).astype(np.float64) * 2.0 ** -24
    v = sm[mi]
    over = v - dp["allowance"]
    target = np.zeros(n)
    target[mi] = np.where(over > 0, dp["gain"] * over, 0.0)
    lo, hi = float(v.min()), float(v.max())
    span = max(abs(lo), abs(hi))
    b = np.minimum(63, np.maximum(0, np.floor((v / span + 1.0) * 32.0))).astype(np.int64)
    stats = dict(n=n, matched=len(mi), too_far=int((status == TOO_FAR).sum()), no_normal=0, dropped=int((status == DROPPED).sum()),
                 proud=int((v > dp["allowance"]).sum()), below=int((v < 0).sum()), min_dev=lo, max_dev=hi,
                 mean_dev=float(np.rint(v * F24).astype(np.int64).sum(dtype=np.int64)) / float(len(mi)) * 2.0 ** -24,
                 rms_dev=math.sqrt(math.fsum(v * v) / len(mi)), max_dist2=float(first["D2"][mi].astype(np.float32).max()),
                 target_sum=math.fsum(target), hist=np.bincount(b, minlength=64).astype(np.int64))
    return sm, target, stats


@pytest.mark.gpu
@pytest.mark.parametrize("smooth", [0.0, 1.5])
def test_mesh_deviation_end_to_end(engine_mod, smooth):
    from test_deviation import EXACT_STATS
    rng = np.random.default_rng(21)
    x, y = np.meshgrid(np.linspace(-3, 43, 80), np.linspace(-2, 27, 50), indexing="ij")
    z = 0.4 * np.sin(x * 0.35) * np.cos(y * 0.3) + 0.15
    scan = np.stack([x, y, z], axis=2).reshape(-1, 3).astype(np.float32)
    scan[rng.integers(0, len(scan), 25)] = np.nan
    scan[rng.integers(0, len(scan), 10), 1] = np.inf
    scan[rng.integers(0, len(scan), 40), 2] += np.float32(30)                 # far away
    plate = np.array([[0, 0, 0], [40, 0, 0], [40, 25, 0], [0, 25, 0]], np.float32)
    tris = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    dp = dict(max_dist=2.0, smooth_radius=smooth, allowance=0.1, gain=3.0)
    e = engine_mod.Engine(0, change_range=0)
    e.set_cloud(scan)
    m = e.trimesh(plate, tris)
    P = e.cloud()
    first = nearest_on_mesh(plate, tris, P, max_dist=dp["max_dist"])
    sm_w, target_w, stats_w = restate_tail(P, first, dp)
    dev, sm, dist, idx, region, status, target, stats = e.mesh_deviation(m, **dp)
    for k, g in (("deviation", dev), ("distance", dist), ("tri_index", idx), ("region", region), ("status", status)):
        assert same_bits(g, first[k]), k
    assert same_bits(sm, sm_w) and same_bits(target, target_w)
    print("stats:", {k: v for k, v in stats.items() if k != "hist"})
    for k in EXACT_STATS:
        assert same_bits(np.asarray(stats[k]), np.asarray(stats_w[k]).astype(np.asarray(stats[k]).dtype)), (k, stats[k], stats_w[k])
    # the two ordered sums: the order differs from fsum's, by at most n roundings of the partial sums
    assert abs(stats["rms_dev"] - stats_w["rms_dev"]) <= 1e-12 * stats_w["rms_dev"]
    assert abs(stats["target_sum"] - stats_w["target_sum"]) <= 1e-12 * max(stats_w["target_sum"], 1.0)
    reg = first["region"][first["status"] == MATCHED]
    assert (stats["on_face"], stats["on_edge"], stats["on_vertex"]) == tuple(int((reg == k).sum()) for k in (FACE, EDGE, VERTEX))
    assert stats["on_face"] + stats["on_edge"] + stats["on_vertex"] == stats["matched"] > 3000
    assert stats["on_face"] > 0 and stats["on_edge"] > 0 and stats["too_far"] >= 40 and stats["dropped"] >= 30
    assert stats["max_distance"] == np.nanmax(first["distance"])
    none = e.mesh_deviation(m, maps=False, **dp)                              # cap = 0: the statistics alone
    assert all(a is None for a in none[:7])
    for k in stats:
        assert same_bits(np.asarray(none[7][k]), np.asarray(stats[k])), k
    m.close()
    e.close()


def dome(n=24, half=20.0, rise=6.0):
    v, t = sheet(n, n, 2 * half / n)
    v[:, :2] -= np.float32(half)
    v[:, 2] = (rise * (1 - (v[:, 0] ** 2 + v[:, 1] ** 2) / (2 * half * half))).astype(np.float32)
    return v, t


@pytest.mark.gpu
def test_exact_distance_is_a_lower_bound_of_the_sampled_one(engine_mod):
    """samples lie on the triangles, so the exact distance cannot exceed the distance to the nearest sample (the float d2 of
    ppp_get_deviation's partner, whose rounding 2^-20 covers); and somewhere it is strictly smaller"""
    v, t = dome()
    rng = np.random.default_rng(4)
    scan = np.stack([rng.uniform(-19, 19, 3000), rng.uniform(-19, 19, 3000), np.zeros(3000)], axis=1)
    scan[:, 2] = 6.0 * (1 - (scan[:, 0] ** 2 + scan[:, 1] ** 2) / 800.0) + rng.uniform(-0.3, 0.6, 3000)
    scan = scan.astype(np.float32)
    ref = engine_mod.Engine(0, change_range=0)
    ref.set_cloud_mesh(v, t, pitch=0.5)
    s = engine_mod.Engine(0, change_range=0)
    s.set_cloud(scan)
    m = s.trimesh(v, t)
    _, _, ref_index, status_s, _, _ = s.deviation(ref)
    _, _, dist, _, _, status_m, _, _ = s.mesh_deviation(m)
    assert (status_m == MATCHED).all() and (ref_index >= 0).all()
    samples = ref.cloud()
    P = s.cloud()
    S = samples[ref_index]
    dx, dy, dz = P[:, 0] - S[:, 0], P[:, 1] - S[:, 1], P[:, 2] - S[:, 2]
    d2 = ((dx * dx) + dy * dy) + dz * dz                                      # float, ppp_get_deviation's order
    assert d2.dtype == np.float32
    sampled = np.sqrt(d2.astype(np.float64))
    assert (dist <= sampled * (1 + 2.0 ** -20)).all()
    gain = sampled - dist
    print("exact below sampled: max %.4f mm, mean %.4f mm, strictly smaller at %d of %d points" % (gain.max(), gain.mean(), (dist < sampled).sum(), len(P)))
    assert (dist < sampled).any()
    for x in (m, s, ref):
        x.close()


@pytest.mark.gpu
def test_stl_path_and_refusals(engine_mod, tmp_path):
    E = engine_mod
    verts = soup_case(0)[:90]
    path = str(tmp_path / "soup.stl")
    E.save_stl(path, verts)
    e = E.Engine(0, change_range=0)
    a, b = e.trimesh(verts), e.trimesh_stl(path)
    assert {k: v for k, v in a.stats.items() if k not in ("mn", "mx")} == {k: v for k, v in b.stats.items() if k not in ("mn", "mx")}
    q = np.random.default_rng(3).uniform(-60, 60, (400, 3)).astype(np.float32)
    assert_same_maps(got_maps(b, q), got_maps(a, q))
    b.close()

    def refused(code, call):
        with pytest.raises(E.PPPError) as ei:
            call()
        assert ei.value.code == code, ei.value
        return ei.value

    assert refused(E.ERR_IO, lambda: e.trimesh_stl(str(tmp_path / "missing.stl"))).handle is None
    assert refused(E.ERR_ARG, lambda: e.trimesh(verts, cell=-1.0)).handle is None
    assert refused(E.ERR_ARG, lambda: e.trimesh(verts, cell=float("nan"))).handle is None
    assert refused(E.ERR_ARG, lambda: e.trimesh(verts, orient=7)).handle is None
    assert refused(E.ERR_ARG, lambda: e.trimesh(verts[:0])).handle is None                       # no triangle
    assert refused(E.ERR_ARG, lambda: e.trimesh(verts, np.zeros((0, 3), np.int32))).handle is None
    assert refused(E.ERR_CAPACITY, lambda: e.trimesh(verts, cell=1e-4)).handle is None           # 100 mm / 1e-4 per axis: far past 2^24 cells
    L = E.lib()                                                                                   # a soup whose vertices are not 3 per triangle
    import ctypes as C
    tp, out = E.TriMeshParams(0.0, 0), C.c_void_p(1)
    v = np.ascontiguousarray(verts[:8])
    assert L.ppp_trimesh_create(e.h, v.ctypes.data_as(C.POINTER(C.c_float)), 8, None, 2, C.byref(tp), None, C.byref(out), None) == E.ERR_ARG and not out.value
    out = C.c_void_p(1)
    assert L.ppp_trimesh_create(e.h, None, 9, None, 3, C.byref(tp), None, C.byref(out), None) == E.ERR_ARG and not out.value
    assert L.ppp_trimesh_nearest(None, None, 0, 1.0, None, None, None, None, None, None) == E.ERR_ARG
    assert L.ppp_trimesh_nearest(a.m, v.ctypes.data_as(C.POINTER(C.c_float)), 2, 0.0, None, None, None, None, None, None) == E.ERR_ARG
    L.ppp_trimesh_destroy(None)
    # ppp_get_mesh_deviation
    scan = np.random.default_rng(9).uniform(-40, 40, (2000, 3)).astype(np.float32)
    refused(E.ERR_ARG, lambda: e.mesh_deviation(a))                                               # no cloud
    e.set_cloud(scan)
    refused(E.ERR_ARG, lambda: e.mesh_deviation(None))
    refused(E.ERR_ARG, lambda: e.mesh_deviation(a, max_dist=0.0))
    refused(E.ERR_ARG, lambda: e.mesh_deviation(a, smooth_radius=1.0))                            # smoothing needs a finite max_dist
    refused(E.ERR_ARG, lambda: e.mesh_deviation(a, max_dist=2.0, gain=-1.0))
    assert e.mesh_deviation(a, max_dist=5.0, maps=False)[7]["n"] == 2000                          # the handle still works
    ranged = E.Engine(0, change_range=0, tool_radius=6.0, walk=1, slice_begin=2, slice_end=5)
    ranged.set_cloud(scan)
    refused(E.ERR_UNSUPPORTED, lambda: ranged.mesh_deviation(a, max_dist=5.0))
    ranged.close()
    a.close()
    a.close()                                                                                     # twice is allowed
    e.close()
