"""The welded topology of a resident triangle mesh, its angle-weighted pseudonormals and the signed distance they give
(ppp_trimesh_topology, ppp_trimesh_get_topology, ppp_trimesh_signed_nearest, ppp_get_mesh_signed_deviation).  The
yardstick is restate_topology() / restate_signed(): the rule of include/ppp_hip.h's comment in numpy float64 and plain Python
loops -- dictionaries where the device sorts, so a wrong run boundary, a wrong order of a sum or a wrong shift of the rotated frame
shows as unequal ids or bits.  The CPU tests check the restatement itself against solids whose inside is known analytically."""
import functools
import math
import os

import numpy as np
import pytest

from test_mesh_cloud import resident, same_bits
from test_trimesh import (DROPPED, EDGE, FACE, INF, MATCHED, TOO_FAR, VERTEX, VIEWPOINT, WINDING, file_units, frames, nearest_on_mesh,
                          restate_tail, sheet)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BORDER, MANIFOLD, INCONSISTENT, NONMANIFOLD = 0, 1, 2, 3
V_BORDER, V_IRREGULAR = 1, 2
S_BORDER, S_IRREGULAR, S_FALLBACK = 1, 2, 4
TOPO_MAPS = ("vertex_id", "edge_id", "edge_class", "vertex_bits")
COUNTS = ("vertices", "edges", "border_edges", "manifold_edges", "inconsistent_edges", "nonmanifold_edges", "border_vertices", "irregular_vertices", "closed")
# the walk's branch (a, b, ab, c, ac, bc, face: test_trimesh's order) as the rotated frame's feature 0 a, 1 b, 2 c, 3 ab, 4 ac, 5 bc, 6 face
BRANCH_FEATURE = np.array([0, 1, 3, 2, 4, 5, 6])


# ---------------------------------------------------------------- the restatement


def corners_of(rv, tris):
    """(corner positions float64[nt, 3, 3] in the caller's order, rot int[nt], and frames()'s N, A2, p0, valid)"""
    rv = np.ascontiguousarray(rv, np.float32).reshape(-1, 3)
    idx = np.arange(len(rv) // 3 * 3).reshape(-1, 3) if tris is None else np.asarray(tris, np.int64).reshape(-1, 3)
    p0, p1, p2, N, A2, valid = frames(rv, tris)
    inside = ((idx >= 0) & (idx < len(rv))).all(axis=1)
    v = rv[np.where(inside[:, None], idx, 0)].astype(np.float64)
    d = [v[:, (k + 1) % 3] - v[:, k] for k in range(3)]
    ab, bc, ca = ((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2] for e in d)
    with np.errstate(invalid="ignore"):
        rot = np.where((ab >= bc) & (ab >= ca), 0, np.where(bc >= ca, 1, 2))
    return v, rot, N, A2, p0, valid


def facet_normals(N, A2, p0, valid, orient, vp):
    """(n_f float64[nt, 3] as the search forms it, flipped bool[nt])"""
    with np.errstate(all="ignore"):
        n = N / A2[:, None]
        vpd = np.asarray(vp, np.float64)
        s = (N[:, 0] * (vpd[0] - p0[:, 0]) + N[:, 1] * (vpd[1] - p0[:, 1])) + N[:, 2] * (vpd[2] - p0[:, 2])
        flipped = (s < 0) & valid if orient == VIEWPOINT else np.zeros(len(N), bool)
    return np.where(flipped[:, None], -n, n), flipped


def restate_topology(rv, tris, orient=WINDING, vp=(0.0, 0.0, 0.0), weighted=True):
    """dict of ppp_trimesh_get_topology's six maps and the counts, from the header's comment.  weighted=False: alpha = 1"""
    v, rot, N, A2, p0, valid = corners_of(rv, tris)
    nt = len(v)
    nf, flipped = facet_normals(N, A2, p0, valid, orient, vp)
    out = dict(vertex_id=np.full((nt, 3), -1, np.int32), edge_id=np.full((nt, 3), -1, np.int32), edge_class=np.full((nt, 3), 255, np.uint8),
               vertex_bits=np.full((nt, 3), 255, np.uint8), vertex_normal=np.full((nt, 3, 3), np.nan), edge_normal=np.full((nt, 3, 3), np.nan))
    # weld: equal floats, -0 == +0; a dictionary keeps the first corner it sees, and the corners come in ascending 3 f + k
    vid, members = {}, {}
    for f in np.nonzero(valid)[0]:
        for k in range(3):
            key = tuple(float(c) + 0.0 for c in v[f, k])
            c = 3 * int(f) + k
            vid.setdefault(key, c)
            members.setdefault(vid[key], []).append(c)
            out["vertex_id"][f, k] = vid[key]
    # half-edges and edges
    edges = {}
    for f in np.nonzero(valid)[0]:
        for k in range(3):
            a, b = int(out["vertex_id"][f, k]), int(out["vertex_id"][f, (k + 1) % 3])
            if flipped[f]:
                a, b = b, a
            edges.setdefault((min(a, b), max(a, b)), []).append((3 * int(f) + k, a < b))
    vbits = {c: 0 for c in members}
    epn, ecls = {}, {}
    by_class = [0, 0, 0, 0]
    for (lo, hi), hs in edges.items():
        eid = hs[0][0]                                                       # ascending: the first is the smallest
        cls = BORDER if len(hs) == 1 else (NONMANIFOLD if len(hs) > 2 else (MANIFOLD if hs[0][1] != hs[1][1] else INCONSISTENT))
        by_class[cls] += 1
        s = np.zeros(3)
        for c, _ in hs:
            s = s + nf[c // 3]
        epn[eid], ecls[eid] = s, cls
        bit = V_BORDER if cls == BORDER else (0 if cls == MANIFOLD else V_IRREGULAR)
        vbits[lo] |= bit
        vbits[hi] |= bit
        for c, _ in hs:
            out["edge_id"][c // 3, c % 3] = eid
    vpn = {}
    for vtx, cs in members.items():
        s = np.zeros(3)
        for c in cs:
            f, k = c // 3, c % 3
            u, w = v[f, (k + 1) % 3] - v[f, k], v[f, (k + 2) % 3] - v[f, k]
            x = np.array([u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]])
            alpha = np.arctan2(np.sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]), (u[0] * w[0] + u[1] * w[1]) + u[2] * w[2]) if weighted else 1.0
            s = s + alpha * nf[f]
        vpn[vtx] = s
    for f in np.nonzero(valid)[0]:
        for k in range(3):
            e, x = int(out["edge_id"][f, k]), int(out["vertex_id"][f, k])
            out["edge_class"][f, k], out["vertex_bits"][f, k] = ecls[e], vbits[x]
            out["edge_normal"][f, k], out["vertex_normal"][f, k] = epn[e], vpn[x]
    out["stats"] = dict(vertices=len(members), edges=len(edges), border_edges=by_class[BORDER], manifold_edges=by_class[MANIFOLD],
                        inconsistent_edges=by_class[INCONSISTENT], nonmanifold_edges=by_class[NONMANIFOLD],
                        border_vertices=sum(1 for b in vbits.values() if b & V_BORDER), irregular_vertices=sum(1 for b in vbits.values() if b & V_IRREGULAR),
                        closed=int(by_class[BORDER] == 0 and by_class[INCONSISTENT] == 0 and by_class[NONMANIFOLD] == 0))
    out["rot"], out["nf"] = rot, nf
    return out


def restate_signed(rv, tris, P, topo=None, max_dist=INF, orient=WINDING, vp=(0.0, 0.0, 0.0)):
    """nearest_on_mesh's maps and the four signed maps beside them; s, |e| and |g| for the margin the GPU tests assert"""
    topo = topo or restate_topology(rv, tris, orient, vp)
    P = np.ascontiguousarray(P, np.float32).reshape(-1, 3)
    first = nearest_on_mesh(rv, tris, P, max_dist=max_dist, orient=orient, vp=vp)
    n = len(P)
    out = dict(first, signed_distance=np.full(n, np.nan), pseudonormal=np.full((n, 3), np.nan), feature=np.full(n, 255, np.uint8), flags=np.zeros(n, np.uint8),
               s=np.full(n, np.nan), e_len=np.full(n, np.nan), g_len=np.full(n, np.nan))
    for i in np.nonzero(first["status"] == MATCHED)[0]:
        f = int(first["tri_index"][i])
        feat, rot = int(BRANCH_FEATURE[first["branch"][i]]), int(topo["rot"][f])
        flags = 0
        if feat == 6:
            g, feature = topo["nf"][f], 6
        elif feat < 3:
            k = (feat + rot) % 3
            g, feature, flags = topo["vertex_normal"][f, k], k, int(topo["vertex_bits"][f, k])
        else:
            k = (rot + {3: 0, 5: 1, 4: 2}[feat]) % 3                         # ab, bc, ca: the caller's half-edges rot, rot + 1, rot + 2
            g, feature = topo["edge_normal"][f, k], 3 + k
            cls = int(topo["edge_class"][f, k])
            flags = S_BORDER if cls == BORDER else (0 if cls == MANIFOLD else S_IRREGULAR)
        e = P[i].astype(np.float64) - first["closest"][i]
        s = (e[0] * g[0] + e[1] * g[1]) + e[2] * g[2]
        if (s > 0 or s < 0) and (g != 0).any():
            sd = math.copysign(first["distance"][i], s)
        else:
            sd = math.copysign(first["distance"][i], first["deviation"][i])
            flags |= S_FALLBACK
        out["signed_distance"][i], out["pseudonormal"][i], out["feature"][i], out["flags"][i] = sd, g, feature, flags
        out["s"][i], out["e_len"][i], out["g_len"][i] = s, math.sqrt(float(e @ e)), math.sqrt(float(g @ g))
    return out


# ---------------------------------------------------------------- the meshes


def soup(verts, tris):
    return np.ascontiguousarray(np.asarray(verts, np.float32)[np.asarray(tris).ravel()])


def extrude(poly, apex, z0=0.0, z1=1.0):
    """(verts, tris) of the prism over the counter-clockwise polygon `poly`, caps fanned from poly[apex] (which must see the whole
    polygon), wound counter-clockwise seen from outside"""
    n = len(poly)
    verts = [(x, y, z0) for x, y in poly] + [(x, y, z1) for x, y in poly]
    ring = [(apex + 1 + i) % n for i in range(n - 1)]
    tris = []
    for a, b in zip(ring[:-1], ring[1:]):
        tris.append((n + apex, n + a, n + b))                                 # top: +z
        tris.append((apex, b, a))                                             # bottom: -z
    for a in range(n):
        b = (a + 1) % n
        tris += [(a, b, n + b), (a, n + b, n + a)]
    return np.array(verts, np.float32), np.array(tris, np.int32)


def cube(lo=(0.0, 0.0, 0.0), size=1.0):
    v, t = extrude([(0, 0), (1, 0), (1, 1), (0, 1)], 0)
    return (v * np.float32(size) + np.float32(lo)).astype(np.float32), t


def l_prism():
    return extrude([(0, 0), (2, 0), (2, 1), (1, 1), (1, 2), (0, 2)], 3)       # fanned from the concave corner (1, 1)


def tetrahedron():
    v = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], np.float32)
    t = []
    for tri in ((0, 1, 2), (0, 1, 3), (0, 2, 3), (1, 2, 3)):
        a, b, c = (v[i].astype(np.float64) for i in tri)
        t.append(tri if np.dot(np.cross(b - a, c - a), a + b + c) > 0 else tri[::-1])
    return v, np.array(t, np.int32)


def fan_cube(m=8):
    """the unit cube with its top fanned from (0, 0, 1) into 2 m triangles; the two sides that share the subdivided top edges are
    fanned from their far bottom corners, so the mesh stays closed"""
    s = [i / m for i in range(m + 1)]
    faces = [[(0, 0, 1)] + [(1, y, 1) for y in s] + [(x, 1, 1) for x in s[-2::-1]],                      # top, +z
             [(1, 0, 0), (1, 1, 0)] + [(1, y, 1) for y in s[::-1]],                                      # +x
             [(1, 1, 0), (0, 1, 0)] + [(x, 1, 1) for x in s],                                            # +y
             [(0, 0, 0), (0, 1, 0), (1, 1, 0), (1, 0, 0)],                                               # -z
             [(0, 0, 0), (0, 0, 1), (0, 1, 1), (0, 1, 0)],                                               # -x
             [(0, 0, 0), (1, 0, 0), (1, 0, 1), (0, 0, 1)]]                                               # -y
    out = []
    for ring in faces:
        for a, b in zip(ring[1:-1], ring[2:]):
            out.append([ring[0], a, b])
    return np.array(out, np.float32).reshape(-1, 3)


def reversed_cube():
    v, t = cube()
    t = t.copy()
    t[5] = t[5][::-1]
    return v, t


def two_cubes_on_an_edge():
    v, t = cube()
    w, _ = cube(lo=(1.0, 1.0, 0.0))
    return np.concatenate([v, w]), np.concatenate([t, t + 8])


def sheet_with_hole(nx=10, ny=8, pitch=2.0, wave=0.7):
    v, t = sheet(nx, ny, pitch, wave)
    i, j = np.divmod(np.arange(nx * ny), ny)
    hole = (i >= 4) & (i < 6) & (j >= 3) & (j < 5)
    keep = np.concatenate([~hole, ~hole])
    return v, t[keep]


def signed_zero_soup():
    """a cube centred on the origin's planes -- coordinates 0 and +-1 -- as a soup whose zeros are -0.0 in every second corner, with
    degenerate triangles (zero area, a NaN) between the real ones"""
    v, t = cube(lo=(-1.0, 0.0, 0.0))
    tri = soup(v, t).reshape(-1, 3, 3).copy()
    flat = tri.reshape(-1, 3)
    z = (flat == 0) & (np.arange(len(flat)) % 2 == 1)[:, None]
    flat[z] = np.float32(-0.0)
    bad = np.array([[[0, 0, 0], [1, 1, 1], [2, 2, 2]], [[np.nan, 0, 0], [1, 0, 0], [0, 1, 0]]], np.float32)
    rows = []
    for i, x in enumerate(tri):
        rows.append(x)
        if i % 3 == 0:
            rows.append(bad[(i // 3) % 2])
    return np.array(rows, np.float32).reshape(-1, 3)


def mixed_winding_cube():
    v, t = cube()
    t = t.copy()
    for f in (1, 4, 6, 11):
        t[f] = t[f][::-1]
    return v, t


def inside_cube(P):
    return ((P > 0) & (P < 1)).all(axis=1)


def inside_l(P):
    x, y, z = P[:, 0], P[:, 1], P[:, 2]
    return (z > 0) & (z < 1) & (x > 0) & (y > 0) & (((x < 2) & (y < 1)) | ((x < 1) & (y < 2)))


def inside_tetra(P):
    v, t = tetrahedron()
    ok = np.ones(len(P), bool)
    for tri in t:
        a, b, c = (v[i].astype(np.float64) for i in tri)
        ok &= (P.astype(np.float64) - a) @ np.cross(b - a, c - a) < 0
    return ok


def solid_queries(seed, lo, hi, n=400):
    return np.random.default_rng(seed).uniform(lo, hi, (n, 3)).astype(np.float32)


SOLIDS = {"cube": (lambda: (soup(*cube()), None), inside_cube, (-0.4, 1.4)), "tetrahedron": (tetrahedron, inside_tetra, (-1.4, 1.4)),
          "l_prism": (l_prism, inside_l, (-0.5, 2.5))}                      # the solids fill 17, 12 and 11 per cent of these boxes


# ---------------------------------------------------------------- CPU


def test_header_declares_and_engine_exports_the_topology_calls(engine_mod):
    txt = open(os.path.join(ROOT, "include", "ppp_hip.h")).read()
    for name in ("ppp_trimesh_topology", "ppp_trimesh_get_topology", "ppp_trimesh_signed_nearest", "ppp_get_mesh_signed_deviation"):
        assert name + "(" in txt and name in engine_mod.EXPORTS, name
    for name in ("PPP_MESH_SIGN_BORDER", "PPP_MESH_SIGN_IRREGULAR", "PPP_MESH_SIGN_FALLBACK", "PPP_EDGE_NONMANIFOLD", "ppp_trimesh_topology_stats"):
        assert name in txt, name
    assert hasattr(engine_mod.TriMesh, "topology") and hasattr(engine_mod.TriMesh, "signed_nearest") and hasattr(engine_mod.Engine, "mesh_signed_deviation")
    assert (engine_mod.MESH_SIGN_BORDER, engine_mod.MESH_SIGN_IRREGULAR, engine_mod.MESH_SIGN_FALLBACK) == (S_BORDER, S_IRREGULAR, S_FALLBACK)
    assert (engine_mod.EDGE_BORDER, engine_mod.EDGE_MANIFOLD, engine_mod.EDGE_INCONSISTENT, engine_mod.EDGE_NONMANIFOLD) == (0, 1, 2, 3)
    assert "inside / outside of closed meshes are out of scope" not in txt


@pytest.mark.parametrize("name", sorted(SOLIDS))
def test_restated_sign_is_the_analytic_inside_test(name):
    make, inside, (lo, hi) = SOLIDS[name]
    v, t = make()
    topo = restate_topology(v, t)
    assert topo["stats"]["closed"] == 1
    q = solid_queries(41, lo, hi)
    r = restate_signed(v, t, q, topo)
    want = inside(q)
    print("%s: %d inside, %d outside; features %s" % (name, want.sum(), (~want).sum(), np.bincount(r["feature"], minlength=7)))
    assert want.sum() >= 30 and (~want).sum() >= 100 and (r["status"] == MATCHED).all() and not (r["flags"] & S_FALLBACK).any()
    assert ((r["signed_distance"] < 0) == want).all()
    assert same_bits(np.abs(r["signed_distance"]), r["distance"])
    assert (r["region"] != FACE).sum() >= 50                                  # edges and vertices decided signs too


def test_restated_counts_on_known_meshes():
    st = restate_topology(soup(*cube()), None)["stats"]
    assert (st["vertices"], st["edges"], st["manifold_edges"], st["closed"]) == (8, 18, 18, 1)
    v, t = sheet(4, 3, 1.0)
    st = restate_topology(v, t)["stats"]
    assert (st["vertices"], st["edges"], st["border_edges"], st["border_vertices"], st["closed"]) == (20, 4 * 4 + 5 * 3 + 12, 14, 14, 0)
    st = restate_topology(*reversed_cube())["stats"]
    assert (st["inconsistent_edges"], st["manifold_edges"], st["irregular_vertices"], st["closed"]) == (3, 15, 3, 0)
    st = restate_topology(*two_cubes_on_an_edge())["stats"]
    assert (st["vertices"], st["edges"], st["nonmanifold_edges"], st["manifold_edges"], st["irregular_vertices"], st["closed"]) == (14, 35, 1, 34, 2, 0)
    assert restate_topology(fan_cube(), None)["stats"]["closed"] == 1 and restate_topology(*l_prism())["stats"]["closed"] == 1


def test_angle_weights_make_the_vertex_pseudonormal_independent_of_the_tessellation():
    plain = restate_topology(soup(*cube()), None)
    v = soup(*cube())
    k = np.nonzero((v == np.float32([0, 0, 1])).all(axis=1))[0][0]
    want = plain["vertex_normal"][k // 3, k % 3]
    assert np.abs(want - np.array([-1.0, -1.0, 1.0]) * (math.pi / 2)).max() <= 2.0 ** -40
    fan = fan_cube()
    k = np.nonzero((fan == np.float32([0, 0, 1])).all(axis=1))[0][0]
    members = (restate_topology(fan, None)["vertex_id"] == k).sum()
    got = restate_topology(fan, None)["vertex_normal"][k // 3, k % 3]
    flat = restate_topology(fan, None, weighted=False)["vertex_normal"][k // 3, k % 3]
    print("corners at the fan's apex: %d; weighted %s, unweighted %s" % (members, got, flat))
    assert members >= 18
    assert np.abs(got - want).max() <= 2.0 ** -40
    assert np.abs(flat / np.linalg.norm(flat) - want / np.linalg.norm(want)).max() > 0.3


def blade():
    """two facets that meet along the z axis at a 30 degree dihedral, the far one listed first; the query lies outside, in the
    edge's region, at 60 degrees to the blade's axis on the near facet's side"""
    c, s = math.cos(math.radians(15)), math.sin(math.radians(15))
    near = [(0, 0, 2), (0, 0, -2), (-4 * c, 4 * s, 0)]                        # normal (s, c, 0): up
    far = [(0, 0, -2), (0, 0, 2), (-4 * c, -4 * s, 0)]                        # normal (s, -c, 0): down
    v = np.array(far + near, np.float32)
    q = np.array([[math.cos(math.radians(60)), math.sin(math.radians(60)), 0.0]], np.float32)
    return v, q


def test_the_blade_old_convention_negative_signed_distance_positive():
    v, q = blade()
    topo = restate_topology(v, None)
    assert topo["stats"]["manifold_edges"] == 1 and topo["stats"]["border_edges"] == 4
    r = restate_signed(v, None, q, topo)
    print("blade: deviation %.6f, signed distance %.6f, distance %.6f" % (r["deviation"][0], r["signed_distance"][0], r["distance"][0]))
    assert r["region"][0] == EDGE and r["tri_index"][0] == 0
    assert r["deviation"][0] < -0.7 * r["distance"][0]                        # cos 135 degrees of the far facet's normal: the old convention
    assert r["signed_distance"][0] == r["distance"][0] > 0.99 and r["flags"][0] == 0


# ---------------------------------------------------------------- GPU

TOL = 2.0 ** -40


def cells_for(rv):
    ext = float((np.nanmax(rv, axis=0).astype(np.float64) - np.nanmin(rv, axis=0)).max())
    return (0.0, ext / 3.3)


def assert_topology(got_stats, got, want, what):
    assert {k: got_stats[k] for k in COUNTS} == want["stats"], (what, got_stats, want["stats"])
    for k in TOPO_MAPS:
        assert same_bits(got[k], want[k]), (what, k, np.nonzero(got[k] != want[k]))
    worst = 0.0
    for k in ("vertex_normal", "edge_normal"):
        assert (np.isnan(got[k]) == np.isnan(want[k])).all(), (what, k)
        d = np.abs(got[k] - want[k])
        d = d[~np.isnan(d)]
        worst = max(worst, float(d.max()))
    assert same_bits(got["edge_normal"], want["edge_normal"]), what           # no atan2 in it: plain sums in a fixed order
    return worst


TOPOLOGY_CASES = {
    "cube soup": lambda: (soup(*cube()), None, 0, WINDING, None),
    "cube soup, metres": lambda: (soup(*cube()), None, 1, WINDING, None),
    "fan cube": lambda: (fan_cube(), None, 0, WINDING, None),
    "l prism": lambda: l_prism() + (0, WINDING, None),
    "wavy sheet with a hole": lambda: sheet_with_hole() + (0, WINDING, None),
    "reversed facet": lambda: reversed_cube() + (0, WINDING, None),
    "two cubes on an edge": lambda: two_cubes_on_an_edge() + (0, WINDING, None),
    "signed zeros and degenerates": lambda: (signed_zero_soup(), None, 0, WINDING, None),
    "mixed winding by viewpoint": lambda: mixed_winding_cube() + (0, VIEWPOINT, (0.5, 0.5, 0.5)),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(TOPOLOGY_CASES))
def test_topology_matches_the_restatement(engine_mod, name):
    """ids, classes, bits and counts equal; pseudonormals within 2^-40 per component.  Facet normals have unit length and
    alpha < 4; with a 4 ulp atan2 on either side a term differs by about 2^-49 and a vertex of 20 corners (the fan's apex: 16 and
    the two plain sides) by less than 2^-44, plus the sums' own roundings: 2^-40 leaves a factor above ten."""
    verts, tris, change_range, orient, vp = TOPOLOGY_CASES[name]()
    fv = file_units(verts, change_range)
    rv = resident(engine_mod, fv, change_range)
    want = restate_topology(rv, tris, orient, (0, 0, 0) if vp is None else vp)
    e = engine_mod.Engine(0, change_range=change_range)
    worst, first = 0.0, None
    for cell in cells_for(rv):
        m = e.trimesh(fv, tris, cell=cell, orient=orient, viewpoint=vp)
        st, got = m.topology()
        worst = max(worst, assert_topology(st, got, want, "%s, cell %g" % (name, cell)))
        st2, again = m.topology()                                            # built once: the same arrays
        assert st2 == st and all(same_bits(again[k], got[k]) for k in got)
        assert m.topology(maps=False) == (st, None)
        if first is not None:
            assert all(same_bits(first[k], got[k]) for k in got), "the maps depend on the cell"
        first = got
        m.close()
    e.close()
    print("%s: %s; largest pseudonormal difference %.3e (2^%.1f)" % (name, want["stats"], worst, math.log2(worst) if worst else -math.inf))
    assert worst <= TOL
    if name == "signed zeros and degenerates":
        assert want["stats"]["vertices"] == 8 and want["stats"]["closed"] == 1 and (want["vertex_id"] == -1).any()
    if name == "mixed winding by viewpoint":
        assert want["stats"]["closed"] == 1 and want["stats"]["manifold_edges"] == 18
        assert restate_topology(rv, tris)["stats"]["inconsistent_edges"] > 0  # (by winding it is not)


def on_mesh_queries(rv, tris):
    """every vertex and every edge midpoint of an indexed mesh (exact where the coordinates are dyadic)"""
    idx = np.arange(len(rv) // 3 * 3).reshape(-1, 3) if tris is None else np.asarray(tris)
    c = rv[idx].astype(np.float64)
    mids = np.concatenate([(c[:, k] + c[:, (k + 1) % 3]) * 0.5 for k in range(3)])
    return np.concatenate([rv.astype(np.float64), mids]).astype(np.float32)


def signed_queries(rv, tris, seed, n=900):
    rng = np.random.default_rng(seed)
    mn, mx = rv.min(axis=0).astype(np.float64), rv.max(axis=0).astype(np.float64)
    ext = (mx - mn).max()
    q = [rng.uniform(mn - 0.6 * ext, mx + 0.6 * ext, (n, 3)), on_mesh_queries(rv, tris)]
    near = rv[rng.integers(0, len(rv), 300)].astype(np.float64) + rng.normal(0, 0.05 * ext, (300, 3))     # around vertices: vertex and edge regions
    q.append(near)
    q.append(np.array([[np.nan, 0, 0], [0, np.inf, 0]]))
    return np.concatenate(q).astype(np.float32)


SIGNED_MAPS = ("signed_distance", "pseudonormal", "feature", "flags", "distance", "closest", "deviation", "tri_index", "region", "status")


def got_signed(mesh, q, max_dist=INF):
    return dict(zip(SIGNED_MAPS, mesh.signed_nearest(q, max_dist)))


def assert_margin(want, what):
    """every matched query's sign is decided with room: |s| >= 2^-30 |e| |g|, or s is exactly 0 (the fallback)"""
    hit = want["status"] == MATCHED
    s, bound = want["s"][hit], 2.0 ** -30 * want["e_len"][hit] * want["g_len"][hit]
    bad = ~((np.abs(s) >= bound) | (s == 0))
    assert not bad.any(), "%s: %d queries decide their sign inside the margin: choose another seed" % (what, bad.sum())


SIGNED_CASES = {
    "cube soup": (lambda: (soup(*cube()), None, WINDING, None), 51),
    "l prism": (lambda: l_prism() + (WINDING, None), 52),
    "fan cube": (lambda: (fan_cube(), None, WINDING, None), 53),
    "wavy sheet with a hole": (lambda: sheet_with_hole() + (WINDING, None), 54),
    "reversed facet": (lambda: reversed_cube() + (WINDING, None), 55),
    "two cubes on an edge": (lambda: two_cubes_on_an_edge() + (WINDING, None), 56),
    "mixed winding by viewpoint": (lambda: mixed_winding_cube() + (VIEWPOINT, (0.5, 0.5, 0.5)), 57),
}


@functools.lru_cache(maxsize=None)
def signed_reference(name):
    make, seed = SIGNED_CASES[name]
    verts, tris, orient, vp = make()
    q = signed_queries(verts, tris, seed)                                     # (change_range 0 and floats: resident = given)
    want = restate_signed(verts, tris, q, orient=orient, vp=(0, 0, 0) if vp is None else vp)
    return verts, tris, orient, vp, q, want


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SIGNED_CASES))
def test_signed_query_matches_the_restatement(engine_mod, name):
    verts, tris, orient, vp, q, want = signed_reference(name)
    assert same_bits(resident(engine_mod, verts, 0), verts)
    assert_margin(want, name)
    hit = want["status"] == MATCHED
    fl = want["flags"][hit]
    print("%s: %d queries, features %s, border %d, irregular %d, fallback %d, negative %d" % (
        name, len(q), np.bincount(want["feature"][hit], minlength=7), (fl & S_BORDER > 0).sum(), (fl & S_IRREGULAR > 0).sum(), (fl & S_FALLBACK > 0).sum(),
        (want["signed_distance"] < 0).sum()))
    assert (np.bincount(want["feature"][hit], minlength=7) > 0).all() and (fl & S_FALLBACK).any() and (~hit).sum() == 2
    e = engine_mod.Engine(0, change_range=0)
    first = None
    for cell in cells_for(verts):
        m = e.trimesh(verts, tris, cell=cell, orient=orient, viewpoint=vp)
        got = got_signed(m, q)
        for k in ("feature", "flags", "signed_distance", "distance", "closest", "deviation", "tri_index", "region", "status"):
            assert same_bits(got[k], want[k]), (name, cell, k, np.nonzero(np.atleast_2d(got[k].T != want[k].T).any(axis=0))[0][:8])
        d = np.abs(got["pseudonormal"] - want["pseudonormal"])
        assert (np.isnan(got["pseudonormal"]) == np.isnan(want["pseudonormal"])).all() and np.nanmax(d) <= TOL
        plain = dict(zip(SIGNED_MAPS[4:], m.nearest(q)))                     # the plain outputs are TriMesh.nearest's bytes
        for k in SIGNED_MAPS[4:]:
            assert same_bits(got[k], plain[k]), (name, k)
        again = got_signed(m, q)                                             # a second call: the same bytes
        assert all(same_bits(again[k], got[k]) for k in SIGNED_MAPS)
        if first is not None:
            assert all(same_bits(first[k], got[k]) for k in SIGNED_MAPS), "the maps depend on the cell"
        first = got
        m.close()
    e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cube", "l_prism"])
def test_signs_are_the_analytic_inside_test(engine_mod, name):
    make, inside, (lo, hi) = SOLIDS[name]
    v, t = make()
    q = solid_queries(61, lo, hi, 2000)
    want = inside(q)
    e = engine_mod.Engine(0, change_range=0)
    for cell in cells_for(v):
        m = e.trimesh(v, t, cell=cell)
        assert m.topology(maps=False)[0]["closed"] == 1
        got = got_signed(m, q)
        assert (got["status"] == MATCHED).all() and not got["flags"].any()
        assert ((got["signed_distance"] < 0) == want).all() and same_bits(np.abs(got["signed_distance"]), got["distance"])
        m.close()
    e.close()
    assert want.sum() > 100 and (~want).sum() > 1000


@pytest.mark.gpu
def test_the_blade_on_the_device(engine_mod):
    v, q = blade()
    e = engine_mod.Engine(0, change_range=0)
    e.set_cloud(np.concatenate([q, q + np.float32([0, 0, 0.5])]))
    out = []
    for cell in (0.0, 1.7):
        m = e.trimesh(v, cell=cell)
        dev, _, dist, idx, region, status, _, _ = e.mesh_deviation(m)
        sd, _, dist2, idx2, region2, feature, flags, status2, _, stats = e.mesh_signed_deviation(m)
        assert (status == MATCHED).all() and (region == EDGE).all() and (idx == 0).all()
        assert (dev < -0.7 * dist).all()                                     # the old convention, still
        assert same_bits(sd, dist) and (sd > 0.99).all() and not flags.any() and (feature >= 3).all() and (feature <= 5).all()
        assert same_bits(dist2, dist) and same_bits(idx2, idx) and same_bits(region2, region) and same_bits(status2, status)
        assert (stats["positive"], stats["negative"], stats["fallback"], stats["on_border"], stats["on_edge"]) == (2, 0, 0, 0, 2)
        out.append((dev, sd, feature))
        m.close()
    e.close()
    assert all(same_bits(a, b) for a, b in zip(*out))


@pytest.mark.gpu
def test_border_flags_on_the_sheet_with_a_hole(engine_mod):
    v, t = sheet_with_hole()
    rng = np.random.default_rng(71)
    over = np.stack([rng.uniform(-3, 23, 1500), rng.uniform(-3, 19, 1500), rng.uniform(0.5, 2.5, 1500)], axis=1).astype(np.float32)
    interior = np.float32([[3.1, 2.9, 1.5], [15.2, 11.3, 2.0]])               # above triangles away from the rim and the hole
    scan = np.concatenate([over, interior])
    e = engine_mod.Engine(0, change_range=0)
    e.set_cloud(scan)
    P = e.cloud()
    want = restate_signed(v, t, P)
    assert_margin(want, "sheet with a hole")
    on_border = int((want["flags"] & S_BORDER > 0).sum())
    assert 100 < on_border < len(P) - 100
    outs = []
    for cell in cells_for(v):
        m = e.trimesh(v, t, cell=cell)
        out = e.mesh_signed_deviation(m)
        sd, flags, stats = out[0], out[6], out[9]
        assert same_bits(flags, want["flags"]) and same_bits(sd, want["signed_distance"]) and same_bits(out[5], want["feature"])
        assert stats["on_border"] == on_border and stats["irregular"] == 0
        assert (flags[-2:] == 0).all() and (out[4][-2:] == FACE).all()
        outs.append(out[:9])
        m.close()
    e.close()
    assert all(same_bits(a, b) for a, b in zip(*outs))


@pytest.mark.gpu
@pytest.mark.parametrize("smooth", [0.0, 1.5])
def test_mesh_signed_deviation_end_to_end(engine_mod, smooth):
    from test_deviation import EXACT_STATS
    rng = np.random.default_rng(23)
    x, y = np.meshgrid(np.linspace(-3, 25, 56), np.linspace(-2, 21, 40), indexing="ij")
    z = 0.4 * np.sin(x * 0.35) * np.cos(y * 0.3) + 0.15
    scan = np.stack([x, y, z], axis=2).reshape(-1, 3).astype(np.float32)
    scan[rng.integers(0, len(scan), 25)] = np.nan
    scan[rng.integers(0, len(scan), 10), 1] = np.inf
    scan[rng.integers(0, len(scan), 40), 2] += np.float32(30)                 # far away
    v, t = sheet_with_hole(wave=0.0)
    v = v.copy()
    v[:, 2] = (0.3 * np.sin(v[:, 0] * 0.5) + 0.1).astype(np.float32)          # folds along y: edges whose two facets disagree on the side
    dp = dict(max_dist=2.0, smooth_radius=smooth, allowance=0.1, gain=3.0)
    e = engine_mod.Engine(0, change_range=0)
    e.set_cloud(scan)
    P = e.cloud()
    want = restate_signed(v, t, P, max_dist=dp["max_dist"])
    assert_margin(want, "end to end")
    hit = want["status"] == MATCHED
    first = dict(want, deviation=want["signed_distance"])
    sm_w, target_w, stats_w = restate_tail(P, first, dp)
    outs = []
    for cell in cells_for(v):
        m = e.trimesh(v, t, cell=cell)
        sd, sm, dist, idx, region, feature, flags, status, target, stats = e.mesh_signed_deviation(m, **dp)
        for k, g in (("signed_distance", sd), ("distance", dist), ("tri_index", idx), ("region", region), ("feature", feature), ("flags", flags), ("status", status)):
            assert same_bits(g, want[k]), k
        assert same_bits(sm, sm_w) and same_bits(target, target_w)
        for k in EXACT_STATS:
            assert same_bits(np.asarray(stats[k]), np.asarray(stats_w[k]).astype(np.asarray(stats[k]).dtype)), (k, stats[k], stats_w[k])
        assert abs(stats["rms_dev"] - stats_w["rms_dev"]) <= 1e-12 * stats_w["rms_dev"]
        assert abs(stats["target_sum"] - stats_w["target_sum"]) <= 1e-12 * max(stats_w["target_sum"], 1.0)
        fl, s = want["flags"][hit], want["signed_distance"][hit]
        assert (stats["on_border"], stats["irregular"], stats["fallback"]) == tuple(int((fl & b > 0).sum()) for b in (S_BORDER, S_IRREGULAR, S_FALLBACK))
        assert (stats["negative"], stats["positive"]) == (int((s < 0).sum()), int((s > 0).sum()))
        assert stats["negative"] > 100 and stats["positive"] > 100 and stats["on_border"] > 0 and stats["matched"] == hit.sum() > 1500
        reg = want["region"][hit]
        assert (stats["on_face"], stats["on_edge"], stats["on_vertex"]) == tuple(int((reg == k).sum()) for k in (FACE, EDGE, VERTEX))
        none = e.mesh_signed_deviation(m, maps=False, **dp)                   # cap = 0: the statistics alone
        assert all(a is None for a in none[:9])
        for k in stats:
            assert same_bits(np.asarray(none[9][k]), np.asarray(stats[k])), k
        plain = e.mesh_deviation(m, **dp)                                     # the unsigned call is what it was
        assert same_bits(plain[0], want["deviation"]) and same_bits(plain[2], dist)
        outs.append((sd, sm, dist, idx, region, feature, flags, status, target))
        m.close()
    e.close()
    assert all(same_bits(a, b) for a, b in zip(*outs))
    print("stats:", {k: v for k, v in stats.items() if k != "hist"})


@pytest.mark.gpu
def test_refusals(engine_mod):
    import ctypes as C
    E = engine_mod
    L = E.lib()
    v, t = cube()
    e = E.Engine(0, change_range=0)
    m = e.trimesh(v, t)
    q = np.ascontiguousarray(np.float32([[0.5, 0.5, 2.0], [0.5, 0.5, 0.5]]))
    qp = q.ctypes.data_as(C.POINTER(C.c_float))
    none10 = [None] * 10

    def refused(code, call):
        with pytest.raises(E.PPPError) as ei:
            call()
        assert ei.value.code == code, ei.value

    assert L.ppp_trimesh_topology(None, None) == E.ERR_ARG
    assert L.ppp_trimesh_get_topology(None, None, None, None, None, None, None, 0, None) == E.ERR_ARG
    assert L.ppp_trimesh_signed_nearest(None, qp, 2, 1.0, *none10) == E.ERR_ARG
    assert L.ppp_trimesh_signed_nearest(m.m, None, 2, 1.0, *none10) == E.ERR_ARG
    assert L.ppp_trimesh_signed_nearest(m.m, qp, 2, 0.0, *none10) == E.ERR_ARG
    assert L.ppp_trimesh_signed_nearest(m.m, qp, 2, float("nan"), *none10) == E.ERR_ARG
    assert L.ppp_trimesh_signed_nearest(m.m, qp, 2, 1.0, *none10) == 0        # every output may be NULL
    assert L.ppp_trimesh_topology(m.m, None) == 0 and L.ppp_trimesh_get_topology(m.m, None, None, None, None, None, None, 5, None) == 0
    sd = m.signed_nearest(q)[0]
    assert list(sd) == [1.0, -0.5]
    sd, _, feature, flags = m.signed_nearest(q, max_dist=0.75)[:4]           # beyond max_dist: NaN, 255, 0
    assert np.isnan(sd[0]) and feature[0] == 255 and flags[0] == 0 and sd[1] == -0.5
    vid = np.zeros((4, 3), np.int32)                                         # cap: the first triangles only
    assert L.ppp_trimesh_get_topology(m.m, vid.ctypes.data_as(C.POINTER(C.c_int)), None, None, None, None, None, 3, None) == 0
    assert same_bits(vid[:3], m.topology()[1]["vertex_id"][:3]) and (vid[3] == 0).all()
    refused(E.ERR_ARG, lambda: e.mesh_signed_deviation(m))                    # no cloud
    scan = np.random.default_rng(9).uniform(-1, 2, (2000, 3)).astype(np.float32)
    e.set_cloud(scan)
    refused(E.ERR_ARG, lambda: e.mesh_signed_deviation(None))
    refused(E.ERR_ARG, lambda: e.mesh_signed_deviation(m, max_dist=0.0))
    refused(E.ERR_ARG, lambda: e.mesh_signed_deviation(m, max_dist=-1.0))
    refused(E.ERR_ARG, lambda: e.mesh_signed_deviation(m, smooth_radius=1.0))  # smoothing needs a finite max_dist
    refused(E.ERR_ARG, lambda: e.mesh_signed_deviation(m, max_dist=2.0, gain=-1.0))
    assert L.ppp_get_mesh_signed_deviation(e.h, m.m, None, *([None] * 9), 0, None) == E.ERR_ARG
    assert L.ppp_get_mesh_signed_deviation(None, m.m, None, *([None] * 9), 0, None) == E.ERR_ARG
    assert e.mesh_signed_deviation(m, max_dist=5.0, maps=False)[9]["n"] == 2000   # the handle still works
    ranged = E.Engine(0, change_range=0, tool_radius=6.0, walk=1, slice_begin=2, slice_end=5)
    ranged.set_cloud(scan)
    refused(E.ERR_UNSUPPORTED, lambda: ranged.mesh_signed_deviation(m, max_dist=5.0))
    ranged.close()
    m.close()
    e.close()


@pytest.mark.gpu
def test_a_mesh_on_another_device_is_refused(engine_mod):
    from test_deviation_tiles import device_count
    if device_count() < 2:
        pytest.skip("needs two GPUs in one process: this machine shows %d" % device_count())
    E = engine_mod
    s = E.Engine(0, change_range=0)
    s.set_cloud(np.random.default_rng(9).uniform(-1, 2, (500, 3)).astype(np.float32))
    other = E.Engine(1, change_range=0)
    far = other.trimesh(*cube())
    with pytest.raises(E.PPPError) as ex:
        s.mesh_signed_deviation(far)
    assert ex.value.code == E.ERR_ARG
    far.close(); other.close(); s.close()
