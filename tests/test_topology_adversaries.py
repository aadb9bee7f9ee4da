"""The welded topology and the signed distance off their small meshes: slot counts on all three paths of the
library sort (one block up to 1 024 items, merge sort up to 2^20, onesweep above), slot counts S where S - 1 crosses a power of
two (the bits the half-edge passes sort on), runs of thousands of corners and hundreds of half-edges under one head thread, a
two-sided lamina whose pseudonormals vanish, subnormal coordinates, degenerates and both orient rules at size, and the same
soup through an STL file.  The yardstick is restate_topology_fast(), test_trimesh_topology's dictionary restatement in
vectorised numpy, proved equal to it on the CPU (ids, classes, bits, counts, and both pseudonormals bit for bit); the signed
queries go against restate_signed()'s brute force.  What a case must have to mean anything (a top bit, a run length, a count in
closed form, a zero pseudonormal, a subnormal) is asserted on the restatement alone, before the engine is looked at."""
import functools
import math

import numpy as np
import pytest

from test_mesh_cloud import resident, same_bits
from test_trimesh import MATCHED, VIEWPOINT, WINDING, file_units, frames, sheet
from test_trimesh_topology import (BORDER, COUNTS, INCONSISTENT, MANIFOLD, NONMANIFOLD, S_FALLBACK, SIGNED_MAPS, TOL, TOPOLOGY_CASES, V_BORDER, V_IRREGULAR,
                                   assert_margin, assert_topology, cells_for, corners_of, facet_normals, fan_cube, got_signed, restate_signed, restate_topology,
                                   solid_queries, soup)

F32 = np.float32
ONE_BLOCK = 1024                                                             # the library's one-block sort: up to 256 x 4 items
MERGE = 2 ** 20                                                              # its merge sort: up to here; onesweep above
LONG = 20                                                                    # the longest run of test_trimesh_topology: up to here 2^-40 stands


def sort_path(slots):
    return "one block" if slots <= ONE_BLOCK else ("merge" if slots <= MERGE else "onesweep")


def id_bits(slots):
    """the bits of a vertex id that the half-edge passes sort on, as trimesh_topology_build counts them"""
    bits = 1
    while bits < 32 and (slots - 1) >> bits:
        bits += 1
    return bits


# ---------------------------------------------------------------- the restatement, vectorised


def restate_topology_fast(rv, tris, orient=WINDING, vp=(0.0, 0.0, 0.0)):
    """restate_topology() without its Python loops: np.unique (first occurrence, inverse) where it keeps dictionaries, and
    np.add.at, which applies its additions one by one in the order of its input, where it sums -- the corners ascend, so the bits
    are those of s = s + term.  Beside the maps: longest_run / longest_edge_run, the most corners of one vertex and half-edges of
    one edge, and peak, the largest |component| of a partial sum over the vertices of more than LONG corners"""
    v, rot, N, A2, p0, valid = corners_of(rv, tris)
    nt = len(v)
    nf, flipped = facet_normals(N, A2, p0, valid, orient, vp)
    out = dict(vertex_id=np.full((nt, 3), -1, np.int32), edge_id=np.full((nt, 3), -1, np.int32), edge_class=np.full((nt, 3), 255, np.uint8),
               vertex_bits=np.full((nt, 3), 255, np.uint8), vertex_normal=np.full((nt, 3, 3), np.nan), edge_normal=np.full((nt, 3, 3), np.nan))
    c = (3 * np.nonzero(valid)[0][:, None] + np.arange(3)).ravel()           # the corners of the indexed triangles, ascending
    f, k = c // 3, c % 3
    pos = v[f, k]
    # weld: equal floats, -0 == +0: the bit patterns of float32(x) + 0, an axis at a time (a rank per axis, then a rank per pair)
    bits = np.ascontiguousarray(pos.astype(F32) + F32(0)).view(np.uint32)
    key = np.zeros(len(c), np.int64)
    for d in range(3):
        _, inv = np.unique(bits[:, d], return_inverse=True)
        _, key = np.unique(key * (int(inv.max()) + 1) + inv.astype(np.int64), return_inverse=True)
        key = key.astype(np.int64)
    _, first, vinv, members = np.unique(key, return_index=True, return_inverse=True, return_counts=True)
    vid = c[first][vinv]                                                     # the first corner of its position
    by_corner = np.full(3 * nt, -1, np.int64)
    by_corner[c] = vid
    # half-edges and edges
    a, b = vid, by_corner[3 * f + (k + 1) % 3]
    a, b = np.where(flipped[f], b, a), np.where(flipped[f], a, b)
    lo, hi, up = np.minimum(a, b), np.maximum(a, b), a < b
    _, efirst, einv, ecount = np.unique(lo * (3 * nt) + hi, return_index=True, return_inverse=True, return_counts=True)
    ups = np.bincount(einv, weights=up, minlength=len(efirst)).astype(np.int64)
    cls = np.where(ecount == 1, BORDER, np.where(ecount > 2, NONMANIFOLD, np.where(ups == 1, MANIFOLD, INCONSISTENT)))
    epn = np.zeros((len(efirst), 3))
    np.add.at(epn, einv, nf[f])
    bit = np.where(cls == BORDER, V_BORDER, np.where(cls == MANIFOLD, 0, V_IRREGULAR)).astype(np.uint8)
    vbits = np.zeros(3 * nt, np.uint8)                                        # at a vertex's own corner
    np.bitwise_or.at(vbits, lo[efirst], bit)
    np.bitwise_or.at(vbits, hi[efirst], bit)
    # the angle at every corner: restate_topology's expressions
    u, w = v[f, (k + 1) % 3] - pos, v[f, (k + 2) % 3] - pos
    x = [u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2], u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]]
    alpha = np.arctan2(np.sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]), (u[:, 0] * w[:, 0] + u[:, 1] * w[:, 1]) + u[:, 2] * w[:, 2])
    terms = alpha[:, None] * nf[f]
    vpn = np.zeros((len(first), 3))
    np.add.at(vpn, vinv, terms)
    out["vertex_id"][f, k], out["edge_id"][f, k] = vid, c[efirst][einv]
    out["edge_class"][f, k], out["vertex_bits"][f, k] = cls[einv], vbits[vid]
    out["edge_normal"][f, k], out["vertex_normal"][f, k] = epn[einv], vpn[vinv]
    by_class = np.bincount(cls, minlength=4)
    own = vbits[c[first]]
    out["stats"] = dict(vertices=len(first), edges=len(efirst), border_edges=int(by_class[BORDER]), manifold_edges=int(by_class[MANIFOLD]),
                        inconsistent_edges=int(by_class[INCONSISTENT]), nonmanifold_edges=int(by_class[NONMANIFOLD]),
                        border_vertices=int((own & V_BORDER > 0).sum()), irregular_vertices=int((own & V_IRREGULAR > 0).sum()),
                        closed=int(by_class[BORDER] == 0 and by_class[INCONSISTENT] == 0 and by_class[NONMANIFOLD] == 0))
    out["rot"], out["nf"] = rot, nf
    peak = 0.0
    for j in np.nonzero(members > LONG)[0]:
        s = np.zeros(3)
        for t in terms[vinv == j]:
            s = s + t
            peak = max(peak, float(np.abs(s).max()))
    out["longest_run"], out["longest_edge_run"], out["peak"], out["slots"] = int(members.max()), int(ecount.max()), peak, len(c)
    return out


def vertex_tolerance(topo):
    """The bound on a component of a vertex pseudonormal against the restatement.  test_topology_matches_the_restatement argues
    for runs of up to 20 corners: a term alpha n_f (|n_f| = 1, alpha < 4) computed with an atan2 of 4 ulp on either side differs
    by about 2^-49, 20 of them by less than 2^-44, and 2^-40 leaves a factor above ten.  For a run of m corners the terms are
    smaller (the angles of one vertex add up to a few pi), but each of the m ordered additions may now round differently on the
    two sides, because its operands already differ: by an ulp of the partial sum, 2^-52 |s|, which with the terms' own 2^-51 (4 ulp
    of an alpha below 2, times a unit normal's component) stays below 2^-50 max(1, |s|) an addition.  m of them, the largest
    |component| of a partial sum in the restatement for |s|, and the same factor of ten:
        tol = 10 m 2^-50 max(1, peak)              for m > 20, and 2^-40 up to there."""
    m = topo["longest_run"]
    return TOL if m <= LONG else 10 * m * 2.0 ** -50 * max(1.0, topo["peak"])


def restate_signed_in_pieces(rv, tris, q, topo, orient, vp, piece):
    """restate_signed() `piece` queries at a time: its brute force holds queries x triangles x 3 doubles several times over"""
    parts = [restate_signed(rv, tris, q[s:s + piece], topo, orient=orient, vp=vp) for s in range(0, len(q), piece)]
    return {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}


def probe_queries(rv, tris, seed, picks=40, away=60):
    """queries at the scale of the triangles themselves, since these meshes are long, thin or huge: the corners and the edge
    midpoints of `picks` indexed triangles (the first two and the last two of the list among them: the lowest and the highest
    ids), each of them again moved by a third of its triangle's longest edge in a random direction (the regions of vertices,
    edges and faces), `away` points in the widened box, a NaN and an infinity"""
    rng = np.random.default_rng(seed)
    p0, p1, p2, _, _, valid = frames(rv, tris)
    fi = np.nonzero(valid)[0]
    f = fi[rng.integers(0, len(fi), picks)]
    ends = fi[[0, 1, -2, -1]][:picks]
    f[:len(ends)] = ends
    tri = np.stack([p0[f], p1[f], p2[f]], axis=1)
    side = np.sqrt(((tri - np.roll(tri, -1, axis=1)) ** 2).sum(axis=2).max(axis=1))
    on = np.concatenate([tri.reshape(-1, 3), ((tri + np.roll(tri, -1, axis=1)) * 0.5).reshape(-1, 3)])
    near = on + rng.normal(0, 1, on.shape) * np.tile(np.repeat(side, 3), 2)[:, None] / 3
    every = np.concatenate([p0[fi], p1[fi], p2[fi]])
    mn, mx = every.min(axis=0), every.max(axis=0)
    ext = (mx - mn).max()
    box = rng.uniform(mn - 0.2 * ext, mx + 0.2 * ext, (away, 3))
    return np.concatenate([on, near, box, np.array([[np.nan, 0, 0], [0, np.inf, 0]])]).astype(F32)


# ---------------------------------------------------------------- the meshes


def strip(R):
    """a planar (z = x / 4) triangle strip of exactly R triangles as a soup: dyadic coordinates, no three corners in line, one
    winding, and every triangle's new vertex as its corner 2 -- so the vertex ids are 0, 1 and 3 t + 2, the largest one S - 1"""
    i = np.arange(R + 2)
    p = np.stack([i * 0.5, (i % 2) * 1.0, i * 0.125], axis=1).astype(F32)
    t = np.arange(R)
    odd = t % 2 == 1
    tris = np.stack([np.where(odd, t + 1, t), np.where(odd, t, t + 1), t + 2], axis=1)
    return soup(p, tris)


STRIPS = (341, 342, 5461, 5462)                                               # S = 1 023, 1 026: 2^10 and the one-block limit; 16 383, 16 386: 2^14


@functools.lru_cache(maxsize=None)
def mixed_sheet():
    """test_trimesh's wavy sheet(48, 40): 3 840 triangles, moved so that x, y and z take both signs (and x and y the value 0)"""
    v, t = sheet(48, 40, 1.0, wave=1.5)
    return (v - F32([24, 20, 0])).astype(F32), t


BAD_SOUP = np.array([[[0, 0, 0], [1, 1, 1], [2, 2, 2]], [[np.nan, 0, 0], [1, 0, 0], [0, 1, 0]]], F32)   # zero area; a NaN corner


def mixed_soup(reverse_third=False):
    """the sheet as a soup whose zeros are -0.0 in every second corner, a degenerate triangle after every third facet as in
    signed_zero_soup (zero area, a NaN corner, in turn); reverse_third: every third facet wound the other way"""
    v, t = mixed_sheet()
    t = t.copy()
    if reverse_third:
        t[1::3] = t[1::3, ::-1]
    tri = v[t].copy()
    flat = tri.reshape(-1, 3)
    flat[(flat == 0) & (np.arange(len(flat)) % 2 == 1)[:, None]] = F32(-0.0)
    rows = []
    for i, x in enumerate(tri):
        rows.append(x)
        if i % 3 == 0:
            rows.append(BAD_SOUP[(i // 3) % 2])
    return np.array(rows, F32).reshape(-1, 3)


def mixed_indexed():
    """the sheet as an indexed list with a degenerate triangle after every third facet, three ways in turn: a repeated index, an
    index of an extra NaN vertex, an index past the vertices"""
    v, t = mixed_sheet()
    nan_vertex = len(v)
    v = np.concatenate([v, np.array([[np.nan, 0, 0]], F32)])
    rows = []
    for i, x in enumerate(t):
        rows.append(x)
        if i % 3 == 0:
            way = (i // 3) % 3
            rows.append([x[0], x[0], x[1]] if way == 0 else ([nan_vertex, x[1], x[2]] if way == 1 else [x[0], x[1], len(v) + 5]))
    return v, np.array(rows, np.int32)


ABOVE = (0.0, 0.0, 1000.0)                                                   # resident units: every facet of the sheet faces it
MIXED = {
    "soup by winding": lambda: (mixed_soup(), None, WINDING, None),
    "indexed by winding": lambda: mixed_indexed() + (WINDING, None),
    "every third facet reversed, by viewpoint": lambda: (mixed_soup(reverse_third=True), None, VIEWPOINT, ABOVE),
}
BIG = (420, 420)


@functools.lru_cache(maxsize=None)
def big_sheet():
    """a flat-ish sheet(420, 420) as a soup: 352 800 triangles, 1 058 400 slots"""
    return soup(*sheet(BIG[0], BIG[1], 0.5, wave=0.25))


@functools.lru_cache(maxsize=None)
def big_sheet_restated():
    return restate_topology_fast(big_sheet(), None)


def cone(n=3000):
    """n triangles round the apex (0, 0, 1), the fan closed: triangle i is (apex, rim i, rim i + 1), the last one back to rim 0.
    The apex is vertex 0, rim 0 vertex 1 and rim i + 1 vertex 3 i + 2"""
    th = 2 * math.pi * np.arange(n) / n
    rim = np.stack([np.cos(th), np.sin(th), np.zeros(n)], axis=1).astype(F32)
    tri = np.empty((n, 3, 3), F32)
    tri[:, 0], tri[:, 1], tri[:, 2] = F32([0, 0, 1]), rim, np.roll(rim, -1, axis=0)
    return tri.reshape(-1, 3)


def book(n=300):
    """n triangular pages (spine bottom, spine top, a point of a half circle round the spine): one edge with n half-edges"""
    th = math.pi * np.arange(n) / n
    tri = np.empty((n, 3, 3), F32)
    tri[:, 0], tri[:, 1] = F32([0, 0, 0]), F32([0, 0, 1])
    tri[:, 2] = np.stack([np.cos(th), np.sin(th), np.full(n, 0.5)], axis=1).astype(F32)
    return tri.reshape(-1, 3)


ALIAS_FAN = 400                                                              # cone(400): S - 1 = 1 199, 11 bits, vertex 1 + 2^10 = rim 342


def lamina():
    """the 10 x 8 wavy sheet with every facet listed again right behind itself, wound the other way"""
    v, t = sheet(10, 8, 2.0, 0.7)
    return v, np.stack([t, t[:, ::-1]], axis=1).reshape(-1, 3)


def beyond_the_rim(v, nx, ny, seed, times=3):
    """points outside the sheet's outline and off its surface: every rim vertex moved straight out of the outline in x or y (or
    both, at the four corners) and up or down -- the regions of the rim's vertices and edges"""
    rng = np.random.default_rng(seed)
    i, j = np.divmod(np.arange(len(v)), ny + 1)
    out = np.stack([(i == nx) * 1.0 - (i == 0), (j == ny) * 1.0 - (j == 0), np.zeros(len(v))], axis=1)
    rim = (out != 0).any(axis=1)
    q = []
    for _ in range(times):
        step = out[rim] * rng.uniform(0.3, 1.5, (rim.sum(), 1))
        step[:, 2] = rng.uniform(0.2, 1.0, rim.sum()) * rng.choice([-1.0, 1.0], rim.sum())
        q.append(v[rim].astype(np.float64) + step)
    return np.concatenate(q)


TINY, TINIER = 2.0 ** -140, 2.0 ** -141
SUBNORMALS = {"2^-140 beside 0": (0.0, TINY), "-2^-140 beside 0": (0.0, -TINY), "2^-141 beside 2^-140": (TINIER, TINY)}


def subnormal_pair(a, b):
    return np.array([[a, 0, 0], [1, 0, 0], [0, 1, 0], [b, 0, 0], [0, 1, 0], [1, 0, 0]], F32)


LONG_RUNS = {"cone": cone, "book": book, "closing spoke": lambda: cone(ALIAS_FAN)}


# ---------------------------------------------------------------- CPU: the fast restatement is the dictionary one


def assert_same_restatement(fast, slow, what):
    assert fast["stats"] == slow["stats"], (what, fast["stats"], slow["stats"])
    for k in ("vertex_id", "edge_id", "edge_class", "vertex_bits", "edge_normal", "vertex_normal", "rot", "nf"):
        assert same_bits(fast[k], np.asarray(slow[k])), (what, k)


@pytest.mark.parametrize("orient", [WINDING, VIEWPOINT])
@pytest.mark.parametrize("name", sorted(TOPOLOGY_CASES))
def test_fast_restatement_is_the_dictionary_one(name, orient):
    verts, tris, _, _, vp = TOPOLOGY_CASES[name]()
    vp = (0.3, 0.4, 5.0) if vp is None else vp                                 # above the solids: it turns their lower facets
    fast, slow = restate_topology_fast(verts, tris, orient, vp), restate_topology(verts, tris, orient, vp)
    assert_same_restatement(fast, slow, name)
    if orient == VIEWPOINT and "sheet" not in name:
        flipped = (fast["nf"] != restate_topology_fast(verts, tris)["nf"]).any(axis=1)
        assert flipped.any() and not flipped.all()


@pytest.mark.parametrize("name", sorted(MIXED))
def test_fast_restatement_is_the_dictionary_one_on_the_merge_path_sheet(name):
    verts, tris, orient, vp = MIXED[name]()
    vp = (0, 0, 0) if vp is None else vp
    fast = restate_topology_fast(verts, tris, orient, vp)
    assert_same_restatement(fast, restate_topology(verts, tris, orient, vp), name)
    assert sort_path(fast["slots"]) == "merge" and fast["slots"] == 11520


def test_fast_restatement_is_the_dictionary_one_on_long_runs_and_zeros():
    for what, (verts, tris) in (("cone 300", (cone(300), None)), ("book", (book(), None)), ("lamina", lamina()),
                                ("subnormals", (subnormal_pair(TINIER, TINY), None))):
        fast = restate_topology_fast(verts, tris)
        assert_same_restatement(fast, restate_topology(verts, tris), what)


# ---------------------------------------------------------------- CPU: every case is what it claims


@pytest.mark.parametrize("R", STRIPS)
def test_strip_counts_and_top_bit(R):
    rv = strip(R)
    S = 3 * R
    assert len(rv) == S and (rv * 8 == np.round(rv * 8)).all() and (rv[:, 2] * 4 == rv[:, 0]).all()
    t = restate_topology_fast(rv, None)
    assert t["slots"] == S and (t["vertex_id"][1:, 2] == 3 * np.arange(1, R) + 2).all()     # the new vertex is corner 2
    st = t["stats"]
    assert (st["vertices"], st["edges"], st["border_edges"], st["manifold_edges"]) == (R + 2, 2 * R + 1, R + 2, R - 1)
    assert (st["inconsistent_edges"], st["nonmanifold_edges"], st["border_vertices"], st["irregular_vertices"], st["closed"]) == (0, 0, R + 2, 0, 0)
    bits = id_bits(S)
    print("R %d: %d slots (%s), %d id bits, largest vertex id %d" % (R, S, sort_path(S), bits, t["vertex_id"].max()))
    assert bits == {341: 10, 342: 11, 5461: 14, 5462: 15}[R] and sort_path(S) == ("one block" if R == 341 else "merge")
    assert t["vertex_id"].max() == S - 1 < 2 ** bits
    if R in (342, 5462):
        assert t["vertex_id"].max() >= 2 ** (bits - 1)                       # the top bit is in use


def test_mixed_sheet_is_what_it_claims():
    v, _ = mixed_sheet()
    assert (v.min(axis=0) < 0).all() and (v.max(axis=0) > 0).all() and (v[:, 0] == 0).any() and (v[:, 1] == 0).any()
    plain = restate_topology_fast(*mixed_sheet())["stats"]
    for name in sorted(MIXED):
        verts, tris, orient, vp = MIXED[name]()
        t = restate_topology_fast(verts, tris, orient, (0, 0, 0) if vp is None else vp)
        nt = len(verts) // 3 if tris is None else len(tris)
        assert nt == 3840 + 1280 and (t["vertex_id"][:, 0] == -1).sum() == 1280 and t["slots"] == 11520
        assert t["stats"] == plain, name                                     # the degenerates, the -0.0 and the viewpoint change nothing
        assert (t["stats"]["vertices"], t["stats"]["edges"], t["stats"]["border_edges"], t["stats"]["closed"]) == (49 * 41, 48 * 41 + 49 * 40 + 48 * 40, 176, 0)
        if tris is None:
            signbit = np.signbit(verts) & (verts == 0)
            assert signbit.any() and ((verts == 0) & ~signbit).any()         # both zeros
    verts, tris, orient, vp = MIXED["every third facet reversed, by viewpoint"]()
    by_viewpoint, by_winding = restate_topology_fast(verts, None, VIEWPOINT, vp), restate_topology_fast(verts, None)
    flipped = (by_viewpoint["nf"] != by_winding["nf"]).any(axis=1) & np.isfinite(by_winding["nf"]).all(axis=1)
    print("facets the viewpoint turns: %d; inconsistent edges by winding: %d" % (flipped.sum(), by_winding["stats"]["inconsistent_edges"]))
    assert flipped.sum() == 1280 and (by_viewpoint["nf"][np.isfinite(by_viewpoint["nf"][:, 2]), 2] > 0).all()
    assert by_viewpoint["stats"]["closed"] == 0 and by_viewpoint["stats"]["inconsistent_edges"] == 0
    assert by_winding["stats"]["inconsistent_edges"] > 1000


def test_big_sheet_counts_in_closed_form():
    nx, ny = BIG
    t = big_sheet_restated()
    assert t["slots"] == 1058400 > MERGE and sort_path(t["slots"]) == "onesweep" and len(big_sheet()) == 3 * 352800
    edges = nx * (ny + 1) + (nx + 1) * ny + nx * ny
    assert t["stats"] == dict(vertices=(nx + 1) * (ny + 1), edges=edges, border_edges=2 * (nx + ny), manifold_edges=edges - 2 * (nx + ny),
                              inconsistent_edges=0, nonmanifold_edges=0, border_vertices=2 * (nx + ny), irregular_vertices=0, closed=0)
    assert t["longest_run"] == 6 and t["longest_edge_run"] == 2


def test_long_runs_are_long():
    t = restate_topology_fast(cone(), None)
    assert (t["vertex_id"] == 0).sum() == 3000 == t["longest_run"] and t["longest_edge_run"] == 2
    assert t["stats"] == dict(vertices=3001, edges=6000, border_edges=3000, manifold_edges=3000, inconsistent_edges=0, nonmanifold_edges=0,
                              border_vertices=3000, irregular_vertices=0, closed=0)
    assert 3000 / 256 > 11                                                   # a dozen workgroups of the sorted order
    print("cone: peak partial sum %.3f, tolerance %.3e" % (t["peak"], vertex_tolerance(t)))
    t = restate_topology_fast(book(), None)
    assert (t["edge_id"] == 0).sum() == 300 == t["longest_edge_run"] and t["longest_run"] == 300
    assert (t["vertex_id"] == 0).sum() == 300 == (t["vertex_id"] == 1).sum()
    assert t["stats"] == dict(vertices=302, edges=601, border_edges=600, manifold_edges=0, inconsistent_edges=0, nonmanifold_edges=1,
                              border_vertices=302, irregular_vertices=2, closed=0)
    assert t["edge_class"][0, 0] == NONMANIFOLD and (t["vertex_bits"][:, :2] == V_BORDER | V_IRREGULAR).all()
    assert np.abs(t["edge_normal"][0, 0]).max() > 100                        # the pages' normals do not cancel: the spine's sign is no accident
    print("book: peak partial sum %.3f, tolerance %.3e" % (t["peak"], vertex_tolerance(t)))


def test_closing_spoke_has_an_alias_between_its_half_edges():
    """Sorted on one bit too few, vertex 1 + 2^(bits - 1) falls on vertex 1.  Only where a half-edge of (0, 1 + 2^(bits - 1)) lies
    BETWEEN the two of (0, 1) in slot order does a stable sort then split the run of (0, 1): the strips cannot show that (an id
    with the top bit belongs to the last triangles, whose slots come last), the fan's closing spoke can."""
    n = ALIAS_FAN
    t = restate_topology_fast(cone(n), None)
    S, bits = 3 * n, id_bits(3 * n)
    alias = 1 + 2 ** (bits - 1)
    assert bits == 11 and alias == 1025
    spoke = np.nonzero(t["edge_id"].ravel() == 0)[0]                          # the edge of apex 0 and rim 0 = vertex 1
    assert list(spoke) == [0, S - 1] and t["vertex_id"][0, 1] == 1
    other = np.nonzero((t["vertex_id"].ravel() == alias))[0]
    assert len(other) == 2 and t["vertex_id"].ravel()[alias] == alias
    between = np.nonzero(t["edge_id"].ravel() == t["edge_id"].ravel()[alias])[0]   # half-edge `alias` runs from rim 342 to the apex
    assert len(between) == 2 and (between > 0).all() and (between < S - 1).all()
    lo_hi = sorted((int(t["vertex_id"].ravel()[alias]), int(t["vertex_id"].ravel()[3 * (alias // 3)])))
    assert lo_hi == [0, alias] and t["stats"]["manifold_edges"] == n


def test_lamina_pseudonormals_vanish():
    v, t = lamina()
    topo = restate_topology_fast(v, t)
    one = restate_topology_fast(*sheet(10, 8, 2.0, 0.7))
    rim = np.repeat(one["edge_class"] == BORDER, 2, axis=0)                   # the twin's half-edges are its facet's, reversed
    rim[1::2] = rim[1::2][:, [1, 0, 2]]
    assert (topo["edge_class"][rim] == MANIFOLD).all() and (topo["edge_class"][~rim] == NONMANIFOLD).all()
    runs = np.bincount(topo["edge_id"].ravel())
    assert set(runs[runs > 0]) == {2, 4} and (runs[topo["edge_id"][~rim]] == 4).all() and (runs[topo["edge_id"][rim]] == 2).all()
    assert (topo["edge_normal"][rim] == 0).all() and (topo["vertex_normal"] == 0).all()
    assert (topo["edge_normal"] == 0).all()                                  # (the interior edges too: each twin cancels its facet at once)
    assert topo["stats"]["vertices"] == 99 and topo["stats"]["border_edges"] == 0 and topo["stats"]["manifold_edges"] == 36 and topo["stats"]["closed"] == 0
    assert (topo["nf"][1::2] == -topo["nf"][::2]).all()


@pytest.mark.parametrize("name", sorted(SUBNORMALS))
def test_subnormal_corners_are_positions(name):
    a, b = SUBNORMALS[name]
    verts = subnormal_pair(a, b)
    tiny = float(np.finfo(F32).tiny)
    for x, got in ((a, verts[0, 0]), (b, verts[3, 0])):
        assert float(got) == x and (x == 0 or 0 < abs(x) < tiny)              # a float32, subnormal, as written
    assert verts[0, 0] != verts[3, 0]
    st = restate_topology_fast(verts, None)["stats"]
    assert (st["vertices"], st["edges"], st["manifold_edges"], st["border_edges"]) == (4, 5, 1, 4)
    assert restate_topology(verts, None)["stats"] == st


# ---------------------------------------------------------------- GPU


def run_case(E, what, verts, tris=None, change_range=0, orient=WINDING, vp=None, picks=40, away=60, seed=0, piece=256, want=None, extra=None):
    """the topology for cells_for's two cells against the fast restatement (assert_topology; the vertex pseudonormals within
    vertex_tolerance), the maps independent of the cell, and probe_queries' signed queries against restate_signed: every map
    bit for bit but the pseudonormal, which is compared within the same tolerance.  Returns (restated topology, restated queries)"""
    verts = np.ascontiguousarray(verts, F32).reshape(-1, 3)
    fv = file_units(verts, change_range)
    rv = resident(E, fv, change_range)
    vp0 = (0, 0, 0) if vp is None else vp
    want = want or restate_topology_fast(rv, tris, orient, vp0)
    tol = vertex_tolerance(want)
    q = probe_queries(rv, tris, seed, picks, away)
    if extra is not None:
        q = np.concatenate([extra.astype(F32), q])
    ref = restate_signed_in_pieces(rv, tris, q, want, orient, vp0, piece)
    assert_margin(ref, what)
    hit = ref["status"] == MATCHED
    assert (~hit).sum() == 2
    e = E.Engine(0, change_range=change_range)
    worst, worst_q, first = 0.0, 0.0, None
    for cell in cells_for(rv):
        m = e.trimesh(fv, tris, cell=cell, orient=orient, viewpoint=vp)
        st, got = m.topology()
        worst = max(worst, assert_topology(st, got, want, "%s, cell %g" % (what, cell)))
        got.update(got_signed(m, q))
        for k in SIGNED_MAPS:
            if k != "pseudonormal":
                assert same_bits(got[k], ref[k]), (what, cell, k, np.nonzero(np.atleast_2d(got[k].T != ref[k].T).any(axis=0))[0][:8])
        assert (np.isnan(got["pseudonormal"]) == np.isnan(ref["pseudonormal"])).all()
        worst_q = max(worst_q, float(np.nanmax(np.abs(got["pseudonormal"] - ref["pseudonormal"]))))
        if first is not None:
            assert all(same_bits(first[k], got[k]) for k in got), "%s: the maps depend on the cell" % what
        first = got
        m.close()
    e.close()
    print("%s: %d slots (%s sort, %d id bits), longest runs %d corners / %d half-edges; %s" % (
        what, want["slots"], sort_path(want["slots"]), id_bits(want["slots"]), want["longest_run"], want["longest_edge_run"], want["stats"]))
    print("%s: largest pseudonormal difference %.3e in the maps, %.3e in %d queries; tolerance %.3e; features %s, fallback %d" % (
        what, worst, worst_q, len(q), tol, np.bincount(ref["feature"][hit], minlength=7), (ref["flags"][hit] & S_FALLBACK > 0).sum()))
    assert worst <= tol and worst_q <= tol
    return want, ref


@pytest.mark.gpu
@pytest.mark.parametrize("R", STRIPS)
def test_strips_at_the_id_bit_and_one_block_boundaries(engine_mod, R):
    want, ref = run_case(engine_mod, "strip of %d" % R, strip(R), seed=81 + R, picks=30, away=30)
    assert want["stats"]["vertices"] == R + 2 and want["stats"]["manifold_edges"] == R - 1
    assert (ref["tri_index"] >= R - 2).sum() >= 12                           # queries on the triangles of the highest ids


@pytest.mark.gpu
@pytest.mark.parametrize("change_range", [0, 1])
@pytest.mark.parametrize("name", sorted(MIXED))
def test_merge_path_sheet_with_everything_mixed(engine_mod, name, change_range):
    verts, tris, orient, vp = MIXED[name]()
    want, ref = run_case(engine_mod, "%s, change_range %d" % (name, change_range), verts, tris, change_range, orient, vp, seed=91, picks=60, away=120)
    assert sort_path(want["slots"]) == "merge" and (want["vertex_id"][:, 0] == -1).sum() == 1280
    assert want["stats"]["inconsistent_edges"] == 0 and want["stats"]["vertices"] == 49 * 41
    hit = ref["status"] == MATCHED
    assert (np.bincount(ref["feature"][hit], minlength=7) > 0).all() and (ref["signed_distance"] < 0).sum() > 50 < (ref["signed_distance"] > 0).sum()
    assert (want["vertex_id"][ref["tri_index"][hit], 0] >= 0).all()           # no degenerate wins


@pytest.mark.gpu
def test_onesweep_path_sheet(engine_mod):
    """1 058 400 slots, above the merge sort's 2^20.  64 queries: the brute force walks 352 800 triangles for each"""
    want, ref = run_case(engine_mod, "sheet %d x %d" % BIG, big_sheet(), seed=101, picks=5, away=2, piece=4, want=big_sheet_restated())
    assert len(ref["status"]) == 64 and sort_path(want["slots"]) == "onesweep"
    assert want["stats"]["vertices"] == 421 * 421


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(LONG_RUNS))
def test_long_runs_under_one_head(engine_mod, name):
    """the cone's apex: 3 000 corners in one run; the book's spine: 300 half-edges in one run and 300 corners at either end; the
    fan of 400, whose closing spoke's run a sort on one id bit too few would split.  The edge pseudonormals stay bit for bit;
    the vertex pseudonormals within vertex_tolerance() (its docstring has the derivation), printed beside what was seen"""
    want, ref = run_case(engine_mod, name, LONG_RUNS[name](), seed=111, picks=40, away=60)
    hit = ref["status"] == MATCHED
    assert want["longest_run"] == {"cone": 3000, "book": 300, "closing spoke": ALIAS_FAN}[name]
    assert ((ref["feature"] < 3) & hit & (ref["tri_index"] == 0)).sum() >= 2   # (ties at the apex / the spine's ends go to triangle 0)
    if name == "book":
        assert want["longest_edge_run"] == 300 and ((ref["feature"] >= 3) & (ref["feature"] < 6) & (ref["tri_index"] == 0)).sum() >= 2


@pytest.mark.gpu
def test_two_sided_lamina_falls_back_to_the_winning_facet(engine_mod):
    v, t = lamina()
    want, ref = run_case(engine_mod, "lamina", v, t, seed=121, picks=60, away=150, extra=beyond_the_rim(v, 10, 8, 122))
    hit = ref["status"] == MATCHED
    off = hit & (ref["distance"] > 0) & (ref["feature"] < 6)                  # off the surface, over an edge or a vertex
    print("lamina: %d queries off the surface over edges and vertices, %d over faces" % (off.sum(), (hit & (ref["feature"] == 6)).sum()))
    assert off.sum() >= 150 and (ref["feature"][off] < 3).sum() >= 30 and (ref["feature"][off] >= 3).sum() >= 30
    assert (ref["pseudonormal"][off] == 0).all() and (ref["flags"][off] & S_FALLBACK > 0).all()
    tied = off & (ref["feature"] < 3)                                        # at a vertex the facet and its twin are at one D2: the lower index
    assert (ref["tri_index"][tied] % 2 == 0).all()
    assert same_bits(ref["signed_distance"][off], np.copysign(ref["distance"][off], ref["deviation"][off]))
    assert (ref["deviation"][off] > 0).sum() >= 30 <= (ref["deviation"][off] < 0).sum()


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SUBNORMALS))
def test_subnormal_corners_stay_apart_on_the_device(engine_mod, name):
    verts = subnormal_pair(*SUBNORMALS[name])
    assert same_bits(resident(engine_mod, verts, 0), verts)                   # the upload keeps subnormals
    want, _ = run_case(engine_mod, name, verts, seed=131, picks=2, away=40)
    st = want["stats"]
    assert (st["vertices"], st["edges"], st["manifold_edges"], st["border_edges"]) == (4, 5, 1, 4)


@pytest.mark.gpu
def test_stl_file_gives_the_soups_topology(engine_mod, tmp_path):
    E = engine_mod
    fan = fan_cube()
    path = str(tmp_path / "fan_cube.stl")
    E.save_stl(path, fan)
    assert same_bits(E.load_stl(path).reshape(-1, 3), fan)
    q = np.concatenate([solid_queries(141, -0.4, 1.4, 300), fan[::5]])
    e = E.Engine(0, change_range=0)
    a, b = e.trimesh(fan), e.trimesh_stl(path)
    (sa, ta), (sb, tb) = a.topology(), b.topology()
    assert sa == sb == dict(restate_topology_fast(fan, None)["stats"]) and sa["closed"] == 1
    assert all(same_bits(ta[k], tb[k]) for k in ta)
    ga, gb = got_signed(a, q), got_signed(b, q)
    assert all(same_bits(ga[k], gb[k]) for k in SIGNED_MAPS)
    assert (ga["status"] == MATCHED).all() and (ga["signed_distance"] < 0).sum() > 20 and len(set(ga["feature"])) == 7
    a.close(); b.close(); e.close()
