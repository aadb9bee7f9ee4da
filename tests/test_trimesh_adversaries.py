"""The triangle grid off its easy cases: meshes of thousands of triangles with degenerates interleaved, the
automatic cell and its doubling, the capacity refusals, a finite max_dist on a real grid, and queries on cell faces of meshes far
from the origin and of slab-shaped grids.  The yardstick is test_trimesh's nearest_on_mesh(), the brute force over all indexed
triangles on the resident vertices; every comparison of maps is assert_same_maps: equal bytes.  What a case must have to mean
anything (a doubling, a pair count past 2^32, both statuses side by side, ties) is asserted on the restatement alone, before
the engine is looked at.

Not pinned here: an automatic grid that doubles because of the PAIR cap.  Such a grid ends with at least 2^28 pairs, gigabytes
of lists; the automatic path shares the `fits` expression (pairs <= TM_MAX_PAIRS after the saturating scan) that the refusal of
an explicit cell tests in test_pair_count_is_refused_where_a_wrapping_sum_would_pass."""
import functools

import numpy as np
import pytest

from test_mesh_cloud import rand_triangles, resident, same_bits
from test_trimesh import (DROPPED, INF, MAPS, MATCHED, NONE, TOO_FAR, assert_same_maps, closest_on_triangles, file_units, frames, got_maps,
                          nearest_on_mesh, sheet, soup_case)

F32 = np.float32
MAX_CELLS = 2 ** 24                                                          # TM_MAX_CELLS
MAX_PAIRS = 2 ** 31 - 2                                                      # TM_MAX_PAIRS
CLOUD_MAX = (2 ** 31 - 1) // 8                                               # the points of a resident cloud


# ---------------------------------------------------------------- the build, restated


def show(what, st):
    print("%s: %s" % (what, {k: v for k, v in st.items() if k not in ("mn", "mx")}))


def boxes(rv, tris):
    """(lo, hi float64[indexed, 3], valid bool[n_tris]): the boxes of the indexed triangles, resident floats widened"""
    p0, p1, p2, _, _, valid = frames(rv, tris)
    v = np.stack([p0, p1, p2], axis=1)[valid]
    return v.min(axis=1), v.max(axis=1), valid


def grid_dims(mn, mx, cell):
    """floor((mx - mn) / cell) + 1 per axis in double; None where an axis or the product is above 2^24"""
    d = np.floor((mx - mn) / float(cell)) + 1.0
    if (d > MAX_CELLS).any() or d.prod() > MAX_CELLS:
        return None
    return tuple(int(x) for x in d)


def cell_ranges(lo, hi, mn, cell, dims):
    """the cells per axis that each box overlaps: floor((x - mn) / cell) in double per corner, clamped into [0, dim)"""
    d = np.array(dims, np.float64) - 1
    return (np.clip(np.floor((lo - mn) / float(cell)), 0, d).astype(np.int64), np.clip(np.floor((hi - mn) / float(cell)), 0, d).astype(np.int64))


def pair_stats(lo, hi, mn, cell, dims):
    """(pairs, max_per_cell) by expanding every (triangle, cell) pair and counting per cell"""
    a, b = cell_ranges(lo, hi, mn, cell, dims)
    n = b - a + 1
    per = n.prod(axis=1)
    own = np.repeat(np.arange(len(per)), per)
    k = np.arange(per.sum()) - (np.cumsum(per) - per)[own]
    ix = a[own, 0] + k % n[own, 0]
    k = k // n[own, 0]
    iy, iz = a[own, 1] + k % n[own, 1], a[own, 2] + k // n[own, 1]
    key = (iz * dims[1] + iy) * dims[0] + ix
    return int(per.sum()), int(np.bincount(key, minlength=int(np.prod(dims))).max())


def automatic_cell(rv, tris):
    """(cell0, k, cell float32, dims): the mean longest box side in 2^-32 of the extent, an integer sum, as a float32; doubled
    until the dims fit"""
    lo, hi, _ = boxes(rv, tris)
    mn, mx = lo.min(axis=0), hi.max(axis=0)
    extent = float((mx - mn).max())
    side = (hi - lo).max(axis=1)
    total = int(np.rint(side / extent * 2.0 ** 32).astype(np.int64).sum(dtype=np.int64))
    cell0 = F32(float(total) / float(len(side)) / 2.0 ** 32 * extent)
    k, cell = 0, cell0
    while grid_dims(mn, mx, cell) is None:
        k, cell = k + 1, F32(cell * F32(2))
    return cell0, k, cell, grid_dims(mn, mx, cell)


def ordered_extreme(corner, pick):
    """the smallest (np.argmin) or largest (np.argmax) float32 per axis in the order of the floats' bits, sign folded: -0 is below
    +0 there, which a comparison of values leaves open"""
    c = np.ascontiguousarray(corner.astype(F32))
    bits = c.view(np.uint32).astype(np.int64)
    key = np.where(bits >> 31, 0xffffffff - bits, bits + 0x80000000)
    return c[pick(key, axis=0), np.arange(3)]


def assert_stats_match(st, rv, tris, pairs=True):
    """the build's statistics against the restatement: counts, box, dims, and (unless the lists are too long to expand) the pairs"""
    lo, hi, valid = boxes(rv, tris)
    assert (st["triangles"], st["indexed"], st["degenerate"]) == (len(valid), int(valid.sum()), int((~valid).sum()))
    mn, mx = lo.min(axis=0), hi.max(axis=0)
    assert same_bits(st["mn"], ordered_extreme(lo, np.argmin)) and same_bits(st["mx"], ordered_extreme(hi, np.argmax))
    dims = grid_dims(mn, mx, F32(st["cell"]))
    assert st["cells"] == dims, (st["cells"], dims)
    a, b = cell_ranges(lo, hi, mn, F32(st["cell"]), dims)
    assert st["pairs"] == int((b - a + 1).prod(axis=1).sum())
    if pairs:
        want = pair_stats(lo, hi, mn, F32(st["cell"]), dims)
        assert (st["pairs"], st["max_per_cell"]) == want, (st["pairs"], st["max_per_cell"], want)


def limited(want, max_dist):
    """nearest_on_mesh(..., max_dist) from its unlimited answer: beyond the limit the maps hold TOO_FAR / NaN / -1 / 255"""
    md2 = float(F32(max_dist)) * float(F32(max_dist))
    far = (want["status"] == MATCHED) & ~(want["D2"] <= md2)
    out = {k: want[k].copy() for k in MAPS}
    out["status"][far] = TOO_FAR
    out["tri_index"][far] = -1
    out["region"][far] = NONE
    for k in ("distance", "closest", "deviation"):
        out[k][far] = np.nan
    return out


def shares(want, max_dist):
    """(share MATCHED, share TOO_FAR) of the reference under this limit"""
    s = limited(want, max_dist)["status"]
    return float((s == MATCHED).mean()), float((s == TOO_FAR).mean())


def face_queries(st, rng, most=None, per_box_face=10):
    """queries on the interior faces of the grid on each axis, at float32(mn + k cell) and one ulp to both sides, and on the six
    faces of the box and one ulp outside them; the other coordinates uniform in the box.  most: at most that many faces per axis"""
    mn, mx, cell = st["mn"].astype(np.float64), st["mx"].astype(np.float64), float(F32(st["cell"]))
    up, down = F32(np.inf), F32(-np.inf)
    q = []

    def at(xs, d):
        p = rng.uniform(mn, mx, (len(xs), 3)).astype(F32)
        p[:, d] = xs
        q.append(p)

    for d in range(3):
        k = np.arange(1, st["cells"][d])
        if most is not None and len(k) > most:
            k = np.sort(rng.choice(k, most, replace=False))
        x = (mn[d] + k * cell).astype(F32)
        for xs in (x, np.nextafter(x, down), np.nextafter(x, up)):
            at(xs, d)
        for face, outward in ((st["mn"][d], down), (st["mx"][d], up)):
            at(np.full(per_box_face, face, F32), d)
            at(np.full(per_box_face, np.nextafter(F32(face), outward), F32), d)
    return np.concatenate(q)


# ---------------------------------------------------------------- CPU: the helpers themselves


def test_limited_is_the_reference_with_a_limit():
    rng = np.random.default_rng(31)
    tri = rand_triangles(rng, 30, 3.0, 10.0).reshape(-1, 3)
    q = rng.uniform(-20, 20, (80, 3)).astype(F32)
    q[7] = np.nan
    free = nearest_on_mesh(tri, None, q)
    for md in (2.0, 5.0, 9.0):
        want = nearest_on_mesh(tri, None, q, max_dist=md)
        print("max_dist %g: statuses %s" % (md, np.bincount(want["status"], minlength=4)))
        if md == 5.0:
            assert (want["status"] == TOO_FAR).sum() >= 10 and (want["status"] == MATCHED).sum() >= 10
        assert_same_maps(limited(free, md), want, "max_dist %g" % md)


def test_pair_expansion_counts_a_known_grid():
    lo = np.array([[0.0, 0.0, 0.0], [0.5, 0.5, 0.5], [0.2, 0.0, 0.0]])
    hi = np.array([[1.0, 1.0, 0.0], [0.6, 2.5, 0.5], [9.0, 0.2, 0.0]])              # 2 x 2 x 1, 1 x 3 x 1, 2 x 1 x 1 after the clamp
    assert pair_stats(lo, hi, np.zeros(3), 1.0, (2, 3, 1)) == (9, 3)
    assert grid_dims(np.zeros(3), np.array([255.5, 255.5, 255.5]), 1.0) == (256, 256, 256)
    assert grid_dims(np.zeros(3), np.array([256.0, 255.5, 255.5]), 1.0) is None


# ---------------------------------------------------------------- 1. thousands of triangles, degenerates interleaved


@functools.lru_cache(maxsize=None)
def wavy_sheet():
    """sheet(96, 96, 1.0, wave=2.0) with every 7th triangle made degenerate, three ways in turn: a repeated index, an index
    >= n_verts, an index of an extra NaN vertex.  (verts, tris, degenerate bool[n_tris])"""
    v, t = sheet(96, 96, 1.0, wave=2.0)
    nan_vertex = len(v)
    v = np.concatenate([v, np.array([[np.nan, 0, 0]], F32)])
    t = t.copy()
    f = np.arange(0, len(t), 7)
    way = (f // 7) % 3
    t[f[way == 0], 1] = t[f[way == 0], 0]
    t[f[way == 1], 2] = len(v) + 5
    t[f[way == 2], 0] = nan_vertex
    bad = np.zeros(len(t), bool)
    bad[f] = True
    return v, t, bad


@functools.lru_cache(maxsize=None)
def wavy_reference(engine_mod):
    v, t, bad = wavy_sheet()
    rv = resident(engine_mod, v, 0)
    lo, hi, valid = boxes(rv, t)
    assert len(t) == 18432 and (valid == ~bad).all()
    mn, mx = lo.min(axis=0), hi.max(axis=0)
    rng = np.random.default_rng(41)
    q = [rng.uniform(mn, mx, (700, 3))]
    for d in range(3):                                                       # outside on every side
        for sign in (-1, 1):
            p = rng.uniform(mn, mx, (50, 3))
            p[:, d] = (mx[d] if sign > 0 else mn[d]) + sign * rng.uniform(0.05, 20.0, 50)
            q.append(p)
    good = np.nonzero(valid)[0]
    on_vertex = rv[t[rng.choice(good, 250), rng.integers(0, 3, 250)]].astype(np.float64)
    e = t[rng.choice(good, 250)]
    above_edge = ((rv[e[:, 0]] + rv[e[:, 1]]) * F32(0.5)).astype(np.float64) + np.array([0, 0, 0.75])
    q += [on_vertex, above_edge]
    q = np.concatenate(q).astype(F32)
    assert len(q) == 1500
    want = nearest_on_mesh(rv, t, q, chunk=64)
    # ties: a query on a vertex is at D2 = 0 from every indexed triangle around it
    p0, p1, p2 = (z[valid][None] for z in frames(rv, t)[:3])
    probe = np.concatenate([np.arange(1000, 1064), np.arange(1250, 1314)])
    _, D2, _ = closest_on_triangles(q[probe].astype(np.float64)[:, None, :], p0, p1, p2)
    ties = (D2 == D2.min(axis=1, keepdims=True)).sum(axis=1)
    return rv, q, want, ties


@pytest.mark.gpu
def test_large_sheet_with_degenerates_interleaved(engine_mod):
    v, t, bad = wavy_sheet()
    rv, q, want, ties = wavy_reference(engine_mod)
    print("probed queries by number of tied triangles:", np.bincount(ties))
    assert (ties >= 2).sum() > 0 and (want["status"] == MATCHED).all()
    assert not bad[want["tri_index"]].any()
    md = 1.5                                                                 # a limit too, on the large grid
    near, far = shares(want, md)
    assert near > 0.15 and far > 0.15, (near, far)
    e = engine_mod.Engine(0, change_range=0)
    for what, cell in (("automatic", 0.0), ("cell 0.37", 0.37), ("cell 25", 25.0)):
        m = e.trimesh(v, t, cell=cell)
        show(what, m.stats)
        assert_stats_match(m.stats, rv, t)
        if cell == 0.37:
            assert 200000 < m.stats["pairs"] < 1000000
        if cell == 25.0:
            assert m.stats["max_per_cell"] > 500
        got = got_maps(m, q)
        assert_same_maps(got, want, what)
        assert not bad[got["tri_index"]].any()
        assert_same_maps(got_maps(m, q, md), limited(want, md), what + ", max_dist %g" % md)
        m.close()
    e.close()


@pytest.mark.gpu
def test_mesh_deviation_reads_the_large_grid_as_nearest_does(engine_mod):
    """ppp_get_mesh_deviation's q4 input path against ppp_trimesh_nearest's packed one on the same resident points, and both
    against the brute force on the part of the scan that test 1 has a reference for"""
    v, t, bad = wavy_sheet()
    rv, q, want, _ = wavy_reference(engine_mod)
    rng = np.random.default_rng(42)
    mn, mx = np.nanmin(rv, axis=0).astype(np.float64), np.nanmax(rv, axis=0).astype(np.float64)
    extra = rng.uniform(mn - [5, 5, 3], mx + [5, 5, 3], (2500, 3)).astype(F32)
    extra[rng.choice(len(extra), 40, replace=False)] = np.nan
    extra[rng.choice(len(extra), 10, replace=False), 2] = np.inf
    scan = np.concatenate([q, extra])
    md = 1.5
    e = engine_mod.Engine(0, change_range=0)
    e.set_cloud(scan)
    P = e.cloud()
    assert same_bits(P[:len(q)], q)
    m = e.trimesh(v, t)
    show("automatic", m.stats)
    _, _, dist, idx, region, status, _, stats = e.mesh_deviation(m, max_dist=md)
    got = got_maps(m, P, md)
    print("matched %d, too far %d, dropped %d of %d" % (stats["matched"], stats["too_far"], stats["dropped"], len(P)))
    for k, g in (("status", status), ("tri_index", idx), ("distance", dist), ("region", region)):
        assert same_bits(g, got[k]), k
        assert same_bits(g[:len(q)], limited(want, md)[k]), k
    assert stats["dropped"] >= 40 and stats["matched"] > 1000 and stats["too_far"] > 300
    assert (status[np.isnan(P).any(axis=1)] == DROPPED).all() and not bad[idx[status == MATCHED]].any()
    m.close()
    e.close()


# ---------------------------------------------------------------- 2. the automatic cell and its doubling


@pytest.mark.gpu
def test_automatic_cell_restated_and_doubled(engine_mod):
    """the accepted cell is cell0 2^k for the smallest k whose dims fit.  The sheet of test 1 fits at once (k = 0); the dust mesh,
    4000 triangles of size 0.02 over +-100, needs k >= 3 and leaves a grid of mostly empty cells: a query walks many shells.  Only
    eight queries lie far outside the box, since each of them walks the whole grid in one thread."""
    e = engine_mod.Engine(0, change_range=0)
    v, t, _ = wavy_sheet()
    rv = resident(engine_mod, v, 0)
    cell0, k, cell, dims = automatic_cell(rv, t)
    print("sheet: cell0 %.9g, k %d, dims %s" % (cell0, k, dims))
    assert k == 0
    m = e.trimesh(v, t)
    show("sheet", m.stats)
    assert same_bits(F32(m.stats["cell"]), cell) and m.stats["cells"] == dims
    m.close()

    rng = np.random.default_rng(43)
    dust = rand_triangles(rng, 4000, 0.02, 100.0).reshape(-1, 3)
    rv = resident(engine_mod, dust, 0)
    cell0, k, cell, dims = automatic_cell(rv, None)
    print("dust: cell0 %.9g, k %d, cell %.9g, dims %s" % (cell0, k, cell, dims))
    assert k >= 3 and same_bits(cell, F32(float(cell0) * 2.0 ** k))
    mn, mx = rv.min(axis=0).astype(np.float64), rv.max(axis=0).astype(np.float64)
    centre, half = (mn + mx) / 2, (mx - mn) / 2
    far = centre + 3 * half * np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, 0, -1], [1, 1, 0], [1, 1, 1], [-1, 1, -1], [0, -1, 1]], np.float64)
    q = np.concatenate([rng.uniform(mn, mx, (1000, 3)), far]).astype(F32)
    want = nearest_on_mesh(rv, None, q, chunk=64)
    m = e.trimesh(dust)
    show("dust", m.stats)
    assert same_bits(F32(m.stats["cell"]), cell) and m.stats["cells"] == dims
    assert_stats_match(m.stats, rv, None)
    assert m.stats["pairs"] < 8 * 4000                                       # the re-count of the accepted pass, not of the first
    assert_same_maps(got_maps(m, q), want, "dust")
    m.close()
    e.close()


# ---------------------------------------------------------------- 3. capacity: pairs, not cells


def spanning_triangles(rng, n, half=31.0):
    """n skew triangles whose boxes are each the whole cube [-half, half]^3"""
    b = rng.uniform(-0.9 * half, 0.9 * half, (n, 2))
    tri = np.empty((n, 3, 3))
    tri[:, 0] = -half
    tri[:, 1] = np.stack([np.full(n, half), np.full(n, half), b[:, 0]], axis=1)
    tri[:, 2] = np.stack([b[:, 1], np.full(n, half), np.full(n, half)], axis=1)
    for i in range(n):
        tri[i] = tri[i][:, rng.permutation(3)] * rng.choice([-1.0, 1.0], 3)
    return tri.astype(F32)


def spanning_mesh(n):
    rng = np.random.default_rng(44)
    small = rand_triangles(rng, 200, 1.0, 29.0)
    return np.concatenate([small[:100], spanning_triangles(rng, n), small[100:]]).reshape(-1, 3)


@pytest.mark.gpu
def test_pair_count_is_refused_where_a_wrapping_sum_would_pass(engine_mod):
    E = engine_mod
    e = E.Engine(0, change_range=0)
    for n in (300, 600):
        verts = spanning_mesh(n)
        rv = resident(E, verts, 0)
        lo, hi, valid = boxes(rv, None)
        assert valid.all()
        mn, mx = lo.min(axis=0), hi.max(axis=0)
        extent = float((mx - mn).max())
        cell = F32(extent / 200)
        dims = grid_dims(mn, mx, cell)
        assert dims is not None                                              # the cells fit: the pairs do not
        a, b = cell_ranges(lo, hi, mn, cell, dims)
        per = (b - a + 1).prod(axis=1)
        count = sum(int(c) for c in per)
        print("%d spanning triangles: dims %s, %d cells, %d pairs = 2^32 + %d" % (n, dims, np.prod(dims), count, count - 2 ** 32))
        assert (per[100:100 + n] == np.prod(dims)).all()
        if n == 300:
            assert 2 ** 31 - 1 < count < 2 ** 32
        else:
            assert count > 2 ** 32 and count % 2 ** 32 <= MAX_PAIRS          # a sum modulo 2^32 would be accepted
        with pytest.raises(E.PPPError) as ei:
            e.trimesh(verts, cell=float(cell))
        assert ei.value.code == E.ERR_CAPACITY and ei.value.handle is None
        st = ei.value.stats
        assert (st["triangles"], st["indexed"], st["degenerate"]) == (n + 200, n + 200, 0)
    # control: the same 600 at a cell ten times as large build, and answer as the brute force does, out of lists of 600 and more
    cell = F32(extent / 20)
    m = e.trimesh(verts, cell=float(cell))
    show("control", m.stats)
    assert_stats_match(m.stats, rv, None)
    assert 3000000 < m.stats["pairs"] < 8000000 and m.stats["max_per_cell"] >= 600
    q = np.random.default_rng(45).uniform(-35, 35, (1000, 3)).astype(F32)
    want = nearest_on_mesh(rv, None, q, chunk=64)
    print("winners among the spanning triangles: %d of %d" % (((want["tri_index"] >= 100) & (want["tri_index"] < 700)).sum(), len(q)))
    assert_same_maps(got_maps(m, q), want, "control")
    m.close()
    e.close()


def sampler_rows(rv, pitch):
    """the sampler's rows per triangle of a soup: max(1, ceil(hgt / pitch)), hgt = A2 / L on the rotated frame"""
    p0, p1, _, _, A2, valid = frames(rv, None)
    d = p1 - p0
    L = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    assert valid.all()
    return np.maximum(1.0, np.ceil(A2 / L / float(pitch)))


@pytest.mark.gpu
def test_sampler_row_sum_past_2_32_is_refused(engine_mod):
    """ppp_set_cloud_mesh has the same sums.  At the smallest pitch the argument checks admit, the smallest positive float, four
    triangles of height (2^30 + 128) pitches have fewer than 2^31 rows each and 2^32 + 512 together: modulo 2^32 that is 512
    rows, which the row check would let through."""
    E = engine_mod
    from polishpathplanning_amd import synth
    pts, cfg = synth.make_config("tiny_5k")
    e = E.Engine(0, change_range=0, tool_radius=cfg["tool_radius"])
    e.set_cloud((pts * F32(1000)).astype(F32))
    e.gen_path(); e.get_path()
    cloud0, wp0 = e.cloud(), e.waypoints()

    def unchanged():
        assert same_bits(e.cloud(), cloud0)
        e.gen_path(); e.get_path()
        assert same_bits(e.waypoints(), wp0)

    pitch = F32(2.0 ** -149)
    assert pitch > 0 and np.nextafter(pitch, F32(0)) == 0
    h = F32((2.0 ** 30 + 128) * 2.0 ** -149)
    assert float(h) == (2.0 ** 30 + 128) * 2.0 ** -149                       # (a float: 2^-119 (1 + 2^-23))
    base = np.array([[0, 0, 0], [2, 0, 0], [1, 1, 0]], np.float64) * float(h)   # the base is the longest edge, the height is h
    tris = np.stack([base, base[:, [2, 0, 1]], base[:, [1, 2, 0]], -base]).astype(F32)
    verts = tris.reshape(-1, 3)
    anchor = np.array([[-50, -50, -50], [50, 50, 50]], F32)                  # (the cloud that is read back has an extent)
    rv = resident(E, np.concatenate([verts, anchor]), 0)[:len(verts)]
    rows = sampler_rows(rv, pitch)
    total = sum(int(r) for r in rows)
    print("rows per triangle %s, together 2^32 + %d" % (rows.astype(np.int64), total - 2 ** 32))
    assert (rows < 2 ** 31).all() and total > 2 ** 32 and 0 < total % 2 ** 32 <= CLOUD_MAX
    with pytest.raises(E.PPPError) as ei:
        e.set_cloud_mesh(verts, None, pitch=float(pitch))
    assert ei.value.code == E.ERR_CAPACITY
    assert (ei.value.stats["triangles"], ei.value.stats["sampled"], ei.value.stats["samples"]) == (4, 4, 0)
    unchanged()
    e.close()


# ---------------------------------------------------------------- 4. a finite max_dist on a real grid


@functools.lru_cache(maxsize=None)
def limit_case(engine_mod):
    """(rv, cell, q, want): test_trimesh's 200-triangle soup, its automatic cell, and about 2000 queries -- half of them beside the
    triangles at 0.01 to 10 cells, half uniform in a box that is widened until, for every limit of 0.25, 1 and 4 cells, the
    reference has at least 15 % MATCHED and at least 15 % TOO_FAR"""
    verts = soup_case(0)
    rv = resident(engine_mod, verts, 0)
    e = engine_mod.Engine(0, change_range=0)
    m = e.trimesh(verts)
    cell = F32(m.stats["cell"])
    m.close()
    e.close()
    rng = np.random.default_rng(46)
    tri = rv.reshape(-1, 3, 3).astype(np.float64)
    w = rng.dirichlet([1, 1, 1], 1000)
    on = (tri[rng.integers(0, len(tri), 1000)] * w[:, :, None]).sum(axis=1)
    step = rng.normal(size=(1000, 3))
    step *= (float(cell) * 10.0 ** rng.uniform(-2, 1, 1000) / np.linalg.norm(step, axis=1))[:, None]
    mn, mx = rv.min(axis=0).astype(np.float64), rv.max(axis=0).astype(np.float64)
    u = rng.uniform(0, 1, (1000, 3))
    for widen in np.arange(0.0, 8.25, 0.25):
        q = np.concatenate([on + step, (mn - widen * (mx - mn)) + u * (1 + 2 * widen) * (mx - mn)]).astype(F32)
        want = nearest_on_mesh(rv, None, q)
        if all(min(shares(want, F32(float(cell) * mult))) >= 0.15 for mult in (0.25, 1.0, 4.0)):
            break
    print("query box widened by %.2f extents on every side" % widen)
    return rv, cell, q, want


@pytest.mark.gpu
def test_finite_max_dist_on_a_real_grid(engine_mod):
    verts = soup_case(0)
    rv, cell, q, free = limit_case(engine_mod)
    limits = []
    for mult in (0.25, 1.0, 4.0):
        md = F32(float(cell) * mult)
        near, far = shares(free, md)
        print("max_dist %.9g (%.2f cells): %.1f %% MATCHED, %.1f %% TOO_FAR in the reference" % (md, mult, 100 * near, 100 * far))
        assert near >= 0.15 and far >= 0.15
        limits.append(("%.2f cells" % mult, md, None, None))
    # the limit at float32(sqrt(D2)) of a query: its square lies below that query's D2 (the query is TOO_FAR) or above it (MATCHED)
    D2 = free["D2"]
    root = np.sqrt(D2).astype(F32)
    back = root.astype(np.float64) * root.astype(np.float64)
    mid = (D2 > np.quantile(D2, 0.3)) & (D2 < np.quantile(D2, 0.7))
    below, above = np.nonzero(mid & (back < D2))[0][0], np.nonzero(mid & (back > D2))[0][0]
    limits += [("the root of query %d's D2, rounded down" % below, root[below], below, TOO_FAR),
               ("the root of query %d's D2, rounded up" % above, root[above], above, MATCHED)]
    # ... and exactly on it: beyond the vertex of the largest x, straight along x, D2 is the square of a float
    top = int(rv[:, 0].argmax())
    assert (np.delete(rv[:, 0], top) < rv[top, 0]).all()
    beyond = rv[top] + F32([3.0, 0, 0])
    gap = F32(beyond[0] - rv[top, 0])
    assert float(gap) == float(beyond[0]) - float(rv[top, 0])
    q = np.concatenate([q, beyond[None]])
    last = nearest_on_mesh(rv, None, beyond[None])
    assert last["D2"][0] == float(gap) * float(gap) and last["tri_index"][0] == top // 3
    free = {k: np.concatenate([free[k], last[k]]) for k in free}
    limits += [("exactly query %d's distance" % (len(q) - 1), gap, len(q) - 1, MATCHED),
               ("one ulp below query %d's distance" % (len(q) - 1), np.nextafter(gap, F32(0)), len(q) - 1, TOO_FAR)]
    wants = []
    for what, md, pick, status in limits:
        want = nearest_on_mesh(rv, None, q, max_dist=md)
        assert_same_maps(limited(free, md), want, what)                      # (the restatement with itself)
        if pick is not None:
            assert want["status"][pick] == status, (what, want["status"][pick])
        wants.append(want)
    extent = float((rv.max(axis=0).astype(np.float64) - rv.min(axis=0)).max())
    e = engine_mod.Engine(0, change_range=0)
    for name, c in (("automatic", 0.0), ("box / 64", extent / 64)):
        m = e.trimesh(verts, cell=c)
        show(name, m.stats)
        for (what, md, _, _), want in zip(limits, wants):
            assert_same_maps(got_maps(m, q, md), want, "%s, max_dist %s" % (name, what))
        m.close()
    e.close()


# ---------------------------------------------------------------- 5. faces, ulps, offsets, slabs


@pytest.mark.gpu
@pytest.mark.parametrize("change_range", [0, 1])
def test_cell_faces_of_a_mesh_far_from_the_origin(engine_mod, change_range):
    """the 200-triangle soup moved by (60000, -30000, 10000) mm -- (60, -30, 10) in a file in metres --: a float's ulp is 2^-8 mm
    there.  Queries on every interior face of the grid and one ulp to both sides, on the box's faces and one ulp outside."""
    moved = (soup_case(0) + F32([60000, -30000, 10000])).astype(F32)
    verts = file_units(moved, change_range)
    rv = resident(engine_mod, verts, change_range)
    extent = float((rv.max(axis=0).astype(np.float64) - rv.min(axis=0)).max())
    rng = np.random.default_rng(47)
    e = engine_mod.Engine(0, change_range=change_range)
    for what, cell in (("automatic", 0.0), ("box / 128", extent / 128))[:1 if change_range else 2]:
        m = e.trimesh(verts, cell=cell)
        st = m.stats
        show(what, st)
        assert_stats_match(st, rv, None, pairs=cell == 0.0)
        mn, mx = st["mn"].astype(np.float64), st["mx"].astype(np.float64)
        q = np.concatenate([face_queries(st, rng), rng.uniform(mn, mx, (500, 3)).astype(F32)])
        print("%d queries" % len(q))
        assert len(q) == 3 * (sum(st["cells"]) - 3) + 6 * 20 + 500         # every interior face three times
        want = nearest_on_mesh(rv, None, q)
        assert (want["status"] == MATCHED).all()
        assert_same_maps(got_maps(m, q), want, what)
        m.close()
    e.close()


def slab_queries(mn, mx, rng, whole_grid=True):
    """inside, above, below and beside the box, three 1000 along z, and (whole_grid) three 10^6 along z: for those the bound never
    passes the best D2, which TM_REL holds above it, so the lateral shells run out and the block covers the grid"""
    q = [rng.uniform(mn, mx, (200, 3))]
    for sign in (-1, 1):
        p = rng.uniform(mn, mx, (100, 3))
        p[:, 2] = (mx[2] if sign > 0 else mn[2]) + sign * rng.uniform(0.01, 30.0, 100)
        q.append(p)
        for d in (0, 1):
            p = rng.uniform(mn, mx, (25, 3))
            p[:, d] = (mx[d] if sign > 0 else mn[d]) + sign * rng.uniform(0.01, 10.0, 25)
            q.append(p)
    c = (mn + mx) / 2
    q.append(np.array([[c[0], c[1], 1e3], [c[0], c[1], -1e3], [mn[0], mx[1], 1e3]]))
    if whole_grid:
        q.append(np.array([[c[0], c[1], 1e6], [mx[0], mn[1], -1e6], [c[0] + 1, c[1] - 2, -1e6]]))
    return np.concatenate(q).astype(F32)


@pytest.mark.gpu
def test_slab_grids_and_a_planar_sheet(engine_mod):
    """a sheet whose box is 200 x 200 x 0.5: one layer of cells (cell 1.0), a few layers under many columns (the smallest cell of
    the ladder 0.1 (1 + j / 64) whose dims fit), and an exactly planar sheet, whose z extent is 0.  The queries that walk the
    whole grid are left out of the grid of a few layers: it has 1.7 10^7 cells, and each such query took seconds in one thread."""
    e = engine_mod.Engine(0, change_range=0)
    rng = np.random.default_rng(48)
    v, t = sheet(40, 40, 5.0, wave=0.25)
    rv = resident(engine_mod, v, 0)
    mn, mx = rv.min(axis=0).astype(np.float64), rv.max(axis=0).astype(np.float64)
    assert (mx - mn)[0] == 200 == (mx - mn)[1] and 0.45 < (mx - mn)[2] <= 0.5
    fine = next(c for c in (F32(0.1 * (1 + j / 64)) for j in range(64)) if grid_dims(mn, mx, c) is not None)
    assert grid_dims(mn, mx, F32(0.1)) is None and grid_dims(mn, mx, F32(1.0))[2] == 1 and 2 <= grid_dims(mn, mx, fine)[2] <= 5
    for what, cell in (("one layer", 1.0), ("a few layers", float(fine))):
        m = e.trimesh(v, t, cell=cell)
        show(what, m.stats)
        assert_stats_match(m.stats, rv, t, pairs=False)
        assert m.stats["cells"] == grid_dims(mn, mx, F32(cell))
        q = np.concatenate([slab_queries(mn, mx, rng, whole_grid=cell == 1.0), face_queries(m.stats, rng, most=30, per_box_face=5)])
        want = nearest_on_mesh(rv, t, q, chunk=64)
        assert_same_maps(got_maps(m, q), want, what)
        m.close()
    v, t = sheet(32, 32, 2.0)
    rv = resident(engine_mod, v, 0)
    mn, mx = rv.min(axis=0).astype(np.float64), rv.max(axis=0).astype(np.float64)
    assert mn[2] == 0 == mx[2]
    base = slab_queries(mn, mx, rng)
    for what, cell in (("planar, automatic", 0.0), ("planar, cell 1.3", 1.3)):
        m = e.trimesh(v, t, cell=cell)
        show(what, m.stats)
        assert_stats_match(m.stats, rv, t)
        assert m.stats["cells"][2] == 1
        q = np.concatenate([base, face_queries(m.stats, rng, most=30, per_box_face=5)])
        want = nearest_on_mesh(rv, t, q, chunk=64)
        assert_same_maps(got_maps(m, q), want, what)
        m.close()
    e.close()
