"""Connected regions of selected cloud points (ppp_get_regions): the connected components of a
per-point selection under "closer than a link radius", each with its label (smallest cloud index), size, bounding box and
fixed-point centroid.

The restatement is independent of the engine: scipy's k-d tree proposes the pairs within 1.001 r, every pair is re-tested with
the float32 expression the engine's radius searches use (flann_dist2 of test_contact_field against the float32 product r * r),
scipy.sparse.csgraph labels the components, numpy restates the rows.  Both sides decide a link by the same float32 comparison,
so every comparison below is for equality: labels arrays equal, rows equal field by field, floats by bits, centroids ==.  The
restatement also counts the candidate pairs within 4e-7 r2 of the threshold and prints the count, so that a mismatch could be
told from a last-bit question at a glance; it is a printed figure, not a condition."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components
from scipy.spatial import cKDTree

from polishpathplanning_amd import synth
from test_contact_field import RELEASED_DEPTH, bits
from test_path_coverage import V1, cloud_of, restate_path_coverage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXED = float(1 << 20)
MASK = 3  # PPP_REGIONS_MASK
# the four passes whose uncovered sets the regions were first counted on (oracle + scipy, link 2.5 mm):
# (cloud, parameters, uncovered points, regions)
PASSES = [
    ("small_40k", dict(walk=0, pairing=0, dynamic_adjustment=0), 858, 47),
    ("small_40k", dict(walk=1, pairing=0, dynamic_adjustment=1), 1708, 489),
    ("small_40k", dict(walk=0, pairing=0, dynamic_adjustment=0, depth=RELEASED_DEPTH), 12190, 163),
    ("dome_brute_v1", dict(V1, walk=3, pairing=1, dynamic_adjustment=1), 389, 47),
]


def pass_params(case, kw):
    pts, R = cloud_of(case)
    return pts, dict(kw, tool_radius=R)


def restate_regions(P, selected, r):
    """(labels int32[n], rows, stats, near): P = the resident float32 coordinates [n, 3], selected = bool[n], r = link radius.
    rows = dict of arrays in ascending label; near = candidate pairs with |d2 - r2| <= 4e-7 r2"""
    P = np.ascontiguousarray(P, np.float32)
    n = len(P)
    sel = np.asarray(selected, bool) & np.isfinite(P).all(axis=1)
    idx = np.nonzero(sel)[0]
    Q = P[idx]
    m = len(idx)
    r32 = np.float32(r)
    r2 = r32 * r32
    labels = np.full(n, -1, np.int32)
    if m == 0:
        rows = dict(label=np.zeros(0, np.int32), count=np.zeros(0, np.uint32), mn=np.zeros((0, 3), np.float32),
                    mx=np.zeros((0, 3), np.float32), centroid=np.zeros((0, 3)))
        return labels, rows, dict(n=n, selected=0, regions=0, singletons=0, largest=0), 0
    pairs = cKDTree(Q.astype(np.float64)).query_pairs(float(r) * 1.001, output_type="ndarray")
    d = Q[pairs[:, 0]] - Q[pairs[:, 1]]
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]        # flann_dist2's order, float32
    assert d2.dtype == np.float32
    near = int((np.abs(d2.astype(np.float64) - float(r2)) <= 4e-7 * float(r2)).sum())
    keep = d2 <= r2
    g = coo_matrix((np.ones(int(keep.sum()), np.int8), (pairs[keep, 0], pairs[keep, 1])), shape=(m, m))
    ncomp, comp = connected_components(g, directed=False)
    lab = np.full(ncomp, np.iinfo(np.int64).max, np.int64)
    np.minimum.at(lab, comp, idx)
    labels[idx] = lab[comp]
    order = np.argsort(lab)
    count = np.bincount(comp, minlength=ncomp)
    mn = np.full((ncomp, 3), np.inf, np.float32)
    mx = np.full((ncomp, 3), -np.inf, np.float32)
    np.minimum.at(mn, comp, Q)
    np.maximum.at(mx, comp, Q)
    fixed = np.rint(Q.astype(np.float64) * FIXED).astype(np.int64)
    sums = np.zeros((ncomp, 3), np.int64)
    np.add.at(sums, comp, fixed)
    centroid = sums.astype(np.float64) / count[:, None].astype(np.float64) / FIXED
    rows = dict(label=lab[order].astype(np.int32), count=count[order].astype(np.uint32), mn=mn[order], mx=mx[order],
                centroid=centroid[order])
    stats = dict(n=n, selected=m, regions=ncomp, singletons=int((count == 1).sum()), largest=int(count.max()))
    return labels, rows, stats, near


def assert_same(got, want, what=""):
    """Engine.regions()'s triple against restate_regions()'s: exact"""
    labels, rows, st = got
    wl, wr, wst = want[:3]
    assert st == wst, (what, st, wst)
    assert labels.dtype == np.int32 and np.array_equal(labels, wl), (what, int((labels != wl).sum()))
    assert len(rows) == len(wr["label"]), what
    assert np.array_equal(rows["label"], wr["label"]) and np.array_equal(rows["count"], wr["count"]), what
    assert np.array_equal(bits(rows["mn"]), bits(wr["mn"])) and np.array_equal(bits(rows["mx"]), bits(wr["mx"])), what
    assert np.array_equal(rows["centroid"], wr["centroid"]), what


def assert_equal_results(a, b, what=""):
    """two Engine.regions() triples: identical bytes"""
    assert a[2] == b[2], (what, a[2], b[2])
    assert np.array_equal(a[0], b[0]), what
    assert a[1].tobytes() == b[1].tobytes(), what


# ---------------------------------------------------------------- CPU


def test_header_declares_and_engine_exports_regions(engine_mod):
    hdr = open(os.path.join(ROOT, "include", "ppp_hip.h")).read()
    assert ("int ppp_get_regions(ppp_handle h, int source, const unsigned char *mask, float threshold, float link_radius,\n"
            "                    int *labels, size_t cap, ppp_region *regions, size_t region_cap, ppp_region_stats *stats);") in hdr
    assert "typedef struct { size_t n, selected, regions, singletons, largest; } ppp_region_stats;" in hdr
    for name in ("PPP_REGIONS_UNCOVERED = 0", "PPP_REGIONS_OVERLAP   = 1", "PPP_REGIONS_NARROW    = 2", "PPP_REGIONS_MASK      = 3",
                 "} ppp_region;"):
        assert name in hdr, name
    assert "ppp_get_regions" in engine_mod.EXPORTS
    assert hasattr(engine_mod.Engine, "regions")
    assert (engine_mod.REGIONS_UNCOVERED, engine_mod.REGIONS_OVERLAP, engine_mod.REGIONS_NARROW, engine_mod.REGIONS_MASK) == (0, 1, 2, 3)
    for h in ("Path_Generate.h", "Path_Generate_Algorithm.h", "robot_path.h"):
        assert "void get_gaps()" in open(os.path.join(ROOT, "include", h)).read(), h
    planner = open(os.path.join(ROOT, "include", "ppp_planner.hpp")).read()
    assert "bool regions(ppp_region_stats &st, std::vector<ppp_region> *rows = nullptr" in planner
    assert "void print_gaps()" in planner and "PPP_GAPS_MIN" in planner


def test_header_is_c99_clean_with_regions(tmp_path):
    src = tmp_path / "c99.c"
    src.write_text('#include "ppp_hip.h"\nint main(void) {\n'
                   '    int (*f)(ppp_handle, int, const unsigned char *, float, float, int *, size_t, ppp_region *, size_t,\n'
                   '             ppp_region_stats *) = ppp_get_regions;\n'
                   '    ppp_region r; ppp_region_stats st;\n'
                   '    r.label = PPP_REGIONS_MASK; r.count = 0u; r.mn[2] = 0.f; r.mx[2] = 0.f; r.centroid[2] = 0.0; st.largest = 0;\n'
                   '    return f == 0 || r.label != 3 || st.largest != 0;\n}\n')
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                           str(src)])


def test_region_structs_layout_matches_the_header(engine_mod, tmp_path):
    """the ctypes mirrors and the numpy row type have the C structs' sizes and offsets"""
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ppp_hip.h"\nint main(void) {\n'
                   '    printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(ppp_region), offsetof(ppp_region, label), offsetof(ppp_region, count),\n'
                   '           offsetof(ppp_region, mn), offsetof(ppp_region, mx), offsetof(ppp_region, centroid));\n'
                   '    printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(ppp_region_stats), offsetof(ppp_region_stats, n),\n'
                   '           offsetof(ppp_region_stats, selected), offsetof(ppp_region_stats, regions),\n'
                   '           offsetof(ppp_region_stats, singletons), offsetof(ppp_region_stats, largest));\n    return 0;\n}\n')
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)])
    got = [int(v) for v in subprocess.check_output([exe]).split()]
    R, S, D = engine_mod.Region, engine_mod.RegionStats, engine_mod.REGION_DTYPE
    assert got[:6] == [ctypes.sizeof(R), R.label.offset, R.count.offset, R.mn.offset, R.mx.offset, R.centroid.offset]
    assert got[:6] == [D.itemsize] + [D.fields[k][1] for k in ("label", "count", "mn", "mx", "centroid")]
    assert got[6:] == [ctypes.sizeof(S), S.n.offset, S.selected.offset, S.regions.offset, S.singletons.offset, S.largest.offset]


def test_examples_build_with_the_gaps_switch(engine_mod):
    for ex in ("connect.cpp", "robot.cpp"):
        src = open(os.path.join(ROOT, "examples", ex)).read()
        assert 'getenv("PPP_GAPS")' in src and "get_gaps()" in src, ex
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "examples"), "connect", "connect1", "robot", "main"])
    for exe in ("connect", "connect1", "robot", "main"):
        assert os.access(os.path.join(ROOT, "examples", exe), os.X_OK)


def test_restatement_on_the_oracles_uncovered_points_of_small_40k(oracle_mod):
    """small_40k, walk 0: the points the oracle's path coverage leaves out fall into more than one region, none of them the
    whole set: 858 points in 47 regions at link 2.5 mm, the two end strips of 400 points the largest"""
    case, kw, uncovered, regions = PASSES[0]
    pts, kw = pass_params(case, kw)
    flags, _ = restate_path_coverage(pts, kw, oracle_mod)
    o = oracle_mod.Oracle(pts, **kw)
    P = o.points()
    o.close()
    labels, rows, st, near = restate_regions(P, flags == 0, 2.5)
    print("small_40k walk 0: %d uncovered in %d regions, largest %d, singletons %d, near-threshold pairs %d"
          % (st["selected"], st["regions"], st["largest"], st["singletons"], near))
    assert st["regions"] > 1 and st["largest"] < st["selected"]
    assert (st["selected"], st["regions"]) == (uncovered, regions)
    assert sorted(rows["count"])[-2:] == [400, 400] and st["singletons"] == 34
    assert int(rows["count"].sum()) == st["selected"] and np.array_equal(np.unique(labels[labels >= 0]), rows["label"])
    assert (labels[rows["label"]] == rows["label"]).all()      # a region is named after its smallest cloud index


# ---------------------------------------------------------------- GPU


def mask_regions(e, P, mask, link, what):
    got = e.regions(MASK, mask=mask, link_radius=link)
    want = restate_regions(P, mask != 0, link)
    print("%s link %g: %d selected, %d regions, largest %d, singletons %d; near-threshold pairs %d"
          % (what, link, want[2]["selected"], want[2]["regions"], want[2]["largest"], want[2]["singletons"], want[3]))
    assert_same(got, want, what)
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["tiny_5k", "small_40k"])
def test_mask_regions_match_scipy(engine_mod, case):
    """seeded Bernoulli masks (30 %, 3 %) at link 1.5, 2.5, 4.0"""
    pts, cfg = synth.make_config(case)
    e = engine_mod.Engine(0, tool_radius=cfg["tool_radius"])
    e.set_cloud(pts)
    P = e.cloud()
    rng = np.random.default_rng(len(pts))
    for share in (0.30, 0.03):
        mask = (rng.random(len(pts)) < share).astype(np.uint8)
        for link in (1.5, 2.5, 4.0):
            mask_regions(e, P, mask, link, "%s %g" % (case, share))
    # link_radius <= 0: the handle's normal_radius (2.5)
    assert_equal_results(e.regions(engine_mod.REGIONS_MASK, mask=mask), e.regions(engine_mod.REGIONS_MASK, mask=mask, link_radius=2.5))
    e.close()


@pytest.mark.gpu
def test_union_find_adversaries_on_small_40k(engine_mod):
    """a strip across every slab, the full mask at link 4, the empty mask, NaN points and exact duplicates, every second point"""
    pts, cfg = synth.make_config("small_40k")
    R = cfg["tool_radius"]
    e = engine_mod.Engine(0, tool_radius=R)
    e.set_cloud(pts)
    P = e.cloud()
    n = len(pts)
    ymid = 0.5 * (float(P[:, 1].min()) + float(P[:, 1].max()))
    strip = (np.abs(P[:, 1] - np.float32(ymid)) < 1.5).astype(np.uint8)
    got = mask_regions(e, P, strip, 2.5, "strip")
    assert got[2]["selected"] > 0
    full = np.ones(n, np.uint8)
    got = mask_regions(e, P, full, 4.0, "full")
    assert got[2]["selected"] == n
    labels, rows, st = e.regions(engine_mod.REGIONS_MASK, mask=np.zeros(n, np.uint8))
    assert st == dict(n=n, selected=0, regions=0, singletons=0, largest=0) and len(rows) == 0 and (labels == -1).all()
    mask_regions(e, P, (np.arange(n) % 2 == 0).astype(np.uint8), 2.5, "every second point")
    e.close()
    rng = np.random.default_rng(50)
    bad = pts.copy()
    pick = rng.choice(n, 150, replace=False)
    bad[pick[:50], rng.integers(0, 3, 50)] = np.nan
    bad[pick[50:100]] = bad[pick[100:150]]                   # 50 exact duplicates of other points
    d = engine_mod.Engine(0, tool_radius=R)
    d.set_cloud(bad)
    Pd = d.cloud()
    got = mask_regions(d, Pd, full, 2.5, "NaNs and duplicates")
    assert got[2]["selected"] == n - 50 and (got[0][pick[:50]] == -1).all()
    assert np.array_equal(got[0][pick[50:100]], got[0][pick[100:150]])     # distance 0: linked
    d.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case,kw,uncovered,regions", PASSES)
def test_uncovered_regions_of_the_passes(engine_mod, oracle_mod, case, kw, uncovered, regions):
    """UNCOVERED equals MASK of path_coverage()[0] == 0 from the same handle and scipy on the oracle restatement's flags"""
    pts, kw = pass_params(case, kw)
    want_flags, S = restate_path_coverage(pts, kw, oracle_mod)
    e = engine_mod.Engine(0, **kw)
    e.set_cloud(pts)
    assert e.gen_path() == S
    got = e.regions(engine_mod.REGIONS_UNCOVERED, link_radius=2.5)
    flags, _ = e.path_coverage()
    assert_equal_results(got, e.regions(engine_mod.REGIONS_MASK, mask=(flags == 0).astype(np.uint8), link_radius=2.5), case)
    want = restate_regions(e.cloud(), want_flags == 0, 2.5)
    print("%s %s: oracle: %d uncovered in %d regions (first counted: %d in %d), largest %d, singletons %d; near-threshold pairs %d"
          % (case, kw, want[2]["selected"], want[2]["regions"], uncovered, regions, want[2]["largest"], want[2]["singletons"], want[3]))
    assert_same(got, want, case)
    assert got[0].shape == (len(pts),)
    e.close()


@pytest.mark.gpu
def test_overlap_and_narrow_regions_equal_their_masks(engine_mod):
    pts, cfg = synth.make_config("small_40k")
    R = cfg["tool_radius"]
    e = engine_mod.Engine(0, tool_radius=R, walk=1, dynamic_adjustment=1)
    e.set_cloud(pts)
    e.gen_path()
    got = e.regions(engine_mod.REGIONS_OVERLAP)
    _, first, last, _ = e.path_contacts()
    assert got[2]["selected"] == int((last > first).sum()) > 0
    assert_equal_results(got, e.regions(engine_mod.REGIONS_MASK, mask=(last > first).astype(np.uint8)), "overlap")
    assert_same(got, restate_regions(e.cloud(), last > first, 2.5), "overlap")
    e.close()
    f = engine_mod.Engine(0, tool_radius=R, depth=RELEASED_DEPTH)
    f.set_cloud(pts)
    got = f.regions(engine_mod.REGIONS_NARROW, threshold=10.8)              # needs no pass
    _, hw, _ = f.contact_field()
    with np.errstate(invalid="ignore"):
        narrow = np.isfinite(hw) & (np.float32(2) * np.abs(hw) < np.float32(10.8))
    assert got[2]["selected"] == int(narrow.sum()) > 0
    assert f.contact_field(maps=False, min_width=10.8)[2]["narrow"] == got[2]["selected"]
    assert_equal_results(got, f.regions(engine_mod.REGIONS_MASK, mask=narrow.astype(np.uint8)), "narrow")
    assert_same(got, restate_regions(f.cloud(), narrow, 2.5), "narrow")
    f.close()


@pytest.mark.gpu
def test_regions_at_cfg2_match_scipy_and_are_deterministic(engine_mod):
    """1 M points: UNCOVERED with the default depth and with depth = 1e-7, and a 30 % Bernoulli MASK, each equal to scipy on the
    engine's own mask; two fresh handles give identical bytes"""
    pts, cfg = synth.make_config("cfg2_1m_s256")
    R = cfg["tool_radius"]
    mask = (np.random.default_rng(2).random(len(pts)) < 0.30).astype(np.uint8)
    results = []
    for fresh in range(2):
        out = []
        for depth in (None, RELEASED_DEPTH):
            kw = dict(tool_radius=R, walk=1) if depth is None else dict(tool_radius=R, walk=1, depth=depth)
            e = engine_mod.Engine(0, **kw)
            e.set_cloud(pts)
            e.gen_path()
            got = e.regions(engine_mod.REGIONS_UNCOVERED)
            out.append(got)
            if fresh == 0:
                flags, _ = e.path_coverage()
                want = restate_regions(e.cloud(), flags == 0, 2.5)
                print("cfg2 depth %s: %d uncovered in %d regions, largest %d, singletons %d; near-threshold pairs %d"
                      % (depth, want[2]["selected"], want[2]["regions"], want[2]["largest"], want[2]["singletons"], want[3]))
                assert_same(got, want, "cfg2 uncovered depth %s" % depth)
            if depth is None:
                got = e.regions(engine_mod.REGIONS_MASK, mask=mask)
                out.append(got)
                if fresh == 0:
                    want = restate_regions(e.cloud(), mask != 0, 2.5)
                    print("cfg2 mask 30 %%: %d selected in %d regions, largest %d, singletons %d; near-threshold pairs %d"
                          % (want[2]["selected"], want[2]["regions"], want[2]["largest"], want[2]["singletons"], want[3]))
                    assert_same(got, want, "cfg2 mask")
            e.close()
        results.append(out)
    for a, b in zip(*results):
        assert_equal_results(a, b, "fresh handles")


@pytest.mark.gpu
def test_regions_call_order_and_reuse(engine_mod):
    """a repeated call launches nothing; the handle stays on the window path and plans the same bytes afterwards; the three
    contact results are the same before and after; a new pass makes UNCOVERED recompute and does not make NARROW recompute"""
    new = ("k_reg_select", "k_reg_link", "k_reg_flatten", "k_reg_labels")
    older = ("k_pcov_balls", "k_pcon_points", "k_field_batch")
    E = engine_mod
    pts, cfg = synth.make_config("small_40k")
    kw = dict(tool_radius=cfg["tool_radius"], walk=1)
    e = E.Engine(0, **kw)
    ref = E.Engine(0, **kw)
    for h in (e, ref):
        h.set_cloud(pts)
    with pytest.raises(E.PPPError) as ex:                     # no pass yet
        e.regions(E.REGIONS_UNCOVERED)
    assert ex.value.code == E.ERR_ARG
    n0 = e.regions(E.REGIONS_NARROW, threshold=11.9)         # before any pass
    for h in (e, ref):
        h.gen_path(); h.get_path()
    assert e.fast_path()
    pc_before = e.path_coverage()
    con_before = e.path_contacts()
    cf_before = e.contact_field()
    e.enable_timing(True)
    e.kernel_times()
    u1 = e.regions(E.REGIONS_UNCOVERED)                       # (Engine.regions asks twice: the sizes, then the maps)
    _, launches = e.kernel_times(with_launches=True)
    assert u1[2]["selected"] > 0 and all(launches.get(k) == 1 for k in new), launches
    assert not any(launches.get(k) for k in older), launches
    u2 = e.regions(E.REGIONS_UNCOVERED)
    _, launches = e.kernel_times(with_launches=True)
    assert not any(launches.get(k) for k in new + older + ("k_compact_count",)), launches
    assert_equal_results(u1, u2)
    assert e.regions(E.REGIONS_UNCOVERED, labels=False)[0] is None
    o1 = e.regions(E.REGIONS_OVERLAP)
    n1 = e.regions(E.REGIONS_NARROW, threshold=11.9)
    _, launches = e.kernel_times(with_launches=True)
    assert not any(launches.get(k) for k in older), launches  # the sources' results were there
    assert_equal_results(n0, n1)
    assert e.fast_path()
    pc_after, con_after, cf_after = e.path_coverage(), e.path_contacts(), e.contact_field()
    assert pc_before[1] == pc_after[1] and np.array_equal(pc_before[0], pc_after[0])
    assert all(np.array_equal(a, b) for a, b in zip(con_before[:3], con_after[:3])) and con_before[3]["total"] == con_after[3]["total"]
    assert bits(cf_before[0]).tobytes() == bits(cf_after[0]).tobytes() and bits(cf_before[1]).tobytes() == bits(cf_after[1]).tobytes()
    _, launches = e.kernel_times(with_launches=True)
    assert not any(launches.get(k) for k in new + older), launches
    for h in (e, ref):                                        # a new pass
        h.gen_path(); h.get_path()
    assert e.fast_path()
    assert e.waypoints().tobytes() == ref.waypoints().tobytes()
    e.kernel_times()
    n2 = e.regions(E.REGIONS_NARROW, threshold=11.9)         # the field did not change: answered from the result
    _, launches = e.kernel_times(with_launches=True)
    assert not any(launches.get(k) for k in new + older), launches
    assert_equal_results(n1, n2)
    u3 = e.regions(E.REGIONS_UNCOVERED)                       # the pass is new: its coverage and its regions are computed
    _, launches = e.kernel_times(with_launches=True)
    assert launches.get("k_pcov_balls") == 1 and all(launches.get(k) == 1 for k in new), launches
    assert_equal_results(u1, u3)                              # (the same cloud and parameters: the same pass)
    assert o1[2]["n"] == len(pts)
    e.close(); ref.close()


@pytest.mark.gpu
def test_regions_refusals_and_the_size_protocol(engine_mod):
    E = engine_mod
    pts, cfg = synth.make_config("small_40k")
    R = cfg["tool_radius"]
    n = len(pts)
    full = np.ones(n, np.uint8)

    def code_of(h, *a, **k):
        with pytest.raises(E.PPPError) as ex:
            h.regions(*a, **k)
        return ex.value.code

    e = E.Engine(0, tool_radius=R)
    assert code_of(e, E.REGIONS_MASK, mask=full) == E.ERR_ARG                     # no cloud
    e.set_cloud(pts)
    assert code_of(e, E.REGIONS_UNCOVERED) == E.ERR_ARG                             # no pass
    assert code_of(e, E.REGIONS_OVERLAP) == E.ERR_ARG
    assert code_of(e, 4, mask=full) == E.ERR_ARG and code_of(e, -1, mask=full) == E.ERR_ARG
    assert code_of(e, E.REGIONS_MASK) == E.ERR_ARG                                  # no mask
    for thr in (0.0, -1.0, float("nan"), float("inf")):
        assert code_of(e, E.REGIONS_NARROW, threshold=thr) == E.ERR_ARG
    for link in (float("nan"), float("inf"), float("-inf")):
        assert code_of(e, E.REGIONS_MASK, mask=full, link_radius=link) == E.ERR_ARG
    e.set_params(curvature_k=2)
    assert code_of(e, E.REGIONS_NARROW, threshold=10.0) == E.ERR_ARG
    e.set_params(curvature_k=50)
    # the two-call protocol on the C call itself
    mask = (np.random.default_rng(1).random(n) < 0.3).astype(np.uint8)
    labels, rows, st = e.regions(E.REGIONS_MASK, mask=mask)
    assert st["regions"] > 8
    L = E.lib()
    mp = mask.ctypes.data_as(ctypes.POINTER(ctypes.c_ubyte))
    st2 = E.RegionStats()
    assert L.ppp_get_regions(e.h, E.REGIONS_MASK, mp, 0.0, 0.0, None, 0, None, 0, ctypes.byref(st2)) == 0
    assert (st2.n, st2.selected, st2.regions, st2.singletons, st2.largest) == tuple(st[k] for k in ("n", "selected", "regions", "singletons", "largest"))
    lab5 = np.full(8, -7, np.int32)
    row5 = np.zeros(8, E.REGION_DTYPE)
    assert L.ppp_get_regions(e.h, E.REGIONS_MASK, mp, 0.0, 0.0, lab5.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), 5,
                             row5.ctypes.data_as(ctypes.POINTER(E.Region)), 5, None) == 0
    assert np.array_equal(lab5[:5], labels[:5]) and (lab5[5:] == -7).all()
    assert row5[:5].tobytes() == rows[:5].tobytes() and row5[5:].tobytes() == np.zeros(3, E.REGION_DTYPE).tobytes()
    assert e.gen_path() > 0 and e.regions(E.REGIONS_UNCOVERED)[2]["n"] == n        # the handle stays usable
    r = E.Engine(0, tool_radius=R, slice_begin=2, slice_end=9)
    r.set_cloud(pts)
    assert code_of(r, E.REGIONS_MASK, mask=full) == E.ERR_UNSUPPORTED
    assert code_of(r, E.REGIONS_NARROW, threshold=10.0) == E.ERR_UNSUPPORTED
    assert r.gen_path() > 0
    assert code_of(r, E.REGIONS_UNCOVERED) == E.ERR_UNSUPPORTED
    scaled = (pts * np.float32(1000)).astype(np.float32)
    mn, mx = scaled.min(axis=0), scaled.max(axis=0)
    g = E.Engine(0, tool_radius=R, slice_begin=2, slice_end=9)
    lo, hi, _ = g.range_interval(mn[0], mx[0])
    keep = np.nonzero((scaled[:, 0] >= lo) & (scaled[:, 0] <= hi))[0]
    g.set_cloud_part(pts[keep], keep, mn, mx, n, lo, hi)
    assert code_of(g, E.REGIONS_MASK, mask=np.ones(len(keep), np.uint8)) == E.ERR_UNSUPPORTED
    assert g.gen_path() > 0
    assert code_of(g, E.REGIONS_UNCOVERED) == E.ERR_UNSUPPORTED
    e.close(); r.close(); g.close()


@pytest.mark.gpu
def test_connect_prints_the_gaps(engine_mod, tmp_path):
    """PPP_GAPS=1 ./connect prints the gap lines with Engine.regions()'s numbers; without it the output is what it was"""
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "examples"), "connect"])
    pts, _ = synth.make_config("small_40k")
    pcd = str(tmp_path / "workpiece.pcd")
    engine_mod.save_pcd(pcd, pts)
    conf = tmp_path / "config.txt"
    conf.write_text("Tool_Radius = 6\npathFile = %s\nPathResolution = 7\nRPYresolution = 7\nEnd effector length = 0.3\n"
                    "Smooth = false\nAlignment = false\nChangeRange = true\nRemoveOutlier = false\nDynamic_adjustment = false\n"
                    "Adjust_Threshold = 1\ntoolthickness = 10\ndepth = 0.01\n" % str(tmp_path / "wp.txt"))
    exe = os.path.join(ROOT, "examples", "connect")
    heads = ("gaps: ", "gap ")

    def run(**extra):
        env = {k: v for k, v in os.environ.items() if k not in ("PPP_GAPS", "PPP_GAPS_MIN", "PPP_SHOW_PCD")}
        env.update(PPP_CONFIG=str(conf), **extra)
        r = subprocess.run([exe, pcd], env=env, capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
        assert r.returncode == 0, r.stderr
        return r.stdout

    plain, with_g = run(), run(PPP_GAPS="1")
    lines = [ln for ln in with_g.splitlines() if ln.startswith(heads)]
    assert not any(ln.startswith(heads) for ln in plain.splitlines())
    strip = lambda out: [ln for ln in out.splitlines() if not ln.startswith("Toal Using Time") and ln not in lines]
    assert strip(plain) == strip(with_g)
    e = engine_mod.Engine(0, tool_radius=6.0, walk=1, dynamic_adjustment=0)
    e.set_cloud(engine_mod.load_pcd(pcd)[0])
    e.gen_path()
    _, rows, st = e.regions(engine_mod.REGIONS_UNCOVERED)
    e.close()
    big = sorted((r for r in rows if r["count"] >= 10), key=lambda r: (-int(r["count"]), int(r["label"])))
    want = ["gaps: %d of %d points uncovered in %d regions (link %g mm)" % (st["selected"], st["n"], st["regions"], 2.5)]
    want += ["gap %d: %d points, x [%f, %f] y [%f, %f], centre (%f, %f, %f)"
             % (r["label"], r["count"], r["mn"][0], r["mx"][0], r["mn"][1], r["mx"][1], r["centroid"][0], r["centroid"][1], r["centroid"][2])
             for r in big]
    want += ["gaps: %d regions below %d points" % (len(rows) - len(big), 10)]
    assert st["regions"] > 0 and len(big) > 0
    assert lines == want
    few = [ln for ln in run(PPP_GAPS="1", PPP_GAPS_MIN="300").splitlines() if ln.startswith(heads)]
    assert few[0] == want[0] and len(few) == 2 + int((rows["count"] >= 300).sum()) and few[-1].endswith("below 300 points")
