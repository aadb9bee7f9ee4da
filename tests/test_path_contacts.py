"""Path contacts (ppp_get_path_contacts): how many of path coverage's contact balls hold each
cloud point, and the first and last slice that has one of them.

The balls are those of ppp_get_path_coverage (tests/test_path_coverage.py): for every slice of the pass, every
compute_boundary sample of its final spline holds the cloud points within half the x-extent of its contact ellipse.  The
restatement below rebuilds the three maps from ONE oracle of the same walk and parameters, through its public methods only
(nodes, eval_spline, area2cloud, radius_search)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from polishpathplanning_amd import synth
from test_path_coverage import CASES, boundary_samples, case_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BINS = 64


def restate_path_contacts(pts, kw, oracle_mod):
    """(counts uint32[n], first int32[n], last int32[n], S): every ball of every slice's final spline adds one to the count of
    each point inside it; first / last are the smallest / largest slice with such a ball, -1 where there is none"""
    R = kw["tool_radius"]
    o = oracle_mod.Oracle(pts, **kw)
    S = o.gen_path()
    n = len(pts)
    counts = np.zeros(n, np.int64)
    first = np.full(n, np.iinfo(np.int32).max, np.int64)
    last = np.full(n, -1, np.int64)
    for s in range(S):
        y, _, _ = o.nodes(s)
        if len(y) < 3:
            continue
        dys = boundary_samples(y, R)
        if not dys:
            continue                              # B.15: a loop that runs zero times adds no ball
        rc, P = o.eval_spline(s, dys)
        assert rc == 0
        for p in P:
            lo, hi = o.area2cloud(p, 0), o.area2cloud(p, 1)
            r = (np.float32(lo[0]) - np.float32(hi[0])) / np.float32(2)
            if np.isnan(r):
                continue                          # B.16
            idx = np.asarray(o.radius_search(p.astype(np.float32), float(r)), np.int64)
            np.add.at(counts, idx, 1)
            first[idx] = np.minimum(first[idx], s)
            last[idx] = np.maximum(last[idx], s)
    o.close()
    first[counts == 0] = -1
    return counts.astype(np.uint32), first.astype(np.int32), last.astype(np.int32), S


def check_stats(counts, first, last, st):
    """the statistics are those of the maps"""
    assert st["n"] == len(counts)
    assert st["covered"] == int((counts > 0).sum())
    assert st["total"] == int(counts.astype(np.int64).sum())
    assert st["max_count"] == (int(counts.max()) if len(counts) else 0)
    assert st["multi_slice"] == int((last > first).sum())
    hist = np.bincount(np.minimum(counts, BINS - 1).astype(np.int64), minlength=BINS)
    assert st["hist"].shape == (BINS,) and int(st["hist"].sum()) == len(counts)
    assert np.array_equal(st["hist"], hist)


def contact_rgb(c, mx):
    """show()'s ramp under PPP_SHOW_CONTACTS (ppp::Planner::contact_rgb), packed 0xRRGGBB; count 0 yellow"""
    if c == 0 or mx == 0:
        return 0xFFFF00
    t = min(1.0, float(c) / float(mx))
    if t < 1.0 / 3:
        r, g, b = 0.0, 3 * t, 1.0
    elif t < 2.0 / 3:
        r, g, b = 0.0, 1.0, 1 - 3 * (t - 1.0 / 3)
    else:
        r, g, b = 3 * (t - 2.0 / 3), 1 - 3 * (t - 2.0 / 3), 0.0
    q = [int(np.floor(255 * v + 0.5)) for v in (r, g, b)]
    return (q[0] << 16) | (q[1] << 8) | q[2]


def test_header_declares_and_engine_exports_path_contacts(engine_mod):
    hdr = open(os.path.join(ROOT, "include", "ppp_hip.h")).read()
    assert "#define PPP_CONTACT_BINS 64" in hdr and "} ppp_contact_stats;" in hdr
    assert ("int ppp_get_path_contacts(ppp_handle h, unsigned int *counts, int *first_slice, int *last_slice, size_t cap,\n"
            "                          ppp_contact_stats *stats);") in hdr
    assert "ppp_get_path_contacts" in engine_mod.EXPORTS
    assert hasattr(engine_mod.Engine, "path_contacts")
    for h in ("Path_Generate.h", "Path_Generate_Algorithm.h", "robot_path.h"):
        assert "void get_path_contacts()" in open(os.path.join(ROOT, "include", h)).read(), h
    planner = open(os.path.join(ROOT, "include", "ppp_planner.hpp")).read()
    assert "bool path_contacts(ppp_contact_stats &st, std::vector<unsigned> *counts = nullptr" in planner
    assert "void print_path_contacts()" in planner


def test_header_is_c99_clean_with_path_contacts(tmp_path):
    src = tmp_path / "c99.c"
    src.write_text('#include "ppp_hip.h"\nint main(void) {\n'
                   '    int (*f)(ppp_handle, unsigned int *, int *, int *, size_t, ppp_contact_stats *) = ppp_get_path_contacts;\n'
                   '    ppp_contact_stats st;\n    st.hist[PPP_CONTACT_BINS - 1] = 0; st.max_count = 0u; st.total = 0ull;\n'
                   '    return f == 0 || st.hist[63] != 0;\n}\n')
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                           str(src)])


def test_contact_stats_layout_matches_the_header(engine_mod, tmp_path):
    """the ctypes mirror of ppp_contact_stats has the C struct's size and offsets"""
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ppp_hip.h"\nint main(void) {\n'
                   '    printf("%zu %zu %zu %zu\\n", sizeof(ppp_contact_stats), offsetof(ppp_contact_stats, max_count),\n'
                   '           offsetof(ppp_contact_stats, total), offsetof(ppp_contact_stats, hist));\n    return 0;\n}\n')
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)])
    got = [int(v) for v in subprocess.check_output([exe]).split()]
    S = engine_mod.ContactStats
    assert got == [ctypes.sizeof(S), S.max_count.offset, S.total.offset, S.hist.offset]
    assert engine_mod.CONTACT_BINS == BINS


def test_examples_build_with_the_path_contacts_switch(engine_mod):
    for ex in ("connect.cpp", "robot.cpp"):
        src = open(os.path.join(ROOT, "examples", ex)).read()
        assert 'getenv("PPP_PATH_CONTACTS")' in src and "get_path_contacts()" in src, ex
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "examples"), "connect", "connect1", "robot", "main"])
    for exe in ("connect", "connect1", "robot", "main"):
        assert os.access(os.path.join(ROOT, "examples", exe), os.X_OK)


def test_restatement_counts_repeated_contacts_and_slice_overlap(oracle_mod):
    """the restatement on CPU, small_40k walk 1: points held by two or more balls, and points that two slices touch -- a
    definition that counted flags, or one slice per point, would give neither"""
    pts, kw = case_params("small_40k", 1, 0, 0, {})
    counts, first, last, S = restate_path_contacts(pts, kw, oracle_mod)
    assert S > 2
    assert int(counts.max()) >= 2
    assert int((last > first).sum()) > 0
    assert np.array_equal(counts > 0, first >= 0) and np.array_equal(first >= 0, last >= 0)
    assert np.all(last >= first)


@pytest.mark.gpu
@pytest.mark.parametrize("case,walk,pairing,dynamic,extra", CASES)
def test_path_contacts_match_the_restatement(engine_mod, oracle_mod, case, walk, pairing, dynamic, extra):
    """Engine.path_contacts(): every count, first and last slice as the restatement has them, for every walk; counts > 0 is
    path_coverage()'s flags; the statistics are the maps'"""
    pts, kw = case_params(case, walk, pairing, dynamic, extra)
    want_c, want_f, want_l, S = restate_path_contacts(pts, kw, oracle_mod)
    e = engine_mod.Engine(0, **kw)
    e.set_cloud(pts)
    assert e.gen_path() == S
    counts, first, last, st = e.path_contacts()
    assert counts.dtype == np.uint32 and first.dtype == np.int32 and last.dtype == np.int32
    assert counts.shape == first.shape == last.shape == (len(pts),)
    assert np.array_equal(counts, want_c), (int(counts.sum()), int(want_c.sum()), int((counts != want_c).sum()))
    assert np.array_equal(first, want_f), int((first != want_f).sum())
    assert np.array_equal(last, want_l), int((last != want_l).sum())
    check_stats(counts, first, last, st)
    flags, covered = e.path_coverage()
    assert np.array_equal(counts > 0, flags.astype(bool))
    assert st["covered"] == covered
    n0, n1, n2, st2 = e.path_contacts(maps=False)
    assert n0 is None and n1 is None and n2 is None
    assert {k: v for k, v in st2.items() if k != "hist"} == {k: v for k, v in st.items() if k != "hist"}
    assert np.array_equal(st2["hist"], st["hist"])
    e.close()


@pytest.mark.gpu
def test_window_path_and_slab_path_give_the_same_contacts(engine_mod):
    pts, cfg = synth.make_config("small_40k")
    kw = dict(tool_radius=cfg["tool_radius"], walk=1)
    a = engine_mod.Engine(0, **kw)
    b = engine_mod.Engine(0, fast_path=False, **kw)
    for e in (a, b):
        e.set_cloud(pts)
        e.gen_path(); e.get_path()
    assert a.fast_path() and not b.fast_path()
    ca, fa, la, sa = a.path_contacts()
    cb, fb, lb, sb = b.path_contacts()
    assert np.array_equal(ca, cb) and np.array_equal(fa, fb) and np.array_equal(la, lb)
    assert sa["total"] == sb["total"] and np.array_equal(sa["hist"], sb["hist"])
    assert sa["max_count"] >= 2 and sa["multi_slice"] > 0
    a.close(); b.close()


@pytest.mark.gpu
def test_path_contacts_are_computed_once_per_pass_and_leave_the_window_path_alone(engine_mod):
    """each new kernel launches once per pass, path coverage's and coverage's kernels not at all; a pass after the call gives
    the bytes of a handle that never asked, still on the window path, also when replayed from its capture"""
    new = ("k_pcon_offsets", "k_pcon_samples", "k_pcon_points", "k_pcon_stats")
    old = ("k_pcov_balls", "k_cov_balls", "k_cov_count")
    pts, cfg = synth.make_config("small_40k")
    kw = dict(tool_radius=cfg["tool_radius"], walk=1)
    e = engine_mod.Engine(0, **kw)
    ref = engine_mod.Engine(0, **kw)
    for h in (e, ref):
        h.set_cloud(pts)
        h.gen_path(); h.get_path()
    assert e.fast_path()
    e.enable_timing(True)
    e.kernel_times()
    c1, f1, l1, s1 = e.path_contacts()
    _, launches = e.kernel_times(with_launches=True)
    assert all(launches.get(k) == 1 for k in new), launches
    assert not any(launches.get(k) for k in old), launches
    c2, f2, l2, s2 = e.path_contacts()
    _, launches = e.kernel_times(with_launches=True)
    assert not any(launches.get(k) for k in new + old), launches
    assert np.array_equal(c1, c2) and np.array_equal(f1, f2) and np.array_equal(l1, l2) and s1["total"] == s2["total"]
    for h in (e, ref):
        h.gen_path(); h.get_path()
    assert e.fast_path()
    assert e.waypoints().tobytes() == ref.waypoints().tobytes()
    c3, f3, l3, _ = e.path_contacts()
    _, launches = e.kernel_times(with_launches=True)
    assert all(launches.get(k) == 1 for k in new), launches
    assert np.array_equal(c3, c1) and np.array_equal(f3, f1) and np.array_equal(l3, l1)
    for _ in range(3):                                   # the captured pass, replayed
        for h in (e, ref):
            h.run_async(); h.sync()
        assert e.fast_path()
        assert e.waypoints().tobytes() == ref.waypoints().tobytes()
    c4, f4, l4, _ = e.path_contacts()
    assert np.array_equal(c4, c1) and np.array_equal(f4, f1) and np.array_equal(l4, l1)
    e.close(); ref.close()


@pytest.mark.gpu
def test_ranged_handles_tile_the_whole_cloud_contacts(engine_mod):
    """4 slice ranges: the counts add up, first is the minimum and last the maximum over the ranges that touch a point; a
    range_margin too small for the balls is refused, never answered"""
    from polishpathplanning_amd.robot_path import slice_ranges
    pts, cfg = synth.make_config("cfg1_50k_s32")
    kw = dict(tool_radius=cfg["tool_radius"], walk=1)
    whole = engine_mod.Engine(0, **kw)
    whole.set_cloud(pts)
    S = whole.gen_path()
    wc, wf, wl, ws = whole.path_contacts()
    assert ws["max_count"] >= 2 and ws["multi_slice"] > 0
    n = len(pts)
    got_c = np.zeros(n, np.int64)
    got_f = np.full(n, np.iinfo(np.int32).max, np.int64)
    got_l = np.full(n, -1, np.int64)
    ranges = slice_ranges(S, 4)
    assert len(ranges) == 4
    for b, e in ranges:
        h = engine_mod.Engine(0, slice_begin=b, slice_end=e, **kw)
        h.set_cloud(pts)
        h.gen_path()
        c, f, l, st = h.path_contacts()
        assert c.shape == (n,) and 0 < st["covered"] <= ws["covered"]
        check_stats(c, f, l, st)
        touched = c > 0
        assert np.all((f[touched] >= b) & (l[touched] < e)) and np.all(f[~touched] == -1) and np.all(l[~touched] == -1)
        got_c += c
        got_f[touched] = np.minimum(got_f[touched], f[touched])
        got_l[touched] = np.maximum(got_l[touched], l[touched])
        h.close()
    got_f[got_c == 0] = -1
    assert np.array_equal(got_c, wc), int((got_c != wc).sum())
    assert np.array_equal(got_f, wf) and np.array_equal(got_l, wl)
    b, e = ranges[1]
    h = engine_mod.Engine(0, slice_begin=b, slice_end=e, range_margin=5.0, **kw)
    h.set_cloud(pts)
    h.gen_path()
    with pytest.raises(engine_mod.PPPError) as ex:
        h.path_contacts()
    assert ex.value.code == engine_mod.ERR_CAPACITY and "range_margin" in str(ex.value)
    h.close(); whole.close()


@pytest.mark.gpu
def test_batch_member_answers_as_a_lone_handle_and_refusals(engine_mod):
    kinds = [("small_40k", 1, {}), ("tiny_5k", 2, {}), ("small_40k", 3, dict(walk=2))]
    clouds = [synth.make_config(n, seed=s)[0] for n, s, _ in kinds]
    want = []
    for pts, (_, _, kw) in zip(clouds, kinds):
        e = engine_mod.Engine(0, tool_radius=6.0, **kw); e.set_cloud(pts); e.gen_path(); e.get_path()
        want.append(e.path_contacts())
        e.close()
    engines = []
    for pts, (_, _, kw) in zip(clouds, kinds):
        e = engine_mod.Engine(0, tool_radius=6.0, **kw); e.set_cloud(pts); engines.append(e)
    for _ in range(2):                                   # capture, then a replay
        engine_mod.run_batch_async(engines)
        engine_mod.sync_batch(engines)
        for e, w in zip(engines, want):
            got = e.path_contacts()
            for a, b in zip(got[:3], w[:3]):
                assert np.array_equal(a, b)
            assert got[3]["total"] == w[3]["total"] and np.array_equal(got[3]["hist"], w[3]["hist"])
    for e in engines:
        e.close()
    pts, cfg = synth.make_config("small_40k")
    R = cfg["tool_radius"]
    e = engine_mod.Engine(0, tool_radius=R)
    e.set_cloud(pts)
    with pytest.raises(engine_mod.PPPError) as ex:                   # before any pass
        e.path_contacts()
    assert ex.value.code == engine_mod.ERR_ARG
    k = engine_mod.Engine(0, tool_radius=R, curvature_k=2)
    k.set_cloud(pts)
    k.gen_path()
    with pytest.raises(engine_mod.PPPError) as ex:
        k.path_contacts()
    assert ex.value.code == engine_mod.ERR_ARG
    scaled = (pts * np.float32(1000)).astype(np.float32)             # a part handle: its maps would need the caller's index map
    mn, mx = scaled.min(axis=0), scaled.max(axis=0)
    g = engine_mod.Engine(0, tool_radius=R, slice_begin=2, slice_end=9)
    lo, hi, _ = g.range_interval(mn[0], mx[0])
    keep = np.nonzero((scaled[:, 0] >= lo) & (scaled[:, 0] <= hi))[0]
    g.set_cloud_part(pts[keep], keep, mn, mx, len(pts), lo, hi)
    g.gen_path()
    with pytest.raises(engine_mod.PPPError) as ex:
        g.path_contacts()
    assert ex.value.code == engine_mod.ERR_UNSUPPORTED
    e.close(); k.close(); g.close()


@pytest.mark.gpu
def test_path_contacts_at_cfg2_are_deterministic_and_leave_path_coverage_alone(engine_mod):
    """1 M points, 256 slices, window path: two fresh handles give the same maps and statistics; asking for the contacts
    first leaves path_coverage()'s flags as a handle that never asked has them"""
    pts, cfg = synth.make_config("cfg2_1m_s256")
    kw = dict(tool_radius=cfg["tool_radius"], walk=1)
    e1 = engine_mod.Engine(0, **kw)
    e1.set_cloud(pts)
    S = e1.gen_path()
    assert S == 256 and e1.fast_path()
    c1, f1, l1, s1 = e1.path_contacts()
    check_stats(c1, f1, l1, s1)
    assert 0.05 * len(pts) < s1["covered"] < 0.999 * len(pts)
    assert s1["max_count"] >= 2 and s1["multi_slice"] > 0
    p1, pc1 = e1.path_coverage()
    e2 = engine_mod.Engine(0, **kw)
    e2.set_cloud(pts)
    assert e2.gen_path() == S
    p2, pc2 = e2.path_coverage()
    c2, f2, l2, s2 = e2.path_contacts()
    assert np.array_equal(c2, c1) and np.array_equal(f2, f1) and np.array_equal(l2, l1)
    assert {k: v for k, v in s2.items() if k != "hist"} == {k: v for k, v in s1.items() if k != "hist"}
    assert np.array_equal(s2["hist"], s1["hist"])
    assert pc1 == pc2 and np.array_equal(p1, p2)
    assert np.array_equal(c1 > 0, p1.astype(bool)) and s1["covered"] == pc1
    e1.close(); e2.close()


def _read_rgb_pcd(path):
    raw = open(path, "rb").read()
    k = raw.index(b"DATA binary\n") + len(b"DATA binary\n")
    hdr = raw[:k].decode()
    assert "FIELDS x y z rgb" in hdr and "SIZE 4 4 4 4" in hdr
    n = int([ln for ln in hdr.splitlines() if ln.startswith("POINTS")][0].split()[1])
    rec = np.frombuffer(raw[k:], dtype=np.dtype([("xyz", "<f4", 3), ("rgb", "<u4")]), count=n)
    return rec["xyz"].copy(), rec["rgb"].copy()


@pytest.mark.gpu
def test_connect_prints_the_path_contacts_and_paints_them(engine_mod, tmp_path):
    """PPP_PATH_CONTACTS=1 ./connect prints two lines with Engine.path_contacts()'s numbers; without the variable the output
    is what it was.  PPP_SHOW_CONTACTS=1 paints every cloud point of show()'s dump by its count on the fixed ramp, over
    PPP_SHOW_COVERAGE, and says so"""
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "examples"), "connect"])
    pts, _ = synth.make_config("small_40k")
    pcd = str(tmp_path / "workpiece.pcd")
    engine_mod.save_pcd(pcd, pts)
    conf = tmp_path / "config.txt"
    conf.write_text("Tool_Radius = 6\npathFile = %s\nPathResolution = 7\nRPYresolution = 7\nEnd effector length = 0.3\n"
                    "Smooth = false\nAlignment = false\nChangeRange = true\nRemoveOutlier = false\nDynamic_adjustment = false\n"
                    "Adjust_Threshold = 1\ntoolthickness = 10\ndepth = 0.01\n" % str(tmp_path / "wp.txt"))
    exe = os.path.join(ROOT, "examples", "connect")

    def run(**extra):
        env = {k: v for k, v in os.environ.items()
               if k not in ("PPP_PATH_COVERAGE", "PPP_PATH_CONTACTS", "PPP_SHOW_PCD", "PPP_SHOW_COVERAGE", "PPP_SHOW_CONTACTS")}
        env.update(PPP_CONFIG=str(conf), **extra)
        r = subprocess.run([exe, pcd], env=env, capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
        assert r.returncode == 0, r.stderr
        return r.stdout

    plain, with_con = run(), run(PPP_PATH_CONTACTS="1")
    lines = [ln for ln in with_con.splitlines() if ln.startswith("contacts: ") or ln.startswith("overlap: ")]
    assert len(lines) == 2, with_con
    assert not any(ln.startswith("contacts: ") or ln.startswith("overlap: ") for ln in plain.splitlines())
    strip = lambda out: [ln for ln in out.splitlines() if not ln.startswith("Toal Using Time") and ln not in lines]
    assert strip(plain) == strip(with_con)
    e = engine_mod.Engine(0, tool_radius=6.0, walk=1, dynamic_adjustment=0)
    cloud = engine_mod.load_pcd(pcd)[0]
    e.set_cloud(cloud)
    e.gen_path()
    counts, _, _, st = e.path_contacts()
    e.close()
    assert st["max_count"] >= 2 and st["multi_slice"] > 0
    mean = st["total"] / st["covered"]
    assert lines[0] == "contacts: max %u, mean %f over %d covered points" % (st["max_count"], mean, st["covered"])
    assert lines[1] == "overlap: %d points touched by two or more slices (%f of the cloud)" % (st["multi_slice"],
                                                                                                st["multi_slice"] / st["n"])
    dump = str(tmp_path / "show.pcd")
    out = run(PPP_SHOW_PCD=dump, PPP_SHOW_CONTACTS="1", PPP_SHOW_COVERAGE="1")
    assert "show(): PPP_SHOW_CONTACTS paints over PPP_SHOW_COVERAGE" in out
    _, rgb = _read_rgb_pcd(dump)
    crgb = rgb[len(rgb) - len(cloud):]                  # the inserted knots first, then the cloud in cloud order
    want = np.array([contact_rgb(int(c), st["max_count"]) for c in counts], np.uint32)
    assert np.array_equal(crgb, want), int((crgb != want).sum())
    assert len(np.unique(crgb)) > 3
