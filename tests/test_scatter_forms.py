"""The forms of the window path's binning launch (k_win_scatter<PPT, STAGED, T>): which workgroup reserves which run inside a
window differs from form to form (and from run to run), the slice kernel orders every window on (class, y, cloud index), so every
form must give the default form's list bit for bit.

A form is forced by PPP_WIN_SCAT_T / PPP_WIN_PPT, which only the tuning build of the engine reads (libppp_hip_tune.so, made by
build()), once per plan: each form is a fresh child process (tests/helpers/scatter_forms_child.py) that plans all of its clouds
and leaves the results in a file; the children run side by side, once per session."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from polishpathplanning_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "helpers", "scatter_forms_child.py")
TOL_M = 1e-4      # BASELINE.json north_star, as tests/test_gpu_parity.py

# every instantiated (threads, points per thread) of the plain form; None: what the plan chooses by itself
FORMS = [(1024, 2), (1024, 4), (1024, 8), (512, 8), (512, 16), (256, 8), (256, 16)]
NARROWEST, FATTEST = (256, 8), (512, 16)            # by points of a workgroup: 2048 and 8192
EDGE = {NARROWEST: [1, 700, 2047, 2048, 2049, 4099], FATTEST: [1, 700, 8191, 8192, 8193, 16387]}


def _cases(form):
    cases = ["shapes"]
    if form is None:
        cases += ["edge" + "+".join(str(n) for n in sorted(set(EDGE[NARROWEST] + EDGE[FATTEST]))), "nan", "range", "piled"]
    if form in EDGE:
        cases.append("edge" + "+".join(str(n) for n in EDGE[form]))
    if form == NARROWEST:
        cases += ["nan", "range", "piled"]
    return ",".join(cases)


@pytest.fixture(scope="module")
def planned(tmp_path_factory):
    """{form: the arrays its child left, and under "log" what it printed (PPP_WIN_DEBUG: the plans, the batch records, the passes
    handed back)}; every child is started before any of them is waited for (8 processes on the device), and none outlives this"""
    d = tmp_path_factory.mktemp("scatter_forms")
    jobs = {}
    res = {}
    try:
        for form in [None] + FORMS:
            env = {k: v for k, v in os.environ.items() if k not in ("PPP_WIN_SCAT_T", "PPP_WIN_PPT")}
            env["PPP_WIN_DEBUG"] = "1"
            if form:
                env["PPP_WIN_SCAT_T"], env["PPP_WIN_PPT"] = str(form[0]), str(form[1])
            out = str(d / ("form_%s.npz" % ("default" if form is None else "%d_%d" % form)))
            jobs[form] = (out, subprocess.Popen([sys.executable, CHILD, out, _cases(form)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
        for form, (out, p) in jobs.items():
            log = p.communicate(timeout=300)[0]
            assert p.returncode == 0, (form, log[-3000:])
            res[form] = dict(np.load(out))
            res[form]["log"] = log
    finally:
        for _, p in jobs.values():
            if p.poll() is None:
                p.kill()
                p.communicate()
    return res


def _same(got, want, key, what=("SW", "wp", "counts", "bounds")):
    assert (key + ".error" in got) == (key + ".error" in want), key
    if key + ".error" in want:
        assert np.array_equal(got[key + ".error"], want[key + ".error"])
        return
    for w in what:
        assert np.array_equal(got[key + "." + w], want[key + "." + w]), (key, w)


@pytest.mark.parametrize("form", FORMS)
def test_every_form_gives_the_default_forms_list(planned, form):
    """tiny_5k (5 k points) and cfg1_50k_s32: waypoints() and waypoint_counts() of every instantiated form equal the default form's,
    and the handle really planned the forced form on the window path -- through the handle's own launches (k_win_scatter) and as a
    batch of one (k_win_scatter_b)."""
    got, want = planned[form], planned[None]
    for name in ("tiny_5k", "cfg1_50k_s32"):
        assert tuple(got[name + ".form"]) == (form[0], form[1], 1), (name, got[name + ".form"])
        assert tuple(want[name + ".form"])[2] == 1
        _same(got, want, name)
        assert got[name + ".wp"].tobytes() == want[name + ".wp"].tobytes()
        # the same pass as a batch of one (bench.py's entry point: the k_win_scatter_b kernels)
        assert got[name + ".wp_batch"].tobytes() == want[name + ".wp"].tobytes()
        assert np.array_equal(got[name + ".counts_batch"], want[name + ".counts"])
    # ... which launched this form: two batch records (one per cloud), each naming it (1024 threads: 4 points per thread at least)
    launched = re.findall(r"window batch: 1 members.* ppt (\d+) x (\d+) threads", got["log"])
    assert launched == [(str(max(form[1], 4) if form[0] == 1024 else form[1]), str(form[0]))] * 2, launched


@pytest.mark.parametrize("form", [NARROWEST, FATTEST])
def test_partial_last_workgroup_against_the_oracle(planned, oracle_mod, form):
    """Point counts around a workgroup's T x PPT points -- one point, one workgroup, T*PPT - 1, T*PPT, T*PPT + 1, and a last workgroup
    with three points -- for the narrowest and the fattest form: the default form's list bit for bit, and the oracle's list within
    the bar of tests/test_gpu_parity.py (a cloud the reference cannot plan ends in ERR_SLICE under every form)."""
    sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
    import scatter_forms_child as child
    got, want = planned[form], planned[None]
    windowed = 0
    for n in EDGE[form]:
        key = "edge%d" % n
        _same(got, want, key)
        pts = child.edge_cloud(n)
        o = oracle_mod.Oracle(pts, tool_radius=6.0)
        So = o.gen_path()
        if So < 0:      # a slice the reference cannot plan (one point: no spline): -(slice + 1) there, ERR_SLICE here, under any form
            assert tuple(got[key + ".error"]) == (-4,), key
            continue
        Wo = o.get_path()
        assert key + ".error" not in got, (key, got.get(key + ".error"))
        assert tuple(got[key + ".SW"]) == (So, Wo), key
        if Wo:
            assert np.linalg.norm(got[key + ".wp"][:, :3] - o.waypoints()[:, :3], axis=1).max() <= TOL_M, key
        if got[key + ".form"][2]:
            assert tuple(got[key + ".form"][:2]) == form
            windowed += 1
    assert windowed >= 4, "the counts around T*PPT must run the binning launch (window path)"


def test_nan_points_and_a_slice_range_through_a_narrow_form(planned):
    """A cloud with NaN points, and a slice-range handle (slice_begin / slice_end), through 256 threads x 8 points: bounds, counts
    and list (the range handle: its block of sampled waypoints and their nearest points) equal the default form's."""
    got, want = planned[NARROWEST], planned[None]
    assert tuple(got["nan.form"]) == NARROWEST + (1,)
    _same(got, want, "nan")
    assert tuple(got["range.form"]) == NARROWEST + (1,)
    _same(got, want, "range", what=("SW", "wp", "nn", "counts", "bounds"))


def test_window_overflow_under_a_narrow_form_hands_the_pass_back(planned, engine_mod):
    """The construction of test_plan_reuse_for_a_stream_of_clouds_of_one_size: a window that overflows the capacities its plan
    inherited (pos >= capw in the binning launch: the points beyond are not stored, the slice kernel sees count > capw and the pass
    is handed back -- the engine says so under PPP_WIN_DEBUG).  Under 256 x 8 the repeated pass gives the default form's list bit for
    bit.  Against the slab path: the same slices and waypoint counts; the list itself is NOT bit-equal between the two paths on any
    cloud (they add a normal's covariance sums in another order), so it is held to the bounds the suite already grants the two
    paths: positions within 1e-6 m (test_window_path_and_slab_path_agree), angles within 1e-4 rad modulo 2 pi (assert_full_parity)."""
    got, want = planned[NARROWEST], planned[None]
    assert tuple(got["piled.form0"]) == NARROWEST + (1,)
    # the overflow happened, under this form, on inherited capacities -- and only in the piled case (every other handle is fresh) ...
    for r in (got, want):
        back = re.findall(r"window pass handed back: flags (\d+) .*capacities were inherited", r["log"])
        assert len(back) == 1 and int(back[0]) & 1, back
    assert tuple(got["piled.form"]) == NARROWEST + (1,)     # ... and the cloud was planned again in the same form, on the window path
    _same(got, want, "piled", what=("SW", "wp", "counts"))
    sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
    import scatter_forms_child as child
    _, piled = child.piled_cloud()
    b = engine_mod.Engine(0, tool_radius=6.0, fast_path=False); b.set_cloud(piled)
    assert tuple(got["piled.SW"]) == (b.gen_path(), b.get_path())
    assert np.array_equal(got["piled.counts"], b.waypoint_counts())
    slab = b.waypoints()
    assert np.abs(got["piled.wp"][:, :3] - slab[:, :3]).max() <= 1e-6      # test_window_path_and_slab_path_agree's bound for the two paths
    da = np.abs(got["piled.wp"][:, 3:] - slab[:, 3:])
    assert np.minimum(da, np.abs(da - 2 * np.pi)).max() <= 1e-4            # assert_full_parity's TOL_RAD


@pytest.mark.parametrize("name", ["cfg1_50k_s32", "cfg2_1m_s256"])
def test_side_by_side_hint_changes_the_batch_launch_not_the_list(engine_mod, name):
    """ppp_run_batch_async of one workpiece into a caller's buffer (bench.py's step) with ppp_set_side_by_side 3, then 1, then 2,
    then 3 again: the list and the buffer's rows stay what a handle that was never told plans; every change of the hint across 2
    or 3 plans again (the batch graph goes with the plan's epoch).  The headline's cloud bins in the narrow form from THREE handles
    on (where it was measured to gain); with two handles, and after 3 -> 1, the handle reports the binning form of a pass alone; a
    small cloud keeps that form whatever it is told."""
    from polishpathplanning_amd.hipbuf import DeviceBuffer
    pts, cfg = synth.make_config(name)
    ref = engine_mod.Engine(0, tool_radius=cfg["tool_radius"]); ref.set_cloud(pts); ref.gen_path(); W = ref.get_path()
    want = ref.waypoints()
    alone = ref.binning_form()
    assert ref.fast_path() and alone[0] == 1024 and alone[1] in (4, 8)
    e = engine_mod.Engine(0, tool_radius=cfg["tool_radius"]); e.set_cloud(pts)
    buf = DeviceBuffer(W * 24)
    forms = []
    for hint in (3, 1, 2, 3):
        e.set_side_by_side(hint)
        forms.append(e.binning_form())
        for _ in range(3):                               # capture, then two replays of the batch graph
            engine_mod.run_batch_async([e], buf.ptr, [0], [W])
            engine_mod.sync_batch([e])
            assert buf.to_host(W * 6).reshape(-1, 6).tobytes() == want.tobytes()
        assert e.waypoints().tobytes() == want.tobytes() and np.array_equal(e.waypoint_counts(), ref.waypoint_counts())
        assert e.fast_path()
    assert forms[1] == alone                             # taken back: the launch of a pass alone
    assert forms[2] == alone                             # two handles: the parent's form (the narrow one loses there)
    assert forms[3] == forms[0]                          # three again: the plan's choice for three passes side by side
    if name == "cfg2_1m_s256":                           # the headline's cloud: large enough for the narrow form (cfg 1 keeps a pass's own)
        assert forms[0] == (512, 16)
    else:
        assert forms[0] == alone
