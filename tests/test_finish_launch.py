"""The window path's finish launch (k_win_finish / k_win_finish_b) and the stage lists it no longer writes in every pass.

A pass enqueued call by call (gen_path / get_path) writes wp_pre and wp_smooth itself; a pass of a graph (run_async) or of a
batch leaves them to k_win_stage_lists, which runs when a getter asks.  So "plain calls" against "replay" compares the two
forms of the same text, window path against window path, with equality; the slab path's lists differ from the window path's in
the last bits of the normals' float sums and are compared at the tolerances of test_window_path_and_slab_path_agree.

The list lengths W the cases need were found with the CPU oracle (oracle.ppo.Oracle: its W is the engine's, smoke() asserts
that): tiny_5k gives W = 88 at the default path_resolution 7 and W = 173 at 3.5; small_40k cropped to y <= 0.0184 / 0.0185 /
0.01853 m gives W = 511 / 512 / 513 (a scan of the crop in steps of 1e-5 m).  Every case asserts the W it reached.
"""
import numpy as np
import pytest

from polishpathplanning_amd import synth

pytestmark = pytest.mark.gpu

TOL_SLAB = 1e-6  # window path against slab path, positions in metres (test_window_path_and_slab_path_agree)


@pytest.fixture(scope="module")
def clouds():
    tiny = synth.make_config("tiny_5k")[0]
    small = synth.make_config("small_40k")[0]
    crop = {W: np.ascontiguousarray(small[small[:, 1] <= np.float32(ymax)]) for W, ymax in ((511, 0.0184), (512, 0.0185), (513, 0.01853))}
    return {"tiny": tiny, "small": small, "crop": crop}


def _stages(e, em):
    return e.stage(em.STAGE_WP_PRESMOOTH), e.stage(em.STAGE_WP_SMOOTHED)


def _plain_against_replay(em, pts, W_want=None, slab=True, **kw):
    """One cloud and one set of parameters: a handle that goes call by call (the pass writes the lists), the slab path, a handle
    that has only ever replayed (its lists come from k_win_stage_lists, into buffers no pass wrote), and the first handle again
    after replays."""
    kw.setdefault("tool_radius", 6.0)
    a = em.Engine(0, **kw); a.set_cloud(pts)
    S = a.gen_path(); W = a.get_path()
    assert a.fast_path()
    if W_want is not None:
        assert W == W_want, W
    want = a.waypoints()
    pre, sm = _stages(a, em)
    assert pre.shape == (W, 6) and sm.shape == (W, 6)
    if slab:
        b = em.Engine(0, fast_path=False, **kw); b.set_cloud(pts)
        assert (S, W) == (b.gen_path(), b.get_path())
        bpre, bsm = _stages(b, em)
        assert np.abs(want[:, :3] - b.waypoints()[:, :3]).max() <= TOL_SLAB
        assert np.abs(pre[:, :3] - bpre[:, :3]).max() <= TOL_SLAB and np.abs(sm[:, :3] - bsm[:, :3]).max() <= TOL_SLAB
        assert np.array_equal(a.waypoint_counts(), b.waypoint_counts())
        b.close()
    # a handle that never went call by call
    c = em.Engine(0, **kw); c.set_cloud(pts)
    c.run_async(); c.sync()                      # the first pass of a plan is enqueued directly
    assert c.fast_path() and c.num_waypoints() == W
    assert c.waypoints().tobytes() == want.tobytes()
    csm = c.stage(em.STAGE_WP_SMOOTHED)          # (the smoothed list first: it must not lean on the other one having been asked for)
    assert np.array_equal(csm, sm, equal_nan=True)
    assert np.array_equal(c.stage(em.STAGE_WP_PRESMOOTH), pre, equal_nan=True)
    c.run_async(); c.sync(); c.run_async(); c.sync()   # captured, replayed; no getter in between
    assert c.waypoints().tobytes() == want.tobytes()
    for _ in range(2):                           # asked twice in a row
        p2, s2 = _stages(c, em)
        assert np.array_equal(p2, pre, equal_nan=True) and np.array_equal(s2, sm, equal_nan=True)
    c.close()
    # the first handle after replays of its own
    a.run_async(); a.sync(); a.run_async(); a.sync()
    assert a.waypoints().tobytes() == want.tobytes()
    p2, s2 = _stages(a, em)
    assert np.array_equal(p2, pre, equal_nan=True) and np.array_equal(s2, sm, equal_nan=True)
    assert a.fast_path()
    return a, want, pre, sm


@pytest.mark.parametrize("path_resolution,W_want", [(7.0, 88), (3.5, 173)])
def test_list_inside_one_tile(engine_mod, clouds, path_resolution, W_want):
    """Both end corrections fall into the one tile: W < 128 (every waypoint near both ends) and 128 <= W < 256."""
    a, *_ = _plain_against_replay(engine_mod, clouds["tiny"], W_want, path_resolution=path_resolution)
    a.close()


@pytest.mark.parametrize("W_want", [511, 512, 513])
def test_list_ends_at_a_tile_edge(engine_mod, clouds, W_want):
    """W = 256 k - 1, 256 k, 256 k + 1 with k = 2: the last tile full but for one, full, and a third tile of one waypoint."""
    a, *_ = _plain_against_replay(engine_mod, clouds["crop"][W_want], W_want)
    a.close()


@pytest.mark.parametrize("kw", [dict(smooth=0), dict(rpy_resolution=2.0), dict(rpy_resolution=3.0)])
def test_smooth_off_and_small_rpy_resolutions(engine_mod, clouds, kw):
    """No filter; no reduceRPY (rpy_resolution 2); the smallest interval reduceRPY works on (3)."""
    a, want, pre, sm = _plain_against_replay(engine_mod, clouds["small"], 891, **kw)
    if kw.get("smooth") == 0:
        assert np.array_equal(pre, sm)
    if kw.get("rpy_resolution") == 2.0:
        assert np.array_equal(want[:, 3:], sm[:, 3:])   # the angles pass through: no interval, no +-pi limit
    a.close()


def test_a_slice_shorter_than_the_rpy_interval_takes_the_in_order_finish(engine_mod, clouds):
    """tiny_5k has about seven waypoints per slice: rpy_resolution 9 makes every slice short (App. B.6), the last tile finishes the
    list in order, and that launch writes its stage lists whatever the pass was enqueued by."""
    a, want, pre, sm = _plain_against_replay(engine_mod, clouds["tiny"], 88, rpy_resolution=9.0)
    assert (a.waypoint_counts() <= 9).any()
    a.close()


def test_stage_lists_after_a_batch_with_a_destination(engine_mod, clouds):
    """run_batch_async with two window members and a destination buffer: the lists in the buffer and in the handles are the plain
    calls' lists, and so are the stage lists made afterwards -- also after a second replay with no getter in between."""
    from polishpathplanning_amd.hipbuf import DeviceBuffer
    em = engine_mod
    members, wants = [], []
    for pts in (clouds["small"], clouds["crop"][513]):
        ref = em.Engine(0, tool_radius=6.0); ref.set_cloud(pts); ref.gen_path(); ref.get_path()
        wants.append((ref.waypoints(), *_stages(ref, em)))
        ref.close()
        e = em.Engine(0, tool_radius=6.0); e.set_cloud(pts)
        members.append(e)
    Ws = [w[0].shape[0] for w in wants]
    assert Ws == [891, 513]
    dst = DeviceBuffer(sum(Ws) * 24)
    offsets, caps = [0, Ws[0]], Ws
    for replays in (1, 2):
        for _ in range(replays):
            em.run_batch_async(members, dst.ptr, offsets, caps)
        em.sync_batch(members)
        rows = dst.to_host(sum(Ws) * 6).reshape(-1, 6)
        for i, e in enumerate(members):
            assert e.fast_path()
            assert rows[offsets[i]:offsets[i] + Ws[i]].tobytes() == wants[i][0].tobytes()
            assert e.waypoints().tobytes() == wants[i][0].tobytes()
            sm = e.stage(em.STAGE_WP_SMOOTHED)
            assert np.array_equal(sm, wants[i][2]) and np.array_equal(e.stage(em.STAGE_WP_PRESMOOTH), wants[i][1])
    for e in members:
        e.close()


def test_slice_range_handles_still_leave_their_compact_list(engine_mod, clouds):
    """World 2 on tiny_5k: a slice-range handle's finish launch stops at the compact list and always writes it;
    copy_stage_to_device hands it on and finish_path_async finishes the gathered list -- identical to the list of the one handle,
    whose own compact list here comes from k_win_stage_lists."""
    from polishpathplanning_amd.hipbuf import DeviceBuffer
    from polishpathplanning_amd.robot_path import slice_ranges
    em, pts = engine_mod, clouds["tiny"]
    one = em.Engine(0, tool_radius=6.0); one.set_cloud(pts); one.run_async(); one.sync()
    W, S = one.num_waypoints(), one.num_slices()
    assert W == 88 and one.fast_path()
    gathered = DeviceBuffer(W * 24)
    engines, counts, off = [], None, 0
    for b, e in slice_ranges(S, 2):
        g = em.Engine(0, tool_radius=6.0, slice_begin=b, slice_end=e); g.set_cloud(pts)
        g.gen_path(); w = g.get_path()
        assert g.fast_path()
        assert g.copy_stage_to_device(em.STAGE_WP_PRESMOOTH, gathered.ptr + 24 * off, W - off) == w
        off += w
        c = g.waypoint_counts()
        counts = c if counts is None else counts + c
        engines.append(g)
    assert off == W and np.array_equal(counts, one.waypoint_counts())
    assert np.array_equal(gathered.to_host(W * 6).reshape(-1, 6), one.stage(em.STAGE_WP_PRESMOOTH))
    fin = engines[0]
    fin.finish_path_async(gathered.ptr, W, counts); fin.sync()
    assert fin.waypoints().tobytes() == one.waypoints().tobytes()
    assert np.array_equal(fin.stage(em.STAGE_WP_SMOOTHED), one.stage(em.STAGE_WP_SMOOTHED))
    assert np.array_equal(fin.stage(em.STAGE_WP_PRESMOOTH), one.stage(em.STAGE_WP_PRESMOOTH))


def test_a_pass_that_is_handed_back_leaves_early_and_runs_again(engine_mod, clouds):
    """A hole wider than the windows' reach (test_window_path_hands_a_pass_back_when_a_search_leaves_its_window): the finish launch
    finds the flag with its count loads in flight and leaves, the meta block reaches the host, and the pass runs again on the slab
    index: lists and stage lists are the slab path's, bit for bit."""
    em, pts = engine_mod, clouds["small"]
    x, y = pts[:, 0] * 1000.0, pts[:, 1] * 1000.0
    probe = em.Engine(0, tool_radius=6.0); probe.set_cloud(pts)
    px = probe.slice_positions()
    cx = float(px[len(px) // 2])
    holed = np.ascontiguousarray(pts[~((np.abs(x - cx) < 9.0) & (np.abs(y - 10.0) < 9.0))])
    b = em.Engine(0, tool_radius=6.0, fast_path=False); b.set_cloud(holed); b.gen_path(); W = b.get_path()
    bpre, bsm = _stages(b, em)
    for replay in (False, True):
        a = em.Engine(0, tool_radius=6.0); a.set_cloud(holed)
        assert a.fast_path()
        if replay:
            a.run_async(); a.sync()
        else:
            a.gen_path(); a.get_path()
        assert a.num_waypoints() == W
        assert a.waypoints().tobytes() == b.waypoints().tobytes()
        assert not a.fast_path()
        pre, sm = _stages(a, em)
        assert np.array_equal(pre, bpre) and np.array_equal(sm, bsm)
        a.close()
