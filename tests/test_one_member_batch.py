"""ppp_run_batch_async with ONE window-path member: the member's own three launches with their arguments by value
(k_win_scatter / k_win_slice / k_win_finish) instead of the batched forms reading a one-entry record array.

The list must not depend on the launch form: byte-equal to the same cloud planned by ppp_run_async and as a member of
a batch of two (which keeps the batched forms), with the same place in the caller's buffer, the same hand-back to the
slab path, the same getters behind it.
"""
import numpy as np
import pytest

from polishpathplanning_amd import synth
from polishpathplanning_amd.hipbuf import DeviceBuffer

pytestmark = pytest.mark.gpu

SENTINEL = np.uint32(0xA5C3F00D)  # no waypoint row holds this bit pattern (a NaN with a payload)


def _filled(rows):
    buf = DeviceBuffer(rows * 24)
    buf.upload(np.full(rows * 6, SENTINEL, np.uint32))
    return buf


def _rows(buf, rows):
    return buf.to_host(rows * 6).view(np.uint32).reshape(rows, 6)


def _check_block(buf, rows, off, want):
    """rows [off, off + W) hold the list, every other row still holds the fill"""
    got = _rows(buf, rows)
    W = len(want)
    assert got[off:off + W].tobytes() == want.tobytes()
    assert (got[:off] == SENTINEL).all() and (got[off + W:] == SENTINEL).all()


@pytest.fixture(scope="module")
def plate(engine_mod):
    """cfg 1 (50 k points, 32 slices) and its list from ppp_run_async on a handle of its own"""
    pts, cfg = synth.make_config("cfg1_50k_s32")
    e = engine_mod.Engine(0, tool_radius=cfg["tool_radius"]); e.set_cloud(pts)
    assert e.fast_path()
    e.run_async(); e.sync()
    want = e.waypoints().copy()
    assert e.fast_path() and len(want) > 0       # nothing handed back
    want.setflags(write=False)
    return pts, cfg, want, e


def test_list_equals_run_async_and_the_member_of_a_batch_of_two(engine_mod, plate):
    pts, cfg, want, ref = plate
    W, off, cap = len(want), 5, len(want) + 7
    rows = off + cap + 3
    e = engine_mod.Engine(0, tool_radius=cfg["tool_radius"]); e.set_cloud(pts)
    assert e.fast_path()
    buf = _filled(rows)
    for _ in range(3):                            # capture, then two replays
        engine_mod.run_batch_async([e], buf.ptr, [off], [cap])
        engine_mod.sync_batch([e])
    _check_block(buf, rows, off, want)
    assert e.fast_path()
    # the getters behind a one-member pass: the list, the counts, the stage lists made on demand
    assert e.num_waypoints() == W and e.waypoints().tobytes() == want.tobytes()
    assert np.array_equal(e.waypoint_counts(), ref.waypoint_counts()) and np.array_equal(e.tail_index(), ref.tail_index())
    for st in (engine_mod.STAGE_WP_XYZ, engine_mod.STAGE_WP_NN, engine_mod.STAGE_WP_NORMAL, engine_mod.STAGE_WP_PRESMOOTH, engine_mod.STAGE_WP_SMOOTHED):
        assert e.stage(st).tobytes() == ref.stage(st).tobytes(), st
    # member 0 of a batch of two (the batched forms): beside a twin of itself, beside and behind a cloud of another seed
    other, _ = synth.make_config("cfg1_50k_s32", seed=11)
    for clouds, who in (((pts, pts), 0), ((pts, other), 0), ((other, pts), 1)):
        pair = []
        for c in clouds:
            m = engine_mod.Engine(0, tool_radius=cfg["tool_radius"]); m.set_cloud(c); pair.append(m)
        engine_mod.run_batch_async(pair); engine_mod.sync_batch(pair)
        ws = [m.num_waypoints() for m in pair]
        assert ws[who] == W
        offs = [3, 3 + ws[0] + 4]
        caps = [ws[0] + 2, ws[1] + 1]
        prow = offs[1] + caps[1] + 2
        pbuf = _filled(prow)
        engine_mod.run_batch_async(pair, pbuf.ptr, offs, caps); engine_mod.sync_batch(pair)
        got = _rows(pbuf, prow)
        assert got[offs[who]:offs[who] + W].tobytes() == want.tobytes()
        assert pair[who].waypoints().tobytes() == want.tobytes()
        assert all(m.fast_path() for m in pair)
        pbuf.free()
    buf.free()


def test_two_destinations_in_turn_and_a_plan_change_between(engine_mod, plate):
    pts, cfg, want, _ = plate
    W, off, cap = len(want), 2, len(want) + 1
    rows = off + cap + 1
    e = engine_mod.Engine(0, tool_radius=cfg["tool_radius"]); e.set_cloud(pts)
    bufs = [_filled(rows), _filled(rows)]
    for k in range(6):
        engine_mod.run_batch_async([e], bufs[k % 2].ptr, [off], [cap])
    engine_mod.sync_batch([e])
    for b in bufs:
        _check_block(b, rows, off, want)
    # a plan made again (another epoch) and the first one back: both destinations are written anew, by graphs captured anew
    for handles in (3, 1):
        e.set_side_by_side(handles)
        for b in bufs:
            b.upload(np.full(rows * 6, SENTINEL, np.uint32))
        for k in range(4):
            engine_mod.run_batch_async([e], bufs[k % 2].ptr, [off], [cap])
        engine_mod.sync_batch([e])
        for b in bufs:
            _check_block(b, rows, off, want)
        assert e.fast_path() and e.waypoints().tobytes() == want.tobytes()
    for b in bufs:
        b.free()


def test_a_pass_handed_back_lands_in_the_callers_rows(engine_mod):
    """A hole wider than the windows' reach (tests/test_gpu_parity.py, the hand-back case): the engine repeats the pass on the
    slab index by itself and the list -- in the handle and in the caller's rows -- is the slab path's."""
    pts, _ = synth.make_config("small_40k")
    x, y = pts[:, 0] * 1000.0, pts[:, 1] * 1000.0
    probe = engine_mod.Engine(0, tool_radius=6.0); probe.set_cloud(pts)
    px = probe.slice_positions()
    cx = float(px[len(px) // 2])
    holed = np.ascontiguousarray(pts[~((np.abs(x - cx) < 9.0) & (np.abs(y - 10.0) < 9.0))])
    b = engine_mod.Engine(0, tool_radius=6.0, fast_path=False); b.set_cloud(holed)
    b.gen_path(); b.get_path()
    want = b.waypoints()
    a = engine_mod.Engine(0, tool_radius=6.0); a.set_cloud(holed)
    assert a.fast_path()
    W, off, cap = len(want), 4, len(want) + 3
    rows = off + cap + 2
    buf = _filled(rows)
    engine_mod.run_batch_async([a], buf.ptr, [off], [cap])
    engine_mod.sync_batch([a])
    assert not a.fast_path()                      # handed back: this cloud stays on the slab index
    _check_block(buf, rows, off, want)
    assert a.waypoints().tobytes() == want.tobytes()
    engine_mod.run_batch_async([a], buf.ptr, [off], [cap])   # the next step: a batch of one on the slab path
    engine_mod.sync_batch([a])
    _check_block(buf, rows, off, want)
    buf.free()


def test_timed_pass_reports_the_by_value_launches(engine_mod, plate):
    pts, cfg, want, _ = plate
    W, off, cap = len(want), 1, len(want) + 2
    rows = off + cap + 1
    e = engine_mod.Engine(0, tool_radius=cfg["tool_radius"]); e.set_cloud(pts)
    assert e.fast_path()
    e.enable_timing(True)
    e.kernel_times()                              # (whatever was timed before the pass)
    buf = _filled(rows)
    engine_mod.run_batch_async([e], buf.ptr, [off], [cap])
    engine_mod.sync_batch([e])
    ms, launches = e.kernel_times(with_launches=True)
    assert launches == {"k_win_scatter": 1, "k_win_slice": 1, "k_win_finish": 1}, launches
    assert all(v > 0.0 for v in ms.values()), ms
    _check_block(buf, rows, off, want)
    assert e.waypoints().tobytes() == want.tobytes() and e.fast_path()
    e.enable_timing(False)
    engine_mod.run_batch_async([e], buf.ptr, [off], [cap])   # and back to the graph
    engine_mod.sync_batch([e])
    _check_block(buf, rows, off, want)
    buf.free()


def _outcome(engine_mod, e, run):
    try:
        run()
        return ("ok", e.num_slices(), e.num_waypoints(), e.waypoints().tobytes(), e.fast_path())
    except engine_mod.PPPError as ex:
        return ("error", ex.code)


@pytest.mark.parametrize("nx", [0, 14, 26, 40])
def test_degenerate_clouds_end_as_run_async_does(engine_mod, nx):
    """No point at all, too few slices for any to be kept (the first and the last are dropped), the first cloud with one kept
    slice, a few kept slices: a one-member batch ends exactly as ppp_run_async on a handle of its own -- whose launches this
    change leaves alone -- does: the same status code, or the same slices and list."""
    pts = synth.make_plate(nx, 30, kind="wavy", amp=3.0, seed=3) if nx else np.zeros((0, 3), np.float32)
    a = engine_mod.Engine(0, tool_radius=6.0); a.set_cloud(pts)
    b = engine_mod.Engine(0, tool_radius=6.0); b.set_cloud(pts)

    def one_member():
        for _ in range(2):                        # capture, replay
            engine_mod.run_batch_async([a]); engine_mod.sync_batch([a])

    def alone():
        for _ in range(2):
            b.run_async(); b.sync()

    assert _outcome(engine_mod, a, one_member) == _outcome(engine_mod, b, alone)
