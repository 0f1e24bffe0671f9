"""[EXTENSION] X3 ego motion on the device: gv_grid_move resamples the three resident layers (log_odds, occupancy, the
packed int8 in OccupancyGrid.data order) by the whole-cell resample S its planner picks.  Every layer must equal a
numpy gather bit for bit -- the cell centre and source point in fp64 in include/gridvision_hip.h's operation order,
grid_map getIndex of the source, the constructor state (0.0, 0.5, 50) off the map -- using the cos / sin / tx / ty the
call reports.  Then the oracle end to end with moves between its updates, the ordering against pipelined frames and a
pending tick (the twin-handle pattern of test_gpu_tick.py), stable layer pointers, the residue reset and bad input.
Last, the scenes of tests/grid_move_cases.py (proved on the CPU by tests/test_grid_move_cases_host.py): grids that take
k_grid_move1, partial row blocks and k_copy_segments' byte tail, quarter turns whose every source lies on a cell border
so that get_index_fast's exact division decides, and planted layers -- log-odds distinct in every cell by bits, NaNs and
infinities among them -- on which any wrong source index shows."""
import numpy as np
import pytest

import grid_move_cases as gc
import grid_move_ref as R
import oracle_lib as ol
from grid_move_ref import np_move   # (tests/test_gpu_grid_skip.py imports it from here)
from gvamd import synth
from test_gpu_parity import _ground_scene, check_grid, make_handle

pytestmark = pytest.mark.gpu

GV_ERR_BAD_ARG = 1


@pytest.fixture(scope="module")
def gvamd():
    import gvamd as m
    m.load()
    return m


def _tf(yaw=0.0, tx=0.0, ty=0.0, tz=0.0):
    return np.array([0.0, 0.0, np.sin(0.5 * yaw), np.cos(0.5 * yaw), tx, ty, tz])


def _poses(h, res, n, seed):
    """n axis-aligned objects inside the handle's map (a few across the border)"""
    rng = np.random.default_rng(seed)
    lx, ly = h.nx * res, h.ny * res
    p = np.zeros(n, dtype=synth.LSHAPE_DTYPE)
    p["px"] = rng.uniform(h.pos_x - 0.55 * lx, h.pos_x + 0.55 * lx, n)
    p["py"] = rng.uniform(h.pos_y - 0.55 * ly, h.pos_y + 0.55 * ly, n)
    p["qw"] = 1.0
    p["length"] = rng.uniform(0.5, 0.1 * lx, n)
    p["width"] = rng.uniform(0.5, 0.1 * ly, n)
    p["height"] = 1.5
    return p


def _fill(h, res, seed, ticks=12):
    """non-trivial layers: objects of different ages (decayed, saturated, free) from update_map_poses"""
    for t in range(ticks):
        h.update_map_poses(_poses(h, res, 40, seed * 100 + t))


def _state(h):
    return h.log_odds(), h.occupancy(), h.to_occupancy_grid()[0]


def _same(a, b, tag):
    for k, (x, y) in enumerate(zip(a, b)):
        assert x.tobytes() == y.tobytes(), (tag, ("log_odds", "occupancy", "int8")[k])


def _geom(h, res):
    return h.nx, h.ny, res, h.pos_x, h.pos_y


# (grid_x, grid_y, res): the reference's own 50 x 20 m at 0.1 m (500 x 200 cells) and 2000 x 2000 cells
GRIDS = [(50, 20, 0.1), (200, 200, 0.1)]


@pytest.mark.parametrize("gx,gy,res", GRIDS)
def test_whole_cell_translations(gvamd, gx, gy, res):
    h = gvamd.GridVisionHIP(gx, gy, res)
    _fill(h, res, 1)
    st = _state(h)
    info = h.grid_move(_tf())   # identity: nothing enqueued, nothing changes
    assert not info["applied"] and info["cos_yaw"] == 1.0 and info["sin_yaw"] == 0.0 and info["tx"] == info["ty"] == 0.0
    _same(_state(h), st, "identity")
    lx, ly = h.nx * res, h.ny * res
    for k, (tx, ty) in enumerate([(3 * res, 0.0), (0.0, -7 * res), (-12 * res, 5 * res), (41 * res, 41 * res),
                                  (-0.5 * lx, 0.25 * ly), (lx + 2.0, 0.0), (0.0, -(ly + 0.3))]):
        info = h.grid_move(_tf(0.0, tx, ty, tz=0.7))
        assert info["applied"] and info["cos_yaw"] == 1.0 and info["sin_yaw"] == 0.0
        want = np_move(st, *_geom(h, res), info)
        st = _state(h)
        _same(st, want, (k, tx, ty))
        if abs(tx) > lx or abs(ty) > ly:   # off the map: every cell is the prior
            assert not st[0].any() and (st[1] == 0.5).all() and (st[2] == 50).all()
            _fill(h, res, 10 + k)
            st = _state(h)
        else:
            assert np.count_nonzero(st[0]) > 0
    h.close()


@pytest.mark.parametrize("gx,gy,res", GRIDS)
def test_rotation_and_translation(gvamd, gx, gy, res):
    h = gvamd.GridVisionHIP(gx, gy, res)
    for k, deg in enumerate([0.3, 3.0, 90.0, 180.0, -179.9]):
        h.reset()
        _fill(h, res, 20 + k)
        st = _state(h)
        info = h.grid_move(_tf(np.radians(deg), 1.37, -0.62))
        assert info["applied"] and info["sin_yaw"] != 0.0
        assert abs(np.arctan2(info["sin_yaw"], info["cos_yaw"]) - np.radians(deg)) < 1e-9
        assert info["res_yaw"] == 0.0 and max(abs(info["res_x"]), abs(info["res_y"])) <= 0.75 * res
        got, want = _state(h), np_move(st, *_geom(h, res), info)
        _same(got, want, deg)
        assert np.count_nonzero(got[0]) > 0
    h.close()


def test_sub_cell_steps_accumulate(gvamd):
    """3 cm per tick at 0.1 m: the first call moves nothing, later ones whole cells; the layers are the numpy chain"""
    h = gvamd.GridVisionHIP(50, 20, 0.1)
    _fill(h, 0.1, 3)
    st = _state(h)
    applied = []
    for i in range(30):
        info = h.grid_move(_tf(0.0, 0.03, 0.0))
        applied.append(info["applied"])
        if info["applied"]:
            st = np_move(st, *_geom(h, 0.1), info)
        else:
            assert info["tx"] == 0.0 and info["ty"] == 0.0
    assert applied[0] is False and sum(applied) >= 8
    _same(_state(h), st, "30 steps")
    h.close()


def test_oracle_with_moves_between_updates(gvamd):
    """K ticks of updateMap(poses) alternating with moves on the device; the oracle gets the numpy move written into
    its own log_odds / occupancy in between.  Log-odds bit-equal, the layers within check_grid's tolerances."""
    res = 0.1
    h = gvamd.GridVisionHIP(50, 20, res)
    og = ol.OGrid(50, 20, res)
    rng = np.random.default_rng(8)
    n_applied = 0
    for t in range(16):
        p = _poses(h, res, 30, 500 + t)
        h.update_map_poses(p)
        og.update_map_poses(p)
        info = h.grid_move(_tf(rng.normal(0.0, 0.02), rng.uniform(0.0, 1.2), rng.normal(0.0, 0.1)))
        if info["applied"]:
            n_applied += 1
            lo, occ, _ = np_move((og.log_odds.copy(), og.occupancy.copy(), np.zeros(og.G, np.int8)), *_geom(h, res), info)
            og.log_odds[:] = lo
            og.occupancy[:] = occ
        nlo, _, _ = check_grid(h, og)
        assert nlo == 0, t
    assert n_applied >= 10
    h.close()


def test_move_between_pipelined_frames(gvamd):
    """frame, move, frame, move, frame enqueued back to back == the same with a synchronize after every call"""
    hA, tfs = make_handle(gvamd, 2)
    hB, _ = make_handle(gvamd, 2)
    res = synth.CONFIGS[2]["grid"].resolution
    x, y, z, _ = synth.cloud_uniform(2)
    flags = gvamd.FRAME_BIN | gvamd.FRAME_RAYMARCH
    poses = _poses(hA, res, 20, 77)
    moves = [_tf(0.01, 0.9, 0.1), _tf(-0.004, 1.3, -0.2)]
    for h in (hA, hB):
        h.upload_xyz(x, y, z)
        h.set_detections(flags, poses=poses)
    for i in range(3):
        hA.enqueue_frame()
        hB.enqueue_frame()
        hB.synchronize()
        if i < 2:
            ia, ib = hA.grid_move(moves[i]), hB.grid_move(moves[i])
            assert ia == ib and ia["applied"]
            hB.synchronize()
    hA.synchronize()
    a, b = _state(hA), _state(hB)
    _same(a, b, "frames")
    hA.close(); hB.close()


def test_move_during_a_pending_tick(gvamd):
    """tick_enqueue(grid_out), move, tick_wait: grid_out holds the grid before the move, the layers after it equal the
    twin's grid after its own move"""
    hA, tfs = make_handle(gvamd, 2, perturbed=True)
    hB, _ = make_handle(gvamd, 2, perturbed=True)
    x, y, z, K, b = _ground_scene(tfs, seed=9)
    pinA, pinB = gvamd.PinnedI8(hA.G), gvamd.PinnedI8(hB.G)
    motion = _tf(np.radians(2.0), 2.3, -0.4)
    try:
        for h in (hA, hB):
            h.upload_xyz(x, y, z)
            h.tick(b, k_near=4)
        hA.tick_enqueue(b, k_near=4, grid_out=pinA.array)
        ia = hA.grid_move(motion)
        rA = hA.tick_wait()
        rB = hB.tick(b, k_near=4, grid_out=pinB.array)
        pre = _state(hB)
        ib = hB.grid_move(motion)
        assert ia == ib and ia["applied"]
        assert len(rA["poses"]) == len(rB["poses"]) >= 1
        assert pinA.array.tobytes() == pinB.array.tobytes() == pre[2].tobytes()
        post = _state(hA)
        _same(post, _state(hB), "after the move")
        _same(post, np_move(pre, *_geom(hB, synth.CONFIGS[2]["grid"].resolution), ib), "numpy")
    finally:
        pinA.close(); pinB.close()
    hA.close(); hB.close()


def test_pointers_residue_reset_and_bad_motion(gvamd):
    h = gvamd.GridVisionHIP(50, 20, 0.1)
    _fill(h, 0.1, 5)
    ptrs = h.device_layers()
    assert h.grid_move(_tf(0.2, 1.0, 0.0))["applied"]
    h.synchronize()
    assert h.device_layers() == ptrs
    info = h.grid_move(_tf(0.0, 0.03, 0.0))
    assert not info["applied"] and info["res_x"] == pytest.approx(0.03, abs=0.05)
    h.reset()
    info = h.grid_move(_tf(0.0, 0.03, 0.0))
    assert not info["applied"] and (info["res_yaw"], info["res_x"], info["res_y"]) == (0.0, 0.03, 0.0)
    h.set_log_odds(np.zeros(h.G, np.float32))
    info = h.grid_move(_tf(0.0, 0.03, 0.0))
    assert (info["res_yaw"], info["res_x"], info["res_y"]) == (0.0, 0.03, 0.0)
    before = _state(h)
    for bad in ([0, 0, 0, 1, np.nan, 0, 0], [0, 0, 0, 1, 0, 0, np.inf], [0, 0, 0, 0, 1.0, 0, 0], [np.inf, 0, 0, 1, 0, 0, 0]):
        with pytest.raises(gvamd.GVError) as e:
            h.grid_move(bad)
        assert e.value.code == GV_ERR_BAD_ARG
    info = h.grid_move(_tf(0.0, 0.03, 0.0))   # the rejected calls left the residue alone
    assert info["applied"] and info["tx"] == pytest.approx(0.1) and info["res_x"] == pytest.approx(-0.04)
    _same(_state(h), np_move(before, *_geom(h, 0.1), info), "after rejected calls")
    h.close()


# ------------------------------------------------------------------------ the scenes of tests/grid_move_cases.py --
@pytest.fixture(scope="module")
def handles(gvamd):
    """one handle per grid, made on first use; every scene plants all three layers anew"""
    cache = {}

    def get(name):
        if name not in cache:
            g = gc.GRID[name]
            cache[name] = h = gvamd.GridVisionHIP(*g.args)
            assert (h.nx, h.ny, h.G, h.pos_x, h.pos_y) == (g.nx, g.ny, g.nx * g.ny, g.pos_x, g.pos_y)
        return cache[name]
    yield get
    for h in cache.values():
        h.close()


def _check_move(h, res, before, info, tag):
    """all three layers by bytes against np_move of the readback; returns the state after the move"""
    geom = _geom(h, res)
    got, want = _state(h), np_move(before, *geom, info)
    assert not R.same(got, want), (tag, R.first_difference(got, want, h.nx, R.np_sources(*geom, info)[0]))
    return got


@pytest.mark.parametrize("key", gc.SCENES, ids="-".join)
def test_scene_equals_np_move_by_bytes(handles, key):
    g, m = gc.scene(key)
    res = g.args[2]
    h = handles(key[0])
    before = gc.plant(h, g)   # checked on the readback: distinct log-odds words, int8 and occupancy unlike any neighbour's
    info = h.grid_move(m.tf)
    assert info["applied"]
    got = _check_move(h, res, before, info, key)
    if m.cells:
        assert (info["cos_yaw"], info["sin_yaw"], info["tx"], info["ty"]) == (1.0, 0.0, res * m.cells[0], res * m.cells[1])
        assert not R.same(got, R.slice_move(before, h.nx, h.ny, *m.cells)), key
    if gc.is_border(key):   # with what this call reports, every in-map source is on a cell border on both axes
        sx, sy = R.np_sources(*_geom(h, res), info)[1:]
        inside, fx, _, fy, _ = R.fast_quotients(*_geom(h, res), sx, sy)
        assert inside.sum() >= 50 and (np.abs(fx - np.rint(fx))[inside] < 1e-6).all() and (np.abs(fy - np.rint(fy))[inside] < 1e-6).all()
    if m.name == "far_away":
        assert not got[0].any() and (got[1] == 0.5).all() and (got[2] == 50).all()


@pytest.mark.parametrize("name", ["25x10@0.2", "167x67@0.3"])
def test_four_quarter_turns_in_a_row(handles, name):
    g = gc.GRID[name]
    h = handles(name)
    st = gc.plant(h, g)
    for k in range(4):
        info = h.grid_move((0.0, 0.0, gc.Q[0], gc.Q[1], 0.0, 0.0, 0.0))
        assert info["applied"] and abs(info["sin_yaw"]) == 1.0
        st = _check_move(h, g.args[2], st, info, (name, k))
        assert np.isnan(st[0]).any() and np.isinf(st[0]).any(), k   # non-finite log-odds are still aboard


def test_layer_pointers_stay_on_an_odd_grid(handles):
    g = gc.GRID["167x67@0.3"]
    h = handles(g.name)
    assert h.G % 2 == 1
    before = gc.plant(h, g)
    ptrs = h.device_layers()
    for tf in ((0.0, 0.0, 0.0, 1.0, 2 * g.args[2], -g.args[2], 0.0), (0.0, 0.0, gc.Q[0], gc.Q[1], 0.0, 0.0, 0.0)):
        info = h.grid_move(tf)
        assert info["applied"]
        h.synchronize()
        assert h.device_layers() == ptrs
        before = _check_move(h, g.args[2], before, info, tf)
